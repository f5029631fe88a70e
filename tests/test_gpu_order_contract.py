"""The one order of rat_topn_seg, rat_rank_seg and rat_topn_merge (csrc/order_common.h) on the MI355X: one request of 64 rows holding
NaN, both zeros, both infinities, denormals and runs of equal values — the two kernels' orders equal each other and numpy's stable sort
on the documented key, and the page cut at slot 20 merges back into itself."""
import pytest

import order_contract_cases as oc

pytestmark = pytest.mark.gpu


def test_topn_rank_and_merge_share_one_order_gpu():
    import rat_amd._lib as L
    oc.check_one_order("cuda:0", L.get_lib())
