"""Online scoring on the MI355X: query-side IDF mapping, the split top-K against the oracle and — bit for bit — against the single-range
kernel, and the whole request (retrieve -> assemble -> eval forward; eager and as a replayed hipGraph) against the offline pipeline."""
import pytest

import online_cases as oc
import retrieval_cases as rc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


@pytest.mark.parametrize("name", list(rc.CASES))
def test_query_prepare_matches_host_mapping_gpu(name):
    oc.check_prepare(name, "cuda:0", _lib())


@pytest.mark.parametrize("name", list(rc.CASES))
def test_split_topk_gpu(name):
    oc.check_split_case(name, "cuda:0", _lib())


def test_split_topk_ties_across_ranges_gpu():
    oc.check_split_ties("cuda:0", _lib())


@pytest.mark.parametrize("topk", [5, 12])
@pytest.mark.parametrize("n_qry", [1, 4, 5, 64])
def test_split_topk_large_pool_bitwise_gpu(n_qry, topk):
    oc.check_split_large_bitwise("cuda:0", _lib(), n_qry, topk)


# RAT_m2 and one variant; two request sizes; eager and replayed; a replay after a training step
@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_online_equals_offline_gpu(name):
    oc.check_online_vs_offline(name, 0, _lib(), sizes=(5, 17), graph=True, train_step=True)


def test_refusals_gpu():
    oc.check_refusals(0, _lib())
