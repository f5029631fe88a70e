"""The one order of rat_topn_seg, rat_rank_seg and rat_topn_merge (csrc/order_common.h) on the CPU, through the host-emulation build
(tests/emu).  The same check runs on the MI355X in tests/test_gpu_order_contract.py."""
import os
import sys

import pytest

import order_contract_cases as oc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    return L.RatLib(build_emu.build())


def test_inputs_reach_the_contract():
    oc.assert_inputs_reach_the_contract()


def test_topn_rank_and_merge_share_one_order_emulated(emu_lib):
    oc.check_one_order("cpu", emu_lib)
