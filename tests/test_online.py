"""Online scoring on the CPU: the kernels of csrc/online.hip through the host-emulation build (tests/emu), the host API of
rat_amd/online.py on top of them.  The same checks (and the larger ones) run on the MI355X in tests/test_gpu_online.py."""
import os
import sys

import pytest

import online_cases as oc
import retrieval_cases as rc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


@pytest.mark.parametrize("name", list(rc.CASES))
def test_query_prepare_matches_host_mapping_emulated(name, emu_lib):
    oc.check_prepare(name, "cpu", emu_lib)


# the emulator runs one OS thread per GPU thread: two cases here (ties everywhere; topK > pool), all four on the GPU
@pytest.mark.parametrize("name", ["mltag_like", "tiny_pool"])
def test_split_topk_emulated(name, emu_lib):
    oc.check_split_case(name, "cpu", emu_lib)


def test_split_topk_ties_across_ranges_emulated(emu_lib):
    oc.check_split_ties("cpu", emu_lib)


def test_online_equals_offline_emulated(emu_lib):
    oc.check_online_vs_offline("tiny_seq_bn", -1, emu_lib, sizes=(7,), graph=False)


def test_refusals(emu_lib):
    oc.check_refusals(-1, emu_lib)
