"""Each request's full ranking on the CPU: rat_rank_seg through the host-emulation build (tests/emu), ops.rank_seg, and
OnlineScorer.rank_requests / rank_candidates on top of them.  The same checks, with the captured chains, run on the MI355X in
tests/test_gpu_online_rank.py; the corrupt-input check runs here only."""
import os
import sys

import pytest

import online_rank_cases as rc
from conftest import FULL_CPU, twin

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


def test_constants_are_the_kernels():
    assert rc.kernel_constants() == (256, 1024)


# one thread per row, no rounds: every set and every variant is cheap in the emulator; rat_topn_seg beside it costs n rounds, so the
# prefix is compared at one n per set here and at every n on the GPU
@pytest.mark.parametrize("set_name,ns", [("special", (5,)),("eighths", (32,)), ("distinct", (1,)), ("constant", (64,))])
def test_rank_seg_equals_numpy_stable_sort_emulated(emu_lib, set_name, ns):
    rc.check_rank_kernel("cpu", emu_lib, set_name, ns=ns)


def test_rank_seg_at_the_tile_and_across_work_groups_emulated(emu_lib):
    rc.check_rank_own("cpu", emu_lib, "tile", ns=(64,))


@pytest.mark.skipif(not FULL_CPU, reason="emulator repeat of a -m gpu test at another shape; RAT_CPU_FULL=1 runs it")
def test_rank_seg_4097_row_segment_emulated(emu_lib):
    rc.check_rank_own("cpu", emu_lib, "long", ns=(64,))


def test_corrupt_first_row_stays_inside_the_buffers_emulated(emu_lib):
    rc.check_corrupt(emu_lib)


def test_abi_refusals_emulated(emu_lib):
    rc.check_abi_refusals("cpu", emu_lib)


def test_ops_refusals_emulated(emu_lib):
    rc.check_ops_refusals("cpu", emu_lib)


# (every form's launch chain runs below; the ranking itself does not depend on the form)
@pytest.mark.parametrize("form", ["window", twin("immutable"), twin("capacity")])
def test_rank_requests_equal_numpy_over_score_requests_emulated(emu_lib, form):
    rc.check_rank_requests("tiny_seq_bn", -1, emu_lib, form, ns=(5,))


@pytest.mark.parametrize("form", ["window", twin("immutable"), twin("capacity")])
def test_rank_candidates_equal_rank_requests_over_host_rows_emulated(emu_lib, form):
    rc.check_rank_candidates("tiny_seq_bn", -1, emu_lib, form)


def test_rank_refusals_reach_no_entry_point_emulated(emu_lib):
    rc.check_refusals(-1, emu_lib)


@pytest.mark.parametrize("form", rc.rq.FORMS)
def test_rank_launch_chain_emulated(emu_lib, form):
    rc.check_launch_chain(-1, emu_lib, form)
