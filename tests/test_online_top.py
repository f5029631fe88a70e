"""Each request's top-n candidates on the CPU: rat_topn_seg and rat_candidates_expand through the host-emulation build (tests/emu),
ops.topn_seg / ops.candidates_expand, and OnlineScorer.top_requests / top_candidates / expand_candidates on top of them.  The same
checks, with the captured chains, run on the MI355X in tests/test_gpu_online_top.py; the corrupt-input check runs here only."""
import os
import sys

import pytest

import online_top_cases as tc
from conftest import twin

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


def test_inputs_reach_every_regime():
    tc.assert_regimes()


# the emulator runs one OS thread per GPU thread: the set with NaN, infinities and both zeros at every n, the other sets at the n
# whose cut falls on both sides of the short segments; the whole matrix runs on the GPU
@pytest.mark.parametrize("set_name,ns", [("special", tc.NS), ("eighths", (5,)), twin("eighths", (1, 32, 64)), twin("distinct", tc.NS),
                                         ("constant", (64,)), twin("constant", (1, 5, 32))])
def test_topn_seg_equals_numpy_stable_sort_emulated(emu_lib, set_name, ns):
    tc.check_topn_kernel("cpu", emu_lib, set_name, ns=ns)


def test_candidates_expand_equals_numpy_emulated(emu_lib):
    tc.check_expand_kernel("cpu", emu_lib)


def test_corrupt_first_row_and_cols_stay_inside_the_buffers_emulated(emu_lib):
    tc.check_corrupt(emu_lib)


def test_abi_refusals_emulated(emu_lib):
    tc.check_abi_refusals("cpu", emu_lib)


def test_ops_refusals_emulated(emu_lib):
    tc.check_ops_refusals("cpu", emu_lib)


# (every form's launch chain runs below; the ranking itself does not depend on the form)
@pytest.mark.parametrize("form", ["window", twin("immutable"), twin("capacity")])
def test_top_requests_equal_numpy_over_score_requests_emulated(emu_lib, form):
    tc.check_top_requests("tiny_seq_bn", -1, emu_lib, form, ns=(3,))


@pytest.mark.parametrize("form", ["window", twin("immutable"), twin("capacity")])
def test_top_candidates_equal_top_requests_over_host_rows_emulated(emu_lib, form):
    tc.check_top_candidates("tiny_seq_bn", -1, emu_lib, form, ns=(3,))


def test_top_refusals_reach_no_entry_point_emulated(emu_lib):
    tc.check_refusals(-1, emu_lib)


@pytest.mark.parametrize("form", tc.rq.FORMS)
def test_top_launch_chain_emulated(emu_lib, form):
    tc.check_launch_chain(-1, emu_lib, form)
