"""Kernel-level parity of the prediction head (csrc/gemm.hip, csrc/head.hip) on CPU: the kernel sources through the host emulation
(tests/emu) on the smallest member of each class of tests/head_cases.py; RAT_CPU_FULL=1 runs the rest.  The GPU twin, with the
complete matrix, is tests/test_gpu_head_kernels.py."""
import os
import sys

import pytest
from conftest import twin

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))

import head_cases as hc  # noqa: E402
from rat_amd._lib import RatLib  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return RatLib(build_emu.build())


def test_the_gemm_cases_have_both_bf16x3_routes_for_every_transposition():
    """what the matrix promises: per (ta, tb) a shape the bf16x3 kernel takes and one the documented rule sends to exact fp32, among
    the cases the emulator runs by default as well; every condition of the rule as the ONLY reason of some case; every split-K shape
    with a ragged last k tile for every (ta, tb); the product forms; beta 0 / 0.5 / 1 with and without a bias on both routes"""
    names = [c.name for c in hc.GEMM_ALL]
    assert len(set(names)) == len(names) and len(set(hc.GEMM_ALL)) == len(hc.GEMM_ALL)
    for cases in (hc.GEMM_CORE, hc.GEMM_ALL):
        for ta, tb in hc.TT:
            kinds = {bool(hc.bf16x3_fallback_reasons(c)) for c in cases if (c.ta, c.tb) == (ta, tb)}
            assert kinds == {True, False}, (ta, tb)
        for route in (True, False):
            mine = [c for c in cases if bool(hc.bf16x3_fallback_reasons(c)) == route]
            assert {c.beta for c in mine} == {0.0, 0.5, 1.0} and {c.bias for c in mine} == {True, False}, route
            assert any(c.beta == 0.0 and not c.bias for c in mine) and any(c.beta == 0.0 and c.bias for c in mine), route
    sole = {next(iter(r)) for r in map(hc.bf16x3_fallback_reasons, hc.GEMM_ALL) if len(r) == 1}
    assert sole == {"lda", "ldb", "base A", "base B", "K", "M", "N"}, sole
    for shape in hc.SPLITK_SHAPES:
        assert shape[2] % 32 != 0
        assert {(c.ta, c.tb) for c in hc.GEMM_ALL if (c.M, c.N, c.K) == shape} == set(hc.TT), shape
        assert any((c.M, c.N, c.K) == shape for c in hc.GEMM_CORE), shape
    for d in (10, 40, 64):
        fwd, wg = (next(c for c in hc.GEMM_ALL if c.name == "product-%s-d%d" % (k, d)) for k in ("forward", "weight-gradient"))
        assert (fwd.ta, fwd.tb, wg.ta, wg.tb) == (0, 1, 1, 0)
        assert bool(hc.bf16x3_fallback_reasons(fwd)) == bool(hc.bf16x3_fallback_reasons(wg)) == (d == 10)


def test_the_logit_matrix_has_every_value_of_every_axis():
    for cases, Bs in ((hc.LOGIT_ALL, {1, 15, 16, 17, 33, 1000}), (hc.LOGIT_CORE, {1, 15, 16, 17, 33})):
        assert {c.B for c in cases} == Bs
        assert {c.d for c in cases} == {7, 10, 40, 64, 100, 200, 256}
        assert {c.nfields for c in cases} == {0, 3, 5, 16, 17, 37}
        for axis, values in (("head", {0, 1}), ("gscale", {1.0, 0.5}), ("gscale_dev", {None, hc.GDEV}), ("averaged", {False, True})):
            assert {getattr(c, axis) for c in cases} == values, axis
        assert {(c.d + c.pad) % 4 == 0 for c in cases} == {True, False}
        for averaged in (False, True):                       # both forward and both backward variants of either family
            assert {c.dnn for c in cases if c.averaged == averaged} >= {"out", hc.LAST52, hc.LAST7}, averaged
        assert any(c.clamp for c in cases)
        assert any(c.d % 4 == 0 and (c.d + c.pad) % 4 == 0 for c in cases) and any(c.d % 4 == 0 and (c.d + c.pad) % 4 for c in cases)


@pytest.mark.parametrize("case", hc.GEMM_CORE + [twin(c) for c in hc.GEMM_REST], ids=hc.gemm_id)
def test_gemm_in_the_product_call_forms(emu, case):
    if (case.M, case.N, case.K) in hc.SPLITK_SHAPES:
        assert emu.size("rat_sgemm_workspace", case.M, case.N, case.K) > 0
    hc.check_gemm(emu, "cpu", case)


def test_gemm_entry_points_agree_on_a_split_k_shape(emu):
    hc.check_gemm_entry_points(emu, "cpu")


@pytest.mark.parametrize("case", hc.LOGIT_CORE + [twin(c) for c in hc.LOGIT_REST], ids=hc.logit_id)
def test_logit_forward_and_backward_through_every_entry_point(emu, case):
    hc.check_logit_case(emu, "cpu", case)


def test_logit_saturated_logits_clamp_both_logs(emu):
    hc.check_logit_saturation(emu, "cpu")


def test_logit_backward_refuses_rows_above_its_block_size(emu):
    hc.check_logit_refusal(emu, "cpu")


@pytest.mark.parametrize("act", hc.ACTS)
@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("M,N", hc.BN_TWO_LAUNCH_CORE + [twin(*s) for s in hc.BN_TWO_LAUNCH_REST])
def test_bn_activation_two_launch_kernels(emu, M, N, use_bn, act):
    hc.check_bn_two_launch(emu, "cpu", M, N, use_bn, act)


@pytest.mark.parametrize("act", hc.ACTS)
@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("M,N", hc.BN_STRIP_CORE + [twin(*s) for s in hc.BN_STRIP_REST])
def test_bn_activation_column_strips(emu, M, N, use_bn, act):
    hc.check_bn_strips(emu, "cpu", M, N, use_bn, act)
