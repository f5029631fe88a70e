"""Kernel-level parity of the prediction head (csrc/gemm.hip, csrc/head.hip) on the MI355X (-m gpu): the complete matrix of
tests/head_cases.py — the GEMM in the product's call forms on both arithmetics, the logit forward / backward through every entry
point, BatchNorm + the six activations on the two-launch and the column-strip kernels.  The emulator twin is
tests/test_head_kernels.py."""
import pytest
import torch

import head_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from rat_amd._lib import get_lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return get_lib()


@pytest.mark.parametrize("case", hc.GEMM_ALL, ids=hc.gemm_id)
def test_gemm_in_the_product_call_forms(lib, case):
    if (case.M, case.N, case.K) in hc.SPLITK_SHAPES:
        assert lib.size("rat_sgemm_workspace", case.M, case.N, case.K) > 0
    hc.check_gemm(lib, "cuda", case)


def test_gemm_entry_points_agree_on_a_split_k_shape(lib):
    hc.check_gemm_entry_points(lib, "cuda")


@pytest.mark.parametrize("case", hc.LOGIT_ALL, ids=hc.logit_id)
def test_logit_forward_and_backward_through_every_entry_point(lib, case):
    hc.check_logit_case(lib, "cuda", case)


def test_logit_saturated_logits_clamp_both_logs(lib):
    hc.check_logit_saturation(lib, "cuda")


@pytest.mark.parametrize("act", hc.ACTS)
@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("M,N", hc.BN_TWO_LAUNCH_CORE + hc.BN_TWO_LAUNCH_REST)
def test_bn_activation_two_launch_kernels(lib, M, N, use_bn, act):
    hc.check_bn_two_launch(lib, "cuda", M, N, use_bn, act)


@pytest.mark.parametrize("act", hc.ACTS)
@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("M,N", hc.BN_STRIP_CORE + hc.BN_STRIP_REST)
def test_bn_activation_column_strips(lib, M, N, use_bn, act):
    hc.check_bn_strips(lib, "cuda", M, N, use_bn, act)
