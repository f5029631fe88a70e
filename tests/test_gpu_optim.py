"""Kernel-level parity of the optimizer sweeps and the row-update kernels on the MI355X (-m gpu): the complete matrix of
tests/optim_cases.py, the shapes past the grid caps included.  The emulator twin is tests/test_optim_kernels.py."""
import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from rat_amd._lib import get_lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return get_lib()


@pytest.mark.parametrize("case", oc.FUSED_ADAM_CORE + oc.FUSED_ADAM_REPEATS + oc.FUSED_ADAM_GPU_ONLY, ids=oc.case_id)
def test_sumsq_reg_and_clip_adam_fused(lib, case):
    oc.check_fused_adam(lib, "cuda", *case)


@pytest.mark.parametrize("n", [(16 << 20) + 5, (16 << 20) + 20001])
def test_sumsq_reg_past_the_grid_rule_switch(lib, n):
    oc.check_sumsq_reg_large(lib, "cuda", n)


@pytest.mark.parametrize("kind", ["Adam", "SGD", "Adagrad", "RMSprop"])
@pytest.mark.parametrize("n,n_split", [(1027, 512), (20483, 4)])
def test_three_steps_from_zero_state_against_torch_optim(lib, kind, n, n_split):
    oc.check_fused_training_run(lib, "cuda", kind, n, n_split)


@pytest.mark.parametrize("kind", ["Adam", "RMSprop"])
def test_three_steps_from_zero_state_grid_striding(lib, kind):
    n = 4198307
    oc.check_fused_training_run(lib, "cuda", kind, n, (n // 8) * 4)


def test_clip_opt_fused_scales_lambda_from_device_memory(lib):
    oc.check_fused_training_run(lib, "cuda", "RMSprop", 1027, 513, steps=2, lam_scale=0.5)


@pytest.mark.parametrize("d", [1, 8, 10, 64])
@pytest.mark.parametrize("total_rows,max_rows,count", [(11, 7, 5), (300, 256, 200)])
def test_adam_rows_dev_and_sumsq_rows(lib, d, total_rows, max_rows, count):
    oc.check_adam_rows_dev(lib, "cuda", d, total_rows, max_rows, count)


def test_adam_rows_dev_grid_striding(lib):
    oc.check_adam_rows_dev(lib, "cuda", 64, 50000, 40000, 39999)


@pytest.mark.parametrize("d", [1, 8, 64])
def test_scatter_rows_lists(lib, d):
    oc.check_scatter_rows_lists(lib, "cuda", d)


@pytest.mark.parametrize("d", [8, 10, 40, 64])
@pytest.mark.parametrize("nbt", [1, 7, 300])
def test_label_grad(lib, nbt, d):
    oc.check_label_grad(lib, "cuda", nbt, 3, d)


def test_label_grad_at_the_north_star_row_count(lib):
    oc.check_label_grad(lib, "cuda", 45056, 3, 64)


@pytest.mark.parametrize("B,T", [(5, 4), (60000, 10)])
def test_check_ids_counts(lib, B, T):
    oc.check_check_ids(lib, "cuda", B, T)


@pytest.mark.parametrize("n,p", [(100003, 0.0), (100003, 0.3), (4198307, 0.3)])
def test_dropout_with_the_seed_in_device_memory(lib, n, p):
    oc.check_dropout_dev(lib, "cuda", n, p)
