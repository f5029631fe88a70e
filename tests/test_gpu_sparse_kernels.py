"""Kernel-level parity of the row-sparse plan and the segmented reduction on the MI355X (-m gpu): the complete matrix of
tests/sparse_kernel_cases.py — every reduce instantiation on real wave64 lanes, rocPRIM's radix sort at key widths on both sides of a
power of two and at 25 bits, and every launch_reduce branch past its cap of 8192 blocks — bit for bit against a sequential float32 numpy
reference.  The emulator twin is tests/test_sparse_kernels.py."""
import pytest
import torch

import sparse_kernel_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from rat_amd._lib import get_lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return get_lib()


@pytest.mark.parametrize("d,shape", [pytest.param(*c, id=kc.grid_id(c)) for c in kc.GRID_CORE + kc.GRID_TWIN])
def test_grid_reduce_every_instantiation_bit_for_bit(lib, d, shape):
    kc.check_grid(lib, "cuda", d, shapes=(shape,))


@pytest.mark.parametrize("d,which", kc.GRID_MISALIGNED_CORE)
def test_grid_reduce_unaligned_fallback_gives_the_aligned_bits(lib, d, which):
    kc.check_grid(lib, "cuda", d, misaligned=which)


@pytest.mark.parametrize("d", [8, 10])
def test_one_segment_of_14135_entries(lib, d):
    kc.check_long_segment(lib, "cuda", d)


@pytest.mark.parametrize("total_rows", kc.KEY_WIDTH_TOTALS_CORE)
def test_key_width_plan_from_ids(lib, total_rows):
    kc.check_key_width_grid(lib, "cuda", total_rows)


@pytest.mark.parametrize("total_rows", [31, 32, 33])
def test_key_width_plan_from_lists(lib, total_rows):
    kc.check_lists_key_width(lib, "cuda", total_rows)


def test_key_width_25_bits_on_a_width_1_table(lib):
    kc.check_scalar_key_width(lib, "cuda")


@pytest.mark.parametrize("name", kc.DEGENERATE_CORE)
def test_degenerate_plans_both_entry_points(lib, name):
    kc.check_degenerate(lib, "cuda", name)


@pytest.mark.parametrize("world,cap,d", kc.LISTS_CORE)
def test_gathered_lists_sum_in_rank_order(lib, world, cap, d):
    kc.check_lists_case(lib, "cuda", world, cap, d)


def test_gathered_lists_past_the_grid_cap(lib):
    kc.check_lists_past_the_cap(lib, "cuda")


@pytest.mark.parametrize("B", [9, 700])
def test_scalar_and_pooled_scalar_reduce(lib, B):
    kc.check_scalar_small(lib, "cuda", B)


@pytest.mark.parametrize("name", kc.PAST_THE_CAP_GPU_ONLY)
def test_grid_reduce_past_the_grid_cap(lib, name):
    kc.check_past_the_cap(lib, "cuda", name)


def test_scalar_and_pooled_scalar_reduce_past_the_grid_cap(lib):
    kc.check_scalar_past_the_cap(lib, "cuda")


@pytest.mark.parametrize("name", kc.WORKSPACE_SIZES_CORE + kc.WORKSPACE_SIZES_TWIN + kc.WORKSPACE_SIZES_GPU_ONLY)
def test_workspace_between_sentinels(lib, name):
    kc.check_degenerate(lib, "cuda", name)


def test_workspace_one_byte_short_is_refused(lib):
    kc.check_workspace_one_byte_short(lib, "cuda")


def test_refusals_launch_nothing(lib):
    kc.check_refusals(lib, "cuda")
