"""Kernel-level parity of the row-sparse plan and the segmented reduction on CPU: the kernel sources through the host emulation (tests/emu)
at the core shapes of tests/sparse_kernel_cases.py, every comparison bit for bit against a sequential float32 numpy reference.  The GPU
twin, with the cases past the grid caps and the 25-bit sort keys, is tests/test_gpu_sparse_kernels.py."""
import os
import sys

import pytest
from conftest import twin

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))

import sparse_kernel_cases as kc  # noqa: E402
from rat_amd._lib import RatLib  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return RatLib(build_emu.build())


@pytest.mark.parametrize("d,shape", [pytest.param(*c, id=kc.grid_id(c)) for c in kc.GRID_CORE]
                         + [twin(*c, id=kc.grid_id(c)) for c in kc.GRID_TWIN])
def test_grid_reduce_every_instantiation_bit_for_bit(emu, d, shape):
    kc.check_grid(emu, "cpu", d, shapes=(shape,))


@pytest.mark.parametrize("d,which", kc.GRID_MISALIGNED_CORE)
def test_grid_reduce_unaligned_fallback_gives_the_aligned_bits(emu, d, which):
    kc.check_grid(emu, "cpu", d, misaligned=which)


@pytest.mark.parametrize("d", [8, 10])
def test_one_segment_of_14135_entries(emu, d):
    kc.check_long_segment(emu, "cpu", d)


@pytest.mark.parametrize("total_rows", kc.KEY_WIDTH_TOTALS_CORE)
def test_key_width_plan_from_ids(emu, total_rows):
    kc.check_key_width_grid(emu, "cpu", total_rows)


@pytest.mark.parametrize("total_rows", [31, 32, 33])
def test_key_width_plan_from_lists(emu, total_rows):
    kc.check_lists_key_width(emu, "cpu", total_rows)


@pytest.mark.parametrize("name", kc.DEGENERATE_CORE)
def test_degenerate_plans_both_entry_points(emu, name):
    kc.check_degenerate(emu, "cpu", name)


@pytest.mark.parametrize("world,cap,d", kc.LISTS_CORE)
def test_gathered_lists_sum_in_rank_order(emu, world, cap, d):
    kc.check_lists_case(emu, "cpu", world, cap, d)


@pytest.mark.parametrize("B", [9, 700])
def test_scalar_and_pooled_scalar_reduce(emu, B):
    kc.check_scalar_small(emu, "cpu", B)


@pytest.mark.parametrize("name", kc.WORKSPACE_SIZES_CORE + [twin(n) for n in kc.WORKSPACE_SIZES_TWIN])
def test_workspace_between_sentinels(emu, name):
    kc.check_degenerate(emu, "cpu", name)


def test_workspace_one_byte_short_is_refused(emu):
    kc.check_workspace_one_byte_short(emu, "cpu")


def test_refusals_launch_nothing(emu):
    kc.check_refusals(emu, "cpu")
