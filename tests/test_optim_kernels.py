"""Kernel-level parity of the optimizer sweeps and the row-update kernels on CPU: the kernel sources through the host emulation
(tests/emu) at the small shapes of tests/optim_cases.py.  The GPU twin, with the complete matrix, is tests/test_gpu_optim.py."""
import os
import sys

import pytest
from conftest import twin

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))

import optim_cases as oc  # noqa: E402
from rat_amd._lib import RatLib  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return RatLib(build_emu.build())


def test_the_fused_adam_matrix_has_every_axis_value_on_both_paths():
    """what the matrix promises, checked on the cases the emulator runs by default: every n with n_split strictly inside (where an
    inside exists), every offset set that keeps 16-byte alignment on both paths, the misaligned ones (scalar by definition), every
    n_split form, clip, lam_scale and zero_g value with the vector path and with the scalar path"""
    cases = oc.FUSED_ADAM_CORE
    assert len(set(cases)) == len(cases) and not (set(cases) & set(oc.FUSED_ADAM_REPEATS))

    def seen(pred):
        return {oc._path(c[1], c[2]) for c in cases if pred(c)}
    both = {"vector", "scalar"}
    for n in (1, 3, 4, 5, 1027, 4096, 4100, 24576, 24579, 20483):
        assert seen(lambda c: c[0] == n) == both, n
        if n > 1:
            assert any(c[0] == n and 0 < c[1] < n for c in cases), n
        if n > 4:
            assert "vector" in seen(lambda c: c[0] == n and 0 < c[1] < n), n
    for off in (oc.A0, oc.A4):
        assert seen(lambda c: c[2] == off) == both, off
    for off in (oc.M1, oc.MM, oc.MV):
        assert seen(lambda c: c[2] == off) == {"scalar"}, off
    for clip in (None, "off", "on"):
        assert seen(lambda c: c[3] == clip) == both, clip
    for lam_scale in (None, 0.5):
        assert seen(lambda c: c[4] == lam_scale) == both, lam_scale
    for zero_g in (True, False):
        assert seen(lambda c: c[5] == zero_g) == both, zero_g
    assert seen(lambda c: c[1] == 0) == both and seen(lambda c: c[1] == c[0]) == both
    assert seen(lambda c: c[1] == 4 and c[0] > 4) == {"vector"} and seen(lambda c: c[1] == (c[0] // 8) * 4 and c[0] > 8) == both
    assert seen(lambda c: c[1] % 4 == 1) == {"scalar"}
    big = oc.FUSED_ADAM_GPU_ONLY
    assert {c[0] for c in big} == {4198307} and {oc._path(c[1], c[2]) for c in big} == both


@pytest.mark.parametrize("case", oc.FUSED_ADAM_CORE + [twin(c) for c in oc.FUSED_ADAM_REPEATS], ids=oc.case_id)
def test_sumsq_reg_and_clip_adam_fused(emu, case):
    oc.check_fused_adam(emu, "cpu", *case)


@pytest.mark.parametrize("kind", ["Adam", "SGD", "Adagrad", "RMSprop"])
@pytest.mark.parametrize("n,n_split", [(1027, 512), (20483, 4)])
def test_three_steps_from_zero_state_against_torch_optim(emu, kind, n, n_split):
    oc.check_fused_training_run(emu, "cpu", kind, n, n_split)


def test_clip_opt_fused_scales_lambda_from_device_memory(emu):
    oc.check_fused_training_run(emu, "cpu", "RMSprop", 1027, 513, steps=2, lam_scale=0.5)


@pytest.mark.parametrize("d", [1, 8, 10, 64])
@pytest.mark.parametrize("total_rows,max_rows,count", [(11, 7, 5), (300, 256, 200)])
def test_adam_rows_dev_and_sumsq_rows(emu, d, total_rows, max_rows, count):
    oc.check_adam_rows_dev(emu, "cpu", d, total_rows, max_rows, count)


@pytest.mark.parametrize("d", [1, 8, 64])
def test_scatter_rows_lists(emu, d):
    oc.check_scatter_rows_lists(emu, "cpu", d)


# (a launch of rat_label_grad is 256 emulated work-groups whatever the shape — tens of seconds: the emulator keeps the two widths that
# do not divide the 256-thread group, one with fewer rows than work-groups and one with more)
@pytest.mark.parametrize("nbt,d", [(7, 10), (300, 40), twin(1, 8), twin(7, 8), twin(300, 8), twin(1, 10), twin(300, 10), twin(1, 40),
                                   twin(7, 40), twin(1, 64), twin(7, 64), twin(300, 64)])
def test_label_grad(emu, nbt, d):
    oc.check_label_grad(emu, "cpu", nbt, 3, d)


def test_check_ids_counts(emu):
    oc.check_check_ids(emu, "cpu", 5, 4)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_dropout_with_the_seed_in_device_memory(emu, p):
    oc.check_dropout_dev(emu, "cpu", 100003, p)
