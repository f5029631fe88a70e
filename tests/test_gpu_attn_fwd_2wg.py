"""attn_fwd3_2wg_kernel (69 KB of LDS, 128 VGPRs: two work-groups per CU) against attn_fwd3_kernel's one-group form, which the attn_fwd_2wg
knob forces, in one process: y, o_save and lse must be BITWISE equal — the two forms run the same per-element arithmetic in the same order
(K-step order of the GEMMs, softmax loop, split, Dropout indexing); only the LDS regions, the register budget and the grid differ.  (Both
forms against the float64 oracle: the bf16x3 cases of test_gpu_kernels.py / test_emu_kernels.py, which run whichever form the host picks.)

On the MI355X (-m gpu) and, at a smaller token grid, through the host-emulation build of the same sources."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import kernel_cases as kc
from rat_amd import ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

# plain: PreNorm(Attention)(x) + x -> the <false> instantiation; the others -> <true> (EX): a separate residual tensor ("add"), out_scale,
# Dropout behind the projection on and off; save: o_save / lse_save written or not
FORMS = [pytest.param("plain", 0.0, True, id="plain_save"), pytest.param("plain", 0.0, False, id="plain"),
         pytest.param("ex", 0.0, True, id="ex_add_scale_save"), pytest.param("ex", 0.0, False, id="ex_add_scale"),
         pytest.param("ex", 0.25, True, id="ex_dropout_save"), pytest.param("ex", 0.25, False, id="ex_dropout")]
MODES = [pytest.param("intra", id="L21"), pytest.param("cross", id="L11")]       # (B, 11, 21): intra-sample L = 21, cross-sample L = 11


def run_form(lib, x, other, params, smap, form, dropout_p, save):
    d, heads, dh = 64, 8, 10
    if form == "plain":
        return ops.attn_fwd(x, params, smap, d, heads, dh, save=save, arith="bf16x3", lib=lib)
    return ops.attn_fwd_ex(x, other, params, smap, d, heads, dh, 0.4, 0.5, save=save, arith="bf16x3", dropout=(dropout_p, 987654321), lib=lib)


def check_two_groups_bitwise(lib, dev, knob, B, max_blocks, mode, form, dropout_p, save):
    T, S, d, heads, dh = 11, 21, 64, 8, 10
    rs = np.random.RandomState(11)
    x, other = kc.rnd(rs, B, T, S, d).to(dev), kc.rnd(rs, B, T, S, d).to(dev)
    wd = [w.to(dev) for w in kc.attn_weights(rs, d, heads, dh, True)]
    params = ops.attn_params(*wd)
    smap = ops.intra_map(B, T, S) if mode == "intra" else ops.cross_map(B, T, S)
    L = S if mode == "intra" else T
    # the token grid: several chunks per work-group (max_blocks work-groups in the one-group form, twice as many in the other) and a last chunk
    # with fewer sequences than the others
    nseq, per_chunk = (B * T if mode == "intra" else B * S), 64 // L
    assert nseq % per_chunk != 0 and (nseq + per_chunk - 1) // per_chunk >= 2 * (2 * (max_blocks or 256))
    knob(lib, "max_blocks", max_blocks)
    launches = lib.cdll.rat_debug_attn_fwd_2wg_launches                # launches of attn_fwd3_2wg_kernel so far: tells which kernel a call ran
    launches.restype, launches.argtypes = ctypes.c_longlong, []
    out = {}
    for value in (1, 0):
        knob(lib, "attn_fwd_2wg", value)
        before = launches()
        out[value] = run_form(lib, x, other, params, smap, form, dropout_p, save)
        assert launches() - before == value, "knob %d: the %s-group kernel must have been the one launched" % (value, "two" if value else "one")
    for name, a_, b_ in zip(["y", "o_save", "lse"], out[1], out[0]):
        if name != "y" and not save:
            assert a_ is None and b_ is None
            continue
        assert bool(torch.isfinite(a_).all()), name
        assert torch.equal(a_, b_), ("two work-groups per CU vs one", name, float((a_ - b_).abs().max()))


@pytest.fixture(scope="module")
def lib():
    from rat_amd._lib import get_lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return get_lib()


@pytest.fixture(scope="module")
def emu():
    import build_emu
    from rat_amd._lib import RatLib
    return RatLib(build_emu.build())


@pytest.mark.gpu
@pytest.mark.parametrize("form,dropout_p,save", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_two_groups_bitwise_equal_to_one_group(lib, knob, mode, form, dropout_p, save):
    """3 / 6 work-groups: intra 1100 sequences = 367 chunks of 3 (the last one holds 2), cross 2121 sequences = 425 chunks of 5 (the last one holds 1)"""
    check_two_groups_bitwise(lib, "cuda", knob, 100 if mode == "intra" else 101, 3, mode, form, dropout_p, save)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_two_groups_bitwise_equal_at_the_full_grid(lib, knob, mode):
    """no max_blocks cap: 256 / 512 work-groups, every one with several chunks (B = 1024: 3755 / 4301 chunks)"""
    check_two_groups_bitwise(lib, "cuda", knob, 1024, 0, mode, "plain", 0.0, True)
    check_two_groups_bitwise(lib, "cuda", knob, 1024, 0, mode, "ex", 0.25, True)


@pytest.mark.parametrize("form,dropout_p,save", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_two_groups_bitwise_equal_to_one_group_emulated(emu, knob, mode, form, dropout_p, save):
    """the same comparison through the host emulation: 1 / 2 work-groups over 8 (intra: 22 sequences) / 9 (cross: 42 sequences) chunks"""
    check_two_groups_bitwise(emu, "cpu", knob, 2, 1, mode, form, dropout_p, save)
