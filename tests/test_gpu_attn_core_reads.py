"""The VALU attention cores of the bf16x3 kernels (attn_fwd3_kernel / attn_fwd3_2wg_kernel's online-softmax loop, the two passes of
attn_bwd3_kernel) read their K / V / dO / Q rows from LDS as unpaired 8-byte reads (HeadVec::load_lds) and pass 2 fetches a query's
{lse, delta} pair in one read.  Only the load instructions change: the checks are those of the existing tests of the same kernels
(kernel_cases.py, same tolerances against the float64 oracle), at the lengths where the loops take another path:

    L  7       9 sequences per chunk
    L 11, 12   the probabilities of pass 1 handed to pass 2 (PH)
    L 13       PH off
    L 21       the intra-sample length of the north-star step
    L 32, 64   the VALU cores forced by the knobs (the host's rule runs the matrix-pipe cores there); at 64 one sequence fills a chunk

Every length with both sequence maps (intra and cross).  Every case: embedding_dim 64, 8 heads x 10, max_blocks 2 or 3 (every work-group loops over several chunks, the two-group forward too),
and a batch that leaves the last chunk short of sequences (except at L 64, where a chunk holds one).  Forward and backward, the plain
layer and the `ex` form with Dropout 0.25, O / lse saved and not.

On the MI355X (-m gpu) and, at smaller token grids and a subset of the lengths, through the host-emulation build of the same sources (which
compiles load_lds to the plain loads: there the twins check the {lse, delta} layout and the host side)."""
import os
import sys

import numpy as np
import pytest
import torch

import kernel_cases as kc
from rat_amd import ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

D, HEADS, DH = 64, 8, 10
# id: (B, T, S), map, max_blocks
EMU_CASES = {          # the host emulation runs the same loops a chunk at a time: one work-group (two in the forward) over five or six chunks
    "L7_intra": ((7, 7, 7), "intra", 1),         # 49 sequences, 9 per chunk: 6 chunks, the last one holds 4
    "L11_cross": ((3, 11, 7), "cross", 1),       # 21 sequences, 5 per chunk: 5 chunks, the last one holds 1
    "L11_intra": ((2, 11, 11), "intra", 1),      # 22 sequences: 5 chunks, the last one holds 2
    "L12_intra": ((11, 2, 12), "intra", 1),      # 22 sequences, 5 per chunk: 5 chunks, the last one holds 2
    "L13_cross": ((9, 13, 2), "cross", 1),       # 18 sequences, 4 per chunk: 5 chunks, the last one holds 2
    "L21_intra": ((13, 1, 21), "intra", 1),      # 13 sequences, 3 per chunk: 5 chunks, the last one holds 1
    "L21_cross": ((7, 21, 2), "cross", 1),       # 14 sequences: 5 chunks, the last one holds 2
    "L32_intra": ((9, 1, 32), "intra", 1),       # 9 sequences, 2 per chunk: 5 chunks, the last one holds 1
    "L64_cross": ((5, 64, 1), "cross", 1),       # 5 sequences, one per chunk
    "L7_cross": ((7, 7, 7), "cross", 1),         # 49 sequences: 6 chunks, the last one holds 4
    "L12_cross": ((11, 12, 2), "cross", 1),      # 22 sequences: 5 chunks, the last one holds 2
    "L13_intra": ((9, 2, 13), "intra", 1),       # 18 sequences: 5 chunks, the last one holds 2
    "L32_cross": ((9, 32, 1), "cross", 1),       # 9 sequences: 5 chunks, the last one holds 1
    "L64_intra": ((5, 1, 64), "intra", 1),       # 5 sequences, one per chunk
}
CASES = {
    "L7_intra": ((15, 5, 7), "intra", 2),        # 75 sequences, 9 per chunk: 9 chunks, the last one holds 3
    "L11_cross": ((6, 11, 7), "cross", 2),       # 42 sequences, 5 per chunk: 9 chunks, the last one holds 2
    "L11_intra": ((8, 7, 11), "intra", 3),       # 56 sequences: 12 chunks over 3 (forward: 6) work-groups, the last one holds 1
    "L12_intra": ((11, 4, 12), "intra", 2),      # 44 sequences, 5 per chunk: 9 chunks, the last one holds 4
    "L13_cross": ((17, 13, 2), "cross", 2),      # 34 sequences, 4 per chunk: 9 chunks, the last one holds 2
    "L21_intra": ((13, 2, 21), "intra", 2),      # 26 sequences, 3 per chunk: 9 chunks, the last one holds 2
    "L21_cross": ((17, 21, 2), "cross", 3),      # 34 sequences: 12 chunks over 3 (forward: 6) work-groups, the last one holds 1
    "L32_intra": ((17, 1, 32), "intra", 2),      # 17 sequences, 2 per chunk: 9 chunks, the last one holds 1
    "L64_cross": ((3, 64, 3), "cross", 2),       # 9 sequences, one per chunk
    "L7_cross": ((15, 7, 5), "cross", 2),        # 75 sequences: 9 chunks, the last one holds 3
    "L12_cross": ((14, 12, 4), "cross", 3),      # 56 sequences: 12 chunks over 3 (forward: 6) work-groups, the last one holds 1
    "L13_intra": ((17, 2, 13), "intra", 2),      # 34 sequences: 9 chunks, the last one holds 2
    "L32_cross": ((17, 32, 1), "cross", 2),      # 17 sequences: 9 chunks, the last one holds 1
    "L64_intra": ((4, 3, 64), "intra", 3),       # 12 sequences, one per chunk, over 3 (forward: 6) work-groups
}
IDS = sorted(CASES)


def setup(lib, knob, name, cases=None):
    (B, T, S), mode, max_blocks = (cases or CASES)[name]
    L = S if mode == "intra" else T
    nseq, per_chunk = (B * T if mode == "intra" else B * S), 64 // L
    assert (nseq + per_chunk - 1) // per_chunk >= 2 * (2 * max_blocks) and (per_chunk == 1 or nseq % per_chunk != 0)
    knob(lib, "max_blocks", max_blocks)
    if L >= 28:                                   # the host would run the matrix-pipe cores: keep the VALU loops
        knob(lib, "attn_bwd_core_mfma", 0)
        knob(lib, "attn_fwd_core_mfma", 3)
    return (B, T, S, D, HEADS, DH, True), mode


def check_plain(lib, dev, knob, name, cases=None):
    case, mode = setup(lib, knob, name, cases)
    kc.check_attn(lib, dev, case, mode, arith="bf16x3")


def check_ex(lib, dev, knob, name, cases=None):
    case, mode = setup(lib, knob, name, cases)
    kc.check_attn_dropout(lib, dev, case, mode, p=0.25, arith="bf16x3")
    kc.check_attn_ex(lib, dev, case, mode, "other", 0.5, 0.4, arith="bf16x3")


def check_unsaved(lib, dev, knob, name, cases=None):
    """O / lse not saved (the inference form): the same y, bit for bit, and nothing returned"""
    case, mode = setup(lib, knob, name, cases)
    B, T, S = case[:3]
    rs = np.random.RandomState(11)
    x, other = kc.rnd(rs, B, T, S, D).to(dev), kc.rnd(rs, B, T, S, D).to(dev)
    wd = [w.to(dev) for w in kc.attn_weights(rs, D, HEADS, DH, True)]          # (kept alive: the parameter block holds pointers)
    params = ops.attn_params(*wd)
    smap = ops.intra_map(B, T, S) if mode == "intra" else ops.cross_map(B, T, S)
    for form in ("plain", "ex"):
        out = {}
        for save in (True, False):
            if form == "plain":
                out[save] = ops.attn_fwd(x, params, smap, D, HEADS, DH, save=save, arith="bf16x3", lib=lib)
            else:
                out[save] = ops.attn_fwd_ex(x, other, params, smap, D, HEADS, DH, 0.4, 0.5, save=save, arith="bf16x3",
                                            dropout=(0.25, 987654321), lib=lib)
        assert out[False][1] is None and out[False][2] is None
        assert bool(torch.isfinite(out[True][0]).all()) and torch.equal(out[True][0], out[False][0]), form


def check_queries(lib, dev, knob, cases=None):
    """RatSeqMap.queries < L (the QSUB instantiations share the loops): three query positions of 21"""
    case, mode = setup(lib, knob, "L21_intra", cases)
    kc.check_attn_queries(lib, dev, case, mode, nq=3, arith="bf16x3")


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
@pytest.mark.parametrize("name", IDS)
def test_core_reads_plain(lib, knob, name):
    check_plain(lib, "cuda", knob, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_core_reads_ex_dropout(lib, knob, name):
    check_ex(lib, "cuda", knob, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_core_reads_unsaved(lib, knob, name):
    check_unsaved(lib, "cuda", knob, name)


@pytest.mark.gpu
def test_core_reads_query_subset(lib, knob):
    check_queries(lib, "cuda", knob)


# (an emulated launch costs seconds whatever its size: the plain twin — forward and backward — runs every length, the maps alternating;
#  the other twins a few of the remaining (length, map) pairs)
@pytest.mark.parametrize("name", ["L7_intra", "L11_cross", "L12_intra", "L13_cross", "L21_intra", "L32_cross", "L64_intra"])
def test_core_reads_plain_emulated(emu, knob, name):
    check_plain(emu, "cpu", knob, name, EMU_CASES)


@pytest.mark.parametrize("name", ["L11_intra", "L13_intra", "L21_cross"])
def test_core_reads_ex_dropout_emulated(emu, knob, name):
    check_ex(emu, "cpu", knob, name, EMU_CASES)


@pytest.mark.parametrize("name", ["L7_cross", "L12_cross", "L32_intra", "L64_cross"])
def test_core_reads_unsaved_emulated(emu, knob, name):
    check_unsaved(emu, "cpu", knob, name, EMU_CASES)


def test_core_reads_query_subset_emulated(emu, knob):
    check_queries(emu, "cpu", knob, EMU_CASES)
