"""Pass 2 of attn_bwd3_kernel steps a query's dO row, Q row and {lse, delta} pair (PH: delta and its P row) as LDS addresses that hold their
tile's base (RatLdsRow, one add per row and trip), and both passes decode a task with one division instead of two.  Only addresses and indices
change: the checks are those of the existing tests of the same kernels (kernel_cases.py, same tolerances against the float64
oracle), at the smallest shapes at which a stepped pointer can go wrong — every work-group loops over several chunks, the last chunk is
short of sequences, both sequence maps:

    L 21       the intra-sample length of the north-star step: 3 sequences per chunk, the interleaved {lse, delta} pair
    L 11       the cross-sample length: the probabilities of pass 1 handed to pass 2 (PH), delta and P read through their own pointers
    L 13       PH off, 4 sequences per chunk
    L  7       9 sequences per chunk
    queries    RatSeqMap.queries = 1 and L - 1 at L 21 and L 11 (the QSUB instantiations): one trip of pass 2's loop, and a trip count
               that differs from the number of keys
    d 40       embedding_dim 40 inside the 64-wide tiles (DPAD: plain loads through the same stepped rows, lse | delta as two arrays)
    ex         softmax scale, out_scale, a residual and an `add` term, with and without Dropout 0.25

Embedding_dim 64 (but d 40), 8 heads x 10, no dropout (but ex).  On the MI355X (-m gpu) and, at smaller token grids, through the host-emulation
build of the same sources (RatLdsRow is a plain pointer there: the twins check the stepping itself and the task decode)."""
import os
import sys

import pytest
import torch

import kernel_cases as kc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

HEADS, DH = 8, 10
# id: (B, T, S), map, max_blocks, embedding_dim
CASES = {
    "L21_intra": ((13, 2, 21), "intra", 2, 64),       # 26 sequences, 3 per chunk: 9 chunks, the last one holds 2
    "L21_cross": ((17, 21, 2), "cross", 3, 64),       # 34 sequences: 12 chunks over 3 work-groups, the last one holds 1
    "L11_cross": ((6, 11, 7), "cross", 2, 64),        # 42 sequences, 5 per chunk: 9 chunks, the last one holds 2
    "L11_intra": ((8, 7, 11), "intra", 3, 64),        # 56 sequences: 12 chunks over 3 work-groups, the last one holds 1
    "L13_cross": ((17, 13, 2), "cross", 2, 64),       # 34 sequences, 4 per chunk: 9 chunks, the last one holds 2
    "L7_intra": ((15, 5, 7), "intra", 2, 64),         # 75 sequences, 9 per chunk: 9 chunks, the last one holds 3
    "d40_L11_cross": ((6, 11, 7), "cross", 2, 40),    # DPAD with the hand-over of the probabilities
    "d40_L21_intra": ((13, 2, 21), "intra", 2, 40),   # DPAD without it
}
EMU_CASES = {          # the host emulation runs the same loops a chunk at a time: one work-group over five or six chunks
    "L21_intra": ((13, 1, 21), "intra", 1, 64),       # 13 sequences, 3 per chunk: 5 chunks, the last one holds 1
    "L21_cross": ((7, 21, 2), "cross", 1, 64),        # 14 sequences: 5 chunks, the last one holds 2
    "L11_cross": ((3, 11, 7), "cross", 1, 64),        # 21 sequences, 5 per chunk: 5 chunks, the last one holds 1
    "L11_intra": ((2, 11, 11), "intra", 1, 64),       # 22 sequences: 5 chunks, the last one holds 2
    "L13_cross": ((9, 13, 2), "cross", 1, 64),        # 18 sequences, 4 per chunk: 5 chunks, the last one holds 2
    "L7_intra": ((7, 7, 7), "intra", 1, 64),          # 49 sequences, 9 per chunk: 6 chunks, the last one holds 4
    "d40_L11_cross": ((3, 11, 7), "cross", 1, 40),
    "d40_L21_intra": ((13, 1, 21), "intra", 1, 40),
}
PLAIN = ["L21_intra", "L21_cross", "L11_cross", "L11_intra", "L13_cross", "L7_intra"]
QUERIES = [("L21_intra", 1), ("L21_cross", 20), ("L11_cross", 1), ("L11_intra", 10)]
DPAD = ["d40_L11_cross", "d40_L21_intra"]


def setup(lib, knob, name, cases):
    (B, T, S), mode, max_blocks, d = cases[name]
    L = S if mode == "intra" else T
    nseq, per_chunk = (B * T if mode == "intra" else B * S), 64 // L
    assert (nseq + per_chunk - 1) // per_chunk >= 4 * max_blocks and nseq % per_chunk != 0      # several chunks per work-group, a short last one
    knob(lib, "max_blocks", max_blocks)
    return (B, T, S, d, HEADS, DH, True), mode, L


def check_plain(lib, dev, knob, name, cases=CASES):
    case, mode, _ = setup(lib, knob, name, cases)
    kc.check_attn(lib, dev, case, mode, arith="bf16x3")


def check_queries(lib, dev, knob, name, nq, cases=CASES):
    case, mode, L = setup(lib, knob, name, cases)
    assert nq in (1, L - 1)
    kc.check_attn_queries(lib, dev, case, mode, nq=nq, arith="bf16x3")


def check_ex(lib, dev, knob, name, cases=CASES):
    case, mode, _ = setup(lib, knob, name, cases)
    kc.check_attn_dropout(lib, dev, case, mode, p=0.25, arith="bf16x3")
    kc.check_attn_ex(lib, dev, case, mode, "other", 0.5, 0.4, arith="bf16x3")


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
@pytest.mark.parametrize("name", PLAIN)
def test_bwd_addr_plain(lib, knob, name):
    check_plain(lib, "cuda", knob, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nq", QUERIES)
def test_bwd_addr_query_subset(lib, knob, name, nq):
    check_queries(lib, "cuda", knob, name, nq)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DPAD)
def test_bwd_addr_small_d(lib, knob, name):
    check_plain(lib, "cuda", knob, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L21_intra", "L11_cross"])
def test_bwd_addr_ex_dropout(lib, knob, name):
    check_ex(lib, "cuda", knob, name)


# (an emulated launch costs seconds whatever its size: one twin per path of pass 2's loop — the pair, the hand-over, the two arrays — and per
#  trip count; L 7 and the `ex` form at these grids are twins of test_gpu_attn_core_reads.py already)
@pytest.mark.parametrize("name", ["L21_intra", "L11_cross", "L13_cross"])
def test_bwd_addr_plain_emulated(emu, knob, name):
    check_plain(emu, "cpu", knob, name, EMU_CASES)


@pytest.mark.parametrize("name,nq", [("L21_cross", 20), ("L11_intra", 1)])
def test_bwd_addr_query_subset_emulated(emu, knob, name, nq):
    check_queries(emu, "cpu", knob, name, nq, EMU_CASES)


def test_bwd_addr_small_d_emulated(emu, knob):
    check_plain(emu, "cpu", knob, "d40_L11_cross", EMU_CASES)
