"""The one order of the request's endings (csrc/order_common.h: ``order_key``), checked across the three kernels that must agree on it:
``rat_topn_seg``, ``rat_rank_seg`` and ``rat_topn_merge``.  Shared by tests/test_order_contract.py (CPU, host-emulation build) and
tests/test_gpu_order_contract.py (MI355X).

One request of 64 rows, n = 64.  The documented key — fp32 -> uint32, ascending with the value, NaN -> 0 (below -inf), -0.0 -> the key
of +0.0, the largest key +inf's 0xFF800000 — is computed in numpy, and the expected order is numpy's stable sort on it, descending.
Everything is exact: positions equal, values bit for bit."""
import numpy as np
import torch

N = 64
SPLIT = 20


def values():
    """y fp32 [64]: NaNs of both signs and payloads, both zeros, both infinities, denormals of both signs, runs of equal values"""
    bits = np.zeros(N, dtype=np.uint32)
    special = [0x7fc00000, 0xffc00000, 0x7f800001,             # quiet NaN, negative NaN, a signalling payload
               0x00000000, 0x80000000, 0x80000000, 0x00000000,  # +0.0 and -0.0, interleaved: one run of four equal keys
               0x7f800000, 0xff800000, 0x7f800000,              # +inf twice, -inf
               0x00000001, 0x80000001, 0x007fffff, 0x807fffff,  # the smallest and the largest denormals
               0x00800000, 0x80800000,                          # the smallest normals
               0x7f7fffff, 0xff7fffff]                          # the largest finite values
    bits[:len(special)] = special
    rest = np.float32([0.5, 0.25, 0.5, -1.5, 0.5, 0.25, -1.5, 0.75]).view(np.uint32)       # runs of equal values, apart
    bits[len(special):] = np.resize(rest, N - len(special))
    bits[SPLIT - 1] = bits[SPLIT + 3] = np.float32(0.5).view(np.uint32)
    y = bits.view(np.float32).copy()
    y.setflags(write=False)
    return y


def documented_key(y):
    u = y.view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    u = np.where(u == 0x80000000, 0, u)
    key = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)
    return np.where(nan, 0, key).astype(np.int64)


def expected_order(y):
    return np.argsort(-documented_key(y), kind="stable")


def assert_inputs_reach_the_contract():
    y = values()
    key = documented_key(y)
    order = expected_order(y)
    assert np.isnan(y).sum() == 3 and (key[np.isnan(y)] == 0).all() and key[y == -np.inf][0] == 0x007fffff
    assert key.max() == 0xFF800000 and (key[y == np.inf] == 0xFF800000).all()
    zeros = np.nonzero(y == 0.0)[0]
    assert len(zeros) == 4 and len(set(key[zeros])) == 1 and np.signbit(y[zeros]).sum() == 2
    assert list(order[np.isin(order, zeros)]) == sorted(zeros)               # -0.0 and +0.0 tie: by position
    assert (np.isnan(y[order[-3:]])).all() and list(order[-3:]) == sorted(order[-3:])      # NaN after every number, by position
    # the documented order is numpy's stable descending sort of the values themselves
    assert np.array_equal(order, np.argsort(-y, kind="stable"))
    # a run of equal values straddles the split of the page
    assert y[order[SPLIT - 1]] == y[order[SPLIT]]


def check_one_order(device, lib):
    from rat_amd import ops
    y = values()
    want = expected_order(y)
    want_bits = y[want].view(np.int32)
    t_y = torch.from_numpy(y.copy()).to(device)
    first = torch.zeros(N, dtype=torch.int64, device=device)

    pos, val, lens = ops.topn_seg(t_y, first, N, lib=lib)
    order, oval, rank = ops.rank_seg(t_y, first, lib=lib)
    page_pos, page_val = pos[0].cpu().numpy(), val[0].cpu().numpy()
    assert int(lens[0]) == N
    assert np.array_equal(page_pos, order.cpu().numpy()), "rat_topn_seg and rat_rank_seg order differently"
    assert np.array_equal(page_pos, want), "the kernels' order is not the stable sort on the documented key"
    assert np.array_equal(page_val.view(np.int32), want_bits) and np.array_equal(oval.cpu().numpy().view(np.int32), want_bits)
    assert np.array_equal(rank.cpu().numpy()[want], np.arange(N))

    # the page cut at slot SPLIT: its head as the running page, its tail as a chunk's page (item = position: item0 = 0)
    run_item = torch.full((1, N), -1, dtype=torch.int32, device=device)
    run_val = torch.zeros((1, N), dtype=torch.float32, device=device)
    run_item[0, :SPLIT], run_val[0, :SPLIT] = pos[0, :SPLIT], val[0, :SPLIT]
    run_len = torch.tensor([SPLIT], dtype=torch.int32, device=device)
    c_pos = torch.full((1, N), -1, dtype=torch.int32, device=device)
    c_val = torch.zeros((1, N), dtype=torch.float32, device=device)
    c_pos[0, :N - SPLIT], c_val[0, :N - SPLIT] = pos[0, SPLIT:], val[0, SPLIT:]
    c_len = torch.tensor([N - SPLIT], dtype=torch.int32, device=device)
    heads = torch.zeros(1, dtype=torch.int64, device=device)
    ops.topn_merge(run_item, run_val, run_len, c_pos, c_val, c_len, heads, 0, lib=lib)
    assert int(run_len[0]) == N
    assert np.array_equal(run_item[0].cpu().numpy(), page_pos), "rat_topn_merge does not merge by the key rat_topn_seg ranked by"
    assert np.array_equal(run_val[0].cpu().numpy().view(np.int32), page_val.view(np.int32))
