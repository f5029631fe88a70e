"""Shared kernel-level checks of the half of csrc/sparse.hip that everything else consumes — the plan (rat_sparse_plan_ids,
rat_sparse_plan_rows, rat_sparse_workspace) and the segmented reduction (rat_sparse_reduce_grid, _rows, _scalar, _scalar_pool) — used
with the host-emulation build on CPU (tests/test_sparse_kernels.py) and the HIP build on the GPU (tests/test_gpu_sparse_kernels.py).
The optimizer and exchange half of that file is tests/optim_cases.py and tests/dp_cases.py; the model level is tests/sparse_cases.py.

The reference is numpy on the CPU and shares nothing with the kernels:
  key    of entry e = (row r of the batch, id column c): the field's first global row + the id clamped into [0, vocab - 1]; the entry is
         dropped when the clamped id is the field's padding id or no field reads the column; target_only: bt = r T.  Of a gathered list
         entry e = (rank, i): the row itself, dropped when i >= counts[rank] or the row is outside [0, total_rows)
  order  np.lexsort by (key, e)
  sum    float32 and STRICTLY sequential: acc = 0; acc = acc + v over the segment's entries in that order (np.sum is pairwise: not used);
         v = dgrid[bt, 1 + f] (+ dflat[bt / T, f] first, when bt % T == 0) | the gathered row | dlogit[b] | dlogit[b] / den[b, f]
Every assertion is bit-exact (floats as their 32-bit patterns): the unique-row count, the row list (strictly ascending), the sums, the dense
block (the scatter of those rows, the caller's fill everywhere else), and the sentinels behind the count in both lists, around every output,
around the count and around the workspace, which is always a view at a 256-byte-aligned offset between two sentinel runs.

Conditions on the INPUTS are asserted on the reference alone: the values are spread over six decades, so wherever a segment has three or
more entries the same reference summed in reversed order must differ in bits (otherwise the case could not see an unstable sort); every
case states the number of unique rows it needs and asserts that the reference reaches it.

Every comparison records its margin (tests/margins.py): the number of differing words."""
import functools

import numpy as np
import torch

from dp_cases import exact
from kernel_cases import F
from rat_amd import ops
from rat_amd._lib import RatError

F_SENT = 12345.0                      # behind the count in out_grads, and in every float guard
I_SENT = -7                           # behind the count in out_rows, and in every int guard
WS_SENT = 0xA5                        # the bytes around (and, before the plan runs, inside) the workspace
DENSE_FILL = 7.0                      # the dense block before the reduce (zeros in production: any fill must survive outside the rows)
GUARD = 8                             # sentinel words in front of and behind a buffer (32 bytes: 16-byte alignment is kept)
LOOP_MAX = 64                         # segments up to this length are summed rank by rank across segments, longer ones by np.cumsum


# ----------------------------------------------------------------------------- buffers
class Buf:
    """`n` words of `dtype` holding `fill` between two runs of sentinels on `dev`; shift = 1 puts the view one word off 16-byte alignment"""

    def __init__(self, n, dtype, fill, dev, shift=0):
        self.n, self.lo = int(n), GUARD + shift
        self.sent = F_SENT if dtype == torch.float32 else I_SENT
        self.buf = torch.full((self.lo + self.n + GUARD,), self.sent, dtype=dtype, device=dev)
        self.view = self.buf[self.lo:self.lo + self.n]
        if torch.is_tensor(fill) or isinstance(fill, np.ndarray):
            self.view.copy_(torch.as_tensor(fill).reshape(-1))
        else:
            self.view.fill_(fill)
        assert self.view.data_ptr() % 16 == 4 * shift

    def intact(self):
        return bool((self.buf[:self.lo] == self.sent).all()) and bool((self.buf[self.lo + self.n:] == self.sent).all())


class Plan:
    """what ops.SparsePlan holds (.ws, .count, .n), for the wrappers' plan= argument: rat_sparse_workspace(n) bytes (less `short`) as a view
    at a 256-byte-aligned offset between two sentinel runs, and the counter between guard words"""

    def __init__(self, n, dev, lib, short=0):
        self.n = int(n)
        self.bytes = lib.size("rat_sparse_workspace", self.n)
        self.raw = torch.full((512 + self.bytes + 256,), WS_SENT, dtype=torch.uint8, device=dev)
        self.off = 256 + (-self.raw.data_ptr()) % 256
        self.ws = self.raw[self.off:self.off + self.bytes - short]
        assert self.ws.data_ptr() % 256 == 0
        self.cnt = Buf(1, torch.int32, -5, dev)
        self.count = self.cnt.view

    def intact(self):
        return (bool((self.raw[:self.off] == WS_SENT).all()) and bool((self.raw[self.off + self.bytes:] == WS_SENT).all())
                and self.cnt.intact())


def spread(rs, *shape):
    """magnitudes over about six decades: fp32 sums of such values depend on the order of their terms"""
    return (rs.standard_normal(shape) * 10.0 ** rs.uniform(-3, 3, shape)).astype(np.float32)


# ----------------------------------------------------------------------------- the reference
def seq_sums(keys, vals, reverse=False):
    """keys: int64 [n], < 0 = dropped; vals: float32 [n][d] -> (rows int32 [U] ascending, sums float32 [U][d], longest segment).
    reverse: every segment summed from its last entry to its first (only to prove that the data can tell the order)"""
    n, d = vals.shape
    order = np.lexsort((np.arange(n), keys))
    order = order[keys[order] >= 0]
    k = keys[order]
    if k.size == 0:
        return np.zeros(0, np.int32), np.zeros((0, d), np.float32), 0
    head = np.concatenate([[True], k[1:] != k[:-1]])
    seg = np.cumsum(head) - 1
    start = np.flatnonzero(head)
    length = np.diff(np.concatenate([start, [k.size]]))
    rank = np.arange(k.size) - start[seg]
    if reverse:
        rank = length[seg] - 1 - rank
    v = vals[order]
    acc = np.zeros((start.size, d), np.float32)
    short = np.flatnonzero(length[seg] <= LOOP_MAX)
    by_rank = short[np.argsort(rank[short], kind="stable")]
    cnt = np.bincount(rank[short], minlength=1)
    end = np.cumsum(cnt)
    for j in range(cnt.size):                                    # the j-th entry of every segment that has one: no index twice
        sel = by_rank[end[j] - cnt[j]:end[j]]
        acc[seg[sel]] = acc[seg[sel]] + v[sel]
    for s in np.flatnonzero(length > LOOP_MAX):                  # np.add.accumulate is sequential along the axis, in float32
        rows = v[start[s]:start[s] + length[s]]
        rows = rows[::-1] if reverse else rows
        acc[s] = np.cumsum(np.concatenate([np.zeros((1, d), np.float32), rows]), axis=0, dtype=np.float32)[-1]
    return k[start].astype(np.int32), acc, int(length.max())


class Ref:
    """the reference of one reduce + the conditions the case puts on its inputs"""

    def __init__(self, keys, vals, total_rows, need_u=0, need_longest=0, order_matters=None):
        self.rows, self.sums, self.longest = seq_sums(keys, vals)
        self.U, self.d, self.total_rows, self.n = int(self.rows.size), int(vals.shape[1]), int(total_rows), int(keys.size)
        assert bool((self.rows[1:] > self.rows[:-1]).all()) and (self.U == 0 or (self.rows[0] >= 0 and self.rows[-1] < total_rows))
        assert self.U >= need_u, "the case needs %d unique rows, its reference has %d" % (need_u, self.U)
        assert self.longest >= need_longest, "the case needs a segment of %d entries, its longest has %d" % (need_longest, self.longest)
        if self.longest >= 3 if order_matters is None else order_matters:
            _, rev, _ = seq_sums(keys, vals, reverse=True)
            assert bool((rev.view(np.int32) != self.sums.view(np.int32)).any()), "these values cannot tell a reversed segment"

    def dense(self, fill=DENSE_FILL):
        want = np.full((self.total_rows, self.d), fill, dtype=np.float32)
        want[self.rows] = self.sums
        return want


def id_keys(idx, fields, target_only):
    """idx: int32 [B][T][L] -> (keys int64 [n], bt [n], field [n]) with entry e = r L + c"""
    B, T, L = idx.shape
    c2f = np.full(L, -1, dtype=np.int64)
    for i, f in enumerate(fields):
        c2f[f.col:f.col + f.ncols] = i
    first = np.concatenate([[0], np.cumsum([f.vocab for f in fields])]).astype(np.int64)
    vocab = np.array([fields[i].vocab if i >= 0 else 1 for i in c2f], dtype=np.int64)
    pad = np.array([(-1 if fields[i].padding_idx is None else fields[i].padding_idx) if i >= 0 else -1 for i in c2f], dtype=np.int64)
    base = np.array([first[i] if i >= 0 else 0 for i in c2f], dtype=np.int64)
    bt = np.arange(B, dtype=np.int64) * T if target_only else np.arange(B * T, dtype=np.int64)
    ids = np.clip(idx.reshape(B * T, L)[bt].astype(np.int64), 0, vocab - 1)
    keys = np.where((c2f >= 0) & (ids != pad), base + ids, -1)
    return keys.reshape(-1), np.repeat(bt, L), np.tile(c2f, bt.size)


def grid_values(dgrid, dflat, bt, fi, T):
    """dgrid: [B T][F + 1][d], dflat: [B][F][d] or None -> float32 [n][d] (zeros where no field reads the column)"""
    f = np.maximum(fi, 0)
    v = dgrid[bt, 1 + f]
    if dflat is not None:
        first = (bt % T) == 0
        v = np.where(first[:, None], v + dflat[bt // T, f], v)
    return np.where((fi >= 0)[:, None], v, np.float32(0)).astype(np.float32)


def row_keys(rows, counts, total_rows):
    """rows: int32 [world][cap] -> keys int64 [world cap]"""
    world, cap = rows.shape
    r = rows.astype(np.int64)
    ok = (np.arange(cap)[None, :] < np.asarray(counts)[:, None]) & (r >= 0) & (r < total_rows)
    return np.where(ok, r, -1).reshape(-1)


# ----------------------------------------------------------------------------- device side
def tables(fields, width, dev):
    first = np.concatenate([[0], np.cumsum([f.vocab for f in fields])]).astype(np.int64)
    flat = torch.zeros(int(first[-1]) * width, dtype=torch.float32, device=dev)
    tabs = [flat[int(first[i]) * width:int(first[i + 1]) * width].view(f.vocab, width) for i, f in enumerate(fields)]
    return flat, ops.field_table(fields, tabs, dev), int(first[-1])


class Outs:
    """the three outputs of a reduce, each between guards; which: 'lists' (out_rows + out_grads), 'dense', 'all'"""

    def __init__(self, which, ref, dev, shift_grads=0, shift_dense=0):
        self.cap = max(1, min(ref.n, ref.total_rows))
        lists, dense = which in ("lists", "all"), which in ("dense", "all")
        self.rows = Buf(self.cap, torch.int32, I_SENT, dev) if lists else None
        self.grads = Buf(self.cap * ref.d, torch.float32, F_SENT, dev, shift=shift_grads) if lists else None
        self.dense = Buf(ref.total_rows * ref.d, torch.float32, DENSE_FILL, dev, shift=shift_dense) if dense else None

    def args(self, d):
        return dict(out_rows=self.rows.view if self.rows else None, out_grads=self.grads.view.view(self.cap, d) if self.grads else None,
                    dense_base=self.dense.view if self.dense else None)


def compare(test, workload, where, ref, plan, outs, inputs=()):
    """U, rows, sums, dense block, the sentinels behind U and every guard"""
    U, d = ref.U, ref.d
    exact(test, workload, "U", plan.count, np.array([U], dtype=np.int32), where=where)
    if outs.rows is not None:
        got = outs.rows.view.cpu().numpy()
        assert bool((got[1:U] > got[:U - 1]).all()) if U > 1 else True, "%s %s: unique rows not strictly ascending (%s)" % (test, workload, where)
        exact(test, workload, "out_rows, sentinels behind U", got, np.concatenate([ref.rows, np.full(outs.cap - U, I_SENT, np.int32)]),
              where=where)
        exact(test, workload, "out_grads as bits, sentinels behind U", outs.grads.view.view(outs.cap, d),
              np.concatenate([ref.sums, np.full((outs.cap - U, d), F_SENT, np.float32)]), where=where)
    if outs.dense is not None:
        exact(test, workload, "dense block = scatter of the rows, untouched elsewhere", outs.dense.view.view(ref.total_rows, d), ref.dense(),
              where=where)
    for name, b in (("out_rows", outs.rows), ("out_grads", outs.grads), ("dense block", outs.dense)) + tuple(inputs):
        assert b is None or b.intact(), "%s %s: the guard words around %s were overwritten (%s)" % (test, workload, name, where)
    assert plan.intact(), "%s %s: the guard words around the workspace or the count were overwritten (%s)" % (test, workload, where)


# ----------------------------------------------------------------------------- 1. every reduce instantiation, grid source
# three fields as in sparse_cases.check_sorted_reduce plus a column no field reads: a single-id field, a bag field of three columns with a
# padding id, a single-id field with a padding id.  Field 0 also receives ids above its vocabulary and negative ids.
GRID_FIELDS = (F(0, 1, 7), F(2, 3, 6, padding_idx=5), F(5, 1, 9, padding_idx=8))
GRID_L = 6
GRID_COLS_HI = (7, 50, 6, 6, 6, 9)
GRID_SHAPES = ((5, 4), (37, 3))


@functools.lru_cache(maxsize=None)
def grid_inputs(d, B, T):
    rs = np.random.RandomState(81)
    idx = np.stack([rs.randint(0, GRID_COLS_HI[c], size=(B, T)) for c in range(GRID_L)], -1).astype(np.int32)
    idx[0, 0, 0], idx[1, 0, 0], idx[2, 1, 0], idx[3, 2, 0] = 99, -3, 10 ** 6, -1        # clamped to field 0's last / first row
    idx[4, 0, 5], idx[4, 1, 2] = 8, 5                                                   # padding ids in both padded fields
    return idx, spread(rs, B * T, 4, d), spread(rs, B, 3, d)


@functools.lru_cache(maxsize=None)
def grid_ref(d, B, T, target_only, with_dflat):
    idx, dgrid, dflat = grid_inputs(d, B, T)
    keys, bt, fi = id_keys(idx, GRID_FIELDS, target_only)
    total = sum(f.vocab for f in GRID_FIELDS)
    # (5, 4) target-only is 5 rows: 8 unique rows; everything else names 12 or more of the 20 rows that are no padding row
    ref = Ref(keys, grid_values(dgrid, dflat if with_dflat else None, bt, fi, T), total, need_u=8 if target_only and B == 5 else 12,
              need_longest=3)
    assert 0 in ref.rows and 6 in ref.rows, "the clamped ids land on field 0's first and last row"
    assert not ({7 + 5, 7 + 6 + 8} & set(ref.rows.tolist())), "padding rows never appear"
    return ref


def check_grid(lib, dev, d, shapes=GRID_SHAPES, misaligned=None):
    """misaligned: None, or which of 'dgrid', 'dflat', 'out_grads', 'dense_base' is a view one float off 16-byte alignment (then the
    scalar fall-back runs, and must give the bits of the aligned run: the reference is the same)"""
    test = "sparse_kernel_cases.check_grid"
    c2f = ops.col2field_table(GRID_FIELDS, GRID_L, dev)
    for B, T in shapes:
        idx, dgrid, dflat = grid_inputs(d, B, T)
        flat_d, ftab, total = tables(GRID_FIELDS, d, dev)
        idx_d = torch.from_numpy(idx).to(dev)
        dgrid_b = Buf(dgrid.size, torch.float32, dgrid, dev, shift=int(misaligned == "dgrid"))
        dflat_b = Buf(dflat.size, torch.float32, dflat, dev, shift=int(misaligned == "dflat"))
        for target_only in ((False, True) if d in (8, 10) and misaligned is None else (False,)):
            n = (B if target_only else B * T) * GRID_L
            plan = Plan(n, dev, lib)
            assert ops.sparse_plan_ids(idx_d, ftab, c2f, 3, flat_d, d, total, B, T, GRID_L, target_only=target_only, plan=plan, lib=lib) is plan
            for with_dflat in ((True,) if misaligned else (False, True)):
                ref = grid_ref(d, B, T, target_only, with_dflat)
                for which in (("all",) if misaligned else ("lists", "dense", "all")):
                    workload = "d=%d B=%d T=%d%s%s %s%s" % (d, B, T, " target_only" if target_only else "", " dflat" if with_dflat else "",
                                                             which, " misaligned " + misaligned if misaligned else "")
                    outs = Outs(which, ref, dev, shift_grads=int(misaligned == "out_grads"), shift_dense=int(misaligned == "dense_base"))
                    ops.sparse_reduce_grid(plan, dgrid_b.view, dflat_b.view if with_dflat else None, c2f, B, T, GRID_L, 3, d,
                                           target_only=target_only, lib=lib, **outs.args(d))
                    compare(test, workload, "", ref, plan, outs, inputs=(("dgrid", dgrid_b), ("dflat", dflat_b)))


GRID_WIDTHS = [4, 8, 16, 32, 64, 128, 256, 40, 100, 200, 10, 6]
# (width, (B, T)); the emulator launches one OS thread per GPU thread and a reduce launches n G / 256 blocks: the wide rows at the larger
# shape take it ten seconds each, so they run there only under RAT_CPU_FULL=1 (and always on the GPU)
GRID_CORE = [(d, s) for d in GRID_WIDTHS for s in GRID_SHAPES if d < 100 or s == GRID_SHAPES[0]]
GRID_TWIN = [(d, s) for d in GRID_WIDTHS for s in GRID_SHAPES if (d, s) not in GRID_CORE]
GRID_BRANCH = {4: "G1", 8: "G2", 16: "G4", 32: "G8", 64: "G16", 128: "G32", 256: "G64", 40: "G16-masked", 100: "G32-masked",
               200: "G64-masked", 10: "scalar", 6: "scalar"}
GRID_MISALIGNED_CORE = [(d, m) for d in (64, 40) for m in ("dgrid", "out_grads", "dense_base", "dflat")]


def grid_id(case):
    d, (B, T) = case
    return "d%d-%s-B%dT%d" % (d, GRID_BRANCH[d], B, T)


# ----------------------------------------------------------------------------- 2. bag-field cases: long segments, key widths, grid caps
def check_bag(lib, dev, name, d, B, T, L, fields, idx, seed, need_u=0, need_longest=0, which=("all",), with_dflat=True):
    """idx: int32 [B][T][L] over `fields`; full plan + grid reduce at width d"""
    test = "sparse_kernel_cases.check_bag"
    rs = np.random.RandomState(seed)
    nf = len(fields)
    dgrid = spread(rs, B * T, nf + 1, d)
    dflat = spread(rs, B, nf, d) if with_dflat else None
    keys, bt, fi = id_keys(idx, fields, False)
    flat_d, ftab, total = tables(fields, d, dev)
    ref = Ref(keys, grid_values(dgrid, dflat, bt, fi, T), total, need_u=need_u, need_longest=need_longest)
    c2f = ops.col2field_table(fields, L, dev)
    plan = Plan(B * T * L, dev, lib)
    ops.sparse_plan_ids(torch.from_numpy(idx).to(dev), ftab, c2f, nf, flat_d, d, total, B, T, L, plan=plan, lib=lib)
    dgrid_d = torch.from_numpy(dgrid).to(dev)
    dflat_d = torch.from_numpy(dflat).to(dev) if with_dflat else None
    for w in which:
        outs = Outs(w, ref, dev)
        ops.sparse_reduce_grid(plan, dgrid_d, dflat_d, c2f, B, T, L, nf, d, lib=lib, **outs.args(d))
        compare(test, "%s d=%d n=%d total_rows=%d %s" % (name, d, B * T * L, total, w), "U = %d, longest segment %d" % (ref.U, ref.longest),
                ref, plan, outs)
    return ref


def check_long_segment(lib, dev, d):
    """one row named by every entry: n = 14 135 in one segment (one lane group walks all of it)"""
    B, T, L = 257, 11, 5
    ref = check_bag(lib, dev, "long-segment", d, B, T, L, [F(0, L, 1)], np.zeros((B, T, L), np.int32), 82, need_u=1,
                    need_longest=B * T * L)
    assert ref.U == 1


def key_width_ids(total_rows, B, T, seed):
    """two fields over L = 4 columns (column 3 unread): rows 0 and total_rows - 1 are named, padding ids are present"""
    fields = [F(0, 2, total_rows - 3, padding_idx=1), F(2, 1, 3)]
    rs = np.random.RandomState(seed)
    idx = np.stack([rs.randint(0, hi, size=(B, T)) for hi in (total_rows - 3, total_rows - 3, 3, 9)], -1).astype(np.int32)
    idx[0, 0, 0], idx[0, 0, 1], idx[0, 0, 2], idx[1, 0, 2] = 0, 1, 2, 2
    idx[B - 1, T - 1, 1], idx[B - 1, T - 1, 2], idx[B - 1, 0, 0] = total_rows - 4, 2, 1
    return fields, idx


def check_key_width_grid(lib, dev, total_rows, T=3):
    """the sort key must hold total_rows ITSELF (the invalid key): one bit more than the largest valid row at a power of two"""
    B = 9 if total_rows < 1000 else 300                          # n = 108 and 3600
    fields, idx = key_width_ids(total_rows, B, T, 83)
    ref = check_bag(lib, dev, "key-width", 8, B, T, 4, fields, idx, 84, need_u=min(total_rows, B * T) // 2, need_longest=2)
    assert ref.rows[0] == 0 and ref.rows[-1] == total_rows - 1 and ref.n > int((id_keys(idx, fields, False)[0] >= 0).sum())


KEY_WIDTH_TOTALS_CORE = [31, 32, 33, 4095, 4096, 4097]


def permuted_ids(rs, shape, vocab, n_dup):
    """ids from a permutation of the vocabulary, then n_dup of them overwritten with ids of a pool of n_dup / 4 others: segments of
    about five entries, none longer than LOOP_MAX"""
    n = int(np.prod(shape))
    ids = rs.permutation(vocab)[:n].astype(np.int32)
    where = rs.choice(n, size=n_dup + n_dup // 4, replace=False)
    ids[where[:n_dup]] = ids[where[n_dup:]][rs.randint(0, n_dup // 4, size=n_dup)]
    return ids.reshape(shape)


def check_past_the_cap(lib, dev, name):
    """every launch_reduce branch caps its grid at 8192 blocks and strides: these pass the cap of the branch they name"""
    rs = np.random.RandomState(85)
    if name == "G64-d256":                                       # four segments per block x 8192
        B, T, L, d, need = 512, 8, 10, 256, 32768
        fields = [F(c, 1, 6000) for c in range(L)]
        idx = np.stack([permuted_ids(rs, (B, T), 6000, 300) for _ in range(L)], -1)
    elif name == "G16-d64":                                      # sixteen segments per block x 8192; one bag field over all columns
        B, T, L, d, need = 2048, 8, 10, 64, 131072
        fields = [F(0, L, 400000)]
        idx = permuted_ids(rs, (B, T, L), 400000, 4000)
    elif name == "scalar-d10":                                   # U d past 8192 x 256 items
        B, T, L, d, need = 2048, 11, 10, 10, 209716
        fields = [F(c, 1, 30000) for c in range(L)]
        idx = np.stack([permuted_ids(rs, (B, T), 30000, 800) for _ in range(L)], -1)
    elif name in NARROW_PAST_THE_CAP:                            # 256 / G segments per block x 8192; one bag field over all columns
        d, rows, need = NARROW_PAST_THE_CAP[name]
        B, T, L = rows // 8, 8, 10
        fields = [F(0, L, rows * L * 4 // 3)]
        idx = permuted_ids(rs, (B, T, L), fields[0].vocab, 4000)
    else:
        raise KeyError(name)
    ref = check_bag(lib, dev, "past-the-cap " + name, d, B, T, L, fields, np.ascontiguousarray(idx, dtype=np.int32), 86, need_u=need + 1,
                    need_longest=3)
    assert ref.longest <= LOOP_MAX
    return ref


NARROW_PAST_THE_CAP = {"G8-d32": (32, 30000, 262144), "G4-d16": (16, 60000, 524288), "G2-d8": (8, 120000, 1048576),
                       "G1-d4": (4, 240000, 2097152)}              # name: (d, B T, unique rows to exceed)
PAST_THE_CAP_GPU_ONLY = ["G64-d256", "G16-d64", "scalar-d10"] + list(NARROW_PAST_THE_CAP)


# ----------------------------------------------------------------------------- 3. scalar forms (target-only plan over width-1 tables)
def check_scalar(lib, dev, name, B, T, L, fields, idx, seed, need_u=0, need_longest=0, den_free_field=None, which=("lists", "dense", "all")):
    """rat_sparse_reduce_scalar against the sequential fp32 sum of dlogit[b]; rat_sparse_reduce_scalar_pool against that of
    dlogit[b] / den[b][f] (numpy's float32 division is correctly rounded, and so is the device's under -ffp-contract=off without
    fast-math: identical bits are demanded), den from {1, 2, 3, 7} and 1 everywhere for `den_free_field`; and the pool entry point with
    lr_den = NULL against the plain form"""
    test = "sparse_kernel_cases.check_scalar"
    rs = np.random.RandomState(seed)
    nf = len(fields)
    dlogit = spread(rs, B, 1)
    den = rs.choice(np.array([1, 2, 3, 7], np.float32), size=(B, nf)).astype(np.float32)
    if den_free_field is not None:
        den[:, den_free_field] = 1.0
    keys, bt, fi = id_keys(idx, fields, True)
    b = bt // T
    flat_d, ftab, total = tables(fields, 1, dev)
    f = np.maximum(fi, 0)
    plain = Ref(keys, dlogit[b], total, need_u=need_u, need_longest=need_longest)
    pooled = Ref(keys, (dlogit[b, 0] / den[b, f]).astype(np.float32)[:, None], total, order_matters=False)     # (the same order as `plain`)
    assert bool((plain.sums.view(np.int32) != pooled.sums.view(np.int32)).any()), "the denominators change nothing"
    if den_free_field is not None:
        lo = sum(x.vocab for x in fields[:den_free_field])
        sel = (plain.rows >= lo) & (plain.rows < lo + fields[den_free_field].vocab)
        assert sel.any() and np.array_equal(plain.sums[sel].view(np.int32), pooled.sums[sel].view(np.int32))
    c2f = ops.col2field_table(fields, L, dev)
    plan = Plan(B * L, dev, lib)
    ops.sparse_plan_ids(torch.from_numpy(idx).to(dev), ftab, c2f, nf, flat_d, 1, total, B, T, L, target_only=True, plan=plan, lib=lib)
    dlogit_b = Buf(B, torch.float32, dlogit, dev)
    den_b = Buf(B * nf, torch.float32, den, dev)
    inputs = (("dlogit", dlogit_b), ("lr_den", den_b))
    workload = "%s B=%d L=%d total_rows=%d" % (name, B, L, total)
    for w in which:
        for form, ref in (("plain", plain), ("pooled", pooled), ("pool entry point, lr_den = NULL", plain)):
            outs = Outs(w, ref, dev)
            a = outs.args(1)
            if form == "plain":
                ops.sparse_reduce_scalar(plan, dlogit_b.view.view(B, 1), B, L, out_rows=a["out_rows"], out_vals=a["out_grads"],
                                         dense_base=a["dense_base"], lib=lib)
            elif form == "pooled":
                ops.sparse_reduce_scalar(plan, dlogit_b.view.view(B, 1), B, L, out_rows=a["out_rows"], out_vals=a["out_grads"],
                                         dense_base=a["dense_base"], lr_den=den_b.view.view(B, nf), col2field=c2f, lib=lib)
            else:
                # (the one call past the wrapper: ops.sparse_reduce_scalar routes lr_den=None to the plain entry point itself)
                lib.call("rat_sparse_reduce_scalar_pool", ops._p(plan.ws), ops._p(plan.count), ops._p(dlogit_b.view), None, ops._p(c2f), nf,
                         B, L, ops._p(a["out_rows"]), ops._p(a["out_grads"]), ops._p(a["dense_base"]), ops._stream(dlogit_b.view))
            compare(test, workload, "%s, %s; U = %d, longest segment %d" % (form, w, ref.U, ref.longest), ref, plan, outs, inputs=inputs)
    return plain


def check_scalar_small(lib, dev, B):
    """sparse_cases.check_scalar_reduce's shape"""
    rs = np.random.RandomState(87)
    T, L = 3, 4
    fields = [F(0, 1, 5), F(1, 2, 4, padding_idx=3), F(3, 1, 6)]
    idx = np.stack([rs.randint(0, hi, size=(B, T)) for hi in (5, 4, 4, 6)], -1).astype(np.int32)
    idx[0, 0, 1], idx[1, 0, 2] = 3, 3
    check_scalar(lib, dev, "scalar", B, T, L, fields, idx, 88, need_u=8, need_longest=3, den_free_field=2)


def check_scalar_key_width(lib, dev):
    """total_rows = 2^24 + 3: a 64 MB width-1 table, 25-bit keys"""
    total, B, T, L = 2 ** 24 + 3, 3000, 2, 5
    fields = [F(0, 3, total - 3, padding_idx=1), F(3, 1, 3)]
    rs = np.random.RandomState(89)
    idx = np.stack([rs.randint(0, hi, size=(B, T)) for hi in (total - 3, total - 3, 50, 3, 9)], -1).astype(np.int32)
    idx[0, 0, 0], idx[0, 0, 1], idx[0, 0, 3], idx[B - 1, 0, 0] = 0, 1, 2, total - 4
    ref = check_scalar(lib, dev, "key-width", B, T, L, fields, idx, 90, need_u=B, need_longest=3, which=("all",))
    assert ref.rows[0] == 0 and ref.rows[-1] == total - 1 and int(ref.rows[-2]) >= 2 ** 24


def check_scalar_past_the_cap(lib, dev):
    """reduce_scalar_kernel<2> and <3> past 8192 x 256 segments: B = 300 000, L = 8, one bag field over a 4 M-row width-1 table"""
    B, T, L, vocab = 300000, 1, 8, 4000000
    idx = permuted_ids(np.random.RandomState(91), (B, T, L), vocab, 4000)
    ref = check_scalar(lib, dev, "past-the-cap scalar", B, T, L, [F(0, L, vocab)], idx, 92, need_u=2097152 + 1, need_longest=3,
                       which=("all",))
    assert ref.longest <= LOOP_MAX
    return ref


# ----------------------------------------------------------------------------- 4. lists (rat_sparse_plan_rows + rat_sparse_reduce_rows)
def check_lists(lib, dev, name, rows, counts, grads, total_rows, need_u=0, need_longest=0, order_matters=None):
    """rows: int32 [world][cap], counts: [world], grads: float32 [world][cap][d]; sums must come out in rank order"""
    test = "sparse_kernel_cases.check_lists"
    world, cap = rows.shape
    d = grads.shape[2]
    ref = Ref(row_keys(rows, counts, total_rows), grads.reshape(world * cap, d), total_rows, need_u=need_u, need_longest=need_longest,
              order_matters=order_matters)
    plan = Plan(world * cap, dev, lib)
    rows_b = Buf(world * cap, torch.int32, rows, dev)
    counts_b = Buf(world, torch.int32, np.asarray(counts, np.int32), dev)
    grads_b = Buf(world * cap * d, torch.float32, grads, dev)
    ops.sparse_plan_rows(rows_b.view, counts_b.view, cap, world, total_rows, plan=plan, lib=lib)
    outs = Outs("lists", ref, dev)
    ops.sparse_reduce_rows(plan, grads_b.view.view(world * cap, d), cap, world, d, outs.rows.view, outs.grads.view.view(outs.cap, d), lib=lib)
    compare(test, "%s world=%d cap=%d d=%d total_rows=%d" % (name, world, cap, d, total_rows), "U = %d, longest segment %d" % (ref.U, ref.longest),
            ref, plan, outs, inputs=(("rows", rows_b), ("counts", counts_b), ("gradient rows", grads_b)))
    return ref


def gathered_lists(world, cap, d, total_rows, seed):
    """a rank with count 0, a rank with count = cap; behind the count junk that LOOKS valid (rows in range, finite gradients); inside it
    negative rows, rows = total_rows and above; row 3 named twice by every rank that has a count"""
    rs = np.random.RandomState(seed)
    rows = rs.randint(0, total_rows, size=(world, cap)).astype(np.int32)
    counts = rs.randint(4, cap + 1, size=world)
    counts[1], counts[world - 1] = 0, cap
    for r in range(world):
        if counts[r]:
            spots = rs.choice(counts[r], size=4, replace=False)
            rows[r, spots[0]], rows[r, spots[1]] = -1 - r, total_rows + r      # rank 0: total_rows itself, the sort's invalid key
            rows[r, spots[2]] = rows[r, spots[3]] = 3
    return rows, counts, order_sensitive_row(rows, counts, spread(rs, world, cap, d), 3)


def order_sensitive_row(rows, counts, grads, row):
    """the gradients of `row`'s entries become 1, 2^-24, 2^-24, ...: in list order 1 + 2^-24 rounds back to 1 every time, in any order
    that adds two of the small terms first it does not — a width-1 list can tell the order too"""
    r, i = np.nonzero((rows == row) & (np.arange(rows.shape[1])[None, :] < np.asarray(counts)[:, None]))
    grads[r, i] = np.float32(2.0 ** -24)
    grads[r[0], i[0]] = 1.0
    return grads


def check_lists_case(lib, dev, world, cap, d):
    total_rows = 11 if cap < 100 else 500
    rows, counts, grads = gathered_lists(world, cap, d, total_rows, 93)
    ref = check_lists(lib, dev, "lists", rows, counts, grads, total_rows, need_u=min(total_rows, int(counts.sum())) // 3, need_longest=3)
    named = int(((rows == 3) & (np.arange(cap)[None, :] < counts[:, None])).sum())
    assert named >= world - 1 and 3 in ref.rows and ref.longest >= named


LISTS_CORE = [(3, 7, 1), (3, 7, 4), (3, 7, 10), (3, 7, 64), (8, 300, 1), (8, 300, 4), (8, 300, 10), (8, 300, 64)]


def check_lists_key_width(lib, dev, total_rows):
    rows, counts, grads = gathered_lists(3, 7, 4, total_rows, 94)
    counts[0] = 7
    rows[0, 0], rows[0, 1], rows[0, 2], rows[2, 0] = 0, total_rows - 1, total_rows, total_rows - 1
    grads = order_sensitive_row(rows, counts, spread(np.random.RandomState(99), 3, 7, 4), 3)
    ref = check_lists(lib, dev, "key-width", rows, counts, grads, total_rows, need_u=4, need_longest=2)
    assert ref.rows[0] == 0 and ref.rows[-1] == total_rows - 1 and bool((row_keys(rows, counts, total_rows) < 0).any())


def check_lists_past_the_cap(lib, dev):
    """world 8 x cap 20 000 at d = 64: more than 16 x 8192 unique rows"""
    world, cap, d, total_rows = 8, 20000, 64, 1000000
    rs = np.random.RandomState(95)
    rows = np.stack([rs.choice(total_rows, size=cap, replace=False) for _ in range(world)]).astype(np.int32)
    rows[:, 17] = 3
    counts = np.array([cap, cap - 1, cap, cap - 100, cap, cap, cap - 7, cap])
    return check_lists(lib, dev, "past-the-cap lists", rows, counts, spread(rs, world, cap, d), total_rows, need_u=131072 + 1, need_longest=8)


# ----------------------------------------------------------------------------- 5. degenerate plans and the workspace
def _ids_plan_case(lib, dev, name, ids, vocab, padding_idx, d=16):
    """B = len(ids), T = L = 1: one single-id field"""
    n = len(ids)
    idx = np.asarray(ids, np.int32).reshape(n, 1, 1)
    return check_bag(lib, dev, "%s (ids)" % name, d, n, 1, 1, [F(0, 1, vocab, padding_idx=padding_idx)], idx, 96, which=("all",))


def _rows_plan_case(lib, dev, name, rows, count, total_rows, d=16):
    """world = 1, cap = len(rows)"""
    rs = np.random.RandomState(97)
    rows = np.asarray(rows, np.int32).reshape(1, -1)
    return check_lists(lib, dev, "%s (rows)" % name, rows, [count], spread(rs, 1, rows.shape[1], d), total_rows)


def check_degenerate(lib, dev, name):
    """both plan entry points; invalid = the padding id (ids) / behind the count or outside the table (rows)"""
    rs = np.random.RandomState(98)
    if name == "n1-valid":
        a, b = _ids_plan_case(lib, dev, name, [2], 5, 4), _rows_plan_case(lib, dev, name, [2], 1, 5)
        assert a.U == 1 and b.U == 1
    elif name == "n1-invalid":
        a, b = _ids_plan_case(lib, dev, name, [4], 5, 4), _rows_plan_case(lib, dev, name, [2], 0, 5)
        c = _rows_plan_case(lib, dev, name + " row = total_rows", [5], 1, 5)
        assert a.U == 0 and b.U == 0 and c.U == 0
    elif name == "all-invalid":                                  # U = 0 and nothing written
        a, b = _ids_plan_case(lib, dev, name, [4] * 7, 5, 4), _rows_plan_case(lib, dev, name, [2, -1, 5, 0, 1, 3, 4], 0, 5)
        c = _rows_plan_case(lib, dev, name + " rows outside", [-1, 5, 6, -2, 2 ** 31 - 1, -2 ** 31, 5], 7, 5)
        assert a.U == 0 and b.U == 0 and c.U == 0
    elif name == "no-invalid":                                   # the last segment ends at n: seg_start[U] from the i == n - 1 branch
        a = _ids_plan_case(lib, dev, name, [0, 3, 1, 3, 0, 2, 3, 1, 0], 5, 4)
        b = _rows_plan_case(lib, dev, name, [0, 3, 1, 3, 0, 2, 3, 1, 0], 9, 5)
        c = _ids_plan_case(lib, dev, name + " one segment", [3] * 5, 5, 4)
        assert a.U == 4 and b.U == 4 and c.U == 1 and a.n == 9
    elif name == "one-invalid":
        a = _ids_plan_case(lib, dev, name, [0, 3, 1, 3, 4, 2, 3, 1, 0], 5, 4)
        b = _rows_plan_case(lib, dev, name, [0, 3, 1, 3, 0, 2, 3, 1, 0], 8, 5)
        assert a.U == 4 and b.U == 4
    elif name in ("n255", "n256", "n257", "n4097", "n163840"):    # the sizes around one block of the plan's kernels, and the workspace's
        n = int(name[1:])
        vocab = max(300, n // 2)
        a = _ids_plan_case(lib, dev, name, rs.randint(0, vocab, size=n), vocab, 4)
        b = _rows_plan_case(lib, dev, name, rs.randint(-2, vocab + 2, size=n), n - 3, vocab)
        assert a.U > min(n, vocab) // 3 and b.U > min(n, vocab) // 3 and a.n == n and b.n == n
    else:
        raise KeyError(name)


DEGENERATE_CORE = ["n1-valid", "n1-invalid", "all-invalid", "no-invalid", "one-invalid", "n255", "n256", "n257"]
WORKSPACE_SIZES_CORE = ["n1-valid", "n255", "n256", "n257"]                       # n = 1, 255, 256, 257 (the degenerate cases above)
WORKSPACE_SIZES_TWIN = ["n4097"]
WORKSPACE_SIZES_GPU_ONLY = ["n163840"]


def _refused(lib, text, fn, *args, **kw):
    try:
        fn(*args, lib=lib, **kw)
    except RatError as e:
        assert text in str(e), "refused with %r, expected %r" % (str(e), text)
        return
    raise AssertionError("the call was not refused (%s)" % text)


def check_workspace_one_byte_short(lib, dev):
    for n in (1, 257):
        plan = Plan(n, dev, lib, short=1)
        fields = [F(0, 1, 5)]
        flat_d, ftab, total = tables(fields, 4, dev)
        c2f = ops.col2field_table(fields, 1, dev)
        idx = torch.zeros((n, 1, 1), dtype=torch.int32, device=dev)
        _refused(lib, "workspace too small", ops.sparse_plan_ids, idx, ftab, c2f, 1, flat_d, 4, total, n, 1, 1, plan=plan)
        _refused(lib, "workspace too small", ops.sparse_plan_rows, idx.view(-1), torch.ones(1, dtype=torch.int32, device=dev), n, 1, 5, plan=plan)
        assert plan.intact() and int(plan.count.cpu()[0]) == -5 and bool((plan.ws == WS_SENT).all()), "a refused plan wrote something"


def check_refusals(lib, dev):
    """each returns the library's error without launching: nothing is written"""
    fields = [F(0, 1, 5)]
    B, T, L, d = 3, 1, 1, 260
    flat_d, ftab, total = tables(fields, d, dev)
    c2f = ops.col2field_table(fields, L, dev)
    idx = torch.tensor([0, 1, 1], dtype=torch.int32, device=dev).view(B, T, L)
    plan = Plan(B * T * L, dev, lib)
    ops.sparse_plan_ids(idx, ftab, c2f, 1, flat_d, d, total, B, T, L, plan=plan, lib=lib)
    assert int(plan.count.cpu()[0]) == 2
    rows = Buf(3, torch.int32, I_SENT, dev)
    grads = Buf(3 * d, torch.float32, F_SENT, dev)
    dense = Buf(total * d, torch.float32, DENSE_FILL, dev)
    dgrid = torch.ones(B * T * 2 * d, dtype=torch.float32, device=dev)
    _refused(lib, "row width above 256 floats", ops.sparse_reduce_grid, plan, dgrid, None, c2f, B, T, L, 1, d, out_rows=rows.view,
             out_grads=grads.view.view(3, d), dense_base=dense.view)
    _refused(lib, "null pointer", ops.sparse_reduce_grid, plan, dgrid, None, c2f, B, T, L, 1, 8, out_rows=rows.view)
    _refused(lib, "bad dims", ops.sparse_plan_ids, idx, ftab, c2f, 1, flat_d, d, 0, B, T, L, plan=plan)
    _refused(lib, "bad dims", ops.sparse_plan_rows, idx.view(-1), torch.ones(1, dtype=torch.int32, device=dev), 3, 1, 0, plan=plan)
    for b, fill in ((rows, I_SENT), (grads, F_SENT), (dense, DENSE_FILL)):
        assert b.intact() and bool((b.view == fill).all()), "a refused call wrote to an output"
    assert plan.intact() and int(plan.count.cpu()[0]) == 2
