"""Shared kernel-level checks of the eight entry points that exist only for data parallelism — SyncBN (rat_bn_local_stats,
rat_bn_relu_fwd_sync, rat_bn_bwd_local_sums, rat_bn_relu_bwd_sync; csrc/head.hip) and the owner-partitioned row-list exchange
(rat_owner_counts, rat_owner_pack, rat_owner_unpack, rat_owner_scatter; csrc/sparse.hip) — used with the host-emulation build on CPU
(tests/test_dp_kernels.py) and the HIP build on the GPU (tests/test_gpu_dp_kernels.py).

ONE process plays every rank in turn on ONE device: the collectives between the kernels belong to the caller, so the "all-gather" is a
torch.cat of what the ranks produced and the "all-to-all" is slicing.  Only the public `ops` wrappers are called.

SyncBN is compared with float64 torch.nn.functional.batch_norm over the WHOLE batch (+ the activation, + .backward); the tolerances are
the project's own BatchNorm tolerances (kernel_cases.check_bn_relu / check_bn_strip).  The two gates on a rank's local record are derived
where they are applied.  The owner exchange is data movement plus sums in a documented order: every assertion on it is bit-exact (floats
are compared as their 32-bit patterns, so a NaN that must survive compares equal and -0.0 does not pass for 0.0).

Every comparison records its margin (tests/margins.py); for the exact ones the recorded figure is the number of differing words."""
import numpy as np
import torch

import margins
from kernel_cases import F, rnd
from rat_amd import ops

SENT = 12345.0
JUNK_ROW = 777777
GUARD = 8                             # sentinel floats in front of and behind a guarded buffer (32 bytes: 16-byte alignment is kept)

ACT_FN = {"relu": torch.relu, "none": lambda t: t, "sigmoid": torch.sigmoid, "tanh": torch.tanh,
          "leakyrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.01), "elu": lambda t: torch.nn.functional.elu(t, 1.0)}


# ----------------------------------------------------------------------------- helpers
def gated(test, workload, quantity, got, ref, rtol, atol, where=""):
    """|got - ref| <= atol + rtol |ref| element by element (numpy's assert_allclose rule); the worst element goes to the margins file"""
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.detach().cpu().double().reshape(-1)
    assert got.shape == ref.shape, (test, quantity, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite %s (%s)" % (test, workload, quantity, where)
    allowed = atol + rtol * ref.abs()
    err = (got - ref).abs()
    k = int((err / (allowed + 1e-300)).argmax())
    margins.record(test, workload, quantity, float(err[k]), float(allowed[k]), arith="f32", where=where)
    assert float(err[k]) <= float(allowed[k]), "%s %s %s: |error| %.3g at element %d exceeds the gate %.3g (%s)" % (
        test, workload, quantity, float(err[k]), k, float(allowed[k]), where)


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def exact(test, workload, quantity, got, want, where=""):
    """the same shape, type and bits"""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, "%s %s %s: %s %s against %s %s (%s)" % (
        test, workload, quantity, g.shape, g.dtype, w.shape, w.dtype, where)
    bad = int((g != w).sum())
    margins.record(test, workload, quantity, bad, 0, arith="exact", where=where)
    first = int(np.flatnonzero((g != w).reshape(-1))[0]) if bad else -1
    assert bad == 0, "%s %s %s: %d of %d words differ, the first at %d (%s)" % (test, workload, quantity, bad, g.size, first, where)


class Guarded:
    """a float32 buffer of `shape` filled with `fill` between two runs of sentinels on `dev`"""

    def __init__(self, shape, fill, dev):
        self.n = int(np.prod(shape))
        buf = torch.full((GUARD + self.n + GUARD,), SENT, dtype=torch.float32)
        buf[GUARD:GUARD + self.n] = fill
        self.buf = buf.to(dev)
        self.view = self.buf[GUARD:GUARD + self.n].view(*shape)
        assert self.view.data_ptr() % 16 == 0

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.n:] == SENT).all())


def pad4(n):
    return (n + 3) // 4 * 4


def _owner_of(rows, per, world):
    return np.minimum(np.asarray(rows, dtype=np.int64) // per, world - 1)


# ----------------------------------------------------------------------------- 1. SyncBN
def check_sync_bn(lib, dev, shards, N, act, use_offsets=True):
    """shards: rows per simulated rank.  use_offsets: a rank's shard is a view into the one [M][N] matrix at its row offset (for N % 4
    != 0 the shards then start off a 16-byte boundary); otherwise every shard is a tensor of its own"""
    test = "dp_cases.check_sync_bn"
    world, M = len(shards), int(sum(shards))
    workload = "shards=%s N=%d %s" % ("%dx%d" % (world, shards[0]) if len(set(shards)) == 1 else list(shards), N, act)
    code, fn = ops.ACT[act], ACT_FN[act]
    rs = np.random.RandomState(71)
    z = rnd(rs, M, N) + 3.0 * rnd(rs, N)                       # column means of a few standard deviations, as check_bn_strip
    gamma, beta = 1 + 0.1 * rnd(rs, N), 0.1 * rnd(rs, N)
    rm, rv = 0.1 * rnd(rs, N), 1 + 0.1 * rnd(rs, N).abs()
    da = rnd(rs, M, N)
    # reference: float64 BatchNorm over the whole batch
    zr = z.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm_ref, rv_ref = rm.double().clone(), rv.double().clone()
    yr = fn(torch.nn.functional.batch_norm(zr, rm_ref, rv_ref, gr, br, training=True, momentum=0.1, eps=1e-5))
    yr.backward(da.double())

    zd_all, dad_all, gd, bd = z.to(dev), da.to(dev), gamma.to(dev), beta.to(dev)

    def fresh(t):                                               # (on the CPU .to(dev) alone would hand out the tensor itself)
        return t.clone().to(dev)
    starts = np.concatenate([[0], np.cumsum(shards)]).astype(int)

    def shard(t, r):
        v = t[starts[r]:starts[r + 1]]
        return v if use_offsets else v.clone()
    zs, das = [shard(zd_all, r) for r in range(world)], [shard(dad_all, r) for r in range(world)]

    # forward pass 1: every rank's local record
    got = []
    for r in range(world):
        ops.bn_relu_fwd_sync(zs[r], gd, bd, fresh(rm), fresh(rv), lambda s: (got.append(s.clone()), s)[1], act=code, lib=lib)
    assert len(got) == world and all(g.shape == (2 * N + 1,) for g in got)
    for r in range(world):
        rec, rows = got[r].cpu(), int(shards[r])
        z64 = z[starts[r]:starts[r + 1]].double()
        where = "rank %d, %d rows" % (r, rows)
        assert float(rec[2 * N]) == float(rows), "the record's row count (%s)" % where
        if rows == 1:
            exact(test, workload, "local mean of a one-row shard", rec[:N], z[starts[r]], where=where)
            exact(test, workload, "local M2 of a one-row shard", rec[N:2 * N], torch.zeros(N), where=where)
            continue
        mean64 = z64.mean(0)
        m2_64 = ((z64 - mean64) ** 2).sum(0)
        # mean = pivot + s1 / rows with the pivot a row of the shard: the shifted terms, their sum, the division and the final addition
        # are each good to a few roundings of a number no larger than 2 max|z| -> 16 ulp of max|z| of the column
        zmax = z64.abs().max(0).values
        err = (rec[:N].double() - mean64).abs()
        k = int((err / zmax).argmax())
        margins.record(test, workload, "local mean", float(err[k]), float(16 * 2.0 ** -24 * zmax[k]), arith="f32", where=where)
        assert bool((err <= 16 * 2.0 ** -24 * zmax).all()), "local mean: %.3g against %.3g (%s)" % (
            float(err[k]), float(16 * 2.0 ** -24 * zmax[k]), where)
        # M2 = s2 - s1 d1 about a pivot within ~3 sigma of the mean: the subtraction amplifies rounding by at most ~10, and s2 is a
        # chain of ~50 fp32 additions (rows / 8 per thread, 8 row groups, 32 splits) -> 10 x 50 x 2^-24 = 3e-5 relative
        gated(test, workload, "local M2", rec[N:2 * N], m2_64, 3e-5, 0.0, where=where)

    # forward pass 2: the gathered records, rank after rank
    all_stats = torch.cat(got).contiguous()
    fwd = []
    for r in range(world):
        rmd, rvd = fresh(rm), fresh(rv)
        a, sm, sr, st = ops.bn_relu_fwd_sync(zs[r], gd, bd, rmd, rvd, lambda s: all_stats, act=code, lib=lib)
        assert st is all_stats
        fwd.append(dict(a=a, sm=sm, sr=sr, rm=rmd, rv=rvd))
    gated(test, workload, "a", torch.cat([f["a"] for f in fwd]), yr, 1e-5, 1e-5)
    for r in range(world):
        gated(test, workload, "running_mean", fwd[r]["rm"], rm_ref, 1e-5, 1e-6, where="rank %d" % r)
        gated(test, workload, "running_var", fwd[r]["rv"], rv_ref, 1e-5, 1e-6, where="rank %d" % r)     # unbiased with the GLOBAL n
        for q in ("sm", "sr", "rm", "rv"):
            exact(test, workload, "%s: the same bits on every rank" % q, fwd[r][q], fwd[0][q], where="rank %d against rank 0" % r)

    # backward, the same two passes: local sums first, then their fp32 sum in rank order
    local = []
    for r in range(world):
        f = fwd[r]
        ops.bn_relu_bwd_sync(zs[r], f["a"], das[r], gd, f["sm"], f["sr"], torch.zeros(N, device=dev), torch.zeros(N, device=dev),
                             lambda t: (local.append(t.clone()), t)[1], all_stats, act=code, lib=lib)
    assert len(local) == world and all(t.shape == (2 * N,) for t in local)
    glob = torch.zeros(2 * N, dtype=torch.float32, device=dev)
    for t in local:
        glob = glob + t
    bwd = []
    for r in range(world):
        f = fwd[r]
        dg, db = torch.full((N,), SENT, device=dev), torch.full((N,), SENT, device=dev)
        dz = ops.bn_relu_bwd_sync(zs[r], f["a"], das[r], gd, f["sm"], f["sr"], dg, db, lambda t: glob, all_stats, act=code, lib=lib)
        exact(test, workload, "dbeta = this rank's local sum of g", db, local[r][:N], where="rank %d" % r)
        exact(test, workload, "dgamma = this rank's local sum of g xhat", dg, local[r][N:], where="rank %d" % r)
        bwd.append(dict(dz=dz, dg=dg, db=db))
    gated(test, workload, "dz", torch.cat([b["dz"] for b in bwd]), zr.grad, 1e-4, 1e-5)
    scale = max(1.0, M ** 0.5)
    gated(test, workload, "dgamma summed over the ranks", sum(b["dg"].cpu().double() for b in bwd), gr.grad, 1e-4, 1e-5 * scale)
    gated(test, workload, "dbeta summed over the ranks", sum(b["db"].cpu().double() for b in bwd), br.grad, 1e-4, 1e-5 * scale)

    # a record with row count 0 (its mean and M2 are junk) between the others, world + 1: the same bits, forward and backward
    junk = torch.full((2 * N + 1,), 1e30, dtype=torch.float32)
    junk[2 * N] = 0.0
    cut = min(1, world) * (2 * N + 1)
    spliced = torch.cat([all_stats[:cut], junk.to(dev), all_stats[cut:]]).contiguous()
    rmd, rvd = fresh(rm), fresh(rv)
    a2, sm2, sr2, _ = ops.bn_relu_fwd_sync(zs[0], gd, bd, rmd, rvd, lambda s: spliced, act=code, lib=lib)
    dg2, db2 = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    dz2 = ops.bn_relu_bwd_sync(zs[0], a2, das[0], gd, sm2, sr2, dg2, db2, lambda t: glob, spliced, act=code, lib=lib)
    for q, x, y in (("a", a2, fwd[0]["a"]), ("save_mean", sm2, fwd[0]["sm"]), ("save_rstd", sr2, fwd[0]["sr"]),
                    ("running_mean", rmd, fwd[0]["rm"]), ("running_var", rvd, fwd[0]["rv"]), ("dz", dz2, bwd[0]["dz"]),
                    ("dgamma", dg2, bwd[0]["dg"]), ("dbeta", db2, bwd[0]["db"])):
        exact(test, workload, "%s with an empty rank's record spliced in" % q, x, y)

    if world == 1:
        # one rank: the sync chain against the two-launch kernels (the strip-against-two-launch tolerances of check_bn_strip)
        rm1, rv1 = fresh(rm), fresh(rv)
        a1, sm1, sr1 = ops.bn_relu_fwd(zs[0], gd, bd, rm1, rv1, True, True, act=code, lib=lib)
        dg1, db1 = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        dz1 = ops.bn_relu_bwd(zs[0], a1, das[0], gd, sm1, sr1, dg1, db1, True, act=code, lib=lib)
        gated(test, workload, "a against rat_bn_relu_fwd", fwd[0]["a"], a1, 1e-5, 1e-5)
        gated(test, workload, "save_mean against rat_bn_relu_fwd", fwd[0]["sm"], sm1, 1e-6, 1e-6)
        gated(test, workload, "save_rstd against rat_bn_relu_fwd", fwd[0]["sr"], sr1, 1e-5, 1e-6)
        gated(test, workload, "dz against rat_bn_relu_bwd", bwd[0]["dz"], dz1, 1e-4, 1e-5)


def sync_bn_id(case):
    shards, N, act = case
    return "%s-N%d-%s" % ("%dx%d" % (len(shards), shards[0]) if len(set(shards)) == 1 else "_".join(map(str, shards)), N, act)


RAGGED8 = [512, 511, 1, 300, 77, 512, 33, 64]
SYNC_BN_CORE = [([5, 4], 12, "relu"), ([37, 1, 64, 9], 40, "relu"), ([33, 31], 37, "tanh"), ([20], 12, "relu")]
SYNC_BN_TWIN = [([33] * 8, 37, "none"), ([64, 64], 400, "relu")]
SYNC_BN_GPU_ONLY = [([512] * 8, 400, "relu"), (RAGGED8, 400, "relu"), (RAGGED8, 37, "sigmoid"), (RAGGED8, 37, "elu"),
                    ([4100, 3], 64, "leakyrelu"), ([4096], 400, "relu")]


# ----------------------------------------------------------------------------- 2. the owner exchange chain
def edge_lists(world, total_a, total_b, n_a, n_b, seed, quiet=None):
    """per rank (sorted unique rows A, sorted unique rows B): n_a[r] / n_b[r] random rows plus, for each family, the rows on both sides
    of every range edge, row 0 and the family's last row — all of them on one rank (A: the last, B: rank 0), each on the others with
    probability 1/2.  Rank 0 holds no A row, the last rank no B row; owner `quiet` receives nothing"""
    rs = np.random.RandomState(seed)
    out = [[None, None] for _ in range(world)]
    for f, (total, counts, full, empty) in enumerate(((total_a, n_a, world - 1, 0), (total_b, n_b, 0, world - 1))):
        per = -(-total // world)
        edges = {0, total - 1}
        for k in range(1, world):
            edges |= {r_ for r_ in (k * per - 1, k * per) if 0 <= r_ < total}
        edges = np.array(sorted(edges), dtype=np.int64)
        for r in range(world):
            if r == empty:
                rows = np.zeros(0, dtype=np.int64)
            else:
                rows = rs.choice(total, size=min(int(counts[r]), total), replace=False)
                rows = np.union1d(rows, edges if r == full else edges[rs.rand(len(edges)) < 0.5])
                if quiet is not None:
                    rows = rows[_owner_of(rows, per, world) != quiet]
            out[r][f] = np.unique(rows).astype(np.int32)
    return [tuple(x) for x in out]


def skewed_lists(world, total_a, total_b, heavy, target, seed):
    """rank 0 holds `heavy` A rows that all lie in owner `target`'s range; the other ranks a few hundred rows anywhere"""
    rs = np.random.RandomState(seed)
    per = -(-total_a // world)
    lo, hi = target * per, min((target + 1) * per, total_a)
    assert hi - lo >= heavy
    out = [(np.sort(lo + rs.choice(hi - lo, size=heavy, replace=False)).astype(np.int32),
            np.sort(rs.choice(total_b, size=50, replace=False)).astype(np.int32))]
    for r in range(1, world):
        out.append((np.sort(rs.choice(total_a, size=200 + 37 * r, replace=False)).astype(np.int32),
                    np.sort(rs.choice(total_b, size=100 + 11 * r, replace=False)).astype(np.int32)))
    return out


def check_owner_chain(lib, dev, world, d, total_a, total_b, lists, n_extra, bucket):
    """counts -> pack -> ("all-to-all") -> unpack -> owner merge -> ("all-gather") -> scatter, the steps of
    dp.py::_exchange_lists_owner, every intermediate buffer compared bit for bit with what its layout (include/rat_hip.h) says"""
    test = "dp_cases.check_owner_chain"
    workload = "world=%d d=%d totals=%d/%d extra=%d" % (world, d, total_a, total_b, n_extra)
    assert len(lists) == world and d % 4 == 0 and bucket % 4 == 0
    rs = np.random.RandomState(72)
    totals, widths = (total_a, total_b), (d, 1)
    per = tuple(-(-t // world) for t in totals)

    def bucketed(n):
        return max(bucket, -(-n // bucket) * bucket)

    def chunk(na, nb):
        return pad4(na) + na * d + 2 * pad4(nb)
    # this rank's local lists: buffers longer than the count, junk rows and random gradients behind it
    rows_h, grads_h, rows_d, grads_d, extra_h, extra_d = [], [], [], [], [], []
    for r in range(world):
        rh, gh, rd, gdv = [], [], [], []
        for f in (0, 1):
            mine = np.asarray(lists[r][f], dtype=np.int32)
            assert np.array_equal(mine, np.unique(mine)) and (mine.size == 0 or (mine[0] >= 0 and mine[-1] < totals[f]))
            cap = mine.size + 5 + 2 * r
            buf = np.full(cap, JUNK_ROW, dtype=np.int32)
            buf[:mine.size] = mine
            g = rnd(rs, cap, widths[f]).numpy()
            rh.append(mine), gh.append(g[:mine.size])
            rd.append(torch.from_numpy(buf).to(dev)), gdv.append(torch.from_numpy(g).to(dev))
        rows_h.append(rh), grads_h.append(gh), rows_d.append(rd), grads_d.append(gdv)
        extra_h.append(rnd(rs, n_extra).numpy())
        extra_d.append(torch.from_numpy(extra_h[r]).to(dev) if n_extra else None)
    owner_h = [[_owner_of(rows_h[r][f], per[f], world) for f in (0, 1)] for r in range(world)]

    # 1. counts: the plan of a rank's list -> its pairs per owner
    mat_d = torch.full((world, 2, world), -9, dtype=torch.int32, device=dev)
    for r in range(world):
        for f in (0, 1):
            cnt = torch.tensor([rows_h[r][f].size], dtype=torch.int32).to(dev)
            plan = ops.sparse_plan_rows(rows_d[r][f], cnt, rows_d[r][f].numel(), 1, totals[f], lib=lib)
            ops.owner_counts(plan, per[f], world, mat_d[r, f], lib=lib)
    S = np.stack([np.stack([np.bincount(owner_h[r][f], minlength=world) for f in (0, 1)]) for r in range(world)]).astype(np.int32)
    exact(test, workload, "count matrix", mat_d, S)
    S = S.astype(np.int64)
    max_pairs = int(S.sum(1).max())

    # 2. pack: one chunk per owner, [rows A pad 4][gradient rows A][rows B pad 4][values B pad 4]
    wires = []
    for r in range(world):
        n_send = sum(chunk(int(S[r, 0, k]), int(S[r, 1, k])) for k in range(world))
        wire = torch.full((n_send + 8,), float("nan"), dtype=torch.float32, device=dev)
        ops.owner_pack(mat_d, world, r, d, rows_d[r][0], grads_d[r][0], rows_d[r][1], grads_d[r][1], max_pairs, wire, lib=lib)
        w = wire.cpu().numpy()
        want = w.copy()                                         # padding words are unspecified: they are taken from the result
        wanti = want.view(np.int32)
        off, bounds = 0, []
        for k in range(world):
            na, nb = int(S[r, 0, k]), int(S[r, 1, k])
            sel_a, sel_b = owner_h[r][0] == k, owner_h[r][1] == k
            o_ga = off + pad4(na)
            o_rb = o_ga + na * d
            o_vb = o_rb + pad4(nb)
            wanti[off:off + na] = rows_h[r][0][sel_a]
            want[o_ga:o_rb] = grads_h[r][0][sel_a].reshape(-1)
            wanti[o_rb:o_rb + nb] = rows_h[r][1][sel_b]
            want[o_vb:o_vb + nb] = grads_h[r][1][sel_b].reshape(-1)
            bounds.append((off, o_vb + pad4(nb)))
            off = o_vb + pad4(nb)
        assert off == n_send
        exact(test, workload, "wire: rows and gradient rows of both families, chunk by chunk", w, want, where="sender %d" % r)
        assert bool(np.isnan(w[n_send:]).all()), "rat_owner_pack wrote behind the last chunk (sender %d)" % r
        wires.append((w, bounds))

    # 3. + 4. the all-to-all (owner r receives every sender's chunk r, in rank order) and the unpack into the list this rank will gather
    cap_a, cap_b = bucketed(int(S[:, 0, :].sum(0).max())), bucketed(int(S[:, 1, :].sum(0).max()))
    xpad = pad4(n_extra)
    stride = 4 + xpad + cap_a * (1 + d) + 2 * cap_b
    o_ra = 4 + xpad
    o_ga, o_rb = o_ra + cap_a, o_ra + cap_a * (1 + d)
    o_vb = o_rb + cap_b
    mines, merged = [], []
    for r in range(world):
        recv_h = np.concatenate([w[b[r][0]:b[r][1]] for w, b in wires] + [np.zeros(0, dtype=np.float32)])
        n_recv = recv_h.size
        recv = torch.full((max(n_recv, 4),), float("nan"), dtype=torch.float32)
        recv[:n_recv] = torch.from_numpy(recv_h)
        recv = recv.to(dev)
        mine = torch.full((stride,), float("nan"), dtype=torch.float32, device=dev)       # dp.py: torch.empty
        mine_i = mine.view(torch.int32)
        mine_i[o_ra:o_ga] = JUNK_ROW
        mine_i[o_rb:o_vb] = JUNK_ROW
        before = mine.cpu().numpy().copy()
        got_ra = torch.full((cap_a,), -5, dtype=torch.int32, device=dev)
        got_ga = torch.full((cap_a, d), SENT, dtype=torch.float32, device=dev)
        got_rb = torch.full((cap_b,), -5, dtype=torch.int32, device=dev)
        got_vb = torch.full((cap_b,), SENT, dtype=torch.float32, device=dev)
        tot = torch.full((2,), -1, dtype=torch.int32, device=dev)
        ops.owner_unpack(mat_d, world, r, d, recv, max_pairs, got_ra, got_ga, got_rb, got_vb, tot,
                         extra_src=extra_d[r], extra_dst=mine[4:4 + n_extra] if n_extra else None, lib=lib)
        want_r = [np.concatenate([rows_h[s][f][owner_h[s][f] == r] for s in range(world)]) for f in (0, 1)]
        want_g = [np.concatenate([grads_h[s][f][owner_h[s][f] == r] for s in range(world)]) for f in (0, 1)]
        ta, tb = want_r[0].size, want_r[1].size
        where = "owner %d" % r
        exact(test, workload, "unpack: totals", tot, np.array([ta, tb], dtype=np.int32), where=where)
        exact(test, workload, "unpack: rows A", got_ra, np.concatenate([want_r[0], np.full(cap_a - ta, -5, dtype=np.int32)]), where=where)
        exact(test, workload, "unpack: gradient rows A", got_ga,
              np.concatenate([want_g[0], np.full((cap_a - ta, d), SENT, dtype=np.float32)]), where=where)
        exact(test, workload, "unpack: rows B", got_rb, np.concatenate([want_r[1], np.full(cap_b - tb, -5, dtype=np.int32)]), where=where)
        exact(test, workload, "unpack: values B", got_vb,
              np.concatenate([want_g[1].reshape(-1), np.full(cap_b - tb, SENT, dtype=np.float32)]), where=where)
        after = mine.cpu().numpy()
        exact(test, workload, "unpack: extra floats", after[4:4 + n_extra], extra_h[r], where=where)
        before[4:4 + n_extra] = extra_h[r]
        exact(test, workload, "unpack: the rest of the list", after, before, where=where)
        # 5. the owner's merge, exactly as dp.py runs it: sort + in-order segment sums, written straight into the list
        plan = ops.sparse_plan_rows(got_ra, tot[0:1], cap_a, 1, total_a, count_out=mine_i[0:1], lib=lib)
        ops.sparse_reduce_rows(plan, got_ga, cap_a, 1, d, mine_i[o_ra:o_ga], mine[o_ga:o_rb].view(cap_a, d), count=mine_i[0:1], lib=lib)
        plan = ops.sparse_plan_rows(got_rb, tot[1:2], cap_b, 1, total_b, count_out=mine_i[1:2], lib=lib)
        ops.sparse_reduce_rows(plan, got_vb.view(cap_b, 1), cap_b, 1, 1, mine_i[o_rb:o_vb], mine[o_vb:].view(cap_b, 1), count=mine_i[1:2],
                               lib=lib)
        m = mine.cpu().numpy()
        mi = m.view(np.int32)
        ref = []
        for f, (o_r, o_g) in enumerate(((o_ra, o_ga), (o_rb, o_vb))):
            uniq = np.unique(want_r[f])
            acc = np.zeros((uniq.size, widths[f]), dtype=np.float32)
            pos = np.searchsorted(uniq, want_r[f])
            first = 0
            for s in range(world):                              # a sender's rows are unique: one fp32 addition per row and sender
                n_s = int((owner_h[s][f] == r).sum())
                acc[pos[first:first + n_s]] += want_g[f][first:first + n_s]
                first += n_s
            assert int(mi[f]) == uniq.size, "merged count of family %d on owner %d: %d against %d" % (f, r, int(mi[f]), uniq.size)
            exact(test, workload, "merge: rows", mi[o_r:o_r + uniq.size], uniq.astype(np.int32), where="%s family %d" % (where, f))
            exact(test, workload, "merge: sums", m[o_g:o_g + uniq.size * widths[f]], acc.reshape(-1), where="%s family %d" % (where, f))
            ref.append((uniq, acc))
        merged.append(ref)
        mines.append(mine)

    # 6. the all-gather and the scatter into the dense blocks: zeros where a list names a row, 7.0 elsewhere
    everyone = torch.cat(mines).contiguous()
    dense, want_dense = [], []
    for f in (0, 1):
        fill = np.full((totals[f], widths[f]), 7.0, dtype=np.float32)
        named = np.unique(np.concatenate([rows_h[r][f] for r in range(world)]))
        fill[named] = 0.0
        blk = Guarded(fill.shape, torch.from_numpy(fill).reshape(-1), dev)
        for r in range(world):                                  # "for each rank in order, ref[rows] += grads", fp32
            fill[rows_h[r][f]] += grads_h[r][f]
        dense.append(blk), want_dense.append(fill)
    extra_out = Guarded((max(n_extra, 1),), 3.0, dev)
    ops.owner_scatter(dense[0].view, dense[1].view, extra_out.view if n_extra else None, everyone, stride, world, cap_a, cap_b, d, n_extra,
                      lib=lib)
    assert dense[0].intact() and dense[1].intact() and extra_out.intact()
    exact(test, workload, "scatter: dense A", dense[0].view, want_dense[0])
    exact(test, workload, "scatter: dense B", dense[1].view, want_dense[1])
    acc = np.zeros(n_extra, dtype=np.float32)
    for r in range(world):
        acc = acc + extra_h[r]
    if n_extra:
        exact(test, workload, "scatter: extra floats summed in rank order", extra_out.view, acc)
    else:
        assert float(extra_out.view[0]) == 3.0
    return dict(max_pairs=max_pairs, cap_a=cap_a, cap_b=cap_b, S=S)


def _chain_w3():
    return (3, 8, 50, 23, edge_lists(3, 50, 23, [0, 9, 12], [6, 5, 0], 1, quiet=1), 3, 8)


def _chain_w2():
    # 400 A rows on rank 1, about half of them for each owner: more than 121 pairs for a (sender, owner) -> two blocks per peer
    return (2, 64, 1000, 300, edge_lists(2, 1000, 300, [0, 400], [40, 0], 2), 4, 64)


def _chain_w8():
    return (8, 4, 37, 11, edge_lists(8, 37, 11, [0, 5, 9, 3, 12, 1, 7, 4], [3, 2, 5, 1, 4, 2, 3, 0], 3, quiet=6), 5, 4)


def _chain_w8_large():
    return (8, 64, 200000, 50000, edge_lists(8, 200000, 50000, [0] + [6900] * 7, [1700] * 7 + [0], 4, quiet=5), 0, 4096)


def _chain_w8_skewed():
    total_a = 320003
    return (8, 64, total_a, 50000, skewed_lists(8, total_a, 50000, 40000, 3, 5), 3, 4096)


OWNER_CHAIN_CORE = {"world3-d8": _chain_w3, "world2-d64-two-blocks-per-peer": _chain_w2, "world8-d4": _chain_w8}
OWNER_CHAIN_GPU_ONLY = {"world8-d64-200000-rows": _chain_w8_large, "world8-d64-skewed-40000-rows-for-one-owner": _chain_w8_skewed}


def check_owner_chain_case(lib, dev, name):
    make = OWNER_CHAIN_CORE.get(name) or OWNER_CHAIN_GPU_ONLY[name]
    world, d, total_a, total_b, lists, n_extra, bucket = make()
    res = check_owner_chain(lib, dev, world, d, total_a, total_b, lists, n_extra, bucket)
    # what the case is there for (csrc/sparse.hip: owner_blocks_per_peer, rat_owner_scatter's grid)
    bpp = -(-res["max_pairs"] * (d // 4 + 1) // 2048)
    S = res["S"]
    if name != "world8-d64-skewed-40000-rows-for-one-owner":
        assert any(r_.size == 0 for r_, _ in lists) and any(r_.size == 0 for _, r_ in lists), "a rank without A rows, one without B rows"
    if name in ("world3-d8", "world8-d4"):
        assert total_a % world and total_b % world, "totals that the world does not divide"
    if world > 2 and name != "world8-d64-skewed-40000-rows-for-one-owner":
        assert any(S[:, :, k].sum() == 0 for k in range(world)), "an owner that receives nothing"
    if name == "world2-d64-two-blocks-per-peer":
        assert 2 <= bpp <= 2048 // world
    if name == "world8-d64-200000-rows":
        assert 4 <= bpp <= 2048 // world and res["cap_a"] * (d // 4) > 1024
    if name == "world8-d64-skewed-40000-rows-for-one-owner":
        assert res["max_pairs"] > 30841 and bpp > 2048 // world
    return res


# ----------------------------------------------------------------------------- 3a. rat_owner_counts directly
def _counts_from_rows(lib, dev, rows, count, total, per, world, where):
    test, workload = "dp_cases.check_owner_counts", where
    rows = np.asarray(rows, dtype=np.int32)
    buf = np.concatenate([rows, np.full(3, JUNK_ROW, dtype=np.int32)])
    assert count <= rows.size
    plan = ops.sparse_plan_rows(torch.from_numpy(buf).to(dev), torch.tensor([count], dtype=torch.int32).to(dev), buf.size, 1, total, lib=lib)
    out = torch.full((world + 2,), -9, dtype=torch.int32, device=dev)
    ops.owner_counts(plan, per, world, out[1:1 + world], lib=lib)
    uniq = np.unique(rows[:count])
    want = np.concatenate([[-9], np.bincount(_owner_of(uniq, per, world), minlength=world), [-9]]).astype(np.int32)
    exact(test, workload, "counts", out, want)
    assert int(plan.count.cpu()[0]) == uniq.size


def check_owner_counts(lib, dev, case):
    cpw = lambda total, world: -(-total // world)               # noqa: E731
    if case == "empty-plan":
        _counts_from_rows(lib, dev, [3, 7, 11], 0, 50, cpw(50, 4), 4, case)
    elif case == "world1":
        _counts_from_rows(lib, dev, [0, 3, 7, 49], 4, 50, 50, 1, case)
    elif case == "world8-total5":                               # per = 1: more owners than rows, owners 5 .. 7 hold nothing
        _counts_from_rows(lib, dev, [0, 2, 4, 1], 4, 5, cpw(5, 8), 8, case)
        _counts_from_rows(lib, dev, [4], 1, 5, cpw(5, 8), 8, case)
    elif case == "all-in-the-last-range":                       # world 4, total 50: per = 13, the last owner holds rows 39 .. 49
        _counts_from_rows(lib, dev, list(range(39, 50)), 11, 50, cpw(50, 4), 4, case)
    elif case == "range-edges":                                 # both sides of every edge, and only one side of it
        _counts_from_rows(lib, dev, [0, 12, 13, 25, 26, 38, 39, 49], 8, 50, cpw(50, 4), 4, case)
        _counts_from_rows(lib, dev, [13, 26, 39], 3, 50, cpw(50, 4), 4, case)
        _counts_from_rows(lib, dev, [12, 25, 38], 3, 50, cpw(50, 4), 4, case)
    elif case == "duplicates":                                  # the counts are of UNIQUE rows, in whatever order the rows come
        _counts_from_rows(lib, dev, [26, 3, 3, 49, 26, 13, 3, 12, 49, 0, 26], 11, 50, cpw(50, 4), 4, case)
    elif case == "short-ranges":                                # per x world < total: the rows behind the last edge are the last owner's
        _counts_from_rows(lib, dev, [0, 11, 12, 35, 36, 47, 48, 49], 8, 50, 12, 4, case)
    elif case == "plan-from-ids":
        _counts_from_ids(lib, dev)
    else:
        raise KeyError(case)


OWNER_COUNTS_CASES = ["empty-plan", "world1", "world8-total5", "all-in-the-last-range", "range-edges", "duplicates", "short-ranges",
                      "plan-from-ids"]


def _counts_from_ids(lib, dev, B=5, T=4, d=8):
    """the production path of dp.py::_owner_prepare: a plan of the batch's ids (a bag field with a padding id, repeated ids, an id
    outside its vocabulary) as sparse_cases.check_sorted_reduce builds it; reference: np.unique of the global rows on the host"""
    test = "dp_cases.check_owner_counts"
    rs = np.random.RandomState(73)
    L = 5
    fields = [F(0, 1, 7), F(1, 3, 6, padding_idx=5), F(4, 1, 9, padding_idx=8)]
    col_field = [0, 1, 1, 1, 2]
    first_row = np.concatenate([[0], np.cumsum([f.vocab for f in fields])])
    total_rows = int(first_row[-1])
    idx = torch.stack([torch.from_numpy(rs.randint(0, [7, 6, 6, 6, 9][c], size=(B, T))) for c in range(L)], -1).int().contiguous()
    idx[0, 1, 0] = 99                                           # clamped to the vocabulary's last row, like the forward gather
    rows = []
    for c in range(L):
        f = fields[col_field[c]]
        ids = np.clip(idx[..., c].numpy().reshape(-1), 0, f.vocab - 1)
        rows.append(first_row[col_field[c]] + ids[ids != (f.padding_idx if f.padding_idx is not None else -1)])
    flat_d = torch.zeros(total_rows * d, dtype=torch.float32, device=dev)
    tabs = [flat_d[first_row[i] * d:first_row[i + 1] * d].view(f.vocab, d) for i, f in enumerate(fields)]
    ftab, c2f = ops.field_table(fields, tabs, dev), ops.col2field_table(fields, L, dev)
    for target_only in (False, True):
        if target_only:
            hits = []
            for c in range(L):
                f = fields[col_field[c]]
                ids = np.clip(idx[:, 0, c].numpy(), 0, f.vocab - 1)
                hits.append(first_row[col_field[c]] + ids[ids != (f.padding_idx if f.padding_idx is not None else -1)])
        else:
            hits = rows
        uniq = np.unique(np.concatenate(hits))
        plan = ops.sparse_plan_ids(idx.to(dev), ftab, c2f, 3, flat_d, d, total_rows, B, T, L, target_only=target_only, lib=lib)
        assert int(plan.count.cpu()[0]) == uniq.size
        for world in (3, 8):
            per = -(-total_rows // world)
            out = torch.full((world,), -9, dtype=torch.int32, device=dev)
            ops.owner_counts(plan, per, world, out, lib=lib)
            exact(test, "plan-from-ids", "counts", out, np.bincount(_owner_of(uniq, per, world), minlength=world).astype(np.int32),
                  where="world %d, target_only %s" % (world, target_only))


# ----------------------------------------------------------------------------- 3b. rat_owner_scatter on hand-built lists
def check_owner_scatter(lib, dev, world, d, cap_a, cap_b, counts, n_extra, total_a, total_b):
    """counts: per list (rows A, rows B), each no larger than its capacity; behind the count a list holds row 777777 and NaN gradients.
    The lists' rows are disjoint (the owners' ranges are), so the dense blocks receive plain stores"""
    test = "dp_cases.check_owner_scatter"
    workload = "world=%d d=%d cap=%d/%d extra=%d" % (world, d, cap_a, cap_b, n_extra)
    assert len(counts) == world and all(na <= cap_a and nb <= cap_b for na, nb in counts)
    rs = np.random.RandomState(74)
    xpad = pad4(n_extra)
    stride = 4 + xpad + cap_a * (1 + d) + 2 * cap_b
    o_ra = 4 + xpad
    o_ga, o_rb = o_ra + cap_a, o_ra + cap_a * (1 + d)
    o_vb = o_rb + cap_b
    lists = np.full((world, stride), np.nan, dtype=np.float32)
    li = lists.view(np.int32)
    li[:, o_ra:o_ga] = JUNK_ROW
    li[:, o_rb:o_vb] = JUNK_ROW
    perm_a, perm_b = rs.permutation(total_a), rs.permutation(max(total_b, 1))
    want_a = np.full((total_a, d), 7.0, dtype=np.float32)
    want_b = np.full(max(total_b, 1), 7.0, dtype=np.float32)
    want_x = np.zeros(n_extra, dtype=np.float32)
    ua = ub = 0
    for k, (na, nb) in enumerate(counts):
        li[k, 0], li[k, 1] = na, nb
        li[k, 2], li[k, 3] = -1, JUNK_ROW                        # the two unused header words
        x = rs.standard_normal(n_extra).astype(np.float32)
        lists[k, 4:4 + n_extra] = x
        want_x = want_x + x
        ra, rb = perm_a[ua:ua + na], perm_b[ub:ub + nb]
        ua, ub = ua + na, ub + nb
        ga = rs.standard_normal((na, d)).astype(np.float32)
        gb = rs.standard_normal(nb).astype(np.float32)
        li[k, o_ra:o_ra + na] = ra
        lists[k, o_ga:o_ga + na * d] = ga.reshape(-1)
        li[k, o_rb:o_rb + nb] = rb
        lists[k, o_vb:o_vb + nb] = gb
        want_a[ra] = ga
        want_b[rb] = gb
    assert ua <= total_a and ub <= max(total_b, 1)
    dense_a = Guarded((total_a, d), 7.0, dev)
    dense_b = Guarded((max(total_b, 1),), 7.0, dev)
    extra_out = Guarded((max(n_extra, 1),), 3.0, dev)
    ops.owner_scatter(dense_a.view, dense_b.view if cap_b else None, extra_out.view if n_extra else None,
                      torch.from_numpy(lists.reshape(-1)).to(dev), stride, world, cap_a, cap_b, d, n_extra, lib=lib)
    assert dense_a.intact() and dense_b.intact() and extra_out.intact()
    exact(test, workload, "dense A", dense_a.view, want_a)
    exact(test, workload, "dense B", dense_b.view, want_b)
    if n_extra:
        exact(test, workload, "extra floats summed in list order", extra_out.view, want_x)
    else:
        assert float(extra_out.view[0]) == 3.0


# (world, d, cap_a, cap_b, counts, n_extra, total_a, total_b)
OWNER_SCATTER_CORE = {
    "counts-below-capacity": (3, 8, 8, 4, [(5, 3), (0, 0), (8, 1)], 3, 29, 11),
    "no-family-b": (2, 8, 8, 0, [(3, 0), (7, 0)], 5, 17, 0),
    "small-cap-a": (3, 4, 4, 8, [(1, 8), (4, 0), (0, 5)], 0, 9, 31),
    "d64-extra4": (2, 64, 8, 4, [(7, 4), (8, 2)], 4, 40, 13),
}
OWNER_SCATTER_GPU_ONLY = {                                       # cap_a > 131072: the grid is capped at 2048 blocks, the loops stride
    "world2-d64-cap135168": (2, 64, 135168, 4096, [(135000, 4000), (70001, 100)], 3, 205003, 5000),
}
