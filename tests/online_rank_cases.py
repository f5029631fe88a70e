"""Checks of each request's full ranking on the device (``rat_rank_seg``; ``ops.rank_seg``; ``OnlineScorer.rank_requests`` /
``rank_candidates``), shared by tests/test_online_rank.py (CPU, host-emulation build) and tests/test_gpu_online_rank.py (MI355X).

The oracle is numpy's stable sort over the very vector the kernel saw — ``np.argsort(-y[h:e], kind="stable")`` per segment, its inverse
for ``rank``, ``y[h:e][order]`` for ``val``: positions and ranks must be equal as integers, values bit-equal (compared as integers, so
NaN and -0.0 count), so no tolerance enters a ranking check.  The only tolerance in this file is the eval forward's recorded margin
(``EVAL_GATE``), where a prediction vector is compared with one computed at another batch size.  Inputs, the recorder and the request
mixes are those of online_top_cases / online_requests_cases."""
import ctypes
import functools
import os
import re

import numpy as np
import torch

import online_requests_cases as rq
import online_top_cases as tc

EVAL_GATE = rq.EVAL_GATE
TOP_NS = (1, 5, 64)
OLD_GRAPHS = ("_graphs", "_bucket_graphs", "_rows_graphs", "_same_graphs", "_same_rows_graphs", "_top_graphs", "_top_cand_graphs")
NEW_GRAPHS = ("_rank_graphs", "_rank_cand_graphs")
_bits = tc._bits


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def reference_rank(y, segments):
    """numpy's stable sort, segment by segment -> (order int32 [B], val fp32 [B], rank int32 [B]); rows of no segment: -1 / 0.0 / -1"""
    B = len(y)
    order = np.full(B, -1, dtype=np.int32)
    val = np.zeros(B, dtype=np.float32)
    rank = np.full(B, -1, dtype=np.int32)
    for h, m in segments:
        seg = y[h:h + m]
        o = np.argsort(-seg, kind="stable")
        order[h:h + m] = o
        val[h:h + m] = seg[o]
        rank[h:h + m][o] = np.arange(m)
    return order, val, rank


def assert_rank_equal(got, want, what):
    order, val, rank = (torch.as_tensor(w) for w in want)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32, what
    assert tuple(got[0].shape) == tuple(got[1].shape) == tuple(got[2].shape) == tuple(order.shape), what
    assert torch.equal(got[2].cpu(), rank), (what, "rank")
    assert torch.equal(got[0].cpu(), order), (what, "order")
    assert torch.equal(_bits(got[1].cpu()), _bits(val)), (what, "val bits")


def assert_topn_is_prefix(top, ranked, segments, n, what):
    """(pos [B, n], val [B, n], lens [B]) at every head == the first min(n, len) entries of the full order"""
    pos, val, lens = (t.cpu() for t in top)
    order, rval = ranked[0].cpu(), ranked[1].cpu()
    for h, m in segments:
        k = min(n, m)
        assert int(lens[h]) == k, (what, h)
        assert torch.equal(pos[h, :k], order[h:h + k]), (what, h, "pos")
        assert torch.equal(_bits(val[h, :k]), _bits(rval[h:h + k])), (what, h, "val bits")


# ---- 1. rat_rank_seg == numpy's stable sort --------------------------------------------------------------------------------------------------
def kernel_constants():
    """(rows per work-group, rows per LDS tile) as csrc/rank.hip spells them; ops.RANK_ROWS / RANK_TILE quote them"""
    from rat_amd import ops
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "www24-rat_amd", "csrc", "rank.hip")).read()
    rows = int(re.search(r"constexpr int RK_THREADS = (\d+);", src).group(1))
    tile = int(re.search(r"constexpr int RK_TILE = (\d+);", src).group(1))
    assert (ops.RANK_ROWS, ops.RANK_TILE) == (rows, tile)
    return rows, tile


def _planted(y, lengths, seed):
    """into every segment of 6+ rows a NaN, both infinities and both zeros; a NaN as the last row of those of odd length"""
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    rng = np.random.default_rng(seed)
    for s, m in zip(starts, lengths):
        if m >= 6:
            rows = s + rng.choice(m, size=5, replace=False)
            y[rows] = [np.nan, np.inf, -np.inf, -0.0, 0.0]
            y[s + m - 1] = np.nan if m % 2 else y[s + m - 1]                   # a NaN as a segment's last row
    return y


@functools.lru_cache(maxsize=None)
def own_inputs(which):
    """-> (y, first_row, segments) from the new kernel's own constants.  "tile": segments of tile - 1, tile and tile + 1 rows (3 tiles
    = a whole number of work-groups), half a work-group of filler, a segment that starts in the MIDDLE of a work-group's rows and ends
    in the third work-group after it, and a last segment that ends exactly at B, which is no multiple of anything.  "long": a
    4097-row segment (one past graph_max_batch) between two short ones."""
    G, T = kernel_constants()
    if which == "tile":
        lengths = [T - 1, T, T + 1, G // 2, 3 * G, 77]
        start = 3 * T + G // 2
        assert (3 * T) % G == 0 and start % G == G // 2 and (start + 3 * G - 1) // G == start // G + 3
    else:
        lengths = [5, 4097, 3]
    first, starts = tc._first_row(lengths)
    B = len(first)
    rng = np.random.default_rng(tc.SEED + 300 + len(lengths))
    y = (np.round(rng.random(B) * 8) / 8).astype(np.float32)
    y = _planted(y, lengths, tc.SEED + 301)
    y.setflags(write=False), first.setflags(write=False)
    return y, first, tuple(zip(starts.tolist(), lengths))


def _check_one(device, lib, y, first, segments, what, ns=()):
    from rat_amd import ops
    ty, tf = torch.from_numpy(y.copy()).to(device), torch.from_numpy(first.copy()).to(device)
    got = ops.rank_seg(ty, tf, lib=lib)
    assert_rank_equal(got, reference_rank(y, segments), what)
    for n in ns:
        assert_topn_is_prefix(ops.topn_seg(ty, tf, n, lib=lib), got, segments, n, (what, n))
    assert torch.equal(_bits(ty.cpu()), _bits(torch.from_numpy(y.copy()))) and torch.equal(tf.cpu(), torch.from_numpy(first.copy()))
    return got


def check_rank_kernel(device, lib, set_name, variants=tc.VARIANTS, ns=tc.NS):
    """online_top_cases' inputs: segments of 1 .. 1025 rows, ties, NaN, infinities, both zeros, a trailing pad request, a first_row
    that clamps — and rat_topn_seg on the same y is the prefix of the order at every head"""
    tc.assert_regimes()
    for variant in variants:
        y, first, segments = tc.kernel_inputs(set_name, variant)
        _check_one(device, lib, y, first, segments, (set_name, variant), ns=ns)


def check_rank_own(device, lib, which, ns=(64,)):
    y, first, segments = own_inputs(which)
    assert segments[-1][0] + segments[-1][1] == len(y)
    assert any(np.isnan(y[h:h + m]).any() and len(np.unique(y[h:h + m])) < m for h, m in segments)
    _check_one(device, lib, y, first, segments, which, ns=ns)


# ---- 2. corrupt first_row addresses nothing outside the buffers (host-emulation build only) ------------------------------------------------
def members_of(first, B):
    """the contract's membership for ANY first_row, restated: -> the segments (head, length) whose rows are the members"""
    def f(b):
        return min(max(int(first[b]), 0), B - 1)
    out = []
    for h in range(B):
        if f(h) != h:
            continue
        e = h + 1
        while e < B and f(e) == h:
            e += 1
        out.append((h, e - h))
    covered = [b for h, m in out for b in range(h, h + m)]
    assert len(covered) == len(set(covered)), "segments overlap"
    return out


def check_corrupt(lib, guard=4096):
    """rat_rank_seg through the C ABI, every buffer between poisoned guard regions: first_row holds negative values, values >= B,
    non-monotone values, zeros only, heads that point forward.  The calls return normally, no guard byte changes, the inputs are only
    read, members get their segment's ranking and every other row the padding."""
    FILL = -99
    rng = np.random.default_rng(tc.SEED + 400)
    B = 300                                                                   # two work-groups

    def guarded(values, dtype):
        values = torch.as_tensor(np.ascontiguousarray(values), dtype=dtype).reshape(-1)
        whole = torch.full((values.numel() + 2 * guard,), FILL, dtype=dtype)
        whole[guard:guard + values.numel()] = values
        return whole, whole[guard:guard + values.numel()]

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    y = (np.round(rng.random(B) * 8) / 8).astype(np.float32)
    y[3], y[17], y[280] = np.nan, -np.inf, np.nan
    forward = np.arange(B) + 1                                                # every row names the row behind it; the last one clamps to itself
    blocks = np.repeat(np.arange(0, B, 50), 50)
    blocks[120:130] = 250                                                     # rows that name a head far ahead, inside another segment
    blocks[260] = 0                                                           # ... and one far behind: it ends the segment of 250 early
    lists = [np.arange(B) - 500, np.arange(B) + B, np.full(B, -2 ** 63), np.full(B, 2 ** 63 - 1), rng.integers(-10, B + 10, size=B),
             rng.permutation(B), np.arange(B)[::-1], np.zeros(B, dtype=np.int64), forward, blocks,
             np.array([0, 0, 0, 3, 3, 0, 0, 7, 2 ** 40, -2 ** 40] * (B // 10))]
    padded = 0
    for k, first in enumerate(lists):
        first = np.asarray(first, dtype=np.int64)
        bufs = dict(y=guarded(y, torch.float32), first=guarded(first, torch.int64), order=guarded(np.full(B, 7), torch.int32),
                    val=guarded(np.full(B, 7.0), torch.float32), rank=guarded(np.full(B, 7), torch.int32))
        y_bits, first_copy = _bits(bufs["y"][0]).clone(), bufs["first"][0].clone()
        lib.call("rat_rank_seg", p(bufs["y"][1]), p(bufs["first"][1]), B, p(bufs["order"][1]), p(bufs["val"][1]), p(bufs["rank"][1]), None)
        for name, (whole, _) in bufs.items():
            assert (whole[:guard] == FILL).all() and (whole[-guard:] == FILL).all(), (name, k)
        assert torch.equal(_bits(bufs["y"][0]), y_bits) and torch.equal(bufs["first"][0], first_copy), k
        segments = members_of(first, B)
        want = reference_rank(y, segments)
        padded += int((want[2] < 0).sum())
        assert_rank_equal((bufs["order"][1], bufs["val"][1], bufs["rank"][1]), want, ("corrupt first_row", k))
    assert padded > B, "the lists leave too few rows without a segment"


def check_abi_refusals(device, lib):
    """a null pointer, B < 1, B > 2^31 - 1: -1 and a message, nothing launched (the outputs keep their content)"""
    B = 4
    y = torch.zeros(B, dtype=torch.float32, device=device)
    first = torch.zeros(B, dtype=torch.int64, device=device)
    order = torch.full((B,), 7, dtype=torch.int32, device=device)
    val = torch.full((B,), 7.0, dtype=torch.float32, device=device)
    rank = torch.full((B,), 7, dtype=torch.int32, device=device)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    good = [p(y), p(first), B, p(order), p(val), p(rank), None]
    for slot, value in [(0, None), (1, None), (3, None), (4, None), (5, None), (2, 0), (2, -1), (2, 2 ** 31), (2, 2 ** 40)]:
        args = list(good)
        args[slot] = value
        assert lib.cdll.rat_rank_seg(*args) == -1 and "rat_rank_seg" in lib.last_error(), (slot, value)
    assert (order == 7).all() and (val == 7).all() and (rank == 7).all()
    assert lib.cdll.rat_rank_seg(*good) == 0 and order.cpu().tolist() == [0, 1, 2, 3] and rank.cpu().tolist() == [0, 1, 2, 3]


def check_ops_refusals(device, lib):
    """the wrapper checks shape, dtype, device and contiguity, and reads no contents"""
    import pytest
    from rat_amd import ops
    y = torch.zeros(6, dtype=torch.float32, device=device)
    first = torch.zeros(6, dtype=torch.int64, device=device)
    rec = tc.Recorder(lib)
    for exc, fn in ((TypeError, lambda: ops.rank_seg(y.double(), first, lib=rec)),
                    (TypeError, lambda: ops.rank_seg(y, first.int(), lib=rec)),
                    (ValueError, lambda: ops.rank_seg(y, first[:5], lib=rec)),
                    (ValueError, lambda: ops.rank_seg(y.reshape(2, 3), first, lib=rec)),
                    (ValueError, lambda: ops.rank_seg(y[:0], first[:0], lib=rec)),
                    (ValueError, lambda: ops.rank_seg(torch.zeros(12, dtype=torch.float32, device=device)[::2], first, lib=rec)),
                    (ValueError, lambda: ops.rank_seg(y, torch.zeros(12, dtype=torch.int64, device=device)[::2], lib=rec))):
        with pytest.raises(exc):
            fn()
        assert rec.take() == []
    if device != "cpu":
        with pytest.raises(ValueError, match="different devices"):
            ops.rank_seg(y, first.cpu(), lib=rec)
        assert rec.take() == []
    order, val, rank = ops.rank_seg(y, first, lib=rec)
    assert rec.take() == ["rat_rank_seg"] and order.cpu().tolist() == list(range(6)) and rank.cpu().tolist() == list(range(6))


# ---- 3. the scorer ----------------------------------------------------------------------------------------------------------------------
def _segments(off):
    return [(int(a), int(b - a)) for a, b in zip(off[:-1], off[1:])]


def assert_ranking(got, off, what, scores=True):
    """a Ranking of a scores=True call: numpy's ranking of that very y_pred, exactly"""
    from rat_amd.online import Ranking
    assert isinstance(got, Ranking) and got._fields == ("order", "val", "rank", "offsets", "y_pred"), what
    B = int(off[-1])
    assert np.array_equal(got.offsets.cpu().numpy(), np.asarray(off)) and got.offsets.dtype == torch.int64, what
    if not scores:
        assert got.y_pred is None, what
        return
    assert got.y_pred.dtype == torch.float32 and tuple(got.y_pred.shape) == (B,), what
    assert_rank_equal(got[:3], reference_rank(got.y_pred.cpu().numpy(), _segments(off)), what)


def assert_same_ranking(a, b, what):
    tc.assert_same_result(tuple(a[:3]) + ((a.y_pred,) if a.y_pred is not None else ()),
                          tuple(b[:3]) + ((b.y_pred,) if b.y_pred is not None else ()), what)


def _head(r, B):
    """the first B rows of a Ranking computed over more rows (a pad request spelled out), as a tuple"""
    return tuple(t[:B] for t in r[:3]) + (r.y_pred[:B],)


def check_rank_requests(name, gpu, lib, form, n_pool=14, ns=TOP_NS):
    scorer, case, _model, data, cols, _cfg, live = tc._scorer(name, gpu, lib, form, n_pool)
    device = scorer.device
    ties = False
    for tag, reqs in tc.request_mixes(case, data, live, cols).items():
        what = "%s %s" % (form, tag)
        cat, off = np.concatenate(reqs), rq._offsets(reqs)
        y_ref, off_ref = scorer.score_requests(reqs)
        got = scorer.rank_requests(reqs, scores=True)
        assert torch.equal(_bits(got.y_pred), _bits(y_ref)) and torch.equal(got.offsets, off_ref), what   # graph=False on both sides: the same launches
        assert_ranking(got, off, what)
        plain = scorer.rank_requests(reqs)
        assert_ranking(plain, off, what, scores=False)
        tc.assert_same_result(plain[:3], got[:3], what)
        pairs = [(cat, off), (torch.from_numpy(cat), off.tolist())]
        if gpu >= 0:
            pairs.append((torch.from_numpy(cat.astype(np.int32)).to(device), torch.from_numpy(off).to(device)))
        for pair in pairs:
            assert_same_ranking(scorer.rank_requests(pair, scores=True), got, what)
        for n in ns:                                                          # top_requests(n) is the prefix of the full order
            pos, val, lens = (t.cpu() for t in scorer.top_requests(reqs, n))
            for r, (h, m) in enumerate(_segments(off)):
                k = min(n, m)
                assert int(lens[r]) == k and torch.equal(pos[r, :k], got.order.cpu()[h:h + k]), (what, n, r)
                assert torch.equal(_bits(val[r, :k]), _bits(got.val.cpu()[h:h + k])), (what, n, r)
        y = y_ref.cpu().numpy()
        ties |= any(len(np.unique(y[a:b])) < b - a for a, b in zip(off[:-1], off[1:]))
    assert ties, "no request holds two equal predictions"


def check_rank_candidates(name, gpu, lib, form, n_pool=14):
    scorer, _case, _model, data, cols, _cfg, live = tc._scorer(name, gpu, lib, form, n_pool)
    device = scorer.device
    contexts, candidates, cand_cols, off, rows = tc.candidate_requests(data, live, cols)
    want = scorer.rank_requests((rows, off), scores=True)
    got = scorer.rank_candidates(contexts, candidates, cand_cols, off, scores=True)
    assert_same_ranking(got, want, form)
    assert_ranking(got, off, form)
    plain = scorer.rank_candidates(contexts, candidates, cand_cols, off)
    assert_ranking(plain, off, form, scores=False)
    tc.assert_same_result(plain[:3], want[:3], form)
    variants = [(torch.from_numpy(contexts), torch.from_numpy(candidates), list(cand_cols), off.tolist())]
    if gpu >= 0:
        variants.append((torch.from_numpy(contexts.astype(np.int32)).to(device), torch.from_numpy(candidates.astype(np.int32)).to(device),
                         np.asarray(cand_cols), torch.from_numpy(off).to(device)))
    for c, k, cc, o in variants:
        assert_same_ranking(scorer.rank_candidates(c, k, cc, o, scores=True), want, form)


# ---- 4. graphs (GPU only) ------------------------------------------------------------------------------------------------------------------
def check_rank_graphs(name, gpu, lib, form, train_step=True, n_pool=14):
    """After the warm-up the replayed rank_requests / rank_candidates equal a fresh graph=False scorer bit for bit — for a padded total
    the fresh scorer gets the same P rows, the pad request spelled out with OTHER rows, and the unpadded eager prediction lies within
    the eval forward's margin — for two request mixes and two padded totals of one bucket, before and after the pool and the weights
    change; the seven older dictionaries are untouched by the new calls, and the new ones by the old calls."""
    from rat_amd.data import DeviceBatch
    from rat_amd.online import OnlineScorer, _RankCandGraph, _RankGraph
    assert gpu >= 0
    scorer, case, model, data, cols, cfg, live = tc._scorer(name, gpu, lib, form, n_pool, graph=True)
    mixes = rq.make_mixes(case, data, live, cols)
    A, Bm = mixes["hit0"], mixes["miss0"]
    eight = [[A[0], A[1], A[2]], [Bm[0], Bm[1], Bm[2]]]                        # two mixes of 8 rows: 3 + 1 + 4, 4 + 1 + 3
    padded = [[A[2], A[3]], [Bm[0], Bm[1]]]                                    # two padded totals of the same bucket: 6 and 5 rows
    filler = live[-1, :-1]
    cur = [live.copy()]
    cand_cols = (cols[-1], cols[0]) if len(cols) > 1 else (cols[0],)

    def fresh():
        return OnlineScorer(model, cur[0], cfg, graph=False, lib=lib)

    def split(reqs):
        contexts = np.stack([r[0] for r in reqs])
        candidates = np.concatenate(reqs)[:, list(cand_cols)]
        rows = [np.repeat(r[:1], len(r), axis=0) for r in reqs]
        for r, full in zip(reqs, rows):
            full[:, list(cand_cols)] = r[:, list(cand_cols)]
        return contexts, candidates, rows

    def sizes(which):
        return {k: len(getattr(scorer, k)) for k in which}

    def check(reqs, tag):
        B = sum(len(r) for r in reqs)
        P = 1 << (B - 1).bit_length()
        off = rq._offsets(reqs)
        f = fresh()
        before = sizes(OLD_GRAPHS)
        got = scorer.rank_requests(reqs, scores=True)
        assert_ranking(got, off, tag)
        explicit, _ = rq._padded(reqs, P, filler)
        want = f.rank_requests(explicit, scores=True)
        tc.assert_same_result(tuple(got[:3]) + (got.y_pred,), _head(want, B), tag)
        worst = float((got.y_pred - f.score_requests(reqs)[0]).abs().max())
        print("replayed rank_requests vs unpadded eager score_requests, %s B=%d: worst |dy| = %.3g" % (tag, B, worst))
        assert worst <= EVAL_GATE, (tag, worst)
        contexts, candidates, rows = split(reqs)                               # the same requests as contexts + candidates
        gc_ = scorer.rank_candidates(contexts, candidates, cand_cols, off, scores=True)
        assert_ranking(gc_, off, tag)
        ec, ek, eo = contexts, candidates, off
        if P > B:
            ec = np.concatenate([contexts, filler[None]])
            ek = np.concatenate([candidates, np.repeat(filler[None, list(cand_cols)], P - B, axis=0)])
            eo = np.concatenate([off, [P]])
        tc.assert_same_result(tuple(gc_[:3]) + (gc_.y_pred,), _head(f.rank_candidates(ec, ek, cand_cols, eo, scores=True), B), tag)
        wr = f.rank_requests(rq._padded(rows, P, filler)[0], scores=True)     # ... and against the rows built on the host
        tc.assert_same_result(tuple(gc_[:3]) + (gc_.y_pred,), _head(wr, B), tag)
        assert sizes(OLD_GRAPHS) == before, "a fully ranked call touched another call's graphs"
        return got

    def graphs(which):
        return [e[1] for e in getattr(scorer, which).values()]

    for k in range(scorer.graph_warmup):
        check(eight[k], "warm-up %d" % k)
        assert not any(isinstance(g, (_RankGraph, _RankCandGraph)) for g in graphs("_rank_graphs") + graphs("_rank_cand_graphs"))
    first = check(eight[0], "capture")
    assert [type(g) for g in graphs("_rank_graphs")] == [_RankGraph] and [type(g) for g in graphs("_rank_cand_graphs")] == [_RankCandGraph]
    captured = graphs("_rank_graphs") + graphs("_rank_cand_graphs")
    for k, reqs in enumerate(eight + padded):
        check(reqs, "bucket 8, mix %d" % k)
    assert_same_ranking(check(eight[0], "again"), first, "again")
    assert all(a is b for a, b in zip(graphs("_rank_graphs") + graphs("_rank_cand_graphs"), captured)) and len(captured) == 2
    assert sizes(OLD_GRAPHS) == dict.fromkeys(OLD_GRAPHS, 0)
    # the older calls beside them: their own graphs, and ours are not touched
    ids = torch.from_numpy(np.concatenate(eight[0]).astype(np.int32)).to(scorer.device)
    contexts, candidates, _rows = split(eight[0])
    for _ in range(scorer.graph_warmup + 1):
        scorer.score(ids)
        scorer.score_requests(eight[0])
        scorer.top_requests(eight[0], 3)
        scorer.top_candidates(contexts, candidates, cand_cols, rq._offsets(eight[0]), 3)
    assert sizes(("_graphs", "_bucket_graphs", "_top_graphs", "_top_cand_graphs")) == dict(_graphs=1, _bucket_graphs=1, _top_graphs=1, _top_cand_graphs=1)
    assert sizes(NEW_GRAPHS) == dict(_rank_graphs=1, _rank_cand_graphs=1)
    assert all(a is b for a, b in zip(graphs("_rank_graphs") + graphs("_rank_cand_graphs"), captured))
    # other columns: another entry of _rank_cand_graphs only
    scorer.rank_candidates(contexts, candidates[:, ::-1].copy(), cand_cols[::-1], rq._offsets(eight[0]))
    assert sizes(NEW_GRAPHS) == dict(_rank_graphs=1, _rank_cand_graphs=2 if len(cand_cols) > 1 else 1)
    # the pool and the weights change under the captured graphs
    n_ids = live.shape[1] - 1
    steps = ["relabel"] + (["append"] if form != "immutable" else []) + (["evict", "delete"] if form == "window" else []) + ["train"]
    for step in steps:
        y_old = scorer.rank_requests(eight[1], scores=True).y_pred
        _v, i, _l = scorer.index.retrieve(np.concatenate(eight[1]), rq._offsets(eight[1]))
        hit = np.unique(i.cpu().numpy())
        hit = hit[hit >= 0]
        if step == "relabel":
            keys = cur[0][hit][:, :-1].astype(np.int64)
            rows = (cur[0][:, None, :-1].astype(np.int64) == keys[None]).all(axis=2).any(axis=1)
            new = 1.0 - float(np.round(cur[0][rows, -1].mean()))
            scorer.relabel_where(list(range(n_ids)), keys, new)
            cur[0] = cur[0].copy()
            cur[0][rows, -1] = new
        elif step == "append":
            rows = data[-3:].copy()
            rows[:, cols] = np.concatenate(eight[1])[:3][:, cols]               # rows the requests will retrieve
            scorer.append(rows)
            cur[0] = np.concatenate([cur[0], rows])[-rq.CAPACITY:] if form == "window" else np.concatenate([cur[0], rows])
        elif step == "evict":
            m = min(int(hit.min()) + 1, 4)
            scorer.evict(m)
            cur[0] = cur[0][m:]
        elif step == "delete":
            scorer.delete(hit[:2])
            cur[0] = np.delete(cur[0], hit[:2], axis=0)
        else:
            if not train_step:
                continue
            model.train()
            model.train_step(DeviceBatch(*scorer._assemble(ids)))
            model.eval()
        for reqs in (eight[1], padded[0]):
            check(reqs, "after %s" % step)
        assert all(a is b for a, b in zip(graphs("_rank_graphs"), captured[:1])) and graphs("_rank_cand_graphs")[0] is captured[1], \
            "%s invalidated a captured chain" % step
        assert not torch.equal(scorer.rank_requests(eight[1], scores=True).y_pred, y_old), "%s changed no prediction" % step


# ---- 5. refusals and the launch chain ------------------------------------------------------------------------------------------------------
def check_refusals(gpu, lib):
    """every refusal is raised before any entry point of the library is reached"""
    import pytest
    from rat_amd.online import OnlineScorer
    _case, model, data, pool, cols, cfg = rq._setup("tiny_seq_bn", gpu)
    rec = tc.Recorder(lib)
    scorer = OnlineScorer(model, pool[:14], cfg, graph=False, lib=rec)
    rec.take()
    ids = np.ascontiguousarray(data[:6, :-1])
    L = ids.shape[1]
    reqs = [ids[:2], ids[2:]]
    cc = [cols[-1], [c for c in range(L) if c != cols[-1]][0]]
    contexts, candidates, off = ids[:2], np.ascontiguousarray(ids[:, cc]), [0, 2, 6]

    def refused(exc, word, fn):
        with pytest.raises(exc, match=word):
            fn()
        assert rec.take() == [], "a refused call reached the library"
    for bad, word in (([], "non-empty"), ([cc[0], cc[0]], "repeated"), ([0.0, 1.0], "integer"), ([cc[0], L], "outside"), ([-1, cc[0]], "outside"),
                      ([[0, 1]], "1-D")):
        refused(ValueError, word, lambda: scorer.rank_candidates(contexts, candidates, bad, off))
    refused(ValueError, "candidates have", lambda: scorer.rank_candidates(contexts, candidates[:, :1], cc, off))
    refused(ValueError, "one encoded row per request", lambda: scorer.rank_candidates(ids[:3], candidates, cc, off))
    refused(ValueError, "one encoded row per request", lambda: scorer.rank_candidates(ids[:1], candidates, cc, off))
    refused(ValueError, "columns", lambda: scorer.rank_candidates(contexts[:, :-1], candidates, cc, off))
    refused(ValueError, "end at", lambda: scorer.rank_candidates(contexts, candidates, cc, [0, 2, 5]))
    refused(ValueError, "empty request", lambda: scorer.rank_candidates(contexts, candidates, cc, [0, 6, 6]))
    refused(ValueError, "start at 0", lambda: scorer.rank_candidates(contexts, candidates, cc, [1, 2, 6]))
    refused(ValueError, "empty request", lambda: scorer.rank_requests([]))
    refused(ValueError, "columns", lambda: scorer.rank_requests([ids[:2], ids[2:, :-1]]))
    refused(ValueError, "ascending", lambda: scorer.rank_requests((ids, [0, 4, 2, 6])))
    refused(ValueError, "integers", lambda: scorer.rank_requests((ids, [0.0, 2.0, 6.0])))
    refused(TypeError, "same", lambda: scorer.rank_requests(reqs, same=[cols[0]]))               # no same= / before= / n on these calls
    refused(TypeError, "before", lambda: scorer.rank_candidates(contexts, candidates, cc, off, before=[0] * 6))
    refused(TypeError, "n", lambda: scorer.rank_requests(reqs, n=65))
    model.train()
    refused(RuntimeError, r"OnlineScorer\.rank_requests needs the model in eval mode \(model\.eval\(\)\)", lambda: scorer.rank_requests(reqs))
    refused(RuntimeError, r"OnlineScorer\.rank_candidates needs the model in eval mode \(model\.eval\(\)\)",
            lambda: scorer.rank_candidates(contexts, candidates, cc, off))
    model.eval()
    got = scorer.rank_requests(reqs)                                               # and good ones go through
    assert tuple(got.order.shape) == (6,) and sorted(got.order.cpu().tolist()[:2]) == [0, 1] and rec.take()
    got = scorer.rank_candidates(contexts, candidates, cc, off)
    assert tuple(got.order.shape) == (6,) and sorted(got.rank.cpu().tolist()[2:]) == [0, 1, 2, 3] and rec.take()


def check_launch_chain(gpu, lib, form, n_pool=14):
    """rank_requests reaches score_requests' entry points in score_requests' order, then rat_rank_seg; rank_candidates the same behind
    rat_candidates_expand.  The reference list is recorded from score_requests itself, on the same scorer."""
    from rat_amd.online import OnlineScorer
    _case, model, data, pool, cols, cfg = rq._setup("tiny_seq_bn", gpu, n_pool=n_pool)
    first, kw, later, live = rq._form(form, pool, n_pool)
    rec = tc.Recorder(lib)
    scorer = OnlineScorer(model, first, cfg, graph=False, lib=rec, **kw)
    if later is not None:
        scorer.append(later)
    rec.take()
    contexts, candidates, cand_cols, off, rows = tc.candidate_requests(data, live, cols, sizes=(3, 1, 4))
    scorer.score_requests((rows, off))
    chain = rec.take()
    assert len(chain) >= 3 and not any(name in ("rat_rank_seg", "rat_topn_seg", "rat_candidates_expand") for name in chain)
    scorer.rank_requests((rows, off))
    assert rec.take() == chain + ["rat_rank_seg"]
    scorer.rank_requests((rows, off), scores=True)
    assert rec.take() == chain + ["rat_rank_seg"]
    scorer.rank_candidates(contexts, candidates, cand_cols, off)
    assert rec.take() == ["rat_candidates_expand"] + chain + ["rat_rank_seg"]
    scorer.top_requests((rows, off), 3)                                            # the page's chain is what it was
    assert rec.take() == chain + ["rat_topn_seg"]
