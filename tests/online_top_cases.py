"""Checks of each request's top-n candidates on the device (``rat_topn_seg``, ``rat_candidates_expand``; ``ops.topn_seg``,
``ops.candidates_expand``; ``OnlineScorer.top_requests`` / ``top_candidates`` / ``expand_candidates``), shared by
tests/test_online_top.py (CPU, host-emulation build) and tests/test_gpu_online_top.py (MI355X).

The oracle of the ranking is numpy's stable sort, ``np.argsort(-y_request, kind="stable")[:n]``, over the very vector the kernel saw:
positions and counts must be equal, values bit-equal (compared as integers, so NaN and -0.0 count), so no tolerance enters a ranking
check.  The oracle of the expansion is the same rows built on the host.  The only tolerance in this file is the eval forward's
recorded margin (``EVAL_GATE``), where a prediction vector is compared with one computed at another batch size."""
import ctypes
import functools

import numpy as np
import torch

import online_requests_cases as rq

EVAL_GATE = rq.EVAL_GATE
NS = (1, 5, 32, 64)
# n - 1 / n / n + 1 for every n above, a wave (64), a work-group (256), and a segment longer than the 1024 rows whose keys the kernel
# stages in LDS.  The order is part of the cases: the 1025-row segment is last, so it ends exactly at B.
LENGTHS = (1, 2, 4, 5, 6, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025)
SETS = ("distinct", "eighths", "constant", "special")
VARIANTS = ("plain", "pad", "one")
PAD_ROWS = 13
SEED = 20241
POISON = -777


def _first_row(lengths):
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    return np.repeat(starts, lengths), starts


def _specials(starts, lengths):
    """(row, value) planted into set "special": a NaN that is a whole segment (its first AND last row), NaNs inside short segments and
    in the long one, infinities and both zeros — among them a segment's first and its last row"""
    seg = {n: (int(s), int(n)) for s, n in zip(starts, lengths)}
    out = [(seg[1][0], np.nan),                                                # the 1-row segment
           (seg[4][0] + 1, np.nan), (seg[4][0], -0.0), (seg[4][0] + 3, 0.0),  # NaN inside the top 5 of a 4-row segment; zeros at both ends
           (seg[31][0] + 30, np.nan), (seg[31][0], np.inf),                   # a segment's last row / first row
           (seg[63][0] + 7, np.nan), (seg[63][0] + 8, np.nan), (seg[63][0] + 62, -np.inf),
           (seg[257][0] + 100, -np.inf), (seg[257][0] + 101, np.inf), (seg[257][0] + 102, -0.0), (seg[257][0] + 256, 0.0),
           (seg[1025][0], np.nan), (seg[1025][0] + 1024, np.nan), (seg[1025][0] + 500, np.inf), (seg[1025][0] + 501, np.inf)]
    return out


@functools.lru_cache(maxsize=None)
def kernel_inputs(set_name, variant):
    """-> (y fp32 [B], first_row int64 [B], the segments as (start, length) pairs), numpy, from a fixed seed"""
    lengths = list(LENGTHS)
    if variant == "pad":
        lengths = lengths + [PAD_ROWS]                                         # a trailing pad request, as score_requests appends it
    elif variant == "one":
        lengths = [1]
    first, starts = _first_row(lengths)
    B = len(first)
    rng = np.random.default_rng(SEED + SETS.index(set_name))
    if set_name == "distinct":
        y = rng.standard_normal(B).astype(np.float32)
        assert len(np.unique(y)) == B
    elif set_name == "constant":
        y = np.full(B, 0.5, dtype=np.float32)
    else:
        y = (np.round(rng.random(B) * 8) / 8).astype(np.float32)              # 9 values: ties in every segment longer than 9
        if set_name == "special" and variant != "one":
            for row, v in _specials(starts, lengths):
                y[row] = v
        elif set_name == "special":
            y[0] = np.nan
    first = first.copy()
    if variant != "plain":
        first[0] = -3                                                          # clamps to row 0: still the head of the first segment
    y.setflags(write=False), first.setflags(write=False)
    return y, first, tuple(zip(starts.tolist(), lengths))


def reference_topn(y, segments, n):
    """numpy's stable sort, segment by segment -> (pos int32 [B, n], val fp32 [B, n], lens int32 [B]) with the kernel's padding"""
    B = len(y)
    pos = np.full((B, n), -1, dtype=np.int32)
    val = np.zeros((B, n), dtype=np.float32)
    lens = np.zeros(B, dtype=np.int32)
    for h, m in segments:
        seg = y[h:h + m]
        order = np.argsort(-seg, kind="stable")[:n]
        pos[h, :len(order)] = order
        val[h, :len(order)] = seg[order]
        lens[h] = len(order)
    return pos, val, lens


@functools.lru_cache(maxsize=None)
def kernel_reference(set_name, variant, n):
    y, _first, segments = kernel_inputs(set_name, variant)
    return reference_topn(y, segments, n)


def assert_regimes():
    """what the inputs above reach, established in numpy: for every n a tie that straddles the cut and a cut between different values,
    and a NaN inside the top n of a short segment and outside it in a long one"""
    for n in NS:
        straddle = differ = nan_in = nan_out = False
        for set_name in SETS:
            y, _f, segments = kernel_inputs(set_name, "plain")
            for h, m in segments:
                seg = y[h:h + m]
                order = np.argsort(-seg, kind="stable")
                if m > n:
                    a, b = seg[order[n - 1]], seg[order[n]]
                    straddle |= bool(a == b)
                    differ |= bool(a != b and not np.isnan(a) and not np.isnan(b))
                top = seg[order[:n]]
                if np.isnan(seg).any():
                    nan_in |= bool(np.isnan(top).any() and m <= 64)
                    nan_out |= bool(not np.isnan(top).any() and m > 64)
        assert straddle and differ and nan_in and nan_out, (n, straddle, differ, nan_in, nan_out)
    y, _f, segments = kernel_inputs("special", "plain")
    zeros = y[(y == 0) & np.signbit(y)]
    assert len(zeros) and np.isposinf(y).any() and np.isneginf(y).any()
    assert any(np.isnan(y[h]) for h, _m in segments) and any(np.isnan(y[h + m - 1]) for h, m in segments)


def _bits(t):
    return t.contiguous().view(torch.int32)


def assert_topn_equal(got, want, what):
    pos, val, lens = (torch.as_tensor(w) for w in want)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32, what
    assert torch.equal(got[2].cpu(), lens), (what, "lens")
    assert torch.equal(got[0].cpu(), pos), (what, "pos")
    assert torch.equal(_bits(got[1].cpu()), _bits(val)), (what, "val bits")


# ---- 1. rat_topn_seg == numpy's stable sort ----------------------------------------------------------------------------------------------
def check_topn_kernel(device, lib, set_name, ns=NS, variants=VARIANTS):
    from rat_amd import ops
    assert_regimes()
    for variant in variants:
        y, first, _segments = kernel_inputs(set_name, variant)
        ty, tf = torch.from_numpy(y.copy()).to(device), torch.from_numpy(first.copy()).to(device)
        for n in ns:
            got = ops.topn_seg(ty, tf, n, lib=lib)
            assert tuple(got[0].shape) == (len(y), n) and tuple(got[1].shape) == (len(y), n) and tuple(got[2].shape) == (len(y),)
            assert_topn_equal(got, kernel_reference(set_name, variant, n), (set_name, variant, n))
        assert torch.equal(_bits(ty.cpu()), _bits(torch.from_numpy(y.copy()))) and torch.equal(tf.cpu(), torch.from_numpy(first.copy()))


# ---- 2. rat_candidates_expand == the rows built in numpy -------------------------------------------------------------------------------------
EXPAND_SHAPES = ((7, (4,)), (7, (5, 0, 3)), (7, (6, 2, 0, 5, 1, 4, 3)),       # L = 7: word by word; W = 1, 3 and every column, unsorted
                 (8, (5, 0, 3)), (8, (7, 6, 5, 4, 3, 2, 1, 0)))                # L = 8: rows move as 16-byte words


def reference_expand(ctx, cand, cols, first, B):
    f = np.clip(first, 0, B - 1)
    out = ctx[f].copy()
    for w, c in enumerate(cols):
        if 0 <= c < ctx.shape[1]:
            out[:, c] = cand[:, w]
    return out


def check_expand_kernel(device, lib, shapes=EXPAND_SHAPES):
    from rat_amd import ops
    _y, first, segments = kernel_inputs("distinct", "pad")
    B = len(first)
    heads = np.array([h for h, _m in segments])
    rng = np.random.default_rng(SEED + 100)
    for L, cols in shapes:
        ctx = np.full((B, L), POISON, dtype=np.int32)                         # rows that open no request: never read
        ctx[heads] = rng.integers(0, 1000, size=(len(heads), L))
        cand = rng.integers(1000, 2000, size=(B, len(cols))).astype(np.int32)
        want = reference_expand(ctx, cand, cols, first, B)
        assert (want != POISON).all()
        t = [torch.from_numpy(a.copy()).to(device) for a in (ctx, cand, np.asarray(cols, dtype=np.int32), first)]
        got = ops.candidates_expand(*t, lib=lib)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, L)
        assert np.array_equal(got.cpu().numpy(), want), (L, cols)
        assert not (got == POISON).any()
        assert np.array_equal(t[0].cpu().numpy(), ctx) and np.array_equal(t[1].cpu().numpy(), cand)


# ---- 3. corrupt first_row / cols address nothing outside the buffers (host-emulation build only) ------------------------------------------
def _segments_of(first, B):
    """the contract's segments for ANY first_row: heads are the rows h with clamp(first[h]) == h"""
    f = np.clip(np.asarray(first, dtype=object), 0, B - 1).astype(np.int64)
    out = []
    for h in range(B):
        if f[h] == h:
            e = h + 1
            while e < B and f[e] == h:
                e += 1
            out.append((h, e - h))
    return out


def check_corrupt(lib, guard=4096):
    """both kernels through the C ABI, every buffer between guard regions: first_row holds negative values, values >= B, non-monotone
    values or zeros only, cols entries outside [0, L).  The calls return normally, no guard byte changes, the inputs are only read, and
    the outputs are what the contract says for the clamped first_row."""
    FILL = -99
    rng = np.random.default_rng(SEED + 200)
    B, n, L = 40, 5, 8

    def guarded(values, dtype):
        values = torch.as_tensor(np.ascontiguousarray(values), dtype=dtype).reshape(-1)
        whole = torch.full((values.numel() + 2 * guard,), FILL, dtype=dtype)
        whole[guard:guard + values.numel()] = values
        return whole, whole[guard:guard + values.numel()]

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def intact(bufs, read_only, what):
        for name, (whole, _) in bufs.items():
            assert (whole[:guard] == FILL).all() and (whole[-guard:] == FILL).all(), (name, what)
        assert all(torch.equal(_bits(bufs[b][0]) if bufs[b][0].dtype == torch.float32 else bufs[b][0], v) for b, v in read_only.items()), what
    y = (np.round(rng.random(B) * 8) / 8).astype(np.float32)
    y[3], y[17] = np.nan, -np.inf
    lists = [np.arange(B) - 50, np.arange(B) + B, np.full(B, -2 ** 63), np.full(B, 2 ** 63 - 1),
             rng.integers(-10, B + 10, size=B), rng.permutation(B), np.arange(B)[::-1], np.zeros(B, dtype=np.int64),
             np.array([0, 0, 0, 3, 3, 0, 0, 7, 2 ** 40, -2 ** 40] * 4)]
    for k, first in enumerate(lists):
        first = np.asarray(first, dtype=np.int64)
        bufs = dict(y=guarded(y, torch.float32), first=guarded(first, torch.int64), pos=guarded(np.full(B * n, 7), torch.int32),
                    val=guarded(np.full(B * n, 7.0), torch.float32), lens=guarded(np.full(B, 7), torch.int32))
        read_only = dict(y=_bits(bufs["y"][0]).clone(), first=bufs["first"][0].clone())
        lib.call("rat_topn_seg", p(bufs["y"][1]), p(bufs["first"][1]), B, n, p(bufs["pos"][1]), p(bufs["val"][1]), p(bufs["lens"][1]), None)
        intact(bufs, read_only, ("topn", k))
        got = (bufs["pos"][1].reshape(B, n), bufs["val"][1].reshape(B, n), bufs["lens"][1])
        assert_topn_equal(got, reference_topn(y, _segments_of(first, B), n), ("corrupt first_row", k))
        for cols in ([5, 0, 3], [-1, 3, L, 10 ** 6, -2 ** 31, 2 ** 31 - 1, 6]):
            W = len(cols)
            ctx = rng.integers(0, 1000, size=(B, L)).astype(np.int32)
            cand = rng.integers(1000, 2000, size=(B, W)).astype(np.int32)
            for width in (L, L - 1):                                           # 16-byte words, and word by word
                ebufs = dict(ctx=guarded(ctx[:, :width], torch.int32), cand=guarded(cand, torch.int32), cols=guarded(cols, torch.int32),
                             first=guarded(first, torch.int64), out=guarded(np.full(B * width, 7), torch.int32))
                ro = {b: ebufs[b][0].clone() for b in ("ctx", "cand", "cols", "first")}
                lib.call("rat_candidates_expand", p(ebufs["ctx"][1]), p(ebufs["cand"][1]), p(ebufs["cols"][1]), p(ebufs["first"][1]), B,
                         width, W, p(ebufs["out"][1]), None)
                intact(ebufs, ro, ("expand", k, cols, width))
                want = reference_expand(np.ascontiguousarray(ctx[:, :width]), cand, cols, first, B)
                assert np.array_equal(ebufs["out"][1].reshape(B, width).numpy(), want), ("expand", k, cols, width)


def check_abi_refusals(device, lib):
    """a null pointer, B < 1, n / L / W out of range: -1 and a message, nothing launched (the outputs keep their content)"""
    B, n = 4, 3
    y = torch.zeros(B, dtype=torch.float32, device=device)
    first = torch.zeros(B, dtype=torch.int64, device=device)
    pos = torch.full((B, n), 7, dtype=torch.int32, device=device)
    val = torch.full((B, n), 7.0, dtype=torch.float32, device=device)
    lens = torch.full((B,), 7, dtype=torch.int32, device=device)
    ids = torch.full((B, 4), 7, dtype=torch.int32, device=device)

    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None
    good = [p(y), p(first), B, n, p(pos), p(val), p(lens), None]
    bad = [(0, None), (1, None), (4, None), (5, None), (6, None), (2, 0), (2, -1), (2, 2 ** 31), (3, 0), (3, 65), (3, -1)]
    for slot, value in bad:
        args = list(good)
        args[slot] = value
        assert lib.cdll.rat_topn_seg(*args) == -1 and "rat_topn_seg" in lib.last_error(), (slot, value)
    good = [p(ids), p(ids), p(ids), p(first), B, 4, 4, p(ids), None]
    bad = [(0, None), (1, None), (2, None), (3, None), (7, None), (4, 0), (4, -5), (5, 0), (5, 8193), (6, 0), (6, 8193)]
    for slot, value in bad:
        args = list(good)
        args[slot] = value
        assert lib.cdll.rat_candidates_expand(*args) == -1 and "rat_candidates_expand" in lib.last_error(), (slot, value)
    assert (pos == 7).all() and (val == 7).all() and (lens == 7).all() and (ids == 7).all()


# ---- 4. the scorer ----------------------------------------------------------------------------------------------------------------------
TOP_NS = (1, 3, 8)
BIG = 40


def _scorer(name, gpu, lib, form, n_pool, graph=False):
    from rat_amd.online import OnlineScorer
    case, model, data, pool, cols, cfg = rq._setup(name, gpu, n_pool=n_pool)
    first, kw, later, live = rq._form(form, pool, n_pool)
    scorer = OnlineScorer(model, first, cfg, graph=graph, lib=lib, **kw)
    if later is not None:
        scorer.append(later)
    if form == "window":
        assert int(scorer.index.count[1]) + len(live) > rq.CAPACITY, "the window does not wrap"
    return scorer, case, model, data, cols, cfg, live


def big_request(data, live, cols, m=BIG):
    """one request of m candidates: the query rows over and over with pool ids in the used columns — rows repeat, so predictions tie"""
    rows = data[np.arange(m) % 5, :-1].copy()
    rows[:, cols] = live[np.arange(m) % 10 % len(live)][:, cols]
    return rows


def request_mixes(case, data, live, cols):
    mixes = rq.make_mixes(case, data, live, cols)                              # sizes (3, 1, 4, 2, 6, 1), in two orders
    big = big_request(data, live, cols)
    return dict(hit0=mixes["hit0"] + [big], miss0=[big] + mixes["miss0"])


def numpy_top(y, off, n):
    """the oracle over the vector the kernel saw -> (pos [R, n], val [R, n], lens [R])"""
    segments = [(int(a), int(b - a)) for a, b in zip(off[:-1], off[1:])]
    pos, val, lens = reference_topn(y, segments, n)
    heads = np.asarray(off[:-1])
    return pos[heads], val[heads], lens[heads]


def assert_ranked(got, off, n, what):
    """(pos, val, lens, y_pred) of a scores=True call: the ranking is numpy's over that y_pred, exactly"""
    pos, val, lens, y = got
    R = len(off) - 1
    assert tuple(pos.shape) == (R, n) and tuple(val.shape) == (R, n) and tuple(lens.shape) == (R,) and tuple(y.shape) == (int(off[-1]),), what
    assert y.dtype == torch.float32
    assert_topn_equal((pos, val, lens), numpy_top(y.cpu().numpy(), np.asarray(off), n), what)
    assert lens.cpu().tolist() == [min(n, int(m)) for m in np.diff(off)], what


def assert_same_result(a, b, what):
    assert len(a) == len(b), what
    for k, (x, z) in enumerate(zip(a, b)):
        assert x.dtype == z.dtype and torch.equal(_bits(x.cpu()), _bits(z.cpu())), (what, k)


def check_top_requests(name, gpu, lib, form, n_pool=14, ns=TOP_NS):
    scorer, case, _model, data, cols, _cfg, live = _scorer(name, gpu, lib, form, n_pool)
    device = scorer.device
    ties = False
    for tag, reqs in request_mixes(case, data, live, cols).items():
        cat, off = np.concatenate(reqs), rq._offsets(reqs)
        y_ref, _off = scorer.score_requests(reqs)
        for n in ns:
            what = "%s %s n=%d" % (form, tag, n)
            got = scorer.top_requests(reqs, n, scores=True)
            assert torch.equal(_bits(got[3]), _bits(y_ref)), what                 # graph=False on both sides: the same launches
            assert float((got[3] - y_ref).abs().max()) <= EVAL_GATE
            assert_ranked(got, off, n, what)
            assert_same_result(scorer.top_requests(reqs, n), got[:3], what)
            pairs = [(cat, off), (torch.from_numpy(cat), off.tolist())]
            if gpu >= 0:
                pairs.append((torch.from_numpy(cat.astype(np.int32)).to(device), torch.from_numpy(off).to(device)))
            for pair in pairs:
                assert_same_result(scorer.top_requests(pair, n, scores=True), got, what)
        y = y_ref.cpu().numpy()
        ties |= any(len(np.unique(y[a:b])) < b - a for a, b in zip(off[:-1], off[1:]))
    assert ties, "no request holds two equal predictions"
    one = scorer.top_requests([reqs[0][:2]], 64, scores=True)                    # n beyond every request: lens carries the count
    assert_ranked(one, np.array([0, 2]), 64, "n = 64")


def candidate_requests(data, live, cols, sizes=(3, 1, 4, 2, 6, 1, BIG)):
    """-> (contexts [R, L], candidates [C, W], the candidate columns — unsorted —, offsets, the full rows built on the host)"""
    cand_cols = (cols[-1], cols[0]) if len(cols) > 1 else (cols[0],)
    R, C = len(sizes), sum(sizes)
    contexts = data[:R, :-1].copy()
    contexts[:, cols] = live[np.arange(R) % len(live)][:, cols]
    contexts[:, list(cand_cols)] = POISON                                      # the contexts' own entries in these columns are ignored
    pick = (5 * np.arange(C)) % 9 % len(live)                                  # repeats inside the big request: ties
    candidates = live[pick][:, list(cand_cols)].copy()
    off = rq._offsets([np.zeros((m, 1)) for m in sizes])
    rows = np.repeat(contexts, sizes, axis=0)
    rows[:, list(cand_cols)] = candidates
    assert (rows != POISON).all()
    return contexts, candidates, cand_cols, off, rows


def check_top_candidates(name, gpu, lib, form, n_pool=14, ns=TOP_NS):
    scorer, _case, _model, data, cols, _cfg, live = _scorer(name, gpu, lib, form, n_pool)
    device = scorer.device
    contexts, candidates, cand_cols, off, rows = candidate_requests(data, live, cols)
    assert list(cand_cols) != sorted(cand_cols) or len(cand_cols) == 1
    ids = scorer.expand_candidates(contexts, candidates, cand_cols, off)
    assert ids.dtype == torch.int32 and np.array_equal(ids.cpu().numpy(), rows.astype(np.int32))
    for n in ns:
        what = "%s n=%d" % (form, n)
        want = scorer.top_requests((rows, off), n, scores=True)
        got = scorer.top_candidates(contexts, candidates, cand_cols, off, n, scores=True)
        assert_same_result(got, want, what)
        assert_ranked(got, off, n, what)
        assert_same_result(scorer.top_candidates(contexts, candidates, cand_cols, off, n), want[:3], what)
        variants = [(torch.from_numpy(contexts), torch.from_numpy(candidates), list(cand_cols), off.tolist())]
        if gpu >= 0:
            variants.append((torch.from_numpy(contexts.astype(np.int32)).to(device), torch.from_numpy(candidates.astype(np.int32)).to(device),
                             np.asarray(cand_cols), torch.from_numpy(off).to(device)))
        for c, k, cc, o in variants:
            assert_same_result(scorer.top_candidates(c, k, cc, o, n, scores=True), want, what)
            assert torch.equal(scorer.expand_candidates(c, k, cc, o), ids), what


# ---- 5. graphs (GPU only) ------------------------------------------------------------------------------------------------------------------
def check_top_graphs(name, gpu, lib, form, n=3, train_step=True, n_pool=14):
    """After the warm-up the replayed top_requests / top_candidates equal a fresh graph=False scorer bit for bit — for a padded total
    the fresh scorer gets the same P rows, the pad request spelled out with OTHER rows (whose content is thereby shown not to matter),
    and the unpadded eager prediction lies within the eval forward's margin — for two request mixes and two padded totals of one
    bucket, before and after the pool and the weights change; no dictionary of another call is touched."""
    from rat_amd.data import DeviceBatch
    from rat_amd.online import OnlineScorer, _TopCandGraph, _TopGraph
    assert gpu >= 0
    scorer, case, model, data, cols, cfg, live = _scorer(name, gpu, lib, form, n_pool, graph=True)
    mixes = rq.make_mixes(case, data, live, cols)
    A, Bm = mixes["hit0"], mixes["miss0"]
    eight = [[A[0], A[1], A[2]], [Bm[0], Bm[1], Bm[2]]]                        # two mixes of 8 rows: 3 + 1 + 4, 4 + 1 + 3
    padded = [[A[2], A[3]], [Bm[0], Bm[1]]]                                    # two padded totals of the same bucket: 6 and 5 rows
    filler = live[-1, :-1]
    cur = [live.copy()]
    cand_cols = (cols[-1], cols[0]) if len(cols) > 1 else (cols[0],)
    old = ("_graphs", "_bucket_graphs", "_rows_graphs", "_same_graphs", "_same_rows_graphs")

    def fresh():
        return OnlineScorer(model, cur[0], cfg, graph=False, lib=lib)

    def split(reqs):
        """the requests as contexts + candidate columns: request r's context is its first row"""
        contexts = np.stack([r[0] for r in reqs])
        candidates = np.concatenate(reqs)[:, list(cand_cols)]
        rows = [np.repeat(r[:1], len(r), axis=0) for r in reqs]
        for r, full in zip(reqs, rows):
            full[:, list(cand_cols)] = r[:, list(cand_cols)]
        return contexts, candidates, rows

    def check(reqs, tag):
        B = sum(len(r) for r in reqs)
        P = 1 << (B - 1).bit_length()
        off = rq._offsets(reqs)
        f = fresh()
        sizes = {k: len(getattr(scorer, k)) for k in old}
        got = scorer.top_requests(reqs, n, scores=True)
        assert_ranked(got, off, n, tag)
        explicit, _ = rq._padded(reqs, P, filler)
        want = f.top_requests(explicit, n, scores=True)
        R = len(reqs)
        assert_same_result(got, (want[0][:R], want[1][:R], want[2][:R], want[3][:B]), tag)
        loose = f.score_requests(reqs)[0]
        worst = float((got[3] - loose).abs().max())
        print("replayed top_requests vs unpadded eager score_requests, %s B=%d: worst |dy| = %.3g" % (tag, B, worst))
        assert worst <= EVAL_GATE, (tag, worst)
        # the same requests as contexts + candidates
        contexts, candidates, rows = split(reqs)
        gc_ = scorer.top_candidates(contexts, candidates, cand_cols, off, n, scores=True)
        assert_ranked(gc_, off, n, tag)
        ec, ek, eo = contexts, candidates, off
        if P > B:
            ec = np.concatenate([contexts, filler[None]])
            ek = np.concatenate([candidates, np.repeat(filler[None, list(cand_cols)], P - B, axis=0)])
            eo = np.concatenate([off, [P]])
        wc = f.top_candidates(ec, ek, cand_cols, eo, n, scores=True)
        assert_same_result(gc_, (wc[0][:R], wc[1][:R], wc[2][:R], wc[3][:B]), tag)
        wr = f.top_requests(rq._padded(rows, P, filler)[0], n, scores=True)   # ... and against the rows built on the host
        assert_same_result(gc_, (wr[0][:R], wr[1][:R], wr[2][:R], wr[3][:B]), tag)
        assert {k: len(getattr(scorer, k)) for k in old} == sizes, "a ranked call touched another call's graphs"
        return got

    def graphs(which):
        return [e[1] for e in getattr(scorer, which).values()]

    for k in range(scorer.graph_warmup):
        check(eight[k], "warm-up %d" % k)
        assert not any(isinstance(g, (_TopGraph, _TopCandGraph)) for g in graphs("_top_graphs") + graphs("_top_cand_graphs"))
    first = check(eight[0], "capture")
    assert [type(g) for g in graphs("_top_graphs")] == [_TopGraph] and [type(g) for g in graphs("_top_cand_graphs")] == [_TopCandGraph]
    captured = graphs("_top_graphs") + graphs("_top_cand_graphs")
    for k, reqs in enumerate(eight + padded):
        check(reqs, "bucket 8, mix %d" % k)
    assert_same_result(check(eight[0], "again"), first, "again")
    assert all(a is b for a, b in zip(graphs("_top_graphs") + graphs("_top_cand_graphs"), captured)) and len(captured) == 2
    # score / score_requests beside them: their own graphs, and ours are not touched
    ids = torch.from_numpy(np.concatenate(eight[0]).astype(np.int32)).to(scorer.device)
    for _ in range(scorer.graph_warmup + 1):
        scorer.score(ids)
        scorer.score_requests(eight[0])
    assert len(scorer._graphs) == 1 and len(scorer._bucket_graphs) == 1
    assert len(scorer._top_graphs) == 1 and len(scorer._top_cand_graphs) == 1
    # another n, other columns: other entries
    scorer.top_requests(eight[0], n + 1)
    contexts, candidates, _rows = split(eight[0])
    scorer.top_candidates(contexts, candidates[:, ::-1].copy(), cand_cols[::-1], rq._offsets(eight[0]), n + 1)
    assert len(scorer._top_graphs) == 2 and len(scorer._top_cand_graphs) == 2
    assert graphs("_top_graphs")[0] is captured[0] and graphs("_top_cand_graphs")[0] is captured[1]
    captured = graphs("_top_graphs") + graphs("_top_cand_graphs")              # (the new entries are still warming up)
    # the pool and the weights change under the captured graphs
    n_ids = live.shape[1] - 1
    steps = ["relabel"] + (["append"] if form != "immutable" else []) + (["evict", "delete"] if form == "window" else []) + ["train"]
    for step in steps:
        y_old = scorer.top_requests(eight[1], n, scores=True)[3]
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
            m = min(int(hit.min()) + 1, 4)                                     # the oldest rows leave (a retrieved one among them, or the weights move anyway)
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
        assert all(a is b for a, b in zip(graphs("_top_graphs") + graphs("_top_cand_graphs"), captured)), "%s invalidated a captured chain" % step
        assert not torch.equal(scorer.top_requests(eight[1], n, scores=True)[3], y_old), "%s changed no prediction" % step


# ---- 6. refusals and the launch chain ------------------------------------------------------------------------------------------------------
class Recorder:
    """a RatLib whose ``call`` and ``size`` note the entry point's name before forwarding"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def call(self, name, *args):
        self.names.append(name)
        return self._lib.call(name, *args)

    def size(self, name, *args):
        self.names.append(name)
        return self._lib.size(name, *args)

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def take(self):
        names, self.names = self.names, []
        return names


def check_refusals(gpu, lib):
    """every refusal is raised before any entry point of the library is reached"""
    import pytest
    from rat_amd.online import MAX_TOPN, OnlineScorer
    _case, model, data, pool, cols, cfg = rq._setup("tiny_seq_bn", gpu)
    rec = Recorder(lib)
    scorer = OnlineScorer(model, pool[:14], cfg, graph=False, lib=rec)
    rec.take()
    assert MAX_TOPN == 64
    ids = np.ascontiguousarray(data[:6, :-1])
    L = ids.shape[1]
    reqs = [ids[:2], ids[2:]]
    cc = [cols[-1], [c for c in range(L) if c != cols[-1]][0]]
    contexts, candidates, off = ids[:2], np.ascontiguousarray(ids[:, cc]), [0, 2, 6]

    def refused(exc, word, fn):
        with pytest.raises(exc, match=word):
            fn()
        assert rec.take() == [], "a refused call reached the library"
    for bad, word in ((2.5, "integer"), ("3", "integer"), (None, "integer"), (True, "integer"), (np.float32(2), "integer"),
                      (0, "MAX_TOPN"), (-1, "MAX_TOPN"), (65, "MAX_TOPN")):
        refused(ValueError, word, lambda: scorer.top_requests(reqs, bad))
        refused(ValueError, word, lambda: scorer.top_candidates(contexts, candidates, cc, off, bad))
    for bad, word in (([], "non-empty"), ([cc[0], cc[0]], "repeated"), ([0.0, 1.0], "integer"), ([cc[0], L], "outside"), ([-1, cc[0]], "outside"),
                      ([[0, 1]], "1-D")):
        refused(ValueError, word, lambda: scorer.top_candidates(contexts, candidates, bad, off, 3))
        refused(ValueError, word, lambda: scorer.expand_candidates(contexts, candidates, bad, off))
    refused(ValueError, "candidates have", lambda: scorer.top_candidates(contexts, candidates[:, :1], cc, off, 3))
    refused(ValueError, "candidates have", lambda: scorer.top_candidates(contexts, candidates, cc + [(set(range(L)) - set(cc)).pop()], off, 3))
    refused(ValueError, "one encoded row per request", lambda: scorer.top_candidates(ids[:3], candidates, cc, off, 3))
    refused(ValueError, "one encoded row per request", lambda: scorer.top_candidates(ids[:1], candidates, cc, off, 3))
    refused(ValueError, "columns", lambda: scorer.top_candidates(contexts[:, :-1], candidates, cc, off, 3))
    refused(ValueError, "end at", lambda: scorer.top_candidates(contexts, candidates, cc, [0, 2, 5], 3))
    refused(ValueError, "empty request", lambda: scorer.top_candidates(contexts, candidates, cc, [0, 6, 6], 3))
    refused(ValueError, "empty request", lambda: scorer.top_requests([], 3))
    refused(ValueError, "columns", lambda: scorer.top_requests([ids[:2], ids[2:, :-1]], 3))
    refused(ValueError, "ascending", lambda: scorer.top_requests((ids, [0, 4, 2, 6]), 3))
    refused(TypeError, "same", lambda: scorer.top_requests(reqs, 3, same=[cols[0]]))             # no same= / before= on these calls
    refused(TypeError, "before", lambda: scorer.top_candidates(contexts, candidates, cc, off, 3, before=[0] * 6))
    model.train()
    refused(RuntimeError, "needs the model in eval mode", lambda: scorer.top_requests(reqs, 3))
    refused(RuntimeError, "needs the model in eval mode", lambda: scorer.top_candidates(contexts, candidates, cc, off, 3))
    model.eval()
    got = scorer.top_requests(reqs, 3)                                             # and good ones go through
    assert tuple(got[0].shape) == (2, 3) and got[2].cpu().tolist() == [2, 3] and rec.take()
    got = scorer.top_candidates(contexts, candidates, cc, off, 3)
    assert tuple(got[0].shape) == (2, 3) and got[2].cpu().tolist() == [2, 3] and rec.take()


def check_ops_refusals(device, lib):
    """the wrappers check shape, dtype and device, and read no contents"""
    import pytest
    from rat_amd import ops
    y = torch.zeros(6, dtype=torch.float32, device=device)
    first = torch.zeros(6, dtype=torch.int64, device=device)
    ids = torch.zeros((6, 4), dtype=torch.int32, device=device)
    cols = torch.tensor([1, 3], dtype=torch.int32, device=device)
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            ops.topn_seg(y, first, bad, lib=lib)
    with pytest.raises(TypeError):
        ops.topn_seg(y.double(), first, 3, lib=lib)
    with pytest.raises(TypeError):
        ops.topn_seg(y, first.int(), 3, lib=lib)
    with pytest.raises(ValueError):
        ops.topn_seg(y, first[:5], 3, lib=lib)
    with pytest.raises(ValueError):
        ops.topn_seg(y.reshape(2, 3), first, 3, lib=lib)
    with pytest.raises(ValueError):
        ops.topn_seg(y[:0], first[:0], 3, lib=lib)
    with pytest.raises(TypeError):
        ops.candidates_expand(ids.long(), ids[:, :2].contiguous(), cols, first, lib=lib)
    with pytest.raises(TypeError):
        ops.candidates_expand(ids, ids[:, :2].contiguous(), cols.long(), first, lib=lib)
    with pytest.raises(ValueError):
        ops.candidates_expand(ids, ids[:, :2], cols, first, lib=lib)                 # not contiguous
    with pytest.raises(ValueError):
        ops.candidates_expand(ids, ids[:, :3].contiguous(), cols, first, lib=lib)    # cand's width is not len(cols)
    with pytest.raises(ValueError):
        ops.candidates_expand(ids, ids[:5, :2].contiguous(), cols, first, lib=lib)
    with pytest.raises(ValueError):
        ops.candidates_expand(ids, ids[:, :2].contiguous(), cols, first[:5], lib=lib)


def check_launch_chain(gpu, lib, form, n_pool=14):
    """top_requests reaches score_requests' entry points in score_requests' order, then rat_topn_seg; top_candidates the same behind
    rat_candidates_expand.  The reference list is recorded from score_requests itself, on the same scorer."""
    from rat_amd.online import OnlineScorer
    _case, model, data, pool, cols, cfg = rq._setup("tiny_seq_bn", gpu, n_pool=n_pool)
    first, kw, later, live = rq._form(form, pool, n_pool)
    rec = Recorder(lib)
    scorer = OnlineScorer(model, first, cfg, graph=False, lib=rec, **kw)
    if later is not None:
        scorer.append(later)
    rec.take()
    contexts, candidates, cand_cols, off, rows = candidate_requests(data, live, cols, sizes=(3, 1, 4))
    scorer.score_requests((rows, off))
    chain = rec.take()
    assert len(chain) >= 3 and not any(name in ("rat_topn_seg", "rat_candidates_expand") for name in chain)
    scorer.top_requests((rows, off), 3)
    assert rec.take() == chain + ["rat_topn_seg"]
    scorer.top_candidates(contexts, candidates, cand_cols, off, 3)
    assert rec.take() == ["rat_candidates_expand"] + chain + ["rat_topn_seg"]
    scorer.expand_candidates(contexts, candidates, cand_cols, off)
    assert rec.take() == ["rat_candidates_expand"]
    return chain
