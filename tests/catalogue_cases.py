"""Checks of the device-resident item catalogue (``rat_catalogue_expand``, ``rat_topn_exclude``, ``rat_topn_merge``; their ``ops``
wrappers; ``OnlineScorer.set_catalogue`` / ``top_items`` / ``rank_items`` / ``top_catalogue``), shared by tests/test_catalogue.py (CPU,
host-emulation build) and tests/test_gpu_catalogue.py (MI355X).

Everything is bit for bit: the kernels move and compare values, they never compute with them.  The oracle of the expansion is the same
rows built in numpy; the oracle of a merge is ``np.argsort(-concat, kind="stable")[:n]`` over everything the sweep has seen so far
(excluded items removed first); the oracle of the scorer calls is the older calls over rows built on the host — ``top_candidates`` /
``rank_candidates`` over ``catalogue[items]``, and per pass ``score_requests`` over host-built rows followed by numpy's stable sort.
The only tolerance in this file is the eval forward's recorded margin (``EVAL_GATE``), where a replayed, padded prediction vector is
compared with an unpadded one."""
import ctypes
import functools

import numpy as np
import torch

import online_requests_cases as rq
import online_top_cases as tc

EVAL_GATE = rq.EVAL_GATE
POISON = tc.POISON
SEED = 20252
NS = (1, 5, 64)
R_MERGE = 3
CHUNKS = (3, 70, 2, 40)                    # items per request per pass: a page shorter than every n > 3, full pages, a 2-item pass
M_MERGE = sum(CHUNKS)
VALUE_SETS = ("eighths", "special")
EXCLUSIONS = ("empty", "edges", "whole", "one")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(device)


# ---- 1. rat_catalogue_expand == the rows built in numpy ------------------------------------------------------------------------------------
M_EXPAND = 5
SEGMENTS = (1, 2, 5, 3, 1)                 # segment lengths: the sweep form reaches items item0 .. item0 + 4


def reference_cat_expand(ctx, cat, cols, first, items=None, item0=0):
    B, M = len(first), len(cat)
    f = np.clip(np.asarray(first, dtype=object), 0, B - 1).astype(np.int64)
    i = np.asarray(items, dtype=object) if items is not None else int(item0) + (np.arange(B) - f).astype(object)
    i = np.clip(i, 0, M - 1).astype(np.int64)
    out = ctx[f].copy()
    for w, c in enumerate(cols):
        if 0 <= c < ctx.shape[1]:
            out[:, c] = cat[i, w]
    return out


def check_expand_kernel(device, lib, shapes=tc.EXPAND_SHAPES):
    from rat_amd import ops
    first, starts = tc._first_row(list(SEGMENTS))
    B, M = len(first), M_EXPAND
    rng = np.random.default_rng(SEED)
    lists = {"ends and repeats": np.array([0, M - 1, M - 1, 0, 2, 2, 2, M - 1, 0, 1, 3, 3], dtype=np.int32),
             "clamped": np.array([-3, M, 2 ** 31 - 1, 0, -2 ** 31, 4, M + 1, 1, -1, 2, 3, M - 1], dtype=np.int32)}
    assert all(len(v) == B for v in lists.values())
    for L, cols in shapes:
        ctx = np.full((B, L), POISON, dtype=np.int32)                         # rows that open no request: never read
        ctx[starts] = rng.integers(0, 1000, size=(len(starts), L))
        cat = rng.integers(1000, 2000, size=(M, len(cols))).astype(np.int32)
        t_ctx, t_cat, t_cols, t_first = (_dev(a, device) for a in (ctx, cat, np.asarray(cols, dtype=np.int32), first))
        for what, items in lists.items():
            got = ops.catalogue_expand(t_ctx, t_cat, t_cols, t_first, items=_dev(items, device), lib=lib)
            want = reference_cat_expand(ctx, cat, cols, first, items=items)
            assert (want != POISON).all()
            assert got.dtype == torch.int32 and tuple(got.shape) == (B, L)
            assert np.array_equal(got.cpu().numpy(), want), (L, cols, what)
        for item0 in (0, 3):                                                   # the sweep form: row k of a request is item item0 + k
            got = ops.catalogue_expand(t_ctx, t_cat, t_cols, t_first, item0=item0, lib=lib)
            want = reference_cat_expand(ctx, cat, cols, first, item0=item0)
            for s, m in zip(starts, SEGMENTS):
                assert np.array_equal(want[s:s + m][:, list(cols)], cat[np.minimum(item0 + np.arange(m), M - 1)])
            assert np.array_equal(got.cpu().numpy(), want), (L, cols, "sweep", item0)
        assert np.array_equal(t_ctx.cpu().numpy(), ctx) and np.array_equal(t_cat.cpu().numpy(), cat)
        # B = 1
        one = [t_ctx[:1].contiguous(), t_cat, t_cols, t_first[:1].contiguous()]
        got = ops.catalogue_expand(*one, items=_dev(np.array([M - 1], dtype=np.int32), device), lib=lib)
        assert np.array_equal(got.cpu().numpy(), reference_cat_expand(ctx[:1], cat, cols, first[:1], items=[M - 1])), (L, cols, "B = 1")
        got = ops.catalogue_expand(*one, item0=2, lib=lib)
        assert np.array_equal(got.cpu().numpy(), reference_cat_expand(ctx[:1], cat, cols, first[:1], item0=2)), (L, cols, "B = 1 sweep")


# ---- 2. rat_topn_exclude and rat_topn_merge against numpy ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def merge_values(set_name):
    """-> y fp32 [R][M]: request r's predictions for the M items of the sweep, from a fixed seed"""
    rng = np.random.default_rng(SEED + 10 + VALUE_SETS.index(set_name))
    y = (np.round(rng.random((R_MERGE, M_MERGE)) * 8) / 8).astype(np.float32)  # 9 values: ties inside and across the chunks
    c1 = CHUNKS[0]
    if set_name == "eighths":
        # request 2 holds one 1.0, four 0.875 — in three different chunks — and 64 values >= 0.5: once everything is seen, the cuts at
        # n = 1, 5 and 64 fall between different values (the random rows put them inside runs of equal values)
        row = y[2]
        row[row >= 0.875] = 0.75
        row[c1 + 10] = 1.0
        row[[1, c1 + 20, c1 + 69, M_MERGE - 5]] = 0.875
        high = np.nonzero(row >= 0.5)[0]
        low = np.nonzero(row == 0.375)[0]
        if len(high) > 64:
            row[[i for i in high[::-1] if row[i] == 0.5][:len(high) - 64]] = 0.375
        else:
            row[low[:64 - len(high)]] = 0.5
        assert (row >= 0.5).sum() == 64 and (row == 1.0).sum() == 1 and (row == 0.875).sum() == 4
    if set_name == "special":
        y[0, 0], y[0, c1 + 5], y[0, c1 + 6] = np.nan, np.inf, np.inf
        y[0, c1 + 69], y[0, M_MERGE - 1] = np.nan, np.inf                      # a chunk's last item; an infinity that arrives last
        y[1, :] = np.where(y[1] == 0.5, np.float32(-0.0), y[1])
        y[1, 1], y[1, c1], y[1, M_MERGE - 2] = 0.0, -np.inf, -0.0
        y[2, :CHUNKS[0]] = np.nan                                              # a whole first pass of NaN: every later number comes before it
        y[2, c1 + 1], y[2, c1 + 2] = -np.inf, np.nan
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def exclusion_lists(which):
    """-> (ex_items int32 [E], ex_offsets int64 [R + 1]): ascending per request"""
    y = merge_values("eighths")
    a, b = CHUNKS[0], CHUNKS[0] + CHUNKS[1]                                    # the second chunk's items: a .. b - 1
    if which == "empty":
        per = [[], [], []]
    elif which == "edges":
        per = [[a, b - 1], [a], [b - 1, b]]                                    # a chunk's first and last item
    elif which == "whole":
        per = [list(range(a, b)), list(range(a, b)), list(range(0, a)) + list(range(b, b + CHUNKS[2]))]     # all of a chunk
    else:
        per = [[], sorted(np.argsort(-y[1], kind="stable")[:7].tolist()), []]   # one request only: its seven best items
    off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
    items = np.asarray([i for p in per for i in p], dtype=np.int32)
    return items, off


def _chunk_starts():
    return np.concatenate([[0], np.cumsum(CHUNKS)])[:-1]


def reference_running(y, seen, n, lists=None):
    """numpy's stable sort over the first ``seen`` items of every request, excluded items removed -> (items [R][n], val [R][n], len [R])"""
    R = len(y)
    items = np.full((R, n), -1, dtype=np.int32)
    val = np.zeros((R, n), dtype=np.float32)
    lens = np.zeros(R, dtype=np.int32)
    for r in range(R):
        keep = np.arange(seen)
        if lists is not None:
            keep = keep[~np.isin(keep, lists[0][lists[1][r]:lists[1][r + 1]])]
        order = np.argsort(-y[r, keep], kind="stable")[:n]
        items[r, :len(order)], val[r, :len(order)], lens[r] = keep[order], y[r, keep][order], len(order)
    return items, val, lens


def chunk_page(y, i0, m, n, lists=None):
    """what the passes before the merge leave for the items i0 .. i0 + m - 1: y as [R * m] (request r's rows at r * m), the excluded
    rows at -inf, and rat_topn_seg's three outputs over it, computed in numpy — rows that open no request hold POISON, never read"""
    R = len(y)
    flat = np.ascontiguousarray(y[:, i0:i0 + m]).reshape(-1).copy()
    masked = flat.copy()
    if lists is not None:
        for r in range(R):
            ex = lists[0][lists[1][r]:lists[1][r + 1]]
            masked[r * m:(r + 1) * m][np.isin(i0 + np.arange(m), ex)] = -np.inf
    pos, val, lens = tc.reference_topn(masked, [(r * m, m) for r in range(R)], n)
    heads = np.arange(R, dtype=np.int64) * m
    other = np.setdiff1d(np.arange(R * m), heads)
    pos[other], val[other], lens[other] = POISON, 7.0, 9
    first = np.repeat(heads, m)
    return flat, masked, first, heads, (pos, val, lens)


def assert_merge_regimes():
    """what the eighths reach, established in numpy: for every n a tie that straddles the cut, a cut between different values, and
    a value held by the running page and by the arriving chunk's page that survives the merge (a tie across the chunk boundary);
    running pages that are empty, partly filled and full; a chunk's page shorter than n"""
    y = merge_values("eighths")
    starts = _chunk_starts()
    for n in NS:
        straddle = differ = boundary = False
        lens_seen, short = set(), False
        for k, (i0, m) in enumerate(zip(starts, CHUNKS)):
            before = reference_running(y, i0, n)
            after = reference_running(y, i0 + m, n)
            short |= m < n
            for r in range(R_MERGE):
                lens_seen.add("empty" if before[2][r] == 0 else ("full" if before[2][r] == n else "partial"))
                order = np.argsort(-y[r, :i0 + m], kind="stable")
                if len(order) > n:
                    a, b = y[r, order[n - 1]], y[r, order[n]]
                    straddle |= bool(a == b)
                    differ |= bool(a != b)
                if before[2][r]:                                               # a value both pages hold, at or above the cut
                    arriving = np.sort(y[r, i0:i0 + m])[::-1][:n]
                    cut = after[1][r, after[2][r] - 1]
                    both = np.intersect1d(before[1][r, :before[2][r]], arriving)
                    boundary |= bool((both >= cut).any())
        assert straddle and differ and boundary, (n, straddle, differ, boundary)
        assert short or n == 1
        assert lens_seen >= ({"empty", "full"} if n == 1 else {"empty", "partial", "full"}), (n, lens_seen)
    s = merge_values("special")
    assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any() and ((s == 0) & np.signbit(s)).any() and ((s == 0) & ~np.signbit(s)).any()


def _new_page(R, n, device):
    return (torch.full((R, n), -1, dtype=torch.int32, device=device), torch.zeros((R, n), dtype=torch.float32, device=device),
            torch.zeros((R,), dtype=torch.int32, device=device))


def assert_page_equal(got, want, what):
    tc.assert_topn_equal(got, want, what)


def check_merge_kernel(device, lib, set_name, which=None, ns=NS):
    """a sweep over CHUNKS: after every pass the running page equals numpy's stable sort over everything seen so far"""
    from rat_amd import ops
    assert_merge_regimes()
    assert (set_name == "eighths") or which is None, "exclusion is claimed for predictions that are not NaN"
    y = merge_values(set_name)
    lists = exclusion_lists(which) if which is not None else None
    t_lists = (None, None) if lists is None else (_dev(lists[0], device), _dev(lists[1], device))
    for n in ns:
        run = _new_page(R_MERGE, n, device)
        for i0, m in zip(_chunk_starts(), CHUNKS):
            flat, masked, first, heads, page = chunk_page(y, int(i0), m, n, lists)
            if lists is not None:                                              # rat_topn_exclude on the same lists
                out = ops.topn_exclude(_dev(flat, device), _dev(first, device), int(i0), m, t_lists[0], t_lists[1], lib=lib)
                assert torch.equal(_bits(out.cpu()), _bits(torch.from_numpy(masked))), (set_name, which, n, int(i0))
            t_page = [_dev(a, device) for a in page]
            ops.topn_merge(run[0], run[1], run[2], t_page[0], t_page[1], t_page[2], _dev(heads, device), int(i0), t_lists[0], t_lists[1],
                           lib=lib)
            assert_page_equal(run, reference_running(y, int(i0) + m, n, lists), (set_name, which, n, int(i0)))
            assert all(np.array_equal(t.cpu().numpy(), a) or (a.dtype == np.float32 and torch.equal(_bits(t.cpu()), _bits(torch.from_numpy(a))))
                       for t, a in zip(t_page, page)), "the chunk's page was written"


def check_two_merges_equal_one(device, lib, ns=(5, 64)):
    """merging the pages of two consecutive chunks equals merging the page of their union"""
    from rat_amd import ops
    y = merge_values("eighths")
    i0, m1, m2 = CHUNKS[0], 30, 40
    for which in (None, "edges"):
        lists = exclusion_lists(which) if which else None
        t_lists = (None, None) if lists is None else (_dev(lists[0], device), _dev(lists[1], device))
        for n in ns:
            two, one = _new_page(R_MERGE, n, device), _new_page(R_MERGE, n, device)
            for page_of, start, m in ((two, i0, m1), (two, i0 + m1, m2), (one, i0, m1 + m2)):
                _flat, _masked, _first, heads, page = chunk_page(y, start, m, n, lists)
                ops.topn_merge(*page_of, *[_dev(a, device) for a in page], _dev(heads, device), start, *t_lists, lib=lib)
            tc.assert_same_result(two, one, ("two merges", which, n))
            assert int(one[2].min()) >= min(n, m1 + m2 - 2)


# ---- 3. corrupt arguments address nothing outside the buffers (host-emulation build only) ---------------------------------------------------
def reference_exclude_contract(y, first, item0, per, ex_items, ex_off, R):
    """rat_topn_exclude's contract for ANY first_row and offsets (the list is globally ascending, so every clamped range is)"""
    B, E = len(y), len(ex_items)
    out = y.copy()
    for b in range(B):
        f = min(max(int(first[b]), 0), B - 1)
        r = min(max(f // per, 0), R - 1)
        lo = min(max(int(ex_off[r]), 0), E)
        hi = min(max(int(ex_off[r + 1]), lo), E)
        if (item0 + (b - f)) in ex_items[lo:hi].tolist():
            out[b] = -np.inf
    return out


def reference_merge_contract(run, page, heads, item0, n, B, ex_items=None, ex_off=None):
    """rat_topn_merge's contract for ANY heads, lengths and offsets"""
    R = len(heads)
    items = np.full((R, n), -1, dtype=np.int32)
    val = np.zeros((R, n), dtype=np.float32)
    lens = np.zeros(R, dtype=np.int32)
    for r in range(R):
        rl = min(max(int(run[2][r]), 0), n)
        h = min(max(int(heads[r]), 0), B - 1)
        cl = min(max(int(page[2][h]), 0), n)
        ent = [(int(run[0][r, t]), run[1][r, t]) for t in range(rl)]
        for t in range(cl):
            it = item0 + int(page[0][h, t])
            if ex_items is not None:
                E = len(ex_items)
                lo = min(max(int(ex_off[r]), 0), E)
                hi = min(max(int(ex_off[r + 1]), lo), E)
                if it in ex_items[lo:hi].tolist():
                    continue
            ent.append((it, page[1][h, t]))
        v = np.asarray([e[1] for e in ent], dtype=np.float32)
        order = np.argsort(-v, kind="stable")[:n]
        items[r, :len(order)] = np.asarray([ent[j][0] for j in order], dtype=np.int64).astype(np.int32)
        val[r, :len(order)], lens[r] = v[order], len(order)
    return items, val, lens


def check_corrupt(lib, guard=4096):
    """the three kernels through the C ABI, every buffer between guard regions: first_row negative, >= B and non-monotone, cols outside
    [0, L), items outside [0, M), heads and lengths out of range, ex_offsets non-monotone and out of range, item0 at the ends of
    int64.  The calls return normally, no guard byte changes, the inputs are only read, and the outputs are what the contract says."""
    FILL = -99
    rng = np.random.default_rng(SEED + 200)
    B, L, M, n, R = 40, 8, 6, 5, 4

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
        for b, v in read_only.items():
            assert torch.equal(_bits(bufs[b][0]) if bufs[b][0].dtype == torch.float32 else bufs[b][0], v), (b, what)

    def snapshot(bufs, names):
        return {b: (_bits(bufs[b][0]) if bufs[b][0].dtype == torch.float32 else bufs[b][0]).clone() for b in names}
    firsts = [np.arange(B) - 50, np.arange(B) + B, np.full(B, -2 ** 63), np.full(B, 2 ** 63 - 1), rng.integers(-10, B + 10, size=B),
              rng.permutation(B), np.arange(B)[::-1], np.array([0, 0, 0, 3, 3, 0, 0, 7, 2 ** 40, -2 ** 40] * 4)]
    item_lists = [rng.integers(0, M, size=B), rng.integers(-10, M + 10, size=B), np.full(B, -2 ** 31), np.full(B, 2 ** 31 - 1)]
    y = (np.round(rng.random(B) * 8) / 8).astype(np.float32)
    y[3], y[17] = np.nan, -np.inf
    ex_items = np.sort(rng.integers(-3, 12, size=9)).astype(np.int32)         # globally ascending: every clamped range of it is a list
    offsets = [np.array([0, 2, 5, 7, 9]), np.array([5, 2, 9, 0, 4]), np.array([-7, 100, -2 ** 63, 2 ** 63 - 1, 3]), np.array([9, 9, 9, 9, 9]),
               np.array([2 ** 40, 0, 0, 0, -1])]
    for k, first in enumerate(firsts):
        first = np.asarray(first, dtype=np.int64)
        # --- expansion
        for cols in ([5, 0, 3], [-1, 3, L, 10 ** 6, -2 ** 31, 2 ** 31 - 1, 6]):
            W = len(cols)
            ctx = rng.integers(0, 1000, size=(B, L)).astype(np.int32)
            cat = rng.integers(1000, 2000, size=(M, W)).astype(np.int32)
            for width in (L, L - 1):                                           # 16-byte words, and word by word
                modes = [(items, 0) for items in item_lists[k % 2::2]] + [(None, 0), (None, 3), (None, -2 ** 63), (None, 2 ** 63 - 1)]
                for items, item0 in modes:
                    bufs = dict(ctx=guarded(ctx[:, :width], torch.int32), cat=guarded(cat, torch.int32), cols=guarded(cols, torch.int32),
                                first=guarded(first, torch.int64), out=guarded(np.full(B * width, 7), torch.int32))
                    if items is not None:
                        bufs["items"] = guarded(items, torch.int32)
                    ro = snapshot(bufs, [b for b in bufs if b != "out"])
                    lib.call("rat_catalogue_expand", p(bufs["ctx"][1]), p(bufs["cat"][1]), p(bufs["items"][1]) if items is not None else None,
                             item0, p(bufs["cols"][1]), p(bufs["first"][1]), B, width, W, M, p(bufs["out"][1]), None)
                    intact(bufs, ro, ("expand", k, cols, width, item0))
                    want = reference_cat_expand(np.ascontiguousarray(ctx[:, :width]), cat, cols, first, items=items, item0=item0)
                    assert np.array_equal(bufs["out"][1].reshape(B, width).numpy(), want), ("expand", k, cols, width, item0, items is None)
        # --- exclusion
        off = np.asarray(offsets[k % len(offsets)], dtype=np.int64)
        for per, item0 in ((10, 0), (7, 3), (1, -2), (2 ** 40, 2 ** 63 - 1)):
            bufs = dict(y=guarded(y, torch.float32), first=guarded(first, torch.int64), ex=guarded(ex_items, torch.int32),
                        off=guarded(off, torch.int64), out=guarded(np.full(B, 7.0), torch.float32))
            ro = snapshot(bufs, ("y", "first", "ex", "off"))
            lib.call("rat_topn_exclude", p(bufs["y"][1]), p(bufs["first"][1]), item0, per, p(bufs["ex"][1]), p(bufs["off"][1]), len(ex_items),
                     R, B, p(bufs["out"][1]), None)
            intact(bufs, ro, ("exclude", k, per, item0))
            want = reference_exclude_contract(y, first, min(item0, 2 ** 32), per, ex_items, off, R)
            assert torch.equal(_bits(bufs["out"][1]), _bits(torch.from_numpy(want))), ("exclude", k, per, item0)
    # --- merge
    pos = rng.integers(0, 10, size=(B, n)).astype(np.int32)
    val = (np.round(rng.random((B, n)) * 8) / 8).astype(np.float32)
    val[2, 1], val[5, 0] = np.nan, np.inf
    lens_lists = [rng.integers(0, n + 1, size=B), rng.integers(-5, n + 10, size=B), np.full(B, 2 ** 31 - 1), np.full(B, -2 ** 31)]
    heads_lists = [np.array([0, 10, 20, 30]), np.array([-5, B, 2 ** 63 - 1, -2 ** 63]), np.array([39, 39, 0, 0]), np.array([7, 3, 2 ** 40, 5])]
    run_lens = [np.array([0, 2, n, 3]), np.array([-5, n + 10, 2 ** 31 - 1, -2 ** 31])]
    k = 0
    for lens in lens_lists:
        for heads in heads_lists:
            for run_len in run_lens:
                for off in offsets + [None]:
                    k += 1
                    run_item = rng.integers(0, 50, size=(R, n)).astype(np.int32)
                    run_val = (np.round(rng.random((R, n)) * 8) / 8).astype(np.float32)
                    item0 = (0, 3, -4, 2 ** 63 - 1, -2 ** 63)[k % 5]
                    bufs = dict(run_item=guarded(run_item, torch.int32), run_val=guarded(run_val, torch.float32),
                                run_len=guarded(run_len, torch.int32), pos=guarded(pos, torch.int32), val=guarded(val, torch.float32),
                                lens=guarded(lens, torch.int32), heads=guarded(heads, torch.int64), ex=guarded(ex_items, torch.int32))
                    if off is not None:
                        bufs["off"] = guarded(off, torch.int64)
                    ro = snapshot(bufs, [b for b in bufs if not b.startswith("run")])
                    lib.call("rat_topn_merge", p(bufs["run_item"][1]), p(bufs["run_val"][1]), p(bufs["run_len"][1]), p(bufs["pos"][1]),
                             p(bufs["val"][1]), p(bufs["lens"][1]), p(bufs["heads"][1]), item0, p(bufs["ex"][1]) if off is not None else None,
                             p(bufs["off"][1]) if off is not None else None, len(ex_items), R, B, n, None)
                    intact(bufs, ro, ("merge", k))
                    clamped0 = min(max(item0, -2 ** 31), 2 ** 32)
                    want = reference_merge_contract((run_item, run_val, np.asarray(run_len, dtype=np.int64)), (pos, val, np.asarray(lens, dtype=np.int64)),
                                                    heads, clamped0, n, B, ex_items if off is not None else None, off)
                    got = (bufs["run_item"][1].reshape(R, n), bufs["run_val"][1].reshape(R, n), bufs["run_len"][1])
                    assert_page_equal(got, want, ("merge", k))


def check_abi_refusals(device, lib):
    """a null pointer, B, R, M < 1, L / W / n out of range, E < 0, rows_per_request < 1: -1 and a message, nothing launched"""
    B, n, R = 4, 3, 2
    y = torch.zeros(B, dtype=torch.float32, device=device)
    first = torch.zeros(B, dtype=torch.int64, device=device)
    ids = torch.full((B, 4), 7, dtype=torch.int32, device=device)
    out_y = torch.full((B,), 7.0, dtype=torch.float32, device=device)
    off = torch.zeros(R + 1, dtype=torch.int64, device=device)
    ri = torch.full((R, n), 7, dtype=torch.int32, device=device)
    rv = torch.full((R, n), 7.0, dtype=torch.float32, device=device)
    rl = torch.full((R,), 7, dtype=torch.int32, device=device)
    pos = torch.zeros((B, n), dtype=torch.int32, device=device)
    val = torch.zeros((B, n), dtype=torch.float32, device=device)
    lens = torch.zeros((B,), dtype=torch.int32, device=device)
    heads = torch.zeros((R,), dtype=torch.int64, device=device)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def refuse(name, good, bad):
        for slot, value in bad:
            args = list(good)
            args[slot] = value
            assert getattr(lib.cdll, name)(*args) == -1 and name in lib.last_error(), (name, slot, value)
    good = [p(ids), p(ids), p(first.int()), 0, p(ids), p(first), B, 4, 4, 4, p(ids), None]
    refuse("rat_catalogue_expand", good, [(0, None), (1, None), (4, None), (5, None), (10, None), (6, 0), (6, -5), (6, 2 ** 31), (7, 0), (7, 8193),
                                          (8, 0), (8, 8193), (9, 0), (9, -1), (9, 2 ** 31)])
    good = [p(y), p(first), 0, 2, p(ids), p(off), 2, R, B, p(out_y), None]
    refuse("rat_topn_exclude", good, [(0, None), (1, None), (4, None), (5, None), (9, None), (3, 0), (3, -1), (6, -1), (7, 0), (7, 2 ** 31), (8, 0),
                                      (8, 2 ** 31)])
    good = [p(ri), p(rv), p(rl), p(pos), p(val), p(lens), p(heads), 0, p(ids), p(off), 2, R, B, n, None]
    refuse("rat_topn_merge", good, [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (9, None), (8, None), (10, -1),
                                    (11, 0), (11, 2 ** 31), (12, 0), (12, 2 ** 31), (13, 0), (13, 65), (13, -1)])
    assert (ids == 7).all() and (out_y == 7).all() and (ri == 7).all() and (rv == 7).all() and (rl == 7).all()
    # the forms the contract allows: no lists at all, and E == 0 with no ex_items.  Two empty pages merge into an empty page
    rl.zero_()
    assert lib.cdll.rat_topn_merge(p(ri), p(rv), p(rl), p(pos), p(val), p(lens), p(heads), 0, None, None, 0, R, B, n, None) == 0
    assert lib.cdll.rat_topn_merge(p(ri), p(rv), p(rl), p(pos), p(val), p(lens), p(heads), 0, None, p(off), 0, R, B, n, None) == 0
    assert lib.cdll.rat_topn_exclude(p(y), p(first), 0, 2, None, p(off), 0, R, B, p(out_y), None) == 0
    assert (out_y == 0).all() and rl.cpu().tolist() == [0, 0] and (ri == -1).all() and (rv == 0).all()


def check_ops_refusals(device, lib):
    """the wrappers check shape, dtype and device, and read no contents"""
    import pytest
    from rat_amd import ops
    y = torch.zeros(6, dtype=torch.float32, device=device)
    first = torch.zeros(6, dtype=torch.int64, device=device)
    ids = torch.zeros((6, 4), dtype=torch.int32, device=device)
    cat = torch.zeros((3, 2), dtype=torch.int32, device=device)
    cols = torch.tensor([1, 3], dtype=torch.int32, device=device)
    items = torch.zeros(6, dtype=torch.int32, device=device)
    off = torch.zeros(3, dtype=torch.int64, device=device)
    run = _new_page(2, 3, device)
    page = (torch.zeros((6, 3), dtype=torch.int32, device=device), torch.zeros((6, 3), dtype=torch.float32, device=device),
            torch.zeros(6, dtype=torch.int32, device=device))
    heads = torch.zeros(2, dtype=torch.int64, device=device)
    for bad in (lambda: ops.catalogue_expand(ids.long(), cat, cols, first, lib=lib), lambda: ops.catalogue_expand(ids, cat.long(), cols, first, lib=lib),
                lambda: ops.catalogue_expand(ids, cat, cols, first, items=items.long(), lib=lib), lambda: ops.topn_exclude(y.double(), first, 0, 2, items, off, lib=lib),
                lambda: ops.topn_exclude(y, first, 0, 2, items.long(), off, lib=lib), lambda: ops.topn_exclude(y, first, 0, 2, items, off.int(), lib=lib),
                lambda: ops.topn_merge(run[0].long(), run[1], run[2], *page, heads, 0, lib=lib), lambda: ops.topn_merge(*run, *page, heads.int(), 0, lib=lib)):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: ops.catalogue_expand(ids, cat[:, :1].contiguous(), cols, first, lib=lib),          # the catalogue's width is not len(cols)
                lambda: ops.catalogue_expand(ids, cat[:, :1], cols[:1], first, lib=lib),                   # not contiguous
                lambda: ops.catalogue_expand(ids, cat, cols, first, items=items[:5], lib=lib), lambda: ops.catalogue_expand(ids, cat, cols, first[:5], lib=lib),
                lambda: ops.catalogue_expand(ids, cat[:0], cols, first, lib=lib), lambda: ops.catalogue_expand(ids, cat, cols, first, item0=1.5, lib=lib),
                lambda: ops.topn_exclude(y, first, 0, 0, items, off, lib=lib), lambda: ops.topn_exclude(y, first, 0, 2.0, items, off, lib=lib),
                lambda: ops.topn_exclude(y, first[:5], 0, 2, items, off, lib=lib), lambda: ops.topn_exclude(y, first, 0, 2, items, off[:1], lib=lib),
                lambda: ops.topn_exclude(y.reshape(2, 3), first, 0, 2, items, off, lib=lib),
                lambda: ops.topn_merge(*run, page[0][:, :2].contiguous(), page[1], page[2], heads, 0, lib=lib),
                lambda: ops.topn_merge(*run, *page, heads[:1], 0, lib=lib), lambda: ops.topn_merge(*run, *page, heads, 0, ex_items=items, lib=lib),
                lambda: ops.topn_merge(*run, *page, heads, 0, ex_items=items, ex_offsets=off[:2], lib=lib),
                lambda: ops.topn_merge(*_new_page(2, 65, device), *page, heads, 0, lib=lib)):
        with pytest.raises(ValueError):
            bad()
    assert (run[0] == -1).all() and (run[2] == 0).all()


# ---- 4. the scorer ----------------------------------------------------------------------------------------------------------------------
M_CAT = 37
CHUNK = 16                                  # passes of 16, 16 and 5 items per request
R_CAT = 3
TOP_NS = (5, 64)


def _catalogue(live, cols, M=M_CAT, shift=0):
    """-> (the catalogue [M, W] — ids of live rows, item i and item i + 9 alike: predictions tie —, its columns, unsorted)"""
    cand_cols = (cols[-1], cols[0]) if len(cols) > 1 else (cols[0],)
    pick = (5 * np.arange(M) + shift) % 9 % len(live)
    return live[pick][:, list(cand_cols)].astype(np.int64), cand_cols


def _contexts(data, live, cols, cand_cols, R=R_CAT):
    contexts = data[:R, :-1].copy()
    contexts[:, cols] = live[np.arange(R) % len(live)][:, cols]
    contexts[:, list(cand_cols)] = POISON                                      # the contexts' own entries in these columns are ignored
    return contexts


def _host_rows(contexts, cat, cand_cols, i0, m):
    """the rows of one pass, request after request: every context with the items i0 .. i0 + m - 1"""
    rows = np.repeat(contexts, m, axis=0)
    rows[:, list(cand_cols)] = np.tile(cat[i0:i0 + m], (len(contexts), 1))
    assert (rows != POISON).all()
    return rows, np.arange(len(contexts) + 1, dtype=np.int64) * m


def reference_scores(scorer, contexts, cat, cand_cols, chunk, pad_filler=None, on_pass=None):
    """per pass host-built rows through score_requests, the passes concatenated per request -> the full predictions fp32 [R, M].
    ``pad_filler``: every pass is padded to the next power of two with an explicit trailing request of that row (what a bucket
    graph's launches see)"""
    R, M = len(contexts), len(cat)
    full = np.zeros((R, M), dtype=np.float32)
    for i0 in range(0, M, chunk):
        m = min(chunk, M - i0)
        rows, off = _host_rows(contexts, cat, cand_cols, i0, m)
        B = len(rows)
        P = 1 << (B - 1).bit_length()
        if pad_filler is not None and P > B:
            rows, off = np.concatenate([rows, np.repeat(pad_filler[None], P - B, axis=0)]), np.concatenate([off, [P]])
        y = scorer.score_requests((rows, off))[0].cpu().numpy()[:B]
        if on_pass is not None:
            on_pass()
        full[:, i0:i0 + m] = y.reshape(R, m)
    full.setflags(write=False)
    return full


def reference_pages(full, n, per_request=None):
    """excluded entries removed in numpy, then numpy's stable sort over a request's M predictions -> (items [R, n], val [R, n],
    lens [R], the full predictions)"""
    M = full.shape[1]
    lists = None
    if per_request is not None:
        off = np.concatenate([[0], np.cumsum([len(p) for p in per_request])]).astype(np.int64)
        lists = (np.asarray([i for p in per_request for i in p], dtype=np.int64), off)
    return reference_running(full, M, n, lists) + (full,)


def assert_catalogue_equal(got, want, what):
    tc.assert_topn_equal(got[:3], want[:3], what)
    if len(got) > 3:
        assert got[3].dtype == torch.float32 and torch.equal(_bits(got[3].cpu()), _bits(torch.from_numpy(want[3].copy()))), (what, "scores")


def check_items(name, gpu, lib, form, n_pool=14, ns=(3, 8)):
    """top_items / rank_items equal top_candidates / rank_candidates over catalogue[items] built on the host"""
    scorer, _case, _model, data, cols, _cfg, live = tc._scorer(name, gpu, lib, form, n_pool)
    device = scorer.device
    cat, cand_cols = _catalogue(live, cols)
    sizes = (3, 1, 4, 2, 6, 1, tc.BIG)
    contexts = _contexts(data, live, cols, cand_cols, R=len(sizes))
    C = sum(sizes)
    items = (7 * np.arange(C) + 3) % M_CAT
    items[0], items[1], items[5], items[6] = 0, M_CAT - 1, 11, 11               # the ends of the catalogue, a repeat
    off = rq._offsets([np.zeros((m, 1)) for m in sizes])
    assert scorer.catalogue_size == 0
    scorer.set_catalogue(cat, cand_cols)
    assert scorer.catalogue_size == M_CAT
    candidates = cat[items]
    for n in ns:
        what = "%s n=%d" % (form, n)
        want = scorer.top_candidates(contexts, candidates, cand_cols, off, n, scores=True)
        got = scorer.top_items(contexts, items, off, n, scores=True)
        tc.assert_same_result(got, want, what)
        tc.assert_ranked(got, off, n, what)
        tc.assert_same_result(scorer.top_items(contexts, items, off, n), want[:3], what)
        variants = [(torch.from_numpy(contexts), torch.from_numpy(items), off.tolist()), (contexts, items.tolist(), torch.from_numpy(off))]
        if gpu >= 0:
            variants.append((torch.from_numpy(contexts.astype(np.int32)).to(device), torch.from_numpy(items).to(device), torch.from_numpy(off).to(device)))
            variants.append((contexts, torch.from_numpy(items.astype(np.int32)).to(device), off))
        for c, i, o in variants:
            tc.assert_same_result(scorer.top_items(c, i, o, n, scores=True), want, what)
    want = scorer.rank_candidates(contexts, candidates, cand_cols, off, scores=True)
    got = scorer.rank_items(contexts, items, off, scores=True)
    assert type(got) is type(want) and torch.equal(got.offsets, want.offsets)
    tc.assert_same_result([got.order, got.val, got.rank, got.y_pred], [want.order, want.val, want.rank, want.y_pred], form)
    assert scorer.rank_items(contexts, items, off).y_pred is None
    # a catalogue given as a tensor, and replaced: the calls follow it
    other, _ = _catalogue(live, cols, shift=2)
    assert not np.array_equal(other, cat)
    scorer.set_catalogue(torch.from_numpy(other) if gpu < 0 else torch.from_numpy(other).to(device), list(cand_cols))
    tc.assert_same_result(scorer.top_items(contexts, items, off, 3, scores=True),
                          scorer.top_candidates(contexts, other[items], cand_cols, off, 3, scores=True), "replaced catalogue")


def _exclusions(want_plain):
    """lists that remove the best item of request 0, a whole pass of request 1 — the second —, and nothing of request 2"""
    return [[int(want_plain[0][0, 0])], list(range(CHUNK, 2 * CHUNK)), []]


def check_top_catalogue(name, gpu, lib, form, n_pool=14, ns=TOP_NS, chunks=(CHUNK,), variants=True):
    """top_catalogue equals, per pass, host-built rows through score_requests, the passes concatenated and sorted by numpy — without
    and with exclusion lists.  The predictions of a chunking are computed once and shared by every n and every list.  ``variants``:
    the other forms of the arguments as well (host tensors, lists with repeats, device lists)"""
    scorer, _case, _model, data, cols, _cfg, live = tc._scorer(name, gpu, lib, form, n_pool)
    device = scorer.device
    cat, cand_cols = _catalogue(live, cols)
    contexts = _contexts(data, live, cols, cand_cols)
    scorer.set_catalogue(cat, cand_cols)
    for chunk in chunks:
        full = reference_scores(scorer, contexts, cat, cand_cols, chunk)
        assert any(len(np.unique(full[r])) < M_CAT for r in range(R_CAT)), "no request holds two equal predictions"
        for n in ns:
            what = "%s chunk=%d n=%d" % (form, chunk, n)
            want = reference_pages(full, n)
            got = scorer.top_catalogue(contexts, n, chunk=chunk, scores=True)
            assert tuple(got[0].shape) == (R_CAT, n) and tuple(got[3].shape) == (R_CAT, M_CAT)
            assert_catalogue_equal(got, want, what)
            assert got[2].cpu().tolist() == [min(n, M_CAT)] * R_CAT
            if variants:
                assert_catalogue_equal(scorer.top_catalogue(torch.from_numpy(contexts), n, chunk=chunk), want, what)
            per = _exclusions(want)
            want_ex = reference_pages(full, n, per_request=per)
            assert want_ex[0][0, 0] != want[0][0, 0] and not np.isin(want_ex[0][1], per[1]).any()
            assert np.array_equal(want_ex[0][2], want[0][2])
            off = np.concatenate([[0], np.cumsum([len(p) for p in per])])
            flat = np.asarray([i for p in per for i in p])
            shuffled = flat.copy()
            shuffled[1:1 + CHUNK] = shuffled[1:1 + CHUNK][::-1]                    # unsorted on the host: sorted per request by the call
            forms = [(shuffled, off)]
            if variants:                                                       # ... and a repeat
                forms.append((torch.from_numpy(np.concatenate([flat[:1], flat])), (off + np.array([0, 1, 1, 1])).tolist()))
            if gpu >= 0:
                forms.append((torch.from_numpy(flat).to(device), torch.from_numpy(off).to(device)))
            for ex in forms:
                got = scorer.top_catalogue(contexts, n, chunk=chunk, exclude=ex, scores=True)
                assert_catalogue_equal(got, want_ex, what + " exclude")
                assert got[2].cpu().tolist() == [min(n, M_CAT - len(p)) for p in per]
        if chunk == M_CAT:                                                     # the default chunk is one pass here: graph_max_batch // R >= M
            assert scorer.graph_max_batch // R_CAT >= M_CAT
            assert_catalogue_equal(scorer.top_catalogue(contexts, ns[0]), reference_pages(full, ns[0]), "default chunk")
            one = reference_scores(scorer, contexts[:1], cat, cand_cols, chunk)    # a single user
            assert_catalogue_equal(scorer.top_catalogue(contexts[:1], ns[0], chunk=chunk, scores=True), reference_pages(one, ns[0]), "R = 1")


# ---- 5. graphs (GPU only) ------------------------------------------------------------------------------------------------------------------
def check_catalogue_graphs(name, gpu, lib, n=5, n_pool=14):
    """top_catalogue on a graph=True scorer goes through score_requests' bucket graphs: the first call warms the 64-row bucket up (two
    passes of 48 rows), the second captures and replays it, the third captures and replays the 16-row bucket (the pass of 15 rows) as
    well.  Every call equals, bit for bit, the eager launches over the same padded rows on a graph=False scorer — the pad request
    spelled out with another row —, and lies within the eval forward's margin of the unpadded eager call; again with exclusion lists,
    and after append, relabel_where and set_catalogue with a new catalogue.  A direct score_requests call of the bucket uses the
    graph top_catalogue captured."""
    from rat_amd.online import OnlineScorer, _BucketGraph
    assert gpu >= 0
    case, model, data, pool, cols, cfg = rq._setup(name, gpu, n_pool=n_pool)
    cur = [pool[:n_pool].copy()]
    scorer = OnlineScorer(model, cur[0], cfg, graph=True, lib=lib, capacity=n_pool + 8)
    live = cur[0]
    cat, cand_cols = _catalogue(live, cols)
    contexts = _contexts(data, live, cols, cand_cols)
    filler = live[-1, :-1]
    scorer.set_catalogue(cat, cand_cols)
    per = None
    other = ("_graphs", "_rows_graphs", "_same_graphs", "_same_rows_graphs", "_top_graphs", "_top_cand_graphs", "_rank_graphs", "_rank_cand_graphs")

    def fresh():
        return OnlineScorer(model, cur[0], cfg, graph=False, lib=lib)

    def captured():
        return sorted(k[0] for k, e in scorer._bucket_graphs.items() if isinstance(e[1], _BucketGraph))

    def check(tag, cat_now, exclude=True):
        f = fresh()
        f.set_catalogue(cat_now, cand_cols)
        full = reference_scores(f, contexts, cat_now, cand_cols, CHUNK, pad_filler=filler)
        want = reference_pages(full, n)
        got = scorer.top_catalogue(contexts, n, chunk=CHUNK, scores=True)
        assert_catalogue_equal(got, want, tag)
        loose = f.top_catalogue(contexts, n, chunk=CHUNK, scores=True)
        worst = float((got[3] - loose[3]).abs().max())
        print("replayed top_catalogue vs unpadded eager top_catalogue, %s: worst |dy| = %.3g" % (tag, worst))
        assert worst <= EVAL_GATE, (tag, worst)
        if exclude:
            p = _exclusions(want)
            ex_want = reference_pages(full, n, per_request=p)
            ex = (np.asarray([i for q in p for i in q]), np.concatenate([[0], np.cumsum([len(q) for q in p])]))
            assert_catalogue_equal(scorer.top_catalogue(contexts, n, chunk=CHUNK, exclude=ex, scores=True), ex_want, tag + " exclude")
        assert all(len(getattr(scorer, k)) == 0 for k in other), "top_catalogue touched another call's graphs"
        return got

    assert scorer.graph_warmup == 2
    first = check("first call", cat, exclude=False)                           # passes of 48, 48, 15 rows: bucket 64 twice, bucket 16 once
    assert captured() == []
    tc.assert_same_result(check("second call", cat, exclude=False), first, "second call")
    assert captured() == [64]
    tc.assert_same_result(check("third call", cat, exclude=False), first, "third call")
    assert captured() == [16, 64]
    graphs = {k: e[1] for k, e in scorer._bucket_graphs.items()}
    tc.assert_same_result(check("fourth call", cat), first, "fourth call")
    assert {k: e[1] for k, e in scorer._bucket_graphs.items()} == graphs and len(graphs) == 2
    # the graph is score_requests' own: a direct caller of the bucket replays it
    rows, off = _host_rows(contexts, cat, cand_cols, 0, CHUNK)
    y_direct = scorer.score_requests((rows, off))[0]
    assert torch.equal(_bits(y_direct), _bits(first[3][:, :CHUNK].reshape(-1))) and len(scorer._bucket_graphs) == 2
    # the pool, the labels and the catalogue change under the captured graphs
    for step in ("append", "relabel", "catalogue"):
        y_old = scorer.top_catalogue(contexts, n, chunk=CHUNK, scores=True)[3]
        if step == "append":
            rows = data[-3:].copy()
            rows[:, cols] = live[:3][:, cols]                                  # rows the requests will retrieve
            scorer.append(rows)
            cur[0] = np.concatenate([cur[0], rows])
        elif step == "relabel":
            n_ids = cur[0].shape[1] - 1
            keys = cur[0][:6, :-1].astype(np.int64)
            hit = (cur[0][:, None, :-1].astype(np.int64) == keys[None]).all(axis=2).any(axis=1)
            new = 1.0 - float(np.round(cur[0][hit, -1].mean()))
            scorer.relabel_where(list(range(n_ids)), keys, new)
            cur[0] = cur[0].copy()
            cur[0][hit, -1] = new
        else:
            cat, _ = _catalogue(live, cols, shift=2)
            scorer.set_catalogue(cat, cand_cols)
        check("after %s" % step, cat)
        assert {k: e[1] for k, e in scorer._bucket_graphs.items()} == graphs, "%s invalidated a captured chain" % step
        assert not torch.equal(scorer.top_catalogue(contexts, n, chunk=CHUNK, scores=True)[3], y_old), "%s changed no prediction" % step


# ---- 6. refusals and the launch chain ------------------------------------------------------------------------------------------------------
def check_refusals(gpu, lib):
    """every refusal is raised before any entry point of the library is reached"""
    import pytest
    from rat_amd.online import OnlineScorer
    _case, model, data, pool, cols, cfg = rq._setup("tiny_seq_bn", gpu)
    rec = tc.Recorder(lib)
    scorer = OnlineScorer(model, pool[:14], cfg, graph=False, lib=rec)
    rec.take()
    live = pool[:14]
    cat, cand_cols = _catalogue(live, cols, M=9)
    contexts = _contexts(data, live, cols, cand_cols, R=2)
    L = contexts.shape[1]
    items, off = np.array([0, 8, 3, 3, 1, 2]), [0, 2, 6]

    def refused(exc, word, fn):
        with pytest.raises(exc, match=word):
            fn()
        assert rec.take() == [], "a refused call reached the library"
    # no catalogue yet
    refused(ValueError, "no catalogue", lambda: scorer.top_items(contexts, items, off, 3))
    refused(ValueError, "no catalogue", lambda: scorer.rank_items(contexts, items, off))
    refused(ValueError, "no catalogue", lambda: scorer.top_catalogue(contexts, 3))
    # set_catalogue
    refused(ValueError, "empty catalogue", lambda: scorer.set_catalogue(cat[:0], cand_cols))
    refused(ValueError, "columns", lambda: scorer.set_catalogue(cat[:, :1], cand_cols))
    refused(ValueError, "columns", lambda: scorer.set_catalogue(cat, list(cand_cols) + [(set(range(L)) - set(cand_cols)).pop()]))
    refused(ValueError, "M, W", lambda: scorer.set_catalogue(cat[:, 0], cand_cols[:1]))
    refused(ValueError, "int32", lambda: scorer.set_catalogue(np.where(cat == cat[0, 0], 2 ** 31, cat), cand_cols))
    refused(ValueError, "int32", lambda: scorer.set_catalogue(np.where(cat == cat[0, 0], -2 ** 31 - 1, cat), cand_cols))
    refused(ValueError, "integers", lambda: scorer.set_catalogue(cat.astype(np.float64), cand_cols))
    assert len(cand_cols) == 2
    for bad, word in (([], "non-empty"), ([cand_cols[0]] * 2, "repeated"), ([0.0], "integer"), ([L], "outside"), ([-1], "outside"), ([[0]], "1-D")):
        refused(ValueError, word, lambda: scorer.set_catalogue(cat[:, :len(bad)] if len(bad) else cat, bad))
    assert scorer.catalogue_size == 0
    scorer.set_catalogue(cat, cand_cols)
    assert scorer.catalogue_size == 9 and rec.take() == []
    # contexts
    for fn in (lambda c: scorer.top_items(c, items, off, 3), lambda c: scorer.rank_items(c, items, off), lambda c: scorer.top_catalogue(c, 3)):
        refused(ValueError, "columns", lambda: fn(contexts[:, :-1]))
        refused(ValueError, "R, L", lambda: fn(contexts[0]))
        refused(ValueError, "R, L", lambda: fn(contexts[:0]))
    refused(ValueError, "one encoded row per request", lambda: scorer.top_items(contexts[:1], items, off, 3))
    refused(ValueError, "one encoded row per request", lambda: scorer.rank_items(np.concatenate([contexts, contexts]), items, off))
    # items and offsets
    for bad, word in ((np.array([0, 9, 3, 3, 1, 2]), "outside"), (np.array([0, -1, 3, 3, 1, 2]), "outside"), (items.astype(np.float64), "integers"),
                      (items.reshape(2, 3), "1-D"), (np.zeros(0, dtype=np.int64), "empty request")):
        refused(ValueError, word, lambda: scorer.top_items(contexts, bad, off if len(bad) else [0, 0, 0], 3))
        refused(ValueError, word, lambda: scorer.rank_items(contexts, bad, off if len(bad) else [0, 0, 0]))
    refused(ValueError, "end at", lambda: scorer.top_items(contexts, items, [0, 2, 5], 3))
    refused(ValueError, "empty request", lambda: scorer.rank_items(contexts, items, [0, 6, 6]))
    # n, as _top_n refuses it
    for bad, word in ((2.5, "integer"), ("3", "integer"), (None, "integer"), (True, "integer"), (0, "MAX_TOPN"), (-1, "MAX_TOPN"), (65, "MAX_TOPN")):
        refused(ValueError, word, lambda: scorer.top_items(contexts, items, off, bad))
        refused(ValueError, word, lambda: scorer.top_catalogue(contexts, bad))
    # chunk
    for bad in (0, -1, 2.5, "3", True, np.float32(2)):
        refused(ValueError, "chunk", lambda: scorer.top_catalogue(contexts, 3, chunk=bad))
    # exclude
    for bad, word in ((([0, 9], [0, 1, 2]), "outside"), (([-1], [0, 1, 1]), "outside"), (([0, 1], [0, 1]), "ex_offsets"), (([0, 1], [0, 2, 1]), "ascend"),
                      (([0, 1], [1, 1, 2]), "ascend"), (([0, 1], [0, 1, 3]), "ascend"), (([0.5], [0, 1, 1]), "ex_items"), (([[0]], [0, 1, 1]), "ex_items"),
                      (([0], [0.0, 1.0, 1.0]), "ex_offsets"), ([0, 1, 1], "pair"), (np.array([0, 1]), "pair")):
        refused(ValueError, word, lambda: scorer.top_catalogue(contexts, 3, exclude=bad))
    # same= / before= are not offered
    refused(TypeError, "same", lambda: scorer.top_items(contexts, items, off, 3, same=[cols[0]]))
    refused(TypeError, "before", lambda: scorer.rank_items(contexts, items, off, before=[0] * 6))
    refused(TypeError, "same", lambda: scorer.top_catalogue(contexts, 3, same=[cols[0]]))
    model.train()
    refused(RuntimeError, "needs the model in eval mode", lambda: scorer.top_items(contexts, items, off, 3))
    refused(RuntimeError, "needs the model in eval mode", lambda: scorer.rank_items(contexts, items, off))
    refused(RuntimeError, "needs the model in eval mode", lambda: scorer.top_catalogue(contexts, 3))
    model.eval()
    got = scorer.top_items(contexts, items, off, 3)                                # and good ones go through
    assert tuple(got[0].shape) == (2, 3) and got[2].cpu().tolist() == [2, 3] and rec.take()
    got = scorer.top_catalogue(contexts, 3, chunk=4, exclude=([8, 0], [0, 0, 2]))
    assert tuple(got[0].shape) == (2, 3) and got[2].cpu().tolist() == [3, 3] and not np.isin(got[0][1].cpu().numpy(), [0, 8]).any() and rec.take()


def check_launch_chain(gpu, lib, form, n_pool=14):
    """top_items / rank_items reach rat_catalogue_expand, then top_requests' / rank_requests' entry points in their order; every pass
    of top_catalogue reaches rat_catalogue_expand, score_requests' entry points, (rat_topn_exclude,) rat_topn_seg, rat_topn_merge.
    The reference lists are recorded from the older calls themselves, on the same scorer."""
    from rat_amd.online import OnlineScorer
    _case, model, data, pool, cols, cfg = rq._setup("tiny_seq_bn", gpu, n_pool=n_pool)
    first, kw, later, live = rq._form(form, pool, n_pool)
    rec = tc.Recorder(lib)
    scorer = OnlineScorer(model, first, cfg, graph=False, lib=rec, **kw)
    if later is not None:
        scorer.append(later)
    rec.take()
    cat, cand_cols = _catalogue(live, cols)
    contexts = _contexts(data, live, cols, cand_cols)
    scorer.set_catalogue(cat, cand_cols)
    assert rec.take() == []
    items, off = np.array([0, 36, 5, 5, 1, 2, 7, 30]), np.array([0, 3, 4, 8])
    rows = np.repeat(contexts, np.diff(off), axis=0)
    rows[:, list(cand_cols)] = cat[items]
    scorer.top_requests((rows, off), 3)
    top_chain = rec.take()
    scorer.rank_requests((rows, off))
    rank_chain = rec.take()
    assert top_chain[-1] == "rat_topn_seg" and rank_chain[-1] == "rat_rank_seg" and "rat_catalogue_expand" not in top_chain + rank_chain
    scorer.top_items(contexts, items, off, 3)
    assert rec.take() == ["rat_catalogue_expand"] + top_chain
    scorer.rank_items(contexts, items, off)
    assert rec.take() == ["rat_catalogue_expand"] + rank_chain
    chains = []
    chunk = 20                                                                 # two passes: 20 and 17 items per request
    reference_scores(scorer, contexts, cat, cand_cols, chunk, on_pass=lambda: chains.append(rec.take()))
    assert len(chains) == 2 and all(len(c) >= 3 for c in chains)
    new = ("rat_catalogue_expand", "rat_topn_exclude", "rat_topn_seg", "rat_topn_merge")
    assert not any(name in new for c in chains for name in c)
    scorer.top_catalogue(contexts, 3, chunk=chunk)
    assert rec.take() == sum((["rat_catalogue_expand"] + c + ["rat_topn_seg", "rat_topn_merge"] for c in chains), [])
    scorer.top_catalogue(contexts, 3, chunk=chunk, exclude=([4], [0, 0, 1, 1]), scores=True)
    assert rec.take() == sum((["rat_catalogue_expand"] + c + ["rat_topn_exclude", "rat_topn_seg", "rat_topn_merge"] for c in chains), [])
