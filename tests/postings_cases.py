"""Checks of the candidate retrieval through posting lists (``rat_bm25_topk_postings``; ``ops.bm25_topk_postings``;
``RetrievalIndex.build_postings`` / ``retrieve_shared``; ``postings=True`` of ``OnlineScorer.top_candidates`` / ``rank_candidates`` /
``top_items`` / ``rank_items`` / ``top_catalogue``), shared by tests/test_postings.py (CPU, host-emulation build) and
tests/test_gpu_postings.py (MI355X).

Every comparison is bit for bit.  The oracle of the kernel is a plain numpy restatement of ``rat_bm25_topk``'s contract — fp64 sums with f
ascending, zero scores dropped, ``np.lexsort((index, -score))[:K]`` — over the live rows, never the code under test;
``ops.bm25_topk_split`` over the same query tables is a second witness.  The oracle of a scorer call with ``postings=True`` is the same
call with ``postings=False``.  The only tolerance in this file is the eval forward's recorded margin (``EVAL_GATE``), where a replayed,
padded prediction vector is compared with an unpadded one."""
import ctypes
import functools

import numpy as np
import torch

import catalogue_cases as cc
import online_requests_cases as rq
import online_top_cases as tc

EVAL_GATE = rq.EVAL_GATE
SEED = 20261
N_POOL = 300
TAIL = 50                                   # n_sorted = N - 50: the last 50 rows are the lists' tail
CAPACITY = N_POOL + 12                      # the slots past the live rows hold ids that would win
VOCABS = (3, 40, 7, 1)                      # the last column: one id, weight log(N / N) = 0.0 everywhere
F = len(VOCABS)
KS = (1, 3, 8, 32)
SIZES = (1, 2, 7, 70)                       # rows per request
ABSENT = (9, 45, 99, 5)                     # per column an id no pool row holds
# (name, the varying columns of the ENCODED row — L = 6 here, the used columns are 0 .. 3 —, their mask over the used columns)
VARYING = (("col1", [1], 0b0010), ("col0", [0], 0b0001), ("col12", [1, 2], 0b0110), ("all", [0, 1, 2, 3], 0b1111), ("unused", [5], 0))
ROW_LEN = 6


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.array(a))                                          # (a copy: the cached inputs are read-only)
    return (t if dtype is None else t.to(dtype)).to(device)


# ---- the numpy oracle --------------------------------------------------------------------------------------------------------------------
def reference_scores(db, qry_ids, qry_idf):
    """-> fp64 [Q, N]: score[b, n] = sum over f ascending of (db[n, f] == qry_ids[b, f]) * qry_idf[b, f]"""
    s = np.zeros((len(qry_ids), len(db)), dtype=np.float64)
    for f in range(db.shape[1]):
        s = s + np.where(db[None, :, f] == qry_ids[:, None, f], qry_idf[:, None, f], 0.0)
    return s


def reference_topk(scores, K, rows=None):
    """rat_bm25_topk's contract over the rows ``rows`` (default: all) of a score table -> (values [Q, K], indices [Q, K], lens [Q])"""
    Q, N = scores.shape
    rows = np.arange(N) if rows is None else np.asarray(rows, dtype=np.int64)
    values, indices, lens = np.zeros((Q, K)), np.full((Q, K), -1, dtype=np.int64), np.zeros(Q, dtype=np.int64)
    for b in range(Q):
        s = scores[b, rows]
        keep = np.nonzero(s > 0)[0]
        order = keep[np.lexsort((rows[keep], -s[keep]))][:K]
        lens[b] = len(order)
        values[b, :len(order)], indices[b, :len(order)] = s[order], rows[order]
    return values, indices, lens


def assert_topk_equal(got, want, what):
    v, i, n = (t.cpu() for t in got)
    assert v.dtype == torch.float64 and i.dtype == torch.int64 and n.dtype == torch.int64, what
    assert torch.equal(n, torch.from_numpy(want[2])), (what, "lens")
    assert torch.equal(i, torch.from_numpy(want[1])), (what, "indices")
    assert torch.equal(v.view(torch.int64), torch.from_numpy(want[0]).view(torch.int64)), (what, "value bits")


# ---- the kernel's inputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_table():
    """-> the pool [N, L + 1] (label last; columns 4 and 5 are not used columns), read-only"""
    rng = np.random.default_rng(SEED)
    pool = np.stack([rng.integers(0, v, size=N_POOL) for v in VOCABS] + [rng.integers(0, 11, size=N_POOL), rng.integers(0, 11, size=N_POOL),
                                                                            rng.integers(0, 2, size=N_POOL)], axis=1).astype(np.int64)
    # rows 10 and 260 — an indexed row and a tail row — are alike in the used columns: whatever one scores the other scores
    pool[260, :F] = pool[10, :F]
    # id 39 of column 1 stands in two rows only, one of them in the tail: a posting list shorter than every K > 2
    pool[pool[:, 1] == 39, 1] = 38
    pool[[20, 270], 1] = 39
    pool.setflags(write=False)
    return pool


@functools.lru_cache(maxsize=None)
def request_rows(name):
    """-> (ids int64 [80, L], offsets [5]) for one varying set: four requests of 1, 2, 7 and 70 rows, each one context row with the
    varying columns swapped.  Request 1 (2 rows) has a context that matches nothing; an id absent from the pool stands at the head row of
    request 2 and at a later row of request 3, and at a later row of request 2 where its head row hits (both directions of the dtype rule)."""
    cols = dict((n, c) for n, c, _m in VARYING)[name]
    pool = pool_table()
    rng = np.random.default_rng(SEED + 1 + [n for n, _c, _m in VARYING].index(name))
    parts = []
    for r, m in enumerate(SIZES):
        ctx = pool[(17 * r + 3) % N_POOL, :ROW_LEN].copy()
        if r == 1:
            ctx[:F] = ABSENT                                                   # no pool row equals this context in any column
            ctx[3] = 0 if 3 in cols else ABSENT[3]
        rows = np.repeat(ctx[None], m, axis=0)
        for c in cols:
            if c < F:                                                          # ids of pool rows (so that lists are hit), some absent ones
                rows[:, c] = pool[rng.integers(0, N_POOL, size=m), c]
                rows[rng.random(m) < 0.1, c] = ABSENT[c]
            else:
                rows[:, c] = rng.integers(0, 11, size=m)
        if r == 1 and 1 in cols:
            rows[1, 1] = 39                                                    # ... and a candidate id that two pool rows hold
        if r == 2:
            for c in cols:
                if c < F - 1:
                    rows[0, c] = ABSENT[c]                                     # the head row misses: the column's weights are truncated
                    rows[1, c] = pool[4, c]
        if r == 3:
            for c in cols:
                if c < F - 1:
                    rows[0, c], rows[5, c] = pool[10, c], ABSENT[c]            # the head row hits, a later row misses: weight 0.0 for it alone
            if name == "col12":
                rows[1, 1], rows[1, 2] = pool[10, 1], pool[10, 2]              # row 10 stands in both posting lists of this query
        parts.append(rows)
    ids = np.concatenate(parts)
    ids.setflags(write=False)
    return ids, np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)


def eighths(qry_ids):
    """weights replaced by multiples of 1/8, a function of (column, id) only — so rows that share an id share its weight —, 0.0 in the
    last column: scores tie"""
    w = ((qry_ids.astype(np.int64) * 3 + np.arange(F)[None] * 5) % 4 + 1) / 8.0
    w[:, F - 1] = 0.0
    return w


class KernelCase:
    """one (varying set, weights) pair on a device: the index, the query tables from the real rat_bm25_query_prepare_seg, the numpy
    scores of every (query, live row), and the posting lists / context lists per n_sorted"""

    def __init__(self, device, lib, name, weights="idf"):
        from rat_amd import ops
        from rat_amd.online import RetrievalIndex
        self.device, self.lib, self.name = device, lib, name
        self.cols, self.mask = dict((n, (c, m)) for n, c, m in VARYING)[name]
        pool = pool_table()
        self.db = pool[:, :F]
        self.index = RetrievalIndex(pool, list(range(F)), 1, device, lib=lib, capacity=CAPACITY)
        ids, self.off = request_rows(name)
        self.first = np.repeat(self.off[:-1], np.diff(self.off))
        self.heads = self.off[:-1]
        t_ids = _dev(ids, device, torch.int32)
        ix = self.index
        self.qry_ids, self.qry_idf = ops.bm25_query_prepare(t_ids, ix.cols, ix.table_ids, ix.table_idf, ix.table_offsets,
                                                            first_row=_dev(self.first, device), lib=lib)
        self.np_ids = self.qry_ids.cpu().numpy()
        assert np.array_equal(self.np_ids, ids[:, :F])
        if weights == "eighths":
            self.qry_idf = _dev(eighths(self.np_ids), device)
        self.np_idf = self.qry_idf.cpu().numpy()
        assert (self.np_idf >= 0).all() and (self.np_idf[:, F - 1] == 0).all()
        self.scores = reference_scores(self.db, self.np_ids, self.np_idf)
        # the slots past the live rows: ids every query of request 3 would score highest on
        self.db_t = ix.db_t.clone()
        self.db_t[:, N_POOL:] = _dev(self.np_ids[self.heads[3]], device)[:, None]
        self.count = ix.count.clone()
        # the precondition, established here: inside a request the rows are equal outside the varying columns, and so are their weights
        fixed = [f for f in range(F) if not (self.mask >> f) & 1]
        assert np.array_equal(self.np_ids[:, fixed], self.np_ids[self.first][:, fixed])
        assert np.array_equal(self.np_idf[:, fixed], self.np_idf[self.first][:, fixed])

    def context_scores(self):
        """a(n): the head rows' scores with the varying weights at 0.0 -> fp64 [R, N]"""
        w = self.np_idf[self.heads].copy()
        w[:, [f for f in range(F) if (self.mask >> f) & 1]] = 0.0
        return reference_scores(self.db, self.np_ids[self.heads], w), w

    def lists(self, n_sorted, K):
        """-> (post_ids, post_rows int32 [F, capacity], n_sorted int64 [1], T int64 [R, K], ctx_row int64 [Q]) on the device, built in
        numpy: the stable sort of rows [0, n_sorted) per column — the slots past it hold a winning id and a row past the live rows —,
        and T from the numpy oracle over the indexed rows"""
        post_ids = np.zeros((F, CAPACITY), dtype=np.int32)
        post_rows = np.zeros((F, CAPACITY), dtype=np.int32)
        for f in range(F):
            order = np.argsort(self.db[:n_sorted, f], kind="stable")
            post_ids[f, :n_sorted], post_rows[f, :n_sorted] = self.db[:n_sorted, f][order], order
            post_ids[f, n_sorted:], post_rows[f, n_sorted:] = self.np_ids[self.heads[3], f], N_POOL + 1
        a, _w = self.context_scores()
        T = reference_topk(a, K, rows=np.arange(n_sorted))[1]
        ctx_row = np.searchsorted(self.heads, self.first)
        dev = self.device
        return (_dev(post_ids, dev), _dev(post_rows, dev), _dev(np.array([n_sorted], dtype=np.int64), dev), _dev(T, dev), _dev(ctx_row, dev)), T

    def sources(self, n_sorted, K, T, want):
        """per query, where the rows of the expected result come from -> bool [Q, K] x 3: a posting list, the context list only, the tail"""
        idx = want[1]
        valid = idx >= 0
        safe = np.where(valid, idx, 0)
        vary = [f for f in range(F) if (self.mask >> f) & 1]
        hit = np.zeros(idx.shape, dtype=bool)
        for f in vary:
            hit |= self.db[safe, f] == self.np_ids[:, None, f]
        in_T = np.zeros(idx.shape, dtype=bool)
        for b in range(len(idx)):
            in_T[b] = np.isin(idx[b], T[np.searchsorted(self.heads, self.first[b])])
        tail = valid & (idx >= n_sorted)
        posting = valid & ~tail & hit
        return posting, valid & ~tail & ~hit & in_T, tail, valid & ~tail & hit & in_T

    def run(self, n_sorted, K, host_form):
        from rat_amd import ops
        (post_ids, post_rows, ns, T_dev, ctx_row), T = self.lists(n_sorted, K)
        form = dict(n_rows=N_POOL) if host_form else dict(header=self.count)
        got = ops.bm25_topk_postings(self.db_t, post_ids, post_rows, ns, self.qry_ids, self.qry_idf, self.mask, T_dev, ctx_row, lib=self.lib,
                                     **form)
        return got, T


def n_sorted_values(K):
    return sorted({0, 1, K - 1, N_POOL - TAIL, N_POOL})


def check_kernel(device, lib, K, full=True):
    """every varying set at every n_sorted (``full=False``: every set at N - 50, and one set at the other values) against the numpy
    oracle, both pool forms; the existing scans are a second witness of the oracle and of the context lists"""
    from rat_amd import ops
    seen = dict(three_sources=False, in_T_and_posting=False, two_lists=False, short=False, empty=False, nothing_matches=False,
                absent_head=False, absent_later=False)
    launches = 0
    for name, _cols, mask in VARYING:
        case = KernelCase(device, lib, name)
        want = reference_topk(case.scores, K)
        # second witness: the split scan over the same query tables and the live rows
        assert_topk_equal(ops.bm25_topk_split(case.db_t, case.qry_ids, case.qry_idf, K, header=case.count, lib=lib), want, (name, K, "scan"))
        # the inputs hold what the cases are about
        ids = case.np_ids
        hits = np.stack([np.isin(ids[:, f], case.db[:, f]) for f in range(F)], axis=1)
        vary = [f for f in range(F - 1) if (mask >> f) & 1]
        for f in vary:
            seen["absent_head"] |= bool((~hits[case.first, f] & hits[:, f]).any())         # the head misses where a later row hits
            seen["absent_later"] |= bool((hits[case.first, f] & ~hits[:, f]).any())        # ... and the other way round
        a, _w = case.context_scores()
        seen["nothing_matches"] |= bool((a[1] == 0).all())
        seen["short"] |= bool(((want[2] > 0) & (want[2] < K)).any())
        seen["empty"] |= bool((want[2] == 0).any())
        if name == "col12":
            b = int(case.off[3]) + 1
            both = (case.db[:, 1] == ids[b, 1]) & (case.db[:, 2] == ids[b, 2])
            seen["two_lists"] |= bool(both[:N_POOL - TAIL].any())
            assert both[10] and (K < 3 or 10 in want[1][b]), "the row in two posting lists is not in the result"
        for n_sorted in (n_sorted_values(K) if full or name == "col12" else [N_POOL - TAIL]):
            got, T = case.run(n_sorted, K, host_form=launches % 2 == 0)
            launches += 1
            assert_topk_equal(got, want, (name, K, n_sorted))
            if n_sorted == N_POOL - TAIL:
                posting, ctx_only, tail, both = case.sources(n_sorted, K, T, want)
                seen["three_sources"] |= bool((posting.any(axis=1) & ctx_only.any(axis=1) & tail.any(axis=1)).any())
                seen["in_T_and_posting"] |= bool(both.any())
                if name == "all":
                    assert (T == -1).all(), "every column varies: the context lists are empty"
                if name == "unused":
                    assert not posting.any() and mask == 0
            # the context lists the kernel was given are what the existing horizon scan returns for the head rows
            if n_sorted > 0 and name in ("col1", "col12"):
                a, w = case.context_scores()
                scan = ops.bm25_topk_split(case.db_t, case.qry_ids[_dev(case.heads, device)].contiguous(), _dev(w, device), K,
                                           before=_dev(np.full(len(case.heads), n_sorted, dtype=np.int64), device), header=case.count, lib=lib)
                assert torch.equal(scan[1].cpu(), torch.from_numpy(T)), (name, K, n_sorted, "T")
    needed = set(seen) - ({"three_sources", "short"} if K == 1 else set())     # a page of one entry has one source and no shorter list
    missing = sorted(k for k in needed if not seen[k])
    assert not missing, "K = %d: the inputs never reach %s" % (K, missing)


def check_ties(device, lib):
    """weights in eighths: scores tie, and the K-th place is decided by the index between a row that comes from the context list only
    and a row that comes from a posting list — once with each holding the lower index"""
    seen = {"posting_first": False, "context_first": False}
    for K in (3, 8):
        for name in ("col1", "col12"):
            case = KernelCase(device, lib, name, weights="eighths")
            more = reference_topk(case.scores, K + 1)
            want = reference_topk(case.scores, K)
            for n_sorted in (N_POOL, N_POOL - TAIL):
                got, T = case.run(n_sorted, K, host_form=n_sorted == N_POOL)
                assert_topk_equal(got, want, ("eighths", name, K, n_sorted))
                if n_sorted != N_POOL:
                    continue
                posting, ctx_only, _tail, _both = case.sources(n_sorted, K + 1, T, more)
                tie = (more[2] == K + 1) & (more[0][:, K - 1] == more[0][:, K])
                seen["posting_first"] |= bool((tie & posting[:, K - 1] & ~posting[:, K]).any())
                # (the row just outside the page: not a posting row; it stood in T or was pushed out of it by rows that are in the page)
                seen["context_first"] |= bool((tie & ctx_only[:, K - 1] & posting[:, K]).any())
    assert all(seen.values()), "no tie straddles the K-th place in both orders: %s" % seen


def check_long_lists(device, lib, N=5000, K=8):
    """a two-valued varying column: posting lists of about N / 2 rows, forty trips of a wave"""
    from rat_amd import ops
    from rat_amd.online import RetrievalIndex
    rng = np.random.default_rng(SEED + 50)
    pool = np.stack([rng.integers(0, 2, size=N), rng.integers(0, 50, size=N), rng.integers(0, 9, size=N), rng.integers(0, 2, size=N)], axis=1)
    index = RetrievalIndex(pool, [0, 1, 2], K, device, lib=lib, capacity=N + 100)
    index.build_postings()
    assert index.postings_rows == N
    tail = np.stack([rng.integers(0, 2, size=60), rng.integers(0, 50, size=60), rng.integers(0, 9, size=60), rng.integers(0, 2, size=60)], axis=1)
    index.append(tail)
    live = np.concatenate([pool, tail])
    sizes = (5, 1, 6)
    rows = np.concatenate([np.repeat(live[[N + 7 * r + 1], :3], m, axis=0) for r, m in enumerate(sizes)])   # contexts of tail rows
    rows[:, 0] = np.arange(len(rows)) % 2
    rows[3, 0] = 7                                                             # absent: this row's list is empty
    off = np.concatenate([[0], np.cumsum(sizes)])
    got = index.retrieve_shared(rows, off, [0])
    first = np.repeat(off[:-1], np.diff(off))
    qi, qw = ops.bm25_query_prepare(_dev(rows, device, torch.int32), index.cols, index.table_ids, index.table_idf, index.table_offsets,
                                    first_row=_dev(first, device), lib=lib)
    want = reference_topk(reference_scores(live[:, :3], qi.cpu().numpy(), qw.cpu().numpy()), K)
    assert ((live[:N, 0] == 0).sum() > 2000) and ((live[:N, 0] == 1).sum() > 2000) and (want[1] >= N).any()
    assert_topk_equal(got, want, "long lists")
    assert_topk_equal(index.retrieve(rows, request_offsets=off), want, "long lists, the scan")


# ---- the index: build_postings and retrieve_shared -------------------------------------------------------------------------------------------
def check_index(device, lib):
    """build_postings equals the stable sort in numpy, keeps its buffers over a rebuild, reports its rows; retrieve_shared equals
    retrieve(ids, request_offsets) and the numpy oracle in every form it serves, before and after an append and a rebuild"""
    import pytest
    from rat_amd import ops
    from rat_amd.online import RetrievalIndex
    pool = pool_table()
    K = 8
    for capacity in (None, CAPACITY):
        n0 = N_POOL if capacity is None else N_POOL - TAIL
        index = RetrievalIndex(pool[:n0], list(range(F)), K, device, lib=lib, capacity=capacity)
        assert index.postings_rows is None
        with pytest.raises(ValueError, match="build_postings"):
            index.retrieve_shared(request_rows("col1")[0], request_rows("col1")[1], [1])
        index.build_postings()
        assert index.postings_rows == n0
        buffers = [t.data_ptr() for t in index._post]

        def sorted_ok(n):
            post_ids, post_rows, n_sorted = (t.cpu().numpy() for t in index._post)
            assert int(n_sorted[0]) == n and post_ids.shape == tuple(index.db_t.shape)
            for f in range(F):
                order = np.argsort(pool[:n, f], kind="stable")
                assert np.array_equal(post_rows[f, :n], order) and np.array_equal(post_ids[f, :n], pool[:n, f][order]), f

        def retrieval_ok(live, tag):
            for name, cols, _mask in VARYING:
                ids, off = (np.array(a) for a in request_rows(name))
                want = index.retrieve(ids, request_offsets=off)
                for given in ((ids, off), (_dev(ids, device), _dev(off, device)))[:2 if name == "col12" else 1]:
                    got = index.retrieve_shared(given[0], given[1], cols)
                    for g, w in zip(got, want):
                        assert g.dtype == w.dtype and torch.equal(g, w), (tag, name)
            ids, off = (np.array(a) for a in request_rows("col1"))             # ... and the numpy oracle over this index's weights
            qi, qw = ops.bm25_query_prepare(_dev(ids, device, torch.int32), index.cols, index.table_ids, index.table_idf, index.table_offsets,
                                            first_row=_dev(np.repeat(off[:-1], np.diff(off)), device), lib=lib)
            want = reference_topk(reference_scores(live[:, :F], qi.cpu().numpy(), qw.cpu().numpy()), K)
            assert_topk_equal(index.retrieve_shared(ids, off, [1]), want, (tag, "numpy"))
        sorted_ok(n0)
        retrieval_ok(pool[:n0], "built")
        if capacity is None:
            with pytest.raises(ValueError, match="capacity"):
                index.append(pool[:1])
            continue
        index.append(pool[n0:])                                                # a real tail
        assert index.postings_rows == n0 and len(index) == N_POOL
        sorted_ok(n0)
        retrieval_ok(pool, "tail")
        index.build_postings()
        assert index.postings_rows == N_POOL and [t.data_ptr() for t in index._post] == buffers, "a rebuild moved the buffers"
        sorted_ok(N_POOL)
        retrieval_ok(pool, "rebuilt")


# ---- corrupt arguments (emulator only) ------------------------------------------------------------------------------------------------------
def reference_contract(db_t, N_live, capacity, post_ids, post_rows, n_sorted, qry_ids, qry_idf, mask, ctx_idx, ctx_row, K):
    """the clamps and skips of rat_bm25_topk_postings restated: the candidate SET of every query under any content of n_sorted,
    post_rows, ctx_indices and ctx_row, scored and ranked by the oracle.  (The corrupt inputs below never offer a row twice.)"""
    Q, n_ctx = len(qry_ids), len(ctx_idx)
    N = min(max(int(N_live), 0), capacity)
    ns = min(max(int(n_sorted), 0), N)
    db = db_t.T
    values, indices, lens = np.zeros((Q, K)), np.full((Q, K), -1, dtype=np.int64), np.zeros(Q, dtype=np.int64)
    vary = [f for f in range(db.shape[1]) if (mask >> f) & 1]
    for b in range(Q):
        cand = []
        for k, f in enumerate(vary):
            lo = np.searchsorted(post_ids[f, :ns], qry_ids[b, f], side="left")
            hi = np.searchsorted(post_ids[f, :ns], qry_ids[b, f], side="right")
            for n in post_rows[f, lo:hi].astype(np.int64):
                if 0 <= n < ns and not any(db[n, e] == qry_ids[b, e] for e in vary[:k]):
                    cand.append(int(n))
        c = min(max(int(ctx_row[b]), 0), n_ctx - 1)
        for n in ctx_idx[c]:
            n = int(n)
            if 0 <= n < ns and not any(db[n, e] == qry_ids[b, e] for e in vary):
                cand.append(n)
        cand += list(range(ns, N))
        assert len(set(cand)) == len(cand), ("the corrupt inputs offer a row twice: the restatement does not cover that", b, sorted(cand))
        rows = np.asarray(sorted(cand), dtype=np.int64)
        s = reference_scores(db[rows], qry_ids[b:b + 1], qry_idf[b:b + 1]) if len(rows) else np.zeros((1, 0))
        v, i, n = reference_topk(s, K)
        values[b], lens[b] = v[0], n[0]
        indices[b] = np.where(i[0] >= 0, rows[np.maximum(i[0], 0)] if len(rows) else -1, -1)
    return values, indices, lens


def check_corrupt(lib, guard=4096):
    """the kernel through the C ABI, every buffer between guard regions: ctx_row and ctx_indices out of range (to +-2^63), post_rows out
    of range, shuffled inside a list and pointing at rows that do not hold the id, n_sorted negative, past the live rows and at +-2^63,
    the header's count out of range.  The calls return normally, no guard changes, the inputs are only read, and the outputs are what the
    restated clamps give"""
    FILL = -99
    K = 8
    case = KernelCase("cpu", lib, "col12")
    rng = np.random.default_rng(SEED + 70)
    Q, R = len(case.np_ids), len(case.heads)

    def guarded(values, dtype):
        values = torch.as_tensor(np.ascontiguousarray(values), dtype=dtype).reshape(-1)
        whole = torch.full((values.numel() + 2 * guard,), FILL, dtype=dtype)
        whole[guard:guard + values.numel()] = values
        return whole, whole[guard:guard + values.numel()]

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    n_build = N_POOL - TAIL
    (post_ids, post_rows, _ns, _T, ctx_row), T = case.lists(n_build, K)
    post_ids, post_rows, ctx_row = post_ids.numpy().copy(), post_rows.numpy().copy(), ctx_row.numpy().copy()
    post_ids[:, n_build:] = 2 ** 31 - 1                                        # sorted past the build too: n_sorted may be clamped to N
    db_t = case.db_t.numpy()
    bad_rows = post_rows.copy()
    f = 1
    lo, hi = np.searchsorted(post_ids[f, :n_build], [5, 6])
    bad_rows[f, lo:hi] = bad_rows[f, lo:hi][::-1]                              # a list in another order: the same set
    bad_rows[f, np.searchsorted(post_ids[f, :n_build], 7)] = -1
    bad_rows[f, np.searchsorted(post_ids[f, :n_build], 8)] = -2 ** 31
    bad_rows[f, np.searchsorted(post_ids[f, :n_build], 9)] = 2 ** 31 - 1
    bad_rows[f, np.searchsorted(post_ids[f, :n_build], 10)] = N_POOL + 3       # a slot past the live rows that holds winning ids
    bad_rows[2, :20] = n_build + np.arange(20)                                 # tail rows in a list: skipped, the tail offers them
    bad_T = T.copy()
    bad_T[0, :] = [-2 ** 63, 2 ** 63 - 1, -1, N_POOL, CAPACITY + 5, CAPACITY - 1, 2 ** 40, -2 ** 40][:K]
    bad_T[3, ::2] = rng.permutation(n_build)[:len(bad_T[3, ::2])] + 0          # distinct rows, anywhere in the indexed part
    bad_T[3, 1::2] = -7
    bad_ctx = ctx_row.copy()
    bad_ctx[::5] = [-2 ** 63, 2 ** 63 - 1, -1, R, 2 ** 40, 1, 0, 3, R + 7, -5, 2, 2, 0, 1, 3, 3][:len(bad_ctx[::5])]
    runs = [("clean", post_rows, T, ctx_row, n_build, N_POOL)]
    runs += [("post_rows", bad_rows, T, ctx_row, n_build, N_POOL), ("ctx_indices", post_rows, bad_T, ctx_row, n_build, N_POOL),
             ("ctx_row", post_rows, T, bad_ctx, n_build, N_POOL), ("all", bad_rows, bad_T, bad_ctx, n_build, N_POOL)]
    runs += [("n_sorted=%d" % v, bad_rows, bad_T, bad_ctx, v, N_POOL) for v in (-2 ** 63, -1, 0, 1, N_POOL, N_POOL + 5, 2 ** 63 - 1)]
    runs += [("header=%d" % v, bad_rows, bad_T, bad_ctx, n_build, v) for v in (-2 ** 63, -3, 0, 5, CAPACITY, CAPACITY + 9, 2 ** 63 - 1)]
    for what, rows, ctx, crow, n_sorted, header in runs:
        bufs = dict(db_t=guarded(db_t, torch.int32), header=guarded([header], torch.int64), post_ids=guarded(post_ids, torch.int32),
                    post_rows=guarded(rows, torch.int32), n_sorted=guarded([n_sorted], torch.int64), qry=guarded(case.np_ids, torch.int32),
                    idf=guarded(case.np_idf, torch.float64), ctx=guarded(ctx, torch.int64), crow=guarded(crow, torch.int64),
                    out_v=guarded(np.full(Q * K, 7.0), torch.float64), out_i=guarded(np.full(Q * K, 7), torch.int64),
                    out_l=guarded(np.full(Q, 7), torch.int64))
        before = {k: v[0].clone() for k, v in bufs.items() if not k.startswith("out")}
        lib.call("rat_bm25_topk_postings", p(bufs["db_t"][1]), 1, p(bufs["header"][1]), 0, CAPACITY, p(bufs["post_ids"][1]),
                 p(bufs["post_rows"][1]), p(bufs["n_sorted"][1]), p(bufs["qry"][1]), p(bufs["idf"][1]), case.mask, p(bufs["ctx"][1]),
                 p(bufs["crow"][1]), R, p(bufs["out_v"][1]), p(bufs["out_i"][1]), p(bufs["out_l"][1]), Q, F, K, None)
        for name, (whole, _) in bufs.items():
            assert (whole[:guard] == FILL).all() and (whole[-guard:] == FILL).all(), (name, what)
        for name, t in before.items():
            assert torch.equal(bufs[name][0].view(torch.int64) if t.dtype == torch.float64 else bufs[name][0],
                               t.view(torch.int64) if t.dtype == torch.float64 else t), (name, what)
        want = reference_contract(db_t, header, CAPACITY, post_ids, rows, n_sorted, case.np_ids, case.np_idf, case.mask, ctx, crow, K)
        got = (bufs["out_v"][1].reshape(Q, K), bufs["out_i"][1].reshape(Q, K), bufs["out_l"][1])
        assert_topk_equal(got, want, what)
        if what == "clean":
            assert_topk_equal(got, reference_topk(case.scores, K), "clean through the ABI")


# ---- refusals of the entry point and of its wrapper -------------------------------------------------------------------------------------------
def _small(device):
    """well-formed arguments of ops.bm25_topk_postings, F = 2, capacity = 6, Q = 3, R = 2, K = 4"""
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)      # noqa: E731
    return dict(db_t=z((2, 6), torch.int32), post_ids=z((2, 6), torch.int32), post_rows=z((2, 6), torch.int32), n_sorted=z((1,), torch.int64),
                qry_ids=z((3, 2), torch.int32), qry_idf=z((3, 2), torch.float64), vary_mask=1, ctx_indices=z((2, 4), torch.int64),
                ctx_row=z((3,), torch.int64))


def check_abi_refusals(device, lib):
    """a null pointer, the ring form, a bad form or header, dims out of range: -1 and a message that names the entry point, nothing
    launched (the outputs keep their fill)"""
    a = _small(device)
    out = (torch.full((3, 4), 7.0, dtype=torch.float64, device=device), torch.full((3, 4), 7, dtype=torch.int64, device=device),
           torch.full((3,), 7, dtype=torch.int64, device=device))
    header = torch.tensor([6], dtype=torch.int64, device=device)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    good = [p(a["db_t"]), 1, p(header), 0, 6, p(a["post_ids"]), p(a["post_rows"]), p(a["n_sorted"]), p(a["qry_ids"]), p(a["qry_idf"]), 1,
            p(a["ctx_indices"]), p(a["ctx_row"]), 2, p(out[0]), p(out[1]), p(out[2]), 3, 2, 4, None]
    fn = lib.cdll.rat_bm25_topk_postings
    bad = [(s, None) for s in (0, 2, 5, 6, 7, 8, 9, 11, 12, 14, 15, 16)]
    bad += [(1, 2), (1, 3), (1, -1), (4, 0), (4, 2 ** 31), (13, 0), (13, -1), (17, 0), (17, -4), (18, 0), (18, 33), (19, 0), (19, 33)]
    for slot, value in bad:
        args = list(good)
        args[slot] = value
        assert fn(*args) == -1 and "rat_bm25_topk_postings" in lib.last_error(), (slot, value)
    args = list(good)
    args[1], args[2], args[3] = 0, None, 7                                     # the host form: a row count past the capacity
    assert fn(*args) == -1 and "rat_bm25_topk_postings" in lib.last_error()
    assert all((t == 7).all() for t in out), "a refused call wrote its outputs"
    assert fn(*good) == 0                                                      # and the good call goes through: an empty result
    args = list(good)
    args[1], args[2], args[3] = 0, None, 6
    assert fn(*args) == 0
    if device != "cpu":
        torch.cuda.synchronize()
    assert (out[2] == 0).all() and (out[1] == -1).all() and (out[0] == 0).all()


def check_ops_refusals(device, lib):
    """the wrapper checks shape, dtype, device and contiguity, and reads no contents"""
    import pytest
    from rat_amd import ops
    good = _small(device)
    got = ops.bm25_topk_postings(lib=lib, **good)
    assert tuple(got[0].shape) == (3, 4) and (got[2] == 0).all()
    for key, dtype in (("db_t", torch.int64), ("post_ids", torch.int64), ("post_rows", torch.int16), ("n_sorted", torch.int32),
                       ("qry_ids", torch.int64), ("qry_idf", torch.float32), ("ctx_indices", torch.int32), ("ctx_row", torch.int32)):
        with pytest.raises(TypeError, match=key):
            ops.bm25_topk_postings(lib=lib, **dict(good, **{key: good[key].to(dtype)}))
    with pytest.raises(TypeError, match="ctx_row"):
        ops.bm25_topk_postings(lib=lib, **dict(good, ctx_row=[0, 0, 0]))
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)      # noqa: E731
    for change in (dict(post_ids=z((2, 5), torch.int32)), dict(post_rows=z((1, 6), torch.int32)), dict(db_t=z((33, 6), torch.int32)),
                   dict(db_t=z((6,), torch.int32)), dict(n_sorted=z((0,), torch.int64)), dict(qry_ids=z((3, 3), torch.int32)),
                   dict(qry_idf=z((2, 2), torch.float64)), dict(qry_ids=z((0, 2), torch.int32), qry_idf=z((0, 2), torch.float64)),
                   dict(ctx_indices=z((2, 33), torch.int64)), dict(ctx_indices=z((0, 4), torch.int64)), dict(ctx_indices=z((8,), torch.int64)),
                   dict(ctx_row=z((2,), torch.int64)), dict(ctx_row=z((3, 1), torch.int64)), dict(vary_mask=-1), dict(vary_mask=2 ** 32),
                   dict(vary_mask=1.0), dict(vary_mask=True), dict(db_t=z((6, 2), torch.int32).t()),
                   dict(qry_idf=z((3, 4), torch.float64)[:, ::2])):
        with pytest.raises(ValueError):
            ops.bm25_topk_postings(lib=lib, **dict(good, **change))
    if device != "cpu":
        with pytest.raises(ValueError, match="different devices"):
            ops.bm25_topk_postings(lib=lib, **dict(good, ctx_row=good["ctx_row"].cpu()))
    with pytest.raises(AssertionError):                                        # a header without its word (_pool_form)
        ops.bm25_topk_postings(lib=lib, header=z((0,), torch.int64), **good)


# ---- the scorer ---------------------------------------------------------------------------------------------------------------------------
CHUNKS = (cc.CHUNK, cc.M_CAT, 1)
N_SCORER = 14
SIZES_SCORER = (3, 1, 4, 2, 6, 1, tc.BIG)


def _stages(form, pool, model, cfg, lib, graph=False):
    """the scorer of a form at every stage it is served in -> (tag, scorer, live rows): immutable — built; capacity — built, with a tail
    after an append, and after a second build"""
    from rat_amd.online import OnlineScorer
    n = N_SCORER
    if form == "immutable":
        scorer = OnlineScorer(model, pool[:n], cfg, graph=graph, lib=lib)
        scorer.build_postings()
        assert scorer.index.postings_rows == n
        yield "built", scorer, pool[:n]
        return
    scorer = OnlineScorer(model, pool[:n - 3], cfg, graph=graph, lib=lib, capacity=n + 5)
    assert scorer.index.postings_rows is None
    scorer.build_postings()
    assert scorer.index.postings_rows == n - 3
    yield "built", scorer, pool[:n - 3]
    scorer.append(pool[n - 3:n])
    assert scorer.index.postings_rows == n - 3 and len(scorer.index) == n
    yield "tail", scorer, pool[:n]
    scorer.build_postings()
    assert scorer.index.postings_rows == n
    yield "rebuilt", scorer, pool[:n]


def _same_ranking(got, want, what):
    assert type(got) is type(want) and torch.equal(got.offsets, want.offsets), what
    assert (got.y_pred is None) == (want.y_pred is None), what
    both = [[r.order, r.val, r.rank] + ([r.y_pred] if r.y_pred is not None else []) for r in (got, want)]
    tc.assert_same_result(both[0], both[1], what)


def check_scorer_calls(name, gpu, lib, form, chunks=CHUNKS, n=5, light=False):
    """each of the five calls with postings=True equals the same call with postings=False bit for bit — positions, values, lens and
    scores=True — at every stage of the form.  ``light`` (the emulator): the stage with the most in it only — a capacity pool's lists with
    a tail behind them —, one n, scores=True"""
    _case, model, data, pool, cols, cfg = rq._setup(name, gpu, n_pool=N_SCORER)
    for tag, scorer, live in _stages(form, pool, model, cfg, lib):
        if light and tag != ("tail" if form == "capacity" else "built"):
            continue
        cat, cand_cols = cc._catalogue(live, cols)
        assert any(c in cols for c in cand_cols)
        contexts = cc._contexts(data, live, cols, cand_cols, R=len(SIZES_SCORER))
        C = sum(SIZES_SCORER)
        items = (7 * np.arange(C) + 3) % cc.M_CAT
        off = rq._offsets([np.zeros((m, 1)) for m in SIZES_SCORER])
        candidates = cat[items]
        scorer.set_catalogue(cat, cand_cols)
        what = "%s %s" % (form, tag)
        for scores in ((True,) if light else (False, True)):
            for k in ((3,) if light else (3, 64)):
                tc.assert_same_result(scorer.top_candidates(contexts, candidates, cand_cols, off, k, scores=scores, postings=True),
                                      scorer.top_candidates(contexts, candidates, cand_cols, off, k, scores=scores), what + " top_candidates")
                tc.assert_same_result(scorer.top_items(contexts, items, off, k, scores=scores, postings=True),
                                      scorer.top_items(contexts, items, off, k, scores=scores), what + " top_items")
            _same_ranking(scorer.rank_candidates(contexts, candidates, cand_cols, off, scores=scores, postings=True),
                          scorer.rank_candidates(contexts, candidates, cand_cols, off, scores=scores), what + " rank_candidates")
            _same_ranking(scorer.rank_items(contexts, items, off, scores=scores, postings=True),
                          scorer.rank_items(contexts, items, off, scores=scores), what + " rank_items")
        if gpu >= 0:                                                           # device lists are used unread
            dev = scorer.device
            given = (torch.from_numpy(contexts.astype(np.int32)).to(dev), torch.from_numpy(items).to(dev), torch.from_numpy(off).to(dev))
            tc.assert_same_result(scorer.top_items(*given, 3, scores=True, postings=True), scorer.top_items(contexts, items, off, 3, scores=True),
                                  what + " device lists")
        three = contexts[:cc.R_CAT]
        for chunk in chunks:
            want = scorer.top_catalogue(three, n, chunk=chunk, scores=True)
            got = scorer.top_catalogue(three, n, chunk=chunk, scores=True, postings=True)
            assert tuple(got[3].shape) == (cc.R_CAT, cc.M_CAT)
            tc.assert_same_result(got, want, what + " top_catalogue chunk=%d" % chunk)
            if not light:
                tc.assert_same_result(scorer.top_catalogue(three, n, chunk=chunk, postings=True), want[:3], what + " top_catalogue chunk=%d" % chunk)
        if light:
            continue
        ex = ([int(want[0][0, 0]), 2, 1], [0, 1, 3, 3])
        tc.assert_same_result(scorer.top_catalogue(three, n, chunk=chunks[0], exclude=ex, postings=True),
                              scorer.top_catalogue(three, n, chunk=chunks[0], exclude=ex), what + " top_catalogue exclude")


def check_refusals(gpu, lib):
    """every refusal is raised before any entry point of the library is reached"""
    import pytest
    from rat_amd.online import OnlineScorer, RetrievalIndex
    _case, model, data, pool, cols, cfg = rq._setup("tiny_seq_bn", gpu)
    rec = tc.Recorder(lib)
    live = pool[:N_SCORER]
    cat, cand_cols = cc._catalogue(live, cols, M=9)
    contexts = cc._contexts(data, live, cols, cand_cols, R=2)
    items, off = np.array([0, 8, 3, 3, 1, 2]), [0, 2, 6]

    def refused(exc, word, fn):
        with pytest.raises(exc, match=word):
            fn()
        assert rec.take() == [], "a refused call reached the library"

    def five(scorer, word):
        refused(ValueError, word, lambda: scorer.top_candidates(contexts, cat[items], cand_cols, off, 3, postings=True))
        refused(ValueError, word, lambda: scorer.rank_candidates(contexts, cat[items], cand_cols, off, postings=True))
        refused(ValueError, word, lambda: scorer.top_items(contexts, items, off, 3, postings=True))
        refused(ValueError, word, lambda: scorer.rank_items(contexts, items, off, postings=True))
        refused(ValueError, word, lambda: scorer.top_catalogue(contexts, 3, postings=True))
    # no posting lists yet
    scorer = OnlineScorer(model, live, cfg, graph=False, lib=rec)
    scorer.set_catalogue(cat, cand_cols)
    rec.take()
    five(scorer, "no posting lists")
    ids = np.repeat(contexts[:1], 3, axis=0)
    ids[:, list(cand_cols)] = cat[:3]
    refused(ValueError, "no posting lists", lambda: scorer.index.retrieve_shared(ids, [0, 3], list(cand_cols)))
    # a window
    window = OnlineScorer(model, live, cfg, graph=False, lib=rec, capacity=rq.CAPACITY, window=True)
    window.set_catalogue(cat, cand_cols)
    rec.take()
    refused(ValueError, "window", window.build_postings)
    refused(ValueError, "window", window.index.build_postings)
    assert window.index.postings_rows is None
    five(window, "window")
    refused(ValueError, "window", lambda: window.index.retrieve_shared(ids, [0, 3], list(cand_cols)))
    # retrieve_shared: what it does not offer, a bad varying, rows that do not share their context
    scorer.build_postings()
    rec.take()
    index = scorer.index
    assert isinstance(index, RetrievalIndex)
    refused(ValueError, "same", lambda: index.retrieve_shared(ids, [0, 3], list(cand_cols), same=[cols[0]]))
    refused(ValueError, "before", lambda: index.retrieve_shared(ids, [0, 3], list(cand_cols), before=[0, 0, 0]))
    for bad, word in (([], "non-empty"), ([cand_cols[0]] * 2, "repeated"), ([0.5], "integer"), ([ids.shape[1]], "outside"), ([-1], "outside"),
                      ([[0]], "1-D")):
        refused(ValueError, word, lambda: index.retrieve_shared(ids, [0, 3], bad))
    refused(ValueError, "end at", lambda: index.retrieve_shared(ids, [0, 2], list(cand_cols)))
    refused(ValueError, "empty request", lambda: index.retrieve_shared(ids, [0, 3, 3], list(cand_cols)))
    refused(ValueError, "columns", lambda: index.retrieve_shared(ids[:, :-1], [0, 3], list(cand_cols)))
    fixed = [c for c in cols if c not in cand_cols]
    if fixed:
        broken = ids.copy()
        broken[2, fixed[0]] += 1
        refused(ValueError, "share their context", lambda: index.retrieve_shared(broken, [0, 3], list(cand_cols)))
        got = index.retrieve_shared(broken, [0, 2, 3], list(cand_cols))        # ... as a request of its own the row is fine
        assert rec.take() and tuple(got[1].shape) == (3, index.topK)
    unused = [c for c in range(ids.shape[1]) if c not in cols]
    if unused:                                                                 # a column the index does not use changes nothing: mask 0
        moved = np.repeat(ids[:1], 3, axis=0)
        moved[:, unused[0]] += np.arange(3)
        got = index.retrieve_shared(moved, [0, 3], [unused[0]])
        want = index.retrieve(moved, request_offsets=[0, 3])
        assert all(torch.equal(g, w) for g, w in zip(got, want)) and rec.take()
    model.train()
    refused(RuntimeError, "needs the model in eval mode", lambda: scorer.top_catalogue(contexts, 3, postings=True))
    model.eval()
    got = scorer.top_catalogue(contexts, 3, postings=True)                     # and a good one goes through
    assert tuple(got[0].shape) == (2, 3) and rec.take()


def _shared_chain(chain):
    """a chain of entry points as postings=False records it -> what postings=True must record: every scan of the request chain (its
    workspace query and the entry point) replaced by the horizon scan over the head rows and the posting-list kernel"""
    out = []
    for name in chain:
        if name.startswith("rat_bm25_topk") and name != "rat_bm25_topk_split_workspace":
            out += ["rat_bm25_topk_split_before", "rat_bm25_topk_postings"]
        else:
            out.append(name)
    return out


def check_launch_chain(gpu, lib, form, n_pool=N_SCORER, light=False):
    """postings=False reaches today's entry points, call for call; postings=True reaches the same ones with the scan per row replaced
    by rat_bm25_topk_split_before (the head rows) and rat_bm25_topk_postings"""
    from rat_amd.online import OnlineScorer
    _case, model, data, pool, cols, cfg = rq._setup("tiny_seq_bn", gpu, n_pool=n_pool)
    first, kw, later, live = rq._form(form, pool, n_pool)
    rec = tc.Recorder(lib)
    plain = OnlineScorer(model, first, cfg, graph=False, lib=rec, **kw)         # never builds: what a call reached before this feature
    scorer = OnlineScorer(model, first, cfg, graph=False, lib=rec, **kw)
    scorer.build_postings()
    assert rec.take() == [], "build_postings is torch plumbing: no entry point"
    if later is not None:
        plain.append(later)
        scorer.append(later)
    rec.take()
    cat, cand_cols = cc._catalogue(live, cols)
    contexts = cc._contexts(data, live, cols, cand_cols)
    plain.set_catalogue(cat, cand_cols)
    scorer.set_catalogue(cat, cand_cols)
    items, off = np.array([0, 36, 5, 5, 1, 2, 7, 30]), np.array([0, 3, 4, 8])
    calls = {"top_candidates": lambda s, **k: s.top_candidates(contexts, cat[items], cand_cols, off, 3, **k),
             "rank_candidates": lambda s, **k: s.rank_candidates(contexts, cat[items], cand_cols, off, **k),
             "top_items": lambda s, **k: s.top_items(contexts, items, off, 3, **k),
             "rank_items": lambda s, **k: s.rank_items(contexts, items, off, **k),
             "top_catalogue": lambda s, **k: s.top_catalogue(contexts, 3, chunk=20, **k),
             "top_catalogue exclude": lambda s, **k: s.top_catalogue(contexts, 3, chunk=20, exclude=([4], [0, 0, 1, 1]), scores=True, **k)}
    if light:                                                                  # (the emulator: one top_catalogue)
        del calls["top_catalogue exclude"]
    for what, call in calls.items():
        call(plain)
        before = rec.take()
        assert before and "rat_bm25_topk_postings" not in before
        call(scorer)
        assert rec.take() == before, (what, "without the keyword")
        if not light:
            call(scorer, postings=False)
            assert rec.take() == before, (what, "postings=False")
        call(scorer, postings=True)
        got = rec.take()
        assert got == _shared_chain(before) and got.count("rat_bm25_topk_postings") == (2 if "catalogue" in what else 1), (what, got, before)


# ---- graphs (GPU only) ----------------------------------------------------------------------------------------------------------------------
def check_postings_graphs(name, gpu, lib, n=5):
    """top_catalogue(postings=True) on a graph=True scorer: the first two calls warm the 64-row bucket up eagerly (two passes of 48 rows
    each), then its chain is captured and replayed, then the 16-row bucket's (the pass of 15 rows).  Every call — warm-up and replay —
    equals, bit for bit, the eager launches over the same padded rows on a graph=False scorer without posting lists (the pad request
    spelled out with another row), and lies within the eval forward's margin of the unpadded eager call.  The same graph objects serve
    after an append and after a rebuild, and no other dictionary of graphs gains an entry"""
    from rat_amd.online import OnlineScorer, _SharedGraph
    assert gpu >= 0
    _case, model, data, pool, cols, cfg = rq._setup(name, gpu, n_pool=N_SCORER)
    cur = [pool[:N_SCORER].copy()]
    scorer = OnlineScorer(model, cur[0], cfg, graph=True, lib=lib, capacity=N_SCORER + 8)
    scorer.build_postings()
    live = cur[0]
    cat, cand_cols = cc._catalogue(live, cols)
    contexts = cc._contexts(data, live, cols, cand_cols)
    filler = live[-1, :-1]
    scorer.set_catalogue(cat, cand_cols)
    other = ("_graphs", "_bucket_graphs", "_rows_graphs", "_same_graphs", "_same_rows_graphs", "_top_graphs", "_top_cand_graphs", "_rank_graphs",
             "_rank_cand_graphs")

    def captured():
        return sorted(k[0] for k, e in scorer._postings_graphs.items() if isinstance(e[1], _SharedGraph))

    def check(tag):
        f = OnlineScorer(model, cur[0], cfg, graph=False, lib=lib)
        f.set_catalogue(cat, cand_cols)
        full = cc.reference_scores(f, contexts, cat, cand_cols, cc.CHUNK, pad_filler=filler)
        want = cc.reference_pages(full, n)
        got = scorer.top_catalogue(contexts, n, chunk=cc.CHUNK, scores=True, postings=True)
        cc.assert_catalogue_equal(got, want, tag)
        loose = f.top_catalogue(contexts, n, chunk=cc.CHUNK, scores=True)
        worst = float((got[3] - loose[3]).abs().max())
        print("replayed top_catalogue(postings=True) vs unpadded eager top_catalogue, %s: worst |dy| = %.3g" % (tag, worst))
        assert worst <= EVAL_GATE, (tag, worst)
        assert all(len(getattr(scorer, k)) == 0 for k in other), "top_catalogue(postings=True) touched another call's graphs"
        return got

    assert scorer.graph_warmup == 2
    first = check("first call")                                               # passes of 48, 48, 15 rows: bucket 64 twice, bucket 16 once
    assert captured() == []
    tc.assert_same_result(check("second call"), first, "second call")
    assert captured() == [64]
    tc.assert_same_result(check("third call"), first, "third call")
    assert captured() == [16, 64]
    graphs = {k: e[1] for k, e in scorer._postings_graphs.items()}
    tc.assert_same_result(check("fourth call"), first, "fourth call")
    assert {k: e[1] for k, e in scorer._postings_graphs.items()} == graphs and len(graphs) == 2
    for step in ("append", "rebuild"):
        y_old = scorer.top_catalogue(contexts, n, chunk=cc.CHUNK, scores=True, postings=True)[3]
        if step == "append":
            rows = data[-3:].copy()
            rows[:, cols] = live[:3][:, cols]                                  # rows the requests will retrieve: a real tail
            scorer.append(rows)
            cur[0] = np.concatenate([cur[0], rows])
            assert scorer.index.postings_rows == N_SCORER
        else:
            scorer.build_postings()
            assert scorer.index.postings_rows == N_SCORER + 3
        check("after %s" % step)
        assert {k: e[1] for k, e in scorer._postings_graphs.items()} == graphs, "%s invalidated a captured chain" % step
        if step == "append":
            assert not torch.equal(scorer.top_catalogue(contexts, n, chunk=cc.CHUNK, scores=True, postings=True)[3], y_old), "append changed no prediction"
