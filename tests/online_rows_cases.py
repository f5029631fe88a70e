"""Checks of a pool that looks at itself (``rat_bm25_topk_split_before``, ``rat_pool_gather_rows``; ``RetrievalIndex.retrieve(ids,
before=...)``, ``OnlineScorer.batch_rows`` / ``score_rows`` / ``evaluate_rows``) shared by tests/test_online_rows.py (CPU,
host-emulation build) and tests/test_gpu_online_rows.py (MI355X).

The reference of the scan is the single-range kernel ``rat_bm25_topk`` (the offline kernel, unchanged) over a CONTIGUOUS COPY of the
logical rows [0, h) with the same weights — computed once per (rows, K), shared by the three pool forms, never the horizon scan against
itself.  The reference of the gather is numpy over a host model of the live rows in age order; the reference of a batch is a numpy
assembly from those reference neighbour lists.  Every comparison is exact except the predictions, which are held to the eval forward's
recorded margin.  The ids come from 2 to 6 values per retrieval column, so equal scores are the rule and the tie rule (the older row
wins) decides at the horizon."""
import ctypes

import numpy as np
import torch

import golden_cases as gc
import model_cases as mc
import online_cases as oc
import online_find_cases as fc

FORMS = ("immutable", "capacity", "window")
CASE = "tiny_seq_bn"                 # 6 id columns, 3 of them categorical (the retrieval columns), topK = 3
EVAL_GATE = 2e-6                     # model_cases.check_eval's absolute gate on y_pred, as tests/online_requests_cases.py uses it
N_QUERIES = 9


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _device(gpu):
    return "cpu" if gpu < 0 else "cuda:%d" % gpu


def make_rows(n, seed=5):
    """-> (case, live [n, L + 1] in age order, junk [64, L + 1] (rows that pass through a window and leave), data [24, L + 1], cols)"""
    case = gc.case_by_name(CASE)
    data, pool, cols = oc.make_tables(case, n + 64, 24, seed=seed)
    return case, pool[:n], pool[n:], data, cols


def build_form(form, live, junk, make):
    """``make(rows, **kw)`` builds an index or a scorer; -> the object holding exactly `live`, oldest first, in the given form.  The
    capacity form has grown by an append; the window has been filled past its capacity and evicted, so its head has moved and the
    live rows straddle the end of the buffers."""
    n = len(live)
    if form == "immutable":
        return make(live)
    if form == "capacity":
        obj = make(live[:n - 40], capacity=n + 20)
        obj.append(live[n - 40:])
        return obj
    assert form == "window"
    obj = make(np.concatenate([junk[:40], live[:n - 30]]), capacity=n + 10, window=True)      # full, head 0
    obj.append(live[n - 30:])                                                                   # 30 junk rows leave: head 30
    obj.evict(10)                                                                               # the last junk rows: head 40
    index = getattr(obj, "index", obj)
    assert len(index) == n and index.count.cpu().tolist() == [n, 40] and 40 + n > index.capacity, "the window does not wrap"
    return obj


def self_retrieving_rows(live, cols, K, count):
    """`count` live rows, spread over the pool, that the PLAIN retrieve of their own ids returns: a row matches itself on every column,
    and among the rows that equal it there (equal scores: the older row wins) it is one of the K oldest.  Row 0 is always one."""
    used = live[:, cols].astype(np.int64)
    _u, inverse = np.unique(used, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    rank = np.array([int((inverse[:i] == inverse[i]).sum()) for i in range(len(live))])
    ok = np.flatnonzero(rank < K)
    assert ok[0] == 0 and len(ok) >= count
    picks = sorted({int(ok[j]) for j in np.linspace(0, len(ok) - 1, count).round().astype(int)} | {int(x) for x in ok[:3]})
    return np.array(picks[:3] + picks[3:][-(count - 3):])


def _queries(live, data, rows):
    """ids of N_QUERIES queries: live rows (a row asked about itself: exact matches at and behind its own position) and fresh ones"""
    return np.ascontiguousarray(np.concatenate([live[rows, :-1], data[:N_QUERIES - len(rows), :-1]]))


# ---- the reference: rat_bm25_topk over a contiguous copy of the rows [0, h) ------------------------------------------------------------
class Reference:
    """(query j, horizon h) -> (values [K], indices [K], lens) as rat_bm25_topk answers over live[:h]; one launch per horizon, cached"""

    def __init__(self, lib, device, live, cols, q_ids, q_idf, K):
        self.lib, self.device, self.K, self.n = lib, device, K, len(live)
        self.db = retr_int32(live[:, cols])
        self.q_ids, self.q_idf = q_ids, q_idf
        self._by_h = {}

    def at(self, h):
        h = int(min(max(h, 0), self.n))
        if h not in self._by_h:
            Q = self.q_ids.shape[0]
            if h == 0:                                                         # nobody to retrieve: rat_bm25_topk takes no empty pool
                out = (torch.zeros((Q, self.K), dtype=torch.float64), torch.full((Q, self.K), -1, dtype=torch.int64),
                       torch.zeros(Q, dtype=torch.int64))
            else:
                out = oc.single_range_topk(self.lib, _up(self.db[:h].T, self.device), self.q_ids, self.q_idf, self.K)
            self._by_h[h] = tuple(t.cpu() for t in out)
        return self._by_h[h]

    def score(self, j, row):
        """query j's score of live row `row`: the kernel's sum, f ascending, in float64"""
        q, w, s = self.q_ids[j].cpu().numpy(), self.q_idf[j].cpu().numpy(), 0.0
        for f in range(len(q)):
            s += float(w[f]) if q[f] == self.db[row, f] else 0.0
        return s

    def tie_horizon(self, j):
        """the first horizon h at which query j's list over [0, h) is full and row h — the first row excluded — scores exactly what
        the list's last entry scores: only the tie rule (the older row wins) and the horizon keep row h out"""
        sc = np.array([self.score(j, r) for r in range(self.n)])
        for h in range(self.K, self.n):
            kth = np.sort(sc[:h])[-self.K]
            if kth > 0.0 and sc[h] == kth:
                return h
        raise AssertionError("query %d has no tie at any horizon" % j)

    def rows(self, before):
        """-> the three tensors for query j under horizon before[j], j = 0 .. len(before) - 1"""
        parts = [self.at(h) for h in before]
        return tuple(torch.stack([p[k][j] for j, p in enumerate(parts)]) for k in range(3))


def retr_int32(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.int64).astype(np.int32))


_SHARED = {}


def _shared_reference(lib, device, n, K, index, ids):
    """the weights rat_bm25_query_prepare maps from the index's tables, and the reference over them — built with the first form that
    asks and reused by the others, whose weights must be the same bits (the three forms hold the same live rows)"""
    from rat_amd import ops
    q_ids, q_idf = ops.bm25_query_prepare(_up(retr_int32(ids), device), index.cols, index.table_ids, index.table_idf, index.table_offsets,
                                          lib=lib)
    key = (str(device), n, K)
    if key not in _SHARED:
        _case, live, _junk, _data, cols = make_rows(n)
        _SHARED[key] = Reference(lib, device, live, cols, q_ids, q_idf, K)
    ref = _SHARED[key]
    assert torch.equal(ref.q_ids, q_ids) and torch.equal(ref.q_idf.view(torch.int64), q_idf.view(torch.int64)), "the forms disagree on the weights"
    return ref


def ranges(splits, capacity):
    """the number of ranges the scan cuts: `splits`, or for splits = 0 the most the library's rule allows at this capacity (every range
    at least 1024 rows of the capacity, at most 256 ranges; fewer when the query tiles alone fill the chip) — below 2048 rows: one"""
    return splits if splits > 0 else max(1, min(256, capacity // 1024))


def horizons(n, splits):
    """0, 1, n - 1, n, n + 7, -3 and the rows around a range boundary: c = ceil(n / splits) is where the second range starts"""
    c = -(-n // splits)
    return [0, 1, n - 1, n, n + 7, -3, c - 1, c, c + 1, min(2 * c, n) - 1]


# ---- 1. the horizon scan == rat_bm25_topk over truncated copies, bit for bit --------------------------------------------------------------
def check_scan_parity(gpu, lib, form, K, n=300, splits=(1, 3, 64), sizes=(1, 5, 9)):
    from rat_amd.online import RetrievalIndex
    device = _device(gpu)
    case, live, junk, data, cols = make_rows(n)
    index = build_form(form, live, junk, lambda rows, **kw: RetrievalIndex(rows, cols, K, device, lib=lib, **kw))
    own = [int(r) for r in self_retrieving_rows(live, cols, 3, 4)]
    ids = _queries(live, data, own)
    ref = _shared_reference(lib, device, n, K, index, ids)
    seen = dict(ragged_tile=False, four_horizons_in_a_tile=False, empty_ranges=False, short_ranges=False, boundary=False,
                ties_at_the_horizon=False, short_lists=False, self_excluded=False)
    for given in splits:
        index.splits = given
        s = ranges(given, index.db_t.shape[1])
        H = horizons(n, s)
        c = -(-n // s)
        seen["empty_ranges"] |= s * c >= n + c
        seen["short_ranges"] |= c < 256
        seen["boundary"] |= s > 1 and {c - 1, c, c + 1} <= set(H)
        for Q in sizes:
            for start in range(0, len(H), Q):
                before = [H[(start + j) % len(H)] for j in range(Q)]
                what = "%s K=%d splits=%d Q=%d before=%s" % (form, K, s, Q, before)
                want = ref.rows(before)
                # the horizons in every accepted form (once per range count): a list, int32 numpy, a tensor on the index's device
                forms = (before, np.asarray(before, dtype=np.int32), _up(np.asarray(before, dtype=np.int64), device))
                for b in forms[:3 if start == 0 else 1]:
                    got = index.retrieve(ids[:Q], before=b)
                    oc.assert_bitwise(tuple(t.cpu() for t in got), want, what)
                assert got[0].dtype == torch.float64 and got[1].dtype == torch.int64 and tuple(got[1].shape) == (Q, K), what
                idx = want[1].numpy()
                clamped = np.clip(before, 0, n)
                assert (idx < clamped[:, None]).all(), what
                seen["ragged_tile"] |= Q % 4 != 0
                seen["four_horizons_in_a_tile"] |= Q >= 4 and len(set(clamped[:4])) == 4
                seen["short_lists"] |= bool(((want[2].numpy() < K) & (clamped > 0)).any())
        # a live row asked about itself with its own position as the horizon: it is its own best match, and it is not in the list
        got = index.retrieve(ids[:4], before=own)
        oc.assert_bitwise(tuple(t.cpu() for t in got), ref.rows(own), "%s K=%d splits=%d own rows" % (form, K, s))
        # equal scores on both sides of the horizon: the first row behind it scores exactly what the list's last entry scores
        tie = [ref.tie_horizon(j) for j in range(4)]
        want = ref.rows(tie)
        assert all(int(want[2][j]) == K and float(want[0][j, K - 1]) == ref.score(j, h) for j, h in enumerate(tie))
        oc.assert_bitwise(tuple(t.cpu() for t in index.retrieve(ids[:4], before=tie)), want, "%s K=%d splits=%d ties" % (form, K, s))
        seen["ties_at_the_horizon"] = True
        plain = index.retrieve(ids[:4])
        seen["self_excluded"] |= bool((plain[1].cpu().numpy() == np.asarray(own)[:, None]).any(axis=1).all())
        # before = n for every query is the plain retrieve
        for Q in sizes:
            oc.assert_bitwise(index.retrieve(ids[:Q], before=[n] * Q), index.retrieve(ids[:Q]), "%s K=%d splits=%d before=n" % (form, K, s))
            oc.assert_bitwise(tuple(t.cpu() for t in index.retrieve(ids[:Q])), ref.rows([n] * Q), "plain retrieve")
    if max(splits) * 2 <= n:                                                   # (the emulated run has no range count that leaves ranges empty)
        del seen["empty_ranges"]
    assert all(seen.values()), seen


def check_scan_poisoned(gpu, lib, form, K, n=300, splits=(1, 3, 64), h=30):
    """the rows at and behind the horizon are overwritten, on the device, with ids that win every query: each query is a combination
    of ids that no row in front of the horizon holds in full, and the rows behind it hold exactly the queries' ids — they are the only
    full matches, so they lead the plain retrieve — while the horizon scan still answers like the reference over the rows in front"""
    import itertools
    from rat_amd import ops
    from rat_amd.online import RetrievalIndex
    device = _device(gpu)
    case, live, junk, data, cols = make_rows(n)
    index = build_form(form, live, junk, lambda rows, **kw: RetrievalIndex(rows, cols, K, device, lib=lib, **kw))
    used = live[:, cols].astype(np.int64)
    in_front = {tuple(r) for r in used[:h]}
    absent = [c for c in itertools.product(*[np.unique(used[:, f]) for f in range(len(cols))]) if c not in in_front]
    assert len(absent) >= N_QUERIES, "every combination of ids stands in front of the horizon"
    ids = np.ascontiguousarray(data[:N_QUERIES, :-1])
    ids[:, cols] = np.asarray(absent[:N_QUERIES])
    q_ids, q_idf = ops.bm25_query_prepare(_up(retr_int32(ids), device), index.cols, index.table_ids, index.table_idf, index.table_offsets,
                                          lib=lib)
    assert float(q_idf.min()) > 0.0
    want = Reference(lib, device, live, cols, q_ids, q_idf, K).rows([h] * N_QUERIES)
    assert int(want[2].min()) > 0                                              # partial matches in front of the horizon: lists to compare
    cap = index.db_t.shape[1]
    head = int(index.count[1]) if form == "window" else 0
    later = np.arange(h, n)
    winners = retr_int32(ids[:, cols])[(later - h) % N_QUERIES]                # row h + j holds query (j mod 9)'s ids
    index.db_t[:, _up((head + later) % cap, device)] = _up(winners.T, device)
    for s in splits:
        index.splits = s
        got = index.retrieve(ids, before=[h] * N_QUERIES)
        oc.assert_bitwise(tuple(t.cpu() for t in got), want, "%s K=%d splits=%d poisoned" % (form, K, s))
        assert int(got[1].max()) < h
        plain = index.retrieve(ids)[1].cpu().numpy()
        assert (plain >= h).all(), "the overwritten rows do not win the plain retrieve: the case checks nothing"


# ---- 2. batch_rows: no row retrieves itself or a younger row; the batch equals a numpy assembly from the reference lists ---------------------
def _setup_scorer(gpu, lib, form, n, graph=False):
    from rat_amd.online import OnlineScorer
    case, live, junk, data, cols = make_rows(n)
    model = mc.build_model(case, gpu=gpu, seed=1)
    mc.load_weights(model, case)
    model.eval()
    cfg = dict(topK=case["topk"], used_col_indices=cols, qry_batch_size=None, label_wise=False, split_type="random")
    scorer = build_form(form, live, junk, lambda rows, **kw: OnlineScorer(model, rows, cfg, graph=graph, lib=lib, **kw))
    return case, model, cfg, scorer, live, data, cols


def numpy_batch(lib, device, live, cols, K, rows, q_idf_of):
    """the batch of the live rows `rows` as the issue defines it, assembled on the host: neighbours from rat_bm25_topk over live[:i]
    with the weights `q_idf_of(ids)` maps, a padding -> row max(i - 1, 0), the target's label token 2, y_true the stored label"""
    ids = np.ascontiguousarray(live[rows, :-1])
    q_ids, q_idf = q_idf_of(ids)
    ref = Reference(lib, device, live, cols, q_ids, q_idf, K)
    _v, nbr, lens = ref.rows(list(rows))
    nbr = nbr.numpy().copy()
    raw = nbr.copy()
    pad = np.maximum(np.asarray(rows) - 1, 0)
    nbr = np.where(nbr < 0, pad[:, None], nbr)
    idx = np.concatenate([ids[:, None, :], live[nbr][:, :, :-1]], axis=1).astype(np.int32)
    label_ids = np.concatenate([np.full((len(rows), 1), 2), live[nbr][:, :, -1]], axis=1).astype(np.int32)
    return raw, lens.numpy(), idx, label_ids, live[rows, -1].astype(np.float32)


def check_batch_rows(gpu, lib, form, n=300):
    from rat_amd import ops
    from rat_amd.data import DeviceBatch
    device = _device(gpu)
    case, model, cfg, scorer, live, data, cols = _setup_scorer(gpu, lib, form, n)
    K = case["topk"]
    index = scorer.index
    rows = self_retrieving_rows(live, cols, K, 8)[[4, 0, 1, 7, 2, 5, 6, 3]]      # rows 0, 1, 2 (paddings) and five later ones, unordered
    prepare = lambda ids: ops.bm25_query_prepare(_up(retr_int32(ids), device), index.cols, index.table_ids, index.table_idf,   # noqa: E731
                                                 index.table_offsets, lib=lib)
    raw, lens, idx_np, label_np, y_np = numpy_batch(lib, device, live, cols, K, rows, prepare)
    assert (raw < rows[:, None]).all() and (lens[rows > 0] > 0).any() and (raw < 0).any(), "the case needs neighbours and paddings"
    variants = [rows, rows.tolist(), torch.from_numpy(rows)] + ([torch.from_numpy(rows).to(device)] if gpu >= 0 else [])
    for r in variants:
        b = scorer.batch_rows(r)
        assert isinstance(b, DeviceBatch) and len(b) == len(rows)
        assert np.array_equal(b.idx.cpu().numpy(), idx_np), form
        assert np.array_equal(b.label_ids.cpu().numpy(), label_np), form
        assert np.array_equal(b.y_true.cpu().numpy(), y_np), form
    assert (y_np == 1).any() and (y_np == 0).any()
    # what the horizon scan itself returned: nobody at or behind the row, padding still -1
    ids_dev, labels_dev, before = ops.pool_gather_rows(scorer.pool_ids, scorer.pool_labels, _up(rows.astype(np.int64), device), lib=lib,
                                                       **index._pool_form())
    assert np.array_equal(before.cpu().numpy(), rows) and np.array_equal(ids_dev.cpu().numpy(), retr_int32(live[rows, :-1]))
    got = index.retrieve(ids_dev, before=before)[1].cpu().numpy()
    assert np.array_equal(got, raw) and (got < rows[:, None]).all()
    # the leak this is about: the plain batch of a live row's ids holds the row itself among its neighbours, label attached
    leak = index.retrieve(live[rows, :-1])[1].cpu().numpy()
    assert (leak == rows[:, None]).any(axis=1).all(), "the plain retrieve does not return the row itself: the inputs exercise nothing"
    plain = scorer.batch(live[rows, :-1])
    own = retr_int32(live[rows, :-1])
    assert all((plain.idx[j, 1:].cpu().numpy() == own[j]).all(axis=1).any() for j in range(len(rows)))
    assert float(plain.y_true.abs().max()) == 0.0
    return scorer, model, rows, (idx_np, label_np, y_np)


# ---- 3. rat_pool_gather_rows == numpy over the live rows in age order -----------------------------------------------------------------------
def check_gather(device, lib):
    from rat_amd import ops
    rs = np.random.RandomState(41)
    seen = dict(wrapped=False, out_of_range=False, one_row=False)
    for pool in fc._pools(device, rs, live=(1, 7, 33, 50)):
        n = pool.n
        inside = rs.permutation(n)[:max(1, (2 * n) // 3)]
        outside = np.array([-1, n, n + 5, pool.capacity, -2 ** 40, 2 ** 40, -2 ** 63, 2 ** 63 - 1])
        for indices in (inside, np.concatenate([outside[:3], inside, outside[3:], inside[:2]]), np.arange(n), outside):
            indices = indices.astype(np.int64)
            ids, labels, before = ops.pool_gather_rows(pool.pool_ids, pool.pool_labels, _up(indices, device), lib=lib, **pool.form_args())
            ok = (indices >= 0) & (indices < n)
            want_ids = np.zeros((len(indices), fc.L), dtype=np.int32)
            want_labels = np.zeros(len(indices), dtype=np.float32)
            want_ids[ok], want_labels[ok] = pool.ids[indices[ok]], pool.labels[indices[ok]]
            tag = "%s n=%d head=%d" % (pool.form, n, pool.head)
            assert ids.dtype == torch.int32 and labels.dtype == torch.float32 and before.dtype == torch.int64, tag
            assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(labels.cpu().numpy(), want_labels), tag
            assert np.array_equal(before.cpu().numpy(), np.clip(indices, 0, n)), tag
            w = pool.capacity - pool.head
            seen["wrapped"] |= pool.head + n > pool.capacity and (indices[ok] < w).any() and (indices[ok] >= w).any()
            seen["out_of_range"] |= bool((~ok).any())
            seen["one_row"] |= n == 1
    assert all(seen.values()), seen


def check_corrupt(lib, capacity=fc.CAPACITY, guard=4096):
    """both entry points through the C ABI with every buffer between guard regions and headers outside their domains, indices and
    horizons far outside: the calls return normally, the guards are intact, the inputs are only read and what comes out is in range"""
    FILL = -99
    rs = np.random.RandomState(43)
    L, F, Q, K = fc.L, 3, 5, 3

    def guarded(numel, dtype, fill):
        whole = torch.full((numel + 2 * guard,), FILL, dtype=dtype)
        whole[guard:guard + numel] = fill
        return whole, whole[guard:guard + numel]

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def intact(bufs, read_only, what):
        for name, (whole, _) in bufs.items():
            assert (whole[:guard] == FILL).all() and (whole[-guard:] == FILL).all(), (name, what)
        assert all(torch.equal(bufs[b][0], v) for b, v in read_only.items()), what
    headers = [(capacity + 77, 5), (10 ** 12, 0), (-5, 0), (30, capacity), (30, capacity + 10 ** 9), (30, -3), (capacity + 1, capacity + 1),
               (-2 ** 62, 2 ** 62), (capacity, capacity - 1), (0, 0)]
    hostile = [-1, capacity, 10 ** 12, -10 ** 12, 2 ** 62, -2 ** 63, 2 ** 63 - 1, 0, capacity - 1, 3, 2 ** 31, -2 ** 31]
    for form in (2, 1):
        for n, head in headers:
            bufs = dict(pool_ids=guarded(capacity * L, torch.int32, 0), pool_labels=guarded(capacity, torch.float32, 0.5),
                        hdr=guarded(2, torch.int64, 0), idx=guarded(len(hostile), torch.int64, 0),
                        out_ids=guarded(len(hostile) * L, torch.int32, 77), out_labels=guarded(len(hostile), torch.float32, 7.0),
                        out_before=guarded(len(hostile), torch.int64, 77))
            bufs["pool_ids"][1][:] = torch.from_numpy(rs.randint(1, 9, size=capacity * L).astype(np.int32))
            bufs["hdr"][1][:] = torch.tensor([n, head])
            bufs["idx"][1][:] = torch.tensor(hostile)
            read_only = {k: bufs[k][0].clone() for k in ("pool_ids", "pool_labels", "hdr", "idx")}
            lib.call("rat_pool_gather_rows", p(bufs["pool_ids"][1]), p(bufs["pool_labels"][1]), form, p(bufs["hdr"][1]), 0, capacity,
                     p(bufs["idx"][1]), p(bufs["out_ids"][1]), p(bufs["out_labels"][1]), p(bufs["out_before"][1]), len(hostile), L, None)
            intact(bufs, read_only, ("gather", form, n, head))
            nc = min(max(n, 0), capacity)
            assert np.array_equal(bufs["out_before"][1].numpy(), np.clip(np.asarray(hostile, dtype=object), 0, nc).astype(np.int64))
            dead = np.array([not 0 <= i < nc for i in hostile])
            assert (bufs["out_ids"][1].numpy().reshape(-1, L)[dead] == 0).all() and (bufs["out_labels"][1].numpy()[dead] == 0).all()
            # the scan under the same header, the horizons hostile as well
            for splits in (1, 3):
                ws_words = Q * splits * K * 2
                bufs = dict(db_t=guarded(F * capacity, torch.int32, 0), hdr=guarded(2, torch.int64, 0), q_ids=guarded(Q * F, torch.int32, 1),
                            q_idf=guarded(Q * F, torch.float64, 1.5), before=guarded(Q, torch.int64, 0), out_v=guarded(Q * K, torch.float64, 7.0),
                            out_i=guarded(Q * K, torch.int64, 77), out_l=guarded(Q, torch.int64, 77), ws=guarded(ws_words, torch.int64, 5))
                bufs["db_t"][1][:] = torch.from_numpy(rs.randint(0, 3, size=F * capacity).astype(np.int32))
                bufs["hdr"][1][:] = torch.tensor([n, head])
                bufs["before"][1][:] = torch.tensor(hostile[3 * (splits - 1):3 * (splits - 1) + Q])
                read_only = {k: bufs[k][0].clone() for k in ("db_t", "hdr", "q_ids", "q_idf", "before")}
                lib.call("rat_bm25_topk_split_before", p(bufs["db_t"][1]), form, p(bufs["hdr"][1]), 0, capacity, p(bufs["q_ids"][1]),
                         p(bufs["q_idf"][1]), p(bufs["before"][1]), p(bufs["out_v"][1]), p(bufs["out_i"][1]), p(bufs["out_l"][1]),
                         p(bufs["ws"][1]), ws_words * 8, Q, F, K, splits, None)
                intact(bufs, read_only, ("scan", form, n, head, splits))
                got_i, got_l = bufs["out_i"][1].numpy().reshape(Q, K), bufs["out_l"][1].numpy()
                horizon = np.clip(np.asarray(bufs["before"][1].tolist(), dtype=object), 0, nc).astype(np.int64)
                assert ((got_i >= -1) & (got_i < np.maximum(horizon, 0)[:, None])).all() and ((got_l >= 0) & (got_l <= K)).all()
                assert (got_l[horizon == 0] == 0).all()


# ---- 4. score_rows and evaluate_rows ---------------------------------------------------------------------------------------------------------
def check_scores(gpu, lib, form, n=300):
    from rat_amd import metrics
    from rat_amd.data import DeviceBatch
    device = _device(gpu)
    scorer, model, rows, (idx_np, label_np, y_np) = check_batch_rows(gpu, lib, form, n=n)
    with torch.no_grad():
        want = model.forward(DeviceBatch(_up(idx_np, device), _up(label_np, device), _up(y_np, device)))["y_pred"].reshape(-1).clone()
    y = scorer.score_rows(rows)
    assert y.dtype == torch.float32 and tuple(y.shape) == (len(rows),)
    worst = float((y - want).abs().max())
    print("score_rows vs the eval forward over the numpy batch, %s: worst |dy| = %.3g, bit-equal: %s" % (form, worst, torch.equal(y, want)))
    if gpu >= 0:
        import margins
        margins.record("check_scores", "%s/%s" % (CASE, form), "y_pred, absolute", worst, EVAL_GATE, arith=model.arith)
    assert worst <= EVAL_GATE, (form, worst)
    leaked = scorer.score(scorer.pool_ids.new_tensor(idx_np[:, 0]))           # the same rows through score(): their labels in hand
    assert not torch.equal(leaked, y), "scoring a row against itself changes nothing: the inputs exercise nothing"
    got = scorer.evaluate_rows(rows)
    ref = metrics.evaluate_metrics(y_np.astype(np.float64), y.cpu().numpy().astype(np.float64), ["logloss", "AUC"])
    assert set(got) == {"logloss", "AUC"} and got == ref, (got, ref)
    assert 0.0 < got["logloss"] < 10.0 and 0.0 <= got["AUC"] <= 1.0


# ---- 5. graphs (GPU only) ----------------------------------------------------------------------------------------------------------------------
def check_rows_graph(gpu, lib, form, n=300, B=8):
    """a score_rows graph captured BEFORE any mutation answers after append / evict / delete / relabel_where / a training step like a
    fresh graph=False scorer over the live rows, bit for bit; the number of captured graphs does not change and a second index set
    of the same size goes through the same graph"""
    from rat_amd.data import DeviceBatch
    from rat_amd.online import OnlineScorer, _RowsGraph
    assert gpu >= 0
    device = _device(gpu)
    case, model, cfg, scorer, live, data, cols = _setup_scorer(gpu, lib, form, n, graph=True)
    cap = scorer.index.capacity
    cur = [live.copy()]
    sets = [np.array([n // 2 + 1, 5, 1, n - 1, 2, 150, 37, 3]), np.array([0, n - 2, 99, 100, 101, 12, 201, 64])]
    assert all(len(s) == B for s in sets)

    def graphs():
        return [e[1] for e in scorer._rows_graphs.values()]

    def check(tag, which=(0, 1)):
        fresh = OnlineScorer(model, cur[0], cfg, graph=False, lib=lib)
        out = []
        for s in [sets[w] for w in which]:
            s = np.minimum(s, len(cur[0]) - 1 - np.arange(B))                  # inside the live rows, still distinct
            idx = _up(s.astype(np.int64), device)
            y, want = scorer.score_rows(idx), fresh.score_rows(idx)
            assert tuple(y.shape) == (B,) and torch.equal(y, want), (tag, float((y - want).abs().max()))
            out.append(y)
        return out
    for k in range(scorer.graph_warmup):                                      # eager, counted per size: nothing captured yet
        check("warm-up %d" % k, which=(k % 2,))
        assert not any(isinstance(g, _RowsGraph) for g in graphs())
    assert len(scorer._rows_graphs) == 1
    y_prev = check("capture")                                                 # the first set is captured, the second one replays it
    captured = graphs()
    assert [isinstance(g, _RowsGraph) for g in captured] == [True], "score_rows was not captured"
    assert len(scorer._graphs) == 0 and len(scorer._bucket_graphs) == 0         # score()'s and score_requests()'s own: untouched
    n_ids = live.shape[1] - 1
    steps = ["relabel"] + (["append"] if form != "immutable" else []) + (["evict", "delete"] if form == "window" else []) + ["train"]
    for step in steps:
        if step == "relabel":                                                 # every row that shares its first retrieval column with row 5
            keys = cur[0][5:6, [cols[0]]].astype(np.int64)
            hit = cur[0][:, cols[0]] == cur[0][5, cols[0]]
            new = 1.0 - float(np.round(cur[0][hit, -1].mean()))
            count = scorer.relabel_where([cols[0]], keys, new)
            cur[0] = cur[0].copy()
            cur[0][hit, -1] = new
            assert int(count) == int(hit.sum()) > 1
        elif step == "append":
            rows = data[:6].copy()
            scorer.append(rows)
            cur[0] = np.concatenate([cur[0], rows])
            if form == "window":
                cur[0] = cur[0][-cap:]
        elif step == "evict":
            scorer.evict(4)
            cur[0] = cur[0][4:]
        elif step == "delete":
            gone = np.array([1, 30, 100])
            scorer.delete(gone)
            cur[0] = np.delete(cur[0], gone, axis=0)
        else:
            model.train()
            model.train_step(scorer.batch_rows(_up(sets[0].astype(np.int64), device)))      # the rows' real labels: a fine-tuning step
            model.eval()
        assert len(scorer.index) == len(cur[0])
        y_new = check("after %s" % step)
        assert [a is b for a, b in zip(graphs(), captured)] == [True], "%s invalidated the captured graph" % step
        assert len(scorer._rows_graphs) == 1 and len(scorer._graphs) == 0 and len(scorer._bucket_graphs) == 0
        assert not all(torch.equal(a, b) for a, b in zip(y_new, y_prev)), "%s changed no prediction" % step
        y_prev = y_new


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def check_rows_refusals(gpu, lib):
    import pytest
    from rat_amd import ops
    device = _device(gpu)
    case, model, cfg, scorer, live, data, cols = _setup_scorer(gpu, lib, "immutable", 60)
    n = len(live)
    ids = np.ascontiguousarray(data[:6, :-1])
    launches = []
    real = (ops.bm25_query_prepare, ops.pool_gather_rows)
    ops.bm25_query_prepare = lambda *a, **k: launches.append("prepare") or real[0](*a, **k)
    ops.pool_gather_rows = lambda *a, **k: launches.append("gather") or real[1](*a, **k)
    try:
        with pytest.raises(ValueError, match="request_offsets"):
            scorer.index.retrieve(ids, [0, 2, 6], before=[1] * 6)
        with pytest.raises(ValueError, match="request_offsets"):
            scorer.index.retrieve(ids, request_offsets=np.array([0, 6]), before=np.arange(6))
        bad = [([1] * 5, "horizons"), ([1] * 7, "horizons"), (np.ones(6), "integers"), (torch.ones(6), "integers"), (np.ones((6, 1), dtype=np.int64), "horizons"),
               (3, "horizons"), (np.array([True] * 6), "integers")]
        if gpu >= 0:
            bad += [(torch.ones(6, device=device), "integers"), (torch.ones(5, dtype=torch.int64, device=device), "horizons")]
        for before, word in bad:
            with pytest.raises(ValueError, match=word):
                scorer.index.retrieve(ids, before=before)
        for call in (scorer.score_rows, scorer.batch_rows, scorer.evaluate_rows):
            for idx, word in (([n], "outside"), ([-1], "outside"), ([0, n + 5], "outside"), ([0.0, 1.0], "integer"), ([3, 5, 3], "duplicate"),
                              (np.zeros((2, 2), dtype=np.int64), "1-D"), ([], "empty"), (torch.tensor([2, -17]), "outside")):
                with pytest.raises(ValueError, match=word):
                    call(idx)
        assert launches == [], "a refused call launched something"
        model.train()
        for call in (scorer.score_rows, scorer.evaluate_rows):
            with pytest.raises(RuntimeError, match="eval mode"):
                call([0, 1])
        assert launches == []
        assert len(scorer.batch_rows([0, 1])) == 2                           # a batch for train_step needs no eval mode
        model.eval()
        launches.clear()
        y = scorer.score_rows([n - 1, 0])                                     # and a good one goes through
        assert tuple(y.shape) == (2,) and launches == ["gather", "prepare"]
        v, i, ln = scorer.index.retrieve(ids, before=[0, 1, -3, n, n + 7, 2])
        assert ln.cpu().tolist()[0] == 0 and ln.cpu().tolist()[2] == 0 and (i[0] == -1).all() and (v[2] == 0).all()
    finally:
        ops.bm25_query_prepare, ops.pool_gather_rows = real
