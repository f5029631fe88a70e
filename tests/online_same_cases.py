"""Checks of neighbours restricted to rows equal on given columns (``rat_bm25_exact_count``, ``rat_bm25_exact_plan``,
``rat_bm25_topk_split_exact``; ``RetrievalIndex.retrieve(ids, same=...)``, ``OnlineScorer.batch / score / batch_rows / score_rows /
evaluate_rows(..., same=...)``) shared by tests/test_online_same.py (CPU, host-emulation build) and tests/test_gpu_online_same.py
(MI355X).

The reference is the offline path of this repository, ``retrieval.BM25_topk_retrieval_v4(live[:, U], ids[:, U],
exact_match_col_indices=E, qry_batch_size=None)`` — the host numbers the groups, ``rat_bm25_topk_grouped`` scores — compared bit for
bit, computed once per (K, columns, request) and shared by the three pool forms; the same results are held to
``oracle.retrieval_oracle.topk_exact`` through its tie-tolerant helper.  Horizons have no offline counterpart: their reference is a
numpy restatement of the three rules (``brute``), itself compared with the offline path where that exists (no horizon).

The pool: 300 rows, four used columns with 40 / 3 / 5 / 4 distinct ids from ``default_rng(5)``.  The groups of the first used column
have 1 .. 12 rows, those of (first, third) 1 .. 6: K = 3 and K = 12 fall on both sides of the listing rule, and with 3 to 5 ids per
scored column equal scores are the rule."""
import ctypes

import numpy as np
import torch

import online_cases as oc
import online_rows_cases as rc
from oracle import retrieval_oracle as ro

FORMS = rc.FORMS
L = 6                                # id columns of an encoded row
COLS = [4, 0, 5, 2]                  # the used columns U, in the index's order: 40 / 3 / 5 / 4 distinct ids
VOCAB = (40, 3, 5, 4)
SAMES = ([4], [4, 5])                # one column (E = [0]); two columns that are not neighbours inside U (E = [0, 2])
ABSENT = 99                          # an id no pool column holds
EVAL_GATE = rc.EVAL_GATE


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _device(gpu):
    return "cpu" if gpu < 0 else "cuda:%d" % gpu


def positions(same):
    return [COLS.index(c) for c in same]


def make_pool(n=300, seed=5):
    """-> (live [n, L + 1] in age order, junk [64, L + 1]: rows that pass through a window and leave), label last"""
    rng = np.random.default_rng(seed)
    used = np.stack([rng.integers(0, v, size=n) for v in VOCAB], axis=1)                     # the live rows first: they are the pool
    used = np.concatenate([used, np.stack([rng.integers(0, v, size=64) for v in VOCAB], axis=1)])
    rows = rng.integers(0, 7, size=(n + 64, L + 1))
    rows[:, COLS] = used
    rows[:, -1] = rng.integers(0, 2, size=n + 64)
    rows = rows.astype(np.float64)
    if n == 300:
        sizes0 = np.unique(rows[:n, COLS[0]], return_counts=True)[1]
        sizes02 = np.unique(rows[:n][:, [COLS[0], COLS[2]]], axis=0, return_counts=True)[1]
        assert (sizes0.min(), sizes0.max(), sizes02.min(), sizes02.max()) == (1, 12, 1, 6), "the pool is not the one the cases are built on"
    return rows[:n], rows[n:]


def used_of(rows):
    return np.ascontiguousarray(np.asarray(rows)[:, COLS].astype(np.int64))


def counts_of(live_u, q_u, E, before=None):
    """c[q]: live rows (below the clamped horizon) equal to query q on the columns E"""
    n = len(live_u)
    h = np.full(len(q_u), n) if before is None else np.clip(np.asarray(before, dtype=object), 0, n).astype(np.int64)
    return np.array([int((live_u[:h[j], E] == q_u[j, E]).all(axis=1).sum()) for j in range(len(q_u))])


# ---- the numpy restatement of the contract (horizons included) -----------------------------------------------------------------------
def brute(live_u, q_u, E, K, before=None):
    """(values, indices, lens) of one call: candidates and counts, the listing rule, the scoring rule with the weights of the WHOLE live
    pool and the dtype rule taken from the first candidate-bearing query"""
    from rat_amd import retrieval
    n, Q = len(live_u), len(q_u)
    R = [f for f in range(live_u.shape[1]) if f not in E]
    h = np.full(Q, n) if before is None else np.clip(np.asarray(before, dtype=object), 0, n).astype(np.int64)
    cand = [np.flatnonzero((live_u[:h[j], E] == q_u[j, E]).all(axis=1)) for j in range(Q)]
    c = np.array([len(m) for m in cand])
    values, indices, lens = np.zeros((Q, K)), np.full((Q, K), -1, dtype=np.int64), np.zeros(Q, dtype=np.int64)
    has = np.flatnonzero(c > 0)
    if len(has) == 0:
        return values, indices, lens
    if c.max() <= K:
        for j in has:
            indices[j, :c[j]], values[j, :c[j]], lens[j] = cand[j], 1.0, c[j]
        return values, indices, lens
    w = retrieval.map_data_to_idf(q_u[has][:, R], retrieval.idf_tables(live_u[:, R]))
    for row, j in enumerate(has):
        m = cand[j]
        s = np.zeros(len(m))
        for k, f in enumerate(R):
            s = s + np.where(live_u[m, f] == q_u[j, f], w[row, k], 0.0)
        s = s + 1.0
        order = np.lexsort((m, -s))[:K]
        indices[j, :len(order)], values[j, :len(order)], lens[j] = m[order], s[order], len(order)
    return values, indices, lens


# ---- the requests ----------------------------------------------------------------------------------------------------------------
def make_requests(live, E, K, sizes=(1, 5, 9)):
    """-> [(name, ids [Q, L])]: per size a request of small groups only, one with a large group, one whose first row has no candidate,
    one whose first candidate-bearing row misses in a scored column, and one without any candidate"""
    rng = np.random.default_rng(11 + K + 100 * len(E))
    live_u = used_of(live)
    R = [f for f in range(len(COLS)) if f not in E]
    g = counts_of(live_u, live_u, E)
    small, big = np.flatnonzero(g <= max(min(K, 3), g.min())), np.flatnonzero(g == g.max())
    out = []

    def rows_of(idx, fresh=True):
        ids = live[idx, :-1].copy()
        if fresh:                                       # half of them ask with other ids on the scored columns: partial matches
            for j in range(0, len(idx), 2):
                for f in R:
                    ids[j, COLS[f]] = rng.integers(0, VOCAB[f])
        return ids

    def absent(k):
        ids = rows_of(rng.choice(len(live), size=k), fresh=False)
        ids[:, COLS[E[0]]] = ABSENT
        return ids
    for Q in sizes:
        out.append(("small groups Q=%d" % Q, rows_of(rng.choice(small, size=Q))))
        mixed = rng.choice(small, size=Q)
        mixed[Q // 2] = big[0]
        out.append(("a large group Q=%d" % Q, rows_of(mixed)))
        out.append(("no candidate Q=%d" % Q, absent(Q)))
        if Q > 1:
            late = rows_of(mixed)
            late[0] = absent(1)[0]
            out.append(("first row without a candidate Q=%d" % Q, late))
            miss = rows_of(mixed, fresh=False)
            miss[0] = live[big[-1], :-1]
            miss[0, COLS[R[0]]] = ABSENT                # the first candidate-bearing row misses in a scored column
            miss[1] = absent(1)[0]
            miss[1, COLS[R[0]]] = live[0, COLS[R[0]]]
            if Q > 5:                                   # ... and is not the request's first row either
                miss[[0, 1]] = miss[[1, 0]]
            out.append(("truncation Q=%d" % Q, miss))
    return [(name, np.ascontiguousarray(ids)) for name, ids in out]


def regimes(live, E, K, requests):
    """which regimes the requests enter, from counts computed here in numpy"""
    from rat_amd import retrieval
    live_u = used_of(live)
    R = [f for f in range(len(COLS)) if f not in E]
    tables = retrieval.idf_tables(live_u[:, R])
    seen = dict(listing=False, scoring=False, first_row_without_candidate=False, truncation=False, no_candidate=False)
    for _name, ids in requests:
        q_u = used_of(ids)
        c = counts_of(live_u, q_u, E)
        has = np.flatnonzero(c > 0)
        if len(has) == 0:
            seen["no_candidate"] = True
            continue
        scoring = c.max() > K
        seen["scoring"] |= scoring
        seen["listing"] |= (not scoring) and K <= 3
        seen["first_row_without_candidate"] |= c[0] == 0
        if scoring:
            first = q_u[has[0]]
            for k, f in enumerate(R):
                vals, idf = tables[k]
                if first[f] not in vals:                # ... and the truncated weights differ from the plain ones for a later row
                    hit = np.isin(q_u[has][:, f], vals)
                    w = idf[np.searchsorted(vals, q_u[has][hit, f])]
                    seen["truncation"] |= bool((w != np.trunc(w)).any())
    return seen


_REFERENCE = {}


def reference(lib, device, n, live, E, K, name, ids):
    """the offline path's answer, computed by the first pool form that asks and shared with the others"""
    from rat_amd import retrieval
    key = (str(device), n, tuple(E), K, name)
    if key not in _REFERENCE:
        r = retrieval.BM25_topk_retrieval_v4(used_of(live), used_of(ids), exact_match_col_indices=list(E), qry_batch_size=None, topK=K,
                                             device=device, lib=lib)
        _REFERENCE[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (r.values, r.indices, r.lens))
    return _REFERENCE[key]


def _index(form, live, junk, K, device, lib):
    from rat_amd.online import RetrievalIndex
    return rc.build_form(form, live, junk, lambda rows, **kw: RetrievalIndex(rows, COLS, K, device, lib=lib, **kw))


# ---- 1. retrieve(ids, same=) == the offline path, bit for bit ------------------------------------------------------------------------
def check_offline_parity(gpu, lib, form, K, same, n=300, splits=(1, 3, 64), sizes=(1, 5, 9)):
    device = _device(gpu)
    live, junk = make_pool(n)
    E = positions(same)
    index = _index(form, live, junk, K, device, lib)
    requests = make_requests(live, E, K, sizes)
    seen = regimes(live, E, K, requests)
    if n == 300:
        if K > 3:                                       # no group of this pool exceeds 12 rows: every request lists
            assert not seen["scoring"] and seen["no_candidate"] and seen["first_row_without_candidate"], seen
        else:
            assert all(seen.values()), seen
    live_u = used_of(live)
    for s in splits:
        index.splits = s
        for name, ids in requests:
            what = "%s K=%d same=%s ranges=%d %s" % (form, K, same, s, name)
            want = reference(lib, device, n, live, E, K, name, ids)
            got = index.retrieve(ids, same=same)
            assert got[0].dtype == torch.float64 and got[1].dtype == torch.int64 and tuple(got[1].shape) == (len(ids), K), what
            oc.assert_bitwise(tuple(t.cpu() for t in got), want, what)          # every query of every request
            if s == splits[0]:
                ov, oi, ol, score = ro.topk_exact(live_u, used_of(ids), E, K)
                ro.assert_topk_equivalent(score, tuple(t.cpu().numpy() for t in got), (ov, oi, ol))
                mine = brute(live_u, used_of(ids), E, K)                       # the restatement the horizon check relies on
                oc.assert_bitwise(tuple(torch.from_numpy(a) for a in mine), want, what + " (numpy restatement)")
    # the forms of `same` a caller may pass, and ids on the device
    name, ids = [r for r in requests if r[0].startswith("a large group")][-1]
    want = reference(lib, device, n, live, E, K, name, ids)
    for given in (tuple(same), np.asarray(same), np.asarray(same, dtype=np.int32), torch.tensor(same)):
        oc.assert_bitwise(tuple(t.cpu() for t in index.retrieve(_up(ids.astype(np.int32), device), same=given)), want, "same as %r" % (given,))
    # the plain retrieve is something else: the restriction is per call, the object serves both
    plain = index.retrieve(ids)
    assert not torch.equal(plain[1].cpu(), want[1]), "the restriction changes nothing: the inputs exercise nothing"


# ---- 2. horizons --------------------------------------------------------------------------------------------------------------------
def check_horizons(gpu, lib, form, K, same, n=300, splits=(1, 3), Q=5):
    device = _device(gpu)
    live, junk = make_pool(n)
    E = positions(same)
    index = _index(form, live, junk, K, device, lib)
    live_u = used_of(live)
    requests = [r for r in make_requests(live, E, K, (Q,)) if "no candidate" not in r[0]]
    seen = dict(listing_below_the_horizon=False, scoring=False, emptied=False)
    for s in splits:
        index.splits = s
        H = rc.horizons(n, rc.ranges(s, index.db_t.shape[1]))
        for name, ids in requests:
            q_u = used_of(ids)
            for start in range(0, len(H), Q):
                before = [H[(start + j) % len(H)] for j in range(Q)]
                what = "%s K=%d same=%s ranges=%d %s before=%s" % (form, K, same, s, name, before)
                want = brute(live_u, q_u, E, K, before)
                for b in ((before, _up(np.asarray(before, dtype=np.int64), device)) if start == 0 else (before,)):
                    got = index.retrieve(ids, before=b, same=same)
                    oc.assert_bitwise(tuple(t.cpu() for t in got), tuple(torch.from_numpy(a) for a in want), what)
                clamped = np.clip(before, 0, n)
                assert (want[1] < clamped[:, None]).all(), what
                c_all, c_below = counts_of(live_u, q_u, E), counts_of(live_u, q_u, E, before)
                seen["listing_below_the_horizon"] |= c_all.max() > K >= c_below.max() > 0
                seen["scoring"] |= c_below.max() > K
                seen["emptied"] |= bool(((c_all > 0) & (c_below == 0)).any())
            # every query's horizon just behind its K-th candidate: groups larger than K in the pool, none below the horizons
            c_all = counts_of(live_u, q_u, E)
            before = [int(np.flatnonzero((live_u[:, E] == q_u[j, E]).all(axis=1))[K - 1]) + 1 if c_all[j] >= K else n for j in range(Q)]
            want = brute(live_u, q_u, E, K, before)
            oc.assert_bitwise(tuple(t.cpu() for t in index.retrieve(ids, before=before, same=same)), tuple(torch.from_numpy(a) for a in want),
                              "%s horizons behind the K-th candidate" % name)
            seen["listing_below_the_horizon"] |= c_all.max() > K >= counts_of(live_u, q_u, E, before).max() > 0
            # before = n for every query is the call without before
            oc.assert_bitwise(index.retrieve(ids, before=[n] * Q, same=same), index.retrieve(ids, same=same), "before = n")
    if K <= 3:
        assert all(seen.values()), seen
    else:
        assert seen["emptied"], seen


# ---- 3. the objects -----------------------------------------------------------------------------------------------------------------
def _numpy_batch(live, ids, nbr, pad, y_true):
    nbr = np.where(nbr < 0, np.asarray(pad).reshape(-1, 1), nbr)
    idx = np.concatenate([ids[:, None, :], live[nbr][:, :, :-1]], axis=1).astype(np.int32)
    label_ids = np.concatenate([np.full((len(ids), 1), 2), live[nbr][:, :, -1]], axis=1).astype(np.int32)
    return idx, label_ids, np.asarray(y_true, dtype=np.float32)


def check_objects(gpu, lib, form, n=300):
    """batch / batch_rows == a numpy assembly from the reference lists; eager score / score_rows within the eval forward's margin of
    the forward over that batch; evaluate_rows returns both metrics.  The model's case has three retrieval columns, 4 / 2 / 6 ids:
    the groups of the first hold dozens of rows (the scoring rule), those of (first, third) a handful."""
    from rat_amd import metrics, retrieval
    from rat_amd.data import DeviceBatch
    device = _device(gpu)
    case, model, cfg, scorer, live, data, cols = rc._setup_scorer(gpu, lib, form, n)
    K = case["topk"]
    live_u = live[:, cols].astype(np.int64)
    rows = rc.self_retrieving_rows(live, cols, K, 8)[[4, 0, 1, 7, 2, 5, 6, 3]]
    ids = np.ascontiguousarray(np.concatenate([live[rows[:5], :-1], data[:4, :-1]]))
    for same in ([cols[0]], [cols[0], cols[2]]):
        E = [cols.index(c) for c in same]
        r = retrieval.BM25_topk_retrieval_v4(live_u, ids[:, cols].astype(np.int64), exact_match_col_indices=E, qry_batch_size=None,
                                             topK=K, device=device, lib=lib)
        assert (r.indices < 0).any() and (r.lens > 0).any(), "the case needs neighbours and paddings"
        idx_np, label_np, y_np = _numpy_batch(live, ids, r.indices, [n - 1] * len(ids), np.zeros(len(ids)))     # -1: the pool's newest row
        b = scorer.batch(ids, same=same)
        assert isinstance(b, DeviceBatch) and np.array_equal(b.idx.cpu().numpy(), idx_np), (form, same)
        assert np.array_equal(b.label_ids.cpu().numpy(), label_np) and float(b.y_true.abs().max()) == 0.0, (form, same)
        assert not np.array_equal(scorer.batch(ids).idx.cpu().numpy(), idx_np), "the restriction changes nothing"
        with torch.no_grad():
            want = model.forward(DeviceBatch(_up(idx_np, device), _up(label_np, device), _up(y_np, device)))["y_pred"].reshape(-1).clone()
        y = scorer.score(ids, same=same)
        worst = float((y - want).abs().max())
        print("score(same=%s) vs the eval forward over the numpy batch, %s: worst |dy| = %.3g" % (same, form, worst))
        assert y.dtype == torch.float32 and tuple(y.shape) == (len(ids),) and worst <= EVAL_GATE, (form, same, worst)
        # the pool looks at itself: row i against the OLDER rows equal to it on `same`; a padding is row max(i - 1, 0)
        own = np.ascontiguousarray(live[rows, :-1])
        v, nbr, lens = brute(live_u, own[:, cols].astype(np.int64), E, K, before=rows)
        assert (nbr < rows[:, None]).all() and (lens > 0).any() and (nbr < 0).any()
        idx_np, label_np, y_np = _numpy_batch(live, own, nbr, np.maximum(rows - 1, 0), live[rows, -1])
        b = scorer.batch_rows(rows, same=same)
        assert np.array_equal(b.idx.cpu().numpy(), idx_np) and np.array_equal(b.label_ids.cpu().numpy(), label_np), (form, same)
        assert np.array_equal(b.y_true.cpu().numpy(), y_np), (form, same)
        with torch.no_grad():
            want = model.forward(DeviceBatch(_up(idx_np, device), _up(label_np, device), _up(y_np, device)))["y_pred"].reshape(-1).clone()
        y = scorer.score_rows(rows, same=same)
        worst = float((y - want).abs().max())
        print("score_rows(same=%s) vs the eval forward over the numpy batch, %s: worst |dy| = %.3g" % (same, form, worst))
        assert tuple(y.shape) == (len(rows),) and worst <= EVAL_GATE, (form, same, worst)
        got = scorer.evaluate_rows(rows, same=same)
        ref = metrics.evaluate_metrics(y_np.astype(np.float64), y.cpu().numpy().astype(np.float64), ["logloss", "AUC"])
        assert set(got) == {"logloss", "AUC"} and got == ref, (got, ref)
    assert not scorer._graphs and not scorer._bucket_graphs and not scorer._rows_graphs
    assert not scorer._same_graphs and not scorer._same_rows_graphs             # graph=False: nothing is counted, nothing captured


# ---- 4. graphs (GPU only) ------------------------------------------------------------------------------------------------------------
def check_graphs(gpu, lib, form, n=300, B=8):
    """a score(ids, same=) graph and a score_rows(indices, same=) graph captured BEFORE any mutation answer after relabel_where /
    append / evict / delete / a training step like a fresh graph=False scorer over the live rows, bit for bit; the dictionaries of
    the same=None paths are never touched"""
    from rat_amd.online import OnlineScorer, _RequestGraph, _RowsGraph
    assert gpu >= 0
    device = _device(gpu)
    case, model, cfg, scorer, live, data, cols = rc._setup_scorer(gpu, lib, form, n, graph=True)
    same = [cols[0]]
    cap = scorer.index.capacity
    cur = [live.copy()]
    ids = _up(np.concatenate([live[[5, 150, 37, n - 1], :-1], data[:B - 4, :-1]]).astype(np.int32), device)
    sets = [np.array([n // 2 + 1, 5, 1, n - 1, 2, 150, 37, 3]), np.array([0, n - 2, 99, 100, 101, 12, 201, 64])]

    def graphs():
        return [e[1] for e in scorer._same_graphs.values()] + [e[1] for e in scorer._same_rows_graphs.values()]

    def untouched():
        return len(scorer._graphs) == 0 and len(scorer._bucket_graphs) == 0 and len(scorer._rows_graphs) == 0

    def check(tag, which=(0, 1)):
        fresh = OnlineScorer(model, cur[0], cfg, graph=False, lib=lib)
        y, want = scorer.score(ids, same=same), fresh.score(ids, same=same)
        assert tuple(y.shape) == (B,) and torch.equal(y, want), (tag, "score", float((y - want).abs().max()))
        out = [y]
        for s in [sets[w] for w in which]:
            s = np.minimum(s, len(cur[0]) - 1 - np.arange(B))                  # inside the live rows, still distinct
            idx = _up(s.astype(np.int64), device)
            y, want = scorer.score_rows(idx, same=same), fresh.score_rows(idx, same=same)
            assert tuple(y.shape) == (B,) and torch.equal(y, want), (tag, "score_rows", float((y - want).abs().max()))
            out.append(y)
        return out
    for k in range(scorer.graph_warmup):                                      # eager, counted per (size, same): nothing captured yet
        check("warm-up %d" % k, which=(k % 2,))
        assert not any(isinstance(g, (_RequestGraph, _RowsGraph)) for g in graphs())
    y_prev = check("capture")
    captured = graphs()
    assert [type(g) for g in captured] == [_RequestGraph, _RowsGraph], "score / score_rows with same= were not captured"
    assert untouched()
    where = tuple(cols.index(c) for c in same)                                 # keyed by the columns' positions inside the used columns
    assert list(scorer._same_graphs)[0][-1] == where and list(scorer._same_rows_graphs)[0][-1] == where
    steps = ["relabel"] + (["append"] if form != "immutable" else []) + (["evict", "delete"] if form == "window" else []) + ["train"]
    for step in steps:
        if step == "relabel":
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
            model.train_step(scorer.batch_rows(_up(sets[0].astype(np.int64), device), same=same))
            model.eval()
        assert len(scorer.index) == len(cur[0])
        y_new = check("after %s" % step)
        assert [a is b for a, b in zip(graphs(), captured)] == [True, True], "%s invalidated a captured graph" % step
        assert len(scorer._same_graphs) == 1 and len(scorer._same_rows_graphs) == 1 and untouched()
        assert not all(torch.equal(a, b) for a, b in zip(y_new, y_prev)), "%s changed no prediction" % step
        y_prev = y_new
    # another `same` is another entry; the plain calls go to their own dictionaries
    scorer.score(ids, same=[cols[0], cols[2]])
    scorer.score(ids, same=[cols[2], cols[0]])                                 # ... whatever order the columns are named in
    assert len(scorer._same_graphs) == 2 and untouched()
    scorer.score(ids)
    assert len(scorer._graphs) == 1 and len(scorer._same_graphs) == 2


# ---- 5. corrupt inputs (emulator only) ---------------------------------------------------------------------------------------------------
def check_corrupt(lib, capacity=600, guard=4096):
    """the entry points through the C ABI with every buffer between guard regions: headers outside their domains, horizons far
    outside, counts, the flag and first_row hostile.  The calls return normally, the guards are intact, the inputs are only read and
    what comes out is in range."""
    FILL = -99
    rs = np.random.RandomState(47)
    F, Q, K, Lr = 3, 5, 3, 4
    mask = 0b101

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
        for case, (n, head) in enumerate(headers):
            nc = min(max(n, 0), capacity)
            for groups in (1, 3):
                horizons = (hostile * 2)[3 * (groups - 1) + case % 3:][:Q]
                bufs = dict(db_t=guarded(F * capacity, torch.int32, 0), hdr=guarded(2, torch.int64, 0), ids=guarded(Q * Lr, torch.int32, 1),
                            cols=guarded(F, torch.int32, 0), before=guarded(Q, torch.int64, 0), counts=guarded(Q, torch.int64, 77),
                            ws=guarded(Q * groups, torch.int64, 5))
                bufs["db_t"][1][:] = torch.from_numpy(rs.randint(0, 3, size=F * capacity).astype(np.int32))
                bufs["hdr"][1][:] = torch.tensor([n, head])
                bufs["cols"][1][:] = torch.tensor([2, 0, 3], dtype=torch.int32)
                bufs["before"][1][:] = torch.tensor(horizons)
                read_only = {k: bufs[k][0].clone() for k in ("db_t", "hdr", "ids", "cols", "before")}
                lib.call("rat_bm25_exact_count", p(bufs["db_t"][1]), form, p(bufs["hdr"][1]), 0, capacity, p(bufs["ids"][1]),
                         p(bufs["cols"][1]), mask, p(bufs["before"][1]), p(bufs["counts"][1]), p(bufs["ws"][1]), Q * groups * 8, Q, Lr, F,
                         groups, None)
                intact(bufs, read_only, ("count", form, n, head, groups))
                horizon = np.clip(np.asarray(horizons, dtype=object), 0, nc).astype(np.int64)
                c = bufs["counts"][1].numpy()
                assert ((c >= 0) & (c <= horizon)).all(), ("count", form, n, head, c, horizon)
                # the scan under the same header and horizons, the flag hostile as well
                ws_words = Q * groups * K * 2
                for flag in (0, (1, -7, 2 ** 31 - 1)[case % 3]):
                    bufs = dict(db_t=guarded(F * capacity, torch.int32, 0), hdr=guarded(2, torch.int64, 0), q_ids=guarded(Q * F, torch.int32, 1),
                                q_idf=guarded(Q * F, torch.float64, 1.5), before=guarded(Q, torch.int64, 0), flag=guarded(1, torch.int32, flag),
                                out_v=guarded(Q * K, torch.float64, 7.0), out_i=guarded(Q * K, torch.int64, 77),
                                out_l=guarded(Q, torch.int64, 77), ws=guarded(ws_words, torch.int64, 5))
                    bufs["db_t"][1][:] = torch.from_numpy(rs.randint(0, 3, size=F * capacity).astype(np.int32))
                    bufs["hdr"][1][:] = torch.tensor([n, head])
                    bufs["before"][1][:] = torch.tensor(horizons)
                    read_only = {k: bufs[k][0].clone() for k in ("db_t", "hdr", "q_ids", "q_idf", "before", "flag")}
                    lib.call("rat_bm25_topk_split_exact", p(bufs["db_t"][1]), form, p(bufs["hdr"][1]), 0, capacity, p(bufs["q_ids"][1]),
                             p(bufs["q_idf"][1]), mask, p(bufs["before"][1]), p(bufs["flag"][1]), p(bufs["out_v"][1]), p(bufs["out_i"][1]),
                             p(bufs["out_l"][1]), p(bufs["ws"][1]), ws_words * 8, Q, F, K, groups, None)
                    intact(bufs, read_only, ("scan", form, n, head, groups, flag))
                    got_i, got_l = bufs["out_i"][1].numpy().reshape(Q, K), bufs["out_l"][1].numpy()
                    assert ((got_i >= -1) & (got_i < np.maximum(horizon, 0)[:, None])).all() and ((got_l >= 0) & (got_l <= K)).all()
                    assert (got_l[horizon == 0] == 0).all()
                    if flag:                                # listed: ascending, value 1.0
                        for j in range(Q):
                            kept = got_i[j][got_i[j] >= 0]
                            assert len(kept) == got_l[j] and (np.diff(kept) > 0).all()
                            assert (bufs["out_v"][1].numpy().reshape(Q, K)[j, :len(kept)] == 1.0).all()
    # the plan over hostile counts, and the prepare over what a plan could never write
    for counts in ([0] * Q, hostile[:Q], hostile[5:5 + Q], [-1, -2 ** 63, 0, 2 ** 63 - 1, 1], [2 ** 40] * Q):
        bufs = dict(counts=guarded(Q, torch.int64, 0), first=guarded(Q, torch.int64, 77), flag=guarded(1, torch.int32, 77))
        bufs["counts"][1][:] = torch.tensor(counts)
        read_only = {"counts": bufs["counts"][0].clone()}
        lib.call("rat_bm25_exact_plan", p(bufs["counts"][1]), p(bufs["first"][1]), p(bufs["flag"][1]), Q, K, None)
        intact(bufs, read_only, ("plan", counts))
        pos = [j for j, c in enumerate(counts) if c > 0]
        assert bufs["first"][1].tolist() == [pos[0] if pos else 0] * Q and int(bufs["flag"][1][0]) == int(max(counts + [0]) <= K)
    tab_ids, tab_idf = torch.arange(6, dtype=torch.int32), torch.full((6,), 1.5, dtype=torch.float64)
    tab_off = torch.tensor([0, 2, 4, 6], dtype=torch.int64)
    bufs = dict(ids=guarded(Q * Lr, torch.int32, 1), first=guarded(Q, torch.int64, 0), q_ids=guarded(Q * F, torch.int32, 77),
                q_idf=guarded(Q * F, torch.float64, 7.0))
    bufs["first"][1][:] = torch.tensor(hostile[1:1 + Q])
    read_only = {k: bufs[k][0].clone() for k in ("ids", "first")}
    cols = torch.tensor([2, 0, 3], dtype=torch.int32)
    lib.call("rat_bm25_query_prepare_seg", p(bufs["ids"][1]), p(bufs["first"][1]), p(cols), p(tab_ids),
             p(tab_idf), p(tab_off), p(bufs["q_ids"][1]), p(bufs["q_idf"][1]), Q, Lr, F, None)
    intact(bufs, read_only, "prepare")
    assert (bufs["q_ids"][1] == 1).all()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def check_refusals(gpu, lib):
    import pytest
    from rat_amd import ops
    from rat_amd.online import OnlineScorer, RetrievalIndex
    device = _device(gpu)
    case, model, cfg, scorer, live, data, cols = rc._setup_scorer(gpu, lib, "immutable", 60)
    ids = np.ascontiguousarray(data[:6, :-1])
    unused = [c for c in range(live.shape[1] - 1) if c not in cols][0]
    launches = []
    names = ("bm25_query_prepare", "pool_gather_rows", "bm25_exact_count", "bm25_exact_plan", "bm25_topk_split_exact")
    real = [getattr(ops, name) for name in names]
    for name, fn in zip(names, real):
        setattr(ops, name, lambda *a, _fn=fn, _name=name, **k: launches.append(_name) or _fn(*a, **k))
    try:
        bad = [([], "non-empty"), ([cols[0], cols[0]], "repeated"), ([0.0], "integer"), ([True], "integer"), ([[cols[0]]], "1-D"),
               (cols[0], "1-D"), ([unused], "not a used column"), ([-1], "not a used column"), ([cols[0], 10 ** 6], "not a used column"),
               (list(cols), "at least one used column"), (np.zeros((1, 1), dtype=np.int64), "1-D")]
        calls = [lambda s: scorer.index.retrieve(ids, same=s), lambda s: scorer.index.retrieve(ids, before=[1] * 6, same=s),
                 lambda s: scorer.batch(ids, same=s), lambda s: scorer.score(ids, same=s), lambda s: scorer.batch_rows([0, 1], same=s),
                 lambda s: scorer.score_rows([0, 1], same=s), lambda s: scorer.evaluate_rows([0, 1], same=s)]
        for same, word in bad:
            for call in calls:
                with pytest.raises(ValueError, match=word):
                    call(same)
        with pytest.raises(ValueError, match="request_offsets"):
            scorer.index.retrieve(ids, [0, 2, 6], same=[cols[0]])
        with pytest.raises(ValueError, match="request_offsets"):
            scorer.index.retrieve(ids, request_offsets=np.array([0, 6]), same=[cols[0]])
        assert launches == [], "a refused call launched something"
        # the constructor refusals are what they were: the restriction is per call, the config keys stay refused
        good = dict(topK=3, used_col_indices=cols, label_wise=False)
        with pytest.raises(ValueError, match="exact-match"):
            OnlineScorer(model, live, dict(good, exact_match_col_indices=[0]), lib=lib)
        with pytest.raises(ValueError, match="exact-match"):
            OnlineScorer(model, live, dict(topK=3, used_cols=["a", "b"], exact_match_cols=["a"]), lib=lib)
        with pytest.raises(ValueError, match="exact-match"):
            RetrievalIndex(live, cols, 3, device, lib=lib, exact_match_col_indices=[1])
        y = scorer.score(ids, same=[cols[0]])                                  # and a good one goes through, in this order
        assert tuple(y.shape) == (6,)
        assert launches == ["bm25_exact_count", "bm25_exact_plan", "bm25_query_prepare", "bm25_topk_split_exact"], launches
    finally:
        for name, fn in zip(names, real):
            setattr(ops, name, fn)
