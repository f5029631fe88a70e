"""Checks of the growing pool (RetrievalIndex / OnlineScorer with ``capacity``) shared by tests/test_online_append.py (CPU,
host-emulation build) and tests/test_gpu_online_append.py (MI355X).

The reference of every comparison is the immutable path over the rows that count: rat_bm25_topk on a contiguous copy of the first n
rows at kernel level, a FRESH immutable RetrievalIndex / OnlineScorer over np.concatenate([pool, appended rows]) at object level
(itself tied to the offline pipeline and the oracle by tests/online_cases.py) — never the appended object against itself."""
import numpy as np
import torch

import golden_cases as gc
import model_cases as mc
import online_cases as oc

SPLITS = (1, 3, 64, 256)
POISON_ID = 7


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _count(n, device):
    return torch.full((1,), n, dtype=torch.int64, device=device)


# ---- 1. rat_bm25_topk_split_dev == rat_bm25_topk over the first n rows --------------------------------------------------------------
def poisoned_pool(capacity, seed):
    """-> (db [capacity, 3], qry [5, 3], weights [5, 3]).  Every query carries POISON_ID in column 0 with a weight above the sum of its
    other weights; a live row carries it rarely, so a scanned row with POISON_ID in column 0 beats almost every live row of EVERY query.
    Few distinct ids and weights: ties everywhere."""
    rs = np.random.RandomState(seed)
    db = np.stack([rs.randint(1, 6, size=capacity), rs.randint(0, 4, size=capacity), rs.randint(0, 3, size=capacity)], axis=1)
    db[rs.rand(capacity) < 0.02, 0] = POISON_ID
    qry = np.stack([np.full(5, POISON_ID), rs.randint(0, 4, size=5), rs.randint(0, 3, size=5)], axis=1)
    w = np.stack([np.full(5, 4.0), rs.choice([0.5, 1.0, 1.5], size=5), rs.choice([0.5, 1.0, 1.5], size=5)], axis=1)
    return db.astype(np.int64), qry.astype(np.int64), w.astype(np.float64)


def poison(db, n, rs):
    """rows [n, capacity) <- ids that match every query in its heaviest column (and some query in the others)"""
    out = db.copy()
    out[n:, 0] = POISON_ID
    out[n:, 1] = rs.randint(0, 4, size=len(db) - n)
    out[n:, 2] = rs.randint(0, 3, size=len(db) - n)
    return out


def check_split_dev(device, lib, capacity=1200, ns=(1, 255, 256, 1000, None), splits=SPLITS, topks=(3, 9)):
    from rat_amd import ops
    rs = np.random.RandomState(3)
    base, qry, w = poisoned_pool(capacity, seed=17)
    q_ids, q_idf = _up(qry.astype(np.int32), device), _up(w, device)
    assert max(splits) > min(ns[0], capacity) / 256                        # whole ranges are empty
    poison_would_win = False
    for n in ns:
        n = capacity if n is None else n
        db = poison(base, n, rs)
        db_t = _up(db.astype(np.int32).T, device)                          # [F][capacity]
        live_t = _up(db[:n].astype(np.int32).T, device)                    # [F][n], what the immutable path would hold
        for topk in topks:
            want = oc.single_range_topk(lib, live_t, q_ids, q_idf, topk)
            if n < capacity:
                whole = oc.single_range_topk(lib, db_t, q_ids, q_idf, topk)
                poison_would_win |= bool((whole[1] >= n).any())
            for s in splits + (0,):
                got = ops.bm25_topk_split(db_t, q_ids, q_idf, topk, splits=s, header=_count(n, device), lib=lib)
                oc.assert_bitwise(got, want, "n=%d K=%d splits=%d" % (n, topk, s))
    assert poison_would_win, "the rows beyond n would not have been retrieved anyway: the test shows nothing"


def check_split_dev_ties(device, lib, capacity=1500):
    """online_cases.check_split_ties' pool (equal scores at rows 0, 256 and 512, a better one arriving later) as the first 1024 rows
    of a larger buffer whose tail is poisoned: the tied rows fall into different ranges of the CURRENT row count"""
    from rat_amd import ops
    n = 1024
    for topk in (2, 3, 9):
        db = np.full((capacity, 2), 7, dtype=np.int64)
        db[:n, 0] = np.arange(n) % 5 + 10
        for r in (0, 256, 300, 512, 700):
            db[r, 1] = 3
        db[512, 0], db[700, 0] = 99, 98
        db[[0, 256, 300], 0] = 50
        db[n:] = [99, 3]                                                   # beyond n: the best possible match of query 0
        qry = np.array([[99, 3], [98, 3]], dtype=np.int64)
        db_t_live, q_ids, q_idf = oc.device_inputs(db[:n], qry, device)
        want = oc.single_range_topk(lib, db_t_live, q_ids, q_idf, topk)
        assert want[1][0][:2].tolist() == [512, 0] and (topk < 3 or int(want[1][0][2]) == 256)
        db_t = _up(db.astype(np.int32).T, device)
        for s in (2, 3, 4):
            chunk = -(-n // s)
            assert len({r // chunk for r in (0, 256, 512)}) >= 2
            got = ops.bm25_topk_split(db_t, q_ids, q_idf, topk, splits=s, header=_count(n, device), lib=lib)
            oc.assert_bitwise(got, want, "ties K=%d splits=%d" % (topk, s))


def check_split_dev_after_append(device, lib, capacity=700, n=300, M=70):
    """the SAME buffers and the same count tensor: poisoned rows are invisible, then rat_pool_append overwrites M of them with rows
    equal to query 0 and raises the count on the device — they are found, ahead of everything else, and nothing beyond them"""
    from rat_amd import ops
    rs = np.random.RandomState(4)
    base, qry, w = poisoned_pool(capacity, seed=23)
    db = poison(base, n, rs)
    twins = (db[:n] == qry[0]).all(axis=1)                                 # no live row equals query 0: the appended ones will be its best
    db[:n][twins, 1] = (db[:n][twins, 1] + 1) % 4
    q_ids, q_idf = _up(qry.astype(np.int32), device), _up(w, device)
    db_t, count, cols = _up(db.astype(np.int32).T, device), _count(n, device), _up(np.array([2, 0, 1], dtype=np.int32), device)
    topk = 5
    before = ops.bm25_topk_split(db_t, q_ids, q_idf, topk, splits=3, header=count, lib=lib)
    oc.assert_bitwise(before, oc.single_range_topk(lib, _up(db[:n].astype(np.int32).T, device), q_ids, q_idf, topk), "before")
    new = np.repeat(qry[:1], M, axis=0)                                    # [M, 3] in pool-column order
    wide = np.zeros((M, 4), dtype=np.int32)                                # encoded rows of 4 ids: pool column f is row column cols[f]
    wide[:, [2, 0, 1]] = new
    ops.pool_append(_up(wide, device), _up(np.ones(M, dtype=np.float32), device), cols, db_t, count, lib=lib)
    assert int(count.cpu()[0]) == n + M
    grown = np.concatenate([db[:n], new])
    for s in (1, 3, 64):
        got = ops.bm25_topk_split(db_t, q_ids, q_idf, topk, splits=s, header=count, lib=lib)
        oc.assert_bitwise(got, oc.single_range_topk(lib, _up(grown.astype(np.int32).T, device), q_ids, q_idf, topk), "after s=%d" % s)
        assert got[1][0].cpu().tolist() == list(range(n, n + topk))        # query 0: the appended rows, lowest index first
        assert int(got[1].max()) < n + M


# ---- 2. rat_pool_append == numpy concatenation ----------------------------------------------------------------------------------------
def check_pool_append(device, lib, sizes=(1, 63, 64, 65, 1000), spare=9):
    from rat_amd import ops
    rs = np.random.RandomState(8)
    L, cols, n0 = 5, [3, 0], 3
    capacity = n0 + sum(sizes) + 2 + 5 + spare
    FILL = -7
    ids = rs.randint(0, 1000, size=(capacity, L)).astype(np.int32)
    labels = rs.randint(0, 2, size=capacity).astype(np.float32)
    db_t = torch.full((len(cols), capacity), FILL, dtype=torch.int32, device=device)
    pool_ids = torch.full((capacity, L), FILL, dtype=torch.int32, device=device)
    pool_labels = torch.full((capacity,), float(FILL), dtype=torch.float32, device=device)
    db_t[:, :n0] = _up(ids[:n0][:, cols].T, device)
    pool_ids[:n0], pool_labels[:n0] = _up(ids[:n0], device), _up(labels[:n0], device)
    count, cols_d = _count(n0, device), _up(np.array(cols, dtype=np.int32), device)

    def append(lo, hi):
        ops.pool_append(_up(ids[lo:hi], device), _up(labels[lo:hi], device), cols_d, db_t, count, pool_ids, pool_labels, lib=lib)

    def check(n):
        assert int(count.cpu()[0]) == n
        assert np.array_equal(db_t.cpu().numpy()[:, :n], ids[:n][:, cols].T)
        assert np.array_equal(pool_ids.cpu().numpy()[:n], ids[:n]) and np.array_equal(pool_labels.cpu().numpy()[:n], labels[:n])
        assert (db_t.cpu().numpy()[:, n:] == FILL).all() and (pool_ids.cpu().numpy()[n:] == FILL).all()
        assert (pool_labels.cpu().numpy()[n:] == FILL).all()
    n = n0
    check(n)
    for M in sizes:
        append(n, n + M)
        n += M
        check(n)
    append(n, n + 2)                                                       # two appends queued back to back: the second reads the
    append(n + 2, n + 7)                                                   # count the first one's tail launch wrote, on the device
    n += 7
    check(n)
    # the bound on the device (the host API refuses before it gets here): a batch that does not fit writes nothing
    assert capacity - n == spare
    ops.pool_append(_up(ids[:spare + 1], device), _up(labels[:spare + 1], device), cols_d, db_t, count, pool_ids, pool_labels, lib=lib)
    check(n)
    # an index without the row store
    ops.pool_append(_up(ids[n:n + spare], device), _up(labels[n:n + spare], device), cols_d, db_t, count, lib=lib)
    assert int(count.cpu()[0]) == capacity and np.array_equal(db_t.cpu().numpy(), ids[:, cols].T)
    assert (pool_ids.cpu().numpy()[n:] == FILL).all()


# ---- 3. appended index / scorer == fresh immutable one over the concatenated pool ------------------------------------------------------
def _tables(case, n0, n_qry, seed):
    """online_cases.make_tables plus the rows to append: the request's own rows (so a query equals an appended row, and ids the narrow
    pool cannot hold arrive), then more pool-like and more request-like rows"""
    data, pool, cols = oc.make_tables(case, n0, n_qry, seed=seed)
    data[0, cols[0]] = pool[:, cols[0]].max() + 1       # the request's FIRST row misses in a column until its own row is appended
    _, more_pool, _ = oc.make_tables(case, 40, 1, seed=seed + 1)
    more_data, _, _ = oc.make_tables(case, 1, 40, seed=seed + 2)
    extra = np.concatenate([data[:1], data[1:], more_pool[:20], more_data[:20], more_pool[20:], more_data[20:]])
    return data, pool, cols, extra


def check_append_equals_fresh(name, gpu, lib, n0=4, pieces=(1, 7, 64), B=6, graph=False, train_step=False, seed=5):
    from rat_amd.online import OnlineScorer, RetrievalIndex, _RequestGraph
    case = gc.case_by_name(name)
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    mc.load_weights(model, case)
    model.eval()
    K = case["topk"]
    data, pool, cols, extra = _tables(case, n0, B, seed)
    capacity = n0 + sum(pieces)
    assert len(extra) >= sum(pieces)
    ids = np.ascontiguousarray(data[:, :-1])
    ids_dev = torch.from_numpy(ids.astype(np.int32)).to(device)
    cfg = dict(topK=K, used_col_indices=cols, qry_batch_size=None, label_wise=False, split_type="random")

    scorer = OnlineScorer(model, pool, cfg, graph=graph, lib=lib, capacity=capacity)
    index = RetrievalIndex(pool, cols, K, device, lib=lib, capacity=capacity)
    assert len(index) == index.n_db == n0 and scorer.index.capacity == capacity
    # what lies beyond the live rows must not matter: other ids than any row that will ever stand there
    scorer.pool_ids[n0:] = 1
    scorer.pool_labels[n0:] = 1.0
    scorer.index.db_t[:, n0:] = torch.from_numpy(ids[:1, cols].T.astype(np.int32)).to(device)        # would match request row 0
    exercised = dict(table_grows=False, miss_then_hit=False, first_row_flips=False, own_row_on_top=False, short_then_full=False,
                     short_after=False, padding_is_last_live_row=False)
    captured = None
    if graph:
        for _ in range(scorer.graph_warmup):
            scorer.score(ids_dev)
        scorer.score(ids_dev)
        captured = [e[1] for e in scorer._graphs.values()]
        assert [isinstance(g, _RequestGraph) for g in captured] == [True], "the request was not captured"

    def fresh_objects(cur):
        return OnlineScorer(model, cur, cfg, graph=False, lib=lib), RetrievalIndex(cur, cols, K, device, lib=lib)

    def compare(cur, tag):
        f_scorer, f_index = fresh_objects(cur)
        want = f_index.retrieve(ids)
        for obj in (index, scorer.index):
            assert len(obj) == obj.n_db == len(cur) and int(obj.count.cpu()[0]) == len(cur)
            oc.assert_bitwise(obj.retrieve(ids), want, tag)
        fb, b = f_scorer.batch(ids), scorer.batch(ids)
        assert torch.equal(b.idx, fb.idx) and torch.equal(b.label_ids, fb.label_ids) and torch.equal(b.y_true, fb.y_true), tag
        y_want, y_again = f_scorer.score(ids_dev), f_scorer.score(ids_dev)
        y = scorer.score(ids_dev)
        assert y.shape == y_want.shape and y.dtype == torch.float32
        # online_cases.check_online_vs_offline's rule: bitwise when the parent's forward is run-to-run bitwise, else its 2e-6
        assert torch.equal(y, y_want) if torch.equal(y_want, y_again) else float((y - y_want).abs().max()) <= 2e-6, tag
        if graph:
            now = [e[1] for e in scorer._graphs.values()]
            assert len(now) == len(captured) and all(a is b_ for a, b_ in zip(now, captured)), "append invalidated a captured request"
        return want, fb

    cur = pool
    (v0, i0, l0), _ = compare(cur, "no append")
    prev_lens, prev_hit0 = l0.cpu().numpy(), [bool(np.isin(data[0, c], cur[:, c])) for c in cols]
    at = 0
    for M in pieces:
        rows = extra[at:at + M]
        at += M
        exercised["table_grows"] |= any(not np.isin(rows[:, c], cur[:, c]).all() for c in cols)
        exercised["miss_then_hit"] |= any((~np.isin(data[:, c], cur[:, c]) & np.isin(data[:, c], rows[:, c])).any() for c in cols)
        # the three input forms, in turn: numpy float64, host tensor, device tensor
        form = {1: rows, 7: torch.from_numpy(rows)}.get(M, torch.from_numpy(rows).to(device))
        scorer.append(form)
        index.append(rows)
        n_before, cur = len(cur), np.concatenate([cur, rows])
        (v, i, ln), fb = compare(cur, "after +%d" % M)
        i, ln, v = i.cpu().numpy(), ln.cpu().numpy(), v.cpu().numpy()
        hit0 = [bool(np.isin(data[0, c], cur[:, c])) for c in cols]
        exercised["first_row_flips"] |= any(h and not p for h, p in zip(hit0, prev_hit0))
        for q in range(len(data)):                      # a query equal to an appended row: that row (or an equal, earlier one) on top
            same = np.nonzero((cur[:, cols] == data[q, cols]).all(axis=1))[0]
            if len(same) and same[0] >= n_before and v[q, 0] > 0:
                assert i[q, 0] == same[0]
                exercised["own_row_on_top"] = True
        exercised["short_then_full"] |= bool(((prev_lens < K) & (ln == K)).any())
        if (ln < K).any() and len(cur) < capacity:
            exercised["short_after"] = True
            q = int(np.nonzero(ln < K)[0][0])
            got_row = scorer.batch(ids).idx[q, K].cpu().numpy()            # the last neighbour slot is padding (-1)
            assert i[q, K - 1] == -1 and np.array_equal(got_row, cur[-1, :-1].astype(np.int32))
            assert not np.array_equal(got_row, scorer.pool_ids[capacity - 1].cpu().numpy())
            exercised["padding_is_last_live_row"] = True
        prev_lens, prev_hit0 = ln, hit0
    assert len(cur) == capacity and all(exercised.values()), exercised
    if graph and train_step:
        from rat_amd.data import DeviceBatch
        model.train()
        model.train_step(DeviceBatch(*scorer._assemble(ids_dev)))
        model.eval()
        y_new = scorer.score(ids_dev)                                      # still the graph captured before every append
        assert all(a is b_ for a, b_ in zip([e[1] for e in scorer._graphs.values()], captured)) and len(scorer._graphs) == 1
        assert torch.equal(y_new, OnlineScorer(model, cur, cfg, graph=False, lib=lib).score(ids_dev))


# ---- 4. refusals; capacity without appends == the immutable path ---------------------------------------------------------------------
def check_append_refusals(gpu, lib):
    import pytest
    from rat_amd.online import OnlineScorer, RetrievalIndex
    case = gc.case_by_name("tiny_seq_bn")
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    model.eval()
    data, pool, cols = oc.make_tables(case, 14, 4, seed=5)
    cfg = dict(topK=3, used_col_indices=cols, label_wise=False)
    with pytest.raises(ValueError, match="capacity"):
        OnlineScorer(model, pool, cfg, graph=False, lib=lib).append(data[:1])
    with pytest.raises(ValueError, match="capacity"):
        RetrievalIndex(pool, cols, 3, device, lib=lib).append(data[:1])
    with pytest.raises(ValueError, match="capacity"):
        RetrievalIndex(pool, cols, 3, device, lib=lib, capacity=len(pool) - 1)
    scorer = OnlineScorer(model, pool, cfg, graph=False, lib=lib, capacity=len(pool) + 3)
    ids = np.ascontiguousarray(data[:, :-1])
    state = lambda: [t.clone() for t in (scorer.index.db_t, scorer.index.count, scorer.pool_ids, scorer.pool_labels,   # noqa: E731
                                         scorer.index.table_ids, scorer.index.table_idf, scorer.index.table_offsets)]
    before, y_before = state(), scorer.batch(ids).idx.clone()
    with pytest.raises(ValueError, match="capacity"):
        scorer.append(data[:4])                                            # 14 + 4 > 17
    with pytest.raises(ValueError, match="columns"):
        scorer.append(data[:1, :-1])
    with pytest.raises(ValueError, match="columns"):
        scorer.append(np.concatenate([data[:1], data[:1]], axis=1))
    big = data[:1].copy()
    big[0, cols[0]] = 2.0 ** 31
    with pytest.raises(ValueError, match="int32"):
        scorer.append(big)
    with pytest.raises(ValueError, match="non-empty"):
        scorer.append(data[:0])
    assert len(scorer.index) == 14 and all(torch.equal(a, b) for a, b in zip(before, state()))
    assert torch.equal(scorer.batch(ids).idx, y_before)
    scorer.append(data[:3])                                                # exactly full is fine
    assert len(scorer.index) == 17
    with pytest.raises(ValueError, match="capacity"):
        scorer.append(data[:1])


def check_capacity_without_appends(name, gpu, lib, sizes, graph, train_step=False):
    """online_cases.check_online_vs_offline — every comparison with the offline pipeline — through scorers built with
    capacity = len(pool) and never appended to"""
    import rat_amd.online as online
    orig = online.OnlineScorer

    class Full(orig):
        def __init__(self, model, pool_array, retrieval_configs, graph=True, lib=None):
            super().__init__(model, pool_array, retrieval_configs, graph=graph, lib=lib, capacity=len(pool_array))
            assert self.index.capacity == len(pool_array)
    online.OnlineScorer = Full
    try:
        oc.check_online_vs_offline(name, gpu, lib, sizes=sizes, graph=graph, train_step=train_step)
    finally:
        online.OnlineScorer = orig
