"""Checks of requests that share a launch (RetrievalIndex.retrieve(ids, request_offsets), OnlineScorer.batch_requests /
score_requests, rat_bm25_query_prepare_seg), shared by tests/test_online_requests.py (CPU, host-emulation build) and
tests/test_gpu_online_requests.py (MI355X).

The reference of every check is the request sent ALONE through the path that was there before: ``retrieve(request_r)``,
``batch(request_r)``, ``score(request_r)`` — one query batch of the reference each (tests/online_cases.py holds that path to the
offline pipeline).  The inputs are built against ``retrieval.map_data_to_idf`` on the host so that the requests of one batch disagree
on the mapping's dtype rule: concatenating them into one query batch gives other weights than mapping them one by one."""
import ctypes

import numpy as np
import torch

import golden_cases as gc
import model_cases as mc
import online_cases as oc

FORMS = ("immutable", "capacity", "window")
CAPACITY = 16
EVAL_GATE = 2e-6                     # model_cases.check_eval's absolute gate on y_pred: the margin recorded for the eval forward


def _setup(name, gpu, n_pool=14, seed=5):
    case = gc.case_by_name(name)
    model = mc.build_model(case, gpu=gpu, seed=1)
    mc.load_weights(model, case)
    model.eval()
    data, pool, cols = oc.make_tables(case, n_pool + 8, 24, seed=seed)
    cfg = dict(topK=case["topk"], used_col_indices=cols, qry_batch_size=None, label_wise=False, split_type="random")
    return case, model, data, pool, cols, cfg


def _form(form, pool, n_pool):
    """-> (constructor rows, constructor keywords, rows appended afterwards, the live rows in age order).  The window is filled past
    its capacity, so its head has moved and the live rows wrap around the end of the buffers."""
    if form == "immutable":
        return pool[:n_pool], {}, None, pool[:n_pool]
    if form == "capacity":
        return pool[:n_pool - 3], dict(capacity=n_pool + 5), pool[n_pool - 3:n_pool], pool[:n_pool]
    assert form == "window" and n_pool + 5 > CAPACITY > n_pool - 3
    live = pool[:n_pool + 5][-CAPACITY:]
    return pool[:n_pool], dict(capacity=CAPACITY, window=True), pool[n_pool:n_pool + 5], live


def _absent_ids(case, live, cols):
    """per used column an id inside the model's vocabulary that no live row holds (the pool draws from the lower part only)"""
    cat = [f for f in case["fields"] if f["type"] == "categorical"]
    assert len(cat) == len(cols)
    out = {}
    for c, f in zip(cols, cat):
        free = [v for v in range(f["vocab_size"]) if v != f.get("padding_idx") and not (live[:, c] == v).any()]
        assert free, "column %d: the pool holds the whole vocabulary" % c
        out[c] = free[-1]
    return out


def make_mixes(case, data, live, cols, sizes=(3, 1, 4, 2, 6, 1)):
    """-> two lists of requests (id arrays [B_r, L], float64 as the encoded tables are) over the same rows.  Mix "hit0": request 0
    opens with a row that hits in every used column, requests 2 and 4 open with a row that misses in one (an id no live row holds)
    while their later rows hit there.  Mix "miss0" is the same requests with request 0 moved behind request 2: now the batch opens
    with a miss and a later request opens with a hit."""
    rows = data[:sum(sizes), :-1].copy()
    absent = _absent_ids(case, live, cols)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    reqs = [rows[a:b] for a, b in zip(starts[:-1], starts[1:])]
    for r, req in enumerate(reqs):
        for k in range(len(req)):
            req[k, cols] = live[(3 * r + 5 * k) % len(live), cols]            # every row hits in every used column ...
    reqs[2][0, cols[0]] = absent[cols[0]]                                      # ... but for these first rows
    reqs[4][0, cols[-1]] = absent[cols[-1]]
    reqs[4][0, cols[0]] = absent[cols[0]]
    reqs[5][0, cols[0]] = absent[cols[0]]                                      # a one-row request that misses
    return dict(hit0=reqs, miss0=[reqs[2], reqs[1], reqs[0], reqs[3], reqs[4], reqs[5]])


def _offsets(reqs):
    return np.concatenate([[0], np.cumsum([len(r) for r in reqs])]).astype(np.int64)


def host_properties(reqs, live, cols, exercised):
    """what the inputs are, established on the host against retrieval.map_data_to_idf (nothing of the code under test)"""
    from rat_amd import retrieval
    db = live[:, cols].astype(int)
    tables = retrieval.idf_tables(db)
    first_hits = [np.array([np.isin(r[0, c], db[:, f]) for f, c in enumerate(cols)]) for r in reqs]
    for r in range(1, len(reqs)):
        exercised["first_row_misses_where_request0_hits"] |= bool((first_hits[0] & ~first_hits[r]).any())
        exercised["first_row_hits_where_request0_misses"] |= bool((~first_hits[0] & first_hits[r]).any())
    cat = np.concatenate(reqs)[:, cols].astype(int)
    whole = retrieval.map_data_to_idf(cat, tables)
    each = np.concatenate([retrieval.map_data_to_idf(r[:, cols].astype(int), tables) for r in reqs])
    exercised["host_mapping_differs"] |= bool((whole != each).any())
    return each


# ---- 1. retrieval parity, bit for bit ----------------------------------------------------------------------------------------------
def check_retrieval_parity(name, gpu, lib, form, splits, n_pool=14):
    from rat_amd import ops
    from rat_amd.online import RetrievalIndex
    case, _model, data, pool, cols, _cfg = _setup(name, gpu, n_pool=n_pool)
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    K = case["topk"]
    first, kw, later, live = _form(form, pool, n_pool)
    exercised = dict(first_row_misses_where_request0_hits=False, first_row_hits_where_request0_misses=False, host_mapping_differs=False,
                     plain_retrieve_differs=False)
    for s in splits:
        index = RetrievalIndex(first, cols, K, device, lib=lib, splits=s, **kw)
        if later is not None:
            index.append(later)
        assert len(index) == len(live)
        if form == "window":
            assert int(index.count[1]) + len(live) > CAPACITY, "the window does not wrap"
        for tag, reqs in make_mixes(case, data, live, cols).items():
            what = "%s %s splits=%d" % (form, tag, s)
            want_idf = host_properties(reqs, live, cols, exercised)
            cat, off = np.concatenate(reqs), _offsets(reqs)
            assert len({len(r) for r in reqs}) > 2                          # requests of unequal sizes
            alone = [index.retrieve(r) for r in reqs]
            want = tuple(torch.cat([a[k] for a in alone]) for k in range(3))
            got = index.retrieve(cat, off)
            oc.assert_bitwise(got, want, what)
            assert got[0].dtype == torch.float64 and got[1].dtype == torch.int64 and tuple(got[1].shape) == (len(cat), K)
            # the offsets in every accepted form: a list, int32 numpy, a host tensor and - unread - a device tensor
            variants = [off.tolist(), off.astype(np.int32), torch.from_numpy(off)] + ([torch.from_numpy(off).to(device)] if gpu >= 0 else [])
            for o in variants:
                oc.assert_bitwise(index.retrieve(cat, o), want, what)
            # the mapping itself against the host function, request by request
            first_row = torch.from_numpy(np.repeat(off[:-1], np.diff(off))).to(device)
            ids_dev = torch.from_numpy(cat.astype(np.int32)).to(device)
            _q, idf = ops.bm25_query_prepare(ids_dev, index.cols, index.table_ids, index.table_idf, index.table_offsets,
                                             first_row=first_row, lib=lib)
            assert np.array_equal(idf.cpu().numpy(), want_idf), what
            plain = index.retrieve(cat)                                       # ONE query batch: another question, another answer
            exercised["plain_retrieve_differs"] |= not torch.equal(plain[0], want[0])
            one = index.retrieve(cat, [0, len(cat)])                          # a single request with offsets is the plain call
            oc.assert_bitwise(one, plain, what)
    assert all(exercised.values()), exercised


# ---- 2. assembly and prediction ----------------------------------------------------------------------------------------------------
def check_assembly_and_prediction(name, gpu, lib, form, n_pool=14):
    from rat_amd.online import OnlineScorer
    case, model, data, pool, cols, cfg = _setup(name, gpu, n_pool=n_pool)
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    first, kw, later, live = _form(form, pool, n_pool)
    scorer = OnlineScorer(model, first, cfg, graph=False, lib=lib, **kw)
    if later is not None:
        scorer.append(later)
    exercised = dict(plain_batch_differs=False)
    for tag, reqs in make_mixes(case, data, live, cols).items():
        what = "%s %s" % (form, tag)
        cat, off = np.concatenate(reqs), _offsets(reqs)
        alone = [scorer.batch(r) for r in reqs]
        b = scorer.batch_requests(reqs)
        assert len(b) == len(cat)
        for part in ("idx", "label_ids", "y_true"):
            assert torch.equal(getattr(b, part), torch.cat([getattr(a, part) for a in alone])), (what, part)
        exercised["plain_batch_differs"] |= not torch.equal(scorer.batch(cat).idx, b.idx)
        with torch.no_grad():
            y_model = model.forward(b)["y_pred"].reshape(-1).clone()         # the eval forward over the same B rows: the same launches
        y, got_off = scorer.score_requests(reqs)
        assert y.dtype == torch.float32 and tuple(y.shape) == (len(cat),) and torch.equal(y, y_model), what
        assert got_off.dtype == torch.int64 and np.array_equal(got_off.cpu().numpy(), off), what
        # the pair form, ids and offsets on the host or on the device
        pairs = [(cat, off), (torch.from_numpy(cat), off.tolist())]
        if gpu >= 0:
            pairs.append((torch.from_numpy(cat.astype(np.int32)).to(device), torch.from_numpy(off).to(device)))
        for ids, o in pairs:
            y2, off2 = scorer.score_requests((ids, o))
            assert torch.equal(y2, y) and np.array_equal(off2.cpu().numpy(), off), what
            b2 = scorer.batch_requests((ids, o))
            assert torch.equal(b2.idx, b.idx) and torch.equal(b2.label_ids, b.label_ids), what
        # request by request through score(): other batch sizes, so the head GEMMs may choose other shapes - the eval forward's margin
        y_alone = torch.cat([scorer.score(r) for r in reqs])
        worst = float((y - y_alone).abs().max())
        print("score_requests vs per-request score(), %s: worst |dy| = %.3g, bit-equal: %s" % (what, worst, torch.equal(y, y_alone)))
        if gpu >= 0:
            import margins
            margins.record("check_assembly_and_prediction", "%s/%s" % (name, what), "y_pred, absolute", worst, EVAL_GATE, arith=model.arith)
        assert worst <= EVAL_GATE, (what, worst)
        parts = [y[a:c] for a, c in zip(got_off[:-1].tolist(), got_off[1:].tolist())]
        assert [len(p) for p in parts] == [len(r) for r in reqs]
    assert all(exercised.values()), exercised


# ---- 3. graphs by bucket (GPU only) ------------------------------------------------------------------------------------------------
def _padded(reqs, P, filler):
    """the requests plus an explicit trailing request of P - B rows of `filler` (NOT the rows score_requests pads with)"""
    B = sum(len(r) for r in reqs)
    return reqs + ([np.repeat(filler[None, :], P - B, axis=0)] if P > B else []), B


def check_bucket_graphs(name, gpu, lib, form, train_step=True, n_pool=14):
    """One captured graph per bucket serves every request mix of the bucket, padded totals included, and survives append / delete /
    relabel_where / a training step.  Reference: a fresh OnlineScorer(graph=False) over the modelled pool — for a total that is a
    power of two its score_requests over the same requests (the same B rows, the same launches: exact); for a padded total its
    score_requests over the requests plus an explicit trailing request of OTHER rows (again the same P rows per launch: exact, and
    the pad rows' content is shown not to matter), and the unpadded eager result within the eval forward's margin."""
    from rat_amd.data import DeviceBatch
    from rat_amd.online import OnlineScorer, _BucketGraph
    assert gpu >= 0
    case, model, data, pool, cols, cfg = _setup(name, gpu, n_pool=n_pool)
    first, kw, later, live = _form(form, pool, n_pool)
    scorer = OnlineScorer(model, first, cfg, graph=True, lib=lib, **kw)
    if later is not None:
        scorer.append(later)
    mixes = make_mixes(case, data, live, cols)
    A, Bm = mixes["hit0"], mixes["miss0"]
    eight = [[A[0], A[1], A[2]], [Bm[0], Bm[1], Bm[2]], [A[2], A[3], A[5], A[1]]]       # 3 + 1 + 4, 4 + 1 + 3, 4 + 2 + 1 + 1 rows
    padded = [[A[2], A[3]], [A[4]], [Bm[0], Bm[1]], [A[0], A[3]]]                        # 6, 6, 5 and 5 rows: bucket 8
    sixteen = [A[:5]]                                                                    # 16 rows
    seventeen = [A]                                                                      # 17 rows: bucket 32
    filler = live[-1, :-1]
    cur = [live.copy()]

    def fresh():
        return OnlineScorer(model, cur[0], cfg, graph=False, lib=lib)

    def check(reqs, tag):
        B = sum(len(r) for r in reqs)
        P = 1 << (B - 1).bit_length()
        f = fresh()
        y, off = scorer.score_requests(reqs)
        assert tuple(y.shape) == (B,) and np.array_equal(off.numpy(), _offsets(reqs)), tag
        explicit, _ = _padded(reqs, P, filler)
        want = f.score_requests(explicit)[0][:B]
        assert torch.equal(y, want), (tag, float((y - want).abs().max()))
        if P > B:
            loose = f.score_requests(reqs)[0]
            worst = float((y - loose).abs().max())
            print("padded replay vs unpadded eager, %s B=%d: worst |dy| = %.3g, bit-equal: %s" % (tag, B, worst, torch.equal(y, loose)))
            assert worst <= EVAL_GATE, (tag, worst)
        return y

    def graphs():
        return [e[1] for e in scorer._bucket_graphs.values()]

    # warm-up: eager, nothing captured; then the capture; from then on replays
    for k in range(scorer.graph_warmup):
        check(eight[k], "warm-up %d" % k)
        assert not any(isinstance(g, _BucketGraph) for g in graphs())
    y_first = check(eight[0], "capture")
    assert [isinstance(g, _BucketGraph) for g in graphs()] == [True], "the bucket was not captured"
    captured = graphs()[0]
    for k, reqs in enumerate(eight + padded):                                 # other mixes, other totals: the same graph
        y = check(reqs, "bucket 8, mix %d" % k)
        assert len(scorer._bucket_graphs) == 1 and graphs()[0] is captured
    assert torch.equal(check(eight[0], "again"), y_first)
    assert len(scorer._graphs) == 0                                           # score()'s own dictionary: untouched
    # score() beside it: its graphs, its warm-up counting
    ids = torch.from_numpy(np.concatenate(eight[0]).astype(np.int32)).to(scorer.device)
    for _ in range(scorer.graph_warmup + 1):
        y_plain = scorer.score(ids)
    assert len(scorer._graphs) == 1 and len(scorer._bucket_graphs) == 1
    assert torch.equal(y_plain, fresh().score(ids))
    # further buckets
    for reqs in sixteen + seventeen:
        for k in range(scorer.graph_warmup + 2):
            check(reqs, "B=%d call %d" % (sum(len(r) for r in reqs), k))
    assert sorted(k[0] for k in scorer._bucket_graphs) == [8, 16, 32] and all(isinstance(g, _BucketGraph) for g in graphs())
    assert len(scorer._graphs) == 1
    before = graphs()
    # the pool changes under the captured graphs
    n_ids = live.shape[1] - 1
    steps = ["relabel"] + (["append"] if form != "immutable" else []) + (["delete"] if form == "window" else []) + ["train"]
    for step in steps:
        y_old = scorer.score_requests(eight[1])[0]
        if step == "relabel":
            _v, i, _l = scorer.index.retrieve(np.concatenate(eight[1]), _offsets(eight[1]))
            hit = np.unique(i.cpu().numpy())
            hit = hit[hit >= 0]
            keys = cur[0][hit][:, :-1].astype(np.int64)
            rows = (cur[0][:, None, :-1].astype(np.int64) == keys[None]).all(axis=2).any(axis=1)
            new = 1.0 - float(np.round(cur[0][rows, -1].mean()))
            count = scorer.relabel_where(list(range(n_ids)), keys, new)
            cur[0] = cur[0].copy()
            cur[0][rows, -1] = new
            assert int(count) == int(rows.sum())
        elif step == "append":
            rows = data[-3:].copy()
            rows[:, cols] = np.concatenate(eight[1])[:3][:, cols]               # rows the requests will retrieve
            scorer.append(rows)
            cur[0] = np.concatenate([cur[0], rows])[-CAPACITY:] if form == "window" else np.concatenate([cur[0], rows])
        elif step == "delete":
            _v, i, _l = scorer.index.retrieve(np.concatenate(eight[1]), _offsets(eight[1]))
            gone = np.unique(i.cpu().numpy())
            gone = gone[gone >= 0][:2]
            scorer.delete(gone)
            cur[0] = np.delete(cur[0], gone, axis=0)
        else:
            if not train_step:
                continue
            model.train()
            model.train_step(DeviceBatch(*scorer._assemble(ids)))
            model.eval()
        for reqs in (eight[1], padded[0], seventeen[0]):
            y_new = check(reqs, "after %s" % step)
        assert [a is b for a, b in zip(graphs(), before)] == [True] * 3, "%s invalidated a captured bucket" % step
        assert len(scorer._graphs) == 1
        assert not torch.equal(scorer.score_requests(eight[1])[0], y_old), "%s changed no prediction" % step


# ---- 4. a corrupt first_row addresses nothing outside the buffers (host-emulation build only) --------------------------------------
def check_seg_corrupt(lib, guard=4096):
    """rat_bm25_query_prepare_seg through the C ABI with every buffer between guard regions and first_row holding negative and
    far-too-large values: the call returns normally, the guards are intact, the inputs are only read, and rows whose first_row is
    valid get the weights of the host mapping"""
    from rat_amd import retrieval
    FILL = -99
    rs = np.random.RandomState(31)

    def guarded(values, dtype):
        values = torch.as_tensor(values, dtype=dtype).reshape(-1)
        whole = torch.full((values.numel() + 2 * guard,), FILL, dtype=dtype)
        whole[guard:guard + values.numel()] = values
        return whole, whole[guard:guard + values.numel()]

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    Q, L, cols = 9, 5, [3, 0]
    db = rs.randint(0, 6, size=(20, 2))
    tables = retrieval.idf_tables(db)
    ids = rs.randint(0, 9, size=(Q, L))
    ids[0, cols] = db[0]                                                       # row 0 hits, row 4 misses in both columns
    ids[4, cols] = 50
    lists = [[0] * Q, [0, 0, 0, 0, 4, 4, 4, 4, 4], [-1, Q, 10 ** 12, -10 ** 12, 2 ** 62, -2 ** 63, 2 ** 63 - 1, 2 ** 31, -2 ** 31], [Q - 1] * Q]
    for first_row in lists:
        bufs = dict(ids=guarded(ids, torch.int32), first_row=guarded(first_row, torch.int64), cols=guarded(cols, torch.int32),
                    table_ids=guarded(np.concatenate([v for v, _ in tables]), torch.int32),
                    table_idf=guarded(np.concatenate([w for _, w in tables]), torch.float64),
                    table_off=guarded(np.concatenate([[0], np.cumsum([len(v) for v, _ in tables])]), torch.int64),
                    qry_ids=guarded(np.zeros(Q * 2), torch.int32), qry_idf=guarded(np.zeros(Q * 2), torch.float64))
        read_only = {k: bufs[k][0].clone() for k in ("ids", "first_row", "cols", "table_ids", "table_idf", "table_off")}
        lib.call("rat_bm25_query_prepare_seg", p(bufs["ids"][1]), p(bufs["first_row"][1]), p(bufs["cols"][1]), p(bufs["table_ids"][1]),
                 p(bufs["table_idf"][1]), p(bufs["table_off"][1]), p(bufs["qry_ids"][1]), p(bufs["qry_idf"][1]), Q, L, 2, None)
        for name, (whole, _) in bufs.items():
            assert (whole[:guard] == FILL).all() and (whole[-guard:] == FILL).all(), (name, first_row)
        assert all(torch.equal(bufs[b][0], v) for b, v in read_only.items())
        assert np.array_equal(bufs["qry_ids"][1].numpy().reshape(Q, 2), ids[:, cols])
        got = bufs["qry_idf"][1].numpy().reshape(Q, 2)
        whole_w = retrieval.map_data_to_idf(ids[:, cols], tables)                 # row 0 opens: nothing truncated
        assert (whole_w != np.trunc(whole_w)).any()
        clamped = np.clip(np.asarray(first_row, dtype=object), 0, Q - 1).astype(np.int64)
        for q in range(Q):                                                     # the clamp is the contract: row `clamped[q]` decides
            want = retrieval.map_data_to_idf(ids[[clamped[q], q]][:, cols], tables)[1]
            assert np.array_equal(got[q], want), (first_row, q)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def check_request_refusals(gpu, lib):
    import pytest
    from rat_amd import ops
    from rat_amd.online import OnlineScorer
    case, model, data, pool, cols, cfg = _setup("tiny_seq_bn", gpu)
    scorer = OnlineScorer(model, pool[:14], cfg, graph=False, lib=lib)
    ids = np.ascontiguousarray(data[:6, :-1])
    launches = []
    real = ops.bm25_query_prepare
    ops.bm25_query_prepare = lambda *a, **k: launches.append(1) or real(*a, **k)      # the first launch of every chain
    try:
        bad = [([1, 3, 6], "start at 0"), ([0, 3, 5], "end at"), ([0, 3, 7], "end at"), ([0, 4, 2, 6], "ascending"), ([0, 3, 3, 6], "empty request"),
               (np.array([0.0, 3.0, 6.0]), "integers"), (torch.tensor([0.0, 6.0]), "integers"), (np.array([[0, 6]]), "1-D"), ([6], "1-D")]
        for off, word in bad:
            with pytest.raises(ValueError, match=word):
                scorer.index.retrieve(ids, off)
            for call in (scorer.score_requests, scorer.batch_requests):
                with pytest.raises(ValueError, match=word):
                    call((ids, off))
        for call in (scorer.score_requests, scorer.batch_requests):
            with pytest.raises(ValueError, match="columns"):
                call((ids[:, :-1], [0, 6]))
            with pytest.raises(ValueError, match="columns"):
                call([ids[:2], ids[2:, :-1]])
            with pytest.raises(ValueError, match="empty request"):
                call([ids[:2], ids[:0]])
            with pytest.raises(ValueError, match="empty request"):
                call([])
            with pytest.raises(ValueError, match="B_r, L"):
                call([ids[:2], ids[0]])
        with pytest.raises(ValueError, match="columns"):
            scorer.index.retrieve(ids[:, :-1], [0, 6])
        with pytest.raises(ValueError, match="empty request"):
            scorer.index.retrieve(ids[:0], [0, 0])
        assert launches == [], "a refused call launched something"
        model.train()
        with pytest.raises(RuntimeError, match="eval mode"):
            scorer.score_requests([ids[:2], ids[2:]])
        assert launches == []
        model.eval()
        y, off = scorer.score_requests([ids[:2], ids[2:]])                    # and a good one goes through
        assert tuple(y.shape) == (6,) and off.tolist() == [0, 2, 6] and len(launches) == 1
    finally:
        ops.bm25_query_prepare = real
