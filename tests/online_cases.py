"""Checks of the online scoring path shared by tests/test_online.py (CPU, host-emulation build) and tests/test_gpu_online.py (MI355X).

References: the query-side IDF mapping against the host function the offline path uses (rat_amd.retrieval.map_data_to_idf, itself
held to the real reference's output by tests/golden/retrieval.npz); the split top-K against oracle/retrieval_oracle.py, the golden
arrays and — bit for bit — the single-range kernel rat_bm25_topk; the whole chain against the offline pipeline
(precompute_retrieval -> DeviceRetrievalBatches -> forward) on the same rows."""
import ctypes
import os

import numpy as np
import torch

import golden_cases as gc
import model_cases as mc
import retrieval_cases as rc
from oracle import retrieval_oracle as ro

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retrieval.npz")
SPLITS = (1, 2, 3, 7, 64)


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def upload_tables(tables, device):
    """retrieval.idf_tables -> the three flat device arrays rat_bm25_query_prepare reads"""
    return (_up(np.concatenate([v for v, _ in tables]).astype(np.int32), device),
            _up(np.concatenate([w for _, w in tables]).astype(np.float64), device),
            _up(np.concatenate([[0], np.cumsum([len(v) for v, _ in tables])]).astype(np.int64), device))


# ---- 1. prepare == host mapping ---------------------------------------------------------------------------------------------------
def check_prepare(name, device, lib):
    from rat_amd import ops, retrieval
    case = rc.CASES[name]
    db, qry = rc.make_case(case)
    F = db.shape[1]
    tables = retrieval.idf_tables(db)
    dev_tables = upload_tables(tables, device)
    hits = np.stack([np.isin(qry[:, c], tables[c][0]) for c in range(F)], axis=1)
    first_full_hit = int(np.nonzero(hits.all(axis=1))[0][0])
    variants = {"as_is": qry, "row0_hits": np.roll(qry, -first_full_hit, axis=0)}
    if case["unseen"]:
        assert not hits[0].any() and not hits[1, 0]                       # row 0 misses in every column: every weight is truncated
    for tag, q in variants.items():
        want = retrieval.map_data_to_idf(q, tables)
        if tag == "row0_hits":
            assert (want != np.trunc(want)).any()                         # the untruncated weights are really compared
        got_ids, got_idf = ops.bm25_query_prepare(_up(q.astype(np.int32), device), _up(np.arange(F, dtype=np.int32), device),
                                                  *dev_tables, lib=lib)
        assert np.array_equal(got_ids.cpu().numpy(), q.astype(np.int32)), (name, tag)
        assert np.array_equal(got_idf.cpu().numpy(), want), (name, tag)
        # the used columns as a non-monotone subset of a wider encoded row
        rs = np.random.RandomState(77)
        L = F + 3
        cols = rs.permutation(L)[:F]
        if F > 1 and (np.diff(cols) > 0).all():
            cols = cols[::-1].copy()
        wide = rs.randint(0, 50, size=(len(q), L))
        wide[:, cols] = q
        got_ids, got_idf = ops.bm25_query_prepare(_up(wide.astype(np.int32), device), _up(cols.astype(np.int32), device), *dev_tables,
                                                  lib=lib)
        assert np.array_equal(got_ids.cpu().numpy(), q.astype(np.int32)), (name, tag, "subset")
        assert np.array_equal(got_idf.cpu().numpy(), want), (name, tag, "subset")


# ---- 2. split top-K == oracle, golden arrays and the single-range kernel ------------------------------------------------------------
def device_inputs(db, qry, device):
    from rat_amd import retrieval
    q_idf = retrieval.map_data_to_idf(qry, retrieval.idf_tables(db))
    return _up(db.astype(np.int32).T, device), _up(qry.astype(np.int32), device), _up(q_idf, device)


def single_range_topk(lib, db_t, q_ids, q_idf, topk):
    """rat_bm25_topk (the offline kernel, unchanged) on device tensors"""
    F, N = db_t.shape
    Q = q_ids.shape[0]
    out_v = torch.empty((Q, topk), dtype=torch.float64, device=db_t.device)
    out_i = torch.empty((Q, topk), dtype=torch.int64, device=db_t.device)
    out_l = torch.empty((Q,), dtype=torch.int64, device=db_t.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(db_t.device).cuda_stream) if db_t.is_cuda else None
    lib.call("rat_bm25_topk", *[ctypes.c_void_p(t.data_ptr()) for t in (db_t, q_ids, q_idf, out_v, out_i, out_l)], N, Q, F, topk, stream)
    return out_v, out_i, out_l


def assert_bitwise(got, want, what):
    for g, w, part in zip(got, want, ("values", "indices", "lens")):
        assert torch.equal(g.view(torch.int64), w.view(torch.int64)), (what, part)


def check_split_case(name, device, lib, splits=SPLITS):
    from rat_amd import ops
    case = rc.CASES[name]
    db, qry = rc.make_case(case)
    K = case["topk"]
    assert max(splits) > len(db) / 256                                     # some ranges are shorter than 256 rows or empty
    g = np.load(GOLD)
    gold = tuple(g["%s/whole/%s" % (name, k)] for k in ("values", "indices", "lens"))
    want = ro.topk(db, qry, K)
    sc = ro.scores(db, qry)
    db_t, q_ids, q_idf = device_inputs(db, qry, device)
    single = single_range_topk(lib, db_t, q_ids, q_idf, K)
    for s in splits:
        got_t = ops.bm25_topk_split(db_t, q_ids, q_idf, K, splits=s, lib=lib)
        got = tuple(t.cpu().numpy() for t in got_t)
        np.testing.assert_array_equal(got[1], want[1], err_msg="%s splits=%d" % (name, s))
        np.testing.assert_array_equal(got[2], want[2], err_msg="%s splits=%d" % (name, s))
        np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-12)
        ro.assert_topk_equivalent(sc, got, gold)
        assert_bitwise(got_t, single, "%s splits=%d" % (name, s))


def check_split_ties(device, lib):
    """tests/test_retrieval.py:check_same_lane_ties' pool — equal scores at rows 0, 256 and 512, a better one arriving later — with
    2, 3 and 4 ranges (512 / 342 / 256 rows each): the tied rows fall into different ranges and meet again in the merge."""
    from rat_amd import ops
    for topk in (2, 3, 9):
        db = np.full((1024, 2), 7, dtype=np.int64)
        db[:, 0] = np.arange(1024) % 5 + 10
        for r in (0, 256, 300, 512, 700):
            db[r, 1] = 3
        db[512, 0], db[700, 0] = 99, 98
        db[[0, 256, 300], 0] = 50
        qry = np.array([[99, 3], [98, 3]], dtype=np.int64)
        want = ro.topk(db, qry, topk)
        assert want[1][0][:2].tolist() == [512, 0] and (topk < 3 or want[1][0][2] == 256)
        db_t, q_ids, q_idf = device_inputs(db, qry, device)
        for s in (2, 3, 4):
            chunk = -(-1024 // s)
            assert len({r // chunk for r in (0, 256, 512)}) >= 2
            got = tuple(t.cpu().numpy() for t in ops.bm25_topk_split(db_t, q_ids, q_idf, topk, splits=s, lib=lib))
            np.testing.assert_array_equal(got[1], want[1], err_msg="topk=%d splits=%d" % (topk, s))
            np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-12)
            np.testing.assert_array_equal(got[2], want[2])


def check_split_large_bitwise(device, lib, n_qry, topk):
    """200 000-row pool, three columns: values, indices and lens bitwise equal to rat_bm25_topk's for the library's own choice and
    for explicit range counts, one of which does not divide the pool and one of which leaves ranges under a thousand rows"""
    from rat_amd import ops
    rs = np.random.RandomState(100 + n_qry + topk)
    vocab = [5000, 3000, 200]
    db = np.stack([rs.randint(0, v, size=200_000) for v in vocab], axis=1).astype(np.int64)
    qry = np.stack([rs.randint(0, v, size=n_qry) for v in vocab], axis=1).astype(np.int64)
    db_t, q_ids, q_idf = device_inputs(db, qry, device)
    single = single_range_topk(lib, db_t, q_ids, q_idf, topk)
    assert int(single[2].min()) > 0
    for s in (0, 1, 8, 61, 256):
        assert_bitwise(ops.bm25_topk_split(db_t, q_ids, q_idf, topk, splits=s, lib=lib), single, "Q=%d K=%d splits=%d" % (n_qry, topk, s))


# ---- 3. online == offline, end to end ---------------------------------------------------------------------------------------------
def make_tables(case, n_pool, n_qry, seed):
    """-> (data [n_qry, L + 1], pool [n_pool, L + 1], used column indices): encoded rows inside the model's vocabularies, label last.
    The pool draws its categorical ids from the lower part of each vocabulary only, so some query ids are absent from it."""
    rs = np.random.RandomState(seed)
    specs = gc.feature_specs(case)

    def table(n, narrow):
        cols = []
        for f in case["fields"]:
            v = f["vocab_size"]
            if f["type"] == "sequence":
                ids = rs.randint(0, v - 1, size=(n, f["max_len"]))
                pad = np.arange(f["max_len"])[None, :] >= rs.randint(0, f["max_len"] + 1, size=(n, 1))
                ids[pad] = v - 1
            else:
                ids = rs.randint(0, max(v - 3, 2) if narrow else v, size=(n, 1))
            cols.append(ids)
        return np.concatenate(cols + [rs.randint(0, 2, size=(n, 1))], axis=1).astype(np.float64)
    used = [s["index"] for s in specs.values() if s["type"] == "categorical"]
    return table(n_qry, False), table(n_pool, True), used


def offline(model, data, pool, cfg, cols, device, lib):
    from rat_amd import retrieval
    from rat_amd.data import DeviceRetrievalBatches
    idx, val, lens = retrieval.precompute_retrieval(data, cfg, cols, pool_array=pool, device=device, lib=lib)
    src = DeviceRetrievalBatches(data, pool, idx, batch_size=len(data), device=device, lib=lib, retr_lens=lens)
    batches = list(src)
    assert len(batches) == 1
    with torch.no_grad():
        y = model.forward(batches[0])["y_pred"].reshape(-1).clone()
    return idx, val, lens, batches[0], y


def check_online_vs_offline(name, gpu, lib, sizes, graph, n_pool=14, train_step=False):
    from rat_amd.online import OnlineScorer, _RequestGraph
    case = gc.case_by_name(name)
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    mc.load_weights(model, case)
    model.eval()
    K = case["topk"]
    data_all, pool, cols = make_tables(case, n_pool, max(sizes), seed=5)
    cfg = dict(topK=K, used_col_indices=cols, qry_batch_size=None, label_wise=False, split_type="random")
    exercised = dict(short=False, absent=False)
    for B in sizes:
        data = data_all[:B]
        ids = np.ascontiguousarray(data[:, :-1])
        idx, val, lens, off_batch, y_off = offline(model, data, pool, cfg, cols, device, lib)
        y_again = offline(model, data, pool, cfg, cols, device, lib)[4]
        exact = torch.equal(y_off, y_again)            # the parent's eval forward, run twice on one batch: identical bits expected

        def same_pred(y):
            # identical kernels on identical inputs; were the offline forward itself not run-to-run identical, the tolerance of
            # model_cases.check_eval (2e-6 absolute) applies instead
            assert y.shape == y_off.shape and y.dtype == torch.float32
            assert torch.equal(y, y_off) if exact else float((y - y_off).abs().max()) <= 2e-6
        exercised["short"] |= bool((lens < K).any())
        exercised["absent"] |= any(not np.isin(data[:, c], pool[:, c]).all() for c in cols)
        eager = OnlineScorer(model, pool, cfg, graph=False, lib=lib)
        v, i, ln = eager.index.retrieve(ids)
        assert np.array_equal(i.cpu().numpy(), idx) and np.array_equal(ln.cpu().numpy(), lens)
        assert np.array_equal(v.cpu().numpy(), val)
        b = eager.batch(ids)
        assert torch.equal(b.idx, off_batch.idx) and torch.equal(b.label_ids, off_batch.label_ids)
        assert float(b.y_true.abs().max()) == 0.0 and len(b) == B
        y_eager = eager.score(ids)
        same_pred(y_eager)
        ids_dev = torch.from_numpy(ids.astype(np.int32)).to(device)
        assert torch.equal(eager.score(ids_dev), y_eager)                 # device int32 and host numpy float64: the same request
        assert torch.equal(eager.score(torch.from_numpy(ids)), y_eager)
        if not graph:
            continue
        scorer = OnlineScorer(model, pool, cfg, graph=True, lib=lib)
        for _ in range(scorer.graph_warmup):
            same_pred(scorer.score(ids_dev))
            assert not any(isinstance(e[1], _RequestGraph) for e in scorer._graphs.values())
        y_replay = scorer.score(ids_dev)
        assert [isinstance(e[1], _RequestGraph) for e in scorer._graphs.values()] == [True], "the request was not captured"
        assert torch.equal(y_replay, y_eager)                             # replay == eager, bit for bit
        other = np.roll(ids, 1, axis=0)
        assert torch.equal(scorer.score(other), eager.score(other))       # the static input is refreshed on every replay
        if train_step:
            model.train()
            model.train_step(off_batch)
            model.eval()
            y_new = scorer.score(ids_dev)                                  # still the captured graph: it reads the weights at replay time
            assert len(scorer._graphs) == 1
            assert torch.equal(y_new, OnlineScorer(model, pool, cfg, graph=False, lib=lib).score(ids_dev))
            assert not torch.equal(y_new, y_eager), "the training step changed nothing"
    assert exercised["short"] and exercised["absent"], exercised


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def check_refusals(gpu, lib):
    import pytest
    from rat_amd.online import OnlineScorer, RetrievalIndex
    case = gc.case_by_name("tiny_seq_bn")
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    model.eval()
    _, pool, cols = make_tables(case, 14, 4, seed=5)
    good = dict(topK=3, used_col_indices=cols, label_wise=False)
    OnlineScorer(model, pool, good, graph=False, lib=lib)
    with pytest.raises(ValueError, match="exact-match"):
        OnlineScorer(model, pool, dict(good, exact_match_col_indices=[0]), lib=lib)
    with pytest.raises(ValueError, match="exact-match"):
        OnlineScorer(model, pool, dict(topK=3, used_cols=["a", "b"], exact_match_cols=["a"]), lib=lib)
    with pytest.raises(ValueError, match="exact-match"):
        RetrievalIndex(pool, cols, 3, device, lib=lib, exact_match_col_indices=[1])
    with pytest.raises(ValueError, match="label_wise"):
        OnlineScorer(model, pool, dict(good, label_wise=True), lib=lib)
    with pytest.raises(ValueError, match="topK"):
        OnlineScorer(model, pool, dict(good, topK=33), lib=lib)
    with pytest.raises(ValueError, match="used columns"):
        OnlineScorer(model, np.zeros((5, 41)), dict(good, used_col_indices=list(range(33))), lib=lib)
    model._dp = lambda: True
    with pytest.raises(ValueError, match="data-parallel"):
        OnlineScorer(model, pool, good, lib=lib)
    del model._dp
    # columns by name resolve through the feature map like the offline path's retrieval.used_col_indices
    by_name = OnlineScorer(model, pool, dict(topK=3, used_cols=["e", "a"]), graph=False, lib=lib)
    assert by_name.index.cols.cpu().tolist() == [5, 0]                    # a, b, c (3 columns), e
