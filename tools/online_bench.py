#!/usr/bin/env python3
"""Diagnostic: the request path of the retrieval and of online scoring on the MI355X.

    python tools/online_bench.py [--out profiles/online/online_bench.txt] [--quick]

Part 1 — for N in {100 k, 1.4 M} pool rows, F in {3, 13} columns, K = 5 and Q in {1, 4, 16, 64, 256, 4096} queries: rat_bm25_topk
(the offline kernel: one work-group per tile of four queries scans the whole pool) against rat_bm25_topk_split with splits = 0 (the
library's choice) and a sweep of explicit range counts.  Same process, the variants alternating, outputs compared for equality
before anything is timed.  Every variant is captured as a hipGraph of REPS back-to-back calls and the replays are timed with device
events (warm-up replays first, at least 0.5 s of timed work per point), so a figure is device time per call, free of launch issue.
Part 2 — latency of OnlineScorer.score() (retrieve -> assemble -> eval forward), eager and replayed, at B in {1, 16, 256} for the
MovieLens-real geometry (movielens_real_F3_K5_d10_B4096's model, 1.4 M-row synthetic pool): host clock around score() + synchronise.
--append — the growing pool instead (profiles/online/append_bench.txt): (i) OnlineScorer-independent cost of taking rows in,
RetrievalIndex.append(M rows) on an index with reserved capacity against the only way an immutable index has — a new RetrievalIndex
over np.concatenate([pool, rows]) — for M in {1, 64, 4096}; (ii) replayed score() latency of a scorer with capacity (1.4 M rows in
room for 2 M) against the immutable scorer over the same pool at B in {1, 16, 256}.  Host clock around a synchronise, the two sides
alternating round by round in one process, at least 0.5 s of timed work per point and side; mean, and min .. max over the rounds.
--window — the sliding pool instead (profiles/online/window_bench.txt), same geometry, clock and alternation: (i) replayed score() of a
scorer with capacity and window=True against the capacity-mode scorer over the same rows, at B in {1, 16, 256}, once with the ring's
head at 0 and once after enough pushes that the live rows wrap through the end of the buffer; (ii) append(M) on a FULL window (the M
oldest rows leave) against a new RetrievalIndex over the shifted pool, for M in {1, 64, 4096}.
--delete — deletion from the sliding pool instead (profiles/online/delete_bench.txt), same geometry, clock and alternation:
(i) RetrievalIndex.delete(m seeded random rows) on a window=True index against what an index without it makes a user do — a new
RetrievalIndex over np.delete(pool, rows) — for m in {1, 64, 4096}, with the ring's head at 0 and wrapped (the deleted rows are
appended again between rounds, untimed, so every round sees the same row count); (iii) replayed score() of one scorer at B in
{1, 16, 256} immediately after a deletion of 4096 rows against immediately before it.  --delete --trace runs the deletions of (i)
alone, a few per point, for a kernel trace taken in a run of its own: (ii), the device time of the delete launches.
--find — the pool addressed by key instead (profiles/online/find_bench.txt), same geometry, clock and alternation, with the ring's head
at 0 and wrapped: (i) OnlineScorer.find / RetrievalIndex.find of M in {1, 64, 4096} keys on one and on three columns against
np.flatnonzero over a host copy of the pool (what a caller has to keep without it), and the device time of the three launches alone;
(ii) relabel_where of one key against the only route there was, delete plus append of the corrected row; (iii) replayed score() at B in
{1, 16, 256} immediately after a relabel_where against immediately before it, the same captured request.
--requests — requests that share a launch instead (profiles/online/requests_bench.txt), the immutable 1.4 M-row pool: (i) R in
{1, 4, 16, 64, 256} single-row requests as ONE OnlineScorer.score_requests call against R consecutive replayed score() calls on the same
scorer (each side issues its launches and synchronises once at the end of the R requests); (ii) score_requests with one request of B
rows against score() of the same B at B in {1, 16, 256}: what the segment array and the padding cost.  Same clock and alternation.
--rows — the pool that looks at itself instead (profiles/online/rows_bench.txt), same geometry: (i) the scan alone, device time per call
as in part 1 (hipGraphs of REPS calls, device events, the sides alternating): rat_bm25_topk_split_before with before = n for every
query — the horizon excludes nothing, so the same rows are scored and the same lists come out — against the plain scan of the same
pool form (immutable, capacity, window with the ring wrapped) at Q in {1, 16, 256}: what the compare and select per (row, query)
cost; (ii) replayed score_rows(B indices) against replayed score(the same rows' ids) at B in {1, 16, 256}, host clock + synchronise,
rounds of 200 alternating: what the gather and the horizon cost a request.
--same — neighbours restricted to rows equal on given columns instead (profiles/online/same_bench.txt), same geometry, same = the user
column: (i) device time per call of the chain rat_bm25_exact_count -> rat_bm25_exact_plan -> rat_bm25_topk_split_exact against the plain
split scan of the same pool form (immutable, capacity, window with the ring wrapped) at Q in {1, 16, 256}, splits = 0 on both sides,
measured as in --rows (i); the chain's result is compared bit for bit with the offline path (BM25_topk_retrieval_v4 with
exact_match_col_indices) before anything is timed; (ii) replayed score(ids, same=) against replayed score(ids) at B in {1, 16, 256},
host clock + synchronise, rounds of 200 alternating.
--top — each request's best candidates instead (profiles/online/top_bench.txt), same geometry, the immutable pool, requests of one user
row and C_r candidate items (the candidates differ in the item column), n = 10, on the grid R in {1, 16, 64} requests x C_r in {64, 256,
1024} candidates within graph_max_batch: (i) device time per call of rat_topn_seg alone (a hipGraph of REPS calls, device events)
and of the replayed top_candidates chain (its captured graph, device events), and the kernel's share; (ii) a replayed top_candidates call
plus reading pos, y and lens back against the way without it — the rows expanded on the host, uploaded, a replayed score_requests, all
predictions read back and a numpy stable top-n per request — host clock + synchronise, the sides alternating round by round, results
compared before anything is timed; (iii) the bytes both ways move per call, derived from the shapes.
--rank — each request's full ranking instead (profiles/online/rank_bench.txt), same geometry and grid plus one request of 4096 rows:
(i) device time per call of rat_rank_seg alone, with rat_topn_seg at n = 64 beside it (hipGraphs of REPS calls, device events, the two
alternating), against the replayed rank_requests chain; (ii) a replayed rank_requests call — once with order, val and rank read back, once
with the ranking left on the device — against the host way: replayed score_requests, every prediction read back, one
np.argsort(-y_r, kind="stable") per request — host clock + synchronise, the sides alternating round by round, results compared before
anything is timed; (iii) the bytes the ways move per call, derived from the shapes.
--catalogue — the best n of a whole resident item catalogue instead (profiles/online/catalogue_bench.txt), same geometry, the immutable
pool, R in {1, 16} users against all M in {4096, 65536} items (the items differ in the item column), n = 10, chunk = graph_max_batch // R:
(i) a top_catalogue call plus reading items, y and lens back against the host loop — per chunk the rows expanded on the host, uploaded, a
replayed score_requests, all predictions read back, a numpy merge — host clock + synchronise, one call per round, the sides alternating,
results compared before anything is timed; (ii) the bytes both ways move per call, derived from the shapes.
--catalogue --postings — additionally (profiles/online/postings_bench.txt) a third side, top_catalogue(postings=True), in the same rounds
and compared bit for bit: (iii) the call against the other two, with build_postings() timed once; (iv) the parts of one 4096-row pass
alone — the scan per row, the chain through the posting lists, the assembly and eval forward — as hipGraphs under device events.
There is no CPU fallback: without a GPU the tool exits with an error."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "www24-rat_amd")):
    sys.path.insert(0, p)

REPS = 20
MIN_TIMED_MS = 500.0
SWEEP = (2, 8, 32, 64, 128, 256, 512)


def _graph_of(fn, reps):
    g = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        for _ in range(reps):
            out = fn()
    return g, out


def time_alternating(graphs, reps, min_ms):
    """graphs: {label: CUDAGraph of `reps` calls} -> {label: ms per call}; round-robin replays until every label has min_ms"""
    for g in graphs.values():
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    total = {k: 0.0 for k in graphs}
    count = {k: 0 for k in graphs}
    while min(total.values()) < min_ms:
        pending = []
        for k, g in graphs.items():
            if total[k] >= min_ms and count[k] >= 3:
                continue
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            pending.append((k, s, e))
        torch.cuda.synchronize()
        for k, s, e in pending:
            total[k] += s.elapsed_time(e)
            count[k] += 1
    return {k: total[k] / (count[k] * reps) for k in graphs}


def part1(emit, quick):
    import ctypes
    from rat_amd import ops, retrieval
    from rat_amd._lib import get_lib
    lib = get_lib()
    dev = torch.device("cuda:0")
    K = 5
    emit("== part 1: device time per call [us], K = %d; split(s) = rat_bm25_topk_split with s ranges, split(0) = the library's choice" % K)
    worst_auto = 0.0
    for n_db in ((100_000,) if quick else (100_000, 1_400_000)):
        for F in (3, 13):
            rs = np.random.RandomState(F)
            vocab = ([17_000, 23_000, 49_000, 300, 40, 12] + [1000] * 7)[:F]
            db = np.stack([rs.randint(0, v, size=n_db) for v in vocab], axis=1).astype(np.int64)
            tables = retrieval.idf_tables(db)
            db_t = torch.from_numpy(np.ascontiguousarray(db.astype(np.int32).T)).to(dev)
            for Q in ((4, 256) if quick else (1, 4, 16, 64, 256, 4096)):
                qry = np.stack([rs.randint(0, v, size=Q) for v in vocab], axis=1).astype(np.int64)
                q_ids = torch.from_numpy(qry.astype(np.int32)).to(dev)
                q_idf = torch.from_numpy(retrieval.map_data_to_idf(qry, tables)).to(dev)
                out = (torch.empty((Q, K), dtype=torch.float64, device=dev), torch.empty((Q, K), dtype=torch.int64, device=dev),
                       torch.empty((Q,), dtype=torch.int64, device=dev))

                def parent():
                    lib.call("rat_bm25_topk", *[ctypes.c_void_p(t.data_ptr()) for t in (db_t, q_ids, q_idf) + out], n_db, Q, F, K,
                             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
                    return out
                tiles = (Q + 3) // 4
                variants = {"rat_bm25_topk": parent, "split(0)": lambda: ops.bm25_topk_split(db_t, q_ids, q_idf, K, splits=0, lib=lib)}
                for s in SWEEP:
                    if tiles * s <= 16384 and n_db // s >= 256:
                        variants["split(%d)" % s] = (lambda s=s: ops.bm25_topk_split(db_t, q_ids, q_idf, K, splits=s, lib=lib))
                want = tuple(t.clone() for t in parent())
                torch.cuda.synchronize()
                graphs = {}
                for label, fn in variants.items():
                    got = fn()
                    torch.cuda.synchronize()
                    for g, w in zip(got, want):
                        assert torch.equal(g.view(torch.int64), w.view(torch.int64)), (n_db, F, Q, label)
                    graphs[label], _ = _graph_of(fn, REPS)
                ms = time_alternating(graphs, REPS, 50.0 if quick else MIN_TIMED_MS)
                base = ms["rat_bm25_topk"]
                ratio = ms["split(0)"] / base
                worst_auto = max(worst_auto, ratio)
                emit("N %8d  F %2d  Q %4d | %s | split(0) / rat_bm25_topk = %.3f (speed-up %.1fx)" %
                     (n_db, F, Q, "  ".join("%s %.1f" % (k, v * 1e3) for k, v in ms.items()), ratio, base / ms["split(0)"]))
                del graphs
    emit("worst split(0) / rat_bm25_topk over the table: %.3f (the requirement: <= 1.02)" % worst_auto)


def part2(emit, quick):
    from rat_amd import synthetic
    from rat_amd.model import RAT_m2
    from rat_amd.online import OnlineScorer
    name = "movielens_real_F3_K5_d10_B4096"
    spec = synthetic.WORKLOADS[name]
    fm = synthetic.feature_map_for(name, spec)
    model = RAT_m2(fm, **synthetic.model_kwargs(spec, gpu=0))
    model.eval()
    n_pool = 100_000 if quick else 1_400_000
    rs = np.random.RandomState(3)
    vocab = [s["vocab_size"] for s in fm.feature_specs.values()]
    pool = np.concatenate([np.stack([rs.randint(0, v, size=n_pool) for v in vocab], axis=1), rs.randint(0, 2, size=(n_pool, 1))], axis=1)
    cfg = dict(topK=spec["K"], used_col_indices=list(range(spec["F"])), label_wise=False)
    emit("== part 2: OnlineScorer.score() latency [us per request], %s, %d-row pool, host clock + synchronise" % (name, n_pool))
    for B in (1, 16, 256):
        ids = torch.from_numpy(np.stack([rs.randint(0, v, size=B) for v in vocab], axis=1).astype(np.int32)).to("cuda:0")
        res = {}
        for label, graph in (("eager", False), ("replayed", True)):
            scorer = OnlineScorer(model, pool, cfg, graph=graph)
            for _ in range(5):
                y = scorer.score(ids)
            torch.cuda.synchronize()
            if graph:
                assert any(e[1] for e in scorer._graphs.values()), "the request was not captured"
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < (0.1 if quick else 0.5):
                y = scorer.score(ids)
                torch.cuda.synchronize()
                n += 1
            res[label] = ((time.perf_counter() - t0) / n * 1e6, y)
            del scorer
        assert torch.equal(res["eager"][1], res["replayed"][1])
        emit("B %4d | eager %.1f  replayed %.1f" % (B, res["eager"][0], res["replayed"][0]))


def _movielens(quick):
    from rat_amd import synthetic
    from rat_amd.model import RAT_m2
    name = "movielens_real_F3_K5_d10_B4096"
    spec = synthetic.WORKLOADS[name]
    fm = synthetic.feature_map_for(name, spec)
    model = RAT_m2(fm, **synthetic.model_kwargs(spec, gpu=0))
    model.eval()
    n_pool, capacity = (100_000, 150_000) if quick else (1_400_000, 2_000_000)
    rs = np.random.RandomState(3)
    vocab = [s["vocab_size"] for s in fm.feature_specs.values()]

    def rows(n):
        return np.concatenate([np.stack([rs.randint(0, v, size=n) for v in vocab], axis=1), rs.randint(0, 2, size=(n, 1))], axis=1)
    cfg = dict(topK=spec["K"], used_col_indices=list(range(spec["F"])), label_wise=False)
    return name, model, rows, vocab, cfg, n_pool, capacity


def _stats(xs):
    return "%.1f (%.1f .. %.1f, %d rounds)" % (sum(xs) / len(xs), min(xs), max(xs), len(xs))


def part_append(emit, quick):
    from rat_amd.online import OnlineScorer, RetrievalIndex
    name, model, rows, vocab, cfg, n_pool, capacity = _movielens(quick)
    dev, K, cols = torch.device("cuda:0"), cfg["topK"], cfg["used_col_indices"]
    min_s = 0.05 if quick else MIN_TIMED_MS / 1e3
    pool = rows(n_pool)
    emit("== append (i): taking M labelled rows into a %d-row pool (%s columns), capacity %d [ms per call]: RetrievalIndex.append "
         "against a new RetrievalIndex over np.concatenate([pool, rows]) (concatenate included); host clock + synchronise, alternating"
         % (n_pool, len(cols), capacity))
    index = RetrievalIndex(pool, cols, K, dev, capacity=capacity)
    cur = pool
    for M in (1, 64, 4096):
        t_app, t_new = [], []
        while sum(t_app) < min_s or sum(t_new) < min_s or len(t_app) < 3 or len(t_new) < 3:
            new = rows(M)
            appended = (sum(t_app) < min_s or len(t_app) < 3) and len(index) + M <= capacity
            if appended:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                index.append(new)
                torch.cuda.synchronize()
                t_app.append((time.perf_counter() - t0) * 1e3)
            if sum(t_new) < min_s or len(t_new) < 3:     # the same rows into the same pool, the immutable way
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fresh = RetrievalIndex(np.concatenate([cur, new]), cols, K, dev)
                torch.cuda.synchronize()
                t_new.append((time.perf_counter() - t0) * 1e3)
                del fresh
            elif not appended:
                break
            if appended:
                cur = np.concatenate([cur, new])
        a, b = sum(t_app) / len(t_app), sum(t_new) / len(t_new)
        emit("M %5d | append %s | new index %s | append / new index = %.5f (%.0fx)" % (M, _stats(t_app), _stats(t_new), a / b, b / a))
    # the appended index still answers like a fresh one over the same rows
    ids = torch.from_numpy(np.stack([np.random.RandomState(9).randint(0, v, size=16) for v in vocab], axis=1).astype(np.int32)).to(dev)
    fresh = RetrievalIndex(cur, cols, K, dev)
    for g, w in zip(index.retrieve(ids), fresh.retrieve(ids)):
        assert torch.equal(g.view(torch.int64), w.view(torch.int64)), "appended index != fresh index"
    emit("   (after %d appended rows retrieve() equals a fresh index over the same rows, bit for bit)" % (len(index) - n_pool))
    del index, fresh

    emit("== append (ii): replayed OnlineScorer.score() [us per request], %s, %d-row pool: capacity = %d against the immutable scorer; "
         "host clock + synchronise, rounds of %d requests alternating" % (name, n_pool, capacity, 200))
    grow = OnlineScorer(model, pool, cfg, graph=True, capacity=capacity)
    fixed = OnlineScorer(model, pool, cfg, graph=True)
    rs = np.random.RandomState(5)
    for B in (1, 16, 256):
        ids = torch.from_numpy(np.stack([rs.randint(0, v, size=B) for v in vocab], axis=1).astype(np.int32)).to(dev)
        for sc in (grow, fixed):
            for _ in range(5):
                y = sc.score(ids)
            torch.cuda.synchronize()
            assert any(e[1] for e in sc._graphs.values()), "the request was not captured"
        assert torch.equal(grow.score(ids), fixed.score(ids))
        per = {"capacity": [], "immutable": []}
        while min(sum(v) for v in per.values()) * 200 / 1e6 < min_s:
            for label, sc in (("capacity", grow), ("immutable", fixed)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(200):
                    sc.score(ids)
                    torch.cuda.synchronize()
                per[label].append((time.perf_counter() - t0) / 200 * 1e6)
        a, b = (sum(per[k]) / len(per[k]) for k in ("capacity", "immutable"))
        emit("B %4d | capacity %s | immutable %s | capacity / immutable = %.4f" % (B, _stats(per["capacity"]), _stats(per["immutable"]), a / b))


def _replay_round(sc, ids, rounds_of=200):
    """us per request over one round of `rounds_of` requests, each followed by a synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds_of):
        sc.score(ids)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / rounds_of * 1e6


def _replay_rounds(sides, ids, min_s, rounds_of=200):
    """sides: {label: scorer with the request captured} -> {label: [us per request of every round]}, the sides alternating"""
    per = {k: [] for k in sides}
    while min(sum(v) for v in per.values()) * rounds_of / 1e6 < min_s:
        for label, sc in sides.items():
            per[label].append(_replay_round(sc, ids, rounds_of))
    return per


def part_window(emit, quick):
    from rat_amd.online import OnlineScorer, RetrievalIndex
    name, model, rows, vocab, cfg, n_pool, capacity = _movielens(quick)
    dev, K, cols = torch.device("cuda:0"), cfg["topK"], cfg["used_col_indices"]
    min_s = 0.05 if quick else MIN_TIMED_MS / 1e3
    pool = rows(n_pool)
    rs = np.random.RandomState(5)
    requests = {B: torch.from_numpy(np.stack([rs.randint(0, v, size=B) for v in vocab], axis=1).astype(np.int32)).to(dev)
                for B in (1, 16, 256)}
    emit("== window (i): replayed OnlineScorer.score() [us per request], %s, %d live rows in a capacity of %d: window=True against the "
         "capacity-mode scorer over the same rows; host clock + synchronise, rounds of 200 requests alternating" % (name, n_pool, capacity))
    ring = OnlineScorer(model, pool, cfg, graph=True, capacity=capacity, window=True)
    push = capacity - n_pool + n_pool // 2                                 # afterwards half of the live rows lie before the wrap
    for state in ("head = 0", "wrapped"):
        if state == "wrapped":
            cur = pool
            while push > 0:                                                # the window fills, then slides: n stays at the capacity
                new = rows(min(push, 200_000))
                ring.append(new)
                cur = np.concatenate([cur, new])[-capacity:]
                push -= len(new)
            ring.evict(capacity - n_pool)                                  # ... and back to n_pool live rows, as before
            cur = cur[capacity - n_pool:]
            n, head = ring.index.count.cpu().tolist()
            assert n == n_pool and head + n > capacity, (n, head)
            emit("   after the pushes: n = %d, head = %d — %d live rows before the wrap, %d after it" % (n, head, capacity - head,
                                                                                                      n - (capacity - head)))
        else:
            cur = pool
        flat = OnlineScorer(model, cur, cfg, graph=True, capacity=capacity)
        for B, ids in requests.items():
            for sc in (ring, flat):
                for _ in range(5):
                    sc.score(ids)
                torch.cuda.synchronize()
                assert any(e[1] for e in sc._graphs.values()), "the request was not captured"
            assert torch.equal(ring.score(ids), flat.score(ids)), "window scorer != capacity scorer over the same rows"
            per = _replay_rounds({"window": ring, "capacity": flat}, ids, min_s)
            a, b = (sum(per[k]) / len(per[k]) for k in ("window", "capacity"))
            emit("%-8s B %4d | window %s | capacity %s | window / capacity = %.4f" % (state, B, _stats(per["window"]),
                                                                                     _stats(per["capacity"]), a / b))
        del flat
    del ring

    emit("== window (ii): taking M labelled rows into a FULL window of %d rows (%d columns) [ms per call]: RetrievalIndex.append (the M "
         "oldest rows leave) against a new RetrievalIndex over np.concatenate([pool[M:], rows]) (concatenate included); host clock + "
         "synchronise, alternating" % (n_pool, len(cols)))
    index = RetrievalIndex(pool, cols, K, dev, capacity=n_pool, window=True)
    cur = pool
    for M in (1, 64, 4096):
        t_app, t_new = [], []
        while sum(t_app) < min_s or sum(t_new) < min_s or len(t_app) < 3 or len(t_new) < 3:
            new = rows(M)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index.append(new)
            torch.cuda.synchronize()
            t_app.append((time.perf_counter() - t0) * 1e3)
            if sum(t_new) < min_s or len(t_new) < 3:     # the same rows into the same pool, the immutable way
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fresh = RetrievalIndex(np.concatenate([cur[M:], new]), cols, K, dev)
                torch.cuda.synchronize()
                t_new.append((time.perf_counter() - t0) * 1e3)
                del fresh
            cur = np.concatenate([cur[M:], new])
        a, b = sum(t_app) / len(t_app), sum(t_new) / len(t_new)
        emit("M %5d | append %s | new index %s | append / new index = %.5f (%.0fx)" % (M, _stats(t_app), _stats(t_new), a / b, b / a))
    fresh = RetrievalIndex(cur, cols, K, dev)
    for g, w in zip(index.retrieve(requests[16]), fresh.retrieve(requests[16])):
        assert torch.equal(g.view(torch.int64), w.view(torch.int64)), "window index != fresh index"
    emit("   (afterwards retrieve() equals a fresh index over the live rows, bit for bit; head = %d)" % index.count.cpu().tolist()[1])


def _wrap(obj, rows, cur, n_pool, capacity):
    """obj holds the n_pool rows `cur` from slot 0 on: push until half of the live rows lie before the wrap, then evict back to n_pool
    rows -> the live rows, oldest first"""
    push = capacity - n_pool + n_pool // 2
    while push > 0:
        new = rows(min(push, 200_000))
        obj.append(new)
        cur = np.concatenate([cur, new])[-capacity:]
        push -= len(new)
    obj.evict(capacity - n_pool)
    return cur[capacity - n_pool:]


def part_delete(emit, quick, trace):
    from rat_amd.online import OnlineScorer, RetrievalIndex
    name, model, rows, vocab, cfg, n_pool, capacity = _movielens(quick)
    dev, K, cols = torch.device("cuda:0"), cfg["topK"], cfg["used_col_indices"]
    min_ms = 50.0 if quick else MIN_TIMED_MS                               # of timed work per point and side
    min_s = min_ms / 1e3
    pool = rows(n_pool)
    rs = np.random.RandomState(5)
    requests = {B: torch.from_numpy(np.stack([rs.randint(0, v, size=B) for v in vocab], axis=1).astype(np.int32)).to(dev)
                for B in (1, 16, 256)}
    emit("== delete (i): m seeded random rows leave a window of %d live rows (%d columns) in a capacity of %d [ms per call]: "
         "RetrievalIndex.delete against a new RetrievalIndex over np.delete(pool, rows) (np.delete included); host clock + synchronise, "
         "alternating; the deleted rows are appended again between rounds, untimed" % (n_pool, len(cols), capacity))
    index = RetrievalIndex(pool, cols, K, dev, capacity=capacity, window=True)
    cur = pool
    for state in ("head = 0", "wrapped"):
        if state == "wrapped":
            cur = _wrap(index, rows, cur, n_pool, capacity)
            n, head = index.count.cpu().tolist()
            assert n == n_pool and head + n > capacity, (n, head)
            emit("   after the pushes: n = %d, head = %d — %d live rows before the wrap, %d after it" % (n, head, capacity - head,
                                                                                                      n - (capacity - head)))
        for m in (1, 64, 4096):
            t_del, t_new = [], []
            while len(t_del) < 5 if trace else (sum(t_del) < min_ms or len(t_del) < 3 or sum(t_new) < min_ms or len(t_new) < 3):
                idx = rs.choice(len(index), m, replace=False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                index.delete(idx)
                torch.cuda.synchronize()
                t_del.append((time.perf_counter() - t0) * 1e3)
                if not trace and (sum(t_new) < min_ms or len(t_new) < 3):    # the same rows out of the same pool, the immutable way
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fresh = RetrievalIndex(np.delete(cur, idx, axis=0), cols, K, dev)
                    torch.cuda.synchronize()
                    t_new.append((time.perf_counter() - t0) * 1e3)
                    del fresh
                new = rows(m)
                index.append(new)                              # back to n_pool rows: there is room, nobody leaves
                cur = np.concatenate([np.delete(cur, idx, axis=0), new])
            if trace:
                emit("%-8s m %5d | delete %s" % (state, m, _stats(t_del)))
                continue
            a, b = sum(t_del) / len(t_del), sum(t_new) / len(t_new)
            emit("%-8s m %5d | delete %s | new index %s | delete / new index = %.5f (%.1fx)" % (state, m, _stats(t_del), _stats(t_new),
                                                                                                a / b, b / a))
    fresh = RetrievalIndex(cur, cols, K, dev)
    for g, w in zip(index.retrieve(requests[16]), fresh.retrieve(requests[16])):
        assert torch.equal(g.view(torch.int64), w.view(torch.int64)), "index after deletions != fresh index"
    emit("   (afterwards retrieve() equals a fresh index over the live rows, bit for bit; n, head = %s)" % index.count.cpu().tolist())
    del index, fresh
    if trace:
        return

    m = 4096
    emit("== delete (iii): replayed OnlineScorer.score() [us per request], %s, window=True, %d live rows in a capacity of %d: immediately "
         "after delete(%d random rows) against immediately before it, the same scorer and the same captured request; host clock + "
         "synchronise, rounds of 200 requests, before and after alternating (the rows are appended again after every round)"
         % (name, n_pool, capacity, m))
    scorer = OnlineScorer(model, pool, cfg, graph=True, capacity=capacity, window=True)
    cur = pool
    for B, ids in requests.items():
        for _ in range(5):
            scorer.score(ids)
        torch.cuda.synchronize()
    assert all(e[1] for e in scorer._graphs.values()) and len(scorer._graphs) == 3, "the requests were not captured"
    for B, ids in requests.items():
        per = {"before": [], "after": []}
        while min(sum(v) for v in per.values()) * 200 / 1e6 < min_s:
            per["before"].append(_replay_round(scorer, ids))
            idx = rs.choice(len(scorer.index), m, replace=False)
            scorer.delete(idx)
            per["after"].append(_replay_round(scorer, ids))
            new = rows(m)
            scorer.append(new)
            cur = np.concatenate([np.delete(cur, idx, axis=0), new])
        a, b = (sum(per[k]) / len(per[k]) for k in ("after", "before"))
        emit("B %4d | after %s | before %s | after / before = %.4f" % (B, _stats(per["after"]), _stats(per["before"]), a / b))
    assert len(scorer._graphs) == 3 and all(e[1] for e in scorer._graphs.values()), "a deletion invalidated a captured request"
    idx = rs.choice(len(scorer.index), m, replace=False)
    scorer.delete(idx)
    fresh = OnlineScorer(model, np.delete(cur, idx, axis=0), cfg, graph=False)
    assert torch.equal(scorer.score(requests[16]), fresh.score(requests[16])), "replay after a deletion != fresh scorer"
    emit("   (the replayed request after the last deletion equals a fresh scorer over the remaining rows, bit for bit; %d graphs kept)"
         % len(scorer._graphs))


def _host_find(host, cols, keys):
    """np.flatnonzero over a host copy of the pool's ids: np.isin on the first column, then whole key tuples on its candidates"""
    cand = np.flatnonzero(np.isin(host[:, cols[0]], keys[:, 0]))
    if len(cols) == 1:
        return cand
    void = np.dtype((np.void, 4 * len(cols)))
    rows = np.ascontiguousarray(host[cand][:, cols]).view(void).ravel()
    return cand[np.isin(rows, np.ascontiguousarray(keys).view(void).ravel())]


def part_find(emit, quick):
    from rat_amd import ops
    from rat_amd.online import OnlineScorer
    name, model, rows, vocab, cfg, n_pool, capacity = _movielens(quick)
    dev, cols = torch.device("cuda:0"), cfg["used_col_indices"]
    min_ms = 50.0 if quick else MIN_TIMED_MS                               # of timed work per point and side
    pool = rows(n_pool)
    rs = np.random.RandomState(5)
    requests = {B: torch.from_numpy(np.stack([rs.randint(0, v, size=B) for v in vocab], axis=1).astype(np.int32)).to(dev)
                for B in (1, 16, 256)}
    scorer = OnlineScorer(model, pool, cfg, graph=True, capacity=capacity, window=True)
    cur = pool
    for B, ids in requests.items():
        for _ in range(5):
            scorer.score(ids)
        torch.cuda.synchronize()
    assert all(e[1] for e in scorer._graphs.values()) and len(scorer._graphs) == 3, "the requests were not captured"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for state in ("head = 0", "wrapped"):
        if state == "wrapped":
            cur = _wrap(scorer, rows, cur, n_pool, capacity)
            n, head = scorer.index.count.cpu().tolist()
            assert n == n_pool and head + n > capacity, (n, head)
            emit("   after the pushes: n = %d, head = %d — %d live rows before the wrap, %d after it" % (n, head, capacity - head,
                                                                                                      n - (capacity - head)))
        host = np.ascontiguousarray(cur[:, :-1].astype(np.int32))          # the copy a caller keeps without find
        emit("== find (i), %s: M keys (taken from live rows) on C columns over %d live rows (%d id columns) in a capacity of %d: "
             "OnlineScorer.find (pool_ids) and RetrievalIndex.find (db_t) [ms per call, host clock + synchronise, the count read back "
             "included] against np.flatnonzero over a host copy of the ids, alternating; then the device time of the three launches "
             "alone [us per call, a hipGraph of %d calls, device events]" % (state, n_pool, host.shape[1], capacity, REPS))
        for C in (1, 3):
            cc = cols[:C]
            for M in (1, 64, 4096):
                keys = host[rs.choice(n_pool, M, replace=False)][:, cc].astype(np.int64)
                want = _host_find(host, cc, keys.astype(np.int32))
                for obj in (scorer, scorer.index):
                    assert np.array_equal(obj.find(cc, keys).cpu().numpy(), want), (state, C, M)
                per = {"OnlineScorer.find": [], "RetrievalIndex.find": [], "numpy": []}
                while min(sum(v) for v in per.values()) < min_ms or min(len(v) for v in per.values()) < 3:
                    per["OnlineScorer.find"].append(timed(lambda: scorer.find(cc, keys))[0])
                    per["RetrievalIndex.find"].append(timed(lambda: scorer.index.find(cc, keys))[0])
                    per["numpy"].append(timed(lambda: _host_find(host, cc, keys.astype(np.int32)))[0])
                table = torch.from_numpy(np.unique(keys.astype(np.int32), axis=0)).to(dev)
                pos = torch.from_numpy(np.arange(C, dtype=np.int32)).to(dev)
                form = scorer.index._pool_form()
                out = (torch.empty(capacity, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int64, device=dev))
                graphs = {"pool_ids": _graph_of(lambda: ops.pool_find(scorer.pool_ids, pos, table, False, out_idx=out[0], out_count=out[1],
                                                                      max_out=n_pool, **form), REPS)[0],
                          "db_t": _graph_of(lambda: ops.pool_find(scorer.index.db_t, pos, table, True, out_idx=out[0], out_count=out[1],
                                                                  max_out=n_pool, **form), REPS)[0]}
                dev_ms = time_alternating(graphs, REPS, min_ms / 5)
                a, b, c = (sum(per[k]) / len(per[k]) for k in ("OnlineScorer.find", "RetrievalIndex.find", "numpy"))
                emit("%-8s C %d M %5d  %6d matches | OnlineScorer.find %s | RetrievalIndex.find %s | numpy %s | numpy / find = %.1fx, %.1fx "
                     "| device: pool_ids %.1f us, db_t %.1f us" % (state, C, M, len(want), _stats(per["OnlineScorer.find"]),
                                                                  _stats(per["RetrievalIndex.find"]), _stats(per["numpy"]), c / a, c / b,
                                                                  dev_ms["pool_ids"] * 1e3, dev_ms["db_t"] * 1e3))
                del graphs

        emit("== find (ii), %s: one row's label is corrected [ms per call]: relabel_where of its key (all %d id columns) against delete of "
             "the row (its position known) plus append of the corrected row; host clock + synchronise, alternating" % (state, host.shape[1]))
        per = {"relabel_where": [], "delete + append": []}
        all_cols = list(range(host.shape[1]))
        scorer.relabel_where(all_cols, np.full((1, host.shape[1]), -1), 0.0)       # nobody holds it: allocates the index list, untimed
        while min(sum(v) for v in per.values()) < min_ms or min(len(v) for v in per.values()) < 3:
            i = int(rs.randint(0, len(cur)))
            key = cur[i:i + 1, :-1].astype(np.int64)
            per["relabel_where"].append(timed(lambda: scorer.relabel_where(all_cols, key, 1.0 - cur[i, -1]))[0])
            cur[_host_find(host, all_cols, key.astype(np.int32)), -1] = 1.0 - cur[i, -1]
            j = int(rs.randint(0, len(cur)))
            row = cur[j:j + 1].copy()
            row[0, -1] = 1.0 - row[0, -1]

            def old_route():
                scorer.delete([j])
                scorer.append(row)
            per["delete + append"].append(timed(old_route)[0])
            cur = np.concatenate([np.delete(cur, [j], axis=0), row])
            host = np.ascontiguousarray(cur[:, :-1].astype(np.int32))
        a, b = (sum(per[k]) / len(per[k]) for k in ("relabel_where", "delete + append"))
        emit("%-8s | relabel_where %s | delete + append %s | delete + append / relabel_where = %.1fx" %
             (state, _stats(per["relabel_where"]), _stats(per["delete + append"]), b / a))

        emit("== find (iii), %s: replayed OnlineScorer.score() [us per request], %s: immediately after relabel_where(one key) against "
             "immediately before it, the same scorer and the same captured request; host clock + synchronise, rounds of 200 requests, "
             "before and after alternating" % (state, name))
        for B, ids in requests.items():
            per = {"before": [], "after": []}
            while min(sum(v) for v in per.values()) * 200 / 1e3 < min_ms:
                per["before"].append(_replay_round(scorer, ids))
                i = int(rs.randint(0, len(cur)))
                key = cur[i:i + 1, :-1].astype(np.int64)
                scorer.relabel_where(all_cols, key, 1.0 - cur[i, -1])
                cur[_host_find(host, all_cols, key.astype(np.int32)), -1] = 1.0 - cur[i, -1]
                per["after"].append(_replay_round(scorer, ids))
            a, b = (sum(per[k]) / len(per[k]) for k in ("after", "before"))
            emit("%-8s B %4d | after %s | before %s | after / before = %.4f" % (state, B, _stats(per["after"]), _stats(per["before"]), a / b))
        assert len(scorer._graphs) == 3 and all(e[1] for e in scorer._graphs.values()), "a relabel invalidated a captured request"
    fresh = OnlineScorer(model, cur, cfg, graph=False)
    assert torch.equal(scorer.score(requests[16]), fresh.score(requests[16])), "replay after the relabels != fresh scorer"
    emit("   (the replayed request after the last relabel equals a fresh scorer over the modelled rows and labels, bit for bit; %d graphs kept)"
         % len(scorer._graphs))


def part_requests(emit, quick):
    from rat_amd.online import OnlineScorer
    name, model, rows, vocab, cfg, n_pool, _capacity = _movielens(quick)
    dev = torch.device("cuda:0")
    min_s = 0.05 if quick else MIN_TIMED_MS / 1e3
    pool = rows(n_pool)
    rs = np.random.RandomState(5)
    scorer = OnlineScorer(model, pool, cfg, graph=True)

    def request_rows(B):
        return torch.from_numpy(np.stack([rs.randint(0, v, size=B) for v in vocab], axis=1).astype(np.int32)).to(dev)

    def rounds(sides, calls):
        """sides: {label: fn} -> {label: [us per call of every round]}; a round is `calls` calls, each followed by a synchronise"""
        per = {k: [] for k in sides}
        while min(sum(v) for v in per.values()) * calls / 1e6 < min_s or min(len(v) for v in per.values()) < 3:
            for label, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                    torch.cuda.synchronize()
                per[label].append((time.perf_counter() - t0) / calls * 1e6)
        return per

    emit("== requests (i): R single-row requests [us for all R], %s, %d-row pool: ONE score_requests call (ids on the device, offsets on the "
         "host) against R consecutive replayed score() calls on the same scorer; host clock, one synchronise after the R requests, the "
         "sides alternating round by round" % (name, n_pool))
    for R in (1, 4, 16, 64, 256):
        ids = request_rows(R)
        singles = [ids[r:r + 1].contiguous() for r in range(R)]
        off = np.arange(R + 1, dtype=np.int64)
        for _ in range(5):
            y, _ = scorer.score_requests((ids, off))
            y_alone = torch.cat([scorer.score(x) for x in singles])
        torch.cuda.synchronize()
        assert all(e[1] for e in scorer._bucket_graphs.values()) and all(e[1] for e in scorer._graphs.values()), "not captured"
        worst = float((y - y_alone).abs().max())

        def alone():
            for x in singles:
                scorer.score(x)
        per = rounds({"score_requests": lambda: scorer.score_requests((ids, off)), "score": alone}, max(2, 256 // R))
        a, b = (sum(per[k]) / len(per[k]) for k in ("score_requests", "score"))
        emit("R %4d | score_requests %s | R x score %s | R x score / score_requests = %.2fx | worst |dy| %.1e, bit-equal: %s"
             % (R, _stats(per["score_requests"]), _stats(per["score"]), b / a, worst, torch.equal(y, y_alone)))

    emit("== requests (ii): ONE request of B rows [us per request]: score_requests (segment array, padding to the bucket) against replayed "
         "score() of the same B; host clock + synchronise, rounds of 200 requests alternating")
    for B in (1, 16, 256):
        ids = request_rows(B)
        off = np.array([0, B], dtype=np.int64)
        for _ in range(5):
            y, _ = scorer.score_requests((ids, off))
            y_plain = scorer.score(ids)
        torch.cuda.synchronize()
        assert torch.equal(y, y_plain), "one request through score_requests != score()"
        per = rounds({"score_requests": lambda: scorer.score_requests((ids, off)), "score": lambda: scorer.score(ids)}, 200)
        a, b = (sum(per[k]) / len(per[k]) for k in ("score_requests", "score"))
        lo, hi = min(per["score"]), max(per["score"])
        emit("B %4d | score_requests %s | score %s | score_requests / score = %.4f | inside score()'s min .. max: %s"
             % (B, _stats(per["score_requests"]), _stats(per["score"]), a / b, lo <= a <= hi))
    emit("   (%d bucket graphs, %d score() graphs)" % (len(scorer._bucket_graphs), len(scorer._graphs)))


def part_rows(emit, quick):
    from rat_amd import ops
    from rat_amd.online import OnlineScorer, RetrievalIndex
    name, model, rows, vocab, cfg, n_pool, capacity = _movielens(quick)
    dev, K, cols = torch.device("cuda:0"), cfg["topK"], cfg["used_col_indices"]
    min_s = 0.05 if quick else MIN_TIMED_MS / 1e3
    pool = rows(n_pool)
    rs = np.random.RandomState(13)
    emit("== rows (i): the scan alone [us per call, device time], %d-row pool (%d columns), K = %d: rat_bm25_topk_split_before with before = n "
         "for every query against the plain split scan of the same pool form, splits = 0 on both sides; hipGraphs of %d calls, device "
         "events, alternating" % (n_pool, len(cols), K, REPS))
    wrap = n_pool // 3
    forms = (("immutable", {}, 0), ("capacity", dict(capacity=capacity), 0), ("window wrapped", dict(capacity=n_pool + wrap, window=True), 2 * wrap))
    for label, kw, pushes in forms:
        index = RetrievalIndex(pool, cols, K, dev, **kw)
        for _ in range(pushes // wrap):                                       # the window fills, then loses its oldest rows: the head moves
            index.append(rows(wrap))
        if pushes:
            assert int(index.count[1]) + len(index) > index.capacity, "the window does not wrap"
        n = len(index)
        form = index._pool_form()
        for Q in (1, 16, 256):
            ids = torch.from_numpy(np.stack([rs.randint(0, v, size=Q) for v in vocab], axis=1).astype(np.int32)).to(dev)
            q_ids, q_idf = ops.bm25_query_prepare(ids, index.cols, index.table_ids, index.table_idf, index.table_offsets)
            before = torch.full((Q,), n, dtype=torch.int64, device=dev)
            plain = lambda: ops.bm25_topk_split(index.db_t, q_ids, q_idf, K, **form)                         # noqa: E731
            horizon = lambda: ops.bm25_topk_split(index.db_t, q_ids, q_idf, K, before=before, **form)        # noqa: E731
            want, got = plain(), horizon()
            torch.cuda.synchronize()
            for g, w in zip(got, want):
                assert torch.equal(g.view(torch.int64), w.view(torch.int64)), (label, Q)
            graphs = {"plain": _graph_of(plain, REPS)[0], "before = n": _graph_of(horizon, REPS)[0]}
            ms = time_alternating(graphs, REPS, 50.0 if quick else MIN_TIMED_MS)
            emit("%-14s Q %4d | plain %.1f | before = n %.1f | before / plain = %.4f" %
                 (label, Q, ms["plain"] * 1e3, ms["before = n"] * 1e3, ms["before = n"] / ms["plain"]))
            del graphs
        del index

    emit("== rows (ii): replayed OnlineScorer.score_rows(B indices) against replayed score(the same rows' ids) [us per request], %s, "
         "immutable %d-row pool; host clock + synchronise, rounds of 200 requests alternating" % (name, n_pool))
    scorer = OnlineScorer(model, pool, cfg, graph=True)
    for B in (1, 16, 256):
        idx = torch.from_numpy(rs.choice(n_pool, size=B, replace=False).astype(np.int64)).to(dev)
        ids = scorer.pool_ids[idx].contiguous()
        for _ in range(5):
            y_rows, y_plain = scorer.score_rows(idx), scorer.score(ids)
        torch.cuda.synchronize()
        assert all(e[1] for e in scorer._rows_graphs.values()) and all(e[1] for e in scorer._graphs.values()), "not captured"
        per = {"score_rows": [], "score": []}
        while min(sum(v) for v in per.values()) * 200 / 1e6 < min_s or min(len(v) for v in per.values()) < 3:
            per["score_rows"].append(_replay_round(_RowsSide(scorer), idx))
            per["score"].append(_replay_round(scorer, ids))
        a, b = (sum(per[k]) / len(per[k]) for k in ("score_rows", "score"))
        emit("B %4d | score_rows %s | score %s | score_rows / score = %.4f | predictions differ (the row no longer sees itself): %s"
             % (B, _stats(per["score_rows"]), _stats(per["score"]), a / b, not torch.equal(y_rows, y_plain)))
    emit("   (%d score_rows graphs, %d score() graphs)" % (len(scorer._rows_graphs), len(scorer._graphs)))


def part_same(emit, quick):
    from rat_amd import ops, retrieval
    from rat_amd.online import OnlineScorer, RetrievalIndex
    name, model, rows, vocab, cfg, n_pool, capacity = _movielens(quick)
    dev, K, cols = torch.device("cuda:0"), cfg["topK"], cfg["used_col_indices"]
    min_s = 0.05 if quick else MIN_TIMED_MS / 1e3
    pool = rows(n_pool)
    rs = np.random.RandomState(17)
    same, mask = [cols[0]], 1
    emit("== same (i): the chain alone [us per call, device time], %d-row pool (%d columns), K = %d, same = column %d (%d ids): "
         "rat_bm25_exact_count -> rat_bm25_exact_plan -> rat_bm25_topk_split_exact against the plain split scan of the same pool form, "
         "splits = 0 on both sides; hipGraphs of %d calls, device events, alternating" % (n_pool, len(cols), K, cols[0], vocab[0], REPS))
    wrap = n_pool // 3
    forms = (("immutable", {}, 0), ("capacity", dict(capacity=capacity), 0), ("window wrapped", dict(capacity=n_pool + wrap, window=True), 2 * wrap))
    queries = {Q: np.stack([rs.randint(0, v, size=Q) for v in vocab], axis=1) for Q in (1, 16, 256)}

    def offline_over(live):
        return {Q: retrieval.BM25_topk_retrieval_v4(live[:, cols], q, exact_match_col_indices=[0], qry_batch_size=None, topK=K,
                                                    device="cuda:0") for Q, q in queries.items()}
    offline = offline_over(pool)
    for label, kw, pushes in forms:
        index = RetrievalIndex(pool, cols, K, dev, **kw)
        live = pool
        for _ in range(pushes // wrap):                                       # the window fills, then loses its oldest rows: the head moves
            new = rows(wrap)
            index.append(new)
            live = np.concatenate([live, new])[-index.capacity:]
        if pushes:
            assert int(index.count[1]) + len(index) > index.capacity and len(live) == len(index), "the window does not wrap"
            offline = offline_over(live)                                      # the offline path over the window's live rows, oldest first
        form = index._pool_form()
        for Q in (1, 16, 256):
            ids = torch.from_numpy(queries[Q].astype(np.int32)).to(dev)
            got = index.retrieve(ids, same=same)
            for g, w in zip(got, offline[Q]):                                 # the offline path over the same live rows: the same bits
                assert np.array_equal(g.cpu().numpy().view(np.int64), np.ascontiguousarray(w).view(np.int64)), (label, Q)
            first_row, _flag = ops.bm25_exact_plan(ops.bm25_exact_count(index.db_t, ids, index.cols, mask, **form), K)
            q_ids, q_idf = ops.bm25_query_prepare(ids, index.cols, index.table_ids, index.table_idf, index.table_offsets, first_row=first_row)
            p_ids, p_idf = ops.bm25_query_prepare(ids, index.cols, index.table_ids, index.table_idf, index.table_offsets)
            plain = lambda: ops.bm25_topk_split(index.db_t, p_ids, p_idf, K, **form)                         # noqa: E731

            def chain():
                counts = ops.bm25_exact_count(index.db_t, ids, index.cols, mask, **form)
                _first, flag = ops.bm25_exact_plan(counts, K)
                return ops.bm25_topk_split_exact(index.db_t, q_ids, q_idf, mask, flag, K, **form)

            def count_only():
                return ops.bm25_exact_count(index.db_t, ids, index.cols, mask, **form)
            again = chain()
            torch.cuda.synchronize()
            for g, w in zip(again, got):
                assert torch.equal(g.view(torch.int64), w.view(torch.int64)), (label, Q)
            graphs = {"plain": _graph_of(plain, REPS)[0], "chain": _graph_of(chain, REPS)[0], "count": _graph_of(count_only, REPS)[0]}
            ms = time_alternating(graphs, REPS, 50.0 if quick else MIN_TIMED_MS)
            emit("%-14s Q %4d | plain %.1f | count + plan + exact scan %.1f (the count alone %.1f) | chain / plain = %.4f" %
                 (label, Q, ms["plain"] * 1e3, ms["chain"] * 1e3, ms["count"] * 1e3, ms["chain"] / ms["plain"]))
            del graphs
        del index
    emit("   (every form: retrieve(ids, same=) equals BM25_topk_retrieval_v4(live rows, ..., exact_match_col_indices=[0]) bit for bit at every Q)")

    emit("== same (ii): replayed OnlineScorer.score(ids, same=) against replayed score(ids) [us per request], %s, immutable %d-row pool; "
         "host clock + synchronise, rounds of 200 requests alternating" % (name, n_pool))
    scorer = OnlineScorer(model, pool, cfg, graph=True)
    for B in (1, 16, 256):
        ids = torch.from_numpy(queries[B].astype(np.int32)).to(dev)
        for _ in range(5):
            y_same, y_plain = scorer.score(ids, same=same), scorer.score(ids)
        torch.cuda.synchronize()
        assert all(e[1] for e in scorer._same_graphs.values()) and all(e[1] for e in scorer._graphs.values()), "not captured"
        per = {"same": [], "score": []}
        while min(sum(v) for v in per.values()) * 200 / 1e6 < min_s or min(len(v) for v in per.values()) < 3:
            per["same"].append(_replay_round(_SameSide(scorer, same), ids))
            per["score"].append(_replay_round(scorer, ids))
        a, b = (sum(per[k]) / len(per[k]) for k in ("same", "score"))
        emit("B %4d | score(same=) %s | score %s | same / plain = %.4f | predictions differ: %s"
             % (B, _stats(per["same"]), _stats(per["score"]), a / b, not torch.equal(y_same, y_plain)))
    emit("   (%d score(same=) graphs, %d score() graphs)" % (len(scorer._same_graphs), len(scorer._graphs)))


def part_top(emit, quick):
    from rat_amd import ops
    from rat_amd.online import OnlineScorer, _first_rows
    name, model, rows, vocab, cfg, n_pool, _capacity = _movielens(quick)
    dev = torch.device("cuda:0")
    min_s = 0.05 if quick else MIN_TIMED_MS / 1e3
    pool = rows(n_pool)
    rs = np.random.RandomState(7)
    scorer = OnlineScorer(model, pool, cfg, graph=True)
    L, n, cols = len(vocab), 10, [1]                                        # the candidates of a request differ in the item column
    W = len(cols)
    grid = [(R, C) for R in ((1, 16) if quick else (1, 16, 64)) for C in (64, 256, 1024) if R * C <= scorer.graph_max_batch]
    emit("== top: %s, %d-row pool, requests of one context row and C_r candidates (column %s), n = %d; grid within graph_max_batch = %d"
         % (name, n_pool, cols, n, scorer.graph_max_batch))

    def point(R, C_r):
        C = R * C_r
        contexts = np.stack([rs.randint(0, v, size=R) for v in vocab], axis=1).astype(np.int32)
        cand = np.stack([rs.randint(0, vocab[c], size=C) for c in cols], axis=1).astype(np.int32)
        off = (np.arange(R + 1) * C_r).astype(np.int64)
        return C, contexts, cand, off

    def host_way(contexts, cand, off):
        """what a caller does without the ranked calls: expand on the host, upload, score, read everything back, sort per request"""
        ids = np.repeat(contexts, np.diff(off), axis=0)
        ids[:, cols] = cand
        y = scorer.score_requests((ids, off))[0].cpu().numpy()
        pos = np.full((len(off) - 1, n), -1, dtype=np.int32)
        val = np.zeros((len(off) - 1, n), dtype=np.float32)
        lens = np.zeros(len(off) - 1, dtype=np.int32)
        for r, (a, b) in enumerate(zip(off[:-1], off[1:])):
            order = np.argsort(-y[a:b], kind="stable")[:n]
            pos[r, :len(order)], val[r, :len(order)], lens[r] = order, y[a:b][order], len(order)
        return pos, val, lens

    def ranked_way(contexts, cand, off):
        pos, val, lens = scorer.top_candidates(contexts, cand, cols, off, n)
        return pos.cpu().numpy(), val.cpu().numpy(), lens.cpu().numpy()

    results = []
    for R, C_r in grid:
        C, contexts, cand, off = point(R, C_r)
        for _ in range(scorer.graph_warmup + 2):
            got = ranked_way(contexts, cand, off)
            want = host_way(contexts, cand, off)
        torch.cuda.synchronize()
        P = 1 << (C - 1).bit_length()
        chain = [e[1] for k, e in scorer._top_cand_graphs.items() if k[0] == P]
        assert len(chain) == 1 and chain[0], "the ranked chain of %d rows was not captured" % P
        same = all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want))
        # (i) the kernel alone against the replayed chain, device events
        y = torch.from_numpy(rs.rand(P).astype(np.float32)).to(dev)
        first = _first_rows(off, None, C, dev, pad_to=P)
        kernel, _ = _graph_of(lambda: ops.topn_seg(y, first, n), REPS)
        t_kernel = time_alternating({"k": kernel}, REPS, 50.0 if quick else 200.0)["k"] * 1e3
        t_chain = time_alternating({"c": chain[0].graph}, 1, 50.0 if quick else 200.0)["c"] * 1e3
        # (ii) the two ways, host clock, alternating
        per = {"ranked": [], "host": []}
        while min(sum(v) for v in per.values()) / 1e6 < min_s or min(len(v) for v in per.values()) < 5:
            for label, fn in (("ranked", ranked_way), ("host", host_way)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    fn(contexts, cand, off)
                per[label].append((time.perf_counter() - t0) / 10 * 1e6)
        results.append((R, C_r, C, P, t_kernel, t_chain, per, same))
    emit("== top (i): device time per call [us]: rat_topn_seg alone (hipGraph of %d calls over P rows, device events) and the replayed "
         "top_candidates chain (expand -> prepare -> scan -> assemble -> forward -> topn; its captured graph, device events)" % REPS)
    for R, C_r, C, P, t_kernel, t_chain, per, same in results:
        emit("R %3d x C_r %4d (P %4d) | rat_topn_seg %.1f | chain %.1f | share %.2f %%" % (R, C_r, P, t_kernel, t_chain, 100.0 * t_kernel / t_chain))
    emit("== top (ii): one call [us], host clock: replayed top_candidates + pos, y and lens read back, against host expansion + upload + "
         "replayed score_requests + all predictions read back + numpy stable top-n per request; rounds of 10 calls alternating; mean "
         "(min .. max over the rounds)")
    for R, C_r, C, P, t_kernel, t_chain, per, same in results:
        a, b = (sum(per[k]) / len(per[k]) for k in ("ranked", "host"))
        emit("R %3d x C_r %4d | ranked %s | host %s | host / ranked = %.2fx | results equal bit for bit: %s"
             % (R, C_r, _stats(per["ranked"]), _stats(per["host"]), b / a, same))
    emit("== top (iii): bytes per call, derived from the shapes (L = %d, W = %d, n = %d; both ways also upload first_row, 8 P bytes, when "
         "the request sizes changed since the last call; the ranked way the R head rows besides, 8 R bytes)" % (L, W, n))
    for R, C_r, C, P, _k, _c, _per, _same in results:
        emit("R %3d x C_r %4d | H2D ranked %7d (R L + C W ids)  host %7d (C L ids) | D2H ranked %6d (R (8 n + 4))  host %6d (4 C)"
             % (R, C_r, 4 * (R * L + C * W), 4 * C * L, R * (8 * n + 4), 4 * C))
    emit("   (%d ranked-candidate graphs, %d bucket graphs)" % (len(scorer._top_cand_graphs), len(scorer._bucket_graphs)))


def part_rank(emit, quick):
    from rat_amd import ops
    from rat_amd.online import OnlineScorer, _first_rows
    name, model, rows, vocab, cfg, n_pool, _capacity = _movielens(quick)
    dev = torch.device("cuda:0")
    min_s = 0.05 if quick else MIN_TIMED_MS / 1e3
    pool = rows(n_pool)
    rs = np.random.RandomState(7)
    scorer = OnlineScorer(model, pool, cfg, graph=True)
    L, n_top, cols = len(vocab), RANK_TOPN, [1]                             # the candidates of a request differ in the item column
    grid = [(R, C) for R in ((1, 16) if quick else (1, 16, 64)) for C in (64, 256, 1024) if R * C <= scorer.graph_max_batch]
    grid.append((1, scorer.graph_max_batch))
    emit("== rank: %s, %d-row pool, requests of C_r candidate rows (one context, the candidates differ in column %s); the --top grid "
         "and one request of graph_max_batch = %d rows" % (name, n_pool, cols, scorer.graph_max_batch))

    def point(R, C_r):
        C = R * C_r
        ids = np.repeat(np.stack([rs.randint(0, v, size=R) for v in vocab], axis=1).astype(np.int32), C_r, axis=0)
        ids[:, cols] = np.stack([rs.randint(0, vocab[c], size=C) for c in cols], axis=1)
        return C, ids, (np.arange(R + 1) * C_r).astype(np.int64)

    def host_way(ids, off):
        """what a caller does without the call: score, read every prediction back, one numpy stable sort per request"""
        y = scorer.score_requests((ids, off))[0].cpu().numpy()
        order, val, rank = np.empty(len(y), np.int32), np.empty(len(y), np.float32), np.empty(len(y), np.int32)
        for a, b in zip(off[:-1], off[1:]):
            o = np.argsort(-y[a:b], kind="stable")
            order[a:b], val[a:b] = o, y[a:b][o]
            rank[a:b][o] = np.arange(b - a)
        return order, val, rank

    def ranked_way(ids, off):
        r = scorer.rank_requests((ids, off))
        return r.order.cpu().numpy(), r.val.cpu().numpy(), r.rank.cpu().numpy()

    def ranked_resident(ids, off):
        """the ranking stays where its consumer is: nothing is read back"""
        r = scorer.rank_requests((ids, off))
        torch.cuda.synchronize()
        return r

    results = []
    for R, C_r in grid:
        C, ids, off = point(R, C_r)
        for _ in range(scorer.graph_warmup + 2):
            got = ranked_way(ids, off)
            want = host_way(ids, off)
        torch.cuda.synchronize()
        P = 1 << (C - 1).bit_length()
        chain = [e[1] for k, e in scorer._rank_graphs.items() if k[0] == P]
        assert len(chain) == 1 and chain[0], "the fully ranked chain of %d rows was not captured" % P
        same = all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want))
        # (i) the kernels alone against the replayed chain, device events
        y = torch.from_numpy(rs.rand(P).astype(np.float32)).to(dev)
        first = _first_rows(off, None, C, dev, pad_to=P)
        alone = {"rank": _graph_of(lambda: ops.rank_seg(y, first), REPS)[0], "topn": _graph_of(lambda: ops.topn_seg(y, first, n_top), REPS)[0]}
        t_alone = {k: v * 1e3 for k, v in time_alternating(alone, REPS, 50.0 if quick else 200.0).items()}
        t_chain = time_alternating({"c": chain[0].graph}, 1, 50.0 if quick else 200.0)["c"] * 1e3
        # (ii) the ways, host clock, alternating
        per = {"ranked": [], "resident": [], "host": []}
        while min(sum(v) for v in per.values()) / 1e6 < min_s or min(len(v) for v in per.values()) < 5:
            for label, fn in (("ranked", ranked_way), ("resident", ranked_resident), ("host", host_way)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    fn(ids, off)
                per[label].append((time.perf_counter() - t0) / 10 * 1e6)
        results.append((R, C_r, C, P, t_alone, t_chain, per, same))
    emit("== rank (i): device time per call [us]: rat_rank_seg alone and rat_topn_seg at n = %d alone (hipGraphs of %d calls over P rows, "
         "device events, alternating) and the replayed rank_requests chain (prepare -> scan -> assemble -> forward -> rank; its captured "
         "graph, device events)" % (n_top, REPS))
    for R, C_r, C, P, t_alone, t_chain, per, same in results:
        emit("R %3d x C_r %4d (P %4d) | rat_rank_seg %.1f | rat_topn_seg(n = %d) %.1f | rank / topn = %.2f | chain %.1f | share %.2f %%"
             % (R, C_r, P, t_alone["rank"], n_top, t_alone["topn"], t_alone["rank"] / t_alone["topn"], t_chain, 100.0 * t_alone["rank"] / t_chain))
    emit("== rank (ii): one call [us], host clock: replayed rank_requests + order, val and rank read back (ranked), the same with the "
         "ranking left on the device and one synchronise (resident), against replayed score_requests + all predictions read back + "
         "np.argsort(-y_r, kind=\"stable\") per request (host); rounds of 10 calls alternating; mean (min .. max over the rounds)")
    for R, C_r, C, P, t_alone, t_chain, per, same in results:
        a, c, b = (sum(per[k]) / len(per[k]) for k in ("ranked", "resident", "host"))
        emit("R %3d x C_r %4d | ranked %s | resident %s | host %s | host / ranked = %.2fx | host / resident = %.2fx | results equal bit for bit: %s"
             % (R, C_r, _stats(per["ranked"]), _stats(per["resident"]), _stats(per["host"]), b / a, b / c, same))
    emit("== rank (iii): bytes per call, derived from the shapes (L = %d; every way uploads C L ids, and first_row, 8 P bytes, when the "
         "request sizes changed since the last call)" % L)
    for R, C_r, C, P, _a, _c, _per, _same in results:
        emit("R %3d x C_r %4d | H2D %8d (C L ids) every way | D2H ranked %6d (order, val, rank: 12 C)  resident %d  host %6d (4 C)"
             % (R, C_r, 4 * C * L, 12 * C, 0, 4 * C))
    emit("   (%d fully-ranked graphs, %d bucket graphs)" % (len(scorer._rank_graphs), len(scorer._bucket_graphs)))


def part_catalogue(emit, quick, postings=False):
    from rat_amd.online import OnlineScorer
    name, model, rows, vocab, cfg, n_pool, _capacity = _movielens(quick)
    min_s = 0.05 if quick else MIN_TIMED_MS / 1e3
    pool = rows(n_pool)
    rs = np.random.RandomState(11)
    scorer = OnlineScorer(model, pool, cfg, graph=True)
    L, n, cols = len(vocab), 10, [1]                                        # the items of the catalogue differ in the item column
    W = len(cols)
    grid = [(M, R) for M in ((4096,) if quick else (4096, 65536)) for R in (1, 16)]
    emit("== catalogue: %s, %d-row pool, R users against ALL M items of a resident catalogue (column %s), n = %d, chunk = graph_max_batch // R "
         "= %d // R items per request per pass" % (name, n_pool, cols, n, scorer.graph_max_batch))

    def host_way(contexts, cat, chunk):
        """what a caller does without the catalogue: per chunk expand on the host, upload, score, read the predictions back, merge in numpy"""
        R, M = len(contexts), len(cat)
        items = np.full((R, n), -1, dtype=np.int32)
        val = np.zeros((R, n), dtype=np.float32)
        lens = np.zeros(R, dtype=np.int32)
        for i0 in range(0, M, chunk):
            m = min(chunk, M - i0)
            ids = np.repeat(contexts, m, axis=0)
            ids[:, cols] = np.tile(cat[i0:i0 + m], (R, 1))
            y = scorer.score_requests((ids, np.arange(R + 1, dtype=np.int64) * m))[0].cpu().numpy().reshape(R, m)
            for r in range(R):
                v = np.concatenate([val[r, :lens[r]], y[r]])
                i = np.concatenate([items[r, :lens[r]], np.arange(i0, i0 + m, dtype=np.int32)])
                order = np.argsort(-v, kind="stable")[:n]
                items[r, :len(order)], val[r, :len(order)], lens[r] = i[order], v[order], len(order)
        return items, val, lens

    def catalogue_way(contexts, _cat, chunk):
        items, val, lens = scorer.top_catalogue(contexts, n, chunk=chunk)
        return items.cpu().numpy(), val.cpu().numpy(), lens.cpu().numpy()

    def postings_way(contexts, _cat, chunk):
        items, val, lens = scorer.top_catalogue(contexts, n, chunk=chunk, postings=True)
        return items.cpu().numpy(), val.cpu().numpy(), lens.cpu().numpy()

    sides = [("catalogue", catalogue_way), ("host", host_way)]
    if postings:
        sides.insert(1, ("postings", postings_way))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scorer.build_postings()
        torch.cuda.synchronize()
        t_build = (time.perf_counter() - t0) * 1e3
    results = []
    for M, R in grid:
        chunk = min(max(1, scorer.graph_max_batch // R), M)
        contexts = np.stack([rs.randint(0, v, size=R) for v in vocab], axis=1).astype(np.int32)
        cat = np.stack([rs.randint(0, vocab[c], size=M) for c in cols], axis=1).astype(np.int32)
        scorer.set_catalogue(cat, cols)
        for _ in range(scorer.graph_warmup + 1):
            got = catalogue_way(contexts, cat, chunk)
            want = host_way(contexts, cat, chunk)
            if postings:
                shared = postings_way(contexts, cat, chunk)
        torch.cuda.synchronize()
        same = all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want))
        same_p = postings and all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(shared, got))
        per = {label: [] for label, _fn in sides}
        while min(sum(v) for v in per.values()) / 1e6 < min_s or min(len(v) for v in per.values()) < 3:
            for label, fn in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(contexts, cat, chunk)
                per[label].append((time.perf_counter() - t0) * 1e6)
        results.append((M, R, chunk, per, same, same_p))
    emit("== catalogue (i): one call [us], host clock: top_catalogue (per pass sweep expansion -> replayed score_requests -> rat_topn_seg -> "
         "rat_topn_merge, eager around the bucket graph) + items, y and lens read back, against the host loop: per chunk host expansion + "
         "upload + replayed score_requests + all predictions read back + numpy merge; one call per round, alternating; mean (min .. max)")
    for M, R, chunk, per, same, _same_p in results:
        a, b = (sum(per[k]) / len(per[k]) for k in ("catalogue", "host"))
        emit("M %5d x R %2d (%3d passes of %4d) | catalogue %s | host %s | host / catalogue = %.2fx | results equal bit for bit: %s"
             % (M, R, (M + chunk - 1) // chunk, chunk, _stats(per["catalogue"]), _stats(per["host"]), b / a, same))
    emit("== catalogue (ii): bytes per call, derived from the shapes (L = %d, W = %d, n = %d; the catalogue itself, 4 M W bytes, goes up once, "
         "at set_catalogue)" % (L, W, n))
    for M, R, chunk, _per, _same, _same_p in results:
        emit("M %5d x R %2d | H2D catalogue %6d (R L ids)  host %9d (R M L ids) | D2H catalogue %5d (R (8 n + 4))  host %8d (4 R M)"
             % (M, R, 4 * R * L, 4 * R * M * L, R * (8 * n + 4), 4 * R * M))
    emit("   (%d bucket graphs, no others: %s)" % (len(scorer._bucket_graphs), not (scorer._top_graphs or scorer._top_cand_graphs)))
    if postings:
        _catalogue_postings(emit, scorer, results, t_build, n_pool, vocab, cols, min_s)


def _catalogue_postings(emit, scorer, results, t_build, n_pool, vocab, cols, min_s):
    """the third side of part_catalogue, and the parts of one pass alone"""
    from rat_amd import ops
    emit("== catalogue (iii): top_catalogue(postings=True) in the same rounds [us] — per pass one scan per USER below n_sorted, then "
         "rat_bm25_topk_postings over the rows, through bucket graphs of its own; build_postings() over the %d-row pool, once: %.1f ms "
         "(8 F capacity = %d bytes of lists)" % (n_pool, t_build, 2 * scorer.index._post[0].numel() * 4))
    for M, R, chunk, per, _same, same_p in results:
        a, c = (sum(per[k]) / len(per[k]) for k in ("catalogue", "postings"))
        apart = min(per["catalogue"]) > max(per["postings"])
        emit("M %5d x R %2d (%3d passes of %4d) | postings %s | catalogue / postings = %.2fx | every postings round faster than every "
             "catalogue round: %s | equal to top_catalogue() bit for bit: %s"
             % (M, R, (M + chunk - 1) // chunk, chunk, _stats(per["postings"]), a / c, apart, same_p))
    emit("   (%d bucket graphs, %d posting-list graphs)" % (len(scorer._bucket_graphs), len(scorer._postings_graphs)))
    # one pass of P = graph_max_batch rows, its parts alone: R users x P / R items
    P, index, dev = scorer.graph_max_batch, scorer.index, scorer.device
    rs = np.random.RandomState(12)
    emit("== catalogue (iv): the parts of one %d-row pass alone [us per pass]: hipGraphs of %d passes under device events, alternating"
         % (P, 5))
    for R in (1, 16):
        m = P // R
        ids = np.repeat(np.stack([rs.randint(0, v, size=R) for v in vocab], axis=1), m, axis=0).astype(np.int32)
        for c in cols:
            ids[:, c] = rs.randint(0, vocab[c], size=P)
        ids = torch.from_numpy(ids).to(dev)
        heads = torch.arange(R, dtype=torch.int64, device=dev) * m
        first_row = heads[:, None].expand(R, m).reshape(-1).contiguous()
        mask = index._varying_mask(cols)
        _rows, labels = scorer._constants(P)
        with torch.no_grad():
            nbr = index.retrieve(ids, _first_row=first_row)
            assert all(torch.equal(a, b) for a, b in zip(nbr, index._retrieve_shared(ids, first_row, heads, mask)))

            def forward():
                y_pred, _loss, _reg, _saved = scorer.model._run_forward(scorer._assemble_batch(ids, labels, nbr[1]), save=False, with_reg=False)
                return y_pred
            graphs = {"scan": _graph_of(lambda: index.retrieve(ids, _first_row=first_row), 5)[0],
                      "lists": _graph_of(lambda: index._retrieve_shared(ids, first_row, heads, mask), 5)[0],
                      "forward": _graph_of(forward, 5)[0]}
        t = time_alternating(graphs, 5, min_s * 1e3)
        emit("R %2d x %4d items | prepare + scan per row %8.1f | prepare + scan per user + posting lists %8.1f | assembly + eval forward %8.1f"
             % (R, m, t["scan"] * 1e3, t["lists"] * 1e3, t["forward"] * 1e3))


RANK_TOPN = 64                                                              # rat_topn_seg's largest page, beside the full ranking


class _SameSide:
    """score(ids, same=) behind the name _replay_round calls"""

    def __init__(self, scorer, same):
        self.score = lambda ids: scorer.score(ids, same=same)


class _RowsSide:
    """score_rows behind the name _replay_round calls"""

    def __init__(self, scorer):
        self.score = scorer.score_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--quick", action="store_true", help="a few small points only (plumbing check)")
    ap.add_argument("--append", action="store_true", help="measure the growing pool (append against a new index; replay with capacity)")
    ap.add_argument("--window", action="store_true", help="measure the sliding pool (replay with window=True; append on a full window)")
    ap.add_argument("--delete", action="store_true", help="measure deletion from the sliding pool (delete against a new index; replay)")
    ap.add_argument("--find", action="store_true", help="measure the pool addressed by key (find against numpy; relabel; replay)")
    ap.add_argument("--requests", action="store_true", help="measure requests that share a launch (score_requests against R x score)")
    ap.add_argument("--rows", action="store_true", help="measure the pool that looks at itself (horizon scan against the plain scan; score_rows)")
    ap.add_argument("--same", action="store_true", help="measure neighbours restricted to equal columns (the chain against the plain scan; score(same=))")
    ap.add_argument("--top", action="store_true", help="measure each request's top-n candidates (rat_topn_seg alone; top_candidates against the host way)")
    ap.add_argument("--rank", action="store_true", help="measure each request's full ranking (rat_rank_seg alone; rank_requests against the host way)")
    ap.add_argument("--catalogue", action="store_true", help="measure the resident item catalogue (top_catalogue against the host loop over chunks)")
    ap.add_argument("--postings", action="store_true", help="with --catalogue: top_catalogue(postings=True) as a third side, and the parts of a pass")
    ap.add_argument("--trace", action="store_true", help="with --delete: only a few deletions per point, for a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("online_bench.py measures on the GPU; no GPU is visible and there is no CPU fallback")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    emit("tools/online_bench.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if args.append:
        part_append(emit, args.quick)
        return
    if args.window:
        part_window(emit, args.quick)
        return
    if args.delete:
        part_delete(emit, args.quick, args.trace)
        return
    if args.find:
        part_find(emit, args.quick)
        return
    if args.requests:
        part_requests(emit, args.quick)
        return
    if args.rows:
        part_rows(emit, args.quick)
        return
    if args.same:
        part_same(emit, args.quick)
        return
    if args.top:
        part_top(emit, args.quick)
        return
    if args.rank:
        part_rank(emit, args.quick)
        return
    if args.catalogue:
        part_catalogue(emit, args.quick, args.postings)
        return
    part1(emit, args.quick)
    part2(emit, args.quick)


if __name__ == "__main__":
    main()
