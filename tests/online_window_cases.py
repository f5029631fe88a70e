"""Checks of the sliding pool (RetrievalIndex / OnlineScorer with ``capacity`` and ``window=True``) shared by
tests/test_online_window.py (CPU, host-emulation build) and tests/test_gpu_online_window.py (MI355X).

The reference of every comparison is the immutable path over the LIVE rows in age order: rat_bm25_topk on a contiguous logical-order
copy at kernel level, a FRESH immutable RetrievalIndex / OnlineScorer over those rows at object level (itself tied to the offline
pipeline and the oracle by tests/online_cases.py) — never the window object against itself."""
import numpy as np
import torch

import golden_cases as gc
import model_cases as mc
import online_append_cases as ac
import online_cases as oc

SPLITS = (1, 3, 64, 256)
FIXED_HEADS = (0, 1, 255, 256, -1)                     # -1: capacity - 1


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _header(n, head, device):
    return torch.tensor([n, head], dtype=torch.int64, device=device)


def _rotate(logical, head):
    """logical row i -> physical slot (head + i) mod capacity"""
    return np.roll(logical, head, axis=0)


# ---- 1. rat_bm25_topk_split_ring == rat_bm25_topk over the live rows in logical order -------------------------------------------------
def check_ring_scan(device, lib, capacity=1200, ns=(1, 255, 1000, None), splits=SPLITS, topks=(3, 9), fixed_heads=FIXED_HEADS):
    """every head x row count x range count.  Per (n, splits) two more heads: one that puts the wrap (the logical row that lives in
    slot 0) strictly inside a range, one that puts it on a range boundary.  Dead slots are poisoned (online_append_cases.poison)."""
    from rat_amd import ops
    rs = np.random.RandomState(3)
    base, qry, w = ac.poisoned_pool(capacity, seed=17)
    q_ids, q_idf = _up(qry.astype(np.int32), device), _up(w, device)
    seen = dict(poison_would_win=False, wrap_inside_a_range=False, wrap_on_a_boundary=False, live_rows_wrap=False)
    for n in ns:
        n = capacity if n is None else n
        logical = ac.poison(base, n, rs)                                   # rows [n, capacity) are dead
        live_t = _up(logical[:n].astype(np.int32).T, device)               # what the immutable path would hold
        want = {k: oc.single_range_topk(lib, live_t, q_ids, q_idf, k) for k in topks}
        if n < capacity:
            whole = oc.single_range_topk(lib, _up(logical.astype(np.int32).T, device), q_ids, q_idf, topks[0])
            seen["poison_would_win"] |= bool((whole[1] >= n).any())
        for s in splits + (0,):
            chunk = -(-n // (s if s > 0 else 3))
            heads = [capacity - 1 if h < 0 else h for h in fixed_heads]
            if chunk < n:                                                  # logical row capacity - head is the one in slot 0
                on_boundary = chunk * ((n - 1) // chunk)                   # the first row of the last range that holds rows
                inside = on_boundary - (chunk + 1) // 2                    # strictly inside the range before it, if that has 2 rows
                if chunk > 1 and 0 < inside < n and inside % chunk:
                    heads.append(capacity - inside)
                    seen["wrap_inside_a_range"] |= s > 0
                heads.append(capacity - on_boundary)
                seen["wrap_on_a_boundary"] |= s > 0
            for head in heads:
                assert 0 <= head < capacity
                seen["live_rows_wrap"] |= head + n > capacity
                db_t, hdr = _up(_rotate(logical, head).astype(np.int32).T, device), _header(n, head, device)
                for topk in topks:
                    got = ops.bm25_topk_split(db_t, q_ids, q_idf, topk, splits=s, header=hdr, ring=True, lib=lib)
                    oc.assert_bitwise(got, want[topk], "n=%d head=%d K=%d splits=%d" % (n, head, topk, s))
    assert all(seen.values()), seen


def check_ring_scan_clamps(device, lib, capacity=300):
    """a header outside its domain addresses no row outside the buffers: the count is clamped to [0, capacity], the head to
    [0, capacity)"""
    from rat_amd import ops
    base, qry, w = ac.poisoned_pool(capacity, seed=5)
    q_ids, q_idf, db_t = _up(qry.astype(np.int32), device), _up(w, device), _up(base.astype(np.int32).T, device)
    full = oc.single_range_topk(lib, db_t, q_ids, q_idf, 3)
    oc.assert_bitwise(ops.bm25_topk_split(db_t, q_ids, q_idf, 3, splits=3, header=_header(capacity + 77, -5, device), ring=True, lib=lib),
                      full, "over")
    got = ops.bm25_topk_split(db_t, q_ids, q_idf, 3, splits=3, header=_header(-4, 0, device), ring=True, lib=lib)
    assert int(got[2].abs().max()) == 0 and int(got[1].max()) == -1
    last = np.roll(base, 1, axis=0)                                        # head = capacity - 1 after the clamp: slot capacity - 1 first
    want = oc.single_range_topk(lib, _up(last.astype(np.int32).T, device), q_ids, q_idf, 3)
    oc.assert_bitwise(ops.bm25_topk_split(db_t, q_ids, q_idf, 3, splits=2, header=_header(capacity, capacity + 9, device), ring=True, lib=lib),
                      want, "head over")


# ---- 2. ties follow age, not address -------------------------------------------------------------------------------------------------
def _tie_pool(n):
    """online_cases.check_split_ties' pool: query 0's best is row 512, then rows 0, 256, 300 and 700 tie"""
    db = np.full((n, 2), 7, dtype=np.int64)
    db[:, 0] = np.arange(n) % 5 + 10
    for r in (0, 256, 300, 512, 700):
        db[r, 1] = 3
    db[512, 0], db[700, 0] = 99, 98
    db[[0, 256, 300], 0] = 50
    return db, np.array([[99, 3], [98, 3]], dtype=np.int64)


def check_ring_ties(device, lib):
    """The tied rows 0 and 256 are logically OLDER than rows 300 and 700 and sit in HIGHER slots (before the wrap; their rivals after
    it).  The older ones must come first; ordering by slot would give another answer, which the test computes to show that."""
    from rat_amd import ops
    n = 1024
    db, qry = _tie_pool(n)
    for capacity in (n, 1500):
        head = capacity - 280                                              # logical rows 0 .. 279 before the wrap, the rest after it
        slot = lambda r: (head + r) % capacity                             # noqa: E731
        assert slot(0) > slot(300) and slot(256) > slot(700) and slot(0) > slot(700)
        logical = np.concatenate([db, np.tile([[99, 3]], (capacity - n, 1))])     # dead slots: the best possible match of query 0
        buf = _rotate(logical, head)
        db_t_live, q_ids, q_idf = oc.device_inputs(db, qry, device)
        db_t = _up(buf.astype(np.int32).T, device)
        for topk in (2, 3, 9):
            want = oc.single_range_topk(lib, db_t_live, q_ids, q_idf, topk)
            assert want[1][0][:2].tolist() == [512, 0] and (topk < 3 or int(want[1][0][2]) == 256)
            if capacity == n:                                              # the answer under physical-index ordering, as logical rows
                by_slot = oc.single_range_topk(lib, db_t, q_ids, q_idf, topk)
                as_logical = torch.where(by_slot[1] >= 0, (by_slot[1] - head) % capacity, by_slot[1])
                assert torch.equal(by_slot[0], want[0]) and not torch.equal(as_logical, want[1]), "slot order == age order: shows nothing"
                assert as_logical[0][:2].tolist() == [512, 300]
            for s in (1, 2, 3, 4, 0):
                got = ops.bm25_topk_split(db_t, q_ids, q_idf, topk, splits=s, header=_header(n, head, device), ring=True, lib=lib)
                oc.assert_bitwise(got, want, "ties capacity=%d K=%d splits=%d" % (capacity, topk, s))


# ---- 3. rat_pool_push / rat_pool_evict == numpy ----------------------------------------------------------------------------------------
def check_pool_push(device, lib, capacity=200, n0=3, sizes=(1, 63, 64, 65), wrapping=64):
    """After every step the header and ALL of the three buffers are compared: global row g (in push order) lives in slot g mod
    capacity, so a slot holds the last row pushed into it — live or not — or its fill value if nothing was ever written there; the
    de-rotated live window equals np.concatenate(everything pushed)[start:]."""
    from rat_amd import ops
    rs = np.random.RandomState(8)
    L, cols, FILL = 5, [3, 0], -7
    assert n0 + sum(sizes) < capacity < n0 + sum(sizes) + wrapping and (capacity - n0 - sum(sizes)) % 64 != 0
    db_t = torch.full((len(cols), capacity), FILL, dtype=torch.int32, device=device)
    pool_ids = torch.full((capacity, L), FILL, dtype=torch.int32, device=device)
    pool_labels = torch.full((capacity,), float(FILL), dtype=torch.float32, device=device)
    hdr, cols_d = _header(n0, 0, device), _up(np.array(cols, dtype=np.int32), device)
    all_ids = rs.randint(0, 1000, size=(n0, L)).astype(np.int32)
    all_labels = rs.randint(0, 2, size=n0).astype(np.float32)
    db_t[:, :n0], pool_ids[:n0], pool_labels[:n0] = _up(all_ids[:, cols].T, device), _up(all_ids, device), _up(all_labels, device)
    state = dict(start=0, stored=n0)                                       # rows [start, total) are live; the row store holds < stored

    def rows(M):
        return rs.randint(0, 1000, size=(M, L)).astype(np.int32), rs.randint(0, 2, size=M).astype(np.float32)

    def push(ids, labels, store=True):
        nonlocal all_ids, all_labels
        ops.pool_push(_up(ids, device), _up(labels, device), cols_d, db_t, hdr, *((pool_ids, pool_labels) if store else ()), lib=lib)
        if len(ids) > capacity:
            return
        all_ids, all_labels = np.concatenate([all_ids, ids]), np.concatenate([all_labels, labels])
        state["start"] = max(state["start"], len(all_ids) - capacity)
        if store:
            state["stored"] = len(all_ids)

    def check(tag):
        total, start = len(all_ids), state["start"]
        assert hdr.cpu().tolist() == [total - start, start % capacity], tag
        want_t = np.full((len(cols), capacity), FILL, dtype=np.int32)
        want_ids, want_lab = np.full((capacity, L), FILL, dtype=np.int32), np.full(capacity, float(FILL), dtype=np.float32)
        g = np.arange(max(0, total - capacity), total)                     # the last row pushed into every slot that ever took one
        want_t[:, g % capacity] = all_ids[g][:, cols].T
        g = np.arange(max(0, state["stored"] - capacity), state["stored"])
        want_ids[g % capacity], want_lab[g % capacity] = all_ids[g], all_labels[g]
        got_t, got_ids, got_lab = db_t.cpu().numpy(), pool_ids.cpu().numpy(), pool_labels.cpu().numpy()
        assert np.array_equal(got_t, want_t), tag
        if state["stored"] == total:
            assert np.array_equal(got_ids, want_ids) and np.array_equal(got_lab, want_lab), tag
        live = (start + np.arange(total - start)) % capacity               # de-rotated: the live window, oldest first
        assert np.array_equal(got_t[:, live], all_ids[start:][:, cols].T), tag
        if state["stored"] == total:
            assert np.array_equal(got_ids[live], all_ids[start:]) and np.array_equal(got_lab[live], all_labels[start:]), tag
        if total < capacity:
            assert (got_t[:, total:] == FILL).all() and (got_ids[total:] == FILL).all() and (got_lab[total:] == FILL).all(), tag

    def evict(m):
        ops.pool_evict(hdr, m, capacity, lib=lib)
        if 0 <= m < len(all_ids) - state["start"]:
            state["start"] += m

    check("start")
    for M in sizes:
        push(*rows(M))
        check("push %d" % M)
    room = capacity - len(all_ids)
    assert 0 < room < wrapping and room % 64 != 0                          # the next push wraps in the middle of a wave
    push(*rows(wrapping))
    assert state["start"] == wrapping - room
    check("wrapping push")
    evict(5)
    check("evict 5")
    push(*rows(2))                                                         # two pushes queued back to back: the second reads the header
    push(*rows(7))                                                         # the first one's tail launch wrote, on the device
    check("queued pushes")
    push(*rows(capacity))                                                  # M == capacity: every live row is replaced
    assert len(all_ids) - state["start"] == capacity
    check("M == capacity")
    before = [t.clone() for t in (db_t, pool_ids, pool_labels, hdr)]
    push(*rows(capacity + 1))                                              # M > capacity and m >= n write nothing
    evict(capacity)
    evict(capacity + 3)
    evict(-1)
    assert all(torch.equal(a, b) for a, b in zip(before, (db_t, pool_ids, pool_labels, hdr)))
    evict(capacity - 1)                                                    # down to one row
    assert hdr.cpu().tolist()[0] == 1
    check("evict all but one")
    evict(1)
    check("evict the last row: refused")
    push(*rows(65))
    check("push 65 after the evictions")
    keep_ids, keep_lab = pool_ids.clone(), pool_labels.clone()
    push(*rows(9), store=False)                                            # an index without the row store
    check("no row store")
    assert torch.equal(pool_ids, keep_ids) and torch.equal(pool_labels, keep_lab)


# ---- 4. the window object == a fresh immutable one over the live rows, through several laps -------------------------------------------
def _scenario(case, capacity, n0, B, seed):
    """-> (data, pool, cols, steps).  Request rows 0 and 1 carry ids in the used columns that no filler row holds (the fillers come
    from the narrow half of every vocabulary), so they match only the copies of themselves that the steps bring in and take out."""
    data, pool, cols = oc.make_tables(case, n0, B, seed=seed)
    vocab = [f["vocab_size"] for f in case["fields"] if f["type"] == "categorical"]
    assert len(vocab) == len(cols) and min(vocab) >= 5
    for r, back in ((0, 1), (1, 2)):
        for c, v in zip(cols, vocab):
            pad = [f.get("padding_idx") for f in case["fields"] if f["type"] == "categorical"][cols.index(c)]
            data[r, c] = v - back - (1 if pad is not None and pad >= v - 2 else 0)
            assert data[r, c] >= max(v - 3, 2) and not (pool[:, c] == data[r, c]).any()
    _, filler, _ = oc.make_tables(case, 8 * capacity, 1, seed=seed + 1)
    at = [0]

    def fill(m):
        at[0] += m
        return filler[at[0] - m:at[0]]
    own, twin = data[:1], data[1:2]
    C = capacity
    assert C >= 14 and n0 == 4
    steps = [("append", np.concatenate([own, fill(2)])),                          # the request's first row arrives: found on top
             ("append", np.concatenate([twin, twin, twin, fill(C - 12)])),        # request row 1's list is full (K = 3 twins)
             ("evict", 5),                                                        # the first pool and `own` leave: its ids leave the tables
             ("append", fill(6)),                                                 # the window wraps; the newest row sits below head
             ("evict", 3),                                                        # a twin leaves: request row 1's list is short again
             ("append", np.concatenate([fill(C - 1), own])),                      # M == capacity: everything is replaced
             ("append", fill(5)),
             ("evict", 2),
             ("append", np.concatenate([fill(3), twin, fill(3)])),
             ("append", fill(C // 2 + 3))]
    return data, pool, cols, steps


def check_window_equals_fresh(name, gpu, lib, capacity=16, B=6, graph=False, train_step=False, seed=5):
    from rat_amd.online import OnlineScorer, RetrievalIndex, _RequestGraph
    case = gc.case_by_name(name)
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    mc.load_weights(model, case)
    model.eval()
    K, n0 = case["topk"], 4
    assert K == 3
    data, pool, cols, steps = _scenario(case, capacity, n0, B, seed)
    assert sum(len(x) for op, x in steps if op == "append") > 2.5 * capacity
    ids = np.ascontiguousarray(data[:, :-1])
    ids_dev = torch.from_numpy(ids.astype(np.int32)).to(device)
    cfg = dict(topK=K, used_col_indices=cols, qry_batch_size=None, label_wise=False, split_type="random")

    scorer = OnlineScorer(model, pool, cfg, graph=graph, lib=lib, capacity=capacity, window=True)
    index = RetrievalIndex(pool, cols, K, device, lib=lib, capacity=capacity, window=True)
    assert len(index) == index.n_db == n0 and scorer.index.capacity == capacity and scorer.index.window
    # what lies outside the live rows must not matter: other ids than any row that will ever stand there
    scorer.pool_ids[n0:] = 1
    scorer.pool_labels[n0:] = 1.0
    scorer.index.db_t[:, n0:] = torch.from_numpy(ids[:1, cols].T.astype(np.int32)).to(device)        # would match request row 0
    exercised = dict(window_wrapped=False, id_left_a_table=False, first_row_hit_then_miss=False, full_then_short=False,
                     padding_is_newest_row_below_head=False, own_row_on_top=False, oldest_rows_left_on_append=False)
    captured = None
    if graph:                                                              # captured before the first append and the first eviction
        for _ in range(scorer.graph_warmup):
            scorer.score(ids_dev)
        scorer.score(ids_dev)
        captured = [e[1] for e in scorer._graphs.values()]
        assert [isinstance(g, _RequestGraph) for g in captured] == [True], "the request was not captured"

    def compare(cur, head, tag):
        f_scorer, f_index = OnlineScorer(model, cur, cfg, graph=False, lib=lib), RetrievalIndex(cur, cols, K, device, lib=lib)
        want = f_index.retrieve(ids)
        for obj in (index, scorer.index):
            assert len(obj) == obj.n_db == len(cur) and obj.count.cpu().tolist() == [len(cur), head], tag
            oc.assert_bitwise(obj.retrieve(ids), want, tag)
            f_tabs = (f_index.table_ids, f_index.table_idf, f_index.table_offsets)
            n_tab = int(f_tabs[2][-1])
            assert torch.equal(obj.table_offsets, f_tabs[2]) and torch.equal(obj.table_ids[:n_tab], f_tabs[0]), tag
            assert torch.equal(obj.table_idf[:n_tab].view(torch.int64), f_tabs[1].view(torch.int64)), tag
        fb, b = f_scorer.batch(ids), scorer.batch(ids)
        assert torch.equal(b.idx, fb.idx) and torch.equal(b.label_ids, fb.label_ids) and torch.equal(b.y_true, fb.y_true), tag
        y_want, y_again = f_scorer.score(ids_dev), f_scorer.score(ids_dev)
        y = scorer.score(ids_dev)
        assert y.shape == y_want.shape and y.dtype == torch.float32
        # online_cases.check_online_vs_offline's rule: bitwise when the parent's forward is run-to-run bitwise, else its 2e-6
        assert torch.equal(y, y_want) if torch.equal(y_want, y_again) else float((y - y_want).abs().max()) <= 2e-6, tag
        if graph:
            now = [e[1] for e in scorer._graphs.values()]
            assert len(now) == len(captured) and all(a is b_ for a, b_ in zip(now, captured)), "%s invalidated a captured request" % tag
        return want, b

    cur, head = pool, 0
    (v0, i0, l0), _ = compare(cur, head, "at the start")
    prev_lens = l0.cpu().numpy()
    for step, (op, arg) in enumerate(steps):
        before = cur
        if op == "append":
            rows, M = arg, len(arg)
            # the three input forms, in turn: numpy float64, host tensor, device tensor
            form = (rows, torch.from_numpy(rows), torch.from_numpy(rows).to(device))[step % 3]
            scorer.append(form)
            index.append(rows)
            E = max(0, len(cur) + M - capacity)
            exercised["oldest_rows_left_on_append"] |= E > 0
            cur = np.concatenate([cur, rows])[E:]
        else:
            E = arg
            scorer.evict(E)
            index.evict(E)
            cur = cur[E:]
        head = (head + E) % capacity
        tag = "step %d: %s %d" % (step, op, len(arg) if op == "append" else arg)
        (v, i, ln), b = compare(cur, head, tag)
        i, ln, v = i.cpu().numpy(), ln.cpu().numpy(), v.cpu().numpy()
        exercised["window_wrapped"] |= head + len(cur) > capacity
        if E:
            exercised["id_left_a_table"] |= any(not np.isin(before[:, c], cur[:, c]).all() for c in cols)
            exercised["first_row_hit_then_miss"] |= any(np.isin(data[0, c], before[:, c]) and not np.isin(data[0, c], cur[:, c])
                                                        for c in cols)
        if op == "evict":
            exercised["full_then_short"] |= bool(((prev_lens == K) & (ln < K)).any())
        if op == "append":
            for q in range(len(data)):                  # a query equal to a just-appended row: that row (or an equal, older one) on top
                same = np.nonzero((cur[:, cols] == data[q, cols]).all(axis=1))[0]
                if len(same) and same[0] >= len(cur) - M and v[q, 0] > 0:
                    assert i[q, 0] == same[0]
                    exercised["own_row_on_top"] = True
        newest_slot = (head + len(cur) - 1) % capacity
        if (ln < K).any() and newest_slot < head:
            q = int(np.nonzero(ln < K)[0][0])
            got_row = b.idx[q, K].cpu().numpy()                            # the last neighbour slot is padding (-1)
            assert i[q, K - 1] == -1 and np.array_equal(got_row, cur[-1, :-1].astype(np.int32))
            assert np.array_equal(got_row, scorer.pool_ids[newest_slot].cpu().numpy())
            assert not np.array_equal(got_row, scorer.pool_ids[capacity - 1].cpu().numpy())
            assert not np.array_equal(got_row, scorer.pool_ids[len(cur) - 1].cpu().numpy())
            exercised["padding_is_newest_row_below_head"] = True
        prev_lens = ln
    assert all(exercised.values()), exercised
    if graph and train_step:
        from rat_amd.data import DeviceBatch
        model.train()
        model.train_step(DeviceBatch(*scorer._assemble(ids_dev)))
        model.eval()
        y_new = scorer.score(ids_dev)                                      # still the graph captured before every append and eviction
        assert all(a is b_ for a, b_ in zip([e[1] for e in scorer._graphs.values()], captured)) and len(scorer._graphs) == 1
        assert torch.equal(y_new, OnlineScorer(model, cur, cfg, graph=False, lib=lib).score(ids_dev))


# ---- 5. refusals; a window never filled and never evicted == the immutable path -------------------------------------------------------
def check_window_refusals(gpu, lib):
    import pytest
    from rat_amd.online import OnlineScorer, RetrievalIndex
    case = gc.case_by_name("tiny_seq_bn")
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    model.eval()
    data, pool, cols = oc.make_tables(case, 14, 20, seed=5)
    cfg = dict(topK=3, used_col_indices=cols, label_wise=False)
    with pytest.raises(ValueError, match="capacity"):
        RetrievalIndex(pool, cols, 3, device, lib=lib, window=True)
    with pytest.raises(ValueError, match="capacity"):
        OnlineScorer(model, pool, cfg, graph=False, lib=lib, window=True)
    with pytest.raises(ValueError, match="capacity"):
        RetrievalIndex(pool, cols, 3, device, lib=lib, capacity=len(pool) - 1, window=True)
    for other in (OnlineScorer(model, pool, cfg, graph=False, lib=lib), OnlineScorer(model, pool, cfg, graph=False, lib=lib, capacity=17)):
        with pytest.raises(ValueError, match="window"):
            other.evict(1)
        with pytest.raises(ValueError, match="window"):
            other.index.evict(1)
    scorer = OnlineScorer(model, pool, cfg, graph=False, lib=lib, capacity=17, window=True)
    scorer.append(data[:5])                                                # 14 + 5 > 17: two rows leave, head = 2
    ids = np.ascontiguousarray(data[:4, :-1])
    state = lambda: [t.clone() for t in (scorer.index.db_t, scorer.index.count, scorer.pool_ids, scorer.pool_labels,   # noqa: E731
                                         scorer.index.table_ids, scorer.index.table_idf, scorer.index.table_offsets)]
    before, y_before = state(), scorer.batch(ids).idx.clone()
    assert before[1].cpu().tolist() == [17, 2]
    with pytest.raises(ValueError, match="capacity"):
        scorer.append(data[:18])                                           # M > capacity
    for m in (17, 18, -1):                                                 # everything, more than everything, a negative count
        with pytest.raises(ValueError, match="evict"):
            scorer.evict(m)
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
    assert len(scorer.index) == 17 and all(torch.equal(a, b) for a, b in zip(before, state()))
    assert torch.equal(scorer.batch(ids).idx, y_before)
    scorer.evict(0)                                                        # nothing leaves, nothing moves
    assert all(torch.equal(a, b) for a, b in zip(before, state()))
    scorer.append(data[:17])                                               # exactly the capacity is fine
    assert scorer.index.count.cpu().tolist() == [17, 2] and len(scorer.index) == 17
    scorer.evict(16)
    assert scorer.index.count.cpu().tolist() == [1, 1]


def check_window_without_pushes(name, gpu, lib, sizes, graph, train_step=False):
    """online_cases.check_online_vs_offline — every comparison with the offline pipeline — through scorers built with room to spare and
    ``window=True``, never filled and never evicted (online_append_cases.check_capacity_without_appends' wrapping)"""
    import rat_amd.online as online
    orig = online.OnlineScorer

    class Window(orig):
        def __init__(self, model, pool_array, retrieval_configs, graph=True, lib=None):
            super().__init__(model, pool_array, retrieval_configs, graph=graph, lib=lib, capacity=len(pool_array) + 3, window=True)
            assert self.index.window and self.index.count.cpu().tolist() == [len(pool_array), 0]
    online.OnlineScorer = Window
    try:
        oc.check_online_vs_offline(name, gpu, lib, sizes=sizes, graph=graph, train_step=train_step)
    finally:
        online.OnlineScorer = orig
