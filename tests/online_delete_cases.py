"""Checks of deletion from the sliding pool (``rat_pool_delete``, ``RetrievalIndex.delete`` / ``OnlineScorer.delete``) shared by
tests/test_online_delete.py (CPU, host-emulation build) and tests/test_gpu_online_delete.py (MI355X).

The reference of every comparison is the immutable path over the SURVIVORS in age order: ``np.delete`` of a logical-order copy at kernel
level, rat_bm25_topk on a contiguous copy of the survivors for the tie rule, a FRESH immutable RetrievalIndex / OnlineScorer over the
live rows at object level — never the window object against itself.  Every comparison is bit-exact; the predictions follow
online_cases' rule (identical bits when the fresh scorer's forward is run-to-run identical, else its 2e-6)."""
import numpy as np
import torch

import golden_cases as gc
import model_cases as mc
import online_cases as oc
import online_window_cases as wc

HEADS = (0, 1, 63, 64, 137, 199)
LIVE = (2, 65, 150, 200)
L, COLS, POISON = 5, [3, 0], -7


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- 1. rat_pool_delete == np.delete ---------------------------------------------------------------------------------------------------
class _Ring:
    """the three stores, poisoned, with n random rows at logical 0 .. n - 1 from slot `head` on; a numpy model of the same"""

    def __init__(self, capacity, n, head, store, rs, device):
        self.capacity, self.head, self.store, self.device = capacity, head, store, device
        self.ids = rs.randint(0, 1000, size=(n, L)).astype(np.int32)           # logical order
        self.labels = rs.rand(n).astype(np.float32)
        slots = (head + np.arange(n)) % capacity
        db_t = np.full((len(COLS), capacity), POISON, dtype=np.int32)
        pool_ids, pool_labels = np.full((capacity, L), POISON, dtype=np.int32), np.full(capacity, float(POISON), dtype=np.float32)
        db_t[:, slots], pool_ids[slots], pool_labels[slots] = self.ids[:, COLS].T, self.ids, self.labels
        self.db_t, self.hdr = _up(db_t, device), wc._header(n, head, device)
        self.pool_ids, self.pool_labels = (_up(pool_ids, device), _up(pool_labels, device)) if store else (None, None)
        self.scratch = torch.full((capacity * max(L, len(COLS)),), POISON, dtype=torch.int32, device=device)
        self.cols = _up(np.array(COLS, dtype=np.int32), device)
        self.never_live = np.ones(capacity, dtype=bool)                        # slots no row ever stood in: they keep their poison
        self.never_live[slots] = False

    def _rows(self):
        return (self.pool_ids, self.pool_labels) if self.store else ()

    def delete(self, lib, idx):
        from rat_amd import ops
        ops.pool_delete(self.db_t, self.hdr, _up(np.asarray(idx, dtype=np.int64), self.device), self.scratch, *self._rows(), lib=lib)
        self.ids, self.labels = np.delete(self.ids, idx, axis=0), np.delete(self.labels, idx)

    def push(self, lib, ids, labels):
        from rat_amd import ops
        ops.pool_push(_up(ids, self.device), _up(labels, self.device), self.cols, self.db_t, self.hdr, *self._rows(), lib=lib)
        E = max(0, len(self.ids) + len(ids) - self.capacity)
        self.never_live[(self.head + len(self.ids) + np.arange(len(ids))) % self.capacity] = False
        self.ids, self.labels = np.concatenate([self.ids, ids])[E:], np.concatenate([self.labels, labels])[E:]
        self.head = (self.head + E) % self.capacity

    def check(self, tag):
        n = len(self.ids)
        assert self.hdr.cpu().tolist() == [n, self.head], tag
        slots = (self.head + np.arange(n)) % self.capacity
        db_t = self.db_t.cpu().numpy()
        assert np.array_equal(db_t[:, slots], self.ids[:, COLS].T), tag
        assert (db_t[:, self.never_live] == POISON).all(), tag
        if self.store:
            pool_ids, pool_labels = self.pool_ids.cpu().numpy(), self.pool_labels.cpu().numpy()
            assert np.array_equal(pool_ids[slots], self.ids) and np.array_equal(pool_labels[slots], self.labels), tag
            assert (pool_ids[self.never_live] == POISON).all() and (pool_labels[self.never_live] == POISON).all(), tag


def deletion_lists(n, head, capacity, rs):
    """name -> ascending list; every one leaves at least one row, none is repeated"""
    cand = {"oldest": [0], "newest": [n - 1], "all but the newest": np.arange(n - 1), "all but the oldest": np.arange(1, n),
            "every other": np.arange(0, n, 2), "run of 64": np.arange(1, 65), "run of 65": np.arange(1, 66),
            "random third": np.sort(rs.choice(n, n // 3, replace=False))}
    if head + n > capacity:                                                # logical row w stands in slot 0
        w = capacity - head
        cand["across the wrap"] = np.unique([w - 1, w, min(w + 1, n - 1)])
    out, seen = {}, set()
    for name, idx in cand.items():
        idx = np.asarray(idx, dtype=np.int64)
        if 0 < len(idx) < n and idx.max() < n and tuple(idx) not in seen:
            seen.add(tuple(idx))
            out[name] = idx
    return out


def check_pool_delete(device, lib, capacity=200, heads=HEADS, live=LIVE):
    rs = np.random.RandomState(11)
    seen = dict(wrapped=False, across=False, run64=False, run65=False, suffix_wraps_in_a_wave=False)
    for store in (True, False):
        for head in heads:
            for n in live:
                for name, idx in deletion_lists(n, head, capacity, rs).items():
                    ring = _Ring(capacity, n, head, store, rs, device)
                    ring.delete(lib, idx)
                    ring.check("store=%s head=%d n=%d %s" % (store, head, n, name))
                    seen["wrapped"] |= head + n > capacity
                    seen["across"] |= name == "across the wrap"
                    seen["run64"] |= name == "run of 64" or (len(idx) == 64 and idx[0] == 1)
                    seen["run65"] |= name == "run of 65" or (len(idx) == 65 and idx[0] == 1)
                    seen["suffix_wraps_in_a_wave"] |= head + idx[0] < capacity < head + n - len(idx) and (capacity - head - idx[0]) % 64 != 0
    assert all(seen.values()), seen


def check_pool_delete_queued(device, lib, capacity=200):
    """push -> delete -> push issued back to back, nothing read in between: every launch takes the header from the one before it"""
    rs = np.random.RandomState(12)

    def rows(M):
        return rs.randint(0, 1000, size=(M, L)).astype(np.int32), rs.rand(M).astype(np.float32)
    for store in (True, False):
        ring = _Ring(capacity, 50, 137, store, rs, device)
        ring.push(lib, *rows(20))                                          # 137 + 70 > 200: the window wraps
        ring.delete(lib, np.sort(rs.choice(70, 23, replace=False)))
        ring.push(lib, *rows(170))                                         # 47 + 170 > 200: the oldest survivors leave
        ring.check("push, delete, push (store=%s)" % store)
        assert len(ring.ids) == capacity and ring.head == (137 + 17) % capacity
        ring.delete(lib, [0, capacity - 1])
        ring.push(lib, *rows(2))                                           # the freed room is refilled: nobody leaves
        ring.check("delete, push (store=%s)" % store)
        assert len(ring.ids) == capacity and ring.head == (137 + 17) % capacity


def check_pool_delete_large(device, lib, capacity=100_000, n=90_000, head=70_000, m=40_000):
    """many work-groups and several trips of the grid-stride loop"""
    rs = np.random.RandomState(13)
    ring = _Ring(capacity, n, head, True, rs, device)
    ring.delete(lib, np.sort(rs.choice(n, m, replace=False)))
    ring.check("%d random deletions" % m)
    ring.delete(lib, [0])
    ring.check("then the oldest")
    ring.delete(lib, [n - m - 2])
    ring.check("then the newest alone")


# ---- 2. a corrupt header or list addresses nothing outside the buffers (host-emulation build only) ----------------------------------
def check_pool_delete_corrupt(lib, capacity=200, guard=4096):
    from rat_amd import ops
    F = len(COLS)

    def guarded(numel, dtype, fill):
        whole = torch.full((numel + 2 * guard,), -99, dtype=dtype)
        whole[guard:guard + numel] = fill
        return whole, whole[guard:guard + numel]

    cases = [((capacity + 77, 5), [0, 3]), ((10 ** 12, 0), [1]), ((-5, 0), [0]), ((150, capacity), [2, 9]), ((150, capacity + 10 ** 9), [0]),
             ((150, -3), [4]), ((capacity + 1, capacity + 1), [0, capacity - 1]), ((150, 60), [3, 150]), ((150, 60), [10 ** 12]),
             ((150, 60), [-4, 2 ** 40]), ((150, 190), [7, 3, 3, -1, 500]), ((capacity, 199), list(range(capacity - 1, -1, -1))),
             ((3, 0), [0, 1, 2, 3, 4])]
    for store in (True, False):
        for (n, head), idx in cases:
            bufs = dict(db_t=guarded(F * capacity, torch.int32, 1), hdr=guarded(2, torch.int64, 0),
                        scratch=guarded(capacity * (L if store else F), torch.int32, 2), idx=guarded(len(idx), torch.int64, 0))
            if store:
                bufs.update(pool_ids=guarded(capacity * L, torch.int32, 3), pool_labels=guarded(capacity, torch.float32, 4.0))
            bufs["hdr"][1][:] = torch.tensor([n, head])
            bufs["idx"][1][:] = torch.tensor(idx)
            before_idx = bufs["idx"][0].clone()
            rows = (bufs["pool_ids"][1].view(capacity, L), bufs["pool_labels"][1]) if store else ()
            ops.pool_delete(bufs["db_t"][1].view(F, capacity), bufs["hdr"][1], bufs["idx"][1], bufs["scratch"][1], *rows, lib=lib)
            for name, (whole, _) in bufs.items():
                assert (whole[:guard] == -99).all() and (whole[-guard:] == -99).all(), (name, n, head, idx, store)
            assert torch.equal(bufs["idx"][0], before_idx)                 # the list is only read


# ---- 3. ties follow age after a deletion -----------------------------------------------------------------------------------------------
def check_delete_ties(device, lib, topks=(3, 9), splits=(1, 3, 0)):
    """online_window_cases._tie_pool: for query 0 rows 0, 256, 300 and 700 tie behind row 512.  The oldest of the group and one from its
    middle leave; the ring scan over the compacted window equals rat_bm25_topk over a contiguous copy of the survivors, whose tied rows
    (old 256 and 700, now 255 and 698) come in age order — wrapped, where the older one stands in the higher slot, and unwrapped"""
    from rat_amd import ops
    n = 1024
    db, qry = wc._tie_pool(n)
    gone = np.array([0, 300], dtype=np.int64)
    left = np.delete(db, gone, axis=0)
    db_t_live, q_ids, q_idf = oc.device_inputs(left, qry, device)
    for capacity, head in ((n, 0), (n, n - 280), (1500, 0), (1500, 1500 - 280)):
        logical = np.concatenate([db, np.tile([[99, 3]], (capacity - n, 1))])     # dead slots: the best possible match of query 0
        db_t, hdr = _up(wc._rotate(logical, head).astype(np.int32).T, device), wc._header(n, head, device)
        scratch = torch.empty(capacity * db.shape[1], dtype=torch.int32, device=device)
        ops.pool_delete(db_t, hdr, _up(gone, device), scratch, lib=lib)
        assert hdr.cpu().tolist() == [n - 2, head]
        if head:
            assert (head + 255) % capacity > (head + 698) % capacity          # age order is not slot order here
        for topk in topks:
            want = oc.single_range_topk(lib, db_t_live, q_ids, q_idf, topk)
            assert want[1][0][:3].tolist() == [510, 255, 698]
            for s in splits:
                got = ops.bm25_topk_split(db_t, q_ids, q_idf, topk, splits=s, header=hdr, ring=True, lib=lib)
                oc.assert_bitwise(got, want, "ties after delete: capacity=%d head=%d K=%d splits=%d" % (capacity, head, topk, s))


# ---- 4. the object == a fresh immutable one over the live rows, through appends, evictions and deletions --------------------------------
def _scenario(case, capacity, B, seed):
    """online_window_cases._scenario's tables (request rows 0 and 1 carry ids in the used columns that no filler row holds) with steps
    of its own.  Indices of a delete are logical positions at that moment; the comments give the row counts for capacity C."""
    data, pool, cols, _ = wc._scenario(case, capacity, 4, B, seed)
    _, filler, _ = oc.make_tables(case, 8 * capacity, 1, seed=seed + 2)
    at = [0]

    def fill(m):
        at[0] += m
        return filler[at[0] - m:at[0]]
    own, twin, C = data[:1], data[1:2], capacity
    steps = [("append", np.concatenate([own, fill(2)])),                          # n = 7; `own` is row 4, the only holder of its ids
             ("delete", [4]),                                                     # ... and leaves: its ids leave the tables.  n = 6
             ("append", np.concatenate([twin, twin, twin, fill(C - 9)])),         # twins at 6, 7, 8; n = C: the window is full
             ("delete", [C - 1, 7]),                                              # the newest row and the middle twin.  n = C - 2
             ("append", fill(2)),                                                 # the freed room is refilled, nobody leaves.  n = C
             ("append", np.concatenate([own, fill(3)])),                          # four rows leave: head = 4, the window is wrapped
             ("delete", [C - 4, 0, C - 5, 3]),                                    # both sides of the wrap, unsorted.  n = C - 4
             ("evict", 2),                                                        # head = 6, n = C - 6
             ("append", fill(5)),                                                 # n = C - 1
             ("delete", [C - 2, 1]),                                              # the newest again, wrapped.  n = C - 3
             ("append", fill(C // 2 + 3)),                                        # evicts
             ("delete", [0, 2, 4]),                                               # n = C - 3
             ("append", np.concatenate([twin, fill(2)])),                         # refilled exactly: n = C
             ("delete", list(range(1, C - 1))),                                   # all but the oldest and the newest
             ("append", fill(C))]                                                 # M == capacity after a deletion
    return data, pool, cols, steps


def check_delete_equals_fresh(name, gpu, lib, capacity=16, B=6, graph=False, train_step=False, seed=5):
    from rat_amd.online import OnlineScorer, RetrievalIndex, _RequestGraph
    case = gc.case_by_name(name)
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    mc.load_weights(model, case)
    model.eval()
    K = case["topk"]
    assert K == 3
    data, pool, cols, steps = _scenario(case, capacity, B, seed)
    ids = np.ascontiguousarray(data[:, :-1])
    ids_dev = torch.from_numpy(ids.astype(np.int32)).to(device)
    cfg = dict(topK=K, used_col_indices=cols, qry_batch_size=None, label_wise=False, split_type="random")

    scorer = OnlineScorer(model, pool, cfg, graph=graph, lib=lib, capacity=capacity, window=True)
    index = RetrievalIndex(pool, cols, K, device, lib=lib, capacity=capacity, window=True)
    assert index._scratch is None and scorer.index._scratch is None          # nobody who never deletes pays for the scratch
    exercised = dict(padding_is_newest_row=False, newest_row_deleted=False, first_row_hit_then_miss=False, deleted_while_wrapped=False,
                     freed_room_refilled=False, evicting_append=False, evict=False)
    captured = None
    if graph:                                                              # captured before the first delete
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
        # online_cases.check_online_vs_offline's rule: bitwise when the fresh scorer's forward is run-to-run bitwise, else its 2e-6
        assert torch.equal(y, y_want) if torch.equal(y_want, y_again) else float((y - y_want).abs().max()) <= 2e-6, tag
        if graph:
            now = [e[1] for e in scorer._graphs.values()]
            assert len(now) == 1 and now[0] is captured[0], "%s invalidated the captured request" % tag
        return want, b

    cur, head = pool, 0
    compare(cur, head, "at the start")
    freed = 0                                                              # rows the last step deleted from a FULL window
    for step, (op, arg) in enumerate(steps):
        before, tag = cur, "step %d: %s %s" % (step, op, len(arg) if op == "append" else arg)
        if op == "append":
            scorer.append(arg)
            index.append(arg)
            E = max(0, len(cur) + len(arg) - capacity)
            exercised["evicting_append"] |= E > 0
            exercised["freed_room_refilled"] |= freed > 0 and len(arg) == freed and E == 0
            cur, head = np.concatenate([cur, arg])[E:], (head + E) % capacity
        elif op == "evict":
            scorer.evict(arg)
            index.evict(arg)
            cur, head = cur[arg:], (head + arg) % capacity
            exercised["evict"] = True
        else:
            # the input forms, in turn: a list, a numpy int32 array, a host tensor, a device tensor
            forms = (arg, np.asarray(arg, dtype=np.int32), torch.tensor(arg), torch.tensor(arg, device=device))
            scorer.delete(forms[step % 4])
            index.delete(forms[(step + 1) % 4])
            exercised["deleted_while_wrapped"] |= head + len(cur) > capacity
            exercised["newest_row_deleted"] |= len(cur) - 1 in arg
            cur = np.delete(cur, arg, axis=0)
            exercised["first_row_hit_then_miss"] |= any(np.isin(data[0, c], before[:, c]) and not np.isin(data[0, c], cur[:, c]) for c in cols)
        freed = len(arg) if op == "delete" and len(before) == capacity else 0
        (v, i, ln), b = compare(cur, head, tag)
        i, ln = i.cpu().numpy(), ln.cpu().numpy()
        if op == "delete" and (ln < K).any():
            q = int(np.nonzero(ln < K)[0][0])
            got_row = b.idx[q, K].cpu().numpy()                            # the last neighbour slot is padding (-1): the newest survivor
            newest_slot = (head + len(cur) - 1) % capacity
            assert i[q, K - 1] == -1 and np.array_equal(got_row, cur[-1, :-1].astype(np.int32)), tag
            assert np.array_equal(got_row, scorer.pool_ids[newest_slot].cpu().numpy()), tag
            exercised["padding_is_newest_row"] = True
            if len(before) - 1 in arg:                                     # the newest row left: the padding moved to another row
                assert not np.array_equal(got_row, before[-1, :-1].astype(np.int32)), tag
    assert all(exercised.values()), exercised
    for obj in (index, scorer.index):                                      # allocated once, the size the class docstring gives
        assert obj._scratch.numel() == capacity * max(len(cols), ids.shape[1] if obj is scorer.index else 0)
    if graph and train_step:
        from rat_amd.data import DeviceBatch
        model.train()
        model.train_step(DeviceBatch(*scorer._assemble(ids_dev)))
        model.eval()
        y_new = scorer.score(ids_dev)                                      # still the graph captured before every deletion
        assert len(scorer._graphs) == 1 and [e[1] for e in scorer._graphs.values()][0] is captured[0]
        assert torch.equal(y_new, OnlineScorer(model, cur, cfg, graph=False, lib=lib).score(ids_dev))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def check_delete_refusals(gpu, lib):
    import pytest
    from rat_amd import ops
    from rat_amd.online import OnlineScorer, RetrievalIndex
    case = gc.case_by_name("tiny_seq_bn")
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    model.eval()
    data, pool, cols = oc.make_tables(case, 14, 20, seed=5)
    cfg = dict(topK=3, used_col_indices=cols, label_wise=False)
    for other in (OnlineScorer(model, pool, cfg, graph=False, lib=lib), OnlineScorer(model, pool, cfg, graph=False, lib=lib, capacity=17)):
        for obj in (other, other.index):
            with pytest.raises(ValueError, match="window"):
                obj.delete([1])
            with pytest.raises(ValueError, match="window"):
                obj.delete([])
    with pytest.raises(ValueError, match="window"):
        RetrievalIndex(pool, cols, 3, device, lib=lib).delete([0])
    scorer = OnlineScorer(model, pool, cfg, graph=False, lib=lib, capacity=17, window=True)
    scorer.append(data[:5])                                                # 14 + 5 > 17: two rows leave, head = 2
    ids = np.ascontiguousarray(data[:4, :-1])
    state = lambda: [t.clone() for t in (scorer.index.db_t, scorer.index.count, scorer.pool_ids, scorer.pool_labels,   # noqa: E731
                                         scorer.index.table_ids, scorer.index.table_idf, scorer.index.table_offsets)]
    host = lambda: (scorer.index._ring.copy(), scorer.index._head, [(v.copy(), c.copy()) for v, c in scorer.index._counts])   # noqa: E731
    before, ring_before, y_before, y_again = state(), host(), scorer.score(ids), scorer.score(ids)
    assert before[1].cpu().tolist() == [17, 2]

    def unchanged():
        assert len(scorer.index) == 17 and scorer.index.count.cpu().tolist() == [17, 2]
        assert all(torch.equal(a, b) for a, b in zip(before, state()))
        now = host()
        assert np.array_equal(now[0], ring_before[0]) and now[1] == ring_before[1]
        assert all(np.array_equal(a, c) and np.array_equal(b, d) for (a, b), (c, d) in zip(now[2], ring_before[2]))
        y = scorer.score(ids)
        assert torch.equal(y, y_before) if torch.equal(y_before, y_again) else float((y - y_before).abs().max()) <= 2e-6

    refused = [([3, 5, 3], "duplicate"), ([17], "outside"), ([-1], "outside"), (torch.tensor([2, -17]), "outside"),
               ([0.0, 1.0], "integer"), (torch.tensor([1.0], device=device), "integer"), (np.array([True, False]), "integer"),
               (np.arange(17)[::-1].copy(), "empty"), (np.zeros((2, 2), dtype=np.int64), "1-D")]
    for arg, word in refused:
        for obj in (scorer, scorer.index):
            with pytest.raises(ValueError, match=word):
                obj.delete(arg)
        unchanged()
    for empty in ([], np.zeros(0, dtype=np.int64), torch.zeros(0, dtype=torch.int64, device=device), ()):
        scorer.delete(empty)
        scorer.index.delete(empty)
    unchanged()
    assert scorer.index._scratch is None                                   # nothing was allocated, nothing launched
    # the entry point itself: an empty list returns before anything is looked at
    ops.pool_delete(scorer.index.db_t, scorer.index.count, torch.zeros(0, dtype=torch.int64, device=device),
                    torch.zeros(0, dtype=torch.int32, device=device), scorer.pool_ids, scorer.pool_labels, lib=lib)
    unchanged()
    scorer.delete([16, 0])                                                 # and a good one goes through
    assert len(scorer.index) == 15 and scorer.index.count.cpu().tolist() == [15, 2]
    scorer.delete(np.arange(14))                                           # down to one row
    assert scorer.index.count.cpu().tolist() == [1, 2]
    with pytest.raises(ValueError, match="empty"):
        scorer.delete([0])
