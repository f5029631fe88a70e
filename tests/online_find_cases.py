"""Checks of the pool addressed by key (``rat_pool_find``, ``rat_pool_set_labels``; ``find`` / ``set_labels`` / ``relabel_where`` /
``delete_where`` of RetrievalIndex and OnlineScorer) shared by tests/test_online_find.py (CPU, host-emulation build) and
tests/test_gpu_online_find.py (MI355X).

The reference of every comparison is numpy over a host model of the LIVE rows in age order: ``np.flatnonzero`` of the rows that equal a
key at kernel level, a FRESH immutable RetrievalIndex / OnlineScorer over the modelled rows and labels at object level — never the
object against itself.  Every comparison is exact."""
import ctypes

import numpy as np
import torch

import golden_cases as gc
import model_cases as mc
import online_cases as oc
import online_window_cases as wc

CAPACITY = 50
LIVE = (1, 2, 7, 33, 50)
GROUPS = (1, 3, 7, 64)
L, DB_COLS = 5, [3, 0, 4]                              # pool_ids has L columns; db_t holds the columns DB_COLS of the same rows
POISON, EVERYWHERE, ABSENT = 2, 7, 1000                # the id of every dead slot; the id ALL rows hold in column 1; an id nobody holds
LO, HI = -25, 26                                       # live ids are drawn from [LO, HI): negative ones too (the key order is signed)
FORMS = ("host", "dev", "ring")


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _sorted_keys(tuples):
    """what the host owes the kernel: distinct keys in lexicographic signed order (python's tuple order: not numpy's, not the library's)"""
    return np.array(sorted(set(tuple(int(x) for x in t) for t in tuples)), dtype=np.int32)


def _matches(live, cols, keys):
    """the model: logical indices of the rows of `live` [n, W] that equal some key on `cols`, ascending"""
    if len(live) == 0:
        return np.zeros(0, dtype=np.int64)
    hit = (live[:, cols][:, None, :] == np.asarray(keys)[None, :, :]).all(axis=2).any(axis=1)
    return np.flatnonzero(hit).astype(np.int64)


class _Pool:
    """n random rows at logical 0 .. n - 1 from slot `head` on, in both layouts; every other slot holds POISON in every column (and a
    poison label), and every key set of these checks contains the all-POISON key: a dead slot matches whatever is searched."""

    def __init__(self, capacity, n, head, form, rs, device):
        assert form in FORMS and (form == "ring" or head == 0) and 0 <= n <= capacity and 0 <= head < capacity
        self.capacity, self.n, self.head, self.form, self.device = capacity, n, head, form, device
        ids = rs.randint(LO, HI, size=(n, L)).astype(np.int32)
        ids[:, 1] = EVERYWHERE
        ids[ids == POISON] = POISON + 1                                        # no live row holds the poison id
        self.ids, self.labels = ids, rs.rand(n).astype(np.float32)
        slots = (head + np.arange(n)) % capacity
        pool_ids, pool_labels = np.full((capacity, L), POISON, dtype=np.int32), np.full(capacity, -5.0, dtype=np.float32)
        pool_ids[slots], pool_labels[slots] = ids, self.labels
        self.slots = slots
        self.pool_ids, self.pool_labels = _up(pool_ids, device), _up(pool_labels, device)
        self.db_t = _up(pool_ids[:, DB_COLS].T, device)
        self.header = None if form == "host" else (wc._header(n, head, device) if form == "ring" else _up(np.array([n], dtype=np.int64), device))

    def form_args(self):
        return dict(n_rows=self.n) if self.form == "host" else dict(header=self.header, ring=self.form == "ring")

    def store(self, field_major):
        """-> (device store, the live rows as that store holds them [n, W])"""
        return (self.db_t, self.ids[:, DB_COLS]) if field_major else (self.pool_ids, self.ids)

    def find(self, lib, field_major, cols, keys, **kw):
        from rat_amd import ops
        store, _ = self.store(field_major)
        return ops.pool_find(store, _up(np.asarray(cols, dtype=np.int32), self.device), _up(keys, self.device), field_major, lib=lib,
                             **self.form_args(), **kw)


def _key_sets(live, cols, rs):
    """name -> sorted distinct keys over `cols`, every set with the all-POISON key: M = 1 (the poison key alone, and a held key),
    3 and 40 keys, held and absent ones mixed, keys nobody holds, and — where column 1 is among `cols` alone — the key every row holds"""
    C, n = len(cols), len(live)
    poison = (POISON,) * C
    held = [tuple(live[i, cols]) for i in rs.randint(0, n, size=24)]
    absent = [tuple(rs.randint(LO, HI, size=C)) for _ in range(200)]
    out = {"M=1 poison only": [poison], "no match": [poison, (ABSENT,) * C, (-ABSENT,) * C],
           "M=3": [poison, held[0], absent[0]]}
    many = {poison, held[1], held[2]}
    for t in held[3:] + absent:
        if len(many) < 40:
            many.add(t)
    out["M=40"] = list(many)
    if C == 1:
        out["M=1 held"] = [held[0]]                                            # the one set without the poison key: M = 1 AND a match
    return {k: _sorted_keys(v) for k, v in out.items()}


def _column_sets(W):
    return [[W - 1], [2, 0], list(range(W))[::-1] if W == 3 else [4, 0, 1, 3, 2]]      # C = 1, 2 and all W columns, in a shuffled order


# ---- 1. rat_pool_find == np.flatnonzero, both layouts, the three forms ---------------------------------------------------------------------
def _pools(device, rs, live=LIVE, capacity=CAPACITY, forms=FORMS):
    for form in forms:
        for n in live:
            heads = [0] if form != "ring" else sorted({0, capacity - (n + 1) // 2, capacity - 1})
            for head in heads:
                yield _Pool(capacity, n, head, form, rs, device)


def check_find(device, lib):
    rs = np.random.RandomState(21)
    seen = dict(wrapped_with_matches_on_both_sides=False, all_rows_match=False, nothing_matches=False, one_row=False, negative_key_hit=False,
                all_columns=False, m40=False)
    for pool in _pools(device, rs):
        for field_major in (True, False):
            store, live = pool.store(field_major)
            W = live.shape[1]
            every = 1 if not field_major else None                             # column 1 (EVERYWHERE) is not among DB_COLS
            for cols in _column_sets(W) + ([[every]] if every is not None else []):
                sets = _key_sets(live, cols, rs)
                if cols == [every]:
                    sets = {"all rows": _sorted_keys([(POISON,), (EVERYWHERE,), (ABSENT,)])}
                for name, keys in sets.items():
                    want = _matches(live, cols, keys)
                    out_idx, out_count = pool.find(lib, field_major, cols, keys)
                    tag = "%s n=%d head=%d field_major=%s cols=%s %s" % (pool.form, pool.n, pool.head, field_major, cols, name)
                    assert out_idx.shape == (pool.capacity,) and int(out_count) == len(want), tag
                    got = out_idx.cpu().numpy()
                    assert np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all(), tag
                    w = pool.capacity - pool.head                              # logical row w stands in slot 0
                    seen["wrapped_with_matches_on_both_sides"] |= pool.head + pool.n > pool.capacity and (want < w).any() and (want >= w).any()
                    seen["all_rows_match"] |= name == "all rows" and len(want) == pool.n > 1
                    seen["nothing_matches"] |= name == "no match" and len(want) == 0
                    seen["one_row"] |= pool.n == 1 and len(want) == 1
                    seen["negative_key_hit"] |= len(want) > 0 and bool((live[want][:, cols[0]] < 0).any())
                    seen["all_columns"] |= len(cols) == W and len(want) > 0
                    seen["m40"] |= len(keys) == 40 and len(want) > 0
    assert all(seen.values()), seen


# ---- 2. the result does not depend on the number of ranges ------------------------------------------------------------------------------
def check_find_groups(device, lib, groups=GROUPS, live=(1, 33, 50), forms=FORMS):
    """empty ranges (more groups than rows), ranges shorter than a work-group, runs of consecutive matches across range boundaries
    (the key every row holds) — and a pool tall enough for several trips of a work-group over its range"""
    rs = np.random.RandomState(22)
    seen = dict(empty_ranges=False, boundary_inside_a_run=False, several_trips=False, wrapped=False)

    def sweep(pool, field_major, cols, keys, gs):
        store, live = pool.store(field_major)
        want = _matches(live, cols, keys)
        for g in gs:
            out_idx, out_count = pool.find(lib, field_major, cols, keys, groups=g)
            got = out_idx.cpu().numpy()
            tag = "%s n=%d head=%d field_major=%s cols=%s groups=%d" % (pool.form, pool.n, pool.head, field_major, cols, g)
            assert int(out_count) == len(want) and np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all(), tag
            if g > 0:
                R = -(-pool.n // g)
                seen["empty_ranges"] |= g * R >= pool.n + R
                seen["boundary_inside_a_run"] |= any(b - 1 in want and b in want for b in range(R, pool.n, R))
                seen["several_trips"] |= R > 2 * 256 and len(want) > 256
        seen["wrapped"] |= pool.head + pool.n > pool.capacity
    for pool in _pools(device, rs, live=live, forms=forms):
        sweep(pool, False, [1], _sorted_keys([(POISON,), (EVERYWHERE,)]), groups)                  # every live row, no dead slot
        sweep(pool, True, [0, 2], _key_sets(pool.ids[:, DB_COLS], [0, 2], rs)["M=40"], groups)
        sweep(pool, False, [4, 2], _key_sets(pool.ids, [4, 2], rs)["M=3"], groups)
    tall = _Pool(1500, 1400, 1300, "ring", rs, device)
    sweep(tall, True, [1], _key_sets(tall.ids[:, DB_COLS], [1], rs)["M=40"], (1, 2, 3))
    sweep(tall, False, [1, 0], _sorted_keys([(EVERYWHERE, v) for v in range(LO, HI, 2)] + [(POISON, POISON)]), (1, 2))
    assert all(seen.values()), seen


def check_find_large(device, lib, capacity=60_000, n=50_000, head=40_000):
    """many work-groups: the library's own choice of ranges at a capacity of several tens of thousands of rows"""
    rs = np.random.RandomState(23)
    pool = _Pool(capacity, n, head, "ring", rs, device)
    for field_major, cols in ((True, [2, 0]), (False, [0]), (False, [1])):
        store, live = pool.store(field_major)
        keys = _key_sets(live, cols, rs)["M=40"] if cols != [1] else _sorted_keys([(POISON,), (EVERYWHERE,)])
        want = _matches(live, cols, keys)
        assert len(want) > 100
        for g in (0, 4096):
            out_idx, out_count = pool.find(lib, field_major, cols, keys, groups=g)
            got = out_idx.cpu().numpy()
            assert int(out_count) == len(want) and np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all(), (cols, g)


# ---- 3. truncation and the -1 tail -----------------------------------------------------------------------------------------------------
def check_find_truncation(device, lib):
    rs = np.random.RandomState(24)
    GUARD = 77
    for pool in (_Pool(CAPACITY, 33, 30, "ring", rs, device), _Pool(CAPACITY, 50, 0, "dev", rs, device), _Pool(CAPACITY, 20, 0, "host", rs, device)):
        for field_major, cols, keys in ((False, [1], _sorted_keys([(POISON,), (EVERYWHERE,)])),
                                        (True, [0], _key_sets(pool.ids[:, DB_COLS], [0], rs)["M=40"])):
            store, live = pool.store(field_major)
            want = _matches(live, cols, keys)
            assert len(want) >= 4
            for max_out in (0, 1, len(want) - 1, len(want), len(want) + 1, len(want) + 9):
                for g in (0, 3):
                    whole = torch.full((max_out + 8,), GUARD, dtype=torch.int64, device=device)
                    _, out_count = pool.find(lib, field_major, cols, keys, out_idx=whole, max_out=max_out, groups=g)
                    got = whole.cpu().numpy()
                    k = min(len(want), max_out)
                    assert int(out_count) == len(want), (max_out, g)                        # the total, also when it does not fit
                    assert np.array_equal(got[:k], want[:k]) and (got[k:max_out] == -1).all(), (max_out, g)
                    assert (got[max_out:] == GUARD).all(), (max_out, g)                     # nothing behind max_out is written


# ---- 4. queued behind pushes, deletions and evictions -----------------------------------------------------------------------------------
def check_find_queued(device, lib, capacity=CAPACITY):
    """push -> find -> delete -> find -> evict -> find issued back to back: every launch takes the header from the one before it; the
    results are looked at only at the end"""
    from rat_amd import ops
    rs = np.random.RandomState(25)
    pool = _Pool(capacity, 30, 35, "ring", rs, device)
    cols_d = _up(np.array(DB_COLS, dtype=np.int32), device)
    scratch = torch.empty(capacity * L, dtype=torch.int32, device=device)
    new_ids = rs.randint(LO, HI, size=(25, L)).astype(np.int32)
    new_ids[:, 1] = EVERYWHERE
    new_ids[new_ids == POISON] = POISON + 1
    new_labels = rs.rand(25).astype(np.float32)
    model, results = pool.ids, []

    def find_both(tag):
        for field_major, cols in ((True, [1, 2]), (False, [3]), (False, [1])):
            live = model[:, DB_COLS] if field_major else model
            keys = _key_sets(live, cols, rs)["M=40"] if cols != [1] else _sorted_keys([(POISON,), (EVERYWHERE,)])
            results.append((tag, cols, pool.find(lib, field_major, cols, keys), _matches(live, cols, keys)))
    ops.pool_push(_up(new_ids, device), _up(new_labels, device), cols_d, pool.db_t, pool.header, pool.pool_ids, pool.pool_labels, lib=lib)
    model = np.concatenate([model, new_ids])[5:]                               # 30 + 25 > 50: five rows leave, head = 40
    find_both("after the push")
    gone = np.sort(rs.choice(capacity, 17, replace=False))
    ops.pool_delete(pool.db_t, pool.header, _up(gone.astype(np.int64), device), scratch, pool.pool_ids, pool.pool_labels, lib=lib)
    model = np.delete(model, gone, axis=0)
    find_both("after the delete")
    ops.pool_evict(pool.header, 11, capacity, lib=lib)
    model = model[11:]
    find_both("after the evict")
    assert pool.header.cpu().tolist() == [22, (40 + 11) % capacity]
    for tag, cols, (out_idx, out_count), want in results:
        got = out_idx.cpu().numpy()
        assert int(out_count) == len(want) and np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all(), (tag, cols)
    assert sum(len(r[3]) > 0 for r in results) >= 6


# ---- 5. rat_pool_set_labels == numpy through the ring -----------------------------------------------------------------------------------
def check_set_labels(device, lib):
    from rat_amd import ops
    rs = np.random.RandomState(26)
    for pool in _pools(device, rs, live=(1, 33, 50)):
        n, cap = pool.n, pool.capacity
        model = np.full(cap, -5.0, dtype=np.float32)
        model[pool.slots] = pool.labels

        def check(tag):
            assert np.array_equal(pool.pool_labels.cpu().numpy(), model), "%s (%s n=%d head=%d)" % (tag, pool.form, n, pool.head)
        idx = rs.permutation(n)[:max(1, n // 2)].astype(np.int64)
        new = rs.rand(len(idx)).astype(np.float32)
        ops.pool_set_labels(pool.pool_labels, _up(idx, device), _up(new, device), lib=lib, **pool.form_args())
        model[pool.slots[idx]] = new
        check("a label per index")
        ops.pool_set_labels(pool.pool_labels, _up(idx[::-1].copy(), device), _up(np.array([0.25], dtype=np.float32), device), lib=lib,
                            **pool.form_args())
        model[pool.slots[idx]] = 0.25
        check("one label for all")
        # entries outside [0, n) are skipped: -1, n, the capacity, far outside — the dead slots keep their labels
        mixed = np.array([-1, n, 0, cap, -2 ** 40, n - 1, 2 ** 40, -1], dtype=np.int64)
        vals = np.arange(len(mixed), dtype=np.float32) + 10
        if n == 1:
            mixed, vals = mixed[:5], vals[:5]                                   # 0 and n - 1 are the same row
        ops.pool_set_labels(pool.pool_labels, _up(mixed, device), _up(vals, device), lib=lib, **pool.form_args())
        ok = (mixed >= 0) & (mixed < n)
        model[pool.slots[mixed[ok]]] = vals[ok]
        check("entries outside the live rows")
        # the padded list of a find, passed whole
        keys = _key_sets(pool.ids, [4], rs)["M=40"]
        want = _matches(pool.ids, [4], keys)
        out_idx, _ = pool.find(lib, False, [4], keys)
        assert out_idx.numel() == cap
        ops.pool_set_labels(pool.pool_labels, out_idx, _up(np.array([3.0], dtype=np.float32), device), lib=lib, **pool.form_args())
        model[pool.slots[want]] = 3.0
        check("the list of a find")
        ops.pool_set_labels(pool.pool_labels, torch.zeros(0, dtype=torch.int64, device=device), _up(np.array([9.0], dtype=np.float32), device),
                            lib=lib, **pool.form_args())
        check("an empty list")


# ---- 6. the objects == fresh immutable ones over the modelled rows and labels ---------------------------------------------------------------
def _flip(rows):
    out = rows.copy()
    out[:, -1] = 1.0 - out[:, -1]
    return out


def check_objects_equal_fresh(name, gpu, lib, form, capacity=24, n0=14, B=6, graph=False, train_step=False, seed=5):
    """set_labels, relabel_where, delete_where, append and evict interleaved; after every step score / batch / find of the object equal
    those of fresh immutable objects over the model.  form: "immutable", "capacity" or "window" (delete_where and evict in the last)."""
    from rat_amd.online import OnlineScorer, RetrievalIndex, _RequestGraph
    case = gc.case_by_name(name)
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    mc.load_weights(model, case)
    model.eval()
    K = case["topk"]
    data, pool, cols = oc.make_tables(case, n0, B, seed=seed)
    _, filler, _ = oc.make_tables(case, 4 * capacity, 1, seed=seed + 3)
    n_ids = pool.shape[1] - 1
    ids = np.ascontiguousarray(data[:, :-1])
    ids_dev = torch.from_numpy(ids.astype(np.int32)).to(device)
    cfg = dict(topK=K, used_col_indices=cols, qry_batch_size=None, label_wise=False, split_type="random")
    kw = dict(immutable={}, capacity=dict(capacity=capacity), window=dict(capacity=capacity, window=True))[form]
    scorer = OnlineScorer(model, pool, cfg, graph=graph, lib=lib, **kw)
    index = RetrievalIndex(pool, cols, K, device, lib=lib, **kw)
    assert scorer._found is None                                           # nobody who never calls relabel_where pays for its list
    if form != "immutable":                                                # what lies outside the live rows must not matter
        scorer.pool_ids[n0:] = torch.from_numpy(pool[0, :-1].astype(np.int32)).to(device)
        scorer.pool_labels[n0:] = 0.5
        for obj in (index, scorer.index):
            obj.db_t[:, n0:] = torch.from_numpy(pool[:1, cols].T.astype(np.int32)).to(device)
    captured = None
    if graph:                                                              # captured before the first relabel
        for _ in range(scorer.graph_warmup):
            scorer.score(ids_dev)
        scorer.score(ids_dev)
        captured = [e[1] for e in scorer._graphs.values()]
        assert [isinstance(g, _RequestGraph) for g in captured] == [True], "the request was not captured"
    other_col = [c for c in range(n_ids) if c not in cols][0]              # an id column the retrieval does not use: the row store only

    def compare(cur, tag):
        f_scorer = OnlineScorer(model, cur, cfg, graph=False, lib=lib)
        fb, b = f_scorer.batch(ids), scorer.batch(ids)
        assert torch.equal(b.idx, fb.idx) and torch.equal(b.label_ids, fb.label_ids) and torch.equal(b.y_true, fb.y_true), tag
        y_want, y = f_scorer.score(ids_dev), scorer.score(ids_dev)
        assert y.shape == y_want.shape and y.dtype == torch.float32 and torch.equal(y, y_want), tag
        oc.assert_bitwise(index.retrieve(ids), RetrievalIndex(cur, cols, K, device, lib=lib).retrieve(ids), tag)
        n = len(cur)
        assert len(scorer.index) == len(index) == n, tag
        head = int(scorer.index.count[1]) if form == "window" else 0
        cap = scorer.pool_labels.numel()
        assert np.array_equal(scorer.pool_labels.cpu().numpy()[(head + np.arange(n)) % cap], cur[:, -1].astype(np.float32)), tag
        # find of both objects against the model: a key held by the newest row and one nobody holds
        for obj, cc in ((index, cols[:2]), (index, cols[-1:]), (scorer, [other_col, cols[0]]), (scorer, list(range(n_ids)))):
            keys = np.stack([cur[-1, cc], cur[0, cc], np.full(len(cc), 10 ** 6)]).astype(np.int64)
            got = obj.find(cc, keys)
            assert got.dtype == torch.int64 and got.device.type == torch.device(device).type, tag
            assert np.array_equal(got.cpu().numpy(), _matches(cur[:, :-1].astype(np.int64), cc, keys)), (tag, cc)
        if graph:
            now = [e[1] for e in scorer._graphs.values()]
            assert len(now) == 1 and now[0] is captured[0], "%s invalidated the captured request" % tag
        return y

    cur = pool.copy()
    y_prev = compare(cur, "at the start")
    exercised = dict(retrieved_rows_relabelled=False, relabel_hit_several=False, relabel_hit_nothing=False, device_list_passed_whole=False,
                     deleted_by_key=form != "window", wrapped=form != "window", appended=form == "immutable")
    steps = ["labels list", "append", "relabel col", "retrieved", "delete item", "append big", "relabel rows", "evict", "labels device",
             "delete none", "relabel none", "delete rows", "retrieved device"]
    at = 0
    for step in steps:
        tag = "%s: %s" % (form, step)
        n = len(cur)
        if step in ("append", "append big"):
            if form == "immutable":
                continue
            M = 3 if step == "append" else capacity - n + (2 if form == "window" else 0)     # the window overflows by two rows
            rows = filler[at:at + M].copy()
            rows[-1, :-1] = cur[3, :-1]                                       # a copy of a row that stays comes in last: a key with two holders
            at += M
            scorer.append(rows)
            index.append(rows)
            E = max(0, n + M - capacity)
            cur = np.concatenate([cur, rows])[E:]
            exercised["appended"] = True
        elif step == "evict":
            if form != "window":
                continue
            scorer.evict(3)
            index.evict(3)
            cur = cur[3:]
        elif step == "labels list":                                         # host-side indices, a label each; then a scalar for some
            idx = [n - 1, 0, 2]
            scorer.set_labels(idx, 1.0 - cur[idx, -1])
            cur[idx, -1] = 1.0 - cur[idx, -1]
            scorer.set_labels(np.array([1], dtype=np.int32), 1)
            cur[1, -1] = 1.0
            scorer.set_labels(torch.tensor([3]), torch.tensor([0.0]))
            cur[3, -1] = 0.0
            scorer.set_labels([], 1.0)                                         # nothing to do
        elif step == "relabel col":                                         # every row that holds the newest row's id in one used column
            c = cols[0]
            keys = cur[-1:, [c]].astype(np.int64)
            want = _matches(cur[:, :-1].astype(np.int64), [c], keys)
            new = 1.0 - cur[-1, -1]
            count = scorer.relabel_where([c], keys, new)
            cur[want, -1] = new
            assert torch.is_tensor(count) and count.dtype == torch.int64 and int(count) == len(want) >= 1, tag
            assert scorer._found.numel() == scorer.pool_labels.numel() == (capacity if form != "immutable" else n0)
        elif step == "relabel rows":                                        # whole rows as keys, the newest (the copy) among them, unsorted
            keys = np.concatenate([cur[[n - 1, n // 2], :-1], np.full((1, n_ids), 10 ** 6)]).astype(np.int64)[::-1]
            want = _matches(cur[:, :-1].astype(np.int64), list(range(n_ids)), keys)
            count = scorer.relabel_where(list(range(n_ids)), torch.from_numpy(keys.copy()), 0.0)
            cur[want, -1] = 0.0
            found_before = scorer._found
            count2 = scorer.relabel_where(list(range(n_ids)), np.concatenate([keys, keys]), 1.0)       # repeated keys are one key
            cur[want, -1] = 1.0
            assert int(count) == int(count2) == len(want) and scorer._found is found_before, tag
            exercised["relabel_hit_several"] |= len(want) >= 3 if form != "immutable" else len(want) >= 2
        elif step == "relabel none":
            before = scorer.pool_labels.clone()
            count = scorer.relabel_where([other_col], [[10 ** 6]], 1.0)
            assert int(count) == 0 and torch.equal(scorer.pool_labels, before), tag
            exercised["relabel_hit_nothing"] = True
        elif step in ("retrieved", "retrieved device"):                     # the rows the request retrieves change their labels
            _v, i, _ln = scorer.index.retrieve(ids)
            got = np.unique(i.cpu().numpy())
            got = got[got >= 0]
            assert len(got) >= 2, tag
            if step == "retrieved":
                scorer.set_labels(got, 1.0 - cur[got, -1])
                cur[got, -1] = 1.0 - cur[got, -1]
            else:                                                              # the kernel's own list, -1 padding and repeats included
                new = 1.0 - float(np.round(cur[got, -1].mean()))               # the label fewer of them hold
                flat = i.reshape(-1)                                           # (a host tensor is validated: the emulated run passes `got`)
                scorer.set_labels(flat if flat.is_cuda else got, new)
                cur[got, -1] = new
                exercised["device_list_passed_whole"] |= not flat.is_cuda or bool((flat < 0).any().item()) or flat.numel() > len(got)
            y = compare(cur, tag)
            assert not torch.equal(y, y_prev), "%s: relabelling the retrieved rows changed no prediction" % tag
            exercised["retrieved_rows_relabelled"] = True
            y_prev = y
            continue
        elif step == "labels device":
            if gpu < 0:
                continue                                                       # no device tensor without a device
            idx = torch.tensor([n - 1, -1, 1, n, 10 ** 9], device=device)
            scorer.set_labels(idx, torch.tensor([0.0, 1.0, 1.0, 1.0, 1.0], device=device))
            cur[n - 1, -1], cur[1, -1] = 0.0, 1.0
        elif step in ("delete item", "delete rows", "delete none"):
            if form != "window":
                continue
            if step == "delete none":
                assert scorer.delete_where([other_col], [[10 ** 6]]) == 0 and index.delete_where(cols[:1], [[10 ** 6]]) == 0, tag
            else:
                cc = cols[:1] if step == "delete item" else cols                  # the index searches its used columns only
                keys = cur[[1, n - 2]][:, cc].astype(np.int64)
                want = _matches(cur[:, :-1].astype(np.int64), cc, keys)
                exercised["wrapped"] |= int(scorer.index.count[1]) + n > capacity
                assert scorer.delete_where(cc, keys) == len(want) and index.delete_where(cc, keys) == len(want), tag
                cur = np.delete(cur, want, axis=0)
                exercised["deleted_by_key"] |= len(want) >= 2
        else:
            raise AssertionError(step)
        y_prev = compare(cur, tag)
    assert all(exercised.values()), exercised
    if graph and train_step:
        from rat_amd.data import DeviceBatch
        model.train()
        model.train_step(DeviceBatch(*scorer._assemble(ids_dev)))
        model.eval()
        y_new = scorer.score(ids_dev)                                      # still the graph captured before the first relabel
        assert len(scorer._graphs) == 1 and [e[1] for e in scorer._graphs.values()][0] is captured[0]
        assert torch.equal(y_new, OnlineScorer(model, cur, cfg, graph=False, lib=lib).score(ids_dev))
        assert not torch.equal(y_new, y_prev), "the training step changed nothing"


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def check_find_refusals(gpu, lib):
    import pytest
    from rat_amd.online import OnlineScorer, RetrievalIndex
    case = gc.case_by_name("tiny_seq_bn")
    device = "cpu" if gpu < 0 else "cuda:%d" % gpu
    model = mc.build_model(case, gpu=gpu, seed=1)
    model.eval()
    data, pool, cols = oc.make_tables(case, 14, 20, seed=5)
    cfg = dict(topK=3, used_col_indices=cols, label_wise=False)
    n_ids = pool.shape[1] - 1
    unused = [c for c in range(n_ids) if c not in cols][0]
    for other in (OnlineScorer(model, pool, cfg, graph=False, lib=lib), OnlineScorer(model, pool, cfg, graph=False, lib=lib, capacity=17)):
        for obj in (other, other.index):
            with pytest.raises(ValueError, match="window"):
                obj.delete_where(cols[:1], [[1]])
    scorer = OnlineScorer(model, pool, cfg, graph=False, lib=lib, capacity=17, window=True)
    scorer.append(data[:5])                                                # 14 + 5 > 17: two rows leave, head = 2
    ids = np.ascontiguousarray(data[:4, :-1])
    state = lambda: [t.clone() for t in (scorer.index.db_t, scorer.index.count, scorer.pool_ids, scorer.pool_labels,   # noqa: E731
                                         scorer.index.table_ids, scorer.index.table_idf, scorer.index.table_offsets)]
    host = lambda: (scorer.index._ring.copy(), scorer.index._head, scorer.index.n_db,                                # noqa: E731
                    [(v.copy(), c.copy()) for v, c in scorer.index._counts])
    before, host_before, y_before = state(), host(), scorer.score(ids)
    assert before[1].cpu().tolist() == [17, 2]

    def unchanged(score=False):
        assert all(torch.equal(a, b) for a, b in zip(before, state()))
        now = host()
        assert np.array_equal(now[0], host_before[0]) and now[1:3] == host_before[1:3]
        assert all(np.array_equal(a, c) and np.array_equal(b, d) for (a, b), (c, d) in zip(now[3], host_before[3]))
        if score:                                                          # every buffer a request reads is unchanged: so is its answer
            assert torch.equal(scorer.score(ids), y_before)

    c0 = cols[0]
    key_calls = [("find", ()), ("relabel_where", (1.0,)), ("delete_where", ())]
    refused = [([n_ids], [[1]], "column"), ([-1], [[1]], "column"), ([c0, c0], [[1, 1]], "repeated"), ([], np.zeros((1, 0), dtype=np.int64), "1 to 32"),
               (list(range(33)), np.zeros((1, 33), dtype=np.int64), "1 to 32"), ([c0], np.zeros((0, 1), dtype=np.int64), "non-empty"),
               ([c0], [[1, 2]], "wide"), ([c0, cols[1]], [[1]], "wide"), ([c0], [1, 2], "M, C"), ([c0], [[1.0]], "integer"),
               ([c0], torch.tensor([[0.5]], device=device), "integer"), ([c0], np.array([[True]]), "integer"), ([float(c0)], [[1]], "integer"),
               ([c0], [[2 ** 31]], "int32"), ([c0], np.array([[-2 ** 31 - 1]]), "int32"), ([[c0]], [[1]], "1-D")]
    for cc, keys, word in refused:
        for name, extra in key_calls:
            with pytest.raises(ValueError, match=word):
                getattr(scorer, name)(cc, keys, *extra)
        for name in ("find", "delete_where"):
            with pytest.raises(ValueError, match=word):
                getattr(scorer.index, name)(cc, keys)
        unchanged()
    with pytest.raises(ValueError, match="used column"):                   # the bare index holds its used columns only
        scorer.index.find([unused], [[1]])
    with pytest.raises(ValueError, match="used column"):
        scorer.index.delete_where([c0, unused], [[1, 1]])
    with pytest.raises(ValueError, match="one label"):
        scorer.relabel_where([c0], [[1]], [1.0, 0.0])
    unchanged(score=True)
    assert scorer._found is None                                           # nothing was allocated, nothing launched
    bad_lists = [([3, 5, 3], 1.0, "duplicate"), ([17], 1.0, "outside"), ([-1], 1.0, "outside"), (torch.tensor([2, -17]), 1.0, "outside"),
                 ([0.0, 1.0], 1.0, "integer"), (np.array([True, False]), 1.0, "integer"), (np.zeros((2, 2), dtype=np.int64), 1.0, "1-D"),
                 ([0, 1], [1.0, 0.0, 1.0], "labels"), ([0, 1, 2], [1.0], "labels"), ([0, 1], np.zeros((2, 1)), "labels")]
    if gpu >= 0:
        bad_lists += [(torch.tensor([1.0], device=device), 1.0, "integer"), (torch.zeros((2, 2), dtype=torch.int64, device=device), 1.0, "1-D"),
                      (torch.tensor([0, 1], device=device), [1.0, 0.0, 1.0], "labels")]
    for idx, labels, word in bad_lists:
        with pytest.raises(ValueError, match=word):
            scorer.set_labels(idx, labels)
        unchanged()
    # a key set that would empty the pool: delete's own refusal, nothing written; no match: 0, nothing written
    every = np.unique(scorer.pool_ids.cpu().numpy()[:, [c0]], axis=0)
    for obj in (scorer, scorer.index):
        with pytest.raises(ValueError, match="empty"):
            obj.delete_where([c0], every)
        assert obj.delete_where([c0], [[10 ** 6]]) == 0
    unchanged(score=True)
    assert scorer.index._scratch is None
    assert scorer.delete_where([c0], every[:1]) >= 1                       # and a good one goes through
    assert len(scorer.index) < 17 and scorer.index.count.cpu().tolist() == [len(scorer.index), 2]


# ---- 8. hostile headers and keys address nothing outside the buffers (host-emulation build only) ----------------------------------------------
def check_find_corrupt(lib, capacity=CAPACITY, guard=4096):
    """both entry points called with every buffer between guard regions: corrupt headers, unsorted and repeated keys, indices far
    outside — what the buffers then hold is unspecified, the guards are intact and the inputs are only read"""
    FILL = -99

    def guarded(numel, dtype, fill):
        whole = torch.full((numel + 2 * guard,), FILL, dtype=dtype)
        whole[guard:guard + numel] = fill
        return whole, whole[guard:guard + numel]

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    rs = np.random.RandomState(27)
    headers = [(capacity + 77, 5), (10 ** 12, 0), (-5, 0), (30, capacity), (30, capacity + 10 ** 9), (30, -3), (capacity + 1, capacity + 1),
               (-2 ** 62, 2 ** 62), (capacity, capacity - 1), (0, 0)]
    key_sets = [rs.randint(LO, HI, size=(40, 2)), np.array([[5, 5], [5, 5], [-3, 9], [5, 5]]), np.array([[9, 9], [8, 8], [7, 7], [-2 ** 31, 2 ** 31 - 1]]),
                np.full((17, 2), EVERYWHERE)]
    for field_major in (True, False):
        W = len(DB_COLS) if field_major else L
        strides = (1, capacity) if field_major else (L, 1)
        for form in (2, 1):
            for (n, head), keys in [(h, key_sets[i % 2]) for i, h in enumerate(headers)] + [(headers[0], k) for k in key_sets[1:]]:
                for groups, max_out in ((0, capacity), (3, 5)) + (((64, 0),) if keys is key_sets[3] else ()):
                    n_groups = groups or 1024
                    bufs = dict(store=guarded(W * capacity, torch.int32, EVERYWHERE), hdr=guarded(2, torch.int64, 0),
                                keys=guarded(keys.size, torch.int32, 0), cols=guarded(2, torch.int32, 0), out_idx=guarded(max_out, torch.int64, 5),
                                out_count=guarded(1, torch.int64, 5), ws=guarded(2 * n_groups + 1, torch.int64, 5))
                    bufs["store"][1][:] = torch.from_numpy(rs.randint(LO, HI, size=W * capacity).astype(np.int32))
                    bufs["hdr"][1][:] = torch.tensor([n, head])
                    bufs["keys"][1][:] = torch.from_numpy(keys.astype(np.int32).reshape(-1))
                    bufs["cols"][1][:] = torch.tensor([W - 1, 0], dtype=torch.int32)
                    read_only = {k: bufs[k][0].clone() for k in ("store", "hdr", "keys", "cols")}
                    lib.call("rat_pool_find", p(bufs["store"][1]), strides[0], strides[1], W, form, p(bufs["hdr"][1]), 0, capacity,
                             p(bufs["cols"][1]), 2, p(bufs["keys"][1]), len(keys), p(bufs["out_idx"][1]), max_out, p(bufs["out_count"][1]),
                             p(bufs["ws"][1]), (2 * n_groups + 1) * 8, groups, None)
                    for name, (whole, _) in bufs.items():
                        assert (whole[:guard] == FILL).all() and (whole[-guard:] == FILL).all(), (name, n, head, form, groups)
                    assert all(torch.equal(bufs[b][0], v) for b, v in read_only.items())
                    got, total = bufs["out_idx"][1].numpy(), int(bufs["out_count"][1])
                    assert 0 <= total <= capacity and ((got >= -1) & (got < capacity)).all()
    indices = [[0, 1, 2], [-1, capacity, 10 ** 12, -10 ** 12, 2 ** 62, -2 ** 63], list(range(capacity - 1, -1, -1)), [5, 5, 5]]
    for form in (2, 1):
        for n, head in headers:
            for k, idx in enumerate(indices):
                stride = k % 2                                                 # a label per index, one label for all: in turn
                bufs = dict(labels_pool=guarded(capacity, torch.float32, 4.0), hdr=guarded(2, torch.int64, 0),
                            idx=guarded(len(idx), torch.int64, 0), labels=guarded(len(idx) if stride else 1, torch.float32, 1.0))
                bufs["hdr"][1][:] = torch.tensor([n, head])
                bufs["idx"][1][:] = torch.tensor(idx)
                read_only = {k: bufs[k][0].clone() for k in ("hdr", "idx", "labels")}
                lib.call("rat_pool_set_labels", p(bufs["labels_pool"][1]), form, p(bufs["hdr"][1]), 0, capacity, p(bufs["idx"][1]),
                         p(bufs["labels"][1]), len(idx), stride, None)
                for name, (whole, _) in bufs.items():
                    assert (whole[:guard] == FILL).all() and (whole[-guard:] == FILL).all(), (name, n, head, form, idx)
                assert all(torch.equal(bufs[b][0], v) for b, v in read_only.items())
