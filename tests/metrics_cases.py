"""Checks of the evaluation metrics on the device (``rat_eval_metrics``; ``ops.eval_metrics``, ``metrics.device_metrics``,
``BaseModel(device_metrics=, group_id=)``, ``OnlineScorer.evaluate_rows(group=, device=)`` / ``metrics_rows``) shared by
tests/test_metrics_device.py (CPU, host-emulation build) and tests/test_gpu_metrics.py (MI355X).

References, never the code under test: ``rat_amd.metrics.auc_score`` and ``log_loss`` (pinned to sklearn by tests/test_host_side.py) and
``sklearn.metrics.roc_auc_score`` per group with the weighting done here in numpy.  Gates: AUC bitwise equal to ``auc_score`` (both
divide the same exact integers once); GAUC within 1e-12 absolute (per-group values are exact, only the order of a weighted mean of
numbers in [0, 1] differs); logloss within 1e-12 absolute (two logs of <= 1 ulp on terms <= 16.2 give <= 7.2e-15 per term, tree
summation adds < 1e-13 at n <= 2^20); the counts exact."""
import ctypes

import numpy as np
import torch

GATE_GAUC = 1e-12
GATE_LOGLOSS = 1e-12
NS_EMU = (2, 3, 63, 64, 65, 255, 256, 257, 1000, 4097)
PREDS = ("continuous", "seven", "equal", "edge")
LABELS = ("balanced", "one_pos", "one_neg")
GROUPS = (None, "one", 5, 300, "wild", "mix")          # ("distinct": every group of size one, in check_status)
EDGE = np.array([0.0, -0.0, 1.0, 1e-9, np.nextafter(np.float32(1), np.float32(0)), 1e-45, -0.25, 3.5], dtype=np.float32)
WILD = np.array([0, -7, 2 ** 31 - 1, -2 ** 31, 12345678, 5, -1, 1 << 30], dtype=np.int64).astype(np.int32)

WORST = {}                                              # (where, metric) -> worst measured difference, printed by the tests


def _device(gpu):
    return "cpu" if gpu < 0 else "cuda:%d" % gpu


def _up(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def note(where, metric, diff):
    key = (where, metric)
    WORST[key] = max(WORST.get(key, 0.0), float(diff))


def report():
    for (where, metric), v in sorted(WORST.items()):
        print("worst |%s - reference| on the %s: %.3g" % (metric, where, v))


def make_preds(kind, n, rs):
    if kind == "continuous":
        return rs.rand(n).astype(np.float32)
    if kind == "seven":
        return (rs.randint(0, 7, size=n) / np.float32(8)).astype(np.float32) + np.float32(0.0625)
    if kind == "equal":
        return np.full(n, 0.3, dtype=np.float32)
    assert kind == "edge"
    p = EDGE[rs.randint(0, len(EDGE), size=n)]
    p[:min(n, len(EDGE))] = rs.permutation(EDGE)[:min(n, len(EDGE))]
    return p


def make_labels(kind, n, rs):
    if kind == "balanced":
        y = (rs.rand(n) < 0.5).astype(np.float32)
        y[0], y[1] = 1.0, 0.0
        return y[rs.permutation(n)]
    y = np.full(n, 0.0 if kind == "one_pos" else 1.0, dtype=np.float32)
    y[rs.randint(0, n)] = 1.0 - y[0]
    return y


def make_groups(kind, n, rs, y=None):
    """-> int32 [n] or None.  "mix" rewrites nothing: it is built around the labels it is given (balanced ones) and asserts, from numpy,
    that at least one group is skipped and at least two are counted"""
    if kind is None:
        return None
    if kind == "one":
        return np.full(n, 41, dtype=np.int32)
    if kind == "distinct":
        return (rs.permutation(n).astype(np.int64) * 3 - n).astype(np.int32)
    if kind == "wild":
        return WILD[rs.randint(0, len(WILD), size=n)]
    if kind == "mix":
        assert y is not None and n >= 63
        g = rs.randint(0, max(3, n // 3), size=n).astype(np.int32) * 5 - 11
        pos, neg = np.flatnonzero(y == 1), np.flatnonzero(y == 0)
        g[pos[0]] = g[neg[0]] = 2 ** 31 - 2                    # two groups that surely hold both classes,
        g[pos[1]] = g[neg[1]] = -2 ** 31 + 1
        g[pos[2]] = 2 ** 31 - 3                                # and one that surely does not
        counted = skipped = 0
        for u in np.unique(g):
            s = float(y[g == u].sum())
            counted += 0 < s < (g == u).sum()
            skipped += not 0 < s < (g == u).sum()
        assert skipped >= 1 and counted >= 2, "the mix case does not mix: the case is wrong, not the gate"
        return g
    return (rs.randint(0, int(kind), size=n).astype(np.int64) * 1000003 - 17).astype(np.int32)


def reference(y, p, g):
    """-> dict(logloss, AUC or None, GAUC or None, n_pos, n_neg, groups, rows) from auc_score / log_loss and sklearn per group"""
    from sklearn.metrics import roc_auc_score
    from rat_amd import metrics
    y64, p64 = y.astype(np.float64), p.astype(np.float64)
    n_pos = int((y == 1).sum())
    ref = dict(logloss=metrics.log_loss(y64, p64), n_pos=n_pos, n_neg=len(y) - n_pos, groups=0, rows=0, GAUC=None,
               AUC=metrics.auc_score(y64, p64) if 0 < n_pos < len(y) else None)
    if g is not None:
        order = np.argsort(g, kind="mergesort")
        bounds = np.flatnonzero(np.concatenate([[True], g[order][1:] != g[order][:-1], [True]]))
        num = 0.0
        for a, b in zip(bounds[:-1], bounds[1:]):
            rows = order[a:b]
            s = int((y[rows] == 1).sum())
            if 0 < s < b - a:
                num += (b - a) * roc_auc_score(y64[rows], p64[rows])
                ref["groups"] += 1
                ref["rows"] += b - a
        ref["GAUC"] = num / ref["rows"] if ref["rows"] else None
    return ref


def run(lib, device, y, p, g):
    from rat_amd import ops
    out = ops.eval_metrics(_up(p, device), _up(y, device), _up(g, device), lib=lib)
    assert out.dtype == torch.float64 and tuple(out.shape) == (8,) and out.device == torch.device(device)
    return out.cpu().numpy()


def compare(where, tag, out, ref, grouped):
    status = 0 if ref["AUC"] is not None else 4
    if grouped and ref["GAUC"] is None:
        status |= 8
    d = abs(out[0] - ref["logloss"])
    note(where, "logloss", d)
    print("%s: |logloss - log_loss| = %.3g" % (tag, d))
    assert d <= GATE_LOGLOSS, (tag, out[0], ref["logloss"])
    if ref["AUC"] is None:
        assert np.isnan(out[1]), tag
    else:
        assert out[1] == ref["AUC"], (tag, out[1], ref["AUC"])                        # bitwise
    if ref["GAUC"] is None or ref["AUC"] is None:
        assert np.isnan(out[2]), tag
    else:
        d = abs(out[2] - ref["GAUC"])
        note(where, "GAUC", d)
        print("%s: |GAUC - sklearn per group| = %.3g" % (tag, d))
        assert d <= GATE_GAUC, (tag, out[2], ref["GAUC"])
    assert (out[3], out[4], out[5], out[6], out[7]) == (ref["n_pos"], ref["n_neg"], ref["groups"], ref["rows"], status), (tag, out, ref)


# ---- 1. parity at one n: every kind of prediction, of labels and of groups, each pairing once -------------------------------------------------
PLAN = (("continuous", "balanced", None), ("continuous", "balanced", "mix"), ("continuous", "one_pos", 5), ("continuous", "one_neg", "wild"),
        ("seven", "balanced", 300), ("seven", "balanced", "wild"), ("seven", "one_pos", "one"), ("seven", "one_neg", None),
        ("equal", "balanced", "one"), ("equal", "one_pos", None), ("equal", "one_neg", 300),
        ("edge", "balanced", 5), ("edge", "balanced", None), ("edge", "one_pos", "wild"), ("edge", "one_neg", "mix"))
PLAN_BIG = (("continuous", "balanced", None), ("continuous", "balanced", 300), ("seven", "balanced", "one"), ("seven", "balanced", 5),
            ("edge", "balanced", "wild"))


def check_parity(gpu, lib, n, big=False):
    device, where = _device(gpu), "emulator" if gpu < 0 else "GPU"
    rs = np.random.RandomState(1000 + n % 997)
    for pk, lk, gk in (PLAN_BIG if big else PLAN):
        p, y = make_preds(pk, n, rs), make_labels(lk, n, rs)
        if gk == "mix" and (lk != "balanced" or n < 63):                             # (the mix needs three rows of either class)
            gk = 5
        g = make_groups(gk, n, rs, y)
        tag = "n=%d %s/%s/%s" % (n, pk, lk, gk)
        out = run(lib, device, y, p, g)
        ref = reference(y, p, g)
        compare(where, tag, out, ref, g is not None)
        if pk == "equal":
            assert out[1] == 0.5, tag
        if gk == "one":
            assert abs(out[2] - out[1]) <= 1e-15, (tag, out[2], out[1])
            assert out[5] == 1 and out[6] == n


# ---- 2. the order of the rows: [1..7] bitwise, logloss within its gate ------------------------------------------------------------------------
def check_row_order(gpu, lib, n):
    device = _device(gpu)
    rs = np.random.RandomState(7 + n % 991)
    for pk, gk in (("seven", 5), ("continuous", "wild"), ("edge", 300)):
        p, y = make_preds(pk, n, rs), make_labels("balanced", n, rs)
        g = make_groups(gk, n, rs, y)
        a = run(lib, device, y, p, g)
        perm = rs.permutation(n)
        b = run(lib, device, y[perm], p[perm], g[perm])
        assert a[1:].tobytes() == b[1:].tobytes(), (n, pk, gk, a, b)
        assert a[7] == 0 and not np.isnan(a[1])
        assert abs(a[0] - b[0]) <= GATE_LOGLOSS and abs(b[0] - reference(y, p, None)["logloss"]) <= GATE_LOGLOSS
        again = run(lib, device, y, p, g)                                            # and the same call twice: bit for bit
        assert a.tobytes() == again.tobytes()


# ---- 3. undefined metrics: NaN in the slot, the bit in the status, the reason in the wrapper's ValueError ----------------------------------------
def check_status(gpu, lib, n=257):
    import pytest
    from rat_amd import metrics
    device = _device(gpu)
    rs = np.random.RandomState(3)
    p = make_preds("continuous", n, rs)
    y = make_labels("balanced", n, rs)
    g = make_groups(5, n, rs)
    names = ["logloss", "AUC", "GAUC"]

    def wrapped(y_, p_, g_, which=names):
        return metrics.device_metrics(_up(y_, device), _up(p_, device), which, group_index=_up(g_, device), lib=lib)

    got = wrapped(y, p, g)
    ref = reference(y, p, g)
    assert list(got) == names and got["AUC"] == ref["AUC"] and abs(got["GAUC"] - ref["GAUC"]) <= GATE_GAUC
    assert abs(got["logloss"] - ref["logloss"]) <= GATE_LOGLOSS
    assert got["GAUC"] == pytest.approx(metrics.gauc_score(y, p, g), abs=GATE_GAUC)                 # the host version, same definition
    assert metrics.evaluate_metrics(y, p, names, group_index=g)["GAUC"] == metrics.gauc_score(y, p, g)
    # one class only: bit 4 (and, with groups, 8), NaN, auc_score's words
    for fill in (0.0, 1.0):
        one = np.full(n, fill, dtype=np.float32)
        out = run(lib, device, one, p, None)
        assert out[7] == 4 and np.isnan(out[1]) and np.isnan(out[2]) and abs(out[0] - reference(one, p, None)["logloss"]) <= GATE_LOGLOSS
        assert (out[3], out[4]) == ((n, 0) if fill else (0, n))
        out = run(lib, device, one, p, g)
        assert out[7] == 12 and np.isnan(out[1]) and np.isnan(out[2]) and out[5] == 0 and out[6] == 0
        with pytest.raises(ValueError, match="Only one class present in y_true. ROC AUC score is not defined in that case."):
            wrapped(one, p, None, ["AUC"])
        assert set(wrapped(one, p, None, ["logloss"])) == {"logloss"}               # logloss alone is defined
    # a 0.5 label: bit 2
    soft = y.copy()
    soft[n // 2] = 0.5
    out = run(lib, device, soft, p, g)
    assert int(out[7]) & 2 and np.isnan(out[1]) and np.isnan(out[2])
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        wrapped(soft, p, g)
    # a NaN prediction: bit 1
    bad = p.copy()
    bad[n - 1] = np.nan
    out = run(lib, device, y, bad, g)
    assert int(out[7]) & 1 and np.isnan(out[0]) and np.isnan(out[1]) and np.isnan(out[2])
    with pytest.raises(ValueError, match="NaN"):
        wrapped(y, bad, g)
    # every group of size one: bit 8 alone, AUC still there
    lone = make_groups("distinct", n, rs)
    out = run(lib, device, y, p, lone)
    assert out[7] == 8 and np.isnan(out[2]) and out[1] == ref["AUC"] and out[5] == 0 and out[6] == 0
    with pytest.raises(ValueError, match="No group holds both classes"):
        wrapped(y, p, lone)
    with pytest.raises(ValueError, match="No group holds both classes"):
        metrics.gauc_score(y, p, lone)
    assert set(wrapped(y, p, lone, ["AUC", "logloss"])) == {"AUC", "logloss"}
    # names outside the contract still raise as evaluate_metrics does
    for which, gi in ((["NDCG"], g), (["GAUC"], None)):
        with pytest.raises(NotImplementedError):
            wrapped(y, p, gi, which)
        with pytest.raises(NotImplementedError):
            metrics.evaluate_metrics(y, p, which, group_index=gi)


# ---- 4. the C ABI refuses, and launches nothing ---------------------------------------------------------------------------------------------
def check_abi_refusals(gpu, lib, n=300):
    device = _device(gpu)
    rs = np.random.RandomState(5)
    p, y, g = _up(make_preds("continuous", n, rs), device), _up(make_labels("balanced", n, rs), device), _up(make_groups(5, n, rs), device)
    fn = lib.cdll.rat_eval_metrics

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    for grouped in (0, 1):
        nbytes = lib.size("rat_eval_metrics_workspace", n, grouped)
        assert nbytes > 0 and lib.size("rat_eval_metrics_workspace", n, 1) > lib.size("rat_eval_metrics_workspace", n, 0)
        raw = torch.zeros(nbytes // 8 + 64, dtype=torch.int64, device=device)
        ws = raw[(-raw.data_ptr() % 256) // 8:]
        out = torch.full((8,), -77.0, dtype=torch.float64, device=device)
        gg = g if grouped else None
        bad = [((ptr(p), ptr(y), ptr(gg), n, ptr(out), ptr(ws), nbytes - 1, None), "workspace too small"),
               ((ptr(p), ptr(y), ptr(gg), n, ptr(out), ctypes.c_void_p(ws.data_ptr() + 8), nbytes, None), "aligned"),
               ((ptr(p), ptr(y), ptr(gg), 0, ptr(out), ptr(ws), nbytes, None), "n must be"),
               ((ptr(p), ptr(y), ptr(gg), -1, ptr(out), ptr(ws), nbytes, None), "n must be"),
               ((ptr(p), ptr(y), ptr(gg), 2 ** 31, ptr(out), ptr(ws), nbytes, None), "n must be"),
               ((None, ptr(y), ptr(gg), n, ptr(out), ptr(ws), nbytes, None), "null pointer"),
               ((ptr(p), None, ptr(gg), n, ptr(out), ptr(ws), nbytes, None), "null pointer"),
               ((ptr(p), ptr(y), ptr(gg), n, None, ptr(ws), nbytes, None), "null pointer"),
               ((ptr(p), ptr(y), ptr(gg), n, ptr(out), None, nbytes, None), "null pointer")]
        for args, word in bad:
            assert fn(*args) != 0, word
            assert word in lib.last_error(), (word, lib.last_error())
        if gpu >= 0:
            torch.cuda.synchronize()
        assert (out.cpu() == -77.0).all() and int(raw.cpu().abs().sum()) == 0, "a refused call wrote something"
        assert fn(ptr(p), ptr(y), ptr(gg), n, ptr(out), ptr(ws), nbytes, None) == 0             # and the good call goes through
        if gpu >= 0:
            torch.cuda.synchronize()
        assert out[3] + out[4] == n


# ---- 5. memory safety (emulator): guard regions around out and the workspace, hostile group ids and labels ------------------------------------
def check_guards(lib, guard=4096):
    FILL = 0x5A
    rs = np.random.RandomState(9)
    for n in (1, 2, 255, 1025, 4097):
        p = rs.rand(n).astype(np.float32)
        y = rs.choice(np.array([0.0, 1.0, 0.5, -3.0, np.inf, -np.inf, np.nan, 1e30, 2.0], dtype=np.float32), size=n)
        g = rs.choice(np.array([0, -1, 2 ** 31 - 1, -2 ** 31, 10 ** 9, -7], dtype=np.int64), size=n).astype(np.int32)
        p[rs.randint(0, n)] = np.nan
        for grouped in (0, 1):
            nbytes = lib.size("rat_eval_metrics_workspace", n, grouped)
            raw = torch.full((nbytes + 2 * guard + 256,), FILL, dtype=torch.uint8)
            off = guard + (-(raw.data_ptr() + guard) % 256)
            out_raw = torch.full((64 + 2 * guard,), FILL, dtype=torch.uint8)
            out_off = guard + (-(out_raw.data_ptr() + guard) % 8)
            tp, ty, tg = torch.from_numpy(p.copy()), torch.from_numpy(y.copy()), torch.from_numpy(g.copy())
            rc = lib.cdll.rat_eval_metrics(ctypes.c_void_p(tp.data_ptr()), ctypes.c_void_p(ty.data_ptr()),
                                           ctypes.c_void_p(tg.data_ptr()) if grouped else None, n,
                                           ctypes.c_void_p(out_raw.data_ptr() + out_off), ctypes.c_void_p(raw.data_ptr() + off), nbytes, None)
            assert rc == 0, lib.last_error()
            assert (raw[:off] == FILL).all() and (raw[off + nbytes:] == FILL).all(), (n, grouped)
            assert (out_raw[:out_off] == FILL).all() and (out_raw[out_off + 64:] == FILL).all(), (n, grouped)
            assert tp.numpy().tobytes() == p.tobytes() and ty.numpy().tobytes() == y.tobytes() and tg.numpy().tobytes() == g.tobytes()
            out = out_raw[out_off:out_off + 64].numpy().view(np.float64)
            assert int(out[7]) & 3 == 3 or n < 3, (n, out)                           # the NaN prediction, the labels outside {0, 1}
            assert out[3] == float((y == 1).sum()) and out[3] + out[4] == n


# ---- 6. objects: OnlineScorer.evaluate_rows / metrics_rows ------------------------------------------------------------------------------------
class _Spy:
    """wraps ops.eval_metrics as online_same_cases.check_refusals wraps its ops: counts the calls that reach it"""

    def __enter__(self):
        from rat_amd import ops
        self.ops, self.real, self.calls = ops, ops.eval_metrics, 0

        def spy(*a, **k):
            self.calls += 1
            return self.real(*a, **k)
        ops.eval_metrics = spy
        return self

    def __exit__(self, *exc):
        self.ops.eval_metrics = self.real


def check_scorer(gpu, lib, form, n=300, rows=np.arange(40, 200, 2)):
    import pytest
    import online_rows_cases as rc
    device, where = _device(gpu), "emulator" if gpu < 0 else "GPU"
    case, model, cfg, scorer, live, data, cols = rc._setup_scorer(gpu, lib, form, n)
    col = int(cols[0])
    labels = live[rows, -1].astype(np.float32)
    assert 0 < labels.sum() < len(rows)
    with _Spy() as spy:
        host = scorer.evaluate_rows(rows)
        assert spy.calls == 0, "the default evaluate_rows reached ops.eval_metrics"
        y = scorer.score_rows(rows).cpu().numpy()
        dev = scorer.evaluate_rows(rows, device=True)
        assert spy.calls == 1
        assert list(dev) == list(host) == ["logloss", "AUC"]
        assert dev["AUC"] == host["AUC"] and abs(dev["logloss"] - host["logloss"]) <= GATE_LOGLOSS, (dev, host)
        note(where, "logloss", abs(dev["logloss"] - host["logloss"]))
        g = live[rows, col].astype(np.int32)
        ref = reference(labels, y, g)
        assert ref["groups"] >= 2, "the rows' first retrieval column does not group them usefully"
        for device_side in (False, True):
            got = scorer.evaluate_rows(rows, group=col, device=device_side)
            assert list(got) == ["logloss", "AUC", "GAUC"]
            assert got["AUC"] == ref["AUC"] and abs(got["logloss"] - ref["logloss"]) <= GATE_LOGLOSS
            assert abs(got["GAUC"] - ref["GAUC"]) <= GATE_GAUC, (device_side, got, ref)
            note(where, "GAUC", abs(got["GAUC"] - ref["GAUC"]))
        assert spy.calls == 2
        # metrics_rows: the raw tensor, still on the device, nothing copied to the host on the way
        idx = _up(rows.astype(np.int64), device)
        copies = []
        names = ("cpu", "item", "tolist", "numpy")
        own = {name: torch.Tensor.__dict__.get(name) for name in names}
        for name in names:
            fn = getattr(torch.Tensor, name)
            setattr(torch.Tensor, name, lambda self, *a, _fn=fn, _name=name, **k: copies.append(_name) or _fn(self, *a, **k))
        try:
            raw = scorer.metrics_rows(idx, group=col)
            plain = scorer.metrics_rows(idx)
        finally:
            for name in names:
                if own[name] is None:
                    delattr(torch.Tensor, name)
                else:
                    setattr(torch.Tensor, name, own[name])
        # (on the CPU a "device" index list is a host tensor and is validated through numpy like any host list)
        assert copies == [] or gpu < 0, copies
        assert raw.dtype == torch.float64 and tuple(raw.shape) == (8,) and raw.device == torch.device(device)
        raw, plain = raw.cpu().numpy(), plain.cpu().numpy()
        compare(where, "metrics_rows %s" % form, raw, ref, True)
        assert np.isnan(plain[2]) and plain[1] == ref["AUC"] and plain[7] == 0 and plain[5] == 0
        assert spy.calls == 4
        # same= composes: the restricted neighbours change the predictions, the metric chain is the same
        same = scorer.evaluate_rows(rows, same=[cols[0]], group=col, device=True)
        assert same == pytest.approx(scorer.evaluate_rows(rows, same=[cols[0]], group=col), abs=GATE_GAUC)
        # refusals: nothing reaches the chain
        calls = spy.calls
        for bad in (-1, live.shape[1] - 1, 10 ** 6, 1.0, True, [col], "a"):
            for call in (lambda b: scorer.evaluate_rows(rows, group=b), lambda b: scorer.evaluate_rows(rows, group=b, device=True),
                         lambda b: scorer.metrics_rows(rows, group=b)):
                with pytest.raises(ValueError, match="id column"):
                    call(bad)
        assert spy.calls == calls


# ---- 7. objects: BaseModel.evaluate_generator ------------------------------------------------------------------------------------------------
CASE = "tiny_seq_bn"
GROUP_ID, SEQUENCE_ID = "b", "c"                         # a plain categorical field (5 ids: column 1), a sequence field


def eval_batches(case, sizes=(12, 7), seed=23):
    """host 4-tuples shaped like golden_cases.make_inputs, several batches, the last one ragged"""
    rs = np.random.RandomState(seed)
    t = case["topk"] + 1
    batches = []
    for b in sizes:
        cols = []
        for f in case["fields"]:
            v = f["vocab_size"]
            if f["type"] == "sequence":
                ids = rs.randint(0, v - 1, size=(b, t, f["max_len"]))
                ids[np.arange(f["max_len"])[None, None, :] >= rs.randint(0, f["max_len"] + 1, size=(b, t, 1))] = v - 1
            else:
                ids = rs.randint(0, v, size=(b, t, 1))
            cols.append(ids)
        X = np.concatenate(cols, axis=-1).astype(np.float64)
        y = rs.randint(0, 2, size=(b, t)).astype(np.float64)
        batches.append((torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(rs.rand(b, t - 1)),
                        torch.from_numpy(np.full((b,), t - 1, dtype=np.int64))))
    return batches


def check_generator(gpu, lib):
    import golden_cases as gc
    import model_cases as mc
    from rat_amd.data import DeviceBatch
    where = "emulator" if gpu < 0 else "GPU"
    case = gc.case_by_name(CASE)
    batches = eval_batches(case)

    def build(**kw):
        model = mc.build_model(case, gpu=gpu, seed=1, **kw)
        mc.load_weights(model, case)
        return model

    plain = build()
    col = plain._feature_map.feature_specs[GROUP_ID]["index"]
    with _Spy() as spy:
        base = plain.evaluate_generator(batches)
        assert spy.calls == 0, "a default model's evaluate_generator reached ops.eval_metrics"
        y_pred = plain.predict_generator(batches).astype(np.float32)
        y_true = np.concatenate([b[1][:, 0].numpy() for b in batches]).astype(np.float32)
        group = np.concatenate([b[0][:, 0, col].numpy() for b in batches]).astype(np.int32)
        ref = reference(y_true, y_pred, group)
        assert list(base) == ["AUC", "logloss"] and base["AUC"] == ref["AUC"] and ref["groups"] >= 2
        on_device = build(device_metrics=True)
        grouped = build(device_metrics=True, metrics=["AUC", "logloss", "GAUC"], group_id=GROUP_ID)
        grouped_host = build(metrics=["AUC", "logloss", "GAUC"], group_id=GROUP_ID)
        sources = {"host 4-tuples": lambda m: batches, "DeviceBatches": lambda m: [DeviceBatch(*m._prepare_batch(b)) for b in batches]}
        for name, source in sources.items():
            calls = spy.calls
            got = on_device.evaluate_generator(source(on_device))
            assert list(got) == ["AUC", "logloss"] and got["AUC"] == base["AUC"], (name, got, base)
            assert abs(got["logloss"] - base["logloss"]) <= GATE_LOGLOSS, (name, got, base)
            note(where, "logloss", abs(got["logloss"] - base["logloss"]))
            assert spy.calls == calls + 1
            got = grouped.evaluate_generator(source(grouped))
            assert list(got) == ["AUC", "logloss", "GAUC"] and got["AUC"] == base["AUC"], (name, got, base)
            assert abs(got["logloss"] - base["logloss"]) <= GATE_LOGLOSS and abs(got["GAUC"] - ref["GAUC"]) <= GATE_GAUC, (name, got, ref)
            note(where, "GAUC", abs(got["GAUC"] - ref["GAUC"]))
            assert spy.calls == calls + 2
            if name != "host 4-tuples":
                continue
            got = grouped_host.evaluate_generator(source(grouped_host))
            assert got["AUC"] == base["AUC"] and abs(got["logloss"] - base["logloss"]) <= GATE_LOGLOSS and abs(got["GAUC"] - ref["GAUC"]) <= GATE_GAUC
            assert spy.calls == calls + 2, "group_id without device_metrics reached ops.eval_metrics"


def check_construction_refusals(gpu, lib, monkeypatch):
    import pytest
    import golden_cases as gc
    import model_cases as mc
    from rat_amd.base_model import BaseModel
    case = gc.case_by_name(CASE)
    with pytest.raises(ValueError, match="sequence field"):
        mc.build_model(case, gpu=gpu, seed=1, group_id=SEQUENCE_ID)
    with pytest.raises(ValueError, match="not a feature"):
        mc.build_model(case, gpu=gpu, seed=1, group_id="nobody")
    with pytest.raises(ValueError, match="no group_id"):
        mc.build_model(case, gpu=gpu, seed=1, metrics=["AUC", "GAUC"])
    with pytest.raises(ValueError, match="no group_id"):
        mc.build_model(case, gpu=gpu, seed=1, metrics=["GAUC"], device_metrics=True)
    model = mc.build_model(case, gpu=gpu, seed=1, device_metrics=True, group_id=GROUP_ID)      # a good one goes through
    monkeypatch.setattr(BaseModel, "_dp", lambda self: True)
    for kw in (dict(device_metrics=True), dict(group_id=GROUP_ID)):
        with pytest.raises(ValueError, match="data parallelism"):
            mc.build_model(case, gpu=gpu, seed=1, **kw)
    with pytest.raises(ValueError, match="data parallelism"):                                  # a process group that came up later
        model.evaluate_generator(eval_batches(case, sizes=(4,)))
