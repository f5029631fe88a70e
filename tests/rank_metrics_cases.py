"""Checks of the ranking metrics on the device (``rat_eval_rank_metrics``; ``ops.eval_rank_metrics``, ``metrics.ndcg_score`` /
``mrr_score`` / ``hitrate_score``, the names ``NDCG(k=K)`` / ``MRR(k=K)`` / ``HitRate(k=K)`` in ``metrics.evaluate_metrics`` and
``device_metrics``, ``BaseModel(metrics=, group_id=)``, ``OnlineScorer.evaluate_rows(cutoffs=)`` / ``rank_metrics_rows``) shared by
tests/test_rank_metrics_device.py (CPU, host-emulation build) and tests/test_gpu_rank_metrics.py (MI355X).

The reference, never the code under test: ``reference`` below, a plain loop over the groups of the definitions in include/rat_hip.h
(order inside a group ``np.argsort(-p_g, kind="stable")``; a group counts if it holds a positive; DCG@k, IDCG@k, NDCG@k, MRR@k, HitRate@k
in float64), cross-checked on tie-free inputs against ``sklearn.metrics.ndcg_score(ignore_ties=True)`` (one-row groups apart: sklearn
refuses them and their NDCG is 1).  Gates: NDCG and MRR within 1e-12 absolute — every group's value is a quotient of sums of at most
n terms <= 1, each sum off by <= n ulp of its value whatever the order of summation, and the mean of G numbers in [0, 1] adds <= G ulp:
< 1e-12 up to n = 2^20 with room for the 1-ulp log2 of either side; HitRate, the group counts, the hits, k and the status exact
(``hits / counted`` is one division of two exact integers)."""
import ctypes
import os

import numpy as np
import torch

from metrics_cases import WILD, _device, _up, eval_batches, make_preds      # the generators of the metrics checks

GATE = 1e-12
GATE_SKLEARN = 1e-13                                    # two float64 evaluations of one formula: a few ulp per group, then a mean
NS_EMU = (2, 3, 63, 64, 65, 255, 256, 257, 1000, 4097)
K_MAX = 2 ** 31 - 1
SIZES = (1, 2, 3, 4, 5, 6, 9, 10, 11)                   # k - 1, k, k + 1 around the cutoffs 1, 2, 5, 10 (a group of 0 rows does not exist)
PARITY_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "metrics", "rank_parity.txt")

WORST = {}                                              # (where, metric) -> worst measured difference


def cutoffs_of(n):
    return (1, 2, 5, 10, n, K_MAX)


def note(where, metric, diff):
    key = (where, metric)
    WORST[key] = max(WORST.get(key, 0.0), float(diff))


def report():
    """prints the worst differences and rewrites this twin's lines of profiles/metrics/rank_parity.txt (the other twin's lines stay)"""
    lines = {}
    try:
        for line in open(PARITY_FILE):
            if line.startswith("worst |"):
                lines[line.split(" on the ")[1].split(":")[0] + line.split("|")[1]] = line.rstrip("\n")
    except OSError:
        pass
    for (where, metric), v in sorted(WORST.items()):
        line = "worst |%s - reference| on the %s: %.3g" % (metric, where, v)
        print(line)
        lines[where + "%s - reference" % metric] = line
    if not WORST:
        return
    head = ["tests/rank_metrics_cases.py — rat_eval_rank_metrics against the per-group numpy loop of the definitions (gate: %g absolute;" % GATE,
            "HitRate, the group counts, the hits, k and the status are compared bit for bit).  Written by report() at the end of",
            "tests/test_rank_metrics_device.py (emulator) and tests/test_gpu_rank_metrics.py (GPU); each rewrites its own lines.", ""]
    try:
        with open(PARITY_FILE, "w") as f:
            f.write("\n".join(head + [lines[k] for k in sorted(lines)]) + "\n")
    except OSError:
        pass                                             # a read-only checkout: the lines were printed


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def make_groups(kind, n, rs):
    if kind == "one":
        return np.full(n, 41, dtype=np.int32)
    if kind == "distinct":                               # n groups of one row
        return (rs.permutation(n).astype(np.int64) * 3 - n).astype(np.int32)
    if kind == "wild":                                   # ids 0, -7, the int32 limits
        return WILD[rs.randint(0, len(WILD), size=n)]
    if kind == "n10":
        return (rs.randint(0, max(1, n // 10), size=n).astype(np.int64) * 7 - 3).astype(np.int32)
    if kind in ("sized", "mix"):                         # consecutive blocks of the sizes in SIZES, then scattered over the rows
        sizes = []
        while sum(sizes) < n:
            sizes.append(SIZES[len(sizes) % len(SIZES)])
        g = np.repeat(np.arange(len(sizes), dtype=np.int64) * 11 - 5, sizes)[:n].astype(np.int32)
        return g[rs.permutation(n)]
    return (rs.randint(0, int(kind), size=n).astype(np.int64) * 1000003 - 17).astype(np.int32)


def make_case(pk, gk, n, rs):
    """-> (p fp32 [n], y fp32 [n], g int32 [n]) with at least one positive, asserted.  "mix": the groups cycle through no positive
    (skipped, still seen), all positives (NDCG 1) and exactly one positive in the last place"""
    p, g = make_preds(pk, n, rs), make_groups(gk, n, rs)
    if gk != "mix":
        y = (rs.rand(n) < 0.3).astype(np.float32)
        y[rs.randint(0, n)] = 1.0
    else:
        y = np.zeros(n, dtype=np.float32)
        kinds = [0, 0, 0]
        ids = np.unique(g)
        for j, u in enumerate(ids):
            rows = np.flatnonzero(g == u)
            kind = 2 if len(ids) < 3 else j % 3
            kinds[kind] += 1
            if kind == 1:
                y[rows] = 1.0
            elif kind == 2:
                y[rows[np.argsort(-p[rows].astype(np.float64), kind="stable")[-1]]] = 1.0
        assert n < 63 or min(kinds) >= 1, "the mix case does not mix: the case is wrong, not the gate"
    assert (y == 1).any(), "a parity input without a positive: the case is wrong, not the gate"
    return p, y, g


# ---- the reference: a plain loop over the groups ------------------------------------------------------------------------------------------
def reference(y, p, g, ks):
    """-> dict(ndcg [m], mrr [m], hits [m], counted, seen) over the groups in g, per cutoff in ks; float64 throughout"""
    y, p64, g = np.asarray(y), np.asarray(p).astype(np.float64), np.asarray(g)
    n = len(y)
    ks = np.asarray(ks, dtype=np.int64)
    disc = 1.0 / np.log2(np.arange(n) + 2.0)             # the discount of place r
    ideal = np.cumsum(disc)                              # ideal[j - 1] = sum_{i < j} disc[i]
    order = np.argsort(g, kind="stable")                 # the groups' rows, each group's in input order
    bounds = np.flatnonzero(np.concatenate([[True], g[order][1:] != g[order][:-1], [True]]))
    ndcg, rr, hit, seen = [], [], [], 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        rows = order[a:b]
        seen += 1
        ranked = rows[np.argsort(-p64[rows], kind="stable")]
        places = np.flatnonzero(y[ranked] == 1)          # the places of the group's positives, ascending
        if len(places) == 0:
            continue
        gain = np.cumsum(disc[places])
        within = np.searchsorted(places, ks)             # positives at a place < k
        dcg = np.where(within > 0, gain[np.maximum(within, 1) - 1], 0.0)
        idcg = ideal[np.minimum(len(places), ks) - 1]
        f = places[0]
        ndcg.append(dcg / idcg)
        rr.append(np.where(f < ks, 1.0 / (f + 1.0), 0.0))
        hit.append(f < ks)
    assert ndcg, "no group holds a positive"
    return dict(ndcg=np.mean(np.stack(ndcg), axis=0), mrr=np.mean(np.stack(rr), axis=0), hits=np.stack(hit).sum(axis=0),
                counted=len(ndcg), seen=seen)


def run(lib, device, y, p, g, ks):
    from rat_amd import ops
    out = ops.eval_rank_metrics(_up(p, device), _up(y, device), _up(g, device), ks, lib=lib)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(ks), 8) and out.device == torch.device(device)
    return out.cpu().numpy()


def compare(where, tag, out, ref, ks):
    for i, k in enumerate(ks):
        d_ndcg, d_mrr = abs(out[i, 0] - ref["ndcg"][i]), abs(out[i, 1] - ref["mrr"][i])
        note(where, "NDCG", d_ndcg)
        note(where, "MRR", d_mrr)
        print("%s k=%d: |NDCG - loop| = %.3g, |MRR - loop| = %.3g" % (tag, k, d_ndcg, d_mrr))
        assert d_ndcg <= GATE, (tag, k, out[i, 0], ref["ndcg"][i])
        assert d_mrr <= GATE, (tag, k, out[i, 1], ref["mrr"][i])
        hits = int(ref["hits"][i])
        want = (hits / float(ref["counted"]), ref["counted"], ref["seen"], hits, min(k, K_MAX), 0)
        assert tuple(out[i, 2:]) == want, (tag, k, out[i], want)                        # bitwise


# ---- 0. the loop against sklearn, on tie-free inputs (no library involved) ---------------------------------------------------------------------
def check_reference_against_sklearn():
    from sklearn.metrics import ndcg_score
    rs = np.random.RandomState(0)
    for n in (65, 1000, 4097):
        p = rs.permutation(n).astype(np.float32) / np.float32(n)                       # tie-free
        y = (rs.rand(n) < 0.3).astype(np.float32)
        g = rs.randint(0, max(2, n // 10), size=n).astype(np.int32)
        ks = (1, 3, 10, 10 ** 9)
        ref = reference(y, p, g, ks)
        for i, k in enumerate(ks):
            per = []
            for u in np.unique(g):
                m = g == u
                if not (y[m] == 1).any():
                    continue
                if m.sum() == 1:                         # sklearn refuses one-row lists; their NDCG is 1
                    per.append(1.0)
                    continue
                per.append(ndcg_score(y[m][None].astype(np.float64), p[m][None].astype(np.float64), k=min(k, int(m.sum())), ignore_ties=True))
            assert len(per) == ref["counted"]
            assert abs(np.mean(per) - ref["ndcg"][i]) <= GATE_SKLEARN, (n, k, np.mean(per), ref["ndcg"][i])


# ---- 1. parity at one n: every kind of prediction and of groups ---------------------------------------------------------------------------------
PLAN = (("continuous", "one"), ("continuous", "n10"), ("continuous", "mix"), ("continuous", 300), ("seven", "distinct"), ("seven", 5),
        ("seven", "sized"), ("seven", "wild"), ("equal", 300), ("equal", "mix"), ("equal", "sized"), ("edge", "wild"), ("edge", "n10"),
        ("edge", "one"))
PLAN_BIG = (("continuous", 300), ("seven", "n10"), ("edge", "wild"), ("equal", 5), ("continuous", "one"))


def check_parity(gpu, lib, n, big=False):
    device, where = _device(gpu), "emulator" if gpu < 0 else "GPU"
    rs = np.random.RandomState(2000 + n % 997)
    ks = cutoffs_of(n)
    for pk, gk in (PLAN_BIG if big else PLAN):
        p, y, g = make_case(pk, gk, n, rs)
        tag = "n=%d %s/%s" % (n, pk, gk)
        out = run(lib, device, y, p, g, ks)
        ref = reference(y, p, g, ks)
        compare(where, tag, out, ref, ks)
        if gk == "one":
            assert out[0, 3] == 1 and out[0, 4] == 1
        if gk == "distinct":                             # one-row groups: every counted group is a hit with NDCG 1
            assert (out[:, 0] == 1.0).all() and (out[:, 1] == 1.0).all() and (out[:, 2] == 1.0).all() and out[0, 4] == n
        assert (out[-1] == out[-2])[[0, 1, 2, 3, 4, 5, 7]].all(), (tag, "k = n and k = 2^31 - 1 both mean no cutoff")


# ---- 2. one call with eight cutoffs against eight calls with one: bitwise per row ----------------------------------------------------------------
def check_eight_cutoffs(gpu, lib, n):
    device = _device(gpu)
    rs = np.random.RandomState(11 + n % 991)
    ks = cutoffs_of(n) + (3, 50)
    assert len(ks) == 8
    for pk, gk in (("seven", "n10"), ("continuous", "sized")):
        p, y, g = make_case(pk, gk, n, rs)
        many = run(lib, device, y, p, g, ks)
        for i, k in enumerate(ks):
            single = run(lib, device, y, p, g, (k,))
            assert single[0].tobytes() == many[i].tobytes(), (n, pk, gk, k, single[0], many[i])
        assert run(lib, device, y, p, g, ks).tobytes() == many.tobytes()               # and the same call twice: bit for bit


# ---- 3. the tie rule ------------------------------------------------------------------------------------------------------------------------
def check_tie_rule(gpu, lib, n):
    device, where = _device(gpu), "emulator" if gpu < 0 else "GPU"
    rs = np.random.RandomState(13 + n % 983)
    ks = cutoffs_of(n)
    # all predictions equal: the order inside a group IS the input order, so two input orders of the same rows score differently
    p = np.full(n, 0.3, dtype=np.float32)
    g = make_groups(5 if n >= 63 else "one", n, rs)
    y = np.zeros(n, dtype=np.float32)
    y[0] = 1.0                                           # one positive: first of its group in one order, last in the other
    y[1:][rs.rand(n - 1) < 0.2] = 1.0 if n >= 63 else 0.0
    back = np.arange(n)[::-1]
    ref_a, ref_b = reference(y, p, g, ks), reference(y[back], p[back], g[back], ks)
    assert not np.array_equal(ref_a["mrr"], ref_b["mrr"]) or not np.array_equal(ref_a["ndcg"], ref_b["ndcg"]), \
        "the two orders score the same: the case is wrong"
    compare(where, "n=%d ties, input order" % n, run(lib, device, y, p, g, ks), ref_a, ks)
    compare(where, "n=%d ties, reversed" % n, run(lib, device, y[back], p[back], g[back], ks), ref_b, ks)
    # tie-free predictions: a permutation of the rows changes nothing, bit for bit
    for gk in ("n10", "wild", "sized"):
        q = (rs.permutation(n).astype(np.float32) - np.float32(n // 2)) / np.float32(n)
        _p, y, g = make_case("continuous", gk, n, rs)
        a = run(lib, device, y, q, g, ks)
        perm = rs.permutation(n)
        b = run(lib, device, y[perm], q[perm], g[perm], ks)
        assert a.tobytes() == b.tobytes(), (n, gk, a, b)
        assert (a[:, 7] == 0).all()


# ---- 4. undefined metrics: NaN in the slots, the bit in the status, the reason in the ValueError of both implementations ---------------------------
def check_status(gpu, lib, n=257):
    import pytest
    from rat_amd import metrics
    device = _device(gpu)
    rs = np.random.RandomState(3)
    p, y, g = make_case("continuous", 5, n, rs)
    ks = (1, 10)
    names = ["NDCG(k=10)", "logloss", "HitRate(k=1)", "MRR(k=10)", "AUC", "NDCG(k=1)"]

    def wrapped(y_, p_, g_, which=names):
        return metrics.device_metrics(_up(y_, device), _up(p_, device), which, group_index=_up(g_, device), lib=lib)

    def hosted(y_, p_, g_, which=names):
        return metrics.evaluate_metrics(y_, p_, which, group_index=g_)

    ref = reference(y, p, g, ks)
    want = {"NDCG(k=10)": ref["ndcg"][1], "HitRate(k=1)": ref["hits"][0] / float(ref["counted"]), "MRR(k=10)": ref["mrr"][1],
            "NDCG(k=1)": ref["ndcg"][0]}
    for got in (wrapped(y, p, g), hosted(y, p, g)):
        assert list(got) == names                        # the caller's order
        for name, v in want.items():
            assert abs(got[name] - v) <= GATE, (name, got[name], v)
        assert got["HitRate(k=1)"] == want["HitRate(k=1)"]
    assert wrapped(y, p, g)["AUC"] == hosted(y, p, g)["AUC"]
    # a cutoff past the C ABI's largest means "no cutoff" on both sides
    huge = "MRR(k=%d)" % (2 ** 40)
    assert abs(wrapped(y, p, g, [huge])[huge] - hosted(y, p, g, [huge])[huge]) <= GATE
    # no positive anywhere: bit 16
    none = np.zeros(n, dtype=np.float32)
    out = run(lib, device, none, p, g, ks)
    assert (out[:, 7] == 16).all() and np.isnan(out[:, :3]).all() and (out[:, 3] == 0).all() and (out[:, 4] == 5).all()
    assert (out[:, 5] == 0).all() and tuple(out[:, 6]) == ks
    # a 0.5 label: bit 2
    soft = y.copy()
    soft[n // 2] = 0.5
    out = run(lib, device, soft, p, g, ks)
    assert (out[:, 7].astype(np.int64) & 2).all() and np.isnan(out[:, :3]).all()
    # a NaN prediction: bit 1
    bad = p.copy()
    bad[n - 1] = np.nan
    out = run(lib, device, y, bad, g, ks)
    assert (out[:, 7].astype(np.int64) & 1).all() and np.isnan(out[:, :3]).all()
    for call in (wrapped, hosted):
        with pytest.raises(ValueError, match="No group holds a positive"):
            call(none, p, g, ["MRR(k=10)"])
        with pytest.raises(ValueError, match="neither 0 nor 1"):
            call(soft, p, g, ["NDCG(k=1)"])
        with pytest.raises(ValueError, match="NaN"):
            call(y, bad, g, ["HitRate(k=1)"])
    for fn in (metrics.ndcg_score, metrics.mrr_score, metrics.hitrate_score):
        with pytest.raises(ValueError, match="No group holds a positive"):
            fn(none, p, g, 10)
        with pytest.raises(ValueError, match="positive integer"):
            fn(y, p, g, 0)
    # bare names, names that are no names, grouped names without groups
    for which, gi in ((["NDCG"], g), (["MRR"], g), (["HitRate"], g), (["NDCG(k=0)"], g), (["NDCG(k=-1)"], g), (["NDCG(k=3)"], None),
                      (["MRR(k=3)"], None), (["HitRate(k=3)"], None)):
        with pytest.raises(NotImplementedError):
            wrapped(y, p, gi, which)
        with pytest.raises(NotImplementedError):
            hosted(y, p, gi, which)
    # ops refuses what the C ABI would, with words of its own
    from rat_amd import ops
    tp, ty, tg = _up(p, device), _up(y, device), _up(g, device)
    for ks_bad in ((), tuple(range(1, 10)), (0,), (2 ** 31,), (1.0,), (True,)):
        with pytest.raises(ValueError):
            ops.eval_rank_metrics(tp, ty, tg, ks_bad, lib=lib)
    with pytest.raises(ValueError):
        ops.eval_rank_metrics(tp, ty, None, (1,), lib=lib)
    with pytest.raises(ValueError):
        ops.eval_rank_metrics(tp, ty[:-1], tg, (1,), lib=lib)
    with pytest.raises(TypeError):
        ops.eval_rank_metrics(tp, ty, tg.to(torch.int64), (1,), lib=lib)


# ---- 5. the host functions against the loop ----------------------------------------------------------------------------------------------------
def check_host_functions():
    from rat_amd import metrics
    rs = np.random.RandomState(17)
    for n in (2, 65, 1000, 4097):
        ks = cutoffs_of(n)
        for pk, gk in PLAN:
            p, y, g = make_case(pk, gk, n, rs)
            ref = reference(y, p, g, ks)
            for i, k in enumerate(ks):
                tag = (n, pk, gk, k)
                assert abs(metrics.ndcg_score(y, p, g, k) - ref["ndcg"][i]) <= GATE, tag
                assert abs(metrics.mrr_score(y, p, g, k) - ref["mrr"][i]) <= GATE, tag
                assert metrics.hitrate_score(y, p, g, k) == ref["hits"][i] / float(ref["counted"]), tag


# ---- 6. the C ABI refuses, and launches nothing ---------------------------------------------------------------------------------------------
def check_abi_refusals(gpu, lib, n=300):
    device = _device(gpu)
    rs = np.random.RandomState(5)
    p, y, g = (_up(a, device) for a in make_case("continuous", 5, n, rs))
    fn = lib.cdll.rat_eval_rank_metrics
    m = 3
    ks = (ctypes.c_int32 * 8)(1, 5, 10, 1, 1, 1, 1, 1)
    zero = (ctypes.c_int32 * 8)(1, 0, 10, 1, 1, 1, 1, 1)
    minus = (ctypes.c_int32 * 8)(1, 5, -3, 1, 1, 1, 1, 1)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def host(a):
        return ctypes.cast(a, ctypes.c_void_p)

    nbytes = lib.size("rat_eval_rank_metrics_workspace", n, m)
    assert nbytes > 0
    raw = torch.zeros(nbytes // 8 + 64, dtype=torch.int64, device=device)
    ws = raw[(-raw.data_ptr() % 256) // 8:]
    out = torch.full((8, 8), -77.0, dtype=torch.float64, device=device)
    good = [ptr(p), ptr(y), ptr(g), n, host(ks), m, ptr(out), ptr(ws), nbytes, None]

    def but(**kw):
        args = list(good)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return args

    bad = [(but(a8=nbytes - 1), "workspace too small"), (but(a7=ctypes.c_void_p(ws.data_ptr() + 8)), "aligned"),
           (but(a3=0), "n must be"), (but(a3=-1), "n must be"), (but(a3=2 ** 31), "n must be"),
           (but(a5=0), "n_cutoffs must be"), (but(a5=9), "n_cutoffs must be"), (but(a5=-1), "n_cutoffs must be"),
           (but(a4=host(zero)), "cutoff"), (but(a4=host(minus)), "cutoff"),
           (but(a0=None), "null pointer"), (but(a1=None), "null pointer"), (but(a2=None), "null pointer"), (but(a4=None), "null pointer"),
           (but(a6=None), "null pointer"), (but(a7=None), "null pointer")]
    for args, word in bad:
        assert fn(*args) != 0, word
        assert word in lib.last_error(), (word, lib.last_error())
    if gpu >= 0:
        torch.cuda.synchronize()
    assert (out.cpu() == -77.0).all() and int(raw.cpu().abs().sum()) == 0, "a refused call wrote something"
    assert fn(*good) == 0, lib.last_error()              # and the good call goes through
    if gpu >= 0:
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[m:] == -77.0).all() and tuple(got[:m, 6]) == (1, 5, 10) and (got[:m, 7] == 0).all() and (got[:m, 4] == 5).all()


# ---- 7. memory safety (emulator): guard regions around out and the workspace, hostile group ids and labels, a full cutoff list ---------------------
def check_guards(lib, guard=4096):
    FILL = 0x5A
    rs = np.random.RandomState(9)
    for n in (1, 2, 255, 1025, 4097):
        p = rs.rand(n).astype(np.float32)
        y = rs.choice(np.array([0.0, 1.0, 0.5, -3.0, np.inf, -np.inf, np.nan, 1e30, 2.0], dtype=np.float32), size=n)
        g = rs.choice(np.array([0, -1, 2 ** 31 - 1, -2 ** 31, 10 ** 9, -7], dtype=np.int64), size=n).astype(np.int32)
        p[rs.randint(0, n)] = np.nan
        cut = (1, 2, 5, 10, n, K_MAX, 3, 1024)
        ks = (ctypes.c_int32 * 8)(*cut)
        nbytes = lib.size("rat_eval_rank_metrics_workspace", n, 8)
        raw = torch.full((nbytes + 2 * guard + 256,), FILL, dtype=torch.uint8)
        off = guard + (-(raw.data_ptr() + guard) % 256)
        out_raw = torch.full((8 * 64 + 2 * guard,), FILL, dtype=torch.uint8)
        out_off = guard + (-(out_raw.data_ptr() + guard) % 8)
        tp, ty, tg = torch.from_numpy(p.copy()), torch.from_numpy(y.copy()), torch.from_numpy(g.copy())
        rc = lib.cdll.rat_eval_rank_metrics(ctypes.c_void_p(tp.data_ptr()), ctypes.c_void_p(ty.data_ptr()), ctypes.c_void_p(tg.data_ptr()), n,
                                            ctypes.cast(ks, ctypes.c_void_p), 8, ctypes.c_void_p(out_raw.data_ptr() + out_off),
                                            ctypes.c_void_p(raw.data_ptr() + off), nbytes, None)
        assert rc == 0, lib.last_error()
        assert (raw[:off] == FILL).all() and (raw[off + nbytes:] == FILL).all(), n
        assert (out_raw[:out_off] == FILL).all() and (out_raw[out_off + 8 * 64:] == FILL).all(), n
        assert tp.numpy().tobytes() == p.tobytes() and ty.numpy().tobytes() == y.tobytes() and tg.numpy().tobytes() == g.tobytes()
        assert tuple(ks) == cut
        out = out_raw[out_off:out_off + 8 * 64].numpy().view(np.float64).reshape(8, 8)
        assert (out[:, 7].astype(np.int64) & 1).all(), (n, out)                       # the NaN prediction
        assert tuple(out[:, 6]) == cut and (out[:, 4] == len(np.unique(g))).all() and np.isnan(out[:, :3]).all()


# ---- 8. objects: OnlineScorer.evaluate_rows(cutoffs=) / rank_metrics_rows ------------------------------------------------------------------------
def check_scorer(gpu, lib, form, n=300, rows=np.arange(40, 200, 2)):
    import pytest
    import online_rows_cases as rc
    device, where = _device(gpu), "emulator" if gpu < 0 else "GPU"
    case, model, cfg, scorer, live, data, cols = rc._setup_scorer(gpu, lib, form, n)
    col = int(cols[0])
    ks = (1, 3)
    labels = live[rows, -1].astype(np.float32)
    g = live[rows, col].astype(np.int32)
    y = scorer.score_rows(rows).cpu().numpy()
    ref = reference(labels, y, g, ks)
    assert ref["counted"] >= 2 and ref["seen"] >= 2, "the rows' first retrieval column does not group them usefully"
    names = ["logloss", "AUC", "GAUC"] + ["%s(k=%d)" % (kind, k) for k in ks for kind in ("NDCG", "MRR", "HitRate")]
    today = scorer.evaluate_rows(rows, group=col)
    for device_side in (False, True):
        got = scorer.evaluate_rows(rows, group=col, device=device_side, cutoffs=ks)
        assert list(got) == names
        for i, k in enumerate(ks):
            assert abs(got["NDCG(k=%d)" % k] - ref["ndcg"][i]) <= GATE and abs(got["MRR(k=%d)" % k] - ref["mrr"][i]) <= GATE, (device_side, got)
            assert got["HitRate(k=%d)" % k] == ref["hits"][i] / float(ref["counted"])
            note(where, "NDCG", abs(got["NDCG(k=%d)" % k] - ref["ndcg"][i]))
            note(where, "MRR", abs(got["MRR(k=%d)" % k] - ref["mrr"][i]))
        assert got["AUC"] == today["AUC"]
        assert scorer.evaluate_rows(rows, group=col, device=device_side, cutoffs=()) == scorer.evaluate_rows(rows, group=col, device=device_side)
    # rank_metrics_rows: the raw tensor, still on the device, nothing copied to the host on the way
    idx = _up(rows.astype(np.int64), device)
    copies = []
    methods = ("cpu", "item", "tolist", "numpy")
    own = {name: torch.Tensor.__dict__.get(name) for name in methods}
    for name in methods:
        fn = getattr(torch.Tensor, name)
        setattr(torch.Tensor, name, lambda self, *a, _fn=fn, _name=name, **k: copies.append(_name) or _fn(self, *a, **k))
    try:
        raw = scorer.rank_metrics_rows(idx, ks, group=col)
    finally:
        for name in methods:
            if own[name] is None:
                delattr(torch.Tensor, name)
            else:
                setattr(torch.Tensor, name, own[name])
    # (on the CPU a "device" index list is a host tensor and is validated through numpy like any host list)
    assert copies == [] or gpu < 0, copies
    assert raw.dtype == torch.float64 and tuple(raw.shape) == (len(ks), 8) and raw.device == torch.device(device)
    compare(where, "rank_metrics_rows %s" % form, raw.cpu().numpy(), ref, ks)
    # same= composes: the restricted neighbours change the predictions, the metric chain is the same
    same = scorer.evaluate_rows(rows, same=[cols[0]], group=col, device=True, cutoffs=ks)
    assert same == pytest.approx(scorer.evaluate_rows(rows, same=[cols[0]], group=col, cutoffs=ks), abs=GATE)
    # refusals
    for call in (lambda: scorer.evaluate_rows(rows, cutoffs=ks), lambda: scorer.evaluate_rows(rows, device=True, cutoffs=ks),
                 lambda: scorer.rank_metrics_rows(rows, ks), lambda: scorer.rank_metrics_rows(rows, ks, group=None)):
        with pytest.raises(ValueError, match="group"):
            call()
    for bad in ((0,), (1.5,), (True,), (-2,)):
        with pytest.raises(ValueError, match="cutoff"):
            scorer.evaluate_rows(rows, group=col, cutoffs=bad)
        with pytest.raises(ValueError, match="cutoff"):
            scorer.rank_metrics_rows(rows, bad, group=col)


# ---- 9. objects: BaseModel.evaluate_generator ------------------------------------------------------------------------------------------------
CASE = "tiny_seq_bn"
GROUP_ID = "b"                                           # a plain categorical field (5 ids: column 1)
NAMES = ["AUC", "NDCG(k=3)", "MRR(k=3)", "HitRate(k=3)"]


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
    base = plain.evaluate_generator(batches)
    y_pred = plain.predict_generator(batches).astype(np.float32)
    y_true = np.concatenate([b[1][:, 0].numpy() for b in batches]).astype(np.float32)
    group = np.concatenate([b[0][:, 0, col].numpy() for b in batches]).astype(np.int32)
    ref = reference(y_true, y_pred, group, (3,))
    assert ref["counted"] >= 2
    for device_metrics in (False, True):
        model = build(device_metrics=device_metrics, metrics=NAMES, group_id=GROUP_ID)
        for name, source in (("host 4-tuples", batches), ("DeviceBatches", [DeviceBatch(*model._prepare_batch(b)) for b in batches])):
            got = model.evaluate_generator(source)
            tag = (device_metrics, name, got, ref)
            assert list(got) == NAMES and got["AUC"] == base["AUC"], tag
            assert abs(got["NDCG(k=3)"] - ref["ndcg"][0]) <= GATE and abs(got["MRR(k=3)"] - ref["mrr"][0]) <= GATE, tag
            assert got["HitRate(k=3)"] == ref["hits"][0] / float(ref["counted"]), tag
            note(where, "NDCG", abs(got["NDCG(k=3)"] - ref["ndcg"][0]))
            note(where, "MRR", abs(got["MRR(k=3)"] - ref["mrr"][0]))


def check_construction_refusals(gpu, lib):
    import pytest
    import golden_cases as gc
    import model_cases as mc
    case = gc.case_by_name(CASE)
    for name in ("NDCG(k=3)", "MRR(k=10)", "HitRate(k=1)"):
        for kw in (dict(), dict(device_metrics=True)):
            with pytest.raises(ValueError, match="no group_id"):
                mc.build_model(case, gpu=gpu, seed=1, metrics=["AUC", name], **kw)
    for name in ("NDCG", "MRR", "HitRate"):              # the bare names stay outside the contract: refused when they are evaluated
        model = mc.build_model(case, gpu=gpu, seed=1, metrics=["AUC", name], group_id=GROUP_ID)
        mc.load_weights(model, case)
        with pytest.raises(NotImplementedError):
            model.evaluate_generator(eval_batches(case, sizes=(4,)))
