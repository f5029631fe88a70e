"""Kernel-level parity cases of the prediction head (csrc/gemm.hip, csrc/head.hip), shared by tests/test_head_kernels.py (the kernel
sources through the host emulation) and tests/test_gpu_head_kernels.py (-m gpu, the MI355X): the GEMM in the forms model.py calls it,
the logit forward / backward through every entry point, and BatchNorm + the six activations on both kernel families.

Every reference is float64 (numpy or torch autograd) of the same operation on the same float32 inputs.  The gates are the ones the
existing checks use (kernel_cases.check_sgemm / check_logit / check_bn_relu / check_bn_strip, pooling_cases.check_pool_kernels); the
few that are new are derived where they are applied.  Conditions on the inputs (value bands, sizes of what must have happened) are
asserted on the reference alone.  Whatever a kernel must not read is NaN, whatever it must not write is a sentinel compared bit for
bit, and all of it lies inside the test's own allocations: no assertion depends on an access outside a buffer.

Every comparison records its margin (tests/margins.py); for the exact ones the recorded figure is the number of differing words."""
import collections

import numpy as np
import torch

import margins
from kernel_cases import close, rnd
from pooling_cases import Field
from rat_amd import ops
from rat_amd._lib import RatError

SENT = 12345.0
TAIL = 8                              # floats behind every embedded matrix, filled like the rest of its buffer
GUARD = 8                             # elements in front of and behind an LR table inside its buffer
TT = [(0, 1), (0, 0), (1, 0), (1, 1)]

ACT_FN = {"relu": torch.relu, "none": lambda t: t, "sigmoid": torch.sigmoid, "tanh": torch.tanh,
          "leakyrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.01), "elu": lambda t: torch.nn.functional.elu(t, 1.0)}
ACTS = list(ACT_FN)


# ----------------------------------------------------------------------------- helpers
def _t64(x):
    return (x.detach().cpu() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).double().reshape(-1)


def gated(test, workload, quantity, got, ref, rtol, atol, arith="f32", where=""):
    """|got - ref| <= atol + rtol |ref| element by element (numpy's assert_allclose rule, asserted by kernel_cases.close); the element
    closest to its gate goes to the margins file.  atol may be a tensor of the reference's shape."""
    g, r = _t64(got), _t64(ref)
    assert g.shape == r.shape, (test, quantity, g.shape, r.shape)
    assert bool(torch.isfinite(g).all()), "%s %s: non-finite %s (%s)" % (test, workload, quantity, where)
    a = _t64(atol) if (torch.is_tensor(atol) or isinstance(atol, np.ndarray)) else torch.full_like(r, float(atol))
    allowed = a + rtol * r.abs()
    err = (g - r).abs()
    k = int((err / (allowed + 1e-300)).argmax())
    margins.record(test, workload, quantity, float(err[k]), float(allowed[k]), arith=arith, where=where)
    if a.numel() and float(a.min()) == float(a.max()):
        close(g, r, rtol, float(a[0]), "%s %s %s (%s)" % (test, workload, quantity, where))
    assert float(err[k]) <= float(allowed[k]), "%s %s %s: |error| %.3g at element %d exceeds the gate %.3g (%s)" % (
        test, workload, quantity, float(err[k]), k, float(allowed[k]), where)


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def exact(test, workload, quantity, got, want, where=""):
    """the same shape, type and bits (a NaN that must survive compares equal, -0.0 does not pass for 0.0)"""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (test, workload, quantity, g.shape, g.dtype, w.shape, w.dtype)
    bad = int((g != w).sum())
    margins.record(test, workload, quantity, bad, 0, arith="exact", where=where)
    assert bad == 0, "%s %s %s: %d of %d words differ, the first at %d (%s)" % (
        test, workload, quantity, bad, g.size, int(np.flatnonzero((g != w).reshape(-1))[0]), where)


def relative(test, workload, quantity, a, b, gate, arith=None, where=""):
    """max |a - b| <= gate x max |b|: the form check_attn / check_ffn use for the two arithmetics side by side"""
    err = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)
    margins.record(test, workload, quantity, err, gate, arith=arith, where=where)
    assert err < gate, (test, workload, quantity, err, gate, where)


def embed(mat, pitch, off, fill):
    """-> (flat buffer filled with `fill`, [rows][cols] view of it with row pitch `pitch` starting `off` floats in, holding mat)"""
    rows, cols = mat.shape
    assert pitch >= cols or rows == 1
    buf = torch.full((off + rows * max(pitch, cols) + TAIL,), float(fill), dtype=torch.float32)
    view = buf.as_strided((rows, cols), (pitch, 1), off)
    view.copy_(mat)
    return buf, view


def on_device(buf, view, dev):
    b = buf.to(dev)
    assert b.data_ptr() % 16 == 0
    return b, b.as_strided(view.shape, view.stride(), view.storage_offset())


def outside(buf, view):
    """the elements of the flat buffer that are not part of the view"""
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    rows, cols = view.shape
    idx = (view.storage_offset() + torch.arange(rows).unsqueeze(1) * view.stride(0) + torch.arange(cols).unsqueeze(0)).reshape(-1)
    mask[idx] = False
    return mask


# ----------------------------------------------------------------------------- 1. GEMM in the product's call forms
# pitch kinds: "w" the row width itself, "q" wider and a multiple of 4, "o" wider and no multiple of 4
G = collections.namedtuple("G", "name ta tb M N K pitch off beta bias")


def _pitch(width, kind):
    return {"w": width, "q": (width + 3) // 4 * 4 + 4, "o": (width + 3) // 4 * 4 + 5}[kind] if isinstance(kind, str) else int(kind)


def gemm_geometry(c):
    """-> ((rows, cols), pitch) of A, B and C as stored"""
    sa = (c.K, c.M) if c.ta else (c.M, c.K)
    sb = (c.N, c.K) if c.tb else (c.K, c.N)
    sc = (c.M, c.N)
    return [(s, _pitch(s[1], k)) for s, k in zip((sa, sb, sc), c.pitch)]


def bf16x3_fallback_reasons(c):
    """the documented rule (include/rat_hip.h, rat_sgemm_arith): which of its conditions send RAT_ARITH_BF16X3 to the exact-fp32 kernel
    (buffers themselves are 16-byte aligned: on_device asserts it)"""
    (_, lda), (_, ldb), _ = gemm_geometry(c)
    why = set()
    if lda % 4:
        why.add("lda")
    if ldb % 4:
        why.add("ldb")
    if c.off[0] % 4:
        why.add("base A")
    if c.off[1] % 4:
        why.add("base B")
    if c.K < 64:
        why.add("K")
    if c.M < 16:
        why.add("M")
    if c.N < 16:
        why.add("N")
    return why


def _gemm_cases():
    core, rest = [], []
    for i, (ta, tb) in enumerate(TT):
        t = "t%d%d-" % (ta, tb)
        # pitch / offset: 72 x 40 x 100 = two row tiles, a partial column tile, a ragged last k tile
        v = [G(t + "dense-beta0", ta, tb, 72, 40, 100, "www", (0, 0, 0), 0.0, False),
             G(t + "pitch4-off4-beta1-bias", ta, tb, 72, 40, 100, "qqo", (4, 4, 1), 1.0, True),
             G(t + "A-pitch-odd", ta, tb, 72, 40, 100, "oqq", (0, 4, 0), 0.5, False),
             G(t + "B-pitch-odd", ta, tb, 72, 40, 100, "qoq", (4, 0, 2), 0.0, True),
             G(t + "A-off1", ta, tb, 72, 40, 100, "qqw", (1, 0, 0), 0.0, True),
             G(t + "B-off2", ta, tb, 72, 40, 100, "qqq", (0, 2, 4), 1.0, False),
             G(t + "K29", ta, tb, 70, 37, 29, "qqo", (0, 0, 0), 0.5, True),
             G(t + "M12", ta, tb, 12, 40, 100, "qqq", (4, 0, 0), 0.0, False),
             G(t + "N12", ta, tb, 70, 12, 100, "qqq", (0, 4, 0), 1.0, True),
             G(t + "one-tile", ta, tb, 64, 64, 64, "qqq", (0, 0, 0), 0.0, False),
             G(t + "one-past-a-tile", ta, tb, 65, 65, 65, "qqo", (4, 4, 1), 0.5, True)]
        # split-K with a ragged last k tile (pitches multiples of 4: the bf16x3 kernel runs), and M < 16 (it does not)
        s = [G(t + "splitk-17x16x515", ta, tb, 17, 16, 515, "qqo", (0, 4, 1), 0.5, True),
             G(t + "splitk-40x36x707", ta, tb, 40, 36, 707, "qqq", (4, 0, 0), 0.0, False),
             G(t + "splitk-70x130x263", ta, tb, 70, 130, 263, "qqo", (0, 0, 2), 1.0, True),
             G(t + "splitk-3x70x515", ta, tb, 3, 70, 515, "qqq", (0, 0, 0), 0.0, True)]
        # by default on the emulator: per (ta, tb) one shape bf16x3 takes and one it does not, the NaN-filled C, one ragged split-K;
        # the other members of each class rotate over the four (ta, tb)
        pick = {1, 4 + i % 2, 0 if i % 2 else 9, 10 if i % 2 else 6, 2 + i % 2, 7 + i % 2}
        mine = [c for j, c in enumerate(v) if j in pick] + [s[i % 3]] + ([s[3]] if i == 0 else [])
        core += mine
        rest += [c for c in v + s if c not in mine]
    # the literal product form (model.py: the first head layer and its weight gradient): grid [B][T][S][d], x0 = grid[:, 0, 1:, :]
    # with a row pitch of T S d, starting d floats into the allocation — 40 bytes at d = 10
    Bq, T, S, width = 70, 2, 4, 24
    for d in (10, 40, 64):
        fwd = G("product-forward-d%d" % d, 0, 1, Bq, width, (S - 1) * d, (T * S * d, "w", "w"), (d, 0, 0), 0.0, True)
        wgrad = G("product-weight-gradient-d%d" % d, 1, 0, width, (S - 1) * d, Bq, ("w", T * S * d, "w"), (0, d, 0), 0.0, False)
        (core if d in (10, 64) else rest).extend([fwd, wgrad])
    # the one-output Linear of the DNN (model.py: forward N = 1, weight gradient M = 1 with lda = 1, input gradient K = 1)
    core += [G("N1-ldc1", 0, 1, 70, 1, 40, "qww", (4, 0, 0), 0.0, True),
             G("M1-lda1", 1, 0, 1, 40, 70, "wqw", (0, 0, 0), 0.0, False),
             G("K1", 0, 0, 70, 40, 1, "wwq", (0, 0, 0), 0.0, False)]
    rest += [G("N1-ldc1-beta1", 0, 1, 70, 1, 100, "www", (0, 0, 0), 1.0, False),
             G("M1-lda1-beta.5", 1, 0, 1, 40, 515, "wqo", (0, 4, 1), 0.5, True),
             G("K1-beta1", 0, 0, 17, 70, 1, "wqo", (0, 0, 3), 1.0, True)]
    return core, rest


GEMM_CORE, GEMM_REST = _gemm_cases()
GEMM_ALL = GEMM_CORE + GEMM_REST
SPLITK_SHAPES = [(40, 36, 707), (17, 16, 515), (70, 130, 263), (3, 70, 515)]


def gemm_id(c):
    return c.name


def gemm_problem(c, seed=11):
    rs = np.random.RandomState(seed)
    (sa, lda), (sb, ldb), (sc, ldc) = gemm_geometry(c)
    A, Bm = rnd(rs, *sa), rnd(rs, *sb)
    C0 = rnd(rs, *sc) if c.beta != 0.0 else torch.full(sc, float("nan"))
    bias = rnd(rs, c.N) if c.bias else None
    ref = (A.t() if c.ta else A).double() @ (Bm.t() if c.tb else Bm).double()
    if bias is not None:
        ref = ref + bias.double()
    if c.beta != 0.0:
        ref = ref + c.beta * C0.double()
    return (A, lda), (Bm, ldb), (C0, ldc), bias, ref


def run_gemm(lib, dev, c, prob, call):
    """operands inside larger buffers (NaN around A and B, the sentinel around C); call(A, lda, B, ldb, C, ldc, bias) runs the product.
    -> the result [M][N] on the host, after checking that it is finite and that nothing around C changed"""
    (A, lda), (Bm, ldb), (C0, ldc), bias, _ = prob
    bufs = [embed(m, p, o, fill) for m, p, o, fill in ((A, lda, c.off[0], float("nan")), (Bm, ldb, c.off[1], float("nan")), (C0, ldc, c.off[2], SENT))]
    (_, Ad), (_, Bd), (Cbuf, Cd) = [on_device(b, v, dev) for b, v in bufs]
    call(Ad, lda, Bd, ldb, Cd, ldc, bias.to(dev) if bias is not None else None)
    got = Cbuf.cpu()
    out = got.as_strided(C0.shape, (ldc, 1), c.off[2]).clone()
    return out, got[outside(*bufs[2])]


def check_gemm(lib, dev, c):
    """both arithmetics on one problem: each against float64 with check_sgemm's gate, C[:, N:ldc] and everything else around C bit for
    bit, the result finite (beta = 0: C held NaN) — and the two side by side: bit-identical where the documented rule sends bf16x3 to
    the exact-fp32 kernel, within 4e-6 of the largest element where it does not"""
    test = "head_cases.check_gemm"
    prob = gemm_problem(c)
    ref = prob[4]
    atol = 1e-5 * max(1.0, c.K ** 0.5)
    res = {}
    for arith in ("f32", "bf16x3"):
        out, around = run_gemm(lib, dev, c, prob, lambda A, lda, B, ldb, C, ldc, bias: ops.sgemm(
            c.ta, c.tb, c.M, c.N, c.K, A, lda, B, ldb, C, ldc, bias=bias, beta=c.beta, arith=arith, lib=lib))
        assert bool(torch.isfinite(out).all()), (c.name, arith, "non-finite result")
        gated(test, c.name, "C", out, ref, 1e-5, atol, arith=arith)
        exact(test, c.name, "around C", around, torch.full_like(around, SENT), where=arith)
        res[arith] = out
    if bf16x3_fallback_reasons(c):
        exact(test, c.name, "bf16x3 request served by the exact-fp32 kernel", res["bf16x3"], res["f32"], where=",".join(sorted(bf16x3_fallback_reasons(c))))
    else:
        relative(test, c.name, "bf16x3 against exact fp32", res["bf16x3"], res["f32"], 4e-6, arith="bf16x3")


def check_gemm_entry_points(lib, dev, shape=(40, 36, 707), ta=1, tb=0):
    """rat_sgemm (no workspace), rat_sgemm_ws one byte short and rat_sgemm_ws with the whole workspace on a split-K shape: the first
    two are the single pass over k and bit-identical, all three within check_sgemm's gate of float64"""
    from rat_amd.ops import _p, _stream
    test = "head_cases.check_gemm_entry_points"
    M, N, K = shape
    need = lib.size("rat_sgemm_workspace", M, N, K)
    assert need > 0 and K % 32 != 0
    c = G("entry-points-%dx%dx%d" % shape, ta, tb, M, N, K, "qqo", (4, 0, 1), 0.5, True)
    prob = gemm_problem(c)
    atol = 1e-5 * max(1.0, K ** 0.5)
    res = {}
    for name in ("rat_sgemm", "rat_sgemm_ws short", "rat_sgemm_ws"):
        def call(A, lda, B, ldb, C, ldc, bias):
            if name == "rat_sgemm":
                lib.call("rat_sgemm", ta, tb, M, N, K, _p(A), lda, _p(B), ldb, _p(C), ldc, _p(bias), c.beta, _stream(C))
                return
            ws = torch.full(((need + 3) // 4 + TAIL,), SENT, dtype=torch.float32, device=C.device)
            nbytes = need - 1 if name.endswith("short") else need
            lib.call("rat_sgemm_ws", ta, tb, M, N, K, _p(A), lda, _p(B), ldb, _p(C), ldc, _p(bias), c.beta, _p(ws), nbytes, _stream(C))
            w = ws.cpu()
            exact(test, c.name, "behind the workspace", w[(need + 3) // 4:], torch.full((TAIL,), SENT), where=name)
            if name.endswith("short"):
                exact(test, c.name, "a too small workspace stays unused", w, torch.full_like(w, SENT), where=name)
            else:
                assert bool((w[:need // 4] != SENT).any()), "nothing was written into a sufficient workspace: the split-K plan did not run"
        out, around = run_gemm(lib, dev, c, prob, call)
        gated(test, c.name, "C", out, prob[4], 1e-5, atol, where=name)
        exact(test, c.name, "around C", around, torch.full_like(around, SENT), where=name)
        res[name] = out
    exact(test, c.name, "single pass: no workspace against a too small one", res["rat_sgemm"], res["rat_sgemm_ws short"])


# ----------------------------------------------------------------------------- 2. logit forward / backward
# dnn: None, "out" (a ready [B] vector), ("last", K, ld) (the one-output Linear inside the launch); pad: cls_stride = d + pad
L = collections.namedtuple("L", "B d nfields head averaged gscale gscale_dev dnn pad clamp", defaults=(False,))
GDEV = 1.75
LAST52, LAST7 = ("last", 52, 52), ("last", 7, 9)

LOGIT_CORE = [
    L(1, 7, 0, 0, False, 1.0, None, None, 1),                 # no LR term, one sample, the scalar dot
    L(15, 10, 3, 1, False, 0.5, GDEV, "out", 2),              # head 1, both gradient scales, stride % 4 == 0 under d % 4 != 0
    L(16, 40, 16, 0, False, 1.0, None, LAST52, 4),            # the vector dots, 16 fields = one trip of both field loops
    L(17, 64, 17, 0, True, 1.0, GDEV, "out", 4),              # averaged: rat_logit_fwd_pool / rat_logit_bwd_pool without ddnn_b
    L(33, 100, 37, 1, True, 0.5, None, LAST52, 3),            # averaged: rat_logit_fwd_dnn_pool, three trips, d % 4 == 0 on a stride that is not
    L(17, 200, 3, 0, True, 1.0, None, LAST7, 0),              # one column group in the backward, the scalar DNN dot
    L(16, 256, 17, 1, False, 1.0, GDEV, LAST7, 4),            # the widest row the backward accepts
    L(17, 10, 5, 0, True, 1.0, None, "out", 0, True),         # ids outside [0, vocab): the clamp
]
LOGIT_REST = [
    L(1000, 64, 3, 0, False, 1.0, None, "out", 0),
    L(1000, 40, 37, 0, True, 0.5, GDEV, LAST52, 4),
    L(33, 7, 16, 1, True, 1.0, GDEV, None, 2),
    L(1, 256, 37, 0, True, 1.0, None, LAST7, 1),
    L(15, 100, 17, 0, False, 0.5, None, LAST52, 0),
    L(16, 200, 0, 1, False, 1.0, GDEV, "out", 4),
    L(17, 40, 3, 1, False, 1.0, None, None, 3),
    L(33, 64, 37, 0, False, 1.0, GDEV, "out", 0, True),
    L(15, 10, 17, 1, True, 0.5, GDEV, LAST52, 2),
]
LOGIT_ALL = LOGIT_CORE + LOGIT_REST


def logit_id(c):
    dnn = "-" if c.dnn is None else (c.dnn if isinstance(c.dnn, str) else "last%d" % c.dnn[1])
    return "B%d-d%d-f%d-head%d-%s-g%g-dev%s-%s-pad%d%s" % (c.B, c.d, c.nfields, c.head, "avg" if c.averaged else "sum", c.gscale,
                                                           c.gscale_dev, dnn, c.pad, "-clamp" if c.clamp else "")


def logit_fields(nfields, averaged):
    """categorical, bag of 3, bag of 2, bag of 4 in turn; with `averaged` the bags of 3 and 4 are MaskedAveragePooling fields"""
    fields, col = [], 0
    for i in range(nfields):
        ncols, pooling = [(1, "sum"), (3, "average"), (2, "sum"), (4, "average")][i % 4]
        vocab = 6 + (5 * i) % 7
        fields.append(Field(col, ncols, vocab, padding_idx=vocab - 1 if ncols > 1 else None, pooling=pooling if averaged else "sum"))
        col += ncols
    return fields


def logit_problem(c, seed=21):
    """-> dict of float32 / int32 numpy inputs and the float64 statement of everything the kernels produce.
    LR tables hold exact 0.0 (row 0) and -0.0 (row 1, and scattered) in non-padding rows, padding rows are zero, some bags are padding
    only and some hold only zero-weight rows: both count 0.  The logit is kept inside |z| <= 3 for head 0 (asserted): p - t is then
    resolved by float32 to better than any gate used here (1 - p >= 0.047 against 6e-8 spacing).  For head 1 the labels keep
    |z - t| >= 0.5, so that the forward's rounding of z (about 1e-6) is below 1e-5 of every gradient term."""
    rs = np.random.RandomState(seed + 1000 * c.B + c.d + 7 * c.nfields)
    B, d, nf = c.B, c.d, c.nfields
    fields = logit_fields(nf, c.averaged)
    Lc = max([f.col + f.ncols for f in fields] + [1])
    T = 2
    tables = []
    for f in fields:
        t = (0.2 / max(1, nf) ** 0.5 * rs.standard_normal((f.vocab, 1))).astype(np.float32)
        u = rs.rand(f.vocab, 1)
        t[u < 0.1] = 0.0
        t[(u >= 0.1) & (u < 0.2)] = -0.0
        t[0], t[1] = 0.0, -0.0
        if f.padding_idx is not None:
            t[f.padding_idx] = 0.0
        tables.append(t)
    idx = np.zeros((B, T, Lc), dtype=np.int32)
    for i, f in enumerate(fields):
        ids = rs.randint(0, f.vocab, size=(B, T, f.ncols))
        if f.padding_idx is not None:
            ids[rs.rand(B, T) < 0.2] = f.padding_idx                      # bags made of padding only
            ids[i % B, 0] = [0, 1, f.padding_idx, 0][:f.ncols]            # a bag of zero-weight rows that are no padding
        if c.clamp:
            for b, bad in zip(range(i, B, 4), (-1, -3, f.vocab, f.vocab + 2)):
                ids[b, 0, (i + b) % f.ncols] = bad
        idx[..., f.col:f.col + f.ncols] = ids
    cls = rs.standard_normal((B, d)).astype(np.float32)
    fc_w = (0.3 * d ** -0.5 * rs.standard_normal((1, d))).astype(np.float32)
    fc_b = (0.1 * rs.standard_normal(1)).astype(np.float32)
    p = dict(case=c, fields=fields, tables=tables, idx=idx, T=T, Lc=Lc, cls=cls, fc_w=fc_w, fc_b=fc_b)
    z = cls.astype(np.float64) @ fc_w[0].astype(np.float64) + float(fc_b[0])
    if c.dnn == "out":
        p["dnn_out"] = (0.3 * rs.standard_normal(B)).astype(np.float32)
        z = z + p["dnn_out"]
    elif c.dnn is not None:
        _, K, ld = c.dnn
        p["dnn_a"] = rs.standard_normal((B, K)).astype(np.float32)
        p["dnn_w"] = (0.3 * K ** -0.5 * rs.standard_normal((1, K))).astype(np.float32)
        p["dnn_b"] = (0.1 * rs.standard_normal(1)).astype(np.float32)
        z = z + p["dnn_a"].astype(np.float64) @ p["dnn_w"][0].astype(np.float64) + float(p["dnn_b"][0])
    # LR term: ids clamped to [0, vocab - 1]; den = float32(count of non-zero weights) + float32(1e-16) where averaged, else 1
    den = np.ones((B, max(nf, 1)), dtype=np.float32)
    cid = []
    for i, f in enumerate(fields):
        ids = np.clip(idx[:, 0, f.col:f.col + f.ncols].astype(np.int64), 0, f.vocab - 1)
        cid.append(ids)
        w = tables[i][ids, 0]                                             # [B, ncols]
        s = w.astype(np.float64).sum(1)
        if f.pooling == "average":
            den[:, i] = (w != 0).sum(1).astype(np.float32) + np.float32(1e-16)
            s = s / den[:, i].astype(np.float64)
        z = z + s
    p["den"], p["cid"] = den, cid
    if c.head == 1:
        y = (z + np.where(rs.rand(B) < 0.5, -1.0, 1.0) * (0.5 + np.abs(rs.standard_normal(B)))).astype(np.float32)
        assert np.abs(z - y).min() >= 0.499
        pred = z
        loss = np.mean((z - y.astype(np.float64)) ** 2)
    else:
        assert np.abs(z).max() <= 3.0, ("the logit left the band the gates are stated for", float(np.abs(z).max()))
        y = rs.randint(0, 2, size=B).astype(np.float32)
        pred = 1.0 / (1.0 + np.exp(-z))
        loss = np.mean(-(y * np.maximum(np.log(pred), -100.0) + (1.0 - y) * np.maximum(np.log1p(-pred), -100.0)))
    p.update(y=y, z=z, pred=pred, loss=loss)
    # backward
    scale = c.gscale * (c.gscale_dev if c.gscale_dev is not None else 1.0) * (2.0 if c.head == 1 else 1.0)
    dl = scale * (pred - y.astype(np.float64)) / B
    p["dlogit"] = dl
    p["dcls"] = dl[:, None] * fc_w.astype(np.float64)
    p["dfc_w"] = (dl[:, None] * cls.astype(np.float64)).sum(0)
    p["dfc_b"] = dl.sum()
    grads, mags = [], []
    for i, f in enumerate(fields):
        g, m = np.zeros(f.vocab), np.zeros(f.vocab)
        if f.pooling == "average":                                        # divided in float32, as the kernel (and torch) do, then added
            term = (dl.astype(np.float32) / den[:, i]).astype(np.float64)
        else:
            term = dl
        for b in range(B):
            for j in cid[i][b]:
                if j != f.padding_idx:
                    g[j] += term[b]
                    m[j] += abs(term[b])
        grads.append(g)
        mags.append(m)
    p["lr_grads"], p["lr_mags"] = grads, mags
    return p


def _guarded_tables(arrs, fill, dev):
    """each [vocab][1] table as a view in the middle of a larger buffer filled with `fill` -> (buffers, views)"""
    bufs, views = [], []
    for a in arrs:
        b = torch.full((GUARD + a.shape[0] + GUARD,), float(fill), dtype=torch.float32)
        b[GUARD:GUARD + a.shape[0]] = torch.from_numpy(a[:, 0].copy())
        b = b.to(dev)
        bufs.append(b)
        views.append(b[GUARD:GUARD + a.shape[0]].view(-1, 1))
    return bufs, views


def run_logit_fwd(lib, dev, p, with_labels=True):
    c = p["case"]
    B, d, nf = c.B, c.d, c.nfields
    stride = d + c.pad
    cbuf, cview = on_device(*embed(torch.from_numpy(p["cls"]), stride, 0, float("nan")), dev)
    st = dict(cls=cview, stride=stride, fc_w=torch.from_numpy(p["fc_w"]).to(dev), idx=torch.from_numpy(p["idx"]).to(dev),
              y=torch.from_numpy(p["y"]).to(dev))
    ftab = modes = lr_den = None
    if nf:
        st["tab_bufs"], tabs = _guarded_tables(p["tables"], float("nan"), dev)
        ftab = ops.field_table(p["fields"], tabs, dev)
        modes = ops.pool_modes(p["fields"], dev)
        assert (modes is not None) == c.averaged
        if c.averaged:
            lr_den = torch.full((B * nf + TAIL,), SENT, dtype=torch.float32, device=dev)
    dnn_out = torch.from_numpy(p["dnn_out"]).to(dev) if c.dnn == "out" else None
    dnn_last = None
    if c.dnn is not None and c.dnn != "out":
        _, K, ld = c.dnn
        _, aview = on_device(*embed(torch.from_numpy(p["dnn_a"]), ld, 0, float("nan")), dev)
        dnn_last = (aview, ld, K, torch.from_numpy(p["dnn_w"]).to(dev), torch.from_numpy(p["dnn_b"]).to(dev))
    loss_sum = torch.zeros(1, device=dev) if with_labels else None
    yp = ops.logit_fwd(cview, stride, st["fc_w"], torch.from_numpy(p["fc_b"]).to(dev), dnn_out, ftab, nf, st["idx"], p["T"] * p["Lc"],
                       st["y"] if with_labels else None, loss_sum, B, d, head=c.head, dnn_last=dnn_last, modes=modes, lr_den=lr_den, lib=lib)
    st.update(y_pred=yp, loss_sum=loss_sum, lr_den=lr_den)
    return st


def check_logit_case(lib, dev, c):
    """one row of the matrix: forward (y_pred, loss, lr_den exactly, the eval form), backward (dlogit, dcls inside a sentinel buffer,
    dfc_w, dfc_b, ddnn_b onto a start value, the LR table gradients) against float64 with check_logit's gates; averaged fields with the
    accumulation-order gate of pooling_cases.check_pool_kernels"""
    test, wl = "head_cases.check_logit_case", logit_id(c)
    p = logit_problem(c)
    B, d, nf = c.B, c.d, c.nfields
    st = run_logit_fwd(lib, dev, p)
    gated(test, wl, "y_pred", st["y_pred"], p["pred"], 1e-5, 1e-6)
    gated(test, wl, "loss", st["loss_sum"], np.array([p["loss"]]), 1e-5, 1e-6)
    ev = run_logit_fwd(lib, dev, p, with_labels=False)
    exact(test, wl, "y_pred without labels (eval form)", ev["y_pred"], st["y_pred"])
    if c.averaged:
        den = st["lr_den"].cpu()
        exact(test, wl, "lr_den", den[:B * nf].view(B, nf), torch.from_numpy(p["den"]))
        exact(test, wl, "behind lr_den", den[B * nf:], torch.full((TAIL,), SENT))
        assert float(p["den"].min()) == float(np.float32(1e-16)), "no bag with a zero count"
    if nf:
        for b, t in zip(st["tab_bufs"], p["tables"]):
            side = torch.cat([b[:GUARD], b[GUARD + t.shape[0]:]]).cpu()
            assert bool(torch.isnan(side).all())
    # backward, on the forward's own y_pred as the product runs it
    dstride = d + 5
    dbuf, dview = on_device(*embed(torch.zeros(B, d), dstride, 0, SENT), dev)
    dfw, dfb = torch.zeros(1, d, device=dev), torch.zeros(1, device=dev)
    gftab = gbufs = None
    if nf:
        gbufs, gtabs = _guarded_tables([np.zeros_like(t) for t in p["tables"]], 0.0, dev)
        gftab = ops.field_table(p["fields"], gtabs, dev)
    gdev = torch.tensor([c.gscale_dev], dtype=torch.float32, device=dev) if c.gscale_dev is not None else None
    dob = torch.full((1,), 0.5, device=dev) if (c.dnn is not None and c.dnn != "out") else None
    dlogit = ops.logit_bwd(st["y_pred"], st["y"], st["cls"], st["stride"], st["fc_w"], dview, dstride, dfw, dfb, gftab, nf, st["idx"],
                           p["T"] * p["Lc"], c.gscale, B, d, gscale_dev=gdev, head=c.head, ddnn_b=dob, lr_den=st["lr_den"][:B * nf] if c.averaged else None,
                           lib=lib)
    gated(test, wl, "dlogit", dlogit, p["dlogit"], 1e-4, 1e-7)
    full = dbuf.cpu()
    gated(test, wl, "dcls", full.as_strided((B, d), (dstride, 1), 0), p["dcls"], 1e-4, 1e-7)
    around = full[outside(full, full.as_strided((B, d), (dstride, 1), 0))]
    exact(test, wl, "around dcls", around, torch.full_like(around, SENT))
    gated(test, wl, "dfc_w", dfw, p["dfc_w"], 1e-4, 1e-6)
    gated(test, wl, "dfc_b", dfb, np.array([p["dfc_b"]]), 1e-4, 1e-6)
    if dob is not None:
        gated(test, wl, "ddnn_b onto 0.5", dob - 0.5, np.array([p["dfc_b"]]), 1e-4, 1e-6)
    for i in range(nf):
        g = gbufs[i].cpu()
        v = p["fields"][i].vocab
        exact(test, wl, "around an LR gradient table", torch.cat([g[:GUARD], g[GUARD + v:]]), torch.zeros(2 * GUARD), where="field %d" % i)
        got, want, mag = g[GUARD:GUARD + v].double().numpy(), p["lr_grads"][i], p["lr_mags"][i]
        if c.averaged:                      # a fixed atol means nothing beside 1e16-sized elements: 1e-5 of the sum of |terms|
            err = np.abs(got - want)
            k = int((err / (1e-5 * mag + 1e-30)).argmax())
            margins.record(test, wl, "LR table gradient (averaged run)", float(err[k]), float(1e-5 * mag[k] + 1e-30), arith="f32", where="field %d" % i)
            assert np.all(np.isfinite(got)) and np.all(err <= 1e-5 * mag + 1e-30), (wl, i, float(err[k]), float(mag[k]))
        else:
            gated(test, wl, "LR table gradient", got, want, 1e-4, 1e-7, where="field %d" % i)
    if c.averaged:
        assert max(float(np.abs(w).max()) for w in p["lr_grads"]) > 1e12, "no element with a zero count: the 1e16 path went untested"
    if c.clamp:
        for f in p["fields"][:4]:
            assert {-1, -3, f.vocab, f.vocab + 2} <= set(p["idx"][:, 0, f.col:f.col + f.ncols].reshape(-1).tolist()), "ids on both sides of [0, vocab)"


def check_logit_saturation(lib, dev):
    """head 0 at saturated logits: the two logs clamped at -100.  z comes through dnn_out alone (cls = 0, fc_b = 0), from the bands
    |z| <= 6, 25 <= |z| <= 60 and |z| >= 110 with both labels at each value; outside those bands one ulp of p moves log p or log(1 - p)
    by more than any gate.  The reference is torch's: p in float64, rounded to float32, BCE in float64 on that with both logs clamped."""
    test, wl = "head_cases.check_logit_saturation", "bands 0-6, 25-60, 110+"
    zs = np.array([0.0, 0.5, 2.0, 6.0, 25.0, 33.5, 47.25, 60.0, 110.0, 150.0, 1000.0], dtype=np.float32)
    z = np.concatenate([zs, -zs, zs, -zs]).astype(np.float32)
    y = np.concatenate([np.ones(2 * len(zs)), np.zeros(2 * len(zs))]).astype(np.float32)
    az = np.abs(z)
    assert np.all((az <= 6) | ((az >= 25) & (az <= 60)) | (az >= 110)) and all(((az >= lo) & (az <= hi)).any() for lo, hi in ((0, 6), (25, 60), (110, 1e9)))
    B, d = len(z), 8
    with np.errstate(over="ignore", divide="ignore"):
        p32 = (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
        p64 = p32.astype(np.float64)
        per = -(y * np.maximum(np.log(p64), -100.0) + (1.0 - y) * np.maximum(np.log(1.0 - p64), -100.0))
    assert (per[y == 1] == 100.0).any() and (per[y == 0] == 100.0).any() and (p32 == 1.0).any() and (p32 == 0.0).any()
    rs = np.random.RandomState(3)
    cls = torch.zeros(B, d, device=dev)
    fc_w, fc_b = rnd(rs, 1, d).to(dev), torch.zeros(1, device=dev)
    loss_sum = torch.zeros(1, device=dev)
    yp = ops.logit_fwd(cls, d, fc_w, fc_b, torch.from_numpy(z).to(dev), None, 0, None, 0, torch.from_numpy(y).to(dev), loss_sum, B, d, lib=lib)
    gated(test, wl, "y_pred", yp, p32, 1e-5, 1e-6)
    gated(test, wl, "loss", loss_sum, np.array([per.mean()]), 1e-5, 1e-6)
    got = yp.cpu().reshape(-1).numpy()
    assert (got == 1.0).any() and (got == 0.0).any(), "y_pred must saturate to exactly 1 and exactly 0"
    exact(test, wl, "y_pred where the reference is exactly 0 or 1", got[(p32 == 0) | (p32 == 1)], p32[(p32 == 0) | (p32 == 1)])


def check_logit_refusal(lib, dev):
    """embedding_dim above the backward's block size: refused on the host, nothing launched (every output keeps its sentinel)"""
    B, d = 4, 257
    yp, y, cls, fc_w = (torch.zeros(n, device=dev) for n in (B, B, B * d, d))
    outs = [torch.full((n,), SENT, device=dev) for n in (B * d, d, 1)]
    try:
        ops.logit_bwd(yp, y, cls, d, fc_w, outs[0], d, outs[1], outs[2], None, 0, None, 0, 1.0, B, d, lib=lib)
    except RatError as e:
        assert "embedding_dim above the block size" in str(e), str(e)
    else:
        raise AssertionError("d = 257 was accepted")
    for o in outs:
        exact("head_cases.check_logit_refusal", "d=257", "outputs of a refused call", o, torch.full_like(o, SENT))


# ----------------------------------------------------------------------------- 3. BatchNorm + activation, all six codes
BN_TWO_LAUNCH_CORE = [(37, 40)]
BN_TWO_LAUNCH_REST = [(9, 5), (1000, 33)]                    # a partial column block whose width is no multiple of 4
BN_STRIP_CORE = [(37, 12)]
BN_STRIP_REST = [(8, 4), (256, 400), (1500, 64), (5000, 40)]  # with (37, 12): one shape of each rows-per-thread instantiation
CONST_COL = 1


def bn_problem(M, N, use_bn, act, seed):
    """column means far from zero; column 1 constant (variance 0, rstd = eps^-1/2, the output is act(beta)); without BN exact zeros of
    both signs in z, where the backward's derivative-from-the-output must follow torch's conventions"""
    rs = np.random.RandomState(seed)
    z = rnd(rs, M, N) + 3.0 * rnd(rs, N)
    if use_bn:
        if N > CONST_COL:
            z[:, CONST_COL] = 2.5
    else:
        flat = z.view(-1)
        flat[0::5] = 0.0
        flat[2::7] = -0.0
    gamma, beta = 1 + 0.1 * rnd(rs, N), 0.1 * rnd(rs, N)
    rm, rv = 0.1 * rnd(rs, N), 1 + 0.1 * rnd(rs, N).abs()
    da = rnd(rs, M, N)
    fn = ACT_FN[act]
    zr = z.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm_ref, rv_ref = rm.double().clone(), rv.double().clone()
    pre = torch.nn.functional.batch_norm(zr, rm_ref, rv_ref, gr, br, training=True, momentum=0.1, eps=1e-5) if use_bn else zr
    yr = fn(pre)
    yr.backward(da.double())
    ye = fn(torch.nn.functional.batch_norm(z.double(), rm_ref, rv_ref, gamma.double(), beta.double(), training=False, eps=1e-5)) if use_bn else None
    if not use_bn:                                             # the conventions at the kink, stated on the reference
        at0 = (z == 0)
        want = {"relu": 0.0, "leakyrelu": 0.01, "elu": 1.0, "none": 1.0, "sigmoid": 0.25, "tanh": 1.0}[act]
        assert int(at0.sum()) >= 2 and torch.equal(zr.grad[at0], want * da.double()[at0])
    return dict(z=z, gamma=gamma, beta=beta, rm=rm, rv=rv, da=da, a=yr.detach(), dz=zr.grad, dgamma=gr.grad, dbeta=br.grad,
                rm_ref=rm_ref, rv_ref=rv_ref, a_eval=ye)


def _column_sum_factor(use_bn, N):
    """for the gate on the column sums of dz (the strips' Linear bias gradient), whose absolute part is sized for a sum of O(1)
    elements: 1 per column — except the constant column under BatchNorm, where dz = rstd gamma (g - mean g) with rstd = eps^-1/2 =
    316.  Its elements are 316 times larger, their true sum is 0, and the float32 rounding of the sum grows with the elements:
    atol x eps^-1/2 in this one column.  dz itself keeps the plain gate everywhere."""
    f = torch.ones(N, dtype=torch.float64)
    if use_bn and N > CONST_COL:
        f[CONST_COL] = 1e-5 ** -0.5
    return f


def check_bn_two_launch(lib, dev, M, N, use_bn, act):
    """rat_bn_relu_fwd / rat_bn_relu_bwd with any activation against float64 autograd: training, then eval on the updated statistics"""
    test, wl = "head_cases.check_bn_two_launch", "%dx%d %s %s" % (M, N, "bn" if use_bn else "no-bn", act)
    p = bn_problem(M, N, use_bn, act, seed=4)
    code = ops.ACT[act]
    zd, rmd, rvd, gd, bd = (p[k].to(dev) for k in ("z", "rm", "rv", "gamma", "beta"))
    a, sm, sr = ops.bn_relu_fwd(zd, gd, bd, rmd, rvd, True, use_bn, act=code, lib=lib)
    gated(test, wl, "a", a, p["a"], 1e-5, 1e-5)
    dg, db = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    dz = ops.bn_relu_bwd(zd, a, p["da"].to(dev), gd, sm, sr, dg, db, use_bn, act=code, lib=lib)
    gated(test, wl, "dz", dz, p["dz"], 1e-4, 1e-5)
    if use_bn:
        if N > CONST_COL:
            gated(test, wl, "a of the constant column = act(beta)", a[:, CONST_COL], ACT_FN[act](p["beta"][CONST_COL].double()).expand(M), 1e-5, 1e-5)
            exact(test, wl, "save_mean of the constant column", sm[CONST_COL:CONST_COL + 1], torch.tensor([2.5]))
            gated(test, wl, "save_rstd of the constant column", sr[CONST_COL:CONST_COL + 1], torch.tensor([1e-5 ** -0.5]), 1e-5, 0.0)
        gated(test, wl, "running_mean", rmd, p["rm_ref"], 1e-5, 1e-6)
        gated(test, wl, "running_var", rvd, p["rv_ref"], 1e-5, 1e-6)
        gated(test, wl, "dgamma", dg, p["dgamma"], 1e-4, 1e-4)
        gated(test, wl, "dbeta", db, p["dbeta"], 1e-4, 1e-4)
        a2, _, _ = ops.bn_relu_fwd(zd, gd, bd, rmd, rvd, False, True, act=code, lib=lib)
        gated(test, wl, "a (eval)", a2, p["a_eval"], 1e-5, 1e-5)


def check_bn_strips(lib, dev, M, N, use_bn, act):
    """rat_bn_act_fwd_strip / _bwd_strip / _bwd_strip_outer with any activation: against float64 autograd with check_bn_strip's gates,
    the outer-product form against the plain strip backward with check_bn_strip_outer's"""
    test, wl = "head_cases.check_bn_strips", "%dx%d %s %s" % (M, N, "bn" if use_bn else "no-bn", act)
    p = bn_problem(M, N, use_bn, act, seed=14)
    code = ops.ACT[act]
    zd, rmd, rvd, gd, bd = (p[k].to(dev) for k in ("z", "rm", "rv", "gamma", "beta"))
    if use_bn:
        a, sm, sr = ops.bn_act_fwd_strip(zd, gd, bd, rmd, rvd, True, True, act=code, lib=lib)
    else:
        a, sm, sr = ops.bn_act_fwd_strip(zd, None, None, None, None, True, False, act=code, lib=lib)
    gated(test, wl, "a", a, p["a"], 1e-5, 1e-5)
    scale = max(1.0, M ** 0.5)

    def grads():
        return (torch.zeros(N, device=dev) if use_bn else None, torch.zeros(N, device=dev) if use_bn else None, torch.full((N,), 7.0, device=dev))
    dg, db, dbl = grads()
    dz = ops.bn_act_bwd_strip(zd, a, p["da"].to(dev), gd if use_bn else None, sm, sr, dg, db, dbl, use_bn, act=code, lib=lib)
    gated(test, wl, "dz", dz, p["dz"], 1e-4, 1e-5)
    gated(test, wl, "Linear bias gradient", dbl, dz.double().sum(0), 1e-5, 1e-5 * scale * _column_sum_factor(use_bn, N))
    if use_bn:
        if N > CONST_COL:
            gated(test, wl, "a of the constant column = act(beta)", a[:, CONST_COL], ACT_FN[act](p["beta"][CONST_COL].double()).expand(M), 1e-5, 1e-5)
        gated(test, wl, "running_mean", rmd, p["rm_ref"], 1e-5, 1e-6)
        gated(test, wl, "running_var", rvd, p["rv_ref"], 1e-5, 1e-6)
        gated(test, wl, "dgamma", dg, p["dgamma"], 1e-4, 1e-5 * scale)
        gated(test, wl, "dbeta", db, p["dbeta"], 1e-4, 1e-5 * scale)
        a2, _, _ = ops.bn_act_fwd_strip(zd, gd, bd, rmd, rvd, False, True, act=code, lib=lib)
        gated(test, wl, "a (eval)", a2, p["a_eval"], 1e-5, 1e-5)
        rm2, rv2 = p["rm"].to(dev), p["rv"].to(dev)
        a3, sm3, sr3 = ops.bn_relu_fwd(zd, gd, bd, rm2, rv2, True, True, act=code, lib=lib)
        gated(test, wl, "a against the two-launch kernels", a, a3, 1e-5, 1e-5)
        gated(test, wl, "save_mean against the two-launch kernels", sm, sm3, 1e-6, 1e-6)
        gated(test, wl, "save_rstd against the two-launch kernels", sr, sr3, 1e-5, 1e-6)
    # the last hidden layer's form: da = dl (x) w inside the launch, dw = dl^T a returned
    rs = np.random.RandomState(15)
    dl, w = rnd(rs, M, 1), rnd(rs, 1, N)
    da = (dl.double() @ w.double()).float().to(dev)
    dg1, db1, dbl1 = grads()
    ref = ops.bn_act_bwd_strip(zd, a, da, gd if use_bn else None, sm, sr, dg1, db1, dbl1, use_bn, act=code, lib=lib)
    dg2, db2, dbl2 = grads()
    dw = torch.zeros(N, device=dev)
    dz2 = ops.bn_act_bwd_strip_outer(zd, a, dl.to(dev), w.to(dev), dw, gd if use_bn else None, sm, sr, dg2, db2, dbl2, use_bn, act=code, lib=lib)
    gated(test, wl, "outer dz against the plain strip", dz2, ref, 1e-5, 1e-6)
    gated(test, wl, "outer Linear bias gradient", dbl2, dbl1, 1e-4, 1e-5 * scale)
    gated(test, wl, "outer dw = dl^T a", dw, (dl.double().t() @ a.double().cpu()).reshape(-1), 1e-5, 1e-5 * scale)
    if use_bn:
        gated(test, wl, "outer dgamma", dg2, dg1, 1e-4, 1e-5 * scale)
        gated(test, wl, "outer dbeta", db2, db1, 1e-4, 1e-5 * scale)
