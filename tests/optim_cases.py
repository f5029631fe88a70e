"""Shared kernel-level checks of the optimizer sweeps and the row-update kernels (csrc/optim.hip, csrc/sparse.hip, csrc/gather.hip) —
used with the host-emulation build on CPU (tests/test_optim_kernels.py) and the HIP build on the GPU (tests/test_gpu_optim.py).

Every numeric comparison is against float64 on the CPU, computed independently of the kernels: torch.optim on float64 parameters where
the optimizer starts from zero state, the closed formulas of kernel_cases.check_optim where a case starts from non-zero moments.

Gates (rtol, atol) are check_optim's — the arithmetic per element is the same — with the atol scaled by the step count.  They were never
measured for several steps from zero state, so the SAME reference also runs in float32 on the CPU (plain torch) and its largest distance
from the float64 result is taken: the gate of a quantity is the larger of check_optim's gate and 4 x that distance (the factor absorbs
summation order and fma contraction, which differ between torch and the kernels).  No gate is derived from a kernel's output.

Every array a kernel writes (and the gradient it may only clear) is a view into a larger buffer whose other elements hold a sentinel;
every check asserts that the sentinels survive — a vector tail that runs over the end of a view lands there."""
import functools
import math

import numpy as np
import torch

import margins
from kernel_cases import F, rnd
from rat_amd import ops

SENT = 12345.0
FRONT = BACK = 8                    # sentinel floats around every view; FRONT % 4 == 0: a view's 16-byte alignment is its offset's
LAM_A, LAM_B = 0.02, 0.005
GATES = {"m": (1e-5, 1e-7), "v": (1e-5, 1e-8), "w": (1e-5, 1e-6), "norm_sq": (1e-5, 1e-5), "reg": (1e-5, 1e-6)}   # kernel_cases.check_optim
KINDS = {"Adam": 0, "SGD": 1, "Adagrad": 2, "RMSprop": 3}
STATE_KEY = {"Adam": "exp_avg_sq", "Adagrad": "sum", "RMSprop": "square_avg"}
OPT_ARGS = {"SGD": (0.0, 0.0), "Adagrad": (0.0, 1e-10), "RMSprop": (0.99, 1e-8)}       # (p0, eps): torch.optim's defaults

A0, A4, M1, MM, MV = (0, 0, 0, 0), (4, 4, 4, 4), (1, 1, 1, 1), (0, 0, 1, 0), (0, 0, 0, 3)   # view starts of (w, g, m, v), in floats


class Guarded:
    """`data` as a view `off` floats behind a 16-byte-aligned position of a sentinel-filled buffer on `dev`"""

    def __init__(self, data, off, dev):
        self.n, self.start = data.numel(), FRONT + off
        buf = torch.full((self.start + self.n + BACK,), SENT, dtype=torch.float32)
        buf[self.start:self.start + self.n] = data.reshape(-1)
        self.buf = buf.to(dev)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.start:self.start + self.n].view(data.shape)
        assert self.view.data_ptr() % 16 == (4 * off) % 16

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:self.start] == SENT).all()) and bool((b[self.start + self.n:] == SENT).all())

    def cpu(self):
        return self.view.cpu().clone()


def gated(test, workload, quantity, got, ref64, ref32=None, steps=1, gate=None, against=None, where=""):
    """|got - ref64| (or |got - against|: two device results held to the reference's gate) <= max(atol steps + rtol |ref64|,
    4 max|ref32 - ref64|), element by element; the worst element goes to the margins file"""
    rtol, atol = gate or GATES[quantity]
    got = got.detach().cpu().double().reshape(-1)
    ref = ref64.detach().double().reshape(-1)
    other = ref if against is None else against.detach().cpu().double().reshape(-1)
    assert got.shape == ref.shape == other.shape
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite %s" % (test, workload, quantity)
    d32 = float((ref32.detach().double().reshape(-1) - ref).abs().max()) if ref32 is not None else 0.0
    allowed = torch.clamp(atol * steps + rtol * ref.abs(), min=4.0 * d32)
    err = (got - other).abs()
    k = int((err / allowed).argmax())
    margins.record(test, workload, quantity, float(err[k]), float(allowed[k]), arith="f32",
                   where=("%s; float32 CPU reference distance %.3g" % (where, d32)).strip("; "))
    assert float(err[k]) <= float(allowed[k]), "%s %s %s: |error| %.3g at element %d exceeds the gate %.3g (%s)" % (
        test, workload, quantity, float(err[k]), k, float(allowed[k]), where)


def _lam_vec(n, n_split, scale=1.0):
    return torch.where(torch.arange(n) < n_split, LAM_A * scale, LAM_B * scale).double()


def _clock(lib, dev, step, lr, b1=0.9, b2=0.999):
    """the device clock one tick before `step`: adam_tick(...) on the returned tensors makes hyper the scalars of `step`"""
    return (torch.tensor([step - 1], dtype=torch.int32).to(dev), torch.tensor([lr], dtype=torch.float32).to(dev),
            torch.zeros(4, dtype=torch.float32).to(dev))


def _path(n_split, offsets):
    return "vector" if (n_split % 4 == 0 and all(o % 4 == 0 for o in offsets)) else "scalar"


# ----------------------------------------------------------------------------- 1. rat_sumsq_reg + rat_clip_adam_fused from state
def _fused_adam_ref(w, g, m, v, n_split, scale, start, clip_norm, max_norm, lr, b1, b2, eps, step, dt):
    """closed formulas (kernel_cases.check_optim) in `dt`; the norm the clip reads is start + sum, as the kernel accumulates it"""
    n = w.numel()
    w, g, m, v = (t.to(dt) for t in (w, g, m, v))
    t = g + _lam_vec(n, n_split, scale).to(dt) * w
    acc = torch.tensor(start, dtype=dt) + (t * t).sum()
    reg_acc = torch.tensor(start, dtype=dt) + (0.5 * _lam_vec(n, n_split).to(dt) * w * w).sum()
    coef = torch.clamp(max_norm / (acc.sqrt() + 1e-6), max=1.0) if clip_norm else torch.tensor(1.0, dtype=dt)
    gc_ = t * coef
    mr = b1 * m + (1 - b1) * gc_
    vr = b2 * v + (1 - b2) * gc_ * gc_
    wr = w - lr / (1 - b1 ** step) * mr / (vr.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
    return {"norm_sq": (acc.double() - start).reshape(1), "reg": (reg_acc.double() - start).reshape(1), "coef": float(coef),
            "m": mr, "v": vr, "w": wr}


def check_fused_adam(lib, dev, n, n_split, offsets, clip, lam_scale, zero_g):
    """clip: None (no norm pointer), "off" (max_norm 1e9: coef == 1 exactly) or "on" (max_norm 10: coef < 1)"""
    assert 0 <= n_split <= n and clip in (None, "off", "on")
    test = "optim_cases.check_fused_adam"
    workload = "%s path, n %s" % (_path(n_split, offsets), "> 2 Mi" if n > (2 << 20) else "<= 24579")
    where = "n=%d split=%d offsets=%s clip=%s scale=%s zero_g=%s" % (n, n_split, offsets, clip, lam_scale, zero_g)
    rs = np.random.RandomState(61)
    w, g = rnd(rs, n), rnd(rs, n, scale=3.0)
    m, v = 0.1 * rnd(rs, n), 0.01 * rnd(rs, n).abs()
    lr, b1, b2, eps, step, start = 1e-3, 0.9, 0.999, 1e-8, 3, 2.5
    max_norm = {None: 0.0, "off": 1e9, "on": 10.0}[clip]
    scale = 1.0 if lam_scale is None else lam_scale
    args = (w, g, m, v, n_split, scale, start, clip is not None, max_norm, lr, b1, b2, eps, step)
    r64, r32 = _fused_adam_ref(*args, torch.float64), _fused_adam_ref(*args, torch.float32)
    if clip == "on":
        assert r64["coef"] < 1.0, "the case does not clip: choose a larger n"
    else:
        assert r64["coef"] == 1.0

    def run(with_norm):
        W, G, M, V = (Guarded(t, o, dev) for t, o in zip((w, g, m, v), offsets))
        scal = torch.tensor([SENT, start, start, SENT], dtype=torch.float32).to(dev)      # both outputs ACCUMULATE: they start at 2.5
        ls = None if lam_scale is None else torch.tensor([lam_scale], dtype=torch.float32).to(dev)
        step_dev, lr_dev, hyper = _clock(lib, dev, step, lr)
        ops.adam_tick(step_dev, lr_dev, b1, b2, hyper, lib=lib)
        ops.sumsq_reg(G.view, W.view, n_split, LAM_A, LAM_B, scal[1:2], reg_out=scal[2:3], lam_scale_dev=ls, lib=lib)
        assert torch.equal(G.cpu(), g) and torch.equal(W.cpu(), w), "rat_sumsq_reg only reads g and w"
        sums = scal.cpu().clone()
        ops.clip_adam_fused(W.view, G.view, M.view, V.view, n_split, LAM_A, LAM_B, scal[1:2] if with_norm else None, max_norm, hyper,
                            b1, b2, eps, zero_g=zero_g, lam_scale_dev=ls, lib=lib)
        assert all(t.intact() for t in (W, G, M, V)), "a sentinel next to w, g, m or v was overwritten (%s)" % where
        assert torch.equal(scal.cpu(), sums) and float(sums[0]) == SENT and float(sums[3]) == SENT
        assert int(step_dev.cpu()) == step
        return sums, W.cpu(), G.cpu(), M.cpu(), V.cpu()

    sums, wd, gd, md, vd = run(clip is not None)
    gated(test, workload, "norm_sq", sums[1:2].double() - start, r64["norm_sq"], r32["norm_sq"], where=where)
    gated(test, workload, "reg", sums[2:3].double() - start, r64["reg"], r32["reg"], where=where)      # the UNSCALED lambdas
    for q, got in (("m", md), ("v", vd), ("w", wd)):
        gated(test, workload, q, got, r64[q], r32[q], where=where)
    if zero_g:
        assert float(gd.abs().max()) == 0.0 and not bool(torch.signbit(gd).any()), "zero_g must clear every element, the tail included"
    else:
        assert torch.equal(gd, g), "without zero_g the gradient is only read"
    if clip == "off":                                     # coef == 1 exactly: the same bits as without a norm pointer
        _, w2, g2, m2, v2 = run(False)
        assert torch.equal(w2, wd) and torch.equal(m2, md) and torch.equal(v2, vd) and torch.equal(g2, gd)


def _std_cases(n):
    mid = (n // 8) * 4
    core = [(n, 4, A0, "on", None, True),                 # vector path, boundary inside the first float4 trip
            (n, mid, A4, "off", 0.5, False),              # vector path, views 16 bytes into an aligned buffer
            (n, mid + 1, A0, "on", 0.5, True)]            # n_split % 4 == 1: scalar path although every pointer is aligned
    more = [(n, 0, M1, None, None, False), (n, n, MM, "off", None, True), (n, mid, MV, "on", 0.5, False), (n, 0, A0, None, 0.5, True),
            (n, 5, A4, None, None, False), (n, n, A0 if n % 4 == 0 else M1, "on", None, False)]
    return core, more


def _fused_adam_matrix():
    tiny = [(1, 0, A0, None, None, True), (1, 1, M1, "off", 0.5, False), (1, 1, A4, None, None, True),
            (3, 0, A4, "off", 0.5, True), (3, 1, A0, None, None, False), (3, 3, MM, None, 0.5, True), (3, 2, MV, "off", None, False),
            (4, 4, A0, None, 0.5, False), (4, 0, A0, "off", None, True), (4, 1, A4, "off", None, True), (4, 3, M1, None, None, False),
            (5, 4, A0, "off", None, True), (5, 4, A4, None, 0.5, False), (5, 1, A0, None, 0.5, True), (5, 5, MV, "off", None, False),
            (5, 0, A0, None, None, False)]
    core, repeats = list(tiny), []
    for n in (1027, 4096, 20483, 24576):
        c, m_ = _std_cases(n)
        core += c + m_
    for n in (4100, 24579):                               # the same branches as 4096 / 20483 at another remainder
        c, m_ = _std_cases(n)
        core += c
        repeats += m_
    big, more = _std_cases(2 * 2097152 + 4 * 1000 + 3)    # the Adam sweep grid-strides: two full trips, a partial third, the scalar tail
    return core, repeats, big + [more[0], more[2]]


def case_id(case):
    n, n_split, offsets, clip, lam_scale, zero_g = case
    return "n%d-split%d-off%s-clip_%s-scale_%s-%s" % (n, n_split, "".join(map(str, offsets)), clip, lam_scale, "zero_g" if zero_g else "keep_g")


FUSED_ADAM_CORE, FUSED_ADAM_REPEATS, FUSED_ADAM_GPU_ONLY = _fused_adam_matrix()


@functools.lru_cache(maxsize=1)
def _large_inputs():
    rs = np.random.RandomState(62)
    n = (16 << 20) + 20001
    return rnd(rs, n), rnd(rs, n, scale=3.0)


def check_sumsq_reg_large(lib, dev, n):
    """rat_sumsq_reg alone past the 16 Mi switch of its grid rule: the norm and the regulariser value against float64 dot products"""
    w_all, g_all = _large_inputs()
    assert (16 << 20) <= n <= w_all.numel()
    test, workload = "optim_cases.check_sumsq_reg_large", "n >= 16 Mi"
    w, g = w_all[:n], g_all[:n]
    n_split, scale, start = (n // 8) * 4, 0.5, 2.5
    ref = {}
    for dt in (torch.float64, torch.float32):
        wa, wb = w[:n_split].to(dt), w[n_split:].to(dt)
        ta, tb = g[:n_split].to(dt) + (LAM_A * scale) * wa, g[n_split:].to(dt) + (LAM_B * scale) * wb
        ref[dt] = ((torch.tensor(start, dtype=dt) + (ta @ ta + tb @ tb)).double() - start,
                   (torch.tensor(start, dtype=dt) + (0.5 * LAM_A * (wa @ wa) + 0.5 * LAM_B * (wb @ wb))).double() - start)
    G, W = Guarded(g, 0, dev), Guarded(w, 0, dev)
    scal = torch.tensor([SENT, start, start, SENT], dtype=torch.float32).to(dev)
    ls = torch.tensor([scale], dtype=torch.float32).to(dev)
    ops.sumsq_reg(G.view, W.view, n_split, LAM_A, LAM_B, scal[1:2], reg_out=scal[2:3], lam_scale_dev=ls, lib=lib)
    sums = scal.cpu()
    assert float(sums[0]) == SENT and float(sums[3]) == SENT and G.intact() and W.intact()
    gated(test, workload, "norm_sq", sums[1:2].double() - start, ref[torch.float64][0].reshape(1), ref[torch.float32][0].reshape(1), where="n=%d" % n)
    gated(test, workload, "reg", sums[2:3].double() - start, ref[torch.float64][1].reshape(1), ref[torch.float32][1].reshape(1), where="n=%d" % n)


# ----------------------------------------------------------------------------- 2. several steps from zero state against torch.optim
def _torch_optim_run(kind, w0, grads, lam, lr, max_norm, dt):
    """getattr(torch.optim, kind)([p], lr=lr) — the defaults the reference's get_optimizer builds — on g + lambda w, clipped by
    clip_grad_norm_; per step: w, the state buffers and the squared norm the clip saw"""
    p = torch.nn.Parameter(w0.to(dt).clone())
    opt = getattr(torch.optim, kind)([p], lr=lr)
    out = []
    for g in grads:
        p.grad = g.to(dt) + lam.to(dt) * p.detach()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        st = opt.state[p]
        rec = {"w": p.detach().clone(), "norm_sq": (norm.detach().double() ** 2).reshape(1)}
        if kind == "Adam":
            rec["m"] = st["exp_avg"].clone()
        if kind != "SGD":
            rec["v"] = st[STATE_KEY[kind]].clone()
        out.append(rec)
    return out


def check_fused_training_run(lib, dev, kind, n, n_split, steps=3, lam_scale=None):
    """`steps` optimizer steps from zero state, a fresh gradient each step, the clock from rat_adam_tick: Adam through rat_clip_adam_fused;
    SGD / Adagrad / RMSprop through rat_clip_opt_fused AND through the unfused rat_clip_opt (gradient already holding lambda w, norm from
    rat_sumsq), both against torch.optim in float64 and against each other"""
    test = "optim_cases.check_fused_training_run"
    workload = "%s, n %s" % (kind, "> 2 Mi" if n > (2 << 20) else "<= 20483")
    lr, max_norm, b1, b2 = 1e-2, 10.0, 0.9, 0.999
    p0, eps = (b1, 1e-8) if kind == "Adam" else OPT_ARGS[kind]
    scale = 1.0 if lam_scale is None else lam_scale
    rs = np.random.RandomState(63)
    w0 = rnd(rs, n)
    grads = [rnd(rs, n, scale=3.0) for _ in range(steps)]
    lam = _lam_vec(n, n_split, scale)
    r64 = _torch_optim_run(kind, w0, grads, lam, lr, max_norm, torch.float64)
    r32 = _torch_optim_run(kind, w0, grads, lam, lr, max_norm, torch.float32)
    quantities = ["w"] + (["m"] if kind == "Adam" else []) + (["v"] if kind != "SGD" else [])
    zeros = torch.zeros(n)

    def fused(nsteps, state_fill=0.0):
        W, G = Guarded(w0, 0, dev), Guarded(zeros, 0, dev)
        M = Guarded(zeros, 0, dev) if kind == "Adam" else None
        V = Guarded(zeros + state_fill, 0, dev) if (kind != "SGD" or state_fill) else None
        nsq, reg = torch.zeros(1).to(dev), torch.zeros(1).to(dev)
        ls = None if lam_scale is None else torch.tensor([lam_scale], dtype=torch.float32).to(dev)
        step_dev, lr_dev, hyper = _clock(lib, dev, 1, lr)
        out = []
        for t in range(nsteps):
            G.view.copy_(grads[t].to(dev))
            ops.adam_tick(step_dev, lr_dev, b1, b2, hyper, lib=lib)
            nsq.zero_(), reg.zero_()
            ops.sumsq_reg(G.view, W.view, n_split, LAM_A, LAM_B, nsq, reg_out=reg, lam_scale_dev=ls, lib=lib)
            if kind == "Adam":
                ops.clip_adam_fused(W.view, G.view, M.view, V.view, n_split, LAM_A, LAM_B, nsq, max_norm, hyper, b1, b2, eps, zero_g=True,
                                    lam_scale_dev=ls, lib=lib)
            else:
                ops.clip_opt_fused(W.view, G.view, V.view if V is not None else None, n_split, LAM_A, LAM_B, nsq, max_norm, hyper,
                                   KINDS[kind], p0, eps, zero_g=True, lam_scale_dev=ls, lib=lib)
            assert float(G.view.abs().max()) == 0.0, "the fused sweep leaves g = 0 behind"
            assert all(b.intact() for b in (W, G, M, V) if b is not None)
            out.append({"w": W.cpu(), "m": M.cpu() if M is not None else None, "v": V.cpu() if V is not None else None,
                        "norm_sq": nsq.cpu().clone()})
        assert int(step_dev.cpu()) == nsteps
        return out

    def unfused(nsteps, state_fill=0.0):
        W = Guarded(w0, 0, dev)
        V = Guarded(zeros + state_fill, 0, dev) if (kind != "SGD" or state_fill) else None
        nsq = torch.zeros(1).to(dev)
        lam32 = lam.float().to(dev)
        out = []
        for t in range(nsteps):
            G = Guarded(grads[t], 0, dev)
            G.view.add_(lam32 * W.view)                    # optim.py::clip_and_step receives the gradient with lambda w already in it
            before = G.cpu()
            nsq.zero_()
            ops.sumsq(G.view, nsq, lib=lib)
            ops.clip_opt(W.view, G.view, V.view if V is not None else None, nsq, max_norm, lr, KINDS[kind], p0, eps, lib=lib)
            assert torch.equal(G.cpu(), before) and all(b.intact() for b in (W, G, V) if b is not None)
            out.append({"w": W.cpu(), "v": V.cpu() if V is not None else None, "norm_sq": nsq.cpu().clone()})
        return out

    runs = {"fused": fused(steps)}
    if kind != "Adam":
        runs["unfused"] = unfused(steps)
    for t in range(steps):
        where = "n=%d split=%d step %d" % (n, n_split, t + 1)
        for form, res in runs.items():
            gated(test, workload, "norm_sq", res[t]["norm_sq"], r64[t]["norm_sq"], r32[t]["norm_sq"], where=where + " " + form)
            for q in quantities:
                gated(test, workload, q, res[t][q], r64[t][q], r32[t][q], steps=t + 1, where=where + " " + form)
        if kind != "Adam":
            for q in quantities:
                gated(test, workload, q, runs["fused"][t][q], r64[t][q], r32[t][q], steps=t + 1, against=runs["unfused"][t][q],
                      where=where + " fused against unfused")
    if kind == "SGD":                                      # a state buffer passed to SGD is never touched, and changes nothing
        for form, fn in (("fused", fused), ("unfused", unfused)):
            res = fn(1, state_fill=SENT)[0]
            assert bool((res["v"] == SENT).all()), "SGD wrote its state buffer (%s)" % form
            assert torch.equal(res["w"], runs[form][0]["w"])


# ----------------------------------------------------------------------------- 3. row lists: rat_adam_rows_dev, rat_adam_rows, rat_sumsq_rows
def check_adam_rows_dev(lib, dev, d, total_rows, max_rows, count):
    """`count` < max_rows valid, distinct, unsorted rows; the entries behind `count` name a valid row that is NOT listed (and carry
    gradient rows): it must not move"""
    assert 0 < count < max_rows and count < total_rows
    test = "optim_cases.check_adam_rows_dev"
    workload = "d=%d rows=%d/%d/%d" % (d, total_rows, max_rows, count)
    rs = np.random.RandomState(64)
    w = rnd(rs, total_rows, d)
    m, v = 0.1 * rnd(rs, total_rows, d), 0.01 * rnd(rs, total_rows, d).abs()
    perm = rs.permutation(total_rows)
    listed, spare = torch.from_numpy(perm[:count]).long(), int(perm[count])
    rows = torch.full((max_rows,), spare, dtype=torch.int32)
    rows[:count] = listed.int()
    grads = rnd(rs, max_rows, d, scale=3.0)
    lr, b1, b2, eps, step, max_norm, norm_sq = 1e-3, 0.9, 0.999, 1e-8, 3, 10.0, 400.0
    ref = {}
    for dt in (torch.float64, torch.float32):
        coef = torch.clamp(max_norm / (torch.tensor(norm_sq, dtype=dt).sqrt() + 1e-6), max=1.0)
        gc_ = grads[:count].to(dt) * coef
        mr = b1 * m[listed].to(dt) + (1 - b1) * gc_
        vr = b2 * v[listed].to(dt) + (1 - b2) * gc_ * gc_
        wr = w[listed].to(dt) - lr / (1 - b1 ** step) * mr / (vr.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
        ref[dt] = {"m": mr, "v": vr, "w": wr, "coef": float(coef),
                   "norm_sq": ((torch.tensor(2.5, dtype=dt) + (grads[:count].to(dt) ** 2).sum()).double() - 2.5).reshape(1)}
    assert ref[torch.float64]["coef"] < 1.0
    others = torch.ones(total_rows, dtype=torch.bool)
    others[listed] = False
    rows_d, grads_d, nsq_d = rows.to(dev), grads.to(dev), torch.tensor([norm_sq], dtype=torch.float32).to(dev)

    def run(cnt, host_scalars=False):
        W, M, V = (Guarded(t, 0, dev) for t in (w, m, v))
        cnt_d = torch.tensor([cnt], dtype=torch.int32).to(dev)
        if host_scalars:
            ops.adam_rows(W.view, M.view, V.view, rows_d, grads_d, cnt_d, max_rows, d, nsq_d, max_norm, lr, b1, b2, eps, step, lib=lib)
        else:
            step_dev, lr_dev, hyper = _clock(lib, dev, step, lr)
            ops.adam_tick(step_dev, lr_dev, b1, b2, hyper, lib=lib)
            ops.adam_rows_dev(W.view, M.view, V.view, rows_d, grads_d, cnt_d, max_rows, d, nsq_d, max_norm, hyper, b1, b2, eps, lib=lib)
        assert W.intact() and M.intact() and V.intact()
        return {"w": W.cpu(), "m": M.cpu(), "v": V.cpu()}

    res = run(count)
    for q, orig in (("m", m), ("v", v), ("w", w)):
        gated(test, workload, q, res[q][listed], ref[torch.float64][q], ref[torch.float32][q])
        assert torch.equal(res[q][others], orig[others]), "a row outside the list moved (%s)" % q
    none = run(0)
    assert all(torch.equal(none[q], orig) for q, orig in (("m", m), ("v", v), ("w", w))), "count = 0 changes nothing"
    host = run(count, host_scalars=True)                    # the same expression and the same scalars: the same bits
    assert all(torch.equal(host[q], res[q]) for q in ("m", "v", "w")), "rat_adam_rows and rat_adam_rows_dev differ"
    # rat_sumsq_rows accumulates onto its output and reads only the first `count` rows
    out = torch.tensor([SENT, 2.5, SENT], dtype=torch.float32).to(dev)
    ops.sumsq_rows(grads_d, torch.tensor([count], dtype=torch.int32).to(dev), max_rows, d, out[1:2], lib=lib)
    got = out.cpu().clone()
    assert float(got[0]) == SENT and float(got[2]) == SENT
    gated(test, workload, "norm_sq", got[1:2].double() - 2.5, ref[torch.float64]["norm_sq"], ref[torch.float32]["norm_sq"])
    ops.sumsq_rows(grads_d, torch.tensor([0], dtype=torch.int32).to(dev), max_rows, d, out[1:2], lib=lib)
    assert torch.equal(out.cpu(), got), "count = 0 adds 0"


# ----------------------------------------------------------------------------- 4. rat_scatter_rows_lists
def check_scatter_rows_lists(lib, dev, d):
    rs = np.random.RandomState(65)
    cap, counts, total_rows = 7, [5, 0, 7], 29
    perm = rs.permutation(total_rows)
    listed = [perm[0:5], perm[0:0], perm[5:12]]
    rows = torch.full((3, cap), int(perm[12]), dtype=torch.int32)       # behind a list's count: a valid row that no list names
    for k, r in enumerate(listed):
        rows[k, :len(r)] = torch.from_numpy(r).int()
    grads = rnd(rs, 3, cap, d)
    want = torch.full((total_rows, d), SENT)
    for k, r in enumerate(listed):
        want[torch.from_numpy(r).long()] = grads[k, :len(r)]
    rows_d, grads_d, counts_d = rows.to(dev), grads.to(dev), torch.tensor(counts, dtype=torch.int32).to(dev)
    block = Guarded(torch.full((total_rows, d), SENT), 0, dev)
    ops.scatter_rows_lists(block.view, rows_d, grads_d, counts_d, d, lib=lib)
    assert block.intact()
    assert torch.equal(block.cpu(), want), "listed rows hold their gradient rows bit for bit, every other row keeps the sentinel"
    single = Guarded(torch.full((total_rows, d), SENT), 0, dev)
    for k in range(3):
        ops.scatter_rows(single.view, rows_d[k], grads_d[k], counts_d[k:k + 1], d, lib=lib)
    assert single.intact() and torch.equal(single.cpu(), block.cpu())


# ----------------------------------------------------------------------------- 5. rat_label_grad
def check_label_grad(lib, dev, nbt, S, d):
    """against a float64 index_add of dgrid[:, 0, :] by label; the gate is summation-order rounding of up to nbt O(1) terms per
    element, the form sparse_cases.check_sorted_reduce uses"""
    test, workload = "optim_cases.check_label_grad", "nbt=%d S=%d d=%d" % (nbt, S, d)
    gate = (1e-5, 1e-6 + 1e-7 * nbt)
    rs = np.random.RandomState(66)
    dgrid = rnd(rs, nbt, S, d)
    labels = torch.from_numpy(rs.randint(0, 3, size=nbt)).int()
    if nbt >= 7:
        labels[3], labels[5], labels[6] = -1, 3, 2           # outside {0, 1, 2}: the kernel clamps (rat_check_ids reports them)
    start = rnd(rs, 3, d)
    ref = start.double().index_add(0, labels.clamp(0, 2).long(), dgrid[:, 0, :].double())
    dgrid_d, labels_d = dgrid.to(dev), labels.to(dev)

    def run():
        out = Guarded(start, 0, dev)                        # it accumulates: the table starts non-zero
        ops.label_grad(dgrid_d, labels_d, out.view, nbt, S, d, lib=lib)
        assert out.intact()
        return out.cpu()
    got = run()
    gated(test, workload, "dlabel_table", got, ref, gate=gate)
    assert torch.equal(run(), got), "rat_label_grad is bit-reproducible"
    # the atomic form inside rat_gather_bwd, from the same inputs
    nf = S - 1
    fields = [F(i, 1, 5) for i in range(nf)]
    gtabs = [torch.zeros(5, d).to(dev) for _ in fields]
    idx = torch.from_numpy(rs.randint(0, 5, size=(nbt, 1, max(nf, 1)))).int().contiguous().to(dev)
    atomic = Guarded(start, 0, dev)
    ops.gather_bwd(dgrid_d, None, idx, labels_d, ops.field_table(fields, gtabs, dev) if nf else None, nf, atomic.view, nbt, 1, max(nf, 1), d,
                   lib=lib)
    assert atomic.intact()
    gated(test, workload, "dlabel_table", got, ref, gate=gate, against=atomic.cpu(), where="against rat_gather_bwd")


# ----------------------------------------------------------------------------- 6. rat_check_ids
def check_check_ids(lib, dev, B, T):
    rs = np.random.RandomState(67)
    L = 6                                                   # column 5 belongs to no field: whatever it holds is never counted
    fields = [F(0, 1, 7), F(1, 3, 6, padding_idx=5), F(4, 1, 9)]
    hi = [7, 6, 6, 6, 9, 1]
    idx = torch.stack([torch.from_numpy(rs.randint(0, hi[c], size=(B, T))) for c in range(L)], -1).int().contiguous()
    idx[..., 5] = -5
    labels = torch.from_numpy(rs.randint(0, 3, size=(B, T))).int()
    # negative, equal to the vocabulary and far above it, in target (t = 0) and retrieved rows, the very last row included
    bad = [(0, 0, 0, -1), (0, 1, 2, 6), (B - 1, T - 1, 4, 1 << 30), (B - 1, 0, 1, -7), (B // 2, T - 1, 3, 6), (B - 1, T - 1, 0, 7)]
    assert len({b[:3] for b in bad}) == len(bad)
    for b, t, c, val in bad:
        idx[b, t, c] = val
    labels[0, 1], labels[B - 1, T - 1] = -1, 3
    tables = [torch.zeros(f.vocab, 1).to(dev) for f in fields]
    ftab = ops.field_table(fields, tables, dev)
    counts = torch.zeros(2, dtype=torch.int32).to(dev)
    idx_d, labels_d = idx.to(dev), labels.to(dev)
    ops.check_ids(idx_d, labels_d, ftab, 3, counts, B, T, L, lib=lib)
    assert counts.cpu().tolist() == [len(bad), 2]
    ops.check_ids(idx_d, labels_d, ftab, 3, counts, B, T, L, lib=lib)
    assert counts.cpu().tolist() == [2 * len(bad), 4], "a second call adds to the counters"


# ----------------------------------------------------------------------------- 7. rat_dropout_dev
def check_dropout_dev(lib, dev, n, p):
    rs = np.random.RandomState(68)
    x = rnd(rs, n)
    assert bool((x != 0).all())
    seed = 0x1234567887654321
    x_d = x.to(dev)
    by_value = ops.dropout(x_d, p, seed, lib=lib).cpu()
    word = torch.tensor([seed], dtype=torch.int64).to(dev)
    y = ops.dropout(x_d, p, word, lib=lib).cpu()
    assert torch.equal(y, by_value), "the seed word in device memory gives the mask of the same seed by value"
    buf = Guarded(x, 1, dev)
    ops.dropout(buf.view, p, word, out=buf.view, lib=lib)
    assert buf.intact() and torch.equal(buf.cpu(), y), "in place == out of place"
    if p == 0:
        assert torch.equal(y, x), "p = 0 is the identity"
        return
    kept = y != 0
    # y = x * fl(1 / fl(1 - p)): the product rounds once (1/2 ulp) and the scale is within 0.8 * 2^-24 of 1 / (1 - p) for the p used here
    # (p = 0.3: 0.4 * 2^-24), at most 0.8 ulp of y more — 1 ulp in all would fail only for a scale more than 2^-25 off
    want = x.double()[kept] / (1.0 - p)
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64))
    assert abs(float(np.float32(1) / (np.float32(1) - np.float32(p))) * (1.0 - p) - 1.0) <= 2.0 ** -25
    assert bool(((y.double()[kept] - want).abs() <= ulp).all()), "kept elements are x / (1 - p) within 1 ulp"
    frac = float(kept.double().mean())
    bound = 5.0 * math.sqrt(p * (1.0 - p) / n)              # five standard deviations of a Bernoulli(1 - p) mean over n draws
    assert abs(frac - (1.0 - p)) <= bound, (frac, 1.0 - p, bound)
