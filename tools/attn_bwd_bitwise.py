#!/usr/bin/env python3
"""Diagnostic: another build of the library (the parent commit's, say) against this tree's in one process, the same seeded inputs through
both: every output of rat_attn_bwd_ex — dx, the five parameter gradients, the workspace with the gradient slabs — bit for bit, at the shapes
of tests/test_gpu_attn_bwd_addr.py.

    python tools/attn_bwd_bitwise.py <path of the other librat_hip.so>

Never used by the product or the tests."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "www24-rat_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kernel_cases as kc  # noqa: E402
import test_gpu_attn_bwd_addr as T  # noqa: E402
from rat_amd import ops  # noqa: E402
from rat_amd._lib import RatLib  # noqa: E402

parent = RatLib(sys.argv[1])
new = RatLib(os.path.join(ROOT, "www24-rat_amd", "lib", "librat_hip.so"))
dev = "cuda"
NAMES = ["dx", "d_gamma", "d_beta", "dW_qkv", "dW_out", "d_bias", "slabs"]


def knob(lib, name, value):
    fn = lib.cdll.rat_debug_set_knob
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]
    assert fn(name.encode(), int(value)) != -2 ** 31


def run(lib, form, x, dy, add, o_save, lse, wd, smap, d):
    gs = [torch.zeros_like(w) for w in wd]
    need = lib.size("rat_attn_bwd_workspace", d, T.HEADS, T.DH)
    ws = torch.zeros((need + 3) // 4, dtype=torch.float32, device=dev)
    params = ops.attn_params(*wd)
    if form == "plain":
        dx, ws = ops.attn_bwd(x, dy, o_save, lse, params, ops.attn_params(*gs), smap, d, T.HEADS, T.DH, workspace=ws, arith="bf16x3", lib=lib)
    else:
        dx, ws = ops.attn_bwd_ex(x, dy, add, o_save, lse, params, ops.attn_params(*gs), smap, d, T.HEADS, T.DH, 0.4, 0.5, workspace=ws,
                                 arith="bf16x3", dropout=(0.25, 987654321), lib=lib)
    torch.cuda.synchronize()
    return [dx] + gs + [ws]


rows = [(n, None) for n in T.PLAIN] + [(n, q) for n, q in T.QUERIES] + [(n, None) for n in T.DPAD]
print("# case            form   " + " ".join(NAMES))
bad = 0
for name, nq in rows:
    (B, Tt, S), mode, mb, d = T.CASES[name]
    for lib in (parent, new):
        knob(lib, "max_blocks", mb)
    rs = np.random.RandomState(7)
    x, dy, add = (kc.rnd(rs, B, Tt, S, d).to(dev) for _ in range(3))
    wd = [w.to(dev) for w in kc.attn_weights(rs, d, T.HEADS, T.DH, True)]
    smap = ops.intra_map(B, Tt, S) if mode == "intra" else ops.cross_map(B, Tt, S)
    if nq is not None:
        if mode == "intra":
            smap = ops.intra_map(B, Tt, S, queries=nq)
            dy[:, :, nq:, :] = 0.0
        else:
            smap.queries = nq
            dy[:, nq:, :, :] = 0.0
    for form in ("plain", "ex"):
        params = ops.attn_params(*wd)
        if form == "plain":
            _, o_save, lse = ops.attn_fwd(x, params, smap, d, T.HEADS, T.DH, save=True, arith="bf16x3", lib=new)
        else:
            _, o_save, lse = ops.attn_fwd_ex(x, add, params, smap, d, T.HEADS, T.DH, 0.4, 0.5, save=True, arith="bf16x3",
                                             dropout=(0.25, 987654321), lib=new)
        a = run(parent, form, x, dy, add, o_save, lse, wd, smap, d)
        b = run(new, form, x, dy, add, o_save, lse, wd, smap, d)
        res = []
        for u, v in zip(a, b):
            ok = torch.equal(u, v) and bool(torch.isfinite(u).all()) and bool((u != 0).any())
            bad += 0 if ok else 1
            res.append("equal" if ok else "DIFFERENT")
        print("%-17s %-6s " % (name + (":nq%d" % nq if nq is not None else ""), form) + " ".join(res), flush=True)
print("RESULT: " + ("all bit-equal" if bad == 0 else "%d DIFFERENT" % bad))
sys.exit(1 if bad else 0)
