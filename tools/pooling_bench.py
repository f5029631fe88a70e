#!/usr/bin/env python3
"""Diagnostic: what MaskedAveragePooling costs on the kernels it touches, at the KKBox-real geometry (B 4096, K 5 -> T 6, d 40,
13 fields of 7076 rows; genre_ids and artist_name — fields 9 and 10 — as bags of 3 ids, as in kkbox_x1.yaml).  Every line is timed
with both bags summed (the sum-only entry points) and with both averaged (the *_pool entry points).

    python tools/pooling_bench.py [--reps 50] [--B 4096]

Never used by the product or the tests; bench.py is the contract benchmark."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "www24-rat_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402
from rat_amd import ops  # noqa: E402
from rat_amd._lib import get_lib  # noqa: E402


class Field:
    def __init__(self, col, ncols, vocab, padding_idx, pooling):
        self.col, self.ncols, self.vocab, self.padding_idx, self.pooling = col, ncols, vocab, padding_idx, pooling


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--B", type=int, default=4096)
    args = ap.parse_args()
    lib, dev = get_lib(), "cuda:0"
    B, T, d, F, vocab, bag = args.B, 6, 40, 13, 92_000 // 13, 3
    g = torch.Generator().manual_seed(0)

    def fields_for(pooling):
        out, col = [], 0
        for i in range(F):
            n = bag if i in (9, 10) else 1
            out.append(Field(col, n, vocab, vocab - 1 if n > 1 else None, pooling if n > 1 else "sum"))
            col += n
        return out

    fs_sum, fs_avg = fields_for("sum"), fields_for("average")
    L = fs_sum[-1].col + 1
    tables = [torch.randn(vocab, d, generator=g).to(dev) for _ in range(F)]
    lr_tables = [torch.randn(vocab, 1, generator=g).to(dev) for _ in range(F)]
    for f, t, w in zip(fs_sum, tables, lr_tables):
        if f.padding_idx is not None:
            t[f.padding_idx] = 0
            w[f.padding_idx] = 0
    idx = torch.randint(0, vocab, (B, T, L), generator=g, dtype=torch.int32).to(dev)
    labels = torch.randint(0, 3, (B, T), generator=g, dtype=torch.int32).to(dev)
    label_table = torch.randn(3, d, generator=g).to(dev)
    ftab = ops.field_table(fs_sum, tables, dev)
    lr_ftab = ops.field_table(fs_sum, lr_tables, dev)
    gtabs = [torch.zeros_like(t) for t in tables]
    gftab = ops.field_table(fs_sum, gtabs, dev)
    glr = [torch.zeros_like(t) for t in lr_tables]
    lr_gftab = ops.field_table(fs_sum, glr, dev)
    modes = ops.pool_modes(fs_avg, dev)
    avg = torch.tensor([9, 10], dtype=torch.int32, device=dev)
    dgrid = torch.randn(B, T, F + 1, d, generator=g).to(dev)
    dflat = torch.randn(B, F * d, generator=g).to(dev)
    cls = torch.randn(B, d, generator=g).to(dev)
    fc_w, fc_b = torch.randn(1, d, generator=g).to(dev), torch.zeros(1, device=dev)
    y_true = torch.randint(0, 2, (B, 1), generator=g).float().to(dev)
    loss = torch.zeros(1, device=dev)
    lr_den = torch.empty(B, F, device=dev)
    y_pred = ops.logit_fwd(cls, d, fc_w, fc_b, None, lr_ftab, F, idx, T * L, y_true, loss, B, d, lib=lib)
    dcls, dfc_w, dfc_b = torch.empty(B, d, device=dev), torch.zeros(1, d, device=dev), torch.zeros(1, device=dev)
    lab = torch.zeros(3, d, device=dev)

    rows = [
        ("gather_fwd", lambda: ops.gather_fwd(idx, labels, ftab, F, label_table, B, T, L, d, lib=lib),
         lambda: ops.gather_fwd(idx, labels, ftab, F, label_table, B, T, L, d, modes=modes, lib=lib)),
        ("scale_bwd (averaged rows)", None,
         lambda: ops.pool_scale_bwd(dgrid, dflat, idx, ftab, avg, F, B, T, L, d, lib=lib)),
        ("gather_bwd (atomic)", lambda: ops.gather_bwd(dgrid, dflat, idx, labels, gftab, F, lab, B, T, L, d, lib=lib), None),
        ("logit_fwd (+LR)", lambda: ops.logit_fwd(cls, d, fc_w, fc_b, None, lr_ftab, F, idx, T * L, y_true, loss, B, d, lib=lib),
         lambda: ops.logit_fwd(cls, d, fc_w, fc_b, None, lr_ftab, F, idx, T * L, y_true, loss, B, d, modes=modes, lr_den=lr_den,
                               lib=lib)),
        ("logit_bwd (+LR atomics)", lambda: ops.logit_bwd(y_pred, y_true, cls, d, fc_w, dcls, d, dfc_w, dfc_b, lr_gftab, F, idx, T * L,
                                                          1.0, B, d, lib=lib),
         lambda: ops.logit_bwd(y_pred, y_true, cls, d, fc_w, dcls, d, dfc_w, dfc_b, lr_gftab, F, idx, T * L, 1.0, B, d, lr_den=lr_den,
                               lib=lib)),
    ]
    print("# KKBox-real geometry: B %d, T %d, d %d, %d fields (two bags of %d), %d reps; microseconds per launch" % (B, T, d, F, bag,
                                                                                                                    args.reps))
    print("%-28s %12s %12s" % ("kernel", "sum", "average"))
    for name, fs, fa in rows:
        ts = timeit(fs, args.reps) if fs else float("nan")
        ta = timeit(fa, args.reps) if fa else float("nan")
        print("%-28s %12.1f %12.1f" % (name, ts, ta))


if __name__ == "__main__":
    main()
