#!/usr/bin/env python3
"""Evaluation metrics: today's host path against the device chain, end to end.

    python tools/metrics_bench.py [--sizes 100000,1000000,10000000] [--out FILE] [--rank]

For every N and every grouping (none, 10^4 groups, N / 10 groups), two sides over the SAME device vectors:
  (a) host  : the copy evaluate_generator makes (y_pred / y_true widened to float64 on the device, copied to the host; the group ids
              as int32) followed by metrics.evaluate_metrics;
  (b) device: metrics.device_metrics — the launch chain of rat_eval_metrics plus its 64-byte read-back.
Timed with the host clock around calls that end in a synchronise (side (a) ends in numpy, side (b) in the read-back; a
torch.cuda.synchronize() follows both), the sides alternating in rounds; min, median and max of the per-call time over the rounds.
--rank measures the ranking names instead: N / 10 groups, one cutoff (10) and four cutoffs (1, 5, 10, 50), every K with its three names
NDCG(k=K), MRR(k=K), HitRate(k=K); (b) is then the launch chain of rat_eval_rank_metrics plus its 64-byte read-back per cutoff.
No ratio is gated: the table is what was measured.  Needs a GPU: there is no fallback."""
import argparse
import logging
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "www24-rat_amd"))


def make(n, groups, device, seed=0):
    rs = np.random.RandomState(seed)
    p = rs.rand(n).astype(np.float32)
    y = (rs.rand(n) < 0.25 + 0.5 * p).astype(np.float32)                             # labels that follow the predictions: AUC ~ 0.67
    g = None if groups is None else rs.randint(0, groups, size=n).astype(np.int32)
    up = lambda a: None if a is None else torch.from_numpy(a).to(device)             # noqa: E731
    return up(p), up(y), up(g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.25, help="seconds of calls per side and round (at least one call)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rank", action="store_true", help="the ranking names NDCG / MRR / HitRate instead of logloss / AUC / GAUC")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/metrics_bench.py measures on a GPU; none is visible")
    from rat_amd import metrics
    logging.getLogger().setLevel(logging.WARNING)
    device = "cuda:0"
    lines = ["tools/metrics_bench.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "per call [ms]: min / median / max over the rounds, host clock + synchronise, sides alternating; (a) = D2H copy of the vectors + "
             "metrics.evaluate_metrics, (b) = metrics.device_metrics (chain + 64-byte read-back)"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    for n in [int(x) for x in args.sizes.split(",")]:
        plans = [("ungrouped", None, None), ("10^4 groups", 10 ** 4, None), ("N/10 groups", n // 10, None)]
        if args.rank:
            plans = [("k = 10", n // 10, (10,)), ("k = 1,5,10,50", n // 10, (1, 5, 10, 50))]
        for label, groups, cutoffs in plans:
            y_pred, y_true, group = make(n, groups, device)
            names = ["logloss", "AUC"] + ([] if group is None else ["GAUC"])
            if cutoffs:
                names = ["%s(k=%d)" % (kind, k) for k in cutoffs for kind in ("NDCG", "MRR", "HitRate")]

            def host():
                yp = y_pred.double().cpu().numpy()
                yt = y_true.double().cpu().numpy()
                gi = None if group is None else group.cpu().numpy()
                return metrics.evaluate_metrics(yt, yp, names, group_index=gi)

            def dev():
                return metrics.device_metrics(y_true, y_pred, names, group_index=group)

            def timed(fn, calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    r = fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / calls, r

            calls, results = {}, {}
            for name, fn in (("a", host), ("b", dev)):                                # warm-up, and the calls a round holds
                t, results[name] = timed(fn, 1)
                if t < 1.0:
                    t, results[name] = timed(fn, 1)
                calls[name] = max(1, min(500, int(args.budget / max(t, 1e-6))))
            times = {"a": [], "b": []}
            for r in range(args.rounds):
                for name, fn in ((("a", host), ("b", dev)) if r % 2 == 0 else (("b", dev), ("a", host))):
                    times[name].append(timed(fn, calls[name])[0] * 1e3)
            a, b = results["a"], results["b"]
            diffs = " ".join("%s %.3g" % (k, abs(a[k] - b[k])) for k in names)
            if cutoffs:
                diffs = "worst NDCG %.3g, MRR %.3g; HitRate equal: %s" % tuple(
                    [max(abs(a[k] - b[k]) for k in names if k.startswith(kind)) for kind in ("NDCG", "MRR")]
                    + [all(a[k] == b[k] for k in names if k.startswith("HitRate"))])
            fmt = lambda v: "%.3f / %.3f / %.3f" % (min(v), statistics.median(v), max(v))      # noqa: E731
            tail = "" if cutoffs else " | AUC equal: %s" % (a["AUC"] == b["AUC"])
            emit("N %9d %-12s | (a) host %s (%d calls x %d rounds) | (b) device %s (%d calls x %d rounds) | |a - b|: %s%s"
                 % (n, label, fmt(times["a"]), calls["a"], args.rounds, fmt(times["b"]), calls["b"], args.rounds, diffs, tail))
            del y_pred, y_true, group
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
