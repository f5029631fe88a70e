"""AUC / logloss with the reference's definitions (fuxictr/metrics.py:22-41): roc_auc_score, and log_loss with
predictions clipped to [1e-7, 1-1e-7] (the ``eps=1e-7`` of the sklearn the reference pinned; newer sklearn
dropped that kwarg, so the clip is explicit here), plus GAUC, which the reference names and leaves unimplemented
(fuxictr/metrics.py:29-39): the per-group AUC weighted by the groups' rows, as later FuxiCTR releases define it.

Two implementations of one contract: ``evaluate_metrics`` in numpy on the host, and ``device_metrics`` on the device
(``ops.eval_metrics`` -> csrc/metrics.hip: one launch chain over the device vectors, 64 bytes read back).  The host one is the
default of every caller and the reference of the device one's parity tests.

Ranking metrics per group, as later FuxiCTR releases report them beside gAUC — ``NDCG(k=K)``, ``MRR(k=K)``, ``HitRate(k=K)``, K a positive
integer — under the same two-implementation contract (``ops.eval_rank_metrics`` -> csrc/rankmetrics.hip, 64 bytes per cutoff read back):

  order   : inside a group ``np.argsort(-p_g, kind="stable")`` over the group's rows in input order — descending prediction, ties keep
            input order, -0.0 equal to +0.0 (the order ``rank_requests`` documents).  A row's place r is 0-based.
  counted : a group counts if it holds at least one positive (y == 1); a group without one is skipped.  Each metric is the unweighted
            mean over the counted groups.  A cutoff K >= n means "no cutoff".
  for a counted group with P positives and f the place of its first positive:
            DCG@k = sum_{r < k, y_r = 1} 1 / log2(r + 2),  IDCG@k = sum_{j < min(P, k)} 1 / log2(j + 2),  NDCG@k = DCG@k / IDCG@k,
            MRR@k = 1 / (f + 1) if f < k else 0,  HitRate@k = 1 if f < k else 0.  All arithmetic is float64."""
import logging
import re

import numpy as np


def auc_score(y_true, y_pred):
    y_true = np.asarray(y_true, dtype=np.float64).reshape(-1)
    y_pred = np.asarray(y_pred, dtype=np.float64).reshape(-1)
    order = np.argsort(y_pred, kind="mergesort")
    sorted_pred = y_pred[order]
    # average ranks over ties
    boundaries = np.concatenate([[True], sorted_pred[1:] != sorted_pred[:-1], [True]])
    starts = np.flatnonzero(boundaries[:-1])
    ends = np.flatnonzero(boundaries[1:])
    avg = 0.5 * (starts + ends) + 1.0
    group = np.cumsum(boundaries[:-1]) - 1
    ranks = np.empty_like(sorted_pred)
    ranks[order] = avg[group]
    pos = y_true == 1
    n_pos = float(pos.sum())
    n_neg = float(len(y_true) - n_pos)
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return float((ranks[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def log_loss(y_true, y_pred, eps=1e-7):
    y_true = np.asarray(y_true, dtype=np.float64).reshape(-1)
    p = np.clip(np.asarray(y_pred, dtype=np.float64).reshape(-1), eps, 1 - eps)
    return float(-(y_true * np.log(p) + (1 - y_true) * np.log(1 - p)).mean())


def gauc_score(y_true, y_pred, group_index):
    """sum_g n_g AUC_g / sum_g n_g over the groups that hold both classes (n_g = the rows of group g); ValueError when none does.
    One lexsort by (group, prediction), no loop over the groups; every AUC_g is the quotient of the exact integers auc_score divides:
    U2_g = sum over the group's runs of equal predictions of pos_run * (2 * neg_before_run + neg_run), AUC_g = U2_g / (2 pos_g neg_g)."""
    y_true = np.asarray(y_true, dtype=np.float64).reshape(-1)
    y_pred = np.asarray(y_pred, dtype=np.float64).reshape(-1)
    group_index = np.asarray(group_index).reshape(-1)
    n = len(y_true)
    if len(group_index) != n:
        raise ValueError("group_index holds %d entries for %d rows" % (len(group_index), n))
    order = np.lexsort((y_pred, group_index))
    g, p, neg = group_index[order], y_pred[order], y_true[order] != 1
    group_head = np.concatenate([[True], g[1:] != g[:-1]])
    run_head = group_head | np.concatenate([[True], p[1:] != p[:-1]])
    neg_before = np.concatenate([[0], np.cumsum(neg, dtype=np.int64)])            # negatives in [0, i)
    run_start, group_start = np.flatnonzero(run_head), np.flatnonzero(group_head)
    run_end, group_end = np.append(run_start[1:], n), np.append(group_start[1:], n)
    first_run = np.searchsorted(run_start, group_start)                           # a group's first run starts where the group does
    group_of_run = np.cumsum(group_head)[run_start] - 1
    neg_run = neg_before[run_end] - neg_before[run_start]
    pos_run = (run_end - run_start) - neg_run
    terms = pos_run * (2 * (neg_before[run_start] - neg_before[group_start[group_of_run]]) + neg_run)
    u2 = np.add.reduceat(terms, first_run)
    rows = group_end - group_start
    n_neg = neg_before[group_end] - neg_before[group_start]
    n_pos = rows - n_neg
    both = (n_pos > 0) & (n_neg > 0)
    if not both.any():
        raise ValueError("No group holds both classes. GAUC is not defined in that case.")
    auc = u2[both] / (2.0 * n_pos[both] * n_neg[both])
    return float((rows[both] * auc).sum() / rows[both].sum())


class _RankedRows:
    """the rows sorted by (group, descending prediction, input order) — one stable lexsort, no loop over the groups — and what every cutoff
    shares: each row's place in its group, each positive's index among its group's positives, the groups' first rows"""

    def __init__(self, y_true, y_pred, group_index):
        y_true = np.asarray(y_true, dtype=np.float64).reshape(-1)
        y_pred = np.asarray(y_pred, dtype=np.float64).reshape(-1)
        group_index = np.asarray(group_index).reshape(-1)
        n = len(y_true)
        if len(group_index) != n or len(y_pred) != n:
            raise ValueError("group_index holds %d entries and y_pred %d for %d rows" % (len(group_index), len(y_pred), n))
        if np.isnan(y_pred).any():
            raise ValueError("Input y_pred contains NaN.")
        if not ((y_true == 0) | (y_true == 1)).all():
            raise ValueError("y_true holds a label that is neither 0 nor 1.")
        order = np.lexsort((-y_pred, group_index))                                 # stable: ties keep input order; -0.0 == +0.0
        g, self.pos = group_index[order], y_true[order] == 1
        self.start = np.flatnonzero(np.concatenate([[True], g[1:] != g[:-1]])) if n else np.zeros(0, dtype=np.int64)
        rows = np.diff(np.append(self.start, n))
        self.place = np.arange(n) - np.repeat(self.start, rows)
        pos_before = np.concatenate([[0], np.cumsum(self.pos, dtype=np.int64)])    # positives in [0, i)
        self.nth = pos_before[:-1] - np.repeat(pos_before[self.start], rows)
        self.first = np.flatnonzero(self.pos & (self.nth == 0))                    # one row per counted group: its first positive
        if len(self.first) == 0:
            raise ValueError("No group holds a positive. NDCG, MRR and HitRate are not defined in that case.")
        self.counted = np.add.reduceat(self.pos, self.start) > 0

    def scores(self, k):
        """-> (NDCG@k, MRR@k, HitRate@k)"""
        k = _cutoff(k)
        dcg = np.where(self.pos & (self.place < k), 1.0 / np.log2(self.place + 2.0), 0.0)
        idcg = np.where(self.pos & (self.nth < k), 1.0 / np.log2(self.nth + 2.0), 0.0)
        dcg, idcg = np.add.reduceat(dcg, self.start)[self.counted], np.add.reduceat(idcg, self.start)[self.counted]
        f = self.place[self.first]
        hit = f < k
        return float((dcg / idcg).mean()), float(np.where(hit, 1.0 / (f + 1.0), 0.0).mean()), float(hit.sum() / float(len(f)))


def _cutoff(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
        raise ValueError("a cutoff k is a positive integer, got %r" % (k,))
    return int(k)


def ndcg_score(y_true, y_pred, group_index, k):
    """the mean over the groups that hold a positive of DCG@k / IDCG@k (binary relevance, the module's definitions); ValueError when
    no group holds one, a prediction is NaN or a label is neither 0 nor 1"""
    return _RankedRows(y_true, y_pred, group_index).scores(k)[0]


def mrr_score(y_true, y_pred, group_index, k):
    """the mean over the groups that hold a positive of 1 / (place of the first positive + 1), 0 where that place is >= k"""
    return _RankedRows(y_true, y_pred, group_index).scores(k)[1]


def hitrate_score(y_true, y_pred, group_index, k):
    """the share of the groups that hold a positive whose first positive sits at a place < k"""
    return _RankedRows(y_true, y_pred, group_index).scores(k)[2]


_RANK_NAME = re.compile(r"^(NDCG|MRR|HitRate)\(k=([1-9][0-9]*)\)$")
_RANK_SLOT = {"NDCG": 0, "MRR": 1, "HitRate": 2}


def rank_metric(metric):
    """"NDCG(k=10)" -> ("NDCG", 10); any other name (the bare "NDCG" included) -> None"""
    m = _RANK_NAME.match(metric) if isinstance(metric, str) else None
    return (m.group(1), int(m.group(2))) if m else None


def is_grouped(metric):
    """does the metric need group_index?"""
    return metric == "GAUC" or rank_metric(metric) is not None


def evaluate_metrics(y_true, y_pred, metrics, group_index=None, **kwargs):
    result = dict()
    ranked = None
    for metric in metrics:
        if metric in ("logloss", "binary_crossentropy"):
            result[metric] = log_loss(y_true, y_pred, eps=1e-7)
        elif metric == "AUC":
            result[metric] = auc_score(y_true, y_pred)
        elif metric == "GAUC" and group_index is not None:
            result[metric] = gauc_score(y_true, y_pred, group_index)
        elif rank_metric(metric) is not None and group_index is not None:
            kind, k = rank_metric(metric)
            ranked = ranked or _RankedRows(y_true, y_pred, group_index)           # one sort for every ranking name of the call
            result[metric] = ranked.scores(k)[_RANK_SLOT[kind]]
        else:
            raise NotImplementedError("metric=%s is outside the RAT_m2 hot path" % metric)
    logging.info("[Metrics] " + " - ".join("{}: {:.6f}".format(k, v) for k, v in result.items()))
    return result


_SLOT = {"logloss": 0, "binary_crossentropy": 0, "AUC": 1, "GAUC": 2}
_MAX_CUTOFF = 2 ** 31 - 1                                # the C ABI's largest; a cutoff >= n means "no cutoff" and n <= 2^31 - 1


def device_metrics(y_true, y_pred, metrics, group_index=None, lib=None):
    """``evaluate_metrics`` computed on the device: y_true, y_pred fp32 tensors [n] (group_index int32 [n], needed for "GAUC" and the
    ranking names) where they already are; one 64-byte copy comes back, and one of 64 bytes per distinct cutoff when ranking names are
    asked for (their chain runs once for all of them).  Raises what the host functions raise: ValueError when only one class is present
    (``auc_score``'s words), when a prediction is NaN, a label is neither 0 nor 1, no group holds both classes, or none a positive."""
    import torch
    from . import ops
    for metric in metrics:
        if (metric not in _SLOT and rank_metric(metric) is None) or (is_grouped(metric) and group_index is None):
            raise NotImplementedError("metric=%s is outside the RAT_m2 hot path" % metric)
    y_pred = y_pred.detach().reshape(-1).to(torch.float32).contiguous()
    y_true = y_true.detach().reshape(-1).to(device=y_pred.device, dtype=torch.float32).contiguous()
    group = None
    if any(is_grouped(m) for m in metrics):
        group = group_index.detach().reshape(-1).to(device=y_pred.device, dtype=torch.int32).contiguous()
    result, status, rows = {}, 0, {}
    if any(m in _SLOT for m in metrics):
        out = ops.eval_metrics(y_pred, y_true, group if "GAUC" in metrics else None, lib=lib).cpu().numpy()      # the one copy: 8 doubles
        status = int(out[7])
    cutoffs = sorted({min(rank_metric(m)[1], _MAX_CUTOFF) for m in metrics if rank_metric(m) is not None})
    for at in range(0, len(cutoffs), ops.MAX_CUTOFFS):                            # (one call unless more than 8 distinct cutoffs are named)
        part = cutoffs[at:at + ops.MAX_CUTOFFS]
        got = ops.eval_rank_metrics(y_pred, y_true, group, part, lib=lib).cpu().numpy()                          # 8 doubles per cutoff
        rows.update({k: got[i] for i, k in enumerate(part)})
        status |= int(got[0][7])
    if status & 1:
        raise ValueError("Input y_pred contains NaN.")
    if status & 2:
        raise ValueError("y_true holds a label that is neither 0 nor 1.")
    ranked = [m for m in metrics if m in ("AUC", "GAUC")]
    if status & 4 and ranked:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    if status & 8 and "GAUC" in metrics:
        raise ValueError("No group holds both classes. GAUC is not defined in that case.")
    if status & 16:
        raise ValueError("No group holds a positive. NDCG, MRR and HitRate are not defined in that case.")
    for metric in metrics:
        if metric in _SLOT:
            result[metric] = float(out[_SLOT[metric]])
        else:
            kind, k = rank_metric(metric)
            result[metric] = float(rows[min(k, _MAX_CUTOFF)][_RANK_SLOT[kind]])
    logging.info("[Metrics] " + " - ".join("{}: {:.6f}".format(k, v) for k, v in result.items()))
    return result
