"""AUC / logloss with the reference's definitions (fuxictr/metrics.py:22-41): roc_auc_score, and log_loss with
predictions clipped to [1e-7, 1-1e-7] (the ``eps=1e-7`` of the sklearn the reference pinned; newer sklearn
dropped that kwarg, so the clip is explicit here), plus GAUC, which the reference names and leaves unimplemented
(fuxictr/metrics.py:29-39): the per-group AUC weighted by the groups' rows, as later FuxiCTR releases define it.

Two implementations of one contract: ``evaluate_metrics`` in numpy on the host, and ``device_metrics`` on the device
(``ops.eval_metrics`` -> csrc/metrics.hip: one launch chain over the device vectors, 64 bytes read back).  The host one is the
default of every caller and the reference of the device one's parity tests."""
import logging

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


def evaluate_metrics(y_true, y_pred, metrics, group_index=None, **kwargs):
    result = dict()
    for metric in metrics:
        if metric in ("logloss", "binary_crossentropy"):
            result[metric] = log_loss(y_true, y_pred, eps=1e-7)
        elif metric == "AUC":
            result[metric] = auc_score(y_true, y_pred)
        elif metric == "GAUC" and group_index is not None:
            result[metric] = gauc_score(y_true, y_pred, group_index)
        else:
            raise NotImplementedError("metric=%s is outside the RAT_m2 hot path" % metric)
    logging.info("[Metrics] " + " - ".join("{}: {:.6f}".format(k, v) for k, v in result.items()))
    return result


_SLOT = {"logloss": 0, "binary_crossentropy": 0, "AUC": 1, "GAUC": 2}


def device_metrics(y_true, y_pred, metrics, group_index=None, lib=None):
    """``evaluate_metrics`` computed on the device: y_true, y_pred fp32 tensors [n] (group_index int32 [n], needed for "GAUC") where
    they already are; one 64-byte copy comes back.  Raises what the host functions raise: ValueError when only one class is present
    (``auc_score``'s words), when a prediction is NaN, a label is neither 0 nor 1, or no group holds both classes."""
    import torch
    from . import ops
    for metric in metrics:
        if metric not in _SLOT or (metric == "GAUC" and group_index is None):
            raise NotImplementedError("metric=%s is outside the RAT_m2 hot path" % metric)
    y_pred = y_pred.detach().reshape(-1).to(torch.float32).contiguous()
    y_true = y_true.detach().reshape(-1).to(device=y_pred.device, dtype=torch.float32).contiguous()
    group = None
    if "GAUC" in metrics:
        group = group_index.detach().reshape(-1).to(device=y_pred.device, dtype=torch.int32).contiguous()
    out = ops.eval_metrics(y_pred, y_true, group, lib=lib).cpu().numpy()          # the one copy: 8 doubles
    status = int(out[7])
    if status & 1:
        raise ValueError("Input y_pred contains NaN.")
    if status & 2:
        raise ValueError("y_true holds a label that is neither 0 nor 1.")
    ranked = [m for m in metrics if m in ("AUC", "GAUC")]
    if status & 4 and ranked:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    if status & 8 and "GAUC" in metrics:
        raise ValueError("No group holds both classes. GAUC is not defined in that case.")
    result = {metric: float(out[_SLOT[metric]]) for metric in metrics}
    logging.info("[Metrics] " + " - ".join("{}: {:.6f}".format(k, v) for k, v in result.items()))
    return result
