"""Tensor-level wrappers over the C ABI (include/rat_hip.h).  No arithmetic happens here: every function checks
layout/dtype, takes raw ``data_ptr()``s plus the current HIP stream and calls into librat_hip.so.

``lib`` defaults to the process-wide HIP library; tests may pass another ``RatLib`` (the host-emulation build).
"""
import ctypes

import numpy as np
import torch

from ._lib import RatAttnParams, RatSeqMap, RatSplitJob, get_lib

FIELD_DTYPE = np.dtype([("table", "<u8"), ("col", "<i4"), ("ncols", "<i4"), ("vocab", "<i4"), ("padding_idx", "<i4")])
assert FIELD_DTYPE.itemsize == 24


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(t):
    if t.is_cuda:
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return None


def _chk(t, dtype=torch.float32, name="tensor"):
    if t is None:
        return
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def field_table(fields, tables, device):
    """Device array of RatField records.  fields: objects with .col/.ncols/.vocab/.padding_idx; tables: tensors."""
    arr = np.zeros(len(fields), dtype=FIELD_DTYPE)
    for i, (f, t) in enumerate(zip(fields, tables)):
        _chk(t, name="table")
        arr[i] = (t.data_ptr(), f.col, f.ncols, f.vocab, -1 if f.padding_idx is None else f.padding_idx)
    raw = torch.from_numpy(arr.view(np.uint8).copy())
    return raw.to(device)


def intra_map(B, T, S, queries=0):
    """queries: RatSeqMap.queries — 0 = every position; n: only the outputs of positions [0, n) of each sequence are wanted"""
    return RatSeqMap(nseq=B * T, L=S, queries=queries, q_div=B * T, hi_stride=0, lo_stride=S, pos_stride=1)


def cross_map(B, T, S):
    return RatSeqMap(nseq=B * S, L=T, q_div=S, hi_stride=T * S, lo_stride=1, pos_stride=S)


def cross_map_label_token(B, T, S, queries=0):
    """the cross-sample sequences of token position 0 (the label / class token) only: B sequences of T tokens, S tokens apart"""
    return RatSeqMap(nseq=B, L=T, queries=queries, q_div=1, hi_stride=T * S, lo_stride=0, pos_stride=S)


def intra_map_target_sample(B, T, S, queries=0):
    """the intra-sample sequences of retrieved-sample index 0 (the target) only: B sequences of S tokens"""
    return RatSeqMap(nseq=B, L=S, queries=queries, q_div=1, hi_stride=T * S, lo_stride=0, pos_stride=1)


def attn_params(ln_g, ln_b, w_qkv, w_out, b_out, planes=None):
    """planes: optional uint8 tensor of ``attn_planes_bytes`` bytes holding the bf16x3 fragment planes of these weights (filled by
    ``split_weights_batch`` from ``attn_split_jobs``); without it the bf16x3 entry points split the weights on every call."""
    for t in (ln_g, ln_b, w_qkv, w_out, b_out):
        _chk(t, name="attention parameter")
    return RatAttnParams(ln_g.data_ptr(), ln_b.data_ptr(), w_qkv.data_ptr(),
                         w_out.data_ptr() if w_out is not None else None,
                         b_out.data_ptr() if b_out is not None else None,
                         planes.data_ptr() if planes is not None else None)


# ----------------------------------------------------------------------------- bf16x3 weight planes, once per step
def attn_planes_bytes(d, heads, dim_head, lib=None):
    return (lib or get_lib()).size("rat_attn_planes_bytes", d, heads, dim_head)


def ffn_planes_bytes(d, hidden, lib=None):
    return (lib or get_lib()).size("rat_ffn_planes_bytes", d, hidden)


def attn_split_jobs(params, d, heads, dim_head, planes, lib=None):
    """-> list of RatSplitJob that fill ``planes`` (uint8 tensor, 16-byte aligned) from the weights of ``params``"""
    lib = lib or get_lib()
    jobs = (RatSplitJob * 4)()
    n = lib.cdll.rat_attn_split_jobs(ctypes.byref(params), d, heads, dim_head, _p(planes), jobs)
    if n < 0:
        raise RuntimeError("rat_attn_split_jobs: " + lib.last_error())
    return [jobs[i] for i in range(n)]


def attn_groups_planes_bytes(d, heads, dim_head, lib=None):
    """bytes of the per-group [W_qkv | W_out] fragment planes attn_fwd_groups reads; 0: that form does not serve these dimensions"""
    return (lib or get_lib()).size("rat_attn_groups_planes_bytes", d, heads, dim_head)


def attn_groups_split_jobs(params, d, heads, dim_head, planes, lib=None):
    """-> list of RatSplitJob (4 per head group) that fill ``planes`` from the FULL-width weights of ``params``, in place"""
    lib = lib or get_lib()
    jobs = (RatSplitJob * (4 * max(heads // 8, 1)))()
    n = lib.cdll.rat_attn_groups_split_jobs(ctypes.byref(params), d, heads, dim_head, _p(planes), jobs)
    if n < 0:
        raise RuntimeError("rat_attn_groups_split_jobs: " + lib.last_error())
    return [jobs[i] for i in range(n)]


def ffn_split_jobs(w1, w2, d, hidden, planes, lib=None):
    lib = lib or get_lib()
    jobs = (RatSplitJob * 3)()
    n = lib.cdll.rat_ffn_split_jobs(_p(w1), _p(w2), d, hidden, _p(planes), jobs)
    if n < 0:
        raise RuntimeError("rat_ffn_split_jobs: " + lib.last_error())
    return [jobs[i] for i in range(n)]


def split_job_array(jobs):
    """a ctypes array that can be kept and replayed every step (the pointers inside must stay valid)"""
    arr = (RatSplitJob * max(len(jobs), 1))()
    for i, j in enumerate(jobs):
        arr[i] = j
    return arr, len(jobs)


def split_weights_batch(job_array, njobs, like, lib=None):
    """ONE launch for every job; `like`: any tensor on the target device (stream selection)"""
    if njobs:
        (lib or get_lib()).call("rat_split_weights_batch", job_array, njobs, _stream(like))


# ----------------------------------------------------------------------------- K0
def batch_assemble(data_ids, data_labels, pool_ids, pool_labels, retr_indices, rows, header=None, ring=False, lib=None):
    """Device-side Dataset.__getitem__ + collate: -> (idx [B,1+K,L] int32, label_ids [B,1+K] int32, y_true [B] fp32).
    ``header`` (int64, device): the pool's row count is header[0], read on the device — a negative neighbour counts back from there
    (rat_batch_assemble_dev).  With ``ring`` pool_ids [capacity, L] is a ring and header = [n, head]: neighbour indices are logical
    positions, a negative one counts back from n (rat_batch_assemble_ring)."""
    lib = lib or get_lib()
    _chk(data_ids, torch.int32, "data_ids"), _chk(pool_ids, torch.int32, "pool_ids")
    _chk(data_labels, name="data_labels"), _chk(pool_labels, name="pool_labels")
    _chk(retr_indices, torch.int64, "retr_indices"), _chk(rows, torch.int64, "rows"), _chk(header, torch.int64, "header")
    Q, L = data_ids.shape
    N, K, B = pool_ids.shape[0], retr_indices.shape[1], rows.numel()
    dev = data_ids.device
    idx = torch.empty((B, K + 1, L), dtype=torch.int32, device=dev)
    label_ids = torch.empty((B, K + 1), dtype=torch.int32, device=dev)
    y_true = torch.empty((B,), dtype=torch.float32, device=dev)
    head = (_p(data_ids), _p(data_labels), _p(pool_ids), _p(pool_labels), _p(retr_indices), _p(rows), _p(idx), _p(label_ids), _p(y_true), Q)
    tail = (B, K, L, _stream(data_ids))
    if ring:
        assert header is not None and header.numel() >= 2 and pool_ids.shape[1] == L and pool_labels.numel() == N
        lib.call("rat_batch_assemble_ring", *head, _p(header), N, *tail)
    elif header is not None:
        assert header.numel() >= 1
        lib.call("rat_batch_assemble_dev", *head, _p(header), *tail)
    else:
        lib.call("rat_batch_assemble", *head, N, *tail)
    return idx, label_ids, y_true


# ----------------------------------------------------------------------------- K1
_DTYPE_CODE = {torch.int32: 0, torch.int64: 1, torch.float32: 2, torch.float64: 3}       # RAT_DTYPE_* (include/rat_hip.h)


def batch_prepare(X, y, out=None, lib=None):
    """device tensors X [B,T,L] (int32 / int64 / fp32 / fp64), y [B,T] (fp32 / fp64) -> (idx int32, label ids int32, y_true fp32 [B]);
    `out`: three tensors of those shapes to write into (the static inputs of a captured step)"""
    lib = lib or get_lib()
    B, T, L = X.shape
    if X.dtype not in _DTYPE_CODE or y.dtype not in (torch.float32, torch.float64):
        raise TypeError("batch_prepare: X %s / y %s" % (X.dtype, y.dtype))
    X, y = X.contiguous(), y.contiguous()
    if out is None:
        out = (torch.empty((B, T, L), dtype=torch.int32, device=X.device), torch.empty((B, T), dtype=torch.int32, device=X.device),
               torch.empty((B,), dtype=torch.float32, device=X.device))
    idx, labels, y_true = out
    _chk(idx, torch.int32, "idx"), _chk(labels, torch.int32, "label_ids"), _chk(y_true, name="y_true")
    assert tuple(idx.shape) == (B, T, L) and tuple(labels.shape) == (B, T) and y_true.numel() == B
    lib.call("rat_batch_prepare", _p(X), _DTYPE_CODE[X.dtype], _p(y), _DTYPE_CODE[y.dtype], _p(idx), _p(labels), _p(y_true), B, T, L,
             _stream(X))
    return idx, labels, y_true


def pool_modes(fields, device):
    """int32 [F] per-field pooling modes (0 = sum / categorical, 1 = MaskedAveragePooling), or None when no field averages —
    the sum-only entry points then run unchanged"""
    modes = [1 if getattr(f, "pooling", "sum") == "average" else 0 for f in fields]
    if not any(modes):
        return None
    return torch.tensor(modes, dtype=torch.int32, device=device)


def gather_fwd(idx, label_ids, ftab, nfields, label_table, B, T, L, d, modes=None, lib=None):
    """modes: pool_modes(...) (None: every field sums)"""
    lib = lib or get_lib()
    _chk(idx, torch.int32, "idx"), _chk(label_ids, torch.int32, "label_ids"), _chk(label_table, name="label_table")
    grid = torch.empty((B, T, nfields + 1, d), dtype=torch.float32, device=idx.device)
    if modes is not None:
        _chk(modes, torch.int32, "modes")
        lib.call("rat_gather_fwd_pool", _p(idx), _p(label_ids), _p(ftab), _p(modes), nfields, _p(label_table), _p(grid), B, T, L, d,
                 _stream(idx))
        return grid
    lib.call("rat_gather_fwd", _p(idx), _p(label_ids), _p(ftab), nfields, _p(label_table), _p(grid), B, T, L, d, _stream(idx))
    return grid


def pool_scale_bwd(dgrid, dflat, idx, ftab, avg_fields, nfields, B, T, L, d, lib=None):
    """divides, in place, the averaged fields' rows of dgrid (and their target rows of dflat) by the forward's denominators;
    avg_fields: int32 [navg] device tensor of averaged field indices"""
    lib = lib or get_lib()
    _chk(dgrid, name="dgrid"), _chk(dflat, name="dflat"), _chk(idx, torch.int32, "idx"), _chk(avg_fields, torch.int32, "avg_fields")
    lib.call("rat_pool_scale_bwd", _p(dgrid), _p(dflat), _p(idx), _p(ftab), _p(avg_fields), avg_fields.numel(), nfields, B, T, L, d,
             _stream(dgrid))


def check_ids(idx, label_ids, ftab, nfields, counts, B, T, L, lib=None):
    """counts (device int32[2]) += [feature ids outside their table, label ids outside {0,1,2}] — see rat_check_ids."""
    lib = lib or get_lib()
    _chk(idx, torch.int32, "idx"), _chk(label_ids, torch.int32, "label_ids"), _chk(counts, torch.int32, "counts")
    lib.call("rat_check_ids", _p(idx), _p(label_ids), _p(ftab), nfields, B, T, L, _p(counts), _stream(idx))


def gather_bwd(dgrid, dflat, idx, label_ids, gftab, nfields, dlabel_table, B, T, L, d, lib=None):
    lib = lib or get_lib()
    _chk(dgrid, name="dgrid"), _chk(dflat, name="dflat"), _chk(dlabel_table, name="dlabel_table")
    lib.call("rat_gather_bwd", _p(dgrid), _p(dflat), _p(idx), _p(label_ids), _p(gftab), nfields, _p(dlabel_table),
             B, T, L, d, _stream(dgrid))


# ----------------------------------------------------------------------------- K1s (row-sparse / deterministic table gradients)
def col2field_table(fields, L, device):
    """int32 [L]: the field that owns each id column of idx (-1: no field reads it)"""
    arr = np.full(L, -1, dtype=np.int32)
    for i, f in enumerate(fields):
        arr[f.col:f.col + f.ncols] = i
    return torch.from_numpy(arr).to(device)


class SparsePlan:
    """Workspace + device-side unique-row count of one rat_sparse_plan_* call (what the matching reduce call needs)."""

    __slots__ = ("ws", "count", "n")

    def __init__(self, n, device, lib):
        self.n = int(n)
        self.ws = torch.empty(lib.size("rat_sparse_workspace", self.n), dtype=torch.uint8, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)


def sparse_plan_ids(idx, ftab, col2field, nfields, flat_base, width, total_rows, B, T, L, target_only=False, plan=None, lib=None):
    """flat_base: the tensor whose first element is row 0 of the table block the RatField pointers of `ftab` point into."""
    lib = lib or get_lib()
    _chk(idx, torch.int32, "idx"), _chk(col2field, torch.int32, "col2field")
    n = (B if target_only else B * T) * L
    if plan is None or plan.n != n:
        plan = SparsePlan(n, idx.device, lib)
    lib.call("rat_sparse_plan_ids", _p(idx), _p(ftab), _p(col2field), nfields, _p(flat_base), int(width), int(total_rows), B, T, L,
             int(bool(target_only)), _p(plan.ws), plan.ws.numel(), _p(plan.count), _stream(idx))
    return plan


def sparse_plan_rows(rows, counts, cap, world, total_rows, plan=None, count_out=None, lib=None):
    """count_out: where the number of unique rows is written (default: the plan's own counter) — pass the same tensor to the reduce"""
    lib = lib or get_lib()
    _chk(rows, torch.int32, "rows"), _chk(counts, torch.int32, "counts")
    n = cap * world
    if plan is None or plan.n != n:
        plan = SparsePlan(n, rows.device, lib)
    lib.call("rat_sparse_plan_rows", _p(rows), _p(counts), int(cap), int(world), int(total_rows), _p(plan.ws), plan.ws.numel(),
             _p(plan.count if count_out is None else count_out), _stream(rows))
    return plan


def sparse_reduce_grid(plan, dgrid, dflat, col2field, B, T, L, nfields, d, out_rows=None, out_grads=None, dense_base=None,
                       target_only=False, lib=None):
    lib = lib or get_lib()
    _chk(dgrid, name="dgrid"), _chk(dflat, name="dflat"), _chk(out_grads, name="out_grads"), _chk(out_rows, torch.int32, "out_rows")
    lib.call("rat_sparse_reduce_grid", _p(plan.ws), _p(plan.count), _p(dgrid), _p(dflat), _p(col2field), B, T, L, nfields, d,
             int(bool(target_only)), _p(out_rows), _p(out_grads), _p(dense_base), _stream(dgrid))


def sparse_reduce_rows(plan, src_rows, cap, world, d, out_rows, out_grads, count=None, lib=None):
    lib = lib or get_lib()
    _chk(src_rows, name="src_rows"), _chk(out_grads, name="out_grads"), _chk(out_rows, torch.int32, "out_rows")
    lib.call("rat_sparse_reduce_rows", _p(plan.ws), _p(plan.count if count is None else count), _p(src_rows), int(cap), int(world), d,
             _p(out_rows), _p(out_grads), _stream(src_rows))


def sparse_reduce_scalar(plan, per_sample, B, L, out_rows=None, out_vals=None, dense_base=None, lr_den=None, col2field=None, lib=None):
    """lr_den: [B][F] denominators of logit_fwd(..., lr_den=...) (averaged LR fields) with the col2field table they are indexed by"""
    lib = lib or get_lib()
    _chk(per_sample, name="per_sample"), _chk(out_vals, name="out_vals"), _chk(out_rows, torch.int32, "out_rows")
    if lr_den is not None:
        _chk(lr_den, name="lr_den"), _chk(col2field, torch.int32, "col2field")
        lib.call("rat_sparse_reduce_scalar_pool", _p(plan.ws), _p(plan.count), _p(per_sample), _p(lr_den), _p(col2field), lr_den.shape[1],
                 B, L, _p(out_rows), _p(out_vals), _p(dense_base), _stream(per_sample))
        return
    lib.call("rat_sparse_reduce_scalar", _p(plan.ws), _p(plan.count), _p(per_sample), B, L, _p(out_rows), _p(out_vals), _p(dense_base),
             _stream(per_sample))


def sumsq_rows(grads, count, max_rows, d, out, lib=None):
    lib = lib or get_lib()
    lib.call("rat_sumsq_rows", _p(grads), _p(count), int(max_rows), d, _p(out), _stream(grads))


def adam_rows(w_base, m_base, v_base, rows, grads, count, max_rows, d, norm_sq, max_norm, lr, beta1, beta2, eps, step, lib=None):
    lib = lib or get_lib()
    lib.call("rat_adam_rows", _p(w_base), _p(m_base), _p(v_base), _p(rows), _p(grads), _p(count), int(max_rows), d, _p(norm_sq),
             float(max_norm), float(lr), float(beta1), float(beta2), float(eps), int(step), _stream(grads))


def label_grad(dgrid, label_ids, dlabel, nbt, S, d, lib=None):
    """deterministic gradient of the 3-row label table: per-block partial sums + fixed-order combine (no atomics)"""
    lib = lib or get_lib()
    ws = torch.empty(lib.size("rat_label_grad_workspace", d) // 4, dtype=torch.float32, device=dgrid.device)
    lib.call("rat_label_grad", _p(dgrid), _p(label_ids), _p(dlabel), _p(ws), int(nbt), S, d, _stream(dgrid))


# ----------------------------------------------------------------------------- K2
ARITH = {"f32": 0, "bf16x3": 1}       # RAT_ARITH_* of include/rat_hip.h


def attn_fwd(x, params, seqmap, d, heads, dim_head, save=False, eps=1e-5, out=None, arith="f32", dropout=(0.0, 0), lib=None):
    """PreNorm(Attention)(x) + x.  arith "f32": rat_attn_fwd (exact fp32 MFMA); "bf16x3": the split-operand bf16 MFMA kernels.
    dropout = (p, seed) of the Dropout behind the output projection (training only)."""
    if arith != "f32" or dropout[0] > 0:
        return attn_fwd_ex(x, x, params, seqmap, d, heads, dim_head, save=save, eps=eps, out=out, arith=arith, dropout=dropout, lib=lib)
    lib = lib or get_lib()
    _chk(x, name="x")
    y = out if out is not None else torch.empty_like(x)
    ntok = x.numel() // d
    o_save = lse = None
    if save:
        o_save = torch.empty((ntok, heads * dim_head), dtype=torch.float32, device=x.device)
        lse = torch.empty((ntok, heads), dtype=torch.float32, device=x.device)
    lib.call("rat_attn_fwd", _p(x), _p(y), _p(o_save), _p(lse), ctypes.byref(params), ctypes.byref(seqmap), d, heads,
             dim_head, eps, _stream(x))
    return y, o_save, lse


def attn_bwd(x, dy, o_save, lse, params, grads, seqmap, d, heads, dim_head, eps=1e-5, workspace=None, arith="f32", dropout=(0.0, 0),
             out=None, lib=None):
    """out: where dx goes (default: a new tensor); `out is dy` is allowed — a work-group reads the dy rows of its sequences before it
    writes their dx rows, and rows outside the map's sequences are left as they are."""
    if arith != "f32" or dropout[0] > 0:
        return attn_bwd_ex(x, dy, dy, o_save, lse, params, grads, seqmap, d, heads, dim_head, eps=eps, workspace=workspace,
                           out=out, arith=arith, dropout=dropout, lib=lib)
    lib = lib or get_lib()
    _chk(x, name="x"), _chk(dy, name="dy")
    need = lib.size("rat_attn_bwd_workspace", d, heads, dim_head)
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    dx = out if out is not None else torch.empty_like(x)
    lib.call("rat_attn_bwd", _p(x), _p(dy), _p(o_save), _p(lse), _p(dx), ctypes.byref(params), ctypes.byref(grads),
             _p(workspace), workspace.numel() * 4, ctypes.byref(seqmap), d, heads, dim_head, eps, _stream(x))
    return dx, workspace


_FWD_WS = {}


def _attn_fwd_workspace(lib, d, heads, dim_head, device):
    """per (library, shape, device, stream) scratch for the pre-split weight fragments of the bf16x3 forward: launches on one
    stream are ordered, so consecutive layers may share it"""
    need = lib.size("rat_attn_fwd_workspace", d, heads, dim_head)
    if not need:
        return None
    key = (id(lib), d, heads, dim_head, str(device), torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    ws = _FWD_WS.get(key)
    if ws is None:
        ws = _FWD_WS[key] = torch.empty((need + 3) // 4, dtype=torch.float32, device=device)
    return ws


def attn_fwd_ex(x, res, params, seqmap, d, heads, dim_head, softmax_scale=0.0, out_scale=1.0, save=False, eps=1e-5, out=None,
                arith="f32", dropout=(0.0, 0), lib=None):
    """y = out_scale * attention(LayerNorm(x)) + res (res: a tensor laid out like x, the output itself, or None)."""
    lib = lib or get_lib()
    _chk(x, name="x")
    y = out if out is not None else torch.empty_like(x)
    ntok = x.numel() // d
    o_save = lse = None
    if save:
        o_save = torch.empty((ntok, heads * dim_head), dtype=torch.float32, device=x.device)
        lse = torch.empty((ntok, heads), dtype=torch.float32, device=x.device)
    ws = _attn_fwd_workspace(lib, d, heads, dim_head, x.device) if arith != "f32" else None
    drop_p, drop_seed = _drop_args(params, dropout)
    lib.call("rat_attn_fwd_ex", _p(x), _p(res), _p(y), _p(o_save), _p(lse), ctypes.byref(params), ctypes.byref(seqmap), d, heads,
             dim_head, float(softmax_scale), float(out_scale), eps, drop_p, drop_seed, ARITH[arith],
             _p(ws), ws.numel() * 4 if ws is not None else 0, _stream(x))
    return y, o_save, lse


def attn_groups_supported(d, heads, dim_head, lib=None):
    """bit 0: attn_fwd_groups serves these dimensions (d = 64 on bf16x3 planes, or d <= 16 in place); bit 1: attn_bwd_groups does too"""
    return int((lib or get_lib()).size("rat_attn_groups_supported", int(d), int(heads), int(dim_head)))


def attn_bwd_groups(x, dy, add, o_save, lse, params, grads, seqmap, d, heads, dim_head, softmax_scale=0.0, out_scale=1.0, eps=1e-5,
                    workspace=None, out=None, dropout=(0.0, 0), lib=None):
    """Backward of attn_fwd_groups in ONE launch (small embedding dimensions): dx = add + LayerNorm-backward(...); `grads` receives the
    gradients in the layer's full-width layout."""
    lib = lib or get_lib()
    _chk(x, name="x"), _chk(dy, name="dy"), _chk(o_save, name="o_save"), _chk(lse, name="lse")
    need = lib.size("rat_attn_bwd_groups_workspace", d, heads, dim_head)
    if need == 0:
        raise ValueError("attn_bwd_groups does not serve d=%d heads=%d dim_head=%d" % (d, heads, dim_head))
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    dx = out if out is not None else torch.empty_like(x)
    drop_p, drop_seed = _drop_args(params, dropout)
    lib.call("rat_attn_bwd_groups", _p(x), _p(dy), _p(add), _p(o_save), _p(lse), x.numel() // d, _p(dx), ctypes.byref(params),
             ctypes.byref(grads), _p(workspace), workspace.numel() * 4, ctypes.byref(seqmap), d, heads, dim_head, float(softmax_scale),
             float(out_scale), eps, drop_p, drop_seed, _stream(x))
    return dx, workspace


def attn_fwd_groups(x, res, params, planes, seqmap, d, heads, dim_head, softmax_scale=0.0, out_scale=1.0, save=False, eps=1e-5, out=None,
                    dropout=(0.0, 0), lib=None):
    """Wide heads (heads = G x 8 of width 10; at small embedding dimensions also G x 4 of width 20) in ONE launch: y = out_scale *
    Dropout(to_out(attention(LayerNorm(x)))) + res, the head groups looped over inside each chunk.  -> (y, o_save [G, ntok, 80],
    lse [G, ntok, heads per group]); slice g is what attn_bwd_ex takes for group g."""
    lib = lib or get_lib()
    _chk(x, name="x"), _chk(planes, torch.uint8, "planes")                    # planes: None at small embedding dimensions
    y = out if out is not None else torch.empty_like(x)
    per = 80 // dim_head                                     # heads per group: 8 x 10, or 4 x 20 (RAT_m3's halved head count; small d only)
    ntok, G = x.numel() // d, heads // per
    o_save = lse = None
    if save:
        o_save = torch.empty((G, ntok, 80), dtype=torch.float32, device=x.device)
        lse = torch.empty((G, ntok, per), dtype=torch.float32, device=x.device)
    drop_p, drop_seed = _drop_args(params, dropout)
    lib.call("rat_attn_fwd_groups", _p(x), _p(res), _p(y), _p(o_save), _p(lse), ntok, ctypes.byref(params), _p(planes),
             ctypes.byref(seqmap), d, heads, dim_head, float(softmax_scale), float(out_scale), eps, drop_p, drop_seed, _stream(x))
    return y, o_save, lse


def attn_bwd_ex(x, dy, add, o_save, lse, params, grads, seqmap, d, heads, dim_head, softmax_scale=0.0, out_scale=1.0, eps=1e-5,
                workspace=None, out=None, arith="f32", dropout=(0.0, 0), lib=None):
    """dx = add + LayerNorm-backward(... out_scale * dy ...) (add: tensor laid out like x, or None)."""
    lib = lib or get_lib()
    _chk(x, name="x"), _chk(dy, name="dy")
    need = lib.size("rat_attn_bwd_workspace", d, heads, dim_head)
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    dx = out if out is not None else torch.empty_like(x)
    drop_p, drop_seed = _drop_args(params, dropout)
    lib.call("rat_attn_bwd_ex", _p(x), _p(dy), _p(add), _p(o_save), _p(lse), _p(dx), ctypes.byref(params), ctypes.byref(grads),
             _p(workspace), workspace.numel() * 4, ctypes.byref(seqmap), d, heads, dim_head, float(softmax_scale),
             float(out_scale), eps, drop_p, drop_seed, ARITH[arith], _stream(x))
    return dx, workspace


def attn_fused_supported(d, heads, dim_head, L, lib=None):
    """True when rat_attn_fwd / rat_attn_bwd serve these dimensions (else: the composed path, see model._attn_composed_*)."""
    lib = lib or get_lib()
    return bool(lib.size("rat_attn_fused_supported", int(d), int(heads), int(dim_head), int(L)))


def attn_core_fwd_map(qkv, seqmap, heads, dim_head, softmax_scale=0.0, save=True, lib=None):
    """attn_core_fwd with RatSeqMap addressing (strided sequences); qkv is [ntok, 3*heads*dim_head] over the WHOLE token grid."""
    lib = lib or get_lib()
    _chk(qkv, name="qkv")
    ntok = qkv.shape[0]
    o = torch.empty((ntok, heads * dim_head), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((ntok, heads), dtype=torch.float32, device=qkv.device) if save else None
    lib.call("rat_attn_core_fwd_map", _p(qkv), _p(o), _p(lse), ctypes.byref(seqmap), heads, dim_head, float(softmax_scale), _stream(qkv))
    return o, lse


def attn_core_bwd_map(qkv, o, lse, dout, seqmap, heads, dim_head, softmax_scale=0.0, lib=None):
    lib = lib or get_lib()
    _chk(qkv, name="qkv"), _chk(o, name="o"), _chk(lse, name="lse"), _chk(dout, name="dout")
    dqkv = torch.empty_like(qkv)
    lib.call("rat_attn_core_bwd_map", _p(qkv), _p(o), _p(lse), _p(dout), _p(dqkv), ctypes.byref(seqmap), heads, dim_head,
             float(softmax_scale), _stream(qkv))
    return dqkv


def attn_core_fwd(qkv, nseq, L, heads, dim_head, softmax_scale=0.0, save=True, lib=None):
    """softmax(Q K^T * scale) V on projected rows qkv [nseq*L, 3*heads*dim_head] -> (o [ntok, heads*dim_head], lse [ntok, heads])."""
    lib = lib or get_lib()
    _chk(qkv, name="qkv")
    ntok = nseq * L
    o = torch.empty((ntok, heads * dim_head), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((ntok, heads), dtype=torch.float32, device=qkv.device) if save else None
    lib.call("rat_attn_core_fwd", _p(qkv), _p(o), _p(lse), int(nseq), int(L), heads, dim_head, float(softmax_scale), _stream(qkv))
    return o, lse


def attn_core_bwd(qkv, o, lse, dout, nseq, L, heads, dim_head, softmax_scale=0.0, lib=None):
    lib = lib or get_lib()
    _chk(qkv, name="qkv"), _chk(o, name="o"), _chk(lse, name="lse"), _chk(dout, name="dout")
    dqkv = torch.empty_like(qkv)
    lib.call("rat_attn_core_bwd", _p(qkv), _p(o), _p(lse), _p(dout), _p(dqkv), int(nseq), int(L), heads, dim_head,
             float(softmax_scale), _stream(qkv))
    return dqkv


def ffn_fwd(x, w1, b1, w2, b2, d, hidden, out=None, arith="f32", lib=None):
    if arith != "f32":
        return ffn_fwd_res(x, x, w1, b1, w2, b2, d, hidden, out=out, arith=arith, lib=lib)
    lib = lib or get_lib()
    _chk(x, name="x")
    y = out if out is not None else torch.empty_like(x)
    lib.call("rat_ffn_fwd", _p(x), _p(y), _p(w1), _p(b1), _p(w2), _p(b2), x.numel() // d, d, hidden, _stream(x))
    return y


def ffn_bwd(x, dy, w1, b1, w2, b2, dw1, db1, dw2, db2, d, hidden, workspace=None, arith="f32", planes=None, lib=None):
    if arith != "f32":
        return ffn_bwd_res(x, dy, w1, b1, w2, b2, dw1, db1, dw2, db2, d, hidden, True, workspace=workspace, arith=arith, planes=planes,
                           lib=lib)
    lib = lib or get_lib()
    _chk(x, name="x"), _chk(dy, name="dy")
    need = lib.size("rat_ffn_bwd_workspace", d, hidden)
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    lib.call("rat_ffn_bwd", _p(x), _p(dy), _p(dx), _p(w1), _p(b1), _p(w2), _p(b2), _p(dw1), _p(db1), _p(dw2), _p(db2),
             _p(workspace), workspace.numel() * 4, x.numel() // d, d, hidden, _stream(x))
    return dx, workspace


def ffn_fwd_res(x, res, w1, b1, w2, b2, d, hidden, out=None, arith="f32", dropout=None, lib=None):
    """y = FFN(x) + res (res None: no residual) — rat_ffn_fwd_res.  dropout = (p, word1, word2): FeedForward's two Dropout layers in
    training mode (rat_ffn_fwd_drop; exact fp32, generic kernels)."""
    lib = lib or get_lib()
    _chk(x, name="x")
    if res is not None:
        _chk(res, name="res")
    y = out if out is not None else torch.empty_like(x)
    if dropout is not None and dropout[0] > 0:
        _chk(dropout[1], torch.int64, "seed word"), _chk(dropout[2], torch.int64, "seed word")
        lib.call("rat_ffn_fwd_drop", _p(x), _p(res), _p(y), _p(w1), _p(b1), _p(w2), _p(b2), x.numel() // d, d, hidden, float(dropout[0]),
                 _p(dropout[1]), _p(dropout[2]), _stream(x))
        return y
    lib.call("rat_ffn_fwd_res", _p(x), _p(res), _p(y), _p(w1), _p(b1), _p(w2), _p(b2), x.numel() // d, d, hidden, ARITH[arith],
             _stream(x))
    return y


def ffn_bwd_res(x, dy, w1, b1, w2, b2, dw1, db1, dw2, db2, d, hidden, add_dy, workspace=None, arith="f32", planes=None, dropout=None,
                lib=None):
    lib = lib or get_lib()
    _chk(x, name="x"), _chk(dy, name="dy")
    need = lib.size("rat_ffn_bwd_workspace", d, hidden)
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    if dropout is not None and dropout[0] > 0:
        lib.call("rat_ffn_bwd_drop", _p(x), _p(dy), _p(dx), _p(w1), _p(b1), _p(w2), _p(b2), _p(dw1), _p(db1), _p(dw2), _p(db2),
                 _p(workspace), workspace.numel() * 4, x.numel() // d, d, hidden, int(bool(add_dy)), float(dropout[0]), _p(dropout[1]),
                 _p(dropout[2]), _stream(x))
        return dx, workspace
    lib.call("rat_ffn_bwd_res", _p(x), _p(dy), _p(dx), _p(w1), _p(b1), _p(w2), _p(b2), _p(dw1), _p(db1), _p(dw2), _p(db2),
             _p(workspace), workspace.numel() * 4, _p(planes), x.numel() // d, d, hidden, int(bool(add_dy)), ARITH[arith], _stream(x))
    return dx, workspace


def ffn_bwd_rows_supported(d, hidden, arith, lib=None):
    return bool((lib or get_lib()).cdll.rat_ffn_bwd_rows_supported(int(d), int(hidden), ARITH[arith]))


def ffn_bwd_rows(x, dy_rows, period, w1, b1, w2, b2, dw1, db1, dw2, db2, d, hidden, workspace=None, arith="bf16x3", planes=None, lib=None):
    """ffn_bwd (residual from x itself) where dy is zero except on the token rows k * period, held compactly in dy_rows [*, d]"""
    lib = lib or get_lib()
    _chk(x, name="x"), _chk(dy_rows, name="dy_rows")
    ntok = x.numel() // d
    assert dy_rows.numel() == (ntok + period - 1) // period * d, (tuple(dy_rows.shape), ntok, period)
    need = lib.size("rat_ffn_bwd_workspace", d, hidden)
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    lib.call("rat_ffn_bwd_res_rows", _p(x), _p(dy_rows), int(period), _p(dx), _p(w1), _p(b1), _p(w2), _p(b2), _p(dw1), _p(db1), _p(dw2),
             _p(db2), _p(workspace), workspace.numel() * 4, _p(planes), ntok, d, hidden, 1, ARITH[arith], _stream(x))
    return dx, workspace


class deferred_reductions:
    """with deferred_reductions(tensor_on_the_stream, lib): ... — the gradient-slab reductions of the attention / feed-forward backward
    calls inside run as ONE launch at the end (rat_reduce_defer_begin / _end).  Every call inside needs a workspace of its own."""

    def __init__(self, like, lib=None, enabled=True):
        self.lib, self.like, self.enabled = lib or get_lib(), like, enabled

    def __enter__(self):
        if self.enabled:
            self.lib.call("rat_reduce_defer_begin")
        return self

    def __exit__(self, exc_type, exc, tb):
        if self.enabled:
            self.lib.call("rat_reduce_defer_end", _stream(self.like), 0 if exc_type is not None else 1)
        return False


# ----------------------------------------------------------------------------- K2c
def layernorm_fwd(x, x_stride, nrows, gamma, beta, d, eps=1e-5, lib=None):
    """LayerNorm of rows x[r * x_stride : r * x_stride + d] -> compact [nrows, d]."""
    lib = lib or get_lib()
    _chk(x, name="x")
    y = torch.empty((nrows, d), dtype=torch.float32, device=x.device)
    lib.call("rat_layernorm_fwd", _p(x), int(x_stride), _p(y), _p(gamma), _p(beta), int(nrows), d, float(eps), _stream(x))
    return y


def layernorm_bwd(x, x_stride, dy, gamma, dx, dx_stride, dgamma, dbeta, d, add=None, eps=1e-5, lib=None):
    """dx rows (stride dx_stride) = [add +] LN-backward(dy); dgamma / dbeta overwritten."""
    lib = lib or get_lib()
    _chk(x, name="x"), _chk(dy, name="dy"), _chk(dx, name="dx")
    nrows = dy.numel() // d
    need = lib.size("rat_layernorm_bwd_workspace", nrows, d)
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    lib.call("rat_layernorm_bwd", _p(x), int(x_stride), _p(dy), _p(gamma), _p(add), _p(dx), int(dx_stride), _p(dgamma),
             _p(dbeta), _p(ws), ws.numel() * 4, int(nrows), d, float(eps), _stream(x))
    return dx


# ----------------------------------------------------------------------------- K3
def sgemm(ta, tb, M, N, K, A, lda, Bm, ldb, C, ldc, bias=None, beta=0.0, arith="f32", lib=None):
    lib = lib or get_lib()
    need = lib.size("rat_sgemm_workspace", M, N, K)
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=C.device) if need else None   # long-K / few-tile products: split-K
    lib.call("rat_sgemm_arith", int(ta), int(tb), M, N, K, _p(A), lda, _p(Bm), ldb, _p(C), ldc, _p(bias), float(beta),
             _p(ws), ws.numel() * 4 if ws is not None else 0, 1 if arith == "bf16x3" else 0, _stream(C))


def _bn_ws(N, device, lib):
    return torch.empty((lib.size("rat_bn_workspace", N) + 3) // 4, dtype=torch.float32, device=device)


ACT = {"relu": 0, "none": 1, "identity": 1, "sigmoid": 2, "tanh": 3, "leakyrelu": 4, "elu": 5}     # RAT_ACT_* (include/rat_hip.h)


def bn_relu_fwd(z, gamma, beta, running_mean, running_var, training, use_bn, eps=1e-5, momentum=0.1, act=0, lib=None):
    """[BatchNorm1d] + activation (act: a RAT_ACT_* code, 0 = ReLU)"""
    lib = lib or get_lib()
    _chk(z, name="z")
    M, N = z.shape
    a = torch.empty_like(z)
    save_mean = save_rstd = ws = None
    if use_bn and training:
        save_mean = torch.empty(N, dtype=torch.float32, device=z.device)
        save_rstd = torch.empty(N, dtype=torch.float32, device=z.device)
        ws = _bn_ws(N, z.device, lib)
    lib.call("rat_bn_relu_fwd", _p(z), _p(a), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(save_mean),
             _p(save_rstd), _p(ws), M, N, int(training), int(use_bn), eps, momentum, int(act), _stream(z))
    return a, save_mean, save_rstd


def bn_strip_ok(M, N, lib=None):
    return bool((lib or get_lib()).cdll.rat_bn_strip_ok(int(M), int(N)))


def bn_act_fwd_strip(z, gamma, beta, running_mean, running_var, training, use_bn, eps=1e-5, momentum=0.1, act=0, lib=None):
    """bn_relu_fwd in one launch (column strips; N % 4 == 0)"""
    lib = lib or get_lib()
    _chk(z, name="z")
    M, N = z.shape
    a = torch.empty_like(z)
    save_mean = save_rstd = None
    if use_bn and training:
        save = torch.empty((2, (N + 3) // 4 * 4), dtype=torch.float32, device=z.device)
        save_mean, save_rstd = save[0, :N], save[1, :N]
    lib.call("rat_bn_act_fwd_strip", _p(z), _p(a), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(save_mean),
             _p(save_rstd), M, N, int(training), int(use_bn), eps, momentum, int(act), _stream(z))
    return a, save_mean, save_rstd


def bn_act_bwd_strip(z, a, da, gamma, save_mean, save_rstd, dgamma, dbeta, dbias_lin, use_bn, act=0, lib=None):
    """bn_relu_bwd + colsum(dz) -> dbias_lin in one launch"""
    lib = lib or get_lib()
    M, N = z.shape
    dz = torch.empty_like(z)
    lib.call("rat_bn_act_bwd_strip", _p(z), _p(a), _p(da), _p(dz), _p(gamma), _p(save_mean), _p(save_rstd), _p(dgamma), _p(dbeta),
             _p(dbias_lin), M, N, int(use_bn), int(act), _stream(z))
    return dz


def bn_act_bwd_strip_outer(z, a, dl, w, dw, gamma, save_mean, save_rstd, dgamma, dbeta, dbias_lin, use_bn, act=0, lib=None):
    """bn_act_bwd_strip of the last hidden layer with da = dl (x) w formed in the kernel; dw <- sum_r dl[r] a[r][:]"""
    lib = lib or get_lib()
    M, N = z.shape
    dz = torch.empty_like(z)
    lib.call("rat_bn_act_bwd_strip_outer", _p(z), _p(a), _p(dl), _p(w), _p(dw), _p(dz), _p(gamma), _p(save_mean), _p(save_rstd),
             _p(dgamma), _p(dbeta), _p(dbias_lin), M, N, int(use_bn), int(act), _stream(z))
    return dz


def bn_relu_bwd(z, a, da, gamma, save_mean, save_rstd, dgamma, dbeta, use_bn, act=0, lib=None):
    lib = lib or get_lib()
    M, N = z.shape
    dz = torch.empty_like(z)
    ws = _bn_ws(N, z.device, lib) if use_bn else None
    lib.call("rat_bn_relu_bwd", _p(z), _p(a), _p(da), _p(dz), _p(gamma), _p(save_mean), _p(save_rstd), _p(dgamma), _p(dbeta),
             _p(ws), M, N, int(use_bn), int(act), _stream(z))
    return dz


def bn_relu_fwd_sync(z, gamma, beta, running_mean, running_var, all_gather, eps=1e-5, momentum=0.1, act=0, lib=None):
    """SyncBN training forward: local (mean, M2, count) -> `all_gather(stats) -> [world, 2N+1]` (the caller's
    collective: torch.distributed over RCCL / gloo) -> normalise with the GLOBAL batch statistics + ReLU."""
    lib = lib or get_lib()
    _chk(z, name="z")
    M, N = z.shape
    stats = torch.empty(2 * N + 1, dtype=torch.float32, device=z.device)
    ws = _bn_ws(N, z.device, lib)
    lib.call("rat_bn_local_stats", _p(z), _p(stats), _p(ws), M, N, _stream(z))
    all_stats = all_gather(stats)
    _chk(all_stats, name="all_stats")
    world = all_stats.numel() // (2 * N + 1)
    a = torch.empty_like(z)
    save_mean = torch.empty(N, dtype=torch.float32, device=z.device)
    save_rstd = torch.empty(N, dtype=torch.float32, device=z.device)
    lib.call("rat_bn_relu_fwd_sync", _p(z), _p(a), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(save_mean),
             _p(save_rstd), _p(all_stats), world, M, N, eps, momentum, int(act), _stream(z))
    return a, save_mean, save_rstd, all_stats


def bn_relu_bwd_sync(z, a, da, gamma, save_mean, save_rstd, dgamma, dbeta, all_reduce_sum, all_stats, act=0, lib=None):
    """SyncBN backward: local (sum g, sum g*xhat) -> `all_reduce_sum(copy)` (caller's collective) -> dz; dgamma/dbeta = LOCAL sums."""
    lib = lib or get_lib()
    M, N = z.shape
    local = torch.empty(2 * N, dtype=torch.float32, device=z.device)
    ws = _bn_ws(N, z.device, lib)
    lib.call("rat_bn_bwd_local_sums", _p(z), _p(a), _p(da), _p(save_mean), _p(save_rstd), _p(local), _p(ws), M, N, int(act), _stream(z))
    glob = all_reduce_sum(local.clone())
    dz = torch.empty_like(z)
    lib.call("rat_bn_relu_bwd_sync", _p(z), _p(a), _p(da), _p(dz), _p(gamma), _p(save_mean), _p(save_rstd), _p(local), _p(glob),
             _p(dgamma), _p(dbeta), _p(all_stats), all_stats.numel() // (2 * N + 1), M, N, int(act), _stream(z))
    return dz


def colsum(a, lda, out, M, N, lib=None):
    lib = lib or get_lib()
    ws = torch.empty((lib.size("rat_colsum_workspace", M, N) + 3) // 4, dtype=torch.float32, device=out.device)
    lib.call("rat_colsum", _p(a), lda, _p(out), _p(ws), M, N, _stream(out))


def logit_fwd(cls, cls_stride, fc_w, fc_b, dnn_out, lr_ftab, nfields, idx, idx_stride, y_true, loss_sum, B, d, head=0, dnn_last=None,
              modes=None, lr_den=None, lib=None):
    """head: 0 = sigmoid + binary cross-entropy, 1 = no output activation + mean squared error (task "regression")
    dnn_last = (a [B][K], lda, K, w [1][K], b [1]): the DNN's one-output Linear is evaluated inside the launch (dnn_out must be None)
    modes: pool_modes(...) of the LR fields (None: every field sums); lr_den (with modes): float [B][nfields] <- the LR denominators"""
    lib = lib or get_lib()
    y_pred = torch.empty((B, 1), dtype=torch.float32, device=fc_w.device)
    if modes is not None and lr_ftab is not None:
        _chk(modes, torch.int32, "modes"), _chk(lr_den, name="lr_den")
        if dnn_last is not None:
            assert dnn_out is None
            a, lda, K, w, b = dnn_last
            lib.call("rat_logit_fwd_dnn_pool", _p(cls), cls_stride, _p(fc_w), _p(fc_b), _p(a), lda, _p(w), _p(b), K, _p(lr_ftab), _p(modes),
                     nfields, _p(idx), idx_stride, _p(y_true), _p(y_pred), _p(loss_sum), _p(lr_den), B, d, int(head), _stream(fc_w))
        else:
            lib.call("rat_logit_fwd_pool", _p(cls), cls_stride, _p(fc_w), _p(fc_b), _p(dnn_out), _p(lr_ftab), _p(modes), nfields, _p(idx),
                     idx_stride, _p(y_true), _p(y_pred), _p(loss_sum), _p(lr_den), B, d, int(head), _stream(fc_w))
        return y_pred
    if dnn_last is not None:
        assert dnn_out is None
        a, lda, K, w, b = dnn_last
        lib.call("rat_logit_fwd_dnn", _p(cls), cls_stride, _p(fc_w), _p(fc_b), _p(a), lda, _p(w), _p(b), K, _p(lr_ftab), nfields,
                 _p(idx), idx_stride, _p(y_true), _p(y_pred), _p(loss_sum), B, d, int(head), _stream(fc_w))
        return y_pred
    lib.call("rat_logit_fwd", _p(cls), cls_stride, _p(fc_w), _p(fc_b), _p(dnn_out), _p(lr_ftab), nfields, _p(idx),
             idx_stride, _p(y_true), _p(y_pred), _p(loss_sum), B, d, int(head), _stream(fc_w))
    return y_pred


def logit_bwd(y_pred, y_true, cls, cls_stride, fc_w, dcls, dcls_stride, dfc_w, dfc_b, lr_gftab, nfields, idx, idx_stride,
              gscale, B, d, gscale_dev=None, head=0, ddnn_b=None, lr_den=None, lib=None):
    """gscale: host factor; gscale_dev: optional DEVICE scalar multiplied in by the kernel (autograd's incoming gradient).
    ddnn_b: also accumulate sum_b dlogit[b] there (bias gradient of the DNN's one-output Linear)
    lr_den: the LR denominators logit_fwd wrote (averaged LR fields): field f of sample b scatters dlogit[b] / lr_den[b][f]"""
    lib = lib or get_lib()
    dlogit = torch.empty((B, 1), dtype=torch.float32, device=fc_w.device)
    if lr_den is not None and lr_gftab is not None:
        _chk(lr_den, name="lr_den")
        lib.call("rat_logit_bwd_pool", _p(y_pred), _p(y_true), _p(cls), cls_stride, _p(fc_w), _p(dlogit), _p(dcls), dcls_stride,
                 _p(dfc_w), _p(dfc_b), _p(ddnn_b), _p(lr_gftab), _p(lr_den), nfields, _p(idx), idx_stride, float(gscale), _p(gscale_dev),
                 B, d, int(head), _stream(fc_w))
        return dlogit
    if ddnn_b is not None:
        lib.call("rat_logit_bwd_dnn", _p(y_pred), _p(y_true), _p(cls), cls_stride, _p(fc_w), _p(dlogit), _p(dcls), dcls_stride,
                 _p(dfc_w), _p(dfc_b), _p(ddnn_b), _p(lr_gftab), nfields, _p(idx), idx_stride, float(gscale), _p(gscale_dev), B, d,
                 int(head), _stream(fc_w))
        return dlogit
    lib.call("rat_logit_bwd", _p(y_pred), _p(y_true), _p(cls), cls_stride, _p(fc_w), _p(dlogit), _p(dcls), dcls_stride,
             _p(dfc_w), _p(dfc_b), _p(lr_gftab), nfields, _p(idx), idx_stride, float(gscale), _p(gscale_dev), B, d, int(head),
             _stream(fc_w))
    return dlogit


# ----------------------------------------------------------------------------- K4 / K5
def l2_reg(w, g, lam, reg_out, lam_scale_dev=None, lib=None):
    lib = lib or get_lib()
    lib.call("rat_l2_reg", _p(w), _p(g), w.numel(), float(lam), _p(lam_scale_dev), _p(reg_out), _stream(w))


def sumsq(g, out, lib=None):
    lib = lib or get_lib()
    lib.call("rat_sumsq", _p(g), g.numel(), _p(out), _stream(g))


def clip_adam(w, g, m, v, norm_sq, max_norm, lr, beta1, beta2, eps, step, lib=None):
    lib = lib or get_lib()
    lib.call("rat_clip_adam", _p(w), _p(g), _p(m), _p(v), w.numel(), _p(norm_sq), float(max_norm), float(lr), float(beta1),
             float(beta2), float(eps), int(step), _stream(w))


def clip_opt(w, g, state, norm_sq, max_norm, lr, kind, p0, eps, lib=None):
    """SGD / Adagrad / RMSprop (kind 1 / 2 / 3) on a flat buffer, after the clip factor derived from norm_sq"""
    lib = lib or get_lib()
    lib.call("rat_clip_opt", _p(w), _p(g), _p(state), w.numel(), _p(norm_sq), float(max_norm), float(lr), int(kind), float(p0), float(eps),
             _stream(w))


def clip_opt_fused(w, g, state, n_split, lam_a, lam_b, norm_sq, max_norm, hyper, kind, p0, eps, zero_g=True, lam_scale_dev=None,
                   lib=None):
    lib = lib or get_lib()
    lib.call("rat_clip_opt_fused", _p(w), _p(g), _p(state), w.numel(), int(n_split), float(lam_a), float(lam_b), _p(lam_scale_dev),
             _p(norm_sq), float(max_norm), _p(hyper), int(kind), float(p0), float(eps), int(bool(zero_g)), _stream(w))


def dropout(x, p, seed, out=None, lib=None):
    """seed: an int (by value) or a one-element int64 DEVICE tensor — one of the words `dropout_seeds` refreshes per step"""
    lib = lib or get_lib()
    _chk(x, name="x")
    y = out if out is not None else torch.empty_like(x)
    if torch.is_tensor(seed):
        _chk(seed, torch.int64, "seed word")
        lib.call("rat_dropout_dev", _p(x), _p(y), x.numel(), float(p), _p(seed), _stream(x))
    else:
        lib.call("rat_dropout", _p(x), _p(y), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream(x))
    return y


def dropout_seeds(words, base_seed, counter, lib=None):
    """counter += 1; words[i] = mix(base_seed, counter, i): the dropout state of one training step, on the device"""
    lib = lib or get_lib()
    _chk(words, torch.int64, "seed words"), _chk(counter, torch.int64, "counter")
    lib.call("rat_dropout_seeds", _p(words), words.numel(), int(base_seed) & 0xFFFFFFFFFFFFFFFF, _p(counter), _stream(words))


def _drop_args(params, dropout):
    """(p, seed) -> the by-value arguments; a tensor seed goes into the parameter struct (RatAttnParams.drop_seed_dev, ABI v6)"""
    p, seed = dropout
    if torch.is_tensor(seed):
        _chk(seed, torch.int64, "seed word")
        params.drop_seed_dev = seed.data_ptr()
        return float(p), 0
    params.drop_seed_dev = None
    return float(p), int(seed) & 0xFFFFFFFFFFFFFFFF


# ----------------------------------------------------------------------------- ABI v4: two-sweep optimizer, device-side clock
def adam_tick(step_dev, lr_dev, beta1, beta2, hyper, lib=None):
    """*step_dev += 1; hyper[0..2] = lr/(1-beta1^t), 1/sqrt(1-beta2^t), lr"""
    lib = lib or get_lib()
    _chk(step_dev, torch.int32, "step_dev"), _chk(lr_dev, name="lr_dev"), _chk(hyper, name="hyper")
    lib.call("rat_adam_tick", _p(step_dev), _p(lr_dev), float(beta1), float(beta2), _p(hyper), _stream(hyper))


def step_begin(step_dev, lr_dev, beta1, beta2, hyper, scalars, counters=None, lib=None):
    """adam_tick + scalars[:] = 0 + counters[:] += 1 (int64) in one launch"""
    lib = lib or get_lib()
    _chk(step_dev, torch.int32, "step_dev"), _chk(lr_dev, name="lr_dev"), _chk(hyper, name="hyper"), _chk(scalars, name="scalars")
    if counters is not None:
        _chk(counters, torch.int64, "counters")
    lib.call("rat_step_begin", _p(step_dev), _p(lr_dev), float(beta1), float(beta2), _p(hyper), _p(scalars), scalars.numel(),
             _p(counters), counters.numel() if counters is not None else 0, _stream(hyper))


def sumsq_reg(g, w, n_split, lam_a, lam_b, norm_sq_out, reg_out=None, lam_scale_dev=None, lib=None):
    lib = lib or get_lib()
    assert g.numel() == w.numel()
    lib.call("rat_sumsq_reg", _p(g), _p(w), g.numel(), int(n_split), float(lam_a), float(lam_b), _p(lam_scale_dev), _p(norm_sq_out),
             _p(reg_out), _stream(g))


def clip_adam_fused(w, g, m, v, n_split, lam_a, lam_b, norm_sq, max_norm, hyper, beta1, beta2, eps, zero_g=True, lam_scale_dev=None,
                    lib=None):
    lib = lib or get_lib()
    lib.call("rat_clip_adam_fused", _p(w), _p(g), _p(m), _p(v), w.numel(), int(n_split), float(lam_a), float(lam_b), _p(lam_scale_dev),
             _p(norm_sq), float(max_norm), _p(hyper), float(beta1), float(beta2), float(eps), 1 if zero_g else 0, _stream(w))


def adam_rows_dev(w_base, m_base, v_base, rows, grads, count, max_rows, d, norm_sq, max_norm, hyper, beta1, beta2, eps, lib=None):
    lib = lib or get_lib()
    lib.call("rat_adam_rows_dev", _p(w_base), _p(m_base), _p(v_base), _p(rows), _p(grads), _p(count), int(max_rows), d, _p(norm_sq),
             float(max_norm), _p(hyper), float(beta1), float(beta2), float(eps), _stream(grads))


def scatter_rows_lists(dense_base, rows, grads, counts, d, lib=None):
    """rows [lists, cap] int32, grads [lists, cap, d], counts [lists] int32 -> the zeroed dense gradient block"""
    lib = lib or get_lib()
    _chk(rows, torch.int32, "rows"), _chk(counts, torch.int32, "counts"), _chk(grads, name="grads")
    lib.call("rat_scatter_rows_lists", _p(dense_base), _p(rows), _p(grads), _p(counts), rows.shape[1], rows.shape[0], int(d), _stream(grads))


def scatter_rows(dense_base, rows, grads, count, d, lib=None):
    """merged (unique rows, gradient rows) lists -> the zeroed dense gradient block"""
    lib = lib or get_lib()
    _chk(rows, torch.int32, "rows"), _chk(count, torch.int32, "count")
    lib.call("rat_scatter_rows", _p(dense_base), _p(rows), _p(grads), _p(count), rows.numel(), int(d), _stream(grads))


# ---- owner-partitioned exchange of the row lists (data parallelism; include/rat_hip.h ABI v8) -----------------------------------------
def owner_counts(plan, rows_per_owner, world, out, lib=None):
    """out[k] (int32 [world]) = unique rows of `plan` in owner k's range [k per, (k + 1) per)"""
    lib = lib or get_lib()
    _chk(out, torch.int32, "out")
    assert out.numel() == world
    lib.call("rat_owner_counts", _p(plan.ws), _p(plan.count), int(plan.n), int(rows_per_owner), int(world), _p(out), _stream(out))


def owner_pack(mat, world, rank, d, rows_a, grads_a, rows_b, vals_b, max_pairs, wire, lib=None):
    lib = lib or get_lib()
    _chk(mat, torch.int32, "mat"), _chk(rows_a, torch.int32, "rows_a"), _chk(grads_a, name="grads_a"), _chk(wire, name="wire")
    lib.call("rat_owner_pack", _p(mat), int(world), int(rank), int(d), _p(rows_a), _p(grads_a), _p(rows_b), _p(vals_b), int(max_pairs),
             _p(wire), _stream(wire))


def owner_unpack(mat, world, rank, d, wire, max_pairs, rows_a, grads_a, rows_b, vals_b, totals, extra_src=None, extra_dst=None, lib=None):
    lib = lib or get_lib()
    _chk(mat, torch.int32, "mat"), _chk(rows_a, torch.int32, "rows_a"), _chk(grads_a, name="grads_a"), _chk(wire, name="wire")
    _chk(totals, torch.int32, "totals")
    n_extra = 0 if extra_src is None else extra_src.numel()
    lib.call("rat_owner_unpack", _p(mat), int(world), int(rank), int(d), _p(wire), int(max_pairs), _p(rows_a), _p(grads_a), _p(rows_b),
             _p(vals_b), _p(totals), _p(extra_src), _p(extra_dst), int(n_extra), _stream(wire))


def owner_scatter(dense_a, dense_b, extra_out, lists, stride, world, cap_a, cap_b, d, n_extra, lib=None):
    lib = lib or get_lib()
    _chk(lists, name="lists")
    lib.call("rat_owner_scatter", _p(dense_a), _p(dense_b), _p(extra_out), _p(lists), int(stride), int(world), int(cap_a), int(cap_b),
             int(d), int(n_extra), _stream(lists))


# ----------------------------------------------------------------------------- K6b: the request path (rat_amd/online.py)
def bm25_query_prepare(ids, cols, table_ids, table_idf, table_offsets, first_row=None, lib=None):
    """ids int32 [Q, L] (full encoded rows) -> (qry_ids int32 [Q, F], qry_idf fp64 [Q, F]): retrieval.map_data_to_idf of ONE query
    batch against the pool's IDF tables (flat: sorted ids int32, weights fp64, offsets int64 [F + 1]), all on the device.
    ``first_row`` int64 [Q] (device): the batch holds several requests, row q belongs to the one that starts at row first_row[q], and
    every request is mapped as a query batch of its own (rat_bm25_query_prepare_seg)"""
    lib = lib or get_lib()
    _chk(ids, torch.int32, "ids"), _chk(cols, torch.int32, "cols"), _chk(table_ids, torch.int32, "table_ids")
    _chk(table_idf, torch.float64, "table_idf"), _chk(table_offsets, torch.int64, "table_offsets")
    Q, L = ids.shape
    F = cols.numel()
    assert table_offsets.numel() == F + 1
    qry_ids = torch.empty((Q, F), dtype=torch.int32, device=ids.device)
    qry_idf = torch.empty((Q, F), dtype=torch.float64, device=ids.device)
    if first_row is not None:
        _chk(first_row, torch.int64, "first_row")
        assert first_row.numel() == Q
        lib.call("rat_bm25_query_prepare_seg", _p(ids), _p(first_row), _p(cols), _p(table_ids), _p(table_idf), _p(table_offsets),
                 _p(qry_ids), _p(qry_idf), Q, L, F, _stream(ids))
        return qry_ids, qry_idf
    lib.call("rat_bm25_query_prepare", _p(ids), _p(cols), _p(table_ids), _p(table_idf), _p(table_offsets), _p(qry_ids), _p(qry_idf),
             Q, L, F, _stream(ids))
    return qry_ids, qry_idf


def _split_scan(lib, db_t, qry_ids, qry_idf, before, topk, splits):
    """what every split scan checks and allocates -> (capacity, Q, F, the workspace (int64 words), the outputs (values fp64 [Q, K],
    indices int64 [Q, K], lens int64 [Q]))"""
    _chk(db_t, torch.int32, "db_t"), _chk(qry_ids, torch.int32, "qry_ids"), _chk(qry_idf, torch.float64, "qry_idf")
    _chk(before, torch.int64, "before")
    F, capacity = db_t.shape
    Q = qry_ids.shape[0]
    assert tuple(qry_ids.shape) == (Q, F) and tuple(qry_idf.shape) == (Q, F)
    assert before is None or (before.ndim == 1 and before.numel() == Q)
    dev = db_t.device
    nbytes = lib.size("rat_bm25_topk_split_workspace", Q, int(topk), int(splits))
    ws = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.int64, device=dev)
    out = (torch.empty((Q, topk), dtype=torch.float64, device=dev), torch.empty((Q, topk), dtype=torch.int64, device=dev),
           torch.empty((Q,), dtype=torch.int64, device=dev))
    return capacity, Q, F, ws, out


def bm25_topk_split(db_t, qry_ids, qry_idf, topk, splits=0, before=None, header=None, ring=False, n_rows=None, lib=None):
    """rat_bm25_topk over `splits` ranges (0: the library chooses, from the capacity) of the live rows of db_t int32 [F, capacity],
    field-major -> (values fp64 [Q, K], indices int64 [Q, K], lens int64 [Q]).  The pool's form as in _pool_form: no header — all of
    db_t (rat_bm25_topk_split; its row count is db_t's row stride as well, so ``n_rows`` can only repeat it); a header — its first
    word is the row count, read on the device (rat_bm25_topk_split_dev); with ``ring`` the live rows start at slot header[1] and the
    indices returned are logical positions (rat_bm25_topk_split_ring).  ``before`` (int64 [Q], device): query q sees the logical rows
    i < before[q] only, clamped to [0, live row count] on the device (rat_bm25_topk_split_before, every form)."""
    lib = lib or get_lib()
    capacity, Q, F, ws, out = _split_scan(lib, db_t, qry_ids, qry_idf, before, topk, splits)
    bufs, tail = [_p(t) for t in out] + [_p(ws), ws.numel() * 8], (Q, F, int(topk), int(splits), _stream(db_t))
    if before is not None:
        form, n_rows = _pool_form(header, ring, n_rows, capacity)
        lib.call("rat_bm25_topk_split_before", _p(db_t), form, _p(header), n_rows, capacity, _p(qry_ids), _p(qry_idf), _p(before), *bufs,
                 *tail)
    elif ring or header is not None:
        _chk(header, torch.int64, "header")
        assert header is not None and header.numel() >= (2 if ring else 1)
        lib.call("rat_bm25_topk_split_ring" if ring else "rat_bm25_topk_split_dev", _p(db_t), _p(header), _p(qry_ids), _p(qry_idf),
                 *bufs, capacity, *tail)
    else:
        assert n_rows is None or int(n_rows) == capacity, "without a header the scan covers all of db_t: n_db is its row stride too"
        lib.call("rat_bm25_topk_split", _p(db_t), _p(qry_ids), _p(qry_idf), *bufs, capacity, *tail)
    return out


# ----------------------------------------------------------------------------- K6c: a pool that grows in place (rat_amd/online.py)
def pool_append(ids, labels, cols, db_t, count, pool_ids=None, pool_labels=None, lib=None):
    """rows `ids` int32 [M, L] / `labels` fp32 [M] (device) -> rows n .. n + M - 1 of db_t int32 [F, capacity] (transposed, the columns
    `cols`), pool_ids int32 [capacity, L] and pool_labels fp32 [capacity]; n = count[0] (int64, device) becomes n + M, on the device"""
    lib = lib or get_lib()
    _chk(ids, torch.int32, "ids"), _chk(labels, name="labels"), _chk(cols, torch.int32, "cols"), _chk(db_t, torch.int32, "db_t")
    _chk(count, torch.int64, "count"), _chk(pool_ids, torch.int32, "pool_ids"), _chk(pool_labels, name="pool_labels")
    M, L = ids.shape
    F, capacity = db_t.shape
    assert cols.numel() == F and labels.numel() == M and count.numel() >= 1 and (pool_ids is None) == (pool_labels is None)
    if pool_ids is not None:
        assert tuple(pool_ids.shape) == (capacity, L) and pool_labels.numel() == capacity
    lib.call("rat_pool_append", _p(ids), _p(labels), _p(cols), _p(db_t), _p(pool_ids), _p(pool_labels), _p(count), M, capacity, L, F,
             _stream(db_t))


# ----------------------------------------------------------------------------- a pool that slides: the same buffers as a ring
def pool_push(ids, labels, cols, db_t, header, pool_ids=None, pool_labels=None, lib=None):
    """pool_append into a ring: header = [n, head] (int64, device); row i goes to slot head + n + i (wrapped) of db_t, pool_ids and
    pool_labels, the max(0, n + M - capacity) oldest rows leave, all on the device.  M > capacity writes nothing."""
    lib = lib or get_lib()
    _chk(ids, torch.int32, "ids"), _chk(labels, name="labels"), _chk(cols, torch.int32, "cols"), _chk(db_t, torch.int32, "db_t")
    _chk(header, torch.int64, "header"), _chk(pool_ids, torch.int32, "pool_ids"), _chk(pool_labels, name="pool_labels")
    M, L = ids.shape
    F, capacity = db_t.shape
    assert cols.numel() == F and labels.numel() == M and header.numel() >= 2 and (pool_ids is None) == (pool_labels is None)
    if pool_ids is not None:
        assert tuple(pool_ids.shape) == (capacity, L) and pool_labels.numel() == capacity
    lib.call("rat_pool_push", _p(ids), _p(labels), _p(cols), _p(db_t), _p(pool_ids), _p(pool_labels), _p(header), M, capacity, L, F,
             _stream(db_t))


def pool_evict(header, m, capacity, lib=None):
    """the m oldest rows of a ring leave: header = [n, head] (int64, device) -> [n - m, head + m wrapped]; m < 0 or m >= n: nothing"""
    lib = lib or get_lib()
    _chk(header, torch.int64, "header")
    assert header.numel() >= 2
    lib.call("rat_pool_evict", _p(header), int(m), int(capacity), _stream(header))


def pool_delete(db_t, header, indices, scratch, pool_ids=None, pool_labels=None, lib=None):
    """the logical rows `indices` (int64, device, strictly ascending) of a ring leave; the survivors close up in place and in age order
    in db_t, pool_ids and pool_labels, header = [n, head] -> [n - len(indices), head], all on the device.  `scratch`: int32, at least
    capacity * max(F, L) elements (capacity * F without the row store).  An empty list launches nothing."""
    lib = lib or get_lib()
    _chk(db_t, torch.int32, "db_t"), _chk(header, torch.int64, "header"), _chk(indices, torch.int64, "indices")
    _chk(scratch, torch.int32, "scratch"), _chk(pool_ids, torch.int32, "pool_ids"), _chk(pool_labels, name="pool_labels")
    F, capacity = db_t.shape
    assert header.numel() >= 2 and indices.ndim == 1 and (pool_ids is None) == (pool_labels is None)
    L = F
    if pool_ids is not None:
        L = pool_ids.shape[1]
        assert pool_ids.shape[0] == capacity and pool_labels.numel() == capacity
    lib.call("rat_pool_delete", _p(db_t), _p(pool_ids), _p(pool_labels), _p(header), _p(indices), _p(scratch), scratch.numel() * 4,
             indices.numel(), capacity, L, F, _stream(db_t))


POOL_HOST, POOL_DEV, POOL_RING = 0, 1, 2               # rat_hip.h: where a kernel takes the pool's extent from
POOL_FIND_AUTO_GROUPS = 1024                           # RAT_POOL_FIND_AUTO_GROUPS


def _pool_form(header, ring, n_rows, capacity):
    """(pool_form, n_rows) of rat_pool_find / rat_pool_set_labels: no header — the row count by value (default: all `capacity` rows);
    a header — its first word, and with `ring` its second word as the slot of the oldest row"""
    if header is None:
        assert not ring
        n_rows = capacity if n_rows is None else int(n_rows)
        assert 0 <= n_rows <= capacity
        return POOL_HOST, n_rows
    _chk(header, torch.int64, "header")
    assert header.numel() >= (2 if ring else 1)
    return (POOL_RING if ring else POOL_DEV), 0


def pool_find(store, cols, keys, field_major, header=None, ring=False, n_rows=None, max_out=None, groups=0, out_idx=None,
              out_count=None, lib=None):
    """-> (out_idx int64 [max_out], out_count int64 [1]), on the device: the logical indices of the live rows of `store` that equal one
    of `keys` (int32 [M, C], sorted lexicographically and distinct) on the store's columns `cols` (int32 [C]), ascending, then -1;
    out_count is the number of matches even when max_out (default: the rows the store holds) is smaller.  `store`: int32
    [F, capacity] (field_major, as db_t) or [capacity, L] (as pool_ids).  The pool's form as in _pool_form.  groups = 0: the number of
    row ranges is chosen from the capacity."""
    lib = lib or get_lib()
    _chk(store, torch.int32, "store"), _chk(cols, torch.int32, "cols"), _chk(keys, torch.int32, "keys")
    assert store.ndim == 2 and keys.ndim == 2 and cols.ndim == 1 and keys.shape[1] == cols.numel() and keys.shape[0] >= 1
    if field_major:
        (store_cols, capacity), row_stride, col_stride = store.shape, 1, store.shape[1]
    else:
        (capacity, store_cols), row_stride, col_stride = store.shape, store.shape[1], 1
    form, n_rows = _pool_form(header, ring, n_rows, capacity)
    dev = store.device
    if out_idx is None:
        out_idx = torch.empty(capacity if max_out is None else int(max_out), dtype=torch.int64, device=dev)
    if out_count is None:
        out_count = torch.empty(1, dtype=torch.int64, device=dev)
    _chk(out_idx, torch.int64, "out_idx"), _chk(out_count, torch.int64, "out_count")
    max_out = out_idx.numel() if max_out is None else int(max_out)
    assert 0 <= max_out <= out_idx.numel() and out_count.numel() >= 1
    ws = torch.empty(2 * (int(groups) or POOL_FIND_AUTO_GROUPS) + 1, dtype=torch.int64, device=dev)
    lib.call("rat_pool_find", _p(store), row_stride, col_stride, store_cols, form, _p(header), n_rows, capacity, _p(cols), cols.numel(),
             _p(keys), keys.shape[0], _p(out_idx), max_out, _p(out_count), _p(ws), ws.numel() * 8, int(groups), _stream(store))
    return out_idx, out_count


def pool_set_labels(pool_labels, indices, labels, header=None, ring=False, n_rows=None, lib=None):
    """pool_labels[slot of logical indices[j]] = labels[j] (labels fp32 [m]) or labels[0] (fp32 [1]: one value for all), on the device;
    indices int64 [m], entries < 0 or >= the live row count are skipped (the -1 tail of pool_find's list).  The pool's form as in
    _pool_form."""
    lib = lib or get_lib()
    _chk(pool_labels, name="pool_labels"), _chk(indices, torch.int64, "indices"), _chk(labels, name="labels")
    m = indices.numel()
    assert indices.ndim == 1 and labels.numel() in (1, m)
    capacity = pool_labels.numel()
    form, n_rows = _pool_form(header, ring, n_rows, capacity)
    lib.call("rat_pool_set_labels", _p(pool_labels), form, _p(header), n_rows, capacity, _p(indices), _p(labels), m,
             0 if labels.numel() == 1 else 1, _stream(pool_labels))


# ----------------------------------------------------------------------------- a pool that looks at itself (rat_amd/online.py)
def pool_gather_rows(pool_ids, pool_labels, indices, header=None, ring=False, n_rows=None, lib=None):
    """-> (ids int32 [B, L], labels fp32 [B], before int64 [B]), on the device: the logical rows `indices` (int64 [B], device) of
    pool_ids int32 [capacity, L] / pool_labels fp32 [capacity]; an index < 0 or >= the live row count gives a row of zeros, label 0.
    before = the indices clamped to [0, live row count] — every row's horizon for bm25_topk_split(before=).  The pool's form as in
    _pool_form."""
    lib = lib or get_lib()
    _chk(pool_ids, torch.int32, "pool_ids"), _chk(pool_labels, name="pool_labels"), _chk(indices, torch.int64, "indices")
    capacity, L = pool_ids.shape
    B = indices.numel()
    assert indices.ndim == 1 and pool_labels.numel() == capacity
    form, n_rows = _pool_form(header, ring, n_rows, capacity)
    dev = pool_ids.device
    out_ids = torch.empty((B, L), dtype=torch.int32, device=dev)
    out_labels = torch.empty((B,), dtype=torch.float32, device=dev)
    out_before = torch.empty((B,), dtype=torch.int64, device=dev)
    lib.call("rat_pool_gather_rows", _p(pool_ids), _p(pool_labels), form, _p(header), n_rows, capacity, _p(indices), _p(out_ids),
             _p(out_labels), _p(out_before), B, L, _stream(pool_ids))
    return out_ids, out_labels, out_before


# ----------------------------------------------------------------------------- neighbours equal on given columns (rat_amd/online.py)
BM25_EXACT_AUTO_GROUPS = 256                           # RAT_BM25_EXACT_AUTO_GROUPS


def bm25_exact_count(db_t, ids, cols, exact_mask, before=None, header=None, ring=False, n_rows=None, groups=0, lib=None):
    """-> counts int64 [Q], on the device: for every row of ids int32 [Q, L] the number of live rows of db_t int32 [F, capacity] (below
    before[q], int64 [Q], when given) that equal it on every used column whose bit is set in `exact_mask` (bit f = used column f =
    column cols[f] of ids).  The pool's form as in _pool_form; groups = 0: the number of row ranges is chosen from the capacity."""
    lib = lib or get_lib()
    _chk(db_t, torch.int32, "db_t"), _chk(ids, torch.int32, "ids"), _chk(cols, torch.int32, "cols"), _chk(before, torch.int64, "before")
    F, capacity = db_t.shape
    Q, L = ids.shape
    assert cols.numel() == F and (before is None or (before.ndim == 1 and before.numel() == Q))
    form, n_rows = _pool_form(header, ring, n_rows, capacity)
    dev = db_t.device
    counts = torch.empty((Q,), dtype=torch.int64, device=dev)
    ws = torch.empty(Q * (int(groups) or BM25_EXACT_AUTO_GROUPS), dtype=torch.int64, device=dev)
    lib.call("rat_bm25_exact_count", _p(db_t), form, _p(header), n_rows, capacity, _p(ids), _p(cols), int(exact_mask), _p(before),
             _p(counts), _p(ws), ws.numel() * 8, Q, L, F, int(groups), _stream(db_t))
    return counts


def bm25_exact_plan(counts, topk, lib=None):
    """counts int64 [Q] (device) -> (first_row int64 [Q]: the first query with a candidate, for every query, 0 when there is none — what
    bm25_query_prepare takes as ``first_row``; listing int32 [1]: 1 when no count exceeds topk), on the device"""
    lib = lib or get_lib()
    _chk(counts, torch.int64, "counts")
    Q = counts.numel()
    first_row = torch.empty((Q,), dtype=torch.int64, device=counts.device)
    listing = torch.empty((1,), dtype=torch.int32, device=counts.device)
    lib.call("rat_bm25_exact_plan", _p(counts), _p(first_row), _p(listing), Q, int(topk), _stream(counts))
    return first_row, listing


def bm25_topk_split_exact(db_t, qry_ids, qry_idf, exact_mask, listing, topk, before=None, header=None, ring=False, n_rows=None, splits=0,
                          lib=None):
    """bm25_topk_split(before=) whose candidates are the rows equal to the query on the used columns in `exact_mask`: a candidate
    scores (the weights of the other columns it matches) + 1, anything else 0; listing int32 [1] (device) != 0: each query's entries in
    ascending index with value 1.0 instead.  before (int64 [Q], device) may be None.  The pool's form as in _pool_form."""
    lib = lib or get_lib()
    _chk(listing, torch.int32, "listing")
    assert listing.numel() >= 1
    capacity, Q, F, ws, out = _split_scan(lib, db_t, qry_ids, qry_idf, before, topk, splits)
    form, n_rows = _pool_form(header, ring, n_rows, capacity)
    lib.call("rat_bm25_topk_split_exact", _p(db_t), form, _p(header), n_rows, capacity, _p(qry_ids), _p(qry_idf), int(exact_mask),
             _p(before), _p(listing), *[_p(t) for t in out], _p(ws), ws.numel() * 8, Q, F, int(topk), int(splits), _stream(db_t))
    return out


# ----------------------------------------------------------------------------- evaluation metrics on the device (rat_amd/metrics.py)
def eval_metrics(y_pred, y_true, group=None, lib=None):
    """-> float64 [8] on the inputs' device, nothing read back: {logloss, AUC, GAUC, n_pos, n_neg, groups counted, rows in the counted
    groups, status bits} (include/rat_hip.h: rat_eval_metrics) of y_pred fp32 [n] against y_true fp32 [n]; group int32 [n] or None
    (then GAUC is NaN).  Status bits: 1 a NaN prediction, 2 a label that is neither 0 nor 1, 4 one class only, 8 no group holds both
    classes — the metric a bit concerns is NaN."""
    lib = lib or get_lib()
    _chk(y_pred, name="y_pred"), _chk(y_true, name="y_true"), _chk(group, torch.int32, "group")
    n = y_pred.numel()
    if y_pred.ndim != 1 or tuple(y_true.shape) != (n,) or (group is not None and tuple(group.shape) != (n,)):
        raise ValueError("eval_metrics takes 1-D vectors of one length")
    dev = y_pred.device
    if y_true.device != dev or (group is not None and group.device != dev):
        raise ValueError("eval_metrics: the vectors sit on different devices")
    nbytes = lib.size("rat_eval_metrics_workspace", n, 0 if group is None else 1)
    ws = torch.empty((nbytes + 255) // 8 + 32, dtype=torch.int64, device=dev)
    skip = (-ws.data_ptr() % 256) // 8                                           # the C ABI wants 256-byte alignment
    ws = ws[skip:]
    out = torch.empty(8, dtype=torch.float64, device=dev)
    lib.call("rat_eval_metrics", _p(y_pred), _p(y_true), _p(group), n, _p(out), _p(ws), nbytes, _stream(y_pred))
    return out


MAX_CUTOFFS = 8


def eval_rank_metrics(y_pred, y_true, group, cutoffs, lib=None):
    """-> float64 [m, 8] on the inputs' device, nothing read back: per cutoff {NDCG@k, MRR@k, HitRate@k, groups counted, groups seen,
    hits, k, status bits} (include/rat_hip.h: rat_eval_rank_metrics) of y_pred fp32 [n] against y_true fp32 [n] inside the groups of
    group int32 [n]; cutoffs: 1 <= m <= 8 host integers in [1, 2^31 - 1].  Status bits: 1 a NaN prediction, 2 a label that is neither 0
    nor 1, 16 no group holds a positive — any of them makes the three metrics NaN."""
    lib = lib or get_lib()
    if group is None:
        raise ValueError("eval_rank_metrics needs the group ids")
    _chk(y_pred, name="y_pred"), _chk(y_true, name="y_true"), _chk(group, torch.int32, "group")
    n = y_pred.numel()
    if y_pred.ndim != 1 or tuple(y_true.shape) != (n,) or tuple(group.shape) != (n,):
        raise ValueError("eval_rank_metrics takes 1-D vectors of one length")
    dev = y_pred.device
    if y_true.device != dev or group.device != dev:
        raise ValueError("eval_rank_metrics: the vectors sit on different devices")
    ks = [k for k in cutoffs]
    if not 1 <= len(ks) <= MAX_CUTOFFS:
        raise ValueError("eval_rank_metrics takes 1 to %d cutoffs, got %d" % (MAX_CUTOFFS, len(ks)))
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 2 ** 31 - 1:
            raise ValueError("eval_rank_metrics: a cutoff is an integer in [1, 2^31 - 1], got %r" % (k,))
    host_ks = (ctypes.c_int32 * len(ks))(*[int(k) for k in ks])
    nbytes = lib.size("rat_eval_rank_metrics_workspace", n, len(ks))
    ws = torch.empty((nbytes + 255) // 8 + 32, dtype=torch.int64, device=dev)
    skip = (-ws.data_ptr() % 256) // 8                                           # the C ABI wants 256-byte alignment
    ws = ws[skip:]
    out = torch.empty((len(ks), 8), dtype=torch.float64, device=dev)
    lib.call("rat_eval_rank_metrics", _p(y_pred), _p(y_true), _p(group), n, ctypes.cast(host_ks, ctypes.c_void_p), len(ks), _p(out),
             _p(ws), nbytes, _stream(y_pred))
    return out


# ----------------------------------------------------------------------------- the end of a request (rat_amd/online.py)
MAX_TOPN = 64                                          # RAT_MAX_TOPN


def _first_row_arg(first_row, B, dev, what):
    """first_row int64 [B] on `dev`, checked by shape, dtype and device; its contents are the kernels' business (they clamp)"""
    _chk(first_row, torch.int64, "first_row")
    if tuple(first_row.shape) != (B,):
        raise ValueError("%s: first_row must be [%d] (one entry per row), got shape %s" % (what, B, tuple(first_row.shape)))
    if first_row.device != dev:
        raise ValueError("%s: the tensors sit on different devices" % what)


def topn_seg(y, first_row, n, lib=None):
    """-> (pos int32 [B, n], val fp32 [B, n], lens int32 [B]) on the inputs' device, nothing read back: at every row h that opens a
    request — first_row[h] == h; first_row int64 [B]: for every row the row that opens its request — the positions inside the request
    and the values of its min(n, request size) largest entries of y fp32 [B], in the order np.argsort(-y_request, kind="stable")[:n],
    padded with -1 / 0.0; lens[h] their number.  Every other row: -1 / 0.0 / 0.  1 <= n <= MAX_TOPN (include/rat_hip.h: rat_topn_seg)."""
    lib = lib or get_lib()
    _chk(y, name="y")
    if y.ndim != 1 or y.numel() < 1:
        raise ValueError("topn_seg takes a non-empty 1-D vector y, got shape %s" % (tuple(y.shape),))
    B, dev = y.numel(), y.device
    _first_row_arg(first_row, B, dev, "topn_seg")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_TOPN:
        raise ValueError("topn_seg takes an integer 1 <= n <= %d, got %r" % (MAX_TOPN, n))
    n = int(n)
    pos = torch.empty((B, n), dtype=torch.int32, device=dev)
    val = torch.empty((B, n), dtype=torch.float32, device=dev)
    lens = torch.empty((B,), dtype=torch.int32, device=dev)
    lib.call("rat_topn_seg", _p(y), _p(first_row), B, n, _p(pos), _p(val), _p(lens), _stream(y))
    return pos, val, lens


def candidates_expand(ctx, cand, cols, first_row, lib=None):
    """-> ids int32 [B, L] on the inputs' device: ids[b, cols[w]] = cand[b, w] (cand int32 [B, W], cols int32 [W] on the device,
    distinct and in [0, L)), every other column from ctx[first_row[b]] (ctx int32 [B, L]: the row that opens a request holds the
    request's context, no other row is read; first_row int64 [B]) — the full rows of a request's candidates from one context row
    (include/rat_hip.h: rat_candidates_expand)."""
    lib = lib or get_lib()
    _chk(ctx, torch.int32, "ctx"), _chk(cand, torch.int32, "cand"), _chk(cols, torch.int32, "cols")
    if ctx.ndim != 2 or cand.ndim != 2 or cols.ndim != 1 or ctx.shape[0] < 1 or ctx.shape[1] < 1 or cols.numel() < 1:
        raise ValueError("candidates_expand takes ctx [B, L], cand [B, W] and cols [W], got shapes %s, %s, %s"
                         % (tuple(ctx.shape), tuple(cand.shape), tuple(cols.shape)))
    B, L = ctx.shape
    W = cols.numel()
    if tuple(cand.shape) != (B, W):
        raise ValueError("candidates_expand: cand must be [%d, %d] (one row per row of ctx, one column per entry of cols), got shape %s"
                         % (B, W, tuple(cand.shape)))
    dev = ctx.device
    if cand.device != dev or cols.device != dev:
        raise ValueError("candidates_expand: the tensors sit on different devices")
    _first_row_arg(first_row, B, dev, "candidates_expand")
    out = torch.empty((B, L), dtype=torch.int32, device=dev)
    lib.call("rat_candidates_expand", _p(ctx), _p(cand), _p(cols), _p(first_row), B, L, W, _p(out), _stream(ctx))
    return out


RANK_ROWS, RANK_TILE = 256, 1024                       # csrc/rank.hip: RK_THREADS rows per work-group, RK_TILE rows per LDS tile


def rank_seg(y, first_row, lib=None):
    """-> (order int32 [B], val fp32 [B], rank int32 [B]) on the inputs' device, nothing read back: every request's whole ranking.
    For the request that opens at row h and ends before row e (first_row int64 [B]: for every row the row that opens its request),
    order[h:e] = np.argsort(-y[h:e], kind="stable") — positions inside the request, best first; equal values in input order, a NaN
    last —, val[h:e] = y[h:e][order[h:e]] bit for bit, and rank[b] is row b's place in its request: order[h + rank[b]] == b - h.  A row
    of no request: -1 / 0.0 / -1.  Any request length (include/rat_hip.h: rat_rank_seg)."""
    lib = lib or get_lib()
    _chk(y, name="y")
    if y.ndim != 1 or y.numel() < 1:
        raise ValueError("rank_seg takes a non-empty 1-D vector y, got shape %s" % (tuple(y.shape),))
    B, dev = y.numel(), y.device
    _first_row_arg(first_row, B, dev, "rank_seg")
    order = torch.empty((B,), dtype=torch.int32, device=dev)
    val = torch.empty((B,), dtype=torch.float32, device=dev)
    rank = torch.empty((B,), dtype=torch.int32, device=dev)
    lib.call("rat_rank_seg", _p(y), _p(first_row), B, _p(order), _p(val), _p(rank), _stream(y))
    return order, val, rank


# ----------------------------------------------------------------------------- a device-resident item catalogue (rat_amd/online.py)
def _int_arg(v, what, lo):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo:
        raise ValueError("%s must be an integer >= %d, got %r" % (what, lo, v))
    return int(v)


def _exclusion_arg(ex_items, ex_offsets, R, dev, what):
    """ex_items int32 [E] and ex_offsets int64 [R + 1] on `dev`, checked by shape, dtype and device; the kernels clamp the offsets"""
    _chk(ex_items, torch.int32, "ex_items"), _chk(ex_offsets, torch.int64, "ex_offsets")
    if ex_items.ndim != 1 or tuple(ex_offsets.shape) != (R + 1,):
        raise ValueError("%s: the exclusion lists are ex_items [E] and ex_offsets [%d] (one more than requests), got shapes %s, %s"
                         % (what, R + 1, tuple(ex_items.shape), tuple(ex_offsets.shape)))
    if ex_items.device != dev or ex_offsets.device != dev:
        raise ValueError("%s: the tensors sit on different devices" % what)


def catalogue_expand(ctx, cat, cols, first_row, items=None, item0=0, lib=None):
    """-> ids int32 [B, L] on the inputs' device: ids[b, cols[w]] = cat[i(b), w] (cat int32 [M, W], the catalogue; cols int32 [W] on
    the device, distinct and in [0, L)), every other column from ctx[first_row[b]] (ctx int32 [B, L]: the row that opens a request
    holds its context, no other row is read; first_row int64 [B]).  ``items`` int32 [B]: i(b) = items[b]; ``items=None``, the sweep
    form: i(b) = item0 + (b - first_row[b]), the k-th row of a request is item item0 + k.  Either way i(b) is clamped to [0, M)
    (include/rat_hip.h: rat_catalogue_expand)."""
    lib = lib or get_lib()
    _chk(ctx, torch.int32, "ctx"), _chk(cat, torch.int32, "cat"), _chk(cols, torch.int32, "cols"), _chk(items, torch.int32, "items")
    if ctx.ndim != 2 or cat.ndim != 2 or cols.ndim != 1 or ctx.shape[0] < 1 or ctx.shape[1] < 1 or cat.shape[0] < 1 or cols.numel() < 1:
        raise ValueError("catalogue_expand takes ctx [B, L], cat [M, W] and cols [W], got shapes %s, %s, %s"
                         % (tuple(ctx.shape), tuple(cat.shape), tuple(cols.shape)))
    B, L = ctx.shape
    M, W = cat.shape
    if cols.numel() != W:
        raise ValueError("catalogue_expand: cat is %d wide for the %d columns in cols" % (W, cols.numel()))
    if items is not None and tuple(items.shape) != (B,):
        raise ValueError("catalogue_expand: items must be [%d] (one catalogue index per row of ctx), got shape %s" % (B, tuple(items.shape)))
    if isinstance(item0, bool) or not isinstance(item0, (int, np.integer)):
        raise ValueError("catalogue_expand: item0 must be an integer, got %r" % (item0,))
    dev = ctx.device
    if cat.device != dev or cols.device != dev or (items is not None and items.device != dev):
        raise ValueError("catalogue_expand: the tensors sit on different devices")
    _first_row_arg(first_row, B, dev, "catalogue_expand")
    out = torch.empty((B, L), dtype=torch.int32, device=dev)
    lib.call("rat_catalogue_expand", _p(ctx), _p(cat), _p(items), int(item0), _p(cols), _p(first_row), B, L, W, M, _p(out), _stream(ctx))
    return out


def topn_exclude(y, first_row, item0, rows_per_request, ex_items, ex_offsets, lib=None):
    """-> y' fp32 [B]: -inf where the catalogue item of row b, item0 + (b - first_row[b]), is in the exclusion list of request
    first_row[b] // rows_per_request — ex_items int32 [E], ascending inside ex_offsets[r] .. ex_offsets[r + 1] (int64 [R + 1]) —,
    otherwise y[b] bit for bit (include/rat_hip.h: rat_topn_exclude)."""
    lib = lib or get_lib()
    _chk(y, name="y")
    if y.ndim != 1 or y.numel() < 1:
        raise ValueError("topn_exclude takes a non-empty 1-D vector y, got shape %s" % (tuple(y.shape),))
    B, dev = y.numel(), y.device
    _first_row_arg(first_row, B, dev, "topn_exclude")
    if isinstance(item0, bool) or not isinstance(item0, (int, np.integer)):
        raise ValueError("topn_exclude: item0 must be an integer, got %r" % (item0,))
    m = _int_arg(rows_per_request, "topn_exclude: rows_per_request", 1)
    if ex_offsets is None or ex_items is None or ex_offsets.ndim != 1 or ex_offsets.numel() < 2:
        raise ValueError("topn_exclude takes ex_items [E] and ex_offsets [R + 1]")
    R = ex_offsets.numel() - 1
    _exclusion_arg(ex_items, ex_offsets, R, dev, "topn_exclude")
    out = torch.empty_like(y)
    lib.call("rat_topn_exclude", _p(y), _p(first_row), int(item0), m, _p(ex_items), _p(ex_offsets), ex_items.numel(), R, B, _p(out),
             _stream(y))
    return out


def topn_merge(run_item, run_val, run_len, pos, val, lens, heads, item0, ex_items=None, ex_offsets=None, lib=None):
    """Merges a chunk's page into the running page of R requests IN PLACE (nothing is returned): run_item int32 [R, n], run_val fp32
    [R, n], run_len int32 [R]; the chunk's page is ``topn_seg``'s (pos int32 [B, n], val fp32 [B, n], lens int32 [B]) at the rows
    heads int64 [R], an entry's catalogue item item0 + pos.  Entries whose item is in the request's exclusion list (ex_items int32
    [E], ex_offsets int64 [R + 1]; both None: no lists) are dropped; the rest merge in topn_seg's order over (value, item), a running
    entry before a chunk entry of equal value; the first n survive, padded with -1 / 0.0 (include/rat_hip.h: rat_topn_merge)."""
    lib = lib or get_lib()
    _chk(run_item, torch.int32, "run_item"), _chk(run_val, name="run_val"), _chk(run_len, torch.int32, "run_len")
    _chk(pos, torch.int32, "pos"), _chk(val, name="val"), _chk(lens, torch.int32, "lens"), _chk(heads, torch.int64, "heads")
    if run_item.ndim != 2 or run_item.shape[0] < 1 or not 1 <= run_item.shape[1] <= MAX_TOPN:
        raise ValueError("topn_merge takes a running page run_item [R, n] with 1 <= n <= %d, got shape %s" % (MAX_TOPN, tuple(run_item.shape)))
    R, n = run_item.shape
    if tuple(run_val.shape) != (R, n) or tuple(run_len.shape) != (R,) or tuple(heads.shape) != (R,):
        raise ValueError("topn_merge: run_val must be [%d, %d], run_len and heads [%d], got shapes %s, %s, %s"
                         % (R, n, R, tuple(run_val.shape), tuple(run_len.shape), tuple(heads.shape)))
    if pos.ndim != 2 or pos.shape[0] < 1 or pos.shape[1] != n or val.shape != pos.shape or tuple(lens.shape) != (pos.shape[0],):
        raise ValueError("topn_merge: the chunk's page is pos [B, %d], val [B, %d], lens [B], got shapes %s, %s, %s"
                         % (n, n, tuple(pos.shape), tuple(val.shape), tuple(lens.shape)))
    if isinstance(item0, bool) or not isinstance(item0, (int, np.integer)):
        raise ValueError("topn_merge: item0 must be an integer, got %r" % (item0,))
    dev = run_item.device
    if any(t.device != dev for t in (run_val, run_len, pos, val, lens, heads)):
        raise ValueError("topn_merge: the tensors sit on different devices")
    if (ex_items is None) != (ex_offsets is None):
        raise ValueError("topn_merge: ex_items and ex_offsets come together")
    E = 0
    if ex_items is not None:
        _exclusion_arg(ex_items, ex_offsets, R, dev, "topn_merge")
        E = ex_items.numel()
    lib.call("rat_topn_merge", _p(run_item), _p(run_val), _p(run_len), _p(pos), _p(val), _p(lens), _p(heads), int(item0),
             _p(ex_items) if E else None, _p(ex_offsets) if E else None, E, R, pos.shape[0], n, _stream(run_item))


# ----------------------------------------------------------------------------- candidate retrieval through posting lists
def bm25_topk_postings(db_t, post_ids, post_rows, n_sorted, qry_ids, qry_idf, vary_mask, ctx_indices, ctx_row, header=None,
                       n_rows=None, lib=None):
    """rat_bm25_topk's result for queries whose requests share a context, from posting lists instead of a scan (include/rat_hip.h:
    rat_bm25_topk_postings) -> (values fp64 [Q, K], indices int64 [Q, K], lens int64 [Q]).  db_t, post_ids, post_rows int32
    [F, capacity]; n_sorted int64 [1]; qry_ids int32 / qry_idf fp64 [Q, F]; vary_mask: bit f = used column f varies inside a request;
    ctx_indices int64 [R, K], the requests' context lists (K = its width); ctx_row int64 [Q], the list of every query.  The pool's
    form as in _pool_form, without ``ring``.  Shapes, dtypes, devices and contiguity are checked; no content is read."""
    lib = lib or get_lib()
    for t, dtype, name in ((db_t, torch.int32, "db_t"), (post_ids, torch.int32, "post_ids"), (post_rows, torch.int32, "post_rows"),
                           (n_sorted, torch.int64, "n_sorted"), (qry_ids, torch.int32, "qry_ids"), (qry_idf, torch.float64, "qry_idf"),
                           (ctx_indices, torch.int64, "ctx_indices"), (ctx_row, torch.int64, "ctx_row")):
        if not torch.is_tensor(t):
            raise TypeError("bm25_topk_postings: %s must be a tensor" % name)
        _chk(t, dtype, name)
    if db_t.ndim != 2 or not 1 <= db_t.shape[0] <= 32 or db_t.shape[1] < 1:
        raise ValueError("bm25_topk_postings: db_t must be [F, capacity] with 1 <= F <= 32, got shape %s" % (tuple(db_t.shape),))
    F, capacity = db_t.shape
    if tuple(post_ids.shape) != (F, capacity) or tuple(post_rows.shape) != (F, capacity):
        raise ValueError("bm25_topk_postings: post_ids and post_rows must be [%d, %d] as db_t, got shapes %s, %s"
                         % (F, capacity, tuple(post_ids.shape), tuple(post_rows.shape)))
    if n_sorted.numel() < 1:
        raise ValueError("bm25_topk_postings: n_sorted must hold one int64")
    if qry_ids.ndim != 2 or qry_ids.shape[0] < 1 or qry_ids.shape[1] != F or qry_idf.shape != qry_ids.shape:
        raise ValueError("bm25_topk_postings: qry_ids and qry_idf must be [Q, %d], got shapes %s, %s"
                         % (F, tuple(qry_ids.shape), tuple(qry_idf.shape)))
    Q = qry_ids.shape[0]
    if ctx_indices.ndim != 2 or ctx_indices.shape[0] < 1 or not 1 <= ctx_indices.shape[1] <= 32:
        raise ValueError("bm25_topk_postings: ctx_indices must be [R, K] with R >= 1 and 1 <= K <= 32, got shape %s"
                         % (tuple(ctx_indices.shape),))
    R, K = ctx_indices.shape
    if tuple(ctx_row.shape) != (Q,):
        raise ValueError("bm25_topk_postings: ctx_row must be [%d], got shape %s" % (Q, tuple(ctx_row.shape)))
    if isinstance(vary_mask, bool) or not isinstance(vary_mask, (int, np.integer)) or not 0 <= int(vary_mask) < (1 << 32):
        raise ValueError("bm25_topk_postings: vary_mask must be an unsigned 32-bit integer, got %r" % (vary_mask,))
    dev = db_t.device
    if any(t.device != dev for t in (post_ids, post_rows, n_sorted, qry_ids, qry_idf, ctx_indices, ctx_row)) or \
            (header is not None and header.device != dev):
        raise ValueError("bm25_topk_postings: the tensors sit on different devices")
    form, n_rows = _pool_form(header, False, n_rows, capacity)
    out = (torch.empty((Q, K), dtype=torch.float64, device=dev), torch.empty((Q, K), dtype=torch.int64, device=dev),
           torch.empty((Q,), dtype=torch.int64, device=dev))
    lib.call("rat_bm25_topk_postings", _p(db_t), form, _p(header), n_rows, capacity, _p(post_ids), _p(post_rows), _p(n_sorted),
             _p(qry_ids), _p(qry_idf), int(vary_mask), _p(ctx_indices), _p(ctx_row), R, *[_p(t) for t in out], Q, F, K, _stream(db_t))
    return out
