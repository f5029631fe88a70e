"""Online scoring: a fresh batch of encoded rows in, click probabilities out — retrieval, batch assembly and the eval forward on the
device, against a pool that stays resident in HBM.

The offline path needs the neighbours of every row pre-computed (``retrieval.precompute_retrieval`` -> ``retrieval_{K}_{split}.h5`` ->
``data.DeviceRetrievalBatches`` -> ``predict_generator``).  Here a request runs

    rat_bm25_query_prepare  ->  rat_bm25_topk_split  ->  rat_batch_assemble  ->  the model's eval forward

with nothing but the request's ids going in and ``y_pred`` coming out: no D2H copy, no ``.item()``, no numpy in between.  One
request = one query batch of the reference (the IDF mapping's dtype rule looks at the request's first row, ``retrieval.map_data_to_idf``),
so ``OnlineScorer.score(ids)`` returns what the offline path returns for ``precompute_retrieval(..., qry_batch_size=None)`` over the
same rows.  From the third request of a batch size on the whole chain is ONE hipGraph on one stream (``graph.EvalGraph``'s scheme: a
static input, weights read at replay time).

Not served online (refused at construction): exact-match columns (numbering the groups needs a host ``np.unique`` over pool and
queries), label-wise retrieval, topK > 32, more than 32 retrieval columns, data-parallel models.  A changed pool is a new
``RetrievalIndex``.
"""
import numpy as np
import torch

from . import ops, retrieval
from ._lib import get_lib
from .data import DeviceBatch

MAX_TOPK = 32
MAX_COLS = 32


def _as_device_ids(ids, device):
    """numpy / host tensor / device tensor, integer-valued, any of the usual dtypes -> contiguous int32 [B, L] on `device`"""
    if not torch.is_tensor(ids):
        ids = torch.from_numpy(np.ascontiguousarray(np.asarray(ids)))
    if ids.ndim != 2:
        raise ValueError("ids must be [B, L] encoded rows, got shape %s" % (tuple(ids.shape),))
    ids = ids.to(device, non_blocking=True)
    if ids.dtype != torch.int32:
        ids = ids.to(torch.int32)
    return ids.contiguous()


class RetrievalIndex:
    """A retrieval pool resident in HBM: its id columns field-major (what the top-K scan streams) and its per-column IDF tables
    (built once, on the host, by ``retrieval.idf_tables`` — numpy's float64 ``log``, so the weights are bit-identical to the offline
    path's).  ``retrieve(ids)`` is ``BM25_topk_retrieval_v4(pool, ids[:, cols], topK=K)`` of one query batch, device tensors out."""

    def __init__(self, pool_array, col_indices, topK, device, lib=None, exact_match_col_indices=None, splits=0):
        if exact_match_col_indices:
            raise ValueError("online retrieval does not support exact-match columns (exact_match_col_indices=%s): numbering the groups "
                             "needs a host pass over pool and queries" % (list(exact_match_col_indices),))
        self.topK, self.splits = int(topK), int(splits)
        if not 0 < self.topK <= MAX_TOPK:
            raise ValueError("online retrieval supports 1 <= topK <= %d, got topK = %d" % (MAX_TOPK, self.topK))
        cols = [int(c) for c in col_indices]
        if not 0 < len(cols) <= MAX_COLS:
            raise ValueError("online retrieval supports 1 to %d used columns, got %d" % (MAX_COLS, len(cols)))
        pool_array = np.asarray(pool_array)
        if pool_array.ndim != 2 or len(pool_array) == 0:
            raise ValueError("pool_array must be a non-empty [N, L + 1] encoded table (label last)")
        self.row_len = pool_array.shape[1] - 1
        if min(cols) < 0 or max(cols) >= self.row_len:
            raise ValueError("used column %s outside the %d id columns of the pool" % (cols, self.row_len))
        self._lib = lib or get_lib()
        self.device = dev = torch.device(device)
        db = pool_array[:, cols].astype(int)                                   # as precompute_retrieval slices the pool
        tables = retrieval.idf_tables(db)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
        self.n_db = len(db)
        self.db_t = up(retrieval._as_int32(db, "pool").T)                      # [F][N] field-major
        self.cols = up(np.asarray(cols, dtype=np.int32))
        self.table_ids = up(np.concatenate([retrieval._as_int32(v, "pool") for v, _ in tables]))
        self.table_idf = up(np.concatenate([w for _, w in tables]).astype(np.float64))
        self.table_offsets = up(np.concatenate([[0], np.cumsum([len(v) for v, _ in tables])]).astype(np.int64))

    def retrieve(self, ids):
        """ids [B, L] (full encoded rows) -> (values fp64 [B, K], indices int64 [B, K] with -1 padding, lens int64 [B]), on the device"""
        ids = _as_device_ids(ids, self.device)
        if ids.shape[1] != self.row_len:
            raise ValueError("ids have %d columns, the pool's rows have %d" % (ids.shape[1], self.row_len))
        if ids.shape[0] == 0:
            raise ValueError("empty request")
        qry_ids, qry_idf = ops.bm25_query_prepare(ids, self.cols, self.table_ids, self.table_idf, self.table_offsets, lib=self._lib)
        return ops.bm25_topk_split(self.db_t, qry_ids, qry_idf, self.topK, splits=self.splits, lib=self._lib)


class _RequestGraph:
    """retrieve -> assemble -> eval forward of one request size as one linear hipGraph (one stream, no parallel branches)"""

    def __init__(self, scorer, ids):
        self.static_ids = ids.clone()
        self._stream = torch.cuda.Stream(device=ids.device)
        self.graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.no_grad(), torch.cuda.graph(self.graph, stream=self._stream, capture_error_mode="thread_local"):
            self.y_pred = scorer._score_eager(self.static_ids)

    def run(self, ids):
        if ids.data_ptr() != self.static_ids.data_ptr():
            self.static_ids.copy_(ids, non_blocking=True)
        self.graph.replay()
        return self.y_pred.clone()


class OnlineScorer:
    """``score(ids)``: fp32 [B] predictions of a trained model for fresh encoded rows ``ids`` [B, L], the neighbours retrieved from
    ``pool_array`` ([N, L + 1], label last) on the spot.  ``retrieval_configs`` is the dataset's block (``topK``, ``used_cols`` or
    ``used_col_indices``, ...).  ``graph=True``: after ``graph_warmup`` eager requests of a batch size (<= ``graph_max_batch``) the
    chain is captured and replayed; the weights are read at replay time, so the graph survives optimizer steps and load_state_dict."""

    graph_warmup = 2
    graph_max_batch = 4096
    graph_sizes = 16               # at most this many request sizes get a graph; others stay eager

    def __init__(self, model, pool_array, retrieval_configs, graph=True, lib=None):
        cfg = retrieval_configs
        if cfg.get("exact_match_col_indices") or cfg.get("exact_match_cols"):
            raise ValueError("online scoring does not support exact-match columns (exact_match_cols / exact_match_col_indices are set)")
        if cfg.get("label_wise", False):
            raise ValueError("online scoring does not support label_wise retrieval (the model takes [B, 1 + K] samples, not [B, 1 + 2K])")
        if model._dp():
            raise ValueError("online scoring serves a single device; this model runs data-parallel")
        cols = cfg.get("used_col_indices")
        if cols is None:
            cols = retrieval.used_col_indices(model._feature_map, cfg)
        self.model = model
        self.device = model.device
        self._lib = lib or model._lib
        self.index = RetrievalIndex(pool_array, cols, cfg["topK"], self.device, lib=self._lib)
        pool_array = np.asarray(pool_array)
        self.pool_ids = torch.from_numpy(np.ascontiguousarray(pool_array[:, :-1].astype(np.int32))).to(self.device)
        self.pool_labels = torch.from_numpy(np.ascontiguousarray(pool_array[:, -1].astype(np.float32))).to(self.device)
        self.graph = bool(graph)
        self._consts = {}              # request size -> (rows = arange(B), labels = zeros(B))
        self._graphs = {}              # key -> [eager requests seen, _RequestGraph | False | None]

    # ------------------------------------------------------------------------------------------------------------------
    def _constants(self, B):
        c = self._consts.get(B)
        if c is None:
            c = self._consts[B] = (torch.arange(B, dtype=torch.int64, device=self.device),
                                   torch.zeros(B, dtype=torch.float32, device=self.device))
        return c

    def _assemble(self, ids):
        rows, labels = self._constants(ids.shape[0])
        _values, indices, _lens = self.index.retrieve(ids)
        # the request is the query table, the kernel's own index output the neighbour lists; -1 keeps its numpy meaning, as offline
        return ops.batch_assemble(ids, labels, self.pool_ids, self.pool_labels, indices, rows, lib=self._lib)

    def _score_eager(self, ids):
        y_pred, _loss, _reg, _saved = self.model._run_forward(self._assemble(ids), save=False, with_reg=False)
        return y_pred.reshape(-1)

    def batch(self, ids):
        """-> data.DeviceBatch (idx [B, 1 + K, L], label_ids [B, 1 + K], y_true = zeros): what the model's forward consumes"""
        return DeviceBatch(*self._assemble(_as_device_ids(ids, self.device)))

    def score(self, ids):
        if self.model.training:
            raise RuntimeError("OnlineScorer.score needs the model in eval mode (model.eval())")
        ids = _as_device_ids(ids, self.device)
        with torch.no_grad():
            g = self._graph_for(ids)
            return g.run(ids) if g is not None else self._score_eager(ids)

    def _graph_for(self, ids):
        B = ids.shape[0]
        if not (self.graph and ids.is_cuda and B <= self.graph_max_batch):
            return None
        key = (B, self.model._eval_graph_key((B, self.index.topK + 1, ids.shape[1])))
        entry = self._graphs.get(key)
        if entry is None:
            if len(self._graphs) >= self.graph_sizes:
                return None
            entry = self._graphs[key] = [0, None]
        if entry[1] is None:
            entry[0] += 1
            if entry[0] <= self.graph_warmup:
                return None
            try:
                entry[1] = _RequestGraph(self, ids)
            except Exception as exc:
                import logging
                logging.warning("hipGraph capture of the online request failed (%s: %s); continuing with eager launches",
                                type(exc).__name__, exc)
                entry[1] = False
        return entry[1] or None
