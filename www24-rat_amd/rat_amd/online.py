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

The pool can grow.  ``RetrievalIndex(..., capacity=C)`` / ``OnlineScorer(..., capacity=C)`` allocate every device buffer for C rows
once; ``append(rows)`` writes labelled rows behind the current ones on the device (``rat_pool_append``), and the scan and the assembly
read the row count from device memory (``rat_bm25_topk_split_dev``, ``rat_batch_assemble_dev``) — so no address and no kernel argument
of a request changes, and a request graph captured before an append serves the grown pool after it.  The IDF weights stay numpy's
float64 ``log``: the index keeps the per-column (distinct ids, counts) on the host, merges the new rows into them and uploads the
tables into the same device buffers.  After ``append`` the object answers exactly like a fresh one over ``concatenate([pool, rows])``.
Without ``capacity`` nothing changes: the immutable index, the same kernels and launches as before.

The pool can slide.  ``capacity=C, window=True`` uses the same buffers as a ring: the device header is two words, the live row count
and ``head``, the physical slot of the oldest live row.  ``append(rows)`` never refuses for lack of room — when the window is full the
oldest rows leave in the same call (``rat_pool_push``) — and ``evict(m)`` drops the m oldest (``rat_pool_evict``).  Everything a
request sees is LOGICAL (0 = the oldest live row): the indices ``retrieve`` returns, the tie rule (the older row wins), the row a
``-1`` padding resolves to (the newest).  The scan and the assembly map a logical row to its slot on the device
(``rat_bm25_topk_split_ring``, ``rat_batch_assemble_ring``) from that header, so captured request graphs survive appends and evictions
alike, and at any moment the object answers exactly like a fresh one over the live rows in age order.  The index keeps the used columns
of the live rows in a host ring to know which ids leave; an id whose count reaches zero leaves its column's table.
Without ``window`` a pool with ``capacity`` is append-only and refuses rows when it is full.

The window can lose any row.  ``delete(indices)`` (``window=True`` only) takes logical positions as ``retrieve`` returns them; the
survivors close up in place and in age order on the device (``rat_pool_delete``, staged through a scratch buffer the index allocates
on the first delete), every survivor's index drops by the number of deleted rows older than it, and ``head`` stays.  The host ring is
compacted the same way and the counts of the deleted rows leave the tables, so afterwards the object again answers exactly like a fresh
one over the live rows in age order — and captured request graphs are kept, as the row count is read on the device.

The pool is addressed by key as well as by position.  ``find(cols, keys)`` searches the live rows on the device for rows that equal one
of ``keys`` on the columns ``cols`` (``rat_pool_find``: three launches through the ring, no host copy of the pool) and returns their
logical positions in age order — ``RetrievalIndex.find`` over the used columns in ``db_t``, ``OnlineScorer.find`` over any id column in
``pool_ids``.  ``OnlineScorer.set_labels(indices, labels)`` rewrites labels in place (``rat_pool_set_labels``): a label is in no IDF
table, so nothing else moves, and captured request graphs read the new labels at their next replay.  ``relabel_where(cols, keys,
label)`` chains the two on the stream without reading anything back — the list a find leaves is padded with ``-1``, which the label
kernel skips — for the click that arrives after its impression; ``delete_where(cols, keys)`` (``window=True`` only) is ``find`` then
``delete``, for the item that is taken down.  All of them serve the immutable, the ``capacity=`` and the ``window=True`` form (the
deletion the last only), and afterwards the object answers exactly like a fresh one over the live rows with those labels.

Requests can share a launch.  ``score_requests(requests)`` concatenates R independent requests to B rows and sends them through ONE
chain of launches, each request answered exactly as if it had been sent alone: the only step of the chain in which a row looks at
another row is the mapping's dtype rule, and ``rat_bm25_query_prepare_seg`` takes it from the first row of the row's OWN request
(``first_row`` [B], derived from the request offsets; the scan, the merge and the assembly work query by query already).  With
``graph=True`` the batch is padded to the next power of two — the pad rows are a trailing request of their own, copies of the batch's
first row, whose outputs are dropped — so 13 captured graphs serve every request mix of every total up to 4096 rows; ids and
``first_row`` live in static buffers refreshed before each replay.  ``score()`` and its graphs are untouched.

The pool can look at itself.  A live row sent through ``score()`` finds ITSELF as its best neighbour, label attached, and every row
that arrived after it besides.  ``score_rows(indices)`` / ``batch_rows(indices)`` / ``evaluate_rows(indices)`` take logical positions
instead of ids: ``rat_pool_gather_rows`` copies the rows' ids and labels out of the row store and leaves every row's own position as
its HORIZON, and ``rat_bm25_topk_split_before`` scans with that horizon per query — row i is scored against the rows older than it
only, the way the reference's <X>-fold retrieval keeps a self-pool honest (``RetrievalIndex.retrieve(ids, before=...)`` is that scan
for any ids and horizons).  A ``-1`` padding resolves to the newest row the query may see, ``max(i - 1, 0)``.  The IDF weights are
those of the whole live pool as it stands, not of the pool as it was when the row arrived.  ``batch_rows`` carries the rows' real
labels as ``y_true``, so it feeds ``model.train_step`` as well as the eval forward.  Nothing is read back in between, and with
``graph=True`` the chain gather -> prepare -> scan -> assemble -> forward of a size is captured like a request's, in a dictionary of
its own.

Neighbours can be restricted to rows equal on given columns.  ``retrieve(ids, same=cols)``, ``batch / score(ids, same=cols)`` and
``batch_rows / score_rows / evaluate_rows(indices, same=cols)`` take a row's candidates only from the live rows that EQUAL it on the
columns ``cols`` (used columns of the index; at least one used column must remain to score) — the reference's
``exact_match_col_indices``, "this user's history", offered per call so that one resident pool serves both kinds of request.  No group
is numbered: ``db_t`` holds every used column, and the scan compares ids.  The chain is ``rat_bm25_exact_count`` (candidates per
query, through the pool form and below the horizon) -> ``rat_bm25_exact_plan`` (the first query with a candidate, whose row decides the
mapping's dtype rule, and whether the call LISTS: no query has more than K candidates) -> ``rat_bm25_query_prepare_seg`` ->
``rat_bm25_topk_split_exact`` (an exact column gates a row instead of adding a weight, a candidate scores BM25 + 1; a listing call
returns the candidates in ascending index with value 1.0), nothing read back in between, and the result equals
``retrieval.BM25_topk_retrieval_v4(live[:, U], ids[:, U], exact_match_col_indices=E, qry_batch_size=None)`` bit for bit.  With
``graph=True`` the chains of ``score(ids, same=)`` and ``score_rows(indices, same=)`` are captured in dictionaries of their own, keyed
by the columns as well; the ``same=None`` paths and their graphs are untouched.

A request can end on the device.  A CTR request is one user with a slate of candidates, and the caller wants the best n of them:
``top_requests(requests, n)`` runs ``score_requests``' chain unchanged, then ``rat_topn_seg`` — per request the positions and values
of its n largest predictions in the order ``np.argsort(-y_request, kind="stable")[:n]`` (equal predictions in input order, a NaN
last), values bit for bit, 1 <= n <= 64 — then one gather of the rows that open the requests, and returns device tensors (pos [R, n],
y [R, n], lens [R]); nothing is read back in between.  ``top_candidates(contexts, candidates, cols, request_offsets, n)`` takes ONE
encoded row per request and, for every candidate, only the columns ``cols`` in which the candidates differ: the contexts go to the
rows that open their requests with one indexed copy, ``rat_candidates_expand`` builds the [C, L] ids on the device
(``expand_candidates`` returns them), and the rest is ``top_requests``' chain — R L + C W ids go up instead of C L, R (8 n + 4) bytes
come down instead of 4 C.  With ``graph=True`` the padding rule is ``score_requests``' and the chains are captured in two dictionaries
of their own (``_top_graphs`` by bucket and n, ``_top_cand_graphs`` by the columns as well); the older calls and their graphs are
untouched.  No ``same=`` / ``before=`` on these calls.

A request can also end with its WHOLE order, for a re-ranker behind the model, rules that walk down the list, deeper pages or rank metrics:
``rank_requests(requests)`` and ``rank_candidates(contexts, candidates, cols, request_offsets)`` take what ``top_requests`` /
``top_candidates`` take, without n, run the same chains with ``rat_rank_seg`` in ``rat_topn_seg``'s place, and return
``Ranking(order, val, rank, offsets, y_pred)``: ``order[o_r:o_{r+1}]`` is ``np.argsort(-y_r, kind="stable")``, ``val`` those predictions
bit for bit, ``rank`` every row's place in its request — device tensors of B entries, any request length, nothing read back.  Their
captured chains live in ``_rank_graphs`` / ``_rank_cand_graphs``; n > 64 on ``top_*`` stays refused.

The candidates can be INDICES into an item catalogue that lives on the device.  ``set_catalogue(items, cols)`` stores [M, W] ids — per
item the ids of the columns ``cols`` — as int32 on the device.  ``top_items(contexts, items, request_offsets, n)`` and
``rank_items(contexts, items, request_offsets)`` are ``top_candidates`` / ``rank_candidates`` with ``items`` [C] catalogue indices in
place of the [C, W] tuples: ``rat_catalogue_expand`` builds the rows, and the rest is ``top_requests`` / ``rank_requests`` over device
ids — their chains and their captured graphs, shared with direct callers.  ``top_catalogue(contexts, n, chunk=None, exclude=None)``
scores every one of R users against ALL M items and returns the best n (catalogue indices, predictions, counts): the catalogue is
swept in passes of ``chunk`` items per user — the sweep form of the expansion, ``score_requests`` with offsets built on the device,
``rat_topn_seg``, and ``rat_topn_merge`` into a running page per user — with nothing read back between the passes; ``exclude`` =
(ex_items [E], ex_offsets [R + 1]) names per user the items never to return ("already seen": ``rat_topn_exclude`` before the page,
a lookup in the merge).  The new kernels run eagerly around the chain; no graph class and no graph dictionary is new.  No ``same=`` /
``before=`` on these calls either.

The candidates of a request are ONE context row with a few columns swapped, yet every candidate row scans the whole pool.
``build_postings()`` keeps an inverted index over the pool — per used column the rows sorted by (id, row), built on the device — and
``RetrievalIndex.retrieve_shared(ids, request_offsets, varying)`` uses it for such rows: one scan per REQUEST (its head row, the varying
columns' weights at 0.0, over the indexed rows) gives the request's context list, and ``rat_bm25_topk_postings`` scores, per row, the
posting lists of its ids in the varying columns, that list and the rows appended since the build — the scan's result bit for bit.
``postings=True`` on ``top_candidates`` / ``rank_candidates`` / ``top_items`` / ``rank_items`` (their chain launched eagerly) and on
``top_catalogue`` (its pass through ``_SharedGraph``, bucket graphs of its own in ``_postings_graphs``) retrieves that way; the
default, ``False``, is the code as it was, launch for launch.  Served on the immutable and the ``capacity=`` pool, not on a window.

Not served online (refused at construction): the config keys ``exact_match_cols`` / ``exact_match_col_indices`` (the restriction is
per call, ``same=``; not built: ``same`` with ``request_offsets``, and all used columns exact), label-wise retrieval, topK > 32, more
than 32 retrieval columns, data-parallel models.  Rows are deleted from a
``window=True`` pool only: the append-only form reserves its IDF tables for the rows that can still come, which deletions would undo.
"""
import collections
import logging

import numpy as np
import torch

from . import ops, retrieval
from ._lib import get_lib
from .data import DeviceBatch

MAX_TOPK = 32
MAX_COLS = 32
MAX_TOPN = ops.MAX_TOPN          # candidates returned per request: a page of results

# what rank_requests / rank_candidates return: device tensors over the caller's B rows (y_pred: None unless scores=True)
Ranking = collections.namedtuple("Ranking", "order val rank offsets y_pred")


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


_INT_DTYPES = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def _device_list(t, shape, dtype, device=None, fits=lambda n: True):
    """a DEVICE tensor of integers -> int64, contiguous (on ``device``, when given), checked by shape (1-D, and ``fits(numel)``) and
    dtype only and passed through UNREAD: no synchronisation, the kernels clamp or skip what is out of range.  ``shape`` / ``dtype``:
    what the ValueError says the list must be.  Anything else -> None: the caller validates it on the host"""
    if not (torch.is_tensor(t) and t.is_cuda):
        return None
    if t.ndim != 1 or not fits(t.numel()):
        raise ValueError("%s, got shape %s" % (shape, tuple(t.shape)))
    if t.dtype not in _INT_DTYPES:
        raise ValueError("%s, got dtype %s" % (dtype, t.dtype))
    return t.detach().to(device=device, dtype=torch.int64).contiguous()


def _request_offsets(offsets, B):
    """what ``retrieve(ids, request_offsets)`` takes -> (int64 [R + 1] on the host, None) for host-side offsets, validated — 1-D,
    integer dtype, from 0 to B, strictly ascending, or ValueError — or (None, the device tensor as int64), passed through UNREAD: no
    synchronisation, and the kernel clamps what it derives from it"""
    shape, dtype = "request_offsets must be a 1-D list of R + 1 row offsets", "request_offsets must be integers"
    off_dev = _device_list(offsets, shape, dtype, fits=lambda n: n >= 2)
    if off_dev is not None:
        return None, off_dev
    if torch.is_tensor(offsets):
        offsets = offsets.detach().numpy()
    off = np.asarray(offsets)
    if off.ndim != 1 or off.size < 2:
        raise ValueError("%s, got shape %s" % (shape, tuple(off.shape)))
    if not np.issubdtype(off.dtype, np.integer):
        raise ValueError("%s, got dtype %s" % (dtype, off.dtype))
    off = off.astype(np.int64)
    if off[0] != 0:
        raise ValueError("request_offsets must start at 0, got %d" % off[0])
    if off[-1] != B:
        raise ValueError("request_offsets must end at the number of rows (%d), got %d" % (B, off[-1]))
    steps = np.diff(off)
    if (steps < 0).any():
        raise ValueError("request_offsets must be ascending")
    if (steps == 0).any():
        raise ValueError("empty request (request %d has no rows)" % int(np.nonzero(steps == 0)[0][0]))
    return np.ascontiguousarray(off), None


def _first_rows(off_host, off_dev, B, device, pad_to=None, upload=True):
    """request offsets -> first_row int64 [B]: for every batch row the row that opens its request.  ``pad_to`` > B: rows
    B .. pad_to - 1 are one more request, which starts at row B.  Host offsets: built on the host (``upload=False`` returns that
    numpy array), one upload; device offsets: a search on the device, nothing read back"""
    P = B if pad_to is None else pad_to
    if off_host is not None:
        first = np.repeat(off_host[:-1], np.diff(off_host))
        if P > B:
            first = np.concatenate([first, np.full(P - B, B, dtype=np.int64)])
        return torch.from_numpy(first).to(device, non_blocking=True) if upload else first
    rows = torch.arange(B, dtype=torch.int64, device=device)
    req = (torch.searchsorted(off_dev, rows, right=True) - 1).clamp_(0, off_dev.numel() - 1)
    first = off_dev[req]
    if P > B:
        first = torch.cat([first, torch.full((P - B,), B, dtype=torch.int64, device=device)])
    return first.contiguous()


def _host_rows(rows, row_len):
    """rows [M, L + 1] (numpy / host or device tensor; label last) -> (ids int32 [M, L], ids as int [M, L], labels fp32 [M]) on the host,
    converted the way the constructors convert the pool"""
    if torch.is_tensor(rows):
        rows = rows.detach().cpu().numpy()
    rows = np.asarray(rows)
    if rows.ndim != 2 or len(rows) == 0:
        raise ValueError("rows must be a non-empty [M, L + 1] encoded table (label last), got shape %s" % (tuple(rows.shape),))
    if rows.shape[1] != row_len + 1:
        raise ValueError("rows have %d columns, the pool's rows have %d (%d ids and the label)" % (rows.shape[1], row_len + 1, row_len))
    as_int = rows[:, :-1].astype(int)
    return np.ascontiguousarray(retrieval._as_int32(as_int, "appended")), as_int, np.ascontiguousarray(rows[:, -1].astype(np.float32))


def _key_table(cols, keys, where, what):
    """what ``find`` takes -> (positions inside the store int32 [C], keys int32 [M, C] sorted lexicographically and distinct), on the
    host, or ValueError.  ``where``: column number of the encoded row -> its position inside the store searched"""
    c = np.asarray(cols)
    if c.ndim != 1 or not 1 <= c.size <= MAX_COLS:
        raise ValueError("find takes 1 to %d columns as a 1-D list, got shape %s" % (MAX_COLS, tuple(c.shape)))
    if not np.issubdtype(c.dtype, np.integer):
        raise ValueError("find takes integer column numbers, got dtype %s" % c.dtype)
    c = [int(x) for x in c]
    if len(set(c)) != len(c):
        raise ValueError("find: repeated column in %s" % (c,))
    if any(x not in where for x in c):
        raise ValueError("find: column %s is not %s" % ([x for x in c if x not in where], what))
    if torch.is_tensor(keys):
        keys = keys.detach().cpu().numpy()
    k = np.asarray(keys)
    if k.ndim != 2 or k.shape[0] < 1:
        raise ValueError("find takes keys as a non-empty [M, C] table (one row per key), got shape %s" % (tuple(k.shape),))
    if k.shape[1] != len(c):
        raise ValueError("find: keys are %d wide for %d columns" % (k.shape[1], len(c)))
    if not np.issubdtype(k.dtype, np.integer):
        raise ValueError("find takes integer keys, got dtype %s" % k.dtype)
    k = np.unique(retrieval._as_int32(k, "key"), axis=0)                       # rows in lexicographic (signed) order, each once
    return np.asarray([where[x] for x in c], dtype=np.int32), np.ascontiguousarray(k)


def _row_list(indices, n, what, rows="pool", distinct=True):
    """host-side logical row indices -> int64 [m] in the caller's order, or ValueError: integer dtype, inside [0, n) — the live rows of
    the ``rows`` —, no duplicates (``distinct=False``: left to the caller)"""
    if torch.is_tensor(indices):
        indices = indices.detach().cpu().numpy()
    idx = np.atleast_1d(np.asarray(indices))
    if idx.ndim != 1:
        raise ValueError("%s takes a 1-D list of logical row indices, got shape %s" % (what, tuple(idx.shape)))
    if idx.size == 0:
        return np.zeros(0, dtype=np.int64)
    if not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("%s takes integer row indices, got dtype %s" % (what, idx.dtype))
    if idx.min() < 0 or idx.max() >= n:
        raise ValueError("%s: index outside [0, %d), the live rows of the %s (a negative index does not count from the end)"
                         % (what, n, rows))
    idx = idx.astype(np.int64)
    if distinct and len(np.unique(idx)) != len(idx):
        raise ValueError("%s: duplicate index" % what)
    return np.ascontiguousarray(idx)


def _before_list(before, B, device):
    """what ``retrieve(ids, before=...)`` takes -> int64 [B] on the device.  A host array is validated — 1-D, integer dtype, B entries,
    or ValueError — and uploaded; a device tensor is checked by shape and dtype only and passed through UNREAD (the kernel clamps)"""
    shape, dtype = "before must be a 1-D list of %d horizons (one per row)" % B, "before must be integers"
    on_device = _device_list(before, shape, dtype, device, fits=lambda n: n == B)
    if on_device is not None:
        return on_device
    if torch.is_tensor(before):
        before = before.detach().numpy()
    b = np.asarray(before)
    if b.ndim != 1 or b.size != B:
        raise ValueError("%s, got shape %s" % (shape, tuple(b.shape)))
    if not np.issubdtype(b.dtype, np.integer):
        raise ValueError("%s, got dtype %s" % (dtype, b.dtype))
    return torch.from_numpy(np.ascontiguousarray(b.astype(np.int64))).to(device, non_blocking=True)


def _same_positions(same, col_list):
    """what ``retrieve(ids, same=...)`` takes -> the positions of those columns inside the index's used columns (a tuple, ascending:
    the order in which the caller names the columns means nothing), or ValueError: a non-empty 1-D list of distinct integer column numbers of the encoded row, each a used column,
    and at least one used column left to score"""
    if torch.is_tensor(same):
        same = same.detach().cpu().numpy()
    c = np.asarray(same)
    if c.ndim != 1 or c.size == 0:
        raise ValueError("same takes a non-empty 1-D list of column numbers, got shape %s" % (tuple(c.shape),))
    if not np.issubdtype(c.dtype, np.integer):
        raise ValueError("same takes integer column numbers, got dtype %s" % c.dtype)
    c = [int(x) for x in c]
    if len(set(c)) != len(c):
        raise ValueError("same: repeated column in %s" % (c,))
    if any(x not in col_list for x in c):
        raise ValueError("same: column %s is not a used column of this index (%s)" % ([x for x in c if x not in col_list], col_list))
    if len(c) >= len(col_list):
        raise ValueError("same covers all %d used columns: at least one used column must remain to score" % len(col_list))
    return tuple(sorted(col_list.index(x) for x in c))


def _top_n(n):
    """what ``top_requests`` / ``top_candidates`` take as n -> int, or ValueError: an integer, 1 <= n <= MAX_TOPN"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise ValueError("n must be an integer (how many candidates to return per request), got %r" % (n,))
    if not 1 <= int(n) <= MAX_TOPN:
        raise ValueError("1 <= n <= %d (MAX_TOPN) is required, got n = %d" % (MAX_TOPN, int(n)))
    return int(n)


def _candidate_cols(cols, L):
    """the columns of the encoded row that differ between the candidates of a request -> a tuple of ints in the caller's order, or
    ValueError: a non-empty 1-D list of distinct integer column numbers inside [0, L)"""
    if torch.is_tensor(cols):
        cols = cols.detach().cpu().numpy()
    c = np.asarray(cols)
    if c.ndim != 1 or c.size == 0:
        raise ValueError("cols takes a non-empty 1-D list of column numbers, got shape %s" % (tuple(c.shape),))
    if not np.issubdtype(c.dtype, np.integer):
        raise ValueError("cols takes integer column numbers, got dtype %s" % c.dtype)
    c = tuple(int(x) for x in c)
    if len(set(c)) != len(c):
        raise ValueError("cols: repeated column in %s" % (c,))
    if min(c) < 0 or max(c) >= L:
        raise ValueError("cols: column %s outside [0, %d), the id columns of the encoded row" % ([x for x in c if not 0 <= x < L], L))
    return c


class _Exact(tuple):
    """positions of the ``same`` columns inside the used columns, ascending, validated: what the scorer hands on internally"""


class RetrievalIndex:
    """A retrieval pool resident in HBM: its id columns field-major (what the top-K scan streams) and its per-column IDF tables
    (built once, on the host, by ``retrieval.idf_tables`` — numpy's float64 ``log``, so the weights are bit-identical to the offline
    path's).  ``retrieve(ids)`` is ``BM25_topk_retrieval_v4(pool, ids[:, cols], topK=K)`` of one query batch, device tensors out.

    ``capacity`` (>= len(pool)): the buffers are allocated for that many rows, once, and ``append(rows)`` adds rows in place; the
    index then equals a fresh one over the concatenated pool.  Append-only (no eviction, no deletion).  Memory: ``db_t`` is
    4 F capacity bytes; column f's IDF table is reserved for (its distinct ids now + capacity - len(pool)) entries of 12 bytes — every
    appended row adds at most one distinct id per column.

    ``window=True`` (needs ``capacity``): the buffers are a ring over the most recent rows.  ``append`` evicts the oldest rows when
    they do not fit, ``evict(m)`` drops the m oldest; the index then equals a fresh one over the live rows, oldest first.  Memory:
    ``db_t`` is 4 F capacity bytes as before; a column can hold up to capacity distinct ids at some time, so every column's IDF table
    is reserved in full — 12 F capacity bytes, three times ``db_t`` — and the host keeps 8 F capacity bytes of the live rows' ids.
    ``delete(indices)`` drops arbitrary live rows of a window; the index then equals a fresh one over the survivors, oldest first.
    Its first call allocates a scratch buffer the size of the largest store it moves, kept from then on: 4 F capacity bytes, or
    4 max(F, L) capacity bytes with an ``OnlineScorer``'s row store (L ids per row).  An index that never deletes does not pay for it."""

    def __init__(self, pool_array, col_indices, topK, device, lib=None, exact_match_col_indices=None, splits=0, capacity=None,
                 window=False):
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
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
        self.n_db = len(db)
        self.capacity = None
        self.window = bool(window)
        if self.window and capacity is None:
            raise ValueError("window=True needs capacity= (the number of rows the sliding window holds)")
        self._col_list = cols
        self.cols = up(np.asarray(cols, dtype=np.int32))
        if capacity is not None:
            self._init_growable(db, int(capacity))
            return
        tables = retrieval.idf_tables(db)
        self.db_t = up(retrieval._as_int32(db, "pool").T)                      # [F][N] field-major
        self.table_ids = up(np.concatenate([retrieval._as_int32(v, "pool") for v, _ in tables]))
        self.table_idf = up(np.concatenate([w for _, w in tables]).astype(np.float64))
        self.table_offsets = up(np.concatenate([[0], np.cumsum([len(v) for v, _ in tables])]).astype(np.int64))

    def retrieve(self, ids, request_offsets=None, _first_row=None, before=None, same=None, _exact=None):
        """ids [B, L] (full encoded rows) -> (values fp64 [B, K], indices int64 [B, K] with -1 padding, lens int64 [B]), on the device.
        With ``window=True`` the indices are LOGICAL positions (0 = the oldest live row, len(index) - 1 = the newest): they hold until
        the next eviction (an ``evict``, or an ``append`` into a full window) or ``delete``, which renumber the rows.
        ``request_offsets`` (int64 [R + 1], ascending from 0 to B; host or device): rows [off[r], off[r + 1]) are request r, and the
        result is the row-wise concatenation of ``retrieve(request_r)`` — one chain of launches for all of them.  Host-side offsets
        are validated (ValueError, nothing launched: not 1-D, not integer, not from 0 to B, not ascending, an empty request); device
        offsets are used unread, without a synchronisation.
        ``before`` (integers [B]; host or device): row q's candidates are the logical rows i < before[q] only — clamped to
        [0, len(index)] on the device, so 0 or a negative value retrieves nothing and a value past the end sees the whole pool — and
        the result equals, bit for bit, a retrieval of the same weights over a copy of the rows [0, before[q])
        (``rat_bm25_topk_split_before``).  The weights are those of the WHOLE live pool.  A host array is validated (ValueError,
        nothing launched: not 1-D, not integer, not B entries); a device tensor is used unread.  Not combined with
        ``request_offsets`` (ValueError).
        ``same`` (a non-empty 1-D list of distinct column numbers of the encoded row, as ``find`` takes them; each a used column, and
        at least one used column left over): row q's candidates are only the live rows (below ``before[q]``, when given) that EQUAL
        it on those columns, scored over the remaining used columns — the reference's ``exact_match_col_indices``.  The result equals,
        bit for bit, ``retrieval.BM25_topk_retrieval_v4(live[:, U], ids[:, U], exact_match_col_indices=E, qry_batch_size=None,
        topK=K)`` (U the used columns, E the positions of ``same`` in U), the offline path's batch-wide rules included: with no more
        than K candidates for any row of the call every list is the candidates in ascending index with value 1.0; otherwise a
        candidate scores BM25 + 1 and the dtype rule of the weights looks at the first row that has a candidate.  Nothing is read
        back (``rat_bm25_exact_count`` -> ``rat_bm25_exact_plan`` -> ``rat_bm25_query_prepare_seg`` -> ``rat_bm25_topk_split_exact``).
        A bad ``same`` is a ValueError with nothing launched; so is ``same`` with ``request_offsets``."""
        exact = _exact                                 # (an OnlineScorer passes the positions it has validated already)
        if same is not None:
            if request_offsets is not None or _first_row is not None:
                raise ValueError("same cannot be combined with request_offsets: groups inside request segments are not supported")
            exact = _same_positions(same, self._col_list)
        if before is not None and (request_offsets is not None or _first_row is not None):
            raise ValueError("before cannot be combined with request_offsets: horizons inside request segments are not supported")
        ids = _as_device_ids(ids, self.device)
        if ids.shape[1] != self.row_len:
            raise ValueError("ids have %d columns, the pool's rows have %d" % (ids.shape[1], self.row_len))
        if ids.shape[0] == 0:
            raise ValueError("empty request")
        if request_offsets is not None:
            _first_row = _first_rows(*_request_offsets(request_offsets, ids.shape[0]), ids.shape[0], self.device)
        if before is not None:
            before = _before_list(before, ids.shape[0], self.device)
        if exact is not None:
            return self._retrieve_same(ids, before, sum(1 << f for f in exact))
        qry_ids, qry_idf = ops.bm25_query_prepare(ids, self.cols, self.table_ids, self.table_idf, self.table_offsets,
                                                  first_row=_first_row, lib=self._lib)
        return ops.bm25_topk_split(self.db_t, qry_ids, qry_idf, self.topK, splits=self.splits, before=before, lib=self._lib,
                                   **self._pool_form())

    def _retrieve_same(self, ids, before, mask):
        """count -> plan -> prepare -> gated scan, chained on the stream: the counts, the first candidate-bearing row and the listing
        flag stay on the device"""
        form = self._pool_form()
        counts = ops.bm25_exact_count(self.db_t, ids, self.cols, mask, before=before, groups=self.splits, lib=self._lib, **form)
        first_row, listing = ops.bm25_exact_plan(counts, self.topK, lib=self._lib)
        qry_ids, qry_idf = ops.bm25_query_prepare(ids, self.cols, self.table_ids, self.table_idf, self.table_offsets,
                                                  first_row=first_row, lib=self._lib)
        return ops.bm25_topk_split_exact(self.db_t, qry_ids, qry_idf, mask, listing, self.topK, before=before, splits=self.splits,
                                         lib=self._lib, **form)

    def __len__(self):
        return self.n_db

    # ---- requests that share a context: posting lists -----------------------------------------------------------------------
    _post = None                       # build_postings: (post_ids int32 [F, capacity], post_rows int32 [F, capacity], n_sorted int64 [1])
    _n_sorted_host = None

    @property
    def postings_rows(self):
        """the number of rows the posting lists cover (the pool's size at the last ``build_postings``), None before a build; rows
        appended since are the TAIL, which ``retrieve_shared`` scores one by one until the next build"""
        return self._n_sorted_host

    def build_postings(self):
        """The inverted index ``retrieve_shared`` reads: per used column the live rows sorted stably by (id, row) — the ids in
        ``post_ids``, the rows in ``post_rows`` — and their number in device memory.  Built on the device (one stable sort over
        ``db_t``'s live part), ordered with the requests on the current stream.  The buffers are allocated once, at the pool's capacity
        (8 F capacity bytes); a later call sorts into the same buffers and rewrites the count, so captured graphs stay valid.
        ValueError for a ``window=True`` pool: evictions and deletions renumber the rows the lists would hold."""
        if self.window:
            raise ValueError("build_postings: a window=True pool is not served (evictions and deletions renumber the rows the posting "
                             "lists hold)")
        if self._post is None:
            self._post = (torch.zeros_like(self.db_t), torch.zeros_like(self.db_t), torch.zeros(1, dtype=torch.int64, device=self.device))
            self._keep = {}            # vary mask -> bool [F], False at the varying columns
        post_ids, post_rows, n_sorted = self._post
        n = self.n_db
        ids, order = torch.sort(self.db_t[:, :n], dim=1, stable=True)          # equal ids keep ascending rows
        post_ids[:, :n].copy_(ids)
        post_rows[:, :n].copy_(order)
        n_sorted.fill_(n)
        self._n_sorted_host = n

    def _varying_mask(self, varying, what="retrieve_shared"):
        """column numbers of the encoded row -> bit f set = used column f is among them (a column the index does not use cannot
        change a retrieval and is dropped), or ValueError: no posting lists, or not a non-empty 1-D list of distinct columns in [0, L)"""
        if self.window:
            raise ValueError("%s: a window=True pool has no posting lists (its rows are renumbered by evictions and deletions)" % what)
        if self._post is None:
            raise ValueError("%s: no posting lists are built (build_postings())" % what)
        try:
            cols = _candidate_cols(varying, self.row_len)
        except ValueError as exc:
            raise ValueError("%s: varying: %s" % (what, exc)) from None
        return sum(1 << f for f, c in enumerate(self._col_list) if c in cols)

    def _keep_columns(self, mask):
        """bool [F] on the device: False at the varying columns (one upload per mask, kept: a captured chain reads it)"""
        keep = self._keep.get(mask)
        if keep is None:
            keep = self._keep[mask] = torch.tensor([not (mask >> f) & 1 for f in range(len(self._col_list))]).to(self.device)
        return keep

    def _retrieve_shared(self, ids, first_row, heads, mask):
        """prepare over all rows -> the head rows' queries with the varying weights at 0.0 -> the scan over the R of them, below
        n_sorted: the context lists T -> rat_bm25_topk_postings.  first_row int64 [B] and heads int64 [R] (ascending, the rows that
        open the requests) on the device; nothing is read back"""
        post_ids, post_rows, n_sorted = self._post
        form = self._pool_form()
        qry_ids, qry_idf = ops.bm25_query_prepare(ids, self.cols, self.table_ids, self.table_idf, self.table_offsets, first_row=first_row,
                                                  lib=self._lib)
        head_ids = qry_ids.index_select(0, heads)
        head_idf = torch.where(self._keep_columns(mask), qry_idf.index_select(0, heads), 0.0)
        _values, ctx, _lens = ops.bm25_topk_split(self.db_t, head_ids, head_idf, self.topK, splits=self.splits,
                                                  before=n_sorted.expand(heads.numel()).contiguous(), lib=self._lib, **form)
        ctx_row = torch.searchsorted(heads, first_row)
        return ops.bm25_topk_postings(self.db_t, post_ids, post_rows, n_sorted, qry_ids, qry_idf, mask, ctx, ctx_row,
                                      header=form.get("header"), n_rows=form.get("n_rows"), lib=self._lib)

    def retrieve_shared(self, ids, request_offsets, varying, same=None, before=None):
        """``retrieve(ids, request_offsets)`` — the same values, indices and lens, bit for bit — for requests whose rows SHARE A
        CONTEXT: inside a request the rows differ only in the columns ``varying`` (column numbers of the encoded row, as ``cols`` of
        ``OnlineScorer.top_candidates``; entries that are not used columns do not affect a retrieval and are dropped).  Instead of one
        scan of the pool per row: one scan per REQUEST — its head row with the varying columns' weights at 0.0, over the rows the
        posting lists cover —, then per row the posting lists of its ids in the varying columns, the request's list and the rows
        appended since ``build_postings`` (``rat_bm25_topk_postings``).  Needs ``build_postings()``.
        PRECONDITION: the rows of a request are equal on every used column outside ``varying``.  Host ids with host offsets are
        validated (ValueError, nothing launched); device ids are used unread, and rows that break the precondition then get the
        neighbours of a request that kept it — a wrong answer, never a wrong address.
        ``same`` / ``before`` are not offered here (ValueError), nor is a ``window=True`` pool."""
        if same is not None or before is not None:
            raise ValueError("retrieve_shared: same= and before= are not offered for requests that share a context")
        mask = self._varying_mask(varying)
        on_host = not (torch.is_tensor(ids) and ids.is_cuda)
        host = None
        if on_host:
            host = ids.detach().numpy() if torch.is_tensor(ids) else np.asarray(ids)
            if host.ndim != 2:
                raise ValueError("ids must be [B, L] encoded rows, got shape %s" % (tuple(host.shape),))
            B, L = host.shape
        else:
            if ids.ndim != 2:
                raise ValueError("ids must be [B, L] encoded rows, got shape %s" % (tuple(ids.shape),))
            B, L = ids.shape
        if L != self.row_len:
            raise ValueError("ids have %d columns, the pool's rows have %d" % (L, self.row_len))
        if B == 0:
            raise ValueError("empty request")
        off_host, off_dev = _request_offsets(request_offsets, B)
        if host is not None and off_host is not None:
            fixed = [c for f, c in enumerate(self._col_list) if not (mask >> f) & 1]
            first = np.repeat(off_host[:-1], np.diff(off_host))
            differ = (host[:, fixed] != host[first][:, fixed]).any(axis=1)
            if differ.any():
                b = int(np.nonzero(differ)[0][0])
                raise ValueError("retrieve_shared: row %d differs from the row that opens its request (row %d) in a used column outside "
                                 "varying: the rows of a request must share their context" % (b, int(first[b])))
        ids = _as_device_ids(ids, self.device)
        first_row = _first_rows(off_host, off_dev, B, self.device)
        if off_host is not None:
            heads = torch.from_numpy(np.ascontiguousarray(off_host[:-1])).to(self.device, non_blocking=True)
        else:
            heads = off_dev[:-1].clamp(0, B - 1).contiguous()
        return self._retrieve_shared(ids, first_row, heads, mask)

    # ---- the growable form -------------------------------------------------------------------------------------------
    def _init_growable(self, db, capacity):
        if capacity < len(db):
            raise ValueError("capacity = %d is smaller than the pool (%d rows)" % (capacity, len(db)))
        dev, n, F = self.device, len(db), db.shape[1]
        self.capacity = capacity
        self.db_t = torch.zeros((F, capacity), dtype=torch.int32, device=dev)
        self.db_t[:, :n] = torch.from_numpy(np.ascontiguousarray(retrieval._as_int32(db, "pool").T)).to(dev)
        # the header the kernels read the row count from; a window's has a second word, the slot of the oldest live row
        self.count = torch.tensor([n, 0] if self.window else [n], dtype=torch.int64, device=dev)
        # host mirror of the tables' integer half: per column (sorted distinct ids, counts); the weights are derived from it
        self._counts = [np.unique(db[:, c], return_counts=True) for c in range(F)]
        table_cap = sum(len(v) for v, _ in self._counts) + F * (capacity - n)
        if self.window:                                                        # any column may hold `capacity` distinct ids some day
            table_cap = F * capacity
            self._ring = np.zeros((capacity, F), dtype=db.dtype)               # used columns of the live rows, slot-major: who leaves
            self._ring[:n] = db
            self._head = 0
            self._scratch = None                                               # rat_pool_delete's staging buffer, from the first delete on
        self.table_ids = torch.zeros(table_cap, dtype=torch.int32, device=dev)
        self.table_idf = torch.zeros(table_cap, dtype=torch.float64, device=dev)
        self.table_offsets = torch.zeros(F + 1, dtype=torch.int64, device=dev)
        self._upload_tables()

    def _upload_tables(self):
        """retrieval.idf_tables' arithmetic (numpy's float64 log of n / counts) over the mirrored counts -> the SAME device buffers,
        packed front to back (rat_bm25_query_prepare reads the extents from table_offsets on the device)"""
        ids = np.concatenate([retrieval._as_int32(v, "pool") for v, _ in self._counts])
        idf = np.concatenate([np.log(self.n_db / c) for _, c in self._counts]).astype(np.float64)
        off = np.concatenate([[0], np.cumsum([len(v) for v, _ in self._counts])]).astype(np.int64)
        assert len(ids) <= self.table_ids.numel()
        self.table_ids[:len(ids)].copy_(torch.from_numpy(ids))
        self.table_idf[:len(idf)].copy_(torch.from_numpy(idf))
        self.table_offsets.copy_(torch.from_numpy(off))

    def append(self, rows, _pool_ids=None, _pool_labels=None):
        """rows [M, L + 1] (label last; numpy, host or device tensor) become pool rows n .. n + M - 1: retrievable by the next request,
        and every IDF weight moves (N and the counts).  Ordered with the requests on the current stream.  ValueError — and nothing
        written — for an index without ``capacity``, rows that do not fit, a wrong column count or an id outside int32.
        With ``window=True`` rows always fit: the len(index) + M - capacity oldest rows leave in the same call (only M > capacity is
        refused), and every logical index moves down by that many."""
        if self.capacity is None:
            raise ValueError("this index was built without capacity: its pool is immutable (pass capacity= to append rows)")
        ids32, as_int, labels = _host_rows(rows, self.row_len)
        M = len(ids32)
        if self.window:
            return self._push(ids32, as_int, labels, _pool_ids, _pool_labels)
        if self.n_db + M > self.capacity:
            raise ValueError("appending %d rows to %d exceeds the capacity of %d rows" % (M, self.n_db, self.capacity))
        self._count_in(as_int[:, self._col_list])
        self.n_db += M
        dev = self.device
        ops.pool_append(torch.from_numpy(ids32).to(dev), torch.from_numpy(labels).to(dev), self.cols, self.db_t, self.count,
                        _pool_ids, _pool_labels, lib=self._lib)
        self._upload_tables()

    def _count_in(self, used):
        """used [M, F] (the used columns of rows coming in) -> the mirrored (distinct ids, counts): np.unique over the M rows only"""
        for f in range(used.shape[1]):
            vals, counts = self._counts[f]
            u, uc = np.unique(used[:, f], return_counts=True)
            pos = np.searchsorted(vals, u)
            hit = vals[np.minimum(pos, len(vals) - 1)] == u if len(vals) else np.zeros(len(u), dtype=bool)
            counts = counts.copy()
            counts[pos[hit]] += uc[hit]
            self._counts[f] = (np.insert(vals, pos[~hit], u[~hit]), np.insert(counts, pos[~hit], uc[~hit]))

    # ---- the sliding form ----------------------------------------------------------------------------------------------
    def _slots(self, first, m):
        """physical slots of the logical rows first .. first + m - 1"""
        return (self._head + first + np.arange(m)) % self.capacity

    def _count_out(self, m):
        """the m oldest rows leave the mirrored counts and the host ring"""
        self._count_gone(self._ring[self._slots(0, m)])
        self._head = (self._head + m) % self.capacity
        self.n_db -= m

    def _count_gone(self, gone):
        """gone [m, F] (the used columns of rows going out) leave the mirrored counts; an id nobody holds any more leaves its column's
        table, as a fresh index over the remaining rows would not hold it (a request whose first row carries it then MISSES: the
        dtype rule of rat_bm25_query_prepare depends on that)"""
        for f in range(gone.shape[1]):
            vals, counts = self._counts[f]
            u, uc = np.unique(gone[:, f], return_counts=True)
            counts = counts.copy()
            counts[np.searchsorted(vals, u)] -= uc
            keep = counts > 0
            self._counts[f] = (vals[keep], counts[keep])

    def _push(self, ids32, as_int, labels, pool_ids, pool_labels):
        M = len(ids32)
        if M > self.capacity:
            raise ValueError("appending %d rows exceeds the capacity of the window (%d rows)" % (M, self.capacity))
        E = max(0, self.n_db + M - self.capacity)
        if E:
            self._count_out(E)
        used = as_int[:, self._col_list]
        self._count_in(used)
        self._ring[self._slots(self.n_db, M)] = used
        self.n_db += M
        dev = self.device
        ops.pool_push(torch.from_numpy(ids32).to(dev), torch.from_numpy(labels).to(dev), self.cols, self.db_t, self.count,
                      pool_ids, pool_labels, lib=self._lib)
        self._upload_tables()

    def evict(self, m):
        """The m oldest rows leave the window (``window=True`` only): every IDF weight moves (N and the counts), ids nobody holds any
        more leave the tables, and every logical index moves down by m.  Ordered with the requests on the current stream.
        ValueError — and nothing written — for m < 0 or m >= len(index): the pool never becomes empty."""
        if not self.window:
            raise ValueError("this index was built without window=True: rows cannot be evicted")
        m = int(m)
        if m < 0 or m >= self.n_db:
            raise ValueError("evict(%d) on a window of %d rows: 0 <= m < len(index) is required (the pool never becomes empty)"
                             % (m, self.n_db))
        if m == 0:
            return
        self._count_out(m)
        ops.pool_evict(self.count, m, self.capacity, lib=self._lib)
        self._upload_tables()

    def _delete_list(self, indices):
        """what ``delete`` accepts -> sorted int64 [m] on the host, or ValueError"""
        idx = np.sort(_row_list(indices, self.n_db, "delete", rows="window", distinct=False))
        if (np.diff(idx) == 0).any():
            raise ValueError("delete: duplicate index %d" % idx[1:][np.diff(idx) == 0][0])
        if len(idx) >= self.n_db:
            raise ValueError("delete of all %d rows would leave the pool empty (the window never becomes empty)" % self.n_db)
        return idx

    def delete(self, indices, _pool_ids=None, _pool_labels=None):
        """The live rows at the logical positions ``indices`` (as ``retrieve`` returns them: an int array-like, a host or a device
        tensor, in any order) leave the window (``window=True`` only).  The survivors keep their age order: every survivor's index
        drops by the number of deleted rows older than it, every IDF weight moves (N and the counts) and ids nobody holds any more
        leave the tables.  Ordered with the requests on the current stream; an empty list does nothing.  ValueError — and nothing
        written — for a duplicate, an index outside [0, len(index)) (negative ones included), a non-integer dtype, a list that would
        leave the pool empty."""
        if not self.window:
            raise ValueError("this index was built without window=True: rows cannot be deleted")
        idx = self._delete_list(indices)
        m, n = len(idx), self.n_db
        if m == 0:
            return
        # what can fail comes first — the allocation, the upload of the list, the launches: the host state changes after them
        words = self.capacity * max(len(self._col_list), self.row_len if _pool_ids is not None else 0)
        if self._scratch is None or self._scratch.numel() < words:                 # outside every captured graph: no request reads it
            self._scratch = torch.empty(words, dtype=torch.int32, device=self.device)
        ops.pool_delete(self.db_t, self.count, torch.from_numpy(idx).to(self.device), self._scratch, _pool_ids, _pool_labels,
                        lib=self._lib)
        self._count_gone(self._ring[(self._head + idx) % self.capacity])
        suffix = np.arange(idx[0], n)                                          # rows older than the first deleted one stay where they are
        keep = np.ones(len(suffix), dtype=bool)
        keep[idx - idx[0]] = False
        self._ring[self._slots(idx[0], n - m - idx[0])] = self._ring[(self._head + suffix[keep]) % self.capacity]
        self.n_db -= m
        self._upload_tables()


    # ---- addressed by key -----------------------------------------------------------------------------------------------
    def _pool_form(self):
        """where the ops wrappers (the scan, the assembly, pool_find, ...) take the live rows from: the three forms of the pool"""
        if self.capacity is None:
            return dict(n_rows=self.n_db)
        return dict(header=self.count, ring=self.window)

    def _find(self, store, field_major, positions, keys):
        dev = self.device
        out_idx, out_count = ops.pool_find(store, torch.from_numpy(positions).to(dev), torch.from_numpy(keys).to(dev), field_major,
                                           max_out=self.n_db, lib=self._lib, **self._pool_form())
        return out_idx[:int(out_count.item())].clone()                         # the one read-back: the number of matches

    def find(self, cols, keys):
        """The logical positions (0 = the oldest live row, as ``retrieve`` returns them), ascending, of the live rows that equal one of
        ``keys`` on the columns ``cols``: an int64 device tensor of exactly the matches.  ``cols``: column numbers of the encoded row,
        as ``col_indices`` — among the index's used columns, the only ones it stores; ``keys``: [M, C] integers, M >= 1, C = len(cols)
        <= 32, in any order, repeats allowed.  The search runs on the device (``rat_pool_find``) in every form of the index; sizing the
        result costs one small device-to-host read of the match count, so this call SYNCHRONISES with the stream.  ValueError for a
        column that is not a used column, a repeated column, C or M out of range, a wrong key width, a non-integer dtype, a key
        outside int32."""
        positions, table = _key_table(cols, keys, {c: f for f, c in enumerate(self._col_list)},
                                      "a used column of this index (%s)" % (self._col_list,))
        return self._find(self.db_t, True, positions, table)

    def delete_where(self, cols, keys):
        """``find(cols, keys)`` then ``delete`` of what it found (``window=True`` only) -> the number of rows removed.  No match
        returns 0 and changes nothing; a match set that would empty the pool is refused by ``delete``, with nothing written."""
        if not self.window:
            raise ValueError("this index was built without window=True: rows cannot be deleted")
        found = self.find(cols, keys)
        if found.numel():
            self.delete(found)
        return int(found.numel())


class _ChainGraph:
    """one chain of launches ending in the eval forward as one linear hipGraph (one stream, no parallel branches): the inputs are
    cloned into static buffers and ``chain(*static)`` is captured under no_grad; what the chain reads besides — the pool's header, the
    labels, the weights — is read at replay time"""

    def __init__(self, chain, *inputs):
        self.static = tuple(t.clone() for t in inputs)
        self._stream = torch.cuda.Stream(device=inputs[0].device)
        self.graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.no_grad(), torch.cuda.graph(self.graph, stream=self._stream, capture_error_mode="thread_local"):
            self.y_pred = chain(*self.static)

    def run(self, x):
        if x.data_ptr() != self.static[0].data_ptr():
            self.static[0].copy_(x, non_blocking=True)
        self.graph.replay()
        return self.y_pred.clone()


class _RequestGraph(_ChainGraph):
    """retrieve -> assemble -> eval forward of one request size; the ids are the static input"""

    def __init__(self, scorer, ids, same=None):
        super().__init__(lambda static_ids: scorer._score_eager(static_ids, same=same), ids)


class _RowsGraph(_ChainGraph):
    """gather -> prepare -> horizon scan -> assemble -> eval forward of one number of pool rows; the logical indices are the static
    input"""

    def __init__(self, scorer, indices, same=None):
        super().__init__(lambda static_idx: scorer._score_rows_eager(static_idx, same=same), indices)


class _BucketGraph(_ChainGraph):
    """the request chain for P rows (a power of two) that hold ANY mix of requests: ids and first_row are static inputs, refreshed
    before each replay"""

    def __init__(self, scorer, ids, first_row):
        super().__init__(scorer._score_eager, ids, first_row)
        self._first_host = None        # the host array the static first_row was last uploaded from

    def run(self, ids, first_row):
        """first_row: a device tensor, or the host array it is built from — uploaded straight into the static buffer, and not at all
        when it equals the last one (the same request sizes again: a batcher with fixed slots, one request of B rows).  Returns the
        static y_pred, uncloned"""
        static_ids, static_first = self.static
        static_ids.copy_(ids, non_blocking=True)
        if torch.is_tensor(first_row):
            self._first_host = None
            static_first.copy_(first_row, non_blocking=True)
        elif self._first_host is None or not np.array_equal(first_row, self._first_host):
            self._first_host = first_row                                       # (kept: the upload reads it)
            static_first.copy_(torch.from_numpy(first_row), non_blocking=True)
        self.graph.replay()
        return self.y_pred


class _SharedGraph(_BucketGraph):
    """``_BucketGraph`` over the chain of requests that share a context (``RetrievalIndex._retrieve_shared`` instead of the scan per
    row), for one mask of varying columns: ids, first_row and the rows that open the requests are the static inputs, all refreshed
    from device tensors before each replay"""

    def __init__(self, scorer, mask, ids, first_row, heads):
        _ChainGraph.__init__(self, lambda i, f, h: scorer._score_eager(i, f, shared=(mask, h)), ids, first_row, heads)

    def run(self, ids, first_row, heads):
        for static, t in zip(self.static, (ids, first_row, heads)):
            static.copy_(t, non_blocking=True)
        self.graph.replay()
        return self.y_pred


class _HeadRows:
    """the rows that open the requests, as the ranked calls gather them: a device tensor is passed through, a host array is uploaded
    only when it differs from the last one (the same request sizes again)"""
    _heads_host = _heads_dev = None

    def heads(self, heads, device):
        if torch.is_tensor(heads):
            return heads
        if self._heads_host is None or not np.array_equal(heads, self._heads_host):
            self._heads_host, self._heads_dev = heads, torch.from_numpy(heads).to(device, non_blocking=True)
        return self._heads_dev


class _TopGraph(_BucketGraph, _HeadRows):
    """the request chain for P rows followed by rat_topn_seg, for one n: ids and first_row are the static inputs; ``run`` returns the
    static (pos [P, n], val [P, n], lens [P], y_pred [P]), uncloned"""

    def __init__(self, scorer, n, ids, first_row):
        _ChainGraph.__init__(self, lambda static_ids, static_first: scorer._top_eager(static_ids, static_first, n), ids, first_row)
        self._first_host = None


class _TopCandGraph(_ChainGraph, _HeadRows):
    """rat_candidates_expand -> the request chain -> rat_topn_seg for P candidate rows, one n and one tuple of candidate columns: the
    context slab, the candidates' columns and first_row are the static inputs.  The slab is refreshed at the head rows only (no other
    row of it is read); first_row as in ``_BucketGraph.run``"""

    def __init__(self, scorer, n, cols_dev, slab, cand, first_row):
        super().__init__(lambda s, c, f: scorer._top_cand_eager(s, c, cols_dev, f, n), slab, cand, first_row)
        self._cols = cols_dev          # (the captured launches read it)
        self._first_host = None

    def run(self, contexts, heads, cand, first_row):
        """heads: the rows the contexts go to (the pad request's included), device tensor or host array"""
        static_slab, static_cand, static_first = self.static
        static_slab.index_copy_(0, self.heads(heads, static_slab.device), contexts)
        static_cand.copy_(cand, non_blocking=True)
        if torch.is_tensor(first_row):
            self._first_host = None
            static_first.copy_(first_row, non_blocking=True)
        elif self._first_host is None or not np.array_equal(first_row, self._first_host):
            self._first_host = first_row
            static_first.copy_(torch.from_numpy(first_row), non_blocking=True)
        self.graph.replay()
        return self.y_pred


class _RankGraph(_BucketGraph):
    """the request chain for P rows followed by rat_rank_seg: ids and first_row are the static inputs; ``run`` returns the static
    (order [P], val [P], rank [P], y_pred [P]), uncloned"""

    def __init__(self, scorer, ids, first_row):
        _ChainGraph.__init__(self, scorer._rank_eager, ids, first_row)
        self._first_host = None


class _RankCandGraph(_TopCandGraph):
    """rat_candidates_expand -> the request chain -> rat_rank_seg for P candidate rows and one tuple of candidate columns; inputs and
    ``run`` are ``_TopCandGraph``'s"""

    def __init__(self, scorer, cols_dev, slab, cand, first_row):
        _ChainGraph.__init__(self, lambda s, c, f: scorer._rank_cand_eager(s, c, cols_dev, f), slab, cand, first_row)
        self._cols = cols_dev
        self._first_host = None


class OnlineScorer:
    """``score(ids)``: fp32 [B] predictions of a trained model for fresh encoded rows ``ids`` [B, L], the neighbours retrieved from
    ``pool_array`` ([N, L + 1], label last) on the spot.  ``retrieval_configs`` is the dataset's block (``topK``, ``used_cols`` or
    ``used_col_indices``, ...).  ``graph=True``: after ``graph_warmup`` eager requests of a batch size (<= ``graph_max_batch``) the
    chain is captured and replayed; the weights are read at replay time, so the graph survives optimizer steps and load_state_dict.
    ``capacity``: room for that many pool rows; ``append(rows)`` then adds labelled rows in place and the captured graphs stay valid
    (they read the row count from device memory).  Append-only, unless ``window=True``: the pool is then a sliding window over the most
    recent ``capacity`` rows — ``append`` evicts the oldest rows when the new ones do not fit, ``evict(m)`` drops the m oldest,
    ``delete(indices)`` drops arbitrary rows, and the captured graphs stay valid through all three."""

    graph_warmup = 2
    graph_max_batch = 4096
    graph_sizes = 16               # at most this many request sizes get a graph; others stay eager

    def __init__(self, model, pool_array, retrieval_configs, graph=True, lib=None, capacity=None, window=False):
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
        self.index = RetrievalIndex(pool_array, cols, cfg["topK"], self.device, lib=self._lib, capacity=capacity, window=window)
        pool_array = np.asarray(pool_array)
        self.pool_ids = torch.from_numpy(np.ascontiguousarray(pool_array[:, :-1].astype(np.int32))).to(self.device)
        self.pool_labels = torch.from_numpy(np.ascontiguousarray(pool_array[:, -1].astype(np.float32))).to(self.device)
        if self.index.capacity is not None:                                    # the row store at full size, the pool in front
            n, cap = len(pool_array), self.index.capacity
            ids, labels = self.pool_ids, self.pool_labels
            self.pool_ids = torch.zeros((cap, ids.shape[1]), dtype=torch.int32, device=self.device)
            self.pool_labels = torch.zeros(cap, dtype=torch.float32, device=self.device)
            self.pool_ids[:n] = ids
            self.pool_labels[:n] = labels
        self.graph = bool(graph)
        self._consts = {}              # request size -> (rows = arange(B), labels = zeros(B))
        self._graphs = {}              # key -> [eager requests seen, _RequestGraph | False | None]
        self._bucket_graphs = {}       # score_requests: (bucket, ...) -> [eager calls seen, _BucketGraph | False | None]
        self._rows_graphs = {}         # score_rows: key -> [eager calls seen, _RowsGraph | False | None]
        self._same_graphs = {}         # score(ids, same=): key + (the columns as ascending positions,) -> [eager requests seen, _RequestGraph | False | None]
        self._same_rows_graphs = {}    # score_rows(indices, same=): the same for _RowsGraph
        self._top_graphs = {}          # top_requests: (bucket, n, ...) -> [eager calls seen, _TopGraph | False | None]
        self._top_cand_graphs = {}     # top_candidates: (bucket, n, ..., the candidate columns) -> [eager calls seen, _TopCandGraph | False | None]
        self._rank_graphs = {}         # rank_requests: (bucket, ...) -> [eager calls seen, _RankGraph | False | None]
        self._rank_cand_graphs = {}    # rank_candidates: (bucket, ..., the candidate columns) -> [eager calls seen, _RankCandGraph | False | None]
        self._cols_dev = {}            # top_candidates / rank_candidates: the candidate columns as a tuple -> the same as an int32 device tensor
        self._found = None             # relabel_where's index list (one entry per row the pool can hold), from its first call on
        self._catalogue = None         # set_catalogue: (items int32 [M, W] on the device, the columns as an int32 device tensor)
        self._catalogue_cols = None    # ... and the columns as a tuple
        self._postings_graphs = {}     # top_catalogue(postings=True): (bucket, ..., the columns, requests) -> [eager passes seen, _SharedGraph | False | None]

    # ------------------------------------------------------------------------------------------------------------------
    def _constants(self, B):
        c = self._consts.get(B)
        if c is None:
            c = self._consts[B] = (torch.arange(B, dtype=torch.int64, device=self.device),
                                   torch.zeros(B, dtype=torch.float32, device=self.device))
        return c

    def _assemble_batch(self, ids, labels, neighbours):
        """the rows (ids, labels) are the query table, ``neighbours`` their lists: logical positions in the row store, where -1 keeps its
        numpy meaning, as offline — counted back from the pool's last LIVE row (a ring's newest)"""
        form = self.index._pool_form()
        form.pop("n_rows", None)                                               # the immutable row store holds the live rows and no others
        rows, _zeros = self._constants(ids.shape[0])
        return ops.batch_assemble(ids, labels, self.pool_ids, self.pool_labels, neighbours, rows, lib=self._lib, **form)

    def _assemble(self, ids, first_row=None, same=None, shared=None):
        """``shared`` = (mask of varying used columns, heads int64 [R] on the device): the requests share a context, and the neighbours
        come through the posting lists (``RetrievalIndex._retrieve_shared``) — the same lists, bit for bit"""
        _rows, labels = self._constants(ids.shape[0])
        if shared is not None:
            _values, indices, _lens = self.index._retrieve_shared(ids, first_row, shared[1], shared[0])
        else:
            _values, indices, _lens = self.index.retrieve(ids, _first_row=first_row, _exact=same)
        return self._assemble_batch(ids, labels, indices)                      # the neighbour lists: the scan's own index output

    def _score_eager(self, ids, first_row=None, same=None, shared=None):
        y_pred, _loss, _reg, _saved = self.model._run_forward(self._assemble(ids, first_row, same, shared), save=False, with_reg=False)
        return y_pred.reshape(-1)

    def build_postings(self):
        """``RetrievalIndex.build_postings``: the posting lists that ``postings=True`` retrieves through (``top_candidates``,
        ``rank_candidates``, ``top_items``, ``rank_items``, ``top_catalogue``).  Rows appended afterwards are served as the lists'
        tail; a second call covers them.  Captured graphs stay valid.  ValueError for a ``window=True`` pool."""
        self.index.build_postings()

    def _shared_mask(self, cols, postings, what):
        """``postings`` as a call takes it -> None (False: today's chain), or the mask of the used columns among ``cols`` — ValueError
        before any entry point without ``build_postings()`` or on a window pool"""
        if not postings:
            return None
        return self.index._varying_mask(cols, "%s(postings=True)" % what)

    def append(self, rows):
        """``RetrievalIndex.append`` plus the row store (ids and labels of the new rows, the same launch).  Afterwards the scorer equals
        ``OnlineScorer(model, np.concatenate([pool, rows]), cfg)``; captured request graphs are kept and serve the grown pool.
        With ``window=True``: over the last ``capacity`` rows of that concatenation."""
        self.index.append(rows, self.pool_ids, self.pool_labels)

    def evict(self, m):
        """``RetrievalIndex.evict``: the m oldest pool rows leave (``window=True`` only).  Afterwards the scorer equals a fresh one over
        the remaining rows; captured request graphs are kept."""
        self.index.evict(m)

    def delete(self, indices):
        """``RetrievalIndex.delete`` plus the row store (the same call moves the survivors' ids and labels): the rows at the logical
        positions ``indices`` leave (``window=True`` only).  Afterwards the scorer equals a fresh one over the remaining rows in age
        order; captured request graphs are kept."""
        self.index.delete(indices, self.pool_ids, self.pool_labels)

    def find(self, cols, keys):
        """``RetrievalIndex.find`` over the row store: the logical positions, ascending, of the live rows that equal one of ``keys``
        ([M, C]) on ``cols`` — ANY of the L id columns of the encoded row, not only the retrieval columns.  An int64 device tensor of
        exactly the matches; reading their number back SYNCHRONISES with the stream.  Same refusals."""
        L = self.index.row_len
        positions, table = _key_table(cols, keys, {c: c for c in range(L)}, "one of the %d id columns of the pool" % L)
        return self.index._find(self.pool_ids, False, positions, table)

    def _labels(self, labels, m):
        """a scalar, or one label per index -> fp32 device tensor [1] or [m], converted as the constructor converts the pool's"""
        if not torch.is_tensor(labels):
            labels = torch.from_numpy(np.asarray(labels).astype(np.float32))       # (a 0-d array stays 0-d)
        lab = labels.detach().to(self.device, torch.float32)
        if lab.ndim == 0:
            return lab.reshape(1)
        if lab.ndim != 1 or lab.numel() != m:
            raise ValueError("labels must be a scalar or one label per index ([%d]), got shape %s" % (m, tuple(lab.shape)))
        return lab.contiguous()

    def _index_list(self, indices, what):
        """logical row indices -> int64 [m] on the device.  Host-side ones (a list, numpy, a host tensor) are validated (ValueError: a
        non-integer dtype, an index outside [0, len(pool)), a duplicate, not 1-D); a DEVICE tensor is checked by shape and dtype and
        passed through unread"""
        idx = _device_list(indices, "%s takes a 1-D list of logical row indices" % what, "%s takes integer row indices" % what, self.device)
        return idx if idx is not None else torch.from_numpy(_row_list(indices, len(self.index), what)).to(self.device)

    def set_labels(self, indices, labels):
        """The live rows at the logical positions ``indices`` get ``labels`` (a scalar for all, or [m], one per index) in place, in
        every form of the pool (``rat_pool_set_labels``).  A label is in no IDF table: nothing else moves, no captured request graph is
        touched, and the next request — eager or replayed — reads the new labels.  Ordered with the requests on the current stream.
        Host-side indices (a list, numpy, a host tensor) are validated — ValueError, and nothing written, for a non-integer dtype, an
        index outside [0, len(pool)) or a duplicate.  A DEVICE tensor is passed through unread, without a synchronisation: entries < 0
        or >= len(pool) are skipped by the kernel (so the ``-1``-padded list of a find can be passed whole), and duplicates are the
        caller's business."""
        idx = self._index_list(indices, "set_labels")
        lab = self._labels(labels, idx.numel())
        if idx.numel():
            ops.pool_set_labels(self.pool_labels, idx, lab, lib=self._lib, **self.index._pool_form())

    def relabel_where(self, cols, keys, label):
        """Every live row that equals one of ``keys`` on ``cols`` (as ``find`` takes them) gets ``label`` (a scalar): the find and the
        label kernel are chained on the current stream, with no read-back and no synchronisation of its own — the impression whose
        click arrived.  Returns the number of rows relabelled as an int64 DEVICE tensor [1].  The list in between holds one entry per
        row the pool can hold (8 bytes each, allocated on the first call and kept), so no match set is ever truncated."""
        L = self.index.row_len
        positions, table = _key_table(cols, keys, {c: c for c in range(L)}, "one of the %d id columns of the pool" % L)
        if np.ndim(label) != 0:
            raise ValueError("relabel_where takes one label for all matching rows, got shape %s" % (np.shape(label),))
        lab = self._labels(label, 1)
        dev, form = self.device, self.index._pool_form()
        if self._found is None:                                                # outside every captured graph: no request reads it
            self._found = torch.empty(self.pool_labels.numel(), dtype=torch.int64, device=dev)
        _, count = ops.pool_find(self.pool_ids, torch.from_numpy(positions).to(dev), torch.from_numpy(table).to(dev), False,
                                 out_idx=self._found, lib=self._lib, **form)
        ops.pool_set_labels(self.pool_labels, self._found, lab, lib=self._lib, **form)
        return count

    def delete_where(self, cols, keys):
        """``find(cols, keys)`` then ``delete`` of what it found (``window=True`` only) -> the number of rows removed: the item that is
        taken down, the user who opts out.  No match returns 0 and changes nothing; a match set that would empty the pool is refused
        by ``delete``, with nothing written."""
        if not self.index.window:
            raise ValueError("this scorer's pool was built without window=True: rows cannot be deleted")
        found = self.find(cols, keys)
        if found.numel():
            self.delete(found)
        return int(found.numel())

    def _same_key(self, same):
        """``same`` as the caller gave it -> its positions inside the used columns, ascending (validated here, once, as
        ``RetrievalIndex.retrieve`` validates it: ValueError before anything is launched), or None.  The internal calls below pass
        that tuple on; it is also what the ``same=`` graphs are keyed by, so the order the caller names the columns in costs no
        second graph."""
        if same is None or isinstance(same, _Exact):
            return same
        return _Exact(_same_positions(same, self.index._col_list))

    def batch(self, ids, same=None):
        """-> data.DeviceBatch (idx [B, 1 + K, L], label_ids [B, 1 + K], y_true = zeros): what the model's forward consumes.
        ``same``: the neighbours of a row are taken only from pool rows equal to it on those columns (``RetrievalIndex.retrieve``)."""
        return DeviceBatch(*self._assemble(_as_device_ids(ids, self.device), same=self._same_key(same)))

    def score(self, ids, same=None):
        """fp32 [B] predictions for the encoded rows ``ids``.  ``same`` (column numbers of the encoded row, among the used columns):
        every row's neighbours come only from pool rows that equal it on those columns — this user's history instead of anyone's
        traffic, from the same resident pool.  With ``graph=True`` the chain of a (size, ``same``) pair is captured after
        ``graph_warmup`` eager calls, in a dictionary of its own; the ``same=None`` graphs are not touched."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.score needs the model in eval mode (model.eval())")
        same = self._same_key(same)
        ids = _as_device_ids(ids, self.device)
        with torch.no_grad():
            g = self._graph_for(ids, same)
            return g.run(ids) if g is not None else self._score_eager(ids, same=same)

    # ---- the pool looks at itself ------------------------------------------------------------------------------------------
    def _row_indices(self, indices, what):
        """``_index_list`` that refuses an empty list; the gather answers a device index outside the live rows with a row of zeros"""
        idx = self._index_list(indices, what)
        if idx.numel() == 0:
            raise ValueError("%s: empty list of rows" % what)
        return idx

    def _assemble_rows(self, idx, same=None):
        """idx int64 [B] (device) -> (idx, label_ids, y_true) of the rows at those logical positions, each with the neighbours it had
        when it arrived: horizon = its own position.  Nothing is read back between the launches."""
        form = self.index._pool_form()
        ids, labels, before = ops.pool_gather_rows(self.pool_ids, self.pool_labels, idx, lib=self._lib, **form)
        _values, nbr, _lens = self.index.retrieve(ids, before=before, _exact=same)
        # a -1 padding is the newest row the query may see, not the pool's newest row (which the assembly would take for it)
        return self._assemble_batch(ids, labels, torch.where(nbr < 0, (before - 1).clamp_(min=0).unsqueeze(1), nbr))

    def _score_rows_eager(self, idx, same=None):
        y_pred, _loss, _reg, _saved = self.model._run_forward(self._assemble_rows(idx, same), save=False, with_reg=False)
        return y_pred.reshape(-1)

    def batch_rows(self, indices, same=None):
        """-> data.DeviceBatch of the live rows at the logical positions ``indices``: ``idx[:, 0]`` their ids, ``y_true`` their REAL
        labels (the batch can go straight into ``model.train_step``), and as neighbours of row i only rows OLDER than i — the scan
        runs with the row's own position as its horizon, so the row never retrieves itself or anything that arrived after it.  A
        ``-1`` padding resolves to row ``max(i - 1, 0)``, the newest row i may see (row 0, which has nobody before it, pads with
        itself).  The IDF weights are those of the whole live pool as it stands.  ``same``: only OLDER rows equal to row i on those columns
        (the same user's earlier rows) are its candidates, as ``RetrievalIndex.retrieve(ids, before=, same=)`` defines them."""
        same = self._same_key(same)
        return DeviceBatch(*self._assemble_rows(self._row_indices(indices, "batch_rows"), same))

    def score_rows(self, indices, same=None):
        """fp32 [B] predictions for the live rows at ``indices``, each scored against the rows older than it (``batch_rows``).  With
        ``graph=True`` and device indices, the chain of a size (<= ``graph_max_batch``) is captured after ``graph_warmup`` eager calls
        and replayed with the indices as its static input; it reads the header, the labels and the weights at replay time."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.score_rows needs the model in eval mode (model.eval())")
        same = self._same_key(same)
        given_on_device = torch.is_tensor(indices) and indices.is_cuda
        idx = self._row_indices(indices, "score_rows")
        with torch.no_grad():
            g = self._rows_graph_for(idx, same) if given_on_device else None   # (``same``: as ``batch_rows``; graphs of its own)
            return g.run(idx) if g is not None else self._score_rows_eager(idx, same)

    def _group_column(self, group):
        """``group``: None, or the index of one id column of the pool's rows -> that index, checked"""
        if group is None:
            return None
        L = int(self.pool_ids.shape[1])
        if isinstance(group, bool) or not isinstance(group, (int, np.integer)):
            raise ValueError("group takes the index of one id column of the rows, got %r" % (group,))
        if not 0 <= int(group) < L:
            raise ValueError("group=%d is not an id column of the rows (they hold %d)" % (int(group), L))
        return int(group)

    def _rows_vectors(self, indices, same, group, what):
        """-> (y_pred fp32 [B], labels fp32 [B], group ids int32 [B] or None) of the live rows at ``indices``, on the device"""
        same = self._same_key(same)
        col = self._group_column(group)
        idx = self._row_indices(indices, what)
        y_pred = self.score_rows(idx, same=same)
        ids, labels, _before = ops.pool_gather_rows(self.pool_ids, self.pool_labels, idx, lib=self._lib, **self.index._pool_form())
        return y_pred, labels, (None if col is None else ids[:, col].contiguous())

    @staticmethod
    def _cutoff_list(cutoffs, group, what):
        """``cutoffs``: an iterable of positive integers (at most 8 for the raw tensor) -> a list; they need ``group``"""
        ks = [k for k in cutoffs]
        for k in ks:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
                raise ValueError("%s: a cutoff is a positive integer, got %r" % (what, k))
        if ks and group is None:
            raise ValueError("%s: cutoffs rank the rows inside groups; name the id column with group=" % what)
        return [int(k) for k in ks]

    def evaluate_rows(self, indices, same=None, group=None, device=False, cutoffs=()):
        """{"logloss": ..., "AUC": ...} of ``score_rows(indices)`` against the rows' stored labels: how well the model does on the
        traffic in the window.  ``group=col`` (the index of one id column of the rows, e.g. the user's) adds "GAUC": the per-group AUC
        weighted by the groups' rows; every K in ``cutoffs`` (they need ``group``) adds "NDCG(k=K)", "MRR(k=K)" and "HitRate(k=K)", the
        ranking metrics per group (rat_amd/metrics.py).  By default ``metrics.evaluate_metrics`` runs on the host after one
        device-to-host copy of the vectors; ``device=True`` runs the metric chains on the device (``metrics.device_metrics``) and copies
        64 bytes, plus 64 per cutoff."""
        from .metrics import device_metrics, evaluate_metrics
        ks = self._cutoff_list(cutoffs, group, "evaluate_rows")
        y_pred, labels, gids = self._rows_vectors(indices, same, group, "evaluate_rows")
        names = ["logloss", "AUC"] + (["GAUC"] if gids is not None else [])
        names += ["%s(k=%d)" % (kind, k) for k in ks for kind in ("NDCG", "MRR", "HitRate")]
        if device:
            return device_metrics(labels, y_pred, names, group_index=gids, lib=self._lib)
        both = torch.stack([y_pred, labels]).cpu().numpy()
        return evaluate_metrics(both[1].astype(np.float64), both[0].astype(np.float64), names,
                                group_index=None if gids is None else gids.cpu().numpy())

    def metrics_rows(self, indices, same=None, group=None):
        """the raw float64 [8] device tensor of ``ops.eval_metrics`` over ``score_rows(indices)`` and the rows' stored labels (logloss, AUC,
        GAUC — NaN without ``group`` —, n_pos, n_neg, groups counted, their rows, status bits): nothing is read back, a monitor can collect many of them and copy once"""
        y_pred, labels, gids = self._rows_vectors(indices, same, group, "metrics_rows")
        return ops.eval_metrics(y_pred.contiguous(), labels, gids, lib=self._lib)

    def rank_metrics_rows(self, indices, cutoffs, same=None, group=None):
        """the raw float64 [m, 8] device tensor of ``ops.eval_rank_metrics`` over ``score_rows(indices)`` and the rows' stored labels inside
        the groups of id column ``group`` — per cutoff NDCG, MRR, HitRate, groups counted, groups seen, hits, k, status bits: nothing is
        read back"""
        ks = self._cutoff_list(cutoffs, group, "rank_metrics_rows")
        if group is None:
            raise ValueError("rank_metrics_rows: name the id column that groups the rows with group=")
        y_pred, labels, gids = self._rows_vectors(indices, same, group, "rank_metrics_rows")
        return ops.eval_rank_metrics(y_pred.contiguous(), labels, gids, ks, lib=self._lib)

    def _graph_for(self, ids, same=None):
        """the captured chain of ``score(ids)``, or None: launch eagerly.  ``same``: a dictionary of its own, the key extended by the
        columns"""
        B = ids.shape[0]
        if not (self.graph and ids.is_cuda and B <= self.graph_max_batch):
            return None
        key = (B, self.model._eval_graph_key((B, self.index.topK + 1, ids.shape[1])))
        if same is None:
            return self._captured(self._graphs, key, lambda: _RequestGraph(self, ids), "the online request", self.graph_sizes)
        return self._captured(self._same_graphs, key + (same,), lambda: _RequestGraph(self, ids, same), "the online request with same=",
                              self.graph_sizes)

    def _rows_graph_for(self, idx, same=None):
        """``_graph_for`` for ``score_rows(indices)``"""
        B = idx.numel()
        if not (self.graph and idx.is_cuda and B <= self.graph_max_batch):
            return None
        key = (B, self.model._eval_graph_key((B, self.index.topK + 1, self.index.row_len)))
        if same is None:
            return self._captured(self._rows_graphs, key, lambda: _RowsGraph(self, idx), "the pool-row scoring", self.graph_sizes)
        return self._captured(self._same_rows_graphs, key + (same,), lambda: _RowsGraph(self, idx, same),
                              "the pool-row scoring with same=", self.graph_sizes)

    def _captured(self, graphs, key, capture, what, limit=None):
        """the entry ``key`` of one of the graph dictionaries (at most ``limit`` entries; None: any number): counts the eager calls up
        to ``graph_warmup``, then captures once -> the graph, or None while the caller is to launch eagerly — during the warm-up, past
        the limit, and for good after a capture that failed"""
        entry = graphs.get(key)
        if entry is None:
            if limit is not None and len(graphs) >= limit:
                return None
            entry = graphs[key] = [0, None]
        if entry[1] is None:
            entry[0] += 1
            if entry[0] <= self.graph_warmup:
                return None
            try:
                entry[1] = capture()
            except Exception as exc:
                logging.warning("hipGraph capture of %s failed (%s: %s); continuing with eager launches", what, type(exc).__name__, exc)
                entry[1] = False
        return entry[1] or None

    # ---- requests that share a launch ------------------------------------------------------------------------------------
    def _requests(self, requests):
        """a list of [B_r, L] id arrays, or a pair (ids [B, L], request_offsets) -> (ids int32 [B, L] on the device, host offsets
        int64 [R + 1] | None, device offsets | None), or ValueError"""
        if isinstance(requests, tuple) and len(requests) == 2:                 # a TUPLE of two is the pair, a list holds requests
            ids = _as_device_ids(requests[0], self.device)
            off_host, off_dev = _request_offsets(requests[1], ids.shape[0])
        else:
            if len(requests) == 0:
                raise ValueError("empty request list")
            parts = [r if torch.is_tensor(r) else torch.from_numpy(np.ascontiguousarray(np.asarray(r))) for r in requests]
            for k, r in enumerate(parts):
                if r.ndim != 2:
                    raise ValueError("request %d must be [B_r, L] encoded rows, got shape %s" % (k, tuple(r.shape)))
                if r.shape[1] != self.index.row_len:
                    raise ValueError("request %d has %d columns, the pool's rows have %d" % (k, r.shape[1], self.index.row_len))
                if r.shape[0] == 0:
                    raise ValueError("empty request (request %d has no rows)" % k)
            if any(r.is_cuda for r in parts) or len({r.dtype for r in parts}) > 1:
                parts = [_as_device_ids(r, self.device) for r in parts]
            ids = _as_device_ids(torch.cat(parts), self.device)                # host arrays of one dtype: one upload for all of them
            off_host, off_dev = np.concatenate([[0], np.cumsum([r.shape[0] for r in parts])]).astype(np.int64), None
        if ids.shape[1] != self.index.row_len:
            raise ValueError("ids have %d columns, the pool's rows have %d" % (ids.shape[1], self.index.row_len))
        if ids.shape[0] == 0:
            raise ValueError("empty request")
        return ids, off_host, off_dev

    def batch_requests(self, requests):
        """``batch()`` for requests that share a launch (as ``score_requests`` takes them) -> data.DeviceBatch over all B rows, equal
        to the concatenation of the per-request ``batch(request_r)``"""
        ids, off_host, off_dev = self._requests(requests)
        return DeviceBatch(*self._assemble(ids, _first_rows(off_host, off_dev, ids.shape[0], self.device)))

    def score_requests(self, requests):
        """R independent requests in one chain of launches, each answered as if it had been sent alone to ``score``.  ``requests``: a
        LIST of [B_r, L] id arrays, or a pair — a TUPLE (ids [B, L], request_offsets int64 [R + 1] ascending from 0 to B, host or device).
        Returns (y_pred fp32 [B] in input order, request_offsets int64 [R + 1] — a host tensor, or the device tensor that was passed):
        request r's predictions are ``y_pred[off[r]:off[r + 1]]``.  With ``graph=True`` the batch is padded to the next power of two
        (<= ``graph_max_batch``) with a trailing request of copies of its first row, whose outputs are dropped; after ``graph_warmup``
        eager calls of a bucket its chain is captured and serves every request mix of that bucket."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.score_requests needs the model in eval mode (model.eval())")
        ids, off_host, off_dev = self._requests(requests)
        B = ids.shape[0]
        offsets = torch.from_numpy(off_host) if off_host is not None else off_dev
        with torch.no_grad():
            P = 1 << (B - 1).bit_length()
            if not (self.graph and ids.is_cuda and P <= self.graph_max_batch):
                return self._score_eager(ids, _first_rows(off_host, off_dev, B, self.device)), offsets
            first_row = _first_rows(off_host, off_dev, B, self.device, pad_to=P, upload=False)
            if P > B:                                                          # the pad rows: valid ids, a request of their own
                ids = torch.cat([ids, ids[:1].expand(P - B, -1)])
            g = self._bucket_graph_for(ids, first_row)
            if g is not None:
                return g.run(ids, first_row)[:B].clone(), offsets
            return self._score_eager(ids, self._on_device(first_row))[:B].clone(), offsets

    def _on_device(self, first_row):
        return first_row if torch.is_tensor(first_row) else torch.from_numpy(first_row).to(self.device, non_blocking=True)

    def _bucket_graph_for(self, ids, first_row):
        P = ids.shape[0]
        key = (P, self.model._eval_graph_key((P, self.index.topK + 1, ids.shape[1])))
        return self._captured(self._bucket_graphs, key, lambda: _BucketGraph(self, ids, self._on_device(first_row)),
                              "the batched online requests")

    # ---- each request's best candidates ----------------------------------------------------------------------------------------
    def _top_eager(self, ids, first_row, n, shared=None):
        """the request chain, then rat_topn_seg over its predictions -> (pos [B, n], val [B, n], lens [B], y_pred [B]); rows that open
        no request hold padding"""
        y_pred = self._score_eager(ids, first_row, shared=shared).contiguous()
        return ops.topn_seg(y_pred, first_row, n, lib=self._lib) + (y_pred,)

    def _top_cand_eager(self, slab, cand, cols_dev, first_row, n, shared=None):
        return self._top_eager(ops.candidates_expand(slab, cand, cols_dev, first_row, lib=self._lib), first_row, n, shared)

    def _heads(self, off_host, off_dev, B, pad, upload=True):
        """the rows that open the requests, int64 [R] on the device (``pad``: and row B, which opens the pad request).  Device offsets
        are used unread: clamped, so that the gather stays inside whatever they hold.  Host offsets with ``upload=False``: the host
        array"""
        if off_host is not None:
            heads = np.ascontiguousarray(off_host[:-1] if not pad else np.concatenate([off_host[:-1], [B]]))
            return torch.from_numpy(heads).to(self.device, non_blocking=True) if upload else heads
        heads = off_dev[:-1].clamp(0, B - 1)
        return torch.cat([heads, torch.full((1,), B, dtype=torch.int64, device=self.device)]) if pad else heads

    @staticmethod
    def _top_result(out, heads, B, scores):
        pos, val, lens, y_pred = out
        picked = (pos[heads], val[heads], lens[heads])                         # one gather each: new tensors, not the graph's buffers
        return picked + (y_pred[:B].clone(),) if scores else picked

    def top_requests(self, requests, n, scores=False):
        """The best ``n`` rows of every request: ``requests`` as ``score_requests`` takes them (a LIST of [B_r, L] id arrays, or a
        TUPLE (ids [B, L], request_offsets [R + 1], host or device)) -> device tensors (pos int32 [R, n], y fp32 [R, n], lens int32
        [R]): ``pos[r, :lens[r]]`` are the positions INSIDE request r of its ``lens[r] = min(n, B_r)`` largest predictions, best
        first — ``np.argsort(-y_r, kind="stable")[:n]``: equal predictions in input order — ``y[r]`` those predictions, the rest
        ``-1`` / ``0.0``.  ``n`` larger than a request is no error.  ``scores=True``: additionally the full y_pred fp32 [B] that was
        ranked.  The launches are ``score_requests``' chain, then ``rat_topn_seg``, then one gather of the rows that open the requests
        — nothing is read back (device offsets are used unread).  1 <= n <= MAX_TOPN.  With ``graph=True`` the padding rule of
        ``score_requests`` holds, and the chain of a (bucket, n) pair is captured after ``graph_warmup`` eager calls into
        ``_top_graphs`` (at most ``graph_sizes`` pairs; others stay eager)."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.top_requests needs the model in eval mode (model.eval())")
        n = _top_n(n)
        ids, off_host, off_dev = self._requests(requests)
        B = ids.shape[0]
        with torch.no_grad():
            P = 1 << (B - 1).bit_length()
            if not (self.graph and ids.is_cuda and P <= self.graph_max_batch):
                out = self._top_eager(ids, _first_rows(off_host, off_dev, B, self.device), n)
                return self._top_result(out, self._heads(off_host, off_dev, B, False), B, scores)
            first_row = _first_rows(off_host, off_dev, B, self.device, pad_to=P, upload=False)
            if P > B:                                                          # the pad rows: valid ids, a request of their own
                ids = torch.cat([ids, ids[:1].expand(P - B, -1)])
            key = (P, n, self.model._eval_graph_key((P, self.index.topK + 1, ids.shape[1])))
            g = self._captured(self._top_graphs, key, lambda: _TopGraph(self, n, ids, self._on_device(first_row)),
                               "the ranked online requests", self.graph_sizes)
            if g is not None:
                return self._top_result(g.run(ids, first_row), g.heads(self._heads(off_host, off_dev, B, False, upload=False), self.device), B, scores)
            return self._top_result(self._top_eager(ids, self._on_device(first_row), n), self._heads(off_host, off_dev, B, False), B, scores)

    def _candidates(self, contexts, candidates, cols, request_offsets):
        """what ``top_candidates`` takes -> (contexts int32 [R, L], candidates int32 [C, W], the columns as a tuple and as an int32
        device tensor, host offsets | None, device offsets | None), or ValueError with nothing launched"""
        L = self.index.row_len
        cols = _candidate_cols(cols, L)
        shapes = []                                                            # everything that can be refused, before the first upload
        for t, what in ((contexts, "contexts must be [R, L] encoded rows"), (candidates, "candidates must be [C, W] ids")):
            shapes.append(tuple(t.shape) if hasattr(t, "shape") else np.shape(t))
            if len(shapes[-1]) != 2:
                raise ValueError("%s, got shape %s" % (what, shapes[-1]))
        (R_given, L_given), (C, W) = shapes
        if L_given != L:
            raise ValueError("contexts have %d columns, the pool's rows have %d" % (L_given, L))
        if W != len(cols):
            raise ValueError("candidates have %d columns for the %d columns in cols" % (W, len(cols)))
        if C == 0:
            raise ValueError("empty request")
        off_host, off_dev = _request_offsets(request_offsets, C)
        R = (len(off_host) if off_host is not None else off_dev.numel()) - 1
        if R_given != R:
            raise ValueError("contexts hold %d rows for %d requests (one encoded row per request)" % (R_given, R))
        contexts, candidates = _as_device_ids(contexts, self.device), _as_device_ids(candidates, self.device)
        return contexts, candidates, cols, self._cols_tensor(cols), off_host, off_dev

    def _cols_tensor(self, cols):
        cols_dev = self._cols_dev.get(cols)
        if cols_dev is None:                                                   # one upload per tuple of columns
            cols_dev = self._cols_dev[cols] = torch.tensor(cols, dtype=torch.int32).to(self.device)
        return cols_dev

    def _slab(self, contexts, heads, rows):
        """[rows, L] with the contexts at the rows that open their requests: one indexed copy; no other row is ever read"""
        return torch.empty((rows, contexts.shape[1]), dtype=torch.int32, device=self.device).index_copy_(0, heads, contexts)

    def expand_candidates(self, contexts, candidates, cols, request_offsets):
        """-> ids int32 [C, L] on the device: the full encoded row of every candidate — the columns ``cols`` from ``candidates``
        [C, W], every other column from the context row of the candidate's request (``contexts`` [R, L]; request r owns the candidates
        ``request_offsets[r] .. request_offsets[r + 1] - 1``).  What ``top_candidates`` scores; built by ``rat_candidates_expand``."""
        contexts, candidates, _cols, cols_dev, off_host, off_dev = self._candidates(contexts, candidates, cols, request_offsets)
        C = candidates.shape[0]
        slab = self._slab(contexts, self._heads(off_host, off_dev, C, False), C)
        return ops.candidates_expand(slab, candidates, cols_dev, _first_rows(off_host, off_dev, C, self.device), lib=self._lib)

    def top_candidates(self, contexts, candidates, cols, request_offsets, n, scores=False, postings=False):
        """``top_requests`` for requests given as ONE context row each plus the columns in which their candidates differ:
        ``contexts`` [R, L] encoded rows (their ``cols`` entries are ignored), ``candidates`` [C, W] the ids of the columns ``cols``
        (W distinct column numbers of the encoded row) of all C candidates, ``request_offsets`` [R + 1] over the candidates (host:
        validated; device: used unread).  The caller uploads R L + C W ids instead of C L: the rows are built on the device
        (``rat_candidates_expand``, after one indexed copy of the contexts to the rows that open their requests), and the rest is
        ``top_requests``' chain.  Returns what ``top_requests`` returns, positions counting the candidates of a request from 0.
        With ``graph=True`` the chain of a (bucket, n, cols) triple is captured into ``_top_cand_graphs``.
        ``postings=True`` (needs ``build_postings()``; not on a window pool): the candidates of a request share its context and differ
        in ``cols``, so the neighbours are retrieved through the posting lists (``RetrievalIndex.retrieve_shared``'s chain with
        ``varying = cols``) — the same result bit for bit, launched eagerly."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.top_candidates needs the model in eval mode (model.eval())")
        n = _top_n(n)
        mask = self._shared_mask(cols, postings, "top_candidates")
        contexts, cand, cols, cols_dev, off_host, off_dev = self._candidates(contexts, candidates, cols, request_offsets)
        C = cand.shape[0]
        with torch.no_grad():
            P = 1 << (C - 1).bit_length()
            if mask is not None:
                heads = self._heads(off_host, off_dev, C, False)
                out = self._top_cand_eager(self._slab(contexts, heads, C), cand, cols_dev, _first_rows(off_host, off_dev, C, self.device), n,
                                           shared=(mask, heads))
                return self._top_result(out, heads, C, scores)
            if not (self.graph and cand.is_cuda and P <= self.graph_max_batch):
                slab = self._slab(contexts, self._heads(off_host, off_dev, C, False), C)
                out = self._top_cand_eager(slab, cand, cols_dev, _first_rows(off_host, off_dev, C, self.device), n)
                return self._top_result(out, self._heads(off_host, off_dev, C, False), C, scores)
            first_row = _first_rows(off_host, off_dev, C, self.device, pad_to=P, upload=False)
            heads = self._heads(off_host, off_dev, C, P > C, upload=False)
            if P > C:                                                          # the pad request: the first request's context, copies of its first candidate
                contexts = torch.cat([contexts, contexts[:1]])
                cand = torch.cat([cand, cand[:1].expand(P - C, -1)])
            key = (P, n, self.model._eval_graph_key((P, self.index.topK + 1, contexts.shape[1])), cols)
            g = self._captured(self._top_cand_graphs, key,
                               lambda: _TopCandGraph(self, n, cols_dev, self._slab(contexts, self._on_device(heads), P), cand,
                                                     self._on_device(first_row)),
                               "the ranked candidate requests", self.graph_sizes)
            if g is not None:
                out, heads = g.run(contexts, heads, cand, first_row), g.heads(heads, self.device)
            else:
                heads = self._on_device(heads)
                out = self._top_cand_eager(self._slab(contexts, heads, P), cand, cols_dev, self._on_device(first_row), n)
            return self._top_result(out, heads[:-1] if P > C else heads, C, scores)

    # ---- each request's full ranking ---------------------------------------------------------------------------------------------
    def _rank_eager(self, ids, first_row, shared=None):
        """the request chain, then rat_rank_seg over its predictions -> (order [B], val [B], rank [B], y_pred [B])"""
        y_pred = self._score_eager(ids, first_row, shared=shared).contiguous()
        return ops.rank_seg(y_pred, first_row, lib=self._lib) + (y_pred,)

    def _rank_cand_eager(self, slab, cand, cols_dev, first_row, shared=None):
        return self._rank_eager(ops.candidates_expand(slab, cand, cols_dev, first_row, lib=self._lib), first_row, shared)

    @staticmethod
    def _rank_result(out, B, offsets, scores):
        order, val, rank = (t[:B].clone() for t in out[:3])                   # new tensors, not the graph's buffers; a pad request lies behind B
        return Ranking(order, val, rank, offsets, out[3][:B].clone() if scores else None)

    def rank_requests(self, requests, scores=False):
        """The whole order of every request: ``requests`` as ``score_requests`` takes them -> ``Ranking(order, val, rank, offsets,
        y_pred)`` of device tensors over the B rows: for request r, ``order[off[r]:off[r + 1]]`` are the positions INSIDE the request,
        best first — ``np.argsort(-y_r, kind="stable")``: equal predictions in input order, a NaN last —, ``val`` those predictions bit
        for bit, ``rank[b]`` row b's place in its request (``order[off[r] + rank[b]] == b - off[r]``); ``offsets`` as
        ``score_requests`` returns them; ``y_pred`` the unsorted fp32 [B] when ``scores=True``, else None.  Any request length.  The
        launches are ``score_requests``' chain, then ``rat_rank_seg`` — nothing is read back (device offsets are used unread).  With
        ``graph=True`` the padding rule of ``score_requests`` holds, and a bucket's chain is captured after ``graph_warmup`` eager
        calls into ``_rank_graphs`` (at most ``graph_sizes`` buckets; others stay eager)."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.rank_requests needs the model in eval mode (model.eval())")
        ids, off_host, off_dev = self._requests(requests)
        B = ids.shape[0]
        offsets = torch.from_numpy(off_host) if off_host is not None else off_dev
        with torch.no_grad():
            P = 1 << (B - 1).bit_length()
            if not (self.graph and ids.is_cuda and P <= self.graph_max_batch):
                return self._rank_result(self._rank_eager(ids, _first_rows(off_host, off_dev, B, self.device)), B, offsets, scores)
            first_row = _first_rows(off_host, off_dev, B, self.device, pad_to=P, upload=False)
            if P > B:                                                          # the pad rows: valid ids, a request of their own
                ids = torch.cat([ids, ids[:1].expand(P - B, -1)])
            key = (P, self.model._eval_graph_key((P, self.index.topK + 1, ids.shape[1])))
            g = self._captured(self._rank_graphs, key, lambda: _RankGraph(self, ids, self._on_device(first_row)),
                               "the fully ranked online requests", self.graph_sizes)
            out = g.run(ids, first_row) if g is not None else self._rank_eager(ids, self._on_device(first_row))
            return self._rank_result(out, B, offsets, scores)

    def rank_candidates(self, contexts, candidates, cols, request_offsets, scores=False, postings=False):
        """``rank_requests`` for requests given as ``top_candidates`` takes them — ONE context row each (``contexts`` [R, L]) plus the
        columns ``cols`` in which their candidates differ (``candidates`` [C, W], ``request_offsets`` [R + 1] over the candidates) —
        without n: ``rat_candidates_expand`` after one indexed copy of the contexts, then ``rank_requests``' chain.  Returns what
        ``rank_requests`` returns, positions counting the candidates of a request from 0.  With ``graph=True`` the chain of a
        (bucket, cols) pair is captured into ``_rank_cand_graphs``.  ``postings=True``: as ``top_candidates`` takes it."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.rank_candidates needs the model in eval mode (model.eval())")
        mask = self._shared_mask(cols, postings, "rank_candidates")
        contexts, cand, cols, cols_dev, off_host, off_dev = self._candidates(contexts, candidates, cols, request_offsets)
        C = cand.shape[0]
        offsets = torch.from_numpy(off_host) if off_host is not None else off_dev
        with torch.no_grad():
            P = 1 << (C - 1).bit_length()
            if mask is not None:
                heads = self._heads(off_host, off_dev, C, False)
                out = self._rank_cand_eager(self._slab(contexts, heads, C), cand, cols_dev, _first_rows(off_host, off_dev, C, self.device),
                                            shared=(mask, heads))
                return self._rank_result(out, C, offsets, scores)
            if not (self.graph and cand.is_cuda and P <= self.graph_max_batch):
                slab = self._slab(contexts, self._heads(off_host, off_dev, C, False), C)
                out = self._rank_cand_eager(slab, cand, cols_dev, _first_rows(off_host, off_dev, C, self.device))
                return self._rank_result(out, C, offsets, scores)
            first_row = _first_rows(off_host, off_dev, C, self.device, pad_to=P, upload=False)
            heads = self._heads(off_host, off_dev, C, P > C, upload=False)
            if P > C:                                                          # the pad request: the first request's context, copies of its first candidate
                contexts = torch.cat([contexts, contexts[:1]])
                cand = torch.cat([cand, cand[:1].expand(P - C, -1)])
            key = (P, self.model._eval_graph_key((P, self.index.topK + 1, contexts.shape[1])), cols)
            g = self._captured(self._rank_cand_graphs, key,
                               lambda: _RankCandGraph(self, cols_dev, self._slab(contexts, self._on_device(heads), P), cand,
                                                      self._on_device(first_row)),
                               "the fully ranked candidate requests", self.graph_sizes)
            if g is not None:
                out = g.run(contexts, heads, cand, first_row)
            else:
                out = self._rank_cand_eager(self._slab(contexts, self._on_device(heads), P), cand, cols_dev, self._on_device(first_row))
            return self._rank_result(out, C, offsets, scores)

    # ---- a resident item catalogue: candidates as indices, and the best n of all of it ---------------------------------------------
    def set_catalogue(self, items, cols):
        """The item catalogue the ``*_items`` / ``top_catalogue`` calls draw candidates from: ``items`` [M, W] integer ids (numpy, host
        or device tensor) — for each of M items the ids of the columns ``cols`` (W distinct column numbers of the encoded row), what a
        row of ``top_candidates``' ``candidates`` holds.  Stored as contiguous int32 on the device; replaces any earlier catalogue.
        Host ids are validated (ValueError before any upload); a device tensor is checked by shape and dtype and converted unread."""
        cols = _candidate_cols(cols, self.index.row_len)
        shape = tuple(items.shape) if hasattr(items, "shape") else np.shape(items)
        if len(shape) != 2:
            raise ValueError("the catalogue must be [M, W] ids (one row per item), got shape %s" % (shape,))
        if shape[0] == 0:
            raise ValueError("empty catalogue")
        if shape[1] != len(cols):
            raise ValueError("the catalogue has %d columns for the %d columns in cols" % (shape[1], len(cols)))
        if torch.is_tensor(items) and items.is_cuda:
            if items.dtype not in _INT_DTYPES:
                raise ValueError("the catalogue must hold integers, got dtype %s" % items.dtype)
            cat = items.detach().to(device=self.device, dtype=torch.int32).contiguous().clone()
        else:
            host = items.detach().numpy() if torch.is_tensor(items) else np.asarray(items)
            if not np.issubdtype(host.dtype, np.integer):
                raise ValueError("the catalogue must hold integers, got dtype %s" % host.dtype)
            cat = torch.from_numpy(np.ascontiguousarray(retrieval._as_int32(host, "catalogue"))).to(self.device)
        self._catalogue = (cat, self._cols_tensor(cols))
        self._catalogue_cols = cols

    @property
    def catalogue_size(self):
        """M, the number of items of the catalogue (0: none set)"""
        return 0 if self._catalogue is None else self._catalogue[0].shape[0]

    def _catalogue_contexts(self, contexts, what):
        """-> (the catalogue, its columns on the device, the [R, L] shape of ``contexts``), or ValueError with nothing launched"""
        if self._catalogue is None:
            raise ValueError("%s: no catalogue is set (set_catalogue(items, cols))" % what)
        shape = tuple(contexts.shape) if hasattr(contexts, "shape") else np.shape(contexts)
        if len(shape) != 2 or shape[0] == 0:
            raise ValueError("contexts must be [R, L] encoded rows, one per request, got shape %s" % (shape,))
        if shape[1] != self.index.row_len:
            raise ValueError("contexts have %d columns, the pool's rows have %d" % (shape[1], self.index.row_len))
        return self._catalogue + (shape[0],)

    def _item_requests(self, contexts, items, request_offsets, what):
        """what ``top_items`` takes -> (ids int32 [C, L] on the device, built by ``rat_catalogue_expand``; the offsets as passed on to the
        request chains), or ValueError with nothing launched"""
        cat, cols_dev, R_given = self._catalogue_contexts(contexts, what)
        M = cat.shape[0]
        shape, dtype = "items must be a 1-D list of catalogue indices", "items must be integers"
        idx = _device_list(items, shape, dtype, self.device)
        if idx is None:                                                        # host side: validated
            host = items.detach().numpy() if torch.is_tensor(items) else np.asarray(items)
            if host.ndim != 1:
                raise ValueError("%s, got shape %s" % (shape, tuple(host.shape)))
            if host.size and not np.issubdtype(host.dtype, np.integer):
                raise ValueError("%s, got dtype %s" % (dtype, host.dtype))
            if host.size and (host.min() < 0 or host.max() >= M):
                raise ValueError("items: index outside [0, %d), the items of the catalogue" % M)
        C = idx.numel() if idx is not None else host.size
        if C == 0:
            raise ValueError("empty request")
        off_host, off_dev = _request_offsets(request_offsets, C)
        R = (len(off_host) if off_host is not None else off_dev.numel()) - 1
        if R_given != R:
            raise ValueError("contexts hold %d rows for %d requests (one encoded row per request)" % (R_given, R))
        if idx is None:
            idx = torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(self.device, non_blocking=True)
        else:                                                                  # device side: unread; clamped here so that no wide index wraps
            idx = idx.clamp(0, M - 1).to(torch.int32)
        contexts = _as_device_ids(contexts, self.device)
        slab = self._slab(contexts, self._heads(off_host, off_dev, C, False), C)
        ids = ops.catalogue_expand(slab, cat, cols_dev, _first_rows(off_host, off_dev, C, self.device), items=idx, lib=self._lib)
        return ids, off_host if off_host is not None else off_dev

    def _shared_items(self, request, mask):
        """what ``_item_requests`` returns -> (ids, first_row, heads, the offsets as a tensor, shared) for the eager chains"""
        ids, off = request
        off_host, off_dev = (None, off) if torch.is_tensor(off) else (off, None)
        C = ids.shape[0]
        heads = self._heads(off_host, off_dev, C, False)
        offsets = torch.from_numpy(off_host) if off_host is not None else off_dev
        return ids, _first_rows(off_host, off_dev, C, self.device), heads, offsets, (mask, heads)

    def top_items(self, contexts, items, request_offsets, n, scores=False, postings=False):
        """``top_candidates`` with the candidates given as INDICES into the catalogue: ``contexts`` [R, L] encoded rows (their entries in
        the catalogue's columns are ignored), ``items`` [C] catalogue indices (host: validated, every entry in [0, M); device: used
        unread, clamped), ``request_offsets`` [R + 1] over them.  C indices go up instead of C W ids.  The rows are built on the device
        (``rat_catalogue_expand``, after one indexed copy of the contexts) and handed to ``top_requests`` as a pair of device ids and
        the offsets, so its chain and its captured graphs are shared with direct callers.  Returns what ``top_candidates`` returns,
        positions counting a request's items from 0.  ``postings=True``: as ``top_candidates`` takes it, the varying columns being the
        catalogue's; the chain is launched eagerly."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.top_items needs the model in eval mode (model.eval())")
        n = _top_n(n)
        mask = self._shared_mask(self._catalogue_cols, postings, "top_items") if self._catalogue is not None else None
        with torch.no_grad():
            request = self._item_requests(contexts, items, request_offsets, "top_items")
            if mask is None:
                return self.top_requests(request, n, scores=scores)
            ids, first_row, heads, _offsets, shared = self._shared_items(request, mask)
            return self._top_result(self._top_eager(ids, first_row, n, shared), heads, ids.shape[0], scores)

    def rank_items(self, contexts, items, request_offsets, scores=False, postings=False):
        """``rank_candidates`` with the candidates given as indices into the catalogue (as ``top_items`` takes them), through
        ``rank_requests``' chain.  Returns what ``rank_candidates`` returns.  ``postings=True``: as ``top_items`` takes it."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.rank_items needs the model in eval mode (model.eval())")
        mask = self._shared_mask(self._catalogue_cols, postings, "rank_items") if self._catalogue is not None else None
        with torch.no_grad():
            request = self._item_requests(contexts, items, request_offsets, "rank_items")
            if mask is None:
                return self.rank_requests(request, scores=scores)
            ids, first_row, _heads, offsets, shared = self._shared_items(request, mask)
            return self._rank_result(self._rank_eager(ids, first_row, shared), ids.shape[0], offsets, scores)

    def _exclusion(self, exclude, R, M):
        """what ``top_catalogue`` takes as ``exclude`` -> (ex_items int32 [E], ex_offsets int64 [R + 1]) on the device.  Host lists are
        validated — integers in [0, M), offsets from 0 to E ascending — and sorted per request; device lists are checked by shape and
        dtype and used unread (they must be sorted per request)"""
        if not isinstance(exclude, (tuple, list)) or len(exclude) != 2:
            raise ValueError("exclude is a pair (ex_items [E], ex_offsets [R + 1])")
        ex_items, ex_offsets = exclude
        dev_items = _device_list(ex_items, "ex_items must be a 1-D list of catalogue indices", "ex_items must be integers", self.device)
        dev_off = _device_list(ex_offsets, "ex_offsets must be a 1-D list of %d offsets (one more than requests)" % (R + 1),
                               "ex_offsets must be integers", self.device, fits=lambda k: k == R + 1)
        if (dev_items is None) != (dev_off is None):
            raise ValueError("exclude: ex_items and ex_offsets sit both on the host or both on the device")
        if dev_items is not None:
            return dev_items.clamp(-1, M).to(torch.int32), dev_off
        items = ex_items.detach().numpy() if torch.is_tensor(ex_items) else np.asarray(ex_items)
        off = ex_offsets.detach().numpy() if torch.is_tensor(ex_offsets) else np.asarray(ex_offsets)
        if items.ndim != 1 or (items.size and not np.issubdtype(items.dtype, np.integer)):
            raise ValueError("ex_items must be a 1-D list of integer catalogue indices, got shape %s, dtype %s" % (tuple(items.shape), items.dtype))
        if off.ndim != 1 or off.size != R + 1 or not np.issubdtype(off.dtype, np.integer):
            raise ValueError("ex_offsets must be a 1-D list of %d integer offsets (one more than requests), got shape %s, dtype %s"
                             % (R + 1, tuple(off.shape), off.dtype))
        off = off.astype(np.int64)
        if off[0] != 0 or off[-1] != items.size or (np.diff(off) < 0).any():
            raise ValueError("ex_offsets must ascend from 0 to the number of excluded items (%d)" % items.size)
        if items.size and (items.min() < 0 or items.max() >= M):
            raise ValueError("exclude: index outside [0, %d), the items of the catalogue" % M)
        items = items.astype(np.int32)
        ordered = np.concatenate([np.sort(items[a:b]) for a, b in zip(off[:-1], off[1:])] + [np.zeros(0, dtype=np.int32)])
        return (torch.from_numpy(np.ascontiguousarray(ordered)).to(self.device, non_blocking=True),
                torch.from_numpy(np.ascontiguousarray(off)).to(self.device, non_blocking=True))

    def _score_shared(self, ids, first_row, heads, padded, cols, mask):
        """``score_requests`` over device ids for requests that share a context -> y_pred fp32 [B]: the chain through the posting
        lists, padded to the bucket as ``score_requests`` pads (``padded``: first_row and heads with the pad request, or None when the
        rows fill the bucket), captured per (bucket, eval key, cols, requests) in ``_postings_graphs`` — the rows that open the
        requests are a static input of the chain, so their number is part of its shape"""
        B = ids.shape[0]
        P = 1 << (B - 1).bit_length()
        if not (self.graph and ids.is_cuda and P <= self.graph_max_batch):
            return self._score_eager(ids, first_row, shared=(mask, heads))
        if P > B:                                                              # the pad rows: copies of the first row, a request of their own
            ids = torch.cat([ids, ids[:1].expand(P - B, -1)])
            first_row, heads = padded
        key = (P, self.model._eval_graph_key((P, self.index.topK + 1, ids.shape[1])), cols, heads.numel())
        g = self._captured(self._postings_graphs, key, lambda: _SharedGraph(self, mask, ids, first_row, heads),
                           "the batched online requests that share a context")
        y_pred = g.run(ids, first_row, heads) if g is not None else self._score_eager(ids, first_row, shared=(mask, heads))
        return y_pred[:B].clone()

    def top_catalogue(self, contexts, n, chunk=None, exclude=None, scores=False, postings=False):
        """The best ``n`` items of the WHOLE catalogue for each of R users: ``contexts`` [R, L] encoded rows -> device tensors (items
        int32 [R, n], catalogue indices, best first, -1 padded; y fp32 [R, n] their predictions; lens int32 [R]) — per request
        ``np.argsort(-y_r, kind="stable")[:n]`` over its M predictions, equal predictions by ascending index.  ``scores=True``:
        additionally the full predictions fp32 [R, M].  The catalogue is swept in passes of ``chunk`` items per request (default
        ``max(1, graph_max_batch // R)``, at most M; the last pass takes what remains).  Per pass: ``rat_catalogue_expand`` in its sweep
        form, ``score_requests`` over device ids and device offsets (its chain, its bucket graphs), ``rat_topn_exclude`` (with
        ``exclude`` only), ``rat_topn_seg``, ``rat_topn_merge`` into the running page — nothing is read back between the passes.
        ``exclude`` = (ex_items [E], ex_offsets [R + 1]): request r never gets the items ``ex_items[ex_offsets[r]:ex_offsets[r + 1]]``
        ("what the user has already seen").  On the host the lists are validated and sorted per request (repeats allowed, entries in
        [0, M)); on the device they are used unread and must be sorted per request.  Excluded items keep their real values in the full
        predictions.  Limit: with ``exclude``, the result equals the reference order for predictions that are not NaN; an excluded
        item is never returned, NaN-valued items may be missing from the tail of a page.
        ``postings=True`` (needs ``build_postings()``; not on a window pool): every pass retrieves through the posting lists — one scan
        per user instead of one per (user, item), ``RetrievalIndex.retrieve_shared``'s chain with the catalogue's columns varying —
        with the same results bit for bit; with ``graph=True`` the pass runs through bucket graphs of its own (``_postings_graphs``),
        and ``score_requests``' are not touched."""
        if self.model.training:
            raise RuntimeError("OnlineScorer.top_catalogue needs the model in eval mode (model.eval())")
        n = _top_n(n)
        cat, cols_dev, R = self._catalogue_contexts(contexts, "top_catalogue")
        mask = self._shared_mask(self._catalogue_cols, postings, "top_catalogue")
        M = cat.shape[0]
        if chunk is None:
            chunk = max(1, self.graph_max_batch // R)
        elif isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or int(chunk) < 1:
            raise ValueError("chunk must be an integer >= 1 (items per request per pass), got %r" % (chunk,))
        chunk = min(int(chunk), M)
        ex_items = ex_off = None
        if exclude is not None:
            ex_items, ex_off = self._exclusion(exclude, R, M)
        contexts = _as_device_ids(contexts, self.device)
        with torch.no_grad():
            run_item = torch.full((R, n), -1, dtype=torch.int32, device=self.device)
            run_val = torch.zeros((R, n), dtype=torch.float32, device=self.device)
            run_len = torch.zeros((R,), dtype=torch.int32, device=self.device)
            full = torch.empty((R, M), dtype=torch.float32, device=self.device) if scores else None
            requests = torch.arange(R + 1, dtype=torch.int64, device=self.device)
            plans = {}                                                         # items per request -> (offsets, heads, first_row, those with a pad request): two sizes at most
            for i0 in range(0, M, chunk):
                m = min(chunk, M - i0)
                if m not in plans:
                    off = requests * m
                    first_row = off[:-1, None].expand(R, m).reshape(-1).contiguous()                   # (R = 1: the reshape is a view of stride 0)
                    padded, P = None, 1 << (R * m - 1).bit_length()
                    if mask is not None and P > R * m:                         # postings: and with the pad request, which opens at row R m
                        padded = (torch.cat([first_row, off[-1:].expand(P - R * m)]), off)
                    plans[m] = (off, off[:-1].contiguous(), first_row, padded)
                off, heads, first_row, padded = plans[m]
                ids = ops.catalogue_expand(self._slab(contexts, heads, R * m), cat, cols_dev, first_row, item0=i0, lib=self._lib)
                if mask is not None:
                    y_pred = self._score_shared(ids, first_row, heads, padded, self._catalogue_cols, mask).contiguous()
                else:
                    y_pred = self.score_requests((ids, off))[0].contiguous()
                ranked = y_pred if ex_items is None else ops.topn_exclude(y_pred, first_row, i0, m, ex_items, ex_off, lib=self._lib)
                pos, val, lens = ops.topn_seg(ranked, first_row, n, lib=self._lib)
                ops.topn_merge(run_item, run_val, run_len, pos, val, lens, heads, i0, ex_items, ex_off, lib=self._lib)
                if scores:
                    full[:, i0:i0 + m] = y_pred.view(R, m)
            return (run_item, run_val, run_len, full) if scores else (run_item, run_val, run_len)
