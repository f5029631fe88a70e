"""Which entry points of the library every call of the online request path reaches, and in which order, for the three forms of the
pool: the lists below were recorded before ops.py's scan and assembly wrappers were folded into one each, so a wrapper that picks
another entry point (the plain scan through the horizon kernel, say) or another order fails here, on the host-emulation build."""
import os
import sys

import numpy as np
import pytest

import online_requests_cases as rq

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

WATCHED = ("rat_bm25_", "rat_batch_assemble", "rat_pool_")


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


class Recorder:
    """a RatLib whose ``call`` and ``size`` note the entry point's name before forwarding"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def call(self, name, *args):
        self.names.append(name)
        return self._lib.call(name, *args)

    def size(self, name, *args):
        self.names.append(name)
        return self._lib.size(name, *args)

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def take(self):
        names, self.names = [n for n in self.names if n.startswith(WATCHED)], []
        return names


def record_chains(form, lib, n_pool=14):
    """-> {call: [entry points in launch order]} of one scorer of that form (graph=False: a capture runs the eager chain)"""
    from rat_amd.online import OnlineScorer
    _case, model, data, pool, cols, cfg = rq._setup("tiny_seq_bn", -1, n_pool=n_pool)
    first, kw, later, _live = rq._form(form, pool, n_pool)
    rec = Recorder(lib)
    scorer = OnlineScorer(model, first, cfg, graph=False, lib=rec, **kw)
    if later is not None:
        scorer.append(later)
    rec.take()
    index = scorer.index
    ids = np.ascontiguousarray(data[:6, :-1])
    same, rows = [cols[0]], [5, 2, 9]
    key = data[-1:, cols].astype(np.int64)                                     # the used columns of the row appended below
    chains = {}

    def note(what, fn):
        fn()
        chains[what] = rec.take()
    note("retrieve(ids)", lambda: index.retrieve(ids))
    note("retrieve(ids, before=)", lambda: index.retrieve(ids, before=[3, 0, 14, 7, 99, 1]))
    note("retrieve(ids, same=)", lambda: index.retrieve(ids, same=same))
    note("retrieve(ids, request_offsets=)", lambda: index.retrieve(ids, request_offsets=[0, 2, 6]))
    note("score", lambda: scorer.score(ids))
    note("score(same=)", lambda: scorer.score(ids, same=same))
    note("score_rows", lambda: scorer.score_rows(rows))
    note("score_rows(same=)", lambda: scorer.score_rows(rows, same=same))
    note("score_requests", lambda: scorer.score_requests([ids[:2], ids[2:]]))
    note("batch_rows", lambda: scorer.batch_rows(rows))
    note("find", lambda: scorer.find(list(cols), key))
    note("set_labels", lambda: scorer.set_labels([0, 2], 1.0))
    note("relabel_where", lambda: scorer.relabel_where(list(cols), key, 0.0))
    if form != "immutable":
        note("append", lambda: scorer.append(data[-2:]))
    if form == "window":
        note("evict", lambda: scorer.evict(2))
        note("delete", lambda: scorer.delete([1, 3]))
        removed = []
        note("delete_where", lambda: removed.append(scorer.delete_where(list(cols), key)))
        assert 0 < removed[0] < 12, "delete_where found nothing to delete, or refused"
    return chains


# record_chains() of the three forms, printed by pprint at the commit before the wrappers were unified (rat_bm25_topk_split_workspace is
# the sizing call every scan wrapper makes first)
CHAINS = {"immutable": {"retrieve(ids)": ["rat_bm25_query_prepare", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split"],
               "retrieve(ids, before=)": ["rat_bm25_query_prepare", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_before"],
               "retrieve(ids, same=)": ["rat_bm25_exact_count",
                                        "rat_bm25_exact_plan",
                                        "rat_bm25_query_prepare_seg",
                                        "rat_bm25_topk_split_workspace",
                                        "rat_bm25_topk_split_exact"],
               "retrieve(ids, request_offsets=)": ["rat_bm25_query_prepare_seg", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split"],
               "score": ["rat_bm25_query_prepare", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split", "rat_batch_assemble"],
               "score(same=)": ["rat_bm25_exact_count",
                                "rat_bm25_exact_plan",
                                "rat_bm25_query_prepare_seg",
                                "rat_bm25_topk_split_workspace",
                                "rat_bm25_topk_split_exact",
                                "rat_batch_assemble"],
               "score_rows": ["rat_pool_gather_rows",
                              "rat_bm25_query_prepare",
                              "rat_bm25_topk_split_workspace",
                              "rat_bm25_topk_split_before",
                              "rat_batch_assemble"],
               "score_rows(same=)": ["rat_pool_gather_rows",
                                     "rat_bm25_exact_count",
                                     "rat_bm25_exact_plan",
                                     "rat_bm25_query_prepare_seg",
                                     "rat_bm25_topk_split_workspace",
                                     "rat_bm25_topk_split_exact",
                                     "rat_batch_assemble"],
               "score_requests": ["rat_bm25_query_prepare_seg", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split", "rat_batch_assemble"],
               "batch_rows": ["rat_pool_gather_rows",
                              "rat_bm25_query_prepare",
                              "rat_bm25_topk_split_workspace",
                              "rat_bm25_topk_split_before",
                              "rat_batch_assemble"],
               "find": ["rat_pool_find"],
               "set_labels": ["rat_pool_set_labels"],
               "relabel_where": ["rat_pool_find", "rat_pool_set_labels"]},
 "capacity": {"retrieve(ids)": ["rat_bm25_query_prepare", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_dev"],
              "retrieve(ids, before=)": ["rat_bm25_query_prepare", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_before"],
              "retrieve(ids, same=)": ["rat_bm25_exact_count",
                                       "rat_bm25_exact_plan",
                                       "rat_bm25_query_prepare_seg",
                                       "rat_bm25_topk_split_workspace",
                                       "rat_bm25_topk_split_exact"],
              "retrieve(ids, request_offsets=)": ["rat_bm25_query_prepare_seg", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_dev"],
              "score": ["rat_bm25_query_prepare", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_dev", "rat_batch_assemble_dev"],
              "score(same=)": ["rat_bm25_exact_count",
                               "rat_bm25_exact_plan",
                               "rat_bm25_query_prepare_seg",
                               "rat_bm25_topk_split_workspace",
                               "rat_bm25_topk_split_exact",
                               "rat_batch_assemble_dev"],
              "score_rows": ["rat_pool_gather_rows",
                             "rat_bm25_query_prepare",
                             "rat_bm25_topk_split_workspace",
                             "rat_bm25_topk_split_before",
                             "rat_batch_assemble_dev"],
              "score_rows(same=)": ["rat_pool_gather_rows",
                                    "rat_bm25_exact_count",
                                    "rat_bm25_exact_plan",
                                    "rat_bm25_query_prepare_seg",
                                    "rat_bm25_topk_split_workspace",
                                    "rat_bm25_topk_split_exact",
                                    "rat_batch_assemble_dev"],
              "score_requests": ["rat_bm25_query_prepare_seg", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_dev", "rat_batch_assemble_dev"],
              "batch_rows": ["rat_pool_gather_rows",
                             "rat_bm25_query_prepare",
                             "rat_bm25_topk_split_workspace",
                             "rat_bm25_topk_split_before",
                             "rat_batch_assemble_dev"],
              "find": ["rat_pool_find"],
              "set_labels": ["rat_pool_set_labels"],
              "relabel_where": ["rat_pool_find", "rat_pool_set_labels"],
              "append": ["rat_pool_append"]},
 "window": {"retrieve(ids)": ["rat_bm25_query_prepare", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_ring"],
            "retrieve(ids, before=)": ["rat_bm25_query_prepare", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_before"],
            "retrieve(ids, same=)": ["rat_bm25_exact_count",
                                     "rat_bm25_exact_plan",
                                     "rat_bm25_query_prepare_seg",
                                     "rat_bm25_topk_split_workspace",
                                     "rat_bm25_topk_split_exact"],
            "retrieve(ids, request_offsets=)": ["rat_bm25_query_prepare_seg", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_ring"],
            "score": ["rat_bm25_query_prepare", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_ring", "rat_batch_assemble_ring"],
            "score(same=)": ["rat_bm25_exact_count",
                             "rat_bm25_exact_plan",
                             "rat_bm25_query_prepare_seg",
                             "rat_bm25_topk_split_workspace",
                             "rat_bm25_topk_split_exact",
                             "rat_batch_assemble_ring"],
            "score_rows": ["rat_pool_gather_rows",
                           "rat_bm25_query_prepare",
                           "rat_bm25_topk_split_workspace",
                           "rat_bm25_topk_split_before",
                           "rat_batch_assemble_ring"],
            "score_rows(same=)": ["rat_pool_gather_rows",
                                  "rat_bm25_exact_count",
                                  "rat_bm25_exact_plan",
                                  "rat_bm25_query_prepare_seg",
                                  "rat_bm25_topk_split_workspace",
                                  "rat_bm25_topk_split_exact",
                                  "rat_batch_assemble_ring"],
            "score_requests": ["rat_bm25_query_prepare_seg", "rat_bm25_topk_split_workspace", "rat_bm25_topk_split_ring", "rat_batch_assemble_ring"],
            "batch_rows": ["rat_pool_gather_rows",
                           "rat_bm25_query_prepare",
                           "rat_bm25_topk_split_workspace",
                           "rat_bm25_topk_split_before",
                           "rat_batch_assemble_ring"],
            "find": ["rat_pool_find"],
            "set_labels": ["rat_pool_set_labels"],
            "relabel_where": ["rat_pool_find", "rat_pool_set_labels"],
            "append": ["rat_pool_push"],
            "evict": ["rat_pool_evict"],
            "delete": ["rat_pool_delete"],
            "delete_where": ["rat_pool_find", "rat_pool_delete"]}}


@pytest.mark.parametrize("form", rq.FORMS)
def test_every_call_reaches_the_recorded_entry_points_in_order(emu_lib, form):
    got = record_chains(form, emu_lib)
    want = CHAINS[form]
    assert sorted(got) == sorted(want)
    for what in want:
        assert got[what] == want[what], (form, what)
