"""Candidate retrieval through posting lists on the MI355X: rat_bm25_topk_postings against the numpy restatement of rat_bm25_topk's
contract at every (K, varying set, n_sorted) — a result drawn from a posting list, the context list and the tail at once, ties at the
K-th place, rows in two lists, absent ids, empty contexts, short lists —, posting lists of 2500 rows, RetrievalIndex.build_postings /
retrieve_shared, postings=True of the five OnlineScorer calls against postings=False, and top_catalogue(postings=True) through bucket
graphs of its own, before and after an append and a rebuild."""
import pytest

import postings_cases as pc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


@pytest.mark.parametrize("K", pc.KS)
def test_postings_kernel_equals_numpy_gpu(K):
    pc.check_kernel("cuda:0", _lib(), K)


def test_ties_at_the_kth_place_between_context_and_posting_rows_gpu():
    pc.check_ties("cuda:0", _lib())


def test_long_posting_lists_gpu():
    pc.check_long_lists("cuda:0", _lib())


def test_build_postings_and_retrieve_shared_gpu():
    pc.check_index("cuda:0", _lib())


def test_abi_refusals_gpu():
    pc.check_abi_refusals("cuda:0", _lib())


def test_ops_refusals_gpu():
    pc.check_ops_refusals("cuda:0", _lib())


@pytest.mark.parametrize("form", ["immutable", "capacity"])
def test_calls_with_postings_equal_calls_without_gpu(form):
    pc.check_scorer_calls("tiny_seq_bn", 0, _lib(), form)


def test_top_catalogue_with_postings_replays_bucket_graphs_of_its_own_gpu():
    pc.check_postings_graphs("tiny_seq_bn", 0, _lib())


def test_postings_refusals_reach_no_entry_point_gpu():
    pc.check_refusals(0, _lib())


@pytest.mark.parametrize("form", ["immutable", "capacity"])
def test_postings_launch_chain_gpu(form):
    pc.check_launch_chain(0, _lib(), form)
