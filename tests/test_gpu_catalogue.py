"""The device-resident item catalogue on the MI355X: rat_catalogue_expand against the rows built in numpy; rat_topn_exclude and
rat_topn_merge against numpy's stable sort over everything a sweep has seen — items exact, values bit for bit; OnlineScorer.top_items /
rank_items against top_candidates / rank_candidates over catalogue[items]; top_catalogue against per-pass score_requests over host-built
rows; and the shared bucket graphs: top_catalogue replays score_requests' own graphs, before and after the pool, the labels and the
catalogue change."""
import pytest

import catalogue_cases as cc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


def test_catalogue_expand_equals_numpy_gpu():
    cc.check_expand_kernel("cuda:0", _lib())


@pytest.mark.parametrize("set_name,which", [("eighths", None), ("special", None)] + [("eighths", w) for w in cc.EXCLUSIONS])
def test_topn_merge_equals_numpy_stable_sort_gpu(set_name, which):
    cc.check_merge_kernel("cuda:0", _lib(), set_name, which)


def test_two_merges_equal_one_merge_over_the_union_gpu():
    cc.check_two_merges_equal_one("cuda:0", _lib())


def test_abi_refusals_gpu():
    cc.check_abi_refusals("cuda:0", _lib())


def test_ops_refusals_gpu():
    cc.check_ops_refusals("cuda:0", _lib())


@pytest.mark.parametrize("form", cc.rq.FORMS)
def test_top_and_rank_items_equal_candidates_over_host_rows_gpu(form):
    cc.check_items("tiny_seq_bn", 0, _lib(), form)


@pytest.mark.parametrize("form", cc.rq.FORMS)
def test_top_catalogue_equals_numpy_over_score_requests_gpu(form):
    cc.check_top_catalogue("tiny_seq_bn", 0, _lib(), form)


@pytest.mark.parametrize("chunk", [cc.M_CAT, 1])
def test_top_catalogue_in_one_pass_and_item_by_item_gpu(chunk):
    cc.check_top_catalogue("tiny_seq_bn", 0, _lib(), "immutable", ns=(5,), chunks=(chunk,))


def test_top_catalogue_replays_the_shared_bucket_graphs_gpu():
    cc.check_catalogue_graphs("tiny_seq_bn", 0, _lib())


def test_catalogue_refusals_reach_no_entry_point_gpu():
    cc.check_refusals(0, _lib())


@pytest.mark.parametrize("form", cc.rq.FORMS)
def test_catalogue_launch_chain_gpu(form):
    cc.check_launch_chain(0, _lib(), form)
