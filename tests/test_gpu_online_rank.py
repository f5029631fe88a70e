"""Each request's full ranking on the MI355X: rat_rank_seg against numpy's stable sort — positions and ranks exact, values bit for
bit — over online_top_cases' segments, segments at the kernel's own tile and work-group sizes and a 4097-row segment, with rat_topn_seg
as the prefix at every n; OnlineScorer.rank_requests / rank_candidates in the three pool forms; and the captured chains: one graph per
bucket serves every request mix and every padded total of its bucket, before and after the pool and the weights change."""
import pytest

import online_rank_cases as rc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


@pytest.mark.parametrize("set_name", rc.tc.SETS)
def test_rank_seg_equals_numpy_stable_sort_gpu(set_name):
    rc.check_rank_kernel("cuda:0", _lib(), set_name)


@pytest.mark.parametrize("which", ["tile", "long"])
def test_rank_seg_at_the_tile_across_work_groups_and_past_the_graph_limit_gpu(which):
    rc.check_rank_own("cuda:0", _lib(), which, ns=rc.tc.NS)


def test_abi_refusals_gpu():
    rc.check_abi_refusals("cuda:0", _lib())


def test_ops_refusals_gpu():
    rc.check_ops_refusals("cuda:0", _lib())


@pytest.mark.parametrize("form", rc.rq.FORMS)
def test_rank_requests_equal_numpy_over_score_requests_gpu(form):
    rc.check_rank_requests("tiny_seq_bn", 0, _lib(), form)


def test_rank_requests_300_row_pool_gpu():
    rc.check_rank_requests("tiny_seq_bn", 0, _lib(), "immutable", n_pool=300)


@pytest.mark.parametrize("form", rc.rq.FORMS)
def test_rank_candidates_equal_rank_requests_over_host_rows_gpu(form):
    rc.check_rank_candidates("tiny_seq_bn", 0, _lib(), form)


def test_rank_candidates_300_row_pool_gpu():
    rc.check_rank_candidates("tiny_seq_bn", 0, _lib(), "immutable", n_pool=300)


@pytest.mark.parametrize("form", rc.rq.FORMS)
def test_rank_graphs_serve_every_mix_and_survive_pool_changes_gpu(form):
    rc.check_rank_graphs("tiny_seq_bn", 0, _lib(), form)


def test_rank_refusals_reach_no_entry_point_gpu():
    rc.check_refusals(0, _lib())


@pytest.mark.parametrize("form", rc.rq.FORMS)
def test_rank_launch_chain_gpu(form):
    rc.check_launch_chain(0, _lib(), form)
