"""Each request's top-n candidates on the MI355X: rat_topn_seg against numpy's stable sort — positions exact, values bit for bit — over
segments on both sides of n, a wave, a work-group and the staged length; rat_candidates_expand against the rows built on the host;
OnlineScorer.top_requests / top_candidates in the three pool forms; and the captured chains: one graph per (bucket, n) serves every
request mix and every padded total of its bucket, before and after the pool and the weights change."""
import pytest

import online_top_cases as tc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


@pytest.mark.parametrize("set_name", tc.SETS)
def test_topn_seg_equals_numpy_stable_sort_gpu(set_name):
    tc.check_topn_kernel("cuda:0", _lib(), set_name)


def test_candidates_expand_equals_numpy_gpu():
    tc.check_expand_kernel("cuda:0", _lib())


def test_abi_refusals_gpu():
    tc.check_abi_refusals("cuda:0", _lib())


def test_ops_refusals_gpu():
    tc.check_ops_refusals("cuda:0", _lib())


@pytest.mark.parametrize("form", tc.rq.FORMS)
def test_top_requests_equal_numpy_over_score_requests_gpu(form):
    tc.check_top_requests("tiny_seq_bn", 0, _lib(), form)


def test_top_requests_300_row_pool_gpu():
    tc.check_top_requests("tiny_seq_bn", 0, _lib(), "immutable", n_pool=300)


@pytest.mark.parametrize("form", tc.rq.FORMS)
def test_top_candidates_equal_top_requests_over_host_rows_gpu(form):
    tc.check_top_candidates("tiny_seq_bn", 0, _lib(), form)


def test_top_candidates_300_row_pool_gpu():
    tc.check_top_candidates("tiny_seq_bn", 0, _lib(), "immutable", n_pool=300)


@pytest.mark.parametrize("form", tc.rq.FORMS)
def test_top_graphs_serve_every_mix_and_survive_pool_changes_gpu(form):
    tc.check_top_graphs("tiny_seq_bn", 0, _lib(), form)


def test_top_refusals_reach_no_entry_point_gpu():
    tc.check_refusals(0, _lib())


@pytest.mark.parametrize("form", tc.rq.FORMS)
def test_top_launch_chain_gpu(form):
    tc.check_launch_chain(0, _lib(), form)
