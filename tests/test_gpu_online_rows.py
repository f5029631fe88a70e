"""A pool that looks at itself on the MI355X: the horizon scan against rat_bm25_topk over truncated copies — bit for bit, the three
pool forms, K = 3 and 12, 1 to 64 ranges —, the gather against numpy, batch_rows / score_rows / evaluate_rows against a numpy assembly,
and a score_rows graph captured before the pool and the weights change."""
import pytest

import online_rows_cases as rc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


@pytest.mark.parametrize("K", [3, 12])
@pytest.mark.parametrize("form", rc.FORMS)
def test_horizon_scan_equals_topk_over_truncated_copies_gpu(form, K):
    rc.check_scan_parity(0, _lib(), form, K)


@pytest.mark.parametrize("K", [3, 12])
@pytest.mark.parametrize("form", rc.FORMS)
def test_rows_behind_the_horizon_never_win_gpu(form, K):
    rc.check_scan_poisoned(0, _lib(), form, K)


def test_horizon_scan_1500_row_pool_gpu():
    rc.check_scan_parity(0, _lib(), "window", 3, n=1500, splits=(7, 0), sizes=(9,))


def test_gather_rows_equals_numpy_gpu():
    rc.check_gather("cuda:0", _lib())


@pytest.mark.parametrize("form", rc.FORMS)
def test_batch_score_and_evaluate_rows_see_only_older_rows_gpu(form):
    rc.check_scores(0, _lib(), form)


@pytest.mark.parametrize("form", rc.FORMS)
def test_score_rows_graph_survives_pool_and_weight_changes_gpu(form):
    rc.check_rows_graph(0, _lib(), form)


def test_rows_refusals_gpu():
    rc.check_rows_refusals(0, _lib())
