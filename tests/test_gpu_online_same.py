"""Neighbours restricted to rows equal on given columns on the MI355X: retrieve(ids, same=...) against the offline exact-match path —
bit for bit, the three pool forms, one and two columns, K = 3 and 12, 1 to 64 ranges —, horizons against a numpy restatement, batch /
score / batch_rows / score_rows / evaluate_rows against a numpy assembly, and graphs of score(ids, same=) and score_rows(indices,
same=) captured before the pool and the weights change."""
import pytest

import online_same_cases as sc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


@pytest.mark.parametrize("same", sc.SAMES, ids=["one_column", "two_columns"])
@pytest.mark.parametrize("K", [3, 12])
@pytest.mark.parametrize("form", sc.FORMS)
def test_same_equals_the_offline_exact_match_path_gpu(form, K, same):
    sc.check_offline_parity(0, _lib(), form, K, same)


def test_same_1500_row_window_gpu():
    sc.check_offline_parity(0, _lib(), "window", 3, sc.SAMES[1], n=1500, splits=(7, 0), sizes=(9,))


@pytest.mark.parametrize("same", sc.SAMES, ids=["one_column", "two_columns"])
@pytest.mark.parametrize("K", [3, 12])
@pytest.mark.parametrize("form", sc.FORMS)
def test_same_below_a_horizon_equals_the_numpy_restatement_gpu(form, K, same):
    sc.check_horizons(0, _lib(), form, K, same, splits=(1, 3, 64))


@pytest.mark.parametrize("form", sc.FORMS)
def test_batch_score_and_rows_with_same_gpu(form):
    sc.check_objects(0, _lib(), form)


@pytest.mark.parametrize("form", sc.FORMS)
def test_same_graphs_survive_pool_and_weight_changes_gpu(form):
    sc.check_graphs(0, _lib(), form)


def test_same_refusals_gpu():
    sc.check_refusals(0, _lib())
