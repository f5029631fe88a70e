"""Ranking metrics on the device, on the MI355X: rat_eval_rank_metrics against the per-group numpy loop at n = 2 ... 2^20 (several sort
tiles, several reduction levels), eight cutoffs in one call against eight calls, the tie rule, the status bits, the ABI refusals, and the
objects on top: OnlineScorer.evaluate_rows(cutoffs=) / rank_metrics_rows in the three pool forms and BaseModel.evaluate_generator with
the ranking names on host 4-tuples and DeviceBatches, device_metrics off and on."""
import pytest

import rank_metrics_cases as rk

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rk.report()


@pytest.mark.parametrize("n", rk.NS_EMU)
def test_ndcg_mrr_hitrate_equal_the_loop_reference_gpu(n):
    rk.check_parity(0, _lib(), n)


@pytest.mark.parametrize("n", [70001, 1 << 20])                  # several sort tiles, several reduction levels
def test_ndcg_mrr_hitrate_equal_the_loop_reference_large_gpu(n):
    rk.check_parity(0, _lib(), n, big=True)


@pytest.mark.parametrize("n", [65, 4097, 70001])
def test_eight_cutoffs_in_one_call_equal_eight_calls_gpu(n):
    rk.check_eight_cutoffs(0, _lib(), n)


@pytest.mark.parametrize("n", [65, 4097, 70001])
def test_ties_keep_input_order_and_tie_free_rows_may_be_permuted_gpu(n):
    rk.check_tie_rule(0, _lib(), n)


def test_undefined_metrics_are_nan_with_a_status_bit_and_a_value_error_gpu():
    rk.check_status(0, _lib())


def test_abi_refusals_launch_nothing_gpu():
    rk.check_abi_refusals(0, _lib())


@pytest.mark.parametrize("form", ["immutable", "capacity", "window"])
def test_evaluate_rows_cutoffs_and_rank_metrics_rows_gpu(form):
    rk.check_scorer(0, _lib(), form)


def test_evaluate_generator_ranking_names_gpu():
    rk.check_generator(0, _lib())


def test_construction_refusals_gpu():
    rk.check_construction_refusals(0, _lib())
