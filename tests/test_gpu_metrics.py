"""Evaluation metrics on the device, on the MI355X: rat_eval_metrics against auc_score / log_loss / sklearn per group at n = 2 ... 2^20
(several sort tiles, several reduction levels), the order of the rows, the status bits, the ABI refusals, and the objects on top:
OnlineScorer.evaluate_rows(group=, device=) / metrics_rows in the three pool forms and BaseModel.evaluate_generator with
device_metrics / group_id on host 4-tuples and DeviceBatches."""
import pytest

import metrics_cases as mx

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    mx.report()


@pytest.mark.parametrize("n", mx.NS_EMU)
def test_logloss_auc_gauc_equal_the_host_references_gpu(n):
    mx.check_parity(0, _lib(), n)


@pytest.mark.parametrize("n", [70001, 1 << 20])                  # several sort tiles, several reduction levels
def test_logloss_auc_gauc_equal_the_host_references_large_gpu(n):
    mx.check_parity(0, _lib(), n, big=True)


@pytest.mark.parametrize("n", [65, 4097, 70001])
def test_row_order_changes_nothing_but_logloss_rounding_gpu(n):
    mx.check_row_order(0, _lib(), n)


def test_undefined_metrics_are_nan_with_a_status_bit_and_a_value_error_gpu():
    mx.check_status(0, _lib())


def test_abi_refusals_launch_nothing_gpu():
    mx.check_abi_refusals(0, _lib())


@pytest.mark.parametrize("form", ["immutable", "capacity", "window"])
def test_evaluate_rows_and_metrics_rows_gpu(form):
    mx.check_scorer(0, _lib(), form)


def test_evaluate_generator_device_metrics_and_gauc_gpu():
    mx.check_generator(0, _lib())


def test_construction_refusals_gpu(monkeypatch):
    mx.check_construction_refusals(0, _lib(), monkeypatch)
