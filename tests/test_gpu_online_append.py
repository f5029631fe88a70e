"""The growing pool on the MI355X: the device-side append, the scan and the assembly with the row count in device memory, and
RetrievalIndex / OnlineScorer with ``capacity`` against fresh immutable objects over the concatenated pool — eager and through request
graphs captured BEFORE the appends."""
import pytest

import online_append_cases as ac

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


def test_split_dev_ignores_rows_beyond_the_count_gpu():
    ac.check_split_dev("cuda:0", _lib())


def test_split_dev_large_capacity_gpu():
    # the library's own range count for a 200 000-row capacity (196 ranges for one query tile), most of them empty at first
    ac.check_split_dev("cuda:0", _lib(), capacity=200_000, ns=(1, 1000, 150_001, None), splits=(1, 61, 256))


def test_split_dev_ties_across_ranges_gpu():
    ac.check_split_dev_ties("cuda:0", _lib())


def test_split_dev_finds_appended_rows_gpu():
    ac.check_split_dev_after_append("cuda:0", _lib())
    ac.check_split_dev_after_append("cuda:0", _lib(), capacity=100_000, n=60_000, M=30_000)


def test_pool_append_equals_concatenation_gpu():
    ac.check_pool_append("cuda:0", _lib())
    ac.check_pool_append("cuda:0", _lib(), sizes=(40_000, 1, 70_000))


# RAT_m2 and one variant; eager
@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_append_equals_fresh_scorer_gpu(name):
    ac.check_append_equals_fresh(name, 0, _lib())


# the request graph is captured before the first append and replayed after every one, and after a training step
@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_captured_request_serves_the_grown_pool_gpu(name):
    ac.check_append_equals_fresh(name, 0, _lib(), graph=True, train_step=True)


def test_append_refusals_gpu():
    ac.check_append_refusals(0, _lib())


@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_capacity_without_appends_equals_offline_gpu(name):
    ac.check_capacity_without_appends(name, 0, _lib(), sizes=(5, 17), graph=True, train_step=True)
