"""The sliding pool on the MI355X: the device-side push and evict, the scan and the assembly over a ring whose header lives in device
memory, and RetrievalIndex / OnlineScorer with ``window=True`` against fresh immutable objects over the live rows — eager and through
request graphs captured BEFORE the first append and the first eviction."""
import pytest

import online_window_cases as wc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


def test_ring_scan_equals_single_range_over_live_rows_gpu():
    wc.check_ring_scan("cuda:0", _lib())


def test_ring_scan_large_capacity_gpu():
    # the library's own range count for a 200 000-row capacity (196 ranges for one query tile), the wrap inside and between them
    wc.check_ring_scan("cuda:0", _lib(), capacity=200_000, ns=(1, 1000, 150_001, None), splits=(1, 61, 256),
                       fixed_heads=(0, 1, 255, 256, 100_000, -1))


def test_ring_scan_clamps_the_header_gpu():
    wc.check_ring_scan_clamps("cuda:0", _lib())


def test_ring_ties_follow_age_not_address_gpu():
    wc.check_ring_ties("cuda:0", _lib())


def test_pool_push_and_evict_equal_numpy_gpu():
    wc.check_pool_push("cuda:0", _lib())
    wc.check_pool_push("cuda:0", _lib(), capacity=100_000, sizes=(40_000, 1, 59_000), wrapping=70_000)


# RAT_m2 and one variant; eager
@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_window_equals_fresh_scorer_through_several_laps_gpu(name):
    wc.check_window_equals_fresh(name, 0, _lib())
    wc.check_window_equals_fresh(name, 0, _lib(), capacity=50)


# the request graph is captured before the first append / eviction and replayed after every one, and after a training step
@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_captured_request_serves_the_sliding_pool_gpu(name):
    wc.check_window_equals_fresh(name, 0, _lib(), graph=True, train_step=True)


def test_window_refusals_gpu():
    wc.check_window_refusals(0, _lib())


@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_window_without_pushes_equals_offline_gpu(name):
    wc.check_window_without_pushes(name, 0, _lib(), sizes=(5, 17), graph=True, train_step=True)
