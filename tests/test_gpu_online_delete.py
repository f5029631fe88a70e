"""Deletion from the sliding pool on the MI355X: the device-side compaction against numpy, the tie rule after it, and RetrievalIndex /
OnlineScorer ``delete`` against fresh immutable objects over the survivors — eager and through a request graph captured BEFORE the
first deletion."""
import pytest

import online_delete_cases as dc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


def test_pool_delete_equals_numpy_delete_gpu():
    dc.check_pool_delete("cuda:0", _lib())


def test_pool_delete_queued_between_pushes_gpu():
    dc.check_pool_delete_queued("cuda:0", _lib())


def test_pool_delete_many_work_groups_gpu():
    dc.check_pool_delete_large("cuda:0", _lib())


def test_ties_follow_age_after_a_deletion_gpu():
    dc.check_delete_ties("cuda:0", _lib())


# RAT_m2 and one variant; eager
@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_delete_equals_fresh_scorer_gpu(name):
    dc.check_delete_equals_fresh(name, 0, _lib())
    dc.check_delete_equals_fresh(name, 0, _lib(), capacity=50)


# the request graph is captured before the first deletion and replayed after every operation, and after a training step
@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_captured_request_serves_the_pool_after_deletions_gpu(name):
    dc.check_delete_equals_fresh(name, 0, _lib(), graph=True, train_step=True)


def test_delete_refusals_gpu():
    dc.check_delete_refusals(0, _lib())
