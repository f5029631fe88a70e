"""The pool addressed by key on the MI355X: the device-side search against numpy (both layouts, the three pool forms, forced and chosen
ranges, truncation, queued behind pushes, deletions and evictions), labels written through the ring, and find / set_labels /
relabel_where / delete_where of RetrievalIndex and OnlineScorer against fresh immutable objects — eager and through a request graph
captured BEFORE the first relabel."""
import pytest

import online_find_cases as fc

pytestmark = pytest.mark.gpu


def _lib():
    import rat_amd._lib as L
    return L.get_lib()


def test_pool_find_equals_numpy_gpu():
    fc.check_find("cuda:0", _lib())


def test_pool_find_does_not_depend_on_the_ranges_gpu():
    fc.check_find_groups("cuda:0", _lib())


def test_pool_find_many_work_groups_gpu():
    fc.check_find_large("cuda:0", _lib())


def test_pool_find_truncates_and_pads_gpu():
    fc.check_find_truncation("cuda:0", _lib())


def test_pool_find_queued_behind_push_delete_evict_gpu():
    fc.check_find_queued("cuda:0", _lib())


def test_pool_set_labels_equals_numpy_gpu():
    fc.check_set_labels("cuda:0", _lib())


# RAT_m2 and one variant; eager
@pytest.mark.parametrize("form", ["immutable", "capacity", "window"])
@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_objects_equal_fresh_scorer_gpu(name, form):
    fc.check_objects_equal_fresh(name, 0, _lib(), form)


# the request graph is captured before the first relabel and replayed after every step, and after a training step
@pytest.mark.parametrize("form", ["immutable", "capacity", "window"])
@pytest.mark.parametrize("name", ["tiny_seq_bn", "m1_tiny_seq"])
def test_captured_request_serves_the_pool_after_relabels_gpu(name, form):
    fc.check_objects_equal_fresh(name, 0, _lib(), form, graph=True, train_step=True)


def test_find_refusals_gpu():
    fc.check_find_refusals(0, _lib())
