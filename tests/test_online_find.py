"""The pool addressed by key on the CPU: rat_pool_find and rat_pool_set_labels through the host-emulation build (tests/emu), find /
set_labels / relabel_where / delete_where of RetrievalIndex and OnlineScorer on top of them.  The same checks, with many work-groups
and captured request graphs, run on the MI355X in tests/test_gpu_online_find.py; the corrupt-input check runs here only."""
import os
import sys

import pytest

import online_find_cases as fc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


# the emulator runs one OS thread per GPU thread: pools of 50 slots, one tall one for the several-trips path
def test_pool_find_equals_numpy_emulated(emu_lib):
    fc.check_find("cpu", emu_lib)


def test_pool_find_does_not_depend_on_the_ranges_emulated(emu_lib):
    fc.check_find_groups("cpu", emu_lib, live=(1, 50), forms=("dev", "ring"))      # 64 ranges are 129 emulated work-groups a find


def test_pool_find_truncates_and_pads_emulated(emu_lib):
    fc.check_find_truncation("cpu", emu_lib)


def test_pool_find_queued_behind_push_delete_evict_emulated(emu_lib):
    fc.check_find_queued("cpu", emu_lib)


def test_pool_set_labels_equals_numpy_emulated(emu_lib):
    fc.check_set_labels("cpu", emu_lib)


def test_pool_find_and_set_labels_corrupt_inputs_stay_inside_the_buffers_emulated(emu_lib):
    fc.check_find_corrupt(emu_lib)


@pytest.mark.parametrize("form", ["immutable", "capacity", "window"])
def test_objects_equal_fresh_scorer_emulated(emu_lib, form):
    fc.check_objects_equal_fresh("tiny_seq_bn", -1, emu_lib, form)


def test_find_refusals(emu_lib):
    fc.check_find_refusals(-1, emu_lib)
