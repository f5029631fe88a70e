"""Deletion from the sliding pool on the CPU: rat_pool_delete through the host-emulation build (tests/emu), RetrievalIndex.delete /
OnlineScorer.delete on top of it.  The same checks, larger and with captured request graphs, run on the MI355X in
tests/test_gpu_online_delete.py; the corrupt-input check runs here only."""
import os
import sys

import pytest

import online_delete_cases as dc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


# the emulator runs one OS thread per GPU thread: the capacity stays at 200 rows here (one work-group per launch)
def test_pool_delete_equals_numpy_delete_emulated(emu_lib):
    dc.check_pool_delete("cpu", emu_lib)


def test_pool_delete_queued_between_pushes_emulated(emu_lib):
    dc.check_pool_delete_queued("cpu", emu_lib)


def test_pool_delete_corrupt_header_or_list_stays_inside_the_buffers_emulated(emu_lib):
    dc.check_pool_delete_corrupt(emu_lib)


def test_ties_follow_age_after_a_deletion_emulated(emu_lib):
    dc.check_delete_ties("cpu", emu_lib, topks=(3,), splits=(1, 3))


def test_delete_equals_fresh_scorer_emulated(emu_lib):
    dc.check_delete_equals_fresh("tiny_seq_bn", -1, emu_lib)


def test_delete_refusals(emu_lib):
    dc.check_delete_refusals(-1, emu_lib)
