"""The sliding pool on the CPU: rat_pool_push, rat_pool_evict, rat_bm25_topk_split_ring and rat_batch_assemble_ring through the
host-emulation build (tests/emu), RetrievalIndex / OnlineScorer with ``capacity`` and ``window=True`` on top of them.  The same checks,
larger and with captured request graphs, run on the MI355X in tests/test_gpu_online_window.py."""
import os
import sys

import pytest

import online_window_cases as wc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


# the emulator runs one OS thread per GPU thread: every head x every row count for 1, 3, 64 ranges and the library's choice, and every
# head at one row count for 256 ranges (most of the work-groups), for the four-query-tile instantiation (topK <= 8); a subset of row and
# range counts (every head) for the one-query-tile instantiation (five times the work-groups); the GPU test runs every combination
def test_ring_scan_equals_single_range_over_live_rows_emulated(emu_lib):
    wc.check_ring_scan("cpu", emu_lib, topks=(3,), splits=(1, 3, 64))


def test_ring_scan_256_ranges_emulated(emu_lib):
    wc.check_ring_scan("cpu", emu_lib, topks=(3,), ns=(1000,), splits=(256,))


def test_ring_scan_equals_single_range_over_live_rows_topk9_emulated(emu_lib):
    wc.check_ring_scan("cpu", emu_lib, topks=(9,), ns=(255, None), splits=(3, 64))


def test_ring_scan_clamps_the_header_emulated(emu_lib):
    wc.check_ring_scan_clamps("cpu", emu_lib)


def test_ring_ties_follow_age_not_address_emulated(emu_lib):
    wc.check_ring_ties("cpu", emu_lib)


def test_pool_push_and_evict_equal_numpy_emulated(emu_lib):
    wc.check_pool_push("cpu", emu_lib)


def test_window_equals_fresh_scorer_through_several_laps_emulated(emu_lib):
    wc.check_window_equals_fresh("tiny_seq_bn", -1, emu_lib)


def test_window_refusals(emu_lib):
    wc.check_window_refusals(-1, emu_lib)


def test_window_without_pushes_equals_offline_emulated(emu_lib):
    wc.check_window_without_pushes("tiny_seq_bn", -1, emu_lib, sizes=(7,), graph=False)
