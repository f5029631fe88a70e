"""The growing pool on the CPU: rat_pool_append, rat_bm25_topk_split_dev and rat_batch_assemble_dev through the host-emulation build
(tests/emu), RetrievalIndex / OnlineScorer with ``capacity`` on top of them.  The same checks, larger and with captured request
graphs, run on the MI355X in tests/test_gpu_online_append.py."""
import os
import sys

import pytest

import online_append_cases as ac

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


# the emulator runs one OS thread per GPU thread: every row count x every range count for the four-query-tile instantiation (topK <= 8),
# a subset for the one-query-tile instantiation (five times the work-groups); the GPU test runs every combination for both
def test_split_dev_ignores_rows_beyond_the_count_emulated(emu_lib):
    ac.check_split_dev("cpu", emu_lib, topks=(3,))


def test_split_dev_ignores_rows_beyond_the_count_topk9_emulated(emu_lib):
    ac.check_split_dev("cpu", emu_lib, topks=(9,), ns=(1, 256, None), splits=(3, 64))


def test_split_dev_ties_across_ranges_emulated(emu_lib):
    ac.check_split_dev_ties("cpu", emu_lib)


def test_split_dev_finds_appended_rows_emulated(emu_lib):
    ac.check_split_dev_after_append("cpu", emu_lib)


def test_pool_append_equals_concatenation_emulated(emu_lib):
    ac.check_pool_append("cpu", emu_lib)


def test_append_equals_fresh_scorer_emulated(emu_lib):
    ac.check_append_equals_fresh("tiny_seq_bn", -1, emu_lib)


def test_append_refusals(emu_lib):
    ac.check_append_refusals(-1, emu_lib)


def test_capacity_without_appends_equals_offline_emulated(emu_lib):
    ac.check_capacity_without_appends("tiny_seq_bn", -1, emu_lib, sizes=(7,), graph=False)
