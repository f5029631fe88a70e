"""Neighbours restricted to rows equal on given columns on the CPU: rat_bm25_exact_count, rat_bm25_exact_plan and
rat_bm25_topk_split_exact through the host-emulation build (tests/emu), RetrievalIndex.retrieve(ids, same=...) and OnlineScorer.batch /
score / batch_rows / score_rows / evaluate_rows(..., same=...) on top of them.  The same checks, with 64 ranges and captured graphs, run
on the MI355X in tests/test_gpu_online_same.py; the corrupt-input check runs here only."""
import os
import sys

import pytest

import online_same_cases as sc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


# the emulator runs one OS thread per GPU thread: one range and three here, 64 ranges (empty ones among them) on the GPU
@pytest.mark.parametrize("same", sc.SAMES, ids=["one_column", "two_columns"])
@pytest.mark.parametrize("K", [3, 12])
@pytest.mark.parametrize("form", sc.FORMS)
def test_same_equals_the_offline_exact_match_path_emulated(emu_lib, form, K, same):
    sc.check_offline_parity(-1, emu_lib, form, K, same, splits=(1, 3))


# (K = 12, where every request of this pool lists, runs under horizons in one form here and in all of them on the GPU)
@pytest.mark.parametrize("same", sc.SAMES, ids=["one_column", "two_columns"])
@pytest.mark.parametrize("form", sc.FORMS)
def test_same_below_a_horizon_equals_the_numpy_restatement_emulated(emu_lib, form, same):
    sc.check_horizons(-1, emu_lib, form, 3, same)


def test_same_listing_below_a_horizon_topk12_emulated(emu_lib):
    sc.check_horizons(-1, emu_lib, "window", 12, sc.SAMES[1])


@pytest.mark.parametrize("form", sc.FORMS)
def test_batch_score_and_rows_with_same_emulated(emu_lib, form):
    sc.check_objects(-1, emu_lib, form)


def test_corrupt_headers_horizons_counts_flag_and_first_row_stay_inside_the_buffers_emulated(emu_lib):
    sc.check_corrupt(emu_lib)


def test_same_refusals(emu_lib):
    sc.check_refusals(-1, emu_lib)
