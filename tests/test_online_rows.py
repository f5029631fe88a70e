"""A pool that looks at itself on the CPU: rat_bm25_topk_split_before and rat_pool_gather_rows through the host-emulation build
(tests/emu), RetrievalIndex.retrieve(ids, before=...) and OnlineScorer.batch_rows / score_rows / evaluate_rows on top of them.  The same
checks, with 64 ranges and captured graphs, run on the MI355X in tests/test_gpu_online_rows.py; the corrupt-input check runs here only."""
import os
import sys

import pytest

import online_rows_cases as rc

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
@pytest.mark.parametrize("K", [3, 12])
@pytest.mark.parametrize("form", rc.FORMS)
def test_horizon_scan_equals_topk_over_truncated_copies_emulated(emu_lib, form, K):
    rc.check_scan_parity(-1, emu_lib, form, K, splits=(1, 3))


@pytest.mark.parametrize("form", rc.FORMS)
def test_rows_behind_the_horizon_never_win_emulated(emu_lib, form):
    rc.check_scan_poisoned(-1, emu_lib, form, 3, splits=(1, 3))


def test_gather_rows_equals_numpy_emulated(emu_lib):
    rc.check_gather("cpu", emu_lib)


def test_corrupt_headers_indices_and_horizons_stay_inside_the_buffers_emulated(emu_lib):
    rc.check_corrupt(emu_lib)


@pytest.mark.parametrize("form", rc.FORMS)
def test_batch_score_and_evaluate_rows_see_only_older_rows_emulated(emu_lib, form):
    rc.check_scores(-1, emu_lib, form)


def test_rows_refusals(emu_lib):
    rc.check_rows_refusals(-1, emu_lib)
