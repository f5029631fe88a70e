"""Candidate retrieval through posting lists on the CPU: rat_bm25_topk_postings through the host-emulation build (tests/emu) against the
numpy restatement of rat_bm25_topk's contract, its ops wrapper, RetrievalIndex.build_postings / retrieve_shared, and postings=True of the
five OnlineScorer calls against postings=False.  The same checks, the whole matrix of (K, varying set, n_sorted) and the bucket graphs
run on the MI355X in tests/test_gpu_postings.py; the corrupt-input check runs here only."""
import os
import sys

import pytest

import postings_cases as pc
from conftest import FULL_CPU, twin

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


# every varying set with a tail of 50 rows, and one set at every n_sorted; the whole matrix runs on the GPU (and here with RAT_CPU_FULL=1)
@pytest.mark.parametrize("K", pc.KS)
def test_postings_kernel_equals_numpy_emulated(emu_lib, K):
    pc.check_kernel("cpu", emu_lib, K, full=FULL_CPU)


def test_ties_at_the_kth_place_between_context_and_posting_rows_emulated(emu_lib):
    pc.check_ties("cpu", emu_lib)


@pytest.mark.skipif(not FULL_CPU, reason="emulator repeat of a -m gpu test at another shape; RAT_CPU_FULL=1 runs it")
def test_long_posting_lists_emulated(emu_lib):
    pc.check_long_lists("cpu", emu_lib)


def test_build_postings_and_retrieve_shared_emulated(emu_lib):
    pc.check_index("cpu", emu_lib)


def test_corrupt_arguments_stay_inside_the_buffers_emulated(emu_lib):
    pc.check_corrupt(emu_lib)


def test_abi_refusals_emulated(emu_lib):
    pc.check_abi_refusals("cpu", emu_lib)


def test_ops_refusals_emulated(emu_lib):
    pc.check_ops_refusals("cpu", emu_lib)


# (one pass of 16 items per request here; one pass over all 37 and item by item — 37 emulated forwards per call — on the GPU)
@pytest.mark.parametrize("form,chunks", [("capacity", pc.CHUNKS[:1]), twin("immutable", pc.CHUNKS[:1]), twin("capacity", pc.CHUNKS[1:])])
def test_calls_with_postings_equal_calls_without_emulated(emu_lib, form, chunks):
    pc.check_scorer_calls("tiny_seq_bn", -1, emu_lib, form, chunks=chunks, light=not FULL_CPU)


def test_postings_refusals_reach_no_entry_point_emulated(emu_lib):
    pc.check_refusals(-1, emu_lib)


@pytest.mark.parametrize("form", ["capacity", twin("immutable")])
def test_postings_launch_chain_emulated(emu_lib, form):
    pc.check_launch_chain(-1, emu_lib, form, light=not FULL_CPU)
