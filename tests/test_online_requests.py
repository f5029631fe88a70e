"""Requests that share a launch on the CPU: rat_bm25_query_prepare_seg through the host-emulation build (tests/emu),
RetrievalIndex.retrieve(ids, request_offsets) and OnlineScorer.batch_requests / score_requests on top of it.  The same checks, with
captured bucket graphs, run on the MI355X in tests/test_gpu_online_requests.py; the corrupt-input check runs here only."""
import os
import sys

import pytest

import online_requests_cases as qc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


# the emulator runs one OS thread per GPU thread: one range and three here, more ranges and the 300-row pool on the GPU
@pytest.mark.parametrize("form", qc.FORMS)
def test_segmented_retrieve_equals_requests_sent_alone_emulated(emu_lib, form):
    qc.check_retrieval_parity("tiny_seq_bn", -1, emu_lib, form, splits=(1, 3))


@pytest.mark.parametrize("form", qc.FORMS)
def test_batch_and_score_requests_equal_requests_sent_alone_emulated(emu_lib, form):
    qc.check_assembly_and_prediction("tiny_seq_bn", -1, emu_lib, form)


def test_segmented_prepare_corrupt_first_row_stays_inside_the_buffers_emulated(emu_lib):
    qc.check_seg_corrupt(emu_lib)


def test_request_refusals(emu_lib):
    qc.check_request_refusals(-1, emu_lib)
