"""The device-resident item catalogue on the CPU: rat_catalogue_expand, rat_topn_exclude and rat_topn_merge through the host-emulation
build (tests/emu), their ops wrappers, and OnlineScorer.set_catalogue / top_items / rank_items / top_catalogue on top of them.  The same
checks, with the shared bucket graphs, run on the MI355X in tests/test_gpu_catalogue.py; the corrupt-input check runs here only."""
import os
import sys

import pytest

import catalogue_cases as cc
from conftest import twin

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


def test_merge_inputs_reach_every_regime():
    cc.assert_merge_regimes()


def test_catalogue_expand_equals_numpy_emulated(emu_lib):
    cc.check_expand_kernel("cpu", emu_lib)


@pytest.mark.parametrize("set_name,which", [("eighths", None), ("special", None)] + [("eighths", w) for w in cc.EXCLUSIONS])
def test_topn_merge_equals_numpy_stable_sort_emulated(emu_lib, set_name, which):
    cc.check_merge_kernel("cpu", emu_lib, set_name, which)


def test_two_merges_equal_one_merge_over_the_union_emulated(emu_lib):
    cc.check_two_merges_equal_one("cpu", emu_lib)


def test_corrupt_arguments_stay_inside_the_buffers_emulated(emu_lib):
    cc.check_corrupt(emu_lib)


def test_abi_refusals_emulated(emu_lib):
    cc.check_abi_refusals("cpu", emu_lib)


def test_ops_refusals_emulated(emu_lib):
    cc.check_ops_refusals("cpu", emu_lib)


# (every form's launch chain runs below; the expansion and the merge do not depend on the form)
@pytest.mark.parametrize("form", ["window", twin("immutable"), twin("capacity")])
def test_top_and_rank_items_equal_candidates_over_host_rows_emulated(emu_lib, form):
    cc.check_items("tiny_seq_bn", -1, emu_lib, form, ns=(3,))


@pytest.mark.parametrize("form", ["window", twin("immutable"), twin("capacity")])
def test_top_catalogue_equals_numpy_over_score_requests_emulated(emu_lib, form):
    cc.check_top_catalogue("tiny_seq_bn", -1, emu_lib, form, variants=False)


# one pass over the whole catalogue (the default chunk too); item by item is 37 emulated forwards per call: on the GPU
@pytest.mark.parametrize("chunk", [cc.M_CAT, twin(1)])
def test_top_catalogue_in_one_pass_and_item_by_item_emulated(emu_lib, chunk):
    cc.check_top_catalogue("tiny_seq_bn", -1, emu_lib, "immutable", ns=(5,), chunks=(chunk,), variants=False)


def test_catalogue_refusals_reach_no_entry_point_emulated(emu_lib):
    cc.check_refusals(-1, emu_lib)


@pytest.mark.parametrize("form", cc.rq.FORMS)
def test_catalogue_launch_chain_emulated(emu_lib, form):
    cc.check_launch_chain(-1, emu_lib, form)
