"""Ranking metrics on the device, on the CPU: rat_eval_rank_metrics through the host-emulation build (tests/emu), ops.eval_rank_metrics,
metrics.ndcg_score / mrr_score / hitrate_score and the names NDCG(k=K) / MRR(k=K) / HitRate(k=K), BaseModel(metrics=, group_id=) and
OnlineScorer.evaluate_rows(cutoffs=) / rank_metrics_rows on top of it.  The same checks, with n up to 2^20, run on the MI355X in
tests/test_gpu_rank_metrics.py; the guard-region check, the host functions and the sklearn cross-check of the reference run here only."""
import os
import sys

import numpy as np
import pytest

import rank_metrics_cases as rk

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old
    rk.report()


def test_the_loop_reference_equals_sklearn_on_tie_free_inputs():
    rk.check_reference_against_sklearn()


def test_host_functions_equal_the_loop_reference():
    rk.check_host_functions()


@pytest.mark.parametrize("n", rk.NS_EMU)
def test_ndcg_mrr_hitrate_equal_the_loop_reference_emulated(emu_lib, n):
    rk.check_parity(-1, emu_lib, n)


@pytest.mark.parametrize("n", [65, 1000, 4097])
def test_eight_cutoffs_in_one_call_equal_eight_calls_emulated(emu_lib, n):
    rk.check_eight_cutoffs(-1, emu_lib, n)


@pytest.mark.parametrize("n", [65, 1000, 4097])
def test_ties_keep_input_order_and_tie_free_rows_may_be_permuted_emulated(emu_lib, n):
    rk.check_tie_rule(-1, emu_lib, n)


def test_undefined_metrics_are_nan_with_a_status_bit_and_a_value_error_emulated(emu_lib):
    rk.check_status(-1, emu_lib)


def test_abi_refusals_launch_nothing_emulated(emu_lib):
    rk.check_abi_refusals(-1, emu_lib)


def test_hostile_labels_and_group_ids_stay_inside_the_buffers_emulated(emu_lib):
    rk.check_guards(emu_lib)


@pytest.mark.parametrize("form", ["immutable", "capacity", "window"])
def test_evaluate_rows_cutoffs_and_rank_metrics_rows_emulated(emu_lib, form):
    rk.check_scorer(-1, emu_lib, form, n=120, rows=np.arange(30, 110, 5))      # (one OS thread per GPU thread: 16 rows here, 80 on the GPU)


def test_evaluate_generator_ranking_names_emulated(emu_lib):
    rk.check_generator(-1, emu_lib)


def test_construction_refusals(emu_lib):
    rk.check_construction_refusals(-1, emu_lib)
