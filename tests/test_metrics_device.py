"""Evaluation metrics on the device, on the CPU: rat_eval_metrics through the host-emulation build (tests/emu), ops.eval_metrics,
metrics.device_metrics / gauc_score, BaseModel(device_metrics=, group_id=) and OnlineScorer.evaluate_rows(group=, device=) /
metrics_rows on top of it.  The same checks, with n up to 2^20, run on the MI355X in tests/test_gpu_metrics.py; the guard-region check
runs here only."""
import os
import sys

import numpy as np
import pytest

import metrics_cases as mx

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old
    mx.report()


@pytest.mark.parametrize("n", mx.NS_EMU)
def test_logloss_auc_gauc_equal_the_host_references_emulated(emu_lib, n):
    mx.check_parity(-1, emu_lib, n)


@pytest.mark.parametrize("n", [65, 1000, 4097])
def test_row_order_changes_nothing_but_logloss_rounding_emulated(emu_lib, n):
    mx.check_row_order(-1, emu_lib, n)


def test_undefined_metrics_are_nan_with_a_status_bit_and_a_value_error_emulated(emu_lib):
    mx.check_status(-1, emu_lib)


def test_abi_refusals_launch_nothing_emulated(emu_lib):
    mx.check_abi_refusals(-1, emu_lib)


def test_hostile_labels_and_group_ids_stay_inside_the_buffers_emulated(emu_lib):
    mx.check_guards(emu_lib)


@pytest.mark.parametrize("form", ["immutable", "capacity", "window"])
def test_evaluate_rows_and_metrics_rows_emulated(emu_lib, form):
    mx.check_scorer(-1, emu_lib, form, n=120, rows=np.arange(30, 110, 5))      # (one OS thread per GPU thread: 16 rows here, 80 on the GPU)


def test_evaluate_generator_device_metrics_and_gauc_emulated(emu_lib):
    mx.check_generator(-1, emu_lib)


def test_construction_refusals(emu_lib, monkeypatch):
    mx.check_construction_refusals(-1, emu_lib, monkeypatch)
