"""Kernel-level parity of the SyncBN and owner-exchange kernels on CPU: the kernel sources through the host emulation (tests/emu) at the
small shapes of tests/dp_cases.py, one process playing every rank.  The GPU twin, with the complete matrix, is
tests/test_gpu_dp_kernels.py."""
import os
import sys

import pytest
from conftest import twin

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))

import dp_cases as dc  # noqa: E402
from rat_amd._lib import RatLib  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build_emu
    return RatLib(build_emu.build())


@pytest.mark.parametrize("case", dc.SYNC_BN_CORE + [twin(c) for c in dc.SYNC_BN_TWIN], ids=dc.sync_bn_id)
def test_sync_bn_chain_against_float64_batch_norm_of_the_whole_batch(emu, case):
    dc.check_sync_bn(emu, "cpu", *case)


def test_sync_bn_on_shards_that_are_tensors_of_their_own(emu):
    dc.check_sync_bn(emu, "cpu", [7, 6], 13, "sigmoid", use_offsets=False)


@pytest.mark.parametrize("name", list(dc.OWNER_CHAIN_CORE))
def test_owner_exchange_chain_bit_for_bit(emu, name):
    dc.check_owner_chain_case(emu, "cpu", name)


@pytest.mark.parametrize("case", dc.OWNER_COUNTS_CASES)
def test_owner_counts(emu, case):
    dc.check_owner_counts(emu, "cpu", case)


@pytest.mark.parametrize("name", list(dc.OWNER_SCATTER_CORE))
def test_owner_scatter_on_hand_built_lists(emu, name):
    dc.check_owner_scatter(emu, "cpu", *dc.OWNER_SCATTER_CORE[name])
