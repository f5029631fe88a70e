"""Kernel-level parity of the SyncBN and owner-exchange kernels on the MI355X (-m gpu): the complete matrix of tests/dp_cases.py — the
per-rank head shape of the 8-rank benchmark, ragged shards, every activation, and the row-list sizes past the grid caps of
rat_owner_pack / rat_owner_unpack / rat_owner_scatter — in one process on one device.  The emulator twin is tests/test_dp_kernels.py."""
import pytest
import torch

import dp_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from rat_amd._lib import get_lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return get_lib()


@pytest.mark.parametrize("case", dc.SYNC_BN_CORE + dc.SYNC_BN_TWIN + dc.SYNC_BN_GPU_ONLY, ids=dc.sync_bn_id)
def test_sync_bn_chain_against_float64_batch_norm_of_the_whole_batch(lib, case):
    dc.check_sync_bn(lib, "cuda", *case)


def test_sync_bn_on_shards_that_are_tensors_of_their_own(lib):
    dc.check_sync_bn(lib, "cuda", [7, 6], 13, "sigmoid", use_offsets=False)


@pytest.mark.parametrize("name", list(dc.OWNER_CHAIN_CORE) + list(dc.OWNER_CHAIN_GPU_ONLY))
def test_owner_exchange_chain_bit_for_bit(lib, name):
    dc.check_owner_chain_case(lib, "cuda", name)


@pytest.mark.parametrize("case", dc.OWNER_COUNTS_CASES)
def test_owner_counts(lib, case):
    dc.check_owner_counts(lib, "cuda", case)


@pytest.mark.parametrize("name", list(dc.OWNER_SCATTER_CORE) + list(dc.OWNER_SCATTER_GPU_ONLY))
def test_owner_scatter_on_hand_built_lists(lib, name):
    dc.check_owner_scatter(lib, "cuda", *{**dc.OWNER_SCATTER_CORE, **dc.OWNER_SCATTER_GPU_ONLY}[name])
