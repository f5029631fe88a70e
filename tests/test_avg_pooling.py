"""MaskedAveragePooling sequence fields (sequence.py:21-29) on the CPU: the product model against golden vectors the real reference
produced with averaged fields (tests/golden/make_golden_pooling.py), and the kernels against an fp64 statement — through the
host-emulation build of the same kernel sources (tests/emu).  tests/test_gpu_avg_pooling.py runs the same on the MI355X."""
import os
import sys

import pytest

import model_cases as mc
import pooling_cases as pc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    import build_emu
    import rat_amd._lib as L
    old = L._default
    L._default = L.RatLib(build_emu.build())
    yield L._default
    L._default = old


@pytest.fixture(autouse=True)
def pooling_cases(monkeypatch):
    pc.register(monkeypatch)


@pytest.mark.parametrize("name", ["avgpool_tiny_seq_bn", "avgpool_m0_tiny_seq", "avgpool_m1_tiny_seq", "avgpool_m3_tiny_seq"])
def test_init_and_eval_match_the_reference(name):
    mc.check_init(name, gpu=-1)
    mc.check_eval(name, gpu=-1)


# the emulator runs one OS thread per GPU thread: one training case here, every case in the GPU suite
@pytest.mark.parametrize("name", ["avgpool_tiny_seq_bn"])
def test_training_matches_the_reference(name):
    mc.check_training(name, gpu=-1)


# d = 10: scalar gather, d = 40: vectorised gather, d = 64: the rows64 gather (its non-temporal form: tests/test_gpu_avg_pooling.py)
@pytest.mark.parametrize("d", [10, 40, 64])
def test_kernels_against_fp64(d, emu_lib):
    pc.check_pool_kernels(emu_lib, "cpu", d)


def test_feature_map_encoders():
    from rat_amd.features import FieldInfo
    spec = {"type": "sequence", "index": [2, 3, 4], "vocab_size": 9, "max_len": 3}
    assert FieldInfo("s", dict(spec, encoder="MaskedAveragePooling")).pooling == "average"
    assert FieldInfo("s", dict(spec, encoder="MaskedSumPooling")).pooling == "sum"
    assert FieldInfo("c", {"type": "categorical", "index": 0, "vocab_size": 5}).pooling == "sum"
    for enc in (None, "null", "MaskedMaxPooling"):
        with pytest.raises(NotImplementedError, match="sequence encoder"):
            FieldInfo("s", dict(spec, encoder=enc))
