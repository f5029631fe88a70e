"""MaskedAveragePooling sequence fields on the MI355X (-m gpu): the product model against the reference's golden vectors in both
arithmetic modes, the table-gradient modes against each other, the captured training step against the eager one, and the kernels
against an fp64 statement (tests/test_avg_pooling.py runs the CPU part through the emulator)."""
import numpy as np
import pytest
import torch

import golden_cases as gc
import model_cases as mc
import pooling_cases as pc
import sparse_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip_lib():
    from rat_amd._lib import get_lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return get_lib()


@pytest.fixture(autouse=True)
def pooling_cases(monkeypatch):
    pc.register(monkeypatch)


def _with_arith(monkeypatch, arith):
    build = mc.build_model

    def build_model(case, gpu=-1, seed=None, **overrides):
        overrides.setdefault("arith", arith)
        return build(case, gpu, seed, **overrides)
    monkeypatch.setattr(mc, "build_model", build_model)


@pytest.mark.parametrize("name", pc.NAMES)
def test_init_matches_reference(name):
    mc.check_init(name, gpu=0)


@pytest.mark.parametrize("arith", ["f32", "auto"])
@pytest.mark.parametrize("name", pc.NAMES)
def test_eval_and_two_training_steps(name, arith, monkeypatch):
    _with_arith(monkeypatch, arith)
    mc.check_eval(name, gpu=0)
    mc.check_training(name, gpu=0)


@pytest.mark.parametrize("name", ["avgpool_tiny_seq_bn", "avgpool_northstar_shape", "avgpool_m1_tiny_seq"])
def test_train_step_replay_matches_the_reference_run(name):
    """steps 1-2 eager against the golden run, steps 3-5 hipGraph replays against the literal sequence on a twin model"""
    model = mc.check_train_step_api(name, gpu=0, steps=5)
    assert any(e[1] for e in model._step_graphs.values())


@pytest.mark.parametrize("name", ["avgpool_tiny_seq_bn", "avgpool_kkbox_shape", "avgpool_northstar_shape", "avgpool_m3_tiny_seq"])
def test_sorted_matches_atomic(name):
    sc.check_model_sorted_equals_atomic(name, 0)


@pytest.mark.parametrize("name", ["avgpool_tiny_seq_bn", "avgpool_kkbox_shape", "avgpool_northstar_shape"])
def test_sparse_equals_dense(name):
    sc.check_model_sparse_training(name, 0)


@pytest.mark.parametrize("mode", ["sorted", "sparse"])
def test_captured_step_with_sorted_and_sparse_table_gradients(mode):
    case = gc.case_by_name("avgpool_kkbox_shape")
    kw = dict(embedding_grad=mode)
    if mode == "sparse":
        kw["embedding_regularizer"] = 0.0
    a = mc.build_model(case, gpu=0, seed=1, **kw)
    b = mc.build_model(case, gpu=0, seed=1, **kw)
    mc.load_weights(a, case), mc.load_weights(b, case)
    b.use_graph = False
    batch = mc.batch_of(case)
    a.train(), b.train()
    for step in range(5):
        la, lb = float(a.train_step(batch)), float(b.train_step(batch))
        assert abs(la - lb) < 1e-6, (step, la, lb)
    assert any(e[1] for e in a._step_graphs.values())
    noise = mc.noise_tensors(a)
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        if k in noise or k.endswith(("running_mean", "num_batches_tracked")):
            continue
        x, y = va.detach().cpu().double(), vb.detach().cpu().double()
        bad = (x - y).abs() > 1.5e-5 + 3e-4 * y.abs()
        assert float(bad.double().mean()) < 1e-3 and float((x - y).abs().max()) <= 1.05e-2, (k, float((x - y).abs().max()))


def test_checkpoint_round_trip(tmp_path):
    """averaging adds no parameter: a trained model's .model file reloads into a fresh one with the same predictions"""
    case = gc.case_by_name("avgpool_tiny_seq_bn")
    a = mc.build_model(case, gpu=0, seed=1)
    mc.load_weights(a, case)
    batch = mc.batch_of(case)
    a.train()
    for _ in range(2):
        a.train_step(batch)
    path = str(tmp_path / "avg.model")
    a.save_weights(path)
    b = mc.build_model(case, gpu=0, seed=2)
    b.load_weights(path)
    a.eval(), b.eval()
    with torch.no_grad():
        ya, yb = a.forward(batch)["y_pred"], b.forward(batch)["y_pred"]
    assert torch.equal(ya, yb)


@pytest.mark.parametrize("d", [10, 40, 64])
def test_kernels_against_fp64(d, hip_lib):
    pc.check_pool_kernels(hip_lib, "cuda:0", d, B=7, T=5)


def test_rows64_non_temporal_gather_above_160_mb(hip_lib):
    pc.check_pool_gather_large(hip_lib, "cuda:0")
    torch.cuda.synchronize()
