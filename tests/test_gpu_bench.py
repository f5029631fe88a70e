"""bench.py --dump-outputs on the GPU (-m gpu): in graph mode the timed steps are hipGraph replays, and the loss train_step returns is
the graph's static output — copied after the timed region's synchronize and before the eager kernel-timing pass (--full) reuses it.
The same K steps run eagerly (--no-graph: no replay, no kernel pass) must return the same loss, and one more timed step (a plain run:
no kernel pass, no per-kernel figures) must not."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    # --warmup 5: graph_warmup + 2, so that the capture happens inside the warm-up and graph and eager runs take the same steps
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--warmup", "5", "--no-extras",
                        "--no-cpu-baseline", "--dump-outputs", str(out_dir)] + list(extra), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert os.listdir(str(out_dir)) == ["loss.npy"]
    return line, np.load(str(out_dir / "loss.npy"))


def test_dump_of_a_graph_replay_is_the_last_timed_step(tmp_path):
    graph, lg = _bench(tmp_path / "graph", "--steps", "3", "--full")
    eager, le = _bench(tmp_path / "eager", "--steps", "3", "--no-graph")
    later, l4 = _bench(tmp_path / "later", "--steps", "4")
    assert graph["step_mode"]["graph"] is True and graph["step_mode"]["graph_prepare_steps"] == 0 and eager["step_mode"]["graph"] is False
    assert graph["kernels"] and "eager_instrumented_ms_per_step" in graph["step_mode"]
    assert later["step_mode"]["graph"] is True and "kernels" not in later and "eager_instrumented_ms_per_step" not in later["step_mode"]
    assert lg.dtype == np.float32 and lg.shape == (1,) and np.isfinite(lg).all()
    np.testing.assert_allclose(lg, le, rtol=2e-5, atol=0)
    assert not np.allclose(lg, l4, rtol=1e-3, atol=0)
