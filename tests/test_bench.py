"""bench.py's --dump-outputs: the sample of the train state it writes (CPU) and a plain run that dumps (GPU)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_fixed_sample_within_size_limit(tmp_path, monkeypatch):
    """Two dumps of the same state are identical file for file, float32, and at LAP-3B size the four state samples stay
    under the 64 MB the option promises."""
    import bench
    from lap_amd.config import get_config
    from lap_amd.params import ParamStore

    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    ps = ParamStore(get_config("debug").model, "cpu")
    ps.init_random(0)
    state = types.SimpleNamespace(model=types.SimpleNamespace(ps=ps))
    info = {"loss": torch.tensor(1.5), "grad_norm": torch.tensor(2.0)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), state, info)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["adam_m.npy", "adam_v.npy", "ema.npy", "grad_norm.npy", "loss.npy", "params.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert np.load(tmp_path / "a" / "params.npy").shape == (sum(min(ps.master[u.name].numel(), bench.DUMP_SAMPLES_PER_UNIT) for u in ps.units),)

    full = ParamStore(get_config("lap_bench").model, device="meta")
    n = sum(min(full.master[u.name].numel(), bench.DUMP_SAMPLES_PER_UNIT) for u in full.units)
    assert 4 * n * 4 < 64e6


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(hip, tmp_path):
    """A plain run prints the headline line without the --full figures and dumps the last timed step: `loss.npy` is the
    line's `final_loss`."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "debug", "--steps", "2", "--warmup", "1",
                        "--batch", "2", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and not {"roofline", "serve", "cpu_baseline"} & set(d)
    loss = np.load(out / "loss.npy")
    assert loss.dtype == np.float32 and round(float(loss), 5) == d["final_loss"]
    for n in ("params", "adam_m", "adam_v", "ema"):
        a = np.load(out / f"{n}.npy")
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all()
