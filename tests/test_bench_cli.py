"""bench.py's command line: a plain run measures the headline only and
--dump-outputs writes the last timed step's image; the rest sits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("grad_value", "grad_ms_per_step", "roofline", "hbm", "cpu_baseline", "secondary")


def test_options(monkeypatch):
    """--full is off and --dump-outputs unset by default; --steps and --warmup are taken as given."""
    pytest.importorskip("torch")
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "out")


@pytest.mark.gpu
def test_plain_run_dumps_last_timed_frame(tmp_path):
    """A plain run prints one result line without the --full figures, and
    DIR/hdr.npy is bitwise the frame of the last timed step (step K - 1 of the
    run's seed) rendered alone."""
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    steps, seed = 4, 3
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--seed",
                        str(seed), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["full"] is False and d["unit"] == "Msamples/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(512 * 512 * 64 / d["ms_per_step"] / 1e3, rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(out)) == ["hdr.npy"]
    got = np.load(out / "hdr.npy")
    assert got.dtype == np.float32 and got.shape == (512, 512, 3)

    import bench

    torch.cuda.set_device(0)
    cx = bench.Ctx(torch.device("cuda", 0), 1, 0)
    leg = bench.Leg(cx, bench.CORNELL, bench.W, bench.H, bench.SPP, bench.BOUNCES, seed=seed)
    leg.fwd(steps - 1)
    torch.cuda.synchronize()
    want = leg.hdr.cpu().numpy().reshape(got.shape)
    leg.close()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
