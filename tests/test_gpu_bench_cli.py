"""bench.py's plain run: the headline line, ``--steps`` and ``--dump-outputs``.

A plain run (no ``--full``) times exactly ``--steps`` steps and prints only
the headline line; ``--dump-outputs DIR`` writes what the last timed step
computed as float32 ``DIR/<name>.npy``.  Run in this process (``bench.main``
with patched arguments) so the test pays for two small runs, not two
interpreter starts.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

STEPS, WARMUP = 3, 2
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "d3_kernels", "bf16", "step_roofline", "gather_roofline", "dist_check",
             "synthetic_5k", "parity", "cpu_baseline", "losses_mean")


def _plain_run(monkeypatch, capsys, out_dir):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                                      "--dataset", "32", "--dump-outputs", str(out_dir)])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_run_line_and_dump(monkeypatch, capsys, tmp_path):
    line, a = _plain_run(monkeypatch, capsys, tmp_path / "a")
    for k in HEADLINE:
        assert k in line, k
    assert [k for k in FULL_ONLY if k in line] == []  # those take runs of their own: --full
    assert line["unit"] == "meshes/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: 16 meshes per step
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 16) < 1e-6 * 16
    nv = line["config"]["template_vertices"]
    assert set(a) == {"recon", "z", "mulv", "losses", "loss_acc", "grad", "params", "exp_avg", "exp_avg_sq"}
    assert a["recon"].shape == (16, nv, 3) and a["z"].shape == (16, 75) and a["losses"].shape == (5,)
    assert a["params"].shape == a["grad"].shape == a["exp_avg"].shape
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # --steps really sets the timed steps: the accumulator counts the capture's
    # one real step, the warm-up and the timed steps, nothing else
    assert a["loss_acc"][5] == 1 + WARMUP + STEPS
    assert np.abs(a["grad"]).max() > 0 and np.abs(a["recon"]).max() > 0
    # same arguments, same inputs: the data set, initial weights, batch order
    # and noise are seeded, and every reduction of the step has a fixed order
    # (no floating-point atomics), so a second run reproduces every bit
    _, b = _plain_run(monkeypatch, capsys, tmp_path / "b")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
