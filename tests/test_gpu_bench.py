"""bench.py's plain run: the result line holds the headline figures and none
of the `--full` measurements, `--steps` sets the number of timed steps, and
`--dump-outputs` writes what the timed call returns for the seeded frames --
checked against the same call made here; the row sampling of a large dump is
checked on the host.  Small frames: the arguments, the line and the files are
under test, not the rate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT

N, W, H, STEPS = 3, 320, 213, 2
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "stage_ms_per_step", "host_fetch", "cpu_baseline", "configs", "keypoint_stages")


def test_dump_row_sample_is_fixed():
    """The rows of a sampled dump depend on the result count and the cap alone."""
    sys.path.insert(0, ROOT)
    import bench
    assert np.array_equal(bench.sample_rows(np.random.default_rng(0), 7, 7), np.arange(7))
    a = bench.sample_rows(np.random.default_rng(0), 1000, 50)
    assert a.shape == (50,) and np.all(np.diff(a) > 0) and 0 <= a[0] and a[-1] < 1000
    assert np.array_equal(a, bench.sample_rows(np.random.default_rng(0), 1000, 50))
    # the caps keep a dump of any size under 64 MB: f32 keypoints + f64 rows, f32 descriptors + f64 rows
    assert bench.DUMP_KEYPOINT_ROWS * (5 * 4 + 8) + bench.DUMP_DESCRIPTOR_ROWS * (128 * 4 + 8) + (1 << 20) < 64e6


@pytest.mark.gpu
def test_plain_run_line_and_dump(pkg, ctx, tmp_path):
    import synth
    import torch
    dump = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                          "--warmup", "1", "--frames", str(N), "--width", str(W), "--height", str(H),
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for k in HEADLINE:
        assert k in d, k
    for k in FULL_ONLY:
        assert k not in d, k
    assert (d["steps"], d["warmup"], d["n_gpus"]) == (STEPS, 1, 1)
    assert (d["unit"], d["dtype"], d["higher_is_better"]) == ("keypoints/s", "f32", True)
    assert d["ms_per_step"] > 0

    t = synth.frames_torch(N, W, H, seed0=0, device="cuda")
    torch.cuda.synchronize()
    offs, res = ctx.sift_batch_device(t.data_ptr(), N, W, H, t.stride(1), t.stride(0), fetch=True)
    n = int(offs[-1])
    assert n > 0
    # value = keypoints of all timed steps / their time
    assert d["value"] == pytest.approx(n * STEPS / (d["ms_per_step"] * 1e-3 * STEPS), rel=1e-9)
    got = {f[:-4]: np.load(dump / f) for f in sorted(os.listdir(dump))}
    assert sorted(got) == ["descriptor_rows", "descriptors", "keypoints", "offsets"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["offsets"], offs.astype(np.float64))
    assert np.array_equal(got["keypoints"].view(np.uint32), res.keypoints_array.view(np.uint32))
    assert np.array_equal(got["descriptor_rows"], np.arange(n))  # under the sampling threshold: every row
    assert np.array_equal(got["descriptors"], res.descriptors.astype(np.float32))
