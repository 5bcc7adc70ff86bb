"""bench.py's plain run and ``--dump-outputs``: the plain line carries the
headline fields and none of the ``--full`` side measurements, and the dumped
array is what the timed path returns for the seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_output_whole_and_sampled(tmp_path):
    """Below its share an array is written whole (float32, logical order, also
    from a permuted view); above it, the same seeded sample every time."""
    t = torch.arange(2 * 3 * 4 * 5, dtype=torch.float64).reshape(2, 3, 4, 5)
    nhwc = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # same values, other strides
    e = bench.dump_output(str(tmp_path), "whole", nhwc, 0, share=t.numel() * 4)
    got = np.load(tmp_path / "whole.npy")
    assert e == {"file": "whole.npy", "shape": [2, 3, 4, 5], "dtype": "float32"}
    assert got.dtype == np.float32 and np.array_equal(got, t.numpy().astype(np.float32))

    e1 = bench.dump_output(str(tmp_path), "a", nhwc, 0, share=40)
    e2 = bench.dump_output(str(tmp_path), "b", t, 1, share=40)
    assert e1["sampled"] == 10 and e1["shape"] == [2, 3, 4, 5] and e2["file"] == "b.rank1.npy"
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.rank1.npy")
    assert a.dtype == np.float32 and a.shape == (10,)
    assert np.array_equal(a, b)                      # same indices, whatever the strides
    assert np.all(np.diff(a) >= 0) and a.min() >= 0 and a.max() < t.numel()   # values are the indices


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_paths_output(tmp_path):
    """The plumbing of a plain run: line fields, and that the dump is the last
    timed step's output for the seeded inputs, in float32 and logical element
    order.  The expected array comes from the same CorrBlock1D, so this does
    not check the kernels' values; the golden and oracle tests do that."""
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "realtime",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-9)   # batch 1, one GPU
    for side in ("kernel_ms", "roofline", "latency_ms", "e2e", "backward", "cpu_baseline", "config4_network"):
        assert side not in line
    assert sorted(os.listdir(out_dir)) == ["corr_out.npy"]
    assert line["dumped"]["corr_out"]["file"] == "corr_out.npy" and "sampled" not in line["dumped"]["corr_out"]

    from raft_stereo_amd import CorrBlock1D
    cfg = bench.CONFIGS["realtime"]
    B, D, H, W1, W2, L, r, iters, _ = cfg
    f1, f2, coords = bench.make_inputs(cfg, torch.device("cuda", 0), seed=1)
    with torch.no_grad():
        blk = CorrBlock1D(f1, f2, num_levels=L, radius=r, low_latency=True)
        want = blk(coords[iters - 1])
    got = np.load(out_dir / "corr_out.npy")
    assert got.dtype == np.float32 and list(got.shape) == line["dumped"]["corr_out"]["shape"]
    assert np.array_equal(got, want.float().cpu().numpy(), equal_nan=True)
