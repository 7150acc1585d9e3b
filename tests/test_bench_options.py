"""bench.py's output dump (--dump-outputs), its --full legs and its argument checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restore(values, codes):
    """The frame as it was before the dump wrote its non-finite values as 0."""
    return np.select([codes == 1, codes == 2, codes == 3], [np.nan, np.inf, -np.inf], values).astype(np.float32)


def _frame_with_nonfinite(n, seed):
    fb = torch.rand(n, generator=torch.Generator().manual_seed(seed))
    fb[5], fb[7], fb[n // 2], fb[n - 1] = float("nan"), float("inf"), -float("inf"), float("nan")
    return fb


def _load_all(d):
    out = {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in out.values())
    return out


def test_dump_outputs_writes_the_whole_frame(tmp_path):
    W, H = 40, 24
    fb = _frame_with_nonfinite(H * W * 3, 1)
    bench.dump_outputs(str(tmp_path / "out"), fb, W, H)
    out = _load_all(tmp_path / "out")
    assert sorted(out) == ["framebuffer.npy", "framebuffer_nonfinite.npy"]
    a, codes = out["framebuffer.npy"], out["framebuffer_nonfinite.npy"]
    assert a.dtype == np.float32 and a.shape == (H, W, 3) and codes.shape == (H, W, 3)
    assert codes.reshape(-1)[[5, 7, H * W * 3 // 2, H * W * 3 - 1]].tolist() == [1, 2, 3, 1] and int((codes != 0).sum()) == 4
    assert np.array_equal(_restore(a, codes).reshape(-1), fb.numpy(), equal_nan=True)


def test_dump_outputs_samples_a_frame_above_the_limit(tmp_path):
    W, H = 4000, 1500  # 72 MB of float32
    fb = _frame_with_nonfinite(H * W * 3, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), fb, W, H)
    out = _load_all(tmp_path / "a")
    assert sorted(out) == ["framebuffer_sample.npy", "framebuffer_sample_nonfinite.npy", "framebuffer_sample_pixels.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in out) <= bench.DUMP_LIMIT_BYTES
    vals, codes, pix = out["framebuffer_sample.npy"], out["framebuffer_sample_nonfinite.npy"], out["framebuffer_sample_pixels.npy"]
    assert vals.dtype == np.float32 and pix.dtype == np.float64 and vals.shape == codes.shape == (len(pix), 3)
    assert np.all(np.diff(pix) > 0) and pix[0] >= 0 and pix[-1] < H * W
    assert np.array_equal(_restore(vals, codes), fb.numpy().reshape(-1, 3)[pix.astype(np.int64)], equal_nan=True)
    for f, a in out.items():  # the same pixels in every run
        assert np.array_equal(a, np.load(tmp_path / "b" / f))


def _bench(args, cwd):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, cwd=cwd, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_dump_is_the_timed_frame_and_full_adds_the_legs(pkg, tmp_path):
    """A plain run writes the frame of its timed steps (the frame --save-png tone-maps), as finite arrays, and runs none of the --full
    legs; a --full run with the same arguments dumps the identical frame and carries parity and the CPU baseline."""
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--spp-per-step", "4", "--width", "256", "--height", "144"]
    plain = _bench(common + ["--dump-outputs", str(tmp_path / "plain"), "--save-png", str(tmp_path / "plain.png")], ROOT)
    full = _bench(common + ["--full", "--cpu-spp", "1", "--dump-outputs", str(tmp_path / "full")], ROOT)
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0
    assert all(plain[k] is None for k in ("parity", "psnr_vs_cpu_db", "cpu_baseline", "cpu_baseline_8threads", "value_incl_d2h", "d2h_ms"))
    assert full["parity"]["psnr_db"] >= 60.0 and full["cpu_baseline"]["value"] > 0 and full["value_incl_d2h"] > 0
    a, b = _load_all(tmp_path / "plain"), _load_all(tmp_path / "full")
    assert sorted(a) == sorted(b) == ["framebuffer.npy", "framebuffer_nonfinite.npy"]
    assert a["framebuffer.npy"].dtype == np.float32 and a["framebuffer.npy"].shape == (144, 256, 3)
    assert all(np.array_equal(a[f], b[f]) for f in a)
    frame = _restore(a["framebuffer.npy"], a["framebuffer_nonfinite.npy"])
    assert np.array_equal(pkg.pngio.tonemap_u8(frame), pkg.pngio.read_png(str(tmp_path / "plain.png"))[:, :, :3])


def test_bench_rejects_zero_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode != 0 and "--steps must be >= 1" in p.stderr
