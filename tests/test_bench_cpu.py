"""bench.py without a GPU: the --dump-outputs writer (file layout, dtypes, the sample counts of the accumulation target, the size cap) and
the options of a plain run."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench():
    # bench.py sets HSA_ENABLE_IPC_MODE_LEGACY for its own process at import; keep this process's environment as it was
    saved = os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    yield mod
    if saved is None:
        os.environ.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)
    else:
        os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = saved


def _frame(H, W, seed=3):
    rng = np.random.default_rng(seed)
    frame = rng.random((H, W, 4), dtype=np.float32)
    frame[..., 3] = rng.integers(0, 5000, (H, W)).astype(np.uint32).view(np.float32)   # channel 3: sample count as uint32 bits
    return frame


def test_dump_outputs_writes_the_whole_frame(bench, tmp_path):
    frame = _frame(9, 16)
    bench.dump_outputs(str(tmp_path / "out"), frame)
    rgb = np.load(tmp_path / "out" / "framebuffer_rgb.npy")
    samples = np.load(tmp_path / "out" / "framebuffer_samples.npy")
    assert sorted(os.listdir(tmp_path / "out")) == ["framebuffer_rgb.npy", "framebuffer_samples.npy"]
    assert rgb.dtype == np.float32 and rgb.shape == (9, 16, 3)
    assert np.array_equal(rgb.view(np.uint32), frame[..., :3].view(np.uint32))
    assert samples.dtype == np.float64 and samples.shape == (9, 16)
    assert np.array_equal(samples, frame[..., 3].view(np.uint32).astype(np.float64))


def test_dump_outputs_samples_a_frame_over_the_cap(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    H, W = 40, 64
    frame = _frame(H, W)
    bench.dump_outputs(str(tmp_path / "a"), frame)
    bench.dump_outputs(str(tmp_path / "b"), frame)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["framebuffer_rgb.npy", "framebuffer_samples.npy", "pixel_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 4096 + 3 * 128   # + the .npy headers
    for f in files:   # a fixed sample: the same pixels every time
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and idx.size > 0 and np.all(np.diff(idx) > 0) and idx[-1] < H * W
    k = idx.astype(np.int64)
    rgb = np.load(tmp_path / "a" / "framebuffer_rgb.npy")
    samples = np.load(tmp_path / "a" / "framebuffer_samples.npy")
    assert rgb.dtype == np.float32 and rgb.shape == (k.size, 3)
    assert np.array_equal(rgb, frame.reshape(H * W, 4)[k, :3])
    assert np.array_equal(samples, frame[..., 3].view(np.uint32).reshape(H * W)[k].astype(np.float64))


def test_the_default_frame_is_dumped_whole(bench):
    assert 1920 * 1080 * (3 * 4 + 8) <= bench.DUMP_LIMIT_BYTES <= 64 << 20


def test_a_plain_run_is_headline_only(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    args = bench.parse_args()
    assert args.steps == 7 and args.warmup == 3 and not args.full and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse_args()
    assert args.full and args.dump_outputs == "d"
