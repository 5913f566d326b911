"""bench.py --dump-outputs on the CPU: arrays within their share of the 64 MB are written whole as float32, a larger one becomes the same
seeded sample of its pixels every time."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frame(h, w):
    """float64 frame whose w channel is the pixel's index (exact in float32 up to 3840x2160)"""
    a = np.zeros((h, w, 4))
    a[..., 0] = 0.25
    a[..., 3] = np.arange(h * w).reshape(h, w)
    return a


def _dump(out_dir, h, w):
    code = ("import sys, bench\nfrom tests.test_bench_dump import frame\n"
            "bench.dump_outputs(sys.argv[1], {'hdr': frame(%d, %d), 'result': frame(%d, %d) * 2})\n" % (h, w, h, w))
    p = subprocess.run([sys.executable, "-c", code, str(out_dir)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return {n: np.load(os.path.join(out_dir, n + ".npy")) for n in ("hdr", "result")}


def test_dump_outputs_whole_and_sampled(tmp_path):
    d = _dump(tmp_path / "a", 1080, 1920)
    assert d["hdr"].dtype == np.float32 and np.array_equal(d["hdr"], frame(1080, 1920))     # 33 MB, within its 48 MB share: whole
    res = d["result"]                                                                       # 33 MB over its 12 MB share: sampled
    assert res.dtype == np.float32 and res.shape == (750_000, 4)
    idx = res[:, 3].astype(np.int64) // 2
    assert (np.diff(idx) > 0).all() and np.array_equal(res, (frame(1080, 1920) * 2).reshape(-1, 4)[idx])
    assert np.array_equal(_dump(tmp_path / "b", 1080, 1920)["result"], res)                # the same pixels again
    big = _dump(tmp_path / "c", 2160, 3840)
    assert big["hdr"].shape == (3_000_000, 4) and big["result"].shape == (750_000, 4)
    assert sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c")) <= 64_000_000
