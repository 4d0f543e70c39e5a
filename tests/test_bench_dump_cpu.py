"""bench.py --dump-outputs on the CPU: dump_outputs() over host tensors standing in for the device buffers (whole batch, and the seeded
sample a batch over the size bound falls back to), and the argument checks that run before any device is touched."""
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT


def _buffers(n, rs):
    from aim_amd import capi
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    res["score"] = np.arange(n) * 3 - 5
    res["idx"] = np.arange(n) + 7
    res["max_operations"] = 2 * rs
    res["begin_offset"] = 4
    res["end_offset"] = 4 + np.arange(n) % 20
    res["status"][::97] = 1
    ops = np.full((n, 2 * rs), ord("M"), dtype=np.uint8)          # bytes outside [begin, end) are unspecified: must not be dumped
    ops[:, 4:24] = np.frombuffer(b"MMXIMDDMMMMIMMXMMMMM", dtype=np.uint8)
    d_res = torch.from_numpy(np.frombuffer(res.tobytes() + bytes(64), dtype=np.uint8).copy())
    d_ops = torch.from_numpy(np.concatenate([ops.reshape(-1), np.zeros(64, dtype=np.uint8)]))
    return res, ops, d_res, d_ops


def test_dump_outputs_whole_batch_and_seeded_sample(tmp_path, monkeypatch):
    import bench
    from aim_amd import capi
    n, rs = 1000, 16
    res, ops, d_res, d_ops = _buffers(n, rs)
    for bound in (10 ** 9, 20000):
        monkeypatch.setattr(bench, "DUMP_BYTES", bound)
        dumps = []
        for k in range(2):
            d = tmp_path / ("%d_%d" % (bound, k))
            bench.dump_outputs(str(d), d_res, d_ops, n, capi.RESULT_DTYPE, rs)
            assert sum(f.stat().st_size for f in d.iterdir()) <= bound
            dumps.append({f.stem: np.load(f) for f in d.glob("*.npy")})
        a = dumps[0]
        assert sorted(a) == sorted(capi.RESULT_DTYPE.names + ("ops",))
        for name in a:
            assert a[name].dtype in (np.float32, np.float64) and np.array_equal(a[name], dumps[1][name]), name
        rows = a["idx"].astype(np.int64) - 7
        assert len(rows) == n if bound > 10 ** 6 else 0 < len(rows) < n
        assert np.all(np.diff(rows) > 0)
        for name in capi.RESULT_DTYPE.names:
            assert np.array_equal(a[name], res[name][rows]), name
        for j, i in enumerate(rows):
            b, e = res["begin_offset"][i], res["end_offset"][i]
            assert np.array_equal(a["ops"][j, b:e], ops[i, b:e]) and not a["ops"][j, :b].any() and not a["ops"][j, e:].any()


def test_dump_outputs_score_only_is_exact(tmp_path):
    """{idx, score} results: float32 where every value is exact in it (AIM_SCORE_FAILED = -2^31 is), float64 where one is not."""
    import bench
    from aim_amd import capi
    res = np.zeros(5, dtype=capi.RESULT8_DTYPE)
    res["idx"] = [0, 1, 2, 3, (1 << 24) + 1]
    res["score"] = [0, 7, -(1 << 31), 5, 2]
    bench.dump_outputs(str(tmp_path), torch.from_numpy(np.frombuffer(res.tobytes(), dtype=np.uint8).copy()), None, 5, capi.RESULT8_DTYPE, 112)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["idx.npy", "score.npy"]
    idx, score = np.load(tmp_path / "idx.npy"), np.load(tmp_path / "score.npy")
    assert idx.dtype == np.float64 and score.dtype == np.float32
    assert np.array_equal(idx, res["idx"]) and np.array_equal(score, res["score"])


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr
