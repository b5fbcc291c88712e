"""bench.py --dump-outputs: the files a run writes for a given batch of
verdicts (CPU; the verdict arrays are stand-ins for the engine's)."""
import os

import numpy as np

import bench


class _Arr:
    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a


class _Verdicts:
    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        self.status = _Arr(rng.integers(0, 8, n).astype(np.uint8))
        self.wait_ms = _Arr((rng.integers(0, 500, n) * (rng.random(n) < 0.02)).astype(np.int32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_small_batch_is_whole(tmp_path):
    v = _Verdicts(1000, 1)
    bench.dump_outputs(str(tmp_path / "a"), v, 1, 0)
    d = _load(tmp_path / "a")
    assert sorted(d) == ["sample_index", "status", "status_counts", "wait_ms", "wait_ms_sum"]
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert np.array_equal(d["sample_index"], np.arange(1000))
    assert np.array_equal(d["status"], v.status.a) and np.array_equal(d["wait_ms"], v.wait_ms.a)
    assert np.array_equal(d["status_counts"], np.bincount(v.status.a, minlength=256))
    assert d["wait_ms_sum"][0] == v.wait_ms.a.sum()


def test_dump_large_batch_is_a_fixed_sample(tmp_path):
    n = bench.DUMP_SAMPLE + 12345
    v = _Verdicts(n, 2)
    bench.dump_outputs(str(tmp_path / "a"), v, 1, 0)
    bench.dump_outputs(str(tmp_path / "b"), v, 1, 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a)                      # the same events every run
    idx = a["sample_index"].astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE and (np.diff(idx) >= 0).all() and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(a["status"], v.status.a[idx]) and np.array_equal(a["wait_ms"], v.wait_ms.a[idx])
    assert a["status_counts"].sum() == n
    size = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert size <= 64 * 1000 * 1000


def test_dump_names_carry_the_rank_of_a_sharded_run(tmp_path):
    bench.dump_outputs(str(tmp_path), _Verdicts(100, 3), 2, 1)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}_rank1.npy" for k in
                                                  ("sample_index", "status", "status_counts", "wait_ms", "wait_ms_sum"))
