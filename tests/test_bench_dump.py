"""bench.py --dump-outputs on the CPU: factor_sample's index arithmetic against a fake factor store
(fronts with L panels M x ns and U12 blocks ns x nu at padded offsets, the store's values equal to
their own offsets), dump_outputs' files, and which side measurements each combination of --full,
--no-cpu, --no-configs and --check-single turns on (side_legs)."""
import ctypes
import os

import numpy as np
import pytest

NS = 50


class _FakeStore:
    def __init__(self, seed=1, empty=False):
        rng = np.random.default_rng(seed)
        self.w = np.zeros(NS, np.int64) if empty else rng.integers(1, 40, NS)
        nu = rng.integers(0, 300, NS)
        nu[-1] = 0                                    # the root front has no U12
        self.M = self.w + nu
        sizes = np.stack([self.M * self.w, self.w * nu], 1).ravel()
        offs = np.concatenate([[0], np.cumsum(sizes + rng.integers(0, 7, sizes.size))])   # padded blocks
        self.store = np.arange(max(int(offs[-1]), 1), dtype=np.float64)
        Loff, Uoff = offs[0:-1:2], offs[1:-1:2].copy()
        self.blocks = [(int(Loff[s]), int(Loff[s] + self.M[s] * self.w[s])) for s in range(NS)]
        self.blocks += [(int(Uoff[s]), int(Uoff[s] + self.w[s] * nu[s])) for s in range(NS) if nu[s]]
        Uoff[nu == 0] = -1
        self.table = np.stack([Loff, Uoff, np.full(NS, -1), self.M], 1).astype(np.int64)
        self.copies = []

    # the two C-ABI calls factor_sample makes
    def smlu_dev_front_offsets(self, h, out):
        a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_int64)), (4 * NS,))
        a[:] = self.table.ravel()
        return 0

    def smlu_dev_copy(self, h, which, off, cnt, out, ln):
        assert which == 0 and cnt > 0 and 0 <= off and off + cnt <= self.store.size
        self.copies.append((off, cnt))
        a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_double)), (cnt,))
        a[:] = self.store[off:off + cnt]
        return 0

    # the handle's side
    _h = None

    def stat(self, key):
        assert key == "nsuper"
        return float(NS)

    def fronts(self):
        return {"first": np.concatenate([[0], np.cumsum(self.w)])}


@pytest.fixture
def fake(monkeypatch):
    from smlu import _lib as C
    S = _FakeStore()
    monkeypatch.setattr(C, "lib", lambda: S)
    return S


def test_factor_sample_runs_stay_inside_blocks(fake):
    import bench
    chunk = 64
    v, o = bench.factor_sample(fake, total=64 * chunk, chunk=chunk)
    assert o.size == 64 == len(fake.copies)
    assert [c[0] for c in fake.copies] == o.astype(np.int64).tolist()
    cut = 0
    for off, cnt in fake.copies:
        inside = [(lo, hi) for lo, hi in fake.blocks if lo <= off < hi]
        assert len(inside) == 1, off                      # starts in exactly one L panel or U12 block
        assert cnt == min(chunk, inside[0][1] - off)      # a whole run, or cut at the block's end
        cut += cnt < chunk
    assert cut >= 1                                       # the cut is exercised
    assert np.array_equal(v, np.concatenate([np.arange(off, off + cnt, dtype=np.float64)
                                             for off, cnt in fake.copies]))
    v2, o2 = bench.factor_sample(fake, total=64 * chunk, chunk=chunk)
    assert np.array_equal(v, v2) and np.array_equal(o, o2)   # the same entries on every call
    v3, _ = bench.factor_sample(fake, total=64 * chunk, chunk=chunk, seed=48)
    assert not np.array_equal(v, v3)


def test_factor_sample_weights_fronts_by_size(fake):
    """Single-double runs drawn over the concatenated blocks: every value is a block entry, and a
    block's share of the sample follows its share of the factor values."""
    import bench
    v, o = bench.factor_sample(fake, total=20000, chunk=1)
    assert v.size == 20000 and np.array_equal(v, o)
    sizes = np.array([hi - lo for lo, hi in fake.blocks], float)
    hits = np.array([((v >= lo) & (v < hi)).sum() for lo, hi in fake.blocks], float)
    assert hits.sum() == v.size                            # no value from the padding
    share, want = hits / v.size, sizes / sizes.sum()
    # binomial: 5 standard deviations of each block's count, plus one count
    assert (np.abs(share - want) <= 5 * np.sqrt(want * (1 - want) / v.size) + 1 / v.size).all()


def test_factor_sample_small_store_and_empty_store(monkeypatch):
    import bench
    from smlu import _lib as C
    S = _FakeStore()
    monkeypatch.setattr(C, "lib", lambda: S)
    total = sum(hi - lo for lo, hi in S.blocks)
    v, o = bench.factor_sample(S, total=1 << 30, chunk=4096)   # asks for more than there is
    assert o.size == total // 4096 and v.size <= total
    E = _FakeStore(empty=True)
    monkeypatch.setattr(C, "lib", lambda: E)
    with pytest.raises(AssertionError, match="no factor values"):
        bench.factor_sample(E)


def test_dump_outputs_files(fake, tmp_path):
    import bench
    x = np.linspace(0.0, 1.0, 1000)
    bench.dump_outputs(str(tmp_path / "d"), fake, x, partitioned=False, rank=0)
    names = sorted(os.listdir(tmp_path / "d"))
    assert names == ["factor_sample.npy", "factor_sample_offsets.npy", "x.npy"]
    arr = {f[:-4]: np.load(tmp_path / "d" / f) for f in names}
    assert all(a.dtype == np.float64 for a in arr.values())
    assert np.array_equal(arr["x"], x)
    assert arr["factor_sample_offsets"].size == len(fake.copies)
    bench.dump_outputs(str(tmp_path / "p"), fake, x, partitioned=True, rank=0)   # partitioned: x alone
    assert sorted(os.listdir(tmp_path / "p")) == ["x.npy"]
    bench.dump_outputs(str(tmp_path / "r1"), fake, x, partitioned=True, rank=1)  # rank 0 writes
    assert not (tmp_path / "r1").exists()


@pytest.mark.parametrize("argv, world, partitioned, want", [
    ([], 1, False, (False, False, False)),                       # a plain run: no side leg
    (["--gpus", "1", "--steps", "20", "--warmup", "5"], 1, False, (False, False, False)),
    (["--dump-outputs", "d"], 1, False, (False, False, False)),  # a dump is not a side measurement
    (["--full"], 1, False, (True, True, True)),                  # --full alone: every leg
    (["--full", "--no-cpu"], 1, False, (True, False, True)),
    (["--full", "--no-configs"], 1, False, (True, True, False)),
    (["--no-cpu"], 1, False, (True, False, True)),               # naming a leg to leave out asks for the rest
    (["--no-cpu", "--no-configs"], 1, False, (True, False, False)),
    (["--full", "--gpus", "2"], 2, True, (True, False, False)),  # CPU and config legs: one GPU only
    (["--gpus", "2", "--check-single"], 2, True, (True, False, False)),
    (["--gpus", "2", "--replicas", "--check-single"], 2, False, (False, False, False)),
    (["--check-single"], 1, False, (False, False, False)),
])
def test_side_legs(argv, world, partitioned, want):
    import bench
    assert bench.side_legs(bench.parse_args(argv), world, partitioned) == want
