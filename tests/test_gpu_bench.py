"""bench.py on the GPU at a small size (12^3, in process): a plain run times exactly --steps
refactors and prints the headline line without the side measurements; --dump-outputs writes what
the last timed step computed (float64 .npy, under 64 MB), and those arrays are the factorization
of that step's matrix; --full (here without its CPU and C1/C2/C5 legs) adds the solves."""
import json
import os
import sys

import numpy as np
import pytest

SIDE, STEPS, WARMUP = 12, 2, 1


def _run_bench(monkeypatch, capsys, *extra):
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                                      "--side", str(SIDE), *extra])
    bench.main()
    cap = capsys.readouterr()
    lines = [ln for ln in cap.out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, cap.out   # one JSON line
    return json.loads(lines[0]), cap.err


@pytest.mark.gpu
def test_plain_run_and_dump(gpu, monkeypatch, capsys, tmp_path):
    from smlu import matrices as mats
    out = tmp_path / "dump"
    rec, err = _run_bench(monkeypatch, capsys, "--dump-outputs", str(out))
    assert rec["steps"] == STEPS and rec["warmup"] == WARMUP and rec["full"] is False
    assert err.count(": step ") == STEPS and err.count(": warmup ") == WARMUP   # one log line per refactor
    assert rec["unit"] == "nnz(L+U)/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(rec["config"]["nnzLU"] / (rec["ms_per_step"] * 1e-3))
    for k in ("cpu_baseline", "configs", "solve_ms", "solve_8rhs_ms", "solve_residual", "refactor_host_values_ms"):
        assert k not in rec, k
    assert "ordering_compare" not in rec["config"]

    names = sorted(os.listdir(out))
    assert names == ["factor_sample.npy", "factor_sample_offsets.npy", "x.npy"]
    arr = {f[:-4]: np.load(out / f) for f in names}
    assert sum(os.path.getsize(out / f) for f in names) < 64e6
    for a in arr.values():
        assert a.dtype == np.float64 and a.size > 0 and np.isfinite(a).all()
    # the last timed step's matrix and the dump's right-hand side, from their seeds
    A = mats.poisson3d(SIDE)
    n = A.shape[0]
    A.data[mats.diag_positions(A)] += np.random.default_rng(47 + WARMUP + STEPS - 1).random(n)
    b = np.random.default_rng(5).random(n)
    x = arr["x"]
    assert x.shape == (n,)
    # the reference's sparse tolerance (1e-12): a backward-stable solve of this diagonally dominant
    # matrix leaves a residual of a few eps relative to |b|
    assert np.abs(A @ x - b).max() / np.abs(b).max() < 1e-12
    fs, off = arr["factor_sample"], arr["factor_sample_offsets"]
    assert off.size >= 1 and (off >= 0).all() and off.size <= fs.size <= (1 << 21)
    assert np.abs(fs).max() > 0


@pytest.mark.gpu
def test_factor_sample_reads_factor_values(gpu):
    """Single-double runs: every sampled value is the factor store's entry at its offset, inside
    some front's L panel or U12 block, and the sample is the same on a second call."""
    import bench
    import smlu
    from smlu import matrices as mats
    F = smlu.ParallelSparseLU(mats.poisson3d(SIDE), device=0)
    try:
        store, off = F.front_store()
        w = np.diff(F.fronts()["first"])
        inside = np.zeros(store.size, bool)
        for (lo, uo, _, m), ns in zip(off, w):
            inside[lo:lo + m * ns] = True
            if m > ns:
                inside[uo:uo + ns * (m - ns)] = True
        v, o = bench.factor_sample(F, total=300, chunk=1)
        o = o.astype(np.int64)
        assert v.size == o.size == 300 and len(set(o.tolist())) > 250
        assert inside[o].all() and np.array_equal(v, store[o])
        v2, o2 = bench.factor_sample(F, total=300, chunk=1)
        assert np.array_equal(v, v2) and np.array_equal(o, o2)
        v64, o64 = bench.factor_sample(F, total=640, chunk=64)
        assert o64.size == 10 and o64.size <= v64.size <= 640
        assert np.array_equal(v64[:1], store[o64[:1].astype(np.int64)])
    finally:
        F.close()


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements(gpu, monkeypatch, capsys):
    rec, _ = _run_bench(monkeypatch, capsys, "--full", "--no-cpu", "--no-configs")
    assert rec["full"] is True and rec["steps"] == STEPS
    assert rec["solve_ms"] > 0 and rec["solve_8rhs_ms"] > 0 and rec["refactor_host_values_ms"] > 0
    assert rec["solve_residual"] < 1e-12
