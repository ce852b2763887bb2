"""The static schedule, pinned on the CPU: section hashes of every launch sequence, task array, work
list and communication step (smlu_plan_schedule_digest) against tests/golden/schedule_digests.json.

A refactor of the schedule builder must leave every hash as recorded; a change that means to move
the schedule regenerates the file and says so:

    python tests/test_schedule_digest.py --record

The file was first recorded from the one-function builder that schedule_build.cpp replaced (the
digest hooked into its host-only exit), and has not been regenerated since.  It holds, per case, the hashes and per-kind launch counts as integers and the
statistics (GEMM flops / bytes, allocation sizes) as doubles; the doubles are compared to 1e-12
relative, not hashed, so a change of summation order does not fail the test."""
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "schedule_digests.json")
RECORD_CMD = "python tests/test_schedule_digest.py --record"

SECTIONS = ["nodes", "fac", "fwd", "bwd", "fwdm", "bwdm", "segments", "comm", "ilist", "xt", "ae", "xc", "ft",
            "gptr", "gent", "gt", "st_tasks", "ur_tasks", "scalars"]
KINDS = ["EXTADD", "FRONT_LDS", "PANEL", "TRSMU", "TRSML", "GEMM", "FWD", "BWD", "FWDG", "TRIF", "BWDU", "TRIB",
         "GEMM22", "LASWP", "STEPTRSM", "GEMMU", "GEMMO", "TRIINV", "BWDU12C", "VCOPY", "FWDT", "BWDT", "SWEEPF",
         "SWEEPB", "UROWS", "FWDP"]
NS, NK = len(SECTIONS), len(KINDS)
NCOUNT = 3 * NK + 2          # launches per kind of fac, fwd, bwd; exchange and broadcast steps
NTAIL = 8                    # gemm_flops, gemm22_flops, gemm_bytes, host_bytes[0..4]

KNOBS = ("SMLU_OB", "SMLU_T128MIN", "SMLU_SMALLK", "SMLU_FULLPIV_NS", "SMLU_SOLVE_STEPS")


def _matrix(name):
    from smlu import matrices as mats
    if name == "random_dominant_200":
        z = np.load(os.path.join(HERE, "golden", "random_dominant_200.npz"), allow_pickle=False)
        n = int(z["A_indptr"].size - 1)
        return sp.csc_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=(n, n))
    kind, N = name.split("_")
    return {"poisson3d": mats.poisson3d, "poisson2d": mats.poisson2d}[kind](int(N))


def _cases():
    """(id, matrix, ordering, nparts, rank, flags, env)"""
    out = []
    for m in ("poisson3d_12", "poisson3d_24", "poisson2d_64", "random_dominant_200"):
        for flags in (0, 1, 2, 4, 8):
            out.append((f"{m}-f{flags}", m, "auto", 1, 0, flags, {}))
    for k, v in (("SMLU_OB", "128"), ("SMLU_OB", "512"), ("SMLU_SMALLK", "0"), ("SMLU_T128MIN", "1"),
                 ("SMLU_SOLVE_STEPS", "1"), ("SMLU_FULLPIV_NS", "0")):
        out.append((f"poisson3d_24-{k}={v}", "poisson3d_24", "auto", 1, 0, 0, {k: v}))
    for np_ in (2, 8):
        for r in range(np_):
            out.append((f"poisson3d_40-nd-{np_}r{r}", "poisson3d_40", "nd", np_, r, 0, {}))
    return out


CASES = _cases()
_plans = {}


def _plan(matrix, ordering):
    import smlu
    key = (matrix, ordering)
    if key not in _plans:
        _plans[key] = smlu.Plan(_matrix(matrix), ordering=ordering)
    return _plans[key]


def _digest(case, setenv, delenv):
    _, matrix, ordering, nparts, rank, flags, env = case
    for k in KNOBS:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    d = _plan(matrix, ordering).schedule_digest(nparts, rank, flags)
    assert d.size == NS + NCOUNT + NTAIL, d.size
    return d


def _split(d):
    return ([int(v) for v in d[:NS]], [int(v) for v in d[NS:NS + NCOUNT]],
            [float(v) for v in d[NS + NCOUNT:].view(np.float64)])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_schedule_matches_recorded(case, golden, monkeypatch):
    d = _digest(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    again = _digest(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert np.array_equal(d, again), f"{case[0]}: two builds of the same schedule differ"
    assert case[0] in golden, f"{case[0]} not recorded; run: {RECORD_CMD}"
    hashes, counts, tail = _split(d)
    rec = golden[case[0]]
    diff = [SECTIONS[i] for i in range(NS) if f"{hashes[i]:016x}" != rec["hashes"][i]]
    assert not diff, (f"{case[0]}: schedule sections {diff} differ from the recorded schedule; if the change "
                      f"is intended, regenerate with: {RECORD_CMD}")
    assert counts == rec["counts"], f"{case[0]}: launch counts differ; regenerate with: {RECORD_CMD}"
    for name, a, b in zip(("gemm_flops", "gemm22_flops", "gemm_bytes", "device_bytes", "store_bytes",
                           "scratch_bytes", "staging_bytes", "host_staging_bytes"), tail, rec["doubles"]):
        assert abs(a - b) <= 1e-12 * abs(b), (case[0], name, a, b)


def test_cases_cover_every_launch_kind_and_step_type(golden):
    """The recorded set exercises every launch kind and both kinds of communication step."""
    seen = np.zeros(NK, np.int64)
    steps = np.zeros(2, np.int64)
    for c in CASES:
        cnt = np.asarray(golden[c[0]]["counts"], np.int64)
        seen += cnt[:3 * NK].reshape(3, NK).sum(axis=0)
        steps += cnt[3 * NK:]
    missing = [KINDS[k] for k in range(NK) if seen[k] == 0]
    assert not missing, f"no case schedules a launch of kind {missing}"
    assert steps[0] > 0 and steps[1] > 0, steps


def record():
    out = {}
    for case in CASES:
        d = _digest(case, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
        hashes, counts, tail = _split(d)
        out[case[0]] = {"hashes": [f"{h:016x}" for h in hashes], "counts": counts, "doubles": tail}
    for k in KNOBS:
        os.environ.pop(k, None)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, len(out), "cases")


if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    sys.path.insert(0, os.path.join(ROOT, "sharedmemsparselu.jl_amd"))
    if "--record" in sys.argv:
        record()
    else:
        sys.exit(f"usage: {RECORD_CMD}")
