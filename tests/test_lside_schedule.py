"""The schedule of the L rows below an outer block (SMLU_LSIDE_MIN: a step's L-row solve and
in-block update cut at the block's last row, the lower parts as side launches), on the CPU through
Plan.schedule_digest.

Every build here runs the builder's own checks -- each side task starts at or below its outer
block's end, no main-stream task of a front writes rows its pending side launches own, and a join
comes before the next level -- and a failed check makes schedule_digest raise.  The knob is forced
to 64 so that the fronts of oracle-sized matrices qualify (poisson3d_24: root 576 = 384 + 192, and
fronts with update rows below it); at the default none of the recorded digests moves."""
import numpy as np
import pytest

import smlu
from smlu import matrices as mats

import test_schedule_digest as tsd
from test_schedule_digest import KINDS, KNOBS, NCOUNT, NK, NS, NTAIL, SECTIONS

KNOB = "SMLU_LSIDE_MIN"
FAC = SECTIONS.index("fac")

_plans = {}


def _plan(N):
    if N not in _plans:
        _plans[N] = smlu.Plan(mats.poisson3d(N))
    return _plans[N]


def _digest(monkeypatch, N, env, nparts=1, rank=0, flags=0):
    for k in KNOBS + (KNOB,):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = _plan(N).schedule_digest(nparts, rank, flags)
    assert d.size == NS + NCOUNT + NTAIL
    return d


def _fac_counts(d):
    return {KINDS[k]: int(d[NS + k]) for k in range(NK)}


def _flops(d):
    return d[NS + NCOUNT:].view(np.float64)[:2]   # gemm_flops, gemm22_flops


@pytest.mark.parametrize("ob", [None, "128"])
def test_forced_split_adds_only_step_launches(monkeypatch, ob):
    # OB = 128: ns = 576 gives four full blocks and a partial one
    env = {} if ob is None else {"SMLU_OB": ob}
    on = _digest(monkeypatch, 24, dict(env, **{KNOB: "64"}))
    again = _digest(monkeypatch, 24, dict(env, **{KNOB: "64"}))
    assert np.array_equal(on, again), "two builds of the same schedule differ"
    off = _digest(monkeypatch, 24, dict(env, **{KNOB: "0"}))
    assert on[FAC] != off[FAC], "the knob does not act"
    c_on, c_off = _fac_counts(on), _fac_counts(off)
    assert c_on["TRSML"] > c_off["TRSML"] and c_on["GEMM"] > c_off["GEMM"], (c_on, c_off)
    for k in KINDS:
        if k not in ("TRSML", "GEMM"):
            assert c_on[k] == c_off[k], (k, c_on[k], c_off[k])
    # the solves' launch counts and the communication steps stay
    assert np.array_equal(on[NS + NK:NS + NCOUNT], off[NS + NK:NS + NCOUNT])
    for a, b in zip(_flops(on), _flops(off)):
        assert abs(a - b) <= 1e-12 * abs(b), (a, b)


def test_full_candidate_panels_ignore_the_knob(monkeypatch):
    on = _digest(monkeypatch, 24, {KNOB: "64"}, flags=1)
    off = _digest(monkeypatch, 24, {KNOB: "0"}, flags=1)
    assert np.array_equal(on, off)


def test_partitioned_schedules_ignore_the_knob(monkeypatch):
    for rank in (0, 1):
        on = _digest(monkeypatch, 24, {KNOB: "64"}, nparts=2, rank=rank)
        off = _digest(monkeypatch, 24, {KNOB: "0"}, nparts=2, rank=rank)
        assert np.array_equal(on, off)


@pytest.mark.parametrize("case", tsd.CASES, ids=[c[0] for c in tsd.CASES])
def test_default_knob_is_the_schedule_with_the_knob_off(case, monkeypatch):
    # every matrix of the digest test: at most 192 rows lie below a block on one GPU, under any default
    monkeypatch.delenv(KNOB, raising=False)
    default = tsd._digest(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    monkeypatch.setenv(KNOB, "0")
    off = tsd._digest(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert np.array_equal(default, off)
