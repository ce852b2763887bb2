"""The schedule of the F22 gather (large fronts' F22 assembled inside the Schur GEMM's C prologue),
on the CPU through Plan.schedule_digest.

Every build here runs the builder's own checks -- each inverse map inverts its row map, and no F22
launch writes a child F22 block it gathers from -- and a failed check makes schedule_digest raise.
The knobs are forced (SMLU_F22_GATHER_NU=1 with SMLU_T128MIN=1, SMLU_SMALLK=0) so that the fronts
of oracle-sized matrices qualify; at the defaults none of the recorded digests moves
(tests/test_schedule_digest.py)."""
import numpy as np
import pytest

import smlu
from smlu import matrices as mats

from test_schedule_digest import KNOBS, NCOUNT, NS, NTAIL, SECTIONS

GATHER_KNOBS = ("SMLU_F22_GATHER_NU", "SMLU_F22_GATHER_CH")
FORCED = {"SMLU_T128MIN": "1", "SMLU_SMALLK": "0"}
FAC, XC = SECTIONS.index("fac"), SECTIONS.index("xc")

_plans = {}


def _plan(N):
    if N not in _plans:
        _plans[N] = smlu.Plan(mats.poisson3d(N))
    return _plans[N]


def _digest(monkeypatch, N, env, nparts=1, rank=0, flags=0):
    for k in KNOBS + GATHER_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = _plan(N).schedule_digest(nparts, rank, flags)
    assert d.size == NS + NCOUNT + NTAIL
    return d


@pytest.mark.parametrize("ch", ["8", "64"])
@pytest.mark.parametrize("N", [24, 32])
def test_forced_gather_builds_and_acts(monkeypatch, N, ch):
    env = dict(FORCED, SMLU_F22_GATHER_NU="1", SMLU_F22_GATHER_CH=ch)
    d = _digest(monkeypatch, N, env)
    again = _digest(monkeypatch, N, env)
    assert np.array_equal(d, again), "two builds of the same schedule differ"
    base = _digest(monkeypatch, N, FORCED | {"SMLU_F22_GATHER_NU": "0"})
    assert d[FAC] != base[FAC] and d[XC] != base[XC], "the knob does not act"
    # the launches themselves stay: same count per kind, same GEMM tasks
    assert np.array_equal(d[NS:NS + NCOUNT], base[NS:NS + NCOUNT])
    assert d[SECTIONS.index("gt")] == base[SECTIONS.index("gt")]


def test_child_cap_changes_the_fused_set(monkeypatch):
    # 24^3 has fronts with more than 8 contributing children: the two caps fuse different sets
    d8 = _digest(monkeypatch, 24, dict(FORCED, SMLU_F22_GATHER_NU="1", SMLU_F22_GATHER_CH="8"))
    d64 = _digest(monkeypatch, 24, dict(FORCED, SMLU_F22_GATHER_NU="1", SMLU_F22_GATHER_CH="64"))
    assert d8[XC] != d64[XC]


def test_gather_off_is_the_default_schedule(monkeypatch):
    # poisson3d_24's largest nu is 387 < 512: the default build fuses nothing, as does NU=0
    off = _digest(monkeypatch, 24, {"SMLU_F22_GATHER_NU": "0"})
    default = _digest(monkeypatch, 24, {})
    assert np.array_equal(off, default)
    off = _digest(monkeypatch, 24, FORCED | {"SMLU_F22_GATHER_NU": "0"})
    default = _digest(monkeypatch, 24, FORCED)
    assert np.array_equal(off, default)


@pytest.mark.parametrize("nparts,flags", [(2, 0), (1, 4)])
def test_partitioned_and_pair_schedules_ignore_the_knob(monkeypatch, nparts, flags):
    forced = _digest(monkeypatch, 24, dict(FORCED, SMLU_F22_GATHER_NU="1", SMLU_F22_GATHER_CH="64"), nparts, 0, flags)
    plain = _digest(monkeypatch, 24, FORCED, nparts, 0, flags)
    assert np.array_equal(forced, plain)
