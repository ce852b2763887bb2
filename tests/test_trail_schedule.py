"""The trailing updates in tree order (SMLU_TRAIL_SPAN, SMLU_TRAIL_NS), on the CPU through
Plan.schedule_digest.

After j finished outer blocks a qualifying front updates only the blocks of its next lowbit(j)
block rows and columns, with the last lowbit(j) outer blocks as one k-range; every span-th boundary
updates everything right of it with k = span outer blocks.  Every build runs the builder's own
check (trail_check: each K_GEMMO task starts exactly where its blocks stand, every outer block and
the F22 update find their operands complete), and a failed check makes schedule_digest raise.
SMLU_TRAIL_NS is forced to its lower bound for tests (64) so that oracle-sized fronts qualify:
poisson3d_24 at OB = 128 has a root of 576 pivots (four full blocks and a 64-wide one) over fronts
with update rows; poisson3d_32 at OB = 128 a root of 1024 (eight blocks: boundaries with lowbit 1, 2
and 4).  At the shipped defaults none of the recorded digests moves."""
import numpy as np
import pytest

import smlu
from smlu import matrices as mats

import test_schedule_digest as tsd
from test_schedule_digest import KINDS, KNOBS, NCOUNT, NK, NS, NTAIL, SECTIONS

SPAN, MINNS, LSIDE = "SMLU_TRAIL_SPAN", "SMLU_TRAIL_NS", "SMLU_LSIDE_MIN"
NS_TEST = "64"   # the lower bound SMLU_TRAIL_NS accepts for tests (include/smlu.h)
FAC, GT = SECTIONS.index("fac"), SECTIONS.index("gt")
SOLVES = [SECTIONS.index(k) for k in ("fwd", "bwd", "fwdm", "bwdm", "comm")]

_plans = {}


def _plan(N):
    if N not in _plans:
        _plans[N] = smlu.Plan(mats.poisson3d(N))
    return _plans[N]


def _digest(monkeypatch, N, env, nparts=1, rank=0, flags=0):
    for k in KNOBS + (SPAN, MINNS, LSIDE):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = _plan(N).schedule_digest(nparts, rank, flags)
    assert d.size == NS + NCOUNT + NTAIL
    return d


def _fac_counts(d):
    return {KINDS[k]: int(d[NS + k]) for k in range(NK)}


def _tail(d):
    return d[NS + NCOUNT:].view(np.float64)   # gemm_flops, gemm22_flops, gemm_bytes, ...


@pytest.mark.parametrize("span", ["0", "2", "4"])
@pytest.mark.parametrize("N", [24, 32])
def test_forced_tree_order(monkeypatch, N, span):
    env = {"SMLU_OB": "128", MINNS: NS_TEST}
    on = _digest(monkeypatch, N, dict(env, **{SPAN: span}))       # builds: trail_check passed
    again = _digest(monkeypatch, N, dict(env, **{SPAN: span}))
    assert np.array_equal(on, again), "two builds of the same schedule differ"
    one = _digest(monkeypatch, N, dict(env, **{SPAN: "1"}))
    assert on[FAC] != one[FAC] and on[GT] != one[GT], "the knob does not act"
    assert _fac_counts(on) == _fac_counts(one)                    # GEMMO included
    for a, b in zip(_tail(on)[:2], _tail(one)[:2]):               # gemm_flops, gemm22_flops
        assert abs(a - b) <= 1e-12 * abs(b), (a, b)
    assert _tail(on)[2] < _tail(one)[2], "fewer C round trips: gemm_bytes must fall"
    # the solve sequences, their launch counts and the communication steps stay
    for i in SOLVES:
        assert on[i] == one[i], SECTIONS[i]
    assert np.array_equal(on[NS + NK:NS + NCOUNT], one[NS + NK:NS + NCOUNT])


def test_spans_differ_from_each_other(monkeypatch):
    # eight blocks: span 2, span 4 and the unbounded order are three schedules
    env = {"SMLU_OB": "128", MINNS: NS_TEST}
    fac = {s: int(_digest(monkeypatch, 32, dict(env, **{SPAN: s}))[FAC]) for s in ("0", "2", "4")}
    assert len(set(fac.values())) == 3, fac
    # a span that is no power of two is rounded down to one
    assert np.array_equal(_digest(monkeypatch, 32, dict(env, **{SPAN: "6"})),
                          _digest(monkeypatch, 32, dict(env, **{SPAN: "4"})))


def test_minimum_ns_is_held_at_1024(monkeypatch):
    # anything under 1024 other than the tests' bound is raised to 1024: the root of 576 stays out
    one = _digest(monkeypatch, 24, {"SMLU_OB": "128", SPAN: "1"})
    for v in ("0", "65", "512", "1023"):
        assert np.array_equal(_digest(monkeypatch, 24, {"SMLU_OB": "128", SPAN: "0", MINNS: v}), one), v
    # the 32^3 root (a 32 x 32 separator and more) qualifies at the clamp, and not at 4096
    one = _digest(monkeypatch, 32, {"SMLU_OB": "128", SPAN: "1"})
    assert _digest(monkeypatch, 32, {"SMLU_OB": "128", SPAN: "0", MINNS: "512"})[FAC] != one[FAC]
    assert np.array_equal(_digest(monkeypatch, 32, {"SMLU_OB": "128", SPAN: "0", MINNS: "4096"}), one)


@pytest.mark.parametrize("case", tsd.CASES, ids=[c[0] for c in tsd.CASES])
def test_span_one_and_the_defaults_are_the_recorded_schedule(case, monkeypatch):
    """Span 1 is the knob unset, and so are the shipped defaults with SMLU_TRAIL_NS at its clamp and
    any span: no front of these cases has 1024 pivots on one GPU.  This is what lets the golden file
    stand."""
    for k in (SPAN, MINNS):
        monkeypatch.delenv(k, raising=False)
    unset = tsd._digest(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    monkeypatch.setenv(SPAN, "1")
    monkeypatch.setenv(MINNS, NS_TEST)
    one = tsd._digest(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert np.array_equal(unset, one)
    monkeypatch.delenv(MINNS)
    for span in ("0", "2", "4", "8"):
        monkeypatch.setenv(SPAN, span)
        d = tsd._digest(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
        assert np.array_equal(unset, d), span


def test_full_candidate_panels_ignore_the_knobs(monkeypatch):
    on = _digest(monkeypatch, 24, {"SMLU_OB": "128", SPAN: "0", MINNS: NS_TEST}, flags=1)
    off = _digest(monkeypatch, 24, {"SMLU_OB": "128", SPAN: "1"}, flags=1)
    assert np.array_equal(on, off)


def test_partitioned_schedules_ignore_the_knobs(monkeypatch):
    for rank in (0, 1):
        on = _digest(monkeypatch, 24, {"SMLU_OB": "128", SPAN: "0", MINNS: NS_TEST}, nparts=2, rank=rank)
        off = _digest(monkeypatch, 24, {"SMLU_OB": "128", SPAN: "1"}, nparts=2, rank=rank)
        assert np.array_equal(on, off)


@pytest.mark.parametrize("N,span", [(24, "0"), (32, "4")])
def test_with_the_side_stream_both_checks_pass(monkeypatch, N, span):
    env = {"SMLU_OB": "128", LSIDE: "64"}
    both = _digest(monkeypatch, N, dict(env, **{SPAN: span, MINNS: NS_TEST}))
    side = _digest(monkeypatch, N, dict(env, **{SPAN: "1"}))
    assert both[FAC] != side[FAC]
    assert _fac_counts(both) == _fac_counts(side)
    for a, b in zip(_tail(both)[:2], _tail(side)[:2]):
        assert abs(a - b) <= 1e-12 * abs(b), (a, b)
