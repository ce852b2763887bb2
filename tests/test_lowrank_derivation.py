"""What tests/test_gpu_lowrank.py relies on, shown on the CPU with the NumPy restatement
(tests/_lowrank_ref.py): on every (input, k, kind, op) the GPU test runs, refinement on the updated
system reaches berr <= 2^-51 (stop 1) within 3 corrections, and on the goldens the forward-error check
is never skipped: eta * cond_inf(A') stays below 1/2."""
import numpy as np
import pytest

import _lowrank_ref as R
from _diag_ref import GOLDEN


@pytest.mark.parametrize("name,k,kind,op", R.gpu_cases())
def test_restatement_stops_on_the_target(name, k, kind, op):
    ref = R.reference(name, k, kind, op)
    print(f"{name} k={k} {kind} op={op}: steps {ref['steps']} stop {ref['stop']} berrs "
          + " ".join(f"{b:.2e}" for b in ref["berrs"]))
    assert ref["stop"] == 1
    assert ref["steps"] <= 3
    assert np.isfinite(ref["x"]).all()


@pytest.mark.parametrize("name,k,kind,op", [c for c in R.gpu_cases() if c[0] in GOLDEN])
def test_forward_check_is_never_skipped(name, k, kind, op):
    P = R.problem(name)
    U, V, _ = R.update(name, k, kind)
    ref = R.reference(name, k, kind, op)
    A2 = P["A"].toarray() + U @ V.T
    M = A2 if op == "N" else A2.T
    kappa = float(np.linalg.cond(M, np.inf))
    eta = R.normwise(P["A"], U, V, ref["x"], P["b"], op, anorm=float(np.abs(M).sum(axis=1).max()))
    xs = R.polished_solve(M, P["b"])
    err = float(np.abs(ref["x"] - xs).max() / np.abs(xs).max())
    print(f"{name} k={k} {kind} op={op}: eta {eta:.2e} kappa {kappa:.2e} forward {err:.2e}")
    assert eta * kappa < 0.5
    assert err <= 2 * eta * kappa / (1 - eta * kappa)
