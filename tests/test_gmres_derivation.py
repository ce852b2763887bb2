"""Conditions on the inputs of tests/test_gpu_gmres.py, established on the CPU with the NumPy
restatement of the algorithm (tests/_gmres_ref.py); nothing here runs the code under test.

Right-preconditioned GMRES on A' = A + E with M = A works on A' A^-1 = I + E A^-1.  With
rho = ||E A^-1||_2 the polynomial (1 - z)^k, which is 1 at 0, gives (-E A^-1)^k there, so the relative
residual after k steps is at most rho^k and the count to rtol at most ceil(log rtol / log rho).
(Transposed: A'^T A^-T = I + E^T A^-T, rho = ||E^T A^-T||_2.)  For the shifted Poisson inputs
lambda_min(A) >= 1, so ||A^-1||_2 <= 1 and rho <= ||E||_2 <= || |E| ||_inf <= delta || |A| ||_inf by hand
(|E| is symmetric, so its 2-norm is at most its inf-norm)."""
import math

import numpy as np
import pytest

import _gmres_ref as G


def rho_dense(name, op):
    P = G.problem(name)
    A, A2 = P["A"].toarray(), P["A2"].toarray()
    EAinv = (A2 - A) @ np.linalg.inv(A)
    if op != "N":
        EAinv = (A2 - A).T @ np.linalg.inv(A).T
    return float(np.linalg.norm(EAinv, 2))


@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("name", list(G.SMALL))
def test_small_inputs_converge_like_rho_to_the_k(name, op):
    rho = rho_dense(name, op)
    R = G.reference(name, op, 30)
    print(f"{name} op={op}: rho {rho:.3e} rtol {G.rtol_of(name):.3e} iters {R['iters']} hist "
          + " ".join(f"{v:.1e}" for v in R["hist"]))
    assert R["converged"] and R["cycles"] == 1
    if name == "fe_8":
        assert rho > 1.0     # no bound from rho here; it converges all the same
        assert R["iters"] <= 10
        return
    assert rho < 1.0
    for k, v in enumerate(R["hist"]):
        assert v <= rho ** k, (k, v, rho ** k)
    assert R["iters"] <= max(1, math.ceil(math.log(G.rtol_of(name)) / math.log(rho)))


@pytest.mark.parametrize("name", list(G.LARGE))
def test_shifted_poisson_bound_by_hand(name):
    P = G.problem(name)
    A = P["A"]
    assert abs(A - A.T).max() == 0.0
    width = float(abs(A).sum(axis=1).max())
    assert width == (13.0 if name.startswith("poisson3d") else 9.0)
    # Gershgorin: every eigenvalue of the Poisson part is >= 0, so lambda_min(A) >= 1
    d = A.diagonal()
    off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
    assert (d - off >= 1.0).all()
    rho = P["delta"] * width
    assert rho < 1.0
    for op in ["N"] + (["T"] if name in G.TRANS_TOO else []):
        R = G.reference(name, op, 30)
        print(f"{name} op={op}: rho <= {rho:.3f} iters {R['iters']} hist " + " ".join(f"{v:.1e}" for v in R["hist"]))
        assert R["converged"]
        for k, v in enumerate(R["hist"]):
            assert v <= rho ** k, (k, v)
        assert R["iters"] <= math.ceil(math.log(G.rtol_of(name)) / math.log(rho))


@pytest.mark.parametrize("name,op,restart", G.gpu_cases())
def test_rtol_keeps_a_factor_of_four_from_both_neighbours(name, op, restart):
    """A condition on the input: one that fails it gets another seed (tests/_gmres_ref.py)."""
    rtol = G.rtol_of(name, restart)
    R = G.reference(name, op, restart)
    h, k = R["hist"], R["iters"]
    print(f"{name} op={op} restart={restart}: rtol {rtol:.3e} iters {k} cycles {R['cycles']} before "
          f"{min(h[:k]):.3e} at {h[k]:.3e} true {R['true'][-1]:.3e}")
    assert R["converged"] and R["solves"] == R["iters"] + R["cycles"]
    assert len(h) == k + 1
    assert min(h[:k]) >= 4.0 * rtol      # no earlier step comes near the stop
    assert h[k] <= rtol / 4.0
    assert R["true"][-1] <= rtol / 2.0   # and the true residual agrees with the estimate
    if restart < k:
        assert R["cycles"] == -(-k // restart)


def test_three_steps_reach_half_rho_cubed():
    """The maxit = 3 case: what three steps must have reached."""
    name = G.MAXIT_INPUT
    rho = rho_dense(name, "N")
    R = G.reference(name, "N", 30, rtol=1e-14, maxit=3)
    print(f"{name}: rho {rho:.3e} after 3 steps: estimate {R['hist'][3]:.3e} true {R['true'][-1]:.3e}")
    assert not R["converged"] and R["iters"] == 3 and R["cycles"] == 1
    assert R["hist"][3] <= 0.5 * rho ** 3
    assert R["true"][-1] <= 0.5 * rho ** 3
