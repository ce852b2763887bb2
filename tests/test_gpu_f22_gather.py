"""F22 gathered in the Schur GEMM's C prologue (tile code 143, k_gemm128_mfma3<false, true, true>)
against the plain path, bit for bit.

A gathered front's F22 is never written by the assembly kernel: the tile that applies
F22 -= L21 U12 starts from the sum of the children's F22 entries, formed in child order exactly as
the assembly forms it.  So factors, pivots and row scaling must be bitwise those of the same library
with the gather off.  The knobs are forced so that oracle-sized fronts qualify: SMLU_T128MIN=1 and
SMLU_SMALLK=0 put every GEMM launch on the 128 tile, SMLU_F22_GATHER_NU=1 gathers every blocked
front within the child cap."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import smlu
from smlu import matrices as mats

from _parity import TOL, factor_parity, isapprox

pytestmark = pytest.mark.gpu

BASE = {"SMLU_T128MIN": "1", "SMLU_SMALLK": "0"}


def make(A, monkeypatch, gather, ch="8"):
    env = dict(BASE, SMLU_F22_GATHER_NU="1" if gather else "0", SMLU_F22_GATHER_CH=ch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    F = smlu.ParallelSparseLU(A)
    for k in env:
        monkeypatch.delenv(k)
    return F


def check_ran(Fg, Fo):
    assert Fg.stat("f22_gather_fronts") > 0 and Fg.stat("launches_mfma128_gather") > 0
    assert Fg.stat("f22_gather_entries") > 0
    assert Fo.stat("f22_gather_fronts") == 0 and Fo.stat("launches_mfma128_gather") == 0


def same_factors(Fg, Fo):
    assert np.array_equal(Fg.L.indices, Fo.L.indices)
    assert np.array_equal(Fg.L.data, Fo.L.data)
    assert np.array_equal(Fg.U.data, Fo.U.data)
    assert np.array_equal(Fg.p, Fo.p)
    assert np.array_equal(Fg.Rs, Fo.Rs)


def pair(A, monkeypatch, ch="8"):
    Fg, Fo = make(A, monkeypatch, True, ch), make(A, monkeypatch, False, ch)
    check_ran(Fg, Fo)
    same_factors(Fg, Fo)
    return Fg, Fo


@pytest.mark.parametrize("ch", ["8", "64"])
def test_poisson3d_24_bitwise_and_oracle(gpu, monkeypatch, ch):
    # nu up to 387 (interior and edge tiles), parents with up to 21 children, gathered parents of
    # gathered children, children that are small fronts
    A = mats.poisson3d(24)
    Fg, Fo = pair(A, monkeypatch, ch)
    if ch == "64":
        # a front the cap of 8 leaves to the assembly is gathered here
        F8 = make(A, monkeypatch, True, "8")
        assert Fg.stat("f22_gather_fronts") > F8.stat("f22_gather_fronts")
        F8.close()
    else:
        factor_parity(A, Fg)
        b = np.random.default_rng(24).random(A.shape[0])
        x = np.empty_like(b)
        smlu.ldiv_(x, Fg, b)
        assert isapprox(x, spla.spsolve(A, b), TOL, TOL)
    Fg.close()
    Fo.close()


def test_poisson3d_16_edge_tiles_only(gpu, monkeypatch):
    # every gathered F22 is smaller than one 128 tile: only the guarded edge body runs
    A = mats.poisson3d(16)
    Fg, Fo = pair(A, monkeypatch, "64")
    Fg.close()
    Fo.close()


def test_random_dominant_irregular_maps(gpu, monkeypatch):
    # irregular, non-contiguous row maps
    A = mats.random_dominant(1000, 0.01, seed=47)
    Fg, Fo = pair(A, monkeypatch, "64")
    Fg.close()
    Fo.close()


def test_replay_with_new_values(gpu, monkeypatch):
    # the captured graph replayed with two other value sets: no read of a stale F22
    import torch
    A = mats.poisson3d(20)
    Fg, Fo = pair(A, monkeypatch, "64")
    for seed in (5, 6):
        v = torch.from_numpy(np.ascontiguousarray(mats.perturb_diag(A, seed).data)).cuda()
        Fg.refactor_device(v)
        Fo.refactor_device(v)
        same_factors(Fg, Fo)
    Fg.close()
    Fo.close()


def test_poisson3d_16_nondominant_mode1(gpu, monkeypatch):
    # values far from dominant: the full-candidate (mode 1) schedule of the mid-size fronts
    A = mats.poisson3d(16)
    A2 = A.copy()
    A2.data = np.random.default_rng(9).standard_normal(A.nnz)
    Fg, Fo = pair(A2, monkeypatch, "64")
    assert Fg.stat("dominant") == 0.0 and Fg.stat("fronts_mode1") > 0
    Fg.close()
    Fo.close()
