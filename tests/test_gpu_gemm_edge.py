"""The 128 x 128 MFMA tile's edge path (gemm128_mfma3_edge: tiles with fewer than 128 live rows or
columns) against the VALU 64 tile, bit for bit, and against the oracle.

An edge tile lays its four waves over the live region (four layouts, chosen from the live extents
lm, ln: both > 64, ln <= 64, lm <= 64, both <= 64), skips the MFMA blocks beyond the extents, stages
A by LDS-DMA (even m) or through registers (odd m) and B by LDS-DMA from clamped columns, and guards
C per row pair and column.  Each C element is still acc = C (or the gathered child sum), then one
multiply-add per k in ascending k, so L, U, p and Rs must be bitwise those of the VALU 64 tile.

SMLU_T128MIN=1 and SMLU_SMALLK=0 put every GEMM launch on the 128 tile; the fronts here are all
smaller than four tiles, so nearly every tile is an edge tile.  Dense fronts of order 129 ... 449 give
in-block and trailing updates with live extents 1, 63, 64, 65 and 127 in both dimensions (odd and
even m, every layout); the Poisson cases add the GEMM-form triangular solves (growth epilogue) and,
with SMLU_F22_GATHER_NU=1, F22 tasks with ragged nu through the gathering edge path."""
import numpy as np
import pytest
import scipy.sparse as sp

import smlu
from smlu import matrices as mats

from _parity import factor_parity, tile_pivoting_matrix

pytestmark = pytest.mark.gpu

MFMA128 = {"SMLU_T128MIN": "1", "SMLU_SMALLK": "0"}
VALU64 = {"SMLU_T128MIN": str(1 << 60), "SMLU_SMALLK": "0"}


def make(A, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    F = smlu.ParallelSparseLU(A)
    for k in env:
        monkeypatch.delenv(k)
    return F


def ran_mfma128(F):
    assert F.stat("launches_mfma128") > 0 and F.stat("launches_valu64") == 0
    assert F.stat("launches_k64") == 0 and F.stat("vendor_calls") == 0


def ran_valu64(F):
    assert F.stat("launches_valu64") > 0
    assert F.stat("launches_mfma128") == 0 and F.stat("launches_k64") == 0


def same_factors(Fa, Fb):
    assert np.array_equal(Fa.L.indices, Fb.L.indices)
    assert np.array_equal(Fa.L.data, Fb.L.data)
    assert np.array_equal(Fa.U.data, Fb.U.data)
    assert np.array_equal(Fa.p, Fb.p)
    assert np.array_equal(Fa.Rs, Fb.Rs)


def dominant_dense(n, seed):
    rng = np.random.default_rng(seed)
    D = rng.random((n, n))
    D += np.diag(D.sum(axis=1) + 1)
    return D


def tile_pair(A, monkeypatch, rtol):
    Fm, Fv = make(A, monkeypatch, MFMA128), make(A, monkeypatch, VALU64)
    ran_mfma128(Fm)
    ran_valu64(Fv)
    same_factors(Fm, Fv)
    factor_parity(A, Fm, rtol=rtol)
    Fm.close()
    Fv.close()


@pytest.mark.parametrize("n", [129, 191, 192, 193, 257, 321, 449])
def test_dense_front_ragged_extents(gpu, monkeypatch, n):
    tile_pair(sp.csc_matrix(dominant_dense(n, n)), monkeypatch, 1e-11)


def test_dense_front_tile_pivoting(gpu, monkeypatch):
    # row interchanges inside the diagonal tiles
    tile_pair(sp.csc_matrix(tile_pivoting_matrix(449, 449)), monkeypatch, 1e-10)


@pytest.mark.parametrize("N", [16, 20])
def test_poisson3d_gathering_edge_tiles(gpu, monkeypatch, N):
    # F22 tasks with ragged nu: gathered in the edge tiles' C prologue, against the plain edge
    # tiles and against the VALU tile; the GEMM-form triangular solves run on edge tiles too
    A = mats.poisson3d(N)
    gather = {"SMLU_F22_GATHER_NU": "1", "SMLU_F22_GATHER_CH": "64"}
    Fg = make(A, monkeypatch, MFMA128 | gather)
    Fo = make(A, monkeypatch, MFMA128 | {"SMLU_F22_GATHER_NU": "0"})
    Fv = make(A, monkeypatch, VALU64)
    ran_mfma128(Fg)
    ran_mfma128(Fo)
    ran_valu64(Fv)
    assert Fg.stat("f22_gather_fronts") > 0 and Fg.stat("launches_mfma128_gather") > 0
    assert Fo.stat("f22_gather_fronts") == 0 and Fo.stat("launches_mfma128_gather") == 0
    assert Fg.stat("launches_mfma128_trsm") > 0
    same_factors(Fg, Fo)
    same_factors(Fg, Fv)
    factor_parity(A, Fg)
    for F in (Fg, Fo, Fv):
        F.close()


def test_refactor_replay_new_values(gpu, monkeypatch):
    # the captured graph replayed with other values: bitwise the VALU tile's factors again, and
    # two refactors of the same values bitwise equal
    import torch
    A = mats.poisson3d(20)
    Fg = make(A, monkeypatch, MFMA128 | {"SMLU_F22_GATHER_NU": "1", "SMLU_F22_GATHER_CH": "64"})
    Fv = make(A, monkeypatch, VALU64)
    ran_mfma128(Fg)
    ran_valu64(Fv)
    A2 = mats.perturb_diag(A, 7)
    v = torch.from_numpy(np.ascontiguousarray(A2.data)).cuda()
    Fg.refactor_device(v)
    Fv.refactor_device(v)
    same_factors(Fg, Fv)
    L1, U1, p1 = Fg.L.data.copy(), Fg.U.data.copy(), np.array(Fg.p)
    Fg.refactor_device(v)
    assert np.array_equal(Fg.L.data, L1) and np.array_equal(Fg.U.data, U1) and np.array_equal(Fg.p, p1)
    factor_parity(A2, Fg)
    Fg.close()
    Fv.close()
