"""The interior K loop of the 128 x 128 MFMA tile (gemm128_mfma3_interior) against the VALU 64 tile,
bit for bit, and against the oracle.

The loop pins its own instruction order: fragment reads behind the first MFMA of the quad before
the one that uses them, the next slice's LDS-DMA in pairs behind the first MFMAs of quad 0, the
barrier between quads 2 and 3, two slices per loop trip (the LDS buffer is a compile-time constant),
a barrier and a (stale, unused) fragment read on the last slice too.  It can go wrong in the first
and last slices, the partial slice (K % 16), the buffer parity (odd and even slice counts) and the
early exit of the two-slice trip.  Each C element is still acc = C (or the gathered child sum), then
one multiply-add per k in ascending k, so L, U, p and Rs must be bitwise those of the VALU 64 tile.

SMLU_T128MIN=1 and SMLU_SMALLK=0 put every GEMM launch on the 128 tile.  The shapes are the smallest
that put INTERIOR tiles (full 128 x 128) through those places:
  * one dense front of order 640, default outer block: a 256 x 256 trailing update at k = 384 (24
    slices, four interior tiles); order 384 with SMLU_OB=128: k = 128 and the in-block k = 64;
  * F22 with k = ns across the slice boundaries: two dense ns x ns blocks, each fully coupled to a
    common dense block of order 256.  Such a child has the structure of its parent's first column,
    so relaxed amalgamation always folds both into the root whatever the border's size (there is no
    fill to pay), and even the fundamental supernodes fold the LAST child into the root: the tests
    build with relax=False and assert from the assembly tree that the first child stands alone with
    ns columns and 256 update rows, i.e. an F22 task of 256 x 256 (four interior tiles) at k = ns;
  * the gathering instantiation: the same two blocks under a border that has an update block of its
    own (natural order, a small last child keeps the border front out of the root), so that the
    border front's F22 (256 x 256, k = ns + 256) is gathered from the first child's F22."""
import numpy as np
import pytest
import scipy.sparse as sp

import smlu

from _parity import DENSE_TOL, factor_parity, tile_pivoting_matrix

pytestmark = pytest.mark.gpu

MFMA128 = {"SMLU_T128MIN": "1", "SMLU_SMALLK": "0"}
VALU64 = {"SMLU_T128MIN": str(1 << 60), "SMLU_SMALLK": "0"}
GATHER = {"SMLU_F22_GATHER_NU": "1", "SMLU_F22_GATHER_CH": "64"}
NB = 256   # border: two tiles in each direction


def make(A, monkeypatch, env, **kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    F = smlu.ParallelSparseLU(A, **kw)
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


def dominant(D):
    D += np.diag(np.abs(D).sum(axis=1) + 1)
    return sp.csc_matrix(D)


def dominant_dense(n, seed):
    return dominant(np.random.default_rng(seed).random((n, n)))


def two_children(ns, seed):
    """Two dense ns x ns blocks, each fully coupled to a common dense block of order NB."""
    rng = np.random.default_rng(seed)
    n = 2 * ns + NB
    D = np.zeros((n, n))
    for c in range(2):
        s = slice(c * ns, (c + 1) * ns)
        D[s, s] = rng.random((ns, ns))
        D[s, 2 * ns:] = rng.random((ns, NB))
        D[2 * ns:, s] = rng.random((NB, ns))
    D[2 * ns:, 2 * ns:] = rng.random((NB, NB))
    return dominant(D)


def two_children_gathered(ns, seed):
    """Blocks a1, a2 (ns each), border (NB), b (8), outer (NB) in this order: a1 and a2 coupled to
    the border and the outer block, the border and b to the outer block.  Fundamental supernodes in
    natural order: a1 | a2 + border | b + outer, so the border front (nu = NB) gathers its F22 from
    a1's."""
    rng = np.random.default_rng(seed)
    o_b, o_s, o_r = 2 * ns, 2 * ns + NB, 2 * ns + NB + 8
    n = o_r + NB
    D = np.zeros((n, n))

    def couple(r, c):
        D[r, c] = rng.random(D[r, c].shape)
        D[c, r] = rng.random(D[c, r].shape)

    border, small, outer = slice(o_b, o_s), slice(o_s, o_r), slice(o_r, n)
    for c in range(2):
        s = slice(c * ns, (c + 1) * ns)
        couple(s, s)
        couple(s, border)
        couple(s, outer)
    for s in (border, small, outer):
        couple(s, s)
    couple(border, outer)
    couple(small, outer)
    return dominant(D)


def tile_pair(A, monkeypatch, rtol, env=None, **kw):
    env = env or {}
    Fm, Fv = make(A, monkeypatch, MFMA128 | env, **kw), make(A, monkeypatch, VALU64 | env, **kw)
    ran_mfma128(Fm)
    ran_valu64(Fv)
    same_factors(Fm, Fv)
    factor_parity(A, Fm, rtol=rtol)
    return Fm, Fv


def close(*Fs):
    for F in Fs:
        F.close()


def test_trailing_k384_four_interior_tiles(gpu, monkeypatch):
    close(*tile_pair(dominant_dense(640, 640), monkeypatch, DENSE_TOL))


def test_outer_block_128_inblock_k64(gpu, monkeypatch):
    close(*tile_pair(dominant_dense(384, 384), monkeypatch, DENSE_TOL, env={"SMLU_OB": "128"}))


def test_tile_pivoting_640(gpu, monkeypatch):
    close(*tile_pair(sp.csc_matrix(tile_pivoting_matrix(640, 640)), monkeypatch, DENSE_TOL))


def child_fronts(F, ns, nu):
    t = F.fronts()
    cols, rows = np.diff(t["first"]), np.diff(t["rowptr"])
    return [s for s in range(cols.size) if cols[s] == ns and rows[s] == nu and t["parent"][s] >= 0]


@pytest.mark.parametrize("ns", [15, 16, 17, 31, 32, 33, 47, 48, 49, 65])
def test_f22_k_across_slice_boundaries(gpu, monkeypatch, ns):
    A = two_children(ns, ns)
    Fm, Fv = tile_pair(A, monkeypatch, DENSE_TOL, relax=False)
    # the first child was not amalgamated: its F22 task is NB x NB at k = ns, on the 128 tile
    assert len(child_fronts(Fm, ns, NB)) == 1
    assert Fm.stat("launches_mfma128") >= 2   # the child's F22 and the root's trailing updates
    close(Fm, Fv)


@pytest.mark.parametrize("ns", [17, 32, 49])
def test_f22_gathering_instantiation(gpu, monkeypatch, ns):
    A = two_children_gathered(ns, ns)
    kw = dict(relax=False, ordering="natural")
    Fg = make(A, monkeypatch, MFMA128 | GATHER, **kw)
    Fo = make(A, monkeypatch, MFMA128 | {"SMLU_F22_GATHER_NU": "0"}, **kw)
    Fv = make(A, monkeypatch, VALU64, **kw)
    ran_mfma128(Fg)
    ran_mfma128(Fo)
    ran_valu64(Fv)
    assert len(child_fronts(Fg, ns, 2 * NB)) == 1          # a1: F22 of 2 NB x 2 NB at k = ns
    assert len(child_fronts(Fg, ns + NB, NB)) == 1         # a2 + border: F22 of NB x NB at k = ns + NB
    assert Fg.stat("f22_gather_fronts") > 0 and Fg.stat("launches_mfma128_gather") > 0
    assert Fo.stat("launches_mfma128_gather") == 0
    same_factors(Fg, Fo)
    same_factors(Fg, Fv)
    factor_parity(A, Fg, rtol=DENSE_TOL)
    close(Fg, Fo, Fv)


def test_graph_replay_new_values(gpu, monkeypatch):
    # the captured graph replayed with other values: bitwise the VALU tile's factors again, and
    # two refactors of the same values bitwise equal
    import torch
    A = dominant_dense(640, 641)
    Fm, Fv = make(A, monkeypatch, MFMA128), make(A, monkeypatch, VALU64)
    ran_mfma128(Fm)
    ran_valu64(Fv)
    A2 = A.copy()
    A2.data = A.data * (1.0 + 0.25 * np.random.default_rng(7).random(A.nnz))
    A2 = A2 + sp.diags(np.full(640, 80.0))   # same pattern (dense), still dominant
    A2 = sp.csc_matrix(A2)
    A2.sort_indices()
    assert np.array_equal(A2.indptr, A.indptr) and np.array_equal(A2.indices, A.indices)
    v = torch.from_numpy(np.ascontiguousarray(A2.data)).cuda()
    Fm.refactor_device(v)
    Fv.refactor_device(v)
    same_factors(Fm, Fv)
    L1, U1, p1 = Fm.L.data.copy(), Fm.U.data.copy(), np.array(Fm.p)
    Fm.refactor_device(v)
    assert np.array_equal(Fm.L.data, L1) and np.array_equal(Fm.U.data, U1) and np.array_equal(Fm.p, p1)
    factor_parity(A2, Fm, rtol=DENSE_TOL)
    close(Fm, Fv)
