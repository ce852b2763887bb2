"""Batched forward solves: up to 16 right-hand sides per pass of the solve kernels
(smlu_solve_multi[_device]; solve_multi_device, ldiv_ with 2D arrays), on factors whose front
permutations exchange rows as well as on dominant ones.

Two oracles throughout.  Column j of a batch must be bitwise solve_device of that column alone on
the same handle; and once per matrix the batch is held against a reference that is not the library
(tests/_batch_ref.py: the fixed-pivot oracle's unrefined ldiv on the GPU's pivot order, componentwise
backward error within 4x of the oracle's or under 2^-51, and agreement in norm), so that both being
wrong is caught.  Every handle is created with refine=0: under the default options a non-dominant
matrix is refined, and solve_cols then goes column by column, which would compare the
single-vector solve with itself.  Every batch asserts through the "solve_passes" stat that the batch
kernels ran: ceil(nrhs / 16) passes per call.  Outputs start as NaN.

Shapes, the smallest that reach each kernel: poisson3d(12) (micro, tiny and small fronts, identity
permutations), poisson3d(28) (sweeps), poisson2d(300) (tall fronts), tile_pivoting_matrix(700, 5)
(blocked front, row exchanges in every tile, partial last block), a dense 321 front (one pivoting
front above kSolveBigNs on the sweeps), the non-dominant FE matrix and golden fe_5 / dense_13 /
dense_1 / dense_2 (pivoting inside micro, tiny and small fronts, n = 1, 2), and two complex handles,
one with its real-equivalent pairs exchanged.  Widths: 8 against 9 is sweep against per-block
schedule (fwdm / bwdm), 17 ends in a single-vector pass with a leading dimension, 33 is three passes.

Measured on an MI355X over the columns of a 5-wide batch (test_every_matrix_against_the_oracle): the
largest backward-error ratio GPU / oracle (the bound is 4, or any ratio while the GPU's error is
under 2^-51 = 4.4e-16), the two errors of that column, the largest |x - xo| / |xo| with its
tolerance, and the rows that pivoting moved inside their fronts.

    matrix                 ratio   berr GPU   berr oracle  |x-xo|/|xo|  tol    rows moved
    pivoting_small_fronts  1.073   5.384e-16  5.018e-16    2.374e-14    1e-10  648 of 690 (16 micro, 16 tiny, 1 small front)
    poisson3d_12           0.639   5.225e-16  8.174e-16    5.740e-16    1e-12  0
    poisson3d_28           0.546   1.747e-15  3.200e-15    3.428e-15    1e-12  0
    poisson2d_300          0.683   2.523e-15  3.696e-15    1.010e-13    1e-12  0
    tile_pivoting_700_5    1.426   6.700e-14  4.698e-14    4.263e-12    1e-10  28 of 700 (1 big front)
    dense_321              0.865   5.657e-14  6.542e-14    4.452e-12    1e-10  2 of 321 (1 big front)
    nondominant_fe_300     0.984   5.944e-14  6.042e-14    1.953e-12    2e-12  0
    fe_5                   2.455   1.302e-15  5.302e-16    4.750e-15    1e-12  0
    dense_13               3.169   1.773e-15  5.595e-16    2.585e-14    1e-10  0
    dense_1                1.000   2.820e-17  2.820e-17    0            1e-10  0
    dense_2                3.312   8.362e-17  2.524e-17    1.544e-16    1e-10  0
    complex_tile_150       1.555   6.979e-15  4.490e-15    5.965e-14    1e-10  (pairs moved and exchanged)
    complex_poisson3d_12   0.604   8.564e-16  1.419e-15    8.200e-16    1e-12
    nondominant_fe_300, default options, against spsolve:  0.416  1.018e-16  2.449e-16  5.453e-14  1e-12
    the same handle refactored with dominant values:        1.093  3.845e-16  3.516e-16  2.886e-16  1e-12

Under the default diagonal tolerance the fe and dense fixtures keep every diagonal (0 rows moved), so
pivoting_small_fronts, factored with partial pivoting, is what exchanges rows in the micro, tiny
and small fronts.  nondominant_fe_300 without refinement misses the 1e-12 agreement in norm (see
NORM_TOL below).
"""
import ctypes
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import oracle as O
import smlu
from smlu import _lib as C
from smlu import matrices as mats

from _batch_ref import assert_batch_against_oracle, complex_tile_150, stale_slot_sequence
from _parity import TOL, DENSE_TOL, tile_pivoting_matrix
from test_gpu_solve_trans import load_golden
from test_gpu_solve_trans_batched import _rhs, complex_p12, nondominant_fe

pytestmark = pytest.mark.gpu


def dense_321():
    return sp.csc_matrix(np.random.default_rng(321).random((321, 321)))


def pivoting_small_fronts():
    """Row exchanges inside micro, tiny and small fronts (k_fwd_micro, k_fwd_tiny, k_fwd_front): two
    chains of dense random element blocks (5 and 30 wide, O.test_matrix), one dense 200 block and
    sixteen separate dense blocks of 6 and 3 rows.
    Its handle is created with diag_pivot_tol=1 (HANDLE_KW): a diagonal entry is then kept only
    where it is the largest of its column, which is partial pivoting, and rows are exchanged in
    most fronts.  Under the default diagonal tolerance of 0.001 the row matching ahead of the
    analysis leaves the fronts almost nothing to exchange: the fe and dense fixtures move 0 rows
    (measured table), and tiny diagonals instead of the option moved 8 rows of the first 612."""
    rng = np.random.default_rng(88)
    parts = [O.test_matrix(rng, 30, 5), O.test_matrix(rng, 10, 30), rng.random((200, 200))]
    parts += [rng.random((m, m)) for m in (6,) * 10 + (3,) * 6]   # separate blocks: fronts of M <= 8
    return sp.csc_matrix(sp.block_diag(parts))


def moved_rows_by_front_class(F):
    """Fronts with rows moved by pivoting, counted by the solve kernel that takes them
    (schedule.hpp: micro M <= 8, tiny M <= 128 and ns <= 64, big ns > 256 or ns M > 2^16)."""
    fr = F.fronts()
    ns = np.diff(fr["first"])
    M = ns + np.diff(fr["rowptr"])
    moved = F.p != fr["p0"]
    out = dict(micro=0, tiny=0, small=0, big=0)
    for s in range(ns.size):
        if moved[fr["first"][s]:fr["first"][s + 1]].any():
            big = ns[s] > 256 or ns[s] * M[s] > 1 << 16
            out["big" if big else "micro" if M[s] <= 8 else "tiny" if M[s] <= 128 and ns[s] <= 64 else "small"] += 1
    return out


MATRICES = {
    "pivoting_small_fronts": pivoting_small_fronts,
    "poisson3d_12": lambda: mats.poisson3d(12),
    "poisson3d_28": lambda: mats.poisson3d(28),
    "poisson2d_300": lambda: mats.poisson2d(300),
    "tile_pivoting_700_5": lambda: tile_pivoting_matrix(700, 5),
    "dense_321": dense_321,
    "nondominant_fe_300": nondominant_fe,
    "fe_5": lambda: load_golden("fe_5"),
    "dense_13": lambda: load_golden("dense_13"),
    "dense_1": lambda: load_golden("dense_1"),
    "dense_2": lambda: load_golden("dense_2"),
    "complex_tile_150": complex_tile_150,
    "complex_poisson3d_12": complex_p12,
}
COMPLEX = ["complex_tile_150", "complex_poisson3d_12"]
EXCHANGING = ["tile_pivoting_700_5", "pivoting_small_fronts"]   # F.p must differ from the fronts' p0 (the diagonal is never acceptable)


# Agreement in norm with the oracle where it is not the default (1e-10 for a full matrix, 1e-12
# otherwise).  nondominant_fe_300 unrefined: both solves have a backward error of 6e-14 (ratio 0.98)
# and differ by 1.953e-12 |x| in the worst of the five columns, over the 1e-12 that its refined
# solves meet (5e-14); the smallest power of two times 1e-12 that holds.  pivoting_small_fronts is
# made of dense random blocks: the tolerance of the dense cases.
NORM_TOL = {"nondominant_fe_300": 2 * TOL, "pivoting_small_fronts": DENSE_TOL}


HANDLE_KW = {"pivoting_small_fronts": dict(diag_pivot_tol=1.0)}


def make_handle(name):
    A = sp.csc_matrix(MATRICES[name]())
    return A, smlu.ParallelSparseLU(A, refine=0, **HANDLE_KW.get(name, {}))


@pytest.fixture(scope="module")
def handles(gpu):
    """name -> (A, F), each matrix factored once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = make_handle(name)
        return cache[name]

    yield get
    for _, F in cache.values():
        F.close()


def single(F, bj, trans="N"):
    import torch
    xj = torch.full_like(bj, float("nan"))
    F.solve_device(xj, bj, trans=trans)
    return xj


def solve_batch(F, B, X=None):
    """One solve_multi_device call into X (NaN before), with the pass count of the batch path."""
    import torch
    if X is None:
        X = torch.full_like(B, float("nan"))
    p0 = F.stat("solve_passes")
    assert np.isfinite(p0)
    F.solve_multi_device(X, B)
    assert F.stat("solve_passes") - p0 == math.ceil(B.shape[0] / 16), (B.shape[0], F.stat("solve_passes") - p0)
    return X


def check_batch(F, B, singles=None):
    """The batch of B's rows; every column bitwise its single solve (singles: those already known)."""
    import torch
    X = solve_batch(F, B)
    for j in range(B.shape[0]):
        xj = singles[j] if singles is not None else single(F, B[j].contiguous())
        assert torch.equal(X[j], xj), (B.shape[0], j, (X[j] - xj).abs().max().item())
    return X


# ---- a. width edges ------------------------------------------------------------------------------
def test_pass_count(handles):
    import torch
    A, F = handles("poisson3d_12")
    B = _rhs(F.n, 17, 130)
    X = torch.empty_like(B)
    p0 = F.stat("solve_passes")
    F.solve_multi_device(X[:8], B[:8])
    assert F.stat("solve_passes") - p0 == 1
    F.solve_multi_device(X, B)
    assert F.stat("solve_passes") - p0 == 3
    F.solve_device(X[0], B[0])
    assert F.stat("solve_passes") - p0 == 4
    t0 = F.stat("solve_trans_passes")
    F.solve_multi_device(X[:8], B[:8], trans="T")   # the transposed counter is another one
    assert F.stat("solve_passes") - p0 == 4 and F.stat("solve_trans_passes") - t0 == 1


@pytest.mark.parametrize("nrhs", [2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33])
def test_width_edges_poisson3d_12(handles, nrhs):
    A, F = handles("poisson3d_12")
    check_batch(F, _rhs(F.n, nrhs, 131 + nrhs))


@pytest.fixture(scope="module")
def big17(handles):
    """17 right-hand sides and their single solves on the two handles with sweeps, computed once."""
    out = {}
    for name in ("poisson3d_28", "dense_321"):
        A, F = handles(name)
        assert F.stat("solve_sweeps") > 0
        B = _rhs(F.n, 17, 170)
        out[name] = (B, [single(F, B[j].contiguous()) for j in range(17)])
    return out


@pytest.mark.parametrize("nrhs", [4, 7, 8, 9, 16, 17])
@pytest.mark.parametrize("name", ["poisson3d_28", "dense_321"])
def test_width_edges_on_the_sweeps(handles, big17, name, nrhs):
    """8 columns run the sweeps, 9 the per-block schedule, 17 end in a single-vector pass.  The batch
    is the last nrhs of the 17 columns, so a slot holds another column at every width."""
    A, F = handles(name)
    B, singles = big17[name]
    t0 = F.stat("sweep_timeouts")
    check_batch(F, B[17 - nrhs:].contiguous(), singles[17 - nrhs:])
    assert F.stat("sweep_timeouts") == t0


@pytest.mark.parametrize("name", list(MATRICES))
def test_every_matrix_against_the_oracle(handles, name):
    """Widths 5 and 16 (17 as well on the complex handles), every column bitwise its single solve,
    and the 5-wide batch against the oracle's unrefined solves on the same pivot order."""
    A, F = handles(name)
    if not F.is_complex:
        moved = int((F.p != F.fronts()["p0"]).sum())
        classes = moved_rows_by_front_class(F)
        print(f"{name}: {moved} of {F.n} rows moved inside their fronts; fronts with moved rows: {classes}")
        if name in EXCHANGING:
            assert moved > 0   # the fronts' row permutation is not the identity
        if name == "pivoting_small_fronts":
            assert classes["micro"] > 0 and classes["tiny"] > 0 and classes["small"] > 0, classes
        if name in ("tile_pivoting_700_5", "dense_321"):
            assert classes["big"] > 0, classes
    if name == "complex_tile_150":
        pk = F.real_equivalent_factors()["p"]
        assert F.stat("cpair") == 1 and int((pk[0::2] > pk[1::2]).sum()) > 0   # pairs exchanged inside themselves
    z = F.is_complex
    assert z == (name in COMPLEX)
    B = _rhs(F.n, 5, 150, z)
    X = check_batch(F, B)
    check_batch(F, _rhs(F.n, 16, 151, z))
    if z:
        check_batch(F, _rhs(F.n, 17, 152, z))
    assert_batch_against_oracle(A, F, B.cpu().numpy(), X.cpu().numpy(), "N", tol=NORM_TOL.get(name), label=name)


# ---- b. stale slots ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson3d_28", "tile_pivoting_700_5", "nondominant_fe_300", "pivoting_small_fronts"])
def test_stale_slots(gpu, name):
    A, F = make_handle(name)   # a fresh handle: nothing was solved on it before
    stale_slot_sequence(F)
    F.close()


# ---- c. layout -----------------------------------------------------------------------------------
def multi_device(F, nrhs, Bbuf, ldb, Xbuf, ldx):
    with C.caller_stream(F._h, Bbuf):
        return C.lib().smlu_solve_multi_device(F._h, nrhs, ctypes.c_void_p(Bbuf.data_ptr()), ldb,
                                               ctypes.c_void_p(Xbuf.data_ptr()), ldx)


def padded(Bc, ld):
    """The rows of Bc at pitch ld in one flat buffer, NaN in the padding."""
    import torch
    nr, n = Bc.shape
    buf = torch.full((nr * ld,), float("nan"), dtype=torch.float64, device="cuda:0")
    buf.view(nr, ld)[:, :n] = Bc
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("nrhs", [5, 17])
@pytest.mark.parametrize("name", ["poisson3d_12", "tile_pivoting_700_5"])
def test_leading_dimensions(handles, name, nrhs):
    import torch
    A, F = handles(name)
    n = F.n
    ldb, ldx = n + 3, n + 7
    Bc = _rhs(n, nrhs, 140 + nrhs)
    singles = [single(F, Bc[j].contiguous()) for j in range(nrhs)]
    Bbuf = padded(Bc, ldb)
    Xbuf = torch.full((nrhs * ldx,), float("nan"), dtype=torch.float64, device="cuda:0")
    p0 = F.stat("solve_passes")
    assert multi_device(F, nrhs, Bbuf, ldb, Xbuf, ldx) == C.SMLU_OK
    assert F.stat("solve_passes") - p0 == math.ceil(nrhs / 16)
    Xv = Xbuf.view(nrhs, ldx)
    for j in range(nrhs):
        assert torch.equal(Xv[j, :n], singles[j]), j
    assert torch.isnan(Xv[:, n:]).all()                      # the padding of X is never written
    assert torch.equal(Bbuf.view(nrhs, ldb)[:, :n], Bc)      # B is only read
    # in place, X is B: contiguous columns, then a pitch of n + 5
    V = Bc.clone()
    solve_batch(F, V, V)
    for j in range(nrhs):
        assert torch.equal(V[j], singles[j]), j
    ld = n + 5
    Vbuf = padded(Bc, ld)
    p0 = F.stat("solve_passes")
    assert multi_device(F, nrhs, Vbuf, ld, Vbuf, ld) == C.SMLU_OK
    assert F.stat("solve_passes") - p0 == math.ceil(nrhs / 16)
    Vv = Vbuf.view(nrhs, ld)
    for j in range(nrhs):
        assert torch.equal(Vv[j, :n], singles[j]), j
    assert torch.isnan(Vv[:, n:]).all()


def test_argument_checks(handles):
    import torch
    A, F = handles("poisson3d_12")
    n = F.n
    B = _rhs(n, 3, 145)
    X = torch.full_like(B, float("nan"))
    p0 = F.stat("solve_passes")
    assert multi_device(F, 3, B, n - 1, X, n) == C.SMLU_ERR_ARG
    assert multi_device(F, 3, B, n, X, n - 1) == C.SMLU_ERR_ARG
    assert multi_device(F, 0, B, n, X, n) == C.SMLU_OK
    torch.cuda.synchronize()
    assert torch.isnan(X).all()                              # nothing written
    assert F.stat("solve_passes") == p0


# ---- d. host path equals device path -------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson3d_12", "tile_pivoting_700_5"])
def test_host_path_equals_device_path(handles, name):
    A, F = handles(name)
    B = _rhs(F.n, 17, 146)
    X = check_batch(F, B)
    Bh = np.asfortranarray(B.cpu().numpy().T)   # n x 17, column-major
    Xh = np.full_like(Bh, np.nan)
    p0 = F.stat("solve_passes")
    smlu.ldiv_(Xh, F, Bh)
    assert F.stat("solve_passes") - p0 == 2
    assert np.array_equal(Xh, X.cpu().numpy().T)
    V = Bh.copy(order="F")
    smlu.ldiv_(V, F, V)                         # in place on the host
    assert np.array_equal(V, Xh)


@pytest.mark.parametrize("name", ["poisson3d_28", "tile_pivoting_700_5"])
def test_eager_launches_equal_graph_replay(handles, monkeypatch, name):
    import torch
    A, F = handles(name)
    for nrhs in (8, 16):
        B = _rhs(F.n, nrhs, 147 + nrhs)
        X = solve_batch(F, B)
        monkeypatch.setenv("SMLU_NO_GRAPH", "1")
        Xe = solve_batch(F, B)
        monkeypatch.delenv("SMLU_NO_GRAPH")
        assert torch.equal(Xe, X), nrhs


# ---- e. a sweep wait that gives up during a batch ------------------------------------------------
@pytest.mark.parametrize("name", ["poisson3d_28", "dense_321"])
def test_forced_sweep_timeout_in_a_batch(handles, monkeypatch, name):
    """SMLU_SWEEP_SPIN=0: every sweep wait reports a timeout, the batch is re-run on the per-block
    schedule from the kept input (bstash when x is b, at the caller's pitch otherwise) and is bitwise
    the normal handle's -- one re-run per call, not per column, and still one pass."""
    import torch
    A, F = handles(name)
    monkeypatch.setenv("SMLU_SWEEP_SPIN", "0")
    At, Ft = make_handle(name)                  # every sweep wait times out
    monkeypatch.delenv("SMLU_SWEEP_SPIN")
    assert Ft.stat("solve_sweeps") > 0
    n = F.n
    for nrhs in (3, 8):
        B = _rhs(n, nrhs, 180 + nrhs)
        X = solve_batch(F, B)
        t0 = Ft.stat("sweep_timeouts")
        assert torch.equal(solve_batch(Ft, B), X)                    # separate X
        assert Ft.stat("sweep_timeouts") == t0 + 1 and Ft.stat("sweep_status") == 0
        V = B.clone()
        solve_batch(Ft, V, V)                                        # X is B
        assert torch.equal(V, X)
        assert Ft.stat("sweep_timeouts") == t0 + 2 and Ft.stat("sweep_status") == 0
        ldb = n + 3
        Bbuf = padded(B, ldb)
        Xl = torch.full_like(B, float("nan"))
        p0 = Ft.stat("solve_passes")
        assert multi_device(Ft, nrhs, Bbuf, ldb, Xl, n) == C.SMLU_OK   # ldb = n + 3, separate X
        assert Ft.stat("solve_passes") - p0 == 1
        assert torch.equal(Xl, X)
        assert Ft.stat("sweep_timeouts") == t0 + 3 and Ft.stat("sweep_status") == 0
        Bh = np.asfortranarray(B.cpu().numpy().T)
        Xh = np.full_like(Bh, np.nan)
        smlu.ldiv_(Xh, Ft, Bh)                                       # the host entry: in place in its staging buffer
        assert np.array_equal(Xh, X.cpu().numpy().T)
        assert Ft.stat("sweep_timeouts") == t0 + 4 and Ft.stat("sweep_status") == 0
    t0 = Ft.stat("sweep_timeouts")
    B = _rhs(n, 9, 189)
    assert torch.equal(solve_batch(Ft, B), solve_batch(F, B))        # 9 columns never run the sweeps
    assert Ft.stat("sweep_timeouts") == t0
    assert F.stat("sweep_timeouts") == 0
    Ft.close()


# ---- f. interleaving -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson3d_28", "tile_pivoting_700_5"])
def test_interleaved_with_transposed_batches(handles, name):
    """single, batch of 8, transposed batch of 8, batch of 16, single: the batches share wrkm / vbufm."""
    import torch
    A, F = handles(name)
    n = F.n
    b = _rhs(n, 1, 190)[0].contiguous()
    B8, B16 = _rhs(n, 8, 191), _rhs(n, 16, 192)
    x_first = single(F, b)
    X8 = solve_batch(F, B8)
    Xt = torch.full_like(B8, float("nan"))
    F.solve_multi_device(Xt, B8, trans="T")
    X16 = solve_batch(F, B16)
    assert torch.equal(single(F, b), x_first)
    assert torch.equal(solve_batch(F, B8), X8)
    for j in (0, 7):
        assert torch.equal(X8[j], single(F, B8[j].contiguous()))
        assert torch.equal(Xt[j], single(F, B8[j].contiguous(), "T"))
    for j in (0, 15):
        assert torch.equal(X16[j], single(F, B16[j].contiguous()))


# ---- g. fallback and stats -----------------------------------------------------------------------
def test_refinement_falls_back_to_columns_and_batches_after_dominant_values(gpu):
    import torch
    A = sp.csc_matrix(nondominant_fe())
    F = smlu.ParallelSparseLU(A)   # default options: refined, one solve per column
    assert F.stat("dominant") == 0
    B = _rhs(F.n, 3, 195)
    X = torch.full_like(B, float("nan"))
    p0 = F.stat("solve_passes")
    F.solve_multi_device(X, B)
    assert F.stat("solve_passes") - p0 >= 3
    assert F.stat("refine_berr") >= 0   # a residual was taken
    Bh, Xh = B.cpu().numpy(), X.cpu().numpy()
    Xr = np.stack([spla.spsolve(A, Bh[j]) for j in range(3)])
    assert_batch_against_oracle(A, F, Bh, Xh, "N", Xo=Xr, tol=TOL, label="nondominant_fe_300 refined")
    # the same pattern with dominant values: no refinement, so a batch, and no stale refinement stats
    A2 = sp.csc_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel()))
    A2.sort_indices()
    assert np.array_equal(A2.indptr, A.indptr) and np.array_equal(A2.indices, A.indices)
    smlu.lu_(F, A2)
    assert F.stat("dominant") == 1
    B5 = _rhs(F.n, 5, 196)
    p0 = F.stat("solve_passes")
    X5 = torch.full_like(B5, float("nan"))
    F.solve_multi_device(X5, B5)
    assert F.stat("solve_passes") - p0 == 1
    assert F.stat("refine_steps") == 0 and F.stat("refine_residual") == -1 and F.stat("refine_berr") == -1
    for j in range(5):
        assert torch.equal(X5[j], single(F, B5[j].contiguous())), j
    assert_batch_against_oracle(A2, F, B5.cpu().numpy(), X5.cpu().numpy(), "N", label="nondominant_fe_300 made dominant")
    F.close()
