"""The inputs of test_gpu_options.py, in one place so that test_options_inputs.py can prove on the
CPU that they are what the GPU tests assume."""
import functools
import os

import numpy as np
import scipy.sparse as sp

import oracle as O
import smlu
from smlu import matrices as mats

from _parity import tile_pivoting_matrix
from test_gpu_kernel_parity import _dominant_dense as dominant_dense, _weak_tile_matrix as weak_tile_matrix  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))


def csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    A.sum_duplicates()
    return A


def golden(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)
    n = int(z["n"])
    return csc(sp.csc_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=(n, n)))


# use_mfma = False: name -> (matrix, factor_parity's rtol for it in test_gpu_kernel_parity.py)
NO_MFMA = {
    "poisson3d_16": (lambda: mats.poisson3d(16), 1e-12),
    "poisson3d_24": (lambda: mats.poisson3d(24), 1e-12),
    "dominant_dense_700": (lambda: dominant_dense(700, 5), 1e-11),
    "tile_pivoting_1100": (lambda: tile_pivoting_matrix(1100, 1111), 1e-10),
}

# scale = False: name -> (matrix, rtol of the existing parity tests of that kind of matrix, the value
# O.dominant has for A and for its row-scaled twin B)
NO_SCALE = {
    "random_dominant_300": (lambda: mats.random_dominant(300, 0.02, seed=3), 1e-11, True),
    "tile_pivoting_700": (lambda: tile_pivoting_matrix(700, 5), 1e-10, False),
    "poisson2d_20": (lambda: mats.poisson2d(20), 1e-12, True),
    "poisson3d_10": (lambda: mats.poisson3d(10), 1e-12, True),
    "fe_8": (lambda: golden("fe_8"), 1e-10, False),
}

# pivot_tol: the matrix whose re-pivoting decision flips, the default and the stricter tolerance
FLIP_SEED = (1100, 1111)
FLIP_TOLS = (0.1, 0.6)

LEAF = {"poisson2d_40": lambda: mats.poisson2d(40), "poisson3d_12": lambda: mats.poisson3d(12)}
LEAF_SIZES = (16, 256)


@functools.lru_cache(maxsize=None)
def matrix(group, name):
    table = {"no_mfma": NO_MFMA, "no_scale": NO_SCALE}[group]
    return csc(table[name][0]())


def row_scaled_twin(A):
    """(B, r): B = diag(r) A with r = O.rowscale(A), each product rounded once -- the entries
    Rs[row] * a that a scale=True handle of A assembles."""
    A = csc(A)
    r = O.rowscale(A)
    B = A.copy()
    B.data = r[A.indices] * A.data
    return B, r


def plan_fronts(A, **kw):
    """(q, fronts dict) of the host plan of A, as oracle.gpu_pivot_choice takes them."""
    P = smlu.Plan(A, **kw)
    first, parent, rowptr, rows, p0 = P.fronts()
    return P.q(), dict(first=first, parent=parent, rowptr=rowptr, rows=rows, p0=p0)
