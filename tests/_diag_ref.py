"""Host references shared by test_gpu_logabsdet.py and test_gpu_rcond.py: fixtures, the derived
tolerance, and one SuperLU factorization of poisson3d(28) (computed once per session)."""
import functools
import os

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from smlu import matrices as mats

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -52

GOLDEN = ["dense_1", "dense_2", "dense_13", "fe_5", "fe_8", "poisson2d_16", "poisson3d_6", "random_dominant_200"]


def load_golden(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)
    n = int(z["n"])
    return sp.csc_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=(n, n))


def cond1(Ad):
    """cond_1(A) of a dense matrix, from its explicit inverse."""
    return np.abs(Ad).sum(axis=0).max() * np.abs(np.linalg.inv(Ad)).sum(axis=0).max()


def rounding(n, cond):
    """8 n 2^-52 cond_1(A): the first-order effect of the factorization's backward error on log det
    (d log det = tr(A^-1 dA)) and on the solves behind the norm estimate; 8 as in ctol."""
    return 8.0 * n * EPS * cond


@functools.lru_cache(maxsize=None)
def poisson(kind):
    """poisson3d(28) ("3d_28": large fronts) or poisson2d(300) ("2d_300": n = 90,000, more than the
    65,536 indices one pass of the reduction grid covers) with SuperLU's log|det| and exact inverse
    norms.  Both are M-matrices, A^-1 >= 0, so ||A^-1||_1 = ||A^-T 1||_inf and
    ||A^-1||_inf = ||A^-1 1||_inf exactly: one solve each."""
    A = mats.poisson3d(28) if kind == "3d_28" else mats.poisson2d(300)
    n = A.shape[0]
    lu = spla.splu(A)
    logabs = float(np.log(np.abs(lu.U.diagonal())).sum() + np.log(np.abs(lu.L.diagonal())).sum())
    one = np.ones(n)
    inv1 = float(np.abs(lu.solve(one, trans="T")).max())
    invinf = float(np.abs(lu.solve(one)).max())
    return dict(A=A, n=n, logabs=logabs, inv1=inv1, invinf=invinf, anorm1=float(abs(A).sum(axis=0).max()),
                anorminf=float(abs(A).sum(axis=1).max()))
