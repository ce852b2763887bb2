"""A partitioned handle (smlu_dist_*) refuses the determinant and the condition estimate: both
read one GPU's factors and run the transposed solve, which are single-GPU.  Two ranks share cuda:0
over the host-memory transport (the rehearsal of test_gpu_dist.py); on each rank smlu_logabsdet,
smlu_logabsdet_z and smlu_rcond return SMLU_ERR_STATE, run nothing, and leave the handle solving."""
import ctypes
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from test_gpu_dist import _free_port, _matrix

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q):
    try:
        import torch
        import torch.distributed as dist
        import smlu
        from smlu import _lib as C
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        A = _matrix("poisson")
        n = A.shape[0]
        F = smlu.DistributedSparseLU(A, device=0)
        L = C.lib()
        a, b, r = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        ph = (ctypes.c_double * 2)()
        passes = F.stat("solve_trans_passes")
        codes = [L.smlu_logabsdet(F._h, ctypes.byref(a), ctypes.byref(b)),
                 L.smlu_logabsdet_z(F._h, ctypes.byref(a), ph),
                 L.smlu_rcond(F._h, C.SMLU_NORM_ONE, ctypes.byref(r), None, None),
                 L.smlu_rcond(F._h, C.SMLU_NORM_INF, ctypes.byref(r), ctypes.byref(a), ctypes.byref(b))]
        ran = (F.stat("solve_trans_passes") - passes, F.stat("rcond_solves"), F.stat("logabsdet_evals"))
        msg = C.last_error(F._h)
        rhs = np.random.default_rng(11).random(n)
        db = torch.from_numpy(rhs).cuda()
        dx = torch.empty_like(db)
        F.solve_device(dx, db)            # collective: the refused calls left every rank in step
        x = dx.cpu().numpy()
        res = float(np.abs(A @ x - rhs).max() / np.abs(rhs).max())
        q.put((rank, codes, ran, msg, F.stat("nranks"), res, None))
        F.close()
        dist.destroy_process_group()
    except Exception:  # report instead of hanging the parent
        import traceback
        q.put((rank, None, None, None, None, None, traceback.format_exc()))


def test_partitioned_handle_is_a_state_error():
    from smlu import _lib as C
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=240) for _ in ps]
    for p in ps:
        p.join(timeout=120)
    errs = [r[6] for r in res if r[6]]
    assert not errs, errs[0]
    for p in ps:
        assert p.exitcode == 0
    for rank, codes, ran, msg, nranks, resid, _ in res:
        assert nranks == world
        assert codes == [C.SMLU_ERR_STATE] * 4, (rank, codes)
        assert ran == (0, 0, 0), (rank, ran)          # no solve and no device evaluation ran
        assert "single-GPU" in msg, msg
        assert resid < 1e-12, (rank, resid)
