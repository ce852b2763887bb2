"""A partitioned handle (smlu_dist_*) refuses smlu_lowrank_set* and smlu_solve_lowrank*: Y = A^-1 U, the
update's vectors and the transposed solve are single-GPU.  Two ranks share cuda:0 over the host-memory
transport (the rehearsal of test_gpu_dist.py); on each rank both entry points, in both forms, return
SMLU_ERR_STATE, run no solve, and leave the handle solving."""
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
        rhs = np.random.default_rng(11).random(n)
        W = np.asfortranarray(np.random.default_rng(12).random((n, 2)))
        xh = np.empty(n)
        db = torch.from_numpy(rhs).cuda()
        dx = torch.empty_like(db)
        dW = torch.from_numpy(W.T.copy()).cuda()
        ci = C.SmluLowrankInfo()
        passes = (F.stat("solve_passes"), F.stat("solve_trans_passes"))
        codes = [L.smlu_lowrank_set(F._h, 2, C.ptr(W), n, C.ptr(W), n, ctypes.byref(ci)),
                 L.smlu_lowrank_set_device(F._h, 2, ctypes.c_void_p(dW.data_ptr()), n, ctypes.c_void_p(dW.data_ptr()), n,
                                           None)]
        for op in (C.SMLU_OP_N, C.SMLU_OP_T, C.SMLU_OP_H):
            codes.append(L.smlu_solve_lowrank(F._h, op, -1, C.ptr(rhs), C.ptr(xh), ctypes.byref(ci)))
            codes.append(L.smlu_solve_lowrank_device(F._h, op, 0, ctypes.c_void_p(db.data_ptr()),
                                                     ctypes.c_void_p(dx.data_ptr()), None))
        ran = (F.stat("solve_passes") - passes[0], F.stat("solve_trans_passes") - passes[1], F.stat("lowrank_solves"),
               F.stat("lowrank_k"))
        msg = C.last_error(F._h)
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
        assert codes == [C.SMLU_ERR_STATE] * 8, (rank, codes)
        assert ran == (0, 0, 0, 0), (rank, ran)       # no solve ran and nothing is installed
        assert "single-GPU" in msg, msg
        assert resid < 1e-12, (rank, resid)
