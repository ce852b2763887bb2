"""Solve timing on the 3D Poisson workload: one right-hand side (smlu_solve_device) and batches
of 8 / 16 (smlu_solve_multi_device), median of several device-resident runs.  Run under
`rocprofv3 --kernel-trace --stats` to split the time over the solve kernels.

    python tools/solve_timing.py [--side 128] [--reps 5]

--trans: the transposed solve (smlu_solve_trans_device, A^T x = b) against its yardstick, the
forward solve of a handle created under SMLU_SOLVE_STEPS=1 (the structurally identical per-block
launch sequences), both on one handle in one process: warm-up, then alternating blocks of --reps
solves each, median over all of them; host clock around a solve that ends in a device
synchronise, clocks as the device runs them (no pinning).

    python tools/solve_timing.py --trans [--side 128] [--reps 5]

--trans --nrhs K: the same protocol for K columns, the batched transposed solve
(solve_multi_device(..., trans="T")) against the forward solve_multi_device of the same columns on
the per-block sequences; prints both times, the ratio and the number of transposed pass pairs one
call took (K on a library that solves column by column, ceil(K / 16) with the batched kernels).

    python tools/solve_timing.py --trans --nrhs 8 [--side 128] [--reps 5]

--rcond: the condition estimate (smlu_rcond) beside the forward and transposed solves of the same
handle (the default schedule: forward on the sync-free sweeps), same protocol: warm-up, then
alternating blocks of --reps calls each, median over all of them.  Every timed estimate follows a
refactor of the same values (untimed), since the result is cached per factorization.  The yardstick
is the estimate's own solve counts times the two solve times; what is left is the estimator's
overhead (its elementwise kernels and record readbacks).  Also times smlu_logabsdet.

    python tools/solve_timing.py --rcond [--side 128] [--reps 5] [--norm 1]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sharedmemsparselu.jl_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trans", action="store_true")
    ap.add_argument("--nrhs", type=int, default=1, help="with --trans: columns per solve")
    ap.add_argument("--rcond", action="store_true")
    ap.add_argument("--norm", default="1", help='with --rcond: "1" or "inf"')
    args = ap.parse_args()
    if args.trans:
        os.environ["SMLU_SOLVE_STEPS"] = "1"   # read when the handle's schedule is built
    import torch
    import smlu
    from smlu import matrices as mats
    A = mats.poisson3d(args.side)
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A, profile=False)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    out = {"side": args.side, "n": n}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    b = torch.from_numpy(rng.random(n)).to(dev)
    x = torch.empty_like(b)
    if args.rcond:
        xt = torch.empty_like(b)
        vals = torch.from_numpy(np.ascontiguousarray(A.data)).to(dev)

        def clock(fn):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        fwd = lambda: F.solve_device(x, b)
        trn = lambda: F.solve_device(xt, b, trans="T")
        est = lambda: F.rcond(args.norm, parts=True)
        for fn in (fwd, trn, est, F.logabsdet):   # warm-up: code objects, buffers, the captured graphs
            fn()
        torch.cuda.synchronize()
        ts = {"fwd": [], "trans": [], "rcond": [], "logabsdet": []}
        res = set()
        for _ in range(3):      # alternating blocks
            for key, fn in (("fwd", fwd), ("trans", trn)):
                for _ in range(args.reps):
                    ts[key].append(clock(fn)[0])
            for _ in range(args.reps):
                F.refactor_device(vals)
                torch.cuda.synchronize()
                t, r = clock(est)
                ts["rcond"].append(t)
                res.add(r)
                ts["logabsdet"].append(clock(F.logabsdet)[0])
        assert len(res) == 1, res   # the same values: bitwise the same estimate
        for key, v in ts.items():
            out[f"ms_{key}"] = float(np.median(v))
            out[f"ms_{key}_min_max"] = (float(min(v)), float(max(v)))
        out["norm"] = args.norm
        out["rcond"], out["anorm"], out["ainvnorm"] = res.pop()
        nf, na = F.stat("rcond_solves_fwd"), F.stat("rcond_solves_adj")
        out["rcond_solves_fwd"], out["rcond_solves_adj"], out["rcond_iters"] = nf, na, F.stat("rcond_iters")
        out["ms_yardstick"] = nf * out["ms_fwd"] + na * out["ms_trans"]
        out["overhead_share"] = (out["ms_rcond"] - out["ms_yardstick"]) / out["ms_yardstick"]
        out["logabsdet"] = F.logabsdet()
        print(out, flush=True)
        return
    if args.trans:
        assert F.stat("solve_sweeps") == 0
        xt = torch.empty_like(b)
        fwd = lambda: F.solve_device(x, b)
        trn = lambda: F.solve_device(xt, b, trans="T")
        if args.nrhs > 1:
            out["nrhs"] = args.nrhs
            B = torch.from_numpy(rng.random((args.nrhs, n))).to(dev)
            X, Xt = torch.empty_like(B), torch.empty_like(B)
            fwd = lambda: F.solve_multi_device(X, B)
            trn = lambda: F.solve_multi_device(Xt, B, trans="T")
        ts = {"fwd": [], "trans": []}
        for fn in (fwd, trn):   # warm-up: code objects, the captured graphs
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        for _ in range(3):      # alternating blocks
            for key, fn in (("fwd", fwd), ("trans", trn)):
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ts[key].append((time.perf_counter() - t0) * 1e3)
        for key, v in ts.items():
            out[f"ms_{key}"] = float(np.median(v))
            out[f"ms_{key}_min_max"] = (float(min(v)), float(max(v)))
        out["ratio_trans_fwd"] = out["ms_trans"] / out["ms_fwd"]
        if args.nrhs > 1:
            passes = F.stat("solve_trans_passes")   # NaN on a library without the counter
            trn()
            out["trans_passes_per_call"] = F.stat("solve_trans_passes") - passes
            F.solve_device(xt, B[-1].contiguous(), trans="T")
            assert torch.equal(xt, Xt[-1])          # the last column is the single-vector solve, bitwise
            b, x = B[-1].contiguous(), X[-1]
        bh, xh = b.cpu().numpy(), xt.cpu().numpy()
        out["resid_trans"] = float(np.abs(A.T @ xh - bh).max() / np.abs(bh).max())
        out["resid_fwd"] = float(np.abs(A @ x.cpu().numpy() - bh).max() / np.abs(bh).max())
        print(out, flush=True)
        return
    out["ms_1"] = timed(lambda: F.solve_device(x, b))
    for k in (2, 4, 8, 16, 32):
        B = torch.from_numpy(rng.random((k, n))).to(dev)
        X = torch.empty_like(B)
        out[f"ms_{k}"] = timed(lambda: F.solve_multi_device(X, B))
        # columns agree with single-vector solves
        F.solve_device(x, B[k - 1].contiguous())
        assert torch.equal(x, X[k - 1]), k
    out["ratio_8"] = out["ms_8"] / out["ms_1"]
    print(out, flush=True)


if __name__ == "__main__":
    main()
