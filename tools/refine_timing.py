"""Dev: what refining several right-hand sides as a batch saves at 128^3 (smlu_solve_refined_multi_device,
DESIGN §14).

The matrix has the 3D Poisson pattern with values that are not diagonally dominant, so that the default
options refine (smlu_opts.refine = -1): poisson3d(N) with 1 added to every diagonal entry (7 instead of
6) and every off-diagonal entry -1 multiplied by 1 + 0.4 u, u uniform in [-1, 1] from default_rng(61).
A row's off-diagonal moduli then sum to 6 on average and to more than 7 in a few percent of the rows
and of the columns, which is what makes the handle refine; the matrix stays far from singular.

On one handle, in one process, for op N and T and 1, 8 and 16 columns: the new call
(solve_refined_multi_device) against the existing solve_multi_device, which under refinement runs one
refined solve per column.  Both are warmed up once (work buffers, solve graphs), then timed
alternately, a host clock around calls that end synchronised, and reported as medians.  The two
results must be bitwise equal.  A plain batch (steps=0, one pass, nothing refined) is timed next to them:
what one pass costs at that width.  Pass counts come from "solve_passes" / "solve_trans_passes".

  python tools/refine_timing.py [N] [--out DIR] [--reps R]      (default 128, profiles/refine, 7)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sharedmemsparselu.jl_amd"))

import numpy as np  # noqa: E402

VALUES = ("poisson3d(N) pattern; diagonal 6 + 1; off-diagonal -1 * (1 + 0.4 u), u uniform in [-1, 1], "
          "numpy default_rng(61), in CSC order")


def nondominant_poisson3d(N):
    from smlu import matrices as mats
    A = mats.poisson3d(N)
    dpos = mats.diag_positions(A)
    off = np.ones(A.nnz, bool)
    off[dpos] = False
    u = np.random.default_rng(61).uniform(-1.0, 1.0, int(off.sum()))
    A.data[dpos] += 1.0
    A.data[off] *= 1.0 + 0.4 * u
    return A


def main():
    import torch
    import smlu
    ap = argparse.ArgumentParser()
    ap.add_argument("N", type=int, nargs="?", default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    N = args.N
    dev = torch.device("cuda:0")
    A = nondominant_poisson3d(N)
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A, device=0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"N={N} n={n} nnz={A.nnz}; values: {VALUES}")
    say(f"dominant {F.stat('dominant'):.0f}, weak pivots {F.stat('weak'):.0f}, growth {F.stat('growth_max'):.3g}, "
        f"refactor {F.stat('refactor_ms_last'):.1f} ms; default options (refine = -1)")
    if F.stat("dominant") != 0:
        raise SystemExit("the values came out dominant: nothing would be refined")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    rows = []
    Ball = torch.from_numpy(np.random.default_rng(62).random((16, n))).to(dev)
    for trans in ("N", "T"):
        key = "solve_passes" if trans == "N" else "solve_trans_passes"
        for nrhs in (1, 8, 16):
            B = Ball[:nrhs].contiguous()
            Xn = torch.full_like(B, float("nan"))
            Xo = torch.full_like(B, float("nan"))
            new = lambda: F.solve_refined_multi_device(Xn, B, trans=trans)   # noqa: E731
            old = lambda: F.solve_multi_device(Xo, B, trans=trans)           # noqa: E731
            Xp = torch.empty_like(B)
            plain = lambda: F.solve_refined_multi_device(Xp, B, trans=trans, steps=0)   # noqa: E731
            new()
            old()                                                            # warm-up of both paths
            tn, to, tp = [], [], []
            for _ in range(args.reps):                                       # alternating
                p0 = F.stat(key)
                r0 = F.stat("refine_batch_residuals")
                t, info = timed(new)
                tn.append(t)
                passes_new = int(F.stat(key) - p0)
                rounds = int(F.stat("refine_batch_residuals") - r0)
                p0 = F.stat(key)
                t, _ = timed(old)
                to.append(t)
                passes_old = int(F.stat(key) - p0)
                tp.append(timed(plain)[0])                                   # one unrefined pass at this width
            steps = [int(s) for s in info["steps"]]
            assert passes_new == 1 + max(steps), (passes_new, steps)
            assert passes_old == sum(1 + s for s in steps), (passes_old, steps)
            same = bool(torch.equal(Xn, Xo))
            row = dict(op=trans, nrhs=nrhs, steps=steps, stop=[int(s) for s in info["stop"]],
                       berr_max=float(info["berr"].max()), passes_batched=passes_new, passes_column_loop=passes_old,
                       residual_launches_batched=rounds, ms_batched=float(np.median(tn)),
                       ms_column_loop=float(np.median(to)), ms_plain_batch=float(np.median(tp)),
                       ms_batched_all=tn, ms_column_loop_all=to, ms_plain_batch_all=tp,
                       bitwise_equal=same)
            rows.append(row)
            say(f"op {trans} nrhs {nrhs:2d}: steps per column {steps}; passes {passes_new} batched "
                f"(1 + max steps) against {passes_old} column by column (sum of 1 + steps); "
                f"{rounds} batched residual launches; median of {args.reps}: {row['ms_batched']:.1f} ms batched "
                f"[{min(tn):.1f}, {max(tn):.1f}], {row['ms_column_loop']:.1f} ms column loop "
                f"[{min(to):.1f}, {max(to):.1f}], ratio {row['ms_column_loop'] / row['ms_batched']:.2f}; "
                f"one unrefined batch (steps=0) {row['ms_plain_batch']:.1f} ms; "
                f"largest berr {row['berr_max']:.2e}; results bitwise equal: {same}")
            if not same:
                raise SystemExit("the two paths differ")
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"refine_{N}.json"), "w") as f:
        json.dump(dict(N=N, n=n, nnz=int(A.nnz), values=VALUES, reps=args.reps, cases=rows), f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, f"refine_{N}.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    say(f"wrote {args.out}/refine_{N}.json and .txt")
    F.close()


if __name__ == "__main__":
    main()
