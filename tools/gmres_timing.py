"""Dev: what solving with stale factors costs at 128^3 (smlu_solve_gmres_device).

Factor once on the bench's first value set (A + diag U(0,1), default_rng(47)), then in the same process
time one refactor, the plain smlu_solve_device, and GMRES on those factors for
  * the bench's later value sets (default_rng(48), (49), (50): every diagonal entry moves by up to 1),
  * entrywise relative perturbations of the factored values, (1 + delta u), u uniform in [-1, 1],
  * the factored values themselves (values = None: GMRES-based refinement).
Reports per case iterations, total ms, ms per iteration and per iteration beyond its factor solve, and
the number of iterations at which a refactor plus one solve is cheaper.

  python tools/gmres_timing.py [N] [--out DIR]      (default 128, profiles/gmres)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sharedmemsparselu.jl_amd"))

import numpy as np  # noqa: E402


def main():
    import torch
    import smlu
    from smlu import matrices as mats
    ap = argparse.ArgumentParser()
    ap.add_argument("N", type=int, nargs="?", default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmres"))
    ap.add_argument("--maxiter", type=int, default=200)
    args = ap.parse_args()
    N = args.N
    dev = torch.device("cuda:0")
    A = mats.poisson3d(N)
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A, device=0)
    dpos = torch.from_numpy(mats.diag_positions(A)).to(dev)
    base = torch.from_numpy(np.ascontiguousarray(A.data)).to(dev)

    def bench_values(seed):
        v = base.clone()
        v[dpos] += torch.from_numpy(np.random.default_rng(seed).random(n)).to(dev)
        return v

    def wall(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    factored = bench_values(47)
    F.refactor_device(factored)
    refactor_ms = wall(lambda: F.refactor_device(factored), 3)
    db = torch.from_numpy(np.random.default_rng(7).random(n)).to(dev)
    dx = torch.empty_like(db)
    F.solve_device(dx, db)
    solve_ms = wall(lambda: F.solve_device(dx, db), 7)
    F.solve_device(dx, db, trans="T")
    solve_t_ms = wall(lambda: F.solve_device(dx, db, trans="T"), 5)
    print(f"N={N} n={n}: refactor {refactor_ms:.1f} ms, solve {solve_ms:.2f} ms, transposed solve {solve_t_ms:.2f} ms",
          flush=True)

    cases = [(f"bench values seed {s}", bench_values(s), "N") for s in (48, 49, 50)]
    for delta in (1e-3, 1e-2, 5e-2):
        u = torch.from_numpy(np.random.default_rng(1000).uniform(-1.0, 1.0, A.nnz)).to(dev)
        cases.append((f"entrywise delta {delta:g}", factored * (1.0 + delta * u), "N"))
    u = torch.from_numpy(np.random.default_rng(1000).uniform(-1.0, 1.0, A.nnz)).to(dev)
    cases.append(("entrywise delta 0.01, transposed", factored * (1.0 + 1e-2 * u), "T"))
    cases.append(("own values (refinement)", None, "N"))
    rows = []
    for name, vals, op in cases:
        F.gmres_device(dx, db, vals, trans=op, maxiter=args.maxiter)       # first call: buffers, graphs
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = F.gmres_device(dx, db, vals, trans=op, maxiter=args.maxiter)
            t.append((time.perf_counter() - t0) * 1e3)
        total = float(np.median(t))
        one = solve_t_ms if op == "T" else solve_ms
        per_iter = total / max(info.iters, 1)
        beyond = (total - info.solves * one) / max(info.iters, 1)
        row = dict(case=name, op=op, converged=info.converged, iters=info.iters, cycles=info.cycles,
                   solves=info.solves, relres=info.relres, berr=info.berr, total_ms=total, ms_per_iter=per_iter,
                   ms_per_iter_beyond_solve=beyond, overhead_vs_solve=beyond / one,
                   break_even_iters=(refactor_ms + one) / per_iter)
        rows.append(row)
        print(f"{name}: converged {info.converged} iters {info.iters} cycles {info.cycles} solves {info.solves} "
              f"relres {info.relres:.2e} total {total:.1f} ms, {per_iter:.2f} ms/iter, {beyond:.2f} ms/iter beyond "
              f"the solve ({100 * beyond / one:.1f} % of it); a refactor + solve wins above "
              f"{row['break_even_iters']:.1f} iterations", flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"gmres_timing_{N}.json")
    with open(path, "w") as f:
        json.dump(dict(N=N, n=n, nnz=int(A.nnz), refactor_ms=refactor_ms, solve_ms=solve_ms, solve_trans_ms=solve_t_ms,
                       rtol=1e-10, restart=30, maxiter=args.maxiter, cases=rows), f, indent=1)
        f.write("\n")
    print("wrote", path)
    F.close()


if __name__ == "__main__":
    main()
