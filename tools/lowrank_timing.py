"""Dev: what a low-rank update costs at 128^3 (smlu_lowrank_set_device, smlu_solve_lowrank_device,
DESIGN §15).

Factor once on the bench's first value set (A + diag U(0,1), default_rng(47)), then in the same process
time one refactor, the plain solve of both directions and the batched solves at the widths a set runs,
and, for k in {1, 8, 16, 32} replaced columns (U[:, t] = A[:, j_t] * u, V = e_{j_t}),
  * lowrank_set,
  * solve_lowrank at steps 0 and -1, op N and T (the first transposed solve, which computes Yt, apart).
Medians of three after one untimed call.  Reports per call the time beyond its factor solves,
total - (sum of the plain solves it ran), as a share of one plain solve, and the k at which set + one
refined solve stops beating refactor + solve.

  python tools/lowrank_timing.py [N] [--out DIR]      (default 128, profiles/lowrank)"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowrank"))
    ap.add_argument("--ranks", type=int, nargs="*", default=[1, 8, 16, 32])
    args = ap.parse_args()
    N = args.N
    dev = torch.device("cuda:0")
    A = mats.poisson3d(N)
    n = A.shape[0]
    F = smlu.ParallelSparseLU(A, device=0)
    dpos = torch.from_numpy(mats.diag_positions(A)).to(dev)
    factored = torch.from_numpy(np.ascontiguousarray(A.data)).to(dev)
    factored[dpos] += torch.from_numpy(np.random.default_rng(47).random(n)).to(dev)
    vals = factored.cpu().numpy()

    def wall(fn, reps=3):
        fn()                                   # untimed: buffers, graphs
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    refactor_ms = wall(lambda: F.refactor_device(factored))
    db = torch.from_numpy(np.random.default_rng(7).random(n)).to(dev)
    dx = torch.empty_like(db)
    solve_ms = {op: wall(lambda: F.solve_device(dx, db, trans=op)) for op in ("N", "T")}
    batch_ms = {}
    for w in sorted({min(k, 16) for k in args.ranks}):
        dB = torch.from_numpy(np.random.default_rng(8).random((w, n))).to(dev)
        dX = torch.empty_like(dB)
        batch_ms[w] = {op: wall(lambda: F.solve_multi_device(dX, dB, trans=op)) for op in ("N", "T")}
        del dB, dX
    print(f"N={N} n={n}: refactor {refactor_ms:.1f} ms, solve {solve_ms['N']:.2f} ms, transposed {solve_ms['T']:.2f} ms, "
          + ", ".join(f"{w} columns {batch_ms[w]['N']:.1f} / {batch_ms[w]['T']:.1f} ms" for w in batch_ms), flush=True)

    def batches_ms(k, op):                     # the solve passes behind k columns
        return sum(batch_ms[min(16, k - j)][op] if min(16, k - j) in batch_ms else float("nan") for j in range(0, k, 16))

    rows = []
    for k in args.ranks:
        rng = np.random.default_rng(1000 + k)
        cols = np.sort(rng.choice(n, size=k, replace=False))
        dU = torch.zeros((k, n), dtype=torch.float64, device=dev)
        dV = torch.zeros((k, n), dtype=torch.float64, device=dev)
        for t, j in enumerate(cols):
            lo, hi = A.indptr[j], A.indptr[j + 1]
            dU[t, torch.from_numpy(A.indices[lo:hi].astype(np.int64)).to(dev)] = \
                torch.from_numpy(vals[lo:hi] * rng.uniform(-1.0, 1.0, hi - lo)).to(dev)
            dV[t, int(j)] = 1.0
        set_ms = wall(lambda: F.lowrank_set_device(dU, dV))
        si = F.lowrank_set_device(dU, dV)
        row = dict(k=k, set_ms=set_ms, set_solves=si.solves, set_beyond_ms=set_ms - batches_ms(k, "N"),
                   rcond_c=si.rcond_c, solves=[])
        print(f"k={k}: set {set_ms:.1f} ms ({si.solves} solve passes, {row['set_beyond_ms']:.2f} ms beyond them), "
              f"rcond_c {si.rcond_c:.2e}", flush=True)
        for op in ("N", "T"):
            if op == "T":                      # the first transposed solve after a set computes Yt
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                F.solve_lowrank_device(dx, db, trans="T", steps=0)
                torch.cuda.synchronize()
                row["first_trans_ms"] = (time.perf_counter() - t0) * 1e3
            for steps in (0, -1):
                info = []
                total = wall(lambda: info.append(F.solve_lowrank_device(dx, db, trans=op, steps=steps)))
                i = info[-1]
                beyond = total - i.solves * solve_ms[op]
                row["solves"].append(dict(op=op, steps=steps, total_ms=total, corrections=i.steps, stop=i.stop,
                                          factor_solves=i.solves, berr=i.berr, beyond_ms=beyond,
                                          beyond_share_of_solve=beyond / solve_ms[op]))
                print(f"  op {op} steps {steps}: {total:.2f} ms, {i.solves} factor solves, {i.steps} corrections, "
                      f"berr {i.berr:.2e}, {beyond:.2f} ms beyond the solves ({100 * beyond / solve_ms[op]:.1f} % of one)",
                      flush=True)
        refined = next(s for s in row["solves"] if s["op"] == "N" and s["steps"] == -1)
        row["set_plus_refined_ms"] = set_ms + refined["total_ms"]
        rows.append(row)
        del dU, dV
    target = refactor_ms + solve_ms["N"]
    beats = [r["k"] for r in rows if r["set_plus_refined_ms"] < target]
    loses = [r["k"] for r in rows if r["set_plus_refined_ms"] >= target]
    print(f"refactor + solve {target:.1f} ms; set + one refined solve: "
          + ", ".join(f"k={r['k']} {r['set_plus_refined_ms']:.1f} ms" for r in rows)
          + f"; beats it at k in {beats}, not at k in {loses}", flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"lowrank_timing_{N}.json")
    with open(path, "w") as f:
        json.dump(dict(N=N, n=n, nnz=int(A.nnz), refactor_ms=refactor_ms, solve_ms=solve_ms, batch_ms=batch_ms,
                       refactor_plus_solve_ms=target, ranks=rows), f, indent=1)
        f.write("\n")
    print("wrote", path)
    F.close()


if __name__ == "__main__":
    main()
