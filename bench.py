#!/usr/bin/env python3
"""bench.py — numeric sparse-LU refactorization throughput on MI355X (BASELINE.json metric).

Step = one numeric refactorization (lu!(F, A): same pattern, new values) of the 3D 7-point
Poisson matrix (default 128^3, BASELINE config C3/C5), values already resident in HBM.
Prints ONE JSON line (rank 0).  Launch: ``python bench.py`` (1 GPU) or, for N GPUs,
``python -m torch.distributed.run --nproc-per-node N bench.py --gpus N``.

A plain run sets up, warms up, times `--steps` refactorizations and prints the line (metric, value,
ms_per_step, the per-kernel HIP-event times of those same steps).  `--full` adds, after the timed
steps, everything else: solves and their residual, the refactor with host values, the ordering
comparison, the CPU baselines and the C1/C2/C5 configs (`--no-cpu`, `--no-configs`: the full run
without those legs).  `--dump-outputs DIR` writes what the last
timed step computed as DIR/<name>.npy; the inputs are seeded, so two builds run with the same
arguments can be compared file by file.

Multi-GPU (N > 1): ONE factorization split over the ranks — subtrees of the assembly tree per
rank, update blocks moved at exchange points over RCCL point-to-point ("scaling": "strong";
`--replicas` runs independent copies instead).  DESIGN.md §7.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "sharedmemsparselu.jl_amd"))

FP64_PEAK_TFLOPS = 78.6   # MI355X fp64 dense peak (vector == matrix on gfx950), AMD spec
HBM_PEAK_GBS = 8000.0     # MI355X HBM3E peak, MI355X_MICROARCH.md


def log(*a):
    print("[bench]", *a, file=sys.stderr, flush=True)


def cpu_threads():
    """Host threads for the CPU baseline: OMP_NUM_THREADS when set (the GPU box sets it to its CPU
    share, 16), else every core this process may run on."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    env = os.environ.get("OMP_NUM_THREADS")
    return max(1, min(aff, int(env))) if env and env.isdigit() else aff


def cpu_baseline(N_head, flops_head, nnz_head, grid_hint, samples=(64, 108), reps=(3, 1)):
    """CPU baseline on the GPU box's host, reported beside the GPU number:

    * value: the multifrontal CPU port (oracle/mf.c: the same assembly tree as the GPU plan,
      threshold partial pivoting inside every front, AVX2 register-blocked updates, OpenMP tasks
      over the assembly tree and inside the large fronts) refactoring ONE matrix on all host threads
      (`cores`).  Each sample size is factored once untimed (heap growth, page faults), then timed
      `reps` times (median).  The headline is the 108^3 refactor scaled by the flop ratio to 128^3
      (2.8x: the CPU's rate still rises with size, so this is a conservative, i.e. fast, CPU
      estimate); 64^3 gives the rate's size trend.  The reference's own path (UMFPACK through Julia)
      does not exist on the box.  tools/cpu_c3.py times the full 128^3 refactor directly (a
      profile, not the default bench: ~2 minutes).
    * single_core: the same port on one thread at 40^3 (the reference's UMFPACK runs single-threaded).
    * superlu: scipy's SuperLU (splu, MMD on A'+A, diag_pivot_thresh 0.1) at C2, a third-party anchor.
    * c1_chunked_solve: the reference's own dense-chunk solve (oracle.ChunkedSolve, a line-by-line
      restatement of get_chunking_parameters / fill_chunks! / lsolve! / rsolve!, :101-392) at C1."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    import scipy.sparse.linalg as spla
    import smlu
    from smlu import matrices as mats
    threads = cpu_threads()

    def mf_time(N, th, nrep=1):
        A = mats.poisson3d(N)
        A.sort_indices()
        P = smlu.Plan(A, grid=(N,) * 3 if grid_hint else None)
        first, parent, rowptr, rows, p0 = P.fronts()
        fr = dict(first=first, parent=parent, rowptr=rowptr, rows=rows, p0=p0)
        mf = O.MultifrontalOracle(A, P.q(), fr, None, threads=th)
        st = mf.factor(A.data)   # untimed: heap growth and page faults of the first factorization
        ts = []
        for _ in range(nrep):
            t0 = time.perf_counter()
            st = mf.factor(A.data)   # the timed refactor (same pattern, as lu!)
            ts.append(time.perf_counter() - t0)
        mf.close()
        assert st == 0
        dt = float(np.median(ts))
        return {"N": N, "seconds": dt, "timings": ts, "dense_flops": P.stat("dense_flops"), "upd": P.stat("upd"),
                "nnzLU": P.stat("nnzLU"), "nnzLU_per_s": P.stat("nnzLU") / dt,
                "gflops": P.stat("dense_flops") / dt / 1e9}

    rows = []
    for N, k in zip(samples, reps):
        rows.append(mf_time(N, threads, k))
        log(f"cpu baseline {N}^3 on {threads} threads: {rows[-1]['timings']} s, "
            f"{rows[-1]['gflops']:.1f} GFLOP/s")
    big = rows[-1]
    ratio = flops_head / big["dense_flops"]
    t_head = big["seconds"] * ratio
    alpha = float(np.log(big["seconds"] / rows[0]["seconds"]) / np.log(big["dense_flops"] / rows[0]["dense_flops"]))
    res = {"value": nnz_head / t_head, "unit": "nnz(L+U)/s", "cores": threads, "kind": "port",
           "nproc": os.cpu_count(),
           "sample": (f"multifrontal CPU port (oracle/mf.c, same plan, partial pivoting, OpenMP on "
                      f"{threads} threads, AVX2): 3D Poisson {big['N']}^3 refactor "
                      f"{big['seconds']:.1f} s ({big['gflops']:.0f} GFLOP/s), scaled by the flop ratio "
                      f"{ratio:.2f}x to {N_head}^3: {t_head:.1f} s per refactor"),
           "extrapolated": True, "extrapolation_factor": ratio, "headline_seconds": t_head,
           "time_vs_flops_exponent_64_to_largest": alpha, "samples": rows}
    one = mf_time(40, 1)
    res["single_core"] = dict(one, cores=1)
    log(f"cpu baseline 40^3 on 1 thread: {one['seconds']:.2f} s")
    A2 = mats.poisson2d(512)
    t0 = time.perf_counter()
    lu = spla.splu(A2.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.1)
    t_c2 = time.perf_counter() - t0
    res["superlu"] = {"kind": "third-party", "cores": 1, "c2_poisson2d_512_seconds": t_c2,
                      "c2_nnzLU": int(lu.L.nnz + lu.U.nnz - A2.shape[0]),
                      "note": "scipy.sparse.linalg.splu (SuperLU), MMD on A'+A, diag_pivot_thresh 0.1"}
    # C1: the reference's chunked solve, restated verbatim, on its own CPU layout
    A1 = mats.random_dominant(1000, 0.01, seed=47)
    q1 = smlu.Plan(A1).q()   # the GPU plan's column order; diagonal pivots (row-dominant C1)
    ref = O.OracleLU(A1, q1, q1)
    cs = O.ChunkedSolve(ref.L, ref.U)
    b1 = np.random.default_rng(3).random(A1.shape[0])
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        w = ref.Rs * b1
        cs.lsolve(w)
        cs.rsolve(w)
    res["c1_chunked_solve"] = {"ms_per_solve": (time.perf_counter() - t0) / reps * 1e3, "cores": 1,
                               "chunks": cs.total_chunks,
                               "note": "oracle.ChunkedSolve: trsv on 8x8 diagonal chunks + gemv on the "
                                       "negated dense rectangles (src/SharedMemSparseLU.jl:349-392)"}
    return res


def gpu_configs(dev):
    """The BASELINE configs besides the headline, on this GPU (reported, not the metric):
    C1 factorize + solve (1000x1000 random 1 %); C2 factorize + solve (2D 5-point Poisson 512^2);
    C5 steady state: 1000 numeric refactorizations of C2 with new values (8 value sets cycled,
    resident in HBM), the solution checked after the last one."""
    import torch
    import smlu
    from smlu import matrices as mats
    out = {}
    A1 = mats.random_dominant(1000, 0.01, seed=47)
    t0 = time.perf_counter()
    F1 = smlu.ParallelSparseLU(A1, device=dev.index)
    c1_create = time.perf_counter() - t0
    b1 = np.random.default_rng(3).random(A1.shape[0])
    x1 = np.empty_like(b1)
    smlu.ldiv_(x1, F1, b1)
    t0 = time.perf_counter()
    for _ in range(20):
        smlu.ldiv_(x1, F1, b1)
    out["c1"] = {"create_s": c1_create, "solve_ms_host_vectors": (time.perf_counter() - t0) / 20 * 1e3,
                 "residual": float(np.abs(A1 @ x1 - b1).max() / np.abs(b1).max()), "nnzLU": F1.stat("nnzLU")}
    F1.close()
    A2 = mats.poisson2d(512)
    n2 = A2.shape[0]
    t0 = time.perf_counter()
    F2 = smlu.ParallelSparseLU(A2, device=dev.index)
    c2_create = time.perf_counter() - t0
    dpos = torch.from_numpy(mats.diag_positions(A2)).to(dev)
    base = torch.from_numpy(np.ascontiguousarray(A2.data)).to(dev)
    vals = []
    for r in range(8):
        v = base.clone()
        v[dpos] += torch.from_numpy(np.random.default_rng(100 + r).random(n2)).to(dev)
        vals.append(v)
    b = torch.from_numpy(np.random.default_rng(5).random(n2)).to(dev)
    x = torch.empty_like(b)
    F2.refactor_device(vals[0])
    F2.solve_device(x, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    F2.refactor_device(vals[1])
    torch.cuda.synchronize()
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    F2.solve_device(x, b)
    torch.cuda.synchronize()
    t_sol = time.perf_counter() - t0
    hv = vals[2].cpu().numpy()   # lu! with host values (smlu_refactor), median of 5
    th = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        F2.refactor(hv)
        torch.cuda.synchronize()
        th.append((time.perf_counter() - t0) * 1e3)
    R = 1000
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(R):
        F2.refactor_device(vals[r % 8])
    torch.cuda.synchronize()
    t_ss = time.perf_counter() - t0
    F2.solve_device(x, b)
    Al = A2.copy()
    Al.data = vals[(R - 1) % 8].cpu().numpy()
    xh, bh = x.cpu().numpy(), b.cpu().numpy()
    nnz2 = F2.stat("nnzLU")
    out["c2"] = {"create_s": c2_create, "refactor_ms": t_ref * 1e3, "refactor_host_values_ms": float(np.median(th)),
                 "solve_ms": t_sol * 1e3,
                 "factorize_plus_solve_ms": (t_ref + t_sol) * 1e3, "nnzLU": nnz2,
                 "nnzLU_per_s": nnz2 / t_ref}
    out["c5_steady_state_c2"] = {"refactors": R, "seconds": t_ss, "ms_per_refactor": t_ss / R * 1e3,
                                 "nnzLU_per_s": nnz2 * R / t_ss,
                                 "residual_after": float(np.abs(Al @ xh - bh).max() / np.abs(bh).max())}
    F2.close()
    return out


def ordering_compare(N):
    """nnz(L+U) and upd = sum_k |L_k||U_k| of the native orderings on the headline config (C3) and
    on C2 (2D 512^2): graph nested dissection (the default) against SMLU_ORDER_AMD, the
    minimum-degree ordering of UMFPACK's symmetric strategy.  Host symbolic
    analysis only, outside the timed region."""
    import smlu
    from smlu import matrices as mats
    out = {}
    for name, A in ((f"c3_poisson3d_{N}", mats.poisson3d(N)), ("c2_poisson2d_512", mats.poisson2d(512))):
        row = {}
        for o in ("nd", "amd"):
            t0 = time.perf_counter()
            P = smlu.Plan(A, ordering=o)
            row[o] = {"nnzLU": P.stat("nnzLU"), "upd": P.stat("upd"),
                      "analysis_s": round(time.perf_counter() - t0, 2)}
        out[name] = row
    return out


def kernel_source_sha():
    """Hash of the library sources: a committed PMC profile applies to this build only if its
    recorded hash matches (otherwise its traffic numbers are stale and are not reported)."""
    import hashlib
    hs = hashlib.sha1()
    d = os.path.join(ROOT, "sharedmemsparselu.jl_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".cpp", ".hpp")):
            with open(os.path.join(d, f), "rb") as fh:
                hs.update(f.encode() + fh.read())
    return hs.hexdigest()[:12]


DUMP_FACTOR_DOUBLES = 1 << 21   # --dump-outputs: sampled doubles of the factor store (16 MiB)
DUMP_CHUNK = 4096               # ... read in runs of this many consecutive doubles
DUMP_SEED = 47


def factor_sample(F, total=DUMP_FACTOR_DOUBLES, chunk=DUMP_CHUNK, seed=DUMP_SEED):
    """A fixed sample of the factor values a one-GPU handle holds (128^3: 2.9e9 doubles, far more
    than a dump may hold).  The values are the fronts' L panels (M x ns) and U12 blocks (ns x nu)
    laid end to end in front order; `total // chunk` run starts are drawn from default_rng(seed)
    over that concatenation (so a front is sampled in proportion to its size) and each run is
    `chunk` doubles, cut at the end of its block.  The plan fixes the layout, so two builds with
    the same plan sample the same entries.  Returns (values, store offsets of the runs)."""
    from smlu import _lib as C
    L = C.lib()
    ns = int(F.stat("nsuper"))
    off = np.empty(4 * ns, np.int64)
    rc = L.smlu_dev_front_offsets(F._h, C.ptr(off))
    assert rc == 0, C.last_error(F._h)
    off = off.reshape(ns, 4)
    w = np.diff(F.fronts()["first"])                 # pivot columns per front
    M = off[:, 3]
    start = np.concatenate([off[:, 0], off[:, 1]])   # L panels, then U12 blocks
    length = np.concatenate([M * w, w * (M - w)])
    keep = length > 0
    start, length = start[keep], length[keep]
    cum = np.concatenate([[0], np.cumsum(length)])
    assert cum[-1] > 0, "the handle holds no factor values"
    nrun = max(1, min(total // chunk, int(cum[-1]) // chunk))
    at = np.sort(np.random.default_rng(seed).integers(0, cum[-1], size=nrun))
    seg = np.searchsorted(cum, at, side="right") - 1
    vals, offs = [], []
    for a, s in zip(at, seg):
        o = int(start[s] + (a - cum[s]))
        cnt = int(min(chunk, start[s] + length[s] - o))
        buf = np.empty(cnt)
        rc = L.smlu_dev_copy(F._h, 0, o, cnt, C.ptr(buf), None)   # range-checked by the library
        assert rc == 0, C.last_error(F._h)
        vals.append(buf)
        offs.append(o)
    return np.concatenate(vals), np.asarray(offs, np.float64)


def dump_outputs(path, F, x, partitioned, rank):
    """--dump-outputs: what the last timed refactor left in the handle, as float64 .npy files (32.6 MB
    at 128^3; 33.6 MB if no run were cut): `x`, the solution of A x = b on those factors (b = default_rng(5): the whole
    factorization, pivots and row scaling included, in one vector), and on one GPU a seeded sample
    of the factor values (factor_sample) with the store offsets of its runs.  F.p, F.q and F.Rs are
    left out: the library hands them out only with a host export of all of L and U (47 GB here);
    F.perm_scale() does not avoid that, it passes NULL factor pointers to smlu_get_factors, which
    builds the whole export before it looks at them."""
    if rank != 0:
        return
    os.makedirs(path, exist_ok=True)
    if x.size > DUMP_FACTOR_DOUBLES:   # sides above 128: entries at sorted indices from the seed
        x = x[np.sort(np.random.default_rng(DUMP_SEED).choice(x.size, DUMP_FACTOR_DOUBLES, replace=False))]
    out = {"x": x}
    if not partitioned:
        out["factor_sample"], out["factor_sample_offsets"] = factor_sample(F)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    log(f"wrote {sorted(out)} to {path} ({sum(a.size for a in out.values()) * 8 / 1e6:.1f} MB)")


def max_over_ranks(x, device=None):
    """Max of a float over all ranks (identity when torch.distributed is not initialised)."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return x
    t = torch.tensor([x], dtype=torch.float64, device=device or "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def timed_region(step, steps, warmup, sync, device=None):
    """Contract of the driver: W untimed warmup steps, then EXACTLY `steps` steps bracketed by
    a barrier + device sync on both sides; returns the MAX wall time over ranks."""
    import torch.distributed as dist
    dist_on = dist.is_available() and dist.is_initialized()
    for r in range(warmup):
        step(r)
    if dist_on:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for r in range(steps):
        step(warmup + r)
    sync()
    if dist_on:
        dist.barrier()
    return max_over_ranks(time.perf_counter() - t0, device)


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n):
    """`python bench.py --gpus N` (N > 1, no WORLD_SIZE in the environment): run this script under
    torch.distributed.run with N ranks on this node (127.0.0.1 rendezvous) and return their exit
    status.  The child launcher is a subprocess; this process never initialises the GPU."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    log(f"--gpus {n} without a launcher: starting {n} ranks: {' '.join(cmd[1:6])} ...")
    return subprocess.call(cmd)


def init_gloo():
    """Control-plane process group (barriers, max-over-ranks timing, the RCCL unique id).  gloo
    prints its connection banner on the C-level stdout: keep stdout for the JSON line."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        dist.init_process_group("gloo")
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


def launch_check(rank, world, local):
    """The launcher path alone: every rank joins a gloo group and reports itself; rank 0 prints
    {"launch_check": true, "world": W, "ranks": [...]} (no GPU call)."""
    import torch.distributed as dist
    if world > 1:
        init_gloo()
    me = {"rank": rank, "local_rank": local, "pid": os.getpid()}
    allr = [None] * world
    if world > 1:
        dist.all_gather_object(allr, me)
    else:
        allr = [me]
    if rank == 0:
        print(json.dumps({"launch_check": True, "world": world, "ranks": allr}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


def side_legs(args, world, partitioned):
    """Which side measurements run after the timed steps: (full, cpu, configs).  `full` (solves and
    their residual, the refactor with host values) is asked for by --full, by --no-cpu / --no-configs
    (they name a leg of the full run to leave out) and by --check-single on a partitioned run (it
    compares solutions); `cpu` (ordering comparison, CPU baselines) and `configs` (C1/C2/C5) are
    legs of the full run on one GPU."""
    full = bool(args.full or args.no_cpu or args.no_configs or (args.check_single and partitioned))
    return full, full and not args.no_cpu and world == 1, full and not args.no_configs and world == 1


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--side", "--n", dest="n", type=int, default=128,
                    help="grid side of the 3D Poisson workload")
    ap.add_argument("--ordering", default="nd", choices=["nd", "geometric"])
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what the headline does not need: solves and "
                         "their residual, the refactor with host values, the ordering comparison, the CPU "
                         "baselines and the C1/C2/C5 configs (minutes; a plain run skips all of them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed to DIR/<name>.npy "
                         "(float64, under 64 MB; see dump_outputs)")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the CPU legs (implies --full)")
    ap.add_argument("--no-configs", action="store_true",
                    help="--full without the C1/C2/C5 side measurements (implies --full)")
    ap.add_argument("--no-profile", action="store_true", help="skip per-kernel HIP events")
    ap.add_argument("--test-one-gpu", action="store_true",
                    help="rehearsal: all ranks on cuda:0, gloo transport (never for measurements)")
    ap.add_argument("--one-gpu-transport", default="host", choices=["host", "device"],
                    help="--test-one-gpu: the host-memory transport, or the RCCL calling convention "
                         "(device buffers on the library's stream) carried over gloo")
    ap.add_argument("--check-single", action="store_true",
                    help="partitioned run: after the timed steps, rank 0 factors the last values on one GPU "
                         "and every rank's solution is compared with that one (rehearsals, VERDICT r05); "
                         "the line then also carries --full's solve time and residual")
    ap.add_argument("--replicas", action="store_true",
                    help="N > 1: independent replicas instead of the partitioned factorization")
    ap.add_argument("--launch-check", action="store_true",
                    help="launcher check only: every rank reports (rank, world) over gloo, rank 0 prints "
                         "one JSON line; no GPU call (tests/test_bench_launch.py)")
    return ap.parse_args(argv)


def main():
    args = parse_args()

    # --gpus N without a launcher: start the N ranks here, before anything touches the GPU, as
    # child processes of torch.distributed.run (never an exec), and exit with their status.
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    import torch
    import torch.distributed as dist
    if args.launch_check:
        sys.exit(launch_check(rank, world, local))
    if args.test_one_gpu:
        local = 0
    if world > 1:
        # control plane (barriers, the max-over-ranks timing, the RCCL unique id) over gloo; the
        # data path is the library's own RCCL communicator (xGMI point-to-point), so a process
        # holds exactly one RCCL instance
        torch.cuda.set_device(local)
        init_gloo()
    else:
        torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")

    import smlu
    from smlu import matrices as mats
    N = args.n
    t0 = time.perf_counter()
    A = mats.poisson3d(N)
    n = A.shape[0]
    log(f"rank {rank}: generated 3D Poisson {N}^3 n={n} nnz={A.nnz} in {time.perf_counter()-t0:.1f}s")
    grid = (N, N, N) if args.ordering == "geometric" else None
    partitioned = world > 1 and not args.replicas
    t0 = time.perf_counter()
    if partitioned:   # one factorization split over the ranks (subtrees + RCCL exchanges)
        F = smlu.DistributedSparseLU(A, device=local, ordering=args.ordering,
                                     transport=args.one_gpu_transport if args.test_one_gpu else "rccl",
                                     **({"grid": grid} if grid else {}))
    else:
        F = smlu.ParallelSparseLU(A, grid=grid, device=local, profile=not args.no_profile)
    t_create = time.perf_counter() - t0
    nnzLU = F.stat("nnzLU")
    log(f"rank {rank}: analysis {F.stat('analysis_ms')/1e3:.1f}s, create+first factor {t_create:.1f}s, "
        f"nnz(L+U)={nnzLU:.4g}, upd={F.stat('upd'):.4g}, launches={F.stat('launches'):.0f}"
        + (f", comm steps={F.stat('comm_steps'):.0f}, shared fronts={F.stat('shared_fronts'):.0f}" if partitioned else ""))

    # C5 inputs: same pattern, new values (diag += U(0,1) from default_rng(47+r)), uploaded to HBM
    dpos = torch.from_numpy(mats.diag_positions(A)).to(dev)
    base = torch.from_numpy(np.ascontiguousarray(A.data)).to(dev)
    vals = []
    for r in range(args.warmup + args.steps):
        v = base.clone()
        d = torch.from_numpy(np.random.default_rng(47 + r).random(n)).to(dev)
        v[dpos] += d
        vals.append(v)
    torch.cuda.synchronize()

    kinds = ["gemm", "gemmu", "gemmo", "gemm22", "panel", "trsm", "urows", "small", "assemble"]
    kind_ms = {k: 0.0 for k in kinds}

    def step(r):
        F.refactor_device(vals[r])
        if r >= args.warmup and not partitioned:
            for k in kinds:
                kind_ms[k] += F.stat("ms_" + k)
        log(f"rank {rank}: {'warmup' if r < args.warmup else 'step'} {r} refactor "
            f"{F.stat('refactor_ms_last'):.1f} ms")

    dt = timed_region(step, args.steps, args.warmup, torch.cuda.synchronize)
    full, cpu_leg, configs_leg = side_legs(args, world, partitioned)
    solve_ms = solve8_ms = solve_residual = refactor_host_ms = None
    xh = None
    if full or args.dump_outputs:
        # one solve on the last timed step's factors (reported under --full, not the metric)
        b = torch.from_numpy(np.random.default_rng(5).random(n)).to(dev)   # same b on every rank
        x = torch.empty_like(b)
        F.solve_device(x, b)
        torch.cuda.synchronize()
        xh = x.cpu().numpy()
    if args.dump_outputs:   # before anything below refactors again
        dump_outputs(args.dump_outputs, F, xh, partitioned, rank)
    if full:
        t1 = time.perf_counter()
        F.solve_device(x, b)
        torch.cuda.synchronize()
        solve_ms = (time.perf_counter() - t1) * 1e3
    # eight right-hand sides in one batched call (single GPU)
    if full and not partitioned and hasattr(F, "solve_multi_device"):
        B8 = torch.from_numpy(np.random.default_rng(6).random((8, n))).to(dev)
        X8 = torch.empty_like(B8)
        F.solve_multi_device(X8, B8)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        F.solve_multi_device(X8, B8)
        torch.cuda.synchronize()
        solve8_ms = (time.perf_counter() - t1) * 1e3
    if full:
        # residual of that solve on the last refactored values (host SpMV)
        Al = A.copy()
        Al.data = vals[-1].cpu().numpy()
        bh = b.cpu().numpy()
        solve_residual = float(np.abs(Al @ xh - bh).max() / np.abs(bh).max())
    # lu!(F, A) with HOST values (the Julia shim's smlu_refactor: pageable upload of the values, the
    # dominance test on the device, the factorization) -- a side figure beside the resident-values
    # metric (within 3 % of ms_per_step)
    if full and not partitioned:
        hv = [vals[r % len(vals)].cpu().numpy() for r in range(2)]
        F.refactor(hv[1])
        th = []
        for r in range(3):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            F.refactor(hv[r % 2])
            torch.cuda.synchronize()
            th.append((time.perf_counter() - t1) * 1e3)
        refactor_host_ms = float(np.median(th))
        log(f"refactor with host values: {th} ms")
    ms_per_step = dt / args.steps * 1e3
    # per-rank evidence of the partitioned run: the communicator's own rank count and what this rank
    # moved in its last refactor (gathered to rank 0 over the gloo control plane)
    me = {"rank": rank, "device": local, "create_s": round(t_create, 3),
          "refactor_ms_last": F.stat("refactor_ms_last")}
    if partitioned:
        me.update({"rccl_nranks": int(F.stat("rccl_nranks")), "comm_steps": int(F.stat("comm_steps")),
                   "comm_bytes_sent_refactor": F.stat("comm_bytes_sent_refactor"),
                   "comm_bytes_recv_refactor": F.stat("comm_bytes_recv_refactor"),
                   "shared_fronts": int(F.stat("shared_fronts")),
                   "store_bytes_rank": F.stat("store_bytes_rank")})
    fst = {k: F.stat(k) for k in ['dense_flops', 'gemm22_flops', 'gemm_bytes', 'gemm_flops', 'gemm_launches', 'launches', 'upd']}   # the handle's figures for the line (before any close)
    if args.check_single and partitioned:
        # the partitioned solution against the single-GPU factorization of the same values (the
        # partitioned handles are released first: on a one-GPU rehearsal they share the card)
        F.close()
        dist.barrier()
        xs = torch.zeros(n, dtype=torch.float64)
        if rank == 0:
            Fs = smlu.ParallelSparseLU(A, grid=grid, device=local)
            Fs.refactor_device(vals[-1])
            xd = torch.empty_like(b)
            Fs.solve_device(xd, b)
            torch.cuda.synchronize()
            xs = xd.cpu()
            Fs.close()
        dist.broadcast(xs, 0)
        xs = xs.numpy()
        me["x_vs_single_gpu_max_rel"] = float(np.abs(xh - xs).max() / np.abs(xs).max())
        me["single_gpu_residual"] = float(np.abs(Al @ xs - bh).max() / np.abs(bh).max())
    per_rank = [me]
    if world > 1:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, me)

    if rank == 0:
        K = args.steps
        gemm_flops = fst["gemm_flops"]
        ms_gemm = (kind_ms["gemm"] + kind_ms["gemmu"] + kind_ms["gemmo"] + kind_ms["gemm22"]) / K
        upd = fst["upd"]
        dense_flops = fst["dense_flops"]
        achieved = gemm_flops / (ms_gemm * 1e-3) / 1e12 if ms_gemm > 0 else None
        n_gemm = fst["gemm_launches"]
        avg_us = ms_gemm * 1e3 / n_gemm if (n_gemm and ms_gemm > 0) else None
        # PMC traffic comes from a committed rocprofv3 profile (profiles/<round>/pmc_gemm_N.json);
        # it is reported only when that profile was taken from this exact library source
        # (kernels_sha) on the single-GPU path, otherwise null.
        sha = kernel_source_sha()
        traffic, traffic_src, hbm_refactor, pm = None, "no profile of this build", None, None
        import glob
        for pmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", f"pmc_gemm_{N}.json")), reverse=True):
            with open(pmc) as fh:
                cand = json.load(fh)
            if cand.get("kernels_sha") == sha:
                pm, traffic_src = cand, os.path.relpath(pmc, ROOT)
                break
        if pm is not None and not partitioned:
            traffic = pm.get("hbm_bytes_per_launch")
            hbm_refactor = pm.get("refactor_all_kernels", {}).get("hbm_bytes")
        nnzA = A.nnz
        res = {
            "metric": "nnz(L+U)/s + achieved HBM GB/s, 3D Poisson 128³ numeric LU, 1/2/4/8 GPU",
            "value": nnzLU * (1 if partitioned else world) / (ms_per_step * 1e-3),
            "unit": "nnz(L+U)/s",
            "n_gpus": world,
            "steps": K,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong" if partitioned else "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"3D 7-point Poisson {N}^3 numeric refactorize (same pattern, "
                                   f"new diagonal values per step, values resident in HBM)",
                       "n": n, "nnzA": int(nnzA), "nnzLU": nnzLU, "upd": upd,
                       "dense_flops": dense_flops, "ordering": args.ordering,
                       "parallelism": (f"tree-partition{world} (proportional mapping, RCCL p2p)"
                                       if partitioned else f"replicas{world}" if world > 1 else "single")},
            "roofline": {"bound": "mfma", "kernel": "Schur-complement GEMM group: k_gemm128_mfma3 (fp64 MFMA 128x128 tile) + k_gemm_k64 (k <= 64, one-shot MFMA 64x64) + k_gemm64_mfma (MFMA 64x64, small launches)",
                         "achieved": achieved, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": (achieved / FP64_PEAK_TFLOPS) if achieved else None,
                         "traffic": traffic,
                         "launches_per_step": n_gemm if not partitioned else None,
                         "avg_launch_us": avg_us,
                         "flops_per_launch": gemm_flops / n_gemm if (n_gemm and not partitioned) else None,
                         "algorithmic_bytes_per_launch": fst["gemm_bytes"] / n_gemm if (n_gemm and not partitioned) else None,
                         "traffic_source": traffic_src, "kernels_sha": sha,
                         "note": "fp64 MFMA (v_mfma_f64_16x16x4) 128x128 tiles for large launches, fp64 MFMA "
                                 "64x64 tiles for small ones; peak = MI355X fp64 dense peak; "
                                 "achieved = GEMM flops per refactor / HIP-event time of the GEMM "
                                 "launches per refactor (graph-captured events on the launch "
                                 "stream); traffic = HBM bytes per launch from rocprofv3 PMC "
                                 "(FETCH_SIZE x2 + WRITE_SIZE, " + traffic_src + ")"},
            "kernel_ms_per_step": {k: v / K for k, v in kind_ms.items()},
            "launches_per_refactor": fst["launches"],
            # per-kind HIP-event times exist for the single-GPU path only (partitioned: None)
            "gemm_split": ({"panel_tflops": (gemm_flops - fst["gemm22_flops"]) / ((kind_ms["gemm"] + kind_ms["gemmu"] + kind_ms["gemmo"]) / K) / 1e9,
                            "f22_tflops": fst["gemm22_flops"] / (kind_ms["gemm22"] / K) / 1e9,
                            "panel_gflop": (gemm_flops - fst["gemm22_flops"]) / 1e9,
                            "f22_gflop": fst["gemm22_flops"] / 1e9}
                           if ms_gemm > 0 and kind_ms["gemm22"] > 0 else None),
            "refactor_tflops": dense_flops / (ms_per_step * 1e-3) / 1e12,
            # measured HBM traffic of a whole refactor (PMC FETCH_SIZE x2 + WRITE_SIZE over every
            # kernel, profiles/) over this run's time per refactor
            "achieved_hbm_GBs": (hbm_refactor / (ms_per_step * 1e-3) / 1e9) if hbm_refactor else None,
            "achieved_hbm_frac": (hbm_refactor / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS) if hbm_refactor else None,
            "create_s": t_create,
            "ranks": per_rank,
            "full": full,
        }
        if full:   # the side measurements a plain run skips
            res.update({"refactor_host_values_ms": refactor_host_ms, "solve_ms": solve_ms,
                        "solve_8rhs_ms": solve8_ms, "solve_residual": solve_residual})
        if partitioned:
            res["rccl_nranks"] = min(r.get("rccl_nranks", 0) for r in per_rank)
            res["transport"] = (f"{args.one_gpu_transport} (gloo, one-GPU rehearsal)" if args.test_one_gpu
                                else "rccl")
            if args.check_single:
                res["x_vs_single_gpu_max_rel"] = max(r["x_vs_single_gpu_max_rel"] for r in per_rank)
        if cpu_leg:
            log("ordering comparison (host symbolic analysis) ...")
            res["config"]["ordering_compare"] = ordering_compare(N)
            log("cpu baseline ...")
            res["cpu_baseline"] = cpu_baseline(N, dense_flops, nnzLU, args.ordering == "geometric")
        if configs_leg:
            log("configs C1 / C2 / C5 steady state ...")
            res["configs"] = gpu_configs(dev)
        print(json.dumps(res), flush=True)
    F.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
