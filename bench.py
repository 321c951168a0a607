#!/usr/bin/env python3
"""Headline benchmark: assembled+solved DoF/s of the 3-D weak-Dirichlet phi-FEM Poisson path.

One "step" = one full pass of the hot path over one synthetic problem already resident in HBM:
  tag cells + facets  ->  assemble (element integration, scatter, CSR, SELL)  ->  Krylov solve.
Workload at N=1: BASELINE.json configs[1] -- spherical level-set, P1 x P1, 256^3 Kuhn box
(100 663 296 tetrahedra, 16 974 593 vertices) on [-1.5,1.5]^3, manufactured f / u_D,
gamma = sigma = 1, detection degree 1, single-layer cut, box mode.
N>1: weak scaling -- every rank owns a 256x256x256 slab of a 256x256x(256 N) box around the capsule
x^2 + y^2 + max(|z| - 1.5 (N - 1), 0)^2 = 1 (the sphere of N = 1 stretched by a cylinder of radius 1: same h,
same work per unit length, full cross-sections at every slab interface), see phifem_amd/distributed.py.

Contract (driver): `python bench.py --gpus N --steps K --warmup W` prints ONE JSON line on rank 0.
With N > 1 the driver starts the ranks itself (`python -m torch.distributed.run --nproc-per-node N ... bench.py
--gpus N`, WORLD_SIZE in the environment).  Started WITHOUT a launcher, `python bench.py --gpus N` starts the N
ranks itself (a child `torch.distributed.run`, before this process has touched a GPU) and relays rank 0's line;
a WORLD_SIZE that contradicts --gpus is an error, never a silent N = 1 run.
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cubes", type=int, default=256, help="cubes per axis per GPU")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--cpu-n", type=int, default=0,
                    help="box size of the CPU-baseline sample (0: the full 256^3 workload when the host "
                         "grants >= 12 cores, else 160^3; ~10-30 s of CPU work either way)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--config4", action="store_true",
                    help="BASELINE configs[3]: 3-D interface elasticity (5-field mixed, 27 components per "
                         "vertex) on a --cubes^3 box (256 in the config) split into z-slabs over the GPUs "
                         "(strong scaling); not the default workload")
    ap.add_argument("--config3", action="store_true",
                    help="BASELINE configs[2]: 3-D Poisson with P2 x P2 elements + stabilisation on a --cubes^3 box, "
                         "one GPU; not the default workload")
    ap.add_argument("--config5", action="store_true",
                    help="BASELINE configs[4]: 1024 x 1024 x 128 cubes per GPU (805 306 368 tets), unit "
                         "sphere, 1024^3 box at 8 GPUs; not the default workload")
    ap.add_argument("--no-configs4-extra", action="store_true",
                    help="default runs also time BASELINE configs[4] (the slab above, 2 steps) after the headline "
                         "workload and report it under the key `configs4_slab` of the same line; this skips it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (solution vector, cell tags) as "
                         "DIR/<name>.npy: a fixed, seeded sample of each array, at most 64 MB in all")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def hbm_in_use_gb():
    """Device memory in use on this rank's GPU when the line is written (whole device: systems, pool, torch)."""
    try:
        import torch
        free, total = torch.cuda.mem_get_info()
        return round((total - free) / 2 ** 30, 2)
    except Exception:
        return None


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a CHILD torch.distributed.run
    (this process has not initialised any GPU -- nothing is re-exec'd), relay its output, return its exit
    code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    import tempfile
    mark = os.path.join(tempfile.gettempdir(), f"phifem_watchdog_{os.getpid()}")
    if os.path.exists(mark):
        os.remove(mark)
    env["PHIFEM_WATCHDOG_FILE"] = mark
    proc = subprocess.run(cmd, env=env)
    if proc.returncode != 0 and os.path.exists(mark) and env.get("PHIFEM_NATIVE_LOOP", "") != "0":
        # a rank left through the watchdog (phifem_amd.dist_solver.Watchdog: a collective of the native RCCL loop
        # never completed; it leaves this file behind).  This process has not touched a GPU: start FRESH ranks
        # once with the Python-driven loop over torch.distributed.
        print("bench.py: a rank left through the RCCL watchdog; retrying once with PHIFEM_NATIVE_LOOP=0",
              file=sys.stderr, flush=True)
        os.remove(mark)
        env["PHIFEM_NATIVE_LOOP"] = "0"
        cmd[cmd.index("--master-port") + 1] = str(free_port())
        proc = subprocess.run(cmd, env=env)
    if os.path.exists(mark):
        os.remove(mark)
    return proc.returncode


def host_cores(cap=16):
    """Threads for the CPU baseline: the CPU share of this process (affinity mask, cgroup quota),
    never more than `cap` -- a GPU box exposes every core of the host (256) but grants one GPU's
    share (16); oversubscribing OpenMP there turns seconds into minutes."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
        except (OSError, ValueError, IndexError):
            pass
    return max(1, min(n, cap))


def cpu_baseline(n, rtol):
    """The C/OpenMP restatement of the same pipeline (oracle/phifem_oracle.c, "port": a CPU
    restatement, NOT dolfinx/PETSc -- those are not installed here or on the GPU box) on a bounded
    sample of the same workload: the same sphere problem on an n^3 box, all host cores.  The system is
    tagged and assembled once and solved twice: with Jacobi-BiCGStab and with the box sine-transform
    preconditioner the GPU path runs ("the same preconditioned Krylov solver run on
    the CPU"); `value` takes the FASTER of the two solves, both are quoted in `sample`.
    Mesh generation is untimed, as on the GPU."""
    from oracle import c_oracle
    cores = host_cores()
    r = c_oracle.poisson_sphere(n, threads=cores, rtol=rtol, precond=1)
    t_j, t_p = r["t_solve"], (r["t_solve_pc"] if r["pc_built"] else float("inf"))
    pre = r["t_tag"] + r["t_assemble"]
    dt = pre + min(t_j, t_p)
    r1 = c_oracle.poisson_sphere(max(n // 2, 8), threads=1, rtol=rtol)
    dt1 = r1["t_tag"] + r1["t_assemble"] + r1["t_solve"]
    return {"value": r["n_active"] / dt, "unit": "DoF/s", "cores": int(r["threads"]), "kind": "port",
            "value_same_algorithm": r["n_active"] / (pre + t_p) if r["pc_built"] else None,
            "value_jacobi": r["n_active"] / (pre + t_j),
            "sample": f"C/OpenMP restatement (oracle/phifem_oracle.c), same sphere problem on a {n}^3 "
                      f"box: {int(r['n_active'])} active DoFs, tag {r['t_tag']:.2f} s + assemble "
                      f"{r['t_assemble']:.2f} s + solve to rtol {rtol:g}: Jacobi-BiCGStab {t_j:.2f} s "
                      f"({int(r['iterations'])} it) | box sine-transform preconditioner as on the GPU "
                      f"{t_p:.2f} s ({int(r['iterations_pc'])} it); value = the faster solve; single core, "
                      f"Jacobi, {max(n // 2, 8)}^3: {r1['n_active'] / dt1:.0f} DoF/s"}


# every 8th SpMV launch of the timed region is bracketed by HIP events on the launch stream
SPMV_EVENT_STRIDE = 8

# --dump-outputs: bytes all ranks together may write (values + sample positions), below the 64 MB the option promises
DUMP_BUDGET_BYTES = 48 << 20


def sample_positions(n, k, seed):
    """k increasing positions in [0, n) when n > k, one drawn uniformly from each of k consecutive strata (fixed seed:
    the same positions on every run); all of them otherwise."""
    import numpy as np
    if n <= k:
        return np.arange(n, dtype=np.int64)
    edges = np.arange(k + 1, dtype=np.int64) * n // k
    u = np.random.default_rng(seed).random(k)
    return edges[:-1] + (u * (edges[1:] - edges[:-1])).astype(np.int64)


def dump_outputs(dirname, prob, rank, world):
    """What the last timed step handed its caller: the solution vector in the full numbering (`prob.out`, inactive
    DoFs at zero) and the cell tags it was assembled on, as DIR/<name>.npy with <name>_index.npy (float64) naming the
    sampled positions.  Each rank writes its own slab (<name>_rank<r>) within its share of DUMP_BUDGET_BYTES."""
    import numpy as np
    import torch
    os.makedirs(dirname, exist_ok=True)
    sfx = f"_rank{rank}" if world > 1 else ""
    share = DUMP_BUDGET_BYTES // world // 2                     # half for the solution, half for the tags
    out = prob.out
    idx = sample_positions(out.numel(), share // 16, seed=1)    # f64 value + f64 position
    sol = out[torch.from_numpy(idx).to(out.device)].cpu().numpy()
    tags = prob.mesh.cell_tag_values()
    tidx = sample_positions(tags.shape[0], share // 12, seed=2)  # f32 value + f64 position
    arrays = {"solution": sol.astype(np.float64), "solution_index": idx.astype(np.float64),
              "cell_tags": tags[tidx].astype(np.float32), "cell_tags_index": tidx.astype(np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + sfx + ".npy"), a)


def event_pair_overhead_us(mesh):
    import ctypes as C
    from phifem_amd import _lib as L
    sec = C.c_double(0.0)
    L.check(L.lib.phx_event_pair_overhead(mesh._h, C.byref(sec)))
    return 1e6 * sec.value


def pmc_traffic(kernel, algorithmic_bytes):
    """HBM bytes per launch of `kernel` from a COMMITTED PMC record (profiles/r*/pmc_*.json; rocprofv3 --pmc in
    separate passes, corrected as the MI355X guide prescribes).  A record only speaks for the launch it was
    measured on: it must name the same kernel AND its algorithmic bytes per launch must equal this run's
    (same system size, element degree and lattice) to 0.5 %.  Otherwise the bench line says null."""
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc_*.json"))):
        try:
            with open(f) as fh:
                d = json.load(fh)
        except (OSError, ValueError):
            continue
        if d.get("kernel_key") != kernel or not d.get("algorithmic_bytes_per_launch"):
            continue
        if abs(d["algorithmic_bytes_per_launch"] - algorithmic_bytes) <= 5e-3 * algorithmic_bytes:
            best = (d["traffic_bytes_per_launch"], os.path.relpath(f, ROOT))
    return best if best else (None, None)


def configs4_extra(args, prob, world, rank, local_rank, dev, barrier, dist, torch, D):
    """Two timed steps (one warm-up) of BASELINE configs[4] per rank after the headline problem has been released.
    Never fatal: whatever goes wrong is reported in the record, the headline line is printed regardless."""
    import gc
    rec = None
    try:
        prob.__dict__.clear()          # mesh, system, nodal data of the headline problem: freed before the slab is built
        gc.collect()
        torch.cuda.empty_cache()
        p5 = D.SlabProblem(n_per_rank=128, rank=rank, world=world, device=local_rank, rtol=args.rtol, nxy=1024)
        p5.setup()                     # (several ranks: its own communicator and halo self-test on the first solve)
        steps = 2
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p5.step()
            barrier()
            t0 = time.perf_counter()
            for _ in range(steps):
                r5 = p5.step()
            barrier()
            dt = time.perf_counter() - t0
        n_act, ok = r5["n_active_owned"], bool(r5["converged"])
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
            tot = torch.tensor([float(n_act), 1.0 if ok else 0.0], dtype=torch.float64, device=dev)
            dist.all_reduce(tot)
            n_act, ok = int(tot[0].item()), int(round(tot[1].item())) == world
        rec = {"workload": "BASELINE configs[4]: 3D weak-Dirichlet Poisson phi-FEM, P1xP1, unit sphere, 1024x1024x128 Kuhn "
                           f"slab per GPU (805306368 tets each; {world} of the 8 slabs of the 1024^3 box, z-range "
                           f"+-{1.5 * world / 8:g})",
               "value": n_act * steps / dt, "unit": "DoF/s", "ms_per_step": 1e3 * dt / steps, "steps": steps, "warmup": 1,
               "active_dofs": n_act, "iterations": r5["iterations"], "relres": r5["relres"], "converged": ok,
               "stage_ms": {k: 1e3 * v for k, v in r5["stage_s"].items()},
               "dist_loop": getattr(getattr(p5, "dk", None), "path", "native-single"),
               "hbm_in_use_gb": hbm_in_use_gb()}
    except Exception as e:   # noqa: BLE001 -- the headline measurement must survive
        rec = {"error": f"{type(e).__name__}: {e}"[:300]}
    return rec


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        # no launcher around us: become one (before any GPU / torch.cuda call in this process)
        raise SystemExit(launch_ranks(args, argv))
    world = int(env_world or "1")
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} contradicts WORLD_SIZE={world}; refusing to run a different "
              f"number of ranks than asked for", file=sys.stderr)
        raise SystemExit(2)

    import numpy as np  # noqa: F401
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # PHIFEM_DIST_BACKEND=gloo: rehearsal of the N>1 path with several ranks on ONE GPU (RCCL
    # refuses two ranks per device); the driver's runs use nccl (= RCCL), one rank per GPU.
    backend = os.environ.get("PHIFEM_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if ndev == 0:
        print("bench.py: no GPU visible (the hot path has no CPU fallback)", file=sys.stderr)
        raise SystemExit(2)
    if world > 1 and backend == "nccl" and ndev < world:
        print(f"bench.py: {world} ranks over RCCL need {world} GPUs, {ndev} visible (one rank per GPU; "
              f"PHIFEM_DIST_BACKEND=gloo rehearses several ranks on one GPU)", file=sys.stderr)
        raise SystemExit(2)
    local_rank = local_rank % ndev
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import phifem_amd as P  # noqa: F401
    from phifem_amd import distributed as D

    n = 128 if args.config5 else args.cubes
    default_workload = not (args.config3 or args.config4 or args.config5) and args.cubes == 256
    if args.config3:
        if world != 1:
            raise SystemExit("--config3 runs on one GPU")
        prob = D.P2Problem(n, device=local_rank, rtol=args.rtol)
    elif args.config4:
        if n % world:
            raise SystemExit("--config4 needs --cubes divisible by the number of GPUs")
        prob = D.ElasticitySlabProblem(n, n // world, rank=rank, world=world, device=local_rank,
                                       rtol=args.rtol)
    else:
        prob = D.SlabProblem(n_per_rank=n, rank=rank, world=world, device=local_rank, rtol=args.rtol,
                             nxy=1024 if args.config5 else None)
    prob.setup()  # mesh generation + nodal data on the device: inputs resident before timing

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(args.warmup):
            prob.step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = prob.step(profile_spmv=SPMV_EVENT_STRIDE)
        barrier()
        dt = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, prob, rank, world)
    ranks_seen, converged = 1, bool(res["converged"])
    if world > 1:
        # max time over ranks, DoFs summed, every rank counted, convergence agreed (MIN)
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        tot = torch.tensor([res["n_active_owned"], 1.0], dtype=torch.float64, device=dev)
        dist.all_reduce(tot)
        n_active, ranks_seen = int(tot[0].item()), int(round(tot[1].item()))
        ok = torch.tensor([1 if converged else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        converged = bool(ok.item())
        # the roofline figures come from the busiest rank (rank 0 may own an empty slab)
        allres = [None] * world
        dist.all_gather_object(allres, res)
        res = max(allres, key=lambda r: r["n_active_owned"])
    else:
        n_active = res["n_active_owned"]

    rc = 0
    if rank == 0:
        value = n_active * args.steps / dt
        spmv_s = res["spmv_avg_s"]
        achieved = res["spmv_algorithmic_bytes"] / spmv_s / 1e9 if spmv_s > 0 else 0.0
        # bytes the FORMAT has to move per launch: the stored matrix stream (columns, values, slice / run records)
        # + x read once + y written once.  For a structured system most rows are applied from a 4-double stencil,
        # so this is far below the CSR figure of SURVEY 8(d) and it is the one a bus fraction must be taken of.
        required = res["spmv_stream_bytes"] + 16.0 * res["spmv_rows"]
        ach_req = required / spmv_s / 1e9 if spmv_s > 0 else 0.0
        tr, src = pmc_traffic("k_spmv_sell+k_spmv_p2s" if args.config3 else "k_spmv_sell", res["spmv_algorithmic_bytes"])
        # (a small --cubes run whose streams sit in L2 / the Infinity Cache may exceed the HBM peak: flagged, not fatal -- ADVICE r3)
        cache_resident = ach_req > HBM_PEAK_GBS
        spmv_roof = {
            "bound": "hbm",
            "kernel": ("k_spmv_sell + k_spmv_p2s (f64 SpMV of the structured P2 system: SELL-16 slices with f64 values / i32 "
                       "columns for the stored band rows, the interior rows from eight class stencils over runs of fine-lattice "
                       "points)" if args.config3 else
                       "k_spmv_sell (f64 SpMV of the assembled system in one launch: SELL slices with f64 values / i32 columns, "
                       "value-indexed where values repeat)" if args.config4 else
                       "k_spmv_sell (f64 SpMV of the assembled system in one launch: 7-point stencil blocks over the "
                       "translation-invariant interior rows of a structured P1 box system, SELL slices with f64 values / "
                       "i32 columns for the stored rows)"),
            # `achieved` / `frac`: SURVEY 8(d)'s algorithmic bytes of the CSR product, 12 nnz + 20 n -- a THROUGHPUT
            # figure (CSR-equivalent GB/s); `achieved_required` / `frac_required`: bytes this format must move
            "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "achieved_required": ach_req, "frac_required": ach_req / HBM_PEAK_GBS, "cache_resident": cache_resident,
            "required_bytes_per_launch": required,
            "traffic": tr, "traffic_source": src, "traffic_over_required": (tr / required) if tr else None,
            "bytes_per_launch": res["spmv_algorithmic_bytes"],
            "avg_launch_us": 1e6 * spmv_s, "launches_timed": res["spmv_count"],
            "launches_per_iteration": 2,
        }
        dst_s = res.get("dst_avg_s", 0.0)
        dst_roof = None
        if dst_s > 0:
            a2 = res["dst_algorithmic_bytes"] / dst_s / 1e9
            # f64 lattices of a wave-mode length run the shape-specialised kernel (phx_dst_wave.inc.hip)
            wave = res["precond_value_bytes"] == 8 and res["precond_L"][1] in (192, 256, 512)
            long_ = res["precond_value_bytes"] == 8 and res["precond_L"][1] in (384, 768, 1024)   # phx_dst_pair.inc.hip
            kname = (f"k_dst_yw<{res['precond_L'][1]}>" if wave else f"k_dst_yp<{res['precond_L'][1]}>" if long_ else
                     f"k_dst_s<{'float' if res['precond_value_bytes'] == 4 else 'double'},1,false>")
            tr2, src2 = pmc_traffic("k_dst_yw" if wave else "k_dst_yp" if long_ else "k_dst_s_y", res["dst_algorithmic_bytes"])
            dst_roof = {
                "bound": "hbm",
                "kernel": f"{kname} (type-I sine "
                          f"transform along y of the preconditioner lattice, "
                          f"f{8 * res['precond_value_bytes']}, one read + one write of every lattice point)",
                "achieved": a2, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": a2 / HBM_PEAK_GBS,
                "traffic": tr2, "traffic_source": src2, "bytes_per_launch": res["dst_algorithmic_bytes"],
                "avg_launch_us": 1e6 * dst_s, "launches_timed": res["dst_count"],
                "launches_per_iteration": 4, "lattice": res["precond_L"],
            }
        # the dominant kernel is the one with the larger share of an iteration
        dominant, other = spmv_roof, dst_roof
        if dst_roof and 4 * dst_s > 2 * spmv_s:
            dominant, other = dst_roof, spmv_roof
        if args.config3:
            workload = (f"3D weak-Dirichlet Poisson phi-FEM, P2xP2 with div(grad) + ghost-penalty stabilisation, "
                        f"P2 spherical level-set, {n}^3 Kuhn box ({6 * n ** 3} tets), box mode, single-layer cut")
        elif args.config4:
            workload = (f"3D interface elasticity phi-FEM, 5-field mixed P1 (27 comps/vertex), E_in=1, E_out=1e-3, "
                        f"nu=0.3, {n}^3 Kuhn box in {world} z-slab(s), box mode")
        elif args.config5:
            workload = ("3D weak-Dirichlet Poisson phi-FEM, P1xP1, unit sphere, 1024x1024x128 Kuhn slab per GPU "
                        "(805306368 tets), box mode, single-layer cut, gamma=sigma=1")
        else:
            shape = "spherical level-set" if world == 1 else (
                f"capsule level-set (radius 1, cylinder length {3 * (world - 1)}: the sphere stretched along z over "
                f"the {world} slabs)")
            workload = (f"3D weak-Dirichlet Poisson phi-FEM, P1xP1, {shape}, {n}^3 Kuhn box per GPU "
                        f"({6 * n ** 3} tets), box mode, single-layer cut, gamma=sigma=1")
        out = {
            "metric": ("assembled+solved DoF/s, 3D interface elasticity phi-FEM (tag+assemble+solve)" if args.config4
                       else "assembled+solved DoF/s, 3D Poisson phi-FEM (tag+assemble+solve)"),
            "value": value, "unit": "DoF/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "strong" if args.config4 else "weak",
            "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": workload,
                "active_dofs": n_active,
                "krylov": ("BiCGStab (f64), right-preconditioned: lattice Laplacian of a box around the active "
                           f"vertices inverted by f{8 * res.get('precond_value_bytes', 8)} sine transforms (u), "
                           "Jacobi (p)") if res.get("precond") == "box-dst"
                else ("BiCGStab (f64), right-preconditioned: the dense 27 x 27 block of the DoFs of each vertex, "
                      "inverted once per system (vertex-block Jacobi)")
                + ("" if res.get("precond") == "vertex-block-jacobi" else
                   f" + Galerkin coarse correction on trilinear functions of spacing {res['precond_L'][0]} h per "
                   f"displacement block ({res.get('precond_points')} coarse DoFs, dense inverse)")
                if str(res.get("precond", "")).startswith("vertex-block-jacobi") else "BiCGStab + Jacobi (right)",
                "rtol": args.rtol, "iterations": res["iterations"], "relres": res["relres"],
                "converged": converged,
                "stage_ms": {k: 1e3 * v for k, v in res["stage_s"].items()},
                "parallelism": f"slab{world}", "ranks_seen": ranks_seen,
                "dist_backend": backend if world > 1 else None,
                "dist_loop": getattr(getattr(prob, "dk", None), "path", "native-single"),
                # what actually ran (a retry with PHIFEM_NATIVE_LOOP=0 keeps the vertex blocks WITHOUT the coarse correction)
                "precond_in_force": res.get("precond"), "precond_slab_exact": bool(res.get("precond_exact", False)),
                "collective_library": getattr(getattr(prob, "dk", None), "library", None),
                "halo_overlap": bool(getattr(getattr(prob, "dk", None), "overlap", False)),
                "system": res.get("system"),
                "deterministic": bool(getattr(prob.solver, "deterministic", False)),
                "hbm_in_use_gb": hbm_in_use_gb(),
            },
            "roofline": dominant,
        }
        dominant["event_pair_overhead_us"] = event_pair_overhead_us(prob.mesh)
        if other:
            out["roofline_other"] = other
        if world > 1:
            print(f"bench.py: {ranks_seen} of {world} ranks took part; loop {out['config']['dist_loop']}; collective library "
                  f"{out['config']['collective_library'] or backend + ' (torch.distributed)'}; preconditioner "
                  f"{out['config']['precond_in_force']}" + (" (slab-exact)" if out['config']['precond_slab_exact'] else ""),
                  file=sys.stderr, flush=True)
        if not converged or ranks_seen != world:
            # an unconverged iterate is not a solution (the reference solves directly): the figure is invalid
            out["valid"] = False
            out["invalid_reason"] = ("BiCGStab stopped at max_iter above rtol" if not converged
                                     else f"{ranks_seen} of {world} ranks took part")
            rc = 3
        if not args.no_cpu_baseline and world == 1:
            cpu_n = args.cpu_n or (256 if host_cores() >= 12 else 160)
            out["cpu_baseline"] = cpu_baseline(cpu_n, args.rtol)
    # ---- BASELINE configs[4] next to the headline: the workload `north_star` states its target on --
    # 1024 x 1024 x 128 cubes per GPU around the unit sphere, the 1024^3 box at 8 GPUs -- timed with the same barriers on
    # every rank and reported under its own key; `value` above stays configs[1] (one GPU) / its capsule weak scaling
    # (several), so that the driver's scaling curve compares like with like.
    extra = None
    if default_workload and not args.no_configs4_extra:
        # The headline must not depend on the extra measurement: if it does not return within its deadline (a collective of
        # the second problem that never completes), rank 0 prints the line it has -- with the reason under `configs4_slab` --
        # and every rank leaves; nothing is re-exec'd.
        import threading
        deadline = float(os.environ.get("BENCH_CONFIGS4_DEADLINE_S", "300"))
        done = threading.Event()

        def give_up():
            if done.wait(deadline):
                return
            if rank == 0:
                out["configs4_slab"] = {"error": f"not finished within {deadline:g} s (BENCH_CONFIGS4_DEADLINE_S); headline unaffected"}
                print(json.dumps(out), flush=True)
            os._exit(rc)
        threading.Thread(target=give_up, daemon=True).start()
        extra = configs4_extra(args, prob, world, rank, local_rank, dev, barrier, dist, torch, D)
        done.set()
    if rank == 0:
        if extra is not None:
            out["configs4_slab"] = extra
        print(json.dumps(out), flush=True)
    if world > 1:
        code = torch.tensor([rc], dtype=torch.int32, device=dev)
        dist.broadcast(code, src=0)
        rc = int(code.item())
        dist.destroy_process_group()
    if rc:
        raise SystemExit(rc)


if __name__ == "__main__":
    main()
