"""Weak-Dirichlet phi-FEM Poisson on an UNSTRUCTURED background mesh partitioned over several ranks
(`phifem_amd.distributed.PartitionedProblem`; the flower demo next door is the single-rank flow).

    python demo/weak-dirichlet/partitioned.py --ranks 4 [--n 48] [--backend gloo|nccl]

The script starts its own ranks as fresh child processes (one per GPU with nccl; with gloo they share GPU 0 -- a
rehearsal).  The background mesh is a graded, shuffled triangulation of [-1.5, 1.5]^2 around the unit disk; every rank is
handed the whole mesh, so it has to fit one GPU.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def background_mesh(n, seed=0):
    """Graded (planes at a power law of the lattice index) right-diagonal triangulation, vertices and cells shuffled."""
    t = np.linspace(-1.0, 1.0, n + 1)
    ax = 1.5 * np.sign(t) * np.abs(t) ** 1.3
    X, Y = np.meshgrid(ax, ax, indexing="xy")
    x = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    v = (i + (n + 1) * j).reshape(-1)
    cells = np.concatenate([np.stack([v, v + 1, v + n + 2], axis=1), np.stack([v, v + n + 1, v + n + 2], axis=1)])
    rng = np.random.default_rng(seed)
    pv = rng.permutation(x.shape[0])
    inv = np.empty_like(pv)
    inv[pv] = np.arange(pv.size)
    return np.ascontiguousarray(x[pv]), np.ascontiguousarray(inv[cells[rng.permutation(cells.shape[0])]])


def rank_main(args):
    import warnings
    import torch.distributed as dist
    from phifem_amd.distributed import PartitionedProblem
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group(args.backend, rank=rank, world_size=world)
    try:
        x, cells = background_mesh(args.n)
        phi = (x ** 2).sum(axis=1) - 1.0
        u_ex = np.sin(x[:, 0]) * np.sin(x[:, 1])            # -Laplace(u) = 2 u
        prob = PartitionedProblem("triangle", x, cells, phi, 2.0 * u_ex, u_ex, rank=rank, world=world,
                                  device=rank if args.backend == "nccl" else 0, rtol=args.rtol)
        prob.setup()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = prob.step()
        v, u, _ = prob.solution()
        err = float(np.abs(u - u_ex[v]).max()) if v.size else 0.0
        print(f"rank {rank}: {res['n_active_owned']} owned rows, {res['n_peers']} peers, {res['halo_entries']} halo "
              f"entries, {res['ghost_cells']} ghost / {res['owned_cells']} owned cells, {res['iterations']} iterations, "
              f"relres {res['relres']:.2e}, max |u - u_ex| on owned vertices {err:.3e}", flush=True)
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--n", type=int, default=48, help="squares per axis of the background mesh")
    ap.add_argument("--rtol", type=float, default=1e-9)
    ap.add_argument("--backend", default="gloo", choices=["gloo", "nccl"])
    args = ap.parse_args()
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:
        return rank_main(args)
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.ranks):                               # fresh child processes, never exec
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(args.ranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("PHX_DIST_TIMEOUT_S", "300")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    codes = [p.wait() for p in procs]
    if any(codes):
        raise SystemExit(f"a rank failed: exit codes {codes}")


if __name__ == "__main__":
    main()
