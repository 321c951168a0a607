"""Iterations and seconds of the P2 weak-Dirichlet step (P2Problem, deterministic) with and without the coarse-space
correction (PhiFEMSolver(coarse_space=...)).  Every (n, coarse_space) run is a child process under its own `timeout`;
one JSON line per run.

    python tools/p2_coarse_timing.py --sizes 64,128,256 --spaces none,5,8,auto --repeat 1 [--timeout 600]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys, time, warnings
import torch
sys.path.insert(0, {root!r})
from phifem_amd.distributed import P2Problem
n, cs = {n}, {cs!r}
prob = P2Problem(n, rtol=1e-8, coarse_space=cs)
prob.setup()
torch.cuda.reset_peak_memory_stats()
t0 = time.perf_counter()
with warnings.catch_warnings(record=True) as wl:
    warnings.simplefilter("always")
    res = prob.step()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
st = prob.solver.stats
free, total = torch.cuda.mem_get_info()
print(json.dumps({{"n": n, "coarse_space": cs, "iterations": res["iterations"], "relres": res["relres"],
                  "converged": res["converged"], "step_s": dt, "solve_s": res["stage_s"]["solve"],
                  "precond": st["precond"], "coarse_ratio": st.get("coarse_ratio", 0),
                  "coarse_dofs": st.get("coarse_dofs", 0), "coarse_build_s": st.get("coarse_build_s", 0.0),
                  "coarse_reason": st.get("coarse_reason"), "device_used_gb": (total - free) / 1e9,
                  "warnings": [str(w.message)[:160] for w in wl]}}))
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--spaces", default="none,5,8,auto")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    for n in (int(v) for v in a.sizes.split(",")):
        for sp in a.spaces.split(","):
            cs = None if sp == "none" else ("auto" if sp == "auto" else int(sp))
            for _ in range(a.repeat):
                code = CHILD.format(root=ROOT, n=n, cs=cs)
                p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, "-c", code],
                                   capture_output=True, text=True)
                line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
                if p.returncode != 0:
                    print(json.dumps({"n": n, "coarse_space": cs, "exit": p.returncode, "stderr": p.stderr[-400:]}), flush=True)
                    return p.returncode   # a failed or timed-out GPU step ends the sweep
                print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
