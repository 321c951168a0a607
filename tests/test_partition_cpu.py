"""General mesh partition on the CPU: the numpy specification of tests/partition_ref.py (what the device partitioner
and layout kernels have to equal, tests/test_hip_partition.py), the invariants of the layout it defines, and the
multi-rank host logic (`partition_ownership_and_halos`, `DistributedSolver` with any number of peers) over gloo with the
numpy stand-in of the phase kernels.  No GPU is touched."""
import math
import os
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import partition_ref as PR
from partition_ref import case, free_port
from cpu_backend import CpuBackend
from oracle import assembly as OA, tagging as OT
from oracle.topology import Topology


def oracle_tags(topo, x, phi):
    ls = OT.NodalP1(phi)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cv = OT.tag_cells_values(topo, x, ls, 1, single_layer_cut=True)
        bc = OT.boundary_cell_cut_flags(topo, x, ls, 1)
    fv, _ = OT.tag_facets_values(topo, cv, bc)
    return cv, fv


def oracle_system(topo, x, cv, fv, phi, f, uD):
    ds = OT.integration_entities(topo, np.flatnonzero((cv == 1) | (cv == 2)), np.flatnonzero(fv == 4))
    return OA.assemble_poisson_wd(topo, x, cv, fv, ds, phi, f, uD)


MESHES = ["disk", "square_tri", "tetbox"]
NPARTS = [2, 3, 5, 8]


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("nparts", NPARTS)
def test_reference_partition(name, nparts):
    ctype, x, cells, phi, f, uD = case(name)
    nc = cells.shape[0]
    part = PR.partition_cells_ref(x, cells, nparts)
    assert part.shape == (nc,) and part.min() >= 0 and part.max() < nparts      # every cell in exactly one part
    assert np.array_equal(part, PR.partition_cells_ref(x.copy(), cells.copy(), nparts))   # deterministic
    w = np.bincount(part, minlength=nparts)
    assert w.min() > 0
    # one rounding per bisection level: every part within ceil(log2 nparts) of W / nparts
    assert np.abs(w - nc / nparts).max() <= math.ceil(math.log2(nparts)), (w, nc / nparts)
    # weighted: the exterior carries no weight, the parts share Omega_h
    topo = Topology(ctype, cells, x.shape[0])
    cv, _ = oracle_tags(topo, x, phi)
    wt = PR.weights_from_tags(cv)
    pw = PR.partition_cells_ref(x, cells, nparts, wt)
    ww = np.bincount(pw, weights=wt, minlength=nparts)
    assert ww.sum() == wt.sum() and ww.min() > 0
    assert np.abs(ww - wt.sum() / nparts).max() <= math.ceil(math.log2(nparts)), (ww, wt.sum() / nparts)
    # the order of the cells is part of the rule only through the tie-break: a mesh without equal centroid
    # coordinates is partitioned the same way in any cell order
    if name == "disk":
        perm = np.random.default_rng(1).permutation(nc)
        assert np.array_equal(PR.partition_cells_ref(x, cells[perm], nparts), part[perm])


def test_reference_partition_edge_cases():
    ctype, x, cells, phi, f, uD = case("square_tri")
    assert np.all(PR.partition_cells_ref(x, cells, 1) == 0)
    w = np.zeros(cells.shape[0], dtype=np.int32)
    # without weight the prefix of every split is empty: everything ends in the last part
    assert np.all(PR.partition_cells_ref(x, cells, 4, w) == 3)
    w[7] = 1
    p = PR.partition_cells_ref(x, cells, 2, w)
    assert np.bincount(p, weights=w, minlength=2).tolist() == [1.0, 0.0]
    assert [sorted(lv.items()) for lv in PR.level_ranges(5)] == [[(0, 5)], [(0, 2), (2, 5)], [(0, 1), (1, 2), (2, 3), (3, 5)]]


@pytest.mark.parametrize("name,world", [("disk", 3), ("square_tri", 5), ("tetbox", 3), ("tetbox", 5), ("corner", 4)])
def test_layout_invariants(name, world):
    ctype, x, cells, phi, f, uD = case(name)
    topo = Topology(ctype, cells, x.shape[0])
    cv, fv = oracle_tags(topo, x, phi)
    A, b, act = oracle_system(topo, x, cv, fv, phi, f, uD)
    nv = topo.nv
    active_v = act[:nv]
    balance = "cells" if name == "corner" else "domain"
    lays = [PR.layout_ref(ctype, x, cells, cv, fv, world, r, topo=topo, balance=balance) for r in range(world)]
    owner = lays[0]["owner"]
    # every active vertex is owned by exactly one rank, and nobody owns the others
    assert np.array_equal(owner >= 0, active_v) and owner.max() < world
    assert sum(int(l["owned_v"].sum()) for l in lays) == int(active_v.sum())
    # cells that contribute to a row in the single-mesh assembly: the cells of Omega_h containing the vertex, and
    # through a ghost-penalty facet the cell on its other side
    om = (cv == 1) | (cv == 2)
    gp = np.flatnonzero(((fv == 2) | (fv == 3)) & (topo.f2c[:, 1] >= 0))
    for r, lay in enumerate(lays):
        local = lay["flags"] != 0
        mine = owner == r
        if not mine.any():
            assert local.sum() == 1 and not om[local].any()     # the placeholder: one exterior cell
            continue
        need = np.zeros(topo.nc, dtype=bool)
        need[om & mine[cells].any(axis=1)] = True
        for a, bcell in ((topo.f2c[gp, 0], topo.f2c[gp, 1]), (topo.f2c[gp, 1], topo.f2c[gp, 0])):
            need[bcell[mine[cells[a]].any(axis=1)]] = True
        assert not np.any(need & ~local), "a contributing cell is not local"
        # the owned rows of the local oracle matrix are the same rows of the global one
        lt, lx, v_map = lay["topo"], lay["x"], lay["v_map"]
        Al, bl, actl = oracle_system(lt, lx, lay["cell_tags"], lay["facet_tags"], phi[v_map], f[v_map], uD[v_map])
        nvl = v_map.size
        ov = np.flatnonzero(lay["owned_v"])
        rows_l = np.concatenate([ov, nvl + ov])
        rows_g = np.concatenate([v_map[ov], nv + v_map[ov]])
        assert np.array_equal(actl[rows_l], act[rows_g])
        col_g = np.concatenate([v_map, nv + v_map])
        G = A[rows_g].tocsc()[:, col_g].tocsr()
        assert abs(A[rows_g]).sum() == pytest.approx(abs(G).sum(), rel=1e-14), "an owned row has an entry outside the local mesh"
        D = (Al[rows_l] - G).tocoo()
        scale = abs(A).max()
        assert D.nnz == 0 or np.abs(D.data).max() <= 1e-12 * scale
        assert np.abs(bl[rows_l] - b[rows_g]).max() <= 1e-12 * max(np.abs(b).max(), 1.0)
    if name == "corner":
        assert any(not (owner == r).any() for r in range(world)), "the case was chosen to leave a rank empty"


def _worker(rank, world, name, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from phifem_amd.dist_solver import DistributedSolver, partition_ownership_and_halos
        ctype, x, cells, phi, f, uD = case(name)
        topo = Topology(ctype, cells, x.shape[0])
        cv, fv = oracle_tags(topo, x, phi)
        lay = PR.layout_ref(ctype, x, cells, cv, fv, world, rank, topo=topo,
                            balance="cells" if name == "corner" else "domain")
        v_map = lay["v_map"]
        A, b, act = oracle_system(lay["topo"], lay["x"], lay["cell_tags"], lay["facet_tags"], phi[v_map], f[v_map], uD[v_map])
        nvl = v_map.size
        # rows of vertices this rank does not own may be incomplete: they are never used (ownership mask), but the
        # stand-in scales by the diagonal, which must not vanish
        be = CpuBackend(A, b, act, nvl)
        cache = {}
        layout = partition_ownership_and_halos(torch, dist, be, lay["owned_v"], lay["owner_v"], v_map, x.shape[0],
                                               rank, world, cache=cache)
        # a second call maps the cached lists and exchanges nothing
        again = partition_ownership_and_halos(torch, dist, be, lay["owned_v"], lay["owner_v"], v_map, x.shape[0],
                                              rank, world, cache=cache)
        assert torch.equal(layout[0], again[0]) and len(layout[1]) == len(again[1])
        for h, g in zip(layout[1], again[1]):
            assert h["peer"] == g["peer"] and all(torch.equal(a, c) for k in ("send", "recv") for a, c in zip(h[k], g[k]))
        ds = DistributedSolver(be, dist, torch, rank, world, rtol=1e-11, max_iter=6000, check_every=4, layout=layout)
        out = torch.zeros(2 * nvl, dtype=torch.float64)
        st = ds.solve(out)
        w = out.numpy()
        own = lay["owned_v"]
        np.savez(os.path.join(outdir, f"r{rank}.npz"), gid=v_map[own], u=w[:nvl][own], p=w[nvl:][own],
                 it=st["iterations"], relres=st["relres"], n_owned=st["n_owned"], n_peers=len(ds.halos))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name,world", [("disk", 2), ("disk", 3), ("tetbox", 3), ("square_tri", 5), ("corner", 4)])
def test_partitioned_solver_matches_single_mesh(name, world, tmp_path):
    mp.spawn(_worker, args=(world, name, free_port(), str(tmp_path)), nprocs=world, join=True)
    ctype, x, cells, phi, f, uD = case(name)
    topo = Topology(ctype, cells, x.shape[0])
    cv, fv = oracle_tags(topo, x, phi)
    A, b, act = oracle_system(topo, x, cv, fv, phi, f, uD)
    wref = OA.solve_direct(A, b, act)
    nvg = topo.nv
    u = np.full(nvg, np.nan)
    p = np.full(nvg, np.nan)
    n_owned, peers = 0, []
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), f"r{r}.npz"))
        assert np.all(np.isnan(u[d["gid"]])), "a vertex is owned by two ranks"
        u[d["gid"]] = d["u"]
        p[d["gid"]] = d["p"]
        n_owned += int(d["n_owned"])
        peers.append(int(d["n_peers"]))
        assert d["relres"] <= 1e-11 and d["it"] > 0
    assert np.array_equal(~np.isnan(u), act[:nvg]), "the owned sets do not tile the active vertices"
    assert n_owned == int(act.sum()), "owned active DoFs do not add up to the global system"
    u, p = np.nan_to_num(u), np.nan_to_num(p)
    # the tolerance of tests/test_distributed_cpu.py for this comparison
    scale = np.abs(wref).max()
    assert np.abs(u - wref[:nvg]).max() <= 1e-7 * scale
    assert np.abs(p - wref[nvg:]).max() <= 1e-7 * scale
    if (name, world) == ("square_tri", 5):
        assert max(peers) >= 3, peers       # more than a slab ever has
    if name == "corner":
        assert 0 in [int(np.load(os.path.join(str(tmp_path), f"r{r}.npz"))["n_owned"]) for r in range(world)]
