"""General mesh partition on the GPU: the device partitioner and layout kernels against the numpy specification
(tests/partition_ref.py), and `PartitionedProblem` with several ranks sharing the one GPU of the test box -- native
loop through the host-staged RCCL stand-in, Python loop over gloo -- against the single-mesh HIP solve."""
import os
import warnings

import numpy as np
import pytest

import partition_ref as PR
from partition_ref import case, free_port

pytestmark = pytest.mark.gpu

_FAKE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_rccl", "libfake_rccl.so")


def _tagged(name):
    import phifem_amd as P
    from phifem_amd.mesh_scripts import NodalFunction
    ctype, x, cells, phi, f, uD = case(name)
    mesh = P.Mesh.from_arrays(ctype, x, cells)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
    return mesh, (ctype, x, cells, phi, f, uD)


@pytest.mark.parametrize("name", ["disk", "square_tri", "tetbox"])
@pytest.mark.parametrize("nparts", [2, 3, 5, 8])
def test_partition_cells_equals_reference(name, nparts):
    import torch
    import phifem_amd as P
    mesh, (ctype, x, cells, phi, f, uD) = _tagged(name)
    assert np.array_equal(P.partition_cells(mesh, nparts), PR.partition_cells_ref(x, cells, nparts))
    w = PR.weights_from_tags(mesh.cell_tag_values())
    ref = PR.partition_cells_ref(x, cells, nparts, w)
    assert np.array_equal(P.partition_cells(mesh, nparts, w), ref)
    wd = torch.from_numpy(w).cuda()
    assert np.array_equal(P.partition_cells(mesh, nparts, wd).cpu().numpy(), ref)      # device in, device out
    with pytest.raises(ValueError):
        P.partition_cells(mesh, nparts, -w - 1)


def test_partition_cells_shuffled_kuhn_box():
    """A 24^3 Kuhn box in shuffled vertex and cell order (many equal centroid coordinates: the tie-break by cell index
    decides), weights from the tags of a sphere."""
    import phifem_amd as P
    from phifem_amd.mesh_scripts import NodalFunction
    x, cells = PR.graded_tet_box(n=(24, 24, 24), seed=2, grade=1.0)
    mesh = P.Mesh.from_arrays("tetrahedron", x, cells)
    phi = (x ** 2).sum(axis=1) - 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.compute_tags_measures(mesh, NodalFunction(phi), 1, box_mode=True, single_layer_cut=True)
    w = PR.weights_from_tags(mesh.cell_tag_values())
    for nparts in (2, 5, 8):
        assert np.array_equal(P.partition_cells(mesh, nparts, w), PR.partition_cells_ref(x, cells, nparts, w))
        assert np.array_equal(P.partition_cells(mesh, nparts), PR.partition_cells_ref(x, cells, nparts))


@pytest.mark.parametrize("name", ["disk", "tetbox"])
@pytest.mark.parametrize("world", [3, 5])
def test_layout_equals_reference(name, world):
    import phifem_amd as P
    from phifem_amd.partition import local_mesh
    mesh, (ctype, x, cells, phi, f, uD) = _tagged(name)
    cv, fv = mesh.cell_tag_values(), mesh.facet_tag_values()
    from oracle.topology import Topology
    topo = Topology(ctype, cells, x.shape[0])
    assert np.array_equal(topo.c2f, mesh.c2f)       # the library numbers the facets as the oracle does
    part = P.partition_cells(mesh, world, PR.weights_from_tags(cv))
    for rank in range(world):
        ref = PR.layout_ref(ctype, x, cells, cv, fv, world, rank, topo=topo)
        assert np.array_equal(part, ref["part"])
        owner, flags = P.partition_layout(mesh, world, part, rank)
        assert np.array_equal(owner, ref["owner"]) and np.array_equal(flags, ref["flags"])
        sub, c_map, v_map = local_mesh(mesh, flags)
        assert np.array_equal(c_map, ref["c_map"]) and np.array_equal(v_map, ref["v_map"])
        assert np.array_equal(sub.cells, ref["cells"]) and np.array_equal(sub.x, ref["x"])
        assert np.array_equal(sub.c2f, ref["topo"].c2f)
        assert np.array_equal(sub.cell_tag_values(), ref["cell_tags"])
        assert np.array_equal(sub.facet_tag_values(), ref["facet_tags"])


def _worker(rank, world, name, port, outdir, native, deterministic, balance, tag):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["PHIFEM_NATIVE_LOOP"] = "1" if native else "0"
    os.environ["PHX_RCCL_LIB"] = _FAKE
    os.environ["PHX_DIST_TIMEOUT_S"] = "120"        # trouble ends the worker
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from phifem_amd.distributed import PartitionedProblem
        ctype, x, cells, phi, f, uD = case(name)
        prob = PartitionedProblem(ctype, x, cells, phi, f, uD, rank=rank, world=world, device=0, rtol=1e-11,
                                  deterministic=deterministic, balance=balance)
        prob.setup()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = prob.step()
        v, u, p = prob.solution()
        np.savez(os.path.join(outdir, f"{tag}{rank}.npz"), v=v, u=u, p=p, it=res["iterations"], relres=res["relres"],
                 n_owned=res["n_active_owned"], n_peers=res["n_peers"], halo=res["halo_entries"], path=prob.dk.path,
                 converged=res["converged"], precond=res["precond"])
    finally:
        dist.destroy_process_group()


def _single_mesh(name):
    import phifem_amd as P
    from phifem_amd import _lib as L
    mesh, (ctype, x, cells, phi, f, uD) = _tagged(name)
    L.check(L.lib.phx_set_option(mesh._h, L.OPT_PRECOND, 0))      # Jacobi, as the partitioned solve
    s = P.PhiFEMSolver(mesh)
    info = s.assemble(phi, f, uD)
    w = s.solve(rtol=1e-11)
    return mesh, info, w, s.stats


def _run(name, world, native, tmp_path, deterministic=False, balance="domain", tag="r"):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, name, free_port(), str(tmp_path), native, deterministic, balance, tag),
             nprocs=world, join=True)
    return [np.load(os.path.join(str(tmp_path), f"{tag}{r}.npz")) for r in range(world)]


def _compare(rows, mesh, info, wref, native):
    nv = mesh.nv
    u = np.full(nv, np.nan)
    p = np.full(nv, np.nan)
    for d in rows:
        assert np.all(np.isnan(u[d["v"]])), "a vertex is owned by two ranks"
        u[d["v"]], p[d["v"]] = d["u"], d["p"]
        assert d["relres"] <= 1e-11 and bool(d["converged"])
        assert str(d["path"]) == ("native" if native else "python"), "the wrong loop ran"
        assert str(d["precond"]) == "jacobi"
    active_u = wref[:nv] != 0.0
    assert not np.any(np.isnan(u) & active_u), "an active vertex is owned by no rank"
    assert sum(int(d["n_owned"]) for d in rows) == info["n_active"]
    assert len({int(d["it"]) for d in rows}) == 1, "ranks stopped at different iterations"
    u, p = np.nan_to_num(u), np.nan_to_num(p)
    scale = np.abs(wref).max()
    assert np.abs(u - wref[:nv]).max() <= 1e-7 * scale
    assert np.abs(p - wref[nv:]).max() <= 1e-7 * scale


@pytest.mark.skipif(not os.path.exists(_FAKE), reason="tests/fake_rccl/libfake_rccl.so not built (build())")
@pytest.mark.parametrize("name,world,native", [("disk", 2, True), ("disk", 3, False), ("square_tri", 5, True),
                                               ("square_tri", 4, False), ("tetbox", 3, True), ("tetbox", 4, True),
                                               ("tetbox", 5, False)])
def test_partitioned_solve_matches_single_mesh(name, world, native, tmp_path):
    rows = _run(name, world, native, tmp_path)
    mesh, info, wref, st = _single_mesh(name)
    _compare(rows, mesh, info, wref, native)
    its = int(rows[0]["it"])
    print(f"{name} world {world} native {native}: {its} iterations, single mesh {st['iterations']}, "
          f"peers {[int(d['n_peers']) for d in rows]}, halo entries {[int(d['halo']) for d in rows]}")
    # the margin tests/test_hip_multirank.py allows between slab and single-mesh counts of ONE operator
    assert abs(its - st["iterations"]) <= max(5, st["iterations"] // 5), (its, st["iterations"])
    if (name, world) == ("square_tri", 5):
        # chosen on the CPU reference (tests/test_partition_cpu.py): some rank talks to more peers than a slab ever has
        assert max(int(d["n_peers"]) for d in rows) >= 3


@pytest.mark.skipif(not os.path.exists(_FAKE), reason="tests/fake_rccl/libfake_rccl.so not built (build())")
def test_deterministic_iteration_count_repeats(tmp_path):
    """With deterministic=True the iteration count of a given (mesh, world) repeats exactly, and so does the solution,
    bit for bit: partition, layout and halo lists are the same bits by construction, the P1 assembly of the local
    meshes accumulates exactly, the records of the rows that read halo entries are in row order and the dot products are
    folded in a fixed order (PHX_OPT_DETERMINISTIC).  Three ranks with two peers each: the overlapped exchange runs."""
    a = _run("tetbox", 3, True, tmp_path, deterministic=True, tag="a")
    b = _run("tetbox", 3, True, tmp_path, deterministic=True, tag="b")
    assert int(a[0]["it"]) == int(b[0]["it"]), (int(a[0]["it"]), int(b[0]["it"]))
    for da, db in zip(a, b):
        assert np.array_equal(da["v"], db["v"]) and np.array_equal(da["u"], db["u"]) and np.array_equal(da["p"], db["p"])


@pytest.mark.parametrize("local", [True, False])
def test_deterministic_p1_assembly_on_unstructured_mesh(local):
    """PHX_OPT_DETERMINISTIC covers the P1 assembly of meshes that are no Kuhn boxes: two assemblies on freshly built
    meshes (the vertex-to-cell adjacency is filled in a different order each time) give the same matrix, right-hand
    side and solver ordering bit for bit, and the single-rank solve the same iterations and solution.  local = True: the
    local mesh of rank 0 of 3; False: the whole graded tet box."""
    import ctypes as C
    import torch
    import phifem_amd as P
    from phifem_amd import _lib as L
    from phifem_amd.partition import local_mesh

    def build():
        mesh, (ctype, x, cells, phi, f, uD) = _tagged("tetbox")
        keep = mesh
        if local:
            part = P.partition_cells(mesh, 3, PR.weights_from_tags(mesh.cell_tag_values()))
            _, flags = P.partition_layout(mesh, 3, part, 0)
            mesh, _, v_map = local_mesh(mesh, flags)
            phi, f, uD = phi[v_map], f[v_map], uD[v_map]
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, 1))
        s = P.PhiFEMSolver(mesh, deterministic=True)
        info = s.assemble(phi, f, uD)
        rowptr, col, val, rhs, dof = s.export_csr()
        perm = torch.empty(info["n_active"], dtype=torch.int32, device="cuda")
        L.check(L.lib.phx_system_get_perm(s._sys, C.c_void_p(perm.data_ptr()), None, None, L.DEVICE))
        out = [rowptr, col, val, rhs, dof, perm.cpu().numpy()]
        if not local:       # (the rows of ghost vertices of a local mesh are incomplete: nothing to solve there)
            out += [s.solve(rtol=1e-11), np.array(s.stats["iterations"])]
        del keep
        return out

    a, b = build(), build()
    assert all(np.array_equal(p, q) for p, q in zip(a, b)), [bool(np.array_equal(p, q)) for p, q in zip(a, b)]
    # and against plain atomics: the same numbers to round-off
    mesh, (ctype, x, cells, phi, f, uD) = _tagged("tetbox")
    if not local:
        L.check(L.lib.phx_set_option(mesh._h, L.OPT_EXPORT_CSR, 1))
        s = P.PhiFEMSolver(mesh)
        s.assemble(phi, f, uD)
        rowptr, col, val, rhs, dof = s.export_csr()
        assert np.array_equal(rowptr, a[0]) and np.array_equal(col, a[1])
        assert np.abs(val - a[2]).max() <= 1e-13 * np.abs(val).max()
        assert np.abs(rhs - a[3]).max() <= 1e-13 * np.abs(rhs).max()


@pytest.mark.skipif(not os.path.exists(_FAKE), reason="tests/fake_rccl/libfake_rccl.so not built (build())")
@pytest.mark.parametrize("native", [True, False])
def test_rank_that_owns_nothing(native, tmp_path):
    """World 4, the domain in one corner of the box, the parts balanced over the background cells: ranks away from the
    corner own no row, hold an empty system and still join every collective."""
    rows = _run("corner", 4, native, tmp_path, balance="cells")
    mesh, info, wref, st = _single_mesh("corner")
    owned = [int(d["n_owned"]) for d in rows]
    assert 0 in owned and max(owned) > 0, owned
    _compare(rows, mesh, info, wref, native)
