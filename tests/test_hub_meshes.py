"""CPU checks of tests/hub_meshes.py: the builder, and -- against the oracle alone -- the conditions that put every
case of tests/test_hip_high_valence.py on the branch it is meant for.  A seed or a scipy / qhull version that moves a
case off its branch fails here, before any GPU run."""
import numpy as np
import pytest

import hub_meshes as H


@pytest.mark.parametrize("d,m", [(2, 7), (2, 70), (3, 12), (3, 150)])
def test_ring_points_lie_on_the_sphere_and_are_distinct(d, m):
    c = np.array([0.2, -0.1, 0.3])[:d]
    p = H.ring_points(d, c, m, 0.12)
    assert p.shape == (m, d)
    assert np.abs(np.linalg.norm(p - c, axis=1) - 0.12).max() < 1e-15
    gap = np.linalg.norm(p[:, None] - p[None], axis=2) + np.eye(m)
    # 2-D: the chord of 2 pi / m; 3-D: the Fibonacci lattice keeps points about sqrt(4 pi / m) apart
    assert gap.min() > 0.12 * (0.99 * 2.0 * np.sin(np.pi / m) if d == 2 else 1.0 / np.sqrt(m))


@pytest.mark.parametrize("d", [2, 3])
def test_builder_joins_every_hub_to_its_ring_only(d):
    hubs = [(H.IN2 if d == 2 else H.IN3, 25, 0.1), ((-0.7, 0.6, 0.5)[:d], 18, 0.08)]
    x, cells, hub = H.build_hub_mesh(d, 3, 200, hubs)
    assert cells.dtype == np.int64 and cells.shape[1] == d + 1 and x.shape[1] == d
    assert np.array_equal(np.unique(cells), np.arange(x.shape[0]))
    assert np.array_equal(x[:2 ** d].min(axis=0), [H.LO] * d) and np.array_equal(x[:2 ** d].max(axis=0), [H.HI] * d)
    assert abs(H.cell_volumes(x, cells).sum() - (H.HI - H.LO) ** d) < 1e-12     # the cells tile the box
    nn = H.neighbour_counts(x.shape[0], cells)
    first_ring = hub[-1] + 1
    for k, (h, (c, m, r)) in enumerate(zip(hub, hubs)):
        assert np.array_equal(x[h], np.asarray(c)[:d]) and nn[h] == m
        ring = first_ring + sum(hh[1] for hh in hubs[:k]) + np.arange(m)
        nb = np.setdiff1d(np.unique(cells[(cells == h).any(axis=1)]), [h])
        assert np.array_equal(nb, ring)
        others = np.setdiff1d(np.arange(x.shape[0]), np.concatenate([[h], ring]))
        assert np.linalg.norm(x[others] - x[h], axis=1).min() >= 2.2 * r
    # same seed, same mesh
    x2, cells2, _ = H.build_hub_mesh(d, 3, 200, hubs)
    assert np.array_equal(x, x2) and np.array_equal(cells, cells2)


def test_builder_refuses_a_hub_that_is_not_joined_to_all_its_ring():
    # a second hub inside the ring of the first: neither has exactly its m neighbours
    with pytest.raises(AssertionError, match="neighbours"):
        H.build_hub_mesh(2, 1, 50, [(H.IN2, 20, 0.1), ((H.IN2[0] + 0.03, H.IN2[1]), 20, 0.1)])


def test_predicted_capacity():
    assert [H.predicted_capacity("p1", 3, w) for w in (1, 64, 65, 128, 129, 256, 257)] == [64, 64, 128, 128, 256, 256, None]
    assert [H.predicted_capacity("p1", 2, w) for w in (32, 33, 64, 65, 128, 129)] == [32, 64, 64, 128, 128, None]
    assert H.predicted_capacity("el", 2, 244) == 256 and H.predicted_capacity("flux", 3, 325) == 512


@pytest.mark.parametrize("name", list(H.CASES))
def test_case_sits_on_its_branch(name):
    c = H.CASES[name]
    kind, d = c["kind"], c["d"]
    x, cells, hub = H.case_mesh(name)
    o = H.case_oracle(name)
    widths, nn = o["widths"], o["neighbours"]
    widest = int(widths.max())
    caps = H.CAPACITIES[kind][d]
    print(f"{name}: nv={x.shape[0]} nc={cells.shape[0]} n_active={widths.size} widest row {widest}, "
          f"hub neighbours {[int(nn[h]) for h in hub]}, capacities {caps}")
    assert c["lo"] <= widest and (c["hi"] is None or widest <= c["hi"])
    assert [int(nn[h]) for h in hub] == [m for _, m, _ in c["hubs"]]
    # the interval is the one between two capacities of the library (or at / behind one)
    if c["hi"] is None:
        assert c["lo"] == caps[-1] + 1 and H.predicted_capacity(kind, d, widest) is None
    else:
        assert c["hi"] in caps and H.predicted_capacity(kind, d, widest) == c["hi"]
    if name.endswith("_a_fits"):
        assert c["hi"] == caps[0] and c["lo"] == caps[0] - 4
    if name.endswith("_b_full"):
        assert c["lo"] == c["hi"] == caps[0] and np.count_nonzero(widths == caps[0]) >= 1
    if c["bulk"]:
        bulk = H.bulk_row_widths(x, cells, o["cell_tags"], o["idx"], widths)
        print(f"{name}: widest row away from the cut cells {int(bulk.max())}")
        assert bulk.max() > H.EL_BOX_BULK_SLOTS
    if name.endswith("_d_retry") or (kind != "p1" and not name.startswith("el_2d")):
        assert c["lo"] == caps[0] + 1 and c["hi"] == caps[1]
    if name.endswith("_d_retry_twice"):
        assert c["lo"] == caps[1] + 1 and c["hi"] == caps[2]
    if c["spill"]:
        # an interior hub: its u row is active and holds more keys than the LDS table of the row kernel, its p row is
        # not active; every cell around it lies inside, so the row is the stiffness row: the hub and its neighbours
        nv, h = x.shape[0], int(hub[0])
        rows = {int(i) // nv: int(w) for i, w in zip(o["idx"], widths) if int(i) % nv == h}
        assert set(rows) == {0}, rows
        assert nn[h] >= H.ROW_LDS_SLOTS + 1 and rows[0] == nn[h] + 1 > H.ROW_LDS_SLOTS
        assert np.all(o["cell_tags"][(cells == h).any(axis=1)] == 1)
        if d == 3:
            assert widest <= caps[0]     # the spill alone, without a retry


def test_capacities_match_the_library_source():
    """CAPACITIES is a copy of the lists of the `retry_capacity` calls, read back here from the source: literal lists
    (P1, interface elasticity), and `{W, 2 * W}` with the `const int W = ...` line in front of the call (P2, strong
    Dirichlet at degree 1, flux on simplices)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(__file__), "..", "phifem_amd", "csrc")

    def src(name):
        return open(os.path.join(csrc, name)).read()

    def literal(text):
        return [tuple(int(v) for v in m.split(",")) for m in re.findall(r"retry_capacity\(\{([0-9, ]+)\}", text)]

    def doubled(text):      # -> (3-D, 2-D) first capacity of the `const int W = ... gdim == 3 ? a : b` line
        assert "retry_capacity({W, 2 * W}" in text
        line, = [ln for ln in text.splitlines() if ln.strip().startswith("const int W = ")]
        a, b = re.findall(r"gdim == 3 \? (\d+) : (\d+)", line)[0]
        return int(a), int(b)

    p1 = literal(src("phx_assemble.hip"))
    assert H.CAPACITIES["p1"][3] in p1 and H.CAPACITIES["p1"][2] in p1
    assert literal(src("phx_assemble_el.inc.hip")) == [H.CAPACITIES["el"][2]] == [H.CAPACITIES["el"][3]]
    for kind, name in (("p2", "phx_assemble_p2.inc.hip"), ("sd", "phx_assemble_sd.inc.hip"),
                       ("flux", "phx_assemble_flux.inc.hip")):
        w3, w2 = doubled(src(name))
        assert H.CAPACITIES[kind][3] == (w3, 2 * w3) and H.CAPACITIES[kind][2] == (w2, 2 * w2), kind
