"""The unstructured test meshes (tests/unstructured_meshes.py) on the CPU: they are valid polyMesh input
(closed cells, positive volumes, upper-triangular order), they have the row widths and graph properties the
GPU tests rely on to reach the library's non-hex branches, and the oracle obeys, on them, properties that do
not rest on its own arithmetic (a uniform state stays put, the pressure matrix is symmetric, rhoEqn
conserves mass). CPU-A steps them against the oracle at test_cpu_a's thresholds."""
import os

import numpy as np
import pytest

import unstructured_meshes as um
from conftest import GOLDEN, ROOT, rel_err

CPU_A = os.path.join(ROOT, "baseline", "cpu_a", "libdfmi_cpu_a.so")
EPS = np.finfo(np.float64).eps
FAMILIES = ("prisms", "hexprism", "refined")
ALL = [(n, s, c) for n in FAMILIES for s in ("small", "large") for c in (False, True)]
IDS = [f"{n}-{s}{'-cyclic-z' if c else ''}" for n, s, c in ALL]


@pytest.mark.parametrize("name,size,cyc", ALL, ids=IDS)
def test_geometry_and_topology(name, size, cyc):
    m = um.get(name, size, cyc)
    _, W, hist, cells = (um.SMALL if size == "small" else um.LARGE)[name]
    assert m.n_cells == cells
    if size == "large":
        assert m.n_cells > 4096 and m.n_cells % 64 != 0
    # closed cells: the outward area vectors of every cell sum to rounding of the largest face
    assert um.closedness(m) <= 3e-16
    assert m.volume.min() > 0
    assert abs(m.volume.sum() - um.L0 ** 3) <= 4 * EPS * um.L0 ** 3
    # upper-triangular order: (owner, neighbour) strictly ascending, owner < neighbour
    assert np.all(m.owner < m.neighbour)
    key = m.owner.astype(np.int64) * m.n_cells + m.neighbour
    assert np.all(np.diff(key) > 0)
    # ... so for any cell the faces where it is the neighbour precede the faces it owns, and both groups
    # ascend in the other cell: ascending face index == ascending column
    F = m.n_faces
    cell = np.concatenate([m.neighbour, m.owner]); other = np.concatenate([m.owner, m.neighbour])
    face = np.concatenate([np.arange(F), np.arange(F)])
    o = np.lexsort((face, cell))
    same = cell[o][1:] == cell[o][:-1]
    assert np.all(other[o][1:][same] > other[o][:-1][same])
    # row widths and the graph
    if hist is not None and not cyc:
        assert np.bincount(um.faces_per_cell(m)).tolist() == hist
    if not cyc:
        assert np.bincount(um.faces_per_cell(m)).size - 1 == W
    assert um.ell_width(m) == W
    from test_gpu_parity import _ell_width
    assert _ell_width(m) == W
    assert len(set(um.faces_per_cell(m).tolist())) > 1      # rows of unequal length: padding in interior rows
    assert not um.is_bipartite(m)
    # the reader's polygon branches ran: triangles (prisms) and the fan on 5-vertex faces (refined)
    sizes = set(m.face_sizes.tolist())
    assert sizes == ({4, 5} if name == "refined" else {3, 4})
    assert [p.name for p in m.patches] == list(um.PATCH_ORDER)
    kinds = {p.name: p.kind for p in m.patches}
    assert kinds["front"] == kinds["back"] == ("cyclic" if cyc else "wall")
    assert all(kinds[k] == "wall" for k in ("left", "right", "top", "down"))


@pytest.mark.parametrize("name", FAMILIES)
def test_cyclic_halves_pair_up(name):
    m = um.get(name, "small", True)
    idx = {p.name: i for i, p in enumerate(m.patches)}
    a, b = m.patches[idx["front"]], m.patches[idx["back"]]
    assert a.neighbour_patch == idx["back"] and b.neighbour_patch == idx["front"]
    assert a.size == b.size > 0
    # equal and opposite to rounding: the reader's triangle fan walks the two halves' vertices in opposite order
    assert np.abs(a.mag_sf - b.mag_sf).max() <= 4 * EPS * a.mag_sf.max()
    assert np.abs(a.sf + b.sf).max() <= 4 * EPS * a.mag_sf.max()
    assert np.abs(a.weight + b.weight - 1.0).max() <= 2 * EPS
    assert np.abs(a.delta_coeffs - b.delta_coeffs).max() <= 4 * EPS * a.delta_coeffs.max()
    # partners face each other across the box: same (x, y), opposite ends in z
    d = m.cell_centres[a.face_cells] - m.cell_centres[b.face_cells]
    assert np.abs(d[:, :2]).max() <= 1e-12 * um.L0 and d[:, 2].min() > 0
    # the patches' faces are not all alike: triangles next to quads, fine next to coarse
    assert np.unique(np.round(a.mag_sf / a.mag_sf.max(), 6)).size > 1


def test_hanging_nodes_leave_the_face_geometry_unchanged():
    """a 5-vertex face is a rectangle with one collinear extra point: its area vector is the rectangle's
    (to rounding) and its centre is the rectangle's -- the fan about the point average must not be biased by the
    extra point"""
    m = um.get("refined", "small")
    five = np.nonzero(m.face_sizes[:m.n_faces] == 5)[0]
    assert five.size > 0
    # such a face lies between two coarse cells, an orthogonal pair of boxes
    o = m.owner[five]
    n = m.sf[five] / m.mag_sf[five, None]
    assert np.abs(np.abs(n).max(axis=1) - 1.0).max() <= 4 * EPS
    d = np.einsum("ij,ij->i", m.mesh_distance[five], n)
    assert np.abs(np.linalg.norm(m.mesh_distance[five], axis=1) - d).max() <= 1e-15 * um.L0
    # the owner is a box: its volume is face area x its extent along the normal, 2 x (Cf - C).n
    half_o = (1.0 - m.weight[five]) * d        # |Cf - Co| along n, from the weight's definition
    assert np.abs(m.mag_sf[five] * 2 * half_o - m.volume[o]).max() <= 1e-13 * m.volume[o].max()


# ------------------------------------------------------------------------------------ oracle properties
def _mech():
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "Burke2012_s9r23.yaml"))
    return ym, read_thermo_table(os.path.join(GOLDEN, "thermo_Burke2012_s9r23.txt"), ym["species"])


def _ctx():
    from dfmi.lib import Context
    if not os.path.exists(CPU_A):
        pytest.fail("CPU-A library not built (make -C baseline/cpu_a)")
    return Context(0, lib_path=CPU_A)


def _state(m, fields, pt, perturb=True):
    """the state after init on CPU-A (thermo from T, phi from rho U), old-time fields perturbed as the parity
    suite does"""
    from dfmi import case
    ym, t = _mech()
    ctx = _ctx()
    inert = ym["species"].index("N2")
    dt = 1e-6
    case.setup_context(ctx, m, t, inert, dt, pt)
    f = fields(m, ym["species"])
    case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"])
    ctx.call("pre_time_step")
    st = case.pull_state(ctx, m, t.S)
    if perturb:
        rng = np.random.default_rng(7)
        st["rho_old"] = st["rho"] * (1 + 1e-3 * rng.standard_normal(m.n_cells))
        st["RR"] = 1e2 * rng.standard_normal((t.S, m.n_cells))
        st["dpdt"] = 1e3 * rng.standard_normal(m.n_cells)
        case.push_state(ctx, st)
    return ctx, t, st, inert, dt


def _tgv(m, species):
    from dfmi import case
    return case.tgv_fields(m, species, kernel_radius=1.2e-3)


def _walls(m):
    from dfmi import case
    pt = case.default_patch_types(m)
    pt.update(um.wall_types(m))
    return pt


@pytest.mark.parametrize("name,cyc", [(n, c) for n in FAMILIES for c in (False, True)],
                         ids=[f"{n}{'-cyclic-z' if c else ''}" for n in FAMILIES for c in (False, True)])
def test_oracle_keeps_a_uniform_state(name, cyc):
    import oracle as O
    from dfmi import case
    m = um.get(name, "small", cyc)
    pt = case.default_patch_types(m)               # zeroGradient walls
    ctx, t, st, inert, dt = _state(m, um.uniform_fields, pt, perturb=False)
    o = O.Oracle(m, t, {k: v.copy() for k, v in st.items()}, pt, inert, 1.0 / dt)
    o.time_step(2)
    ub, sb = um.uniform_state_bounds(m, st, dt)
    for n in ("T", "p", "rho", "he"):
        d = np.abs(o[n] - st[n]).max() / np.abs(st[n]).max()
        print(name, n, d, sb)
        assert d <= sb, (n, d, sb)
    dY = np.abs(o["Y"] - st["Y"]).max()
    print(name, "Y", dY, "U", np.abs(o["U"]).max(), ub)
    assert dY <= sb
    assert np.abs(o["U"]).max() <= ub
    ctx.close()


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_pressure_matrix_is_symmetric(name):
    import oracle as O
    m = um.get(name, "small")
    pt = _walls(m)
    ctx, t, st, inert, dt = _state(m, _tgv, pt)
    o = O.Oracle(m, t, {k: v.copy() for k, v in st.items()}, pt, inert, 1.0 / dt)
    o.u_assemble(); o.u_hbya()
    ref = o.p_assemble()
    assert np.array_equal(ref["lower"], ref["upper"])
    assert np.abs(ref["lower"]).min() > 0
    ctx.close()


@pytest.mark.parametrize("name,cyc", [(n, c) for n in FAMILIES for c in (False, True)],
                         ids=[f"{n}{'-cyclic-z' if c else ''}" for n in FAMILIES for c in (False, True)])
def test_oracle_rho_eqn_conserves_mass(name, cyc):
    """rhoEqn on the closed box (no flux through the walls; what leaves through one cyclic half enters
    through the other): sum(rho V) changes by rounding only -- the bound of test_gpu_fullsize"""
    import oracle as O
    from dfmi import case
    m = um.get(name, "small", cyc)
    pt = case.default_patch_types(m)
    def through_flow(m, species):      # the TGV has no z velocity: add one, so that the cyclic pair carries flux
        f = _tgv(m, species)
        f["U"][2] = 1.0 + 2.0 * np.cos(m.cell_centres[:, 0] / 1e-3) * np.sin(m.cell_centres[:, 1] / 1e-3)
        return f
    ctx, t, st, inert, dt = _state(m, through_flow, pt)
    st = {k: v.copy() for k, v in st.items()}
    rng = np.random.default_rng(11)
    st["phi"] = st["phi"] * (1 + 0.3 * rng.standard_normal(m.n_faces))
    off = 0
    for p in m.patches:
        if p.kind != "cyclic":
            st["boundary_phi"][off:off + p.slots] = 0.0
        off += p.slots
    if cyc:
        assert np.abs(st["boundary_phi"]).max() > 0
    o = O.Oracle(m, t, st, pt, inert, 1.0 / dt)
    o.set("rho_old", st["rho"])
    o.rho_eqn()
    V = m.volume
    m0 = np.sum(st["rho"] * V)
    assert abs(np.sum(o["rho"] * V) - m0) <= 1e-13 * m0
    assert np.abs(o["rho"] - st["rho"]).max() > 1e-6 * st["rho"].max()     # the fluxes were not zero
    ctx.close()


@pytest.mark.parametrize("name", FAMILIES)
def test_cpu_a_outer_iteration_matches_oracle(name):
    """fixedValue U / T / Y on left and right, Burke-9, tight solves: test_cpu_a's thresholds"""
    import oracle as O
    m = um.get(name, "small")
    pt = _walls(m)
    ctx, t, st, inert, dt = _state(m, _tgv, pt)
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-15, 1e-300)
    o = O.Oracle(m, t, {k: v.copy() for k, v in st.items()}, pt, inert, 1.0 / dt)
    o.time_step(2)
    ctx.time_step(2)
    err = {n: rel_err(ctx.get_field(n, (m.n_cells,)), o[n]) for n in ("T", "p", "rho", "he")}
    err["U"] = rel_err(ctx.get_field("U", (3, m.n_cells)), o["U"])
    err["Y"] = rel_err(ctx.get_field("Y", (t.S, m.n_cells)), o["Y"])
    err["phi"] = rel_err(ctx.get_field("phi", (m.n_faces,)), o["phi"])
    err["boundary_p"] = rel_err(ctx.get_field("boundary_p", (m.n_boundary_slots,)), o["boundary_p"])
    print(name, err)
    for n, tl in {"T": 1e-10, "p": 1e-11, "rho": 1e-10, "he": 1e-10, "U": 1e-9, "Y": 1e-9, "phi": 1e-9,
                  "boundary_p": 1e-9}.items():
        assert err[n] < tl, (n, err[n])
    ctx.close()
