"""Adjustable time step on the MI355X (dfLowMachFoam.C:261-262): the device Courant number (k_courant and its
fixed-order reduction) against the NumPy restatement (tests/courant_reference.py) on the meshes where a reduction can
go wrong, dfmi_set_delta_t against a context set up at the new step (bitwise) and against the oracle, the AMG reuse
window across step changes, the closed loop of dfmi.timestep.advance, two in-process ranks, and the error returns.

The Courant tolerance is courant_reference.tolerance: (faces per cell + C) 2^-52 relative, from the summation
lengths. Face walks covered: the computed hex walk (boxes in blockMesh order), the gather rows (the renumbered box:
six couplings per cell, no blockMesh order) and the CSR lists (the 1D flame). Every mesh the suite builds, renumbered
or read from polyMesh, has at most 3 owned faces per cell and so takes the owner-slot face storage (fslot = 1; _fslot
restates capi.cpp's rule and the test asserts it): the OpenFOAM-order storage (fslot = 0) differs in one index
expression of the CSR walk and is not reached here."""
import os
import threading

import numpy as np
import pytest

from conftest import GOLDEN, rel_err, ulp_diff
import courant_reference as CR

pytestmark = pytest.mark.gpu

TPB = 256   # k_courant's workgroup (fv_kernels.hip TPB)
_HUB = [700]


def _es80():
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
    return ym, read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])


def _burke():
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "Burke2012_s9r23.yaml"))
    return ym, read_thermo_table(os.path.join(GOLDEN, "thermo_Burke2012_s9r23.txt"), ym["species"])


def _fslot(m) -> bool:
    """capi.cpp dfmi_set_constant_indexes: owner-slot face storage unless a cell owns > 3 faces and padding > 25 %"""
    kmax = int(np.bincount(m.owner, minlength=m.n_cells).max())
    return kmax <= 3 or kmax * m.n_cells <= m.n_faces + m.n_faces // 4


def _distorted(nx, ny, nz, seed=5, amp=0.15):
    """the non-orthogonal fixture of test_gpu_parity.py: a walled box with its interior points moved, through polyMesh"""
    import tempfile
    from dfmi.polymesh import hex_polymesh, read_polymesh, write_polymesh
    L = (2 * np.pi * 1e-3,) * 3
    P, faces, own, nei, bnd = hex_polymesh(nx, ny, nz, lengths=L, periodic=(False,) * 3)
    h = np.array(L) / np.array([nx, ny, nz])
    inner = np.all((P > 1e-12) & (P < np.array(L) - 1e-12), axis=1)
    P = P.copy()
    P[inner] += amp * h * np.random.default_rng(seed).uniform(-1, 1, (inner.sum(), 3))
    with tempfile.TemporaryDirectory() as d:
        write_polymesh(d, P, faces, own, nei, bnd)
        return read_polymesh(d)


def _open_outlet_types(m):
    """test_cpu_a.py's walled box: fixed inlet on "left", inletOutlet U / Y and waveTransmissive p on "right" """
    from dfmi import case
    from dfmi.mesh import FIXED_VALUE, FIXED_ENERGY, GRADIENT_ENERGY, INLET_OUTLET, WAVE_TRANSMISSIVE
    pt = case.default_patch_types(m)
    left = [i for i, p in enumerate(m.patches) if p.name == "left"]
    right = [i for i, p in enumerate(m.patches) if p.name == "right"]
    for f in ("U", "T", "Y"):
        pt[f] = m.patch_types(0).copy(); pt[f][left] = FIXED_VALUE
    pt["he"] = m.patch_types(GRADIENT_ENERGY).copy(); pt["he"][left] = FIXED_ENERGY
    pt["U"][right] = INLET_OUTLET; pt["Y"][right] = INLET_OUTLET
    pt["p"] = m.patch_types(0).copy(); pt["p"][right] = WAVE_TRANSMISSIVE
    return pt


# ------------------------------------------------------------------ 1. the Courant number against the restatement
def _mesh(kind):
    from dfmi import case
    from dfmi.mesh import hex_box
    L = (2 * np.pi * 1e-3,) * 3
    walls = (False,) * 3
    if kind == "255":
        return hex_box(3, 5, 17, lengths=L, periodic=walls), None
    if kind == "256":
        return hex_box(4, 8, 8, lengths=L, periodic=walls), None
    if kind == "257":
        return hex_box(1, 1, 257, lengths=L, periodic=walls), None
    if kind == "ragged-17-blocks":      # 4335 cells: 16 full blocks and 239 cells; >= 16 blocks: the XCD block remap
        return hex_box(15, 17, 17, lengths=L, periodic=(True,) * 3, gradings=(1.0, 1.4, 0.8)), None
    if kind == "263-blocks":            # more partials than the second stage has threads
        return hex_box(41, 41, 40, lengths=L, periodic=(True, False, True), gradings=(1.0, 1.3, 1.0)), None
    if kind == "graded":
        return hex_box(9, 7, 6, lengths=L, periodic=(True,) * 3, gradings=(2.0, 0.5, 1.7)), None
    if kind == "open-outlet":
        m = hex_box(8, 6, 5, lengths=L, periodic=walls, gradings=(1.0, 1.4, 1.0))
        return m, _open_outlet_types(m)
    if kind == "flame1d":
        m = case.flame1d_mesh()
        return m, case.flame1d_patch_types(m)
    if kind == "distorted":
        return _distorted(7, 6, 5), None
    if kind in ("bricks", "traversal"):
        m = hex_box(16, 12, 9, lengths=L, periodic=(True, False, True), gradings=(1.0, 1.3, 1.0))
        if kind == "bricks":
            from dfmi.renumber import renumber_mesh
            m, _ = renumber_mesh(m, "bricks")
        return m, None
    raise KeyError(kind)


MESHES = ["255", "256", "257", "ragged-17-blocks", "263-blocks", "graded", "open-outlet", "flame1d", "distorted",
          "bricks", "traversal"]


def _courant_ctx(kind, dt=1e-6):
    from dfmi import case
    from dfmi.lib import Context, renumber_cells
    ym, t = _burke() if kind == "flame1d" else _es80()
    m, pt = _mesh(kind)
    ctx = Context(0)
    case.setup_context(ctx, m, t, ym["species"].index("N2"), dt, pt)
    if kind == "traversal":
        ijk = np.stack(m.local_index, axis=1).astype(np.float64)
        ctx.set_traversal(renumber_cells(m.n_cells, ijk, m.owner, m.neighbour, "bricks"))
    return ctx, m


def _spiked(m, rng, where):
    """random fluxes of both signs, rho in [0.5, 1.5), and a spike that puts the maximum of sumPhi / V at a chosen
    place: cell 0, the last cell (the last lane of the ragged block), or through a boundary face"""
    C, F, B = m.n_cells, m.n_faces, m.n_boundary_slots
    phi = rng.uniform(-1, 1, F) * 1e-9
    bphi = rng.uniform(-1, 1, B) * 1e-9
    rho = rng.uniform(0.5, 1.5, C)
    if where == "cell0":
        cell = 0
        f = np.flatnonzero((m.owner == 0) | (m.neighbour == 0))
        phi[f[0]] = -3e-6
    elif where == "last":
        cell = C - 1
        f = np.flatnonzero((m.owner == C - 1) | (m.neighbour == C - 1))
        phi[f[-1]] = 3e-6
    else:
        fc, off, kind = [p for p in CR.mesh_patches(m) if p[2] != "empty" and len(p[0])][-1]
        cell = int(fc[len(fc) // 2])
        bphi[off + len(fc) // 2] = -3e-6
    rho[cell] *= 1e-3      # the spiked face's other cell stays 1000 times below
    return phi, bphi, rho, cell


@pytest.mark.parametrize("kind", MESHES)
def test_courant_number_matches_the_restatement(kind):
    dt = 1e-6
    ctx, m = _courant_ctx(kind, dt)
    assert _fslot(m)   # no mesh the suite builds takes the OpenFOAM-order face storage (see the module docstring)
    tol = CR.tolerance(m)
    rng = np.random.default_rng(11)
    for where in ("cell0", "last", "boundary"):
        phi, bphi, rho, cell = _spiked(m, rng, where)
        ctx.set_field("phi", phi); ctx.set_field("boundary_phi", bphi); ctx.set_field("rho", rho)
        sp = CR.sum_phi(m.n_cells, m.owner, m.neighbour, CR.mesh_patches(m), phi, bphi, rho)
        assert int(np.argmax(sp / m.volume)) == cell
        ref = CR.courant_no(m, phi, bphi, rho, dt)
        got = ctx.courant_no()
        print(kind, where, "cells", m.n_cells, "blocks", -(-m.n_cells // TPB), "got", got, "ref", ref,
              "rel", [abs(g - r) / r for g, r in zip(got, ref)], "tol", tol)
        for g, r in zip(got, ref):
            assert abs(g - r) <= tol * r, (kind, where)
        assert ctx.courant_no() == got      # a second evaluation of the same fields: the same bits
    ctx.close()


# ------------------------------------------------------------------ 2. / 3. a changed step: bitwise, and the oracle
def _box_state(dt_setup, chem):
    """8^3 walled ES80 box with the open outlet; returns a context set up at dt_setup"""
    from dfmi import case
    from dfmi.kinetics import parse_mechanism
    from dfmi.lib import Context
    from dfmi.mesh import hex_box
    ym, t = _es80()
    m = hex_box(8, 8, 8, lengths=(2 * np.pi * 1e-3,) * 3, periodic=(False,) * 3, gradings=(1.0, 1.3, 1.0))
    pt = _open_outlet_types(m)
    inert = ym["species"].index("N2")
    ctx = Context(0)
    case.setup_context(ctx, m, t, inert, dt_setup, pt)
    if chem:
        ctx.chem_set_mechanism(parse_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml")))
        ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
    yu, _ = case.h2_air_compositions(ym["species"])
    f = case.tgv_fields(m, ym["species"], kernel_radius=1.2e-3)
    case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"],
                    refs={"U": {"right": np.array([0.3, -0.1, 0.2])}, "Y": {"right": yu}}, gammas={"right": 1.4})
    ctx.call("pre_time_step")
    return ctx, m, t, pt, inert


def _flame_state(dt_setup):
    """test_gpu_flame1d.py's case (waveTransmissive outlet, Burke chemistry) set up at dt_setup"""
    from dfmi import case
    from dfmi.kinetics import parse_mechanism
    from dfmi.lib import Context
    ym, t = _burke()
    m = case.flame1d_mesh()
    pt = case.flame1d_patch_types(m)
    inert = ym["species"].index("N2")
    ctx = Context(0)
    case.setup_context(ctx, m, t, inert, dt_setup, pt)
    ctx.chem_set_mechanism(parse_mechanism(os.path.join(GOLDEN, "Burke2012_s9r23.yaml")))
    ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
    f, bv = case.flame1d_fields(os.path.join(GOLDEN, "flame1d"), ym["species"])
    case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"], bvals=bv,
                    gammas=case.flame1d_gamma(os.path.join(GOLDEN, "flame1d")))
    ctx.call("pre_time_step")
    return ctx, m, t, pt, inert


@pytest.mark.parametrize("which", ["box-es80-chem", "flame1d"])
def test_changed_step_is_bitwise_a_context_set_up_at_it(which):
    from dfmi import case
    dt1, dt2 = 1e-6, 4e-7
    make = (lambda d: _box_state(d, True)) if which.startswith("box") else _flame_state
    B_, m, t, pt, inert = make(dt2)
    st = case.pull_state(B_, m, t.S)
    A, *_ = make(dt1)
    for c in (A, B_):
        case.push_state(c, st)
    A.set_delta_t(dt2)
    assert A.delta_t() == dt2
    for c in (A, B_):
        c.time_step(2)
    a, b = case.pull_state(A, m, t.S), case.pull_state(B_, m, t.S)
    worst = {k: ulp_diff(a[k], b[k]) for k in a}
    print(which, "max ulp", max(worst.values()), "boundary_p_vf", worst["boundary_p_vf"])
    assert all(v == 0 for v in worst.values()), {k: v for k, v in worst.items() if v}
    assert np.abs(b["RR"]).max() > 0 and b["boundary_p_vf"].max() > 0
    assert ulp_diff(A.get_field("chem_stats", (3, m.n_cells)), B_.get_field("chem_stats", (3, m.n_cells))) == 0
    for e in ("U", "Y", "E", "p"):
        assert A.solver_stats(e) == B_.solver_stats(e), e
    # ... and it is not the step the context was set up with
    C_, *_ = make(dt1)
    case.push_state(C_, st)
    C_.time_step(2)
    assert ulp_diff(C_.get_field("p", (m.n_cells,)), b["p"]) > 0
    for c in (A, B_, C_):
        c.close()


def test_step_after_set_delta_t_matches_oracle_at_the_new_step():
    """the full-step tolerances of test_gpu_parity.py / test_gpu_flame1d.py, the waveTransmissive valueFraction
    1 / (1 + w dt deltaCoeffs) included"""
    import oracle as O
    from dfmi import case
    dt1, dt2 = 1e-6, 2.5e-7
    ctx, m, t, pt, inert = _box_state(dt1, False)
    rng = np.random.default_rng(7)
    st = case.pull_state(ctx, m, t.S)
    st["rho_old"] = st["rho"] * (1 + 1e-3 * rng.standard_normal(m.n_cells))
    st["U_old"] = st["U"] * (1 + 1e-2 * rng.standard_normal((3, m.n_cells)))
    st["phi_old"] = st["phi"] * (1 + 1e-2 * rng.standard_normal(m.n_faces))
    st["p_old"] = st["p"] * (1 + 1e-4 * rng.standard_normal(m.n_cells))
    st["RR"] = 1e2 * rng.standard_normal((t.S, m.n_cells))
    st["dpdt"] = 1e3 * rng.standard_normal(m.n_cells)
    case.push_state(ctx, st)
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-15, 1e-300)
    ctx.set_delta_t(dt2)
    o = O.Oracle(m, t, {k: v.copy() for k, v in st.items()}, pt, inert, 1.0 / dt2)
    o.time_step(2)
    ctx.time_step(2)
    B = m.n_boundary_slots
    for n, tl in {"T": 1e-10, "p": 1e-11, "rho": 1e-10, "he": 1e-10}.items():
        e = rel_err(ctx.get_field(n, (m.n_cells,)), o[n])
        assert e < tl, (n, e)
    assert rel_err(ctx.get_field("U", (3, m.n_cells)), o["U"]) < 1e-9
    assert rel_err(ctx.get_field("Y", (t.S, m.n_cells)), o["Y"]) < 1e-9
    assert rel_err(ctx.get_field("phi", (m.n_faces,)), o["phi"]) < 1e-9
    assert rel_err(ctx.get_field("dpdt", (m.n_cells,)), o["dpdt"]) < 1e-9
    assert rel_err(ctx.get_field("boundary_p", (B,)), o["boundary_p"]) < 1e-9
    vf = ctx.get_field("boundary_p_vf", (B,))
    right = case.patch_slots(m, "right")
    assert np.all((vf[right] > 0) & (vf[right] < 1))
    assert rel_err(vf, o["boundary_p_vf"]) < 1e-12
    o1 = O.Oracle(m, t, {k: v.copy() for k, v in st.items()}, pt, inert, 1.0 / dt1)
    o1.time_step(2)
    assert rel_err(o1["boundary_p_vf"], o["boundary_p_vf"]) > 1e-3   # the old step's is another one
    ctx.close()


# ------------------------------------------------------------------ 4. the AMG reuse window
def _tgv(n, dt, opts=None, u0=4.0):
    from dfmi import case
    from dfmi.lib import Context, DEFAULT_OPTIONS
    from dfmi.mesh import hex_box
    ym, t = _es80()
    m = hex_box(n, n, n, lengths=(2 * np.pi * 1e-3,) * 3, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3)
    DEFAULT_OPTIONS.update(opts or {})
    try:
        ctx = Context(0)
    finally:
        for k in (opts or {}):
            DEFAULT_OPTIONS.pop(k, None)
    case.setup_context(ctx, m, t, ym["species"].index("N2"), dt, case.default_patch_types(m))
    f = case.tgv_fields(m, ym["species"], kernel_radius=1.2e-3, u0=u0)
    case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"])
    ctx.call("pre_time_step")
    return ctx, m, t


def _fields(ctx, m, t):
    out = {k: ctx.get_field(k, (m.n_cells,)) for k in ("p", "T", "rho", "he")}
    out["U"] = ctx.get_field("U", (3, m.n_cells))
    out["Y"] = ctx.get_field("Y", (t.S, m.n_cells))
    out["phi"] = ctx.get_field("phi", (m.n_faces,))
    return out


STEP_FACTORS = [1.2] * 5 + [0.5] * 5


def _window(n, n_corr, opts, factors, set_same=False):
    dt = 1e-6
    ctx, m, t = _tgv(n, dt, opts)
    stats = []
    for f in factors:
        if f is not None:
            dt = dt * f
            ctx.set_delta_t(dt)
        elif set_same:
            ctx.set_delta_t(dt)
        ctx.time_step(n_corr)
        stats.append(ctx.solver_stats("p"))
    out = _fields(ctx, m, t)
    ctx.close()
    return out, stats


@pytest.mark.parametrize("n", [16, 20], ids=["16^3-one-workgroup-solves", "20^3-batched-solves"])
@pytest.mark.parametrize("n_corr", [2, 1], ids=["second-corrector", "first-corrector"])
def test_changed_step_ends_the_reuse_window(n, n_corr):
    """10 steps, the step size changed before every one (x 1.2 five times, then x 0.5): with the default
    amg.reuse_steps the run is bitwise the run that rebuilds the hierarchy values every step (amg.reuse_steps = 1).
    dfmi_solver_stats reports a step's last p solve: n_corr = 2 shows every step's second corrector, n_corr = 1 its
    first -- the solve the window would have preconditioned with old operators. Each meets the tolerance before
    max_iter (amgxpOptions: 1e-5, 1000)."""
    a, sa = _window(n, n_corr, None, STEP_FACTORS)
    b, sb = _window(n, n_corr, {"amg.reuse_steps": 1}, STEP_FACTORS)
    print("p solves (iters, res0, rel):", sa)
    assert {k: ulp_diff(a[k], b[k]) for k in a} == {k: 0 for k in a}
    assert sa == sb
    for it, _, rel in sa:
        assert rel <= 1e-5 and 0 < it < 1000, (it, rel)


def test_setting_the_step_in_force_resets_nothing():
    """constant step: dfmi_set_delta_t(the same value) before every step is bitwise the run without the calls, reuse
    window included (the hierarchy is rebuilt on steps 1 and 9 in both: the p iteration counts agree step by step)"""
    a, sa = _window(16, 2, None, [None] * 10)
    b, sb = _window(16, 2, None, [None] * 10, set_same=True)
    assert {k: ulp_diff(a[k], b[k]) for k in a} == {k: 0 for k in a}
    assert sa == sb
    # the window is live in this run: rebuilding every step gives other bits
    c, _ = _window(16, 2, {"amg.reuse_steps": 1}, [None] * 10)
    assert ulp_diff(a["p"], c["p"]) > 0


# ------------------------------------------------------------------ 5. the closed loop
def test_closed_loop_follows_the_rules_and_the_record_is_the_restatement():
    from dfmi.timestep import advance, initial_delta_t, next_delta_t
    dt0, max_co, n_steps = 1e-6, 0.5, 12
    probe, m, t = _tgv(16, dt0)
    co4, _ = probe.courant_no()
    probe.close()
    u0 = 4.0 * (2 * max_co) / co4          # Co is linear in u0: the first Courant number ~ 2 maxCo
    ctx, m, t = _tgv(16, dt0, u0=u0)
    co0, mean0 = ctx.courant_no()
    assert co0 == pytest.approx(2 * max_co, rel=1e-3) and 0 < mean0 < co0
    dt_init = max_co * dt0 / co0
    ctl = {"deltaT": dt0, "adjustTimeStep": True, "maxCo": max_co, "maxDeltaT": 1.6 * dt_init}
    assert initial_delta_t(dt0, co0, max_co, ctl["maxDeltaT"]) == dt_init    # shrinks by exactly maxCo / Co0
    pulled = []

    def grab(c, i):
        pulled.append((c.get_field("phi", (m.n_faces,)), c.get_field("boundary_phi", (m.n_boundary_slots,)),
                       c.get_field("rho", (m.n_cells,))))
    hist = advance(ctx, ctl, n_steps, after_step=grab)
    assert ctx.get_option("step.courant") == 1.0
    last = ctx.courant_no()                 # the record of the last step
    on = _fields(ctx, m, t)
    ctx.close()
    tol = CR.tolerance(m)
    dt = dt_init
    for i, (got_dt, co, mean) in enumerate(hist):
        new = next_delta_t(dt, co, max_co, ctl["maxDeltaT"])
        assert got_dt == new                                   # the history is the rule on the reported Co, bitwise
        assert new <= 1.2 * dt and new <= ctl["maxDeltaT"]
        dt = new
    # every number reported from a step's record is the restatement on the fields pulled after that step
    reported = [(h[1], h[2]) for h in hist[1:]] + [last]
    for i, (phi, bphi, rho) in enumerate(pulled):
        ref = CR.courant_no(m, phi, bphi, rho, hist[i][0])
        for g, r in zip(reported[i], ref):
            assert abs(g - r) <= tol * r, (i, g, r)
    # step.courant off: the same loop with the number launched on demand -- the same history and fields, bitwise
    ctx, m, t = _tgv(16, dt0, u0=u0)
    co, mean = ctx.courant_no()
    ctx.set_delta_t(initial_delta_t(ctx.delta_t(), co, max_co, ctl["maxDeltaT"]))
    hist_off = []
    for _ in range(n_steps):
        co, mean = ctx.courant_no()
        ctx.set_delta_t(next_delta_t(ctx.delta_t(), co, max_co, ctl["maxDeltaT"]))
        ctx.time_step(2)
        hist_off.append((ctx.delta_t(), co, mean))
    assert ctx.get_option("step.courant") == 0.0
    assert hist_off == hist
    off = _fields(ctx, m, t)
    assert {k: ulp_diff(on[k], off[k]) for k in on} == {k: 0 for k in on}
    ctx.close()


# ------------------------------------------------------------------ 6. two in-process ranks
def test_two_ranks_agree_bitwise_and_with_the_single_domain():
    import oracle as O
    from dfmi import case
    from dfmi.lib import Context
    from dfmi.mesh import hex_box, global_cell_ids
    ym, t = _es80()
    inert = ym["species"].index("N2")
    L = (2 * np.pi * 1e-3,) * 3
    dims, dt1, dt2 = (8, 6, 4), 1e-6, 4e-7
    kw = dict(lengths=L, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3)
    mg = hex_box(*dims, **kw)
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)

    def setup(m, comm=None):
        c = Context(0)
        case.setup_context(c, m, t, inert, dt1, case.default_patch_types(m), comm=comm)
        for e in ("U", "Y", "E"):
            c.set_solver(e, 300, 1e-14, 1e-300)
        c.set_solver("p", 3000, 1e-14, 1e-300)
        return c
    ctx = setup(mg)
    case.init_state(ctx, mg, t.S, f["T"], f["p"], f["U"], f["Y"])
    ctx.call("pre_time_step")
    st = case.pull_state(ctx, mg, t.S)
    single = ctx.courant_no()
    ctx.close()
    ref = CR.courant_no(mg, st["phi"], st["boundary_phi"], st["rho"], dt1)
    orc = O.Oracle(mg, t, {k: v.copy() for k, v in st.items()}, case.default_patch_types(mg), inert, 1.0 / dt2)
    orc.time_step(2)
    nr = 2
    meshes = [hex_box(*dims, decomp=(2, 1, 1), rank=r, **kw) for r in range(nr)]
    gids = [global_cell_ids(mm, dims[0], dims[1]) for mm in meshes]
    out, err = [None] * nr, [None] * nr
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            m, g = meshes[r], gids[r]
            c = setup(m, comm={"hub": hub, "nranks": nr, "rank": r})
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            c.call("pre_time_step")
            o = {"co": c.courant_no()}
            c.set_delta_t(dt2)
            o["co2"] = c.courant_no()
            c.time_step(2)
            for n in ("T", "p", "rho", "he"):
                o[n] = c.get_field(n, (m.n_cells,))
            o["U"] = c.get_field("U", (3, m.n_cells))
            o["Y"] = c.get_field("Y", (t.S, m.n_cells))
            out[r] = o
            c.close()
        except Exception as e:   # surfaced below
            err[r] = e
    th = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    assert not any(x.is_alive() for x in th), "decomposed run hung"
    for e in err:
        if e is not None:
            raise e
    assert out[0]["co"] == out[1]["co"] and out[0]["co2"] == out[1]["co2"]      # the same bits on both ranks
    tol = CR.tolerance(mg)
    print("two ranks", out[0]["co"], "single", single, "restatement", ref, "tol", tol)
    for g, s, r in zip(out[0]["co"], single, ref):
        assert abs(g - s) <= tol * s and abs(g - r) <= tol * r
    for g, r in zip(out[0]["co2"], CR.courant_no(mg, st["phi"], st["boundary_phi"], st["rho"], dt2)):
        assert abs(g - r) <= tol * r
    for n, k in (("T", 1), ("p", 1), ("rho", 1), ("he", 1), ("U", 3), ("Y", t.S)):
        a = np.zeros((k, mg.n_cells))
        for r in range(nr):
            a[:, gids[r]] = out[r][n].reshape(k, -1)
        e = rel_err(a, orc[n].reshape(k, -1))
        assert e < 1e-9, (n, e)


# ------------------------------------------------------------------ 7. errors
def test_errors_leave_the_step_unchanged():
    import ctypes
    from dfmi.lib import Context, DfmiError
    ctx, m = _courant_ctx("graded", 1e-6)

    def last_error():
        buf = ctypes.create_string_buffer(1024)
        ctx.lib.dfmi_last_error(buf, 1024)
        return buf.value.decode()
    for bad in (0.0, -1e-6, float("nan"), float("inf")):
        assert ctx.lib.dfmi_set_delta_t(ctx.h, ctypes.c_double(bad)) != 0
        assert "delta_t" in last_error()
        assert ctx.delta_t() == 1e-6
    co = ctypes.c_double()
    for args in ((None, None), (ctypes.byref(co), None), (None, ctypes.byref(co))):
        assert ctx.lib.dfmi_courant_no(ctx.h, *args) != 0
        assert "null" in last_error()
    assert ctx.delta_t() == 1e-6
    rng = np.random.default_rng(3)
    phi, bphi, rho, _ = _spiked(m, rng, "cell0")
    ctx.set_field("phi", phi); ctx.set_field("boundary_phi", bphi); ctx.set_field("rho", rho)
    assert ctx.courant_no()[0] > 0          # and the context still works
    fresh = Context(0)
    with pytest.raises(DfmiError, match="dfmi_set_constant_values"):
        fresh.set_delta_t(1e-6)
    with pytest.raises(DfmiError):
        fresh.delta_t()
    with pytest.raises(DfmiError):
        fresh.courant_no()
    fresh.close()
    ctx.close()
