"""Spray coupling on the device (MI355X): the parcel source terms of the rho, U, Yi and he equations (include/dfmi.h, spray
block) against tests/spray_reference.py.

The fold is held bitwise twice over: the spray.model = 1 matrices are the same context's spray.model = 0 matrices plus the
NumPy terms, and they are the oracle's assembled matrices plus the terms (0 ulp, the parity suite's bound, on the hex box and
on the prism meshes alike). Off is off: fields set but spray.model = 0 changes no bit and no launch. A full outer iteration is
compared with the oracle's stages restated around the terms at the parity suite's bounds (T 1e-10, p 1e-11, rho 1e-10, U and
Y 1e-9). Then the solver audit, mass conservation of the explicit rho term, a decomposed step and the refusals by name.
"""
import threading

import numpy as np
import pytest

import spray_reference as R
import test_gpu_parity as P
import unstructured_meshes as um
from conftest import rel_err, ulp_diff

pytestmark = pytest.mark.gpu

EXPL = {"rho": 0, "U": 0, "Yi": 0, "h": 0}
SEMI = {"rho": 1, "U": 1, "Yi": 1, "h": 1}
SCH = {"explicit": EXPL, "semiImplicit": SEMI}
FIELD_OF = {"rhoTrans": "parcel_rhoTrans", "UTrans": "parcel_UTrans", "UCoeff": "parcel_UCoeff",
            "hsTrans": "parcel_hsTrans", "hsCoeffByCp": "parcel_hsCoeffByCp"}
LDU = ["lower", "upper", "internal_coeffs", "boundary_coeffs"]
ASSEMBLY = "k_rho,k_u_assemble,k_y_assemble,k_y_assemble_ell,k_y_assemble_gen,k_y_assemble_ell_gen,k_e_assemble"
FOLDS = "k_rho_spray,k_spray_u,k_spray_y,k_spray_e"


def _mech_n(n):
    """the first n - 1 species of the 53-species table and N2: n = 17 is the smallest count past the register-resident
    species kernels (S <= 16), so its YEqn runs the species-chunked *_gen kernels"""
    from dfmi.mech import ThermoTable
    ym, t = P._mech("gri53")
    idx = np.array(list(range(n - 1)) + [t.S - 1])
    sp = [ym["species"][i] for i in idx]
    assert sp[-1] == "N2" and {"H2", "O2", "H2O"} <= set(sp)
    return {"species": sp}, ThermoTable(sp, t.W[idx].copy(), t.nasa[idx].copy(), t.visc[idx].copy(), t.cond[idx].copy(),
                                        t.bdiff[np.ix_(idx, idx)].copy())


def _case(kind, mech="burke9", traversal=False, schemes=None):
    """hex: the parity suite's small mixed-BC box (6 x 5 x 4: fixedValue left, inletOutlet / waveTransmissive right);
    prisms / prisms-large: tests/unstructured_meshes.py's 210 and 6118 cells with the parity walls"""
    orig = P._mech
    if mech.startswith("s"):
        P._mech = lambda name: _mech_n(int(name[1:])) if name == mech else orig(name)
    try:
        if kind == "hex":
            nx, ny, nz = (16, 12, 8) if traversal else (6, 5, 4)
            return P._case(periodic=False, walls=lambda m: um.wall_types(m, True), mech=mech, mixed=True, nx=nx, ny=ny,
                           nz=nz, traversal=traversal)
        m = um.get("prisms", "large" if kind == "prisms-large" else "small")
        return P._case(periodic=False, walls=lambda mm: um.wall_types(mm, False), mech=mech, mesh=m, schemes=schemes)
    finally:
        P._mech = orig


_cases = {}


def _get(kind, mech="burke9", traversal=False):
    key = (kind, mech, traversal)
    if key not in _cases:
        c = _case(kind, mech, traversal)
        ctx, m, t, st, pt, inert, dt = c
        _cases[key] = c + (R.sources(m, t.S, inert, st["Y"]), R.hc_of(t))
    return _cases[key]


def teardown_module(module):
    for c in _cases.values():
        c[0].close()
    _cases.clear()


def _set_sources(ctx, src):
    for k, name in FIELD_OF.items():
        ctx.set_field(name, np.ascontiguousarray(src[k]))


def _mode(ctx, sch, model):
    for k, v in sch.items():
        ctx.set_option("spray." + k, v)
    ctx.set_option("spray.model", model)


def _tight(ctx):
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-15, 1e-300)


def _loose(ctx):
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 20, 1e-5)
    ctx.set_solver("p", 1000, 1e-5)


def _rows(ctx, m, S):
    W, n, C_ = P._ell_width(m), S - 1, m.n_cells
    return {p: ctx.get_solver_rows("Y", p, n * (W if p == "val" else 1) * C_) for p in ("val", "dS", "rhs")}


def _device(ctx, m, t, st, push):
    """every inspected matrix of the context in its present mode, each assembled from the pushed state"""
    C_, F, B, S = m.n_cells, m.n_faces, m.n_boundary_slots, t.S
    g = ctx.get_matrix
    out = {}
    push(); ctx.assemble("rho")
    out["rho"] = {"diag": ctx.get_field("dbg_rho_diag", (C_,)), "source": ctx.get_field("dbg_rho_source", (C_,)),
                  "rho": ctx.get_field("rho", (C_,)), "boundary_rho": ctx.get_field("boundary_rho", (B,))}
    push(); ctx.assemble("U")
    out["U"] = {p: g("U", p, n) for p, n in (("lower", F), ("upper", F), ("diag", C_), ("source", 3 * C_),
                                             ("source_solve", 3 * C_), ("internal_coeffs", 3 * B), ("boundary_coeffs", 3 * B))}
    out["U"]["rAU"] = ctx.get_field("rAU", (C_,))
    out["U"]["boundary_rAU"] = ctx.get_field("boundary_rAU", (B,))
    ctx.assemble("HbyA")
    out["U"]["HbyA"] = ctx.get_field("HbyA", (3, C_))
    push(); ctx.assemble("Y")
    out["Y"] = {p: g("Y", p, n) for p, n in (("lower", S * F), ("upper", S * F), ("diag", S * C_), ("source", S * C_),
                                             ("internal_coeffs", S * B), ("boundary_coeffs", S * B))}
    ctx.assemble("E")
    out["E"] = {p: g("E", p, n) for p, n in (("lower", F), ("upper", F), ("diag", C_), ("source", C_),
                                             ("internal_coeffs", B), ("boundary_coeffs", B))}
    push(); ctx.assemble("Y_ell")
    out["ell"] = _rows(ctx, m, S)
    push(); ctx.assemble("Y_ell_ref")
    out["ell_ref"] = _rows(ctx, m, S)
    push()
    return out


def _same(a, b, what):
    assert ulp_diff(a, b) == 0, (what, ulp_diff(a, b))


def _check_against_off(on, off, m, t, st, inert, dt, src, sch, hc):
    C_, S, V, rdt = m.n_cells, t.S, m.volume, 1.0 / dt
    d, s = R.rho_term(off["rho"]["diag"], off["rho"]["source"], src["rhoTrans"], rdt, V, st["rho"], sch["rho"])
    _same(on["rho"]["diag"], d, "rho diag"); _same(on["rho"]["source"], s, "rho source"); _same(on["rho"]["rho"], s / d, "rho")
    assert not np.array_equal(on["rho"]["rho"], off["rho"]["rho"])
    d, s, ss = R.u_term(off["U"]["diag"], off["U"]["source"].reshape(3, C_), off["U"]["source_solve"].reshape(3, C_),
                        src["UTrans"], src["UCoeff"], st["U"], rdt, sch["U"])
    _same(on["U"]["diag"], d, "U diag"); _same(on["U"]["source"], s, "U source"); _same(on["U"]["source_solve"], ss, "U source_solve")
    assert not np.array_equal(on["U"]["source"], off["U"]["source"])
    assert not np.array_equal(on["U"]["HbyA"], off["U"]["HbyA"])           # H reads the stored source
    assert np.array_equal(on["U"]["diag"], off["U"]["diag"]) == (not sch["U"])
    assert np.array_equal(on["U"]["rAU"], off["U"]["rAU"]) == (not sch["U"])
    d, s = R.y_term(off["Y"]["diag"].reshape(S, C_), off["Y"]["source"].reshape(S, C_), src["rhoTrans"], st["Y"], rdt, V,
                    inert, sch["Yi"])
    _same(on["Y"]["diag"], d, "Y diag"); _same(on["Y"]["source"], s, "Y source")
    assert not np.array_equal(on["Y"]["source"], off["Y"]["source"])
    keep = [i for i in range(S) if i != inert]
    for rows in ("ell", "ell_ref"):
        dS, rhs = np.zeros((S, C_)), np.zeros((S, C_))
        dS[keep], rhs[keep] = off[rows]["dS"].reshape(S - 1, C_), off[rows]["rhs"].reshape(S - 1, C_)
        d, s = R.y_term(dS, rhs, src["rhoTrans"], st["Y"], rdt, V, inert, sch["Yi"])
        _same(on[rows]["dS"], d[keep], rows + " dS"); _same(on[rows]["rhs"], s[keep], rows + " rhs")
        _same(on[rows]["val"], off[rows]["val"], rows + " val")
    for p in ("val", "dS", "rhs"):
        _same(on["ell"][p], on["ell_ref"][p], "Y_ell against Y_ell_ref " + p)
    d, s = R.e_term(off["E"]["diag"], off["E"]["source"], src["rhoTrans"], hc, src["hsTrans"], src["hsCoeffByCp"], st["he"],
                    rdt, V, sch["h"])
    _same(on["E"]["diag"], d, "E diag"); _same(on["E"]["source"], s, "E source")
    assert not np.array_equal(on["E"]["source"], off["E"]["source"])
    for eq in ("U", "Y", "E"):
        for p in LDU:
            assert np.array_equal(on[eq][p], off[eq][p]), (eq, p)


def _check_against_oracle(on, make_oracle, m, t, src, sch, hc):
    """the oracle's stages plus the terms: rho, U (rAU and HbyA included), Y, E at 0 ulp"""
    o = make_oracle()
    d, s = R.rho_stage(o, src, sch)
    _same(on["rho"]["diag"], d, "oracle rho diag"); _same(on["rho"]["source"], s, "oracle rho source")
    _same(on["rho"]["rho"], o["rho"], "oracle rho"); _same(on["rho"]["boundary_rho"], o["boundary_rho"], "oracle boundary_rho")
    o = make_oracle()
    u = R.u_stage(o, src, sch)
    for p in ("lower", "upper", "diag", "source", "source_solve", "internal_coeffs", "boundary_coeffs"):
        _same(on["U"][p], u[p], "oracle U " + p)
    _same(on["U"]["rAU"], o["rAU"], "oracle rAU"); _same(on["U"]["boundary_rAU"], o["boundary_rAU"], "oracle boundary_rAU")
    o.u_hbya()
    _same(on["U"]["HbyA"], o["HbyA"], "oracle HbyA")
    o = make_oracle()
    y = R.y_stage(o, src, sch)
    for p in ("lower", "upper", "diag", "source", "internal_coeffs", "boundary_coeffs"):
        _same(on["Y"][p], y[p], "oracle Y " + p)
    o.energy_gradient()
    o.correct_bc("he", "he", 1)
    e = R.e_stage(o, src, sch, hc)
    for p in ("lower", "upper", "diag", "source", "internal_coeffs", "boundary_coeffs"):
        _same(on["E"][p], e[p], "oracle E " + p)


def _inputs_cover_the_edges(m, t, st, inert, src):
    i, c = src["zero_cell"]
    assert st["Y"][i, c] == 0.0 and src["rhoTrans"][i, c] < 0 and i != inert      # the `small` denominator
    assert src["rhoTrans"][:, 1].sum() == 0.0 and np.abs(src["rhoTrans"][:, 1]).max() > 0
    assert src["hsCoeffByCp"][2] < 0 < src["hsCoeffByCp"][3]
    nz = (np.abs(src["rhoTrans"]).sum(axis=0) > 0).mean()
    assert 0.03 < nz < 0.4 and (src["rhoTrans"] > 0).any() and (src["rhoTrans"] < 0).any()
    assert (src["hsTrans"] > 0).any() and (src["hsTrans"] < 0).any() and (src["UCoeff"] >= 0).all()


# ------------------------------------------------------------------------------------------------ 1. the fold, bitwise
@pytest.mark.parametrize("scheme", list(SCH))
@pytest.mark.parametrize("kind,mech,trav", [("hex", "burke9", False), ("hex", "s17", False), ("prisms", "burke9", False),
                                           ("prisms", "s17", False), ("prisms-large", "burke9", False),
                                           ("hex", "burke9", True)],
                         ids=["hex-burke9", "hex-s17", "prisms-burke9", "prisms-s17", "prisms6118-burke9", "hex-traversal"])
def test_fold_bitwise(kind, mech, trav, scheme):
    from dfmi import case
    ctx, m, t, st, pt, inert, dt, src, hc = _get(kind, mech, trav)
    sch = SCH[scheme]
    _inputs_cover_the_edges(m, t, st, inert, src)
    push = lambda: case.push_state(ctx, st)
    _set_sources(ctx, src)
    _mode(ctx, sch, 0)
    off = _device(ctx, m, t, st, push)
    _mode(ctx, sch, 1)
    try:
        on = _device(ctx, m, t, st, push)
    finally:
        _mode(ctx, EXPL, 0)
    _check_against_off(on, off, m, t, st, inert, dt, src, sch, hc)
    _check_against_oracle(on, lambda: P._oracle(m, t, st, pt, inert, dt), m, t, src, sch, hc)


@pytest.mark.parametrize("scheme", list(SCH))
def test_fold_comes_after_the_explicit_nonorthogonal_term(scheme):
    """prisms 210 under `laplacian corrected`: the explicit non-orthogonal pass adds to the U, Y (LDU and solver rows) and
    E sources after the assembly kernel, and the parcel terms come after that pass -- the on matrices are still the off
    matrices, then the term, at 0 ulp"""
    from dfmi import case
    ctx, m, t, st, pt, inert, dt = _case("prisms", schemes={"laplacian": "corrected"})
    try:
        sch = SCH[scheme]
        src, hc = R.sources(m, t.S, inert, st["Y"]), R.hc_of(t)
        push = lambda: case.push_state(ctx, st)
        _set_sources(ctx, src)
        _mode(ctx, sch, 0)
        off = _device(ctx, m, t, st, push)
        _mode(ctx, sch, 1)
        ctx.kernel_timer("k_nonorth_corr," + FOLDS)
        on = _device(ctx, m, t, st, push)
        n = {k: ctx.kernel_time(k)[1] for k in ("k_nonorth_corr," + FOLDS).split(",")}
        ctx.kernel_timer("")
        assert n["k_nonorth_corr"] > 0 and n["k_spray_u"] > 0 and n["k_spray_y"] > 0 and n["k_spray_e"] > 0, n
        _check_against_off(on, off, m, t, st, inert, dt, src, sch, hc)
    finally:
        ctx.close()
    # and the corrected scheme is not a no-op on this mesh: the sources differ from the orthogonal context's
    plain = _get("prisms")
    case.push_state(plain[0], plain[3]); plain[0].assemble("U")
    assert not np.array_equal(plain[0].get_matrix("U", "source", 3 * m.n_cells), off["U"]["source"])
    case.push_state(plain[0], plain[3])


def test_species_chunked_kernels_start_at_17_species():
    """the witness of the mechanism choice above: 17 species launch the *_gen assemblies, 16 the register-resident ones"""
    from dfmi import case
    for mech, gen in (("s17", True), ("s16", False)):
        ctx, m, t, st = _get("hex", mech)[:4] if mech == "s17" else _case("hex", mech)[:4]
        try:
            ctx.kernel_timer(ASSEMBLY)
            ctx.assemble("Y"); ctx.assemble("Y_ell")
            n = {k: ctx.kernel_time(k)[1] for k in ASSEMBLY.split(",")}
            ctx.kernel_timer("")
            print(mech, n)
            assert (n["k_y_assemble_gen"] > 0 and n["k_y_assemble_ell_gen"] > 0) == gen, (mech, n)
            assert (n["k_y_assemble"] > 0 and n["k_y_assemble_ell"] > 0) == (not gen), (mech, n)
            case.push_state(ctx, st)
        finally:
            if mech != "s17":
                ctx.close()


@pytest.mark.parametrize("scheme", list(SCH))
@pytest.mark.parametrize("turb", ["les", "ras"])
def test_fold_bitwise_turbulent_instantiations(turb, scheme):
    """the hex box with les.model = 1 and with ras.model = 1: the assemblies' LesDiff<true> instantiations. The oracle is
    the LES one with the device's own nut injected (RAS: nut = Cmu k^2 / epsilon as the device formed it; Prt = Sct = 1 in
    both modes)."""
    from dfmi import case
    from test_gpu_turbulence import Case
    c = Case("mixed")
    ctx, m, t, st, pt, inert, dt = c.ctx, c.m, c.t, c.st, c.pt, c.inert, c.dt
    try:
        sch = SCH[scheme]
        src, hc = R.sources(m, t.S, inert, st["Y"]), R.hc_of(t)
        if turb == "les":
            nut, bnut = c.select(1)
        else:
            rng = np.random.default_rng(23)
            k, eps = 0.5 + rng.random(m.n_cells), 2e3 * (0.5 + rng.random(m.n_cells))
            from dfmi.mesh import ZERO_GRADIENT
            ctx.set_patch_types("k", m.patch_types(ZERO_GRADIENT)); ctx.set_patch_types("epsilon", m.patch_types(ZERO_GRADIENT))
            ctx.set_option("ras.model", 1)
            for n, v in (("k", k), ("epsilon", eps)):
                ctx.set_field(n, v)
                ctx.set_field("boundary_" + n, case.boundary_values(m, v).reshape(-1))
            case.push_state(ctx, st)
            ctx.assemble("U")                     # validates: correctNut() from k and epsilon
            nut, bnut = ctx.get_field("nut", (m.n_cells,)), ctx.get_field("boundary_nut", (m.n_boundary_slots,))
            assert nut.min() > 0
            st = dict(st, boundary_nut=bnut)      # what correctNut() left on the slots, kept across the pushes below

        def push():
            case.push_state(ctx, st)
            if turb == "les":                     # writing U invalidates the LES nut; the same U gives the same nut
                ctx.turbulence_correct()

        _set_sources(ctx, src)
        _mode(ctx, sch, 0)
        off = _device(ctx, m, t, st, push)
        _mode(ctx, sch, 1)
        on = _device(ctx, m, t, st, push)
        _check_against_off(on, off, m, t, st, inert, dt, src, sch, hc)
        _check_against_oracle(on, lambda: c.oracle(1, nut, bnut), m, t, src, sch, hc)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. off is off
def _step_fields(ctx, m, t):
    out = {n: ctx.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he")}
    out["U"] = ctx.get_field("U", (3, m.n_cells))
    out["Y"] = ctx.get_field("Y", (t.S, m.n_cells))
    out["phi"] = ctx.get_field("phi", (m.n_faces,))
    return out


def test_off_is_off():
    from dfmi import case
    res = {}
    for arm in ("never", "fields-set"):
        ctx, m, t, st, pt, inert, dt = _case("hex")
        try:
            if arm == "fields-set":
                _set_sources(ctx, R.sources(m, t.S, inert, st["Y"]))
                _mode(ctx, SEMI, 0)
            mats = _device(ctx, m, t, st, lambda: case.push_state(ctx, st))
            ctx.kernel_timer(ASSEMBLY + "," + FOLDS)
            ctx.time_step(2)
            n = {k: ctx.kernel_time(k)[1] for k in (ASSEMBLY + "," + FOLDS).split(",")}
            ctx.kernel_timer("")
            res[arm] = (mats, _step_fields(ctx, m, t), n)
        finally:
            ctx.close()
    a, b = res["never"], res["fields-set"]
    for eq, parts in a[0].items():
        for p, v in parts.items():
            assert np.array_equal(v, b[0][eq][p]), (eq, p)
    for n, v in a[1].items():
        assert np.array_equal(v, b[1][n]), n
    assert a[2] == b[2], (a[2], b[2])
    assert all(a[2][k] == 0 for k in FOLDS.split(",")) and a[2]["k_rho"] > 0 and a[2]["k_u_assemble"] > 0, a[2]


# ------------------------------------------------------------------------------------------------ 3. a full step
@pytest.mark.parametrize("scheme", list(SCH))
@pytest.mark.parametrize("kind", ["hex", "prisms"])
def test_full_step_against_the_restated_oracle(kind, scheme):
    from dfmi import case
    ctx, m, t, st, pt, inert, dt, src, hc = _get(kind)
    sch = SCH[scheme]
    case.push_state(ctx, st)
    _set_sources(ctx, src)
    _tight(ctx)
    _mode(ctx, sch, 1)
    try:
        ctx.kernel_timer(FOLDS)
        ctx.time_step(2)
        n = {k: ctx.kernel_time(k)[1] for k in FOLDS.split(",")}
        ctx.kernel_timer("")
        got = _step_fields(ctx, m, t)
    finally:
        _mode(ctx, EXPL, 0)
        _loose(ctx)
    assert n["k_rho_spray"] >= 1 and n["k_spray_u"] == 1 and n["k_spray_y"] == 1 and n["k_spray_e"] == 1, n
    o = P._oracle(m, t, st, pt, inert, dt)
    R.spray_time_step(o, src, sch, 2, hc)
    plain = P._oracle(m, t, st, pt, inert, dt)
    plain.time_step(2)
    for name, tol in (("T", 1e-10), ("p", 1e-11), ("rho", 1e-10), ("U", 1e-9), ("Y", 1e-9)):
        e = rel_err(got[name], o[name])
        moved = rel_err(plain[name], o[name])
        print(f"{kind} {scheme} {name}: rel {e:.3e} (bound {tol:g}); the terms move it by {moved:.3e}")
        assert e < tol, (name, e)
        assert moved > 100 * tol, (name, "the sources do not reach this field", moved)
    case.push_state(ctx, st)


# ------------------------------------------------------------------------------------------------ 4. the solver audit
@pytest.mark.parametrize("scheme", list(SCH))
def test_solves_with_sources_report_the_true_residual(scheme):
    """b - A x recomputed from dfmi_get_matrix (tests/solver_audit.py) after dfmi_U_process and dfmi_Y_process with the
    terms in force: the matrices handed out are the ones that were solved"""
    from dfmi import case
    from test_gpu_solver_audit import PRODUCTION, _audit_state, _sequence
    ctx, m, t, st, pt, inert, dt, _, hc = _get("hex")
    st2 = _audit_state(ctx, m, t, st, inert)
    src = R.sources(m, t.S, inert, st2["Y"], seed=13)      # (sinks of 1e-5 of the cell mass: far below the audited Y >= 1e-3)
    _set_sources(ctx, src)
    _mode(ctx, SCH[scheme], 1)
    try:
        tol, mi, mi_p = PRODUCTION
        out = _sequence(ctx, m, t, pt, inert, "spray " + scheme, tol, mi, mi_p, P._ell_width(m), eqns=("U", "Y"))
        assert set(out["iters"]) == {"U", "Y"}
    finally:
        _mode(ctx, EXPL, 0)
        _loose(ctx)
        case.push_state(ctx, st)


# ------------------------------------------------------------------------------------------------ 5. conservation
def test_explicit_rho_term_conserves_mass():
    """walled box at rest (phi = 0), explicit scheme: sum (rho - rho_old) V = sum_c sum_i rhoTrans, to 1e-13 of sum rho V
    (the rhoEqn bound of test_unstructured_meshes.py)"""
    from dfmi import case
    ctx, m, t, st, pt, inert, dt, src, hc = _get("prisms")
    st0 = dict(st, phi=np.zeros(m.n_faces), boundary_phi=np.zeros(m.n_boundary_slots))
    case.push_state(ctx, st0)
    src = dict(src, rhoTrans=100.0 * src["rhoTrans"])      # 1e-3 of the cell mass: the sum is far above the bound
    _set_sources(ctx, src)
    _mode(ctx, EXPL, 1)
    try:
        ctx.call("rho_process")
        rho = ctx.get_field("rho", (m.n_cells,))
    finally:
        _mode(ctx, EXPL, 0)
        case.push_state(ctx, st)
    V = np.asarray(m.volume, dtype=np.longdouble)
    gained = float(((rho.astype(np.longdouble) - st["rho_old"]) * V).sum())
    given = float(src["rhoTrans"].astype(np.longdouble).sum())
    scale = float((rho * V).sum())
    print(f"mass gained {gained:.6e} given {given:.6e} |difference| / sum rho V {abs(gained - given) / scale:.3e}")
    assert abs(given) > 1e-6 * scale
    assert abs(gained - given) <= 1e-13 * scale


# ------------------------------------------------------------------------------------------------ 6. decomposed
_HUB = [700]


def test_decomposed_step_with_sources_matches_single_domain():
    """8 x 4 x 4 split 2 x 1 x 1 over the in-process hub, one step with sources under the semi-implicit schemes: the terms
    are rank-local (no halo), so the ranks' fields are the single-domain ones to the bounds of
    test_decomposed_step_matches_single_domain (1e-9)"""
    from dfmi import case
    from dfmi.mesh import global_cell_ids, hex_box
    from test_gpu_multirank import _setup
    ym, t = P._mech("es80")
    Lb, dt, dims, decomp = (2 * np.pi * 1e-3,) * 3, 1e-6, (8, 4, 4), (2, 1, 1)
    mg = hex_box(*dims, lengths=Lb, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3)
    inert = ym["species"].index("N2")
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    src = R.sources(mg, t.S, inert, f["Y"])

    def run(m, comm, g):
        c = _setup(m, t, ym, dt, comm=comm)
        try:
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            c.call("pre_time_step")
            _set_sources(c, {k: np.ascontiguousarray(v[..., g]) for k, v in src.items() if k in FIELD_OF})
            _mode(c, SEMI, 1)
            c.time_step(2)
            return _step_fields(c, m, t)
        finally:
            c.close()

    ref = run(mg, None, np.arange(mg.n_cells))
    plain = _setup(mg, t, ym, dt)
    try:
        case.init_state(plain, mg, t.S, f["T"], f["p"], f["U"], f["Y"])
        plain.call("pre_time_step")
        plain.time_step(2)
        base = _step_fields(plain, mg, t)
    finally:
        plain.close()
    nr = int(np.prod(decomp))
    meshes = [hex_box(*dims, lengths=Lb, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3, decomp=decomp, rank=r) for r in range(nr)]
    gids = [global_cell_ids(mm, dims[0], dims[1]) for mm in meshes]
    out, err = [None] * nr, [None] * nr
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            out[r] = run(meshes[r], {"hub": hub, "nranks": nr, "rank": r}, gids[r])
        except Exception as e:      # surfaced below
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
    for n in ("T", "p", "rho", "he", "U", "Y"):
        glob = np.zeros_like(ref[n])
        for r in range(nr):
            glob[..., gids[r]] = out[r][n]
        e = rel_err(glob, ref[n])
        print(f"decomposed {n}: rel {e:.3e}; the terms move it by {rel_err(base[n], ref[n]):.3e}")
        assert e < 1e-9, (n, e)
        assert rel_err(base[n], ref[n]) > 1e-7, n


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_by_name():
    from dfmi import case
    from dfmi.lib import DfmiError
    ctx, m, t, st, pt, inert, dt = _case("hex")
    C_, S = m.n_cells, t.S
    try:
        src = R.sources(m, S, inert, st["Y"])
        for key in ("spray.rho", "spray.U", "spray.Yi", "spray.h", "spray.model"):
            for bad in (2, -1, 0.5):
                with pytest.raises(DfmiError, match=key.replace(".", r"\.")):
                    ctx.set_option(key, bad)
            assert ctx.get_option(key) == 0.0
        with pytest.raises(DfmiError, match=r"spray\.nope"):
            ctx.set_option("spray.nope", 1)
        # a required field never set, named; the coefficients only under their semi-implicit scheme
        ctx.set_option("spray.model", 1)
        # the zero-dimensional reactor ignores the model: it runs where every other entry refuses
        import os
        from conftest import GOLDEN
        from dfmi.kinetics import parse_mechanism
        ctx.chem_set_mechanism(parse_mechanism(os.path.join(GOLDEN, "Burke2012_s9r23.yaml")))
        ctx.chem_set_options(1)
        case.push_state(ctx, st)
        ctx.zero_d_step(dt, 1)
        ctx.chem_set_options(0)
        case.push_state(ctx, st)
        order = ["rhoTrans", "UTrans", "hsTrans"]
        for i, k in enumerate(order):
            for entry in ("rho_process", "U_process", "Y_process", "E_process"):
                with pytest.raises(DfmiError, match=FIELD_OF[k]):
                    ctx.call(entry)
            with pytest.raises(DfmiError, match=FIELD_OF[k]):
                ctx.time_step(2)
            with pytest.raises(DfmiError, match=FIELD_OF[k]):
                ctx.assemble("U")
            ctx.set_field(FIELD_OF[k], src[k])
        ctx.assemble("U"); ctx.assemble("E")                      # explicit: neither coefficient is needed
        ctx.set_option("spray.U", 1)
        with pytest.raises(DfmiError, match="parcel_UCoeff"):
            ctx.assemble("U")
        ctx.set_field("parcel_UCoeff", src["UCoeff"])
        ctx.assemble("U")
        ctx.set_option("spray.h", 1)
        with pytest.raises(DfmiError, match="parcel_hsCoeffByCp"):
            ctx.assemble("E")
        ctx.set_field("parcel_hsCoeffByCp", src["hsCoeffByCp"])
        ctx.assemble("E")
        # values and counts
        for k, name in FIELD_OF.items():
            for bad in (np.nan, np.inf, -np.inf):
                v = np.array(src[k], dtype=np.float64); v[..., 7] = bad
                with pytest.raises(DfmiError, match=name + ".*finite"):
                    ctx.set_field(name, v)
            with pytest.raises(DfmiError, match=name + ".*expected"):
                ctx.set_field(name, np.ascontiguousarray(src[k][..., :C_ - 1]))
            assert np.array_equal(ctx.get_field(name, np.shape(src[k])), src[k]), name      # a refused write changes nothing
        v = src["UCoeff"].copy(); v[5] = -1e-12
        with pytest.raises(DfmiError, match="parcel_UCoeff.*negative"):
            ctx.set_field("parcel_UCoeff", v)
        # an equation of state
        a = np.full(S, 1e5); b = np.full(S, 0.02); w = np.full(S, 0.1)
        ctx.thermo_set_eos(1, a, b, w)
        for entry in ("rho_process", "U_process"):
            with pytest.raises(DfmiError, match=r"spray\.model = 1.*equation of state"):
                ctx.call(entry)
        with pytest.raises(DfmiError, match=r"spray\.model = 1.*equation of state"):
            ctx.time_step(2)
        ctx.set_option("spray.model", 0)
        with pytest.raises(DfmiError, match=r"spray\.model = 1.*equation of state"):
            ctx.set_option("spray.model", 1)
        ctx.thermo_set_eos(0)
        ctx.set_option("spray.model", 1)
    finally:
        ctx.close()


def test_refused_with_flarefgm():
    """fgm.model = 1 and spray.model = 1 exclude each other, whichever comes second"""
    from dfmi.lib import DfmiError
    from dfmi.mesh import hex_box
    from test_gpu_fgm import FR, _bare_context, _species_maps
    m = hex_box(3, 2, 2, lengths=(3e-3, 2e-3, 2e-3), periodic=(False,) * 3)
    ctx, t, pt = _bare_context(m, ras=True)
    try:
        tab = FR.make_table("full")
        ctx.fgm_set_table(tab, *_species_maps(tab, t.S))
        ctx.set_option("fgm.model", 1)
        with pytest.raises(DfmiError, match=r"spray\.model = 1.*fgm\.model = 1"):
            ctx.set_option("spray.model", 1)
        ctx.set_option("fgm.model", 0)
        ctx.set_option("spray.model", 1)
        with pytest.raises(DfmiError, match=r"fgm\.model = 1.*spray\.model = 1"):
            ctx.set_option("fgm.model", 1)
    finally:
        ctx.close()
