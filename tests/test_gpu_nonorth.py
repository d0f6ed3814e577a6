"""Non-orthogonal laplacians on the GPU (MI355X): dfmi_set_scheme("laplacian", uncorrected | corrected) and the pEqn's
non-orthogonal corrector loop (option p.n_nonorth), DESIGN.md 13.

  geometry    the four geometry fields are bitwise Mesh.nonorth_geometry
  implicit    the matrices are bitwise the unchanged oracle's on a Mesh whose delta_coeffs are the non-orthogonal ones
  explicit    source - that oracle's source = the NumPy restatement's correction (tests/nonorth_reference.py), within
              gpu_bound(): 4x the restatement's own error against long double on the same kind of state, per mesh and
              field, floored at 1e-13, of the per-cell scale; beside it only the rounding of fl(source + term)
  exactness   the assembled E and Y matrices applied to a quadratic leave the ddt part minus gamma tr(H) V
  p loop      p and phi equal the restated loop with exact solves to 1e-9; the continuity residual formed from the
              returned phi is at solver tolerance for every p.n_nonorth
  consistency, decomposition, errors

Every test fails without the feature at the dfmi_set_scheme("laplacian", ...) call.
"""
import threading

import numpy as np
import pytest

import nonorth_reference as R
import unstructured_meshes as um
from conftest import rel_err, ulp_diff
from test_gpu_parity import _case, _oracle, _mech

pytestmark = pytest.mark.gpu

PARTS = ["lower", "upper", "diag", "internal_coeffs", "boundary_coeffs"]
BOUNDS = R.load_bounds()
_HUB = [900]


def _walls(mm):
    """unstructured_meshes.wall_types on the patches that are walls; coupled patches keep their own codes"""
    fv = um.wall_types(mm)
    base = mm.patch_types(0)
    coupled = [i for i, p in enumerate(mm.patches) if p.kind in R.COUPLED_KINDS]
    for k in fv:
        fv[k][coupled] = base[coupled]
    return fv


def _build(name, scheme, mesh=None):
    m = mesh if mesh is not None else R.get_mesh(name)
    return _case(periodic=False, walls=_walls, mech="burke9",
                 schemes={"laplacian": scheme} if scheme else None, mesh=m)


def _fields(ctx, m, S):
    out = {n: ctx.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he")}
    out["U"] = ctx.get_field("U", (3, m.n_cells))
    out["Y"] = ctx.get_field("Y", (S, m.n_cells))
    out["phi"] = ctx.get_field("phi", (m.n_faces,))
    return out


def _within(diff, want, scale, bound, what, rounding=0.0):
    """|diff - want| <= bound * scale + rounding per entry. `rounding` is what the format costs where the term is
    added to a much larger number: the library stores fl(source + term), so source' - source carries half a unit in
    the last place of the source whatever the term's own accuracy (the callers say how many such roundings)."""
    err = np.abs(diff - want)
    over = np.maximum(err - rounding, 0.0)
    has = scale > 0
    safe = np.where(has, scale, 1.0)
    worst = float((over / safe)[has].max()) if has.any() else 0.0
    print(f"{what}: max (|gpu - restated| - rounding) / scale = {worst:.3e} (bound {bound:.3e}), max |gpu - restated| / "
          f"scale = {float((err / safe)[has].max()):.3e}, max |term| / scale = {float((np.abs(want) / safe)[has].max()):.3e}, "
          f"median rounding allowance / scale = {float(np.median((np.broadcast_to(rounding, err.shape) / safe)[has])):.3e}")
    assert np.isfinite(diff).all() and (over <= bound * scale).all(), (what, worst, bound)


def _half_ulp(*a):
    """half a unit in the last place of the largest of the arrays, per entry: one rounding of a sum that large"""
    return 0.5 * np.spacing(np.maximum.reduce([np.abs(x) for x in a]))


# ----------------------------------------------------------------------------------------------- 1. geometry
@pytest.mark.parametrize("name", ["sheared-periodic", "refined"])
def test_geometry_fields_bitwise(name):
    ctx, m, t, st, pt, inert, dt = _build(name, "corrected")
    dc, k, bdc, bk = m.nonorth_geometry()
    F, B = m.n_faces, m.n_boundary_slots
    assert np.array_equal(ctx.get_field("nonorth_delta_coeffs", (F,)), dc)
    assert np.array_equal(ctx.get_field("nonorth_corr", (3, F)), k.T)
    assert np.array_equal(ctx.get_field("nonorth_corr", (F, 3), layout=1), k)
    assert np.array_equal(ctx.get_field("boundary_nonorth_delta_coeffs", (B,)), bdc)
    assert np.array_equal(ctx.get_field("boundary_nonorth_corr", (3, B)), bk.T)
    assert np.abs(k).max() > (0.1 if name.startswith("sheared") else 0.0)
    from dfmi.lib import DfmiError
    with pytest.raises(DfmiError, match="cannot be set"):
        ctx.set_field("nonorth_delta_coeffs", dc)
    ctx.close()


# ----------------------------------------------------------------------------------------------- 2. implicit part
@pytest.fixture(scope="module", params=[f"{n}:{s}" for n in R.MESHES for s in ("uncorrected", "corrected")])
def nc(request):
    name, scheme = request.param.split(":")
    out = _build(name, scheme)
    request.addfinalizer(out[0].close)
    return out + (name, scheme)


def _bitwise(ctx, eqn, ref, parts):
    bad = {p: ulp_diff(ctx.get_matrix(eqn, p, ref[p].size), ref[p]) for p in parts}
    assert not any(bad.values()), (eqn, bad)


def _oracle_p(ctx, o):
    """the oracle's pEqn behind the library's U source (under `corrected` it carries the explicit term, which HbyA
    reads)"""
    o.u_assemble()
    o.set("ueqn_source", ctx.get_matrix("U", "source", 3 * o.m.n_cells))
    o.u_hbya()
    return o.p_assemble()


def test_implicit_part_bitwise_oracle_on_nonorth_mesh(nc):
    from dfmi import case
    ctx, m, t, st, pt, inert, dt, name, scheme = nc
    unc = scheme == "uncorrected"
    o = _oracle(R.nonorth_mesh(m), t, st, pt, inert, dt)
    ctx.assemble("U")
    _bitwise(ctx, "U", o.u_assemble(), PARTS + (["source", "source_solve"] if unc else []))
    assert ulp_diff(ctx.get_field("rAU", (m.n_cells,)), o["rAU"]) == 0
    ctx.assemble("HbyA"); ctx.assemble("p")
    _bitwise(ctx, "p", _oracle_p(ctx, o), PARTS + (["source"] if unc else []))
    o.y_prep()
    ctx.assemble("Y")
    _bitwise(ctx, "Y", o.y_assemble(), PARTS + (["source"] if unc else []))
    if unc:
        assert ulp_diff(ctx.get_field("diffAlphaD", (m.n_cells,)), o["diffAlphaD"]) == 0
    o.energy_gradient(); o.correct_bc("he", "he", 1)
    ctx.assemble("E")
    _bitwise(ctx, "E", o.e_assemble(), PARTS + (["source"] if unc else []))
    # the production rows against the folded LDU rows: values bitwise, rhs bitwise without the explicit term
    W = um.ell_width(m)
    n = t.S - 1
    ctx.assemble("Y_ell")
    got = {p: ctx.get_solver_rows("Y", p, n * (W if p == "val" else 1) * m.n_cells) for p in ("val", "dS", "rhs")}
    ctx.assemble("Y_ell_ref")
    for p in ("val", "dS") + (("rhs",) if unc else ()):
        assert ulp_diff(got[p], ctx.get_solver_rows("Y", p, got[p].size)) == 0, p
    # the non-orthogonal coefficients are not the orthogonal ones
    o0 = _oracle(m, t, st, pt, inert, dt)
    o0.y_prep()
    d = np.abs(o0.y_assemble()["lower"] - ctx.get_matrix("Y", "lower", t.S * m.n_faces)).max()
    assert d > 0
    case.push_state(ctx, st)


# ----------------------------------------------------------------------------------------------- 3. explicit part
def _explicit(out, name):
    """bound per field: R.gpu_bound (4x the restatement's own fp64-against-long-double error on this mesh's case
    state, tests/golden/nonorth_bounds.json, floored at 1e-13) of the per-cell scale; beside it only the rounding of the
    library's fl(source + term), half an ulp of the source per stored addition"""
    from dfmi import case
    ctx, m, t, st, pt, inert, dt = out[:7]
    C, B, S = m.n_cells, m.n_boundary_slots, t.S
    bd = {f: R.gpu_bound(BOUNDS, name, f) for f in R.FIELDS}
    o = _oracle(R.nonorth_mesh(m), t, st, pt, inert, dt)
    # U
    ctx.assemble("U")
    uref = o.u_assemble()
    acc, _, _, sc = R.corrected_term(m, pt["U"], st["U"], st["boundary_U"], np.repeat(st["mu"][None], 3, axis=0),
                                     bgam=np.repeat(st["boundary_mu"][None], 3, axis=0))
    for part in ("source", "source_solve"):
        got = ctx.get_matrix("U", part, 3 * C)
        _within((got - uref[part]).reshape(3, C), acc, sc, bd["U"], f"{name} U {part}",
                _half_ulp(got, uref[part]).reshape(3, C))
    assert np.abs(acc).max() > 0
    # p, first pass
    ctx.assemble("HbyA"); ctx.assemble("p")
    pref = _oracle_p(ctx, o)
    sl, ts = R.Slots(m), R.slot_types(m, pt["p"])
    g = R.gauss_grad(m, sl, ts, st["p"], st["boundary_p"])[None]
    accp, _, _, scp = R.correction(m, sl, ts, g, gam_face=pref["rhorAUf"], bgam_face=pref["boundary_rhorAUf"])
    gotp = ctx.get_matrix("p", "source", C)
    _within((gotp - pref["source"])[None], accp, scp, bd["p"], f"{name} p source", _half_ulp(gotp, pref["source"])[None])
    # Y and diffAlphaD
    o.y_prep()
    yref = o.y_assemble()
    ctx.assemble("Y")
    accy, _, _, scy = R.corrected_term(m, pt["Y"], st["Y"], st["boundary_Y"], st["rhoD"], bgam=st["boundary_rhoD"])
    goty = ctx.get_matrix("Y", "source", S * C)
    keep = np.arange(S) != inert
    _within((goty - yref["source"]).reshape(S, C)[keep], accy[keep], scy[keep], bd["Y"], f"{name} Y source",
            _half_ulp(goty, yref["source"]).reshape(S, C)[keep])
    ah, bah = st["alpha"][None] * st["hai"], st["boundary_alpha"][None] * st["boundary_hai"]
    acca, _, _, sca = R.corrected_term(m, pt["Y"], st["Y"], st["boundary_Y"], ah, bgam=bah)
    gotd = ctx.get_field("diffAlphaD", (C,))
    # diffAlphaD gains its S terms one stored addition at a time: half an ulp of the largest partial sum each
    rd = S * _half_ulp(gotd, o["diffAlphaD"], np.abs(o["diffAlphaD"]) + np.abs(acca / m.volume).sum(axis=0))
    _within(gotd - o["diffAlphaD"], acca.sum(axis=0) / m.volume, sca.sum(axis=0) / m.volume, bd["diffAlphaD"],
            f"{name} diffAlphaD", rd)
    # the production rows' rhs: what `corrected` adds to the rows `uncorrected` writes (the same context, the scheme
    # switched and back) is the restated term at the row's position. The rows' order is the solver's (even-odd); it is
    # recovered from the folded LDU rows
    n = S - 1
    ctx.assemble("Y_ell")
    rhs = ctx.get_solver_rows("Y", "rhs", n * C).reshape(n, C)
    ctx.assemble("Y_ell_ref")
    rref = ctx.get_solver_rows("Y", "rhs", n * C).reshape(n, C)
    src = ctx.get_matrix("Y", "source", S * C).reshape(S, C)[keep]
    bcf = ctx.get_matrix("Y", "boundary_coeffs", S * B).reshape(S, B)[keep]
    tsy = R.slot_types(m, pt["Y"])
    cell_rhs = src.copy()
    on = sl.prim & ~sl.coupled & (tsy != R.EMPTY)
    for i in range(n):
        np.add.at(cell_rhs[i], sl.cell[on], bcf[i, on])
    row = np.empty(C, int)
    row[np.argsort(cell_rhs[0], kind="stable")] = np.argsort(rref[0], kind="stable")
    assert np.abs(rref[:, row] - cell_rhs).max() <= 1e-12 * np.abs(cell_rhs).max()
    ctx.set_scheme("laplacian", "uncorrected")
    ctx.assemble("Y_ell")
    rhs0 = ctx.get_solver_rows("Y", "rhs", n * C).reshape(n, C)
    ctx.set_scheme("laplacian", "corrected")
    _within((rhs - rhs0)[:, row], accy[keep], scy[keep], bd["Y"], f"{name} Y_ell rhs", _half_ulp(rhs, rhs0)[:, row])
    # E: he's own term, minus V diffAlphaD's
    o.energy_gradient(); o.correct_bc("he", "he", 1)
    eref = o.e_assemble()
    ctx.assemble("Y"); ctx.assemble("E")
    acce, _, _, sce = R.corrected_term(m, pt["he"], st["he"][None], o["boundary_he"][None], st["alpha"][None],
                                       bgam=st["boundary_alpha"][None])
    gote = ctx.get_matrix("E", "source", C)
    # the kernel re-forms source = sL - (V diffAlphaD - div(hDiffCorrFlux)) with the corrected diffAlphaD, and he's term
    # is added after: four roundings that differ from the oracle's, each at most half an ulp of the cell's own largest
    # intermediate, |sL| <= |source| + |sR|, |sR| <= |V diffAlphaD| + sum_f |Sf . hDiffCorrFlux_f|
    hd, bhd = np.abs(o["hDiffCorrFlux"]), np.abs(o["boundary_hDiffCorrFlux"])
    hf = np.maximum(hd[:, m.owner], hd[:, m.neighbour])
    fa = (np.abs(m.sf).T * hf).sum(axis=0)
    divh = np.zeros(C)
    np.add.at(divh, m.owner, fa); np.add.at(divh, m.neighbour, fa)
    bsf = np.abs(m.boundary_arrays()[0]).T
    bh = np.maximum(bhd, hd[:, sl.cell])
    np.add.at(divh, sl.cell[sl.prim], (bsf * bh).sum(axis=0)[sl.prim])
    big = np.maximum(np.abs(gote), np.abs(eref["source"])) + 2 * (np.abs(m.volume * gotd) + divh)
    _within((gote - eref["source"])[None], acce - acca.sum(axis=0)[None], sce + sca.sum(axis=0)[None],
            max(bd["he"], bd["diffAlphaD"]), f"{name} E source", (4 * 0.5 * np.spacing(big))[None])
    case.push_state(ctx, st)


@pytest.mark.parametrize("name", R.MESHES)
def test_explicit_part_matches_restatement(name):
    out = _build(name, "corrected")
    try:
        _explicit(out, name)
    finally:
        out[0].close()


def test_explicit_part_species_generic():
    from dfmi import lib
    lib.DEFAULT_OPTIONS["fv.species_generic"] = 1
    try:
        out = _build("sheared-walls", "corrected")
    finally:
        lib.DEFAULT_OPTIONS.pop("fv.species_generic", None)
    _explicit(out, "sheared-walls")
    out[0].close()


def test_explicit_part_with_les_on_refined():
    """Smagorinsky, Sct = 0.7, Prt = 0.85: the term takes muEff, rhoD_i + mut / Sct and alphaEff, and diffAlphaD (dropped
    by the turbulent branch) stays zero"""
    from test_gpu_turbulence import Case as LesCase
    name = "refined"
    c = LesCase("walls", mesh=um.get(name))
    ctx, m, t, pt, inert = c.ctx, c.m, c.t, c.pt, c.inert
    C, S = m.n_cells, t.S
    c.prt, c.sct = 0.85, 0.7
    ctx.set_scheme("laplacian", "corrected")
    nut, bnut = c.select(1)
    st = c.st
    bd = {f: R.gpu_bound(BOUNDS, name, f) for f in R.FIELDS}
    c.m = R.nonorth_mesh(m)
    try:
        o = c.oracle(1, nut, bnut)
    finally:
        c.m = m
    eff = o.effective()
    # U
    uref = o.u_assemble()
    ctx.assemble("U")
    mu3, bmu3 = np.repeat(eff["mu"][0][None], 3, axis=0), np.repeat(eff["mu"][1][None], 3, axis=0)
    acc, _, _, sc = R.corrected_term(m, pt["U"], st["U"], st["boundary_U"], mu3, bgam=bmu3)
    got = ctx.get_matrix("U", "source", 3 * C)
    _bitwise(ctx, "U", uref, PARTS)
    _within((got - uref["source"]).reshape(3, C), acc, sc, bd["U"], "LES U source",
            _half_ulp(got, uref["source"]).reshape(3, C))
    assert np.abs(eff["mu"][0] - st["mu"]).max() > 0
    # Y
    o.y_prep()
    yref = o.y_assemble()
    ctx.assemble("Y")
    _bitwise(ctx, "Y", yref, PARTS)
    accy, _, _, scy = R.corrected_term(m, pt["Y"], st["Y"], st["boundary_Y"], eff["rhoD"][0], bgam=eff["rhoD"][1])
    goty = ctx.get_matrix("Y", "source", S * C)
    keep = np.arange(S) != inert
    _within((goty - yref["source"]).reshape(S, C)[keep], accy[keep], scy[keep], bd["Y"], "LES Y source",
            _half_ulp(goty, yref["source"]).reshape(S, C)[keep])
    assert not ctx.get_field("diffAlphaD", (C,)).any()
    # E
    o.energy_gradient(); o.correct_bc("he", "he", 1)
    eref = o.e_assemble()
    ctx.assemble("E")
    _bitwise(ctx, "E", eref, PARTS)
    acce, _, _, sce = R.corrected_term(m, pt["he"], st["he"][None], o["boundary_he"][None], eff["alpha"][0][None],
                                       bgam=eff["alpha"][1][None])
    gote = ctx.get_matrix("E", "source", C)
    _within((gote - eref["source"])[None], acce, sce, bd["he"], "LES E source", _half_ulp(gote, eref["source"])[None])
    ctx.close()


# ----------------------------------------------------------------------------------------------- 4. exactness
def test_exactness_through_the_library():
    """The library's implicit and explicit parts add up to the exact laplacian of a quadratic. The walled 9 x 7 x 5
    sheared box (an affine image of a uniform grid), he and one species of Y set to phi = x.H.x / 2 + a.x at the cell
    centres, fixed-value slots to phi at the face centres, uniform diffusivity, U = 0, phi = 0, dpdt = 0, no reaction.
    The Gauss gradient is then exact from the second cell layer inwards and the corrected laplacian in the cells at
    least two layers from every wall (5 x 3 x 1): there the residual of the assembled matrix applied to the field is
    the ddt part minus gamma tr(H) V, to the CPU test's bound (4x the long-double restatement's committed deviation).
    The species' partner carries c - phi with the same rhoD, so sumYDiffError and with it phiUc vanish."""
    from dfmi import case
    from dfmi.mesh import FIXED_VALUE, FIXED_ENERGY
    from oracle import ldu_system
    name = "sheared-315"
    m = R.get_mesh(name)
    fixed = lambda mm: {"U": mm.patch_types(0), "T": mm.patch_types(FIXED_VALUE), "Y": mm.patch_types(FIXED_VALUE),
                        "he": mm.patch_types(FIXED_ENERGY)}
    out = _case(periodic=False, walls=fixed, mech="burke9", schemes={"laplacian": "corrected"}, mesh=m)
    try:
        _exactness(out)
    finally:
        out[0].close()


def _exactness(out):
    from dfmi import case
    from oracle import ldu_system
    ctx, m, t, st, pt, inert, dt = out
    C, B, S = m.n_cells, m.n_boundary_slots, t.S
    sl = R.Slots(m)
    keep = np.ones(C, bool)
    keep[sl.cell] = False                            # the wall layer, then the layer that touches it
    near = ~keep
    keep[m.owner[near[m.neighbour]]] = False
    keep[m.neighbour[near[m.owner]]] = False
    assert keep.sum() == 15
    x0 = m.cell_centres[keep].mean(axis=0)          # values stay small beside their differences in the checked cells
    H = np.array([[1.3, 0.4, -0.2], [0.4, -0.7, 0.5], [-0.2, 0.5, 2.1]]) * 1e6
    a = np.array([3.0, -2.0, 1.0]) * 1e2
    q = lambda x: 0.5 * np.einsum("ci,ij,cj->c", x - x0, H, x - x0) + (x - x0) @ a
    qc, qb = q(m.cell_centres), q(m.boundary_face_centres)
    trH = float(np.trace(H))
    # a diffusivity of order one: the ddt coefficients rdt rho V (1e6 rho V) then round at 1e-16 of the laplacian
    # term instead of 1e-11, and the check sees the laplacian at the bound
    gamma = 1.7
    rdt = 1.0 / dt
    base = dict(st)
    base["rho"] = np.full(C, 1.1); base["rho_old"] = 1.1 * (1 + 1e-3 * np.cos(np.arange(C)))
    for k in ("U", "U_old", "phi", "phi_old", "K", "K_old", "dpdt", "RR", "boundary_U", "boundary_phi", "boundary_K",
              "hai", "boundary_hai"):
        base[k] = np.zeros_like(st[k])
    base["alpha"] = np.full(C, gamma); base["boundary_alpha"] = np.full(B, gamma)
    base["rhoD"] = np.full((S, C), gamma); base["boundary_rhoD"] = np.full((S, B), gamma)
    bound = 4 * BOUNDS["exactness_longdouble"]
    V = np.asarray(m.volume, R.LD)

    def residual(eqn, ptypes, x, parts, sys):
        F = m.n_faces
        g = lambda k, n: ctx.get_matrix(eqn, k, parts * n)[sys * n:(sys + 1) * n]
        rows, cols, vals, b = ldu_system(m, ptypes, g("lower", F), g("upper", F), g("diag", C), g("source", C),
                                         g("internal_coeffs", B), g("boundary_coeffs", B))
        r = -np.asarray(b, R.LD)                       # the matrix applied in long double: the test adds no rounding
        np.add.at(r, rows, np.asarray(vals, R.LD) * np.asarray(x, R.LD)[cols])
        return r

    def miss(r, x, g):
        """|residual - (ddt part - g tr(H) V)| / (g |tr(H)| V) over the checked cells"""
        ddt = (np.asarray(rdt * base["rho"], R.LD) - np.asarray(rdt * base["rho_old"], R.LD)) * V * np.asarray(x, R.LD)
        return float((np.abs(r - (ddt - g * trH * V))[keep] / (g * abs(trH) * V[keep])).max())
    # he, uniform Y
    s = dict(base)
    s["Y"] = np.repeat(st["Y"][:, :1], C, axis=1); s["boundary_Y"] = np.repeat(st["Y"][:, :1], B, axis=1)
    s["he"] = qc; s["boundary_he"] = qb
    case.push_state(ctx, s)
    ctx.assemble("Y"); ctx.assemble("E")
    assert not ctx.get_field("diffAlphaD", (C,)).any()
    ee = miss(residual("E", pt["he"], qc, 1, 0), qc, gamma)
    ctx.set_scheme("laplacian", "uncorrected")     # the implicit part alone misses by tens of percent on the same cells
    ctx.assemble("Y"); ctx.assemble("E")
    eu = miss(residual("E", pt["he"], qc, 1, 0), qc, gamma)
    ctx.set_scheme("laplacian", "corrected")
    # one species: Y_a = amp phi and its partner Y_b = -amp phi with the same rhoD, every other species zero, so
    # sumYDiffError and phiUc are exactly zero (the assembly does not ask Y to be a mixture)
    ia, ib = [i for i in range(S) if i != inert][:2]
    amp = 5e-2 / np.abs(qc).max()
    s = dict(base)
    s["Y"] = np.zeros((S, C)); s["boundary_Y"] = np.zeros((S, B))
    s["Y"][ia] = amp * qc; s["boundary_Y"][ia] = amp * qb
    s["Y"][ib] = -amp * qc; s["boundary_Y"][ib] = -amp * qb
    case.push_state(ctx, s)
    ctx.assemble("Y")
    assert not ctx.get_field("phiUc", (m.n_faces,)).any()
    ey = miss(residual("Y", pt["Y"], s["Y"][ia], S, ia), s["Y"][ia], gamma * amp)
    print(f"exactness through the library: E {ee:.3e}, Y {ey:.3e} (bound {bound:.3e}); uncorrected E misses by {eu:.3e}")
    assert eu > 1e-2
    assert ee <= bound and ey <= bound

# ----------------------------------------------------------------------------------------------- 5. pressure loop
@pytest.fixture(scope="module", params=["sheared-walls", "refined"])
def pl(request):
    out = _build(request.param, "corrected")
    request.addfinalizer(out[0].close)
    res = {}
    return out + (request.param, res)


def _p_residuals(m, st, dt, parts, base, rf, brf, pt_p, p, bp, phi, bphi, phiHbyA_div):
    """(continuity residual from the returned phi, fully corrected residual A p - base - correction(p)), per cell"""
    sl, ts = R.Slots(m), R.slot_types(m, pt_p)
    C = m.n_cells
    div = np.zeros(C)
    np.add.at(div, m.owner, phi); np.add.at(div, m.neighbour, -phi)
    on = sl.prim & (ts != R.EMPTY)
    np.add.at(div, sl.cell[on], bphi[on])
    rdt = 1.0 / dt
    cont = st["psi"] * rdt * m.volume * (p - st["p"]) + m.volume * rdt * (st["rho"] - st["rho_old"]) + div
    from oracle import ldu_system
    import scipy.sparse as sp
    rows, cols, vals, b = ldu_system(m, pt_p, parts["lower"], parts["upper"], parts["diag"], base,
                                     parts["internal_coeffs"], parts["boundary_coeffs"])
    A = sp.coo_matrix((vals, (rows, cols)), shape=(C, C)).tocsr()
    g = R.gauss_grad(m, sl, ts, p, bp)[None]
    acc = R.correction(m, sl, ts, g, gam_face=rf, bgam_face=brf)[0][0]
    return cont, A @ p - b - acc


@pytest.mark.parametrize("n_nonorth", [0, 1, 3])
def test_pressure_corrector_loop(pl, n_nonorth):
    from dfmi import case
    ctx, m, t, st, pt, inert, dt, name, res = pl
    C, F, B = m.n_cells, m.n_faces, m.n_boundary_slots
    case.push_state(ctx, st)
    ctx.set_solver("p", 3000, 1e-12, 1e-300)
    ctx.set_option("p.n_nonorth", n_nonorth)
    ctx.assemble("U"); ctx.assemble("HbyA")
    ctx.call("p_process")
    o = _oracle(R.nonorth_mesh(m), t, st, pt, inert, dt)
    pref = _oracle_p(ctx, o)
    parts = {k: ctx.get_matrix("p", k, pref[k].size) for k in PARTS}
    rf, brf = ctx.get_field("rhorAUf", (F,)), ctx.get_field("boundary_rhorAUf", (B,))
    p, bp, fl, bfl = R.p_loop(m, pt["p"], parts, pref["source"], rf, brf, st["p"], st["boundary_p"], n_nonorth)
    gp, gbp = ctx.get_field("p", (C,)), ctx.get_field("boundary_p", (B,))
    phi, bphi = ctx.get_field("phi", (F,)), ctx.get_field("boundary_phi", (B,))
    ph, bph = ctx.get_field("phiHbyA", (F,)), ctx.get_field("boundary_phiHbyA", (B,))
    # printed beside the assertion on p itself: the error relative to what the solve changed (p moves by ~1e-4 of itself)
    ep = np.abs(gp - p).max() / np.abs(p - st["p"]).max()
    ephi = rel_err(phi, ph + fl)
    ebphi = np.abs(bphi - (bph + bfl)).max() / max(np.abs(bph + bfl).max(), np.abs(ph + fl).max())
    cont, full = _p_residuals(m, st, dt, parts, pref["source"], rf, brf, pt["p"], gp, gbp, phi, bphi, None)
    scale = np.abs(parts["diag"] * gp).max()
    res[n_nonorth] = np.abs(full).max()
    print(f"{name} n_nonorth {n_nonorth}: p {ep:.3e} phi {ephi:.3e} boundary_phi {ebphi:.3e} continuity "
          f"{np.abs(cont).max() / scale:.3e} fully corrected residual {np.abs(full).max() / scale:.3e} "
          f"iters {ctx.solver_stats('p')[0]}")
    assert rel_err(gp, p) < 1e-9
    assert ephi < 1e-9 and ebphi < 1e-9
    # solver tolerance: 1e-12 of the initial residual, itself below |diag p| per cell; rounding of the row sums adds
    # a few eps of |diag p|
    assert np.abs(cont).max() <= 1e-10 * scale
    if n_nonorth == 3:
        print(f"{name}: fully corrected residual after 3 correctors / after 0 = {res[3] / res[0]:.3e}")
        assert res[3] < res[0]
    ctx.set_option("p.n_nonorth", 0)
    case.push_state(ctx, st)


# ----------------------------------------------------------------------------------------------- 6. consistency
def _step(scheme, mesh=None, n_nonorth=0, traversal=None, tight=True):
    from dfmi import case
    if mesh is None:
        out = _case(mech="burke9", schemes={"laplacian": scheme} if scheme else None)   # periodic graded hex_box 6x5x4
    else:
        out = _build(None, scheme, mesh=mesh)
    ctx, m, t, st = out[:4]
    if tight:
        for e in ("U", "Y", "E"):
            ctx.set_solver(e, 300, 1e-14, 1e-300)
        ctx.set_solver("p", 3000, 1e-14, 1e-300)
    if n_nonorth:
        ctx.set_option("p.n_nonorth", n_nonorth)
    if traversal is not None:
        ctx.set_traversal(traversal)
    ctx.time_step(2)
    f = _fields(ctx, m, t.S)
    ctx.close()
    return f


def test_axis_aligned_box_corrected_equals_default():
    a, b = _step(None), _step("corrected")
    for k in a:
        e = rel_err(b[k], a[k])
        print("hex_box corrected vs default", k, e)
        assert e < 1e-12, (k, e)


def test_corrected_runs_are_deterministic_and_default_is_untouched():
    m = R.get_mesh("sheared-315")
    d0 = _step(None, mesh=m, tight=False)
    a = _step("corrected", mesh=m, n_nonorth=1, tight=False)
    b = _step("corrected", mesh=m, n_nonorth=1, tight=False)
    c = _step("corrected", mesh=m, n_nonorth=1, tight=False,
              traversal=np.random.default_rng(3).permutation(m.n_cells).astype(np.int32))
    d1 = _step(None, mesh=m, tight=False)
    for k in a:
        assert np.array_equal(a[k], b[k]), ("two runs", k)
        assert np.array_equal(a[k], c[k]), ("traversal", k)
        assert np.array_equal(d0[k], d1[k]), ("default after a corrected context", k)
    assert rel_err(a["U"], d0["U"]) > 1e-6      # the scheme does change the step on this mesh


# ----------------------------------------------------------------------------------------------- 7. decomposed
@pytest.mark.parametrize("name", ["sheared-315", "refined"])
def test_decomposed_corrected_step_matches_single_domain(name):
    from dfmi import case
    from dfmi.lib import Context
    from dfmi.partition import partition_cells, decompose
    mg = R.get_mesh(name)
    ym, t = _mech("burke9")
    dt = 1e-6
    inert = ym["species"].index("N2")
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)

    def setup(m, comm=None):
        c = Context(0)
        case.setup_context(c, m, t, inert, dt, case.default_patch_types(m), comm=comm, schemes={"laplacian": "corrected"})
        for e in ("U", "Y", "E"):
            c.set_solver(e, 300, 1e-14, 1e-300)
        c.set_solver("p", 3000, 1e-14, 1e-300)
        c.set_option("p.n_nonorth", 1)
        return c

    def run(c, m, g):
        case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
        c.call("pre_time_step")
        c.time_step(2)
        o = {n: c.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he")}
        o["U"] = c.get_field("U", (3, m.n_cells))
        o["Y"] = c.get_field("Y", (t.S, m.n_cells))
        # phi, which carries the face flux correction across processor slots: per cell the sum of the outward fluxes
        # over internal faces and every primary slot (a processor face is an internal face of the single domain), and
        # the sum of their magnitudes as its scale
        phi, bphi = c.get_field("phi", (m.n_faces,)), c.get_field("boundary_phi", (m.n_boundary_slots,))
        sl = R.Slots(m)
        div, mag = np.zeros(m.n_cells), np.zeros(m.n_cells)
        np.add.at(div, m.owner, phi); np.add.at(div, m.neighbour, -phi)
        np.add.at(mag, m.owner, np.abs(phi)); np.add.at(mag, m.neighbour, np.abs(phi))
        np.add.at(div, sl.cell[sl.prim], bphi[sl.prim]); np.add.at(mag, sl.cell[sl.prim], np.abs(bphi[sl.prim]))
        o["div_phi"], o["mag_phi"] = div, mag
        c.close()
        return o

    ref = run(setup(mg), mg, np.arange(mg.n_cells))
    meshes = decompose(mg, partition_cells(mg, 2, "graph"))
    nr = len(meshes)
    out, err = [None] * nr, [None] * nr
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            m = meshes[r]
            out[r] = run(setup(m, comm={"hub": hub, "nranks": nr, "rank": r}), m, m.cell_map)
        except Exception as e:
            err[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not any(x.is_alive() for x in th), "decomposed run hung"
    for e in err:
        if e is not None:
            raise e
    for n, k in (("T", 1), ("p", 1), ("rho", 1), ("he", 1), ("U", 3), ("Y", t.S)):
        a = np.zeros((k, mg.n_cells))
        for r in range(nr):
            a[:, meshes[r].cell_map] = out[r][n].reshape(k, -1)
        e = rel_err(a, ref[n].reshape(k, -1))
        print(name, "decomposed vs single domain", n, e)
        assert e < 1e-9, (n, e)
    got = {k: np.zeros(mg.n_cells) for k in ("div_phi", "mag_phi")}
    for r in range(nr):
        for k in got:
            got[k][meshes[r].cell_map] = out[r][k]
    e_mag = rel_err(got["mag_phi"], ref["mag_phi"])
    e_div = np.abs(got["div_phi"] - ref["div_phi"]).max() / ref["mag_phi"].max()
    print(name, "decomposed vs single domain phi: sum |phi| per cell", e_mag, "div phi over max sum |phi|", e_div)
    assert e_mag < 1e-9 and e_div < 1e-9


# ----------------------------------------------------------------------------------------------- 8. errors
def test_errors_leave_the_context_usable():
    from dfmi import case
    from dfmi.lib import Context, DfmiError, load
    import os
    ym, t = _mech("burke9")
    inert = ym["species"].index("N2")
    m = R.get_mesh("sheared-periodic")

    def ctx_with(mesh_distance=True, bdelta=True, lib_path=None):
        c = Context(0, lib_path)
        pt = case.default_patch_types(m)
        rows, cols = m.proc_rows_cols()
        c.set_constant_values(m.n_cells, m.n_cells, m.n_faces, m.n_boundary_slots, m.n_patches, 0, m.patch_sizes, t.S, 1e6)
        c.set_cyclic_info(m.cyclic_neighbour())
        c.set_constant_indexes(m.owner, m.neighbour, rows, cols, 0)
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (m.sf, m.mag_sf, m.weight, m.delta_coeffs, m.volume,
                                                                    m.mesh_distance)]
        import ctypes as C
        ptrs = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]
        if not mesh_distance:
            ptrs[5] = None
        c._call("dfmi_init_constant_fields_internal", c.h, *ptrs)
        bsf, bmag, bdc, bw, bfc = m.boundary_arrays()
        c.init_constant_fields_boundary(bsf, bmag, bdc, bw, bfc, pt["calculated"], pt["extrapolated"])
        if bdelta:
            c.init_boundary_delta(m.boundary_delta())
        return c

    c = ctx_with(mesh_distance=False)
    with pytest.raises(DfmiError, match="mesh_distance"):
        c.set_scheme("laplacian", "corrected")
    c.set_scheme("laplacian", "orthogonal")
    c.close()
    c = ctx_with(bdelta=False)
    with pytest.raises(DfmiError, match="dfmi_init_boundary_delta"):
        c.set_scheme("laplacian", "Gauss linear corrected")
    c.init_boundary_delta(m.boundary_delta())
    c.set_scheme("laplacian", "Gauss linear corrected")
    with pytest.raises(DfmiError, match="limited"):
        c.set_scheme("laplacian", "Gauss linear limited corrected 0.5")
    with pytest.raises(DfmiError, match="unsupported"):
        c.set_scheme("laplacian", "faceCorrected")
    with pytest.raises(DfmiError, match="p.n_nonorth"):
        c.set_option("p.n_nonorth", -1)
    with pytest.raises(DfmiError, match="p.n_nonorth"):
        c.set_option("p.n_nonorth", 1.5)
    c.set_option("p.n_nonorth", 2)
    assert c.get_option("p.n_nonorth") == 2
    # the scheme in force survived the refused calls
    dc = m.nonorth_geometry()[0]
    assert np.array_equal(c.get_field("nonorth_delta_coeffs", (m.n_faces,)), dc)
    # an initialiser called again re-forms the geometry: other patch deltas, other coupled-slot coefficients
    import copy
    m2 = copy.copy(m)
    m2.patches = [copy.copy(p) for p in m.patches]
    for p in m2.patches:
        p.delta = np.asarray(p.delta) * np.array([1.0, 1.25, 1.0])
    c.init_boundary_delta(m2.boundary_delta())
    _, _, bdc2, bk2 = m2.nonorth_geometry()
    B = m.n_boundary_slots
    assert np.array_equal(c.get_field("boundary_nonorth_delta_coeffs", (B,)), bdc2)
    assert np.array_equal(c.get_field("boundary_nonorth_corr", (3, B)), bk2.T)
    assert not np.array_equal(bdc2, m.nonorth_geometry()[2])
    c.close()
    cpu_a = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "baseline", "cpu_a", "libdfmi_cpu_a.so")
    load(cpu_a)
    c = ctx_with(lib_path=cpu_a)
    for s in ("corrected", "Gauss linear uncorrected"):
        with pytest.raises(DfmiError, match="CPU-A"):
            c.set_scheme("laplacian", s)
    c.set_scheme("laplacian", "Gauss linear orthogonal")
    c.close()
