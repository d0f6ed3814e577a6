"""RAS k-epsilon on the device (MI355X): the k and epsilon equations feeding nut (include/dfmi.h dfmi_turbulence_correct,
RAS block), held to the NumPy restatement tests/ras_reference.py.

Homogeneous decay to 1e-12; G and divU per cell against the long-double restatement at 4x the fp64 restatement's
measured error per mesh (tests/golden/ras_bounds.json), floored at 1e-13; both matrices at 0 ulp with the device's own G,
divU and nut injected; bound() against the restatement's bound() of the device's own solved field; full steps against
RasOracle; validity and options.

bound(): the device keeps the solved fields bound() gathers from (k_prebound / epsilon_prebound, get only), so the
pre-bound solution is read directly. A twin context with ras.kMin / ras.epsilonMin at -1e300 cannot supply it: both
options must be positive, and with such a floor bound() still raises a negative cell to its neighbours' average. Seeds:
epsilon negative, k negative and positive below kMin. An exact zero is not seeded: writing k or epsilon invalidates nut,
which is then Cmu k^2 / epsilon of the seeded fields -- infinite for epsilon = 0 -- and k = 0 makes eps / k infinite in
the assembly, as it would in OpenFOAM.

Two ranks: the in-process transport, graph bisection of the sheared box (corrected laplacian, limitedLinear k) and of
`refined`, against the single-domain run.
"""
import threading

import numpy as np
import pytest

import nonorth_reference as NR
import ras_reference as R
from conftest import rel_err, ulp_diff
from test_gpu_parity import _case

pytestmark = pytest.mark.gpu

PARTS = ["lower", "upper", "diag", "source", "internal_coeffs", "boundary_coeffs"]
NONDEFAULT = {"Cmu": 0.11, "C1": 1.3, "C2": 1.7, "C3": -0.4, "sigmak": 0.9, "sigmaEps": 1.1}


def _tight(ctx):
    for e in ("U", "Y", "E", "k", "epsilon"):
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-15, 1e-300)


class Case:
    """a context on one of ras_reference's meshes in RAS mode; walls: "zg" (zeroGradient everywhere) or "mixed" (the parity
    suite's open outlet; k and epsilon fixedValue on left, inletOutlet on right)"""

    def __init__(self, name, walls="zg", schemes=None, small=1, coef=None):
        from dfmi import lib
        from dfmi.mesh import FIXED_VALUE, INLET_OUTLET, ZERO_GRADIENT
        import unstructured_meshes as um
        self.name, self.m = name, R.get_mesh(name)
        m = self.m
        if not small:
            lib.DEFAULT_OPTIONS["solver.small"] = 0
        try:
            mixed = walls == "mixed"
            self.ctx, _, self.t, self.st, self.pt, self.inert, self.dt = _case(
                periodic=False, walls=(lambda mm: um.wall_types(mm, mixed=True)) if mixed else None, mech="burke9",
                mixed=mixed, schemes=schemes, mesh=m)
        finally:
            lib.DEFAULT_OPTIONS.pop("solver.small", None)
        self.q = dict(R.DEFAULTS, **(coef or {}))
        self.k_pt = m.patch_types(ZERO_GRADIENT).copy()
        self.ref = np.zeros(m.n_boundary_slots)
        if mixed:
            for i, p in enumerate(m.patches):
                if p.name == "left":
                    self.k_pt[i] = FIXED_VALUE
                elif p.name == "right":
                    self.k_pt[i] = INLET_OUTLET
        self.tp = R.Topo(m)
        ctx = self.ctx
        ctx.set_patch_types("k", self.k_pt)
        ctx.set_patch_types("epsilon", self.k_pt)
        for key, v in self.q.items():
            ctx.set_option("ras." + key, v)
        ctx.set_option("ras.model", 1)

    def set_ke(self, k, eps, bk=None, beps=None):
        from dfmi import case
        m, ctx = self.m, self.ctx
        bk = case.boundary_values(m, k).reshape(-1) if bk is None else bk
        beps = case.boundary_values(m, eps).reshape(-1) if beps is None else beps
        for n, v in (("k", k), ("epsilon", eps), ("boundary_k", bk), ("boundary_epsilon", beps)):
            ctx.set_field(n, np.ascontiguousarray(v, dtype=np.float64))
        return bk, beps

    def push(self, st):
        """the fields of a ras_state on the context (k and epsilon included)"""
        for n in ("U", "rho", "mu", "phi"):
            self.ctx.set_field(n, np.ascontiguousarray(st[n]))
            self.ctx.set_field("boundary_" + n, np.ascontiguousarray(st["boundary_" + n]))
        self.ctx.set_field("rho_old", np.ascontiguousarray(st["rho"] * (1 + 1e-3 * np.random.default_rng(5).standard_normal(self.m.n_cells))))
        self.set_ke(st["k"], st["epsilon"], st["boundary_k"], st["boundary_epsilon"])

    def get(self, n, boundary=False):
        return self.ctx.get_field(n, (self.m.n_boundary_slots if boundary or n.startswith("boundary_") else self.m.n_cells,))

    def restated(self, keq, wc=None, bwc=None, dc=None, bdc=None):
        """the restatement's matrix of one equation from the context's fields with the device's own G, divU and nut"""
        m, q = self.m, self.q
        C_, B, F = m.n_cells, m.n_boundary_slots, m.n_faces
        g = {n: self.get(n) for n in ("G", "divU", "nut", "rho", "rho_old", "mu", "k", "epsilon", "boundary_rho",
                                      "boundary_nut", "boundary_mu", "boundary_k", "boundary_epsilon", "boundary_phi")}
        phi = self.ctx.get_field("phi", (F,))
        Su, Sp = R.sources(keq, q, g["G"], g["divU"], g["rho"], g["k"], g["epsilon"])
        sig = q["sigmak"] if keq else q["sigmaEps"]
        D = R.diffusivity(g["rho"], g["nut"], g["mu"], sig)
        bD = R.diffusivity(g["boundary_rho"], g["boundary_nut"], g["boundary_mu"], sig)
        nm = "k" if keq else "epsilon"
        o = R.scalar_assemble(self.tp, self.k_pt, g[nm], g["boundary_" + nm], g["rho"], g["rho_old"], phi, g["boundary_phi"],
                              D, bD, Su, Sp, 1.0 / self.dt, wc=wc, bwc=bwc, ref=self.ref, dc=dc, bdc=bdc)
        return o, g, (Su, Sp, D, bD)

    def device(self, eqn):
        m = self.m
        self.ctx.assemble(eqn)
        size = {"lower": m.n_faces, "upper": m.n_faces, "diag": m.n_cells, "source": m.n_cells,
                "internal_coeffs": m.n_boundary_slots, "boundary_coeffs": m.n_boundary_slots}
        return {p: self.ctx.get_matrix(eqn, p, size[p]) for p in PARTS}


@pytest.fixture(scope="module", params=list(R.MESHES))
def rc(request):
    c = Case(request.param, schemes={"laplacian": "corrected"} if request.param == "sheared-walls" else None)
    yield c
    c.ctx.close()


# ------------------------------------------------------------------------------------------------ 1. homogeneous decay
@pytest.mark.parametrize("name,small,coef", [("periodic-even", 1, None), ("periodic-even", 0, NONDEFAULT), ("periodic-odd", 1, NONDEFAULT),
                                             ("periodic-odd", 0, None), ("walls", 1, None), ("walls", 0, NONDEFAULT)])
def test_homogeneous_decay(name, small, coef):
    import unstructured_meshes as um
    from dfmi import case
    c = Case(name, small=small, coef=coef)
    ctx, m, t = c.ctx, c.m, c.t
    try:
        f = um.uniform_fields(m, _species(c))
        case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"])
        ctx.call("pre_time_step")
        _tight(ctx)
        k0, e0 = 0.37, 2.1e3
        c.set_ke(np.full(m.n_cells, k0), np.full(m.n_cells, e0))
        ctx.turbulence_correct()
        e1, k1, n1 = R.decay(k0, e0, c.dt, c.q)
        got = {n: c.get(n) for n in ("epsilon", "k", "nut", "G", "divU")}
        errs = {"epsilon": np.abs(got["epsilon"] / e1 - 1).max(), "k": np.abs(got["k"] / k1 - 1).max(),
                "nut": np.abs(got["nut"] / n1 - 1).max()}
        print(name, small, {n: f"{v:.2e}" for n, v in errs.items()}, ctx.solver_stats("epsilon"), ctx.solver_stats("k"))
        assert not got["G"].any() and not got["divU"].any()
        for n, v in errs.items():
            assert v <= 1e-12, (n, v)
        assert abs(k1 / k0 - 1) > 1e-4 and abs(e1 / e0 - 1) > 1e-3        # the step moved both
    finally:
        ctx.close()


def _species(c):
    from dfmi.mech import read_yaml_mechanism
    import os
    from conftest import GOLDEN
    return read_yaml_mechanism(os.path.join(GOLDEN, "Burke2012_s9r23.yaml"))["species"]


# ------------------------------------------------------------------------------------------------ 2. production
def test_production_against_long_double(rc):
    c, m = rc, rc.m
    st = R.ras_state(m)
    c.push(st)
    c.ctx.assemble("epsilon")
    G, dv, nut = c.get("G"), c.get("divU"), c.get("nut")
    assert np.array_equal(nut, R.nut_of(c.q["Cmu"], st["k"], st["epsilon"]))       # validate(): Cmu k^2 / eps bitwise
    st = dict(st, nut=nut)
    eG, eD = R.production_error(m, st, G, dv, c.pt["U"], c.pt["rho"])
    bounds = R.load_bounds()
    bG, bD = R.gpu_bound(bounds, c.name, "G"), R.gpu_bound(bounds, c.name, "divU")
    print(f"{c.name}: G err {eG.max():.3e} (bound {bG:.1e}), divU err {eD.max():.3e} (bound {bD:.1e})")
    assert eG.max() <= bG and eD.max() <= bD
    assert dv.min() < 0 < dv.max() and np.abs(G).max() > 0
    c.ctx.assemble("epsilon")                                                       # two runs bitwise
    assert np.array_equal(c.get("G"), G) and np.array_equal(c.get("divU"), dv)


@pytest.fixture(scope="module")
def linear_case():
    from test_gpu_turbulence import _walls
    m = R.get_mesh("walls")
    ctx, _, t, st, pt, inert, dt = _case(periodic=False, walls=_walls(all_fixed_U=True), mech="burke9", mesh=m)
    yield ctx, m, st, dt, pt
    ctx.close()


@pytest.mark.parametrize("cls", ["zero", "shear", "dilatation+", "dilatation-", "general"])
def test_production_of_linear_velocity_fields(linear_case, cls):
    """exact face values of a linear field: G = 0 exactly for zero, nut gamma^2 for shear; divU = +-3a for the dilatations,
    whose SuSp term is implicit for + (in diag) and explicit for - (in source). Every state, the general tensor with its
    nine distinct components included, is also held per cell to the long-double restatement: G and divU at the 1e-13 floor
    of nut |g|^2 and of sum |phi_f / rho_f| / V (the walled box's measured fp64 error is 4e-16, so the floor decides)"""
    from dfmi import case
    from les_reference import LINEAR_G
    ctx, m, st, dt, pt = linear_case
    C_, B = m.n_cells, m.n_boundary_slots
    G9 = LINEAR_G[cls]
    _, _, _, _, bfc = m.boundary_arrays()
    U = (m.cell_centres @ G9).T.copy()
    bU = ((m.cell_centres[bfc] + m.boundary_delta()) @ G9).T.copy()
    rho0 = 1.2
    w = m.weight
    Uf = w * (U[:, m.owner] - U[:, m.neighbour]) + U[:, m.neighbour]
    bsf = m.boundary_arrays()[0]
    ctx.set_option("ras.model", 1)
    for n, v in (("U", U), ("boundary_U", bU), ("rho", np.full(C_, rho0)), ("boundary_rho", np.full(B, rho0)),
                 ("rho_old", np.full(C_, rho0)), ("phi", rho0 * (Uf * np.asarray(m.sf).T).sum(axis=0)),
                 ("boundary_phi", rho0 * (bU * np.asarray(bsf).T).sum(axis=0))):
        ctx.set_field(n, np.ascontiguousarray(v))
    zg = m.patch_types(0)
    ctx.set_patch_types("k", zg); ctx.set_patch_types("epsilon", zg)
    k0, e0 = np.full(C_, 0.3), np.full(C_, 2e3)
    for n, v in (("k", k0), ("epsilon", e0), ("boundary_k", np.full(B, 0.3)), ("boundary_epsilon", np.full(B, 2e3))):
        ctx.set_field(n, v)
    q = R.DEFAULTS
    lin = {"U": U, "boundary_U": bU, "rho": np.full(C_, rho0), "boundary_rho": np.full(B, rho0),
           "phi": rho0 * (Uf * np.asarray(m.sf).T).sum(axis=0), "boundary_phi": rho0 * (bU * np.asarray(bsf).T).sum(axis=0)}
    for eqn, keq in (("epsilon", 0), ("k", 1)):
        ctx.assemble(eqn)
        G, dv, nut = (ctx.get_field(n, (C_,)) for n in ("G", "divU", "nut"))
        gn2 = (G9 * G9).sum()
        eG, eD = R.production_error(m, dict(lin, nut=nut), G, dv, pt["U"], pt["rho"])
        print(f"linear {cls} {eqn}: G err {eG.max():.3e}, divU err {eD.max():.3e} (bound 1.0e-13)")
        assert eG.max() <= 1e-13 and eD.max() <= 1e-13, (cls, eG.max(), eD.max())
        if cls == "zero":
            assert not G.any() and not dv.any()
        elif cls == "shear":
            assert np.abs(G / (nut * 1900.0 ** 2) - 1).max() <= 1e-11 and np.abs(dv).max() <= 1e-11 * 1900.0
        elif cls.startswith("dilatation"):
            a = 1300.0 if cls.endswith("+") else -1300.0
            assert np.abs(dv / (3 * a) - 1).max() <= 1e-11 and np.abs(G).max() <= 1e-11 * nut.max() * gn2
            Su, Sp = R.sources(keq, q, G, dv, np.full(C_, rho0), k0, e0)
            psi = k0 if keq else e0
            diag, src = ctx.get_matrix(eqn, "diag", C_), ctx.get_matrix(eqn, "source", C_)
            plain = (1.0 / dt) * rho0 * psi * m.volume                  # ddt's source alone
            coef = (2 / 3 * q["C1"] - q["C3"]) if not keq else 2 / 3
            if a > 0:    # implicit: Sp carries a, the source only ddt (+ the rounding-level production)
                assert np.all(Sp > (q["C2"] if not keq else 1.0) * rho0 * e0 / k0)
                assert np.abs(src / plain - 1).max() <= 1e-9
            else:        # explicit: Su = -min(a, 0) psi > 0 in the source, Sp the destruction alone
                assert np.abs(Sp / ((q["C2"] if not keq else 1.0) * rho0 * e0 / k0) - 1).max() <= 1e-12
                want = plain + m.volume * (-(coef * rho0 * 3 * a) * psi)
                assert np.abs(src / want - 1).max() <= 1e-9
            assert np.array_equal(src, (1.0 / dt) * rho0 * psi * m.volume + m.volume * Su)
        else:
            assert G.min() > 0 and np.abs(dv / np.trace(G9) - 1).max() <= 1e-10
    ctx.set_option("ras.model", 0)


# ------------------------------------------------------------------------------------------------ 3. matrices
def _oracle_grad(c, v, bv):
    """the oracle's Gauss gradient [3, C] (sequential order: bitwise k_grad_cells)"""
    import oracle as O
    m = c.m
    if not hasattr(c, "_orc"):
        c._orc = O.Oracle(m, c.t, {k: x.copy() for k, x in c.st.items()}, c.pt, c.inert, 1.0 / c.dt)
    o = c._orc
    o._i("ptype_ras", c.k_pt)
    o._d("ras_v", v); o._d("ras_bv", bv)
    g = o.out("ras_g", 3 * m.n_cells)
    o._run("orc_grad_scalar", b"ras_v", b"ras_bv", b"ptype_ras", b"ras_g", None)
    return g.reshape(3, m.n_cells).copy()


def _check_matrices(c, scheme):
    m, ctx = c.m, c.ctx
    corrected = c.name == "sheared-walls"
    dc = bdc = None
    if corrected:
        dc, _, bdc, _ = m.nonorth_geometry()
    for t in ("div(phi,k)", "div(phi,epsilon)"):
        ctx.set_scheme(t, scheme)
    out = {}
    for eqn, keq in (("epsilon", 0), ("k", 1)):
        dev = c.device(eqn)
        wc = bwc = None
        if scheme != "upwind":
            v, bv = c.get(eqn), c.get("boundary_" + eqn)
            wc, bwc = R.limited_weights(c.tp, c.k_pt, 1.0, ctx.get_field("phi", (m.n_faces,)), c.get("boundary_phi"), v, bv,
                                        _oracle_grad(c, v, bv))
        ref, g, (Su, Sp, D, bD) = c.restated(keq, wc, bwc, dc, bdc)
        for p in PARTS:
            if corrected and p == "source":
                continue
            assert ulp_diff(dev[p], ref[p]) == 0, (c.name, scheme, eqn, p, rel_err(dev[p], ref[p]))
        assert np.abs(ref["lower"]).max() > 0 or m.n_faces == 0
        if corrected:   # the explicit term at the non-orthogonal suite's own bound form
            acc, _, _, sc = NR.corrected_term(m, c.k_pt, g[eqn][None], g["boundary_" + eqn][None], D[None])
            accL, _, _, _ = NR.corrected_term(m, c.k_pt, g[eqn][None], g["boundary_" + eqn][None], D[None], T=NR.LD)
            bound = NR.gpu_bound(NR.load_bounds(), "sheared-walls", "he")
            err = np.abs((dev["source"] - ref["source"]) - np.asarray(accL[0], np.float64))
            # the difference of two sources carries the sources' own rounding: eps |source| on top of the term's scale
            tol = bound * np.asarray(sc[0], np.float64) + 4 * np.finfo(float).eps * np.abs(ref["source"])
            print(f"corrected {eqn}: max err / tol {np.max(err / tol):.3e}, term max {np.abs(acc).max():.3e}")
            assert np.all(err <= tol) and np.abs(acc).max() > 0
        out[eqn] = dev
    for t in ("div(phi,k)", "div(phi,epsilon)"):
        ctx.set_scheme(t, "upwind")
    return out


def test_matrices_bitwise_with_device_production(rc):
    c = rc
    c.push(R.ras_state(c.m))
    up = _check_matrices(c, "upwind")
    ll = _check_matrices(c, "limitedLinear 1")
    if c.m.n_faces > 300:
        assert ulp_diff(up["k"]["lower"], ll["k"]["lower"]) > 0                    # the limiter is in the matrix
    # one generic kernel for both equations: with sigmak = sigmaEps the off-diagonals coincide bitwise, else they differ
    assert ulp_diff(up["k"]["lower"], up["epsilon"]["lower"]) > 0
    c.ctx.set_option("ras.sigmak", c.q["sigmaEps"])
    try:
        a, b = c.device("epsilon"), c.device("k")
        for p in ("lower", "upper"):
            assert np.array_equal(a[p], b[p]), p
        assert ulp_diff(a["diag"], b["diag"]) > 0
    finally:
        c.ctx.set_option("ras.sigmak", c.q["sigmak"])


def test_matrices_bitwise_open_outlet():
    """fixedValue / zeroGradient / inletOutlet patches on the parity suite's mixed case: the TGV flow crosses the outlet
    both ways"""
    c = Case("walls", walls="mixed")
    try:
        m = c.m
        rng = np.random.default_rng(41)
        k = 0.3 * (1 + 0.5 * rng.uniform(-1, 1, m.n_cells))
        eps = 2e3 * (1 + 0.5 * rng.uniform(-1, 1, m.n_cells))
        from dfmi import case
        bk, beps = case.boundary_values(m, k).reshape(-1), case.boundary_values(m, eps).reshape(-1)
        off = 0
        for p in m.patches:
            if p.name == "left":
                bk[off:off + p.size] = 0.25; beps[off:off + p.size] = 1.5e3
            if p.name == "right":
                c.ref[off:off + p.size] = 0.2
                bphi = c.ctx.get_field("boundary_phi", (m.n_boundary_slots,))[off:off + p.size]
                assert bphi.min() < 0 < bphi.max()
            off += p.slots
        c.ctx.set_field("boundary_k_ref", c.ref); c.ctx.set_field("boundary_epsilon_ref", c.ref)
        c.set_ke(k, eps, bk, beps)
        _check_matrices(c, "upwind")
        _check_matrices(c, "limitedLinear 1")
    finally:
        c.ctx.close()


# ------------------------------------------------------------------------------------------------ 4. bound()
@pytest.mark.parametrize("name", ["walls", "periodic-even", "refined"])
def test_bound_against_restatement(name):
    c = Case(name)
    ctx, m = c.ctx, c.m
    try:
        st = R.ras_state(m)
        c.push(st)
        _tight(ctx)
        ctx.set_delta_t(1e-12)           # tiny: the solves keep the seeded values
        c.dt = 1e-12
        k, eps = st["k"].copy(), st["epsilon"].copy()
        wall = int(m.patches[0].face_cells[0]) if m.patches[0].kind == "wall" else 0
        a, b = int(m.owner[m.n_faces // 2]), int(m.neighbour[m.n_faces // 2])
        iso = [c_ for c_ in (17, 63, 101) if c_ not in (wall, a, b)]
        eps[iso[0]] = -7.0; eps[iso[1]] = -1e-3; eps[wall] = -3.0; eps[a] = -1.0; eps[b] = -2.0
        k[iso[2]] = -0.2; k[a] = -0.1; k[b] = -0.05; k[wall] = 1e-20
        ctx.set_option("ras.kMin", 1e-9)
        c.set_ke(k, eps)
        ctx.turbulence_correct()
        for nm, lo in (("epsilon", 1e-15), ("k", 1e-9)):
            pre, bpre = c.get(nm + "_prebound"), c.get("boundary_" + nm + "_prebound")
            assert (pre < lo).sum() >= 3, (nm, "the solve kept the seeds below the bound")
            want, bwant = R.bound(c.tp, c.k_pt, pre, bpre, lo)
            got, bgot = c.get(nm), c.get("boundary_" + nm)
            e = np.abs(got - want).max() / np.abs(want).max()
            print(name, nm, f"bound err {e:.2e}; raised cells {(got != pre).sum()}")
            assert np.abs(got / want - 1).max() <= 1e-13 and got.min() >= lo
            assert np.array_equal(bgot, bwant)
            assert np.array_equal(got[pre >= lo], pre[pre >= lo])            # bounded cells bitwise untouched
        # a state that is positive everywhere comes out bitwise its solved field
        ctx.set_option("ras.kMin", 1e-15)
        c.set_ke(st["k"], st["epsilon"])
        ctx.turbulence_correct()
        for nm in ("epsilon", "k"):
            assert np.array_equal(c.get(nm), c.get(nm + "_prebound")), nm
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. full step
def _fields(ctx, m, t):
    out = {n: ctx.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he")}
    out["U"] = ctx.get_field("U", (3, m.n_cells)); out["Y"] = ctx.get_field("Y", (t.S, m.n_cells))
    out["phi"] = ctx.get_field("phi", (m.n_faces,))
    return out


@pytest.mark.parametrize("name", ["periodic-even", "walls"])
def test_full_steps_match_ras_oracle(name):
    from dfmi import case
    c = Case(name, coef={"Prt": 0.85, "Sct": 0.7})
    lam = _case(periodic=False, mech="burke9", mesh=c.m)
    ctx, m, t = c.ctx, c.m, c.t
    try:
        B = m.n_boundary_slots
        state = {k: v.copy() for k, v in c.st.items()}
        # laminar before: this context (RAS off) against a context that never saw the option
        for x in (ctx, lam[0]):
            x.set_option("amg.reuse_steps", 1)
        ctx.set_option("ras.model", 0)
        case.push_state(ctx, state); ctx.time_step(2)
        case.push_state(lam[0], state); lam[0].time_step(2)
        want = _fields(lam[0], m, t)
        got = _fields(ctx, m, t)
        for n in want:
            assert np.array_equal(got[n], want[n]), ("laminar before", n)
        # RAS steps against the oracle
        ctx.set_option("ras.model", 1)
        _tight(ctx)
        case.push_state(ctx, state)
        rng = np.random.default_rng(43)
        k = 30.0 * (1 + 0.5 * rng.uniform(-1, 1, m.n_cells))
        eps = 4e5 * (1 + 0.5 * rng.uniform(-1, 1, m.n_cells))
        bk, beps = c.set_ke(k, eps)
        o = R.RasOracle(m, t, {k_: v.copy() for k_, v in state.items()}, dict(c.pt), c.inert, 1.0 / c.dt, c.q, k, eps, bk, beps)
        for step in (1, 2):
            o.time_step(2)
            ctx.time_step(2)
            for n, tl in {"T": 1e-10, "p": 1e-10, "rho": 1e-10, "he": 1e-10}.items():
                e = rel_err(ctx.get_field(n, (m.n_cells,)), o[n])
                print(name, step, n, f"{e:.2e}")
                assert e < tl, (step, n, e)
            for n, shp in (("U", (3, m.n_cells)), ("Y", (t.S, m.n_cells)), ("phi", (m.n_faces,)), ("k", (m.n_cells,)),
                           ("epsilon", (m.n_cells,)), ("nut", (m.n_cells,)), ("boundary_nut", (B,))):
                e = rel_err(ctx.get_field(n, shp), o[n])
                print(name, step, n, f"{e:.2e}")
                assert e < 1e-9, (step, n, e)
        assert rel_err(ctx.get_field("U", (3, m.n_cells)), want["U"]) > 1e-6     # turbulent differs from laminar
        print("iterations", ctx.solver_stats("epsilon"), ctx.solver_stats("k"))
        # laminar after: bitwise what it was
        ctx.set_option("ras.model", 0)
        for e in ("U", "Y", "E"):
            ctx.set_solver(e, 20, 1e-5)
        ctx.set_solver("p", 1000, 1e-5)
        case.push_state(ctx, state); ctx.time_step(2)
        got = _fields(ctx, m, t)
        for n in want:
            assert np.array_equal(got[n], want[n]), ("laminar after", n)
    finally:
        ctx.close(); lam[0].close()


def test_les_step_bitwise_before_and_after_ras():
    """an LES context that goes through a RAS episode (les.model 1 -> ras.model 1 -> les.model 1) steps bitwise as an
    LES context that never saw a ras.* option: the turbulent flag, the Prt / Sct choice and the validity rule are shared"""
    from dfmi import case, turbulence as T
    c = Case("periodic-even", coef={"Prt": 0.6, "Sct": 0.5})
    twin = _case(periodic=False, mech="burke9", mesh=c.m)
    ctx, m, t = c.ctx, c.m, c.t
    try:
        state = {k: v.copy() for k, v in c.st.items()}
        les = dict(T.DEFAULTS, model=1, Prt=0.85, Sct=0.7, deltaCoeff=1.0)

        def les_step(x):
            case.push_state(x, state)
            T.apply(x, m, les)
            x.time_step(2)
            out = _fields(x, m, t)
            out["nut"] = x.get_field("nut", (m.n_cells,))
            out["boundary_nut"] = x.get_field("boundary_nut", (m.n_boundary_slots,))
            return out
        ctx.set_option("ras.model", 0)
        for x in (ctx, twin[0]):
            x.set_option("amg.reuse_steps", 1)
        before, want = les_step(ctx), les_step(twin[0])
        for n in want:
            assert np.array_equal(before[n], want[n]), ("LES before", n)
        assert want["nut"].max() > 0
        # the RAS episode on this context
        ctx.set_option("les.model", 0)
        ctx.set_option("ras.model", 1)
        case.push_state(ctx, state)
        c.set_ke(np.full(m.n_cells, 30.0), np.full(m.n_cells, 4e5))
        ctx.time_step(2)
        assert rel_err(ctx.get_field("nut", (m.n_cells,)), want["nut"]) > 1e-3
        ctx.set_option("ras.model", 0)
        after, want2 = les_step(ctx), les_step(twin[0])
        for n in want:
            assert np.array_equal(want2[n], want[n]), ("twin repeat", n)
            assert np.array_equal(after[n], want[n]), ("LES after", n)
    finally:
        ctx.close(); twin[0].close()


# ------------------------------------------------------------------------------------------------ 6. validity and options
def test_validity_and_options():
    from dfmi.lib import DfmiError, renumber_cells
    c = Case("walls")
    ctx, m = c.ctx, c.m
    try:
        for key, bad in (("ras.model", 2), ("ras.model", -1), ("ras.model", 0.5), ("ras.Cmu", 0.0), ("ras.C1", -1.0),
                         ("ras.C2", float("nan")), ("ras.C3", float("inf")), ("ras.C3", float("nan")), ("ras.sigmak", 0.0),
                         ("ras.sigmaEps", float("inf")), ("ras.kMin", 0.0), ("ras.epsilonMin", -1.0), ("ras.Prt", 0.0),
                         ("ras.Sct", float("nan")), ("ras.nope", 1.0)):
            with pytest.raises(DfmiError):
                ctx.set_option(key, bad)
        ctx.set_option("ras.C3", -0.5); ctx.set_option("ras.C3", 0.0)            # any finite value
        with pytest.raises(DfmiError, match="les.model.*ras.model|ras.model.*les.model"):
            ctx.set_option("les.model", 1)
        with pytest.raises(DfmiError):
            ctx.set_option("les.model", 3)                                         # stays refused
        for n in ("G", "divU", "k_prebound"):
            with pytest.raises(DfmiError, match=n):
                ctx.set_field(n, np.zeros(m.n_cells))
        with pytest.raises(DfmiError, match="'k'"):                               # never set: named
            ctx.turbulence_correct()
        ctx.set_field("k", np.full(m.n_cells, 0.3))
        with pytest.raises(DfmiError, match="'epsilon'"):
            ctx.turbulence_correct()
        st = R.ras_state(m)
        c.push(st)
        ctx.call("U_process")                                                      # validate(): k_ras_nut only
        nut = c.get("nut")
        assert np.array_equal(nut, R.nut_of(c.q["Cmu"], st["k"], st["epsilon"]))
        assert np.array_equal(c.get("k"), st["k"]) and np.array_equal(c.get("epsilon"), st["epsilon"])
        ctx.set_field("k", 2.0 * st["k"])                                         # writing k invalidates nut
        ctx.kernel_timer("k_ras_nut,k_scalar_assemble")
        ctx.call("E_process")
        assert ctx.kernel_time("k_ras_nut")[1] == 2 and ctx.kernel_time("k_scalar_assemble")[1] == 0
        ctx.kernel_timer("")
        assert np.array_equal(c.get("nut"), R.nut_of(c.q["Cmu"], 2.0 * st["k"], st["epsilon"]))
        assert np.array_equal(c.get("k"), 2.0 * st["k"])
        # so does writing epsilon, a boundary counterpart or a coefficient: validate re-forms nut, never the equations
        B = m.n_boundary_slots
        cur = {"k": 2.0 * st["k"], "epsilon": st["epsilon"], "boundary_k": st["boundary_k"],
               "boundary_epsilon": st["boundary_epsilon"]}
        Cmu = c.q["Cmu"]
        for what, val in (("epsilon", 1.5 * st["epsilon"]), ("boundary_k", 3.0 * st["boundary_k"]),
                          ("boundary_epsilon", 0.5 * st["boundary_epsilon"]), ("ras.Cmu", 0.1), ("ras.C1", 1.5)):
            if what.startswith("ras."):
                ctx.set_option(what, val)
                Cmu = val if what == "ras.Cmu" else Cmu
            else:
                cur[what] = val
                ctx.set_field(what, np.ascontiguousarray(val))
            ctx.kernel_timer("k_ras_nut,k_scalar_assemble")
            ctx.call("U_process")
            assert ctx.kernel_time("k_ras_nut")[1] == 2 and ctx.kernel_time("k_scalar_assemble")[1] == 0, what
            ctx.kernel_timer("")
            assert np.array_equal(c.get("nut"), R.nut_of(Cmu, cur["k"], cur["epsilon"])), what
            # nut's patch types are "calculated" here: every wall slot is Cmu boundary_k^2 / boundary_epsilon
            assert np.array_equal(c.get("boundary_nut"), R.nut_of(Cmu, cur["boundary_k"], cur["boundary_epsilon"])), what
            for n in ("k", "epsilon"):
                assert np.array_equal(c.get(n), cur[n]), (what, n)
            ctx.kernel_timer("k_ras_nut")
            ctx.call("U_process")                                                  # valid again: nothing re-formed
            assert ctx.kernel_time("k_ras_nut")[1] == 0, what
            ctx.kernel_timer("")
        ctx.set_option("ras.Cmu", c.q["Cmu"]); ctx.set_option("ras.C1", c.q["C1"])
        # two runs and a traversal order are bitwise
        res = []
        order = renumber_cells(m.n_cells, m.cell_centres, m.owner, m.neighbour, "morton")
        for trav in (None, None, order):
            c.push(st)
            ctx.set_traversal(trav)
            ctx.turbulence_correct()
            res.append({n: c.get(n) for n in ("k", "epsilon", "nut", "G", "divU", "boundary_nut")})
        ctx.set_traversal(None)
        for r in res[1:]:
            for n, v in res[0].items():
                assert np.array_equal(r[n], v), n
        assert ulp_diff(res[0]["k"], st["k"]) > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 7. two ranks
_HUB = [900]


@pytest.mark.parametrize("name", ["sheared-walls", "refined"])
def test_two_ranks_bound_across_the_cut(name):
    """bound() with negative cells on both sides of a processor face: a coupled slot counts as the face it is, so two
    ranks raise those cells to what the single domain raises them to (one dfmi_turbulence_correct at a tiny time step)"""
    from dfmi import case
    from dfmi.lib import Context
    from dfmi.partition import partition_cells, decompose
    from test_gpu_parity import _mech
    mg = R.get_mesh(name)
    ym, t = _mech("burke9")
    inert = ym["species"].index("N2")
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    part = np.asarray(partition_cells(mg, 2, "graph"))
    cut = np.nonzero(part[mg.owner] != part[mg.neighbour])[0]
    assert cut.size > 2
    a, b = int(mg.owner[cut[cut.size // 2]]), int(mg.neighbour[cut[cut.size // 2]])
    rng = np.random.default_rng(53)
    k = 30.0 * (1 + 0.5 * rng.uniform(-1, 1, mg.n_cells))
    eps = 4e5 * (1 + 0.5 * rng.uniform(-1, 1, mg.n_cells))
    eps[a], eps[b], k[a], k[b] = -1e5, -2e5, -3.0, -1.0

    def run(m, g, comm=None):
        c = Context(0)
        try:
            case.setup_context(c, m, t, inert, 1e-6, case.default_patch_types(m), comm=comm)
            for e in ("k", "epsilon"):
                c.set_solver(e, 300, 1e-15, 1e-300)
            zg = m.patch_types(0)
            c.set_patch_types("k", zg); c.set_patch_types("epsilon", zg)
            c.set_option("ras.model", 1)
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            c.call("pre_time_step")
            c.set_delta_t(1e-12)
            for n, v in (("k", k[g]), ("epsilon", eps[g])):
                c.set_field(n, np.ascontiguousarray(v))
                c.set_field("boundary_" + n, case.boundary_values(m, v).reshape(-1))
            c.turbulence_correct()
            return {n: c.get_field(n, (m.n_cells,)) for n in ("k", "epsilon", "nut", "k_prebound", "epsilon_prebound")}
        finally:
            c.close()

    ref = run(mg, np.arange(mg.n_cells))
    assert ref["epsilon_prebound"][a] < 0 and ref["epsilon_prebound"][b] < 0 and ref["k_prebound"][a] < 0
    assert ref["epsilon"][a] > 0 and ref["epsilon"][b] > 0 and ref["k"].min() > 0
    meshes = decompose(mg, part)
    nr = len(meshes)
    out, err = [None] * nr, [None] * nr
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            out[r] = run(meshes[r], meshes[r].cell_map, comm={"hub": hub, "nranks": nr, "rank": r})
        except Exception as e:   # surfaced below
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
    for n in ("k", "epsilon", "nut"):
        got = np.zeros(mg.n_cells)
        for r in range(nr):
            got[meshes[r].cell_map] = out[r][n]
        e = np.abs(got / ref[n] - 1).max()
        print(name, "bound across the cut", n, f"{e:.2e}", "raised to", got[a], got[b])
        assert e < 1e-9, (n, e)


@pytest.mark.parametrize("name", ["sheared-walls", "refined"])
def test_two_ranks_match_single_domain(name):
    from dfmi import case
    from dfmi.lib import Context
    from dfmi.partition import partition_cells, decompose
    from test_gpu_parity import _mech
    mg = R.get_mesh(name)
    ym, t = _mech("burke9")
    dt = 1e-6
    inert = ym["species"].index("N2")
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    rng = np.random.default_rng(47)
    k = 30.0 * (1 + 0.5 * rng.uniform(-1, 1, mg.n_cells))
    eps = 4e5 * (1 + 0.5 * rng.uniform(-1, 1, mg.n_cells))
    schemes = {"div(phi,k)": "limitedLinear 1"}
    if name == "sheared-walls":
        schemes["laplacian"] = "corrected"

    def run(m, g, comm=None):
        c = Context(0)
        try:
            case.setup_context(c, m, t, inert, dt, case.default_patch_types(m), comm=comm, schemes=schemes)
            for e in ("U", "Y", "E", "k", "epsilon"):
                c.set_solver(e, 300, 1e-14, 1e-300)
            c.set_solver("p", 3000, 1e-14, 1e-300)
            zg = m.patch_types(0)
            c.set_patch_types("k", zg); c.set_patch_types("epsilon", zg)
            c.set_option("ras.Prt", 0.85); c.set_option("ras.Sct", 0.7)
            c.set_option("ras.model", 1)
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            for n, v in (("k", k[g]), ("epsilon", eps[g])):
                c.set_field(n, np.ascontiguousarray(v))
                c.set_field("boundary_" + n, case.boundary_values(m, v).reshape(-1))
            c.call("pre_time_step")
            c.time_step(2)
            o = {n: c.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he", "k", "epsilon", "nut")}
            o["U"] = c.get_field("U", (3, m.n_cells))
            o["Y"] = c.get_field("Y", (t.S, m.n_cells))
            # phi and boundary_nut per cell (the decomposition carries a cell map, no face or slot map): the sum of the
            # outward fluxes and of their magnitudes over the cell's internal faces and primary slots (a processor face is
            # an internal face of the single domain), and the sum of boundary_nut over its physical (non-processor) slots
            phi, bphi = c.get_field("phi", (m.n_faces,)), c.get_field("boundary_phi", (m.n_boundary_slots,))
            bnut = c.get_field("boundary_nut", (m.n_boundary_slots,))
            sl = NR.Slots(m)
            div, mag, sn = np.zeros(m.n_cells), np.zeros(m.n_cells), np.zeros(m.n_cells)
            np.add.at(div, m.owner, phi); np.add.at(div, m.neighbour, -phi)
            np.add.at(mag, m.owner, np.abs(phi)); np.add.at(mag, m.neighbour, np.abs(phi))
            np.add.at(div, sl.cell[sl.prim], bphi[sl.prim]); np.add.at(mag, sl.cell[sl.prim], np.abs(bphi[sl.prim]))
            phys = sl.prim & ~sl.coupled
            np.add.at(sn, sl.cell[phys], bnut[phys])
            o["div_phi"], o["mag_phi"], o["sum_boundary_nut"] = div, mag, sn
            return o
        finally:
            c.close()

    ref = run(mg, np.arange(mg.n_cells))
    meshes = decompose(mg, partition_cells(mg, 2, "graph"))
    nr = len(meshes)
    out, err = [None] * nr, [None] * nr
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            out[r] = run(meshes[r], meshes[r].cell_map, comm={"hub": hub, "nranks": nr, "rank": r})
        except Exception as e:   # surfaced below
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
    for n, kk in (("T", 1), ("p", 1), ("rho", 1), ("he", 1), ("k", 1), ("epsilon", 1), ("nut", 1), ("U", 3), ("Y", t.S)):
        a = np.zeros((kk, mg.n_cells))
        for r in range(nr):
            a[:, meshes[r].cell_map] = out[r][n].reshape(kk, -1)
        e = rel_err(a, ref[n].reshape(kk, -1))
        print(name, "two ranks vs single domain", n, f"{e:.2e}")
        assert e < 1e-9, (n, e)
    assert rel_err(ref["k"], k) > 1e-6
    got = {n: np.zeros(mg.n_cells) for n in ("div_phi", "mag_phi", "sum_boundary_nut")}
    for r in range(nr):
        for n in got:
            got[n][meshes[r].cell_map] = out[r][n]
    e_mag = rel_err(got["mag_phi"], ref["mag_phi"])
    e_div = np.abs(got["div_phi"] - ref["div_phi"]).max() / ref["mag_phi"].max()
    e_bn = rel_err(got["sum_boundary_nut"], ref["sum_boundary_nut"])
    print(name, f"two ranks vs single domain phi: sum |phi| per cell {e_mag:.2e}, div phi {e_div:.2e}; boundary_nut {e_bn:.2e}")
    assert e_mag < 1e-9 and e_div < 1e-9 and e_bn < 1e-9
    assert ref["sum_boundary_nut"].max() > 0
