"""LES eddy viscosity on the device (MI355X): Smagorinsky and WALE in the U, Y and E equations (include/dfmi.h
dfmi_turbulence_correct).

nut is held pointwise to the long-double restatement (tests/les_reference.py) on the oracle's grad(U), at 4x the fp64
restatement's measured error floored at 1e-13 (tests/golden/les_nut_bounds.json -- never a number read off the kernel);
with the device's own nut injected, the three assemblies equal the oracle bit for bit; an LES step launches no YEqn
preparation kernel; full steps, one and two ranks, agree with LesOracle at test_full_outer_iteration's bounds; and
les.model = 0 leaves the laminar step bitwise what it was. Cases: the 6 x 5 x 4 boxes of test_gpu_parity._case, the
TGV velocity with seeded noise of a few per cent so that tr D takes both signs.
"""
import os
import threading

import numpy as np
import pytest

import les_reference as R
from conftest import GOLDEN, rel_err, ulp_diff
from test_gpu_parity import _case, _cmp_matrix, _ell_width

pytestmark = pytest.mark.gpu

NAMES = {1: "Smagorinsky", 2: "WALE"}
CASE_SCHEMES = {"div(phi,Yi_h)": "limitedLinear01 1", "div(phi,K)": "limitedLinear 1", "div(hDiffCorrFlux)": "cubic"}
PARTS = ["lower", "upper", "diag", "source", "internal_coeffs", "boundary_coeffs"]


def _walls(mixed=False, all_fixed_U=False):
    from dfmi.mesh import FIXED_VALUE, FIXED_ENERGY, GRADIENT_ENERGY, INLET_OUTLET, WAVE_TRANSMISSIVE

    def walls(m):
        fv = {}
        names = ("left",) if mixed else ("left", "right")
        fixed = [i for i, p in enumerate(m.patches) if p.name in names]
        for f in ("U", "T", "Y"):
            t = m.patch_types(0).copy()
            t[fixed] = FIXED_VALUE
            fv[f] = t
        if all_fixed_U:
            fv["U"] = m.patch_types(FIXED_VALUE).copy()
        t = m.patch_types(GRADIENT_ENERGY).copy()
        t[fixed] = FIXED_ENERGY
        fv["he"] = t
        if mixed:
            out = [i for i, p in enumerate(m.patches) if p.name == "right"]
            fv["U"][out] = INLET_OUTLET
            fv["Y"][out] = INLET_OUTLET
            fv["p"] = m.patch_types(0).copy()
            fv["p"][out] = WAVE_TRANSMISSIVE
        return fv
    return walls


def _nut_patches(m):
    """nut's patch types and stored boundary values: fixedValue on "left" (a non-uniform stored value), zeroGradient on
    "right", calculated (stored 0) on the other walls; coupled patches keep their kind"""
    from dfmi.mesh import CALCULATED, FIXED_VALUE, ZERO_GRADIENT
    pt = m.patch_types(CALCULATED).copy()
    bnut = np.zeros(m.n_boundary_slots)
    off = 0
    for i, p in enumerate(m.patches):
        if p.kind == "wall" and p.name == "left":
            pt[i] = FIXED_VALUE
            bnut[off:off + p.size] = 1e-5 * (1.0 + 0.1 * np.arange(p.size))
        elif p.kind == "wall" and p.name == "right":
            pt[i] = ZERO_GRADIENT
        off += p.slots
    return pt, bnut


class Case:
    def __init__(self, param, mesh=None):
        from dfmi import case, lib, turbulence as T
        self.param = param
        generic = param.endswith("-generic")
        schemes = param.endswith("-schemes")
        base = param.replace("-generic", "").replace("-schemes", "")
        if generic:
            lib.DEFAULT_OPTIONS["fv.species_generic"] = 1
        try:
            mech = "gri53" if base.startswith("gri53") else ("es80" if base == "es80" else "burke9")
            kind = {"es80": "periodic", "burke9": "periodic", "gri53": "periodic", "gri53-walls": "walls"}.get(base, base)
            self.schemes = CASE_SCHEMES if schemes else None
            if kind == "periodic":
                r = _case(mech=mech, schemes=self.schemes)
            else:
                r = _case(periodic=False, walls=_walls(mixed=kind == "mixed"), mech=mech, distorted=kind == "distorted",
                          mixed=kind == "mixed", schemes=self.schemes, mesh=mesh)
        finally:
            lib.DEFAULT_OPTIONS.pop("fv.species_generic", None)
        self.ctx, self.m, self.t, st, self.pt, self.inert, self.dt = r
        m, ctx = self.m, self.ctx
        st = dict(st)
        st["U"] = st["U"] + 0.03 * 4.0 * np.random.default_rng(19).standard_normal(st["U"].shape)
        case.push_state(ctx, st)
        ctx.correct_boundary("U")
        st["boundary_U"] = ctx.get_field("boundary_U", (3, m.n_boundary_slots))
        self.nut_pt, self.bnut = _nut_patches(m)
        st["boundary_nut"] = self.bnut
        self.st = st
        # non-default Prt / Sct ride on the cases that also carry the case schemes
        self.prt, self.sct = (0.85, 0.7) if schemes else (1.0, 1.0)
        self.delta = T.cube_root_vol_delta(m)
        ctx.set_patch_types("nut", self.nut_pt)
        ctx.set_field("delta", self.delta)
        self._grad = None

    def les(self, model):
        from dfmi import turbulence as T
        return dict(T.DEFAULTS, model=model, Prt=self.prt, Sct=self.sct)

    def select(self, model):
        """state restored, the model in force, nut formed: (nut, boundary_nut)"""
        from dfmi import case, turbulence as T
        case.push_state(self.ctx, self.st)
        T.apply(self.ctx, self.m, dict(self.les(model), deltaCoeff=1.0))
        self.ctx.turbulence_correct()
        return (self.ctx.get_field("nut", (self.m.n_cells,)), self.ctx.get_field("boundary_nut", (self.m.n_boundary_slots,)))

    def oracle(self, model, nut=None, bnut=None):
        o = R.LesOracle(self.m, self.t, {k: v.copy() for k, v in self.st.items() if k != "boundary_nut"}, self.pt,
                        self.inert, 1.0 / self.dt, self.les(model), self.delta, schemes=self.schemes,
                        nut_ptypes=self.nut_pt, boundary_nut=self.bnut.copy())
        if nut is not None:
            o.set_nut(nut, bnut)
        return o

    def grad_u(self):
        """the oracle's out_gradU [9, C] of the case's U (computed once)"""
        if self._grad is None:
            import oracle as O
            o = O.Oracle(self.m, self.t, {k: v.copy() for k, v in self.st.items() if k != "boundary_nut"}, self.pt,
                         self.inert, 1.0 / self.dt)
            self._grad = o.u_assemble()["gradU"].reshape(9, self.m.n_cells).copy()
        return self._grad


PARAMS = ["es80", "burke9", "walls", "distorted", "mixed", "burke9-generic", "walls-generic", "gri53", "gri53-walls",
          "burke9-schemes", "walls-schemes"]


@pytest.fixture(scope="module", params=PARAMS)
def lc(request):
    c = Case(request.param)
    yield c
    c.ctx.close()


def _expected_boundary_nut(c, nut):
    """nut.correctBoundaryConditions(): zeroGradient the cell value, fixedValue / calculated the stored value, cyclic
    w nut_c + (1 - w) nut_partner"""
    from dfmi import case
    from dfmi.mesh import CALCULATED, FIXED_VALUE
    b = case.boundary_values(c.m, nut)
    off = 0
    for i, p in enumerate(c.m.patches):
        if c.nut_pt[i] in (FIXED_VALUE, CALCULATED):
            b[off:off + p.size] = c.bnut[off:off + p.size]
        off += p.slots
    return b


# ------------------------------------------------------------------------------------------------ 1. nut pointwise
def test_nut_pointwise_random_states(lc):
    from dfmi.lib import renumber_cells
    c, ctx, m = lc, lc.ctx, lc.m
    bounds = R.load_bounds()
    g = c.grad_u()
    tr = g[0] + g[4] + g[8]
    assert tr.min() < 0 < tr.max()
    for model, name in NAMES.items():
        nut, bnut = c.select(model)
        err = R.nut_error(nut, g, c.delta, model, c.les(model))
        bound = R.gpu_bound(bounds, name, "random")
        print(f"{c.param} {name}: max |dnut| / (delta^2 |g|) = {err.max():.3e} (bound {bound:.1e}), nut max {nut.max():.3e}")
        assert err.max() <= bound, (name, err.max())                 # every cell
        assert nut.min() >= 0 and nut.max() > 0
        assert ulp_diff(bnut, _expected_boundary_nut(c, nut)) == 0
        ctx.turbulence_correct()                                      # bitwise repeatable
        assert np.array_equal(ctx.get_field("nut", (m.n_cells,)), nut)
        assert np.array_equal(ctx.get_field("boundary_nut", (m.n_boundary_slots,)), bnut)
        # the same nut by the CSR walk, without the computed hex walk, and in a cache-blocked traversal
        key = np.stack(m.local_index, axis=1).astype(np.float64) if hasattr(m, "local_index") else m.cell_centres
        order = renumber_cells(m.n_cells, key, m.owner, m.neighbour, "bricks" if hasattr(m, "local_index") else "morton")
        for opt, val in (("fv.csr_walk", 1), ("fv.hex_walk", 0), ("trav", order)):
            if opt == "trav":
                ctx.set_traversal(val)
            else:
                ctx.set_option(opt, val)
            try:
                ctx.turbulence_correct()
                assert np.array_equal(ctx.get_field("nut", (m.n_cells,)), nut), opt
            finally:
                if opt == "trav":
                    ctx.set_traversal(None)
                else:
                    ctx.set_option(opt, 1 - val)


@pytest.fixture(scope="module")
def linear_case():
    """a walled box with fixedValue U on all six sides: a linear velocity field with its exact face values makes the
    Gauss gradient G in every cell"""
    ctx, m, t, st, pt, inert, dt = _case(periodic=False, walls=_walls(all_fixed_U=True), mech="burke9")
    from dfmi import turbulence as T
    delta = T.cube_root_vol_delta(m)
    ctx.set_field("delta", delta)
    yield ctx, m, t, st, pt, inert, dt, delta
    ctx.close()


@pytest.mark.parametrize("cls", ["zero", "rotation", "shear", "dilatation+", "dilatation-", "general"])
def test_nut_linear_velocity_fields(linear_case, cls):
    """every cell is one chosen state: G = 0 gives exactly 0; pure shear is WALE's zero (g . g = 0: zero to rounding);
    uniform dilatation of either sign is the Smagorinsky -b + sqrt(b^2 + 4ac) cancellation. Solid rotation is not a
    zero of WALE (dev(Omega . Omega) != 0), so there it is held to the reference like every other state."""
    import oracle as O
    ctx, m, t, st, pt, inert, dt, delta = linear_case
    bounds = R.load_bounds()
    G = R.LINEAR_G[cls]
    _, _, _, _, bfc = m.boundary_arrays()
    st2 = dict(st)
    st2["U"] = (m.cell_centres @ G).T.copy()
    st2["boundary_U"] = ((m.cell_centres[bfc] + m.boundary_delta()) @ G).T.copy()
    ctx.set_field("U", st2["U"]); ctx.set_field("boundary_U", st2["boundary_U"])
    g = O.Oracle(m, t, {k: v.copy() for k, v in st2.items()}, pt, inert, 1.0 / dt).u_assemble()["gradU"].reshape(9, m.n_cells)
    scale = max(np.abs(G).max(), 1e-300)
    assert np.abs(g - G.reshape(9, 1)).max() <= 1e-11 * scale          # the Gauss gradient of a linear field is exact
    gnorm = np.sqrt((g * g).sum(axis=0))
    for model, name in NAMES.items():
        ctx.set_option("les.model", model)
        ctx.turbulence_correct()
        nut = ctx.get_field("nut", (m.n_cells,))
        err = R.nut_error(nut, g, delta, model)
        bound = R.gpu_bound(bounds, name, cls)
        print(f"{cls} {name}: max err {err.max():.3e} (bound {bound:.1e}); nut / (delta^2 |g|) max "
              f"{(nut / np.maximum(delta ** 2 * gnorm, 1e-300)).max():.3e}")
        assert err.max() <= bound, (name, cls, err.max())              # no cell excluded
        if cls == "zero":
            assert not nut.any()
        elif cls == "shear" and model == 2:
            assert (nut / (delta ** 2 * gnorm)).max() <= 1e-13
        elif cls == "general" or (cls, model) in (("shear", 1), ("dilatation-", 1), ("rotation", 2)):
            assert nut.min() > 0          # (Smagorinsky has no strain to act on in a rotation, WALE none in a dilatation)
        ctx.turbulence_correct()
        assert np.array_equal(ctx.get_field("nut", (m.n_cells,)), nut)
    ctx.set_option("les.model", 0)


# ------------------------------------------------------------------------------------------------ 2. assembly bitwise
def test_assembly_bitwise_with_device_nut(lc):
    from dfmi.mesh import GRADIENT_ENERGY
    c, ctx, m, t = lc, lc.ctx, lc.m, lc.t
    B, C_, F = m.n_boundary_slots, m.n_cells, m.n_faces
    for model in NAMES:
        nut, bnut = c.select(model)
        assert ctx.get_option("les.Prt") == c.prt and ctx.get_option("les.Sct") == c.sct
        # U
        o = c.oracle(model, nut, bnut)
        ref = o.u_assemble()
        ctx.assemble("U")
        res = _cmp_matrix(ctx, "U", ref, PARTS + ["source_solve"], B)
        assert not {k: v for k, v in res.items() if v[0] != 0}, (model, res)
        assert ulp_diff(ctx.get_field("rAU", (C_,)), o["rAU"]) == 0
        assert np.abs(ref["diag"]).max() > 0
        # Y (LDU) and the dropped fields
        o.y_prep()
        ref = o.y_assemble()
        ctx.assemble("Y")
        res = _cmp_matrix(ctx, "Y", ref, PARTS, B)
        assert not {k: v for k, v in res.items() if v[0] != 0}, (model, res)
        for name, shp in (("sumYDiffError", (3, C_)), ("hDiffCorrFlux", (3, C_)), ("diffAlphaD", (C_,)), ("phiUc", (F,)),
                          ("boundary_phiUc", (B,)), ("boundary_hDiffCorrFlux", (3, B))):
            assert not ctx.get_field(name, shp).any(), name
        # Y in the solver's rows: the production kernel against the LDU assembly folded by the generic gather
        W, n = _ell_width(m), t.S - 1
        ctx.assemble("Y_ell")
        got = {p: ctx.get_solver_rows("Y", p, n * (W if p == "val" else 1) * C_) for p in ("val", "dS", "rhs")}
        ctx.assemble("Y_ell_ref")
        for p in ("val", "dS", "rhs"):
            r = ctx.get_solver_rows("Y", p, got[p].size)
            assert ulp_diff(got[p], r) == 0, (model, p)
            assert np.abs(r).max() > 0, p
        # E, species on gradientEnergy walls off their cell values (test_e_eqn_assembly_bitwise)
        bY = c.st["boundary_Y"].copy()
        ge = np.repeat(np.asarray(c.pt["he"]), [p.slots for p in m.patches]) == GRADIENT_ENERGY
        bY[:, ge] *= 1.0 + 1e-2 * np.random.default_rng(3).standard_normal((t.S, int(ge.sum())))
        ctx.set_field("boundary_Y", bY)
        o = c.oracle(model, nut, bnut)
        o.set("boundary_Y", bY)
        o.y_prep()
        o.energy_gradient()
        o.correct_bc("he", "he", 1)
        ref = o.e_assemble()
        ctx.assemble("Y")
        ctx.assemble("E")
        res = _cmp_matrix(ctx, "E", ref, PARTS, B)
        assert not {k: v for k, v in res.items() if v[0] != 0}, (model, res)
    # the eddy viscosity is in the matrices: the laminar oracle's differ
    import oracle as O
    lam = O.Oracle(m, t, {k: v.copy() for k, v in c.st.items() if k != "boundary_nut"}, c.pt, c.inert, 1.0 / c.dt,
                   schemes=c.schemes).u_assemble()
    assert ulp_diff(lam["diag"], c.oracle(2, nut, bnut).u_assemble()["diag"]) > 0


# ------------------------------------------------------------------------------------------------ 3. dropped work
def _tight(ctx):
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 200, 1e-15, 1e-300)
    ctx.set_solver("p", 2000, 1e-15, 1e-300)


def _loose(ctx):
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 20, 1e-5)
    ctx.set_solver("p", 1000, 1e-5)


@pytest.mark.parametrize("param", ["burke9", "gri53"])
def test_les_step_launches_no_y_prep(param):
    c = Case(param)
    ctx, m = c.ctx, c.m
    try:
        c.select(1)
        ctx.kernel_timer("k_y_prep,k_y_prep_gen,k_les_nut")
        ctx.time_step(2)
        assert ctx.kernel_time("k_y_prep")[1] == 0 and ctx.kernel_time("k_y_prep_gen")[1] == 0
        assert ctx.kernel_time("k_les_nut")[1] == 1                      # the end-of-step update (nut was valid)
        for name, shp in (("phiUc", (m.n_faces,)), ("diffAlphaD", (m.n_cells,)), ("hDiffCorrFlux", (3, m.n_cells)),
                          ("sumYDiffError", (3, m.n_cells))):
            assert not ctx.get_field(name, shp).any(), name
        # the timer names are the ones a laminar step launches under
        ctx.set_option("les.model", 0)
        ctx.kernel_timer("k_y_prep,k_y_prep_gen,k_les_nut")
        ctx.time_step(2)
        assert ctx.kernel_time("k_y_prep")[1] + ctx.kernel_time("k_y_prep_gen")[1] >= 1
        assert ctx.kernel_time("k_les_nut")[1] == 0
        ctx.kernel_timer("")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. full step
def _compare_step(ctx, o, m, t, what, first):
    # the first step at test_full_outer_iteration's own per-field bounds; a step run from it at 1e-9 per component
    for n, tl in {"T": 1e-10, "p": 1e-11, "rho": 1e-10, "he": 1e-10}.items():
        e = rel_err(ctx.get_field(n, (m.n_cells,)), o[n])
        print(what, n, f"{e:.2e}")
        assert e < (tl if first else 1e-9), (what, n, e)
    B = m.n_boundary_slots
    for n, shp in (("U", (3, m.n_cells)), ("Y", (t.S, m.n_cells)), ("phi", (m.n_faces,)), ("nut", (m.n_cells,)),
                   ("boundary_U", (3, B)), ("boundary_Y", (t.S, B)), ("boundary_p", (B,)), ("boundary_phi", (B,)),
                   ("boundary_nut", (B,))):
        e = rel_err(ctx.get_field(n, shp), o[n])
        assert e < 1e-9, (what, n, e)


def test_full_steps_match_les_oracle(lc):
    """two dfLowMachFoam outer iterations (nCorr = 2) against LesOracle with exact solves: the second step's UEqn
    reads the nut the first step ended with"""
    from dfmi.lib import DfmiError
    c, ctx, m, t = lc, lc.ctx, lc.m, lc.t
    both = c.param in ("burke9", "walls", "mixed", "burke9-schemes")
    models = (1, 2) if both else ((1,) if PARAMS.index(c.param) % 2 else (2,))
    _tight(ctx)
    try:
        for model in models:
            nut0, _ = c.select(model)
            o = c.oracle(model)
            assert rel_err(nut0, o["nut"]) < 1e-12
            for step in (1, 2):
                o.time_step(2)
                ctx.time_step(2)
                _compare_step(ctx, o, m, t, (c.param, NAMES[model], step), step == 1)
            assert rel_err(o["nut"], nut0) > 1e-6                       # the field moved, and nut with it
            nut = ctx.get_field("nut", (m.n_cells,))
            bnut = ctx.get_field("boundary_nut", (m.n_boundary_slots,))
            ctx.turbulence_correct()                                     # right after a step: bitwise unchanged
            assert np.array_equal(ctx.get_field("nut", (m.n_cells,)), nut)
            assert np.array_equal(ctx.get_field("boundary_nut", (m.n_boundary_slots,)), bnut)
            ctx.call("U_process")                                        # valid: the per-equation entry runs
            ctx.set_field("U", ctx.get_field("U", (3, m.n_cells)))       # writing U invalidates nut
            with pytest.raises(DfmiError, match="nut is not valid"):
                ctx.call("U_process")
            with pytest.raises(DfmiError, match="nut is not valid"):
                ctx.assemble("Y")
            ctx.turbulence_correct()
            ctx.call("U_process")
    finally:
        _loose(ctx)


# ------------------------------------------------------------------------------------------------ 5. two ranks
_HUB = [700]


@pytest.mark.parametrize("model", [1, 2], ids=["Smagorinsky", "WALE"])
def test_two_ranks_match_undecomposed_les_oracle(model):
    """in-process transport, an 8 x 6 x 4 periodic box cut in x: boundary_nut's neighbour half crosses the processor
    patches through the halo"""
    from dfmi import case, turbulence as T
    from dfmi.lib import Context
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi.mesh import global_cell_ids, hex_box
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
    L, dt, dims = (2 * np.pi * 1e-3,) * 3, 1e-6, (8, 6, 4)
    inert = ym["species"].index("N2")
    les = dict(T.DEFAULTS, model=model, Prt=0.85, Sct=0.7)
    mg = hex_box(*dims, lengths=L, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3)
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    f["U"] = f["U"] + 0.03 * 4.0 * np.random.default_rng(23).standard_normal(f["U"].shape)

    def setup(m, comm=None):
        ctx = Context(0)
        case.setup_context(ctx, m, t, inert, dt, case.default_patch_types(m), comm=comm, turbulence=les)
        for e in ("U", "Y", "E"):
            ctx.set_solver(e, 300, 1e-14, 1e-300)
        ctx.set_solver("p", 3000, 1e-14, 1e-300)
        return ctx

    ctx = setup(mg)
    case.init_state(ctx, mg, t.S, f["T"], f["p"], f["U"], f["Y"])
    ctx.call("pre_time_step")
    st = case.pull_state(ctx, mg, t.S)
    ctx.close()
    o = R.LesOracle(mg, t, st, case.default_patch_types(mg), inert, 1.0 / dt, les, T.cube_root_vol_delta(mg))
    o.time_step(2)

    meshes = [hex_box(*dims, lengths=L, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3, decomp=(2, 1, 1), rank=r) for r in range(2)]
    gids = [global_cell_ids(mm, dims[0], dims[1]) for mm in meshes]
    out, err = [None, None], [None, None]
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            m, g = meshes[r], gids[r]
            c = setup(m, comm={"hub": hub, "nranks": 2, "rank": r})
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            c.call("pre_time_step")
            c.time_step(2)                                               # nut not valid: formed first thing
            res = {n: c.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he", "nut")}
            res["U"] = c.get_field("U", (3, m.n_cells)); res["Y"] = c.get_field("Y", (t.S, m.n_cells))
            out[r] = res
            c.close()
        except Exception as e:   # surfaced below
            err[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    assert not any(x.is_alive() for x in th), "decomposed run hung"
    for e in err:
        if e is not None:
            raise e
    for n in ("T", "p", "rho", "he", "nut", "U", "Y"):
        k = out[0][n].shape[0] if out[0][n].ndim == 2 else 0
        a = np.zeros((k, mg.n_cells)) if k else np.zeros(mg.n_cells)
        for r in range(2):
            a[..., gids[r]] = out[r][n]
        e = rel_err(a, o[n])
        assert e < 1e-9, (n, e)
    assert o["nut"].max() > 0


# ------------------------------------------------------------------------------------------------ 6. laminar untouched
def test_laminar_step_bitwise_after_les_and_refusals():
    from dfmi import case
    from dfmi.lib import DfmiError
    names = (("T", None), ("p", None), ("rho", None), ("he", None), ("U", 3), ("Y", "S"), ("phi", "F"), ("rAU", None),
             ("diffAlphaD", None), ("hDiffCorrFlux", 3), ("phiUc", "F"))

    def fields(ctx, m, t):
        out = {}
        for n, k in names:
            shp = (m.n_faces,) if k == "F" else (m.n_cells,) if k is None else ((t.S if k == "S" else k), m.n_cells)
            out[n] = ctx.get_field(n, shp)
        return out

    c = Case("burke9-schemes")
    fresh = _case(mech="burke9", schemes=CASE_SCHEMES)
    try:
        ctx, m, t = c.ctx, c.m, c.t
        for key, bad in (("les.model", 3), ("les.model", -1), ("les.model", 1.5), ("les.Ck", 0.0), ("les.Ce", -2.0),
                         ("les.Cw", float("nan")), ("les.Prt", float("inf")), ("les.Sct", 0.0), ("les.Cs", 0.1)):
            with pytest.raises(DfmiError):
                ctx.set_option(key, bad)
        with pytest.raises(DfmiError, match="nut"):
            ctx.set_field("nut", np.zeros(m.n_cells))
        assert ctx.get_option("les.model") == 0 and ctx.get_option("les.Ck") == 0.094
        state = {k: v for k, v in c.st.items() if k != "boundary_nut"}
        f = fresh[0]
        # what a context keeps across steps beside its fields is the pressure AMG: its aggregates are formed at the
        # first p solve (the same laminar step on both contexts here) and, with amg.reuse_steps = 1, its operators
        # at every step
        for x in (ctx, f):
            x.set_option("amg.reuse_steps", 1)
            case.push_state(x, state)
            x.time_step(2)
        c.select(1)
        ctx.time_step(2)                                                 # an LES step on this context
        assert ctx.get_field("nut", (m.n_cells,)).max() > 0
        case.push_state(ctx, state)
        ctx.set_option("les.model", 0)
        ctx.turbulence_correct()                                         # laminar: a successful no-op
        ctx.time_step(2)
        got = fields(ctx, m, t)
        case.push_state(f, state)
        f.time_step(2)
        want = fields(f, m, t)
        for n, _ in names:
            assert np.array_equal(got[n], want[n]), n
        assert np.abs(want["phiUc"]).max() > 0 and np.abs(want["diffAlphaD"]).max() > 0
    finally:
        ctx.close()
        fresh[0].close()
