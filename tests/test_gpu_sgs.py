"""The reference's own LES closures on the device (MI355X): Sigma (les.model = 4, k_les_sigma) and dynamicSmagorinsky
(les.model = 5, k_dyn_strain / k_dyn_filter / k_dyn_nut; include/dfmi.h dfmi_turbulence_correct).

Sigma: nut is held pointwise to the long-double restatement at 8 sweeps (tests/sgs_reference.py) on the oracle's
grad(U) -- bitwise the device's -- at 4x the fp64 restatement's measured error floored at 1e-13 of Csg^2 delta^2 |g|_F
(tests/golden/sgs_bounds.json: never a number read off the kernel). Linear velocity fields on the all-fixedValue box
put one chosen state in every cell: the model's zeros and the near-degenerate classes through random rotations.

dynamicSmagorinsky: les_LM and les_MM against the long-double restatement within 4x the fp64 restatement's own error
floored at 1e-13 of sgs_reference.dynamic_scales; les_Cs from the device's own LM and MM at 0 ulp; nut with the -nu
clip acting in some cells and not in others; Cs of both signs; the closed form of a linear velocity field in the
interior cells of a uniform 8^3 box.

Both: with the device's own nut injected the three assemblies equal the oracle bit for bit; full steps on one and two
ranks agree with the subclassed oracle at test_gpu_turbulence's bounds; laminar and Smagorinsky steps are bitwise what
they were, with the launches they had, after a model-4 or model-5 step on the same context; the refusals. Cases:
test_gpu_turbulence's 6 x 5 x 4 boxes and the 210 prisms of tests/unstructured_meshes.py.
"""
import os
import threading

import numpy as np
import pytest

import sgs_reference as R
import unstructured_meshes as um
from conftest import GOLDEN, rel_err, ulp_diff
from test_gpu_parity import _case, _cmp_matrix, _ell_width
from test_gpu_turbulence import (CASE_SCHEMES, PARTS, Case, _compare_step, _expected_boundary_nut, _loose, _nut_patches,
                                 _tight, _walls)

pytestmark = pytest.mark.gpu

SIGMA = R.SIGMA
DYN = R.DYNAMIC
MODEL_IDS = {SIGMA: "Sigma", DYN: "dynamicSmagorinsky"}
BOTH = pytest.mark.parametrize("model", [SIGMA, DYN], ids=["Sigma", "dynamicSmagorinsky"])
CSG = 1.35                        # off the default, so that the option is seen to arrive


class SCase(Case):
    """test_gpu_turbulence's Case with the Sigma / dynamicSmagorinsky settings and oracles; "prisms": the 210
    triangular prisms with the parity walls (the CSR walk of another width)"""

    def __init__(self, param):
        if param != "prisms":
            super().__init__(param)
            return
        from dfmi import case, turbulence as T
        self.param, self.schemes = param, None
        r = _case(periodic=False, walls=lambda mm: um.wall_types(mm, False), mech="burke9", mesh=um.get("prisms", "small"))
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
        self.prt, self.sct = 1.0, 1.0
        self.delta = T.cube_root_vol_delta(m)
        ctx.set_patch_types("nut", self.nut_pt)
        ctx.set_field("delta", self.delta)
        self._grad = None

    def les(self, model=SIGMA):
        from dfmi import turbulence as T
        return dict(T.DEFAULTS, model=model, Prt=self.prt, Sct=self.sct, Csg=CSG)

    def oracle(self, model=SIGMA, nut=None, bnut=None):
        if model not in (SIGMA, DYN):
            return super().oracle(model, nut, bnut)
        cls = R.SigmaOracle if model == SIGMA else R.DynamicOracle
        state = {k: v.copy() for k, v in self.st.items() if k != "boundary_nut"}
        o = cls(self.m, self.t, state, self.pt, self.inert, 1.0 / self.dt, self.les(model), self.delta,
                schemes=self.schemes, nut_ptypes=self.nut_pt, boundary_nut=self.bnut.copy())
        if nut is not None:
            o.set_nut(nut, bnut)
        return o


PARAMS = ["burke9", "walls", "distorted", "mixed", "walls-generic", "burke9-schemes", "prisms"]


@pytest.fixture(scope="module", params=PARAMS)
def sc(request):
    c = SCase(request.param)
    yield c
    c.ctx.close()


# ------------------------------------------------------------------------------------------------ 1. nut pointwise
def test_sigma_pointwise_random_states(sc):
    from dfmi.lib import renumber_cells
    c, ctx, m = sc, sc.ctx, sc.m
    bound = R.gpu_bound(R.load_bounds(), "random")
    g = c.grad_u()
    nut, bnut = c.select(SIGMA)
    assert ctx.get_option("les.model") == SIGMA and ctx.get_option("les.Csg") == CSG
    err = R.nut_error(nut, g, c.delta, CSG)
    print(f"{c.param} Sigma: max |dnut| / (Csg^2 delta^2 |g|) = {err.max():.3e} (bound {bound:.1e}), nut max {nut.max():.3e}")
    assert err.max() <= bound, err.max()                                # every cell
    assert nut.min() >= 0 and nut.max() > 0
    # the option is in the result: the restatement at this Csg, and the default Csg gives (1.5 / 1.35)^2 of it
    assert rel_err(R.nut_from_grad(g, c.delta, CSG), nut) < 1e-12
    ctx.set_option("les.Csg", 1.5)
    ctx.turbulence_correct()
    assert rel_err(ctx.get_field("nut", (m.n_cells,)), (1.5 / CSG) ** 2 * nut) < 1e-14
    ctx.set_option("les.Csg", CSG)
    ctx.turbulence_correct()
    assert np.array_equal(ctx.get_field("nut", (m.n_cells,)), nut)
    assert ulp_diff(bnut, _expected_boundary_nut(c, nut)) == 0
    ctx.kernel_timer("k_les_sigma,k_les_nut")
    ctx.turbulence_correct()                                             # bitwise repeatable, by the kernel of its own
    assert ctx.kernel_time("k_les_sigma")[1] == 1 and ctx.kernel_time("k_les_nut")[1] == 0
    ctx.kernel_timer("")
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
    ctx.set_option("les.model", SIGMA)
    yield ctx, m, t, st, pt, inert, dt, delta
    ctx.close()


def _linear_states(cls):
    """the tensors G [k, 3, 3] of a class: the chosen one, or three random rotations of the near-degenerate diag(s)"""
    if cls in R.L.LINEAR_G:
        return R.L.LINEAR_G[cls][None]
    return R.degenerate_tensors(cls, 3, seed=29)


@pytest.mark.parametrize("cls", ["zero", "shear", "rotation", "dilatation+", "dilatation-", "general"] + list(R.DEGENERATE))
def test_sigma_linear_velocity_fields(linear_case, cls):
    """every cell is one chosen state, one state per launch. G = 0 and rank-1 shear rotate nothing: exactly 0. Solid
    rotation (s1 = s2, s3 = 0) and isotropic dilatation (s1 = s2 = s3) are zeros of the model: at most the floor. The
    near-degenerate classes (two singular values 1e-9 apart, s3 = 1e-9 s1 or 0) are held to the truth like every other
    state: this is where a closed form from the invariants would be seven digits off."""
    import oracle as O
    ctx, m, t, st, pt, inert, dt, delta = linear_case
    bound = R.gpu_bound(R.load_bounds(), cls)
    _, _, _, _, bfc = m.boundary_arrays()
    for G in _linear_states(cls):
        st2 = dict(st)
        st2["U"] = (m.cell_centres @ G).T.copy()
        st2["boundary_U"] = ((m.cell_centres[bfc] + m.boundary_delta()) @ G).T.copy()
        ctx.set_field("U", st2["U"]); ctx.set_field("boundary_U", st2["boundary_U"])
        g = O.Oracle(m, t, {k: v.copy() for k, v in st2.items()}, pt, inert, 1.0 / dt).u_assemble()["gradU"].reshape(9, m.n_cells)
        assert np.abs(g - G.reshape(9, 1)).max() <= 1e-11 * max(np.abs(G).max(), 1e-300)   # the Gauss gradient of a linear field
        gnorm = np.sqrt((g * g).sum(axis=0))
        ctx.turbulence_correct()
        nut = ctx.get_field("nut", (m.n_cells,))
        err = R.nut_error(nut, g, delta)
        rel = nut / np.maximum(1.5 ** 2 * delta ** 2 * gnorm, 1e-300)
        print(f"{cls}: max err {err.max():.3e} (bound {bound:.1e}); nut / (Csg^2 delta^2 |g|) in [{rel.min():.3e}, {rel.max():.3e}]")
        assert err.max() <= bound, (cls, err.max())                      # no cell excluded
        assert nut.min() >= 0
        if cls == "zero":
            assert not nut.any()
        elif cls in ("shear", "rotation", "dilatation+", "dilatation-"):
            assert rel.max() <= 1e-13
        elif cls in ("general", "s3e-5"):
            assert nut.min() > 0
        ctx.turbulence_correct()
        assert np.array_equal(ctx.get_field("nut", (m.n_cells,)), nut)


# ------------------------------------------------------------------------------------------------ 2. assembly bitwise
@BOTH
def test_assembly_bitwise_with_device_nut(sc, model):
    from dfmi.mesh import GRADIENT_ENERGY
    c, ctx, m, t = sc, sc.ctx, sc.m, sc.t
    B, C_ = m.n_boundary_slots, m.n_cells
    nut, bnut = c.select(model)
    if model == DYN:
        assert nut.min() < 0 < nut.max()                                 # backscatter: the assemblies see both signs
    o = c.oracle(model, nut, bnut)
    ref = o.u_assemble()
    ctx.assemble("U")
    res = _cmp_matrix(ctx, "U", ref, PARTS + ["source_solve"], B)
    assert not {k: v for k, v in res.items() if v[0] != 0}, res
    assert ulp_diff(ctx.get_field("rAU", (C_,)), o["rAU"]) == 0
    o.y_prep()
    ref = o.y_assemble()
    ctx.assemble("Y")
    res = _cmp_matrix(ctx, "Y", ref, PARTS, B)
    assert not {k: v for k, v in res.items() if v[0] != 0}, res
    for name, shp in (("sumYDiffError", (3, C_)), ("hDiffCorrFlux", (3, C_)), ("diffAlphaD", (C_,)), ("phiUc", (m.n_faces,))):
        assert not ctx.get_field(name, shp).any(), name
    W, n = _ell_width(m), t.S - 1
    ctx.assemble("Y_ell")
    got = {p: ctx.get_solver_rows("Y", p, n * (W if p == "val" else 1) * C_) for p in ("val", "dS", "rhs")}
    ctx.assemble("Y_ell_ref")
    for p in ("val", "dS", "rhs"):
        assert ulp_diff(got[p], ctx.get_solver_rows("Y", p, got[p].size)) == 0, p
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
    assert not {k: v for k, v in res.items() if v[0] != 0}, res
    # this model's nut is in the matrices: WALE's differ
    wale = c.select(2)
    assert ulp_diff(c.oracle(2, *wale).u_assemble()["diag"], c.oracle(model, nut, bnut).u_assemble()["diag"]) > 0


# ------------------------------------------------------------------------------------------------ 3. full steps
@BOTH
def test_full_steps_match_sgs_oracle(sc, model):
    from dfmi.lib import DfmiError
    c, ctx, m, t = sc, sc.ctx, sc.m, sc.t
    kern = "k_les_sigma" if model == SIGMA else "k_dyn_nut"
    _tight(ctx)
    try:
        nut0, _ = c.select(model)
        o = c.oracle(model)
        assert rel_err(nut0, o["nut"]) < 1e-12
        ctx.kernel_timer(kern + ",k_les_nut,k_y_prep,k_y_prep_gen")
        for step in (1, 2):
            o.time_step(2)
            ctx.time_step(2)
            _compare_step(ctx, o, m, t, (c.param, MODEL_IDS[model], step), step == 1)
        assert ctx.kernel_time(kern)[1] == 2 and ctx.kernel_time("k_les_nut")[1] == 0
        assert ctx.kernel_time("k_y_prep")[1] == 0 and ctx.kernel_time("k_y_prep_gen")[1] == 0
        ctx.kernel_timer("")
        assert rel_err(o["nut"], nut0) > 1e-6                           # the field moved, and nut with it
        ctx.set_field("U", ctx.get_field("U", (3, m.n_cells)))           # writing U invalidates nut
        with pytest.raises(DfmiError, match="nut is not valid"):
            ctx.call("U_process")
        ctx.turbulence_correct()
        ctx.call("U_process")
        if model == SIGMA:
            ctx.set_option("les.Csg", 1.5)                               # so does the coefficient
            with pytest.raises(DfmiError, match="nut is not valid"):
                ctx.assemble("Y")
    finally:
        _loose(ctx)


# ------------------------------------------------------------------------------------------------ 4. two ranks
@BOTH
def test_two_ranks_match_undecomposed_sgs_oracle(model):
    """S, the two contractions and nut cross the processor patches through the halo; in-process transport, an 8 x 6 x 4 periodic box cut in x, against the undecomposed oracle to 1e-9"""
    from dfmi import case, turbulence as T
    from dfmi.lib import Context
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi.mesh import global_cell_ids, hex_box
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
    L, dt, dims = (2 * np.pi * 1e-3,) * 3, 1e-6, (8, 6, 4)
    inert = ym["species"].index("N2")
    les = dict(T.DEFAULTS, model=model, Prt=0.85, Sct=0.7, Csg=CSG)
    mg = hex_box(*dims, lengths=L, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3)
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    f["U"] = f["U"] + 0.03 * 4.0 * np.random.default_rng(23).standard_normal(f["U"].shape)

    def setup(m, comm=None):
        ctx = Context(0)
        case.setup_context(ctx, m, t, inert, dt, case.default_patch_types(m), comm=comm, turbulence=les)
        assert ctx.get_option("les.model") == model and (model == DYN or ctx.get_option("les.Csg") == CSG)
        for e in ("U", "Y", "E"):
            ctx.set_solver(e, 300, 1e-14, 1e-300)
        ctx.set_solver("p", 3000, 1e-14, 1e-300)
        return ctx

    ctx = setup(mg)
    case.init_state(ctx, mg, t.S, f["T"], f["p"], f["U"], f["Y"])
    ctx.call("pre_time_step")
    st = case.pull_state(ctx, mg, t.S)
    ctx.close()
    o = (R.SigmaOracle if model == SIGMA else R.DynamicOracle)(mg, t, st, case.default_patch_types(mg), inert, 1.0 / dt, les, T.cube_root_vol_delta(mg))
    o.time_step(2)

    meshes = [hex_box(*dims, lengths=L, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3, decomp=(2, 1, 1), rank=r) for r in range(2)]
    gids = [global_cell_ids(mm, dims[0], dims[1]) for mm in meshes]
    out, err = [None, None], [None, None]

    def work(r):
        try:
            m, g = meshes[r], gids[r]
            c = setup(m, comm={"hub": 2400 + model, "nranks": 2, "rank": r})
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
    assert o["nut"].max() > 0 and (model == SIGMA or o["nut"].min() < 0)


# ------------------------------------------------------------------------------------------------ 5. off is off
TIMED = "k_les_nut,k_les_sigma,k_dyn_strain,k_dyn_filter,k_dyn_nut,k_les_effective,k_u_grad,k_y_prep,k_u_assemble,k_e_assemble"


@BOTH
def test_laminar_and_smagorinsky_steps_bitwise_after_an_sgs_step(model):
    """a laminar and a Smagorinsky step, fields and launch counts, before and after a Sigma or dynamicSmagorinsky step
    on the same context"""
    sgs = model
    from dfmi import case
    names = (("T", None), ("p", None), ("rho", None), ("he", None), ("U", 3), ("Y", "S"), ("phi", "F"), ("rAU", None),
             ("diffAlphaD", None), ("hDiffCorrFlux", 3), ("phiUc", "F"))
    c = SCase("burke9-schemes")
    ctx, m, t = c.ctx, c.m, c.t
    state = {k: v for k, v in c.st.items() if k != "boundary_nut"}

    def step(model):
        """the state restored, `model` in force, one step: (fields, launches of the timed kernels)"""
        if model:
            c.select(model)
        else:
            case.push_state(ctx, state)
            ctx.set_option("les.model", 0)
        ctx.kernel_timer(TIMED)
        ctx.time_step(2)
        n = {k: ctx.kernel_time(k)[1] for k in TIMED.split(",")}
        ctx.kernel_timer("")
        out = {}
        for f, k in names:
            shp = (m.n_faces,) if k == "F" else (m.n_cells,) if k is None else ((t.S if k == "S" else k), m.n_cells)
            out[f] = ctx.get_field(f, shp)
        if model:
            out["nut"] = ctx.get_field("nut", (m.n_cells,))
        return out, n

    try:
        ctx.set_option("amg.reuse_steps", 1)       # the AMG's operators are formed at every step (test_gpu_turbulence)
        step(0)                                    # its aggregates at the first p solve
        before = {model: step(model) for model in (0, 1)}
        sig, n_sig = step(sgs)
        mine = {SIGMA: ("k_les_sigma",), DYN: ("k_dyn_strain", "k_dyn_filter", "k_dyn_nut")}[sgs]
        assert sig["nut"].max() > 0 and n_sig["k_les_nut"] == 0 and all(n_sig[k] == 1 for k in mine)   # the end-of-step update
        for model in (0, 1):
            got, n = step(model)
            want, n0 = before[model]
            assert n == n0, (model, n, n0)
            assert not any(n[k] for k in ("k_les_sigma", "k_dyn_strain", "k_dyn_filter", "k_dyn_nut")) and n["k_les_nut"] == (1 if model else 0)
            for f in want:
                assert np.array_equal(got[f], want[f]), (model, f)
        assert np.abs(before[0][0]["phiUc"]).max() > 0 and not np.array_equal(before[1][0]["nut"], sig["nut"])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
@BOTH
def test_sgs_options_and_refusals(model):
    from dfmi.lib import DfmiError
    c = SCase("burke9")
    ctx, m = c.ctx, c.m
    try:
        assert ctx.get_option("les.Csg") == 1.5
        for key, bad in (("les.model", 3), ("les.model", 6), ("les.model", 4.5), ("les.Csg", 0.0),
                         ("les.Csg", -1.5), ("les.Csg", float("nan")), ("les.Csg", float("inf")), ("les.Cs", 0.1)):
            with pytest.raises(DfmiError):
                ctx.set_option(key, bad)
        assert ctx.get_option("les.model") == 0 and ctx.get_option("les.Csg") == 1.5
        for n in ("les_Cs", "les_LM", "les_MM"):                          # nothing of model 5 exists before its first use
            with pytest.raises(DfmiError, match=n):
                ctx.get_field(n, (m.n_cells,))
            with pytest.raises(DfmiError, match=n):
                ctx.set_field(n, np.zeros(m.n_cells))
        ctx.set_option("les.model", model)
        with pytest.raises(DfmiError, match="les.model.*ras.model|ras.model.*les.model"):
            ctx.set_option("ras.model", 1)
        with pytest.raises(DfmiError, match="les.model.*tci.model|tci.model.*les.model"):
            ctx.set_option("tci.model", 1)
        with pytest.raises(DfmiError):
            ctx.set_option("fgm.model", 1)
        with pytest.raises(DfmiError, match="nut"):
            ctx.set_field("nut", np.zeros(m.n_cells))
        with pytest.raises(DfmiError, match="nut is not valid"):
            ctx.call("U_process")
        ctx.set_option("les.model", 0)
        ctx.set_option("ras.model", 1)
        with pytest.raises(DfmiError, match="les.model.*ras.model|ras.model.*les.model"):
            ctx.set_option("les.model", model)
        ctx.set_option("ras.model", 0)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 7. dynamicSmagorinsky
def _device_dynamic(ctx, m):
    return {n: ctx.get_field("les_" + n, (m.n_cells,)) for n in ("LM", "MM", "Cs")}


def test_dynamic_fields_random_states(sc):
    """les_LM and les_MM against the long-double restatement on the oracle's g within 4x the fp64 restatement's own
    error floored at 1e-13 of dynamic_scales; les_Cs from the device's own LM and MM at 0 ulp; nut from the device's
    Cs, with the -nu clip acting in some cells and not in others; Cs of both signs"""
    from dfmi.lib import renumber_cells
    c, ctx, m = sc, sc.ctx, sc.m
    bounds = R.load_bounds()
    g = c.grad_u()
    nut, bnut = c.select(DYN)
    d = _device_dynamic(ctx, m)
    mu, rho = ctx.get_field("mu", (m.n_cells,)), ctx.get_field("rho", (m.n_cells,))
    U, bU = c.st["U"], c.st["boundary_U"]
    truth = R.dynamic_model(m, c.pt["U"], U, bU, g, c.delta, mu, rho, R.LD)
    f64 = R.dynamic_model(m, c.pt["U"], U, bU, g, c.delta, mu, rho)
    scales = R.dynamic_scales(m, c.pt["U"], U, bU, f64["S"], f64["bS"], c.delta)
    eLM, eMM = R.dynamic_errors(d["LM"], d["MM"], truth, scales)
    bLM, bMM = R.gpu_bound_dynamic(bounds, "LM"), R.gpu_bound_dynamic(bounds, "MM")
    print(f"{c.param} dynamic: LM err {eLM:.3e} (bound {bLM:.1e}), MM err {eMM:.3e} (bound {bMM:.1e}); Cs in "
          f"[{d['Cs'].min():.3e}, {d['Cs'].max():.3e}]")
    assert eLM <= bLM and eMM <= bMM, (eLM, eMM)
    assert d["MM"].min() > 0
    assert ulp_diff(d["Cs"], 0.5 * d["LM"] / d["MM"]) == 0
    assert d["Cs"].min() < 0 < d["Cs"].max()                             # backscatter is the model
    assert rel_err(d["Cs"], np.asarray(truth["Cs"], dtype=np.float64)) < 1e-9
    # nut = max(Cs delta^2 |S|, -mu / rho): the clip exact where it acts, the rest to a few roundings
    floor = -mu / rho
    magS = np.sqrt(np.asarray(R._dd(f64["S"], f64["S"])))
    want = np.maximum(d["Cs"] * (c.delta * c.delta) * magS, floor)
    clipped = want == floor
    print(f"{c.param} dynamic: the -nu clip acts in {int(clipped.sum())} of {m.n_cells} cells; nut in [{nut.min():.3e}, {nut.max():.3e}]")
    assert 0 < clipped.sum() < m.n_cells
    assert np.array_equal(nut[clipped], floor[clipped])
    assert np.abs(nut - want).max() <= 1e-13 * np.abs(want).max()
    assert nut.min() < 0 < nut.max()
    assert ulp_diff(bnut, _expected_boundary_nut(c, nut)) == 0
    ctx.turbulence_correct()                                             # bitwise repeatable
    assert np.array_equal(ctx.get_field("nut", (m.n_cells,)), nut)
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
            d2 = _device_dynamic(ctx, m)
            assert all(np.array_equal(d2[n], d[n]) for n in d), opt
        finally:
            if opt == "trav":
                ctx.set_traversal(None)
            else:
                ctx.set_option(opt, 1 - val)


def test_dynamic_closed_form_in_interior_cells():
    """U = G^T x on a uniform 8^3 box with exact face values and delta = h: two or more cells away from the boundary
    Cs = -((G^T G) && S) / (36 |S|^3), independent of the restatement"""
    ctx, m, t, st, pt, inert, dt = _case(nx=8, ny=8, nz=8, periodic=False, walls=_walls(all_fixed_U=True), mech="burke9",
                                         gradings=(1.0, 1.0, 1.0))
    try:
        G = R.L.LINEAR_G["general"]
        h = np.cbrt(m.volume)
        assert np.ptp(h) <= 1e-12 * h.max()
        _, _, _, _, bfc = m.boundary_arrays()
        ctx.set_field("delta", h)
        ctx.set_field("U", (m.cell_centres @ G).T.copy())
        ctx.set_field("boundary_U", ((m.cell_centres[bfc] + m.boundary_delta()) @ G).T.copy())
        ctx.set_option("les.model", DYN)
        ctx.turbulence_correct()
        Cs = ctx.get_field("les_Cs", (m.n_cells,))
        S = 0.5 * (G + G.T) - np.trace(G) / 3.0 * np.eye(3)
        want = -((G.T @ G) * S).sum() / (36.0 * np.sqrt((S * S).sum()) ** 3)
        ijk = np.stack(m.local_index, axis=1)
        inner = np.all((ijk >= 2) & (ijk <= 5), axis=1)
        print(f"closed form {want!r}, device Cs in the {int(inner.sum())} interior cells [{Cs[inner].min()!r}, {Cs[inner].max()!r}]")
        # LL is a difference of terms (|U| / (h |G|))^2 ~ 1e2 times its size: 1e-16 x 1e2, with a margin of 1e2
        assert inner.sum() == 64 and np.abs(Cs[inner] - want).max() <= 1e-12 * abs(want)
        assert np.abs(Cs[~inner] - want).max() > 1e-6 * abs(want)        # the boundary values enter the outer two layers
    finally:
        ctx.close()
