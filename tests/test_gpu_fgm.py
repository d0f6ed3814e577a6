"""flareFGM on the device (MI355X): the retrieval kernels, the transport equations, dfmi_fgm_correct and the FGM time step
(include/dfmi.h, flareFGM block), held to the NumPy restatement tests/fgm_reference.py.

Retrieval: every table and state class on grids of 1, 255, 256, 257 and 4355 cells, cells and boundary slots, each call
twice. Every output made of + - * /, max, min, sqrt and table reads is bitwise the float64 restatement; chi_c inside the
flame (RANSsdrFLRmodel: pow, sqrt) is held per point to 4x the float64 restatement's measured error against long double,
floored at 1e-13 (tests/golden/fgm_point_bounds.json). The matrices of the transport equations at 0 ulp against
ras_reference.scalar_assemble; dfmi_fgm_correct, one full time step and two ranks against FgmOracle at 1e-9; every
refusal; fgm.model = 0 after 1 bitwise a context that never set it.
"""
import threading

import numpy as np
import pytest

import fgm_reference as FR
from conftest import rel_err, ulp_diff

pytestmark = pytest.mark.gpu

GRIDS = {1: (1, 1, 1), 255: (255, 1, 1), 256: (256, 1, 1), 257: (257, 1, 1), 4355: (5, 13, 67)}
OUT1 = ("chi_Z", "chi_Zc", "chi_c", "omega_c", "cOmega_c", "ZOmega_c", "Ha_s", "c_s", "Zvar_s", "cvar_s", "Zcvar_s", "Wt", "Cp",
        "Hf", "mu", "T", "psi", "rho", "rho_thermo")
SENTINEL = -777.0


def _mech():
    from test_gpu_parity import _mech as pm
    return pm("burke9")


def _bare_context(m, ras=True):
    """a context on mesh m with the burke9 thermo table and, by default, the k-epsilon model on: no state"""
    from dfmi.lib import Context
    from dfmi import case
    ym, t = _mech()
    ctx = Context(0)
    pt = case.default_patch_types(m)
    case.setup_context(ctx, m, t, ym["species"].index("N2"), 1e-6, pt)
    if ras:
        ctx.set_option("ras.model", 1)
    return ctx, t, pt


def _set_fgm_patch_types(ctx, m, types=None):
    from dfmi.mesh import ZERO_GRADIENT
    for n in ("Z", "Zvar", "c", "cvar", "Zcvar", "Ha"):
        ctx.set_patch_types(n, m.patch_types(ZERO_GRADIENT) if types is None else types[n])


def _species_maps(tab, S):
    """distinct mechanism indices for the table's species, descending from S - 1, and for its source species"""
    return [S - 1 - 2 * j if S - 1 - 2 * j >= 0 else j for j in range(tab.NY)][:tab.NY], list(range(tab.NYomega))


@pytest.fixture(scope="module", params=list(GRIDS))
def grid(request):
    from dfmi.mesh import hex_box
    nx, ny, nz = GRIDS[request.param]
    m = hex_box(nx, ny, nz, lengths=(1e-3 * nx, 1e-3 * ny, 1e-3 * nz), periodic=(False,) * 3)
    assert m.n_cells == request.param
    ctx, t, pt = _bare_context(m)
    _set_fgm_patch_types(ctx, m)
    yield ctx, m, t
    ctx.close()


def _spread(st, n, stride, shift):
    idx = (np.arange(n) * stride + shift) % len(st["Z"])
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}


def _push_inputs(ctx, cells, slots, S, C, B):
    for k in FR.STATE_FIELDS:
        ctx.set_field(k, cells[k])
        ctx.set_field("boundary_" + k, slots[k])
    ctx.set_field("Y", np.full((S, C), SENTINEL))
    ctx.set_field("boundary_Y", np.full((S, B), SENTINEL))
    for n in ("Cp", "Hf"):
        ctx.set_field(n, np.full(C, SENTINEL))
        ctx.set_field("boundary_" + n, np.full(B, SENTINEL))


def _pull_outputs(ctx, tab, S, C, B):
    out = {}
    for pre, n in (("", C), ("boundary_", B)):
        for f in OUT1:
            out[pre + f] = ctx.get_field(pre + f, (n,))
        out[pre + "Y"] = ctx.get_field(pre + "Y", (S, n))
        out[pre + "omega_Yi"] = ctx.get_field(pre + "omega_Yi", (max(tab.NYomega, 1), n))
    return out


def _check_side(tab, opts, st, got, pre, slot, ysp, bound, where):
    with np.errstate(all="ignore"):
        ref = FR.retrieve(tab, opts, st, slot=slot, write_rho=False)
    n = len(st["Z"])
    for f in FR.BITWISE:
        if f in ("Y", "omega_Yi"):
            continue
        want = ref[f] if ref[f] is not None else np.full(n, SENTINEL)       # flameletT: Cp and Hf untouched
        assert np.array_equal(got[pre + f], want), (where, pre + f, ulp_diff(got[pre + f], want))
    Y = got[pre + "Y"]
    for j in range(tab.NY):
        assert np.array_equal(Y[ysp[j]], ref["Y"][j]), (where, pre + "Y", j)
    others = [s for s in range(Y.shape[0]) if s not in ysp]
    assert np.all(Y[others] == SENTINEL), (where, "species outside the table were written")
    for j in range(tab.NYomega):
        assert np.array_equal(got[pre + "omega_Yi"][j], ref["omega_Yi"][j]), (where, pre + "omega_Yi", j)
    chi = got[pre + "chi_c"]
    err, fl = FR.chi_c_error(tab, opts, st, chi, slot)
    assert np.array_equal(chi[~fl], ref["chi_c"][~fl]), (where, pre + "chi_c outside the flame")
    worst = float(err.max()) if err.size else 0.0
    assert worst <= bound, (where, pre + "chi_c", worst, bound)
    return worst, int(fl.sum())


@pytest.mark.parametrize("cls", FR.CLASSES)
@pytest.mark.parametrize("name", FR.TABLES)
def test_retrieval_of_cells_and_slots(grid, name, cls):
    ctx, m, t = grid
    C, B, S = m.n_cells, m.n_boundary_slots, t.S
    tab = FR.class_table(name, cls)
    st, dropped = FR.states(name, cls)
    assert dropped <= FR.MAX_DROPPED
    ysp, osp = _species_maps(tab, S)
    ctx.fgm_set_table(tab, ysp, osp)
    cells, slots = _spread(st, C, 1, 0), _spread(st, B, 7, 3)
    bound = FR.gpu_bound(FR.load_bounds(), name, cls)
    runs = [{"combustion": 1, "flameletT": 0, "incompPref": -10.0}, {"combustion": 1, "flameletT": 1, "incompPref": 101325.0}]
    if cls == "no_flame":
        runs.append({"combustion": 0, "flameletT": 0, "incompPref": -10.0})
    worst, nflame = 0.0, 0
    for o in runs:
        for k, v in o.items():
            ctx.set_option("fgm." + k, v)
        both = []
        for rep in range(2):
            _push_inputs(ctx, cells, slots, S, C, B)
            ctx.set_field("rho_thermo", np.full(C, SENTINEL))
            ctx.fgm_retrieve()
            both.append(_pull_outputs(ctx, tab, S, C, B))
        for f, v in both[0].items():
            assert np.array_equal(v, both[1][f], equal_nan=True), (f, "two runs differ")
        got = both[0]
        where = (m.n_cells, name, cls, tuple(o.values()))
        # the constructor's retrieval: cell rho is left alone and rho_thermo is that rho
        assert np.array_equal(got["rho"], cells["rho"]) and np.array_equal(got["rho_thermo"], cells["rho"]), where
        got_c = dict(got, rho=cells["rho"], rho_thermo=cells["rho"])
        w1, n1 = _check_side(tab, o, cells, got_c, "", False, ysp, bound, where)
        w2, n2 = _check_side(tab, o, slots, got, "boundary_", True, ysp, bound, where)
        worst, nflame = max(worst, w1, w2), nflame + n1 + n2
    print(f"fgm retrieval {m.n_cells} cells {name} {cls}: chi_c worst {worst:.3e} over {nflame} flame points (bound {bound:.1e})")
    ctx.set_option("fgm.combustion", 0)      # the library's defaults again for the next case of the shared context
    ctx.set_option("fgm.flameletT", 0)
    ctx.set_option("fgm.incompPref", -10.0)


# ------------------------------------------------------------------------------------------------ refusals
def _raises(fn, *needles):
    from dfmi.lib import DfmiError
    with pytest.raises(DfmiError) as e:
        fn()
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def _copy_table(tab, **kw):
    import copy
    t = copy.copy(tab)
    t.axes = [a.copy() for a in tab.axes]
    t.laminar, t.values = tab.laminar.copy(), tab.values.copy()
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_refusals_by_name():
    from dfmi.mesh import hex_box
    m = hex_box(3, 2, 2, lengths=(3e-3, 2e-3, 2e-3), periodic=(False,) * 3)
    ctx, t, pt = _bare_context(m, ras=False)
    C, B, S = m.n_cells, m.n_boundary_slots, t.S
    tab = FR.make_table("full")
    ysp, osp = _species_maps(tab, S)
    try:
        # the model without what it needs
        _raises(lambda: ctx.set_option("fgm.model", 1), "fgm.model = 1", "dfmi_fgm_set_table")
        _raises(lambda: ctx.set_option("fgm.no_such_key", 1), "fgm.no_such_key")
        _raises(lambda: ctx.set_option("fgm.model", 2), "fgm.model must be 0 or 1")
        _raises(lambda: ctx.set_option("fgm.Sct", 0.0), "fgm.Sct must be positive")
        _raises(lambda: ctx.set_option("fgm.TMax", float("inf")), "fgm.TMax must be positive and finite")
        _raises(lambda: ctx.set_option("fgm.incompPref", float("nan")), "fgm.incompPref must be finite")
        # the table
        bad = _copy_table(tab, NS=12)
        _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), "NS = 12 must be 8 + NYomega")
        bad = _copy_table(tab)
        bad.axes[1][2] = bad.axes[1][1]
        _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), "axis z is not strictly increasing at index 2")
        bad = _copy_table(tab)
        bad.axes[3][0] = float("nan")
        _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), "axis gz holds a value that is not finite")
        bad = _copy_table(tab)
        bad.values[5, 17] = float("inf")
        _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), "a value table holds a value that is not finite")
        bad = _copy_table(tab)
        bad.laminar[2, 3] = float("nan")
        _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), "the laminar block holds a value that is not finite")
        bad = _copy_table(tab)
        bad.laminar[0, 5] = bad.laminar[0, 4]
        _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), "axis z of the laminar block is not strictly increasing in row 1")
        bad = _copy_table(tab, d2Yeq=np.where(np.arange(tab.d2Yeq.size) == 4, np.nan, tab.d2Yeq))
        _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), "d2Yeq / d1Yeq holds a value that is not finite")
        _raises(lambda: ctx.fgm_set_table(tab, [0, 1, S], osp), f"species index {S}", "out of range")
        _raises(lambda: ctx.fgm_set_table(tab, ysp, [-1]), "species index -1", "omega species 0")

        class Dims(type(tab)):
            def dims(self):
                return self._dims
        for i, nm in ((0, "NH"), (4, "NGC")):
            bad = _copy_table(tab)
            bad.__class__ = Dims
            bad._dims = tab.dims()
            bad._dims[i] = 0
            _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), f"dimension {nm} = 0 must be at least 1")
        bad = _copy_table(tab)
        bad.__class__ = Dims
        bad._dims = tab.dims()
        bad._dims[0] = 1 << 28
        _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), "more than 2^28 entries", "too large")
        bad = _copy_table(tab)
        bad.__class__ = Dims
        bad._dims = tab.dims()
        bad._dims[9] = 1
        _raises(lambda: ctx.fgm_set_table(bad, ysp, osp), "NZL = 1 must be at least 2")
        _raises(lambda: ctx.fgm_retrieve(), "no flamelet table set")
        ctx.fgm_set_table(tab, ysp, osp)
        # the model against the other models
        _raises(lambda: ctx.set_option("fgm.model", 1), "needs ras.model = 1")
        _raises(lambda: ctx.fgm_retrieve(), "needs ras.model = 1")
        ctx.set_option("les.model", 1)
        _raises(lambda: ctx.set_option("fgm.model", 1), "ras.model = 1")
        ctx.set_option("les.model", 0)
        ctx.set_option("ras.model", 1)
        ctx.chem_set_options(1)
        _raises(lambda: ctx.set_option("fgm.model", 1), "chemistry mode != 0")
        ctx.chem_set_options(0)
        ctx.thermo_set_eos(1, np.full(S, 1e5), np.full(S, 0.02), np.full(S, 0.1))
        _raises(lambda: ctx.set_option("fgm.model", 1), "equation of state")
        ctx.thermo_set_eos(0)
        ctx.set_option("tci.model", 1)
        _raises(lambda: ctx.set_option("fgm.model", 1), "tci.model != 0")
        ctx.set_option("tci.model", 0)
        # patch types and fields
        _raises(lambda: ctx.fgm_retrieve(), "patch types not set for field 'Z'")
        from dfmi.mesh import INLET_OUTLET
        _raises(lambda: ctx.set_patch_types("Zvar", m.patch_types(INLET_OUTLET)), "Zvar takes zeroGradient, fixedValue")
        _set_fgm_patch_types(ctx, m)
        _raises(lambda: ctx.fgm_retrieve(), "the field 'k' is not set")
        _raises(lambda: ctx.set_field("fgm_Su", np.zeros(C)), "fgm_Su", "cannot be set")
        _raises(lambda: ctx.set_scheme("div(phi,Zvar)", "linear"), "div(phi,Zvar): upwind, limitedLinear or limitedLinear01")
        _raises(lambda: ctx.set_scheme("div(phi,Zq)", "upwind"), "unknown scheme term 'div(phi,Zq)'")
        for term in ("div(phi,Z)", "div(phi,Zvar)", "div(phi,c)", "div(phi,cvar)", "div(phi,Zcvar)", "div(phi,Ha)"):
            ctx.set_scheme(term, "Gauss limitedLinear01 1")
            ctx.set_scheme(term, "limitedLinear 1")
            ctx.set_scheme(term, "upwind")
        # with the model on: the entries it replaces, and the models that exclude it
        ctx.set_option("fgm.model", 1)
        assert ctx.get_option("fgm.model") == 1.0
        _raises(lambda: ctx.call("Y_process"), "dfmi_Y_process is not available with fgm.model = 1")
        _raises(lambda: ctx.call("E_process"), "dfmi_E_process is not available with fgm.model = 1")
        _raises(lambda: ctx.zero_d_step(1e-6), "dfmi_zero_d_step is not available with fgm.model = 1")
        _raises(lambda: ctx.set_option("ras.model", 0), "ras.model = 0 is refused while fgm.model = 1")
        _raises(lambda: ctx.set_option("les.model", 1), "exclude each other")
        _raises(lambda: ctx.set_option("tci.model", 1), "fgm.model = 1 exclude each other")
        ctx.chem_set_options(1)
        _raises(lambda: ctx.time_step(1), "chemistry mode != 0")
        ctx.chem_set_options(0)
        ctx.set_option("fgm.model", 0)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ transport, correct, time step
PARTS = ["lower", "upper", "diag", "source", "internal_coeffs", "boundary_coeffs"]
L0 = 1e-3
INLET = {"Z": 0.4, "c": 0.1}
FIELDS_OUT = ("T", "p", "rho", "rho_thermo", "psi", "mu", "k", "epsilon", "nut") + FR.EQS + FR.FGM_OUT


def _mesh(name):
    import ras_reference as R
    from dfmi.mesh import hex_box
    if name == "periodic-xy":
        return hex_box(8, 8, 8, lengths=(2 * np.pi * L0,) * 3, periodic=(True, True, False), gradings=(1.0, 1.3, 1.2))
    return R.get_mesh(name)


def _global_fields(mg, tab):
    """the six scalars, k and epsilon as functions of the cell centres (the same on any decomposition). The phases keep
    the fields off the boxes' mirror planes: sin x alone takes exactly the same value in the cells either side of x = pi / 2
    on a uniform axis, and on a face whose two values are exactly equal limitedLinear's r = 2 * 1000 * sign(gradc) *
    sign(gradf) - 1 depends on which side evaluates it (sign(0) = 1 for both), so a processor face there gets the weight
    each rank's own orientation gives, as OpenFOAM's coupled patches do, and no longer the single domain's"""
    x, y, z = (mg.cell_centres / L0).T
    Z = 0.35 + 0.25 * np.sin(x + 0.3) * np.cos(y) + 0.05 * np.cos(z + 0.2)
    c = 0.45 + 0.3 * np.cos(x + 0.4) * np.sin(y) * np.cos(0.5 * z)
    f = {"Z": Z, "c": c, "Zvar": 0.25 * Z * (1 - Z) * (0.6 + 0.3 * np.sin(y + z)),
         "cvar": 0.2 * c * (1 - c) * (0.5 + 0.4 * np.cos(x - z)), "k": 0.3 * (1 + 0.4 * np.sin(x + y)),
         "epsilon": 2e3 * (1 + 0.4 * np.cos(y - z))}
    f["Zcvar"] = 0.4 * np.sin(x + 2 * y) * np.sqrt(f["Zvar"] * f["cvar"])
    f["Ha"] = (Z * (tab.Hfu - tab.Hox) + tab.Hox) - (-6e4 + 5e4 * np.sin(x) * np.sin(z))
    return f


def _fgm_ptypes(m):
    """fixedValue inlets of Z, c and Ha on the patch `left` (where the mesh has that wall), zeroGradient / coupled elsewhere"""
    from dfmi.mesh import FIXED_VALUE, ZERO_GRADIENT
    out = {}
    for n in FR.EQS:
        t = m.patch_types(ZERO_GRADIENT).copy()
        if n in ("Z", "c", "Ha"):
            for i, p in enumerate(m.patches):
                if p.name == "left" and p.kind not in ("cyclic", "processor", "processorCyclic"):
                    t[i] = FIXED_VALUE
        out[n] = t
    return out


def _setup(m, g, mg, tabname, opts, comm=None, mesh_schemes=None, fgm_schemes=None, model=1):
    """a context on mesh m (cells g of the global mesh mg) with the k-epsilon model, the table and the flareFGM fields;
    returns (ctx, thermo table, patch types, fgm patch types, species map, dt, inert)"""
    from dfmi import case
    from dfmi.lib import Context
    ym, t = _mech()
    inert = ym["species"].index("N2")
    dt = 1e-6
    tab = FR.make_table(tabname)
    ctx = Context(0)
    pt = case.default_patch_types(m)
    case.setup_context(ctx, m, t, inert, dt, pt, comm=comm, schemes=mesh_schemes)
    for e in ("U", "Y", "E", "k", "epsilon") + FR.EQS:
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-15, 1e-300)
    zg = m.patch_types(0)
    ctx.set_patch_types("k", zg); ctx.set_patch_types("epsilon", zg)
    ctx.set_option("ras.model", 1)
    tg = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    case.init_state(ctx, m, t.S, tg["T"][g], tg["p"][g], tg["U"][:, g], tg["Y"][:, g])
    fpt = _fgm_ptypes(m)
    for n in FR.EQS:
        ctx.set_patch_types(n, fpt[n])
    F = _global_fields(mg, tab)
    inlet = dict(INLET, Ha=(INLET["Z"] * (tab.Hfu - tab.Hox) + tab.Hox) + 4e4)
    for n, v in F.items():
        b = case.boundary_values(m, v[g]).reshape(-1)
        if n in inlet:
            for i, p in enumerate(m.patches):
                if fpt[n][i] == 1:
                    b[case.patch_slots(m, p.name)] = inlet[n]
        ctx.set_field(n, np.ascontiguousarray(v[g]))
        ctx.set_field("boundary_" + n, b)
    ysp, osp = _species_maps(tab, t.S)
    ctx.fgm_set_table(tab, ysp, osp)
    for kk, v in opts.items():
        ctx.set_option("fgm." + kk, v)
    for n, s in (fgm_schemes or {}).items():
        ctx.set_scheme(f"div(phi,{n})", s)
    ctx.set_option("fgm.model", model)
    ctx.call("pre_time_step")
    return ctx, t, pt, fpt, ysp, dt, inert


def _pull(ctx, m, t, tab):
    """the state an FgmOracle starts from: the solver's fields, k and epsilon, and the flareFGM fields"""
    from dfmi import case
    C, B = m.n_cells, m.n_boundary_slots
    st = case.pull_state(ctx, m, t.S)
    extra = {}
    for n in ("k", "epsilon", "rho_thermo") + FR.EQS + FR.FGM_OUT:
        extra[n] = ctx.get_field(n, (C,))
        extra["boundary_" + n] = ctx.get_field("boundary_" + n, (B,))
    no = max(tab.NYomega, 1)
    extra["omega_Yi"], extra["boundary_omega_Yi"] = ctx.get_field("omega_Yi", (no, C)), ctx.get_field("boundary_omega_Yi", (no, B))
    return st, extra


def _oracle(m, t, st, extra, pt, fpt, inert, dt, tabname, opts, ysp, fgm_schemes=None):
    st = {k: v.copy() for k, v in st.items()}
    for pre in ("", "boundary_"):
        st[pre + "rho_thermo"] = extra[pre + "rho_thermo"].copy()
    zg = m.patch_types(0)
    return FR.make_oracle(m, t, st, dict(pt), inert, 1.0 / dt, {}, extra["k"], extra["epsilon"], extra["boundary_k"],
                          extra["boundary_epsilon"], FR.make_table(tabname), opts, extra, fpt, ysp, schemes_fgm=fgm_schemes,
                          k_ptypes=zg, eps_ptypes=zg)


SCHEMES = {"Z": "limitedLinear01 1", "Zvar": "limitedLinear 1", "c": "limitedLinear01 1", "cvar": "limitedLinear 1",
           "Zcvar": "limitedLinear 1", "Ha": "limitedLinear 1"}


@pytest.mark.parametrize("name", ["walls", "periodic-xy", "sheared-walls"])
def test_transport_matrices_bitwise(name):
    """the six assembled matrices at 0 ulp against ras_reference.scalar_assemble with the restated D and Su, upwind and the
    fgm cases' limited schemes; Z and c pushed outside [0, 1] in places so limitedLinear01's cut acts; the corrected
    laplacian on the sheared box (its explicit term at the non-orthogonal suite's own bound form)"""
    import nonorth_reference as NR
    m = _mesh(name)
    corrected = name == "sheared-walls"
    C, B, F = m.n_cells, m.n_boundary_slots, m.n_faces
    opts = {"combustion": 1, "solveEnthalpy": 1, "Sct": 0.8, "Sc": 0.9}
    ctx, t, pt, fpt, ysp, dt, inert = _setup(m, np.arange(C), m, "full", opts, mesh_schemes={"laplacian": "corrected"} if corrected else None)
    try:
        ctx.fgm_retrieve()                                     # chi_*, the omegas, mu: the state a first correct() meets
        rng = np.random.default_rng(3)
        for n in ("Z", "c"):                                   # a few cells outside [0, 1]
            v = ctx.get_field(n, (C,))
            idx = rng.choice(C, max(C // 10, 4), replace=False)
            v[idx] += np.where(rng.integers(0, 2, idx.size) == 1, 0.9, -0.9)
            ctx.set_field(n, v)
        tab = FR.make_table("full")
        st, extra = _pull(ctx, m, t, tab)
        for scheme in ("upwind", "limited"):
            sch = SCHEMES if scheme == "limited" else {n: "upwind" for n in FR.EQS}
            for n, s in sch.items():
                ctx.set_scheme(f"div(phi,{n})", "Gauss " + s)
            orc = _oracle(m, t, st, extra, pt, fpt, inert, dt, "full", opts, ysp, fgm_schemes=sch)
            dc = bdc = None
            if corrected:
                dc, _, bdc, _ = m.nonorth_geometry()
                orc.dc, orc.bdc = dc, bdc
            for eq in FR.EQS:
                ctx.assemble(eq)
                size = {"lower": F, "upper": F, "diag": C, "source": C, "internal_coeffs": B, "boundary_coeffs": B}
                dev = {p: ctx.get_matrix(eq, p, size[p]) for p in PARTS}
                ref = orc.assemble(eq)
                q = orc.matrices[eq]
                assert np.array_equal(ctx.get_field("fgm_Su", (C,)), q["Su"]), (name, scheme, eq, "Su")
                assert np.array_equal(ctx.get_field("fgm_D", (C,)), q["D"]) and np.array_equal(ctx.get_field("boundary_fgm_D", (B,)), q["bD"])
                for p in PARTS:
                    if corrected and p == "source":
                        continue
                    assert ulp_diff(dev[p], ref[p]) == 0, (name, scheme, eq, p, rel_err(dev[p], ref[p]))
                if eq in ("Zvar", "cvar", "Zcvar"):
                    assert np.abs(q["Su"]).max() > 0
                if corrected:
                    a = orc.arr
                    acc, _, _, sc = NR.corrected_term(m, fpt[eq], a[eq][None], a["boundary_" + eq][None], q["D"][None])
                    accL, _, _, _ = NR.corrected_term(m, fpt[eq], a[eq][None], a["boundary_" + eq][None], q["D"][None], T=NR.LD)
                    bound = NR.gpu_bound(NR.load_bounds(), "sheared-walls", "he")
                    err = np.abs((dev["source"] - ref["source"]) - np.asarray(accL[0], np.float64))
                    tol = bound * np.asarray(sc[0], np.float64) + 4 * np.finfo(float).eps * np.abs(ref["source"])
                    print(f"fgm corrected {eq}: max err / tol {np.max(err / tol):.3e}, term max {np.abs(acc).max():.3e}")
                    assert np.all(err <= tol) and np.abs(acc).max() > 0
            if scheme == "limited":
                assert ulp_diff(orc.matrices["Z"]["lower"], ref_z["lower"]) > 0      # the limiter is in the matrix
            else:
                ref_z = orc.matrices["Z"]
    finally:
        ctx.close()


CASES = [("full", 0, -10.0, 0), ("full", 1, 101325.0, 0), ("full_u", 1, -10.0, 1), ("full_u", 0, 101325.0, 0)]


@pytest.mark.parametrize("tabname,enthalpy,pref,flT", CASES)
def test_correct_and_time_step_against_oracle(tabname, enthalpy, pref, flT):
    """dfmi_fgm_correct, then one full dfmi_time_step (nCorr 2, kEpsilon, fixedValue inlets of Z / c / Ha on `left`,
    zeroGradient elsewhere) against FgmOracle at 1e-9 per field"""
    m = _mesh("walls")
    C, B = m.n_cells, m.n_boundary_slots
    tab = FR.make_table(tabname)
    opts = {"combustion": 1, "solveEnthalpy": enthalpy, "incompPref": pref, "flameletT": flT}
    fsch = {"Zvar": "limitedLinear 1", "c": "limitedLinear01 1"}
    ctx, t, pt, fpt, ysp, dt, inert = _setup(m, np.arange(C), m, tabname, opts, fgm_schemes=fsch)
    try:
        rho0 = ctx.get_field("rho", (C,))
        ctx.fgm_retrieve()                                     # the constructor's retrieval
        assert np.array_equal(ctx.get_field("rho", (C,)), rho0)
        st, extra = _pull(ctx, m, t, tab)
        worst = {}
        for stage in ("correct", "time_step"):
            orc = _oracle(m, t, st, extra, pt, fpt, inert, dt, tabname, opts, ysp, fgm_schemes=fsch)
            if stage == "correct":
                ctx.fgm_correct()
                orc.fgm_correct()
            else:
                ctx.time_step(2)
                orc.time_step(2)
            for n in FIELDS_OUT:
                for pre, cnt in (("", C), ("boundary_", B)):
                    if pre and n in ("nut",):
                        continue
                    e = rel_err(ctx.get_field(pre + n, (cnt,)), orc.arr[pre + n])
                    worst[stage] = max(worst.get(stage, 0.0), e)
                    assert e < 1e-9, (stage, pre + n, e)
            for n, kk in (("U", 3), ("Y", t.S)):
                e = rel_err(ctx.get_field(n, (kk, C)), orc.arr[n].reshape(kk, C))
                worst[stage] = max(worst.get(stage, 0.0), e)
                assert e < 1e-9, (stage, n, e)
            if stage == "correct":
                # the call moved what it should: the scalars, T, and the cells' rho = (incompPref > 0 ? incompPref : p) psi
                psi, p = ctx.get_field("psi", (C,)), ctx.get_field("p", (C,))
                assert np.array_equal(ctx.get_field("rho", (C,)), (pref if pref > 0 else p) * psi)
                assert np.array_equal(ctx.get_field("rho_thermo", (C,)), ctx.get_field("rho", (C,)))
                assert rel_err(ctx.get_field("Z", (C,)), extra["Z"]) > 1e-6 and rel_err(ctx.get_field("c", (C,)), extra["c"]) > 1e-6
                if enthalpy:
                    assert rel_err(ctx.get_field("Ha", (C,)), extra["Ha"]) > 1e-7
                else:
                    Z = ctx.get_field("Z", (C,))
                    assert np.array_equal(ctx.get_field("Ha", (C,)), Z * (tab.Hfu - tab.Hox) + tab.Hox)
                st, extra = _pull(ctx, m, t, tab)               # the time step starts from the device's own state
        print(f"fgm {tabname} solveEnthalpy {enthalpy} incompPref {pref} flameletT {flT}: worst rel err correct "
              f"{worst['correct']:.2e}, time step {worst['time_step']:.2e}")
        assert np.array_equal(ctx.get_field("rho", (C,)), ctx.get_field("rho_thermo", (C,)))
    finally:
        ctx.close()


_HUB = [1700]


@pytest.mark.parametrize("name,limited", [("periodic-xy", 1), ("walls", 1), ("periodic-xy", 0)])
def test_two_ranks_match_single_domain(name, limited):
    """retrieve and one full step on two ranks (graph bisection, the in-process transport) against the single domain: the
    x-y periodic box and the walled box with the fgm cases' limited schemes of Z and Zvar, the periodic box with upwind.
    With the limited schemes the limiter of Z must be active on the cut: some processor face carries a weight that is
    neither the upwind nor the linear one, so an error in the neighbour side's gradient, delta or weight would show."""
    from dfmi.partition import partition_cells, decompose
    mg = _mesh(name)
    opts = {"combustion": 1, "solveEnthalpy": 1}
    fsch = {"Z": "limitedLinear01 1", "Zvar": "limitedLinear 1"} if limited else {}
    names = ("T", "p", "rho", "rho_thermo", "psi", "mu", "k", "epsilon") + FR.EQS + ("chi_c", "omega_c", "Wt")

    def run(m, g, comm=None):
        ctx, t, *_ = _setup(m, g, mg, "full", opts, comm=comm, fgm_schemes=fsch)
        try:
            ctx.fgm_retrieve()
            ctx.time_step(2)
            o = {n: ctx.get_field(n, (m.n_cells,)) for n in names}
            o["U"] = ctx.get_field("U", (3, m.n_cells))
            if limited and comm is not None:      # the weights of the last limited assembly (Zvar's) on the processor slots
                import nonorth_reference as NR
                sl = NR.Slots(m)
                kind = np.concatenate([np.full(p.slots, p.kind in ("processor", "processorCyclic")) for p in m.patches])
                pr = kind & sl.prim
                bw = ctx.get_field("boundary_fgm_w", (m.n_boundary_slots,))[pr]
                lin = np.asarray(m.boundary_arrays()[3])[pr]
                o["active"] = int(((bw != 0.0) & (bw != 1.0) & (bw != lin)).sum())
                o["cut"] = int(pr.sum())
            return o
        finally:
            ctx.close()

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
    errs = {}
    for n in names + ("U",):
        kk = 3 if n == "U" else 1
        a = np.zeros((kk, mg.n_cells))
        for r in range(nr):
            a[:, meshes[r].cell_map] = out[r][n].reshape(kk, -1)
        errs[n] = rel_err(a, ref[n].reshape(kk, -1))
    print(f"fgm two ranks vs single domain {name} limited {limited}:", {n: f"{e:.2e}" for n, e in errs.items()})
    if limited:
        act = [(o_["active"], o_["cut"]) for o_ in out]
        print("  processor faces with a limiter strictly between upwind and linear (active, of):", act)
        assert all(a > 0 for a, _ in act), act
    for n, e in errs.items():
        assert e < 1e-9, (n, e)


# ------------------------------------------------------------------------------------------------ fgm.model = 0 after 1
def _plain_ras_context(m):
    """the context _setup builds, without a table, an fgm option, an fgm field or an fgm patch type"""
    from dfmi import case
    from dfmi.lib import Context
    ym, t = _mech()
    ctx = Context(0)
    case.setup_context(ctx, m, t, ym["species"].index("N2"), 1e-6, case.default_patch_types(m))
    for e in ("U", "Y", "E", "k", "epsilon"):
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-15, 1e-300)
    zg = m.patch_types(0)
    ctx.set_patch_types("k", zg); ctx.set_patch_types("epsilon", zg)
    ctx.set_option("ras.model", 1)
    tg = case.tgv_fields(m, ym["species"], kernel_radius=1.2e-3)
    case.init_state(ctx, m, t.S, tg["T"], tg["p"], tg["U"], tg["Y"])
    F = _global_fields(m, FR.make_table("full"))
    for n in ("k", "epsilon"):
        ctx.set_field(n, np.ascontiguousarray(F[n]))
        ctx.set_field("boundary_" + n, case.boundary_values(m, F[n]).reshape(-1))
    ctx.call("pre_time_step")
    return ctx, t


@pytest.mark.parametrize("ras", [0, 1])
def test_model_off_after_on_is_bitwise_a_context_that_never_set_it(ras):
    """one laminar step (ras 0) and one k-epsilon step (ras 1): a context that set the table, the fields and fgm.model = 1,
    retrieved once and then set fgm.model = 0 -- its thermo state put back -- against one that never touched the model"""
    from dfmi import case
    m = _mesh("walls")
    C = m.n_cells
    outs = []
    for touched in (False, True):
        if touched:
            ctx, t, *_ = _setup(m, np.arange(C), m, "full", {"combustion": 1}, model=1)
            B = m.n_boundary_slots
            keep = {}
            for n, kk in (("T", 1), ("psi", 1), ("mu", 1), ("rho", 1), ("Y", t.S)):
                for pre, cnt in (("", C), ("boundary_", B)):
                    keep[pre + n] = ctx.get_field(pre + n, (kk, cnt) if kk > 1 else (cnt,))
            ctx.fgm_retrieve()
            assert not np.array_equal(ctx.get_field("T", (C,)), keep["T"])      # the retrieval wrote the thermo fields
            for n, v in keep.items():
                ctx.set_field(n, v)
            ctx.set_option("fgm.model", 0)
        else:
            ctx, t = _plain_ras_context(m)
        try:
            ctx.set_option("ras.model", ras)
            ctx.time_step(2)
            o = {n: ctx.get_field(n, (C,)) for n in ("T", "p", "rho", "he", "psi", "mu")}
            o["U"], o["Y"] = ctx.get_field("U", (3, C)), ctx.get_field("Y", (t.S, C))
            if ras:
                o["k"], o["nut"] = ctx.get_field("k", (C,)), ctx.get_field("nut", (C,))
            outs.append(o)
        finally:
            ctx.close()
    for n in outs[0]:
        assert np.array_equal(outs[0][n], outs[1][n]), (ras, n, ulp_diff(outs[0][n], outs[1][n]))
