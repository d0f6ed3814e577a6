"""PaSR and EDC combustion closures on the device (MI355X): include/dfmi.h dfmi_combustion_correct, DESIGN 15.

Pointwise quantities (tci_tmix, tci_tc, tci_kappa, tci_tauStar) are held per cell to the long-double restatement
tests/tci_reference.py at 4x the fp64 restatement's measured error (tests/golden/tci_bounds.json), floored at 1e-13. They are
formed by dfmi_assemble("tci") -- the closure's passes without the solve -- so RR can be seeded by hand on every side of
every comparison. The per-cell integration interval of the three integrator families is held bitwise to the scalar solve,
the consumers and full steps bitwise to a twin context that is handed RR_eff as its RR.

Integrator families: "gen" Burke 9 species on the generated kernel, "generic" the same with chem.generated = 0, "coop21"
DRM19 (21 species) on the cooperative kernel, "coop9" Burke with chem.coop = 1.
"""
import json
import os
import threading

import numpy as np
import pytest

import tci_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GRIDS = {1: (1, 1, 1), 255: (3, 5, 17), 256: (4, 8, 8), 257: (257, 1, 1), 309: (3, 103, 1)}
FAMILIES = {"gen": "burke9", "generic": "burke9", "coop21": "drm19", "coop9": "burke9"}
THERMO = {"burke9": "thermo_Burke2012_s9r23.txt", "drm19": "thermo_drm19.txt"}
POINT_FIELDS = ("T", "p", "rho", "mu", "k", "epsilon", "Y", "RR", "Qdot", "tci_tc")
_mechs, _refs = {}, {}


def _mech(name):
    if name not in _mechs:
        from dfmi.mech import read_thermo_table
        species, mc, nasa, W = R.load_mech(name)
        _mechs[name] = (species, mc, nasa, W, read_thermo_table(os.path.join(GOLDEN, THERMO[name]), species))
    return _mechs[name]


def _ctx(family, n, ras=True):
    from dfmi import case
    from dfmi.lib import Context
    from dfmi.mesh import hex_box
    species, mc, nasa, W, t = _mech(FAMILIES[family])
    m = hex_box(*n)
    ctx = Context(0)
    case.setup_context(ctx, m, t, species.index("N2"), 1e-6)
    ctx.chem_set_mechanism(mc)
    ctx.chem_set_options(1, rtol=1e-8, atol=1e-14)
    if family == "generic":
        ctx.set_option("chem.generated", 0)
    if family == "coop9":
        ctx.set_option("chem.coop", 1)
    if ras:
        ctx.set_option("ras.model", 1)
    return ctx, m


def _push(ctx, st, names=POINT_FIELDS):
    for n in names:
        ctx.set_field(n, np.ascontiguousarray(st[n]))


def _state(mech, cls, n):
    """(state, coefficient overrides) of a class on n cells, with a pure-inert cell (the reactionRate scale is vGreat)"""
    species, mc, nasa, W, t = _mech(mech)
    S = len(species)
    idx = R.species_idx(species)
    st, coef = {"broad": (R.broad(n, S, W), None), "branches": (R.branches_pasr(n, S, W, idx), {"Cmix": 1e-15}),
                "branches_edc": (R.branches_edc(n, S, W), {"Cgamma": 1.0})}[cls]
    if n > 5:
        R.inert_cell(st, n - 1, S, species.index("N2"))
    return st, coef


def _tc_reaction_ld(mech, cls, n):
    """the long-double reactionRate scale of a class, computed once per (mechanism, class, size)"""
    key = (mech, cls, n)
    if key not in _refs:
        species, mc, nasa, W, t = _mech(mech)
        st, _ = _state(mech, cls, n)
        _refs[key] = R.tc_reaction(mc, nasa, W, st["T"], st["p"], st["rho"], st["Y"], T=R.LD)
    return _refs[key]


@pytest.fixture(scope="module")
def bounds():
    return R.load_bounds()


def _hold(got, ref, bound, what):
    e = R.rel_error(got, ref)
    worst = float(np.nanmax(e, initial=0.0))
    print(f"{what}: {worst:.3e} (bound {bound:.1e})")
    assert np.all(np.isfinite(e)) and worst <= bound, (what, worst, bound)


def _set_tci(ctx, model, idx=None, coef=None, **kw):
    for k, v in dict(R.DEFAULTS, **(coef or {})).items():
        ctx.set_option("tci." + k, v)
    for k in R.IDX_NAMES:
        ctx.set_option("tci." + k, (idx or {}).get(k, -1))
    for k, v in kw.items():
        ctx.set_option("tci." + k, v)
    ctx.set_option("tci.model", model)


# ------------------------------------------------------------------------------------------------ 1. pointwise
def _pointwise(family, ncell, bounds, full):
    mech = FAMILIES[family]
    species, mc, nasa, W, t = _mech(mech)
    S = len(species)
    idx = R.species_idx(species)
    ctx, m = _ctx(family, GRIDS[ncell])
    C = m.n_cells
    assert C == ncell
    get = lambda n: ctx.get_field(n, (C,))
    try:
        for cls in ("broad", "branches", "branches_edc"):
            st, coef = _state(mech, cls, C)
            _push(ctx, st)
            combos = [(mx, ch) for mx in (1, 2, 3) for ch in (1, 2, 3)] if full else [(1, 3), (3, 1)]
            for mixing, chem in combos:
                _set_tci(ctx, 1, idx, coef, mixing=mixing, chemistry=chem)
                c64, cLD = [], []
                mech3 = (mc, nasa, W)
                R.evaluate_pasr(st, mixing, chem if chem != 3 else 2, idx, coef, cmp=c64)
                ref = R.evaluate_pasr(st, mixing, chem if chem != 3 else 2, idx, coef, T=R.LD, cmp=cLD)
                if chem == 3:
                    ref["tci_tc"] = _tc_reaction_ld(mech, cls, C)
                    c64, cLD = [], []
                    ref["tci_kappa"] = R.kappa_pasr(ref["tci_tmix"], ref["tci_tc"], R.LD, cLD)
                    R.kappa_pasr(np.asarray(ref["tci_tmix"], np.float64), np.asarray(ref["tci_tc"], np.float64), cmp=c64)
                assert R.branch_report(c64, cLD) == [], (cls, mixing, chem)
                runs = []
                for _ in range(2):
                    ctx.set_field("tci_tc", st["tci_tc"])                     # globalConvertion reads it as t0 and writes it
                    ctx.assemble("tci")
                    runs.append({n: get(n) for n in ("tci_tmix", "tci_tc", "tci_kappa", "Qdot_eff")})
                    runs[-1]["RR_eff"] = ctx.get_field("RR_eff", (S, C))
                for n, v in runs[0].items():
                    assert np.array_equal(v, runs[1][n], equal_nan=True), ("two runs", n)
                got = runs[0]
                for q in ("tci_tmix", "tci_tc", "tci_kappa"):
                    _hold(got[q], ref[q], R.gpu_bound(bounds, mech, cls, f"pasr.c{chem}.{q}"), f"{family} {C} {cls} m{mixing} c{chem} {q}")
                assert np.all((got["tci_kappa"] >= 0) & (got["tci_kappa"] <= 1))
                assert np.array_equal(got["RR_eff"], got["tci_kappa"][None, :] * st["RR"])      # one rounding each
                assert np.array_equal(got["Qdot_eff"], got["tci_kappa"] * st["Qdot"])
                assert np.array_equal(ctx.get_field("RR", (S, C)), st["RR"]) and np.array_equal(get("Qdot"), st["Qdot"])
                if chem == 3 and C > 5:
                    assert got["tci_tc"][C - 1] == R.VGREAT and got["tci_kappa"][C - 1] == 1.0   # pure inert: every rate 0
                    assert np.all(got["tci_tc"][:C - 1] < 1e200)
            if full and cls == "broad":                                      # an index of -1 for each of the four species
                for drop in R.IDX_NAMES:
                    if idx[drop] < 0 or drop == "fuel":
                        continue
                    sub = dict(idx, **{drop: -1})
                    _set_tci(ctx, 1, sub, coef, mixing=1, chemistry=1)
                    ctx.set_field("tci_tc", st["tci_tc"])
                    ctx.assemble("tci")
                    ref = R.evaluate_pasr(st, 1, 1, sub, coef, T=R.LD)
                    _hold(get("tci_tc"), ref["tci_tc"], R.gpu_bound(bounds, mech, cls, "pasr.c1.tci_tc"), f"{family} without {drop}")
                only_fuel = {k: (idx[k] if k == "fuel" else -1) for k in R.IDX_NAMES}
                _set_tci(ctx, 1, only_fuel, coef, mixing=1, chemistry=1)
                ctx.set_field("tci_tc", st["tci_tc"])
                ctx.assemble("tci")
                _hold(get("tci_tc"), R.evaluate_pasr(st, 1, 1, only_fuel, coef, T=R.LD)["tci_tc"],
                      R.gpu_bound(bounds, mech, cls, "pasr.c1.tci_tc"), f"{family} fuel only")
            versions = [(v, e) for v in R.VERSION_EXP for e in ((0, 0), (1, 4), (4, 1), (3, 2))] if full else [(2005, (0, 0)), (2016, (3, 2))]
            for ver, (e1, e2) in versions:
                _set_tci(ctx, 2, idx, coef, version=ver, exp1=e1, exp2=e2)
                c64, cLD = [], []
                r64 = R.evaluate_edc(st, ver, coef, e1, e2, cmp=c64)
                ref = R.evaluate_edc(st, ver, coef, e1, e2, T=R.LD, cmp=cLD)
                assert R.branch_report(c64, cLD) == [], (cls, ver, e1, e2)
                if ver == 2016 and cls == "branches_edc" and C >= 64:        # every clamp of v2016 is active somewhere
                    for a, b, _ in cLD[:5]:
                        fin = np.isfinite(np.asarray(a, np.float64))
                        assert (a[fin] > b[fin]).any() and (a[fin] < b[fin]).any()
                runs = []
                for _ in range(2):
                    ctx.assemble("tci")
                    runs.append({n: get(n) for n in ("tci_kappa", "tci_tauStar", "tci_tc", "Qdot_eff")})
                    runs[-1]["RR_eff"] = ctx.get_field("RR_eff", (S, C))
                    runs[-1]["bad"] = ctx.get_option("tci.bad_tauStar")
                for n, v in runs[0].items():
                    assert np.array_equal(v, runs[1][n], equal_nan=True), ("two runs", n)
                got = runs[0]
                for q in ref:
                    _hold(got[q], ref[q], R.gpu_bound(bounds, mech, cls, f"edc.v{ver}.{q}"), f"{family} {C} {cls} v{ver} {e1}{e2} {q}")
                tau = r64["tci_tauStar"]
                assert got["bad"] == np.count_nonzero(~((tau > 0) & np.isfinite(tau)))
                if cls == "branches_edc" and C >= 64:
                    assert got["bad"] >= 1
                ok = np.isfinite(got["tci_kappa"])
                assert np.all((got["tci_kappa"][ok] >= 0) & (got["tci_kappa"][ok] <= 1))
                assert np.array_equal(got["RR_eff"], got["tci_kappa"][None, :] * st["RR"], equal_nan=True)
                assert np.array_equal(got["Qdot_eff"], got["tci_kappa"] * st["Qdot"], equal_nan=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_pointwise_against_long_double(family, bounds):
    """all three mixing scales x three chemistry scales, all four EDC versions with default and overridden exponents, on
    309 cells of every state class"""
    _pointwise(family, 309, bounds, full=True)


@pytest.mark.parametrize("ncell", [1, 255, 256, 257])
@pytest.mark.parametrize("family", ["gen", "coop21"])
def test_pointwise_grid_sizes(family, ncell, bounds):
    """the per-lane and the cooperative k_tci_rates and the pointwise pass on 1, 255, 256 and 257 cells"""
    _pointwise(family, ncell, bounds, full=False)


# ------------------------------------------------------------------------------------------------ 2. per-cell interval
def _reacting_states(family, C, seed=0):
    """T, p, rho, Y of C reacting cells: test_gpu_chemistry's H2 states, or DRM19's fixture states tiled"""
    mech = FAMILIES[family]
    species, mc, nasa, W, t = _mech(mech)
    if mech == "drm19":
        f = json.load(open(os.path.join(GOLDEN, "chem_large_states.json")))["mechanisms"]["drm19"]
        i = np.arange(C) % len(f["T"])
        return np.asarray(f["T"])[i], np.asarray(f["p"])[i], np.asarray(f["rho"])[i], np.asarray(f["Y"])[:, i]
    from dfmi.case import h2_air_compositions
    rng = np.random.default_rng(seed)
    yu, yb = h2_air_compositions(species)
    prog = rng.random(C)
    Y = (1 - prog) * yu[:, None] + prog * yb[:, None] + rng.random((len(species), C)) * 1e-3
    Y /= Y.sum(axis=0)
    T = 300.0 + 2200.0 * rng.random(C)
    Wm = 1.0 / (Y / W[:, None]).sum(axis=0)
    p = 101325.0 * (1.0 + 0.05 * rng.standard_normal(C))
    return T, p, p * Wm / (R.RU * T) * (1.0 + 0.02 * rng.standard_normal(C)), Y


@pytest.mark.parametrize("family", list(FAMILIES))
def test_per_cell_interval(family):
    """EDC v2005 with uniform rho and mu: tauStar = Ctau sqrt(mu / (rho + small) / (eps + small)) takes exactly the values
    epsilon gives it. One value everywhere, then five values over two decades shuffled over the cells (and two cells
    without a usable interval), each against the scalar solve of a twin context at that value -- with the remembered steps
    zeroed, and again with the first round's chem_stats in both contexts, so that the cost binning permutes the cells."""
    from chem_oracle import Kinetics
    species, mc, nasa, W, t = _mech(FAMILIES[family])
    S = len(species)
    n = (8, 8, 4) if FAMILIES[family] == "burke9" else (5, 5, 3)
    ctx, m = _ctx(family, n)
    twin, _ = _ctx(family, n, ras=False)
    C = m.n_cells
    try:
        T, p, _, Y = _reacting_states(family, C)
        one = np.ones(C)
        rho = one.copy()                                  # the density RR is scaled by; uniform, so that nu and tauStar are
        for x in (ctx, twin):
            for nm, v in (("T", T), ("p", p), ("rho", rho), ("Y", Y)):
                x.set_field(nm, np.ascontiguousarray(v))
        mu = 2e-5 * one                                   # nu = mu / (rho + small): the same bits in every cell
        ctx.set_field("mu", mu); ctx.set_field("k", 30.0 * one)
        _set_tci(ctx, 2, None, None, version=2005)
        rng = np.random.default_rng(3)
        eps5 = 2e-5 * R.DEFAULTS["Ctau"] ** 2 / np.array([1e-7, 3e-7, 1e-6, 4e-6, 1e-5]) ** 2
        zeros = np.zeros((3, C))

        def edc(eps, stats):
            ctx.set_field("epsilon", eps); ctx.set_field("chem_stats", stats)
            ctx.combustion_correct(1e-6)                 # dt is not read: every cell has its own interval
            o = {"RR": ctx.get_field("RR", (S, C)), "RR_eff": ctx.get_field("RR_eff", (S, C)), "stats": ctx.get_field("chem_stats", (3, C))}
            for q in ("Qdot", "Qdot_eff", "tci_tauStar", "tci_kappa"):
                o[q] = ctx.get_field(q, (C,))
            o["bad"] = ctx.get_option("tci.bad_tauStar")
            return o

        def scalar(dt, stats):
            twin.set_field("chem_stats", stats)
            twin.chem_solve(dt)
            return {"RR": twin.get_field("RR", (S, C)), "Qdot": twin.get_field("Qdot", (C,)), "stats": twin.get_field("chem_stats", (3, C))}

        # one value everywhere
        a = edc(eps5[2] * one, zeros)
        tau = np.unique(a["tci_tauStar"])
        assert tau.size == 1 and 0.5e-6 < tau[0] < 2e-6 and a["bad"] == 0
        b = scalar(float(tau[0]), zeros)
        for q in ("RR", "Qdot", "stats"):
            assert np.array_equal(a[q], b[q]), ("uniform", q)
        assert np.abs(a["RR"]).max() > 0 and a["stats"][0].min() >= 1
        assert np.array_equal(a["RR_eff"], a["tci_kappa"][None, :] * a["RR"]) and np.array_equal(a["Qdot_eff"], a["tci_kappa"] * a["Qdot"])
        # five values shuffled over lanes and binning groups; two cells without a usable interval
        pick = rng.integers(0, 5, C)
        eps = eps5[pick]
        badc = [C // 3, C // 2]
        eps[badc[0]] = -1.0                               # sqrt of a negative number: NaN
        mu2 = mu.copy(); mu2[badc[1]] = 0.0               # tauStar = 0
        ctx.set_field("mu", mu2)
        good = np.ones(C, bool); good[badc] = False
        for rnd, stats in (("zeroed", zeros), ("binned", a["stats"])):
            d = edc(eps, stats)
            assert d["bad"] == 2
            assert not np.any(d["RR"][:, badc]) and not np.any(d["Qdot"][badc]) and not np.any(d["stats"][:2, badc])
            taus = np.unique(d["tci_tauStar"][good])
            assert taus.size == 5 and taus[-1] / taus[0] > 90
            for v in taus:
                sel = good & (d["tci_tauStar"] == v)
                u = scalar(float(v), stats)
                assert sel.sum() > 3
                for q in ("RR", "Qdot", "stats"):
                    assert np.array_equal(d[q][..., sel], u[q][..., sel]), (rnd, v, q)
        # against the oracle, each cell over its own interval (test_gpu_chemistry's tolerances at rtol 1e-8 / atol 1e-14)
        kin = Kinetics(mc, nasa, W)
        idx = np.flatnonzero(good)[::(13 if S < 12 else 19)]
        key = ("oracle", FAMILIES[family])
        if key not in _refs:                              # the same states and intervals for every family of a mechanism
            ref = np.zeros((S, idx.size))
            for j, c in enumerate(idx):
                ref[:, j] = kin.reaction_rates(T[c:c + 1], p[c:c + 1], rho[c:c + 1], Y[:, c:c + 1], float(d["tci_tauStar"][c]))[:, 0]
            _refs[key] = (d["tci_tauStar"][idx].copy(), ref)
        assert np.array_equal(_refs[key][0], d["tci_tauStar"][idx])
        ref = _refs[key][1]
        scale = np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1e-3 * np.abs(ref).max())
        rr = d["RR"][:, idx]
        e_glob, e_spec = np.abs(rr - ref).max() / scale.max(), (np.abs(rr - ref) / scale).max()
        print(f"{family}: per-cell intervals against the oracle {e_glob:.3e} global, {e_spec:.3e} per species")
        assert e_glob < 1e-5 and e_spec < 1e-4
    finally:
        ctx.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 3. consumers
def _ras_case(tci=None, chem=1):
    """test_gpu_ras's RAS box (walls, Burke) with the mechanism set, k and epsilon seeded"""
    from test_gpu_ras import Case
    species, mc, nasa, W, t = _mech("burke9")
    c = Case("walls")
    c.ctx.chem_set_mechanism(mc)
    c.ctx.chem_set_options(chem)
    rng = np.random.default_rng(61)
    C = c.m.n_cells
    c.k0 = 30.0 * (1 + 0.5 * rng.uniform(-1, 1, C))
    c.e0 = 4e5 * 10.0 ** rng.uniform(-2, 2, C)
    c.set_ke(c.k0, c.e0)
    if tci:
        _set_tci(c.ctx, tci["model"], R.species_idx(species), tci.get("coef"), **{k: v for k, v in tci.items() if k not in ("model", "coef")})
    return c


def _hot(c):
    """the case's state with a burning kernel (T to 2000 K at the box centre), thermo re-evaluated"""
    from dfmi import case
    species = _mech("burke9")[0]
    f = case.tgv_fields(c.m, species, kernel_radius=2.5e-3, T_hot=2000.0)
    case.init_state(c.ctx, c.m, len(species), f["T"], f["p"], f["U"], f["Y"])
    c.ctx.call("pre_time_step")
    st = case.pull_state(c.ctx, c.m, len(species))
    return st


def test_consumers():
    from dfmi import case
    from test_gpu_parity import _ell_width
    a = _ras_case({"model": 1, "mixing": 1, "chemistry": 1, "coef": {"Cmix": 100.0}})
    b = _ras_case(None)
    z = _ras_case(None, chem=0)
    m, S = a.m, a.t.S
    C = m.n_cells
    try:
        st = _hot(a)
        for x in (b, z):
            case.push_state(x.ctx, st)
        a.ctx.combustion_correct(1e-6)
        b.ctx.combustion_correct(1e-6)                    # tci.model = 0: the solve and nothing else
        RR, Q = a.ctx.get_field("RR", (S, C)), a.get("Qdot")
        assert np.abs(RR).max() > 0
        assert np.array_equal(RR, b.ctx.get_field("RR", (S, C))) and np.array_equal(Q, b.get("Qdot"))
        assert np.array_equal(a.ctx.get_field("chem_stats", (3, C)), b.ctx.get_field("chem_stats", (3, C)))
        kap = a.get("tci_kappa")
        assert 0 < kap.min() and kap.max() <= 1 and kap.min() < 0.999
        RRe, Qe = a.ctx.get_field("RR_eff", (S, C)), a.get("Qdot_eff")
        assert np.array_equal(RRe, kap[None, :] * RR) and np.array_equal(Qe, kap * Q)
        ref = R.evaluate_pasr({"k": a.k0, "epsilon": a.e0, "mu": st["mu"], "rho": st["rho"], "RR": RR, "Y": st["Y"],
                               "tci_tc": np.full(C, 0.1)}, 1, 1, R.species_idx(_mech("burke9")[0]), {"Cmix": 100.0}, T=R.LD)
        assert R.rel_error(kap, ref["tci_kappa"]).max() <= 1e-13
        # the YEqn assemblies read RR_eff: bitwise a context without chemistry whose RR is that array
        z.ctx.set_field("RR", RRe)
        W = _ell_width(m)
        sizes = {"lower": S * m.n_faces, "upper": S * m.n_faces, "diag": S * C, "source": S * C}
        for x in (a, z):
            x.ctx.assemble("Y")
        for part, n in sizes.items():
            assert np.array_equal(a.ctx.get_matrix("Y", part, n), z.ctx.get_matrix("Y", part, n)), part
        for x in (a, z):
            x.ctx.assemble("Y_ell")
        for part in ("val", "dS", "rhs"):
            n = (S - 1) * (W if part == "val" else 1) * C
            assert np.array_equal(a.ctx.get_solver_rows("Y", part, n), z.ctx.get_solver_rows("Y", part, n)), part
        z.ctx.set_field("RR", RR)                         # and the unscaled RR gives another source
        z.ctx.assemble("Y")
        assert not np.array_equal(a.ctx.get_matrix("Y", "source", S * C), z.ctx.get_matrix("Y", "source", S * C))
    finally:
        for x in (a, b, z):
            x.ctx.close()


# ------------------------------------------------------------------------------------------------ 4. full steps
STEP_FIELDS = ("T", "p", "rho", "k", "epsilon", "he")


def _fields(c):
    o = {n: c.get(n) for n in STEP_FIELDS}
    o["U"] = c.ctx.get_field("U", (3, c.m.n_cells))
    o["Y"] = c.ctx.get_field("Y", (c.t.S, c.m.n_cells))
    return o


@pytest.mark.parametrize("closure", ["PaSR", "EDC"])
def test_full_steps_match_the_injected_source(closure):
    """three dfmi_time_step calls with the closure are bitwise the steps of a twin without chemistry that is handed the
    first context's RR_eff as its RR before each step"""
    from dfmi import case
    tci = {"model": 1, "mixing": 1, "chemistry": 1, "coef": {"Cmix": 100.0}} if closure == "PaSR" else {"model": 2, "version": 2005}
    a = _ras_case(tci)
    z = _ras_case(None, chem=0)
    S, C = a.t.S, a.m.n_cells
    try:
        st = _hot(a)
        case.push_state(z.ctx, st)
        for x in (a, z):
            x.ctx.set_option("amg.reuse_steps", 1)
        moved = 0.0
        for step in range(3):
            a.ctx.time_step(2)
            RRe = a.ctx.get_field("RR_eff", (S, C))
            kap = a.get("tci_kappa")
            assert np.all((kap >= 0) & (kap <= 1)) and np.abs(RRe).max() > 0
            assert np.array_equal(RRe, kap[None, :] * a.ctx.get_field("RR", (S, C)))
            z.ctx.set_field("RR", RRe)
            z.ctx.time_step(2)
            fa, fz = _fields(a), _fields(z)
            for n in fa:
                assert np.array_equal(fa[n], fz[n]), (closure, step, n)
            moved = max(moved, float(np.abs(1 - kap).max()))
        assert moved > 1e-3                                # the closure scaled something
        if closure == "EDC":
            assert a.ctx.get_option("tci.bad_tauStar") == 0
    finally:
        a.ctx.close(); z.ctx.close()


# ------------------------------------------------------------------------------------------------ 5. nothing else moved
def test_steps_without_a_closure_are_unmoved():
    """a laminar step, an LES step and a RAS step with tci.model = 0 are bitwise the same before and after a tci.model = 1
    context lived in the process, and after the option went to 1 and back in the same context"""
    from dfmi import case, turbulence as T
    from test_gpu_parity import _case
    species, mc, nasa, W, t = _mech("burke9")
    res = {}

    def lam(tag, toggle=False):
        ctx, m, tt, st, pt, inert, dt = _case(periodic=False, mech="burke9")
        try:
            ctx.chem_set_mechanism(mc); ctx.chem_set_options(1)
            if toggle:
                ctx.set_option("tci.model", 1); ctx.set_option("tci.chemistry", 2); ctx.set_option("tci.model", 0)
            ctx.time_step(2)
            res[tag] = {n: ctx.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho")}
            res[tag]["Y"] = ctx.get_field("Y", (tt.S, m.n_cells)); res[tag]["RR"] = ctx.get_field("RR", (tt.S, m.n_cells))
        finally:
            ctx.close()

    def les(tag, toggle=False):
        ctx, m, tt, st, pt, inert, dt = _case(periodic=False, mech="burke9")
        try:
            ctx.chem_set_mechanism(mc); ctx.chem_set_options(1)
            if toggle:
                ctx.set_option("tci.model", 2); ctx.set_option("tci.model", 0)
            T.apply(ctx, m, dict(T.DEFAULTS, model=1, deltaCoeff=1.0))
            ctx.time_step(2)
            res[tag] = {n: ctx.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "nut")}
            res[tag]["Y"] = ctx.get_field("Y", (tt.S, m.n_cells))
        finally:
            ctx.close()

    def ras(tag, toggle=False):
        c = _ras_case(None)
        try:
            c.ctx.set_option("amg.reuse_steps", 1)
            st = _hot(c)
            if toggle:
                _set_tci(c.ctx, 1, R.species_idx(species), None, chemistry=2)
                c.ctx.time_step(2)                             # a step with the closure in between
                assert c.get("tci_kappa").min() < 1
                case.push_state(c.ctx, st)                     # every field of the state back, old-time ones and dpdt included
                c.ctx.set_option("tci.model", 0)
            c.set_ke(c.k0, c.e0)
            c.ctx.set_field("chem_stats", np.zeros((3, c.m.n_cells)))
            c.ctx.time_step(2)
            res[tag] = _fields(c)
            res[tag]["RR"] = c.ctx.get_field("RR", (c.t.S, c.m.n_cells))
        finally:
            c.ctx.close()

    for f, name in ((lam, "lam"), (les, "les"), (ras, "ras")):
        f(name + "0")
    c = _ras_case({"model": 1, "chemistry": 2})             # a closure context is created, steps and is destroyed
    try:
        _hot(c); c.set_ke(c.k0, c.e0); c.ctx.time_step(2)
        assert c.get("tci_kappa").min() < 1
    finally:
        c.ctx.close()
    for f, name in ((lam, "lam"), (les, "les"), (ras, "ras")):
        f(name + "1")
        f(name + "2", toggle=True)
        for tag in (name + "1", name + "2"):
            for n, v in res[name + "0"].items():
                assert np.array_equal(res[tag][n], v), (tag, n)


def test_no_closure_no_launch_no_field():
    """tci.model = 0: dfmi_combustion_correct is the solve (bitwise chem_solve's RR), no k_tci_* launch"""
    ctx, m = _ctx("gen", (8, 8, 4), ras=False)
    try:
        S = len(_mech("burke9")[0])
        T, p, rho, Y = _reacting_states("gen", m.n_cells)
        for nm, v in (("T", T), ("p", p), ("rho", rho), ("Y", Y)):
            ctx.set_field(nm, np.ascontiguousarray(v))
        ctx.chem_solve(1e-6)
        want = ctx.get_field("RR", (S, m.n_cells))
        ctx.set_field("chem_stats", np.zeros((3, m.n_cells)))
        ctx.kernel_timer("k_tci_kappa,k_tci_rates,k_tci_scale,k_chem")
        ctx.combustion_correct(1e-6)
        assert [ctx.kernel_time(k)[1] for k in ("k_tci_kappa", "k_tci_rates", "k_tci_scale", "k_chem")] == [0, 0, 0, 1]
        ctx.kernel_timer("")
        assert np.array_equal(ctx.get_field("RR", (S, m.n_cells)), want)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. validity and options
def test_validity_and_options():
    from dfmi.lib import DfmiError
    import test_tci_cpu as TC
    ctx, m = _ctx("gen", (4, 4, 4), ras=False)
    C = m.n_cells
    try:
        for key, v in TC.TCI_DEFAULTS.items():
            assert ctx.get_option(key) == v, key
        assert ctx.get_option("tci.bad_tauStar") == 0
        for key, bad, word in (("tci.model", 3, "tci.model"), ("tci.mixing", 4, "dynamicScale"), ("tci.mixing", 0, "tci.mixing"),
                               ("tci.chemistry", 0, "tci.chemistry"), ("tci.version", 2010, "tci.version"), ("tci.exp1", 5, "tci.exp1"),
                               ("tci.exp2", 2.5, "tci.exp2"), ("tci.Cmix", 0.0, "tci.Cmix"), ("tci.C1", float("nan"), "tci.C1"),
                               ("tci.Cgamma", float("inf"), "tci.Cgamma"), ("tci.fuel", 9, "tci.fuel"), ("tci.CO2", -2, "tci.CO2"),
                               ("tci.nope", 1.0, "tci.nope"), ("tci.bad_tauStar", 0.0, "tci.bad_tauStar")):
            with pytest.raises(DfmiError, match=word):
                ctx.set_option(key, bad)
        T, p, rho, Y = _reacting_states("gen", C)
        for nm, v in (("T", T), ("p", p), ("rho", rho), ("Y", Y), ("mu", 2e-5 * np.ones(C))):
            ctx.set_field(nm, np.ascontiguousarray(v))
        ctx.set_option("tci.model", 1)
        with pytest.raises(DfmiError, match="les.model.*tci.model|tci.model.*les.model"):
            ctx.set_option("les.model", 1)
        with pytest.raises(DfmiError, match="ras.model"):                       # k and epsilon exist only there
            ctx.combustion_correct(1e-6)
        ctx.set_option("ras.model", 1)
        with pytest.raises(DfmiError, match="'k'"):
            ctx.combustion_correct(1e-6)
        ctx.set_field("k", np.full(C, 30.0)); ctx.set_field("epsilon", np.full(C, 4e5))
        with pytest.raises(DfmiError, match="tci.fuel"):                        # globalConvertion without a fuel
            ctx.combustion_correct(1e-6)
        ctx.set_option("tci.fuel", 0)
        ctx.chem_set_options(0)
        with pytest.raises(DfmiError, match="chemistry mode 1"):
            ctx.combustion_correct(1e-6)
        with pytest.raises(DfmiError, match="DNN"):
            ctx.chem_set_options(2)
        ctx.chem_set_options(1)
        ctx.combustion_correct(1e-6)                                            # valid now
        for n in ("tci_kappa", "tci_tmix", "tci_tauStar", "RR_eff", "Qdot_eff"):
            with pytest.raises(DfmiError, match=n):
                ctx.set_field(n, np.zeros(C))
        # tci_tc: starts at 0.1, can be set, persists, and is reset when the model or the chemistry scale changes
        ctx.set_field("tci_tc", np.full(C, 0.25))
        assert np.array_equal(ctx.get_field("tci_tc", (C,)), np.full(C, 0.25))
        ctx.set_option("tci.Cmix", 0.3); ctx.set_option("tci.mixing", 2); ctx.set_option("tci.chemistry", 1)   # no change of the scale
        assert np.array_equal(ctx.get_field("tci_tc", (C,)), np.full(C, 0.25))
        ctx.set_option("tci.chemistry", 2)
        assert np.array_equal(ctx.get_field("tci_tc", (C,)), np.full(C, 0.1))
        ctx.set_field("tci_tc", np.full(C, 0.25))
        ctx.set_option("tci.model", 2)
        assert np.array_equal(ctx.get_field("tci_tc", (C,)), np.full(C, 0.1))
        ctx.set_option("tci.model", 0)
        with pytest.raises(DfmiError, match="tci.model"):
            ctx.assemble("tci")
        ctx.set_option("ras.model", 0); ctx.set_option("les.model", 1)
        with pytest.raises(DfmiError, match="les.model.*tci.model|tci.model.*les.model"):
            ctx.set_option("tci.model", 1)
    finally:
        ctx.close()
    fresh, m = _ctx("gen", (2, 2, 2), ras=False)
    try:
        assert np.array_equal(fresh.get_field("tci_tc", (8,)), np.full(8, 0.1))  # the start value, before any call
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 7. two ranks
_HUB = [1700]


def test_two_ranks_match_single_domain():
    """the in-process transport: a graph bisection of the sheared box against the single domain after one step"""
    import ras_reference as RR_
    from dfmi import case
    from dfmi.lib import Context
    from dfmi.partition import partition_cells, decompose
    species, mc, nasa, W, t = _mech("burke9")
    mg = RR_.get_mesh("sheared-walls")
    inert = species.index("N2")
    f = case.tgv_fields(mg, species, kernel_radius=2.5e-3, T_hot=2000.0)
    rng = np.random.default_rng(47)
    k = 30.0 * (1 + 0.5 * rng.uniform(-1, 1, mg.n_cells))
    eps = 4e5 * 10.0 ** rng.uniform(-2, 2, mg.n_cells)
    idx = R.species_idx(species)

    def run(m, g, comm=None):
        c = Context(0)
        try:
            case.setup_context(c, m, t, inert, 1e-6, case.default_patch_types(m), comm=comm, schemes={"laplacian": "corrected"})
            for e in ("U", "Y", "E", "k", "epsilon"):
                c.set_solver(e, 300, 1e-14, 1e-300)
            c.set_solver("p", 3000, 1e-14, 1e-300)
            zg = m.patch_types(0)
            c.set_patch_types("k", zg); c.set_patch_types("epsilon", zg)
            c.set_option("ras.model", 1)
            c.chem_set_mechanism(mc); c.chem_set_options(1, rtol=1e-8, atol=1e-14)
            _set_tci(c, 1, idx, None, mixing=3, chemistry=1)
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            for n, v in (("k", k[g]), ("epsilon", eps[g])):
                c.set_field(n, np.ascontiguousarray(v))
                c.set_field("boundary_" + n, case.boundary_values(m, v).reshape(-1))
            c.call("pre_time_step")
            c.time_step(2)
            return {"tci_kappa": c.get_field("tci_kappa", (m.n_cells,)), "RR_eff": c.get_field("RR_eff", (t.S, m.n_cells)),
                    "Y": c.get_field("Y", (t.S, m.n_cells))}
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
    for n in ("tci_kappa", "RR_eff", "Y"):
        a = np.zeros((ref[n].reshape(-1, mg.n_cells).shape[0], mg.n_cells))
        for r in range(nr):
            a[:, meshes[r].cell_map] = out[r][n].reshape(a.shape[0], -1)
        w = ref[n].reshape(a.shape)
        e = np.abs(a - w).max() / np.abs(w).max()
        print("two ranks vs single domain", n, f"{e:.2e}")
        assert e < 1e-9, (n, e)
    assert ref["tci_kappa"].min() < 0.999 and np.abs(ref["RR_eff"]).max() > 0
