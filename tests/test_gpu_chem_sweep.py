"""The stiff-chemistry kernels of csrc/chem.hip at every species count and reaction form (MI355X; DESIGN 6b has the
coverage table).

Mechanisms come from tests/chem_mechs.py: gri30 restricted to its first S species (S = 4..12 on the register kernels
k_chem<S>, 13, 16, 17, 32, 33 on the cooperative kernel), 63- and 64-species clones, and one-reaction mechanisms of every
reaction form. States, oracle rates and the fp64-against-long-double errors of the reference are the fixture
tests/golden/chem_sweep_states.json (make_chem_sweep_fixtures.py): 16 states per mechanism at 0.1..32 atm, four of them
with half the species at 0 or at -1e-12, tiled over 75 cells (a ragged last workgroup at 1, 2, 4 and 64 cells per
workgroup).

Bounds: against the oracle those of test_gpu_chemistry.py::test_chem_rr_matches_oracle (TIGHT_GLOBAL, TIGHT_SPECIES,
LOOSE_SPECIES, MASS, and Qdot to 1e-12); cooperative against register kernel the 2e-5 of
test_gpu_chem_large.py::test_chem_coop_matches_register_kernels; the reactionRate scale per cell against long double at
4x the fixture's measured fp64 error, floored at 1e-13 (the rule of tci_reference.gpu_bound). Nothing measured on a kernel
feeds a bound.
"""
import json
import os

import numpy as np
import pytest

import chem_mechs as cm
import tci_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TIGHT_GLOBAL, TIGHT_SPECIES, LOOSE_SPECIES, MASS, QDOT = 1e-5, 1e-4, 2e-3, 1e-9, 1e-12
COOP_VS_REGISTER = 2e-5
STEP_RATIO = 0.05          # a missing fall-off term in a Jacobian costs 2-5x the steps; rounding costs none
DT = 1e-6
BOX = (5, 5, 3)
SMALL = [f"p{S}" for S in range(4, 13)]
REFUSED_LANES = {("c63", 16), ("c64", 16)}      # 4 cells x 47 KB of LDS per workgroup
_FIX, _LD = {}, {}


def _fixture():
    if not _FIX:
        _FIX.update(json.load(open(os.path.join(GOLDEN, "chem_sweep_states.json"))))
    return _FIX


def _case(name):
    f = _fixture()["cases"][name]
    mt = cm.case(name)
    assert list(mt[0].species) == f["species"] and mt[0].R == f["R"]
    return mt, {k: np.asarray(f[k]) for k in ("T", "p", "rho", "Y", "RR")}


def _ctx(mt, n=BOX, ras=False):
    from dfmi import case
    from dfmi.lib import Context
    from dfmi.mesh import hex_box
    mesh = hex_box(*n)
    ctx = Context(0)
    case.setup_context(ctx, mesh, mt[3], cm.inert_index(mt[0]), DT)
    ctx.chem_set_mechanism(mt[0])
    ctx.chem_set_options(1, rtol=1e-8, atol=1e-14)
    if ras:
        ctx.set_option("ras.model", 1)
    return ctx, mesh.n_cells


def _tile(ctx, C, st, perm=None):
    idx = np.arange(C) % st["T"].size
    Y = st["Y"] if perm is None else st["Y"][perm]
    for n, v in (("T", st["T"][idx]), ("p", st["p"][idx]), ("rho", st["rho"][idx]), ("Y", Y[:, idx])):
        ctx.set_field(n, np.ascontiguousarray(v))
    ref = st["RR"] if perm is None else st["RR"][perm]
    return ref[:, idx]


def _solve(ctx, S, C, dt=DT):
    ctx.set_field("chem_stats", np.zeros((3, C)))       # no carried step sizes
    ctx.chem_solve(dt)
    return {"RR": ctx.get_field("RR", (S, C)), "Qdot": ctx.get_field("Qdot", (C,)), "stats": ctx.get_field("chem_stats", (3, C))}


def _same(a, b, what):
    for q in ("RR", "Qdot", "stats"):
        assert np.array_equal(a[q], b[q]), (what, q, np.abs(a[q] - b[q]).max())


def _against_oracle(label, ctx, mt, C, ref, info, repeat=False):
    """the thresholds of test_chem_rr_matches_oracle at both tolerance pairs -> (tight result, default-tolerance result).
    repeat: the solve at the default tolerances runs twice and must repeat bitwise (the tight one costs six times the
    steps and runs the same code)"""
    from chem_oracle import heat_release, hf298_per_mass
    S = mt[0].S
    scale = np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1e-3 * np.abs(ref).max())
    hc = hf298_per_mass(mt[1], mt[2])
    out = None
    for rtol, atol in ((1e-8, 1e-14), (1e-6, 1e-10)):
        ctx.chem_set_options(1, rtol=rtol, atol=atol)
        a = _solve(ctx, S, C)
        assert ctx.chem_info() == info
        if repeat and out is not None:
            _same(a, _solve(ctx, S, C), f"{label}: two runs")
        rr = a["RR"]
        assert np.all(np.isfinite(rr)) and a["stats"][0].min() >= 1
        e_glob = np.abs(rr - ref).max() / scale.max()
        e_spec = (np.abs(rr - ref) / scale).max()
        e_mass = np.abs(rr.sum(axis=0)).max() / np.abs(rr).max()
        q = heat_release(hc, rr)
        e_q = np.abs(a["Qdot"] - q).max() / np.abs(q).max()
        print(f"{label} rtol {rtol:g}: {e_glob:.3e} global, {e_spec:.3e} per species, sum RR {e_mass:.1e}, Qdot {e_q:.1e}, "
              f"steps {int(a['stats'][:2].sum())}")
        if out is None:
            assert e_glob < TIGHT_GLOBAL and e_spec < TIGHT_SPECIES
            out = a
        else:
            assert e_spec < LOOSE_SPECIES
        assert e_mass < MASS and e_q <= QDOT
    return out, a


# ------------------------------------------------------------------------------------------- a. register kernels
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("name", SMALL)
def test_register_kernel(name, method):
    """k_chem<S> at every S = 4..12: ROS3 (chem.generated = 0) and the chem.method = 1 extrapolation"""
    mt, st = _case(name)
    ctx, C = _ctx(mt)
    try:
        ctx.set_option("chem.generated", 0)
        ctx.set_option("chem.method", method)
        _against_oracle(f"{name} register method {method}", ctx, mt, C, _tile(ctx, C, st), 0, repeat=True)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------- b. the same, cooperative
@pytest.mark.parametrize("name", SMALL)
def test_coop_below_13(name):
    """chem.coop = 1 (16 lanes, one row per lane) on the nine small mechanisms: the oracle, the register kernel, and the
    step counts of the two independently written Jacobians"""
    mt, st = _case(name)
    ctx, C = _ctx(mt)
    try:
        ctx.set_option("chem.generated", 0)
        ref = _tile(ctx, C, st)
        ctx.set_option("chem.coop", 1)
        co, _ = _against_oracle(f"{name} coop", ctx, mt, C, ref, -1, repeat=True)
        ctx.set_option("chem.coop", 0)
        ctx.chem_set_options(1, rtol=1e-8, atol=1e-14)
        reg = _solve(ctx, mt[0].S, C)
        assert ctx.chem_info() == 0
        d = np.abs(co["RR"] - reg["RR"]).max() / np.abs(reg["RR"]).max()
        n_co, n_reg = co["stats"][:2].sum(), reg["stats"][:2].sum()
        print(f"{name}: |RR_coop - RR_reg| = {d:.3e} of the scale; steps coop {int(n_co)} register {int(n_reg)} ratio {n_co / n_reg:.4f}")
        assert d < COOP_VS_REGISTER
        assert abs(n_co / n_reg - 1.0) <= STEP_RATIO
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------- c. cooperative, 13..64
@pytest.mark.parametrize("name", cm.LARGE)
def test_coop_large(name):
    """k_chem_coop at the lane-count boundaries (S = 13, 16 | 17, 32 | 33, 63, 64) against the oracle, and bitwise the same
    RR, Qdot and statistics at 16, 32 and 64 lanes per cell (at the default tolerances): every sum has one order inside one
    lane"""
    from dfmi.lib import DfmiError
    mt, st = _case(name)
    S = mt[0].S
    ctx, C = _ctx(mt)
    try:
        _, base = _against_oracle(f"{name} coop", ctx, mt, C, _tile(ctx, C, st), -1)
        for lanes in (16, 32, 64):
            ctx.set_option("chem.coop_lanes", lanes)
            if (name, lanes) in REFUSED_LANES:
                with pytest.raises(DfmiError, match="LDS"):
                    _solve(ctx, S, C)
                continue
            a = _solve(ctx, S, C)
            assert ctx.chem_info() == -1
            _same(a, base, f"{name}: {lanes} lanes against the default")
        ctx.set_option("chem.coop_lanes", 0)
        _same(_solve(ctx, S, C), base, f"{name}: default again")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------- d. species order
@pytest.mark.parametrize("name,coop", [("p12", 0), ("p12", 1), ("p16", 1), ("p33", 1), ("c64", 1)])
def test_species_reversed(name, coop):
    """the species in reverse order: the un-pivoted LUs eliminate in another order"""
    mt, st = _case(name)
    perm = np.arange(mt[0].S)[::-1]
    pt = cm.permuted(mt, perm)
    ctx, C = _ctx(pt)
    try:
        ctx.set_option("chem.generated", 0)
        ctx.set_option("chem.coop", coop)
        _against_oracle(f"{name} reversed coop {coop}", ctx, pt, C, _tile(ctx, C, st, perm), -1 if coop else 0)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------- e. rates pointwise
def _tci_fields(ctx, mt, T, p, rho, Y):
    n = T.size
    st = R.broad(n, mt[0].S, mt[2])              # mu, k, epsilon, RR, Qdot: read by the passes, not by the reactionRate scale
    st.update({"T": T, "p": p, "rho": rho, "Y": Y})
    for q in ("T", "p", "rho", "mu", "k", "epsilon", "Y", "RR", "Qdot", "tci_tc"):
        ctx.set_field(q, np.ascontiguousarray(st[q]))
    for k, v in R.DEFAULTS.items():
        ctx.set_option("tci." + k, v)
    for k in R.IDX_NAMES:
        ctx.set_option("tci." + k, -1)
    ctx.set_option("tci.mixing", 1)
    ctx.set_option("tci.chemistry", 3)
    ctx.set_option("tci.model", 1)


def _tc_ld(key, mt, T, p, rho, Y):
    if key not in _LD:
        _LD[key] = R.tc_reaction(mt[0], mt[1], mt[2], T, p, rho, Y, T=R.LD)
    return _LD[key]


def _hold_tc(ctx, C, ref, bound, what):
    runs = []
    for _ in range(2):
        ctx.assemble("tci")
        runs.append(ctx.get_field("tci_tc", (C,)))
    assert np.array_equal(runs[0], runs[1]), (what, "two runs")
    e = R.rel_error(runs[0], ref)
    worst = float(np.nanmax(e, initial=0.0))
    print(f"{what}: {worst:.3e} (bound {bound:.1e})")
    assert np.all(np.isfinite(e)) and worst <= bound, (what, worst, bound, np.flatnonzero(~(e <= bound))[:8])
    return runs[0]


@pytest.mark.parametrize("name", list(cm.SWEEP))
def test_tci_rates_sweep(name):
    """k_tci_rates<S> at every S = 4..12 and k_tci_rates_coop at 16, 32 and 64 lanes: tci_tc per cell against long double"""
    from dfmi.lib import DfmiError
    mt, st = _case(name)
    bound = max(4.0 * _fixture()["cases"][name]["tc_fp64_error"], 1e-13)
    ctx, C = _ctx(mt, ras=True)
    try:
        idx = np.arange(C) % st["T"].size
        _tci_fields(ctx, mt, st["T"][idx], st["p"][idx], st["rho"][idx], np.ascontiguousarray(st["Y"][:, idx]))
        ref = _tc_ld(name, mt, st["T"], st["p"], st["rho"], st["Y"])[idx]
        if name == "p12x58":      # 3 R x 64 lanes x 8 B = 89 KB of rate constants: the per-lane kernel's host check refuses
            with pytest.raises(DfmiError, match="tci reactionRate: mechanism too large for the LDS layout"):
                ctx.assemble("tci")
        else:
            _hold_tc(ctx, C, ref, bound, f"{name} tci_tc")
        if mt[0].S <= 12:
            ctx.set_option("chem.coop", 1)
            _hold_tc(ctx, C, ref, bound, f"{name} tci_tc coop")
    finally:
        ctx.close()


@pytest.mark.parametrize("key", [k for k, _ in cm.single_variants()])
def test_tci_rates_single(key):
    """one reaction of each form on 256 states over T 300..3000 K and every fall-off regime, per-lane and cooperative. With
    R = 1 the scale is a function of that reaction's forward and reverse rates of progress: the irreversible variant pins
    the forward rate, the reversible one then 1 / Kc."""
    mt = dict(cm.single_variants())[key]
    bound = max(4.0 * _fixture()["singles"][key]["tc_fp64_error"], 1e-13)
    T, p, rho, Y = cm.single_states(mt)
    ref = _tc_ld(key, mt, T, p, rho, Y)
    C = T.size
    assert ref[C - 1] == R.VGREAT and (ref[:C - 1] < 1e200).sum() > 240          # pure inert: every rate is 0
    if not mt[0].reversible[0]:
        assert ref[1] == R.VGREAT                                              # its first reactant is exactly 0
    ctx, Cm = _ctx(mt, n=(4, 8, 8), ras=True)
    assert Cm == C
    try:
        _tci_fields(ctx, mt, T, p, rho, Y)
        for coop in (0, 1):
            ctx.set_option("chem.coop", coop)
            got = _hold_tc(ctx, C, ref, bound, f"{key} coop {coop}")
            assert np.array_equal(got == R.VGREAT, np.asarray(ref == R.VGREAT))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------- f. per-cell interval
@pytest.mark.parametrize("name", ["p4", "p12", "p13", "c64"])
def test_per_cell_interval_sweep(name):
    """k_chem<S, const double*> at S = 4 and 12 and k_chem_coop<., ., const double*> at 16 and 64 lanes: the "one value
    everywhere" and "five values shuffled" parts of test_gpu_tci.py::test_per_cell_interval, bitwise against the scalar
    solve of a twin context"""
    mt, st = _case(name)
    S = mt[0].S
    ctx, C = _ctx(mt, ras=True)
    twin, _ = _ctx(mt)
    try:
        idx = np.arange(C) % st["T"].size
        one = np.ones(C)
        for x in (ctx, twin):
            x.set_option("chem.generated", 0)
            x.chem_set_options(1, rtol=1e-6, atol=1e-10)      # bitwise comparisons: the default tolerances do
            for q, v in (("T", st["T"][idx]), ("p", st["p"][idx]), ("rho", one), ("Y", st["Y"][:, idx])):
                x.set_field(q, np.ascontiguousarray(v))
        mu = 2e-5 * one                                   # nu = mu / (rho + small): the same bits in every cell
        ctx.set_field("mu", mu); ctx.set_field("k", 30.0 * one)
        for k, v in R.DEFAULTS.items():
            ctx.set_option("tci." + k, v)
        for k in R.IDX_NAMES:
            ctx.set_option("tci." + k, -1)
        ctx.set_option("tci.version", 2005)
        ctx.set_option("tci.model", 2)
        eps5 = 2e-5 * R.DEFAULTS["Ctau"] ** 2 / np.array([1e-7, 3e-7, 1e-6, 4e-6, 1e-5]) ** 2
        zeros = np.zeros((3, C))

        def edc(eps, stats):
            ctx.set_field("epsilon", eps); ctx.set_field("chem_stats", stats)
            ctx.combustion_correct(DT)                    # dt is not read: every cell has its own interval
            return {"RR": ctx.get_field("RR", (S, C)), "Qdot": ctx.get_field("Qdot", (C,)), "stats": ctx.get_field("chem_stats", (3, C)),
                    "tau": ctx.get_field("tci_tauStar", (C,)), "bad": ctx.get_option("tci.bad_tauStar")}

        def scalar(dt, stats):
            twin.set_field("chem_stats", stats)
            twin.chem_solve(dt)
            return {"RR": twin.get_field("RR", (S, C)), "Qdot": twin.get_field("Qdot", (C,)), "stats": twin.get_field("chem_stats", (3, C))}

        a = edc(eps5[2] * one, zeros)
        tau = np.unique(a["tau"])
        assert tau.size == 1 and 0.5e-6 < tau[0] < 2e-6 and a["bad"] == 0
        _same(a, scalar(float(tau[0]), zeros), f"{name}: uniform")
        assert np.abs(a["RR"]).max() > 0 and a["stats"][0].min() >= 1
        pick = np.random.default_rng(3).integers(0, 5, C)
        d = edc(eps5[pick], zeros)
        taus = np.unique(d["tau"])
        assert d["bad"] == 0 and taus.size == 5 and taus[-1] / taus[0] > 90
        for v in taus:
            sel = d["tau"] == v
            assert sel.sum() > 3
            u = scalar(float(v), zeros)
            for q in ("RR", "Qdot", "stats"):
                assert np.array_equal(d[q][..., sel], u[q][..., sel]), (name, v, q)
    finally:
        ctx.close(); twin.close()


# ------------------------------------------------------------------------------------------- g. LDS edges, refusals
def test_register_kernel_largest_lds():
    """58 reactions at 12 species: (3 R + S^2) x 64 x 8 B = 162,816 B of dynamic LDS, the largest request k_chem accepts"""
    mt, st = _case("p12x58")
    assert (3 * mt[0].R + mt[0].S ** 2) * 64 * 8 == 162816
    ctx, C = _ctx(mt)
    try:
        _against_oracle("p12x58 register", ctx, mt, C, _tile(ctx, C, st), 0)
    finally:
        ctx.close()


def test_register_kernel_refuses_59_reactions():
    from dfmi.lib import DfmiError
    mt = cm.with_duplicates(cm.case("p12"), 59)
    _, st = _case("p12")
    ctx, C = _ctx(mt)
    try:
        _tile(ctx, C, st)
        ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
        with pytest.raises(DfmiError, match="too large for the LDS layout"):
            ctx.chem_solve(DT)
        ctx.set_option("chem.coop", 1)                   # the cooperative layout holds it
        assert _solve(ctx, 12, C)["stats"][0].min() >= 1
    finally:
        ctx.close()


def test_coop_refusals_at_13():
    """a lane count that is no wave divisor the kernel is built for, and the extrapolation method above 12 species"""
    from dfmi.lib import DfmiError
    mt, st = _case("p13")
    ctx, C = _ctx(mt)
    try:
        _tile(ctx, C, st)
        ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
        ctx.set_option("chem.coop_lanes", 8)
        with pytest.raises(DfmiError, match="chem.coop_lanes"):
            ctx.chem_solve(DT)
        ctx.set_option("chem.coop_lanes", 0)
        ctx.set_option("chem.method", 1)
        with pytest.raises(DfmiError, match="extrapolation is not available above 12 species"):
            ctx.chem_solve(DT)
        ctx.set_option("chem.method", 0)
        assert _solve(ctx, 13, C)["stats"][0].min() >= 1
    finally:
        ctx.close()
