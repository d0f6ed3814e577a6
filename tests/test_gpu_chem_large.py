"""The cooperative stiff-chemistry kernel (k_chem_coop, 13..64 species; chem.coop = 1 forces it below) on DRM19
(21 species / 84 reactions) and the 36-species gri30 (219 reactions).

The oracle (SciPy BDF in Python) costs seconds per cell on these mechanisms, so its rates for 48 states per mechanism
are a fixture (tests/golden/chem_large_states.json, made by tests/golden/make_chem_large_fixtures.py, which also
checked every state against a 100x looser oracle run); the meshes tile those states over their cells. Thresholds
against the oracle are those of test_gpu_chemistry.py::test_chem_rr_matches_oracle."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

H2_MECHS = [("Burke2012_s9r23.yaml", "thermo_Burke2012_s9r23.txt"), ("ES80_H2-7-16.yaml", "thermo_ES80_H2-7-16.txt")]
_FIX = {}


def _fixture(name):
    if not _FIX:
        _FIX.update(json.load(open(os.path.join(GOLDEN, "chem_large_states.json")))["mechanisms"])
    f = _FIX[name]
    return f, np.asarray(f["T"]), np.asarray(f["p"]), np.asarray(f["rho"]), np.asarray(f["Y"]), np.asarray(f["RR"])


def _setup(mech_file, table_file, n):
    from dfmi.mesh import hex_box
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi.kinetics import parse_mechanism
    from dfmi.lib import Context
    from dfmi import case
    ym = read_yaml_mechanism(os.path.join(GOLDEN, mech_file))
    t = read_thermo_table(os.path.join(GOLDEN, table_file), ym["species"])
    mech = parse_mechanism(os.path.join(GOLDEN, mech_file))
    m = hex_box(*n)
    ctx = Context(0)
    case.setup_context(ctx, m, t, ym["species"].index("N2"), 1e-6)
    ctx.chem_set_mechanism(mech)
    return ctx, m, ym, mech


def _tiled(name, n):
    """context on an n box of mechanism `name` with the fixture states tiled over the cells"""
    f, T, p, rho, Y, RR = _fixture(name)
    ctx, m, ym, mc = _setup(f["mechanism"], f["thermo"], n)
    idx = np.arange(m.n_cells) % T.size
    ctx.set_field("T", T[idx]); ctx.set_field("p", p[idx]); ctx.set_field("rho", rho[idx]); ctx.set_field("Y", Y[:, idx])
    return ctx, m, mc, idx, RR


def _h2_states(ym, n, seed=0):
    """_states of test_gpu_chemistry.py"""
    rng = np.random.default_rng(seed)
    sp = ym["species"]
    from dfmi.case import h2_air_compositions
    yu, yb = h2_air_compositions(sp)
    prog = rng.random(n)
    Y = (1 - prog) * yu[:, None] + prog * yb[:, None]
    Y = Y + rng.random((len(sp), n)) * 1e-3
    Y /= Y.sum(axis=0)
    T = 300.0 + 2200.0 * rng.random(n)
    Wm = 1.0 / (Y / ym["W"][:, None]).sum(axis=0)
    p = 101325.0 * (1.0 + 0.05 * rng.standard_normal(n))
    rho = p * Wm / (8314.46261815324 * T) * (1.0 + 0.02 * rng.standard_normal(n))
    return T, p, rho, Y


@pytest.mark.parametrize("name", ["drm19", "gri30"])
def test_chem_large_rr_matches_oracle(name):
    """75 cells: the last workgroup is ragged at 2 and 4 cells per workgroup."""
    ctx, m, mc, idx, RR = _tiled(name, (5, 5, 3))
    C = m.n_cells
    ref = RR[:, idx]
    scale = np.maximum(np.abs(RR).max(axis=1, keepdims=True), 1e-3 * np.abs(RR).max())
    dt = 1e-6
    ctx.chem_set_options(1, rtol=1e-8, atol=1e-14)
    ctx.chem_solve(dt)
    assert ctx.chem_info() == -1                                  # the cooperative kernel ran
    assert ctx.get_field("chem_stats", (3, C))[0].min() >= 1      # no cell hit the step limit
    rr = ctx.get_field("RR", (mc.S, C))
    assert np.all(np.isfinite(rr))
    e_glob = np.abs(rr - ref).max() / scale.max()
    e_spec = (np.abs(rr - ref) / scale).max()
    print(f"{name}: tight {e_glob:.3e} of the global scale, {e_spec:.3e} of the per-species scale")
    assert e_glob < 1e-5
    assert e_spec < 1e-4
    assert np.abs(rr.sum(axis=0)).max() < 1e-9 * np.abs(rr).max()     # mass conservation
    ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
    ctx.chem_solve(dt)
    rr = ctx.get_field("RR", (mc.S, C))
    e_spec = (np.abs(rr - ref) / scale).max()
    print(f"{name}: default tolerances {e_spec:.3e} of the per-species scale")
    assert e_spec < 2e-3
    assert ctx.get_field("chem_stats", (3, C))[0].min() >= 1
    ctx.close()


@pytest.mark.parametrize("mech", H2_MECHS)
def test_chem_coop_matches_register_kernels(mech):
    """chem.coop = 1 against the one-cell-per-lane kernels on the hydrogen mechanisms; Qdot is the ordered sum."""
    from chem_oracle import hf298_per_mass, heat_release
    ctx, m, ym, mc = _setup(*mech, (8, 8, 4))
    C = m.n_cells
    T, p, rho, Y = _h2_states(ym, C)
    ctx.set_field("T", T); ctx.set_field("p", p); ctx.set_field("rho", rho); ctx.set_field("Y", Y)
    ctx.chem_set_options(1, rtol=1e-8, atol=1e-14)
    out = {}
    for coop in (1, 0):
        ctx.set_option("chem.coop", coop)
        ctx.set_field("chem_stats", np.zeros((3, C)))
        ctx.chem_solve(1e-6)
        info = ctx.chem_info()
        assert info == -1 if coop else info in (1, 2)
        assert ctx.get_field("chem_stats", (3, C))[0].min() >= 1
        out[coop] = (ctx.get_field("RR", (mc.S, C)), ctx.get_field("Qdot", (C,)))
    scale = np.abs(out[0][0]).max()
    d = np.abs(out[1][0] - out[0][0]).max() / scale
    print(f"{mech[0]}: |RR_coop - RR_reg| = {d:.3e} of the scale")
    assert d < 2e-5
    hc = hf298_per_mass(ym["nasa"], ym["W"])
    for coop in (1, 0):
        q = heat_release(hc, out[coop][0])
        assert np.abs(out[coop][1] - q).max() <= 1e-12 * np.abs(q).max()
    ctx.close()


def test_chem_large_mixed_workgroups():
    """Cells below T_min between hot ones: exactly zero RR and statistics, and the hot cells' bits do not depend on
    what their neighbours in the workgroup do."""
    ctx, m, mc, idx, _ = _tiled("drm19", (5, 5, 3))
    C = m.n_cells
    T = np.maximum(ctx.get_field("T", (C,)), 1200.0)
    cold = np.arange(C) % 3 == 0
    ctx.chem_set_options(1, rtol=1e-6, atol=1e-10, T_min=600.0)
    out = []
    for Tc in (400.0, 1500.0):
        Tr = T.copy()
        Tr[cold] = Tc
        ctx.set_field("T", Tr)
        ctx.set_field("chem_stats", np.zeros((3, C)))
        ctx.chem_solve(1e-6)
        out.append((ctx.get_field("RR", (mc.S, C)), ctx.get_field("chem_stats", (3, C))))
    rr, st = out[0]
    assert np.all(rr[:, cold] == 0.0) and np.all(st[:2, cold] == 0.0)
    assert st[0, ~cold].min() >= 1 and np.abs(rr[:, ~cold]).max() > 0
    assert out[1][1][0, cold].min() >= 1                         # the same cells, hot, did integrate
    assert np.array_equal(rr[:, ~cold], out[1][0][:, ~cold])
    assert np.array_equal(st[:, ~cold], out[1][1][:, ~cold])
    ctx.close()


def test_chem_large_order_independent():
    """Cost-binned launch order (three binning tiles, the last one ragged): bitwise the natural order."""
    ctx, m, mc, idx, _ = _tiled("drm19", (24, 24, 16))
    C = m.n_cells
    ctx.chem_set_options(1)
    out = {}
    for flag in (0, 1, 2):
        ctx.set_option("chem.binning", flag)
        ctx.set_field("chem_stats", np.zeros((3, C)))   # same start: no carried step sizes
        ctx.chem_solve(1e-6)
        ctx.chem_solve(1e-6)
        assert ctx.chem_info() == -1
        out[flag] = (ctx.get_field("RR", (mc.S, C)), ctx.get_field("chem_stats", (3, C))[:2])
    st = out[1][1]
    assert st[0].min() >= 1 and (st[0] + st[1]).max() > (st[0] + st[1]).min()   # costs really differ
    for f in (1, 2):
        assert np.array_equal(out[0][0], out[f][0])
        assert np.array_equal(out[0][1], out[f][1])
    ctx.close()


def test_chem_large_step_limit():
    """Cells that run out of steps leave their wave early while others go on: the call fails with the step-limit
    error, returns (no deadlock), and a sufficient budget clears it."""
    from dfmi.lib import DfmiError
    ctx, m, mc, idx, _ = _tiled("drm19", (5, 5, 3))
    C = m.n_cells
    easy = np.arange(C) % 5 == 0                    # pure N2: nothing reacts, one step covers dt
    Y = ctx.get_field("Y", (mc.S, C))
    Y[:, easy] = 0.0
    Y[mc.species.index("N2"), easy] = 1.0
    ctx.set_field("Y", Y)
    ctx.chem_set_options(1, rtol=1e-10, atol=1e-16)
    ctx.chem_set_max_steps(1)
    ctx.set_field("chem_stats", np.zeros((3, C)))
    with pytest.raises(DfmiError, match="step limit"):
        ctx.chem_solve(1e-6)
    st = ctx.get_field("chem_stats", (3, C))
    assert (st[0] < 0).any()
    assert np.all(st[0, easy] == 1) and np.all((st[0] == 1) | (st[0] < 0))   # the other cells finished (in their one step)
    ctx.chem_set_max_steps(100000)
    ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
    ctx.set_field("chem_stats", np.zeros((3, C)))
    ctx.chem_solve(1e-6)                             # a sufficient budget clears the error
    assert ctx.get_field("chem_stats", (3, C))[0].min() >= 1
    ctx.close()


def test_chem_large_refuses_extrapolation():
    from dfmi.lib import DfmiError
    ctx, m, mc, idx, _ = _tiled("drm19", (5, 5, 3))
    ctx.chem_set_options(1)
    ctx.set_option("chem.method", 1)
    with pytest.raises(DfmiError, match="extrapolation is not available above 12 species"):
        ctx.chem_solve(1e-6)
    ctx.set_option("chem.method", 0)
    ctx.chem_solve(1e-6)
    ctx.close()


def test_chem_large_refuses_65_species():
    from dfmi.lib import Context, DfmiError
    from dfmi.mech import ThermoTable, read_thermo_table, read_yaml_mechanism
    from dfmi.mesh import hex_box
    from dfmi import case
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "gri30.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_gri30_36.txt"), ym["species"])
    i = np.arange(65) % t.S
    t65 = ThermoTable([f"{t.species[k]}_{n}" for n, k in enumerate(i)], t.W[i].copy(), t.nasa[i].copy(), t.visc[i].copy(),
                      t.cond[i].copy(), t.bdiff[np.ix_(i, i)].copy())
    ctx = Context(0)
    with pytest.raises(DfmiError, match="species"):
        case.setup_context(ctx, hex_box(4, 4, 4), t65, 64, 1e-6)
    ctx.close()


def test_chem_large_in_time_step():
    """mode 1 with DRM19 inside dfmi_time_step: the step stays finite and the chemistry did something."""
    from dfmi import case
    f = _fixture("drm19")[0]
    ctx, m, ym, mc = _setup(f["mechanism"], f["thermo"], (8, 8, 4))
    sp = ym["species"]
    g = case.tgv_fields(m, sp, kernel_radius=1.5e-3, T_hot=2000.0)
    prog = (g["T"] - 300.0) / (2000.0 - 300.0)
    yu, yb = case.ch4_air_compositions(sp)
    Y = (1 - prog)[None, :] * yu[:, None] + prog[None, :] * (0.5 * (yu + yb))[:, None]   # half-burnt hot kernel
    case.init_state(ctx, m, len(sp), g["T"], g["p"], g["U"], Y)
    ctx.chem_set_options(1)
    ctx.call("pre_time_step")
    ctx.time_step(2)
    assert ctx.chem_info() == -1
    RR = ctx.get_field("RR", (mc.S, m.n_cells))
    T = ctx.get_field("T", (m.n_cells,))
    Yn = ctx.get_field("Y", (mc.S, m.n_cells))
    assert np.all(np.isfinite(RR)) and np.abs(RR).max() > 0 and np.all(np.isfinite(T)) and np.all(np.isfinite(Yn))
    ctx.close()


def test_chem_large_zero_d_trajectory():
    """dfmi_zero_d_step with DRM19 through ignition against tests/golden/zeroD_drm19.json, within
    test_gpu_zero_d.py's tolerances (T 2e-5 relative, species 2e-3 of their trajectory maximum).

    The integrator runs at rtol 1e-8 / atol 1e-16 (the RR test's tight rtol, a smaller atol), not at test_gpu_zero_d.py's 1e-12:
    a third-order method pays (1e4)^(1/3) ~ 20x the steps for the difference, on 60 sequential solves. At that pair
    RR is within 1e-5 of its scale (the RR test's bound), which moves the ignition time of 46 us by at most that
    fraction, 5e-10 s; at the trajectory's steepest slope (126 K per 1e-6 s) that is 0.06 K, 2e-5 of 2800 K -- the
    bound itself, reached only if every step erred by the full 1e-5 in the same direction."""
    from dfmi.mesh import hex_box
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi.kinetics import parse_mechanism
    from dfmi.lib import Context
    from dfmi import case
    ref = json.load(open(os.path.join(GOLDEN, "zeroD_drm19.json")))
    ym = read_yaml_mechanism(os.path.join(GOLDEN, ref["mechanism"]))
    sp = ym["species"]
    t = read_thermo_table(os.path.join(GOLDEN, ref["thermo"]), sp)
    m = hex_box(2, 2, 2, lengths=(5e-3,) * 3, periodic=(False,) * 3)
    ctx = Context(0)
    case.setup_context(ctx, m, t, sp.index("N2"), ref["dt"])
    ctx.chem_set_mechanism(parse_mechanism(os.path.join(GOLDEN, ref["mechanism"])))
    ctx.chem_set_options(1, rtol=1e-8, atol=1e-16)
    C = m.n_cells
    Y0 = np.repeat(np.asarray(ref["Y0"])[:, None], C, axis=1)
    case.init_state(ctx, m, t.S, np.full(C, ref["T0"]), np.full(C, ref["p"]), np.zeros((3, C)), Y0)
    Tref = np.asarray(ref["T"])
    Yref = np.asarray(ref["Y"])
    n = ref["n_steps"]
    T = np.zeros(n + 1); Y = np.zeros((n + 1, t.S))
    T[0] = ref["T0"]; Y[0] = ref["Y0"]
    for k in range(1, n + 1):
        ctx.zero_d_step(ref["dt"], 1)
        Tc = ctx.get_field("T", (C,))
        assert np.ptp(Tc) <= 1e-12 * Tc[0]        # identical reactors stay identical
        T[k] = Tc[0]
        Y[k] = ctx.get_field("Y", (t.S, C))[:, 0]
    assert ctx.chem_info() == -1
    assert Tref.max() - Tref[0] > 500.0           # the oracle trajectory ignites inside the window
    eT = np.abs(T - Tref).max() / Tref.max()
    scale = np.maximum(np.abs(Yref).max(axis=0), 1e-12)
    eY = (np.abs(Y - Yref).max(axis=0) / scale).max()
    print(f"zero-D DRM19: T {eT:.3e} relative, species {eY:.3e} of their maximum")
    assert eT < 2e-5, np.abs(T - Tref).max()
    assert eY < 2e-3
    ctx.close()
