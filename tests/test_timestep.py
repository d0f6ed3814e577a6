"""Adjustable time step without a GPU (dfLowMachFoam.C:261-262): the step-size rules of dfmi.timestep against
hand-computed numbers, the controlDict reader, the three new entries at the C-ABI boundary, and CPU-A's
implementation of them -- its Courant number against the NumPy restatement (tests/courant_reference.py) and a step
after dfmi_set_delta_t against the oracle at the new step size."""
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, rel_err
import courant_reference as CR

CPU_A = os.path.join(ROOT, "baseline", "cpu_a", "libdfmi_cpu_a.so")
ENTRIES = ("dfmi_courant_no", "dfmi_set_delta_t", "dfmi_get_delta_t")


# ------------------------------------------------------------------ controller (setInitialDeltaT.H, setDeltaT.H)
# the small guard (1e-15 added to Co) moves a result by at most 1e-15 / Co relative: 1e-12 separates every branch
def _close(a, b):
    return a == pytest.approx(b, rel=1e-12, abs=0.0)


def test_next_delta_t_zero_courant_number_grows_by_the_cap():
    from dfmi.timestep import next_delta_t
    # f = 0.5 / 1e-15 = 5e14, 1 + 0.1 f = 5e13 + 1, capped at 1.2
    assert next_delta_t(1e-6, 0.0, 0.5, 1e-4) == 1.2 * 1e-6


def test_next_delta_t_far_below_max_co_grows_by_the_cap():
    from dfmi.timestep import next_delta_t
    # Co = 0.01: f = 50, 1 + 0.1 f = 6 -> 1.2
    assert next_delta_t(1e-6, 0.01, 0.5, 1e-4) == 1.2 * 1e-6


def test_next_delta_t_just_below_max_co_takes_the_damped_branch():
    from dfmi.timestep import next_delta_t
    # Co = 0.4: f = 1.25, 1 + 0.1 f = 1.125 < f and < 1.2
    assert _close(next_delta_t(1e-6, 0.4, 0.5, 1e-4), 1.125e-6)
    # Co = 0.48: f = 1.041666..., 1 + 0.1 f = 1.1041666... > f: the factor is f itself
    assert _close(next_delta_t(1e-6, 0.48, 0.5, 1e-4), 1e-6 * 0.5 / 0.48)


def test_next_delta_t_above_max_co_shrinks_by_max_co_over_co():
    from dfmi.timestep import next_delta_t
    assert _close(next_delta_t(1e-6, 1.0, 0.5, 1e-4), 0.5e-6)
    assert _close(next_delta_t(3e-7, 4.0, 0.8, 1e-4), 0.6e-7)


def test_next_delta_t_is_capped_by_max_delta_t():
    from dfmi.timestep import next_delta_t
    assert next_delta_t(9e-5, 0.01, 0.5, 1e-4) == 1e-4      # 1.2 x 9e-5 = 1.08e-4
    assert next_delta_t(4e-4, 1.0, 0.5, 1e-4) == 1e-4       # even a halved step (2e-4) stays under the cap
    assert next_delta_t(1e-6, 0.01, 0.5, math.inf) == 1.2 * 1e-6


def test_initial_delta_t_never_grows():
    from dfmi.timestep import initial_delta_t
    assert initial_delta_t(1e-6, 0.0, 0.5, 1e-4) == 1e-6         # Co <= small: unchanged
    assert initial_delta_t(1e-6, 1e-16, 0.5, 1e-4) == 1e-6
    assert initial_delta_t(1e-6, 0.01, 0.5, 1e-4) == 1e-6        # maxCo dt / Co = 50 dt, but never above dt
    assert initial_delta_t(1e-6, 2.0, 0.5, 1e-4) == 0.5 * 1e-6 / 2.0
    assert initial_delta_t(1e-3, 0.01, 0.5, 1e-4) == 1e-4        # nor above maxDeltaT
    for co in (1e-3, 0.3, 0.5, 0.7, 10.0):
        assert initial_delta_t(1e-6, co, 0.5, 1e-4) <= 1e-6


# ------------------------------------------------------------------ reader
def test_reader_tgv2d_is_off_and_ignores_the_commented_entries():
    from dfmi.timestep import read_control_dict
    c = read_control_dict(os.path.join(GOLDEN, "tgv2d", "controlDict"))
    assert c == {"deltaT": 1e-6, "adjustTimeStep": False, "maxCo": 1.0, "maxDeltaT": 1e-4}


def test_reader_evolving_jet():
    from dfmi.timestep import read_control_dict
    c = read_control_dict(os.path.join(GOLDEN, "controlDict_evolving_jet"))
    assert c == {"deltaT": 1e-9, "adjustTimeStep": True, "maxCo": 0.5, "maxDeltaT": 1e-4}


def test_reader_last_entry_wins_and_defaults():
    from dfmi.timestep import parse_control_dict
    txt = """FoamFile { version 2.0; class dictionary; deltaT 7; }
    deltaT 1e-7; adjustTimeStep no; /* maxCo 9; */ maxCo 0.3;
    functions { probe { deltaT 5; maxCo 2; } }
    adjustTimeStep  yes;   // adjustTimeStep off;
    maxCo 0.4;
    """
    assert parse_control_dict(txt) == {"deltaT": 1e-7, "adjustTimeStep": True, "maxCo": 0.4, "maxDeltaT": math.inf}
    assert parse_control_dict("deltaT 1;") == {"deltaT": 1.0, "adjustTimeStep": False, "maxCo": 1.0,
                                               "maxDeltaT": math.inf}
    for word, val in (("yes", True), ("on", True), ("true", True), ("no", False), ("off", False), ("false", False)):
        assert parse_control_dict(f"deltaT 1; adjustTimeStep {word};")["adjustTimeStep"] is val
    with pytest.raises(ValueError):
        parse_control_dict("deltaT 1; adjustTimeStep maybe;")
    with pytest.raises(ValueError):
        parse_control_dict("maxCo 1;")


# ------------------------------------------------------------------ header, binding, exports, documented option
def test_header_declares_the_entries_and_cites_the_loop_lines():
    txt = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(\s*dfmi_ctx\s*\*" % s, code), s
    assert "dfLowMachFoam.C:261" in txt and "dfLowMachFoam.C:262" in txt
    assert "meanCoNum" in txt and "dt_infer" in txt


def test_library_exports_and_binding_mirrors_them():
    import ctypes
    from dfmi import lib
    L = lib.load()
    A = ctypes.CDLL(CPU_A)
    for s in ENTRIES:
        assert hasattr(L, s), s
        assert hasattr(A, s), s
        assert s in lib.exported_symbols(), s
    for meth in ("courant_no", "set_delta_t", "delta_t"):
        assert hasattr(lib.Context, meth), meth


def test_option_is_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`step.courant`" in doc
    for s in ENTRIES:
        assert s in doc, s
    ctx_h = open(os.path.join(ROOT, "deepflame-dev_amd", "csrc", "dfmi_ctx.h")).read()
    assert '{"step.courant", 0}' in ctx_h   # off by default: the fixed-step path launches what it launched before


# ------------------------------------------------------------------ CPU-A
def _mech():
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "Burke2012_s9r23.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_Burke2012_s9r23.txt"), ym["species"])
    return ym, t


def _case(walls, dt=1e-6):
    """test_cpu_a.py's two boxes: periodic, and walled with a fixed inlet and an open outlet (inletOutlet U / Y,
    waveTransmissive p); phi and boundary_phi are case.face_flux of the initial state (case.init_state)"""
    from dfmi import case
    from dfmi.lib import Context
    from dfmi.mesh import hex_box, FIXED_VALUE, FIXED_ENERGY, GRADIENT_ENERGY, INLET_OUTLET, WAVE_TRANSMISSIVE
    if not os.path.exists(CPU_A):
        pytest.fail("CPU-A library not built (make -C baseline/cpu_a)")
    ym, t = _mech()
    L = 2 * np.pi * 1e-3
    m = hex_box(8, 6, 5, lengths=(L,) * 3, periodic=(not walls,) * 3, gradings=(1.0, 1.4, 1.0))
    pt = case.default_patch_types(m)
    refs = gammas = None
    if walls:
        left = [i for i, p in enumerate(m.patches) if p.name == "left"]
        right = [i for i, p in enumerate(m.patches) if p.name == "right"]
        for f in ("U", "T", "Y"):
            pt[f] = m.patch_types(0).copy(); pt[f][left] = FIXED_VALUE
        pt["he"] = m.patch_types(GRADIENT_ENERGY).copy(); pt["he"][left] = FIXED_ENERGY
        pt["U"][right] = INLET_OUTLET; pt["Y"][right] = INLET_OUTLET
        pt["p"] = m.patch_types(0).copy(); pt["p"][right] = WAVE_TRANSMISSIVE
        yu, _ = case.h2_air_compositions(ym["species"])
        refs = {"U": {"right": np.array([0.3, -0.1, 0.2])}, "Y": {"right": yu}}
        gammas = {"right": 1.4}
    ctx = Context(0, lib_path=CPU_A)
    inert = ym["species"].index("N2")
    case.setup_context(ctx, m, t, inert, dt, pt)
    f = case.tgv_fields(m, ym["species"], kernel_radius=1.2e-3)
    case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"], refs=refs, gammas=gammas)
    return ctx, m, t, pt, inert


@pytest.mark.parametrize("walls", [False, True], ids=["periodic", "open-outlet"])
def test_cpu_a_courant_number_matches_the_restatement(walls):
    dt = 1e-6
    ctx, m, t, pt, inert = _case(walls, dt)
    phi = ctx.get_field("phi", (m.n_faces,))
    bphi = ctx.get_field("boundary_phi", (m.n_boundary_slots,))
    rho = ctx.get_field("rho", (m.n_cells,))
    assert np.abs(phi).max() > 0 and (not walls or np.abs(bphi).max() > 0)
    ref = CR.courant_no(m, phi, bphi, rho, dt)
    got = ctx.courant_no()
    tol = CR.tolerance(m)
    print("CPU-A Courant", got, "restatement", ref, "tol", tol)
    assert ref[0] > ref[1] > 0
    for g, r in zip(got, ref):
        assert abs(g - r) <= tol * r
    # the number scales with the step in force
    ctx.set_delta_t(3e-6)
    assert ctx.delta_t() == 3e-6
    got3 = ctx.courant_no()
    for g, r in zip(got3, CR.courant_no(m, phi, bphi, rho, 3e-6)):
        assert abs(g - r) <= tol * r


def test_cpu_a_refuses_bad_step_sizes_and_null_outputs():
    from dfmi.lib import Context, DfmiError
    ctx, m, t, pt, inert = _case(False)
    for bad in (0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(DfmiError):
            ctx.set_delta_t(bad)
        assert ctx.delta_t() == 1e-6
    assert ctx.lib.dfmi_courant_no(ctx.h, None, None) != 0
    fresh = Context(0, lib_path=CPU_A)
    with pytest.raises(DfmiError):
        fresh.set_delta_t(1e-6)


@pytest.mark.parametrize("walls", [False, True], ids=["periodic", "open-outlet"])
def test_cpu_a_step_after_set_delta_t_matches_oracle_at_the_new_step(walls):
    """set up at dt1, then dfmi_set_delta_t(dt2), then one outer iteration: the oracle built with rdt = 1 / dt2 on
    the same state (tolerances of test_cpu_a.py::test_outer_iteration_matches_oracle); the open outlet's
    waveTransmissive valueFraction 1 / (1 + w dt deltaCoeffs) is part of the comparison"""
    import oracle as O
    from dfmi import case
    dt1, dt2 = 1e-6, 2.5e-7
    ctx, m, t, pt, inert = _case(walls, dt1)
    ctx.call("pre_time_step")
    rng = np.random.default_rng(7)
    st = case.pull_state(ctx, m, t.S)
    st["rho_old"] = st["rho"] * (1 + 1e-3 * rng.standard_normal(m.n_cells))
    st["RR"] = 1e2 * rng.standard_normal((t.S, m.n_cells))
    st["dpdt"] = 1e3 * rng.standard_normal(m.n_cells)
    case.push_state(ctx, st)
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-15, 1e-300)
    ctx.set_delta_t(dt2)
    assert ctx.delta_t() == dt2
    o = O.Oracle(m, t, {k: v.copy() for k, v in st.items()}, pt, inert, 1.0 / dt2)
    o.time_step(2)
    ctx.time_step(2)
    for n, tl in {"T": 1e-10, "p": 1e-11, "rho": 1e-10, "he": 1e-10}.items():
        assert rel_err(ctx.get_field(n, (m.n_cells,)), o[n]) < tl, n
    assert rel_err(ctx.get_field("U", (3, m.n_cells)), o["U"]) < 1e-9
    assert rel_err(ctx.get_field("Y", (t.S, m.n_cells)), o["Y"]) < 1e-9
    assert rel_err(ctx.get_field("phi", (m.n_faces,)), o["phi"]) < 1e-9
    B = m.n_boundary_slots
    assert rel_err(ctx.get_field("boundary_p", (B,)), o["boundary_p"]) < 1e-9
    if walls:
        vf = ctx.get_field("boundary_p_vf", (B,))
        assert rel_err(vf, o["boundary_p_vf"]) < 1e-12 and vf.max() > 0
        # ... and it is the new step's: the oracle at dt1 gives another one
        o1 = O.Oracle(m, t, {k: v.copy() for k, v in st.items()}, pt, inert, 1.0 / dt1)
        o1.time_step(2)
        assert rel_err(o1["boundary_p_vf"], o["boundary_p_vf"]) > 1e-3


def test_cpu_a_advance_follows_the_step_size_rules():
    """dfmi.timestep.advance on CPU-A: the history is the rules applied to the reported Courant numbers"""
    from dfmi.timestep import advance, initial_delta_t, next_delta_t
    dt0 = 1e-6
    ctx, m, t, pt, inert = _case(False, dt0)
    co0, _ = ctx.courant_no()
    ctl = {"deltaT": dt0, "adjustTimeStep": True, "maxCo": 0.5 * co0, "maxDeltaT": 1.5 * dt0}
    hist = advance(ctx, ctl, 3)
    dt = initial_delta_t(dt0, co0, ctl["maxCo"], ctl["maxDeltaT"])
    assert dt == ctl["maxCo"] * dt0 / co0
    for got_dt, co, mean in hist:
        dt = next_delta_t(dt, co, ctl["maxCo"], ctl["maxDeltaT"])
        assert got_dt == dt and dt <= ctl["maxDeltaT"] and co > mean > 0
