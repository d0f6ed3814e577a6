"""LES eddy viscosity, the parts that run without a GPU: the reference's bounds file, the turbulenceProperties
reader and the two delta rules against hand values, refusals by name, header / export / binding parity of
dfmi_turbulence_correct, and CPU-A (baseline/cpu_a) -- the second implementation of the options, fields and entry --
against LesOracle."""
import ctypes
import os
import re

import numpy as np
import pytest

import les_reference as R
from conftest import GOLDEN, ROOT, rel_err
from test_cpu_a import CPU_A, _case

FIXTURE = os.path.join(GOLDEN, "turbulenceProperties_LES")


# ------------------------------------------------------------------------------------------------ reference
def test_fp64_restatement_within_committed_bounds():
    bounds = R.load_bounds()
    measured = R.measure()
    assert set(measured) == set(bounds["models"]) == set(R.MODELS)
    bad = []
    for name, per_cls in measured.items():
        assert set(per_cls) == set(R.CLASSES)
        for cls, v in per_cls.items():
            print(f"{name:12s} {cls:12s} {v:.3e}  (committed {bounds['models'][name][cls]:.3e})")
            if not (np.isfinite(v) and v <= bounds["models"][name][cls]):
                bad.append((name, cls, v))
            # rounding of a dozen fp64 operations: the GPU bound is the floor 1e-13 unless this grows a thousandfold
            assert bounds["models"][name][cls] < 1e-15
    assert not bad, bad


def test_reference_values_by_hand():
    """pure shear d_x U_y = gamma: Smagorinsky k from its quadratic by hand; WALE exactly 0 (g . g = 0); G = 0 gives 0;
    solid rotation is NOT a zero of WALE (Omega . Omega has a deviatoric part): nut = Ck delta Cw^2 delta / Ck m^(1/4)"""
    gamma, delta = 1900.0, 2e-4
    g = np.zeros((9, 1)); g[1] = gamma
    Ck, Ce, Cw = 0.094, 1.048, 0.325
    # D_xy = gamma / 2, tr D = 0: c = 2 Ck delta gamma^2 / 2, k = c / a = Ck delta^2 gamma^2 / Ce
    want = Ck * delta * np.sqrt(Ck * delta ** 2 * gamma ** 2 / Ce)
    assert abs(R.nut_from_grad(g, [delta], 1)[0] - want) <= 4e-16 * want
    assert R.nut_from_grad(g, [delta], 2)[0] == 0.0
    for model in (1, 2):
        assert R.nut_from_grad(np.zeros((9, 3)), np.full(3, delta), model).tolist() == [0.0] * 3
    w = 700.0
    g = np.zeros((9, 1)); g[1], g[3] = w, -w            # rotation about z: Omega^2 = diag(-w^2, -w^2, 0)
    # dev(Omega^2) = (-1/3, -1/3, 2/3) w^2: m = 6 (w^2 / 3)^2, s = 0, k = (Cw^2 delta / Ck)^2 sqrt(m)
    want = Ck * delta * (Cw * Cw * delta / Ck) * (6 * (w * w / 3) ** 2) ** 0.25
    assert abs(R.nut_from_grad(g, [delta], 2)[0] - want) <= 1e-12 * want
    # the long-double restatement agrees with fp64 to fp64 rounding
    gg, dd = R.class_states("random", 64)
    for model in (1, 2):
        assert R.nut_error(R.nut_from_grad(gg, dd, model), gg, dd, model).max() < 1e-15


def test_effective_fields_order():
    rng = np.random.default_rng(2)
    rho, nut, mu, al = (rng.uniform(0.1, 2.0, 7) for _ in range(4))
    rhoD = rng.uniform(1e-5, 1e-4, (3, 7))
    muEff, alEff, DEff, ms = R.effective(rho, nut, mu, al, rhoD, 0.85, 0.7)
    mut = rho * nut
    assert np.array_equal(muEff, mut + mu) and np.array_equal(alEff, al + mut / 0.85)
    assert np.array_equal(ms, mut / 0.7) and np.array_equal(DEff, rhoD + (mut / 0.7)[None, :])


# ------------------------------------------------------------------------------------------------ dictionary, delta
def test_turbulence_properties_fixture():
    from dfmi import turbulence as T
    s = T.read_turbulence_properties(FIXTURE)
    assert s == {"model": 2, "LESModel": "WALE", "Ck": 0.1, "Ce": 1.048, "Cw": 0.3, "Prt": 0.85, "Sct": 1.0, "deltaCoeff": 2.0}
    txt = open(FIXTURE).read()
    s = T.parse_turbulence_properties(txt.replace("LESModel        WALE", "LESModel Smagorinsky"), "Sct 0.7; odeCoeffs { relTol 1e-6; }")
    assert (s["model"], s["Ck"], s["Ce"], s["Sct"], s["Prt"]) == (1, 0.2, 1.1, 0.7, 0.85)
    assert T.parse_turbulence_properties("simulationType laminar;")["model"] == 0
    # the last entry of a keyword wins, as in OpenFOAM's dictionaries
    s = T.parse_turbulence_properties("simulationType LES; LES { LESModel WALE; LESModel Smagorinsky; delta cubeRootVol; }")
    assert s["model"] == 1 and s["deltaCoeff"] == 1.0 and s["Ck"] == 0.094


@pytest.mark.parametrize("txt, names", [
    ("simulationType RAS; RAS { RASModel kEpsilon; }", ("simulationType", "RAS")),
    ("LES { LESModel WALE; }", ("simulationType",)),
    ("simulationType LES;", ("LES",)),
    ("simulationType LES; LES { LESModel Sigma; delta cubeRootVol; }", ("LESModel", "Sigma")),
    ("simulationType LES; LES { LESModel dynamicKEqn; delta cubeRootVol; }", ("LESModel", "dynamicKEqn")),
    ("simulationType LES; LES { LESModel WALE; delta vanDriest; }", ("delta", "vanDriest")),
    ("simulationType LES; LES { LESModel WALE; }", ("delta",)),
    ("simulationType LES; LES { LESModel WALE; delta cubeRootVol; WALECoeffs { Cw -1; } }", ("Cw", "-1")),
    ("simulationType LES; LES { LESModel WALE; delta cubeRootVol; WALECoeffs { Cz 1; } }", ("WALECoeffs", "Cz")),
    ("simulationType LES; LES { LESModel WALE; delta cubeRootVol; cubeRootVolCoeffs { deltaCoeff x; } }", ("deltaCoeff", "x")),
    ("simulationType LES; LES { LESModel WALE; delta cubeRootVol; turbulence off; }", ("turbulence", "off")),
])
def test_refusals_name_the_entry(txt, names):
    from dfmi import turbulence as T
    with pytest.raises(ValueError) as e:
        T.parse_turbulence_properties(txt)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_delta_rules_by_hand():
    from dfmi import turbulence as T
    from dfmi.case import flame1d_mesh
    from dfmi.mesh import hex_box
    m = hex_box(4, 3, 2, lengths=(4e-3, 3e-3, 2e-3), periodic=(False,) * 3)          # V = 1e-9 everywhere
    assert np.allclose(T.cube_root_vol_delta(m, 2.0), 2e-3, rtol=1e-14, atol=0)
    mg = hex_box(4, 3, 2, lengths=(4e-3, 3e-3, 2e-3), periodic=(True,) * 3, gradings=(1.0, 1.4, 1.0))
    assert np.array_equal(T.cube_root_vol_delta(mg), np.cbrt(mg.volume)) and np.ptp(mg.volume) > 0
    # one empty direction: V = 1e-3 x 1e-3 x 5e-4, thickness 5e-4 -> sqrt(V / thickness) = 1e-3
    m2 = hex_box(4, 3, 1, lengths=(4e-3, 3e-3, 5e-4), periodic=(False,) * 3, wall_kinds={"front": "empty", "back": "empty"})
    assert T.empty_directions(m2) == [2]
    assert np.allclose(T.cube_root_vol_delta(m2, 2.0), 2e-3, rtol=1e-14, atol=0)
    assert np.allclose(T.cube_root_vol_delta(m2, 1.0, thickness=2e-3), 5e-4, rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match="two empty directions"):
        T.cube_root_vol_delta(flame1d_mesh(8))


# ------------------------------------------------------------------------------------------------ interface parity
def test_entry_in_header_binding_and_libraries():
    from dfmi import lib
    hdr = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    assert re.search(r"\bint\s+dfmi_turbulence_correct\s*\(\s*dfmi_ctx\s*\*\s*ctx\s*\)\s*;", hdr)
    for cite in ("dfLowMachFoam.C:508", "UEqn.H:6", "YEqn.H:96", "EEqn.H:20-37", "dfUEqn.cu:305-353", "les.model", "les.Sct",
                 "delta", "boundary_nut"):
        assert cite in hdr, cite
    assert lib.SIGNATURES["dfmi_turbulence_correct"] == [lib._P]
    assert hasattr(lib.Context, "turbulence_correct")
    assert hasattr(ctypes.CDLL(CPU_A), "dfmi_turbulence_correct")
    assert hasattr(lib.load(), "dfmi_turbulence_correct")          # the HIP library (loads without a device)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ("les.model", "les.Ck", "les.Ce", "les.Cw", "les.Prt", "les.Sct", "dfmi_turbulence_correct"):
        assert key in doc, key


# ------------------------------------------------------------------------------------------------ CPU-A
def _les_case(model, prt=1.0, sct=1.0, walls=False):
    """test_cpu_a's case with seeded noise of a few per cent on the TGV velocity (tr D of both signs) in LES mode"""
    from dfmi import case, turbulence as T
    ctx, m, t, st, pt, inert, dt, ym, mech = _case(walls)
    rng = np.random.default_rng(19)
    st = dict(st)
    st["U"] = st["U"] + 0.03 * 4.0 * rng.standard_normal(st["U"].shape)
    case.push_state(ctx, st)
    ctx.correct_boundary("U")
    st["boundary_U"] = ctx.get_field("boundary_U", (3, m.n_boundary_slots))
    les = dict(T.DEFAULTS, model=model, Prt=prt, Sct=sct)
    T.apply(ctx, m, les)
    return ctx, m, t, st, pt, inert, dt, les, T.cube_root_vol_delta(m)


@pytest.mark.parametrize("model", [1, 2], ids=["Smagorinsky", "WALE"])
def test_cpu_a_les_step_matches_les_oracle(model):
    ctx, m, t, st, pt, inert, dt, les, delta = _les_case(model, prt=0.85, sct=0.7)
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-15, 1e-300)
    o = R.LesOracle(m, t, {k: v.copy() for k, v in st.items()}, pt, inert, 1.0 / dt, les, delta)
    nut0 = o["nut"].copy()
    assert nut0.min() >= 0 and nut0.max() > 0
    D = o.grad_u()
    assert (D[0] + D[4] + D[8]).min() < 0 < (D[0] + D[4] + D[8]).max()
    ctx.turbulence_correct()
    assert rel_err(ctx.get_field("nut", (m.n_cells,)), nut0) < 1e-13
    o.time_step(2)
    ctx.time_step(2)
    for n, tl in {"T": 1e-10, "p": 1e-11, "rho": 1e-10, "he": 1e-10}.items():
        assert rel_err(ctx.get_field(n, (m.n_cells,)), o[n]) < tl, n
    assert rel_err(ctx.get_field("U", (3, m.n_cells)), o["U"]) < 1e-9
    assert rel_err(ctx.get_field("Y", (t.S, m.n_cells)), o["Y"]) < 1e-9
    assert rel_err(ctx.get_field("phi", (m.n_faces,)), o["phi"]) < 1e-9
    assert rel_err(ctx.get_field("nut", (m.n_cells,)), o["nut"]) < 1e-9
    assert rel_err(ctx.get_field("boundary_nut", (m.n_boundary_slots,)), o["boundary_nut"]) < 1e-9
    assert not np.array_equal(o["nut"], nut0)                       # the end-of-step update moved it
    for n, shp in (("sumYDiffError", (3, m.n_cells)), ("hDiffCorrFlux", (3, m.n_cells)), ("diffAlphaD", (m.n_cells,)),
                   ("phiUc", (m.n_faces,))):
        assert not ctx.get_field(n, shp).any(), n
    # the turbulent step is not the laminar one
    import oracle as O
    lam = O.Oracle(m, t, {k: v.copy() for k, v in st.items()}, pt, inert, 1.0 / dt)
    lam.time_step(2)
    assert rel_err(lam["U"], o["U"]) > 1e-6


def test_cpu_a_options_validity_and_laminar_noop():
    from dfmi.lib import DfmiError
    ctx, m, t, st, pt, inert, dt, les, delta = _les_case(1)
    for key, bad in (("les.model", 3), ("les.model", -1), ("les.model", 0.5), ("les.Ck", 0.0), ("les.Sct", -1.0),
                     ("les.Prt", float("inf")), ("les.Cw", float("nan")), ("les.nope", 1.0)):
        with pytest.raises(DfmiError):
            ctx.set_option(key, bad)
    assert ctx.get_option("les.model") == 1 and ctx.get_option("les.Ce") == 1.048
    with pytest.raises(DfmiError, match="nut"):
        ctx.set_field("nut", np.zeros(m.n_cells))
    with pytest.raises(DfmiError, match="nut is not valid"):
        ctx.call("U_process")                                       # never formed
    ctx.turbulence_correct()
    ctx.call("U_process")
    ctx.set_field("U", st["U"])                                     # writing U invalidates nut
    with pytest.raises(DfmiError, match="nut is not valid"):
        ctx.call("U_process")
    ctx.turbulence_correct()
    ctx.call("U_process")
    for key, v in (("les.Ck", 0.1), ("les.model", 2)):              # so does a coefficient or the model
        ctx.set_option(key, v)
        with pytest.raises(DfmiError, match="nut is not valid"):
            ctx.call("E_process")
        ctx.turbulence_correct()
    ctx.set_field("delta", delta)
    with pytest.raises(DfmiError, match="nut is not valid"):
        ctx.call("Y_process")
    with pytest.raises(DfmiError, match="delta"):
        ctx.set_field("delta", np.zeros(m.n_cells))
    ctx.set_option("les.model", 0)                                  # laminar: the entry is a successful no-op
    nut = ctx.get_field("nut", (m.n_cells,))
    ctx.turbulence_correct()
    assert np.array_equal(ctx.get_field("nut", (m.n_cells,)), nut)
    ctx.call("U_process")
