"""k-epsilon wall functions and turbulent inlets without a GPU: the case reader (foam_io.turbulence_boundary on the three
boundary files of the reference's Sandia D case, tests/golden/sandiaD_0), the restatement tests/wallfn_reference.py
(yPlusLam, the continuity of nut_w, the constraint as linear algebra, the seeded state's conditions, the committed bounds)
and the contract's formulas in the header and the documents."""
import os
import re

import numpy as np
import pytest

import ras_reference as R
import wallfn_reference as W
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANDIA = os.path.join(GOLDEN, "sandiaD_0")


def _read(field):
    from dfmi import foam_io
    entries, internal = foam_io.read_boundary_entries(os.path.join(SANDIA, field))
    types = {p: e["type"] for p, e in entries.items()}
    return types, entries, internal


def _no_wedge(types):
    return {p: t for p, t in types.items() if t != "wedge"}


# ------------------------------------------------------------------------------------------------ the case reader
def test_turbulence_boundary_on_the_sandia_files():
    from dfmi import foam_io, mesh as M
    out = {}
    for f in ("k", "epsilon", "nut"):
        types, entries, internal = _read(f)
        assert set(types) == {"wallTube", "outlet", "inletPilot", "inletAir", "wallOutside", "inletCH4", "frontAndBack_pos",
                              "frontAndBack_neg"}
        with pytest.raises(ValueError, match=rf"{f}: patch frontAndBack_pos: boundary condition wedge"):
            foam_io.turbulence_boundary(f, types, entries, internal)
        out[f] = foam_io.turbulence_boundary(f, _no_wedge(types), entries, internal)
    k, e, n = out["k"], out["epsilon"], out["nut"]
    for w in ("wallTube", "wallOutside"):
        assert k["types"][w] == M.ZERO_GRADIENT                                   # kqRWallFunction
        assert e["types"][w] == M.EPSILON_WALL_FUNCTION == 13 and w not in e["params"]   # 0/epsilon's copies are ignored
        assert n["types"][w] == M.NUTK_WALL_FUNCTION == 14
        assert n["params"][w] == {"Cmu": 0.09, "kappa": 0.41, "E": 9.8}
        assert n["values"][w] == 0.0 and e["values"][w] == 30000.0 and k["values"][w] == 30.0   # $internalField resolved
    for i, I, L in (("inletPilot", 0.0628, 0.000735), ("inletAir", 0.0471, 0.019677), ("inletCH4", 0.0458, 0.000504)):
        assert k["types"][i] == M.TURBULENT_INTENSITY_K_INLET == 15 and k["params"][i] == {"intensity": I}
        assert e["types"][i] == M.TURBULENT_MIXING_LENGTH_EPSILON_INLET == 16 and e["params"][i] == {"mixingLength": L}
        assert n["types"][i] == M.CALCULATED and n["values"][i] == 0.0
    assert k["types"]["outlet"] == e["types"]["outlet"] == M.ZERO_GRADIENT and n["types"]["outlet"] == M.CALCULATED
    assert k["values"]["outlet"] is None
    for name, code in (("epsilonWallFunction", 13), ("nutkWallFunction", 14), ("turbulentIntensityKineticEnergyInlet", 15),
                       ("turbulentMixingLengthDissipationRateInlet", 16)):
        assert M.BC_NAMES[name] == code


def test_turbulence_boundary_refusals_name_their_subject():
    from dfmi import foam_io
    tb = foam_io.turbulence_boundary
    for t in ("nutUWallFunction", "nutkRoughWallFunction", "nutUSpaldingWallFunction", "nutLowReWallFunction"):
        with pytest.raises(ValueError, match=rf"nut: patch w: boundary condition {t}"):
            tb("nut", {"w": t}, {"w": {"type": t}})
    with pytest.raises(ValueError, match="k: patch w: boundary condition epsilonWallFunction belongs to the field epsilon"):
        tb("k", {"w": "epsilonWallFunction"}, {})
    with pytest.raises(ValueError, match="k: patch i: turbulentIntensityKineticEnergyInlet without a intensity"):
        tb("k", {"i": "turbulentIntensityKineticEnergyInlet"}, {"i": {}})
    with pytest.raises(ValueError, match="mixingLength -1 must be positive"):
        tb("epsilon", {"i": "turbulentMixingLengthDissipationRateInlet"}, {"i": {"mixingLength": "-1"}})
    with pytest.raises(ValueError, match=r"value \$internalField"):
        tb("nut", {"w": "calculated"}, {"w": {"value": "$internalField"}})
    with pytest.raises(ValueError, match="boundary condition codedFixedValue is not supported"):
        tb("k", {"w": "codedFixedValue"}, {})
    # the strict mapper keeps refusing them all
    with pytest.raises(ValueError, match="epsilonWallFunction"):
        foam_io.turbulence_patch_types("epsilon", {"w": "epsilonWallFunction"})
    assert "strict mapper" in foam_io.turbulence_patch_types.__doc__


def test_apply_ras_passes_patch_params_after_the_types():
    from dfmi import turbulence as T

    class Rec:
        def __init__(self):
            self.calls = []

        def set_option(self, *a):
            pass

        def set_patch_types(self, f, t):
            self.calls.append(("types", f))

        def set_patch_param(self, f, p, n, v):
            self.calls.append(("param", f, p, n, v))
    r = Rec()
    T.apply_ras(r, None, T.RAS_DEFAULTS, {"k": [0], "epsilon": [0], "nut": [14]},
                patch_params={"nut": {0: {"E": 9.0}}, "k": {1: {"intensity": 0.05}}})
    assert r.calls == [("types", "k"), ("types", "epsilon"), ("types", "nut"), ("param", "nut", 0, "E", 9.0),
                       ("param", "k", 1, "intensity", 0.05)]
    r = Rec()
    T.apply_ras(r, None, T.RAS_DEFAULTS)                                            # without the argument: as before
    assert r.calls == []


def test_cpu_a_refuses_the_codes_and_parameters_by_name():
    from dfmi.lib import DfmiError
    from test_cpu_a import _case
    ctx, m = _case(True)[:2]
    try:
        for field, code, name in (("epsilon", 13, "epsilonWallFunction"), ("nut", 14, "nutkWallFunction"),
                                  ("k", 15, "turbulentIntensityKineticEnergyInlet"),
                                  ("epsilon", 16, "turbulentMixingLengthDissipationRateInlet"), ("U", 13, "epsilonWallFunction")):
            t = m.patch_types(0).copy()
            t[0] = code
            with pytest.raises(DfmiError, match=rf"{name} \(field '{field}'\): CPU-A does not implement"):
                ctx.set_patch_types(field, t)
        for f, n in (("nut", "Cmu"), ("nut", "kappa"), ("nut", "E"), ("k", "intensity"), ("epsilon", "mixingLength")):
            with pytest.raises(DfmiError, match=rf"\('{f}', '{n}'\): CPU-A does not implement"):
                ctx.set_patch_param(f, 0, n, 1.0)
        ctx.set_patch_types("nut", m.patch_types(5))                               # the codes it had stay accepted
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the restatement
def test_y_plus_lam_is_the_fixed_point():
    """the ten-step yPlusLam of (0.41, 9.8) is the fixed point of yPlusLam kappa = log(E yPlusLam) to 1e-8 of its value.
    The map contracts by 1 / (kappa yPlusLam) = 0.21 per step, so ten steps from 11 (0.53 away) end 0.53 * 0.21^10 = 9.5e-8
    from it: 8.2e-9 relative. The same distance read as the equation's residual |yPlusLam kappa - log(E yPlusLam)| is
    3.2e-8 (the distance times kappa (1 - 0.21)), which is printed and held to that reasoning's 4e-8, not to 1e-8."""
    ypl = W.y_plus_lam(0.41, 9.8)
    fix = 11.0
    for _ in range(200):
        fix = np.log(9.8 * fix) / 0.41
    assert abs(fix * 0.41 - np.log(9.8 * fix)) <= 1e-14
    res = abs(ypl * 0.41 - np.log(9.8 * ypl))
    print(f"yPlusLam {ypl!r}, fixed point {fix!r}, relative distance {abs(ypl / fix - 1):.2e}, residual {res:.2e}")
    assert abs(ypl / fix - 1) <= 1e-8
    assert res <= 4e-8
    assert 11.5 < ypl < 11.6
    assert abs(float(W.y_plus_lam(0.41, 9.8, W.LD)) - ypl) <= 1e-13 * ypl


def test_nut_w_vanishes_continuously_at_y_plus_lam():
    m = R.get_mesh("walls")
    ws = W.default_setup(m)
    c25, _, _, _, ypl = ws.consts()
    B = m.n_boundary_slots
    brho = np.full(B, 1.1)
    k = np.full(m.n_cells, 30.0)
    y = 1.0 / ws.bdc
    last = None
    for rel in (1e-3, 1e-6, 1e-9, -1e-9):
        bmu = brho * (c25 * y) * np.sqrt(30.0) / (ypl * (1 + rel))
        bn, yp = W.wall_nut(ws, k, bmu, brho)
        assert np.abs(yp / (ypl * (1 + rel)) - 1).max() <= 1e-14
        r = np.abs(bn / (bmu / brho)).max()
        if rel > 0:
            # f = yPlus kappa / log(E yPlus): f(yPlusLam (1 + rel)) - 1 = (f(yPlusLam) - 1) + rel (1 - 1 / log(E yPlusLam)),
            # the first term the ten-step iteration's residual over log(E yPlusLam) = 3.2e-8 / 4.73 < 1e-8, the slope 0.79
            assert 0 < r <= rel + 1e-8, (rel, r)
            assert last is None or r < last
            last = r
        else:
            assert r == 0.0


def _constrained_system(name="walls", seed=3):
    m = R.get_mesh(name)
    ws = W.default_setup(m, "yz")
    tp = W.Topo(m)
    st = W.wall_state(m, ws)
    rng = np.random.default_rng(seed)
    C_, B = m.n_cells, m.n_boundary_slots
    q = R.DEFAULTS
    G, dv = rng.uniform(0, 1e6, C_), rng.uniform(-1e3, 1e3, C_)
    bnut, _ = W.wall_nut(ws, st["k"], st["boundary_mu"], st["boundary_rho"])
    eps, G, beps, con, _ = W.wall_update(ws, tp, st["k"], st["U"], st["boundary_U"], st["boundary_mu"], st["boundary_rho"], bnut,
                                         st["epsilon"], G, st["boundary_epsilon"])
    Su, Sp = R.sources(0, q, G, dv, st["rho"], st["k"], eps)
    D = R.diffusivity(st["rho"], st["nut"], st["mu"], q["sigmaEps"])
    bD = R.diffusivity(st["boundary_rho"], bnut, st["boundary_mu"], q["sigmaEps"])
    pt = W.device_types(ws.eps_pt)
    o = R.scalar_assemble(tp, pt, eps, beps, st["rho"], st["rho"], st["phi"], st["boundary_phi"], D, bD, Su, Sp, 1e6)
    return m, tp, pt, o, eps, con


def _dense(m, o):
    """the assembled system as a dense matrix and right-hand side (no coupled patches on these meshes)"""
    C_ = m.n_cells
    A = np.diag(o["diag"].copy())
    b = o["source"].copy()
    A[m.neighbour, m.owner] += o["lower"]
    A[m.owner, m.neighbour] += o["upper"]
    cell = R.NR.Slots(m).cell
    np.add.at(A, (cell, cell), o["internal_coeffs"])
    np.add.at(b, cell, o["boundary_coeffs"])
    return A, b


def test_constrained_matrix_returns_the_wall_values_and_the_eliminated_system():
    m, tp, pt, o, eps, con = _constrained_system()
    assert 0 < con.sum() < m.n_cells
    shared = [(f) for c in range(m.n_cells) for f, n, own in tp.faces[c] if own and con[c] != con[n]]
    assert shared, "constrained and unconstrained cells share faces"
    A0, b0 = _dense(m, {k: v.copy() for k, v in o.items()})
    oc = W.constrain(tp, {k: v.copy() for k, v in o.items()}, con, eps)
    A, b = _dense(m, oc)
    x = np.linalg.solve(A, b)
    assert np.abs(x[con] / eps[con] - 1).max() <= 4 * 2.0 ** -52                  # v on the wall cells
    # the rest: the unconstrained rows of the original system with the constrained unknowns moved to the right
    free = ~con
    xs = np.linalg.solve(A0[np.ix_(free, free)], b0[free] - A0[np.ix_(free, con)] @ eps[con])
    assert np.abs(x[free] / xs - 1).max() <= 1e-11
    # rows of constrained cells are diagonal, and no row keeps a constrained column
    off = A - np.diag(np.diag(A))
    assert not off[con].any() and not off[:, con].any()
    assert np.array_equal(np.diag(A)[con], o["diag"][con])                         # slot coefficients gone from the diagonal


def test_wall_update_weights_corner_and_edge_cells():
    m = R.get_mesh("walls")
    ws = W.default_setup(m)
    tp = W.Topo(m)
    n = np.array([sum(ws.eps_wall[b] for b in tp.slots[c]) for c in range(m.n_cells)])
    assert set(n) == {0, 1, 2, 3}
    st = W.wall_state(m, ws)
    bnut, _ = W.wall_nut(ws, st["k"], st["boundary_mu"], st["boundary_rho"])
    zC = np.zeros(m.n_cells)
    eps, G, beps, con, _ = W.wall_update(ws, tp, st["k"], st["U"], st["boundary_U"], st["boundary_mu"], st["boundary_rho"], bnut,
                                         zC, zC, np.zeros(m.n_boundary_slots))
    assert np.array_equal(con, n > 0)
    # each slot alone (weight 1), then averaged by hand
    yp, y, nuw = W.y_plus(ws, st["k"], st["boundary_mu"], st["boundary_rho"])
    c25, c75, kap, _, ypl = ws.consts()
    for c in np.nonzero(n >= 2)[0][:6]:
        kc = st["k"][c]
        one = [c75[b] * kc ** 1.5 / (kap[b] * y[b]) if yp[b] > ypl[b] else 2 * kc * nuw[b] / y[b] ** 2 for b in tp.slots[c]]
        assert abs(eps[c] / np.mean(one) - 1) <= 1e-14
        assert all(beps[b] == eps[c] for b in tp.slots[c])


@pytest.mark.parametrize("name", W.MESHES)
def test_seeded_state_meets_the_gpu_suite_conditions(name):
    m = R.get_mesh(name)
    for which in ("all", "yz"):
        ws = W.default_setup(m, which)
        lo, hi, gap, kmin, emin, ymin, ymax = W.state_conditions(ws, W.wall_state(m, ws))
        print(name, which, f"below {lo:.2f} above {hi:.2f} gap {gap:.1e} yPlus {ymin:.2f} .. {ymax:.1f}")
        assert lo >= 0.2 and hi >= 0.2 and gap > 1e-6 and kmin > 0 and emin > 0
        assert ymin < 3 and ymax > 100


def test_bounds_file_is_current_and_small():
    doc = W.load_bounds()
    assert set(doc["meshes"]) == set(W.MESHES)
    for name, v in doc["meshes"].items():
        assert set(v) == {"boundary_nut", "boundary_yPlus", "epsilon", "G"}
        for what, x in v.items():
            assert 0 <= x <= 5e-15, (name, what, x)          # a few roundings: the restatement is the definition in fp64
            assert W.gpu_bound(doc, name, what) == 1e-13
    got = W.measure()["walls"]
    for what, x in got.items():
        assert abs(x - doc["meshes"]["walls"][what]) <= 1e-16, what


# ------------------------------------------------------------------------------------------------ the contract in words
def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return re.sub(r"\s+", " ", f.read().replace("//", " ").replace("*", " * "))


def test_header_and_documents_state_the_contract():
    h = _text("include", "dfmi.h")
    for tok in ("epsilonWallFunction", "nutkWallFunction", "turbulentIntensityKineticEnergyInlet",
                "turbulentMixingLengthDissipationRateInlet", "boundary_yPlus", "yPlusLam", "Cmu25 = sqrt(sqrt(Cmu))",
                "Cmu75 = Cmu25 * sqrt(Cmu)", "log(max(E * ypl, 1)) / kappa", "yPlus = ((Cmu25 * y) * sqrt(k_c)) / nuw",
                "nuw * ((yPlus * kappa) / log(E * yPlus) - 1)", "((w * Cmu75) * (k_c * sqrt(k_c))) / (kappa * y)",
                "(((w * 2) * k_c) * nuw) / (y * y)", "fvMatrix::setValues", "source = v_c * diag",
                "(1.5 * (I * I)) * ((Ux * Ux + Uy * Uy) + Uz * Uz)", "(Cmu75 / L) * (kb * sqrt(kb))", "intensity", "mixingLength"):
        assert re.sub(r"\s+", " ", tok.replace("*", " * ")) in h, tok
    d = _text("DESIGN.md")
    for tok in ("epsilonWallFunction", "RNGkEpsilon", "nearWallDist", "wedge", "boundary_yPlus", "k_ras_wall", "k_ras_nut_wall",
                "k_ras_inlet_ref"):
        assert tok in d, tok
    i = _text("INTEGRATION.md")
    for tok in ("epsilonWallFunction", "nutkWallFunction", "intensity", "mixingLength", "kappa"):
        assert tok in i, tok
