"""The Peng-Robinson point reference (tests/realfluid_reference.py) checked against itself and against what it must
reduce to, the YAML reader's refusals, the committed bounds and the new ABI symbol. No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

import realfluid_reference as RF

LD, F64 = RF.LD, RF.F64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.mark.parametrize("name", RF.TABLES)
@pytest.mark.parametrize("cls", RF.CLASSES)
def test_classes_keep_their_states(name, cls):
    """every class keeps at least 95 % of its draw (asserted inside states()) and holds a few hundred states, or, for
    pure, every species and pair"""
    st, ref, drop = RF.states(name, cls)
    assert drop <= RF.MAX_DROP
    assert st.n >= (200 if cls != "pure" else RF.table(name)[0].S)
    kinks = RF.kink_temperatures(RF.table(name)[1])
    T = np.asarray(ref["T"], dtype=F64)
    assert (np.abs(T[:, None] - kinks[None, :]) >= RF.KINK_MARGIN * T[:, None]).all()
    Z = np.asarray(ref["Z"], dtype=F64)
    rt = ref["roots"]
    if cls == "dense":
        assert ((Z >= 0.2) & (Z <= 0.5)).all()
    if cls == "near_critical":
        assert not np.asarray(rt["three"]).any()
    if cls == "three_root":
        assert (np.asarray(rt["n_adm"]) == 3).all()
        assert (np.abs(np.asarray(rt["dlnphi"], dtype=F64)) >= RF.DLNPHI_MIN).all()
        # the middle root is never the stable one: the kernels compare the outer two only
        assert (np.asarray(rt["lmid"] - rt["lbest"], dtype=F64) > 0).all()
        assert np.asarray(rt["low"]).any() and not np.asarray(rt["low"]).all(), "both phases occur"
    if cls == "pure":
        assert (np.asarray(ref["rhoD"], dtype=F64)[np.asarray(ref["X"], dtype=F64) + 1e-10 > 1] == 0).all()


@pytest.mark.parametrize("cls", RF.CLASSES)
def test_cubic_residual_at_rounding(cls):
    """the float64 root, put back into the cubic in long double: |f(Z)| <= 16 eps (|Z|^3 + |a2| Z^2 + |a1 Z| + |a0|) --
    the last Newton step (<= 4 eps |Z|) times |f'| <= 3 sum / |Z|, plus the 4 eps sum of f's own evaluation"""
    for name in ("bfer6", "drawn9"):
        st, ref, _ = RF.states(name, cls)
        got = RF.restatement(name, st)
        t, eos = RF.table(name)
        mx = RF.Mix(t, eos, st.Y, LD)
        T, p = np.asarray(got["T"], dtype=LD), np.asarray(st.p, dtype=LD)
        s = RF.state_at(mx, T, p, want_roots=True)
        a2, a1, a0 = s["roots"]["coef"]
        Z = np.asarray(got["Z"], dtype=LD)
        f = np.abs(((Z + a2) * Z + a1) * Z + a0)
        scale = np.abs(Z) ** 3 + np.abs(a2) * Z * Z + np.abs(a1 * Z) + np.abs(a0)
        assert float((f / scale).max()) <= 16 * EPS, (name, float((f / scale).max()))


@pytest.mark.parametrize("cls", ("supercritical", "dense", "near_critical", "dilute"))
def test_cp_is_dh_dT(cls):
    """cp against the central difference of the long-double h along the isobar, extrapolated once (steps 2e-6 T and
    1e-6 T: truncation ~ step^4, rounding ~ 2^-63 / step). States whose step would cross a kink of |s_i| or that have
    three admissible roots (the phase may flip inside the step) are left out of this check only."""
    name = "bfer6"
    st, ref, _ = RF.states(name, cls)
    t, eos = RF.table(name)
    mx = RF.Mix(t, eos, st.Y, LD)
    T, p = np.asarray(st.T, dtype=LD), np.asarray(st.p, dtype=LD)
    kinks = RF.kink_temperatures(eos)
    ok = (np.abs(st.T[:, None] - kinks[None, :]) > 1e-5 * st.T[:, None]).all(axis=1) & (np.asarray(ref["roots"]["n_adm"]) < 3)
    tm = np.asarray(t.nasa[:, 0])
    ok &= (np.abs(st.T[:, None] - tm[None, :]) > 1e-5 * st.T[:, None]).all(axis=1)      # nor a NASA range switch
    assert ok.mean() > 0.5
    hh = T * LD(2e-6)
    h = lambda x: RF.state_at(mx, x, p)["h"]
    c1 = (h(T + hh) - h(T - hh)) / (2 * hh)
    c2 = (h(T + hh / 2) - h(T - hh / 2)) / hh
    d = (4 * c2 - c1) / 3
    err = np.asarray(np.abs(d - ref["cp"]) / ref["cp"], dtype=F64)[ok]
    assert err.max() <= 1e-9, float(err.max())


@pytest.mark.parametrize("cls", ("supercritical", "dense", "dilute"))
def test_psi_quotient_against_analytic(cls):
    """the one-sided quotient is first order in dx: psi(dx) - psi(dx / 2) is half its error, so the extrapolation
    2 psi(dx / 2) - psi(dx) must meet the analytic (d rho / d p)_h to second order, and psi(dx) itself to within
    3 |psi(dx) - psi(dx / 2)|. One-phase states (a flip between p and p (1 - dx) is not a derivative)."""
    name = "bfer6"
    st, ref, _ = RF.states(name, cls)
    t, eos = RF.table(name)
    one = np.asarray(ref["roots"]["n_adm"]) < 3
    kinks = RF.kink_temperatures(eos)
    one &= (np.abs(st.T[:, None] - kinks[None, :]) > 1e-4 * st.T[:, None]).all(axis=1)
    one &= (np.abs(st.T[:, None] - np.asarray(t.nasa[:, 0])[None, :]) > 1e-4 * st.T[:, None]).all(axis=1)
    k = np.where(one)[0]
    assert k.size > st.n // 2
    p, Y, T = st.p[k], st.Y[:, k], st.T[k]
    full = RF.point(t, eos, p, Y, T=T)
    half = RF.point(t, eos, p, Y, T=T, dx=RF.DX / 2)
    exact = RF.psi_analytic(t, eos, p, Y, T)
    d = np.abs(full["psi"] - half["psi"])
    e1 = np.abs(full["psi"] - exact)
    e2 = np.abs(2 * half["psi"] - full["psi"] - exact)
    tiny = LD(1e-9) * np.abs(exact)
    assert np.all(e1 <= 3 * d + tiny), float(np.max(e1 / (3 * d + tiny)))
    assert float(np.max(e2 / np.abs(exact))) <= 1e-5, float(np.max(e2 / np.abs(exact)))
    assert np.all(np.asarray(full["psi"], dtype=F64) > 0)


def test_dilute_is_the_ideal_gas_to_the_second_virial_bound():
    import oracle as O
    for name in RF.TABLES:
        st, ref, _ = RF.states(name, "dilute")
        t, eos = RF.table(name)
        ig = O.thermo_points(t, st.T, np.zeros(st.n), st.p, st.Y, True)
        mx = RF.Mix(t, eos, st.Y, F64)
        aal = mx.attraction(st.T)[0]
        RT = RF.R_GAS * st.T
        bound = 2 * st.p * np.maximum(mx.bm, aal / RT) / RT
        rho = np.asarray(ref["rho"], dtype=F64)
        assert (np.abs(rho / ig["rho"] - 1) <= bound + 4 * EPS).all(), name
        # and what does not depend on the equation of state is the ideal value
        assert np.allclose(np.asarray(ref["mu"], dtype=F64), ig["mu"], rtol=1e-12, atol=0), name
        sc = np.maximum(np.abs(ig["hai"]), RT[None, :] / t.W[:, None])      # thermo_reference.errors' scale for hai
        assert (np.abs(np.asarray(ref["hai"], dtype=F64) - ig["hai"]) <= 1e-12 * sc).all(), name


def test_critical_temperatures_of_the_fixture():
    t, eos = RF.bfer6()
    Tc = dict(zip(RF.load_fixture()["species"], RF.species_params(eos)["Tc"]))
    known = {"O2": 154.6, "H2O": 647.1, "CH4": 190.56, "CO": 132.9, "CO2": 304.1, "N2": 126.2}
    for s, v in known.items():
        assert abs(Tc[s] - v) < 0.15, (s, Tc[s])
    kink = dict(zip(RF.load_fixture()["species"], RF.kink_temperatures(eos)))
    assert 1800 < kink["O2"] < 1950      # inside a flame (the kink hazard)


def test_restatement_converges_within_its_step_limit():
    for name in RF.TABLES:
        st, _, _ = RF.states(name, "newton")
        got = RF.restatement(name, st)
        assert np.asarray(got["converged"]).all(), name


def test_oracle_step_reduces_to_the_ideal_step():
    """RealFluidOracle with a_i = 0 and a vanishing b_i is the ideal gas, so its rho_thermo sequence must land where
    the ideal shortcut rho = psi p does: the whole step at the project's full-step tolerance (psi itself carries the
    quotient's rounding, 2^-52 / dx). One oracle alive at a time: the C oracle keeps one registry."""
    import oracle as O
    from conftest import rel_err
    from dfmi import case
    from dfmi.mesh import hex_box, FIXED_VALUE
    t, _ = RF.bfer6()
    L = 1e-3
    m = hex_box(6, 5, 4, lengths=(2 * np.pi * L,) * 3, periodic=(False,) * 3, gradings=(1.0, 1.3, 1.0))
    pt = case.default_patch_types(m)
    name = [p.name for p in m.patches]
    pt["T"] = pt["T"].copy()
    for side in ("left", "right", "top"):
        pt["T"][name.index(side)] = FIXED_VALUE
    f = RF.flow_fields(m, t.species, L)
    f["p"] = np.full(m.n_cells, 101325.0)
    wall_T = {p.name: 300.0 + 40.0 * k for k, p in enumerate(m.patches)}
    inert = t.species.index("N2")
    eos0 = {"a": np.zeros(t.S), "b": np.full(t.S, 1e-12), "w": np.zeros(t.S)}
    a = RF.cpu_state(m, t, eos0, pt, inert, 1e6, f, wall_T)
    a.time_step(2)
    got = {k: v.copy() for k, v in a.arr.items()}
    b = RF.cpu_state(m, t, None, pt, inert, 1e6, f, wall_T, cls=O.Oracle)
    b.time_step(2)
    for n in ("T", "p", "rho", "he", "psi", "U", "Y", "phi", "boundary_rho", "boundary_p", "boundary_psi"):
        assert rel_err(got[n], b[n]) < 1e-9, (n, rel_err(got[n], b[n]))
    assert np.array_equal(got["rho"], got["rho_thermo"])


# ------------------------------------------------------------------------------------------------ the YAML reader
_YAML = """
units: {length: cm, quantity: mol, activation-energy: cal/mol}
phases:
- name: gas
  thermo: %(thermo)s
  species: [O2, N2]
species:
- name: O2
  composition: {O: 2}
  equation-of-state:
    model: %(m0)s
    a: 1.498106185641390e+11
    b: 19.83052918
    acentric-factor: 0.0222
%(extra)s
- name: N2
  composition: {N: 2}
  equation-of-state:
    model: %(m1)s
    a: 1.481521374117060e+11
    b: 24.02424579
    acentric-factor: 0.0372
"""


def _yaml(tmp_path, thermo="Peng-Robinson", m0="Peng-Robinson", m1="Peng-Robinson", extra=""):
    p = tmp_path / "mech.yaml"
    p.write_text(_YAML % {"thermo": thermo, "m0": m0, "m1": m1, "extra": extra})
    return str(p)


def test_parse_eos_units_and_order(tmp_path):
    from dfmi import realfluid
    fx = RF.load_fixture()
    eos = realfluid.parse_eos(_yaml(tmp_path), ["N2", "O2"])
    assert eos["model"] == realfluid.PENG_ROBINSON and eos["species"] == ["N2", "O2"]
    i, j = fx["species"].index("N2"), fx["species"].index("O2")
    assert np.allclose(eos["a"], [fx["a"][i], fx["a"][j]], rtol=1e-14)
    assert np.allclose(eos["b"], [fx["b"][i], fx["b"][j]], rtol=1e-14)
    assert np.array_equal(eos["acentric"], [fx["acentric"][i], fx["acentric"][j]])
    assert realfluid.parse_eos(_yaml(tmp_path, thermo="ideal-gas"))["model"] == realfluid.IDEAL


def test_parse_eos_refusals(tmp_path):
    from dfmi import realfluid
    with pytest.raises(realfluid.RealFluidError, match="Redlich-Kwong"):
        realfluid.parse_eos(_yaml(tmp_path, thermo="Redlich-Kwong", m0="Redlich-Kwong", m1="Redlich-Kwong"))
    with pytest.raises(realfluid.RealFluidError, match="Redlich-Kwong"):
        realfluid.parse_eos(_yaml(tmp_path, m1="Redlich-Kwong"))
    with pytest.raises(realfluid.RealFluidError, match="mix of models"):
        realfluid.parse_eos(_yaml(tmp_path, m1="ideal-gas"))
    with pytest.raises(realfluid.RealFluidError, match="binary-a"):
        realfluid.parse_eos(_yaml(tmp_path, extra="    binary-a: {N2: 1.0e+11}"))
    with pytest.raises(realfluid.RealFluidError, match="'AR'"):
        realfluid.parse_eos(_yaml(tmp_path), ["O2", "AR"])


def test_read_case_eos_refuses_chung_by_name(tmp_path):
    from dfmi import realfluid
    (tmp_path / "constant").mkdir()
    _yaml(tmp_path)
    props = tmp_path / "constant" / "CanteraTorchProperties"
    props.write_text('chemistry off;\nCanteraMechanismFile "mech.yaml";\ntransportModel "Chung"; // high pressure\n')
    with pytest.raises(realfluid.RealFluidError, match="Chung"):
        realfluid.read_case_eos(str(tmp_path))
    eos = realfluid.read_case_eos(str(tmp_path), transport="Mix")
    assert eos["model"] == realfluid.PENG_ROBINSON and eos["transport"] == "Mix" and eos["species"] == ["O2", "N2"]
    props.write_text('CanteraMechanismFile "mech.yaml";\ntransportModel "Mix";\n')
    assert realfluid.read_case_eos(str(tmp_path))["model"] == realfluid.PENG_ROBINSON


# ------------------------------------------------------------------------------------------------ bounds and ABI
def test_committed_bounds_equal_a_fresh_measure():
    """The committed file is what --measure writes: the same tables, classes, state counts and drop fractions exactly,
    and every maximum reproduced. The maxima are sums of roundings of the host's libm (log, cbrt, acos in float64 and
    long double), so on another host the last digits move (seen: 4.4029e-14 against 4.4023e-14); a maximum is held to
    a factor 2 either way where it matters to a tolerance, i.e. above a quarter of the 1e-13 floor of gpu_bound."""
    doc = RF.load_bounds()
    fresh = json.loads(json.dumps(RF.measure()))
    assert set(fresh) == set(doc["tables"]) == set(RF.TABLES)
    assert json.loads(json.dumps(RF.class_maxima(doc["tables"]))) == doc["classes"]
    bad = []
    for name, per_cls in fresh.items():
        assert set(per_cls) == set(doc["tables"][name]) == set(RF.CLASSES)
        for cls, per_q in per_cls.items():
            want = doc["tables"][name][cls]
            assert per_q["states"] == want["states"] and per_q["dropped"] == want["dropped"], (name, cls)
            for q in RF.QUANTITIES:
                a, b = per_q[q], want[q]
                floor = 2.5e-14 if q not in ("rhoD_kappa", "rhoD_dominant") else 1.0
                if max(a, b) > floor and not (a <= 2 * b and b <= 2 * a):
                    bad.append((name, cls, q, a, b))
    assert not bad, bad


def test_new_symbol_is_exported_by_both_libraries():
    with open(os.path.join(ROOT, "include", "dfmi.h")) as f:
        assert "int dfmi_thermo_set_eos(dfmi_ctx* ctx, int model, int num_species," in f.read()
    from dfmi import lib
    assert "dfmi_thermo_set_eos" in lib.exported_symbols()
    assert hasattr(lib.load(), "dfmi_thermo_set_eos")
    cpu_a = ctypes.CDLL(os.path.join(ROOT, "baseline", "cpu_a", "libdfmi_cpu_a.so"))
    assert hasattr(cpu_a, "dfmi_thermo_set_eos")


def test_cpu_a_accepts_the_ideal_gas_and_refuses_peng_robinson_by_name():
    cpu_a = ctypes.CDLL(os.path.join(ROOT, "baseline", "cpu_a", "libdfmi_cpu_a.so"))
    h = ctypes.c_void_p()
    assert cpu_a.dfmi_create(ctypes.byref(h), 0) == 0
    dp = ctypes.POINTER(ctypes.c_double)
    cpu_a.dfmi_thermo_set_eos.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, dp, dp, dp]
    assert cpu_a.dfmi_thermo_set_eos(h, 0, 0, None, None, None) == 0
    one = (ctypes.c_double * 1)(1.0)
    assert cpu_a.dfmi_thermo_set_eos(h, 1, 1, one, one, one) != 0
    buf = ctypes.create_string_buffer(1024)
    cpu_a.dfmi_last_error(buf, 1024)
    assert b"dfmi_thermo_set_eos" in buf.value and b"Peng-Robinson" in buf.value
    cpu_a.dfmi_destroy(h)
