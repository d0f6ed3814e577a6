"""flareFGM without a GPU (include/dfmi.h, flareFGM block): the table file format, the flareFGMCoeffs
parser and their refusals, the NumPy restatement of the retrieval (tests/fgm_reference.py) against hand-evaluated
corners and the properties of multilinear interpolation, the drawn state classes' drop cap, the committed chi_c
bounds, and the exports of the three new entries by the header, the binding and both libraries."""
import ctypes
import json
import os

import numpy as np
import pytest

import fgm_reference as FR
from conftest import ROOT
from dfmi import fgm


# ------------------------------------------------------------------------------------------------ table files
@pytest.mark.parametrize("name", ["full", "full_u", "four_d", "full_u_deg"])
def test_table_write_read_round_trip_is_bitwise(tmp_path, name):
    t = FR.make_table(name)
    p = str(tmp_path / "flare.tbl")
    fgm.write_table(p, t)
    r = fgm.read_table(p)
    assert r.dims() == t.dims() and r.scaled == t.scaled
    assert r.omega_names == t.omega_names and r.species_names == t.species_names
    assert (r.Hfu, r.Hox) == (t.Hfu, t.Hox)
    for a, b in zip(r.axes, t.axes):
        assert np.array_equal(a, b)
    assert np.array_equal(r.laminar, t.laminar) and np.array_equal(r.values, t.values)
    if t.scaled:
        assert np.array_equal(r.d2Yeq, t.d2Yeq) and np.array_equal(r.d1Yeq, t.d1Yeq)
    else:
        assert r.d2Yeq is None and r.d1Yeq is None
    assert len(r.table_names()) == t.NS + t.NY
    # a second write of what was read is the same file
    p2 = str(tmp_path / "again.tbl")
    fgm.write_table(p2, r)
    assert open(p).read() == open(p2).read()


def _lines(tmp_path, name="full"):
    p = str(tmp_path / "t.tbl")
    fgm.write_table(p, FR.make_table(name))
    return p, open(p).read().split("\n")


def _rewrite(p, lines):
    with open(p, "w") as f:
        f.write("\n".join(lines))


def test_reader_refusals_by_name(tmp_path):
    with pytest.raises(ValueError, match="no such file"):
        fgm.read_table(str(tmp_path / "missing.tbl"))
    p, L = _lines(tmp_path)
    cases = [
        (lambda l: [" ".join(l[0].split()[:9])] + l[1:], "needs 10 values"),
        (lambda l: [l[0].replace("3 5", "3 x", 1)] + l[1:], "not ten integers"),
        (lambda l: ["0 " + " ".join(l[0].split()[1:])] + l[1:], "dimension NH = 0"),
        (lambda l: [" ".join(l[0].split()[:9] + ["1"])] + l[1:], "NZL = 1"),
        (lambda l: [" ".join(l[0].split()[:6] + ["12"] + l[0].split()[7:])] + l[1:], "NS = 12 must be 8 \\+ NYomega"),
        (lambda l: [l[0], ""] + l[2:], "source-term species names needs 1 values"),
        (lambda l: [l[0], l[1], "O2 H2O"] + l[3:], "species names needs 3 values"),
        (lambda l: l[:3] + ["abc"] + l[4:], "axis h holds a value that is not a number"),
        (lambda l: l[:40], "the file ends before"),
        (lambda l: l[:-2] + ["1.0", ""], "non-premixed block .* needs 2 values"),
    ]
    for edit, msg in cases:
        _rewrite(p, edit(list(L)))
        with pytest.raises(ValueError, match=msg):
            fgm.read_table(p)


PROPS = """
combustionModel  flareFGM;//PaSR;
EDCCoeffs { version v2005; }
flareFGMCoeffs
{
  nOmega_Yis        1;
  omega_YiNames (CH4);
  scaledPV         true;
  combustion       true;
  solveEnthalpy    true;
  flameletT        false;
  relaxation       false;
  DpDt             false;
  buffer           false;
  bufferTime       0.0;
  ignition         false;
  /* ignBeginTime     0.0; */
  Sct              0.7;
  tablePath    flare_CH4_SandiaD_4D.tbl;
}
"""


def test_parser_reads_the_shipped_case_form():
    s = fgm.parse_fgm_properties(PROPS)
    assert s["model"] == 1 and s["combustionModel"] == "flareFGM"
    assert s["scaledPV"] and s["combustion"] and s["solveEnthalpy"] and not s["flameletT"]
    assert s["Sct"] == 0.7 and s["Sc"] == 1.0 and s["incompPref"] == -10.0 and (s["TMin"], s["TMax"]) == (200.0, 5000.0)
    assert s["tablePath"] == "flare_CH4_SandiaD_4D.tbl" and s["omega_YiNames"] == ["CH4"]
    fgm.parse_fgm_properties(PROPS, FR.make_table("full"))          # agrees with the table
    s2 = fgm.parse_fgm_properties(PROPS.replace("Sct              0.7;", "Sct 0.9; Sc 0.8; incompPref 101325; p_operateDim 101325; TMin 250; TMax 3000;"))
    assert (s2["Sct"], s2["Sc"], s2["incompPref"], s2["TMin"], s2["TMax"]) == (0.9, 0.8, 101325.0, 250.0, 3000.0)


@pytest.mark.parametrize("old,new,msg", [
    ("combustionModel  flareFGM", "combustionModel  DeePFGM", "DeePFGM is not supported"),
    ("combustionModel  flareFGM", "combustionModel  PaSR", "PaSR is not flareFGM"),
    ("combustionModel  flareFGM;", "", "no combustionModel entry"),
    ("flareFGMCoeffs", "otherCoeffs", "without a flareFGMCoeffs"),
    ("buffer           false", "buffer           true", "buffer true is not supported"),
    ("bufferTime       0.0", "bufferTime       0.4", "bufferTime 0.4 > 0 is not supported"),
    ("relaxation       false", "relaxation       true", "relaxation true is not supported"),
    ("DpDt             false", "DpDt             true", "DpDt true is not supported"),
    ("ignition         false", "ignition         true", "ignition true is not supported"),
    ("Sct              0.7;", "Sct 0.7; incompPref 101325; p_operateDim 100000;", "p_operateDim 100000.0 differs from incompPref"),
    ("Sct              0.7;", "Sct -1;", "Sct -1 must be positive"),
    ("Sct              0.7;", "Sct 0.7; LESdelta 1;", "entry LESdelta is not supported"),
    ("combustion       true", "combustion       maybe", "is not a switch"),
    ("omega_YiNames (CH4)", "omega_YiNames CH4", "is not a word list"),
])
def test_parser_refusals_by_name(old, new, msg):
    assert old in PROPS
    with pytest.raises(ValueError, match=msg):
        fgm.parse_fgm_properties(PROPS.replace(old, new))


def test_parser_refuses_what_disagrees_with_the_table():
    with pytest.raises(ValueError, match="omega_YiNames \\(O2\\) disagrees with the table's \\(CH4\\)"):
        fgm.parse_fgm_properties(PROPS.replace("(CH4)", "(O2)"), FR.make_table("full"))
    with pytest.raises(ValueError, match="scaledPV true disagrees with the table"):
        fgm.parse_fgm_properties(PROPS, FR.make_table("full_u"))
    with pytest.raises(ValueError, match="species H2O is not a species of the mechanism"):
        fgm.species_indices(FR.make_table("full"), ["CH4", "O2", "N2"])
    assert fgm.species_indices(FR.make_table("full"), ["N2", "CO2", "H2O", "O2", "CH4"]) == ([3, 2, 1], [4])


def test_read_case_fgm(tmp_path):
    os.makedirs(tmp_path / "constant")
    (tmp_path / "constant" / "combustionProperties").write_text(PROPS)
    fgm.write_table(str(tmp_path / "flare_CH4_SandiaD_4D.tbl"), FR.make_table("full"))
    s, t = fgm.read_case_fgm(str(tmp_path))
    assert s["combustion"] and t.dims() == FR.make_table("full").dims()
    # combustion.parse_combustion_properties keeps refusing the FGM models: they have their own module
    from dfmi.combustion import parse_combustion_properties
    with pytest.raises(ValueError, match="flareFGM is not supported"):
        parse_combustion_properties(PROPS)


# ------------------------------------------------------------------------------------------------ the restatement
def _node_value(tab, v, idx):
    return np.asarray(tab.values[v]).reshape(tab.shape)[tuple(idx)]


@pytest.mark.parametrize("name", FR.TABLES)
def test_restatement_at_nodes_is_the_hand_evaluated_corner(name):
    """every coordinate exactly on a node: each lookup is the table's own entry there, read by hand"""
    tab = FR.make_table(name)
    st, dropped = FR.states(name, "nodes")
    assert dropped <= FR.MAX_DROPPED
    r = FR.retrieve(tab, {}, st)
    coords = (r["Ha_s"], st["Z"], r["c_s"], r["Zvar_s"], r["cvar_s"], r["Zcvar_s"])
    idx = []
    for d, x in enumerate(coords):
        a = tab.axes[d]
        idx.append(np.zeros(len(x), int) if len(a) == 1 else np.array([int(np.nonzero(a == v)[0][0]) for v in x]))
    idx = np.array(idx).T
    seen_first, seen_last = set(), set()
    for i, ix in enumerate(idx):
        for d in range(6):
            if ix[d] == 0:
                seen_first.add(d)
            if ix[d] == len(tab.axes[d]) - 1:
                seen_last.add(d)
        assert r["Wt"][i] == _node_value(tab, 4, ix)
        assert r["mu"][i] == _node_value(tab, 7, ix) * st["rho"][i]
        assert r["Cp"][i] == _node_value(tab, 3, ix) and r["Hf"][i] == _node_value(tab, 5, ix)
        for j in range(tab.NY):
            assert r["Y"][j, i] == _node_value(tab, tab.NS + j, ix)
        for j in range(tab.NYomega):
            assert r["omega_Yi"][j, i] == _node_value(tab, tab.NS - tab.NYomega + j, ix)
        if r["flame"][i] and not tab.scaled:
            assert r["cOmega_c"][i] == _node_value(tab, 1, ix) * st["rho"][i]
    multi = {d for d in range(6) if len(tab.axes[d]) > 1}
    assert seen_first == set(range(6)) and multi <= seen_last | ({2} if not tab.scaled else set())


def test_affine_table_is_interpolated_exactly_and_factors_sum_to_one():
    rng = np.random.default_rng(3)
    tab = FR.make_table("full")
    n = 400
    x = [rng.uniform(a[0] - 0.1 * (a[-1] - a[0]), a[-1] + 0.1 * (a[-1] - a[0]), n) for a in tab.axes]
    pairs = [FR.pair(a, v) for a, v in zip(tab.axes, x)]
    fac = FR.corner_factors([p[1] for p in pairs])
    assert np.abs(fac.sum(axis=0) - 1.0).max() <= 4 * np.finfo(float).eps      # partition of unity
    assert fac.min() >= 0.0
    g = np.meshgrid(*tab.axes, indexing="ij")
    coef = rng.uniform(-2, 2, 7)
    scale = [max(abs(a[0]), abs(a[-1])) for a in tab.axes]
    affine = coef[0] + sum(coef[d + 1] * g[d] / scale[d] for d in range(6))
    got = FR.lookup_nd(tab.shape, pairs, affine.reshape(-1))
    xc = [np.clip(v, a[0], a[-1]) for a, v in zip(tab.axes, x)]      # outside the axis the lookup holds the end value
    want = coef[0] + sum(coef[d + 1] * xc[d] / scale[d] for d in range(6))
    # rounding of the restatement itself: a factor is five products of weights that each carry two roundings (<= 8 eps),
    # and the sum runs over 64 non-negative terms in sequence (<= 32 eps of the sum of magnitudes): 40 eps in all
    tol = 40 * np.finfo(float).eps
    assert np.abs(got - want).max() <= tol * np.abs(coef).sum()
    const = FR.lookup_nd(tab.shape, pairs, np.full(tab.size, 3.25))
    assert np.abs(const - 3.25).max() <= tol * 3.25


def test_length_one_axis_has_factor_zero():
    """the deliberate deviation: fac = 0 exactly on an axis of length 1, whatever x (the reference reads a[1] there)"""
    loc, fac = FR.pair(np.array([0.25]), np.array([-1.0, 0.25, 7.0, np.nan]))
    assert not loc.any() and not fac.any()
    tab = FR.make_table("four_d")
    st, _ = FR.states("four_d", "interior")
    r = FR.retrieve(tab, {}, st)
    st2 = dict(st, Ha=st["Ha"] - 1.0e4)                  # h has one node: hLoss is clamped to it, nothing moves
    r2 = FR.retrieve(tab, {}, st2)
    assert np.array_equal(r["Wt"], r2["Wt"]) and np.array_equal(r["Y"], r2["Y"]) and not r2["Ha_s"].any()
    for d in (0, 4, 5):
        assert not r["pairs"][d][0].any() and not r["pairs"][d][1].any()


@pytest.mark.parametrize("name", FR.TABLES)
@pytest.mark.parametrize("cls", FR.CLASSES)
def test_state_classes_hold_what_they_promise(name, cls):
    tab = FR.class_table(name, cls)
    st, dropped = FR.states(name, cls)
    assert dropped <= FR.MAX_DROPPED and len(st["Z"]) >= FR.N_STATES - FR.MAX_DROPPED
    with np.errstate(all="ignore"):
        r = FR.retrieve(tab, {}, st)
    ax = tab.axes
    coords = (r["Ha_s"], st["Z"], r["c_s"], r["Zvar_s"], r["cvar_s"], r["Zcvar_s"])
    if cls == "interior":
        assert r["flame"].sum() > 60
    elif cls == "outside":
        for d in (1, 2):
            assert (coords[d] < ax[d][0]).any() and (coords[d] > ax[d][-1]).any(), d
        for d in (3, 4, 5):
            if len(ax[d]) > 1:
                assert (coords[d] > ax[d][-1]).any(), d
        if len(ax[5]) > 1:
            assert (coords[5] < ax[5][0]).any()
        raw = (st["Z"] * (tab.Hfu - tab.Hox) + tab.Hox) - st["Ha"]
        assert (raw < ax[0][0]).any() and (raw > ax[0][-1]).any()
    elif cls == "no_flame":
        n = len(st["Z"])
        assert not r["flame"][: n // 3].any() and not r["flame"][n // 3: 2 * (n // 3)].any() and r["flame"][2 * (n // 3):].any()
        assert not FR.retrieve(tab, {"combustion": 0}, st)["flame"].any()
    elif cls == "degenerate":
        Z, c = st["Z"], st["c"]
        assert ((Z < 1e-4) | (Z > 1 - 1e-4)).any() and (c < 1e-4).any()
        assert (st["cvar"] < 1e-4).any() and (st["Zvar"] < 1e-6).any()
        assert (np.abs(st["Zcvar"]) > np.sqrt(st["Zvar"]) * np.sqrt(st["cvar"])).any() and (np.abs(r["Zcvar_s"]) == 1.0).any()
        if not tab.scaled:
            assert np.asarray(tab.values[tab.NS - 1]).min() <= 1e-6      # a corner with Ycmax <= 1e-6 ...
            zero = np.zeros_like(Z)
            q = (r["pairs"][0], r["pairs"][1], FR.pair(ax[2], zero), r["pairs"][3], FR.pair(ax[4], zero), FR.pair(ax[5], zero))
            assert (FR.lookup_nd(tab.shape, q, tab.values[tab.NS - 1]) < 0.02).any()      # ... and points that reach towards it


def test_committed_chi_c_bounds_are_reproduced():
    """tests/golden/fgm_point_bounds.json is what `python tests/fgm_reference.py --measure` writes: the fp64
    restatement of RANSsdrFLRmodel against long double. libm's pow and sqrt may move the last digit between hosts, so a
    maximum is held to a factor 2 either way where it matters to a tolerance (above a quarter of gpu_bound's 1e-13
    floor); every measured maximum is far below the floor, which therefore decides the device bound."""
    doc = FR.load_bounds()
    fresh = json.loads(json.dumps(FR.measure()))
    assert set(fresh) == set(doc["tables"]) == set(FR.TABLES)
    for name, per in fresh.items():
        assert set(per) == set(doc["tables"][name]) == set(FR.CLASSES)
        for cls, v in per.items():
            w = doc["tables"][name][cls]
            assert (v["states"], v["dropped"], v["flame_points"]) == (w["states"], w["dropped"], w["flame_points"]), (name, cls)
            a, b = v["chi_c"], w["chi_c"]
            assert max(a, b) <= 2.5e-14 or (a <= 2 * b and b <= 2 * a), (name, cls, a, b)
            assert v["flame_points"] > 30 and FR.gpu_bound(doc, name, cls) == 1e-13


def test_long_double_restatement_agrees_with_float64():
    """the same code in long double: the lookups agree to a few float64 ulp of their scale wherever both locate the same cell"""
    tab = FR.make_table("full")
    st, _ = FR.states("full", "interior")
    r64, rL = FR.retrieve(tab, {}, st), FR.retrieve(tab, {}, st, T=FR.LD)
    same = np.ones(len(st["Z"]), bool)
    for d in range(6):
        same &= r64["pairs"][d][0] == rL["pairs"][d][0]
    assert same.sum() >= 0.95 * same.size
    for n in ("Wt", "T", "psi", "omega_c"):
        e = np.abs(np.asarray(rL[n], np.float64) - r64[n])[same] / np.abs(r64[n]).max()
        assert e.max() <= 1e-13, (n, e.max())


def test_oracle_with_a_constant_table_is_pure_transport_of_z():
    """FgmOracle, a table constant in every variable, combustion off: the scalars see no source, so with the density of
    the rhoEqn a uniform Z stays uniform (the discrete continuity equation is the Z equation of a constant) and Zvar
    stays 0, a non-uniform Z stays inside its bounds (implicit upwind), and the retrieval returns the constants"""
    import ras_reference as R
    m = R.get_mesh("walls")
    C_, B = m.n_cells, m.n_boundary_slots
    t, st, pt, inert = FR.cpu_state(m)
    tab = FR.make_table("full")
    import copy
    ct = copy.copy(tab)
    const = np.array([0.0, 0.0, 0.0, 1200.0, 27.5, -3.0e5, 900.0, 2.0e-5, 0.0, 0.1, 0.2, 0.3])
    ct.values = np.repeat(const[:, None], tab.size, axis=1)
    ct.d2Yeq, ct.d1Yeq = np.zeros_like(tab.d2Yeq), np.zeros_like(tab.d1Yeq)
    zg = m.patch_types(0)
    x = m.cell_centres[:, 0] / m.cell_centres[:, 0].max()
    for Z0 in (np.full(C_, 0.3), 0.2 + 0.5 * x):
        from dfmi import case
        fields = {"Z": Z0, "Zvar": np.zeros(C_), "c": np.full(C_, 0.4), "cvar": np.zeros(C_), "Zcvar": np.zeros(C_),
                  "Ha": Z0 * (tab.Hfu - tab.Hox) + tab.Hox}
        for n in list(fields):
            fields["boundary_" + n] = case.boundary_values(m, fields[n]).reshape(-1)
        o = FR.make_oracle(m, t, {k: v.copy() for k, v in st.items() if not k.startswith("ras_")}, dict(pt), inert, 1e6, {},
                           st["ras_k"], st["ras_epsilon"], st["ras_boundary_k"], st["ras_boundary_epsilon"], ct,
                           {"combustion": 0, "solveEnthalpy": 0}, fields, {n: zg for n in FR.EQS}, [8, 6, 4],
                           k_ptypes=zg, eps_ptypes=zg)
        o.rho_eqn()                                   # rho consistent with rho_old and phi
        o.fgm_correct()
        a = o.arr
        assert np.abs(o.matrices["Z"]["Su"]).max() == 0
        if Z0.min() == Z0.max():
            assert np.abs(a["Z"] - 0.3).max() <= 1e-12
            # Zvar's production 2 mut / Sct |grad Z|^2 of a uniform Z: the Gauss gradient's rounding residue, squared
            assert np.abs(o.matrices["Zvar"]["Su"]).max() <= 1e-20 and np.abs(a["Zvar"]).max() <= 1e-25
        else:
            assert a["Z"].min() >= Z0.min() - 1e-12 and a["Z"].max() <= Z0.max() + 1e-12 and np.abs(a["Z"] - Z0).max() > 1e-6
        assert np.array_equal(a["c"], fields["c"]) and a["Zvar"].min() >= 0.0
        assert np.array_equal(a["Ha"], a["Z"] * (tab.Hfu - tab.Hox) + tab.Hox)
        for n, v in (("Wt", 27.5), ("Cp", 1200.0), ("Hf", -3.0e5)):
            assert np.abs(a[n] / v - 1).max() <= 1e-14, n
        T = np.clip((a["Ha"] + 3.0e5) / 1200.0 + 298.15, 200.0, 5000.0)
        assert np.abs(a["T"] / T - 1).max() <= 1e-13
        assert np.abs(a["psi"] / (27.5 / (8.314e3 * a["T"])) - 1).max() <= 1e-14
        assert np.array_equal(a["rho"], a["p"] * a["psi"]) and np.array_equal(a["rho_thermo"], a["rho"])
        assert np.abs(a["Y"][8] - 0.1).max() <= 1e-15 and np.abs(a["Y"][4] - 0.3).max() <= 1e-15
        assert not a["omega_c"].any()


# ------------------------------------------------------------------------------------------------ exports
NEW = ("dfmi_fgm_set_table", "dfmi_fgm_retrieve", "dfmi_fgm_correct")


def test_new_symbols_are_exported_by_header_binding_and_both_libraries():
    with open(os.path.join(ROOT, "include", "dfmi.h")) as f:
        hdr = f.read()
    from dfmi import lib
    cpu_a = ctypes.CDLL(os.path.join(ROOT, "baseline", "cpu_a", "libdfmi_cpu_a.so"))
    for s in NEW:
        assert f"int {s}(dfmi_ctx* ctx" in hdr
        assert s in lib.exported_symbols()
        assert hasattr(lib.load(), s) and hasattr(cpu_a, s)


def test_cpu_a_keeps_the_keys_and_refuses_the_model_by_name():
    cpu_a = ctypes.CDLL(os.path.join(ROOT, "baseline", "cpu_a", "libdfmi_cpu_a.so"))
    h = ctypes.c_void_p()
    assert cpu_a.dfmi_create(ctypes.byref(h), 0) == 0
    cpu_a.dfmi_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double]
    cpu_a.dfmi_get_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)]
    buf = ctypes.create_string_buffer(1024)
    v = ctypes.c_double()
    for key, dflt in (("fgm.model", 0), ("fgm.combustion", 0), ("fgm.solveEnthalpy", 0), ("fgm.flameletT", 0), ("fgm.Sct", 0.7),
                      ("fgm.Sc", 1.0), ("fgm.incompPref", -10.0), ("fgm.TMin", 200.0), ("fgm.TMax", 5000.0)):
        assert cpu_a.dfmi_get_option(h, key.encode(), ctypes.byref(v)) == 0 and v.value == dflt, key
    assert cpu_a.dfmi_set_option(h, b"fgm.Sct", 0.9) == 0 and cpu_a.dfmi_set_option(h, b"fgm.combustion", 1.0) == 0
    assert cpu_a.dfmi_set_option(h, b"fgm.incompPref", 101325.0) == 0 and cpu_a.dfmi_set_option(h, b"fgm.model", 0.0) == 0
    assert cpu_a.dfmi_get_option(h, b"fgm.Sct", ctypes.byref(v)) == 0 and v.value == 0.9
    assert cpu_a.dfmi_set_option(h, b"fgm.model", 1.0) != 0
    cpu_a.dfmi_last_error(buf, 1024)
    assert b"fgm.model = 1" in buf.value and b"flareFGM" in buf.value
    assert cpu_a.dfmi_set_option(h, b"fgm.no_such_key", 1.0) != 0
    cpu_a.dfmi_last_error(buf, 1024)
    assert b"fgm.no_such_key" in buf.value
    assert cpu_a.dfmi_set_option(h, b"fgm.Sct", -1.0) != 0
    for s in ("dfmi_fgm_retrieve", "dfmi_fgm_correct"):
        getattr(cpu_a, s).argtypes = [ctypes.c_void_p]
        assert getattr(cpu_a, s)(h) != 0
        cpu_a.dfmi_last_error(buf, 1024)
        assert s.encode() in buf.value and b"flareFGM" in buf.value
    cpu_a.dfmi_destroy(h)


def test_option_keys_and_scheme_terms_are_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in ("fgm.model", "fgm.combustion", "fgm.solveEnthalpy", "fgm.flameletT", "fgm.Sct", "fgm.Sc", "fgm.incompPref",
                "fgm.TMin", "fgm.TMax"):
        assert f"`{key}`" in doc, key
    for t in fgm.SCHEME_TERMS:
        assert t in doc, t
