"""The mechanisms and the fixture of the chemistry sweep (tests/chem_mechs.py, tests/golden/chem_sweep_states.json), on the
CPU: the helpers build what they say, the fixture kept its caps, the generator reproduces it, and the oracle does not
care about the species order."""
import importlib.util
import json
import os

import numpy as np
import pytest

import chem_mechs as cm
from conftest import GOLDEN

# S -> (R, [elementary, three-body, Lindemann, Troe] or None): gri30 restricted to the first S species of chem_mechs.order()
TABLE = {4: (5, [3, 2, 0, 0]), 5: (6, [4, 2, 0, 0]), 6: (11, None), 7: (19, None), 8: (27, [21, 5, 0, 1]), 9: (28, None),
         10: (28, None), 11: (33, [26, 5, 1, 1]), 12: (40, [32, 6, 1, 1]), 13: (41, None), 16: (60, [49, 6, 1, 4]),
         17: (62, None), 32: (186, [158, 6, 1, 21]), 33: (192, None), 36: (219, None)}


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(GOLDEN, "chem_sweep_states.json")))


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_chem_sweep_fixtures", os.path.join(GOLDEN, "make_chem_sweep_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_prefix_table():
    for S, (R, ty) in TABLE.items():
        m, nasa, W, t = cm.prefix(S)
        assert (m.S, m.R) == (S, R) and m.species == cm.order()[:S]
        if ty is not None:
            assert cm.types(m) == ty
        assert nasa.shape == (S, 15) and W.shape == (S,) and t.S == S and t.bdiff.shape == (S, S, 5)
        # every species takes part in a reaction -- but CO at S = 10, which reacts only once CO2 has joined it at 11
        assert np.flatnonzero(~cm.reacting(m)).tolist() == ([9] if S == 10 else [])
    troe = cm.prefix(36)[0]
    assert np.all(troe.has_T2[troe.itype == 3] == 1)            # every Troe reaction of gri30 carries T2


def test_clones_top_rows_react():
    m64, m63 = cm.cloned(28, 11)[0], cm.cloned(27, 11)[0]
    assert (m64.S, m64.R, m63.S, m63.R) == (64, 252, 63, 252)
    for m in (m64, m63):
        on = cm.reacting(m)
        assert on.sum() == 47 and on[m.S - 11:].all() and not on[36:m.S - 11].any()
        assert on[m.S - m.S // 4:].sum() == 11 and on[m.S - 11:].all()      # the top quarter of the rows: its last 11 react
        assert m.species[m.S - 1] == "H_b" and m.species[36] == cm.order()[m.S - 37] + "_b"
    # the copies carry their origin's thermo rows and efficiency columns
    mt = cm.cloned(28, 11)
    assert np.array_equal(mt[1][63], mt[1][0]) and mt[2][63] == mt[2][0] and np.array_equal(mt[0].eff[:, 63], mt[0].eff[:, 0])
    assert np.array_equal(mt[3].bdiff[63, 5], mt[3].bdiff[0, 5])


def test_top_quarter_indices_take_part():
    """every row band a lane layout adds last (rows 48..63 at 16 lanes, 32..63 at 32) holds reacting species"""
    for n in (27, 28):
        m = cm.cloned(n, 11)[0]
        on = cm.reacting(m)
        assert on[48:].any() and on[32:48].any() and on[m.S - 11:].all()


def test_permuted_and_duplicates():
    mt = cm.prefix(12)
    perm = np.arange(12)[::-1]
    m, nasa, W, t = cm.permuted(mt, perm)
    assert m.species == mt[0].species[::-1] and np.array_equal(W, mt[2][::-1]) and np.array_equal(nasa, mt[1][::-1])
    assert np.array_equal(m.eff, mt[0].eff[:, ::-1]) and np.array_equal(t.bdiff, mt[3].bdiff[::-1, ::-1])
    r = 7
    assert [m.species[i] for i in m.reac[r] if i >= 0] == [mt[0].species[i] for i in mt[0].reac[r] if i >= 0]
    d = cm.with_duplicates(mt, 58)[0]
    assert d.R == 58 and np.array_equal(d.A[40:], d.A[:18]) and np.array_equal(d.reac[40:], d.reac[:18])
    assert (3 * d.R + d.S ** 2) * 64 * 8 == 162816 <= 160 * 1024 < (3 * 59 + d.S ** 2) * 64 * 8


def test_single_forms_pack_round_trip():
    from dfmi.kinetics import ND0
    keys = [k for k, _ in cm.single_variants()]
    assert len(keys) == 19 and "irreversible-irrev" not in keys
    for key, (m, nasa, W, t) in cm.single_variants():
        assert m.R == 1 and m.S >= 4 and t.S == m.S and (~cm.reacting(m)).any()
        idata, irs, d = m.pack()
        assert idata.shape == (1, 8) and irs.shape == (1, 6) and d.shape == (1, ND0 + m.S)
        assert idata[0, 0] == m.itype[0] and idata[0, 1] == m.reversible[0] and idata[0, 4] == m.has_T2[0]
        assert idata[0, 2] == (m.reac[0] >= 0).sum() and idata[0, 3] == (m.prod[0] >= 0).sum()
        assert np.array_equal(irs[0, :3], m.reac[0]) and np.array_equal(irs[0, 3:], m.prod[0])
        assert (d[0, 0], d[0, 1], d[0, 2]) == (m.A[0], m.b[0], m.Ta[0]) and (d[0, 9], d[0, 10], d[0, 11]) == (m.A0[0], m.b0[0], m.Ta0[0])
        assert np.array_equal(d[0, 3:6], m.nu_r[0]) and np.array_equal(d[0, 6:9], m.nu_p[0])
        assert np.array_equal(d[0, 12:16], m.troe[0]) and np.array_equal(d[0, ND0:], m.eff[0])
        assert m.reversible[0] == (0 if key.endswith("-irrev") or key == "irreversible" else 1)
    f = dict(cm.single_variants())
    assert f["nu2"][0].nu_r[0, 0] == 2 and f["h_2o2"][0].nu_r[0].tolist() == [1, 2, 0] and (f["three_products"][0].prod[0] >= 0).all()
    assert f["three_body"][0].itype[0] == 1 and (f["three_body"][0].eff[0] == 0).any()
    assert f["lindemann"][0].itype[0] == 2 and f["troe_T2"][0].has_T2[0] == 1
    assert f["troe_T2_cleared"][0].has_T2[0] == 0 and f["troe_T2_cleared"][0].troe[0, 3] == f["troe_T2"][0].troe[0, 3]
    assert f["burke_troe"][0].itype[0] == 3 and f["burke_troe"][0].has_T2[0] == 0


def test_fixture_caps(fixture):
    assert set(fixture["cases"]) == set(cm.SWEEP) and set(fixture["singles"]) == {k for k, _ in cm.single_variants()}
    for name, f in fixture["cases"].items():
        m = cm.case(name)[0]
        n = 4 if name == "p12x58" else 16
        assert (f["S"], f["R"], f["species"]) == (m.S, m.R, m.species)
        assert f["kept"] == n and f["examined"] - f["kept"] == f["dropped"] and f["dropped"] <= 0.1 * f["examined"]
        assert f["worst_kept"] <= 1e-6
        Y, RR = np.asarray(f["Y"]), np.asarray(f["RR"])
        assert Y.shape == RR.shape == (m.S, n) and np.all(np.isfinite(RR)) and len(f["T"]) == len(f["p"]) == len(f["rho"]) == n
        assert np.abs(Y.sum(axis=0) - 1).max() < 1e-12
        if n == 16:
            assert f["kind"] == ["broad"] * 12 + ["zero"] * 2 + ["negative"] * 2
            assert ((Y[:, 12:14] == 0).sum(axis=0) == m.S // 2).all() and ((Y[:, 14:] < 0).sum(axis=0) == m.S // 2).all()
            assert Y[:, :14].min() >= 0
        p = np.asarray(f["p"]) / cm.P_ATM
        assert 0.1 <= p.min() and p.max() <= 32 and (n < 16 or p.max() / p.min() > 30)
        assert 0 < f["tc_fp64_error"] < 1e-12
    for key, f in fixture["singles"].items():
        assert 0 < f["tc_fp64_error"] < 1e-12
        if key.split("-")[0] in cm.FALLOFF_FORMS:
            assert min(f["Pr_cells"]) > 0             # Pr < 1e-2, 0.1 < Pr < 10 and Pr > 1e2 are all sampled


def test_states_are_the_generators(fixture):
    """the committed states are what chem_mechs.sweep_candidates draws (nothing was dropped, so: its first ones)"""
    for name in ("p4", "p13", "c64"):
        f = fixture["cases"][name]
        assert f["dropped"] == 0
        T, p, rho, Y = cm.sweep_candidates(cm.case(name), "broad", 14, f["seed"])
        assert np.allclose(T[:12], f["T"][:12], rtol=1e-14) and np.allclose(Y[:, :12], np.asarray(f["Y"])[:, :12], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", [n for n, k in cm.SWEEP.items() if k[0] == "prefix" and k[1] <= 13])
def test_regenerated_rates(name, fixture, generator):
    """two states per mechanism through the generator's own function (S <= 13: the oracle costs seconds per state above)"""
    f = fixture["cases"][name]
    RR = np.asarray(f["RR"])
    scale = np.abs(RR).max()
    for c in (0, 13):
        rr = generator.reference_rr(name, f["T"][c], f["p"][c], f["rho"][c], np.asarray(f["Y"])[:, c])
        assert np.abs(rr - RR[:, c]).max() <= 1e-6 * scale


def test_oracle_is_permutation_equivariant(fixture):
    from chem_oracle import Kinetics
    f = fixture["cases"]["p12"]
    mt = cm.case("p12")
    perm = np.arange(12)[::-1]
    m, nasa, W, _ = cm.permuted(mt, perm)
    kin = Kinetics(m, nasa, W)
    RR, Y = np.asarray(f["RR"]), np.asarray(f["Y"])
    for c in (1, 14):
        rr = kin.reaction_rates(np.array([f["T"][c]]), np.array([f["p"][c]]), np.array([f["rho"][c]]), Y[perm][:, c:c + 1],
                                fixture["dt"], rtol=1e-11, atol=1e-22)[:, 0]
        assert np.abs(rr - RR[perm, c]).max() <= 1e-8 * np.abs(RR).max()
