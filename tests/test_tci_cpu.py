"""PaSR / EDC combustion closures, the parts that run without a GPU: the combustionProperties reader on the reference
case's file and its refusals by name, CPU-A's handling of the tci.* keys, header / export / binding parity of
dfmi_combustion_correct, the committed bounds file, and the NumPy restatement's own invariants (tests/tci_reference.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import tci_reference as R
from conftest import GOLDEN, ROOT

FIXTURE = os.path.join(GOLDEN, "combustionProperties_SandiaD")
TCI_DEFAULTS = {"tci.model": 0, "tci.mixing": 1, "tci.chemistry": 1, "tci.Cmix": 0.1, "tci.fuel": -1, "tci.oxidizer": -1,
                "tci.CO2": -1, "tci.H2": -1, "tci.version": 2005, "tci.C1": 0.05774, "tci.C2": 0.5, "tci.Cgamma": 2.1377,
                "tci.Ctau": 0.4083, "tci.exp1": 0, "tci.exp2": 0}


def _pasr(mix="globalScale", chem="formationRate", extra=""):
    return ("combustionModel PaSR;\nPaSRCoeffs\n{\n  mixingScale { type %s; %sCoeffs { Cmix 0.3; } }\n"
            "  chemistryScale { type %s; %s }\n}\n" % (mix, mix, chem, extra))


def test_parser_reads_the_reference_case():
    from dfmi import combustion as Cb
    s = Cb.read_combustion_properties(FIXTURE)
    assert s["combustionModel"] == "PaSR" and s["model"] == 1
    assert s["mixing"] == Cb.MIXING["globalScale"] == 1 and s["Cmix"] == 0.01
    assert s["chemistry"] == Cb.CHEMISTRY["globalConvertion"] == 1
    assert s["fuel"] == "CH4" and s["oxidizer"] == "O2"
    assert s["version"] == 2005 and s["exp1"] == 0 and s["exp2"] == 0
    assert (s["C1"], s["C2"], s["Cgamma"], s["Ctau"]) == (0.05774, 0.5, 2.1377, 0.4083)


def test_parser_variations():
    from dfmi import combustion as Cb
    # the comment after the model name decides nothing
    assert Cb.parse_combustion_properties("combustionModel EDC;//PaSR; laminar\nEDCCoeffs { version v2016; }\n")["model"] == 2
    assert Cb.parse_combustion_properties("combustionModel EDC;//PaSR\nEDCCoeffs { version v2016; }\n")["version"] == 2016
    assert Cb.parse_combustion_properties("combustionModel laminar;// EDC\n")["model"] == 0
    assert Cb.parse_combustion_properties("combustionModel  EDC ; /* PaSR; */\n")["version"] == 2005
    s = Cb.parse_combustion_properties("combustionModel EDC;\nEDCCoeffs { version v1981; Cgamma 2.0; Ctau 0.5; exp1 2; exp2 4; }\n")
    assert (s["version"], s["Cgamma"], s["Ctau"], s["exp1"], s["exp2"]) == (1981, 2.0, 0.5, 2, 4)
    s = Cb.parse_combustion_properties(_pasr("kolmogorovScale", "reactionRate"))
    assert (s["mixing"], s["chemistry"], s["Cmix"]) == (2, 3, 0.3)
    s = Cb.parse_combustion_properties(_pasr("geometriMeanScale", "globalConvertion", "globalConvertionCoeffs { fuel H2; oxidizer O2; }"))
    assert (s["mixing"], s["chemistry"], s["fuel"], s["oxidizer"]) == (3, 1, "H2", "O2")


@pytest.mark.parametrize("txt,name", [
    ("combustionModel flareFGM;\n", "flareFGM"), ("combustionModel DeePFGM;\n", "DeePFGM"),
    ("combustionModel infinitelyFastChemistry;\n", "infinitelyFastChemistry"), ("EDCCoeffs { version v2005; }\n", "combustionModel"),
    (_pasr("dynamicScale"), "dynamicScale"), (_pasr("integralScale"), "integralScale"), (_pasr(chem="eigenvalue"), "eigenvalue"),
    (_pasr(chem="globalConvertion"), "fuel"), ("combustionModel PaSR;\n", "PaSRCoeffs"),
    ("combustionModel EDC;\nEDCCoeffs { version v2020; }\n", "v2020"), ("combustionModel EDC;\nEDCCoeffs { Cgamma -1; }\n", "Cgamma"),
    ("combustionModel EDC;\nEDCCoeffs { exp1 5; }\n", "exp1"), ("combustionModel EDC;\nEDCCoeffs { Ctheta 1; }\n", "Ctheta")])
def test_parser_refusals_name_their_entry(txt, name):
    from dfmi import combustion as Cb
    with pytest.raises(ValueError, match=name):
        Cb.parse_combustion_properties(txt)


class _Rec:
    def __init__(self):
        self.opts = {}

    def set_option(self, k, v):
        self.opts[k] = v


def test_apply_maps_species_names_to_indices():
    from dfmi import combustion as Cb
    names = ["H2", "O2", "CH4", "CO2", "N2"]
    r = _Rec()
    Cb.apply_combustion(r, Cb.read_combustion_properties(FIXTURE), names)
    assert r.opts["tci.model"] == 1 and r.opts["tci.fuel"] == 2 and r.opts["tci.oxidizer"] == 1
    assert r.opts["tci.CO2"] == 3 and r.opts["tci.H2"] == 0 and r.opts["tci.Cmix"] == 0.01
    assert list(r.opts)[-1] == "tci.model"                       # the model last: every other key is in place when it switches on
    r = _Rec()
    Cb.apply_combustion(r, Cb.read_combustion_properties(FIXTURE), ["CH4", "O2", "N2"])   # no CO2, no H2: left out
    assert r.opts["tci.CO2"] == -1 and r.opts["tci.H2"] == -1
    with pytest.raises(ValueError, match="CH4"):
        Cb.apply_combustion(_Rec(), Cb.read_combustion_properties(FIXTURE), ["H2", "O2", "N2"])
    r = _Rec()
    Cb.apply_combustion(r, Cb.parse_combustion_properties("combustionModel laminar;\n"), names)
    assert r.opts == {"tci.model": 0}


def test_header_export_and_binding():
    from dfmi import lib
    from test_cpu_a import CPU_A
    hdr = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    assert re.search(r"\bint\s+dfmi_combustion_correct\s*\(\s*dfmi_ctx\s*\*\s*ctx\s*,\s*double\s+dt\s*\)\s*;", hdr)
    assert lib.SIGNATURES["dfmi_combustion_correct"] == [lib._P, ctypes.c_double]
    assert "dfmi_combustion_correct" in lib.exported_symbols()
    assert hasattr(ctypes.CDLL(CPU_A), "dfmi_combustion_correct")
    assert hasattr(lib.load(), "dfmi_combustion_correct")        # the HIP library (loads without a device)
    for key in list(TCI_DEFAULTS) + ["tci.bad_tauStar", "tci_kappa", "tci_tmix", "tci_tauStar", "tci_tc", "RR_eff", "Qdot_eff"]:
        assert key in hdr, key
    for tok in ("PaSR.C:205-396", "EDC.C:83-171", "tc / (tc + tmix)", "sumW / sumSq * cSum", "gammaL^exp1 / (1 - gammaL^exp2)",
                "Ctau sqrt(nu / (eps + small))", "dynamicScale"):
        assert tok in hdr, tok


def test_cpu_a_keeps_the_keys_and_refuses_the_models():
    from dfmi.lib import DfmiError
    from test_cpu_a import _case
    ctx = _case(False)[0]
    try:
        for key, v in TCI_DEFAULTS.items():
            assert ctx.get_option(key) == v, key
        ctx.set_option("tci.model", 0)
        ctx.set_option("tci.Cmix", 0.01)
        ctx.set_option("tci.fuel", 3)
        ctx.set_option("tci.version", 2016)
        ctx.set_option("tci.exp1", 4)
        assert (ctx.get_option("tci.Cmix"), ctx.get_option("tci.fuel"), ctx.get_option("tci.version"), ctx.get_option("tci.exp1")) == \
            (0.01, 3, 2016, 4)
        for v in (1, 2):
            with pytest.raises(DfmiError, match="tci.model"):
                ctx.set_option("tci.model", v)
        for key, bad, word in (("tci.model", 3, "tci.model"), ("tci.mixing", 4, "dynamicScale"), ("tci.mixing", 0, "tci.mixing"),
                               ("tci.chemistry", 4, "tci.chemistry"), ("tci.version", 2000, "tci.version"), ("tci.exp2", 5, "tci.exp2"),
                               ("tci.exp1", 1.5, "tci.exp1"), ("tci.Cmix", 0.0, "tci.Cmix"), ("tci.Ctau", float("inf"), "tci.Ctau"),
                               ("tci.fuel", -2, "tci.fuel"), ("tci.H2", 0.5, "tci.H2"), ("tci.nope", 1.0, "tci.nope"),
                               ("tci.bad_tauStar", 1.0, "tci.bad_tauStar")):
            with pytest.raises(DfmiError, match=word):
                ctx.set_option(key, bad)
        assert ctx.get_option("tci.model") == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_fp64_restatement_within_committed_bounds():
    bounds = R.load_bounds()["mechanisms"]
    measured = R.measure()
    assert set(measured) == set(bounds) == set(R.MECHS)
    for mech, per_cls in measured.items():
        assert set(per_cls) == set(bounds[mech])
        for cls, per_q in per_cls.items():
            assert set(per_q) == set(bounds[mech][cls])
            for q, v in per_q.items():
                assert np.isfinite(v) and v <= bounds[mech][cls][q], (mech, cls, q, v)
                assert v < 1e-12, (mech, cls, q, v)               # every quantity is well conditioned


@pytest.fixture(scope="module")
def burke():
    species, m, nasa, W = R.load_mech("burke9")
    return species, m, nasa, W


def test_kappa_lies_in_the_unit_interval(burke):
    species, m, nasa, W = burke
    S = len(species)
    idx = R.species_idx(species)
    for st, coef in ((R.broad(400, S, W), None), (R.branches_pasr(400, S, W, idx), {"Cmix": 1e-15}),
                     (R.branches_edc(400, S, W), {"Cgamma": 1.0})):
        for T in (np.float64, R.LD):
            for mixing in (1, 2, 3):
                for chem in (1, 2):
                    kap = R.evaluate_pasr(st, mixing, chem, idx, coef, T=T)["tci_kappa"]
                    assert np.all((kap >= 0) & (kap <= 1))
            for ver in R.VERSION_EXP:
                for e1, e2 in ((0, 0), (1, 4), (4, 1)):
                    out = R.evaluate_edc(st, ver, coef, e1, e2, T=T)
                    fin = np.isfinite(np.asarray(out["tci_kappa"], dtype=np.float64))
                    assert fin.sum() >= 399                      # the mu = 0 cell of branches_edc may give 0 / 0 in v2016
                    assert np.all((out["tci_kappa"][fin] >= 0) & (out["tci_kappa"][fin] <= 1))


def test_gammaL_at_or_above_one_gives_one(burke):
    species, m, nasa, W = burke
    st = R.branches_edc(64, len(species), W)
    for T in (np.float64, R.LD):
        for ver in (1981, 1996, 2005):
            kap, tau, g = R.edc(ver, {"Cgamma": 1.0}, 0, 0, st["k"], st["epsilon"], st["mu"], st["rho"], T=T)
            assert g[0] == 1 and g[1] > 1 and g[2] < 1           # the three hand-built cells: at, above, below
            assert kap[0] == 1 and kap[1] == 1
            assert np.all(kap[g >= 1] == 1)
    kap, _, g = R.edc(2005, {"Cgamma": 50.0}, 0, 0, st["k"], st["epsilon"], st["mu"], st["rho"])
    assert (g >= 1).sum() > 10 and np.all(kap[g >= 1] == 1.0)


def test_vgreat_gives_kappa_exactly_one(burke):
    species, m, nasa, W = burke
    S = len(species)
    st = R.broad(8, S, W)
    R.inert_cell(st, 3, S, species.index("N2"))
    for T in (np.float64, R.LD):
        tc = R.tc_reaction(m, nasa, W, st["T"], st["p"], st["rho"], st["Y"], T=T)
        assert tc[3] == T(R.VGREAT) and np.all(tc[np.arange(8) != 3] < 1e100) and np.all(tc > 0)
        for mixing in (1, 2, 3):
            tm = R.tmix_of(mixing, 0.1, st["k"], st["epsilon"], st["mu"], st["rho"], T)
            assert R.kappa_pasr(tm, tc, T)[3] == 1.0
    assert R.kappa_pasr(np.array([1e3]), np.array([R.VGREAT]))[0] == 1.0


def test_split_rates_difference_is_the_oracles_rate_of_progress(burke):
    """fwd - rev of the split restatement against chem_oracle.Kinetics.rates_of_progress (another operation order: 1e-12)"""
    from chem_oracle import Kinetics
    species, m, nasa, W = burke
    st = R.broad(6, len(species), W)
    kin = Kinetics(m, nasa, W)
    for c in range(6):
        rho, y = kin.reactor_state(st["T"][c], st["p"][c], st["Y"][:, c])
        C = rho * y / W
        fwd, rev = R.fwd_rev(m, nasa, st["T"][c], list(C))
        q = kin.rates_of_progress(st["T"][c], C)
        fwd, rev = np.array(fwd), np.array(rev)
        assert np.all(fwd >= 0) and np.all(rev >= 0)
        assert np.all(rev[np.asarray(m.reversible) == 0] == 0)
        assert np.abs((fwd - rev) - q).max() <= 1e-12 * np.maximum(fwd, rev).max()


def test_branch_states_sit_on_or_clear_of_every_comparison(burke):
    species, m, nasa, W = burke
    S = len(species)
    idx = R.species_idx(species)
    st = R.branches_pasr(300, S, W, idx)
    for chem in (1, 2):
        c64, cLD = [], []
        R.evaluate_pasr(st, 1, chem, idx, {"Cmix": 1e-15}, cmp=c64)
        R.evaluate_pasr(st, 1, chem, idx, {"Cmix": 1e-15}, T=R.LD, cmp=cLD)
        assert R.branch_report(c64, cLD) == []
    st = R.branches_edc(300, S, W)
    for ver in R.VERSION_EXP:
        c64, cLD = [], []
        R.evaluate_edc(st, ver, {"Cgamma": 1.0}, cmp=c64)
        R.evaluate_edc(st, ver, {"Cgamma": 1.0}, T=R.LD, cmp=cLD)
        assert R.branch_report(c64, cLD) == []
