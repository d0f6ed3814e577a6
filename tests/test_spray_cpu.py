"""Spray coupling, the parts that run without a GPU: the sprayCloudProperties reader on the two reference cases' files and
its refusals by name, apply_spray's key order, CPU-A's handling of the spray.* keys and the field names, the header /
option table / documents naming every key and field, the committed bounds of the NumPy term functions against
numpy.longdouble, and the terms' zero cases (tests/spray_reference.py)."""
import json
import os

import numpy as np
import pytest

import spray_reference as R
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("spray.model", "spray.rho", "spray.U", "spray.Yi", "spray.h")
FIELDS = ("parcel_rhoTrans", "parcel_UTrans", "parcel_UCoeff", "parcel_hsTrans", "parcel_hsCoeffByCp")
CASES = ("threeD_aachenBomb", "twoD_sydneySprayBurner")


def _text(case):
    with open(os.path.join(GOLDEN, "spray", case + ".sprayCloudProperties")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ the reader
@pytest.mark.parametrize("case", CASES)
def test_reader_on_the_reference_cases(case):
    from dfmi.spray import parse_spray_cloud_properties
    s = parse_spray_cloud_properties(_text(case))
    assert {k: s[k] for k in ("model", "rho", "U", "Yi", "h")} == {"model": 1, "rho": 0, "U": 0, "Yi": 0, "h": 0}
    assert s["relax"] == {"rho": 1.0, "U": 1.0, "Yi": 1.0, "h": 1.0}


def test_reader_schemes_switches_and_case_directory(tmp_path):
    from dfmi.spray import parse_spray_cloud_properties, read_case_spray
    txt = _text(CASES[0])
    semi = txt.replace("U               explicit 1;", "U               semiImplicit 0.7;") \
              .replace("h               explicit 1;", "h               semiImplicit 1;   // hsCoeff")
    s = parse_spray_cloud_properties(semi)
    assert (s["model"], s["rho"], s["U"], s["Yi"], s["h"]) == (1, 0, 1, 0, 1)
    assert s["relax"]["U"] == 0.7 and s["relax"]["h"] == 1.0
    for key in ("active", "coupled"):
        for word in ("false", "off", "no"):
            off = txt.replace(f"{key:16s}true;", f"{key:16s}{word};")
            assert off != txt
            assert parse_spray_cloud_properties(off)["model"] == 0
    # an uncoupled cloud's schemes are not looked at beyond their names
    bare = "solution { active false; }"
    assert parse_spray_cloud_properties(bare) == {"model": 0, "rho": 0, "U": 0, "Yi": 0, "h": 0,
                                                  "relax": {"rho": 1.0, "U": 1.0, "Yi": 1.0, "h": 1.0}}
    d = tmp_path / "case"
    (d / "constant").mkdir(parents=True)
    assert read_case_spray(str(d))["model"] == 0              # no cloud file: no cloud
    (d / "constant" / "sprayCloudProperties").write_text(semi)
    assert read_case_spray(str(d)) == s


def test_reader_refusals_by_name():
    from dfmi.spray import parse_spray_cloud_properties
    txt = _text(CASES[0])
    with pytest.raises(ValueError, match="implicit"):
        parse_spray_cloud_properties(txt.replace("Yi              explicit 1;", "Yi              implicit 1;"))
    with pytest.raises(ValueError, match="sourceTerms scheme semiimplicit of rho"):
        parse_spray_cloud_properties(txt.replace("rho             explicit 1;", "rho             semiimplicit 1;"))
    with pytest.raises(ValueError, match="no entry for h"):
        parse_spray_cloud_properties(txt.replace("h               explicit 1;", ""))
    with pytest.raises(ValueError, match="relaxation coefficient"):
        parse_spray_cloud_properties(txt.replace("U               explicit 1;", "U               explicit one;"))
    with pytest.raises(ValueError, match="not a switch"):
        parse_spray_cloud_properties(txt.replace("coupled         true;", "coupled         maybe;"))
    with pytest.raises(ValueError, match="no solution"):
        parse_spray_cloud_properties("constantProperties { T0 320; }")
    with pytest.raises(ValueError, match="no active"):
        parse_spray_cloud_properties("solution { coupled true; }")
    with pytest.raises(ValueError, match="no coupled"):          # a misspelt entry must not run the cloud uncoupled
        parse_spray_cloud_properties(txt.replace("coupled         true;", "coupeld         true;"))


class _Rec:
    def __init__(self):
        self.calls = []

    def set_option(self, k, v):
        self.calls.append((k, v))


def test_apply_spray_sets_the_model_last():
    from dfmi.spray import apply_spray
    r = _Rec()
    apply_spray(r, {"model": 1, "rho": 1, "U": 0, "Yi": 1, "h": 1, "relax": {}})
    assert r.calls == [("spray.rho", 1), ("spray.U", 0), ("spray.Yi", 1), ("spray.h", 1), ("spray.model", 1)]
    r = _Rec()
    apply_spray(r, {"model": 0, "rho": 1, "U": 1, "Yi": 1, "h": 1, "relax": {}})
    assert r.calls == [("spray.model", 0)]


# ------------------------------------------------------------------------------------------------ CPU-A, header, documents
def test_cpu_a_keeps_the_keys_and_fields_and_refuses_the_model():
    from dfmi.lib import DfmiError
    from test_cpu_a import _case
    out = _case(False)
    ctx, m = out[0], out[1]
    try:
        for key in KEYS:
            assert ctx.get_option(key) == 0.0, key
        for key in KEYS[1:]:
            ctx.set_option(key, 1)
            assert ctx.get_option(key) == 1.0
            with pytest.raises(DfmiError, match=key.replace(".", r"\.")):
                ctx.set_option(key, 2)
        ctx.set_option("spray.model", 0)
        with pytest.raises(DfmiError, match=r"spray\.model = 1"):
            ctx.set_option("spray.model", 1)
        with pytest.raises(DfmiError, match=r"spray\.nope"):
            ctx.set_option("spray.nope", 1)
        assert ctx.get_option("spray.model") == 0.0
        S = ctx.get_field("Y", (9, m.n_cells)).shape[0]
        for name, shape in zip(FIELDS, ((S, m.n_cells), (3, m.n_cells), (m.n_cells,), (m.n_cells,), (m.n_cells,))):
            v = np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
            ctx.set_field(name, v)
            assert np.array_equal(ctx.get_field(name, shape), v), name
    finally:
        ctx.close()


def test_header_option_table_and_documents_name_every_key_and_field():
    docs = {n: open(os.path.join(ROOT, *n.split("/"))).read()
            for n in ("include/dfmi.h", "DESIGN.md", "INTEGRATION.md", "deepflame-dev_amd/csrc/dfmi_ctx.h",
                      "baseline/cpu_a/cpu_a.cpp")}
    for name, txt in docs.items():
        for key in KEYS:
            assert key in txt, (name, key)
        for f in FIELDS:
            assert f in txt, (name, f)
    hdr = docs["include/dfmi.h"]
    for tok in ("KinematicCloudI.H", "ThermoCloudI.H", "ReactingCloudI.H", "semiImplicit", "hcSource", "1e-15"):
        assert tok in hdr, tok
    assert "spray.py" in open(os.path.join(ROOT, "README.md")).read()
    assert "hsCoeff()" in docs["INTEGRATION.md"] and "parcels.evolve()" in docs["INTEGRATION.md"]


# ------------------------------------------------------------------------------------------------ the term functions
def test_fp64_terms_within_committed_bounds():
    bounds = R.load_bounds()["terms"]
    measured = R.measure()
    assert set(measured) == set(bounds) == set(R.TERMS)
    for term, v in measured.items():
        print(f"{term:18s} {v:.3e}  (committed {bounds[term]:.3e})")
        assert np.isfinite(v) and v <= 4 * bounds[term], (term, v)
        assert bounds[term] < 1e-14, term          # a handful of roundings: nothing here is ill-conditioned


def _inputs(n=257, S=5, seed=3):
    rng = np.random.default_rng(seed)
    V, rho = rng.uniform(0.5e-9, 2e-9, n), rng.uniform(0.5, 2, n)
    return dict(n=n, S=S, rdt=1e6, V=V, rho=rho, diag=1e6 * rho * V, src=rng.standard_normal(n),
                Y=rng.random((S, n)), U=rng.standard_normal((3, n)), he=1e5 * rng.standard_normal(n),
                hc=1e6 * rng.standard_normal(S), UC=V * rng.random(n), hC=V * rng.standard_normal(n))


@pytest.mark.parametrize("semi", [0, 1])
def test_zero_transfers_add_exactly_nothing(semi):
    """rhoTrans = UTrans = hsTrans = 0: diag and source come back bit for bit -- also under the semi-implicit forms
    with non-zero coefficients, whose implicit and explicit halves must cancel in the solved equation and whose
    source echo is exactly coefficient x field"""
    q = _inputs()
    n, S = q["n"], q["S"]
    z = np.zeros
    d, s = R.rho_term(q["diag"], q["src"], z((S, n)), q["rdt"], q["V"], q["rho"], semi)
    assert np.array_equal(d, q["diag"]) and np.array_equal(s, q["src"])
    s3 = np.stack([q["src"]] * 3)
    d, a, b = R.u_term(q["diag"], s3, s3, z((3, n)), z(n), q["U"], q["rdt"], semi)
    assert np.array_equal(d, q["diag"]) and np.array_equal(a, s3) and np.array_equal(b, s3)
    dS, sS = np.tile(q["diag"], (S, 1)), np.tile(q["src"], (S, 1))
    d, s = R.y_term(dS, sS, z((S, n)), q["Y"], q["rdt"], q["V"], S - 1, semi)
    assert np.array_equal(d, dS) and np.array_equal(s, sS)
    d, s = R.e_term(q["diag"], q["src"], z((S, n)), q["hc"], z(n), z(n), q["he"], q["rdt"], q["V"], semi)
    assert np.array_equal(d, q["diag"]) and np.array_equal(s, q["src"])


def test_semi_implicit_h_with_a_negative_coefficient_is_the_explicit_form():
    q = _inputs()
    n, S = q["n"], q["S"]
    rng = np.random.default_rng(9)
    rT, hT = q["V"] * 1e-3 * rng.standard_normal((S, n)), q["V"] * 1e3 * rng.standard_normal(n)
    neg = -np.abs(q["hC"]) - 1e-30
    ex = R.e_term(q["diag"], q["src"], rT, q["hc"], hT, None, q["he"], q["rdt"], q["V"], 0)
    si = R.e_term(q["diag"], q["src"], rT, q["hc"], hT, neg, q["he"], q["rdt"], q["V"], 1)
    assert np.array_equal(ex[0], si[0]) and np.array_equal(ex[1], si[1])
    # and a positive one moves both the diagonal and the source
    si = R.e_term(q["diag"], q["src"], rT, q["hc"], hT, -neg, q["he"], q["rdt"], q["V"], 1)
    assert (si[0] > q["diag"]).all() and not np.array_equal(si[1], ex[1])


def test_inert_species_row_is_left_alone_and_a_sink_at_zero_Y_goes_to_the_diagonal():
    q = _inputs()
    n, S = q["n"], q["S"]
    inert = 2
    rT = -np.abs(q["V"] * 1e-3 * np.ones((S, n)))
    Y = q["Y"].copy(); Y[0, :5] = 0.0
    dS, sS = np.tile(q["diag"], (S, 1)), np.tile(q["src"], (S, 1))
    for semi in (0, 1):
        d, s = R.y_term(dS, sS, rT, Y, q["rdt"], q["V"], inert, semi)
        assert np.array_equal(d[inert], dS[inert]) and np.array_equal(s[inert], sS[inert])
    assert np.array_equal(s[0], sS[0])                      # sinks: nothing explicit
    want = dS[0, :5] + (q["V"][:5] * (-(rT[0, :5] * q["rdt"] / q["V"][:5]))) / 1e-15
    assert np.array_equal(d[0, :5], want) and np.isfinite(d).all()
