"""RAS k-epsilon, the parts that run without a GPU: the turbulenceProperties reader for simulationType RAS and its
refusals by name, the dispatching front end, the patch-type mapping of 0/k, 0/epsilon and 0/nut, the header's contract,
the documents, CPU-A's handling of the ras.* keys, and the NumPy restatement's own invariants (tests/ras_reference.py)."""
import os

import numpy as np
import pytest

import ras_reference as R
from conftest import GOLDEN, ROOT

FIXTURE = os.path.join(GOLDEN, "turbulenceProperties_ras")
RAS_KEYS = ("ras.model", "ras.Cmu", "ras.C1", "ras.C2", "ras.C3", "ras.sigmak", "ras.sigmaEps", "ras.kMin",
            "ras.epsilonMin", "ras.Prt", "ras.Sct")


def _ras(model="kEpsilon", extra="", coeffs=""):
    return ("simulationType RAS;\nRAS\n{\n    RASModel %s;\n    turbulence on;\n%s\n    %sCoeffs { %s }\n}\n"
            % (model, extra, model, coeffs))


def test_parser_reads_the_fixture():
    from dfmi import turbulence as T
    s = T.read_ras_properties(FIXTURE)
    assert s["RASModel"] == "kEpsilon" and s["ras_model"] == 1 and s["model"] == 0
    assert (s["Cmu"], s["C1"], s["C2"], s["C3"], s["sigmak"], s["sigmaEps"]) == (0.09, 1.52, 1.92, -0.33, 1.0, 1.2)
    assert s["Prt"] == 0.85 and s["Sct"] == 1.0 and s["kMin"] == 1e-15 and s["epsilonMin"] == 1e-15
    s = T.parse_ras_properties(open(FIXTURE).read(), "Sct 0.7;\n")
    assert s["Sct"] == 0.7


@pytest.mark.parametrize("txt,name", [
    (_ras("RNGkEpsilon"), "RNGkEpsilon"), (_ras("kOmegaSST"), "kOmegaSST"), (_ras("realizableKE"), "realizableKE"),
    (_ras(coeffs="Cmu 0.09; C4 1.0;"), "C4"), (_ras(coeffs="sigmaK 1.0;"), "sigmaK"),
    (_ras(extra="    turbulence off;"), "turbulence off"), (_ras(coeffs="Cmu -0.09;"), "Cmu"), (_ras(coeffs="C3 inf;"), "C3"),
    (_ras(coeffs="C1 abc;"), "C1"), ("simulationType RAS;\n", "RAS sub-dictionary"), ("simulationType LES;\n", "LES"),
    ("simulationType RAS;\nRAS { turbulence on; }\n", "RASModel")])
def test_parser_refusals_name_their_entry(txt, name):
    from dfmi import turbulence as T
    with pytest.raises(ValueError, match=name):
        T.parse_ras_properties(txt)


def test_front_end_dispatches(tmp_path):
    from dfmi import turbulence as T
    lam = tmp_path / "lam"
    lam.write_text("simulationType laminar;\n")
    assert T.read_case_turbulence(str(lam))["model"] == 0 and "RASModel" not in T.read_case_turbulence(str(lam))
    les = T.read_case_turbulence(os.path.join(GOLDEN, "turbulenceProperties_LES"))
    assert les["LESModel"] == "WALE" and les["model"] == 2
    ras = T.read_case_turbulence(FIXTURE)
    assert ras["RASModel"] == "kEpsilon" and ras["C1"] == 1.52
    with pytest.raises(ValueError, match="RAS"):            # the LES reader keeps refusing RAS
        T.parse_turbulence_properties(open(FIXTURE).read())


def test_patch_type_mapping_and_refusals():
    from dfmi.foam_io import turbulence_patch_types as tp
    assert tp("k", {"wall": "kqRWallFunction", "in": "fixedValue", "out": "inletOutlet"}) == \
        {"wall": "zeroGradient", "in": "fixedValue", "out": "inletOutlet"}
    for field, t in (("epsilon", "epsilonWallFunction"), ("nut", "nutkWallFunction"), ("nut", "nutUWallFunction"),
                     ("nut", "nutkRoughWallFunction"), ("epsilon", "turbulentMixingLengthDissipationRateInlet"),
                     ("k", "turbulentIntensityKineticEnergyInlet")):
        with pytest.raises(ValueError, match=t):
            tp(field, {"wall": t})


def test_scheme_keys_pass_through(tmp_path):
    from dfmi import schemes as S
    f = tmp_path / "fvSchemes"
    f.write_text("divSchemes\n{\n  default none;\n  div(phi,k) Gauss limitedLinear 1;\n  div(phi,epsilon) Gauss upwind;\n"
                 "  div(phi,K) Gauss linear;\n}\n")
    assert S.read_fv_schemes(str(f)) == {"div(phi,K)": "Gauss linear"}            # a laminar / LES case: not read
    got = S.read_fv_schemes(str(f), ras=True)
    assert got["div(phi,k)"] == "Gauss limitedLinear 1" and got["div(phi,epsilon)"] == "Gauss upwind"
    assert S.parse("div(phi,k)", "Gauss limitedLinear 1") == (S.LIMITED_LINEAR, 1.0)
    assert S.parse("div(phi,epsilon)", "linear") == (S.LINEAR, 1.0)
    with pytest.raises(ValueError):
        S.parse("div(phi,k)", "cubic")
    assert S.scheme_codes(got) == S.scheme_codes({"div(phi,K)": "Gauss linear"})   # the oracle's four are untouched


def test_header_and_documents_state_the_contract():
    hdr = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    for tok in RAS_KEYS[:1] + tuple("ras." + k for k in ("Cmu", "C1", "C2", "C3", "sigmak", "sigmaEps", "kMin", "epsilonMin",
                                                          "Prt", "Sct")):
        assert tok in hdr, tok
    for tok in ("dev(twoSymm(g)) && g", "interp_f(w, rho_P, rho_N)", "rho (nut/sigmak + mu/rho)", "rho (nut/sigmaEps + mu/rho)",
                "SuSp((2/3 C1 - C3) rho divU, eps)", "Sp(C2 rho eps/k, eps)", "SuSp(2/3 rho divU, k)", "Sp(rho eps/k, k)",
                "bound(eps, epsilonMin)", "bound(k, kMin)", "nut = Cmu k^2 / eps", "max(max(psi, avg(max(psi,m)) * pos0(-psi)), m)",
                "dfLowMachFoam.C:508", "div(phi,k)", "div(phi,epsilon)", "k_prebound"):
        assert tok in hdr, tok
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for key in RAS_KEYS + ("boundary_epsilon", "div(phi,epsilon)", "dfmi_turbulence_correct"):
        assert key in doc, key
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for tok in ("k_scalar_assemble", "k_ras_production", "epsilonWallFunction", "RNGkEpsilon"):
        assert tok in design, tok


def test_cpu_a_accepts_the_keys_and_refuses_the_model():
    from dfmi.lib import DfmiError
    from test_cpu_a import _case
    ctx = _case(False)[0]
    try:
        ctx.set_option("ras.model", 0)
        ctx.set_option("ras.C1", 1.52)
        ctx.set_option("ras.C3", -0.33)
        assert ctx.get_option("ras.C1") == 1.52 and ctx.get_option("ras.Cmu") == 0.09 and ctx.get_option("ras.model") == 0
        with pytest.raises(DfmiError, match="ras.model"):
            ctx.set_option("ras.model", 1)
        for key, bad in (("ras.Cmu", 0.0), ("ras.C3", float("nan")), ("ras.nope", 1.0), ("ras.kMin", -1.0)):
            with pytest.raises(DfmiError):
                ctx.set_option(key, bad)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.fixture(scope="module")
def box():
    m = R.get_mesh("periodic-even")
    return m, R.Topo(m)


def test_homogeneous_decay_of_the_restatement(box):
    """a fluid at rest, uniform k0, eps0, rho: one correct() of the restated equations is the closed form to 1e-14"""
    import oracle as O
    m, tp = box
    C_, B = m.n_cells, m.n_boundary_slots
    for q in ({}, {"C2": 1.7, "Cmu": 0.11, "C1": 1.3, "sigmak": 0.9, "sigmaEps": 1.1, "C3": -0.4}):
        q = dict(R.DEFAULTS, **q)
        k0, e0, rho, dt, mu = 0.37, 2.1e3, 1.1, 1e-5, 1.8e-5
        one, bone = np.ones(C_), np.ones(B)
        pt = m.patch_types(R.ZG)
        nut = R.nut_of(q["Cmu"], k0 * one, e0 * one)
        G, dv = np.zeros(C_), np.zeros(C_)
        k, eps = k0 * one, e0 * one
        for keq in (0, 1):
            Su, Sp = R.sources(keq, q, G, dv, rho * one, k, eps)
            sig = q["sigmak"] if keq else q["sigmaEps"]
            D = R.diffusivity(rho * one, nut, mu * one, sig)
            bD = R.diffusivity(rho * bone, R.nut_of(q["Cmu"], k0 * bone, e0 * bone), mu * bone, sig)
            psi = k if keq else eps
            o = R.scalar_assemble(tp, pt, psi, psi[0] * bone, rho * one, rho * one, np.zeros(m.n_faces), np.zeros(B), D, bD,
                                  Su, Sp, 1.0 / dt)
            import scipy.sparse as sp
            import scipy.sparse.linalg as spla
            r, c, v, b = O.ldu_system(m, pt, o["lower"], o["upper"], o["diag"], o["source"], o["internal_coeffs"],
                                      o["boundary_coeffs"])
            x = spla.spsolve(sp.coo_matrix((v, (r, c)), shape=(C_, C_)).tocsc(), b)
            if keq:
                k = x
            else:
                eps = x
        e1, k1, n1 = R.decay(k0, e0, dt, q)
        assert np.abs(eps / e1 - 1).max() <= 1e-14 and np.abs(k / k1 - 1).max() <= 1e-14
        assert np.abs(R.nut_of(q["Cmu"], k, eps) / n1 - 1).max() <= 1e-14


def test_production_of_chosen_tensors():
    from les_reference import LINEAR_G
    nut = 3e-4
    g = LINEAR_G["shear"].reshape(9, 1)
    gam = 1900.0
    assert R.production(g, [nut])[0] == nut * gam * gam                     # pure shear: nut gamma^2, exactly
    for cls in ("dilatation+", "dilatation-"):
        g = LINEAR_G[cls].reshape(9, 1)
        # dev() removes the trace: what is left is one rounding of (1/3) tr T against the diagonal, eps |g|^2 at most
        assert abs(R.production(g, [nut])[0]) <= 4 * np.finfo(float).eps * nut * (g * g).sum()
    assert R.production(np.zeros((9, 1)), [nut])[0] == 0.0
    assert R.production(LINEAR_G["general"].reshape(9, 1), [nut])[0] > 0


def test_bound_leaves_a_bounded_field_bitwise(box):
    m, tp = box
    rng = np.random.default_rng(3)
    pre = 10.0 ** rng.uniform(-12, 3, m.n_cells)
    from dfmi import case
    bpre = case.boundary_values(m, pre).reshape(-1)
    out, bout = R.bound(tp, m.patch_types(R.ZG), pre, bpre, 1e-15)
    assert np.array_equal(out, pre) and np.array_equal(bout, bpre)
    pre2 = pre.copy()
    pre2[[5, 6, 40]] = [-1.0, 0.0, -3.0]
    out2, _ = R.bound(tp, m.patch_types(R.ZG), pre2, case.boundary_values(m, pre2).reshape(-1), 1e-15)
    assert (out2 >= 1e-15).all() and out2[5] > 0 and np.array_equal(np.delete(out2, [5, 6, 40]), np.delete(pre, [5, 6, 40]))


def test_bounds_file_is_the_measurement():
    b = R.load_bounds()
    assert set(b["meshes"]) == set(R.MESHES)
    for v in b["meshes"].values():
        assert 0 < v["G"] < 1e-13 and 0 < v["divU"] < 1e-14
