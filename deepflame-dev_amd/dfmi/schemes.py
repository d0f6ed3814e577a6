"""fvSchemes selection for the terms the reference GPU path hard-wires.

The reference GPU path interpolates Yi and ha upwind and K and hDiffCorrFlux linearly whatever the case
asks for (src_gpu/dfYEqn.cu:543,587-593, dfEEqn.cu:166-174; limitedLinear is disabled,
dfMatrixOpBase.cu:2540-2600). The reference's own dfLowMachFoam cases ask for bounded schemes
(examples/dfLowMachFoam/notorch/threeD_reactingTGV/H2/cvodeIntegrator/system/fvSchemes:33-41,
test/dfLowMachFoam/twoD_reactingTGV/H2/cvodeSolver/system/fvSchemes:32-40), which the CPU
dfLowMachFoam runs (YEqn.H:6-14 multivariate convection over every Y_i and he, createFields.H:118-129;
EEqn.H fvc::div(phi, K) and fvc::div(hDiffCorrFlux)). dfmi_set_scheme (include/dfmi.h) selects them.
"""
from __future__ import annotations

TERMS = ("div(phi,Yi_h)", "div(phi,K)", "div(hDiffCorrFlux)", "div(phi,U)")
# the convection of the RAS model's transported scalars (k-epsilon; include/dfmi.h): upwind by default
RAS_TERMS = ("div(phi,k)", "div(phi,epsilon)")
UPWIND, LINEAR, LIMITED_LINEAR, LIMITED_LINEAR01, CUBIC, LIMITED_LINEAR_V = 0, 1, 2, 3, 4, 5
DEFAULT = {"div(phi,Yi_h)": "upwind", "div(phi,K)": "linear", "div(hDiffCorrFlux)": "linear", "div(phi,U)": "linear"}
# the reference cases' own divSchemes for these terms
REFERENCE_CASE = {"div(phi,Yi_h)": "limitedLinear01 1", "div(phi,K)": "limitedLinear 1",
                  "div(hDiffCorrFlux)": "cubic"}
_ALLOWED = {"div(phi,Yi_h)": (UPWIND, LIMITED_LINEAR, LIMITED_LINEAR01),
            "div(phi,K)": (UPWIND, LINEAR, LIMITED_LINEAR, LIMITED_LINEAR01),
            "div(hDiffCorrFlux)": (LINEAR, CUBIC), "div(phi,U)": (LINEAR, LIMITED_LINEAR_V),
            "div(phi,k)": (UPWIND, LINEAR, LIMITED_LINEAR), "div(phi,epsilon)": (UPWIND, LINEAR, LIMITED_LINEAR)}


def parse(term: str, scheme: str) -> tuple[int, float]:
    """'limitedLinear01 1' -> (LIMITED_LINEAR01, 1.0); a leading 'Gauss' is accepted"""
    if term not in TERMS + RAS_TERMS:
        raise ValueError(f"unknown scheme term {term!r}; expected one of {TERMS + RAS_TERMS}")
    tok = scheme.split()
    if tok and tok[0] == "Gauss":
        tok = tok[1:]
    names = {"upwind": UPWIND, "linear": LINEAR, "limitedLinear": LIMITED_LINEAR,
             "limitedLinear01": LIMITED_LINEAR01, "cubic": CUBIC, "limitedLinearV": LIMITED_LINEAR_V}
    if not tok or tok[0] not in names:
        raise ValueError(f"{term}: unsupported scheme {scheme!r}")
    code = names[tok[0]]
    k = 1.0
    if code in (LIMITED_LINEAR, LIMITED_LINEAR01, LIMITED_LINEAR_V):
        if len(tok) != 2:
            raise ValueError(f"{term}: {tok[0]} needs its coefficient k")
        k = float(tok[1])
        if not 0.0 <= k <= 1.0:
            raise ValueError(f"{term}: limitedLinear coefficient must be in [0, 1]")
    elif len(tok) != 1:
        raise ValueError(f"{term}: unexpected arguments in {scheme!r}")
    if code not in _ALLOWED[term]:
        raise ValueError(f"{term}: scheme {tok[0]} not supported for this term")
    return code, k


def scheme_codes(schemes: dict) -> tuple[list, list]:
    """{term: scheme} -> (codes[4], k[3]) in TERMS order (k of Yi_h, K, U), defaults filled in; the RAS_TERMS are
    checked and left out (they are not among the four)"""
    full = dict(DEFAULT)
    for t, v in schemes.items():
        parse(t, v)
        if t in TERMS:
            full[t] = v
    codes, ks = [], [1.0, 1.0, 1.0]
    kslot = {0: 0, 1: 1, 3: 2}
    for i, t in enumerate(TERMS):
        c, k = parse(t, full[t])
        codes.append(c)
        if i in kslot:
            ks[kslot[i]] = k
    return codes, ks


def strip_comments(txt: str) -> str:
    """OpenFOAM dictionary text without its /* */ and // comments"""
    import re
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//.*", "", txt)


def dict_entries(txt: str) -> list:
    """the `keyword value...;` entries of a piece of OpenFOAM dictionary text in file order, as
    (keyword, value) pairs; // and /* */ comments are dropped, and so is every { } block with its name
    (FoamFile, sub-dictionaries): the entries of one level only"""
    import re
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//.*", "", txt)
    while True:
        flat = re.sub(r"[^\s;{}]+\s*\{[^{}]*\}", "", txt)
        if flat == txt:
            break
        txt = flat
    out = []
    for line in txt.split(";"):
        tok = line.split()
        if len(tok) >= 2:
            out.append((tok[0], " ".join(tok[1:])))
    return out


LAPLACIAN = "laplacian"
LAPLACIAN_SCHEMES = ("orthogonal", "uncorrected", "corrected")


def parse_laplacian(scheme: str) -> str:
    """'Gauss linear corrected' -> 'corrected': the snGrad part of a laplacianSchemes entry. The library runs one
    laplacian scheme for the U, Yi, he and p equations, Gauss with linear interpolation of the diffusivity;
    'limited <psi>' and every other snGrad scheme are refused by name."""
    tok = scheme.split()
    if tok and tok[0] == "Gauss":
        tok = tok[1:]
    if tok and tok[0] == "linear":
        tok = tok[1:]
    if not tok:
        raise ValueError("laplacian: empty scheme")
    if tok[0] == "limited":
        raise ValueError(f"laplacian: the snGrad scheme 'limited' is not supported ({scheme!r})")
    if tok[0] not in LAPLACIAN_SCHEMES:
        raise ValueError(f"laplacian: unsupported scheme {scheme!r}; expected one of {LAPLACIAN_SCHEMES}")
    if len(tok) != 1:
        raise ValueError(f"laplacian: unexpected arguments in {scheme!r}")
    return tok[0]


def _block(txt: str, name: str):
    """the text between the braces of the first-level dictionary `name` (nested braces kept), or None"""
    import re
    mo = re.search(r"(?<![\w()])" + re.escape(name) + r"\s*\{", txt)
    if not mo:
        return None
    depth, i = 1, mo.end()
    while i < len(txt) and depth:
        depth += {"{": 1, "}": -1}.get(txt[i], 0)
        i += 1
    return txt[mo.end():i - 1]


def read_fv_schemes(path: str, ras: bool = False) -> dict:
    """the entries of a case's system/fvSchemes that dfmi_set_scheme selects ({term: scheme}): the divSchemes entries
    for TERMS (with ras=True, a RAS case, also those for RAS_TERMS: laminar and LES cases carry div(phi,k) and
    div(phi,epsilon) entries that nothing reads), and 'laplacian' from laplacianSchemes { default ...; } when it is not the default 'orthogonal'. A per-term laplacian entry that differs from
    the default (or per-term entries that differ from each other, without a default) is an error: the library runs
    one laplacian scheme."""
    import re
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//.*", "", txt)
    out = {}
    div = _block(txt, "divSchemes")
    if div is not None:
        out.update({k: v for k, v in dict_entries(div) if k in (TERMS + RAS_TERMS if ras else TERMS)})
    lap = _block(txt, "laplacianSchemes")
    if lap is not None:
        entries = dict_entries(lap)
        default = [v for k, v in entries if k == "default"]
        kinds = {k: parse_laplacian(v) for k, v in entries if k != "default"}
        if default and default[-1].split()[0] != "none":
            want = parse_laplacian(default[-1])
        elif kinds:
            want = next(iter(kinds.values()))
        else:
            want = None
        for k, v in kinds.items():
            if v != want:
                raise ValueError(f"laplacianSchemes: {k} selects {v!r} but the other laplacians {want!r}; "
                                 "one scheme serves every laplacian")
        if want is not None and want != "orthogonal":   # the default is left out, as an absent block is
            out[LAPLACIAN] = want
    return out


def read_fv_solution(path: str) -> dict:
    """the PIMPLE block of a case's system/fvSolution: {'nCorrectors': int (dfmi_time_step's n_corr),
    'nNonOrthogonalCorrectors': int (option p.n_nonorth)}, OpenFOAM's defaults (1, 0) where an entry is absent.
    nOuterCorrectors other than 1 is refused: dfmi_time_step is one outer iteration."""
    import re
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//.*", "", txt)
    blk = _block(txt, "PIMPLE")
    if blk is None:
        raise ValueError(f"{path}: no PIMPLE dictionary")
    e = dict(dict_entries(blk))

    def count(key, default, least):
        try:
            v = int(e.get(key, default))
        except ValueError:
            raise ValueError(f"PIMPLE: {key} must be an integer, got {e[key]!r}") from None
        if v < least:
            raise ValueError(f"PIMPLE: {key} must be >= {least}, got {v}")
        return v
    if count("nOuterCorrectors", 1, 1) != 1:
        raise ValueError("PIMPLE: nOuterCorrectors other than 1 is not supported (one outer iteration per time step)")
    return {"nCorrectors": count("nCorrectors", 1, 0), "nNonOrthogonalCorrectors": count("nNonOrthogonalCorrectors", 0, 0)}
