"""LES eddy viscosity and RAS k-epsilon: the host side of `turbulence->` (dfLowMachFoam.C:207, :508; include/dfmi.h
dfmi_turbulence_correct).

The eddy viscosity itself is formed on the device. This module reads a case's constant/turbulenceProperties (and Sct
from the chemistry dictionary, createFields.H:133), computes the filter width `delta` on the host as OpenFOAM-7's
cubeRootVolDelta does, and sets the options and fields of a context.

Supported: simulationType laminar | LES; LESModel Smagorinsky | WALE (OpenFOAM-7) | Sigma |
dynamicSmagorinsky with `filter simple` (the reference's own, src/TurbulenceModels/turbulenceModels); delta
cubeRootVol. Everything else (dynamicKEqn, dynamicLagrangian and every other LESModel, the `laplace` and `anisotropic`
filters, the other delta types) is refused by name: DESIGN.md 10. parse_turbulence_properties reads the laminar and the
OpenFOAM-7 LES files and refuses Sigma, dynamicSmagorinsky and RAS; parse_les_properties reads those, `LESModel Sigma` with `SigmaCoeffs { Csg }`
and `LESModel dynamicSmagorinsky` with `dynamicSmagorinskyCoeffs { filter simple; }`, and returns the same dictionary plus
"Csg" and "filter"; parse_ras_properties reads simulationType RAS with RASModel kEpsilon
 and refuses RNGkEpsilon, every other RASModel and `turbulence off` by name; read_case_turbulence reads
simulationType and hands laminar and LES files to parse_les_properties, RAS files to parse_ras_properties.
"""
from __future__ import annotations

import re

import numpy as np

from .schemes import dict_entries

MODELS = {"Smagorinsky": 1, "WALE": 2}
# OpenFOAM-7 defaults (LESeddyViscosity: Ce 1.048; Smagorinsky / WALE: Ck 0.094; WALE: Cw 0.325), Prt = Sct = 1
DEFAULTS = {"Ck": 0.094, "Ce": 1.048, "Cw": 0.325, "Prt": 1.0, "Sct": 1.0, "deltaCoeff": 1.0}
_COEFFS = {"Smagorinsky": ("Ck", "Ce"), "WALE": ("Ck", "Ce", "Cw")}
# parse_les_properties: the reference's Sigma beside them (Csg 1.5, Sigma.C:118-126; it is an LESeddyViscosity, whose Ce
# it reads and never uses)
LES_MODELS = dict(MODELS, Sigma=4, dynamicSmagorinsky=5)
_LES_COEFFS = dict(_COEFFS, Sigma=("Csg", "Ce"), dynamicSmagorinsky=("Ce", "filter"))
FILTERS = ("simple",)          # `laplace` and `anisotropic` are refused by name
CSG_DEFAULT = 1.5


def _strip(txt: str) -> str:
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//.*", "", txt)


def sub_dict(txt: str, name: str) -> str | None:
    """the text between the braces of the sub-dictionary `name` of (comment-free) dictionary text at this level, or
    None; nested braces are matched"""
    depth = 0
    for mo in re.finditer(r"[{}]|(?<![\w.])" + re.escape(name) + r"\s*\{", txt):
        tok = mo.group(0)
        if tok == "{":
            depth += 1
        elif tok == "}":
            depth -= 1
        elif depth == 0:
            d, i = 1, mo.end()
            while i < len(txt) and d:
                d += {"{": 1, "}": -1}.get(txt[i], 0)
                i += 1
            if d:
                raise ValueError(f"turbulenceProperties: sub-dictionary {name} is not closed")
            return txt[mo.end():i - 1]
        else:
            depth += 1
    return None


def _number(where: str, key: str, text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"{where}: {key} {text!r} is not a number") from None
    if not (v > 0 and np.isfinite(v)):
        raise ValueError(f"{where}: {key} {text} must be positive and finite")
    return v


def parse_turbulence_properties(txt: str, chemistry_txt: str | None = None) -> dict:
    """{"model": 0 | 1 | 2, "LESModel": name | None, "Ck", "Ce", "Cw", "Prt", "Sct", "deltaCoeff"} from the text of
    constant/turbulenceProperties and, for Sct, of the chemistry dictionary (CanteraTorchProperties). The last entry of a
    keyword wins; coefficients not given take OpenFOAM-7's defaults."""
    return _parse_les(txt, chemistry_txt, MODELS, _COEFFS)


def parse_les_properties(txt: str, chemistry_txt: str | None = None) -> dict:
    """parse_turbulence_properties' dictionary plus "Csg" and "filter" (None unless the model has a test filter),
    with `LESModel Sigma` and `SigmaCoeffs { Csg }` accepted beside Smagorinsky and WALE ("model": 4), and
    `LESModel dynamicSmagorinsky` with `dynamicSmagorinskyCoeffs { filter simple; }` ("model": 5, "filter": "simple").
    Every other model, filter, delta type and unknown coefficient is refused by name."""
    out = _parse_les(txt, chemistry_txt, LES_MODELS, _LES_COEFFS)
    out.setdefault("Csg", CSG_DEFAULT)
    out.setdefault("filter", None)
    if out["model"] == 5 and out["filter"] is None:
        raise ValueError("turbulenceProperties: dynamicSmagorinskyCoeffs has no filter entry (simple)")
    return out


def _parse_les(txt: str, chemistry_txt: str | None, MODELS: dict, _COEFFS: dict) -> dict:
    txt = _strip(txt)
    top = dict(dict_entries(txt))
    sim = top.get("simulationType")
    if sim is None:
        raise ValueError("turbulenceProperties: no simulationType entry")
    out = dict(DEFAULTS, model=0, LESModel=None)
    if chemistry_txt is not None:
        chem = dict(dict_entries(_strip(chemistry_txt)))
        if "Sct" in chem:
            out["Sct"] = _number("chemistry dictionary", "Sct", chem["Sct"])
    if sim == "laminar":
        return out
    if sim != "LES":
        raise ValueError(f"turbulenceProperties: simulationType {sim} is not supported (laminar or LES)")
    les = sub_dict(txt, "LES")
    if les is None:
        raise ValueError("turbulenceProperties: simulationType LES without an LES sub-dictionary")
    ent = dict(dict_entries(les))
    name = ent.get("LESModel")
    if name is None:
        raise ValueError("turbulenceProperties: LES has no LESModel entry")
    if name not in MODELS:
        raise ValueError(f"turbulenceProperties: LESModel {name} is not supported ({', '.join(MODELS)})")
    if ent.get("turbulence", "on") not in ("on", "yes", "true"):
        raise ValueError(f"turbulenceProperties: LES turbulence {ent['turbulence']} is not supported (on)")
    delta = ent.get("delta")
    if delta is None:
        raise ValueError("turbulenceProperties: LES has no delta entry")
    if delta != "cubeRootVol":
        raise ValueError(f"turbulenceProperties: delta {delta} is not supported (cubeRootVol)")
    out["model"], out["LESModel"] = MODELS[name], name
    if "Prt" in ent:
        out["Prt"] = _number("turbulenceProperties LES", "Prt", ent["Prt"])
    coeffs = sub_dict(les, name + "Coeffs")
    for k, v in dict_entries(coeffs or ""):
        if k == "filter" and k in _COEFFS[name]:
            if v not in FILTERS:
                raise ValueError(f"turbulenceProperties: {name}Coeffs filter {v} is not supported ({', '.join(FILTERS)})")
            out["filter"] = v
        elif k in _COEFFS[name] or k == "Prt":
            out[k] = _number(f"turbulenceProperties {name}Coeffs", k, v)
        else:
            raise ValueError(f"turbulenceProperties: {name}Coeffs entry {k} is not supported ({', '.join(_COEFFS[name])})")
    crv = sub_dict(les, "cubeRootVolCoeffs")
    for k, v in dict_entries(crv or ""):
        if k == "deltaCoeff":
            out["deltaCoeff"] = _number("turbulenceProperties cubeRootVolCoeffs", k, v)
        else:
            raise ValueError(f"turbulenceProperties: cubeRootVolCoeffs entry {k} is not supported (deltaCoeff)")
    return out


def read_turbulence_properties(path: str, chemistry_path: str | None = None) -> dict:
    """parse_turbulence_properties of a case's constant/turbulenceProperties (and chemistry dictionary)"""
    with open(path) as f:
        txt = f.read()
    chem = None
    if chemistry_path is not None:
        with open(chemistry_path) as f:
            chem = f.read()
    return parse_turbulence_properties(txt, chem)


def empty_directions(m) -> list:
    """the axes (0, 1, 2) a mesh with `empty` patches does not solve. The host arrays carry no faces for an empty
    patch; OpenFOAM requires one cell across such a direction, so it is one in which every cell centre has the same
    coordinate."""
    if not any(p.kind == "empty" for p in m.patches):
        return []
    spread = np.ptp(np.asarray(m.cell_centres, dtype=np.float64), axis=0)
    axes = [k for k in range(3) if spread[k] <= 1e-9 * max(spread.max(), 1e-300)]
    if not axes:
        raise ValueError("delta cubeRootVol: the mesh has empty patches but more than one cell across every axis")
    return axes


def cube_root_vol_delta(m, delta_coeff: float = 1.0, thickness: float | None = None) -> np.ndarray:
    """OpenFOAM-7 cubeRootVolDelta::calcDelta per cell: three solved directions deltaCoeff cbrt(V); one `empty`
    direction deltaCoeff sqrt(V / thickness), thickness the mesh's extent in that direction (Mesh.extent, which
    hex_box and read_polymesh set, or the argument). Two empty directions are refused, as there ("Case must be either
    2D or 3D")."""
    V = np.asarray(m.volume, dtype=np.float64)
    axes = empty_directions(m)
    if not axes:
        return delta_coeff * np.cbrt(V)
    if len(axes) > 1:
        raise ValueError("delta cubeRootVol: a case with two empty directions is neither 2D nor 3D")
    if thickness is None:
        if not hasattr(m, "extent"):
            raise ValueError("delta cubeRootVol: a 2-D case needs the mesh's extent in the empty direction (thickness=)")
        thickness = float(m.extent[axes[0]])
    return delta_coeff * np.sqrt(V / thickness)


def apply(ctx, m, settings: dict, nut_patch_types=None) -> None:
    """the options les.*, the field delta and (if given) nut's patch types on a context that has been set up
    (case.setup_context). settings: parse_turbulence_properties' or parse_les_properties' result. Laminar: only
    les.model = 0 is set. Sigma (model 4): les.Csg too."""
    ctx.set_option("les.model", settings["model"])
    if not settings["model"]:
        return
    for k in ("Ck", "Ce", "Cw", "Prt", "Sct"):
        ctx.set_option("les." + k, settings[k])
    if settings["model"] == 4:
        ctx.set_option("les.Csg", settings.get("Csg", CSG_DEFAULT))
    if nut_patch_types is not None:
        ctx.set_patch_types("nut", nut_patch_types)
    ctx.set_field("delta", cube_root_vol_delta(m, settings["deltaCoeff"]))


# ------------------------------------------------------------------------------------------------ RAS k-epsilon
RAS_MODELS = {"kEpsilon": 1}
# OpenFOAM-7 kEpsilon defaults; kMin / epsilonMin are the model's bounds (SMALL^... of RASModel: 1e-15 here, dfmi.h)
RAS_DEFAULTS = {"Cmu": 0.09, "C1": 1.44, "C2": 1.92, "C3": 0.0, "sigmak": 1.0, "sigmaEps": 1.3, "kMin": 1e-15,
                "epsilonMin": 1e-15, "Prt": 1.0, "Sct": 1.0}
_RAS_COEFFS = ("Cmu", "C1", "C2", "C3", "sigmak", "sigmaEps")


def parse_ras_properties(txt: str, chemistry_txt: str | None = None) -> dict:
    """{"model": 0, "ras_model": 1, "RASModel": "kEpsilon", "Cmu", "C1", "C2", "C3", "sigmak", "sigmaEps", "kMin",
    "epsilonMin", "Prt", "Sct"} from `simulationType RAS; RAS { RASModel kEpsilon; turbulence on; Prt ...;
    kEpsilonCoeffs { ... } }` and, for Sct, the chemistry dictionary. "model" is the LES model (0)."""
    txt = _strip(txt)
    sim = dict(dict_entries(txt)).get("simulationType")
    if sim is None:
        raise ValueError("turbulenceProperties: no simulationType entry")
    if sim != "RAS":
        raise ValueError(f"turbulenceProperties: simulationType {sim} is not RAS")
    out = dict(RAS_DEFAULTS, model=0, ras_model=1, RASModel="kEpsilon")
    if chemistry_txt is not None:
        chem = dict(dict_entries(_strip(chemistry_txt)))
        if "Sct" in chem:
            out["Sct"] = _number("chemistry dictionary", "Sct", chem["Sct"])
    ras = sub_dict(txt, "RAS")
    if ras is None:
        raise ValueError("turbulenceProperties: simulationType RAS without a RAS sub-dictionary")
    ent = dict(dict_entries(ras))
    name = ent.get("RASModel")
    if name is None:
        raise ValueError("turbulenceProperties: RAS has no RASModel entry")
    if name not in RAS_MODELS:
        raise ValueError(f"turbulenceProperties: RASModel {name} is not supported ({', '.join(RAS_MODELS)})")
    if ent.get("turbulence", "on") not in ("on", "yes", "true"):
        raise ValueError(f"turbulenceProperties: RAS turbulence {ent['turbulence']} is not supported (on)")
    if "Prt" in ent:
        out["Prt"] = _number("turbulenceProperties RAS", "Prt", ent["Prt"])
    for k, v in dict_entries(sub_dict(ras, name + "Coeffs") or ""):
        if k == "C3":
            try:
                out[k] = float(v)
            except ValueError:
                raise ValueError(f"turbulenceProperties {name}Coeffs: C3 {v!r} is not a number") from None
            if not np.isfinite(out[k]):
                raise ValueError(f"turbulenceProperties {name}Coeffs: C3 {v} must be finite")
        elif k in _RAS_COEFFS or k == "Prt":
            out[k] = _number(f"turbulenceProperties {name}Coeffs", k, v)
        else:
            raise ValueError(f"turbulenceProperties: {name}Coeffs entry {k} is not supported ({', '.join(_RAS_COEFFS)})")
    return out


def read_ras_properties(path: str, chemistry_path: str | None = None) -> dict:
    """parse_ras_properties of a case's constant/turbulenceProperties (and chemistry dictionary)"""
    with open(path) as f:
        txt = f.read()
    chem = None
    if chemistry_path is not None:
        with open(chemistry_path) as f:
            chem = f.read()
    return parse_ras_properties(txt, chem)


def read_les_properties(path: str, chemistry_path: str | None = None) -> dict:
    """parse_les_properties of a case's constant/turbulenceProperties (and chemistry dictionary)"""
    with open(path) as f:
        txt = f.read()
    chem = None
    if chemistry_path is not None:
        with open(chemistry_path) as f:
            chem = f.read()
    return parse_les_properties(txt, chem)


def read_case_turbulence(path: str, chemistry_path: str | None = None) -> dict:
    """the settings of a case's constant/turbulenceProperties whatever its simulationType: laminar and LES through
    read_les_properties, RAS through read_ras_properties (its result has "RASModel")"""
    with open(path) as f:
        sim = dict(dict_entries(_strip(f.read()))).get("simulationType")
    if sim == "RAS":
        return read_ras_properties(path, chemistry_path)
    return read_les_properties(path, chemistry_path)


def apply_ras(ctx, m, settings: dict, patch_types: dict | None = None, k=None, epsilon=None, patch_params: dict | None = None) -> None:
    """the options ras.* on a context that has been set up (case.setup_context), the patch types of "k", "epsilon" and
    "nut" where patch_types has them, and, where given, the cell fields k and epsilon with boundary values as
    correctBoundaryConditions would leave them (zeroGradient / coupled; fixed-value slots are the caller's to set).
    settings: parse_ras_properties' result. patch_params: {field: {patch index: {name: value}}} of the wall functions and
    turbulent inlets (foam_io.turbulence_boundary's "params" by patch index), set after the types."""
    from . import case
    ctx.set_option("les.model", 0)
    for key in ("Cmu", "C1", "C2", "C3", "sigmak", "sigmaEps", "kMin", "epsilonMin", "Prt", "Sct"):
        ctx.set_option("ras." + key, settings[key])
    ctx.set_option("ras.model", settings.get("ras_model", 1))
    for f in ("k", "epsilon", "nut"):
        if patch_types is not None and patch_types.get(f) is not None:
            ctx.set_patch_types(f, patch_types[f])
    for f, per_patch in (patch_params or {}).items():
        for patch, par in per_patch.items():
            for name, v in par.items():
                ctx.set_patch_param(f, int(patch), name, v)
    for name, v in (("k", k), ("epsilon", epsilon)):
        if v is not None:
            v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (m.n_cells,)))
            ctx.set_field(name, v)
            ctx.set_field("boundary_" + name, case.boundary_values(m, v).reshape(-1))
