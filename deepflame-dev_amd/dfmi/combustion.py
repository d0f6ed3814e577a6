"""Turbulence-chemistry interaction: the host side of `combustion->correct()` (YEqn.H:76; include/dfmi.h
dfmi_combustion_correct).

kappa, the time scales and the scaled source are formed on the device. This module reads a case's
constant/combustionProperties and sets the tci.* options of a context.

Supported: combustionModel laminar | PaSR | EDC; PaSR mixingScale globalScale | kolmogorovScale | geometriMeanScale,
chemistryScale globalConvertion | formationRate | reactionRate; EDC version v1981 | v1996 | v2005 | v2016. dynamicScale,
the FGM models (flareFGM, DeePFGM) and every other name are refused by name: DESIGN.md 10 and 15.
"""
from __future__ import annotations

import re

from .schemes import dict_entries
from .turbulence import _number, _strip, sub_dict

MODELS = {"laminar": 0, "PaSR": 1, "EDC": 2}
MIXING = {"globalScale": 1, "kolmogorovScale": 2, "geometriMeanScale": 3}
CHEMISTRY = {"globalConvertion": 1, "formationRate": 2, "reactionRate": 3}
VERSIONS = {"v1981": 1981, "v1996": 1996, "v2005": 2005, "v2016": 2016}
# PaSR.C / EDC.H defaults (include/dfmi.h)
DEFAULTS = {"model": 0, "combustionModel": "laminar", "mixing": 1, "chemistry": 1, "Cmix": 0.1, "fuel": None,
            "oxidizer": None, "version": 2005, "C1": 0.05774, "C2": 0.5, "Cgamma": 2.1377, "Ctau": 0.4083, "exp1": 0,
            "exp2": 0}
_EDC_COEFFS = ("C1", "C2", "Cgamma", "Ctau")


def _sub(txt: str, name: str) -> str | None:
    try:
        return sub_dict(txt, name)
    except ValueError:
        raise ValueError(f"combustionProperties: sub-dictionary {name} is not closed") from None


def parse_combustion_properties(txt: str) -> dict:
    """{"model": 0 | 1 | 2, "combustionModel": name, "mixing", "chemistry", "Cmix", "fuel", "oxidizer" (species names
    or None), "version", "C1", "C2", "Cgamma", "Ctau", "exp1", "exp2"} from the text of constant/combustionProperties.
    A `//` comment may follow the model name on its line (`combustionModel PaSR;//EDC; PaSR`)."""
    txt = _strip(txt)
    top = dict(dict_entries(txt))
    name = top.get("combustionModel")
    if name is None:
        raise ValueError("combustionProperties: no combustionModel entry")
    if name not in MODELS:
        raise ValueError(f"combustionProperties: combustionModel {name} is not supported ({', '.join(MODELS)})")
    out = dict(DEFAULTS, model=MODELS[name], combustionModel=name)
    edc = _sub(txt, "EDCCoeffs")
    for k, v in dict_entries(edc or ""):
        if k == "version":
            if v not in VERSIONS:
                raise ValueError(f"combustionProperties EDCCoeffs: version {v} is not supported ({', '.join(VERSIONS)})")
            out["version"] = VERSIONS[v]
        elif k in _EDC_COEFFS:
            out[k] = _number("combustionProperties EDCCoeffs", k, v)
        elif k in ("exp1", "exp2"):
            e = _number("combustionProperties EDCCoeffs", k, v)
            if e not in (1.0, 2.0, 3.0, 4.0):
                raise ValueError(f"combustionProperties EDCCoeffs: {k} {v} is not supported (an integer 1..4)")
            out[k] = int(e)
        else:
            raise ValueError(f"combustionProperties: EDCCoeffs entry {k} is not supported "
                             f"(version, {', '.join(_EDC_COEFFS)}, exp1, exp2)")
    pasr = _sub(txt, "PaSRCoeffs")
    if pasr is not None:
        mix = _sub(pasr, "mixingScale")
        if mix is not None:
            t = dict(dict_entries(mix)).get("type")
            if t is None:
                raise ValueError("combustionProperties: PaSRCoeffs mixingScale has no type entry")
            if t not in MIXING:
                raise ValueError(f"combustionProperties: mixingScale type {t} is not supported ({', '.join(MIXING)})")
            out["mixing"] = MIXING[t]
            for k, v in dict_entries(_sub(mix, t + "Coeffs") or ""):
                if k != "Cmix":
                    raise ValueError(f"combustionProperties: {t}Coeffs entry {k} is not supported (Cmix)")
                out["Cmix"] = _number(f"combustionProperties {t}Coeffs", k, v)
        che = _sub(pasr, "chemistryScale")
        if che is not None:
            t = dict(dict_entries(che)).get("type")
            if t is None:
                raise ValueError("combustionProperties: PaSRCoeffs chemistryScale has no type entry")
            if t not in CHEMISTRY:
                raise ValueError(f"combustionProperties: chemistryScale type {t} is not supported ({', '.join(CHEMISTRY)})")
            out["chemistry"] = CHEMISTRY[t]
            for k, v in dict_entries(_sub(che, "globalConvertionCoeffs") or ""):
                if k not in ("fuel", "oxidizer"):
                    raise ValueError(f"combustionProperties: globalConvertionCoeffs entry {k} is not supported (fuel, oxidizer)")
                if not re.fullmatch(r"[\w()+\-*]+", v):
                    raise ValueError(f"combustionProperties globalConvertionCoeffs: {k} {v!r} is not a species name")
                out[k] = v
    elif name == "PaSR":
        raise ValueError("combustionProperties: combustionModel PaSR without a PaSRCoeffs sub-dictionary")
    if name == "PaSR" and out["chemistry"] == 1 and out["fuel"] is None:
        raise ValueError("combustionProperties: chemistryScale globalConvertion needs globalConvertionCoeffs { fuel ...; }")
    return out


def read_combustion_properties(path: str) -> dict:
    """parse_combustion_properties of a case's constant/combustionProperties"""
    with open(path) as f:
        return parse_combustion_properties(f.read())


def apply_combustion(ctx, settings: dict, species_names: list) -> None:
    """the options tci.* on a context (settings: parse_combustion_properties' result; species_names: the mechanism's
    species in field order). fuel and oxidizer are the dictionary's; CO2 and H2 are looked up by name as PaSR.C does and
    left out (-1) where the mechanism has none. laminar: only tci.model = 0 is set."""
    if not settings["model"]:
        ctx.set_option("tci.model", 0)
        return
    names = list(species_names)

    def index(key):
        n = settings.get(key)
        if n is None:
            return -1
        if n not in names:
            raise ValueError(f"combustionProperties: {key} {n} is not a species of the mechanism")
        return names.index(n)

    for k in ("Cmix", "C1", "C2", "Cgamma", "Ctau", "exp1", "exp2", "version", "mixing", "chemistry"):
        ctx.set_option("tci." + k, settings[k])
    ctx.set_option("tci.fuel", index("fuel"))
    ctx.set_option("tci.oxidizer", index("oxidizer"))
    ctx.set_option("tci.CO2", names.index("CO2") if "CO2" in names else -1)
    ctx.set_option("tci.H2", names.index("H2") if "H2" in names else -1)
    ctx.set_option("tci.model", settings["model"])
