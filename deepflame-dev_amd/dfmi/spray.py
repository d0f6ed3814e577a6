"""Spray coupling: the host side of the Lagrangian source terms `parcels.Srho / SU / SYi / Sh` (rhoEqn.H:38, UEqn.H:9,
YEqn.H:110-111, EEqn.H:3-8; include/dfmi.h, spray block).

The cloud itself (tracking, injection, break-up, evaporation) stays with the caller; the device takes the cloud's per-cell
transfer fields (parcel_rhoTrans, parcel_UTrans, parcel_UCoeff, parcel_hsTrans, parcel_hsCoeffByCp) and folds them into the
rho, U, Yi and he equations. This module reads the `solution` block of a case's constant/sprayCloudProperties and sets the
spray.* options of a context.

Supported: sourceTerms.schemes rho | U | Yi | h with `explicit` or `semiImplicit`. Every other scheme name is refused by
name; entries for other fields (radiation) are ignored, as the gas-phase equations here carry no such term.
"""
from __future__ import annotations

import os
import re

from .schemes import dict_entries
from .turbulence import sub_dict

SCHEMES = {"explicit": 0, "semiImplicit": 1}
FIELDS = ("rho", "U", "Yi", "h")
_TRUE = ("true", "on", "yes", "y", "t")
_FALSE = ("false", "off", "no", "n", "f", "none")


def _strip(txt: str) -> str:
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//.*", "", txt)


def _sub(txt: str, name: str) -> str | None:
    try:
        return sub_dict(txt, name)
    except ValueError:
        raise ValueError(f"sprayCloudProperties: sub-dictionary {name} is not closed") from None


def _switch(key: str, text: str) -> bool:
    if text in _TRUE:
        return True
    if text in _FALSE:
        return False
    raise ValueError(f"sprayCloudProperties solution: {key} {text} is not a switch (true / false, on / off, yes / no)")


def parse_spray_cloud_properties(txt: str) -> dict:
    """{"model": 0 | 1, "rho", "U", "Yi", "h": 0 explicit | 1 semiImplicit, "relax": {field: coefficient}} from the text
    of constant/sprayCloudProperties. model = 1 when the cloud is active and coupled (`solution { active; coupled; }`); an
    inactive or uncoupled cloud adds nothing to the gas phase and its schemes are not required. The relaxation
    coefficient after a scheme name is returned (1 where absent) and not used: the cloud applies it to its own
    accumulators before they are handed over."""
    txt = _strip(txt)
    sol = _sub(txt, "solution")
    if sol is None:
        raise ValueError("sprayCloudProperties: no solution sub-dictionary")
    top = dict(dict_entries(sol))
    if "active" not in top:
        raise ValueError("sprayCloudProperties solution: no active entry")
    active = _switch("active", top["active"])
    if active and "coupled" not in top:      # cloudSolution reads it as mandatory once the cloud is active
        raise ValueError("sprayCloudProperties solution: no coupled entry")
    coupled = active and _switch("coupled", top["coupled"])
    out = {"model": 1 if (active and coupled) else 0, "relax": {}}
    for f in FIELDS:
        out[f] = 0
        out["relax"][f] = 1.0
    src = _sub(sol, "sourceTerms")
    sch = _sub(src, "schemes") if src is not None else None
    entries = dict(dict_entries(sch or ""))
    for f in FIELDS:
        if f not in entries:
            if out["model"]:
                raise ValueError(f"sprayCloudProperties solution: sourceTerms.schemes has no entry for {f}")
            continue
        tok = entries[f].split()
        if tok[0] not in SCHEMES:
            raise ValueError(f"sprayCloudProperties: sourceTerms scheme {tok[0]} of {f} is not supported "
                             f"({', '.join(SCHEMES)})")
        out[f] = SCHEMES[tok[0]]
        if len(tok) > 1:
            try:
                out["relax"][f] = float(tok[1])
            except ValueError:
                raise ValueError(f"sprayCloudProperties: sourceTerms scheme of {f}: relaxation coefficient {tok[1]!r} "
                                 "is not a number") from None
    return out


def read_case_spray(case_dir: str) -> dict:
    """parse_spray_cloud_properties of a case's constant/sprayCloudProperties; a case without the file has no cloud:
    model = 0 with explicit schemes"""
    path = os.path.join(case_dir, "constant", "sprayCloudProperties")
    if not os.path.exists(path):
        return {"model": 0, "rho": 0, "U": 0, "Yi": 0, "h": 0, "relax": {f: 1.0 for f in FIELDS}}
    with open(path) as f:
        return parse_spray_cloud_properties(f.read())


def apply_spray(ctx, settings: dict) -> None:
    """the options spray.* on a context (settings: parse_spray_cloud_properties' result): the four schemes, then
    spray.model last. No cloud: only spray.model = 0 is set."""
    if not settings["model"]:
        ctx.set_option("spray.model", 0)
        return
    for f in FIELDS:
        ctx.set_option("spray." + f, settings[f])
    ctx.set_option("spray.model", settings["model"])
