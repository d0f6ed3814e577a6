"""Real-fluid thermo: the Peng-Robinson species parameters of a Cantera YAML mechanism, for dfmi_thermo_set_eos
(include/dfmi.h).

A phase with ``thermo: Peng-Robinson`` carries, per species, ``equation-of-state: {model: Peng-Robinson, a, b,
acentric-factor}``. a and b are converted from the file's ``units`` block to Cantera's internal units, Pa m^6 / kmol^2
and m^3 / kmol (pressure stays Pa unless the block names one). What the device model does not hold is refused by name:
the Redlich-Kwong model, ``binary-a`` overrides (the mixture's cross terms are the geometric mean), a mix of models, and
the high-pressure ``Chung`` transport model.
"""
from __future__ import annotations

import os
import re

import numpy as np
import yaml

IDEAL, PENG_ROBINSON = 0, 1
_LENGTH = {"m": 1.0, "cm": 1e-2, "mm": 1e-3}
_QUANTITY = {"kmol": 1.0, "mol": 1e-3}
_PRESSURE = {"Pa": 1.0, "kPa": 1e3, "MPa": 1e6, "bar": 1e5, "atm": 101325.0}


class RealFluidError(ValueError):
    pass


def _unit(table, doc_units, key, default, what):
    u = (doc_units or {}).get(key, default)
    if u not in table:
        raise RealFluidError(f"{what}: unit '{u}' of '{key}' is not supported")
    return table[u]


def parse_eos(yaml_path: str, species=None) -> dict:
    """{"model": 0 | 1, "species", "a", "b", "acentric"} of the mechanism's first phase; species: the order wanted
    (default: the phase's). An ideal-gas phase gives model 0 and empty arrays."""
    with open(yaml_path) as f:
        doc = yaml.load(f, Loader=yaml.SafeLoader)
    phase = doc["phases"][0]
    thermo = str(phase.get("thermo", "ideal-gas"))
    names = list(species) if species is not None else list(phase["species"])
    if thermo == "ideal-gas":
        return {"model": IDEAL, "species": names, "a": np.zeros(0), "b": np.zeros(0), "acentric": np.zeros(0)}
    if thermo == "Redlich-Kwong":
        raise RealFluidError(f"{yaml_path}: phase thermo 'Redlich-Kwong' is not supported (Peng-Robinson only)")
    if thermo != "Peng-Robinson":
        raise RealFluidError(f"{yaml_path}: phase thermo '{thermo}' is not supported (ideal-gas or Peng-Robinson)")
    units = doc.get("units", {})
    L = _unit(_LENGTH, units, "length", "m", yaml_path)
    N = _unit(_QUANTITY, units, "quantity", "kmol", yaml_path)
    P = _unit(_PRESSURE, units, "pressure", "Pa", yaml_path)
    spec = {s["name"]: s for s in doc["species"]}
    a, b, w = [], [], []
    for n in names:
        if n not in spec:
            raise RealFluidError(f"{yaml_path}: species '{n}' is not in the mechanism")
        eos = spec[n].get("equation-of-state")
        if isinstance(eos, list):
            models = {str(e.get("model")) for e in eos}
            if len(models) != 1:
                raise RealFluidError(f"{yaml_path}: species '{n}' carries a mix of equation-of-state models {sorted(models)}")
            eos = eos[0]
        if eos is None:
            raise RealFluidError(f"{yaml_path}: species '{n}' has no equation-of-state block in a Peng-Robinson phase "
                                 f"(a mix of models is not supported)")
        model = str(eos.get("model"))
        if model == "Redlich-Kwong":
            raise RealFluidError(f"{yaml_path}: species '{n}': equation-of-state model 'Redlich-Kwong' is not supported")
        if model != "Peng-Robinson":
            raise RealFluidError(f"{yaml_path}: species '{n}': equation-of-state model '{model}' in a Peng-Robinson phase "
                                 f"(a mix of models is not supported)")
        if "binary-a" in eos:
            raise RealFluidError(f"{yaml_path}: species '{n}': 'binary-a' overrides are not supported "
                                 f"(the cross terms are the geometric mean)")
        for k in ("a", "b", "acentric-factor"):
            if k not in eos:
                raise RealFluidError(f"{yaml_path}: species '{n}': equation-of-state lacks '{k}'")
        a.append(float(eos["a"]) * P * L ** 6 / N ** 2)
        b.append(float(eos["b"]) * L ** 3 / N)
        w.append(float(eos["acentric-factor"]))
    return {"model": PENG_ROBINSON, "species": names, "a": np.array(a), "b": np.array(b), "acentric": np.array(w)}


def _dict_entry(text: str, key: str):
    m = re.search(r"^\s*" + re.escape(key) + r"\s+\"?([^\";\s]+)\"?\s*;", text, re.M)
    return m.group(1) if m else None


def read_case_eos(case_dir: str, species=None, transport: str | None = None) -> dict:
    """parse_eos of the mechanism constant/CanteraTorchProperties names. transportModel "Chung" (the high-pressure
    transport, which the device model does not hold) is refused by name unless the caller asks for transport="Mix"
    explicitly: the mixture-averaged fits are then used in its place."""
    path = os.path.join(case_dir, "constant", "CanteraTorchProperties")
    with open(path) as f:
        text = re.sub(r"//.*", "", f.read())
    mech = _dict_entry(text, "CanteraMechanismFile")
    if mech is None:
        raise RealFluidError(f"{path}: no CanteraMechanismFile entry")
    model = _dict_entry(text, "transportModel") or "Mix"
    if model == "Chung" and transport != "Mix":
        raise RealFluidError(f"{path}: transportModel \"Chung\" is not supported; pass transport=\"Mix\" to run the case "
                             f"with the mixture-averaged transport")
    if model not in ("Mix", "Chung"):
        raise RealFluidError(f"{path}: transportModel \"{model}\" is not supported")
    mech_path = mech if os.path.isabs(mech) else os.path.join(case_dir, mech)
    eos = parse_eos(mech_path, species)
    eos["transport"] = "Mix"
    return eos


def apply_eos(solver, eos: dict) -> None:
    """hand the parameters to a dfmi.lib.Context (after its thermo table is set); model 0 clears"""
    if eos["model"] == IDEAL:
        solver.thermo_set_eos(IDEAL)
    else:
        solver.thermo_set_eos(eos["model"], eos["a"], eos["b"], eos["acentric"])
