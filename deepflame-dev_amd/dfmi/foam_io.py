"""OpenFOAM ASCII field files (volScalarField / volVectorField, optionally gzip'd): the reader part
of the case I/O row. Parses `internalField uniform v` / `nonuniform
List<scalar|vector> N ( ... )` and the patch types of `boundaryField`; writes the same format.
Text parsing only (nothing is executed)."""
from __future__ import annotations

import gzip
import re

import numpy as np


def _open(path):
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path)


def read_field(path: str):
    """-> (values, patch_types): values [n] (scalar) or [n, 3] (vector); uniform fields return a
    0-d / [3] array."""
    txt = _open(path).read()
    cls = re.search(r"class\s+(\w+);", txt).group(1)
    vector = cls.endswith("VectorField")
    m = re.search(r"internalField\s+(uniform|nonuniform)", txt)
    if m is None:
        raise ValueError(f"{path}: no internalField")
    rest = txt[m.end():]
    if m.group(1) == "uniform":
        if vector:
            v = re.match(r"\s*\(([^)]*)\)", rest).group(1)
            vals = np.array([float(x) for x in v.split()])
        else:
            vals = np.array(float(re.match(r"\s*([^;\s]+)", rest).group(1)))
    else:
        hdr = re.match(r"\s*List<(\w+)>\s*(\d+)\s*\(", rest)
        n = int(hdr.group(2))
        body = rest[hdr.end():]
        end = body.find("\n)")
        body = body[:end]
        if vector:
            nums = np.array(body.replace("(", " ").replace(")", " ").split(), dtype=np.float64)
            vals = nums.reshape(n, 3)
        else:
            vals = np.array(body.split(), dtype=np.float64)
            assert vals.size == n, (path, vals.size, n)
    types = {}
    b = txt.find("boundaryField")
    if b >= 0:
        for pm in re.finditer(r"(\w+)\s*\{\s*type\s+(\w+);", txt[b:]):
            types[pm.group(1)] = pm.group(2)
    return vals, types


def read_boundary(path: str) -> dict:
    """boundaryField of a field file -> {patch: (type, value or None)}; `value uniform v` entries
    only (scalar or vector)."""
    txt = _open(path).read()
    b = txt.find("boundaryField")
    out = {}
    if b < 0:
        return out
    for pm in re.finditer(r"(\w+)\s*\{([^{}]*)\}", txt[b + len("boundaryField"):]):
        body = pm.group(2)
        t = re.search(r"type\s+(\w+);", body)
        if not t:
            continue
        v = re.search(r"value\s+uniform\s+(\([^)]*\)|[^;\s]+)\s*;", body)
        val = None
        if v:
            txtv = v.group(1).strip("()")
            val = np.array([float(x) for x in txtv.split()])
            val = val[0] if val.size == 1 else val
        out[pm.group(1)] = (t.group(1), val)
    return out


# Patch types of 0/k, 0/epsilon and 0/nut (RAS k-epsilon): kqRWallFunction is zeroGradient by definition;
# the wall functions proper and the turbulent inlets are not implemented and are refused by name.
_TURBULENCE_REFUSED = ("epsilonWallFunction", "turbulentMixingLengthDissipationRateInlet", "turbulentIntensityKineticEnergyInlet")


def turbulence_patch_types(field: str, types: dict) -> dict:
    """The strict mapper: {patch: type name} of a k, epsilon or nut file (read_field's second result) with
    kqRWallFunction mapped to zeroGradient; epsilonWallFunction, the nut*WallFunction family and the turbulent inlet
    conditions raise a ValueError that names the field, the patch and the type. It serves callers that set no patch
    parameters; turbulence_boundary (below) maps the wall functions and turbulent inlets the device implements."""
    out = {}
    for patch, t in types.items():
        if t == "kqRWallFunction":
            t = "zeroGradient"
        elif t in _TURBULENCE_REFUSED or (t.startswith("nut") and t.endswith("WallFunction")):
            raise ValueError(f"{field}: patch {patch}: boundary condition {t} is not supported "
                             "(wall functions and turbulent inlet conditions are not implemented)")
        out[patch] = t
    return out


def read_boundary_entries(path: str):
    """({patch: {keyword: text}}, internalField text or None) of a field file: every `keyword value;` entry of each
    patch dictionary as text, "type" included, in file order"""
    txt = re.sub(r"/\*.*?\*/", "", _open(path).read(), flags=re.S)
    txt = re.sub(r"//.*", "", txt)
    mi = re.search(r"internalField\s+([^;]+);", txt)
    b = txt.find("boundaryField")
    out = {}
    if b >= 0:
        for pm in re.finditer(r"(\w+)\s*\{([^{}]*)\}", txt[b + len("boundaryField"):]):
            out[pm.group(1)] = {k: v.strip() for k, v in re.findall(r"(\w+)\s+([^;]+);", pm.group(2))}
    return out, (mi.group(1).strip() if mi else None)


# The wall functions and turbulent inlets of the k-epsilon model on the device (include/dfmi.h, RAS block):
# type -> (the field it belongs to, the parameters read from its patch dictionary). The coefficients in 0/epsilon's
# epsilonWallFunction entries are not read: OpenFOAM-7 takes them from the patch's nutkWallFunction.
_TURBULENCE_MAPPED = {
    "epsilonWallFunction": ("epsilon", ()),
    "nutkWallFunction": ("nut", ("Cmu", "kappa", "E")),
    "turbulentIntensityKineticEnergyInlet": ("k", ("intensity",)),
    "turbulentMixingLengthDissipationRateInlet": ("epsilon", ("mixingLength",)),
}
_TURBULENCE_REQUIRED = ("intensity", "mixingLength")


def _uniform(where: str, text: str, internal: str | None) -> float:
    if text == "$internalField":
        if internal is None:
            raise ValueError(f"{where}: value $internalField, but the file's internalField was not given")
        text = internal
    mo = re.fullmatch(r"uniform\s+(\S+)", text)
    if not mo:
        raise ValueError(f"{where}: value {text!r} is not `uniform <number>`")
    return float(mo.group(1))


def turbulence_boundary(field: str, types: dict, entries: dict, internal_field: str | None = None) -> dict:
    """{"types": {patch: code}, "params": {patch: {name: number}}, "values": {patch: number or None}} of a k, epsilon
    or nut file. types: {patch: type name}; entries: {patch: {keyword: text}} (read_boundary_entries). The codes are
    dfmi.mesh's; kqRWallFunction is zeroGradient; the wall functions and turbulent inlets map to their own codes with the
    parameters their patch dictionaries carry (Cmu / kappa / E of 0/nut where given, intensity, mixingLength: required),
    ready for Context.set_patch_types and Context.set_patch_param. `value uniform v` and `value $internalField` (resolved
    with internal_field, the file's internalField text) are returned per patch. The rest of the nut*WallFunction family,
    wedge, a mapped type in the wrong file and every unknown type raise a ValueError naming field, patch and type."""
    from .mesh import BC_NAMES
    out = {"types": {}, "params": {}, "values": {}}
    for patch, t in types.items():
        where = f"{field}: patch {patch}"
        ent = entries.get(patch, {})
        if t == "kqRWallFunction":
            code = BC_NAMES["zeroGradient"]
        elif t in _TURBULENCE_MAPPED:
            owner, names = _TURBULENCE_MAPPED[t]
            if owner != field:
                raise ValueError(f"{where}: boundary condition {t} belongs to the field {owner}")
            code = BC_NAMES[t]
            par = {}
            for n in names:
                if n in ent:
                    try:
                        par[n] = float(ent[n])
                    except ValueError:
                        raise ValueError(f"{where}: {t}: {n} {ent[n]!r} is not a number") from None
                    if not (par[n] > 0 and np.isfinite(par[n])):
                        raise ValueError(f"{where}: {t}: {n} {ent[n]} must be positive and finite")
                elif n in _TURBULENCE_REQUIRED:
                    raise ValueError(f"{where}: {t} without a {n} entry")
            if par:
                out["params"][patch] = par
        elif t.startswith("nut") and t.endswith("WallFunction"):
            raise ValueError(f"{where}: boundary condition {t} is not supported (of the nut wall functions only "
                             "nutkWallFunction is implemented)")
        elif t == "wedge":
            raise ValueError(f"{where}: boundary condition wedge is not supported (a transform condition on U and on "
                             "every gradient)")
        elif t in BC_NAMES and t != "coupled":
            code = BC_NAMES[t]
        else:
            raise ValueError(f"{where}: boundary condition {t} is not supported")
        out["types"][patch] = code
        out["values"][patch] = _uniform(where, ent["value"], internal_field) if "value" in ent else None
    return out


def write_field(path: str, name: str, values: np.ndarray, patch_types: dict, dims="[0 0 0 0 0 0 0]"):
    vector = values.ndim == 2
    cls = "volVectorField" if vector else "volScalarField"
    lines = ["FoamFile", "{", "    version     2.0;", "    format      ascii;", f"    class       {cls};",
             f"    object      {name};", "}", "", f"dimensions      {dims};", "",
             f"internalField   nonuniform List<{'vector' if vector else 'scalar'}>", str(len(values)), "("]
    if vector:
        lines += [f"({float(v[0])!r} {float(v[1])!r} {float(v[2])!r})" for v in values]
    else:
        lines += [repr(float(v)) for v in values]
    lines += [")", ";", "", "boundaryField", "{"]
    for p, t in patch_types.items():
        lines += [f"    {p}", "    {", f"        type            {t};", "    }"]
    lines += ["}"]
    with (gzip.open(path, "wt") if path.endswith(".gz") else open(path, "w")) as f:
        f.write("\n".join(lines) + "\n")


def read_case_fields(directory: str, species: list):
    """T, p, U and Y of a case's 0/ directory in the species order given."""
    import os
    def rd(n):
        for ext in (".gz", ""):
            pth = os.path.join(directory, n + ext)
            if os.path.exists(pth):
                return read_field(pth)[0]
        raise FileNotFoundError(os.path.join(directory, n))
    T = rd("T")
    p = rd("p")
    U = rd("U")
    n = T.size
    Y = np.stack([np.broadcast_to(rd(s), (n,)) for s in species])
    return {"T": T, "p": np.broadcast_to(p, (n,)).copy(), "U": np.ascontiguousarray(np.broadcast_to(U, (n, 3)).T),
            "Y": np.ascontiguousarray(Y)}


def tile_fields(f: dict, n_src: int, reps=(2, 2, 2)) -> dict:
    """Tile fields of an n_src^3 block (i fastest) reps times per direction (BASELINE config 3:
    the 64^3 TGV fields tiled 2x2x2 into 128^3)."""
    def tile(a):
        lead = a.shape[:-1]
        b = a.reshape(lead + (n_src, n_src, n_src))            # [..., k, j, i]
        b = np.tile(b, (1,) * len(lead) + (reps[2], reps[1], reps[0]))
        return np.ascontiguousarray(b.reshape(lead + (-1,)))
    return {k: tile(v) for k, v in f.items()}
