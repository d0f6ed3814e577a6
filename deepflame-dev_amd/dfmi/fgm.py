"""flareFGM: the host side of the tabulated flamelet combustion model (include/dfmi.h, flareFGM block).

The transport equations and the table retrieval run on the device (dfmi_fgm_correct / dfmi_fgm_retrieve). This module
reads and writes the `flare.tbl` text format as flameletTableSolver/tableSolver.C:42-337 reads it, reads the
flareFGMCoeffs of a case's constant/combustionProperties, and sets the table and the fgm.* options of a context.

File layout (one record per line; of a line only the leading tokens are read, as `iss >>` does):
    NH NZ NC NGZ NGC NZC NS NYomega NY NZL
    the NYomega source-term species names          (a line of its own, empty when NYomega = 0)
    the NY species names                           (likewise)
    NH + NZ + NC + NGZ + NGC + NZC lines: the axes h, z, c, gz, gc, gzc, one value per line
    Hfu Hox
    NH NZL lines:  z sl th tau kctau               (the laminar block, h outermost)
    NH NZ NC NGZ NGC NZC lines of NS + NY values   (h outermost, gzc fastest)
    NH NZ NGZ lines:  d2Yeq d1Yeq                  (only when NS == 8 + NYomega: scaled progress variable)

Not supported, refused by name: combustionModel DeePFGM; flareFGMCoeffs buffer / bufferTime > 0, relaxation, DpDt,
ignition; a p_operateDim that differs from incompPref.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass

import numpy as np

from .schemes import dict_entries, strip_comments
from .turbulence import sub_dict

AXES = ("h", "z", "c", "gz", "gc", "gzc")
FIXED_TABLES = ("omgc_Tb3", "cOc_Tb3", "ZOc_Tb3", "cp_Tb3", "mwt_Tb3", "hiyi_Tb3", "Tf_Tb3", "nu_Tb3")
LAMINAR = ("z", "sl", "th", "tau", "kctau")
# baseFGM.C:42-48, 336-337, 354-355
DEFAULTS = {"model": 1, "combustionModel": "flareFGM", "scaledPV": False, "combustion": False, "solveEnthalpy": False,
            "flameletT": False, "Sct": 0.7, "Sc": 1.0, "incompPref": -10.0, "TMin": 200.0, "TMax": 5000.0,
            "tablePath": None, "omega_YiNames": []}
_REFUSED_SWITCHES = ("buffer", "relaxation", "DpDt", "ignition")
_IGNORED = ("nOmega_Yis", "ignBeginTime", "ignDurationTime", "x0", "y0", "z0", "R0", "speciesName")
SCHEME_TERMS = tuple(f"div(phi,{n})" for n in ("Z", "Zvar", "c", "cvar", "Zcvar", "Ha"))


@dataclass
class Table:
    """a flamelet table in memory: axes [h, z, c, gz, gc, gzc]; laminar [5, NH NZL] = z, sl, th, tau, kctau; values
    [NS + NY, NH NZ NC NGZ NGC NZC] in the reference's index order; d2Yeq / d1Yeq [NH NZ NGZ] (scaled only)"""
    axes: list
    NS: int
    NZL: int
    omega_names: list
    species_names: list
    Hfu: float
    Hox: float
    laminar: np.ndarray
    values: np.ndarray
    d2Yeq: np.ndarray | None = None
    d1Yeq: np.ndarray | None = None

    @property
    def shape(self):
        return tuple(int(np.size(a)) for a in self.axes)

    @property
    def NYomega(self):
        return len(self.omega_names)

    @property
    def NY(self):
        return len(self.species_names)

    @property
    def scaled(self):
        return self.NS == 8 + self.NYomega

    @property
    def size(self):
        return int(np.prod(self.shape))

    def dims(self):
        return list(self.shape) + [self.NS, self.NYomega, self.NY, self.NZL]

    def table_names(self):
        """the NS + NY column names as tableSolver.C:65-108 builds them"""
        names = list(FIXED_TABLES) + [f"omega_{n}" for n in self.omega_names]
        if not self.scaled:
            names.append("Ycmax_Tb3")
        return names + list(self.species_names)


def _fmt(v) -> str:
    return repr(float(v))


def write_table(path: str, t: Table) -> None:
    """the inverse of read_table: every value with the shortest text that reads back to the same bits"""
    NH, NZ, NC, NGZ, NGC, NZC = t.shape
    nv = t.NS + t.NY
    vals = np.asarray(t.values, np.float64).reshape(nv, t.size)
    lam = np.asarray(t.laminar, np.float64).reshape(5, NH * t.NZL)
    out = [" ".join(str(int(v)) for v in t.dims()), " ".join(t.omega_names), " ".join(t.species_names)]
    for a in t.axes:
        out.extend(_fmt(v) for v in np.asarray(a, np.float64).reshape(-1))
    out.append(f"{_fmt(t.Hfu)} {_fmt(t.Hox)}")
    for i in range(NH * t.NZL):
        out.append(" ".join(_fmt(lam[k, i]) for k in range(5)))
    for i in range(t.size):
        out.append(" ".join(_fmt(v) for v in vals[:, i]))
    if t.scaled:
        d2, d1 = np.asarray(t.d2Yeq, np.float64).reshape(-1), np.asarray(t.d1Yeq, np.float64).reshape(-1)
        for i in range(NH * NZ * NGZ):
            out.append(f"{_fmt(d2[i])} {_fmt(d1[i])}")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def read_table(path: str) -> Table:
    """a flare.tbl file as tableSolver.C:42-337 reads it. Refused by name: a missing file; a header that is not ten
    integers; a dimension < 1 or NZL < 2; an NS that is neither 8 + NYomega nor 9 + NYomega (the reference only warns);
    a name line with too few names; a file that ends early; a record with too few values or one that is not a number."""
    if not os.path.isfile(path):
        raise ValueError(f"flare table {path}: no such file")
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    pos = 0

    def record(what, n, as_float=True):
        nonlocal pos
        if pos >= len(lines):
            raise ValueError(f"flare table {path}: the file ends before {what} (line {pos + 1})")
        tok = lines[pos].split()
        pos += 1
        if len(tok) < n:
            raise ValueError(f"flare table {path}: line {pos}: {what} needs {n} values, found {len(tok)}")
        if not as_float:
            return tok[:n]
        try:
            return [float(x) for x in tok[:n]]
        except ValueError:
            raise ValueError(f"flare table {path}: line {pos}: {what} holds a value that is not a number") from None

    head = record("the header NH NZ NC NGZ NGC NZC NS NYomega NY NZL", 10, as_float=False)
    try:
        NH, NZ, NC, NGZ, NGC, NZC, NS, NYo, NY, NZL = (int(x) for x in head)
    except ValueError:
        raise ValueError(f"flare table {path}: the header is not ten integers: {' '.join(head)}") from None
    for n, v in zip(("NH", "NZ", "NC", "NGZ", "NGC", "NZC"), (NH, NZ, NC, NGZ, NGC, NZC)):
        if v < 1:
            raise ValueError(f"flare table {path}: dimension {n} = {v} must be at least 1")
    if NYo < 0 or NY < 0:
        raise ValueError(f"flare table {path}: NYomega and NY must not be negative")
    if NZL < 2:
        raise ValueError(f"flare table {path}: NZL = {NZL} must be at least 2")
    if NS not in (8 + NYo, 9 + NYo):
        raise ValueError(f"flare table {path}: NS = {NS} must be 8 + NYomega (scaled progress variable) or 9 + NYomega "
                         f"(unscaled); NYomega = {NYo}")
    omega_names = record("the source-term species names", NYo, as_float=False)
    species_names = record("the species names", NY, as_float=False)
    axes = []
    for name, n in zip(AXES, (NH, NZ, NC, NGZ, NGC, NZC)):
        axes.append(np.array([record(f"axis {name}", 1)[0] for _ in range(n)]))
    Hfu, Hox = record("Hfu Hox", 2)
    lam = np.array([record("the laminar block (z sl th tau kctau)", 5) for _ in range(NH * NZL)]).T.copy()
    N = NH * NZ * NC * NGZ * NGC * NZC
    vals = np.array([record(f"the value tables ({NS + NY} columns)", NS + NY) for _ in range(N)]).T.copy()
    d2 = d1 = None
    if NS == 8 + NYo:
        d = np.array([record("the non-premixed block (d2Yeq d1Yeq)", 2) for _ in range(NH * NZ * NGZ)])
        d2, d1 = d[:, 0].copy(), d[:, 1].copy()
    return Table(axes, NS, NZL, omega_names, species_names, Hfu, Hox, lam.reshape(5, NH * NZL), vals.reshape(NS + NY, N), d2, d1)


def _switch(where, key, text) -> bool:
    if text in ("true", "on", "yes", "1"):
        return True
    if text in ("false", "off", "no", "0"):
        return False
    raise ValueError(f"{where}: {key} {text!r} is not a switch (true / false)")


def _real(where, key, text, positive=True) -> float:
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"{where}: {key} {text!r} is not a number") from None
    if not np.isfinite(v) or (positive and not v > 0):
        raise ValueError(f"{where}: {key} {text} must be {'positive and ' if positive else ''}finite")
    return v


def parse_fgm_properties(txt: str, table: Table | None = None) -> dict:
    """{"model": 1, "combustionModel": "flareFGM", "scaledPV", "combustion", "solveEnthalpy", "flameletT", "Sct", "Sc",
    "incompPref", "TMin", "TMax", "tablePath", "omega_YiNames"} from the text of constant/combustionProperties.
    Refused by name: a combustionModel other than flareFGM (DeePFGM among them); buffer true or bufferTime > 0;
    relaxation, DpDt or ignition true; a p_operateDim that differs from incompPref; an unknown flareFGMCoeffs entry;
    and, given the table, a scaledPV or an omega_YiNames list that disagrees with it (flareFGM.C:50-70)."""
    where = "combustionProperties flareFGMCoeffs"
    txt = strip_comments(txt)
    name = dict(dict_entries(txt)).get("combustionModel")
    if name is None:
        raise ValueError("combustionProperties: no combustionModel entry")
    if name == "DeePFGM":
        raise ValueError("combustionProperties: combustionModel DeePFGM is not supported (its table is a neural network; flareFGM)")
    if name != "flareFGM":
        raise ValueError(f"combustionProperties: combustionModel {name} is not flareFGM (dfmi.combustion reads laminar, PaSR and EDC)")
    try:
        sub = sub_dict(txt, "flareFGMCoeffs")
    except ValueError:
        raise ValueError("combustionProperties: sub-dictionary flareFGMCoeffs is not closed") from None
    if sub is None:
        raise ValueError("combustionProperties: combustionModel flareFGM without a flareFGMCoeffs sub-dictionary")
    out = dict(DEFAULTS, omega_YiNames=[])
    p_op = None
    for k, v in dict_entries(sub):
        if k in _REFUSED_SWITCHES:
            if _switch(where, k, v):
                raise ValueError(f"{where}: {k} true is not supported")
        elif k == "bufferTime":
            if _real(where, k, v, positive=False) > 0:
                raise ValueError(f"{where}: bufferTime {v} > 0 is not supported")
        elif k in ("scaledPV", "combustion", "solveEnthalpy", "flameletT"):
            out[k] = _switch(where, k, v)
        elif k in ("Sct", "Sc", "TMin", "TMax"):
            out[k] = _real(where, k, v)
        elif k == "incompPref":
            out[k] = _real(where, k, v, positive=False)
        elif k == "p_operateDim":
            p_op = _real(where, k, v, positive=False)
        elif k == "tablePath":
            out[k] = v.strip('"')
        elif k == "omega_YiNames":
            mo = re.fullmatch(r"(?:\d+\s*)?\(([^()]*)\)", v.strip())
            if mo is None:
                raise ValueError(f"{where}: omega_YiNames {v!r} is not a word list")
            out[k] = mo.group(1).split()
        elif k in _IGNORED:
            continue
        else:
            raise ValueError(f"{where}: entry {k} is not supported")
    if p_op is not None and p_op != out["incompPref"]:
        raise ValueError(f"{where}: p_operateDim {p_op} differs from incompPref {out['incompPref']} (not supported)")
    if table is not None:
        check_against_table(out, table)
    return out


def check_against_table(settings: dict, table: Table) -> None:
    """flareFGM's checks before running (flareFGM.C:50-70)"""
    if bool(settings["scaledPV"]) != table.scaled:
        raise ValueError(f"combustionProperties flareFGMCoeffs: scaledPV {str(bool(settings['scaledPV'])).lower()} disagrees "
                         f"with the table (NS = {table.NS}, NYomega = {table.NYomega}: {'scaled' if table.scaled else 'unscaled'})")
    if list(settings["omega_YiNames"]) != list(table.omega_names):
        raise ValueError(f"combustionProperties flareFGMCoeffs: omega_YiNames ({' '.join(settings['omega_YiNames'])}) disagrees "
                         f"with the table's ({' '.join(table.omega_names)})")


def read_case_fgm(case_dir: str):
    """(settings, table) of a case: constant/combustionProperties and the table at its tablePath (relative to the case)"""
    with open(os.path.join(case_dir, "constant", "combustionProperties")) as f:
        settings = parse_fgm_properties(f.read())
    if not settings["tablePath"]:
        raise ValueError("combustionProperties flareFGMCoeffs: no tablePath entry")
    path = settings["tablePath"]
    table = read_table(path if os.path.isabs(path) else os.path.join(case_dir, path))
    check_against_table(settings, table)
    return settings, table


def species_indices(table: Table, species_names: list):
    """(mechanism index of every table species, of every source-term species); a name the mechanism lacks is refused"""
    names = list(species_names)

    def index(n, what):
        if n not in names:
            raise ValueError(f"flare table: {what} {n} is not a species of the mechanism")
        return names.index(n)
    return [index(n, "species") for n in table.species_names], [index(n, "source-term species") for n in table.omega_names]


def apply_fgm(ctx, settings: dict, table: Table, species_names: list) -> None:
    """the table and the fgm.* options on a context (settings: parse_fgm_properties' result; species_names: the
    mechanism's species in field order). The model is set last: it needs the table and ras.model = 1."""
    check_against_table(settings, table)
    ysp, osp = species_indices(table, species_names)
    ctx.fgm_set_table(table, ysp, osp)
    for k in ("combustion", "solveEnthalpy", "flameletT"):
        ctx.set_option("fgm." + k, 1 if settings[k] else 0)
    for k in ("Sct", "Sc", "incompPref", "TMin", "TMax"):
        ctx.set_option("fgm." + k, settings[k])
    ctx.set_option("fgm.model", settings["model"])
