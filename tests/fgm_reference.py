"""Reference side of the flareFGM tests (include/dfmi.h, flareFGM block): seeded synthetic flamelet tables, the
drawn state classes, the retrieval restated in NumPy for any float type, and FgmOracle, the restatement of
flareFGM::correct() and of the FGM time step on ras_reference.RasOracle / scalar_assemble.

The restatement follows the header's statement order and operation order, so in float64 every output made of + - * /,
max, min, sqrt and table reads equals the device's bit for bit. chi_c inside the flame goes through
RANSsdrFLRmodel (pow, sqrt): `python tests/fgm_reference.py --measure` evaluates that formula in float64 against long
double on every table's states, from the float64 laminar lookups, and writes the maxima of |chi64 - chiL| / scale to
tests/golden/fgm_point_bounds.json; the device bound derives from that file (gpu_bound), never from a kernel's output.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUNDS_PATH = os.path.join(GOLDEN, "fgm_point_bounds.json")
for _p in (os.path.join(os.path.dirname(HERE), "deepflame-dev_amd"), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from dfmi.fgm import Table   # noqa: E402

LD = np.longdouble
SMALL, SMALLER, FOAM_SMALL = 1.0e-4, 1.0e-6, 1.0e-15
T0, RU = 298.15, 8.314e3
TABLES = ("full", "full_u", "four_d")
CLASSES = ("interior", "nodes", "outside", "no_flame", "degenerate")
N_STATES = 240
MAX_DROPPED = N_STATES // 20           # 5 %
DEFAULT_OPTS = {"combustion": 1, "solveEnthalpy": 0, "flameletT": 0, "Sct": 0.7, "Sc": 1.0, "incompPref": -10.0,
                "TMin": 200.0, "TMax": 5000.0}
STATE_FIELDS = ("Z", "Zvar", "c", "cvar", "Zcvar", "Ha", "k", "epsilon", "mu", "rho", "p")
# outputs made of + - * /, max, min, sqrt and table reads: bitwise on the device
BITWISE = ("chi_Z", "chi_Zc", "omega_c", "cOmega_c", "ZOmega_c", "Ha_s", "c_s", "Zvar_s", "cvar_s", "Zcvar_s", "Wt", "mu",
           "Cp", "Hf", "T", "psi", "rho", "rho_thermo", "Y", "omega_Yi")
_cache = {}


# ------------------------------------------------------------------------------------------------ tables
def _grid(axes):
    return np.meshgrid(*[np.asarray(a, np.float64) for a in axes], indexing="ij")


def make_table(name: str, seed: int = 11) -> Table:
    """a seeded synthetic table: smooth analytic functions of the six coordinates on non-uniform dyadic axes (so the
    `nodes` class can sit exactly on them; gz and gc start at `smaller`, the floor cal_gvar clamps to, so their first
    node is reached exactly and nothing lies below them), [Zl, Zr] narrower than the z axis and varying with h, Ycmax > 0.
    `full` (scaled) and `full_u` (unscaled) are 3 x 5 x 4 x 3 x 2 x 3 with NZL 4, NY 3, NYomega 1; `four_d` (scaled) is
    1 x 6 x 5 x 3 x 1 x 1 with NZL 3, NY 5, NYomega 2; `full_u_deg` is full_u with Ycmax = 0 on the plane z = z[0]."""
    if name in _cache:
        return _cache[name]
    rng = np.random.default_rng(seed + sum(map(ord, name.replace("_deg", ""))))
    deg = name.endswith("_deg")
    base = name[:-4] if deg else name
    if base in ("full", "full_u"):
        axes = [np.array([-262144.0, -32768.0, 131072.0]), np.array([0.0, 0.0625, 0.25, 0.5, 1.0]),
                np.array([0.0, 0.25, 0.5, 1.0]), np.array([SMALLER, 0.25, 0.5]), np.array([SMALLER, 0.5]),
                np.array([-0.5, 0.0, 0.25])]
        NZL, NY, NYo = 4, 3, 1
    elif base == "four_d":
        axes = [np.array([0.0]), np.array([0.0, 0.03125, 0.125, 0.25, 0.5, 1.0]), np.array([0.0, 0.125, 0.25, 0.5, 1.0]),
                np.array([SMALLER, 0.25, 0.5]), np.array([0.25]), np.array([0.0])]
        NZL, NY, NYo = 3, 5, 2
    else:
        raise KeyError(name)
    scaled = base != "full_u"
    NS = (8 if scaled else 9) + NYo
    H, Zg, Cg, GZ, GC, GZC = _grid(axes)
    hs = H / 262144.0
    shape = H.shape

    def wob(i):
        a = rng.uniform(0.05, 0.3, 6)
        ph = rng.uniform(0, 2 * np.pi, 6)
        return (1.0 + a[0] * np.sin(2.1 * hs + ph[0]) + a[1] * np.sin(3.3 * Zg + ph[1]) + a[2] * np.cos(2.7 * Cg + ph[2])
                + a[3] * np.sin(4.1 * GZ + ph[3]) + a[4] * np.cos(1.9 * GC + ph[4]) + a[5] * np.sin(2.3 * GZC + ph[5]) + 0.01 * i)
    bell = 4.0 * Zg * (1.0 - Zg)
    cols = [400.0 * bell * Cg * (1.0 - 0.8 * Cg) * wob(0) + 5.0,        # omgc
            300.0 * bell * Cg * Cg * wob(1) + 2.0,                     # cOc
            150.0 * bell * Zg * Cg * wob(2) + 1.0,                     # ZOc
            1100.0 * wob(3) + 300.0 * Cg,                              # cp
            28.0 * wob(4) - 6.0 * Zg,                                  # mwt
            (Zg * (-4653056.0 + 2048.0) - 2048.0) - 1.3e6 * bell * Cg * wob(5) - 5.0e4 * np.sin(3.0 * Zg + hs),   # hiyi
            300.0 + 1700.0 * bell * Cg * wob(6) * (1.0 + 0.1 * hs),    # Tf
            1.6e-5 * wob(7) * (1.0 + 6.0 * Cg * bell)]                 # nu
    for j in range(NYo):
        cols.append(-200.0 * bell * Cg * wob(8 + j) - 1.0)              # omega of the source species
    if not scaled:
        yc = np.clip(0.3 + 0.3 * bell * wob(20) * (1.0 + 0.1 * hs), 0.3, 0.9)
        if deg:
            yc = np.where(Zg == axes[1][0], 0.0, yc)
        cols.append(yc)                                                # Ycmax
    for j in range(NY):
        cols.append(np.clip(0.2 * wob(30 + j) * (Zg if j % 2 else 1.0 - Zg) * (0.3 + Cg), 0.0, 1.0))
    values = np.stack([np.broadcast_to(c, shape).reshape(-1) for c in cols]).astype(np.float64)
    NH = shape[0]
    lam = np.zeros((5, NH * NZL))
    for ih in range(NH):
        zl, zr = 0.09375 + 0.03125 * ih, 0.75 - 0.0625 * ih
        t = np.linspace(0.0, 1.0, NZL) ** 1.5
        z = zl + (zr - zl) * t
        sl = 0.1 + 0.3 * np.sin(np.pi * t) + 0.02 * ih
        lam[:, ih * NZL:(ih + 1) * NZL] = [z, sl, 4.0e-4 * (1.0 + 0.5 * t), 5.0 + 2.0 * t + 0.1 * ih, 0.7 + 0.2 * t]
    d2 = d1 = None
    if scaled:
        n3 = NH * shape[1] * shape[3]
        d2, d1 = rng.uniform(-3.0, 3.0, n3), rng.uniform(-1.0, 1.0, n3)
    sp = ["CH4", "O2", "H2O", "CO2", "CO", "H2", "N2"]
    tab = Table(axes, NS, NZL, sp[:NYo], sp[1:1 + NY] if base != "four_d" else sp[:NY], -4653056.0, -2048.0, lam, values, d2, d1)
    _cache[name] = tab
    return tab


# ------------------------------------------------------------------------------------------------ lookups
def pair(a, x, T=np.float64):
    """(loc, fac) of x on axis a (tableSolver.C:854-865; an axis of length 1 has fac = 0)"""
    a = np.asarray(a, T)
    x = np.asarray(x, T)
    n = len(a)
    if n == 1:
        return np.zeros(x.shape, np.int64), np.zeros(x.shape, T)
    # locate on the value in T (long double: the same cell unless x sits within rounding of a node)
    loc = np.clip(np.searchsorted(a, x, side="right") - 1, 0, n - 2)
    lo, hi = a[loc], a[loc + 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(x <= lo, T(0), np.where(x >= hi, T(1), np.where((hi - lo) < T(1e-30), T(0), (x - lo) / (hi - lo))))
    return loc, np.asarray(f, T)


def _w(i, f, T):
    return (T(1.0) - f) + T(i) * (T(2.0) * f - T(1.0))


def corner_factors(facs, T=np.float64):
    """the 64 factors of a 6-D lookup in the nesting's order [64, n]"""
    out = []
    for cnr in range(64):
        bits = [(cnr >> (5 - d)) & 1 for d in range(6)]
        f = _w(bits[0], facs[0], T) * _w(bits[1], facs[1], T)
        for d in range(2, 6):
            f = f * _w(bits[d], facs[d], T)
        out.append(f)
    return np.array(out)


def lookup_nd(shape, pairs, table, T=np.float64):
    """tableSolver::interp2d / 3d / 6d: the sum over the 2^d corners, first axis outermost, result = result + factor * value"""
    d = len(shape)
    table = np.asarray(table, T)
    res = np.zeros(np.shape(pairs[0][1]), T)
    for cnr in range(1 << d):
        bits = [(cnr >> (d - 1 - k)) & 1 for k in range(d)]
        f = _w(bits[0], pairs[0][1], T)
        for k in range(1, d):
            f = f * _w(bits[k], pairs[k][1], T)
        idx = np.zeros(np.shape(pairs[0][0]), np.int64)
        for k in range(d):
            idx = idx * shape[k] + (pairs[k][0] + (bits[k] if shape[k] > 1 else 0))
        res = res + f * table[idx]
    return res


def _fmax(a, b):
    return np.where(a > b, a, b)      # Foam::max


def _fmin(a, b):
    return np.where(a < b, a, b)


def gvar(mean, var, Ycmax, T=np.float64):
    mean, var = np.asarray(mean, T), np.asarray(var, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = mean * ((T(1.0) - mean) if Ycmax is None else (np.asarray(Ycmax, T) - mean))
        g = np.where((mean < T(SMALL)) | (mean > (T(1.0) - T(SMALL))), T(0.0), var / den)
    return _fmax(T(SMALLER), _fmin(T(1.0), g))


def gcor(Zvar, cvar, Zcvar, T=np.float64):
    Zvar, cvar, Zcvar = (np.asarray(a, T) for a in (Zvar, cvar, Zcvar))
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where((cvar < T(1.0e-4)) | (Zvar < T(1.0e-6)), T(0.0), Zcvar / (np.sqrt(Zvar) * np.sqrt(cvar)))
    return np.fmax(T(-1.0), np.fmin(T(1.0), g))


def rans_sdr(cvar, eps, k, nu, sl, dl, tau, kc_s, rho, T=np.float64):
    """tableSolver::RANSsdrFLRmodel: (chi_c, scale); scale = |rho / beta cvar| (|2 Kc sl / dl| + |tau C4 sl / dl| + |C3 eps / k|)"""
    cvar, eps, k, nu, sl, dl, tau, kc_s, rho = (np.asarray(a, T) for a in (cvar, eps, k, nu, sl, dl, tau, kc_s, rho))
    S, beta = T(FOAM_SMALL), T(6.7)
    Ka = (dl / (sl + S)) / (np.sqrt(nu / eps) + S)
    Kc = kc_s * tau
    C3 = T(1.5) * np.sqrt(Ka) / (T(1) + np.sqrt(Ka))
    C4 = T(1.1) / np.power(T(1) + Ka, T(0.4))
    chi = rho / beta * cvar * ((T(2.0) * Kc - tau * C4) * sl / (dl + S) + C3 * eps / (k + S))
    scale = np.abs(rho / beta * cvar) * (np.abs(T(2.0) * Kc * sl / (dl + S)) + np.abs(tau * C4 * sl / (dl + S)) + np.abs(C3 * eps / (k + S)))
    return chi, scale


def retrieve(tab: Table, opts: dict, st: dict, slot: bool = False, write_rho: bool = True, T=np.float64) -> dict:
    """flareFGM::retrieval() of the points of `st` (arrays of STATE_FIELDS) in the header's statement order. Y and omega_Yi
    come back as [NY, n] / [NYomega, n] in table order. `lam` holds the four float64 laminar lookups of the flame points
    and `flame` the mask (for the chi_c bound)."""
    o = dict(DEFAULT_OPTS, **opts)
    s = {n: np.asarray(st[n], T) for n in STATE_FIELDS}
    Z, Zvar, c, cvar, Zcvar, Ha, k, eps = (s[n] for n in ("Z", "Zvar", "c", "cvar", "Zcvar", "Ha", "k", "epsilon"))
    rho_in, mu_in = s["rho"], s["mu"]
    ax = tab.axes
    shape = tab.shape
    NZL = tab.NZL
    lam = np.asarray(tab.laminar, T).reshape(5, shape[0] * NZL)
    out = {}
    ek = T(1.0) * eps / k
    chiZ, chiZc = ek * Zvar, ek * Zcvar
    out["chi_Z"], out["chi_Zc"] = chiZ, chiZc
    hLoss = (Z * (T(tab.Hfu) - T(tab.Hox)) + T(tab.Hox)) - Ha
    hLoss = _fmax(hLoss, T(ax[0][0]))
    hLoss = _fmin(hLoss, T(ax[0][-1]))
    ph = pair(ax[0], hLoss, T)
    ih = ph[0]
    Zl, Zr = lam[0][ih * NZL], lam[0][(ih + 1) * NZL - 1]
    flame = (Z >= Zl) & (Z <= Zr) & bool(o["combustion"]) & (c > T(SMALL))
    pzl = pair(lam[0][:NZL], Z, T)
    l2 = {n: lookup_nd((shape[0], NZL), (ph, pzl), lam[i], T) for i, n in enumerate(("z", "sl", "th", "tau", "kctau"))}
    with np.errstate(divide="ignore", invalid="ignore"):
        chic_f, scale = rans_sdr(cvar, eps, k, mu_in / rho_in, l2["sl"], l2["th"], l2["tau"], l2["kctau"], rho_in, T)
        chic_n = (T(1.0) * eps / (k + T(FOAM_SMALL)) if slot else ek) * cvar
    out["chi_c"] = np.where(flame, chic_f, chic_n)
    out["flame"], out["chi_c_scale"] = flame, np.where(flame, scale, np.abs(chic_n))
    out["lam"] = {n: l2[n] for n in ("sl", "th", "tau", "kctau")}
    gz = gvar(Z, Zvar, None, T)
    gcz = gcor(Zvar, cvar, Zcvar, T)
    pz, pgz = pair(ax[1], Z, T), pair(ax[3], gz, T)
    vals = np.asarray(tab.values, T)
    if tab.scaled:
        Ycmax, cNorm = None, c
    else:
        zero = np.zeros_like(Z)
        q = (ph, pz, pair(ax[2], zero, T), pgz, pair(ax[4], zero, T), pair(ax[5], zero, T))
        Ycmax = _fmax(T(SMALLER), lookup_nd(shape, q, vals[tab.NS - 1], T))
        cNorm = c / Ycmax
    gc = gvar(c, cvar, Ycmax, T)
    p6 = (ph, pz, pair(ax[2], cNorm, T), pgz, pair(ax[4], gc, T), pair(ax[5], gcz, T))
    out["pairs"] = p6
    L = [lookup_nd(shape, p6, vals[v], T) for v in range(8)]
    if tab.scaled:
        p3 = (ph, pz, pgz)
        s3 = (shape[0], shape[1], shape[3])
        extra = chiZ * c * lookup_nd(s3, p3, tab.d2Yeq, T) + T(2.0) * chiZc * lookup_nd(s3, p3, tab.d1Yeq, T)
    else:
        extra = np.zeros_like(Z)
    zero = np.zeros_like(Z)
    out["omega_c"] = np.where(flame, L[0] + extra, zero) * rho_in
    out["cOmega_c"] = np.where(flame, L[1], zero) * rho_in
    out["ZOmega_c"] = np.where(flame, L[2], zero) * rho_in
    out["Ha_s"], out["c_s"], out["Zvar_s"], out["cvar_s"], out["Zcvar_s"] = hLoss, cNorm, gz, gc, gcz
    out["Wt"] = L[4]
    out["mu"] = L[7] * rho_in
    out["omega_Yi"] = np.array([lookup_nd(shape, p6, vals[tab.NS - tab.NYomega + j], T) for j in range(tab.NYomega)]).reshape(tab.NYomega, -1)
    out["Y"] = np.array([lookup_nd(shape, p6, vals[tab.NS + j], T) for j in range(tab.NY)]).reshape(tab.NY, -1)
    if o["flameletT"]:
        Tt = L[6]
        out["Cp"] = out["Hf"] = None      # untouched
    else:
        out["Cp"], out["Hf"] = L[3], L[5]
        with np.errstate(divide="ignore", invalid="ignore"):
            Tt = (Ha - L[5]) / L[3] + T(T0)
    Tt = _fmin(_fmax(Tt, T(o["TMin"])), T(o["TMax"]))
    out["T"] = Tt
    psi = L[4] / (T(RU) * Tt)
    out["psi"] = psi
    if slot or write_rho:
        r = (T(o["incompPref"]) if o["incompPref"] > 0 else s["p"]) * psi
        out["rho"] = out["rho_thermo"] = r
    else:
        out["rho"] = out["rho_thermo"] = rho_in
    return out


# ------------------------------------------------------------------------------------------------ state classes
def degenerate_table(name):
    """the table a class runs on: `degenerate` of the unscaled table needs a corner with Ycmax <= 1e-6"""
    return name + "_deg" if name == "full_u" else name


def class_table(name, cls):
    return make_table(degenerate_table(name) if cls == "degenerate" else name)


def states(name: str, cls: str, seed: int = 5):
    """(state dict of N_STATES points minus the dropped ones, number dropped). A class drops the draws its own condition
    rejects; the cap MAX_DROPPED is asserted. no_flame: a third with Z outside [Zl, Zr], a third with c <= 1e-4, and a
    third that burns unless the run switches combustion off (class_combustion)."""
    tab = class_table(name, cls)
    rng = np.random.default_rng(seed + 101 * TABLES.index(name) + 7 * CLASSES.index(cls))
    n = N_STATES
    ax = tab.axes
    dH = tab.Hfu - tab.Hox

    def between(a, lo=0.05, hi=0.95):
        a = np.asarray(a)
        if len(a) == 1:
            return np.full(n, a[0])
        i = rng.integers(0, len(a) - 1, n)
        return a[i] + rng.uniform(lo, hi, n) * (a[i + 1] - a[i])
    # the defaults sit strictly inside every axis (an axis of length 1: anywhere)
    Z = between(ax[1])
    cfrac = between(ax[2])
    gz_t = between(ax[3]) if len(ax[3]) > 1 else rng.uniform(0.02, 0.9, n)
    gc_t = between(ax[4]) if len(ax[4]) > 1 else rng.uniform(0.02, 0.9, n)
    r_t = between(ax[5]) if len(ax[5]) > 1 else rng.uniform(-0.9, 0.9, n)
    h_t = between(ax[0]) if len(ax[0]) > 1 else np.zeros(n)
    k = rng.uniform(0.1, 1.0, n)
    eps = 10.0 ** rng.uniform(2.0, 4.0, n)
    mu = rng.uniform(1.5e-5, 6e-5, n)
    rho = rng.uniform(0.2, 1.2, n)
    p = 101325.0 * rng.uniform(0.9, 1.1, n)
    keep = np.ones(n, bool)
    ymax = np.ones(n)

    if cls == "nodes":
        Z = ax[1][rng.integers(0, len(ax[1]), n)]
        h_t = ax[0][rng.integers(0, len(ax[0]), n)]
        gz_t = ax[3][rng.integers(0, len(ax[3]), n)]
        gc_t = ax[4][rng.integers(0, len(ax[4]), n)]
        r_t = ax[5][rng.integers(0, len(ax[5]), n)]
        # unscaled: cNorm = 1 means c = Ycmax, where the reference's own gc is 0 / 0; the last c node is left out there
        cfrac = ax[2][rng.integers(0, len(ax[2]) - (0 if tab.scaled else 1), n)]
        zero_zvar, zero_cvar = gz_t == ax[3][0], (gc_t == ax[4][0]) & (len(ax[4]) > 1)
    elif cls == "outside":
        g = rng.integers(0, 2, (6, n))
        Z = np.where(g[0], rng.uniform(-0.2, -0.01, n), rng.uniform(1.01, 1.2, n))
        h_t = np.where(g[1], ax[0][0] - rng.uniform(1e3, 1e5, n), ax[0][-1] + rng.uniform(1e3, 1e5, n))
        cfrac = np.where(g[2], rng.uniform(-0.3, -0.01, n), rng.uniform(1.05, 1.5, n))
        # Z outside (0, 1) gives gz = 0 -> smaller (below the axis); half the points keep Z inside and push gz above it
        inside = rng.integers(0, 2, n).astype(bool)
        Z = np.where(inside, rng.uniform(0.1, 0.9, n), Z)
        gz_t = np.where(g[3], rng.uniform(0.0, 0.03, n), rng.uniform(0.6, 2.0, n))
        gc_t = np.where(g[4], rng.uniform(0.0, 0.05, n), rng.uniform(0.7, 2.0, n))
        r_t = np.where(g[5], rng.uniform(-3.0, -0.6, n), rng.uniform(0.6, 3.0, n))
        cfrac = np.where(inside & (rng.integers(0, 2, n) == 1), rng.uniform(0.1, 0.9, n), cfrac)
    elif cls == "no_flame":
        third = np.arange(n) // (n // 3)
        lamz = np.asarray(tab.laminar)[0]
        zl, zr = lamz[0], lamz[tab.NZL - 1]
        Z = np.where(third == 0, np.where(rng.integers(0, 2, n) == 1, rng.uniform(0.001, 0.9 * zl, n), rng.uniform(0.8, 0.99, n)), Z)
        cfrac = np.where(third == 1, rng.uniform(0.0, 9e-5, n), cfrac)
    elif cls == "degenerate":
        g = np.arange(n) % 6
        Z = np.where(g == 0, np.where(rng.integers(0, 2, n) == 1, rng.uniform(0.0, 9e-5, n), 1.0 - rng.uniform(0.0, 9e-5, n)), Z)
        cfrac = np.where(g == 1, np.where(rng.integers(0, 2, n) == 1, rng.uniform(0.0, 9e-5, n), 1.0 - rng.uniform(0.0, 9e-5, n)), cfrac)
        if not tab.scaled:
            Z = np.where(g == 5, rng.uniform(0.0, 0.03, n), Z)          # towards the Ycmax = 0 plane z = z[0]
    # variances from the targets; unscaled: c and cvar are scaled by the point's Ycmax (looked up at the final gz)
    m = Z * (1.0 - Z)
    Zvar = gz_t * m
    if cls == "nodes":
        Zvar = np.where(zero_zvar, 0.0, Zvar)      # gz's first node is the clamp's floor
    if cls == "degenerate":
        Zvar = np.where(g == 3, rng.uniform(0.0, 9e-7, n), Zvar)
    Ha = (Z * dH + tab.Hox) - h_t
    if tab.scaled:
        ymax = np.ones(n)
    else:
        st0 = {f: np.zeros(n) for f in STATE_FIELDS}
        st0.update(Z=Z, Zvar=Zvar, Ha=Ha, k=k, epsilon=eps, mu=mu, rho=rho, p=p)
        with np.errstate(all="ignore"):
            c0 = retrieve(tab, {}, st0)
        # c_s = c / Ycmax with c = 0 is 0; Ycmax itself: evaluate through the lookup used by retrieve
        zero = np.zeros(n)
        q = (pair(ax[0], c0["Ha_s"]), pair(ax[1], Z), pair(ax[2], zero), pair(ax[3], c0["Zvar_s"]), pair(ax[4], zero), pair(ax[5], zero))
        ymax = np.maximum(SMALLER, lookup_nd(tab.shape, q, tab.values[tab.NS - 1]))
    c = cfrac * ymax
    cm = c * ((1.0 if tab.scaled else ymax) - c)
    cvar = gc_t * cm
    if cls == "nodes":
        cvar = np.where(zero_cvar, 0.0, cvar)
    if cls == "degenerate":
        cvar = np.where(g == 2, rng.uniform(0.0, 9e-5, n), cvar)
    with np.errstate(invalid="ignore"):
        Zcvar = r_t * (np.sqrt(np.abs(Zvar)) * np.sqrt(np.abs(cvar)))
    if cls == "degenerate":
        with np.errstate(invalid="ignore"):
            Zcvar = np.where(g == 4, np.where(rng.integers(0, 2, n) == 1, 1.5, -1.5) * (np.sqrt(np.abs(Zvar)) * np.sqrt(np.abs(cvar))), Zcvar)
    st = {"Z": Z, "Zvar": Zvar, "c": c, "cvar": cvar, "Zcvar": Zcvar, "Ha": Ha, "k": k, "epsilon": eps, "mu": mu, "rho": rho, "p": p}
    with np.errstate(all="ignore"):
        r = retrieve(tab, {}, st)
    finite = np.all([np.isfinite(np.asarray(v, np.float64)).reshape(-1, n).all(axis=0) for kk, v in r.items()
                     if kk in BITWISE and v is not None] + [np.isfinite(r["chi_c"])], axis=0)
    keep &= finite
    if cls == "nodes":      # the class's own condition: every coordinate exactly on a node
        for d, x in enumerate((r["Ha_s"], Z, r["c_s"], r["Zvar_s"], r["cvar_s"], r["Zcvar_s"])):
            if len(ax[d]) > 1:
                keep &= np.isin(x, ax[d])
    elif cls == "interior":
        for d, x in enumerate((r["Ha_s"], Z, r["c_s"], r["Zvar_s"], r["cvar_s"], r["Zcvar_s"])):
            if len(ax[d]) > 1:
                keep &= (x > ax[d][0]) & (x < ax[d][-1]) & ~np.isin(x, ax[d])
    dropped = int(n - keep.sum())
    assert dropped <= MAX_DROPPED, (name, cls, dropped)
    return {f: np.ascontiguousarray(v[keep]) for f, v in st.items()}, dropped


def class_combustion(cls, n_kept=0):
    """per-run combustion switch: no_flame runs its states twice, once with combustion off"""
    return (1, 0) if cls == "no_flame" else (1,)


# ------------------------------------------------------------------------------------------------ chi_c bound
def chi_c_error(tab, opts, st, chi, slot=False):
    """|chi - chi_longdouble| / scale per flame point: the RANSsdrFLRmodel formula in long double from the float64 laminar
    lookups (which are bitwise on the device) and the float64 inputs; 0 outside the flame, where chi_c is bitwise"""
    r = retrieve(tab, opts, st, slot=slot)
    fl = r["flame"]
    l2 = r["lam"]
    with np.errstate(all="ignore"):
        nu64 = np.asarray(st["mu"], np.float64) / np.asarray(st["rho"], np.float64)
        chiL, scL = rans_sdr(st["cvar"], st["epsilon"], st["k"], nu64, l2["sl"], l2["th"], l2["tau"], l2["kctau"], st["rho"], LD)
        err = np.where(fl, np.abs(np.asarray(chi, LD) - chiL) / np.where(scL > 0, scL, 1), 0)
    return np.asarray(err, np.float64), fl


def measure():
    out = {}
    for name in TABLES:
        out[name] = {}
        for cls in CLASSES:
            tab = class_table(name, cls)
            st, dropped = states(name, cls)
            worst, nfl = 0.0, 0
            for comb in class_combustion(cls, 0):
                for slot in (False, True):
                    o = {"combustion": comb}
                    r = retrieve(tab, o, st, slot=slot)
                    e, fl = chi_c_error(tab, o, st, r["chi_c"], slot)
                    worst, nfl = max(worst, float(e.max()) if e.size else 0.0), max(nfl, int(fl.sum()))
            out[name][cls] = {"chi_c": worst, "flame_points": nfl, "states": int(len(st["Z"])), "dropped": dropped}
    return out


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def gpu_bound(bounds, name, cls):
    """4x the fp64 restatement's measured maximum for that table and class, floored at 1e-13"""
    return max(4.0 * bounds["tables"][name][cls]["chi_c"], 1e-13)


# ------------------------------------------------------------------------------------------------ transport and oracle
EQS = ("Z", "Zvar", "c", "cvar", "Zcvar", "Ha")
CLIP = {"Z": (0.0, 1.0), "Zvar": (0.0, 0.25), "c": (0.0, 1.0), "cvar": (0.0, 0.25), "Zcvar": (-0.25, 0.25)}
FGM_OUT = ("chi_Z", "chi_Zc", "chi_c", "omega_c", "cOmega_c", "ZOmega_c", "Ha_s", "c_s", "Zvar_s", "cvar_s", "Zcvar_s", "Wt",
           "Cp", "Hf")


def diffusivity(rho, nut, mu, Sct, Sc):
    """D = (rho nut) / Sct + mu / Sc (cells and slots alike)"""
    return (np.asarray(rho) * np.asarray(nut)) / Sct + np.asarray(mu) / Sc


def source(eq, Sct, rho, nut, g1=None, g2=None, chi=None, omc=None, xOmc=None, psi=None):
    """Su per unit volume of equation eq (k_fgm_source's operation order)"""
    if eq in ("Z", "Ha"):
        return np.zeros_like(rho)
    if eq == "c":
        return np.array(omc, dtype=np.float64)
    dot = (g1[0] * g2[0] + g1[1] * g2[1]) + g1[2] * g2[2]
    v = ((2.0 * (rho * nut)) / Sct) * dot - (2.0 * rho) * chi
    if eq == "Zvar":
        return v
    if eq == "cvar":
        return v + 2.0 * (xOmc - omc * psi)
    return v + (xOmc - omc * psi)


def clip(eq, v):
    if eq not in CLIP:
        return v
    lo, hi = CLIP[eq]
    v = np.where(v < hi, v, hi)
    return np.where(v > lo, v, lo)


def out01(ph, vP, vN):
    return (ph > 0 and (vP < 0 or vN > 1)) or (ph < 0 and (vN < 0 or vP > 1))


def limited_weights(tp, ptypes, scheme, phi, bphi, v, bv, g):
    """the convection weights of one scalar under `upwind` (None, None), `limitedLinear k` or `limitedLinear01 k`:
    ras_reference.limited_weights, and for limitedLinear01 the limiter zeroed where a face's values leave [0, 1]
    (fv_kernels.hip out01)"""
    import ras_reference as R
    tok = scheme.replace("Gauss", "").split()
    if tok[0] == "upwind":
        return None, None
    k = float(tok[1])
    w, bw = R.limited_weights(tp, ptypes, k, phi, bphi, v, bv, g)
    if tok[0] == "limitedLinear01":
        m = tp.m
        for f in range(m.n_faces):
            if out01(phi[f], v[m.owner[f]], v[m.neighbour[f]]):
                w[f] = 1.0 if phi[f] >= 0 else 0.0
        import nonorth_reference as NR
        ts = NR.slot_types(m, ptypes)
        for b in range(m.n_boundary_slots):
            if ts[b] in R.COUPLED and tp.sl.prim[b]:
                pc = tp.sl.partner[b]
                if out01(bphi[b], v[tp.sl.cell[b]], v[pc] if pc >= 0 else bv[b]):
                    bw[b] = 1.0 if bphi[b] >= 0 else 0.0
    return w, bw


def make_oracle(*args, **kw):
    """FgmOracle(...) (the class is built on first use: ras_reference loads the compiled oracle)"""
    import ras_reference as R

    class FgmOracle(R.RasOracle):
        """RasOracle with flareFGM::correct() and the FGM time step restated on it. tab: the flamelet table; opts: the
        fgm.* options; fields: Z .. Ha and their boundary values; fgm_ptypes: {field: patch types}; ysp: the mechanism
        index of every table species; schemes_fgm: {field: scheme text} (default upwind). dc / bdc (attributes, default
        None): the delta coefficients of the laplacian scheme in force, for the matrix comparison on a skewed mesh."""

        def __init__(self, mesh, table, state, ptypes, inert, rdt, ras, k, epsilon, bk, beps, tab, opts, fields, fgm_ptypes,
                     ysp, schemes_fgm=None, **kw):
            super().__init__(mesh, table, state, ptypes, inert, rdt, ras, k, epsilon, bk, beps, **kw)
            self.tab, self.o, self.ysp = tab, dict(DEFAULT_OPTS, **opts), list(ysp)
            self.fgm_pt = fgm_ptypes
            self.sch = dict({n: "upwind" for n in EQS}, **(schemes_fgm or {}))
            C_, B = mesh.n_cells, mesh.n_boundary_slots
            for n in EQS:
                self._i("ptype_" + n, fgm_ptypes[n])
                self.ptypes[n] = fgm_ptypes[n]
                self._d(n, fields[n]); self._d("boundary_" + n, fields["boundary_" + n])
            for n in FGM_OUT:
                for pre, cnt in (("", C_), ("boundary_", B)):
                    self._d(pre + n, fields.get(pre + n, np.zeros(cnt)))
            no = max(tab.NYomega, 1)
            self._d("omega_Yi", fields.get("omega_Yi", np.zeros((no, C_))))
            self._d("boundary_omega_Yi", fields.get("boundary_omega_Yi", np.zeros((no, B))))
            for pre in ("", "boundary_"):
                if pre + "rho_thermo" not in self.arr:
                    self._d(pre + "rho_thermo", self.arr[pre + "rho"].copy())
            self.matrices = {}

        def grad(self, nm):
            C_ = self.m.n_cells
            self._d("fgm_v", self.arr[nm]); self._d("fgm_bv", self.arr["boundary_" + nm])
            g = self.out("fgm_g", 3 * C_)
            self._run("orc_grad_scalar", b"fgm_v", b"fgm_bv", ("ptype_" + nm).encode(), b"fgm_g", None)
            return g.reshape(3, C_).copy()

        def assemble(self, eq):
            a, o = self.arr, self.o
            rho, nut = a["rho"], a["nut"]
            kw = {}
            if eq == "Zvar":
                g = self.grad("Z")
                kw = dict(g1=g, g2=g, chi=a["chi_Z"])
            elif eq == "cvar":
                g = self.grad("c")
                kw = dict(g1=g, g2=g, chi=a["chi_c"], xOmc=a["cOmega_c"], psi=a["c"])
            elif eq == "Zcvar":
                kw = dict(g1=self.grad("Z"), g2=self.grad("c"), chi=a["chi_Zc"], xOmc=a["ZOmega_c"], psi=a["Z"])
            Su = source(eq, o["Sct"], rho, nut, omc=a["omega_c"], **kw)
            D = diffusivity(rho, nut, a["mu"], o["Sct"], o["Sc"])
            bD = diffusivity(a["boundary_rho"], a["boundary_nut"], a["boundary_mu"], o["Sct"], o["Sc"])
            wc = bwc = None
            if self.sch[eq].replace("Gauss", "").split()[0] != "upwind":
                wc, bwc = limited_weights(self.tp, self.fgm_pt[eq], self.sch[eq], a["phi"], a["boundary_phi"], a[eq],
                                          a["boundary_" + eq], self.grad(eq))
            mat = R.scalar_assemble(self.tp, self.fgm_pt[eq], a[eq], a["boundary_" + eq], rho, a["rho_old"], a["phi"],
                                    a["boundary_phi"], D, bD, Su, np.zeros_like(rho), self.rdt, wc=wc, bwc=bwc,
                                    dc=getattr(self, "dc", None), bdc=getattr(self, "bdc", None))
            self.matrices[eq] = dict(mat, Su=Su, D=D, bD=bD)
            return mat

        def equation(self, eq):
            a = self.arr
            q = self.assemble(eq)
            a[eq][...] = self.solve_ldu(q["lower"], q["upper"], q["diag"], q["source"], q["internal_coeffs"],
                                        q["boundary_coeffs"], eq)
            self.correct_bc(eq, eq, 1)
            for pre in ("", "boundary_"):
                a[pre + eq][...] = clip(eq, a[pre + eq])

        def retrieval(self, write_rho=True):
            a, tab = self.arr, self.tab
            import nonorth_reference as NR
            ts = NR.slot_types(self.m, self.ptypes["calculated"])
            for pre, slot in (("", False), ("boundary_", True)):
                st = {n: a[pre + ("epsilon" if n == "epsilon" else n)] for n in STATE_FIELDS}
                with np.errstate(all="ignore"):
                    r = retrieve(tab, self.o, st, slot=slot, write_rho=write_rho)
                live = np.ones(len(st["Z"]), bool) if not slot else ts != 3      # empty slots are untouched
                for n in FGM_OUT + ("mu", "T", "psi", "rho", "rho_thermo"):
                    if r[n] is not None:
                        a[pre + n][live] = r[n][live]
                for j in range(tab.NY):
                    a[pre + "Y"][self.ysp[j]][live] = r["Y"][j][live]
                for j in range(tab.NYomega):
                    a[pre + "omega_Yi"][j][live] = r["omega_Yi"][j][live]

        def fgm_correct(self):
            self.equation("Z")
            self.equation("Zvar")
            if self.o["combustion"]:
                for eq in ("c", "cvar", "Zcvar"):
                    self.equation(eq)
            a = self.arr
            if self.o["solveEnthalpy"]:
                self.equation("Ha")
            else:
                for pre in ("", "boundary_"):
                    a[pre + "Ha"][...] = a[pre + "Z"] * (self.tab.Hfu - self.tab.Hox) + self.tab.Hox
            self.retrieval(True)

        def time_step(self, n_corr=2):
            m = self.m
            C_, B = m.n_cells, m.n_boundary_slots
            a = self.arr
            for n, o in (("rho_old", "rho"), ("boundary_rho_old", "boundary_rho"), ("phi_old", "phi"),
                         ("boundary_phi_old", "boundary_phi"), ("U_old", "U"), ("boundary_U_old", "boundary_U"),
                         ("K_old", "K"), ("p_old", "p"), ("boundary_p_old", "boundary_p")):
                a[n][...] = a[o]
            self.rho_eqn()
            u = self.u_assemble()
            for k in range(3):
                a["U"][k] = self.solve_ldu(u["lower"], u["upper"], u["diag"], u["source_solve"][k * C_:(k + 1) * C_],
                                           u["internal_coeffs"][k * B:(k + 1) * B], u["boundary_coeffs"][k * B:(k + 1) * B], "U")
            self.correct_bc("U", "U", 3)
            Ux, Uy, Uz = a["U"]
            a["K"][...] = 0.5 * (Ux * Ux + Uy * Uy + Uz * Uz)
            bx, by, bz = a["boundary_U"]
            a["boundary_K"][...] = 0.5 * (bx * bx + by * by + bz * bz)
            self.fgm_correct()
            for i in range(n_corr):
                for pre in ("", "boundary_"):
                    a[pre + "rho"][...] = a[pre + "rho_thermo"]
                    a[pre + "psip0"][...] = a[pre + "psi"] * a[pre + "p"]
                self.u_hbya()
                pq = self.p_assemble()
                a["p"][...] = self.solve_ldu(pq["lower"], pq["upper"], pq["diag"], pq["source"], pq["internal_coeffs"],
                                             pq["boundary_coeffs"], "p")
                self.p_post()
                for pre in ("", "boundary_"):
                    a[pre + "rho_thermo"][...] = a[pre + "rho_thermo"] + (a[pre + "psi"] * a[pre + "p"] - a[pre + "psip0"])
                self.rho_eqn()
            self.turbulence_correct()
            for pre in ("", "boundary_"):
                a[pre + "rho"][...] = a[pre + "rho_thermo"]

    return FgmOracle(*args, **kw)


def cpu_state(m):
    """a complete oracle state formed without a GPU (ras_reference.ras_state: the noisy Taylor-Green flow, k, epsilon;
    nonorth_reference.case_state: p, Y and the thermo's transport), every other array of the solver zero:
    (thermo table, state, patch types, inert index)"""
    import nonorth_reference as NR
    import ras_reference as R
    from dfmi import case
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "Burke2012_s9r23.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_Burke2012_s9r23.txt"), ym["species"])
    C_, B, F = m.n_cells, m.n_boundary_slots, m.n_faces
    rs, cs = R.ras_state(m), NR.case_state(m)
    st = {}
    for n in case.SCALARS:
        st[n], st["boundary_" + n] = np.zeros(C_), np.zeros(B)
    for n in case.VECTORS:
        st[n], st["boundary_" + n] = np.zeros((3, C_)), np.zeros((3, B))
    for n in case.SPECIES:
        st[n], st["boundary_" + n] = np.zeros((t.S, C_)), np.zeros((t.S, B))
    for n in case.FACES:
        st[n], st["boundary_" + n] = np.zeros(F), np.zeros(B)
    for n, k in case.BOUNDARY_ONLY.items():
        k = t.S if k == "S" else k
        st[n] = np.zeros((k, B)) if k > 1 else np.zeros(B)
    for n in ("U", "rho", "mu", "phi"):
        st[n], st["boundary_" + n] = rs[n], rs["boundary_" + n]
    for n in ("p", "Y", "he", "alpha", "rhoD", "hai"):
        st[n], st["boundary_" + n] = cs[n], cs["boundary_" + n]
    st["rho_old"], st["boundary_rho_old"] = st["rho"].copy(), st["boundary_rho"].copy()
    st["psi"], st["boundary_psi"] = st["rho"] / st["p"], st["boundary_rho"] / st["boundary_p"]
    st["T"], st["boundary_T"] = np.full(C_, 300.0), np.full(B, 300.0)
    for n in ("k", "epsilon"):
        st["ras_" + n], st["ras_boundary_" + n] = rs[n], rs["boundary_" + n]
    return t, st, case.default_patch_types(m), cs["inert"]


if __name__ == "__main__":
    if "--measure" not in sys.argv:
        sys.exit("usage: fgm_reference.py --measure")
    doc = {"about": "max over the flame points of |chi_c_fp64 - chi_c_longdouble| / (|rho / 6.7 cvar| (|2 Kc sl / dl| + |tau C4 sl / dl| "
                    "+ |C3 eps / k|)) of the NumPy restatement of RANSsdrFLRmodel on the drawn states of every table and class "
                    "(tests/fgm_reference.py); written by tests/fgm_reference.py --measure",
           "tables": measure()}
    with open(BOUNDS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, per in doc["tables"].items():
        for cls, v in per.items():
            print(name, cls, v)
