"""Point reference of the Peng-Robinson real-fluid thermo update (include/dfmi.h dfmi_thermo_set_eos),
the states the kernels are tested at, and the oracle of the real-fluid time step.

The model, per state, from Y [S], p and T or he (kmol, m^3/kmol; a in Pa m^6/kmol^2), written once for any NumPy
float type -- long double (x87 extended, 64-bit mantissa) is the reference, float64 the restatement whose error
against it sets the GPU tolerances:

    kappa_i = 0.37464 + 1.54226 w - 0.26992 w^2 (w <= 0.491), else 0.379642 + 1.487503 w - 0.164423 w^2 + 0.016666 w^3
    Tc_i    = (Omega_b / Omega_a) a_i / (b_i R)          s_i(T) = 1 + kappa_i (1 - sqrt(T / Tc_i))
    A0 = sum_i X_i sqrt(a_i) |s_i|      (a alpha) = A0^2      b = sum_i X_i b_i
    Q  = sum_i X_i sqrt(a_i) sign(s_i) kappa_i / sqrt(Tc_i)   A1 = dA0/dT = -Q / (2 sqrt T)   A2 = Q / (4 T sqrt T)
    (a alpha)' = 2 A0 A1                (a alpha)'' = 2 (A1^2 + A0 A2)
    A = (a alpha) p / (R T)^2, B = b p / (R T):   Z^3 - (1 - B) Z^2 + (A - 3 B^2 - 2 B) Z - (A B - B^2 - B^3) = 0
    closed-form roots (Cardano for one real root, the trigonometric form for three), each polished by Newton steps on
    the cubic to rounding; of the largest and the smallest root above B the one with the lower
    ln phi = Z - 1 - ln(Z - B) - A / (2 sqrt2 B) L,   L = log1p(2 sqrt2 B / (Z + (1 - sqrt2) B))
    rho = p Wm / (Z R T)
    h   = h_ig + [R T (Z - 1) + (T (a alpha)' - (a alpha)) / (2 sqrt2 b) L] / Wm
    cp  = cp_ig + [-R + T (a alpha)'' / (2 sqrt2 b) L - T (dp/dT)_v^2 / (dp/dv)_T] / Wm
    T(he): Newton, dT = (h - he) / cp, from the stored T, until |dT| <= 4 eps T, or the step has stopped shrinking
           below 1e-9 T, at most 40 steps (float64; the long-double reference takes 200)
    psi = (rho(he, p) - rho(he, p (1 - dx))) / (dx p), dx = 1e-4: a second constant-enthalpy solve, started at T
    mu, lambda: the ideal fits;  alpha = lambda / cp;  rhoD_i = (p D_i) rho / p;  hai_i = h_i,ig(T)

The transport at the final T comes from the existing references (thermo_reference.evaluate in long double,
oracle.thermo_points in float64) and is rescaled by cp_ig / cp and (rho / p) / psi_ig.

`python tests/realfluid_reference.py --measure` writes tests/golden/realfluid_point_bounds.json.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

import thermo_reference as R

LD = np.longdouble
F64 = np.float64
R_GAS = R.R_GAS
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUNDS_PATH = os.path.join(GOLDEN, "realfluid_point_bounds.json")
FIXTURE = os.path.join(GOLDEN, "pr_bfer6.json")
OMEGA_A = 0.45723552892138218
OMEGA_B = 0.0777960739038885
DX = 1e-4
T_FIT_LOW = 100.0       # bfer6: the transport fits start here (bfer6())
KINK_MARGIN = 1e-6      # no test state within this fraction of T of a temperature where some s_i = 0
DLNPHI_MIN = 1e-6       # three admissible roots: the outer two differ by at least this in ln phi
MAX_DROP = 0.05
CLASSES = ("supercritical", "dense", "near_critical", "three_root", "dilute", "newton", "zeros", "pure")
QUANTITIES = R.QUANTITIES
TABLES = ("bfer6", "drawn2", "drawn9", "drawn16")

R._dfmi_path()


# ------------------------------------------------------------------------------------------------ species sets
def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


_tables: dict = {}


def bfer6():
    """(ThermoTable, eos) of the six species of the supercritical Taylor-Green case: the table is fitted by
    dfmi.transport_fit from the committed gri30.yaml rows of the same species, the cubic parameters are the fixture's.
    The transport fits are made from T_FIT_LOW = 100 K upwards, the coldest state of the classes below: a fit made over
    the NASA range alone (300-3500 K) and evaluated at 118 K gives H2O a negative conductivity and a fit polynomial
    that cancels to 1 part in 4e4, which is an error of the table and not of whoever evaluates it."""
    if "bfer6" not in _tables:
        from dfmi.mech import read_yaml_mechanism
        from dfmi.transport_fit import fit_mechanism
        fx = load_fixture()
        ym = read_yaml_mechanism(os.path.join(GOLDEN, "gri30.yaml"))
        idx = [ym["species"].index(n) for n in fx["species"]]
        sub = {"species": list(fx["species"]), "W": np.asarray(ym["W"])[idx], "nasa": np.asarray(ym["nasa"])[idx],
               "transport": [ym["transport"][i] for i in idx], "trange": [(T_FIT_LOW, ym["trange"][i][1]) for i in idx]}
        t = fit_mechanism(sub)
        assert np.allclose(t.W, fx["W"], rtol=1e-3)
        _tables["bfer6"] = (t, {"a": np.array(fx["a"]), "b": np.array(fx["b"]), "w": np.array(fx["acentric"])})
    return _tables["bfer6"]


def drawn(S, seed=5):
    """(ThermoTable, eos) with S species: thermo_reference.gri_table(S) and cubic parameters drawn in the physical
    range (Tc 300-650 K, pc 2-8 MPa, acentric factor 0-0.6, so both kappa branches occur). Tc starts at 300 K so that
    the sub-critical classes (dense: 0.66-0.84 Tc, three_root: 0.7-0.9 Tc) stay above 198 K, inside the range that
    table's transport fits were made over (200 K upwards); its supercritical and zeros classes start at 200 K too."""
    key = f"drawn{S}"
    if key not in _tables:
        rng = np.random.default_rng([seed, S])
        Tc = rng.uniform(300.0, 650.0, S); pc = rng.uniform(2e6, 8e6, S); w = rng.uniform(0.0, 0.6, S)
        _tables[key] = (R.gri_table(S), {"a": OMEGA_A * (R_GAS * Tc) ** 2 / pc, "b": OMEGA_B * R_GAS * Tc / pc, "w": w})
    return _tables[key]


def table(name):
    return bfer6() if name == "bfer6" else drawn(int(name[5:]))


# ------------------------------------------------------------------------------------------------ the model
def _c(dt, x):
    return np.asarray(x, dtype=dt)


def species_params(eos, dt=F64):
    """kappa, Tc, sqrt(a), 1 / sqrt(Tc) per species (a_i = 0: no attraction, 1 / sqrt(Tc) := 0)"""
    a, b, w = _c(dt, eos["a"]), _c(dt, eos["b"]), _c(dt, eos["w"])
    kap = np.where(w <= dt(0.491), dt(0.37464) + dt(1.54226) * w - dt(0.26992) * w * w,
                   dt(0.379642) + dt(1.487503) * w - dt(0.164423) * w * w + dt(0.016666) * w * w * w)
    Tc = (dt(OMEGA_B) / dt(OMEGA_A)) * a / (b * dt(R_GAS))
    with np.errstate(divide="ignore"):
        rsTc = np.where(Tc > 0, 1 / np.sqrt(np.where(Tc > 0, Tc, 1)), dt(0))
    return {"kap": kap, "Tc": Tc, "sqa": np.sqrt(a), "rsTc": rsTc, "b": b}


def kink_temperatures(eos):
    """T where s_i = 0: Tc_i (1 + 1 / kappa_i)^2"""
    q = species_params(eos)
    return q["Tc"] * (1 + 1 / q["kap"]) ** 2


class Mix:
    """composition-dependent constants of n states"""

    def __init__(self, t, eos, Y, dt):
        self.dt = dt
        self.t = t
        self.q = species_params(eos, dt)
        W = _c(dt, t.W)[:, None]
        self.Y = _c(dt, Y)
        yw = self.Y / W
        self.X = yw / yw.sum(axis=0)
        self.Wm = (self.X * W).sum(axis=0)
        self.bm = (self.X * self.q["b"][:, None]).sum(axis=0)
        self.c0 = self.X * self.q["sqa"][:, None]
        self.nasa = _c(dt, t.nasa)
        self.rw = dt(R_GAS) / _c(dt, t.W)[:, None]

    def hcp_ig(self, T):
        nasa = self.nasa
        up = T[None, :] > nasa[:, 0][:, None]
        a = np.where(up[:, :, None], nasa[:, None, 1:8], nasa[:, None, 8:15])
        T2 = T * T; T3 = T2 * T; T4 = T3 * T
        cpR = a[..., 0] + a[..., 1] * T + a[..., 2] * T2 + a[..., 3] * T3 + a[..., 4] * T4
        hRT = a[..., 0] + a[..., 1] * T / 2 + a[..., 2] * T2 / 3 + a[..., 3] * T3 / 4 + a[..., 4] * T4 / 5 + a[..., 5] / T
        return (self.Y * hRT * T * self.rw).sum(axis=0), (self.Y * cpR * self.rw).sum(axis=0)

    def attraction(self, T):
        """(a alpha), its first and second T derivative"""
        dt = self.dt
        sT = np.sqrt(T)
        kap = self.q["kap"][:, None]; rs = self.q["rsTc"][:, None]
        s = 1 + kap * (1 - sT[None, :] * rs)
        sg = np.where(s < 0, dt(-1), dt(1))
        A0 = (self.c0 * np.abs(s)).sum(axis=0)
        Q = (self.c0 * sg * kap * rs).sum(axis=0)
        A1 = -Q / (2 * sT)
        A2 = Q / (4 * T * sT)
        return A0 * A0, 2 * A0 * A1, 2 * (A1 * A1 + A0 * A2)


def _polish(z, a2, a1, a0, dt, steps=30):
    eps = np.finfo(dt).eps
    z = z.copy()
    prev = np.full(z.shape, np.inf, dtype=dt)
    done = np.zeros(z.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            f = ((z + a2) * z + a1) * z + a0
            fp = (3 * z + 2 * a2) * z + a1
            done = done | (fp == 0)
            dz = np.where(done, dt(0), f / np.where(fp == 0, dt(1), fp))
            a = np.abs(dz)
            done = done | ((a >= prev) & (prev <= dt(1e-9) * np.abs(z)))
            z = np.where(done, z, z - dz)
            prev = np.where(done, prev, a)
            done = done | (a <= 4 * eps * np.abs(z))
            if done.all():
                break
    return z


def lnphi(z, A, B, dt):
    sq2 = np.sqrt(dt(2))
    with np.errstate(all="ignore"):
        return z - 1 - np.log(z - B) - A / (2 * sq2 * B) * np.log1p(2 * sq2 * B / (z + (1 - sq2) * B))


def cubic(A, B, dt):
    """the compressibility factor chosen per state, and what a test wants to know about the roots: three (the
    trigonometric branch was taken), zmin / zmid / zmax, n_adm (roots above B), dlnphi (smallest minus largest root's,
    nan unless both are admissible)"""
    pi = 4 * np.arctan(dt(1))
    a2 = -(1 - B); a1 = A - 3 * B * B - 2 * B; a0 = -(A * B - B * B - B * B * B)
    sh = -a2 / 3
    pp = a1 - a2 * a2 / 3
    qq = 2 * a2 * a2 * a2 / 27 - a2 * a1 / 3 + a0
    D = qq * qq / 4 + pp * pp * pp / 27
    three = ~(D > 0)
    with np.errstate(all="ignore"):
        sD = np.sqrt(np.where(three, dt(0), D))
        u = np.where(qq > 0, dt(-1), dt(1)) * np.cbrt(np.abs(qq) / 2 + sD)
        z1 = np.where(u == 0, dt(0), u - pp / (3 * np.where(u == 0, dt(1), u))) + sh
        r = 2 * np.sqrt(np.maximum(-pp / 3, dt(0)))
        den = pp * r
        arg = np.clip(np.where(den == 0, dt(0), 3 * qq / np.where(den == 0, dt(1), den)), dt(-1), dt(1))
        th = np.arccos(arg) / 3
        zmax = r * np.cos(th) + sh
        zmid = r * np.cos(th - 2 * pi / 3) + sh
        zmin = r * np.cos(th - 4 * pi / 3) + sh
    zmax = _polish(np.where(three, zmax, z1), a2, a1, a0, dt)
    zmin = _polish(np.where(three, zmin, z1), a2, a1, a0, dt)
    zmid = _polish(np.where(three, zmid, z1), a2, a1, a0, dt)
    lmax = lnphi(zmax, A, B, dt)
    lmin = lnphi(zmin, A, B, dt)
    both = three & (zmin > B)
    with np.errstate(invalid="ignore"):
        low = both & (lmin < lmax)
    Z = np.where(low, zmin, zmax)
    n_adm = np.where(three, (zmin > B).astype(int) + (zmid > B).astype(int) + (zmax > B).astype(int), 1)
    return Z, {"three": three, "zmin": zmin, "zmid": zmid, "zmax": zmax, "n_adm": n_adm, "low": low,
               "dlnphi": np.where(both, lmin - lmax, dt(np.nan)),
               "lmid": np.where(three & (zmid > B), lnphi(zmid, A, B, dt), dt(np.inf)), "lbest": np.where(low, lmin, lmax),
               "coef": (a2, a1, a0)}


def state_at(mx: Mix, T, p, want_roots=False):
    """rho, h, cp, Z (and the cubic's diagnostics) at T, p"""
    dt = mx.dt
    sq2 = np.sqrt(dt(2))
    Rg = dt(R_GAS)
    h_ig, cp_ig = mx.hcp_ig(T)
    aal, d1, d2 = mx.attraction(T)
    RT = Rg * T
    bm = mx.bm
    A = aal * p / (RT * RT); B = bm * p / RT
    Z, info = cubic(A, B, dt)
    v = Z * RT / p
    L = np.log1p(2 * sq2 * B / (Z + (1 - sq2) * B))
    k = 1 / (2 * sq2 * bm)
    h = h_ig + (RT * (Z - 1) + (T * d1 - aal) * k * L) / mx.Wm
    vb = v - bm; den = v * v + 2 * bm * v - bm * bm
    pT = Rg / vb - d1 / den
    pv = -RT / (vb * vb) + aal * (2 * v + 2 * bm) / (den * den)
    cp = cp_ig + (-Rg + T * d2 * k * L - T * pT * pT / pv) / mx.Wm
    out = {"rho": p * mx.Wm / (Z * RT), "h": h, "cp": cp, "Z": Z, "cp_ig": cp_ig, "A": A, "B": B, "aal": aal}
    if want_roots:
        out["roots"] = info
    return out


def solve_T(mx: Mix, he, p, T0, steps=None):
    dt = mx.dt
    eps = np.finfo(dt).eps
    steps = steps or (40 if dt is F64 else 200)
    tt = _c(dt, T0).copy()
    prev = np.full(tt.shape, np.inf, dtype=dt)
    done = np.zeros(tt.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            st = state_at(mx, tt, p)
            dT = (st["h"] - he) / st["cp"]
            a = np.abs(dT)
            done = done | ((a >= prev) & (prev <= dt(1e-9) * tt))
            tt = np.where(done, tt, tt - dT)
            prev = np.where(done, prev, a)
            done = done | (a <= 4 * eps * np.abs(tt))
            if done.all():
                break
    return tt, done


def point(t, eos, p, Y, T=None, he=None, T0=None, dtype=LD, dx=DX):
    """One real-fluid thermo point per column of Y, from T (he returned) or from he with the start T0 (T returned).
    dtype long double: the reference; float64: the restatement the kernels port. Returns T, he, psi, rho, mu, alpha,
    cp, Z [n], rhoD, hai [S, n], the conditioning data of thermo_reference (X, Wm, kappa), and `roots` at (T, p)."""
    dt = dtype
    mx = Mix(t, eos, Y, dt)
    p = _c(dt, p)
    if T is None:
        he = _c(dt, he)
        T, conv = solve_T(mx, he, p, T0)
    else:
        T = _c(dt, T)
        conv = np.ones(T.shape, dtype=bool)
        he = state_at(mx, T, p)["h"]
    st = state_at(mx, T, p, want_roots=True)
    p2 = p * (1 - dt(dx))
    T2, conv2 = solve_T(mx, he, p2, T)
    st2 = state_at(mx, T2, p2)
    psi = (st["rho"] - st2["rho"]) / (dt(dx) * p)
    if dt is F64:
        import oracle as O
        ig = O.thermo_points(t, T, np.zeros(T.size), p, np.asarray(Y, dtype=F64), True)
        ig = {k: ig[k] for k in ("mu", "alpha", "rhoD", "hai", "psi")}
    else:
        ig = R.evaluate(t, p, Y, T=T)
    cond = ig["alpha"] * st["cp_ig"]
    out = {"T": T, "he": he, "psi": psi, "rho": st["rho"], "mu": ig["mu"], "alpha": cond / st["cp"],
           "rhoD": ig["rhoD"] / ig["psi"][None, :] * (st["rho"] / p)[None, :], "hai": ig["hai"], "cp": st["cp"], "Z": st["Z"],
           "roots": st["roots"], "converged": conv & conv2, "T2": T2, "X": mx.X, "Wm": mx.Wm}
    with np.errstate(divide="ignore", invalid="ignore"):
        den = mx.Wm[None, :] - mx.X * _c(dt, t.W)[:, None]
        out["kappa"] = np.where(den > 0, mx.Wm[None, :] / den, dt(np.inf))
    return out


def psi_analytic(t, eos, p, Y, T, dtype=LD):
    """(d rho / d p)_h from the derivatives of rho(T, p) and h(T, p), themselves central differences of the long-double
    model extrapolated once (Richardson): what the quotient approximates to first order in dx"""
    dt = dtype
    mx = Mix(t, eos, Y, dt)
    p = _c(dt, p); T = _c(dt, T)

    def d(fn, x, rel):
        hh = x * dt(rel)
        c1 = (fn(x + hh) - fn(x - hh)) / (2 * hh)
        c2 = (fn(x + hh / 2) - fn(x - hh / 2)) / hh
        return (4 * c2 - c1) / 3

    rT = d(lambda x: state_at(mx, x, p)["rho"], T, 1e-5); rp = d(lambda x: state_at(mx, T, x)["rho"], p, 1e-5)
    hT = d(lambda x: state_at(mx, x, p)["h"], T, 1e-5); hp = d(lambda x: state_at(mx, T, x)["h"], p, 1e-5)
    return rp - rT * hp / hT


def critical_point(t, eos, Y):
    """(Tc, pc) of each mixture treated as one fluid: (a alpha)(Tc) = (Omega_a / Omega_b) R Tc b, pc = Omega_b R Tc / b"""
    mx = Mix(t, eos, Y, F64)
    lo = np.full(mx.bm.shape, 1.0); hi = np.full(mx.bm.shape, 5000.0)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        f = mx.attraction(mid)[0] - (OMEGA_A / OMEGA_B) * R_GAS * mid * mx.bm
        lo = np.where(f > 0, mid, lo); hi = np.where(f > 0, hi, mid)
    Tc = 0.5 * (lo + hi)
    return Tc, OMEGA_B * R_GAS * Tc / mx.bm


# ------------------------------------------------------------------------------------------------ states
class States(R.States):
    pass


def _gamma_Y(rng, S, n):
    Y = np.maximum(rng.gamma(0.3, 1.0, (S, n)), 1e-300)
    return Y / Y.sum(axis=0)


def _rich_Y(rng, S, n, rich):
    """each column dominated (X about 0.9 to 0.999) by one species of `rich`"""
    Y = _gamma_Y(rng, S, n) * 10.0 ** rng.uniform(-3.0, -1.0, n)[None, :]
    i = rng.choice(np.asarray(rich), n)
    Y[i, np.arange(n)] = 1.0
    return Y / Y.sum(axis=0), i


def _rich_species(name, S):
    if name == "bfer6":
        sp = load_fixture()["species"]
        return [sp.index(s) for s in ("O2", "CH4", "N2")]
    return list(range(S))


def _draw(name, cls, seed, n):
    t, eos = table(name)
    S = t.S
    rng = np.random.default_rng([seed, S, CLASSES.index(cls)])
    q = species_params(eos)
    from_T = cls != "newton"
    he = None
    if cls in ("supercritical", "zeros"):
        T = rng.uniform(120.0 if name == "bfer6" else 200.0, 3000.0, n)
        p = np.exp(rng.uniform(np.log(5e6), np.log(30e6), n))
        Y = _gamma_Y(rng, S, n)
        if cls == "zeros":
            for k in range(n):
                Y[rng.permutation(S)[: S // 2], k] = 0.0
            Y = Y / Y.sum(axis=0)
    elif cls == "pure":
        cols = [np.eye(S)[:, i] for i in range(S)] * 3
        pairs = sorted({(min(a, b), max(a, b)) for a, b in ((0, 1), (0, S - 1), (S // 2, S - 1)) if a != b})
        for i, j in pairs:
            for f in (0.5, 0.1, 0.9):
                y = np.zeros(S); y[i] = f; y[j] = 1.0 - f
                cols.append(y)
        Y = np.stack(cols, axis=1)
        m = Y.shape[1]
        Tc, pc = critical_point(t, eos, Y)
        T = Tc * rng.uniform(1.05, 8.0, m)          # above the one-fluid critical temperature: one phase
        p = np.exp(rng.uniform(np.log(5e6), np.log(30e6), m))
    elif cls == "dense":
        Y, i = _rich_Y(rng, S, n, _rich_species(name, S))
        T = q["Tc"][i] * rng.uniform(0.66, 0.84, n)
        if name == "bfer6":
            T = np.clip(T, 100.0, 200.0)
            p = np.full(n, 1.0e7)
        else:   # drawn critical pressures (2-8 MPa): the same reduced pressures as the three species at 10 MPa
            p = OMEGA_B * R_GAS * q["Tc"][i] / q["b"][i] * rng.uniform(2.0, 2.9, n)
    elif cls == "near_critical":
        Y = _gamma_Y(rng, S, n)
        Tc, pc = critical_point(t, eos, Y)
        T = Tc * (1 + rng.choice([1e-2, 1e-3], n))
        p = pc * rng.choice([1.05, 1.5], n)
    elif cls == "three_root":
        Y, i = _rich_Y(rng, S, n, list(range(S)))
        Y = Y * 0 + 5e-4 / (S - 1); Y[i, np.arange(n)] = 1.0 - 5e-4; Y = Y / Y.sum(axis=0)
        Tr = rng.uniform(0.7, 0.9, n)
        T = q["Tc"][i] * Tr
        pc_i = OMEGA_B * R_GAS * q["Tc"][i] / q["b"][i]
        psat = pc_i * 10.0 ** ((7.0 / 3.0) * (1 + np.asarray(eos["w"])[i]) * (1 - 1 / Tr))
        p = psat * np.exp(rng.uniform(-0.12, 0.12, n))
    elif cls == "dilute":
        T = rng.uniform(200.0, 3000.0, n)
        p = np.exp(rng.uniform(np.log(1e2), np.log(1e5), n))
        Y = _gamma_Y(rng, S, n)
    elif cls == "newton":
        nb = n // 4
        Yb = _gamma_Y(rng, S, nb)
        Tc, pc = critical_point(t, eos, Yb)
        pb = pc * rng.uniform(1.2, 3.0, nb)          # above the one-fluid critical pressure: h(T) is smooth along the isobar
        Ts = rng.uniform(np.maximum(1.1 * Tc, 250.0), 3000.0)
        heb = np.asarray(point(t, eos, pb, Yb, T=Ts)["he"], dtype=F64)
        starts = [0.9 * Ts, 1.1 * Ts, np.full(nb, 300.0), np.full(nb, 3000.0)]
        T = np.concatenate(starts); he = np.tile(heb, 4); p = np.tile(pb, 4); Y = np.tile(Yb, (1, 4))
    else:
        raise KeyError(cls)
    return t, eos, States(cls, from_T, T, np.zeros(T.size) if he is None else he, p, Y)


_state_cache: dict = {}


def states(name, cls, seed=0, n=240):
    """(States, reference, dropped fraction) of one class on one table: the drawn states, less those that miss the
    class's own condition (module constants; at most MAX_DROP of the draw, asserted), and the long-double reference"""
    key = (name, cls, seed, n)
    if key in _state_cache:
        return _state_cache[key]
    t, eos, st = _draw(name, cls, seed, n)
    ref = point(t, eos, st.p, st.Y, T=st.T if st.from_T else None, he=None if st.from_T else st.he,
                T0=None if st.from_T else st.T)
    Tf = np.asarray(ref["T"], dtype=F64)
    rt = ref["roots"]
    keep = np.asarray(ref["converged"]).copy()
    kinks = kink_temperatures(eos)
    for Tx in (Tf, np.asarray(ref["T2"], dtype=F64)):
        keep &= (np.abs(Tx[:, None] - kinks[None, :]) >= KINK_MARGIN * Tx[:, None]).all(axis=1)
    dl = np.asarray(rt["dlnphi"], dtype=F64)
    n_adm = np.asarray(rt["n_adm"])
    if cls == "three_root":
        keep &= (n_adm == 3) & (np.abs(dl) >= DLNPHI_MIN)
    else:
        keep &= ~((n_adm == 3) & (np.abs(dl) < DLNPHI_MIN))      # two roundings must not disagree about the phase
    Z = np.asarray(ref["Z"], dtype=F64)
    if cls == "dense":
        keep &= (Z >= 0.2) & (Z <= 0.5)
    if cls == "near_critical":
        keep &= ~np.asarray(rt["three"])
    if cls == "dilute":
        keep &= ~np.asarray(rt["low"])      # the gas: the virial bound of the CPU test is about that root
    if cls == "newton":
        keep &= np.abs(np.asarray(ref["he"] - R._ld(st.he), dtype=F64)) <= 1e-30      # he is the input
    drop = 1.0 - keep.mean()
    assert drop <= MAX_DROP, f"{name}/{cls}: {drop:.1%} of the drawn states miss the class condition"
    k = np.where(keep)[0]
    st = States(cls, st.from_T, st.T[k], st.he[k], st.p[k], np.ascontiguousarray(st.Y[:, k]))
    sub = {}
    for q_, v in ref.items():
        if q_ == "roots":
            sub[q_] = {a: (b[k] if isinstance(b, np.ndarray) else b) for a, b in v.items() if a != "coef"}
        else:
            sub[q_] = v[..., k]
    R._check_cut_margin(t, st.Y)
    _state_cache[key] = (st, sub, drop)
    return _state_cache[key]


def restatement(name, st):
    t, eos = table(name)
    return point(t, eos, st.p, st.Y, T=st.T if st.from_T else None, he=None if st.from_T else st.he,
                 T0=None if st.from_T else st.T, dtype=F64)


# ------------------------------------------------------------------------------------------------ bounds
def errors(t, got, ref):
    """thermo_reference.errors (per element; rho_thermo is judged as rho)"""
    return R.errors(t, got, ref)


def measure():
    out = {}
    for name in TABLES:
        t, _ = table(name)
        out[name] = {}
        for cls in CLASSES:
            st, ref, drop = states(name, cls)
            got = restatement(name, st)
            e = errors(t, {q: np.asarray(got[q], dtype=F64) for q in ("T", "he", "psi", "rho", "mu", "alpha", "rhoD", "hai")}, ref)
            out[name][cls] = dict(R.maxima(cls, e, ref), states=int(st.n), dropped=round(float(drop), 4))
    return out


def class_maxima(per_table):
    return {cls: {q: max(per_table[n][cls][q] for n in per_table) for q in QUANTITIES} for cls in CLASSES}


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def gpu_bound(bounds, cls, q):
    """4x the float64 restatement's measured maximum, floored at 1e-13; psi carries its own measured bound
    like every other quantity: the quotient's amplification by 1 / dx is in the measurement"""
    b = 4.0 * bounds["classes"][cls][q]
    return b if q in ("rhoD_kappa", "rhoD_dominant") else max(b, 1e-13)


def rhoD_bounds(bounds, cls, kappa):
    k = np.asarray(kappa, dtype=F64)
    with np.errstate(invalid="ignore", over="ignore"):
        kb = np.maximum(gpu_bound(bounds, cls, "rhoD_kappa") * k * R.EPS, 1e-13)
    return np.where(k > 10, kb, gpu_bound(bounds, cls, "rhoD"))


# ------------------------------------------------------------------------------------------------ oracle
def _oracle_base():
    import oracle as O
    return O.Oracle


class _StopAtThermo(Exception):
    pass


class RealFluidOracle(_oracle_base()):
    """The sequential oracle with the real-fluid thermo: thermo_correct is the float64 restatement over cells and
    slots (fixedValue-T slots from T, others from he, processor [internal n] slots copy cells), time_step keeps
    OpenFOAM's thermo.rho_ as rho_thermo (pEqn.H:1-4, 8, 95; dfLowMachFoam.C:517)."""

    def __init__(self, mesh, table_, eos, state, ptypes, inert, rdt, schemes=None, psi_dtype=F64):
        super().__init__(mesh, table_, state, ptypes, inert, rdt, schemes)
        self.table = table_
        self.eos = eos
        self.psi_dtype = psi_dtype
        self._stop_at_thermo = False
        if "rho_thermo" not in self.arr:
            self._d("rho_thermo", self.arr["rho"].copy())
            self._d("boundary_rho_thermo", self.arr["boundary_rho"].copy())

    def _points(self, T, he, p, Y, fixT):
        """the float64 restatement at n states, from T where fixT and from he (start T) elsewhere"""
        n = T.size
        out = {q: np.zeros((self.S, n) if q in ("rhoD", "hai") else n) for q in ("T", "he", "psi", "rho", "mu", "alpha", "rhoD", "hai")}
        for flag in (True, False):
            k = np.where(fixT == flag)[0]
            if not k.size:
                continue
            kw = {"T": T[k]} if flag else {"he": he[k], "T0": T[k]}
            r = point(self.table, self.eos, p[k], Y[:, k], dtype=F64, **kw)
            if self.psi_dtype is not F64:
                r["psi"] = point(self.table, self.eos, p[k], Y[:, k], dtype=self.psi_dtype, **kw)["psi"]
            for q in out:
                out[q][..., k] = np.asarray(r[q], dtype=F64)
        return out

    def thermo_correct(self, from_T=False):
        if self._stop_at_thermo:
            raise _StopAtThermo()
        from dfmi.mesh import EMPTY, FIXED_VALUE
        m = self.m
        a = self.arr
        C_, B, S = m.n_cells, m.n_boundary_slots, self.S
        cells = self._points(a["T"], a["he"], a["p"], a["Y"].reshape(S, C_), np.full(C_, bool(from_T)))
        for q, v in cells.items():
            a[q].reshape(v.shape)[...] = v
        a["rho_thermo"][...] = cells["rho"]
        if not B:
            return
        ty = np.repeat(np.asarray(self.ptypes["T"]), [p.slots for p in m.patches])
        prim = np.concatenate([np.arange(p.slots) < p.size for p in m.patches])
        proc = np.repeat(self._kind == 2, [p.slots for p in m.patches])
        bfc = np.concatenate([np.tile(p.face_cells, p.slots // max(p.size, 1)) for p in m.patches])
        names = ("T", "he", "psi", "rho", "mu", "alpha", "rhoD", "hai")
        inner = np.where(proc & ~prim)[0]          # processor [internal n] slots copy their cells
        for q in names + ("rho_thermo",):
            src = a[q].reshape(-1, C_)
            a["boundary_" + q].reshape(-1, B)[:, inner] = src[:, bfc[inner]]
        idx = np.where((ty != EMPTY) & ~(proc & ~prim))[0]
        fix = (ty == FIXED_VALUE) | bool(from_T)
        sl = self._points(a["boundary_T"][idx], a["boundary_he"][idx], a["boundary_p"][idx],
                          a["boundary_Y"].reshape(S, B)[:, idx], fix[idx])
        for q, v in sl.items():
            a["boundary_" + q].reshape(-1, B)[:, idx] = v.reshape(-1, idx.size)
        a["boundary_rho_thermo"][idx] = sl["rho"]

    def time_step(self, n_corr=2):
        a = self.arr
        # the inherited step up to its correctThermo, then the CPU solver's corrector sequence
        self._stop_at_thermo = True
        try:
            super().time_step(n_corr)
            raise AssertionError("the inherited step did not reach correctThermo")
        except _StopAtThermo:
            pass
        finally:
            self._stop_at_thermo = False
        self.thermo_correct(False)
        for _ in range(n_corr):
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
        for pre in ("", "boundary_"):
            a[pre + "rho"][...] = a[pre + "rho_thermo"]


def flow_fields(m, species, L):
    """10 MPa, 150-600 K, a CH4 / O2 / N2 mixture that varies over the box, the Taylor-Green velocity"""
    cc = m.cell_centres / L
    x, y, z = cc[:, 0], cc[:, 1], cc[:, 2]
    u0 = 4.0
    U = np.stack([u0 * np.sin(x) * np.cos(y) * np.cos(z), -u0 * np.cos(x) * np.sin(y) * np.cos(z), np.zeros_like(x)])
    T = 375.0 + 225.0 * np.sin(x + 0.3) * np.cos(y - 0.2) * np.cos(0.5 * z)
    Y = np.zeros((len(species), m.n_cells))
    f = 0.5 + 0.4 * np.cos(x) * np.sin(y + 0.4)
    Y[species.index("CH4")] = 0.3 * f
    Y[species.index("O2")] = 0.4 * (1 - f) + 0.05
    Y[species.index("CO2")] = 0.02 + 0.01 * np.sin(z)
    Y[species.index("H2O")] = 0.01
    Y[species.index("CO")] = 0.005
    Y[species.index("N2")] = 1.0 - Y.sum(axis=0)
    assert Y.min() > 0 and T.min() >= 150.0 and T.max() <= 600.0
    return {"T": T, "p": np.full(m.n_cells, 1.0e7), "U": U, "Y": Y}


def cpu_state(m, t, eos, ptypes, inert, rdt, f, wall_T=None, cls=None):
    """An oracle holding the initial state dfmi.case.init_state would leave, formed on the CPU: boundary values by the
    patch rules, the thermo from T by the oracle's own thermo_correct, phi = interpolate(rho U) . Sf, K.
    wall_T = {patch: T} sets fixedValue temperatures; cls: the oracle class (default RealFluidOracle)."""
    from dfmi import case
    C_, F, B, S = m.n_cells, m.n_faces, m.n_boundary_slots, t.S
    st = {}
    for n in case.SCALARS:
        st[n] = np.zeros(C_); st["boundary_" + n] = np.zeros(B)
    for n in case.VECTORS:
        st[n] = np.zeros((3, C_)); st["boundary_" + n] = np.zeros((3, B))
    for n in case.SPECIES:
        st[n] = np.zeros((S, C_)); st["boundary_" + n] = np.zeros((S, B))
    for n in case.FACES:
        st[n] = np.zeros(F); st["boundary_" + n] = np.zeros(B)
    for n, k in case.BOUNDARY_ONLY.items():
        k = S if k == "S" else k
        st[n] = np.zeros((k, B) if k > 1 else B)
    for n in ("T", "p", "U", "Y"):
        st[n] = np.array(f[n], dtype=F64)
        st["boundary_" + n] = case.boundary_values(m, st[n])
    for patch, v in (wall_T or {}).items():
        st["boundary_T"][case.patch_slots(m, patch)] = v
    st["he"][...] = 1.0; st["boundary_he"][...] = 1.0      # overwritten from T
    if cls is None:
        o = RealFluidOracle(m, t, eos, st, ptypes, inert, rdt)
    else:
        o = cls(m, t, st, ptypes, inert, rdt)
    o.thermo_correct(True)
    a = o.arr
    phi, bphi = case.face_flux(m, a["rho"], a["U"], a["boundary_rho"], a["boundary_U"])
    a["phi"][...] = phi; a["boundary_phi"][...] = bphi
    a["K"][...] = 0.5 * (a["U"] * a["U"]).sum(axis=0)
    a["boundary_K"][...] = 0.5 * (a["boundary_U"] * a["boundary_U"]).sum(axis=0)
    return o


if __name__ == "__main__":
    if "--measure" not in sys.argv:
        sys.exit("usage: realfluid_reference.py --measure")
    per_table = measure()
    doc = {"about": "max error of the float64 restatement of the Peng-Robinson thermo point against the long-double one "
                    "(tests/realfluid_reference.py), per state class and quantity, errors as thermo_reference.errors; "
                    "written by tests/realfluid_reference.py --measure",
           "classes": class_maxima(per_table), "tables": per_table}
    with open(BOUNDS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for cls, v in doc["classes"].items():
        print(cls, {q: f"{x:.2e}" for q, x in v.items()})
