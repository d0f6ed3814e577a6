"""Extended-precision point reference of the thermo / transport update, and the states the
thermo kernels are tested at.

One thermo point, restated from the formulas in NumPy longdouble (x87 extended: 64-bit mantissa), vectorised over
n states. With Y [S, n], the table's W, NASA7 blocks [T_mid, hi a0..a6, lo a0..a6] and the fits in ln T:

    X_i   = (Y_i / W_i) / sum_j (Y_j / W_j)            Wm = sum_i X_i W_i
    h_i   = (R T / W_i) (a0 + a1 T/2 + a2 T^2/3 + a3 T^3/4 + a4 T^4/5 + a5 / T)     range hi iff T > T_mid_i (strict)
    cp_i  = (R / W_i) (a0 + a1 T + a2 T^2 + a3 T^3 + a4 T^4)
    he    = sum_i Y_i h_i     cp = sum_i Y_i cp_i     psi = Wm / (R T)     rho = p psi
    mu_i  = sqrt(T) (visc_i . L)^2,  L = (1, ln T, ln^2 T, ln^3 T, ln^4 T)
    mu    = sum_i X_i mu_i / sum_j X_j Phi_ij,   Phi_ij = (1 + sqrt(mu_i / mu_j) (W_j / W_i)^(1/4))^2 / sqrt(8 (1 + W_i / W_j))
    lam_i = sqrt(T) (cond_i . L)        alpha = (sum_i X_i lam_i + 1 / sum_i (X_i / lam_i)) / (2 cp)
    p D_ij = T^1.5 (bdiff_ij . L)
    rhoD_i = (rho / p) / (sum_{j != i} X_j / (p D_ij) + X_i / (Wm - X_i W_i) sum_{j != i} X_j W_j / (p D_ij)),
             0 where X_i + 1e-10 > 1
    hai_i = h_i(T)

From he, T solves he = sum_i Y_i h_i(T) to convergence in long double by Newton steps kept inside a bisection
bracket (h(T) is piecewise: the NASA fits jump at T_mid, so a plain Newton iteration can cycle there).

Beside the outputs the reference returns kappa_i = Wm / (Wm - X_i W_i), the conditioning of rhoD_i (the
denominator cancels as X_i -> 1), and the mixture's h just below and just above every distinct T_mid of the table,
so a test can tell whether a target he lies inside a jump, where no T solves it.

`python tests/thermo_reference.py --measure` evaluates the fp64 sequential oracle (oracle.thermo_points) against
this reference on every state class and writes the maxima to tests/golden/thermo_point_bounds.json; the GPU
tolerances are derived from that file (gpu_bound), never from a kernel's output.
"""
from __future__ import annotations

import json
import os
import sys
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
R_GAS = 8314.46261815324
EPS = 2.0 ** -52
ATM = 101325.0
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUNDS_PATH = os.path.join(GOLDEN, "thermo_point_bounds.json")
CUT = 1e-10            # rhoD_i = 0 where X_i + CUT > 1
CUT_MARGIN = 1e-13     # no test state has an X_i closer than this to 1 - CUT
JUMP_ZONE = 4e-6       # |T - T_mid| <= JUMP_ZONE T_mid: T(he) is not compared (4x the largest measured jump)
JUMP_STOP = 8e-6       # where the iteration may end, as a fraction of T_mid
QUANTITIES = ("T", "he", "psi", "rho", "mu", "alpha", "rhoD", "rhoD_kappa", "rhoD_dominant", "hai")
CLASSES = ("broad", "zeros", "pure", "near_pure", "switch_T", "newton", "jump")


# ------------------------------------------------------------------------------------------------ tables
def _dfmi_path():
    for p in (os.path.join(os.path.dirname(HERE), "deepflame-dev_amd"), os.path.join(os.path.dirname(HERE), "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)


_cache: dict = {}


def mech_table(name):
    """the committed ES80 (S = 7) or Burke (S = 9) table"""
    _dfmi_path()
    from dfmi.mech import read_thermo_table
    if name not in _cache:
        f = {"es80": "thermo_ES80_H2-7-16.txt", "burke9": "thermo_Burke2012_s9r23.txt",
             "gri53": "thermo_gri53_synthetic.txt"}[name]
        _cache[name] = read_thermo_table(os.path.join(GOLDEN, f))
    return _cache[name]


def gri_table(S):
    """a table of any S in 2..64 from the synthetic 53-species one: its first S - 1 rows and N2 (its last row) last;
    past 53 the 52 non-inert rows are cycled again, a species and its copy using the species' self-diffusion fit
    (what dfmi.synthetic does to reach 53 from 36)"""
    _dfmi_path()
    from dfmi.mech import ThermoTable
    assert 2 <= S <= 64
    g = mech_table("gri53")
    idx = np.array([k % 52 for k in range(S - 1)] + [52])
    return ThermoTable([f"s{k}" for k in range(S)], g.W[idx].copy(), g.nasa[idx].copy(), g.visc[idx].copy(),
                       g.cond[idx].copy(), g.bdiff[np.ix_(idx, idx)].copy())


def is_symmetric(t):
    return bool(np.array_equal(t.bdiff, t.bdiff.transpose(1, 0, 2)))


def nonsymmetric(t):
    """the table with bdiff[i][j] of a handful of ordered pairs scaled by 1.01 and [j][i] left alone"""
    _dfmi_path()
    from dfmi.mech import ThermoTable
    S = t.S
    assert S >= 3
    pairs, seen = [], set()
    for i, j in ((0, 1), (2, 0), (1, S - 1), (S - 1, S - 2), (S // 2, 0)):
        if i != j and frozenset((i, j)) not in seen:
            seen.add(frozenset((i, j)))
            pairs.append((i, j))
    bd = t.bdiff.copy()
    for i, j in pairs:
        bd[i, j] *= 1.01
    out = ThermoTable(list(t.species), t.W.copy(), t.nasa.copy(), t.visc.copy(), t.cond.copy(), bd)
    assert not is_symmetric(out)
    return out


def distinct_tmid(t):
    return np.unique(np.asarray(t.nasa[:, 0], dtype=np.float64))


def switching_tmid(t):
    """the distinct T_mid at which some species really changes its NASA block. A species fitted with one range
    carries the same block twice and the end of its range as T_mid (AR in the GRI table: 5000 K): nothing switches
    there, and that far above the other species' fits (they end at 3500 K) the extrapolated mixture h(T) turns over
    near 7000 K, so he = h(T) has a second root (near 8700 K for T* = 5000 K) which a Newton iteration started at
    300 K reaches first. T(he) has no single value there; the classes that solve for T use the real switches."""
    real = [i for i in range(t.S) if not np.array_equal(t.nasa[i, 1:8], t.nasa[i, 8:15])]
    return np.unique(np.asarray(t.nasa[real, 0], dtype=np.float64))


# ------------------------------------------------------------------------------------------------ the reference
def _ld(a):
    return np.asarray(a, dtype=LD)


def composition(t, Y):
    """X [S, n], Wm [n]"""
    W = _ld(t.W)[:, None]
    yw = _ld(Y) / W
    X = yw / yw.sum(axis=0)
    return X, (X * W).sum(axis=0)


def species_h_cp(t, T, up=None):
    """h_i [S, n] (J/kg) and cp_i [S, n] at T [n]; up [S, n] overrides the range choice T > T_mid_i"""
    T = _ld(T)
    nasa = _ld(t.nasa)
    if up is None:
        up = T[None, :] > nasa[:, 0][:, None]
    a = np.where(np.asarray(up)[:, :, None], nasa[:, None, 1:8], nasa[:, None, 8:15])
    T2 = T * T; T3 = T2 * T; T4 = T3 * T
    cpR = a[..., 0] + a[..., 1] * T + a[..., 2] * T2 + a[..., 3] * T3 + a[..., 4] * T4
    hRT = a[..., 0] + a[..., 1] * T / 2 + a[..., 2] * T2 / 3 + a[..., 3] * T3 / 4 + a[..., 4] * T4 / 5 + a[..., 5] / T
    rw = LD(R_GAS) / _ld(t.W)[:, None]
    return hRT * T * rw, cpR * rw


def mixture_h_cp(t, T, Y, up=None):
    h, cp = species_h_cp(t, T, up)
    Y = _ld(Y)
    return (Y * h).sum(axis=0), (Y * cp).sum(axis=0)


def one_sided_h(t, Y):
    """(T_mid [m], h_below [m, n], h_above [m, n]): the mixture's h at each distinct T_mid with the species switching
    there on their low / on their high range"""
    tms = distinct_tmid(t)
    n = np.shape(Y)[1]
    tmid = np.asarray(t.nasa[:, 0])[:, None]
    lo, hi = [], []
    for tm in tms:
        T = np.full(n, tm, dtype=LD)
        lo.append(mixture_h_cp(t, T, Y, np.broadcast_to(tmid < tm, (t.S, n)))[0])
        hi.append(mixture_h_cp(t, T, Y, np.broadcast_to(tmid <= tm, (t.S, n)))[0])
    return tms, np.array(lo), np.array(hi)


def solve_T(t, Y, he, T0, bracket=(100.0, 6000.0)):
    """T [n] with mixture h(T) = he, to convergence in long double: Newton steps from T0, replaced by a bisection
    step whenever one leaves the bracket that the signs of h - he seen so far define"""
    he = _ld(he)
    n = he.shape[0]
    lo = np.full(n, bracket[0], dtype=LD); hi = np.full(n, bracket[1], dtype=LD)
    flo = mixture_h_cp(t, lo, Y)[0] - he
    fhi = mixture_h_cp(t, hi, Y)[0] - he
    assert np.all(flo < 0) and np.all(fhi > 0), "target enthalpy outside the bracket"
    T = np.clip(_ld(T0), lo * LD(1.001), hi * LD(0.999))
    tol = LD(4) * np.finfo(LD).eps
    done = np.zeros(n, dtype=bool)
    for _ in range(300):
        h, cp = mixture_h_cp(t, T, Y)
        f = h - he
        lo = np.where(f < 0, np.maximum(lo, T), lo)
        hi = np.where(f > 0, np.minimum(hi, T), hi)
        Tn = T - f / cp
        out = ~((Tn > lo) & (Tn < hi))
        Tn = np.where(out, (lo + hi) / 2, Tn)
        Tn = np.where(f == 0, T, Tn)
        done = done | (np.abs(Tn - T) <= tol * T) | (hi - lo <= tol * T)
        T = np.where(done, T, Tn)
        if done.all():
            break
    assert done.all(), "T(he) did not converge"
    return T


def newton_limit(t, Y, he, T0, steps=200):
    """where the plain Newton iteration T <- T - (h(T) - he) / cp(T) started at T0 ends when it is carried to
    convergence in long double: (T [n], converged [n])"""
    he = _ld(he)
    T = _ld(T0).copy()
    conv = np.zeros(T.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            h, cp = mixture_h_cp(t, T, Y)
            Tn = T - (h - he) / cp
            T = np.where(conv, T, Tn)       # a last step of under 1e-16 T is still taken: the limit to rounding
            conv = conv | (np.abs((h - he) / cp) <= LD(1e-16) * np.abs(T))
    return T, conv


def evaluate(t, p, Y, T=None, he=None, T0=None):
    """One thermo point per column of Y, from T (he returned) or from he with the start T0 (T returned).
    Returns longdouble arrays T, he, psi, rho, mu, alpha [n], rhoD, hai, X, kappa [S, n], Wm, cp [n], and the mixture's
    h just below and just above each distinct T_mid (tmid [m], h_below, h_above [m, n])."""
    S = t.S
    Y = _ld(Y); p = _ld(p)
    X, Wm = composition(t, Y)
    if T is None:
        T = solve_T(t, Y, he, T0)
        he = _ld(he)
    else:
        T = _ld(T)
        he = mixture_h_cp(t, T, Y)[0]
    hai, _ = species_h_cp(t, T)
    cp = mixture_h_cp(t, T, Y)[1]
    psi = Wm / (LD(R_GAS) * T)
    rho = p * psi
    lnT = np.log(T)
    L = np.stack([np.ones_like(lnT), lnT, lnT ** 2, lnT ** 3, lnT ** 4])          # [5, n]
    sT = np.sqrt(T)
    W = _ld(t.W)
    sv = _ld(t.visc) @ L                                                          # sqrt(mu_i / sqrt T)  [S, n]
    mu_i = sT * sv * sv
    wr = W[:, None] / W[None, :]                                                  # W_i / W_j
    phi = (1 + (sv[:, None, :] / sv[None, :, :]) * ((1 / wr) ** LD(0.25))[:, :, None]) ** 2 \
        / np.sqrt(LD(8) * (1 + wr))[:, :, None]                                   # [i, j, n]
    mu = (X * mu_i / (X[None, :, :] * phi).sum(axis=1)).sum(axis=0)
    lam = sT * (_ld(t.cond) @ L)
    alpha = ((X * lam).sum(axis=0) + 1 / (X / lam).sum(axis=0)) / (2 * cp)
    pD = (T * sT)[None, None, :] * np.einsum("ijk,kn->ijn", _ld(t.bdiff), L)      # p D_ij  [i, j, n]
    off = ~np.eye(S, dtype=bool)[:, :, None]
    s1 = np.where(off, X[None, :, :] / pD, 0).sum(axis=1)
    s2 = np.where(off, (X * W[:, None])[None, :, :] / pD, 0).sum(axis=1)
    cut = X + LD(CUT) > 1
    with np.errstate(divide="ignore", invalid="ignore"):
        den = Wm[None, :] - X * W[:, None]
        kappa = np.where(den > 0, Wm[None, :] / den, LD(np.inf))
        rhoD = np.where(cut, LD(0), psi[None, :] / (s1 + s2 * X / den))
    tmid, h_below, h_above = one_sided_h(t, Y)
    return {"T": T, "he": he, "psi": psi, "rho": rho, "mu": mu, "alpha": alpha, "rhoD": rhoD, "hai": hai, "X": X,
            "Wm": Wm, "kappa": kappa, "cp": cp, "mu_i": mu_i, "tmid": tmid, "h_below": h_below, "h_above": h_above}


# ------------------------------------------------------------------------------------------------ error measure
def _rel(a, b):
    b = _ld(b)
    return np.asarray(np.abs(_ld(a) - b) / np.abs(b), dtype=np.float64)


def errors(t, got, ref):
    """per-element errors of got (float64 arrays) against ref (evaluate's result): relative for the positive T, psi,
    rho, mu, alpha and non-zero rhoD; he over max(|ref|, R T / Wm), hai_i over max(|ref|, R T / W_i). rhoD_kappa =
    rhoD's error over kappa_i 2^-52. Where the reference's rhoD is exactly 0 the value must be exactly 0 (error
    inf otherwise)."""
    e = {q: _rel(got[q], ref[q]) for q in ("T", "psi", "rho", "mu", "alpha")}
    RT = LD(R_GAS) * ref["T"]
    e["he"] = np.asarray(np.abs(_ld(got["he"]) - ref["he"]) / np.maximum(np.abs(ref["he"]), RT / ref["Wm"]), dtype=np.float64)
    sc = np.maximum(np.abs(ref["hai"]), RT[None, :] / _ld(t.W)[:, None])
    e["hai"] = np.asarray(np.abs(_ld(got["hai"]) - ref["hai"]) / sc, dtype=np.float64)
    zero = np.asarray(ref["rhoD"] == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(zero, np.where(np.asarray(got["rhoD"]) == 0.0, 0.0, np.inf), _rel(got["rhoD"], np.where(zero, 1, ref["rhoD"])))
        e["rhoD"] = r
        e["rhoD_kappa"] = np.where(zero, r, r / (np.asarray(ref["kappa"], dtype=np.float64) * EPS))
    e["rhoD_dominant"] = np.where(dominant(ref["X"]), e["rhoD_kappa"], 0.0)
    return e


def dominant(X):
    """the species that makes up most of a state (X_i > 1/2): on near_pure the one whose rhoD_i cancels"""
    return np.asarray(X, dtype=np.float64) > 0.5


def kappa_form(cls, kappa):
    """where rhoD is held to (constant) kappa_i 2^-52 instead of a plain relative bound: the near-pure class, and
    any element with kappa_i > 10"""
    k = np.asarray(kappa, dtype=np.float64)
    return np.ones(k.shape, dtype=bool) if cls == "near_pure" else k > 10


def maxima(cls, e, ref):
    """the figures kept per class: the largest error of each quantity; rhoD over the elements held to a plain
    relative bound, rhoD_kappa over all, rhoD_dominant (the same ratio over the dominant species alone) on near_pure"""
    kf = kappa_form(cls, ref["kappa"])
    out = {}
    for q in QUANTITIES:
        v = e[q]
        if q == "rhoD":
            v = v[~kf]
        if q == "rhoD_dominant" and cls != "near_pure":
            v = v[:0]
        out[q] = float(v.max()) if v.size else 0.0
    return out


# ------------------------------------------------------------------------------------------------ states
@dataclass
class States:
    cls: str
    from_T: bool          # evaluated from T (he is an output) or from he (T holds the Newton start T0)
    T: np.ndarray         # [n]
    he: np.ndarray        # [n] (from_T: unused, zeros)
    p: np.ndarray         # [n]
    Y: np.ndarray         # [S, n]
    tmid: np.ndarray | None = None   # jump: the switch each state sits at

    @property
    def n(self):
        return int(self.T.shape[0])


def _rng(t, cls, seed):
    return np.random.default_rng([seed, t.S, CLASSES.index(cls)])


def _broad(t, rng, n):
    T = rng.uniform(200.0, 3500.0, n)
    p = ATM * np.exp(rng.uniform(np.log(0.1), np.log(50.0), n))
    Y = rng.gamma(0.3, 1.0, (t.S, n))
    Y = np.maximum(Y, 1e-300)
    return T, p, Y / Y.sum(axis=0)


def _he_of(t, T, Y):
    return np.asarray(mixture_h_cp(t, T, Y)[0], dtype=np.float64)


def _check_cut_margin(t, Y):
    X, _ = composition(t, Y)
    d = np.abs(np.asarray(X - (1 - LD(CUT)), dtype=np.float64))
    assert d.min() >= CUT_MARGIN, "a state sits on the rhoD cut"


def states(t, cls, seed=0, n=160):
    """the seeded states of one class for table t"""
    S = t.S
    rng = _rng(t, cls, seed)
    tms = distinct_tmid(t) if cls == "switch_T" else switching_tmid(t)
    if cls == "broad":
        T, p, Y = _broad(t, rng, n)
        st = States(cls, True, T, np.zeros(n), p, Y)
    elif cls == "zeros":
        T, p, Y = _broad(t, rng, n)
        for k in range(n):
            Y[rng.permutation(S)[: S // 2], k] = 0.0
        st = States(cls, True, T, np.zeros(n), p, Y / Y.sum(axis=0))
    elif cls == "pure":
        cols = [np.eye(S)[:, i] for i in range(S)]
        pairs = sorted({(min(a, b), max(a, b)) for a, b in ((0, 1), (0, S - 1), (S // 2, S - 1)) if a != b})
        for i, j in pairs:
            for f in (0.5, 0.1, 0.9):
                y = np.zeros(S); y[i] = f; y[j] = 1.0 - f
                cols.append(y)
        Y = np.stack(cols, axis=1)
        m = Y.shape[1]
        T = rng.uniform(250.0, 3200.0, m)
        p = ATM * np.exp(rng.uniform(np.log(0.1), np.log(50.0), m))
        st = States(cls, True, T, np.zeros(m), p, Y)
    elif cls == "near_pure":
        cols = []
        for i in range(S):
            for d in (1e-3, 1e-6, 1e-9):
                x = np.full(S, d / (S - 1)); x[i] = 1.0 - d
                y = x * t.W
                cols.append(y / y.sum())
        Y = np.stack(cols, axis=1)
        m = Y.shape[1]
        T = rng.uniform(250.0, 3200.0, m)
        p = ATM * np.exp(rng.uniform(np.log(0.1), np.log(50.0), m))
        st = States(cls, True, T, np.zeros(m), p, Y)
    elif cls == "switch_T":
        Ts = []
        for tm in tms:
            Ts += [tm, np.nextafter(tm, -np.inf), np.nextafter(tm, np.inf), tm * (1 - 1e-12), tm * (1 + 1e-12),
                   tm * (1 - 1e-6), tm * (1 + 1e-6)]
        k = 6
        _, p, Y = _broad(t, rng, k * len(Ts))
        T = np.repeat(np.array(Ts), k)
        st = States(cls, True, T, np.zeros(T.size), p, Y)
    elif cls == "newton":
        nb = max(n // 5, 8)
        Tb, pb, Yb = _broad(t, rng, nb)
        Tn = np.array([tm * (1 + s * d) for tm in tms for d in (1e-3, 1e-2) for s in (-1, 1)])
        Tn = np.repeat(Tn, 2)
        _, pn, Yn = _broad(t, rng, Tn.size)
        Ts, p, Y = np.concatenate([Tb, Tn]), np.concatenate([pb, pn]), np.concatenate([Yb, Yn], axis=1)
        he = _he_of(t, Ts, Y)
        near = tms[np.abs(Ts[:, None] - tms[None, :]).argmin(axis=1)]
        other = np.maximum(np.where(Ts > near, near - 150.0, near + 150.0), 150.0)
        starts = [0.9 * Ts, 1.1 * Ts, np.full(Ts.size, 300.0), np.full(Ts.size, 3000.0), other]
        st = States(cls, False, np.concatenate(starts), np.tile(he, 5), np.tile(p, 5), np.tile(Y, (1, 5)))
        Tref = np.asarray(solve_T(t, st.Y, st.he, st.T), dtype=np.float64)
        assert np.all(np.abs(Tref[:, None] - tms[None, :]) > JUMP_ZONE * tms[None, :]), "a newton state sits in a jump zone"
    elif cls == "jump":
        k = 6
        T0, he, p, Y, tmid = [], [], [], [], []
        for tm in tms:
            _, pk, Yk = _broad(t, rng, k)
            alltm, lo, hi = one_sided_h(t, Yk)
            i = int(np.where(alltm == tm)[0][0])
            lo64, hi64 = np.asarray(lo[i], dtype=np.float64), np.asarray(hi[i], dtype=np.float64)
            targets = [lo64 + f * (hi64 - lo64) for f in (0.25, 0.5, 0.75)]
            targets += [_he_of(t, np.full(k, tm * (1 + s)), Yk) for s in (-4e-6, -1e-6, -1e-7, 0.0, 1e-7, 1e-6, 4e-6)]
            for q, h in enumerate(targets):
                T0.append(np.full(k, tm + (100.0 if q % 2 else -100.0))); he.append(h); p.append(pk); Y.append(Yk)
                tmid.append(np.full(k, tm))
        st = States(cls, False, np.concatenate(T0), np.concatenate(he), np.concatenate(p), np.concatenate(Y, axis=1),
                    np.concatenate(tmid))
    else:
        raise KeyError(cls)
    _check_cut_margin(t, st.Y)
    return st


def reference_for(t, st, got_T=None):
    """the reference at the states; jump: evaluated from the T the code under test returned (T(he) is undefined there)"""
    if st.from_T:
        return evaluate(t, st.p, st.Y, T=st.T)
    if st.cls == "jump":
        r = evaluate(t, st.p, st.Y, T=got_T)
        r["he_from_T"] = r["he"]
        r["he"] = _ld(st.he)       # from he the energy is passed through
        return r
    # newton. The equation he = h(T) is solved between 100 K and 6000 K, where h rises with T and the root is the
    # only one. Far above the fits' ranges (they end at 3500 K for most species) the extrapolated h(T) turns over
    # near 7000 K and the same equation has a second root there. The Newton iteration the kernels port (dfThermo.cu:
    # 296-320, no safeguard) overshoots into that region from a start thousands of kelvin below a hot target
    # (T0 = 300 K, T* near 3450 K) and then converges to the upper root: T(he, T0) is that root, by the method's own
    # definition. For such a state (`stray`) the reference is evaluated at the limit of the plain iteration carried
    # to convergence in long double, which must itself be a root; no state is left out and the bound is unchanged.
    Ts = solve_T(t, st.Y, st.he, st.T)
    Tn, conv = newton_limit(t, st.Y, st.he, st.T)
    assert conv.all(), "the plain Newton iteration has no limit for a newton state"
    stray = np.abs(Tn - Ts) > LD(1e-12) * Ts
    r = evaluate(t, st.p, st.Y, T=np.where(stray, Tn, Ts))
    scale = np.maximum(np.abs(_ld(st.he)), LD(R_GAS) * r["T"] / r["Wm"])
    assert float((np.abs(r["he"] - _ld(st.he)) / scale).max()) < 1e-15, "the reference T is not a root"
    r["he"] = _ld(st.he)
    r["stray"] = np.asarray(stray)
    return r


def jump_he_slack(t, st, ref):
    """jump states: how far he may sit from h(T returned), in the units errors() judges he by. The target lies inside
    (or within JUMP_ZONE T_mid of) a discontinuity of h, so the iteration ends on one side of it with a residual of
    up to the jump itself plus the slope times the distance it may stop at."""
    tms, lo, hi = ref["tmid"], ref["h_below"], ref["h_above"]
    i = np.searchsorted(tms, st.tmid)
    k = np.arange(st.n)
    jump = np.abs(hi[i, k] - lo[i, k])
    scale = np.maximum(np.abs(ref["he"]), LD(R_GAS) * ref["T"] / ref["Wm"])
    return np.asarray((jump + ref["cp"] * LD(JUMP_STOP) * _ld(st.tmid)) / scale, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ bounds
def cpu_tables():
    """the tables the oracle is measured on: S = 7 (ES80), 9 (Burke), 16, 53, 64 and a non-symmetric variant; S = 32
    because its newton class holds a state whose Newton iteration strays to the upper root (reference_for)"""
    return {"es80": mech_table("es80"), "burke9": mech_table("burke9"), "gri16": gri_table(16), "gri32": gri_table(32),
            "gri53": gri_table(53),
            "gri64": gri_table(64), "gri9-nonsym": nonsymmetric(gri_table(9))}


def oracle_errors(t, st):
    """errors of the fp64 sequential oracle at the states, and the reference used"""
    _dfmi_path()
    import oracle as O
    got = O.thermo_points(t, st.T, st.he, st.p, st.Y, st.from_T)
    ref = reference_for(t, st, got["T"])
    return errors(t, got, ref), ref, got


def measure():
    """{table: {class: {quantity: max}}} of the oracle against the reference"""
    out = {}
    for name, t in cpu_tables().items():
        out[name] = {}
        for cls in CLASSES:
            st = states(t, cls)
            e, ref, _ = oracle_errors(t, st)
            out[name][cls] = maxima(cls, e, ref)
    return out


def class_maxima(per_table):
    return {cls: {q: max(per_table[n][cls][q] for n in per_table) for q in QUANTITIES} for cls in CLASSES}


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def gpu_bound(bounds, cls, q):
    """4x the oracle's measured maximum, floored at 1e-13 (the factor covers contracted FMAs, Newton-refined
    reciprocals, shared T powers, rotation-order row sums and the device log / sqrt: one more rounding per term
    each). For rhoD_kappa and rhoD_dominant the result is the constant c of the per-element bound
    max(1e-13, c kappa_i 2^-52)."""
    b = 4.0 * bounds["classes"][cls][q]
    return b if q in ("rhoD_kappa", "rhoD_dominant") else max(b, 1e-13)


def rhoD_bounds(bounds, cls, kappa, X):
    """per-element bound on rhoD's relative error. The class constant of the kappa form is set by the minor species
    (kappa = 1, the rounding of S-term sums); near_pure's dominant species, whose error is the cancellation's alone,
    are held to the constant measured on them."""
    k = np.asarray(kappa, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        kb = np.maximum(gpu_bound(bounds, cls, "rhoD_kappa") * k * EPS, 1e-13)
        if cls == "near_pure":
            kb = np.where(dominant(X), np.maximum(gpu_bound(bounds, cls, "rhoD_dominant") * k * EPS, 1e-13), kb)
    return np.where(kappa_form(cls, k), kb, gpu_bound(bounds, cls, "rhoD"))


if __name__ == "__main__":
    if "--measure" not in sys.argv:
        sys.exit("usage: thermo_reference.py --measure")
    per_table = measure()
    doc = {"about": "max error of the fp64 sequential oracle (oracle.thermo_points) against tests/thermo_reference.py, "
                    "per state class and quantity; rhoD over the elements with kappa <= 10 outside near_pure, "
                    "rhoD_kappa = error / (kappa 2^-52) over all; written by tests/thermo_reference.py --measure",
           "classes": class_maxima(per_table), "tables": per_table}
    with open(BOUNDS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for cls, v in doc["classes"].items():
        print(cls, {q: f"{x:.2e}" for q, x in v.items()})
