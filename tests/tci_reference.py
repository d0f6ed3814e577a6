"""NumPy restatement of the PaSR and EDC combustion closures (include/dfmi.h dfmi_combustion_correct).

TEST INFRASTRUCTURE -- never the product path. Every function evaluates the header's statement in the number type it is
given (np.float64 or np.longdouble), one cell per array element, with the sums over species and over reactions as Python
loops in species / reaction order; nothing is reassociated. The long-double evaluation is the yardstick, the fp64 one
measures what fp64 can do with the same statement:

`python tests/tci_reference.py --measure` evaluates every quantity on every state class in both types and writes the
maximum error of the fp64 evaluation per quantity and class to tests/golden/tci_bounds.json. A device value is held to 4x that
figure, floored at 1e-13 (gpu_bound; the rule of thermo_point_bounds.json and ras_bounds.json). Errors are relative to
the long-double value; where that is exactly 0 the other value must be 0 too (the error is then reported as its magnitude).

The forward and reverse rates of progress are chem_oracle.Kinetics.rates_of_progress split into its two halves, in the
operation order of the library's kernels (k = A exp(b ln T - Ta / T), 1 / Kc = exp(dG - dnu ln(p_atm / (R T)))).

Every comparison of the statement is also returned as a pair (left, right, kind): `branch_report` checks that the fp64
and the long-double evaluation take the same side and that a computed left side is either equal to the right side in both
or at least MARGIN_ULPS fp64 ulps away from it, so that two roundings cannot disagree about a branch.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUNDS_PATH = os.path.join(GOLDEN, "tci_bounds.json")
for _p in (os.path.join(os.path.dirname(HERE), "deepflame-dev_amd"), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

LD = np.longdouble
SMALL = 1e-15
VGREAT = 1e300
RU = 8314.46261815324
P_ATM = 101325.0
MARGIN_ULPS = 4
EPS64 = float(np.finfo(np.float64).eps)
DEFAULTS = {"Cmix": 0.1, "C1": 0.05774, "C2": 0.5, "Cgamma": 2.1377, "Ctau": 0.4083}
VERSION_EXP = {1981: (3, 3), 1996: (2, 3), 2005: (2, 2), 2016: (2, 2)}
MECHS = {"burke9": ("Burke2012_s9r23.yaml", "thermo_Burke2012_s9r23.txt"), "drm19": ("drm19.yaml", None)}


# ------------------------------------------------------------------------------------------------ pointwise statement
def _a(v, T):
    return np.asarray(v, dtype=T)


def tmix_of(mixing, Cmix, k, eps, mu, rho, T=np.float64):
    k, eps, mu, rho = _a(k, T), _a(eps, T), _a(mu, T), _a(rho, T)
    e = eps + T(SMALL)
    if mixing == 1:
        return T(Cmix) * k / e
    if mixing == 2:
        return np.sqrt(np.abs(mu / rho / e))
    return np.sqrt(np.abs(k / e) * np.sqrt(np.abs(mu / rho / e)))


def tc_formation(RR, Y, T=np.float64):
    """laminar::tc(): max_i (|RR_i| > small ? Y_i / |RR_i| : 0), from 0, in species order"""
    RR, Y = _a(RR, T), _a(Y, T)
    t = np.zeros(RR.shape[1], dtype=T)
    for i in range(RR.shape[0]):
        a = np.abs(RR[i])
        on = a > T(SMALL)
        t = np.maximum(t, np.where(on, Y[i] / np.where(on, a, T(1)), T(0)))
    return t


def tc_global(idx, rho, RR, Y, t0, T=np.float64, cmp=None):
    """globalConvertion; idx = {"oxidizer", "fuel", "CO2", "H2"} -> species index or -1"""
    rho, RR, Y, t0 = _a(rho, T), _a(RR, T), _a(Y, T), _a(t0, T)
    tc = None
    for key in ("oxidizer", "fuel", "CO2", "H2"):
        i = idx.get(key, -1)
        if i < 0:
            continue
        r, y = RR[i], Y[i]
        sgn = T(1) if key == "CO2" else T(-1)
        on = ((r > 0) if key == "CO2" else (r < 0)) & (y > T(1e-10))
        if cmp is not None:
            cmp.append((r, np.zeros_like(r), "input"))
            cmp.append((y, np.full_like(y, T(1e-10)), "input"))
        t = np.where(on, sgn * rho * y / np.where(on, r, T(1)), t0)
        tc = t if tc is None else np.maximum(tc, t)
    return tc


def kappa_pasr(tmix, tc, T=np.float64, cmp=None):
    tmix, tc = _a(tmix, T), _a(tc, T)
    if cmp is not None:
        cmp.append((tmix, np.full_like(tmix, T(SMALL)), "computed"))
        cmp.append((tc, np.full_like(tc, T(SMALL)), "computed"))
    on = (tmix > T(SMALL)) & (tc > T(SMALL))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(on, tc / (tc + tmix), T(1))


def ipow(g, e):
    v = g
    for _ in range(1, e):
        v = v * g
    return v


def edc(version, coef, e1, e2, k, eps, mu, rho, tc=None, T=np.float64, cmp=None):
    """(kappa, tauStar, gammaL); tc: the formationRate scale (v2016). e1, e2 = 0: the version's own exponents"""
    q = dict(DEFAULTS, **(coef or {}))
    k, eps, mu, rho = _a(k, T), _a(eps, T), _a(mu, T), _a(rho, T)
    d1, d2 = VERSION_EXP[version]
    e1, e2 = e1 or d1, e2 or d2
    nu = mu / (rho + T(SMALL))
    tk = np.sqrt(nu / (eps + T(SMALL)))
    g4 = np.sqrt(np.sqrt(nu * eps / (k * k + T(SMALL))))
    if version == 2016:
        tc = _a(tc, T)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = tk / tc
        Da = np.maximum(np.minimum(ratio, T(10)), T(1e-10))
        ReT = k * k / (nu * eps + T(SMALL))
        a = T(q["C1"]) / (Da * np.sqrt(ReT + T(1)))
        b = T(q["C2"]) * np.sqrt(Da * (ReT + T(1)))
        CtauI = np.minimum(a, T(2.1377))
        CgammaI = np.maximum(np.minimum(b, T(5)), T(0.4082))
        if cmp is not None:
            cmp += [(ratio, np.full_like(ratio, T(10)), "computed"), (ratio, np.full_like(ratio, T(1e-10)), "computed"),
                    (a, np.full_like(a, T(2.1377)), "computed"), (b, np.full_like(b, T(5)), "computed"),
                    (b, np.full_like(b, T(0.4082)), "computed")]
        gammaL = CgammaI * g4
        tau = CtauI * tk
    else:
        gammaL = T(q["Cgamma"]) * g4
        tau = T(q["Ctau"]) * tk
    one = gammaL >= T(1)
    gs = np.where(one, T(0.5), gammaL)
    quot = ipow(gs, e1) / (T(1) - ipow(gs, e2))
    if cmp is not None:
        cmp.append((gammaL, np.ones_like(gammaL), "computed"))
        cmp.append((np.where(one, T(0.5), quot), np.ones_like(quot), "computed"))
    kappa = np.where(one, T(1), np.maximum(np.minimum(quot, T(1)), T(0)))
    return kappa, tau, gammaL


def branch_report(pairs64, pairsLD):
    """problems (strings) of the comparisons of one evaluation in fp64 and in long double: sides that differ, and computed
    left sides closer than MARGIN_ULPS fp64 ulps to the right side without being equal to it in both"""
    bad = []
    for n, ((a, b, kind), (A, B, _)) in enumerate(zip(pairs64, pairsLD)):
        a, b, A, B = np.asarray(a), np.asarray(b), np.asarray(A), np.asarray(B)
        fin = np.isfinite(A.astype(np.float64)) & np.isfinite(a)
        s64, sLD = np.sign(a - b), np.sign(A - B)
        differ = fin & (s64 != sLD.astype(np.float64))
        if differ.any():
            bad.append(f"comparison {n}: fp64 and long double take different sides in cells {np.flatnonzero(differ)[:5]}")
        if kind == "computed":
            gap = np.abs(A - B)
            near = fin & ~((a == b) & (A == B)) & (gap.astype(np.float64) < MARGIN_ULPS * EPS64 * np.abs(b))
            if near.any():
                bad.append(f"comparison {n}: cells {np.flatnonzero(near)[:5]} within {MARGIN_ULPS} ulps of the threshold")
    return bad


# ------------------------------------------------------------------------------------------------ rates of progress
def load_mech(name):
    """(species, mechanism, nasa, W) of a tests/golden mechanism"""
    from dfmi.kinetics import parse_mechanism
    from dfmi.mech import read_yaml_mechanism
    path = os.path.join(GOLDEN, MECHS[name][0])
    ym = read_yaml_mechanism(path)
    return ym["species"], parse_mechanism(path), np.asarray(ym["nasa"], dtype=np.float64), np.asarray(ym["W"], dtype=np.float64)


def _g_rt(nasa, Tk, T):
    lnT = np.log(Tk)
    out = []
    for row in nasa:
        a = [T(v) for v in (row[1:8] if Tk > T(row[0]) else row[8:15])]
        h = a[0] + a[1] * Tk / T(2) + a[2] * Tk * Tk / T(3) + a[3] * Tk * Tk * Tk / T(4) + a[4] * Tk * Tk * Tk * Tk / T(5) + a[5] / Tk
        s = a[0] * lnT + a[1] * Tk + a[2] * Tk * Tk / T(2) + a[3] * Tk * Tk * Tk / T(3) + a[4] * Tk * Tk * Tk * Tk / T(4) + a[6]
        out.append(h - s)
    return out


def _cpow(c, nu, T):
    return c if nu == 1.0 else (c * c if nu == 2.0 else (c * c * c if nu == 3.0 else np.power(c, T(nu))))


def fwd_rev(m, nasa, Tk, C, T=np.float64):
    """(fwd[R], rev[R]): getFwdRatesOfProgress / getRevRatesOfProgress of one cell at temperature Tk and concentrations C
    -- the two halves Kinetics.rates_of_progress differences, third-body and fall-off factors included"""
    Tk = T(Tk)
    lnT, rT = np.log(Tk), T(1) / Tk
    g = _g_rt(nasa, Tk, T)
    fwd, rev = [], []
    for r in range(m.R):
        kf = T(m.A[r]) * np.exp(T(m.b[r]) * lnT - T(m.Ta[r]) * rT)
        typ = int(m.itype[r])
        k, Mf = kf, T(1)
        if typ != 0:
            M = T(0)
            for i in range(m.S):
                M = M + T(m.eff[r][i]) * C[i]
            if typ == 1:
                Mf = M
            else:
                k0 = T(m.A0[r]) * np.exp(T(m.b0[r]) * lnT - T(m.Ta0[r]) * rT)
                Pr = k0 * M / kf
                F = T(1)
                if typ == 3:
                    a, T3, T1, T2 = (T(v) for v in m.troe[r])
                    Fc = (T(1) - a) * np.exp(-Tk / T3) + a * np.exp(-Tk / T1) + (np.exp(-T2 / Tk) if m.has_T2[r] else T(0))
                    lFc = np.log10(max(Fc, T(1e-300)))
                    c = T(-0.4) - T(0.67) * lFc
                    n = T(0.75) - T(1.27) * lFc
                    lPr = np.log10(max(Pr, T(1e-300)))
                    f1 = (lPr + c) / (n - T(0.14) * (lPr + c))
                    F = np.power(T(10), lFc / (T(1) + f1 * f1))
                k = kf * Pr / (T(1) + Pr) * F
        ik = T(0)
        if m.reversible[r]:
            dG, dnu = T(0), T(0)
            for j in range(3):
                ip, ir = int(m.prod[r, j]), int(m.reac[r, j])
                if ip >= 0:
                    dG = dG + T(m.nu_p[r, j]) * g[ip]
                if ir >= 0:
                    dG = dG - T(m.nu_r[r, j]) * g[ir]
                if ip >= 0:
                    dnu = dnu + T(m.nu_p[r, j])
                if ir >= 0:
                    dnu = dnu - T(m.nu_r[r, j])
            ik = np.exp(dG - dnu * np.log(T(P_ATM) / (T(RU) * Tk)))
        f = k
        b = k * ik if m.reversible[r] else T(0)
        for j in range(3):
            if m.reac[r, j] >= 0:
                f = f * _cpow(C[int(m.reac[r, j])], float(m.nu_r[r, j]), T)
            if m.prod[r, j] >= 0:
                b = b * _cpow(C[int(m.prod[r, j])], float(m.nu_p[r, j]), T)
        fwd.append(Mf * f)
        rev.append(Mf * b)
    return fwd, rev


def tc_reaction(m, nasa, W, Tc, p, rho, Y, T=np.float64):
    """PaSR reactionRate per cell: sumW / sumSq * cSum at setState_TPX(T, p, X), X_i = rho Y_i / W_i"""
    Y = np.asarray(Y)
    n = Y.shape[1]
    out = np.zeros(n, dtype=T)
    with np.errstate(all="ignore"):
        for c in range(n):
            X = [T(rho[c]) * T(Y[i, c]) / T(W[i]) for i in range(m.S)]
            cSum = T(0)
            for i in range(m.S):
                cSum = cSum + X[i]
            xs = T(0)
            for i in range(m.S):
                xs = xs + max(X[i], T(0))
            ct = T(p[c]) / (T(RU) * T(Tc[c]))
            C = [max(X[i], T(0)) / xs * ct for i in range(m.S)]
            fwd, rev = fwd_rev(m, nasa, Tc[c], C, T)
            sumW, sumSq = T(0), T(0)
            for r in range(m.R):
                wf, wr = T(0), T(0)
                for j in range(3):
                    if m.prod[r, j] >= 0:
                        wf = wf + T(m.nu_p[r, j]) * fwd[r]
                    if m.reac[r, j] >= 0:
                        wr = wr + T(m.nu_r[r, j]) * rev[r]
                sumW = sumW + wf
                sumW = sumW + wr
                sumSq = sumSq + wf * wf
                sumSq = sumSq + wr * wr
            out[c] = T(VGREAT) if sumSq == 0 else sumW / sumSq * cSum
    return out


# ------------------------------------------------------------------------------------------------ state classes
def _ulps(v, n):
    v = np.float64(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.inf if n > 0 else -np.inf)
    return v


def broad(n, S, W, seed=11):
    """T 300..2500 K, k and epsilon log-uniform over six decades, Y from gamma draws; RR of both signs over eight decades
    with a tenth of the entries exactly 0"""
    rng = np.random.default_rng(seed)
    T = 300.0 + 2200.0 * rng.random(n)
    Y = rng.gamma(0.4, 1.0, (S, n)) + 1e-300
    Y /= Y.sum(axis=0)
    p = 101325.0 * (1.0 + 0.05 * rng.standard_normal(n))
    Wm = 1.0 / (Y / np.asarray(W)[:, None]).sum(axis=0)
    rho = p * Wm / (RU * T) * (1.0 + 0.02 * rng.standard_normal(n))
    mu = 10.0 ** rng.uniform(-5.5, -3.5, n)
    k = 10.0 ** rng.uniform(-3, 3, n)
    eps = 10.0 ** rng.uniform(-1, 5, n)
    RR = rng.choice([-1.0, 1.0], (S, n)) * 10.0 ** rng.uniform(-4, 4, (S, n))
    RR[rng.random((S, n)) < 0.1] = 0.0
    Qdot = 1e6 * rng.standard_normal(n)
    t0 = 10.0 ** rng.uniform(-6, 0, n)
    return {"T": T, "p": p, "rho": rho, "mu": mu, "k": k, "epsilon": eps, "Y": Y, "RR": RR, "Qdot": Qdot, "tci_tc": t0}


def branches_pasr(n, S, W, idx, seed=12):
    """every side of the PaSR comparisons. The first cells are built by hand, the rest repeat `broad`:
    RR of the four species of each sign and zero; their Y at 1e-10 exactly, one ulp above and below;
    tmix at SMALL and 8 ulps beside it (Cmix = 1e-15 with k = e = 2^60 (1, 1 + 2^-49, 1 - 2^-49): use coef Cmix = 1e-15);
    tc at SMALL and beside it (rho = 2^-20, RR = -1, Y = 2^20 1e-15 (1, 1 +- 2^-49) for the fuel)"""
    st = broad(n, S, W, seed)
    sp = [idx[k] for k in ("oxidizer", "fuel", "CO2", "H2") if idx.get(k, -1) >= 0]
    c = 0
    ys = [1e-10, _ulps(1e-10, 1), _ulps(1e-10, -1), 1e-3]
    for i in sp:
        for r in (-3.0, 0.0, 2.0):
            for y in ys:
                if c >= n:
                    return st
                st["RR"][i, c], st["Y"][i, c] = r, y
                c += 1
    for f in (1.0, 1.0 + 2.0 ** -49, 1.0 - 2.0 ** -49):        # tmix = Cmix k / e at and beside SMALL when Cmix = 1e-15
        if c >= n:
            return st
        st["k"][c], st["epsilon"][c] = 2.0 ** 60 * f, 2.0 ** 60
        c += 1
    fu = idx.get("fuel", -1)
    if fu >= 0:
        for f in (1.0, 1.0 + 2.0 ** -49, 1.0 - 2.0 ** -49):    # tc = rho Y / -RR at and beside SMALL
            if c >= n:
                return st
            st["rho"][c] = 2.0 ** -20
            st["RR"][:, c] = 0.0
            st["RR"][fu, c] = -1.0
            st["Y"][fu, c] = 2.0 ** 20 * 1e-15 * f
            st["tci_tc"][c] = 1e-30                             # t0 below everything: the maximum is the fuel's scale
            c += 1
    return st


def branches_edc(n, S, W, seed=13):
    """gammaL at 1 and 8 ulps beside it (coef Cgamma = 1: mu = rho = 2^70, k = 2^40, eps = 2^80 (1, 1 +- 2^-47)); every
    clamp of v2016 active (tc = Y_0 / |RR_0| from 1e-14 to 1e8 against sqrt(nu / eps) at eps = 1e3, k from 1e-3 to 1e3);
    a cell with mu = 0 (tauStar = 0: not usable)"""
    st = broad(n, S, W, seed)
    c = 0
    for f in (1.0, 1.0 + 2.0 ** -47, 1.0 - 2.0 ** -47):
        if c >= n:
            return st
        st["mu"][c] = st["rho"][c] = 2.0 ** 70
        st["k"][c], st["epsilon"][c] = 2.0 ** 40, 2.0 ** 80 * f
        c += 1
    for tcv in (1e-14, 1e-9, 1e-3, 1e8):
        for kv in (1e-3, 1.0, 1e3):
            if c >= n:
                return st
            st["k"][c], st["epsilon"][c] = kv, 1e3
            st["RR"][:, c] = 0.0
            st["RR"][0, c] = 1e-9
            st["Y"][0, c] = tcv * 1e-9                           # formationRate tc = Y_0 / |RR_0|
            c += 1
    if c < n:
        st["mu"][c] = 0.0
    return st


def inert_cell(st, c, S, inert):
    """cell c pure inert species: every rate of progress is 0"""
    st["Y"][:, c] = 0.0
    st["Y"][inert, c] = 1.0


# ------------------------------------------------------------------------------------------------ evaluation
def evaluate_pasr(st, mixing, chemistry, idx, coef=None, mech=None, T=np.float64, cmp=None):
    """{"tci_tmix", "tci_tc", "tci_kappa"} of a state; mech = (m, nasa, W) for reactionRate"""
    q = dict(DEFAULTS, **(coef or {}))
    tm = tmix_of(mixing, q["Cmix"], st["k"], st["epsilon"], st["mu"], st["rho"], T)
    if chemistry == 1:
        tc = tc_global(idx, st["rho"], st["RR"], st["Y"], st["tci_tc"], T, cmp)
    elif chemistry == 2:
        tc = tc_formation(st["RR"], st["Y"], T)
    else:
        tc = tc_reaction(mech[0], mech[1], mech[2], st["T"], st["p"], st["rho"], st["Y"], T)
    return {"tci_tmix": tm, "tci_tc": tc, "tci_kappa": kappa_pasr(tm, tc, T, cmp)}


def evaluate_edc(st, version, coef=None, e1=0, e2=0, T=np.float64, cmp=None):
    tc = tc_formation(st["RR"], st["Y"], T) if version == 2016 else None
    kap, tau, g = edc(version, coef, e1, e2, st["k"], st["epsilon"], st["mu"], st["rho"], tc, T, cmp)
    out = {"tci_kappa": kap, "tci_tauStar": tau}
    if tc is not None:
        out["tci_tc"] = tc
    return out


def rel_error(got, ref):
    """|got - ref| / |ref| per element in long double (|got| where ref is 0; 0 where both are the same infinity or NaN)"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    with np.errstate(all="ignore"):
        e = np.where(ref != 0, np.abs(got - ref) / np.abs(ref), np.abs(got))
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    return np.where(same, LD(0), e).astype(np.float64)


N_MEASURE = 512
IDX_NAMES = ("oxidizer", "fuel", "CO2", "H2")


def species_idx(species):
    want = {"oxidizer": "O2", "fuel": "CH4" if "CH4" in species else "H2", "CO2": "CO2", "H2": "H2"}
    return {k: (species.index(v) if v in species else -1) for k, v in want.items()}


def measure():
    out = {}
    for name in MECHS:
        species, m, nasa, W = load_mech(name)
        S = len(species)
        idx = species_idx(species)
        classes = {"broad": (broad(N_MEASURE, S, W), None), "branches": (branches_pasr(N_MEASURE, S, W, idx), {"Cmix": 1e-15}),
                   "branches_edc": (branches_edc(N_MEASURE, S, W), {"Cgamma": 1.0})}
        res = {}
        for cname, (st, coef) in classes.items():
            acc = {}

            def take(tag, a, b):
                for qn in a:
                    e = rel_error(a[qn], b[qn])
                    e = e[np.isfinite(e)]
                    acc[f"{tag}.{qn}"] = max(acc.get(f"{tag}.{qn}", 0.0), float(e.max(initial=0.0)))
            for mixing in (1, 2, 3):
                for chem in (1, 2):
                    take(f"pasr.c{chem}", evaluate_pasr(st, mixing, chem, idx, coef), evaluate_pasr(st, mixing, chem, idx, coef, T=LD))
            sub = {k: (v[..., :64] if isinstance(v, np.ndarray) else v) for k, v in st.items()}   # the reaction loop is slow
            inert_cell(sub, 5, S, species.index("N2"))
            for mixing in (1, 2, 3):
                take("pasr.c3", evaluate_pasr(sub, mixing, 3, idx, coef, (m, nasa, W)),
                     evaluate_pasr(sub, mixing, 3, idx, coef, (m, nasa, W), T=LD))
            for ver in VERSION_EXP:
                for e1, e2 in ((0, 0), (1, 4), (4, 1), (3, 2)):
                    take(f"edc.v{ver}", evaluate_edc(st, ver, coef, e1, e2), evaluate_edc(st, ver, coef, e1, e2, T=LD))
            res[cname] = acc
        out[name] = res
    return out


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def gpu_bound(bounds, mech, cls, what):
    """4x the fp64 restatement's measured maximum for that mechanism, class and quantity, floored at 1e-13"""
    return max(4.0 * bounds["mechanisms"][mech][cls][what], 1e-13)


if __name__ == "__main__":
    if "--measure" not in sys.argv:
        sys.exit("usage: tci_reference.py --measure")
    doc = {"about": "max over cells of the relative error of the fp64 evaluation of the PaSR / EDC statement (include/dfmi.h) "
                    "against its long-double evaluation, per mechanism, state class and quantity (pasr.c<chemistry scale>.<field>, "
                    "edc.v<version>.<field>; maximum over the mixing scales / exponent choices); written by "
                    "tests/tci_reference.py --measure",
           "mechanisms": measure()}
    with open(BOUNDS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, v in doc["mechanisms"].items():
        for c, w in v.items():
            print(name, c, {q: f"{x:.2e}" for q, x in w.items()})
