"""Reaction mechanisms at any species count and one-reaction mechanisms of every reaction form, for the chemistry sweep
(tests/test_chem_sweep_cpu.py, tests/test_gpu_chem_sweep.py, tests/golden/make_chem_sweep_fixtures.py).

TEST INFRASTRUCTURE. Everything is cut from tests/golden/gri30.yaml (36 species, 219 reactions) with
thermo_gri30_36.txt, and one form from Burke2012_s9r23.yaml. A mechanism is the tuple (Mechanism, nasa, W, ThermoTable):
what chem_oracle.Kinetics, tci_reference.tc_reaction and case.setup_context / Context.chem_set_mechanism take.

  prefix(S)              the first S species of ORDER and every gri30 reaction among them (4 <= S <= 36)
  cloned(n_clone, n_react)   prefix(36) plus renamed copies of the first n_clone species; the reactions of
                         prefix(n_react) act on the copies as well. The copies are stored in reverse, so the reacting
                         ones sit at the highest indices. cloned(28, 11): S = 64, R = 252; cloned(27, 11): S = 63.
  permuted(mt, perm)     species reordered everywhere (new species i is old species perm[i])
  with_duplicates(mt, R) the leading reactions appended again until there are R
  single(form)           one reaction of FORMS, its species padded with inert N2 / AR to 4
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
for _p in (os.path.join(os.path.dirname(HERE), "deepflame-dev_amd"), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

RU = 8314.46261815324
P_ATM = 101325.0
HEAD = ["H", "H2", "O2", "HO2", "OH", "O", "H2O", "H2O2", "N2", "CO", "CO2", "HCO", "AR", "CH2O", "CH3", "CH4"]
STABLE = {"H2", "O2", "H2O", "H2O2", "N2", "AR", "CO", "CO2", "CH4", "CH2O", "CH3OH", "C2H2", "C2H4", "C2H6", "CH2CO",
          "C3H8", "CH3CHO"}
# form -> (source, equation as the file writes it); single() clears has_T2 for "troe_T2_cleared"
FORMS = {
    "elementary": ("gri30", "O + H2 <=> H + OH"),
    "nu2": ("gri30", "2 OH <=> O + H2O"),
    "irreversible": ("gri30", "OH + CH3 => H2 + CH2O"),
    "three_body": ("gri30", "H + O2 + M <=> HO2 + M"),
    "h_2o2": ("gri30", "H + 2 O2 <=> HO2 + O2"),
    "lindemann": ("gri30", "O + CO (+M) <=> CO2 (+M)"),
    "troe_T2": ("gri30", "2 OH (+M) <=> H2O2 (+M)"),
    "troe_T2_cleared": ("gri30", "2 OH (+M) <=> H2O2 (+M)"),
    "three_products": ("gri30", "CH2(S) + O2 <=> H + OH + CO"),
    "burke_troe": ("burke", "H + O2 (+ M) <=> HO2 (+ M)"),
}
FALLOFF_FORMS = ("lindemann", "troe_T2", "troe_T2_cleared", "burke_troe")
SOURCES = {"gri30": ("gri30.yaml", "thermo_gri30_36.txt"), "burke": ("Burke2012_s9r23.yaml", "thermo_Burke2012_s9r23.txt")}
_src = {}


def source(name="gri30"):
    """(Mechanism, nasa, W, ThermoTable, equations) of a tests/golden mechanism as the file has it"""
    if name not in _src:
        from dfmi.kinetics import parse_mechanism
        from dfmi.mech import read_thermo_table, read_yaml_mechanism
        path = os.path.join(GOLDEN, SOURCES[name][0])
        ym = read_yaml_mechanism(path)
        t = read_thermo_table(os.path.join(GOLDEN, SOURCES[name][1]), ym["species"])
        eqs = [" ".join(str(x["equation"]).split()) for x in ym["reactions"]]
        _src[name] = (parse_mechanism(path), np.asarray(ym["nasa"], dtype=np.float64), np.asarray(ym["W"], dtype=np.float64), t, eqs)
    return _src[name]


def order():
    """gri30's 36 species: HEAD, then the rest in the file's order"""
    sp = source()[0].species
    return HEAD + [s for s in sp if s not in HEAD]


def _build(mt, names, sidx, rx):
    """mechanism of species mt[sidx] (indices may repeat) named `names` with the reactions rx = [(r, map)]: reaction r of
    mt with its species ids translated by map (old id -> new id). Efficiency columns and thermo rows follow sidx."""
    from dfmi.kinetics import Mechanism
    from dfmi.mech import ThermoTable
    m, nasa, W, t = mt[:4]
    sidx = np.asarray(sidx, dtype=np.int64)
    rr = np.asarray([r for r, _ in rx], dtype=np.int64)
    R = rr.size
    reac = -np.ones((R, 3), np.int32)
    prod = -np.ones((R, 3), np.int32)
    for k, (r, mp) in enumerate(rx):
        for j in range(3):
            if m.reac[r, j] >= 0:
                reac[k, j] = mp[int(m.reac[r, j])]
            if m.prod[r, j] >= 0:
                prod[k, j] = mp[int(m.prod[r, j])]
    take = lambda a: np.array(a[rr], copy=True)
    mech = Mechanism(list(names), len(names), R, take(m.itype), take(m.reversible), reac, prod, take(m.nu_r), take(m.nu_p),
                     take(m.A), take(m.b), take(m.Ta), take(m.A0), take(m.b0), take(m.Ta0), take(m.troe), take(m.has_T2),
                     np.ascontiguousarray(m.eff[rr][:, sidx]))
    table = ThermoTable(list(names), t.W[sidx].copy(), t.nasa[sidx].copy(), t.visc[sidx].copy(), t.cond[sidx].copy(),
                        t.bdiff[np.ix_(sidx, sidx)].copy())
    return mech, nasa[sidx].copy(), W[sidx].copy(), table


def _species_of(m, r):
    return [int(i) for i in list(m.reac[r]) + list(m.prod[r]) if i >= 0]


def _reactions_within(m, ids):
    ids = set(int(i) for i in ids)
    return [r for r in range(m.R) if all(i in ids for i in _species_of(m, r))]


def prefix(S):
    assert 4 <= S <= 36
    src = source()
    m = src[0]
    sidx = [m.species.index(s) for s in order()[:S]]
    mp = {old: new for new, old in enumerate(sidx)}
    return _build(src, order()[:S], sidx, [(r, mp) for r in _reactions_within(m, sidx)])


def cloned(n_clone, n_react):
    assert 0 < n_react <= n_clone <= 28
    src = source()
    m = src[0]
    names = order()
    base = [m.species.index(s) for s in names]
    sidx = base + [base[j] for j in reversed(range(n_clone))]          # the copy of species j sits at 36 + n_clone - 1 - j
    all_names = names + [names[j] + "_b" for j in reversed(range(n_clone))]
    mp = {old: new for new, old in enumerate(base)}
    mpc = {base[j]: 36 + n_clone - 1 - j for j in range(n_clone)}
    rx = [(r, mp) for r in _reactions_within(m, base)] + [(r, mpc) for r in _reactions_within(m, base[:n_react])]
    assert len(rx) <= 256
    return _build(src, all_names, sidx, rx)


def permuted(mt, perm):
    perm = [int(i) for i in perm]
    m = mt[0]
    assert sorted(perm) == list(range(m.S))
    inv = {old: new for new, old in enumerate(perm)}
    return _build(mt, [m.species[i] for i in perm], perm, [(r, inv) for r in range(m.R)])


def with_duplicates(mt, R_target):
    m = mt[0]
    assert m.R <= R_target <= 2 * m.R
    same = {i: i for i in range(m.S)}
    return _build(mt, m.species, range(m.S), [(r, same) for r in list(range(m.R)) + list(range(R_target - m.R))])


def single(form, reversible=None):
    """the one-reaction mechanism of a form; reversible = False clears the flag of a reversible form"""
    name, eq = FORMS[form]
    src = source(name)
    m = src[0]
    r = src[4].index(eq)
    ids = list(dict.fromkeys(_species_of(m, r)))
    n_own = len(ids)
    for pad in ("N2", "AR") + tuple(m.species):
        if len(ids) >= 4 and len(ids) > n_own:          # at least one inert species, for the pure-inert cell
            break
        if pad in m.species and m.species.index(pad) not in ids:
            ids.append(m.species.index(pad))
    mt = _build(src, [m.species[i] for i in ids], ids, [(r, {old: new for new, old in enumerate(ids)})])
    if form == "troe_T2_cleared":
        assert mt[0].has_T2[0] == 1 and mt[0].troe[0, 3] > 0
        mt[0].has_T2[0] = 0
    if reversible is not None:
        assert not reversible and mt[0].reversible[0] == 1
        mt[0].reversible[0] = 0
    return mt


def single_variants():
    """[(id, mechanism tuple)] of every form as written and, where reversible, with the flag cleared"""
    out = []
    for f in FORMS:
        mt = single(f)
        out.append((f, mt))
        if mt[0].reversible[0]:
            out.append((f + "-irrev", single(f, reversible=False)))
    return out


def types(m):
    """[elementary, three-body, Lindemann, Troe] counts"""
    return [int((m.itype == k).sum()) for k in range(4)]


def reacting(m):
    """mask [S]: the species takes part in a reaction"""
    on = np.zeros(m.S, bool)
    for r in range(m.R):
        on[_species_of(m, r)] = True
    return on


def inert_index(m):
    """the species the Y equation leaves out (any index will do for the chemistry): N2, or the last one below 9 species"""
    return m.species.index("N2") if "N2" in m.species else m.S - 1


# ---------------------------------------------------------------------------------------------------------- the sweep
SWEEP = {**{f"p{S}": ("prefix", S) for S in list(range(4, 13)) + [13, 16, 17, 32, 33]},
         "c63": ("cloned", 27, 11), "c64": ("cloned", 28, 11), "p12x58": ("dup", 12, 58)}
LARGE = ("p13", "p16", "p17", "p32", "p33", "c63", "c64")
_cases = {}


def case(name):
    if name not in _cases:
        k = SWEEP[name]
        _cases[name] = prefix(k[1]) if k[0] == "prefix" else cloned(k[1], k[2]) if k[0] == "cloned" else with_duplicates(prefix(k[1]), k[2])
    return _cases[name]


def _stable(species):
    return np.array([s[:-2] in STABLE if s.endswith("_b") else s in STABLE for s in species])


def sweep_candidates(mt, kind, n, seed):
    """n candidate states (T, p, rho, Y) of a kind: "broad" -- T uniform in 900..2500 K, p log-uniform in 0.1..32 atm, Y from
    gamma(0.5) draws with every species that is no stable molecule scaled by 1e-3, normalised, rho = p W / (R T) off by 2 %
    -- or the same with a random half of the species (never the largest) at exactly 0 ("zero") or at -1e-12 ("negative"),
    normalised again so that RR still sums to zero"""
    m, _, W, _ = mt
    rng = np.random.default_rng([seed, {"broad": 0, "zero": 1, "negative": 2}[kind]])
    T = rng.uniform(900.0, 2500.0, n)
    p = P_ATM * 10.0 ** rng.uniform(np.log10(0.1), np.log10(32.0), n)
    Y = rng.gamma(0.5, 1.0, (m.S, n)) + 1e-300
    Y[~_stable(m.species)] *= 1e-3
    Y /= Y.sum(axis=0)
    if kind != "broad":
        for c in range(n):
            others = np.delete(np.arange(m.S), int(np.argmax(Y[:, c])))
            Y[rng.choice(others, m.S // 2, replace=False), c] = 0.0 if kind == "zero" else -1e-12
        Y /= Y.sum(axis=0)                       # sum Y = 1 with the zeros and the negative entries in it
    Wm = 1.0 / (Y / W[:, None]).sum(axis=0)
    rho = p * Wm / (RU * T) * (1.0 + 0.02 * rng.standard_normal(n))
    return T, p, rho, Y


N_SINGLE = 256
PR_TARGETS = (1e-4, 1e-3, 0.3, 1.0, 3.0, 3e2, 1e3, 1e4)


def single_states(mt, seed=5):
    """256 states of a one-reaction mechanism: T log-uniform in 300..3000 K, p log-uniform in 0.01..100 atm, Y from gamma
    draws; cells 1..6 have one reactant or product at exactly 0 (each in turn), the last cell is pure inert.

    Those ranges do not reach every fall-off regime (O + CO (+M) stays below Pr = 60 at 300 K and 100 atm in pure CO2,
    Burke's H + O2 (+M) below 1), so cells 7..14 of a fall-off form have their pressure rescaled -- Pr is linear in p at
    fixed T and composition -- to Pr = PR_TARGETS, whatever pressure that takes."""
    m, _, W, _ = mt
    n = N_SINGLE
    rng = np.random.default_rng(seed)
    T = 10.0 ** rng.uniform(np.log10(300.0), np.log10(3000.0), n)
    p = P_ATM * 10.0 ** rng.uniform(-2.0, 2.0, n)
    Y = rng.gamma(0.5, 1.0, (m.S, n)) + 1e-300
    Y /= Y.sum(axis=0)
    sp = list(dict.fromkeys(_species_of(m, 0)))
    for c in range(1, 7):
        Y[sp[(c - 1) % len(sp)], c] = 0.0
    inert = int(np.flatnonzero(~reacting(m))[0])
    Y[:, n - 1] = 0.0
    Y[inert, n - 1] = 1.0
    if m.itype[0] >= 2:
        c = np.arange(7, 7 + len(PR_TARGETS))
        p[c] *= np.asarray(PR_TARGETS) / reduced_pressure(mt, T[c], p[c], None, Y[:, c])
    Wm = 1.0 / (Y / W[:, None]).sum(axis=0)
    rho = p * Wm / (RU * T) * (1.0 + 0.02 * rng.standard_normal(n))
    return T, p, rho, Y


def reduced_pressure(mt, T, p, rho, Y):
    """Pr = k0 [M] / kf of a one-reaction fall-off mechanism per state (fp64, chem_oracle's expressions)"""
    from chem_oracle import Kinetics
    m, nasa, W, _ = mt
    kin = Kinetics(m, nasa, W)
    out = np.zeros(T.size)
    for c in range(T.size):
        rc, y = kin.reactor_state(T[c], p[c], Y[:, c])
        kf, k0, _ = kin.rate_constants(T[c])
        out[c] = k0[0] * float(np.dot(m.eff[0], rc * y / W)) / kf[0]
    return out
