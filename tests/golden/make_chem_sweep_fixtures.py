#!/usr/bin/env python3
"""Fixture of the chemistry sweep (tests/test_gpu_chem_sweep.py, tests/test_chem_sweep_cpu.py): chem_sweep_states.json.

  cases    for every mechanism of chem_mechs.SWEEP -- prefix(S) at S = 4..12, 13, 16, 17, 32, 33, the 63- and 64-species
           clones and prefix(12) with duplicates up to 58 reactions -- 16 states (4 for the last): 12 "broad" ones
           (chem_mechs.sweep_candidates: T 900..2500 K, p log-uniform in 0.1..32 atm, so that the fall-off reactions
           cross their regimes), 2 with half the species at exactly 0 and 2 with half of them at -1e-12 (the clip of
           setState_TPY), and the oracle's Kinetics.reaction_rates(..., dt = 1e-6) for them. As
           make_chem_large_fixtures.py: SciPy BDF at rtol 1e-11 / atol 1e-22 and again 100x looser; a state is kept where
           the two agree to 1e-6 of the global RR scale and 1e-5 of the floored per-species scale; at most 10 % of the
           examined candidates of a mechanism may be dropped.
  bounds   the maximum relative error of tci_reference.tc_reaction in fp64 against long double: per case over its
           states, and per one-reaction mechanism of chem_mechs.single_variants() over its 256 chem_mechs.single_states
           (for which it also asserts that every fall-off form has cells with Pr < 1e-2, 0.1 < Pr < 10 and Pr > 1e2).
           The GPU test holds the device to 4x these figures, floored at 1e-13.

The oracle costs seconds per cell at 32 species and more, so the states are spread over --jobs processes."""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import chem_mechs as cm          # noqa: E402  (also puts the package and the oracle on the path)
import tci_reference as R        # noqa: E402

DT = 1e-6
TIGHT = dict(rtol=1e-11, atol=1e-22)
LOOSE = dict(rtol=1e-9, atol=1e-20)
SEED = {name: 0 for name in cm.SWEEP}
KINDS = (("broad", 12, 14), ("zero", 2, 3), ("negative", 2, 3))        # kind, kept, candidates
KINDS_DUP = (("broad", 4, 5),)
OUT = os.path.join(HERE, "chem_sweep_states.json")


def kinds_of(name):
    return KINDS_DUP if cm.SWEEP[name][0] == "dup" else KINDS


def reference_rr(name, T, p, rho, Y, **kw):
    """the oracle's RR [S] of one state of a sweep case (tight tolerances unless given)"""
    from chem_oracle import Kinetics
    m, nasa, W, _ = cm.case(name)
    kw = kw or TIGHT
    return Kinetics(m, nasa, W).reaction_rates(np.array([T]), np.array([p]), np.array([rho]), np.asarray(Y, dtype=np.float64)[:, None], DT, **kw)[:, 0]


def _one(job):
    name, T, p, rho, Y, kw = job
    return reference_rr(name, T, p, rho, Y, **kw)


def tc_error(mt, T, p, rho, Y):
    """max relative error of the fp64 reactionRate scale against the long-double one"""
    m, nasa, W, _ = mt
    a = R.tc_reaction(m, nasa, W, T, p, rho, Y)
    b = R.tc_reaction(m, nasa, W, T, p, rho, Y, T=R.LD)
    e = R.rel_error(a, b)
    assert np.all(np.isfinite(e))
    return float(e.max())


def make_case(name, pool):
    mt = cm.case(name)
    m = mt[0]
    cand, work = [], []
    for kind, keep, n in kinds_of(name):
        T, p, rho, Y = cm.sweep_candidates(mt, kind, n, SEED[name])
        cand.append((kind, keep, T, p, rho, Y))
        work += [(name, T[c], p[c], rho[c], Y[:, c].tolist(), kw) for kw in (TIGHT, LOOSE) for c in range(n)]
    res = pool.map(_one, work, chunksize=1)
    ref_all, loose_all, o = [], [], 0
    for kind, keep, T, *_ in cand:
        n = T.size
        ref_all.append(np.array(res[o:o + n]).T); loose_all.append(np.array(res[o + n:o + 2 * n]).T)
        o += 2 * n
    ref = np.concatenate(ref_all, axis=1)
    scale = np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1e-3 * np.abs(ref).max())
    out = {k: [] for k in ("T", "p", "rho", "Y", "RR", "kind")}
    examined = kept = 0
    worst = 0.0
    for (kind, keep, T, p, rho, Y), rr, lo in zip(cand, ref_all, loose_all):
        d = np.abs(rr - lo)
        ok = np.all(np.isfinite(rr), axis=0) & (d.max(axis=0) <= 1e-6 * scale.max()) & ((d / scale).max(axis=0) <= 1e-5)
        k = np.flatnonzero(ok)[:keep]
        assert k.size == keep, f"{name} {kind}: only {k.size} of {T.size} candidates converged; change the seed"
        examined += int(k[-1]) + 1
        kept += keep
        worst = max(worst, float(d[:, k].max() / scale.max()))
        out["T"] += T[k].tolist(); out["p"] += p[k].tolist(); out["rho"] += rho[k].tolist()
        out["Y"].append(Y[:, k]); out["RR"].append(rr[:, k]); out["kind"] += [kind] * keep
    dropped = examined - kept
    assert dropped <= 0.1 * examined, f"{name}: {dropped} of {examined} dropped; change the seed"
    Y = np.concatenate(out["Y"], axis=1); RR = np.concatenate(out["RR"], axis=1)
    err = tc_error(mt, np.asarray(out["T"]), np.asarray(out["p"]), np.asarray(out["rho"]), Y)
    print(f"{name}: S {m.S} R {m.R}, kept {kept} of {examined} examined, worst kept {worst:.2e} of the scale, "
          f"tc fp64 error {err:.2e}", flush=True)
    return {"S": m.S, "R": m.R, "species": list(m.species), "seed": SEED[name], "examined": examined, "dropped": dropped,
            "kept": kept, "worst_kept": worst, "kind": out["kind"], "T": out["T"], "p": out["p"], "rho": out["rho"],
            "Y": Y.tolist(), "RR": RR.tolist(), "tc_fp64_error": err}


def make_singles():
    out = {}
    for key, mt in cm.single_variants():
        st = cm.single_states(mt)
        rec = {"equation": cm.FORMS[key.split("-")[0]][1], "species": list(mt[0].species), "tc_fp64_error": tc_error(mt, *st)}
        if key.split("-")[0] in cm.FALLOFF_FORMS:
            Pr = cm.reduced_pressure(mt, *st)
            rec["Pr_cells"] = [int((Pr < 1e-2).sum()), int(((Pr > 0.1) & (Pr < 10)).sum()), int((Pr > 1e2).sum())]
            assert min(rec["Pr_cells"]) > 0, (key, rec["Pr_cells"])
        print(key, rec, flush=True)
        out[key] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--only", nargs="*", default=None, help="regenerate these cases only (the others are kept from the file)")
    a = ap.parse_args()
    doc = json.load(open(OUT)) if a.only and os.path.exists(OUT) else {"cases": {}}
    doc.update({"dt": DT, "oracle": "chem_oracle.Kinetics.reaction_rates, SciPy BDF rtol %g atol %g" % (TIGHT["rtol"], TIGHT["atol"]),
                "loose": "rtol %g atol %g; kept where |RR - RR_loose| <= 1e-6 of the global scale and <= 1e-5 of the floored "
                         "per-species scale" % (LOOSE["rtol"], LOOSE["atol"]),
                "tc_fp64_error": "max relative error of tci_reference.tc_reaction in fp64 against long double"})
    doc["singles"] = make_singles()
    with multiprocessing.Pool(a.jobs) as pool:
        for name in (a.only or list(cm.SWEEP)):
            doc["cases"][name] = make_case(name, pool)
            with open(OUT, "w") as f:
                json.dump(doc, f)
                f.write("\n")


if __name__ == "__main__":
    main()
