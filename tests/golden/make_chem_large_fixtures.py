#!/usr/bin/env python3
"""Fixtures of the 13..64-species chemistry tests (tests/test_gpu_chem_large.py, tests/test_chem_large_fixtures.py):

  files   drm19.yaml (a copy of the reference's mechanisms/CH4/drm19.yaml; pass its directory as --reference),
          thermo_drm19.txt and thermo_gri30_36.txt (dfmi.transport_fit.fit_mechanism + write_thermo_table)
  states  chem_large_states.json: for DRM19 and the 36-species gri30.yaml, 48 states (T, p, rho, Y) built as
          _states of tests/test_gpu_chemistry.py builds them -- stoichiometric CH4/air unburnt, CO2/H2O/N2 burnt, a
          1e-3 radical pool, T in 300..2500 K, rho deliberately off p W / (R T) -- and the oracle's
          Kinetics.reaction_rates(..., dt = 1e-6) for them (SciPy BDF, rtol 1e-11 / atol 1e-22). The oracle also runs
          100x looser (1e-9 / 1e-20); a state is kept only where the two agree to a tenth of the tightest threshold
          of the GPU test (1e-5 of the global RR scale -> 1e-6; and 1e-4 of the floored per-species scale -> 1e-5).
          Candidates are drawn until 48 are kept; at most 10 % of the examined ones may be dropped.
  zerod   zeroD_drm19.json: a constant-pressure df0DFoam trajectory (oracle.zero_d_trajectory, as
          make_zero_d_fixture.py) of stoichiometric CH4/air, dt = 1e-6, from --T0 over --steps steps.

The oracle costs seconds per cell, so the states are spread over --jobs processes. make_chem_sweep_fixtures.py makes the
states of the species-count sweep the same way."""
import argparse
import json
import multiprocessing
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "deepflame-dev_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

MECHS = {"drm19": ("drm19.yaml", "thermo_drm19.txt"), "gri30": ("gri30.yaml", "thermo_gri30_36.txt")}
N_STATES, DT = 48, 1e-6
TIGHT = dict(rtol=1e-11, atol=1e-22)
LOOSE = dict(rtol=1e-9, atol=1e-20)
SEED = {"drm19": 0, "gri30": 0}


def states(ym, n, seed):
    """_states of tests/test_gpu_chemistry.py with the CH4/air compositions (T up to 2500 K)."""
    rng = np.random.default_rng(seed)
    from dfmi.case import ch4_air_compositions
    sp = ym["species"]
    yu, yb = ch4_air_compositions(sp)
    prog = rng.random(n)
    Y = (1 - prog) * yu[:, None] + prog * yb[:, None]
    Y = Y + rng.random((len(sp), n)) * 1e-3        # radical pool
    Y /= Y.sum(axis=0)
    T = 300.0 + 2200.0 * rng.random(n)
    Wm = 1.0 / (Y / np.asarray(ym["W"])[:, None]).sum(axis=0)
    p = 101325.0 * (1.0 + 0.05 * rng.standard_normal(n))
    rho = p * Wm / (8314.46261815324 * T) * (1.0 + 0.02 * rng.standard_normal(n))   # thermo rho != reactor rho
    return T, p, rho, Y


_KIN = {}


def _kin(name):
    if name not in _KIN:
        from dfmi.mech import read_yaml_mechanism
        from dfmi.kinetics import parse_mechanism
        from chem_oracle import Kinetics
        path = os.path.join(HERE, MECHS[name][0])
        ym = read_yaml_mechanism(path)
        _KIN[name] = Kinetics(parse_mechanism(path), ym["nasa"], ym["W"])
    return _KIN[name]


def _one(job):
    name, T, p, rho, Y, kw = job
    return _kin(name).reaction_rates(np.array([T]), np.array([p]), np.array([rho]), np.asarray(Y)[:, None], DT, **kw)[:, 0]


def make_files(reference):
    from dfmi.mech import read_yaml_mechanism, write_thermo_table
    from dfmi.transport_fit import fit_mechanism
    if reference:
        shutil.copyfile(os.path.join(reference, "drm19.yaml"), os.path.join(HERE, "drm19.yaml"))
        os.chmod(os.path.join(HERE, "drm19.yaml"), 0o644)
    for mech, table in MECHS.values():
        write_thermo_table(os.path.join(HERE, table), fit_mechanism(read_yaml_mechanism(os.path.join(HERE, mech))))
        print("wrote", table)


def make_states(jobs):
    from dfmi.mech import read_yaml_mechanism
    out = {"dt": DT, "oracle": "chem_oracle.Kinetics.reaction_rates, SciPy BDF rtol %g atol %g" % (TIGHT["rtol"], TIGHT["atol"]),
           "loose": "rtol %g atol %g; kept where |RR - RR_loose| <= 1e-6 of the global scale and <= 1e-5 of the floored "
                    "per-species scale" % (LOOSE["rtol"], LOOSE["atol"]),
           "mechanisms": {}}
    n_cand = N_STATES + N_STATES // 10 + 1
    with multiprocessing.Pool(jobs) as pool:
        for name, (mech, _) in MECHS.items():
            ym = read_yaml_mechanism(os.path.join(HERE, mech))
            T, p, rho, Y = states(ym, n_cand, SEED[name])
            work = [(name, T[c], p[c], rho[c], Y[:, c].tolist(), kw) for kw in (TIGHT, LOOSE) for c in range(n_cand)]
            res = pool.map(_one, work, chunksize=1)
            ref = np.array(res[:n_cand]).T
            loose = np.array(res[n_cand:]).T
            scale = np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1e-3 * np.abs(ref).max())
            d = np.abs(ref - loose)
            ok = (d.max(axis=0) <= 1e-6 * scale.max()) & ((d / scale).max(axis=0) <= 1e-5)
            keep = np.flatnonzero(ok)[:N_STATES]
            assert keep.size == N_STATES, f"{name}: only {keep.size} of {n_cand} candidates converged; change the seed"
            examined = int(keep[-1]) + 1
            dropped = examined - N_STATES
            assert dropped <= 0.1 * examined, f"{name}: {dropped} of {examined} dropped; change the seed"
            print(f"{name}: kept {N_STATES} of {examined} examined ({dropped} dropped), worst kept "
                  f"{d[:, keep].max() / scale.max():.2e} of the scale")
            out["mechanisms"][name] = {
                "mechanism": mech, "thermo": MECHS[name][1], "species": ym["species"], "seed": SEED[name],
                "examined": examined, "dropped": dropped, "kept": N_STATES,
                "T": T[keep].tolist(), "p": p[keep].tolist(), "rho": rho[keep].tolist(), "Y": Y[:, keep].tolist(),
                "RR": ref[:, keep].tolist()}
    with open(os.path.join(HERE, "chem_large_states.json"), "w") as f:
        json.dump(out, f)


def make_zerod(T0, n, rtol, atol, out_name):
    from dfmi.case import ch4_air_compositions
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    import oracle as O
    mech, table = MECHS["drm19"]
    ym = read_yaml_mechanism(os.path.join(HERE, mech))
    sp = ym["species"]
    t = read_thermo_table(os.path.join(HERE, table), sp)
    Y0, _ = ch4_air_compositions(sp)
    p0 = 101325.0
    T, Y = O.zero_d_trajectory(t, _kin("drm19"), T0, p0, Y0, DT, n, rtol=rtol, atol=atol, inert=sp.index("N2"))
    print(f"T: {T[0]:.2f} -> {T[-1]:.2f} K over {n} steps")
    out = {"source": "stoichiometric CH4/air, constant pressure (df0DFoam, constantProperty pressure); T0 and the step "
                     "count chosen so that T rises by more than 500 K inside the window",
           "mechanism": mech, "thermo": table, "species": sp, "T0": T0, "p": p0, "Y0": Y0.tolist(), "dt": DT, "n_steps": n,
           "oracle": "oracle.zero_d_trajectory, SciPy BDF rtol %g atol %g" % (rtol, atol), "T": T.tolist(), "Y": Y.tolist()}
    with open(os.path.join(HERE, out_name), "w") as f:
        json.dump(out, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["files", "states", "zerod", "all"])
    ap.add_argument("--reference", default=None, help="directory that holds the reference's drm19.yaml")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--T0", type=float, default=2000.0)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rtol", type=float, default=1e-14)
    ap.add_argument("--atol", type=float, default=1e-25)
    ap.add_argument("--out", default="zeroD_drm19.json")
    a = ap.parse_args()
    if a.what in ("files", "all"):
        make_files(a.reference)
    if a.what in ("states", "all"):
        make_states(a.jobs)
    if a.what in ("zerod", "all"):
        make_zerod(a.T0, a.steps, a.rtol, a.atol, a.out)


if __name__ == "__main__":
    main()
