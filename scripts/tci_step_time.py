#!/usr/bin/env python3
"""Step time of the headline workload with a PaSR or EDC combustion closure beside the kEpsilon step.

The bench.py headline state (128^3 box, Burke 9 species, ODE chemistry, the case's schemes) with the RAS state of
scripts/ras_step_time.py, one context per arm: kEpsilon alone, + PaSR with each chemistry scale (globalConvertion,
formationRate, reactionRate; globalScale mixing), + EDC v2005. Per arm: warm-up steps, timed steps (median of the per-step
HIP events), then a few steps with dfmi_kernel_timer armed on the closure's kernels and the integrator; k_tci_kappa's
algorithmic bytes and share of the 8 TB/s bound, k_tci_rates' counted flops and share of the FP64 vector peak; the integrator
under EDC's per-cell intervals beside the same state under the scalar dt; what kappa looks like (min / median / max). The arms
alternate ROUNDS times. Writes one JSON document (--out; default stdout)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepflame-dev_amd"))

KERNELS = ("k_tci_kappa", "k_tci_rates", "k_tci_scale", "k_chem", "k_ras_sources")
ARMS = {"kEpsilon": None, "PaSR globalConvertion": {"model": 1, "chemistry": 1}, "PaSR formationRate": {"model": 1, "chemistry": 2},
        "PaSR reactionRate": {"model": 1, "chemistry": 3}, "EDC v2005": {"model": 2, "version": 2005}}
FP64_PEAK = 78.6e12


def kappa_bytes(C, S, chemistry):
    """k_tci_kappa, PaSR, per cell: k, epsilon, mu, rho, Qdot and RR (S) in; tci_tc in for globalConvertion (t0) and
    reactionRate; Y of the four species (globalConvertion) or of all (formationRate); tci_tc, tci_tmix, tci_kappa, Qdot_eff
    and RR_eff (S) out"""
    y = {1: 4, 2: S, 3: 0}[chemistry]
    return C * 8.0 * (5 + S + (1 if chemistry != 2 else 0) + y + 4 + S)


def rates_flops(C, S, mech):
    """k_tci_rates per cell, counted from the source with a transcendental (exp, log, log10, exp10) as one operation:
    the state (5 S), the species' g / RT (36 S + 1), per reaction the Arrhenius constant (5), the equilibrium constant of a
    reversible one (12 + 4), the third-body sum (2 S) and fall-off factor (10; Troe 30 more), the two mass-action products
    (8), the weights and the four sums (10)"""
    n = 5 * S + 36 * S + 1
    for r in range(mech.R):
        n += 5 + 8 + 10
        if mech.reversible[r]:
            n += 16
        if mech.itype[r] != 0:
            n += 2 * S
        if mech.itype[r] >= 2:
            n += 15
        if mech.itype[r] == 3:
            n += 30
    return float(C) * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--kernel-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (loads the HIP runtime first, as bench.py does)
    import bench
    from dfmi import case, turbulence
    from dfmi.kinetics import parse_mechanism
    from dfmi.lib import Context
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    golden = os.path.join(ROOT, "tests", "golden")
    yml, tab = bench.MECHS["burke9"]
    ym = read_yaml_mechanism(os.path.join(golden, yml))
    species = ym["species"]
    table = read_thermo_table(os.path.join(golden, tab), species)
    inert = species.index("N2")
    m = bench.rank_block(args.n, bench.decomposition(1), 0)
    f = bench.reference_fields(m, species)
    mech = parse_mechanism(os.path.join(golden, yml))
    C, S = m.n_cells, table.S
    runs = {n: [] for n in ARMS}
    kern, kappa = {}, {}
    for rnd in range(args.rounds):
        for name, tci in ARMS.items():
            ctx = Context(0)
            case.setup_context(ctx, m, table, inert, 1e-6, schemes=bench.case_schemes())
            ctx.chem_set_mechanism(mech)
            ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
            case.init_state(ctx, m, table.S, f["T"], f["p"], f["U"], f["Y"])
            k0 = 1.5 * (0.05 * 4.0) ** 2          # u' = 5 % of the 4 m/s TGV velocity, a length scale of 0.1 mm
            e0 = 0.09 ** 0.75 * k0 ** 1.5 / 1e-4
            turbulence.apply_ras(ctx, m, dict(turbulence.RAS_DEFAULTS, ras_model=1),
                                 patch_types={"k": m.patch_types(0), "epsilon": m.patch_types(0)}, k=k0, epsilon=e0)
            if tci:
                ctx.set_option("tci.fuel", species.index("H2")); ctx.set_option("tci.oxidizer", species.index("O2"))
                ctx.set_option("tci.H2", species.index("H2"))
                for key, v in tci.items():
                    if key != "model":
                        ctx.set_option("tci." + key, v)
                ctx.set_option("tci.model", tci["model"])
            for _ in range(args.warmup):
                ctx.time_step(2)
            ctx.sync()
            ctx.step_timer(True)
            for _ in range(args.steps):
                ctx.time_step(2)
            ctx.sync()
            ms = ctx.step_times(args.steps)
            ctx.step_timer(False)
            runs[name].append({"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())})
            if rnd == 0:
                ctx.kernel_timer(",".join(KERNELS))
                for _ in range(args.kernel_steps):
                    ctx.time_step(2)
                kt = {kn: ctx.kernel_time(kn) for kn in KERNELS}
                ctx.kernel_timer("")
                kern[name] = {kn: {"launches": v[1], "us_per_launch": (1e3 * v[0] / v[1]) if v[1] else None} for kn, v in kt.items()}
                kern[name]["finite"] = bool(np.isfinite(ctx.get_field("T", (C,))).all())
                if tci:
                    kp = ctx.get_field("tci_kappa", (C,))
                    kappa[name] = {"min": float(kp.min()), "median": float(np.median(kp)), "max": float(kp.max())}
                    if tci["model"] == 2:
                        tau = ctx.get_field("tci_tauStar", (C,))
                        kappa[name]["tauStar"] = {"min": float(tau.min()), "median": float(np.median(tau)), "max": float(tau.max())}
                        kappa[name]["bad_tauStar"] = ctx.get_option("tci.bad_tauStar")
                        st = ctx.get_field("chem_stats", (3, C))
                        kappa[name]["integrator_steps_per_cell"] = float(st[0].mean())
                else:
                    kappa[name] = {"integrator_steps_per_cell": float(ctx.get_field("chem_stats", (3, C))[0].mean())}
            ctx.close()
    doc = {"workload": f"{args.n}^3 headline state, Burke 9 species, ODE chemistry, case schemes, kEpsilon (k = {k0:.3g}, epsilon = "
                       f"{e0:.3g}); {args.steps} timed steps after {args.warmup}, {args.rounds} alternating rounds, one context per arm",
           "step_ms": runs, "kernels_us": kern, "kappa": kappa, "cells": C, "species": S,
           "algorithmic_bytes": {"k_tci_kappa " + n: kappa_bytes(C, S, t["chemistry"]) for n, t in ARMS.items() if t and t["model"] == 1},
           "counted_flops": {"k_tci_rates": rates_flops(C, S, mech)}}
    for n, t in ARMS.items():
        us = kern.get(n, {}).get("k_tci_kappa", {}).get("us_per_launch")
        if t and t["model"] == 1 and us:
            doc.setdefault("share_of_8TBs", {})["k_tci_kappa " + n] = kappa_bytes(C, S, t["chemistry"]) / (us * 1e-6) / 8e12
    us = kern.get("PaSR reactionRate", {}).get("k_tci_rates", {}).get("us_per_launch")
    if us:
        doc["share_of_fp64_valu_peak"] = {"k_tci_rates": rates_flops(C, S, mech) / (us * 1e-6) / FP64_PEAK}
    txt = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
