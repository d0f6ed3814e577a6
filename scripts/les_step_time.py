#!/usr/bin/env python3
"""Step time of the headline workload in LES mode beside the laminar step.

The bench.py headline state (128^3 box, Burke 9 species, ODE chemistry, the case's schemes), one context per arm:
les.model = 0 (laminar), 1 (Smagorinsky), 2 (WALE), 4 (Sigma: k_les_sigma), 5 (dynamicSmagorinsky: k_dyn_strain, k_dyn_filter,
k_dyn_nut); delta = cubeRootVol. Per arm: warm-up steps, timed steps (median
of the per-step HIP events, dfmi_step_timer), then a few steps with dfmi_kernel_timer armed on the eddy-viscosity
kernel and the YEqn preparation, and the kernel's algorithmic bytes and share of the 8 TB/s bound. The arms alternate
ROUNDS times. Writes one JSON document (argument: output path; default stdout)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepflame-dev_amd"))


def nut_bytes(C, F, Bc, hex_walk):
    """k_les_nut: U (3), delta, V in, nut out per cell; w and Sf per face, bw and bSf per coupled slot; the gather
    topology k_u_grad counts (bench.py algorithmic_bytes)"""
    topo = (4.0 * C + 9.0 * Bc) if hex_walk else (12.0 * C + 12.0 * F + 9.0 * Bc)
    return C * (24.0 + 16.0 + 8.0) + F * 32.0 + Bc * 32.0 + topo


def dyn_bytes(C, F, Bc, hex_walk):
    """the three dynamicSmagorinsky passes, each input and output once. strain: k_les_nut's gather without delta, S (6)
    out; filter: U (3), S (6), delta in and the two contractions out per cell, w and |Sf| per face and coupled slot;
    nut: the two contractions, S (6), delta, mu, rho in and LM, MM, Cs, nut out per cell, w and |Sf| per face"""
    topo = (4.0 * C + 9.0 * Bc) if hex_walk else (12.0 * C + 12.0 * F + 9.0 * Bc)
    return {"k_dyn_strain": C * (24.0 + 8.0 + 48.0) + F * 32.0 + Bc * 32.0 + topo,
            "k_dyn_filter": C * (72.0 + 8.0 + 16.0) + F * 16.0 + Bc * 16.0 + topo,
            "k_dyn_nut": C * (16.0 + 48.0 + 24.0 + 32.0) + F * 16.0 + Bc * 16.0 + topo}


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
    table = read_thermo_table(os.path.join(golden, tab), ym["species"])
    inert = ym["species"].index("N2")
    m = bench.rank_block(args.n, bench.decomposition(1), 0)
    f = bench.reference_fields(m, ym["species"])
    mech = parse_mechanism(os.path.join(golden, yml))
    Bc = sum(p.size for p in m.patches if p.kind in ("cyclic", "processor", "processorCyclic"))
    names = {0: "laminar", 1: "Smagorinsky", 2: "WALE", 4: "Sigma", 5: "dynamicSmagorinsky"}
    runs = {n: [] for n in names.values()}
    kern = {}
    for rnd in range(args.rounds):
        for model, name in names.items():
            les = dict(turbulence.DEFAULTS, model=model)
            ctx = Context(0)
            case.setup_context(ctx, m, table, inert, 1e-6, schemes=bench.case_schemes(), turbulence=les)
            ctx.chem_set_mechanism(mech)
            ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
            case.init_state(ctx, m, table.S, f["T"], f["p"], f["U"], f["Y"])
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
                ctx.kernel_timer("k_les_nut,k_les_sigma,k_dyn_strain,k_dyn_filter,k_dyn_nut,k_y_prep,k_les_effective,k_u_grad")
                for _ in range(args.kernel_steps):
                    ctx.time_step(2)
                k = {kn: ctx.kernel_time(kn) for kn in ("k_les_nut", "k_les_sigma", "k_dyn_strain", "k_dyn_filter", "k_dyn_nut", "k_y_prep",
                                                         "k_les_effective", "k_u_grad")}
                ctx.kernel_timer("")
                kern[name] = {kn: {"launches": v[1], "us_per_launch": (1e3 * v[0] / v[1]) if v[1] else None} for kn, v in k.items()}
                if model:
                    nut = ctx.get_field("nut", (m.n_cells,))
                    mu = ctx.get_field("mu", (m.n_cells,))
                    rho = ctx.get_field("rho", (m.n_cells,))
                    kern[name]["nut_max"] = float(nut.max())
                    kern[name]["nut_min"] = float(nut.min())
                    kern[name]["mut_over_mu_max"] = float((rho * nut / mu).max())
                    kern[name]["finite"] = bool(np.isfinite(ctx.get_field("T", (m.n_cells,))).all())
            ctx.close()
    hexw = True
    nb = nut_bytes(m.n_cells, m.n_faces, Bc, hexw)
    doc = {"workload": f"{args.n}^3 headline state, Burke 9 species, ODE chemistry, case schemes; {args.steps} timed steps "
                       f"after {args.warmup}, {args.rounds} alternating rounds, one context per arm",
           "step_ms": runs, "kernels_us": kern,
           "k_les_nut_algorithmic_bytes": nb, "cells": m.n_cells, "faces": m.n_faces, "coupled_slots": Bc}
    # k_les_sigma moves k_les_nut's bytes: the same gather, one coefficient fewer
    for name, kn in (("Smagorinsky", "k_les_nut"), ("WALE", "k_les_nut"), ("Sigma", "k_les_sigma")):
        us = kern.get(name, {}).get(kn, {}).get("us_per_launch")
        if us:
            doc.setdefault(kn + "_share_of_8TBs", {})[name] = nb / (us * 1e-6) / 8e12
    db = dyn_bytes(m.n_cells, m.n_faces, Bc, hexw)
    doc["k_dyn_algorithmic_bytes"] = db
    for kn, b in db.items():
        us = kern.get("dynamicSmagorinsky", {}).get(kn, {}).get("us_per_launch")
        if us:
            doc.setdefault("k_dyn_share_of_8TBs", {})[kn] = b / (us * 1e-6) / 8e12
    txt = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
