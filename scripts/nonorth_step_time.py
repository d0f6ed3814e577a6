#!/usr/bin/env python3
"""Step time of the headline workload under `laplacian corrected` beside the default scheme.

The bench.py headline state (128^3 box, Burke 9 species, ODE chemistry, the case's schemes), one context per arm:
orthogonal, corrected with p.n_nonorth = 0 and corrected with p.n_nonorth = 1. The box is axis-aligned, so the
correction is numerically nil; it costs what it costs. Per arm: warm-up steps, timed steps (median of the per-step HIP
events, dfmi_step_timer), then a few steps with dfmi_kernel_timer armed on the correction kernel, its gradient kernel
and k_les_nut's sibling k_u_grad; the correction kernel's algorithmic bytes per step and share of the 8 TB/s bound.
The arms alternate ROUNDS times. Writes one JSON document (argument: output path; default stdout)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepflame-dev_amd"))

KERNELS = ("k_nonorth_corr", "k_grad_cells", "k_u_grad", "k_nonorth_flux_face")


def corr_bytes(C, F, Bc, S, n_corr, n_nonorth):
    """k_nonorth_corr per time step: each gradient, diffusivity, k, w and |Sf| once, the source read and written; the
    hex walk's topology (4 B per cell, 9 per coupled slot) per launch. Launches: U (3 fields, two sources), the species
    in chunks of 4 then singly (rhoD, alpha, hai, the rows' rhs and diffAlphaD read and written), he, and p once per
    corrector pass (rhorAUf read, base read, source and the face flux correction written)."""
    face = F * 40.0 + Bc * 40.0
    topo = 4.0 * C + 9.0 * Bc
    u = C * (72.0 + 8.0 + 4 * 24.0) + face + topo
    he = C * (24.0 + 8.0 + 16.0) + face + topo
    y, launches, s0 = 0.0, 0, 0
    while s0 < S:
        n = 4 if S - s0 >= 4 else 1
        y += C * (n * (24.0 + 8.0 + 8.0 + 16.0) + 8.0 + 16.0) + face + topo
        launches += 1
        s0 += n
    p = C * (24.0 + 16.0) + face + (F + Bc) * 16.0 + topo
    npass = n_corr * (1 + n_nonorth)
    return u + he + y + npass * p, 2 + launches + npass


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
    from dfmi import case
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
    arms = {"orthogonal": (None, 0), "corrected": ("corrected", 0), "corrected+1": ("corrected", 1)}
    runs = {n: [] for n in arms}
    kern = {}
    for rnd in range(args.rounds):
        for name, (scheme, nno) in arms.items():
            sch = dict(bench.case_schemes())
            if scheme:
                sch["laplacian"] = scheme
            ctx = Context(0)
            case.setup_context(ctx, m, table, inert, 1e-6, schemes=sch)
            ctx.set_option("p.n_nonorth", nno)
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
            runs[name].append({"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                               "p_iters_last": ctx.solver_stats("p")[0]})
            if rnd == 0:
                ctx.kernel_timer(",".join(KERNELS))
                for _ in range(args.kernel_steps):
                    ctx.time_step(2)
                k = {kn: ctx.kernel_time(kn) for kn in KERNELS}
                ctx.kernel_timer("")
                kern[name] = {kn: {"launches_per_step": v[1] / args.kernel_steps,
                                   "us_per_launch": (1e3 * v[0] / v[1]) if v[1] else None,
                                   "us_per_step": 1e3 * v[0] / args.kernel_steps} for kn, v in k.items()}
                kern[name]["finite"] = bool(np.isfinite(ctx.get_field("T", (m.n_cells,))).all())
            ctx.close()
    doc = {"workload": f"{args.n}^3 headline state, Burke 9 species, ODE chemistry, case schemes; {args.steps} timed steps "
                       f"after {args.warmup}, {args.rounds} alternating rounds, one context per arm; kernel times on one "
                       "stream (dfmi_kernel_timer)",
           "step_ms": runs, "kernels_us": kern, "cells": m.n_cells, "faces": m.n_faces, "coupled_slots": Bc}
    for name, (scheme, nno) in arms.items():
        us = kern.get(name, {}).get("k_nonorth_corr", {}).get("us_per_step")
        if scheme and us:
            nb, nl = corr_bytes(m.n_cells, m.n_faces, Bc, table.S, 2, nno)
            doc.setdefault("k_nonorth_corr", {})[name] = {"algorithmic_bytes_per_step": nb, "launches_expected": nl,
                                                          "share_of_8TBs": nb / (us * 1e-6) / 8e12}
    txt = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
