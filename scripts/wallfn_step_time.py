#!/usr/bin/env python3
"""Step time of a k-epsilon step between wall-function walls beside one between zeroGradient walls.

A walled 128^3 box with the bench.py headline fields (Burke 9 species, ODE chemistry, the case's schemes, fixedValue U on the walls),
one context per arm: kEpsilon with zeroGradient k / epsilon and calculated nut on every wall, and kEpsilon with
epsilonWallFunction / nutkWallFunction on the y- and z-walls (kqRWallFunction k) and the two turbulent inlet
conditions on the x-walls. Per arm: warm-up steps, timed steps (median of
the per-step HIP events), then a few steps with dfmi_kernel_timer armed on the wall kernels and the scalar assembly. The
arms alternate ROUNDS times. Writes one JSON document (--out; default stdout)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepflame-dev_amd"))

KERNELS = ("k_ras_wall", "k_ras_nut_wall", "k_ras_inlet_ref", "k_scalar_assemble", "k_ras_production", "k_ras_nut")


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
    from dfmi.mesh import (hex_box, CALCULATED, EPSILON_WALL_FUNCTION, FIXED_VALUE, NUTK_WALL_FUNCTION, ZERO_GRADIENT,
                           TURBULENT_INTENSITY_K_INLET, TURBULENT_MIXING_LENGTH_EPSILON_INLET)
    golden = os.path.join(ROOT, "tests", "golden")
    yml, tab = bench.MECHS["burke9"]
    ym = read_yaml_mechanism(os.path.join(golden, yml))
    table = read_thermo_table(os.path.join(golden, tab), ym["species"])
    inert = ym["species"].index("N2")
    n = args.n
    L = 2 * np.pi * 1e-3
    m = hex_box(n, n, n, lengths=(L,) * 3, periodic=(False,) * 3)
    f = bench.reference_fields(m, ym["species"])
    mech = parse_mechanism(os.path.join(golden, yml))
    pt = case.default_patch_types(m)
    pt["U"] = m.patch_types(FIXED_VALUE)
    wall_slots = sum(p.size for p in m.patches if p.kind == "wall" and p.name not in ("left", "right"))
    wall_cells = n ** 3 - n * (n - 2) ** 2
    inlet_slots = sum(p.size for p in m.patches if p.name in ("left", "right"))
    arms = ("zeroGradient", "wallFunctions")
    runs = {a: [] for a in arms}
    kern, info = {}, {}
    k0 = 1.5 * (0.05 * 4.0) ** 2            # u' = 5 % of the 4 m/s TGV velocity, a length scale of 0.1 mm
    e0 = 0.09 ** 0.75 * k0 ** 1.5 / 1e-4
    for rnd in range(args.rounds):
        for name in arms:
            ctx = Context(0)
            case.setup_context(ctx, m, table, inert, 1e-6, pt, schemes=bench.case_schemes())
            ctx.chem_set_mechanism(mech)
            ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
            case.init_state(ctx, m, table.S, f["T"], f["p"], f["U"], f["Y"])
            types = {"k": m.patch_types(ZERO_GRADIENT), "epsilon": m.patch_types(ZERO_GRADIENT), "nut": m.patch_types(CALCULATED)}
            params = None
            if name == "wallFunctions":   # wall functions on the y- and z-walls, turbulent inlets on the two x-walls
                types["epsilon"] = m.patch_types(EPSILON_WALL_FUNCTION)
                types["nut"] = m.patch_types(NUTK_WALL_FUNCTION)
                params = {"k": {}, "epsilon": {}}
                for i, p in enumerate(m.patches):
                    if p.name in ("left", "right"):
                        types["k"][i], types["epsilon"][i], types["nut"][i] = TURBULENT_INTENSITY_K_INLET, TURBULENT_MIXING_LENGTH_EPSILON_INLET, CALCULATED
                        params["k"][i] = {"intensity": 0.05}
                        params["epsilon"][i] = {"mixingLength": 1e-4}
            turbulence.apply_ras(ctx, m, dict(turbulence.RAS_DEFAULTS, ras_model=1), patch_types=types, k=k0, epsilon=e0,
                                 patch_params=params)
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
                k = {kn: ctx.kernel_time(kn) for kn in KERNELS}
                ctx.kernel_timer("")
                kern[name] = {kn: {"launches": v[1], "us_per_launch": (1e3 * v[0] / v[1]) if v[1] else None} for kn, v in k.items()}
                kern[name]["us_per_step"] = {kn: 1e3 * v[0] / args.kernel_steps for kn, v in k.items()}
                info[name] = {"solver_iterations": {e: ctx.solver_stats(e)[0] for e in ("epsilon", "k")},
                              "finite": bool(np.isfinite(ctx.get_field("T", (m.n_cells,))).all())}
                if name == "wallFunctions":
                    yp = ctx.get_field("boundary_yPlus", (m.n_boundary_slots,))
                    yp = yp[yp > 0]
                    info[name]["yPlus_min_median_max"] = [float(yp.min()), float(np.median(yp)), float(yp.max())]
            ctx.close()
    doc = {"workload": f"walled {n}^3 box, headline fields, Burke 9 species, ODE chemistry, case schemes, fixedValue U on the walls; "
                       f"{args.steps} timed steps after {args.warmup}, {args.rounds} alternating rounds, one context per arm",
           "step_ms": runs, "kernels": kern, "info": info, "cells": m.n_cells, "wall_slots": wall_slots,
           "wall_cells": wall_cells, "inlet_slots": inlet_slots}
    w = kern.get("wallFunctions", {}).get("us_per_step")
    if w and runs["wallFunctions"]:
        step_us = 1e3 * float(np.median([r["median_ms"] for r in runs["wallFunctions"]]))
        doc["wall_kernels_share_of_step"] = (w["k_ras_wall"] + w["k_ras_nut_wall"] + w["k_ras_inlet_ref"]) / step_us
    txt = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
