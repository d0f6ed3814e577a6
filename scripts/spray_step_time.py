#!/usr/bin/env python3
"""Step time of the headline workload with the spray coupling off and on.

The bench.py headline state (128^3 box, Burke 9 species, ODE chemistry, the case's schemes), one context per arm:
  parent    the parent commit's library (--parent-lib; left out when not given), no spray option touched
  off       this tree, no spray option or field touched (what every spray-free case runs)
  explicit  this tree, spray.model = 1, explicit schemes, sources non-zero in 10 % of the cells
  semi      the same under the semiImplicit schemes
  zero      spray.model = 1, semiImplicit schemes, every transfer field zero: the state evolves as in `off`, so the
            difference to `off` is the cost of the fold itself (the other two arms also pay for what the sources do to
            the state: more chemistry sub-steps and solver iterations)
Setting the five fields (what an adapter does once per step, outside the timed steps here) is timed on the host.
Per arm: warm-up steps, then timed steps (median of the per-step HIP events, dfmi_step_timer). The arms alternate
ROUNDS times (parent, off, off, parent, ...: alternating pairs). Writes one JSON document (--out; default stdout)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepflame-dev_amd"))


def sources(m, S, seed=11, frac=0.1):
    """per-step transfers of a cloud at 1e-5 of the cell mass (tests/spray_reference.py sources), in `frac` of the cells"""
    rng = np.random.default_rng(seed)
    C = m.n_cells
    mass = np.asarray(m.volume) * 1.0
    hit = rng.random(C) < frac
    return {"parcel_rhoTrans": np.where(hit, mass * 1e-5 * rng.standard_normal((S, C)), 0.0),
            "parcel_UTrans": np.where(hit, mass * 1e-2 * rng.standard_normal((3, C)), 0.0),
            "parcel_UCoeff": np.where(hit, mass * 1e-2 * rng.random(C), 0.0),
            "parcel_hsTrans": np.where(hit, mass * 1e3 * rng.standard_normal(C), 0.0),
            "parcel_hsCoeffByCp": np.where(hit, mass * 1e-2 * rng.standard_normal(C), 0.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
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
    src = {k: np.ascontiguousarray(v) for k, v in sources(m, table.S).items()}
    set_ms = []
    arms = (["parent"] if args.parent_lib else []) + ["off", "explicit", "semi", "zero"]
    runs = {a: [] for a in arms}
    launches = {}
    for rnd in range(args.rounds):
        for arm in (arms if rnd % 2 == 0 else arms[::-1]):
            ctx = Context(0, lib_path=args.parent_lib) if arm == "parent" else Context(0)
            case.setup_context(ctx, m, table, inert, 1e-6, schemes=bench.case_schemes())
            ctx.chem_set_mechanism(mech)
            ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
            case.init_state(ctx, m, table.S, f["T"], f["p"], f["U"], f["Y"])
            if arm in ("explicit", "semi", "zero"):
                ctx.sync()
                t0 = time.perf_counter()
                for k, v in src.items():
                    ctx.set_field(k, np.zeros_like(v) if arm == "zero" else v)
                set_ms.append(1e3 * (time.perf_counter() - t0))   # host: the finiteness scan, then the copy, per field
                for k in ("rho", "U", "Yi", "h"):
                    ctx.set_option("spray." + k, 0 if arm == "explicit" else 1)
                ctx.set_option("spray.model", 1)
            for _ in range(args.warmup):
                ctx.time_step(2)
            ctx.sync()
            ctx.step_timer(True)
            for _ in range(args.steps):
                ctx.time_step(2)
            ctx.sync()
            ms = ctx.step_times(args.steps)
            ctx.step_timer(False)
            runs[arm].append({"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                              "last_step_iters": {e: int(ctx.solver_stats(e)[0]) for e in ("U", "Y", "E", "p")}})
            if rnd == 0 and arm != "parent":
                names = "k_rho,k_rho_spray,k_spray_u,k_spray_y,k_spray_e"
                ctx.kernel_timer(names)
                ctx.time_step(2)
                k = {n: ctx.kernel_time(n) for n in names.split(",")}
                ctx.kernel_timer("")
                launches[arm] = {n: {"launches": v[1], "us_per_launch": (1e3 * v[0] / v[1]) if v[1] else None} for n, v in k.items()}
                launches[arm]["finite"] = bool(np.isfinite(ctx.get_field("T", (m.n_cells,))).all())
            ctx.close()
    med = {a: [r["median_ms"] for r in runs[a]] for a in arms}
    doc = {"workload": f"{args.n}^3 headline state, Burke 9 species, ODE chemistry, case schemes; {args.steps} timed steps after "
                       f"{args.warmup}, {args.rounds} alternating rounds, one context per arm; sources in 10 % of the cells",
           "cells": m.n_cells, "step_ms": runs, "set_five_fields_host_ms": set_ms, "kernels_one_step": launches,
           "median_of_medians_ms": {a: float(np.median(v)) for a, v in med.items()},
           "spread_ms": {a: float(max(v) - min(v)) for a, v in med.items()}}
    if "parent" in med:
        d = doc["median_of_medians_ms"]["off"] - doc["median_of_medians_ms"]["parent"]
        doc["off_minus_parent_ms"] = d
        doc["inside_parent_spread"] = bool(abs(d) <= doc["spread_ms"]["parent"])
    doc["fold_cost_ms"] = doc["median_of_medians_ms"]["zero"] - doc["median_of_medians_ms"]["off"]
    txt = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
