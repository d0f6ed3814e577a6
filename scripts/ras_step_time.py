#!/usr/bin/env python3
"""Step time of the headline workload in RAS k-epsilon mode beside the laminar and the Smagorinsky step.

The bench.py headline state (128^3 box, Burke 9 species, ODE chemistry, the case's schemes), one context per arm:
laminar, Smagorinsky (les.model = 1), kEpsilon (ras.model = 1; uniform k and epsilon of a few per cent turbulence
intensity, upwind convection). Per arm: warm-up steps, timed steps (median of the per-step HIP events), then a few steps
with dfmi_kernel_timer armed on the RAS kernels; their algorithmic bytes and share of the 8 TB/s bound; the iteration
counts of the epsilon and k solves at the production tolerance. The arms alternate ROUNDS times. Writes one JSON document
(--out; default stdout)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deepflame-dev_amd"))

KERNELS = ("k_ras_production", "k_scalar_assemble", "k_ras_sources", "k_ras_bound", "k_ras_nut", "k_les_nut", "k_e_assemble")


def production_bytes(C, F, Bc):
    """k_ras_production on the hex walk: U (3), rho, nut, V in, G and divU out per cell; w, Sf (3) and phi per face; bw,
    bSf, bphi per coupled slot; the slot ranges (k_les_nut's count plus rho, nut, phi and one more output)"""
    return C * (24.0 + 8.0 + 8.0 + 8.0 + 16.0) + F * (32.0 + 8.0) + Bc * 40.0 + 4.0 * C + 9.0 * Bc


def assemble_bytes(C, F, Bc):
    """k_scalar_assemble on the hex walk: psi, rho, rho_old, D, Su, Sp, V in, diag and source out per cell; phi, w, dc,
    |Sf| in and lower, upper out per face; per coupled slot bphi, bw, bdc, |bSf| in and two coefficients out"""
    return C * (7 * 8.0 + 16.0) + F * (32.0 + 16.0) + Bc * 48.0 + 4.0 * C + 9.0 * Bc


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
    arms = ("laminar", "Smagorinsky", "kEpsilon")
    runs = {n: [] for n in arms}
    kern, iters = {}, {}
    for rnd in range(args.rounds):
        for name in arms:
            turb = dict(turbulence.DEFAULTS, model=1) if name == "Smagorinsky" else None
            ctx = Context(0)
            case.setup_context(ctx, m, table, inert, 1e-6, schemes=bench.case_schemes(), turbulence=turb)
            ctx.chem_set_mechanism(mech)
            ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
            case.init_state(ctx, m, table.S, f["T"], f["p"], f["U"], f["Y"])
            if name == "kEpsilon":   # u' = 5 % of the 4 m/s TGV velocity, a length scale of 0.1 mm
                k0 = 1.5 * (0.05 * 4.0) ** 2
                e0 = 0.09 ** 0.75 * k0 ** 1.5 / 1e-4
                turbulence.apply_ras(ctx, m, dict(turbulence.RAS_DEFAULTS, ras_model=1),
                                     patch_types={"k": m.patch_types(0), "epsilon": m.patch_types(0)}, k=k0, epsilon=e0)
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
                if name == "kEpsilon":
                    iters = {e: ctx.solver_stats(e)[0] for e in ("epsilon", "k")}
                    nut, mu, rho = (ctx.get_field(n, (m.n_cells,)) for n in ("nut", "mu", "rho"))
                    kern[name]["mut_over_mu_max"] = float((rho * nut / mu).max())
                    kern[name]["finite"] = bool(np.isfinite(ctx.get_field("T", (m.n_cells,))).all())
            ctx.close()
    pb, ab = production_bytes(m.n_cells, m.n_faces, Bc), assemble_bytes(m.n_cells, m.n_faces, Bc)
    doc = {"workload": f"{args.n}^3 headline state, Burke 9 species, ODE chemistry, case schemes; {args.steps} timed steps "
                       f"after {args.warmup}, {args.rounds} alternating rounds, one context per arm",
           "step_ms": runs, "kernels_us": kern, "solver_iterations": iters,
           "algorithmic_bytes": {"k_ras_production": pb, "k_scalar_assemble": ab},
           "cells": m.n_cells, "faces": m.n_faces, "coupled_slots": Bc}
    for kn, nb in (("k_ras_production", pb), ("k_scalar_assemble", ab)):
        us = kern.get("kEpsilon", {}).get(kn, {}).get("us_per_launch")
        if us:
            doc.setdefault("share_of_8TBs", {})[kn] = nb / (us * 1e-6) / 8e12
    txt = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
