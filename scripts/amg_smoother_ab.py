"""p-solve kernel time of the headline step with the weighted-Jacobi and the multicolour-DILU V-cycle smoother.

The headline case of bench.py (128^3 box, 9 species, ODE chemistry, 2 correctors) is set up through bench.py's own
helpers; after the warm-up steps the library's kernel timers (dfmi_kernel_timer: HIP events around every launch of
the named kernels) are armed over the p solve's kernels for a few steps. Prints one JSON line per smoother:
ms per step and launches per step of every kernel, their sum, and the p iterations per solve (dfmi_solver_work).
The timed steps carry two event records per launch, so their wall time is not the headline's: bench.py measures
that (DFMI_OPTIONS=amg.smoother=1 python bench.py).

usage: python scripts/amg_smoother_ab.py [--n 128] [--steps 5] [--out profiles/FILE.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deepflame-dev_amd")]

PCG = ("k_ell_build", "k_cg_init", "k_cg_spmv", "k_cg_x", "k_cg_x_smooth")
BUILD = ("k_round_f32", "k_galerkin", "k_dilu_factor")
JACOBI = ("k_smooth_res", "k_restrict", "k_prolong_smooth", "k_vtail", "k_coarsest")
DILU = ("k_dilu_fwd", "k_dilu_bwd", "k_dilu_res", "k_dilu_small")


def run(smoother, n, steps, warmup, ncorr):
    import numpy as np
    import bench
    from dfmi import case
    from dfmi.kinetics import parse_mechanism
    from dfmi.lib import Context, DEFAULT_OPTIONS
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    golden = os.path.join(ROOT, "tests", "golden")
    yml, tab = bench.MECHS["burke9"]
    ym = read_yaml_mechanism(os.path.join(golden, yml))
    table = read_thermo_table(os.path.join(golden, tab), ym["species"])
    m = bench.rank_block(n, bench.decomposition(1), 0)
    DEFAULT_OPTIONS["amg.smoother"] = smoother
    try:
        ctx = Context(0)
    finally:
        DEFAULT_OPTIONS.pop("amg.smoother", None)
    case.setup_context(ctx, m, table, ym["species"].index("N2"), 1e-6, schemes=bench.case_schemes())
    ctx.chem_set_mechanism(parse_mechanism(os.path.join(golden, yml)))
    ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
    f = bench.reference_fields(m, ym["species"])
    case.init_state(ctx, m, table.S, f["T"], f["p"], f["U"], f["Y"])
    for _ in range(warmup):
        ctx.time_step(ncorr)
    ctx.sync()
    names = PCG + BUILD + JACOBI + DILU
    ctx.solver_work("p", reset=True)
    ctx.kernel_timer(",".join(names))
    for _ in range(steps):
        ctx.time_step(ncorr)
    ctx.sync()
    t = {k: ctx.kernel_time(k) for k in names}
    ctx.kernel_timer("")
    iters = ctx.solver_work("p") / (steps * ncorr)
    stats = ctx.solver_stats("p")
    ctx.close()
    kern = {k: {"ms_per_step": v[0] / steps, "launches_per_step": v[1] / steps} for k, v in t.items() if v[1]}
    return {"smoother": "dilu" if smoother else "jacobi", "cells": m.n_cells, "steps": steps, "ncorr": ncorr,
            "p_iters_per_solve": iters, "last_p_solve": {"iters": stats[0], "rel": stats[2]},
            "p_kernel_ms_per_step": float(np.sum([v["ms_per_step"] for v in kern.values()])),
            "p_launches_per_step": float(np.sum([v["launches_per_step"] for v in kern.values()])), "kernels": kern}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncorr", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [json.dumps(run(s, a.n, a.steps, a.warmup, a.ncorr)) for s in (0, 1)]
    for l in lines:
        print(l, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
