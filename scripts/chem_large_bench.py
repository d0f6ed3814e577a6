#!/usr/bin/env python3
"""k_chem on large mechanisms: DRM19 (21 / 84) and the 36-species gri30 (36 / 219) on an N^3 box (default 64) with the
fixture-style state mix (tests/golden/make_chem_large_fixtures.py: states), for each lanes-per-cell variant of the
cooperative kernel (option chem.coop_lanes); beside them Burke-9 with chem.coop 0 and 1.

Per variant and repetition: chem_stats zeroed, one solve (natural order, first step = dt), then the timed solve (cost
binned by the first one's step counts, first step carried over -- the state a running case is in). The repetitions
loop outside the variants, so the variants alternate. k_chem milliseconds come from dfmi_kernel_timer (device events
around the launch). Writes profiles/chem_coop.json (or --out); progress goes to stdout.

    python scripts/chem_large_bench.py [--box 64] [--reps 3] [--out profiles/chem_coop.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "deepflame-dev_amd"))
sys.path.insert(0, GOLDEN)


def h2_states(ym, n, seed=0):
    from dfmi.case import h2_air_compositions
    rng = np.random.default_rng(seed)
    yu, yb = h2_air_compositions(ym["species"])
    prog = rng.random(n)
    Y = (1 - prog) * yu[:, None] + prog * yb[:, None] + rng.random((len(ym["species"]), n)) * 1e-3
    Y /= Y.sum(axis=0)
    T = 300.0 + 2200.0 * rng.random(n)
    Wm = 1.0 / (Y / ym["W"][:, None]).sum(axis=0)
    p = 101325.0 * (1.0 + 0.05 * rng.standard_normal(n))
    rho = p * Wm / (8314.46261815324 * T) * (1.0 + 0.02 * rng.standard_normal(n))
    return T, p, rho, Y


def run_case(name, mech_file, table_file, states, variants, box, reps, dt=1e-6):
    from dfmi.mesh import hex_box
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi.kinetics import parse_mechanism
    from dfmi.lib import Context, DfmiError
    from dfmi import case
    ym = read_yaml_mechanism(os.path.join(GOLDEN, mech_file))
    t = read_thermo_table(os.path.join(GOLDEN, table_file), ym["species"])
    mech = parse_mechanism(os.path.join(GOLDEN, mech_file))
    m = hex_box(box, box, box)
    C = m.n_cells
    ctx = Context(0)
    case.setup_context(ctx, m, t, ym["species"].index("N2"), dt)
    ctx.chem_set_mechanism(mech)
    T, p, rho, Y = states(ym, C)
    ctx.set_field("T", T); ctx.set_field("p", p); ctx.set_field("rho", rho); ctx.set_field("Y", Y)
    ctx.chem_set_options(1)
    out = {"species": mech.S, "reactions": mech.R, "cells": C, "dt": dt, "rtol": 1e-6, "atol": 1e-10, "variants": {}}
    rr0 = None
    for rep in range(reps):
        for label, opts in variants.items():
            rec = out["variants"].setdefault(label, {"options": opts, "k_chem_ms": []})
            if "error" in rec:
                continue
            for k, v in opts.items():
                ctx.set_option(k, v)
            try:
                ctx.set_field("chem_stats", np.zeros((3, C)))
                ctx.chem_solve(dt)
                ctx.kernel_timer("k_chem")
                ctx.chem_solve(dt)
                ms, launches = ctx.kernel_time("k_chem")
            except DfmiError as e:
                rec["error"] = str(e)
                print(f"{name} {label}: {e}", flush=True)
                continue
            assert launches == 1
            rec["k_chem_ms"].append(ms)
            if rep == 0:
                st = ctx.get_field("chem_stats", (3, C))
                cost = st[0] + st[1]
                rec.update(kernel=ctx.chem_info(), steps_mean=float(cost.mean()), steps_max=float(cost.max()))
                rr = ctx.get_field("RR", (mech.S, C))
                if rr0 is None:
                    rr0 = rr
                rec["max_rr_diff_vs_first_variant"] = float(np.abs(rr - rr0).max() / np.abs(rr0).max())
            print(f"{name} {label} rep {rep}: k_chem {ms:.3f} ms", flush=True)
    for rec in out["variants"].values():
        if rec["k_chem_ms"]:
            med = float(np.median(rec["k_chem_ms"]))
            rec["k_chem_ms_median"] = med
            rec["chem_integrations_per_s"] = C / (med * 1e-3)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--box", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chem_coop.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "chem_large_bench.py measures on the GPU"
    from make_chem_large_fixtures import states as ch4_states
    lanes = {f"coop_lanes_{tg}": {"chem.coop_lanes": tg} for tg in (16, 32, 64)}
    res = {"device": torch.cuda.get_device_name(0), "box": a.box, "reps": a.reps,
           "method": "per repetition and variant: chem_stats zeroed, one untimed solve, then the timed solve (binned by "
                     "the first one's step counts, chem.binning = 2); k_chem ms from dfmi_kernel_timer; variants alternate",
           "cases": {}}
    cases = [
        ("drm19", "drm19.yaml", "thermo_drm19.txt", lambda ym, n: ch4_states(ym, n, 0), lanes),
        ("gri30", "gri30.yaml", "thermo_gri30_36.txt", lambda ym, n: ch4_states(ym, n, 0), lanes),
        ("burke9", "Burke2012_s9r23.yaml", "thermo_Burke2012_s9r23.txt", h2_states,
         {"coop_0": {"chem.coop": 0}, **{f"coop_1_lanes_{tg}": {"chem.coop": 1, "chem.coop_lanes": tg} for tg in (16, 32, 64)}}),
    ]
    for name, mech, table, st, variants in cases:
        res["cases"][name] = run_case(name, mech, table, st, variants, a.box, a.reps)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:          # after every case: a partial file survives an interrupted run
            json.dump(res, f, indent=1)
    print(json.dumps({k: {v: r.get("k_chem_ms_median") for v, r in c["variants"].items()} for k, c in res["cases"].items()}))


if __name__ == "__main__":
    main()
