"""Adjustable time step: the first two lines of dfLowMachFoam's time loop (dfLowMachFoam.C:261-262,
#include "compressibleCourantNo.H" and #include "setDeltaT.H") on the host side of the C ABI.

The Courant number itself is computed on the device (include/dfmi.h dfmi_courant_no); this module holds the
controlDict entries that steer the step (readTimeControls.H), OpenFOAM-7's two step-size rules
(setInitialDeltaT.H, setDeltaT.H) restated, and a small loop in the reference's order.

Out of scope: Time::adjustDeltaT, which snaps the step so that write times are hit exactly. The step
returned here is the one setDeltaT.H computes before that adjustment; nothing here writes time directories.
"""
from __future__ import annotations

import math

from .schemes import dict_entries

SMALL = 1e-15   # OpenFOAM's small (double precision)
_SWITCH = {"yes": True, "on": True, "true": True, "no": False, "off": False, "false": False}


def parse_control_dict(txt: str) -> dict:
    """deltaT, adjustTimeStep, maxCo, maxDeltaT from controlDict text. The last entry of a keyword wins, as in
    OpenFOAM's dictionary reading; maxCo defaults to 1 and maxDeltaT to +inf (readTimeControls.H), adjustTimeStep
    to off. deltaT has no default."""
    last = dict(dict_entries(txt))   # later pairs overwrite earlier ones
    if "deltaT" not in last:
        raise ValueError("controlDict: no deltaT entry")
    sw = last.get("adjustTimeStep", "no")
    if sw not in _SWITCH:
        raise ValueError(f"controlDict: adjustTimeStep {sw!r} is not one of {sorted(_SWITCH)}")
    return {"deltaT": float(last["deltaT"]), "adjustTimeStep": _SWITCH[sw],
            "maxCo": float(last.get("maxCo", 1.0)), "maxDeltaT": float(last.get("maxDeltaT", math.inf))}


def read_control_dict(path: str) -> dict:
    """parse_control_dict of a case's system/controlDict"""
    with open(path) as f:
        return parse_control_dict(f.read())


def initial_delta_t(dt: float, co: float, max_co: float, max_dt: float) -> float:
    """setInitialDeltaT.H: the first step never grows -- min(maxCo dt / Co, min(dt, maxDeltaT)) once Co > small"""
    if co > SMALL:
        return min(max_co * dt / co, min(dt, max_dt))
    return dt


def next_delta_t(dt: float, co: float, max_co: float, max_dt: float) -> float:
    """setDeltaT.H: shrink by maxCo / Co at once, grow by at most 20 % (and by a tenth of the headroom) per step"""
    f = max_co / (co + SMALL)
    g = min(min(f, 1.0 + 0.1 * f), 1.2)
    return min(g * dt, max_dt)


def advance(ctx, control: dict, n_steps: int, n_corr: int = 2, after_step=None) -> list:
    """n_steps time steps of `ctx` under the controlDict entries `control`, in the reference's order
    (dfLowMachFoam.C:246-262): the initial Courant number and setInitialDeltaT once, then per step the Courant
    number, setDeltaT, the step. `ctx` was set up with control["deltaT"]. Returns [(dt, Co, meanCo)] per step:
    the step size taken and the Courant numbers it was chosen from (those of the fields before the step, at the
    step size then in force). With adjustTimeStep off the step stays fixed and the numbers are only reported.
    after_step(ctx, i), if given, runs after step i (reading fields there leaves the step's record valid).

    The option step.courant is switched on, so from the second step on each Courant number is the record the
    previous dfmi_time_step left behind: one read of pinned memory, no launch and no stream drain."""
    adjust, max_co, max_dt = control["adjustTimeStep"], control["maxCo"], control["maxDeltaT"]
    ctx.set_option("step.courant", 1)
    co, mean = ctx.courant_no()
    if adjust:
        ctx.set_delta_t(initial_delta_t(ctx.delta_t(), co, max_co, max_dt))
    hist = []
    for _ in range(n_steps):
        co, mean = ctx.courant_no()
        if adjust:
            ctx.set_delta_t(next_delta_t(ctx.delta_t(), co, max_co, max_dt))
        ctx.time_step(n_corr)
        hist.append((ctx.delta_t(), co, mean))
        if after_step is not None:
            after_step(ctx, len(hist) - 1)
    return hist
