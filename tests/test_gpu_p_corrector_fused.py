"""The pressure corrector's fused forms against the separate launches, bit for bit (0 ulp):

  step.hbya_early   the first corrector's HbyA right after the U solve, ahead of the Y and E equations (capi.cpp do_U_Y_E)
  pcg.fuse_setup    k_p_cell + k_ell_build + k_copy_x + k_cg_init<0, true> as one launch, k_p_setup_fused, on the
                    face-form PCG that reuses the V-cycle (linsolve.hip)
  fv.p_post_fused   k_p_flux_face folded into k_p_cell_post's cell walk, k_p_cell_post_phi (fv_kernels.hip)

Every case runs one state with all three options 0 (the reference, computed once per mesh and scenario and shared)
and again with all 1 and with each option alone, and compares the fields the corrector writes, the p matrix as
dfmi_get_matrix holds it and the p solve's statistics. The meshes are the smallest on which each path can go wrong;
solver.small = 0 puts them on the batched face-form path and amg.coarsest_size = 8 gives their V-cycle the second level
the reuse shortcut needs (amg_l0_fusable)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NEW = ("step.hbya_early", "pcg.fuse_setup", "fv.p_post_fused")
VARIANTS = ("all",) + NEW
# 8x6x4 periodic: every cell has coupled slots, even extents keep the face form and the even-odd solvers;
# 7x5x3 walled (p fixed on one wall): non-coupled slots add to dS / rhs, padding face slots, C no multiple of 256;
# 12x10x8 periodic, graded in every direction: a geometry index mix-up shows
MESHES = {
    "periodic8x6x4": dict(n=(8, 6, 4), periodic=(True,) * 3, gradings=(1.0, 1.0, 1.0)),
    "walled7x5x3": dict(n=(7, 5, 3), periodic=(False,) * 3, gradings=(1.0, 1.3, 1.0)),
    "graded12x10x8": dict(n=(12, 10, 8), periodic=(True,) * 3, gradings=(1.4, 0.7, 1.9)),
}
TIMED = "k_p_setup_fused,k_p_cell_post_phi,k_p_cell,k_cg_init,k_p_flux_face,k_p_cell_post"

_cache = {}


def _opts(variant):
    on = NEW if variant == "all" else () if variant == "none" else (variant,)
    o = {k: float(k in on) for k in NEW}
    o.update({"solver.small": 0, "amg.coarsest_size": 8, "amg.reuse_steps": 2})
    return o


def _collect(ctx, m):
    C, F, B = m.n_cells, m.n_faces, m.n_boundary_slots
    out = {k: ctx.get_field(k, (C,)) for k in ("p", "K", "dpdt", "rho")}
    for k in ("U", "HbyA"):
        out[k] = ctx.get_field(k, (3, C))
    for k in ("phi", "rhorAUf", "phiHbyA"):
        out[k] = ctx.get_field(k, (F,))
    out["boundary_phi"] = ctx.get_field("boundary_phi", (B,))
    for part, n in (("lower", F), ("upper", F), ("diag", C), ("source", C), ("internal_coeffs", B),
                    ("boundary_coeffs", B)):
        out["matrix." + part] = ctx.get_matrix("p", part, n)
    out["stats"] = np.array(ctx.solver_stats("p"), dtype=np.float64)
    return out


def _run(mesh, scenario, variant):
    key = (mesh, scenario, variant)
    if key in _cache:
        return _cache[key]
    from dfmi.lib import Context, DEFAULT_OPTIONS
    from dfmi.mesh import hex_box, FIXED_VALUE
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi import case
    opts = _opts(variant)
    DEFAULT_OPTIONS.update(opts)
    try:
        ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
        t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
        spec = MESHES[mesh]
        m = hex_box(*spec["n"], lengths=(2 * np.pi * 1e-3,) * 3, gradings=spec["gradings"], periodic=spec["periodic"])
        pt = case.default_patch_types(m)
        bvals = None
        if not spec["periodic"][0]:
            right = [i for i, p in enumerate(m.patches) if p.name == "right"][0]
            pt["p"][right] = FIXED_VALUE
            bvals = {"p": {"right": 101325.0}}
        ctx = Context(0)
        case.setup_context(ctx, m, t, ym["species"].index("N2"), 1e-6, pt)
        ctx.set_solver("p", 1000, 1e-9, 1e-300)
        f = case.tgv_fields(m, ym["species"], kernel_radius=1.2e-3)
        case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"], bvals=bvals)
        out = {}
        if scenario in ("p_process", "set_U_old"):
            # the separate entries, nothing precomputed by a time step
            ctx.call("pre_time_step")
            ctx.call("rho_process")
            ctx.call("U_process")
            if scenario == "set_U_old":
                ctx.set_field("U_old", 0.5 * ctx.get_field("U_old", (3, m.n_cells)))
            ctx.call("U_get_HbyA")
            ctx.call("p_process")
        elif scenario == "steps":
            # amg.reuse_steps = 2: first correctors that rebuild the V-cycle (steps 1, 3) and one that reuses it (2)
            for _ in range(3):
                ctx.time_step(2)
        elif scenario == "set_delta_t":
            ctx.time_step(2)
            ctx.set_delta_t(0.4e-6)
            ctx.time_step(2)
        elif scenario == "timers":
            # armed kernel timers: the step runs on one stream
            ctx.time_step(2)
            ctx.kernel_timer(TIMED)
            ctx.time_step(2)
            out["launches"] = {k: ctx.kernel_time(k)[1] for k in TIMED.split(",")}
            ctx.kernel_timer("")
        out.update(_collect(ctx, m))
        ctx.close()
    finally:
        for k in opts:
            DEFAULT_OPTIONS.pop(k, None)
    _cache[key] = out
    return out


def _assert_same(a, b, label):
    for k in b:
        if k == "launches":
            continue
        assert a[k].shape == b[k].shape, (label, k)
        diff = np.flatnonzero(a[k].ravel().view(np.int64) != b[k].ravel().view(np.int64))
        assert diff.size == 0, (label, k, diff.size, diff[:4], a[k].ravel()[diff[:4]], b[k].ravel()[diff[:4]])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scenario", ("p_process", "steps"))
@pytest.mark.parametrize("mesh", list(MESHES))
def test_fused_corrector_is_bitwise_the_separate_launches(mesh, scenario, variant):
    ref = _run(mesh, scenario, "none")
    got = _run(mesh, scenario, variant)
    assert ref["stats"][0] > 1, ref["stats"]   # a p solve that iterates
    assert np.all(np.isfinite(ref["p"])) and np.all(np.isfinite(ref["U"]))
    _assert_same(got, ref, (mesh, scenario, variant))


@pytest.mark.parametrize("scenario", ("set_delta_t", "set_U_old"))
def test_changed_step_size_and_old_fields_reach_the_corrector(scenario):
    """a dfmi_set_delta_t between two steps, and a dfmi_set_field("U_old") before dfmi_p_process: nothing the fused
    forms keep may outlive either"""
    mesh = "graded12x10x8"
    ref = _run(mesh, scenario, "none")
    if scenario == "set_U_old":   # the change does reach the corrector (ddtCorr reads U_old)
        assert not np.array_equal(ref["phiHbyA"], _run(mesh, "p_process", "none")["phiHbyA"])
    _assert_same(_run(mesh, scenario, "all"), ref, (mesh, scenario))


@pytest.mark.parametrize("mesh", list(MESHES))
def test_one_stream_step_and_the_kernels_that_ran(mesh):
    """kernel timers armed (the step on one stream): the same bits, and the fused kernels ran in place of the
    separate ones with the options on and not at all with them off"""
    off, on = _run(mesh, "timers", "none"), _run(mesh, "timers", "all")
    _assert_same(on, off, (mesh, "timers"))
    a, b = on["launches"], off["launches"]
    print(mesh, "launches on", a, "off", b)
    # step 2 of amg.reuse_steps = 2: both correctors reuse the V-cycle, so both take the fused setup
    assert a["k_p_setup_fused"] == 2 and a["k_p_cell"] == 0 and a["k_cg_init"] == 0, a
    assert a["k_p_cell_post_phi"] == 2 and a["k_p_flux_face"] == 0 and a["k_p_cell_post"] == 0, a
    assert b["k_p_setup_fused"] == 0 and b["k_p_cell_post_phi"] == 0, b
    assert b["k_p_cell"] == 2 and b["k_cg_init"] == 2 and b["k_p_flux_face"] == 2 and b["k_p_cell_post"] == 2, b
