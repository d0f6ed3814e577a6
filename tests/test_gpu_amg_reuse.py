"""The second pressure corrector preconditioned with the first corrector's V-cycle (option amg.reuse) against a
V-cycle rebuilt per solve, for the mixed-precision (fp32, face-wise level 0) and the fp64 V-cycle: both meet the
system's own tolerance (AmgX RELATIVE_INI 1e-5, amgxpOptions) in about the same number of PCG iterations and
land on the same fields to that tolerance. The fp64 V-cycle's level 0 reads the current solve's ELL values --
the reuse path must keep writing them."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu


def _run(reuse, precision, steps=2):
    from dfmi.lib import Context, DEFAULT_OPTIONS
    from dfmi.mesh import hex_box
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi import case
    opts = {"amg.reuse": reuse, "amg.precision": precision}
    DEFAULT_OPTIONS.update(opts)
    try:
        ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
        t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
        m = hex_box(32, 32, 24, lengths=(2 * np.pi * 1e-3,) * 3, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3)
        ctx = Context(0)
        case.setup_context(ctx, m, t, ym["species"].index("N2"), 1e-6, case.default_patch_types(m))
        f = case.tgv_fields(m, ym["species"], kernel_radius=1.2e-3)
        case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"])
        ctx.call("pre_time_step")
        its, rels = [], []
        for _ in range(steps):
            ctx.time_step(2)
            it, _, rel = ctx.solver_stats("p")   # the second corrector's solve
            its.append(it)
            rels.append(rel)
        out = {k: ctx.get_field(k, (m.n_cells,)) for k in ("p", "T", "rho")}
        out["U"] = ctx.get_field("U", (3, m.n_cells))
        ctx.close()
        return its, rels, out
    finally:
        for k in opts:
            DEFAULT_OPTIONS.pop(k, None)


@pytest.mark.parametrize("precision", [32, 64])
def test_reused_vcycle_meets_tolerance(precision):
    it0, rel0, a = _run(0, precision)
    it1, rel1, b = _run(1, precision)
    assert max(rel0) <= 1e-5 and max(rel1) <= 1e-5, (rel0, rel1)
    assert all(i1 <= i0 + 2 for i0, i1 in zip(it0, it1)), (it0, it1)
    assert min(it1) > 1
    # the same pressure to the solver tolerance (the p field's variation is a tiny part of its 1e5 Pa level)
    for k, tol in (("p", 1e-6), ("T", 1e-6), ("rho", 1e-6), ("U", 1e-4)):
        assert rel_err(a[k], b[k]) < tol, (k, rel_err(a[k], b[k]))


# ---- the cross-step reuse window (amg.reuse_steps): with one corrector per step the corrector is the first one,
# the solve that may precondition with operators up to reuse_steps - 1 steps old; solver_stats("p") is its own.
# Each step's p system is rebuilt from dfmi_get_matrix and its true residual audited (tests/solver_audit.py), and
# the k_galerkin launch count says whether the hierarchy was rebuilt.
WINDOW = 17
REBUILT = (1, 9, 17)      # by capi.cpp's age rule with the default amg.reuse_steps = 8


def _window(ctx, m, pt, S, inert, label, steps=WINDOW):
    """`steps` time steps of one corrector; per step the audit of the p solve (reconstruction, convergence before
    max_iter against the true residual, honest report) and the k_galerkin launches. Returns (iters, launches)."""
    from oracle import ldu_system
    from solver_audit import check, matrix_parts, split_systems
    from test_gpu_parity import _ell_width
    W = _ell_width(m)
    C = m.n_cells
    its, gal = [], []
    for k in range(1, steps + 1):
        x0 = ctx.get_field("p", (C,))
        ctx.kernel_timer("k_galerkin")
        ctx.time_step(1)
        gal.append(ctx.kernel_time("k_galerkin")[1])
        ctx.kernel_timer("")
        parts = matrix_parts(ctx, m, "p", S)
        x = ctx.get_field("p", (C,))
        stats = ctx.solver_stats("p")
        systems = [ldu_system(m, pt["p"], *p) for p in split_systems(m, "p", parts, S, inert)]
        check(f"{label} step {k} p", systems, x0[None, :], x[None, :], stats, 1e-5, 1000, W)
        its.append(stats[0])
    return its, gal


def _tgv_window(reuse_steps):
    from dfmi.lib import Context, DEFAULT_OPTIONS
    from dfmi.mesh import hex_box
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi import case
    opts = {} if reuse_steps is None else {"amg.reuse_steps": reuse_steps}
    DEFAULT_OPTIONS.update(opts)
    try:
        ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
        t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
        m = hex_box(32, 32, 24, lengths=(2 * np.pi * 1e-3,) * 3, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3)
        ctx = Context(0)
        inert = ym["species"].index("N2")
        pt = case.setup_context(ctx, m, t, inert, 1e-6, case.default_patch_types(m))
        f = case.tgv_fields(m, ym["species"], kernel_radius=1.2e-3)
        case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"])
        ctx.call("pre_time_step")
        assert ctx.get_option("amg.reuse_steps") == (8 if reuse_steps is None else reuse_steps)
        its, gal = _window(ctx, m, pt, t.S, inert, f"tgv reuse_steps {reuse_steps or 8}")
        out = {k: ctx.get_field(k, (m.n_cells,)) for k in ("p", "T", "rho")}
        out["U"] = ctx.get_field("U", (3, m.n_cells))
        ctx.close()
        return its, gal, out
    finally:
        for k in opts:
            DEFAULT_OPTIONS.pop(k, None)


def test_reuse_window_first_corrector_converges_on_old_operators():
    """17 steps of the TGV box, fp32 V-cycle, chemistry off, default amg.reuse_steps = 8: the hierarchy is rebuilt on
    steps 1, 9 and 17 and reused on the other 14; every step's first corrector meets the tolerance on the residual
    recomputed outside the library, in no more than the fresh hierarchy's iterations + 2, and the fields after the
    window agree with the run that rebuilds every step (amg.reuse_steps = 1)."""
    it8, gal8, a = _tgv_window(None)
    it1, gal1, b = _tgv_window(1)
    print("tgv p iterations per step: reuse_steps 8", it8, "reuse_steps 1", it1)
    assert [k for k in range(1, WINDOW + 1) if gal8[k - 1] > 0] == list(REBUILT), gal8
    assert all(g > 0 for g in gal1), gal1
    assert all(i8 <= i1 + 2 for i8, i1 in zip(it8, it1)), (it8, it1)
    assert min(it8) > 1
    for k, tol in (("p", 1e-6), ("T", 1e-6), ("rho", 1e-6), ("U", 1e-4)):
        assert rel_err(a[k], b[k]) < tol, (k, rel_err(a[k], b[k]))


@pytest.mark.parametrize("reuse_steps", [8, 1])
def test_reuse_window_flame1d(reuse_steps):
    """The 1D flame with chemistry (the case whose p matrix moves from step to step): over a full reuse window every
    step's p solve converges before max_iter on the true residual and reports it honestly, with the hierarchy 0 - 7
    steps old (reuse_steps = 8) as with a fresh one (1). No iteration margin is asserted (the project has none for
    this case); the counts are printed for DESIGN.md."""
    from dfmi.lib import DEFAULT_OPTIONS
    from test_gpu_flame1d import _setup
    DEFAULT_OPTIONS["amg.reuse_steps"] = reuse_steps
    try:
        ctx, m, t, ym, mech, pt, inert, dt, bv = _setup()
    finally:
        DEFAULT_OPTIONS.pop("amg.reuse_steps", None)
    ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
    its, gal = _window(ctx, m, pt, t.S, inert, f"flame1d reuse_steps {reuse_steps}")
    print(f"flame1d p iterations per step, reuse_steps {reuse_steps}:", its)
    rebuilt = [k for k in range(1, WINDOW + 1) if gal[k - 1] > 0]
    assert rebuilt == (list(REBUILT) if reuse_steps == 8 else list(range(1, WINDOW + 1))), gal
    ctx.close()
