"""The HIP path on genuinely unstructured meshes (MI355X), against the CPU oracle.

Every other GPU test runs a hex block: six quad faces per cell, a coupling graph that 2-colours, gather rows
with padding at walls only. Here the meshes of tests/unstructured_meshes.py -- triangular prisms (W = 5), a mix
of prisms and hexahedra (W = 6 without being a hex box) and a 2:1 refined box with hanging nodes (W = 9, mostly
6-entry rows) -- take the library's other branches: the CSR face walk (kern<0>) and kern<6> with padding in
interior rows, the runtime-width solver and AMG loops at level 0, the Jacobi BiCGStab of a graph that does not
2-colour, row classes on many distinct rows, the one-workgroup solves at W != 6.

The stage assertions are test_gpu_parity's and test_gpu_schemes' own functions, imported and run on a fixture of
the same name over these meshes: assembly at 0 ulp, thermo at 1e-12, a full outer iteration at 1e-10 / 1e-11 /
1e-9. Upper-triangular face order makes "ascending face index" and "ascending column" the same order on any
mesh, so bitwise parity carries over from the hex box.
"""
import numpy as np
import pytest

import unstructured_meshes as um
from test_gpu_parity import (_case, _ell_width,
                             test_rho_eqn_bitwise, test_u_eqn_assembly_bitwise, test_hbya_bitwise,
                             test_p_eqn_assembly_bitwise, test_y_eqn_assembly_bitwise, test_y_ell_rows_bitwise,
                             test_e_eqn_assembly_bitwise, test_thermo_correct, test_full_outer_iteration)
from test_gpu_schemes import (REF, LL,
                              test_u_eqn_assembly_bitwise as test_schemes_u_eqn_assembly_bitwise,
                              test_y_eqn_assembly_bitwise as test_schemes_y_eqn_assembly_bitwise,
                              test_y_ell_rows_bitwise as test_schemes_y_ell_rows_bitwise,
                              test_e_eqn_assembly_bitwise as test_schemes_e_eqn_assembly_bitwise,
                              test_schemes_change_the_matrices,
                              test_full_outer_iteration as test_schemes_full_outer_iteration)
from test_gpu_turbulence import Case as LesCase, test_nut_pointwise_random_states, test_assembly_bitwise_with_device_nut

pytestmark = pytest.mark.gpu

FAMILIES = ("prisms", "hexprism", "refined")
W = {n: um.SMALL[n][1] for n in FAMILIES}
TIMED = "k_bcg_eo,k_bcg_spmv,k_bcg_small,k_pcg_small,k_cg_spmv"


def _build(name, cyclic_z=False, mixed=False, mech="burke9", schemes=None, size="small"):
    m = um.get(name, size, cyclic_z)
    return _case(periodic=False, walls=lambda mm: um.wall_types(mm, mixed), mech=mech, mixed=mixed, schemes=schemes,
                 mesh=m)


# ----------------------------------------------------------------------------- the parity suite's stages
@pytest.fixture(scope="module", params=["prisms", "prisms-cyclic-z", "hexprism", "refined", "refined-mixed",
                                        "prisms-generic", "refined-gri53"])
def periodic(request):
    """test_gpu_parity's fixture (its name is what the imported tests ask for) over the unstructured cases"""
    from dfmi import lib
    p = request.param
    if p.endswith("-generic"):
        lib.DEFAULT_OPTIONS["fv.species_generic"] = 1
        request.addfinalizer(lambda: lib.DEFAULT_OPTIONS.pop("fv.species_generic", None))
    name = p.split("-")[0]
    out = _build(name, cyclic_z=p.endswith("-cyclic-z"), mixed=p.endswith("-mixed"),
                 mech="gri53" if p.endswith("-gri53") else "burke9")
    request.addfinalizer(out[0].close)
    return out


def test_path_witnesses(periodic):
    """the case is not a hex box to the library, its rows have the family's width, and with default options
    a mesh of this size solves in the one-workgroup kernels; AMG level 0 has the rows' width"""
    ctx, m, t, st, pt, inert, dt = periodic
    from dfmi import case
    name = [n for n in FAMILIES if um.get(n, "small", False) is m or um.get(n, "small", True) is m][0]
    assert _ell_width(m) == W[name]
    case.push_state(ctx, st)
    ctx.kernel_timer(TIMED)
    ctx.time_step(2)
    n = {k: ctx.kernel_time(k)[1] for k in TIMED.split(",")}
    ctx.kernel_timer("")
    print(name, "launches", n, "amg", ctx.amg_info(), "row classes", ctx.row_classes(),
          "iters", {e: ctx.solver_stats(e)[0] for e in ("U", "Y", "E", "p")})
    assert ctx.hex_dims() == (0, 0, 0)
    assert ctx.amg_info()[0] == (m.n_cells, W[name])
    assert n["k_bcg_small"] > 0 and n["k_pcg_small"] > 0, n
    assert n["k_bcg_eo"] == 0 and n["k_bcg_spmv"] == 0 and n["k_cg_spmv"] == 0, n
    for e, cap in {"U": 20, "Y": 20, "E": 20, "p": 1000}.items():
        it, r0, rel = ctx.solver_stats(e)
        assert it < cap and rel <= 1e-5, (e, it, r0, rel)
    case.push_state(ctx, st)


# ----------------------------------------------------------------------------- the case schemes
@pytest.fixture(scope="module", params=["ref-prisms", "ll-prisms", "ref-refined", "ll-refined"])
def sc(request):
    """test_gpu_schemes' fixture: limitedLinear(01 / V) and cubic, whose limiter reads mesh_distance and the
    on-the-fly gradients across faces of unequal size"""
    schemes = REF if request.param.startswith("ref") else LL
    out = _build(request.param.split("-")[1], schemes=schemes)
    request.addfinalizer(out[0].close)
    return out + (schemes,)


# ----------------------------------------------------------------------------- option equivalences
_runs = {}


def _run(name, **opts):
    """one outer iteration at production tolerances on the batched solver path (solver.small = 0: the path
    meshes above 4096 cells take) and an AMG coarsened to 64 cells (several levels on these sizes), with the
    given options; cached per (mesh, options)"""
    from dfmi import lib
    key = (name, tuple(sorted(opts.items())))
    if key in _runs:
        return _runs[key]
    opts = {"solver.small": 0, "amg.coarsest_size": 64, **opts}
    lib.DEFAULT_OPTIONS.update(opts)
    try:
        ctx, m, t, st, pt, inert, dt = _build(name)
        ctx.kernel_timer(TIMED)
        ctx.time_step(2)
        out = {k: ctx.get_field(k, (m.n_cells,)) for k in ("p", "T", "rho", "he")}
        out["U"] = ctx.get_field("U", (3, m.n_cells))
        out["Y"] = ctx.get_field("Y", (t.S, m.n_cells))
        out["iters"] = {e: ctx.solver_stats(e)[0] for e in ("U", "Y", "E", "p")}
        out["launches"] = {k: ctx.kernel_time(k)[1] for k in TIMED.split(",")}
        ctx.kernel_timer("")
        out["ncls"] = ctx.row_classes()
        out["hex"] = ctx.hex_dims()
        out["amg"] = ctx.amg_info()
        out["face_form"] = ctx.get_option("pcg.face_form")
        ctx.close()
    finally:
        for k in opts:
            lib.DEFAULT_OPTIONS.pop(k, None)
    _runs[key] = out
    return out


def _same(a, b):
    assert a["iters"] == b["iters"], (a["iters"], b["iters"])
    for k in ("p", "T", "rho", "he", "U", "Y"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", FAMILIES)
def test_batched_path_witnesses(name):
    """solver.small = 0: the coupling graph does not 2-colour, so BiCGStab keeps the Jacobi path (k_bcg_spmv, no
    k_bcg_eo launch), the p solve runs the multi-launch PCG, and level 0 of the AMG has the rows' width"""
    a = _run(name)
    print(name, a["launches"], "amg", a["amg"], "row classes", a["ncls"], "iters", a["iters"])
    assert a["hex"] == (0, 0, 0)
    assert a["launches"]["k_bcg_eo"] == 0 and a["launches"]["k_bcg_spmv"] > 0, a["launches"]
    assert a["launches"]["k_cg_spmv"] > 0 and a["launches"]["k_bcg_small"] == 0 and a["launches"]["k_pcg_small"] == 0
    assert a["amg"][0] == (um.SMALL[name][3], W[name]) and len(a["amg"]) >= 2, a["amg"]
    assert all(np.isfinite(a[k]).all() for k in ("p", "T", "rho", "he", "U", "Y"))
    for e, cap in {"U": 20, "Y": 20, "E": 20, "p": 1000}.items():
        assert 0 < a["iters"][e] < cap, a["iters"]


@pytest.mark.parametrize("name", FAMILIES)
def test_row_classes_bitwise_explicit_rows(name):
    a, b = _run(name), _run(name, **{"solver.row_classes": 0})
    print(name, "row classes", a["ncls"])
    assert b["ncls"] == 0
    _same(a, b)


def test_csr_walk_bitwise_face_rows_on_hexprism():
    """kern<0> against kern<6> on a W = 6 mesh that is not a hex box: padding entries in interior rows"""
    _same(_run("hexprism"), _run("hexprism", **{"fv.csr_walk": 1}))


@pytest.mark.parametrize("name", FAMILIES)
def test_face_form_stays_off_by_itself(name):
    """pcg.face_form is on by default; without a detected hex box the FaceOp is not used, so switching the option
    off changes nothing"""
    a = _run(name)
    assert a["face_form"] == 1 and a["hex"] == (0, 0, 0)
    _same(a, _run(name, **{"pcg.face_form": 0}))


@pytest.mark.parametrize("opt", ["fv.p_post_fused", "pcg.fuse_setup", "step.hbya_early"])
@pytest.mark.parametrize("name", FAMILIES)
def test_fused_corrector_options_bitwise(name, opt):
    _same(_run(name), _run(name, **{opt: 0}))


@pytest.mark.parametrize("small", [1, 0], ids=["one-workgroup", "batched"])
@pytest.mark.parametrize("name", FAMILIES)
def test_amg_levels_full_step(name, small, monkeypatch):
    """a multi-level V-cycle whose level 0 has the family's width (the W == 6 specialisations of the smoother
    kernels do not apply: their runtime-width twins run at level 0), inside the one-workgroup PCG and on the
    launch-per-level path: the p solves reach the oracle's exact solution (test_amg_pcg_full_step's bounds)"""
    from dfmi import lib
    from conftest import rel_err
    from test_gpu_parity import _oracle
    monkeypatch.setitem(lib.DEFAULT_OPTIONS, "amg.coarsest_size", 64)
    monkeypatch.setitem(lib.DEFAULT_OPTIONS, "solver.small", small)
    ctx, m, t, st, pt, inert, dt = _build(name)
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-14, 1e-300)
    o = _oracle(m, t, st, pt, inert, dt)
    o.time_step(2)
    ctx.kernel_timer(TIMED)
    ctx.time_step(2)
    n = {k: ctx.kernel_time(k)[1] for k in TIMED.split(",")}
    ctx.kernel_timer("")
    amg = ctx.amg_info()
    err = {k: rel_err(ctx.get_field(k, (m.n_cells,)), o[k]) for k in ("T", "p", "rho")}
    err["U"] = rel_err(ctx.get_field("U", (3, m.n_cells)), o["U"])
    print(name, "small" if small else "batched", "amg", amg, "p iters", ctx.solver_stats("p")[0], err)
    assert len(amg) >= 2 and amg[0] == (m.n_cells, W[name]), amg
    assert (n["k_pcg_small"] > 0) == bool(small) and (n["k_cg_spmv"] > 0) == (not small), n
    for k, tl in {"T": 1e-10, "p": 1e-11, "rho": 1e-10, "U": 1e-9}.items():
        assert err[k] < tl, (k, err[k])
    ctx.close()


# ----------------------------------------------------------------------------- uniform state
def test_device_keeps_a_uniform_state():
    """U = 0 and uniform T, p, Y inside zeroGradient walls on `refined`: one outer iteration moves nothing beyond
    the rounding residual of the cells' closed surfaces (unstructured_meshes.uniform_state_bounds, the CPU test's
    bound)"""
    from dfmi import case
    from dfmi.lib import Context
    from test_gpu_parity import _mech
    m = um.get("refined")
    ym, t = _mech("burke9")
    ctx = Context(0)
    pt = case.default_patch_types(m)
    dt = 1e-6
    case.setup_context(ctx, m, t, ym["species"].index("N2"), dt, pt)
    f = um.uniform_fields(m, ym["species"])
    case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"])
    ctx.call("pre_time_step")
    st = case.pull_state(ctx, m, t.S)
    ctx.time_step(2)
    ub, sb = um.uniform_state_bounds(m, st, dt)
    for n in ("T", "p", "rho", "he"):
        d = np.abs(ctx.get_field(n, (m.n_cells,)) - st[n]).max() / np.abs(st[n]).max()
        print("uniform", n, d, "bound", sb)
        assert d <= sb, (n, d, sb)
    dY = np.abs(ctx.get_field("Y", (t.S, m.n_cells)) - st["Y"]).max()
    dU = np.abs(ctx.get_field("U", (3, m.n_cells))).max()
    print("uniform Y", dY, "bound", sb, "U", dU, "bound", ub)
    assert dY <= sb and dU <= ub
    ctx.close()


# ----------------------------------------------------------------------------- LES
@pytest.fixture(scope="module")
def lc():
    """test_gpu_turbulence's fixture: its walled case on `refined` (Smagorinsky and WALE; the filter width
    cbrt(V) jumps by 2 across the refinement interface)"""
    c = LesCase("walls", mesh=um.get("refined"))
    yield c
    c.ctx.close()


# ----------------------------------------------------------------------------- above 4096 cells
@pytest.fixture(scope="module")
def big():
    out = _build("prisms", size="large")
    yield out
    out[0].close()


def test_large_prisms_full_outer_iteration(big):
    """6118 prisms, default options: the batched solvers (Jacobi BiCGStab, multi-launch PCG), an AMG of several
    levels, ragged last workgroups (6118 = 95 x 64 + 38) -- one outer iteration against the oracle at
    test_full_outer_iteration's thresholds"""
    ctx, m, t, st, pt, inert, dt = big
    assert m.n_cells == 6118
    ctx.kernel_timer(TIMED)
    test_full_outer_iteration(big)
    n = {k: ctx.kernel_time(k)[1] for k in TIMED.split(",")}
    ctx.kernel_timer("")
    amg = ctx.amg_info()
    print("large prisms launches", n, "amg", amg, "row classes", ctx.row_classes())
    assert ctx.hex_dims() == (0, 0, 0)
    assert n["k_bcg_spmv"] > 0 and n["k_cg_spmv"] > 0, n
    assert n["k_bcg_eo"] == 0 and n["k_bcg_small"] == 0 and n["k_pcg_small"] == 0, n
    assert len(amg) >= 3 and amg[0] == (6118, 5), amg


def test_large_prisms_steps_are_deterministic(big):
    """the same state stepped twice gives bitwise identical fields (test_gpu_fullsize's check)"""
    from dfmi import case
    ctx, m, t, st, pt, inert, dt = big
    runs = []
    for _ in range(2):
        case.push_state(ctx, st)
        ctx.time_step(2)
        runs.append({n: ctx.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he")} |
                    {"U": ctx.get_field("U", (3, m.n_cells)), "Y": ctx.get_field("Y", (t.S, m.n_cells))})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    for e, cap in {"U": 20, "Y": 20, "E": 20, "p": 1000}.items():
        it, r0, rel = ctx.solver_stats(e)
        assert it < cap and rel <= 1e-5, (e, it, r0, rel)
    case.push_state(ctx, st)
