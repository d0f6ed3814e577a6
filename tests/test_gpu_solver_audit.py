"""Every linear-solver path's reported residual against b - A x evaluated outside the library (MI355X).

`dfmi_solver_stats` reports what the solver kernels kept in their scalars: recurrence residuals (r -= alpha q,
r = s - omega t, the even-odd path's reduced ||D r||, the single-reduction PCG's recurrences). Here each solve's
system is rebuilt from `dfmi_get_matrix` (oracle.ldu_system, the fold k_ell_build performs) and b - A x is
evaluated in np.longdouble (tests/solver_audit.py) for the initial guess and the returned solution. For every
system s of every solve (`dfmi_solver_stats` reports the worst system):

 1. reconstruction   |max_s res0_true - res0_reported| <= max_s floor0_s  (the audit rebuilt the solver's system);
 2. convergence      iters < max_iter  =>  res_true_s <= tol res0_true_s + floor_s for every s;
 3. report           |max_s res_true_s / res0_true_s - rel_reported| <= max_s floor_s / res0_true_s
                     (for one system: |rel_true - rel_reported| res0 <= floor);
 4. cap              max_iter 3 (U, Y, E) / 4 (p) at tol 1e-12: iters == max_iter, 3 holds, res_true < res0_true
                     (a path that reaches 1e-12 before the cap: 2 holds at 1e-12, then the cap one below its need);
 5. keep             a second *_process on the converged state with abs_tol above its residual: 0 iterations, x
                     bitwise unchanged.

floor0 / floor are the derived rounding bounds of solver_audit (one fp64 residual evaluation; the drift of a
recurrence over `iters` updates). 1-3 run at the production tolerance 1e-5 (max_iter 20 / 1000) and at 1e-9
(300 / 3000).

State: species are overwritten with smooth, species-dependent, strictly positive fields and RR = 0 (chemistry
off), because y_post_solve clips Y at 0: the field after Y_process is the solver's x only where nothing was
clipped, which the test asserts (a clipped entry is exactly 0.0). The YEqn's production path writes the solver
rows directly and leaves no LDU parts behind, so Y's parts come from dfmi_assemble("Y") on the same inputs just
before Y_process (the two assemblies are bitwise equal: test_gpu_parity.test_y_ell_rows_bitwise); U, E and p are
read after their process call.
"""
import os
import threading

import numpy as np
import pytest

from conftest import GOLDEN
from solver_audit import ROWS, assemble_ranks, audit, check as _check, matrix_parts as _parts, split_systems as _split
from test_gpu_eo import _walls
from test_gpu_parity import _case, _ell_width

pytestmark = pytest.mark.gpu

L = 2 * np.pi * 1e-3
PT_KEY = {"U": "U", "Y": "Y", "E": "he", "p": "p"}
FIELD = {"U": "U", "Y": "Y", "E": "he", "p": "p"}
TIMED = "k_bcg_eo,k_bcg_spmv,k_bcg_small,k_pcg_small,k_cg_spmv,k_cg_x,k_cg_x_smooth,k_vtail,k_dilu_fwd"
PRODUCTION = (1e-5, 20, 1000)
TIGHT = (1e-9, 300, 3000)


def _positive_species(cc, Y, inert):
    """every species present, smooth, non-uniform and species-dependent; min Y > 1e-2 after normalising"""
    x = cc / L
    ph = np.arange(Y.shape[0])[:, None]
    Yn = (np.maximum(Y, 0.0) + 0.02) * (1 + 0.2 * np.sin(2 * np.pi * x[:, 0] + 0.3 + ph)
                                        * np.cos(2 * np.pi * x[:, 1] + 0.7 * ph)
                                        * (1 + 0.1 * np.sin(2 * np.pi * x[:, 2] + 0.2)))
    return Yn / Yn.sum(axis=0)


def _audit_state(ctx, m, t, st, inert, own_species=False):
    """the audited state: positive species (unless the case brings its own), RR = 0, a non-uniform pressure"""
    from dfmi import case
    st = dict(st)
    if not own_species:
        st["Y"] = _positive_species(m.cell_centres, st["Y"], inert)
        st["boundary_Y"] = case.boundary_values(m, st["Y"])
    st["RR"] = np.zeros((t.S, m.n_cells))
    # a pressure field with a gradient (the TGV state's is uniform): U's solved right-hand side source_solve then
    # differs from the matrix source, and the p solve starts from a non-trivial guess
    x = m.cell_centres / L
    st["p"] = st["p"] * (1 + 1e-3 * np.sin(2 * np.pi * x[:, 0] + 0.4) * np.cos(2 * np.pi * x[:, 1] + 0.1)
                         * (1 + 0.3 * np.sin(2 * np.pi * x[:, 2])))
    st["boundary_p"] = case.boundary_values(m, st["p"])
    case.push_state(ctx, st)
    for fld, shape in (("Y", (t.S, m.n_boundary_slots)), ("p", (m.n_boundary_slots,))):
        ctx.correct_boundary(fld)
        st["boundary_" + fld] = ctx.get_field("boundary_" + fld, shape)
    assert st["Y"].min() >= (0.0 if own_species else 1e-3) and st["Y"].min() > 0
    return st


def _x(ctx, m, eqn, S, inert):
    C = m.n_cells
    if eqn == "U":
        return ctx.get_field("U", (3, C))
    if eqn == "Y":
        return np.delete(ctx.get_field("Y", (S, C)), inert, axis=0)
    return ctx.get_field(FIELD[eqn], (C,))[None, :]


def _solve(ctx, m, S, inert, eqn):
    """one *_process call: (parts, x0, x, stats)"""
    x0 = _x(ctx, m, eqn, S, inert)
    if eqn == "Y":
        ctx.assemble("Y")
        parts = _parts(ctx, m, eqn, S)
    ctx.call(eqn + "_process")
    if eqn != "Y":
        parts = _parts(ctx, m, eqn, S)
    x = _x(ctx, m, eqn, S, inert)
    if eqn == "Y":
        assert all(x[s].min() > 0 for s in range(x.shape[0])), "a species was clipped at 0: x is not the solver's"
    return parts, x0, x, ctx.solver_stats(eqn)


def _sequence(ctx, m, t, pt, inert, name, tol, mi, mi_p, W, eqns=("U", "Y", "E", "p"), audited=None, cap=False,
              keep=False, caps=None):
    """U_process -> Y_process -> E_process -> U_get_HbyA -> p_process, each solve audited; caps: max_iter per
    equation instead of mi / mi_p"""
    from oracle import ldu_system
    out = {"iters": {}}
    mis = {"U": mi, "Y": mi, "E": mi, "p": mi_p, **(caps or {})}
    for e, n in mis.items():
        ctx.set_solver(e, n, tol)
    for eqn in eqns:
        if eqn == "p":
            ctx.call("U_get_HbyA")
        parts, x0, x, stats = _solve(ctx, m, t.S, inert, eqn)
        if audited is not None and eqn not in audited:
            continue
        systems = [ldu_system(m, pt[PT_KEY[eqn]], *p) for p in _split(m, eqn, parts, t.S, inert)]
        cfg_mi = mis[eqn]
        out["iters"][eqn] = stats[0]
        out[eqn] = _check(f"{name} {eqn} tol {tol:g}", systems, x0, x, stats, tol, cfg_mi, W, cap=cap)
        if keep:   # the converged state again, abs_tol above its residual under the re-assembled system
            ctx.assemble(eqn)
            systems = [ldu_system(m, pt[PT_KEY[eqn]], *p) for p in _split(m, eqn, _parts(ctx, m, eqn, t.S), t.S, inert)]
            A = [audit(sy, x[s], x[s], tol, 0, W) for s, sy in enumerate(systems)]
            abs_tol = 2 * max(a["res0"] + a["floor0"] for a in A)
            ctx.set_solver(eqn, cfg_mi, tol, abs_tol)
            ctx.call(eqn + "_process")
            ctx.set_solver(eqn, cfg_mi, tol)
            it2, r02, _ = ctx.solver_stats(eqn)
            x2 = _x(ctx, m, eqn, t.S, inert)
            print(f"{name} {eqn} keep: abs_tol {abs_tol:.3e} iters {it2} res0 reported {r02:.3e}")
            assert it2 == 0, (name, eqn, "keep", it2)
            assert np.array_equal(x2, x), (name, eqn, "keep changed x")
            assert abs(max(a["res0"] for a in A) - r02) <= max(a["floor0"] for a in A), (name, eqn, "keep res0")
    return out


def _capped(ctx, m, t, pt, inert, name, st, W, **kw):
    """Assertion 4: max_iter 3 (U, Y, E) / 4 (p) at tol 1e-12. These systems are strongly diagonally dominant
    (dt = 1e-6), and the even-odd BiCGStab reaches 1e-12 in two iterations: a solve that converges before its cap
    is held to assertion 2 at 1e-12, and the sequence is run again from the same state with that equation's cap one
    below the iterations it needed, so every path's cap exit is taken."""
    from dfmi import case
    caps = {"U": 3, "Y": 3, "E": 3, "p": 4}
    case.push_state(ctx, st)
    first = _sequence(ctx, m, t, pt, inert, name, 1e-12, 3, 4, W, cap=True, **kw)["iters"]
    early = {e: it - 1 for e, it in first.items() if it < caps[e]}
    if early:
        assert min(early.values()) >= 1, (name, first)
        caps.update(early)
        case.push_state(ctx, st)
        again = _sequence(ctx, m, t, pt, inert, name + " lowered cap", 1e-12, 3, 4, W, cap=True, caps=caps, **kw)["iters"]
        assert all(again[e] == caps[e] for e in again), (name, caps, again)


def _mixed_walls(m):
    """test_gpu_parity's "mixed" case: fixedValue on left, an open outlet (inletOutlet U / Y, waveTransmissive p)
    on right, zeroGradient elsewhere"""
    from dfmi.mesh import FIXED_VALUE, FIXED_ENERGY, GRADIENT_ENERGY, INLET_OUTLET, WAVE_TRANSMISSIVE
    fixed = [i for i, p in enumerate(m.patches) if p.name == "left"]
    out = [i for i, p in enumerate(m.patches) if p.name == "right"]
    fv = {}
    for f in ("U", "T", "Y"):
        ty = m.patch_types(0).copy()
        ty[fixed] = FIXED_VALUE
        fv[f] = ty
    ty = m.patch_types(GRADIENT_ENERGY).copy()
    ty[fixed] = FIXED_ENERGY
    fv["he"] = ty
    fv["U"][out] = INLET_OUTLET
    fv["Y"][out] = INLET_OUTLET
    fv["p"] = m.patch_types(0).copy()
    fv["p"][out] = WAVE_TRANSMISSIVE
    return fv


BOX = dict(nx=16, ny=12, nz=8, mech="burke9")
BIG = dict(nx=20, ny=20, nz=14, gradings=(1.0, 1.3, 1.0), mech="burke9")
# name: (kwargs of _case, options, kernels that must have launched, kernels that must not)
CASES = {
    "eo-batched": (BOX, {"solver.small": 0}, ("k_bcg_eo", "k_cg_spmv", "k_cg_x_smooth"), ()),
    "eo-ne-no": (dict(nx=15, ny=11, nz=7, periodic=False, walls=_walls, mech="burke9"), {"solver.small": 0},
                 ("k_bcg_eo",), ()),
    "jacobi-bicgstab": (dict(nx=15, ny=12, nz=8, mech="burke9"), {"solver.small": 0}, ("k_bcg_spmv",), ("k_bcg_eo",)),
    "jacobi-forced": (BOX, {"solver.small": 0, "solver.even_odd": 0}, ("k_bcg_spmv",), ("k_bcg_eo",)),
    "one-workgroup": (BOX, {"amg.coarsest_size": 64}, ("k_bcg_small", "k_pcg_small"), ("k_bcg_eo", "k_cg_spmv")),
    "one-workgroup-f64": (BOX, {"amg.coarsest_size": 64, "amg.precision": 64}, ("k_pcg_small",), ("k_cg_spmv",)),
    "pcg-ell": (BOX, {"solver.small": 0, "pcg.face_form": 0}, ("k_cg_spmv",), ()),
    "pcg-unfused": (BOX, {"solver.small": 0, "pcg.fuse_l0": 0}, ("k_cg_x",), ("k_cg_x_smooth",)),
    "pcg-jacobi": (BOX, {"solver.small": 0}, ("k_cg_x",), ("k_cg_x_smooth", "k_vtail")),
    "amg-tail": (BIG, {}, ("k_vtail", "k_cg_x_smooth"), ()),
    "amg-f64-notail": (BIG, {"amg.precision": 64, "amg.tail": 0}, ("k_cg_spmv",), ("k_vtail",)),
    # the distorted box is still a hex box in blockMesh order to the library's face walk (topology, not geometry):
    # renumbered (RCM), its rows carry explicit columns and hex_dims() is (0, 0, 0) -- no FaceOp, no computed walk
    "non-hex": (dict(periodic=False, walls=_walls, distorted=True, renumber="rcm", mech="burke9"), {"solver.small": 0},
                (), ()),
    "mixed-bcs": (dict(periodic=False, walls=_mixed_walls, mixed=True, mech="burke9"), {"solver.small": 0}, (), ()),
    "gri53": (dict(nx=16, ny=12, nz=8, mech="gri53"), {"solver.small": 0}, ("k_bcg_eo",), ()),
}


def _unstructured(name):
    """kwargs of _case for a mesh of tests/unstructured_meshes.py (built when the case runs)"""
    def mesh():
        import unstructured_meshes as um
        return um.get(name)
    return dict(periodic=False, walls=_walls, mech="burke9", mesh=mesh)


# prisms (W = 5), prisms and hexahedra (W = 6, not a hex box), a 2:1 refined box (W = 9): none of them 2-colours, so
# the batched BiCGStab keeps the Jacobi path; the AMG is coarsened to 64 cells so that these sizes have levels
UNSTRUCTURED = {"solver.small": 0, "amg.coarsest_size": 64}
CASES.update({
    "prisms": (_unstructured("prisms"), UNSTRUCTURED, ("k_bcg_spmv", "k_cg_spmv"), ("k_bcg_eo", "k_bcg_small", "k_pcg_small")),
    "hexprism": (_unstructured("hexprism"), UNSTRUCTURED, ("k_bcg_spmv", "k_cg_spmv"), ("k_bcg_eo", "k_bcg_small", "k_pcg_small")),
    "refined": (_unstructured("refined"), UNSTRUCTURED, ("k_bcg_spmv", "k_cg_spmv"), ("k_bcg_eo", "k_bcg_small", "k_pcg_small")),
    "refined-one-workgroup": (_unstructured("refined"), {"amg.coarsest_size": 64}, ("k_bcg_small", "k_pcg_small"),
                              ("k_bcg_eo", "k_bcg_spmv", "k_cg_spmv")),
    "refined-dilu": (_unstructured("refined"), dict(UNSTRUCTURED, **{"amg.smoother": 1}), ("k_bcg_spmv", "k_cg_spmv", "k_dilu_fwd"),
                     ("k_bcg_eo", "k_cg_x_smooth", "k_vtail", "k_pcg_small")),
})
UNSTRUCTURED_W = {"prisms": 5, "hexprism": 6, "refined": 9}


@pytest.mark.parametrize("name", list(CASES))
def test_solver_paths_report_the_true_residual(name, monkeypatch):
    from dfmi import case, lib
    kw, opts, ran, not_ran = CASES[name]
    for k, v in opts.items():
        monkeypatch.setitem(lib.DEFAULT_OPTIONS, k, v)
    if callable(kw.get("mesh")):
        kw = dict(kw, mesh=kw["mesh"]())
    ctx, m, t, st, pt, inert, dt = _case(**kw)
    if name == "pcg-jacobi":
        ctx.set_preconditioner("p", "jacobi")
    if name == "non-hex":
        assert ctx.hex_dims() == (0, 0, 0)
    W = _ell_width(m)
    if name.split("-")[0] in UNSTRUCTURED_W:
        assert ctx.hex_dims() == (0, 0, 0) and W == UNSTRUCTURED_W[name.split("-")[0]]
    st = _audit_state(ctx, m, t, st, inert, own_species=name == "gri53")
    # 1-3 at the production tolerance, with the path's kernels counted
    ctx.kernel_timer(TIMED)
    A = _sequence(ctx, m, t, pt, inert, name, *PRODUCTION, W)
    n = {k: ctx.kernel_time(k)[1] for k in TIMED.split(",")}
    ctx.kernel_timer("")
    print(name, "launches", n)
    assert all(n[k] > 0 for k in ran), (name, n)
    assert all(n[k] == 0 for k in not_ran), (name, n)
    if name == "gri53":   # 52 systems converging at different iterations: each one's own true residual met the
        rels = [a["rel"] for a in A["Y"]]     # tolerance (assertion 2), and they are 52 different solves
        print("gri53 Y res_true/res0_true: min %.3e median %.3e max %.3e, %d distinct" %
              (min(rels), float(np.median(rels)), max(rels), len(set(rels))))
        assert len(rels) == 52 and len(set(rels)) > 26, rels
    # 1-3 at 1e-9, and the keep exit on each converged system
    case.push_state(ctx, st)
    _sequence(ctx, m, t, pt, inert, name, *TIGHT, W, keep=True)
    # the iteration cap
    _capped(ctx, m, t, pt, inert, name, st, W)
    ctx.close()


def test_flame1d_pressure_reports_the_true_residual():
    """the 1D flame's p system (880 cells, W = 2, waveTransmissive outlet) in the one-workgroup PCG, chemistry off;
    its species have exact zeros, so only p is audited"""
    from dfmi import case
    from test_gpu_flame1d import _setup
    ctx, m, t, ym, mech, pt, inert, dt, bv = _setup()
    ctx.chem_set_options(0)
    ctx.call("pre_time_step")
    st = case.pull_state(ctx, m, t.S)
    W = _ell_width(m)
    assert W == 2
    ctx.kernel_timer(TIMED)
    _sequence(ctx, m, t, pt, inert, "flame1d", *PRODUCTION, W, eqns=("U", "p"), audited=("p",))
    n = {k: ctx.kernel_time(k)[1] for k in TIMED.split(",")}
    ctx.kernel_timer("")
    assert n["k_pcg_small"] > 0 and n["k_cg_spmv"] == 0, n
    case.push_state(ctx, st)
    _sequence(ctx, m, t, pt, inert, "flame1d", *TIGHT, W, eqns=("U", "p"), audited=("p",), keep=True)
    _capped(ctx, m, t, pt, inert, "flame1d", st, W, eqns=("U", "p"), audited=("p",))
    ctx.close()


_HUB = [700]


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("dims,decomp", [((8, 6, 4), (2, 1, 1)), ((8, 6, 4), (2, 2, 2)), ((12, 6, 4), (3, 1, 1))])
def test_decomposed_solves_report_the_true_global_residual(dims, decomp, overlap):
    """Several ranks on one card (the in-process transport, threaded as test_gpu_multirank._run): every rank runs
    the same sequence at the production tolerance and returns its parts, x0 and x; the global system is assembled
    here (solver_audit.assemble_ranks) and 1-3 hold for the global norms; every rank reports identical stats. Covers
    the single-reduction PCG (k_cgcg_*), the even-odd stop test deferred to k_eo_c, the part-1 / part-2 row sets of
    the overlapped halos, and (3, 1, 1) on 12 cells: neighbouring ranks' colourings flipped."""
    from dfmi import case, lib
    from dfmi.lib import Context
    from dfmi.mesh import hex_box, global_cell_ids
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    nx, ny, nz = dims
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
    inert = ym["species"].index("N2")
    dt = 1e-6
    tol, mi, mi_p = PRODUCTION
    mg = hex_box(nx, ny, nz, lengths=(L,) * 3, gradings=(1.0, 1.3, 1.0))
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    f["Y"] = _positive_species(mg.cell_centres, f["Y"], inert)
    nr = int(np.prod(decomp))
    meshes = [hex_box(nx, ny, nz, lengths=(L,) * 3, gradings=(1.0, 1.3, 1.0), decomp=decomp, rank=r) for r in range(nr)]
    gids = [global_cell_ids(mm, nx, ny) for mm in meshes]
    pts = [case.default_patch_types(mm) for mm in meshes]
    out, err = [None] * nr, [None] * nr
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            m, g = meshes[r], gids[r]
            c = Context(0)
            case.setup_context(c, m, t, inert, dt, pts[r], comm={"hub": hub, "nranks": nr, "rank": r})
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            c.call("pre_time_step")
            for e in ("U", "Y", "E"):
                c.set_solver(e, mi, tol)
            c.set_solver("p", mi_p, tol)
            c.kernel_timer("k_bcg_eo")
            o = {}
            for eqn in ("U", "Y", "E", "p"):
                if eqn == "p":
                    c.call("U_get_HbyA")
                o[eqn] = _solve(c, m, t.S, inert, eqn)
            o["eo"] = c.kernel_time("k_bcg_eo")[1]
            c.kernel_timer("")
            out[r] = o
            c.close()
        except Exception as e:   # surfaced below
            err[r] = e

    prev = os.environ.get("DFMI_HALO_OVERLAP")
    os.environ["DFMI_HALO_OVERLAP"] = str(overlap)
    th = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    if prev is None:
        os.environ.pop("DFMI_HALO_OVERLAP", None)
    else:
        os.environ["DFMI_HALO_OVERLAP"] = prev
    assert not any(x.is_alive() for x in th), "decomposed run hung"
    for e in err:
        if e is not None:
            raise e
    assert all(o["eo"] > 0 for o in out), [o["eo"] for o in out]
    W = max(_ell_width(mm) for mm in meshes)
    C = mg.n_cells
    for eqn in ("U", "Y", "E", "p"):
        stats = out[0][eqn][3]
        assert all(out[r][eqn][3] == stats for r in range(nr)), (eqn, [out[r][eqn][3] for r in range(nr)])
        per_rank = [_split(meshes[r], eqn, out[r][eqn][0], t.S, inert) for r in range(nr)]
        nsys = len(per_rank[0])
        systems = [assemble_ranks(meshes, gids, [pts[r][PT_KEY[eqn]] for r in range(nr)],
                                  [per_rank[r][s] for r in range(nr)]) for s in range(nsys)]
        X0, X = np.zeros((nsys, C)), np.zeros((nsys, C))
        for r in range(nr):
            X0[:, gids[r]] = out[r][eqn][1]
            X[:, gids[r]] = out[r][eqn][2]
        _check(f"ranks{decomp} overlap {overlap} {eqn}", systems, X0, X, stats, tol, mi_p if eqn == "p" else mi, W)


def teardown_module(module):
    """the figures of DESIGN.md's "Solver audit" table"""
    for label, tol, it, rel_true, rel_rep, g in ROWS:
        print(f"AUDIT | {label} | {it} | {rel_true:.3e} | {rel_rep:.3e} | {g:.2g}")
