"""The multicolour DILU smoother of the pressure AMG V-cycle (option amg.smoother = 1, amg.hip k_dilu_*) on the GPU.

M = (E + L) E^-1 (E + U) over a greedy colouring, L / U a row's couplings to lower / higher colours and
E_i = D_i - sum_{j in L(i)} a_ij^2 / E_j. Checked here from outside the library: the option's life cycle, the
default path left bitwise alone, the colouring and the factor against a NumPy recurrence on the system rebuilt
from dfmi_get_matrix (oracle.ldu_system), the V-cycle as a symmetric positive-definite operator
(dfmi_amg_apply), the p solve's true residual (tests/solver_audit.py) with no more PCG iterations than weighted
Jacobi, a matrix that moves from step to step (1D flame), the reuse window (the factor stays with the operator
it was built from) and two ranks.

Meshes: (a) hex_box(20, 20, 14) periodic, y-grading 1.3 (test_gpu_amg_tail's, 5600 cells: three levels);
(b) hex_box(21, 20, 14) periodic (the odd periodic direction forces a third colour); (c) hex_box(11, 9, 7) with
the audit test's mixed walls (693 cells: the one-workgroup small solve has to be bypassed); (d) the 2:1 refined box
of tests/unstructured_meshes.py with the same walls (243 cells, W = 9, a graph with triangles; coarsened to 64 cells
so that it has levels).
"""
import os
import threading

import numpy as np
import pytest

from conftest import GOLDEN
from solver_audit import assemble_ranks, check, matrix_parts, split_systems

pytestmark = pytest.mark.gpu

L = 2 * np.pi * 1e-3
DILU_KERNELS = ("k_dilu_factor", "k_dilu_fwd", "k_dilu_bwd", "k_dilu_small")
JACOBI_ONLY = ("k_vtail", "k_cg_x_smooth", "k_pcg_small")
U53, U24 = 2.0 ** -53, 2.0 ** -24


class _options:
    """dfmi.lib.DEFAULT_OPTIONS set around the creation of a context"""

    def __init__(self, opts):
        self.opts = dict(opts)

    def __enter__(self):
        from dfmi.lib import DEFAULT_OPTIONS
        DEFAULT_OPTIONS.update(self.opts)

    def __exit__(self, *a):
        from dfmi.lib import DEFAULT_OPTIONS
        for k in self.opts:
            DEFAULT_OPTIONS.pop(k, None)


def _audit_case(mesh, opts):
    """meshes (a), (b), (c) through test_gpu_parity._case with the audit test's state (positive species, RR = 0, a
    pressure with a gradient): (ctx, m, t, st, pt, inert, W)"""
    from test_gpu_parity import _case, _ell_width
    from test_gpu_solver_audit import _audit_state, _mixed_walls
    kw = {"a": dict(nx=20, ny=20, nz=14, gradings=(1.0, 1.3, 1.0), mech="burke9"),
          "b": dict(nx=21, ny=20, nz=14, gradings=(1.0, 1.0, 1.0), mech="burke9"),
          "c": dict(nx=11, ny=9, nz=7, periodic=False, walls=_mixed_walls, mixed=True, mech="burke9"),
          "d": dict(periodic=False, walls=_mixed_walls, mixed=True, mech="burke9")}[mesh]
    if mesh == "d":
        import unstructured_meshes as um
        kw["mesh"] = um.get("refined")
        opts = dict(opts, **{"amg.coarsest_size": 64})
    with _options(opts):
        ctx, m, t, st, pt, inert, dt = _case(**kw)
    st = _audit_state(ctx, m, t, st, inert)
    return ctx, m, t, st, pt, inert, _ell_width(m)


def _tgv(opts, dims=(20, 20, 14)):
    """mesh (a) with the Taylor-Green fields, as test_gpu_amg_tail sets it up: (ctx, m, t, pt, inert)"""
    from dfmi.lib import Context
    from dfmi.mesh import hex_box
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi import case
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
    m = hex_box(*dims, lengths=(L,) * 3, gradings=(1.0, 1.3, 1.0), periodic=(True,) * 3)
    inert = ym["species"].index("N2")
    with _options(opts):
        ctx = Context(0)
    pt = case.setup_context(ctx, m, t, inert, 1e-6, case.default_patch_types(m))
    f = case.tgv_fields(m, ym["species"], kernel_radius=1.2e-3)
    case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"])
    ctx.call("pre_time_step")
    return ctx, m, t, pt, inert


def _up_to_p(ctx, tol=1e-5):
    """U, Y, E solved at the production settings and HbyA formed: the next p_process solves a physical p system
    (dfmi_time_step on _case's randomly perturbed old-time fields does not: test_non_m_matrix_is_reported)"""
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 20, 1e-5)
        ctx.call(e + "_process")
    ctx.set_solver("p", 3000, tol)
    ctx.call("U_get_HbyA")


def _p_system(ctx, m, t, pt, inert):
    """the p system of the last solve, from dfmi_get_matrix: (rows, cols, vals, b)"""
    from oracle import ldu_system
    parts = matrix_parts(ctx, m, "p", t.S)
    (p,) = split_systems(m, "p", parts, t.S, inert)
    return ldu_system(m, pt["p"], *p)


def _recurrence(system, n, colour, u):
    """E of the DILU recurrence, colour by colour in float64, from the COO system with its entries first rounded
    to the V-cycle's precision (u = 2^-53: unchanged; 2^-24: float32). Returns (E, off-diagonal rows, cols)."""
    rows, cols, vals, _ = system
    rnd = (lambda v: v) if u == U53 else (lambda v: v.astype(np.float32).astype(np.float64))
    off = (rows != cols) & (cols >= 0)
    D = np.zeros(n)
    np.add.at(D, rows[~off & (cols >= 0)], vals[~off & (cols >= 0)])
    D = rnd(D)
    r, c, a = rows[off], cols[off], rnd(vals[off])
    assert len(set(zip(r.tolist(), c.tolist()))) == r.size, "a (row, column) pair stored twice"
    E = D.copy()
    for k in range(1, int(colour.max()) + 1):
        sel = (colour[r] == k) & (colour[c] < k)
        s = np.zeros(n)
        np.add.at(s, r[sel], a[sel] * a[sel] / E[c[sel]])
        rows_k = colour == k
        E[rows_k] = D[rows_k] - s[rows_k]
    return E, r, c


def _check_factor(label, system, n, colour, E, W, u):
    """Colouring and factor of level 0 against the recurrence.

    Bound. In precision u, E_i is D_i less at most W quotients a_ij^2 / E_j: W + 1 terms, every quotient rounded
    twice (the square, the division), every subtraction once, so E_i's own arithmetic is off by at most
    3 (W + 1) u relative to the terms' magnitudes, first order -- and the terms sum to less than D_i, which for
    this diagonally dominant matrix is within a small factor of E_i. On top, every quotient carries the relative
    error of E_j, a row of an EARLIER colour: one such inherited error per term, the terms again summing to less
    than D_i. By induction a row of colour c (0-based) is within (c + 1) * 4 (W + 1) u of the exact recurrence,
    the 4 in place of 3 covering the summation order of D_i itself (diag + internalCoeffs) and the ratio
    D_i / E_i. The NumPy side runs the same recurrence in float64 on the same (rounded) inputs; its own error is
    of the same form with u = 2^-53 and sits inside the bound."""
    ref, r, c = _recurrence(system, n, colour, u)
    assert not np.any(colour[r] == colour[c]), (label, "a stored coupling joins two rows of one colour")
    ncol = int(colour.max()) + 1
    assert colour.min() == 0 and ncol <= W + 1, (label, ncol, W)
    assert E.min() > 0, (label, E.min())
    err = np.abs(E - ref) / np.abs(ref)
    bound = u * 4 * (W + 1) * (colour + 1)
    print(f"{label}: {ncol} colours {np.bincount(colour).tolist()} E in [{E.min():.3e}, {E.max():.3e}] "
          f"worst err/bound {float((err / bound).max()):.3g} (max rel err {float(err.max()):.3e})")
    assert np.all(err <= bound), (label, float((err / bound).max()))
    return ncol


def test_option_life_cycle():
    """default 0; 1 accepted before the first solve, refused after it; 2 refused"""
    from dfmi.lib import Context, DfmiError
    from test_gpu_parity import _case
    ctx = Context(0)
    assert ctx.get_option("amg.smoother") == 0
    with pytest.raises(DfmiError):
        ctx.set_option("amg.smoother", 2)
    assert ctx.get_option("amg.smoother") == 0
    ctx.set_option("amg.smoother", 1)
    assert ctx.get_option("amg.smoother") == 1
    ctx.close()
    ctx, m, t, st, pt, inert, dt = _case()   # (its set-up has built the solver rows already)
    assert ctx.get_option("amg.smoother") == 0
    with pytest.raises(DfmiError):   # the inspection entries before any p solve: a clean error
        ctx.amg_apply(np.zeros(m.n_cells))
    ctx.time_step(1)
    with pytest.raises(DfmiError, match="before the first solve"):
        ctx.set_option("amg.smoother", 1)
    assert ctx.get_option("amg.smoother") == 0
    ctx.close()


def test_default_path_is_bitwise_untouched():
    """amg.smoother = 0 set explicitly: bitwise the run that never sets it (two steps on (a))"""
    def run(opts):
        ctx, m, t, pt, inert = _tgv(opts)
        ctx.set_solver("p", 3000, 1e-12, 1e-300)
        its = []
        for _ in range(2):
            ctx.time_step(2)
            its.append(ctx.solver_stats("p")[0])
        out = {k: ctx.get_field(k, (m.n_cells,)) for k in ("p", "T", "rho")}
        out["U"] = ctx.get_field("U", (3, m.n_cells))
        ctx.close()
        return its, out
    ia, a = run({})
    ib, b = run({"amg.smoother": 0})
    assert ia == ib and min(ia) > 3, (ia, ib)
    for k in ("p", "T", "rho", "U"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("mesh", ["a", "b", "c", "d"])
def test_colouring_and_factor(mesh):
    """level 0 in fp64 against the recurrence (bound: _check_factor); every coarser level has E > 0 and a
    non-empty colour 0. (d): an irregular graph -- the colour count is printed and held to W + 1 only"""
    ctx, m, t, st, pt, inert, W = _audit_case(mesh, {"amg.smoother": 1, "amg.precision": 64})
    _up_to_p(ctx)
    ctx.call("p_process")
    assert 0 < ctx.solver_stats("p")[0] < 3000
    system = _p_system(ctx, m, t, pt, inert)
    colour, E = ctx.amg_smoother_info(0)
    ncol = _check_factor(f"mesh ({mesh}) level 0", system, m.n_cells, colour, E, W, U53)
    if mesh == "a":
        assert ncol == 2
    if mesh == "b":
        assert ncol == 3
    levels = ctx.amg_info()
    if mesh == "d":
        assert len(levels) >= 2 and levels[0] == (m.n_cells, 9), levels
    for l in range(1, len(levels)):
        cl, El = ctx.amg_smoother_info(l)
        print(f"mesh ({mesh}) level {l}: {levels[l]} colours {np.bincount(cl).tolist()} E min {El.min():.3e}")
        assert El.min() > 0 and np.any(cl == 0), (mesh, l)
        assert cl.max() + 1 <= levels[l][1] + 1
    ctx.close()


def test_non_m_matrix_is_reported():
    """dfmi_time_step on _case's state (old-time fields perturbed at random, which the step's own pre-time-step
    copies do not undo for phi / dpdt) assembles a p matrix with negative diagonal entries: weighted Jacobi grinds
    through it, the DILU factor has E_i <= 0 and says so where the solve's scalars are read"""
    from dfmi.lib import DfmiError
    ctx, m, t, st, pt, inert, W = _audit_case("c", {"amg.smoother": 1})
    ctx.time_step(1)
    rows, cols, vals, _ = _p_system(ctx, m, t, pt, inert)
    assert vals[rows == cols].min() < 0   # the premise: not an M-matrix
    with pytest.raises(DfmiError, match="not an M-matrix; use amg.smoother = 0"):
        ctx.solver_stats("p")
    with pytest.raises(DfmiError, match="not an M-matrix"):
        ctx.amg_smoother_info(0)
    ctx.close()


def _asym(precision, smoother):
    """worst |u'Sv - v'Su| / (|u| |Sv|) over 6 seeded pairs, S the V-cycle of the last build on (a); u'Su > 0"""
    ctx, m, t, pt, inert = _tgv({"amg.smoother": smoother, "amg.precision": precision, "amg.reuse": 0})
    ctx.time_step(2)
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(6):
        u, v = rng.standard_normal(m.n_cells), rng.standard_normal(m.n_cells)
        Su, Sv = ctx.amg_apply(u), ctx.amg_apply(v)
        assert u @ Su > 0 and v @ Sv > 0
        worst = max(worst, abs(u @ Sv - v @ Su) / (np.linalg.norm(u) * np.linalg.norm(Sv)))
    ctx.close()
    return worst


@pytest.mark.parametrize("precision", [32, 64])
def test_vcycle_is_symmetric_positive_definite(precision):
    """DILU's asymmetry stays within 32x that of the Jacobi V-cycle (the known-good path, the yardstick for
    rounding in the same precision on the same vectors: DILU makes up to 2 colours + 1 operator passes per level
    visit against 2, rounding grows at worst linearly in passes, ~5x; the rest is margin) and below 1e-3 absolutely
    (a missing backward pass or a wrong colour order gives ~0.1)."""
    jac, dilu = _asym(precision, 0), _asym(precision, 1)
    print(f"V-cycle asymmetry fp{precision}: jacobi {jac:.3e} dilu {dilu:.3e}")
    assert dilu <= 32 * jac and dilu < 1e-3, (precision, jac, dilu)


def _p_solve(mesh, smoother, tol):
    """U, Y, E at the production settings, then one audited p solve at `tol`: (iterations, kernel launches)"""
    ctx, m, t, st, pt, inert, W = _audit_case(mesh, {"amg.smoother": smoother})
    _up_to_p(ctx, tol)
    names = DILU_KERNELS + JACOBI_ONLY
    ctx.kernel_timer(",".join(names))
    x0 = ctx.get_field("p", (m.n_cells,))
    ctx.call("p_process")
    n = {k: ctx.kernel_time(k)[1] for k in names}
    ctx.kernel_timer("")
    x = ctx.get_field("p", (m.n_cells,))
    stats = ctx.solver_stats("p")
    check(f"mesh ({mesh}) smoother {smoother} p tol {tol:g}", [_p_system(ctx, m, t, pt, inert)], x0[None, :], x[None, :],
          stats, tol, 3000, W)
    ctx.close()
    return stats[0], n


@pytest.mark.parametrize("tol", [1e-12, 1e-5])
@pytest.mark.parametrize("mesh", ["a", "b", "c"])
def test_converges_honestly_and_no_slower_than_jacobi(mesh, tol):
    """the true residual (np.longdouble, solver_audit.check) meets the tolerance and is the one reported; the
    same system with weighted Jacobi needs at least as many PCG iterations; the DILU kernels ran and none of the
    Jacobi-only fused kernels did"""
    it_d, n_d = _p_solve(mesh, 1, tol)
    it_j, n_j = _p_solve(mesh, 0, tol)
    print(f"mesh ({mesh}) tol {tol:g}: p iterations dilu {it_d} jacobi {it_j}; launches {n_d}")
    assert all(n_d[k] > 0 for k in DILU_KERNELS), n_d
    assert all(n_d[k] == 0 for k in JACOBI_ONLY), n_d
    assert all(n_j[k] == 0 for k in DILU_KERNELS), n_j
    assert it_d <= it_j, (mesh, tol, it_d, it_j)


def test_flame1d_matrix_that_moves():
    """the 880-cell 1D flame (graded, waveTransmissive outlet, chemistry on): 3 steps with DILU, every p solve
    converged before max_iter to its tolerance and audited (test_gpu_amg_reuse._window audits each step).
    Measured: 47 / 45 / 52 iterations, against 19 / 20 / 21 with weighted Jacobi (DESIGN.md section 6 has the
    V-cycle's spectrum on this chain); no iteration margin is asserted here."""
    from test_gpu_flame1d import _setup
    from test_gpu_amg_reuse import _window
    with _options({"amg.smoother": 1}):
        ctx, m, t, ym, mech, pt, inert, dt, bv = _setup()
    assert ctx.get_option("amg.smoother") == 1
    ctx.chem_set_options(1, rtol=1e-6, atol=1e-10)
    its, _ = _window(ctx, m, pt, t.S, inert, "flame1d dilu", steps=3)
    it, _, rel = ctx.solver_stats("p")
    colour, E = ctx.amg_smoother_info(0)
    print("flame1d dilu p iterations per step", its, "colours", np.bincount(colour).tolist())
    assert all(0 < i < 1000 for i in its) and rel <= 1e-5
    assert colour.max() == 1 and E.min() > 0   # the 1D chain two-coloured: the DILU V-cycle was the one built
    ctx.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_reuse_window_keeps_factor_with_its_operator(precision):
    """amg.reuse_steps = 2 over 4 one-corrector steps: the operators are built on steps 1 and 3 and reused on 2
    and 4; every step's solve converges, and after step 4 the factor is still the recurrence of the matrix of
    step 3, the build it belongs to (fp32: the inputs rounded to float32 first, the bound with u = 2^-24)"""
    ctx, m, t, pt, inert = _tgv({"amg.smoother": 1, "amg.reuse_steps": 2, "amg.precision": precision})
    from test_gpu_parity import _ell_width
    built = None
    for step in range(1, 5):
        ctx.kernel_timer("k_dilu_factor")
        ctx.time_step(1)
        fac = ctx.kernel_time("k_dilu_factor")[1]
        ctx.kernel_timer("")
        it, _, rel = ctx.solver_stats("p")
        print(f"reuse window fp{precision} step {step}: p iters {it} rel {rel:.3e} factor launches {fac}")
        assert 0 < it < 1000 and rel <= 1e-5, (step, it, rel)
        assert (fac > 0) == (step in (1, 3)), (step, fac)
        if fac > 0:
            built = _p_system(ctx, m, t, pt, inert)
    colour, E = ctx.amg_smoother_info(0)
    _check_factor(f"reuse window fp{precision}", built, m.n_cells, colour, E, _ell_width(m),
                  U53 if precision == 64 else U24)
    ctx.close()


def test_two_ranks_block_dilu():
    """2 x 1 x 1 ranks of a 24 x 12 x 12 periodic box on one card (in-process transport): both ranks converge with
    equal iteration counts and the global true residual passes the audit; amg.global_coarse = 1 is refused"""
    import test_gpu_solver_audit as A
    from test_gpu_parity import _ell_width
    from dfmi import case
    from dfmi.lib import Context, DfmiError
    from dfmi.mesh import hex_box, global_cell_ids
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    nx, ny, nz, decomp, nr = 24, 12, 12, (2, 1, 1), 2
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
    inert = ym["species"].index("N2")
    tol, mi, mi_p = A.PRODUCTION
    mg = hex_box(nx, ny, nz, lengths=(L,) * 3, gradings=(1.0, 1.3, 1.0))
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    f["Y"] = A._positive_species(mg.cell_centres, f["Y"], inert)
    meshes = [hex_box(nx, ny, nz, lengths=(L,) * 3, gradings=(1.0, 1.3, 1.0), decomp=decomp, rank=r) for r in range(nr)]
    gids = [global_cell_ids(mm, nx, ny) for mm in meshes]
    pts = [case.default_patch_types(mm) for mm in meshes]
    out, err = [None] * nr, [None] * nr
    hub = A._HUB[0]; A._HUB[0] += 1

    def work(r):
        try:
            m, g = meshes[r], gids[r]
            c = Context(0)
            assert c.get_option("amg.smoother") == 1
            case.setup_context(c, m, t, inert, 1e-6, pts[r], comm={"hub": hub, "nranks": nr, "rank": r})
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            c.call("pre_time_step")
            for e in ("U", "Y", "E"):
                c.set_solver(e, mi, tol)
            c.set_solver("p", mi_p, tol)
            c.kernel_timer("k_dilu_fwd")
            o = {}
            for eqn in ("U", "Y", "E", "p"):
                if eqn == "p":
                    c.call("U_get_HbyA")
                o[eqn] = A._solve(c, m, t.S, inert, eqn)
            o["dilu"] = c.kernel_time("k_dilu_fwd")[1]
            c.kernel_timer("")
            out[r] = o
            c.close()
        except Exception as e:   # surfaced below
            err[r] = e

    with _options({"amg.smoother": 1}):
        th = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
        for x in th:
            x.start()
        for x in th:
            x.join(timeout=300)
    assert not any(x.is_alive() for x in th), "decomposed run hung"
    for e in err:
        if e is not None:
            raise e
    assert all(o["dilu"] > 0 for o in out)
    stats = out[0]["p"][3]
    assert all(out[r]["p"][3] == stats for r in range(nr)), [out[r]["p"][3] for r in range(nr)]
    assert 0 < stats[0] < mi_p
    per_rank = [split_systems(meshes[r], "p", out[r]["p"][0], t.S, inert) for r in range(nr)]
    system = assemble_ranks(meshes, gids, [pts[r]["p"] for r in range(nr)], [per_rank[r][0] for r in range(nr)])
    X0, X = np.zeros((1, mg.n_cells)), np.zeros((1, mg.n_cells))
    for r in range(nr):
        X0[:, gids[r]] = out[r]["p"][1]
        X[:, gids[r]] = out[r]["p"][2]
    check("2 ranks dilu p", [system], X0, X, stats, tol, mi_p, max(_ell_width(mm) for mm in meshes))
    # the agglomerated coarsest level and the rank-local smoother exclude each other, in either order
    c = Context(0)
    c.set_option("amg.smoother", 1)
    with pytest.raises(DfmiError, match="global_coarse"):
        c.set_option("amg.global_coarse", 1)
    c.set_option("amg.smoother", 0)
    c.set_option("amg.global_coarse", 1)
    with pytest.raises(DfmiError, match="global_coarse"):
        c.set_option("amg.smoother", 1)
    c.close()
