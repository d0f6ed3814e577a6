"""An audit of the linear solvers' reported residuals from outside the library.

`dfmi_solver_stats` returns what the solver kernels kept: the norm of a residual that a recurrence carried
through the iteration (r -= alpha q, r = s - omega t, the even-odd path's reduced ||D r||). This module
rebuilds the system A x = b from the LDU parts and boundary coefficients the ABI hands out
(oracle.ldu_system: the same fold the solver rows are built from) and evaluates b - A x itself, in
np.longdouble from the COO triplets, so nothing of the library's (or SciPy's) matrix-vector product is
trusted. The bounds it compares against are derived, not measured:

  floor0 = (W + 3) 2^-53 || |A||x0| + |b| ||_2
      one fp64 evaluation of a residual, first order: a row is a sum of at most W + 1 products and the
      right-hand side (W + 1 additions), each product rounded once -- (W + 3) u |A||x| + |b| per row with
      u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 and eq. 3.5);
  floor  = (iters + 1) (W + 3) 2^-53 || |A| max(|x0|, |x|) + |b| ||_2
      the drift between a recurrence residual and the true one after `iters` updates: each update adds one
      such rounding term at the size of the iterate (Greenbaum, SIAM J. Matrix Anal. Appl. 18 (1997),
      "Estimating the attainable accuracy of recursively computed residual methods"), the iterates bounded
      here by max(|x0|, |x|) entry by entry.

W is the ELL width (coupling entries of the busiest row).
"""
import numpy as np

U53 = 2.0 ** -53
LD = np.longdouble


def true_residual(rows, cols, vals, b, x):
    """(b - A x, || |A||x| + |b| ||_2) of the COO system, accumulated in np.longdouble"""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    v = np.asarray(vals, dtype=LD); xl = np.asarray(x, dtype=LD); bl = np.asarray(b, dtype=LD)
    prod = v * xl[cols]
    ax = np.zeros(bl.shape[0], dtype=LD)
    np.add.at(ax, rows, prod)
    mag = np.abs(bl).copy()
    np.add.at(mag, rows, np.abs(prod))
    return bl - ax, float(np.sqrt((mag * mag).sum()))


def norm2(r):
    r = np.asarray(r, dtype=LD)
    return float(np.sqrt((r * r).sum()))


def audit(system, x0, x, tol, iters, W):
    """system: (rows, cols, vals, b). Returns the true initial and final residual norms, the rounding floors
    above and `bound` = tol res0 + floor, what an honestly converged solve's true residual stays below."""
    rows, cols, vals, b = system
    r0, s0 = true_residual(rows, cols, vals, b, x0)
    r1, _ = true_residual(rows, cols, vals, b, x)
    _, sm = true_residual(rows, cols, vals, b, np.maximum(np.abs(x0), np.abs(x)))
    res0, res = norm2(r0), norm2(r1)
    floor0 = (W + 3) * U53 * s0
    floor = (iters + 1) * (W + 3) * U53 * sm
    return {"res0": res0, "res": res, "floor0": floor0, "floor": floor, "bound": tol * res0 + floor,
            "rel": res / res0 if res0 > 0 else 0.0}


def assemble_ranks(meshes, gids, ptypes, parts):
    """The undecomposed system from every rank's parts. meshes[r]: the rank's block (hex_box(..., decomp=,
    rank=r)); gids[r]: its cells' ids in the undecomposed numbering (dfmi.mesh.global_cell_ids); ptypes[r]: the
    field's per-patch codes on rank r; parts[r]: (lower, upper, diag, source, ic, bc) of that rank. Internal
    faces and cyclic slots as oracle.ldu_system folds them; a processor patch's primary slot i (the first
    p.size of its 2 p.size) is the entry -bc[slot] at row p.face_cells[i] against the peer's cell
    p.nbr_cells_global[i] = peer_rank * C_local + local id. Returns (rows, cols, vals, b) in global ids."""
    from oracle import ldu_system
    R, Cc, V = [], [], []
    n = int(sum(m.n_cells for m in meshes))
    b = np.zeros(n)
    for r, m in enumerate(meshes):
        rows, cols, vals, bl = ldu_system(m, ptypes[r], *parts[r])
        g = np.asarray(gids[r], dtype=np.int64)
        types = np.asarray(ptypes[r])
        peer_cols = [np.asarray(p.nbr_cells_global, dtype=np.int64) for pi, p in enumerate(m.patches)
                     if p.kind in ("processor", "processorCyclic") and types[pi] != 3 and p.size]
        across = cols < 0
        gc = np.empty(cols.shape[0], dtype=np.int64)
        gc[~across] = g[cols[~across]]
        if across.any():
            pc = np.concatenate(peer_cols)
            assert pc.shape[0] == int(across.sum())
            peer, loc = pc // m.n_cells, pc % m.n_cells
            gc[across] = np.array([gids[pr][lc] for pr, lc in zip(peer, loc)], dtype=np.int64)
        R.append(g[rows]); Cc.append(gc); V.append(vals)
        b[g] = bl
    return np.concatenate(R), np.concatenate(Cc), np.concatenate(V), b


# ---- the audit of one solve through the ABI (dfmi.lib.Context)
ROWS = []          # (label, tol, iters, rel_true, rel_reported, gap / floor) of every checked solve


def matrix_parts(ctx, m, eqn, S):
    """the LDU parts and boundary coefficients of `eqn` as dfmi_get_matrix holds them (U: source_solve)"""
    C, F, B = m.n_cells, m.n_faces, m.n_boundary_slots
    nf, nc, nb = {"U": (1, 3, 3), "Y": (S, S, S), "E": (1, 1, 1), "p": (1, 1, 1)}[eqn]
    g = lambda part, n: ctx.get_matrix(eqn, part, n)
    return {"lower": g("lower", nf * F), "upper": g("upper", nf * F), "diag": g("diag", (S if eqn == "Y" else 1) * C),
            "source": g("source_solve" if eqn == "U" else "source", nc * C),
            "ic": g("internal_coeffs", nb * B), "bc": g("boundary_coeffs", nb * B)}


def split_systems(m, eqn, parts, S, inert):
    """per system (lower, upper, diag, source, ic, bc) of one rank's parts"""
    C, F, B = m.n_cells, m.n_faces, m.n_boundary_slots
    p = parts
    if eqn == "U":
        return [(p["lower"], p["upper"], p["diag"], p["source"][k * C:(k + 1) * C], p["ic"][k * B:(k + 1) * B],
                 p["bc"][k * B:(k + 1) * B]) for k in range(3)]
    if eqn == "Y":
        return [(p["lower"][s * F:(s + 1) * F], p["upper"][s * F:(s + 1) * F], p["diag"][s * C:(s + 1) * C],
                 p["source"][s * C:(s + 1) * C], p["ic"][s * B:(s + 1) * B], p["bc"][s * B:(s + 1) * B])
                for s in range(S) if s != inert]
    return [(p["lower"], p["upper"], p["diag"], p["source"], p["ic"], p["bc"])]


def check(label, systems, X0, X, stats, tol, max_iter, W, cap=False):
    """One solve's systems (systems[s] = (rows, cols, vals, b), X0[s], X[s]) against its dfmi_solver_stats, which
    reports the worst system: the reconstruction check |max_s res0_true - res0_reported| <= max_s floor0_s; then,
    converged (iters < max_iter), every res_true_s <= tol res0_true_s + floor_s -- or, with `cap` and iters == max_iter,
    res_true_s < res0_true_s; and the honest report |max_s rel_true_s - rel_reported| <= max_s floor_s /
    res0_true_s (per system |rel_true - rel_reported| res0 <= floor, so the maxima differ by no more than the
    largest such allowance). Every figure is printed before it is asserted. Returns the per-system audits."""
    it, res0_rep, rel_rep = stats
    A = [audit(sy, X0[s], X[s], tol, it, W) for s, sy in enumerate(systems)]
    res0_true = max(a["res0"] for a in A)
    rel_true = max(a["rel"] for a in A)
    gap = abs(rel_true - rel_rep)
    allow = max(a["floor"] / a["res0"] for a in A if a["res0"] > 0)   # (a system with b - A x0 = 0 has rel = 0)
    print(f"{label}: iters {it}/{max_iter} res0 true {res0_true:.6e} reported {res0_rep:.6e} "
          f"floor0 {max(a['floor0'] for a in A):.2e} | rel true {rel_true:.4e} reported {rel_rep:.4e} "
          f"gap/floor {gap / allow:.3g} | worst res/bound {max(a['res'] / a['bound'] for a in A):.3g}")
    ROWS.append((label, tol, it, rel_true, rel_rep, gap / allow))
    assert abs(res0_true - res0_rep) <= max(a["floor0"] for a in A), (label, "reconstruction", res0_true, res0_rep)
    assert res0_true > 100 * max(a["floor0"] for a in A), (label, "the initial residual is rounding: nothing to solve")
    if cap and it == max_iter:
        assert all(a["res"] < a["res0"] for a in A), (label, [(a["res"], a["res0"]) for a in A])
    else:   # (a capped solve that converged before its cap is held to its tolerance; the caller lowers the cap)
        assert 0 < it < max_iter, (label, it)
        bad = [(s, a["res"], a["bound"]) for s, a in enumerate(A) if a["res"] > a["bound"]]
        assert not bad, (label, "stopped before the true residual met the tolerance", bad)
    assert gap <= allow, (label, "reported residual is not the true one", rel_true, rel_rep, allow)
    return A
