"""The solver audit's own arithmetic (tests/solver_audit.py, oracle.ldu_system), on the CPU: the COO residual in
np.longdouble against a dense evaluation, against the oracle's exact solve and against a known perturbation,
and the several-rank assembler against the undecomposed system it is cut from."""
import numpy as np
import pytest

from solver_audit import LD, U53, assemble_ranks, audit, norm2, true_residual

L3 = (2 * np.pi * 1e-3,) * 3


def _mesh(walls):
    from dfmi.mesh import hex_box, FIXED_VALUE
    m = hex_box(6, 5, 4, lengths=L3, periodic=(not walls,) * 3, gradings=(1.0, 1.4, 1.0))
    types = m.patch_types(0).copy()
    if walls:   # zeroGradient walls with one fixedValue pair
        types[[i for i, p in enumerate(m.patches) if p.name in ("left", "right")]] = FIXED_VALUE
    return m, types


def _random_ldu(m, seed):
    """non-symmetric, diagonally dominant LDU parts with random boundary coefficients"""
    rng = np.random.default_rng(seed)
    F, C, B = m.n_faces, m.n_cells, m.n_boundary_slots
    lower = -rng.uniform(0.2, 1.0, F)
    upper = -rng.uniform(0.2, 1.0, F) * rng.choice([1.0, -0.5], F)
    ic = rng.uniform(0.1, 1.0, B)
    bc = rng.uniform(-1.0, 1.0, B)
    off = np.zeros(C)
    np.add.at(off, m.neighbour, np.abs(lower))
    np.add.at(off, m.owner, np.abs(upper))
    np.add.at(off, m.boundary_arrays()[4], np.abs(bc))
    diag = 1.2 * off + rng.uniform(0.5, 1.0, C)
    source = rng.standard_normal(C)
    return lower, upper, diag, source, ic, bc


def _dense(system, n):
    rows, cols, vals, b = system
    A = np.zeros((n, n), dtype=LD)
    np.add.at(A, (rows, cols), np.asarray(vals, dtype=LD))
    return A, np.asarray(b, dtype=LD)


def _oracle(m, types, es80):
    import oracle as O
    t, _ = es80
    pt = {k: types for k in ("U", "Y", "he", "p", "T")}
    return O.Oracle(m, t, {}, pt, 0, 1e6)


@pytest.mark.parametrize("walls", [False, True], ids=["periodic", "walls"])
def test_true_residual_and_floors(walls, es80):
    import oracle as O
    from test_gpu_parity import _ell_width
    m, types = _mesh(walls)
    parts = _random_ldu(m, 11 + walls)
    system = O.ldu_system(m, types, *parts)
    rows, cols, vals, b = system
    n = m.n_cells
    W = _ell_width(m)
    assert abs(vals[rows != cols]).min() > 0 and (rows >= 0).all() and (cols >= 0).all()
    # the folds of k_ell_build: coupled slots are matrix entries, the others go to the right-hand side
    n_coupled = m.n_coupled_slots
    assert rows.shape[0] == 2 * m.n_faces + n + n_coupled
    assert (n_coupled > 0) == (not walls)
    if walls:
        assert np.abs(b - parts[3]).max() > 0
    A, bl = _dense(system, n)
    assert (A != A.T).any()
    rng = np.random.default_rng(3)
    x = rng.standard_normal(n) * 10.0
    r, scale = true_residual(rows, cols, vals, b, x)
    mag = np.abs(A) @ np.abs(x.astype(LD)) + np.abs(bl)
    ref = bl - A @ x.astype(LD)
    assert r.dtype == LD
    assert float((np.abs(r - ref) / mag).max()) <= 1e-17
    assert abs(scale - norm2(mag)) <= 1e-15 * scale
    # the oracle's exact solve: its residual is one fp64 evaluation's rounding
    xs = _oracle(m, types, es80).solve_ldu(*parts, "p")
    a = audit(system, xs, xs, 1e-5, 0, W)
    assert a["floor0"] == (W + 3) * U53 * true_residual(rows, cols, vals, b, xs)[1]
    assert a["floor"] == a["floor0"]
    assert 0 < a["res0"] < a["floor0"], a
    assert a["res0"] == a["res"]
    # x* + e: the residual is -A e to rounding
    e = 1e-3 * np.abs(xs).max() * rng.standard_normal(n)
    xp = xs + e
    ee = xp.astype(LD) - xs.astype(LD)          # the perturbation fp64 actually applied
    rp, _ = true_residual(rows, cols, vals, b, xp)
    rs, _ = true_residual(rows, cols, vals, b, xs)
    Ae = A @ ee
    assert float((np.abs(rp - (rs - Ae)) / mag).max()) <= 1e-17
    a2 = audit(system, xs, xp, 1e-5, 7, W)
    assert abs(a2["res"] - norm2(Ae)) <= a["floor0"]
    assert a2["res"] > 1e6 * a2["floor"]         # a solver that stopped this early would be seen
    assert a2["floor"] >= 8 * a["floor0"] * (1 - 1e-12)


@pytest.mark.parametrize("decomp", [(2, 1, 1), (2, 2, 2)])
def test_rank_assembler_reproduces_undecomposed_system(decomp):
    import oracle as O
    import scipy.sparse as sp
    from dfmi.mesh import hex_box, global_cell_ids
    nx, ny, nz = 8, 6, 4
    mg = hex_box(nx, ny, nz, lengths=L3, gradings=(1.0, 1.3, 1.0))
    tg = mg.patch_types(0)
    gparts = _random_ldu(mg, 5)
    grows, gcols, gvals, gb = O.ldu_system(mg, tg, *gparts)
    n = mg.n_cells
    Ag = sp.coo_matrix((gvals, (grows, gcols)), shape=(n, n)).tocsr()
    assert Ag.nnz == grows.shape[0]              # no duplicate entries: every lookup below is one coefficient
    nr = int(np.prod(decomp))
    meshes = [hex_box(nx, ny, nz, lengths=L3, gradings=(1.0, 1.3, 1.0), decomp=decomp, rank=r) for r in range(nr)]
    gids = [global_cell_ids(mm, nx, ny) for mm in meshes]
    assert np.array_equal(np.sort(np.concatenate(gids)), np.arange(n))
    rng = np.random.default_rng(9)

    def coef(r, c):
        return np.asarray(Ag[r, c]).ravel()

    parts, types = [], []
    for r, m in enumerate(meshes):
        g = gids[r]
        lower = coef(g[m.neighbour], g[m.owner])
        upper = coef(g[m.owner], g[m.neighbour])
        assert (lower != 0).all() and (upper != 0).all()
        B = m.n_boundary_slots
        ic = rng.uniform(0.1, 1.0, B)
        bc = rng.standard_normal(B)              # secondary processor slots keep this noise: never read
        bfc = m.boundary_arrays()[4]
        off = np.concatenate([[0], np.cumsum([p.slots for p in m.patches])])
        dsum = np.zeros(m.n_cells)
        for pi, p in enumerate(m.patches):
            sl = slice(off[pi], off[pi] + p.size)
            if p.kind == "cyclic":
                q = p.neighbour_patch
                partner = g[bfc[off[q]:off[q] + p.size]]
            else:
                assert p.kind in ("processor", "processorCyclic")
                pc = np.asarray(p.nbr_cells_global)
                partner = np.array([gids[a][b_] for a, b_ in zip(pc // m.n_cells, pc % m.n_cells)])
            bc[sl] = -coef(g[p.face_cells], partner)
            assert (bc[sl] != 0).all()
            np.add.at(dsum, p.face_cells, ic[sl])
        diag = Ag.diagonal()[g] - dsum
        parts.append((lower, upper, diag, gb[g], ic, bc))
        types.append(m.patch_types(0))
    rows, cols, vals, b = assemble_ranks(meshes, gids, types, parts)
    assert rows.shape[0] == grows.shape[0]
    assert np.array_equal(b, gb)
    x = rng.standard_normal(n)
    r1, s1 = true_residual(rows, cols, vals, b, x)
    r0, s0 = true_residual(grows, gcols, gvals, gb, x)
    # the diagonal is re-folded per rank ((D - sum ic) + ic): one rounding of D per slot
    assert float(np.abs(r1 - r0).max()) <= 8 * U53 * np.abs(Ag.diagonal()).max() * np.abs(x).max()
    assert abs(s1 - s0) <= 1e-14 * s0
