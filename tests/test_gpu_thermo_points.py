"""The thermo kernels against the extended-precision point reference (tests/thermo_reference.py), through Context
and the C ABI, at every species count, both implementations, both symmetry branches and the grid shapes at which
the block remap changes.

Cells and boundary slots of a walled hex_box carry the reference's test states (its classes broad, zeros, pure,
near_pure, switch_T from T; newton, jump from he) instead of a flow field:

  thermo_update_energy   every cell and slot from T
  thermo_correct         cells and zeroGradient slots (front, back) from he; fixedValue-T slots (left, right) from T

The top / down pair carries the type `empty` for every field. hex_box gives a patch of kind "empty" no slots at
all, so the pair is a wall patch given the empty type: its slots exist, hold a sentinel and must keep it.

Meshes (hex_box dimensions -> cells C, slots B; register blocks of 256 cells, cooperative blocks of 16):
  1x1x1     C = 1      B = 6      a single cell
  3x5x17    C = 255    B = 302    one under a 256-thread block (cooperative: 16 blocks, the last ragged)
  4x8x8     C = 256    B = 256    exact
  257x1x1   C = 257    B = 1030   one over, a one-cell-thick rod (cooperative: 17 blocks, remapped, 17 % 8 = 1)
  3x103x1   C = 309    B = 830    cooperative: 20 blocks, remapped, 20 % 8 = 4, 309 % 16 = 5; every species count
  5x13x67   C = 4355   B = 2542   register: 18 blocks = 17 + 3 cells, remapped, 18 % 8 = 2; cooperative: 273 blocks
The boundary pass runs on B and so gets ragged grids of its own.

Tolerances come from tests/golden/thermo_point_bounds.json (the fp64 sequential oracle against the same reference,
measured on the CPU): per class and quantity 4x the oracle's maximum, floored at 1e-13, all <= 1e-12 (asserted in
test_thermo_reference_cpu.py); rhoD where kappa_i = Wm / (Wm - X_i W_i) > 10, and on near_pure, is held to
4 c kappa_i 2^-52 with c the oracle's measured constant (near_pure's dominant species: the constant measured on them
alone, which is two orders smaller). The error is per element (thermo_reference.errors), not
relative to a field-wide scale. jump is the one class where T is not compared: the target he lies in (or within
4e-6 T_mid of) a discontinuity of h(T), so T must end within 8e-6 T_mid of the switch, everything must be finite
and every output must agree with the reference evaluated at the T the kernel returned. The energy itself is an
input there and is passed through, so it is compared bitwise with the input, and its distance to h(T returned) is
held to the size of the jump plus the slope over the stopping distance (thermo_reference.jump_he_slack) -- a
target inside the jump has no T that reproduces it more closely.
"""
import numpy as np
import pytest

import thermo_reference as R

pytestmark = pytest.mark.gpu

MESHES = {"one": (1, 1, 1), "c255": (3, 5, 17), "c256": (4, 8, 8), "rod257": (257, 1, 1), "c309": (3, 103, 1),
          "c4355": (5, 13, 67)}
OUT1 = ("T", "he", "psi", "rho", "mu", "alpha")
OUTS = ("rhoD", "hai")
SENTINEL = -7.25
FROM_T = ("broad", "zeros", "pure", "near_pure", "switch_T")
FROM_HE = ("newton", "jump")


def _cases():
    out = []
    for S in range(2, 17):
        out.append(("reg", S, True, "c309"))
    for S in (17, 18, 32, 33, 52, 53, 63, 64):
        out.append(("coop", S, True, "c309"))
    for S in (2, 3, 8, 9, 16):
        out.append(("gen", S, True, "c309"))
    for S in (8, 9):
        out.append(("reg", S, False, "c309"))
    out += [("gen", 9, False, "c309"), ("coop", 18, False, "c309"), ("coop", 64, False, "c309")]
    for mesh in ("one", "c255", "c256", "rod257"):
        out += [("reg", 9, True, mesh), ("coop", 18, True, mesh)]
    out += [("reg", 5, True, "c4355"), ("reg", 9, True, "c4355"), ("reg", 16, True, "c4355"), ("coop", 18, True, "c4355")]
    return out


def _id(c):
    return f"{c[0]}-S{c[1]}-{'sym' if c[2] else 'nonsym'}-{c[3]}"


# ------------------------------------------------------------------------------------------------ reference pools
class Pool:
    """the states of several classes side by side, with the reference evaluated once"""

    def __init__(self, t, classes):
        sts = [R.states(t, c) for c in classes]
        self.t = t
        self.cls = np.concatenate([np.full(s.n, c, dtype=object) for s, c in zip(sts, classes)])
        self.T = np.concatenate([s.T for s in sts]); self.he = np.concatenate([s.he for s in sts])
        self.p = np.concatenate([s.p for s in sts]); self.Y = np.concatenate([s.Y for s in sts], axis=1)
        self.tmid = np.concatenate([s.tmid if s.tmid is not None else np.zeros(s.n) for s in sts])
        self.n = self.T.size
        self.ref = {}
        refs = [None if s.cls == "jump" else R.reference_for(t, s) for s in sts]
        for q in ("T", "he", "psi", "rho", "mu", "alpha", "rhoD", "hai", "kappa", "X", "Wm", "cp"):
            parts = []
            for s, r in zip(sts, refs):
                shape = (t.S, s.n) if q in ("rhoD", "hai", "kappa", "X") else (s.n,)
                parts.append(np.full(shape, np.nan, dtype=R.LD) if r is None else r[q])
            self.ref[q] = np.concatenate(parts, axis=-1)


_pools: dict = {}


def _table_and_pools(S, sym):
    key = (S, sym)
    if key not in _pools:
        t = R.gri_table(S)
        if not sym:
            t = R.nonsymmetric(t)
        _pools[key] = (t, Pool(t, FROM_T), Pool(t, FROM_HE))
    return _pools[key]


@pytest.fixture(scope="module")
def bounds():
    return R.load_bounds()


# ------------------------------------------------------------------------------------------------ one case
def _context(kind, t, dims):
    from dfmi import case, lib
    from dfmi.mesh import hex_box, FIXED_VALUE, EMPTY
    m = hex_box(*dims, lengths=(1e-3 * dims[0], 1e-3 * dims[1], 1e-3 * dims[2]), periodic=(False,) * 3)
    pt = case.default_patch_types(m)
    name = [p.name for p in m.patches]
    for f in ("U", "p", "he", "K", "Y", "T", "rho"):
        pt[f] = pt[f].copy()
        for side in ("top", "down"):
            pt[f][name.index(side)] = EMPTY
    for side in ("left", "right"):
        pt["T"][name.index(side)] = FIXED_VALUE
    if kind == "gen":
        lib.DEFAULT_OPTIONS["fv.species_generic"] = 1
    try:
        ctx = lib.Context(0)
    finally:
        lib.DEFAULT_OPTIONS.pop("fv.species_generic", None)
    case.setup_context(ctx, m, t, t.S - 1, 1e-6, pt)
    assert ctx.get_option("fv.species_generic") == (1.0 if kind == "gen" else 0.0)
    slot_side = np.repeat(np.array(name, dtype=object), [p.slots for p in m.patches])
    return ctx, m, slot_side


def _fill(pool, idx):
    return {"T": pool.T[idx], "he": pool.he[idx], "p": pool.p[idx], "Y": np.ascontiguousarray(pool.Y[:, idx])}


def _push(ctx, cells, slots):
    for k in ("T", "he", "p", "Y"):
        ctx.set_field(k, cells[k])
        ctx.set_field("boundary_" + k, slots[k])


def _pull(ctx, S, C, B):
    cells = {q: ctx.get_field(q, (C,)) for q in OUT1}
    slots = {q: ctx.get_field("boundary_" + q, (B,)) for q in OUT1}
    for q in OUTS:
        cells[q] = ctx.get_field(q, (S, C))
        slots[q] = ctx.get_field("boundary_" + q, (S, B))
    return cells, slots


def _check(t, bounds, pool, idx, got, he_in, where):
    """got[q][..., k] is the evaluation of pool state idx[k]"""
    fails = []
    for cls in sorted(set(pool.cls[idx])):
        sel = np.where(pool.cls[idx] == cls)[0]
        ix = idx[sel]
        g = {q: (got[q][:, sel] if q in OUTS else got[q][sel]) for q in OUT1 + OUTS}
        for q in OUT1 + OUTS:
            assert np.isfinite(g[q]).all(), (where, cls, q)
        if cls == "jump":
            tm = pool.tmid[ix]
            assert (np.abs(g["T"] - tm) <= R.JUMP_STOP * tm).all(), (where, cls, float(np.abs(g["T"] / tm - 1).max()))
            assert np.array_equal(g["he"], he_in[sel]), (where, cls, "he is passed through")
            ref = R.evaluate(t, pool.p[ix], pool.Y[:, ix], T=g["T"])
            st = R.States("jump", False, g["T"], he_in[sel], pool.p[ix], pool.Y[:, ix], tm)
            res = np.abs(R.LD(1) * g["he"] - ref["he"]) / np.maximum(np.abs(ref["he"]), R.LD(R.R_GAS) * ref["T"] / ref["Wm"])
            slack = R.jump_he_slack(t, st, ref)
            if not (np.asarray(res, dtype=np.float64) <= slack).all():
                fails.append((where, cls, "he residual", float(np.max(np.asarray(res, dtype=np.float64) / slack))))
            ref["he"] = R.LD(1) * g["he"]
        else:
            ref = {q: pool.ref[q][..., ix] for q in pool.ref}
        e = R.errors(t, g, ref)
        for q in OUT1 + ("hai",):
            b = R.gpu_bound(bounds, cls, q)
            v = float(e[q].max())
            print(f"{where:14s} {cls:10s} {q:6s} {v:.3e}  bound {b:.3e}")
            if not v <= b:
                fails.append((where, cls, q, v, b))
        rb = R.rhoD_bounds(bounds, cls, ref["kappa"], ref["X"])
        zero = np.asarray(ref["rhoD"] == 0)
        assert np.array_equal(g["rhoD"] == 0.0, zero), (where, cls, "rhoD is exactly 0 where X_i + 1e-10 > 1, only there")
        ratio = np.where(zero, 0.0, e["rhoD"] / rb)
        print(f"{where:14s} {cls:10s} rhoD   {float(np.where(zero, 0.0, e['rhoD']).max()):.3e}  worst error / bound {float(ratio.max()):.3f}")
        if not ratio.max() <= 1.0:
            k = np.unravel_index(int(ratio.argmax()), ratio.shape)
            fails.append((where, cls, "rhoD", float(e["rhoD"][k]), float(rb[k]), "species %d" % k[0]))
    return fails


@pytest.mark.parametrize("case_", _cases(), ids=_id)
def test_thermo_points(case_, bounds):
    kind, S, sym, mesh = case_
    t, pT, pH = _table_and_pools(S, sym)
    assert R.is_symmetric(t) == sym
    ctx, m, side = _context(kind, t, MESHES[mesh])
    C, B = m.n_cells, m.n_boundary_slots
    empty = np.isin(side, ("top", "down"))
    fixed = np.isin(side, ("left", "right"))
    zg = np.isin(side, ("front", "back"))
    assert empty.sum() > 0 and fixed.sum() > 0 and zg.sum() > 0 and empty.sum() + fixed.sum() + zg.sum() == B

    def sentinel():
        for q in OUT1:
            v = ctx.get_field("boundary_" + q, (B,)); v[empty] = SENTINEL; ctx.set_field("boundary_" + q, v)
        for q in OUTS:
            v = ctx.get_field("boundary_" + q, (S, B)); v[:, empty] = SENTINEL; ctx.set_field("boundary_" + q, v)

    def run(call, cells_in, slots_in):
        slots_in = {k: v.copy() for k, v in slots_in.items()}
        slots_in["T"][empty] = SENTINEL; slots_in["he"][empty] = SENTINEL
        _push(ctx, cells_in, slots_in)
        sentinel()
        ctx.call(call)
        a = _pull(ctx, S, C, B)
        _push(ctx, cells_in, slots_in)      # T / he are rewritten in place: the same inputs again
        ctx.call(call)
        b = _pull(ctx, S, C, B)
        for x, y in zip(a, b):
            for q in OUT1 + OUTS:
                assert np.array_equal(x[q], y[q]), (call, q, "not repeatable")
        for q in OUT1 + OUTS:
            assert (a[1][q][..., empty] == SENTINEL).all(), (call, q, "an empty slot was written")
        return a

    fails = []
    # ---- from T everywhere
    ic = np.arange(C) % pT.n
    ib = (C + np.arange(B)) % pT.n
    cells, slots = run("thermo_update_energy", _fill(pT, ic), _fill(pT, ib))
    fails += _check(t, bounds, pT, ic, cells, None, "energy/cells")
    live = np.where(~empty)[0]
    fails += _check(t, bounds, pT, ib[live], {q: slots[q][..., live] for q in slots}, None, "energy/slots")

    # ---- the three products, on the state the from-T call left (p moved so that rho != p psi beforehand)
    rng = np.random.default_rng(11)
    for pre, n in (("", C), ("boundary_", B)):
        ctx.set_field(pre + "p", ctx.get_field(pre + "p", (n,)) * (1 + 1e-3 * rng.standard_normal(n)))
    ctx.call("thermo_psip0")
    ctx.call("thermo_update_rho")
    prod = {}
    for pre, n in (("", C), ("boundary_", B)):
        psi = ctx.get_field(pre + "psi", (n,)); p1 = ctx.get_field(pre + "p", (n,))
        assert np.array_equal(ctx.get_field(pre + "psip0", (n,)), psi * p1), pre + "psip0"
        assert np.array_equal(ctx.get_field(pre + "rho", (n,)), p1 * psi), pre + "rho"
        p2 = p1 * (1 + 1e-3 * rng.standard_normal(n))
        ctx.set_field(pre + "p", p2)
        prod[pre] = (psi, p1, p2)
    ctx.call("thermo_correct_psip_rho")
    for pre, n in (("", C), ("boundary_", B)):
        psi, p1, p2 = prod[pre]
        want = p1 * psi + (psi * p2 - psi * p1)       # rho += psi p - psip0, each operation rounded (k_add_psip)
        assert np.array_equal(ctx.get_field(pre + "rho", (n,)), want), pre + "rho after correct_psip_rho"

    # ---- from he in the cells and on zeroGradient slots, from T on fixedValue slots
    ic = np.arange(C) % pH.n
    cells_in = _fill(pH, ic)
    slots_in = _fill(pT, ib)
    iz = (C + np.arange(int(zg.sum()))) % pH.n
    fz = _fill(pH, iz)
    for k in ("T", "he", "p"):
        slots_in[k][zg] = fz[k]
    slots_in["Y"][:, zg] = fz["Y"]
    cells, slots = run("thermo_correct", cells_in, slots_in)
    fails += _check(t, bounds, pH, ic, cells, cells_in["he"], "correct/cells")
    z = np.where(zg)[0]
    fails += _check(t, bounds, pH, iz, {q: slots[q][..., z] for q in slots}, fz["he"], "correct/zeroGrad")
    f = np.where(fixed)[0]
    fails += _check(t, bounds, pT, ib[f], {q: slots[q][..., f] for q in slots}, None, "correct/fixedT")
    ctx.close()
    assert not fails, fails
