"""The Peng-Robinson thermo kernels and the real-fluid time step on the device (include/dfmi.h dfmi_thermo_set_eos;
DESIGN 17) against tests/realfluid_reference.py.

Point parity follows tests/test_gpu_thermo_points.py: cells and boundary slots of a walled hex_box carry the
reference's states. thermo_update_energy evaluates every cell and slot from T (classes supercritical, dense,
near_critical, three_root, dilute, zeros, pure); thermo_correct evaluates cells and zeroGradient slots from he (class
newton) and fixedValue-T slots from T. Every output, per element, is held to 4x the float64 restatement's measured
error for its class and quantity (tests/golden/realfluid_point_bounds.json), floored at 1e-13; psi has its own entry
there, since the quotient amplifies the T solve's rounding by 1 / dx. Each call runs twice and must repeat bitwise.

Figures measured on the MI355X are printed before every assertion (pytest -s).
"""
import threading

import numpy as np
import pytest

import realfluid_reference as RF
import thermo_reference as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

MESHES = {"one": (1, 1, 1), "c255": (3, 5, 17), "c256": (4, 8, 8), "rod257": (257, 1, 1), "c4355": (5, 13, 67)}
OUT1 = ("T", "he", "psi", "rho", "mu", "alpha")
OUTS = ("rhoD", "hai")
SENTINEL = -7.25
FROM_T = ("supercritical", "dense", "near_critical", "three_root", "dilute", "zeros", "pure")
FROM_HE = ("newton",)
CASES = [("bfer6", m) for m in MESHES] + [("drawn2", "rod257"), ("drawn9", "rod257"), ("drawn9", "c4355"), ("drawn16", "rod257")]


class Pool:
    def __init__(self, name, classes):
        parts = [RF.states(name, c) for c in classes]
        self.cls = np.concatenate([np.full(s.n, c, dtype=object) for (s, _, _), c in zip(parts, classes)])
        cat = lambda f, ax=0: np.concatenate([f(s) for s, _, _ in parts], axis=ax)
        self.T, self.he, self.p = cat(lambda s: s.T), cat(lambda s: s.he), cat(lambda s: s.p)
        self.Y = cat(lambda s: s.Y, 1)
        self.n = self.T.size
        self.ref = {q: np.concatenate([r[q] for _, r, _ in parts], axis=-1)
                    for q in ("T", "he", "psi", "rho", "mu", "alpha", "rhoD", "hai", "kappa", "X", "Wm", "Z")}


_pools: dict = {}


def _pools_of(name):
    if name not in _pools:
        _pools[name] = (Pool(name, FROM_T), Pool(name, FROM_HE))
    return _pools[name]


@pytest.fixture(scope="module")
def bounds():
    return RF.load_bounds()


def _point_context(t, eos, dims):
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
    ctx = lib.Context(0)
    case.setup_context(ctx, m, t, t.S - 1, 1e-6, pt)
    ctx.thermo_set_eos(1, eos["a"], eos["b"], eos["w"])
    slot_side = np.repeat(np.array(name, dtype=object), [p.slots for p in m.patches])
    return ctx, m, slot_side


def _fill(pool, idx):
    return {"T": pool.T[idx], "he": pool.he[idx], "p": pool.p[idx], "Y": np.ascontiguousarray(pool.Y[:, idx])}


def _push(ctx, cells, slots):
    for k in ("T", "he", "p", "Y"):
        ctx.set_field(k, cells[k])
        ctx.set_field("boundary_" + k, slots[k])


def _pull(ctx, S, C, B):
    cells = {q: ctx.get_field(q, (C,)) for q in OUT1 + ("rho_thermo",)}
    slots = {q: ctx.get_field("boundary_" + q, (B,)) for q in OUT1 + ("rho_thermo",)}
    for q in OUTS:
        cells[q] = ctx.get_field(q, (S, C))
        slots[q] = ctx.get_field("boundary_" + q, (S, B))
    return cells, slots


def _check(t, bounds, pool, idx, got, where):
    fails = []
    assert np.array_equal(got["rho_thermo"], got["rho"]), (where, "rho_thermo is the density the call wrote to rho")
    for cls in sorted(set(pool.cls[idx])):
        sel = np.where(pool.cls[idx] == cls)[0]
        ix = idx[sel]
        g = {q: (got[q][:, sel] if q in OUTS else got[q][sel]) for q in OUT1 + OUTS}
        for q in OUT1 + OUTS:
            assert np.isfinite(g[q]).all(), (where, cls, q)
        ref = {q: pool.ref[q][..., ix] for q in pool.ref}
        # the same root of the cubic as the reference (another root is another phase: an O(1) error in Z)
        Z = pool.p[ix] * np.asarray(ref["Wm"], dtype=np.float64) / (g["rho"] * R.R_GAS * g["T"])
        zerr = float(np.abs(Z / np.asarray(ref["Z"], dtype=np.float64) - 1).max())
        print(f"{where:16s} {cls:13s} Z      {zerr:.3e}  (same root: < 1e-6)")
        assert zerr < 1e-6, (where, cls, "a different root of the cubic", zerr)
        e = RF.errors(t, g, ref)
        for q in OUT1 + ("hai",):
            b = RF.gpu_bound(bounds, cls, q)
            v = float(e[q].max())
            print(f"{where:16s} {cls:13s} {q:6s} {v:.3e}  bound {b:.3e}")
            if not v <= b:
                fails.append((where, cls, q, v, b))
        rb = RF.rhoD_bounds(bounds, cls, ref["kappa"])
        zero = np.asarray(ref["rhoD"] == 0)
        assert np.array_equal(g["rhoD"] == 0.0, zero), (where, cls, "rhoD is exactly 0 where X_i + 1e-10 > 1, only there")
        ratio = np.where(zero, 0.0, e["rhoD"] / rb)
        print(f"{where:16s} {cls:13s} rhoD   {float(np.where(zero, 0.0, e['rhoD']).max()):.3e}  worst error / bound {float(ratio.max()):.3f}")
        if not ratio.max() <= 1.0:
            fails.append((where, cls, "rhoD", float(ratio.max())))
    return fails


@pytest.mark.parametrize("case_", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_point_parity(case_, bounds):
    name, mesh = case_
    t, eos = RF.table(name)
    S = t.S
    pT, pH = _pools_of(name)
    ctx, m, side = _point_context(t, eos, MESHES[mesh])
    C, B = m.n_cells, m.n_boundary_slots
    empty = np.isin(side, ("top", "down"))
    fixed = np.isin(side, ("left", "right"))
    zg = np.isin(side, ("front", "back"))
    assert empty.sum() > 0 and fixed.sum() > 0 and zg.sum() > 0 and empty.sum() + fixed.sum() + zg.sum() == B
    names1 = OUT1 + ("rho_thermo",)

    def sentinel():
        for q in names1:
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
            for q in names1 + OUTS:
                assert np.array_equal(x[q], y[q]), (call, q, "not repeatable")
        for q in names1 + OUTS:
            assert (a[1][q][..., empty] == SENTINEL).all(), (call, q, "an empty slot was written")
        return a

    fails = []
    # a different stride through the pool per mesh, so the small meshes do not all see its first states
    off = {"one": 0, "c255": 17, "c256": 301, "rod257": 613, "c4355": 0}[mesh]
    ic = (off + np.arange(C)) % pT.n
    ib = (off + C + np.arange(B)) % pT.n
    cells, slots = run("thermo_update_energy", _fill(pT, ic), _fill(pT, ib))
    fails += _check(t, bounds, pT, ic, cells, "energy/cells")
    live = np.where(~empty)[0]
    fails += _check(t, bounds, pT, ib[live], {q: slots[q][..., live] for q in slots}, "energy/slots")

    # the three products on the state that call left, p moved so that rho_thermo != psi p
    rng = np.random.default_rng(11)
    prod = {}
    for pre, n in (("", C), ("boundary_", B)):
        p1 = ctx.get_field(pre + "p", (n,)) * (1 + 1e-3 * rng.standard_normal(n))
        ctx.set_field(pre + "p", p1)
        prod[pre] = [ctx.get_field(pre + "psi", (n,)), p1, ctx.get_field(pre + "rho_thermo", (n,))]
        ctx.set_field(pre + "rho", np.zeros(n))
    ctx.call("thermo_psip0")
    ctx.call("thermo_update_rho")
    for pre, n in (("", C), ("boundary_", B)):
        psi, p1, rt = prod[pre]
        assert np.array_equal(ctx.get_field(pre + "psip0", (n,)), psi * p1), pre + "psip0"
        assert np.array_equal(ctx.get_field(pre + "rho", (n,)), rt), pre + "rho = rho_thermo, not psi p"
        p2 = p1 * (1 + 1e-3 * rng.standard_normal(n))
        ctx.set_field(pre + "p", p2)
        prod[pre].append(p2)
    ctx.call("thermo_correct_psip_rho")
    for pre, n in (("", C), ("boundary_", B)):
        psi, p1, rt, p2 = prod[pre]
        want = rt + (psi * p2 - psi * p1)
        assert np.array_equal(ctx.get_field(pre + "rho_thermo", (n,)), want), pre + "rho_thermo after correct_psip_rho"
        assert np.array_equal(ctx.get_field(pre + "rho", (n,)), rt), pre + "rho is left alone"

    # from he in the cells and on zeroGradient slots, from T on fixedValue slots
    ic = (off + np.arange(C)) % pH.n
    cells_in = _fill(pH, ic)
    slots_in = _fill(pT, ib)
    iz = (off + C + np.arange(int(zg.sum()))) % pH.n
    fz = _fill(pH, iz)
    for k in ("T", "he", "p"):
        slots_in[k][zg] = fz[k]
    slots_in["Y"][:, zg] = fz["Y"]
    cells, slots = run("thermo_correct", cells_in, slots_in)
    assert np.array_equal(cells["he"], cells_in["he"]), "he is passed through"
    fails += _check(t, bounds, pH, ic, cells, "correct/cells")
    z = np.where(zg)[0]
    fails += _check(t, bounds, pH, iz, {q: slots[q][..., z] for q in slots}, "correct/zeroGrad")
    f = np.where(fixed)[0]
    fails += _check(t, bounds, pT, ib[f], {q: slots[q][..., f] for q in slots}, "correct/fixedT")
    ctx.close()
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ the full step
def _walls(m, sides):
    from dfmi import case
    from dfmi.mesh import FIXED_VALUE
    pt = case.default_patch_types(m)
    name = [p.name for p in m.patches]
    pt["T"] = pt["T"].copy()
    for s in sides:
        pt["T"][name.index(s)] = FIXED_VALUE
    return pt


def _step_context(m, t, eos, pt, f, comm=None, set_eos=True):
    from dfmi import case, lib
    ctx = lib.Context(0)
    case.setup_context(ctx, m, t, t.species.index("N2"), 1e-6, pt, comm=comm)
    if set_eos:
        ctx.thermo_set_eos(1, eos["a"], eos["b"], eos["w"])
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 300, 1e-15, 1e-300)
    ctx.set_solver("p", 3000, 1e-15, 1e-300)
    bv = {"T": {p.name: 300.0 + 40.0 * k for k, p in enumerate(m.patches) if p.kind not in ("cyclic", "processor")}}
    case.init_state(ctx, m, t.S, f["T"], f["p"], f["U"], f["Y"], bvals=bv)
    ctx.call("pre_time_step")
    return ctx


BOXES = {"8x8x8-periodic-xy": ((8, 8, 8), (True, True, False), ("front", "back")),
         "6x5x4-walled": ((6, 5, 4), (False, False, False), ("left", "right", "top"))}


@pytest.mark.parametrize("box", list(BOXES))
def test_full_step_matches_the_real_fluid_oracle(box):
    """one outer iteration (nCorr = 2) against RealFluidOracle with exact solves, at the project's full-step tolerance"""
    from dfmi import case
    from dfmi.mesh import hex_box
    dims, periodic, hot = BOXES[box]
    t, eos = RF.bfer6()
    L = 1e-3
    m = hex_box(*dims, lengths=(2 * np.pi * L,) * 3, periodic=periodic, gradings=(1.0, 1.3, 1.0))
    pt = _walls(m, hot)
    f = RF.flow_fields(m, t.species, L)
    ctx = _step_context(m, t, eos, pt, f)
    C, B = m.n_cells, m.n_boundary_slots
    st = case.pull_state(ctx, m, t.S)
    for pre, n in (("", C), ("boundary_", B)):
        st[pre + "rho_thermo"] = ctx.get_field(pre + "rho_thermo", (n,))
    assert np.array_equal(st["rho_thermo"], st["rho"])
    Z = st["p"] * 28.0 / (st["rho"] * R.R_GAS * st["T"])
    assert Z.min() < 0.7, "the state is a real fluid"
    o = RF.RealFluidOracle(m, t, eos, {k: v.copy() for k, v in st.items()}, pt, t.species.index("N2"), 1e6)
    o.time_step(2)
    ctx.time_step(2)
    worst = {}
    for n in ("T", "p", "rho", "rho_thermo", "he", "psi"):
        worst[n] = rel_err(ctx.get_field(n, (C,)), o[n])
        worst["boundary_" + n] = rel_err(ctx.get_field("boundary_" + n, (B,)), o["boundary_" + n])
    worst["U"] = rel_err(ctx.get_field("U", (3, C)), o["U"])
    worst["Y"] = rel_err(ctx.get_field("Y", (t.S, C)), o["Y"])
    worst["phi"] = rel_err(ctx.get_field("phi", (m.n_faces,)), o["phi"])
    for n, e in worst.items():
        print(f"{box:20s} {n:20s} {e:.3e}")
    assert np.array_equal(ctx.get_field("rho", (C,)), ctx.get_field("rho_thermo", (C,))), "rho = thermo.rho() after the loop"
    assert not np.array_equal(ctx.get_field("rho", (C,)), ctx.get_field("psi", (C,)) * ctx.get_field("p", (C,)))
    ctx.close()
    bad = {n: e for n, e in worst.items() if not e < 1e-9}
    assert not bad, bad


_HUB = [700]


def test_two_ranks_match_the_single_domain():
    """an 8x8x8 box cut in x, the in-process transport: rho_thermo travels with psi across the processor patches"""
    from dfmi.mesh import hex_box, global_cell_ids
    t, eos = RF.bfer6()
    L = 1e-3
    kw = dict(lengths=(2 * np.pi * L,) * 3, periodic=(True, True, False), gradings=(1.0, 1.3, 1.0))
    mg = hex_box(8, 8, 8, **kw)
    f = RF.flow_fields(mg, t.species, L)
    names = ("T", "p", "rho", "rho_thermo", "he", "psi")
    ctx = _step_context(mg, t, eos, _walls(mg, ("front", "back")), f)
    ctx.time_step(2)
    ref = {n: ctx.get_field(n, (mg.n_cells,)) for n in names}
    ref["U"] = ctx.get_field("U", (3, mg.n_cells)); ref["Y"] = ctx.get_field("Y", (t.S, mg.n_cells))
    ctx.close()
    meshes = [hex_box(8, 8, 8, decomp=(2, 1, 1), rank=r, **kw) for r in range(2)]
    gids = [global_cell_ids(mm, 8, 8) for mm in meshes]
    out, err = [None, None], [None, None]
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            m, g = meshes[r], gids[r]
            fr = {"T": f["T"][g], "p": f["p"][g], "U": f["U"][:, g], "Y": f["Y"][:, g]}
            c = _step_context(m, t, eos, _walls(m, ("front", "back")), fr, comm={"hub": hub, "nranks": 2, "rank": r})
            c.time_step(2)
            o = {n: c.get_field(n, (m.n_cells,)) for n in names}
            o["U"] = c.get_field("U", (3, m.n_cells)); o["Y"] = c.get_field("Y", (t.S, m.n_cells))
            out[r] = o
            c.close()
        except Exception as e:   # surfaced below
            err[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not any(x.is_alive() for x in th), "decomposed run hung"
    for e in err:
        if e is not None:
            raise e
    for n in names + ("U", "Y"):
        glob = np.zeros_like(ref[n])
        for r in range(2):
            glob[..., gids[r]] = out[r][n]
        e = rel_err(glob, ref[n])
        print(f"two ranks {n:12s} {e:.3e}")
        assert e <= 1e-9, (n, e)


# ------------------------------------------------------------------------------------------------ refusals, clearing
def test_refusals_name_their_key():
    from dfmi import case, lib
    from dfmi.mesh import hex_box
    t, eos = RF.bfer6()
    L = 1e-3
    m = hex_box(4, 3, 2, lengths=(2 * np.pi * L,) * 3, periodic=(True, True, False))
    f = RF.flow_fields(m, t.species, L)
    ctx = _step_context(m, t, eos, _walls(m, ("front", "back")), f)
    a, b, w = eos["a"], eos["b"], eos["w"]

    def refused(fn, *words):
        with pytest.raises(lib.DfmiError) as ei:
            fn()
        for wd in words:
            assert wd in str(ei.value), (wd, str(ei.value))

    refused(lambda: ctx.thermo_set_eos(2, a, b, w), "model must be 0")
    refused(lambda: ctx.thermo_set_eos(1, a[:5], b[:5], w[:5]), "num_species 5")
    bad = a.copy(); bad[2] = np.nan
    refused(lambda: ctx.thermo_set_eos(1, bad, b, w), "finite", "species 2")
    bad = a.copy(); bad[1] = -1.0
    refused(lambda: ctx.thermo_set_eos(1, bad, b, w), "a of species 1", "negative")
    bad = b.copy(); bad[3] = 0.0
    refused(lambda: ctx.thermo_set_eos(1, a, bad, w), "b of species 3", "positive")
    bad = w.copy(); bad[0] = np.inf
    refused(lambda: ctx.thermo_set_eos(1, a, b, bad), "finite", "species 0")
    # a refused call changed nothing: the model in force still steps
    ctx.time_step(2)
    for key in ("les.model", "ras.model", "tci.model"):
        c2 = _step_context(m, t, eos, _walls(m, ("front", "back")), f)
        c2.set_option(key, 1.0)
        refused(lambda: c2.time_step(2), "dfmi_time_step", key)
        c2.close()
    refused(lambda: ctx.zero_d_step(1e-6), "dfmi_zero_d_step", "equation of state")
    ctx.close()
    # the species-chunked kernels
    lib.DEFAULT_OPTIONS["fv.species_generic"] = 1
    try:
        c3 = lib.Context(0)
    finally:
        lib.DEFAULT_OPTIONS.pop("fv.species_generic", None)
    case.setup_context(c3, m, t, t.species.index("N2"), 1e-6, _walls(m, ("front", "back")))
    c3.thermo_set_eos(1, a, b, w)
    refused(lambda: c3.call("thermo_correct"), "fv.species_generic")
    c3.close()
    # more than 16 species
    t17 = R.gri_table(17)
    c4 = lib.Context(0)
    case.setup_context(c4, m, t17, 16, 1e-6, case.default_patch_types(m))
    one = np.ones(17)
    refused(lambda: c4.thermo_set_eos(1, one, one, one), "16 species")
    c4.close()


def test_chemistry_is_refused_at_the_step():
    from dfmi import lib
    from dfmi.mesh import hex_box
    t, eos = RF.bfer6()
    L = 1e-3
    m = hex_box(4, 3, 2, lengths=(2 * np.pi * L,) * 3, periodic=(True, True, False))
    f = RF.flow_fields(m, t.species, L)
    ctx = _step_context(m, t, eos, _walls(m, ("front", "back")), f)
    ctx.chem_set_options(1)
    with pytest.raises(lib.DfmiError) as ei:
        ctx.time_step(2)
    assert "chem.mode" in str(ei.value) and "dfmi_time_step" in str(ei.value)
    ctx.close()


def test_clearing_restores_the_ideal_step_bitwise():
    """model 0 after model 1: a step bitwise equal to a context that never set an equation of state"""
    from dfmi.mesh import hex_box
    t, eos = RF.bfer6()
    L = 1e-3
    m = hex_box(6, 5, 4, lengths=(2 * np.pi * L,) * 3, periodic=(False,) * 3, gradings=(1.0, 1.3, 1.0))
    f = RF.flow_fields(m, t.species, L)
    f["p"] = np.full(m.n_cells, 101325.0)
    pt = _walls(m, ("left", "right"))
    out = []
    for was_set in (False, True):
        ctx = _step_context(m, t, eos, pt, f, set_eos=False)
        if was_set:
            from dfmi import case
            st = case.pull_state(ctx, m, t.S)
            ctx.thermo_set_eos(1, eos["a"], eos["b"], eos["w"])
            ctx.call("thermo_correct")
            assert not np.array_equal(ctx.get_field("rho", (m.n_cells,)), st["rho"])
            ctx.thermo_set_eos(0)
            case.push_state(ctx, st)
        ctx.time_step(2)
        o = {n: ctx.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he", "psi", "mu", "alpha")}
        o["U"] = ctx.get_field("U", (3, m.n_cells)); o["Y"] = ctx.get_field("Y", (t.S, m.n_cells))
        o["phi"] = ctx.get_field("phi", (m.n_faces,))
        out.append(o)
        ctx.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n
