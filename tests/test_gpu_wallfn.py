"""k-epsilon wall functions and turbulent inlets on the device (MI355X): epsilonWallFunction / nutkWallFunction and the two
turbulent inlet conditions (include/dfmi.h dfmi_turbulence_correct, RAS block), held to the NumPy restatement
tests/wallfn_reference.py.

Wall values and the wall update against long double at 4x the fp64 restatement's measured error per mesh
(tests/golden/wallfn_bounds.json), floored at 1e-13; the constrained epsilon matrix and the k matrix at 0 ulp with the
device's own G, divU, nut and wall values injected; the inlets against a twin context with plain inletOutlet; the
constrained cells after the solve; full steps against WallOracle; two ranks; nothing changes when unused; refusals.
"""
import threading

import numpy as np
import pytest

import nonorth_reference as NR
import ras_reference as R
import wallfn_reference as W
from conftest import rel_err, ulp_diff
from test_gpu_parity import _case
from test_gpu_ras import Case, PARTS, _fields, _oracle_grad, _tight

pytestmark = pytest.mark.gpu

NEW_KERNELS = "k_ras_wall,k_ras_nut_wall,k_ras_inlet_ref,k_ras_constrain_source"
EPS4 = 4 * 2.0 ** -52


class WCase(Case):
    """test_gpu_ras.Case with wall functions on the patches `which` ("yz": the y- and z-walls, "all") and wall_state
    pushed"""

    def __init__(self, name, which="yz", schemes=None, small=1, setup=None, walls="zg", push=True):
        if schemes is None and name == "sheared-walls":
            schemes = {"laplacian": "corrected"}
        super().__init__(name, walls=walls, schemes=schemes, small=small)
        self.ws = W.default_setup(self.m, which) if setup is None else setup
        self.ws.apply(self.ctx)
        self.wst = W.wall_state(self.m, self.ws)
        if push:
            self.push(self.wst)

    def restated(self, keq, con=None, wc=None, bwc=None, dc=None, bdc=None, ref=None):
        """the restatement's matrix of one equation from the context's fields as the last dfmi_assemble left them"""
        q, ws = self.q, self.ws
        g = {n: self.get(n) for n in ("G", "divU", "nut", "rho", "rho_old", "mu", "k", "epsilon", "boundary_rho", "boundary_nut",
                                      "boundary_mu", "boundary_k", "boundary_epsilon", "boundary_phi")}
        phi = self.ctx.get_field("phi", (self.m.n_faces,))
        Su, Sp = R.sources(keq, q, g["G"], g["divU"], g["rho"], g["k"], g["epsilon"])
        sig = q["sigmak"] if keq else q["sigmaEps"]
        D = R.diffusivity(g["rho"], g["nut"], g["mu"], sig)
        bD = R.diffusivity(g["boundary_rho"], g["boundary_nut"], g["boundary_mu"], sig)
        nm = "k" if keq else "epsilon"
        pt = W.device_types(ws.k_pt if keq else ws.eps_pt)
        o = R.scalar_assemble(self.tp, pt, g[nm], g["boundary_" + nm], g["rho"], g["rho_old"], phi, g["boundary_phi"], D, bD, Su,
                              Sp, 1.0 / self.dt, wc=wc, bwc=bwc, ref=ref, dc=dc, bdc=bdc)
        if con is not None:
            W.constrain(self.tp, o, con, g["epsilon"])
        return o, g, D


@pytest.fixture(scope="module", params=list(W.MESHES))
def wc(request):
    c = WCase(request.param)
    yield c
    c.ctx.close()


def _conditions(c):
    lo, hi, gap, kmin, emin, _, _ = W.state_conditions(c.ws, c.wst)
    assert lo >= 0.2 and hi >= 0.2 and gap > 1e-6 and kmin > 0 and emin > 0, (c.name, lo, hi, gap)


def _con(c):
    return np.array([any(c.ws.eps_wall[b] for b in c.tp.slots[i]) for i in range(c.m.n_cells)])


# ------------------------------------------------------------------------------------------------ 1. wall values
def test_wall_values_through_validate(wc):
    c, ctx, ws, st = wc, wc.ctx, wc.ws, wc.wst
    _conditions(c)
    ctx.set_field("k", np.ascontiguousarray(st["k"]))                              # invalidates nut
    ctx.kernel_timer("k_ras_nut," + NEW_KERNELS)
    ctx.call("U_process")                                                           # validate(): correctNut() only
    n = {k: ctx.kernel_time(k)[1] for k in ("k_ras_nut",) + tuple(NEW_KERNELS.split(","))}
    ctx.kernel_timer("")
    assert n == {"k_ras_nut": 2, "k_ras_nut_wall": 1, "k_ras_wall": 0, "k_ras_inlet_ref": 0, "k_ras_constrain_source": 0}, n
    bnut, byp = c.get("boundary_nut"), c.get("boundary_yPlus")
    err = W.wall_errors(ws, c.tp, st, bnut, byp, None, None)
    bounds = W.load_bounds()
    for what in ("boundary_nut", "boundary_yPlus"):
        b = W.gpu_bound(bounds, c.name, what)
        print(f"{c.name}: {what} err {err[what]:.3e} (bound {b:.1e})")
        assert err[what] <= b, (what, err[what])
    yp, _, _ = W.y_plus(ws, st["k"], st["boundary_mu"], st["boundary_rho"], W.LD)
    ypl = ws.consts(W.LD)[4]
    lam = ws.nut_wall & (yp <= ypl)
    assert lam.sum() >= 0.2 * ws.nut_wall.sum() and not bnut[lam].any()             # below yPlusLam: exactly 0
    assert bnut[ws.nut_wall & ~lam].min() > 0
    assert not byp[~ws.nut_wall].any()
    # the other slots keep correctNut()'s calculated values
    other = ~ws.nut_wall
    assert np.array_equal(bnut[other], R.nut_of(c.q["Cmu"], st["boundary_k"], st["boundary_epsilon"])[other])


# ------------------------------------------------------------------------------------------------ 2. wall update
def test_wall_update_after_assemble(wc):
    c, ctx, ws, st = wc, wc.ctx, wc.ws, wc.wst
    c.push(st)
    ctx.assemble("epsilon")
    G, eps, beps, bnut = c.get("G"), c.get("epsilon"), c.get("boundary_epsilon"), c.get("boundary_nut")
    con = _con(c)
    err = W.wall_errors(ws, c.tp, st, bnut, c.get("boundary_yPlus"), eps, G, bnut_in=np.asarray(bnut, W.LD))
    bounds = W.load_bounds()
    for what in ("epsilon", "G"):
        b = W.gpu_bound(bounds, c.name, what)
        print(f"{c.name}: wall cells' {what} err {err[what]:.3e} (bound {b:.1e})")
        assert err[what] <= b, (what, err[what])
    for cell in np.nonzero(con)[0]:
        for b in c.tp.slots[cell]:
            if ws.eps_wall[b]:
                assert beps[b] == eps[cell]
    assert np.array_equal(beps[~ws.eps_wall], st["boundary_epsilon"][~ws.eps_wall])
    assert np.array_equal(eps[~con], st["epsilon"][~con]) and eps[con].min() > 0
    # a wall cell whose slots are all below yPlusLam gets no G
    yp, _, _ = W.y_plus(ws, st["k"], st["boundary_mu"], st["boundary_rho"], W.LD)
    ypl = ws.consts(W.LD)[4]
    quiet = [i for i in np.nonzero(con)[0] if all(yp[b] <= ypl[b] for b in c.tp.slots[i] if ws.eps_wall[b])]
    assert quiet and not G[quiet].any()
    assert np.abs(G[con]).max() > 0
    c.G_wall = G


def test_non_wall_cells_and_weights_on_walls():
    """non-wall cells bitwise as in a context without wall functions; with every wall a wall-function patch the corner
    cells carry the weight 1/3 and the edge cells 1/2"""
    c = WCase("walls", "all")
    plain = Case("walls")
    try:
        st, ws = c.wst, c.ws
        plain.push(st)
        plain.ctx.assemble("epsilon")
        c.ctx.assemble("epsilon")
        G, eps = c.get("G"), c.get("epsilon")
        con = _con(c)
        n = np.array([sum(ws.eps_wall[b] for b in c.tp.slots[i]) for i in range(c.m.n_cells)])
        assert set(n) == {0, 1, 2, 3} and (n == 3).sum() == 8
        assert np.array_equal(G[~con], plain.get("G")[~con]) and np.array_equal(eps[~con], plain.get("epsilon")[~con])
        assert np.array_equal(c.get("divU"), plain.get("divU"))
        yp, y, nuw = W.y_plus(ws, st["k"], st["boundary_mu"], st["boundary_rho"])
        c25, c75, kap, _, ypl = ws.consts()
        for i in np.nonzero(n >= 2)[0]:
            kc = st["k"][i]
            one = [c75[b] * kc ** 1.5 / (kap[b] * y[b]) if yp[b] > ypl[b] else 2 * kc * nuw[b] / y[b] ** 2 for b in c.tp.slots[i]]
            assert abs(eps[i] / np.mean(one) - 1) <= 1e-13, (i, n[i])
    finally:
        c.ctx.close(); plain.ctx.close()


# ------------------------------------------------------------------------------------------------ 3. matrices
def _check_matrices(c, scheme):
    m, ctx, ws = c.m, c.ctx, c.ws
    corrected = c.name == "sheared-walls"
    dc = bdc = None
    if corrected:
        dc, _, bdc, _ = m.nonorth_geometry()
    for t in ("div(phi,k)", "div(phi,epsilon)"):
        ctx.set_scheme(t, scheme)
    con = _con(c)
    try:
        for eqn, keq in (("epsilon", 0), ("k", 1)):
            dev = c.device(eqn)
            pt = W.device_types(ws.k_pt if keq else ws.eps_pt)
            wcw = bwc = None
            if scheme != "upwind":
                v, bv = c.get(eqn), c.get("boundary_" + eqn)
                c.k_pt = pt                                                       # _oracle_grad reads the field's types there
                wcw, bwc = R.limited_weights(c.tp, pt, 1.0, ctx.get_field("phi", (m.n_faces,)), c.get("boundary_phi"), v, bv,
                                             _oracle_grad(c, v, bv))
            ref, g, D = c.restated(keq, None if keq else con, wcw, bwc, dc, bdc)
            free = np.ones(m.n_cells, bool) if keq else ~con
            for p in PARTS:
                if corrected and p == "source":
                    continue
                assert ulp_diff(dev[p], ref[p]) == 0, (c.name, scheme, eqn, p, rel_err(dev[p], ref[p]))
            if not keq:   # the constraint is in the matrix
                assert np.array_equal(dev["source"][con], g["epsilon"][con] * dev["diag"][con])
                own, nei = np.asarray(m.owner), np.asarray(m.neighbour)
                cut = con[own] | con[nei]
                assert cut.any() and not dev["lower"][cut].any() and not dev["upper"][cut].any()
                if (~cut).any():
                    assert np.abs(dev["lower"][~cut]).min() > 0
            if corrected:   # the explicit term on the unconstrained rows, at the non-orthogonal suite's own bound form
                acc, _, _, sc = NR.corrected_term(m, pt, g[eqn][None], g["boundary_" + eqn][None], D[None])
                accL, _, _, _ = NR.corrected_term(m, pt, g[eqn][None], g["boundary_" + eqn][None], D[None], T=NR.LD)
                bound = NR.gpu_bound(NR.load_bounds(), "sheared-walls", "he")
                err = np.abs((dev["source"] - ref["source"]) - np.asarray(accL[0], np.float64))
                tol = bound * np.asarray(sc[0], np.float64) + 4 * np.finfo(float).eps * np.abs(ref["source"])
                print(f"corrected {eqn}: max err / tol {np.max(err[free] / tol[free]):.3e}, term max {np.abs(acc).max():.3e}")
                assert np.all(err[free] <= tol[free]) and np.abs(acc).max() > 0
    finally:
        for t in ("div(phi,k)", "div(phi,epsilon)"):
            ctx.set_scheme(t, "upwind")


@pytest.mark.parametrize("scheme", ["upwind", "limitedLinear 1"])
def test_matrices_bitwise_with_the_constraint(wc, scheme):
    c = wc
    c.push(c.wst)
    con = _con(c)
    if c.name != "rod":                                                           # rod: every cell is a wall cell
        assert 0 < con.sum() < c.m.n_cells
    _check_matrices(c, scheme)


# ------------------------------------------------------------------------------------------------ 4. inlets
def test_turbulent_inlets_against_plain_inlet_outlet():
    m = R.get_mesh("walls")
    inl = {"left": (0.0628, 0.000735), "right": (0.0471, 0.0019)}
    ws = W.WallSetup(m, inlets=inl)
    twin_ws = W.WallSetup(m, outlets=("left", "right"))
    c = WCase("walls", setup=ws, walls="mixed", push=False)
    t = WCase("walls", setup=twin_ws, walls="mixed", push=False)
    try:
        rng = np.random.default_rng(41)
        k = 0.3 * (1 + 0.5 * rng.uniform(-1, 1, m.n_cells))
        eps = 2e3 * (1 + 0.5 * rng.uniform(-1, 1, m.n_cells))
        bphi = c.get("boundary_phi")
        on_l, on_r = (NR.slot_types(m, ws.k_pt) == W.K_INLET) & (ws.patch == 2), ws.patch == 3
        assert m.patches[2].name == "left" and m.patches[3].name == "right"
        # x-min carries inflow, x-max (the TGV flow crosses it both ways) outflow too
        bphi[on_l] = -np.abs(bphi[on_l]) - 1e-12
        for x in (c, t):
            x.ctx.set_field("boundary_phi", bphi)
            x.set_ke(k, eps)
        assert bphi[on_l].max() < 0 and bphi[on_r].max() > 0
        bU, bk = c.ctx.get_field("boundary_U", (3, m.n_boundary_slots)), c.get("boundary_k")
        assert np.abs(bU[:, on_l]).max() > 0
        dev = {e: c.device(e) for e in ("epsilon", "k")}
        kref, eref = c.get("boundary_k_ref"), c.get("boundary_epsilon_ref")
        assert np.array_equal(kref, W.inlet_k_ref(ws, bU)) and np.array_equal(eref, W.inlet_eps_ref(ws, c.q["Cmu"], bk))
        assert kref[ws.k_inlet].min() > 0 and eref[ws.eps_inlet].min() > 0 and not kref[~ws.k_inlet].any()
        t.ctx.set_field("boundary_k_ref", kref); t.ctx.set_field("boundary_epsilon_ref", eref)
        for e in ("epsilon", "k"):
            got = t.device(e)
            for p in PARTS:
                assert np.array_equal(got[p], dev[e][p]), (e, p)
        assert np.abs(dev["k"]["boundary_coeffs"][on_l]).min() > 0                 # the inflow slots carry the inletValue
        for x in (c, t):
            _tight(x.ctx)
            x.ctx.turbulence_correct()
        for n in ("k", "epsilon", "nut", "boundary_k", "boundary_epsilon", "boundary_nut"):
            assert np.array_equal(c.get(n), t.get(n)), n
        assert np.array_equal(c.get("boundary_k")[on_l], kref[on_l])               # inflow: the slot takes the inletValue
        # a changed intensity re-forms the reference at the next correct
        c.ctx.set_patch_param("k", 2, "intensity", 0.1)
        c.ctx.turbulence_correct()
        want = W.inlet_k_ref(W.WallSetup(m, inlets=dict(inl, left=(0.1, 0.000735))), bU)
        assert np.array_equal(c.get("boundary_k_ref"), want)
    finally:
        c.ctx.close(); t.ctx.close()


# ------------------------------------------------------------------------------------------------ 5. solve
@pytest.mark.parametrize("path", ["small", "even-odd", "jacobi"])
def test_constrained_cells_hold_the_wall_value_after_the_solve(path):
    from dfmi import lib
    opts = {"small": {}, "even-odd": {"solver.small": 0}, "jacobi": {"solver.small": 0, "solver.even_odd": 0}}[path]
    lib.DEFAULT_OPTIONS.update(opts)
    try:
        c = WCase("rod", "all")
    finally:
        for k in opts:
            lib.DEFAULT_OPTIONS.pop(k, None)
    try:
        ctx, ws = c.ctx, c.ws
        _tight(ctx)
        ctx.turbulence_correct()
        pre, eps, beps = c.get("epsilon_prebound"), c.get("epsilon"), c.get("boundary_epsilon")
        con = _con(c)
        assert con.all()
        cell = ws.cell[ws.eps_wall]
        e = np.abs(pre[cell] / beps[ws.eps_wall] - 1).max()
        print(path, f"constrained cells after the solve: {e:.2e} (bound {EPS4:.2e})", ctx.solver_stats("epsilon"))
        assert e <= EPS4
        assert np.array_equal(eps, pre)                                           # positive: bound() leaves them
        assert ulp_diff(c.get("k"), c.wst["k"]) > 0                               # the k equation moved
    finally:
        c.ctx.close()


def test_constrained_cells_next_to_free_cells_after_the_solve(wc):
    c, ctx, ws = wc, wc.ctx, wc.ws
    c.push(c.wst)
    _tight(ctx)
    ctx.turbulence_correct()
    pre, beps = c.get("epsilon_prebound"), c.get("boundary_epsilon")
    e = np.abs(pre[ws.cell[ws.eps_wall]] / beps[ws.eps_wall] - 1).max()
    print(c.name, f"constrained cells after the solve: {e:.2e}")
    assert e <= EPS4
    con = _con(c)
    if (~con).any():
        assert ulp_diff(pre[~con], c.wst["epsilon"][~con]) > 0


# ------------------------------------------------------------------------------------------------ 6. full steps
def _step_ke(m, seed):
    rng = np.random.default_rng(seed)
    k = np.exp(rng.uniform(np.log(0.05), np.log(30.0), m.n_cells))
    return k, 4e5 * (k / 30.0)


def test_three_steps_match_wall_oracle():
    from dfmi import case
    from dfmi.mesh import FIXED_VALUE
    from test_gpu_turbulence import _walls
    m = R.get_mesh("walls")
    ctx, _, t, st, pt, inert, dt = _case(periodic=False, walls=_walls(all_fixed_U=True), mech="burke9", mesh=m)
    try:
        assert np.all(pt["U"] == FIXED_VALUE)
        q = dict(R.DEFAULTS, Prt=0.85, Sct=0.7)
        for key, v in q.items():
            ctx.set_option("ras." + key, v)
        ctx.set_option("ras.model", 1)
        ws = W.default_setup(m, "all")
        ws.apply(ctx)
        _tight(ctx)
        state = {k_: v.copy() for k_, v in st.items()}
        case.push_state(ctx, state)
        k, eps = _step_ke(m, 43)
        bk, beps = case.boundary_values(m, k).reshape(-1), case.boundary_values(m, eps).reshape(-1)
        for n, v in (("k", k), ("epsilon", eps), ("boundary_k", bk), ("boundary_epsilon", beps)):
            ctx.set_field(n, np.ascontiguousarray(v))
        o = W.WallOracle(m, t, {k_: v.copy() for k_, v in state.items()}, dict(pt), inert, 1.0 / dt, q, k, eps, bk, beps, ws)
        ypl = ws.consts()[4]
        B = m.n_boundary_slots
        seen = set()
        for step in (1, 2, 3):
            o.time_step(2)
            ctx.time_step(2)
            seen |= set((o.yPlus[ws.nut_wall] > ypl[ws.nut_wall]).tolist())
            for n, shp in (("T", (m.n_cells,)), ("p", (m.n_cells,)), ("rho", (m.n_cells,)), ("he", (m.n_cells,)),
                           ("U", (3, m.n_cells)), ("Y", (t.S, m.n_cells)), ("phi", (m.n_faces,)), ("k", (m.n_cells,)),
                           ("epsilon", (m.n_cells,)), ("nut", (m.n_cells,)), ("boundary_nut", (B,))):
                e = rel_err(ctx.get_field(n, shp), o[n])
                print("walls", step, n, f"{e:.2e}")
                assert e < 1e-9, (step, n, e)
            assert rel_err(ctx.get_field("boundary_yPlus", (B,)), o.yPlus) < 1e-9
        assert seen == {True, False}                                              # both branches of the wall functions ran
        assert o.con.sum() > 0 and np.abs(o.G[o.con]).max() > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 7. two ranks
_HUB = [940]


def test_two_ranks_match_single_domain():
    from dfmi import case
    from dfmi.lib import Context
    from dfmi.mesh import FIXED_VALUE
    from dfmi.partition import partition_cells, decompose
    from test_gpu_parity import _mech
    mg = R.get_mesh("sheared-walls")
    ym, t = _mech("burke9")
    dt = 1e-6
    inert = ym["species"].index("N2")
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    k, eps = _step_ke(mg, 47)
    schemes = {"div(phi,k)": "limitedLinear 1", "laplacian": "corrected"}
    part = np.asarray(partition_cells(mg, 2, "graph"))
    wall_cell = np.zeros(mg.n_cells, bool)
    wall_cell[NR.Slots(mg).cell] = True
    cut = part[mg.owner] != part[mg.neighbour]
    assert (cut & wall_cell[mg.owner] & wall_cell[mg.neighbour]).sum() > 2          # the cut crosses the wall layer

    def run(m, g, comm=None):
        c = Context(0)
        try:
            pt = case.default_patch_types(m)
            for i, p in enumerate(m.patches):
                if p.kind == "wall":
                    pt["U"][i] = FIXED_VALUE
            case.setup_context(c, m, t, inert, dt, pt, comm=comm, schemes=schemes)
            for e in ("U", "Y", "E", "k", "epsilon"):
                c.set_solver(e, 300, 1e-14, 1e-300)
            c.set_solver("p", 3000, 1e-14, 1e-300)
            ws = W.default_setup(m, "all")
            ws.apply(c)
            c.set_option("ras.Prt", 0.85); c.set_option("ras.Sct", 0.7)
            c.set_option("ras.model", 1)
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            for n, v in (("k", k[g]), ("epsilon", eps[g])):
                c.set_field(n, np.ascontiguousarray(v))
                c.set_field("boundary_" + n, case.boundary_values(m, v).reshape(-1))
            c.call("pre_time_step")
            c.time_step(2)
            o = {n: c.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he", "k", "epsilon", "nut", "G")}
            o["U"] = c.get_field("U", (3, m.n_cells))
            o["Y"] = c.get_field("Y", (t.S, m.n_cells))
            B = m.n_boundary_slots
            sl = NR.Slots(m)
            phys = sl.prim & ~sl.coupled
            for n in ("boundary_nut", "boundary_yPlus", "boundary_epsilon"):
                s = np.zeros(m.n_cells)
                np.add.at(s, sl.cell[phys], c.get_field(n, (B,))[phys])
                o["sum_" + n] = s
            return o
        finally:
            c.close()

    ref = run(mg, np.arange(mg.n_cells))
    meshes = decompose(mg, part)
    nr = len(meshes)
    out, err = [None] * nr, [None] * nr
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            out[r] = run(meshes[r], meshes[r].cell_map, comm={"hub": hub, "nranks": nr, "rank": r})
        except Exception as e:   # surfaced below
            err[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not any(x.is_alive() for x in th), "decomposed run hung"
    for e in err:
        if e is not None:
            raise e
    for n, kk in (("T", 1), ("p", 1), ("rho", 1), ("he", 1), ("k", 1), ("epsilon", 1), ("nut", 1), ("U", 3), ("Y", t.S),
                  ("sum_boundary_nut", 1), ("sum_boundary_yPlus", 1), ("sum_boundary_epsilon", 1)):
        a = np.zeros((kk, mg.n_cells))
        for r in range(nr):
            a[:, meshes[r].cell_map] = out[r][n].reshape(kk, -1)
        e = rel_err(a, ref[n].reshape(kk, -1))
        print("sheared-walls two ranks vs single domain", n, f"{e:.2e}")
        assert e < 1e-9, (n, e)
    assert rel_err(ref["k"], k) > 1e-6 and ref["sum_boundary_yPlus"].max() > 0 and ref["sum_boundary_nut"].max() > 0


# ------------------------------------------------------------------------------------------------ 8. unused
def test_nothing_changes_when_unused():
    a, b = Case("walls"), Case("walls")
    try:
        m = a.m
        st = R.ras_state(m)
        for i in range(len(m.patches)):                                          # parameters, but none of the patch types
            a.ctx.set_patch_param("nut", i, "E", 5.0)
            a.ctx.set_patch_param("nut", i, "kappa", 0.3)
            a.ctx.set_patch_param("nut", i, "Cmu", 0.2)
            a.ctx.set_patch_param("k", i, "intensity", 0.1)
            a.ctx.set_patch_param("epsilon", i, "mixingLength", 1e-3)
        res = []
        for x in (a, b):
            x.push(st)
            _tight(x.ctx)
            x.ctx.kernel_timer(NEW_KERNELS)
            x.ctx.turbulence_correct()
            x.ctx.time_step(2)
            assert all(x.ctx.kernel_time(k)[1] == 0 for k in NEW_KERNELS.split(","))
            x.ctx.kernel_timer("")
            r = {n: x.get(n) for n in ("k", "epsilon", "nut", "G", "divU", "boundary_nut", "boundary_k", "boundary_epsilon")}
            r.update(_fields(x.ctx, m, x.t))
            res.append(r)
        for n, v in res[0].items():
            assert np.array_equal(v, res[1][n]), n
        assert not a.get("boundary_yPlus").any()
    finally:
        a.ctx.close(); b.ctx.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_name_their_subject():
    from dfmi.lib import DfmiError
    from dfmi.mesh import hex_box
    c = Case("walls")
    ctx, m = c.ctx, c.m
    try:
        P = len(m.patches)
        zg = m.patch_types(R.ZG)

        def types(code, patch=0):
            t = zg.copy(); t[patch] = code
            return t
        # a new code on the wrong field
        for field, code, name in (("k", 13, "epsilonWallFunction"), ("epsilon", 14, "nutkWallFunction"), ("U", 13, "epsilonWallFunction"),
                                  ("epsilon", 15, "turbulentIntensityKineticEnergyInlet"), ("nut", 15, "turbulentIntensityKineticEnergyInlet"),
                                  ("k", 16, "turbulentMixingLengthDissipationRateInlet"), ("p", 14, "nutkWallFunction")):
            with pytest.raises(DfmiError, match=f"patch 0: {name} .*'{field}'"):
                ctx.set_patch_types(field, types(code))
        with pytest.raises(DfmiError, match="unsupported boundary condition code 17"):
            ctx.set_patch_types("epsilon", types(17))
        # code 13 without code 14 on the same patch: at the correct and on the validation path
        c.push(R.ras_state(m))
        ctx.set_patch_types("epsilon", types(13, 4))
        nut = m.patch_types(R.CALC).copy(); nut[3] = 14
        ctx.set_patch_types("nut", nut)
        for call in (ctx.turbulence_correct, lambda: ctx.call("U_process"), lambda: ctx.assemble("epsilon")):
            with pytest.raises(DfmiError, match="patch 4: epsilonWallFunction .* nutkWallFunction"):
                call()
        nut[4] = 14
        ctx.set_patch_types("nut", nut)
        ctx.turbulence_correct()                                                  # nut alone on patch 3 is allowed
        # a missing intensity or mixing length, at the first correct
        ctx.set_patch_types("k", types(15, 2))
        with pytest.raises(DfmiError, match="patch 2: turbulentIntensityKineticEnergyInlet without an intensity"):
            ctx.turbulence_correct()
        ctx.set_patch_param("k", 2, "intensity", 0.05)
        et = types(13, 4); et[2] = 16
        ctx.set_patch_types("epsilon", et)
        with pytest.raises(DfmiError, match="patch 2: turbulentMixingLengthDissipationRateInlet without a mixing length"):
            ctx.turbulence_correct()
        ctx.set_patch_param("epsilon", 2, "mixingLength", 1e-3)
        ctx.turbulence_correct()
        # non-positive and non-finite parameters, unknown parameters, patches out of range
        for f, n in (("nut", "Cmu"), ("nut", "kappa"), ("nut", "E"), ("k", "intensity"), ("epsilon", "mixingLength")):
            for bad in (0.0, -1.0, float("nan"), float("inf")):
                with pytest.raises(DfmiError, match=rf"\('{f}', '{n}'\) of patch 1 must be positive and finite"):
                    ctx.set_patch_param(f, 1, n, bad)
        for f, n in (("k", "mixingLength"), ("epsilon", "intensity"), ("nut", "intensity"), ("k", "E"), ("U", "Cmu")):
            with pytest.raises(DfmiError, match=rf"got \('{f}', '{n}'\)"):
                ctx.set_patch_param(f, 0, n, 1.0)
        with pytest.raises(DfmiError, match="patch index out of range"):
            ctx.set_patch_param("nut", P, "E", 9.8)
        with pytest.raises(DfmiError, match="boundary_yPlus"):
            ctx.set_field("boundary_yPlus", np.zeros(m.n_boundary_slots))
    finally:
        ctx.close()
    # a new code on a cyclic patch
    pm = R.get_mesh("periodic-even")
    p = Case("periodic-even")
    try:
        cyc = [i for i, x in enumerate(pm.patches) if x.kind == "cyclic"]
        assert cyc
        for field, code, name in (("epsilon", 13, "epsilonWallFunction"), ("nut", 14, "nutkWallFunction"),
                                  ("k", 15, "turbulentIntensityKineticEnergyInlet"),
                                  ("epsilon", 16, "turbulentMixingLengthDissipationRateInlet")):
            t = pm.patch_types(R.ZG).copy(); t[cyc[0]] = code
            with pytest.raises(DfmiError, match=f"patch {cyc[0]}: {name} on a cyclic patch"):
                p.ctx.set_patch_types(field, t)
    finally:
        p.ctx.close()
