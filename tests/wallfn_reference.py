"""NumPy restatement of the k-epsilon wall functions and turbulent inlets (include/dfmi.h dfmi_turbulence_correct, RAS
block), in fp64 and in long double, in the stated operation order, and the oracle of a k-epsilon time step
between wall-function walls.

    per wall patch:   Cmu25 = sqrt(sqrt(Cmu));  Cmu75 = Cmu25 sqrt(Cmu);  yPlusLam: ypl = 11, ten times log(max(E ypl, 1)) / kappa
    per wall slot b:  y = 1 / deltaCoeffs_b;  nuw = boundary_mu_b / boundary_rho_b;  yPlus = ((Cmu25 y) sqrt(k_c)) / nuw
    nutkWallFunction: boundary_nut_b = yPlus > yPlusLam ? nuw ((yPlus kappa) / log(E yPlus) - 1) : 0
    epsilonWallFunction, per cell with n >= 1 such slots, w = 1 / n, slots ascending:
        yPlus > yPlusLam:  eps += ((w Cmu75) (k sqrt k)) / (kappa y);  G += ((((w (nutw + nuw)) magGradUw) Cmu25) sqrt k) / (kappa y)
        otherwise:         eps += (((w 2) k) nuw) / (y y)
    the constraint:   fvMatrix::setValues of the epsilon matrix on those cells (constrain)
    inlets:           k_ref = (1.5 (I I)) ((Ux Ux + Uy Uy) + Uz Uz);  eps_ref = (Cmu75 / L) (kb sqrt(kb))

Topo, scalar_assemble, RasOracle and the rest come from ras_reference unchanged.

`python tests/wallfn_reference.py --measure` evaluates the fp64 restatement against long double on wall_state of the GPU
suite's four meshes and writes the maxima to tests/golden/wallfn_bounds.json:
    boundary_nut over nuw max(1, yPlus kappa / log(E yPlus))   (the subtraction cancels at yPlusLam)
    boundary_yPlus, relative;  the wall cells' epsilon, relative;  the wall cells' G over sum of its terms' magnitudes
The device bounds derive from that file (gpu_bound: 4x, floored at 1e-13), never from a kernel's output.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ras_reference as R   # noqa: E402
from ras_reference import LD, NR, Topo, scalar_assemble, RasOracle   # noqa: E402,F401

BOUNDS_PATH = os.path.join(R.GOLDEN, "wallfn_bounds.json")
MESHES = ("walls", "rod", "sheared-walls", "prisms")
EPS_WALL, NUT_WALL, K_INLET, EPS_INLET = 13, 14, 15, 16
WALL_DEFAULTS = {"Cmu": 0.09, "kappa": 0.41, "E": 9.8}
YZ_WALLS = ("top", "down", "front", "back")


def device_types(pt):
    """what the slots of the four codes are to the generic assembly, the post-solve correction and bound(): the wall
    functions hold fixed values, the inlets are inletOutlet"""
    pt = np.asarray(pt).copy()
    pt[(pt == EPS_WALL) | (pt == NUT_WALL)] = R.FV
    pt[(pt == K_INLET) | (pt == EPS_INLET)] = R.INLET_OUTLET
    return pt


def y_plus_lam(kappa, E, T=np.float64):
    ypl = T(11.0)
    for _ in range(10):
        ypl = np.log(max(T(E) * ypl, T(1.0))) / T(kappa)
    return ypl


class WallSetup:
    """the patch types of k, epsilon and nut with the four codes on the patches named, and the per-patch parameters:
    walls: names of the wall-function patches (epsilon 13, nut 14, k zeroGradient = kqRWallFunction); inlets: {name:
    (intensity, mixingLength)} (k 15, epsilon 16, nut calculated); params: {name: {"Cmu" | "kappa" | "E": v}}"""

    def __init__(self, m, walls=(), inlets=None, params=None, outlets=()):
        self.m = m
        inlets = inlets or {}
        params = params or {}
        self.k_pt, self.eps_pt = m.patch_types(R.ZG).copy(), m.patch_types(R.ZG).copy()
        self.nut_pt = m.patch_types(R.CALC).copy()
        P = len(m.patches)
        self.par = {n: np.full(P, v) for n, v in WALL_DEFAULTS.items()}
        self.par["intensity"], self.par["mixingLength"] = np.zeros(P), np.zeros(P)
        for i, p in enumerate(m.patches):
            if p.name in walls:
                self.eps_pt[i], self.nut_pt[i] = EPS_WALL, NUT_WALL
            if p.name in inlets:
                self.k_pt[i], self.eps_pt[i] = K_INLET, EPS_INLET
                self.par["intensity"][i], self.par["mixingLength"][i] = inlets[p.name]
            if p.name in outlets:
                self.k_pt[i] = self.eps_pt[i] = R.INLET_OUTLET
            for n, v in params.get(p.name, {}).items():
                self.par[n][i] = v
        slots = [p.slots for p in m.patches]
        self.patch = np.repeat(np.arange(P), slots)
        self.eps_wall = NR.slot_types(m, self.eps_pt) == EPS_WALL
        self.nut_wall = NR.slot_types(m, self.nut_pt) == NUT_WALL
        self.k_inlet = NR.slot_types(m, self.k_pt) == K_INLET
        self.eps_inlet = NR.slot_types(m, self.eps_pt) == EPS_INLET
        self.cell = NR.Slots(m).cell
        self.bdc = np.asarray(m.boundary_arrays()[2])

    def apply(self, ctx):
        """the types and parameters on a context"""
        ctx.set_patch_types("k", self.k_pt)
        ctx.set_patch_types("epsilon", self.eps_pt)
        ctx.set_patch_types("nut", self.nut_pt)
        for i in range(len(self.m.patches)):
            if self.nut_pt[i] == NUT_WALL:
                for n in WALL_DEFAULTS:
                    ctx.set_patch_param("nut", i, n, self.par[n][i])
            if self.k_pt[i] == K_INLET:
                ctx.set_patch_param("k", i, "intensity", self.par["intensity"][i])
            if self.eps_pt[i] == EPS_INLET:
                ctx.set_patch_param("epsilon", i, "mixingLength", self.par["mixingLength"][i])

    def consts(self, T=np.float64):
        """per slot: Cmu25, Cmu75, kappa, E, yPlusLam"""
        Cmu = np.asarray(self.par["Cmu"], T)
        c25 = np.sqrt(np.sqrt(Cmu))
        c75 = c25 * np.sqrt(Cmu)
        ypl = np.array([y_plus_lam(k_, e_, T) for k_, e_ in zip(self.par["kappa"], self.par["E"])], T)
        p = self.patch
        return c25[p], c75[p], np.asarray(self.par["kappa"], T)[p], np.asarray(self.par["E"], T)[p], ypl[p]


def y_plus(ws, k, bmu, brho, T=np.float64):
    """(yPlus, y, nuw) per slot (meaningful on wall slots)"""
    c25 = ws.consts(T)[0]
    y = T(1.0) / np.asarray(ws.bdc, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        nuw = np.asarray(bmu, T) / np.asarray(brho, T)
        yp = ((c25 * y) * np.sqrt(np.asarray(k, T)[ws.cell])) / nuw
    return yp, y, nuw


def wall_nut(ws, k, bmu, brho, T=np.float64):
    """(boundary_nut of the nutkWallFunction slots, 0 elsewhere; boundary_yPlus, 0 elsewhere)"""
    _, _, kap, E, ypl = ws.consts(T)
    yp, _, nuw = y_plus(ws, k, bmu, brho, T)
    on = ws.nut_wall
    out, byp = np.zeros(len(on), T), np.zeros(len(on), T)
    byp[on] = yp[on]
    tur = on & (np.where(on, yp, 0) > ypl)
    out[tur] = nuw[tur] * ((yp[tur] * kap[tur]) / np.log(E[tur] * yp[tur]) - T(1.0))
    return out, byp


def wall_update(ws, tp, k, U, bU, bmu, brho, bnut, eps, G, beps, T=np.float64):
    """(epsilon, G, boundary_epsilon, constrained [C] bool, G scale [C]) after the epsilonWallFunction update: copies of
    eps / G / beps with the wall cells and slots replaced; the scale is the sum of the magnitudes of G's terms"""
    c25, c75, kap, _, ypl = ws.consts(T)
    yp, y, nuw = y_plus(ws, k, bmu, brho, T)
    k, U, bU, bnut = (np.asarray(a, T) for a in (k, U, bU, bnut))
    bdc = np.asarray(ws.bdc, T)
    eps, G, beps = np.array(eps, T), np.array(G, T), np.array(beps, T)
    C_ = len(k)
    con, scale = np.zeros(C_, bool), np.zeros(C_, T)
    for c in range(C_):
        sl = [b for b in tp.slots[c] if ws.eps_wall[b]]
        if not sl:
            continue
        con[c] = True
        w = T(1.0) / T(len(sl))
        kc = k[c]
        sk = np.sqrt(kc)
        e = g = s = T(0.0)
        for b in sl:
            if yp[b] > ypl[b]:
                dx, dy, dz = bU[0, b] - U[0, c], bU[1, b] - U[1, c], bU[2, b] - U[2, c]
                mg = bdc[b] * np.sqrt((dx * dx + dy * dy) + dz * dz)
                e = e + ((w * c75[b]) * (kc * sk)) / (kap[b] * y[b])
                t = ((((w * (bnut[b] + nuw[b])) * mg) * c25[b]) * sk) / (kap[b] * y[b])
                g = g + t
                s = s + abs(t)
            else:
                e = e + (((w * T(2.0)) * kc) * nuw[b]) / (y[b] * y[b])
        eps[c], G[c], scale[c] = e, g, s
        for b in sl:
            beps[b] = e
    return eps, G, beps, con, scale


def constrain(tp, o, con, v):
    """fvMatrix::setValues on the cells con with the values v[c], on a matrix of scalar_assemble (in place): a
    constrained cell gets source = v diag, zero off-diagonals and zero slot coefficients; an unconstrained one
    source -= A[c][n] v_n once per constrained neighbour in the sequential face order"""
    lower, upper = o["lower"].copy(), o["upper"].copy()
    for c in range(len(con)):
        if con[c]:
            o["source"][c] = v[c] * o["diag"][c]
            for b in tp.slots[c]:
                o["internal_coeffs"][b] = 0.0
                o["boundary_coeffs"][b] = 0.0
            continue
        s = o["source"][c]
        for f, n, own in tp.faces[c]:
            if con[n]:
                s -= (upper[f] if own else lower[f]) * v[n]
        o["source"][c] = s
    for c in range(len(con)):
        for f, n, own in tp.faces[c]:
            if own and (con[c] or con[n]):
                o["lower"][f] = 0.0
                o["upper"][f] = 0.0
    return o


def inlet_k_ref(ws, bU, ref=None, T=np.float64):
    bU = np.asarray(bU, T)
    ref = np.zeros(bU.shape[1], T) if ref is None else np.array(ref, T)
    I = np.asarray(ws.par["intensity"], T)[ws.patch]
    on = ws.k_inlet
    ux, uy, uz = bU[0, on], bU[1, on], bU[2, on]
    ref[on] = (T(1.5) * (I[on] * I[on])) * ((ux * ux + uy * uy) + uz * uz)
    return ref


def inlet_eps_ref(ws, Cmu, bk, ref=None, T=np.float64):
    bk = np.asarray(bk, T)
    ref = np.zeros(len(bk), T) if ref is None else np.array(ref, T)
    c75 = np.sqrt(np.sqrt(T(Cmu))) * np.sqrt(T(Cmu))
    L = np.asarray(ws.par["mixingLength"], T)[ws.patch]
    on = ws.eps_inlet
    ref[on] = (c75 / L[on]) * (bk[on] * np.sqrt(bk[on]))
    return ref


# ------------------------------------------------------------------------------------------------ states
def wall_state(m, ws, seed=31):
    """ras_state with no-slip walls (boundary_U = 0 on the wall-function slots), k of order 30 and boundary_mu of the
    wall slots scaled so that their yPlus is log-uniform over about 1 to 300 (one target per cell: a cell's slots
    differ by their wall distances)"""
    st = R.ras_state(m)
    rng = np.random.default_rng(seed)
    k = 30.0 * (1.0 + 0.5 * rng.uniform(-1, 1, m.n_cells))
    eps = 4e5 * (1.0 + 0.5 * rng.uniform(-1, 1, m.n_cells))
    from dfmi import case
    st["k"], st["epsilon"] = k, eps
    st["boundary_k"] = case.boundary_values(m, k).reshape(-1)
    st["boundary_epsilon"] = case.boundary_values(m, eps).reshape(-1)
    target = np.exp(rng.uniform(np.log(1.0), np.log(300.0), m.n_cells))
    on = ws.eps_wall | ws.nut_wall
    c25 = ws.consts()[0]
    y = 1.0 / ws.bdc
    bmu = st["boundary_mu"].copy()
    bmu[on] = (st["boundary_rho"][on] * (c25[on] * y[on]) * np.sqrt(k[ws.cell[on]])) / target[ws.cell[on]]
    st["boundary_mu"] = bmu
    bU = st["boundary_U"].copy()
    bU[:, on] = 0.0
    st["boundary_U"] = bU
    st["nut"] = R.nut_of(0.09, k, eps)
    return st


def state_conditions(ws, st):
    """(fraction of wall slots below yPlusLam, fraction above, the closest relative distance to it, min k, min epsilon)"""
    yp, _, _ = y_plus(ws, st["k"], st["boundary_mu"], st["boundary_rho"])
    ypl = ws.consts()[4]
    on = ws.nut_wall
    lo, hi = (yp[on] <= ypl[on]).mean(), (yp[on] > ypl[on]).mean()
    return lo, hi, np.abs(yp[on] / ypl[on] - 1).min(), st["k"].min(), st["epsilon"].min(), yp[on].min(), yp[on].max()


def wall_errors(ws, tp, st, bnut, byp, eps, G, bnut_in=None):
    """the four error measures of the bounds file for values (bnut, byp, eps, G) formed from the state st (G / eps from
    the boundary_nut bnut_in, default the long-double wall_nut): each the maximum over the wall slots / wall cells"""
    L_bnut, L_byp = wall_nut(ws, st["k"], st["boundary_mu"], st["boundary_rho"], LD)
    _, _, kap, E, ypl = ws.consts(LD)
    yp, _, nuw = y_plus(ws, st["k"], st["boundary_mu"], st["boundary_rho"], LD)
    on = ws.nut_wall
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = nuw * np.maximum(LD(1.0), np.where(yp > 1 / E, yp * kap / np.log(E * yp), 0))
    e_nut = np.abs(np.asarray(bnut, LD)[on] - L_bnut[on]) / sc[on]
    e_yp = np.abs(np.asarray(byp, LD)[on] / L_byp[on] - 1)
    f = lambda a: float(np.max(a)) if len(a) else 0.0   # noqa: E731
    if eps is None:
        return {"boundary_nut": f(e_nut), "boundary_yPlus": f(e_yp)}
    src = L_bnut if bnut_in is None else bnut_in
    zC = np.zeros(len(st["k"]))
    L_eps, L_G, _, con, scale = wall_update(ws, tp, st["k"], st["U"], st["boundary_U"], st["boundary_mu"], st["boundary_rho"],
                                            src, zC, zC, np.zeros(len(on)), LD)
    e_eps = np.abs(np.asarray(eps, LD)[con] / L_eps[con] - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_G = np.where(scale[con] > 0, np.abs(np.asarray(G, LD)[con] - L_G[con]) / np.where(scale[con] > 0, scale[con], 1), 0)
    return {"boundary_nut": f(e_nut), "boundary_yPlus": f(e_yp), "epsilon": f(e_eps), "G": f(e_G)}


def default_setup(m, which="all"):
    names = [p.name for p in m.patches if p.kind == "wall"] if which == "all" else list(YZ_WALLS)
    return WallSetup(m, walls=names)


def measure():
    out = {}
    for name in MESHES:
        m = R.get_mesh(name)
        ws = default_setup(m)
        st = wall_state(m, ws)
        tp = Topo(m)
        bnut, byp = wall_nut(ws, st["k"], st["boundary_mu"], st["boundary_rho"])
        zC = np.zeros(m.n_cells)
        eps, G, _, _, _ = wall_update(ws, tp, st["k"], st["U"], st["boundary_U"], st["boundary_mu"], st["boundary_rho"], bnut,
                                      zC, zC, np.zeros(m.n_boundary_slots))
        out[name] = wall_errors(ws, tp, st, bnut, byp, eps, G, bnut_in=np.asarray(bnut, LD))
    return out


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def gpu_bound(bounds, mesh_name, what):
    """4x the fp64 restatement's measured maximum on that mesh, floored at 1e-13"""
    return max(4.0 * bounds["meshes"][mesh_name][what], 1e-13)


# ------------------------------------------------------------------------------------------------ oracle
class WallOracle(RasOracle):
    """RasOracle with wall functions and turbulent inlets: turbulence_correct in kEpsilon::correct()'s order -- k's
    inletValue, G and divU, the wall update and epsilon's inletValue, the epsilon equation assembled, constrained and
    solved, bound, the k equation with the modified G, bound, correctNut() with the wall slots"""

    def __init__(self, mesh, table, state, ptypes, inert, rdt, ras, k, epsilon, bk, beps, wall, schemes=None):
        self.wall = wall
        B = mesh.n_boundary_slots
        self.k_ref, self.eps_ref, self.yPlus = np.zeros(B), np.zeros(B), np.zeros(B)
        super().__init__(mesh, table, state, ptypes, inert, rdt, ras, k, epsilon, bk, beps, schemes=schemes,
                         k_ptypes=device_types(wall.k_pt), eps_ptypes=device_types(wall.eps_pt),
                         nut_ptypes=device_types(wall.nut_pt))

    def correct_nut(self):
        super().correct_nut()
        a, ws = self.arr, self.wall
        bn, self.yPlus = wall_nut(ws, a["k"], a["boundary_mu"], a["boundary_rho"])
        a["boundary_nut"][ws.nut_wall] = bn[ws.nut_wall]

    def _mixed(self, nm, pt, ref):
        """inletOutlet slots after correct_bc: vf ref + (1 - vf) cell"""
        a = self.arr
        ts = NR.slot_types(self.m, pt)
        on = ts == R.INLET_OUTLET
        if on.any():
            vf = np.where(a["boundary_phi"][on] >= 0, 0.0, 1.0)
            a["boundary_" + nm][on] = vf * ref[on] + (1.0 - vf) * a[nm][self.wall.cell[on]]

    def _equation(self, keq, G, dv, con=None):
        a, q = self.arr, self.q
        nm = "k" if keq else "epsilon"
        pt = self.k_pt if keq else self.eps_pt
        ref = self.k_ref if keq else self.eps_ref
        Su, Sp = R.sources(keq, q, G, dv, a["rho"], a["k"], a["epsilon"])
        sig = q["sigmak"] if keq else q["sigmaEps"]
        D = R.diffusivity(a["rho"], a["nut"], a["mu"], sig)
        bD = R.diffusivity(a["boundary_rho"], a["boundary_nut"], a["boundary_mu"], sig)
        o = scalar_assemble(self.tp, pt, a[nm], a["boundary_" + nm], a["rho"], a["rho_old"], a["phi"], a["boundary_phi"],
                            D, bD, Su, Sp, self.rdt, ref=ref)
        if con is not None and con.any():
            constrain(self.tp, o, con, a[nm].copy())
        self.ptypes[nm] = pt
        a[nm][...] = self.solve_ldu(o["lower"], o["upper"], o["diag"], o["source"], o["internal_coeffs"],
                                    o["boundary_coeffs"], nm)
        self.correct_bc(nm, nm, 1)
        self._mixed(nm, pt, ref)
        lo = q["kMin"] if keq else q["epsilonMin"]
        a[nm][...], a["boundary_" + nm][...] = R.bound(self.tp, pt, a[nm], a["boundary_" + nm], lo)
        return o

    def turbulence_correct(self):
        if not self._ras_ready:
            return
        a, ws = self.arr, self.wall
        self.k_ref = inlet_k_ref(ws, a["boundary_U"], self.k_ref)
        G = R.production(self.grad_u(), a["nut"])
        dv, _ = R.div_u(self.tp, self.ptypes["rho"], a["phi"], a["boundary_phi"], a["rho"], a["boundary_rho"])
        eps, G, beps, con, _ = wall_update(ws, self.tp, a["k"], a["U"], a["boundary_U"], a["boundary_mu"], a["boundary_rho"],
                                           a["boundary_nut"], a["epsilon"], G, a["boundary_epsilon"])
        a["epsilon"][...], a["boundary_epsilon"][...] = eps, beps
        self.eps_ref = inlet_eps_ref(ws, self.q["Cmu"], a["boundary_k"], self.eps_ref)
        self.G, self.divU, self.con = G, dv, con
        self._equation(0, G, dv, con)
        self._equation(1, G, dv)
        self.correct_nut()


if __name__ == "__main__":
    if "--measure" not in sys.argv:
        sys.exit("usage: wallfn_reference.py --measure")
    doc = {"about": "max over the wall slots / wall cells of the fp64 NumPy restatement's error against long double on "
                    "wall_state of the GPU suite's meshes (tests/wallfn_reference.py): boundary_nut over nuw max(1, yPlus "
                    "kappa / log(E yPlus)), boundary_yPlus relative, the wall cells' epsilon relative, the wall cells' G over "
                    "the sum of its terms' magnitudes; written by tests/wallfn_reference.py --measure",
           "meshes": measure()}
    with open(BOUNDS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, v in doc["meshes"].items():
        print(name, {c: f"{x:.2e}" for c, x in v.items()})
