"""NumPy restatement of the RAS k-epsilon model (include/dfmi.h dfmi_turbulence_correct, RAS block), in fp64
and in long double, in the stated operation order, and the oracle of a k-epsilon time step.

    divU  = (1/V) [ sum_f +-phi_f / interp_f(w, rho_P, rho_N) + sum_slots boundary_phi / boundary_rho ]
    G     = nut (dev(twoSymm(g)) && g)
    D     = rho (nut / sigma + mu / rho)                                   (cells and slots alike)
    eps:    ddt(rho,eps) + div(phi,eps) - laplacian(Deps,eps) == C1 rho G eps/k - SuSp((2/3 C1 - C3) rho divU, eps) - Sp(C2 rho eps/k, eps)
    k:      ddt(rho,k) + div(phi,k) - laplacian(Dk,k) == rho G - SuSp(2/3 rho divU, k) - Sp(rho eps/k, k)
    bound(psi, m): psi = max(max(psi, avg(max(psi,m)) pos0(-psi)), m);  nut = Cmu k^2 / eps

Per-cell Python loops walk a cell's faces in the sequential order (neighbour faces ascending, owned faces ascending,
then its boundary slots), so with the same inputs the matrices equal the device's bit for bit. The Gauss gradients are
nonorth_reference.gauss_grad (any precision) or, for a RasOracle, the oracle's orc_grad_scalar as LesOracle.grad_u.

`python tests/ras_reference.py --measure` evaluates G and divU in fp64 against long double on every test mesh's state
(ras_state) and writes the maxima of |G64 - GL| / (nut |g|^2) and |divU64 - divUL| / (sum_f |phi_f / rho_f| / V) to
tests/golden/ras_bounds.json; the device bounds derive from that file (gpu_bound), never from a kernel's output.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUNDS_PATH = os.path.join(GOLDEN, "ras_bounds.json")
for _p in (os.path.join(os.path.dirname(HERE), "deepflame-dev_amd"), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import nonorth_reference as NR   # noqa: E402
from les_reference import LesOracle   # noqa: E402

LD = np.longdouble
DEFAULTS = {"Cmu": 0.09, "C1": 1.44, "C2": 1.92, "C3": 0.0, "sigmak": 1.0, "sigmaEps": 1.3, "kMin": 1e-15,
            "epsilonMin": 1e-15, "Prt": 1.0, "Sct": 1.0}
ZG, FV, EMPTY, CALC, CYCLIC, PROC, EXTRAP, PROC_CYC, INLET_OUTLET = 0, 1, 3, 5, 6, 7, 8, 10, 12
COUPLED = (CYCLIC, PROC, PROC_CYC)
MESHES = ("walls", "periodic-even", "periodic-odd", "sheared-walls", "refined", "prisms", "rod", "prisms-large")
L0 = NR.L0
_cache = {}


def get_mesh(name):
    """the GPU suite's meshes by name (built once per process; read-only)"""
    if name not in _cache:
        from dfmi.mesh import hex_box
        import unstructured_meshes as um
        if name == "walls":
            m = hex_box(6, 5, 4, lengths=(L0,) * 3, periodic=(False,) * 3, gradings=(1.0, 1.4, 1.0))
        elif name == "periodic-even":   # 2-colourable: the even-odd solver path
            m = hex_box(8, 6, 4, lengths=(L0,) * 3, periodic=(True,) * 3, gradings=(1.0, 1.3, 1.0))
        elif name == "periodic-odd":    # odd periodic directions: the Jacobi path
            m = hex_box(7, 6, 5, lengths=(L0,) * 3, periodic=(True,) * 3, gradings=(1.0, 1.3, 1.0))
        elif name == "rod":             # 257 cells in a row: one cell past the first workgroup
            m = hex_box(257, 1, 1, lengths=(40 * L0, L0 / 6, L0 / 6), periodic=(False,) * 3)
        elif name == "sheared-walls":
            m = NR.get_mesh("sheared-walls")
        elif name == "prisms-large":
            m = um.get("prisms", size="large")
        else:
            m = um.get(name)
        _cache[name] = m
    return _cache[name]


# ------------------------------------------------------------------------------------------------ topology
class Topo:
    """per cell: its internal faces in the sequential order as (face, other cell, is owner), and its primary boundary
    slots ascending; per slot: cell, cyclic partner cell (-1), patch index"""

    def __init__(self, m):
        C_ = m.n_cells
        own, nei = np.asarray(m.owner, np.int64), np.asarray(m.neighbour, np.int64)
        self.faces = [[] for _ in range(C_)]
        for f in np.argsort(nei, kind="stable"):
            self.faces[nei[f]].append((int(f), int(own[f]), False))
        for f in np.argsort(own, kind="stable"):
            self.faces[own[f]].append((int(f), int(nei[f]), True))
        self.sl = NR.Slots(m)
        self.slots = [[] for _ in range(C_)]
        for b in np.nonzero(self.sl.prim)[0]:
            self.slots[self.sl.cell[b]].append(int(b))
        self.m = m


def _interp_f(w, vo, vn):
    return w * (vo - vn) + vn


def _interp_b(w, vo, vn):
    return w * vo + (1 - w) * vn


def _face_value(tp, ts, b, c, vf, bvf, bw):
    """bface: the stored boundary value, or on a coupled slot the interpolate with the cell across it"""
    if ts[b] in COUPLED:
        pc = tp.sl.partner[b]
        return _interp_b(bw[b], vf[c], vf[pc] if pc >= 0 else bvf[b])
    return bvf[b]


# ------------------------------------------------------------------------------------------------ production
def grad_u(m, ptype_U, U, bU, T=np.float64):
    """g [9, C], g[3 i + j] = d_i U_j (Gauss linear; nonorth_reference.gauss_grad per component)"""
    sl, ts = NR.Slots(m), NR.slot_types(m, ptype_U)
    g = np.zeros((9, m.n_cells), T)
    for j in range(3):
        gj = NR.gauss_grad(m, sl, ts, U[j], bU[j], T)
        for i in range(3):
            g[3 * i + j] = gj[i]
    return g


def dev_two_symm_dd(g, T=np.float64):
    """dev(twoSymm(g)) && g per cell, g [9, n], in the header's operation order"""
    g = np.asarray(g, T)
    T00, T11, T22 = g[0] + g[0], g[4] + g[4], g[8] + g[8]
    T01, T02, T12 = g[1] + g[3], g[2] + g[6], g[5] + g[7]
    t3 = (T(1.0) / T(3.0)) * ((T00 + T11) + T22)
    dg = ((T00 - t3) * g[0] + (T11 - t3) * g[4]) + (T22 - t3) * g[8]
    off = ((T01 * g[1] + T01 * g[3]) + (T02 * g[2] + T02 * g[6])) + (T12 * g[5] + T12 * g[7])
    return dg + off


def production(g, nut, T=np.float64):
    return np.asarray(nut, T) * dev_two_symm_dd(g, T)


def div_u(tp, ptype_rho, phi, bphi, rho, brho, T=np.float64):
    """(divU [C], scale [C] = sum_f |phi_f / rho_f| / V) in the sequential face order"""
    m = tp.m
    ts = NR.slot_types(m, ptype_rho)
    w, V = np.asarray(m.weight, T), np.asarray(m.volume, T)
    bw = np.asarray(m.boundary_arrays()[3], T)
    phi, bphi, rho, brho = (np.asarray(a, T) for a in (phi, bphi, rho, brho))
    out, sc = np.zeros(m.n_cells, T), np.zeros(m.n_cells, T)
    for c in range(m.n_cells):
        dv, s = T(0.0), T(0.0)
        for f, o2, own in tp.faces[c]:
            v = phi[f] / (_interp_f(w[f], rho[c], rho[o2]) if own else _interp_f(w[f], rho[o2], rho[c]))
            dv = dv + v if own else dv - v
            s += abs(v)
        for b in tp.slots[c]:
            if ts[b] == EMPTY:
                continue
            v = bphi[b] / _face_value(tp, ts, b, c, rho, brho, bw)
            dv = dv + v
            s += abs(v)
        out[c], sc[c] = dv / V[c], s / V[c]
    return out, sc


# ------------------------------------------------------------------------------------------------ equations
def diffusivity(rho, nut, mu, sigma, T=np.float64):
    rho, nut, mu = (np.asarray(a, T) for a in (rho, nut, mu))
    return rho * (nut / T(sigma) + mu / rho)


def sources(keq, q, G, divU, rho, k, eps, T=np.float64):
    """(Su, Sp) per unit volume of the epsilon (keq 0) or k (keq 1) equation"""
    G, divU, r, kc, ec = (np.asarray(a, T) for a in (G, divU, rho, k, eps))
    ek = ec / kc
    zero = T(0.0)
    if keq:
        a = ((T(2.0) / T(3.0)) * r) * divU
        return r * G - np.minimum(a, zero) * kc, np.maximum(a, zero) + r * ek
    a = (((T(2.0) / T(3.0)) * T(q["C1"]) - T(q["C3"])) * r) * divU
    return ((T(q["C1"]) * r) * G) * ek - np.minimum(a, zero) * ec, np.maximum(a, zero) + (T(q["C2"]) * r) * ek


def _bcoef(t, bval, w, bdc, bphi_b, ref):
    if t == INLET_OUTLET:
        vf = 0.0 if bphi_b >= 0 else 1.0
        return 1.0 - vf, vf * ref, -vf * bdc, vf * bdc * ref
    if t in (ZG, EXTRAP):
        return 1.0, 0.0, 0.0, 0.0
    if t == FV:
        return 0.0, bval, -1 * bdc, bdc * bval
    return w, 1.0 - w, -1 * bdc, bdc


def scalar_assemble(tp, ptypes, psi, bpsi, rho, rho_old, phi, bphi, D, bD, Su, Sp, rdt, wc=None, bwc=None, ref=None,
                    dc=None, bdc=None):
    """the generic scalar transport assembly (fv_kernels.hip k_scalar_assemble) in fp64: lower / upper / diag / source /
    internal_coeffs / boundary_coeffs. wc / bwc: convection weights (None: upwind); ref: inletValue per slot; dc / bdc:
    the delta coefficients of the laplacian scheme in force (None: the mesh's)"""
    m = tp.m
    ts = NR.slot_types(m, ptypes)
    _, bmag, bdc0, bw, _ = m.boundary_arrays()
    dc = m.delta_coeffs if dc is None else dc
    bdc = bdc0 if bdc is None else bdc
    w, ms, V = m.weight, m.mag_sf, m.volume
    F, B, C_ = m.n_faces, m.n_boundary_slots, m.n_cells
    o = {"lower": np.zeros(F), "upper": np.zeros(F), "diag": np.zeros(C_), "source": np.zeros(C_),
         "internal_coeffs": np.zeros(B), "boundary_coeffs": np.zeros(B)}
    ref = np.zeros(B) if ref is None else ref
    for c in range(C_):
        d1 = dL = 0.0
        Dc = D[c]
        for f, o2, own in tp.faces[c]:
            ph = phi[f]
            wu = wc[f] if wc is not None else (1.0 if ph >= 0 else 0.0)
            L1 = -wu * ph
            U1 = L1 + ph
            UL = dc[f] * ((_interp_f(w[f], Dc, D[o2]) if own else _interp_f(w[f], D[o2], Dc)) * ms[f])
            if own:
                d1 -= L1
                o["lower"][f] = L1 - UL
                o["upper"][f] = U1 - UL
            else:
                d1 -= U1
            dL -= UL
        vol = V[c]
        o["diag"][c] = ((rdt * rho[c] * vol + d1) - dL) + vol * Sp[c]
        o["source"][c] = rdt * rho_old[c] * psi[c] * vol + vol * Su[c]
        for b in tp.slots[c]:
            t = ts[b]
            if t == EMPTY:
                continue
            wu = bwc[b] if bwc is not None else (1.0 if bphi[b] >= 0 else 0.0)
            qc = _bcoef(t, bpsi[b], wu, bdc[b], bphi[b], ref[b])
            ql = _bcoef(t, bpsi[b], bw[b], bdc[b], bphi[b], ref[b])
            if t in COUPLED:
                pc = tp.sl.partner[b]
                gam = _interp_b(bw[b], Dc, D[pc] if pc >= 0 else bD[b])
            else:
                gam = bD[b]
            pG = gam * bmag[b]
            o["internal_coeffs"][b] = bphi[b] * qc[0] - pG * ql[2]
            o["boundary_coeffs"][b] = -bphi[b] * qc[1] - (-pG * ql[3])
    return o


def bound(tp, ptypes, pre, bpre, lo, T=np.float64):
    """bound(psi, lo) of the solved field pre / bpre: (psi, boundary_psi)"""
    m = tp.m
    ts = NR.slot_types(m, ptypes)
    w, ms = np.asarray(m.weight, T), np.asarray(m.mag_sf, T)
    _, bmag, _, bw, _ = m.boundary_arrays()
    bmag, bw = np.asarray(bmag, T), np.asarray(bw, T)
    pre, bpre, lo = np.asarray(pre, T), np.asarray(bpre, T), T(lo)
    out = pre.copy()
    for c in range(m.n_cells):
        pc = pre[c]
        pcb = max(pc, lo)
        num = den = T(0.0)
        for f, o2, own in tp.faces[c]:
            pn = max(pre[o2], lo)
            num = num + ms[f] * (_interp_f(w[f], pcb, pn) if own else _interp_f(w[f], pn, pcb))
            den = den + ms[f]
        for b in tp.slots[c]:
            if ts[b] == EMPTY:
                continue
            if ts[b] in COUPLED:      # a face like any other: the interpolate of the two bounded cell values
                pn = tp.sl.partner[b]
                fv = _interp_b(bw[b], pcb, max(pre[pn] if pn >= 0 else bpre[b], lo))
            else:
                fv = max(bpre[b], lo)
            num = num + bmag[b] * fv
            den = den + bmag[b]
        out[c] = max(max(pc, (num / den) * (T(1.0) if -pc >= 0 else T(0.0))), lo)
    return out, np.maximum(bpre, lo)


def nut_of(Cmu, k, eps, T=np.float64):
    k, eps = np.asarray(k, T), np.asarray(eps, T)
    return (T(Cmu) * (k * k)) / eps


def boundary_nut(m, nut_ptypes, Cmu, nut, bk, beps, stored):
    """boundary_nut: calculated slots Cmu bk^2 / beps, fixedValue the stored value, zeroGradient the cell value, cyclic
    the interpolate (processor slots: not on a single domain)"""
    from dfmi import case
    ts = NR.slot_types(m, nut_ptypes)
    b = case.boundary_values(m, nut).reshape(-1)
    calc = ts == CALC
    b[calc] = nut_of(Cmu, bk[calc], beps[calc])
    b[ts == FV] = stored[ts == FV]
    return b


def decay(k0, eps0, dt, q=None):
    """homogeneous decay of one step: (eps1, k1, nut1)"""
    q = dict(DEFAULTS, **(q or {}))
    e1 = eps0 / (1 + q["C2"] * dt * eps0 / k0)
    k1 = k0 / (1 + dt * e1 / k0)
    return e1, k1, q["Cmu"] * k1 * k1 / e1


# ------------------------------------------------------------------------------------------------ limited weights
def limited_weights(tp, ptypes, kcoef, phi, bphi, v, bv, g):
    """limitedLinear <k> weights (fv_kernels.hip k_lim_w_face / k_lim_w_slot, b01 = 0) from the gradient g [3, C]"""
    m = tp.m
    ts = NR.slot_types(m, ptypes)
    twoByk = 2.0 / max(kcoef, 1e-15)
    md, bd = np.asarray(m.mesh_distance), m.boundary_delta()
    bw = m.boundary_arrays()[3]

    def lim(ph, vP, vN, gu, dv):
        gradf = vN - vP
        gradcf = dv[0] * gu[0] + dv[1] * gu[1] + dv[2] * gu[2]
        sg = lambda x: 1.0 if x >= 0 else -1.0   # noqa: E731
        if abs(gradcf) >= 1000 * abs(gradf):
            r = 2 * 1000 * sg(gradcf) * sg(gradf) - 1
        else:
            r = 2 * (gradcf / gradf) - 1
        return max(min(twoByk * r, 1.0), 0.0)
    wo, bwo = np.zeros(m.n_faces), np.zeros(m.n_boundary_slots)
    for f in range(m.n_faces):
        o, n, ph = m.owner[f], m.neighbour[f], phi[f]
        cu = o if ph > 0 else n
        l_ = lim(ph, v[o], v[n], g[:, cu], md[f])
        wo[f] = l_ * m.weight[f] + (1 - l_) * (1.0 if ph >= 0 else 0.0)
    for b in range(m.n_boundary_slots):
        l_ = 1.0
        ph = bphi[b]
        if ts[b] in COUPLED and tp.sl.prim[b]:
            c, pc = tp.sl.cell[b], tp.sl.partner[b]
            l_ = lim(ph, v[c], v[pc], g[:, c] if ph > 0 else g[:, pc], bd[b])
        bwo[b] = l_ * bw[b] + (1 - l_) * (1.0 if ph >= 0 else 0.0)
    return wo, bwo


# ------------------------------------------------------------------------------------------------ states
def ras_state(m, seed=29):
    """a noisy Taylor-Green state for the production tests, formed without a GPU: U (3 % noise, so tr g takes both signs),
    rho of the thermo state (nonorth_reference.case_state), phi = (rho U)_f . Sf, positive k and epsilon; boundary values
    as correctBoundaryConditions leaves zeroGradient / cyclic slots"""
    from dfmi import case
    st = NR.case_state(m)
    rng = np.random.default_rng(seed)
    U = st["U"] + 0.03 * 4.0 * rng.standard_normal(st["U"].shape)
    rho = st["rho"]
    k = 0.3 * (1.0 + 0.5 * rng.uniform(-1, 1, m.n_cells))
    eps = 2e3 * (1.0 + 0.5 * rng.uniform(-1, 1, m.n_cells))
    B = m.n_boundary_slots
    out = {"U": U, "rho": rho, "mu": st["mu"], "k": k, "epsilon": eps}
    for n in list(out):
        out["boundary_" + n] = case.boundary_values(m, out[n]).reshape(np.shape(out[n])[:-1] + (B,))
    w = m.weight
    ru = rho[None] * U
    rf = w * (ru[:, m.owner] - ru[:, m.neighbour]) + ru[:, m.neighbour]
    out["phi"] = (rf * np.asarray(m.sf).T).sum(axis=0)
    bsf, _, _, _, bfc = m.boundary_arrays()
    out["boundary_phi"] = ((out["boundary_rho"][None] * out["boundary_U"]) * np.asarray(bsf).T).sum(axis=0)
    # walls: no flux through them
    off = 0
    for p in m.patches:
        if p.kind == "wall":
            out["boundary_phi"][off:off + p.size] = 0.0
        off += p.slots
    out["nut"] = nut_of(0.09, k, eps)
    return out


def production_error(m, st, G, divU, ptype_U, ptype_rho):
    """(|G - G_longdouble| / (nut |g|^2), |divU - divU_longdouble| / (sum |phi_f / rho_f| / V)) per cell"""
    gL = grad_u(m, ptype_U, st["U"], st["boundary_U"], LD)
    GL = production(gL, st["nut"], LD)
    tp = Topo(m)
    dL, sc = div_u(tp, ptype_rho, st["phi"], st["boundary_phi"], st["rho"], st["boundary_rho"], LD)
    gs = np.asarray(st["nut"], LD) * (gL * gL).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        eG = np.where(gs > 0, np.abs(np.asarray(G, LD) - GL) / np.where(gs > 0, gs, 1), 0)
        eD = np.where(sc > 0, np.abs(np.asarray(divU, LD) - dL) / np.where(sc > 0, sc, 1), 0)
    return np.asarray(eG, np.float64), np.asarray(eD, np.float64)


def measure():
    out = {}
    for name in MESHES:
        m = get_mesh(name)
        st = ras_state(m)
        ptU, ptR = m.patch_types(ZG), m.patch_types(CALC)
        G = production(grad_u(m, ptU, st["U"], st["boundary_U"]), st["nut"])
        dv, _ = div_u(Topo(m), ptR, st["phi"], st["boundary_phi"], st["rho"], st["boundary_rho"])
        eG, eD = production_error(m, st, G, dv, ptU, ptR)
        out[name] = {"G": float(eG.max()), "divU": float(eD.max())}
    return out


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def gpu_bound(bounds, mesh_name, what):
    """4x the fp64 restatement's measured maximum on that mesh, floored at 1e-13 (les_nut_bounds.json's rule)"""
    return max(4.0 * bounds["meshes"][mesh_name][what], 1e-13)


# ------------------------------------------------------------------------------------------------ oracle
class RasOracle(LesOracle):
    """The sequential oracle with the effective fields of a k-epsilon nut injected as LesOracle injects them. ras:
    coefficient overrides; k, epsilon and their boundary values; k_ptypes / eps_ptypes / nut_ptypes. time_step restates
    Oracle.time_step and ends with correct() on the rho the last pressure corrector leaves (its correctPsipRho and
    rhoEqn), before rho = psi p."""

    def __init__(self, mesh, table, state, ptypes, inert, rdt, ras, k, epsilon, bk, beps, schemes=None, k_ptypes=None,
                 eps_ptypes=None, nut_ptypes=None, boundary_nut=None):
        self.q = dict(DEFAULTS, **ras)
        self._ras_ready = False
        super().__init__(mesh, table, state, ptypes, inert, rdt, {"model": 1, "Prt": self.q["Prt"], "Sct": self.q["Sct"]},
                         np.ones(mesh.n_cells), schemes=schemes, nut_ptypes=nut_ptypes, boundary_nut=boundary_nut)
        zg = mesh.patch_types(ZG)
        self.k_pt = zg if k_ptypes is None else k_ptypes
        self.eps_pt = zg if eps_ptypes is None else eps_ptypes
        self.nut_pt = ptypes["calculated"] if nut_ptypes is None else nut_ptypes
        self._i("ptype_k", self.k_pt); self._i("ptype_epsilon", self.eps_pt)
        for n, v in (("k", k), ("epsilon", epsilon), ("boundary_k", bk), ("boundary_epsilon", beps)):
            self._d(n, v)
        self.stored_bnut = self.arr["boundary_nut"].copy()
        self.tp = Topo(mesh)
        self._ras_ready = True
        self.correct_nut()

    def correct_nut(self):
        a = self.arr
        a["nut"][...] = nut_of(self.q["Cmu"], a["k"], a["epsilon"])
        a["boundary_nut"][...] = boundary_nut(self.m, self.nut_pt, self.q["Cmu"], a["nut"], a["boundary_k"],
                                              a["boundary_epsilon"], self.stored_bnut)

    def _equation(self, keq, G, dv):
        a, q, m = self.arr, self.q, self.m
        nm = "k" if keq else "epsilon"
        pt = self.k_pt if keq else self.eps_pt
        Su, Sp = sources(keq, q, G, dv, a["rho"], a["k"], a["epsilon"])
        sig = q["sigmak"] if keq else q["sigmaEps"]
        D = diffusivity(a["rho"], a["nut"], a["mu"], sig)
        bD = diffusivity(a["boundary_rho"], a["boundary_nut"], a["boundary_mu"], sig)
        o = scalar_assemble(self.tp, pt, a[nm], a["boundary_" + nm], a["rho"], a["rho_old"], a["phi"], a["boundary_phi"],
                            D, bD, Su, Sp, self.rdt)
        self.ptypes[nm] = pt
        a[nm][...] = self.solve_ldu(o["lower"], o["upper"], o["diag"], o["source"], o["internal_coeffs"],
                                    o["boundary_coeffs"], nm)
        self.correct_bc(nm, nm, 1)
        lo = q["kMin"] if keq else q["epsilonMin"]
        a[nm][...], a["boundary_" + nm][...] = bound(self.tp, pt, a[nm], a["boundary_" + nm], lo)
        return o

    def turbulence_correct(self):
        """kEpsilon::correct() on the arrays as they stand (upwind convection, orthogonal laplacian)"""
        if not self._ras_ready:
            return
        a = self.arr
        G = production(self.grad_u(), a["nut"])
        dv, _ = div_u(self.tp, self.ptypes["rho"], a["phi"], a["boundary_phi"], a["rho"], a["boundary_rho"])
        self.G, self.divU = G, dv
        self._equation(0, G, dv)
        self._equation(1, G, dv)
        self.correct_nut()

    def time_step(self, n_corr=2):
        m = self.m
        C_, F, B, S = m.n_cells, m.n_faces, m.n_boundary_slots, self.S
        a = self.arr
        for n, o in (("rho_old", "rho"), ("boundary_rho_old", "boundary_rho"), ("phi_old", "phi"),
                     ("boundary_phi_old", "boundary_phi"), ("U_old", "U"), ("boundary_U_old", "boundary_U"),
                     ("K_old", "K"), ("p_old", "p"), ("boundary_p_old", "boundary_p")):
            a[n][...] = a[o]
        self.rho_eqn()
        u = self.u_assemble()
        for k in range(3):
            a["U"][k] = self.solve_ldu(u["lower"], u["upper"], u["diag"], u["source_solve"][k * C_:(k + 1) * C_],
                                       u["internal_coeffs"][k * B:(k + 1) * B], u["boundary_coeffs"][k * B:(k + 1) * B], "U")
        self.correct_bc("U", "U", 3)
        Ux, Uy, Uz = a["U"]
        a["K"][...] = 0.5 * (Ux * Ux + Uy * Uy + Uz * Uz)
        bx, by, bz = a["boundary_U"]
        a["boundary_K"][...] = 0.5 * (bx * bx + by * by + bz * bz)
        self.y_prep()
        y = self.y_assemble()
        for s in range(S):
            if s == self.inert:
                continue
            a["Y"][s] = self.solve_ldu(y["lower"][s * F:(s + 1) * F], y["upper"][s * F:(s + 1) * F],
                                       y["diag"][s * C_:(s + 1) * C_], y["source"][s * C_:(s + 1) * C_],
                                       y["internal_coeffs"][s * B:(s + 1) * B], y["boundary_coeffs"][s * B:(s + 1) * B], "Y")
        self.y_inert()
        self.energy_gradient()
        self.correct_bc("he", "he", 1)
        e = self.e_assemble()
        a["he"][...] = self.solve_ldu(e["lower"], e["upper"], e["diag"], e["source"], e["internal_coeffs"],
                                      e["boundary_coeffs"], "he")
        self.correct_bc("he", "he", 1)
        self.thermo_correct(False)
        for _ in range(n_corr):
            a["rho"][...] = a["p"] * a["psi"]; a["boundary_rho"][...] = a["boundary_p"] * a["boundary_psi"]
            a["psip0"][...] = a["psi"] * a["p"]; a["boundary_psip0"][...] = a["boundary_psi"] * a["boundary_p"]
            self.u_hbya()
            pq = self.p_assemble()
            a["p"][...] = self.solve_ldu(pq["lower"], pq["upper"], pq["diag"], pq["source"], pq["internal_coeffs"],
                                         pq["boundary_coeffs"], "p")
            self.p_post()
            a["rho"][...] = a["rho"] + (a["psi"] * a["p"] - a["psip0"])
            a["boundary_rho"][...] = a["boundary_rho"] + (a["boundary_psi"] * a["boundary_p"] - a["boundary_psip0"])
            self.rho_eqn()
        self.turbulence_correct()                 # dfLowMachFoam.C:508, on the corrector's rho
        a["rho"][...] = a["p"] * a["psi"]
        a["boundary_rho"][...] = a["boundary_p"] * a["boundary_psi"]


if __name__ == "__main__":
    if "--measure" not in sys.argv:
        sys.exit("usage: ras_reference.py --measure")
    doc = {"about": "max over cells of |G_fp64 - G_longdouble| / (nut |g|^2) and |divU_fp64 - divU_longdouble| / (sum_f "
                    "|phi_f / rho_f| / V) of the NumPy restatement of the k-epsilon production terms on ras_state of every "
                    "test mesh (tests/ras_reference.py); written by tests/ras_reference.py --measure",
           "meshes": measure()}
    with open(BOUNDS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, v in doc["meshes"].items():
        print(name, {c: f"{x:.2e}" for c, x in v.items()})
