"""Reference of the reference's two own LES closures, Sigma (les.model = 4) and dynamicSmagorinsky (les.model = 5;
include/dfmi.h dfmi_turbulence_correct), and the oracles of the turbulent equations with them.

Sigma.

With g[3 i + j] = d_i U_j, its singular values s1 >= s2 >= s3 >= 0 and the filter width delta:

    Dsg = s3 (s1 - s2)(s2 - s3) / (s1^2 + 1e-300),   nut = (Csg delta)^2 Dsg

restated in NumPy, vectorised over n states and parameterised by dtype (fp64, and long double: x87 extended, 64-bit
mantissa). The singular values are the column norms of g after `sweeps` cyclic sweeps of one-sided (Hestenes) Jacobi
rotations over the column pairs (0,1), (0,2), (1,2), operation for operation what the kernel does (fv_kernels.hip
sigma_rotate / sigma_nut): a = p.p, b = q.q, c = p.q; c == 0 is the identity; else z = (b - a) / (2c),
t = sign(z) / (|z| + sqrt(1 + z^2)), cs = 1 / sqrt(1 + t^2), sn = cs t, p' = cs p - sn q, q' = sn p + cs q.
s2 is the true middle value (the reference's loop keeps whichever value its unsorted SVD returns last: DESIGN 9).

The truth every error is measured against is the long-double restatement with TRUTH_SWEEPS = 8 sweeps; on the CPU the
fp64 restatement is also held to numpy.linalg.svd (tests/test_sgs_cpu.py).

State classes: les_reference's (random tensors; the linear fields zero, rotation, shear, dilatation, general) and the
near-degenerate ones, g = 1e3 R1 diag(s) R2^T with random rotations R1, R2 and
    s12   (1, 1 - 1e-9, 0.5)      s23   (1, 0.5 + 1e-9, 0.5)      s12eq (1, 1, 0.3)
    s3e-9 (1, 0.6, 1e-9)          s3zero (1, 0.6, 0)              s3e-5 (1, 0.4, 1e-5)
-- two singular values meeting, or s3 small: the model's own zeros (2-D flow, shear, rotation, axisymmetric strain),
where the closed form from the invariants of g^T g loses seven digits.

`python tests/sgs_reference.py --measure` writes tests/golden/sgs_bounds.json:
    "sigma":  per class, max |nut_fp64 - nut_truth| / (Csg^2 delta^2 |g|_F) at SWEEPS sweeps
    "sweeps": per class and sweep count 1..6, max |Dsg_fp64(sweeps) - Dsg_truth| / s1
The second table picks the kernel's sweep count: the first count at which every class is at rounding level (< 1e-15),
plus one. The GPU tolerance is derived from the first (gpu_bound), never from a kernel's output.

dynamicSmagorinsky. dynamic_model restates the header's statement with per-cell sums in the sequential face order
(les_filter: the test filter; gauss_grad: the Gauss gradient for states built without a device), in fp64 and in long
double: S = dev(symm(g)), LL = dev(F(U U) - F(U) F(U)), MM = delta^2 (F(|S| S) - 4 |F(S)| F(S)), LM = F(LL && MM),
MM = max(F(MM && MM), 1e-300), Cs = 0.5 LM / MM, nut = max(Cs delta^2 |S|, -mu / rho). dynamic_scales is what the errors
of les_LM and les_MM are measured against (its docstring says why |U|^2 over the stencil enters); --measure adds
    "dynamic": max |x_fp64 - x_longdouble| / scale of LM and MM on dynamic_case's periodic and walled boxes
and gpu_bound_dynamic derives the GPU tolerance from it. DynamicOracle is LesOracle with this nut.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

import les_reference as L

LD = np.longdouble
BOUNDS_PATH = os.path.join(L.GOLDEN, "sgs_bounds.json")
SIGMA = 4
CSG = 1.5
SWEEPS = 5            # the kernel's SIGMA_SWEEPS
TRUTH_SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (1, 2))
DEGENERATE = {"s12": (1.0, 1.0 - 1e-9, 0.5), "s23": (1.0, 0.5 + 1e-9, 0.5), "s12eq": (1.0, 1.0, 0.3),
              "s3e-9": (1.0, 0.6, 1e-9), "s3zero": (1.0, 0.6, 0.0), "s3e-5": (1.0, 0.4, 1e-5)}
CLASSES = L.CLASSES + tuple(DEGENERATE)


# ------------------------------------------------------------------------------------------------ Sigma
def singular_values(g, dtype=np.float64, sweeps: int = SWEEPS):
    """(s1, s2, s3) [n] each, descending, of g [9, n] by one-sided Jacobi on the columns, every operation in `dtype`"""
    T = dtype
    g = np.asarray(g, dtype=T)
    col = [[g[3 * i + j].copy() for i in range(3)] for j in range(3)]      # col[j][i] = g[i][j]
    one, two = T(1.0), T(2.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                P, Q = col[p], col[q]
                a = P[0] * P[0] + P[1] * P[1] + P[2] * P[2]
                b = Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2]
                c = P[0] * Q[0] + P[1] * Q[1] + P[2] * Q[2]
                rot = c != 0
                z = (b - a) / (two * np.where(rot, c, one))
                t = np.copysign(one, z) / (np.abs(z) + np.sqrt(one + z * z))
                cs = one / np.sqrt(one + t * t)
                sn = cs * t
                for i in range(3):
                    pi, qi = P[i], Q[i]
                    P[i] = np.where(rot, cs * pi - sn * qi, pi)
                    Q[i] = np.where(rot, sn * pi + cs * qi, qi)
        n = [np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) for c in col]
    s1 = np.maximum(n[0], np.maximum(n[1], n[2]))
    s3 = np.minimum(n[0], np.minimum(n[1], n[2]))
    s2 = np.maximum(np.minimum(n[0], n[1]), np.minimum(np.maximum(n[0], n[1]), n[2]))
    return s1, s2, s3


def dsg_from_grad(g, dtype=np.float64, sweeps: int = SWEEPS):
    s1, s2, s3 = singular_values(g, dtype, sweeps)
    return s3 * (s1 - s2) * (s2 - s3) / (s1 * s1 + dtype(1e-300))


def nut_from_grad(g, delta, Csg: float = CSG, dtype=np.float64, sweeps: int = SWEEPS):
    """nut [n] from g [9, n] and delta [n], in the kernel's operation order"""
    cd = dtype(Csg) * np.asarray(delta, dtype=dtype)
    return cd * cd * dsg_from_grad(g, dtype, sweeps)


def nut_error(nut, g, delta, Csg: float = CSG):
    """|nut - nut_truth(g)| / (Csg^2 delta^2 |g|_F) per cell; where g = 0 the truth is exactly 0 and so must nut be
    (error 0, else inf)"""
    ref = nut_from_grad(g, delta, Csg, LD, TRUTH_SWEEPS)
    g = np.asarray(g, dtype=LD)
    scale = LD(Csg) ** 2 * np.asarray(delta, dtype=LD) ** 2 * np.sqrt((g * g).sum(axis=0))
    diff = np.abs(np.asarray(nut, dtype=LD) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(scale > 0, diff / np.where(scale > 0, scale, 1), np.where(diff == 0, LD(0), LD(np.inf)))
    return np.asarray(e, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ state classes
def rotations(n: int, rng):
    """n proper rotations [n, 3, 3] (QR of Gaussian matrices, the determinant fixed)"""
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def degenerate_tensors(cls: str, n: int, seed: int = 5, scale: float = 1e3):
    """G [n, 3, 3] = scale R1 diag(s) R2^T of a near-degenerate class"""
    rng = np.random.default_rng(seed + 100 * list(DEGENERATE).index(cls))
    r1, r2 = rotations(n, rng), rotations(n, rng)
    return scale * np.einsum("nik,k,njk->nij", r1, np.asarray(DEGENERATE[cls]), r2)


def class_states(cls: str, n: int = 4096, seed: int = 11):
    """(g [9, n], delta [n]) of a state class (module docstring)"""
    if cls in L.CLASSES:
        return L.class_states(cls, n, seed)
    rng = np.random.default_rng(seed + CLASSES.index(cls))
    delta = 10.0 ** rng.uniform(-5.0, -2.5, n)
    return degenerate_tensors(cls, n, seed).reshape(n, 9).T.copy(), delta


def measure():
    """{"sigma": {class: max nut error of the fp64 restatement}, "sweeps": {class: [max Dsg error / s1 at 1..6 sweeps]}}"""
    out = {"sigma": {}, "sweeps": {}}
    for cls in CLASSES:
        g, delta = class_states(cls)
        out["sigma"][cls] = float(nut_error(nut_from_grad(g, delta), g, delta).max())
        truth = dsg_from_grad(g, LD, TRUTH_SWEEPS)
        s1 = singular_values(g, LD, TRUTH_SWEEPS)[0]
        per = []
        for k in range(1, 7):
            d = np.abs(np.asarray(dsg_from_grad(g, np.float64, k), dtype=LD) - truth)
            with np.errstate(invalid="ignore", divide="ignore"):
                e = np.where(s1 > 0, d / np.where(s1 > 0, s1, 1), d)
            per.append(float(e.max()))
        out["sweeps"][cls] = per
    return out


def sweeps_needed(table: dict, level: float = 1e-15) -> int:
    """the first sweep count at which every class of the "sweeps" table is below `level`"""
    for k in range(6):
        if all(v[k] < level for v in table.values()):
            return k + 1
    raise ValueError("no sweep count up to 6 reaches rounding level")


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def gpu_bound(bounds, cls: str) -> float:
    """4x the fp64 restatement's measured maximum for that class, floored at 1e-13 of Csg^2 delta^2 |g|_F (DESIGN 3:
    the factor covers the device's square-root and division sequences, one more rounding per term each)"""
    return max(4.0 * bounds["sigma"][cls], 1e-13)


# ------------------------------------------------------------------------------------------------ dynamicSmagorinsky
DYNAMIC = 5


def _slot_info(m, ptypes_U):
    """per boundary slot: (cell, |Sf|, n [B, 3], deltaCoeffs, weight, partner cell or -1, U's patch type); one rank
    (no processor patches), slots in patch order"""
    from dfmi.mesh import CYCLIC
    bsf, bmag, bdc, bw, bfc = m.boundary_arrays()
    partner = np.full(m.n_boundary_slots, -1, dtype=np.int64)
    ty = np.repeat(np.asarray(ptypes_U), [p.slots for p in m.patches])
    off = [0]
    for p in m.patches:
        off.append(off[-1] + p.slots)
    for i, p in enumerate(m.patches):
        assert p.kind in ("wall", "cyclic", "empty"), p.kind
        if p.kind == "cyclic":
            partner[off[i]:off[i + 1]] = m.patches[p.neighbour_patch].face_cells
    assert ((partner >= 0) == (ty == CYCLIC)).all()
    return bfc.astype(np.int64), bmag, bsf / np.maximum(bmag, 1e-300)[:, None], bdc, bw, partner, ty


def les_filter(m, slots, x, bx, dtype=np.float64, own_on_walls=False):
    """F(x)_c = sum_f |Sf| x_f / sum_f |Sf| of x [N, C] with boundary values bx [N, B] (read on non-coupled slots;
    own_on_walls: the cell's own value there), every operation in `dtype`, accumulated per cell in the sequential face
    order: the faces the cell is the neighbour of, ascending, then the faces it owns, then its slots"""
    T = dtype
    bfc, bmag, _, _, bw, partner, _ = slots
    x = np.asarray(x, dtype=T)
    w, a = np.asarray(m.weight, dtype=T), np.asarray(m.mag_sf, dtype=T)
    own, nei = np.asarray(m.owner, dtype=np.int64), np.asarray(m.neighbour, dtype=np.int64)
    s, A = np.zeros(x.shape, dtype=T), np.zeros(x.shape[1], dtype=T)
    xf = w * (x[:, own] - x[:, nei]) + x[:, nei]                      # interp_f(w, owner, neighbour), the same for both
    for side in (nei, own):
        for f in range(own.size):
            c = side[f]
            s[:, c] += a[f] * xf[:, f]
            A[c] += a[f]
    bx = None if bx is None else np.asarray(bx, dtype=T)
    for b in range(bfc.size):
        c, ab = bfc[b], T(bmag[b])
        if partner[b] >= 0:
            xb = T(bw[b]) * x[:, c] + (T(1.0) - T(bw[b])) * x[:, partner[b]]
        else:
            xb = x[:, c] if own_on_walls else bx[:, b]
        s[:, c] += ab * xb
        A[c] += ab
    return s / A


def _dev_symm(g, T):
    t3 = (T(1.0) / T(3.0)) * (g[0] + g[4] + g[8])
    h = T(0.5)
    return np.stack([g[0] - t3, h * (g[1] + g[3]), h * (g[2] + g[6]), g[4] - t3, h * (g[5] + g[7]), g[8] - t3])


def _dd(a, b):
    return (a[0] * b[0] + a[3] * b[3] + a[5] * b[5]) + 2 * (a[1] * b[1] + a[2] * b[2] + a[4] * b[4])


def _point(U, S):
    ms = np.sqrt(_dd(S, S))
    return np.concatenate([U, np.stack([U[0] * U[0], U[0] * U[1], U[0] * U[2], U[1] * U[1], U[1] * U[2], U[2] * U[2]]),
                           S, ms[None] * S])


def dynamic_model(m, ptypes_U, U, bU, g, delta, mu, rho, dtype=np.float64):
    """the dynamicSmagorinsky model as include/dfmi.h states it, every operation in `dtype` and in the kernels' order
    (fv_kernels.hip k_dyn_strain / k_dyn_filter / k_dyn_nut): {"S" [6, C], "LM", "MM", "Cs", "nut" [C]} from U [3, C],
    boundary_U [3, B], g [9, C] (the Gauss gradient of U) and delta, mu, rho [C]"""
    from dfmi.mesh import FIXED_VALUE, INLET_OUTLET, WAVE_TRANSMISSIVE
    T = dtype
    slots = _slot_info(m, ptypes_U)
    bfc, _, nv, bdc, _, partner, ty = slots
    U, bU, g = np.asarray(U, dtype=T), np.asarray(bU, dtype=T), np.asarray(g, dtype=T)
    d = np.asarray(delta, dtype=T)
    S = _dev_symm(g, T)
    # boundary gradient on non-coupled slots: g_c + n (snGrad - n . g_c), snGrad by U's patch type
    nv, bdc = np.asarray(nv, dtype=T), np.asarray(bdc, dtype=T)
    gc = g[:, bfc]
    fixed = np.isin(ty, (FIXED_VALUE, INLET_OUTLET, WAVE_TRANSMISSIVE))
    bg = np.zeros((9, bfc.size), dtype=T)
    for j in range(3):
        sn = np.where(fixed, bdc * (bU[j] - U[j, bfc]), T(0.0))
        corr = sn - (nv[:, 0] * gc[j] + nv[:, 1] * gc[3 + j] + nv[:, 2] * gc[6 + j])
        for i in range(3):
            bg[3 * i + j] = gc[3 * i + j] + nv[:, i] * corr
    bS = _dev_symm(bg, T)
    F = les_filter(m, slots, _point(U, S), _point(bU, bS), T)
    LL = np.stack([F[3] - F[0] * F[0], F[4] - F[0] * F[1], F[5] - F[0] * F[2], F[6] - F[1] * F[1], F[7] - F[1] * F[2],
                   F[8] - F[2] * F[2]])
    t3 = (T(1.0) / T(3.0)) * (LL[0] + LL[3] + LL[5])
    LL[0] -= t3; LL[3] -= t3; LL[5] -= t3
    mfs = np.sqrt(_dd(F[9:15], F[9:15]))
    d2 = d * d
    MMt = d2[None] * (F[15:21] - T(4.0) * mfs[None] * F[9:15])
    sc = np.stack([_dd(LL, MMt), _dd(MMt, MMt)])
    F2 = les_filter(m, slots, sc, None, T, own_on_walls=True)
    MM = np.maximum(F2[1], T(1e-300))
    Cs = T(0.5) * F2[0] / MM
    nut = np.maximum(Cs * d2 * np.sqrt(_dd(S, S)), -np.asarray(mu, dtype=T) / np.asarray(rho, dtype=T))
    return {"S": S, "bS": bS, "LM": F2[0], "MM": MM, "Cs": Cs, "nut": nut}


def ring_max(m, slots, x, bx=None):
    """max of x >= 0 over each cell, its face neighbours and its slots (coupled: the partner cell; else bx, if given)"""
    bfc, _, _, _, _, partner, _ = slots
    out = np.array(x, dtype=np.float64)
    np.maximum.at(out, m.owner, x[m.neighbour])
    np.maximum.at(out, m.neighbour, x[m.owner])
    cp = partner >= 0
    np.maximum.at(out, bfc[cp], x[partner[cp]])
    if bx is not None:
        np.maximum.at(out, bfc[~cp], np.asarray(bx, dtype=np.float64)[~cp])
    return out


def dynamic_scales(m, ptypes_U, U, bU, S, bS, delta):
    """(scale of LM, scale of MM) per cell, what the errors of les_LM and les_MM are measured against. LL is a
    difference of filtered O(|U|^2) terms, so its rounding error is eps u2 with u2 the largest |U|^2 of the filter's
    stencil, however small LL itself is; MM's is eps m with m = 5 delta^2 s^2, s the largest |S| of the stencil (the two
    terms |S| S and 4 |F(S)| F(S)). LL && MM then errs by eps u2 m, MM && MM by eps m^2, and the second filter carries
    the largest of those over its own stencil."""
    slots = _slot_info(m, ptypes_U)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    U, bU, S, bS, d = f64(U), f64(bU), f64(S), f64(bS), f64(delta)
    u2 = ring_max(m, slots, (U * U).sum(axis=0), (bU * bU).sum(axis=0))
    s = ring_max(m, slots, np.sqrt(_dd(S, S)), np.sqrt(_dd(bS, bS)))
    mm = 5.0 * d * d * s * s
    return ring_max(m, slots, u2 * mm), ring_max(m, slots, mm * mm)


def dynamic_errors(got_LM, got_MM, truth, scales):
    """(max |LM - truth| / scale, max |MM - truth| / scale)"""
    e1 = np.abs(np.asarray(got_LM, dtype=LD) - truth["LM"]) / scales[0]
    e2 = np.abs(np.asarray(got_MM, dtype=LD) - truth["MM"]) / scales[1]
    return float(e1.max()), float(e2.max())


def dynamic_case(kind: str, n=(6, 5, 4), seed=3):
    """a NumPy-only state for the measurement: (mesh, U's patch types, U, boundary_U, g, delta, mu, rho). periodic:
    every patch cyclic; walls: fixedValue U on all six sides with boundary values off the cell values. U is a
    Taylor-Green field of 4 m/s with 30 per cent noise on a mean flow of 40 m/s, so that LL cancels three digits."""
    from dfmi.mesh import FIXED_VALUE, hex_box
    from dfmi import case
    rng = np.random.default_rng(seed)
    Lx = 2 * np.pi * 1e-3
    m = hex_box(*n, lengths=(Lx,) * 3, periodic=(kind == "periodic",) * 3, gradings=(1.0, 1.3, 1.0))
    x = m.cell_centres / 1e-3
    U = 4.0 * np.stack([np.sin(x[:, 0]) * np.cos(x[:, 1]) * np.cos(x[:, 2]), -np.cos(x[:, 0]) * np.sin(x[:, 1]) * np.cos(x[:, 2]),
                        0 * x[:, 0]]) + 1.2 * rng.standard_normal((3, m.n_cells)) + np.array([40.0, -25.0, 10.0])[:, None]
    pt = case.default_patch_types(m)["U"] if kind == "periodic" else m.patch_types(FIXED_VALUE)
    slots = _slot_info(m, pt)
    bfc = slots[0]
    bU = U[:, bfc] + 0.5 * rng.standard_normal((3, bfc.size))
    delta = np.cbrt(m.volume)
    mu = np.full(m.n_cells, 1.8e-5) * (1 + 0.1 * rng.standard_normal(m.n_cells))
    rho = 1.1 * (1 + 0.1 * rng.uniform(-1, 1, m.n_cells))
    return m, pt, U, bU, delta, mu, rho


def gauss_grad(m, ptypes_U, U, bU, dtype=np.float64):
    """g [9, C], g[3 i + j] = d_i U_j: the Gauss linear gradient with the sums in the sequential face order"""
    T = dtype
    slots = _slot_info(m, ptypes_U)
    bfc, bmag, nv, _, bw, partner, _ = slots
    U, bU = np.asarray(U, dtype=T), np.asarray(bU, dtype=T)
    w, sf = np.asarray(m.weight, dtype=T), np.asarray(m.sf, dtype=T)
    own, nei = np.asarray(m.owner, dtype=np.int64), np.asarray(m.neighbour, dtype=np.int64)
    uf = w * (U[:, own] - U[:, nei]) + U[:, nei]
    s = np.zeros((9, m.n_cells), dtype=T)
    for side, sign in ((nei, T(-1.0)), (own, T(1.0))):
        for f in range(own.size):
            for i in range(3):
                s[3 * i:3 * i + 3, side[f]] += sign * (sf[f, i] * uf[:, f])
    bsf = np.asarray(m.boundary_arrays()[0], dtype=T)
    for b in range(bfc.size):
        c = bfc[b]
        ub = T(bw[b]) * U[:, c] + (T(1.0) - T(bw[b])) * U[:, partner[b]] if partner[b] >= 0 else bU[:, b]
        for i in range(3):
            s[3 * i:3 * i + 3, c] += bsf[b, i] * ub
    return s / np.asarray(m.volume, dtype=T)


def measure_dynamic():
    """{"LM": {kind: max error of the fp64 restatement against long double}, "MM": {...}} on dynamic_case's states"""
    out = {"LM": {}, "MM": {}}
    for kind in ("periodic", "walls"):
        m, pt, U, bU, delta, mu, rho = dynamic_case(kind)
        g = gauss_grad(m, pt, U, bU)                                   # one fp64 gradient for both, as on the device
        a = dynamic_model(m, pt, U, bU, g, delta, mu, rho)
        t = dynamic_model(m, pt, U, bU, g, delta, mu, rho, LD)
        e = dynamic_errors(a["LM"], a["MM"], t, dynamic_scales(m, pt, U, bU, a["S"], a["bS"], delta))
        out["LM"][kind], out["MM"][kind] = e
    return out


def gpu_bound_dynamic(bounds, name: str) -> float:
    """4x the fp64 restatement's measured maximum of les_LM / les_MM over the measured states, floored at 1e-13 of
    dynamic_scales"""
    return max(4.0 * max(bounds["dynamic"][name].values()), 1e-13)


class DynamicOracle(L.LesOracle):
    """LesOracle with the dynamicSmagorinsky nut: les = {"model": 5, "Prt", "Sct"}; mu and rho as the oracle holds
    them at the call"""

    def turbulence_correct(self):
        a = self.arr
        r = dynamic_model(self.m, self.iarr["ptype_U"], a["U"], a["boundary_U"], self.grad_u(), self.delta, a["mu"], a["rho"])
        self.last = r
        a["nut"][...] = r["nut"]
        self.correct_bc("nut", "nut", 1)


# ------------------------------------------------------------------------------------------------ oracle
class SigmaOracle(L.LesOracle):
    """LesOracle with the Sigma nut: les = {"model": 4, "Csg", "Prt", "Sct"}"""

    def turbulence_correct(self):
        self.arr["nut"][...] = nut_from_grad(self.grad_u(), self.delta, self.les.get("Csg", CSG))
        self.correct_bc("nut", "nut", 1)


if __name__ == "__main__":
    if "--measure" not in sys.argv:
        sys.exit("usage: sgs_reference.py --measure")
    doc = {"about": "the NumPy fp64 restatement of the Sigma eddy viscosity (tests/sgs_reference.py) against the "
                    "long-double one at 8 sweeps, 4096 states per class. sigma: max |nut_fp64 - nut_truth| / (Csg^2 "
                    "delta^2 |g|_F) at 5 sweeps; sweeps: max |Dsg_fp64 - Dsg_truth| / s1 at 1..6 sweeps; written by "
                    "python tests/sgs_reference.py --measure",
           **measure()}
    doc["dynamic"] = measure_dynamic()
    doc["about_dynamic"] = ("dynamic: max |x_fp64 - x_longdouble| / scale of les_LM and les_MM of the dynamicSmagorinsky "
                            "restatement (dynamic_model, dynamic_scales) on dynamic_case's periodic and walled 6 x 5 x 4 boxes")
    doc["sweeps_needed"] = sweeps_needed(doc["sweeps"])
    with open(BOUNDS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("sigma", {c: f"{x:.2e}" for c, x in doc["sigma"].items()})
    for c, v in doc["sweeps"].items():
        print(f"{c:12s}", " ".join(f"{x:.1e}" for x in v))
    print("sweeps needed", doc["sweeps_needed"])
    print("dynamic", doc["dynamic"])
