"""NumPy restatement of the non-orthogonal laplacian correction, in fp64 and in long double.

What the library adds under `laplacian corrected` (csrc/fv_kernels.hip k_nonorth_corr), restated with array operations:

  geometry      Mesh.nonorth_geometry: nonOrthDeltaCoeffs = 1 / max(n.d, 0.05 |d|), k = n - d nonOrthDeltaCoeffs
  gradient      Gauss linear, cell-centred: sum over faces of Sf phi_f (coupled slots interpolate, others read the
                boundary value), / V
  correction    corr_f = (k_x g_x + k_y g_y) + k_z g_z with g = interp_f(w, g_P, g_N); flux_f = (gamma_f |Sf|) corr_f;
                per cell the sum of the outward fluxes of its faces and coupled slots
  pressure loop assemble once; per pass grad(p), source = base + correction, exact solve (SciPy); phi = phiHbyA +
                pEqn.flux() with the last pass's face flux correction

The kernel sums a cell's faces in the sequential face order and these restatements in face-index order, so the two
agree to rounding, not bitwise: the GPU tests bound the difference by gpu_bound() -- 4x this fp64 restatement's own
measured error against the long-double one (tests/golden/nonorth_bounds.json, written by `--measure`), floored at
1e-13, relative to the per-cell scale sum_f |gamma_f| |Sf| |k| |grad phi|_f.
"""
import copy
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUNDS_PATH = os.path.join(GOLDEN, "nonorth_bounds.json")
for _p in (os.path.join(os.path.dirname(HERE), "deepflame-dev_amd"), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

L0 = 2 * np.pi * 1e-3
COUPLED_KINDS = ("cyclic", "processor", "processorCyclic")
EMPTY = 3
LD = np.longdouble
MESHES = ("sheared-walls", "sheared-315", "sheared-periodic", "distorted", "refined", "prisms", "hexprism")

_cache = {}


# ------------------------------------------------------------------------------------------------ meshes
def sheared_mesh(nx, ny, nz, periodic=(False, False, False)):
    """hex_polymesh points mapped by x' = x + 0.7 y + 0.4 z, y' = y + 0.5 z, written and read back: an affine image
    of a uniform grid (no skewness, weights of 1/2), non-orthogonal on every face family"""
    from dfmi.polymesh import hex_polymesh, read_polymesh, write_polymesh
    P, faces, own, nei, bnd = hex_polymesh(nx, ny, nz, lengths=(L0,) * 3, periodic=periodic)
    Q = P.copy()
    Q[:, 0] = P[:, 0] + 0.7 * P[:, 1] + 0.4 * P[:, 2]
    Q[:, 1] = P[:, 1] + 0.5 * P[:, 2]
    from dfmi.polymesh import _read_faces, _read_points, face_centres_areas
    with tempfile.TemporaryDirectory() as d:
        write_polymesh(d, Q, faces, own, nei, bnd)
        m = read_polymesh(d)
        # the centres of the boundary faces, from the points as they were read back (one per boundary slot on a
        # mesh without processor patches): where a fixed-value condition samples an analytic field
        Cf, _ = face_centres_areas(_read_points(os.path.join(d, "points")), _read_faces(os.path.join(d, "faces")))
    m.boundary_face_centres = Cf[m.n_faces:]
    return m


def get_mesh(name):
    """the test meshes by name (built once per process; read-only)"""
    if name not in _cache:
        if name == "sheared-walls":
            m = sheared_mesh(6, 5, 4)
        elif name == "sheared-315":
            m = sheared_mesh(9, 7, 5)
        elif name == "sheared-periodic":
            m = sheared_mesh(6, 6, 4, periodic=(True, True, False))
        elif name == "sheared-periodic-xyz":   # the exactness case (exactness_residual)
            m = sheared_mesh(6, 6, 4, periodic=(True, True, True))
        elif name == "distorted":
            from dfmi.polymesh import hex_polymesh, read_polymesh, write_polymesh
            P, faces, own, nei, bnd = hex_polymesh(6, 5, 4, lengths=(L0,) * 3, periodic=(False,) * 3)
            h = L0 / np.array([6, 5, 4])
            inner = np.all((P > 1e-12) & (P < L0 - 1e-12), axis=1)
            P = P.copy()
            P[inner] += 0.15 * h * np.random.default_rng(5).uniform(-1, 1, (inner.sum(), 3))   # test_gpu_parity's box
            with tempfile.TemporaryDirectory() as d:
                write_polymesh(d, P, faces, own, nei, bnd)
                m = read_polymesh(d)
        else:
            import unstructured_meshes as um
            m = um.get(name)
        _cache[name] = m
    return _cache[name]


def nonorth_mesh(m):
    """a copy of the Mesh whose delta_coeffs (internal faces and coupled patches) are the non-orthogonal ones: what the
    unchanged oracle assembles is then the implicit part of `uncorrected` / `corrected`"""
    dc, _, bdc, _ = m.nonorth_geometry()
    m2 = copy.copy(m)
    m2.delta_coeffs = dc
    m2.patches = []
    off = 0
    for p in m.patches:
        q = copy.copy(p)
        if p.kind in COUPLED_KINDS:
            q.delta_coeffs = bdc[off:off + p.size].copy()
        m2.patches.append(q)
        off += p.slots
    return m2


class Slots:
    """per boundary slot: its cell, the cyclic partner cell (-1: none), coupled / primary flags"""

    def __init__(self, m):
        B = m.n_boundary_slots
        self.cell = m.boundary_arrays()[4].astype(np.int64) if B else np.zeros(0, np.int64)
        self.partner = -np.ones(B, np.int64)
        self.coupled = np.zeros(B, bool)
        self.prim = np.zeros(B, bool)
        off = 0
        for p in m.patches:
            if p.kind == "cyclic":
                self.partner[off:off + p.size] = m.patches[p.neighbour_patch].face_cells
            self.coupled[off:off + p.slots] = p.kind in COUPLED_KINDS
            self.prim[off:off + p.size] = True
            off += p.slots


def slot_types(m, ptypes):
    return np.repeat(np.asarray(ptypes), [p.slots for p in m.patches])


# ------------------------------------------------------------------------------------------------ operators
def _other(sl, vf, bvf):
    """the value across a coupled slot: the cyclic partner cell's, or the slot's exchanged copy"""
    return np.where(sl.partner >= 0, vf[..., np.maximum(sl.partner, 0)], bvf)


def gauss_grad(m, sl, tslot, vf, bvf, T=np.float64):
    """Gauss linear gradient [3, C] of one scalar: faces interpolate linearly, coupled slots interpolate with the
    patch weight, every other slot reads the boundary value; empty slots are skipped"""
    vf, bvf = np.asarray(vf, T), np.asarray(bvf, T)
    w, sf, V = np.asarray(m.weight, T), np.asarray(m.sf, T), np.asarray(m.volume, T)
    o, n = m.owner, m.neighbour
    yf = w * (vf[o] - vf[n]) + vf[n]
    s = np.zeros((3, m.n_cells), T)
    bsf, _, _, bw, _ = m.boundary_arrays()
    bsf, bw = np.asarray(bsf, T), np.asarray(bw, T)
    on = sl.prim & (tslot != EMPTY)
    bval = np.where(sl.coupled, bw * vf[sl.cell] + (1 - bw) * _other(sl, vf, bvf), bvf)
    for d in range(3):
        np.add.at(s[d], o, sf[:, d] * yf)
        np.add.at(s[d], n, -(sf[:, d] * yf))
        np.add.at(s[d], sl.cell[on], bsf[on, d] * bval[on])
    return s / V


def correction(m, sl, tslot, g, gam=None, bgam=None, gam_face=None, bgam_face=None, bg=None, T=np.float64, geom=None):
    """the explicit term of nc fields. g [nc, 3, C] cell gradients (bg [nc, 3, B]: their copies on processor slots);
    the diffusivity is a cell field gam [nc, C] (bgam [nc, B] on processor slots) or a face field gam_face [F] /
    bgam_face [B]. Returns (acc [nc, C] the per-cell sums of the outward fluxes -- what the source gains --,
    flux [nc, F], bflux [nc, B], scale [nc, C]). geom: the geometry arrays to use instead of m.nonorth_geometry(T)."""
    g = np.asarray(g, T)
    nc, C = g.shape[0], m.n_cells
    dc, k, bdc, bk = (np.asarray(a, T) for a in (geom or m.nonorth_geometry(T)))
    w, ms = np.asarray(m.weight, T), np.asarray(m.mag_sf, T)
    o, n = m.owner, m.neighbour
    gf = w * (g[:, :, o] - g[:, :, n]) + g[:, :, n]                      # [nc, 3, F]
    corr = (k[:, 0] * gf[:, 0] + k[:, 1] * gf[:, 1]) + k[:, 2] * gf[:, 2]
    if gam_face is not None:
        gamf = np.broadcast_to(np.asarray(gam_face, T), corr.shape)
    else:
        gam = np.asarray(gam, T)
        gamf = w * (gam[:, o] - gam[:, n]) + gam[:, n]
    flux = (gamf * ms) * corr
    acc = np.zeros((nc, C), T)
    scale = np.zeros((nc, C), T)
    mag = np.abs(gamf) * ms * np.sqrt((k * k).sum(axis=1)) * np.sqrt((gf * gf).sum(axis=1))
    for i in range(nc):
        np.add.at(acc[i], o, flux[i]); np.add.at(acc[i], n, -flux[i])
        np.add.at(scale[i], o, mag[i]); np.add.at(scale[i], n, mag[i])
    B = m.n_boundary_slots
    bflux = np.zeros((nc, B), T)
    on = sl.prim & sl.coupled & (tslot != EMPTY)
    if on.any():
        _, bms, _, bw, _ = m.boundary_arrays()
        bms, bw = np.asarray(bms, T), np.asarray(bw, T)
        c = sl.cell
        zb = np.zeros((nc, 3, B), T) if bg is None else np.asarray(bg, T)
        gb = bw * g[:, :, c] + (1 - bw) * _other(sl, g, zb)
        bcorr = (bk[:, 0] * gb[:, 0] + bk[:, 1] * gb[:, 1]) + bk[:, 2] * gb[:, 2]
        if bgam_face is not None:
            gamb = np.broadcast_to(np.asarray(bgam_face, T), bcorr.shape)
        else:
            zg = np.zeros((nc, B), T) if bgam is None else np.asarray(bgam, T)
            gamb = bw * gam[:, c] + (1 - bw) * _other(sl, gam, zg)
        bflux[:, on] = ((gamb * bms) * bcorr)[:, on]
        bmag = np.abs(gamb) * bms * np.sqrt((bk * bk).sum(axis=1)) * np.sqrt((gb * gb).sum(axis=1))
        for i in range(nc):
            np.add.at(acc[i], c[on], bflux[i, on])
            np.add.at(scale[i], c[on], bmag[i, on])
    return acc, flux, bflux, scale


def corrected_term(m, ptypes, fields, bfields, gam, T=np.float64, **kw):
    """gradients and correction of nc scalars fields [nc, C] / bfields [nc, B] with patch types `ptypes`"""
    sl = Slots(m)
    ts = slot_types(m, ptypes)
    g = np.stack([gauss_grad(m, sl, ts, f, b, T) for f, b in zip(fields, bfields)])
    return correction(m, sl, ts, g, gam=gam, T=T, **kw)


# ------------------------------------------------------------------------------------------------ exactness
# the quadratic's origin, near the middle of the sheared box: values stay small beside their differences, so the fp64
# restatement loses few digits to cancellation
X0 = np.array([1.05, 0.75, 0.5]) * L0


def quadratic(m, T=np.float64):
    """phi = x.H.x / 2 + a.x at the cell centres, and tr(H)"""
    H = np.array([[1.3, 0.4, -0.2], [0.4, -0.7, 0.5], [-0.2, 0.5, 2.1]]) * 1e6
    a = np.array([3.0, -2.0, 1.0]) * 1e2
    x = np.asarray(m.cell_centres, T) - X0
    return 0.5 * np.einsum("ci,ij,cj->c", x, np.asarray(H, T), x) + x @ np.asarray(a, T), float(np.trace(H))


def quadratic_periodic_parts(m, T=np.float64):
    """On the periodic sheared box a quadratic is not periodic; its gradient and its differences across a cyclic
    face are what a periodic field's would be once the jump is taken out, so the restated operator is applied with
    the partner values shifted by the patch translation: phi(x_partner + t) where t = delta - (x_partner - x_c).
    Returns (phi [C], other [B]: the field value at the far side of every cyclic slot)."""
    phi, trH = quadratic(m, T)
    H = np.asarray(np.array([[1.3, 0.4, -0.2], [0.4, -0.7, 0.5], [-0.2, 0.5, 2.1]]) * 1e6, T)
    a = np.asarray(np.array([3.0, -2.0, 1.0]) * 1e2, T)
    sl = Slots(m)
    x = np.asarray(m.cell_centres, T) - X0
    xo = x[sl.cell] + np.asarray(m.boundary_delta(), T)
    other = 0.5 * np.einsum("ci,ij,cj->c", xo, H, xo) + xo @ a
    return phi, other, trH


def exactness_residual(m, T=np.float64, gamma=1.7):
    """(corrected, orthogonal): max over cells of |restated laplacian - gamma tr(H) V| / (gamma |tr(H)| V) for the
    quadratic on a periodic sheared box. The box is closed periodically in z as well: on a wall k = 0 and the wall
    cells' Gauss gradient is not exact, which reaches two cell layers -- every cell of a 4-layer box with z walls."""
    phi, other, trH = quadratic_periodic_parts(m, T)
    sl = Slots(m)
    C, B = m.n_cells, m.n_boundary_slots
    ts = np.where(sl.coupled, 6, 0)
    # the far-side values enter as the slots' exchanged copies: partner = -1 makes every operator read them
    far = copy.copy(sl)
    far.partner = -np.ones(B, np.int64)
    gam = np.full((1, C), gamma, T)
    bgam = np.full((1, B), gamma, T)
    bw = np.asarray(m.boundary_arrays()[3], T)
    bvf = np.where(sl.coupled, other, phi[sl.cell])
    g = gauss_grad(m, far, ts, phi, bvf, T)[None]
    # the far cell's gradient: grad phi is affine, g(x + t) = g(x) + H t, and the partner cell sits at x_c + delta - t
    H = np.asarray(np.array([[1.3, 0.4, -0.2], [0.4, -0.7, 0.5], [-0.2, 0.5, 2.1]]) * 1e6, T)
    x = np.asarray(m.cell_centres, T)
    q = np.maximum(sl.partner, 0)
    t = x[sl.cell] + np.asarray(m.boundary_delta(), T) - x[q]
    bg = (g[0][:, q] + H @ t.T)[None]
    acc, _, _, _ = correction(m, far, ts, g, gam=gam, bgam=bgam, bg=bg, T=T)
    dc, _, bdc, _ = m.nonorth_geometry(T)

    def lap(dcs):
        o, n = m.owner, m.neighbour
        w, ms = np.asarray(m.weight, T), np.asarray(m.mag_sf, T)
        fl = gamma * ms * (dcs[0] * (phi[n] - phi[o]))
        out = np.zeros(C, T)
        np.add.at(out, o, fl); np.add.at(out, n, -fl)
        on = sl.prim & sl.coupled
        bms = np.asarray(m.boundary_arrays()[1], T)
        fb = gamma * bms * (dcs[1] * (other - phi[sl.cell]))
        np.add.at(out, sl.cell[on], fb[on])
        return out
    keep = np.ones(C, bool)
    if (~sl.coupled).any():   # walls: k = 0 there and the wall cells' Gauss gradient is not exact; two layers are lost
        keep[sl.cell[~sl.coupled]] = False
        near = ~keep
        keep[m.owner[near[m.neighbour]]] = False
        keep[m.neighbour[near[m.owner]]] = False
    exact = gamma * trH * np.asarray(m.volume, T)
    bo = np.asarray(m.boundary_arrays()[2], T)
    r_corr = np.abs(lap((dc, bdc)) + acc[0] - exact)[keep] / np.abs(exact[keep])
    r_orth = np.abs(lap((np.asarray(m.delta_coeffs, T), bo)) - exact)[keep] / np.abs(exact[keep])
    assert keep.sum() > 0
    return float(r_corr.max()), float(r_orth.max())


# ------------------------------------------------------------------------------------------------ accuracy
FIELDS = ("U", "p", "Y", "diffAlphaD", "he")


def case_state(m):
    """The state the GPU tests assemble (test_gpu_parity._case: the reacting Taylor-Green fields of case.tgv_fields
    with a hot kernel of radius 1.2 mm, Burke 9 species, uniform p), formed without a GPU: thermo by the oracle's
    point evaluation, boundary values as correctBoundaryConditions leaves them (the slot's cell value; cyclic slots
    interpolate). Its fields are nearly uniform away from the kernel -- p everywhere -- so their Gauss gradients are
    cancellation residues there, which is what the restatement's accuracy has to be measured on."""
    import oracle as O
    from dfmi import case
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "Burke2012_s9r23.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_Burke2012_s9r23.txt"), ym["species"])
    f = case.tgv_fields(m, ym["species"], kernel_radius=1.2e-3)
    th = O.thermo_points(t, f["T"], np.zeros(m.n_cells), f["p"], f["Y"], True)
    st = {"U": f["U"], "p": f["p"], "Y": f["Y"], "he": th["he"], "mu": th["mu"], "alpha": th["alpha"],
          "rhoD": th["rhoD"], "hai": th["hai"], "rho": th["rho"]}
    for k in list(st):
        st["boundary_" + k] = case.boundary_values(m, st[k]).reshape(np.shape(st[k])[:-1] + (m.n_boundary_slots,))
    st["inert"] = ym["species"].index("N2")
    return st


def _field_terms(m, st, T, geom):
    """{field: (acc, scale)} of the five explicit terms on a state, every operation in T"""
    pt = m.patch_types(1)
    kw = dict(T=T, geom=geom)
    S = st["Y"].shape[0]
    keep = np.arange(S) != st["inert"]
    out = {}
    a, _, _, sc = corrected_term(m, pt, st["U"], st["boundary_U"], np.repeat(st["mu"][None], 3, axis=0), **kw)
    out["U"] = (a, sc)
    sl, ts = Slots(m), slot_types(m, pt)
    g = gauss_grad(m, sl, ts, st["p"], st["boundary_p"], T)[None]
    w = m.weight
    rr = st["rho"] * 1e-6 / st["rho"].mean()          # rho rAU of the kind the pEqn interpolates
    rf = w * (rr[m.owner] - rr[m.neighbour]) + rr[m.neighbour]
    a, _, _, sc = correction(m, sl, ts, g, gam_face=rf, bgam_face=rr[sl.cell], **kw)
    out["p"] = (a, sc)
    a, _, _, sc = corrected_term(m, pt, st["Y"], st["boundary_Y"], st["rhoD"], **kw)
    out["Y"] = (a[keep], sc[keep])
    a, _, _, sc = corrected_term(m, pt, st["Y"], st["boundary_Y"], st["alpha"][None] * st["hai"], **kw)
    V = np.asarray(m.volume, T)
    out["diffAlphaD"] = (a.sum(axis=0) / V, sc.sum(axis=0) / V)
    a, _, _, sc = corrected_term(m, pt, st["he"][None], st["boundary_he"][None], st["alpha"][None], **kw)
    out["he"] = (a, sc)
    return out


def reference_error(m):
    """{field: max over cells of |acc_fp64 - acc_longdouble| / scale} on case_state(m). Both read the fp64 geometry
    (the library's is bitwise that, checked on its own): where a face is orthogonal k is the rounding residue of
    n - d / (n.d), which a long-double geometry would not reproduce, and it is all the scale there consists of."""
    st = case_state(m)
    geom = m.nonorth_geometry()
    a64, aL = _field_terms(m, st, np.float64, geom), _field_terms(m, st, LD, geom)
    out = {}
    for f in FIELDS:
        sc = aL[f][1]
        ok = sc > 0
        out[f] = float((np.abs(a64[f][0] - aL[f][0])[ok] / sc[ok]).max()) if ok.any() else 0.0
    return out


def measure():
    per, ort = exactness_residual(get_mesh("sheared-periodic-xyz"), LD)
    return {"reference_error": {n: reference_error(get_mesh(n)) for n in MESHES},
            "exactness_longdouble": per, "orthogonal_miss": ort}


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def gpu_bound(bounds, mesh_name, field):
    """4x the fp64 restatement's measured error for that field on that mesh's case state, floored at 1e-13
    (les_nut_bounds.json's rule)"""
    return max(4.0 * bounds["reference_error"][mesh_name][field], 1e-13)


# ------------------------------------------------------------------------------------------------ pressure loop
def p_boundary(m, sl, tslot, p, bp):
    """p.correctBoundaryConditions() for zeroGradient / fixedValue / cyclic slots (the loop's cases)"""
    bw = m.boundary_arrays()[3]
    out = np.array(bp, dtype=np.float64)
    zg = (tslot == 0) | (tslot == 8)
    out[zg] = p[sl.cell[zg]]
    cy = tslot == 6
    out[cy] = bw[cy] * p[sl.cell[cy]] + (1 - bw[cy]) * p[np.maximum(sl.partner, 0)[cy]]
    return out


def p_loop(m, ptype_p, parts, base, rf, brf, p0, bp0, n_nonorth):
    """the pEqn corrector loop with exact solves: parts = the library's lower / upper / diag / internal_coeffs /
    boundary_coeffs, base = the source without the explicit term. Returns (p, boundary_p, flux [F], bflux [B]) with
    flux = pEqn.flux() including the face flux correction of the last pass."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from oracle import ldu_system
    sl = Slots(m)
    ts = slot_types(m, ptype_p)
    C = m.n_cells
    p, bp = np.array(p0, dtype=np.float64), np.array(bp0, dtype=np.float64)
    for _ in range(n_nonorth + 1):
        g = gauss_grad(m, sl, ts, p, bp)[None]
        acc, fl, bfl, _ = correction(m, sl, ts, g, gam_face=rf, bgam_face=brf)
        rows, cols, vals, b = ldu_system(m, ptype_p, parts["lower"], parts["upper"], parts["diag"], base + acc[0],
                                         parts["internal_coeffs"], parts["boundary_coeffs"])
        p = spla.spsolve(sp.coo_matrix((vals, (rows, cols)), shape=(C, C)).tocsc(), b)
        bp = p_boundary(m, sl, ts, p, bp)
    o, n = m.owner, m.neighbour
    flux = (parts["upper"] * p[n] - parts["lower"] * p[o]) - fl[0]
    ic, bc = parts["internal_coeffs"], parts["boundary_coeffs"]
    other = np.where(sl.partner >= 0, p[np.maximum(sl.partner, 0)], 1.0)
    bflux = np.where(sl.coupled, ic * p[sl.cell] - bc * other, ic * p[sl.cell] - bc) - bfl[0]
    bflux[~sl.prim | (ts == EMPTY)] = 0.0
    return p, bp, flux, bflux


if __name__ == "__main__":
    if "--measure" not in sys.argv:
        sys.exit("usage: nonorth_reference.py --measure")
    doc = {"about": "tests/nonorth_reference.py --measure. reference_error: max of |acc_fp64 - acc_longdouble| / "
                    "sum_f |gamma_f| |Sf| |k| |grad phi|_f of the NumPy restatement of the non-orthogonal correction, per "
                    "mesh and field, on the state the GPU tests assemble (case_state: nearly uniform away from the hot "
                    "kernel, p uniform, so the gradients there are cancellation residues). exactness_longdouble: the long-double restatement's deviation of the corrected laplacian of a "
                    "quadratic from gamma tr(H) V on the periodic sheared box, relative; orthogonal_miss: the "
                    "orthogonal form's on the same cells."}
    doc.update(measure())
    with open(BOUNDS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1))
