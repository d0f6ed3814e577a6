"""The spray coupling terms restated in NumPy (include/dfmi.h, spray block), and one outer iteration with them.

One function per equation applies the header's statement to (diag, source) in the header's operation order; NumPy's
float64 ufuncs round every operation once and never fuse a multiply with an add, so the results are what the device
kernels (built with -ffp-contract=off) produce, bit for bit. The same functions evaluate in numpy.longdouble when
`dtype` says so: test_spray_cpu.py measures the float64 forms against that.

spray_time_step restates Oracle.time_step from the oracle's own stage methods with the terms applied between each
assembly and its solve. Nothing here reads the library under test.
"""
import numpy as np

SMALL = 1e-15          # OpenFOAM's `small`
EMPTY = 3              # dfmi.mesh.EMPTY


def _a(x, dtype):
    return np.asarray(x, dtype=dtype)


def rho_term(diag, source, rhoTrans, rdt, V, rho, semi, dtype=np.float64):
    """parcels.Srho(rho): (diag, source) of the rhoEqn with the term; rho: the cell values before the solve"""
    diag, source, rhoTrans, V, rho = (_a(x, dtype) for x in (diag, source, rhoTrans, V, rho))
    rdt = dtype(rdt)
    s = np.zeros(diag.shape, dtype=dtype)
    for i in range(rhoTrans.shape[0]):
        s = s + rhoTrans[i]
    t = s * rdt
    if semi:
        a = (t / V) / rho
        return diag - V * np.maximum(a, dtype(0)), source + (V * np.minimum(a, dtype(0))) * rho
    return diag.copy(), source + t


def u_term(diag, source, source_solve, UTrans, UCoeff, U, rdt, semi, dtype=np.float64):
    """parcels.SU(U): (diag [C], source [3, C], source_solve [3, C]) with the term; U: the cell values before the solve"""
    diag, source, source_solve, UTrans, U = (_a(x, dtype) for x in (diag, source, source_solve, UTrans, U))
    rdt = dtype(rdt)
    if semi:
        uc = _a(UCoeff, dtype)
        t = (UTrans + uc * U) * rdt
        return diag + uc * rdt, source + t, source_solve + t
    t = UTrans * rdt
    return diag.copy(), source + t, source_solve + t


def y_term(diag, source, rhoTrans, Y, rdt, V, inert, semi, dtype=np.float64):
    """parcels.SYi(i, Yi): (diag [S, C], source [S, C]) with the terms; row `inert` is left as it is"""
    diag, source, rhoTrans, Y, V = (_a(x, dtype) for x in (diag, source, rhoTrans, Y, V))
    rdt = dtype(rdt)
    d, b = diag.copy(), source.copy()
    for i in range(rhoTrans.shape[0]):
        if i == inert:
            continue
        t = rhoTrans[i] * rdt
        if semi:
            s = t / V
            neg = s < 0
            d[i] = np.where(neg, d[i] + (V * (-s)) / (Y[i] + dtype(SMALL)), d[i])
            b[i] = np.where(neg, b[i], b[i] + s * V)
        else:
            b[i] = b[i] + t
    return d, b


def e_term(diag, source, rhoTrans, hc, hsTrans, hsCoeffByCp, he, rdt, V, semi, dtype=np.float64):
    """parcels.Sh(he) and hcSource: (diag, source) of the EEqn with the terms; he: the cell values before the solve"""
    diag, source, rhoTrans, hsTrans, he, V = (_a(x, dtype) for x in (diag, source, rhoTrans, hsTrans, he, V))
    rdt = dtype(rdt)
    sens = hsTrans * rdt
    d = diag.copy()
    if semi:
        a = (_a(hsCoeffByCp, dtype) * rdt) / V
        pos = a >= 0
        aV = a * V
        d = np.where(pos, d + aV, d)
        s = np.where(pos, source + (sens + aV * he), source + sens)
    else:
        s = source + sens
    h = np.zeros(diag.shape, dtype=dtype)
    for i in range(rhoTrans.shape[0]):
        h = h + rhoTrans[i] * dtype(hc[i])
    return d, s + h * rdt


def rAU_of(mesh, ptypes_U, diag, ic, V):
    """1 / UEqn.A(): diag plus the component average of internalCoeffs over the cell's primary non-empty slots in slot
    order, over the volume (df_oracle.cpp u_assemble; k_u_assemble)"""
    m = mesh
    B = m.n_boundary_slots
    ic = np.asarray(ic).reshape(3, B)
    r = np.array(diag, dtype=np.float64)
    bfc = m.boundary_arrays()[4].astype(np.int64)
    off = np.concatenate([[0], np.cumsum([p.slots for p in m.patches])]).astype(np.int64)
    for pi, p in enumerate(m.patches):
        if ptypes_U[pi] == EMPTY or p.size == 0:
            continue
        sl = slice(off[pi], off[pi] + p.size)
        np.add.at(r, bfc[sl], (ic[0, sl] + ic[1, sl] + ic[2, sl]) / 3)
    return 1 / (r / np.asarray(V))


def hc_of(table):
    """hc_i = Hf298_i / W_i, the library's heat_of_formation_per_mass restated by the chemistry oracle"""
    from chem_oracle import hf298_per_mass
    return hf298_per_mass(table.nasa, table.W)


# ---- the stages of one outer iteration, each an oracle stage followed by its term
def rho_stage(o, src, sch):
    a = o.arr
    rho0 = a["rho"].copy()
    o.rho_eqn()
    d, s = rho_term(a["out_rho_diag"], a["out_rho_source"], src["rhoTrans"], o.rdt, o.m.volume, rho0, sch["rho"])
    a["rho"][...] = s / d
    o.correct_bc("rho", "rho", 1)
    return d, s


def u_stage(o, src, sch):
    a = o.arr
    u = o.u_assemble()
    C_ = o.m.n_cells
    d, s, ss = u_term(u["diag"], u["source"].reshape(3, C_), u["source_solve"].reshape(3, C_), src["UTrans"],
                      src.get("UCoeff"), a["U"], o.rdt, sch["U"])
    u = dict(u, diag=d, source=s.reshape(-1), source_solve=ss.reshape(-1))
    o.set("ueqn_source", u["source"].copy())     # what u_hbya reads
    if sch["U"]:                                 # rAU sees the implicit part
        a["rAU"][...] = rAU_of(o.m, o.ptypes["U"], d, u["internal_coeffs"], o.m.volume)
        o.correct_bc("rAU", "extrapolated", 1)
    return u


def y_stage(o, src, sch):
    a = o.arr
    S, C_ = o.S, o.m.n_cells
    o.y_prep()
    y = o.y_assemble()
    d, s = y_term(y["diag"].reshape(S, C_), y["source"].reshape(S, C_), src["rhoTrans"], a["Y"], o.rdt, o.m.volume,
                  o.inert, sch["Yi"])
    return dict(y, diag=d.reshape(-1), source=s.reshape(-1))


def e_stage(o, src, sch, hc, fresh_weights=False):
    a = o.arr
    e = o.e_assemble(fresh_weights)
    d, s = e_term(e["diag"], e["source"], src["rhoTrans"], hc, src["hsTrans"], src.get("hsCoeffByCp"), a["he"], o.rdt,
                  o.m.volume, sch["h"])
    return dict(e, diag=d, source=s)


def spray_time_step(o, sources, schemes, n_corr, hc):
    """Oracle.time_step (dfLowMachFoam.C:284-531, nOuter = 1) with the parcel terms in the rho, U, Yi and he equations,
    the rhoEqn of every pressure corrector included (pEqn.H:103). sources: {"rhoTrans" [S, C], "UTrans" [3, C],
    "UCoeff" [C], "hsTrans" [C], "hsCoeffByCp" [C]}; schemes: {"rho", "U", "Yi", "h"} -> 0 | 1; hc: hc_of(table)."""
    m = o.m
    C_, F, B, S = m.n_cells, m.n_faces, m.n_boundary_slots, o.S
    a = o.arr
    for n, k in (("rho_old", "rho"), ("boundary_rho_old", "boundary_rho"), ("phi_old", "phi"),
                 ("boundary_phi_old", "boundary_phi"), ("U_old", "U"), ("boundary_U_old", "boundary_U"),
                 ("K_old", "K"), ("p_old", "p"), ("boundary_p_old", "boundary_p")):
        a[n][...] = a[k]
    rho_stage(o, sources, schemes)
    u = u_stage(o, sources, schemes)
    for k in range(3):
        a["U"][k] = o.solve_ldu(u["lower"], u["upper"], u["diag"], u["source_solve"][k * C_:(k + 1) * C_],
                                u["internal_coeffs"][k * B:(k + 1) * B], u["boundary_coeffs"][k * B:(k + 1) * B], "U")
    o.correct_bc("U", "U", 3)
    Ux, Uy, Uz = a["U"]
    a["K"][...] = 0.5 * (Ux * Ux + Uy * Uy + Uz * Uz)
    bx, by, bz = a["boundary_U"]
    a["boundary_K"][...] = 0.5 * (bx * bx + by * by + bz * bz)
    y = y_stage(o, sources, schemes)
    for s in range(S):
        if s == o.inert:
            continue
        a["Y"][s] = o.solve_ldu(y["lower"][s * F:(s + 1) * F], y["upper"][s * F:(s + 1) * F],
                                y["diag"][s * C_:(s + 1) * C_], y["source"][s * C_:(s + 1) * C_],
                                y["internal_coeffs"][s * B:(s + 1) * B], y["boundary_coeffs"][s * B:(s + 1) * B], "Y")
    o.y_inert()
    o.energy_gradient()
    o.correct_bc("he", "he", 1)
    e = e_stage(o, sources, schemes, hc)
    a["he"][...] = o.solve_ldu(e["lower"], e["upper"], e["diag"], e["source"], e["internal_coeffs"],
                               e["boundary_coeffs"], "he")
    o.correct_bc("he", "he", 1)
    o.thermo_correct(False)
    for _ in range(n_corr):
        a["rho"][...] = a["p"] * a["psi"]; a["boundary_rho"][...] = a["boundary_p"] * a["boundary_psi"]
        a["psip0"][...] = a["psi"] * a["p"]; a["boundary_psip0"][...] = a["boundary_psi"] * a["boundary_p"]
        o.u_hbya()
        pq = o.p_assemble()
        a["p"][...] = o.solve_ldu(pq["lower"], pq["upper"], pq["diag"], pq["source"], pq["internal_coeffs"],
                                  pq["boundary_coeffs"], "p")
        o.p_post()
        a["rho"][...] = a["rho"] + (a["psi"] * a["p"] - a["psip0"])
        a["boundary_rho"][...] = a["boundary_rho"] + (a["boundary_psi"] * a["boundary_p"] - a["boundary_psip0"])
        rho_stage(o, sources, schemes)
    a["rho"][...] = a["p"] * a["psi"]
    a["boundary_rho"][...] = a["boundary_p"] * a["boundary_psi"]


# ---- the float64 forms against numpy.longdouble (tests/golden/spray/term_bounds.json)
TERMS = ("rho-explicit", "rho-semiImplicit", "U-explicit", "U-semiImplicit", "Yi-explicit", "Yi-semiImplicit",
         "h-explicit", "h-semiImplicit")


def _err(got, ref, base):
    """max |got - ref| / (|base| + |ref|): the rounding of a handful of operations at the size of what went in and
    what came out (0 / 0 counts as 0)"""
    LD = np.longdouble
    num = np.abs(_a(got, LD) - ref)
    den = np.abs(_a(base, LD)) + np.abs(ref)
    return float(np.max(np.where(den > 0, num / np.where(den > 0, den, 1), 0)))


def measure(n=4096, S=9, inert=8, seed=5):
    """{term: max error of the float64 form against the long-double one} on random inputs of both signs, with
    Y = 0 entries under species sinks and hsCoeffByCp of both signs"""
    LD = np.longdouble
    rng = np.random.default_rng(seed)
    rdt = 1e6
    V = rng.uniform(0.5e-9, 2e-9, n)
    rho = rng.uniform(0.5, 2.0, n)
    diag = rdt * rho * V * rng.uniform(0.8, 1.5, n)
    rT = V * 1e-3 * rng.standard_normal((S, n))
    Y = rng.random((S, n)) * (rng.random((S, n)) < 0.7)
    UT, U, UC = V * 1e-2 * rng.standard_normal((3, n)), rng.standard_normal((3, n)), V * 1e-2 * rng.random(n)
    hT, hC, he = V * 1e3 * rng.standard_normal(n), V * 1e-2 * rng.standard_normal(n), 1e5 * rng.standard_normal(n)
    hc = 1e6 * rng.standard_normal(S)
    out = {}
    for semi in (0, 1):
        tag = "semiImplicit" if semi else "explicit"
        src = diag * rng.standard_normal(n)
        got, ref = rho_term(diag, src, rT, rdt, V, rho, semi), rho_term(diag, src, rT, rdt, V, rho, semi, LD)
        out["rho-" + tag] = max(_err(got[0], ref[0], diag), _err(got[1], ref[1], src))
        s3 = diag * rng.standard_normal((3, n))
        got, ref = u_term(diag, s3, s3 * 0.9, UT, UC, U, rdt, semi), u_term(diag, s3, s3 * 0.9, UT, UC, U, rdt, semi, LD)
        out["U-" + tag] = max(_err(got[0], ref[0], diag), _err(got[1], ref[1], s3), _err(got[2], ref[2], s3 * 0.9))
        dS, sS = np.tile(diag, (S, 1)), diag * rng.standard_normal((S, n))
        got, ref = y_term(dS, sS, rT, Y, rdt, V, inert, semi), y_term(dS, sS, rT, Y, rdt, V, inert, semi, LD)
        out["Yi-" + tag] = max(_err(got[0], ref[0], dS), _err(got[1], ref[1], sS))
        sE = diag * he * rng.standard_normal(n)
        got = e_term(diag, sE, rT, hc, hT, hC, he, rdt, V, semi)
        ref = e_term(diag, sE, rT, hc, hT, hC, he, rdt, V, semi, LD)
        out["h-" + tag] = max(_err(got[0], ref[0], diag), _err(got[1], ref[1], sE))
    return out


def load_bounds():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spray", "term_bounds.json")) as f:
        return json.load(f)


# ---- inputs of the tests
def sources(m, S, inert, Y, seed=11, frac=0.1):
    """{"rhoTrans" [S, C], "UTrans" [3, C], "UCoeff" [C], "hsTrans" [C], "hsCoeffByCp" [C]}: non-zero in the first four
    cells and in about `frac` of the others, of both signs, at a cloud's per-step size relative to the cell mass M = V x
    1 kg/m^3 (1e-5 M per species, 1e-2 M m/s, 1e3 M J, coefficients 1e-2 M; DESIGN.md 19 says why). Edge cells: cell 1's
    species sum cancels exactly; cell 2 has a negative and cell 3 a positive hsCoeffByCp; and, where a non-inert species
    i has Y_i = 0 in some cell c != 1, rhoTrans_i < 0 there (the `small` denominator), reported as "zero_cell": (i, c).
    Y [S, C]: the state's mass fractions."""
    rng = np.random.default_rng(seed)
    C_ = m.n_cells
    V = np.asarray(m.volume)
    hit = rng.random(C_) < frac
    hit[:4] = True
    mass = V * 1.0          # about rho V with rho ~ 1 kg/m^3
    out = {"rhoTrans": np.where(hit, mass * 1e-5 * rng.standard_normal((S, C_)), 0.0),
           "UTrans": np.where(hit, mass * 1e-2 * rng.standard_normal((3, C_)), 0.0),
           "UCoeff": np.where(hit, mass * 1e-2 * rng.random(C_), 0.0),
           "hsTrans": np.where(hit, mass * 1e3 * rng.standard_normal(C_), 0.0),
           "hsCoeffByCp": np.where(hit, mass * 1e-2 * rng.standard_normal(C_), 0.0)}
    # cell 1: the species sum cancels exactly
    out["rhoTrans"][:, 1] = 0.0
    j = [i for i in range(S) if i != inert][:2]
    out["rhoTrans"][j[0], 1] = mass[1] * 2e-5
    out["rhoTrans"][j[1], 1] = -mass[1] * 2e-5
    # a sink of a species that is absent from its cell
    for i in range(S):
        absent = [c for c in np.flatnonzero(Y[i] == 0.0) if c != 1]
        if i != inert and absent:
            c = int(absent[0])
            out["rhoTrans"][i, c] = -mass[c] * 1e-5
            out["zero_cell"] = (i, c)
            break
    # cell 2: a negative implicit enthalpy coefficient; cell 3: a positive one
    out["hsCoeffByCp"][2] = -mass[2] * 1e-2
    out["hsCoeffByCp"][3] = mass[3] * 1e-2
    return out
