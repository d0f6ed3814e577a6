"""Reference of the LES eddy viscosity (include/dfmi.h dfmi_turbulence_correct) and the oracle of the
turbulent equations.

nut per cell, restated from the formulas in NumPy, in fp64 and in long double (x87 extended: 64-bit mantissa),
vectorised over n states. With g[3 i + j] = d_i U_j, D = symm(g) and the filter width delta:

    Smagorinsky   a = Ce / delta, b = (2/3) tr D, c = 2 Ck delta (dev(D) && D)
                  k = ((-b + sqrt(b^2 + 4 a c)) / (2 a))^2
    WALE          Sd = dev(symm(g . g)), m = Sd && Sd, s = D && D
                  k = (Cw^2 delta / Ck)^2 m^3 / ((s^(5/2) + m^(5/4))^2 + 1e-15)
    nut = Ck delta sqrt(k)

and the quantities the three assemblies read, in this operation order, on cells and on boundary slots alike:

    mut = rho nut;  muEff = mut + mu;  alphaEff = alpha + mut / Prt;  DEff_i = rhoD_i + mut / Sct

LesOracle is the sequential oracle with these injected: mu := muEff, alpha := alphaEff, rhoD := DEff, and the terms
the reference drops for simulationType != laminar (YEqn.H:101-106, EEqn.H:30-36) zeroed: sumYDiffError (so phiUc),
diffAlphaD, hDiffCorrFlux. Its assemblies are then the turbulent equations, and the added zeros are exact.

`python tests/les_reference.py --measure` evaluates the fp64 restatement against the long-double one on every state
class and writes the maxima of |nut_fp64 - nut_longdouble| / (delta^2 |g|_F) to tests/golden/les_nut_bounds.json; the
GPU tolerance is derived from that file (gpu_bound), never from a kernel's output.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BOUNDS_PATH = os.path.join(GOLDEN, "les_nut_bounds.json")
MODELS = {"Smagorinsky": 1, "WALE": 2}
DEFAULTS = {"Ck": 0.094, "Ce": 1.048, "Cw": 0.325, "Prt": 1.0, "Sct": 1.0}
CLASSES = ("random", "zero", "rotation", "shear", "dilatation+", "dilatation-", "general")

for _p in (os.path.join(os.path.dirname(HERE), "deepflame-dev_amd"), os.path.join(os.path.dirname(HERE), "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


# ------------------------------------------------------------------------------------------------ nut
def nut_from_grad(g, delta, model: int, coef: dict | None = None, dtype=np.float64):
    """nut [n] from g [9, n] (g[3 i + j] = d_i U_j) and delta [n], every operation in `dtype`, in the order the
    kernel takes (fv_kernels.hip les_nut)"""
    q = dict(DEFAULTS, **(coef or {}))
    T = dtype
    g = np.asarray(g, dtype=T)
    del_ = np.asarray(delta, dtype=T)
    Ck, Ce, Cw = T(q["Ck"]), T(q["Ce"]), T(q["Cw"])
    third, half, two = T(1.0) / T(3.0), T(0.5), T(2.0)
    D00, D11, D22 = g[0], g[4], g[8]
    D01, D02, D12 = half * (g[1] + g[3]), half * (g[2] + g[6]), half * (g[5] + g[7])
    with np.errstate(invalid="ignore"):
        if model == 1:
            tr = D00 + D11 + D22
            t3 = third * tr
            dd = ((D00 - t3) * D00 + (D11 - t3) * D11 + (D22 - t3) * D22) + two * (D01 * D01 + D02 * D02 + D12 * D12)
            a, b, c = Ce / del_, (two / T(3.0)) * tr, two * Ck * del_ * dd
            r = (-b + np.sqrt(b * b + T(4.0) * a * c)) / (two * a)
            k = r * r
        elif model == 2:
            P = [[g[3 * i] * g[j] + g[3 * i + 1] * g[3 + j] + g[3 * i + 2] * g[6 + j] for j in range(3)] for i in range(3)]
            t3 = third * (P[0][0] + P[1][1] + P[2][2])
            S00, S11, S22 = P[0][0] - t3, P[1][1] - t3, P[2][2] - t3
            S01, S02, S12 = half * (P[0][1] + P[1][0]), half * (P[0][2] + P[2][0]), half * (P[1][2] + P[2][1])
            mm = (S00 * S00 + S11 * S11 + S22 * S22) + two * (S01 * S01 + S02 * S02 + S12 * S12)
            ss = (D00 * D00 + D11 * D11 + D22 * D22) + two * (D01 * D01 + D02 * D02 + D12 * D12)
            s52, m54 = ss * ss * np.sqrt(ss), mm * np.sqrt(np.sqrt(mm))
            den, cw = s52 + m54, Cw * Cw * del_ / Ck
            k = (cw * cw) * (mm * mm * mm) / (den * den + T(1e-15))
        else:
            raise ValueError(f"LES model {model}")
        return Ck * del_ * np.sqrt(k)


def nut_error(nut, g, delta, model, coef=None):
    """|nut - nut_longdouble(g)| / (delta^2 |g|_F) per cell; where g = 0 the reference is exactly 0 and so must nut
    be (error 0, else inf)"""
    ref = nut_from_grad(g, delta, model, coef, LD)
    g = np.asarray(g, dtype=LD)
    scale = np.asarray(delta, dtype=LD) ** 2 * np.sqrt((g * g).sum(axis=0))
    diff = np.abs(np.asarray(nut, dtype=LD) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(scale > 0, diff / np.where(scale > 0, scale, 1), np.where(diff == 0, LD(0), LD(np.inf)))
    return np.asarray(e, dtype=np.float64)


def effective(rho, nut, mu, alpha, rhoD, Prt=1.0, Sct=1.0):
    """(muEff, alphaEff, DEff [S, n], mut / Sct) in the stated operation order (fp64)"""
    mut = np.asarray(rho, dtype=np.float64) * np.asarray(nut, dtype=np.float64)
    ms = mut / Sct
    return mut + mu, alpha + mut / Prt, np.asarray(rhoD) + ms[None, :], ms


# ------------------------------------------------------------------------------------------------ state classes
LINEAR_G = {   # G[i][j] = d_i U_j of the linear velocity fields U = G^T x (per second)
    "zero": np.zeros((3, 3)),
    "rotation": np.array([[0.0, 700.0, -300.0], [-700.0, 0.0, 500.0], [300.0, -500.0, 0.0]]),
    "shear": np.array([[0.0, 1900.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]),
    "dilatation+": 1300.0 * np.eye(3),
    "dilatation-": -1300.0 * np.eye(3),
    "general": np.array([[820.0, -1430.0, 260.0], [390.0, -1210.0, 1750.0], [-640.0, 980.0, 310.0]]),
}


def class_states(cls: str, n: int = 4096, seed: int = 11):
    """(g [9, n], delta [n]) of a state class: random tensors of the Taylor-Green scale whose trace takes both signs,
    or one chosen tensor G over a range of magnitudes and filter widths, exact and with rounding-level noise on every
    entry (what a Gauss gradient of the linear field returns)"""
    rng = np.random.default_rng(seed + CLASSES.index(cls))
    delta = 10.0 ** rng.uniform(-5.0, -2.5, n)
    if cls == "random":
        g = 4e3 * rng.standard_normal((9, n)) * 10.0 ** rng.uniform(-2.0, 1.0, n)
        return g, delta
    G = LINEAR_G[cls].reshape(9, 1)
    g = G * 10.0 ** rng.uniform(-2.0, 2.0, n)
    rel = 1.0 + 4e-16 * rng.standard_normal((9, n))
    ab = np.abs(g).max(axis=0) * 2e-16 * rng.standard_normal((9, n))   # the zero entries move too
    return np.where(np.arange(n) >= n // 2, g * rel + ab, g), delta


def measure():
    """{model: {class: max error of the fp64 restatement against the long-double one}}"""
    out = {}
    for name, model in MODELS.items():
        out[name] = {}
        for cls in CLASSES:
            g, delta = class_states(cls)
            out[name][cls] = float(nut_error(nut_from_grad(g, delta, model), g, delta, model).max())
    return out


def load_bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def gpu_bound(bounds, model_name: str, cls: str) -> float:
    """4x the fp64 restatement's measured maximum for that class and model, floored at 1e-13 (the factor
    covers the device's square roots and division sequences, one more rounding per term each)"""
    return max(4.0 * bounds["models"][model_name][cls], 1e-13)


# ------------------------------------------------------------------------------------------------ oracle
def _oracle_base():
    import oracle as O
    return O.Oracle


class LesOracle(_oracle_base()):
    """The sequential oracle with the LES fields injected (module docstring). les = {"model": 1 | 2, coefficients};
    delta [C]; nut_ptypes: nut's patch types (default: "calculated"). nut is seeded from the initial U; the inherited
    time_step ends with the nut update from the final U. set_nut() installs a given nut instead (the device's own,
    for the bitwise assembly comparison)."""

    def __init__(self, mesh, table, state, ptypes, inert, rdt, les: dict, delta, schemes=None, nut_ptypes=None,
                 boundary_nut=None):
        super().__init__(mesh, table, state, ptypes, inert, rdt, schemes)
        self.les = dict(DEFAULTS, **les)
        self.delta = np.asarray(delta, dtype=np.float64)
        self._i("ptype_nut", ptypes["calculated"] if nut_ptypes is None else nut_ptypes)
        self._d("nut", np.zeros(mesh.n_cells))
        self._d("boundary_nut", np.zeros(mesh.n_boundary_slots) if boundary_nut is None else boundary_nut)
        self.turbulence_correct()

    def grad_u(self):
        """g [9, C], g[3 i + j] = d_i U_j: the oracle's Gauss gradient of each component of U (the sums of its
        vector gradient, out_gradU)"""
        C_ = self.m.n_cells
        g = np.zeros((9, C_))
        for j in range(3):
            self._d("les_u", self.arr["U"][j]); self._d("les_bu", self.arr["boundary_U"][j])
            gj = self.out("les_gj", 3 * C_)
            self._run("orc_grad_scalar", b"les_u", b"les_bu", b"ptype_U", b"les_gj", None)
            for i in range(3):
                g[3 * i + j] = gj[i * C_:(i + 1) * C_]
        return g

    def turbulence_correct(self):
        self.arr["nut"][...] = nut_from_grad(self.grad_u(), self.delta, self.les["model"], self.les)
        self.correct_bc("nut", "nut", 1)

    def set_nut(self, nut, boundary_nut):
        self.arr["nut"][...] = nut
        self.arr["boundary_nut"][...] = boundary_nut

    def effective(self):
        """{name: (cells, boundary slots)} of muEff, alphaEff, DEff from the arrays as they stand"""
        a = self.arr
        c = effective(a["rho"], a["nut"], a["mu"], a["alpha"], a["rhoD"], self.les["Prt"], self.les["Sct"])
        b = effective(a["boundary_rho"], a["boundary_nut"], a["boundary_mu"], a["boundary_alpha"], a["boundary_rhoD"],
                      self.les["Prt"], self.les["Sct"])
        return {"mu": (c[0], b[0]), "alpha": (c[1], b[1]), "rhoD": (c[2], b[2])}

    def _with(self, names, zero, fn):
        """fn() with the effective fields registered under `names` and the fields of `zero` zeroed; the thermo's own
        mu / alpha / rhoD come back afterwards"""
        eff = self.effective()
        keep = {}
        for n in names:
            for pre, v in (("", eff[n][0]), ("boundary_", eff[n][1])):
                keep[pre + n] = self.arr[pre + n].copy()
                self.arr[pre + n][...] = v
        for n in zero:
            for pre in ("", "boundary_"):
                if pre + n in self.arr:
                    self.arr[pre + n][...] = 0.0
        try:
            return fn()
        finally:
            for n, v in keep.items():
                self.arr[n][...] = v

    def u_assemble(self):
        return self._with(("mu",), (), super().u_assemble)

    def y_prep(self):
        """LES: only the div(phi,Yi_h) weights; the preparation's fields are zero"""
        m = self.m
        for k in ("sumYDiffError", "hDiffCorrFlux"):
            self.set(k, np.zeros((3, m.n_cells)))
            self.set("boundary_" + k, np.zeros((3, m.n_boundary_slots)))
        self.set("diffAlphaD", np.zeros(m.n_cells))
        self._run("orc_conv_weights")

    def y_assemble(self):
        return self._with(("rhoD",), ("sumYDiffError",), super().y_assemble)

    def e_assemble(self, fresh_weights=False):
        return self._with(("alpha",), ("diffAlphaD", "hDiffCorrFlux"), lambda: super(LesOracle, self).e_assemble(fresh_weights))

    def time_step(self, n_corr=2):
        super().time_step(n_corr)
        self.turbulence_correct()


if __name__ == "__main__":
    if "--measure" not in sys.argv:
        sys.exit("usage: les_reference.py --measure")
    doc = {"about": "max of |nut_fp64 - nut_longdouble| / (delta^2 |g|_F) of the NumPy fp64 restatement of the LES eddy "
                    "viscosity against the long-double one (tests/les_reference.py), per model and state class; written "
                    "by tests/les_reference.py --measure",
           "models": measure()}
    with open(BOUNDS_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, v in doc["models"].items():
        print(name, {c: f"{x:.2e}" for c, x in v.items()})
