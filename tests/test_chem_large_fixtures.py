"""The fixtures of the 13..64-species chemistry tests (tests/golden/make_chem_large_fixtures.py) load and are what
tests/test_gpu_chem_large.py takes them for."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

# species / reactions, then elementary, three-body, Lindemann, Troe
MECHS = {"drm19": ("drm19.yaml", "thermo_drm19.txt", 21, 84, (70, 6, 0, 8)),
         "gri30": ("gri30.yaml", "thermo_gri30_36.txt", 36, 219, (187, 6, 1, 25))}


@pytest.mark.parametrize("name", sorted(MECHS))
def test_mechanism_and_table_load(name):
    from dfmi.kinetics import parse_mechanism
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    mech_file, table_file, S, R, types = MECHS[name]
    mc = parse_mechanism(os.path.join(GOLDEN, mech_file))
    assert (mc.S, mc.R) == (S, R)
    assert tuple(int((mc.itype == k).sum()) for k in range(4)) == types
    assert R <= 256 and S <= 64                                   # what the cooperative kernel takes
    assert ((mc.reac >= 0).sum(axis=1) <= 3).all() and ((mc.prod >= 0).sum(axis=1) <= 3).all()
    idata, irs, dd = mc.pack()
    assert idata.size == 8 * R and irs.size == 6 * R and dd.size == R * (17 + S)
    ym = read_yaml_mechanism(os.path.join(GOLDEN, mech_file))
    t = read_thermo_table(os.path.join(GOLDEN, table_file), ym["species"])
    assert t.S == S and np.allclose(t.W, ym["W"], rtol=1e-12) and np.allclose(t.nasa, ym["nasa"], rtol=1e-12)
    assert t.visc.shape == (S, 5) and t.cond.shape == (S, 5) and t.bdiff.shape == (S, S, 5)
    assert all(np.all(np.isfinite(a)) for a in (t.W, t.nasa, t.visc, t.cond, t.bdiff))


@pytest.mark.parametrize("name", sorted(MECHS))
def test_state_fixture(name):
    from dfmi.mech import read_yaml_mechanism
    fix = json.load(open(os.path.join(GOLDEN, "chem_large_states.json")))
    assert fix["dt"] == 1e-6
    f = fix["mechanisms"][name]
    mech_file, table_file, S, R, _ = MECHS[name]
    assert (f["mechanism"], f["thermo"]) == (mech_file, table_file)
    assert f["species"] == read_yaml_mechanism(os.path.join(GOLDEN, mech_file))["species"]
    T, p, rho, Y, RR = (np.asarray(f[k]) for k in ("T", "p", "rho", "Y", "RR"))
    n = f["kept"]
    assert n == 48 and f["examined"] - f["dropped"] == n and f["dropped"] <= 0.1 * f["examined"]
    assert T.shape == p.shape == rho.shape == (n,) and Y.shape == RR.shape == (S, n)
    assert T.min() >= 300.0 and T.max() <= 2500.0 and T.max() - T.min() > 1500.0
    assert np.allclose(Y.sum(axis=0), 1.0, rtol=1e-12) and Y.min() >= 0.0
    W = np.asarray(read_yaml_mechanism(os.path.join(GOLDEN, mech_file))["W"])
    off = rho / (p / (8314.46261815324 * T * (Y / W[:, None]).sum(axis=0))) - 1.0
    assert np.abs(off).max() > 0.01                               # the thermo density is not the reactor's
    # the oracle's rates conserve mass per state: sum_i RR_i = 0 to the rounding of the largest term
    assert np.all(np.isfinite(RR)) and np.abs(RR).max() > 0
    assert np.abs(RR.sum(axis=0)).max() < 1e-9 * np.abs(RR).max()


def test_zero_d_fixture():
    ref = json.load(open(os.path.join(GOLDEN, "zeroD_drm19.json")))
    T, Y = np.asarray(ref["T"]), np.asarray(ref["Y"])
    n = ref["n_steps"]
    assert ref["mechanism"] == "drm19.yaml" and ref["dt"] == 1e-6 and n <= 1000
    assert T.shape == (n + 1,) and Y.shape == (n + 1, 21) and T[0] == ref["T0"]
    assert T.max() - T[0] >= 500.0                                # ignition inside the window
    assert np.allclose(Y.sum(axis=1), 1.0, atol=1e-9) and np.allclose(Y[0], ref["Y0"])
