"""The fp64 sequential oracle's thermo point (oracle.thermo_points) against the extended-precision reference
(tests/thermo_reference.py) on every state class, and the reference against itself. Runs without a GPU.

The maxima measured here are the numbers the GPU tolerances of test_gpu_thermo_points.py are derived from:
tests/golden/thermo_point_bounds.json holds them (written by `python tests/thermo_reference.py --measure`), and
the oracle must stay within that file.
"""
import numpy as np
import pytest

import thermo_reference as R

LD = R.LD


@pytest.fixture(scope="module")
def measured():
    return R.measure()


@pytest.fixture(scope="module")
def bounds():
    return R.load_bounds()


def test_oracle_within_committed_bounds(measured, bounds):
    assert set(measured) == set(bounds["tables"]) == set(R.cpu_tables())
    bad = []
    for name, per_cls in measured.items():
        for cls, per_q in per_cls.items():
            for q, v in per_q.items():
                print(f"{name:12s} {cls:10s} {q:11s} {v:.3e}  (committed class max {bounds['classes'][cls][q]:.3e})")
                if not (np.isfinite(v) and v <= bounds["classes"][cls][q]):
                    bad.append((name, cls, q, v))
    assert not bad, bad


def test_committed_class_maxima_are_the_tables_maxima(bounds):
    assert bounds["classes"] == R.class_maxima(bounds["tables"])


def test_gpu_bounds_stay_within_stated_parity(bounds):
    """4x the oracle's maximum (floored at 1e-13) must not exceed DESIGN's 1e-12 for any class and quantity;
    rhoD where kappa is large is the stated exception (held to a constant times kappa 2^-52)"""
    for cls in R.CLASSES:
        for q in R.QUANTITIES:
            if q in ("rhoD_kappa", "rhoD_dominant"):
                continue
            assert 1e-13 <= R.gpu_bound(bounds, cls, q) <= 1e-12, (cls, q, R.gpu_bound(bounds, cls, q))


def test_tables():
    g = R.mech_table("gri53")
    t53 = R.gri_table(53)
    for a in ("W", "nasa", "visc", "cond", "bdiff"):
        assert np.array_equal(getattr(t53, a), getattr(g, a)), a
    t64 = R.gri_table(64)
    assert t64.S == 64 and t64.W[-1] == g.W[-1]
    assert np.array_equal(t64.nasa[52], g.nasa[0]) and np.array_equal(t64.nasa[62], g.nasa[10])
    assert np.array_equal(t64.bdiff[52, 0], g.bdiff[0, 0])          # a species and its copy: the self-diffusion fit
    for S in (2, 3, 8, 16, 17, 33, 64):
        t = R.gri_table(S)
        assert t.S == S and R.is_symmetric(t)
    for name in ("es80", "burke9"):
        assert R.is_symmetric(R.mech_table(name))
    for S in (8, 9, 18, 64):
        n = R.nonsymmetric(R.gri_table(S))
        assert not R.is_symmetric(n)
        assert 1 <= int((n.bdiff != n.bdiff.transpose(1, 0, 2)).any(axis=2).sum()) // 2 <= 5
    assert list(R.distinct_tmid(g)) == [1000.0, 5000.0] and list(R.switching_tmid(g)) == [1000.0]


@pytest.mark.parametrize("name", ["burke9", "gri16", "gri64"])
def test_state_classes(name):
    t = R.cpu_tables()[name]
    tms = R.distinct_tmid(t)
    for cls in R.CLASSES:
        st = R.states(t, cls)
        assert 0 < st.n <= 400 and st.Y.shape == (t.S, st.n)
        assert np.allclose(st.Y.sum(axis=0), 1.0, rtol=0, atol=1e-14) and (st.Y >= 0).all()
        again = R.states(t, cls)
        assert np.array_equal(st.Y, again.Y) and np.array_equal(st.T, again.T) and np.array_equal(st.he, again.he)
    assert (R.states(t, "zeros").Y == 0.0).sum(axis=0).min() == t.S // 2
    X, _ = R.composition(t, R.states(t, "near_pure").Y)
    top = np.asarray(1 - X.max(axis=0), dtype=np.float64)
    assert np.allclose(np.sort(np.unique(np.round(np.log10(top)))), [-9, -6, -3])
    sw = R.states(t, "switch_T")
    for tm in tms:
        for T in (tm, np.nextafter(tm, 0), np.nextafter(tm, 1e9)):
            assert (sw.T == T).any()
    jp = R.states(t, "jump")
    alltm, lo, hi = R.one_sided_h(t, jp.Y)
    i = np.searchsorted(alltm, jp.tmid)
    k = np.arange(jp.n)
    inside = (jp.he > np.minimum(lo[i, k], hi[i, k])) & (jp.he < np.maximum(lo[i, k], hi[i, k]))
    assert inside.sum() >= 3 * 6          # the targets placed inside the discontinuity itself


def test_oracle_in_jumps():
    """T(he) is undefined inside a jump: the oracle must end within 8e-6 T_mid of the switch with finite outputs
    (everything else is compared at the T it returned, in test_oracle_within_committed_bounds)"""
    for name, t in R.cpu_tables().items():
        st = R.states(t, "jump")
        e, ref, got = R.oracle_errors(t, st)
        for q in ("T", "he", "psi", "rho", "mu", "alpha", "rhoD", "hai"):
            assert np.isfinite(got[q]).all(), (name, q)
        assert (np.abs(got["T"] - st.tmid) <= R.JUMP_STOP * st.tmid).all(), name
        assert np.array_equal(got["he"], st.he)
        res = np.abs(LD(1) * got["he"] - ref["he_from_T"]) / np.maximum(np.abs(ref["he"]), LD(R.R_GAS) * ref["T"] / ref["Wm"])
        assert (np.asarray(res, dtype=np.float64) <= R.jump_he_slack(t, st, ref)).all(), name


def test_stray_newton_state():
    """the one newton state of the tested tables whose plain Newton iteration leaves the fits' range and ends on the
    upper root of he = h(T): start 300 K, target near the top of the range. The oracle follows it there."""
    t = R.gri_table(32)
    st = R.states(t, "newton")
    e, ref, got = R.oracle_errors(t, st)
    k = np.where(ref["stray"])[0]
    assert k.size == 1 and st.T[k[0]] == 300.0
    low = float(R.solve_T(t, st.Y[:, k], st.he[k], [1000.0])[0])
    assert 3400.0 < low < 3500.0 and 7000.0 < float(ref["T"][k[0]]) < 9000.0
    assert e["T"][k[0]] < 1e-13
    for name in ("burke9", "gri16", "gri64"):
        tt = R.cpu_tables()[name]
        assert not R.reference_for(tt, R.states(tt, "newton"))["stray"].any()


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.fixture(scope="module")
def t9():
    return R.mech_table("burke9")


def test_reference_he_is_sum_of_species_enthalpies(t9):
    st = R.states(t9, "broad")
    r = R.evaluate(t9, st.p, st.Y, T=st.T)
    s = (LD(1) * st.Y * r["hai"]).sum(axis=0)
    scale = (np.abs(LD(1) * st.Y * r["hai"])).sum(axis=0)
    assert float((np.abs(s - r["he"]) / scale).max()) < 64 * np.finfo(LD).eps


def test_reference_pure_species_viscosity_is_the_fit(t9):
    st = R.states(t9, "pure")
    r = R.evaluate(t9, st.p, st.Y, T=st.T)
    for i in range(t9.S):
        assert st.Y[i, i] == 1.0
        assert abs(float(r["mu"][i] / r["mu_i"][i, i] - 1)) < 64 * np.finfo(LD).eps
        assert r["rhoD"][i, i] == 0.0
        assert np.isfinite(np.asarray(np.delete(r["rhoD"][:, i], i), dtype=np.float64)).all()


def test_reference_invariant_under_species_permutation():
    from dfmi.mech import ThermoTable
    t = R.nonsymmetric(R.gri_table(9))
    st = R.states(t, "broad")
    perm = np.random.default_rng(3).permutation(t.S)
    tp = ThermoTable([t.species[i] for i in perm], t.W[perm], t.nasa[perm], t.visc[perm], t.cond[perm],
                     t.bdiff[np.ix_(perm, perm)])
    a = R.evaluate(t, st.p, st.Y, T=st.T)
    b = R.evaluate(tp, st.p, st.Y[perm], T=st.T)
    tol = 256 * np.finfo(LD).eps
    assert float(np.abs(b["rhoD"] / a["rhoD"][perm] - 1).max()) < tol
    assert float(np.abs(b["hai"] - a["hai"][perm]).max()) == 0.0
    for q in ("he", "mu", "alpha", "psi"):
        assert float(np.abs(b[q] / a[q] - 1).max()) < tol, q


def test_reference_round_trip(t9):
    """from he then from T gives he back; from T then from he gives T back, whatever the start"""
    st = R.states(t9, "newton")
    r = R.evaluate(t9, st.p, st.Y, he=st.he, T0=st.T)
    back = R.evaluate(t9, st.p, st.Y, T=r["T"])
    scale = np.maximum(np.abs(r["he"]), LD(R.R_GAS) * r["T"] / r["Wm"])
    assert float((np.abs(back["he"] - r["he"]) / scale).max()) < 64 * np.finfo(LD).eps
    n5 = st.n // 5                      # the five starts of one target agree
    T = np.asarray(r["T"]).reshape(5, n5)
    assert float(np.abs(T / T[0] - 1).max()) < 64 * np.finfo(LD).eps


def test_error_measure_is_per_element(t9):
    """one wrong species in one state must show at its own size, whatever the rest of the field is"""
    st = R.states(t9, "broad")
    ref = R.evaluate(t9, st.p, st.Y, T=st.T)
    got = {q: np.asarray(ref[q], dtype=np.float64).copy() for q in ("T", "he", "psi", "rho", "mu", "alpha", "rhoD", "hai")}
    k = int(np.argmin(np.abs(got["hai"][3])))          # where species 3's enthalpy is smallest: judged by R T / W there
    got["hai"][3, k] += 1e-7 * max(abs(got["hai"][3, k]), R.R_GAS * st.T[k] / t9.W[3])
    got["rhoD"][5, 7] *= 1 + 1e-9
    e = R.errors(t9, got, ref)
    assert 0.9e-7 < e["hai"][3, k] < 1.1e-7
    assert np.delete(e["hai"].ravel(), 3 * st.n + k).max() < 1e-15
    assert 0.9e-9 < e["rhoD"][5, 7] < 1.1e-9
    assert np.delete(e["rhoD"].ravel(), 5 * st.n + 7).max() < 1e-15
