"""Non-orthogonal laplacians, the parts that run without a GPU: Mesh.nonorth_geometry, the restatement's exactness on
a quadratic and its committed accuracy bounds (tests/nonorth_reference.py, tests/golden/nonorth_bounds.json), and the
fvSchemes / fvSolution readers."""
import numpy as np
import pytest

import nonorth_reference as R


def test_geometry_identities():
    """k.n = 1 - n.d nonOrthDeltaCoeffs; 1 / (n.d) > 1 / |d| on the sheared box; coupled slots follow the same
    formulas and every other slot keeps its deltaCoeffs with k = 0"""
    for name in ("sheared-walls", "sheared-periodic", "refined"):
        m = R.get_mesh(name)
        dc, k, bdc, bk = m.nonorth_geometry()
        n = m.sf / m.mag_sf[:, None]
        nd = (n * m.mesh_distance).sum(axis=1)
        assert np.abs((k * n).sum(axis=1) - (1.0 - nd * dc)).max() < 8 * np.finfo(float).eps, name
        assert (dc >= m.delta_coeffs * (1 - 4 * np.finfo(float).eps)).all(), name
        sl = R.Slots(m)
        assert np.array_equal(bdc[~sl.coupled], m.boundary_arrays()[2][~sl.coupled]) and not bk[~sl.coupled].any()
        if name.startswith("sheared"):
            assert (dc > m.delta_coeffs * 1.01).all()
        if sl.coupled.any():
            bn = m.boundary_arrays()[0] / m.boundary_arrays()[1][:, None]
            bnd = (bn * m.boundary_delta()).sum(axis=1)
            c = sl.coupled
            assert np.abs((bk * bn).sum(axis=1) - (1.0 - bnd * bdc))[c].max() < 8 * np.finfo(float).eps
            assert np.abs(bk[c]).max() > 0.1


def test_axis_aligned_box_has_no_correction():
    from dfmi.mesh import hex_box
    m = hex_box(6, 5, 4, gradings=(1.0, 1.4, 1.0), periodic=(True, False, True))
    dc, k, bdc, bk = m.nonorth_geometry()
    assert np.abs(k).max() < 4 * np.finfo(float).eps and np.abs(bk).max() < 4 * np.finfo(float).eps
    assert np.abs(dc / m.delta_coeffs - 1).max() < 4 * np.finfo(float).eps
    assert np.abs(bdc / m.boundary_arrays()[2] - 1).max() < 4 * np.finfo(float).eps


def test_corrected_laplacian_is_exact_for_a_quadratic():
    """gamma tr(H) V in every cell of the periodic sheared box, to 4x the long-double restatement's committed
    deviation (the read-back mesh is affine only to the digits the writer keeps); the orthogonal form misses by more
    than 1e-2 on the same cells"""
    b = R.load_bounds()
    m = R.get_mesh("sheared-periodic-xyz")
    corr_ld, orth_ld = R.exactness_residual(m, R.LD)
    corr, orth = R.exactness_residual(m)
    print(f"corrected: long double {corr_ld:.3e} (committed {b['exactness_longdouble']:.3e}), fp64 {corr:.3e}; "
          f"orthogonal {orth:.3e}")
    assert corr_ld <= b["exactness_longdouble"] * (1 + 1e-6)
    assert corr <= 4 * b["exactness_longdouble"]
    assert orth > 1e-2 and orth_ld > 1e-2


def test_fp64_restatement_within_committed_bounds():
    """per mesh and field, on the state the GPU tests assemble (R.case_state). Where a field is nearly uniform its
    Gauss gradient is a cancellation residue and the figure is of order one (p everywhere; Y, diffAlphaD and he on
    the walled sheared boxes, whose corners lie far from the hot kernel); U is resolved everywhere"""
    b = R.load_bounds()
    assert set(b["reference_error"]) == set(R.MESHES)
    for name in R.MESHES:
        v = R.reference_error(R.get_mesh(name))
        assert set(v) == set(b["reference_error"][name]) == set(R.FIELDS)
        for f in R.FIELDS:
            print(f"{name:18s} {f:10s} {v[f]:.3e} (committed {b['reference_error'][name][f]:.3e}) -> GPU bound "
                  f"{R.gpu_bound(b, name, f):.3e}")
            c = b["reference_error"][name][f]
            if c > 1e-6:    # a cancellation residue against another: of order one, and no more reproducible than that
                assert np.isfinite(v[f]) and 1e-6 < v[f] < 10, (name, f)
            else:
                assert np.isfinite(v[f]) and v[f] <= c * (1 + 1e-6) + 1e-300, (name, f)
        assert b["reference_error"][name]["U"] < 1e-14, name


def test_nonorth_mesh_replaces_internal_and_coupled_delta_coeffs():
    m = R.get_mesh("sheared-periodic")
    m2 = R.nonorth_mesh(m)
    dc, _, bdc, _ = m.nonorth_geometry()
    assert np.array_equal(m2.delta_coeffs, dc) and np.array_equal(m2.boundary_arrays()[2], bdc)
    assert m2.delta_coeffs is not m.delta_coeffs and not np.array_equal(m.boundary_arrays()[2], bdc)


# ------------------------------------------------------------------------------------------------ readers
FV_SCHEMES = """FoamFile { version 2.0; format ascii; class dictionary; object fvSchemes; }
divSchemes
{
    default none;
    div(phi,U) Gauss linear;   // comment
    div(phi,K) Gauss limitedLinear 1;
}
laplacianSchemes
{
    %s
}
snGradSchemes { default corrected; }
"""


def _schemes(tmp_path, body):
    from dfmi.schemes import read_fv_schemes
    f = tmp_path / "fvSchemes"
    f.write_text(FV_SCHEMES % body)
    return read_fv_schemes(str(f))


def test_fv_schemes_reader(tmp_path):
    from dfmi.schemes import parse_laplacian
    got = _schemes(tmp_path, "default Gauss linear corrected;")
    assert got == {"div(phi,U)": "Gauss linear", "div(phi,K)": "Gauss limitedLinear 1", "laplacian": "corrected"}
    assert _schemes(tmp_path, "default Gauss linear uncorrected;")["laplacian"] == "uncorrected"
    assert "laplacian" not in _schemes(tmp_path, "default Gauss linear orthogonal;")
    assert _schemes(tmp_path, "default Gauss linear corrected; laplacian(muEff,U) Gauss linear corrected;")["laplacian"] == "corrected"
    assert _schemes(tmp_path, "default none; laplacian(muEff,U) Gauss linear corrected;")["laplacian"] == "corrected"
    for s, want in {"corrected": "corrected", "Gauss linear orthogonal": "orthogonal", "linear uncorrected": "uncorrected"}.items():
        assert parse_laplacian(s) == want
    for bad in ("default Gauss linear limited corrected 0.5;", "default Gauss linear limited 0.33;",
                "default Gauss linear corrected; laplacian(alphaEff,ha) Gauss linear uncorrected;",
                "default none; laplacian(muEff,U) Gauss linear corrected; laplacian(rhorAUf,p) Gauss linear orthogonal;",
                "default Gauss linear faceCorrected;", "default Gauss linear corrected 1;"):
        with pytest.raises(ValueError):
            _schemes(tmp_path, bad)
    with pytest.raises(ValueError, match="limited"):
        parse_laplacian("Gauss linear limited corrected 0.5")


def test_fv_solution_reader(tmp_path):
    from dfmi.schemes import read_fv_solution
    f = tmp_path / "fvSolution"
    txt = """solvers { p { solver PCG; tolerance 1e-6; } }
PIMPLE
{
    momentumPredictor yes;
    nOuterCorrectors %s;
    nCorrectors 2;   /* pressure correctors */
    nNonOrthogonalCorrectors %s;
}
"""
    f.write_text(txt % (1, 1))
    assert read_fv_solution(str(f)) == {"nCorrectors": 2, "nNonOrthogonalCorrectors": 1}
    f.write_text("PIMPLE { nCorrectors 3; }")
    assert read_fv_solution(str(f)) == {"nCorrectors": 3, "nNonOrthogonalCorrectors": 0}
    for outer, nno in ((2, 0), (1, -1), (1, "many")):
        f.write_text(txt % (outer, nno))
        with pytest.raises(ValueError):
            read_fv_solution(str(f))
    f.write_text("solvers { }")
    with pytest.raises(ValueError):
        read_fv_solution(str(f))


def test_golden_cases_keep_their_schemes():
    """the committed cases say `orthogonal`: the reader adds no laplacian entry for them"""
    import os
    from dfmi.schemes import read_fv_schemes
    for case in ("tgv2d", "tgv64", "flame1d"):
        assert "laplacian" not in read_fv_schemes(os.path.join(R.GOLDEN, case, "fvSchemes"))
