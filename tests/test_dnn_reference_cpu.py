"""The float64 reference of the DF-ODENet shape tests (dnn_reference.py) checked on the CPU, and proof that the
bound of test_gpu_dnn_shapes.py bites: each seeded defect, applied to the NumPy model at the shape table's own
shapes, must push err over 8 err(fp16 stand-in) + floor -- the largest bound the GPU test may use (its F <= 8).
The stand-in is a second fp16 implementation (torch's CPU half Linear and GELU, or NumPy with float32 accumulation
in reversed order): it differs from the reference as a correct kernel does, by summation order flipping last bits."""
import numpy as np
import pytest

import dnn_reference as R

F_MAX = 8.0


def _case(name):
    return next(c for c in R.CASES if c["name"] == name)


def test_reference_matches_torch_fp32_on_the_production_chain():
    """[11, 1600, 800, 400, 1], 8 nets: the reference against the torch fp32 CPU restatement test_gpu_dnn.py
    compares the kernels with, within that file's own tolerances (median 2e-3, max 2e-2)"""
    import torch
    S, C = 9, 384
    dims = [S + 2, 1600, 800, 400, 1]
    mods = R.dense_weights(S - 1, dims, seed=0)
    xmu, xstd, ymu, ystd = R.norms(S)
    react = R.mask_alternate(C, 150)
    T, p, rho, Y = R.make_inputs(S, C, react, seed=1)
    RR, _, _, got_react = R.reference(mods, T, p, rho, Y, xmu, xstd, ymu, ystd)
    assert np.array_equal(got_react, react)
    Yr = Y[:, react]
    bct = (Yr ** 0.1 - 1) * 10
    x = np.concatenate([T[react][None, :], np.full((1, react.sum()), 101325.0), bct], axis=0).T
    xt = torch.tensor((x - xmu) / xstd, dtype=torch.float32)
    yn = np.zeros((S - 1, react.sum()))
    for k, layers in enumerate(mods):
        h = xt
        for l, (W, b) in enumerate(layers):
            h = h @ torch.tensor(W).T + torch.tensor(b)
            if l < len(layers) - 1:
                h = torch.nn.functional.gelu(h)
        yn[k] = ((h[:, 0].double().numpy() * ystd[k] + ymu[k] + bct[k]) * 0.1 + 1) ** 10
    yn = yn / (yn.sum(axis=0) + Yr[S - 1])
    ref = np.zeros((S, C))
    ref[:S - 1, react] = (yn - Yr[:S - 1]) * rho[react] * (p[react] / 101325.0) / 1e-6
    assert np.all(RR[:, ~react] == 0.0) and np.all(RR[S - 1] == 0.0) and np.isfinite(RR).all()
    scale = np.abs(ref).max(axis=1, keepdims=True)[:S - 1]
    e = np.abs(RR[:S - 1] - ref[:S - 1])[:, react] / scale
    assert np.median(e) < 2e-3, np.median(e)
    assert e.max() < 2e-2, e.max()


def test_probe_columns_are_the_edges():
    assert R.probe_columns(528, tail_q=2)[:8] == [512, 527, 0, 15, 16, 256, 255, 511]
    assert R.probe_columns(8) == [7, 0]
    cols = R.probe_columns(600)
    for c in (0, 15, 16, 599, 256, 255, 512, 511, 128, 127, 64, 63, 576, 575):
        assert c in cols
    case = _case("pp-512-600-8")
    assert R.families(case) == ["dense", "probe0", "probe1", "probe2"]
    seen = [c for f in R.families(case)[1:] for c in R.case_weights(case, f)[1]]
    assert set(seen) == set(cols) and len(seen) == 24
    mods, probe = R.probe_weights(8, [11, 576, 528, 8, 1], layer=1, tail_q=2)
    for m, layers in enumerate(mods):
        W2, Wo = layers[2][0], layers[3][0]
        assert W2.shape == (8, 528) and np.count_nonzero(W2) == 8 and np.all(W2[:, probe[m]] == 1.0)
        assert np.count_nonzero(Wo) == 1 and Wo[0, 0] == 1.0


def _setup(case, family, rows=R.ROWS, C=R.C_SMALL, seed=3):
    S = case["S"]
    mods, probe = R.case_weights(case, family)
    norms = R.norms(S)
    react = R.mask_alternate(C, rows)
    fields = R.make_inputs(S, C, react, seed=seed)
    return mods, probe, norms, react, fields


def _judge(mods, norms, react, fields, hook=None, mods_mut=None, out_map=None):
    """(err of the defective model, the bound 8 err(stand-in) + floor)"""
    T, p, rho, Y = fields
    xmu, xstd, ymu, ystd = norms
    ref, _, out16, _ = R.reference(mods, T, p, rho, Y, xmu, xstd, ymu, ystd)
    x16 = R.normalised_input(T, Y, react, xmu, xstd)
    standin, _ = R.post_process(R.half_standin(x16, mods), T, p, rho, Y, react, ymu, ystd)
    e_std = R.err(standin, ref)
    assert e_std < 1e-2, e_std   # the input is well conditioned
    floor = R.ulp_floor(out16, ref, T, p, rho, Y, react, ymu, ystd)
    out_mut = R.net_outputs(x16, mods_mut or mods, hook)
    if out_map is not None:
        out_mut = out_map(out_mut)
    mut, _ = R.post_process(out_mut, T, p, rho, Y, react, ymu, ystd)
    e_mut = R.err(mut, ref)
    print(f"err(defect) {e_mut:.3e}  err(stand-in) {e_std:.3e}  floor {floor:.3e}")
    return e_mut, F_MAX * e_std + floor


def test_defect_k_block_dropped():
    """[128,129,136]: the fused last hidden layer (K = 129 padded to 160) loses its second 32-wide K block"""
    case = _case("ring-128-129-136")
    mods, probe, norms, react, fields = _setup(case, "probe0")

    def hook(m, l, h):
        if l == 1:
            h = h.copy(); h[:, 32:64] = 0.0
        return h
    e, bound = _judge(mods, norms, react, fields, hook)
    assert e > bound, (e, bound)


def test_defect_tail_strip_column_from_its_neighbour():
    """[576,528,8]: column 527, the last of the first tail strip, holds column 526's value"""
    case = _case("pp-576-528-8")
    mods, probe, norms, react, fields = _setup(case, "probe0")
    assert 527 in probe and 512 in probe

    def hook(m, l, h):
        if l == 1:
            h = h.copy(); h[:, 527] = h[:, 526]
        return h
    e, bound = _judge(mods, norms, react, fields, hook)
    assert e > bound, (e, bound)


def test_defect_probed_column_zeroed():
    """[512,600,8]: the last column of the ragged third tile written as zero"""
    case = _case("pp-512-600-8")
    mods, probe, norms, react, fields = _setup(case, "probe0")
    assert 599 in probe

    def hook(m, l, h):
        if l == 1:
            h = h.copy(); h[:, 599] = 0.0
        return h
    e, bound = _judge(mods, norms, react, fields, hook)
    assert e > bound, (e, bound)


@pytest.mark.parametrize("family", ["dense", "probe0"])
def test_defect_last_ragged_row_duplicated(family):
    """[96,8], 300 rows: row 299, the last of the ragged second row tile, holds row 298's activations"""
    case = _case("ring-96-8")
    mods, probe, norms, react, fields = _setup(case, family)

    def hook(m, l, h):
        if l == 1:
            h = h.copy(); h[299] = h[298]
        return h
    e, bound = _judge(mods, norms, react, fields, hook)
    assert e > bound, (e, bound)


def test_defect_padding_column_not_zero():
    """[37,100,8]: padding column 37 of the first layer's output (row stride 64) holds 1.0 and the next layer's
    weight behind it is not zero"""
    case = _case("ring-37-100-8")
    mods, probe, norms, react, fields = _setup(case, "dense")
    mods_mut = []
    for layers in mods:
        W1, b1 = layers[1]
        W1a = np.concatenate([W1, np.full((W1.shape[0], 1), 1.0 / np.sqrt(37.0), np.float32)], axis=1)
        mods_mut.append([layers[0], (W1a, b1)] + list(layers[2:]))

    def hook(m, l, h):
        if l == 0:
            h = np.concatenate([h, np.ones((h.shape[0], 1))], axis=1)
        return h
    e, bound = _judge(mods, norms, react, fields, hook, mods_mut=mods_mut)
    assert e > bound, (e, bound)


def test_defect_chunk_offsets_swapped():
    """the chunk-edge case (67,240 rows = 65,536 + 1,704): each chunk's results land at the other's offset"""
    S = R.CHUNK["S"]
    case = dict(S=S, hidden=R.CHUNK["hidden"])
    nx, ny, nz = R.CHUNK["box"]
    C = nx * ny * nz
    mods, _ = R.case_weights(case, "dense")
    norms = R.norms(S)
    react = np.ones(C, bool)
    fields = R.make_inputs(S, C, react, seed=3)
    swap = lambda out: np.concatenate([out[:, 65536:], out[:, :65536]], axis=1)
    e, bound = _judge(mods, norms, react, fields, out_map=swap)
    assert e > bound, (e, bound)
