"""The DF-ODENet GEMM dispatch (csrc/dnn.hip dnn_solve) at every shape edge the public ABI can reach: row counts
around the row tiles and the compaction blocks, a ragged second 65,536-row chunk, widths that are no multiple of
the tiles, every K the 3-buffer ring takes, the K == 64 rule on a hidden layer, every class of N % 256 on the
ping-pong kernel and its tail strips, the fused output layer over 8 to 400 columns, 2- and 8-layer nets, 63 nets.

Every case runs with dnn.tuned_gemm = 0 and 1 and asserts
  (a) Context.dnn_plan() equals the kinds written by hand in dnn_reference.CASES;
  (b) tuned 1 is bitwise equal to tuned 0 (the property dnn.hip documents);
  (c) RR is finite, and exactly 0 in non-reacting cells and for the inert species;
  (d) err(RR) against dnn_reference.reference (float64 accumulation, rounding where the kernels round) is at most
      F err(torch) + floor and below 2e-2, where err(torch) is the same figure for test_gpu_dnn._half_reference
      (torch's own fp16 Linear and GELU on the device) and floor is what one fp16 ulp of every net's output is
      worth in RR (dnn_reference.ulp_floor); F and the measured table are in DESIGN.md section 8;
  (e) dnn_infer() returns the mask's count.

There is one context per species count and mesh, kept for the whole file; every case REPLACES THE MODEL ON THE LIVE
CONTEXT, so the activation, partial-sum and weight buffers grow and shrink from case to case and hold the previous
case's bits (they are never cleared). Model replacement on a live context is thereby itself under test. Before each
case a poison model (_poison) leaves inf and NaN in every activation the case can touch, because the padded weight
columns are zero and would hide a finite stale value: a padding column that is not written as zero then shows as a
non-finite RR."""
import os

import numpy as np
import pytest

import dnn_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# err(gpu) <= F err(torch) + floor. Measured on the MI355X over every case of this file:
# err(gpu) stays below floor in all of them, so the ratio that F has to cover, (err(gpu) - floor) / err(torch), is 0
# everywhere. The raw err(gpu) / err(torch) is no yardstick: both figures are the largest single flipped last bit of
# a case, torch often flips none (err(torch) = 0 in 14 cases, 1e-8 in others), and the raw ratio is then unbounded
# -- the situation the floor term is there for. F is the smallest power of two that keeps the torch term at all.
F = 1.0

_CTX = {}


def _context(S, box=(10, 14, 15)):
    """the live context of (S, mesh): S = 9 with the Burke thermo table (Qdot is computed), any other S as a
    surrogate-only context (no thermo table: Qdot stays 0)"""
    key = (S, box)
    if key in _CTX:
        return _CTX[key]
    from dfmi.mesh import hex_box
    from dfmi.lib import Context
    from dfmi import case
    m = hex_box(*box)
    C = m.n_cells
    ctx = Context(0)
    hc = None
    if S == 9:
        from dfmi.mech import read_thermo_table, read_yaml_mechanism
        from chem_oracle import hf298_per_mass
        ym = read_yaml_mechanism(os.path.join(GOLDEN, "Burke2012_s9r23.yaml"))
        t = read_thermo_table(os.path.join(GOLDEN, "thermo_Burke2012_s9r23.txt"), ym["species"])
        assert ym["species"].index("N2") == S - 1
        case.setup_context(ctx, m, t, S - 1, 1e-6)
        hc = hf298_per_mass(t.nasa, t.W)
    else:
        pt = case.default_patch_types(m)
        rows, cols = m.proc_rows_cols()
        ctx.set_constant_values(C, C, m.n_faces, m.n_boundary_slots, m.n_patches, int(rows.size), m.patch_sizes, S, 1e6)
        ctx.set_cyclic_info(m.cyclic_neighbour())
        ctx.set_constant_indexes(m.owner, m.neighbour, rows, cols, 0)
        ctx.init_constant_fields_internal(m.sf, m.mag_sf, m.weight, m.delta_coeffs, m.volume, m.mesh_distance)
        bsf, bmag, bdc, bw, bfc = m.boundary_arrays()
        ctx.init_constant_fields_boundary(bsf, bmag, bdc, bw, bfc, pt["calculated"], pt["extrapolated"])
        ctx.set_inert_index(S - 1)
    _CTX[key] = (ctx, C, hc)
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx, _, _ in _CTX.values():
        ctx.close()
    _CTX.clear()


def _infer_both(ctx, C, S, fields, plan0, plan1, n_expected):
    """(a), (b), (c), (e); returns tuned 0's (RR, Qdot)"""
    for n, v in zip(("T", "p", "rho", "Y"), fields):
        ctx.set_field(n, v)
    T = fields[0]
    out = []
    for tuned, plan in ((0, plan0), (1, plan1)):
        ctx.set_option("dnn.tuned_gemm", tuned)
        assert ctx.dnn_plan() == plan, (tuned, ctx.dnn_plan(), plan)                       # (a)
        assert ctx.dnn_infer() == n_expected                                              # (e)
        RR, Q = ctx.get_field("RR", (S, C)), ctx.get_field("Qdot", (C,))
        assert np.isfinite(RR).all() and np.isfinite(Q).all(), tuned                      # (c)
        assert np.all(RR[:, T < R.T_REACT] == 0.0) and np.all(RR[S - 1] == 0.0), tuned
        assert np.all(Q[T < R.T_REACT] == 0.0), tuned
        out.append((RR, Q))
    assert np.array_equal(out[1][0], out[0][0]), np.abs(out[1][0] - out[0][0]).max()      # (b)
    assert np.array_equal(out[1][1], out[0][1])
    return out[0]


def _poison(ctx, C, S, fields, width):
    """fill both activation buffers with non-finite fp16 values over everything the next model can touch: a model
    [S + 2, width, width, 8, 1] of zero weights and infinite biases, run on the same rows. Its first layer stores
    inf and its second NaN (0 x inf) in every column of `width`-wide rows with no padding (width % 64 == 0), so a
    padding column the next model fails to write as zero, which its zero-padded weights would otherwise hide,
    reaches that model's MFMAs as 0 x NaN = NaN."""
    assert width % 64 == 0
    dims = [S + 2, width, width, 8, 1]
    layers = [(np.zeros((dims[l + 1], dims[l]), np.float32), np.full(dims[l + 1], np.inf, np.float32))
              for l in range(len(dims) - 1)]
    ctx.dnn_set_model(dims, [layers] * (S - 1), *R.norms(S))
    for n, v in zip(("T", "p", "rho", "Y"), fields):
        ctx.set_field(n, v)
    ctx.dnn_infer()
    react = fields[0] >= R.T_REACT
    if react.any():
        assert not np.isfinite(ctx.get_field("RR", (S, C))[:S - 1, react]).any()


def _check(label, S, box, dims, mods, react, plan0, plan1, seed=3, replace_model=True):
    from test_gpu_dnn import _half_reference
    ctx, C, hc = _context(S, box)
    xmu, xstd, ymu, ystd = R.norms(S)
    fields = R.make_inputs(S, C, react, seed=seed)
    T, p, rho, Y = fields
    n = int(react.sum())
    if replace_model:
        _poison(ctx, C, S, fields, (max(dims[1:-1]) + 63) // 64 * 64)
        ctx.dnn_set_model(dims, mods, xmu, xstd, ymu, ystd)
    RR, Q = _infer_both(ctx, C, S, fields, plan0, plan1, n)
    if n == 0:
        assert not RR.any() and not Q.any()
        return
    ref, qref, out16, got = R.reference(mods, T, p, rho, Y, xmu, xstd, ymu, ystd, hc)
    assert np.array_equal(got, react)
    torch_rr = _half_reference(mods, T, p, rho, Y, xmu, xstd, ymu, ystd)
    e_gpu, e_torch = R.err(RR, ref), R.err(torch_rr, ref)
    floor = R.ulp_floor(out16, ref, T, p, rho, Y, react, ymu, ystd)
    print(f"DNNSHAPE {label} n={n} err_gpu={e_gpu:.3e} err_torch={e_torch:.3e} floor={floor:.3e}")
    assert e_torch < 1e-2, e_torch   # the reference's own condition: the input is well conditioned
    assert e_gpu <= F * e_torch + floor, (e_gpu, e_torch, floor)                          # (d)
    assert e_gpu < 2e-2, e_gpu
    if hc is not None:   # Qdot = -sum hc RR of the library's own RR, in species order (bitwise), and near the reference's
        from chem_oracle import heat_release
        assert np.array_equal(Q, heat_release(hc, RR))
        assert np.abs(Q - qref).max() <= (F * e_torch + floor) * (np.abs(hc[:S - 1]) * np.abs(ref[:S - 1]).max(axis=1)).sum()
    else:
        assert not Q.any()


FAMILIES = ("dense", "probe0")   # the row and chunk cases probe an 8-wide layer: one page holds its edge columns


# ---- rows and compaction: [11, 64, 32, 8, 1] on 2,100 cells (three 1,024-cell compaction blocks) -------------------
_ROW_MASKS = [(f"{pat}-{n}", fn, n) for n in R.ROW_COUNTS
              for pat, fn in (("first", R.mask_first), ("last", R.mask_last), ("alternate", R.mask_alternate))]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("label,fn,n", _ROW_MASKS, ids=[m[0] for m in _ROW_MASKS])
def test_row_counts_and_compaction(label, fn, n, family):
    """n reacting cells as the first n, the last n and every other cell: 0, 1, and one either side of 64 (a
    k_dnn_output group), 128 (the input kernel's row tile), 256 (the row tile) and 512; for n = 0 the call
    succeeds with RR and Qdot all zero"""
    case = dict(R.ROWS_DIMS)
    mods, _ = R.case_weights(case, family)
    _check(f"rows-{label}-{family}", 9, (10, 14, 15), R.case_dims(case), mods, fn(R.C_SMALL, n), case["plan0"],
           case["plan1"])


@pytest.mark.parametrize("family", FAMILIES)
def test_cells_either_side_of_a_compaction_block(family):
    """exactly cells 1023 and 1024 react: the last cell of one compaction block and the first of the next"""
    case = dict(R.ROWS_DIMS)
    mods, _ = R.case_weights(case, family)
    _check(f"rows-1023-1024-{family}", 9, (10, 14, 15), R.case_dims(case), mods, R.mask_cells(R.C_SMALL, (1023, 1024)),
           case["plan0"], case["plan1"])


# ---- chunk edge: 67,240 reacting rows = 65,536 + 1,704 -------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_ragged_second_chunk_then_five_rows_in_stale_buffers(family):
    """all 67,240 cells of hex_box(41, 41, 40) react: a full chunk and a ragged one of 1,704 rows; then 5 reacting
    cells on the same context and model, whose rows sit in the large buffers among the first call's data"""
    case = dict(S=R.CHUNK["S"], hidden=R.CHUNK["hidden"])
    box = R.CHUNK["box"]
    C = box[0] * box[1] * box[2]
    mods, _ = R.case_weights(case, family)
    dims = R.case_dims(case)
    _check(f"chunk-all-{family}", 9, box, dims, mods, np.ones(C, bool), R.CHUNK["plan0"], R.CHUNK["plan1"])
    five = R.mask_cells(C, (0, 1023, 1024, 65536, C - 1))
    _check(f"chunk-five-{family}", 9, box, dims, mods, five, R.CHUNK["plan0"], R.CHUNK["plan1"], seed=4,
           replace_model=False)


# ---- the column structure: 300 reacting rows (one full 256-row tile and 44 ragged rows) ----------------------------
_SHAPES = [(c, f) for c in R.CASES for f in R.families(c)]


@pytest.mark.parametrize("case,family", _SHAPES, ids=[f"{c['name']}-{f}" for c, f in _SHAPES])
def test_layer_shapes(case, family):
    """dnn_reference.CASES: the generic ring and its padding, the input kernel, the ping-pong kernel with and without
    tail strips, the fused output layer on both kernels; every other cell of the first 600 reacts"""
    mods, _ = R.case_weights(case, family)
    _check(f"{case['name']}-{family}", case["S"], (10, 14, 15), R.case_dims(case), mods,
           R.mask_alternate(R.C_SMALL, R.ROWS), case["plan0"], case["plan1"])


# ---- dfmi_dnn_load_model: the header's implied size is checked against the file before anything is sized from it ---
def test_load_model_refuses_a_header_larger_than_its_file(tmp_path):
    """a 100-byte file whose header claims 63 nets of [65536, 65536, 1] (1 TiB of parameters), and a valid file
    cut by one byte: both fail with the truncated-file message and nothing else"""
    import struct
    from dfmi.lib import DfmiError
    from dfmi.dnn_checkpoint import write_packed
    ctx, _, _ = _context(9)
    head = b"DFMIDNN1" + struct.pack("<ii", 63, 2) + struct.pack("<iii", 65536, 65536, 1)
    huge = tmp_path / "huge.dfmidnn"
    huge.write_bytes(head + bytes(100 - len(head)))
    assert huge.stat().st_size == 100
    with pytest.raises(DfmiError, match="truncated DF-ODENet model file"):
        ctx.dnn_load_model(huge)
    dims = [11, 32, 8, 1]
    xmu, xstd, ymu, ystd = R.norms(9)
    whole = tmp_path / "whole.dfmidnn"
    write_packed(str(whole), {"dims": dims, "params": R.dense_weights(8, dims), "x_mu": xmu, "x_std": xstd,
                              "y_mu": ymu, "y_std": ystd})
    ctx.dnn_load_model(whole)   # the uncut file loads
    cut = tmp_path / "cut.dfmidnn"
    cut.write_bytes(whole.read_bytes()[:-1])
    with pytest.raises(DfmiError, match="truncated DF-ODENet model file"):
        ctx.dnn_load_model(cut)
