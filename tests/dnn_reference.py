"""A plain NumPy float64 restatement of the DF-ODENet inference (csrc/dnn.hip), the reference of
test_gpu_dnn_shapes.py and test_dnn_reference_cpu.py. It rounds where the kernels round and nowhere else:

  normalised input        double -> float32 -> fp16                      (k_dnn_input)
  weights, biases         float32 -> fp16                                (dnn_upload)
  Linear                  float64-accumulated dot + bias -> fp16         (the GEMM epilogue's first rounding)
  GELU                    exact erf in float64 -> fp16                   (the epilogue's second rounding)
  the net's output        float64 dot + bias -> fp16                     (k_dnn_output)
  post-processing         double, in k_dnn_output's operation order      (Box-Cox inverse, renormalisation over
                                                                          the species in order, RR, Qdot)

The kernels accumulate in fp32 (MFMA) in tile order and approximate erf to 1.5e-7; both can flip the last fp16
bit of an activation, which is the error test_gpu_dnn_shapes.py bounds. Helper module, not a conftest.

Also here: the seeded input maker (T, p, rho, Y for S species and C cells with a chosen reacting mask), the dense
and probe weight families, the probed columns of a width, err() and the one-ulp floor of the bound."""
import math

import numpy as np

try:
    from scipy.special import erf as _erf
except ImportError:   # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])

T_REACT = 610.0
DT_INFER = 1e-6


def f16(a):
    """round to fp16 (nearest even), kept as float64"""
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def norms(S):
    """normalisation constants for an S-species surrogate: inputs O(1) for T in [300, 2500] K and Box-Cox
    transformed mass fractions in [-8.5, 0]; outputs scaled as the H2 nets' are (O(1e-2))"""
    xmu = np.full(S + 2, -4.0); xstd = np.full(S + 2, 2.5)
    xmu[0], xstd[0], xmu[1], xstd[1] = 1300.0, 400.0, 101325.0, 1.0
    return xmu, xstd, np.zeros(S - 1), np.full(S - 1, 0.01)


def make_inputs(S, C, react, seed=0):
    """T, p, rho [C] and Y [S, C]: cells of the boolean mask `react` at 800-2300 K, the others at 300-600 K
    (T_REACT = 610 K decides); mass fractions gamma-distributed and normalised, none zero"""
    react = np.asarray(react, dtype=bool)
    assert react.shape == (C,)
    rng = np.random.default_rng(seed)
    Y = rng.gamma(0.3, 1.0, (S, C)) + 1e-8
    Y /= Y.sum(axis=0)
    T = np.where(react, 800.0 + 1500.0 * rng.random(C), 300.0 + 300.0 * rng.random(C))
    p = 101325.0 * (1 + 0.05 * rng.standard_normal(C))
    rho = p / (300.0 * T)
    return T, p, rho, Y


def mask_first(C, n):
    m = np.zeros(C, bool); m[:n] = True
    return m


def mask_last(C, n):
    m = np.zeros(C, bool); m[C - n:] = True
    return m


def mask_alternate(C, n):
    """every other cell from cell 1 on, n of them"""
    m = np.zeros(C, bool); m[1:2 * n:2] = True
    assert int(m.sum()) == n
    return m


def mask_cells(C, cells):
    m = np.zeros(C, bool); m[list(cells)] = True
    return m


def dense_weights(n_modules, dims, seed=0):
    from dfmi.dnn_model import seeded_weights
    return seeded_weights(n_modules=n_modules, dims=list(dims), seed=seed)


def probe_columns(N, tail_q=None):
    """the edge columns of an N-wide layer, the sharpest first: for a tail-strip layer
    (N = 256 q + t) the strips' first columns, the last column of the first strip and the first of the second;
    then N - 1, 0, 15, 16, and every multiple of 256, 128 and 64 below N with the column before it"""
    cols = []
    if tail_q is not None:
        cols += [256 * tail_q, 256 * tail_q + 15, 256 * tail_q + 16]
    cols += [N - 1, 0, 15, 16]
    for step in (256, 128, 64):
        for c in range(step, N, step):
            cols += [c, c - 1]
    out = []
    for c in cols:
        if 0 <= c < N and c not in out:
            out.append(c)
    return out


def probe_weights(n_modules, dims, layer=None, seed=0, tail_q=None, page=0):
    """dense hidden layers up to hidden layer `layer` (index into dims[1:-1]; default the last hidden layer), whose
    column probe[m] net m carries undiluted to its output: every later hidden layer copies one column (the probed
    one, then column 0) into all its rows before its bias and GELU, and the output layer is one-hot (at the probed
    column, or column 0 behind a copying layer). A single wrong column of the probed layer then shows at full size
    in one net's RR instead of at 1/sqrt(N). With more edge columns than nets, `page` p takes the p-th n_modules of
    them (the last page wraps round to the first columns). Returns (mods, probe)."""
    L = len(dims) - 1
    t = L - 2 if layer is None else layer       # Linear layer index whose output is probed
    assert 0 <= t <= L - 2
    mods = dense_weights(n_modules, dims, seed)
    cols = probe_columns(dims[t + 1], tail_q)
    assert 0 <= page * n_modules < len(cols)
    probe = [cols[(page * n_modules + m) % len(cols)] for m in range(n_modules)]
    for m, layers in enumerate(mods):
        col = probe[m]
        for l in range(t + 1, L):
            W, b = layers[l]
            W = np.zeros_like(W)
            W[:, col] = 1.0
            layers[l] = (W, b)
            col = 0
    return mods, probe


def normalised_input(T, Y, react, xmu, xstd):
    """[n, S + 2] fp16-rounded rows of the reacting cells in cell order (k_dnn_input; p enters as 101325)"""
    Yr = Y[:, react]
    bct = (Yr ** 0.1 - 1.0) * 10.0
    x = np.concatenate([T[react][None, :], np.full((1, Yr.shape[1]), 101325.0), bct], axis=0).T
    x = (x - np.asarray(xmu)) / np.asarray(xstd)
    return x.astype(np.float32).astype(np.float16).astype(np.float64)


def gelu(v):
    return 0.5 * v * (1.0 + _erf(v * 0.7071067811865476))


def net_outputs(x16, mods, hook=None):
    """fp16 output [n_modules, n] of every net for the fp16 input rows x16 (float64 holding fp16 values).
    hook(m, l, h) -> h may alter hidden layer l's fp16 activations [n, width] of net m (the mutation checks)."""
    out = np.zeros((len(mods), x16.shape[0]))
    for m, layers in enumerate(mods):
        h = x16
        for l, (W, b) in enumerate(layers):
            z = f16(h @ f16(W).T + f16(b))
            if l < len(layers) - 1:
                h = f16(gelu(z))
                if hook is not None:
                    h = hook(m, l, h)
            else:
                out[m] = z[:, 0]
    return out


def post_process(out16, T, p, rho, Y, react, ymu, ystd, hc=None, dt=DT_INFER):
    """k_dnn_output in double: RR [S, C] (0 for non-reacting cells and the inert species) and Qdot [C]
    (-sum hc RR in species order where the formation enthalpies hc [S] are given, else 0)"""
    S, C = Y.shape
    Yr = Y[:, react]
    yn = np.zeros((S - 1, Yr.shape[1]))
    for m in range(S - 1):
        ybct = (Yr[m] ** 0.1 - 1.0) * 10.0
        v = out16[m] * ystd[m] + ymu[m] + ybct
        yn[m] = (v * 0.1 + 1.0) ** 10.0
    tot = np.zeros(Yr.shape[1])
    for m in range(S - 1):
        tot = tot + yn[m]
    tot = tot + Yr[S - 1]
    RR = np.zeros((S, C))
    rr = (yn / tot - Yr[:S - 1]) * rho[react] * (p[react] / 101325.0) / dt
    RR[:S - 1, react] = rr
    Q = np.zeros(C)
    if hc is not None:
        q = np.zeros(Yr.shape[1])
        for m in range(S - 1):
            q = q - hc[m] * rr[m]
        Q[react] = q
    return RR, Q


def reference(mods, T, p, rho, Y, xmu, xstd, ymu, ystd, hc=None, Tr=T_REACT, dt=DT_INFER, hook=None):
    """(RR, Qdot, out16, react) of the whole inference"""
    react = T >= Tr
    x16 = normalised_input(T, Y, react, xmu, xstd)
    out16 = net_outputs(x16, mods, hook)
    RR, Q = post_process(out16, T, p, rho, Y, react, ymu, ystd, hc, dt)
    return RR, Q, out16, react


def err(RR, ref):
    """max over the non-inert species of max |RR - ref| over that species' max |ref|"""
    S = ref.shape[0]
    scale = np.abs(ref[:S - 1]).max(axis=1)
    scale = np.where(scale > 0, scale, 1.0)
    return float((np.abs(RR[:S - 1] - ref[:S - 1]).max(axis=1) / scale).max()) if ref.shape[1] else 0.0


def ulp_floor(out16, ref, T, p, rho, Y, react, ymu, ystd, dt=DT_INFER):
    """err() of the RR change when every net's fp16 output moves by one fp16 ulp (either way) through
    post_process: what one last-bit difference in the nets' outputs is worth in RR"""
    ulp = np.spacing(np.abs(out16).astype(np.float16)).astype(np.float64)
    worst = 0.0
    for sgn in (1.0, -1.0):
        RR1, _ = post_process(out16 + sgn * ulp, T, p, rho, Y, react, ymu, ystd, None, dt)
        worst = max(worst, err(RR1, ref))
    return worst


def half_standin(x16, mods):
    """a second fp16 implementation of net_outputs for the CPU checks: torch's CPU half Linear and GELU where this
    build has them, else NumPy with float32 accumulation in reversed K order"""
    try:
        import torch
        with torch.no_grad():
            xt = torch.tensor(x16, dtype=torch.float64).to(torch.float16)
            out = np.zeros((len(mods), x16.shape[0]))
            for m, layers in enumerate(mods):
                h = xt
                for l, (W, b) in enumerate(layers):
                    h = torch.nn.functional.linear(h, torch.tensor(W).to(torch.float16), torch.tensor(b).to(torch.float16))
                    if l < len(layers) - 1:
                        h = torch.nn.functional.gelu(h)
                out[m] = h[:, 0].to(torch.float64).numpy()
        return out
    except (ImportError, RuntimeError):
        out = np.zeros((len(mods), x16.shape[0]))
        for m, layers in enumerate(mods):
            h = x16.astype(np.float32)
            for l, (W, b) in enumerate(layers):
                W16 = W.astype(np.float16).astype(np.float32)
                acc = np.zeros((h.shape[0], W.shape[0]), np.float32)
                for k in range(W.shape[1] - 1, -1, -1):
                    acc += h[:, k:k + 1] * W16[:, k][None, :]
                z = (acc + b.astype(np.float16).astype(np.float32)).astype(np.float16).astype(np.float64)
                if l < len(layers) - 1:
                    h = gelu(z).astype(np.float16).astype(np.float32)
                else:
                    out[m] = z[:, 0]
        return out


# ---- the shape cases of test_gpu_dnn_shapes.py (and the shapes test_dnn_reference_cpu.py mutates) ----------------
# name, S, hidden widths, the plan (dfmi_dnn_plan kinds per hidden-layer GEMM) for dnn.tuned_gemm = 0 and 1 WRITTEN
# BY HAND from the rules in dnn.hip's comments (never recomputed from the predicate), the hidden layer whose columns
# the probe family probes (None: the last hidden layer) and q of a tail-strip layer (N = 256 q + t).
C_SMALL = 2100            # hex_box(10, 14, 15): three 1024-cell compaction blocks
ROWS = 300                # one full 256-row tile and 44 ragged rows
ROW_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
ROWS_DIMS = dict(S=9, hidden=[64, 32, 8], plan0=[0, 0, 4], plan1=[0, 1, 4])
CHUNK = dict(S=9, hidden=[32, 8], plan0=[0, 4], plan1=[0, 4], box=(41, 41, 40))   # 65,536 + 1,704 rows
CASES = [
    # generic ring and padding
    dict(name="ring-37-100-8", S=9, hidden=[37, 100, 8], plan0=[0, 0, 4], plan1=[0, 1, 4]),
    dict(name="ring-128-129-136", S=9, hidden=[128, 129, 136], plan0=[0, 0, 4], plan1=[0, 0, 4]),
    dict(name="ring-64-64-8", S=9, hidden=[64, 64, 8], plan0=[0, 0, 4], plan1=[0, 1, 4]),
    dict(name="ring-96-8", S=9, hidden=[96, 8], plan0=[0, 4], plan1=[0, 4]),
    dict(name="ring-8", S=9, hidden=[8], plan0=[4], plan1=[4]),
    dict(name="ring-136", S=9, hidden=[136], plan0=[4], plan1=[4]),
    dict(name="ring-72", S=9, hidden=[72], plan0=[4], plan1=[4]),
    dict(name="ring-400", S=9, hidden=[400], plan0=[4], plan1=[4]),
    dict(name="ring-8layers", S=9, hidden=[32, 32, 32, 32, 32, 32, 8], plan0=[0, 0, 0, 0, 0, 0, 4],
         plan1=[0, 0, 0, 0, 0, 0, 4]),
    dict(name="ring-63nets-40-8", S=64, hidden=[40, 8], plan0=[0, 4], plan1=[0, 4], probe_layer=0),
    # input kernel
    dict(name="in-35-200-8", S=33, hidden=[200, 8], plan0=[0, 4], plan1=[1, 4], probe_layer=0),
    dict(name="in-64-136-8", S=62, hidden=[136, 8], plan0=[0, 4], plan1=[1, 4], probe_layer=0),
    # ping-pong and tail strips: the middle layer is the one under test
    dict(name="pp-512-512-8", S=9, hidden=[512, 512, 8], plan0=[0, 0, 4], plan1=[0, 2, 5], probe_layer=1),
    dict(name="pp-576-528-8", S=9, hidden=[576, 528, 8], plan0=[0, 0, 4], plan1=[0, 3, 5], probe_layer=1, tail_q=2),
    dict(name="pp-520-544-8", S=9, hidden=[520, 544, 8], plan0=[0, 0, 4], plan1=[0, 3, 5], probe_layer=1, tail_q=2),
    dict(name="pp-512-784-8", S=9, hidden=[512, 784, 8], plan0=[0, 0, 4], plan1=[0, 3, 5], probe_layer=1, tail_q=3),
    dict(name="pp-512-552-8", S=9, hidden=[512, 552, 8], plan0=[0, 0, 4], plan1=[0, 2, 5], probe_layer=1),
    dict(name="pp-512-600-8", S=9, hidden=[512, 600, 8], plan0=[0, 0, 4], plan1=[0, 2, 5], probe_layer=1),
    # fused output layer on the ping-pong kernel
    dict(name="ppout-512-8", S=9, hidden=[512, 8], plan0=[0, 4], plan1=[0, 5]),
    dict(name="ppout-576-264", S=9, hidden=[576, 264], plan0=[0, 4], plan1=[0, 5]),
    dict(name="ppout-512-400", S=9, hidden=[512, 400], plan0=[0, 4], plan1=[0, 5]),
]


def case_dims(case):
    return [case["S"] + 2] + list(case["hidden"]) + [1]


def probed_width(case):
    dims, t = case_dims(case), case.get("probe_layer")
    return dims[-2] if t is None else dims[t + 1]


def families(case):
    """"dense" and as many probe pages ("probe0", "probe1", ...) as carry every edge column of the probed layer"""
    n = len(probe_columns(probed_width(case), case.get("tail_q")))
    nmod = case["S"] - 1
    return ["dense"] + [f"probe{i}" for i in range((n + nmod - 1) // nmod)]


def case_weights(case, family, seed=7):
    """(mods, probe): probe is None for the dense family"""
    S, dims = case["S"], case_dims(case)
    if family == "dense":
        return dense_weights(S - 1, dims, seed), None
    return probe_weights(S - 1, dims, case.get("probe_layer"), seed, case.get("tail_q"), int(family[5:]))
