// fv_kernels.hip -- finite-volume assembly for dfLowMachFoam on MI355X (gfx950).
//
// Replaces the reference's face-parallel atomicAdd kernels (src_gpu/dfMatrixOpBase.cu:658-2173,
// dfUEqn.cu, dfYEqn.cu, dfEEqn.cu, dfpEqn.cu, dfRhoEqn.cu) with deterministic cell-centric gathers:
// one thread per cell walks its faces in OpenFOAM's sequential order (neighbour faces ascending,
// owned faces ascending, then its boundary slots), keeping one accumulator per fvm/fvc term, so the
// result is bit-identical to the sequential restatement in oracle/df_oracle.cpp and independent of
// scheduling. Owned-face coefficients (lower/upper) are written by the owner thread; the neighbour
// thread recomputes the same face value instead of reading it back (no grid-wide dependency).
// Whole equations are fused into one or two launches (the reference issues 10-40 per equation).
//
// Compiled with -ffp-contract=off: the arithmetic sequence is the oracle's, op for op.
#include "dfmi_ctx.h"
// Occupancy caps of the kernels that share the GPU with the side stream's chemistry: at least n
// waves' worth of registers per SIMD. -DDFMI_NO_CAPS builds the uncapped A/B variant (scripts/pmc_caps_ab.sh).
#ifdef DFMI_NO_CAPS
#define DFMI_WAVES(n)
#else
#define DFMI_WAVES(n) __attribute__((amdgpu_waves_per_eu(n, 8)))
#endif
// Stores of the YEqn assembly's ELL rows go out as sc1 stores (st_drop), which write through and drop the line from
// the XCD's L2 (MI355X_MICROARCH.md: plain / nt stores keep it), leaving the L2 to the neighbour planes the face
// gathers re-read: k_y_assemble_ell 661 -> 625 us, step 13.90 -> 13.86 ms (3 rounds each in one call, round 6,
// gpurun_out r06d). The same stores in k_u_assemble measured slower (335 -> 359 us) and stay plain (st_out).
__device__ __forceinline__ void st_drop(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_out(double* p, double v) { *p = v; }
#include <cstdlib>

namespace dfmi {

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ double interp_f(double w, double vo, double vn) { return w * (vo - vn) + vn; }
__device__ __forceinline__ double interp_b(double w, double vo, double vn) { return w * vo + (1.0 - w) * vn; }

struct BCoef { double vic, vbc, gic, gbc; };

// the cell a gather-kernel thread works on: thread order, or the traversal dfmi_set_traversal installed
// (e.g. 8x8x4 bricks on a Z-order curve over blockMesh-ordered data: same data layout, cache-compact
// visiting order). Each cell's arithmetic is unchanged, so results are bitwise independent of it.
__device__ __forceinline__ int cell_of(const MeshView& m, int t) { return (m.trav && t < m.C) ? m.trav[t] : t; }
// per-slot data of the mixed conditions of one field: waveTransmissive (advectiveFvPatchField, Euler ddt:
// refValue = the old-time boundary value, valueFraction = 1 / (1 + w dt deltaCoeffs) set at the pEqn
// assembly) and inletOutlet (refValue = inletValue, valueFraction = 1 - pos0(phi))
struct MixBC {
  const double* wvf;    // waveTransmissive valueFraction [B]
  const double* wref;   // waveTransmissive refValue (old-time boundary field) [B]
  const double* bphi;   // boundary flux (inletOutlet switch) [B]
  const double* ioref;  // inletValue [ncomp][B]
};
__device__ __forceinline__ void mix_vf_ref(int t, const MixBC& x, int b, long B, int comp, double& vf, double& ref) {
  if (t == WAVE_TRANSMISSIVE) { vf = x.wvf[b]; ref = x.wref[b]; }
  else { vf = x.bphi[b] >= 0.0 ? 0.0 : 1.0; ref = x.ioref[comp * B + b]; }
}
__device__ __forceinline__ BCoef bcoef_mixed(double vf, double ref, double bdc) {
  return {1.0 - vf, vf * ref, -vf * bdc, vf * bdc * ref};
}
__device__ __forceinline__ BCoef bcoef(int t, double bval, double w, double bdc, double egrad = 0.0) {
  switch (t) {
    case ZERO_GRADIENT: case EXTRAPOLATED: return {1., 0., 0., 0.};
    case FIXED_VALUE: case FIXED_ENERGY: return {0., bval, -1 * bdc, bdc * bval};
    case GRADIENT_ENERGY: return {1., egrad / bdc, 0., egrad};
    default: return {w, 1.0 - w, -1 * bdc, bdc};
  }
}

__device__ __forceinline__ BCoef bcoef_f(int t, double bval, double w, double bdc, const MixBC& mx, int b, long B, int comp,
                                        double egrad = 0.0) {
  if (bc_mixed(t)) {
    double vf, ref;
    mix_vf_ref(t, mx, b, B, comp, vf, ref);
    return bcoef_mixed(vf, ref, bdc);
  }
  return bcoef(t, bval, w, bdc, egrad);
}

// coupled neighbour-side cell value: cyclic partner cell, or the processor halo value in the slot
__device__ __forceinline__ double nbrv(const MeshView& m, const double* vf, const double* bvf, int b) {
  int pc = m.partner[b];
  return pc >= 0 ? vf[pc] : bvf[b];
}
__device__ __forceinline__ double bface(const MeshView& m, int t, const double* vf, const double* bvf, int b, int c) {
  return bc_coupled(t) ? interp_b(m.bw[b], vf[c], nbrv(m, vf, bvf, b)) : bvf[b];
}

// upwind weight of a slot's own cell from the flux out of it. A flux of exactly zero gives the weight 1 to the
// cell, as an internal face gives it to its owner -- except on the higher rank's side of a processor face
// (MeshView::sprim == 2, halo_setup), so that one rank only calls itself upwind there: what rides on that weight
// without being phi (the YEqn's phiUc) would otherwise be convected out of both cells. Cyclic and processorCyclic
// faces keep the weight 1 on both halves, which is what a single domain computes for a cyclic pair.
__device__ __forceinline__ double upwind_b(const MeshView& m, const double* __restrict__ bphi, int b) {
  const double ph = bphi[b];
  if (ph > 0) return 1.0;
  if (ph < 0) return 0.0;
  return m.sprim[b] == 2 ? 0.0 : 1.0;
}

// visit faces of cell c in sequential order: fn(face, other_cell, is_owner).
// WT > 0 (meshes whose busiest cell has WT couplings, hex meshes: 6): read the cell's row of the solver
// gather (ELL [W][C], built once: neighbour faces ascending, owned faces ascending, then coupled slots)
// -- coalesced index loads, one indirection, all WT entries loaded up front and the loop unrolled, so
// every face's gathers are in flight together instead of one face's latency after another's.
// WT = 0: the CSR walk (nbrStart/nbrFace, ownStart), same order, any mesh.
// WT = -1: hex box in blockMesh order (MeshView::hx): the same faces in the same order from the cell's
// (i, j, k) -- neighbour faces from the z-, y-, x- cells, then the owned +x, +y, +z faces; a face of
// owner o sits at storage kslot C + o, kslot = the owner's owned faces before it -- no index loads.
template <int WT, class FN> __device__ __forceinline__ void each_face(const MeshView& m, int c, FN&& fn) {
  if constexpr (WT < 0) {
    const int nx = m.hx, ny = m.hy, nxy = m.hx * m.hy;
    const int t = c / nx, i = c - t * nx, k = t / ny, j = t - k * ny;
    const int hxp = i < nx - 1, hyp = j < ny - 1;
    const int C = m.C;
    if (k > 0) { const int o = c - nxy; fn((hxp + hyp) * C + o, o, false); }
    if (j > 0) { const int o = c - nx; fn(hxp * C + o, o, false); }
    if (i > 0) fn(c - 1, c - 1, false);
    if (hxp) fn(c, c + 1, true);
    if (hyp) fn(hxp * C + c, c + nx, true);
    if (k < m.hz - 1) fn((hxp + hyp) * C + c, c + nxy, true);
  } else if constexpr (WT > 0) {
    int es[WT], cs[WT];
    const long C = m.C;
#pragma unroll
    for (int k = 0; k < WT; ++k) { cs[k] = m.ecol[k * C + c]; es[k] = m.esrc[k * C + c]; }
#pragma unroll
    for (int k = 0; k < WT; ++k)
      if (es[k] >= 0) fn(es[k] >> 1, cs[k], (es[k] & 1) != 0);   // slots (< 0) and padding skipped
  } else {
    const int e1 = m.nbrStart[c + 1];
    for (int k = m.nbrStart[c]; k < e1; ++k) { const int f = m.nbrFace[k]; fn(f, m.own[f], false); }
    const int o0 = m.ownStart[c], no = m.ownStart[c + 1] - o0;
    for (int k = 0; k < no; ++k) {
      const int f = m.fslot ? k * m.C + c : o0 + k;   // storage index of the k-th owned face
      fn(f, m.nei[f], true);
    }
  }
}
// visit primary, non-empty boundary slots of c in slot order: fn(slot, type)
template <class FN> __device__ __forceinline__ void each_slot(const MeshView& m, const int8_t* ty, int c, FN&& fn) {
  const int e = m.cbStart[c + 1];
  for (int k = m.cbStart[c]; k < e; ++k) {
    const int b = m.cbSlot[k];
    const int t = ty[b];
    if (t == EMPTY) continue;
    fn(b, t);
  }
}

// ------------------------------------------------------------------ boundary correction
// correct_boundary_conditions_scalar/vector (dfMatrixOpBase.cu:2402-2491)
// gradientEnergy: cell value + gradient / deltaCoeffs (correct_boundary_conditions_gradientEnergy_scalar,
// dfMatrixOpBase.cu:351-366)
__global__ void k_bc_correct(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ vf,
                             double* __restrict__ bvf, int ncomp, const double* __restrict__ egrad, MixBC mx) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  const int t = ty[b];
  const int c = m.bfc[b];
  for (int k = 0; k < ncomp; ++k) {
    const double* v = vf + (long)k * m.C;
    double* bv = bvf + (long)k * m.B;
    if (bc_mixed(t)) {   // mixedFvPatchField::evaluate
      double f, ref;
      mix_vf_ref(t, mx, b, m.B, k, f, ref);
      bv[b] = f * ref + (1.0 - f) * v[c];
    } else if (t == ZERO_GRADIENT || t == EXTRAPOLATED) bv[b] = v[c];
    else if (t == CYCLIC) bv[b] = interp_b(m.bw[b], v[c], v[m.partner[b]]);
    else if (bc_proc(t) && !m.sprim[b]) bv[b] = v[c];
    else if (t == GRADIENT_ENERGY && egrad) bv[b] = v[c] + egrad[b] / m.bdc[b];
  }
}

// ------------------------------------------------------------------ limited / cubic schemes
// The terms the reference GPU path hard-wires (upwind Yi/ha, linear K and hDiffCorrFlux; dfYEqn.cu:543,
// 587-593, dfEEqn.cu:166-174) with the schemes the reference's own cases select (system/fvSchemes:
// div(phi,Yi_h) Gauss limitedLinear01 1 -- multivariate over every Y_i and he, YEqn.H:6-14; div(phi,K)
// Gauss limitedLinear 1; div(hDiffCorrFlux) Gauss cubic), OpenFOAM-7 semantics as restated in
// oracle/df_oracle.cpp (limited_weights, conv_weights, k_weights, cubic_flux) -- the same operations in
// the same order, so the weights and fluxes are bitwise the oracle's.
__device__ __forceinline__ double pos0(double x) { return x >= 0 ? 1.0 : 0.0; }
__device__ __forceinline__ double sgn(double x) { return x >= 0 ? 1.0 : -1.0; }

// limitedLinearLimiter<NVDTVD>::limiter (+ Limited01Limiter's bounds when b01); g = the upwind cell's gradient
__device__ __forceinline__ double ll_limiter(double twoByk, double faceFlux, double phiP, double phiN,
                                             const double* g, const double* dv) {
  const double gradf = phiN - phiP;
  const double gradcf = dv[0] * g[0] + dv[1] * g[1] + dv[2] * g[2];
  double r;
  if (fabs(gradcf) >= 1000 * fabs(gradf)) r = 2 * 1000 * sgn(gradcf) * sgn(gradf) - 1;
  else r = 2 * (gradcf / gradf) - 1;
  return fmax(fmin(twoByk * r, 1.0), 0.0);
}
__device__ __forceinline__ bool out01(double faceFlux, double phiP, double phiN) {
  return (faceFlux > 0 && (phiP < 0 || phiN > 1)) || (faceFlux < 0 && (phiN < 0 || phiP > 1));
}

// Gauss linear gradient of a scalar at cell c (fvc::grad; the oracle's grad_scalar: faces in
// increasing index, then the cell's boundary slots, / V)
template <int WT = 0>
__device__ __forceinline__ void cell_grad(const MeshView& m, const int8_t* __restrict__ ty, const double* __restrict__ vf,
                                          const double* __restrict__ bvf, int c, double* g) {
  const long F = m.F, B = m.B;
  const double vc = vf[c];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double w = m.w[f], vn = vf[o2];
    const double yf = own ? interp_f(w, vc, vn) : interp_f(w, vn, vc);
    const double v0 = m.Sf[f] * yf, v1 = m.Sf[F + f] * yf, v2 = m.Sf[2 * F + f] * yf;
    if (own) { s0 += v0; s1 += v1; s2 += v2; } else { s0 -= v0; s1 -= v1; s2 -= v2; }
  });
  each_slot(m, ty, c, [&](int b, int t) {
    const double yf = bface(m, t, vf, bvf, b, c);
    s0 += m.bSf[b] * yf; s1 += m.bSf[B + b] * yf; s2 += m.bSf[2 * B + b] * yf;
  });
  const double vol = m.V[c];
  g[0] = s0 / vol; g[1] = s1 / vol; g[2] = s2 / vol;
}

// multivariate limited weights of div(phi,Yi_h) over {Y_0 .. Y_{S-1}, he} on the internal faces (face
// storage order), in two passes so that no wave idles behind a few lanes:
//  k_conv_w_check -- one thread per face: Limited01's bounds for every field (he of a real mixture
//    leaves [0, 1] almost everywhere, which makes the minimum 0 without any gradient); such faces get
//    their (upwind) weight here, the others are appended to a list (the order of the list does not
//    matter: every face's weight is computed on its own);
//  k_conv_w_list -- a 16-lane group per listed face, one lane per field: the limiter from the upwind
//    cell's Gauss gradient formed on the fly, the group's minimum (fmin, exact) -> the weight.
// The list is reserved with ONE atomic per workgroup (1024 threads x 4 faces): a per-wavefront atomic on
// the single counter serialised ~10^5 times per launch (most waves hold a listed face) and cost 450 us.
constexpr int CK_TPB = 1024, CK_FPT = 4, CK_NW = CK_TPB / 64;
__global__ void __launch_bounds__(CK_TPB) k_conv_w_check(MeshView m, int S, int b01, const double* __restrict__ phi,
                                                         const double* __restrict__ Y, const double* __restrict__ he,
                                                         double* __restrict__ wout, int* __restrict__ list,
                                                         int* __restrict__ nlist) {
  __shared__ int wcnt[CK_FPT * CK_NW];
  __shared__ int base;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long C = m.C;
  unsigned long long mask[CK_FPT];
#pragma unroll
  for (int j = 0; j < CK_FPT; ++j) {
    const int f = (blockIdx.x * CK_FPT + j) * CK_TPB + threadIdx.x;
    bool need = false;
    const int o = f < m.F ? m.own[f] : -1;
    if (o >= 0) {   // not past the end, not owner-slot padding
      const int n = m.nei[f];
      const double ph = phi[f];
      bool zero = false;
      if (b01) {
        zero = out01(ph, he[o], he[n]);
        // the species' checks without a loop-carried exit: their loads issue together (a wave runs this
        // branch when any of its lanes passed the he check)
        for (int s0 = 0; s0 < S && !zero; s0 += 4) {
          double yo[4], yn[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int sp = s0 + q < S ? s0 + q : S - 1;
            yo[q] = Y[sp * C + o]; yn[q] = Y[sp * C + n];
          }
          bool z = false;
#pragma unroll
          for (int q = 0; q < 4; ++q) z = z || out01(ph, yo[q], yn[q]);
          zero = z;
        }
      }
      if (zero) {
        const double lim = 0.0;
        wout[f] = lim * m.w[f] + (1 - lim) * pos0(ph);
      }
      need = !zero;
    }
    mask[j] = __ballot(need);
    if (lane == 0) wcnt[j * CK_NW + wid] = (int)__popcll(mask[j]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int k = 0; k < CK_FPT * CK_NW; ++k) tot += wcnt[k];
    base = tot ? atomicAdd(nlist, tot) : 0;
  }
  __syncthreads();
  int off = base;   // entries of the (j, wave) runs before this wave's run of pass j
  for (int k = 0; k < wid; ++k) off += wcnt[k];
#pragma unroll
  for (int j = 0; j < CK_FPT; ++j) {
    if ((mask[j] >> lane) & 1ull)
      list[off + (int)__popcll(mask[j] & ((1ull << lane) - 1ull))] = (blockIdx.x * CK_FPT + j) * CK_TPB + threadIdx.x;
    // next pass: skip the remaining waves of pass j and the first waves of pass j + 1
    for (int k = wid; k < CK_NW; ++k) off += wcnt[j * CK_NW + k];
    if (j + 1 < CK_FPT)
      for (int k = 0; k < wid; ++k) off += wcnt[(j + 1) * CK_NW + k];
  }
}
constexpr int CWG = 16;   // lanes per listed face (fields beyond 16 loop)
template <int WT>
__global__ void __launch_bounds__(256) k_conv_w_list(MeshView m, int S, const int8_t* __restrict__ tyY,
    const int8_t* __restrict__ tyH, double twoByk, const double* __restrict__ phi, const double* __restrict__ Y,
    const double* __restrict__ bY, const double* __restrict__ he, const double* __restrict__ bhe,
    const int* __restrict__ list, const int* __restrict__ nlist, double* __restrict__ wout) {
  const int lane = threadIdx.x % CWG;
  const int n_items = *nlist;
  const int groups = gridDim.x * (blockDim.x / CWG);
  const long C = m.C, Fs = m.F, B = m.B;
  // a group's lanes share `it`, so each group runs the loop (and its shuffles) in lockstep
  for (int it = blockIdx.x * (blockDim.x / CWG) + threadIdx.x / CWG; it < n_items; it += groups) {
    const int f = list[it];
    const int o = m.own[f], n = m.nei[f];
    const double ph = phi[f];
    const double dv[3] = {m.md[f], m.md[Fs + f], m.md[2 * Fs + f]};
    const int cu = ph > 0 ? o : n;   // NVDTVD::r reads the upwind cell's gradient
    double lim = 2.0;                // above every limiter: the neutral element of the min
    for (int s = lane; s <= S; s += CWG) {
      const double* v = s < S ? Y + s * C : he;
      const double* bv = s < S ? bY + s * B : bhe;
      double g[3];
      cell_grad<WT>(m, s < S ? tyY : tyH, v, bv, cu, g);
      lim = fmin(lim, ll_limiter(twoByk, ph, v[o], v[n], g, dv));
    }
#pragma unroll
    for (int off = CWG / 2; off > 0; off >>= 1) lim = fmin(lim, __shfl_xor(lim, off, CWG));
    if (lane == 0) wout[f] = lim * m.w[f] + (1 - lim) * pos0(ph);
  }
}

// the same on the boundary slots: coupled (cyclic) slots with the partner cell as N and the patch delta;
// every other slot takes limiter 1 (calcLimiter's non-coupled branch), i.e. its CD weight
// bgx: on decomposed meshes the neighbour-side gradients of every field on the processor slots
// ([3(S+1)][B], exchanged: patchNeighbourField of fvc::grad), nullptr otherwise
__global__ void k_conv_w_slot(MeshView m, int S, const int8_t* __restrict__ tyY, const int8_t* __restrict__ tyH,
                              int b01, double twoByk, const double* __restrict__ bphi, const double* __restrict__ Y,
                              const double* __restrict__ bY, const double* __restrict__ he,
                              const double* __restrict__ bhe, const double* __restrict__ bgx, double* __restrict__ bwout) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  const long C = m.C, B = m.B;
  const int t = tyY[b];
  const double ph = bphi[b];
  double lim = 1.0;
  if (bc_coupled(t) && m.sprim[b]) {
    const int c = m.bfc[b], pc = m.partner[b];   // pc < 0: processor slot, neighbour values in the slot
    auto vn = [&](const double* v, const double* bv) { return pc >= 0 ? v[pc] : bv[b]; };
    lim = 0.0;
    bool zero = false;
    if (b01) {
      zero = out01(ph, he[c], vn(he, bhe));
      for (int s = 0; s < S && !zero; ++s) zero = out01(ph, Y[s * C + c], vn(Y + s * C, bY + s * B));
    }
    if (!zero) {
      const double dv[3] = {m.bdv[b], m.bdv[B + b], m.bdv[2 * B + b]};
      const bool own_up = ph > 0;
      for (int s = 0; s <= S; ++s) {
        const double* v = s < S ? Y + s * C : he;
        const double* bv = s < S ? bY + s * B : bhe;
        double g[3];
        if (own_up || pc >= 0) cell_grad(m, s < S ? tyY : tyH, v, bv, own_up ? c : pc, g);
        else { g[0] = bgx[(3 * s) * B + b]; g[1] = bgx[(3 * s + 1) * B + b]; g[2] = bgx[(3 * s + 2) * B + b]; }
        const double l = ll_limiter(twoByk, ph, v[c], vn(v, bv), g, dv);
        lim = s == 0 ? l : fmin(lim, l);
      }
    }
  }
  bwout[b] = lim * m.bw[b] + (1 - lim) * upwind_b(m, bphi, b);
}

// gradients of every field of the table at the cells of the processor slots -> g [3(S+1)][C] (only those
// cells written; the halo then carries them to the neighbour ranks' processor slots)
__global__ void k_conv_proc_grad(MeshView m, int S, const int8_t* __restrict__ tyY, const int8_t* __restrict__ tyH,
                                 const double* __restrict__ Y, const double* __restrict__ bY,
                                 const double* __restrict__ he, const double* __restrict__ bhe, double* __restrict__ g) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  if (!bc_proc(tyY[b]) || !m.sprim[b]) return;
  const long C = m.C, B = m.B;
  const int c = m.bfc[b];
  for (int s = 0; s <= S; ++s) {
    double gg[3];
    cell_grad(m, s < S ? tyY : tyH, s < S ? Y + s * C : he, s < S ? bY + s * B : bhe, c, gg);
    g[(3 * s) * C + c] = gg[0]; g[(3 * s + 1) * C + c] = gg[1]; g[(3 * s + 2) * C + c] = gg[2];
  }
}

// Gauss linear gradients of NC scalar components (component k at vf + k*C, boundary bvf + k*B)
// -> g [(3k + dir)][C] (fvc::grad of each vf.component(k)); one face walk for all components, each
// component summed in cell_grad's order
template <int NC, int WT>
__global__ void __launch_bounds__(TPB) k_grad_cells(MeshView m, const int8_t* __restrict__ ty,
                                                    const double* __restrict__ vf, const double* __restrict__ bvf,
                                                    double* __restrict__ g) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, F = m.F, B = m.B;
  double s[NC][3], vc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) { s[k][0] = 0.0; s[k][1] = 0.0; s[k][2] = 0.0; vc[k] = vf[k * C + c]; }
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double w = m.w[f], sf0 = m.Sf[f], sf1 = m.Sf[F + f], sf2 = m.Sf[2 * F + f];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const double vn = vf[k * C + o2];
      const double yf = own ? interp_f(w, vc[k], vn) : interp_f(w, vn, vc[k]);
      const double v0 = sf0 * yf, v1 = sf1 * yf, v2 = sf2 * yf;
      if (own) { s[k][0] += v0; s[k][1] += v1; s[k][2] += v2; } else { s[k][0] -= v0; s[k][1] -= v1; s[k][2] -= v2; }
    }
  });
  each_slot(m, ty, c, [&](int b, int t) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const double yf = bface(m, t, vf + k * C, bvf + k * B, b, c);
      s[k][0] += m.bSf[b] * yf; s[k][1] += m.bSf[B + b] * yf; s[k][2] += m.bSf[2 * B + b] * yf;
    }
  });
  const double vol = m.V[c];
#pragma unroll
  for (int k = 0; k < NC; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) g[(3 * k + d) * C + c] = s[k][d] / vol;
}

// single-field limited weights (LimitedScheme: div(phi,K)) from a precomputed gradient g [3][C]
__global__ void k_lim_w_face(MeshView m, int b01, double twoByk, const double* __restrict__ phi,
                             const double* __restrict__ v, const double* __restrict__ g, double* __restrict__ wout) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.F) return;
  const int o = m.own[f];
  if (o < 0) return;
  const int n = m.nei[f];
  const long C = m.C, Fs = m.F;
  const double ph = phi[f];
  double lim = 0.0;
  if (!(b01 && out01(ph, v[o], v[n]))) {
    const double dv[3] = {m.md[f], m.md[Fs + f], m.md[2 * Fs + f]};
    const int cu = ph > 0 ? o : n;
    const double gu[3] = {g[cu], g[C + cu], g[2 * C + cu]};
    lim = ll_limiter(twoByk, ph, v[o], v[n], gu, dv);
  }
  wout[f] = lim * m.w[f] + (1 - lim) * pos0(ph);
}
// the same on a hex box in blockMesh order, one thread per cell over its owned (+x, +y, +z) faces (no owner /
// neighbour index loads, the owner's value read once); bitwise k_lim_w_face
__global__ void k_lim_w_cell(MeshView m, int b01, double twoByk, const double* __restrict__ phi,
                             const double* __restrict__ v, const double* __restrict__ g, double* __restrict__ wout) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const int nx = m.hx, ny = m.hy, nxy = m.hx * m.hy;
  const int t = c / nx, i = c - t * nx, k = t / ny, j = t - k * ny;
  const int hxp = i < nx - 1, hyp = j < ny - 1, hzp = k < m.hz - 1;
  const long C = m.C, Fs = m.F;
  const double vo = v[c];
  auto face = [&](long f, int n) {
    const double ph = phi[f], vn = v[n];
    double lim = 0.0;
    if (!(b01 && out01(ph, vo, vn))) {
      const double dv[3] = {m.md[f], m.md[Fs + f], m.md[2 * Fs + f]};
      const int cu = ph > 0 ? c : n;
      const double gu[3] = {g[cu], g[C + cu], g[2 * C + cu]};
      lim = ll_limiter(twoByk, ph, vo, vn, gu, dv);
    }
    wout[f] = lim * m.w[f] + (1 - lim) * pos0(ph);
  };
  if (hxp) face(c, c + 1);
  if (hyp) face(hxp * C + c, c + nx);
  if (hzp) face((hxp + hyp) * C + c, c + nxy);
}
// boundary slots; bg = the neighbour-side gradient on processor slots ([3][B], halo), cyclic: partner cell
__global__ void k_lim_w_slot(MeshView m, const int8_t* __restrict__ ty, int b01, double twoByk,
                             const double* __restrict__ bphi, const double* __restrict__ v, const double* __restrict__ bv,
                             const double* __restrict__ g, const double* __restrict__ bg, double* __restrict__ bwout) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  const long C = m.C, B = m.B;
  const int t = ty[b];
  const double ph = bphi[b];
  double lim = 1.0;
  if (bc_coupled(t) && m.sprim[b]) {
    const int c = m.bfc[b], pc = m.partner[b];
    const double vn = nbrv(m, v, bv, b);
    lim = 0.0;
    if (!(b01 && out01(ph, v[c], vn))) {
      const double dv[3] = {m.bdv[b], m.bdv[B + b], m.bdv[2 * B + b]};
      double gu[3];
      for (int q = 0; q < 3; ++q) gu[q] = ph > 0 ? g[q * C + c] : (pc >= 0 ? g[q * C + pc] : bg[q * B + b]);
      lim = ll_limiter(twoByk, ph, v[c], vn, gu, dv);
    }
  }
  bwout[b] = lim * m.bw[b] + (1 - lim) * upwind_b(m, bphi, b);
}

__global__ void k_upwind_w_face(MeshView m, const double* __restrict__ phi, double* __restrict__ wout) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.F || m.own[f] < 0) return;
  wout[f] = pos0(phi[f]);
}
__global__ void k_upwind_w_slot(MeshView m, const double* __restrict__ bphi, double* __restrict__ bwout) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  bwout[b] = upwind_b(m, bphi, b);
}

// limitedLinearV weights of div(phi,U) (limitedLinearLimiter<NVDVTVDV>) from grad(U) g [9][C]
__device__ __forceinline__ double llv_limiter(double twoByk, const double* vP, const double* vN, const double* g,
                                              const double* dv) {
  const double gv[3] = {vN[0] - vP[0], vN[1] - vP[1], vN[2] - vP[2]};
  const double gradf = gv[0] * gv[0] + gv[1] * gv[1] + gv[2] * gv[2];
  double dg[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) dg[j] = dv[0] * g[j] + dv[1] * g[3 + j] + dv[2] * g[6 + j];
  const double gradcf = gv[0] * dg[0] + gv[1] * dg[1] + gv[2] * dg[2];
  double r;
  if (fabs(gradcf) >= 1000 * fabs(gradf)) r = 2 * 1000 * sgn(gradcf) * sgn(gradf) - 1;
  else r = 2 * (gradcf / gradf) - 1;
  return fmax(fmin(twoByk * r, 1.0), 0.0);
}
__global__ void k_llv_w_face(MeshView m, double twoByk, const double* __restrict__ phi, const double* __restrict__ U,
                             const double* __restrict__ g, double* __restrict__ wout) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.F) return;
  const int o = m.own[f];
  if (o < 0) return;
  const int n = m.nei[f];
  const long C = m.C, Fs = m.F;
  const double ph = phi[f];
  const double dv[3] = {m.md[f], m.md[Fs + f], m.md[2 * Fs + f]};
  const double vP[3] = {U[o], U[C + o], U[2 * C + o]}, vN[3] = {U[n], U[C + n], U[2 * C + n]};
  const int cu = ph > 0 ? o : n;
  double gu[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) gu[q] = g[q * C + cu];
  const double lim = llv_limiter(twoByk, vP, vN, gu, dv);
  wout[f] = lim * m.w[f] + (1 - lim) * pos0(ph);
}
__global__ void k_llv_w_slot(MeshView m, const int8_t* __restrict__ ty, double twoByk, const double* __restrict__ bphi,
                             const double* __restrict__ U, const double* __restrict__ g, double* __restrict__ bwout) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  const long C = m.C, B = m.B;
  const int t = ty[b];
  const double ph = bphi[b];
  double lim = 1.0;
  if (bc_coupled(t) && m.sprim[b] && m.partner[b] >= 0) {   // cyclic (processor patches are rejected on the host)
    const int c = m.bfc[b], pc = m.partner[b];
    const double dv[3] = {m.bdv[b], m.bdv[B + b], m.bdv[2 * B + b]};
    const double vP[3] = {U[c], U[C + c], U[2 * C + c]}, vN[3] = {U[pc], U[C + pc], U[2 * C + pc]};
    const int cu = ph > 0 ? c : pc;
    double gu[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) gu[q] = g[q * C + cu];
    lim = llv_limiter(twoByk, vP, vN, gu, dv);
  }
  bwout[b] = lim * m.bw[b] + (1 - lim) * upwind_b(m, bphi, b);
}

// cubic::correction of a vector field (3 components), dotted with Sf: the flux cubic adds to the linear
// face flux (surfaceInterpolationScheme::dotInterpolate + Sf & correction); g = its gradients [9][C]
__device__ __forceinline__ double cubic_corr(double lam, const double* S, double ms, double dc, const double* vP,
                                             const double* vN, const double* gP, const double* gN) {
  const double kSc = lam * (1 - lam * (3 - 2 * lam));
  const double kVecP = ((1 - lam) * (1 - lam)) * lam;
  const double kVecN = (lam * lam) * (lam - 1);
  double cr[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v = kSc * vP[c] + (-kSc) * vN[c];
    double gi[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) gi[q] = kVecP * gP[3 * c + q] + kVecN * gN[3 * c + q];
    cr[c] = v + (((gi[0] * S[0] + gi[1] * S[1] + gi[2] * S[2]) / ms) / dc);
  }
  return S[0] * cr[0] + S[1] * cr[1] + S[2] * cr[2];
}
__global__ void k_cubic_face(MeshView m, const double* __restrict__ vf, const double* __restrict__ g,
                             double* __restrict__ cf) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.F) return;
  const int o = m.own[f];
  if (o < 0) return;
  const int n = m.nei[f];
  const long C = m.C, Fs = m.F;
  const double S[3] = {m.Sf[f], m.Sf[Fs + f], m.Sf[2 * Fs + f]};
  double vP[3], vN[3], gP[9], gN[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) { vP[c] = vf[c * C + o]; vN[c] = vf[c * C + n]; }
#pragma unroll
  for (int q = 0; q < 9; ++q) { gP[q] = g[q * C + o]; gN[q] = g[q * C + n]; }
  cf[f] = cubic_corr(m.w[f], S, m.magSf[f], m.dc[f], vP, vN, gP, gN);
}
// the same on a hex box in blockMesh order (MeshView::hx), one thread per cell over its owned (+x, +y, +z) faces:
// the owner's value and gradient are loaded once for its three faces instead of once per face (face-parallel: 24
// gathered doubles per face); bitwise k_cubic_face (the same cubic_corr on the same operands)
__global__ void k_cubic_cell(MeshView m, const double* __restrict__ vf, const double* __restrict__ g,
                             double* __restrict__ cf) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const int nx = m.hx, ny = m.hy, nxy = m.hx * m.hy;
  const int t = c / nx, i = c - t * nx, k = t / ny, j = t - k * ny;
  const int hxp = i < nx - 1, hyp = j < ny - 1, hzp = k < m.hz - 1;
  const long C = m.C, Fs = m.F;
  double vP[3], gP[9];
#pragma unroll
  for (int q = 0; q < 3; ++q) vP[q] = vf[q * C + c];
#pragma unroll
  for (int q = 0; q < 9; ++q) gP[q] = g[q * C + c];
  auto face = [&](long f, int n) {
    const double S[3] = {m.Sf[f], m.Sf[Fs + f], m.Sf[2 * Fs + f]};
    double vN[3], gN[9];
#pragma unroll
    for (int q = 0; q < 3; ++q) vN[q] = vf[q * C + n];
#pragma unroll
    for (int q = 0; q < 9; ++q) gN[q] = g[q * C + n];
    cf[f] = cubic_corr(m.w[f], S, m.magSf[f], m.dc[f], vP, vN, gP, gN);
  };
  if (hxp) face(c, c + 1);
  if (hyp) face(hxp * C + c, c + nx);
  if (hzp) face((hxp + hyp) * C + c, c + nxy);
}
__global__ void k_cubic_slot(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ vf,
                             const double* __restrict__ bvf, const double* __restrict__ g, const double* __restrict__ bg,
                             double* __restrict__ bcf) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  const long C = m.C, B = m.B;
  const int t = ty[b];
  if (!bc_coupled(t) || !m.sprim[b]) { bcf[b] = 0.0; return; }
  const int c0 = m.bfc[b], pc = m.partner[b];
  const double S[3] = {m.bSf[b], m.bSf[B + b], m.bSf[2 * B + b]};
  double vP[3], vN[3], gP[9], gN[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) { vP[c] = vf[c * C + c0]; vN[c] = nbrv(m, vf + c * C, bvf + c * B, b); }
#pragma unroll
  for (int q = 0; q < 9; ++q) { gP[q] = g[q * C + c0]; gN[q] = pc >= 0 ? g[q * C + pc] : bg[q * B + b]; }
  bcf[b] = cubic_corr(m.bw[b], S, m.bmagSf[b], m.bdc[b], vP, vN, gP, gN);
}

// ------------------------------------------------------------------ old <- new (preTimeStep)
// every pair in one launch (grid.y = pair) instead of one copy launch per field
constexpr int MAXCOPY = 12;
struct CopyList { const double* src[MAXCOPY]; double* dst[MAXCOPY]; long n[MAXCOPY]; };
__global__ void k_copy_multi(CopyList L) {
  const int j = blockIdx.y;
  const double* __restrict__ a = L.src[j];
  double* __restrict__ b = L.dst[j];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < L.n[j]; i += (long)gridDim.x * blockDim.x) b[i] = a[i];
}

// ------------------------------------------------------------------ rhoEqn (dfRhoEqn.cu:41-92)
template <int WT>
__global__ void k_rho(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ rho_old,
                      const double* __restrict__ phi, const double* __restrict__ bphi, double* __restrict__ rho,
                      double* __restrict__ odiag, double* __restrict__ osrc) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  double div = 0.0;
  each_face<WT>(m, c, [&](int f, int, bool own) { if (own) div += phi[f]; else div -= phi[f]; });
  each_slot(m, ty, c, [&](int b, int) { div += bphi[b]; });
  const double diag = m.rdt * m.V[c];
  double src = m.rdt * rho_old[c] * m.V[c];
  src = src - div;
  rho[c] = src / diag;
  if (odiag) { odiag[c] = diag; osrc[c] = src; }
}

// ------------------------------------------------------------------ spray coupling (include/dfmi.h, spray block)
// The cloud's per-cell transfer fields folded into the rho, U, Yi and he equations, each term the last thing added to
// its diag / source, in the operation order include/dfmi.h states (-ffp-contract=off: no fused multiply-add). Streaming
// per-cell passes: one thread per cell (per species for Yi), [S][C] reads coalesced, no atomics, no LDS. They run only
// with spray.model = 1; every other kernel of this file is what it was.
//
// rhoEqn with parcels.Srho(rho) (rhoEqn.H:38): k_rho's cell with the term between the source and the diagonal solve.
// semi: SuSp(s / rho, rho) with rho as it stands before this solve (ReactingCloudI.H:211-236).
template <int WT>
__global__ void k_rho_spray(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ rho_old,
                            const double* __restrict__ phi, const double* __restrict__ bphi, double* __restrict__ rho,
                            double* __restrict__ odiag, double* __restrict__ osrc, const double* __restrict__ rhoTrans,
                            int S, int semi) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  double div = 0.0;
  each_face<WT>(m, c, [&](int f, int, bool own) { if (own) div += phi[f]; else div -= phi[f]; });
  each_slot(m, ty, c, [&](int b, int) { div += bphi[b]; });
  const double vol = m.V[c];
  double diag = m.rdt * vol;
  double src = m.rdt * rho_old[c] * vol;
  src = src - div;
  double sum = 0.0;
  for (int i = 0; i < S; ++i) sum += rhoTrans[(long)i * m.C + c];
  const double t = sum * m.rdt;
  if (semi) {
    const double r = rho[c];
    const double a = (t / vol) / r;
    diag = diag - vol * fmax(a, 0.0);
    src = src + (vol * fmin(a, 0.0)) * r;
  } else src = src + t;
  rho[c] = src / diag;
  if (odiag) { odiag[c] = diag; osrc[c] = src; }
}
// UEqn with parcels.SU(U) (UEqn.H:9). semi: UTrans - Sp(UCoeff, U) + UCoeff U (KinematicCloudI.H:432-437): the diagonal
// takes UCoeff rdt, and rAU is formed again from it and the stored internalCoeffs as k_u_assemble forms it.
__global__ void k_spray_u(MeshView m, const int8_t* __restrict__ tyU, int semi, const double* __restrict__ UTrans,
                          const double* __restrict__ UCoeff, const double* __restrict__ U, double* __restrict__ diag,
                          double* __restrict__ src, double* __restrict__ srcs, const double* __restrict__ ic,
                          double* __restrict__ rAU) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.C) return;
  const long C = m.C, B = m.B;
  double uc = 0.0;
  if (semi) {
    uc = UCoeff[c];
    const double dg = diag[c] + uc * m.rdt;
    diag[c] = dg;
    double r = dg;
    each_slot(m, tyU, c, [&](int b, int) { r += (ic[b] + ic[B + b] + ic[2 * B + b]) / 3; });
    rAU[c] = 1 / (r / m.V[c]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double t = semi ? (UTrans[k * C + c] + uc * U[k * C + c]) * m.rdt : UTrans[k * C + c] * m.rdt;
    src[k * C + c] = src[k * C + c] + t;
    srcs[k * C + c] = srcs[k * C + c] + t;
  }
}
// YEqn with parcels.SYi(i, Yi) (YEqn.H:110-111), blockIdx.y = species; the inert species has no equation. ell: the
// solver's rows (system index skips the inert species, row position eopos[c]) instead of the LDU arrays [S][C].
// semi (ReactingCloudI.H:110-131): a sink goes to the diagonal over Yi + small, a source stays explicit.
__global__ void k_spray_y(MeshView m, int inert, int semi, int ell, long stride, const double* __restrict__ rhoTrans,
                          const double* __restrict__ Y, double* __restrict__ diag, double* __restrict__ src) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (c >= m.C || i == inert) return;
  const long C = m.C;
  const long row = ell ? (long)(i < inert ? i : i - 1) * stride + (m.eopos ? m.eopos[c] : c) : (long)i * stride + c;
  const double t = rhoTrans[i * C + c] * m.rdt;
  if (semi) {
    const double vol = m.V[c];
    const double s = t / vol;
    if (s < 0) diag[row] = diag[row] + (vol * (-s)) / (Y[i * C + c] + 1e-15);
    else src[row] = src[row] + s * vol;
  } else src[row] = src[row] + t;
}
// EEqn with parcels.Sh(he) and hcSource = sum_i rhoTrans_i hc_i / deltaT (EEqn.H:3-8, 27-28, 34-35). semi
// (ThermoCloudI.H:236-245): hsTrans - SuSp(hsCoeff / Cp, he) + hsCoeff / Cp he, whose two he terms cancel where the
// coefficient is negative.
__global__ void k_spray_e(MeshView m, int S, int semi, const double* __restrict__ rhoTrans, const double* __restrict__ hc,
                          const double* __restrict__ hsTrans, const double* __restrict__ hsCoeffByCp,
                          const double* __restrict__ he, double* __restrict__ diag, double* __restrict__ src) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.C) return;
  const long C = m.C;
  const double sens = hsTrans[c] * m.rdt;
  double s = src[c];
  bool impl = false;
  if (semi) {
    const double vol = m.V[c];
    const double a = (hsCoeffByCp[c] * m.rdt) / vol;
    if (a >= 0) {
      const double aV = a * vol;
      diag[c] = diag[c] + aV;
      s = s + (sens + aV * he[c]);
      impl = true;
    }
  }
  if (!impl) s = s + sens;
  double h = 0.0;
  for (int i = 0; i < S; ++i) h += rhoTrans[i * C + c] * hc[i];
  src[c] = s + h * m.rdt;
}

// ------------------------------------------------------------------ Courant number
// compressibleCourantNo.H of OpenFOAM-7 (dfLowMachFoam.C:261): sumPhi = fvc::surfaceSum(mag(phi)) / rho,
// CoNum = 0.5 gMax(sumPhi / V) deltaT, meanCoNum = 0.5 (gSum(sumPhi) / gSum(V)) deltaT. One thread per cell sums
// |phi| over the cell's faces in the project's face order (every internal face for its owner and its neighbour, then
// the cell's primary boundary slots: a processor face adds this rank's flux only), divides by rho, and the block leaves
// (sum of sumPhi, max of sumPhi / V) at its LOGICAL block index (xcd_block), so the second stage adds the partials in
// cell order whatever the dispatch order. HBM-bound: per cell |phi| of its owned faces and, from the L2, of its
// neighbour-side faces, rho, V and the boundary-slot range. Threads past the last cell contribute the neutral 0 (every
// term is >= 0) and stay in the reduction: wave_sum needs the whole wave.
__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
template <int WT>
__global__ void __launch_bounds__(TPB) k_courant(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ phi,
                                                 const double* __restrict__ bphi, const double* __restrict__ rho,
                                                 double* __restrict__ partial) {
  __shared__ double sh[TPB / 64][2];
  const int lb = xcd_block();
  const int t = lb * blockDim.x + threadIdx.x;
  double sp = 0.0, ra = 0.0;
  if (t < m.C) {
    const int c = cell_of(m, t);
    double s = 0.0;
    each_face<WT>(m, c, [&](int f, int, bool) { s += fabs(phi[f]); });
    each_slot(m, ty, c, [&](int b, int) { s += fabs(bphi[b]); });
    sp = s / rho[c];
    ra = sp / m.V[c];
  }
  const double ws = wave_sum(sp), wm = wave_max(ra);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { sh[wid][0] = ws; sh[wid][1] = wm; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, mx = 0.0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) { a += sh[w][0]; mx = fmax(mx, sh[w][1]); }
    partial[2 * lb] = a;
    partial[2 * lb + 1] = mx;
  }
}
// the gathered per-rank (max, sum, volume) combined in rank order and posted to host-coherent pinned memory: plain
// stores, then `seq` with a system-scope release (the host spins on it, as on the solvers' PollRec)
__device__ __forceinline__ void courant_record(const double* __restrict__ tri, int nranks, double dt, CoRec* rec, long long seq) {
  double mx = 0.0, s = 0.0, v = 0.0;
  for (int r = 0; r < nranks; ++r) { mx = fmax(mx, tri[3 * r]); s += tri[3 * r + 1]; v += tri[3 * r + 2]; }
  rec->co = 0.5 * mx * dt;
  rec->mean = 0.5 * (s / v) * dt;
  __hip_atomic_store(&rec->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// second stage, one block: the per-block partials in a fixed order (thread i takes partials i, i + 256, ...; any
// count) -> this rank's (max, sum, volume); one rank: the record too
__global__ void __launch_bounds__(TPB) k_courant_reduce(const double* __restrict__ partial, int nblk, double sumV,
                                                        double* __restrict__ tri, CoRec* rec, double dt, long long seq) {
  __shared__ double sh[TPB / 64][2];
  double s = 0.0, mx = 0.0;
  for (int i = threadIdx.x; i < nblk; i += TPB) { s += partial[2 * i]; mx = fmax(mx, partial[2 * i + 1]); }
  const double ws = wave_sum(s), wm = wave_max(mx);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { sh[wid][0] = ws; sh[wid][1] = wm; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t3[3] = {0.0, 0.0, sumV};
#pragma unroll
  for (int w = 0; w < TPB / 64; ++w) { t3[1] += sh[w][0]; t3[0] = fmax(t3[0], sh[w][1]); }
  tri[0] = t3[0]; tri[1] = t3[1]; tri[2] = t3[2];
  if (rec) courant_record(t3, 1, dt, rec, seq);
}
__global__ void k_courant_combine(const double* __restrict__ all, int nranks, double dt, CoRec* rec, long long seq) {
  if (threadIdx.x == 0) courant_record(all, nranks, dt, rec, seq);
}

// ------------------------------------------------------------------ UEqn
// gradU (fvc_grad_vector :944-1107) -> T = mu*dev2(T(gradU)) (scale_dev2t_tensor_kernel :623) for
// cells, and for the cell's non-coupled slots the corrected boundary gradient (:1239-1327) -> bT.
__device__ __forceinline__ void dev2T(double sc, const double* v, double* o) {
  const double tr = (2. / 3.) * (v[0] + v[4] + v[8]);
  o[0] = sc * (v[0] - tr); o[1] = sc * v[3]; o[2] = sc * v[6];
  o[3] = sc * v[1]; o[4] = sc * (v[4] - tr); o[5] = sc * v[7];
  o[6] = sc * v[2]; o[7] = sc * v[5]; o[8] = sc * (v[8] - tr);
}

// g[3 i + j] = d_i U_j at cell c: the Gauss linear gradient (fvc_grad_vector), faces in sequential order, then the
// cell's boundary slots, / V -- the oracle's out_gradU (k_u_grad and the LES kernel k_les_nut share it)
template <int WT>
__device__ __forceinline__ void grad_u_cell(const MeshView& m, const int8_t* __restrict__ ty, const double* __restrict__ U,
                                            const double* __restrict__ bU, int c, double (&g)[9]) {
  const long C = m.C, F = m.F, B = m.B;
  double s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = 0.0;
  const double Uc[3] = {U[c], U[C + c], U[2 * C + c]};   // own-cell values in registers
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double w = m.w[f];
    double uf[3], sf[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double un = U[j * C + o2];
      uf[j] = own ? interp_f(w, Uc[j], un) : interp_f(w, un, Uc[j]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) sf[i] = m.Sf[i * F + f];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) { const double v = sf[i] * uf[j]; if (own) s[i * 3 + j] += v; else s[i * 3 + j] -= v; }
  });
  each_slot(m, ty, c, [&](int b, int t) {
    double uf[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) uf[j] = bface(m, t, U + j * C, bU + j * B, b, c);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) s[i * 3 + j] += m.bSf[i * B + b] * uf[j];
  });
  const double vol = m.V[c];
#pragma unroll
  for (int k = 0; k < 9; ++k) g[k] = s[k] / vol;
}

template <int WT>
__global__ void __launch_bounds__(TPB) DFMI_WAVES(6) k_u_grad(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ U,
                         const double* __restrict__ bU, const double* __restrict__ mu, const double* __restrict__ bmu,
                         double* __restrict__ T, double* __restrict__ bT, double* __restrict__ gout) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, B = m.B;
  double g[9], o[9];
  grad_u_cell<WT>(m, ty, U, bU, c, g);
  if (gout) {
#pragma unroll
    for (int k = 0; k < 9; ++k) gout[k * C + c] = g[k];
  }
  dev2T(mu[c], g, o);
#pragma unroll
  for (int k = 0; k < 9; ++k) T[k * C + c] = o[k];
  each_slot(m, ty, c, [&](int b, int t) {
    if (bc_coupled(t)) return;
    const double ms = m.bmagSf[b];
    const double nv[3] = {m.bSf[b] / ms, m.bSf[B + b] / ms, m.bSf[2 * B + b] / ms};
    double bg[9], bo[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double sn = (t == FIXED_VALUE || bc_mixed(t)) ? m.bdc[b] * (bU[j * B + b] - U[j * C + c]) : 0.0;
      const double corr = sn - (nv[0] * g[0 * 3 + j] + nv[1] * g[1 * 3 + j] + nv[2] * g[2 * 3 + j]);
#pragma unroll
      for (int i = 0; i < 3; ++i) bg[i * 3 + j] = g[i * 3 + j] + nv[i] * corr;
    }
    dev2T(bmu[b], bg, bo);
#pragma unroll
    for (int k = 0; k < 9; ++k) bT[k * B + b] = bo[k];
  });
}

// ------------------------------------------------------------------ LES eddy viscosity (turbulence->correct())
// OpenFOAM-7's LESeddyViscosity family per cell, from g = grad(U) (grad_u_cell: bitwise the UEqn's gradient), D = symm(g)
// and the filter width delta:
//   Smagorinsky (the formula of the reference's unused kernel, dfUEqn.cu:316-341): a = Ce / delta, b = (2/3) tr D,
//     c = 2 Ck delta (dev(D) && D), k = ((-b + sqrt(b^2 + 4 a c)) / (2 a))^2
//   WALE: Sd = dev(symm(g . g)), m = Sd && Sd, s = D && D,
//     k = (Cw^2 delta / Ck)^2 m^3 / ((s^(5/2) + m^(5/4))^2 + 1e-15)
//   nut = Ck delta sqrt(k)
// The powers are products and square roots (s^(5/2) = s s sqrt(s), m^(5/4) = m sqrt(sqrt(m))): no pow().
struct LesCoef { int model; double Ck, Ce, Cw; };
__device__ __forceinline__ double les_nut(const LesCoef& q, const double (&g)[9], double del) {
  const double D00 = g[0], D11 = g[4], D22 = g[8];
  const double D01 = 0.5 * (g[1] + g[3]), D02 = 0.5 * (g[2] + g[6]), D12 = 0.5 * (g[5] + g[7]);
  double k;
  if (q.model == 1) {
    const double tr = D00 + D11 + D22, t3 = (1.0 / 3.0) * tr;
    const double dd = ((D00 - t3) * D00 + (D11 - t3) * D11 + (D22 - t3) * D22) + 2.0 * (D01 * D01 + D02 * D02 + D12 * D12);
    const double a = q.Ce / del, b = (2.0 / 3.0) * tr, c = 2.0 * q.Ck * del * dd;
    const double r = (-b + sqrt(b * b + 4.0 * a * c)) / (2.0 * a);
    k = r * r;
  } else {
    double P[9];   // g . g
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) P[3 * i + j] = g[3 * i] * g[j] + g[3 * i + 1] * g[3 + j] + g[3 * i + 2] * g[6 + j];
    const double t3 = (1.0 / 3.0) * (P[0] + P[4] + P[8]);
    const double S00 = P[0] - t3, S11 = P[4] - t3, S22 = P[8] - t3;
    const double S01 = 0.5 * (P[1] + P[3]), S02 = 0.5 * (P[2] + P[6]), S12 = 0.5 * (P[5] + P[7]);
    const double mm = (S00 * S00 + S11 * S11 + S22 * S22) + 2.0 * (S01 * S01 + S02 * S02 + S12 * S12);
    const double ss = (D00 * D00 + D11 * D11 + D22 * D22) + 2.0 * (D01 * D01 + D02 * D02 + D12 * D12);
    const double s52 = ss * ss * sqrt(ss), m54 = mm * sqrt(sqrt(mm));
    const double den = s52 + m54, cw = q.Cw * q.Cw * del / q.Ck;
    k = (cw * cw) * (mm * mm * mm) / (den * den + 1e-15);
  }
  return q.Ck * del * sqrt(k);
}
// One thread per cell, k_u_grad's gather (U of the face neighbours, Sf and w of the cell's faces; the tensor in
// registers, no atomics) and 8 B out.
template <int WT>
__global__ void __launch_bounds__(TPB) k_les_nut(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ U,
                                                 const double* __restrict__ bU, const double* __restrict__ delta,
                                                 LesCoef q, double* __restrict__ nut) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  double g[9];
  grad_u_cell<WT>(m, ty, U, bU, c, g);
  nut[c] = les_nut(q, g, delta[c]);
}
// Sigma (the reference's Sigma.C:40-89; Nicoud et al. 2011), les.model = 4, a kernel of its own so that k_les_nut keeps
// its code: with the singular values s1 >= s2 >= s3 >= 0 of g,
//   Dsg = s3 (s1 - s2)(s2 - s3) / (s1^2 + 1e-300),  nut = (Csg delta)^2 Dsg
// The singular values come from one-sided (Hestenes) Jacobi on the columns of g in registers: g^T g is never formed and
// there is no acos, because the closed form from the invariants loses seven digits wherever two singular values meet
// or s3 is small -- the model's own zeros. One rotation of the columns p, q:
//   a = p.p, b = q.q, c = p.q;  c == 0: identity (g = 0, rank 1 and orthogonal columns come out exact);
//   z = (b - a) / (2 c), t = sign(z) / (|z| + sqrt(1 + z^2)), cs = 1 / sqrt(1 + t^2), sn = cs t,
//   p' = cs p - sn q, q' = sn p + cs q
// SIGMA_SWEEPS cyclic sweeps over (0,1), (0,2), (1,2), a fixed count: the fp64 restatement reaches rounding level
// (<= 1.5e-16 of s1 in Dsg) in 4 sweeps on every state class of tests/sgs_reference.py; 3 sweeps leave 2.0e-7 where s3
// is 1e-9 s1, 3.8e-7 where it is 0 and 1.6e-9 on random g (tests/golden/sgs_bounds.json "sweeps";
// tests/test_sgs_cpu.py); 4 plus one of margin.
constexpr int SIGMA_SWEEPS = 5;
__device__ __forceinline__ void sigma_rotate(double (&p)[3], double (&q)[3]) {
  const double a = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
  const double b = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
  const double c = p[0] * q[0] + p[1] * q[1] + p[2] * q[2];
  if (c == 0.0) return;
  const double z = (b - a) / (2.0 * c);
  const double t = copysign(1.0, z) / (fabs(z) + sqrt(1.0 + z * z));
  const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double pi = p[i], qi = q[i];
    p[i] = cs * pi - sn * qi;
    q[i] = sn * pi + cs * qi;
  }
}
__device__ __forceinline__ double sigma_nut(double Csg, const double (&g)[9], double del) {
  double c0[3] = {g[0], g[3], g[6]}, c1[3] = {g[1], g[4], g[7]}, c2[3] = {g[2], g[5], g[8]};   // the columns of g
  for (int s = 0; s < SIGMA_SWEEPS; ++s) {
    sigma_rotate(c0, c1);
    sigma_rotate(c0, c2);
    sigma_rotate(c1, c2);
  }
  const double n0 = sqrt(c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2]);
  const double n1 = sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
  const double n2 = sqrt(c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]);
  const double s1 = fmax(n0, fmax(n1, n2)), s3 = fmin(n0, fmin(n1, n2));
  const double s2 = fmax(fmin(n0, n1), fmin(fmax(n0, n1), n2));   // the true middle value
  const double Dsg = s3 * (s1 - s2) * (s2 - s3) / (s1 * s1 + 1e-300);
  const double cd = Csg * del;
  return cd * cd * Dsg;
}
// k_les_nut's gather, then the rotations in registers; 8 B out
template <int WT>
__global__ void __launch_bounds__(TPB) k_les_sigma(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ U,
                                                   const double* __restrict__ bU, const double* __restrict__ delta,
                                                   double Csg, double* __restrict__ nut) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  double g[9];
  grad_u_cell<WT>(m, ty, U, bU, c, g);
  nut[c] = sigma_nut(Csg, g, delta[c]);
}
// dynamicSmagorinsky (the reference's dynamicSmagorinsky.C:38-49, 141-199), les.model = 5: the statement in
// include/dfmi.h is the definition. Three per-cell gathers around one test filter.
//
// The filter (simpleFilter / fvc::average): F(x)_c = sum_f |Sf| x_f / sum_f |Sf| over the cell's faces in the sequential
// order, then its primary non-empty slots; x_f linear on internal and coupled faces, the slot's value elsewhere. N
// quantities at once, one accumulator each. It names none of its operands: cell(c, v) gives the N values of a cell,
// slot(b, t, own, v) those of boundary slot b of type t (a non-coupled slot's boundary values, or, on a processor
// slot, the neighbour cell's from the halo).
template <int WT, int N, class CELL, class SLOT>
__device__ __forceinline__ void les_filter(const MeshView& m, const int8_t* __restrict__ ty, int c, CELL&& cell, SLOT&& slot,
                                           double (&out)[N]) {
  double own[N], s[N], A = 0.0;
  cell(c, own);
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = 0.0;
  each_face<WT>(m, c, [&](int f, int o2, bool isown) {
    const double w = m.w[f], a = m.magSf[f];
    double nb[N];
    cell(o2, nb);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += a * (isown ? interp_f(w, own[k], nb[k]) : interp_f(w, nb[k], own[k]));
    A += a;
  });
  each_slot(m, ty, c, [&](int b, int t) {
    const double a = m.bmagSf[b];
    double xb[N];
    if (bc_coupled(t)) {
      const int pc = m.partner[b];
      if (pc >= 0) cell(pc, xb); else slot(b, t, own, xb);
      const double w = m.bw[b];
#pragma unroll
      for (int k = 0; k < N; ++k) xb[k] = interp_b(w, own[k], xb[k]);
    } else slot(b, t, own, xb);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += a * xb[k];
    A += a;
  });
#pragma unroll
  for (int k = 0; k < N; ++k) out[k] = s[k] / A;
}
// S = dev(symm(g)) as (xx, xy, xz, yy, yz, zz); && of two symmetric tensors in that storage
__device__ __forceinline__ void dev_symm(const double (&g)[9], double (&S)[6]) {
  const double t3 = (1.0 / 3.0) * (g[0] + g[4] + g[8]);
  S[0] = g[0] - t3; S[1] = 0.5 * (g[1] + g[3]); S[2] = 0.5 * (g[2] + g[6]);
  S[3] = g[4] - t3; S[4] = 0.5 * (g[5] + g[7]); S[5] = g[8] - t3;
}
__device__ __forceinline__ double sym_dd(const double* a, const double* b) {
  return (a[0] * b[0] + a[3] * b[3] + a[5] * b[5]) + 2.0 * (a[1] * b[1] + a[2] * b[2] + a[4] * b[4]);
}
// pass 1: g -> S on the cell and, from the boundary gradient k_u_grad forms (g_c + n (snGrad - n . g_c)), on its
// non-coupled slots
template <int WT>
__global__ void __launch_bounds__(TPB) k_dyn_strain(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ U,
                                                    const double* __restrict__ bU, double* __restrict__ S, double* __restrict__ bS) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, B = m.B;
  double g[9], s[6];
  grad_u_cell<WT>(m, ty, U, bU, c, g);
  dev_symm(g, s);
#pragma unroll
  for (int k = 0; k < 6; ++k) S[k * C + c] = s[k];
  each_slot(m, ty, c, [&](int b, int t) {
    if (bc_coupled(t)) return;
    const double ms = m.bmagSf[b];
    const double nv[3] = {m.bSf[b] / ms, m.bSf[B + b] / ms, m.bSf[2 * B + b] / ms};
    double bg[9], bs[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double sn = (t == FIXED_VALUE || bc_mixed(t)) ? m.bdc[b] * (bU[j * B + b] - U[j * C + c]) : 0.0;
      const double corr = sn - (nv[0] * g[0 * 3 + j] + nv[1] * g[1 * 3 + j] + nv[2] * g[2 * 3 + j]);
#pragma unroll
      for (int i = 0; i < 3; ++i) bg[i * 3 + j] = g[i * 3 + j] + nv[i] * corr;
    }
    dev_symm(bg, bs);
#pragma unroll
    for (int k = 0; k < 6; ++k) bS[k * B + b] = bs[k];
  });
}
// the 21 filtered quantities of pass 2 from a point's U (3) and S (6): U, U U (6), S, |S| S. Products are formed
// per point (cell or slot), then interpolated.
__device__ __forceinline__ void dyn_point(const double* __restrict__ U, const double* __restrict__ S, long n, long i, double* v) {
  const double u0 = U[i], u1 = U[n + i], u2 = U[2 * n + i];
  double s[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = S[k * n + i];
  const double ms = sqrt(sym_dd(s, s));
  v[0] = u0; v[1] = u1; v[2] = u2;
  v[3] = u0 * u0; v[4] = u0 * u1; v[5] = u0 * u2; v[6] = u1 * u1; v[7] = u1 * u2; v[8] = u2 * u2;
#pragma unroll
  for (int k = 0; k < 6; ++k) { v[9 + k] = s[k]; v[15 + k] = ms * s[k]; }
}
// pass 2: LL = dev(F(U U) - F(U) F(U)), MM = delta^2 (F(|S| S) - 4 |F(S)| F(S)); out LL && MM and MM && MM
template <int WT>
__global__ void __launch_bounds__(TPB) k_dyn_filter(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ U,
                                                    const double* __restrict__ bU, const double* __restrict__ S,
                                                    const double* __restrict__ bS, const double* __restrict__ delta,
                                                    double* __restrict__ llmm, double* __restrict__ mmmm) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, B = m.B;
  double F[21];
  les_filter<WT, 21>(m, ty, c, [&](int o, double* v) { dyn_point(U, S, C, o, v); },
                     [&](int b, int, const double*, double* v) { dyn_point(bU, bS, B, b, v); }, F);
  double LL[6], MM[6];
  LL[0] = F[3] - F[0] * F[0]; LL[1] = F[4] - F[0] * F[1]; LL[2] = F[5] - F[0] * F[2];
  LL[3] = F[6] - F[1] * F[1]; LL[4] = F[7] - F[1] * F[2]; LL[5] = F[8] - F[2] * F[2];
  const double t3 = (1.0 / 3.0) * (LL[0] + LL[3] + LL[5]);
  LL[0] -= t3; LL[3] -= t3; LL[5] -= t3;
  const double mfs = sqrt(sym_dd(F + 9, F + 9)), d2 = delta[c] * delta[c];
#pragma unroll
  for (int k = 0; k < 6; ++k) MM[k] = d2 * (F[15 + k] - 4.0 * mfs * F[9 + k]);
  llmm[c] = sym_dd(LL, MM);
  mmmm[c] = sym_dd(MM, MM);
}
// pass 3: LM = F(LL && MM), MMMM = max(F(MM && MM), 1e-300) (a non-coupled slot carries the cell's own value:
// surfaceSum returns an extrapolated field), Cs = 0.5 LM / MMMM, nut = max(Cs delta^2 |S|, -mu / rho)
template <int WT>
__global__ void __launch_bounds__(TPB) k_dyn_nut(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ llmm,
                                                 const double* __restrict__ bllmm, const double* __restrict__ mmmm,
                                                 const double* __restrict__ bmmmm, const double* __restrict__ S,
                                                 const double* __restrict__ delta, const double* __restrict__ mu,
                                                 const double* __restrict__ rho, double* __restrict__ LM, double* __restrict__ MMo,
                                                 double* __restrict__ Cs, double* __restrict__ nut) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C;
  double F[2];
  les_filter<WT, 2>(m, ty, c, [&](int o, double* v) { v[0] = llmm[o]; v[1] = mmmm[o]; },
                    [&](int b, int t, const double* own, double* v) {
                      if (bc_coupled(t)) { v[0] = bllmm[b]; v[1] = bmmmm[b]; } else { v[0] = own[0]; v[1] = own[1]; }
                    }, F);
  const double mm = fmax(F[1], 1e-300), cs = 0.5 * F[0] / mm;
  double s[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = S[k * C + c];
  const double d = delta[c];
  LM[c] = F[0]; MMo[c] = mm; Cs[c] = cs;
  nut[c] = fmax(cs * (d * d) * sqrt(sym_dd(s, s)), -mu[c] / rho[c]);
}
// mut = rho nut; muEff = mut + mu; alphaEff = alpha + mut / Prt; mutSct = mut / Sct (in this order, no contraction),
// over n cells or n boundary slots (each slot from its own boundary values)
__global__ void k_les_effective(long n, const double* __restrict__ rho, const double* __restrict__ nut,
                                const double* __restrict__ mu, const double* __restrict__ alpha, double Prt, double Sct,
                                double* __restrict__ muEff, double* __restrict__ alphaEff, double* __restrict__ mutSct) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double mut = rho[i] * nut[i];
  muEff[i] = mut + mu[i];
  alphaEff[i] = alpha[i] + mut / Prt;
  mutSct[i] = mut / Sct;
}

// UEqn matrix (UEqn.H:3-20): ddt(rho,U) + div(phi,U) - laplacian(mu,U) - div(mu dev2 T(gradU)),
// plus source_solve = source - grad(p) and rAU (dfUEqn.cu:721-738).
template <int WT>
__global__ void __launch_bounds__(TPB) DFMI_WAVES(5) k_u_assemble(MeshView m, const int8_t* __restrict__ tyU, const int8_t* __restrict__ tyP,
    const double* __restrict__ rho, const double* __restrict__ rho_old, const double* __restrict__ U_old,
    const double* __restrict__ bU, const double* __restrict__ phi, const double* __restrict__ bphi,
    const double* __restrict__ mu, const double* __restrict__ bmu, const double* __restrict__ p,
    const double* __restrict__ bp, const double* __restrict__ T, const double* __restrict__ bT,
    double* __restrict__ lower, double* __restrict__ upper, double* __restrict__ diag, double* __restrict__ src,
    double* __restrict__ srcs, double* __restrict__ ic, double* __restrict__ bc, double* __restrict__ rAU, MixBC mxU,
    const double* __restrict__ wU, const double* __restrict__ bwU) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, F = m.F, B = m.B;
  double d1 = 0.0, dL = 0.0;
  double dT[3] = {0.0, 0.0, 0.0}, gp[3] = {0.0, 0.0, 0.0};
  // the cell's own tensor, mu and p stay in registers; each face gathers only the other cell's values
  // (interp_f keeps its owner-first argument order, so the arithmetic is unchanged)
  double Tc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Tc[k] = T[k * C + c];
  const double muc = mu[c], pcc = p[c];
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double w = m.w[f], ph = phi[f];
    const double L1 = -(wU ? wU[f] : w) * ph;   // div(phi,U): linear, or limitedLinearV weights
    const double U1 = L1 + ph;
    const double mun = mu[o2];
    const double UL = m.dc[f] * ((own ? interp_f(w, muc, mun) : interp_f(w, mun, muc)) * m.magSf[f]);
    if (own) { d1 -= L1; st_out(&lower[f], L1 + (-UL)); st_out(&upper[f], U1 + (-UL)); }
    else d1 -= U1;
    dL -= UL;
    const double sf0 = m.Sf[f], sf1 = m.Sf[F + f], sf2 = m.Sf[2 * F + f];
    double Tn[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Tn[k] = T[k * C + o2];
    auto fi = [&](int k) { return own ? interp_f(w, Tc[k], Tn[k]) : interp_f(w, Tn[k], Tc[k]); };
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double v = sf0 * fi(0 + j) + sf1 * fi(3 + j) + sf2 * fi(6 + j);
      if (own) dT[j] += v; else dT[j] -= v;
    }
    const double pn = p[o2];
    const double pf = own ? interp_f(w, pcc, pn) : interp_f(w, pn, pcc);
    const double g0 = sf0 * pf, g1 = sf1 * pf, g2 = sf2 * pf;
    if (own) { gp[0] += g0; gp[1] += g1; gp[2] += g2; } else { gp[0] -= g0; gp[1] -= g1; gp[2] -= g2; }
  });
  // boundary contributions: explicit tensor divergence and the pressure gradient
  each_slot(m, tyU, c, [&](int b, int t) {
    double tt[9];
    if (bc_coupled(t)) {
      const int pc = m.partner[b];
#pragma unroll
      for (int k = 0; k < 9; ++k) tt[k] = interp_b(m.bw[b], T[k * C + c], pc >= 0 ? T[k * C + pc] : bT[k * B + b]);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) tt[k] = bT[k * B + b];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) dT[j] += m.bSf[b] * tt[0 + j] + m.bSf[B + b] * tt[3 + j] + m.bSf[2 * B + b] * tt[6 + j];
  });
  each_slot(m, tyP, c, [&](int b, int t) {
    const double pf = bface(m, t, p, bp, b, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) gp[k] += m.bSf[k * B + b] * pf;
  });
  const double vol = m.V[c];
  const double dg = (m.rdt * rho[c] * vol + d1) + (-dL);
  st_out(&diag[c], dg);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double s = m.rdt * rho_old[c] * U_old[k * C + c] * vol + dT[k];
    st_out(&src[k * C + c], s);
    st_out(&srcs[k * C + c], s - gp[k]);
  }
  double r = dg;
  each_slot(m, tyU, c, [&](int b, int t) {
    const double gam = bc_coupled(t) ? interp_b(m.bw[b], mu[c], nbrv(m, mu, bmu, b)) : bmu[b];
    const double pG = gam * m.bmagSf[b];
    double icv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const BCoef q = bcoef_f(t, bU[k * B + b], m.bw[b], m.bdc[b], mxU, b, B, k);
      const BCoef qc = bwU ? bcoef_f(t, bU[k * B + b], bwU[b], m.bdc[b], mxU, b, B, k) : q;   // convection weights
      icv[k] = bphi[b] * qc.vic + (-(pG * q.gic));
      st_out(&ic[k * B + b], icv[k]);
      bc[k * B + b] = -bphi[b] * qc.vbc + (-(-pG * q.gbc));
    }
    r += (icv[0] + icv[1] + icv[2]) / 3;
  });
  st_out(&rAU[c], 1 / (r / vol));
}

// K = 0.5*magSqr(U) on cells (boundary K is done per slot below)
__global__ void k_kinetic(int C, const double* __restrict__ U, double* __restrict__ K) {
  const int c = xcd_block() * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double x = U[c], y = U[(long)C + c], z = U[2L * C + c];
  K[c] = 0.5 * (x * x + y * y + z * z);
}

// HbyA: fvMatrix::H() / V (dfUEqn.cu:753-822), unscaled; rAU scaling and constrainHbyA follow.
template <int WT>
__global__ void __launch_bounds__(TPB) k_u_hbya(MeshView m, const int8_t* __restrict__ tyU, const double* __restrict__ U,
    const double* __restrict__ bU, const double* __restrict__ lower, const double* __restrict__ upper,
    const double* __restrict__ src, const double* __restrict__ ic, const double* __restrict__ bc,
    double* __restrict__ H) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, B = m.B;
  // one pass over the faces for the three components (each face's coefficient loaded once; every
  // component still sums its faces in order)
  double Hl[3] = {0.0, 0.0, 0.0};
  each_face<WT>(m, c, [&](int f, int oc, bool own) {
    const double a = own ? upper[f] : lower[f];
#pragma unroll
    for (int k = 0; k < 3; ++k) Hl[k] -= a * U[k * C + oc];
  });
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double* Uk = U + k * C;
    double bd = 0.0;
    each_slot(m, tyU, c, [&](int b, int) { bd += ic[k * B + b]; });
    bd = -bd;
    each_slot(m, tyU, c, [&](int b, int) { bd += (ic[b] + ic[B + b] + ic[2 * B + b]) / 3; });
    double h = bd * Uk[c] + (Hl[k] + src[k * C + c]);
    each_slot(m, tyU, c, [&](int b, int t) {
      h += bc_coupled(t) ? bc[k * B + b] * nbrv(m, Uk, bU + k * B, b) : bc[k * B + b];
    });
    H[k * C + c] = h / m.V[c];
  }
}

__global__ void k_hbya_scale_cells(int C, const double* __restrict__ rAU, double* __restrict__ H) {
  const int c = xcd_block() * blockDim.x + threadIdx.x;
  if (c >= C) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) H[(long)k * C + c] = rAU[c] * H[(long)k * C + c];
}
__global__ void k_hbya_scale_slots(int B, const int8_t* __restrict__ tyU, const double* __restrict__ brAU,
                                   const double* __restrict__ bU, double* __restrict__ bH) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double v = brAU[b] * bH[(long)k * B + b];
    if (tyU[b] == FIXED_VALUE) v = bU[(long)k * B + b];   // constrainHbyA
    bH[(long)k * B + b] = v;
  }
}

// ------------------------------------------------------------------ pEqn (dfpEqn.cu:379-546)
// per face: rhorAUf = interpolate(rho*rAU); phiHbyA = interpolate(rho)*flux(HbyA) + rhorAUf*ddtCorr;
// symmetric laplacian coefficients lower = upper = -dc*(rhorAUf*magSf).
__global__ void k_p_face(MeshView m, const double* __restrict__ rho, const double* __restrict__ rAU,
                         const double* __restrict__ rho_old, const double* __restrict__ U_old,
                         const double* __restrict__ phi_old, const double* __restrict__ H,
                         double* __restrict__ rf, double* __restrict__ ph, double* __restrict__ lower,
                         double* __restrict__ upper) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.F) return;
  const long C = m.C, F = m.F;
  const int o = m.own[f], n = m.nei[f];
  if (o < 0) return;   // padding slot of the owner-slot face storage
  const double w = m.w[f];
  const double r = interp_f(w, rho[o] * rAU[o], rho[n] * rAU[n]);
  rf[f] = r;
  const double sf0 = m.Sf[f], sf1 = m.Sf[F + f], sf2 = m.Sf[2 * F + f];
  const double ro = rho_old[o], rn = rho_old[n];
  const double phiCorr = phi_old[f] - (sf0 * interp_f(w, ro * U_old[o], rn * U_old[n]) +
                                       sf1 * interp_f(w, ro * U_old[C + o], rn * U_old[C + n]) +
                                       sf2 * interp_f(w, ro * U_old[2 * C + o], rn * U_old[2 * C + n]));
  const double coeff = 1.0 - fmin(fabs(phiCorr) / (fabs(phi_old[f]) + 1e-15), 1.0);
  const double ddtCorr = coeff * m.rdt * phiCorr;
  const double fl = sf0 * interp_f(w, H[o], H[n]) + sf1 * interp_f(w, H[C + o], H[C + n]) +
                    sf2 * interp_f(w, H[2 * C + o], H[2 * C + n]);
  ph[f] = interp_f(w, rho[o], rho[n]) * fl + r * ddtCorr;
  const double UL = m.dc[f] * (r * m.magSf[f]);
  lower[f] = -UL;
  upper[f] = -UL;
}

// Owner-slot face storage (f = k C + c): one thread per cell walks its owned face slots k, so the
// owner's nine values are loaded once instead of once per face (same per-face arithmetic as k_p_face,
// bitwise); writes stay coalesced per slot plane k.
__global__ void k_p_face_cell(MeshView m, const double* __restrict__ rho, const double* __restrict__ rAU,
                              const double* __restrict__ rho_old, const double* __restrict__ U_old,
                              const double* __restrict__ phi_old, const double* __restrict__ H,
                              double* __restrict__ rf, double* __restrict__ ph, double* __restrict__ lower,
                              double* __restrict__ upper) {
  const int c = xcd_block() * blockDim.x + threadIdx.x;
  if (c >= m.C) return;
  const long C = m.C, F = m.F;
  const int km = (int)(F / C);
  const double rho_c = rho[c], rr_c = rho_c * rAU[c], ro = rho_old[c];
  const double uo0 = ro * U_old[c], uo1 = ro * U_old[C + c], uo2 = ro * U_old[2 * C + c];
  const double h0 = H[c], h1 = H[C + c], h2 = H[2 * C + c];
  for (int k = 0; k < km; ++k) {
    const long f = k * C + c;
    if (m.own[f] < 0) continue;   // padding slot
    const int n = m.nei[f];
    const double w = m.w[f];
    const double r = interp_f(w, rr_c, rho[n] * rAU[n]);
    rf[f] = r;
    const double sf0 = m.Sf[f], sf1 = m.Sf[F + f], sf2 = m.Sf[2 * F + f];
    const double rn = rho_old[n];
    const double po = phi_old[f];
    const double phiCorr = po - (sf0 * interp_f(w, uo0, rn * U_old[n]) + sf1 * interp_f(w, uo1, rn * U_old[C + n]) +
                                 sf2 * interp_f(w, uo2, rn * U_old[2 * C + n]));
    const double coeff = 1.0 - fmin(fabs(phiCorr) / (fabs(po) + 1e-15), 1.0);
    const double ddtCorr = coeff * m.rdt * phiCorr;
    const double fl = sf0 * interp_f(w, h0, H[n]) + sf1 * interp_f(w, h1, H[C + n]) + sf2 * interp_f(w, h2, H[2 * C + n]);
    ph[f] = interp_f(w, rho_c, rho[n]) * fl + r * ddtCorr;
    const double UL = m.dc[f] * (r * m.magSf[f]);
    lower[f] = -UL;
    upper[f] = -UL;
  }
}

__global__ void k_p_slot(MeshView m, const int8_t* __restrict__ tyP, const int8_t* __restrict__ tyU,
                         const double* __restrict__ rho, const double* __restrict__ brho, const double* __restrict__ rAU,
                         const double* __restrict__ brAU, const double* __restrict__ rho_old,
                         const double* __restrict__ brho_old, const double* __restrict__ U_old,
                         const double* __restrict__ bU_old, const double* __restrict__ bphi_old,
                         const double* __restrict__ H, const double* __restrict__ bH, const double* __restrict__ bp,
                         double* __restrict__ brf, double* __restrict__ bph, double* __restrict__ ic,
                         double* __restrict__ bc, MixBC mxP, const double* __restrict__ bphi,
                         const double* __restrict__ bpsi, const double* __restrict__ gamma, double* __restrict__ wvf) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  const long C = m.C, B = m.B;
  const int t = tyP[b];
  if (!m.sprim[b] || t == EMPTY) { brf[b] = 0.0; bph[b] = 0.0; ic[b] = 0.0; bc[b] = 0.0; return; }
  const int c = m.bfc[b], pc = m.partner[b];
  const double bw = m.bw[b];
  double r;
  if (bc_coupled(t)) r = interp_b(bw, rho[c] * rAU[c], pc >= 0 ? rho[pc] * rAU[pc] : brho[b] * brAU[b]);
  else r = brho[b] * brAU[b];
  brf[b] = r;
  const int tu = tyU[b];
  double ruo[3], Hb[3], rb;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (bc_coupled(tu)) {
      const double rn = pc >= 0 ? rho_old[pc] * U_old[k * C + pc] : brho_old[b] * bU_old[k * B + b];
      ruo[k] = interp_b(bw, rho_old[c] * U_old[k * C + c], rn);
      Hb[k] = interp_b(bw, H[k * C + c], pc >= 0 ? H[k * C + pc] : bH[k * B + b]);
    } else { ruo[k] = brho_old[b] * bU_old[k * B + b]; Hb[k] = bH[k * B + b]; }
  }
  rb = bc_coupled(tu) ? interp_b(bw, rho[c], pc >= 0 ? rho[pc] : brho[b]) : brho[b];
  const double s0 = m.bSf[b], s1 = m.bSf[B + b], s2 = m.bSf[2 * B + b];
  const double phiCorr = bphi_old[b] - (s0 * ruo[0] + s1 * ruo[1] + s2 * ruo[2]);
  const double coeff = bc_fixes_value(tu) ? 0.0 : 1.0 - fmin(fabs(phiCorr) / (fabs(bphi_old[b]) + 1e-15), 1.0);
  const double fl = s0 * Hb[0] + s1 * Hb[1] + s2 * Hb[2];
  bph[b] = rb * fl + r * (coeff * m.rdt * phiCorr);
  BCoef q;
  if (t == WAVE_TRANSMISSIVE) {
    // waveTransmissiveFvPatchField::advectionSpeed = phi_p / (rho_p |Sf|) + sqrt(gamma / psi_p);
    // advectiveFvPatchField::updateCoeffs (Euler): valueFraction = 1 / (1 + w dt deltaCoeffs),
    // refValue = p.oldTime() on the patch
    const double wsp = fmax(bphi[b] / (brho[b] * m.bmagSf[b]) + sqrt(gamma[b] / bpsi[b]), 0.0);
    const double vf = 1.0 / (1.0 + wsp * (1.0 / m.rdt) * m.bdc[b]);
    wvf[b] = vf;
    q = bcoef_mixed(vf, mxP.wref[b], m.bdc[b]);
  } else q = bcoef_f(t, bp[b], bw, m.bdc[b], mxP, b, m.B, 0);
  const double pG = r * m.bmagSf[b];
  ic[b] = -(pG * q.gic);
  bc[b] = -(-pG * q.gbc);
}

template <int WT>
__global__ void k_p_cell(MeshView m, const int8_t* __restrict__ tyP, const double* __restrict__ lower,
                         const double* __restrict__ ph, const double* __restrict__ bph, const double* __restrict__ p,
                         const double* __restrict__ p_old, const double* __restrict__ psi, const double* __restrict__ rho,
                         const double* __restrict__ rho_old, double* __restrict__ diag, double* __restrict__ src) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  double dL = 0.0, div = 0.0;
  each_face<WT>(m, c, [&](int f, int, bool own) {
    dL -= -lower[f];
    if (own) div += ph[f]; else div -= ph[f];
  });
  each_slot(m, tyP, c, [&](int b, int) { div += bph[b]; });
  const double vol = m.V[c];
  double dg = m.rdt * vol;
  double sr = m.rdt * p_old[c] * vol;
  const double APsi = -dg * p[c] + sr;
  sr = sr - APsi;
  sr = sr * psi[c];
  dg = dg * psi[c];
  sr = sr - vol * (m.rdt * (rho[c] - rho_old[c]));
  sr = sr - div;
  src[c] = sr;
  diag[c] = dg - dL;
}

// after the p solve: phi = phiHbyA + pEqn.flux() (lduMatrix::faceH + fvMatrix::flux boundary)
__global__ void k_p_flux_face(MeshView m, const double* __restrict__ ph, const double* __restrict__ lower,
                              const double* __restrict__ upper, const double* __restrict__ p, double* __restrict__ phi) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.F) return;
  const int o = m.own[f];
  if (o < 0) return;
  phi[f] = ph[f] + (upper[f] * p[m.nei[f]] - lower[f] * p[o]);
}
__global__ void k_p_flux_slot(MeshView m, const int8_t* __restrict__ tyP, const double* __restrict__ bph,
                              const double* __restrict__ ic, const double* __restrict__ bc, const double* __restrict__ p,
                              const double* __restrict__ bp, double* __restrict__ bphi) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  const int t = tyP[b];
  if (!m.sprim[b]) { bphi[b] = 0.0; return; }
  if (t == EMPTY) return;
  const int c = m.bfc[b];
  const double fl = bc_coupled(t) ? ic[b] * p[c] - bc[b] * nbrv(m, p, bp, b) : ic[b] * p[c] - bc[b];
  bphi[b] = bph[b] + fl;
}
// U = HbyA - rAU*grad(p); K; dpdt
// PHI: the walk also writes phi of the cell's owned faces, k_p_flux_face's expression with the p values it gathers
// anyway (every internal face is owned by exactly one cell, so the two kernels write the same faces)
template <int WT, bool PHI>
__device__ __forceinline__ void p_cell_post(const MeshView& m, const int8_t* __restrict__ tyP, const double* __restrict__ p,
                              const double* __restrict__ bp, const double* __restrict__ p_old,
                              const double* __restrict__ H, const double* __restrict__ rAU, double* __restrict__ U,
                              double* __restrict__ K, double* __restrict__ dpdt, const double* __restrict__ ph,
                              const double* __restrict__ lower, const double* __restrict__ upper,
                              double* __restrict__ phi) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, F = m.F, B = m.B;
  double g[3] = {0.0, 0.0, 0.0};
  const double pcc = p[c];
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double pn = p[o2];
    if constexpr (PHI) { if (own) phi[f] = ph[f] + (upper[f] * pn - lower[f] * pcc); }
    const double pf = own ? interp_f(m.w[f], pcc, pn) : interp_f(m.w[f], pn, pcc);
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double v = m.Sf[k * F + f] * pf; if (own) g[k] += v; else g[k] -= v; }
  });
  each_slot(m, tyP, c, [&](int b, int t) {
    const double pf = bface(m, t, p, bp, b, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] += m.bSf[k * B + b] * pf;
  });
  const double vol = m.V[c];
  double u[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { u[k] = H[k * C + c] - rAU[c] * (g[k] / vol); U[k * C + c] = u[k]; }
  K[c] = 0.5 * (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  dpdt[c] = m.rdt * (p[c] - p_old[c]);
}
template <int WT>
__global__ void k_p_cell_post(MeshView m, const int8_t* __restrict__ tyP, const double* __restrict__ p,
                              const double* __restrict__ bp, const double* __restrict__ p_old,
                              const double* __restrict__ H, const double* __restrict__ rAU, double* __restrict__ U,
                              double* __restrict__ K, double* __restrict__ dpdt) {
  p_cell_post<WT, false>(m, tyP, p, bp, p_old, H, rAU, U, K, dpdt, nullptr, nullptr, nullptr, nullptr);
}
template <int WT>
__global__ void k_p_cell_post_phi(MeshView m, const int8_t* __restrict__ tyP, const double* __restrict__ p,
                                  const double* __restrict__ bp, const double* __restrict__ p_old,
                                  const double* __restrict__ H, const double* __restrict__ rAU, double* __restrict__ U,
                                  double* __restrict__ K, double* __restrict__ dpdt, const double* __restrict__ ph,
                                  const double* __restrict__ lower, const double* __restrict__ upper,
                                  double* __restrict__ phi) {
  p_cell_post<WT, true>(m, tyP, p, bp, p_old, H, rAU, U, K, dpdt, ph, lower, upper, phi);
}
__global__ void k_kinetic_slots(int B, const double* __restrict__ bU, double* __restrict__ bK) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double x = bU[b], y = bU[(long)B + b], z = bU[2L * B + b];
  bK[b] = 0.5 * (x * x + y * y + z * z);
}

// ------------------------------------------------------------------ YEqn preparation (YEqn.H:24-118)
// per cell: grad(Y_s), sumYDiffError, hDiffCorrFlux, diffAlphaD; per non-coupled slot of the cell:
// corrected boundary gradients -> boundary sumYDiffError / hDiffCorrFlux.
// the rest of k_y_prep for cell c once its face and slot sums are in: gradients / V, sumYDiffError,
// hDiffCorrFlux, diffAlphaD, and the non-coupled slots' boundary fields (shared with the brick kernel)
// (hc: the cell's own hai values, held by the caller)
template <int S>
__device__ __forceinline__ void y_prep_tail(const MeshView& m, const int8_t* __restrict__ tyY, const double* __restrict__ Y,
    const double* __restrict__ bY, const double* __restrict__ rhoD, const double* __restrict__ brhoD,
    const double (&hc)[S], const double* __restrict__ bhai, double* __restrict__ sumE,
    double* __restrict__ bsumE, double* __restrict__ hD, double* __restrict__ bhD, double* __restrict__ dAD,
    double* __restrict__ gout, int c, double (&g)[S][3], const double (&lap)[S], const double (&yc)[S]) {
  const long C = m.C, B = m.B;
  const double vol = m.V[c];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < 3; ++k) g[s][k] = g[s][k] / vol;
  if (gout) {
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int k = 0; k < 3; ++k) gout[(3L * s + k) * C + c] = g[s][k];
  }
  double se[3], hd[3], rd[S];
#pragma unroll
  for (int s = 0; s < S; ++s) rd[s] = rhoD[s * C + c];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double a = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) a += rd[s] * g[s][k];
    se[k] = a;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double a = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) a += hc[s] * (rd[s] * g[s][k] - yc[s] * se[k]);
    hd[k] = a;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { sumE[k * C + c] = se[k]; hD[k * C + c] = hd[k]; }
  double dad = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s) dad = dad + lap[s] / vol;
  dAD[c] = dad;
  // boundary fields of the non-coupled slots (coupled slots interpolate cell values downstream)
  each_slot(m, tyY, c, [&](int b, int t) {
    if (bc_coupled(t)) return;
    const double ms = m.bmagSf[b];
    const double nv[3] = {m.bSf[b] / ms, m.bSf[B + b] / ms, m.bSf[2 * B + b] / ms};
    double bg[S][3];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double sn = (t == FIXED_VALUE || t == CALCULATED || t == FIXED_ENERGY || bc_mixed(t)) ? m.bdc[b] * (bY[s * B + b] - Y[s * C + c]) : 0.0;
      const double corr = sn - (nv[0] * g[s][0] + nv[1] * g[s][1] + nv[2] * g[s][2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) bg[s][k] = g[s][k] + nv[k] * corr;
    }
    double bse[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double a = 0.0;
#pragma unroll
      for (int s = 0; s < S; ++s) a += brhoD[s * B + b] * bg[s][k];
      bse[k] = a;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double a = 0.0;
#pragma unroll
      for (int s = 0; s < S; ++s)
        a += bhai[s * B + b] * (brhoD[s * B + b] * bg[s][k] - bY[s * B + b] * bse[k]);
      bsumE[k * B + b] = bse[k];
      bhD[k * B + b] = a;
    }
  });
}

template <int S, int WT>
__global__ void __launch_bounds__(TPB) k_y_prep(MeshView m, const int8_t* __restrict__ tyY, const double* __restrict__ Y,
    const double* __restrict__ bY, const double* __restrict__ rhoD, const double* __restrict__ brhoD,
    const double* __restrict__ hai, const double* __restrict__ bhai, const double* __restrict__ alpha,
    const double* __restrict__ balpha, double* __restrict__ sumE, double* __restrict__ bsumE,
    double* __restrict__ hD, double* __restrict__ bhD, double* __restrict__ dAD, double* __restrict__ gout) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, F = m.F, B = m.B;
  // One pass over the cell's faces computes every species' Gauss gradient AND its diffAlphaD
  // laplacian term (the two per-species face loops of the sequential code fused; each accumulator
  // still sums in face order, so the result is bitwise the sequential one). Own-cell values live
  // in registers; each face loads the neighbour's Y_s and hai_s once.
  double g[S][3], lap[S], yc[S], ahc[S];
  const double ac = alpha[c];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    g[s][0] = 0.0; g[s][1] = 0.0; g[s][2] = 0.0; lap[s] = 0.0;
    yc[s] = Y[s * C + c];
    ahc[s] = ac * hai[s * C + c];
  }
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double w = m.w[f], sf0 = m.Sf[f], sf1 = m.Sf[F + f], sf2 = m.Sf[2 * F + f];
    const double ms = m.magSf[f], dcf = m.dc[f];
    const double an = alpha[o2];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double yn = Y[s * C + o2];
      const double ahn = an * hai[s * C + o2];
      const double yf = own ? interp_f(w, yc[s], yn) : interp_f(w, yn, yc[s]);
      const double v0 = sf0 * yf, v1 = sf1 * yf, v2 = sf2 * yf;
      const double gam = own ? interp_f(w, ahc[s], ahn) : interp_f(w, ahn, ahc[s]);
      const double dy = own ? yn - yc[s] : yc[s] - yn;
      const double v = gam * ms * (dcf * dy);
      if (own) { g[s][0] += v0; g[s][1] += v1; g[s][2] += v2; lap[s] += v; }
      else { g[s][0] -= v0; g[s][1] -= v1; g[s][2] -= v2; lap[s] -= v; }
    }
  });
  each_slot(m, tyY, c, [&](int b, int t) {
    const double bs0 = m.bSf[b], bs1 = m.bSf[B + b], bs2 = m.bSf[2 * B + b];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double yf = bface(m, t, Y + s * C, bY + s * B, b, c);
      g[s][0] += bs0 * yf; g[s][1] += bs1 * yf; g[s][2] += bs2 * yf;
      double v;
      if (bc_coupled(t)) {
        const int pc = m.partner[b];
        const double an = pc >= 0 ? alpha[pc] * hai[s * C + pc] : balpha[b] * bhai[s * B + b];
        v = interp_b(m.bw[b], ahc[s], an) * m.bmagSf[b] * (m.bdc[b] * (nbrv(m, Y + s * C, bY + s * B, b) - yc[s]));
      } else {
        const double sng = (t == FIXED_VALUE || t == CALCULATED || t == FIXED_ENERGY || bc_mixed(t)) ? m.bdc[b] * (bY[s * B + b] - yc[s]) : 0.0;
        v = balpha[b] * bhai[s * B + b] * m.bmagSf[b] * sng;
      }
      lap[s] += v;
    }
  });
  double hc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) hc[s] = hai[s * C + c];
  y_prep_tail<S>(m, tyY, Y, bY, rhoD, brhoD, hc, bhai, sumE, bsumE, hD, bhD, dAD, gout, c, g, lap, yc);
}

// k_y_prep on a hex box in blockMesh order (MeshView::hx), one YBX x YBY x YBZ brick of cells per
// workgroup: Y_s and alpha hai_s of the brick and of its face-adjacent halo are staged in LDS with
// coalesced loads (SC species at a time), and every face term reads its neighbour from LDS instead of
// two dependent global gathers per species -- the north star's "face contributions staged in LDS". The
// faces, their order and every product are those of k_y_prep<S, -1> (alpha hai formed at staging is the
// same product), so the results are bitwise the face walk's.
constexpr int YBX = 16, YBY = 4, YBZ = 4;
constexpr int YPY = YBX + 2, YPZ = (YBX + 2) * (YBY + 2), YNB = YPZ * (YBZ + 2);
static_assert(YBX * YBY * YBZ == TPB, "one thread per brick cell");
template <int S, int SC>
__global__ void __launch_bounds__(TPB) k_y_prep_brick(MeshView m, const int8_t* __restrict__ tyY, const double* __restrict__ Y,
    const double* __restrict__ bY, const double* __restrict__ rhoD, const double* __restrict__ brhoD,
    const double* __restrict__ hai, const double* __restrict__ bhai, const double* __restrict__ alpha,
    const double* __restrict__ balpha, double* __restrict__ sumE, double* __restrict__ bsumE,
    double* __restrict__ hD, double* __restrict__ bhD, double* __restrict__ dAD, double* __restrict__ gout) {
  constexpr int NCH = (S + SC - 1) / SC;
  __shared__ double sY[SC][YNB], sA[SC][YNB];
  const int nx = m.hx, ny = m.hy, nz = m.hz;
  const int nbx = nx / YBX, nby = ny / YBY;
  const int bid = xcd_block();
  const int bx = bid % nbx, bt = bid / nbx, by = bt % nby, bz = bt / nby;
  const int i0 = bx * YBX, j0 = by * YBY, k0 = bz * YBZ;
  const int t = threadIdx.x;
  const int li = t % YBX, lj = (t / YBX) % YBY, lk = t / (YBX * YBY);
  const int c = (i0 + li) + nx * ((j0 + lj) + ny * (k0 + lk));
  const int me = (li + 1) + YPY * (lj + 1) + YPZ * (lk + 1);
  const long C = m.C, F = m.F, B = m.B;
  double g[S][3], lap[S], yc[S], ahc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) { g[s][0] = 0.0; g[s][1] = 0.0; g[s][2] = 0.0; lap[s] = 0.0; }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int s0 = ch * SC;
    if (ch > 0) __syncthreads();   // every thread done with the previous chunk's values
    for (int p = t; p < YNB; p += TPB) {   // the brick and its face halo (edges and corners have no face)
      const int a = p % YPY, b = (p / YPY) % (YBY + 2), d = p / YPZ;
      const int oa = (a == 0 || a == YBX + 1), ob = (b == 0 || b == YBY + 1), od = (d == 0 || d == YBZ + 1);
      if (oa + ob + od > 1) continue;
      const int gi = i0 + a - 1, gj = j0 + b - 1, gk = k0 + d - 1;
      if (gi < 0 || gi >= nx || gj < 0 || gj >= ny || gk < 0 || gk >= nz) continue;
      const long gc = gi + (long)nx * (gj + (long)ny * gk);
      const double al = alpha[gc];
#pragma unroll
      for (int q = 0; q < SC; ++q)
        if (s0 + q < S) { sY[q][p] = Y[(s0 + q) * C + gc]; sA[q][p] = al * hai[(s0 + q) * C + gc]; }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SC; ++q)
      if (s0 + q < S) { yc[s0 + q] = sY[q][me]; ahc[s0 + q] = sA[q][me]; }
    each_face<-1>(m, c, [&](int f, int o2, bool own) {
      const int dd = o2 - c;
      const int lo = me + (dd == 1 ? 1 : dd == -1 ? -1 : dd == nx ? YPY : dd == -nx ? -YPY : dd > 0 ? YPZ : -YPZ);
      const double w = m.w[f], sf0 = m.Sf[f], sf1 = m.Sf[F + f], sf2 = m.Sf[2 * F + f];
      const double ms = m.magSf[f], dcf = m.dc[f];
#pragma unroll
      for (int q = 0; q < SC; ++q) {
        if (s0 + q >= S) continue;
        const int s = s0 + q;
        const double yn = sY[q][lo];
        const double ahn = sA[q][lo];
        const double yf = own ? interp_f(w, yc[s], yn) : interp_f(w, yn, yc[s]);
        const double v0 = sf0 * yf, v1 = sf1 * yf, v2 = sf2 * yf;
        const double gam = own ? interp_f(w, ahc[s], ahn) : interp_f(w, ahn, ahc[s]);
        const double dy = own ? yn - yc[s] : yc[s] - yn;
        const double v = gam * ms * (dcf * dy);
        if (own) { g[s][0] += v0; g[s][1] += v1; g[s][2] += v2; lap[s] += v; }
        else { g[s][0] -= v0; g[s][1] -= v1; g[s][2] -= v2; lap[s] -= v; }
      }
    });
  }
  each_slot(m, tyY, c, [&](int b, int tt) {
    const double bs0 = m.bSf[b], bs1 = m.bSf[B + b], bs2 = m.bSf[2 * B + b];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double yf = bface(m, tt, Y + s * C, bY + s * B, b, c);
      g[s][0] += bs0 * yf; g[s][1] += bs1 * yf; g[s][2] += bs2 * yf;
      double v;
      if (bc_coupled(tt)) {
        const int pc = m.partner[b];
        const double an = pc >= 0 ? alpha[pc] * hai[s * C + pc] : balpha[b] * bhai[s * B + b];
        v = interp_b(m.bw[b], ahc[s], an) * m.bmagSf[b] * (m.bdc[b] * (nbrv(m, Y + s * C, bY + s * B, b) - yc[s]));
      } else {
        const double sng = (tt == FIXED_VALUE || tt == CALCULATED || tt == FIXED_ENERGY || bc_mixed(tt)) ? m.bdc[b] * (bY[s * B + b] - yc[s]) : 0.0;
        v = balpha[b] * bhai[s * B + b] * m.bmagSf[b] * sng;
      }
      lap[s] += v;
    }
  });
  double hc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) hc[s] = hai[s * C + c];
  y_prep_tail<S>(m, tyY, Y, bY, rhoD, brhoD, hc, bhai, sumE, bsumE, hD, bhD, dAD, gout, c, g, lap, yc);
}
// species per staged chunk: all (S <= 5) or about half (LDS 2 SC YNB doubles: 9 species -> 5 = 52 KiB)
constexpr int ybrick_sc(int S) { return S <= 5 ? S : (S + 1) / 2; }



// phiUc = linearInterpolate(sumYDiffError) & Sf
__global__ void k_phiuc_face(MeshView m, const double* __restrict__ sumE, double* __restrict__ phiUc) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.F) return;
  const long C = m.C, F = m.F;
  const int o = m.own[f], n = m.nei[f];
  if (o < 0) return;
  const double w = m.w[f];
  phiUc[f] = m.Sf[f] * interp_f(w, sumE[o], sumE[n]) + m.Sf[F + f] * interp_f(w, sumE[C + o], sumE[C + n]) +
             m.Sf[2 * F + f] * interp_f(w, sumE[2 * C + o], sumE[2 * C + n]);
}
__global__ void k_phiuc_slot(MeshView m, const int8_t* __restrict__ tyY, const double* __restrict__ sumE,
                             const double* __restrict__ bsumE, double* __restrict__ bphiUc) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  const long C = m.C, B = m.B;
  const int t = tyY[b];
  if (!m.sprim[b] || t == EMPTY) { bphiUc[b] = 0.0; return; }
  const int c = m.bfc[b];
  double e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    e[k] = bc_coupled(t) ? interp_b(m.bw[b], sumE[k * C + c], nbrv(m, sumE + k * C, bsumE + k * B, b)) : bsumE[k * B + b];
  bphiUc[b] = m.bSf[b] * e[0] + m.bSf[B + b] * e[1] + m.bSf[2 * B + b] * e[2];
}

// Y species matrices, all non-inert species in one pass (dfYEqn.cu:571-638 fused and batched):
// fvm::ddt(rho,Yi) + div(phi,Yi) + div(phiUc,Yi) == laplacian(rhoD_i,Yi) + RR_i
// LES (the launchers' les.model != 0): DEff_i = rhoD_i + mut / Sct wherever rhoD is read, and no phiUc term. A separate
// instantiation whose extra arguments (mut / Sct on cells and slots) exist only there, so the laminar kernels keep
// their arguments, code and registers (profiles/les_resource_usage.md)
template <bool LES> struct LesDiff {};
template <> struct LesDiff<true> { const double *mS, *bmS; };
// the slot's correction-velocity flux: absent in LES mode
template <bool LES> __device__ __forceinline__ double bpu(const double* __restrict__ bphiUc, int b) {
  if constexpr (LES) return 0.0;
  else return bphiUc[b];
}
template <int S, int WT, bool LES = false>
__global__ void __launch_bounds__(TPB) k_y_assemble(MeshView m, const int8_t* __restrict__ tyY, int inert,
    const double* __restrict__ Y, const double* __restrict__ bY, const double* __restrict__ rhoD,
    const double* __restrict__ brhoD, const double* __restrict__ RR, const double* __restrict__ rho,
    const double* __restrict__ rho_old, const double* __restrict__ phi, const double* __restrict__ bphi,
    const double* __restrict__ phiUc, const double* __restrict__ bphiUc, double* __restrict__ lower,
    double* __restrict__ upper, double* __restrict__ diag, double* __restrict__ src, double* __restrict__ ic,
    double* __restrict__ bc, MixBC mxY, const double* __restrict__ wY, const double* __restrict__ bwY,
    LesDiff<LES> ld) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, F = m.F, B = m.B;
  double d1 = 0.0, d2 = 0.0;
  double dL[S], rc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) { dL[s] = 0.0; rc[s] = rhoD[s * C + c]; }
  if constexpr (LES) {   // LES: DEff_i = rhoD_i + mut / Sct wherever rhoD is read
    const double mc = ld.mS[c];
#pragma unroll
    for (int s = 0; s < S; ++s) rc[s] = rc[s] + mc;
  }
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double ph = phi[f], pu = LES ? 0.0 : phiUc[f];   // LES: no correction-velocity convection (YEqn.H:101-106)
    double mn = 0.0;
    if constexpr (LES) mn = ld.mS[o2];
    const double wu = wY ? wY[f] : (ph >= 0 ? 1.0 : 0.0);
    const double L1 = -wu * ph, U1 = L1 + ph;
    const double L2 = -wu * pu, U2 = L2 + pu;
    if (own) { d1 -= L1; d2 -= L2; } else { d1 -= U1; d2 -= U2; }
    const double w = m.w[f], dcf = m.dc[f], ms = m.magSf[f];
    const double Ls = L1 + L2, Us = U1 + U2;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (s == inert) continue;
      const double rn = LES ? rhoD[s * C + o2] + mn : rhoD[s * C + o2];
      const double UL = dcf * ((own ? interp_f(w, rc[s], rn) : interp_f(w, rn, rc[s])) * ms);
      dL[s] -= UL;
      if (own) { lower[s * F + f] = Ls - UL; upper[s * F + f] = Us - UL; }
    }
  });
  const double vol = m.V[c];
  const double dd = m.rdt * rho[c] * vol + (d1 + d2);
  const double ro = m.rdt * rho_old[c];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s == inert) continue;
    diag[s * C + c] = dd - dL[s];
    src[s * C + c] = ro * Y[s * C + c] * vol + vol * RR[s * C + c];
  }
  each_slot(m, tyY, c, [&](int b, int t) {
    const double wu = bwY ? bwY[b] : upwind_b(m, bphi, b);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (s == inert) continue;
      const BCoef qc = bcoef_f(t, bY[s * B + b], wu, m.bdc[b], mxY, b, B, s);
      const BCoef ql = bcoef_f(t, bY[s * B + b], m.bw[b], m.bdc[b], mxY, b, B, s);
      double gam;
      if constexpr (LES) {
        const int pn = m.partner[b];
        gam = bc_coupled(t) ? interp_b(m.bw[b], rhoD[s * C + c] + ld.mS[c], pn >= 0 ? rhoD[s * C + pn] + ld.mS[pn] : brhoD[s * B + b] + ld.bmS[b])
                 : brhoD[s * B + b] + ld.bmS[b];
      } else gam = bc_coupled(t) ? interp_b(m.bw[b], rhoD[s * C + c], nbrv(m, rhoD + s * C, brhoD + s * B, b)) : brhoD[s * B + b];
      const double pG = gam * m.bmagSf[b];
      ic[s * B + b] = (bphi[b] * qc.vic + bpu<LES>(bphiUc, b) * qc.vic) - pG * ql.gic;
      bc[s * B + b] = (-bphi[b] * qc.vbc + -bpu<LES>(bphiUc, b) * qc.vbc) - (-pG * ql.gbc);
    }
  });
}

// The same YEqn assembly, emitted directly in the solver's ELL layout (production path): per
// system (non-inert species) the row values [W][C] in the gather order (neighbour faces, owned
// faces, coupled slots), dS = diag + sum internalCoeffs and rhs = source + non-coupled
// boundaryCoeffs in slot order -- bitwise what k_ell_build makes from the LDU arrays, without writing
// and re-reading lower/upper/internalCoeffs/boundaryCoeffs.
template <int S, int WT, bool LES = false>
__global__ void __launch_bounds__(TPB) DFMI_WAVES(5) k_y_assemble_ell(MeshView m, const int8_t* __restrict__ tyY, int inert,
    const double* __restrict__ Y, const double* __restrict__ bY, const double* __restrict__ rhoD,
    const double* __restrict__ brhoD, const double* __restrict__ RR, const double* __restrict__ rho,
    const double* __restrict__ rho_old, const double* __restrict__ phi, const double* __restrict__ bphi,
    const double* __restrict__ phiUc, const double* __restrict__ bphiUc, int W, long Ce, double* __restrict__ val,
    double* __restrict__ dS, double* __restrict__ rhs, MixBC mxY, const double* __restrict__ wY,
    const double* __restrict__ bwY, LesDiff<LES> ld) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const int pc = m.eopos ? m.eopos[c] : c;   // the solver row of c (even-odd layout)
  const long C = m.C, B = m.B;
  double d1 = 0.0, d2 = 0.0;
  double dL[S], rc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) { dL[s] = 0.0; rc[s] = rhoD[s * C + c]; }
  if constexpr (LES) {   // LES: DEff_i = rhoD_i + mut / Sct wherever rhoD is read
    const double mc = ld.mS[c];
#pragma unroll
    for (int s = 0; s < S; ++s) rc[s] = rc[s] + mc;
  }
  int k = 0;
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double ph = phi[f], pu = LES ? 0.0 : phiUc[f];   // LES: no correction-velocity convection (YEqn.H:101-106)
    double mn = 0.0;
    if constexpr (LES) mn = ld.mS[o2];
    const double wu = wY ? wY[f] : (ph >= 0 ? 1.0 : 0.0);
    const double L1 = -wu * ph, U1 = L1 + ph;
    const double L2 = -wu * pu, U2 = L2 + pu;
    if (own) { d1 -= L1; d2 -= L2; } else { d1 -= U1; d2 -= U2; }
    const double w = m.w[f], dcf = m.dc[f], ms = m.magSf[f];
    const double Ls = L1 + L2, Us = U1 + U2;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (s == inert) continue;
      const int ss = s < inert ? s : s - 1;
      const double rn = LES ? rhoD[s * C + o2] + mn : rhoD[s * C + o2];
      const double UL = dcf * ((own ? interp_f(w, rc[s], rn) : interp_f(w, rn, rc[s])) * ms);
      dL[s] -= UL;
      st_drop(&val[((long)ss * W + k) * C + pc], own ? Us - UL : Ls - UL);
    }
    ++k;
  });
  const double vol = m.V[c];
  const double dd = m.rdt * rho[c] * vol + (d1 + d2);
  const double ro = m.rdt * rho_old[c];
  double dg[S], sr[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    dg[s] = dd - dL[s];
    sr[s] = ro * Y[s * C + c] * vol + vol * RR[s * C + c];
  }
  each_slot(m, tyY, c, [&](int b, int t) {
    const double wu = bwY ? bwY[b] : upwind_b(m, bphi, b);
    const bool cp = bc_coupled(t);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (s == inert) continue;
      const int ss = s < inert ? s : s - 1;
      const BCoef qc = bcoef_f(t, bY[s * B + b], wu, m.bdc[b], mxY, b, B, s);
      const BCoef ql = bcoef_f(t, bY[s * B + b], m.bw[b], m.bdc[b], mxY, b, B, s);
      double gam;
      if constexpr (LES) {
        const int pn = m.partner[b];
        gam = cp ? interp_b(m.bw[b], rhoD[s * C + c] + ld.mS[c], pn >= 0 ? rhoD[s * C + pn] + ld.mS[pn] : brhoD[s * B + b] + ld.bmS[b])
                 : brhoD[s * B + b] + ld.bmS[b];
      } else gam = cp ? interp_b(m.bw[b], rhoD[s * C + c], nbrv(m, rhoD + s * C, brhoD + s * B, b)) : brhoD[s * B + b];
      const double pG = gam * m.bmagSf[b];
      const double icv = (bphi[b] * qc.vic + bpu<LES>(bphiUc, b) * qc.vic) - pG * ql.gic;
      const double bcv = (-bphi[b] * qc.vbc + -bpu<LES>(bphiUc, b) * qc.vbc) - (-pG * ql.gbc);
      dg[s] += icv;
      if (cp) st_drop(&val[((long)ss * W + k) * C + pc], -bcv);
      else sr[s] += bcv;
    }
    if (cp) ++k;
  });
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s == inert) continue;
    const int ss = s < inert ? s : s - 1;
    for (int kk = k; kk < W; ++kk) st_drop(&val[((long)ss * W + kk) * C + pc], 0.0);
    st_drop(&dS[ss * Ce + pc], dg[s]);
    st_drop(&rhs[ss * Ce + pc], sr[s]);
  }
}


template <int S>
__global__ void k_y_inert(int C, int inert, double* __restrict__ Y) {
  const int c = xcd_block() * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double sum = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s == inert) continue;
    double yi = Y[(long)s * C + c];
    yi = yi > 0 ? yi : 0;
    Y[(long)s * C + c] = yi;
    sum += yi;
  }
  sum = 1 - sum;
  Y[(long)inert * C + c] = sum > 0 ? sum : 0;
}


// ------------------------------------------------------------------ species-generic Y kernels
// Mechanisms beyond the register-resident templates (S > 16, e.g. GRI-scale 53 species, BASELINE
// config 4): the species loop runs in chunks of CH species held in registers. Every per-species
// accumulator (gradient, laplacian, matrix coefficients) depends on its own species only, and every
// cross-species sum (sumYDiffError, hDiffCorrFlux, diffAlphaD and their boundary fields) is carried
// across chunks in species order, so the results are bitwise those of the sequential restatement
// (oracle y_prep / y_assemble) -- the same sums in the same order. hDiffCorrFlux needs the finished
// sumYDiffError, so a second pass re-forms the gradients chunk by chunk (neighbour values come from
// L2 the second time; cheaper than spilling S x 3 gradients per cell to HBM).
constexpr int YCH = 8;
constexpr int YPREP_LCH = 8, YASM_LCH = 8;   // species per launch of the chunked y_prep / y_assemble_ell kernels

// gradient (and, with LAP, the diffAlphaD laplacian) of species s0 .. s0+CH-1 at cell c, divided by V
template <int CH, bool LAP, int WT>
__device__ __forceinline__ void y_chunk_grad(const MeshView& m, const int8_t* __restrict__ tyY, int S, int s0, int c,
    const double* __restrict__ Y, const double* __restrict__ bY, const double* __restrict__ hai,
    const double* __restrict__ bhai, const double* __restrict__ alpha, const double* __restrict__ balpha, double ac,
    double (&g)[CH][3], double (&lap)[CH], double (&yc)[CH]) {
  const long C = m.C, F = m.F, B = m.B;
  double ahc[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int s = s0 + j;
    g[j][0] = 0.0; g[j][1] = 0.0; g[j][2] = 0.0; lap[j] = 0.0;
    yc[j] = s < S ? Y[s * C + c] : 0.0;
    ahc[j] = (LAP && s < S) ? ac * hai[s * C + c] : 0.0;
  }
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double w = m.w[f], sf0 = m.Sf[f], sf1 = m.Sf[F + f], sf2 = m.Sf[2 * F + f];
    const double ms = m.magSf[f], dcf = m.dc[f];
    const double an = LAP ? alpha[o2] : 0.0;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int s = s0 + j;
      if (s >= S) break;
      const double yn = Y[s * C + o2];
      const double yf = own ? interp_f(w, yc[j], yn) : interp_f(w, yn, yc[j]);
      const double v0 = sf0 * yf, v1 = sf1 * yf, v2 = sf2 * yf;
      if (own) { g[j][0] += v0; g[j][1] += v1; g[j][2] += v2; } else { g[j][0] -= v0; g[j][1] -= v1; g[j][2] -= v2; }
      if (LAP) {
        const double ahn = an * hai[s * C + o2];
        const double gam = own ? interp_f(w, ahc[j], ahn) : interp_f(w, ahn, ahc[j]);
        const double dy = own ? yn - yc[j] : yc[j] - yn;
        const double v = gam * ms * (dcf * dy);
        if (own) lap[j] += v; else lap[j] -= v;
      }
    }
  });
  each_slot(m, tyY, c, [&](int b, int t) {
    const double bs0 = m.bSf[b], bs1 = m.bSf[B + b], bs2 = m.bSf[2 * B + b];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int s = s0 + j;
      if (s >= S) break;
      const double yf = bface(m, t, Y + s * C, bY + s * B, b, c);
      g[j][0] += bs0 * yf; g[j][1] += bs1 * yf; g[j][2] += bs2 * yf;
      if (LAP) {
        double v;
        if (bc_coupled(t)) {
          const int pc = m.partner[b];
          const double an = pc >= 0 ? alpha[pc] * hai[s * C + pc] : balpha[b] * bhai[s * B + b];
          v = interp_b(m.bw[b], ahc[j], an) * m.bmagSf[b] * (m.bdc[b] * (nbrv(m, Y + s * C, bY + s * B, b) - yc[j]));
        } else {
          const double sng = (t == FIXED_VALUE || t == CALCULATED || t == FIXED_ENERGY || bc_mixed(t)) ? m.bdc[b] * (bY[s * B + b] - yc[j]) : 0.0;
          v = balpha[b] * bhai[s * B + b] * m.bmagSf[b] * sng;
        }
        lap[j] += v;
      }
    }
  });
  const double vol = m.V[c];
#pragma unroll
  for (int j = 0; j < CH; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) g[j][k] = g[j][k] / vol;
}

// corrected gradient of the chunk's species on a non-coupled slot b of cell c (fvc_grad ... correctBC)
template <int CH>
__device__ __forceinline__ void y_chunk_bgrad(const MeshView& m, int t, int b, int S, int s0, int c,
                                              const double* __restrict__ Y, const double* __restrict__ bY,
                                              const double (&g)[CH][3], double (&bg)[CH][3]) {
  const long C = m.C, B = m.B;
  const double ms = m.bmagSf[b];
  const double nv[3] = {m.bSf[b] / ms, m.bSf[B + b] / ms, m.bSf[2 * B + b] / ms};
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int s = s0 + j;
    if (s >= S) break;
    const double sn = (t == FIXED_VALUE || t == CALCULATED || t == FIXED_ENERGY || bc_mixed(t)) ? m.bdc[b] * (bY[s * B + b] - Y[s * C + c]) : 0.0;
    const double corr = sn - (nv[0] * g[j][0] + nv[1] * g[j][1] + nv[2] * g[j][2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) bg[j][k] = g[j][k] + nv[k] * corr;
  }
}

// One launch covers the species [s_lo, s_hi) of one pass (pass 2 needs the finished sumYDiffError). The
// cross-species sums are carried between launches in their output arrays (sumE / dAD, hD, and the boundary
// fields as before), in species order, so any split is bitwise the single launch. The split is for locality:
// a thread walking all S species keeps every species' Y / alpha*hai / rhoD of the cells in flight live in L2
// (2 waves per SIMD: 16k cells per XCD x 53 species x 3 arrays = 20 MB against its 4 MB), so each neighbour
// value is fetched again by each of the cells that read it; a range of species per launch shrinks that set.
template <int CH, int WT>
__global__ void __launch_bounds__(TPB) DFMI_WAVES(4) k_y_prep_gen(MeshView m, int s_lo, int s_hi, int pass,
    const int8_t* __restrict__ tyY,
    const double* __restrict__ Y, const double* __restrict__ bY, const double* __restrict__ rhoD,
    const double* __restrict__ brhoD, const double* __restrict__ hai, const double* __restrict__ bhai,
    const double* __restrict__ alpha, const double* __restrict__ balpha, double* __restrict__ sumE,
    double* __restrict__ bsumE, double* __restrict__ hD, double* __restrict__ bhD, double* __restrict__ dAD,
    double* __restrict__ gout) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, B = m.B;
  const int S = s_hi;   // species bound of this launch
  const double ac = alpha[c], vol = m.V[c];
  double se[3] = {0.0, 0.0, 0.0}, dad = 0.0;
  if (pass == 1) {
  if (s_lo > 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) se[k] = sumE[k * C + c];
    dad = dAD[c];
  }
  // pass 1: gradients + laplacians -> sumYDiffError, diffAlphaD; boundary sumYDiffError summed in place
  for (int s0 = s_lo; s0 < s_hi; s0 += CH) {
    double g[CH][3], lap[CH], yc[CH];
    y_chunk_grad<CH, true, WT>(m, tyY, S, s0, c, Y, bY, hai, bhai, alpha, balpha, ac, g, lap, yc);
    if (gout) {
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (s0 + j < S)
#pragma unroll
          for (int k = 0; k < 3; ++k) gout[(3L * (s0 + j) + k) * C + c] = g[j][k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (s0 + j < S) se[k] += rhoD[(s0 + j) * C + c] * g[j][k];
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (s0 + j < S) dad = dad + lap[j] / vol;
    each_slot(m, tyY, c, [&](int b, int t) {
      if (bc_coupled(t)) return;
      double bg[CH][3];
      y_chunk_bgrad<CH>(m, t, b, S, s0, c, Y, bY, g, bg);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double a = s0 == 0 ? 0.0 : bsumE[k * B + b];
#pragma unroll
        for (int j = 0; j < CH; ++j)
          if (s0 + j < S) a += brhoD[(s0 + j) * B + b] * bg[j][k];
        bsumE[k * B + b] = a;
      }
    });
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) sumE[k * C + c] = se[k];
  dAD[c] = dad;
  return;
  }
  // pass 2: hDiffCorrFlux = sum_i hai_i (rhoD_i grad Y_i - Y_i sumYDiffError) (and on the slots)
#pragma unroll
  for (int k = 0; k < 3; ++k) se[k] = sumE[k * C + c];
  double hd[3] = {0.0, 0.0, 0.0};
  if (s_lo > 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) hd[k] = hD[k * C + c];
  }
  for (int s0 = s_lo; s0 < s_hi; s0 += CH) {
    double g[CH][3], lap[CH], yc[CH];
    y_chunk_grad<CH, false, WT>(m, tyY, s_hi, s0, c, Y, bY, hai, bhai, alpha, balpha, ac, g, lap, yc);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int s = s0 + j;
        if (s < S) hd[k] += hai[s * C + c] * (rhoD[s * C + c] * g[j][k] - yc[j] * se[k]);
      }
    each_slot(m, tyY, c, [&](int b, int t) {
      if (bc_coupled(t)) return;
      double bg[CH][3];
      y_chunk_bgrad<CH>(m, t, b, S, s0, c, Y, bY, g, bg);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double bse = bsumE[k * B + b];
        double a = s0 == 0 ? 0.0 : bhD[k * B + b];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int s = s0 + j;
          if (s < S) a += bhai[s * B + b] * (brhoD[s * B + b] * bg[j][k] - bY[s * B + b] * bse);
        }
        bhD[k * B + b] = a;
      }
    });
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) hD[k * C + c] = hd[k];
}

// YEqn matrices, chunked over species (LDU form: the dfmi_assemble("Y") inspection path)
template <int CH, int WT, bool LES = false>
__global__ void __launch_bounds__(TPB) k_y_assemble_gen(MeshView m, int S, const int8_t* __restrict__ tyY, int inert,
    const double* __restrict__ Y, const double* __restrict__ bY, const double* __restrict__ rhoD,
    const double* __restrict__ brhoD, const double* __restrict__ RR, const double* __restrict__ rho,
    const double* __restrict__ rho_old, const double* __restrict__ phi, const double* __restrict__ bphi,
    const double* __restrict__ phiUc, const double* __restrict__ bphiUc, double* __restrict__ lower,
    double* __restrict__ upper, double* __restrict__ diag, double* __restrict__ src, double* __restrict__ ic,
    double* __restrict__ bc, MixBC mxY, const double* __restrict__ wY, const double* __restrict__ bwY,
    LesDiff<LES> ld) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, F = m.F, B = m.B;
  const double vol = m.V[c];
  for (int s0 = 0; s0 < S; s0 += CH) {
    double d1 = 0.0, d2 = 0.0;
    double dL[CH], rc[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { dL[j] = 0.0; rc[j] = s0 + j < S ? rhoD[(s0 + j) * C + c] : 0.0; }
    if constexpr (LES) {   // LES: DEff_i = rhoD_i + mut / Sct wherever rhoD is read
      const double mc = ld.mS[c];
#pragma unroll
      for (int j = 0; j < CH; ++j) rc[j] = rc[j] + mc;
    }
    each_face<WT>(m, c, [&](int f, int o2, bool own) {
      const double ph = phi[f], pu = LES ? 0.0 : phiUc[f];   // LES: no correction-velocity convection (YEqn.H:101-106)
      double mn = 0.0;
      if constexpr (LES) mn = ld.mS[o2];
      const double wu = wY ? wY[f] : (ph >= 0 ? 1.0 : 0.0);
      const double L1 = -wu * ph, U1 = L1 + ph;
      const double L2 = -wu * pu, U2 = L2 + pu;
      if (own) { d1 -= L1; d2 -= L2; } else { d1 -= U1; d2 -= U2; }
      const double w = m.w[f], dcf = m.dc[f], ms = m.magSf[f];
      const double Ls = L1 + L2, Us = U1 + U2;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int s = s0 + j;
        if (s >= S) break;
        if (s == inert) continue;
        const double rn = LES ? rhoD[s * C + o2] + mn : rhoD[s * C + o2];
        const double UL = dcf * ((own ? interp_f(w, rc[j], rn) : interp_f(w, rn, rc[j])) * ms);
        dL[j] -= UL;
        if (own) { lower[s * F + f] = Ls - UL; upper[s * F + f] = Us - UL; }
      }
    });
    const double dd = m.rdt * rho[c] * vol + (d1 + d2);
    const double ro = m.rdt * rho_old[c];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int s = s0 + j;
      if (s >= S) break;
      if (s == inert) continue;
      diag[s * C + c] = dd - dL[j];
      src[s * C + c] = ro * Y[s * C + c] * vol + vol * RR[s * C + c];
    }
    each_slot(m, tyY, c, [&](int b, int t) {
      const double wu = bwY ? bwY[b] : upwind_b(m, bphi, b);
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int s = s0 + j;
        if (s >= S) break;
        if (s == inert) continue;
        const BCoef qc = bcoef_f(t, bY[s * B + b], wu, m.bdc[b], mxY, b, B, s);
        const BCoef ql = bcoef_f(t, bY[s * B + b], m.bw[b], m.bdc[b], mxY, b, B, s);
        double gam;
        if constexpr (LES) {
          const int pn = m.partner[b];
          gam = bc_coupled(t) ? interp_b(m.bw[b], rhoD[s * C + c] + ld.mS[c], pn >= 0 ? rhoD[s * C + pn] + ld.mS[pn] : brhoD[s * B + b] + ld.bmS[b])
                   : brhoD[s * B + b] + ld.bmS[b];
        } else gam = bc_coupled(t) ? interp_b(m.bw[b], rhoD[s * C + c], nbrv(m, rhoD + s * C, brhoD + s * B, b)) : brhoD[s * B + b];
        const double pG = gam * m.bmagSf[b];
        ic[s * B + b] = (bphi[b] * qc.vic + bpu<LES>(bphiUc, b) * qc.vic) - pG * ql.gic;
        bc[s * B + b] = (-bphi[b] * qc.vbc + -bpu<LES>(bphiUc, b) * qc.vbc) - (-pG * ql.gbc);
      }
    });
  }
}

// YEqn in the solver's ELL rows, chunked over species (production path for S > 16)
// One launch covers the species [s_lo, s_hi) (the species are independent here; split for L2 locality of the
// neighbour rhoD gathers, as k_y_prep_gen)
template <int CH, int WT, bool LES = false>
__global__ void __launch_bounds__(TPB) k_y_assemble_ell_gen(MeshView m, int s_lo, int S, const int8_t* __restrict__ tyY, int inert,
    const double* __restrict__ Y, const double* __restrict__ bY, const double* __restrict__ rhoD,
    const double* __restrict__ brhoD, const double* __restrict__ RR, const double* __restrict__ rho,
    const double* __restrict__ rho_old, const double* __restrict__ phi, const double* __restrict__ bphi,
    const double* __restrict__ phiUc, const double* __restrict__ bphiUc, int W, long Ce, double* __restrict__ val,
    double* __restrict__ dS, double* __restrict__ rhs, MixBC mxY, const double* __restrict__ wY,
    const double* __restrict__ bwY, LesDiff<LES> ld) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const int pc = m.eopos ? m.eopos[c] : c;   // the solver row of c (even-odd layout)
  const long C = m.C, B = m.B;
  const double vol = m.V[c];
  for (int s0 = s_lo; s0 < S; s0 += CH) {
    double d1 = 0.0, d2 = 0.0;
    double dL[CH], rc[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { dL[j] = 0.0; rc[j] = s0 + j < S ? rhoD[(s0 + j) * C + c] : 0.0; }
    if constexpr (LES) {   // LES: DEff_i = rhoD_i + mut / Sct wherever rhoD is read
      const double mc = ld.mS[c];
#pragma unroll
      for (int j = 0; j < CH; ++j) rc[j] = rc[j] + mc;
    }
    int k = 0;
    each_face<WT>(m, c, [&](int f, int o2, bool own) {
      const double ph = phi[f], pu = LES ? 0.0 : phiUc[f];   // LES: no correction-velocity convection (YEqn.H:101-106)
      double mn = 0.0;
      if constexpr (LES) mn = ld.mS[o2];
      const double wu = wY ? wY[f] : (ph >= 0 ? 1.0 : 0.0);
      const double L1 = -wu * ph, U1 = L1 + ph;
      const double L2 = -wu * pu, U2 = L2 + pu;
      if (own) { d1 -= L1; d2 -= L2; } else { d1 -= U1; d2 -= U2; }
      const double w = m.w[f], dcf = m.dc[f], ms = m.magSf[f];
      const double Ls = L1 + L2, Us = U1 + U2;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int s = s0 + j;
        if (s >= S) break;
        if (s == inert) continue;
        const int ss = s < inert ? s : s - 1;
        const double rn = LES ? rhoD[s * C + o2] + mn : rhoD[s * C + o2];
        const double UL = dcf * ((own ? interp_f(w, rc[j], rn) : interp_f(w, rn, rc[j])) * ms);
        dL[j] -= UL;
        val[((long)ss * W + k) * C + pc] = own ? Us - UL : Ls - UL;
      }
      ++k;
    });
    const double dd = m.rdt * rho[c] * vol + (d1 + d2);
    const double ro = m.rdt * rho_old[c];
    double dg[CH], sr[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int s = s0 + j;
      dg[j] = dd - dL[j];
      sr[j] = s < S ? ro * Y[s * C + c] * vol + vol * RR[s * C + c] : 0.0;
    }
    each_slot(m, tyY, c, [&](int b, int t) {
      const double wu = bwY ? bwY[b] : upwind_b(m, bphi, b);
      const bool cp = bc_coupled(t);
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int s = s0 + j;
        if (s >= S) break;
        if (s == inert) continue;
        const int ss = s < inert ? s : s - 1;
        const BCoef qc = bcoef_f(t, bY[s * B + b], wu, m.bdc[b], mxY, b, B, s);
        const BCoef ql = bcoef_f(t, bY[s * B + b], m.bw[b], m.bdc[b], mxY, b, B, s);
        double gam;
        if constexpr (LES) {
          const int pn = m.partner[b];
          gam = cp ? interp_b(m.bw[b], rhoD[s * C + c] + ld.mS[c], pn >= 0 ? rhoD[s * C + pn] + ld.mS[pn] : brhoD[s * B + b] + ld.bmS[b])
                   : brhoD[s * B + b] + ld.bmS[b];
        } else gam = cp ? interp_b(m.bw[b], rhoD[s * C + c], nbrv(m, rhoD + s * C, brhoD + s * B, b)) : brhoD[s * B + b];
        const double pG = gam * m.bmagSf[b];
        const double icv = (bphi[b] * qc.vic + bpu<LES>(bphiUc, b) * qc.vic) - pG * ql.gic;
        const double bcv = (-bphi[b] * qc.vbc + -bpu<LES>(bphiUc, b) * qc.vbc) - (-pG * ql.gbc);
        dg[j] += icv;
        if (cp) val[((long)ss * W + k) * C + pc] = -bcv;
        else sr[j] += bcv;
      }
      if (cp) ++k;
    });
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int s = s0 + j;
      if (s >= S) break;
      if (s == inert) continue;
      const int ss = s < inert ? s : s - 1;
      for (int kk = k; kk < W; ++kk) val[((long)ss * W + kk) * C + pc] = 0.0;
      dS[ss * Ce + pc] = dg[j];
      rhs[ss * Ce + pc] = sr[j];
    }
  }
}

__global__ void k_y_inert_gen(int C, int S, int inert, double* __restrict__ Y) {
  const int c = xcd_block() * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double sum = 0;
  for (int s = 0; s < S; ++s) {
    if (s == inert) continue;
    double yi = Y[(long)s * C + c];
    yi = yi > 0 ? yi : 0;
    Y[(long)s * C + c] = yi;
    sum += yi;
  }
  sum = 1 - sum;
  Y[(long)inert * C + c] = sum > 0 ? sum : 0;
}

// ------------------------------------------------------------------ EEqn (EEqn.H:12-45; dfEEqn.cu:108-264)
template <int WT>
__global__ void __launch_bounds__(TPB) k_e_assemble(MeshView m, const int8_t* __restrict__ tyH, const int8_t* __restrict__ tyK,
    const double* __restrict__ he, const double* __restrict__ bhe, const double* __restrict__ rho,
    const double* __restrict__ rho_old, const double* __restrict__ K, const double* __restrict__ K_old,
    const double* __restrict__ bK, const double* __restrict__ phi, const double* __restrict__ bphi,
    const double* __restrict__ alpha, const double* __restrict__ balpha, const double* __restrict__ hD,
    const double* __restrict__ bhD, const double* __restrict__ dpdt, const double* __restrict__ dAD,
    const double* __restrict__ egrad, double* __restrict__ lower, double* __restrict__ upper,
    double* __restrict__ diag, double* __restrict__ src, double* __restrict__ ic, double* __restrict__ bc,
    const double* __restrict__ wY, const double* __restrict__ bwY, const double* __restrict__ wK,
    const double* __restrict__ bwK, const double* __restrict__ cf, const double* __restrict__ bcf) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, F = m.F, B = m.B;
  double d1 = 0.0, dL = 0.0, divK = 0.0, divh = 0.0;
  const double ac = alpha[c], Kc = K[c], hc0 = hD[c], hc1 = hD[C + c], hc2 = hD[2 * C + c];   // own cell
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double ph = phi[f], w = m.w[f];
    auto fi = [&](double vc, double vn) { return own ? interp_f(w, vc, vn) : interp_f(w, vn, vc); };
    const double wu = wY ? wY[f] : (ph >= 0 ? 1.0 : 0.0);
    const double L1 = -wu * ph, U1 = L1 + ph;
    const double UL = m.dc[f] * (fi(ac, alpha[o2]) * m.magSf[f]);
    if (own) { d1 -= L1; lower[f] = L1 - UL; upper[f] = U1 - UL; } else d1 -= U1;
    dL -= UL;
    const double wk = wK ? wK[f] : w;   // div(phi,K): limited weights, or linear
    const double vk = ph * (own ? interp_f(wk, Kc, K[o2]) : interp_f(wk, K[o2], Kc));
    double vh = m.Sf[f] * fi(hc0, hD[o2]) + m.Sf[F + f] * fi(hc1, hD[C + o2]) +
                m.Sf[2 * F + f] * fi(hc2, hD[2 * C + o2]);
    if (cf) vh = vh + cf[f];            // div(hDiffCorrFlux) cubic: + Sf & correction
    if (own) { divK += vk; divh += vh; } else { divK -= vk; divh -= vh; }
  });
  each_slot(m, tyK, c, [&](int b, int t) {
    const double kb = (wK && bc_coupled(t)) ? interp_b(bwK[b], Kc, nbrv(m, K, bK, b)) : bface(m, t, K, bK, b, c);
    divK += bphi[b] * kb;
  });
  each_slot(m, tyH, c, [&](int b, int t) {
    double h[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) h[k] = bface(m, t, hD + k * C, bhD + k * B, b, c);
    double v = m.bSf[b] * h[0] + m.bSf[B + b] * h[1] + m.bSf[2 * B + b] * h[2];
    if (bcf && bc_coupled(t)) v = v + bcf[b];
    divh += v;
  });
  const double vol = m.V[c];
  diag[c] = (m.rdt * rho[c] * vol + d1) - dL;
  double sL = m.rdt * rho_old[c] * he[c] * vol;
  sL = sL - vol * (m.rdt * (rho[c] * K[c] - rho_old[c] * K_old[c]));
  sL = sL - divK;
  sL = sL + vol * dpdt[c];
  double sR = vol * dAD[c];
  sR = sR - divh;
  src[c] = sL - sR;
  each_slot(m, tyH, c, [&](int b, int t) {
    const double eg = egrad ? egrad[b] : 0.0;
    const BCoef qc = bcoef(t, bhe[b], bwY ? bwY[b] : (bphi[b] >= 0 ? 1.0 : 0.0), m.bdc[b], eg);
    const BCoef ql = bcoef(t, bhe[b], m.bw[b], m.bdc[b], eg);
    const double gam = bc_coupled(t) ? interp_b(m.bw[b], alpha[c], nbrv(m, alpha, balpha, b)) : balpha[b];
    const double pG = gam * m.bmagSf[b];
    ic[b] = bphi[b] * qc.vic - pG * ql.gic;
    bc[b] = -bphi[b] * qc.vbc - (-pG * ql.gbc);
  });
}

// ------------------------------------------------------------------ RAS k-epsilon (include/dfmi.h)
// OpenFOAM-7 kEpsilon::correct() / correctNut() / bound() as the header states them. Every kernel is a per-cell
// gather or a pointwise pass: one accumulator per term, faces in the sequential order, no atomics, no pow().
struct RasCoef { double Cmu, C1, C2, C3, sigmak, sigmaEps, kMin, epsMin; };

// dd = dev(twoSymm(g)) && g with T = g + g^T, t3 = (1/3) tr T:
//   ((T00 - t3) g00 + (T11 - t3) g11 + (T22 - t3) g22) + ((T01 g01 + T01 g10) + (T02 g02 + T02 g20) + (T12 g12 + T12 g21))
__device__ __forceinline__ double ras_dev_two_symm_dd(const double (&g)[9]) {
  const double T00 = g[0] + g[0], T11 = g[4] + g[4], T22 = g[8] + g[8];
  const double T01 = g[1] + g[3], T02 = g[2] + g[6], T12 = g[5] + g[7];
  const double t3 = (1.0 / 3.0) * ((T00 + T11) + T22);
  const double dg = ((T00 - t3) * g[0] + (T11 - t3) * g[4]) + (T22 - t3) * g[8];
  const double off = ((T01 * g[1] + T01 * g[3]) + (T02 * g[2] + T02 * g[6])) + (T12 * g[5] + T12 * g[7]);
  return dg + off;
}
// G = nut (dev(twoSymm(g)) && g) and divU = fvc::div(phi / interpolate(rho)) per cell: grad_u_cell's gather (bitwise the
// UEqn's gradient), then a second walk over the same faces for the volumetric flux (phi, rho of the face neighbours;
// the slots' face density by rho's patch types: the stored value, or the interpolate on a coupled slot). Both are
// written out, 16 B per cell: the epsilon and the k assembly read them with a solve in between.
template <int WT>
__global__ void __launch_bounds__(TPB) k_ras_production(MeshView m, const int8_t* __restrict__ tyU, const int8_t* __restrict__ tyR,
    const double* __restrict__ U, const double* __restrict__ bU, const double* __restrict__ phi,
    const double* __restrict__ bphi, const double* __restrict__ rho, const double* __restrict__ brho,
    const double* __restrict__ nut, double* __restrict__ G, double* __restrict__ divU) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  double g[9];
  grad_u_cell<WT>(m, tyU, U, bU, c, g);
  const double rc = rho[c];
  double dv = 0.0;
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double w = m.w[f], rn = rho[o2];
    const double v = phi[f] / (own ? interp_f(w, rc, rn) : interp_f(w, rn, rc));
    if (own) dv += v; else dv -= v;
  });
  each_slot(m, tyR, c, [&](int b, int t) { dv += bphi[b] / bface(m, t, rho, brho, b, c); });
  divU[c] = dv / m.V[c];
  G[c] = nut[c] * ras_dev_two_symm_dd(g);
}

// D = rho (nut / sigma + mu / rho) over n cells or n boundary slots (each slot from its own boundary values)
__device__ __forceinline__ double ras_diff(double rho, double nut, double mu, double sigma) {
  return rho * (nut / sigma + mu / rho);
}
__global__ void k_ras_diffusivity(long n, const double* __restrict__ rho, const double* __restrict__ nut,
                                  const double* __restrict__ mu, double sigma, double* __restrict__ D) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  D[i] = ras_diff(rho[i], nut[i], mu[i], sigma);
}
// explicit source Su and implicit coefficient Sp (per unit volume) of one of the two equations, and its cell diffusivity:
//   epsilon (keq = 0): a = (((2/3) C1 - C3) rho) divU;  Su = ((C1 rho) G) (eps / k) - min(a, 0) eps;  Sp = max(a, 0) + (C2 rho) (eps / k)
//   k       (keq = 1): a = ((2/3) rho) divU;            Su = rho G - min(a, 0) k;                     Sp = max(a, 0) + rho (eps / k)
__global__ void k_ras_sources(long n, int keq, RasCoef q, const double* __restrict__ G, const double* __restrict__ divU,
                              const double* __restrict__ rho, const double* __restrict__ k, const double* __restrict__ eps,
                              const double* __restrict__ nut, const double* __restrict__ mu, double* __restrict__ Su,
                              double* __restrict__ Sp, double* __restrict__ D) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double r = rho[i], kc = k[i], ec = eps[i], ek = ec / kc;
  if (keq) {
    const double a = ((2.0 / 3.0) * r) * divU[i];
    Su[i] = r * G[i] - fmin(a, 0.0) * kc;
    Sp[i] = fmax(a, 0.0) + r * ek;
    D[i] = ras_diff(r, nut[i], mu[i], q.sigmak);
  } else {
    const double a = (((2.0 / 3.0) * q.C1 - q.C3) * r) * divU[i];
    Su[i] = ((q.C1 * r) * G[i]) * ek - fmin(a, 0.0) * ec;
    Sp[i] = fmax(a, 0.0) + (q.C2 * r) * ek;
    D[i] = ras_diff(r, nut[i], mu[i], q.sigmaEps);
  }
}

// Generic scalar transport assembly: ddt(rho, psi) + div(phi, psi) - laplacian(D, psi) == Su - Sp psi (Su, Sp per
// unit volume), Euler ddt with rho_old and the field's own value, convection by the weights wc / bwc (nullptr:
// upwind), the laplacian by the delta coefficients of the scheme in force. The face and slot arithmetic is
// k_e_assemble's he part; the boundary coefficients k_y_assemble's (inletOutlet included):
//   diag = ((rdt rho V + d1) - dL) + V Sp;   source = rdt rho_old psi V + V Su
// CON: fvMatrix::setValues folded in (the epsilon equation of a wall-function context; include/dfmi.h).
// con[c] != 0 marks a constrained cell, whose value v_c is psi[c] (k_ras_wall wrote it there). Each cell forms both
// L1 - UL and U1 - UL of every face it walks, so it knows A[c][n] without reading lower / upper: the owner writes zeros
// where either side is constrained; a constrained cell gets source = v_c diag and zero slot coefficients; an
// unconstrained one walks its faces once more after its source is complete and takes A[c][n] v_n of every constrained
// neighbour out of it, in the same face order. CON = false is the kernel as it was, op for op.
template <int WT, bool CON = false>
__global__ void __launch_bounds__(TPB) k_scalar_assemble(MeshView m, const int8_t* __restrict__ ty,
    const double* __restrict__ psi, const double* __restrict__ bpsi, const double* __restrict__ rho,
    const double* __restrict__ rho_old, const double* __restrict__ phi, const double* __restrict__ bphi,
    const double* __restrict__ D, const double* __restrict__ bD, const double* __restrict__ Su,
    const double* __restrict__ Sp, double* __restrict__ lower, double* __restrict__ upper, double* __restrict__ diag,
    double* __restrict__ src, double* __restrict__ ic, double* __restrict__ bc, MixBC mx,
    const double* __restrict__ wc, const double* __restrict__ bwc, const int8_t* __restrict__ con = nullptr) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long B = m.B;
  double d1 = 0.0, dL = 0.0;
  const double Dc = D[c];
  bool cc = false, cany = false;
  if constexpr (CON) cc = con[c] != 0;
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double ph = phi[f], w = m.w[f];
    const double wu = wc ? wc[f] : (ph >= 0 ? 1.0 : 0.0);
    const double L1 = -wu * ph, U1 = L1 + ph;
    const double UL = m.dc[f] * ((own ? interp_f(w, Dc, D[o2]) : interp_f(w, D[o2], Dc)) * m.magSf[f]);
    if constexpr (CON) {
      const bool cn = con[o2] != 0;
      cany = cany || cn;
      if (own) { d1 -= L1; lower[f] = (cc || cn) ? 0.0 : L1 - UL; upper[f] = (cc || cn) ? 0.0 : U1 - UL; } else d1 -= U1;
    } else {
      if (own) { d1 -= L1; lower[f] = L1 - UL; upper[f] = U1 - UL; } else d1 -= U1;
    }
    dL -= UL;
  });
  const double vol = m.V[c];
  const double dg = ((m.rdt * rho[c] * vol + d1) - dL) + vol * Sp[c];
  diag[c] = dg;
  if constexpr (CON) {
    if (cc) src[c] = psi[c] * dg;
    else {
      double s = m.rdt * rho_old[c] * psi[c] * vol + vol * Su[c];
      if (cany)
        each_face<WT>(m, c, [&](int f, int o2, bool own) {
          if (con[o2] == 0) return;
          const double ph = phi[f], w = m.w[f];
          const double wu = wc ? wc[f] : (ph >= 0 ? 1.0 : 0.0);
          const double L1 = -wu * ph, U1 = L1 + ph;
          const double UL = m.dc[f] * ((own ? interp_f(w, Dc, D[o2]) : interp_f(w, D[o2], Dc)) * m.magSf[f]);
          s -= (own ? U1 - UL : L1 - UL) * psi[o2];   // A[c][n]: upper of an owned face, lower of a neighbour face
        });
      src[c] = s;
    }
  } else {
    src[c] = m.rdt * rho_old[c] * psi[c] * vol + vol * Su[c];
  }
  each_slot(m, ty, c, [&](int b, int t) {
    if constexpr (CON) if (cc) { ic[b] = 0.0; bc[b] = 0.0; return; }
    const double wu = bwc ? bwc[b] : upwind_b(m, bphi, b);
    const BCoef qc = bcoef_f(t, bpsi[b], wu, m.bdc[b], mx, b, B, 0);
    const BCoef ql = bcoef_f(t, bpsi[b], m.bw[b], m.bdc[b], mx, b, B, 0);
    const double gam = bc_coupled(t) ? interp_b(m.bw[b], Dc, nbrv(m, D, bD, b)) : bD[b];
    const double pG = gam * m.bmagSf[b];
    ic[b] = bphi[b] * qc.vic - pG * ql.gic;
    bc[b] = -bphi[b] * qc.vbc - (-pG * ql.gbc);
  });
}
// the constrained cells' source once more, source = v_c diag, where something was added to the source after the
// assembly (the corrected laplacian's explicit term): each cell writes its own entry
__global__ void k_ras_constrain_source(long n, const int8_t* __restrict__ con, const double* __restrict__ psi,
                                       const double* __restrict__ diag, double* __restrict__ src) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n || con[i] == 0) return;
  src[i] = psi[i] * diag[i];
}

// bound(psi, lo) (OpenFOAM-7 bound.C) as a gather from the solved field `pre` (its slots bpre corrected after the solve):
//   avg = sum_f |Sf| face(max(pre, lo)) / sum_f |Sf| over the cell's faces (interp_f of the two bounded cell values,
//   owner first) and its slots (a coupled slot is a face: interp_b of the two bounded cell values, so the result does
//   not depend on where a decomposition cuts; every other slot max(stored value, lo));
//   psi = max(max(pre, avg pos0(-pre)), lo). A cell with pre >= lo comes out bitwise pre.
template <int WT>
__global__ void __launch_bounds__(TPB) k_ras_bound(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ pre,
                                                   const double* __restrict__ bpre, double lo, double* __restrict__ psi) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const double pc = pre[c], pcb = fmax(pc, lo);
  double num = 0.0, den = 0.0;
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double w = m.w[f], ms = m.magSf[f], pn = fmax(pre[o2], lo);
    num += ms * (own ? interp_f(w, pcb, pn) : interp_f(w, pn, pcb));
    den += ms;
  });
  each_slot(m, ty, c, [&](int b, int t) {
    const double ms = m.bmagSf[b];
    num += ms * (bc_coupled(t) ? interp_b(m.bw[b], pcb, fmax(nbrv(m, pre, bpre, b), lo)) : fmax(bpre[b], lo));
    den += ms;
  });
  psi[c] = fmax(fmax(pc, (num / den) * pos0(-pc)), lo);
}
__global__ void k_ras_bound_slots(long n, double lo, double* __restrict__ bpsi) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  bpsi[i] = fmax(bpsi[i], lo);
}
// nut = (Cmu (k k)) / eps over n cells, or over the n boundary slots whose nut patch type is `calculated` (the field
// expression's own boundary values; the other types are nut.correctBoundaryConditions(), k_bc_correct)
__global__ void k_ras_nut(long n, const int8_t* __restrict__ ty, double Cmu, const double* __restrict__ k,
                          const double* __restrict__ eps, double* __restrict__ nut) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (ty && ty[i] != CALCULATED) return;
  const double kc = k[i];
  nut[i] = (Cmu * (kc * kc)) / eps[i];
}

// ---- wall functions and turbulent inlets (include/dfmi.h, RAS block)
// What a slot is comes from sflag (Ctx::WF_* bits), its patch's constants from the row tab[WF_TAB * spatch[b]]:
//   {Cmu25, Cmu75, kappa, E, yPlusLam, intensity, mixingLength}. bdc is the patch's own deltaCoeffs (never the
// non-orthogonal ones: the two agree on non-coupled slots).
struct WallTab { const int8_t* sflag; const int* spatch; const double* tab; };
//   y = 1 / deltaCoeffs;  nuw = boundary_mu / boundary_rho;  yPlus = ((Cmu25 y) sqrt(k_c)) / nuw
__device__ __forceinline__ double wall_yplus(double Cmu25, double y, double sqrtk, double nuw) { return ((Cmu25 * y) * sqrtk) / nuw; }

// epsilonWallFunction, per cell: the cell's slots of that type in ascending slot order, weight w = 1 / n;
//   yPlus > yPlusLam:  eps += ((w Cmu75) (k sqrt k)) / (kappa y);  G += ((((w (nutw + nuw)) magGradUw) Cmu25) sqrt k) / (kappa y)
//   otherwise:         eps += (((w 2) k) nuw) / (y y)
// with magGradUw = deltaCoeffs |boundary_U - U_c|. epsilon and G of the cell are replaced, boundary_epsilon of those
// slots takes the cell's value, con[c] says whether the cell is constrained. A cell touches only its own entries.
// The slot range is each_slot's (cbStart / cbSlot) walked by hand, three times (count, accumulate, write back): the
// flagged slots are never empty (the codes are refused on empty patches), so each_slot's EMPTY test has nothing to
// skip. The thread's cell is the plain index, not cell_of / xcd_block: no face is gathered, so there is no locality
// for a traversal to improve, and the result does not depend on the order.
__global__ void __launch_bounds__(TPB) k_ras_wall(MeshView m, WallTab t, const double* __restrict__ bdc,
    const double* __restrict__ k, const double* __restrict__ U, const double* __restrict__ bU,
    const double* __restrict__ bmu, const double* __restrict__ brho, const double* __restrict__ bnut,
    double* __restrict__ eps, double* __restrict__ G, double* __restrict__ beps, int8_t* __restrict__ con) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.C) return;
  const int k0 = m.cbStart[c], k1 = m.cbStart[c + 1];
  int n = 0;
  for (int i = k0; i < k1; ++i) n += (t.sflag[m.cbSlot[i]] & Ctx::WF_EPS_WALL) ? 1 : 0;
  con[c] = n ? 1 : 0;
  if (!n) return;
  const double w = 1.0 / (double)n;
  const double kc = k[c], sk = sqrt(kc);
  const long C = m.C, B = m.B;
  const double u0 = U[c], u1 = U[C + c], u2 = U[2 * C + c];
  double e = 0.0, g = 0.0;
  for (int i = k0; i < k1; ++i) {
    const int b = m.cbSlot[i];
    if (!(t.sflag[b] & Ctx::WF_EPS_WALL)) continue;
    const double* q = t.tab + Ctx::WF_TAB * t.spatch[b];
    const double Cmu25 = q[0], Cmu75 = q[1], kappa = q[2], ypl = q[4];
    const double dcb = bdc[b], y = 1.0 / dcb, nuw = bmu[b] / brho[b];
    const double yp = wall_yplus(Cmu25, y, sk, nuw);
    if (yp > ypl) {
      const double dx = bU[b] - u0, dy = bU[B + b] - u1, dz = bU[2 * B + b] - u2;
      const double mg = dcb * sqrt((dx * dx + dy * dy) + dz * dz);
      e += ((w * Cmu75) * (kc * sk)) / (kappa * y);
      g += ((((w * (bnut[b] + nuw)) * mg) * Cmu25) * sk) / (kappa * y);
    } else {
      e += (((w * 2.0) * kc) * nuw) / (y * y);
    }
  }
  eps[c] = e;
  G[c] = g;
  for (int i = k0; i < k1; ++i) {
    const int b = m.cbSlot[i];
    if (t.sflag[b] & Ctx::WF_EPS_WALL) beps[b] = e;
  }
}
// nutkWallFunction, per slot: boundary_nut = yPlus > yPlusLam ? nuw ((yPlus kappa) / log(E yPlus) - 1) : 0, and
// boundary_yPlus (zero on every other slot)
__global__ void k_ras_nut_wall(long n, WallTab t, const int* __restrict__ bfc, const double* __restrict__ bdc,
                               const double* __restrict__ k, const double* __restrict__ bmu, const double* __restrict__ brho,
                               double* __restrict__ bnut, double* __restrict__ byp) {
  const long b = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (b >= n) return;
  if (!(t.sflag[b] & Ctx::WF_NUT_WALL)) { byp[b] = 0.0; return; }
  const double* q = t.tab + Ctx::WF_TAB * t.spatch[b];
  const double Cmu25 = q[0], kappa = q[2], E = q[3], ypl = q[4];
  const double y = 1.0 / bdc[b], nuw = bmu[b] / brho[b];
  const double yp = wall_yplus(Cmu25, y, sqrt(k[bfc[b]]), nuw);
  byp[b] = yp;
  bnut[b] = yp > ypl ? nuw * ((yp * kappa) / log(E * yp) - 1.0) : 0.0;
}
// the turbulent inlets' inletValue, per slot. which = WF_K_INLET: k_ref = (1.5 (I I)) ((Ux Ux + Uy Uy) + Uz Uz) of
// boundary_U; which = WF_EPS_INLET: eps_ref = (Cmu75 / L) (kb sqrt(kb)) of boundary_k, Cmu75 of ras.Cmu
__global__ void k_ras_inlet_ref(long n, int which, WallTab t, double Cmu75, const double* __restrict__ bU,
                                const double* __restrict__ bk, double* __restrict__ ref) {
  const long b = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (b >= n || !(t.sflag[b] & which)) return;
  const double* q = t.tab + Ctx::WF_TAB * t.spatch[b];
  if (which == Ctx::WF_K_INLET) {
    const double I = q[5], ux = bU[b], uy = bU[n + b], uz = bU[2 * n + b];
    ref[b] = (1.5 * (I * I)) * ((ux * ux + uy * uy) + uz * uz);
  } else {
    const double L = q[6], kb = bk[b];
    ref[b] = (Cmu75 / L) * (kb * sqrt(kb));
  }
}

// ------------------------------------------------------------------ non-orthogonal laplacians
// surfaceInterpolation::makeNonOrthDeltaCoeffs / makeNonOrthCorrectionVectors per face of the face storage, from the
// arrays the context holds (Sf, |Sf|, d = mesh_distance), in Mesh.nonorth_geometry's operation order:
//   n = Sf / |Sf|;  nd = (n_x d_x + n_y d_y) + n_z d_z;  |d| = sqrt((d_x d_x + d_y d_y) + d_z d_z)
//   nonOrthDeltaCoeffs = 1 / max(nd, 0.05 |d|);  k = n - d nonOrthDeltaCoeffs
__device__ __forceinline__ void nonorth_face(const double (&s)[3], double ms, const double (&d)[3], double& dc, double (&k)[3]) {
  const double n0 = s[0] / ms, n1 = s[1] / ms, n2 = s[2] / ms;
  const double nd = (n0 * d[0] + n1 * d[1]) + n2 * d[2];
  const double dm = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  dc = 1.0 / fmax(nd, 0.05 * dm);
  k[0] = n0 - d[0] * dc; k[1] = n1 - d[1] * dc; k[2] = n2 - d[2] * dc;
}
__global__ void k_nonorth_geom_face(MeshView m, double* __restrict__ ndc, double* __restrict__ nk) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.F) return;
  const long F = m.F;
  double dc = 0.0, k[3] = {0.0, 0.0, 0.0};
  if (m.own[f] >= 0) {   // padding slots of the owner-slot storage stay zero
    const double s[3] = {m.Sf[f], m.Sf[F + f], m.Sf[2 * F + f]}, d[3] = {m.md[f], m.md[F + f], m.md[2 * F + f]};
    nonorth_face(s, m.magSf[f], d, dc, k);
  }
  ndc[f] = dc;
  nk[f] = k[0]; nk[F + f] = k[1]; nk[2 * F + f] = k[2];
}
// boundary slots: coupled slots (cyclic, processor, processorCyclic; both halves of a processor patch) by the same
// formulas from the patch delta; every other slot keeps its deltaCoeffs and has k = 0 (fvPatchField::gradientCoeffs
// reads patch().deltaCoeffs())
__global__ void k_nonorth_geom_slot(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ bdc0,
                                    double* __restrict__ nbdc, double* __restrict__ nbk) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B) return;
  const long B = m.B;
  double dc = bdc0[b], k[3] = {0.0, 0.0, 0.0};
  if (bc_coupled(ty[b])) {
    const double s[3] = {m.bSf[b], m.bSf[B + b], m.bSf[2 * B + b]}, d[3] = {m.bdv[b], m.bdv[B + b], m.bdv[2 * B + b]};
    nonorth_face(s, m.bmagSf[b], d, dc, k);
  }
  nbdc[b] = dc;
  nbk[b] = k[0]; nbk[B + b] = k[1]; nbk[2 * B + b] = k[2];
}

// The explicit part of a corrected laplacian (correctedSnGrad::correction, gaussLaplacianScheme::fvmLaplacian):
//   fvm.source() -= V div(gamma_f |Sf| (k . (grad phi)_f)),  every laplacian entering its equation with a minus,
// as one per-cell gather over NC fields that share the walk (U's three components, a chunk of species, he, p). The
// cell's own gradients and diffusivities sit in registers; each face gathers the other cell's. Per face, in the
// sequential face order (each_face), then per coupled slot of the cell in slot order:
//   g_d    = interp_f(w, g_P,d, g_N,d)                        d = x, y, z (owner first; slots: interp_b(bw, own, other))
//   corr_f = (k_x g_x + k_y g_y) + k_z g_z
//   flux_f = (gamma_f |Sf|) corr_f                            gamma_f = interp_f(w, gamma_P, gamma_N), or the face field
//   acc   += flux_f (owner) / acc -= flux_f (neighbour) / acc += flux_b (slot)
// then source[c] = source[c] + acc: one accumulator per field, no atomics. k = 0 on non-coupled slots: they add nothing.
// A coupled slot's other cell is the cyclic partner cell, or (processor slots) the exchanged copies bg / bgam.
// Gradient component d of field k of cell c: g[(k gk + d gd) C + c] (k_grad_cells: gk = 3, gd = 1; k_u_grad's gout:
// gk = 1, gd = 3), slots likewise with B.
enum { NO_SHARED = 0, NO_SPECIES = 1, NO_FACE = 2 };
struct NoArgs {
  const double *nk, *bnk;       // correction vectors [3][Fs], [3][B]
  const double *g, *bg;         // cell gradients and their processor-slot copies
  int gk, gd;
  // NO_SHARED: one cell diffusivity for the NC fields (mu / muEff, alpha / alphaEff). NO_SPECIES: field k's own,
  // gam + (s0 + k) C (rhoD), plus `add` where set (LES: mut / Sct). NO_FACE: a face field (rhorAUf) and its slots
  const double *gam, *bgam, *add, *badd;
  double *src, *src2;           // sources [NC][C] the term is added to (src2: U's source_solve; nullptr: none)
  // NO_SPECIES: first species of the chunk, species count, inert species (no equation); the solver rows' rhs
  // [S - 1][Ce] at the row's position (nullptr: none); diffAlphaD's own laplacian(alpha hai_i, Y_i) on the same walk:
  // dAD[c] = dAD[c] + acc2_k / V for the chunk's species in order (nullptr: LES, the term is dropped)
  int s0, S, inert;
  long Ce;
  double* rhs;
  const double *alpha, *balpha, *hai, *bhai;
  double* dAD;
  // NO_FACE: source = base + acc (the pEqn loop re-forms it every pass); the face flux correction of the owned faces and
  // of the coupled slots (pEqn.flux()'s faceFluxCorrectionPtr)
  const double* base;
  double *fcorr, *bfcorr;
};
template <int NC, int WT, int MODE>
__global__ void __launch_bounds__(TPB) k_nonorth_corr(MeshView m, const int8_t* __restrict__ ty, NoArgs a) {
  const int c = cell_of(m, xcd_block() * blockDim.x + threadIdx.x);
  if (c >= m.C) return;
  const long C = m.C, F = m.F, B = m.B;
  const bool dad = MODE == NO_SPECIES && a.dAD != nullptr;
  double gc[NC][3], gamc[NC], ahc[NC], acc[NC], acc2[NC];
  const double addc = (MODE == NO_SPECIES && a.add) ? a.add[c] : 0.0;
  const double alc = dad ? a.alpha[c] : 0.0;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    acc[k] = 0.0; acc2[k] = 0.0; ahc[k] = 0.0; gamc[k] = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) gc[k][d] = a.g[(long)(k * a.gk + d * a.gd) * C + c];
    if constexpr (MODE == NO_SHARED) gamc[k] = a.gam[c];
    if constexpr (MODE == NO_SPECIES) {
      gamc[k] = a.gam[(long)(a.s0 + k) * C + c];
      if (a.add) gamc[k] = gamc[k] + addc;
      if (dad) ahc[k] = alc * a.hai[(long)(a.s0 + k) * C + c];
    }
  }
  each_face<WT>(m, c, [&](int f, int o2, bool own) {
    const double w = m.w[f], ms = m.magSf[f];
    const double k0 = a.nk[f], k1 = a.nk[F + f], k2 = a.nk[2 * F + f];
    auto fi = [&](double vc, double vn) { return own ? interp_f(w, vc, vn) : interp_f(w, vn, vc); };
    double gsh = 0.0, addn = 0.0, aln = 0.0;
    if constexpr (MODE == NO_SHARED) gsh = fi(gamc[0], a.gam[o2]);
    if constexpr (MODE == NO_FACE) gsh = a.gam[f];
    if constexpr (MODE == NO_SPECIES) { if (a.add) addn = a.add[o2]; if (dad) aln = a.alpha[o2]; }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const double g0 = fi(gc[k][0], a.g[(long)(k * a.gk) * C + o2]);
      const double g1 = fi(gc[k][1], a.g[(long)(k * a.gk + a.gd) * C + o2]);
      const double g2 = fi(gc[k][2], a.g[(long)(k * a.gk + 2 * a.gd) * C + o2]);
      const double corr = (k0 * g0 + k1 * g1) + k2 * g2;
      double gf = gsh;
      if constexpr (MODE == NO_SPECIES) {
        double gn = a.gam[(long)(a.s0 + k) * C + o2];
        if (a.add) gn = gn + addn;
        gf = fi(gamc[k], gn);
      }
      const double fl = (gf * ms) * corr;
      if (own) acc[k] += fl; else acc[k] -= fl;
      if constexpr (MODE == NO_FACE) { if (own) a.fcorr[f] = fl; }
      if constexpr (MODE == NO_SPECIES) {
        if (dad) {
          const double fl2 = (fi(ahc[k], aln * a.hai[(long)(a.s0 + k) * C + o2]) * ms) * corr;
          if (own) acc2[k] += fl2; else acc2[k] -= fl2;
        }
      }
    }
  });
  each_slot(m, ty, c, [&](int b, int t) {
    if (!bc_coupled(t)) return;
    const int pc = m.partner[b];
    const double bw = m.bw[b], ms = m.bmagSf[b];
    const double k0 = a.bnk[b], k1 = a.bnk[B + b], k2 = a.bnk[2 * B + b];
    double gsh = 0.0;
    if constexpr (MODE == NO_SHARED) gsh = interp_b(bw, gamc[0], pc >= 0 ? a.gam[pc] : a.bgam[b]);
    if constexpr (MODE == NO_FACE) gsh = a.bgam[b];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      double gg[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const long q = k * a.gk + d * a.gd;
        gg[d] = interp_b(bw, gc[k][d], pc >= 0 ? a.g[q * C + pc] : a.bg[q * B + b]);
      }
      const double corr = (k0 * gg[0] + k1 * gg[1]) + k2 * gg[2];
      double gf = gsh;
      if constexpr (MODE == NO_SPECIES) {
        const long s = a.s0 + k;
        double gn = pc >= 0 ? a.gam[s * C + pc] : a.bgam[s * B + b];
        if (a.add) gn = gn + (pc >= 0 ? a.add[pc] : a.badd[b]);
        gf = interp_b(bw, gamc[k], gn);
      }
      const double fl = (gf * ms) * corr;
      acc[k] += fl;
      if constexpr (MODE == NO_FACE) a.bfcorr[b] = fl;
      if constexpr (MODE == NO_SPECIES) {
        if (dad) {
          const long s = a.s0 + k;
          const double an = pc >= 0 ? a.alpha[pc] * a.hai[s * C + pc] : a.balpha[b] * a.bhai[s * B + b];
          acc2[k] += (interp_b(bw, ahc[k], an) * ms) * corr;
        }
      }
    }
  });
  if constexpr (MODE == NO_FACE) {
    a.src[c] = a.base[c] + acc[0];
  } else if constexpr (MODE == NO_SHARED) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      a.src[k * C + c] = a.src[k * C + c] + acc[k];
      if (a.src2) a.src2[k * C + c] = a.src2[k * C + c] + acc[k];
    }
  } else {
    const int pr = m.eopos ? m.eopos[c] : c;   // the solver row of c (even-odd layout)
    const double vol = m.V[c];
    double dd = dad ? a.dAD[c] : 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int s = a.s0 + k;
      if (dad) dd = dd + acc2[k] / vol;
      if (s == a.inert) continue;
      if (a.src) a.src[(long)s * C + c] = a.src[(long)s * C + c] + acc[k];
      if (a.rhs) {
        const long ss = s < a.inert ? s : s - 1;
        a.rhs[ss * a.Ce + pr] = a.rhs[ss * a.Ce + pr] + acc[k];
      }
    }
    if (dad) a.dAD[c] = dd;
  }
}
// phi -= the face flux correction (internal faces of the face storage; coupled primary slots)
__global__ void k_nonorth_flux_face(MeshView m, const double* __restrict__ fcorr, double* __restrict__ phi) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.F || m.own[f] < 0) return;
  phi[f] = phi[f] - fcorr[f];
}
__global__ void k_nonorth_flux_slot(MeshView m, const int8_t* __restrict__ ty, const double* __restrict__ bfcorr,
                                    double* __restrict__ bphi) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.B || !m.sprim[b] || !bc_coupled(ty[b])) return;
  bphi[b] = bphi[b] - bfcorr[b];
}

// ------------------------------------------------------------------ df0DFoam species update
// YEqn.H of df0DFoam (applications/solvers/df0DFoam/YEqn.H): fvm::ddt(rho, Yi) == RR_i per cell (no
// transport), solved exactly: Y_i = (rdt rho_old Y_i V + V RR_i) / (rdt rho V); Yi.max(0); inert = 1 - sum.
__global__ void k_zero_d_species(int C, int S, int inert, double rdt, const double* __restrict__ V,
                                 const double* __restrict__ rho_old, const double* __restrict__ rho,
                                 const double* __restrict__ RR, double* __restrict__ Y) {
  const int c = xcd_block() * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double vol = V[c];
  const double dg = rdt * rho[c] * vol, ro = rdt * rho_old[c];
  double sum = 0.0;
  for (int s = 0; s < S; ++s) {
    if (s == inert) continue;
    double y = (ro * Y[(long)s * C + c] * vol + vol * RR[(long)s * C + c]) / dg;
    y = y > 0 ? y : 0;
    Y[(long)s * C + c] = y;
    sum += y;
  }
  sum = 1 - sum;
  Y[(long)inert * C + c] = sum > 0 ? sum : 0;
}

// ------------------------------------------------------------------ elementwise thermo bookkeeping
__global__ void k_mul(long n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] * b[i];
}
__global__ void k_add_psip(long n, const double* __restrict__ p, const double* __restrict__ psi,
                           const double* __restrict__ psip0, double* __restrict__ rho) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i < n) rho[i] += psi[i] * p[i] - psip0[i];
}

template <template <int> class K, class... A> void dispatch_S(int S, dim3 g, dim3 b, hipStream_t st, A... a);

}  // namespace

// ====================================================================== launchers
#define LAUNCH(kernel, n, ...) \
  do { KScope _ks(x, #kernel); if ((n) > 0) hipLaunchKernelGGL(kernel, dim3(blocks_for((n), TPB)), dim3(TPB), 0, x.stream, __VA_ARGS__); \
       DFMI_HIP(hipGetLastError()); } while (0)
// a launch timed under another kernel's name (a variant of that kernel: the bench rooflines key on the name)
#define LAUNCH_AS(name, kernel, n, ...) \
  do { KScope _ks(x, name); if ((n) > 0) hipLaunchKernelGGL(kernel, dim3(blocks_for((n), TPB)), dim3(TPB), 0, x.stream, __VA_ARGS__); \
       DFMI_HIP(hipGetLastError()); } while (0)

template <bool L> LesDiff<L> les_diff(Ctx& x) {
  if constexpr (L) return {x.mut_sct(false), x.mut_sct(true)};
  else return {};
}
// kernels templated on the ELL width: the unrolled path for hex meshes (W = 6), the CSR walk otherwise
// (option fv.csr_walk forces the CSR walk everywhere: A/B measurement and parity of both paths)
bool face_rows(const Ctx& x) { return x.ell.W == 6 && !x.on("fv.csr_walk"); }
// hex boxes in blockMesh order: the computed face walk (each_face<-1>) everywhere (fv.hex_walk = 0: off)
bool face_hex(const Ctx& x) { return x.hex[0] > 0 && x.on("fv.hex_walk") && !x.on("fv.csr_walk"); }
#define LAUNCH_W(kern, n, ...) \
  do { if (face_hex(x)) LAUNCH(kern<-1>, n, __VA_ARGS__); else if (face_rows(x)) LAUNCH(kern<6>, n, __VA_ARGS__); \
       else LAUNCH(kern<0>, n, __VA_ARGS__); } while (0)
// species-chunked kernels for large mechanisms walk the CSR face lists on every mesh: 2M cells x 53 species,
// y_prep 9.5 against 17.5 ms by the face rows and 8.61 against 8.71 ms by the computed hex walk (its 179 VGPRs:
// two waves per SIMD), y_assemble_ell 4.5 / 4.43 against 6.1 / 5.84 ms (round 4, scripts/c4_ab.sh)
#define LAUNCH_SWG(kern, NS, n, ...) LAUNCH((kern<NS, 0>), n, __VA_ARGS__)
// the YEqn assembly kernels, whose LES form (Ctx::les.model != 0) is an instantiation of its own
// (the kernels' last argument, LesDiff<L>, is appended here)
#define LAUNCH_SWGL(kern, NS, n, ...) \
  do { if (x.turbulent()) LAUNCH((kern<NS, 0, true>), n, __VA_ARGS__, les_diff<true>(x)); \
       else LAUNCH((kern<NS, 0, false>), n, __VA_ARGS__, les_diff<false>(x)); } while (0)
#define LAUNCH_SW_(kern, NS, L, n, ...) \
  do { if (face_hex(x)) LAUNCH((kern<NS, -1, L>), n, __VA_ARGS__, les_diff<L>(x)); \
       else if (face_rows(x)) LAUNCH((kern<NS, 6, L>), n, __VA_ARGS__, les_diff<L>(x)); \
       else LAUNCH((kern<NS, 0, L>), n, __VA_ARGS__, les_diff<L>(x)); } while (0)
#define LAUNCH_SWL(kern, NS, n, ...) \
  do { if (x.turbulent()) LAUNCH_SW_(kern, NS, true, n, __VA_ARGS__); else LAUNCH_SW_(kern, NS, false, n, __VA_ARGS__); } while (0)
#define LAUNCH_SW(kern, NS, n, ...) \
  do { if (face_hex(x)) LAUNCH((kern<NS, -1>), n, __VA_ARGS__); else if (face_rows(x)) LAUNCH((kern<NS, 6>), n, __VA_ARGS__); \
       else LAUNCH((kern<NS, 0>), n, __VA_ARGS__); } while (0)

// the mixed-condition data of a field (MixBC): p's waveTransmissive state, every field's inletValue
MixBC mixbc(Ctx& x, const std::string& field) {
  MixBC m{nullptr, nullptr, x.f("boundary_phi"), nullptr};
  if (field == "p") { m.wvf = x.f("boundary_p_vf"); m.wref = x.f("boundary_p_old"); }
  auto it = x.fields.find("boundary_" + field + "_ref");
  if (it != x.fields.end()) m.ioref = it->second.buf.p;
  return m;
}

void k_bc_correct(Ctx& x, const char* tf, double* vf, double* bvf, int ncomp) {
  const double* eg = std::string(tf) == "he" ? x.f("boundary_heGradient") : nullptr;
  LAUNCH(k_bc_correct, x.B, x.view(), x.st(tf), vf, bvf, ncomp, eg, mixbc(x, tf));
}

void copy_old(Ctx& x) {   // dfMatrixDataBase::preTimeStep (dfMatrixDataBase.cu:503-517)
  const char* pairs[][2] = {{"rho_old", "rho"}, {"boundary_rho_old", "boundary_rho"}, {"phi_old", "phi"},
                            {"boundary_phi_old", "boundary_phi"}, {"U_old", "U"}, {"boundary_U_old", "boundary_U"},
                            {"K_old", "K"}, {"p_old", "p"}, {"boundary_p_old", "boundary_p"}};
  CopyList L{};
  int k = 0;
  for (auto& pr : pairs) {
    Field& dst = x.fields.at(pr[0]);
    if (dst.buf.n == 0) continue;
    L.src[k] = x.f(pr[1]); L.dst[k] = dst.buf.p; L.n[k] = (long)dst.buf.n; ++k;
  }
  static_assert(sizeof(pairs) / sizeof(pairs[0]) <= MAXCOPY, "CopyList capacity");
  KScope _ks(x, "k_copy_multi");
  if (k) hipLaunchKernelGGL(k_copy_multi, dim3(1024, k), dim3(TPB), 0, x.stream, L);
  DFMI_HIP(hipGetLastError());
}

void rho_process(Ctx& x, bool write_matrix) {
  double* od = write_matrix ? x.f("dbg_rho_diag") : nullptr;
  double* os = write_matrix ? x.f("dbg_rho_source") : nullptr;
  if (spray_on(x))
    LAUNCH_W(k_rho_spray, x.C, x.view(), x.st("rho"), x.f("rho_old"), x.f("phi"), x.f("boundary_phi"), x.f("rho"), od, os,
             x.f("parcel_rhoTrans"), x.S, x.spray.sch[0]);
  else
  LAUNCH_W(k_rho, x.C, x.view(), x.st("rho"), x.f("rho_old"), x.f("phi"), x.f("boundary_phi"), x.f("rho"), od, os);
  k_bc_correct(x, "rho", x.f("rho"), x.f("boundary_rho"), 1);
  halo_fields(x, {"rho"});
}

// ---- spray coupling (include/dfmi.h, spray block)
// spray.model = 0: false, nothing else. Otherwise the refusals by name, then true.
bool spray_on(Ctx& x) {
  if (!x.spray.model) return false;
  const char* why = "spray.model = 1 ";
  DFMI_CHECK(!x.fgm.model, std::string(why) + "is not available with fgm.model = 1 (the flareFGM spray branch is not on the device)");
  DFMI_CHECK(!x.thermo.eos, std::string(why) + "is not available with an equation of state set (dfmi_thermo_set_eos model 1)");
  DFMI_CHECK(x.thermo.dhc.n == (size_t)x.S, std::string(why) + "needs the thermo coefficients (dfmi_thermo_set_coeffs: hc_i)");
  for (int i = 0; i < 5; ++i) {
    const bool need = i == 2 ? x.spray.sch[1] == 1 : i == 4 ? x.spray.sch[3] == 1 : true;
    DFMI_CHECK(!need || (x.spray.have[i] && x.fields.count(spray_field_name(i))),
               std::string(why) + "needs the field '" + spray_field_name(i) + "', which was never set (dfmi_set_field)");
  }
  return true;
}
static void spray_fold_u(Ctx& x) {
  if (!spray_on(x)) return;
  Matrix& A = x.mU;
  const int semi = x.spray.sch[1];
  LAUNCH(k_spray_u, x.C, x.view(), x.st("U"), semi, x.f("parcel_UTrans"), semi ? x.f("parcel_UCoeff") : nullptr, x.f("U"),
         A.diag.p, A.source.p, A.source_solve.p, A.ic.p, x.f("rAU"));
}
void spray_fold_y(Ctx& x, double* diag, double* source, long stride, bool ell) {
  if (!spray_on(x)) return;
  KScope _ks(x, "k_spray_y");
  hipLaunchKernelGGL(k_spray_y, dim3(blocks_for(x.C, TPB), x.S), dim3(TPB), 0, x.stream, x.view(), x.inert, x.spray.sch[2],
                     ell ? 1 : 0, stride, x.f("parcel_rhoTrans"), x.f("Y"), diag, source);
  DFMI_HIP(hipGetLastError());
}
static void spray_fold_e(Ctx& x) {
  if (!spray_on(x)) return;
  Matrix& A = x.mE;
  const int semi = x.spray.sch[3];
  LAUNCH(k_spray_e, x.C, x.view(), x.S, semi, x.f("parcel_rhoTrans"), x.thermo.dhc.p, x.f("parcel_hsTrans"),
         semi ? x.f("parcel_hsCoeffByCp") : nullptr, x.f("he"), A.diag.p, A.source.p);
}

// compressibleCourantNo.H: the per-cell gather, the fixed-order second stage and the record, queued on the context
// stream with no synchronisation (dfmi_courant_no waits on the record; dfmi_time_step with step.courant ends with this).
// Several ranks: the per-rank triples are all-gathered and combined in rank order, every rank to the same bits.
void courant_post(Ctx& x) {
  Courant& co = x.co;
  co.ensure();
  const int nblk = blocks_for(x.C, TPB);
  if (co.partial.n < (size_t)2 * nblk) co.partial.alloc((size_t)2 * nblk);
  if (co.tri.n == 0) co.tri.alloc(3);
  LAUNCH_W(k_courant, x.C, x.view(), x.st("calculated"), x.f("phi"), x.f("boundary_phi"), x.f("rho"), co.partial.p);
  const long long seq = ++co.seq;
  const bool multi = x.nranks > 1;
  hipLaunchKernelGGL(k_courant_reduce, dim3(1), dim3(TPB), 0, x.stream, co.partial.p, nblk, co.sumV, co.tri.p,
                     multi ? nullptr : co.d, x.dt, seq);
  DFMI_HIP(hipGetLastError());
  if (multi) {
    CommTag _ct(x, "courant");
    if (co.all.n < (size_t)3 * x.nranks) co.all.alloc((size_t)3 * x.nranks);
    halo_allgather(x, co.tri.p, co.all.p, 3);
    hipLaunchKernelGGL(k_courant_combine, dim3(1), dim3(64), 0, x.stream, co.all.p, x.nranks, x.dt, co.d, seq);
    DFMI_HIP(hipGetLastError());
  }
  co.fresh = true;
}

// ---- schemes (dfmi_set_scheme): buffers allocated on first use
static double* scheme_buf(Ctx& x, const char* name, long n, int ncomp, bool face = false) {
  auto it = x.fields.find(name);
  if (it == x.fields.end() || it->second.n != n || it->second.ncomp != ncomp) {
    Field& f = x.fields[name];
    f.n = n; f.ncomp = ncomp; f.boundary = std::string(name).rfind("boundary_", 0) == 0; f.face = face;
    f.buf.alloc((size_t)n * ncomp);
    f.buf.zero(x.stream);
    return f.buf.p;
  }
  return it->second.buf.p;
}
static void scheme_checks(Ctx& x, bool limited) {
  bool coupled = false;
  for (int p = 0; p < x.P; ++p) coupled |= x.pkind[p] != 0;
  DFMI_CHECK(!limited || !coupled || x.have_bdelta, "limited schemes on a mesh with coupled patches need dfmi_init_boundary_delta");
  DFMI_CHECK(!limited || x.have_md, "limited schemes need mesh_distance (dfmi_init_constant_fields_internal)");
}

// the explicit part of the corrected laplacians (LAP_CORRECTED), added to the sources the assembly kernels wrote
static void nonorth_u(Ctx& x);
static void nonorth_e(Ctx& x);
static void nonorth_y(Ctx& x, double* src, double* rhs, long Ce);

void u_assemble(Ctx& x) {
  Matrix& A = x.mU;
  const bool llv = x.sch.U == SCH_LLV;
  double* gout = llv || x.lap == LAP_CORRECTED ? scheme_buf(x, "gradU", x.C, 9) : x.fields.count("dbg_gradU") ? x.f("dbg_gradU") : nullptr;
  LAUNCH_W(k_u_grad, x.C, x.view(), x.st("U"), x.f("U"), x.f("boundary_U"), x.visc(false), x.visc(true),
         x.f("tauU"), x.f("boundary_tauU"), gout);
  halo_fields(x, {"tauU"});   // fvc_grad_vector_correctBC_processor (dfMatrixOpBase.cu:1366-1389)
  if (!llv && x.lap == LAP_CORRECTED && x.fields.count("dbg_gradU"))
    DFMI_HIP(hipMemcpyAsync(x.f("dbg_gradU"), gout, 9 * sizeof(double) * x.C, hipMemcpyDeviceToDevice, x.stream));
  if (llv) {   // div(phi,U) limitedLinearV weights from this grad(U)
    scheme_checks(x, true);
    for (int p = 0; p < x.P; ++p)   // dfmi_set_scheme refuses it too; checked again here, where it is launched
      DFMI_CHECK(x.pkind[p] != 2, "div(phi,U) limitedLinearV on a decomposed mesh (processor patches) is not supported");
    if (x.fields.count("dbg_gradU"))
      DFMI_HIP(hipMemcpyAsync(x.f("dbg_gradU"), gout, 9 * sizeof(double) * x.C, hipMemcpyDeviceToDevice, x.stream));
    double* w = scheme_buf(x, "U_w", x.Fs, 1, true);
    double* bw = scheme_buf(x, "boundary_U_w", x.B, 1);
    const double twoByk = 2.0 / std::max(x.sch.k_U, 1e-15);
    LAUNCH(k_llv_w_face, x.Fs, x.view(), twoByk, x.f("phi"), x.f("U"), gout, w);
    LAUNCH(k_llv_w_slot, x.B, x.view(), x.st("U"), twoByk, x.f("boundary_phi"), x.f("U"), gout, bw);
  }
  LAUNCH_W(k_u_assemble, x.C, x.view(), x.st("U"), x.st("p"), x.f("rho"), x.f("rho_old"), x.f("U_old"),
           x.f("boundary_U"), x.f("phi"), x.f("boundary_phi"), x.visc(false), x.visc(true), x.f("p"),
           x.f("boundary_p"), x.f("tauU"), x.f("boundary_tauU"), A.lower.p, A.upper.p, A.diag.p, A.source.p,
           A.source_solve.p, A.ic.p, A.bc.p, x.f("rAU"), mixbc(x, "U"), x.sch_w(6), x.sch_w(7));
  if (x.lap == LAP_CORRECTED) nonorth_u(x);
  spray_fold_u(x);   // parcels.SU(U): the last thing added (after the explicit non-orthogonal term); rAU under semiImplicit
  k_bc_correct(x, "extrapolated", x.f("rAU"), x.f("boundary_rAU"), 1);
  halo_fields(x, {"rAU"});
}

void u_post_solve(Ctx& x) {
  k_bc_correct(x, "U", x.f("U"), x.f("boundary_U"), 3);
  halo_fields(x, {"U"});
  LAUNCH(k_kinetic, x.C, x.C, x.f("U"), x.f("K"));
  LAUNCH(k_kinetic_slots, x.B, x.B, x.f("boundary_U"), x.f("boundary_K"));
}

void u_hbya(Ctx& x) {
  Matrix& A = x.mU;
  LAUNCH_W(k_u_hbya, x.C, x.view(), x.st("U"), x.f("U"), x.f("boundary_U"), A.lower.p, A.upper.p, A.source.p,
         A.ic.p, A.bc.p, x.f("HbyA"));
  k_bc_correct(x, "extrapolated", x.f("HbyA"), x.f("boundary_HbyA"), 3);
  LAUNCH(k_hbya_scale_cells, x.C, x.C, x.f("rAU"), x.f("HbyA"));
  LAUNCH(k_hbya_scale_slots, x.B, x.B, x.st("U"), x.f("boundary_rAU"), x.f("boundary_U"), x.f("boundary_HbyA"));
  halo_fields(x, {"HbyA"});
}

// turbulence->correct() (dfLowMachFoam.C:508): nut from U / boundary_U as they stand, boundary_nut by
// nut.correctBoundaryConditions() with nut's patch types (not set: "calculated", OpenFOAM's default for nut -- the
// stored values are kept), the processor slots' neighbour half through the halo
void turbulence_correct(Ctx& x) {
  if (!x.les.model) return;
  DFMI_CHECK(x.les.have_delta, "LES: the filter width field 'delta' is not set (dfmi_set_field)");
  if (x.les.model == 5) {
    // S, then the two contractions, then nut travel through the halo; mu and rho as the context holds them
    LAUNCH_W(k_dyn_strain, x.C, x.view(), x.st("U"), x.f("U"), x.f("boundary_U"), x.f("les_S"), x.f("boundary_les_S"));
    halo_fields(x, {"les_S"});
    LAUNCH_W(k_dyn_filter, x.C, x.view(), x.st("U"), x.f("U"), x.f("boundary_U"), x.f("les_S"), x.f("boundary_les_S"),
             x.f("delta"), x.f("les_LLMM"), x.f("les_MMMM"));
    halo_fields(x, {"les_LLMM", "les_MMMM"});
    LAUNCH_W(k_dyn_nut, x.C, x.view(), x.st("U"), x.f("les_LLMM"), x.f("boundary_les_LLMM"), x.f("les_MMMM"),
             x.f("boundary_les_MMMM"), x.f("les_S"), x.f("delta"), x.f("mu"), x.f("rho"), x.f("les_LM"), x.f("les_MM"),
             x.f("les_Cs"), x.f("nut"));
  } else if (x.les.model == 4) {
    LAUNCH_W(k_les_sigma, x.C, x.view(), x.st("U"), x.f("U"), x.f("boundary_U"), x.f("delta"), x.opt("les.Csg"), x.f("nut"));
  } else {
    const LesCoef q{x.les.model, x.opt("les.Ck"), x.opt("les.Ce"), x.opt("les.Cw")};
    LAUNCH_W(k_les_nut, x.C, x.view(), x.st("U"), x.f("U"), x.f("boundary_U"), x.f("delta"), q, x.f("nut"));
  }
  k_bc_correct(x, x.stype.count("nut") ? "nut" : "calculated", x.f("nut"), x.f("boundary_nut"), 1);
  halo_fields(x, {"nut"});
  x.les.valid = true;
}

void les_effective(Ctx& x) {
  if (!x.turbulent()) return;
  if (x.ras.model) { if (!x.ras.valid) ras_nut(x); }   // turbulence->validate(): correctNut() from k and epsilon as they stand
  else DFMI_CHECK(x.les.valid, "LES: nut is not valid (the model, a coefficient, delta or U changed): call dfmi_turbulence_correct");
  double* cell[3] = {scheme_buf(x, "muEff", x.C, 1), scheme_buf(x, "alphaEff", x.C, 1), scheme_buf(x, "mutSct", x.C, 1)};
  double* slot[3] = {scheme_buf(x, "boundary_muEff", x.B, 1), scheme_buf(x, "boundary_alphaEff", x.B, 1),
                     scheme_buf(x, "boundary_mutSct", x.B, 1)};
  if (!x.les.zeroed) {   // the dropped terms' fields read back as zeros, and the EEqn kernel reads them as such
    for (const char* n : {"sumYDiffError", "hDiffCorrFlux", "diffAlphaD", "phiUc"})
      for (const char* pre : {"", "boundary_"}) x.fields.at(std::string(pre) + n).buf.zero(x.stream);
    x.les.zeroed = true;
  }
  const double Prt = x.opt(x.ras.model ? "ras.Prt" : "les.Prt"), Sct = x.opt(x.ras.model ? "ras.Sct" : "les.Sct");
  LAUNCH(k_les_effective, x.C, (long)x.C, x.f("rho"), x.f("nut"), x.f("mu"), x.f("alpha"), Prt, Sct, cell[0], cell[1], cell[2]);
  LAUNCH(k_les_effective, x.B, (long)x.B, x.f("boundary_rho"), x.f("boundary_nut"), x.f("boundary_mu"),
         x.f("boundary_alpha"), Prt, Sct, slot[0], slot[1], slot[2]);
}

void p_assemble(Ctx& x, bool cell_pass) {
  Matrix& A = x.mP;
  MeshView m = x.view();
  {
    // the cell walk over the owner-slot storage (measured 176 -> 150 us on the 2M box), else (face order)
    // face-parallel; one timer name for both (bench rooflines)
    const bool cellw = x.fslot;
    KScope _ks(x, "k_p_face");
    if (cellw && x.C > 0)
      hipLaunchKernelGGL(k_p_face_cell, dim3(blocks_for(x.C, TPB)), dim3(TPB), 0, x.stream, m, x.f("rho"), x.f("rAU"),
                         x.f("rho_old"), x.f("U_old"), x.f("phi_old"), x.f("HbyA"), x.f("rhorAUf"), x.f("phiHbyA"),
                         A.lower.p, A.upper.p);
    else if (!cellw && x.Fs > 0)
      hipLaunchKernelGGL(k_p_face, dim3(blocks_for(x.Fs, TPB)), dim3(TPB), 0, x.stream, m, x.f("rho"), x.f("rAU"),
                         x.f("rho_old"), x.f("U_old"), x.f("phi_old"), x.f("HbyA"), x.f("rhorAUf"), x.f("phiHbyA"),
                         A.lower.p, A.upper.p);
    DFMI_HIP(hipGetLastError());
  }
  LAUNCH(k_p_slot, x.B, m, x.st("p"), x.st("U"), x.f("rho"), x.f("boundary_rho"), x.f("rAU"), x.f("boundary_rAU"),
         x.f("rho_old"), x.f("boundary_rho_old"), x.f("U_old"), x.f("boundary_U_old"), x.f("boundary_phi_old"),
         x.f("HbyA"), x.f("boundary_HbyA"), x.f("boundary_p"), x.f("boundary_rhorAUf"), x.f("boundary_phiHbyA"),
         A.ic.p, A.bc.p, mixbc(x, "p"), x.f("boundary_phi"), x.f("boundary_psi"), x.f("boundary_p_gamma"),
         x.f("boundary_p_vf"));
  if (!cell_pass) return;   // solve_pcg's k_p_setup_fused forms diag and source (pcg.fuse_setup)
  LAUNCH_W(k_p_cell, x.C, m, x.st("p"), A.lower.p, x.f("phiHbyA"), x.f("boundary_phiHbyA"), x.f("p"), x.f("p_old"),
         x.f("psi"), x.f("rho"), x.f("rho_old"), A.diag.p, A.source.p);
}

void p_post_solve(Ctx& x) {
  Matrix& A = x.mP;
  MeshView m = x.view();
  k_bc_correct(x, "p", x.f("p"), x.f("boundary_p"), 1);
  halo_fields(x, {"p"});
  // owner-slot face storage: the cell walk of k_p_cell_post writes phi too (fv.p_post_fused), one gather of p at
  // the neighbours instead of two
  const bool fused = x.fslot && x.Fs > 0 && x.on("fv.p_post_fused");
  if (!fused) LAUNCH(k_p_flux_face, x.Fs, m, x.f("phiHbyA"), A.lower.p, A.upper.p, x.f("p"), x.f("phi"));
  LAUNCH(k_p_flux_slot, x.B, m, x.st("p"), x.f("boundary_phiHbyA"), A.ic.p, A.bc.p, x.f("p"), x.f("boundary_p"),
         x.f("boundary_phi"));
  if (fused)
    LAUNCH_W(k_p_cell_post_phi, x.C, m, x.st("p"), x.f("p"), x.f("boundary_p"), x.f("p_old"), x.f("HbyA"), x.f("rAU"),
             x.f("U"), x.f("K"), x.f("dpdt"), x.f("phiHbyA"), A.lower.p, A.upper.p, x.f("phi"));
  else
    LAUNCH_W(k_p_cell_post, x.C, m, x.st("p"), x.f("p"), x.f("boundary_p"), x.f("p_old"), x.f("HbyA"), x.f("rAU"),
             x.f("U"), x.f("K"), x.f("dpdt"));
  k_bc_correct(x, "U", x.f("U"), x.f("boundary_U"), 3);
  halo_fields(x, {"U"});
  LAUNCH(k_kinetic_slots, x.B, x.B, x.f("boundary_U"), x.f("boundary_K"));
}

// species count: register-resident templates for 2..16 species, the chunked kernels above otherwise
// (or always, with the option fv.species_generic -- the parity tests run both on the same mechanisms)
bool species_generic(const Ctx& x) { return x.S > 16 || x.on("fv.species_generic"); }
#define DFMI_SWITCH_S(S, CALL, GEN)                                                              \
  if (species_generic(x)) { GEN; } else switch (S) {                                             \
    case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; case 5: CALL(5); break; \
    case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break; case 9: CALL(9); break; \
    case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;                  \
    case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break;                  \
    case 16: CALL(16); break;                                                                      \
    default: throw Error("dfmi: species count " + std::to_string(S) + " not supported");          \
  }

// div(phi,Yi_h) weights from this step's Y, he and phi (YEqn.H:6-14: the multivariate scheme is built at the
// start of YEqn and EEqn reuses it)
void conv_weights(Ctx& x) {
  if (x.sch.yh == SCH_UPWIND) return;
  scheme_checks(x, true);
  double* w = scheme_buf(x, "conv_w", x.Fs, 1, true);
  double* bw = scheme_buf(x, "boundary_conv_w", x.B, 1);
  const int b01 = x.sch.yh == SCH_LL01;
  const double twoByk = 2.0 / std::max(x.sch.k_yh, 1e-15);
  MeshView m = x.view();
  if (x.conv_list.n < (size_t)std::max(x.Fs, 1)) x.conv_list.alloc(std::max(x.Fs, 1));
  if (!x.conv_nlist.n) x.conv_nlist.alloc(1);
  DFMI_HIP(hipMemsetAsync(x.conv_nlist.p, 0, sizeof(int), x.stream));
  {
    KScope _ks(x, "k_conv_w_check");
    const int blocks = (int)((x.Fs + (long)CK_TPB * CK_FPT - 1) / ((long)CK_TPB * CK_FPT));
    if (blocks > 0)
      hipLaunchKernelGGL(k_conv_w_check, dim3(blocks), dim3(CK_TPB), 0, x.stream, m, x.S, b01, x.f("phi"), x.f("Y"),
                         x.f("he"), w, x.conv_list.p, x.conv_nlist.p);
    DFMI_HIP(hipGetLastError());
  }
  {
    KScope _ks(x, "k_conv_w_list");   // a fixed grid of 16-lane groups strides over the listed faces
    const int blocks = std::min(4096, std::max(1, blocks_for(x.Fs, 256 / CWG)));
    if (face_hex(x))
      hipLaunchKernelGGL(k_conv_w_list<-1>, dim3(blocks), dim3(256), 0, x.stream, m, x.S, x.st("Y"), x.st("he"), twoByk,
                         x.f("phi"), x.f("Y"), x.f("boundary_Y"), x.f("he"), x.f("boundary_he"), x.conv_list.p,
                         x.conv_nlist.p, w);
    else if (face_rows(x))
      hipLaunchKernelGGL(k_conv_w_list<6>, dim3(blocks), dim3(256), 0, x.stream, m, x.S, x.st("Y"), x.st("he"), twoByk,
                         x.f("phi"), x.f("Y"), x.f("boundary_Y"), x.f("he"), x.f("boundary_he"), x.conv_list.p,
                         x.conv_nlist.p, w);
    else
      hipLaunchKernelGGL(k_conv_w_list<0>, dim3(blocks), dim3(256), 0, x.stream, m, x.S, x.st("Y"), x.st("he"), twoByk,
                         x.f("phi"), x.f("Y"), x.f("boundary_Y"), x.f("he"), x.f("boundary_he"), x.conv_list.p,
                         x.conv_nlist.p, w);
    DFMI_HIP(hipGetLastError());
  }
  const double* bgx = nullptr;
  if (halo_active(x)) {   // processor faces: the neighbour cells' gradients (LimitedScheme::calcLimiter's pGradcN)
    double* g = scheme_buf(x, "conv_grad", x.C, 3 * (x.S + 1));
    bgx = scheme_buf(x, "boundary_conv_grad", x.B, 3 * (x.S + 1));
    LAUNCH(k_conv_proc_grad, x.B, m, x.S, x.st("Y"), x.st("he"), x.f("Y"), x.f("boundary_Y"), x.f("he"),
           x.f("boundary_he"), g);
    halo_fields(x, {"conv_grad"});
  }
  LAUNCH(k_conv_w_slot, x.B, m, x.S, x.st("Y"), x.st("he"), b01, twoByk, x.f("boundary_phi"), x.f("Y"),
         x.f("boundary_Y"), x.f("he"), x.f("boundary_he"), bgx, bw);
}

// div(phi,K) weights and div(hDiffCorrFlux)'s cubic correction (EEqn.H's fvc::div(phi, K), fvc::div(hDiffCorrFlux))
static void e_scheme_terms(Ctx& x) {
  MeshView m = x.view();
  if (x.sch.K != SCH_LINEAR) {
    const bool lim = x.sch.K == SCH_LL || x.sch.K == SCH_LL01;
    scheme_checks(x, false);
    double* w = scheme_buf(x, "K_w", x.Fs, 1, true);
    double* bw = scheme_buf(x, "boundary_K_w", x.B, 1);
    double* g = scheme_buf(x, "gradK", x.C, 3);
    double* bg = scheme_buf(x, "boundary_gradK", x.B, 3);
    if (lim) {
      DFMI_CHECK(x.have_md, "limited schemes need mesh_distance (dfmi_init_constant_fields_internal)");
      bool coupled = false;
      for (int p = 0; p < x.P; ++p) coupled |= x.pkind[p] != 0;
      DFMI_CHECK(!coupled || x.have_bdelta, "limited schemes on a mesh with coupled patches need dfmi_init_boundary_delta");
      if (face_hex(x)) LAUNCH((k_grad_cells<1, -1>), x.C, m, x.st("K"), x.f("K"), x.f("boundary_K"), g);
      else if (face_rows(x)) LAUNCH((k_grad_cells<1, 6>), x.C, m, x.st("K"), x.f("K"), x.f("boundary_K"), g);
      else LAUNCH((k_grad_cells<1, 0>), x.C, m, x.st("K"), x.f("K"), x.f("boundary_K"), g);
      halo_fields(x, {"gradK"});   // the neighbour cell's gradient on processor faces (patchNeighbourField)
    }
    // upwind: limiter 0 everywhere (Limited01 with bounds that reject every face)
    const int b01 = lim ? (x.sch.K == SCH_LL01) : 1;
    const double twoByk = 2.0 / std::max(x.sch.k_K, 1e-15);
    if (lim) {
      if (face_hex(x)) LAUNCH(k_lim_w_cell, x.C, m, b01, twoByk, x.f("phi"), x.f("K"), g, w);
      else LAUNCH(k_lim_w_face, x.Fs, m, b01, twoByk, x.f("phi"), x.f("K"), g, w);
      LAUNCH(k_lim_w_slot, x.B, m, x.st("K"), b01, twoByk, x.f("boundary_phi"), x.f("K"), x.f("boundary_K"), g, bg, bw);
    } else {
      LAUNCH(k_upwind_w_face, x.Fs, m, x.f("phi"), w);
      LAUNCH(k_upwind_w_slot, x.B, m, x.f("boundary_phi"), bw);
    }
  }
  if (x.sch.hD == SCH_CUBIC && !x.turbulent()) {   // LES: no div(hDiffCorrFlux) (EEqn.H:30-36), so no correction of it
    double* cf = scheme_buf(x, "cubic_flux", x.Fs, 1, true);
    double* bcf = scheme_buf(x, "boundary_cubic_flux", x.B, 1);
    double* g = scheme_buf(x, "gradHD", x.C, 9);
    scheme_buf(x, "boundary_gradHD", x.B, 9);
    if (face_hex(x)) LAUNCH((k_grad_cells<3, -1>), x.C, m, x.st("calculated"), x.f("hDiffCorrFlux"), x.f("boundary_hDiffCorrFlux"), g);
    else if (face_rows(x)) LAUNCH((k_grad_cells<3, 6>), x.C, m, x.st("calculated"), x.f("hDiffCorrFlux"), x.f("boundary_hDiffCorrFlux"), g);
    else LAUNCH((k_grad_cells<3, 0>), x.C, m, x.st("calculated"), x.f("hDiffCorrFlux"), x.f("boundary_hDiffCorrFlux"), g);
    halo_fields(x, {"gradHD"});
    if (face_hex(x)) LAUNCH(k_cubic_cell, x.C, m, x.f("hDiffCorrFlux"), g, cf);
    else LAUNCH(k_cubic_face, x.Fs, m, x.f("hDiffCorrFlux"), g, cf);
    LAUNCH(k_cubic_slot, x.B, m, x.st("calculated"), x.f("hDiffCorrFlux"), x.f("boundary_hDiffCorrFlux"), g,
           x.f("boundary_gradHD"), bcf);
  }
}

void y_prep(Ctx& x, bool weights) {
  if (weights) conv_weights(x);   // div(phi,Yi_h) weights of this step (before Y changes)
  // LES (simulationType != laminar): the reference drops fvmDiv(phiUc, Yi), diffAlphaD and div(hDiffCorrFlux)
  // (YEqn.H:101-106, EEqn.H:30-36) -- everything below; their fields stay zero (les_effective)
  if (x.turbulent()) return;
  MeshView m = x.view();
  double* gout = x.fields.count("dbg_gradY") ? x.f("dbg_gradY") : nullptr;
// (k_y_prep: the CSR walk measured faster than the gather rows -- 667 vs 848 us on the 2M box; its
// 243 VGPRs leave no room for the up-front row loads). Measured slower and removed (round 5): the species-outer
// row kernel (767-793 vs 657-673 us) and the z-marching tiles (811 vs 620 us), DESIGN.md 8.
  // LDS-staged brick kernel on hex boxes whose dimensions the brick divides (fv.yprep_brick = 0: off)
  const bool brick = face_hex(x) && !x.trav.n && x.hex[0] % YBX == 0 && x.hex[1] % YBY == 0 && x.hex[2] % YBZ == 0 &&
                     x.on("fv.yprep_brick");
#define CALL(NS)                                                                                                     \
  do {                                                                                                               \
    if (brick)                                                                                                       \
      LAUNCH_AS("k_y_prep", (k_y_prep_brick<NS, ybrick_sc(NS)>), x.C, m, x.st("Y"), x.f("Y"), x.f("boundary_Y"),    \
             x.f("rhoD"), x.f("boundary_rhoD"), x.f("hai"), x.f("boundary_hai"), x.f("alpha"), x.f("boundary_alpha"), \
             x.f("sumYDiffError"), x.f("boundary_sumYDiffError"), x.f("hDiffCorrFlux"),                              \
             x.f("boundary_hDiffCorrFlux"), x.f("diffAlphaD"), gout);                                               \
    else if (face_hex(x))                                                                                            \
      LAUNCH((k_y_prep<NS, -1>), x.C, m, x.st("Y"), x.f("Y"), x.f("boundary_Y"), x.f("rhoD"), x.f("boundary_rhoD"),  \
             x.f("hai"), x.f("boundary_hai"), x.f("alpha"), x.f("boundary_alpha"), x.f("sumYDiffError"),             \
             x.f("boundary_sumYDiffError"), x.f("hDiffCorrFlux"), x.f("boundary_hDiffCorrFlux"), x.f("diffAlphaD"),  \
             gout);                                                                                                  \
    else                                                                                                             \
      LAUNCH((k_y_prep<NS, 0>), x.C, m, x.st("Y"), x.f("Y"), x.f("boundary_Y"), x.f("rhoD"), x.f("boundary_rhoD"),   \
             x.f("hai"), x.f("boundary_hai"), x.f("alpha"), x.f("boundary_alpha"), x.f("sumYDiffError"),             \
             x.f("boundary_sumYDiffError"), x.f("hDiffCorrFlux"), x.f("boundary_hDiffCorrFlux"), x.f("diffAlphaD"),  \
             gout);                                                                                                  \
  } while (0)
  // the chunked kernel (4 species per chunk: 7.0 ms against 7.4-9.5 for chunks of 2 / 3 / 8 on 2M x 53 species) in
  // species ranges of YPREP_LCH species per launch (L2 locality of the neighbour gathers: 8.74 -> 8.56-8.62 ms
  // with 8 or 16), pass 1 over every range, then pass 2 (it reads the finished sumYDiffError)
#define GEN(CH)                                                                                                      \
  do {                                                                                                               \
    constexpr int lch = YPREP_LCH / CH * CH;                                                                         \
    for (int pass = 1; pass <= 2; ++pass)                                                                            \
      for (int s_lo = 0; s_lo < x.S; s_lo += lch)                                                                    \
        LAUNCH_SWG(k_y_prep_gen, CH, x.C, m, s_lo, std::min(x.S, s_lo + lch), pass, x.st("Y"), x.f("Y"),             \
                   x.f("boundary_Y"), x.f("rhoD"), x.f("boundary_rhoD"), x.f("hai"), x.f("boundary_hai"), x.f("alpha"), \
                   x.f("boundary_alpha"), x.f("sumYDiffError"), x.f("boundary_sumYDiffError"), x.f("hDiffCorrFlux"),  \
                   x.f("boundary_hDiffCorrFlux"), x.f("diffAlphaD"), pass == 1 ? gout : nullptr);                   \
  } while (0)
  DFMI_SWITCH_S(x.S, CALL, GEN(4))
#undef GEN
#undef CALL
  halo_fields(x, {"sumYDiffError", "hDiffCorrFlux"});
  LAUNCH(k_phiuc_face, x.Fs, m, x.f("sumYDiffError"), x.f("phiUc"));
  LAUNCH(k_phiuc_slot, x.B, m, x.st("Y"), x.f("sumYDiffError"), x.f("boundary_sumYDiffError"), x.f("boundary_phiUc"));
}

void y_assemble(Ctx& x, bool spray) {
  Matrix& A = x.mY;
  MeshView m = x.view();
#define CALL(NS) LAUNCH_SWL(k_y_assemble, NS, x.C, m, x.st("Y"), x.inert, x.f("Y"), x.f("boundary_Y"), x.f("rhoD"),   \
                        x.f("boundary_rhoD"), x.rr_src(), x.f("rho"), x.f("rho_old"), x.f("phi"), x.f("boundary_phi"), \
                        x.f("phiUc"), x.f("boundary_phiUc"), A.lower.p, A.upper.p, A.diag.p, A.source.p, A.ic.p, A.bc.p, mixbc(x, "Y"), x.sch_w(0), x.sch_w(1))
  DFMI_SWITCH_S(x.S, CALL,
                LAUNCH_SWGL(k_y_assemble_gen, YCH, x.C, m, x.S, x.st("Y"), x.inert, x.f("Y"), x.f("boundary_Y"), x.f("rhoD"),
                       x.f("boundary_rhoD"), x.rr_src(), x.f("rho"), x.f("rho_old"), x.f("phi"), x.f("boundary_phi"),
                       x.f("phiUc"), x.f("boundary_phiUc"), A.lower.p, A.upper.p, A.diag.p, A.source.p, A.ic.p, A.bc.p, mixbc(x, "Y"), x.sch_w(0), x.sch_w(1)))
#undef CALL
  if (x.lap == LAP_CORRECTED) nonorth_y(x, A.source.p, nullptr, 0);
  if (spray) spray_fold_y(x, A.diag.p, A.source.p, x.C, false);   // parcels.SYi(i, Yi), after the non-orthogonal term
}

void y_assemble_ell(Ctx& x, int W, long Ce, double* val, double* dS, double* rhs) {
  MeshView m = x.view();
  // (the z-marching tile form measured slower than this cell-parallel kernel, 961 vs 622 us, and is removed)
#define CALL(NS)                                                                                                     \
  LAUNCH_SWL(k_y_assemble_ell, NS, x.C, m, x.st("Y"), x.inert, x.f("Y"), x.f("boundary_Y"), x.f("rhoD"),              \
            x.f("boundary_rhoD"), x.rr_src(), x.f("rho"), x.f("rho_old"), x.f("phi"),                                 \
            x.f("boundary_phi"), x.f("phiUc"), x.f("boundary_phiUc"), W, Ce, val, dS, rhs, mixbc(x, "Y"), x.sch_w(0), x.sch_w(1))
  // chunked kernel: 8 species per chunk, species ranges of YASM_LCH per launch (assembly 5.98 -> 5.86 ms per step
  // on 2M x 53 species with 8)
#define GEN(CH)                                                                                                      \
  do {                                                                                                               \
    constexpr int lch = YASM_LCH / CH * CH;                                                                          \
    for (int s_lo = 0; s_lo < x.S; s_lo += lch)                                                                      \
      LAUNCH_SWGL(k_y_assemble_ell_gen, CH, x.C, m, s_lo, std::min(x.S, s_lo + lch), x.st("Y"), x.inert, x.f("Y"),    \
                 x.f("boundary_Y"), x.f("rhoD"), x.f("boundary_rhoD"), x.rr_src(), x.f("rho"), x.f("rho_old"), x.f("phi"), \
                 x.f("boundary_phi"), x.f("phiUc"), x.f("boundary_phiUc"), W, Ce, val, dS, rhs, mixbc(x, "Y"),       \
                 x.sch_w(0), x.sch_w(1));                                                                            \
  } while (0)
  DFMI_SWITCH_S(x.S, CALL, GEN(8))
#undef GEN
#undef CALL
  if (x.lap == LAP_CORRECTED) nonorth_y(x, nullptr, rhs, Ce);
  spray_fold_y(x, dS, rhs, Ce, true);
}

void y_post_solve(Ctx& x) {
#define CALL(NS) LAUNCH(k_y_inert<NS>, x.C, x.C, x.inert, x.f("Y"))
  DFMI_SWITCH_S(x.S, CALL, LAUNCH(k_y_inert_gen, x.C, x.C, x.S, x.inert, x.f("Y")))
#undef CALL
  k_bc_correct(x, "Y", x.f("Y"), x.f("boundary_Y"), x.S);
  halo_fields(x, {"Y"});
}

// EEqn assembly in two parts: the scheme terms (K's limited weights from the UEqn's K, hDiffCorrFlux's cubic
// correction from the YEqn preparation) read nothing of the Y solve; the boundary energy gradient (the
// thermo at the solved boundary Y), he's boundary values and the matrix come after it
void e_assemble_front(Ctx& x) { e_scheme_terms(x); }
void e_assemble_back(Ctx& x) {
  Matrix& A = x.mE;
  MeshView m = x.view();
  thermo_energy_gradient(x);   // eeqn_calculate_energy_gradient (dfEEqn.cu:148, :266-287)
  k_bc_correct(x, "he", x.f("he"), x.f("boundary_he"), 1);
  const double* eg = x.f("boundary_heGradient");
  LAUNCH_W(k_e_assemble, x.C, m, x.st("he"), x.st("K"), x.f("he"), x.f("boundary_he"), x.f("rho"), x.f("rho_old"),
         x.f("K"), x.f("K_old"), x.f("boundary_K"), x.f("phi"), x.f("boundary_phi"), x.cond(false),
         x.cond(true), x.f("hDiffCorrFlux"), x.f("boundary_hDiffCorrFlux"), x.f("dpdt"), x.f("diffAlphaD"),
         eg, A.lower.p, A.upper.p, A.diag.p, A.source.p, A.ic.p, A.bc.p, x.sch_w(0), x.sch_w(1), x.sch_w(2),
         x.sch_w(3), x.sch_w(4), x.sch_w(5));
  if (x.lap == LAP_CORRECTED) nonorth_e(x);
  spray_fold_e(x);   // parcels.Sh(he) and hcSource, after the non-orthogonal term
}
void e_assemble(Ctx& x) {
  e_assemble_front(x);
  e_assemble_back(x);
}

// ---- non-orthogonal laplacians (dfmi_set_scheme "laplacian")
void nonorth_setup(Ctx& x) {
  double* ndc = scheme_buf(x, "nonorth_delta_coeffs", x.Fs, 1, true);
  double* nk = scheme_buf(x, "nonorth_corr", x.Fs, 3, true);
  double* nbdc = scheme_buf(x, "boundary_nonorth_delta_coeffs", x.B, 1);
  double* nbk = scheme_buf(x, "boundary_nonorth_corr", x.B, 3);
  const int lap = x.lap;
  x.lap = LAP_ORTHOGONAL;   // the view with the caller's deltaCoeffs: the slots that are not coupled copy them
  const MeshView m = x.view();
  x.lap = lap;
  LAUNCH(k_nonorth_geom_face, x.Fs, m, ndc, nk);
  LAUNCH(k_nonorth_geom_slot, x.B, m, x.st("calculated"), x.bdc.p, nbdc, nbk);
  x.no_dc = ndc; x.no_bdc = nbdc; x.no_k = nk; x.no_bk = nbk;
}
#define LAUNCH_NO(NC, MODE, ty, a) \
  do { if (face_hex(x)) LAUNCH((k_nonorth_corr<NC, -1, MODE>), x.C, m, ty, a); \
       else if (face_rows(x)) LAUNCH((k_nonorth_corr<NC, 6, MODE>), x.C, m, ty, a); \
       else LAUNCH((k_nonorth_corr<NC, 0, MODE>), x.C, m, ty, a); } while (0)
#define LAUNCH_GRAD(NC, ty, vf, bvf, g) \
  do { if (face_hex(x)) LAUNCH((k_grad_cells<NC, -1>), x.C, m, ty, vf, bvf, g); \
       else if (face_rows(x)) LAUNCH((k_grad_cells<NC, 6>), x.C, m, ty, vf, bvf, g); \
       else LAUNCH((k_grad_cells<NC, 0>), x.C, m, ty, vf, bvf, g); } while (0)
static NoArgs no_args(Ctx& x) {
  NoArgs a{};
  a.nk = x.no_k; a.bnk = x.no_bk; a.gk = 3; a.gd = 1; a.inert = -1;
  return a;
}
// UEqn: - fvm::laplacian(mu, U), the three components on one walk from k_u_grad's gradient (u_assemble's gout)
static void nonorth_u(Ctx& x) {
  const MeshView m = x.view();
  scheme_buf(x, "boundary_gradU", x.B, 9);
  halo_fields(x, {"gradU"});   // the neighbour cell's gradient on processor faces
  NoArgs a = no_args(x);
  a.g = x.f("gradU"); a.bg = x.f("boundary_gradU"); a.gk = 1; a.gd = 3;
  a.gam = x.visc(false); a.bgam = x.visc(true);
  a.src = x.mU.source.p; a.src2 = x.mU.source_solve.p;
  LAUNCH_NO(3, NO_SHARED, x.st("U"), a);
}
// EEqn: - fvm::laplacian(alpha, he) from he / boundary_he as the assembly read them
static void nonorth_e(Ctx& x) {
  const MeshView m = x.view();
  double* g = scheme_buf(x, "nonorth_grad", x.C, 3);
  scheme_buf(x, "boundary_nonorth_grad", x.B, 3);
  LAUNCH_GRAD(1, x.st("he"), x.f("he"), x.f("boundary_he"), g);
  halo_fields(x, {"nonorth_grad"});
  NoArgs a = no_args(x);
  a.g = g; a.bg = x.f("boundary_nonorth_grad");
  a.gam = x.cond(false); a.bgam = x.cond(true);
  a.src = x.mE.source.p;
  LAUNCH_NO(1, NO_SHARED, x.st("he"), a);
}
// YEqn: laplacian(rhoD_i, Yi) on the right-hand side, into the LDU source (src) or the solver rows' rhs, and
// diffAlphaD's fvc::laplacian(alpha hai_i, Yi) on the same walk (y_prep wrote its orthogonal part just before: every
// YEqn assembly follows a y_prep). Species in chunks of 4 (then singly), so the gradients take [12][C] at any S.
static void nonorth_y(Ctx& x, double* src, double* rhs, long Ce) {
  const MeshView m = x.view();
  double* g = scheme_buf(x, "nonorth_gradY", x.C, 12);
  scheme_buf(x, "boundary_nonorth_gradY", x.B, 12);
  NoArgs a = no_args(x);
  a.g = g; a.bg = x.f("boundary_nonorth_gradY");
  a.gam = x.f("rhoD"); a.bgam = x.f("boundary_rhoD"); a.add = x.mut_sct(false); a.badd = x.mut_sct(true);
  a.src = src; a.rhs = rhs; a.Ce = Ce; a.S = x.S; a.inert = x.inert;
  if (!x.turbulent()) {   // LES / RAS drop diffAlphaD (y_prep)
    a.alpha = x.f("alpha"); a.balpha = x.f("boundary_alpha"); a.hai = x.f("hai"); a.bhai = x.f("boundary_hai");
    a.dAD = x.f("diffAlphaD");
  }
  const int8_t* ty = x.st("Y");
  for (int s0 = 0; s0 < x.S;) {
    const int n = x.S - s0 >= 4 ? 4 : 1;
    const double *vf = x.f("Y") + (long)s0 * x.C, *bvf = x.f("boundary_Y") + (long)s0 * x.B;
    a.s0 = s0;
    if (n == 4) LAUNCH_GRAD(4, ty, vf, bvf, g); else LAUNCH_GRAD(1, ty, vf, bvf, g);
    if (halo_active(x)) {   // the neighbour cells' gradients on processor faces: only the components this chunk formed
      CommTag _ct(x, "fields nonorth_gradY");
      const HaloItem it{g, x.f("boundary_nonorth_gradY"), 3 * n, (long)x.C, (long)x.B, true};
      halo_update(x, &it, 1);
    }
    if (n == 4) LAUNCH_NO(4, NO_SPECIES, ty, a); else LAUNCH_NO(1, NO_SPECIES, ty, a);
    s0 += n;
  }
}
// pEqn (do_p's non-orthogonal corrector loop): the source k_p_cell wrote is kept as the base; every pass forms
// grad(p) from p / boundary_p as they stand and source = base + the divergence of the face flux correction
void nonorth_p_base(Ctx& x) {
  double* base = scheme_buf(x, "nonorth_p_base", x.C, 1);
  DFMI_HIP(hipMemcpyAsync(base, x.mP.source.p, sizeof(double) * x.C, hipMemcpyDeviceToDevice, x.stream));
}
void nonorth_p_correct(Ctx& x) {
  const MeshView m = x.view();
  double* g = scheme_buf(x, "nonorth_grad", x.C, 3);
  scheme_buf(x, "boundary_nonorth_grad", x.B, 3);
  LAUNCH_GRAD(1, x.st("p"), x.f("p"), x.f("boundary_p"), g);
  halo_fields(x, {"nonorth_grad"});
  NoArgs a = no_args(x);
  a.g = g; a.bg = x.f("boundary_nonorth_grad");
  a.gam = x.f("rhorAUf"); a.bgam = x.f("boundary_rhorAUf");
  a.src = x.mP.source.p; a.base = x.f("nonorth_p_base");
  a.fcorr = scheme_buf(x, "nonorth_p_flux", x.Fs, 1, true); a.bfcorr = scheme_buf(x, "boundary_nonorth_p_flux", x.B, 1);
  LAUNCH_NO(1, NO_FACE, x.st("p"), a);
}
// phi = phiHbyA + pEqn.flux() includes the face flux correction of the last pass (after p_post_solve wrote phi)
void nonorth_p_flux(Ctx& x) {
  const MeshView m = x.view();
  LAUNCH(k_nonorth_flux_face, x.Fs, m, x.f("nonorth_p_flux"), x.f("phi"));
  LAUNCH(k_nonorth_flux_slot, x.B, m, x.st("p"), x.f("boundary_nonorth_p_flux"), x.f("boundary_phi"));
}

// ---- RAS k-epsilon (include/dfmi.h)
static RasCoef ras_coef(Ctx& x) {
  return {x.opt("ras.Cmu"), x.opt("ras.C1"), x.opt("ras.C2"), x.opt("ras.C3"), x.opt("ras.sigmak"), x.opt("ras.sigmaEps"),
          x.opt("ras.kMin"), x.opt("ras.epsilonMin")};
}
static void ras_check_set(Ctx& x) {
  static const char* names[4] = {"k", "epsilon", "boundary_k", "boundary_epsilon"};
  for (int i = 0; i < 4; ++i)
    DFMI_CHECK(x.ras.have[i], std::string("RAS: the field '") + names[i] + "' is not set (dfmi_set_field)");
}
void ras_production(Ctx& x) {
  ras_check_set(x);
  // several ranks: the neighbour half of the processor slots of k and epsilon as the caller set them (the limiter's and
  // the corrected laplacian's gradients read the cell across a processor face; later calls find what ras_post_solve left)
  halo_fields(x, {"k", "epsilon"});
  if (!x.ras.valid) ras_nut(x);   // the old nut of k and epsilon as they stand
  LAUNCH_W(k_ras_production, x.C, x.view(), x.st("U"), x.st("rho"), x.f("U"), x.f("boundary_U"), x.f("phi"),
           x.f("boundary_phi"), x.f("rho"), x.f("boundary_rho"), x.f("nut"), x.f("G"), x.f("divU"));
}
// convection weights of one scalar (dfmi_set_scheme div(phi,k) / div(phi,epsilon)): nullptr for upwind, the mesh's for
// linear, k_lim_w_* from the gradient g / bg for limitedLinear
static void ras_weights(Ctx& x, int kind, double kcoef, const char* nm, const double* g, const double* bg, const double*& w,
                        const double*& bw) {
  w = nullptr; bw = nullptr;
  if (kind == SCH_UPWIND) return;
  if (kind == SCH_LINEAR) { w = x.w.p; bw = x.bw.p; return; }
  const MeshView m = x.view();
  const std::string bn = std::string("boundary_") + nm;
  double* wo = scheme_buf(x, "ras_w", x.Fs, 1, true);
  double* bwo = scheme_buf(x, "boundary_ras_w", x.B, 1);
  const double twoByk = 2.0 / std::max(kcoef, 1e-15);
  if (face_hex(x)) LAUNCH(k_lim_w_cell, x.C, m, 0, twoByk, x.f("phi"), x.f(nm), g, wo);
  else LAUNCH(k_lim_w_face, x.Fs, m, 0, twoByk, x.f("phi"), x.f(nm), g, wo);
  LAUNCH(k_lim_w_slot, x.B, m, x.st(nm), 0, twoByk, x.f("boundary_phi"), x.f(nm), x.f(bn), g, bg, bwo);
  w = wo; bw = bwo;
}
void ras_assemble(Ctx& x, int keq) {
  ras_check_set(x);
  const char* nm = keq ? "k" : "epsilon";
  const std::string bn = std::string("boundary_") + nm;
  const RasCoef q = ras_coef(x);
  const MeshView m = x.view();
  Matrix& A = x.mK;
  LAUNCH(k_ras_sources, x.C, (long)x.C, keq, q, x.f("G"), x.f("divU"), x.f("rho"), x.f("k"), x.f("epsilon"), x.f("nut"),
         x.f("mu"), x.f("ras_Su"), x.f("ras_Sp"), x.f("ras_D"));
  LAUNCH(k_ras_diffusivity, x.B, (long)x.B, x.f("boundary_rho"), x.f("boundary_nut"), x.f("boundary_mu"),
         keq ? q.sigmak : q.sigmaEps, x.f("boundary_ras_D"));
  const int kind = keq ? x.sch.tk : x.sch.teps;
  const bool lim = kind == SCH_LL, corr = x.lap == LAP_CORRECTED;
  const int8_t* ty = x.st(nm);
  double *g = nullptr, *bg = nullptr;
  if (lim || corr) {   // the field's Gauss gradient: the limiter's upwind-cell gradient and the corrected laplacian's
    if (lim) scheme_checks(x, true);
    g = scheme_buf(x, "ras_grad", x.C, 3);
    bg = scheme_buf(x, "boundary_ras_grad", x.B, 3);
    LAUNCH_GRAD(1, ty, x.f(nm), x.f(bn), g);
    halo_fields(x, {"ras_grad"});   // the neighbour cell's gradient on processor faces
  }
  const double *w, *bw;
  ras_weights(x, kind, keq ? x.sch.k_tk : x.sch.k_teps, nm, g, bg, w, bw);
  // epsilonWallFunction: the epsilon matrix is constrained on the wall cells (an instantiation of its own)
  const bool con = !keq && (x.wf.bits & Ctx::WF_EPS_WALL);
  if (con) {
    const int8_t* cf = x.wf.cflag.p;
#define SCALAR_CON(WT) \
    LAUNCH_AS("k_scalar_assemble", (k_scalar_assemble<WT, true>), x.C, m, ty, x.f(nm), x.f(bn), x.f("rho"), x.f("rho_old"), \
              x.f("phi"), x.f("boundary_phi"), x.f("ras_D"), x.f("boundary_ras_D"), x.f("ras_Su"), x.f("ras_Sp"), A.lower.p, \
              A.upper.p, A.diag.p, A.source.p, A.ic.p, A.bc.p, mixbc(x, nm), w, bw, cf)
    if (face_hex(x)) SCALAR_CON(-1); else if (face_rows(x)) SCALAR_CON(6); else SCALAR_CON(0);
#undef SCALAR_CON
  } else
  LAUNCH_W(k_scalar_assemble, x.C, m, ty, x.f(nm), x.f(bn), x.f("rho"), x.f("rho_old"), x.f("phi"), x.f("boundary_phi"),
           x.f("ras_D"), x.f("boundary_ras_D"), x.f("ras_Su"), x.f("ras_Sp"), A.lower.p, A.upper.p, A.diag.p, A.source.p,
           A.ic.p, A.bc.p, mixbc(x, nm), w, bw);
  if (corr) {   // - fvm::laplacian(D, psi): the explicit non-orthogonal term
    NoArgs a = no_args(x);
    a.g = g; a.bg = bg;
    a.gam = x.f("ras_D"); a.bgam = x.f("boundary_ras_D");
    a.src = A.source.p;
    LAUNCH_NO(1, NO_SHARED, ty, a);
    if (con) LAUNCH(k_ras_constrain_source, x.C, (long)x.C, x.wf.cflag.p, x.f(nm), A.diag.p, A.source.p);
  }
}
// after the solve: the field's boundary values and halo (fvMatrix::solve's correctBoundaryConditions), then bound()
// as a gather from a copy of the solved field, max(., lo) on every slot, and the bounded cells' halo
void ras_post_solve(Ctx& x, int keq) {
  const char* nm = keq ? "k" : "epsilon";
  const std::string bn = std::string("boundary_") + nm, pre = std::string(nm) + "_prebound", bpre = "boundary_" + pre;
  const double lo = x.opt(keq ? "ras.kMin" : "ras.epsilonMin");
  k_bc_correct(x, nm, x.f(nm), x.f(bn), 1);
  halo_fields(x, {nm});
  DFMI_HIP(hipMemcpyAsync(x.f(pre), x.f(nm), sizeof(double) * x.C, hipMemcpyDeviceToDevice, x.stream));
  if (x.B) DFMI_HIP(hipMemcpyAsync(x.f(bpre), x.f(bn), sizeof(double) * x.B, hipMemcpyDeviceToDevice, x.stream));
  LAUNCH_W(k_ras_bound, x.C, x.view(), x.st(nm), x.f(pre), x.f(bpre), lo, x.f(nm));
  LAUNCH(k_ras_bound_slots, x.B, (long)x.B, lo, x.f(bn));
  halo_fields(x, {nm});
}
static WallTab wall_tab(Ctx& x) { return {x.wf.sflag.p, x.wf.spatch.p, x.wf.tab.p}; }
// correctNut(): nut = Cmu k^2 / epsilon on cells and on nut's `calculated` slots, boundary_nut by nut's patch types, halo
void ras_nut(Ctx& x) {
  ras_check_set(x);
  const double Cmu = x.opt("ras.Cmu");
  const char* tn = x.stype.count("nut") ? "nut" : "calculated";
  LAUNCH(k_ras_nut, x.C, (long)x.C, (const int8_t*)nullptr, Cmu, x.f("k"), x.f("epsilon"), x.f("nut"));
  LAUNCH(k_ras_nut, x.B, (long)x.B, x.st(tn), Cmu, x.f("boundary_k"), x.f("boundary_epsilon"), x.f("boundary_nut"));
  k_bc_correct(x, tn, x.f("nut"), x.f("boundary_nut"), 1);
  ras_wall_refresh(x, false);
  if (x.wf.bits & Ctx::WF_NUT_WALL)   // nutkWallFunction slots from the current k: a launch of its own
    LAUNCH(k_ras_nut_wall, x.B, (long)x.B, wall_tab(x), x.bfc.p, x.bdc.p, x.f("k"), x.f("boundary_mu"), x.f("boundary_rho"),
           x.f("boundary_nut"), x.f("boundary_yPlus"));
  halo_fields(x, {"nut"});
  x.ras.valid = true;
}
// ---- wall functions and turbulent inlets
// yPlusLam of (kappa, E): ypl = 11, then ten times ypl = log(max(E ypl, 1)) / kappa
static double y_plus_lam(double kappa, double E) {
  double ypl = 11.0;
  for (int i = 0; i < 10; ++i) ypl = std::log(std::max(E * ypl, 1.0)) / kappa;
  return ypl;
}
void ras_wall_refresh(Ctx& x, bool inlets) {
  Ctx::WallFn& w = x.wf;
  if (!w.in_use) return;
  auto code = [&](const char* f, int p) { auto it = x.ptype.find(f); return it == x.ptype.end() ? -1 : it->second[p]; };
  for (int p = 0; p < x.P; ++p) {
    DFMI_CHECK(code("epsilon", p) != EPSILON_WALL_FUNCTION || code("nut", p) == NUTK_WALL_FUNCTION,
               "patch " + std::to_string(p) + ": epsilonWallFunction for epsilon needs nutkWallFunction for nut on the same patch");
    if (!inlets) continue;
    DFMI_CHECK(code("k", p) != TURBULENT_INTENSITY_K_INLET || w.intensity[p] > 0,
               "patch " + std::to_string(p) + ": turbulentIntensityKineticEnergyInlet without an intensity (dfmi_set_patch_param 'k', 'intensity')");
    DFMI_CHECK(code("epsilon", p) != TURBULENT_MIXING_LENGTH_EPSILON_INLET || w.mixingLength[p] > 0,
               "patch " + std::to_string(p) + ": turbulentMixingLengthDissipationRateInlet without a mixing length (dfmi_set_patch_param 'epsilon', 'mixingLength')");
  }
  if (!w.dirty) return;
  std::vector<int8_t> sf((size_t)std::max<long>(x.B, 1), 0);
  std::vector<int> sp((size_t)std::max<long>(x.B, 1), 0);
  std::vector<double> tab((size_t)Ctx::WF_TAB * std::max<long>(x.P, 1), 0.0);
  w.bits = 0;
  for (int p = 0; p < x.P; ++p) {
    int bits = 0;
    if (code("epsilon", p) == EPSILON_WALL_FUNCTION) bits |= Ctx::WF_EPS_WALL;
    if (code("nut", p) == NUTK_WALL_FUNCTION) bits |= Ctx::WF_NUT_WALL;
    if (code("k", p) == TURBULENT_INTENSITY_K_INLET) bits |= Ctx::WF_K_INLET;
    if (code("epsilon", p) == TURBULENT_MIXING_LENGTH_EPSILON_INLET) bits |= Ctx::WF_EPS_INLET;
    w.bits |= bits;
    const int slots = x.pkind[p] == 2 ? 2 * x.psize[p] : x.psize[p];
    for (int i = 0; i < slots; ++i) { sf[x.poff[p] + i] = (int8_t)bits; sp[x.poff[p] + i] = p; }
    double* q = &tab[(size_t)Ctx::WF_TAB * p];
    const double Cmu25 = std::sqrt(std::sqrt(w.Cmu[p]));
    q[0] = Cmu25; q[1] = Cmu25 * std::sqrt(w.Cmu[p]); q[2] = w.kappa[p]; q[3] = w.E[p];
    q[4] = y_plus_lam(w.kappa[p], w.E[p]); q[5] = w.intensity[p]; q[6] = w.mixingLength[p];
  }
  w.sflag.upload(sf, x.stream); w.spatch.upload(sp, x.stream); w.tab.upload(tab, x.stream);
  if (w.cflag.n != (size_t)std::max<long>(x.C, 1)) { w.cflag.alloc((size_t)std::max<long>(x.C, 1)); w.cflag.zero(x.stream); }
  DFMI_HIP(hipStreamSynchronize(x.stream));   // the host vectors go out of scope
  w.dirty = false;
}
void ras_inlet_k(Ctx& x) {
  ras_wall_refresh(x, true);
  if (!(x.wf.bits & Ctx::WF_K_INLET)) return;
  LAUNCH(k_ras_inlet_ref, x.B, (long)x.B, (int)Ctx::WF_K_INLET, wall_tab(x), 0.0, x.f("boundary_U"), x.f("boundary_k"),
         x.f("boundary_k_ref"));
}
void ras_wall_update(Ctx& x) {
  if (x.wf.bits & Ctx::WF_EPS_WALL) {
    LAUNCH(k_ras_wall, x.C, x.view(), wall_tab(x), x.bdc.p, x.f("k"), x.f("U"), x.f("boundary_U"), x.f("boundary_mu"),
           x.f("boundary_rho"), x.f("boundary_nut"), x.f("epsilon"), x.f("G"), x.f("boundary_epsilon"), x.wf.cflag.p);
    // several ranks: the wall cells' new epsilon on the processor slots (the epsilon gradient of the limiter and of the
    // corrected laplacian reads the cell across a processor face; ras_production's halo carried the old values)
    halo_fields(x, {"epsilon"});
  }
  if (x.wf.bits & Ctx::WF_EPS_INLET) {
    const double Cmu = x.opt("ras.Cmu"), Cmu75 = std::sqrt(std::sqrt(Cmu)) * std::sqrt(Cmu);
    LAUNCH(k_ras_inlet_ref, x.B, (long)x.B, (int)Ctx::WF_EPS_INLET, wall_tab(x), Cmu75, x.f("boundary_U"), x.f("boundary_k"),
           x.f("boundary_epsilon_ref"));
  }
}

// ---- flareFGM transport (include/dfmi.h, flareFGM block): baseFGM::transport(), the non-spray branch
namespace {
// D = (rho nut) / Sct + mu / Sc over n cells or n boundary slots (each slot from its own boundary values)
__global__ void k_fgm_diffusivity(long n, double Sct, double Sc, const double* __restrict__ rho, const double* __restrict__ nut,
                                  const double* __restrict__ mu, double* __restrict__ D) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  D[i] = (rho[i] * nut[i]) / Sct + mu[i] / Sc;
}
// the explicit source per unit volume of equation eq (0 Z, 1 Zvar, 2 c, 3 cvar, 4 Zcvar, 5 Ha), with a = ((2 mut) / Sct) (g1 . g2),
// g1 . g2 = (x x + y y) + z z of the Gauss gradients g1, g2 [3][n], mut = rho nut:
//   Zvar:  a(gZ, gZ) - (2 rho) chi_Z         cvar:   (a(gc, gc) - (2 rho) chi_c) + 2 (cOmega_c - omega_c c)
//   c:     omega_c                           Zcvar:  (a(gZ, gc) - (2 rho) chi_Zc) + (ZOmega_c - omega_c Z)          Z, Ha: 0
struct FgmSrc {
  const double *rho, *nut, *g1, *g2, *chi, *omc, *xOmc, *psi;
};
__global__ void k_fgm_source(long n, int eq, double Sct, FgmSrc s, double* __restrict__ Su) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (eq == 0 || eq == 5) { Su[i] = 0.0; return; }
  if (eq == 2) { Su[i] = s.omc[i]; return; }
  const double r = s.rho[i];
  const double dot = (s.g1[i] * s.g2[i] + s.g1[n + i] * s.g2[n + i]) + s.g1[2 * n + i] * s.g2[2 * n + i];
  const double a = ((2.0 * (r * s.nut[i])) / Sct) * dot;
  const double v = a - (2.0 * r) * s.chi[i];
  if (eq == 1) Su[i] = v;
  else if (eq == 3) Su[i] = v + 2.0 * (s.xOmc[i] - s.omc[i] * s.psi[i]);
  else Su[i] = v + (s.xOmc[i] - s.omc[i] * s.psi[i]);
}
// psi.min(hi); psi.max(lo) over n cells or slots
__global__ void k_fgm_clip(long n, double lo, double hi, double* __restrict__ psi) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = psi[i];
  v = v < hi ? v : hi;
  v = v > lo ? v : lo;
  psi[i] = v;
}
__global__ void k_fgm_ha(long n, double Hfu, double Hox, const double* __restrict__ Z, double* __restrict__ Ha) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  Ha[i] = Z[i] * (Hfu - Hox) + Hox;
}
}  // namespace

// the Gauss gradient of the flareFGM field nm into the buffer `buf` ([3][C]; its processor slots through the halo)
static double* fgm_grad(Ctx& x, const char* nm, const char* buf) {
  const MeshView m = x.view();
  const std::string bn = std::string("boundary_") + nm, bb = std::string("boundary_") + buf;
  double* g = scheme_buf(x, buf, x.C, 3);
  scheme_buf(x, bb.c_str(), x.B, 3);
  LAUNCH_GRAD(1, x.st(nm), x.f(nm), x.f(bn), g);
  halo_fields(x, {buf});
  return g;
}
void fgm_assemble(Ctx& x, int eq) {
  const char* nm = fgm_eq_name(eq);
  const std::string bn = std::string("boundary_") + nm;
  const MeshView m = x.view();
  Matrix& A = x.mK;
  const double Sct = x.opt("fgm.Sct"), Sc = x.opt("fgm.Sc");
  const int8_t* ty = x.st(nm);
  LAUNCH(k_fgm_diffusivity, x.C, (long)x.C, Sct, Sc, x.f("rho"), x.f("nut"), x.f("mu"), x.f("fgm_D"));
  LAUNCH(k_fgm_diffusivity, x.B, (long)x.B, Sct, Sc, x.f("boundary_rho"), x.f("boundary_nut"), x.f("boundary_mu"),
         x.f("boundary_fgm_D"));
  // the gradients of Z and c as they stand (inside correct(): just solved and clipped)
  FgmSrc s{x.f("rho"), x.f("nut"), nullptr, nullptr, nullptr, x.f("omega_c"), nullptr, nullptr};
  if (eq == 1) { s.g1 = s.g2 = fgm_grad(x, "Z", "fgm_gradZ"); s.chi = x.f("chi_Z"); }
  else if (eq == 3) { s.g1 = s.g2 = fgm_grad(x, "c", "fgm_gradc"); s.chi = x.f("chi_c"); s.xOmc = x.f("cOmega_c"); s.psi = x.f("c"); }
  else if (eq == 4) {
    s.g1 = fgm_grad(x, "Z", "fgm_gradZ"); s.g2 = fgm_grad(x, "c", "fgm_gradc");
    s.chi = x.f("chi_Zc"); s.xOmc = x.f("ZOmega_c"); s.psi = x.f("Z");
  }
  LAUNCH(k_fgm_source, x.C, (long)x.C, eq, Sct, s, x.f("fgm_Su"));
  const int kind = x.sch.fgm[eq];
  const bool lim = kind == SCH_LL || kind == SCH_LL01, corr = x.lap == LAP_CORRECTED;
  double *g = nullptr, *bg = nullptr;
  if (lim || corr) {   // the field's own Gauss gradient: the limiter's upwind-cell gradient and the corrected laplacian's
    if (lim) scheme_checks(x, true);
    g = fgm_grad(x, nm, "fgm_grad");
    bg = x.f("boundary_fgm_grad");
  }
  const double *w = nullptr, *bw = nullptr;
  if (lim) {
    double* wo = scheme_buf(x, "fgm_w", x.Fs, 1, true);
    double* bwo = scheme_buf(x, "boundary_fgm_w", x.B, 1);
    const double twoByk = 2.0 / std::max(x.sch.k_fgm[eq], 1e-15);
    const int b01 = kind == SCH_LL01 ? 1 : 0;
    if (face_hex(x)) LAUNCH(k_lim_w_cell, x.C, m, b01, twoByk, x.f("phi"), x.f(nm), g, wo);
    else LAUNCH(k_lim_w_face, x.Fs, m, b01, twoByk, x.f("phi"), x.f(nm), g, wo);
    LAUNCH(k_lim_w_slot, x.B, m, ty, b01, twoByk, x.f("boundary_phi"), x.f(nm), x.f(bn), g, bg, bwo);
    w = wo; bw = bwo;
  }
  LAUNCH_W(k_scalar_assemble, x.C, m, ty, x.f(nm), x.f(bn), x.f("rho"), x.f("rho_old"), x.f("phi"), x.f("boundary_phi"),
           x.f("fgm_D"), x.f("boundary_fgm_D"), x.f("fgm_Su"), x.f("fgm_Sp"), A.lower.p, A.upper.p, A.diag.p, A.source.p,
           A.ic.p, A.bc.p, mixbc(x, nm), w, bw);
  if (corr) {   // - fvm::laplacian(D, psi): the explicit non-orthogonal term
    NoArgs a = no_args(x);
    a.g = g; a.bg = bg;
    a.gam = x.f("fgm_D"); a.bgam = x.f("boundary_fgm_D");
    a.src = A.source.p;
    LAUNCH_NO(1, NO_SHARED, ty, a);
  }
}
// after the solve: the field's boundary values and halo (fvMatrix::solve's correctBoundaryConditions), then
// psi.min(upper); psi.max(lower) on cells and slots (pointwise: the processor slots' neighbour halves stay the
// neighbour cells' values)
void fgm_post_solve(Ctx& x, int eq) {
  const char* nm = fgm_eq_name(eq);
  const std::string bn = std::string("boundary_") + nm;
  k_bc_correct(x, nm, x.f(nm), x.f(bn), 1);
  halo_fields(x, {nm});
  static const double lo[FGM_NEQ] = {0.0, 0.0, 0.0, 0.0, -0.25, 0.0}, hi[FGM_NEQ] = {1.0, 0.25, 1.0, 0.25, 0.25, 0.0};
  if (eq == 5) return;   // Ha is not clipped
  LAUNCH(k_fgm_clip, x.C, (long)x.C, lo[eq], hi[eq], x.f(nm));
  LAUNCH(k_fgm_clip, x.B, (long)x.B, lo[eq], hi[eq], x.f(bn));
}
void fgm_ha_from_z(Ctx& x) {
  LAUNCH(k_fgm_ha, x.C, (long)x.C, x.fgm.Hfu, x.fgm.Hox, x.f("Z"), x.f("Ha"));
  LAUNCH(k_fgm_ha, x.B, (long)x.B, x.fgm.Hfu, x.fgm.Hox, x.f("boundary_Z"), x.f("boundary_Ha"));
}
#undef LAUNCH_GRAD
#undef LAUNCH_NO

void e_post_solve(Ctx& x) {
  k_bc_correct(x, "he", x.f("he"), x.f("boundary_he"), 1);
  halo_fields(x, {"he"});
}

// one df0DFoam time step (df0DFoam.C:99-113, constantProperty pressure): chemistry.solve(deltaT) on
// every cell (a closed isothermal reactor from setState_TPY, RR scaled by the thermo rho), YEqn
// (ddt(rho, Yi) == RR), EEqn (he held: constant pressure) -> correctThermo (T from he), rho = thermo.rho()
void zero_d_step(Ctx& x, double dt) {
  DFMI_CHECK(x.chem.mode == 1 || x.chem.mode == 2, "0D step: chemistry mode must be 1 (ODE) or 2 (DNN)");
  DFMI_HIP(hipMemcpyAsync(x.f("rho_old"), x.f("rho"), sizeof(double) * x.C, hipMemcpyDeviceToDevice, x.stream));
  if (x.chem.mode == 1) chem_solve(x, dt, "rho");
  else dnn_solve(x, "rho");
  LAUNCH(k_zero_d_species, x.C, x.C, x.S, x.inert, 1.0 / dt, x.V.p, x.f("rho_old"), x.f("rho"), x.f("RR"), x.f("Y"));
  k_bc_correct(x, "Y", x.f("Y"), x.f("boundary_Y"), x.S);
  thermo_correct(x, false);
  thermo_rho_from_psi(x);
}

// ---- measured HBM copy peak (diagnostic): streaming copies with 16-B vector loads/stores, U vectors per
// thread (all loads issued before the stores), one pass over the buffer; the best of U = 1, 2, 4, 8 is the
// measured peak (read + write bytes / time), the reference point for `roofline.achieved` beside 8 TB/s.
template <int U>
__global__ void __launch_bounds__(256) k_stream_copy(long n, const double2* __restrict__ a, double2* __restrict__ b) {
  const long base = (long)blockIdx.x * 256 * U + threadIdx.x;
  double2 v[U];
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const long i = base + (long)k * 256;
    if (i < n) v[k] = a[i];
  }
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const long i = base + (long)k * 256;
    if (i < n) b[i] = v[k];
  }
}

template <int U> double stream_copy_gbs(Ctx& x, long n, const double2* a, double2* b, int reps) {
  const dim3 g((unsigned)((n + 256L * U - 1) / (256L * U))), bl(256);
  hipLaunchKernelGGL(k_stream_copy<U>, g, bl, 0, x.stream, n, a, b);
  hipEvent_t e0, e1;
  DFMI_HIP(hipEventCreate(&e0)); DFMI_HIP(hipEventCreate(&e1));
  DFMI_HIP(hipEventRecord(e0, x.stream));
  for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_stream_copy<U>, g, bl, 0, x.stream, n, a, b);
  DFMI_HIP(hipEventRecord(e1, x.stream));
  DFMI_HIP(hipEventSynchronize(e1));
  float ms = 0.0f;
  DFMI_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return 2.0 * (double)n * sizeof(double2) * reps / (ms / 1e3) / 1e9;
}

double hbm_copy_gbs(Ctx& x, size_t bytes, int reps) {
  const long n = (long)(bytes / sizeof(double2));
  DevBuf<double2> a, b;
  a.alloc(n); b.alloc(n);
  DFMI_HIP(hipMemsetAsync(a.p, 0, n * sizeof(double2), x.stream));
  double best = 0.0;
  best = std::max(best, stream_copy_gbs<1>(x, n, a.p, b.p, reps));
  best = std::max(best, stream_copy_gbs<2>(x, n, a.p, b.p, reps));
  best = std::max(best, stream_copy_gbs<4>(x, n, a.p, b.p, reps));
  best = std::max(best, stream_copy_gbs<8>(x, n, a.p, b.p, reps));
  return best;
}

void thermo_rho_from_psi(Ctx& x) {   // dfThermo::updateRho (dfThermo.cu:673-679)
  if (x.thermo.eos || x.fgm.model) {   // rho = thermo.rho(): with an equation of state, or flareFGM, rho_thermo and not psi p
    DFMI_HIP(hipMemcpyAsync(x.f("rho"), x.f("rho_thermo"), sizeof(double) * x.C, hipMemcpyDeviceToDevice, x.stream));
    if (x.B > 0)
      DFMI_HIP(hipMemcpyAsync(x.f("boundary_rho"), x.f("boundary_rho_thermo"), sizeof(double) * x.B, hipMemcpyDeviceToDevice,
                              x.stream));
    return;
  }
  LAUNCH(k_mul, x.C, (long)x.C, x.f("p"), x.f("psi"), x.f("rho"));
  LAUNCH(k_mul, x.B, (long)x.B, x.f("boundary_p"), x.f("boundary_psi"), x.f("boundary_rho"));
}
void thermo_psip0(Ctx& x) {          // dfThermo::psip0 (:681-686)
  LAUNCH(k_mul, x.C, (long)x.C, x.f("psi"), x.f("p"), x.f("psip0"));
  LAUNCH(k_mul, x.B, (long)x.B, x.f("boundary_psi"), x.f("boundary_p"), x.f("boundary_psip0"));
}
void thermo_correct_psip_rho(Ctx& x) {   // dfThermo::correctPsipRho (:688-695)
  if (x.thermo.eos || x.fgm.model) {   // thermo.rho_ += psi p - psip0
    LAUNCH(k_add_psip, x.C, (long)x.C, x.f("p"), x.f("psi"), x.f("psip0"), x.f("rho_thermo"));
    LAUNCH(k_add_psip, x.B, (long)x.B, x.f("boundary_p"), x.f("boundary_psi"), x.f("boundary_psip0"), x.f("boundary_rho_thermo"));
    return;
  }
  LAUNCH(k_add_psip, x.C, (long)x.C, x.f("p"), x.f("psi"), x.f("psip0"), x.f("rho"));
  LAUNCH(k_add_psip, x.B, (long)x.B, x.f("boundary_p"), x.f("boundary_psi"), x.f("boundary_psip0"), x.f("boundary_rho"));
}

}  // namespace dfmi
