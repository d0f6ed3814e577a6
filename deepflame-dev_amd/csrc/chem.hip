// chem.hip -- per-cell stiff chemistry on MI355X.
//
// Semantics of the reference chemistry step (dfChemistryModel::solveSingle,
// src/dfChemistryModel/dfChemistryModel.C:737-780; GPU ABI precedent opencc_ode_all, YEqn.H:45-77):
// every cell is a closed constant-volume reactor at FIXED temperature and density integrated over
// the flow time step; the species source is RR_i = (Y_i(dt) - Y_i(0)) rho / dt. Kinetics follow
// Cantera GasKinetics: Arrhenius rates, three-body efficiencies, Lindemann/Troe fall-off, reverse
// rates from NASA7 equilibrium constants.
//
// Integrator: ROS3 Rosenbrock (L-stable, order 3, embedded order-2 error estimate, one Jacobian and
// one LU per step) with adaptive step size; alternative (option chem.method = 1): linearly-implicit
// Euler extrapolation with step sequence 1, 2, 3. Analytic Jacobian: mass action, third-body factors and
// the fall-off rate constants' [M]-dependence (without the latter the stiff 1D-flame cells needed 2-5x
// more steps: a Rosenbrock method loses order with an inexact Jacobian). Tolerances mirror the reference's CVODE settings (relTol 1e-6, absTol 1e-10 on
// mass fractions) by default.
//
// Scheduling: cells are launched in descending order of the integrator steps they needed in the
// previous solve (counting sort, k_bin_*): a wave costs its slowest lane, and on the reference TGV
// state natural order loads waves at 23% (mean / per-wave max); binned, k_chem drops 7.3 -> 1.9 ms.
//
// Layout: one cell per lane, 64-lane workgroups. Per-lane rate constants (they depend only on T,
// which is frozen) and the per-lane S x S iteration matrix live in LDS as [entry][lane]
// (bank-conflict free); state vectors live in registers (compile-time S). The mechanism arrays are
// wave-uniform (scalar loads). That layout holds 4..12 species; 13..64 species run the cooperative kernel below
// (k_chem_coop: several lanes per cell, the cell's matrix and rate constants in LDS once per cell).
#include "dfmi_ctx.h"
#include <cmath>
#include <cstdlib>

namespace dfmi {
namespace {

constexpr int LANES = 64;
constexpr double RU = 8314.46261815324;
constexpr double P_ATM = 101325.0;

struct ChemMech {
  int R, ndd;
  const int* idata;    // [R][8]: type, reversible, n_reac, n_prod, has_T2
  const int* irs;      // [R][6]: reactant ids (3), product ids (3), -1 padded
  const double* dd;    // [R][ndd]: A b Ta nu_r[3] nu_p[3] A0 b0 Ta0 troe[4] eff[S]
  const double* nasa;  // [S][15]
  const double* W;     // [S]
};

template <int S> struct Lane {
  double* kf;   // LDS [R][LANES]
  double* k0;
  double* ikc;  // 1/Kc, 0 for irreversible
  double* A;    // LDS [S*S][LANES]
  int lane;
  __device__ double& K(double* b, int r) const { return b[r * LANES + lane]; }
  __device__ double& M(int i, int j) const { return A[(i * S + j) * LANES + lane]; }
};

template <int S>
__device__ void rate_constants(const ChemMech& m, const Lane<S>& L, double T) {
  const double lnT = log(T), rT = 1.0 / T;
  double g[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {   // g_i / RT from NASA7
    const double* row = m.nasa + i * 15;
    const double* a = T > row[0] ? row + 1 : row + 8;
    const double h = a[0] + a[1] * T / 2 + a[2] * T * T / 3 + a[3] * T * T * T / 4 + a[4] * T * T * T * T / 5 + a[5] / T;
    const double s = a[0] * lnT + a[1] * T + a[2] * T * T / 2 + a[3] * T * T * T / 3 + a[4] * T * T * T * T / 4 + a[6];
    g[i] = h - s;
  }
  for (int r = 0; r < m.R; ++r) {
    const int* id = m.idata + r * 8;
    const int* ix = m.irs + r * 6;
    const double* d = m.dd + (long)r * m.ndd;
    L.K(L.kf, r) = d[0] * exp(d[1] * lnT - d[2] * rT);
    L.K(L.k0, r) = id[0] >= 2 ? d[9] * exp(d[10] * lnT - d[11] * rT) : 0.0;
    double ik = 0.0;
    if (id[1]) {
      double dG = 0.0, dnu = 0.0;
      for (int k = 0; k < 3; ++k) {
        const int ip = ix[3 + k], ir = ix[k];
#pragma unroll
        for (int i = 0; i < S; ++i) {   // wave-uniform species ids; unrolled select keeps g in registers
          if (ip == i) { dG += d[6 + k] * g[i]; }
          if (ir == i) { dG -= d[3 + k] * g[i]; }
        }
        if (ip >= 0) dnu += d[6 + k];
        if (ir >= 0) dnu -= d[3 + k];
      }
      // 1/Kc = exp(dG) (p_atm / RT)^-dnu
      ik = exp(dG - dnu * log(P_ATM / (RU * T)));
    }
    L.K(L.ikc, r) = ik;
  }
}

template <int S> __device__ __forceinline__ double sel(const double (&v)[S], int i) {
  double o = 0.0;
#pragma unroll
  for (int k = 0; k < S; ++k) o = (k == i) ? v[k] : o;
  return o;
}
template <int S> __device__ __forceinline__ void add_at(double (&v)[S], int i, double a) {
#pragma unroll
  for (int k = 0; k < S; ++k) if (k == i) v[k] += a;
}

// effective rate coefficient and the third-body factor of reaction r
template <int S>
__device__ __forceinline__ void rcoef(const ChemMech& m, const Lane<S>& L, int r, double T, const double (&C)[S],
                                      double& k, double& Mf, double& Mc) {
  const int* id = m.idata + r * 8;
  const double* d = m.dd + (long)r * m.ndd;
  k = L.K(L.kf, r);
  Mf = 1.0;
  Mc = 0.0;
  if (id[0] == 0) return;
  double M = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) M += d[17 + i] * C[i];
  if (id[0] == 1) { Mf = M; Mc = 1.0; return; }
  const double Pr = L.K(L.k0, r) * M / k;
  double F = 1.0;
  if (id[0] == 3) {
    const double a = d[12], T3 = d[13], T1 = d[14], T2 = d[15];
    const double Fc = (1 - a) * exp(-T / T3) + a * exp(-T / T1) + (id[4] ? exp(-T2 / T) : 0.0);
    const double lFc = log10(fmax(Fc, 1e-300));
    const double c = -0.4 - 0.67 * lFc, n = 0.75 - 1.27 * lFc;
    const double lPr = log10(fmax(Pr, 1e-300));
    const double f1 = (lPr + c) / (n - 0.14 * (lPr + c));
    F = exp10(lFc / (1 + f1 * f1));
  }
  k = k * Pr / (1 + Pr) * F;
}

// d fo / d[M] of a fall-off reaction (k = k_inf fo, fo = Pr / (1 + Pr) F): the [M]-dependence of the rate
// constant, which Rosenbrock methods need in the Jacobian for their order (chem_codegen.py derives the
// same expression for the generated kernels)
template <int S>
__device__ __forceinline__ double falloff_dfo(const ChemMech& m, const Lane<S>& L, int r, double T, const double (&C)[S]) {
  const int* id = m.idata + r * 8;
  const double* d = m.dd + (long)r * m.ndd;
  double M = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) M += d[17 + i] * C[i];
  const double kinf = L.K(L.kf, r), k0 = L.K(L.k0, r);
  const double Pr = k0 * M / kinf;
  double F = 1.0, corr = 0.0;
  if (id[0] == 3) {
    const double a = d[12], T3 = d[13], T1 = d[14], T2 = d[15];
    const double Fc = (1 - a) * exp(-T / T3) + a * exp(-T / T1) + (id[4] ? exp(-T2 / T) : 0.0);
    const double lFc = log10(fmax(Fc, 1e-300));
    const double c = -0.4 - 0.67 * lFc, n = 0.75 - 1.27 * lFc;
    const double lPr = log10(fmax(Pr, 1e-300));
    const double u = n - 0.14 * (lPr + c);
    const double f1 = (lPr + c) / u;
    F = exp10(lFc / (1 + f1 * f1));
    corr = F * 2.0 * lFc * f1 * n / ((1.0 + Pr) * (1.0 + f1 * f1) * (1.0 + f1 * f1) * u * u);
  }
  return k0 / kinf * (F / ((1.0 + Pr) * (1.0 + Pr)) - corr);
}

__device__ __forceinline__ double ipow(double c, double nu) {
  return nu == 1.0 ? c : (nu == 2.0 ? c * c : (nu == 3.0 ? c * c * c : pow(c, nu)));
}
__device__ __forceinline__ double dipow(double c, double nu) {   // d/dc c^nu
  return nu == 1.0 ? 1.0 : (nu == 2.0 ? 2.0 * c : (nu == 3.0 ? 3.0 * c * c : nu * pow(c, nu - 1.0)));
}

// w = dC/dt
template <int S>
__device__ void rhs(const ChemMech& m, const Lane<S>& L, double T, const double (&C)[S], double (&w)[S]) {
#pragma unroll
  for (int i = 0; i < S; ++i) w[i] = 0.0;
  for (int r = 0; r < m.R; ++r) {
    const int* id = m.idata + r * 8;
    const int* ix = m.irs + r * 6;
    const double* d = m.dd + (long)r * m.ndd;
    double k, Mf, Mc;
    rcoef<S>(m, L, r, T, C, k, Mf, Mc);
    double f = k, b = id[1] ? k * L.K(L.ikc, r) : 0.0;
    for (int j = 0; j < 3; ++j) {
      if (ix[j] >= 0) f *= ipow(sel<S>(C, ix[j]), d[3 + j]);
      if (ix[3 + j] >= 0) b *= ipow(sel<S>(C, ix[3 + j]), d[6 + j]);
    }
    const double q = Mf * (f - b);
    for (int j = 0; j < 3; ++j) {
      if (ix[j] >= 0) add_at<S>(w, ix[j], -d[3 + j] * q);
      if (ix[3 + j] >= 0) add_at<S>(w, ix[3 + j], d[6 + j] * q);
    }
  }
}

// A = I - h J  (J = d(dC/dt)/dC, mass-action part + third-body factor)
template <int S>
__device__ void build_matrix(const ChemMech& m, const Lane<S>& L, double T, const double (&C)[S], double h) {
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < S; ++j) L.M(i, j) = (i == j) ? 1.0 : 0.0;
  for (int r = 0; r < m.R; ++r) {
    const int* id = m.idata + r * 8;
    const int* ix = m.irs + r * 6;
    const double* d = m.dd + (long)r * m.ndd;
    double k, Mf, Mc;
    rcoef<S>(m, L, r, T, C, k, Mf, Mc);
    const double kb = id[1] ? k * L.K(L.ikc, r) : 0.0;
    double cr[3], cp[3];
    for (int j = 0; j < 3; ++j) {
      cr[j] = ix[j] >= 0 ? sel<S>(C, ix[j]) : 1.0;
      cp[j] = ix[3 + j] >= 0 ? sel<S>(C, ix[3 + j]) : 1.0;
    }
    // dq/dC for each participating species (3 reactant slots, 3 product slots)
    double dq[6];
    int sp[6];
    for (int a = 0; a < 3; ++a) {
      double t = k;
      for (int j = 0; j < 3; ++j) if (ix[j] >= 0) t *= (j == a) ? dipow(cr[j], d[3 + j]) : ipow(cr[j], d[3 + j]);
      dq[a] = ix[a] >= 0 ? Mf * t : 0.0;
      sp[a] = ix[a];
      double u = kb;
      for (int j = 0; j < 3; ++j) if (ix[3 + j] >= 0) u *= (j == a) ? dipow(cp[j], d[6 + j]) : ipow(cp[j], d[6 + j]);
      dq[3 + a] = ix[3 + a] >= 0 ? -Mf * u : 0.0;
      sp[3 + a] = ix[3 + a];
    }
    double q0 = 0.0;
    if (Mc != 0.0) {
      double f = k, b = kb;
      for (int j = 0; j < 3; ++j) {
        if (ix[j] >= 0) f *= ipow(cr[j], d[3 + j]);
        if (ix[3 + j] >= 0) b *= ipow(cp[j], d[6 + j]);
      }
      q0 = f - b;
    }
    double qf = 0.0;   // fall-off: (d fo / d[M]) (k_inf prod_f - k_inf / Kc prod_b)
    if (id[0] >= 2) {
      const double kinf = L.K(L.kf, r);
      double f = kinf, b = id[1] ? kinf * L.K(L.ikc, r) : 0.0;
      for (int j = 0; j < 3; ++j) {
        if (ix[j] >= 0) f *= ipow(cr[j], d[3 + j]);
        if (ix[3 + j] >= 0) b *= ipow(cp[j], d[6 + j]);
      }
      qf = falloff_dfo<S>(m, L, r, T, C) * (f - b);
    }
    // rows touched: reactants (-nu_r) and products (+nu_p)
    for (int a = 0; a < 6; ++a) {
      const int row = ix[a];   // reactant slots 0..2, product slots 3..5
      if (row < 0) continue;
      const double nu = a < 3 ? -d[3 + a] : d[6 + (a - 3)];
      for (int bb = 0; bb < 6; ++bb)
        if (sp[bb] >= 0 && dq[bb] != 0.0) L.M(row, sp[bb]) -= h * nu * dq[bb];
      if (Mc != 0.0)
#pragma unroll
        for (int j = 0; j < S; ++j) L.M(row, j) -= h * nu * d[17 + j] * q0;
      if (qf != 0.0)
#pragma unroll
        for (int j = 0; j < S; ++j) L.M(row, j) -= h * nu * d[17 + j] * qf;
    }
  }
}

// in-place LU without pivoting (A = I - hJ is an M-matrix-like perturbation of I); false if singular
template <int S> __device__ bool lu(const Lane<S>& L) {
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const double p = L.M(k, k);
    if (!(fabs(p) > 1e-300)) return false;
    const double ip = 1.0 / p;
#pragma unroll
    for (int i = k + 1; i < S; ++i) {
      const double f = L.M(i, k) * ip;
      L.M(i, k) = f;
#pragma unroll
      for (int j = k + 1; j < S; ++j) L.M(i, j) -= f * L.M(k, j);
    }
  }
  return true;
}
template <int S> __device__ void lu_solve(const Lane<S>& L, double (&b)[S]) {
#pragma unroll
  for (int i = 1; i < S; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) b[i] -= L.M(i, j) * b[j];
#pragma unroll
  for (int i = S - 1; i >= 0; --i) {
#pragma unroll
    for (int j = i + 1; j < S; ++j) b[i] -= L.M(i, j) * b[j];
    b[i] = b[i] / L.M(i, i);
  }
}

// n_sub linearly-implicit Euler substeps of size h/n_sub from y0 (f0 = rhs(y0) given)
template <int S>
__device__ bool lie(const ChemMech& m, const Lane<S>& L, double T, const double (&y0)[S], const double (&f0)[S],
                    double h, int n_sub, double (&out)[S]) {
  const double hs = h / n_sub;
  build_matrix<S>(m, L, T, y0, hs);
  if (!lu<S>(L)) return false;
  double y[S], f[S];
#pragma unroll
  for (int i = 0; i < S; ++i) { y[i] = y0[i]; f[i] = f0[i]; }
  for (int s = 0; s < n_sub; ++s) {
    if (s > 0) rhs<S>(m, L, T, y, f);
    double dlt[S];
#pragma unroll
    for (int i = 0; i < S; ++i) dlt[i] = hs * f[i];
    lu_solve<S>(L, dlt);
#pragma unroll
    for (int i = 0; i < S; ++i) y[i] += dlt[i];
  }
#pragma unroll
  for (int i = 0; i < S; ++i) out[i] = y[i];
  return true;
}

// One ROS3 step (Sandu et al. 1997, L-stable, order 3 with embedded order 2; the coefficients
// of KPP's Rosenbrock ROS-3): (I - h g J) K_i = h g [f(y + sum a_ij K_j) + sum (c_ij / h) K_j];
// y_new = y + sum m_i K_i, error = sum e_i K_i. One Jacobian and one LU per step; stage 3 reuses
// f of stage 2 (a31 = a21 = 1, a32 = 0).
template <int S>
__device__ bool ros3(const ChemMech& m, const Lane<S>& L, double T, const double (&y)[S], const double (&f0)[S],
                     double h, double (&ynew)[S], double (&err)[S]) {
  constexpr double g = 0.43586652150845899941601945119356;
  constexpr double c21 = -0.10156171083877702091975600115545e1, c31 = 0.40759956452537699824805835358067e1,
                   c32 = 0.92076794298330791242156818474003e1;
  constexpr double m1 = 1.0, m2 = 0.61697947043828245592553615689730e1, m3 = -0.42772256543218573326238373806514;
  constexpr double e1 = 0.5, e2 = -0.29079558716805469821718236208017e1, e3 = 0.22354069897811569627360909276199;
  const double hg = h * g;
  build_matrix<S>(m, L, T, y, hg);
  if (!lu<S>(L)) return false;
  double k1[S], k2[S], k3[S], y2[S], f2[S];
#pragma unroll
  for (int i = 0; i < S; ++i) k1[i] = hg * f0[i];
  lu_solve<S>(L, k1);
#pragma unroll
  for (int i = 0; i < S; ++i) y2[i] = y[i] + k1[i];
  rhs<S>(m, L, T, y2, f2);
  const double rh = 1.0 / h;
#pragma unroll
  for (int i = 0; i < S; ++i) k2[i] = hg * (f2[i] + c21 * rh * k1[i]);
  lu_solve<S>(L, k2);
#pragma unroll
  for (int i = 0; i < S; ++i) k3[i] = hg * (f2[i] + rh * (c31 * k1[i] + c32 * k2[i]));
  lu_solve<S>(L, k3);
#pragma unroll
  for (int i = 0; i < S; ++i) {
    ynew[i] = y[i] + m1 * k1[i] + m2 * k2[i] + m3 * k3[i];
    err[i] = e1 * k1[i] + e2 * k2[i] + e3 * k3[i];
  }
  return true;
}

// ---- cost binning: a wave runs as long as its slowest lane, so cells are handed to the integrator
// ordered by the integrator steps (accepted + rejected) they took in the previous solve, most
// expensive first. The unit is a group of GRP consecutive cells (costed by its most expensive cell). GRP = 1:
// single cells. Measured (round 5, 2M headline): single-cell binning scatters a bucket's cells over the mesh (PMC
// traffic 1.8 GB per solve, 4.4x the state's 0.42 GB) but keeps every wave's lanes at the same cost (wave
// efficiency 1.0): 1.05 ms; groups of 8 (whole 64-B lines per wave: 0.6 GB, 1.44x) lose that (efficiency 0.61):
// 1.25 ms -- the kernel is bound by its FP64 issue, not by these bytes. Counting sort over NBIN buckets, stable
// inside a bucket (ascending group index). Every cell's integration is independent of its position, so the
// order changes timing only, never results. Default: the sort inside 4096-cell tiles (chem.binning = 2, below):
// traffic 2.06 -> 0.72 GB per solve at wave efficiency 0.977, k_chem 1.029 -> 1.046 ms and the binning
// passes 0.074 -> 0.056 ms (no global scan): the same 1.10 ms per step (profiles/r05_pmc_traffic*.json).
constexpr int NBIN = 32, BCB = 256, BCELLS = 4096, GRP = 1;   // 4096 groups per binning block, 16 passes of 256
__device__ inline int cost_bin(double st, double rj) {
  const int c = (int)(st + rj);
  return NBIN - 1 - (c < 0 ? NBIN - 1 : (c > NBIN - 1 ? NBIN - 1 : c));   // bucket 0 = most expensive
}
// bucket of group g: its most expensive cell (steps + rejects; a failed cell, steps < 0, is most expensive)
__device__ inline int group_bin(long n, const double* __restrict__ stats, long g) {
  int b = NBIN - 1;
  for (long c = g * GRP; c < n && c < (g + 1) * GRP; ++c) b = min(b, cost_bin(stats[c], stats[n + c]));
  return b;
}
// the cell lane t integrates: group perm[t / GRP], its (t % GRP)-th cell (>= n: no cell)
__device__ inline long bin_cell(const int* perm, long t) { return perm ? (long)perm[t / GRP] * GRP + t % GRP : t; }
// chem.binning = 2 (tile-local): the counting sort runs inside each tile of BCELLS groups (one binning block) rather
// than over the whole mesh, so a wave's cells come from one tile; the 64-wave tile runs on one XCD (one L2) and every
// line of the state it reads is fetched once for the tile instead of once per cost bucket. XCD x's k-th workgroup
// (hardware order: workgroup p on XCD p % 8) takes block k % TILE_B of tile (k / TILE_B) * 8 + x -- consecutive tiles
// on different XCDs, so a costly region of the mesh spreads over all eight. The grid is padded to 8 tiles.
constexpr int TILE_B = BCELLS * GRP / LANES;
__device__ inline long chem_thread(int tiled) {
  long b = blockIdx.x;
  if (tiled) { const long x = b % 8, k = b / 8; b = ((k / TILE_B) * 8 + x) * TILE_B + k % TILE_B; }
  return b * LANES + threadIdx.x;
}
// per-block bucket counts, bucket-major [NBIN][nb]
__global__ void __launch_bounds__(BCB) k_bin_count(long n, const double* __restrict__ stats, int nb, int* __restrict__ cnt) {
  const long ng = (n + GRP - 1) / GRP;
  __shared__ int h[NBIN];
  if (threadIdx.x < NBIN) h[threadIdx.x] = 0;
  __syncthreads();
  for (int i = 0; i < BCELLS / BCB; ++i) {
    const long g = (long)blockIdx.x * BCELLS + i * BCB + threadIdx.x;
    if (g < ng) atomicAdd(&h[group_bin(n, stats, g)], 1);
  }
  __syncthreads();
  if (threadIdx.x < NBIN) cnt[(long)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}
// exclusive scan of the bucket-major counts in place (one workgroup, contiguous chunk per thread)
__global__ void __launch_bounds__(1024) k_bin_scan(int total, int* __restrict__ cnt) {
  __shared__ int part[1024];
  const int per = (total + 1023) / 1024, b0 = threadIdx.x * per, b1 = min(b0 + per, total);
  int a = 0;
  for (int i = b0; i < b1; ++i) a += cnt[i];
  part[threadIdx.x] = a;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {   // Hillis-Steele inclusive scan of the 1024 partials
    const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  a = part[threadIdx.x] - a;
  for (int i = b0; i < b1; ++i) { const int v = cnt[i]; cnt[i] = a; a += v; }
}
// chem.binning = 2: exclusive offsets inside each binning block's own range of perm (bucket order, block by block)
__global__ void __launch_bounds__(BCB) k_bin_scan_local(int nb, int* __restrict__ cnt) {
  const int blk = blockIdx.x * blockDim.x + threadIdx.x;
  if (blk >= nb) return;
  int a = blk * BCELLS;
  for (int b = 0; b < NBIN; ++b) { const int v = cnt[(long)b * nb + blk]; cnt[(long)b * nb + blk] = a; a += v; }
}
__global__ void __launch_bounds__(BCB) k_bin_scatter(long n, const double* __restrict__ stats, int nb,
                                                     const int* __restrict__ off, int* __restrict__ perm) {
  const long ng = (n + GRP - 1) / GRP;
  __shared__ int wc[BCB / 64][NBIN];
  __shared__ int base[NBIN];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x < NBIN) base[threadIdx.x] = off[(long)threadIdx.x * nb + blockIdx.x];
  for (int i = 0; i < BCELLS / BCB; ++i) {
    const long g = (long)blockIdx.x * BCELLS + i * BCB + threadIdx.x;
    const int k = g < ng ? group_bin(n, stats, g) : -1;
    int rank = 0;
    for (int b = 0; b < NBIN; ++b) {
      const unsigned long long m = __ballot(k == b);
      if (k == b) rank = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wc[w][b] = __popcll(m);
    }
    __syncthreads();
    if (k >= 0) {
      int pos = base[k] + rank;
      for (int v = 0; v < w; ++v) pos += wc[v][k];
      perm[pos] = (int)g;
    }
    __syncthreads();
    if (threadIdx.x < NBIN) {
      int a = 0;
      for (int v = 0; v < BCB / 64; ++v) a += wc[v][threadIdx.x];
      base[threadIdx.x] += a;
    }
  }
}

// Cantera's setState_TPY(T, p, Y) (dfChemistryModel.C:755): mass fractions clipped at 0 and
// normalised (Phase::setMassFractions), density = p * meanW / (R T); returns that density and the
// reactor's initial concentrations C_i = rho Y_i / W_i. The reactor then runs at this density (closed,
// constant volume), while RR is scaled by the thermo density the caller passes (problem.rhoi =
// rho_[celli], :771 and :807).
template <int S, class WT>
__device__ __forceinline__ double reactor_state(double T, double p, const double (&Y0)[S], const WT& W, double (&C)[S]) {
  double ys = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) ys += fmax(Y0[i], 0.0);
  const double iys = 1.0 / ys;
  double sw = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) sw += fmax(Y0[i], 0.0) * iys / W[i];
  const double rho = p / (sw * RU * T);
#pragma unroll
  for (int i = 0; i < S; ++i) C[i] = rho * (fmax(Y0[i], 0.0) * iys) / W[i];
  return rho;
}

// The integration interval of cell c: the launch's one value, or the cell's own (EDC's chemistryPtr_->solve(tauStar),
// EDC.C:170: the kernels instantiated with DT = const double*). A per-cell interval that is not positive and finite
// integrates nothing and gives RR = 0; the scalar instantiations fold both helpers away and compile as they always did
// (profiles/tci_resource_usage.md).
__device__ __forceinline__ double cell_dt(double dt, long) { return dt; }
__device__ __forceinline__ __attribute__((unused)) double cell_dt(const double* dt, long c) { return dt[c]; }
__device__ __forceinline__ constexpr bool dt_live(double, double) { return true; }
__device__ __forceinline__ __attribute__((unused)) bool dt_live(const double*, double dt) { return dt > 0.0 && dt <= 1.79769313486231570e308; }

template <int S, class DT = double>
__global__ void __launch_bounds__(LANES) k_chem(long n, const int* __restrict__ perm, ChemMech m,
                                                const double* __restrict__ Tf, const double* __restrict__ pf,
                                                const double* __restrict__ rhof, const double* __restrict__ Yf,
                                                DT dt_in, double rtol, double atol, double Tmin, int max_steps,
                                                int method, double* __restrict__ RR, double* __restrict__ stats,
                                                int* __restrict__ fail, int tiled, const double* __restrict__ hc,
                                                double* __restrict__ Qdot) {
  extern __shared__ double lds[];
  Lane<S> L;
  L.lane = threadIdx.x;
  L.kf = lds;
  L.k0 = lds + (long)m.R * LANES;
  L.ikc = lds + 2L * m.R * LANES;
  L.A = lds + 3L * m.R * LANES;
  const long t = chem_thread(tiled);
  if (t >= (perm ? (n + GRP - 1) / GRP * GRP : n)) return;   // no block-level synchronisation below
  const long c = bin_cell(perm, t);
  if (c >= n) return;
  const double T = Tf[c], rho_rr = rhof[c];
  const double dt = cell_dt(dt_in, c);
  double Y0[S], y[S];
#pragma unroll
  for (int i = 0; i < S; ++i) Y0[i] = Yf[(long)i * n + c];
  const double rho = reactor_state<S>(T, pf[c], Y0, m.W, y);
  int steps = 0, rejects = 0;
  double hnext = 0.0;   // the step the integration would take next
  if (T >= Tmin && dt_live(dt_in, dt)) {
    rate_constants<S>(m, L, T);
    double sc[S];
#pragma unroll
    for (int i = 0; i < S; ++i) sc[i] = rho / m.W[i];   // Y -> C scale for the tolerances
    // first step: the size the previous solve of this cell ended with (OpenFOAM's per-cell deltaTChem)
    const double hp = stats[2 * n + c];
    double t = 0.0, h = hp > 0.0 ? fmin(dt, hp) : dt;
    while (t < dt) {
      if (steps + rejects >= max_steps) { steps = -1; break; }
      if (t + h > dt) h = dt - t;
      double f0[S], r1[S], r2[S], t21[S], t22[S];
      rhs<S>(m, L, T, y, f0);
      bool ok;
      double err = 0.0;
      if (method == 0) {   // ROS3
        ok = ros3<S>(m, L, T, y, f0, h, r2, r1);
        if (ok) {   // weighted RMS error norm (KPP / CVODE)
#pragma unroll
          for (int i = 0; i < S; ++i) {
            const double e = r1[i] / (atol * sc[i] + rtol * fmax(fabs(y[i]), fabs(r2[i])));
            err += e * e;
          }
          err = sqrt(err / S);
          if (!(err == err)) ok = false;
        }
      } else {             // linearly-implicit Euler extrapolation, sequence 1, 2, 3
        ok = lie<S>(m, L, T, y, f0, h, 1, r1);
        ok = ok && lie<S>(m, L, T, y, f0, h, 2, t21);
        if (ok) {
#pragma unroll
          for (int i = 0; i < S; ++i) t22[i] = 2.0 * t21[i] - r1[i];
          ok = lie<S>(m, L, T, y, f0, h, 3, r2);
        }
        if (ok) {
#pragma unroll
          for (int i = 0; i < S; ++i) {
            const double t32 = 3.0 * r2[i] - 2.0 * t21[i];
            const double t33 = t32 + (t32 - t22[i]) * 0.5;
            const double e = fabs(t33 - t32) / (atol * sc[i] + rtol * fabs(t33));
            err = fmax(err, e);
            r2[i] = t33;
          }
          if (!(err == err)) ok = false;   // NaN
        }
      }
      if (ok && err <= 1.0) {
#pragma unroll
        for (int i = 0; i < S; ++i) y[i] = r2[i];
        t += h;
        ++steps;
        const double fac = err > 0.0 ? 0.9 * pow(err, -1.0 / 3.0) : 5.0;
        h = h * fmin(5.0, fmax(0.2, fac));
      } else {
        ++rejects;
        const double fac = ok ? 0.9 * pow(err, -1.0 / 3.0) : 0.25;
        h = h * fmin(0.5, fmax(0.1, fac));
      }
    }
    if (steps >= 0) hnext = h;
  }
  double q = 0.0;   // Qdot = -sum_i hc_i RR_i in species order (dfChemistryModel.C:771)
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const double Yn = y[i] * m.W[i] / rho;
    const double rr = T >= Tmin && dt_live(dt_in, dt) ? (Yn - Y0[i]) * rho_rr / dt : 0.0;
    RR[(long)i * n + c] = rr;
    q -= hc[i] * rr;
  }
  Qdot[c] = q;
  stats[c] = steps;
  stats[n + c] = rejects;
  if (hnext > 0.0) stats[2 * n + c] = hnext;
  if (steps < 0) atomicAdd(fail, 1);
}

// ---- generated fast path: the mechanism compiled in (dfmi/chem_codegen.py), state in registers
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-variable"
#define DFMI_HD __device__   // the generated kinetics are plain C++; here they run on the device
// between the reactions of the fused rates + Jacobian pass: nothing is scheduled across, so one reaction's
// temporaries die before the next one's loads are issued (the register peak is J plus one reaction)
// (the scheduler left free across reactions measured 13.90 -> 14.11 ms per step, 3 rounds each in one call, round 6)
#define DFMI_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// 1 / x for the generated kinetics (fall-off factors, LU pivots): the hardware reciprocal estimate refined by two
// Newton steps instead of the ~10-instruction IEEE division sequence (x is a nonzero normal number there)
__device__ __forceinline__ double dfmi_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0);
  r = fma(r, e, r);
  e = fma(-x, r, 1.0);
  return fma(r, e, r);
}
#define DFMI_RCP(x) dfmi_rcp(x)
// products contracted into FMAs inside the generated kinetics (the library builds with -ffp-contract=off for the
// bitwise FV kernels; the chemistry is checked against SciPy BDF to a tolerance, not bitwise)
#define DFMI_CONTRACT() _Pragma("clang fp contract(fast)") do {} while (0)
#include "chem_gen_burke9.inc"
#include "chem_gen_es80.inc"
#pragma clang diagnostic pop

// The integrated state is the mechanism's active species (G::SA; a third-body-only species such as N2 keeps its
// concentration and rides along in y) -- bitwise the full-state integration: the dropped rows and columns
// only ever multiply or add exact zeros (chem_codegen.py).
// Registers: the dense iteration matrix (SA^2 doubles, 128 VGPRs for Burke 9), the state and the stage vectors
// fill the wave's registers, so the NK rate constants -- computed once per cell (T is frozen), read by every
// rate and Jacobian evaluation of the step loop -- live in LDS as [constant][lane] (conflict-free ds_read_b64,
// 24.6 KiB per 64-lane workgroup for Burke 9) instead of 96 more VGPRs that spilled to scratch (round 4:
// 256 VGPR + 256 AGPR + 84 B/lane of scratch at one wave per SIMD).
struct KLds {
  double* base;   // the workgroup's constants, [constant][lane]
  int lane;       // constant i of this lane at base[i * LANES + lane]
  __device__ __forceinline__ double& operator[](int i) const { return base[i * LANES + lane]; }
};

template <class G, class DT = double>
__global__ void __launch_bounds__(LANES, 1) k_chem_gen(long n, const int* __restrict__ perm,
    const double* __restrict__ Tf, const double* __restrict__ pf, const double* __restrict__ rhof,
    const double* __restrict__ Yf, DT dt_in, double rtol, double atol, double Tmin, int max_steps,
    double* __restrict__ RR, double* __restrict__ stats, int* __restrict__ fail, int tiled, const double* __restrict__ hc,
    double* __restrict__ Qdot) {
  constexpr int S = G::S, SA = G::SA;
  constexpr double g = 0.43586652150845899941601945119356;
  constexpr double c21 = -0.10156171083877702091975600115545e1, c31 = 0.40759956452537699824805835358067e1,
                   c32 = 0.92076794298330791242156818474003e1;
  constexpr double m2 = 0.61697947043828245592553615689730e1, m3 = -0.42772256543218573326238373806514;
  constexpr double e1 = 0.5, e2 = -0.29079558716805469821718236208017e1, e3 = 0.22354069897811569627360909276199;
  __shared__ double kl[G::NK * LANES];
  KLds kh{kl, (int)threadIdx.x};
  const long t = chem_thread(tiled);
  if (t >= (perm ? (n + GRP - 1) / GRP * GRP : n)) return;   // no block-level synchronisation below
  const long c = bin_cell(perm, t);
  if (c >= n) return;
  const double T = Tf[c];
  const double dt = cell_dt(dt_in, c);
  double y[S];
  double rho;
  {
    double Y0[S];
#pragma unroll
    for (int i = 0; i < S; ++i) Y0[i] = Yf[(long)i * n + c];
    rho = reactor_state<S>(T, pf[c], Y0, G::W, y);
  }
  int steps = 0, rejects = 0;
  double hnext = 0.0;   // the step the integration would take next
  if (T >= Tmin && dt_live(dt_in, dt)) {
    G::consts(T, kh);
    // first step: the size the previous solve of this cell ended with (OpenFOAM's per-cell deltaTChem)
    const double hp = stats[2 * n + c];
    double t = 0.0, h = hp > 0.0 ? fmin(dt, hp) : dt;
    while (t < dt) {
      // the lane offset passes through an empty asm each iteration: the constants' LDS reads cannot be hoisted
      // out of the loop (held in registers across it, which is what this layout exists to avoid)
      asm volatile("" : "+v"(kh.lane));
      double arho = atol * rho;   // tolerance scale atol rho / W_i, formed per use (not 8 values held across the loop)
      asm volatile("" : "+v"(arho));
      if (steps + rejects >= max_steps) { steps = -1; break; }
      if (t + h > dt) h = dt - t;
      const double hg = h * g, rh = dfmi_rcp(h);
      double f0[SA], A[SA * SA];
#pragma unroll
      for (int e = 0; e < SA * SA; ++e) A[e] = 0.0;
      G::wdot_jac(T, kh, y, f0, A);
#pragma unroll
      for (int e = 0; e < SA * SA; ++e) A[e] = (e % (SA + 1) == 0 ? 1.0 : 0.0) - hg * A[e];
      bool ok = G::factor(A);
      double err = 0.0, yn[SA];
      if (ok) {
        double k1[SA], k2[SA], k3[SA], y2[S], f2[SA];
#pragma unroll
        for (int a = 0; a < SA; ++a) k1[a] = hg * f0[a];
        G::solve(A, k1);
#pragma unroll
        for (int i = 0; i < S; ++i) y2[i] = y[i];
#pragma unroll
        for (int a = 0; a < SA; ++a) y2[G::ACT[a]] = y[G::ACT[a]] + k1[a];
        G::wdot(T, kh, y2, f2);
#pragma unroll
        for (int a = 0; a < SA; ++a) k2[a] = hg * (f2[a] + c21 * rh * k1[a]);
        G::solve(A, k2);
#pragma unroll
        for (int a = 0; a < SA; ++a) k3[a] = hg * (f2[a] + rh * (c31 * k1[a] + c32 * k2[a]));
        G::solve(A, k3);
#pragma unroll
        for (int a = 0; a < SA; ++a) {
          const int i = G::ACT[a];
          yn[a] = y[i] + k1[a] + m2 * k2[a] + m3 * k3[a];
          const double e = (e1 * k1[a] + e2 * k2[a] + e3 * k3[a]) * dfmi_rcp(arho * G::RW[i] + rtol * fmax(fabs(y[i]), fabs(yn[a])));
          err += e * e;   // weighted RMS error norm (KPP / CVODE) over all S species (inactive terms are 0)
        }
        err = sqrt(err / S);
        if (!(err == err)) ok = false;
      }
      if (ok && err <= 1.0) {
#pragma unroll
        for (int a = 0; a < SA; ++a) y[G::ACT[a]] = yn[a];
        t += h;
        ++steps;
        const double fac = err > 0.0 ? 0.9 * pow(err, -1.0 / 3.0) : 5.0;
        h = h * fmin(5.0, fmax(0.2, fac));
      } else {
        ++rejects;
        const double fac = ok ? 0.9 * pow(err, -1.0 / 3.0) : 0.25;
        h = h * fmin(0.5, fmax(0.1, fac));
      }
    }
    if (steps >= 0) hnext = h;
  }
  const double rho_rr = rhof[c];   // Y0 and rho_rr re-read here rather than held through the integration
  double q = 0.0;   // Qdot = -sum_i hc_i RR_i in species order (dfChemistryModel.C:771)
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const double Yn = y[i] * G::W[i] / rho;
    const double rr = T >= Tmin && dt_live(dt_in, dt) ? (Yn - Yf[(long)i * n + c]) * rho_rr / dt : 0.0;
    RR[(long)i * n + c] = rr;
    q -= hc[i] * rr;
  }
  Qdot[c] = q;
  stats[c] = steps;
  stats[n + c] = rejects;
  if (hnext > 0.0) stats[2 * n + c] = hnext;
  if (steps < 0) atomicAdd(fail, 1);
}

// ---- cooperative kernel: 13..64 species (and any S >= 4 under chem.coop = 1)
// The layout above keeps (3R + S^2) doubles per LANE in LDS: 355 KB per workgroup for DRM19 (21 / 84), 1 MB for
// the 36-species gri30. Here TG lanes (16, 32 or 64; one cell never leaves its wave) integrate one cell, and the
// cell's iteration matrix, rate constants and per-reaction rates live in LDS once per CELL:
//   A [S][LD]  LD = S | 1: the lanes of a cell own rows, and a column walk (LU multipliers, the triangular solves)
//              reads A[i][j] at stride LD doubles; ds_read_b64 banks are (byte / 4) % 64 per 32-lane half, so an odd
//              LD puts 32 rows on 32 distinct bank pairs. The pivot row A[k][j] is one address: a broadcast.
//   kf k0 ikc [R]  frozen with T;  ke Mf tb q [R]  per evaluation (effective rate constant, third-body factor, the
//              [M]-derivative term of third-body / fall-off reactions, rate of progress);  C bv [S]  concentrations
//              and the broadcast / reduction vector.
// Lane l of a cell owns species rows l, l + TG, ... (RPL = 64 / TG of them at most, in registers) and reactions
// l, l + TG, ... of the per-reaction pass. Every sum runs in a fixed order inside one lane -- production rates and
// Jacobian rows over the species' reaction list (chem_upload builds it in k_chem's order: reaction, then slot),
// norms and Qdot over the species index -- so there is no floating-point atomic, and a cell's bits depend on
// neither its neighbours in the workgroup nor on where it was launched. A cell lives in one wave, so the kernel has
// no workgroup barrier: cells that finish early, sit below Tmin or lie past the mesh just leave. Lanes of a cell
// exchange data through LDS in program order (one wave executes its LDS instructions in order); cell_sync() keeps
// the compiler from moving LDS accesses across the hand-over points.
struct CoopList {
  const int* off;      // [S + 1]
  const int* ent;      // reaction * 8 + slot (0..2 reactant, 3..5 product), ordered by (reaction, slot)
  const double* nu;    // signed stoichiometric coefficient (-nu_r, +nu_p)
  // the same entries as self-contained records for the Jacobian rows, so that a row's walk is one stream of loads
  // whose addresses do not depend on loaded values: rec_i [E][8] = reaction, its 6 species ids, reversible;
  // rec_d [E][8] = signed coefficient, nu_r[3], nu_p[3], 0
  const int* rec_i;
  const double* rec_d;
};
struct CoopRec {
  int r, ix[6], rev;
  double nu, nr[3], np[3];
};
__device__ __forceinline__ CoopRec coop_rec(const CoopList& cl, int e) {
  const int4* pi = reinterpret_cast<const int4*>(cl.rec_i + (long)e * 8);
  const int4 a = pi[0], b = pi[1];
  const double* pd = cl.rec_d + (long)e * 8;
  CoopRec c;
  c.r = a.x; c.ix[0] = a.y; c.ix[1] = a.z; c.ix[2] = a.w; c.ix[3] = b.x; c.ix[4] = b.y; c.ix[5] = b.z; c.rev = b.w;
  c.nu = pd[0];
  for (int j = 0; j < 3; ++j) { c.nr[j] = pd[1 + j]; c.np[j] = pd[4 + j]; }
  return c;
}

__device__ __forceinline__ void cell_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// doubles of LDS one cell takes
inline size_t coop_cell_doubles(int S, int R) { return (size_t)S * (S | 1) + 7 * (size_t)R + 2 * (size_t)S; }

template <int TG> struct Coop {
  static constexpr int RPL = LANES / TG;   // rows a lane can own (S <= 64)
  int S, R, LD, l;
  double *A, *kf, *k0, *ikc, *ke, *Mf, *tb, *q, *C, *bv;
  __device__ __forceinline__ int row(int s) const { return l + s * TG; }

  // kf, k0, 1 / Kc of every reaction at the cell's (frozen) temperature
  __device__ __forceinline__ void rate_constants(const ChemMech& m, double T) const {
    const double lnT = log(T), rT = 1.0 / T;
    cell_sync();
    for (int i = l; i < S; i += TG) {   // g_i / RT from NASA7
      const double* row = m.nasa + i * 15;
      const double* a = T > row[0] ? row + 1 : row + 8;
      const double h = a[0] + a[1] * T / 2 + a[2] * T * T / 3 + a[3] * T * T * T / 4 + a[4] * T * T * T * T / 5 + a[5] / T;
      const double s = a[0] * lnT + a[1] * T + a[2] * T * T / 2 + a[3] * T * T * T / 3 + a[4] * T * T * T * T / 4 + a[6];
      bv[i] = h - s;
    }
    cell_sync();
    for (int r = l; r < R; r += TG) {
      const int* id = m.idata + r * 8;
      const int* ix = m.irs + r * 6;
      const double* d = m.dd + (long)r * m.ndd;
      kf[r] = d[0] * exp(d[1] * lnT - d[2] * rT);
      k0[r] = id[0] >= 2 ? d[9] * exp(d[10] * lnT - d[11] * rT) : 0.0;
      double ik = 0.0;
      if (id[1]) {
        double dG = 0.0, dnu = 0.0;
        for (int k = 0; k < 3; ++k) {
          const int ip = ix[3 + k], ir = ix[k];
          if (ip >= 0) { dG += d[6 + k] * bv[ip]; dnu += d[6 + k]; }
          if (ir >= 0) { dG -= d[3 + k] * bv[ir]; dnu -= d[3 + k]; }
        }
        ik = exp(dG - dnu * log(P_ATM / (RU * T)));
      }
      ikc[r] = ik;
    }
    cell_sync();
  }

  // per-reaction pass at the concentrations in C: q; with jac also ke, Mf and tb (what the Jacobian rows need)
  __device__ __forceinline__ void reactions(const ChemMech& m, double T, bool jac) const {
    cell_sync();
    for (int r = l; r < R; r += TG) {
      const int* id = m.idata + r * 8;
      const int* ix = m.irs + r * 6;
      const double* d = m.dd + (long)r * m.ndd;
      const int type = id[0];
      const double kinf = kf[r];
      double k = kinf, mf = 1.0, M = 0.0, F = 1.0, Pr = 0.0, corr = 0.0;
      if (type != 0) {
        for (int i = 0; i < S; ++i) M += d[17 + i] * C[i];
        if (type == 1) mf = M;
        else {
          Pr = k0[r] * M / kinf;
          if (type == 3) {
            const double a = d[12], T3 = d[13], T1 = d[14], T2 = d[15];
            const double Fc = (1 - a) * exp(-T / T3) + a * exp(-T / T1) + (id[4] ? exp(-T2 / T) : 0.0);
            const double lFc = log10(fmax(Fc, 1e-300));
            const double c = -0.4 - 0.67 * lFc, n = 0.75 - 1.27 * lFc;
            const double lPr = log10(fmax(Pr, 1e-300));
            const double u = n - 0.14 * (lPr + c);
            const double f1 = (lPr + c) / u;
            F = exp10(lFc / (1 + f1 * f1));
            corr = F * 2.0 * lFc * f1 * n / ((1.0 + Pr) * (1.0 + f1 * f1) * (1.0 + f1 * f1) * u * u);
          }
          k = kinf * Pr / (1 + Pr) * F;
        }
      }
      const double ik = id[1] ? ikc[r] : 0.0;
      // forward / backward rates with the effective constant (f, b) and with k_inf (fi, bi: the fall-off derivative)
      double f = k, b = id[1] ? k * ik : 0.0, fi = kinf, bi = id[1] ? kinf * ik : 0.0;
      for (int j = 0; j < 3; ++j) {
        if (ix[j] >= 0) { const double v = ipow(C[ix[j]], d[3 + j]); f *= v; fi *= v; }
        if (ix[3 + j] >= 0) { const double v = ipow(C[ix[3 + j]], d[6 + j]); b *= v; bi *= v; }
      }
      q[r] = mf * (f - b);
      if (jac) {
        ke[r] = k;
        Mf[r] = mf;
        double t = 0.0;
        if (type == 1) t = f - b;
        else if (type >= 2) t = k0[r] / kinf * (F / ((1.0 + Pr) * (1.0 + Pr)) - corr) * (fi - bi);
        tb[r] = t;
      }
    }
    cell_sync();
  }

  // k_tci_rates: the forward and reverse rates of progress at the concentrations in C -- the f and b that reactions()
  // differences, times the third-body factor -- weighted as PaSR.C:341-371 sums them: wf = sum_products nu_p fwd into ke,
  // wr = sum_reactants nu_r rev into Mf
  __device__ __forceinline__ void progress(const ChemMech& m, double T) const {
    cell_sync();
    for (int r = l; r < R; r += TG) {
      const int* id = m.idata + r * 8;
      const int* ix = m.irs + r * 6;
      const double* d = m.dd + (long)r * m.ndd;
      const int type = id[0];
      const double kinf = kf[r];
      double k = kinf, mf = 1.0, M = 0.0, F = 1.0, Pr = 0.0;
      if (type != 0) {
        for (int i = 0; i < S; ++i) M += d[17 + i] * C[i];
        if (type == 1) mf = M;
        else {
          Pr = k0[r] * M / kinf;
          if (type == 3) {
            const double a = d[12], T3 = d[13], T1 = d[14], T2 = d[15];
            const double Fc = (1 - a) * exp(-T / T3) + a * exp(-T / T1) + (id[4] ? exp(-T2 / T) : 0.0);
            const double lFc = log10(fmax(Fc, 1e-300));
            const double c = -0.4 - 0.67 * lFc, n = 0.75 - 1.27 * lFc;
            const double lPr = log10(fmax(Pr, 1e-300));
            const double u = n - 0.14 * (lPr + c);
            const double f1 = (lPr + c) / u;
            F = exp10(lFc / (1 + f1 * f1));
          }
          k = kinf * Pr / (1 + Pr) * F;
        }
      }
      double f = k, b = id[1] ? k * ikc[r] : 0.0;
      for (int j = 0; j < 3; ++j) {
        if (ix[j] >= 0) f *= ipow(C[ix[j]], d[3 + j]);
        if (ix[3 + j] >= 0) b *= ipow(C[ix[3 + j]], d[6 + j]);
      }
      const double fwd = mf * f, rev = mf * b;
      double wf = 0.0, wr = 0.0;
      for (int j = 0; j < 3; ++j) {
        if (ix[3 + j] >= 0) wf += d[6 + j] * fwd;
        if (ix[j] >= 0) wr += d[3 + j] * rev;
      }
      ke[r] = wf;
      Mf[r] = wr;
    }
    cell_sync();
  }

  // dC_i/dt of the rows this lane owns, from q
  __device__ __forceinline__ void production(const CoopList& cl, double (&w)[RPL]) const {
#pragma unroll
    for (int s = 0; s < RPL; ++s) {
      w[s] = 0.0;
      const int i = row(s);
      if (i < S)
        for (int e = cl.off[i]; e < cl.off[i + 1]; ++e) w[s] += cl.nu[e] * q[cl.ent[e] >> 3];
    }
  }

  // rows of A = I - h J this lane owns (J = d(dC/dt)/dC: mass action, third-body factors, fall-off [M] dependence)
  __device__ __forceinline__ void build_rows(const ChemMech& m, const CoopList& cl, double h) const {
#pragma unroll
    for (int s = 0; s < RPL; ++s) {
      const int i = row(s);
      if (i >= S) continue;
      double* Ai = A + i * LD;
      for (int j = 0; j < S; ++j) Ai[j] = (i == j) ? 1.0 : 0.0;
      const int e0 = cl.off[i], e1 = cl.off[i + 1];
      CoopRec nx = coop_rec(cl, e0);   // the lists are padded by one record
      for (int e = e0; e < e1; ++e) {
        const CoopRec c = nx;
        nx = coop_rec(cl, e + 1);      // the next record's loads fly while this one is worked on
        const int r = c.r;
        const double nu = c.nu;
        const int* ix = c.ix;
        const double k = ke[r], mf = Mf[r];
        const double kb = c.rev ? k * ikc[r] : 0.0;
        double cr[3], cp[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          cr[j] = ix[j] >= 0 ? C[ix[j]] : 1.0;
          cp[j] = ix[3 + j] >= 0 ? C[ix[3 + j]] : 1.0;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          if (ix[a] >= 0) {
            double t = k;
#pragma unroll
            for (int j = 0; j < 3; ++j) if (ix[j] >= 0) t *= (j == a) ? dipow(cr[j], c.nr[j]) : ipow(cr[j], c.nr[j]);
            const double dq = mf * t;
            if (dq != 0.0) Ai[ix[a]] -= h * nu * dq;
          }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          if (ix[3 + a] >= 0) {
            double u = kb;
#pragma unroll
            for (int j = 0; j < 3; ++j) if (ix[3 + j] >= 0) u *= (j == a) ? dipow(cp[j], c.np[j]) : ipow(cp[j], c.np[j]);
            const double dq = -mf * u;
            if (dq != 0.0) Ai[ix[3 + a]] -= h * nu * dq;
          }
        }
        const double* d = m.dd + (long)r * m.ndd;
        const double t = tb[r];
        if (t != 0.0) {
          const double* ef = d + 17;
          int j = 0;
          for (; j + 4 <= S; j += 4) {   // loads first, as in lu()
            const double a0 = Ai[j], a1 = Ai[j + 1], a2 = Ai[j + 2], a3 = Ai[j + 3];
            const double f0 = ef[j], f1 = ef[j + 1], f2 = ef[j + 2], f3 = ef[j + 3];
            Ai[j] = a0 - h * nu * f0 * t; Ai[j + 1] = a1 - h * nu * f1 * t;
            Ai[j + 2] = a2 - h * nu * f2 * t; Ai[j + 3] = a3 - h * nu * f3 * t;
          }
          for (; j < S; ++j) Ai[j] -= h * nu * ef[j] * t;
        }
      }
    }
    cell_sync();
  }

  // in-place LU without pivoting, by row ownership; false if singular (the same for every lane of the cell)
  __device__ __forceinline__ bool lu() const {
    for (int k = 0; k < S; ++k) {
      cell_sync();   // row k is final: its owner last touched it in step k - 1
      const double* Ak = A + k * LD;
      const double p = Ak[k];
      if (!(fabs(p) > 1e-300)) return false;
      const double ip = 1.0 / p;
#pragma unroll
      for (int s = 0; s < RPL; ++s) {
        const int i = row(s);
        if (i > k && i < S) {
          double* Ai = A + i * LD;
          const double f = Ai[k] * ip;
          Ai[k] = f;
          int j = k + 1;
          for (; j + 4 <= S; j += 4) {   // four columns per round: the LDS reads are issued before the first write
            const double a0 = Ai[j], a1 = Ai[j + 1], a2 = Ai[j + 2], a3 = Ai[j + 3];
            const double p0 = Ak[j], p1 = Ak[j + 1], p2 = Ak[j + 2], p3 = Ak[j + 3];
            Ai[j] = a0 - f * p0; Ai[j + 1] = a1 - f * p1; Ai[j + 2] = a2 - f * p2; Ai[j + 3] = a3 - f * p3;
          }
          for (; j < S; ++j) Ai[j] -= f * Ak[j];
        }
      }
    }
    cell_sync();
    return true;
  }

  // L U x = b, column by column: the owner of row j publishes its finished entry, every later (earlier) row takes it
  __device__ __forceinline__ void solve(double (&b)[RPL]) const {
    for (int j = 0; j < S; ++j) {
      cell_sync();
#pragma unroll
      for (int s = 0; s < RPL; ++s) if (row(s) == j) bv[j] = b[s];
      cell_sync();
      const double bj = bv[j];
#pragma unroll
      for (int s = 0; s < RPL; ++s) {
        const int i = row(s);
        if (i > j && i < S) b[s] -= A[i * LD + j] * bj;
      }
    }
    for (int j = S - 1; j >= 0; --j) {
      cell_sync();
#pragma unroll
      for (int s = 0; s < RPL; ++s) if (row(s) == j) { b[s] = b[s] / A[j * LD + j]; bv[j] = b[s]; }
      cell_sync();
      const double bj = bv[j];
#pragma unroll
      for (int s = 0; s < RPL; ++s) {
        const int i = row(s);
        if (i < j) b[s] -= A[i * LD + j] * bj;
      }
    }
  }

  // sum over the species index, in order, of the values the row owners hold (every lane gets the same bits)
  __device__ __forceinline__ double ordered_sum(const double (&v)[RPL]) const {
    cell_sync();
#pragma unroll
    for (int s = 0; s < RPL; ++s) if (row(s) < S) bv[row(s)] = v[s];
    cell_sync();
    double a = 0.0;
    for (int i = 0; i < S; ++i) a += bv[i];
    return a;
  }

  __device__ __forceinline__ void publish(const double (&v)[RPL]) const {   // C = v
    cell_sync();
#pragma unroll
    for (int s = 0; s < RPL; ++s) if (row(s) < S) C[row(s)] = v[s];
  }
};

// the cell slot (position in launch order) of this lane's cell: chem_thread's tile interleave for workgroups of
// NCB cells -- XCD x's k-th workgroup takes block k % TBC of tile (k / TBC) * 8 + x, TBC = blocks per tile
template <int TG, int NCB> __device__ inline long coop_slot(int tiled) {
  constexpr int TBC = BCELLS * GRP / NCB;
  long b = blockIdx.x;
  if (tiled) { const long x = b % 8, k = b / 8; b = ((k / TBC) * 8 + x) * TBC + k % TBC; }
  return b * NCB + threadIdx.x / TG;
}

template <int TG, int NCB, class DT = double>
__global__ void __launch_bounds__(TG * NCB) k_chem_coop(long n, const int* __restrict__ perm, ChemMech m, CoopList cl, int S,
    const double* __restrict__ Tf, const double* __restrict__ pf, const double* __restrict__ rhof,
    const double* __restrict__ Yf, DT dt_in, double rtol, double atol, double Tmin, int max_steps,
    double* __restrict__ RR, double* __restrict__ stats, int* __restrict__ fail, int tiled, const double* __restrict__ hc,
    double* __restrict__ Qdot) {
  static_assert(LANES % TG == 0 && (TG * NCB) % LANES == 0, "a cell must not straddle waves");
  constexpr int RPL = Coop<TG>::RPL;
  constexpr double g = 0.43586652150845899941601945119356;
  constexpr double c21 = -0.10156171083877702091975600115545e1, c31 = 0.40759956452537699824805835358067e1,
                   c32 = 0.92076794298330791242156818474003e1;
  constexpr double m1 = 1.0, m2 = 0.61697947043828245592553615689730e1, m3 = -0.42772256543218573326238373806514;
  constexpr double e1 = 0.5, e2 = -0.29079558716805469821718236208017e1, e3 = 0.22354069897811569627360909276199;
  extern __shared__ double lds[];
  const int R = m.R;
  Coop<TG> L;
  L.S = S; L.R = R; L.LD = S | 1; L.l = threadIdx.x % TG;
  {
    double* base = lds + (size_t)(threadIdx.x / TG) * ((size_t)S * L.LD + 7 * (size_t)R + 2 * (size_t)S);
    L.A = base; base += S * L.LD;
    L.kf = base; L.k0 = base + R; L.ikc = base + 2 * R; L.ke = base + 3 * R; L.Mf = base + 4 * R; L.tb = base + 5 * R;
    L.q = base + 6 * R; base += 7 * R;
    L.C = base; L.bv = base + S;
  }
  const long t = coop_slot<TG, NCB>(tiled);
  if (t >= (perm ? (n + GRP - 1) / GRP * GRP : n)) return;   // no workgroup barrier below: a cell is inside one wave
  const long c = bin_cell(perm, t);
  if (c >= n) return;
  const double T = Tf[c];
  const double dt = cell_dt(dt_in, c);
  double y[RPL], Wl[RPL];
  double rho;
  {   // reactor_state (setState_TPY), sums in species order
    double a[RPL];
#pragma unroll
    for (int s = 0; s < RPL; ++s) {
      const int i = L.row(s);
      a[s] = i < S ? fmax(Yf[(long)i * n + c], 0.0) : 0.0;
      Wl[s] = i < S ? m.W[i] : 1.0;
    }
    const double iys = 1.0 / L.ordered_sum(a);
    double b[RPL];
#pragma unroll
    for (int s = 0; s < RPL; ++s) b[s] = a[s] * iys / Wl[s];
    const double sw = L.ordered_sum(b);
    rho = pf[c] / (sw * RU * T);
#pragma unroll
    for (int s = 0; s < RPL; ++s) y[s] = rho * (a[s] * iys) / Wl[s];
  }
  int steps = 0, rejects = 0;
  double hnext = 0.0;   // the step the integration would take next
  if (T >= Tmin && dt_live(dt_in, dt)) {
    L.rate_constants(m, T);
    // first step: the size the previous solve of this cell ended with (OpenFOAM's per-cell deltaTChem)
    const double hp = stats[2 * n + c];
    double tt = 0.0, h = hp > 0.0 ? fmin(dt, hp) : dt;
    while (tt < dt) {
      if (steps + rejects >= max_steps) { steps = -1; break; }
      if (tt + h > dt) h = dt - tt;
      const double hg = h * g, rh = 1.0 / h;
      double f0[RPL], k1[RPL], k2[RPL], k3[RPL], v[RPL];
      L.publish(y);
      L.reactions(m, T, true);
      L.production(cl, f0);
      L.build_rows(m, cl, hg);
      bool ok = L.lu();
      double err = 0.0;
      if (ok) {   // ROS3 (the stages of ros3 above)
#pragma unroll
        for (int s = 0; s < RPL; ++s) k1[s] = hg * f0[s];
        L.solve(k1);
#pragma unroll
        for (int s = 0; s < RPL; ++s) v[s] = y[s] + k1[s];
        L.publish(v);
        L.reactions(m, T, false);
        L.production(cl, f0);   // f of stage 2 (stage 3 reuses it)
#pragma unroll
        for (int s = 0; s < RPL; ++s) k2[s] = hg * (f0[s] + c21 * rh * k1[s]);
        L.solve(k2);
#pragma unroll
        for (int s = 0; s < RPL; ++s) k3[s] = hg * (f0[s] + rh * (c31 * k1[s] + c32 * k2[s]));
        L.solve(k3);
        double e2s[RPL];
#pragma unroll
        for (int s = 0; s < RPL; ++s) {
          v[s] = y[s] + m1 * k1[s] + m2 * k2[s] + m3 * k3[s];
          const double er = e1 * k1[s] + e2 * k2[s] + e3 * k3[s];
          const double e = er / (atol * (rho / Wl[s]) + rtol * fmax(fabs(y[s]), fabs(v[s])));   // weighted RMS norm
          e2s[s] = L.row(s) < S ? e * e : 0.0;
        }
        err = sqrt(L.ordered_sum(e2s) / S);
        if (!(err == err)) ok = false;
      }
      if (ok && err <= 1.0) {
#pragma unroll
        for (int s = 0; s < RPL; ++s) y[s] = v[s];
        tt += h;
        ++steps;
        const double fac = err > 0.0 ? 0.9 * pow(err, -1.0 / 3.0) : 5.0;
        h = h * fmin(5.0, fmax(0.2, fac));
      } else {
        ++rejects;
        const double fac = ok ? 0.9 * pow(err, -1.0 / 3.0) : 0.25;
        h = h * fmin(0.5, fmax(0.1, fac));
      }
    }
    if (steps >= 0) hnext = h;
  }
  const double rho_rr = rhof[c];
  double qh[RPL];
#pragma unroll
  for (int s = 0; s < RPL; ++s) {
    const int i = L.row(s);
    qh[s] = 0.0;
    if (i < S) {
      const double Yn = y[s] * Wl[s] / rho;
      const double rr = T >= Tmin && dt_live(dt_in, dt) ? (Yn - Yf[(long)i * n + c]) * rho_rr / dt : 0.0;
      RR[(long)i * n + c] = rr;
      qh[s] = hc[i] * rr;
    }
  }
  // Qdot = -sum_i hc_i RR_i in species order (dfChemistryModel.C:771): q -= hc_i rr_i from 0 is -(ordered sum)
  const double qs = L.ordered_sum(qh);
  if (L.l == 0) {
    Qdot[c] = -qs;
    stats[c] = steps;
    stats[n + c] = rejects;
    if (hnext > 0.0) stats[2 * n + c] = hnext;
    if (steps < 0) atomicAdd(fail, 1);   // integer count, one lane per cell
  }
}

// FNV-1a over the packed mechanism, NASA7 rows and molecular weights (dfmi/chem_codegen.py:fingerprint)
unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
  return h;
}

}  // namespace

#ifndef DFMI_CHEM_CELLS
void chem_upload(Ctx& x, int R, const int* idata, const int* irs, const double* dd) {
  Chem& h = x.chem;
  DFMI_CHECK(x.S > 0 && R > 0 && R <= 256, "chemistry: bad reaction count");
  h.R = R;
  h.ndd = 17 + x.S;
  h.h_idata.assign(idata, idata + (size_t)R * 8);
  h.h_irs.assign(irs, irs + (size_t)R * 6);
  h.h_dd.assign(dd, dd + (size_t)R * (17 + x.S));
  h.idata.upload(idata, (size_t)R * 8, x.stream);
  h.irs.upload(irs, (size_t)R * 6, x.stream);
  h.dd.upload(dd, (size_t)R * h.ndd, x.stream);
  for (int r = 0; r < R; ++r) {
    for (int k = 0; k < 6; ++k) DFMI_CHECK(irs[r * 6 + k] < x.S, "chemistry: species index out of range");
    DFMI_CHECK(idata[r * 8] >= 0 && idata[r * 8] <= 3, "chemistry: unknown reaction type");
  }
  // the cooperative kernel's per-species reaction lists, in k_chem's accumulation order (reaction, then slot:
  // reactants 0..2, products 3..5), with the signed stoichiometric coefficient
  std::vector<int> off(x.S + 1, 0), ent;
  std::vector<double> nu;
  for (int i = 0; i < x.S; ++i) {
    for (int r = 0; r < R; ++r)
      for (int a = 0; a < 6; ++a)
        if (irs[r * 6 + a] == i) {
          ent.push_back(r * 8 + a);
          const double* d = dd + (size_t)r * h.ndd;
          nu.push_back(a < 3 ? -d[3 + a] : d[6 + (a - 3)]);
        }
    off[i + 1] = (int)ent.size();
  }
  std::vector<int> rec_i((ent.size() + 1) * 8, -1);       // one padding record: the row walk reads one ahead
  std::vector<double> rec_d((ent.size() + 1) * 8, 0.0);
  for (size_t e = 0; e < ent.size(); ++e) {
    const int r = ent[e] >> 3;
    const double* d = dd + (size_t)r * h.ndd;
    rec_i[e * 8] = r;
    for (int a = 0; a < 6; ++a) rec_i[e * 8 + 1 + a] = irs[r * 6 + a];
    rec_i[e * 8 + 7] = idata[r * 8 + 1];
    rec_d[e * 8] = nu[e];
    for (int j = 0; j < 6; ++j) rec_d[e * 8 + 1 + j] = d[3 + j];
  }
  rec_i[ent.size() * 8] = 0;   // the padding record is loaded, never used; keep its reaction index valid
  if (ent.empty()) { ent.push_back(0); nu.push_back(0.0); }
  h.sp_off.upload(off.data(), off.size(), x.stream);
  h.sp_ent.upload(ent.data(), ent.size(), x.stream);
  h.sp_nu.upload(nu.data(), nu.size(), x.stream);
  h.sp_rec_i.upload(rec_i.data(), rec_i.size(), x.stream);
  h.sp_rec_d.upload(rec_d.data(), rec_d.size(), x.stream);
  DFMI_HIP(hipStreamSynchronize(x.stream));
  h.ready = true;
}

#endif
namespace {
// lanes per cell of the cooperative kernel by species count (profiles/chem_coop.json)
int coop_lanes_for(int S) { return S <= 16 ? 16 : (S <= 32 ? 32 : 64); }
}  // namespace

namespace {
template <class DT> void chem_solve_t(Ctx& x, DT dt, const char* rho_field) {
  Chem& h = x.chem;
  DFMI_CHECK(h.ready, "chemistry mechanism not set (dfmi_chem_set_mechanism)");
  DFMI_CHECK(x.thermo.S == x.S, "chemistry needs the thermo coefficients (NASA7, W)");
  ChemMech m{h.R, h.ndd, h.idata.p, h.irs.p, h.dd.p, x.thermo.dnasa.p, x.thermo.dW.p};
  DFMI_CHECK(x.S >= 4 && x.S <= 64, "chemistry: species count " + std::to_string(x.S) + " outside 4..64");
  const bool coop = x.S > 12 || x.on("chem.coop");
  const size_t lds = ((size_t)3 * h.R + (size_t)x.S * x.S) * LANES * sizeof(double);
  DFMI_CHECK(coop || lds <= 160 * 1024, "chemistry: mechanism too large for the LDS layout");
  double* stats = x.f("chem_stats");
  const double* rho_rr = x.f(rho_field);
  if (h.fail.n == 0) h.fail.alloc(1);
  if (!h.batch) DFMI_HIP(hipMemsetAsync(h.fail.p, 0, sizeof(int), x.stream));
  h.method = (int)x.opt("chem.method");
  h.bin = (int)x.opt("chem.binning");
  const long ng = (x.C + GRP - 1) / GRP;   // binning groups
  const int tiled = h.bin == 2;
  DFMI_CHECK(!(coop && h.method == 1), "chemistry: extrapolation is not available above 12 species (chem.method = 1 "
                                       "with the cooperative kernel; use chem.method = 0)");
  long nblk = blocks_for(h.bin ? ng * GRP : (long)x.C, LANES);
  if (tiled) nblk = (nblk + 8L * TILE_B - 1) / (8L * TILE_B) * (8L * TILE_B);   // whole groups of 8 tiles
  const dim3 g((unsigned)nblk);
  // compiled-in mechanism? (bitwise the same arrays, NASA7 and weights)
  unsigned long long fp = 0xcbf29ce484222325ull;
  const int S32 = x.S;
  fp = fnv(fp, &S32, 4);
  fp = fnv(fp, h.h_idata.data(), h.h_idata.size() * 4);
  fp = fnv(fp, h.h_irs.data(), h.h_irs.size() * 4);
  fp = fnv(fp, h.h_dd.data(), h.h_dd.size() * 8);
  fp = fnv(fp, x.thermo.nasa.data(), x.thermo.nasa.size() * 8);
  fp = fnv(fp, x.thermo.W.data(), x.thermo.W.size() * 8);
  h.generated = 0;
  if (!coop && x.on("chem.generated") && h.method == 0) {
    if (fp == ChemGen_burke9::FINGERPRINT) h.generated = 1;
    else if (fp == ChemGen_es80::FINGERPRINT) h.generated = 2;
  }
  const int* perm = nullptr;
  if (h.bin) {
    KScope _ks(x, "k_bin");
    const int nb = blocks_for(ng, BCELLS);
    if (h.perm.n < (size_t)ng) h.perm.alloc(ng);
    if (h.bcnt.n < (size_t)nb * NBIN) h.bcnt.alloc((size_t)nb * NBIN);
    hipLaunchKernelGGL(k_bin_count, dim3(nb), dim3(BCB), 0, x.stream, (long)x.C, (const double*)stats, nb, h.bcnt.p);
    if (tiled) hipLaunchKernelGGL(k_bin_scan_local, dim3(blocks_for(nb, BCB)), dim3(BCB), 0, x.stream, nb, h.bcnt.p);
    else hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(1024), 0, x.stream, nb * NBIN, h.bcnt.p);
    hipLaunchKernelGGL(k_bin_scatter, dim3(nb), dim3(BCB), 0, x.stream, (long)x.C, (const double*)stats, nb,
                       (const int*)h.bcnt.p, h.perm.p);
    perm = h.perm.p;
  }
  if (coop) {
    int tg = (int)x.opt("chem.coop_lanes");
    DFMI_CHECK(tg == 0 || tg == 16 || tg == 32 || tg == 64, "chem.coop_lanes must be 0 (by species count), 16, 32 or 64");
    const size_t cell = coop_cell_doubles(x.S, h.R) * sizeof(double);
    // by species count: with R <= 256 that asks for at most 67 KB (S = 16, 4 cells) and 47 KB (S = 32, 2 cells; S = 64)
    if (tg == 0) tg = coop_lanes_for(x.S);
    const int ncb = LANES / tg;   // one wave per workgroup
    const size_t clds = cell * ncb;
    DFMI_CHECK(clds <= 160 * 1024, "chemistry: " + std::to_string(x.S) + " species / " + std::to_string(h.R) +
                                       " reactions need " + std::to_string(clds) + " B of LDS per workgroup at " +
                                       std::to_string(tg) + " lanes per cell (160 KiB available)");
    const long slots = h.bin ? ng * GRP : (long)x.C;
    long cb = blocks_for(slots, ncb);
    const long tbc = (long)BCELLS * GRP / ncb;
    if (tiled) cb = (cb + 8 * tbc - 1) / (8 * tbc) * (8 * tbc);   // whole groups of 8 tiles
    DFMI_CHECK(cb < (1L << 31), "chemistry: too many cells for one launch");
    CoopList cl{h.sp_off.p, h.sp_ent.p, h.sp_nu.p, h.sp_rec_i.p, h.sp_rec_d.p};
    KScope _ks(x, "k_chem");
#define COOP(TG, NCB)                                                                                               \
  do {                                                                                                              \
    DFMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chem_coop<TG, NCB, DT>),                             \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)clds));                           \
    hipLaunchKernelGGL((k_chem_coop<TG, NCB, DT>), dim3((unsigned)cb), dim3(TG * NCB), clds, x.stream, (long)x.C, perm, m, \
                       cl, x.S, x.f("T"), x.f("p"), rho_rr, x.f("Y"), dt, h.rtol, h.atol, h.Tmin, h.max_steps,     \
                       x.f("RR"), stats, h.fail.p, tiled, x.thermo.dhc.p, x.f("Qdot"));                            \
  } while (0)
    if (tg == 16) COOP(16, 4); else if (tg == 32) COOP(32, 2); else COOP(64, 1);
#undef COOP
    DFMI_HIP(hipGetLastError());
    h.generated = -1;
    chem_fail_snapshot(x);
    return;
  }
  if (h.generated) {
    KScope _ks(x, "k_chem");
#define GEN(G) hipLaunchKernelGGL((k_chem_gen<G, DT>), g, dim3(LANES), 0, x.stream, (long)x.C, perm, x.f("T"), x.f("p"),  \
                                  rho_rr, x.f("Y"), dt, h.rtol, h.atol, h.Tmin, h.max_steps, x.f("RR"), stats, h.fail.p, tiled,   \
                                  x.thermo.dhc.p, x.f("Qdot"))
    if (h.generated == 1) GEN(ChemGen_burke9); else GEN(ChemGen_es80);
#undef GEN
    DFMI_HIP(hipGetLastError());
    chem_fail_snapshot(x);
    return;
  }
#define CALL(NS)                                                                                                    \
  do {                                                                                                              \
    KScope _ks(x, "k_chem");                                                                                        \
    hipLaunchKernelGGL((k_chem<NS, DT>), g, dim3(LANES), lds, x.stream, (long)x.C, perm, m, x.f("T"), x.f("p"), rho_rr,      \
                       x.f("Y"), dt, h.rtol, h.atol, h.Tmin, h.max_steps, h.method, x.f("RR"), stats, h.fail.p, tiled,   \
                       x.thermo.dhc.p, x.f("Qdot"));                                                          \
  } while (0)
  switch (x.S) {
    case 4: CALL(4); break; case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break;
    case 8: CALL(8); break; case 9: CALL(9); break; case 10: CALL(10); break; case 11: CALL(11); break;
    case 12: CALL(12); break;
    default: throw Error("chemistry: species count " + std::to_string(x.S) + " not instantiated");
  }
#undef CALL
  DFMI_HIP(hipGetLastError());
  chem_fail_snapshot(x);
}
}  // namespace

// The per-cell-interval instantiations are compiled in a translation unit of their own (chem_cells.hip includes this
// file with DFMI_CHEM_CELLS defined): with both sets in one unit the generated kinetics' functions have two callers, the
// inliner decides otherwise, and k_chem_gen<burke9> -- at its register limit -- changes (profiles/tci_resource_usage.md)
#ifdef DFMI_CHEM_CELLS
void chem_solve_cells(Ctx& x, const double* dt_cell, const char* rho_field) { chem_solve_t<const double*>(x, dt_cell, rho_field); }
#else
void chem_solve(Ctx& x, double dt, const char* rho_field) { chem_solve_t<double>(x, dt, rho_field); }

// The failure count leaves the device behind an event (no stream drain); chem_check reads it at the
// next host synchronisation point the caller already has (end of the time step's solver polls).
void chem_fail_snapshot(Ctx& x) {
  Chem& h = x.chem;
  if (h.batch) return;   // the batch's one snapshot follows its last step
  h.fail_host.ensure(1);
  if (!h.fail_ev) DFMI_HIP(hipEventCreateWithFlags(&h.fail_ev, hipEventDisableTiming));
  DFMI_HIP(hipMemcpyAsync(h.fail_host.p, h.fail.p, sizeof(int), hipMemcpyDeviceToHost, x.stream));
  DFMI_HIP(hipEventRecord(h.fail_ev, x.stream));
  h.fail_pending = true;
}

void chem_check(Ctx& x) {
  Chem& h = x.chem;
  if (!h.fail_pending) return;
  DFMI_HIP(hipEventSynchronize(h.fail_ev));
  h.fail_pending = false;
  const int nf = h.fail_host.p[0];
  DFMI_CHECK(nf == 0, "chemistry: " + std::to_string(nf) + " cell(s)" + (h.batch ? " (summed over the batch's steps)" : "") +
                          " hit the integrator step limit (max_steps = " + std::to_string(h.max_steps) +
                          "); their RR is not a completed integration");
}

// ---- turbulence-chemistry interaction: PaSR and EDC (options tci.*; include/dfmi.h) ----------------
namespace {
constexpr double TCI_SMALL = 1e-15, TCI_VGREAT = 1e300;

struct TciPar {
  int model, mixing, chem, version, e1, e2, fuel, ox, co2, h2;
  double Cmix, C1, C2, Cgamma, Ctau;
};

// PaSR chemistryScale reactionRate (PaSR.C:326-377): tc = sumW / sumSq * cSum from the forward and reverse rates of
// progress at Cantera's setState_TPX(T, p, X), X_i = rho Y_i / W_i. One cell per lane, the rate constants in LDS as
// k_chem keeps them; f and b are the expressions rhs() differences. Sums in reaction order, wf then wr.
template <int S>
__global__ void __launch_bounds__(LANES) k_tci_rates(long n, ChemMech m, const double* __restrict__ Tf,
                                                     const double* __restrict__ pf, const double* __restrict__ rhof,
                                                     const double* __restrict__ Yf, double* __restrict__ tc) {
  extern __shared__ double lds[];
  Lane<S> L;
  L.lane = threadIdx.x;
  L.kf = lds;
  L.k0 = lds + (long)m.R * LANES;
  L.ikc = lds + 2L * m.R * LANES;
  L.A = nullptr;
  const long c = (long)blockIdx.x * LANES + threadIdx.x;
  if (c >= n) return;   // no block-level synchronisation below
  const double T = Tf[c], rho = rhof[c];
  double X[S], C[S];
  double cSum = 0.0;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    X[i] = rho * Yf[(long)i * n + c] / m.W[i];
    cSum += X[i];
  }
  {   // setState_TPX: mole fractions clipped at 0 and normalised, C_i = x_i p / (R T)
    double xs = 0.0;
#pragma unroll
    for (int i = 0; i < S; ++i) xs += fmax(X[i], 0.0);
    const double ct = pf[c] / (RU * T);
#pragma unroll
    for (int i = 0; i < S; ++i) C[i] = fmax(X[i], 0.0) / xs * ct;
  }
  rate_constants<S>(m, L, T);
  double sumW = 0.0, sumSq = 0.0;
  for (int r = 0; r < m.R; ++r) {
    const int* id = m.idata + r * 8;
    const int* ix = m.irs + r * 6;
    const double* d = m.dd + (long)r * m.ndd;
    double k, Mf, Mc;
    rcoef<S>(m, L, r, T, C, k, Mf, Mc);
    double f = k, b = id[1] ? k * L.K(L.ikc, r) : 0.0;
    for (int j = 0; j < 3; ++j) {
      if (ix[j] >= 0) f *= ipow(sel<S>(C, ix[j]), d[3 + j]);
      if (ix[3 + j] >= 0) b *= ipow(sel<S>(C, ix[3 + j]), d[6 + j]);
    }
    const double fwd = Mf * f, rev = Mf * b;
    double wf = 0.0, wr = 0.0;
    for (int j = 0; j < 3; ++j) {
      if (ix[3 + j] >= 0) wf += d[6 + j] * fwd;
      if (ix[j] >= 0) wr += d[3 + j] * rev;
    }
    sumW += wf; sumW += wr;
    sumSq += wf * wf; sumSq += wr * wr;
  }
  tc[c] = sumSq == 0.0 ? TCI_VGREAT : sumW / sumSq * cSum;
}

// doubles of LDS one cell of the cooperative rates kernel takes: kf k0 ikc wf wr [R], C bv [S]
inline size_t tci_coop_cell_doubles(int S, int R) { return 5 * (size_t)R + 2 * (size_t)S; }

// the same for 13..64 species (and under chem.coop = 1): TG lanes per cell, the layout of k_chem_coop without its matrix
template <int TG, int NCB>
__global__ void __launch_bounds__(TG * NCB) k_tci_rates_coop(long n, ChemMech m, int S, const double* __restrict__ Tf,
                                                             const double* __restrict__ pf, const double* __restrict__ rhof,
                                                             const double* __restrict__ Yf, double* __restrict__ tc) {
  static_assert(LANES % TG == 0 && (TG * NCB) % LANES == 0, "a cell must not straddle waves");
  constexpr int RPL = Coop<TG>::RPL;
  extern __shared__ double lds[];
  const int R = m.R;
  Coop<TG> L;
  L.S = S; L.R = R; L.LD = S | 1; L.l = threadIdx.x % TG;
  {
    double* base = lds + (size_t)(threadIdx.x / TG) * (5 * (size_t)R + 2 * (size_t)S);
    L.A = nullptr;
    L.kf = base; L.k0 = base + R; L.ikc = base + 2 * R; L.ke = base + 3 * R; L.Mf = base + 4 * R;
    L.tb = nullptr; L.q = nullptr;
    base += 5 * R;
    L.C = base; L.bv = base + S;
  }
  const long c = (long)blockIdx.x * NCB + threadIdx.x / TG;
  if (c >= n) return;   // no workgroup barrier below: a cell is inside one wave
  const double T = Tf[c], rho = rhof[c];
  double X[RPL], a[RPL];
#pragma unroll
  for (int s = 0; s < RPL; ++s) {
    const int i = L.row(s);
    X[s] = i < S ? rho * Yf[(long)i * n + c] / m.W[i] : 0.0;
    a[s] = fmax(X[s], 0.0);
  }
  const double cSum = L.ordered_sum(X);
  const double xs = L.ordered_sum(a);
  const double ct = pf[c] / (RU * T);
#pragma unroll
  for (int s = 0; s < RPL; ++s) a[s] = a[s] / xs * ct;
  L.rate_constants(m, T);
  L.publish(a);
  L.progress(m, T);
  if (L.l == 0) {
    double sumW = 0.0, sumSq = 0.0;
    for (int r = 0; r < R; ++r) {
      const double wf = L.ke[r], wr = L.Mf[r];
      sumW += wf; sumW += wr;
      sumSq += wf * wf; sumSq += wr * wr;
    }
    tc[c] = sumSq == 0.0 ? TCI_VGREAT : sumW / sumSq * cSum;
  }
}

__device__ __forceinline__ double tci_ipow(double g, int e) {   // g^e, e in 1..4, as left-to-right products
  double v = g;
  for (int i = 1; i < e; ++i) v = v * g;
  return v;
}

// The pointwise pass. PaSR (after the solve): tmix, the RR-based tc forms (reactionRate: tc as k_tci_rates left it),
// kappa, and the consumers' RR_eff = kappa RR, Qdot_eff = kappa Qdot. EDC (before the solve): kappa and tauStar, the
// v2016 branch with tc the formationRate form of the RR the previous solve left; tauStar not positive and finite is counted.
// ST > 0: S = ST species held in registers, RR read once; ST = 0: any S, RR read again for the scaling.
template <int ST>
__global__ void __launch_bounds__(256) k_tci_kappa(long n, int S_rt, TciPar P, const double* __restrict__ kf,
                                                   const double* __restrict__ epsf, const double* __restrict__ muf,
                                                   const double* __restrict__ rhof, const double* __restrict__ Yf,
                                                   const double* __restrict__ RR, const double* __restrict__ Qdot,
                                                   double* __restrict__ tcf, double* __restrict__ tmixf,
                                                   double* __restrict__ tauf, double* __restrict__ kappaf,
                                                   double* __restrict__ RReff, double* __restrict__ Qeff,
                                                   int* __restrict__ bad) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const int S = ST ? ST : S_rt;
  const double k = kf[c], eps = epsf[c], mu = muf[c], rho = rhof[c];
  double rr[ST ? ST : 1];
  if (ST) {
#pragma unroll
    for (int i = 0; i < (ST ? ST : 1); ++i) rr[i] = RR[(long)i * n + c];
  }
  auto rr_at = [&](int i) -> double {
    if (ST) {
      double o = 0.0;
#pragma unroll
      for (int j = 0; j < (ST ? ST : 1); ++j) o = (j == i) ? rr[j] : o;
      return o;
    }
    return RR[(long)i * n + c];
  };
  // laminar::tc() (laminar.C:75-102), the formationRate form
  auto formation = [&]() -> double {
    double t = 0.0;
    if (ST) {
#pragma unroll
      for (int i = 0; i < (ST ? ST : 1); ++i) {
        const double a = fabs(rr[i]);
        t = fmax(t, a > TCI_SMALL ? Yf[(long)i * n + c] / a : 0.0);
      }
    } else {
      for (int i = 0; i < S; ++i) {
        const double a = fabs(RR[(long)i * n + c]);
        t = fmax(t, a > TCI_SMALL ? Yf[(long)i * n + c] / a : 0.0);
      }
    }
    return t;
  };
  if (P.model == 1) {
    const double e = eps + TCI_SMALL;
    double tmix;
    if (P.mixing == 1) tmix = P.Cmix * k / e;
    else if (P.mixing == 2) tmix = sqrt(fabs(mu / rho / e));
    else tmix = sqrt(fabs(k / e) * sqrt(fabs(mu / rho / e)));
    double tc;
    if (P.chem == 1) {
      const double t0 = tcf[c];
      bool first = true;
      tc = 0.0;
      auto take = [&](double t) { tc = first ? t : fmax(tc, t); first = false; };
      if (P.ox >= 0) { const double r = rr_at(P.ox), y = Yf[(long)P.ox * n + c]; take(r < 0.0 && y > 1e-10 ? -rho * y / r : t0); }
      if (P.fuel >= 0) { const double r = rr_at(P.fuel), y = Yf[(long)P.fuel * n + c]; take(r < 0.0 && y > 1e-10 ? -rho * y / r : t0); }
      if (P.co2 >= 0) { const double r = rr_at(P.co2), y = Yf[(long)P.co2 * n + c]; take(r > 0.0 && y > 1e-10 ? rho * y / r : t0); }
      if (P.h2 >= 0) { const double r = rr_at(P.h2), y = Yf[(long)P.h2 * n + c]; take(r < 0.0 && y > 1e-10 ? -rho * y / r : t0); }
    } else if (P.chem == 2) tc = formation();
    else tc = tcf[c];
    const double kappa = (tmix > TCI_SMALL && tc > TCI_SMALL) ? tc / (tc + tmix) : 1.0;
    tcf[c] = tc;
    tmixf[c] = tmix;
    kappaf[c] = kappa;
    if (ST) {
#pragma unroll
      for (int i = 0; i < (ST ? ST : 1); ++i) RReff[(long)i * n + c] = kappa * rr[i];
    } else {
      for (int i = 0; i < S; ++i) RReff[(long)i * n + c] = kappa * RR[(long)i * n + c];
    }
    Qeff[c] = kappa * Qdot[c];
    return;
  }
  // EDC (EDC.C:83-171)
  const double nu = mu / (rho + TCI_SMALL);
  const double tk = sqrt(nu / (eps + TCI_SMALL));
  const double g4 = sqrt(sqrt(nu * eps / (k * k + TCI_SMALL)));
  double gammaL, tauStar;
  if (P.version == 2016) {
    const double tc = formation();
    tcf[c] = tc;
    const double Da = fmax(fmin(tk / tc, 10.0), 1e-10);
    const double ReT = k * k / (nu * eps + TCI_SMALL);
    const double CtauI = fmin(P.C1 / (Da * sqrt(ReT + 1.0)), 2.1377);
    const double CgammaI = fmax(fmin(P.C2 * sqrt(Da * (ReT + 1.0)), 5.0), 0.4082);
    gammaL = CgammaI * g4;
    tauStar = CtauI * tk;
  } else {
    gammaL = P.Cgamma * g4;
    tauStar = P.Ctau * tk;
  }
  const double kappa = gammaL >= 1.0 ? 1.0 : fmax(fmin(tci_ipow(gammaL, P.e1) / (1.0 - tci_ipow(gammaL, P.e2)), 1.0), 0.0);
  kappaf[c] = kappa;
  tauf[c] = tauStar;
  if (!(tauStar > 0.0 && tauStar <= 1.79769313486231570e308)) atomicAdd(bad, 1);   // integer count
}

// EDC's consumers after the solve: RR_eff = kappa RR, Qdot_eff = kappa Qdot
__global__ void __launch_bounds__(256) k_tci_scale(long n, int S, const double* __restrict__ kappaf,
                                                   const double* __restrict__ RR, const double* __restrict__ Qdot,
                                                   double* __restrict__ RReff, double* __restrict__ Qeff) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double kappa = kappaf[c];
  for (int i = 0; i < S; ++i) RReff[(long)i * n + c] = kappa * RR[(long)i * n + c];
  Qeff[c] = kappa * Qdot[c];
}

__global__ void __launch_bounds__(256) k_tci_fill(long n, double v, double* __restrict__ a) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) a[c] = v;
}

TciPar tci_par(Ctx& x) {
  TciPar P;
  P.model = x.tci.model;
  P.mixing = (int)x.opt("tci.mixing");
  P.chem = (int)x.opt("tci.chemistry");
  P.version = (int)x.opt("tci.version");
  P.e1 = (int)x.opt("tci.exp1");
  P.e2 = (int)x.opt("tci.exp2");
  const int d1 = P.version == 1981 ? 3 : 2, d2 = (P.version == 1981 || P.version == 1996) ? 3 : 2;
  if (P.e1 == 0) P.e1 = d1;
  if (P.e2 == 0) P.e2 = d2;
  P.fuel = (int)x.opt("tci.fuel"); P.ox = (int)x.opt("tci.oxidizer"); P.co2 = (int)x.opt("tci.CO2"); P.h2 = (int)x.opt("tci.H2");
  P.Cmix = x.opt("tci.Cmix"); P.C1 = x.opt("tci.C1"); P.C2 = x.opt("tci.C2"); P.Cgamma = x.opt("tci.Cgamma"); P.Ctau = x.opt("tci.Ctau");
  return P;
}

void tci_rates(Ctx& x) {
  Chem& h = x.chem;
  ChemMech m{h.R, h.ndd, h.idata.p, h.irs.p, h.dd.p, x.thermo.dnasa.p, x.thermo.dW.p};
  const bool coop = x.S > 12 || x.on("chem.coop");
  KScope _ks(x, "k_tci_rates");
  if (coop) {
    const int tg = coop_lanes_for(x.S);
    const int ncb = LANES / tg;
    const size_t clds = tci_coop_cell_doubles(x.S, h.R) * sizeof(double) * ncb;
    DFMI_CHECK(clds <= 64 * 1024, "tci reactionRate: mechanism too large for the LDS layout");
    const dim3 g((unsigned)blocks_for((long)x.C, ncb));
#define COOP(TG, NCB)                                                                                              \
  hipLaunchKernelGGL((k_tci_rates_coop<TG, NCB>), g, dim3(TG * NCB), clds, x.stream, (long)x.C, m, x.S, x.f("T"),   \
                     x.f("p"), x.f("rho"), x.f("Y"), x.f("tci_tc"))
    if (tg == 16) COOP(16, 4); else if (tg == 32) COOP(32, 2); else COOP(64, 1);
#undef COOP
    DFMI_HIP(hipGetLastError());
    return;
  }
  const size_t lds = (size_t)3 * h.R * LANES * sizeof(double);
  DFMI_CHECK(lds <= 64 * 1024, "tci reactionRate: mechanism too large for the LDS layout");
  const dim3 g((unsigned)blocks_for((long)x.C, LANES));
#define CALL(NS)                                                                                                   \
  hipLaunchKernelGGL(k_tci_rates<NS>, g, dim3(LANES), lds, x.stream, (long)x.C, m, x.f("T"), x.f("p"), x.f("rho"), \
                     x.f("Y"), x.f("tci_tc"))
  switch (x.S) {
    case 4: CALL(4); break; case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break;
    case 8: CALL(8); break; case 9: CALL(9); break; case 10: CALL(10); break; case 11: CALL(11); break;
    case 12: CALL(12); break;
    default: throw Error("tci reactionRate: species count " + std::to_string(x.S) + " not instantiated");
  }
#undef CALL
  DFMI_HIP(hipGetLastError());
}

void tci_kappa(Ctx& x, const TciPar& P) {
  KScope _ks(x, "k_tci_kappa");
  const dim3 g((unsigned)blocks_for((long)x.C, 256));
#define CALL(NS)                                                                                                       \
  hipLaunchKernelGGL(k_tci_kappa<NS>, g, dim3(256), 0, x.stream, (long)x.C, x.S, P, x.f("k"), x.f("epsilon"), x.f("mu"), \
                     x.f("rho"), x.f("Y"), x.f("RR"), x.f("Qdot"), x.f("tci_tc"), x.f("tci_tmix"), x.f("tci_tauStar"),  \
                     x.f("tci_kappa"), x.f("RR_eff"), x.f("Qdot_eff"), x.tci.bad.p)
  switch (x.S) {
    case 4: CALL(4); break; case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break;
    case 8: CALL(8); break; case 9: CALL(9); break; case 10: CALL(10); break; case 11: CALL(11); break;
    case 12: CALL(12); break;
    default: CALL(0); break;
  }
#undef CALL
  DFMI_HIP(hipGetLastError());
}
}  // namespace

void ensure_tci_fields(Ctx& x) {
  if (x.fields.count("tci_kappa")) return;
  DFMI_CHECK(x.have_sizes, "call dfmi_set_constant_values first");
  auto mk = [&](const char* name, long n, int ncomp) {
    Field& f = x.fields[name];
    f.n = n; f.ncomp = ncomp; f.boundary = false; f.face = false;
    f.buf.alloc((size_t)n * ncomp);
    f.buf.zero(x.stream);
  };
  for (auto n : {"tci_kappa", "tci_tmix", "tci_tauStar", "tci_tc", "Qdot_eff"}) mk(n, x.C, 1);
  mk("RR_eff", x.C, x.S);
  x.tci.bad.alloc(1);
  DFMI_HIP(hipMemsetAsync(x.tci.bad.p, 0, sizeof(int), x.stream));
  tci_reset_tc(x);
}

// tci_tc starts at 0.1 (PaSR.C:77: tc_ is constructed with that value) and persists from call to call
void tci_reset_tc(Ctx& x) {
  if (!x.fields.count("tci_tc")) return;
  hipLaunchKernelGGL(k_tci_fill, dim3((unsigned)blocks_for((long)x.C, 256)), dim3(256), 0, x.stream, (long)x.C, 0.1, x.f("tci_tc"));
}

namespace {
TciPar tci_validate(Ctx& x) {
  DFMI_CHECK(x.ras.model == 1, "tci.model != 0 needs ras.model = 1 (k and epsilon exist only there)");
  DFMI_CHECK(!x.les.model, "tci.model != 0 and les.model != 0 exclude each other");
  DFMI_CHECK(x.chem.mode != 2, "tci.model != 0 is not available with the DNN surrogate (chemistry mode 2)");
  DFMI_CHECK(x.chem.mode == 1, "tci.model != 0 needs chemistry mode 1 (stiff integration; dfmi_chem_set_options)");
  for (int i = 0; i < 2; ++i)
    DFMI_CHECK(x.ras.have[i], std::string("tci: the field '") + (i ? "epsilon" : "k") + "' is not set (dfmi_set_field)");
  const TciPar P = tci_par(x);
  DFMI_CHECK(!(P.model == 1 && P.chem == 1 && P.fuel < 0),
             "tci.chemistry = 1 (globalConvertion) needs tci.fuel >= 0 (PaSR.C:259-264: the fuel species is not set)");
  for (int i : {P.fuel, P.ox, P.co2, P.h2}) DFMI_CHECK(i < x.S, "tci: a species index is outside the mechanism's species");
  DFMI_CHECK(x.chem.ready || !(P.model == 1 && P.chem == 3), "chemistry mechanism not set (dfmi_chem_set_mechanism)");
  ensure_tci_fields(x);
  return P;
}
void tci_scale(Ctx& x) {
  KScope _ks(x, "k_tci_scale");
  hipLaunchKernelGGL(k_tci_scale, dim3((unsigned)blocks_for((long)x.C, 256)), dim3(256), 0, x.stream, (long)x.C, x.S,
                     x.f("tci_kappa"), x.f("RR"), x.f("Qdot"), x.f("RR_eff"), x.f("Qdot_eff"));
  DFMI_HIP(hipGetLastError());
}
}  // namespace

void combustion_correct(Ctx& x, double dt, const char* rho_field) {
  if (!x.tci.model) { chem_solve(x, dt, rho_field); return; }   // laminar: combustion->correct() is the solve
  const TciPar P = tci_validate(x);
  if (P.model == 1) {
    chem_solve(x, dt, rho_field);   // laminar::correct()
    if (P.chem == 3) tci_rates(x);
    tci_kappa(x, P);
    return;
  }
  DFMI_HIP(hipMemsetAsync(x.tci.bad.p, 0, sizeof(int), x.stream));
  tci_kappa(x, P);
  chem_solve_cells(x, x.f("tci_tauStar"), rho_field);   // chemistryPtr_->solve(tauStar)
  tci_scale(x);
}

// dfmi_assemble("tci"): the closure's pointwise passes from the fields as they stand, RR and Qdot included -- no solve
void combustion_pointwise(Ctx& x) {
  DFMI_CHECK(x.tci.model, "dfmi_assemble: 'tci' needs tci.model != 0");
  const TciPar P = tci_validate(x);
  if (P.model == 1) {
    if (P.chem == 3) tci_rates(x);
    tci_kappa(x, P);
    return;
  }
  DFMI_HIP(hipMemsetAsync(x.tci.bad.p, 0, sizeof(int), x.stream));
  tci_kappa(x, P);
  tci_scale(x);
}

#endif  // DFMI_CHEM_CELLS
}  // namespace dfmi
