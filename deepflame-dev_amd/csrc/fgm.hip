// fgm.hip -- flareFGM on the device: the flamelet table and the retrieval kernels (include/dfmi.h, flareFGM block;
// DESIGN.md 18). flareFGM::retrieval() (src/dfCombustionModels/FGM/flareFGM/flareFGM.C:147-762, the non-LES branch) and the
// lookups of flameletTableSolver/tableSolver.C, statement for statement, one cell or one boundary slot per lane.
//
// Arithmetic contract (a NumPy float64 restatement reproduces every lookup bitwise; -ffp-contract=off):
//   weight of corner bit i on an axis with factor f:  (1.0 - f) + i * (2.0 * f - 1.0)
//   factor of a corner:  ((((w0 * w1) * w2) * w3) * w4) * w5          sum:  result = result + factor * table[loc]
// in the reference's i0 .. i5 nesting. The six (loc, fac) pairs are formed once per point and shared by every table; the
// unscaled progress variable's Ycmax lookup (c = 0, gc = 0, gzc = 0) comes first with three pairs of its own.
//
// Bounds: locate() returns an index in [0, max(n - 2, 0)] for any x, NaN included, and a corner's upper index is
// loc + 1 only where n > 1, so every gather index lies inside its table for any input; dfmi_fgm_set_table's checks
// (dimensions >= 1, NZL >= 2, species indices inside the mechanism) are what make the table extents what the kernel
// assumes. An axis of length 1 has fac = 0 exactly (the reference reads list[1] past its end).
#include "dfmi_ctx.h"
#include <cmath>

namespace dfmi {

namespace {

constexpr double FGM_SMALL = 1.0e-4, FGM_SMALLER = 1.0e-6;   // tableSolver::small / smaller
constexpr double FOAM_SMALL = 1.0e-15;                        // OpenFOAM's SMALL
constexpr double FGM_T0 = 298.15, FGM_RU = 8.314e3;

struct FgmTab {
  int n[6];                      // NH NZ NC NGZ NGC NZC
  int NS, NYo, NY, NZL, NV, scaled;
  const double* ax[6];
  const double *lz, *sl, *th, *tau, *kct;   // laminar block [NH NZL]
  const double* tab;             // [N][NV]
  const double* dyeq;            // [NH NZ NGZ][2]
  const int* ysp;                // [NY]
  double Hfu, Hox;
};
struct FgmOpt {
  int combustion, flameletT, write_rho;
  double incompPref, TMin, TMax;
};
// the fields of one side (cells or slots); n = values per component
struct FgmIO {
  long n;
  const double *Z, *Zvar, *c, *cvar, *Zcvar, *Ha, *k, *eps, *p;
  double *mu, *rho, *rho_th, *T, *psi, *Y, *omY;
  double *chiZ, *chiZc, *chic, *omc, *cOmc, *ZOmc, *Has, *cs, *Zvs, *cvs, *Zcvs, *Wt, *Cp, *Hf;
};

// Foam::max / Foam::min of two scalars
__host__ __device__ __forceinline__ double fmax2(double a, double b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ double fmin2(double a, double b) { return a < b ? a : b; }

struct LF { int loc; double fac; };

// tableSolver::locate_lower; any x (NaN: n - 2) gives an index in [0, max(n - 2, 0)]
__host__ __device__ __forceinline__ int fgm_locate(int n, const double* __restrict__ a, double x) {
  if (n == 1) return 0;
  if (x <= a[0]) return 0;
  if (x >= a[n - 1]) return n - 2;
  for (int i = 0; i < n - 1; ++i)
    if (x >= a[i] && x < a[i + 1]) return i;
  return n - 2;
}
// tableSolver::intfac
__host__ __device__ __forceinline__ double fgm_intfac(double xx, double low, double high) {
  if (xx <= low) return 0.0;
  if (xx >= high) return 1.0;
  if ((high - low) < 1e-30) return 0.0;
  return (xx - low) / (high - low);
}
__host__ __device__ __forceinline__ LF fgm_pair(int n, const double* __restrict__ a, double x) {
  LF r;
  r.loc = fgm_locate(n, a, x);
  r.fac = n > 1 ? fgm_intfac(x, a[r.loc], a[r.loc + 1]) : 0.0;   // length 1: fac = 0 exactly
  return r;
}
__host__ __device__ __forceinline__ double fgm_w(int i, double f) { return (1.0 - f) + (double)i * (2.0 * f - 1.0); }

// tableSolver::interp6d for the K variables v0 .. v0 + K - 1 of the corner-major table on one sweep over the 64 corners
template <int K>
__host__ __device__ __forceinline__ void fgm_lookup6(const FgmTab& t, const LF (&p)[6], int v0, double (&out)[K]) {
  // the outer four axes as one rolled loop of 16 (i0 i1 i2 i3 in the nesting's order), the inner two unrolled: four
  // corners' loads in flight per trip. Unrolling all 64 hoists 64 K loads and spills (512 registers and 4 KB of scratch
  // per lane at K = 8)
  double w0[6], w1[6];
  long st[6];
  st[5] = 1;
#pragma unroll
  for (int d = 4; d >= 0; --d) st[d] = st[d + 1] * t.n[d + 1];
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    w0[d] = fgm_w(0, p[d].fac); w1[d] = fgm_w(1, p[d].fac);
    if (t.n[d] <= 1) st[d] = 0;   // no upper neighbour: the corner's index stays loc
  }
  long base = 0;
  {
    long s = 1;
#pragma unroll
    for (int d = 5; d >= 0; --d) { base += p[d].loc * s; s *= t.n[d]; }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.0;
#pragma unroll 1
  for (int o = 0; o < 16; ++o) {
    const bool i0 = o & 8, i1 = o & 4, i2 = o & 2, i3 = o & 1;
    const double f3 = (((i0 ? w1[0] : w0[0]) * (i1 ? w1[1] : w0[1])) * (i2 ? w1[2] : w0[2])) * (i3 ? w1[3] : w0[3]);
    const long l3 = base + (i0 ? st[0] : 0) + (i1 ? st[1] : 0) + (i2 ? st[2] : 0) + (i3 ? st[3] : 0);
#pragma unroll
    for (int i4 = 0; i4 < 2; ++i4) {
      const double f4 = f3 * (i4 ? w1[4] : w0[4]);
#pragma unroll
      for (int i5 = 0; i5 < 2; ++i5) {
        const long loc = l3 + (i4 ? st[4] : 0) + (i5 ? st[5] : 0);
        const double factor = f4 * (i5 ? w1[5] : w0[5]);
        const double* __restrict__ row = t.tab + loc * t.NV + v0;
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = out[k] + factor * row[k];
      }
    }
  }
}
// tableSolver::interp2d on the laminar block: (h, z) pairs, z located on the block's first row as lookup2d does
__host__ __device__ __forceinline__ double fgm_lookup2(const FgmTab& t, const LF& ph, const LF& pz, const double* __restrict__ tb) {
  double r = 0.0;
  const int uh = t.n[0] > 1 ? 1 : 0;   // NZL >= 2: the z corner always has an upper neighbour
#pragma unroll
  for (int i1 = 0; i1 < 2; ++i1)
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2) {
      const double factor = fgm_w(i1, ph.fac) * fgm_w(i2, pz.fac);
      r = r + factor * tb[(ph.loc + i1 * uh) * t.NZL + (pz.loc + i2)];
    }
  return r;
}
// tableSolver::interp3d on the non-premixed block: (h, z, gz); comp 0: d2Yeq, 1: d1Yeq
__host__ __device__ __forceinline__ double fgm_lookup3(const FgmTab& t, const LF& ph, const LF& pz, const LF& pg, int comp) {
  double r = 0.0;
  const int u0 = t.n[0] > 1 ? 1 : 0, u1 = t.n[1] > 1 ? 1 : 0, u2 = t.n[3] > 1 ? 1 : 0;
#pragma unroll
  for (int i0 = 0; i0 < 2; ++i0)
#pragma unroll
    for (int i1 = 0; i1 < 2; ++i1)
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        const double factor = (fgm_w(i0, ph.fac) * fgm_w(i1, pz.fac)) * fgm_w(i2, pg.fac);
        const long loc = ((long)(ph.loc + i0 * u0) * t.n[1] + (pz.loc + i1 * u1)) * t.n[3] + (pg.loc + i2 * u2);
        r = r + factor * t.dyeq[2 * loc + comp];
      }
  return r;
}
// tableSolver::cal_gvar (Ycmax < 0: the scaled form)
__host__ __device__ __forceinline__ double fgm_gvar(double mean, double var, double Ycmax) {
  double g;
  if (mean < FGM_SMALL || mean > (1.0 - FGM_SMALL)) g = 0.0;
  else if (Ycmax < 0.0) g = var / (mean * (1. - mean));
  else g = var / (mean * (Ycmax - mean));
  g = fmin2(1.0, g);
  g = fmax2(FGM_SMALLER, g);
  return g;
}
// tableSolver::cal_gcor
__host__ __device__ __forceinline__ double fgm_gcor(double Zvar, double cvar, double Zcvar) {
  double g;
  if ((cvar < 1.0e-4) || (Zvar < 1.0e-6)) g = 0.0;
  else g = Zcvar / (sqrt(Zvar) * sqrt(cvar));
  g = fmin(1.0, g);
  g = fmax(-1.0, g);
  return g;
}
// tableSolver::RANSsdrFLRmodel
__host__ __device__ __forceinline__ double fgm_rans_sdr(double cvar, double eps, double k, double nu, double sl, double dl, double tau,
                                               double kc_s, double rho) {
  const double beta = 6.7;
  const double Ka = (dl / (sl + FOAM_SMALL)) / (sqrt(nu / eps) + FOAM_SMALL);
  const double Kc = kc_s * tau;
  const double C3 = 1.5 * sqrt(Ka) / (1 + sqrt(Ka));
  const double C4 = 1.1 / pow((1 + Ka), 0.4);
  return rho / beta * cvar * ((2.0 * Kc - tau * C4) * sl / (dl + FOAM_SMALL) + C3 * eps / (k + FOAM_SMALL));
}

// one cell (SLOT = false) or boundary slot (SLOT = true): the loop body of flareFGM::retrieval() in its statement order.
// chi_c reads nu = mu / rho from mu and rho as they stand on entry; mu is overwritten with the density as it stands on
// entry; psi and rho come last.
template <bool SLOT>
__host__ __device__ __forceinline__ void fgm_point(const FgmTab& t, const FgmOpt& o, const FgmIO& f, long i) {
  const double Z = f.Z[i], Zvar = f.Zvar[i], c = f.c[i], cvar = f.cvar[i], Zcvar = f.Zcvar[i], Ha = f.Ha[i];
  const double k = f.k[i], eps = f.eps[i], rho_in = f.rho[i], mu_in = f.mu[i];
  const double chiZ = 1.0 * eps / k * Zvar;
  const double chiZc = 1.0 * eps / k * Zcvar;
  f.chiZ[i] = chiZ; f.chiZc[i] = chiZc;

  double hLoss = (Z * (t.Hfu - t.Hox) + t.Hox) - Ha;
  hLoss = fmax2(hLoss, t.ax[0][0]);
  hLoss = fmin2(hLoss, t.ax[0][t.n[0] - 1]);
  LF p[6];
  p[0] = fgm_pair(t.n[0], t.ax[0], hLoss);
  const int ih = p[0].loc;
  const double Zl = t.lz[ih * t.NZL], Zr = t.lz[(ih + 1) * t.NZL - 1];
  const bool flame = Z >= Zl && Z <= Zr && o.combustion && c > FGM_SMALL;

  if (flame) {
    const LF pzl = fgm_pair(t.NZL, t.lz, Z);
    const double kc_s = fgm_lookup2(t, p[0], pzl, t.kct);
    const double tau = fgm_lookup2(t, p[0], pzl, t.tau);
    const double sl = fgm_lookup2(t, p[0], pzl, t.sl);
    const double dl = fgm_lookup2(t, p[0], pzl, t.th);
    f.chic[i] = fgm_rans_sdr(cvar, eps, k, mu_in / rho_in, sl, dl, tau, kc_s, rho_in);
  } else {
    f.chic[i] = SLOT ? 1.0 * eps / (k + FOAM_SMALL) * cvar : 1.0 * eps / k * cvar;
  }

  const double gz = fgm_gvar(Z, Zvar, -1.0);
  const double gcz = fgm_gcor(Zvar, cvar, Zcvar);
  p[1] = fgm_pair(t.n[1], t.ax[1], Z);
  p[3] = fgm_pair(t.n[3], t.ax[3], gz);
  double Ycmax = -1.0, cNorm;
  if (t.scaled) cNorm = c;
  else {
    LF q[6] = {p[0], p[1], fgm_pair(t.n[2], t.ax[2], 0.0), p[3], fgm_pair(t.n[4], t.ax[4], 0.0), fgm_pair(t.n[5], t.ax[5], 0.0)};
    double y[1];
    fgm_lookup6<1>(t, q, t.NS - 1, y);
    Ycmax = fmax2(FGM_SMALLER, y[0]);
    cNorm = c / Ycmax;
  }
  const double gc = fgm_gvar(c, cvar, Ycmax);
  p[2] = fgm_pair(t.n[2], t.ax[2], cNorm);
  p[4] = fgm_pair(t.n[4], t.ax[4], gc);
  p[5] = fgm_pair(t.n[5], t.ax[5], gcz);

  // the eight thermo-chemical tables on one sweep: omgc, cOc, ZOc, cp, mwt, hiyi, Tf, nu
  double L[8];
  fgm_lookup6<8>(t, p, 0, L);
  double omc, cOmc, ZOmc;
  if (flame) {
    omc = L[0] + (t.scaled ? (chiZ * c * fgm_lookup3(t, p[0], p[1], p[3], 0) + 2.0 * chiZc * fgm_lookup3(t, p[0], p[1], p[3], 1))
                           : 0.0);
    cOmc = L[1];
    ZOmc = L[2];
  } else {
    omc = 0.0; cOmc = 0.0; ZOmc = 0.0;
  }
  f.omc[i] = omc * rho_in; f.cOmc[i] = cOmc * rho_in; f.ZOmc[i] = ZOmc * rho_in;
  f.Has[i] = hLoss; f.cs[i] = cNorm; f.Zvs[i] = gz; f.cvs[i] = gc; f.Zcvs[i] = gcz;
  const double Wt = L[4];
  f.Wt[i] = Wt;
  f.mu[i] = L[7] * rho_in;

  // the NYomega source-term species (tables NS - NYomega ..) and the NY species (tables NS ..): one run of variables
  {
    const int v0 = t.NS - t.NYo, nv = t.NYo + t.NY;
    int j = 0;
    auto put = [&](int jj, double val) {
      if (jj < t.NYo) f.omY[(long)jj * f.n + i] = val;
      else f.Y[(long)t.ysp[jj - t.NYo] * f.n + i] = val;
    };
    for (; j + 4 <= nv; j += 4) {
      double y[4];
      fgm_lookup6<4>(t, p, v0 + j, y);
#pragma unroll
      for (int q = 0; q < 4; ++q) put(j + q, y[q]);
    }
    for (; j < nv; ++j) {
      double y[1];
      fgm_lookup6<1>(t, p, v0 + j, y);
      put(j, y[0]);
    }
  }

  double T;
  if (o.flameletT) T = L[6];
  else {
    f.Cp[i] = L[3];
    f.Hf[i] = L[5];
    T = (Ha - L[5]) / L[3] + FGM_T0;
  }
  T = fmax2(T, o.TMin);
  T = fmin2(T, o.TMax);
  f.T[i] = T;
  const double psi = Wt / (FGM_RU * T);
  f.psi[i] = psi;
  if (SLOT || o.write_rho) {
    const double r = o.incompPref > 0.0 ? o.incompPref * psi : f.p[i] * psi;
    f.rho[i] = r;
    f.rho_th[i] = r;
  } else {
    f.rho_th[i] = rho_in;   // rho_inRhoThermo_ = rho_ (flareFGM.C:760)
  }
}

__global__ void __launch_bounds__(256) k_fgm_retrieve_cells(FgmTab t, FgmOpt o, FgmIO f) {
  const long i = xcd_block() * (long)blockDim.x + threadIdx.x;
  if (i >= f.n) return;
  fgm_point<false>(t, o, f, i);
}

// boundary slots by k_thermo_slots' rules: empty slots untouched, processor [internal n] slots copy their cell
__global__ void __launch_bounds__(256) k_fgm_retrieve_slots(MeshView m, const int8_t* __restrict__ ty, FgmTab t, FgmOpt o,
                                                            FgmIO f, FgmIO cf) {
  const long b = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (b >= f.n) return;
  const int tb = ty[b];
  if (tb == EMPTY) return;
  if (bc_proc(tb) && !m.sprim[b]) {
    const long c = m.bfc[b];
    f.chiZ[b] = cf.chiZ[c]; f.chiZc[b] = cf.chiZc[c]; f.chic[b] = cf.chic[c];
    f.omc[b] = cf.omc[c]; f.cOmc[b] = cf.cOmc[c]; f.ZOmc[b] = cf.ZOmc[c];
    f.Has[b] = cf.Has[c]; f.cs[b] = cf.cs[c]; f.Zvs[b] = cf.Zvs[c]; f.cvs[b] = cf.cvs[c]; f.Zcvs[b] = cf.Zcvs[c];
    f.Wt[b] = cf.Wt[c]; f.Cp[b] = cf.Cp[c]; f.Hf[b] = cf.Hf[c]; f.mu[b] = cf.mu[c];
    f.T[b] = cf.T[c]; f.psi[b] = cf.psi[c]; f.rho[b] = cf.rho[c]; f.rho_th[b] = cf.rho_th[c];
    for (int j = 0; j < t.NYo; ++j) f.omY[(long)j * f.n + b] = cf.omY[(long)j * cf.n + c];
    for (int j = 0; j < t.NY; ++j) f.Y[(long)t.ysp[j] * f.n + b] = cf.Y[(long)t.ysp[j] * cf.n + c];
    return;
  }
  fgm_point<true>(t, o, f, b);
}

FgmTab fgm_tab(Ctx& x) {
  const Fgm& g = x.fgm;
  FgmTab t{};
  long off = 0;
  for (int d = 0; d < 6; ++d) { t.n[d] = g.n[d]; t.ax[d] = g.axes.p + off; off += g.n[d]; }
  t.NS = g.NS; t.NYo = g.NYomega; t.NY = g.NY; t.NZL = g.NZL; t.NV = g.NS + g.NY; t.scaled = g.scaled ? 1 : 0;
  const long nl = (long)g.n[0] * g.NZL;
  t.lz = g.lam.p; t.sl = g.lam.p + nl; t.th = g.lam.p + 2 * nl; t.tau = g.lam.p + 3 * nl; t.kct = g.lam.p + 4 * nl;
  t.tab = g.tab.p; t.dyeq = g.dyeq.p; t.ysp = g.ysp.p;
  t.Hfu = g.Hfu; t.Hox = g.Hox;
  return t;
}
FgmIO fgm_io(Ctx& x, bool boundary) {
  const std::string pre = boundary ? "boundary_" : "";
  auto f = [&](const char* n) { return x.f(pre + n); };
  FgmIO io{};
  io.n = boundary ? x.B : x.C;
  io.Z = f("Z"); io.Zvar = f("Zvar"); io.c = f("c"); io.cvar = f("cvar"); io.Zcvar = f("Zcvar"); io.Ha = f("Ha");
  io.k = f("k"); io.eps = f("epsilon"); io.p = f("p");
  io.mu = f("mu"); io.rho = f("rho"); io.rho_th = f("rho_thermo"); io.T = f("T"); io.psi = f("psi"); io.Y = f("Y");
  io.omY = f("omega_Yi");
  io.chiZ = f("chi_Z"); io.chiZc = f("chi_Zc"); io.chic = f("chi_c"); io.omc = f("omega_c"); io.cOmc = f("cOmega_c");
  io.ZOmc = f("ZOmega_c"); io.Has = f("Ha_s"); io.cs = f("c_s"); io.Zvs = f("Zvar_s"); io.cvs = f("cvar_s");
  io.Zcvs = f("Zcvar_s"); io.Wt = f("Wt"); io.Cp = f("Cp"); io.Hf = f("Hf");
  return io;
}

bool finite_all(const double* a, long n) {
  for (long i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false;
  return true;
}

}  // namespace

void fgm_set_table(Ctx& x, const int* dims, const double* axes, double Hfu, double Hox, const double* laminar,
                   const double* tables, const double* d2Yeq, const double* d1Yeq, const int* species_index,
                   const int* omega_index) {
  const char* who = "dfmi_fgm_set_table: ";
  DFMI_CHECK(x.have_sizes, std::string(who) + "call dfmi_set_constant_values first");
  DFMI_CHECK(dims && axes && laminar && tables, std::string(who) + "null argument");
  static const char* dn[6] = {"NH", "NZ", "NC", "NGZ", "NGC", "NZC"};
  static const char* an[6] = {"h", "z", "c", "gz", "gc", "gzc"};
  for (int d = 0; d < 6; ++d)
    DFMI_CHECK(dims[d] >= 1, std::string(who) + "dimension " + dn[d] + " = " + std::to_string(dims[d]) + " must be at least 1");
  const int NS = dims[6], NYo = dims[7], NY = dims[8], NZL = dims[9];
  DFMI_CHECK(NYo >= 0 && NY >= 0, std::string(who) + "NYomega and NY must not be negative");
  DFMI_CHECK(NS == 8 + NYo || NS == 9 + NYo, std::string(who) + "NS = " + std::to_string(NS) + " must be 8 + NYomega (scaled "
             "progress variable) or 9 + NYomega (unscaled, last column Ycmax); NYomega = " + std::to_string(NYo));
  DFMI_CHECK(NZL >= 2, std::string(who) + "NZL = " + std::to_string(NZL) + " must be at least 2");
  const bool scaled = NS == 8 + NYo;
  DFMI_CHECK(NY == 0 || species_index, std::string(who) + "null species index array");
  DFMI_CHECK(NYo == 0 || omega_index, std::string(who) + "null omega species index array");
  DFMI_CHECK(!scaled || (d2Yeq && d1Yeq), std::string(who) + "a scaled-PV table (NS == 8 + NYomega) needs d2Yeq and d1Yeq");
  long N = 1, na = 0;
  for (int d = 0; d < 6; ++d) {
    N *= dims[d];
    // the host transposes the tables once into a second copy, and the device holds them: 2^28 values are 2 GiB
    DFMI_CHECK(N * (long)(NS + NY) <= (1L << 28), std::string(who) + "the value tables hold more than 2^28 entries (" +
               std::to_string(NS + NY) + " tables over the grid): too large");
    const double* a = axes + na;
    DFMI_CHECK(finite_all(a, dims[d]), std::string(who) + "axis " + an[d] + " holds a value that is not finite");
    for (int i = 1; i < dims[d]; ++i)
      DFMI_CHECK(a[i] > a[i - 1], std::string(who) + "axis " + an[d] + " is not strictly increasing at index " + std::to_string(i));
    na += dims[d];
  }
  DFMI_CHECK(std::isfinite(Hfu) && std::isfinite(Hox), std::string(who) + "Hfu / Hox is not finite");
  const int NH = dims[0], NV = NS + NY;
  const long nl = (long)NH * NZL, n3 = (long)NH * dims[1] * dims[3];
  DFMI_CHECK(finite_all(laminar, 5 * nl), std::string(who) + "the laminar block holds a value that is not finite");
  for (int h = 0; h < NH; ++h)
    for (int j = 1; j < NZL; ++j)
      DFMI_CHECK(laminar[h * NZL + j] > laminar[h * NZL + j - 1],
                 std::string(who) + "axis z of the laminar block is not strictly increasing in row " + std::to_string(h));
  DFMI_CHECK(finite_all(tables, (long)NV * N), std::string(who) + "a value table holds a value that is not finite");
  if (scaled)
    DFMI_CHECK(finite_all(d2Yeq, n3) && finite_all(d1Yeq, n3), std::string(who) + "d2Yeq / d1Yeq holds a value that is not finite");
  for (int j = 0; j < NY; ++j)
    DFMI_CHECK(species_index[j] >= 0 && species_index[j] < x.S, std::string(who) + "species index " +
               std::to_string(species_index[j]) + " (table species " + std::to_string(j) + ") out of range");
  for (int j = 0; j < NYo; ++j)
    DFMI_CHECK(omega_index[j] >= 0 && omega_index[j] < x.S, std::string(who) + "species index " +
               std::to_string(omega_index[j]) + " (omega species " + std::to_string(j) + ") out of range");

  Fgm& g = x.fgm;
  for (int d = 0; d < 6; ++d) g.n[d] = dims[d];
  g.NS = NS; g.NYomega = NYo; g.NY = NY; g.NZL = NZL; g.N = N; g.scaled = scaled; g.Hfu = Hfu; g.Hox = Hox;
  g.axes.upload(axes, (size_t)na, x.stream);
  g.lam.upload(laminar, (size_t)(5 * nl), x.stream);
  std::vector<double> cm((size_t)N * NV);   // corner-major: the variables of one corner contiguous
  for (int v = 0; v < NV; ++v)
    for (long l = 0; l < N; ++l) cm[(size_t)l * NV + v] = tables[(size_t)v * N + l];
  g.tab.upload(cm, x.stream);
  std::vector<double> dy;
  if (scaled) {
    dy.resize((size_t)2 * n3);
    for (long l = 0; l < n3; ++l) { dy[2 * l] = d2Yeq[l]; dy[2 * l + 1] = d1Yeq[l]; }
  }
  g.dyeq.upload(dy, x.stream);
  g.h_ysp.assign(species_index, species_index + NY);
  g.h_osp.assign(omega_index, omega_index + NYo);
  g.ysp.upload(g.h_ysp, x.stream);
  DFMI_HIP(hipStreamSynchronize(x.stream));   // the host staging arrays go out of scope
  g.have_table = true;
}

void fgm_retrieve(Ctx& x, bool write_rho) {
  DFMI_CHECK(x.fgm.have_table, "flareFGM: no table set (dfmi_fgm_set_table)");
  const FgmTab t = fgm_tab(x);
  const FgmOpt o{x.on("fgm.combustion") ? 1 : 0, x.on("fgm.flameletT") ? 1 : 0, write_rho ? 1 : 0, x.opt("fgm.incompPref"),
                 x.opt("fgm.TMin"), x.opt("fgm.TMax")};
  const FgmIO fc = fgm_io(x, false), fb = fgm_io(x, true);
  if (x.C > 0) {
    KScope _ks(x, "k_fgm_retrieve_cells");
    hipLaunchKernelGGL(k_fgm_retrieve_cells, dim3(blocks_for(x.C, 256)), dim3(256), 0, x.stream, t, o, fc);
  }
  DFMI_HIP(hipGetLastError());
  if (x.B > 0) {
    KScope _ks(x, "k_fgm_retrieve_slots");
    hipLaunchKernelGGL(k_fgm_retrieve_slots, dim3(blocks_for(x.B, 256)), dim3(256), 0, x.stream, x.view(), x.st("calculated"),
                       t, o, fb, fc);
  }
  DFMI_HIP(hipGetLastError());
  // neighbour halves of the processor slots carry the neighbour rank's cell values: one exchange
  std::vector<const char*> names = {"chi_Z", "chi_Zc", "chi_c", "omega_c", "cOmega_c", "ZOmega_c", "Ha_s", "c_s", "Zvar_s",
                                    "cvar_s", "Zcvar_s", "Wt", "Cp", "Hf", "mu", "T", "psi", "rho", "rho_thermo", "Y"};
  if (x.fgm.NYomega > 0) names.push_back("omega_Yi");
  halo_fields(x, names);
}

}  // namespace dfmi
