// capi.cpp -- extern "C" boundary (include/dfmi.h) and the PIMPLE orchestration.
//
// Host side of the drop-in: what createGPUSolver.H + dfLowMachFoam.C do with the reference's
// C++ classes (dfMatrixDataBase, dfRhoEqn, dfUEqn, dfYEqn, dfEEqn, dfpEqn, dfThermo) is exposed
// here as plain C entry points with pointers and sizes. All device work is stream-ordered on one
// HIP stream per context; the host synchronises only where the reference reads back to the host
// (solver residual checks, dfmi_get_field, dfmi_sync).
#include "dfmi_ctx.h"
#include "../../include/dfmi.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <numeric>

struct dfmi_ctx { dfmi::Ctx x; };

namespace {
thread_local std::string g_err;

template <class FN> int guard(FN&& fn) {
  try { fn(); return 0; }
  catch (std::exception& e) { g_err = e.what(); return 1; }
  catch (...) { g_err = "unknown error"; return 2; }
}

using namespace dfmi;

void alloc_field(Ctx& x, const std::string& name, long n, int ncomp, bool boundary, bool face = false) {
  Field& f = x.fields[name];
  f.n = n; f.ncomp = ncomp; f.boundary = boundary; f.face = face;
  f.buf.alloc((size_t)n * ncomp);
  f.buf.zero(x.stream);
}

void allocate_fields(Ctx& x) {
  const long C = x.C, B = x.B;
  const int S = x.S;
  for (auto n : {"rho", "rho_old", "p", "p_old", "he", "T", "K", "K_old", "psi", "mu", "alpha", "dpdt", "rAU",
                 "diffAlphaD", "psip0"}) {
    alloc_field(x, n, C, 1, false);
    alloc_field(x, std::string("boundary_") + n, B, 1, true);
  }
  for (auto n : {"U", "U_old", "HbyA", "hDiffCorrFlux", "sumYDiffError"}) {
    alloc_field(x, n, C, 3, false);
    alloc_field(x, std::string("boundary_") + n, B, 3, true);
  }
  alloc_field(x, "tauU", C, 9, false);
  alloc_field(x, "chem_stats", C, 3, false);   // per cell: accepted / rejected integrator steps, next step size
  alloc_field(x, "Qdot", C, 1, false);         // heat release -sum_i hc_i RR_i [W/m^3] (dfChemistryModel.C:771)
  alloc_field(x, "boundary_tauU", B, 9, true);
  alloc_field(x, "boundary_heGradient", B, 1, true);   // gradientEnergy patches (dfEEqn.cu:266-287)
  // mixed conditions: p's waveTransmissive valueFraction (set at each pEqn assembly) and gamma; the
  // inletValue of every field that may use inletOutlet
  alloc_field(x, "boundary_p_vf", B, 1, true);
  alloc_field(x, "boundary_p_gamma", B, 1, true);
  alloc_field(x, "boundary_U_ref", B, 3, true);
  alloc_field(x, "boundary_p_ref", B, 1, true);
  alloc_field(x, "boundary_Y_ref", B, S, true);
  alloc_field(x, "boundary_K_ref", B, 1, true);
  for (auto n : {"Y", "rhoD", "hai", "RR"}) {
    alloc_field(x, n, C, S, false);
    alloc_field(x, std::string("boundary_") + n, B, S, true);
  }
  for (auto n : {"phi", "phi_old", "phiUc", "rhorAUf", "phiHbyA"}) {
    alloc_field(x, n, x.Fs, 1, false, true);
    alloc_field(x, std::string("boundary_") + n, B, 1, true);
  }
  const long Fs = x.Fs;
  auto mk = [&](Matrix& A, int ns, int nsrc, int nb) {
    A.nsys = ns;
    A.lower.alloc((size_t)ns * Fs); A.upper.alloc((size_t)ns * Fs); A.diag.alloc((size_t)ns * C);
    A.source.alloc((size_t)nsrc * C); A.ic.alloc((size_t)nb * B); A.bc.alloc((size_t)nb * B);
    A.lower.zero(x.stream); A.upper.zero(x.stream); A.diag.zero(x.stream); A.source.zero(x.stream);
    A.ic.zero(x.stream); A.bc.zero(x.stream);
  };
  mk(x.mU, 1, 3, 3);
  x.mU.source_solve.alloc(3 * C);
  mk(x.mY, S, S, S);
  mk(x.mE, 1, 1, 1);
  mk(x.mP, 1, 1, 1);
  for (auto e : {"U", "Y", "E"}) if (!x.solver.count(e)) x.solver[e] = SolverCfg{20, 1e-5, 0.0};   // amgxUOptions
  if (!x.solver.count("p")) x.solver["p"] = SolverCfg{1000, 1e-5, 0.0, 1};   // amgxpOptions: AMG-preconditioned
}

// LES (options les.*): the filter width and the eddy viscosity dfmi_turbulence_correct forms. Allocated when the mode,
// one of these fields or nut's patch types is first touched: a laminar context allocates what it always did, so its
// buffers sit where they sat (the headline step is sensitive to that: profiles/les_ab.json)
// dynamicSmagorinsky (les.model = 5) alone: S and its non-coupled slots, the two contractions with their halo slots, and
// the get-only results. Allocated on the first use of model 5: every other context allocates what it always did.
void ensure_dyn_fields(Ctx& x) {
  if (x.les.model != 5 || x.fields.count("les_Cs")) return;
  alloc_field(x, "les_S", x.C, 6, false);
  alloc_field(x, "boundary_les_S", x.B, 6, true);
  for (auto n : {"les_LLMM", "les_MMMM"}) {
    alloc_field(x, n, x.C, 1, false);
    alloc_field(x, std::string("boundary_") + n, x.B, 1, true);
  }
  for (auto n : {"les_Cs", "les_LM", "les_MM"}) alloc_field(x, n, x.C, 1, false);
}
void ensure_les_fields(Ctx& x) {
  if (x.fields.count("nut")) { ensure_dyn_fields(x); return; }
  DFMI_CHECK(x.have_bgeom, "call dfmi_init_constant_fields_boundary first");
  alloc_field(x, "delta", x.C, 1, false);
  alloc_field(x, "nut", x.C, 1, false);
  alloc_field(x, "boundary_nut", x.B, 1, true);
  ensure_dyn_fields(x);
}

// RAS k-epsilon (options ras.*): k, epsilon and their slots, the inletValue of both, G and divU, the solved (pre-bound)
// copies bound() gathers from, the per-cell sources and diffusivity, and the scalar assembly's matrix. Allocated when
// ras.model is first non-zero or one of these fields or their patch types is first touched: nothing in a laminar or LES
// context.
void ensure_ras_fields(Ctx& x) {
  if (x.fields.count("epsilon")) return;
  ensure_les_fields(x);
  const long C = x.C, B = x.B;
  for (auto n : {"k", "epsilon", "k_prebound", "epsilon_prebound", "ras_D"}) {
    alloc_field(x, n, C, 1, false);
    alloc_field(x, std::string("boundary_") + n, B, 1, true);
  }
  for (auto n : {"G", "divU", "ras_Su", "ras_Sp"}) alloc_field(x, n, C, 1, false);
  alloc_field(x, "boundary_k_ref", B, 1, true);
  alloc_field(x, "boundary_epsilon_ref", B, 1, true);
  Matrix& A = x.mK;
  A.nsys = 1;
  A.lower.alloc((size_t)x.Fs); A.upper.alloc((size_t)x.Fs); A.diag.alloc((size_t)C); A.source.alloc((size_t)C);
  A.ic.alloc((size_t)B); A.bc.alloc((size_t)B);
  A.lower.zero(x.stream); A.upper.zero(x.stream); A.diag.zero(x.stream); A.source.zero(x.stream);
  A.ic.zero(x.stream); A.bc.zero(x.stream);
  for (auto e : {"k", "epsilon"}) if (!x.solver.count(e)) x.solver[e] = SolverCfg{20, 1e-5, 0.0};
}
// Wall functions and turbulent inlets: the per-patch parameters with the wall function's defaults and the
// get-only boundary_yPlus, when one of the four patch types, one of their parameters or that field is first touched. The
// device tables follow in ras_wall_refresh, and only once a patch carries one of the types (Ctx::wf.in_use).
void ensure_wall_params(Ctx& x) {   // host only: a parameter set on a context without the patch types allocates nothing
  if ((int)x.wf.Cmu.size() == x.P) return;
  x.wf.Cmu.assign(x.P, 0.09); x.wf.kappa.assign(x.P, 0.41); x.wf.E.assign(x.P, 9.8);
  x.wf.intensity.assign(x.P, 0.0); x.wf.mixingLength.assign(x.P, 0.0);
}
void ensure_wall_fields(Ctx& x) {
  ensure_wall_params(x);
  if (x.fields.count("boundary_yPlus")) return;
  ensure_ras_fields(x);
  alloc_field(x, "boundary_yPlus", x.B, 1, true);
}
// Equation of state (dfmi_thermo_set_eos): the thermo's own density, OpenFOAM's thermo.rho_. Allocated when an equation of
// state, or the field itself, is first touched: an ideal-gas context allocates what it always did.
void ensure_eos_fields(Ctx& x) {
  if (x.fields.count("rho_thermo")) return;
  DFMI_CHECK(x.have_sizes, "call dfmi_set_constant_values first");
  alloc_field(x, "rho_thermo", x.C, 1, false);
  alloc_field(x, "boundary_rho_thermo", x.B, 1, true);
}
// flareFGM (options fgm.*): the six transported scalars, what the retrieval writes beside the thermo fields,
// the transport's diffusivity and source, and the thermo's own density (rho_thermo). Allocated when fgm.model is first
// non-zero, a table is set, or one of these fields or their patch types is first touched: nothing in an FGM-free context.
// Wt, Cp and Hf start at the reference's initial values (baseFGM.C:62, 75, 125); omega_Yi has one component per source
// species of the table (one before a table is set).
const char* const kFgmFields[] = {"Z", "Zvar", "c", "cvar", "Zcvar", "Ha", "chi_Z", "chi_Zc", "chi_c", "omega_c", "cOmega_c",
                                  "ZOmega_c", "Ha_s", "c_s", "Zvar_s", "cvar_s", "Zcvar_s", "Wt", "Cp", "Hf", "fgm_D"};
bool fgm_name(const std::string& n) {
  const std::string b = n.rfind("boundary_", 0) == 0 ? n.substr(9) : n;
  for (const char* s : kFgmFields) if (b == s) return true;
  return b == "omega_Yi" || n == "fgm_Su";
}
void fill_field(Ctx& x, const std::string& name, double v) {
  Field& f = x.fields.at(name);
  std::vector<double> h((size_t)f.n * f.ncomp, v);
  DFMI_HIP(hipMemcpyAsync(f.buf.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, x.stream));
  DFMI_HIP(hipStreamSynchronize(x.stream));
}
void ensure_fgm_fields(Ctx& x) {
  const int no = std::max(x.fgm.NYomega, 1);
  if (x.fields.count("Zcvar")) {
    if (x.fields.at("omega_Yi").ncomp != no) {   // a table with another NYomega
      alloc_field(x, "omega_Yi", x.C, no, false);
      alloc_field(x, "boundary_omega_Yi", x.B, no, true);
    }
    return;
  }
  DFMI_CHECK(x.have_bgeom, "call dfmi_init_constant_fields_boundary first");
  ensure_ras_fields(x);
  ensure_eos_fields(x);
  for (const char* n : kFgmFields) {
    alloc_field(x, n, x.C, 1, false);
    alloc_field(x, std::string("boundary_") + n, x.B, 1, true);
  }
  alloc_field(x, "omega_Yi", x.C, no, false);
  alloc_field(x, "boundary_omega_Yi", x.B, no, true);
  alloc_field(x, "fgm_Su", x.C, 1, false);
  alloc_field(x, "fgm_Sp", x.C, 1, false);   // stays zero: no implicit source in any of the six equations
  for (const char* pre : {"", "boundary_"}) {
    fill_field(x, std::string(pre) + "Wt", 28.96);
    fill_field(x, std::string(pre) + "Cp", 1010.1);
    fill_field(x, std::string(pre) + "Hf", 1907.0);
  }
  for (int e = 0; e < FGM_NEQ; ++e) if (!x.solver.count(fgm_eq_name(e))) x.solver[fgm_eq_name(e)] = SolverCfg{20, 1e-5, 0.0};
}
// Spray coupling (options spray.*): the cloud's five transfer fields, cell fields without boundary
// counterparts. Allocated (zeroed) when spray.model is first 1 or one of them is first touched: nothing in a context that
// never mentions spray.
int spray_index(const std::string& n) {
  for (int i = 0; i < 5; ++i) if (n == spray_field_name(i)) return i;
  return -1;
}
void ensure_spray_fields(Ctx& x) {
  if (x.fields.count("parcel_rhoTrans")) return;
  DFMI_CHECK(x.have_sizes, "call dfmi_set_constant_values first");
  alloc_field(x, "parcel_rhoTrans", x.C, x.S, false);
  alloc_field(x, "parcel_UTrans", x.C, 3, false);
  for (auto n : {"parcel_UCoeff", "parcel_hsTrans", "parcel_hsCoeffByCp"}) alloc_field(x, n, x.C, 1, false);
}
bool tci_name(const std::string& n) {
  for (const char* s : {"tci_kappa", "tci_tmix", "tci_tauStar", "tci_tc", "RR_eff", "Qdot_eff"}) if (n == s) return true;
  return false;
}
bool ras_name(const std::string& n) {
  static const char* names[] = {"k", "epsilon", "boundary_k", "boundary_epsilon", "G", "divU", "k_prebound", "epsilon_prebound",
                                "boundary_k_prebound", "boundary_epsilon_prebound", "boundary_k_ref", "boundary_epsilon_ref"};
  for (const char* s : names) if (n == s) return true;
  return false;
}

// Build the deterministic gather topology from owner/neighbour and the boundary face cells.
void build_boundary_topology(Ctx& x) {
  const int C = x.C, B = x.B;
  x.poff.assign(x.P + 1, 0);
  std::vector<int> slot_patch(B, -1);
  std::vector<int8_t> prim(B, 0);
  int off = 0;
  for (int p = 0; p < x.P; ++p) {
    x.poff[p] = off;
    const int n = x.psize[p];
    const int slots = x.pkind[p] == 2 ? 2 * n : n;
    for (int i = 0; i < slots; ++i) { slot_patch[off + i] = p; prim[off + i] = i < n; }
    off += slots;
  }
  x.poff[x.P] = off;
  DFMI_CHECK(off == B, "patch sizes / kinds do not add up to num_boundary_surfaces");
  std::vector<int> partner(B, -1);
  for (int p = 0; p < x.P; ++p) {
    if (x.pkind[p] != 1) continue;
    const int q = x.cyc_nbr.empty() ? -1 : x.cyc_nbr[p];
    DFMI_CHECK(q >= 0 && q < x.P && x.psize[q] == x.psize[p], "cyclic patch without a matching neighbour patch");
    for (int i = 0; i < x.psize[p]; ++i) partner[x.poff[p] + i] = x.h_bfc[x.poff[q] + i];
  }
  std::vector<int> cnt(C + 1, 0);
  for (int b = 0; b < B; ++b) if (prim[b]) {
    const int c = x.h_bfc[b];
    DFMI_CHECK(c >= 0 && c < C, "boundary face cell out of range");
    cnt[c + 1]++;
  }
  for (int c = 0; c < C; ++c) cnt[c + 1] += cnt[c];
  std::vector<int> slot(cnt[C]), pos(cnt.begin(), cnt.end() - 1);
  for (int b = 0; b < B; ++b) if (prim[b]) slot[pos[x.h_bfc[b]]++] = b;
  x.cbStart.upload(cnt, x.stream);
  x.cbSlot.upload(slot.empty() ? std::vector<int>{0} : slot, x.stream);
  x.partner.upload(partner, x.stream);
  x.sprim.upload(prim.data(), prim.size(), x.stream);
  x.bfc.upload(x.h_bfc, x.stream);
}

void set_ptype(Ctx& x, const std::string& field, const int* pt) {
  std::vector<int> v(pt, pt + x.P);
  x.ptype[field] = v;
  std::vector<int8_t> s(x.B, EMPTY);
  for (int p = 0; p < x.P; ++p) {
    const int slots = x.pkind[p] == 2 ? 2 * x.psize[p] : x.psize[p];
    for (int i = 0; i < slots; ++i) s[x.poff[p] + i] = (int8_t)bc_ras_device(pt[p]);
  }
  x.stype[field].upload(s.data(), s.size(), x.stream);
}

void copy_field(Ctx& x, const std::string& name, const double* host, long count, int layout, bool to_dev) {
  auto it = x.fields.find(name);
  DFMI_CHECK(it != x.fields.end(), "unknown field '" + name + "'");
  Field& f = it->second;
  if (f.face) {   // OpenFOAM face order on the host, owner-slot storage on the device
    DFMI_CHECK(count == x.F, "field '" + name + "': expected " + std::to_string(x.F) + " values, got " + std::to_string(count));
    // component k of face i: host[k F + i], or host[i ncomp + k] (DFMI_AOS vectors); device [ncomp][Fs]
    const int nc = f.ncomp;
    const bool aos = layout == DFMI_AOS && nc == 3;
    std::vector<double> st((size_t)f.n * nc, 0.0);
    if (to_dev) {
      for (int k = 0; k < nc; ++k)
        for (long i = 0; i < x.F; ++i) st[k * f.n + x.h_fst[i]] = aos ? host[i * nc + k] : host[k * x.F + i];
      DFMI_HIP(hipMemcpyAsync(f.buf.p, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, x.stream));
      DFMI_HIP(hipStreamSynchronize(x.stream));
    } else {
      DFMI_HIP(hipMemcpyAsync(st.data(), f.buf.p, st.size() * sizeof(double), hipMemcpyDeviceToHost, x.stream));
      DFMI_HIP(hipStreamSynchronize(x.stream));
      double* out = const_cast<double*>(host);
      for (int k = 0; k < nc; ++k)
        for (long i = 0; i < x.F; ++i) (aos ? out[i * nc + k] : out[k * x.F + i]) = st[k * f.n + x.h_fst[i]];
    }
    return;
  }
  DFMI_CHECK(count == f.n, "field '" + name + "': expected " + std::to_string(f.n) + " values per component, got " +
                               std::to_string(count));
  const size_t tot = (size_t)f.n * f.ncomp;
  const bool perm = layout == DFMI_AOS && (f.ncomp == 3 || f.ncomp == 9);
  std::vector<double> tmp;
  if (to_dev) {
    const double* src = host;
    if (perm) {
      tmp.resize(tot);
      for (long i = 0; i < f.n; ++i) for (int k = 0; k < f.ncomp; ++k) tmp[(size_t)k * f.n + i] = host[i * f.ncomp + k];
      src = tmp.data();
    }
    DFMI_HIP(hipMemcpyAsync(f.buf.p, src, tot * sizeof(double), hipMemcpyHostToDevice, x.stream));
    DFMI_HIP(hipStreamSynchronize(x.stream));
  } else {
    double* dst = const_cast<double*>(host);
    if (perm) { tmp.resize(tot); dst = tmp.data(); }
    DFMI_HIP(hipMemcpyAsync(dst, f.buf.p, tot * sizeof(double), hipMemcpyDeviceToHost, x.stream));
    DFMI_HIP(hipStreamSynchronize(x.stream));
    if (perm) {
      double* out = const_cast<double*>(host);
      for (long i = 0; i < f.n; ++i) for (int k = 0; k < f.ncomp; ++k) out[i * f.ncomp + k] = tmp[(size_t)k * f.n + i];
    }
  }
}

void require_ready(Ctx& x) {
  DFMI_CHECK(x.have_sizes && x.have_topo && x.have_geom && x.have_bgeom, "mesh not fully initialised");
  x.co.fresh = false;   // every entry that may rewrite phi or rho comes through here (dfmi_time_step posts a new record)
  if (!x.ell.ready) build_ell(x);   // gather rows (face lists of the assembly kernels, solver columns)
}

void maybe_setup_halo(Ctx& x);

// The non-orthogonal geometry belongs to Sf, mesh_distance and the patch deltas as they stood when it was formed: an
// initialiser that is called again re-forms it, or, where what it needs is gone (no mesh_distance any more), puts the
// laplacian scheme back to orthogonal
void nonorth_refresh(Ctx& x) {
  if (!x.no_dc) return;
  bool coupled = false;
  for (int p = 0; p < x.P; ++p) coupled |= x.pkind[p] != 0;
  if (x.have_geom && x.have_bgeom && x.have_md && (!coupled || x.have_bdelta)) {
    nonorth_setup(x);
    DFMI_HIP(hipStreamSynchronize(x.stream));
  } else {
    x.lap = LAP_ORTHOGONAL;
    x.no_dc = x.no_bdc = x.no_k = x.no_bk = nullptr;
  }
}

// ---- equation drivers
void do_U(Ctx& x) {
  u_assemble(x);
  Matrix& A = x.mU;
  solve_bicgstab(x, "U", 3, nullptr, A.lower, 0, A.upper, 0, A.diag, 0, A.source_solve, x.C, A.ic, A.bc, x.B, "U",
                 x.f("U"), x.C, x.solver["U"]);
  u_post_solve(x);
}
// YEqn up to its assembled rows: the chemistry source, the preparation terms and the rows (no host
// synchronisation inside, so dfmi_time_step can issue it on the side stream beside the UEqn)
// weights = false: the div(phi,Yi_h) weights are formed elsewhere (do_U_Y_fork) and `rows_after` (if set) is the
// event the rows wait for on this stream
void do_Y_front(Ctx& x, bool weights = true, hipEvent_t rows_after = nullptr) {
  DFMI_CHECK(x.inert >= 0 && x.inert < x.S, "inert species index not set");
  YWs _yw(x);
  // chemistry->solve(deltaT) before YEqn (YEqn.H); the thermo density of that call is rho before this
  // step's rhoEqn, i.e. rho_old (dfChemistryModel.C:87,771; the GPU reference passes d_rho_old, dfYEqn.cu:449)
  // (combustion->correct(), YEqn.H:76: with a closure in force -- options tci.* -- the solve, kappa and the scaled source)
  if (x.chem.mode == 1) combustion_correct(x, 1.0 / x.rdt, "rho_old");
  else if (x.chem.mode == 2) dnn_solve(x, "rho_old");   // chemistrySolver_GPU.Inference (YEqn_GPU.H)
  y_prep(x, weights);
  if (rows_after) DFMI_HIP(hipStreamWaitEvent(x.stream, rows_after, 0));
  // production path: the assembly writes the solver's ELL rows directly (no LDU round trip)
  double *val, *dS, *rhs;
  bicg_layout(x, x.S - 1, &val, &dS, &rhs);
  y_assemble_ell(x, x.ell.W, (long)x.C + x.H, val, dS, rhs);
}
void do_Y_back(Ctx& x) {
  YWs _yw(x);
  Matrix& A = x.mY;
  std::vector<int> map;
  for (int s = 0; s < x.S; ++s) if (s != x.inert) map.push_back(s);
  solve_bicgstab(x, "Y", (int)map.size(), map.data(), A.lower, x.Fs, A.upper, x.Fs, A.diag, x.C, A.source, x.C, A.ic,
                 A.bc, x.B, "Y", x.f("Y"), x.C, x.solver["Y"], true);
  y_post_solve(x);
}
void do_Y(Ctx& x) {
  do_Y_front(x);
  do_Y_back(x);
}

// The chemistry and the YEqn preparation/assembly read nothing the UEqn writes (T, p, Y, rho_old, phi, the
// thermo's transport from the last correctThermo) and the UEqn nothing they write, so they run on the side stream
// while the UEqn assembles and solves on the main one: the VALU-bound chemistry beside the memory-bound UEqn. Both
// are issued before the UEqn's convergence polls block the host. With several ranks the side stream's field halos
// (the YEqn preparation's sumYDiffError / hDiffCorrFlux, the EEqn scheme terms' gradients) go through the halo's
// second channel -- its own RCCL communicator and buffers (halo.hip) -- so the two streams' exchanges never
// interleave on one communicator; the chemistry needs no halo at all. DFMI_STEP_OVERLAP=0: off.
// While per-kernel timers are armed (dfmi_kernel_timer: the bench's roofline pass) the step runs on one
// stream, so every timed kernel has the GPU to itself and its HIP-event time is its own.
bool step_overlap(const Ctx& x) {
  static const bool on = [] { const char* e = std::getenv("DFMI_STEP_OVERLAP"); return !(e && std::atoi(e) == 0); }();
  return on && x.ktimer.targets.empty();
}
// the side stream forks from the main one and runs the YEqn front; ev_join marks its end. The side stream is the
// longer of the two (chemistry, preparation, rows against the UEqn), so the div(phi,Yi_h) weights (they read phi,
// Y, he only) run on the main stream ahead of the UEqn and the side stream waits for them just before the rows
// (the step timeline had the main stream idle for ~1 ms at the join)
void do_U_Y_fork(Ctx& x) {
  if (!x.stream2) {
    DFMI_HIP(hipStreamCreateWithFlags(&x.stream2, hipStreamNonBlocking));
    for (hipEvent_t* e : {&x.ev_fork, &x.ev_join, &x.ev_u, &x.ev_e, &x.ev_cw})
      DFMI_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  DFMI_HIP(hipEventRecord(x.ev_fork, x.stream));
  DFMI_HIP(hipStreamWaitEvent(x.stream2, x.ev_fork, 0));
  // the weights' event is recorded on the main stream right after the weights, before the side stream's
  // hipStreamWaitEvent on it is issued (inside do_Y_front: a wait binds to the event's most recent record at call
  // time, so the record must come first); the side stream's chemistry and preparation do not wait for it
  conv_weights(x);
  // (the YEqn preparation on the main stream ahead of the UEqn instead, the side stream holding the chemistry and the
  // rows only: 14.02 / 14.05 -> 14.52 / 14.40 ms per step, round 6 -- not kept)
  DFMI_HIP(hipEventRecord(x.ev_cw, x.stream));
  OnStream _os(x, x.stream2);
  do_Y_front(x, false, x.ev_cw);
  DFMI_HIP(hipEventRecord(x.ev_join, x.stream2));
}
void do_E_back(Ctx& x) {
  Matrix& A = x.mE;
  solve_bicgstab(x, "E", 1, nullptr, A.lower, 0, A.upper, 0, A.diag, 0, A.source, 0, A.ic, A.bc, 0, "he", x.f("he"), 0,
                 x.solver["E"]);
  e_post_solve(x);
}
void do_E(Ctx& x) {
  e_assemble(x);
  do_E_back(x);
}
// UEqn, YEqn, EEqn with the overlap above and one more: the EEqn scheme terms (K's limited weights from the
// UEqn's K, the cubic correction of hDiffCorrFlux from the YEqn preparation) read nothing the Y solve writes,
// so they run on the side stream after both while the main stream solves the species; the rest of the
// assembly needs the solved Y (the thermo's boundary energy gradient) and follows the Y solve
// and a third: between the U solve and the join the main stream waits for the side stream's YEqn rows (about 0.55 ms
// on the headline, k_y_assemble_ell running alone), so the first pressure corrector's HbyA is issued there (hbya:
// step.hbya_early) -- it reads U, the U matrix and rAU as the U solve left them, none of which the Y or E equations or
// correctThermo write, and nothing else reads or writes HbyA before the corrector
void do_U_Y_E(Ctx& x, bool hbya = false) {
  if (!step_overlap(x)) { do_U(x); do_Y(x); do_E(x); return; }
  do_U_Y_fork(x);
  do_U(x);
  DFMI_HIP(hipEventRecord(x.ev_u, x.stream));
  {
    OnStream _os(x, x.stream2);
    DFMI_HIP(hipStreamWaitEvent(x.stream2, x.ev_u, 0));
    e_assemble_front(x);
    DFMI_HIP(hipEventRecord(x.ev_e, x.stream2));
  }
  if (hbya) u_hbya(x);
  DFMI_HIP(hipStreamWaitEvent(x.stream, x.ev_join, 0));
  do_Y_back(x);
  DFMI_HIP(hipStreamWaitEvent(x.stream, x.ev_e, 0));
  e_assemble_back(x);
  do_E_back(x);
}
// pEqn.H:51-62, while (pimple.correctNonOrthogonal()): the matrix is assembled once; each of the 1 + p.n_nonorth passes
// forms the explicit non-orthogonal term from p as it stands (corrected only) and solves. The last pass's face flux
// correction enters phi = phiHbyA + pEqn.flux(). The solver's fused setup (pcg.fuse_setup) is bypassed here: the
// source is re-formed between the cell pass and every solve.
void do_p_nonorth(Ctx& x, int n_nonorth) {
  const bool corr = x.lap == LAP_CORRECTED;
  p_assemble(x, true);
  Matrix& A = x.mP;
  if (corr) nonorth_p_base(x);
  for (int i = 0; i <= n_nonorth; ++i) {
    if (corr) nonorth_p_correct(x);
    solve_pcg(x, "p", A.lower, A.upper, A.diag, A.source, A.ic, A.bc, "p", x.f("p"), x.f("boundary_p"), x.solver["p"],
              false);
    if (i < n_nonorth) {   // the next pass's gradient reads p's boundary values
      k_bc_correct(x, "p", x.f("p"), x.f("boundary_p"), 1);
      halo_fields(x, {"p"});
    }
  }
  p_post_solve(x);
  if (corr) nonorth_p_flux(x);
}
void do_p(Ctx& x) {
  const int n_nonorth = (int)x.opt("p.n_nonorth");
  if (x.lap == LAP_CORRECTED || n_nonorth > 0) { do_p_nonorth(x, n_nonorth); return; }
  // face-form PCG with the reused V-cycle: the solver's setup kernel does the cell pass too (pcg.fuse_setup)
  const bool fuse = pcg_setup_fusable(x, x.solver["p"]);
  p_assemble(x, !fuse);
  Matrix& A = x.mP;
  solve_pcg(x, "p", A.lower, A.upper, A.diag, A.source, A.ic, A.bc, "p", x.f("p"), x.f("boundary_p"), x.solver["p"],
            fuse);
  p_post_solve(x);
}
// kEpsilon::correct() (include/dfmi.h): G and divU, the epsilon equation, bound, the k equation with the new epsilon,
// bound, correctNut(). Everything on the context stream: it runs after the pressure correctors, beside nothing.
void ras_solve(Ctx& x, int keq) {
  const char* nm = keq ? "k" : "epsilon";
  Matrix& A = x.mK;
  ras_assemble(x, keq);
  solve_bicgstab(x, nm, 1, nullptr, A.lower, 0, A.upper, 0, A.diag, 0, A.source, 0, A.ic, A.bc, 0, nm, x.f(nm), 0, x.solver[nm]);
  ras_post_solve(x, keq);
}
void ras_correct(Ctx& x) {
  ensure_ras_fields(x);
  // wall functions and turbulent inlets (nothing without their patch types): k's inletValue first, then
  // after G and divU the wall cells' epsilon and G, the constraint flags and epsilon's inletValue
  ras_inlet_k(x);
  ras_production(x);
  ras_wall_update(x);
  ras_solve(x, 0);
  ras_solve(x, 1);
  ras_nut(x);
}
// flareFGM::correct() (include/dfmi.h, flareFGM block): the transport equations in baseFGM::transport()'s order, each
// assembled from the fields as they stand, solved, boundary-corrected, exchanged and clipped; Ha; the retrieval.
void fgm_solve(Ctx& x, int eq) {
  const char* nm = fgm_eq_name(eq);
  Matrix& A = x.mK;
  fgm_assemble(x, eq);
  solve_bicgstab(x, nm, 1, nullptr, A.lower, 0, A.upper, 0, A.diag, 0, A.source, 0, A.ic, A.bc, 0, nm, x.f(nm), 0, x.solver[nm]);
  fgm_post_solve(x, eq);
}
// what flareFGM needs of the context, refused by name
void fgm_check(Ctx& x, const char* who) {
  const std::string w = std::string(who) + ": ";
  DFMI_CHECK(x.fgm.have_table, w + "no flamelet table set (dfmi_fgm_set_table)");
  DFMI_CHECK(x.ras.model == 1, w + "flareFGM needs ras.model = 1 (the retrieval divides by k)");
  DFMI_CHECK(!x.les.model, w + "flareFGM with les.model != 0 is not available (magUPrime needs an LESfilter)");
  DFMI_CHECK(!x.tci.model, w + "flareFGM and tci.model != 0 exclude each other (one combustion model at a time)");
  DFMI_CHECK(x.chem.mode == 0, w + "flareFGM with chemistry mode != 0 is not available (the table replaces the chemistry)");
  DFMI_CHECK(!x.thermo.eos, w + "flareFGM with an equation of state set (dfmi_thermo_set_eos model 1) is not available");
  ensure_fgm_fields(x);
  for (int e = 0; e < FGM_NEQ; ++e)
    DFMI_CHECK(x.stype.count(fgm_eq_name(e)), w + "patch types not set for field '" + fgm_eq_name(e) + "' (dfmi_set_patch_types)");
  static const char* names[4] = {"k", "epsilon", "boundary_k", "boundary_epsilon"};
  for (int i = 0; i < 4; ++i) DFMI_CHECK(x.ras.have[i], w + "the field '" + names[i] + "' is not set (dfmi_set_field)");
}
// several ranks: the neighbour half of the six scalars' processor slots as the caller set them (the gradients and the
// limiter read the cell across a processor face; later calls find what fgm_post_solve left)
void fgm_halo(Ctx& x) { halo_fields(x, {"Z", "Zvar", "c", "cvar", "Zcvar", "Ha"}); }
void fgm_correct(Ctx& x) {
  fgm_check(x, "dfmi_fgm_correct");
  fgm_halo(x);
  if (!x.ras.valid) ras_nut(x);   // mut = rho nut of k and epsilon as they stand
  fgm_solve(x, 0);
  fgm_solve(x, 1);
  if (x.on("fgm.combustion")) { fgm_solve(x, 2); fgm_solve(x, 3); fgm_solve(x, 4); }
  if (x.on("fgm.solveEnthalpy")) fgm_solve(x, 5);
  else fgm_ha_from_z(x);
  fgm_retrieve(x, true);
}
// step.hbya_early applies: the two-stream step on one rank (several ranks keep today's order: HbyA's field halo
// stays behind the Y and E solves' exchanges)
bool hbya_early(const Ctx& x) {
  return step_overlap(x) && x.nranks == 1 && !halo_active(x) && x.on("step.hbya_early");
}

}  // namespace

extern "C" {

const char* dfmi_version(void) { return "dfmi 0.1 (gfx950)"; }

int dfmi_last_error(char* buf, int len) {
  if (buf && len > 0) std::snprintf(buf, len, "%s", g_err.c_str());
  return (int)g_err.size();
}

int dfmi_create(dfmi_ctx** out, int device) {
  return guard([&] {
    DFMI_CHECK(out, "null output pointer");
    int n = 0;
    DFMI_HIP(hipGetDeviceCount(&n));
    DFMI_CHECK(device >= 0 && device < n, "device " + std::to_string(device) + " not available (" + std::to_string(n) + " devices)");
    DFMI_HIP(hipSetDevice(device));
    auto* c = new dfmi_ctx();
    c->x.device = device;
    DFMI_HIP(hipStreamCreateWithFlags(&c->x.stream, hipStreamNonBlocking));
    *out = c;
  });
}

int dfmi_destroy(dfmi_ctx* ctx) {
  return guard([&] {
    if (!ctx) return;
    DFMI_HIP(hipSetDevice(ctx->x.device));
    (void)hipStreamSynchronize(ctx->x.stream);
    hipStream_t s = ctx->x.stream;
    delete ctx;
    (void)hipStreamDestroy(s);
  });
}

int dfmi_set_constant_values(dfmi_ctx* ctx, int num_cells, int num_total_cells, int num_surfaces,
                             int num_boundary_surfaces, int num_patches, int num_proc_surfaces,
                             const int* patch_size, int num_species, double rdelta_t) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(num_cells > 0 && num_surfaces >= 0 && num_boundary_surfaces >= 0 && num_patches >= 0, "bad sizes");
    // the FV kernels are instantiated for 2..16 species (a larger count fails there, loudly); the DNN
    // surrogate path alone runs up to 64 (BASELINE config 4: GRI-53)
    DFMI_CHECK(num_species >= 2 && num_species <= 64, "num_species must be in [2,64]");
    DFMI_CHECK(rdelta_t > 0, "rdelta_t must be positive");
    x.C = num_cells; x.Ctot = num_total_cells; x.F = num_surfaces; x.B = num_boundary_surfaces; x.P = num_patches;
    x.nproc_faces = num_proc_surfaces; x.S = num_species; x.rdt = rdelta_t; x.dt = 1.0 / rdelta_t;
    x.co.fresh = false;
    x.psize.assign(patch_size, patch_size + num_patches);
    x.pkind.assign(num_patches, 0);
    x.cyc_nbr.assign(num_patches, -1);
    x.peer.assign(num_patches, -1);
    x.have_sizes = true;
  });
}

int dfmi_set_cyclic_info(dfmi_ctx* ctx, const int* cyclic_neighbor) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_sizes, "call dfmi_set_constant_values first");
    x.cyc_nbr.assign(cyclic_neighbor, cyclic_neighbor + x.P);
  });
}

int dfmi_set_constant_indexes(dfmi_ctx* ctx, const int* owner, const int* neighbour, const int* proc_rows,
                              const int* proc_cols, int global_offset) {
  (void)proc_rows;   // global CSR row ids are an AmgX concern; the halo pairs patches by procCols
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_sizes, "call dfmi_set_constant_values first");
    x.global_offset = global_offset;
    x.h_proc_cols.assign(proc_cols, proc_cols + x.nproc_faces);
    const int C = x.C, F = x.F;
    x.h_own.assign(owner, owner + F);
    x.h_nei.assign(neighbour, neighbour + F);
    std::vector<int> ownStart(C + 1, 0), nbrCnt(C + 1, 0);
    for (int f = 0; f < F; ++f) {
      const int o = owner[f], n = neighbour[f];
      DFMI_CHECK(o >= 0 && o < C && n >= 0 && n < C && o < n, "face " + std::to_string(f) + ": owner/neighbour out of range or owner >= neighbour");
      DFMI_CHECK(f == 0 || owner[f - 1] < o || (owner[f - 1] == o && neighbour[f - 1] < n),
                 "faces are not in upper-triangular order (sorted by owner, then neighbour)");
      ownStart[o + 1]++;
      nbrCnt[n + 1]++;
    }
    for (int c = 0; c < C; ++c) { ownStart[c + 1] += ownStart[c]; nbrCnt[c + 1] += nbrCnt[c]; }
    // face storage: owner-slot order (k-th owned face of c at k*C + c) when at most 3 faces per cell
    // are owned or the padding stays small; OpenFOAM order otherwise
    int kmax = 0;
    for (int c = 0; c < C; ++c) kmax = std::max(kmax, ownStart[c + 1] - ownStart[c]);
    x.fslot = F > 0 && (kmax <= 3 || (long)kmax * C <= (long)F + F / 4);
    x.Fs = x.fslot ? kmax * C : F;
    x.h_fst.resize(F);
    for (int f = 0; f < F; ++f) x.h_fst[f] = x.fslot ? (f - ownStart[owner[f]]) * C + owner[f] : f;
    std::vector<int> own_s(std::max(x.Fs, 1), -1), nei_s(std::max(x.Fs, 1), -1);
    for (int f = 0; f < F; ++f) { own_s[x.h_fst[f]] = owner[f]; nei_s[x.h_fst[f]] = neighbour[f]; }
    std::vector<int> nbrFace(std::max(F, 1)), pos(nbrCnt.begin(), nbrCnt.end() - 1);
    for (int f = 0; f < F; ++f) nbrFace[pos[neighbour[f]]++] = x.h_fst[f];   // ascending face order per cell
    x.own.upload(own_s, x.stream);
    x.nei.upload(nei_s, x.stream);
    x.ownStart.upload(ownStart, x.stream);
    x.nbrStart.upload(nbrCnt, x.stream);
    x.nbrFace.upload(nbrFace, x.stream);
    DFMI_HIP(hipStreamSynchronize(x.stream));
    x.have_topo = true;
  });
}

int dfmi_init_constant_fields_internal(dfmi_ctx* ctx, const double* sf, const double* mag_sf, const double* weight,
                                       const double* delta_coeffs, const double* volume, const double* mesh_distance) {
  // mesh_distance (C[nei] - C[own]) is the d the limited schemes' limiter reads (LimitedScheme::calcLimiter);
  // the reference's GPU path uploads it for its disabled limitedLinear (dfMatrixOpBase.cu:2540-2600)
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_topo, "call dfmi_set_constant_indexes first");
    const long F = x.F, Fs = x.Fs;
    std::vector<double> soa(3 * std::max(Fs, 1L), 0.0), ms(std::max(Fs, 1L), 0.0), ww(std::max(Fs, 1L), 0.0),
        dd(std::max(Fs, 1L), 0.0), mdv(3 * std::max(Fs, 1L), 0.0);
    for (long f = 0; f < F; ++f) {   // AoS -> SoA, OpenFOAM face order -> face storage
      const long s = x.h_fst[f];
      for (int k = 0; k < 3; ++k) soa[k * Fs + s] = sf[f * 3 + k];
      if (mesh_distance) for (int k = 0; k < 3; ++k) mdv[k * Fs + s] = mesh_distance[f * 3 + k];
      ms[s] = mag_sf[f]; ww[s] = weight[f]; dd[s] = delta_coeffs[f];
    }
    x.md.upload(mdv, x.stream);
    x.Sf.upload(soa, x.stream);
    x.magSf.upload(ms, x.stream);
    x.w.upload(ww, x.stream);
    x.dc.upload(dd, x.stream);
    x.V.upload(volume, x.C, x.stream);
    x.co.sumV = 0.0;   // gSum(V) of the mean Courant number: constant, summed once, in cell order
    for (int c = 0; c < x.C; ++c) x.co.sumV += volume[c];
    DFMI_HIP(hipStreamSynchronize(x.stream));
    x.have_md = mesh_distance != nullptr;
    x.have_geom = true;
    nonorth_refresh(x);
  });
}

int dfmi_init_constant_fields_boundary(dfmi_ctx* ctx, const double* bsf, const double* bmag, const double* bdelta,
                                       const double* bweight, const int* bface_cell, const int* ptype_calc,
                                       const int* ptype_extrap) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_geom, "call dfmi_init_constant_fields_internal first");
    const long B = x.B;
    for (int p = 0; p < x.P; ++p) {
      const int t = ptype_calc[p];
      x.pkind[p] = (t == CYCLIC) ? 1 : (bc_proc(t) ? 2 : 0);
    }
    x.h_bfc.assign(bface_cell, bface_cell + B);
    std::vector<double> soa(3 * B);
    for (long b = 0; b < B; ++b) for (int k = 0; k < 3; ++k) soa[k * B + b] = bsf[b * 3 + k];
    x.bSf.upload(soa.empty() ? std::vector<double>{0.0} : soa, x.stream);
    x.bmagSf.upload(bmag, B, x.stream);
    x.bdc.upload(bdelta, B, x.stream);
    x.bw.upload(bweight, B, x.stream);
    build_boundary_topology(x);
    allocate_fields(x);
    set_ptype(x, "calculated", ptype_calc);
    set_ptype(x, "extrapolated", ptype_extrap);
    DFMI_HIP(hipStreamSynchronize(x.stream));
    x.have_bgeom = true;
    maybe_setup_halo(x);
    nonorth_refresh(x);
  });
}

int dfmi_set_patch_types(dfmi_ctx* ctx, const char* field, const int* patch_type) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_bgeom, "call dfmi_init_constant_fields_boundary first");
    std::string f(field);
    static const char* ok[] = {"U", "p", "he", "K", "Y", "T", "rho", "nut", "k", "epsilon"};
    const bool ras = f == "k" || f == "epsilon";
    const bool fgm = fgm_eq_index(f) >= 0;   // the flareFGM scalars
    DFMI_CHECK(fgm || std::find_if(std::begin(ok), std::end(ok), [&](const char* s) { return f == s; }) != std::end(ok),
               "unknown patch-type field '" + f + "'");
    for (int p = 0; p < x.P; ++p) {
      const int t = patch_type[p];
      DFMI_CHECK(t >= 0 && t <= 16 && t != COUPLED, "patch " + std::to_string(p) + ": unsupported boundary condition code " + std::to_string(t));
      if (bc_ras_new(t)) {   // the k-epsilon wall functions and turbulent inlets: one field each, plain patches only
        static const char* wname[4] = {"epsilonWallFunction", "nutkWallFunction", "turbulentIntensityKineticEnergyInlet",
                                       "turbulentMixingLengthDissipationRateInlet"};
        static const char* wfield[4] = {"epsilon", "nut", "k", "epsilon"};
        const std::string wn = wname[t - EPSILON_WALL_FUNCTION], wf = wfield[t - EPSILON_WALL_FUNCTION];
        DFMI_CHECK(f == wf, "patch " + std::to_string(p) + ": " + wn + " is a condition of the field '" + wf + "', not of '" + f + "'");
        DFMI_CHECK(x.pkind[p] == 0, "patch " + std::to_string(p) + ": " + wn + " on a " + (x.pkind[p] == 1 ? "cyclic" : "processor") + " patch");
        DFMI_CHECK(x.pt("calculated")[p] != EMPTY, "patch " + std::to_string(p) + ": " + wn + " on an empty patch");
        continue;
      }
      DFMI_CHECK(!fgm || t == ZERO_GRADIENT || t == FIXED_VALUE || t == EMPTY || t == CYCLIC || bc_proc(t),
                 "patch " + std::to_string(p) + ": " + f + " takes zeroGradient, fixedValue, cyclic, processor, processorCyclic or empty");
      DFMI_CHECK(t != WAVE_TRANSMISSIVE || f == "p", "waveTransmissive is supported for p (the 1D flame's outlet)");
      DFMI_CHECK(t != INLET_OUTLET || f == "U" || f == "p" || f == "Y" || f == "K" || ras,
                 "inletOutlet is supported for U, p, Y, K, k and epsilon (energy needs its own mixed form)");
      DFMI_CHECK(!ras || t == ZERO_GRADIENT || t == FIXED_VALUE || t == INLET_OUTLET || t == CALCULATED || t == EMPTY || t == CYCLIC || bc_proc(t),
                 "patch " + std::to_string(p) + ": " + f + " takes zeroGradient, fixedValue, inletOutlet, calculated, cyclic, processor, processorCyclic or empty");
      DFMI_CHECK((x.pkind[p] == 1) == (t == CYCLIC) && (x.pkind[p] == 2) == bc_proc(t),
                 "patch " + std::to_string(p) + ": field '" + f + "' type disagrees with the mesh patch kind");
      DFMI_CHECK(t != GRADIENT_ENERGY || f == "he", "gradientEnergy is an energy boundary condition (field 'he')");
      DFMI_CHECK(t != FIXED_ENERGY || f == "he", "fixedEnergy is an energy boundary condition (field 'he')");
      DFMI_CHECK(f != "nut" || t == ZERO_GRADIENT || t == FIXED_VALUE || t == CALCULATED || t == EMPTY || t == CYCLIC || bc_proc(t),
                 "patch " + std::to_string(p) + ": nut takes zeroGradient, fixedValue, calculated, cyclic, processor, processorCyclic or empty");
    }
    if (ras) ensure_ras_fields(x);
    if (fgm) ensure_fgm_fields(x);
    if (ras || f == "nut") {
      // nut belongs to these patch types too: a wall function's slots are formed by correctNut(). The tables are needed
      // from the first of the four codes on and are dropped with the last
      bool any = false;
      for (const char* g : {"k", "epsilon", "nut"}) {
        if (f == g) { for (int p = 0; p < x.P; ++p) any |= bc_ras_new(patch_type[p]); continue; }
        auto it = x.ptype.find(g);
        if (it != x.ptype.end()) for (int t : it->second) any |= bc_ras_new(t);
      }
      if (any) ensure_wall_fields(x);
      if (any || x.wf.in_use) { x.wf.dirty = true; if (!any) x.wf.bits = 0; }
      x.wf.in_use = any;
      x.ras.valid = false;
    }
    set_ptype(x, f, patch_type);
    DFMI_HIP(hipStreamSynchronize(x.stream));
  });
}

int dfmi_init_boundary_delta(dfmi_ctx* ctx, const double* boundary_delta) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_bgeom, "call dfmi_init_constant_fields_boundary first");
    const long B = x.B;
    std::vector<double> soa(3 * std::max(B, 1L), 0.0);
    for (long b = 0; b < B; ++b) for (int k = 0; k < 3; ++k) soa[k * B + b] = boundary_delta[b * 3 + k];
    x.bdv.upload(soa, x.stream);
    DFMI_HIP(hipStreamSynchronize(x.stream));
    x.have_bdelta = true;
    nonorth_refresh(x);
  });
}

// "limitedLinear01 1" -> (kind, k); a leading "Gauss" accepted (system/fvSchemes divSchemes syntax)
static void parse_scheme(const std::string& term, const std::string& text, int& kind, double& k) {
  std::vector<std::string> tok;
  std::string cur;
  for (char ch : text + " ") {
    if (ch == ' ' || ch == '\t') { if (!cur.empty()) tok.push_back(cur); cur.clear(); }
    else cur += ch;
  }
  if (!tok.empty() && tok[0] == "Gauss") tok.erase(tok.begin());
  DFMI_CHECK(!tok.empty(), term + ": empty scheme");
  const std::string& n = tok[0];
  k = 1.0;
  if (n == "upwind") kind = SCH_UPWIND;
  else if (n == "linear") kind = SCH_LINEAR;
  else if (n == "cubic") kind = SCH_CUBIC;
  else if (n == "limitedLinear" || n == "limitedLinear01" || n == "limitedLinearV") {
    kind = n == "limitedLinear" ? SCH_LL : n == "limitedLinear01" ? SCH_LL01 : SCH_LLV;
    DFMI_CHECK(tok.size() == 2, term + ": " + n + " needs its coefficient k");
    char* end = nullptr;
    k = std::strtod(tok[1].c_str(), &end);
    DFMI_CHECK(end && *end == 0 && k >= 0 && k <= 1, term + ": limitedLinear coefficient must be a number in [0, 1]");
    return;
  } else throw Error("dfmi: " + term + ": unsupported scheme '" + text + "'");
  DFMI_CHECK(tok.size() == 1, term + ": unexpected arguments in '" + text + "'");
}

// laplacianSchemes default: "[Gauss] [linear] orthogonal | uncorrected | corrected" (one scheme for the U, Yi, he and p
// laplacians). Everything is checked before the context changes, so a refused scheme leaves the one in force.
static void set_laplacian(Ctx& x, const std::string& text) {
  std::vector<std::string> tok;
  std::string cur;
  for (char ch : text + " ") {
    if (ch == ' ' || ch == '\t') { if (!cur.empty()) tok.push_back(cur); cur.clear(); }
    else cur += ch;
  }
  if (!tok.empty() && tok[0] == "Gauss") tok.erase(tok.begin());
  if (!tok.empty() && tok[0] == "linear") tok.erase(tok.begin());
  DFMI_CHECK(!tok.empty(), "laplacian: empty scheme");
  DFMI_CHECK(tok[0] != "limited", "laplacian: the snGrad scheme 'limited' is not supported (orthogonal, uncorrected or corrected)");
  const int lap = tok[0] == "orthogonal" ? LAP_ORTHOGONAL : tok[0] == "uncorrected" ? LAP_UNCORRECTED
                  : tok[0] == "corrected" ? LAP_CORRECTED : -1;
  DFMI_CHECK(lap >= 0, "laplacian: unsupported scheme '" + text + "' (orthogonal, uncorrected or corrected)");
  DFMI_CHECK(tok.size() == 1, "laplacian: unexpected arguments in '" + text + "'");
  if (lap != LAP_ORTHOGONAL) {
    bool coupled = false;
    for (int p = 0; p < x.P; ++p) coupled |= x.pkind[p] != 0;
    DFMI_CHECK(x.have_md, "laplacian " + tok[0] + " needs mesh_distance (dfmi_init_constant_fields_internal)");
    DFMI_CHECK(!coupled || x.have_bdelta, "laplacian " + tok[0] + " on a mesh with coupled patches needs dfmi_init_boundary_delta");
    if (!x.no_dc) { nonorth_setup(x); DFMI_HIP(hipStreamSynchronize(x.stream)); }   // the geometry is formed once
  }
  x.lap = lap;
}

int dfmi_set_scheme(dfmi_ctx* ctx, const char* term, const char* scheme) {
  return guard([&] {
    Ctx& x = ctx->x;
    // the patch kinds (processor patches) are known only after the boundary initialisation
    DFMI_CHECK(x.have_bgeom, "call dfmi_init_constant_fields_boundary before dfmi_set_scheme");
    const std::string t(term ? term : ""), s(scheme ? scheme : "");
    if (t == "laplacian") { set_laplacian(x, s); return; }
    int kind;
    double k;
    parse_scheme(t, s, kind, k);
    if (t == "div(phi,Yi_h)") {
      DFMI_CHECK(kind == SCH_UPWIND || kind == SCH_LL || kind == SCH_LL01, t + ": upwind, limitedLinear or limitedLinear01");
      x.sch.yh = kind; x.sch.k_yh = k;
    } else if (t == "div(phi,K)") {
      DFMI_CHECK(kind != SCH_CUBIC, t + ": upwind, linear, limitedLinear or limitedLinear01");
      x.sch.K = kind; x.sch.k_K = k;
    } else if (t == "div(hDiffCorrFlux)") {
      DFMI_CHECK(kind == SCH_LINEAR || kind == SCH_CUBIC, t + ": linear or cubic");
      x.sch.hD = kind;
    } else if (t == "div(phi,U)") {
      DFMI_CHECK(kind == SCH_LINEAR || kind == SCH_LLV, t + ": linear or limitedLinearV");
      bool proc = false;
      for (int p : x.pkind) proc |= p == 2;
      DFMI_CHECK(kind == SCH_LINEAR || !proc, t + ": limited schemes on decomposed meshes (processor patches) are not supported");
      x.sch.U = kind; x.sch.k_U = k;
    } else if (t == "div(phi,k)" || t == "div(phi,epsilon)") {
      DFMI_CHECK(kind == SCH_UPWIND || kind == SCH_LINEAR || kind == SCH_LL, t + ": upwind, limitedLinear or linear");
      if (t == "div(phi,k)") { x.sch.tk = kind; x.sch.k_tk = k; } else { x.sch.teps = kind; x.sch.k_teps = k; }
    } else if (t.size() > 9 && t.rfind("div(phi,", 0) == 0 && t.back() == ')' && fgm_eq_index(t.substr(8, t.size() - 9)) >= 0) {
      const int e = fgm_eq_index(t.substr(8, t.size() - 9));   // the flareFGM scalars (fvSchemes:35-43 of the fgm cases)
      DFMI_CHECK(kind == SCH_UPWIND || kind == SCH_LL || kind == SCH_LL01, t + ": upwind, limitedLinear or limitedLinear01");
      x.sch.fgm[e] = kind; x.sch.k_fgm[e] = k;
    } else throw Error("dfmi: unknown scheme term '" + t + "' (div(phi,Yi_h), div(phi,K), div(hDiffCorrFlux), div(phi,U), div(phi,k), div(phi,epsilon), "
                       "div(phi,Z), div(phi,Zvar), div(phi,c), div(phi,cvar), div(phi,Zcvar), div(phi,Ha), laplacian)");
  });
}

int dfmi_set_traversal(dfmi_ctx* ctx, const int* order) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_sizes, "call dfmi_set_constant_values first");
    if (!order) { x.trav.release(); return; }
    std::vector<char> seen(x.C, 0);
    for (int t = 0; t < x.C; ++t) {
      DFMI_CHECK(order[t] >= 0 && order[t] < x.C && !seen[order[t]], "traversal order is not a permutation of the cells");
      seen[order[t]] = 1;
    }
    x.trav.upload(order, x.C, x.stream);
    DFMI_HIP(hipStreamSynchronize(x.stream));
  });
}

int dfmi_set_patch_param(dfmi_ctx* ctx, const char* field, int patch, const char* name, double value) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_bgeom, "call dfmi_init_constant_fields_boundary first");
    DFMI_CHECK(patch >= 0 && patch < x.P, "patch index out of range");
    const std::string f(field), n(name);
    // the k-epsilon wall function's own coefficients and the turbulent inlets' parameters
    const bool wall = f == "nut" && (n == "Cmu" || n == "kappa" || n == "E");
    if (wall || (f == "k" && n == "intensity") || (f == "epsilon" && n == "mixingLength")) {
      DFMI_CHECK(value > 0 && value <= 1.79769313486231570e308,
                 "patch parameter ('" + f + "', '" + n + "') of patch " + std::to_string(patch) + " must be positive and finite");
      ensure_wall_params(x);
      Ctx::WallFn& w = x.wf;
      (n == "Cmu" ? w.Cmu : n == "kappa" ? w.kappa : n == "E" ? w.E : n == "intensity" ? w.intensity : w.mixingLength)[patch] = value;
      w.dirty = true;
      if (wall) x.ras.valid = false;   // boundary_nut of a nutkWallFunction patch depends on them
      return;
    }
    DFMI_CHECK(f == "p" && n == "gamma",
               "patch parameters: ('p', 'gamma') of waveTransmissive, ('nut', 'Cmu' | 'kappa' | 'E') of nutkWallFunction, "
               "('k', 'intensity'), ('epsilon', 'mixingLength'); got ('" + f + "', '" + n + "')");
    std::vector<double> g(x.B);
    DFMI_HIP(hipMemcpy(g.data(), x.f("boundary_p_gamma"), x.B * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < x.psize[patch]; ++i) g[x.poff[patch] + i] = value;
    DFMI_HIP(hipMemcpy(x.f("boundary_p_gamma"), g.data(), x.B * sizeof(double), hipMemcpyHostToDevice));
  });
}

int dfmi_set_inert_index(dfmi_ctx* ctx, int inert_index) {
  return guard([&] {
    DFMI_CHECK(inert_index >= 0 && inert_index < ctx->x.S, "inert index out of range");
    ctx->x.inert = inert_index;
  });
}

int dfmi_thermo_set_coeffs(dfmi_ctx* ctx, int S, const double* W, const double* nasa, const double* visc,
                           const double* cond, const double* bdiff) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_sizes && S == x.S, "thermo species count differs from num_species");
    Thermo& t = x.thermo;
    t.S = S;
    t.W.assign(W, W + S); t.nasa.assign(nasa, nasa + 15 * S); t.visc.assign(visc, visc + 5 * S);
    t.cond.assign(cond, cond + 5 * S); t.bdiff.assign(bdiff, bdiff + 5 * S * S);
    t.vc1.resize(S * S); t.vc2.resize(S * S);
    for (int i = 0; i < S; ++i) for (int j = 0; j < S; ++j) {   // init_const_coeff_ptr (dfThermo.cu:22-52)
      t.vc1[i * S + j] = std::pow((1 + W[i] / W[j]), -0.5);
      t.vc2[i * S + j] = std::pow(W[j] / W[i], 0.25);
    }
    thermo_upload(x);
    DFMI_HIP(hipStreamSynchronize(x.stream));
  });
}

int dfmi_thermo_set_eos(dfmi_ctx* ctx, int model, int S, const double* a, const double* b, const double* w) {
  return guard([&] {
    DFMI_CHECK(ctx, "null context");
    Ctx& x = ctx->x;
    DFMI_CHECK(model == 0 || model == 1, "dfmi_thermo_set_eos: model must be 0 (ideal gas) or 1 (Peng-Robinson)");
    Thermo& t = x.thermo;
    if (model == 0) {   // clears: every thermo call launches the ideal-gas kernels again
      t.eos = 0;
      t.eos_a.clear(); t.eos_b.clear(); t.eos_w.clear();
      return;
    }
    DFMI_CHECK(t.S > 0 && t.S == x.S, "dfmi_thermo_set_eos: call dfmi_thermo_set_coeffs first");
    DFMI_CHECK(S == t.S, "dfmi_thermo_set_eos: num_species " + std::to_string(S) + " differs from the thermo table's " +
                             std::to_string(t.S));
    DFMI_CHECK(a && b && w, "dfmi_thermo_set_eos: null parameter array");
    DFMI_CHECK(S <= 16, "dfmi_thermo_set_eos: the Peng-Robinson equation of state is not available with more than 16 species "
                        "(the cooperative thermo kernel)");
    auto finite = [](double v) { return v >= -1.79769313486231570e308 && v <= 1.79769313486231570e308; };
    for (int i = 0; i < S; ++i) {
      const std::string at = " of species " + std::to_string(i);
      DFMI_CHECK(finite(a[i]) && finite(b[i]) && finite(w[i]), "dfmi_thermo_set_eos: a, b and acentric" + at + " must be finite");
      DFMI_CHECK(a[i] >= 0.0, "dfmi_thermo_set_eos: a" + at + " must not be negative");
      DFMI_CHECK(b[i] > 0.0, "dfmi_thermo_set_eos: b" + at + " must be positive");
    }
    ensure_eos_fields(x);
    t.eos_a.assign(a, a + S); t.eos_b.assign(b, b + S); t.eos_w.assign(w, w + S);
    thermo_eos_upload(x);
    t.eos = 1;
  });
}

int dfmi_thermo_load(dfmi_ctx* ctx, const char* path) {
  std::vector<double> all;
  int S = 0;
  int rc = guard([&] {
    std::ifstream in(path, std::ios::binary);
    DFMI_CHECK(in.good(), std::string("cannot open thermo coefficient file ") + path);
    in.read(reinterpret_cast<char*>(&S), sizeof(int));
    DFMI_CHECK(S > 0 && S <= 64, "bad species count in thermo file");
    const size_t n = S + 15 * S + 5 * S + 5 * S + 5 * S * S;
    all.resize(n);
    in.read(reinterpret_cast<char*>(all.data()), n * sizeof(double));
    DFMI_CHECK((size_t)in.gcount() == n * sizeof(double), "truncated thermo coefficient file");
  });
  if (rc) return rc;
  const double* p = all.data();
  return dfmi_thermo_set_coeffs(ctx, S, p, p + S, p + 16 * S, p + 21 * S, p + 26 * S);
}

int dfmi_set_field(dfmi_ctx* ctx, const char* name, const double* host, long count, int layout) {
  return guard([&] {
    Ctx& x = ctx->x;
    x.co.fresh = false;
    const std::string n(name ? name : "");
    if (n == "delta" || n == "nut" || n == "boundary_nut") ensure_les_fields(x);
    if (ras_name(n)) ensure_ras_fields(x);
    if (n == "rho_thermo" || n == "boundary_rho_thermo") ensure_eos_fields(x);
    if (fgm_name(n)) {
      DFMI_CHECK(n != "fgm_Su" && n != "fgm_D" && n != "boundary_fgm_D", "field '" + n + "' is formed by the flareFGM transport and cannot be set");
      ensure_fgm_fields(x);
    }
    if (tci_name(n)) {
      DFMI_CHECK(n == "tci_tc", "field '" + n + "' is formed by dfmi_combustion_correct and cannot be set");
      ensure_tci_fields(x);
    }
    DFMI_CHECK(n != "G" && n != "divU" && n.find("_prebound") == std::string::npos,
               "field '" + n + "' is formed by dfmi_turbulence_correct and cannot be set");
    DFMI_CHECK(n != "boundary_yPlus", "field 'boundary_yPlus' is formed by dfmi_turbulence_correct and cannot be set");
    DFMI_CHECK(n != "nut", "field 'nut' is formed by dfmi_turbulence_correct and cannot be set (boundary_nut holds the fixed-value slots)");
    DFMI_CHECK(n.rfind("les_", 0) != 0 && n.rfind("boundary_les_", 0) != 0,
               "field '" + n + "' is formed by dfmi_turbulence_correct (les.model = 5) and cannot be set");
    DFMI_CHECK(n.rfind("nonorth_", 0) != 0 && n.rfind("boundary_nonorth_", 0) != 0,
               "field '" + n + "' is formed by the library (dfmi_set_scheme \"laplacian\") and cannot be set");
    const int spi = spray_index(n);
    if (spi >= 0) {   // the cloud's accumulators: every value finite, UCoeff (a sum of masses over time scales) not negative
      ensure_spray_fields(x);
      DFMI_CHECK(count == x.C, "field '" + n + "': expected " + std::to_string(x.C) + " values per component, got " + std::to_string(count));
      const long tot = count * x.fields.at(n).ncomp;
      for (long i = 0; i < tot; ++i) {
        DFMI_CHECK(host[i] >= -1.79769313486231570e308 && host[i] <= 1.79769313486231570e308, "field '" + n + "': every value must be finite");
        DFMI_CHECK(spi != 2 || host[i] >= 0, "field 'parcel_UCoeff': the coefficient must not be negative");
      }
    }
    if (n == "delta") {
      DFMI_CHECK(count == x.C, "field 'delta': expected " + std::to_string(x.C) + " values, got " + std::to_string(count));
      for (long i = 0; i < count; ++i)
        DFMI_CHECK(host[i] > 0 && host[i] <= 1.79769313486231570e308, "field 'delta': the filter width must be positive and finite");
    }
    copy_field(x, n, host, count, layout, true);
    // nut belongs to delta and U as they stood at the last dfmi_turbulence_correct; the dropped terms' fields are
    // zeroed again before the next LES assembly whatever was written here
    if (n == "delta" || n == "U" || n == "boundary_U") x.les.valid = false;
    if (n == "delta") x.les.have_delta = true;
    x.les.zeroed = false;
    // RAS: nut belongs to k and epsilon and their boundary counterparts
    static const char* rk[4] = {"k", "epsilon", "boundary_k", "boundary_epsilon"};
    for (int i = 0; i < 4; ++i) if (n == rk[i]) { x.ras.have[i] = true; x.ras.valid = false; }
    if (spi >= 0) x.spray.have[spi] = true;
  });
}
int dfmi_get_field(dfmi_ctx* ctx, const char* name, double* host, long count, int layout) {
  return guard([&] {
    const std::string n(name ? name : "");
    if (n == "delta" || n == "nut" || n == "boundary_nut") ensure_les_fields(ctx->x);
    if (n == "les_Cs" || n == "les_LM" || n == "les_MM")
      DFMI_CHECK(ctx->x.fields.count(n), "field '" + n + "' exists with les.model = 5 (dynamicSmagorinsky) only");
    if (ras_name(n)) ensure_ras_fields(ctx->x);
    if (n == "rho_thermo" || n == "boundary_rho_thermo") ensure_eos_fields(ctx->x);
    if (fgm_name(n)) ensure_fgm_fields(ctx->x);
    if (n == "boundary_yPlus") ensure_wall_fields(ctx->x);
    if (tci_name(n)) ensure_tci_fields(ctx->x);
    if (spray_index(n) >= 0) ensure_spray_fields(ctx->x);
    copy_field(ctx->x, n, host, count, layout, false);
  });
}

int dfmi_pre_time_step(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); copy_old(ctx->x); }); }
int dfmi_post_time_step(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); }); }
int dfmi_rho_process(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); rho_process(ctx->x, false); }); }
int dfmi_U_process(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); les_effective(ctx->x); do_U(ctx->x); }); }
int dfmi_Y_process(dfmi_ctx* ctx) {
  return guard([&] {
    require_ready(ctx->x);
    DFMI_CHECK(!ctx->x.fgm.model, "dfmi_Y_process is not available with fgm.model = 1 (flareFGM solves no species equations: dfmi_fgm_correct)");
    ctx->x.dnn.prepared = false;   // a compaction left by an interrupted time step belongs to an old T
    les_effective(ctx->x);
    do_Y(ctx->x);
    if (ctx->x.chem.mode == 1) chem_check(ctx->x);   // the Y solve's polls have passed the chemistry
  });
}
int dfmi_E_process(dfmi_ctx* ctx) {
  return guard([&] {
    require_ready(ctx->x);
    DFMI_CHECK(!ctx->x.fgm.model, "dfmi_E_process is not available with fgm.model = 1 (flareFGM solves no energy equation: dfmi_fgm_correct)");
    les_effective(ctx->x);
    do_E(ctx->x);
  });
}
// flareFGM (include/dfmi.h, flareFGM block)
int dfmi_fgm_set_table(dfmi_ctx* ctx, const int* dims, const double* axes, double Hfu, double Hox, const double* laminar,
                       const double* tables, const double* d2Yeq, const double* d1Yeq, const int* species_index,
                       const int* omega_index) {
  return guard([&] {
    DFMI_CHECK(ctx, "null context");
    Ctx& x = ctx->x;
    fgm_set_table(x, dims, axes, Hfu, Hox, laminar, tables, d2Yeq, d1Yeq, species_index, omega_index);
    if (x.have_bgeom) ensure_fgm_fields(x);
  });
}
int dfmi_fgm_retrieve(dfmi_ctx* ctx) {
  return guard([&] {
    DFMI_CHECK(ctx, "null context");
    Ctx& x = ctx->x;
    require_ready(x);
    fgm_check(x, "dfmi_fgm_retrieve");
    fgm_retrieve(x, false);
    DFMI_HIP(hipStreamSynchronize(x.stream));
  });
}
int dfmi_fgm_correct(dfmi_ctx* ctx) {
  return guard([&] {
    DFMI_CHECK(ctx, "null context");
    Ctx& x = ctx->x;
    require_ready(x);
    fgm_correct(x);
    DFMI_HIP(hipStreamSynchronize(x.stream));
  });
}
// turbulence->correct() (dfLowMachFoam.C:508)
int dfmi_turbulence_correct(dfmi_ctx* ctx) {
  return guard([&] {
    DFMI_CHECK(ctx, "null context");
    if (!ctx->x.turbulent()) return;   // laminar: nothing to form
    require_ready(ctx->x);
    if (ctx->x.ras.model) { ras_correct(ctx->x); return; }   // kEpsilon::correct(): the two equations, then nut
    ensure_les_fields(ctx->x);
    turbulence_correct(ctx->x);
  });
}
int dfmi_p_process(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); do_p(ctx->x); }); }
int dfmi_U_get_HbyA(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); u_hbya(ctx->x); }); }
int dfmi_thermo_correct(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); thermo_correct(ctx->x, false); }); }
int dfmi_thermo_update_energy(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); thermo_correct(ctx->x, true); }); }
int dfmi_thermo_update_rho(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); thermo_rho_from_psi(ctx->x); }); }
int dfmi_thermo_psip0(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); thermo_psip0(ctx->x); }); }
int dfmi_thermo_correct_psip_rho(dfmi_ctx* ctx) { return guard([&] { require_ready(ctx->x); thermo_correct_psip_rho(ctx->x); }); }

// dfLowMachFoam.C:284-531 with nOuterCorrectors = 1 (the configuration every reference GPU case uses)
int dfmi_time_step(dfmi_ctx* ctx, int n_corr) {
  return guard([&] {
    Ctx& x = ctx->x;
    require_ready(x);
    // a step that throws records no end mark: restart the timer's ring so no reported interval spans two steps
    struct TimerReset {
      StepTimer& t;
      bool done = false;
      ~TimerReset() { if (!done) t.used = 0; }
    } treset{x.steptimer};
    const bool fgm = x.fgm.model != 0;
    if (fgm) fgm_check(x, "dfmi_time_step with fgm.model = 1");
    const bool eos = x.thermo.eos != 0;
    if (eos) {   // the real-fluid step is the laminar, non-reacting one (include/dfmi.h dfmi_thermo_set_eos)
      const char* why = "dfmi_time_step: with an equation of state set (dfmi_thermo_set_eos model 1) ";
      DFMI_CHECK(x.chem.mode == 0, std::string(why) + "chem.mode != 0 is not available (real-fluid kinetics needs activity "
                                                      "concentrations and the reactor's own density)");
      DFMI_CHECK(!x.les.model, std::string(why) + "les.model != 0 is not available");
      DFMI_CHECK(!x.ras.model, std::string(why) + "ras.model != 0 is not available");
      DFMI_CHECK(!x.tci.model, std::string(why) + "tci.model != 0 is not available");
    }
    if (x.steptimer.on && x.steptimer.used == 0) x.steptimer.mark(x.stream);
    x.dnn.prepared = false;         // never reuse a compaction of an earlier (failed) step
    if (x.les.model && !x.les.valid) { ensure_les_fields(x); turbulence_correct(x); }   // turbulence->validate() (dfLowMachFoam.C:207)
    if (x.ras.model && !x.ras.valid) { ensure_ras_fields(x); ras_nut(x); }                // RAS: correctNut() only, never the equations
    copy_old(x);                    // preTimeStep
    if (x.chem.mode == 2) dnn_prepare(x);   // reacting cells of this step's T (read after the UEqn polls)
    rho_process(x, false);          // rhoEqn (first PIMPLE iteration)
    les_effective(x);               // LES: muEff, alphaEff, mut / Sct from this rho (laminar: nothing)
    const bool early = !fgm && n_corr > 0 && hbya_early(x);   // the first corrector's HbyA right after the U solve
    if (fgm) {
      // flareFGM (dfLowMachFoam.C:328-455): no YEqn, no EEqn, no correctThermo; combustion->correct() writes T, psi, mu,
      // the table species, rho and rho_thermo
      do_U(x);
      fgm_correct(x);
    } else {
    do_U_Y_E(x, early);             // UEqn, YEqn, EEqn (one rank: the chemistry and YEqn assembly beside the
                                    // UEqn, the EEqn assembly beside the Y solve)
    thermo_correct(x, false);       // correctThermo
    }
    // Equation of state: thermo.rho_ (rho_thermo) is no longer psi p, so the corrector is the CPU solver's (pEqn.H:1-4, 8,
    // 95): rho = thermo.rho(), psip0 = psi p, the p equation, thermo.rho_ += psi p - psip0. Its closing rhoEqn writes a
    // rho that the next statement -- rho = thermo.rho() of the next corrector, or after the loop (dfLowMachFoam.C:517) --
    // overwrites before anything in this laminar step reads it, as in the ideal-gas loop below.
    // flareFGM runs the same corrector (the retrieval wrote rho and rho_thermo) and keeps the closing rhoEqn of the last
    // one, whose rho kEpsilon::correct() reads (the RAS tail of the ideal-gas loop).
    for (int i = 0; (eos || fgm) && i < n_corr; ++i) {
      if (i > 0) thermo_rho_from_psi(x);   // rho = rho_thermo (the first corrector's: correctThermo / the retrieval wrote both)
      thermo_psip0(x);
      if (i > 0 || !early) u_hbya(x);
      const int keep = (int)x.opt("amg.reuse_steps");
      x.amg.reuse_ok = i > 0 || (keep > 1 && x.amg.ready && x.amg.age > 0 && x.amg.age < keep);
      if (i == 0) x.amg.age = x.amg.reuse_ok ? x.amg.age + 1 : 1;
      do_p(x);
      x.amg.reuse_ok = false;
      thermo_correct_psip_rho(x);          // rho_thermo += psi p - psip0
      if (fgm && i == n_corr - 1) rho_process(x, false);
    }
    for (int i = 0; !eos && !fgm && i < n_corr; ++i) {   // pEqn_GPU.H
      // rho = psi p: the first corrector's is what correctThermo just wrote (the same product of the same p and psi,
      // halo included); psip0 = psi p feeds only correctPsipRho, skipped below (the field is not updated here)
      if (i > 0) thermo_rho_from_psi(x);
      const bool ras_tail = x.ras.model && i == n_corr - 1;   // RAS: the last corrector keeps pEqn.H's tail (below)
      if (ras_tail) thermo_psip0(x);
      if (i > 0 || !early) u_hbya(x);
      // a later corrector may precondition with this step's first hierarchy; with amg.reuse_steps = k > 1 the first
      // corrector too, with the operators of up to k - 1 steps before (rebuilt when they are that old)
      const int keep = (int)x.opt("amg.reuse_steps");
      x.amg.reuse_ok = i > 0 || (keep > 1 && x.amg.ready && x.amg.age > 0 && x.amg.age < keep);
      if (i == 0) x.amg.age = x.amg.reuse_ok ? x.amg.age + 1 : 1;
      do_p(x);
      x.amg.reuse_ok = false;
      // pEqn_GPU.H ends with thermo.correctPsipRho() and the rhoEqn; both write rho, which the next statement here
      // -- rho = psi p at the next corrector's start, or after the loop (dfLowMachFoam.C:517) -- overwrites before
      // anything reads it (the oracle's time_step runs them: the fields agree bitwise). dfmi_thermo_correct_psip_rho /
      // dfmi_rho_process keep them for callers that read rho in between.
      // RAS: turbulence->correct() (dfLowMachFoam.C:508) reads that rho -- the last corrector's correctPsipRho and rhoEqn
      // (the oracle's time_step: rho += psi p - psip0, then the rhoEqn from rho_old and the final phi)
      if (ras_tail) { thermo_correct_psip_rho(x); rho_process(x, false); }
    }
    if (x.ras.model) ras_correct(x);   // kEpsilon::correct() on the corrector's rho, before rho = thermo.rho()
    thermo_rho_from_psi(x);         // rho = thermo.rho() (dfLowMachFoam.C:517)
    turbulence_correct(x);          // turbulence->correct() (dfLowMachFoam.C:508) from the last corrector's U; laminar: nothing
    if (x.chem.mode == 1) chem_check(x);   // the p solves' polls have already passed the chemistry
    // compressibleCourantNo.H of the next loop pass, queued now that the step's final phi (last pEqn) and rho are
    // written: dfmi_courant_no then reads the record instead of launching (option step.courant; off: nothing added)
    if (x.on("step.courant")) courant_post(x);
    if (x.steptimer.on) x.steptimer.mark(x.stream);
    treset.done = true;
  });
}

// compressibleCourantNo.H (dfLowMachFoam.C:261)
int dfmi_courant_no(dfmi_ctx* ctx, double* co_num, double* mean_co_num) {
  return guard([&] {
    DFMI_CHECK(ctx, "null context");
    Ctx& x = ctx->x;
    DFMI_CHECK(co_num && mean_co_num, "dfmi_courant_no: null output pointer");
    if (!x.co.fresh) {   // no record of the fields as they stand (step.courant off, or something was set since)
      require_ready(x);
      courant_post(x);
    }
    // wait (spinning) for the record queued last, as the solvers' Poller does: no stream drain. A stream that drained
    // without posting it (a failed launch) is an error rather than a hang.
    const CoRec* r = x.co.h;
    const long long seq = x.co.seq;
    for (long spins = 0; __atomic_load_n(&r->seq, __ATOMIC_ACQUIRE) < seq; ++spins) {
      if ((spins & 0xfff) != 0xfff) continue;
      const hipError_t q = hipStreamQuery(x.stream);
      if (q != hipErrorNotReady && __atomic_load_n(&r->seq, __ATOMIC_ACQUIRE) < seq) {
        x.co.fresh = false;
        DFMI_HIP(q);
        throw Error("dfmi_courant_no: the stream drained without posting the Courant-number record");
      }
    }
    *co_num = r->co;
    *mean_co_num = r->mean;
  });
}

// setDeltaT.H (dfLowMachFoam.C:262). Every kernel takes 1 / deltaT by value at its launch (Ctx::view, MeshView::rdt:
// ddt terms, ddtCorr, dpdt, the waveTransmissive valueFraction) and the chemistry its interval (do_Y_front), so nothing
// on the device keeps the old step; the chemistry's remembered sub-step (chem_stats row 2) is capped by the interval
// where it is read (chem.hip: h = min(dt, remembered)). What does outlive a step is the pressure AMG's operators.
int dfmi_set_delta_t(dfmi_ctx* ctx, double delta_t) {
  return guard([&] {
    DFMI_CHECK(ctx, "null context");
    Ctx& x = ctx->x;
    DFMI_CHECK(x.have_sizes, "dfmi_set_delta_t: call dfmi_set_constant_values first");
    DFMI_CHECK(delta_t > 0 && delta_t <= 1.79769313486231570e308, "dfmi_set_delta_t: delta_t must be positive and finite");
    const double rdt = 1.0 / delta_t;
    DFMI_CHECK(rdt > 0 && rdt <= 1.79769313486231570e308, "dfmi_set_delta_t: 1 / delta_t is not a positive finite number");
    if (delta_t != x.dt) {   // a posted Courant number was formed with the old step
      x.dt = delta_t;
      x.co.fresh = false;
    }
    if (rdt == x.rdt) return;   // the step the kernels run with already: nothing changes, nothing is reset
    x.rdt = rdt;
    x.amg.age = 0;   // ends the cross-step reuse window (amg.reuse_steps): the next first corrector rebuilds
  });
}

int dfmi_get_delta_t(dfmi_ctx* ctx, double* delta_t) {
  return guard([&] {
    DFMI_CHECK(ctx && delta_t, "dfmi_get_delta_t: null pointer");
    DFMI_CHECK(ctx->x.have_sizes, "dfmi_get_delta_t: call dfmi_set_constant_values first");
    *delta_t = ctx->x.dt;
  });
}

int dfmi_step_timer(dfmi_ctx* ctx, int on) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_HIP(hipStreamSynchronize(x.stream));
    x.steptimer.on = on != 0;
    x.steptimer.used = 0;
  });
}

int dfmi_step_times(dfmi_ctx* ctx, double* ms, int n, int* got) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_HIP(hipStreamSynchronize(x.stream));
    const StepTimer& t = x.steptimer;
    // intervals between consecutive marks still in the ring: the last min(used, CAP) - 1 of them
    const size_t kept = std::min(t.used, StepTimer::CAP);
    const int have = kept > 1 ? (int)kept - 1 : 0;
    const size_t m0 = t.used - kept;
    for (int i = 0; i < have && i < n; ++i) {
      float v = 0;
      DFMI_HIP(hipEventElapsedTime(&v, t.at(m0 + i), t.at(m0 + i + 1)));
      ms[i] = v;
    }
    if (got) *got = have;
  });
}

// correct_boundary_conditions_{scalar,vector} of one named field (dfMatrixOpBase.cu:2402-2491)
int dfmi_correct_boundary(dfmi_ctx* ctx, const char* field) {
  return guard([&] {
    Ctx& x = ctx->x;
    require_ready(x);
    std::string f(field);
    if (f == "Y") k_bc_correct(x, "Y", x.f("Y"), x.f("boundary_Y"), x.S);
    else if (f == "U") k_bc_correct(x, "U", x.f("U"), x.f("boundary_U"), 3);
    else if (f == "nut" && (ensure_les_fields(x), true)) k_bc_correct(x, x.stype.count("nut") ? "nut" : "calculated", x.f("nut"), x.f("boundary_nut"), 1);
    else if (f == "p" || f == "he" || f == "T" || f == "rho" || f == "K") k_bc_correct(x, f.c_str(), x.f(f), x.f("boundary_" + f), 1);
    else throw Error("dfmi_correct_boundary: unsupported field '" + f + "'");
    halo_fields(x, {f.c_str()});
    DFMI_HIP(hipStreamSynchronize(x.stream));
  });
}

int dfmi_comm_timer(dfmi_ctx* ctx, int on) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_HIP(hipStreamSynchronize(x.stream));
    x.comm.reset();
    x.comm.on = on != 0;
    x.comm.tag.clear();
  });
}

int dfmi_comm_report(dfmi_ctx* ctx, char* buf, int len, int* needed) {
  return guard([&] {
    const std::string r = comm_report(ctx->x);
    if (needed) *needed = (int)r.size() + 1;
    if (buf && len > 0) std::snprintf(buf, len, "%s", r.c_str());
  });
}

int dfmi_kernel_timer(dfmi_ctx* ctx, const char* kernels) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_HIP(hipStreamSynchronize(x.stream));
    KernelTimer& k = x.ktimer;
    k.targets.clear(); k.rec.clear(); k.used = 0;
    std::string s(kernels ? kernels : ""), cur;
    for (char ch : s + ",") {
      if (ch == ',') { if (!cur.empty()) k.targets.push_back(cur); cur.clear(); }
      else if (ch != ' ') cur += ch;
    }
  });
}

int dfmi_kernel_time_named(dfmi_ctx* ctx, const char* kernel, double* total_ms, int* launches) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_HIP(hipStreamSynchronize(x.stream));
    KernelTimer& k = x.ktimer;
    int t = -1;
    for (size_t i = 0; i < k.targets.size(); ++i) if (k.targets[i] == kernel) t = (int)i;
    DFMI_CHECK(t >= 0, std::string("kernel '") + kernel + "' is not armed");
    double tot = 0;
    int n = 0;
    for (size_t r = 0; r < k.rec.size() && 2 * r + 1 < k.used; ++r) {
      if (k.rec[r] != t) continue;
      float ms = 0;
      DFMI_HIP(hipEventElapsedTime(&ms, k.pool[2 * r], k.pool[2 * r + 1]));
      tot += ms;
      ++n;
    }
    *total_ms = tot;
    *launches = n;
  });
}

int dfmi_kernel_time(dfmi_ctx* ctx, double* total_ms, int* launches) {
  return guard([&] {
    DFMI_CHECK(!ctx->x.ktimer.targets.empty(), "no kernel armed");
    const std::string first = ctx->x.ktimer.targets[0];
    if (dfmi_kernel_time_named(ctx, first.c_str(), total_ms, launches)) throw Error(g_err);
  });
}

int dfmi_sync(dfmi_ctx* ctx) { return guard([&] { DFMI_HIP(hipStreamSynchronize(ctx->x.stream)); }); }

int dfmi_hbm_copy_peak(dfmi_ctx* ctx, double gib, int reps, double* gbs) {
  return guard([&] {
    DFMI_CHECK(gib > 0 && reps > 0 && gbs, "bad arguments");
    *gbs = hbm_copy_gbs(ctx->x, (size_t)(gib * (1ull << 30)), reps);
  });
}

int dfmi_assemble(dfmi_ctx* ctx, const char* eqn) {
  return guard([&] {
    Ctx& x = ctx->x;
    require_ready(x);
    std::string e(eqn);
    if (e == "U" || e == "Y" || e == "Y_ell" || e == "Y_ell_ref" || e == "E") les_effective(x);
    if (e == "rho") {
      if (!x.fields.count("dbg_rho_diag")) { alloc_field(x, "dbg_rho_diag", x.C, 1, false); alloc_field(x, "dbg_rho_source", x.C, 1, false); }
      rho_process(x, true);
    } else if (e == "U") {
      if (!x.fields.count("dbg_gradU")) alloc_field(x, "dbg_gradU", x.C, 9, false);
      u_assemble(x);
    } else if (e == "Y") {
      if (!x.fields.count("dbg_gradY")) alloc_field(x, "dbg_gradY", x.C, 3 * x.S, false);
      y_prep(x); y_assemble(x);
    } else if (e == "Y_ell") {        // production: fused assembly straight into the solver rows
      YWs _yw(x);
      std::vector<int> map;
      for (int s = 0; s < x.S; ++s) if (s != x.inert) map.push_back(s);
      double *val, *dS, *rhs;
      bicg_layout(x, (int)map.size(), &val, &dS, &rhs);
      y_prep(x);
      y_assemble_ell(x, x.ell.W, (long)x.C + x.H, val, dS, rhs);
    } else if (e == "Y_ell_ref") {    // LDU assembly folded by the generic solver gather
      YWs _yw(x);
      // spray: the rows are folded from the LDU parts without the parcel terms, which then go into both forms as the
      // last thing added -- the order y_assemble_ell keeps (dS = diag + internalCoeffs, then the term)
      y_prep(x); y_assemble(x, false);
      bicg_rows_from_ldu_Y(x);
      if (x.spray.model) {
        spray_fold_y(x, x.mY.diag.p, x.mY.source.p, x.C, false);
        double *val, *dS, *rhs;
        bicg_layout(x, x.S - 1, &val, &dS, &rhs);
        spray_fold_y(x, dS, rhs, (long)x.C + x.H, true);
      }
    } else if (e == "E") { conv_weights(x); e_assemble(x); }   // EEqn inspected on its own: fresh div(phi,Yi_h) weights
    else if (e == "k" || e == "epsilon") {   // from the fields as they stand, no solve in between
      DFMI_CHECK(x.ras.model, "dfmi_assemble: '" + e + "' needs ras.model != 0");
      ensure_ras_fields(x);
      // a wall-function context: the complete wall update first (epsilon of the wall cells overwritten), the state the
      // equations see inside correct(); "epsilon" is then the constrained matrix
      ras_inlet_k(x);
      ras_production(x);
      ras_wall_update(x);
      ras_assemble(x, e == "k" ? 1 : 0);
    }
    else if (fgm_eq_index(e) >= 0) {   // a flareFGM transport equation from the fields as they stand, no solve in between
      fgm_check(x, "dfmi_assemble");
      fgm_halo(x);
      if (!x.ras.valid) ras_nut(x);
      fgm_assemble(x, fgm_eq_index(e));
    }
    else if (e == "p") {
      p_assemble(x);
      // corrected laplacian: the source of the corrector loop's first pass (do_p_nonorth)
      if (x.lap == LAP_CORRECTED) { nonorth_p_base(x); nonorth_p_correct(x); }
    }
    else if (e == "tci") combustion_pointwise(x);   // the closure's pointwise passes from RR and Qdot as they stand
    else if (e == "HbyA") u_hbya(x);
    else if (e == "p_post") p_post_solve(x);
    else if (e == "Y_post") y_post_solve(x);
    else throw Error("unknown equation '" + e + "'");
    DFMI_HIP(hipStreamSynchronize(x.stream));
  });
}

int dfmi_get_matrix(dfmi_ctx* ctx, const char* eqn, const char* part, double* host, long count) {
  return guard([&] {
    Ctx& x = ctx->x;
    std::string e(eqn), p(part);
    Matrix* A = e == "U" ? &x.mU : e == "Y" ? &x.mY : e == "E" ? &x.mE : e == "p" ? &x.mP
                : (e == "k" || e == "epsilon" || fgm_eq_index(e) >= 0) ? &x.mK : nullptr;   // the scalar assembly's, whichever it formed last
    DFMI_CHECK(A, "unknown equation '" + e + "'");
    DevBuf<double>* b = p == "lower" ? &A->lower : p == "upper" ? &A->upper : p == "diag" ? &A->diag :
                        p == "source" ? &A->source : p == "source_solve" ? &A->source_solve :
                        p == "internal_coeffs" ? &A->ic : p == "boundary_coeffs" ? &A->bc : nullptr;
    DFMI_CHECK(b && b->p, "unknown matrix part '" + p + "'");
    if (p == "lower" || p == "upper") {   // face storage -> OpenFOAM face order, per system
      const long ns = (long)(b->n / std::max(x.Fs, 1));
      DFMI_CHECK(count == ns * x.F, "matrix part size mismatch: expected " + std::to_string(ns * x.F));
      std::vector<double> st(b->n);
      DFMI_HIP(hipMemcpyAsync(st.data(), b->p, b->n * sizeof(double), hipMemcpyDeviceToHost, x.stream));
      DFMI_HIP(hipStreamSynchronize(x.stream));
      for (long s = 0; s < ns; ++s)
        for (long f = 0; f < x.F; ++f) host[s * x.F + f] = st[s * x.Fs + x.h_fst[f]];
      return;
    }
    DFMI_CHECK((size_t)count == b->n, "matrix part size mismatch: expected " + std::to_string(b->n));
    DFMI_HIP(hipMemcpyAsync(host, b->p, count * sizeof(double), hipMemcpyDeviceToHost, x.stream));
    DFMI_HIP(hipStreamSynchronize(x.stream));
  });
}

int dfmi_get_solver_rows(dfmi_ctx* ctx, const char* eqn, const char* part, double* host, long count) {
  return guard([&] {
    Ctx& x = ctx->x;
    DFMI_CHECK(std::string(eqn) == "Y", "solver rows are inspectable for the YEqn batch only");
    YWs _yw(x);
    bicg_rows_get(x, x.S - 1, part, host, count);
  });
}

int dfmi_set_solver(dfmi_ctx* ctx, const char* eqn, int max_iter, double tol, double abs_tol) {
  return guard([&] {
    std::string e(eqn);
    DFMI_CHECK(e == "U" || e == "Y" || e == "E" || e == "p" || e == "k" || e == "epsilon" || fgm_eq_index(e) >= 0, "unknown equation '" + e + "'");
    DFMI_CHECK(max_iter > 0 && tol >= 0 && abs_tol >= 0, "bad solver controls");
    SolverCfg& c = ctx->x.solver[e];
    c.max_iter = max_iter; c.tol = tol; c.abs_tol = abs_tol;
  });
}

int dfmi_chem_set_mechanism(dfmi_ctx* ctx, int n_reactions, const int* idata, const int* irs, const double* ddata) {
  return guard([&] {
    DFMI_CHECK(ctx->x.have_sizes, "call dfmi_set_constant_values first");
    chem_upload(ctx->x, n_reactions, idata, irs, ddata);
  });
}

int dfmi_chem_set_options(dfmi_ctx* ctx, int mode, double rtol, double atol, double T_min) {
  return guard([&] {
    DFMI_CHECK(mode >= 0 && mode <= 2, "chemistry mode must be 0 (off), 1 (ODE) or 2 (DNN)");
    DFMI_CHECK(rtol > 0 && atol > 0, "chemistry tolerances must be positive");
    DFMI_CHECK(mode != 2 || !ctx->x.tci.model, "chemistry mode 2 (DNN) is not available with tci.model != 0");
    Chem& c = ctx->x.chem;
    c.mode = mode; c.rtol = rtol; c.atol = atol; c.Tmin = T_min;
  });
}

int dfmi_dnn_set_model(dfmi_ctx* ctx, int n_modules, int n_layers, const int* dims, const float* params,
                       const double* x_mu, const double* x_std, const double* y_mu, const double* y_std,
                       double T_react, double dt_infer) {
  return guard([&] {
    DFMI_CHECK(ctx->x.have_sizes && ctx->x.inert >= 0, "set sizes and the inert index first");
    dnn_upload(ctx->x, n_modules, n_layers, dims, params, x_mu, x_std, y_mu, y_std, T_react, dt_infer);
  });
}

int dfmi_dnn_load_model(dfmi_ctx* ctx, const char* path, double T_react, double dt_infer) {
  std::vector<char> raw;
  int rc = guard([&] {
    DFMI_CHECK(path, "null path");
    std::ifstream in(path, std::ios::binary);
    DFMI_CHECK(in.good(), std::string("cannot open DF-ODENet model file ") + path);
    raw.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
  });
  if (rc) return rc;
  int nmod = 0, nl = 0;
  std::vector<int> dims;
  std::vector<double> xmu, xstd, ymu, ystd;
  std::vector<float> params;
  rc = guard([&] {
    size_t o = 0;
    auto take = [&](void* dst, size_t n) {
      DFMI_CHECK(o + n <= raw.size(), std::string("truncated DF-ODENet model file ") + path);
      std::memcpy(dst, raw.data() + o, n);
      o += n;
    };
    char magic[8];
    take(magic, 8);
    DFMI_CHECK(std::memcmp(magic, "DFMIDNN1", 8) == 0, std::string(path) + ": not a packed DF-ODENet file (DFMIDNN1)");
    take(&nmod, 4);
    take(&nl, 4);
    DFMI_CHECK(nmod >= 1 && nmod <= 63 && nl >= 1 && nl <= 8, std::string(path) + ": bad module / layer counts");
    dims.resize(nl + 1);
    take(dims.data(), 4 * dims.size());
    size_t np = 0;
    for (int l = 0; l < nl; ++l) {
      DFMI_CHECK(dims[l] > 0 && dims[l] <= 65536 && dims[l + 1] > 0 && dims[l + 1] <= 65536, std::string(path) + ": bad widths");
      np += (size_t)dims[l] * dims[l + 1] + dims[l + 1];
    }
    // the size the header implies against the file, before anything is sized from the header (widths <= 2^16 and
    // <= 8 layers keep np below 2^36, n_modules <= 63: no product here can wrap a 64-bit size_t, checked anyway)
    static_assert(sizeof(size_t) >= 8, "64-bit size_t expected");
    DFMI_CHECK(np <= (size_t)1 << 40, std::string(path) + ": bad widths");
    const size_t implied = o + 8 * (2 * (size_t)dims[0] + 2 * (size_t)nmod) + 4 * np * (size_t)nmod;
    DFMI_CHECK(implied <= raw.size(), std::string("truncated DF-ODENet model file ") + path);
    xmu.resize(dims[0]); xstd.resize(dims[0]); ymu.resize(nmod); ystd.resize(nmod);
    take(xmu.data(), 8 * xmu.size()); take(xstd.data(), 8 * xstd.size());
    take(ymu.data(), 8 * ymu.size()); take(ystd.data(), 8 * ystd.size());
    params.resize(np * nmod);
    take(params.data(), 4 * params.size());
    DFMI_CHECK(o == raw.size(), std::string(path) + ": trailing bytes after the parameters");
  });
  if (rc) return rc;
  return dfmi_dnn_set_model(ctx, nmod, nl, dims.data(), params.data(), xmu.data(), xstd.data(), ymu.data(), ystd.data(),
                            T_react, dt_infer);
}

int dfmi_dnn_infer(dfmi_ctx* ctx, int* n_reacting) {
  return guard([&] {
    Ctx& x = ctx->x;
    require_ready(x);
    x.dnn.prepared = false;         // standalone inference: compact on the current T
    dnn_solve(x, "rho");
    DFMI_HIP(hipStreamSynchronize(x.stream));
    if (n_reacting) *n_reacting = x.dnn.last_reacting;
  });
}

int dfmi_dnn_stats(dfmi_ctx* ctx, int* n_reacting, double* gemm_flops) {
  return guard([&] {
    Dnn& d = ctx->x.dnn;
    if (n_reacting) *n_reacting = d.last_reacting;
    if (gemm_flops) *gemm_flops = d.gemm_flops;
    d.gemm_flops = 0;
  });
}

int dfmi_dnn_plan(dfmi_ctx* ctx, int max_layers, int* n_layers, int* kinds) {
  return guard([&] {
    DFMI_CHECK(n_layers && (kinds || max_layers <= 0), "null output");
    dnn_plan(ctx->x, max_layers, n_layers, kinds);
  });
}

int dfmi_chem_info(dfmi_ctx* ctx, int* generated) {
  return guard([&] { *generated = ctx->x.chem.generated; });
}

int dfmi_chem_solve(dfmi_ctx* ctx, double dt) {
  return guard([&] {
    Ctx& x = ctx->x;
    require_ready(x);
    DFMI_CHECK(dt > 0, "chemistry time step must be positive");
    chem_solve(x, dt, "rho");
    DFMI_HIP(hipStreamSynchronize(x.stream));
    chem_check(x);
  });
}

// combustion->correct() (YEqn.H:76; PaSR.C:205-396, EDC.C:83-171)
int dfmi_combustion_correct(dfmi_ctx* ctx, double dt) {
  return guard([&] {
    DFMI_CHECK(ctx, "null context");
    Ctx& x = ctx->x;
    require_ready(x);
    DFMI_CHECK(dt > 0, "chemistry time step must be positive");
    combustion_correct(x, dt, "rho");
    DFMI_HIP(hipStreamSynchronize(x.stream));
    chem_check(x);
  });
}

int dfmi_zero_d_step(dfmi_ctx* ctx, double dt, int n_steps) {
  return guard([&] {
    Ctx& x = ctx->x;
    require_ready(x);
    DFMI_CHECK(dt > 0 && n_steps >= 1, "0D step: dt and n_steps must be positive");
    DFMI_CHECK(!x.fgm.model, "dfmi_zero_d_step is not available with fgm.model = 1 (the reactor's chemistry is the mechanism's, not the table's)");
    DFMI_CHECK(!x.thermo.eos, "dfmi_zero_d_step is not available with an equation of state set (dfmi_thermo_set_eos model 1): "
                              "the reactor's chemistry is the ideal-gas one");
    x.dnn.prepared = false;
    // no host synchronisation inside the loop: the steps' launches queue back to back (one round trip per step
    // bounded config 1 at ~0.1 ms/step), the chemistry's failure counter sums over the batch and is read once
    Chem& h = x.chem;
    if (h.mode == 1) {
      if (h.fail.n == 0) h.fail.alloc(1);
      DFMI_HIP(hipMemsetAsync(h.fail.p, 0, sizeof(int), x.stream));
      h.batch = true;
    }
    struct BatchEnd {
      Chem& h;
      ~BatchEnd() { h.batch = false; }
    } bend{h};
    for (int i = 0; i < n_steps; ++i) zero_d_step(x, dt);
    if (h.mode == 1) {
      h.batch = false;
      chem_fail_snapshot(x);
      chem_check(x);
    }
    DFMI_HIP(hipStreamSynchronize(x.stream));
  });
}

int dfmi_chem_set_max_steps(dfmi_ctx* ctx, int max_steps) {
  return guard([&] {
    DFMI_CHECK(max_steps > 0, "max_steps must be positive");
    ctx->x.chem.max_steps = max_steps;
  });
}

int dfmi_amg_info(dfmi_ctx* ctx, int max_levels, int* n_levels, int* cells, int* width) {
  return guard([&] {
    const Amg& a = ctx->x.amg;
    *n_levels = (int)a.lv.size();
    for (int l = 0; l < (int)a.lv.size() && l < max_levels; ++l) { cells[l] = a.lv[l].n; width[l] = a.lv[l].W; }
    if (a.global && (int)a.lv.size() < max_levels) {   // the agglomerated level, listed last
      cells[a.lv.size()] = a.ng; width[a.lv.size()] = a.wg;
      *n_levels += 1;
    }
  });
}

int dfmi_amg_smoother_info(dfmi_ctx* ctx, int level, double* colour, double* dilu_diag, long count) {
  return guard([&] { amg_smoother_info(ctx->x, level, colour, dilu_diag, count); });
}

int dfmi_amg_apply(dfmi_ctx* ctx, const double* r, double* z, long count) {
  return guard([&] { amg_apply_host(ctx->x, r, z, count); });
}

int dfmi_row_classes(dfmi_ctx* ctx, int* n) {
  return guard([&] { *n = ctx->x.ell.ready ? ctx->x.ell.ncls : 0; });
}

int dfmi_hex_dims(dfmi_ctx* ctx, int* nx, int* ny, int* nz) {
  return guard([&] {
    const bool on = ctx->x.ell.ready;
    *nx = on ? ctx->x.hex[0] : 0; *ny = on ? ctx->x.hex[1] : 0; *nz = on ? ctx->x.hex[2] : 0;
  });
}

int dfmi_set_option(dfmi_ctx* ctx, const char* key, double value) {
  return guard([&] {
    Ctx& x = ctx->x;
    (void)x.opt(key);   // throws for an unknown key
    const std::string k(key);
    // keys read when the AMG hierarchy (amg_setup) or the solver rows (build_ell) are built; every other key is
    // read at each call (amg.reuse per p solve, pcg.* / fv.* / chem.* / dnn.* per launch)
    static const char* structural_keys[] = {"amg.omega", "amg.overcorrection", "amg.coarsest_sweeps",
                                            "amg.coarsest_size", "amg.presweeps", "amg.pairwise_passes_l0",
                                            "amg.pairwise_passes", "amg.precision", "amg.padded", "amg.tail",
                                            "amg.halo_l0", "amg.global_coarse", "amg.smoother", "solver.even_odd", "solver.small",
                                            "solver.row_classes"};
    bool structural = false;
    for (const char* s : structural_keys) structural |= k == s;
    DFMI_CHECK(!structural || (!x.amg.ready && !x.ell.ready),
               "dfmi_set_option: '" + k + "' shapes the solver structures; set it before the first solve");
    DFMI_CHECK(k != "amg.smoother" || value == 0.0 || value == 1.0,
               "dfmi_set_option: amg.smoother must be 0 (weighted Jacobi) or 1 (multicolour DILU)");
    // multicolour DILU is rank-local on every level: no agglomerated coarsest level beside it
    const bool dilu = k == "amg.smoother" ? value == 1.0 : x.opt("amg.smoother") == 1.0;
    const bool global = k == "amg.global_coarse" ? value != 0.0 : x.on("amg.global_coarse");
    DFMI_CHECK(!((k == "amg.smoother" || k == "amg.global_coarse") && dilu && global),
               "dfmi_set_option: amg.smoother = 1 (multicolour DILU) and amg.global_coarse = 1 exclude each other");
    if (k == "p.n_nonorth")
      DFMI_CHECK(value >= 0 && value <= 1000 && value == (double)(int)value,
                 "dfmi_set_option: p.n_nonorth (nNonOrthogonalCorrectors) must be an integer >= 0");
    if (k.rfind("les.", 0) == 0) {
      if (k == "les.model")
        DFMI_CHECK(value == 0.0 || value == 1.0 || value == 2.0 || value == 4.0 || value == 5.0,
                   "dfmi_set_option: les.model must be 0 (laminar), 1 (Smagorinsky), 2 (WALE), 4 (Sigma) or 5 "
                   "(dynamicSmagorinsky); 3 is reserved");
      else
        DFMI_CHECK(value > 0 && value <= 1.79769313486231570e308, "dfmi_set_option: " + k + " must be positive and finite");
      // nut belongs to the model and its coefficients (Prt and Sct enter the effective fields, formed at every
      // assembly, but a changed coefficient invalidates all the same: one rule)
      DFMI_CHECK(k != "les.model" || value == 0.0 || !x.ras.model,
                 "dfmi_set_option: les.model != 0 and ras.model != 0 exclude each other (one turbulence model at a time)");
      DFMI_CHECK(k != "les.model" || value == 0.0 || !x.tci.model,
                 "dfmi_set_option: les.model != 0 and tci.model != 0 exclude each other");
      if (value != x.opt(key)) { x.les.valid = false; x.les.zeroed = false; }
      DFMI_CHECK(k != "les.model" || value == 0.0 || !x.fgm.model,
                 "dfmi_set_option: les.model != 0 and fgm.model = 1 exclude each other (magUPrime needs an LESfilter)");
      if (k == "les.model") x.les.model = (int)value;
      if (x.les.model && x.have_bgeom) ensure_les_fields(x);
    }
    if (k.rfind("ras.", 0) == 0) {
      if (k == "ras.model") {
        DFMI_CHECK(value == 0.0 || value == 1.0, "dfmi_set_option: ras.model must be 0 (none) or 1 (kEpsilon)");
        DFMI_CHECK(value == 0.0 || !x.les.model,
                   "dfmi_set_option: ras.model != 0 and les.model != 0 exclude each other (one turbulence model at a time)");
      } else if (k == "ras.C3")
        DFMI_CHECK(value >= -1.79769313486231570e308 && value <= 1.79769313486231570e308, "dfmi_set_option: ras.C3 must be finite");
      else
        DFMI_CHECK(value > 0 && value <= 1.79769313486231570e308, "dfmi_set_option: " + k + " must be positive and finite");
      // nut belongs to the model and its coefficients: one rule, as for les.*
      if (value != x.opt(key)) { x.ras.valid = false; x.les.valid = false; x.les.zeroed = false; }
      DFMI_CHECK(k != "ras.model" || value == 1.0 || !x.fgm.model,
                 "dfmi_set_option: ras.model = 0 is refused while fgm.model = 1 (the retrieval divides by k)");
      if (k == "ras.model") x.ras.model = (int)value;
      if (x.ras.model && x.have_bgeom) ensure_ras_fields(x);
    }
    if (k.rfind("fgm.", 0) == 0) {
      if (k == "fgm.model" || k == "fgm.combustion" || k == "fgm.solveEnthalpy" || k == "fgm.flameletT")
        DFMI_CHECK(value == 0.0 || value == 1.0, "dfmi_set_option: " + k + " must be 0 or 1");
      else if (k == "fgm.incompPref")
        DFMI_CHECK(value >= -1.79769313486231570e308 && value <= 1.79769313486231570e308, "dfmi_set_option: fgm.incompPref must be finite");
      else
        DFMI_CHECK(value > 0 && value <= 1.79769313486231570e308, "dfmi_set_option: " + k + " must be positive and finite");
      if (k == "fgm.model" && value == 1.0) {
        const char* why = "dfmi_set_option: fgm.model = 1 ";
        DFMI_CHECK(x.fgm.have_table, std::string(why) + "needs a flamelet table (dfmi_fgm_set_table first)");
        DFMI_CHECK(x.ras.model == 1, std::string(why) + "needs ras.model = 1 (the retrieval divides by k)");
        DFMI_CHECK(!x.les.model, std::string(why) + "and les.model != 0 exclude each other (magUPrime needs an LESfilter)");
        DFMI_CHECK(!x.tci.model, std::string(why) + "and tci.model != 0 exclude each other (one combustion model at a time)");
        DFMI_CHECK(x.chem.mode == 0, std::string(why) + "is not available with chemistry mode != 0 (the table replaces the chemistry)");
        DFMI_CHECK(!x.thermo.eos, std::string(why) + "is not available with an equation of state set (dfmi_thermo_set_eos model 1)");
        DFMI_CHECK(!x.spray.model, std::string(why) + "is not available with spray.model = 1 (the flareFGM spray branch is not on the device)");
        if (x.have_bgeom) ensure_fgm_fields(x);
      }
      if (k == "fgm.model") x.fgm.model = (int)value;
    }
    if (k.rfind("tci.", 0) == 0) {
      const auto one_of = [&](std::initializer_list<double> vs) { bool ok = false; for (double v : vs) ok |= value == v; return ok; };
      DFMI_CHECK(k != "tci.bad_tauStar", "dfmi_set_option: tci.bad_tauStar is a counter and cannot be set");
      if (k == "tci.model") {
        DFMI_CHECK(one_of({0, 1, 2}), "dfmi_set_option: tci.model must be 0 (none), 1 (PaSR) or 2 (EDC)");
        DFMI_CHECK(value == 0.0 || !x.les.model, "dfmi_set_option: tci.model != 0 and les.model != 0 exclude each other");
        DFMI_CHECK(value == 0.0 || x.chem.mode != 2,
                   "dfmi_set_option: tci.model != 0 is not available with the DNN surrogate (chemistry mode 2)");
      } else if (k == "tci.mixing") {
        DFMI_CHECK(value != 4.0, "dfmi_set_option: tci.mixing dynamicScale is not supported (its Z / Zvar / Chi equations are not on the device)");
        DFMI_CHECK(one_of({1, 2, 3}), "dfmi_set_option: tci.mixing must be 1 (globalScale), 2 (kolmogorovScale) or 3 (geometriMeanScale)");
      } else if (k == "tci.chemistry")
        DFMI_CHECK(one_of({1, 2, 3}), "dfmi_set_option: tci.chemistry must be 1 (globalConvertion), 2 (formationRate) or 3 (reactionRate)");
      else if (k == "tci.version")
        DFMI_CHECK(one_of({1981, 1996, 2005, 2016}), "dfmi_set_option: tci.version must be 1981, 1996, 2005 or 2016");
      else if (k == "tci.exp1" || k == "tci.exp2")
        DFMI_CHECK(one_of({0, 1, 2, 3, 4}), "dfmi_set_option: " + k + " must be 0 (the version's own) or an integer 1..4");
      else if (k == "tci.fuel" || k == "tci.oxidizer" || k == "tci.CO2" || k == "tci.H2")
        DFMI_CHECK(value >= -1 && value < 64 && value == (double)(int)value && (!x.have_sizes || value < x.S),
                   "dfmi_set_option: " + k + " must be a species index, or -1 (not considered)");
      else
        DFMI_CHECK(value > 0 && value <= 1.79769313486231570e308, "dfmi_set_option: " + k + " must be positive and finite");
      if ((k == "tci.model" || k == "tci.chemistry") && value != x.opt(key)) tci_reset_tc(x);
      DFMI_CHECK(k != "tci.model" || value == 0.0 || !x.fgm.model,
                 "dfmi_set_option: tci.model != 0 and fgm.model = 1 exclude each other (one combustion model at a time)");
      if (k == "tci.model") x.tci.model = (int)value;
    }
    if (k.rfind("spray.", 0) == 0) {
      if (k == "spray.model") {
        DFMI_CHECK(value == 0.0 || value == 1.0, "dfmi_set_option: spray.model must be 0 (no cloud, or not coupled) or 1 (active and coupled)");
        DFMI_CHECK(value == 0.0 || !x.fgm.model, "dfmi_set_option: spray.model = 1 is not available with fgm.model = 1 (the flareFGM spray branch is not on the device)");
        DFMI_CHECK(value == 0.0 || !x.thermo.eos,
                   "dfmi_set_option: spray.model = 1 is not available with an equation of state set (dfmi_thermo_set_eos model 1)");
        if (value == 1.0 && x.have_sizes) ensure_spray_fields(x);
        x.spray.model = (int)value;
      } else {
        DFMI_CHECK(value == 0.0 || value == 1.0, "dfmi_set_option: " + k + " must be 0 (explicit) or 1 (semiImplicit)");
        x.spray.sch[k == "spray.rho" ? 0 : k == "spray.U" ? 1 : k == "spray.Yi" ? 2 : 3] = (int)value;
      }
    }
    x.opts[k] = value;
  });
}

int dfmi_get_option(dfmi_ctx* ctx, const char* key, double* value) {
  return guard([&] {
    Ctx& x = ctx->x;
    *value = x.opt(key);
    if (std::string(key) == "tci.bad_tauStar" && x.tci.bad.n) {   // the last EDC correct's count, read back from the device
      int nb = 0;
      DFMI_HIP(hipStreamSynchronize(x.stream));
      DFMI_HIP(hipMemcpy(&nb, x.tci.bad.p, sizeof(int), hipMemcpyDeviceToHost));
      *value = nb;
    }
  });
}

int dfmi_set_preconditioner(dfmi_ctx* ctx, const char* eqn, const char* name) {
  return guard([&] {
    std::string e(eqn), n(name);
    DFMI_CHECK(e == "U" || e == "Y" || e == "E" || e == "p" || e == "k" || e == "epsilon" || fgm_eq_index(e) >= 0, "unknown equation '" + e + "'");
    DFMI_CHECK(n == "jacobi" || (n == "amg" && e == "p"), "preconditioner must be 'jacobi' or ('amg' for p)");
    ctx->x.solver[e].precond = n == "amg" ? 1 : 0;
  });
}

int dfmi_solver_stats(dfmi_ctx* ctx, const char* eqn, int* iters, double* res0, double* rel) {
  return guard([&] {
    const SolveStats st = solve_stats(ctx->x, eqn);
    if (iters) *iters = st.iters;
    if (res0) *res0 = st.res0;
    if (rel) *rel = st.res;
  });
}

int dfmi_solver_work(dfmi_ctx* ctx, const char* eqn, double* iters, int reset) {
  return guard([&] {
    const double v = solver_work(ctx->x, eqn, reset != 0);
    if (iters) *iters = v;
  });
}

namespace {
void set_comm(Ctx& x, int nranks, int rank, const int* neighb) {
  DFMI_CHECK(x.have_sizes, "call dfmi_set_constant_values first");
  DFMI_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank / nranks");
  x.nranks = nranks;
  x.rank = rank;
  x.peer.assign(neighb, neighb + x.P);
  // overlapped solver halos: the option halo.overlap (read per solve); the environment sets its default here
  const char* e = std::getenv("DFMI_HALO_OVERLAP");
  if (e && !x.opts.count("halo.overlap")) x.opts["halo.overlap"] = std::atoi(e) != 0 ? 1.0 : 0.0;
}
// the exchange lists need the boundary topology: built now, or at the end of
// dfmi_init_constant_fields_boundary (every rank reaches both points in the same order)
void maybe_setup_halo(Ctx& x) {
  if (!x.halo || !x.have_bgeom) return;
  int nproc = 0;
  for (int p = 0; p < x.P; ++p) if (x.pkind[p] == 2) nproc += x.psize[p];
  DFMI_CHECK(nproc == x.nproc_faces, "num_proc_surfaces differs from the processor patch sizes");
  halo_setup(x);
}
}  // namespace

int dfmi_set_comm_info(dfmi_ctx* ctx, const void* uid, int nranks, int rank, const int* neighb) {
  return guard([&] {
    Ctx& x = ctx->x;
    set_comm(x, nranks, rank, neighb);
    halo_init_rccl(x, uid, nranks, rank);
    maybe_setup_halo(x);
  });
}

int dfmi_set_comm_local(dfmi_ctx* ctx, int hub_id, int nranks, int rank, const int* neighb) {
  return guard([&] {
    Ctx& x = ctx->x;
    set_comm(x, nranks, rank, neighb);
    halo_init_local(x, hub_id, nranks, rank);
    maybe_setup_halo(x);
  });
}

int dfmi_get_unique_id(void* out) { return guard([&] { rccl_unique_id(out); }); }

int dfmi_renumber_cells(int num_cells, const double* cell_centres, int num_faces, const int* owner,
                        const int* neighbour, const char* method, int* new_to_old) {
  return guard([&] { renumber_cells(num_cells, cell_centres, num_faces, owner, neighbour, method, new_to_old); });
}

int dfmi_renumber_faces(int num_cells, int num_faces, const int* owner, const int* neighbour,
                        const int* cell_new_to_old, int* face_new_to_old, int* new_owner, int* new_neighbour,
                        int* flipped) {
  return guard([&] {
    renumber_faces(num_cells, num_faces, owner, neighbour, cell_new_to_old, face_new_to_old, new_owner, new_neighbour,
                   flipped);
  });
}

}  // extern "C"
