// dfmi_ctx.h -- the device-resident database (the MI355X counterpart of dfMatrixDataBase,
// reference src_gpu/dfMatrixDataBase.H:97-324) plus per-equation workspaces.
//
// HBM layout (all fp64 values SoA, int32 indices):
//   cells: scalar [C]; vector [3][C]; tensor [9][C]; species [S][C] (species-major)
//   faces: [F]; vectors [3][F]
//   boundary slots: [B] in OpenFOAM patch order, processor patches take 2n slots
//                   [neighbour values n | patch-internal values n] (createGPUSolver.H:118-123)
// Topology for deterministic cell gathers (no FP atomics anywhere):
//   ownStart[C+1]           faces owned by c are [ownStart[c], ownStart[c+1]) (upper-triangular order)
//   nbrStart[C+1], nbrFace  faces whose neighbour is c, ascending face index (losort)
// Face STORAGE: every face array lives in "owner-slot" order when the mesh allows it (at most a few
// faces owned per cell, e.g. hex meshes: 3): the k-th face owned by cell c at k*C + c. A wavefront of
// consecutive cells then reads and writes its k-th owned faces as one contiguous run (OpenFOAM order
// interleaves each cell's 3 faces: stride-3 partial lines that the L2 evicts between the three
// visits), and a cell's neighbour-side faces are the owned faces of consecutive cells too. Padding
// slots have own = -1. The API keeps OpenFOAM face order: face fields and lower/upper are mapped
// through h_fst (face -> storage) at the boundary. Meshes with many owned faces per cell keep face order.
//   cbStart[C+1], cbSlot    primary boundary slots of c, ascending slot index
// Visiting nbrFace, then own faces, then cbSlot is exactly OpenFOAM's sequential face order.
#pragma once
#include "dfmi_common.h"
#include "amg.h"
#include <map>
#include <memory>

namespace dfmi {

constexpr int SCODE_PAD = -1;   // row-class source code of a padding entry (esrc PAD; build_ell's class key)

struct MeshView {
  int C, F, B, S;
  const int *own, *nei, *ownStart, *nbrStart, *nbrFace, *cbStart, *cbSlot, *bfc, *partner;
  int fslot;                // face storage in owner-slot order (k*C + c) rather than OpenFOAM order
  const int8_t* sprim;   // != 0: primary slot (2: of a processor patch towards a lower rank), 0 = processor [internal n] slot
  const double *Sf, *magSf, *w, *dc, *V, *bSf, *bmagSf, *bw, *bdc;
  // solver gather rows [W][C] (linsolve.hip build_ell): the face loops read them. Entry k of cell c's row is
  // column ecol[k C + c] and coefficient source esrc[k C + c] (2 f + own for the face at storage f, -(b + 1)
  // for boundary slot b, INT_MIN padding)
  const int *ecol, *esrc;
  int W;
  double rdt;
  // hex box in blockMesh order (cell c = i + nx (j + ny k), internal faces towards +x/+y/+z in owner-slot
  // storage, build_ell checked every row against it): the face walk computes face and neighbour indices
  // instead of loading them (each_face<-1>); hx = 0: not such a mesh
  int hx, hy, hz;
  const int* trav;          // optional traversal order of the per-cell gather kernels (thread t -> cell)
  const double *md, *bdv;   // C[nei] - C[own] [3][F] (face storage) and patch delta vectors [3][B] (limited schemes)
  // even-odd solver layout (Ctx::Ell::eo): row index of cell c in the BiCGStab rows / vectors (first the
  // colour-0 cells, then colour-1, each ascending); nullptr: natural order. Only the writers of the
  // BiCGStab rows (k_ell_build for U/E, k_y_assemble_ell) read it.
  const int* eopos;
};

// interpolation / convection schemes of the terms the reference GPU path hard-wires (dfmi_set_scheme;
// dfmi/schemes.py): div(phi,Yi_h), div(phi,K), div(hDiffCorrFlux)
enum SchemeKind { SCH_UPWIND = 0, SCH_LINEAR = 1, SCH_LL = 2, SCH_LL01 = 3, SCH_CUBIC = 4, SCH_LLV = 5 };
struct Schemes {
  int yh = SCH_UPWIND, K = SCH_LINEAR, hD = SCH_LINEAR, U = SCH_LINEAR;
  double k_yh = 1.0, k_K = 1.0, k_U = 1.0;
  int tk = SCH_UPWIND, teps = SCH_UPWIND;   // div(phi,k), div(phi,epsilon) (RAS)
  double k_tk = 1.0, k_teps = 1.0;
  // div(phi,Z), div(phi,Zvar), div(phi,c), div(phi,cvar), div(phi,Zcvar), div(phi,Ha) (flareFGM; fgm_eq_names order)
  int fgm[6] = {SCH_UPWIND, SCH_UPWIND, SCH_UPWIND, SCH_UPWIND, SCH_UPWIND, SCH_UPWIND};
  double k_fgm[6] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
};
// the flareFGM transport equations in the order they are solved (baseFGM::transport(), baseFGM.C:736-904)
constexpr int FGM_NEQ = 6;
inline const char* fgm_eq_name(int e) {
  static const char* n[FGM_NEQ] = {"Z", "Zvar", "c", "cvar", "Zcvar", "Ha"};
  return n[e];
}
inline int fgm_eq_index(const std::string& s) {
  for (int e = 0; e < FGM_NEQ; ++e) if (s == fgm_eq_name(e)) return e;
  return -1;
}

struct Field {
  DevBuf<double> buf;
  long n = 0;       // values per component (device storage; faces: Fs)
  int ncomp = 1;
  bool boundary = false;
  bool face = false;  // internal-face field: API order F, device storage Fs (Ctx::h_fst)
};

// one assembled fvMatrix (LDU + boundary coefficients), reference storage convention
struct Matrix {
  int nsys = 1;                 // species batch for Y
  DevBuf<double> lower, upper, diag, source, ic, bc;
  DevBuf<double> source_solve;  // U only: source incl. -grad(p)
};

struct SolverCfg {
  int max_iter = 20;
  double tol = 1e-5;           // relative to the initial residual (AmgX RELATIVE_INI, amgxUOptions)
  double abs_tol = 0.0;
  int precond = 0;             // 0 Jacobi, 1 aggregation AMG (p only)
};

struct SolveStats { int iters = 0; double res0 = 0, res = 0; };

struct Thermo {
  int S = 0;
  std::vector<double> W, nasa, visc, cond, bdiff, vc1, vc2;
  DevBuf<double> dW, drW, dnasa, dvisc, dcond, dbdiff, dvc1, dvc2;   // drW = 1 / W
  std::vector<double> hc;        // Hf298_i / W_i [J/kg]: the heat-release weights (dfChemistryModel.C:335-338)
  DevBuf<double> dhc;
  // species-minor copies for the cooperative S > 16 kernel (lanes own consecutive species i, so a
  // coefficient load over a group is one contiguous run): nasa [15][S], bdiff [j][5][i], vc [j][i]
  DevBuf<double> dnasaT, dbdiffT, dvc1T, dvc2T;
  // the same kernel's packed forms: vc1 / vc2 interleaved [j][i][2] (one 16-B load per pair), and, for a symmetric
  // binary-diffusion table, its unique pairs in rotation order [d - 1][i][6] = coefficients of the pair
  // (i, (i + d) mod S), d = 1 .. S / 2, padded to 6 (three 16-B loads)
  DevBuf<double> dvcP, dbdR;
  // equation of state (dfmi_thermo_set_eos): 0 ideal gas, 1 Peng-Robinson with the species' a [Pa m^6 / kmol^2],
  // b [m^3 / kmol] and acentric factor; on the device sqrt(a_i), kappa_i, 1 / sqrt(Tc_i) and b_i (thermo_eos_upload)
  int eos = 0;
  std::vector<double> eos_a, eos_b, eos_w;
  DevBuf<double> dsqa, dkap, drsTc, deb;
};

// flareFGM flamelet table (dfmi_fgm_set_table; fgm.hip). On the device the NS + NY value tables are stored
// corner-major, tab[loc (NS + NY) + variable]: the variables of one table corner are one contiguous run, so a lane's 64
// corner gathers each touch one or two lines whatever the number of variables it reads there. d2Yeq / d1Yeq interleaved.
struct Fgm {
  int model = 0;                 // option fgm.model
  bool have_table = false, scaled = true;
  int n[6] = {0, 0, 0, 0, 0, 0}; // NH NZ NC NGZ NGC NZC
  int NS = 0, NYomega = 0, NY = 0, NZL = 0;
  long N = 0;                    // entries of one value table
  double Hfu = 0, Hox = 0;
  DevBuf<double> axes;           // the six axes, one after the other
  DevBuf<double> lam;            // [5][NH NZL]: z, sl, th, tau, kctau
  DevBuf<double> tab;            // [N][NS + NY]
  DevBuf<double> dyeq;           // [NH NZ NGZ][2]: d2Yeq, d1Yeq (scaled PV only)
  DevBuf<int> ysp;               // mechanism index of each table species [NY]
  std::vector<int> h_ysp, h_osp; // and of the NYomega source species (host: names of omega_Yi's components)
};

struct Halo;   // RCCL processor-patch exchange (halo.hip)

// DF-ODENet surrogate (dnn.hip): S-1 MLPs, fp16 weights per layer [module][out][Kpad], fp32 biases
struct Dnn {
  bool ready = false;
  int nmod = 0;
  std::vector<int> dims, Kp;
  std::vector<DevBuf<_Float16>> W;
  std::vector<DevBuf<float>> b;
  DevBuf<double> xmu, xstd, ymu, ystd;
  double T_react = 610.0, dt = 1e-6;      // unReactT_ (dfChemistrySolver.cu:90), RR divisor (:191)
  int chunk = 65536;                      // reacting cells per inference batch
  int last_reacting = 0;
  double gemm_flops = 0;                  // algorithmic GEMM flops issued since the last query
  DevBuf<int> bc, idx;
  DevBuf<_Float16> x0, h0, h1;
  DevBuf<float> part;           // fused output layer: per-row partial dot products [net][2 N tiles][chunk]
  // reacting-cell count: compacted at the start of the time step (T is frozen until correctThermo) and
  // copied to pinned memory behind an event, read by dnn_solve after the UEqn solve's polls -- no drain
  PinnedBuf<int> nr_host;
  hipEvent_t nr_ev = nullptr;
  bool prepared = false;
  ~Dnn() { if (nr_ev) (void)hipEventDestroy(nr_ev); }
};

// per-cell chemistry (chem.hip): mechanism arrays (dfmi/kinetics.py layout) and integrator controls
struct Chem {
  bool ready = false;
  int mode = 0;                 // 0 off, 1 stiff ODE integration, 2 DNN surrogate
  int R = 0, ndd = 0;
  DevBuf<int> idata, irs;
  DevBuf<double> dd;
  double rtol = 1e-6, atol = 1e-10, Tmin = 0.0;   // CVODE settings of the reference (CanteraTorchProperties)
  int max_steps = 100000;
  int method = 0;               // 0 ROS3 Rosenbrock, 1 linearly-implicit Euler extrapolation
  int generated = 0;            // last solve used a compiled-in mechanism (chem_gen_*.inc): 1 burke9, 2 es80; -1: the cooperative kernel
  int bin = 2;                  // order cells by the previous solve's step count (option chem.binning: 0 natural order, 1 whole mesh, 2 per tile)
  DevBuf<int> perm, bcnt;       // cost-binned cell order; per-block bucket counts / offsets
  DevBuf<int> sp_off, sp_ent;   // cooperative kernel: per-species reaction lists (offsets [S + 1], reaction * 8 + slot)
  DevBuf<double> sp_nu;         // and their signed stoichiometric coefficients
  DevBuf<int> sp_rec_i;         // the same entries as self-contained records (chem.hip CoopList)
  DevBuf<double> sp_rec_d;
  std::vector<int> h_idata, h_irs;
  std::vector<double> h_dd;
  DevBuf<int> fail;             // cells of the last solve that hit max_steps (device counter)
  PinnedBuf<int> fail_host;     // its copy, behind fail_ev
  hipEvent_t fail_ev = nullptr;
  bool fail_pending = false;
  bool batch = false;           // dfmi_zero_d_step's loop: the counter sums over the batch, read once at its end
  ~Chem() { if (fail_ev) (void)hipEventDestroy(fail_ev); }
};

// HIP-event timing of one named kernel (dfmi_kernel_timer / dfmi_kernel_time)
struct KernelTimer {
  std::vector<std::string> targets;   // armed kernel names
  std::vector<hipEvent_t> pool;       // pairs (start, end)
  std::vector<int> rec;               // target index of each recorded pair
  size_t used = 0;
  ~KernelTimer() { for (auto e : pool) (void)hipEventDestroy(e); }
  hipEvent_t next() {
    if (used == pool.size()) {
      hipEvent_t e;
      DFMI_HIP(hipEventCreate(&e));
      pool.push_back(e);
    }
    return pool[used++];
  }
};

// Per-step timing (dfmi_step_timer / dfmi_step_times): while armed, dfmi_time_step records an event on the
// context stream before its first step and after every step (no synchronisation), so the bench reads each
// step's duration -- end of step i to end of step i-1 -- and reports their median beside the bracketed mean.
// The events form a ring of CAP marks, so an armed timer holds a bounded number of events however many steps
// run; dfmi_step_times reports the last CAP - 1 intervals. A step that fails resets the ring (its end mark is
// never recorded, and an interval spanning two steps must not be reported).
struct StepTimer {
  static constexpr size_t CAP = 1024;
  bool on = false;
  std::vector<hipEvent_t> ev;         // mark m at ev[m % CAP]: m = 0 before the first armed step, m = i after step i
  size_t used = 0;                    // marks recorded since arming (or since the last failed step)
  ~StepTimer() { for (auto e : ev) (void)hipEventDestroy(e); }
  void mark(hipStream_t s) {
    const size_t slot = used % CAP;
    if (slot == ev.size()) {
      hipEvent_t e;
      DFMI_HIP(hipEventCreate(&e));
      ev.push_back(e);
    }
    DFMI_HIP(hipEventRecord(ev[slot], s));
    ++used;
  }
  hipEvent_t at(size_t m) const { return ev[m % CAP]; }
};

// Communication accounting per exchange point (dfmi_comm_timer / dfmi_comm_report): every transport call
// of a halo exchange (ncclSend/ncclRecv group) or an all-gather, HIP events around it on the stream it is
// issued on (the compute stream, or the halo's comm stream for overlapped exchanges), with the bytes this
// rank sends, keyed by the exchange point that issued it (Ctx::comm.tag, set by the callers: the field
// names of a boundary-field exchange, the solver and its vectors). The reference's counterparts are the
// per-field NCCL groups of dfMatrixOpBase.cu:441-485 / 2402-2491, timed only by its TIME_GPU host ticks.
struct CommStats {
  bool on = false;
  std::string tag;
  struct Entry { long calls = 0; double bytes = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; };
  std::map<std::string, Entry> pts;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  hipEvent_t next() {
    if (used == pool.size()) {
      hipEvent_t e;
      DFMI_HIP(hipEventCreate(&e));
      pool.push_back(e);
    }
    return pool[used++];
  }
  void reset() { pts.clear(); used = 0; }
  ~CommStats() { for (auto e : pool) (void)hipEventDestroy(e); }
};

// Implementation options (dfmi_set_option; the role the reference's amgx*Options files and
// CanteraTorchProperties switches play for its solvers): the AMG configuration of the p solver, the solver
// and face-walk choices, the chemistry integrator. Every key and its default is listed here; an unknown key is
// an error. They are read when the structure they shape is built (the AMG hierarchy and the solver rows at
// the first solve) or at each call (everything else).
struct OptDef { const char* key; double def; };
inline const OptDef* option_defs(int& n) {
  static const OptDef d[] = {
    {"amg.omega", 0.9},               // weighted-Jacobi smoothing weight (0.85 -> 0.9: 13 -> 12 p-iterations)
    {"amg.overcorrection", 1.4},      // coarse-correction scaling of the plain-aggregation V-cycle
    {"amg.coarsest_sweeps", 6},       // Jacobi sweeps on the coarsest level (amgxpOptions coarsest_sweeps; 2 in the
                                      // reference's AmgX hierarchy). 1.35 / 8 -> 1.4 / 6: 13.88 -> 13.74 and 13.92 -> 13.81
                                      // ms per step, 3 rounds each in two calls (profiles/r06_ab_misc.txt r06m / r06n)
    {"amg.coarsest_size", 512},       // coarsening stops at this many cells
    {"amg.presweeps", 1},             // level-0 pre- and post-sweeps (amgxpOptions presweeps / postsweeps)
    {"amg.pairwise_passes_l0", 3},    // pairwise-matching passes building level 1 (3: 2x2x2 aggregates; SIZE_2 x 3)
    {"amg.pairwise_passes", 3},       // ... building the levels below
    {"amg.precision", 32},            // 32: V-cycle in fp32 (AmgX mixed mode), 64: fp64
    {"amg.padded", 1},                // coarse levels in aligned groups of 8 per aggregate (one launch per level)
    {"amg.tail", 1},                  // the last two levels in one workgroup launch (k_vtail)
    {"amg.halo_l0", 1},               // several ranks: level 0 keeps its processor couplings
    {"amg.global_coarse", 0},         // several ranks: one agglomerated coarsest level
    {"amg.reuse_steps", 8},           // > 1: the first corrector reuses the V-cycle operators of up to this many - 1
                                      // earlier steps (1: rebuilt every step). 1 -> 8: 13.59 -> 13.42 ms per step, 3
                                      // rounds each, 674 against 678 p system-iterations in 28 steps (r06u)
    {"amg.smoother", 0},              // 0: weighted Jacobi; 1: multicolour DILU (amgxpOptions smoother=MULTICOLOR_DILU)
    {"amg.reuse", 1},                 // later correctors of a time step precondition with the step's first V-cycle
                                      // operators (level-0 fp32 copy, Galerkin levels) instead of rebuilding them
    {"solver.even_odd", 1},           // U/Y/E: BiCGStab on the even-odd Schur complement where the rows 2-colour
    {"solver.small", 1},              // one rank, <= 4096 cells: every solve in one workgroup
    {"solver.row_classes", 1},        // solver rows decoded from one byte per cell where the mesh allows
    {"pcg.face_form", 1},             // one rank, hex box: the p operator read face-wise
    {"pcg.fuse_l0", 1},               // the PCG update fused with the V-cycle's level-0 first sweep
    {"pcg.fuse_setup", 1},            // face-form PCG with the reused V-cycle: the pEqn's cell pass (diag, source), dS / rhs,
                                      // the copy of p and the first residual in one launch (k_p_setup_fused)
    {"fv.hex_walk", 1},               // hex box in blockMesh order: face and neighbour indices computed
    {"fv.csr_walk", 0},               // assembly faces walked from the CSR lists instead of the gather rows
    {"fv.species_generic", 0},        // the species-chunked YEqn kernels at any species count (S > 16 always)
    {"fv.yprep_brick", 1},            // k_y_prep staging 16x4x4 bricks in LDS (hex walk)
    {"fv.p_post_fused", 1},           // owner-slot face storage: k_p_cell_post also writes phi of the cell's owned faces
                                      // (no k_p_flux_face pass)
    {"chem.method", 0},               // 0: ROS3 Rosenbrock, 1: linearly-implicit Euler extrapolation
    {"chem.generated", 1},            // compiled-in kinetics when the mechanism's fingerprint matches
    {"chem.binning", 2},              // cells launched in cost-binned order: 1 over the mesh, 2 inside 4096-cell tiles
    {"chem.coop", 0},                 // 1: the cooperative kernel (several lanes per cell) for any S >= 4; always on above 12 species
    {"chem.coop_lanes", 0},           // its lanes per cell: 0 by species count, or 16 / 32 / 64 (measurement)
    {"dnn.tuned_gemm", 1},            // DF-ODENet layers by the shape-tuned kernels (0: k_mlp_gemm for every layer)
    {"halo.overlap", 0},              // several ranks: solver halo exchanges on a comm stream while the interior rows run
                                      // (read per solve; DFMI_HALO_OVERLAP sets the default when the communicator is set)
    {"step.hbya_early", 1},           // one rank, two-stream step: the first corrector's HbyA right after the U solve, while the
                                      // main stream would wait for the side stream's YEqn rows (it reads what the U solve left)
    {"step.courant", 0},              // 1: dfmi_time_step ends with the Courant-number kernel and posts its record for
                                      // dfmi_courant_no (compressibleCourantNo.H, dfLowMachFoam.C:261); 0: nothing added
    {"les.model", 0},                 // turbulence->: 0 laminar, 1 Smagorinsky, 2 WALE (LESeddyViscosity),
                                      // 4 Sigma, 5 dynamicSmagorinsky (the reference's own); 3 is reserved and refused
    {"les.Ck", 0.094},                // nut = Ck delta sqrt(k) (both models)
    {"les.Ce", 1.048},                // Smagorinsky
    {"les.Cw", 0.325},                // WALE
    {"les.Csg", 1.5},                 // Sigma: nut = (Csg delta)^2 Dsg (Sigma.C:84, default :118-126)
    {"les.Prt", 1.0},                 // alphaEff = alpha + mut / Prt (createFields.H:133)
    {"les.Sct", 1.0},                 // DEff_i = rhoD_i + mut / Sct
    {"ras.model", 0},                 // turbulence->: 0 none, 1 kEpsilon (RAS; include/dfmi.h)
    {"ras.Cmu", 0.09},                // nut = Cmu k^2 / epsilon
    {"ras.C1", 1.44},                 // epsilon production
    {"ras.C2", 1.92},                 // epsilon destruction
    {"ras.C3", 0.0},                  // epsilon dilatation term ((2/3) C1 - C3) rho divU; any finite value
    {"ras.sigmak", 1.0},              // Dk = rho (nut / sigmak + mu / rho)
    {"ras.sigmaEps", 1.3},            // Deps = rho (nut / sigmaEps + mu / rho)
    {"ras.kMin", 1e-15},              // bound(k, kMin)
    {"ras.epsilonMin", 1e-15},        // bound(epsilon, epsilonMin)
    {"ras.Prt", 1.0},                 // alphaEff = alpha + mut / Prt (RAS mode)
    {"ras.Sct", 1.0},                 // DEff_i = rhoD_i + mut / Sct (RAS mode)
    {"tci.model", 0},                 // combustion->correct(): 0 none (laminar), 1 PaSR, 2 EDC (include/dfmi.h)
    {"tci.mixing", 1},                // PaSR mixingScale: 1 globalScale, 2 kolmogorovScale, 3 geometriMeanScale
    {"tci.chemistry", 1},             // PaSR chemistryScale: 1 globalConvertion, 2 formationRate, 3 reactionRate
    {"tci.Cmix", 0.1},                // globalScale: tmix = Cmix k / epsilon
    {"tci.fuel", -1},                 // globalConvertion species indices; -1: not considered
    {"tci.oxidizer", -1},
    {"tci.CO2", -1},
    {"tci.H2", -1},
    {"tci.version", 2005},            // EDC: 1981, 1996, 2005, 2016
    {"tci.C1", 0.05774},              // EDC v2016
    {"tci.C2", 0.5},
    {"tci.Cgamma", 2.1377},           // EDC
    {"tci.Ctau", 0.4083},
    {"tci.exp1", 0},                  // EDC exponents: 0 the version's own, otherwise 1..4
    {"tci.exp2", 0},
    {"tci.bad_tauStar", 0},           // get only: cells of the last EDC correct whose tauStar was not positive and finite
    {"fgm.model", 0},                 // combustion->correct(): 0 none, 1 flareFGM (include/dfmi.h)
    {"fgm.combustion", 0},            // flareFGMCoeffs combustion: the c, cvar and Zcvar equations and the source lookups
    {"fgm.solveEnthalpy", 0},         // the Ha equation (off: Ha = Z (Hfu - Hox) + Hox)
    {"fgm.flameletT", 0},             // T from the table (off: (Ha - Hf) / Cp + 298.15)
    {"fgm.Sct", 0.7},                 // D = mut / Sct + mu / Sc
    {"fgm.Sc", 1.0},
    {"fgm.incompPref", -10.0},        // > 0: rho = incompPref psi; otherwise rho = p psi
    {"fgm.TMin", 200.0},              // T clipped to [TMin, TMax]
    {"fgm.TMax", 5000.0},
    {"spray.model", 0},               // the Lagrangian cloud's active && coupled: 1 adds the parcel source terms to the rho,
                                      // U, Yi and he equations (include/dfmi.h, spray block)
    {"spray.rho", 0},                 // sourceTerms.schemes of sprayCloudProperties: 0 explicit, 1 semiImplicit
    {"spray.U", 0},
    {"spray.Yi", 0},
    {"spray.h", 0},
    {"p.n_nonorth", 0},               // nNonOrthogonalCorrectors (system/fvSolution PIMPLE): extra passes of the pEqn's
                                      // non-orthogonal corrector loop (pEqn.H:51-62)
  };
  n = (int)(sizeof(d) / sizeof(d[0]));
  return d;
}

// Courant number (fv_kernels.hip courant_post; dfmi_courant_no): the record the last kernel of the reduction stores
// into host-coherent pinned memory, `seq` last (system-scope release), as the solvers' PollRec
struct CoRec { double co, mean; long long seq; };
struct Courant {
  CoRec* h = nullptr;
  CoRec* d = nullptr;
  long long seq = 0;          // records queued so far
  bool fresh = false;         // the last queued record describes the fields and the step size as they stand
  double sumV = 0;            // sum of this rank's cell volumes, in cell order (constant: summed once at setup)
  DevBuf<double> partial, tri, all;   // per-block (sum, max); this rank's (max, sum, volume); every rank's
  Courant() = default;
  Courant(const Courant&) = delete;
  Courant& operator=(const Courant&) = delete;
  ~Courant() { if (h) (void)hipHostFree(h); }
  void ensure() {
    if (h) return;
    DFMI_HIP(hipHostMalloc((void**)&h, sizeof(CoRec), hipHostMallocCoherent | hipHostMallocMapped));
    h->co = 0; h->mean = 0; h->seq = 0;
    DFMI_HIP(hipHostGetDevicePointer((void**)&d, h, 0));
  }
};

struct Ctx {
  int device = 0;
  std::map<std::string, double> opts;   // dfmi_set_option overrides
  double opt(const char* key) const {
    auto it = opts.find(key);
    if (it != opts.end()) return it->second;
    int n;
    const OptDef* d = option_defs(n);
    for (int i = 0; i < n; ++i) if (std::string(d[i].key) == key) return d[i].def;
    throw Error(std::string("dfmi: unknown option '") + key + "'");
  }
  bool on(const char* key) const { return opt(key) != 0.0; }
  hipStream_t stream = nullptr;
  // sizes (dfMatrixDataBase::setConstantValues, dfMatrixDataBase.cu:114-147)
  int C = 0, Ctot = 0, F = 0, B = 0, P = 0, S = 0, nproc_faces = 0;
  int Fs = 0;                    // face storage size (owner-slot layout: kmax * C; otherwise F)
  bool fslot = false;
  std::vector<int> h_fst;        // OpenFOAM face -> storage index
  double rdt = 0;                // 1 / deltaT: what every kernel reads (MeshView::rdt, by value at each launch)
  double dt = 0;                 // deltaT as the caller gave it (dfmi_set_delta_t; 1 / rdelta_t at setup): dfmi_get_delta_t
                                 // and the Courant number
  Courant co;
  int inert = -1;
  bool have_sizes = false, have_topo = false, have_geom = false, have_bgeom = false;
  bool have_md = false;           // mesh_distance was given (the limited schemes' d; zeros otherwise)
  std::vector<int> psize, poff, pkind, cyc_nbr, peer;   // pkind: 0 plain, 1 cyclic, 2 processor
  std::vector<int> h_bfc, h_own, h_nei;
  // topology
  DevBuf<int> own, nei, ownStart, nbrStart, nbrFace, cbStart, cbSlot, bfc, partner;
  DevBuf<int8_t> sprim;
  // geometry
  DevBuf<double> Sf, magSf, w, dc, V, bSf, bmagSf, bw, bdc;
  DevBuf<double> md, bdv;        // mesh_distance [3][Fs], boundary delta [3][B] (dfmi_init_boundary_delta)
  bool have_bdelta = false;
  Schemes sch;
  // laplacian scheme (dfmi_set_scheme "laplacian"): LAP_ORTHOGONAL reads dc / bdc as the caller gave them;
  // the other two read the non-orthogonal delta coefficients (fields nonorth_delta_coeffs / boundary_nonorth_delta_coeffs,
  // formed on the device by nonorth_setup), LAP_CORRECTED adds the explicit term from the correction vectors
  // (nonorth_corr [3][Fs] / boundary_nonorth_corr [3][B]). The pointers are those fields' buffers (nullptr: orthogonal)
  int lap = 0;
  const double *no_dc = nullptr, *no_bdc = nullptr, *no_k = nullptr, *no_bk = nullptr;
  DevBuf<int> conv_list, conv_nlist;   // faces whose div(phi,Yi_h) limiter needs gradients (k_conv_w_check)
  // per-field patch types (host, per patch) and per-slot device copies
  std::map<std::string, std::vector<int>> ptype;
  std::map<std::string, DevBuf<int8_t>> stype;
  // fields
  std::map<std::string, Field> fields;
  // matrices
  Matrix mU, mY, mE, mP;
  Matrix mK;                     // the generic scalar transport assembly's (k_scalar_assemble: epsilon, then k); RAS mode only
  std::map<std::string, SolverCfg> solver;
  Thermo thermo;
  // scratch
  DevBuf<double> scratch;
  // domain decomposition (halo.cpp): processor patches exchange [neighbour n] slot values
  int nranks = 1, rank = 0, global_offset = 0;
  std::vector<int> h_proc_cols;  // procCols: global id of the cell across each processor face (patch order)
  int H = 0;                     // processor faces = halo values per component
  std::vector<int> h_hidx;       // per boundary slot: halo index of a primary processor slot, else -1
  Halo* halo = nullptr;          // owned; freed by halo_destroy()
  // solver gather (linsolve.hip): per cell W coupling entries, [W][C] (coalesced)
  struct Ell {
    int W = 0;
    bool ready = false;
    DevBuf<int> col;             // column: cell id, or C + halo index for a processor face
    DevBuf<int> src;             // coefficient: 2f = lower[f], 2f+1 = upper[f], -(b+1) = -boundaryCoeffs[b]
    DevBuf<int8_t> bflag;        // [C] 1: the row has a processor (halo) column
    DevBuf<int> brow;            // those rows, ascending
    int nb = 0;
    // row classes (ColView; built when the mesh has <= 255 distinct rows and owner-slot face storage;
    // option solver.row_classes = 0: explicit columns everywhere)
    DevBuf<uint8_t> cls;
    DevBuf<int> ctab;
    DevBuf<int> csStart, csSlot, scol;   // coupled slots per cell and their columns (FaceOp)
    int ncls = 0;
    ColView cols() const {
      ColView v;
      v.col = col.p; v.W = W;
      if (ncls > 0) { v.cls = cls.p; v.tab = ctab.p; v.ntab = ncls * W; }
      return v;
    }
    // even-odd (red-black) reduced BiCGStab (linsolve.hip): on a bipartite coupling graph (hex meshes) the
    // rows are stored colour by colour -- colour-0 cells [0, ne), colour-1 cells [ne, C) -- and the solver
    // iterates on the colour-1 Schur complement. eo_pos: cell -> row, eo_cell: row -> cell; eo_col: the
    // ELL columns in row numbering (every entry points into the other colour), with its own row classes
    int eo = 0, ne = 0;
    DevBuf<int> eo_pos, eo_cell, eo_col, eo_ctab;
    DevBuf<uint8_t> eo_cls;
    int eo_ncls = 0;
    std::vector<int> h_eo_pos;
    ColView eo_cols() const {
      ColView v;
      v.col = eo_col.p; v.W = W;
      if (eo_ncls > 0) { v.cls = eo_cls.p; v.tab = eo_ctab.p; v.ntab = eo_ncls * W; }
      return v;
    }
  } ell;
  Amg amg;                       // pressure preconditioner hierarchy (amg.hip)
  Chem chem;
  Dnn dnn;
  struct SolverWs {
    DevBuf<double> buf, scal, red_local, red_all;
    DevBuf<int> sysmap;
    HostRecs poll;                   // convergence records the device posts (linsolve.hip: Poller)
    long long poll_seq = 0;          // records posted so far
    long gen = 0;                    // bumped whenever a solve or an assembly rewrites buf (Amg::ws_gen)
  } ws, ws_y;
  // the YEqn batch has its own solver workspace (its rows are assembled while the UEqn solve may still be
  // running on the other stream, dfmi_time_step); linsolve.hip reaches the current one through sws()
  bool ws_is_y = false;
  SolverWs& sws() { return ws_is_y ? ws_y : ws; }
  // side stream of the time step (dfmi_time_step: chemistry + YEqn preparation beside the UEqn) and its events
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_u = nullptr, ev_e = nullptr, ev_cw = nullptr;
  // final solver state of the last solve of each equation, copied asynchronously at the end of the
  // solve; dfmi_solver_stats synchronises and reads it (no host sync inside a time step)
  struct StatSnap { PinnedBuf<double> h; int nsys = 0; };
  std::map<std::string, StatSnap> stat_snap;
  std::map<std::string, int> solve_expect;   // iterations of the last solve per equation (linsolve.hip Poller)
  DevBuf<double> work;           // per equation (U, Y, E, p): system-iterations, summed on the device
  DevBuf<double> work_ras;       // the same for epsilon and k (allocated by their first solve)
  DevBuf<double> work_fgm;       // the same for the six flareFGM equations (allocated by their first solve)
  KernelTimer ktimer;
  StepTimer steptimer;
  CommStats comm;
  DevBuf<int> trav;   // dfmi_set_traversal: the order threads visit cells in the gather kernels (empty: natural)
  int hex[3] = {0, 0, 0};   // MeshView::hx/hy/hz (build_ell)
  ~Ctx();
  int n_corr = 2;
  // LES eddy viscosity (options les.*, fv_kernels.hip turbulence_correct): the model in force (a copy of the option,
  // read at every launch), whether the field "nut" belongs to the model, delta and U as they stand, and whether the
  // fields the dropped terms read (sumYDiffError, hDiffCorrFlux, diffAlphaD, phiUc) have been zeroed for this mode
  struct Les { int model = 0; bool valid = false, zeroed = false, have_delta = false; } les;
  // RAS k-epsilon (options ras.*, fv_kernels.hip ras_*): the model in force, whether nut belongs to k and epsilon as
  // they stand, and which of k, epsilon, boundary_k, boundary_epsilon the caller has set
  struct Ras { int model = 0; bool valid = false; bool have[4] = {false, false, false, false}; } ras;
  // k-epsilon wall functions and turbulent inlets. Host, per patch: the wall function's coefficients, the
  // inlets' intensity and mixing length (0: never set). Device, allocated by the first patch type that needs them
  // (ras_wall_refresh): per slot the bits WF_* and the slot's patch, per patch the row {Cmu25, Cmu75, kappa, E,
  // yPlusLam, intensity, mixingLength, 0} of tab, per cell the epsilon equation's constraint flag.
  enum { WF_EPS_WALL = 1, WF_NUT_WALL = 2, WF_K_INLET = 4, WF_EPS_INLET = 8, WF_TAB = 8 };
  struct WallFn {
    std::vector<double> Cmu, kappa, E, intensity, mixingLength;
    bool in_use = false, dirty = true;
    int bits = 0;                  // the union of the slots' bits
    DevBuf<int8_t> sflag, cflag;   // [B], [C]
    DevBuf<int> spatch;            // [B]
    DevBuf<double> tab;            // [P][WF_TAB]
  } wf;
  // the one flag everything downstream of an eddy viscosity reads: either model sets it (the effective fields, the
  // dropped YEqn / EEqn terms, the LES instantiations of the assemblies)
  // combustion closure (options tci.*, chem.hip tci_*): the model in force; bad: the device count of EDC cells without a usable tauStar
  struct Tci { int model = 0; DevBuf<int> bad; } tci;
  Fgm fgm;                       // flareFGM: the table and the model in force (options fgm.*)
  // spray coupling (options spray.*, fv_kernels.hip spray_*): the model in force, the schemes of the rho, U, Yi and h
  // terms (0 explicit, 1 semiImplicit), and which of the cloud's transfer fields the caller has set (spray_field_name order)
  struct Spray { int model = 0; int sch[4] = {0, 0, 0, 0}; bool have[5] = {false, false, false, false, false}; } spray;
  // the chemistry source the YEqn assemblies read: the closure's kappa RR, or the chemistry's own RR
  double* rr_src() { return f(tci.model ? "RR_eff" : "RR"); }
  bool turbulent() const { return les.model != 0 || ras.model != 0; }
  // what the three assemblies read as mu / alpha: the thermo's fields, or in turbulent mode muEff / alphaEff (les_effective)
  double* visc(bool boundary) { return f(std::string(boundary ? "boundary_" : "") + (turbulent() ? "muEff" : "mu")); }
  double* cond(bool boundary) { return f(std::string(boundary ? "boundary_" : "") + (turbulent() ? "alphaEff" : "alpha")); }
  // mut / Sct, which the species kernels add where they read rhoD (nullptr: laminar)
  double* mut_sct(bool boundary) { return turbulent() ? f(boundary ? "boundary_mutSct" : "mutSct") : nullptr; }

  MeshView view() const {
    MeshView m;
    m.C = C; m.F = Fs; m.B = B; m.S = S; m.fslot = fslot ? 1 : 0;
    m.own = own; m.nei = nei; m.ownStart = ownStart; m.nbrStart = nbrStart; m.nbrFace = nbrFace;
    m.cbStart = cbStart; m.cbSlot = cbSlot; m.bfc = bfc; m.partner = partner; m.sprim = sprim;
    m.Sf = Sf; m.magSf = magSf; m.w = w; m.V = V; m.bSf = bSf; m.bmagSf = bmagSf; m.bw = bw;
    m.dc = lap ? no_dc : dc.p; m.bdc = lap ? no_bdc : bdc.p;
    m.ecol = ell.col; m.esrc = ell.src; m.W = ell.ready ? ell.W : 0;
    m.rdt = rdt;
    m.trav = trav.n ? trav.p : nullptr;
    m.hx = hex[0]; m.hy = hex[1]; m.hz = hex[2];
    m.md = md.p; m.bdv = bdv.p;
    m.eopos = ell.ready && ell.eo ? ell.eo_pos.p : nullptr;
    return m;
  }
  double* f(const std::string& name) {
    auto it = fields.find(name);
    DFMI_CHECK(it != fields.end(), "unknown field '" + name + "'");
    return it->second.buf.p;
  }
  const int8_t* st(const std::string& field) {
    auto it = stype.find(field);
    DFMI_CHECK(it != stype.end(), "patch types not set for field '" + field + "'");
    return it->second.p;
  }
  // scheme buffers (fv_kernels.hip scheme launchers): 0/1 div(phi,Yi_h) weights (faces / slots), 2/3
  // div(phi,K) weights, 4/5 cubic flux correction of div(hDiffCorrFlux); nullptr where the term keeps
  // the reference GPU path's scheme (upwind / linear / linear); 6/7 div(phi,U) limitedLinearV weights
  const double* sch_w(int i) {
    static const char* names[8] = {"conv_w", "boundary_conv_w", "K_w", "boundary_K_w", "cubic_flux",
                                   "boundary_cubic_flux", "U_w", "boundary_U_w"};
    const bool on = i < 2 ? sch.yh != SCH_UPWIND : i < 4 ? sch.K != SCH_LINEAR : i < 6 ? sch.hD == SCH_CUBIC && !turbulent()
                                                                                     : sch.U == SCH_LLV;
    if (!on) return nullptr;
    auto it = fields.find(names[i]);
    DFMI_CHECK(it != fields.end(), std::string("scheme buffer '") + names[i] + "' not computed");
    return it->second.buf.p;
  }
  const std::vector<int>& pt(const std::string& field) {
    auto it = ptype.find(field);
    DFMI_CHECK(it != ptype.end(), "patch types not set for field '" + field + "'");
    return it->second;
  }
};

// The YEqn workspace (Ctx::ws_y) for the scope's solver calls.
struct YWs {
  Ctx& x;
  bool prev;
  explicit YWs(Ctx& c) : x(c), prev(c.ws_is_y) { x.ws_is_y = true; }
  ~YWs() { x.ws_is_y = prev; }
};
// Launches of the scope go to stream s (the launchers all read Ctx::stream).
struct OnStream {
  Ctx& x;
  hipStream_t prev;
  OnStream(Ctx& c, hipStream_t s) : x(c), prev(c.stream) { x.stream = s; }
  ~OnStream() { x.stream = prev; }
};

// Records a start/end event pair around a launch when `name` is the armed kernel.
struct KScope {
  Ctx& x;
  int idx;
  static int match(const std::vector<std::string>& ts, const char* name) {   // template arguments ignored
    if (ts.empty() || !name) return -1;
    while (*name == '(') ++name;
    size_t n = 0;
    while (name[n] && name[n] != '<') ++n;
    for (size_t i = 0; i < ts.size(); ++i)
      if (ts[i].size() == n && ts[i].compare(0, n, name, n) == 0) return (int)i;
    return -1;
  }
  KScope(Ctx& c, const char* name) : x(c), idx(match(c.ktimer.targets, name)) {
    if (idx >= 0) { x.ktimer.rec.push_back(idx); DFMI_HIP(hipEventRecord(x.ktimer.next(), x.stream)); }
  }
  ~KScope() noexcept(false) { if (idx >= 0) DFMI_HIP(hipEventRecord(x.ktimer.next(), x.stream)); }
};

// ---- renumber.cpp (host): cell order for cache-local gathers, faces re-sorted upper-triangular
void renumber_cells(int num_cells, const double* cell_centres, int num_faces, const int* owner, const int* neighbour,
                    const char* method, int* new_to_old);
void renumber_faces(int num_cells, int num_faces, const int* owner, const int* neighbour, const int* cell_new_to_old,
                    int* face_new_to_old, int* new_owner, int* new_neighbour, int* flipped);

// ---- launchers (fv_kernels.hip)
void k_bc_correct(Ctx& x, const char* type_field, double* vf, double* bvf, int ncomp);
void rho_process(Ctx& x, bool write_matrix);
void u_assemble(Ctx& x);
void u_post_solve(Ctx& x);
void u_hbya(Ctx& x);
void p_assemble(Ctx& x, bool cell_pass = true);   // cell_pass = false: solve_pcg's fused setup writes diag and source
void p_post_solve(Ctx& x);
void y_prep(Ctx& x, bool weights = true);   // weights = false: the caller formed the div(phi,Yi_h) weights
void y_assemble(Ctx& x, bool spray = true);   // spray = false: the caller adds the parcel terms itself (spray_fold_y)
void y_assemble_ell(Ctx& x, int W, long Ce, double* val, double* dS, double* rhs);
// Spray coupling (include/dfmi.h, spray block): the cloud's transfer fields folded into an equation's diag /
// source as the last thing added to them. rho_process, u_assemble, y_assemble, y_assemble_ell and e_assemble_back call
// these themselves; with spray.model = 0 they return at once and launch nothing. spray_on: the model is in force, after
// the refusals (fgm.model, an equation of state, a required field never set). spray_fold_y: the species rows in LDU form
// (ell = false: diag / source [S][C]) or in the solver's (ell = true: dS / rhs [S - 1][Ce], even-odd positions).
inline const char* spray_field_name(int i) {
  static const char* n[5] = {"parcel_rhoTrans", "parcel_UTrans", "parcel_UCoeff", "parcel_hsTrans", "parcel_hsCoeffByCp"};
  return n[i];
}
bool spray_on(Ctx& x);
void spray_fold_y(Ctx& x, double* diag, double* source, long stride, bool ell);
void y_post_solve(Ctx& x);
void e_assemble(Ctx& x);
void e_assemble_front(Ctx& x);   // the scheme terms (independent of the Y solve)
void e_assemble_back(Ctx& x);    // boundary energy gradient, he's boundary values, the matrix
void e_post_solve(Ctx& x);
void conv_weights(Ctx& x);   // div(phi,Yi_h) weights (start of YEqn; EEqn reuses them)
void copy_old(Ctx& x);
// LES (options les.*): turbulence->correct() -- nut from grad(U) and delta, boundary_nut by nut's patch types, the
// processor slots' neighbour half through the halo; then Ctx::les.valid. Laminar: nothing.
void turbulence_correct(Ctx& x);
// mut = rho nut; muEff = mut + mu; alphaEff = alpha + mut / Prt; mutSct = mut / Sct, on cells and on every boundary
// slot from the slot's own values, from the fields as they stand (after the rhoEqn, before the three assemblies);
// the first call in LES mode also zeroes the fields of the dropped terms. Throws when nut is not valid.
void les_effective(Ctx& x);
// RAS k-epsilon (options ras.*; include/dfmi.h). ras_production: G and divU from U, phi, rho and the old nut.
// ras_assemble: one equation's sources, diffusivity and matrix (keq 0: epsilon, 1: k) into Ctx::mK from the fields as they
// stand. ras_post_solve: the solved field's boundary values, bound() and the halo. ras_nut: correctNut() -- nut = Cmu k^2 /
// epsilon on cells and slots, then Ctx::ras.valid. The solves between them are the caller's (capi.cpp ras_correct).
void ras_production(Ctx& x);
void ras_assemble(Ctx& x, int keq);
void ras_post_solve(Ctx& x, int keq);
void ras_nut(Ctx& x);
// Wall functions and turbulent inlets; every one returns at once in a context without the new patch types.
// ras_wall_refresh: the refusals (epsilonWallFunction without nutkWallFunction; inlets: an intensity or mixing length never
// set) and the per-slot / per-patch tables after a change. ras_inlet_k: boundary_k_ref from boundary_U. ras_wall_update:
// epsilon, G and boundary_epsilon of the wall cells, the constraint flags, boundary_epsilon_ref. ras_correct and
// dfmi_assemble call ras_inlet_k, ras_production, ras_wall_update in that order.
// flareFGM (include/dfmi.h, flareFGM block). fgm_set_table (fgm.hip): the checks and the upload. fgm_retrieve
// (fgm.hip): flareFGM::retrieval() on cells and slots, then the halo; write_rho = false leaves cell rho alone (the
// constructor's call, timeIndex 0). fgm_assemble (fv_kernels.hip): one transport equation's diffusivity, source and matrix
// into Ctx::mK from the fields as they stand. fgm_post_solve: boundary values, halo, the clip to the field's bounds.
// fgm_ha_from_z: Ha = Z (Hfu - Hox) + Hox on cells and slots. The solves between them are the caller's (capi.cpp fgm_correct).
void fgm_set_table(Ctx& x, const int* dims, const double* axes, double Hfu, double Hox, const double* laminar,
                   const double* tables, const double* d2Yeq, const double* d1Yeq, const int* species_index,
                   const int* omega_index);
void fgm_retrieve(Ctx& x, bool write_rho);
void fgm_assemble(Ctx& x, int eq);
void fgm_post_solve(Ctx& x, int eq);
void fgm_ha_from_z(Ctx& x);
void ras_wall_refresh(Ctx& x, bool inlets);
void ras_inlet_k(Ctx& x);
void ras_wall_update(Ctx& x);
// laplacian schemes. nonorth_setup: the non-orthogonal delta coefficients and correction vectors from Sf,
// mesh_distance and the patch deltas (surfaceInterpolation::makeNonOrthDeltaCoeffs / makeNonOrthCorrectionVectors).
// nonorth_p_correct: the pEqn's explicit term from the current p / boundary_p -- source = base + div of the face flux
// correction, which is kept for nonorth_p_flux (phi -= it on internal faces and coupled slots after p_post_solve).
enum { LAP_ORTHOGONAL = 0, LAP_UNCORRECTED = 1, LAP_CORRECTED = 2 };
void nonorth_setup(Ctx& x);
void nonorth_p_base(Ctx& x);
void nonorth_p_correct(Ctx& x);
void nonorth_p_flux(Ctx& x);
void courant_post(Ctx& x);   // queues the Courant-number reduction and its record (Ctx::co), no synchronisation
void zero_d_step(Ctx& x, double dt);   // df0DFoam loop body for every cell
void thermo_rho_from_psi(Ctx& x);
void thermo_psip0(Ctx& x);
void thermo_correct_psip_rho(Ctx& x);
// thermo.hip
void thermo_upload(Ctx& x);
void thermo_eos_upload(Ctx& x);   // the Peng-Robinson species constants from Thermo::eos_a / eos_b / eos_w
std::vector<double> heat_of_formation_per_mass(int S, const double* W, const double* nasa);   // hc_i (Qdot weights)
void thermo_correct(Ctx& x, bool from_T);
// boundary_heGradient on gradientEnergy slots of he (0 elsewhere)
void thermo_energy_gradient(Ctx& x);
// linsolve.hip
SolveStats solve_bicgstab(Ctx& x, const char* eqn, int nsys, const int* sys_map_host, const double* lower, long lstride,
                          const double* upper, long ustride, const double* diag, long dstride, const double* source,
                          long sstride, const double* ic, const double* bc, long bstride, const char* type_field,
                          double* xsol, long xstride, const SolverCfg& cfg, bool prebuilt = false);
void bicg_layout(Ctx& x, int nsys, double** val, double** dS, double** rhs);
void build_ell(Ctx& x);   // solver gather rows; also the face lists of the assembly kernels
void bicg_rows_from_ldu_Y(Ctx& x);
void bicg_rows_get(Ctx& x, int nsys, const std::string& part, double* host, long count);
bool species_generic(const Ctx& x);   // fv_kernels.hip: chunked kernels for S > 16 (or the option fv.species_generic)
// iterations / initial and final relative residual of the last solve of `eqn` (synchronises)
SolveStats solve_stats(Ctx& x, const std::string& eqn);
// system-iterations of the solves of `eqn` since the last reset (synchronises)
double solver_work(Ctx& x, const std::string& eqn, bool reset);
SolveStats solve_pcg(Ctx& x, const char* eqn, const double* lower, const double* upper, const double* diag,
                     const double* source, const double* ic, const double* bc, const char* type_field, double* xsol,
                     double* bxsol, const SolverCfg& cfg, bool fuse_setup = false);
// the p solve about to run takes the face-form path with the reused V-cycle (no ELL values written) and the option
// pcg.fuse_setup is on: the caller skips p_assemble's cell pass and passes fuse_setup = true
bool pcg_setup_fusable(Ctx& x, const SolverCfg& cfg);
// dnn.hip
void dnn_upload(Ctx& x, int nmod, int nlayers, const int* dims, const float* params, const double* xmu,
                const double* xstd, const double* ymu, const double* ystd, double T_react, double dt_infer);
double hbm_copy_gbs(Ctx& x, size_t bytes, int reps);   // measured device copy bandwidth (fv_kernels.hip)
void dnn_prepare(Ctx& x);   // reacting-cell compaction + count read-back, ahead of dnn_solve
void dnn_solve(Ctx& x, const char* rho_field);   // RR scaled by rho_field (reference: d_rho_old, dfYEqn.cu:449)
void dnn_plan(Ctx& x, int max_layers, int* n_layers, int* kinds);   // the kernel form dnn_solve takes per hidden layer
// chem.hip
void chem_upload(Ctx& x, int R, const int* idata, const int* irs, const double* dd);
// rho_field: the thermo density RR is scaled by (dfChemistryModel.C:771, problem.rhoi = rho_[celli]);
// inside dfmi_time_step that is rho_old (thermo.rho() before this step's rhoEqn), standalone "rho"
void chem_solve(Ctx& x, double dt, const char* rho_field);
// the same solve over a per-cell interval dt_cell[c] (EDC's chemistryPtr_->solve(tauStar)); a cell whose interval is not
// positive and finite gets RR = 0
void chem_solve_cells(Ctx& x, const double* dt_cell, const char* rho_field);
// combustion->correct() (PaSR.C:205-396, EDC.C:83-171; include/dfmi.h): tci.model = 0 is chem_solve(dt) alone
void combustion_correct(Ctx& x, double dt, const char* rho_field);
void combustion_pointwise(Ctx& x);   // dfmi_assemble("tci"): kappa, the time scales and the scaled source, no solve
void ensure_tci_fields(Ctx& x);
void tci_reset_tc(Ctx& x);
void chem_fail_snapshot(Ctx& x);
// throws when the last solve left cells at the step limit (waits on the snapshot event only)
void chem_check(Ctx& x);
// halo.hip
// One exchange point: cell values of each item's components are sent across processor faces and land
// in the receiver's neighbour slots (to_slots) or in the extended vector region [C, C+H) (solver vectors).
struct HaloItem {
  const double* cell;
  double* dst;
  int ncomp;
  long cstride, dstride;
  bool to_slots;
  bool split = false;   // the source vector is stored in the even-odd row order (Ell::eo): send value[eo_pos[cell]]
  int colour = -1;      // split vectors: -1 every processor face; k: only the faces whose sending cell has colour k
                        // (the next half-row pass reads no other halo entries; halo.hip Plan)
};
bool halo_active(const Ctx& x);
void halo_update(Ctx& x, const HaloItem* items, int n);
// overlapped form (solver SpMVs, Ctx::halo_overlap): the exchange runs on the halo's comm stream between
// halo_begin and halo_end; the compute stream meanwhile runs only work that touches no halo entry
bool halo_overlap(const Ctx& x);
void halo_begin(Ctx& x, const HaloItem* items, int n);
void halo_end(Ctx& x);
// the exchange point of the halo / all-gather calls made while it lives (communication accounting)
struct CommTag {
  Ctx& x;
  std::string prev;
  bool set;
  CommTag(Ctx& c, const std::string& t) : x(c), set(c.comm.on) { if (set) { prev = x.comm.tag; x.comm.tag = t; } }
  ~CommTag() { if (set) x.comm.tag = prev; }
};
inline void halo_fields(Ctx& x, const std::vector<const char*>& names) {
  if (!halo_active(x)) return;
  std::string tag;
  if (x.comm.on) {
    tag = "fields";
    for (const char* n : names) { tag += ' '; tag += n; }
  }
  CommTag _ct(x, tag);
  std::vector<HaloItem> it;
  for (const char* n : names) {
    const Field& f = x.fields.at(n);
    const Field& bf = x.fields.at(std::string("boundary_") + n);
    it.push_back({f.buf.p, bf.buf.p, f.ncomp, f.n, bf.n, true});
  }
  halo_update(x, it.data(), (int)it.size());
}
// allgather of `count` doubles per rank: recv[r * count + i]
void halo_allgather(Ctx& x, const double* send, double* recv, long count);
std::string comm_report(Ctx& x);   // JSON of the communication accounting (CommStats)
std::vector<int> halo_peers_of(const Ctx& x);   // neighbour rank of every halo index (processor face)
void halo_set_split(Ctx& x);   // the send map of split (even-odd) vectors, after build_ell decided the layout
void halo_setup(Ctx& x);   // builds the exchange lists after dfmi_set_comm_info / dfmi_set_comm_local
void halo_init_rccl(Ctx& x, const void* uid, int nranks, int rank);
void halo_init_local(Ctx& x, int hub_id, int nranks, int rank);
void rccl_unique_id(void* out);
void halo_destroy(Halo* h);

}  // namespace dfmi
