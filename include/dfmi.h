/* dfmi.h -- C ABI of the MI355X-native dfLowMachFoam GPU hot path.
 *
 * Drop-in replacement for the C++ class surface of the reference libdfMatrix.so
 * (show-me-code/deepflame-dev src_gpu/ *.H headers, driven from applications/solvers/dfLowMachFoam/
 * createGPUSolver.H and *_GPU.H). Each entry point names the reference method it replaces.
 *
 * Conventions (same as the reference):
 *  - host arrays are copied during the call, never retained;
 *  - vector/tensor fields: layout DFMI_AOS = OpenFOAM [n][3] / [n][9] (the reference permutes
 *    with permute_vector_h2d, dfMatrixOpBase.cu:18-38), DFMI_SOA = [3][n] / [9][n];
 *  - species fields are species-major [S][n] (createGPUSolver.H:482-500);
 *  - boundary arrays are concatenated in OpenFOAM patch order; a processor/processorCyclic patch
 *    takes 2n slots [neighbour values | patch-internal values] (createGPUSolver.H:118-123);
 *  - patch type codes: zeroGradient 0, fixedValue 1, coupled 2, empty 3, gradientEnergy 4,
 *    calculated 5, cyclic 6, processor 7, extrapolated 8, fixedEnergy 9, processorCyclic 10
 *    (dfMatrixDataBase.H:81-93), plus waveTransmissive 11 (p only; gamma via dfmi_set_patch_param,
 *    OpenFOAM-7 advectiveFvPatchField semantics with Euler ddt) and inletOutlet 12 (U, p, Y, K;
 *    inletValue in the field "boundary_<field>_ref") -- the mixed conditions the reference GPU path
 *    rejects (dfMatrixDataBase.cu:22-27) though its own 1D-flame case uses one (test/Tu500K-Phi1/0/p);
 *  - every call returns 0 on success, non-zero on error, and never exits the process
 *    (the reference exit()s, dfMatrixDataBase.H:40-50); dfmi_last_error() gives the message.
 */
#ifndef DFMI_H
#define DFMI_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dfmi_ctx dfmi_ctx;

enum { DFMI_SOA = 0, DFMI_AOS = 1 };

/* ---- lifetime ------------------------------------------------------------------------- */
/* dfMatrixDataBase(), prepareCudaResources (dfMatrixDataBase.cu:88,103): binds `device`, one stream */
int dfmi_create(dfmi_ctx** ctx, int device);
/* ~dfMatrixDataBase + cleanCudaResources (dfMatrixDataBase.cu:90,107); frees all device memory */
int dfmi_destroy(dfmi_ctx* ctx);
/* copy of the last error message of this thread; returns its length */
int dfmi_last_error(char* buf, int len);
/* library version string */
const char* dfmi_version(void);

/* ---- dfMatrixDataBase setup (createGPUBase, createGPUSolver.H:103-351) ------------------- */
/* dfMatrixDataBase::setConstantValues (dfMatrixDataBase.cu:114-147); rdelta_t = 1/deltaT */
int dfmi_set_constant_values(dfmi_ctx* ctx, int num_cells, int num_total_cells, int num_surfaces,
                             int num_boundary_surfaces, int num_patches, int num_proc_surfaces,
                             const int* patch_size, int num_species, double rdelta_t);
/* dfMatrixDataBase::setCyclicInfo (dfMatrixDataBase.cu:179-182): partner patch index or -1 */
int dfmi_set_cyclic_info(dfmi_ctx* ctx, const int* cyclic_neighbor);
/* dfMatrixDataBase::setCommInfo + ncclInit (dfMatrixDataBase.cu:92-101, dfNcclBase.cu:23-65):
 * nccl_unique_id is the 128-byte RCCL id (rank 0 creates it, the caller broadcasts it),
 * neighb_proc_no[num_patches] the peer rank of each processor patch (-1 otherwise). Collective: every rank calls
 * it; it also splits a second communicator (ncclCommSplit) for the time step's side stream. */
int dfmi_set_comm_info(dfmi_ctx* ctx, const void* nccl_unique_id, int nranks, int rank,
                       const int* neighb_proc_no);
/* rank-0 helper: create a fresh RCCL unique id (128 bytes) */
int dfmi_get_unique_id(void* nccl_unique_id_out);
/* Same as dfmi_set_comm_info, with an in-process transport instead of RCCL: the contexts of one
 * process registered under the same hub_id exchange halos by device copies, each driven by its own
 * host thread. Lets several ranks share one GPU (RCCL refuses two ranks on one device); no
 * reference counterpart. */
int dfmi_set_comm_local(dfmi_ctx* ctx, int hub_id, int nranks, int rank, const int* neighb_proc_no);
/* dfMatrixDataBase::setConstantIndexes (dfMatrixDataBase.cu:184-277) */
int dfmi_set_constant_indexes(dfmi_ctx* ctx, const int* owner, const int* neighbour, const int* proc_rows,
                              const int* proc_cols, int global_offset);
/* dfMatrixDataBase::initConstantFieldsInternal (dfMatrixDataBase.cu:316-333); sf/mesh_distance AoS */
int dfmi_init_constant_fields_internal(dfmi_ctx* ctx, const double* sf, const double* mag_sf,
                                       const double* weight, const double* delta_coeffs,
                                       const double* volume, const double* mesh_distance);
/* dfMatrixDataBase::initConstantFieldsBoundary (dfMatrixDataBase.cu:335-351); boundary_sf AoS */
int dfmi_init_constant_fields_boundary(dfmi_ctx* ctx, const double* boundary_sf, const double* boundary_mag_sf,
                                       const double* boundary_delta_coeffs, const double* boundary_weight,
                                       const int* boundary_face_cell, const int* patch_type_calculated,
                                       const int* patch_type_extrapolated);

/* patch delta vectors [B][3] (AoS, processor patches both halves like the other boundary arrays):
 * fvPatch::delta, on coupled patches (Cf - C) - (Cf' - C') (cyclicFvPatch::delta / processorFvPatch::delta).
 * The d a limited scheme's limiter reads across a coupled face (OpenFOAM-7 LimitedScheme::calcLimiter,
 * patch().delta()); required before a time step when a limited scheme is selected and the mesh has
 * coupled patches. No reference counterpart (its limitedLinear is disabled, dfMatrixOpBase.cu:2540-2600). */
int dfmi_init_boundary_delta(dfmi_ctx* ctx, const double* boundary_delta);

/* ---- convection / interpolation schemes -------------------------------------------------------------
 * The reference GPU path hard-wires upwind for Yi and ha and linear for K and hDiffCorrFlux
 * (dfYEqn.cu:543,587-593; dfEEqn.cu:166-174) whatever system/fvSchemes says; the CPU dfLowMachFoam runs
 * the case's schemes (YEqn.H:6-14 multivariate convection over every Y_i and he, createFields.H:118-129;
 * EEqn.H). term (the fvSchemes divSchemes key) / scheme:
 *   "div(phi,Yi_h)"       "upwind" (default) | "limitedLinear <k>" | "limitedLinear01 <k>"  (Yi and he)
 *   "div(phi,K)"          "linear" (default) | "upwind" | "limitedLinear <k>" | "limitedLinear01 <k>"
 *   "div(hDiffCorrFlux)"  "linear" (default) | "cubic"
 *   "div(phi,U)"          "linear" (default) | "limitedLinearV <k>"  (the 1D flame, test/Tu500K-Phi1/system/fvSchemes)
 * a leading "Gauss" is accepted, e.g. the reference cases' "Gauss limitedLinear01 1" / "Gauss cubic"
 * (test/dfLowMachFoam/twoD_reactingTGV/H2/cvodeSolver/system/fvSchemes:32-40). Call it after
 * dfmi_init_constant_fields_boundary (the patch kinds must be known). On decomposed meshes (processor
 * patches) every term's schemes are supported except div(phi,U) limitedLinearV, which is an error (here
 * and again when the UEqn is assembled). Limited schemes need the mesh_distance argument of
 * dfmi_init_constant_fields_internal (a NULL there makes them an error at the first assembly) and, on
 * meshes with coupled patches, dfmi_init_boundary_delta.
 *
 * Laplacian scheme (system/fvSchemes laplacianSchemes { default ...; }): one more term,
 *   "laplacian"           "orthogonal" (default) | "uncorrected" | "corrected"
 * a leading "Gauss linear" is accepted ("Gauss linear corrected"); "limited <psi>" and every other snGrad scheme are
 * refused by name. It serves the four laplacians: laplacian(mu | muEff, U), laplacian(rhoD_i (+ mut / Sct), Yi) with
 * diffAlphaD's laplacian(alpha hai_i, Yi), laplacian(alpha | alphaEff, he) and laplacian(rhorAUf, p).
 *   orthogonal   the caller's delta_coeffs (1 / |d|) and nothing else: the reference's box cases
 *   uncorrected  OpenFOAM-7's nonOrthDeltaCoeffs = 1 / max(n.d, 0.05 |d|) (n = Sf / |Sf|, d = mesh_distance; on cyclic,
 *                processor and processorCyclic slots d = the patch delta of dfmi_init_boundary_delta) wherever the
 *                assemblies read delta_coeffs; non-coupled patches keep boundary_delta_coeffs
 *   corrected    the same implicit part, and the explicit term of correctedSnGrad: per equation
 *                source += sum over the cell's faces of gamma_f |Sf| (k . (grad phi)_f), outward, with
 *                k = n - d nonOrthDeltaCoeffs (0 on non-coupled patches) and (grad phi)_f the linear interpolate of the
 *                cell-centred Gauss linear gradient (U: source, source_solve and so HbyA; Yi: the LDU source and the
 *                solver rows' rhs; diffAlphaD takes its own term; p: see the option p.n_nonorth below)
 * The library forms both arrays on the device when a scheme other than orthogonal is first selected; dfmi_get_field
 * returns them in OpenFOAM face order as "nonorth_delta_coeffs" [F], "nonorth_corr" [F] x 3,
 * "boundary_nonorth_delta_coeffs" [B] and "boundary_nonorth_corr" [B] x 3 (they cannot be set). Errors, each leaving
 * the scheme in force: no mesh_distance was given; the mesh has coupled patches and dfmi_init_boundary_delta was not
 * called; an unknown or limited scheme.
 * Option p.n_nonorth (integer >= 0, default 0) is PIMPLE's nNonOrthogonalCorrectors: every pEqn assembles once and runs
 * 1 + p.n_nonorth passes of { grad p from p / boundary_p as they stand; source = base + the divergence of the face flux
 * correction; solve } (pEqn.H:51-62); phi = phiHbyA + pEqn.flux() includes the last pass's face flux correction on
 * internal faces and coupled slots. With "corrected" the loop runs once even at p.n_nonorth = 0, with the correction
 * from the incoming p; with the other two schemes and p.n_nonorth = 0 the pEqn is the one solve it always was.
 * dfmi_time_step keeps its signature. The CPU-A baseline returns an error for every laplacian scheme but orthogonal. */
int dfmi_set_scheme(dfmi_ctx* ctx, const char* term, const char* scheme);

/* ---- cell renumbering (the role of OpenFOAM's renumberMesh; run once on the host before
 * dfmi_set_constant_indexes, then permute the mesh and field data with the returned maps) -------- */
/* new_to_old[num_cells]: method "bricks" (structured blocks: cell_centres holds the integer (i, j, k) of
 * each cell; 8x8x4 bricks along a Z-order curve, lexicographic inside a brick -- the order the gathers
 * are tuned for), "morton" (Z-order of the cell centres [C][3], any mesh), "rcm" (reverse Cuthill-McKee
 * of the face graph, no geometry) or "none" */
int dfmi_renumber_cells(int num_cells, const double* cell_centres, int num_faces, const int* owner,
                        const int* neighbour, const char* method, int* new_to_old);
/* faces of the renumbered mesh in upper-triangular order: face_new_to_old[F], new owner/neighbour
 * (owner < neighbour), flipped[F] = 1 where owner and neighbour swapped (negate Sf and face fluxes,
 * w -> 1 - w, reverse the centre-to-centre vector); boundary faces keep their order (faceCells map
 * through the cell permutation) */
int dfmi_renumber_faces(int num_cells, int num_faces, const int* owner, const int* neighbour,
                        const int* cell_new_to_old, int* face_new_to_old, int* new_owner, int* new_neighbour,
                        int* flipped);

/* the order in which the per-cell gather kernels visit cells (order[C]: a permutation; thread t works on
 * cell order[t]) -- e.g. dfmi_renumber_cells(..., "bricks", ...) of a blockMesh box: the data stay in
 * their order, only the visiting order becomes cache-compact. NULL restores the natural order. Results
 * are bitwise independent of it (each cell's arithmetic is unchanged). No reference counterpart. */
int dfmi_set_traversal(dfmi_ctx* ctx, const int* order);

/* ---- per-equation patch types ------------------------------------------------------------ */
/* dfUEqn/dfYEqn/dfEEqn/dfpEqn/dfRhoEqn/dfThermo::setConstantFields (e.g. dfUEqn.cu:364-379,
 * dfEEqn.cu setConstantFields, dfThermo.cu setConstantFields). field in
 * {"U","p","he","K","Y","T","rho","nut","k","epsilon"} and the flareFGM scalars {"Z","Zvar","c","cvar","Zcvar","Ha"} (flareFGM
 * block below); patch_type[num_patches]. "nut" (LES / RAS, below) takes zeroGradient, fixedValue,
 * calculated, cyclic, processor, processorCyclic and empty; not set, it is "calculated" on every non-coupled patch
 * (OpenFOAM's default for nut: the stored boundary_nut is kept, zero unless set).
 * The k-epsilon wall functions and turbulent inlets (RAS block below) have codes of their own, each for one field, on plain
 * (not cyclic, processor or empty) patches only; any other field or patch kind is refused by name:
 *   13 epsilonWallFunction (epsilon), 14 nutkWallFunction (nut), 15 turbulentIntensityKineticEnergyInlet (k),
 *   16 turbulentMixingLengthDissipationRateInlet (epsilon).
 * Setting the patch types of k, epsilon or nut invalidates nut as writing k does. */
int dfmi_set_patch_types(dfmi_ctx* ctx, const char* field, const int* patch_type);
/* a patch parameter, positive and finite: (field "p", name "gamma") of waveTransmissive; ("nut", "Cmu" | "kappa" | "E") of
 * nutkWallFunction (defaults 0.09, 0.41, 9.8: the wall function's own coefficients, which the patch's epsilonWallFunction
 * reads too -- the copies in a case's 0/epsilon are ignored, as in OpenFOAM-7; setting one invalidates nut);
 * ("k", "intensity") of turbulentIntensityKineticEnergyInlet; ("epsilon", "mixingLength") of
 * turbulentMixingLengthDissipationRateInlet (both without a default: never set on a patch of that type is an error at the
 * first dfmi_turbulence_correct). Anything else is refused by name. */
int dfmi_set_patch_param(dfmi_ctx* ctx, const char* field, int patch, const char* name, double value);
/* dfYEqn inertIndex (YEqn.H:119-131) */
int dfmi_set_inert_index(dfmi_ctx* ctx, int inert_index);

/* ---- thermo (dfThermo::setConstantValue, dfThermo.cu:361-435) ---------------------------- */
/* coefficient table in memory: W[S], nasa[S][15], visc[S][5], cond[S][5], bdiff[S][S][5] */
int dfmi_thermo_set_coeffs(dfmi_ctx* ctx, int num_species, const double* W, const double* nasa,
                           const double* visc, const double* cond, const double* bdiff);
/* read the reference's binary thermo_<mech>.txt */
int dfmi_thermo_load(dfmi_ctx* ctx, const char* thermo_coeff_file);
/* Equation of state. model 0: ideal gas (clears; the arrays are not read), 1: Peng-Robinson with the species'
 * a [Pa m^6 / kmol^2], b [m^3 / kmol] and acentric factor (Cantera's units), geometric-mean cross terms, no binary overrides.
 * Call it after dfmi_thermo_set_coeffs with the same num_species. Refused by name: a model other than 0 or 1, a species
 * count that differs, a value that is not finite, a < 0, b <= 0, and model 1 with more than 16 species.
 * With model 1 dfmi_thermo_correct / dfmi_thermo_update_energy take rho from the cubic (the root of lowest fugacity), T from
 * he by Newton steps carried to rounding, psi = (rho(he, p) - rho(he, p (1 - 1e-4))) / (1e-4 p) at constant enthalpy
 * (CanteraMixture.H:116-149), alpha = lambda / cp with the real cp and rhoD_i with the real rho; mu, lambda and hai_i keep
 * the ideal forms. They also write the field rho_thermo (OpenFOAM's thermo.rho_, no longer psi p), and dfmi_time_step follows
 * the CPU solver's corrector (pEqn.H:1-4, 8, 95; dfLowMachFoam.C:517): rho = rho_thermo, psip0 = psi p, the p equation,
 * rho_thermo += psi p - psip0, the rhoEqn; after the loop rho = rho_thermo. dfmi_thermo_update_rho copies rho_thermo to rho,
 * dfmi_thermo_psip0 is unchanged and dfmi_thermo_correct_psip_rho acts on rho_thermo. With model 0 every launch is the
 * ideal-gas one. Refused by name with model 1: option fv.species_generic (at the thermo call); at dfmi_time_step chemistry
 * mode != 0 and les.model / ras.model / tci.model != 0; dfmi_zero_d_step. */
int dfmi_thermo_set_eos(dfmi_ctx* ctx, int model, int num_species, const double* a, const double* b, const double* acentric);

/* ---- fields (initNonConstantFields*, getFieldPointer dfMatrixDataBase.cu:521-539) ---------- */
/* names: cells  rho rho_old p p_old he T K K_old psi mu alpha dpdt rAU diffAlphaD psip0
 *        vector U U_old HbyA hDiffCorrFlux sumYDiffError     species Y rhoD hai RR
 *        faces  phi phi_old phiUc rhorAUf phiHbyA
 *        boundary_<name> for the boundary counterparts; boundary-only: boundary_heGradient,
 *        boundary_{U,p,Y,K}_ref (inletOutlet inletValue), boundary_p_vf (waveTransmissive valueFraction),
 *        boundary_p_gamma, chem_stats [3][C]. count = values per component.
 *        LES: delta (cells; positive), nut (cells; get only), boundary_nut (set: the fixedValue / calculated slots);
 *        les.model = 5, get only: les_Cs les_LM les_MM (cells).
 *        RAS: k epsilon (cells), boundary_{k,epsilon}, boundary_{k,epsilon}_ref; get only: G divU k_prebound epsilon_prebound,
 *        boundary_yPlus (the nutkWallFunction slots' yPlus, zero elsewhere).
 *        Combustion closure: tci_tc (cells); get only: tci_kappa tci_tmix tci_tauStar Qdot_eff (cells), RR_eff (species).
 *        Equation of state: rho_thermo, boundary_rho_thermo (thermo.rho_; allocated at the first dfmi_thermo_set_eos or use).
 *        flareFGM: the fields of the flareFGM block below.
 *        Spray coupling: parcel_rhoTrans (species), parcel_UTrans (vector), parcel_UCoeff parcel_hsTrans parcel_hsCoeffByCp
 *        (cells); no boundary counterparts (the spray block below). */
int dfmi_set_field(dfmi_ctx* ctx, const char* name, const double* host, long count, int layout);
int dfmi_get_field(dfmi_ctx* ctx, const char* name, double* host, long count, int layout);

/* ---- one outer iteration (dfLowMachFoam.C:284-531, pEqn_GPU.H) --------------------------- */
int dfmi_pre_time_step(dfmi_ctx* ctx);          /* dfMatrixDataBase::preTimeStep (:503-517) */
int dfmi_rho_process(dfmi_ctx* ctx);            /* dfRhoEqn::process (dfRhoEqn.cu:41-92) */
int dfmi_U_process(dfmi_ctx* ctx);              /* dfUEqn::process (dfUEqn.cu:487-689) */
int dfmi_Y_process(dfmi_ctx* ctx);              /* dfYEqn::process (dfYEqn.cu:443-695); RR from dfmi_set_field("RR") or the chemistry */
int dfmi_E_process(dfmi_ctx* ctx);              /* dfEEqn::process (dfEEqn.cu:108-264) */
/* ---- LES eddy viscosity: turbulence->correct() (dfLowMachFoam.C:508). Every equation of the reference goes through
 * turbulence-> (UEqn.H:6 divDevRhoReff(U); YEqn.H:96 DEff = rhoD(i) + mut/Sct; EEqn.H:20-37 laplacian(alphaEff, he));
 * its GPU path carries a Smagorinsky kernel it never calls (src_gpu/dfUEqn.cu:305-353). Options (dfmi_set_option):
 *   les.model  0 laminar (default) | 1 Smagorinsky | 2 WALE (OpenFOAM-7 LESeddyViscosity) | 4 Sigma | 5 dynamicSmagorinsky
 *              (the reference's own src/TurbulenceModels/turbulenceModels/Sigma/Sigma.C and
 *              dynamicSmagorinsky/dynamicSmagorinsky.C). 3 is reserved and refused; anything else is refused
 *   les.Ck 0.094, les.Ce 1.048 (Smagorinsky), les.Cw 0.325 (WALE), les.Csg 1.5 (Sigma, Sigma.C:118-126), les.Prt 1,
 *   les.Sct 1 (createFields.H:133)
 * With g = grad(U) (the UEqn's Gauss linear gradient), D = symm(g) and the field "delta":
 *   Smagorinsky  a = Ce/delta, b = (2/3) tr D, c = 2 Ck delta (dev(D) && D), k = ((-b + sqrt(b^2 + 4ac)) / (2a))^2
 *   WALE         Sd = dev(symm(g.g)), m = Sd && Sd, s = D && D, k = (Cw^2 delta/Ck)^2 m^3 / ((s^(5/2) + m^(5/4))^2 + 1e-15)
 *   nut = Ck delta sqrt(k); boundary_nut = nut.correctBoundaryConditions() by the patch types of "nut".
 *   Sigma (Sigma.C:40-89), with the singular values s1 >= s2 >= s3 >= 0 of g:
 *                Dsg = s3 (s1 - s2)(s2 - s3) / (s1^2 + 1e-300), nut = (Csg delta)^2 Dsg
 *     s2 is the true middle singular value. The reference's loop (Sigma.C:64-66) keeps the last value OpenFOAM's unsorted
 *     SVD returns, whichever it is, so its Dsg is zero whenever that is the largest or the smallest: a deliberate deviation
 *     (DESIGN.md 9). The singular values are the column norms of g after 5 cyclic sweeps of one-sided (Hestenes) Jacobi
 *     rotations on the columns of g over the pairs (0,1), (0,2), (1,2): a = p.p, b = q.q, c = p.q; c == 0 is the identity;
 *     else z = (b - a) / (2c), t = sign(z) / (|z| + sqrt(1 + z^2)), cs = 1 / sqrt(1 + t^2), sn = cs t, p' = cs p - sn q,
 *     q' = sn p + cs q. g^T g is never formed. g = 0, a rank-1 g and a g with orthogonal columns give nut = 0 exactly.
 *   dynamicSmagorinsky (dynamicSmagorinsky.C:38-49, 141-199; `filter simple` only). OpenFOAM-7's simpleFilter, fvc::average
 *   and surfaceSum are restated here, and this statement is the definition:
 *     The filter  F(x)_c = sum_f |Sf| x_f / sum_f |Sf| over every face of cell c that carries an internal face or a
 *       boundary slot (`empty` faces carry neither), the cell's internal faces in the sequential order, then its slots.
 *       x_f = w x_P + (1 - w) x_N on internal and coupled faces (cyclic: the partner cell; processor: the neighbour cell's
 *       value from the halo). On a non-coupled slot x_f is the field's boundary value: boundary_U for U; for a product the
 *       product of the boundary values; for S the value formed from the boundary gradient the UEqn forms,
 *       g_b = g_c + n (snGrad - n . g_c) with snGrad = deltaCoeffs (boundary_U - U_c) on fixedValue and mixed slots, 0
 *       elsewhere; for LL && MM and MM && MM the cell's own value (surfaceSum returns an extrapolated field).
 *       fvc::average of a cell field is the same operator. The boundary value of delta is never read (MM multiplies by
 *       the cell's delta after the filter).
 *     S = dev(symm(g)), |S| = sqrt(S && S);  LL = dev(F(U U) - F(U) F(U));  MM = delta^2 (F(|S| S) - 4 |F(S)| F(S))
 *     les_LM = F(LL && MM);  les_MM = max(F(MM && MM), 1e-300);  les_Cs = 0.5 les_LM / les_MM
 *     nut = max(les_Cs delta^2 |S|, -mu / rho), mu and rho as the context holds them at the call
 *     les_Cs and nut take both signs ("to allow for backscatter"). les_Cs, les_LM, les_MM are get-only cell fields that
 *     exist from the first use of les.model = 5. Three kernels (S on cells and non-coupled slots; the four filtered
 *     quantities and the two contractions; their average, Cs and nut); several ranks: S, then the two contractions, then
 *     nut cross the processor patches.
 *     Everything downstream of nut (the validity rule, boundary_nut, the halo, the three assemblies, the refusals together
 *     with ras.model, tci.model, fgm.model, an equation of state and spray) is as for models 1 and 2.
 * This call forms nut and boundary_nut from U / boundary_U as they stand (several ranks: a collective, the processor
 * slots' neighbour half is exchanged). dfmi_time_step runs it after the last pressure corrector, and first thing when
 * nut is not valid (turbulence->validate(), dfLowMachFoam.C:207): after les.model or a coefficient changed, "delta"
 * was set, or "U" / "boundary_U" were written through dfmi_set_field. With les.model != 0 the three assemblies read
 *   mut = rho nut, muEff = mut + mu, alphaEff = alpha + mut/Prt, DEff_i = rhoD_i + mut/Sct
 * (rho after the rhoEqn; on boundary slots from the slot's own values) and drop what the reference drops for
 * simulationType != laminar: fvmDiv(phiUc, Yi) (YEqn.H:101-106), diffAlphaD and div(hDiffCorrFlux) (EEqn.H:30-36) --
 * the YEqn preparation kernel is not launched and sumYDiffError, hDiffCorrFlux, diffAlphaD, phiUc read back as zeros.
 * dfmi_U_process / dfmi_Y_process / dfmi_E_process / dfmi_assemble use the nut in the context and fail when it is not
 * valid. les.model = 0: a successful no-op.
 *
 * ---- RAS k-epsilon (ras.model = 1): the same call is kEpsilon::correct(). The statement below is the definition: it
 * restates OpenFOAM-7 kEpsilon::correct() / correctNut() and bound() for the compressible solver (alpha = 1, no
 * fvOptions; the wall functions and turbulent inlets follow at the end of this block). Options (dfmi_set_option; all positive and finite, C3 any finite value):
 *   ras.model  0 none (default) | 1 kEpsilon          (ras.model != 0 together with les.model != 0 is refused)
 *   ras.Cmu 0.09, ras.C1 1.44, ras.C2 1.92, ras.C3 0, ras.sigmak 1.0, ras.sigmaEps 1.3,
 *   ras.kMin 1e-15, ras.epsilonMin 1e-15, ras.Prt 1, ras.Sct 1     (Prt / Sct replace les.Prt / les.Sct in RAS mode)
 * g = grad(U) is the UEqn's Gauss linear gradient (the same faces in the same order), nut the old value, mu the thermo's:
 *   divU  = (1/V) [ sum_f +-phi_f / interp_f(w, rho_P, rho_N)  +  sum_slots boundary_phi / boundary_rho ]
 *           (a coupled slot's boundary_rho is the face interpolate w rho_c + (1 - w) rho_neighbour)
 *   G     = nut (dev(twoSymm(g)) && g)                 T = g + g^T, t3 = (1/3) tr T,
 *           ((T00-t3) g00 + (T11-t3) g11 + (T22-t3) g22) + ((T01 g01 + T01 g10) + (T02 g02 + T02 g20) + (T12 g12 + T12 g21))
 *   Dk    = rho (nut/sigmak + mu/rho)        Deps = rho (nut/sigmaEps + mu/rho)     (cells and slots alike)
 *   epsEqn:  ddt(rho,eps) + div(phi,eps) - laplacian(Deps,eps)
 *              == C1 rho G eps/k  - SuSp((2/3 C1 - C3) rho divU, eps)  - Sp(C2 rho eps/k, eps)
 *            solve;  bound(eps, epsilonMin)
 *   kEqn:    ddt(rho,k) + div(phi,k) - laplacian(Dk,k)
 *              == rho G  - SuSp(2/3 rho divU, k)  - Sp(rho eps/k, k)          (eps: the new one; k in eps/k: the old one)
 *            solve;  bound(k, kMin)
 *   nut = Cmu k^2 / eps;   boundary_nut by nut's patch types (calculated slots: Cmu boundary_k^2 / boundary_epsilon);   halo
 * ddt is Euler with rho_old and the field's own start-of-call value (k_old / epsilon_old are not part of
 * dfmi_pre_time_step). SuSp(a, psi) is diag += V max(a,0), source -= V min(a,0) psi; Sp(b, psi) is diag += V b. Per cell
 *   diag = ((rdt rho V + d1) - dL) + V Sp,  source = rdt rho_old psi V + V Su      (d1 convection, dL laplacian, as the EEqn)
 * div(phi,k) / div(phi,epsilon): dfmi_set_scheme, upwind (default) | limitedLinear <k> | linear. The laplacians go through
 * the laplacian scheme in force; under "corrected" the explicit term is added from the field's Gauss gradient. Boundary
 * coefficients as the EEqn's for zeroGradient, fixedValue, inletOutlet (boundary_{k,epsilon}_ref), cyclic, processor,
 * processorCyclic, calculated and empty. bound(psi, m) applies to every cell of the solved field psi (its slots corrected):
 *   psi = max(max(psi, avg(max(psi,m)) * pos0(-psi)), m),  avg = sum_f |Sf| interp_f / sum_f |Sf| over the cell's faces and
 *   slots (a coupled slot -- cyclic, processor -- is a face: the interpolate of the two bounded cell values, so the result
 *   does not depend on a decomposition; every other slot max(boundary_psi, m)); then every slot: boundary_psi = max(boundary_psi, m).
 * Applied unconditionally it equals OpenFOAM's gated form (the gate is the global minimum): a field >= m is unchanged bitwise.
 * Which rho: the one dfLowMachFoam.C:508 sees -- after the last pEqn.H (its correctPsipRho and rhoEqn: rho += psi p - psip0,
 * then the rhoEqn from rho_old and the final phi), before rho = thermo.rho() (:517); rho_old and phi are the step's.
 * dfmi_time_step in RAS mode runs that corrector tail (laminar / LES skip it: nothing reads it) and this call before the
 * final rho = psi p. Fields: k, epsilon, boundary_k, boundary_epsilon (set / get; all four must have been set: an error
 * names the missing one), G, divU, k_prebound, epsilon_prebound (get only: production, dilatation, and the solved fields
 * before bound()); patch types "k" and "epsilon". nut belongs to k and epsilon: writing either, a boundary counterpart,
 * ras.model or a coefficient invalidates it; dfmi_time_step and the per-equation entries then run correctNut() only
 * (turbulence->validate()), never the equations. Solver names "epsilon" and "k" (dfmi_set_solver / _stats / _work);
 * dfmi_assemble / dfmi_get_matrix take "epsilon" and "k": each is formed from the fields as they stand, no solve between.
 *
 * ---- wall functions and turbulent inlets (patch-type codes 13-16, dfmi_set_patch_types; parameters, dfmi_set_patch_param).
 * The statement below is the definition; it restates OpenFOAM-7's epsilonWallFunction, nutkWallFunction,
 * turbulentIntensityKineticEnergyInlet and turbulentMixingLengthDissipationRateInlet in the compressible solver
 * (kqRWallFunction is zeroGradient; alphatWallFunction needs nothing: alphaEff = alpha + rho nut / Prt with the wall
 * function's boundary_nut already is it). A context without these patch types launches none of their kernels and
 * allocates nothing for them. One cost reaches every RAS context: dfmi_set_patch_types of k, epsilon or nut invalidates
 * nut whatever the codes, so the next validation runs correctNut() (the two k_ras_nut launches) once more, with the same
 * result; in LES and laminar contexts that flag is not read.
 * Per wall patch, on the host, from its ("nut", ...) parameters:
 *   Cmu25 = sqrt(sqrt(Cmu));   Cmu75 = Cmu25 * sqrt(Cmu);   yPlusLam: ypl = 11, then ten times ypl = log(max(E * ypl, 1)) / kappa
 * Per wall slot b of cell c:
 *   y = 1 / deltaCoeffs_b  (the patch's own deltaCoeffs under every laplacian scheme);   nuw = boundary_mu_b / boundary_rho_b
 *   yPlus = ((Cmu25 * y) * sqrt(k_c)) / nuw
 * nutkWallFunction, wherever boundary_nut is formed (correctNut() at the end of this call and on the validation path), from
 * the current k:
 *   boundary_nut_b = yPlus > yPlusLam ? nuw * ((yPlus * kappa) / log(E * yPlus) - 1) : 0;   boundary_yPlus_b = yPlus
 * epsilonWallFunction, after G and divU are formed and before the epsilon equation, from the old k and the boundary_nut as
 * stored. A patch that is epsilonWallFunction for epsilon must be nutkWallFunction for nut: otherwise this call and the
 * validation path fail, naming the patch. For every cell c with n >= 1 slots of this type (over all such patches):
 * w = 1 / n, G[c] and epsilon[c] are reset to 0, then its slots are accumulated in ascending slot order,
 *   yPlus > yPlusLam:  epsilon[c] += ((w * Cmu75) * (k_c * sqrt(k_c))) / (kappa * y)
 *                      G[c] += ((((w * (boundary_nut_b + nuw)) * magGradUw) * Cmu25) * sqrt(k_c)) / (kappa * y)
 *   otherwise:         epsilon[c] += (((w * 2) * k_c) * nuw) / (y * y)
 *   magGradUw = deltaCoeffs_b * sqrt((dx * dx + dy * dy) + dz * dz),  d = boundary_U_b - U_c
 * and boundary_epsilon_b = epsilon[c] on those slots, which are fixed values from there on (the post-solve correction
 * leaves them; bound()'s slot pass applies). The kEqn sees the modified G.
 * The constraint (fvMatrix::setValues): the epsilon matrix is constrained on those cells after assembly, v_c = epsilon[c].
 *   A constrained cell: source = v_c * diag; its off-diagonals and the internalCoeffs / boundaryCoeffs of all its slots are 0.
 *   An unconstrained cell: source -= A[c][n] * v_n and A[c][n] = 0, once per constrained neighbour n across an internal
 *   face, in the sequential face order (neighbour faces ascending, then owned faces), after the source is otherwise
 *   complete (under the corrected laplacian the explicit non-orthogonal term is added after it).
 *   Nothing is moved across a coupled slot: the cell across keeps its coupling and reads v through the halo or the cyclic column.
 * After the solve a constrained cell holds v_c to within 4 * 2^-52 relative (the even-odd recovery forms (v d) / d).
 * Turbulent inlets: both are inletOutlet (valueFraction = 1 - pos0(phi), refGrad 0) with an inletValue re-formed at each call,
 *   k:        boundary_k_ref_b = (1.5 * (I * I)) * ((Ux * Ux + Uy * Uy) + Uz * Uz)  of boundary_U, first thing in the call
 *   epsilon:  boundary_epsilon_ref_b = (Cmu75 / L) * (kb * sqrt(kb)),  kb = boundary_k_b as it stands before the epsilon
 *             equation, Cmu75 formed as above from ras.Cmu
 * and coefficients, post-solve correction and bound() bitwise those of inletOutlet with those inletValues set by hand.
 * Order of the call: k's inletValue; G and divU; the wall update and epsilon's inletValue; the epsilon equation assembled
 * and constrained, solved, bound; the k equation, solved, bound; correctNut() with the wall slots. Several ranks: the wall
 * update is rank-local; where a patch is epsilonWallFunction the new epsilon goes through the field halo once more before
 * the assembly (a collective: every rank carries every physical patch, of size zero where it has none of its faces, as
 * decomposePar leaves them, and sets the same types on it).
 * dfmi_assemble("epsilon" | "k") in such a context runs the complete wall update first, the overwrite of epsilon in the
 * wall cells included: the state the equations see inside this call. "epsilon" returns the constrained matrix. */
int dfmi_turbulence_correct(dfmi_ctx* ctx);
int dfmi_thermo_correct(dfmi_ctx* ctx);         /* dfThermo::correctThermo (dfThermo.cu:572-671) */
int dfmi_thermo_update_energy(dfmi_ctx* ctx);   /* he, psi, rho, transport from T (dfThermo::updateEnergy) */
int dfmi_thermo_update_rho(dfmi_ctx* ctx);      /* dfThermo::updateRho (:673-679) */
int dfmi_thermo_psip0(dfmi_ctx* ctx);           /* dfThermo::psip0 (:681-686) */
int dfmi_thermo_correct_psip_rho(dfmi_ctx* ctx);/* dfThermo::correctPsipRho (:688-695) */
int dfmi_U_get_HbyA(dfmi_ctx* ctx);             /* dfUEqn::getHbyA (dfUEqn.cu:824-834) */
int dfmi_p_process(dfmi_ctx* ctx);              /* dfpEqn::process (dfpEqn.cu:379-546) */
int dfmi_post_time_step(dfmi_ctx* ctx);         /* dfMatrixDataBase::postTimeStep (:519) */
/* the whole loop body above with n_corr pressure correctors */
int dfmi_time_step(dfmi_ctx* ctx, int n_corr);   /* non-zero also when chemistry hit its step limit */
int dfmi_sync(dfmi_ctx* ctx);

/* ---- spray coupling: the Lagrangian source terms parcels.Srho(rho) (rhoEqn.H:38), parcels.SU(U) (UEqn.H:9),
 * parcels.SYi(i, Yi) (YEqn.H:110-111), parcels.Sh(he) and hcSource (EEqn.H:3-8, 27-28, 34-35). The cloud itself -- tracking,
 * injection, break-up, evaporation, parcels.evolve() -- stays with the caller; this library takes the cloud's per-cell
 * accumulators (already volume-integrated) and adds their terms to the four equations. No new entry point. Options:
 *   spray.model  0 (default) | 1: the cloud's active && coupled
 *   spray.rho, spray.U, spray.Yi, spray.h  0 explicit (default) | 1 semiImplicit   (sourceTerms.schemes of sprayCloudProperties)
 * Fields (dfmi_set_field / dfmi_get_field, cells only, allocated zeroed at first use; values must be finite):
 *   parcel_rhoTrans    [S][C]  kg      ReactingCloud::rhoTrans(i), every species, the inert one included
 *   parcel_UTrans      [3][C]  kg m/s  KinematicCloud::UTrans()
 *   parcel_UCoeff      [C]     kg      UCoeff(), not negative; read only with spray.U = 1
 *   parcel_hsTrans     [C]     J       ThermoCloud::hsTrans()
 *   parcel_hsCoeffByCp [C]     kg      hsCoeff() / thermo.Cp(), the quotient formed by the caller; read only with spray.h = 1
 * They stay as set until written again: the caller sets them after parcels.evolve() (dfLowMachFoam.C:269-279) and before the
 * step. With spray.model = 1 the terms below enter dfmi_rho_process, dfmi_U_process, dfmi_Y_process, dfmi_E_process,
 * dfmi_assemble ("rho", "U", "Y", "Y_ell", "Y_ell_ref", "E"), what dfmi_get_matrix / dfmi_get_solver_rows then return, and
 * dfmi_time_step -- every rhoEqn it runs, those of the pressure correctors included (pEqn.H:103 includes rhoEqn.H). The p
 * equation gets no term (pEqn.H has none); dfmi_zero_d_step ignores the model.
 * The statement below is the definition (KinematicCloudI.H:432-437, ThermoCloudI.H:236-245, ReactingCloudI.H:110-131 and
 * 211-236, with A == T as A - T, fvm::Sp / fvm::SuSp as in the RAS block above, and a volume field added to a matrix as
 * source -= V field). V the cell volume, rdt = 1 / deltaT as the ddt terms read it, rho / U / Yi / he the cell values as they
 * stand when the equation is assembled (before its solve), hc_i = Hf298_i / W_i, the Qdot weights (CanteraMixture.H:325).
 * Every operation is one fp64 rounding, evaluated left to right as written, no fused multiply-add; sums over species run
 * i = 0 .. S-1 from 0.0:
 *   rhoEqn    t = (sum_i rhoTrans_i) rdt
 *     explicit      source = source + t
 *     semiImplicit  a = (t / V) / rho;   diag = diag - V max(a, 0);   source = source + (V min(a, 0)) rho
 *     then rho = source / diag (the diagonal solve); dfmi_assemble("rho") leaves this diag / source in dbg_rho_diag / _source
 *   UEqn      per component k, into source and into source_solve (= source - grad p), hence into H and HbyA:
 *     explicit      t_k = UTrans_k rdt
 *     semiImplicit  diag = diag + UCoeff rdt;   t_k = (UTrans_k + UCoeff U_k) rdt
 *                   rAU = 1 / ((diag + sum_slots (ic_0 + ic_1 + ic_2) / 3) / V) is formed again from this diag, so rAU,
 *                   boundary_rAU and the p equation's rhorAUf carry it
 *     source_k = source_k + t_k;   source_solve_k = source_solve_k + t_k
 *   YEqn      every species i != inert (the inert species has no equation; its rhoTrans still counts in rho and hc):
 *     explicit      source_i = source_i + rhoTrans_i rdt
 *     semiImplicit  s = (rhoTrans_i rdt) / V;   s < 0:  diag_i = diag_i + (V (-s)) / (Y_i + 1e-15)      (OpenFOAM's small)
 *                                               s >= 0: source_i = source_i + s V
 *     the same in the hard-coded, species-chunked and LES / RAS forms of the assembly. In the solver rows the production
 *     assembly writes ("Y_ell": dS = diag + sum internalCoeffs, rhs = source + boundaryCoeffs) the term is added to dS / rhs
 *     after those sums; "Y_ell_ref" keeps that order, so the two stay equal bit for bit
 *   EEqn      sens = hsTrans rdt
 *     explicit      source = source + sens
 *     semiImplicit  a = (hsCoeffByCp rdt) / V;   a >= 0: aV = a V;  diag = diag + aV;  source = source + (sens + aV he)
 *                                                a <  0: source = source + sens   (the SuSp and the explicit echo cancel)
 *     then, under either scheme, hcSource:  h = sum_i rhoTrans_i hc_i;   source = source + h rdt
 * Each term is the last thing added to its equation's diag / source: under the "corrected" laplacian it comes after the
 * explicit non-orthogonal term. So "the matrix with spray.model = 1 is the matrix with spray.model = 0, then the term" is exact.
 * The U and E solver rows are folded from these LDU parts (dS = (diag + term) + sum internalCoeffs).
 * Works with les.model, ras.model, tci.model, every chemistry mode, scheme and traversal order, and on decomposed meshes
 * (the terms are rank-local: no halo). Refused by name: spray.model = 1 with fgm.model = 1 or with an equation of state set;
 * a required field never set (parcel_UCoeff / parcel_hsCoeffByCp only under their semiImplicit scheme); a scheme value other
 * than 0 / 1; non-finite values, a negative parcel_UCoeff, a wrong count. With spray.model = 0 nothing is launched and, in a
 * context that never touches these options or fields, nothing allocated. */

/* ---- adjustable time step: the first two lines of the time loop, dfLowMachFoam.C:261-262
 * (#include "compressibleCourantNo.H", #include "setDeltaT.H"). The reference GPU path has no counterpart: its
 * step is fixed at setup (createGPUSolver.H:152 "TODO: get deltaT from time API"). */
/* compressibleCourantNo.H (dfLowMachFoam.C:261) on the device, from phi, boundary_phi, rho and the cell volumes as
 * they stand, with the step size in force:
 *   sumPhi_c  = (sum over the faces f of cell c of |phi_f|) / rho_c        fvc::surfaceSum(mag(phi)) / rho
 *   CoNum     = 0.5 max_c(sumPhi_c / V_c) deltaT                           (gMax over ranks)
 *   meanCoNum = 0.5 (sum_c sumPhi_c / sum_c V_c) deltaT                    (gSum over ranks)
 * Every internal face counts for its owner and its neighbour, every boundary face of every patch kind for its
 * face cell (a processor face with this rank's flux only). Per-block partials reduced in a fixed order, no
 * floating-point atomics; with several ranks the per-rank (max, sum, volume) are all-gathered and combined in rank
 * order, so every rank returns the same bits (a collective: every rank calls it at the same point). Synchronises on
 * the result only. Right after a dfmi_time_step run with the option step.courant = 1 it returns the record that
 * step left in pinned memory, without a launch. */
int dfmi_courant_no(dfmi_ctx* ctx, double* co_num, double* mean_co_num);
/* setDeltaT.H (dfLowMachFoam.C:262): the step size of every later dfmi_pre_time_step / dfmi_time_step /
 * per-equation call -- ddt terms, ddtCorr, dpdt, the waveTransmissive valueFraction 1 / (1 + w deltaT deltaCoeffs)
 * and the chemistry's integration interval; the chemistry's remembered sub-step is capped by the new interval.
 * RR of the DF-ODENet surrogate is a rate formed with dt_infer and does not depend on deltaT, as in the reference
 * (dfChemistrySolver.cu:191). A changed step ends the cross-step reuse of the pressure AMG operators (option
 * amg.reuse_steps): the p operator scales with deltaT through rAU, and the next first corrector rebuilds the
 * hierarchy values as the reference does at every solve (AmgXSolver.cu:268-281). The step-size rule itself
 * (maxCo, maxDeltaT) stays with the caller, as in OpenFOAM. Errors: delta_t not positive or not finite; a call
 * before dfmi_set_constant_values. Setting the value in force changes and resets nothing. dfmi_zero_d_step keeps
 * its own dt argument. */
int dfmi_set_delta_t(dfmi_ctx* ctx, double delta_t);
/* the step size in force: the last dfmi_set_delta_t value, or 1 / rdelta_t of dfmi_set_constant_values */
int dfmi_get_delta_t(dfmi_ctx* ctx, double* delta_t);

/* per-step HIP events on the context stream (bench: median step time); no reference counterpart (its
 * TIME_GPU host ticks, dfLowMachFoam.C:249-531). dfmi_step_times returns got = steps timed since arming */
int dfmi_step_timer(dfmi_ctx* ctx, int on);
int dfmi_step_times(dfmi_ctx* ctx, double* ms, int n, int* got);
/* diagnostic: measured device-memory copy bandwidth (read + write GB/s) of a gib-GiB buffer copied reps
 * times by a 16-B-vector streaming kernel -- the measured peak beside the datasheet's 8 TB/s */
int dfmi_hbm_copy_peak(dfmi_ctx* ctx, double gib, int reps, double* gbs);
/* correct_boundary_conditions_{scalar,vector} (dfMatrixOpBase.cu:2402-2491) for field in
 * {"U","p","he","T","rho","K","Y","nut"} using that field's patch types */
int dfmi_correct_boundary(dfmi_ctx* ctx, const char* field);

/* ---- matrix inspection (the reference DEBUG_CHECK_LDU / compareResult path, dfYEqn.cu:566-572) */
/* eqn in {"rho","U","Y","E","p","HbyA","Y_ell","Y_ell_ref","epsilon","k","tci","Z","Zvar","c","cvar","Zcvar","Ha"}: run that equation's assembly only (no solve); under
 * the laplacian scheme "corrected" the sources include the explicit term ("p": that of the corrector loop's first pass).
 * "tci" (tci.model != 0): the closure's pointwise passes of dfmi_combustion_correct from the fields as they stand, RR and Qdot
 * included, without the chemistry solve -- tci_tmix, tci_tc, tci_kappa (PaSR) or tci_kappa, tci_tauStar (EDC), then RR_eff
 * and Qdot_eff */
int dfmi_assemble(dfmi_ctx* ctx, const char* eqn);
/* part in {"lower","upper","diag","source","source_solve","internal_coeffs","boundary_coeffs"} */
int dfmi_get_matrix(dfmi_ctx* ctx, const char* eqn, const char* part, double* host, long count);
/* the solver's rows of the YEqn batch after dfmi_assemble("Y_ell") (the production path: assembly
 * written straight into the rows) or dfmi_assemble("Y_ell_ref") (LDU assembly + the generic
 * fvMatrix::addBoundaryDiag/Source fold, the role of ldu_to_csr, dfMatrixOpBase.cu:2276-2336):
 * part "val" [S-1][W][C] (W = coupling entries per row), "dS" (diag + internalCoeffs) or "rhs"
 * [S-1][C]. eqn must be "Y". */
int dfmi_get_solver_rows(dfmi_ctx* ctx, const char* eqn, const char* part, double* host, long count);
/* solver controls (amgxUOptions / amgxpOptions): eqn in {"U","Y","E","p","epsilon","k"} and the flareFGM equations
 * {"Z","Zvar","c","cvar","Zcvar","Ha"} */
int dfmi_set_solver(dfmi_ctx* ctx, const char* eqn, int max_iter, double tol, double abs_tol);
/* preconditioner: "jacobi" (all) or "amg" (p; aggregation AMG V-cycle, the amgxpOptions
 * AGGREGATION solver's role) -- p defaults to "amg", U/Y/E to "jacobi" */
int dfmi_set_preconditioner(dfmi_ctx* ctx, const char* eqn, const char* name);
/* implementation options by key (the role of the reference's amgx*Options files, e.g.
 * examples/dfLowMachFoam/notorch/threeD_reactingTGV/H2/cvodeIntegrator/system/amgxpOptions:1-18, and of the
 * CanteraTorchProperties switches): "amg.*" (omega, overcorrection, coarsest_sweeps, coarsest_size,
 * presweeps, pairwise_passes_l0, pairwise_passes, precision 32|64, padded, tail, halo_l0, global_coarse,
 * smoother 0 weighted Jacobi | 1 multicolour DILU -- amgxpOptions "smoother=MULTICOLOR_DILU"; any other value is
 * refused, and so is 1 together with global_coarse),
 * "solver.*" (even_odd, small, row_classes), "pcg.*" (face_form, fuse_l0), "fv.*" (hex_walk, csr_walk,
 * species_generic, yprep_brick), "chem.*" (method 0 ROS3 | 1 extrapolation, generated, binning),
 * "les.*" (model, Ck, Ce, Cw, Prt, Sct: dfmi_turbulence_correct above),
 * "ras.*" (model, Cmu, C1, C2, C3, sigmak, sigmaEps, kMin, epsilonMin, Prt, Sct: the same call's RAS block),
 * "tci.*" (model, mixing, chemistry, Cmix, fuel, oxidizer, CO2, H2, version, C1, C2, Cgamma, Ctau, exp1, exp2:
 * dfmi_combustion_correct below),
 * "fgm.*" (model, combustion, solveEnthalpy, flameletT, Sct, Sc, incompPref, TMin, TMax: the flareFGM block below),
 * "spray.*" (model, rho, U, Yi, h: the spray block above),
 * "dnn.tuned_gemm", "step.courant" (1: dfmi_time_step queues the Courant-number kernel behind its last
 * kernel and posts the result to pinned memory for dfmi_courant_no; 0, the default: nothing added); keys and
 * defaults in INTEGRATION.md. Solver-structure keys must be set before the first solve; unknown keys fail. */
int dfmi_set_option(dfmi_ctx* ctx, const char* key, double value);
int dfmi_get_option(dfmi_ctx* ctx, const char* key, double* value);
/* AMG hierarchy after the first p solve: level count, cells and ELL width per level (with several ranks
 * and the option amg.global_coarse the agglomerated coarsest level of all ranks is listed last) */
int dfmi_amg_info(dfmi_ctx* ctx, int max_levels, int* n_levels, int* cells, int* width);
/* Inspection of the p preconditioner, in the role of dfmi_get_matrix (no reference counterpart: AmgX keeps its
 * smoother data to itself). Both are valid after the first p solve with the AMG preconditioner, on one rank, and
 * fail cleanly otherwise.
 * dfmi_amg_smoother_info: the colour of every row of `level` (as doubles; count = the level's cells, dfmi_amg_info)
 * and, with amg.smoother = 1, the DILU factor E of that level's current operator, in the V-cycle's precision
 * widened to double; with amg.smoother = 0 colour is all zero and dilu_diag the level's diagonal.
 * dfmi_amg_apply: z = V-cycle(r) (count = cells) with the hierarchy and operators of the last build, through the
 * launch-per-level path (no PCG fusion), either smoother. The fp64 Jacobi V-cycle reads level 0 from the solver's
 * rows: there the call (and level 0 of dfmi_amg_smoother_info) fails once a later solve has overwritten them
 * -- set amg.reuse = 0 and call right after the p solve; stale values are never read. */
int dfmi_amg_smoother_info(dfmi_ctx* ctx, int level, double* colour, double* dilu_diag, long count);
int dfmi_amg_apply(dfmi_ctx* ctx, const double* r, double* z, long count);
/* gather-row classes in use (0: explicit columns): after the first solve, the number of distinct
 * (column offset, coefficient source) rows the solver / assembly gathers decode from one byte per cell
 * instead of reading 2 W ints (hex boxes in blockMesh order: 27). Measurement aid (no reference
 * counterpart; the reference's ldu_to_csr keeps explicit CSR columns, dfMatrixDataBase.cu:166-177). */
int dfmi_row_classes(dfmi_ctx* ctx, int* n_classes);
/* hex box in blockMesh order detected at the first solve (every cell's face rows checked against the
 * computed i + nx (j + ny k) walk the assembly kernels then use instead of loading indices): nx, ny, nz,
 * or zeros. Measurement aid (no reference counterpart). */
int dfmi_hex_dims(dfmi_ctx* ctx, int* nx, int* ny, int* nz);
/* last solve: iterations and final relative residual */
int dfmi_solver_stats(dfmi_ctx* ctx, const char* eqn, int* iters, double* res0, double* rel_res);
/* work done by the solves of `eqn` since the last reset: the sum over solves and systems of the
 * iterations performed (each one = one PCG SpMV, or two BiCGStab SpMVs, of one system); reset != 0
 * zeroes the counter after reading. Measurement aid for bench.py (no reference counterpart). */
int dfmi_solver_work(dfmi_ctx* ctx, const char* eqn, double* system_iterations, int reset);

/* ---- chemistry (dfChemistryModel::solveSingle, dfChemistryModel.C:737-780; GPU ABI
 * precedent opencc_ode_init/opencc_ode_all, YEqn.H:45-77) ------------------------------------- */
/* mechanism arrays as laid out by deepflame-dev_amd/dfmi/kinetics.py (Mechanism.pack):
 * idata[R][8] (type: 0 elementary, 1 three-body, 2 Lindemann, 3 Troe; reversible; n_reac; n_prod;
 * has_T2), irs[R][6] (reactant ids, product ids, -1 padded), ddata[R][17+S] (A, b, Ta, nu_r[3],
 * nu_p[3], A0, b0, Ta0, Troe A/T3/T1/T2, efficiencies[S]) in SI kmol units; the NASA7 and molecular
 * weights come from the thermo coefficients */
int dfmi_chem_set_mechanism(dfmi_ctx* ctx, int n_reactions, const int* idata, const int* irs, const double* ddata);
/* mode 0 off, 1 stiff ODE integration each YEqn (chemistry->solve(deltaT)), 2 DNN surrogate;
 * tolerances on mass fractions (reference CVODE: relTol 1e-6, absTol 1e-10); cells below T_min get RR = 0 */
int dfmi_chem_set_options(dfmi_ctx* ctx, int mode, double rtol, double atol, double T_min);
/* integrate every cell over dt as a closed constant-volume reactor at fixed T whose state is
 * Cantera's setState_TPY(T, p, Y) (Y clipped at 0 and normalised, density p W/(R T);
 * dfChemistryModel.C:755) -> field "RR" = (Y(dt) - Y) rho / dt with rho the field "rho" (the thermo
 * density, problem.rhoi; inside dfmi_time_step / dfmi_Y_process: "rho_old", the thermo density before
 * this step's rhoEqn). 4..64 species, at most 256 reactions. Field "chem_stats" [3][C] = accepted steps (-1: step limit hit), rejected steps,
 * the step size the integration ended with (the next solve's first step). Returns non-zero when any
 * cell hit the step limit (its RR is then not a completed integration). */
int dfmi_chem_solve(dfmi_ctx* ctx, double dt);
/* ---- turbulence-chemistry interaction: combustion->correct() (YEqn.H:76) with combustionModel PaSR or EDC
 * (src/dfCombustionModels/PaSR/PaSR.C:205-396, EDC/EDC.C:83-171; the reference computes both on the host through Cantera and
 * has neither on its GPU path). The statement below is the definition; SMALL = small = 1e-15, vGreat = 1e300.
 * Options (dfmi_set_option; an unknown tci.* key is refused by name; coefficients positive and finite):
 *   tci.model      0 none (default) | 1 PaSR | 2 EDC
 *   tci.mixing     1 globalScale | 2 kolmogorovScale | 3 geometriMeanScale       (PaSR; dynamicScale is refused by name)
 *   tci.chemistry  1 globalConvertion | 2 formationRate | 3 reactionRate          (PaSR)
 *   tci.Cmix 0.1
 *   tci.fuel, tci.oxidizer, tci.CO2, tci.H2     species indices, -1 = not considered (default -1)
 *   tci.version    1981 | 1996 | 2005 (default) | 2016                            (EDC)
 *   tci.C1 0.05774, tci.C2 0.5, tci.Cgamma 2.1377, tci.Ctau 0.4083
 *   tci.exp1, tci.exp2   0 = the version's own (3,3 / 2,3 / 2,2 / 2,2); otherwise an integer 1..4; a power g^e is the
 *                        product ((g g) g) g taken left to right, never pow
 *   tci.bad_tauStar      get only: cells of the last EDC call whose tauStar was not a positive finite number
 * tci.model != 0 needs ras.model = 1 (k and epsilon exist only there) and chemistry mode 1; together with les.model != 0 or
 * with chemistry mode 2 (DNN) it is refused. tci.chemistry = 1 without tci.fuel >= 0 is an error naming the key
 * (PaSR.C:259-264). The reference looks CO2 and H2 up unconditionally and dies on a mechanism without them; here an index
 * of -1 leaves that species out of the maximum.
 * Inputs per cell, all as they stand when the call runs: k, epsilon, mu, rho, T, p, Y, RR. Inside dfmi_time_step rho is the
 * field after the rhoEqn (the rho combustionModel::rho() sees at YEqn.H:76), mu the thermo's, k and epsilon the previous
 * step's. RR is scaled by the density the solve is scaled by (dfmi_chem_solve).
 * PaSR: first laminar::correct(), the solve over dt. Then with e = epsilon + SMALL
 *   tmix  1: Cmix k / e     2: sqrt(|mu / rho / e|)     3: sqrt(|k / e| sqrt(|mu / rho / e|))
 *   tc    1 globalConvertion (:284-317), t0 = the cell's tci_tc before the call (the field starts at 0.1 and persists):
 *            t_ox  = (RR_ox  < 0 && Y_ox  > 1e-10) ? -rho Y_ox  / RR_ox  : t0      t_fuel likewise (RR < 0)
 *            t_CO2 = (RR_CO2 > 0 && Y_CO2 > 1e-10) ?  rho Y_CO2 / RR_CO2 : t0      t_H2 as the fuel (RR < 0)
 *            tc = max(max(max(t_ox, t_fuel), t_CO2), t_H2), a species with index -1 left out
 *         2 formationRate (laminar.C:75-102): tc = max_i (|RR_i| > small ? Y_i / |RR_i| : 0), from 0, in species order
 *         3 reactionRate (:326-377): cSum = sum_i X_i, X_i = rho Y_i / W_i. The gas state is Cantera's setState_TPX(T, p, X):
 *            x_i = max(X_i, 0) / sum_j max(X_j, 0), C_i = x_i (p / (R T)). fwd_r / rev_r are getFwdRatesOfProgress /
 *            getRevRatesOfProgress (third-body and fall-off factors included, rev_r = 0 for an irreversible reaction),
 *            wf_r = sum_products nu_p fwd_r, wr_r = sum_reactants nu_r rev_r, sumW = sum_r (wf_r + wr_r) and
 *            sumSq = sum_r (wf_r^2 + wr_r^2), each accumulated as wf then wr per reaction in reaction order;
 *            tc = sumSq == 0 ? vGreat : sumW / sumSq * cSum
 *   kappa = (tmix > SMALL && tc > SMALL) ? tc / (tc + tmix) : 1
 * EDC: first kappa and tauStar from the fields as they stand (tc in v2016: the formationRate form of the RR the previous
 * solve left), then chemistryPtr_->solve(tauStar): every cell is integrated over its own interval,
 * RR_i = (Y_i(tauStar) - Y_i) rho / tauStar (dfChemistryModel.C:770). With nu = mu / (rho + small), pow025(x) = sqrt(sqrt(x))
 *   v1981/1996/2005: gammaL = Cgamma pow025(nu eps / (k^2 + small));  tauStar = Ctau sqrt(nu / (eps + small))
 *   v2016:           Da = max(min(sqrt(nu / (eps + small)) / tc, 10), 1e-10);  ReT = k^2 / (nu eps + small)
 *                    CtauI = min(C1 / (Da sqrt(ReT + 1)), 2.1377);  CgammaI = max(min(C2 sqrt(Da (ReT + 1)), 5), 0.4082)
 *                    gammaL = CgammaI pow025(nu eps / (k^2 + small));  tauStar = CtauI sqrt(nu / (eps + small))
 *   kappa = gammaL >= 1 ? 1 : max(min(gammaL^exp1 / (1 - gammaL^exp2), 1), 0)
 * A cell whose tauStar is not a positive finite number gets RR = 0, kappa as computed and a count in tci.bad_tauStar (the
 * reference divides by zero there). A cell below T_min keeps its rule: RR = 0.
 * Consumers (PaSR.C:401-404,423-430, EDC.C:176-191): the YEqn source is kappa RR_i and the heat release kappa Qdot; the EEqn
 * is untouched (absolute enthalpy, no Qdot term). Fields: tci_kappa, tci_tmix, tci_tauStar [C] (get), tci_tc [C] (get and
 * set; reset to 0.1 when tci.model or tci.chemistry changes), RR_eff [S][C] and Qdot_eff [C] (get). RR and Qdot stay the
 * chemistry's own unscaled values; with tci.model != 0 the YEqn assemblies (dfmi_Y_process, dfmi_assemble("Y" / "Y_ell"),
 * dfmi_time_step) read RR_eff where they read RR.
 * With tci.model = 0 this call is dfmi_chem_solve(dt) and nothing else. dfmi_time_step and dfmi_Y_process call it where they
 * call the chemistry. Returns non-zero when a cell hit the step limit, as the solve does. The CPU-A baseline keeps the keys
 * and refuses tci.model != 0 by name. */
int dfmi_combustion_correct(dfmi_ctx* ctx, double dt);
/* ---- flareFGM: combustion->correct() with combustionModel flareFGM (dfLowMachFoam.C:328-455; src/dfCombustionModels/FGM/
 * baseFGM/baseFGM.C:478-912, flareFGM/flareFGM.C:122-762, flameletTableSolver/tableSolver.C; the reference computes it on the
 * host). The non-LES, non-spray branch; DESIGN.md 18. The statement below is the definition.
 * Options (dfmi_set_option; an unknown fgm.* key is refused by name):
 *   fgm.model 0 none (default) | 1 flareFGM;   fgm.combustion, fgm.solveEnthalpy, fgm.flameletT  0 (default) | 1
 *   fgm.Sct 0.7, fgm.Sc 1, fgm.TMin 200, fgm.TMax 5000 (positive and finite);   fgm.incompPref -10 (any finite value)
 * Table (dfmi_fgm_set_table): dims[10] = NH NZ NC NGZ NGC NZC NS NYomega NY NZL; axes = the six axes h, z, c, gz, gc, gzc
 * one after the other; laminar [5][NH NZL] = z, sl, th, tau, kctau; tables [NS + NY][NH NZ NC NGZ NGC NZC] in the reference's
 * index order (readThermChemTables.H: variable v of grid point (h, z, c, gz, gc, gzc), the last index fastest) -- variables
 * 0..7 = omgc, cOc, ZOc, cp, mwt, hiyi, Tf, nu, then the NYomega source terms, then (unscaled only) Ycmax, then the NY species;
 * d2Yeq, d1Yeq [NH NZ NGZ] when NS == 8 + NYomega (scaled progress variable), not read (may be null) when NS == 9 + NYomega
 * (unscaled); species_index [NY] and omega_index [NYomega]: the mechanism indices of the table's species and of its source
 * species. Call it after dfmi_set_constant_values. Refused by name: any other NS; a dimension < 1; NZL < 2; an axis (or a row
 * of the laminar z) that is not strictly increasing; a value that is not finite; a species index outside [0, num_species);
 * value tables of more than 2^28 entries in all (2 GiB; the host transposes them once).
 * These checks keep every gather index inside its table; the kernels clamp through locate / intfac only.
 * Lookups (tableSolver.C:425-498, 602-869): locate(n, a, x) = 0 for n == 1 or x <= a[0], n - 2 for x >= a[n-1], else the i with
 * a[i] <= x < a[i+1]; fac = 0 for x <= low, 1 for x >= high, 0 for high - low < 1e-30, else (x - low) / (high - low); AN AXIS
 * OF LENGTH 1 HAS fac = 0 (the reference reads a[1] past the end there: DESIGN.md 9). With w(i, f) = (1 - f) + i (2 f - 1),
 * i = 0, 1, a 6-D lookup is  sum over i0..i5 (i0 outermost) of  (((((w0 w1) w2) w3) w4) w5) table[corner],  accumulated as
 * result = result + factor * value; the upper corner index of an axis is loc + 1 where its length > 1, else loc. lookup2d on
 * the laminar block locates z on the block's FIRST row (tableSolver.C:782-795 passes z_Tb5 itself); lookup3d is (h, z, gz).
 * Fields (cells and boundary_<name>; allocated at the first use of the model): Z Zvar c cvar Zcvar Ha (set / get; patch types
 * of the same names: zeroGradient, fixedValue, cyclic, processor, processorCyclic, empty); get: chi_Z chi_Zc chi_c omega_c
 * cOmega_c ZOmega_c Ha_s c_s Zvar_s cvar_s Zcvar_s Wt Cp Hf (Wt, Cp, Hf start at 28.96, 1010.1, 1907), omega_Yi [NYomega]
 * (component j: the source term of species omega_index[j]), fgm_D, fgm_Su; the retrieval also writes T, psi, mu, rho,
 * rho_thermo and the NY table species of Y.
 * dfmi_fgm_retrieve: flareFGM::retrieval() as the constructor calls it, per cell and per boundary slot from the slot's own
 * values, in this order (small = 1e-4, smaller = 1e-6, SMALL = 1e-15; max / min are (a > b ? a : b) / (a < b ? a : b)):
 *   chi_Z = eps / k Zvar;  chi_Zc = eps / k Zcvar;  hLoss = min(max((Z (Hfu - Hox) + Hox) - Ha, h[0]), h[NH-1]);  ih = locate(h, hLoss)
 *   Zl = z_lam[ih][0], Zr = z_lam[ih][NZL-1];  flame = Z >= Zl && Z <= Zr && fgm.combustion && c > small
 *   flame:  kc_s, tau, sl, dl = lookup2d(hLoss, Z) of kctau, tau, sl, th;  nu = mu / rho (both as they stand on entry)
 *           Ka = (dl / (sl + SMALL)) / (sqrt(nu / eps) + SMALL);  Kc = kc_s tau;  C3 = 1.5 sqrt(Ka) / (1 + sqrt(Ka));
 *           C4 = 1.1 / pow(1 + Ka, 0.4);  chi_c = rho / 6.7 cvar ((2 Kc - tau C4) sl / (dl + SMALL) + C3 eps / (k + SMALL))
 *   else:   chi_c = eps / k cvar  (cells),  eps / (k + SMALL) cvar  (slots)
 *   gvar(m, v, Y) = max(smaller, min(1, m < small || m > 1 - small ? 0 : v / (m ((Y < 0 ? 1 : Y) - m))))
 *   gz = gvar(Z, Zvar, -1);  gcz = fmax(-1, fmin(1, cvar < 1e-4 || Zvar < 1e-6 ? 0 : Zcvar / (sqrt(Zvar) sqrt(cvar))))
 *   scaled: Ycmax = -1, cNorm = c;  unscaled: Ycmax = max(smaller, lookup6d(hLoss, Z, 0, gz, 0, 0) of table NS - 1), cNorm = c / Ycmax
 *   gc = gvar(c, cvar, Ycmax);  every other lookup6d is at (hLoss, Z, cNorm, gz, gc, gcz)
 *   flame:  omega_c = table 0 + (scaled ? chi_Z c lookup3d(d2Yeq) + 2 chi_Zc lookup3d(d1Yeq) : 0);  cOmega_c = table 1;
 *           ZOmega_c = table 2;   else all three 0;   then each times rho (as it stands on entry)
 *   Ha_s = hLoss, c_s = cNorm, Zvar_s = gz, cvar_s = gc, Zcvar_s = gcz;  Wt = table 4;  mu = table 7 times rho (on entry)
 *   Y[species_index[j]] = table NS + j;  omega_Yi[j] = table NS - NYomega + j
 *   fgm.flameletT: T = table 6 (Cp, Hf untouched);  else Cp = table 3, Hf = table 5, T = (Ha - Hf) / Cp + 298.15
 *   T = min(max(T, TMin), TMax);  psi = Wt / (8.314e3 T)
 *   slots: rho = rho_thermo = (incompPref > 0 ? incompPref : p) psi.  cells: rho is left alone (timeIndex == 0,
 *   flareFGM.C:747) and rho_thermo = rho.
 * Empty slots are untouched, processor [internal n] slots copy their cell, and the results cross processor patches in one
 * exchange afterwards (several ranks: a collective), as dfmi_thermo_correct's do. Kernels k_fgm_retrieve_cells /
 * k_fgm_retrieve_slots.
 * dfmi_fgm_correct: flareFGM::correct(). First transport(), each equation
 *   ddt(rho, psi) + div(phi, psi) - laplacian(D, psi) == Su,   D = (rho nut) / Sct + mu / Sc  (cells and slots alike)
 * through the k and epsilon equations' generic assembly (dfmi_turbulence_correct, RAS block: Euler ddt with rho_old and the
 * field's own value, the laplacian scheme in force) with Sp = 0, solved under its own name ("Z", "Zvar", "c", "cvar", "Zcvar",
 * "Ha": dfmi_set_solver / _stats / _work, dfmi_assemble / dfmi_get_matrix), its boundary values corrected and exchanged, then
 * clipped on cells and slots, psi = max(min(psi, upper), lower):  Z [0, 1], Zvar [0, 0.25], c [0, 1] (cMax_ stays 1 in both PV
 * modes: baseFGM.C:805 assigns Ycmaxall_, which is never set from the table), cvar [0, 0.25], Zcvar [-0.25, 0.25]; Ha is not
 * clipped. Order Z, Zvar, then with fgm.combustion c, cvar, Zcvar, then with fgm.solveEnthalpy Ha. Su per unit volume, with
 * mut = rho nut, a(g1, g2) = ((2 mut) / Sct) ((g1x g2x + g1y g2y) + g1z g2z) and the Gauss gradients of Z and c as they stand
 * (just solved and clipped), chi_* and the omegas as the previous retrieval left them:
 *   Z: 0    Zvar: a(gZ, gZ) - (2 rho) chi_Z    c: omega_c    cvar: (a(gc, gc) - (2 rho) chi_c) + 2 (cOmega_c - omega_c c)
 *   Zcvar: (a(gZ, gc) - (2 rho) chi_Zc) + (ZOmega_c - omega_c Z)    Ha: 0
 * div(phi,Z) ... div(phi,Ha): dfmi_set_scheme, upwind (default) | limitedLinear <k> | limitedLinear01 <k>. Without
 * fgm.solveEnthalpy, Ha = Z (Hfu - Hox) + Hox on every cell and slot. Last the retrieval above, which now also writes the
 * cells' rho = rho_thermo = (incompPref > 0 ? incompPref : p) psi.
 * dfmi_time_step with fgm.model = 1: rhoEqn; UEqn; dfmi_fgm_correct; per pressure corrector rho = rho_thermo, psip0 = psi p,
 * the p equation, rho_thermo += psi p - psip0 (the corrector of dfmi_thermo_set_eos) and, in the last one, the rhoEqn;
 * kEpsilon::correct(); rho = rho_thermo. No YEqn, no EEqn, no thermo call, no chemistry. While fgm.model = 1,
 * dfmi_thermo_update_rho and dfmi_thermo_correct_psip_rho act on rho_thermo as under an equation of state.
 * Refused by name: fgm.model = 1 without a table, with ras.model != 1, les.model != 0, tci.model != 0, chemistry mode != 0 or an
 * equation of state set (at dfmi_set_option and again at the calls); dfmi_Y_process, dfmi_E_process and dfmi_zero_d_step while
 * fgm.model = 1; k, epsilon or a patch-type set of the six scalars missing. With fgm.model = 0 every launch of every other
 * entry is the one it was, and a context that never touches the model allocates what it did. The CPU-A baseline exports the
 * three entries, keeps the keys and refuses fgm.model = 1 by name. */
int dfmi_fgm_set_table(dfmi_ctx* ctx, const int* dims, const double* axes, double Hfu, double Hox, const double* laminar,
                       const double* tables, const double* d2Yeq, const double* d1Yeq, const int* species_index,
                       const int* omega_index);
int dfmi_fgm_retrieve(dfmi_ctx* ctx);
int dfmi_fgm_correct(dfmi_ctx* ctx);
/* n_steps df0DFoam time steps (applications/solvers/df0DFoam/df0DFoam.C:99-113, YEqn.H, EEqn.H;
 * zeroDReactor constantProperty pressure): per step chemistry.solve(dt) on every cell, YEqn
 * ddt(rho, Yi) == RR_i (Yi.max(0), inert = 1 - sum), he held, correctThermo (T from he), rho = p psi.
 * Every cell is an independent 0D reactor (BASELINE config 1). The steps are queued without a host
 * synchronisation between them; a chemistry step-limit failure in any of them fails the call once the batch
 * has run (the message gives the count summed over the steps). */
int dfmi_zero_d_step(dfmi_ctx* ctx, double dt, int n_steps);
/* integrator step budget per cell and solve (default 100000); exceeding it is an error of the call */
int dfmi_chem_set_max_steps(dfmi_ctx* ctx, int max_steps);
/* which integrator the last solve used: 0 data-driven generic kernel (one cell per lane, 4..12 species), > 0 a
 * mechanism compiled in by dfmi/chem_codegen.py (1 Burke2012_s9r23, 2 ES80_H2-7-16), -1 the cooperative kernel
 * (several lanes per cell: 13..64 species, or any count from 4 under option chem.coop = 1; ROS3 only) */
int dfmi_chem_info(dfmi_ctx* ctx, int* generated);

/* ---- DF-ODENet surrogate (dfChemistrySolver::setConstantValue/Inference,
 * dfChemistrySolver.cu:78-206; model test/Tu500K-Phi1/inference.py:12-25) ---------------------- */
/* n_modules = S - 1 nets (species 0..S-2; the inert species must be last), each n_layers Linear
 * layers dims[0] = S+2 -> ... -> dims[n_layers] = 1 with GELU between; params (fp32) per module, per
 * layer: weight [out][in] (torch Linear layout) then bias [out]. Normalisation Xmu/Xstd [S+2],
 * Ymu/Ystd [S-1] (the reference hard-codes the H2 values, :95-105). Cells with T >= T_react
 * (reference 610 K) react; RR = (y_new - Y) rho (p/101325) / dt_infer (reference 1e-6). Inference
 * runs in fp16 (MFMA) with fp32 accumulation, as the reference's .to(kHalf) modules. */
int dfmi_dnn_set_model(dfmi_ctx* ctx, int n_modules, int n_layers, const int* dims, const float* params,
                       const double* x_mu, const double* x_std, const double* y_mu, const double* y_std,
                       double T_react, double dt_infer);
/* the same model from a packed file (magic "DFMIDNN1", n_modules, n_layers, dims, the four normalisation vectors,
 * the params above; written by deepflame-dev_amd/dfmi/dnn_checkpoint.py from a checkpoint in inference.py's
 * state_dict layout) -- the file-path entry the reference's setConstantValue has (torch::jit::load of
 * new_Temporary_Chemical_<i>.pt, dfChemistrySolver.cu:112-126), without executing a TorchScript program */
int dfmi_dnn_load_model(dfmi_ctx* ctx, const char* path, double T_react, double dt_infer);
/* run the surrogate on the current T, p, Y -> field "RR" (0 for non-reacting cells), scaled by field
 * "rho" (inside dfmi_time_step: "rho_old", as the reference passes d_rho_old, dfYEqn.cu:449) */
int dfmi_dnn_infer(dfmi_ctx* ctx, int* n_reacting);
/* reacting cells of the last inference; algorithmic hidden-layer GEMM flops since the last call */
int dfmi_dnn_stats(dfmi_ctx* ctx, int* n_reacting, double* gemm_flops);
/* the GEMM kernel form the next dfmi_dnn_infer takes for each hidden layer of the installed model under the current
 * "dnn.tuned_gemm" (n_layers = Linear layers - 1; at most max_layers kinds written): 0 generic 256x128x32 ring,
 * 1 128x128x64 input-layer kernel, 2 256x256x64 ping-pong, 3 ping-pong with two 16-column tail strips, 4 generic with
 * the output layer fused, 5 ping-pong with the output layer fused. Inspection aid in the role of dfmi_amg_info; no
 * reference counterpart. */
int dfmi_dnn_plan(dfmi_ctx* ctx, int max_layers, int* n_layers, int* kinds);

/* ---- communication accounting per exchange point (multi-rank runs). The reference issues one NCCL group
 * per field and processor patch (dfMatrixOpBase.cu:441-485, dispatch :2402-2491; comm set up at
 * dfNcclBase.cu:23-65) and times only whole equations (TIME_GPU, dfMatrixOpBase.H:42-82). on != 0 resets
 * and arms: every halo exchange (one ncclSend/ncclRecv group per exchange point) and every all-gather is
 * bracketed by HIP events on the stream it runs on and its bytes sent counted, keyed by the exchange point
 * ("fields rho", "bicgstab Y", "pcg p amg", "allgather pcg p", ...); on == 0 disarms. */
int dfmi_comm_timer(dfmi_ctx* ctx, int on);
/* synchronise and write {"point": {"calls": n, "bytes": b, "ms": t}, ...} (JSON) into buf (len bytes);
 * *needed = the length it takes including the terminator */
int dfmi_comm_report(dfmi_ctx* ctx, char* buf, int len, int* needed);

/* ---- kernel timing (the reference's TICK_START_EVENT / TICK_END_EVENT cudaEvent pairs,
 * src_gpu/dfMatrixOpBase.H:46-60): arm HIP-event timing of every launch of one kernel
 * (name as in the source, e.g. "k_y_assemble"; "" disarms), recorded on the context stream */
int dfmi_kernel_timer(dfmi_ctx* ctx, const char* kernels);   /* comma-separated names; re-arming resets */
/* synchronise and return the summed duration and count of the first armed kernel's launches */
int dfmi_kernel_time(dfmi_ctx* ctx, double* total_ms, int* launches);
/* the same for one named armed kernel */
int dfmi_kernel_time_named(dfmi_ctx* ctx, const char* kernel, double* total_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* DFMI_H */
