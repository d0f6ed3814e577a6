"""Domain-decomposed runs on one GPU vs the undecomposed run (MI355X).

Several ranks share the card through the in-process transport (dfmi_set_comm_local: one host thread
per rank, halo messages as device copies); everything else -- exchange lists, packing, processor
slots, halo columns in the SpMV, rank-ordered reductions -- is the code the RCCL path runs. RCCL itself
refuses two ranks on one device; it is exercised by `bench.py --gpus N` under torchrun.

Tolerance: one outer iteration with tight solver tolerances; processor faces turn internal faces into
coupled boundary slots (different summation order), so fields agree to ~1e-10 relative, not bitwise.
The decomposed run is also checked against the oracle (exact solves on the undecomposed mesh).
"""
import os
import threading

import numpy as np
import pytest

from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

_HUB = [100]


def _setup(m, t, ym, dt, comm=None, schemes=None):
    from dfmi.lib import Context
    from dfmi import case
    ctx = Context(0)
    inert = ym["species"].index("N2")
    case.setup_context(ctx, m, t, inert, dt, case.default_patch_types(m), comm=comm, schemes=schemes)
    for e in ("U", "Y", "E"):
        ctx.set_solver(e, 300, 1e-14, 1e-300)
    ctx.set_solver("p", 3000, 1e-14, 1e-300)
    return ctx


def _run(nx, ny, nz, decomp, n_steps=1, gradings=(1.0, 1.3, 1.0), periodic=True, renumber=None, overlap=False,
         schemes=None, perturb=False, env=None, timers=True):
    from dfmi.mesh import hex_box, global_cell_ids
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi import case
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
    L = (2 * np.pi * 1e-3,) * 3
    dt = 1e-6
    mg = hex_box(nx, ny, nz, lengths=L, gradings=gradings, periodic=(periodic,) * 3)
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    if perturb:   # every species non-uniform and no mirror symmetry (see test_decomposed_case_schemes_...)
        x = mg.cell_centres / np.array(L)
        ph = np.arange(t.S)[:, None]
        f["Y"] = f["Y"] * (1 + 0.02 * np.sin(2 * np.pi * x[:, 0] + 0.3 + ph) * np.cos(2 * np.pi * x[:, 1] + 0.7 * ph)
                           * (1 + 0.1 * np.sin(2 * np.pi * x[:, 2] + 0.2)))
        f["Y"] /= f["Y"].sum(axis=0)
    # undecomposed reference
    ctx = _setup(mg, t, ym, dt, schemes=schemes)
    case.init_state(ctx, mg, t.S, f["T"], f["p"], f["U"], f["Y"])
    ctx.call("pre_time_step")
    orc = None
    if n_steps == 1:   # the oracle (sequential restatement + exact solves) on the same initial state
        import oracle as O
        st = case.pull_state(ctx, mg, t.S)
        orc = O.Oracle(mg, t, {k: v.copy() for k, v in st.items()}, case.default_patch_types(mg),
                       ym["species"].index("N2"), 1.0 / dt, schemes=schemes)
        orc.time_step(2)
    for _ in range(n_steps):
        ctx.time_step(2)
    ref = {n: ctx.get_field(n, (mg.n_cells,)) for n in ("T", "p", "rho", "he")}
    ref["U"] = ctx.get_field("U", (3, mg.n_cells))
    ref["Y"] = ctx.get_field("Y", (t.S, mg.n_cells))
    ctx.close()

    nr = int(np.prod(decomp))
    meshes = [hex_box(nx, ny, nz, lengths=L, gradings=gradings, periodic=(periodic,) * 3, decomp=decomp, rank=r)
              for r in range(nr)]
    if renumber:      # every rank block renumbered (procCols follow the peers' new local ids)
        from dfmi.renumber import renumber_mesh
        meshes = [renumber_mesh(mm, renumber)[0] for mm in meshes]
    gids = [global_cell_ids(mm, nx, ny) for mm in meshes]
    out = [None] * nr
    err = [None] * nr
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            m = meshes[r]
            g = gids[r]
            c = _setup(m, t, ym, dt, comm={"hub": hub, "nranks": nr, "rank": r}, schemes=schemes)
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            c.call("pre_time_step")
            if timers:
                c.kernel_timer("k_bcg_eo")   # whether the even-odd BiCGStab ran (the ranks' colourings agree)
            else:
                c.comm_timer(True)           # no kernel timers: the time step keeps its side stream
            for _ in range(n_steps):
                c.time_step(2)
            o = {n: c.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he")}
            if timers:
                o["eo"] = c.kernel_time("k_bcg_eo")[1]
                c.kernel_timer("")
            else:
                o["comm"] = c.comm_report()
                o["proc_faces"] = int(m.proc_rows_cols()[0].size)
                c.comm_timer(False)
            o["U"] = c.get_field("U", (3, m.n_cells))
            o["Y"] = c.get_field("Y", (t.S, m.n_cells))
            o["stats"] = {e: c.solver_stats(e) for e in ("U", "Y", "E", "p")}
            out[r] = o
            c.close()
        except Exception as e:   # surfaced below
            err[r] = e

    # DFMI_HALO_OVERLAP is read when a rank's communicator is set up (inside work); `env` holds AMG options
    # (dfmi_set_option) every rank's context takes at creation
    from dfmi import lib
    prev = os.environ.get("DFMI_HALO_OVERLAP")
    os.environ["DFMI_HALO_OVERLAP"] = "1" if overlap else "0"
    for k, v in (env or {}).items():
        lib.DEFAULT_OPTIONS[k] = v
    th = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    for k in (env or {}):
        lib.DEFAULT_OPTIONS.pop(k, None)
    if prev is None:
        os.environ.pop("DFMI_HALO_OVERLAP", None)
    else:
        os.environ["DFMI_HALO_OVERLAP"] = prev
    assert not any(x.is_alive() for x in th), "decomposed run hung"
    for e in err:
        if e is not None:
            raise e
    # reassemble global fields
    glob = {}
    for n in ("T", "p", "rho", "he"):
        a = np.zeros(mg.n_cells)
        for r in range(nr):
            a[gids[r]] = out[r][n]
        glob[n] = a
    for n, k in (("U", 3), ("Y", t.S)):
        a = np.zeros((k, mg.n_cells))
        for r in range(nr):
            a[:, gids[r]] = out[r][n]
        glob[n] = a
    # all ranks agree on solver iteration counts (rank-ordered global reductions)
    for r in range(1, nr):
        assert out[r]["stats"]["p"][0] == out[0]["stats"]["p"][0]
    glob["p_iters"] = out[0]["stats"]["p"][0]
    glob["eo_launches"] = [out[r].get("eo") for r in range(nr)]
    glob["comm"] = [out[r].get("comm") for r in range(nr)]
    glob["proc_faces"] = [out[r].get("proc_faces") for r in range(nr)]
    glob["stats"] = [out[r]["stats"] for r in range(nr)]
    if orc is not None:
        ref["oracle"] = {n: orc[n] for n in ("T", "p", "rho", "he", "U", "Y")}
    return ref, glob


@pytest.mark.parametrize("decomp", [(2, 1, 1), (1, 2, 2), (2, 2, 2)])
def test_decomposed_step_matches_single_domain(decomp):
    ref, glob = _run(8, 6, 4, decomp)
    for n in ("T", "p", "rho", "he", "U", "Y"):
        e = rel_err(glob[n], ref[n])
        assert e < 1e-9, (n, e)
        e = rel_err(glob[n], ref["oracle"][n])      # decomposed GPU run vs the oracle itself
        assert e < 1e-9, ("oracle", n, e)


@pytest.mark.parametrize("dims,decomp,eo", [((8, 6, 4), (2, 2, 2), True), ((9, 6, 4), (3, 1, 1), False),
                                             ((12, 6, 4), (3, 1, 1), True)])
def test_decomposed_even_odd_bicgstab(dims, decomp, eo):
    """The even-odd BiCGStab across ranks: every rank colours its block, the colours across processor faces
    are exchanged and the ranks' flips solved from the all-gathered relations (odd block extents 3 x ... make
    neighbouring ranks' local colourings disagree, which the flips repair); a periodic direction of odd
    length (9) has no 2-colouring and every rank keeps the Jacobi path. Either way the oracle's exact solves."""
    ref, glob = _run(*dims, decomp)
    assert all((n > 0) == eo for n in glob["eo_launches"]), glob["eo_launches"]
    for n in ("T", "p", "rho", "he", "U", "Y"):
        e = rel_err(glob[n], ref["oracle"][n])
        assert e < 1e-9, ("oracle", n, e)


@pytest.mark.parametrize("decomp", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("which", ["case", "ll"])
def test_decomposed_case_schemes_match_single_domain(decomp, which):
    """the reference cases' schemes on a decomposed mesh: the multivariate limiter on processor faces reads
    the neighbour cells' gradients through the halo (LimitedScheme::calcLimiter's patchNeighbourField),
    K's gradient and cubic's component gradients likewise; "ll" = limitedLinear 1 for Yi_h (every face
    limited from gradients) + limitedLinear01 1 for K.

    The unbounded multivariate limiter is discontinuous where one field of the table is uniform: its
    phi_N - phi_P is rounding noise, and r jumps between the NVDTVD branches with the summation order of
    the gradients (a processor face sums the same terms in another order than the internal face it
    replaces) -- the reference's own sensitivity (OpenFOAM would flip there between decompositions too).
    The synthetic TGV state has such a field (N2: the same mass fraction burnt and unburnt) and mirror
    planes, so the "ll" case perturbs every species with a smooth asymmetric field."""
    sch = {"div(phi,Yi_h)": "limitedLinear01 1", "div(phi,K)": "limitedLinear 1", "div(hDiffCorrFlux)": "cubic"}
    if which == "ll":
        sch = dict(sch, **{"div(phi,Yi_h)": "limitedLinear 1", "div(phi,K)": "limitedLinear01 1"})
    ref, glob = _run(8, 6, 4, decomp, schemes=sch, perturb=which == "ll")
    for n in ("T", "p", "rho", "he", "U", "Y"):
        e = rel_err(glob[n], ref[n])
        comp = [rel_err(glob[n][k], ref[n][k]) for k in range(3)] if n == "U" else None
        # the perturbed "ll" state: U measured at 2.8e-9 (per-component scale) for (2, 2, 2), held at 1e-8
        tol = 1e-8 if (n == "U" and which == "ll") else 1e-9
        assert e < tol, (n, e, comp)
        e = rel_err(glob[n], ref["oracle"][n])
        assert e < tol, ("oracle", n, e, comp)


def test_decomposed_renumbered_step_matches_single_domain():
    ref, glob = _run(8, 8, 4, (2, 2, 1), renumber="morton")
    for n in ("T", "p", "rho", "he", "U", "Y"):
        e = rel_err(glob[n], ref["oracle"][n])
        assert e < 1e-9, ("oracle", n, e)


def test_decomposed_walls_two_steps():
    ref, glob = _run(8, 4, 4, (2, 2, 1), n_steps=2, periodic=False)
    for n in ("T", "p", "rho", "U", "Y"):
        e = rel_err(glob[n], ref[n])
        assert e < 1e-9, (n, e)


def _distorted_polymesh(nx, ny, nz, periodic, distort=0.15, seed=5):
    import tempfile
    from dfmi.polymesh import hex_polymesh, write_polymesh, read_polymesh
    L = 2 * np.pi * 1e-3
    P, faces, own, nei, bnd = hex_polymesh(nx, ny, nz, lengths=(L,) * 3, periodic=periodic, gradings=(1.0, 1.3, 1.0))
    h = L / np.array([nx, ny, nz])
    inner = np.all((P > 1e-12) & (P < L - 1e-12), axis=1)
    P = P.copy()
    P[inner] += distort * h * np.random.default_rng(seed).uniform(-1, 1, (inner.sum(), 3))
    d = tempfile.mkdtemp()
    write_polymesh(os.path.join(d, "constant", "polyMesh"), P, faces, own, nei, bnd)
    return d, (P, faces, own, nei, bnd), read_polymesh(os.path.join(d, "constant", "polyMesh"))


@pytest.mark.parametrize("method,nparts,from_dirs,mesh", [("rcb", 3, False, "distorted"), ("graph", 4, True, "distorted"),
                                                          ("graph", 2, False, "refined")],
                         ids=["rcb-3-False", "graph-4-True", "refined-graph-2"])
def test_partitioned_polymesh_matches_oracle(method, nparts, from_dirs, mesh):
    """An arbitrary (non-orthogonal, read from constant/polyMesh) mesh cut by the partitioners
    (dfmi/partition.py: RCB / recursive graph bisection; processor + processorCyclic patches), optionally
    through processor* directories written and read back; the decomposed run equals the oracle's
    single-domain step. "refined": the 2:1 refined box of tests/unstructured_meshes.py (W = 9, hanging nodes) --
    processor patches with faces of unequal size and halo columns in rows of unequal length; its cut crosses
    z-normal faces off the Taylor-Green symmetry plane, whose flux is exactly zero while phiUc is not (both ranks
    once took the upwind weight there: T off by 6.5e-7, U by 3.7e-4)."""
    import oracle as O
    from dfmi import case
    from dfmi.mech import read_thermo_table, read_yaml_mechanism
    from dfmi.partition import partition_cells, decompose, write_decomposed, read_decomposed
    ym = read_yaml_mechanism(os.path.join(GOLDEN, "ES80_H2-7-16.yaml"))
    t = read_thermo_table(os.path.join(GOLDEN, "thermo_ES80_H2-7-16.txt"), ym["species"])
    dt = 1e-6
    if mesh == "refined":
        import unstructured_meshes as um
        d, raw, mg = None, None, um.get("refined")
    else:
        d, raw, mg = _distorted_polymesh(8, 6, 5, (True, False, True))
    f = case.tgv_fields(mg, ym["species"], kernel_radius=1.2e-3)
    ctx = _setup(mg, t, ym, dt)
    case.init_state(ctx, mg, t.S, f["T"], f["p"], f["U"], f["Y"])
    ctx.call("pre_time_step")
    st = case.pull_state(ctx, mg, t.S)
    ctx.close()
    orc = O.Oracle(mg, t, {k: v.copy() for k, v in st.items()}, case.default_patch_types(mg),
                   ym["species"].index("N2"), 1.0 / dt)
    orc.time_step(2)
    part = partition_cells(mg, nparts, method)
    if from_dirs:
        write_decomposed(d, *raw, part)
        meshes = read_decomposed(d)
    else:
        meshes = decompose(mg, part)
    if mesh == "refined":
        assert all(np.unique(np.round(p.mag_sf / p.mag_sf.max(), 6)).size > 1
                   for mm in meshes for p in mm.patches if p.kind == "processor")
    else:
        assert any(p.kind == "processorCyclic" for mm in meshes for p in mm.patches)
    nr = len(meshes)
    out, err = [None] * nr, [None] * nr
    hub = _HUB[0]; _HUB[0] += 1

    def work(r):
        try:
            m = meshes[r]
            g = m.cell_map
            c = _setup(m, t, ym, dt, comm={"hub": hub, "nranks": nr, "rank": r})
            case.init_state(c, m, t.S, f["T"][g], f["p"][g], f["U"][:, g], f["Y"][:, g])
            c.call("pre_time_step")
            c.time_step(2)
            o = {n: c.get_field(n, (m.n_cells,)) for n in ("T", "p", "rho", "he")}
            o["U"] = c.get_field("U", (3, m.n_cells))
            o["Y"] = c.get_field("Y", (t.S, m.n_cells))
            out[r] = o
            c.close()
        except Exception as e:
            err[r] = e

    overlap = method == "graph"   # the graph-partitioned cases run the overlapped solver halos
    # DFMI_HALO_OVERLAP is read when a rank's communicator is set up (inside work)
    prev = os.environ.get("DFMI_HALO_OVERLAP")
    os.environ["DFMI_HALO_OVERLAP"] = "1" if overlap else "0"
    th = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    if prev is None:
        os.environ.pop("DFMI_HALO_OVERLAP", None)
    else:
        os.environ["DFMI_HALO_OVERLAP"] = prev
    assert not any(x.is_alive() for x in th), "decomposed run hung"
    for e in err:
        if e is not None:
            raise e
    for n, k in (("T", 1), ("p", 1), ("rho", 1), ("he", 1), ("U", 3), ("Y", t.S)):
        a = np.zeros((k, mg.n_cells))
        for r in range(nr):
            a[:, meshes[r].cell_map] = out[r][n].reshape(k, -1)
        ref = orc[n].reshape(k, -1)
        e = rel_err(a, ref)
        assert e < 1e-9, (n, e)


@pytest.mark.parametrize("decomp", [(2, 1, 1), (2, 2, 2)])
def test_overlapped_halo_step_matches(decomp):
    """Solver halos on the comm stream (DFMI_HALO_OVERLAP=1): the interior rows of every SpMV run while
    the exchange is in flight, the boundary rows after it. Same per-row arithmetic, reductions summed in
    two halves: agrees with the in-order exchange to rounding, with the oracle to 1e-9, and is bitwise
    reproducible run to run."""
    ref, g1 = _run(10, 8, 6, decomp, overlap=True)
    _, g0 = _run(10, 8, 6, decomp, overlap=False)
    _, g2 = _run(10, 8, 6, decomp, overlap=True)
    for n in ("T", "p", "rho", "he", "U", "Y"):
        assert np.array_equal(g1[n], g2[n]), ("run-to-run", n)
        e = rel_err(g1[n], g0[n])
        assert e < 1e-11, ("overlap vs in-order", n, e)
        e = rel_err(g1[n], ref["oracle"][n])
        assert e < 1e-9, ("oracle", n, e)


def test_overlapped_halo_walls_two_steps():
    ref, glob = _run(8, 4, 4, (2, 2, 1), n_steps=2, periodic=False, overlap=True)
    for n in ("T", "p", "rho", "U", "Y"):
        e = rel_err(glob[n], ref[n])
        assert e < 1e-9, (n, e)


@pytest.mark.parametrize("env", [{"amg.halo_l0": 0}, {"amg.global_coarse": 1},
                                 {"amg.global_coarse": 1, "amg.halo_l0": 0}], ids=["blockjacobi", "global", "global-bj"])
def test_decomposed_amg_variants_match_oracle(env):
    """the decomposed-AMG variants (level 0 smoothed with its processor couplings -- the default -- or
    block-Jacobi; the opt-in agglomerated coarsest level of all ranks) precondition the same PCG: one outer
    iteration matches the single-domain run and the oracle on a mesh with coarse levels on every rank (768
    cells per rank, 2 x 2 x 2)"""
    ref, glob = _run(24, 16, 16, (2, 2, 2), env=env)
    for n in ("T", "p", "rho", "he", "U", "Y"):
        e = rel_err(glob[n], ref[n])
        assert e < 1e-9, (n, e)
        e = rel_err(glob[n], ref["oracle"][n])
        assert e < 1e-9, ("oracle", n, e)


def test_halo_coupled_level0_needs_fewer_pcg_iterations():
    """the V-cycle's level 0 with its processor couplings (default) against block-Jacobi across ranks: the same
    solution, fewer p-iterations (2 x 2 x 2 ranks of 16^3)"""
    ref, hal = _run(32, 32, 32, (2, 2, 2), n_steps=2)
    _, bj = _run(32, 32, 32, (2, 2, 2), n_steps=2, env={"amg.halo_l0": 0})
    print("p-iterations: halo-coupled", hal["p_iters"], "block-Jacobi", bj["p_iters"])
    assert hal["p_iters"] < bj["p_iters"], (hal["p_iters"], bj["p_iters"])
    for n in ("T", "p", "rho", "he", "U", "Y"):
        assert rel_err(hal[n], ref[n]) < 1e-9, n
        assert rel_err(bj[n], ref[n]) < 1e-9, n


def test_decomposed_side_stream_one_colour_halos_single_reduction_pcg():
    """Round 6's multi-rank step: the side stream (chemistry, YEqn front, EEqn scheme terms) runs at N > 1 with
    its field halos on the halo's second channel (reported as "... @side" points); the even-odd BiCGStab
    exchanges carry one colour's faces (fewer bytes per call than a full exchange of the same vectors); the PCG
    takes ONE all-gather per iteration (single-reduction form). Against the oracle's exact solves to 1e-9."""
    ref, glob = _run(12, 8, 8, (2, 2, 2), timers=False)
    for n in ("T", "p", "rho", "he", "U", "Y"):
        e = rel_err(glob[n], ref["oracle"][n])
        assert e < 1e-9, ("oracle", n, e)
    for r, comm in enumerate(glob["comm"]):
        side = [k for k in comm if k.endswith("@side")]
        assert any(k.startswith("fields sumYDiffError hDiffCorrFlux") for k in side), sorted(comm)
        assert not any(k.startswith("bicgstab") or k.startswith("pcg") for k in side), side
        H = glob["proc_faces"][r]
        e = comm["bicgstab E"]
        assert e["bytes"] / e["calls"] < 0.75 * 8.0 * H, (e, H)   # mostly half-face (one-colour) messages
        # PCG: per iteration one all-gather (+ the setup's); the standard form takes two
        its = glob["stats"][r]["p"][0]
        ag = comm.get("allgather pcg p", {}).get("calls", 0)
        assert 0 < ag <= 3 * (its + 3), (ag, its)
