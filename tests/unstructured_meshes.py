"""Unstructured test meshes: boxes whose cells are not all hexahedra, written as constant/polyMesh and
read back through dfmi.polymesh (so the reader's polygon branches are in the loop).

A cell is a list of outward faces, a face a tuple of lattice point keys (integer triples). Faces are
de-duplicated by vertex set; the lower cell id owns a face and the face keeps the owner's orientation
(normal owner -> neighbour). Internal faces are sorted by (owner, neighbour) -- OpenFOAM's upper-triangular
order -- and boundary faces are grouped into front/back/left/right/top/down (mesh.hex_box's patch order) by
face centre and sorted by centre inside each patch, so the two halves of a cyclic pair line up.

Families (sizes of the small members in brackets):

  prisms(nx, ny, nz, frac, seed)   an nx x ny x nz box whose (i, j) columns are cut, with probability
      `frac`, into two triangular prisms along a diagonal drawn per column; the same cut in every layer.
      frac = 1.0 [7, 5, 3: 210 cells, W = 5]; frac = 0.5 ("hexprism") [156 cells, W = 6 without being a
      hex box].
  refined(nx, ny, nz)              a coarse box whose cells with I < nx // 2 are split 2 x 2 x 2. A coarse cell
      behind the interface carries four quads on that side, and the coarse faces that touch the interface
      carry the hanging mid-edge node (5-vertex polygons) [6, 3, 3: 243 cells, W = 9].

None of them 2-colours; every one has rows of unequal length, so the gather rows carry padding in
interior rows."""
import tempfile

import numpy as np

L0 = 2 * np.pi * 1e-3
PATCH_ORDER = ("front", "back", "left", "right", "top", "down")      # mesh.hex_box's order
_SIDE = {"left": (0, 0), "right": (0, 1), "down": (1, 0), "top": (1, 1), "back": (2, 0), "front": (2, 1)}


def _hex_faces(p):
    """outward quads of a hexahedron from its 8 corner keys p[dz][dy][dx]"""
    return [(p[0][0][0], p[0][1][0], p[0][1][1], p[0][0][1]),      # z-
            (p[1][0][0], p[1][0][1], p[1][1][1], p[1][1][0]),      # z+
            (p[0][0][0], p[0][0][1], p[1][0][1], p[1][0][0]),      # y-
            (p[0][1][0], p[1][1][0], p[1][1][1], p[0][1][1]),      # y+
            (p[0][0][0], p[1][0][0], p[1][1][0], p[0][1][0]),      # x-
            (p[0][0][1], p[0][1][1], p[1][1][1], p[1][0][1])]      # x+


def _box(x0, y0, z0, s):
    return [[[(x0 + s * dx, y0 + s * dy, z0 + s * dz) for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]


def _prism_faces(tri, k):
    """outward faces of the prism over the counter-clockwise (seen from +z) triangle `tri` of (i, j)
    keys, between layers k and k + 1"""
    lo = [(i, j, k) for i, j in tri]
    hi = [(i, j, k + 1) for i, j in tri]
    out = [tuple(lo[::-1]), tuple(hi)]
    for a in range(3):
        b = (a + 1) % 3
        out.append((lo[a], lo[b], hi[b], hi[a]))
    return out


def build(cells, nodes, cyclic_z=False):
    """cells: list of lists of outward faces over integer point keys; nodes: three coordinate arrays
    indexed by key component. Returns (points, faces, owner, neighbour, boundary) for write_polymesh."""
    seen = {}                       # vertex set -> face index in `flist`
    flist, own, nei = [], [], []
    for c, faces in enumerate(cells):
        for f in faces:
            key = frozenset(f)
            assert len(key) == len(f)
            if key in seen:
                i = seen[key]
                assert nei[i] < 0 and own[i] != c, "a face is shared by more than two cells"
                nei[i] = c
            else:
                seen[key] = len(flist)
                flist.append(f); own.append(c); nei.append(-1)
    own = np.array(own); nei = np.array(nei)
    keys = sorted({p for f in flist for p in f})
    pid = {p: i for i, p in enumerate(keys)}
    K = np.array(keys)
    points = np.stack([np.asarray(nodes[d])[K[:, d]] for d in range(3)], axis=1)
    top = [len(nodes[d]) - 1 for d in range(3)]
    internal = np.nonzero(nei >= 0)[0]
    internal = internal[np.lexsort((nei[internal], own[internal]))]
    order = list(internal)
    boundary = []
    bfaces = np.nonzero(nei < 0)[0]
    groups = {n: [] for n in PATCH_ORDER}
    for i in bfaces:
        k = np.array(flist[i])
        for name, (axis, side) in _SIDE.items():
            if np.all(k[:, axis] == (top[axis] if side else 0)):
                ta = [a for a in range(3) if a != axis]
                groups[name].append(((float(k[:, ta[1]].mean()), float(k[:, ta[0]].mean())), i))
                break
        else:
            raise AssertionError("a boundary face lies on no side of the box")
    opp = {"front": "back", "back": "front"}
    for name in PATCH_ORDER:
        g = sorted(groups[name])
        cyc = cyclic_z and name in opp
        boundary.append((name, "cyclic" if cyc else "patch", len(g), len(order), opp[name] if cyc else None))
        order += [i for _, i in g]
    faces = [[pid[p] for p in flist[i]] for i in order]
    Fi = len(internal)
    return points, faces, own[order].astype(np.int32), nei[order][:Fi].astype(np.int32), boundary


def _mesh(cells, nodes, cyclic_z):
    from dfmi.polymesh import read_polymesh, write_polymesh
    P, faces, own, nei, bnd = build(cells, nodes, cyclic_z)
    with tempfile.TemporaryDirectory() as d:
        write_polymesh(d, P, faces, own, nei, bnd)
        m = read_polymesh(d)
    m.face_sizes = np.array([len(f) for f in faces])
    return m


def _nodes(n, lengths, gradings):
    from dfmi.mesh import _axis_nodes
    return [_axis_nodes(n[d], lengths[d], gradings[d]) for d in range(3)]


def prism_cuts(nx, ny, frac, seed):
    """per column: -1 = a hexahedron, 0 = cut along (i, j)-(i+1, j+1), 1 = along (i+1, j)-(i, j+1)"""
    rng = np.random.default_rng(seed)
    cut = rng.random((nx, ny)) < frac
    diag = rng.integers(0, 2, (nx, ny))
    return np.where(cut, diag, -1)


def prisms(nx, ny, nz, frac=1.0, seed=1, cyclic_z=False, lengths=(L0,) * 3, gradings=(1.0, 1.3, 1.0)):
    cuts = prism_cuts(nx, ny, frac, seed)
    cells = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                p00, p10, p11, p01 = (i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)
                if cuts[i, j] < 0:
                    cells.append(_hex_faces(_box(i, j, k, 1)))
                elif cuts[i, j] == 0:
                    cells += [_prism_faces((p00, p10, p11), k), _prism_faces((p00, p11, p01), k)]
                else:
                    cells += [_prism_faces((p00, p10, p01), k), _prism_faces((p10, p11, p01), k)]
    return _mesh(cells, _nodes((nx, ny, nz), lengths, gradings), cyclic_z)


def refined(nx, ny, nz, cyclic_z=False, lengths=(L0,) * 3, gradings=(1.0, 1.3, 1.0)):
    """keys live on the doubled lattice: a coarse cell spans 2 units, a fine one 1"""
    n = (nx, ny, nz)
    fine = lambda I, J, K: I < nx // 2
    inside = lambda c: all(0 <= c[d] < n[d] for d in range(3))
    fine_pts = set()
    for K in range(nz):
        for J in range(ny):
            for I in range(nx):
                if fine(I, J, K):
                    fine_pts |= {(2 * I + a, 2 * J + b, 2 * K + c) for a in range(3) for b in range(3) for c in range(3)}
    mid = lambda a, b: tuple((u + v) // 2 for u, v in zip(a, b))
    # neighbour offset of each face of _hex_faces
    nbr = [(0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)]
    cells = []
    for K in range(nz):
        for J in range(ny):
            for I in range(nx):
                if fine(I, J, K):
                    for c in range(2):
                        for b in range(2):
                            for a in range(2):
                                cells.append(_hex_faces(_box(2 * I + a, 2 * J + b, 2 * K + c, 1)))
                    continue
                faces = []
                for q, off in zip(_hex_faces(_box(2 * I, 2 * J, 2 * K, 2)), nbr):
                    o = (I + off[0], J + off[1], K + off[2])
                    m4 = [mid(q[e], q[(e + 1) % 4]) for e in range(4)]
                    if inside(o) and fine(*o):      # four quads against the four fine cells
                        ctr = mid(q[0], q[2])
                        for e in range(4):
                            faces.append((q[e], m4[e], ctr, m4[e - 1]))
                    else:                           # hanging mid-edge nodes of the interface
                        f = []
                        for e in range(4):
                            f.append(q[e])
                            if m4[e] in fine_pts:
                                f.append(m4[e])
                        faces.append(tuple(f))
                cells.append(faces)
    return _mesh(cells, _nodes((2 * nx, 2 * ny, 2 * nz), lengths, gradings), cyclic_z)


# ---------------------------------------------------------------- the families the tests run
# name -> (constructor, W, histogram of internal faces per cell or None, cells)
SMALL = {"prisms": (lambda **kw: prisms(7, 5, 3, 1.0, 1, **kw), 5, [0, 0, 6, 39, 116, 49], 210),
         "hexprism": (lambda **kw: prisms(7, 5, 3, 0.5, 1, **kw), 6, [0, 0, 0, 24, 80, 46, 6], 156),
         "refined": (lambda **kw: refined(6, 3, 3, **kw), 9, [0, 0, 0, 8, 44, 101, 81, 4, 4, 1], 243)}
# above 4096 cells, not a multiple of 64: batched solvers, multi-level AMG, ragged last workgroups
LARGE = {"prisms": (lambda **kw: prisms(23, 19, 7, 1.0, 1, **kw), 5, None, 6118),
         "hexprism": (lambda **kw: prisms(23, 19, 7, 0.5, 1, **kw), 6, None, 4662),
         "refined": (lambda **kw: refined(10, 11, 9, **kw), 9, None, 4455)}

_cache = {}


def get(name, size="small", cyclic_z=False):
    """the mesh of a family (built once per process; treat it as read-only)"""
    key = (name, size, cyclic_z)
    if key not in _cache:
        _cache[key] = (SMALL if size == "small" else LARGE)[name][0](cyclic_z=cyclic_z)
    return _cache[key]


def faces_per_cell(m):
    return np.bincount(m.owner, minlength=m.n_cells) + np.bincount(m.neighbour, minlength=m.n_cells)


def ell_width(m):
    n = faces_per_cell(m)
    for p in m.patches:
        if p.kind in ("cyclic", "processor", "processorCyclic"):
            n = n + np.bincount(p.face_cells, minlength=m.n_cells)
    return int(n.max())


def is_bipartite(m):
    """2-colourability of the cell graph (internal faces and cyclic pairs)"""
    adj = [[] for _ in range(m.n_cells)]
    for o, n in zip(m.owner, m.neighbour):
        adj[o].append(n); adj[n].append(o)
    for p in m.patches:
        if p.kind == "cyclic":
            q = m.patches[p.neighbour_patch]
            for a, b in zip(p.face_cells, q.face_cells):
                adj[a].append(b)
    col = -np.ones(m.n_cells, int)
    for s in range(m.n_cells):
        if col[s] >= 0:
            continue
        col[s] = 0
        stack = [s]
        while stack:
            u = stack.pop()
            for v in adj[u]:
                if col[v] < 0:
                    col[v] = 1 - col[u]; stack.append(v)
                elif col[v] == col[u]:
                    return False
    return True


def wall_types(m, mixed=False):
    """the parity suite's wall conditions by patch name: fixedValue U / T / Y (fixedEnergy he) on left and right,
    zeroGradient (gradientEnergy he) elsewhere; mixed: fixedValue on left only and an open outlet on right
    (inletOutlet U / Y, waveTransmissive p)"""
    from dfmi.mesh import FIXED_VALUE, FIXED_ENERGY, GRADIENT_ENERGY, INLET_OUTLET, WAVE_TRANSMISSIVE
    fv = {}
    names = ("left",) if mixed else ("left", "right")
    fixed = [i for i, p in enumerate(m.patches) if p.name in names]
    for f in ("U", "T", "Y"):
        t = m.patch_types(0).copy()
        t[fixed] = FIXED_VALUE
        fv[f] = t
    t = m.patch_types(GRADIENT_ENERGY).copy()
    t[fixed] = FIXED_ENERGY
    fv["he"] = t
    if mixed:
        out = [i for i, p in enumerate(m.patches) if p.name == "right"]
        fv["U"][out] = INLET_OUTLET
        fv["Y"][out] = INLET_OUTLET
        fv["p"] = m.patch_types(0).copy()
        fv["p"][out] = WAVE_TRANSMISSIVE
    return fv


def closedness(m):
    """max over cells of |sum of outward face area vectors| relative to the largest face area (cyclic and
    wall faces included)"""
    s = np.zeros((m.n_cells, 3))
    np.add.at(s, m.owner, m.sf)
    np.add.at(s, m.neighbour, -m.sf)
    for p in m.patches:
        np.add.at(s, p.face_cells, p.sf)
    big = max(m.mag_sf.max(), max(p.mag_sf.max() for p in m.patches if p.size))
    return float(np.linalg.norm(s, axis=1).max() / big)


def uniform_fields(m, species):
    from dfmi import case
    yu, yb = case.h2_air_compositions(species)
    C = m.n_cells
    return {"T": np.full(C, 800.0), "p": np.full(C, 101325.0), "U": np.zeros((3, C)),
            "Y": np.repeat((0.5 * (yu + yb))[:, None], C, axis=1)}


def uniform_state_bounds(m, st, dt):
    """How far one outer iteration may move a uniform state at rest, from the mesh alone. The only
    non-zero input is the rounding residual of a cell's closed surface, |sum Sf| <= k eps sum |Sf| (k: faces
    per cell). Through grad p it gives U a push  dt p |sum Sf| / (rho V)  and through the pressure equation's
    flux divergence a relative density / pressure change of  dt |U| sum |Sf| / V; the scalars are held to 64 eps of
    their own magnitude plus that."""
    k = ell_width(m) + 2
    a_over_v = np.zeros(m.n_cells)
    np.add.at(a_over_v, m.owner, m.mag_sf); np.add.at(a_over_v, m.neighbour, m.mag_sf)
    for p in m.patches:
        np.add.at(a_over_v, p.face_cells, p.mag_sf)
    a_over_v = (a_over_v / m.volume).max()
    u = k * np.finfo(np.float64).eps * dt * st["p"].max() * a_over_v / st["rho"].min()
    scal = 64 * np.finfo(np.float64).eps + dt * u * a_over_v
    return u, scal
