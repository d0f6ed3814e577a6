"""NumPy float64 restatement of OpenFOAM-7's compressibleCourantNo.H (dfLowMachFoam.C:261) from host arrays, the
reference of the Courant-number tests on the CPU (CPU-A) and on the GPU:

    sumPhi_c  = (sum over the faces f of cell c of |phi_f|) / rho_c      fvc::surfaceSum(mag(phi)) / rho
    CoNum     = 0.5 max_c(sumPhi_c / V_c) dt
    meanCoNum = 0.5 (sum_c sumPhi_c / sum_c V_c) dt

Every internal face counts for its owner and its neighbour; every boundary face of every patch kind for its face
cell. A processor patch holds 2n slots [neighbour values n | patch-internal values n]: its n faces carry this rank's
flux in the FIRST n slots of boundary_phi, and only those are added. Empty patches have no faces.
"""
import numpy as np

EPS = 2.0 ** -52


def sum_phi(n_cells, owner, neighbour, patches, phi, boundary_phi, rho):
    """sumPhi per cell; patches = [(face_cells [n], first slot, kind)] in patch order"""
    s = np.zeros(n_cells)
    a = np.abs(np.asarray(phi, dtype=np.float64))
    np.add.at(s, np.asarray(owner), a)
    np.add.at(s, np.asarray(neighbour), a)
    b = np.abs(np.asarray(boundary_phi, dtype=np.float64))
    for fc, off, kind in patches:
        if kind == "empty":
            continue
        np.add.at(s, np.asarray(fc), b[off:off + len(fc)])
    return s / np.asarray(rho, dtype=np.float64)


def courant_from_arrays(n_cells, owner, neighbour, patches, phi, boundary_phi, rho, V, dt):
    sp = sum_phi(n_cells, owner, neighbour, patches, phi, boundary_phi, rho)
    V = np.asarray(V, dtype=np.float64)
    return 0.5 * float(np.max(sp / V)) * dt, 0.5 * (float(np.sum(sp)) / float(np.sum(V))) * dt


def mesh_patches(m):
    out, off = [], 0
    for p in m.patches:
        out.append((p.face_cells, off, p.kind))
        off += p.slots
    return out


def courant_no(m, phi, boundary_phi, rho, dt):
    """(CoNum, meanCoNum) on a dfmi.mesh.Mesh"""
    return courant_from_arrays(m.n_cells, m.owner, m.neighbour, mesh_patches(m), phi, boundary_phi, rho, m.volume, dt)


def faces_per_cell(m) -> int:
    """the most faces (internal and boundary) any cell has: the length of the longest per-cell sum"""
    n = np.bincount(m.owner, minlength=m.n_cells) + np.bincount(m.neighbour, minlength=m.n_cells)
    for fc, _, kind in mesh_patches(m):
        if kind != "empty":
            n = n + np.bincount(fc, minlength=m.n_cells)
    return int(n.max())


def tolerance(m, n_cells=None) -> float:
    """relative bound on the distance between two float64 evaluations of the formula that add the same terms in
    different orders, from the summation lengths alone: (faces per cell + C) 2^-52, C the cell count (of the whole
    mesh when it is decomposed). Every term is >= 0, so a sum of n terms in ANY order carries a relative error below
    n 2^-53 and two orders differ by less than n 2^-52: n = faces per cell for sumPhi_c (all CoNum needs), n = C for
    the sums over the cells. Both evaluations add the cells pairwise / as a tree (NumPy's sum; per-wave, per-block,
    per-grid on the device), whose error grows with log2 C rather than C, which leaves the room the few divisions
    and products and the second sum (of V) need."""
    return (faces_per_cell(m) + (n_cells or m.n_cells)) * EPS
