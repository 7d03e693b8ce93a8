"""The numpy statement of the per-triangle contact loads (include/deme_hip.h: deme_inspect_tri_loads).

A row of the list is counted when it is a sphere-mesh row (type 2) whose B is a triangle id < n_tri, the owner of sphere A is no
ghost copy, and (double)fx^2 + (double)fy^2 + (double)fz^2 >= (double)thr^2 with f the fp32 record 0 and thr the fp32 value the call
is given.  A counted row adds -f to its triangle, in fp64 (np.add.at: row order), and 1 to the triangle's count."""
import numpy as np

SPHERE_MESH = 2


def tri_loads(idA, idB, ctype, force, sphere_owner, owner_is_ghost, n_tri, thr):
    """-> dict: force [n_tri, 3] float64, counts [n_tri] uint32, abs_sum [n_tri, 3] float64 (sum of |f| per component over the counted
    rows: what a tolerance is relative to), counted (bool per row)"""
    idA, idB, ctype = np.asarray(idA, np.int64), np.asarray(idB, np.int64), np.asarray(ctype)
    f = np.asarray(force, np.float32).astype(np.float64).reshape(-1, 3)
    sphere_owner = np.asarray(sphere_owner, np.int64)
    ghost = np.zeros(int(sphere_owner.max(initial=-1)) + 1, bool) if owner_is_ghost is None else np.asarray(owner_is_ghost, bool)
    thr2 = float(np.float32(thr)) ** 2
    f2 = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2]
    counted = (ctype == SPHERE_MESH) & (idB < n_tri) & (f2 >= thr2)
    counted[counted] &= ~ghost[sphere_owner[idA[counted]]]
    out = np.zeros((n_tri, 3), np.float64)
    abs_sum = np.zeros((n_tri, 3), np.float64)
    counts = np.zeros(n_tri, np.uint32)
    np.add.at(out, idB[counted], -f[counted])
    np.add.at(abs_sum, idB[counted], np.abs(f[counted]))
    np.add.at(counts, idB[counted], 1)
    return {"force": out, "counts": counts, "abs_sum": abs_sum, "counted": counted}
