"""The numpy statement of the contact inspectors (include/deme_hip.h: deme_inspect_contacts, deme_inspect_contact_counts).

A row of the list is COUNTED when (double)fx^2 + (double)fy^2 + (double)fz^2 >= (double)thr^2, f the recorded force.  A SIDE of a
counted row is counted when its owner's entry of `owner_mask` is set (the caller builds the mask: own clump owners inside the
region).  Side A carries +f and cpA, side B -f and cpB.  A counted side adds r (x) f, r = R(q) cp with the owner's stored quaternion
and R(q)v = v + 2w(u x v) + 2u x (u x v), u = (qx, qy, qz); everything converted to float64 first and computed there."""
import numpy as np


def row_owners(whole, tables):
    """both owners of every row: whole holds idA, idB, type of a whole-list download; tables = (sphere -> owner, triangle -> owner,
    analytical component -> owner)"""
    sph, tri, obj = tables
    a, b, t = whole["idA"], whole["idB"], whole["type"]
    oB = np.zeros(len(a), np.int64)
    for cls, table in ((t == 1, sph), (t == 2, tri), (t > 2, obj)):
        oB[cls] = table[b[cls]]
    return sph[a].astype(np.int64), oB


def rotate(q, v):
    """R(q) v for rows of quaternions (w, x, y, z) and vectors, float64"""
    w, u = q[:, :1], q[:, 1:]
    t = np.cross(u, v)
    return v + (2.0 * w) * t + 2.0 * np.cross(u, t)


def contact_sums(whole, tables, state, owner_mask, thr):
    """whole: idA, idB, type, force, cpA, cpB of the whole list; state: the downloaded owner state (oriQw .. oriQz); owner_mask: bool
    per owner.  Returns dict(virial (3, 3), sides, counts (per owner, uint32), abs_sum (3, 3) = sum |r_i| |f_j|)."""
    n_owners = len(owner_mask)
    oA, oB = row_owners(whole, tables)
    f = whole["force"].astype(np.float64)
    thr = np.float64(np.float32(thr))
    counted = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2] >= thr * thr
    quat = np.stack([state[k].astype(np.float64) for k in ("oriQw", "oriQx", "oriQy", "oriQz")], 1)
    virial, abs_sum = np.zeros((3, 3)), np.zeros((3, 3))
    counts = np.zeros(n_owners, np.uint32)
    sides = 0
    for owner, cp, sign in ((oA, whole["cpA"], 1.0), (oB, whole["cpB"], -1.0)):
        take = counted & owner_mask[owner]
        o = owner[take]
        r = rotate(quat[o], cp[take].astype(np.float64))
        ff = sign * f[take]
        virial += np.einsum("ni,nj->ij", r, ff)
        abs_sum += np.einsum("ni,nj->ij", np.abs(r), np.abs(ff))
        counts += np.bincount(o, minlength=n_owners).astype(np.uint32)
        sides += int(take.sum())
    return {"virial": virial, "sides": sides, "counts": counts, "abs_sum": abs_sum}
