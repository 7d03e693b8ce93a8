"""The numpy statement of the field inspector (include/deme_hip.h: deme_inspect_fields), written from the header's text.

Grid: nCells = n[0] * n[1] * n[2], cell id ix + n[0] * (iy + n[1] * iz).  An owner's cell: P its centre of mass in the world frame
(decoded position + (double)LBF), u = (P - origin) / cell in float64; inside iff 0 <= u_k < n[k] on all three axes (NaN: outside),
i_k = trunc(u_k).  A counted owner is an own clump (`own`: the caller builds the mask -- clump owners that are no ghost copies) inside
the grid.  Owner columns: sums over a cell's counted owners of 1, m, volume, m * v_k, (m * v_i) * v_j (xx, yy, zz, xy, xz, yz), every
factor converted to float64 first.  Contact columns: a row is counted as deme_inspect_contacts counts it; a side of a counted row
belongs to the cell of its owner if that owner is counted, and adds 1 and r (x) f (tests/_contact_sums64.py: rotate)."""
import numpy as np

from tests._contact_sums64 import rotate, row_owners

KINETIC_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def positions(decode, p, state):
    """owner centres of mass in the world frame, float64: decode = model.decode_positions"""
    X = decode(state["voxelID"], state["locX"], state["locY"], state["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    return X + np.array([float(p.LBFX), float(p.LBFY), float(p.LBFZ)], np.float64)


def cells_of(X, origin, cell, n):
    """(inside, cell id) per row of X; the id of an outside point is nCells"""
    origin, cell = np.asarray(origin, np.float64), np.asarray(cell, np.float64)
    n = np.asarray(n, np.int64)
    with np.errstate(invalid="ignore"):
        u = (np.asarray(X, np.float64) - origin) / cell
        inside = ((u >= 0.0) & (u < n.astype(np.float64))).all(1)
    i = np.where(inside[:, None], u, 0.0).astype(np.int64)
    cid = i[:, 0] + n[0] * (i[:, 1] + n[1] * i[:, 2])
    return inside, np.where(inside, cid, int(n.prod()))


def fields(X, state, own, owner_mass, owner_volume, origin, cell, n, whole=None, tables=None, thr=0.0):
    """X: positions(); state: the downloaded owner state; own: bool per owner; owner_mass / owner_volume: float32 per owner (the
    table entry of its inertia offset; owner_volume may be None); whole / tables: the whole list with records and the owner tables
    (None: the owner columns only).  Returns every column, abs_<column> (the sums of |term|), terms_owner and terms_side (terms per
    cell) and cell_of (per owner, nCells for an uncounted one)."""
    n_cells = int(np.prod(np.asarray(n, np.int64)))
    inside, cid = cells_of(X, origin, cell, n)
    counted = np.asarray(own, bool) & inside
    cell_of = np.where(counted, cid, n_cells)
    o = np.flatnonzero(counted)
    c = cell_of[o]
    m = np.asarray(owner_mass, np.float32)[o].astype(np.float64)
    v = np.stack([state[k][o].astype(np.float64) for k in ("vX", "vY", "vZ")], 1)
    mom = m[:, None] * v
    kin = np.stack([mom[:, i] * v[:, j] for i, j in KINETIC_PAIRS], 1)
    out = {"cell_of": cell_of, "clumps": np.bincount(c, minlength=n_cells).astype(np.uint32)}
    out["terms_owner"] = out["clumps"].astype(np.int64)
    terms = {"mass": m, "momentum": mom, "kinetic": kin}
    if owner_volume is not None:
        terms["volume"] = np.asarray(owner_volume, np.float32)[o].astype(np.float64)
    for name, t in terms.items():
        for key, val in ((name, t), ("abs_" + name, np.abs(t))):
            out[key] = np.zeros((n_cells,) + t.shape[1:])
            np.add.at(out[key], c, val)
    if whole is None:
        return out
    oA, oB = row_owners(whole, tables)
    f = whole["force"].astype(np.float64)
    thr = np.float64(np.float32(thr))
    row_counted = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2] >= thr * thr
    quat = np.stack([state[k].astype(np.float64) for k in ("oriQw", "oriQx", "oriQy", "oriQz")], 1)
    out["sides"] = np.zeros(n_cells, np.uint32)
    out["virial"], out["abs_virial"] = np.zeros((n_cells, 9)), np.zeros((n_cells, 9))
    out["side_cells"] = []  # per side (A, then B): the cell of every row's side, nCells where it is not counted
    for owner, cp, sign in ((oA, whole["cpA"], 1.0), (oB, whole["cpB"], -1.0)):
        take = row_counted & counted[owner]
        so = owner[take]
        r = rotate(quat[so], cp[take].astype(np.float64))
        ff = sign * f[take]
        term = (r[:, :, None] * ff[:, None, :]).reshape(-1, 9)
        sc = cell_of[so]
        np.add.at(out["virial"], sc, term)
        np.add.at(out["abs_virial"], sc, np.abs(term))
        out["sides"] += np.bincount(sc, minlength=n_cells).astype(np.uint32)
        out["side_cells"].append(np.where(take, cell_of[owner], n_cells))
    out["terms_side"] = out["sides"].astype(np.int64)
    return out
