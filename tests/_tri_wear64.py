"""The numpy statement of one mesh-wear sample (include/deme_hip.h: deme_tri_wear_enable).

A row of the list is counted as deme_inspect_tri_loads counts it (tests/_tri_loads64.py): a sphere-mesh row (type 2) whose B is a
triangle id < n_tri, the owner of sphere A no ghost copy, (double)fx^2 + (double)fy^2 + (double)fz^2 >= (double)thr^2.  Everything is
fp64 over the fp32 values as stored:
    R(q)v = v + 2w(u x v) + 2u x (u x v), u = (qx, qy, qz), the stored quaternion not renormalised
    rA = R(qA) cpA, rB = R(qB) cpB;  wA = R(qA) omgBar_A, wB alike;  vA = v_A + wA x rA, vB = v_B + wB x rB;  u = vA - vB
    g = -f;  N = R(qB) ((n2 - n1) x (n3 - n1));  N.N > 0: nh = N / sqrt(N.N), Fn = g.nh, gt = g - Fn nh, ut = u - (u.nh) nh
    lanes, each times w:  g_x, g_y, g_z, |Fn|, |Fn| |ut|, |gt| |ut|  (a degenerate face adds 0 to the last three)
A counted row adds its lanes to its triangle (np.add.at: row order) and 1 to the triangle's rows."""
import numpy as np

SPHERE_MESH = 2
REL = 1e-10  # the bound of every comparison is REL * abs_scale


def rotate(q, v):
    """R(q)v row by row; q = (w, x, y, z) columns"""
    w, u = q[:, :1], q[:, 1:]
    t = np.cross(u, v)
    s = np.cross(u, t)
    return v + (2.0 * w) * t + 2.0 * s


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def owner_columns(state):
    """(q [n, 4], v [n, 3], omega [n, 3]) float64 of a download_state() dict"""
    q = np.stack([_f64(state[k]) for k in ("oriQw", "oriQx", "oriQy", "oriQz")], 1)
    v = np.stack([_f64(state[k]) for k in ("vX", "vY", "vZ")], 1)
    om = np.stack([_f64(state[k]) for k in ("omgBarX", "omgBarY", "omgBarZ")], 1)
    return q, v, om


def tri_wear(whole, state, tri_nodes, tri_owner, owner_is_ghost, n_tri, thr, w):
    """whole: idA, idB, type, ownerA, force, cpA, cpB of every row (tests/test_owner_contacts.py::_whole_list); state: the owners'
    columns as download_state gives them; tri_nodes: (n1, n2, n3), each [n_tri, 3], owner-local; tri_owner [n_tri].
    -> dict: lanes [n_tri, 6] float64, rows [n_tri] uint64, counted (bool per row), abs_scale [n_tri, 6] float64 -- per triangle and
    lane the sum over its counted rows of the magnitudes before any cancellation: w |f| for lanes 0 to 3,
    w |f| (|v_A| + |w_A| |r_A| + |v_B| + |w_B| |r_B|) for lanes 4 and 5 -- and u_max, the largest |u| of a counted row"""
    idB, ctype = np.asarray(whole["idB"], np.int64), np.asarray(whole["type"])
    oA = np.asarray(whole["ownerA"], np.int64)
    f = _f64(whole["force"]).reshape(-1, 3)
    q, vel, om = owner_columns(state)
    ghost = np.zeros(len(q), bool) if owner_is_ghost is None else np.asarray(owner_is_ghost, bool)
    thr2 = float(np.float32(thr)) ** 2
    w = float(w)
    f2 = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2]
    counted = (ctype == SPHERE_MESH) & (idB < n_tri) & (f2 >= thr2)
    counted[counted] &= ~ghost[oA[counted]]
    lanes = np.zeros((n_tri, 6), np.float64)
    scale = np.zeros((n_tri, 6), np.float64)
    rows = np.zeros(n_tri, np.uint64)
    out = {"lanes": lanes, "rows": rows, "counted": counted, "abs_scale": scale, "u_max": 0.0}
    if not counted.any():
        return out
    assert int(counted.sum()) < 100000  # (the bound's derivation: n * 1.1e-16 with n < 1e5)
    tri = idB[counted]
    a, b = oA[counted], np.asarray(tri_owner, np.int64)[tri]
    g = -f[counted]
    n1, n2, n3 = (_f64(x).reshape(-1, 3)[tri] for x in tri_nodes)
    rA, rB = rotate(q[a], _f64(whole["cpA"]).reshape(-1, 3)[counted]), rotate(q[b], _f64(whole["cpB"]).reshape(-1, 3)[counted])
    wA, wB = rotate(q[a], om[a]), rotate(q[b], om[b])
    u = (vel[a] + np.cross(wA, rA)) - (vel[b] + np.cross(wB, rB))
    N = rotate(q[b], np.cross(n2 - n1, n3 - n1))
    NN = (N * N).sum(1)
    ok = NN > 0
    nh = np.zeros_like(N)
    nh[ok] = N[ok] / np.sqrt(NN[ok])[:, None]
    Fn = (g * nh).sum(1)
    gt = g - Fn[:, None] * nh
    ut = u - (u * nh).sum(1)[:, None] * nh
    slide = np.sqrt((ut * ut).sum(1))
    term = np.zeros((len(tri), 6))
    term[:, :3] = w * g
    term[:, 3] = np.where(ok, w * np.abs(Fn), 0.0)
    term[:, 4] = np.where(ok, w * (np.abs(Fn) * slide), 0.0)
    term[:, 5] = np.where(ok, w * (np.sqrt((gt * gt).sum(1)) * slide), 0.0)
    norm = lambda x: np.sqrt((x * x).sum(1))
    fmag = norm(g)
    speed = norm(vel[a]) + norm(wA) * norm(rA) + norm(vel[b]) + norm(wB) * norm(rB)
    mag = np.zeros((len(tri), 6))
    mag[:, :4] = (w * fmag)[:, None]
    mag[:, 4:] = (w * fmag * speed)[:, None]
    np.add.at(lanes, tri, term)
    np.add.at(scale, tri, mag)
    np.add.at(rows, tri, np.uint64(1))
    out["u_max"] = float(norm(u).max())
    return out
