"""Which contacts a detection must list, stated over ALL PAIRS in float64 (numpy).  No bins, no contact points, no sort: this is the
definition the detection's algorithm (bin spans, the contact-point-in-this-bin rule, the key sort) has to reproduce, not a
restatement of it.

Inputs are the scene arrays as the engine receives them (codec fields, component tables, analytical objects), the per-owner margins
of set_margins, the family masks and the family extra margins.  Every clump of a scene stated here is a single sphere at the owner's
centre or has the identity quaternion, so a sphere's centre is the owner's lattice point (int64, exact) plus the fp32 offset of the
component as it stands.

  inflated radius     R = float64(float32(r)) + float64(float32(margin of the owner))
  sphere - sphere     listed iff the owners differ, the families are not masked and (RA + RB) - |XA - XB| > min(extraA, extraB);
                      A is the sphere with the smaller id
  sphere - plane      depth = R + margin of the plane's owner - (XA - XP) . n                                  (type 11)
  sphere - cylinder   depth = R + margin of the cylinder's owner - s (radius - distance from the axis), s = +1 for a cylinder
                      that holds the spheres inside, -1 for a post                                            (type 13)
                      both listed iff not masked and depth > min(extra)            (sphere_entity of csrc/deme_device.h)

GREY BAND.  The engine forms r + margin in fp32 (and, for the objects, rounds the distance to fp32), the statement in fp64.  A pair
with |depth - threshold| <= 2^-22 x scale is "either": four fp32 units of scale = RA + RB for two spheres, R + |distance| for a
plane, R + radius + distance from the axis for a cylinder.  The band follows from the arithmetic, it is not measured; the function
counts the pairs inside it and the scenes are built so that the count is zero -- with that, nothing is excluded from a comparison.

The list comes out in the canonical order of the engine (by A, then sphere-sphere before sphere-object, then B) because the pairs
are enumerated in that order: rows of A, columns of B.
"""
import numpy as np

BAND = 2.0 ** -22
SS, PLANE, CYL = 1, 11, 13


def lattice_of(arrays, p, n=None):
    """owner centres in lattice units (int64) from the codec fields"""
    vid = np.asarray(arrays["voxelID"], np.uint64)[:n]
    nx, ny = np.uint64(int(p.nvXp2)), np.uint64(int(p.nvYp2))
    one = np.uint64(1)
    vx = (vid & ((one << nx) - one)).astype(np.int64)
    vy = ((vid >> nx) & ((one << ny) - one)).astype(np.int64)
    vz = (vid >> (nx + ny)).astype(np.int64)
    loc = [np.asarray(arrays[k], np.uint16)[:n].astype(np.int64) for k in ("locX", "locY", "locZ")]
    return np.stack([vx * 65536 + loc[0], vy * 65536 + loc[1], vz * 65536 + loc[2]], 1)


def inputs_of(arrays, p, margins, mask_pair, n_anal=None):
    """the statement's inputs from the arrays of a SceneBuilder (after the codec fields were written)"""
    comp = np.asarray(arrays["clumpComponentOffset"], np.int64)
    rel = np.stack([np.asarray(arrays[k], np.float32).astype(np.float64) for k in ("CDRelPosX", "CDRelPosY", "CDRelPosZ")], 1)
    fm = np.asarray(arrays["familyMasks"])
    f = np.arange(256)
    lo, hi = np.minimum(f[:, None], f[None, :]), np.maximum(f[:, None], f[None, :])
    assert mask_pair(3, 7) == (1 + 7) * 7 // 2 + 3
    masked = fm[(1 + hi) * hi // 2 + lo] != 0
    nA = len(arrays["objType"]) if n_anal is None else n_anal
    obj = dict(type=np.asarray(arrays["objType"], np.int64)[:nA], owner=np.asarray(arrays["objOwner"], np.int64)[:nA],
               rel=np.stack([np.asarray(arrays[k], np.float32).astype(np.float64) for k in ("objRelPosX", "objRelPosY", "objRelPosZ")], 1)[:nA],
               dir=np.stack([np.asarray(arrays[k], np.float32).astype(np.float64) for k in ("objRotX", "objRotY", "objRotZ")], 1)[:nA],
               size1=np.asarray(arrays["objSize1"], np.float32).astype(np.float64)[:nA],
               sign=np.asarray(arrays["objNormal"], np.float32).astype(np.float64)[:nA])
    return dict(G=lattice_of(arrays, p), l=float(p.l), sph_owner=np.asarray(arrays["ownerClumpBody"], np.int64), sph_rel=rel[comp],
                sph_r=np.asarray(arrays["Radii"], np.float32)[comp], margin=np.asarray(margins, np.float32),
                family=np.asarray(arrays["familyID"], np.int64), masked=masked,
                extra=np.asarray(arrays["familyExtraMarginSize"], np.float32).astype(np.float64), obj=obj)


def expected(s, rows=128, cols=2048):
    """(A, B, type) of every contact that must be listed, in canonical order, and the number of pairs inside the grey band"""
    own = s["sph_owner"]
    nS = len(own)
    l = s["l"]
    Gs = s["G"][own]                                                          # lattice point of the sphere's owner
    rel = s["sph_rel"]
    R = s["sph_r"].astype(np.float64) + s["margin"].astype(np.float64)[own]  # float64(float32 r) + float64(float32 margin)
    fam = s["family"][own]
    ex = s["extra"][fam]
    o = s["obj"]
    nA = len(o["type"])
    # ---- the objects' columns do not depend on the row chunk: (nS, nA) depth, threshold, band, allowed
    o_depth, o_scale = np.zeros((nS, nA)), np.zeros((nS, nA))
    for k in range(nA):
        d = (Gs - s["G"][o["owner"][k]][None, :]).astype(np.float64) * l + rel - o["rel"][k][None, :]   # sphere - object, metres
        n = o["dir"][k]
        Rk = R + float(s["margin"][o["owner"][k]])
        along = d @ n
        if o["type"][k] == 0:
            o_depth[:, k] = Rk - along
            o_scale[:, k] = R + np.abs(along)
        else:
            perp = d - along[:, None] * n[None, :]
            dr = np.sqrt((perp * perp).sum(1))
            o_depth[:, k] = Rk - o["sign"][k] * (o["size1"][k] - dr)
            o_scale[:, k] = R + o["size1"][k] + dr
    ofam = s["family"][o["owner"]] if nA else np.zeros(0, np.int64)
    o_thr = np.minimum(ex[:, None], s["extra"][ofam][None, :])
    o_ok = ~s["masked"][fam[:, None], ofam[None, :]]
    o_type = np.where(o["type"] == 0, PLANE, CYL)
    A, B, T = [], [], []
    grey = int((o_ok & (np.abs(o_depth - o_thr) <= BAND * o_scale)).sum())
    # lattice differences are whole numbers below 2^53: exact in float64
    X = [Gs[:, k].astype(np.float64) for k in range(3)]
    has_rel, has_fam = bool(rel.any()), bool(s["masked"].any() or ex.any())
    col = np.arange(nS)
    for i0 in range(0, nS, rows):
        i1 = min(nS, i0 + rows)
        hits = [np.zeros((i1 - i0, 0), bool)]
        for c0 in range(i0, nS, cols):                                        # only B > A: columns from the chunk's first row on
            c1 = min(nS, c0 + cols)
            d2 = None
            for k in range(3):
                d = np.subtract.outer(X[k][i0:i1], X[k][c0:c1])
                d *= l
                if has_rel:
                    d += np.subtract.outer(rel[i0:i1, k], rel[c0:c1, k])
                d *= d
                d2 = d if d2 is None else np.add(d2, d, out=d2)
            Rsum = np.add.outer(R[i0:i1], R[c0:c1])
            excess = np.subtract(Rsum, np.sqrt(d2, out=d2), out=d2)           # depth - threshold
            if has_fam:
                excess -= np.minimum.outer(ex[i0:i1], ex[c0:c1])
            hit = excess > -BAND * float(Rsum.max())                          # listed, or inside the band
            if hit.any():                                                     # (most blocks of a scene of isolated pairs have none)
                ok = np.not_equal.outer(own[i0:i1], own[c0:c1]) & np.less.outer(col[i0:i1], col[c0:c1])
                if has_fam:
                    ok &= ~s["masked"][fam[i0:i1, None], fam[None, c0:c1]]
                grey += int((ok & (np.abs(excess) <= BAND * Rsum)).sum())
                hit = ok & (excess > 0)
            hits.append(hit)
        hits.append(o_ok[i0:i1] & (o_depth[i0:i1] - o_thr[i0:i1] > 0))
        r, c = np.nonzero(np.concatenate(hits, 1))                            # row-major: by A, spheres before objects, by B
        is_obj = c >= nS - i0
        A.append(r + i0)
        B.append(np.where(is_obj, c - (nS - i0), c + i0))
        T.append(np.where(is_obj, o_type[np.where(is_obj, c - (nS - i0), 0)] if nA else 0, SS))
    cat = lambda x, dt: np.concatenate(x).astype(dt) if x else np.zeros(0, dt)
    return (cat(A, np.uint32), cat(B, np.uint32), cat(T, np.uint8)), grey


def history_map(prev, new):
    """row of every new (A, B, type) in the previous list, 0xFFFFFFFF where it is absent: a dict, as the definition reads"""
    where = {k: i for i, k in enumerate(zip(*(np.asarray(x).tolist() for x in prev[:3])))}
    return np.array([where.get(k, 0xFFFFFFFF) for k in zip(*(np.asarray(x).tolist() for x in new[:3]))], np.uint32).reshape(-1)
