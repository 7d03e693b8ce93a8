"""Which (sphere, triangle) pairs a detection must list, stated over ALL PAIRS in float64 (numpy): the sibling of tests/_detect64.py
for DESIGN section 0 row a7.  No bins and no sort: the definition of the sandwich, Ericson's closest point on a triangle (the float64
routine of tests/_contact_model64.py) and the directional test as the scheme defines it.  Nothing is taken from csrc/deme_mesh.h or
oracle/deme_oracle.cpp.

Inputs: the scene arrays as the engine receives them (codec lattice, component tables, triangle nodes as fp32 relative to the mesh
owner, the owners' quaternions), the per-owner margins of set_margins, the family masks and extra margins.

  T        the world triangle: owner's lattice point x l + rot(q) node, q the owner's fp32 quaternion in float64
  c        the sphere's centre: owner's lattice point x l + rot(q) offset
  R        float64(float32 r) + float64(float32 margin of the sphere's owner)
  mt       margin of the mesh owner;   e = min(extra of the sphere's family, extra of the mesh's family)
  A, B     T's sandwich triangles: every vertex moved away from the incenter by mt / sin(half the interior angle), then by +mt (A)
           or -mt (B) along the normal of T; B with reversed winding, so that its normal points away from T as A's does
  test(X)  the directional test of sphere (c, R) against triangle X with closest point q, region and height h over X's plane:
           depth = h - R over the face, |c - q| - R on an edge or vertex; passes iff -depth > e (and h < R off the face).  It has
           no far side: a sphere anywhere under the face of X passes
  cpA      the closest point of A to c

THREE VERDICTS -- a property of the scheme, not a weakness of the statement:
  MUST      not masked, test(A) or test(B) passes by more than `band`, and |c - cpA|_inf < R - band: the contact point lies inside
            the sphere's bounding box, so the sphere is registered in the contact point's bin WHATEVER the bins are (and so is the
            triangle: the point is one of A's).
  MUST-NOT  masked; or both tests fail by more than band; or |c_k - cpA_k| >= R + binSize + band on some axis k (no bin of the
            sphere can hold the contact point).
  MAY       the rest: "numerical" when moving every threshold by band settles it, "geometric" otherwise -- the column over and under
            a face beyond R, the back side beyond R - mt (the scheme snaps on A "as standard": below the face the contact point is
            |h| + mt away), where the listing depends on where the bin planes are.
  The issue stated MUST through the sufficient condition  mt < R - e  and  dist(c, T) < (R - e) + mt - mt^2 / (R - e) - band  in
  place of "test(A) or test(B) passes".  That leaves a gap of mt^2 / (R - e) under the exact sandwich boundary in which the designed
  pairs of the pair-geometry scene (threshold - 2 bands) would be MAY; the exact test in float64 is used instead (more pairs are MUST,
  none fewer), and `sufficient_implies_exact` checks the issue's inequality on every candidate pair of every scene.

BAND, per pair.  The engine rounds the sphere's centre and the six sandwich vertices to fp32 WORLD coordinates, rotates the local
nodes with fp32 coefficients, and normalises with an fp32 reciprocal root.  One fp32 unit is 2^-24 x scale with
scale = largest |world coordinate| of the pair + largest |local node coordinate| (the lever of the rotation) + R.  Roundings that
reach the depth: the centre (1), the world vertices of the triangle tested (3, of which the closest feature sees at most 2 on an
edge, 3 on the face), the rotation of the lever (2: coefficients and products), the in-plane enlargement through ev = unit(vertex -
incenter) (1), the reciprocal root and the dot product (1): 8 units.  The in-plane part of a vertex error is amplified where the
sphere sits on an edge next to a sharp vertex: the edge direction turns by (error) / (edge length), and the offset mt / sin(half
angle) along the bisector carries the cos_half error of sandwich_vertex with 1 / sin^2; both are bounded by the factor
amp = 1 / sin(half the smallest angle).  band = 8 x 2^-24 x scale x amp.  At 1 m and 40 degrees: 1.4e-6 m.
MEASURED on the CPU (test_band_measured): the largest |depth of orc.tri_sphere(directional) on the oracle's own fp32 sandwich -
float64 depth| over every designed pair, as a fraction of that pair's band; the band must be at least 4 x it (the factor the other
zoos give fp32 re-association over a measured yardstick).

The list comes out in the engine's canonical order: by sphere A, then class (sphere-sphere 0, sphere-mesh 1, sphere-analytical 2),
then B; a mesh row has type 2 and B = the triangle's id.
"""
import numpy as np

from tests import _contact_model64 as m64
from tests import _detect64 as d64

MESH = 2
BAND_UNITS = 8.0
MUST, MUST_NOT, MAY = 1, -1, 0


def _unit(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def inputs_of(arrays, p, margins, mask_pair, n_anal=None, state=None):
    """d64.inputs_of plus the triangles; sphere offsets rotated by their owner's quaternion (exact for the identity)"""
    a = dict(arrays)
    if state is not None:
        a.update(state)
    s = d64.inputs_of(a, p, margins, mask_pair, n_anal)
    Q = np.stack([np.asarray(a[k], np.float32).astype(np.float64) for k in ("oriQw", "oriQx", "oriQy", "oriQz")], 1)
    Rm = m64.rot_matrix(Q)
    s["sph_rel"] = np.einsum("nij,nj->ni", Rm[s["sph_owner"]], s["sph_rel"])
    nT = len(a["ownerMesh"]) if "ownerMesh" in a else 0
    own = np.asarray(a["ownerMesh"], np.int64) if nT else np.zeros(0, np.int64)
    loc = np.stack([np.asarray(a[k], np.float32).astype(np.float64).reshape(-1, 3) for k in ("triNode1", "triNode2", "triNode3")], 1) \
        if nT else np.zeros((0, 3, 3))
    T = s["G"][own].astype(np.float64)[:, None, :] * s["l"] + np.einsum("nij,nkj->nki", Rm[own], loc)
    s["tri"] = dict(owner=own, local=loc, T=T, mt=s["margin"].astype(np.float64)[own], fam=s["family"][own])
    s["bin"] = float(p.binSize)
    return s


def sandwich(T, mt):
    """A and B (n, 3, 3) of the triangles T (n, 3, 3) with margins mt (n)"""
    p1, p2, p3 = T[:, 0], T[:, 1], T[:, 2]
    ln = lambda v: np.sqrt((v * v).sum(1))  # noqa: E731
    a, b, c = ln(p2 - p3), ln(p1 - p3), ln(p1 - p2)
    inc = (a[:, None] * p1 + b[:, None] * p2 + c[:, None] * p3) / (a + b + c)[:, None]
    n = _unit(np.cross(p2 - p1, p3 - p1))
    out = []
    for v, u, w in ((p1, p2, p3), (p2, p3, p1), (p3, p1, p2)):
        cos_t = (_unit(u - v) * _unit(w - v)).sum(1)
        sin_half = np.sqrt(0.5 * (1.0 - cos_t))
        out.append(v + _unit(v - inc) * (mt / sin_half)[:, None])
    up = (mt[:, None] * n)
    A = np.stack([out[0] + up, out[1] + up, out[2] + up], 1)
    B = np.stack([out[0] - up, out[2] - up, out[1] - up], 1)
    return A, B


def smallest_angle(T):
    ang = []
    for i in range(3):
        v, u, w = T[:, i], T[:, (i + 1) % 3], T[:, (i + 2) % 3]
        ang.append(np.arccos(np.clip((_unit(u - v) * _unit(w - v)).sum(1), -1, 1)))
    return np.min(ang, 0)


def depth_of(X, c, R):
    """(depth of the directional test: h - R over the face, |c - q| - R off it; the closest point q, its region, the height h)"""
    q, region = m64.closest_point_on_triangle(X[:, 0], X[:, 1], X[:, 2], c)
    n = _unit(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]))
    h = ((c - X[:, 0]) * n).sum(1)
    dist = np.sqrt(((c - q) ** 2).sum(1))
    return np.where(region == 0, h, dist) - R, q, region, h


def directional(X, c, R, e):
    """(how far the directional test of spheres (c, R) against triangles X passes: > 0 passes, the closest point, its region, h)"""
    depth, q, region, h = depth_of(X, c, R)
    by = -depth - e
    by = np.where(region == 0, by, np.minimum(by, R - h))
    return by, q, region, h


def band_of(s, i_s, i_t, c, R):
    tr = s["tri"]
    coord = np.maximum(np.abs(c).max(1), np.abs(tr["T"][i_t]).max((1, 2)))
    lever = np.abs(tr["local"][i_t]).max((1, 2))
    amp = 1.0 / np.sin(0.5 * s["tri_angle"][i_t])
    return BAND_UNITS * 2.0 ** -24 * (coord + lever + R) * amp


def centres(s):
    own = s["sph_owner"]
    c = s["G"][own].astype(np.float64) * s["l"] + s["sph_rel"]
    R = s["sph_r"].astype(np.float64) + s["margin"].astype(np.float64)[own]
    return c, R


def pairs(s, rows=512):
    """every candidate (sphere, triangle) pair with its verdict; all other pairs are MUST-NOT by the third MUST-NOT rule (their
    distance to A exceeds sqrt(3) (R + binSize + band)).  Returns a dict of arrays over the candidates."""
    tr = s["tri"]
    nT = len(tr["owner"])
    c_all, R_all = centres(s)
    nS = len(R_all)
    if not nT or not nS:
        kinds = dict(i_s=np.int64, i_t=np.int64, verdict=np.int64, region=np.int64, numerical=bool, sufficient=bool)
        return {k: np.zeros((0, 3) if k in ("cpA", "c") else 0, kinds.get(k, np.float64))
                for k in ("i_s", "i_t", "verdict", "numerical", "region", "side", "by", "band", "box", "cpA", "sufficient", "R", "e", "c")}
    if "tri_angle" not in s:
        s["tri_angle"] = smallest_angle(tr["T"])
    A, B = sandwich(tr["T"], tr["mt"])
    cen = A.mean(1)
    rad = np.sqrt(((A - cen[:, None, :]) ** 2).sum(2)).max(1)
    band_max = BAND_UNITS * 2.0 ** -24 * 8.0 / np.sin(0.5 * s["tri_angle"].min())  # coordinates, levers and R are below 8 m together
    I, J = [], []
    for i0 in range(0, nS, rows):
        cc = c_all[i0:i0 + rows]
        d = np.sqrt(((cc[:, None, :] - cen[None, :, :]) ** 2).sum(2)) - rad[None, :]
        near = d < np.sqrt(3.0) * (R_all[i0:i0 + rows, None] + s["bin"] + band_max)
        i, j = np.nonzero(near)
        I.append(i + i0), J.append(j)
    i_s, i_t = np.concatenate(I), np.concatenate(J)
    c, R = c_all[i_s], R_all[i_s]
    famS, famT = s["family"][s["sph_owner"][i_s]], tr["fam"][i_t]
    e = np.minimum(s["extra"][famS], s["extra"][famT])
    masked = s["masked"][famS, famT] | (s["sph_owner"][i_s] == tr["owner"][i_t])
    band = band_of(s, i_s, i_t, c, R)
    byA, cpA, _, _ = directional(A[i_t], c, R, e)
    byB, _, _, _ = directional(B[i_t], c, R, e)
    by = np.maximum(byA, byB)
    box = np.abs(c - cpA).max(1)
    qT, region = m64.closest_point_on_triangle(tr["T"][i_t, 0], tr["T"][i_t, 1], tr["T"][i_t, 2], c)
    nT_ = _unit(np.cross(tr["T"][i_t, 1] - tr["T"][i_t, 0], tr["T"][i_t, 2] - tr["T"][i_t, 0]))
    side = ((c - tr["T"][i_t, 0]) * nT_).sum(1)
    distT = np.sqrt(((c - qT) ** 2).sum(1))

    def verdict(bd):
        must = ~masked & (by > bd) & (box < R - bd)
        never = masked | (by < -bd) | (box >= R + s["bin"] + bd)
        return must, never
    must, never = verdict(band)
    assert not (must & never).any()
    v = np.where(must, MUST, np.where(never, MUST_NOT, MAY))
    m2, n2 = verdict(-band)
    mt, Re = tr["mt"][i_t], R - e
    with np.errstate(divide="ignore", invalid="ignore"):
        sufficient = (mt < Re) & (distT < Re + mt - mt * mt / Re - band)
    return dict(i_s=i_s, i_t=i_t, verdict=v, numerical=(v == MAY) & (m2 | n2), region=region, side=side, by=by, band=band, box=box,
                cpA=cpA, sufficient=sufficient & ~masked, R=R, e=e, c=c)


def sufficient_implies_exact(pr):
    """the issue's sufficient condition for the directional test, checked against the exact one (see the module's text)"""
    return bool((pr["by"][pr["sufficient"]] > 0).all())


def merged(s, i_s, i_t):
    """the canonical list of the sphere-sphere and sphere-analytical rows of tests/_detect64.py and the given mesh rows; the grey count"""
    (a, b, t), grey = d64.expected(s)
    a = np.concatenate([a.astype(np.uint64), np.asarray(i_s).astype(np.uint64)])
    b = np.concatenate([b.astype(np.uint64), np.asarray(i_t).astype(np.uint64)])
    t = np.concatenate([t, np.full(len(i_s), MESH, np.uint8)])
    cls = np.where(t == d64.SS, 0, np.where(t == MESH, 1, 2)).astype(np.uint64)
    order = np.argsort((a << np.uint64(33)) | (cls << np.uint64(31)) | b, kind="stable")
    return (a[order].astype(np.uint32), b[order].astype(np.uint32), t[order]), grey


def expected(s, pr=None):
    """((A, B, type) of every contact that must be listed, canonical order), numerical MAY pairs (the grey band of the sphere rows
    included), geometric MAY pairs"""
    pr = pairs(s) if pr is None else pr
    m = pr["verdict"] == MUST
    want, grey = merged(s, pr["i_s"][m], pr["i_t"][m])
    n_num = int(pr["numerical"].sum())
    n_geo = int(((pr["verdict"] == MAY) & ~pr["numerical"]).sum())
    return want, grey + n_num, n_geo
