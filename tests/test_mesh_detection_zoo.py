"""The mesh detection zoo: sphere-triangle contact lists of DESIGNED scenes against the all-pairs float64 statement
(tests/_detect_mesh64.py) -- DESIGN section 0 row a7: k_tri_prep, k_tri_fill, k_tri_sweep, sandwich_vertex, tri_box_overlap,
detect_triangles.

The oracle's triangle code is "parity unpinned" (tests/test_mesh.py): the reference's kernels cannot be built on the host, and every
list comparison of the suite held the HIP kernels against a restatement of the same algorithm.  Here the expected list has no bins in
it, and the CPU tests of this file are the first independent check the oracle's triangle detection gets.  The machinery is that of
tests/test_detection_zoo.py: a 1 m box without walls, a bin of an odd whole number of lattice units, codec fields overwritten after
Initialize(), margins from set_margins, SetCDUpdateFreq(0); isolated triangles go in with one AddMeshObject per group.  Every
comparison is integer equality of (A, B, type); the MAY count of the statement is zero in every scene but scene C, so nothing is
excluded from a comparison.

SCENE W, the sweep's buffer and searches (k_tri_sweep).  One cluster per bin (c, 0, 0): K small triangles stacked 2^-22 m apart along
their normal (fp32 nodes cannot carry the one lattice unit the issue asked for), S spheres that each touch every one of them on the
normal side with the contact point in the bin: K S rows, each key once.  Rows (K, S): (1, 1), (63, 4), (64, 3), (64, 4), (64, 5),
(65, 4), (130, 9), (300, 1) -- the arithmetic by which (64, 3..5) reach 192 / 256 / a flush with a remainder stands above ROWS_W --,
clusters of unequal (K, S) in one wavefront, triangle-only bins below, between and above the sphere bins, two mesh owners, a mesh
and no sphere at all, a mesh wholly outside the domain (no incidence: the list is the sphere-sphere one).
SCENE R, registration (k_tri_prep, k_tri_fill, tri_bin_bounds, tri_box_overlap).  Triangles that carry spheres over their face, on
every edge and at every vertex (radii 0.2 and 0.8 bin): inside one bin; axis-aligned exactly in a bin plane (spheres on both sides);
slanted with sides of 3, 10 and 40 bins (apex 20 degrees; under a tenth of the 40-bin bounding boxes is registered); the smallest
angle at the zoo's limit of 15 degrees; in the first and in the last, partial bin of every axis; two nodes outside the domain; mesh
owners with random quaternions 0.5 m from their triangles and on a voxel edge (codec fields 65535 / 0); a two-component clump
with a rotated owner of which one component touches.
SCENE G, pair geometry (sandwich_vertex, tri_sphere_cd, the min of the extra margins, the masks).  The seven regions of a triangle
crossed with: normal side, back side, unequal margins in both orders, unequal extra margins, masked families -- 42 classes of 24
isolated pairs, 4 at each of threshold +-2, +-8, +-1000 bands, the threshold being where the better of the two directional tests
passes by nothing (found by bisection in float64 on the world triangles the kernels see).  Two findings of writing it down:
  over a FACE there is no threshold -- above A's reach the sphere is under B, whose test has no far side -- so all six steps of a face
  row are listed (the normals are oblique, which keeps the contact point inside the sphere's box); where a face pair stops being
  listed is a matter of the bins (scene C);
  behind a face likewise: those rows sit at fixed heights inside R - mt.
Built with the families (masked rows never listed) and without (they are listed, every threshold is that of e = 0).
SCENE C, the column: the only scene with MAY pairs -- see the text above C_HEIGHTS; it asserts the scheme's bin rule itself.
MIXED ROWS AND HISTORY: a sphere with a sphere partner, 70 triangles and a plane; two detections around upload_state and
update_tri_nodes, mesh rows appear, persist and vanish by either means; wildcards that encode the previous row, bit for bit after
migrate(); the map against the dict of tests/_detect64.py.
DRIVER: one context, three detections through detect_triangles' growth path and a repeat of detect_part1 -- the text above D_K.

GPU variants of W, R and G: caller order; engine order ON (fast arithmetic, scattered numbering of more than 256 clumps,
engine_order() asserted); the segmented key arena forced with DEME_KEY_SEG_MIN.  Before the first GPU run the two edge rows of scene
W were read through detect_part1: without a sphere detect_sphere_incidences launches nothing and detect_triangles returns at
`!d.P`; without an incidence k_tri_prep runs (one workgroup), the total is 0 and detect_triangles returns before k_tri_fill.  No
launch with zero workgroups.

MEASURED (CPU, test_band_measured): the oracle's fp32 directional depth on its own fp32 sandwich against the float64 depth, A and B
of every designed pair of scenes G and R (4214 depths): 2.0e-7 m at the most, 0.086 of the pair's band at the most (band = 8 fp32
units of coordinate + lever + R, times 1 / sin(half the smallest angle): 0.9e-6 .. 4e-6 m here); required: at most 1 / 4.
The oracle's detect() equals the statement on every scene (scene C: the bin rule) -- the first independent check of its triangle
code; no disagreement between statement, oracle and engine was met.  The one surprise of the design, that over a face the pair has
no MUST-NOT side, was read against the reference's own sweep (DEMContactKernels_SphereTriangle.cu: in_contact_A || in_contact_B, both
directional, then snap_to_face on A "as standard" and the bin of that point): the engine and the oracle do what it does.

MUTATIONS of csrc/deme_mesh_kernels.h and csrc/deme_mesh.h, each built and run ONCE on an MI355X through the 21 caller-order cases
of this file and the 14 GPU tests of tests/test_mesh.py (2) and tests/test_triangle_zoo.py (12), and not kept.  Each was read before
it ran: none changes an index into the wavefront buffer (at most 64 keys are added per iteration, as before), arena_store guards the
arena's end, k_segment_rank_sort places equal keys by position, the search bounds stay inside [0, P), k_tri_prep and k_tri_fill
share the changed predicates so their counts agree, and every loop keeps its bounds.
                                                                  fails here                                        of the older 14
  1 k_tri_sweep   hit = true (no contact-point-in-bin test)       G (both), R, C, mixed, driver: doubled keys; the    14
                                                                  W rows pass -- every cluster lies in one bin
  2 k_tri_sweep   snap on B instead of A                          C, and R through its "bin plane wide" rows          12
  3 k_tri_sweep   max of the two extra margins instead of min     G with the families                                 0
  4 k_tri_sweep   final flush only if nBuf > 64                   W: 1x1, 64x5, 65x4, 130x9, 300x1, tri-only bins,    14
                                                                  many clumps, 64x5 on two meshes (64x3, 64x4, 63x4
                                                                  pass: 192 and 252 are flushed, 256 inside the loop);
                                                                  G (both), R, C, mixed, driver
  5 k_tri_sweep   the upper search starts from b = P - 1          every W row (the last sphere of the last bin is     0
                                                                  lost), R, driver
  6 k_tri_prep    bin bounds from A only                          NONE, and none of the older 14: an equivalent       0
                                                                  mutant as far as lists go -- a key is emitted in the
                                                                  bin of a point of A, which is inside A's own
                                                                  bounds; the bins only B reaches can emit nothing
  7 sandwich_vertex  the in-plane enlargement dropped             G (both)                                            12
  8 tri_box_overlap  radius of the first edge axis halved         G (both), R, mixed                                  14
The unmutated library passes all 43 GPU cases of this file.
"""
import functools

import numpy as np
import pytest

from tests import _contact_model64 as m64
from tests import _detect64 as d64
from tests import _detect_mesh64 as dm
from tests.conftest import record_measured
from tests.test_detection_zoo import (NULL, Scene, _builder, _context, _pkg, _placeholder, _row_codes, _same_list)
from tests.test_triangle_zoo import _anchor, _fan, _frame, _unit

K6 = (2, -2, 8, -8, 1000, -1000)
BPW = 60.7  # bins per metre of the box: a bin of ~19.8 mm


# ------------------------------------------------------------------------------------------------------------ machinery
def _rand_q(pkg, rng):
    q = pkg.model.random_unit_quaternions(1, rng)[0]  # x y z w
    return np.array([q[3], q[0], q[1], q[2]], np.float32)


IDENT = np.array([1, 0, 0, 0], np.float32)


def _rot(q):
    return m64.rot_matrix(np.asarray(q, np.float32)[None, :].astype(np.float64))[0]


class Mesh:
    """a mesh owner: lattice point G, quaternion q (w x y z, fp32), family, margin, and its triangles as fp32 local nodes"""

    def __init__(self, G, l, q=IDENT, fam=0, margin=0.0):
        self.G, self.l, self.q, self.fam, self.margin = np.asarray(G, np.int64), l, np.asarray(q, np.float32), fam, margin
        self.R = _rot(self.q)
        self.tris = []

    def add(self, world):
        """a triangle given by world nodes (metres from the grid's corner); returns (index in the mesh, the world nodes in float64
        as the kernels will see them: owner + rot x the fp32 local nodes)"""
        loc = np.float32((np.asarray(world, np.float64) - self.G * self.l) @ self.R)  # R^T (W - X)
        self.tris.append(loc)
        return len(self.tris) - 1, self.G * self.l + loc.astype(np.float64) @ self.R.T


def _finish(pkg, b, G_clumps, margins_clumps, M, l, meshes, clump_q=None):
    """add the meshes, Initialize, write lattice points and quaternions of clumps and mesh owners into the arrays"""
    for me in meshes:
        nodes = np.array(me.tris, np.float32).reshape(-1, 3)
        mo = b.AddMeshObject(nodes, np.arange(len(nodes)).reshape(-1, 3), 0)
        mo.SetInitPos((0.5, 0.5, 0.5)), mo.SetMass(1.0), mo.SetMOI((1e-3, 1e-3, 1e-3)), mo.SetFamily(me.fam)
    p, _ = b.Initialize()
    assert p.l == l and abs(p.binSize - M * p.l) < 1e-18
    A = b.arrays
    n_clumps, n_own = int(b.counts["nOwnerClumps"]), int(b.counts["nOwners"])
    G_clumps = np.asarray(G_clumps, np.int64).reshape(-1, 3)
    assert len(G_clumps) == n_clumps
    first_mesh = n_own - len(meshes)
    idx = np.concatenate([np.arange(n_clumps), np.arange(first_mesh, n_own)]).astype(np.int64)
    G = np.concatenate([G_clumps, np.array([me.G for me in meshes], np.int64).reshape(-1, 3)])
    assert (G >= 0).all() and all((G[:, k] < (1 << (16 + (p.nvXp2, p.nvYp2, p.nvZp2)[k]))).all() for k in range(3))
    vox = G // 65536
    A["voxelID"][idx] = (vox[:, 0] + (vox[:, 1] << p.nvXp2) + (vox[:, 2] << (p.nvXp2 + p.nvYp2))).astype(np.uint64)
    for k, name in enumerate(("locX", "locY", "locZ")):
        A[name][idx] = (G[:, k] % 65536).astype(np.uint16)
    Q = np.array([IDENT] * n_clumps + [me.q for me in meshes], np.float32).reshape(-1, 4)
    if clump_q is not None:
        Q[:n_clumps] = clump_q
    for k, name in enumerate(("oriQw", "oriQx", "oriQy", "oriQz")):
        A[name][idx] = Q[:, k]
    z = Scene()
    z.builder, z.params, z.M, z.n_clumps = b, p, M, n_clumps
    z.scene = pkg.abi.make_scene_struct(A, b.counts)
    z.margins = np.zeros(n_own, np.float32)
    z.margins[:n_clumps] = margins_clumps
    z.margins[first_mesh:] = [me.margin for me in meshes]
    z.first_mesh = first_mesh
    z.tri_base = np.cumsum([0] + [len(me.tris) for me in meshes])[:-1]
    if meshes:
        assert np.array_equal(A["ownerMesh"], np.repeat(np.arange(first_mesh, n_own), [len(me.tris) for me in meshes]))
    return z


class Statement:
    pass


def _state(pkg, z, n_anal=None, state=None):
    st = Statement()
    st.inputs = dm.inputs_of(z.builder.arrays, z.params, z.margins, pkg.model.mask_pair, n_anal, state)
    st.pairs = dm.pairs(st.inputs)
    st.want, st.numerical, st.geometric = dm.expected(st.inputs, st.pairs)
    return st


def _verdict_of(st):
    return {(int(a), int(b)): int(v) for a, b, v in zip(st.pairs["i_s"], st.pairs["i_t"], st.pairs["verdict"])}


def _strictly_increasing(lst):
    a, b, t = (np.asarray(x).astype(np.uint64) for x in lst[:3])
    cls = np.where(t == 1, 0, np.where(t == 2, 1, 2)).astype(np.uint64)
    key = (a << np.uint64(33)) | (cls << np.uint64(31)) | b
    assert (key[1:] > key[:-1]).all()


# ------------------------------------------------------------------------------------------------------------ scene W
# (K, S) per cluster, one cluster per bin (c, 0, 0).  k_tri_sweep: the (bin, triangle) list is sorted by bin, then (the sort is
# stable and k_tri_fill writes triangle by triangle) by triangle id, so a single cluster of K triangles is entries 0 .. K - 1:
# wavefront w of workgroup g holds entries 256 g + 64 w .. + 63, and every lane's [lo, hi) is the S spheres of the bin.  In iteration
# i every lane with a triangle tests its i-th sphere and HITS (all S spheres touch all K triangles, contact point in the bin), so a
# full wavefront adds 64 keys to its 256-entry buffer per iteration and flushes when nBuf > 192:
#   (64, 3)  nBuf = 64, 128, 192: no flush inside the loop (192 > 192 is false), the final flush writes 192
#   (64, 4)  ... 192, then 256 = the last entry 255 written, flushed inside the loop, nothing left for the final flush
#   (64, 5)  ... 256 flushed, then 64: a flush and a remainder
#   (63, 4) / (65, 4)  one lane short of / one lane into the next wavefront (63 x 4 = 252: flushed at 252; the 65th triangle's
#            wavefront has one lane and never passes 4)
#   (130, 9) three wavefronts, 64 / 64 / 2 lanes, the full ones flush at 256 twice and end with 64;  (300, 1)  two workgroups
# The last rows: clusters with different (K, S) in one wavefront (lanes with different [lo, hi) lengths); triangle-only bins
# (S = 0: lo == hi) below the smallest sphere bin, between two sphere bins and above the largest; a scene of more than 256 clumps
# for the engine-order variant; a mesh and no sphere at all; a mesh wholly outside the domain.
ROWS_W = {
    "1x1": ((1, 1),), "63x4": ((63, 4),), "64x3": ((64, 3),), "64x4": ((64, 4),), "64x5": ((64, 5),), "65x4": ((65, 4),),
    "130x9": ((130, 9),), "300x1": ((300, 1),),
    "uneven": ((5, 3), (70, 2), (64, 6), (3, 9), (20, 1)),
    "tri-only bins": ((4, 0), (64, 4), (7, 0), (3, 2), (5, 0)),
    "many clumps": ((3, 40),) * 4 + ((66, 30),) * 4,
    "no sphere": ((3, 0),),
    "outside": ((0, 3), (0, 2)),
}
ROWS_W_TWO_MESHES = ("64x5", "uneven")
ROWS_W_REORDERED = ("many clumps",)
W_MT = 2e-4          # the mesh owner's margin
W_STACK = 2.0 ** -22  # metres between stacked triangles: the fp32 nodes cannot carry one lattice unit (9e-12 m); 300 of them 7e-5 m


@functools.lru_cache(maxsize=None)
def scene_w(row, meshes=1, numbering="cluster"):
    pkg = _pkg()
    rng = np.random.default_rng(6100 + len(row))
    b, M, l, _ = _builder(pkg, BPW)
    bin_m = M * l
    r = 0.2 * bin_m
    t = b.LoadSphereType(1e-3, r, 0)
    owners = [Mesh(np.rint(np.array([0.4, 0.3, 0.2]) / l), l, margin=W_MT), Mesh(np.rint(np.array([0.1, 0.6, 0.3]) / l), l, margin=W_MT)][:meshes]
    e1 = _unit(np.array([2.0, 1.0, 0.0]))  # an oblique frame: the stack's normal is along no axis
    n = _unit(np.cross(e1, np.array([-1.0, 2.0, 0.5])))
    e2 = np.cross(n, e1)
    G, cluster, tri_cluster = [], [], []
    for c, (K, S) in enumerate(ROWS_W[row]):
        centre = (np.array([c, 0, 0]) + 0.5) * bin_m
        for k in range(K):
            ang = 2 * np.pi * (np.arange(3) / 3.0) + 0.3 * c
            W = centre + 0.1 * bin_m * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2) + k * W_STACK * n
            me = owners[k % meshes]
            me.add(W)
            tri_cluster.append((k % meshes, c))
        off = np.zeros((0, 2), np.int64)
        while len(off) < S:  # distinct lattice offsets inside a disc of 0.02 bin: over the face of every triangle of the stack
            off = np.unique(np.concatenate([off, rng.integers(-int(0.012 * M), int(0.012 * M), (S - len(off), 2))]), axis=0)
        for o in off[rng.permutation(S)]:
            X = centre + (o[0] * e1 + o[1] * e2) * l + (0.5 * r + 300 * W_STACK) * n
            G.append(np.rint(X / l).astype(np.int64)), cluster.append(c)
    if row == "outside":  # two triangles wholly outside the grid (negative coordinates): no (bin, triangle) incidence
        for k in range(2):
            owners[0].add(np.array([[-0.05, 0.3, 0.3], [-0.04, 0.3, 0.3], [-0.05, 0.31, 0.3 + 0.01 * k]]))
    owners = [me for me in owners if me.tris]
    G, cluster = np.array(G, np.int64).reshape(-1, 3), np.array(cluster, np.int64)
    if numbering == "scattered":
        order = rng.permutation(len(G))
        G, cluster = G[order], cluster[order]
    if len(G):
        b.AddClumps(t, _placeholder(len(G)))
    z = _finish(pkg, b, G, np.zeros(len(G), np.float32), M, l, owners)
    z.cluster, z.row = cluster, ROWS_W[row]
    order = sorted(range(len(tri_cluster)), key=lambda i: tri_cluster[i][0])  # triangle ids: mesh by mesh
    z.tri_cluster = np.array([tri_cluster[i][1] for i in order], np.int64)
    return z


@functools.lru_cache(maxsize=None)
def statement_w(row, meshes=1, numbering="cluster"):
    return _state(_pkg(), scene_w(row, meshes, numbering))


# ------------------------------------------------------------------------------------------------------------ scene G
# conditions x regions; per (condition, region) 4 pairs at each of the six steps of the ladder (so every condition has 28 pairs at
# each step, where the issue asked for 16: seven regions x 96 pairs x 6 conditions would be 4000 spheres)
REGION7 = (0, 4, 5, 6, 1, 2, 3)  # face, edges ab ac bc, vertices a b c (the model's region codes)
CONDITIONS = ("normal", "back", "margin_s", "margin_t", "extra", "masked")
N_STEP = 4
G_EXTRA = {1: 3e-5, 2: 8e-5}
#                       sphere margin, mesh margin, sphere family, mesh family
G_COND = {"normal": [(5e-5, 5e-5, 0, 0)], "back": [(5e-5, 5e-5, 0, 0)], "margin_s": [(1.2e-4, 3e-5, 0, 0)], "margin_t": [(2e-5, 9e-5, 0, 0)],
          "extra": [(5e-5, 5e-5, 1, 2), (5e-5, 5e-5, 2, 1)], "masked": [(5e-5, 5e-5, 3, 4)]}
G_PITCH = 5


def _solve_ray(q, u, R, e, A, B, target, lo, hi, only_a):
    """s with by(q + s u) = target for each row, by bisection on [lo, hi] where by falls from above the target to below it.  by: how
    far the better of the two directional tests passes -- for the rows of `only_a` the test against A alone (over a face the test
    against B always passes: see scene_g)"""
    def f(s):
        c = q + s[:, None] * u
        by_a, by_b = dm.directional(A, c, R, e)[0], dm.directional(B, c, R, e)[0]
        return np.where(only_a, by_a, np.maximum(by_a, by_b)) - target
    lo, hi = np.full(len(q), lo), np.full(len(q), hi)
    assert (f(lo) > 0).all() and (f(hi) < 0).all()
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        up = f(mid) > 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def scene_g(families):
    pkg = _pkg()
    rng = np.random.default_rng(7117)
    b, M, l, nv = _builder(pkg, BPW)
    bin_m = M * l
    r0 = float(np.float32(0.3 * bin_m))
    t = b.LoadSphereType(1e-3, r0, 0)
    if families:
        for fam, ex in G_EXTRA.items():
            b.SetFamilyExtraMargin(fam, ex)
        b.DisableContactBetweenFamilies(3, 4)
    extra = {f: (float(np.float32(G_EXTRA.get(f, 0.0))) if families else 0.0) for f in range(5)}
    # one mesh owner per (mesh margin, mesh family) of the conditions; every second one rotated
    owners, owner_of = [], {}
    for cond, combos in G_COND.items():
        for (ms, mt, fs, ft) in combos:
            if (mt, ft) not in owner_of:
                pos = rng.uniform(0.2, 0.9, 3)
                owner_of[(mt, ft)] = len(owners)
                owners.append(Mesh(np.rint(pos / l), l, q=_rand_q(pkg, rng) if len(owners) % 2 else IDENT, fam=ft, margin=mt))
    cells = [(i, j, k) for i in range(1, 11) for j in range(1, 11) for k in range(1, 12)]
    cells = [cells[i] for i in rng.permutation(len(cells))]
    rows = []  # dict(cond, region, k, mesh, tri, W, q, u, ms, mt, fs, ft)
    for cond in CONDITIONS:
        for region in REGION7:
            for i in range(6 * N_STEP):
                ms, mt, fs, ft = G_COND[cond][i % len(G_COND[cond])]
                me = owners[owner_of[(mt, ft)]]
                centre = (np.array(cells.pop()) * G_PITCH + 0.5 + rng.uniform(-0.3, 0.3, 3)) * bin_m
                while True:
                    ti, W = me.add(centre + _fan(rng, 0.6 * bin_m) @ _frame(rng))
                    O, e_, m_, n_ = _anchor(region, W)
                    sgn = -1.0 if cond == "back" else 1.0
                    if region == 0:
                        w = 0.2 + 0.4 * rng.dirichlet(np.ones(3))
                        q, u = w @ W, sgn * n_
                    else:
                        th, phi = np.radians(rng.uniform(25, 65)), rng.uniform(-0.3, 0.3)
                        q = O + (rng.uniform(-0.2, 0.2) * 0.6 * bin_m * e_ if region >= 4 else 0.0)
                        u = sgn * np.cos(th) * n_ + np.sin(th) * _unit(m_ + (phi * e_ if region < 4 else 0.0))
                    # behind the triangle the scheme snaps on A, two margins further from the centre than B, which passes the test:
                    # the contact point stays inside the sphere's box (|c - cpA|_inf < R) for a direction away from the axes
                    # ... and over a FACE the directional test has no MUST-NOT side at all: above A's reach the sphere is "under" B, whose
                    # test has no far side, and the pair is listed as long as the contact point is inside the sphere's box -- which an
                    # oblique normal guarantees at every step of the ladder (|c - cpA|_inf <= 0.65 (R + 1000 bands) < R).  All six
                    # steps of a face row are MUST; where a face pair stops being listed is a matter of the bins: scene C
                    if (cond != "back" and region != 0) or np.abs(u).max() < (0.65 if region == 0 else 0.8):
                        break
                    me.tris.pop()
                rows.append(dict(cond=cond, region=region, k=K6[i % 6], mesh=owner_of[(mt, ft)], tri=ti, W=W, q=q, u=u, ms=ms, mt=mt, fs=fs, ft=ft))
    # ---- the spheres: on the ray q + s u where the better directional test passes by k bands (float64, on the world triangles
    # the kernels will see).  Behind a FACE there is no such threshold (the test has no far side): fixed heights inside R - mt
    Wt = np.array([r_["W"] for r_ in rows])
    mt_ = np.array([float(np.float32(r_["mt"])) for r_ in rows])
    A, B = dm.sandwich(Wt, mt_)
    R = np.array([r0 + float(np.float32(r_["ms"])) for r_ in rows])
    e = np.array([min(extra[r_["fs"]], extra[r_["ft"]]) for r_ in rows])
    q, u = np.array([r_["q"] for r_ in rows]), np.array([r_["u"] for r_ in rows])
    k = np.array([r_["k"] for r_ in rows], np.float64)
    owner_pos = np.array([owners[r_["mesh"]].G * l for r_ in rows])
    lever = np.abs(Wt - owner_pos[:, None, :]).max((1, 2)) * np.sqrt(3.0)  # (bounds the largest local coordinate of a rotated owner)
    band = dm.BAND_UNITS * 2.0 ** -24 * (np.abs(Wt).max((1, 2)) + r0 + lever + R) / np.sin(0.5 * dm.smallest_angle(Wt))
    back_face = np.array([r_["cond"] == "back" and r_["region"] == 0 for r_ in rows])
    frac = np.array([(0.15, 0.3, 0.45, 0.6, 0.75, 0.9)[i % 6] for i in range(len(rows))])
    s = frac * (R - mt_ - 1000 * band)
    j = np.nonzero(~back_face)[0]
    face = np.array([r_["region"] == 0 for r_ in rows])
    s[j] = _solve_ray(q[j], u[j], R[j], e[j], A[j], B[j], (k * band)[j], 0.3 * r0, 3.0 * r0, face[j])
    c = q + s[:, None] * u
    G = np.rint(c / l).astype(np.int64)
    order = rng.permutation(len(rows))  # numbering: a permutation of the scene
    batch = b.AddClumps(t, _placeholder(len(rows)))
    batch.SetFamily(np.array([rows[i]["fs"] for i in order], np.uint8))
    z = _finish(pkg, b, G[order], np.array([rows[i]["ms"] for i in order], np.float32), M, l, owners)
    z.rows = [dict(rows[i], sphere=n_, tri_id=int(z.tri_base[rows[i]["mesh"]] + rows[i]["tri"]), band=float(band[i])) for n_, i in enumerate(order)]
    z.families = families
    return z


def _g_listed(row, families):
    if row["cond"] == "masked" and families:
        return False
    return row["k"] > 0 or row["region"] == 0


@functools.lru_cache(maxsize=None)
def statement_g(families):
    return _state(_pkg(), scene_g(families))


# ------------------------------------------------------------------------------------------------------------ CPU tests
def _oracle_run(pkg, orc, z):
    sim = orc.make_sim(pkg, z.params, z.scene)
    sim.set_margins(z.margins)
    sim.detect()
    out = sim.contacts(), sim.tri_incidence(), sim.tri_sandwich(), sim.sphere_geometry()
    sim.close()
    return out


_SCENES = {"w": scene_w, "g": scene_g}
_oracle_cached = functools.lru_cache(maxsize=None)(lambda kind, *key: _oracle_run(_pkg(), __import__("__graft_entry__").load_oracle(),
                                                                                  _SCENES[kind](*key)))
W_CASES = [(r, 1, "cluster") for r in ROWS_W] + [(r, 2, "cluster") for r in ROWS_W_TWO_MESHES] + [(r, 1, "scattered") for r in ROWS_W_REORDERED]


def _w_id(x):
    return x if isinstance(x, str) else str(x)


@pytest.mark.parametrize("row,meshes,numbering", W_CASES, ids=_w_id)
def test_sweep_rows_design(pkg, orc, row, meshes, numbering):
    """no MAY pair; K S mesh rows per cluster, each key once; every triangle registered in its cluster's bin alone (the oracle's
    incidence list: entries c's start is the running sum of K); the oracle's list is the statement's"""
    z = scene_w(row, meshes, numbering)
    st = statement_w(row, meshes, numbering)
    assert (st.numerical, st.geometric) == (0, 0)
    assert dm.sufficient_implies_exact(st.pairs)
    a, b_, t = st.want
    mesh = t == 2
    assert int(mesh.sum()) == sum(K * S for K, S in z.row)
    assert int((t == 1).sum()) == sum(S * (S - 1) // 2 for K, S in z.row)
    assert (z.cluster[a[mesh]] == z.tri_cluster[b_[mesh]]).all()
    _strictly_increasing(st.want)
    got, (tb, tt), _, _ = _oracle_cached("w", row, meshes, numbering)
    assert len(tb) == sum(K for K, S in z.row)
    assert np.array_equal(tb, z.tri_cluster[tt]) and (np.diff(tb.astype(np.int64)) >= 0).all()
    _same_list(got, st.want)
    _strictly_increasing(got)


@pytest.mark.parametrize("families", [True, False], ids=["families", "trivial"])
def test_pair_geometry_design(pkg, orc, families):
    """no MAY pair; every designed pair has its designed verdict (MUST inside the threshold, MUST-NOT outside and when masked), its
    region of the triangle and its side; the statement lists the designed pairs and nothing else; the oracle's list is the
    statement's"""
    z = scene_g(families)
    st = statement_g(families)
    assert (st.numerical, st.geometric) == (0, 0)
    assert dm.sufficient_implies_exact(st.pairs)
    verdict = _verdict_of(st)
    at = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(st.pairs["i_s"], st.pairs["i_t"]))}
    for r_ in z.rows:
        key = (r_["sphere"], r_["tri_id"])
        assert verdict[key] == (dm.MUST if _g_listed(r_, families) else dm.MUST_NOT), r_
        i = at[key]
        assert int(st.pairs["region"][i]) == r_["region"], r_
        assert (st.pairs["side"][i] < 0) == (r_["cond"] == "back"), r_
    a, b_, t = st.want
    assert (t == 2).all()
    assert set(zip(a.tolist(), b_.tolist())) == {(r_["sphere"], r_["tri_id"]) for r_ in z.rows if _g_listed(r_, families)}
    for cond in CONDITIONS:
        for region in REGION7:
            ks = sorted(r_["k"] for r_ in z.rows if r_["cond"] == cond and r_["region"] == region)
            assert ks == sorted(K6 * N_STEP)
    A = z.builder.arrays
    assert (A["familyMasks"] != 0).any() == families and (A["familyExtraMarginSize"] != 0).any() == families
    got, _, _, _ = _oracle_cached("g", families)
    _same_list(got, st.want)
    _strictly_increasing(got)


# ------------------------------------------------------------------------------------------------------------ GPU tests
VARIANTS = ("caller order", "engine order", "segmented arena")


def _check_detection(ctx, z, st, oracle):
    ctx.set_margins(z.margins)
    ctx.detect()
    got = ctx.contacts()
    _same_list(got, st.want)
    _same_list(got, oracle[0])
    _strictly_increasing(got)
    assert int(ctx.counts().nContacts) == len(st.want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("variant,row,meshes", [(v, r, m) for v in VARIANTS for (r, m, _) in W_CASES[:len(ROWS_W) + len(ROWS_W_TWO_MESHES)]
                                                if v != "engine order" or r in ROWS_W_REORDERED], ids=_w_id)
def test_sweep_rows(pkg, orc, monkeypatch, variant, row, meshes):
    numbering = "scattered" if variant == "engine order" else "cluster"
    z = scene_w(row, meshes, numbering)
    ctx = _context(pkg, z, variant, monkeypatch)
    _check_detection(ctx, z, statement_w(row, meshes, numbering), _oracle_cached("w", row, meshes, numbering))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("families", [True, False], ids=["families", "trivial"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_pair_geometry(pkg, orc, monkeypatch, variant, families):
    z = scene_g(families)
    ctx = _context(pkg, z, variant, monkeypatch)
    _check_detection(ctx, z, statement_g(families), _oracle_cached("g", families))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ scene R
R_MT = 1e-4
R_ANGLE_MIN = 15.0  # degrees: the zoo's lower limit of a triangle's smallest angle


def _decorate(rng, W, radius, faces, feature_reach=0.6, back=(), features=True):
    """sphere centres on one triangle: `faces` points over the face (barycentric weights), one on each edge, one at each vertex, at
    0.6 R from their closest point; `back`: face points with the sphere 0.5 R BEHIND the triangle.  Returns [(centre, region)]"""
    out = []
    n = _anchor(0, W)[3]
    for w in faces:
        out.append((np.asarray(w) @ W + feature_reach * radius * n, 0))
    for w in back:
        out.append((np.asarray(w) @ W - 0.5 * radius * n, 0))
    for region in (4, 5, 6, 1, 2, 3) if features else ():
        O, e_, m_, n_ = _anchor(region, W)
        th = np.radians(rng.uniform(30, 60))
        out.append((O + feature_reach * radius * (np.cos(th) * n_ + np.sin(th) * m_), region))
    return out


def _iso(P0, d1, d2, L, apex_deg):
    a = np.radians(apex_deg)
    return np.array([P0, P0 + L * d1, P0 + L * (np.cos(a) * d1 + np.sin(a) * d2)])


@functools.lru_cache(maxsize=None)
def scene_r():
    pkg = _pkg()
    rng = np.random.default_rng(8123)
    b, M, l, nv = _builder(pkg, BPW)
    bin_m = M * l
    r_small, r_big = float(np.float32(0.2 * bin_m)), float(np.float32(0.8 * bin_m))
    tmpl = [b.LoadSphereType(1e-3, r_small, 0), b.LoadSphereType(1e-3, r_big, 0),
            b.LoadClumpType(2e-3, (1e-9, 1e-9, 1e-9), [r_small, r_small], [[0.4 * bin_m, 0, 0], [-0.4 * bin_m, 0, 0]], 0)]
    last = [(1 << (16 + nv[k])) // M for k in range(3)]
    world = [(1 << (16 + nv[k])) * l for k in range(3)]
    assert all(0.3 * bin_m < world[k] - last[k] * bin_m < bin_m for k in range(3))  # the last bin of every axis is partial
    voxel_edge = np.array([20 * 65536 * 1024 + 65535, 31 * 65536 * 1024, 17 * 65536 * 1024 + 65535], np.int64)  # codec fields 65535 / 0
    owners = [Mesh(np.rint(np.array([0.6, 0.6, 0.6]) / l), l, margin=R_MT),                           # identity, up to 0.8 m away
              Mesh(np.rint(np.array([0.3, 0.8, 0.5]) / l), l, q=_rand_q(pkg, rng), margin=R_MT),      # rotated, 0.5 m from its triangles
              Mesh(voxel_edge, l, q=_rand_q(pkg, rng), margin=R_MT)]                                  # rotated, on a voxel edge
    assert all(voxel_edge % 65536 == (65535, 0, 65535))
    spheres, design = [], []  # spheres: (tmpl, centre, quaternion); design: (sphere, mesh, tri, region, label)

    def put(label, mi, world_nodes, radius_t, faces, back=(), features=True):
        ti, W = owners[mi].add(world_nodes)
        for c, region in _decorate(rng, W, (r_small, r_big)[radius_t], faces, back=back, features=features):
            spheres.append((radius_t, c, IDENT))
            design.append((len(spheres) - 1, mi, ti, region, label))
        return W

    mid = [(1 / 3, 1 / 3, 1 / 3)]
    spread = [(0.6, 0.2, 0.2), (0.2, 0.6, 0.2), (0.2, 0.2, 0.6), (0.34, 0.33, 0.33), (0.45, 0.45, 0.1)]
    d1 = _unit(np.array([1.0, 0.8, 0.6]))
    d2 = _unit(np.cross(d1, np.array([0.0, 0.0, 1.0])))
    # a triangle inside one bin
    put("one bin", 0, (np.array([8, 8, 8]) + 0.5) * bin_m + 0.3 * bin_m * _fan(rng, 1.0) @ _frame(rng), 0, mid)
    # axis-aligned, lying exactly in the bin plane z = 12 bins (the owner sits on that plane, identity quaternion, local z = 0):
    # spheres over it and behind it; the contact point (on A, one margin over the plane) is in bin 12 for both
    plane_owner = Mesh(np.array([int(0.5 / l), int(0.5 / l), 12 * M], np.int64), l, margin=R_MT)
    owners.append(plane_owner)
    ti, W = plane_owner.add(np.array([[14.2 * bin_m, 14.3 * bin_m, 12 * M * l], [16.9 * bin_m, 14.6 * bin_m, 12 * M * l],
                                      [15.1 * bin_m, 17.2 * bin_m, 12 * M * l]]))
    assert (W[:, 2] == 12 * M * l).all()
    for c, region in _decorate(rng, W, r_small, spread[:3], back=spread[3:]):
        spheres.append((0, c, IDENT)), design.append((len(spheres) - 1, 3, ti, region, "bin plane"))
    # ... and one with a margin of 0.05 bin in the plane z = 30 bins, its spheres half a margin beyond R over the face: inside the
    # reach R + mt of a contact, their boxes wholly above the plane.  The contact point on A is in bin 30 with them; the point on B
    # would be in bin 29, where these spheres are not registered (the scheme snaps on A: a mutant that snaps on B loses the rows)
    wide = float(np.float32(0.05 * bin_m))
    wide_owner = Mesh(np.array([int(0.7 / l), int(0.4 / l), 30 * M], np.int64), l, margin=wide)
    owners.append(wide_owner)
    ti, W = wide_owner.add(np.array([[34.2 * bin_m, 14.3 * bin_m, 30 * M * l], [36.9 * bin_m, 14.6 * bin_m, 30 * M * l],
                                     [35.1 * bin_m, 17.2 * bin_m, 30 * M * l]]))
    assert (W[:, 2] == 30 * M * l).all()
    for w in spread[:3]:
        spheres.append((0, np.asarray(w) @ W + np.array([0, 0, r_small + 0.5 * wide]), IDENT))
        design.append((len(spheres) - 1, 4, ti, 0, "bin plane wide"))
    # slanted triangles of 3, 10 and 40 bins along their longest sides, apex 20 degrees: most of the bounding box is not registered
    put("span 3", 1, _iso(np.array([20.3, 6.2, 6.4]) * bin_m, d1, d2, 3 * bin_m, 20.0), 0, spread)
    put("span 10", 0, _iso(np.array([30.3, 6.2, 20.4]) * bin_m, d1, d2, 10 * bin_m, 20.0), 1, spread)
    put("span 40", 1, _iso(np.array([6.3, 20.2, 25.4]) * bin_m, d1, d2, 40 * bin_m, 20.0), 1, spread + [(0.05, 0.5, 0.45), (0.8, 0.1, 0.1)])
    put("span 40 small", 2, _iso(np.array([8.3, 52.2, 45.4]) * bin_m, d2, d1, 40 * bin_m, 20.0), 0, spread + [(0.05, 0.5, 0.45), (0.8, 0.1, 0.1)])
    # the smallest angle at the zoo's lower limit
    put("15 degrees", 2, _iso(np.array([44.3, 40.2, 10.4]) * bin_m, d1, d2, 3 * bin_m, R_ANGLE_MIN), 0, mid)
    # the first bin and the last, partial bin of every axis: a triangle of 0.1 bin at 0.35 bin from the domain's face, in a plane that
    # holds the axis, two spheres over its face (they and their boxes stay inside the domain and the bin)
    for ax in range(3):
        for end in ("first", "last"):
            centre = (np.array([25.5, 25.5, 25.5]) + 3 * ax) * bin_m
            centre[ax] = 0.35 * bin_m if end == "first" else (last[ax] + 0.35) * bin_m
            ang = 2 * np.pi * np.arange(3) / 3.0 + 0.4
            W0 = centre + 0.1 * bin_m * (np.cos(ang)[:, None] * np.eye(3)[ax] + np.sin(ang)[:, None] * np.eye(3)[(ax + 1) % 3])
            W = put(f"{end} {'xyz'[ax]}", 0, W0, 0, [(0.4, 0.3, 0.3), (0.3, 0.3, 0.4)], features=False)
            assert ((W[:, ax] // bin_m).astype(int) == (0 if end == "first" else last[ax])).all()
    # two nodes outside the domain (negative x), spheres on the part inside
    put("nodes outside", 0, np.array([[-2.1, 40.3, 30.2], [-1.4, 43.1, 31.0], [4.2, 41.0, 30.6]]) * bin_m, 0,
        [(0.1, 0.1, 0.8), (0.15, 0.25, 0.6)])
    design = [d for d in design if not (d[4] == "nodes outside" and spheres[d[0]][1][0] < r_small)]  # (keep the spheres inside)
    keep = sorted({d[0] for d in design})
    # 180 small spheres that touch nothing, in the empty upper half of the box: with them the scene has more than 256 clumps, which
    # is what the engine reorders
    for i in range(180):
        spheres.append((0, (np.array([10 + 7 * (i % 6), 10 + 7 * ((i // 6) % 6), 70 + 7 * (i // 36)]) + 0.4) * bin_m, IDENT))
        keep.append(len(spheres) - 1)
    # a two-component clump with a rotated owner: one component over the face of its own triangle, the other 0.8 bin away
    ti, W = owners[1].add((np.array([50, 50, 50]) + 0.5) * bin_m + 0.45 * bin_m * _fan(rng, 1.0) @ _frame(rng))
    qc = _rand_q(pkg, rng)
    arm = _rot(qc) @ np.array([float(np.float32(0.4 * bin_m)), 0.0, 0.0])
    n_ = _anchor(0, W)[3]
    centre = W.mean(0) + 0.6 * r_small * n_ - arm  # component 0 = centre + arm
    # ---- numbering: the kept spheres in a random order, the clump somewhere among them
    order = [keep[i] for i in rng.permutation(len(keep))]
    at = len(order) // 2
    types = [tmpl[spheres[i][0]] for i in order]
    types.insert(at, tmpl[2])
    G = [np.rint(spheres[i][1] / l).astype(np.int64) for i in order]
    G.insert(at, np.rint(centre / l).astype(np.int64))
    Q = np.array([IDENT] * len(G), np.float32)
    Q[at] = qc
    b.AddClumps(types, _placeholder(len(G)))
    z = _finish(pkg, b, np.array(G), np.zeros(len(G), np.float32), M, l, owners, clump_q=Q)
    sphere_of = {}  # designed sphere -> sphere id: clumps before `at` have one sphere each, the clump has two
    for pos, i in enumerate(order):
        sphere_of[i] = pos if pos < at else pos + 2
    z.design = [(sphere_of[s], int(z.tri_base[mi] + ti_), region, label) for (s, mi, ti_, region, label) in design if s in sphere_of]
    z.design.append((at, int(z.tri_base[1] + ti), 0, "clump"))
    z.clump_spheres = (at, at + 1)
    z.bin_m = bin_m
    return z


@functools.lru_cache(maxsize=None)
def statement_r():
    return _state(_pkg(), scene_r())


# ------------------------------------------------------------------------------------------------------------ scene C
# The column over and under a face, and the back side beyond R - mt: the pairs whose listing depends on where the bin planes are.
# The triangles are axis-aligned right triangles (normal +z, legs 2^-5 m, the owner at vertex A with the identity quaternion, so the
# world nodes are exact); the sandwich triangle A lies one margin above.  The scheme lists a pair that passes a directional test iff
# the bin of its contact point -- the projection of the centre onto A -- is one of the sphere's bins, i.e. (x and y of the projection
# are the centre's) iff  floor((z0 + mt) / bin)  lies in  [floor((cz - R) / bin), floor((cz + R) / bin)].
#   column     z0 at mid-bin; spheres at heights 0.5, 0.7, 0.76 bins over and under the face (beyond the reach R + mt of a contact:
#              listed all the same, the bin of the contact point is the sphere's lowest / highest) and at 0.84, 1.0, 1.25 (not listed)
#   back side  R = 0.6 bin, mt = 0.3 bin, the sphere R - mt / 2 behind the face: the test against B passes, the contact point on A is
#              R + mt / 2 from the centre.  Triangle at mid-bin: listed.  Triangle 0.225 bin under a bin plane (the plane half way
#              between the top of the sphere's box and A): NOT listed -- a sphere behind a triangle, beyond R - mt, is listed only
#              when the bins allow it, and the statement calls such a pair MAY.
# Every bin plane is at least 1000 bands from c +- R and from the projection (asserted), so the rule is decided in float64.
C_HEIGHTS = (0.5, 0.7, 0.76, 0.84, 1.0, 1.25)
C_LEG = 2.0 ** -5


@functools.lru_cache(maxsize=None)
def scene_c():
    pkg = _pkg()
    b, M, l, nv = _builder(pkg, BPW)
    bin_m = M * l
    r_col, r_back = float(np.float32(0.3 * bin_m)), float(np.float32(0.6 * bin_m))
    tmpl = [b.LoadSphereType(1e-3, r_col, 0), b.LoadSphereType(1e-3, r_back, 0)]
    mt_col, mt_back = 1e-4, float(np.float32(0.3 * bin_m))
    owners, G, types, design = [], [], [], []  # design: (sphere, triangle, listed by the rule)
    local = np.array([[0, 0, 0], [C_LEG, 0, 0], [0, C_LEG, 0]], np.float64)

    def tri_at(x_bins, y_bins, z_lattice, mt):
        me = Mesh(np.array([int(x_bins * M), int(y_bins * M), int(z_lattice)], np.int64), l, margin=mt)
        _, W = me.add(me.G * l + local)
        assert (W[:, 2] == me.G[2] * l).all()
        owners.append(me)
        return len(owners) - 1, W

    for col in range(4):
        ti, W = tri_at(10 + 6 * col, 10.2, (20 + col) * M + M // 2, mt_col)
        for side in (1.0, -1.0):
            for j, h in enumerate(C_HEIGHTS):
                c = W[0] + np.array([0.2 + 0.1 * (j % 3), 0.2 + 0.1 * (j // 3), 0.0]) * C_LEG + np.array([0, 0, side * h * bin_m])
                G.append(np.rint(c / l).astype(np.int64)), types.append(tmpl[0])
                design.append((len(G) - 1, ti, h < 0.8))
    for k, (z_frac, listed) in enumerate(((0.5, True), (1.0 - 0.225, False))):
        ti, W = tri_at(40.1, 10.3 + 6 * k, 30 * M + int(z_frac * M), mt_back)
        c = W[0] + np.array([0.3, 0.3, 0.0]) * C_LEG - np.array([0, 0, r_back - 0.5 * mt_back])
        G.append(np.rint(c / l).astype(np.int64)), types.append(tmpl[1])
        design.append((len(G) - 1, ti, listed))
    b.AddClumps(types, _placeholder(len(G)))
    z = _finish(pkg, b, np.array(G), np.zeros(len(G), np.float32), M, l, owners)
    z.design, z.bin_m = design, bin_m
    return z


@functools.lru_cache(maxsize=None)
def statement_c():
    return _state(_pkg(), scene_c())


def lattice_rule(z, st):
    """the scheme's rule on scene C, for every candidate pair: listed iff a directional test passes (by 1000 bands) and the bin of
    the projection onto A is one of the sphere's bins; every bin plane 1000 bands away from what the rule compares"""
    pr = st.pairs
    passes = pr["by"] > 0
    assert (np.abs(pr["by"]) > 1000 * pr["band"]).all()
    lo, hi, at = (pr["c"] - pr["R"][:, None]) / z.bin_m, (pr["c"] + pr["R"][:, None]) / z.bin_m, pr["cpA"] / z.bin_m
    assert np.abs(pr["cpA"][:, :2] - pr["c"][:, :2]).max() < 1e-12  # over the face: x and y of the projection are the centre's
    for x in (lo, hi, at):
        assert (np.abs(x[:, 2] - np.rint(x[:, 2])) * z.bin_m > 1000 * pr["band"]).all()
    inside = ((np.floor(at) >= np.floor(lo)) & (np.floor(at) <= np.floor(hi))).all(1)
    keep = passes & inside
    want, grey = dm.merged(st.inputs, pr["i_s"][keep], pr["i_t"][keep])  # (with the sphere-sphere rows of the columns' neighbours)
    assert grey == 0
    return want, keep


# ------------------------------------------------------------------------------------------------------------ mixed rows, history
# Sphere 0 has a sphere partner, 70 triangles and a plane: its segment of k_segment_rank_sort holds all three classes.  Around it,
# forty isolated triangles with one sphere each in five groups, two detections with upload_state AND update_tri_nodes between them:
#   persist          touching in both states
#   sphere comes / goes     the sphere starts / ends three bins to the side, in the triangle's plane (not over its face)
#   triangle comes / goes   the triangle does, through update_tri_nodes
H_GROUPS = ("persist", "sphere comes", "sphere goes", "triangle comes", "triangle goes")
H_PER_GROUP = 8
H_K = 70


@functools.lru_cache(maxsize=None)
def scene_m():
    pkg = _pkg()
    rng = np.random.default_rng(9001)
    lbf = -0.1
    plane_user_z = 0.35

    def start():
        b, M, l, _ = _builder(pkg, BPW)
        t = b.LoadSphereType(1e-3, float(np.float32(0.3 * M * l)), 0)
        b.AddBCPlane((0.5, 0.5, plane_user_z + lbf), (0, 0, 1), 0)
        return b, M, l, t
    probe, M, l, t = start()
    probe.AddClumps(t, _placeholder(1))
    pp, _ = probe.Initialize()
    A = probe.arrays
    pz = float(d64.lattice_of(A, pp)[int(A["objOwner"][0])][2]) * l + float(np.float32(A["objRelPosZ"][0]))  # the plane, metres from the corner
    b, M, l, t = start()
    bin_m = M * l
    r = float(np.float32(0.3 * bin_m))
    me = Mesh(np.rint(np.array([0.5, 0.5, 0.5]) / l), l, margin=W_MT)
    c0 = np.array([30.4 * bin_m, 30.6 * bin_m, pz + 0.7 * r])
    now, new = [c0, c0 + np.array([1.5 * r, 0, 0])], [c0, c0 + np.array([1.5 * r, 0, 0])]
    ang = 2 * np.pi * np.arange(3) / 3.0
    for k in range(H_K):  # normal -z (towards the spheres): clockwise seen from above
        me.add(c0 + np.array([0, 0, 0.6 * r + k * W_STACK]) + 1.2 * bin_m * np.stack([np.cos(-ang), np.sin(-ang), 0 * ang], 1))
    moved = []  # (triangle, local nodes in the new state)
    design = {"now": [], "new": []}
    for g, group in enumerate(H_GROUPS):
        for i in range(H_PER_GROUP):
            centre = (np.array([8 + 6 * i, 8 + 6 * g, 40]) + 0.5 + rng.uniform(-0.2, 0.2, 3)) * bin_m
            F = _frame(rng)
            W0 = centre + _fan(rng, 0.5 * bin_m) @ F
            aside = 3.0 * bin_m * F[0]
            here = group in ("persist", "sphere comes", "sphere goes", "triangle goes")
            ti, W = me.add(W0 if here else W0 + aside)
            touch = W0.mean(0) + 0.6 * r * F[2]
            now.append(touch + aside if group == "sphere comes" else touch)
            new.append(touch + aside if group == "sphere goes" else touch)
            if group.startswith("triangle"):
                target = W0 + aside if here else W0
                moved.append((ti, np.float32((target - me.G * l) @ me.R)))
            s = len(now) - 1
            if group in ("persist", "sphere goes", "triangle goes"):
                design["now"].append((s, ti))
            if group in ("persist", "sphere comes", "triangle comes"):
                design["new"].append((s, ti))
    b.AddClumps(t, _placeholder(len(now)))
    z = _finish(pkg, b, np.rint(np.array(now) / l).astype(np.int64), np.zeros(len(now), np.float32), M, l, [me])
    p, A = z.params, b.arrays
    z.new_state = {k: np.array(A[k], copy=True) for k in
                   ("voxelID", "locX", "locY", "locZ", "oriQw", "oriQx", "oriQy", "oriQz", "vX", "vY", "vZ", "omgBarX", "omgBarY", "omgBarZ")}
    Gn = np.rint(np.array(new) / l).astype(np.int64)
    vox = Gn // 65536
    z.new_state["voxelID"][:len(Gn)] = (vox[:, 0] + (vox[:, 1] << p.nvXp2) + (vox[:, 2] << (p.nvXp2 + p.nvYp2))).astype(np.uint64)
    for k, name in enumerate(("locX", "locY", "locZ")):
        z.new_state[name][:len(Gn)] = (Gn[:, k] % 65536).astype(np.uint16)
    nodes = [np.array(A[k], np.float32).reshape(-1, 3).copy() for k in ("triNode1", "triNode2", "triNode3")]
    for ti, loc in moved:
        for k in range(3):
            nodes[k][ti] = loc[k]
    z.new_nodes = nodes
    z.design, z.n_wild = design, 4
    return z


@functools.lru_cache(maxsize=None)
def statement_m(which):
    z = scene_m()
    if which == "now":
        return _state(_pkg(), z)
    state = dict(z.new_state, triNode1=z.new_nodes[0].reshape(-1), triNode2=z.new_nodes[1].reshape(-1), triNode3=z.new_nodes[2].reshape(-1))
    return _state(_pkg(), z, state=state)


def _run_mixed_history(z, side):
    side.set_margins(z.margins)
    side.detect()
    side.migrate()
    prev = side.contacts()
    for w in range(z.n_wild):
        side.set_wildcard(w, _row_codes(len(prev[0]), w))
    side.upload_state(z.new_state)
    side.update_tri_nodes(*z.new_nodes)
    side.detect()
    new = side.contacts()
    side.migrate()
    return prev, new, [side.wildcard(w) for w in range(z.n_wild)]


def _check_mixed_history(z, prev, new, wild):
    _same_list(prev, statement_m("now").want)
    _same_list(new, statement_m("new").want)
    want = d64.history_map(prev, new)
    assert np.array_equal(new[3], want)
    mapped = want != NULL
    for w in range(z.n_wild):
        expect = np.zeros(len(want), np.float32)
        expect[mapped] = _row_codes(len(prev[0]), w)[want[mapped]]
        assert np.array_equal(wild[w].view(np.uint32), expect.view(np.uint32)), ("wildcard", w)


# ------------------------------------------------------------------------------------------------------------ driver
# One context, three detections (detect_triangles and detect_part1 of csrc/deme_hip.hip):
#   1  80 stacked small triangles in one bin: TP1 = 80 (bin, triangle) incidences; the driver sizes the incidence buffers to
#      TP1 + TP1 / 4 + 1024 = 1124
#   2  update_tri_nodes makes them right triangles with legs of 6 bins in the middle of a bin layer: 80 x (at least 18 bins) > 1124
#      -- the growth path `TP > triCap`; the spheres are still beside the plate
#   3  upload_state moves the 60 spheres onto the plate: 60 x 80 = 4800 mesh contacts, more than the contact arena of
#      max(6 nSpheres, 4096) = 4096 keys, so detect_part1 grows the arena and repeats the attempt, detect_triangles with it
D_K, D_S = 80, 60


@functools.lru_cache(maxsize=None)
def scene_d():
    pkg = _pkg()
    b, M, l, _ = _builder(pkg, BPW)
    bin_m = M * l
    r = float(np.float32(0.3 * bin_m))
    t = b.LoadSphereType(1e-3, r, 0)
    me = Mesh(np.rint(np.array([0.5, 0.5, 0.5]) / l), l, margin=W_MT)
    corner = np.array([20.2, 20.2, 25.5]) * bin_m
    small = np.array([[0, 0, 0], [0.3, 0, 0], [0, 0.3, 0]]) * bin_m
    large = np.array([[0, 0, 0], [6.0, 0, 0], [0, 6.0, 0]]) * bin_m
    for k in range(D_K):
        me.add(corner + small + np.array([0, 0, k * W_STACK]))
    stages = [np.float32([(corner + tri + np.array([0, 0, k * W_STACK]) - me.G * l) @ me.R for k in range(D_K)]) for tri in (small, large)]
    on, off = [], []
    for i in range(D_S):  # a grid of pitch 0.31 bin well inside the large face (x + y < 6 bins); beside the plate: 4 bins lower in y
        xy = np.array([0.5 + 0.31 * (i % 10), 0.5 + 0.31 * (i // 10)]) * bin_m
        c = corner + np.array([xy[0], xy[1], 0.6 * r + D_K * W_STACK])
        on.append(c), off.append(c - np.array([0, 4.0 * bin_m, 0]))
    b.AddClumps(t, _placeholder(D_S))
    z = _finish(pkg, b, np.rint(np.array(off) / l).astype(np.int64), np.zeros(D_S, np.float32), M, l, [me])
    p, A = z.params, b.arrays
    z.on_state = {k: np.array(A[k], copy=True) for k in
                  ("voxelID", "locX", "locY", "locZ", "oriQw", "oriQx", "oriQy", "oriQz", "vX", "vY", "vZ", "omgBarX", "omgBarY", "omgBarZ")}
    Gn = np.rint(np.array(on) / l).astype(np.int64)
    vox = Gn // 65536
    z.on_state["voxelID"][:D_S] = (vox[:, 0] + (vox[:, 1] << p.nvXp2) + (vox[:, 2] << (p.nvXp2 + p.nvYp2))).astype(np.uint64)
    for k, name in enumerate(("locX", "locY", "locZ")):
        z.on_state[name][:D_S] = (Gn[:, k] % 65536).astype(np.uint16)
    z.large_nodes = [np.ascontiguousarray(stages[1][:, k, :]) for k in range(3)]
    return z


@functools.lru_cache(maxsize=None)
def statement_d(stage):
    z = scene_d()
    if stage == 0:
        return _state(_pkg(), z)
    state = dict(triNode1=z.large_nodes[0].reshape(-1), triNode2=z.large_nodes[1].reshape(-1), triNode3=z.large_nodes[2].reshape(-1))
    if stage == 2:
        state.update(z.on_state)
    return _state(_pkg(), z, state=state)


def _run_driver(z, side, incidences=None):
    """the three detections; returns the three lists (and, from the oracle, the three incidence counts)"""
    side.set_margins(z.margins)
    out = []
    for stage in range(3):
        if stage == 1:
            side.update_tri_nodes(*z.large_nodes)
        if stage == 2:
            side.upload_state(z.on_state)
        side.detect()
        out.append(side.contacts())
        if incidences is not None:
            incidences.append(len(side.tri_incidence()[0]))
    return out


_SCENES.update(r=scene_r, c=scene_c, m=scene_m, d=scene_d)


# ------------------------------------------------------------------------------------------------------------ CPU tests, continued
def test_registration_design(pkg, orc):
    """no MAY pair; every designed pair is MUST with its designed region; the mesh rows of the statement are the designed pairs, each
    once (one component of the clump touches, the other does not); contact points in the first and the last bin of every axis, of
    the long triangles in many different bins; the smallest angle of the scene is the zoo's limit; the oracle's list is the
    statement's"""
    z, st = scene_r(), statement_r()
    assert (st.numerical, st.geometric) == (0, 0)
    assert dm.sufficient_implies_exact(st.pairs)
    verdict = _verdict_of(st)
    at = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(st.pairs["i_s"], st.pairs["i_t"]))}
    bins_of = {}
    for s, t, region, label in z.design:
        assert verdict[(s, t)] == dm.MUST, (s, t, region, label)
        assert int(st.pairs["region"][at[(s, t)]]) == region, (s, t, region, label)
        bins_of.setdefault(label, set()).add(tuple(np.floor(st.pairs["cpA"][at[(s, t)]] / z.bin_m).astype(int)))
    a, b_, t_ = st.want
    mesh = t_ == 2
    assert set(zip(a[mesh].tolist(), b_[mesh].tolist())) == {(s, t) for s, t, _, _ in z.design}
    assert z.clump_spheres[0] in a[mesh] and z.clump_spheres[1] not in a[mesh]
    assert len(bins_of["one bin"]) == 1 and len(bins_of["span 3"]) >= 3 and len(bins_of["span 10"]) >= 5 and len(bins_of["span 40"]) >= 8
    p = z.params
    last = (int(p.nbX) - 1, int(p.nbY) - 1, int(p.nbZ) - 1)
    c_, R_ = dm.centres(st.inputs)
    for s, t, _, label in z.design:
        if label == "bin plane wide":  # the sphere's box is wholly in bin 30, where A is; B is in bin 29
            assert np.floor((c_[s, 2] - R_[s]) / z.bin_m) == 30 and all(bn[2] == 30 for bn in bins_of[label])
    for ax in range(3):
        assert all(bn[ax] == 0 for bn in bins_of[f"first {'xyz'[ax]}"]) and all(bn[ax] == last[ax] for bn in bins_of[f"last {'xyz'[ax]}"])
    assert abs(np.degrees(st.inputs["tri_angle"].min()) - R_ANGLE_MIN) < 1e-3
    assert (st.inputs["tri"]["T"][:, :, 0].min() < 0)  # nodes outside the domain
    _strictly_increasing(st.want)
    got, (tb, tt), _, _ = _oracle_cached("r")
    _same_list(got, st.want)
    # most of a long triangle's bounding box is not registered
    T = st.inputs["tri"]["T"]
    for label, least in (("span 10", 0.5), ("span 40", 0.9), ("span 40 small", 0.9)):
        t = next(t for _, t, _, lb in z.design if lb == label)
        box = np.prod(np.floor(T[t].max(0) / z.bin_m) - np.floor(T[t].min(0) / z.bin_m) + 1)
        assert (tt == t).sum() < (1.0 - least) * box, (label, int((tt == t).sum()), box)


def test_column_design(pkg, orc):
    """scene C: no numerical MAY pair; the designed pairs are MAY (geometric) -- but for the column spheres nearest the face, within
    reach, which are MUST; where the statement decides, the scheme's rule agrees; the rule lists the designed pairs; the oracle's
    list is the rule's"""
    z, st = scene_c(), statement_c()
    assert st.numerical == 0 and st.geometric > 0
    want, keep = lattice_rule(z, st)
    pr = st.pairs
    assert keep[pr["verdict"] == dm.MUST].all() and not keep[pr["verdict"] == dm.MUST_NOT].any()
    verdict = _verdict_of(st)
    listed = set(zip(want[0][want[2] == 2].tolist(), want[1][want[2] == 2].tolist()))
    assert listed == {(s, t) for s, t, yes in z.design if yes}
    assert all(verdict[(s, t)] == dm.MAY for s, t, _ in z.design)
    assert st.geometric == len(z.design)
    got, _, _, _ = _oracle_cached("c")
    _same_list(got, want)
    _strictly_increasing(got)


def test_mixed_rows_and_history_design(pkg, orc):
    """no MAY pair in either state; sphere 0 has rows of all three classes, 70 of them with triangles; the groups' rows appear,
    persist and vanish as designed; the oracle's lists, history map and migrated wildcards are the statement's"""
    z = scene_m()
    for which in ("now", "new"):
        st = statement_m(which)
        assert (st.numerical, st.geometric) == (0, 0)
        a, b_, t = st.want
        assert sorted(set(t[a == 0].tolist())) == [1, 2, 11] and int(((a == 0) & (t == 2)).sum()) == H_K
        far = b_ >= H_K
        assert set(zip(a[(t == 2) & far].tolist(), b_[(t == 2) & far].tolist())) == set(z.design[which])
        _strictly_increasing(st.want)
    sim = orc.make_sim(pkg, z.params, z.scene)
    prev, new, wild = _run_mixed_history(z, sim)
    sim.close()
    _check_mixed_history(z, prev, new, wild)
    hm = d64.history_map(prev, new)
    assert (hm != NULL).sum() == 2 * H_K + 3 + H_PER_GROUP and (hm == NULL).sum() == 2 * H_PER_GROUP


def test_driver_design(pkg, orc):
    """no MAY pair at any stage; the second detection has more incidences than the buffers sized by the first hold, the third more
    contacts than the contact arena (both from the growth rules of the driver); the oracle's three lists are the statement's"""
    z = scene_d()
    sim = orc.make_sim(pkg, z.params, z.scene)
    tp = []
    lists = _run_driver(z, sim, tp)
    sim.close()
    assert tp[0] == D_K and tp[1] > tp[0] + tp[0] // 4 + 1024
    for stage in range(3):
        st = statement_d(stage)
        assert (st.numerical, st.geometric) == (0, 0)
        _same_list(lists[stage], st.want)
    assert int((lists[0][2] == 2).sum()) == int((lists[1][2] == 2).sum()) == 0
    assert int((lists[2][2] == 2).sum()) == D_K * D_S > max(6 * D_S, 4096)


def test_band_measured(pkg, orc):
    """the band against the oracle's own fp32 arithmetic: |depth of orc.tri_sphere(directional) on the oracle's fp32 sandwich - the
    float64 depth| on A and on B for every designed pair of scenes G and R, as a fraction of the pair's band: at most 1 / 4"""
    worst, worst_m, n = 0.0, 0.0, 0
    for kind, key, z, st in (("g", (True,), scene_g(True), statement_g(True)), ("g", (False,), scene_g(False), statement_g(False)),
                             ("r", (), scene_r(), statement_r())):
        _, _, sw, (X, Y, Z, Rf) = _oracle_cached(kind, *key)
        designed = [(r_["sphere"], r_["tri_id"]) for r_ in z.rows] if kind == "g" else [(s, t) for s, t, _, _ in z.design]
        at = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(st.pairs["i_s"], st.pairs["i_t"]))}
        idx = np.array([at[k] for k in designed])
        i_s, i_t = st.pairs["i_s"][idx], st.pairs["i_t"][idx]
        c, R = st.pairs["c"][idx], st.pairs["R"][idx]
        A64, B64 = dm.sandwich(st.inputs["tri"]["T"][i_t], st.inputs["tri"]["mt"][i_t])
        P = np.stack([X, Y, Z], 1)[i_s]
        for X64, k0 in ((A64, 0), (B64, 3)):
            d64_, _, _, _ = dm.depth_of(X64, c, R)
            _, _, d32, _ = orc.tri_sphere(sw[i_t, k0].astype(np.float64), sw[i_t, k0 + 1].astype(np.float64), sw[i_t, k0 + 2].astype(np.float64),
                                          P, Rf[i_s].astype(np.float64), directional=True)
            err = np.abs(d32 - d64_)
            worst, worst_m, n = max(worst, float((err / st.pairs["band"][idx]).max())), max(worst_m, float(err.max())), n + len(err)
    record_measured("mesh_detection_zoo band", depth_error_over_band=worst, depth_error_m=worst_m, depths=n, band_units=dm.BAND_UNITS)
    print(f"oracle fp32 depth against float64: {worst:.3f} of the band at the most, {worst_m:.3e} m, {n} depths")
    assert 4.0 * worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ GPU tests, continued
@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_registration(pkg, orc, monkeypatch, variant):
    z = scene_r()
    ctx = _context(pkg, z, variant, monkeypatch)
    _check_detection(ctx, z, statement_r(), _oracle_cached("r"))
    ctx.close()


@pytest.mark.gpu
def test_column(pkg, orc, monkeypatch):
    z = scene_c()
    ctx = _context(pkg, z, "caller order", monkeypatch)
    ctx.set_margins(z.margins)
    ctx.detect()
    got = ctx.contacts()
    _same_list(got, lattice_rule(z, statement_c())[0])
    _same_list(got, _oracle_cached("c")[0])
    ctx.close()


@pytest.mark.gpu
def test_mixed_rows_and_history(pkg, orc, monkeypatch):
    z = scene_m()
    ctx = _context(pkg, z, "caller order", monkeypatch)
    _check_mixed_history(z, *_run_mixed_history(z, ctx))
    ctx.close()


@pytest.mark.gpu
def test_driver_growth(pkg, orc, monkeypatch):
    z = scene_d()
    ctx = _context(pkg, z, "caller order", monkeypatch)
    lists = _run_driver(z, ctx)
    for stage in range(3):
        _same_list(lists[stage], statement_d(stage).want)
        _strictly_increasing(lists[stage])
    ctx.close()
