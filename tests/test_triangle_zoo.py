"""The triangle zoo: ~3000 ISOLATED sphere-triangle contacts, each of a known Voronoi region of its triangle and of a known branch
of the force model, each compared on its own scale with the float64 model (tests/_contact_model64.py, KIND_TRI: the closest point
on the triangle after Ericson 5.1.5, nothing taken from csrc/deme_mesh.h).  The machinery is that of tests/test_contact_zoo.py.

The mesh beds of the suite rest on a smooth, unrotated, fixed plate: nearly every contact is a face contact, no mesh owner has a
quaternion other than identity or a velocity, and a bed bounds every error by its largest force.  Here:

Classes (the float64 model labels every row; the zoo is built so that region and label are the designed ones):
  the seven regions  face, edge_ab, edge_ac, edge_bc, vert_a, vert_b, vert_c  crossed with the five branches  stick, slip,
  separating, roll_on, normal_only  of the existing zoo (35 classes "region/branch", 64 rows each): friction and rolling
  resistance on edge and vertex normals, and on levers PB of up to 0.8 m
  under        the centre 0.4 r BELOW the face: a face contact of depth 1.4 r along the face normal (sticking)
  deep_under   the centre 1.05 r below the face: listed, retired by the two-sided test (|h| >= r), zero force, history cleared
  margin       gap in (0, extra / 2]: touching, zero force;   apart: gap in [2, 3] x extra: listed, retired
  face/depth_1e-3, _1e-2, _1e-1 and edge_ab/depth_...: d / r across the range (sticking)
  far          nobody's design: the sweep's directional test has no far side, so a sphere over or under a face is listed with it
               where the two share a bin -- some 110 rows between the triangles of the small meshes, 10 extra margins or more
               above a face or two radii or more below it; the force pass retires them (zero force, history cleared)
Meshes: three large unrotated meshes of isolated triangles (two materials, two families; the owners sit up to 0.8 m from their
triangles), 40 small meshes of four triangles each with random unit quaternions (two of radius 2 mm for the small spheres, two
7 mm out for the large ones), four of them in a family that is not fixed and with v and w (set in the uploaded state; there is
one force evaluation).  Two sphere and two triangle materials, pairwise distinct, every pair with overrides.  Radii R0 and 12 R0.
Sphere family 3 is masked against mesh family 11: its 64 designed face contacts must not be listed.  Sphere family 1 and mesh
family 12 have twice the extra margin of the others, mesh family 11 half of it and 13 none, so min (the sweep's filter) and max
(the force body's) of the two sides differ from row to row.  Eight triangles of 60 mm span three or more bins per axis and carry
two large spheres each whose contact points lie in another bin than their centres; twelve ridges of two triangles sharing an edge
carry one sphere on that edge, two rows, each compared on its own.  The smallest angle of every triangle is 40 degrees or more.

What limits the yardstick, and the input rules that follow (ISSUE: a CPU trial with the oracle alone):
  the face normal is normalised with an fp32 reciprocal square root (the reference's normalize()): 1e-7 r in h, so a face contact
  needs d / r >= 0.06 -- or a triangle whose doubled area is a power of two, where that root is exact: the shallow face classes
  sit on axis-aligned right triangles with legs 2^-8 m;
  rot_apply_d multiplies fp64 nodes by fp32 rotation coefficients (the reference's own arithmetic): 1.5 x 2^-24 x lever / overlap,
  so the rotated meshes keep lever / overlap <= 56 (nodes within 2.4 mm for R0, 11 mm for 12 R0, d / r >= 0.1).
Thresholds: the margins, ft against mu |Fn| and the clocks are cleared by a factor 2 as in the existing zoo.  A region boundary is
cleared by a factor 2 in this sense: the region is the same when the in-plane offset of the centre from the region's anchor (the
centroid; the midpoint of the edge; the vertex) is doubled -- along the edge, across it (also halved), and in angle from the
bisector of a vertex's outward cone.  |h| against r: 'under' has |h| = 0.4 r; 'deep_under' is 0.05 r = 2.5e-5 m past the
threshold, 1e5 times the fp64 rounding of h (a factor 2 would leave the listing range of a sphere of radius R0 + 1e-4).

YARDSTICK e_orc[class] = the largest error of the ORACLE against the float64 model, relative to s (contact points: metres); largest
over hertz and frictionless and the two numberings.  Force, per region and branch:
                     stick        slip         separating   roll_on      normal_only
  face               1.1e-06      8.3e-07      2.5e-07      1.1e-06      1.5e-06
  edge_ab            8.5e-07      3.2e-07      1.6e-07      5.3e-07      8.2e-07
  edge_ac            4.5e-07      2.1e-06      1.2e-07      6.0e-07      1.1e-06
  edge_bc            6.0e-07      5.1e-07      1.7e-07      6.6e-07      6.1e-07
  vert_a             1.4e-06      5.0e-07      2.5e-07      7.3e-07      2.8e-06
  vert_b             9.9e-07      1.5e-06      2.4e-07      8.8e-07      5.7e-07
  vert_c             8.5e-07      1.0e-06      1.6e-07      1.0e-06      1.2e-06
  worst region: torque-only 7.4e-08 (roll_on, else 0), history 3.4e-07 (slip), clock 6.7e-08, PA 1.3e-09 m, PB 3.0e-08 m (|PB| <= 0.84 m)
  under 1.8e-07;  face/depth_1e-3, _1e-2, _1e-1: 1.8e-07, 1.2e-07, 9.2e-08;  edge_ab/depth_...: 1.3e-07, 1.6e-07, 1.2e-07
  deep_under, margin, apart, far: 0 (force, torque-only, history);  PA / PB of margin 5.9e-10 / 2.3e-08 m, of the retired classes 0
  per owner (spheres and small meshes): a 2.9e-06 of sum(s / m), alpha 4.8e-07 of sum(s |r| / MOI)
  the model's geometry against orc.tri_sphere on the zoo's rows: point 1e-16 m, edge / vertex depth 0, face depth 9e-08 |h|, normal 9e-08
(by mesh: rotated meshes 2.8e-06 -- 1.5 x 2^-24 x lever / overlap is 4.1e-06 at the most --, unrotated faces 1.5e-06 -- the fp32 root
of the face normal --, unrotated edges and vertices 1.7e-07.  The tests take the table from the
oracle run they make anyway; every figure goes to measured_errors.txt through record_measured.)

FAST-MODE BOUND per class, as in the existing zoo: FACTOR x max(e_orc[class], 2^-23), FACTOR = 4, under the ceiling 1e-5; contact
points FACTOR x max(e_orc, 2^-23 max(|P|max, R0)); dead rows exactly zero; a / alpha of the spheres and the small meshes on the owner's
own scale, of the large meshes (a thousand rows each) within the suite's 1e-3 tree bound; equal and opposite per contact.

ACHIEVED on an MI355X, fast mode (tiled: k_tile_forces<M, true>; untiled, 10 materials: k_calc_forces<M, 0> with recording and
k_forces_fast<M> without; both models, both numberings, with and without recording): F, T, PA, PB and the history of every row are
those of the table above TO THE LAST DIGIT -- the sphere-mesh rows are evaluated by k_calc_forces<M, 1>, the general kernel in the
reference's arithmetic, in both modes; what the fast mode adds is the pull of its records into the tile or the fast kernel and the
sums per owner.  Per owner: a 2.9e-06, alpha 4.9e-07 (bounds 1e-05, 1.9e-06); large meshes a 3.4e-08, alpha 3.4e-08 of their
scale; equal and opposite: 0.08 (forces) and 0.21 (torques) of their bounds.  Exact mode: bit-identical to the oracle (lists,
records, history, a / alpha of the spheres and small meshes).  inspect_tri_loads: equal to the fp64 sums, counts 0 / 1 / 2.

MUTATIONS, each built and run once on an MI355X (not kept).  All twelve GPU cases of this file fail under every one of them:
  snap_to_face, BC edge: w -> 1 - w             the lists differ (the sweep's contact-point bin)
  tri_sphere_cd: `|| h <= -radius` dropped      deep_under and the far rows below a face carry force and records (173 rows)
  k_tri_prep: sandwich vertices not rotated     the lists differ
  mesh branch: bodyBMatType = 0                 every force class off by 0.3 .. 0.5 s; exact mode: records differ
  mesh branch: locCPB from AOwnerPos            PB off by 0.84 m, forces by 4e-4 s (the lever in the relative velocity)
tests/test_mesh.py, tests/test_tri_loads.py and tests/test_fast_mode_features.py (29 GPU tests) without this file: the second and
the fourth mutation pass all 29; the first fails two (test_mesh_contacts_and_forces_match_oracle, test_deforming_free_mesh), the
third one (test_deforming_free_mesh: 494 contacts against 492), the fifth the same two as the first.
"""
import functools

import numpy as np
import pytest

from tests import _contact_model64 as m64
from tests._tri_loads64 import tri_loads
from tests.conftest import record_measured
from tests.test_contact_zoo import (CEILING, EXTRA, FACTOR, H, MARGIN, R0, RHO, U32, _owner_fails, class_errors, positions64,
                                    run_sides)  # (run_sides seeds the history through design_history, by the row's branch: c["cls"])

REGIONS = ("face", "vert_a", "vert_b", "vert_c", "edge_ab", "edge_ac", "edge_bc")  # index = the model's region code
GEO7 = ("face", "edge_ab", "edge_ac", "edge_bc", "vert_a", "vert_b", "vert_c")
BRANCH5 = ("stick", "slip", "separating", "roll_on", "normal_only")
LADDER = tuple(f"{g}/depth_{d}" for g in ("face", "edge_ab") for d in ("1e-3", "1e-2", "1e-1"))
CROSSED = tuple(f"{g}/{b}" for g in GEO7 for b in BRANCH5)
DEAD = ("deep_under", "margin", "apart", "far")
CLASSES = CROSSED + ("under",) + LADDER + DEAD
DESIGNED = CLASSES[:-1]  # 'far' rows are nobody's design: see test_triangle_zoo_design_holds
N_PER_CLASS = 64
NUMBERINGS = ("spheres-first", "scattered")
CELL, CELL0, NCELL = 0.048, 0.06, 18
S0, S1, T0, T1 = 0, 1, 2, 3
MATERIALS = [
    {"E": 1.0e8, "nu": 0.30, "CoR": 0.60, "mu": 0.20, "Crr": 0.00},   # spheres
    {"E": 4.0e6, "nu": 0.22, "CoR": 0.35, "mu": 0.30, "Crr": 0.05},
    {"E": 5.0e7, "nu": 0.28, "CoR": 0.50, "mu": 0.45, "Crr": 0.00},   # triangles
    {"E": 2.0e7, "nu": 0.36, "CoR": 0.65, "mu": 0.15, "Crr": 0.06},
]
OVERRIDES = [("Crr", S1, T1, 0.0), ("mu", S0, T1, 0.61), ("CoR", S1, T0, 0.42), ("CoR", S0, T0, 0.33), ("mu", S1, T1, 0.27),
             ("Crr", S1, T0, 0.07)]
ROLLING = {T0: S1, T1: S0}      # the sphere material that has Crr > 0 with this triangle material ...
NOT_ROLLING = {T0: S0, T1: S1}  # ... and the one that has none
FAM_WIDE, FAM_MASKED, MESH_FIXED, MESH_MASKED, MESH_FREE, MESH_SMALL = 1, 3, 10, 11, 12, 13
FAMILY_EXTRA = {0: EXTRA, FAM_WIDE: 2 * EXTRA, FAM_MASKED: EXTRA, MESH_FIXED: EXTRA, MESH_MASKED: EXTRA / 2, MESH_FREE: 2 * EXTRA,
                MESH_SMALL: 0.0}
N_SMALL_MESHES, N_FREE, N_BIG_TRI, N_RIDGES, N_MASKED = 40, 4, 8, 12, 64
TILE_TABLE_MAX = 4096


def _tables(n_mat):
    def prop(k):
        return np.array([m[k] for m in MATERIALS] + [MATERIALS[0][k]] * (n_mat - len(MATERIALS)), np.float32)

    def pair(k):
        v = prop(k)
        M = ((v[:, None] + v[None, :]) / np.float32(2.0)).astype(np.float32)
        M[np.arange(n_mat), np.arange(n_mat)] = v
        for name, a, b, val in OVERRIDES:
            if name == k:
                M[a, b] = M[b, a] = np.float32(val)
        return M.astype(np.float64)
    E_cnt, G_cnt, beta = m64.pair_table(prop("E"), prop("nu"), pair("CoR"))
    return dict(E_cnt=E_cnt, G_cnt=G_cnt, beta=beta, mu=pair("mu"), Crr=pair("Crr"))


def _unit(v):
    return v / np.linalg.norm(v)


def _frame(rng):
    """a random right-handed orthonormal frame (rows e1, e2, n)"""
    n = _unit(rng.normal(size=3))
    e1 = _unit(np.cross(n, rng.normal(size=3)))
    return np.array([e1, np.cross(n, e1), n])


def _fan(rng, rho):
    """three points on a circle of radius rho, counter-clockwise, arcs of 100 .. 160 degrees: angles of 40 degrees or more"""
    t0 = rng.uniform(0, 2 * np.pi)
    t1 = t0 + np.radians(rng.uniform(100, 140))
    t2 = t1 + np.radians(rng.uniform(100, 140))
    return np.array([[rho * np.cos(t), rho * np.sin(t), 0.0] for t in (t0, t1, t2)])


def _anchor(region, tri):
    """the anchor of a region and its in-plane axes: (point, along, outward); face: the centroid"""
    A, B, C = tri
    n = _unit(np.cross(B - A, C - A))
    if region == 0:
        return tri.mean(0), None, None, n
    if region >= 4:
        X, Y, Z = {4: (A, B, C), 5: (A, C, B), 6: (B, C, A)}[region]
        e = _unit(Y - X)
        m = np.cross(e, n)
        if m @ (Z - X) > 0:
            m = -m
        return 0.5 * (X + Y), e, m, n
    V, Y, Z = {1: (A, B, C), 2: (B, C, A), 3: (C, A, B)}[region]
    b = _unit(-(_unit(Y - V) + _unit(Z - V)))
    return V, np.cross(n, b), b, n


def _place(rng, region, tri, reach):
    """a sphere centre at distance `reach` from its closest point on the triangle, which lies in the given region; for the face
    `reach` is the signed height.  Returns (centre, closest point, normal B2A)"""
    A, B, C = tri
    O, e, m, n = _anchor(region, tri)
    if region == 0:
        w = 0.2 + 0.4 * rng.dirichlet(np.ones(3))
        q = w @ tri
        return q + reach * n, q, n
    th = np.radians(rng.uniform(25, 65))
    if region >= 4:
        L = {4: np.linalg.norm(B - A), 5: np.linalg.norm(C - A), 6: np.linalg.norm(C - B)}[region]
        q = O + rng.uniform(-0.2, 0.2) * L * e
        u = np.cos(th) * n + np.sin(th) * m
        return q + reach * u, q, u
    V, Y, Z = {1: (A, B, C), 2: (B, C, A), 3: (C, A, B)}[region]
    half = 0.5 * (np.pi - np.arccos(np.clip(_unit(Y - V) @ _unit(Z - V), -1, 1)))
    phi = rng.uniform(-0.4, 0.4) * half
    u = np.cos(th) * n + np.sin(th) * (np.cos(phi) * m + np.sin(phi) * e)
    return O + reach * u, O, u


class Zoo:
    pass


@functools.lru_cache(maxsize=None)
def build_zoo(numbering, model, extra_materials=0, seed=4099):
    import __graft_entry__ as entry
    pkg = entry.load_package()
    rng = np.random.default_rng(seed)
    tab = _tables(len(MATERIALS))
    b = pkg.SceneBuilder()
    for mat in MATERIALS:
        b.LoadMaterial(mat)
    for _ in range(extra_materials):  # used by no contact: only the size of the table changes
        b.LoadMaterial(dict(MATERIALS[0]))
    for name, a, c, val in OVERRIDES:
        b.SetMaterialPropertyPair(name, a, c, val)
    b.InstructBoxDomainDimension((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
    b.InstructBoxDomainBoundingBC("none", 0)
    b.SetInitTimeStep(H)
    b.SetGravitationalAcceleration((0, 0, -9.81))
    b.SetCDUpdateFreq(0)
    for fam, ex in FAMILY_EXTRA.items():
        b.SetFamilyExtraMargin(fam, ex)
    for fam in (MESH_FIXED, MESH_MASKED, MESH_SMALL):
        b.SetFamilyFixed(fam)
    b.DisableContactBetweenFamilies(FAM_MASKED, MESH_MASKED)
    if model == "frictionless":
        b.UseFrictionlessHertzianModel()
    radii = (R0, 12 * R0)
    masses = [RHO * 4.0 / 3.0 * np.pi * r ** 3 for r in radii]
    tmpl = [b.LoadClumpType(m, (0.4 * m * r * r,) * 3, [r], [[0, 0, 0]], 0) for m, r in zip(masses, radii)]
    _, lat, _ = b._figure_out_nv()
    # the bin size depends on the domain and the smallest radius alone: a throw-away Initialize of the empty scene tells it
    import copy
    probe = copy.deepcopy(b)
    probe.AddClumps([probe.templates[0]], np.array([[0.5, 0.5, 0.5]], np.float32))
    p0, _ = probe.Initialize()
    bin_size = float(p0.binSize)
    lbf = b.target_box_min.astype(np.float64)
    snap = lambda x: lbf + np.rint((np.asarray(x, np.float64) - lbf) / lat) * lat  # noqa: E731

    # ---- the cells: the two top layers go to the eight 60 mm triangles (blocks of 2 x 2 x 2), the rest one triangle or small mesh each
    free_cells = [k for k in rng.permutation(NCELL ** 3) if k // (NCELL * NCELL) < NCELL - 2]
    cell_i = [0]

    def cell_centre(k):
        return CELL0 + CELL * np.array([k % NCELL, (k // NCELL) % NCELL, k // (NCELL * NCELL)], np.float64)

    def next_cell():
        cell_i[0] += 1
        return cell_centre(int(free_cells[cell_i[0] - 1]))

    # ---- meshes: dicts with pos, q (w x y z, fp32), mat, fam, mass, moi, tris (local fp32 nodes), v, w
    meshes = []

    def add_mesh(pos, q, mat, fam, mass, moi):
        meshes.append(dict(pos=snap(pos), q=np.asarray(q, np.float32), mat=mat, fam=fam, mass=mass, moi=moi, tris=[], v=np.zeros(3),
                           w=np.zeros(3), R=m64.rot_matrix(np.asarray(q, np.float32)[None, :].astype(np.float64))[0]))
        return len(meshes) - 1

    def add_tri(mi, local_nodes):
        """returns (mesh, index within the mesh, the world nodes in float64 as the kernels will see them)"""
        me = meshes[mi]
        loc = np.asarray(local_nodes, np.float32)
        me["tris"].append(loc)
        return mi, len(me["tris"]) - 1, me["pos"][None, :] + loc.astype(np.float64) @ me["R"].T

    ident = (1.0, 0.0, 0.0, 0.0)
    U = [add_mesh((0.5, 0.5, 0.5), ident, T0, MESH_FIXED, 0.5, (1e-3, 1e-3, 2e-3)),
         add_mesh((0.2, 0.7, 0.9), ident, T1, MESH_FIXED, 0.8, (2e-3, 1e-3, 1e-3)),
         add_mesh((0.9, 0.1, 0.3), ident, T0, MESH_MASKED, 0.3, (1e-3, 3e-3, 1e-3))]

    def rand_q():
        q = pkg.model.random_unit_quaternions(1, rng)[0]  # x y z w
        return np.array([q[3], q[0], q[1], q[2]], np.float32)

    small = []  # (mesh, its four triangles: inner up, inner down, outer up, outer down)
    for k in range(N_SMALL_MESHES):
        free = k < N_FREE
        mi = add_mesh(next_cell(), rand_q(), (T0, T1)[k % 2], MESH_FREE if free else MESH_SMALL, 1e-3, (1.0e-7, 1.4e-7, 0.8e-7))
        tris = []
        for rho, zz in ((2.0e-3, 1.2e-3), (2.0e-3, -1.2e-3), (8.0e-3, 7.0e-3), (8.0e-3, -7.0e-3)):
            f = _fan(rng, rho)
            if zz < 0:
                f = f[::-1]  # the normal points away from the mesh's origin
            f[:, 2] = zz
            tris.append(add_tri(mi, f))
        small.append((mi, tris))

    # ---- spheres: dicts with tmpl, pos, q, v, w, mat, fam; rows: (sphere, mesh, tri in mesh) -> (label, region, branch)
    spheres, design, masked = [], {}, []

    def rand_w(size):
        return _unit(rng.normal(size=3)) * size if size else np.zeros(3)

    def tangent(n):
        return _unit(np.cross(n, rng.normal(size=3)))

    def motion(branch, n, a, c, mA, mB, rA, depth):
        if depth <= 0:
            return rng.normal(size=3) * 0.05, 5.0
        if branch == "normal_only":
            return np.zeros(3), 0.0
        k_n, g_n, k_t, g_t, _ = m64.coefficients(tab["E_cnt"][a, c], tab["G_cnt"][a, c], tab["beta"][a, c], mA, mB, rA, m64.HUGE_RADIUS, depth)
        Fn0 = k_n * depth
        mu = tab["mu"][a, c]
        vn, Fn = (3.0 * Fn0 / abs(g_n), 2.0 * Fn0) if branch == "separating" else (-0.3 * Fn0 / abs(g_n), 1.3 * Fn0)
        vt = 0.05 * mu * Fn / abs(g_t)  # (with the seeded history of 0.3 mu Fn / k_t and k_t h v_t: below mu Fn / 2)
        return vn * n + vt * tangent(n), 0.3 * vt / rA

    def add_row(label, region, branch, tri, big, depth=None, reach=None, fam=None):
        """one sphere on one triangle.  depth: overlap (negative: gap); reach overrides it with the signed height over the face"""
        mi, ti, W = tri
        me = meshes[mi]
        r = radii[1] if big else radii[0]
        P, q, n = _place(rng, region, W, (r - depth) if reach is None else reach)
        if reach is not None:
            depth = (r - reach) if -r < reach else -1.0
        a = (ROLLING if branch == "roll_on" else NOT_ROLLING)[me["mat"]]
        vrel, wsz = motion(branch, n, a, me["mat"], masses[big], me["mass"], r, depth)
        spheres.append(dict(tmpl=int(big), pos=snap(P), q=rand_q(), vrel=vrel, w=rand_w(wsz), mat=a, q_contact=q,
                            fam=(FAM_WIDE if len(spheres) % 3 == 0 else 0) if fam is None else fam, mesh=mi))
        design[(len(spheres) - 1, mi, ti)] = (label, region, branch)
        return len(spheres) - 1

    def flat_dyadic_triangle(mi, C):
        """a right triangle with legs 2^-8 m along two coordinate axes: |AB x AC| = 2^-16, whose fp32 reciprocal root is exact"""
        ax = rng.permutation(3)
        leg = 2.0 ** -8
        me = meshes[mi]
        base = np.float32(np.asarray(C) - me["pos"]).astype(np.float64)
        base = np.round(base * 2 ** 20) / 2 ** 20  # nodes on a grid of 2^-20 m, exact in fp32 below 8 m
        A = base.copy()
        B, Cn = base.copy(), base.copy()
        B[ax[0]] += leg
        Cn[ax[1]] += leg
        Cn[ax[0]] += leg * (rng.integers(1, 4) / 4.0)
        nodes = [A, B, Cn] if rng.integers(2) else [A, Cn, B]
        return add_tri(mi, nodes)

    def loose_triangle(mi, C, rho):
        me = meshes[mi]
        return add_tri(mi, np.asarray(C) - me["pos"] + _fan(rng, rho) @ _frame(rng))

    def region_of(name):
        return REGIONS.index(name)

    # the slots of the small meshes go round the 35 crossed classes (and a few 'under' on the inner triangles)
    slots = [(mi, t, k >= 2) for mi, tris in small for k, t in enumerate(tris)]
    n_of = {c: 0 for c in CLASSES}
    for s, (mi, t, big) in enumerate(slots):
        free = meshes[mi]["fam"] == MESH_FREE
        if s % 9 == 8 and not big:
            r = radii[0]
            add_row("under", 0, "stick", t, False, reach=-0.4 * r)
            n_of["under"] += 1
            continue
        cls = CROSSED[(s * 11) % len(CROSSED)]
        g, br = cls.split("/")
        if free and br == "normal_only":
            cls, br = f"{g}/stick", "stick"
        r = radii[big]
        add_row(cls, region_of(g), br, t, big, depth=r * rng.uniform(0.1, 0.15))
        n_of[cls] += 1

    # the bulk on the three unrotated meshes
    def host(k):
        return U[k % 3]

    count = 0
    for cls in DESIGNED:
        while n_of[cls] < N_PER_CLASS:
            k = count
            count += 1
            big = k % 4 == 3
            r = radii[big]
            mi = host(k)
            if cls in CROSSED:
                g, br = cls.split("/")
                dr = rng.uniform(0.06, 0.12) if g == "face" else rng.uniform(0.01, 0.1)
                add_row(cls, region_of(g), br, loose_triangle(mi, next_cell(), 6e-3 if big else 2.5e-3), big, depth=r * dr)
            elif cls in LADDER:
                g, d = cls.split("/depth_")
                tri = flat_dyadic_triangle(mi, next_cell()) if g == "face" else loose_triangle(mi, next_cell(), 2.5e-3)
                add_row(cls, region_of(g), "stick", tri, False, depth=radii[0] * float(d))
            elif cls == "under":
                add_row(cls, 0, "stick", loose_triangle(mi, next_cell(), 6e-3 if big else 2.5e-3), big, reach=-0.4 * r)
            elif cls == "deep_under":
                add_row(cls, 0, "apart", loose_triangle(mi, next_cell(), 6e-3 if big else 2.5e-3), big, reach=-1.05 * r)
            else:
                fam = (0, FAM_WIDE)[k % 2]
                ex = max(FAMILY_EXTRA[fam], FAMILY_EXTRA[meshes[mi]["fam"]])
                gap = ex * (rng.uniform(0.1, 0.5) if cls == "margin" else rng.uniform(2.0, 3.0))
                add_row(cls, int(rng.integers(7)), cls, loose_triangle(mi, next_cell(), 6e-3 if big else 2.5e-3), big, depth=-gap, fam=fam)
            n_of[cls] += 1

    # the masked family: designed face contacts on the masked mesh that must not be listed
    for k in range(N_MASKED):
        tri = loose_triangle(U[2], next_cell(), 2.5e-3)
        s = add_row("masked", 0, "stick", tri, False, depth=radii[0] * 0.08, fam=FAM_MASKED)
        masked.append(s)
        del design[(s, tri[0], tri[1])]

    # ridges: two triangles sharing the edge BC of the first (AB of the second), folded 30 degrees down each; one sphere on the edge
    ridges = []
    for k in range(N_RIDGES):
        mi, C = host(k), next_cell()
        F = _frame(rng)
        half, fold = 2.5e-3, np.radians(30)
        Bn, Cn = -half * F[0], half * F[0]
        down = lambda sgn: 3.5e-3 * (sgn * np.cos(fold) * F[1] - np.sin(fold) * F[2]) + rng.uniform(-0.5e-3, 0.5e-3) * F[0]  # noqa: E731
        me = meshes[mi]
        # fp32 nodes shared bit for bit between the two triangles
        nb, nc = np.float32(C + Bn - me["pos"]), np.float32(C + Cn - me["pos"])
        na, nd = np.float32(C + down(-1.0) - me["pos"]), np.float32(C + down(1.0) - me["pos"])
        t1 = add_tri(mi, [na, nc, nb])           # A on the -F[1] side: the normal has a positive F[2] component
        t2 = add_tri(mi, [nb, nc, nd])           # its AB is the shared edge, reversed; the normal points up as well
        r = radii[0]
        W = t1[2]
        q = W[1] + rng.uniform(0.3, 0.7) * (W[2] - W[1])
        depth = r * rng.uniform(0.03, 0.1)
        a = NOT_ROLLING[me["mat"]]
        spheres.append(dict(tmpl=0, pos=snap(q + (r - depth) * F[2]), q=rand_q(), vrel=np.zeros(3), w=np.zeros(3), mat=a, q_contact=q,
                            fam=0, mesh=mi))
        s = len(spheres) - 1
        design[(s, mi, t1[1])] = ("edge_bc/normal_only", 6, "normal_only")
        design[(s, mi, t2[1])] = ("edge_ab/normal_only", 4, "normal_only")
        ridges.append((s, t1, t2))

    # eight triangles of 60 mm across the diagonal of a block of 2 x 2 x 2 cells: three or more bins per axis; two large spheres each,
    # placed where the contact point and the centre fall into different bins (found after Initialize, below: the bin size is known then)
    bigtris = []
    for k in range(N_BIG_TRI):
        i, j = 2 * (k % 4) + 1, 2 * (k // 4) + 1
        C = CELL0 + CELL * np.array([i + 0.5, j + 0.5, NCELL - 1.5])
        mi = host(k)
        n = _unit(np.array([1.0, 1.0, 1.0]) * rng.choice([-1.0, 1.0], 3))  # oblique: the bounding box is wide along every axis
        e1 = _unit(np.cross(n, [1.0, 0.0, 0.0]))
        while True:  # three bins or more along every axis, wherever the box starts
            nodes = C - meshes[mi]["pos"] + _fan(rng, 34e-3) @ np.array([e1, np.cross(n, e1), n])
            if (np.ptp(nodes, axis=0) >= 3.0 * bin_size).all():
                break
        tri = add_tri(mi, nodes)
        bigtris.append(tri)

    return _finish(pkg, b, rng, numbering, extra_materials, tmpl, radii, meshes, spheres, design, masked, ridges, bigtris, snap, bin_size)


def _finish(pkg, b, rng, numbering, extra_materials, tmpl, radii, meshes, spheres, design, masked, ridges, bigtris, snap, bin_size):
    lbf = b.target_box_min.astype(np.float64)
    bins = lambda x: np.floor((np.asarray(x) - lbf) / bin_size).astype(np.int64)  # noqa: E731
    crossing = []
    for tri in bigtris:
        W = tri[2]
        assert ((bins(W.max(0)) - bins(W.min(0))) >= 2).all(), "a 60 mm triangle spans three or more bins along every axis"
        centres = []
        for _ in range(2):
            for attempt in range(2000):
                w = 0.18 + 0.46 * rng.dirichlet(np.ones(3) * 0.3)
                q = w @ W
                n = _unit(np.cross(W[1] - W[0], W[2] - W[0]))
                r = radii[1]
                depth = r * 0.08
                P = q + (r - depth) * n
                ok = (bins(P) != bins(q)).any() and np.abs((q - lbf) / bin_size - np.rint((q - lbf) / bin_size)).min() > 0.05
                ok = ok and all(np.linalg.norm(P - c) > 2 * r + 4 * MARGIN + 2e-3 for c in centres)
                if ok:
                    break
            assert ok
            me = meshes[tri[0]]
            a = NOT_ROLLING[me["mat"]]
            spheres.append(dict(tmpl=1, pos=snap(P), q=np.array([1, 0, 0, 0], np.float32), vrel=np.zeros(3), w=np.zeros(3), mat=a,
                                q_contact=q, fam=0, mesh=tri[0]))
            design[(len(spheres) - 1, tri[0], tri[1])] = ("face/normal_only", 0, "normal_only")
            crossing.append(len(spheres) - 1)
            centres.append(P)

    # ---- the free meshes move: v and w a fraction of the smallest relative velocity among their rows; the spheres ride on top
    rows_of_mesh = {}
    for (s, mi, ti), d in design.items():
        rows_of_mesh.setdefault(mi, []).append(s)
    for mi, me in enumerate(meshes):
        if me["fam"] != MESH_FREE:
            continue
        vmin = min(np.linalg.norm(spheres[s]["vrel"]) for s in rows_of_mesh[mi])
        me["v"] = _unit(rng.normal(size=3)) * 0.3 * vmin
        me["w"] = _unit(rng.normal(size=3)) * 0.3 * vmin / 11e-3
    for sp in spheres:
        me = meshes[sp["mesh"]]
        PB = me["R"].T @ (sp["q_contact"] - me["pos"])
        sp["v"] = me["v"] + me["R"] @ np.cross(me["w"], PB) + sp["vrel"]

    # ---- numbering of the spheres (the mesh owners follow the clumps in every scene)
    n_sph = len(spheres)
    order = np.arange(n_sph) if numbering == "spheres-first" else rng.permutation(n_sph)
    new_of_old = np.empty(n_sph, np.int64)
    new_of_old[order] = np.arange(n_sph)
    sph = [spheres[i] for i in order]
    batch = b.AddClumps([tmpl[s["tmpl"]] for s in sph], np.array([s["pos"] for s in sph], np.float32))
    batch.SetFamily(np.array([s["fam"] for s in sph], np.uint8))
    tri_base = []
    for me in meshes:
        nodes = np.array(me["tris"], np.float32).reshape(-1, 3)
        mo = b.AddMeshObject(nodes, np.arange(len(nodes)).reshape(-1, 3), me["mat"])
        mo.SetInitPos(me["pos"]), mo.SetMass(me["mass"]), mo.SetMOI(me["moi"]), mo.SetFamily(me["fam"])
        tri_base.append(sum(len(m["tris"]) for m in meshes[:len(tri_base)]))
    p, sc = b.Initialize()
    A = b.arrays
    n_own = n_sph + len(meshes)
    assert n_own == int(b.counts["nOwners"])
    pos = np.array([s["pos"] for s in sph] + [me["pos"] for me in meshes])
    G = np.rint((pos - lbf) / p.l).astype(np.int64)
    vox = G // 65536
    A["voxelID"][:] = (vox[:, 0] + (vox[:, 1] << p.nvXp2) + (vox[:, 2] << (p.nvXp2 + p.nvYp2))).astype(np.uint64)
    for k, name in enumerate(("locX", "locY", "locZ")):
        A[name][:] = (G[:, k] % 65536).astype(np.uint16)
    Q = np.array([s["q"] for s in sph] + [me["q"] for me in meshes], np.float32)
    V = np.array([s["v"] for s in sph] + [me["v"] for me in meshes], np.float32)
    W = np.array([s["w"] for s in sph] + [me["w"] for me in meshes], np.float32)
    for k, name in enumerate(("oriQw", "oriQx", "oriQy", "oriQz")):
        A[name][:] = Q[:, k]
    for k in range(3):
        A[("vX", "vY", "vZ")[k]][:] = V[:, k]
        A[("omgBarX", "omgBarY", "omgBarZ")[k]][:] = W[:, k]
    A["sphereMaterialOffset"][:] = np.array([s["mat"] for s in sph], np.uint16)
    z = Zoo()
    z.builder, z.params = b, p
    z.scene = pkg.abi.make_scene_struct(A, b.counts)
    z.n_clumps = n_sph
    z.tables = _tables(len(MATERIALS) + extra_materials)
    z.margins = np.full(n_own, MARGIN, np.float32)
    z.design = {(int(new_of_old[s]), tri_base[mi] + ti): d for (s, mi, ti), d in design.items()}
    z.masked = new_of_old[np.array(masked)]
    z.crossing = new_of_old[np.array(crossing)]
    z.ridge_spheres = new_of_old[np.array([r[0] for r in ridges])]
    z.big_tris = np.array([tri_base[t[0]] + t[1] for t in bigtris])
    z.small_meshes = np.array([n_sph + mi for mi, me in enumerate(meshes) if me["fam"] in (MESH_FREE, MESH_SMALL)])
    z.free_meshes = np.array([n_sph + mi for mi, me in enumerate(meshes) if me["fam"] == MESH_FREE])
    z.large_meshes = np.array([n_sph + mi for mi, me in enumerate(meshes) if me["fam"] in (MESH_FIXED, MESH_MASKED)])
    z.bin_size = bin_size
    z.gather_inputs = gather_inputs
    return z


def gather_inputs(pkg, z, contacts, hist):
    """the float64 model's inputs for the listed rows (sphere, triangle, type 2), from the scene arrays"""
    A = z.builder.arrays
    idA, idB, typ = (np.asarray(x).astype(np.int64) for x in contacts[:3])
    assert (typ == 2).all(), "the zoo has sphere-triangle rows only"
    f = lambda k: np.asarray(A[k], np.float64)  # noqa: E731
    oA = np.asarray(A["ownerClumpBody"], np.int64)[idA]
    oB = np.asarray(A["ownerMesh"], np.int64)[idB]
    X = positions64(pkg, z)
    Q = np.stack([f("oriQw"), f("oriQx"), f("oriQy"), f("oriQz")], 1)
    V, W = np.stack([f("vX"), f("vY"), f("vZ")], 1), np.stack([f("omgBarX"), f("omgBarY"), f("omgBarZ")], 1)
    ip = np.asarray(A["inertiaPropOffsets"], np.int64)
    mass = f("MassProperties")[ip]
    moi = np.stack([f("moiX"), f("moiY"), f("moiZ")], 1)[ip]
    comp = np.asarray(A["clumpComponentOffset"], np.int64)
    rel = np.stack([f("CDRelPosX"), f("CDRelPosY"), f("CDRelPosZ")], 1)
    tri = np.stack([f("triNode1").reshape(-1, 3), f("triNode2").reshape(-1, 3), f("triNode3").reshape(-1, 3)], 1)[idB]
    mA_, mB_ = np.asarray(A["sphereMaterialOffset"], np.int64)[idA], np.asarray(A["triMaterialOffset"], np.int64)[idB]
    fam = np.asarray(A["familyID"], np.int64)
    ex = f("familyExtraMarginSize")
    T = z.tables
    n = len(idA)
    des = [z.design.get((int(a), int(t)), ("far", -1, "apart")) for a, t in zip(idA, idB)]
    c = dict(posA=X[oA], posB=X[oB], qA=Q[oA], qB=Q[oB], vA=V[oA], vB=V[oB], wA=W[oA], wB=W[oB], mA=mass[oA], mB=mass[oB],
             relA=rel[comp[idA]], rA=f("Radii")[comp[idA]], kind=np.full(n, m64.KIND_TRI), relB=np.zeros((n, 3)),
             rB=np.full(n, m64.HUGE_RADIUS), dirB=np.zeros((n, 3)), sizeB=np.zeros(n), signB=np.zeros(n), tri=tri,
             E_cnt=T["E_cnt"][mA_, mB_], G_cnt=T["G_cnt"][mA_, mB_], beta=T["beta"][mA_, mB_], mu=T["mu"][mA_, mB_], Crr=T["Crr"][mA_, mB_],
             hist=np.asarray(hist, np.float64), extra=np.maximum(ex[fam[oA]], ex[fam[oB]]), extra_min=np.minimum(ex[fam[oA]], ex[fam[oB]]))
    c.update(ownerA=oA, ownerB=oB, matA=mA_, matB=mB_, mass=mass, moi=moi, idA=idA, idB=idB,
             cls=np.array([d[2] for d in des], dtype=object),      # the branch: what design_history seeds by
             label=np.array([d[0] for d in des], dtype=object),    # the class of the tables
             region=np.array([d[1] for d in des]))
    return c


def by_label(c):
    return dict(c, cls=c["label"])


@functools.lru_cache(maxsize=None)
def oracle_yardstick(numbering, model, extra_materials=0):
    """the oracle's run of the zoo and its errors against the float64 model (e_orc), computed once per scene"""
    import __graft_entry__ as entry
    pkg, orc = entry.load_package(), entry.load_oracle()
    z = build_zoo(numbering, model, extra_materials)
    sim = orc.make_sim(pkg, z.params, z.scene)
    c, (ro,) = run_sides(pkg, z, [sim], model)
    ref = m64.contact64(c, H, model)
    e = class_errors(ro, ref, by_label(c), CLASSES)
    nO = int(z.builder.counts["nOwners"])
    a, al, cA, cB, sa, sl = m64.owner_sums64(ref, c["ownerA"], c["ownerB"], nO, c["mass"], c["moi"], c["mB"])
    tight = tight_owners(z)
    with np.errstate(divide="ignore", invalid="ignore"):
        ea = np.where(sa > 0, np.abs(ro["a"] - a).max(1) / sa, 0.0)[tight]
        el = np.where(sl > 0, np.abs(ro["al"] - al).max(1) / sl, 0.0)[tight]
    own = dict(a=a, al=al, sa=sa, sl=sl, cA=cA, cB=cB, e_a=float(ea.max()), e_al=float(el.max()))
    sim_lists = sim.contacts()
    sim.close()
    return z, c, ref, ro, e, own, sim_lists


def tight_owners(z):
    """the owners held to the per-owner bound: the spheres and the small meshes (four rows at the most)"""
    t = np.zeros(int(z.builder.counts["nOwners"]), bool)
    t[:z.n_clumps] = True
    t[z.small_meshes] = True
    return t


def _doubled_offsets_keep_the_region(c, ref, rows):
    """the region of every row is the same with the centre's in-plane offset from the region's anchor doubled (see the docstring)"""
    g = m64.geometry(c)
    N = c["posB"][:, None, :] + np.einsum("nij,nkj->nki", g["RB"], c["tri"])
    P = c["posA"] + m64._mv(g["RA"], c["relA"])
    bad = []
    for i in np.nonzero(rows)[0]:
        reg = int(ref["region"][i])
        O, e, m, n = _anchor(reg, N[i])
        y = P[i] - O
        hgt = y @ n
        y = y - hgt * n
        if reg == 0:
            trial = [O + 2 * y]
        elif reg >= 4:
            a_, x_ = y @ e, y @ m
            trial = [O + 2 * a_ * e + x_ * m, O + a_ * e + 0.5 * x_ * m, O + a_ * e + 2 * x_ * m]
        else:
            rad, phi = np.linalg.norm(y), np.arctan2(y @ e, y @ m)
            trial = [O + s * rad * (np.cos(f * phi) * m + np.sin(f * phi) * e) for s, f in ((1, 2), (2, 1), (0.5, 1))]
        T = np.array(trial) + hgt * n
        _, r2 = m64.closest_point_on_triangle(*(np.repeat(N[i][k][None, :], len(T), 0) for k in range(3)), T)
        if (r2 != reg).any():
            bad.append((i, reg, r2.tolist()))
    return bad


# ------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("numbering", NUMBERINGS)
def test_triangle_zoo_design_holds(pkg, orc, numbering):
    """every designed row is listed by the oracle and none else, the masked ones are not; the float64 model gives every row its
    designed region and label; every class has 60 rows or more; every row is compared; the thresholds are cleared; the oracle's own
    error e_orc is 5e-6 at the most in every class that carries force"""
    z, c, ref, ro, e, own, lists = oracle_yardstick(numbering, "hertz")
    n = len(c["idA"])
    listed = list(zip(c["idA"].tolist(), c["idB"].tolist()))
    assert len(set(listed)) == n and set(listed) >= set(z.design), (n, len(z.design), sorted(set(z.design) - set(listed))[:5])
    assert not np.isin(c["idA"], z.masked).any() and len(z.masked) == N_MASKED
    assert n >= 2900
    # 'far': the sweep's directional test has no far side, so a sphere anywhere over or under a face is listed with it where the two
    # share a bin.  That happens between the four triangles of a small mesh and nowhere else; the force pass retires these rows
    far = c["label"] == "far"
    assert np.isin(c["ownerB"][far], z.small_meshes).all() and not ref["touching"][far].any()
    own_mesh = {int(a): int(o) for a, o, f_ in zip(c["idA"], c["ownerB"], far) if not f_}
    assert all(own_mesh[int(a)] == int(o) for a, o in zip(c["idA"][far], c["ownerB"][far]))
    assert ((ref["depth"][far] <= -10 * c["extra"][far]) | (ref["height"][far] <= -2 * c["rA"][far])).all()
    # regions and labels
    assert np.array_equal(ref["region"][~far], c["region"][~far]), np.nonzero(ref["region"] != c["region"])[0][:10]
    want = np.array([{"stick": "stick", "slip": "slip", "separating": "separating", "roll_on": "roll_on", "normal_only": "normal_only",
                      "margin": "margin", "apart": "apart"}[k] for k in c["cls"]], dtype=object)
    bad = np.nonzero(want != ref["label"])[0]
    assert len(bad) == 0, [(c["label"][i], ref["label"][i]) for i in bad[:10]]
    lab, h, r, d = c["label"], ref["height"], c["rA"], ref["depth"]
    counts = {cls: int((lab == cls).sum()) for cls in CLASSES}
    assert min(counts.values()) >= 60 and sum(counts.values()) == n, counts  # every row is in a class: the excluded share is zero
    for g in GEO7 + ("under",) + DEAD:
        assert sum(v for k, v in counts.items() if k.split("/")[0] == g) >= 60, g
    assert (ref["s"][~np.isin(lab, DEAD)] > 0).all() and not ref["s"][np.isin(lab, DEAD)].any()
    k = lab == "under"
    assert (ref["region"][k] == 0).all() and (h[k] < 0).all() and (h[k] > -r[k] / 2).all() and (d[k] > 1.3 * r[k]).all()
    k = lab == "deep_under"
    assert (ref["region"][k] == 0).all() and (h[k] <= -1.049 * r[k]).all() and (d[k] > 0).all() and not ref["touching"][k].any()
    assert ((h > -r / 2) | (h <= -1.049 * r)).all()
    for cls in LADDER:
        k, want_d = lab == cls, float(cls.split("depth_")[1])
        assert ((d[k] / r[k] > 0.5 * want_d) & (d[k] / r[k] < 2 * want_d)).all(), cls
    # thresholds: the margins (against the row's own extra margin), the region boundaries, ft against mu |Fn|, |v_rot|, the clocks
    assert ((d > 0) | ((d < 0) & (-d <= c["extra"] / 2)) | (-d >= 2 * c["extra"])).all()
    assert len(np.unique(c["extra"])) >= 2 and len(np.unique(c["extra_min"])) >= 3 and (c["extra"] != c["extra_min"]).any()
    assert not _doubled_offsets_keep_the_region(c, ref, ~far)
    live = ref["s"] > 0
    ft, fm = ref["ft"][live], ref["ft_max"][live]
    assert ((ft >= 2 * fm) | (ft <= fm / 2)).all() and ((ft >= 2 * m64.TINY) | (ft <= m64.TINY / 2)).all()
    vr = ref["vrot"][~np.isnan(ref["vrot"])]
    assert ((vr >= 2 * m64.TINY) | (vr <= m64.TINY / 2)).all()
    kk = ~np.isnan(ref["tc"])
    ratio = ref["clock"][kk] / ref["tc"][kk]
    assert kk.sum() >= 400 and ((ratio >= 2.0) | (ratio <= 0.5)).all()
    assert (np.abs(ref["d_coeff"][~np.isnan(ref["d_coeff"])] - 1.0) >= 0.05).all()
    # meshes, materials, radii, families
    A = z.builder.arrays
    q_id = (np.asarray(A["oriQw"]) == 1)
    assert len(z.large_meshes) >= 2 and q_id[z.large_meshes].all() and len(z.small_meshes) >= 20 and not q_id[z.small_meshes].any()
    assert len(z.free_meshes) >= 2
    for o in z.free_meshes:
        rows = (c["ownerB"] == o) & ~far
        assert rows.sum() >= 3 and live[rows].all() and np.abs(c["vB"][rows]).max() > 0 and np.abs(c["wB"][rows]).max() > 0
        assert not (np.asarray(A["familyFlags"])[int(A["familyID"][o])] & pkg.abi.FAMILY_FIXED)
    assert np.isin(c["ownerB"], z.small_meshes).sum() >= 150 and (np.bincount(c["ownerB"][live])[z.small_meshes] <= 4).all()
    seen = set(zip(c["matA"][live].tolist(), c["matB"][live].tolist()))
    assert seen == {(S0, T0), (S0, T1), (S1, T0), (S1, T1)}, seen
    assert set(np.round(r / R0).astype(int)) == {1, 12}
    # lever / overlap on the rotated meshes (the rounding of rot_apply_d's fp32 coefficients): 56 at the most where force is carried
    rot = np.isin(c["ownerB"], z.small_meshes) & live
    lever = np.linalg.norm(c["tri"], axis=2).max(1)
    assert (lever[rot] / d[rot] <= 56).all(), float((lever[rot] / d[rot]).max())
    # the triangles across bins, with contact points in another bin than the centre; the ridges: two rows a sphere
    lbf = np.array([float(z.params.LBFX), float(z.params.LBFY), float(z.params.LBFZ)])
    g = m64.geometry(c)
    binof = lambda x: np.floor((x - lbf) / float(z.params.binSize)).astype(np.int64)  # noqa: E731
    N = c["posB"][:, None, :] + np.einsum("nij,nkj->nki", g["RB"], c["tri"])
    for t in z.big_tris:
        rows = np.nonzero(c["idB"] == t)[0]
        assert len(rows) == 2
        assert ((binof(N[rows[0]].max(0)) - binof(N[rows[0]].min(0))) >= 2).all()
        assert all((binof(g["cp"][i]) != binof(c["posA"][i])).any() for i in rows)
    for s in z.ridge_spheres:
        rows = np.nonzero(c["idA"] == s)[0]
        assert len(rows) == 2 and sorted(ref["region"][rows]) == [4, 6] and live[rows].all()
    single = ~np.isin(c["idA"], z.ridge_spheres) & live  # isolation: one force-carrying row a sphere, two a triangle at the most
    assert (np.bincount(c["idA"][single], minlength=z.n_clumps) <= 1).all()
    assert np.bincount(c["idB"][live]).max() == 2
    # smallest angle
    for a_, b_, c_ in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        u, v = c["tri"][:, b_] - c["tri"][:, a_], c["tri"][:, c_] - c["tri"][:, a_]
        cosang = m64._dot(u, v) / (m64._len(u) * m64._len(v))
        assert (np.degrees(np.arccos(cosang)) >= 20).all()
    # the oracle's own error: 5e-6 in every class that carries force (half of CEILING; the largest entry of the existing zoo's table)
    worst = {cls: max(e[cls][q] for q in ("F", "T", "H", "W")) for cls in CLASSES}
    assert max(worst.values()) <= 5e-6, {k: v for k, v in worst.items() if v > 5e-6}
    # tile limits of this scene: four materials fit, the first table that does not is the untiled build's
    k4 = z.builder.counts
    table = lambda nm: k4["nComp"] * 16 + nm ** 2 * 32 + k4["nAnal"] * 64 + ((k4["nMassProps"] * 4 + 15) & ~15) + 1024  # noqa: E731
    assert k4["nMat"] == 4 and k4["nAnal"] == 0 and table(4) <= TILE_TABLE_MAX and k4["nComp"] + 2 * 16 <= 256
    assert table(untiled_materials(z)) > TILE_TABLE_MAX >= table(untiled_materials(z) - 1)


def untiled_materials(z):
    """the smallest number of materials whose tables no longer fit the tile pass, for this scene's nComp, nAnal and nMassProps"""
    k = z.builder.counts
    base = k["nComp"] * 16 + k["nAnal"] * 64 + ((k["nMassProps"] * 4 + 15) & ~15) + 1024
    nm = len(MATERIALS)
    while base + nm * nm * 32 <= TILE_TABLE_MAX and k["nComp"] + 2 * nm * nm + 4 * k["nAnal"] <= 256:
        nm += 1
    return nm


def test_model_triangle_geometry_against_the_elementwise_oracle(pkg, orc):
    """KIND_TRI of the float64 model against orc.tri_sphere (the restated triangle_sphere_CD, fp64 instantiation) on the zoo's own
    rows: the same decision, contact point to 1e-12 of the scene, depth and normal to the fp32 accuracy of the face normal"""
    z, c, ref, *_ = oracle_yardstick("spheres-first", "hertz")
    g = m64.geometry(c)
    N = c["posB"][:, None, :] + np.einsum("nij,nkj->nki", g["RB"], c["tri"])
    P = c["posA"] + m64._mv(g["RA"], c["relA"])
    hit, nr, depth, pt = orc.tri_sphere(N[:, 0], N[:, 1], N[:, 2], P, c["rA"])
    face = ref["region"] == 0
    in_contact = (ref["depth"] > 0) & (np.abs(ref["height"]) < c["rA"])
    assert np.array_equal(hit.astype(bool), in_contact)
    e_pt = np.abs(pt - g["cp"]).max()
    e_d_face = (np.abs(-depth - ref["depth"]) / np.maximum(np.abs(ref["height"]), c["rA"]))[face].max()  # (h carries the fp32 root)
    e_d_rest = np.abs(-depth - ref["depth"])[~face].max()
    e_n = np.abs(nr - ref["normal"]).max()
    record_measured("test_triangle_zoo model vs orc.tri_sphere", point=float(e_pt), depth_face_over_h=float(e_d_face),
                    depth_edge_vertex=float(e_d_rest), normal=float(e_n))
    assert e_pt <= 1e-12 and e_d_rest <= 1e-12 and e_d_face <= 3e-7 and e_n <= 3e-7
    assert np.bincount(ref["region"], minlength=7).min() >= 300


@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_float64_model_against_the_oracle_sim(pkg, orc, model, numbering):
    """the yardstick e_orc of both models and numberings, and the oracle's outputs on the dead classes"""
    z, c, ref, ro, e, own, _ = oracle_yardstick(numbering, model)
    for cls in CLASSES:
        record_measured(f"test_triangle_zoo e_orc {model} {numbering} {cls}", **{k: e[cls][k] for k in ("F", "T", "H", "W", "PA", "PBfar")})
        assert max(e[cls][k] for k in ("F", "T", "H", "W")) <= 5e-6, (cls, e[cls])
        assert e[cls]["PA"] <= 4 * U32 * max(e[cls]["Pmax"], R0) and e[cls]["PBfar"] <= 4 * U32 * max(e[cls]["PBfarmax"], R0), (cls, e[cls])
    record_measured(f"test_triangle_zoo e_orc {model} {numbering} per owner", a=own["e_a"], alpha=own["e_al"])
    assert own["e_a"] <= CEILING and own["e_al"] <= CEILING, own
    dead = np.isin(c["label"], DEAD)
    assert np.array_equal(~ro["F"].any(1), dead)
    assert np.array_equal(~ro["PA"].any(1), np.isin(c["label"], ("deep_under", "apart", "far")))
    if model == "hertz":
        assert not ro["hist"][dead].any() and c["hist"][dead].any(1).all()
        assert np.array_equal(ro["T"].any(1), c["cls"] == "roll_on")


# ------------------------------------------------------------------------------------------------------------ GPU tests
def _context(pkg, z, mode, record=True):
    ctx = pkg.Context(0)
    ctx.set_arith_mode(mode)
    ctx.set_reorder(False)
    ctx.set_params(z.params), ctx.upload_scene(z.scene)
    if record:
        ctx.set_record_contacts(True)
    return ctx


def _lists_equal(ctx, sim_lists, z):
    a, b, t = (np.asarray(x) for x in ctx.contacts()[:3])
    assert all(np.array_equal(x, y) for x, y in zip((a, b, t), sim_lists[:3])), "contact lists differ"
    rows = list(zip(a.tolist(), b.tolist()))
    assert (t == 2).all() and len(set(rows)) == len(rows) and set(rows) >= set(z.design)  # every designed row exactly once
    assert not np.isin(a, z.masked).any()                                                  # the masked class is absent


def _tri_loads_fails(ctx, z, c, rg):
    """inspect_tri_loads at threshold 0 (every listed row counts, the retired ones with a zero force) and at the shell's (the rows
    that carry a force): the fp64 sum of -F over the triangle's counted rows of the RECORDED F, and their count, exactly -- a
    triangle has two rows with a force at the most, and one fp64 addition of two fp32 values is the same in either order"""
    fails = []
    nT = int(z.builder.counts["nTri"])
    own = np.asarray(z.builder.arrays["ownerClumpBody"], np.int64)
    for thr in (0.0, 1e-12):
        want = tri_loads(c["idA"], c["idB"], np.full(len(c["idA"]), 2), rg["raw"][0], own, None, nT, thr)
        want_n, want_f = want["counts"], want["force"]
        force, counts = ctx.inspect_tri_loads(thr)
        if not np.array_equal(counts, want_n):
            fails.append(("tri loads: counts", thr, int((counts != want_n).sum())))
        if not np.array_equal(force, want_f):
            fails.append(("tri loads: force", thr, float(np.abs(force - want_f).max())))
        if thr and not (set(np.unique(want_n)) == {0, 1, 2}):
            fails.append(("tri loads: the zoo has triangles with 0, 1 and 2 rows that carry a force", np.unique(want_n).tolist()))
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_exact_mode_is_bit_identical_to_the_oracle(pkg, orc, model, numbering):
    """lists, records (F, T, PA, PB), the four wildcards and a / alpha of the spheres and of the small meshes, bit for bit; the large
    meshes (a thousand rows each) within the suite's 1e-3 tree bound; the triangle loads"""
    z, c, ref, ro, e, own, sim_lists = oracle_yardstick(numbering, model)
    ctx = _context(pkg, z, "exact")
    _, (rg,) = run_sides(pkg, z, [ctx], model)
    assert not ctx.engine_order()[0]
    _lists_equal(ctx, sim_lists, z)
    for k in range(4):
        assert np.array_equal(rg["raw"][k], ro["raw"][k]), ("record", k, int((rg["raw"][k] != ro["raw"][k]).any(1).sum()))
    if model == "hertz":
        assert np.array_equal(rg["hist"], ro["hist"])
    t = tight_owners(z)
    assert np.array_equal(rg["a"][t], ro["a"][t]) and np.array_equal(rg["al"][t], ro["al"][t])
    assert ro["a"][z.small_meshes].any() and ro["al"][z.small_meshes].any()
    assert (np.abs(rg["a"][~t] - ro["a"][~t]) <= 1e-3 * np.maximum(np.abs(ro["a"][~t]), 1e-6)).all()
    assert (np.abs(rg["al"][~t] - ro["al"][~t]) <= 1e-3 * np.maximum(np.abs(ro["al"][~t]), 1e-6)).all()
    fails = _tri_loads_fails(ctx, z, c, rg)
    ctx.close()
    assert not fails, fails


def _fast_bounds(e):
    return {cls: {q: min(FACTOR * max(e[cls][q], U32), CEILING) for q in ("F", "T", "H", "W")} for cls in CLASSES}


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["tiled", "untiled"])
@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_fast_mode_row_by_row(pkg, orc, model, numbering, build):
    """k_calc_forces<M, 1> over the sphere-mesh list and the pull of its records into the tile kernels (four materials) or the general
    kernels (one material past the table limit), against the float64 model: per row on the row's own scale, per owner on the owner's,
    with and without recording; the triangle loads"""
    z0 = build_zoo(numbering, model)
    extra = 0 if build == "tiled" else untiled_materials(z0) - len(MATERIALS)
    z, c, ref, ro, e, own, sim_lists = oracle_yardstick(numbering, model, extra)
    M = 0 if model == "hertz" else 1
    tight = tight_owners(z)
    ctx = _context(pkg, z, "fast")
    _, (rg,) = run_sides(pkg, z, [ctx], model)
    assert not ctx.engine_order()[0]
    name = ctx.force_kernel()[0]
    assert name == (f"k_tile_forces<{M}, true>" if build == "tiled" else f"k_calc_forces<{M}, 0>"), name
    _lists_equal(ctx, sim_lists, z)
    eg = class_errors(rg, ref, by_label(c), CLASSES)
    bounds = _fast_bounds(e)
    fails = []
    for cls in CLASSES:
        record_measured(f"test_triangle_zoo fast {build} {model} {numbering} {cls}",
                        **{k: eg[cls][k] for k in ("F", "T", "H", "W", "PA", "PBfar")}, **{"bound_" + k: bounds[cls][k] for k in ("F", "T", "H", "W")})
        for q in ("F", "T", "H", "W"):
            if eg[cls][q] > bounds[cls][q]:
                fails.append((cls, q, eg[cls][q], bounds[cls][q]))
        for q, mx in (("PA", "Pmax"), ("PBfar", "PBfarmax")):
            bp = FACTOR * max(e[cls][q], U32 * max(e[cls][mx], R0))
            if eg[cls][q] > bp:
                fails.append((cls, q, eg[cls][q], bp))
    dead = ref["s"] == 0
    assert not rg["F"][dead].any() and not rg["T"][dead].any()
    retired = ~ref["touching"]
    assert not rg["PA"][retired].any() and not rg["PB"][retired].any() and rg["PA"][~retired].any(1).all()
    if model == "hertz":
        assert not rg["hist"][dead].any()
    assert not rg["T"][~ref["T"].any(1)].any()
    tag = f"triangle zoo fast {build} {model} {numbering}"
    fails += _owner_fails(tag, rg, z, c, ref, own, tight)
    fails += _large_mesh_fails(tag, rg, z, own)
    fails += _tri_loads_fails(ctx, z, c, rg)
    ctx.close()
    # the kernels as a plain step runs them (no recording): history per class, sums per owner
    ctx = _context(pkg, z, "fast", record=False)
    ctx.set_margins(z.margins)
    ctx.detect()
    ctx.migrate()
    if model == "hertz":
        for w in range(4):
            ctx.set_wildcard(w, c["hist"][:, w].astype(np.float32))
    ctx.calc_forces()
    name = ctx.force_kernel()[0]
    assert name == (f"k_tile_forces<{M}, true>" if build == "tiled" else f"k_forces_fast<{M}>"), name
    _lists_equal(ctx, sim_lists, z)
    st = ctx.download_state()
    r2 = dict(a=np.stack([st[k] for k in ("aX", "aY", "aZ")], 1).astype(np.float64),
              al=np.stack([st[k] for k in ("alphaX", "alphaY", "alphaZ")], 1).astype(np.float64))
    if model == "hertz":
        h2 = np.stack([ctx.wildcard(w) for w in range(4)], 1).astype(np.float64)
        e2 = class_errors(dict(F=ref["F"], T=ref["T"], PA=ref["PA"], PB=ref["PB"], hist=h2), ref, by_label(c), CLASSES)
        assert not h2[dead].any()
        for cls in CLASSES:
            record_measured(f"test_triangle_zoo unrecorded {build} {numbering} {cls}", H=e2[cls]["H"], W=e2[cls]["W"])
            for q in ("H", "W"):
                if e2[cls][q] > bounds[cls][q]:
                    fails.append(("unrecorded", cls, q, e2[cls][q], bounds[cls][q]))
    tag = f"triangle zoo unrecorded {build} {model} {numbering}"
    fails += _owner_fails(tag, r2, z, c, ref, own, tight)
    fails += _large_mesh_fails(tag, r2, z, own)
    ctx.close()
    assert not fails, fails


def _large_mesh_fails(tag, rg, z, own):
    """a and alpha of the large meshes against the float64 sums, within the suite's 1e-3 tree bound of the owner's own scale"""
    o = z.large_meshes
    ea = np.abs(rg["a"][o] - own["a"][o]).max(1) / own["sa"][o]
    el = np.abs(rg["al"][o] - own["al"][o]).max(1) / own["sl"][o]
    record_measured(f"test_triangle_zoo {tag} large meshes", a=float(ea.max()), alpha=float(el.max()))
    return [(tag, "large mesh", float(ea.max()), float(el.max()))] if max(ea.max(), el.max()) > 1e-3 else []
