"""The contact zoo: ~2000 ISOLATED contacts, each of a known branch of the force model, each compared on its own scale with a plain
float64 statement of the model (tests/_contact_model64.py).

The bed tests bound the fast kernels by the largest force of a whole bed; a contact at 1 % of that may be 100 % wrong and pass.
Here every contact is alone (a lattice of pairs, spacing 96 small radii), sits on the position codec's integer lattice (exact
float64 positions), belongs to one branch class, and is measured against s = |k_n d| + |g_n v_n| + |k_t||d_t| + |g_t||v_t|.

Branch classes (the float64 model labels every contact; the zoo is built so that the label is the designed one):
  normal_only     axis-aligned normal, no tangential motion, zero history: the |tangential force| <= 1e-12 zeroing
  stick / slip    |tf| < / > mu |Fn| (slip: a large seeded history, clamped and rewritten from the clamped force)
  separating      |g_n v_n| > k_n d: Fn < 0, friction from |Fn|
  roll_young      Crr > 0, d_coeff < 1, seeded clock + h below t_collision / 2: no rolling resistance yet
  roll_on         the same with the clock at 3 t_collision;  roll_on_dcoeff: CoR 1e-4, d_coeff >= 1, on whatever the clock says
  roll_norot      rolling on, both angular velocities zero: no torque-only force
  margin          gap in (0, extra margin / 2]: touching, zero force, history cleared
  apart           gap >= 2 x extra margin: listed, zero force, history destroyed
  depth_1e-5, depth_1e-3, depth_1e-1   d / r across the range (centred spheres, sticking)
Geometry (mixed over the classes): equal spheres, radius ratios 1:3 and 1:12, one-component clumps off-centre by 0.5 and 2 radii,
dumbbells whose two components touch different partners, sphere-plane (the plane's owner 0.7 m away), sphere-cylinder inward and
outward.  Off-centre components carry the fp32 rounding of rot_apply(R, rel) (1e-10 m) into the overlap, so they are used with
d / r >= 0.03 only; the shallow classes use centred spheres.

Materials: the tile pass takes a scene only when its tables fit (nComp + 2 nMat^2 + 4 nAnal <= 256 sixteen-byte pieces, 4096 bytes
with the family margins), which keeps nMat within the 4-bit material fields of tInfo by itself.  With this zoo's 7 components, 3 analytical objects
and a family margin it allows NINE materials, and no scene with 16 can be tiled (2 x 16^2 = 512 pieces).  So the zoo has 9 materials
(7 for spheres, one for the plane, one for the cylinders; pairwise distinct E, nu, CoR, mu, Crr; ~20 pair overrides), every ordered
pair of sphere materials occurs in both roles, and the scene is built three times: 9 materials (tile kernels), 10 (the first table
that does not fit: general fast kernel) and 17 (beyond the 4-bit field of tInfo: general fast kernel).

Numberings (set_reorder(False): the engine keeps them): adjacent (partners consecutive: the local-B list), scattered (partners a
random permutation away: rec32 records and the integrator's gather), dumbbells-first (tile 0 = 128 dumbbells with 256 partners
elsewhere: its halo exceeds DEME_TILE_HMAX and it is evaluated by the per-tile fallback).

YARDSTICK.  e_orc[class] = the largest error of the ORACLE (the reference's fp32 arithmetic) against the float64 model, relative to s
(contact points: metres).  Measured on this zoo (hertz, the three numberings; frictionless is below these):
  class            force     torque-only  history   clock     PA / PB [m]  PB on a plane / cylinder owner [m]
  normal_only      1.5e-06   0            0         2.5e-08   6e-10        2.8e-08
  stick            3.6e-06   0            2.9e-08   6.7e-08   7e-10        2.8e-08
  slip             3.3e-06   0            5.8e-07   6.8e-08   1e-09        2.9e-08
  separating       1.4e-06   0            9.7e-08   6.7e-08   9e-10        2.7e-08
  roll_young       1.6e-07   0            1.7e-08   7.4e-08   1e-09        -
  roll_on          3.9e-06   1.8e-07      6.1e-08   6.4e-08   7e-10        2.9e-08
  roll_on_dcoeff   5.0e-06   4.9e-07      1.4e-08   2.5e-08   8e-10        3.0e-08
  roll_norot       3.4e-06   0            4.8e-08   6.4e-08   9e-10        2.9e-08
  margin / apart   0         0            0         0         1e-09 / 0    2.9e-08 / 0
  depth_1e-5       1.7e-07   0            7.3e-09   6.7e-08   1e-09        -
  depth_1e-3       1.7e-07   0            1.0e-08   6.7e-08   9e-10        -
  depth_1e-1       1.9e-06   0            3.3e-08   6.7e-08   8e-10        2.7e-08
  per owner: a 5.0e-06 of sum(s / m), alpha 2.3e-06 of sum(s |r| / MOI)
(the figures of every run go to measured_errors.txt through record_measured; the entries above 1e-6 belong to the off-centre clumps
and the planes: 1e-10 m of fp32 rounding -- of rot_apply(R, rel), of the plane distance -- in an overlap of 2e-5 m, times 3/2; the
centred classes sit at 2e-7.  Two input rules keep the yardstick there: shallow overlaps only between centred spheres, and a common
velocity of a pair no larger than its relative one -- 0.02 m/s in common puts 1e-9 m/s of fp32 rounding into a 6e-6 m/s approach.)  The tests take the table from the oracle run they make anyway.

FAST-MODE BOUND per class: FACTOR x max(e_orc[class], 2^-23) with FACTOR = 4, under the ceiling 1e-5 (the project's statement for
single contacts, tests/test_fast_mode.py).  Why 4: 1-ulp rcp / rsq / sqrt and FMA contraction along a dozen dependent operations
stay of the order of one fp32 evaluation, which is what e_orc measures; the floor 2^-23 is the fp32 unit roundoff, for classes in
which the oracle happens to be exact.  A wrong coefficient, branch, table entry or lever arm is wrong by 1e-2 s or more.  A torque-only
force that the float64 model does not have must be exactly zero.

ACHIEVED in fast mode on an MI355X (largest over the tile kernels with and without recording, the fallback tile, the general kernels,
both models, the three numberings); no class needed a factor above 4:
  class            force     torque-only  history   clock     PA / PB [m]  PB on a plane / cylinder owner [m]
  normal_only      1.6e-06   0            6.5e-15   2.5e-08   1.2e-09      2.8e-08
  stick            4.5e-06   0            4.3e-08   6.7e-08   7.9e-10      4.9e-08
  slip             4.1e-06   0            5.8e-07   6.8e-08   9.8e-10      4.1e-08
  separating       1.4e-06   0            9.7e-08   6.7e-08   9.2e-10      3.6e-08
  roll_young       2.1e-07   0            2.3e-08   7.4e-08   1.1e-09      -
  roll_on          4.0e-06   1.8e-07      6.2e-08   6.4e-08   9.1e-10      3.1e-08
  roll_on_dcoeff   5.2e-06   4.9e-07      1.4e-08   2.5e-08   9.2e-10      3.0e-08
  roll_norot       4.3e-06   0            4.8e-08   6.4e-08   8.9e-10      4.2e-08
  margin / apart   0         0            0         0         9.9e-10 / 0  4.5e-08 / 0
  depth_1e-5       2.5e-07   0            8.0e-09   6.7e-08   1.2e-09      -
  depth_1e-3       2.9e-07   0            1.0e-08   6.7e-08   9.6e-10      -
  depth_1e-1       2.0e-06   0            3.3e-08   6.7e-08   9.0e-10      3.7e-08
  per owner: a 5.2e-06, alpha 2.5e-06; equal and opposite: 0.35 (forces) and 0.05 (torques) of their bounds;
  fused step against the unfused one: velocities within the fp32 rounding of v + a h, 0.003 of the bound on the angular velocities.
MUTATIONS, each built and run once on an MI355X (not kept), of the tile kernels' tile_contact and of the law it calls, hertz_fast of
deme_force_fast.h (then still a copy inside tile_contact): the 9-material fast-mode cases of this file fail under every one of them
-- tile_contact's T.mat[matA * nMat + matA] (all six cases), hertz_fast's `hist.w <= t_collision` test dropped (the three hertz
cases: roll_young gets a torque-only force), tile_contact's tB negated (all six), B's component read through A's index (all six).  tests/test_fast_mode.py
and tests/test_fast_mode_features.py without this file: the first mutation passes all 17 tests (their beds have one material), the
second fails one (the recording test, whose bed has Crr = 0.05), the last two fail 13 and 14.
"""
import functools

import numpy as np
import pytest

from tests import _contact_model64 as m64
from tests.conftest import record_measured

R0 = 5e-4                 # the small radius
H = 5e-6
EXTRA = 2e-5              # family extra margin
MARGIN = 1e-4             # detection margin of every owner (set_margins): pairs up to 2 MARGIN - EXTRA apart are listed
RHO = 2600.0
U32 = 2.0 ** -23
FACTOR = 4.0
CEILING = 1e-5
N_SPH_MAT, MAT_PLANE, MAT_CYL = 7, 7, 8
CLASSES = ("normal_only", "stick", "slip", "separating", "roll_young", "roll_on", "roll_on_dcoeff", "roll_norot", "margin", "apart",
           "depth_1e-5", "depth_1e-3", "depth_1e-1")
LABEL_OF = {"depth_1e-5": "stick", "depth_1e-3": "stick", "depth_1e-1": "stick"}
NUMBERINGS = ("adjacent", "scattered", "dumbbells-first")
N_PER_CLASS = 150
N_DUMBBELLS = 132
CELL, CELL0, NCELL = 0.048, 0.06, 18   # lattice of pair centres: spacing 8 x the largest radius (12 R0 = 6 mm)

MATERIALS = [  # pairwise distinct; E low where t_collision must exceed 2 h
    {"E": 1.0e8, "nu": 0.30, "CoR": 0.60, "mu": 0.20, "Crr": 0.00},
    {"E": 4.0e6, "nu": 0.22, "CoR": 0.35, "mu": 0.30, "Crr": 0.05},
    {"E": 2.0e6, "nu": 0.34, "CoR": 0.80, "mu": 0.00, "Crr": 0.10},
    {"E": 6.0e7, "nu": 0.26, "CoR": 0.45, "mu": 0.40, "Crr": 0.00},
    {"E": 8.0e6, "nu": 0.38, "CoR": 0.70, "mu": 0.50, "Crr": 0.02},
    {"E": 3.0e7, "nu": 0.24, "CoR": 0.55, "mu": 0.25, "Crr": 0.00},
    {"E": 3.0e6, "nu": 0.32, "CoR": 0.40, "mu": 0.35, "Crr": 0.08},
    {"E": 5.0e7, "nu": 0.28, "CoR": 0.50, "mu": 0.45, "Crr": 0.00},   # the plane
    {"E": 2.0e7, "nu": 0.36, "CoR": 0.65, "mu": 0.15, "Crr": 0.06},   # the cylinders
]
OVERRIDES = [("CoR", 1, 4, 1e-4), ("CoR", 2, 6, 1e-4), ("CoR", 4, 4, 1e-4), ("CoR", 6, 8, 1e-4),  # d_coeff >= 1
             ("mu", 0, 5, 0.0), ("mu", 3, 6, 0.0), ("Crr", 1, 3, 0.0), ("Crr", 2, 5, 0.0), ("Crr", 0, 4, 0.0),
             ("CoR", 0, 3, 0.33), ("CoR", 3, 5, 0.77), ("CoR", 0, 7, 0.42), ("mu", 0, 3, 0.61), ("mu", 5, 7, 0.13),
             ("mu", 1, 2, 0.27), ("mu", 4, 6, 0.72), ("Crr", 1, 6, 0.11), ("Crr", 2, 4, 0.03), ("Crr", 6, 6, 0.09),
             ("Crr", 4, 8, 0.07), ("CoR", 5, 5, 0.58)]

# clump templates: (radii / R0, rel / R0, MOI factors)
TEMPLATES = [([1.0], [[0, 0, 0]], (1, 1, 1)), ([3.0], [[0, 0, 0]], (1, 1, 1)), ([12.0], [[0, 0, 0]], (1, 1, 1)),
             ([1.0], [[0.3, 0.4, 0.0]], (1.0, 1.3, 0.8)), ([1.0], [[1.2, -0.8, 1.36]], (2.0, 1.5, 2.5)),
             ([1.0, 1.0], [[3.0, 0, 0], [-3.0, 0, 0]], (1.0, 6.0, 6.0))]
T_DUMB = 5
# pair geometries on the lattice: (template of the first owner, of the second, centred)
PAIR_GEO = [(0, 0, True), (0, 1, True), (0, 2, True), (2, 2, True), (1, 2, True), (3, 0, False), (4, 3, False), (4, 1, False)]
# sphere against an analytical object: (template, object index, centred); objects: 0 plane, 1 post (outward), 2 drum (inward)
ANAL_GEO = [(0, 0, True), (1, 0, True), (3, 0, False), (0, 1, True), (3, 1, False), (0, 2, True), (4, 2, False)]
PLANE_Z, POST_XY, POST_R, DRUM_XY, DRUM_R = 0.012, (0.95, 0.5), 0.01, (0.5, 0.5), 0.70


def _pair_tables(n_mat):
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


def _tmpl_mass(t):
    return sum(RHO * 4.0 / 3.0 * np.pi * (r * R0) ** 3 for r in TEMPLATES[t][0])


class Zoo:
    pass


@functools.lru_cache(maxsize=None)
def build_zoo(numbering, model, extra_materials=0, seed=2031):
    """the scene (builder, params) plus, per sphere, the designed class; deterministic in its arguments"""
    import __graft_entry__ as entry
    pkg = entry.load_package()
    rng = np.random.default_rng(seed)
    tab = _pair_tables(len(MATERIALS))
    b = pkg.SceneBuilder()
    for mat in MATERIALS:
        b.LoadMaterial(mat)
    for _ in range(extra_materials):  # not used by any contact: only the size of the table changes
        b.LoadMaterial(dict(MATERIALS[0]))
    for name, a, c, val in OVERRIDES:
        b.SetMaterialPropertyPair(name, a, c, val)
    b.InstructBoxDomainDimension((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
    b.InstructBoxDomainBoundingBC("none", 0)
    b.SetInitTimeStep(H)
    b.SetGravitationalAcceleration((0, 0, -9.81))
    b.SetCDUpdateFreq(0)
    b.SetFamilyExtraMargin(0, EXTRA)
    if model == "frictionless":
        b.UseFrictionlessHertzianModel()
    tmpl = []
    for radii, rel, moif in TEMPLATES:
        mass = sum(RHO * 4.0 / 3.0 * np.pi * (r * R0) ** 3 for r in radii)
        lever2 = max(max(radii) ** 2 * 0.4, float((np.asarray(rel) ** 2).sum(1).max())) * R0 * R0
        tmpl.append(b.LoadClumpType(mass, tuple(mass * lever2 * f for f in moif), np.asarray(radii) * R0, np.asarray(rel) * R0, 0))
    b.AddBCPlane((0.5, 0.5, PLANE_Z), (0, 0, 1), MAT_PLANE)
    b.AddExternalObject().AddCylinder((POST_XY[0], POST_XY[1], 0.0), (0, 0, 1), POST_R, MAT_CYL, normal_inward=False)
    b.AddExternalObject().AddCylinder((DRUM_XY[0], DRUM_XY[1], 0.0), (0, 0, 1), DRUM_R, MAT_CYL, normal_inward=True)

    # ---- which (geometry, material pair) a class may use
    sph = range(N_SPH_MAT)

    def pairs_where(pred, b_mats=sph):
        return [(a, c) for a in sph for c in b_mats if pred(a, c)]

    def young_ok(geo_m, rA, rB):
        def pred(a, c):
            d, tc = m64.rolling_clock(tab["E_cnt"][a, c], tab["beta"][a, c], geo_m, rA, rB)
            return tab["Crr"][a, c] > 0 and d < 0.95 and tc >= 2.5 * H
        return pred
    no_roll = lambda a, c: tab["Crr"][a, c] == 0
    stickable = lambda a, c: tab["Crr"][a, c] == 0 and tab["mu"][a, c] > 0
    roll_lt1 = lambda a, c: tab["Crr"][a, c] > 0 and -np.sqrt(1.25) * tab["beta"][a, c] < 0.95
    roll_ge1 = lambda a, c: tab["Crr"][a, c] > 0 and -np.sqrt(1.25) * tab["beta"][a, c] > 1.05
    anyp = lambda a, c: True
    PRED = {"normal_only": no_roll, "stick": stickable, "slip": stickable, "separating": no_roll, "roll_on": roll_lt1,
            "roll_on_dcoeff": roll_ge1, "roll_norot": roll_lt1, "margin": anyp, "apart": anyp, "depth_1e-5": stickable,
            "depth_1e-3": stickable, "depth_1e-1": stickable}

    owners = []    # dicts: tmpl, pos (world, float64), q (wxyz fp32), v, w, mats (per component), cls (per component)
    groups = []    # owner indices that belong together (a pair, or a dumbbell with its two partners)
    cells = rng.permutation(NCELL ** 3)
    cell_i = [0]
    plane_spots = rng.permutation(53 * 53)
    spot_i = {0: 0, 1: 0, 2: 0}

    def next_cell():
        k = int(cells[cell_i[0]])
        cell_i[0] += 1
        return CELL0 + CELL * np.array([k % NCELL, (k // NCELL) % NCELL, k // (NCELL * NCELL)], np.float64)

    def rand_q():
        q = pkg.model.random_unit_quaternions(1, rng)[0]  # x y z w
        return np.array([q[3], q[0], q[1], q[2]], np.float32)

    def unit(v):
        return v / np.linalg.norm(v)

    def tangent(n):
        t = np.cross(n, rng.normal(size=3))
        return unit(t)

    def rotated(q, v):
        return m64.rot_matrix(q[None, :].astype(np.float64))[0] @ np.asarray(v, np.float64)

    def depth_for(cls, centred, r_small):
        if cls == "margin":
            return -rng.uniform(0.1, 0.5) * EXTRA
        if cls == "apart":
            return -rng.uniform(2.0, 4.0) * EXTRA
        if cls.startswith("depth_"):
            return float(cls[6:]) * r_small
        return r_small * (rng.uniform(1e-3, 1e-2) if centred else rng.uniform(0.03, 0.1))

    def motion(cls, n, a, c, mA, mB, rA, rB, depth, lever):
        """relative velocity of the first body against the second at the contact, and the size of the angular velocities"""
        if depth <= 0:
            return rng.normal(size=3) * 0.05, 5.0
        k_n, g_n, k_t, g_t, _ = m64.coefficients(tab["E_cnt"][a, c], tab["G_cnt"][a, c], tab["beta"][a, c], mA, mB, rA, rB, depth)
        Fn0 = k_n * depth
        mu = tab["mu"][a, c] if tab["mu"][a, c] > 0 else 1.0
        if cls == "separating":
            vn, Fn = 3.0 * Fn0 / abs(g_n), 2.0 * Fn0
        else:
            vn, Fn = -0.3 * Fn0 / abs(g_n), 1.3 * Fn0
        if cls == "normal_only":
            return vn * n, 0.0
        vt = 0.1 * mu * Fn / abs(g_t)
        return vn * n + vt * tangent(n), (0.0 if cls == "roll_norot" else 0.3 * vt / lever)

    def add_owner(t, centre_of_comp0, q, mats, cls):
        rel0 = np.asarray(TEMPLATES[t][1][0], np.float64) * R0
        owners.append(dict(tmpl=t, pos=np.asarray(centre_of_comp0) - rotated(q, rel0), q=q, v=np.zeros(3), w=np.zeros(3),
                           mats=list(mats), cls=list(cls)))
        return len(owners) - 1

    def lever_of(t):
        return (max(TEMPLATES[t][0]) + float(np.linalg.norm(TEMPLATES[t][1][0]))) * R0

    def rand_w(size):
        return unit(rng.normal(size=3)) * size if size else np.zeros(3)

    def make_pair(cls, geo, a, c):
        tA, tB, centred = PAIR_GEO[geo]
        rA, rB = TEMPLATES[tA][0][0] * R0, TEMPLATES[tB][0][0] * R0
        C = next_cell()
        n = np.eye(3)[rng.integers(3)] * rng.choice([-1.0, 1.0]) if cls == "normal_only" else unit(rng.normal(size=3))
        depth = depth_for(cls, centred, min(rA, rB))
        D = rA + rB - depth
        iA = add_owner(tA, C + n * D * rA / (rA + rB), rand_q(), [a], [cls])
        iB = add_owner(tB, C - n * D * rB / (rA + rB), rand_q(), [c], [cls])
        mA, mB = _tmpl_mass(tA), _tmpl_mass(tB)
        vrel, wsz = motion(cls, n, a, c, mA, mB, rA, rB, depth, max(lever_of(tA), lever_of(tB)))
        # (a common velocity far above the relative one would put its fp32 rounding into the damping terms)
        vcm = rng.normal(size=3) * 0.2 * np.linalg.norm(vrel) if cls != "normal_only" else np.zeros(3)
        owners[iA]["v"], owners[iB]["v"] = vcm + 0.5 * vrel, vcm - 0.5 * vrel
        owners[iA]["w"], owners[iB]["w"] = rand_w(wsz), rand_w(wsz)
        groups.append([iA, iB])

    def make_dumbbell(cls, mats3, partner_t):
        C, q = next_cell(), rand_q()
        comps = [np.asarray(r, np.float64) * R0 for r in TEMPLATES[T_DUMB][1]]
        iD = add_owner(T_DUMB, C + rotated(q, comps[0]), q, [mats3[0], mats3[0]], [cls, cls])
        mD = _tmpl_mass(T_DUMB)
        g, wmin = [iD], None
        for k in range(2):
            tP = partner_t[k]
            rP = TEMPLATES[tP][0][0] * R0
            axis = unit(rotated(q, comps[k]))
            n = unit(axis + 0.4 * tangent(axis))  # from the component to its partner
            depth = depth_for(cls, False, R0)
            iP = add_owner(tP, C + rotated(q, comps[k]) + n * (R0 + rP - depth), rand_q(), [mats3[1 + k]], [cls])
            vrel, wsz = motion(cls, -n, mats3[0], mats3[1 + k], mD, _tmpl_mass(tP), R0, rP, depth, 4.0 * R0)
            owners[iP]["v"], owners[iP]["w"] = -vrel, rand_w(wsz)  # the dumbbell's centre is at rest
            wmin = wsz if wmin is None else min(wmin, wsz)
            g.append(iP)
        owners[iD]["w"] = rand_w(0.2 * wmin)
        groups.append(g)

    def make_anal(cls, geo, a):
        t, obj, centred = ANAL_GEO[geo]
        rA = TEMPLATES[t][0][0] * R0
        depth = depth_for(cls, centred and obj != 0, rA)  # (a plane rounds its distance to fp32: 6e-11 m at r = 1 mm)
        if obj == 0:
            k = int(plane_spots[spot_i[0]])
            centre = np.array([0.06 + 0.016 * (k % 53), 0.06 + 0.016 * (k // 53), PLANE_Z + rA - depth])
            n = np.array([0.0, 0.0, 1.0])
        else:
            k = spot_i[obj]
            z = 0.06 + 0.012 * (k // 8 if obj == 1 else k // 4)
            if obj == 1:
                th = (k % 8) * np.pi / 4 + 0.1
                n = np.array([np.cos(th), np.sin(th), 0.0])
                centre = np.array([POST_XY[0], POST_XY[1], z]) + n * (POST_R + rA - depth)
            else:
                th = (k % 4) * np.pi / 2 + np.pi / 4 + rng.uniform(-0.008, 0.008)
                out = np.array([np.cos(th), np.sin(th), 0.0])
                centre = np.array([DRUM_XY[0], DRUM_XY[1], z]) + out * (DRUM_R - rA + depth)
                n = -out
        spot_i[obj] += 1
        c = MAT_PLANE if obj == 0 else MAT_CYL
        iA = add_owner(t, centre, rand_q(), [a], [cls])
        vrel, wsz = motion(cls, n, a, c, _tmpl_mass(t), 1e6, rA, m64.HUGE_RADIUS, depth, lever_of(t))
        owners[iA]["v"], owners[iA]["w"] = vrel, rand_w(wsz)
        groups.append([iA])

    n_dumb_per_class = {c: 0 for c in CLASSES}
    dumb_classes = [c for c in CLASSES if c not in ("normal_only", "depth_1e-5", "depth_1e-3", "roll_young")]
    for k in range(N_DUMBBELLS):
        n_dumb_per_class[dumb_classes[k % len(dumb_classes)]] += 1
    for cls in CLASSES:
        shallow = cls in ("depth_1e-5", "depth_1e-3")
        if cls == "roll_young":  # needs t_collision >= 2.5 h: the heavy pairs and the soft materials
            combos = []
            for geo in (3, 4):
                tA, tB, _ = PAIR_GEO[geo]
                mA, mB = _tmpl_mass(tA), _tmpl_mass(tB)
                pr = young_ok(mA * mB / (mA + mB), TEMPLATES[tA][0][0] * R0, TEMPLATES[tB][0][0] * R0)
                combos += [("pair", geo, a, c) for a, c in pairs_where(pr)]
            assert len(combos) >= 8
        else:
            pp = pairs_where(PRED[cls])
            geos = [g for g in range(len(PAIR_GEO)) if PAIR_GEO[g][2] or not (shallow or cls == "normal_only")]
            combos = [("pair", geos[(i + j) % len(geos)], a, c) for j in range(2) for i, (a, c) in enumerate(pp)]
            ageos = [g for g in range(len(ANAL_GEO)) if ((ANAL_GEO[g][2] and ANAL_GEO[g][1] == 0) if cls == "normal_only" else
                                                         ((ANAL_GEO[g][2] and ANAL_GEO[g][1] != 0) or not shallow))]
            for g in ageos:
                cm = MAT_PLANE if ANAL_GEO[g][1] == 0 else MAT_CYL
                combos += [("anal", g, a, cm) for a in sph if PRED[cls](a, cm)]
        order = rng.permutation(len(combos))
        n_single = N_PER_CLASS - 2 * n_dumb_per_class[cls]
        for k in range(n_single):
            kind, geo, a, c = combos[int(order[k % len(order)])]
            if kind == "pair":
                make_pair(cls, geo, a, c)
            else:
                make_anal(cls, geo, a)
        pp = pairs_where(PRED[cls]) if cls != "roll_young" else []
        for k in range(n_dumb_per_class[cls]):
            a, c = pp[int(rng.integers(len(pp)))]
            c2 = [x for (y, x) in pp if y == a][int(rng.integers(len([1 for (y, x) in pp if y == a])))]
            make_dumbbell(cls, (a, c, c2), (int(rng.integers(2)), 0))

    # ---- numbering
    n_own = len(owners)
    if numbering == "adjacent":
        order = [i for g in groups for i in g]
    elif numbering == "scattered":
        order = list(rng.permutation(n_own))
    else:  # the first 128 owners are dumbbells; their partners follow after everything else
        dumb = [g for g in groups if owners[g[0]]["tmpl"] == T_DUMB]
        first = dumb[:128]
        rest = [g for g in groups if not any(g is d for d in first)]
        order = [g[0] for g in first] + [i for g in rest for i in g] + [i for g in first for i in g[1:]]
    assert sorted(order) == list(range(n_own))
    owners = [owners[i] for i in order]
    batch = b.AddClumps([tmpl[o["tmpl"]] for o in owners], np.array([o["pos"] for o in owners], np.float32))
    p, sc = b.Initialize()
    A = b.arrays
    # positions on the codec's lattice, exactly; orientation, velocities; per-sphere materials
    lbf = np.array([float(p.LBFX), float(p.LBFY), float(p.LBFZ)])
    G = np.rint((np.array([o["pos"] for o in owners]) - lbf) / p.l).astype(np.int64)
    vox = G // 65536
    A["voxelID"][:n_own] = (vox[:, 0] + (vox[:, 1] << p.nvXp2) + (vox[:, 2] << (p.nvXp2 + p.nvYp2))).astype(np.uint64)
    for k, name in enumerate(("locX", "locY", "locZ")):
        A[name][:n_own] = (G[:, k] % 65536).astype(np.uint16)
    Q = np.array([o["q"] for o in owners], np.float32)
    for k, name in enumerate(("oriQw", "oriQx", "oriQy", "oriQz")):
        A[name][:n_own] = Q[:, k]
    V, W = np.array([o["v"] for o in owners], np.float32), np.array([o["w"] for o in owners], np.float32)
    for k in range(3):
        A[("vX", "vY", "vZ")[k]][:n_own] = V[:, k]
        A[("omgBarX", "omgBarY", "omgBarZ")[k]][:n_own] = W[:, k]
    mats = np.array([x for o in owners for x in o["mats"]], np.uint16)
    assert len(mats) == len(A["sphereMaterialOffset"])
    A["sphereMaterialOffset"][:] = mats
    z = Zoo()
    z.builder, z.params = b, p
    z.scene = pkg.abi.make_scene_struct(A, b.counts)
    z.cls_of_sphere = np.array([x for o in owners for x in o["cls"]], dtype=object)
    z.n_clumps = n_own
    z.tables = _pair_tables(len(MATERIALS) + extra_materials)
    z.margins = np.full(int(b.counts["nOwners"]), MARGIN, np.float32)
    return z


def positions64(pkg, z, st=None):
    A, p = (st if st is not None else z.builder.arrays), z.params
    X = pkg.model.decode_positions(A["voxelID"], A["locX"], A["locY"], A["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    return X + np.array([float(p.LBFX), float(p.LBFY), float(p.LBFZ)])[None, :]


def gather_inputs(pkg, z, contacts, hist):
    """the float64 model's inputs for the listed contacts (sphere A, sphere B or object index, type), from the scene arrays"""
    A = z.builder.arrays
    idA, idB, typ = (np.asarray(x) for x in contacts[:3])
    f = lambda k: np.asarray(A[k], np.float64)
    ss = typ == 1
    own = np.asarray(A["ownerClumpBody"], np.int64)
    oA = own[idA]
    sB, ob = np.where(ss, idB, 0), np.where(ss, 0, idB)
    oB = np.where(ss, own[sB], np.asarray(A["objOwner"], np.int64)[ob])
    X = positions64(pkg, z)
    Q = np.stack([f("oriQw"), f("oriQx"), f("oriQy"), f("oriQz")], 1)
    V, W = np.stack([f("vX"), f("vY"), f("vZ")], 1), np.stack([f("omgBarX"), f("omgBarY"), f("omgBarZ")], 1)
    mass = f("MassProperties")[np.asarray(A["inertiaPropOffsets"], np.int64)]
    moi = np.stack([f("moiX"), f("moiY"), f("moiZ")], 1)[np.asarray(A["inertiaPropOffsets"], np.int64)]
    comp = np.asarray(A["clumpComponentOffset"], np.int64)
    rel = np.stack([f("CDRelPosX"), f("CDRelPosY"), f("CDRelPosZ")], 1)
    orel = np.stack([f("objRelPosX"), f("objRelPosY"), f("objRelPosZ")], 1)
    odir = np.stack([f("objRotX"), f("objRotY"), f("objRotZ")], 1)
    smat = np.asarray(A["sphereMaterialOffset"], np.int64)
    mA_, mB_ = smat[idA], np.where(ss, smat[sB], np.asarray(A["objMaterial"], np.int64)[ob])
    T = z.tables
    kind = np.where(ss, m64.KIND_SPHERE, np.where(typ == 11, m64.KIND_PLANE, m64.KIND_CYL))
    c = dict(posA=X[oA], posB=X[oB], qA=Q[oA], qB=Q[oB], vA=V[oA], vB=V[oB], wA=W[oA], wB=W[oB], mA=mass[oA],
             mB=np.where(ss, mass[oB], f("objMass")[ob]), relA=rel[comp[idA]], rA=f("Radii")[comp[idA]], kind=kind,
             relB=np.where(ss[:, None], rel[comp[sB]], orel[ob]), rB=np.where(ss, f("Radii")[comp[sB]], m64.HUGE_RADIUS),
             dirB=odir[ob], sizeB=f("objSize1")[ob], signB=f("objNormal")[ob], E_cnt=T["E_cnt"][mA_, mB_], G_cnt=T["G_cnt"][mA_, mB_],
             beta=T["beta"][mA_, mB_], mu=T["mu"][mA_, mB_], Crr=T["Crr"][mA_, mB_], hist=np.asarray(hist, np.float64),
             extra=np.full(len(idA), float(np.float32(EXTRA))))
    c.update(ownerA=oA, ownerB=oB, matA=mA_, matB=mB_, mass=mass, moi=moi, cls=z.cls_of_sphere[idA])
    return c


def design_history(c, seed=5):
    """the history each contact goes in with (fp32), by its designed class; a function of the list alone"""
    rng = np.random.default_rng(seed)
    n = len(c["rA"])
    c0 = dict(c, hist=np.zeros((n, 4)))
    o = m64.contact64(c0, H)
    Fn = np.abs(m64._dot(o["F"], o["normal"]))
    t = np.cross(o["normal"], rng.normal(size=(n, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    mu = np.where(c["mu"] > 0, c["mu"], 1.0)
    cls = c["cls"]
    with np.errstate(divide="ignore", invalid="ignore"):
        size = np.where(cls == "slip", 5.0, 0.3) * mu * Fn / o["kt"]
    size = np.where(np.isin(cls, ("margin", "apart")), 1e-7, np.where(o["kt"] > 0, size, 0.0))
    size[cls == "normal_only"] = 0.0
    hist = np.zeros((n, 4))
    hist[:, :3] = t * size[:, None]
    clock = rng.uniform(1e-5, 3e-5, n)
    tc = np.nan_to_num(o["tc"], nan=0.0)
    u = rng.uniform(0.0, 0.9, n)
    clock = np.where(cls == "roll_young", u * np.maximum(tc / 2.0 - H, 0.0), clock)
    clock = np.where(np.isin(cls, ("roll_on", "roll_norot")), 3.0 * tc, clock)
    clock[cls == "roll_on_dcoeff"] = 0.0
    clock[cls == "normal_only"] = 0.0
    hist[:, 3] = clock
    return hist.astype(np.float32)


def class_errors(x, ref, c, classes=CLASSES):
    """per designed class: the largest |x - ref| relative to the contact's scale s (contact points: metres).  x: dict with F, T,
    PA, PB and, for the full model, hist"""
    s = ref["s"]
    live = s > 0
    out = {}
    far = c["kind"] != m64.KIND_SPHERE
    with np.errstate(divide="ignore", invalid="ignore"):
        eF = np.abs(x["F"] - ref["F"]).max(1) / s
        eT = np.abs(x["T"] - ref["T"]).max(1) / s
        eH = eW = np.zeros(len(s))
        if "hist" in x:
            eH = ref["kt"] * np.abs(x["hist"][:, :3] - ref["hist"][:, :3]).max(1) / s
            eW = np.abs(x["hist"][:, 3] - ref["hist"][:, 3]) / np.maximum(ref["hist"][:, 3], H)
    ePA = np.abs(x["PA"] - ref["PA"]).max(1)
    ePB = np.abs(x["PB"] - ref["PB"]).max(1)
    for cls in classes:
        k = c["cls"] == cls
        kl = k & live
        g = lambda e, m: float(e[m].max()) if m.any() else 0.0
        out[cls] = dict(F=g(eF, kl), T=g(eT, kl), H=g(eH, kl), W=g(eW, kl), PA=g(ePA, k), PB=g(ePB, k & ~far), PBfar=g(ePB, k & far),
                        Pmax=g(np.abs(ref["PA"]).max(1), k), PBmax=g(np.abs(ref["PB"]).max(1), k & ~far),
                        PBfarmax=g(np.abs(ref["PB"]).max(1), k & far))
    return out


def run_sides(pkg, z, sides, model):
    """One call sequence for every side (contexts and oracle sims): detect, migrate, seed the history, one force evaluation.
    Returns the float64 inputs and the per-side results.  (A zoo of another module brings its own gather_inputs.)"""
    for s in sides:
        s.set_margins(z.margins)
        s.detect()
        s.migrate()
    lists = [s.contacts() for s in sides]
    for l in lists[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(l[:3], lists[0][:3])), "contact lists differ"
    c = getattr(z, "gather_inputs", gather_inputs)(pkg, z, lists[0], np.zeros((len(lists[0][0]), 4)))
    hist = design_history(c) if model == "hertz" else np.zeros((len(lists[0][0]), 4), np.float32)
    c["hist"] = hist.astype(np.float64)
    res = []
    for s in sides:
        if model == "hertz":
            for w in range(4):
                s.set_wildcard(w, hist[:, w])
        if hasattr(s, "set_record_contacts"):
            s.calc_forces()
        else:
            s.calc_forces(record=True)
        F, T, PA, PB = (np.asarray(a, np.float64) for a in s.contact_records())
        r = dict(F=F, T=T, PA=PA, PB=PB, raw=(F, T, PA, PB))
        if model == "hertz":
            r["hist"] = np.stack([s.wildcard(w) for w in range(4)], 1).astype(np.float64)
        st = s.download_state()
        r["a"] = np.stack([st[k] for k in ("aX", "aY", "aZ")], 1).astype(np.float64)
        r["al"] = np.stack([st[k] for k in ("alphaX", "alphaY", "alphaZ")], 1).astype(np.float64)
        res.append(r)
    return c, res


@functools.lru_cache(maxsize=None)
def oracle_yardstick(numbering, model, extra_materials=0):
    """the oracle's run of the zoo and its errors against the float64 model (e_orc), computed once per scene"""
    import __graft_entry__ as entry
    pkg, orc = entry.load_package(), entry.load_oracle()
    z = build_zoo(numbering, model, extra_materials)
    sim = orc.make_sim(pkg, z.params, z.scene)
    c, (ro,) = run_sides(pkg, z, [sim], model)
    ref = m64.contact64(c, H, model)
    e = class_errors(ro, ref, c)
    nO = int(z.builder.counts["nOwners"])
    a, al, cA, cB, sa, sl = m64.owner_sums64(ref, c["ownerA"], c["ownerB"], nO, c["mass"], c["moi"], c["mB"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ea = np.where(sa > 0, np.abs(ro["a"] - a).max(1) / sa, 0.0)[:z.n_clumps]
        el = np.where(sl > 0, np.abs(ro["al"] - al).max(1) / sl, 0.0)[:z.n_clumps]
    own = dict(a=a, al=al, sa=sa, sl=sl, cA=cA, cB=cB, e_a=float(ea.max()), e_al=float(el.max()))
    sim_lists = sim.contacts()
    sim.close()
    return z, c, ref, ro, e, own, sim_lists


# ------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("numbering", NUMBERINGS)
def test_zoo_design_holds_in_the_float64_model(pkg, orc, numbering):
    """every designed class is what the float64 model labels the contact, every class has >= 60 contacts, every contact is compared
    (none excluded), every discontinuous threshold is cleared by a factor 2, every ordered pair of sphere materials carries force in
    both roles"""
    z, c, ref, ro, e, own, lists = oracle_yardstick(numbering, "hertz")
    n = len(c["cls"])
    assert n >= 1900 and n == len(ref["label"])
    want = np.array([LABEL_OF.get(k, k) for k in c["cls"]], dtype=object)
    bad = np.nonzero(want != ref["label"])[0]
    assert len(bad) == 0, [(c["cls"][i], ref["label"][i]) for i in bad[:10]]
    for cls in CLASSES:
        assert (c["cls"] == cls).sum() >= 60, cls
    live = ref["s"] > 0
    dr = ref["depth"] / np.minimum(c["rA"], c["rB"])
    for cls, lo, hi in (("depth_1e-5", 0.5e-5, 2e-5), ("depth_1e-3", 0.5e-3, 2e-3), ("depth_1e-1", 0.5e-1, 2e-1)):
        k = c["cls"] == cls
        assert (dr[k] > lo).all() and (dr[k] < hi).all(), cls
    # thresholds: the two margins, 1e-12 on |tf| and |v_rot|, t_collision, d_coeff
    d = ref["depth"]
    assert ((d > 0) | ((d < 0) & (-d <= EXTRA / 2)) | (-d >= 2 * EXTRA)).all()
    ft = ref["ft"][live & ~np.isnan(ref["ft"])]
    assert ((ft >= 2 * m64.TINY) | (ft <= m64.TINY / 2)).all()
    vr = ref["vrot"][~np.isnan(ref["vrot"])]
    assert ((vr >= 2 * m64.TINY) | (vr <= m64.TINY / 2)).all()
    k = ~np.isnan(ref["tc"])
    ratio = ref["clock"][k] / ref["tc"][k]
    assert ((ratio >= 2.0) | (ratio <= 0.5)).all(), (ratio.min(), ratio.max())
    dc = ref["d_coeff"][~np.isnan(ref["d_coeff"])]
    assert (np.abs(dc - 1.0) >= 0.05).all() and (dc > 1).sum() >= 60  # (d_coeff = -sqrt(5/4) beta <= 1.118: no factor 2 to be had)
    assert ((c["Crr"] > 0) & live).sum() > 500 and ((c["mu"] == 0) & live).sum() > 10
    # materials: every ordered pair of sphere materials, both roles, on force-carrying contacts; plane and cylinders their own
    ss = (c["kind"] == m64.KIND_SPHERE) & live
    seen = set(zip(c["matA"][ss].tolist(), c["matB"][ss].tolist()))
    missing = [(a, b) for a in range(N_SPH_MAT) for b in range(N_SPH_MAT) if (a, b) not in seen]
    assert not missing, missing
    assert set(c["matB"][c["kind"] == m64.KIND_PLANE]) == {MAT_PLANE} and set(c["matB"][c["kind"] == m64.KIND_CYL]) == {MAT_CYL}
    assert (c["kind"] == m64.KIND_PLANE).sum() > 100 and ((c["kind"] == m64.KIND_CYL) & (c["signB"] > 0)).sum() > 50
    assert ((c["kind"] == m64.KIND_CYL) & (c["signB"] < 0)).sum() > 50
    # isolation: every sphere is in exactly one contact
    A = z.builder.arrays
    cnt = np.bincount(np.r_[lists[0], lists[1][c["kind"] == m64.KIND_SPHERE]], minlength=len(A["ownerClumpBody"]))
    assert (cnt == 1).all()
    if numbering == "adjacent":  # a pair across a tile boundary (128 owners per tile), and a last partial tile
        assert (c["ownerA"][c["kind"] == m64.KIND_SPHERE] // 128 != c["ownerB"][c["kind"] == m64.KIND_SPHERE] // 128).any()
        assert int(z.builder.counts["nOwners"]) % 128 != 0
    # tile limits of the 9-material scene, and the two builds that leave them
    k9 = z.builder.counts
    pieces = lambda cc: cc["nComp"] + 2 * cc["nMat"] ** 2 + 4 * cc["nAnal"]
    table = lambda cc: cc["nComp"] * 16 + cc["nMat"] ** 2 * 32 + cc["nAnal"] * 64 + ((cc["nMassProps"] * 4 + 15) & ~15) + 1024
    assert k9["nMat"] == 9 and pieces(k9) <= 256 and table(k9) <= 4096
    k10 = dict(k9, nMat=10)
    assert table(k10) > 4096


def test_float64_model_against_the_elementwise_oracle(pkg, orc):
    """orc.force (the force model alone, fp32 reference arithmetic) on the zoo's own inputs, rounded to fp32"""
    z, c, ref, *_ = oracle_yardstick("adjacent", "hertz")
    n = len(c["rA"])
    A = z.builder.arrays
    E, nu = np.asarray(A["E"], np.float32), np.asarray(A["nu"], np.float32)
    nM = len(E)
    fin = np.zeros((n, orc.FORCE_NF), np.float32)
    fin[:, 0:3] = ref["normal"]
    fin[:, 3], fin[:, 4], fin[:, 5], fin[:, 6] = c["mA"], c["mB"], c["rA"], c["rB"]
    fin[:, 7:11], fin[:, 11:15] = c["qA"], c["qB"]
    g = m64.geometry(c)
    PA, PB = m64._mtv(g["RA"], g["cp"] - c["posA"]), m64._mtv(g["RB"], g["cp"] - c["posB"])
    fin[:, 15:18], fin[:, 18:21] = PA, PB
    fin[:, 21:24], fin[:, 24:27], fin[:, 27:30], fin[:, 30:33] = c["vA"], c["vB"], c["wA"], c["wB"]
    fin[:, 33] = H
    fin[:, 34], fin[:, 35], fin[:, 36], fin[:, 37] = E[c["matA"]], nu[c["matA"]], E[c["matB"]], nu[c["matB"]]
    fin[:, 38] = np.asarray(A["CoR"], np.float32).reshape(nM, nM)[c["matA"], c["matB"]]
    for model, code in (("hertz", 0), ("frictionless", 1)):
        r64 = ref if model == "hertz" else m64.contact64(c, H, model)
        depth = np.where(r64["touching"], r64["depth"], -1.0)
        hout, out = orc.force("orc", code, depth, fin, c["mu"], c["Crr"], c["hist"])
        x = dict(F=out[:, :3].astype(np.float64), T=out[:, 3:].astype(np.float64), PA=r64["PA"], PB=r64["PB"])
        if model == "hertz":
            x["hist"] = hout.astype(np.float64)
        e = class_errors(x, r64, c)
        worst = {q: max(e[k][q] for k in CLASSES) for q in ("F", "T", "H", "W")}
        record_measured(f"test_contact_zoo elementwise oracle vs float64 ({model})", **worst)
        assert max(worst.values()) <= CEILING, worst
        dead = r64["s"] == 0
        assert not x["F"][dead].any() and not x["T"][dead].any()
        if model == "hertz":
            assert not x["hist"][dead].any()


@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_float64_model_against_the_oracle_sim(pkg, orc, model, numbering):
    """the whole zoo through OracleSim: records, history, a / alpha.  This is the yardstick e_orc; no entry may exceed 1e-5 (a few
    fp32 ulps times the length of the operation chain), and the oracle's outputs imply the float64 model's branch label"""
    z, c, ref, ro, e, own, _ = oracle_yardstick(numbering, model)
    for cls in CLASSES:
        record_measured(f"test_contact_zoo e_orc {model} {numbering} {cls}", **{k: e[cls][k] for k in ("F", "T", "H", "W", "PA", "PB", "PBfar")})
        assert max(e[cls][k] for k in ("F", "T", "H", "W")) <= CEILING, (cls, e[cls])
        assert e[cls]["PA"] <= 4 * U32 * max(e[cls]["Pmax"], R0) and e[cls]["PB"] <= 4 * U32 * max(e[cls]["PBmax"], R0), (cls, e[cls])
        assert e[cls]["PBfar"] <= 4 * U32 * max(e[cls]["PBfarmax"], R0), (cls, e[cls])
    record_measured(f"test_contact_zoo e_orc {model} {numbering} per owner", a=own["e_a"], alpha=own["e_al"])
    assert own["e_a"] <= CEILING and own["e_al"] <= CEILING, own
    # branch labels from the oracle's outputs alone
    lab = ref["label"]
    zeroF = ~ro["F"].any(1)
    assert np.array_equal(zeroF, np.isin(lab, ("margin", "apart")))
    assert np.array_equal(~ro["PA"].any(1), lab == "apart")
    if model == "hertz":
        assert np.array_equal(ro["T"].any(1), np.isin(lab, ("roll_on", "roll_on_dcoeff")))
        assert not ro["hist"][zeroF].any()
        n_ = ref["normal"]
        Fn = np.abs(m64._dot(ro["F"], n_))
        Ft = np.linalg.norm(ro["F"] - m64._dot(ro["F"], n_)[:, None] * n_, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            clamped = np.abs(Ft / (c["mu"] * Fn) - 1.0) < 1e-4
        assert clamped[lab == "slip"].all() and not clamped[np.isin(lab, ("stick", "normal_only"))].any()
        assert (ro["hist"][~zeroF, 3] > 0).all()


# ------------------------------------------------------------------------------------------------------------ GPU tests
def _context(pkg, z, mode, fused=False):
    ctx = pkg.Context(0)
    ctx.set_arith_mode(mode)
    ctx.set_reorder(False)
    if fused:
        ctx.set_fused_step(True)
    ctx.set_params(z.params), ctx.upload_scene(z.scene)
    ctx.set_record_contacts(True)
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_exact_mode_is_bit_identical_to_the_oracle(pkg, orc, model, numbering):
    """lists, records (F, T, PA, PB), the four wildcards and a / alpha of every owner: the first bit-level check of Crr > 0, of a table
    of 9 materials with overrides and of the two margin classes"""
    z, c, ref, ro, e, own, sim_lists = oracle_yardstick(numbering, model)
    ctx = _context(pkg, z, "exact")
    _, (rg,) = run_sides(pkg, z, [ctx], model)
    assert not ctx.engine_order()[0]
    assert all(np.array_equal(a, b) for a, b in zip(ctx.contacts()[:3], sim_lists[:3]))
    for k in range(4):
        assert np.array_equal(rg["raw"][k], ro["raw"][k]), ("record", k)
    if model == "hertz":
        assert np.array_equal(rg["hist"], ro["hist"])
    n = z.n_clumps  # (every clump has at most two contacts; the plane and cylinder owners are heavy: the tree's bound)
    assert np.array_equal(rg["a"][:n], ro["a"][:n]) and np.array_equal(rg["al"][:n], ro["al"][:n])
    assert (np.abs(rg["a"][n:] - ro["a"][n:]) <= 1e-3 * np.maximum(np.abs(ro["a"][n:]), 1e-6)).all()
    assert (np.abs(rg["al"][n:] - ro["al"][n:]) <= 1e-3 * np.maximum(np.abs(ro["al"][n:]), 1e-6)).all()
    ctx.close()


def _fast_bounds(e):
    """per class and quantity: FACTOR x max(e_orc, 2^-23), under the ceiling"""
    return {cls: {q: min(FACTOR * max(e[cls][q], U32), CEILING) for q in ("F", "T", "H", "W")} for cls in CLASSES}


def _owner_fails(tag, rg, z, c, ref, own, tight=None):
    """a / alpha per owner against the float64 sums, relative to the owner's own sum of s / m (s |r| / MOI); and, for
    every contact, A's and B's contributions equal and opposite.  tight: the owners held to the per-owner bound (default: the
    clumps); the others sum hundreds of terms and keep the suite's 1e-3 tree bound"""
    fails = []
    n = z.n_clumps
    if tight is None:
        tight = np.arange(len(own["sa"])) < n
    ba = min(FACTOR * max(own["e_a"], U32), CEILING)
    bl = min(FACTOR * max(own["e_al"], U32), CEILING)
    with np.errstate(divide="ignore", invalid="ignore"):
        ea = np.where(own["sa"] > 0, np.abs(rg["a"] - own["a"]).max(1) / own["sa"], np.abs(rg["a"]).max(1))[tight]
        el = np.where(own["sl"] > 0, np.abs(rg["al"] - own["al"]).max(1) / own["sl"], np.abs(rg["al"]).max(1))[tight]
    record_measured(f"test_contact_zoo {tag} per owner", a=float(ea.max()), alpha=float(el.max()), bound_a=ba, bound_alpha=bl)
    if ea.max() > ba:
        fails.append((tag, "owner a", float(ea.max()), ba, int(ea.argmax())))
    if el.max() > bl:
        fails.append((tag, "owner alpha", float(el.max()), bl, int(el.argmax())))
    # Equal and opposite, for EVERY contact.  One side's contribution = its owner's sum on the GPU minus the float64 contributions of
    # the owner's other contacts (a dumbbell's second contact; the other contacts of the plane / cylinder owner).  Linear: the two
    # forces cancel.  Angular: the two torques about the owners' centres add up to (x_B - x_A) x (F + T).  Each side may be off by
    # the per-owner bound on its owner's scale; a plane / cylinder owner sums hundreds of terms and keeps the suite's 1e-3 tree bound.
    oA, oB = c["ownerA"], c["ownerB"]
    (aA, alA), (aB, alB) = own["cA"], own["cB"]
    mA, mB = c["mass"][oA], c["mB"]
    IA, IB = c["moi"][oA], c["moi"][oB]
    fA = (rg["a"][oA] - (own["a"][oA] - aA)) * mA[:, None]
    fB = (rg["a"][oB] - (own["a"][oB] - aB)) * mB[:, None]
    bA, bB = np.where(tight[oA], ba, 1e-3), np.where(tight[oB], ba, 1e-3)
    lim = bA * own["sa"][oA] * mA + bB * own["sa"][oB] * mB
    en = np.abs(fA + fB).max(1)
    tA = m64._mv(ref["RA"], (rg["al"][oA] - (own["al"][oA] - alA)) * IA)
    tB = m64._mv(ref["RB"], (rg["al"][oB] - (own["al"][oB] - alB)) * IB)
    want = np.cross(c["posB"] - c["posA"], fA + ref["T"])
    lA, lB = np.where(tight[oA], bl, 1e-3), np.where(tight[oB], bl, 1e-3)
    limt = lA * own["sl"][oA] * IA.max(1) + lB * own["sl"][oB] * IB.max(1)
    et = np.abs(tA + tB - want).max(1)
    live = (lim > 0) & (limt > 0)  # (a contact of two owners without any force: both sides are exactly zero, or the checks below fail)
    record_measured(f"test_contact_zoo {tag} equal and opposite", force_over_bound=float((en[live] / lim[live]).max()),
                    torque_over_bound=float((et[live] / limt[live]).max()))
    if (en > lim).any():
        fails.append((tag, "opposite forces", int((en > lim).sum()), float((en[live] / lim[live]).max())))
    if (et > limt).any():
        fails.append((tag, "opposite torques", int((et > limt).sum()), float((et[live] / limt[live]).max())))
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["9mat-tile", "10mat-general", "17mat-general"])
@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_fast_mode_contact_by_contact(pkg, orc, model, numbering, build):
    """the tile kernels (9 materials; in dumbbells-first also the per-tile fallback) and the general fast kernel (10 and 17
    materials) against the float64 model, per contact and per owner, on each contact's / owner's own scale"""
    extra = {"9mat-tile": 0, "10mat-general": 1, "17mat-general": 8}[build]
    z, c, ref, ro, e, own, sim_lists = oracle_yardstick(numbering, model, extra)
    ctx = _context(pkg, z, "fast")
    _, (rg,) = run_sides(pkg, z, [ctx], model)
    assert not ctx.engine_order()[0]
    name = ctx.force_kernel()[0]
    tiles, big, halo, loc = ctx.tile_stats() if name.startswith("k_tile") else (0, 0, 0, 0)
    M = 0 if model == "hertz" else 1
    if extra == 0:
        assert name.startswith(f"k_tile_forces<{M},"), name
        if numbering == "adjacent":
            # the B side travels through the local-B lists: a tile of 128 consecutive owners holds up to 64 pairs, all of them local
            assert big == 0 and halo <= 8 and loc >= 48, (tiles, big, halo, loc)
        elif numbering == "scattered":
            assert big == 0 and halo >= 100, (tiles, big, halo, loc)                # ... through rec32 and the integrator's gather
        else:
            assert 1 <= big < tiles, (tiles, big)                                   # tile 0 through the per-tile fallback
    else:
        # (with contact recording on, a list that is not tiled goes through the general kernel in its world-frame form; the fast
        # kernel proper keeps no records and is checked below through the history and the per-owner sums)
        assert name.startswith(f"k_calc_forces<{M},"), name
    assert all(np.array_equal(a, b) for a, b in zip(ctx.contacts()[:3], sim_lists[:3]))
    eg = class_errors(rg, ref, c)
    bounds = _fast_bounds(e)
    fails = []
    for cls in CLASSES:
        record_measured(f"test_contact_zoo fast {build} {model} {numbering} {cls}",
                        **{k: eg[cls][k] for k in ("F", "T", "H", "W", "PA", "PB", "PBfar")},
                        **{"bound_" + k: bounds[cls][k] for k in ("F", "T", "H", "W")})
        for q in ("F", "T", "H", "W"):
            if eg[cls][q] > bounds[cls][q]:
                fails.append((cls, q, eg[cls][q], bounds[cls][q]))
        for q, mx in (("PA", "Pmax"), ("PB", "PBmax"), ("PBfar", "PBfarmax")):
            bp = FACTOR * max(e[cls][q], U32 * max(e[cls][mx], R0))
            if eg[cls][q] > bp:
                fails.append((cls, q, eg[cls][q], bp))
    # classes margin and apart are exact statements
    dead = ref["s"] == 0
    assert not rg["F"][dead].any() and not rg["T"][dead].any()
    if model == "hertz":
        assert not rg["hist"][dead].any()
    # ... and so is a torque-only force that the float64 model does not have (no rolling resistance, a young contact, no rotation)
    assert not rg["T"][~ref["T"].any(1)].any()
    fails += _owner_fails(f"fast {build} {model} {numbering}", rg, z, c, ref, own)
    ctx.close()
    # the kernels as a plain step runs them (no recording: k_tile_forces<M, false> / k_forces_fast<M>): history per class, sums per owner
    ctx = pkg.Context(0)
    ctx.set_arith_mode("fast")
    ctx.set_reorder(False)
    ctx.set_params(z.params)
    ctx.upload_scene(z.scene)
    ctx.set_margins(z.margins)
    ctx.detect()
    ctx.migrate()
    if model == "hertz":
        for w in range(4):
            ctx.set_wildcard(w, c["hist"][:, w].astype(np.float32))
    ctx.calc_forces()
    name = ctx.force_kernel()[0]
    assert name == (f"k_tile_forces<{M}, false>" if extra == 0 else f"k_forces_fast<{M}>"), name
    assert all(np.array_equal(a, b) for a, b in zip(ctx.contacts()[:3], sim_lists[:3]))
    st = ctx.download_state()
    r2 = dict(a=np.stack([st[k] for k in ("aX", "aY", "aZ")], 1).astype(np.float64),
              al=np.stack([st[k] for k in ("alphaX", "alphaY", "alphaZ")], 1).astype(np.float64))
    if model == "hertz":
        h2 = np.stack([ctx.wildcard(w) for w in range(4)], 1).astype(np.float64)
        e2 = class_errors(dict(F=ref["F"], T=ref["T"], PA=ref["PA"], PB=ref["PB"], hist=h2), ref, c)
        assert not h2[dead].any()
        for cls in CLASSES:
            record_measured(f"test_contact_zoo unrecorded {build} {numbering} {cls}", H=e2[cls]["H"], W=e2[cls]["W"])
            for q in ("H", "W"):
                if e2[cls][q] > bounds[cls][q]:
                    fails.append(("unrecorded", cls, q, e2[cls][q], bounds[cls][q]))
    fails += _owner_fails(f"unrecorded {build} {model} {numbering}", r2, z, c, ref, own)
    ctx.close()
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_fused_step_per_owner(pkg, orc, model):
    """k_tile_step keeps no records: after one step from the same state its velocities must be those of the unfused fast context, per
    owner within the per-owner bound times h"""
    z, c, ref, ro, e, own, _ = oracle_yardstick("adjacent", model)
    out = []
    for fused in (False, True):
        ctx = pkg.Context(0)
        ctx.set_arith_mode("fast")
        ctx.set_reorder(False)
        ctx.set_fused_step(fused)
        ctx.set_params(z.params), ctx.upload_scene(z.scene)
        ctx.set_margins(z.margins), ctx.detect(), ctx.migrate()
        if model == "hertz":
            for w in range(4):
                ctx.set_wildcard(w, c["hist"][:, w].astype(np.float32))
        ctx.step(1)
        name = ctx.force_kernel()[0]
        M = 0 if model == "hertz" else 1
        assert name == (f"k_tile_step<{M}>" if fused else f"k_tile_forces<{M}, false>"), name
        st = ctx.download_state()
        out.append(st)
        ctx.close()
    n = z.n_clumps
    ba = min(FACTOR * max(own["e_a"], U32), CEILING)
    bl = min(FACTOR * max(own["e_al"], U32), CEILING)
    V = [np.stack([s[k] for k in ("vX", "vY", "vZ")], 1).astype(np.float64)[:n] for s in out]
    W = [np.stack([s[k] for k in ("omgBarX", "omgBarY", "omgBarZ")], 1).astype(np.float64)[:n] for s in out]
    # (both sides round v + a h to fp32: half an ulp of the new velocity each, and a h itself, on top of the bound)
    ev = np.abs(V[0] - V[1]).max(1) - 2 * U32 * np.abs(V[0]).max(1)
    ew = np.abs(W[0] - W[1]).max(1) - 2 * U32 * np.abs(W[0]).max(1)
    record_measured(f"test_contact_zoo fused step {model}", dv_over_bound=float((ev / np.maximum(ba * own["sa"][:n] * H, 1e-300)).max()),
                    dw_over_bound=float((ew / np.maximum(bl * own["sl"][:n] * H, 1e-300)).max()))
    assert (ev <= ba * own["sa"][:n] * H).all(), float((ev / (ba * own["sa"][:n] * H + 1e-300)).max())
    assert (ew <= bl * own["sl"][:n] * H).all(), float((ew / (bl * own["sl"][:n] * H + 1e-300)).max())
    moved = np.abs(V[0] - np.stack([z.builder.arrays[k][:n] for k in ("vX", "vY", "vZ")], 1)).max(1) > 0
    assert moved.sum() > 0.9 * n
