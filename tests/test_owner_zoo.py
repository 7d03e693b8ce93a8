"""The owner zoo: per-owner sums and one step, owner by owner against float64, in a scene in which one dropped, doubled or mis-sliced
contribution of a many-contact owner is an O(1) error on that owner's own scale.

The contact zoo pins the force law contact by contact, but "every clump has at most two contacts": the gather's loops, tiles and
thresholds never turn.  The beds bound a / alpha by the largest acceleration of the bed.  Here the scene is made of STARS: one hub (a
one-sphere clump of radius R_h, at rest) with k satellites (one-sphere clumps of the small radius) on Fibonacci directions, each
overlapping the hub by a designed depth (a factor 1.6 within a star), approaching and sliding (hertz: sticking friction with a seeded
history, so the hub gets a torque).  Gravity is on.  Constants, materials, margins, the lattice rule and the float64 contact model are
the contact zoo's.

  hub contact counts   0 1 2 3 4 5 7 8 9 | 63 64 65 | 191 192 193 (DEME_TILE_HMAX) | 255 256 257 (DEME_HEAVY_THRESHOLD is > 256) |
                       300 600 (k_reduce_heavy with one and several strides of 256); three hubs per count and role, 30 for k = 1, 2
  roles (by numbering) hub-first: A in all its contacts (an A run) | hub-last: B in all (B list / crossing records) | hub-middle: both
  dense block one      256 consecutive hub-last hubs from a multiple of 256, ~4 satellites each numbered into other tiles: >= 1000 B
                       entries in one integrator workgroup = two LDS tiles of DEME_GATHER_TILE = 768, one hub's slice across entry 768
  dense block two      the same with 28 satellites each: 7168 > 8 x 768 entries, gather_block's per-owner fallback without a heavy owner
  tail                 free single clumps within |v| h of a voxel face, moving across it (both directions, three axes), padded so that
                       nOwners % 64 is 1, 63 or 0 (coop_load_owner / coop_store_owner's `lim`)
  builds               tile (9 materials: k_tile_forces, hub-first tiles through k_tile_forces_big), general (10 materials:
                       k_forces_fast, A runs inside one block of DEME_FORCE_BLOCK and across two), closed (stars with k <= 64 only,
                       set_fused_step: k_tile_step), exact mode on the tile scene

FLOAT64 STATEMENT per owner: a = sum(+-F_i) / m, alpha = sum MOI^-1 R^T (r_i x (+-(F_i + T_i))) (owner_sums64 of _contact_model64.py),
scales S_a = sum s_i / m and S_alpha = sum s_i |r_i| / MOI; one explicit step v1 = v0 + (a + g) h, w1 = w0 + alpha h,
x1 = x0 + v_used h, q1 = normalise(q0 (1, h/2 w_used)) with v_used = v0 | v1 | v0 + (v1 - v0) / 2 for the three schemes.

BOUNDS (none chosen freely), per owner with k entries, relative to S_a and S_alpha:
  bound(k) = min(4 max(e_single, 2^-23), 1e-5) + (k + 2) 2^-24
e_single: the oracle's per-owner error on the hubs with 1 <= k <= 2 (one evaluation; FACTOR 4 and the ceiling are the contact zoo's);
(k + 2) 2^-24: the first-order bound of a length-k fp32 sum in any order -- sequential (k - 1) u, tree ceil(log2 k) u -- on sum |x_i|,
every |component| <= s_i / m; + 3 u for the division by m and the rotation of the fast mode's world-frame sum, which the factor 4 holds
too.  The CPU yardstick asserts that the oracle (sequential fp32) stays inside max(e_single, 2^-23) + (k + 2) 2^-24 for every k.
One step: v within bound_a S_a h + 2 x 2^-24 |v1| (the rounding of a h and of v0 + a h), w the same; x within l + 3e-7 |v| h and q
within 5e-7 (tests/test_independent_pins.py derives both for the same update).  Exact mode: non-heavy owners bit-identical to the
oracle; heavy free hubs differ from it by the order of the same fp32 terms only: (k + 2) 2^-24 of S.
SATELLITES (k = 1) are owners too and the step is checked on every owner.  Their evaluation term is measured on themselves (the
oracle's largest per-owner error over the satellites, same FACTOR, floor and ceiling), not on the hubs: the oracle's contact point is
rounded on the scale of the hub's radius, up to 20 small radii, and the satellite's lever arm is one small radius -- its alpha carries
~20 u where a hub's carries ~2 u (measured: 1.3e-6 against 1.3e-7 of S_alpha).
VISIBILITY: for every hub each s_i / m is at least 10 x bound(k) x S_a: one missing term is ten bounds away (asserted on the CPU).

ACHIEVED on an MI355X (largest over the tile, general and closed builds and both models; every figure of the run, with the one-step
ratios, in profiles/owner_zoo_achieved.txt):
  k     fast a     fast alpha  exact a    exact alpha  bound a    bound alpha
  0     0.00e+00   0.00e+00    0.00e+00   0.00e+00     1.20e-06   6.38e-07
  1     2.77e-07   9.96e-08    2.61e-07   1.29e-07     1.26e-06   6.97e-07
  2     2.57e-07   7.80e-08    2.69e-07   1.30e-07     1.31e-06   7.57e-07
  3     1.76e-07   4.66e-08    1.73e-07   9.60e-08     1.37e-06   8.17e-07
  4     2.16e-07   9.04e-08    1.59e-07   6.48e-08     1.43e-06   8.76e-07
  5     1.21e-07   3.40e-08    1.28e-07   6.79e-08     1.49e-06   9.36e-07
  7     8.72e-08   3.03e-08    4.93e-08   3.03e-08     1.61e-06   1.06e-06
  8     8.19e-08   1.99e-08    6.53e-08   2.78e-08     1.67e-06   1.11e-06
  9     7.04e-08   2.16e-08    5.63e-08   2.27e-08     1.73e-06   1.17e-06
  28    7.51e-08   1.95e-08    9.00e-08   1.89e-08     2.86e-06   2.31e-06
  63    5.02e-08   7.11e-09    4.71e-08   1.05e-08     4.95e-06   4.39e-06
  64    1.21e-07   1.06e-08    7.52e-08   1.02e-08     5.01e-06   4.45e-06
  65    3.79e-08   1.26e-08    7.11e-08   9.84e-09     5.07e-06   4.51e-06
  191   1.27e-07   7.08e-09    6.69e-08   7.97e-09     1.26e-05   1.20e-05
  192   7.44e-08   3.93e-09    1.02e-07   6.26e-09     1.26e-05   1.21e-05
  193   1.05e-07   6.07e-09    9.80e-08   8.04e-09     1.27e-05   1.21e-05
  255   1.57e-07   3.17e-09    9.86e-08   5.04e-09     1.64e-05   1.58e-05
  256   9.40e-08   4.73e-09    9.45e-08   4.03e-09     1.65e-05   1.59e-05
  257   1.63e-07   2.78e-09    2.59e-08   5.94e-09     1.65e-05   1.60e-05
  300   9.09e-08   2.99e-09    7.54e-08   4.32e-09     1.91e-05   1.85e-05
  600   1.65e-07   1.99e-09    4.61e-09   4.08e-09     3.70e-05   3.64e-05

  satellites: a 4.2e-07, alpha 1.5e-06 (their own e_single: 3.3e-07 / 1.3e-06); one step: v 0.33, w 0.28 of the bound, x 0.9999 of
  the bound (l: the codec truncates), q 1.3e-07; the two gathers: 854 hubs, none differing, in exact AND fast mode; exact mode, heavy
  hubs against the oracle: 0.009 of (k + 2) 2^-24; momentum per star: 0.033 of the bound.  No bug found.
(c) holds bit for bit in fast mode too: integrate_owner and acc_from_world are compiled without contraction (-ffp-contract=off, no
fp contract pragma in deme_kernels.h), so no 1-ulp allowance is made.

MUTATIONS of the gather, each built and run once on an MI355X (not kept).  Each changes which in-bounds values are summed, never an
address or a bound of a load or store.  "new": failing GPU cases of tests/test_owner_zoo.py (25); "old": failing GPU cases of
tests/test_fast_mode.py + tests/test_fast_mode_features.py + tests/test_contact_zoo.py without this file (43).
  1  gather_block's tile loop stops one tile early (`base + TILE < hiB`: with one tile it never runs)
       new 17: one_step (8), two_gathers (3), staged_step (2), closed_tiles (2), exact_mode (2)      old 12 (every bed loses its B side)
  1b the same, but only the last of several tiles is dropped (the first always runs)
       new 15: one_step (8), two_gathers (3), staged_step (2), exact_mode (2)                        old 1 (test_fast_mode_cylinders)
  2  gather_block's `e` clamp uses base + DEME_GATHER_TILE - 1
       new 15: one_step (8), two_gathers (3), staged_step (2), exact_mode (2)                        old 1 (test_fast_mode_metre_scale)
  3  k_reduce_heavy's tree starts at off = 64
       new 18: standalone_sums (4), one_step (8), exact_mode (2), linear_momentum (4)                old 1 (the raft: free_owner_with_hundreds_of_contacts)
  4  a_side_sum ignores a_run_in_one_block and always takes aSum
       new 8: standalone_sums, one_step, linear_momentum on the general build (2 each), exact_mode (2)   old 18
  5  gather_b_load's tile form swaps r24[1] and r24[2]
       new 12: standalone_sums, one_step (6), closed_tiles, linear_momentum on the tile build          old 19
  6  k_owner_ranges_tile uses >= for the heavy test, k_owner_ranges keeps >
       new 0, old 0 at first: a hub with exactly 256 entries then goes through k_reduce_heavy's tree, whose sum differs from the
       sequential one in rounding only -- inside every bound.  The assertion that should have caught it is "both list forms flag
       exactly the owners with more than 256 entries heavy"; the library could not be asked.  Added: deme_heavy_owners (C ABI,
       Context.heavy_owners) and the assertion in every GPU case (_kernel_checks).  With it:
       new 12: standalone_sums, one_step (6), two_gathers, staged_step (fast), linear_momentum on the tile build      old 0
Mutations 1b, 2, 3 and 6 are the gap: the older files see them through one bed-scale assertion each, or not at all.
"""
import functools

import numpy as np
import pytest

from tests import _contact_model64 as m64
from tests.conftest import record_measured
from tests.test_contact_zoo import (CEILING, EXTRA, FACTOR, MARGIN, MATERIALS, OVERRIDES, R0, RHO, U32, _pair_tables,
                                    design_history, positions64)

U24 = 2.0 ** -24
KS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 191, 192, 193, 255, 256, 257, 300, 600)
ROLES = ("first", "last", "middle")
MEMBERS = {1: 30, 2: 30}          # hubs per (count, role); 3 otherwise
GROUPS = (5, 9, 65, 193, 257, 300, 600)   # one hub template (radius) per group of counts: the tile pass's table holds few components
HUB_SATS = {0: (3, 0, 4), 3: (0, 5, 3, 1), 5: (3, 5, 2)}   # hub material -> satellite materials with Crr = 0 and mu > 0 (sticking)
DEPTH0 = 4e-3 * R0
SEP = 2.6 * R0                    # two satellites are listed together below 2 R0 + 2 MARGIN - EXTRA = 2.36 R0
TILE_NB, GATHER_TILE, FORCE_BLOCK, HEAVY, HMAX = 128, 768, 256, 256, 192   # csrc: DEME_TILE_NB, DEME_GATHER_TILE, ...
CELL, CELL0, NCELL = 0.024, 0.30, 14
DENSE1, DENSE2 = 4, 28
TAILS = (1, 63, 0)


def fib_dirs(k):
    i = np.arange(k) + 0.5
    z = 1.0 - 2.0 * i / max(k, 1)
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


@functools.lru_cache(maxsize=None)
def hub_radius(group):
    """the smallest hub radius (in R0, at least 1) at which the Fibonacci satellites of every count of the group keep SEP apart"""
    lo = max([g for g in GROUPS if g < group], default=-1)
    need = 1.0
    for k in [k for k in KS + (DENSE1 + 1, DENSE2) if lo < k <= group and k >= 2]:
        d = fib_dirs(k)
        c = np.sqrt(((d[:, None, :] - d[None, :, :]) ** 2).sum(2) + 4.0 * np.eye(k)).min()
        need = max(need, SEP / R0 / c - 1.0 + 0.05)
    return float(np.ceil(need * 10.0) / 10.0)


def group_of(k):
    return min(g for g in GROUPS if k <= g)


class Zoo:
    pass


@functools.lru_cache(maxsize=None)
def build_stars(build, model, tail=1, scheme=2, seed=4099):
    """the scene; build: tile (9 materials) | general (10) | closed (9, stars with k <= 64 only, no dense blocks)"""
    import __graft_entry__ as entry
    pkg = entry.load_package()
    rng = np.random.default_rng(seed)
    tab = _pair_tables(len(MATERIALS))
    b = pkg.SceneBuilder()
    for mat in MATERIALS:
        b.LoadMaterial(mat)
    if build == "general":  # not used by any contact: only the size of the table changes
        b.LoadMaterial(dict(MATERIALS[0]))
    for name, a, c, val in OVERRIDES:
        b.SetMaterialPropertyPair(name, a, c, val)
    b.InstructBoxDomainDimension((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
    b.InstructBoxDomainBoundingBC("none", 0)
    b.SetInitTimeStep(5e-6)
    b.SetGravitationalAcceleration((0, 0, -9.81))
    b.SetCDUpdateFreq(0)
    b.SetFamilyExtraMargin(0, EXTRA)
    b.SetIntegrator(["FORWARD_EULER", "CENTERED_DIFFERENCE", "EXTENDED_TAYLOR"][scheme])
    if model == "frictionless":
        b.UseFrictionlessHertzianModel()
    radii = [1.0] + [hub_radius(g) for g in GROUPS]
    tmpl, mass = [], []
    for r in radii:
        m = RHO * 4.0 / 3.0 * np.pi * (r * R0) ** 3
        mass.append(m)
        tmpl.append(b.LoadClumpType(m, (m * 0.4 * (r * R0) ** 2,) * 3, np.array([r * R0]), np.zeros((1, 3)), 0))
    t_of_group = {g: 1 + i for i, g in enumerate(GROUPS)}

    cells = rng.permutation(NCELL ** 3)
    cell_i = [0]

    def next_cell():
        k = int(cells[cell_i[0]])
        cell_i[0] += 1
        return CELL0 + CELL * np.array([k % NCELL, (k // NCELL) % NCELL, k // (NCELL * NCELL)], np.float64)

    def rand_q():
        q = pkg.model.random_unit_quaternions(1, rng)[0]  # x y z w
        return np.array([q[3], q[0], q[1], q[2]], np.float32)

    def unit(v):
        return v / np.linalg.norm(v)

    owners, stars = [], []   # owners: dicts tmpl, pos, q, v, w, mat, star, tail

    def make_star(k, role, kind):
        C, hm = next_cell(), int(rng.choice(list(HUB_SATS)))
        g = group_of(k)
        rh = radii[t_of_group[g]] * R0
        hub = len(owners)
        owners.append(dict(tmpl=t_of_group[g], pos=C, q=rand_q(), v=np.zeros(3), w=np.zeros(3), mat=hm, star=len(stars), tail=None))
        Rm = m64.rot_matrix(rand_q()[None, :].astype(np.float64))[0]
        dirs = fib_dirs(k) @ Rm.T
        one_mat = int(rng.choice(HUB_SATS[hm]))
        sats = []
        for n in dirs:
            sm = int(rng.choice(HUB_SATS[hm])) if k <= 9 else one_mat
            depth = DEPTH0 * rng.uniform(1.0, 1.6)
            k_n, g_n, k_t, g_t, _ = m64.coefficients(tab["E_cnt"][sm, hm], tab["G_cnt"][sm, hm], tab["beta"][sm, hm], mass[0],
                                                     mass[t_of_group[g]], R0, rh, depth)
            Fn0 = k_n * depth   # the contact zoo's `stick` motion: approach at 0.3 Fn0 / |g_n|, slide at 0.1 mu Fn / |g_t|
            vn, vt = -0.3 * Fn0 / abs(g_n), 0.1 * tab["mu"][sm, hm] * 1.3 * Fn0 / abs(g_t)
            t = unit(np.cross(n, rng.normal(size=3)))
            sats.append(len(owners))
            owners.append(dict(tmpl=0, pos=C + n * (rh + R0 - depth), q=rand_q(), v=vn * n + vt * t,
                               w=unit(rng.normal(size=3)) * 0.3 * vt / R0, mat=sm, star=len(stars), tail=None))
        stars.append(dict(hub=hub, sats=sats, k=k, role=role, kind=kind))
        return stars[-1]

    ks = [k for k in KS if k <= 64] if build == "closed" else list(KS)
    plain = [make_star(k, role, "star") for k in ks for role in ROLES for _ in range(MEMBERS.get(k, 3))]
    dense1 = dense2 = []
    if build != "closed":
        n1 = 3 + (np.arange(256) * 5) % 3                     # 3, 4 or 5 satellites, ~4 per hub
        n1[-1] += 256 * DENSE1 - int(n1.sum())                # ... 1024 in all
        if GATHER_TILE in set(np.cumsum(n1).tolist()):        # entry 768 inside a hub's slice, not between two
            n1[0] += 1
            n1[-1] -= 1
        assert n1.min() >= 2 and n1.max() <= DENSE1 + 1 and n1.sum() == 256 * DENSE1
        dense1 = [make_star(int(k), "last", "dense1") for k in n1]
        dense2 = [make_star(DENSE2, "last", "dense2") for _ in range(256)]
    # ---- numbering: the dense blocks' satellites (a multiple of 256), their hubs, the stars in a random order, the tail
    order = [i for s in dense1 + dense2 for i in s["sats"]] + [s["hub"] for s in dense1 + dense2]
    assert len(order) % 256 == 0
    for j in rng.permutation(len(plain)):
        s = plain[int(j)]
        half = {"first": 0, "last": s["k"], "middle": s["k"] // 2}[s["role"]]
        order += s["sats"][:half] + [s["hub"]] + s["sats"][half:]
    n_tail = 18
    while (len(order) + n_tail) % 64 != tail:
        n_tail += 1
    for j in range(n_tail):
        order.append(len(owners))
        owners.append(dict(tmpl=0, pos=next_cell(), q=rand_q(), v=np.zeros(3), w=rng.normal(size=3) * 5.0, mat=int(rng.integers(7)),
                           star=-1, tail=(j % 3, 1 if (j // 3) % 2 else -1)))
    n_own = len(owners)
    assert sorted(order) == list(range(n_own))
    new_id = np.empty(n_own, np.int64)
    new_id[np.array(order)] = np.arange(n_own)
    owners = [owners[i] for i in order]
    b.AddClumps([tmpl[o["tmpl"]] for o in owners], np.array([o["pos"] for o in owners], np.float32))
    p, sc = b.Initialize()
    A = b.arrays
    lbf = np.array([float(p.LBFX), float(p.LBFY), float(p.LBFZ)])
    G = np.rint((np.array([o["pos"] for o in owners]) - lbf) / p.l).astype(np.int64)
    V, W = np.array([o["v"] for o in owners]), np.array([o["w"] for o in owners])
    h = float(p.h)
    for i, o in enumerate(owners):
        if o["tail"] is not None:  # 3 lattice units inside a voxel face, 60 units per step towards it (gravity: 14 units)
            ax, sg = o["tail"]
            G[i, ax] = (G[i, ax] // 65536) * 65536 + (65533 if sg > 0 else 2)
            V[i, ax] = sg * 60.0 * p.l / h
    vox = G // 65536
    A["voxelID"][:n_own] = (vox[:, 0] + (vox[:, 1] << p.nvXp2) + (vox[:, 2] << (p.nvXp2 + p.nvYp2))).astype(np.uint64)
    for k, name in enumerate(("locX", "locY", "locZ")):
        A[name][:n_own] = (G[:, k] % 65536).astype(np.uint16)
    Q = np.array([o["q"] for o in owners], np.float32)
    for k, name in enumerate(("oriQw", "oriQx", "oriQy", "oriQz")):
        A[name][:n_own] = Q[:, k]
    for k in range(3):
        A[("vX", "vY", "vZ")[k]][:n_own] = V[:, k].astype(np.float32)
        A[("omgBarX", "omgBarY", "omgBarZ")[k]][:n_own] = W[:, k].astype(np.float32)
    assert len(A["sphereMaterialOffset"]) == n_own and int(b.counts["nOwners"]) == n_own
    A["sphereMaterialOffset"][:] = np.array([o["mat"] for o in owners], np.uint16)
    z = Zoo()
    z.builder, z.params, z.build, z.model = b, p, build, model
    z.scene = pkg.abi.make_scene_struct(A, b.counts)
    z.n = n_own
    z.tables = _pair_tables(len(MATERIALS) + (1 if build == "general" else 0))
    z.margins = np.full(n_own, MARGIN, np.float32)
    z.cls_of_sphere = np.full(n_own, "stick", dtype=object)
    allst = plain + dense1 + dense2
    z.hub = new_id[np.array([s["hub"] for s in allst])]
    z.hub_k = np.array([s["k"] for s in allst])
    z.hub_role = np.array([s["role"] for s in allst], dtype=object)
    z.hub_kind = np.array([s["kind"] for s in allst], dtype=object)
    z.star_of = np.array([o["star"] for o in owners])
    z.is_hub = np.zeros(n_own, bool)
    z.is_hub[z.hub] = True
    z.tail = np.array([i for i, o in enumerate(owners) if o["tail"] is not None])
    z.tail_axis = np.array([owners[i]["tail"] for i in z.tail])
    z.mass = np.asarray(A["MassProperties"], np.float64)[np.asarray(A["inertiaPropOffsets"], np.int64)][:n_own]
    return z


def gather_inputs(pkg, z, contacts, hist):
    """the float64 model's inputs for the listed contacts: the contact zoo's, for a scene of one-sphere clumps without objects"""
    A = z.builder.arrays
    idA, idB, typ = (np.asarray(x).astype(np.int64) for x in contacts[:3])
    assert (typ == 1).all()
    f = lambda k: np.asarray(A[k], np.float64)
    own = np.asarray(A["ownerClumpBody"], np.int64)
    oA, oB = own[idA], own[idB]
    X = positions64(pkg, z)
    Q = np.stack([f("oriQw"), f("oriQx"), f("oriQy"), f("oriQz")], 1)
    V, W = np.stack([f("vX"), f("vY"), f("vZ")], 1), np.stack([f("omgBarX"), f("omgBarY"), f("omgBarZ")], 1)
    ipo = np.asarray(A["inertiaPropOffsets"], np.int64)
    mass = f("MassProperties")[ipo]
    moi = np.stack([f("moiX"), f("moiY"), f("moiZ")], 1)[ipo]
    comp = np.asarray(A["clumpComponentOffset"], np.int64)
    rel = np.stack([f("CDRelPosX"), f("CDRelPosY"), f("CDRelPosZ")], 1)
    smat = np.asarray(A["sphereMaterialOffset"], np.int64)
    mA_, mB_ = smat[idA], smat[idB]
    T, n = z.tables, len(idA)
    c = dict(posA=X[oA], posB=X[oB], qA=Q[oA], qB=Q[oB], vA=V[oA], vB=V[oB], wA=W[oA], wB=W[oB], mA=mass[oA], mB=mass[oB],
             relA=rel[comp[idA]], rA=f("Radii")[comp[idA]], kind=np.full(n, m64.KIND_SPHERE), relB=rel[comp[idB]],
             rB=f("Radii")[comp[idB]], dirB=np.zeros((n, 3)), sizeB=np.zeros(n), signB=np.zeros(n), E_cnt=T["E_cnt"][mA_, mB_],
             G_cnt=T["G_cnt"][mA_, mB_], beta=T["beta"][mA_, mB_], mu=T["mu"][mA_, mB_], Crr=T["Crr"][mA_, mB_],
             hist=np.asarray(hist, np.float64), extra=np.full(n, float(np.float32(EXTRA))))
    c.update(ownerA=oA, ownerB=oB, matA=mA_, matB=mB_, mass=mass, moi=moi, cls=z.cls_of_sphere[idA])
    return c


def _vec(st, names):
    return np.stack([np.asarray(st[k]) for k in names], 1)


V_, W_, Q_ = ("vX", "vY", "vZ"), ("omgBarX", "omgBarY", "omgBarZ"), ("oriQw", "oriQx", "oriQy", "oriQz")
A_, AL_ = ("aX", "aY", "aZ"), ("alphaX", "alphaY", "alphaZ")
STATE = ("voxelID", "locX", "locY", "locZ") + V_ + W_ + Q_


def prepare(side, z, hist=None):
    """detect, migrate, seed the history"""
    side.set_margins(z.margins)
    side.detect()
    side.migrate()
    if hist is not None and z.model == "hertz":
        for w in range(4):
            side.set_wildcard(w, np.ascontiguousarray(hist[:, w], np.float32))


def step64(pkg, z, a, al, scheme):
    """one explicit step of every owner in float64 from the scene's state and the float64 sums"""
    A, p, n = z.builder.arrays, z.params, z.n
    h = float(p.h)
    g = np.array([float(p.Gx), float(p.Gy), float(p.Gz)])
    X0 = positions64(pkg, z)[:n]
    V0, W0, Q0 = (_vec(A, k)[:n].astype(np.float64) for k in (V_, W_, Q_))
    v_upd, w_upd = (a[:n] + g) * h, al[:n] * h
    f = (0.0, 1.0, 0.5)[scheme]
    vu, wu = V0 + f * v_upd, W0 + f * w_upd
    ha = 0.5 * h * wu
    a1, b1, c1, d1 = Q0.T
    b2, c2, d2 = ha.T
    q = np.stack([a1 - b1 * b2 - c1 * c2 - d1 * d2, a1 * b2 + b1 + c1 * d2 - d1 * c2, a1 * c2 - b1 * d2 + c1 + d1 * b2,
                  a1 * d2 + b1 * c2 - c1 * b2 + d1], 1)
    q /= np.sqrt((q * q).sum(1))[:, None]
    return dict(V=V0 + v_upd, W=W0 + w_upd, X=X0 + vu * h, Q=q, vu=vu)


def bound_of(e_single, k):
    return min(FACTOR * max(e_single, U32), CEILING) + (k + 2.0) * U24


@functools.lru_cache(maxsize=None)
def oracle_yardstick(build, model, tail=1, scheme=2):
    """the oracle's run of the zoo (sums, and one step from the same state) and the float64 statement, once per scene"""
    import __graft_entry__ as entry
    pkg, orc = entry.load_package(), entry.load_oracle()
    z = build_stars(build, model, tail, scheme)
    n = z.n
    sim = orc.make_sim(pkg, z.params, z.scene)
    prepare(sim, z)
    lists = sim.contacts()
    c = gather_inputs(pkg, z, lists, np.zeros((len(lists[0]), 4)))
    hist = design_history(c) if model == "hertz" else np.zeros((len(lists[0]), 4), np.float32)
    c["hist"] = hist.astype(np.float64)
    if model == "hertz":
        for w in range(4):
            sim.set_wildcard(w, hist[:, w])
    sim.calc_forces(record=True)
    st = sim.download_state()
    ro = dict(a=_vec(st, A_).astype(np.float64), al=_vec(st, AL_).astype(np.float64))
    sim.integrate()
    ro["state"] = {k: np.array(v) for k, v in sim.download_state().items()}
    sim.close()
    ref = m64.contact64(c, float(z.params.h), model)
    a, al, cA, cB, sa, sl = m64.owner_sums64(ref, c["ownerA"], c["ownerB"], n, c["mass"], c["moi"], c["mB"])
    nA, nB = np.bincount(c["ownerA"], minlength=n), np.bincount(c["ownerB"], minlength=n)
    k = nA + nB
    with np.errstate(divide="ignore", invalid="ignore"):
        ea = np.where(sa > 0, np.abs(ro["a"] - a).max(1) / sa, np.abs(ro["a"]).max(1))
        el = np.where(sl > 0, np.abs(ro["al"] - al).max(1) / sl, np.abs(ro["al"]).max(1))
    single = z.is_hub & (k >= 1) & (k <= 2)
    own = dict(a=a, al=al, sa=sa, sl=sl, cA=cA, cB=cB, k=k, nA=nA, nB=nB, ea=ea, el=el, e_a=float(ea[single].max()),
               e_al=float(el[single].max()))
    sat = ~z.is_hub   # one evaluation each, measured on themselves: see SATELLITES in the module docstring
    own["e_a_sat"], own["e_al_sat"] = float(ea[sat].max()), float(el[sat].max())
    own["ba"] = np.array([bound_of(own["e_a_sat"] if s else own["e_a"], x) for x, s in zip(k, sat)])
    own["bl"] = np.array([bound_of(own["e_al_sat"] if s else own["e_al"], x) for x, s in zip(k, sat)])
    own["step"] = step64(pkg, z, a, al, scheme)
    return z, c, ref, ro, own, lists


def path_conditions(z, c, own, tiled):
    """what the list says about the paths the gather takes: asserted by every case, on the CPU and on the GPU"""
    n, k = z.n, own["k"]
    out = {}
    hub_k = k[z.hub]
    free_star = z.hub_kind == "star"
    assert np.array_equal(hub_k, z.hub_k), "a hub's entries are not its designed count"
    assert (k[~z.is_hub] <= 1).all()
    for kk in (255, 256, 257):  # both sides of the heavy threshold, every role
        for role in ROLES:
            assert ((z.hub_k == kk) & (z.hub_role == role) & free_star).sum() >= 3 or z.build == "closed"
    out["heavy"] = int((k > HEAVY).sum())
    if z.build == "closed":
        assert out["heavy"] == 0
        return out
    assert out["heavy"] == 3 * 3 * 3   # 257, 300, 600
    # B entries as the integrator's workgroups of 256 owners see them: all of them, or (tile form) the crossing ones only
    cross = (c["ownerA"] // TILE_NB) != (c["ownerB"] // TILE_NB)
    nB = np.bincount(c["ownerB"][cross] if tiled else c["ownerB"], minlength=n)
    bStart = np.r_[0, np.cumsum(nB)]
    for name, lo_ in (("dense1", int(z.hub[z.hub_kind == "dense1"].min())), ("dense2", int(z.hub[z.hub_kind == "dense2"].min()))):
        hubs = np.sort(z.hub[z.hub_kind == name])
        assert lo_ % 256 == 0 and np.array_equal(hubs, lo_ + np.arange(256))
        assert (own["nA"][hubs] == 0).all() and (k[hubs] <= HEAVY).all()
        loB, hiB = int(bStart[lo_]), int(bStart[lo_ + 256])
        assert hiB - loB == int(k[hubs].sum()), "the block's satellites are numbered into other tiles"
        if name == "dense1":
            assert GATHER_TILE + 200 < hiB - loB <= 2 * GATHER_TILE and hiB - loB >= 1000
            s, e = bStart[hubs] - loB, bStart[hubs + 1] - loB
            assert ((s < GATHER_TILE) & (e > GATHER_TILE)).sum() == 1, "no slice straddles the LDS tile"
        else:
            assert hiB - loB > 8 * GATHER_TILE
    # hub-first runs inside one force block and across two (general form: aSum against conA)
    aStart = np.r_[0, np.cumsum(own["nA"])]
    first = z.hub[(z.hub_role != "last") & (own["nA"][z.hub] > 0) & (k[z.hub] <= HEAVY)]
    s, e = aStart[first], aStart[first + 1]
    one = s // FORCE_BLOCK == (e - 1) // FORCE_BLOCK
    out["runs_one_block"], out["runs_straddling"] = int(one.sum()), int((~one).sum())
    assert out["runs_one_block"] >= 10 and out["runs_straddling"] >= 5, out
    return out


# ------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("build,tail", [("tile", 1), ("tile", 63), ("tile", 0), ("general", 1), ("closed", 1)])
def test_design_holds(pkg, orc, build, tail):
    """counts per hub and role as designed, only hub-satellite pairs of one star listed, >= 3 hubs per count and role, the dense
    blocks' straddle and fallback conditions, sticking contacts clear of the friction limit, the tail crosses voxel faces"""
    z, c, ref, ro, own, lists = oracle_yardstick(build, "hertz", tail)
    oA, oB = c["ownerA"], c["ownerB"]
    assert z.n % 64 == tail
    assert (z.star_of[oA] == z.star_of[oB]).all() and (z.star_of[oA] >= 0).all()
    assert (z.is_hub[oA] ^ z.is_hub[oB]).all(), "a listed pair that is not hub-satellite"
    assert len(oA) == int(z.hub_k.sum())
    ks = [k for k in KS if k <= 64] if build == "closed" else KS
    for k in ks:
        for role in ROLES:
            m = (z.hub_k == k) & (z.hub_role == role) & (z.hub_kind == "star")
            assert m.sum() >= 3, (k, role)
            hubs = z.hub[m]
            nA, nB = own["nA"][hubs], own["nB"][hubs]
            want_a = {"first": k, "last": 0, "middle": k - k // 2}[role]
            assert (nA == want_a).all() and (nB == k - want_a).all(), (k, role, nA, nB)
    path_conditions(z, c, own, tiled=(build != "general"))
    # the float64 model: every contact carries force and sticks, well inside the friction limit; depths within a factor 2 per star
    assert (ref["label"] == "stick").all() and (ref["s"] > 0).all()
    assert (ref["ft"] <= 0.7 * ref["ft_max"]).all() and (ref["ft"] >= 2 * m64.TINY).all()
    hub_of = np.where(z.is_hub[oA], oA, oB)
    dmin, dmax = np.full(z.n, np.inf), np.zeros(z.n)
    np.minimum.at(dmin, hub_of, ref["depth"])
    np.maximum.at(dmax, hub_of, ref["depth"])
    assert (dmax[z.hub[z.hub_k > 0]] <= 2.0 * dmin[z.hub[z.hub_k > 0]]).all()
    A = z.builder.arrays
    assert not _vec(A, V_)[z.hub].any() and not _vec(A, W_)[z.hub].any()
    assert (np.abs(own["al"][z.hub[z.hub_k > 0]]).max(1) > 0).all()
    # the tail: in the float64 statement every clump leaves its voxel along its axis, in its direction
    p = z.params
    lbf = np.array([float(p.LBFX), float(p.LBFY), float(p.LBFZ)])
    X0, X1 = positions64(pkg, z)[z.tail] - lbf, own["step"]["X"][z.tail] - lbf
    v0, v1 = np.floor(X0 / p.voxelSize), np.floor(X1 / p.voxelSize)
    ax, sg = z.tail_axis[:, 0], z.tail_axis[:, 1]
    i = np.arange(len(z.tail))
    assert np.array_equal(v1[i, ax] - v0[i, ax], sg)
    assert {(int(a), int(s)) for a, s in z.tail_axis} == {(a, s) for a in range(3) for s in (-1, 1)}
    frac = X1[i, ax] / p.l - np.floor(X1[i, ax] / p.voxelSize) * 65536
    assert ((frac > 8) & (frac < 65536 - 8)).all()   # ... and lands clear of the face: no either-or for the codec's truncation


@pytest.mark.parametrize("build", ["tile", "general", "closed"])
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_oracle_against_float64_per_owner(pkg, orc, build, model):
    """YARDSTICK e_orc_owner: the oracle sums sequentially in fp32; it must stay inside max(e_single, 2^-23) + (k + 2) 2^-24 for every
    k, or the summation term is wrong.  VISIBILITY: each s_i / m of a hub is at least 10 bounds of that hub"""
    z, c, ref, ro, own, lists = oracle_yardstick(build, model)
    k = own["k"]
    assert own["e_a"] <= CEILING and own["e_al"] <= CEILING
    lim_a, lim_l = max(own["e_a"], U32) + (k + 2.0) * U24, max(own["e_al"], U32) + (k + 2.0) * U24
    for kk in sorted(set(z.hub_k.tolist())):
        hubs = z.hub[z.hub_k == kk]
        record_measured(f"test_owner_zoo e_orc_owner {build} {model} k={kk}", a=float(own["ea"][hubs].max()),
                        alpha=float(own["el"][hubs].max()), limit_a=float(lim_a[hubs].max()), bound_fast_a=float(own["ba"][hubs].max()))
    record_measured(f"test_owner_zoo e_single {build} {model}", a=own["e_a"], alpha=own["e_al"],
                    satellites_a=float(own["ea"][~z.is_hub].max()), satellites_alpha=float(own["el"][~z.is_hub].max()))
    hb = z.hub
    assert (own["ea"][hb] <= lim_a[hb]).all(), (float((own["ea"] / lim_a)[hb].max()), int(k[hb][(own["ea"] / lim_a)[hb].argmax()]))
    assert (own["el"][hb] <= lim_l[hb]).all(), (float((own["el"] / lim_l)[hb].max()), int(k[hb][(own["el"] / lim_l)[hb].argmax()]))
    assert own["e_a_sat"] <= CEILING and own["e_al_sat"] <= CEILING, (own["e_a_sat"], own["e_al_sat"])
    # visibility
    hub_of = np.where(z.is_hub[c["ownerA"]], c["ownerA"], c["ownerB"])
    share = ref["s"] / z.mass[hub_of] / own["sa"][hub_of]
    vis = share / own["ba"][hub_of]
    record_measured(f"test_owner_zoo visibility {build} {model}", smallest_share_over_bound=float(vis.min()))
    assert (vis >= 10.0).all(), (float(vis.min()), int(k[hub_of[vis.argmin()]]))


# ------------------------------------------------------------------------------------------------------------ GPU tests
def _kernel_checks(ctx, z, model, n_heavy, fused=False):
    """the kernel that ran, the tile statistics and the owners flagged heavy, by build.  k_owner_ranges (general form) and
    k_owner_ranges_tile (tile form) count an owner's entries from different structures: both must flag exactly the owners with more
    than DEME_HEAVY_THRESHOLD entries in the list -- the hubs with 256 are not among them, those with 257 are"""
    name = ctx.force_kernel()[0]
    assert ctx.heavy_owners() == (n_heavy, n_heavy), (ctx.heavy_owners(), n_heavy)
    M = 0 if model == "hertz" else 1
    mode = ctx.arith_mode()
    tiles = big = 0
    if mode == "exact":
        assert name.startswith(f"k_calc_forces<{M},"), name
    elif z.build == "general":
        assert name == f"k_forces_fast<{M}>", name
    else:
        tiles, big, halo, loc = ctx.tile_stats()
        if fused:
            assert name == f"k_tile_step<{M}>", name
        else:
            assert name == f"k_tile_forces<{M}, false>", name
        assert tiles == (z.n + TILE_NB - 1) // TILE_NB
        if z.build == "tile":
            assert 1 <= big < tiles, (tiles, big)   # the tiles of hub-first hubs with hundreds of foreign satellites
        else:
            assert big == 0 and halo <= HMAX, (tiles, big, halo)
    return name, tiles, big


@functools.lru_cache(maxsize=None)
def gpu_run(build, model, mode, tail=1, scheme=2, fused=False):
    """(a) detect, migrate, seed, calc_forces, download: a / alpha of the stand-alone reduction; then integrate(): the staged step
    (d); (b) a second context from the same state: step(1).  One run per case, shared by the tests"""
    import __graft_entry__ as entry
    pkg = entry.load_package()
    z, c, ref, ro, own, lists = oracle_yardstick(build, model, tail, scheme)
    out = {}
    n_heavy = int((own["k"] > HEAVY).sum())
    for which in ("staged", "stepped"):
        ctx = pkg.Context(0)
        ctx.set_arith_mode(mode)
        ctx.set_reorder(False)
        ctx.set_fused_step(fused)
        ctx.set_params(z.params), ctx.upload_scene(z.scene)
        prepare(ctx, z, c["hist"])
        assert not ctx.engine_order()[0]
        assert all(np.array_equal(a, b) for a, b in zip(ctx.contacts()[:3], lists[:3])), "contact lists differ"
        if which == "staged":
            ctx.calc_forces()
            out["kernel_staged"] = _kernel_checks(ctx, z, model, n_heavy)
            st = ctx.download_state()
            out["a"], out["al"] = _vec(st, A_), _vec(st, AL_)
            ctx.integrate()
        else:
            ctx.step(1)
            out["kernel_stepped"] = _kernel_checks(ctx, z, model, n_heavy, fused)
        out[which] = {k: np.array(v) for k, v in ctx.download_state().items()}
        ctx.close()
    return out


def _rel(x, ref, scale):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, np.abs(x - ref).max(1) / scale, np.abs(x).max(1))


def _worst_by_k(z, e, b):
    """{k: (largest error, bound)} over the hubs"""
    return {int(k): (float(e[z.hub[z.hub_k == k]].max()), float(b[z.hub[z.hub_k == k]].max())) for k in sorted(set(z.hub_k.tolist()))}


def _check_sums(tag, z, own, a, al):
    ea, el = _rel(a.astype(np.float64), own["a"], own["sa"]), _rel(al.astype(np.float64), own["al"], own["sl"])
    for k, (e, b) in _worst_by_k(z, ea, own["ba"]).items():
        record_measured(f"test_owner_zoo {tag} k={k}", a=e, bound_a=b, alpha=float(el[z.hub[z.hub_k == k]].max()),
                        bound_alpha=float(own["bl"][z.hub[z.hub_k == k]].max()))
    record_measured(f"test_owner_zoo {tag} satellites", a=float(ea[~z.is_hub].max()), alpha=float(el[~z.is_hub].max()))
    bad_a, bad_l = np.nonzero(ea > own["ba"])[0], np.nonzero(el > own["bl"])[0]
    return [(tag, "a", int(o), int(own["k"][o]), float(ea[o]), float(own["ba"][o])) for o in bad_a[:8]] + \
           [(tag, "alpha", int(o), int(own["k"][o]), float(el[o]), float(own["bl"][o])) for o in bad_l[:8]]


CASES = [("tile", "hertz"), ("tile", "frictionless"), ("general", "hertz"), ("general", "frictionless")]


@pytest.mark.gpu
@pytest.mark.parametrize("build,model", CASES)
def test_standalone_sums_per_owner(pkg, orc, build, model):
    """(a) k_gather_acc / gather_owner and the stand-alone k_reduce_heavy: a and alpha of every owner against float64"""
    z, c, ref, ro, own, lists = oracle_yardstick(build, model)
    path_conditions(z, c, own, tiled=(build == "tile"))
    r = gpu_run(build, model, "fast")
    fails = _check_sums(f"standalone fast {build} {model}", z, own, r["a"], r["al"])
    assert not fails, fails


def _check_step(tag, pkg, z, own, st):
    """v1, w1, x1, q1 of every owner against the float64 step"""
    s64, p, n = own["step"], z.params, z.n
    h = float(p.h)
    V, W, Q = (_vec(st, k)[:n].astype(np.float64) for k in (V_, W_, Q_))
    X = pkg.model.decode_positions(st["voxelID"], st["locX"], st["locY"], st["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)[:n]
    X = X + np.array([float(p.LBFX), float(p.LBFY), float(p.LBFZ)])[None, :]
    bv = own["ba"] * own["sa"] * h + 2 * U24 * np.abs(s64["V"]).max(1)
    bw = own["bl"] * own["sl"] * h + 2 * U24 * np.abs(s64["W"]).max(1)
    ev, ew = np.abs(V - s64["V"]).max(1), np.abs(W - s64["W"]).max(1)
    bx = p.l + 3e-7 * np.abs(s64["vu"]) * h + 1e-15 * np.maximum(np.abs(s64["X"]), 1.0)
    ex, eq = np.abs(X - s64["X"]), np.abs(Q - s64["Q"]).max(1)
    tiny = 1e-300
    record_measured(f"test_owner_zoo {tag}", dv_over_bound=float((ev / np.maximum(bv, tiny)).max()),
                    dw_over_bound=float((ew / np.maximum(bw, tiny)).max()), dx_over_bound=float((ex / bx).max()), dq=float(eq.max()),
                    hubs_dv_over_bound=float((ev / np.maximum(bv, tiny))[z.hub].max()))
    fails = []
    for name, e, b in (("v", ev, bv), ("w", ew, bw), ("x", (ex - bx).max(1), 0.0), ("q", eq, 5e-7)):
        bad = np.nonzero(e > b)[0]
        fails += [(tag, name, int(o), int(own["k"][o]), float(e[o])) for o in bad[:8]]
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("build,model,tail,scheme", [("tile", "hertz", 1, 2), ("tile", "hertz", 63, 2), ("tile", "hertz", 0, 2),
                                                     ("tile", "hertz", 1, 0), ("tile", "hertz", 1, 1), ("tile", "frictionless", 1, 2),
                                                     ("general", "hertz", 1, 2), ("general", "frictionless", 1, 2)])
def test_one_step_per_owner(pkg, orc, build, model, tail, scheme):
    """(b) k_integrate<true> / gather_block and the loop's k_reduce_heavy: the state of every owner after step(1) against the float64
    step; the tail's clumps change their voxel"""
    z, c, ref, ro, own, lists = oracle_yardstick(build, model, tail, scheme)
    assert int(z.params.integrator) == scheme and z.n % 64 == tail
    path_conditions(z, c, own, tiled=(build == "tile"))
    r = gpu_run(build, model, "fast", tail, scheme)
    fails = _check_step(f"step fast {build} {model} tail={tail} scheme={scheme}", pkg, z, own, r["stepped"])
    assert (r["stepped"]["voxelID"][z.tail] != z.builder.arrays["voxelID"][z.tail]).all()
    assert not fails, fails


def _fp32_update(z, a, al):
    """fl(fl(a + G) h) and fl(alpha h) in fp32, as integrate_owner states them (compiled without contraction)"""
    p = z.params
    g, h = np.array([p.Gx, p.Gy, p.Gz], np.float32), np.float32(p.h)
    return ((a.astype(np.float32) + g[None, :]) * h).astype(np.float32), (al.astype(np.float32) * h).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("build,mode", [("tile", "exact"), ("tile", "fast"), ("general", "fast")])
def test_the_two_gathers_agree_bit_for_bit(pkg, orc, build, mode):
    """(c) "gather_owner == gather_block bit for bit": fl(fl(a + G) h) from the stand-alone reduction's downloaded a is the new
    velocity of every hub at rest after step(1), and fl(alpha h) its new angular velocity -- in both arithmetic modes: integrate_owner
    and acc_from_world are compiled without contraction (-ffp-contract=off; deme_kernels.h carries no fp contract pragma)"""
    z, c, ref, ro, own, lists = oracle_yardstick(build, "hertz")
    r = gpu_run(build, "hertz", mode)
    v, w = _fp32_update(z, r["a"], r["al"])
    hubs = z.hub
    V1, W1 = _vec(r["stepped"], V_), _vec(r["stepped"], W_)
    bad = np.nonzero((v[hubs] != V1[hubs]).any(1) | (w[hubs] != W1[hubs]).any(1))[0]
    record_measured(f"test_owner_zoo two gathers {build} {mode}", hubs=len(hubs), differing=len(bad))
    assert len(bad) == 0, [(int(hubs[i]), int(z.hub_k[i]), z.hub_role[i], z.hub_kind[i]) for i in bad[:10]]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_staged_step_equals_the_stepping_loop(pkg, orc, mode):
    """(d) calc_forces then integrate() (k_integrate<false>) leaves the state step(1) leaves, bit for bit"""
    r = gpu_run("tile", "hertz", mode)
    for k in STATE:
        assert np.array_equal(r["staged"][k], r["stepped"][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_closed_tiles_fused_step(pkg, orc, model):
    """k_tile_step<M> (every tile closes: k <= 64) against the float64 step and against the unfused context, per owner"""
    z, c, ref, ro, own, lists = oracle_yardstick("closed", model)
    path_conditions(z, c, own, tiled=True)
    rf, ru = gpu_run("closed", model, "fast", fused=True), gpu_run("closed", model, "fast")
    fails = _check_step(f"closed fused step {model}", pkg, z, own, rf["stepped"])
    fails += _check_step(f"closed unfused step {model}", pkg, z, own, ru["stepped"])
    fails += _check_sums(f"closed standalone {model}", z, own, ru["a"], ru["al"])
    # fused against unfused: each within its bound of the float64 step; together within two
    h = float(z.params.h)
    for names, b, s in ((V_, own["ba"], own["sa"]), (W_, own["bl"], own["sl"])):
        x, y = _vec(rf["stepped"], names).astype(np.float64), _vec(ru["stepped"], names).astype(np.float64)
        lim = 2 * (b * s * h + 2 * U24 * np.abs(y).max(1))
        assert (np.abs(x - y).max(1) <= lim).all(), names
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["hertz", "frictionless"])
def test_exact_mode_against_the_oracle(pkg, orc, model):
    """non-heavy owners: a / alpha and the state after one step bit-identical to the oracle; heavy free hubs (k > 256: the tree of
    k_reduce_heavy sums the same fp32 terms in another order) within (k + 2) 2^-24 of S, and their new velocities within that times h"""
    z, c, ref, ro, own, lists = oracle_yardstick("tile", model)
    r = gpu_run("tile", model, "exact")
    k = own["k"]
    light, heavy = k <= HEAVY, np.nonzero(k > HEAVY)[0]
    assert len(heavy) == 27 and (k[z.hub] == HEAVY).sum() == 9
    assert np.array_equal(r["a"][light], ro["a"][light].astype(np.float32)) and np.array_equal(r["al"][light], ro["al"][light].astype(np.float32))
    for which in ("staged", "stepped"):
        for name in STATE:
            assert np.array_equal(r[which][name][light], ro["state"][name][light]), (which, name)
    ea = _rel(r["a"][heavy].astype(np.float64), ro["a"][heavy], own["sa"][heavy])
    el = _rel(r["al"][heavy].astype(np.float64), ro["al"][heavy], own["sl"][heavy])
    lim = (k[heavy] + 2.0) * U24
    record_measured(f"test_owner_zoo exact heavy {model}", a_over_limit=float((ea / lim).max()), alpha_over_limit=float((el / lim).max()))
    assert (ea <= lim).all() and (el <= lim).all(), (ea / lim, el / lim)
    h = float(z.params.h)
    for names, s in ((V_, own["sa"]), (W_, own["sl"])):
        x, y = _vec(r["stepped"], names)[heavy].astype(np.float64), _vec(ro["state"], names)[heavy].astype(np.float64)
        assert (np.abs(x - y).max(1) <= lim * s[heavy] * h + 2 * U24 * np.abs(y).max(1)).all(), names
    fails = _check_sums(f"standalone exact tile {model}", z, own, r["a"], r["al"])
    fails += _check_step(f"step exact tile {model}", pkg, z, own, r["stepped"])
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("build,model", CASES)
def test_linear_momentum_per_star(pkg, orc, build, model):
    """sum of m a over a star's hub and satellites (the downloaded a carries no gravity) is zero within the sum of its members'
    bounds: a contribution credited to the wrong owner, which per-owner checks on a symmetric star could miss"""
    z, c, ref, ro, own, lists = oracle_yardstick(build, model)
    r = gpu_run(build, model, "fast")
    ns = int(z.star_of.max()) + 1
    in_star = z.star_of >= 0
    P, L = np.zeros((ns, 3)), np.zeros(ns)
    np.add.at(P, z.star_of[in_star], (r["a"].astype(np.float64) * z.mass[:, None])[in_star])
    np.add.at(L, z.star_of[in_star], (own["ba"] * own["sa"] * z.mass)[in_star])
    e = np.abs(P).max(1)
    live = L > 0
    record_measured(f"test_owner_zoo momentum {build} {model}", over_bound=float((e[live] / L[live]).max()))
    assert (e <= L).all(), float((e[live] / L[live]).max())
    assert not r["a"][~in_star].any() and not r["al"][~in_star].any()   # the tail touches nothing
