"""The detection zoo: contact lists and history maps of DESIGNED scenes against the all-pairs float64 statement (tests/_detect64.py).

The bed tests compare the detection with an oracle that restates the same algorithm (bin spans, the contact-point-in-this-bin rule):
a fault of the scheme is shared by both sides, and the structural edges of k_sweep are reached by luck.  Here every scene is written
onto the position codec's integer lattice (bin size a whole number of lattice units, codec fields overwritten after Initialize(), as
test_contact_zoo.build_zoo does), the margins come from set_margins, and the expected list is the statement's: no bins in it.  Everything
is integer or bit equality.  The statement's grey band (pairs within 2^-22 of the radius sum of their threshold) is EMPTY in every
scene -- a CPU test asserts it -- so nothing is excluded from any comparison.

SCENE P, population rows (k_sweep's cyclic pairing, windows, output buffer; k_segment_rank_sort).  A row is a list of populations;
cluster c has n spheres of radius 0.2 bin at distinct lattice points inside a cube of 0.1 bin at the centre of bin (c, 0, 0) -- the
smallest bin ids of the scene, so the incidence list is the clusters one after the other and bin c starts at the running sum of the
populations before it.  Every sphere lies inside its bin (one incidence); all n (n - 1) / 2 pairs overlap and have their contact
point in the bin: a lost or doubled pair of the pairing f = (m - 1) n + k is a lost or doubled contact.
  (2, 3, 4, 63, 64, 65, 127, 128, 129)   the half round of even n; c2 = (uint32_t)(64.5f * rn) going 1 -> 1 -> 0; n around 128
  (511,) (512,) (255, 256) (255, 257)    start + n = 511 (LDS) and 512 (giant) from starts 0 and 255: `end >= SW_W`
  (200, 1100, 5)                         a giant bin that begins mid-window, covers whole later windows (which must do nothing), a small
                                         bin after it; sphere 0's 1099 partners are one segment of k_segment_rank_sort
  (256,) (256, 256) (1,) ()              list end on a window edge, a lone entry, an empty list
  (40,) * 30                             780 keys per bin, ~5000 per window against SW_OUT = 256: sweep_emit's spill and sweep_flush's
                                         min(nOut, SW_OUT)
SCENE G, pair geometry (pair_near_f / sweep_radius, bin_range, point_bin): 21 classes of 96 isolated pairs in bins of ~1 cm, small
radius 1 mm.  Inside EVERY class the pairs sit at depth - threshold = +-2, +-8 and +-1000 grey bands (16 of each): the fp32
pre-filter must keep the +2 ones, the exact test must drop the -2 ones.
  interior, cross1 / cross2 / cross3 (the centres on two sides of one, two, three bin planes), face (contact point ON a bin face),
  first_x / _y / _z and last_x / _y / _z (the last bin of every axis is partial: the domain is no multiple of the bin), voxel (codec
  fields 65535 and 0), corner (the far corner of the bin, pairs along its diagonal: the largest fp32 coordinates and so the largest
  rounding that the pre-filter's slack has to cover), ratio_3, ratio_12 (the big centre 1.2 bins from the contact), ratio_300 (a 0.3 m sphere -- 61^3 bins, its centre
  30 bins from the contact point -- against 1 mm spheres, one with the smallest and one with the largest id of the scene),
  margin_owner (unequal per-owner margins), extra_fam (unequal family extra margins: the min rule), same_owner (two overlapping
  components of one clump: never listed), masked (two families masked against each other, overlapping: never listed), big (r = 0.8 bin:
  registered together in up to 27 bins, listed once).
  Built twice: with the masks and extra margins (familyTrivial false) and without any (familyTrivial true: the masked pairs ARE
  listed then, and the threshold of every pair is zero).  Owner ids are a permutation of the scene (either sphere of a pair may be A).
SCENE A, analytical objects (k_sphere_prep's `ob0 += 64`): 130 parallel planes and 4 cylinders (two posts, two drums; at list
positions 1, 63, 64 and 129), six spheres at the +-2, +-8, +-1000 bands of every object, run with the first 64, 65, 130 and all 134
objects.  sphere_entity rounds a plane's distance to fp32 and forms the cylinder's inflated radius in fp32, so the band of these
rows is 2^-22 x (R + |distance|), for a cylinder 2^-22 x (R + radius + distance from the axis).
HISTORY (k_history's gallop from c * nPrev / nNew, k_migrate): isolated pairs moved together or apart with upload_state between two
detections; nPrev -> nNew = 0 -> n, n -> 0, 1 -> n, n -> 1, n -> 10 n, 10 n -> n, identical, disjoint with all new keys below / above
the old ones, interleaved (n = 3000).  Every previous row carries wildcards that encode its row number; after migrate() mapped rows
must hold them bit for bit and new rows zero -- with the built-in model (4 wildcards: the float4 path) and with a run-time compiled
model of 2 (the general path).  The map's statement is a dict from the previous (A, B, type) to its row.

GPU variants of P and G: engine order off; engine order ON (fast arithmetic, scattered numbering, engine_order() asserted -- the
engine only reorders scenes of more than 256 clumps whose numbering is not compact already, so the single-cluster rows have no such
variant); the segmented key arena forced with DEME_KEY_SEG_MIN.

A FINDING of the first GPU run, fixed in csrc/deme_hip.hip: the row () -- a scene without a single owner -- launched k_set_ghost_bits
(and would have launched k_set_margins, k_margins, the integrators) with no workgroups.  That is a launch error which nobody looked
at, which stays in the runtime's state, and which the NEXT detection of the process reported as its own ("invalid configuration
argument" from the key sort of the (40,) * 30 row, in another context).  The owner-sized launches are skipped for such a scene now.

MUTATIONS of csrc/deme_kernels.h, each built and run ONCE on an MI355X through the caller-order cases of this file, and not kept.
Each was checked to stay inside its buffers before it ran.
  k_sweep        c1 = 64 - c2 n + 1 (off by one)                   8 population rows fail: all but (512,) (its bin is giant), (1,), ()
  k_sweep        the wrap j = min(j, j - n) gone (j clamped to     the same 8 rows
                 n - 1 so that the mutant stays inside LDS)
  k_sweep        giant bin if end > SW_W instead of >=             (200, 1100, 5) fails.  (512,) and (255, 257) PASS: their bin ends
                                                                   with the list at entry 512, which the LDS range holds exactly --
                                                                   the >= matters when the bin goes on past the window
  sweep_emit     the spill branch dropped (keys past SW_OUT lost)  9 rows fail: all but (1,) and ()
  sweep_radius   slack 0: return r                                 scene G fails in both flavours, by ONE contact: a +2-band pair of
                                                                   the corner class.  (Without that class the mutant passed: at 1 mm
                                                                   in 1 cm bins the fp32 rounding of the coordinates reaches two
                                                                   bands only in the far corner of a bin.)
  k_sphere_prep  key of object k instead of ob0 + k                scene A with 65, 130 and 134 objects fails; 64 passes
  k_history      lo = g + 4 instead of g + 1 after a low guess     "10n->n" fails (the guess c nPrev / nNew is three rows low there)
The unmutated library passes all 58 GPU cases.
"""
import functools

import numpy as np
import pytest

from tests import _detect64 as d64

NULL = 0xFFFFFFFF
K6 = (2, -2, 8, -8, 1000, -1000)
MAT = {"E": 1e8, "nu": 0.3, "CoR": 0.5, "mu": 0.3, "Crr": 0.0}


class Scene:
    pass


def _pkg():
    import __graft_entry__ as entry
    return entry.load_package()


def _builder(pkg, bins_per_world):
    """a 1 m box without walls; bin = M lattice units with world / bin = bins_per_world along x and y (not whole: the last bin of
    every axis is partial)"""
    b = pkg.SceneBuilder()
    b.LoadMaterial(dict(MAT))
    b.InstructBoxDomainDimension((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))
    b.InstructBoxDomainBoundingBC("none", 0)
    b.SetCDUpdateFreq(0)
    b.SetInitTimeStep(1e-6)
    nv, l, voxel = b._figure_out_nv()
    M = int((1 << (16 + min(nv))) / bins_per_world) | 1
    b.SetInitBinSize(M * l)
    return b, M, l, nv


def _finish(pkg, b, G, margins_clumps, n_clumps, M, l):
    """Initialize, write the clumps' lattice points into the codec fields, return the Scene"""
    p, _ = b.Initialize()
    assert p.l == l and abs(p.binSize - M * p.l) < 1e-18
    G = np.asarray(G, np.int64).reshape(-1, 3)
    assert len(G) == n_clumps and (G >= 0).all()
    assert all((G[:, k] < (1 << (16 + (p.nvXp2, p.nvYp2, p.nvZp2)[k]))).all() for k in range(3))
    vox = G // 65536
    A = b.arrays
    A["voxelID"][:n_clumps] = (vox[:, 0] + (vox[:, 1] << p.nvXp2) + (vox[:, 2] << (p.nvXp2 + p.nvYp2))).astype(np.uint64)
    for k, name in enumerate(("locX", "locY", "locZ")):
        A[name][:n_clumps] = (G[:, k] % 65536).astype(np.uint16)
    z = Scene()
    z.builder, z.params, z.M, z.n_clumps = b, p, M, n_clumps
    z.scene = pkg.abi.make_scene_struct(A, b.counts)
    z.margins = np.zeros(int(b.counts["nOwners"]), np.float32)
    z.margins[:len(margins_clumps)] = margins_clumps
    return z


def _statement(pkg, z, n_anal=None):
    return d64.expected(d64.inputs_of(z.builder.arrays, z.params, z.margins, pkg.model.mask_pair, n_anal))


def _placeholder(n):
    return np.full((n, 3), 0.5, np.float32)  # inside the box (Initialize warns otherwise); the codec fields are written afterwards


# ------------------------------------------------------------------------------------------------------------ scene P
ROWS = [(2, 3, 4, 63, 64, 65, 127, 128, 129), (511,), (512,), (255, 256), (255, 257), (200, 1100, 5), (256,), (256, 256), (1,), (),
        (40,) * 30]
ROWS_REORDERED = [r for r in ROWS if len(r) > 1 and sum(r) > 256]  # what the engine reorders: > 2 tiles, spread over several bins


def _row_id(r):
    return "empty" if not r else ("40x30" if len(r) == 30 else "-".join(str(x) for x in r))


@functools.lru_cache(maxsize=None)
def scene_p(row, numbering):
    pkg = _pkg()
    rng = np.random.default_rng(4000 + 7 * len(row) + sum(row))
    b, M, l, _ = _builder(pkg, 60.7)
    t = b.LoadSphereType(1e-3, 0.2 * M * l, 0)
    n = sum(row)
    G, cluster = np.zeros((n, 3), np.int64), np.zeros(n, np.int64)
    at = 0
    for c, pop in enumerate(row):
        half = int(0.05 * M)
        off = np.zeros((0, 3), np.int64)
        while len(off) < pop:  # distinct lattice points
            off = np.unique(np.concatenate([off, rng.integers(-half, half + 1, (pop - len(off), 3))]), axis=0)
        off = off[rng.permutation(pop)]  # (np.unique left them in spatial order: ids inside a cluster are a permutation of it)
        G[at:at + pop] = np.array([c * M + M // 2, M // 2, M // 2]) + off
        cluster[at:at + pop] = c
        at += pop
    if numbering == "scattered":  # ids scattered over the whole row
        order = rng.permutation(n)
        G, cluster = G[order], cluster[order]
    if n:
        b.AddClumps(t, _placeholder(n))
    z = _finish(pkg, b, G, np.zeros(n, np.float32), n, M, l)
    z.cluster, z.row = cluster, row
    return z


@functools.lru_cache(maxsize=None)
def statement_p(row, numbering):
    return _statement(_pkg(), scene_p(row, numbering))


# ------------------------------------------------------------------------------------------------------------ scene G
N_G = 96
R1 = 1e-3
G_CLASSES = ("interior", "cross1", "cross2", "cross3", "face", "first_x", "first_y", "first_z", "last_x", "last_y", "last_z", "voxel",
             "corner",
             "ratio_3", "ratio_12", "ratio_300", "margin_owner", "extra_fam", "same_owner", "masked", "big")
EXTRA = {1: 3e-5, 2: 8e-5}
BIG_AT = (31.5, 89.5)  # centres of the two 0.3 m spheres, in bins, on the diagonal
PITCH = 6              # pair cells: contact point in bin 6 c + 2 of every axis


@functools.lru_cache(maxsize=None)
def scene_g(families):
    pkg = _pkg()
    rng = np.random.default_rng(515)
    b, M, l, nv = _builder(pkg, 120.7)
    f32 = lambda x: float(np.float32(x))
    bin_m = M * l
    radii = [R1, 3 * R1, 12 * R1, 0.3, 0.8 * bin_m]
    tmpl = [b.LoadSphereType(1e-3, r, 0) for r in radii]
    tmpl.append(b.LoadClumpType(2e-3, (1e-9, 1e-9, 1e-9), [R1, R1], [[0.4e-3, 0, 0], [-0.4e-3, 0, 0]], 0))
    radii = [f32(r) for r in radii]
    if families:
        for fam, e in EXTRA.items():
            b.SetFamilyExtraMargin(fam, e)
        b.DisableContactBetweenFamilies(3, 4)
    nbx = (1 << (16 + nv[0])) // M  # index of the last (partial) bin of x and y; z has twice the range
    last = [((1 << (16 + nv[k])) // M) for k in range(3)]
    assert nbx == 120 and all(((1 << (16 + nv[k])) % M) > 0.3 * M for k in range(3))
    r_big_bins = 0.3 / bin_m

    def clear_of_big(pb, reach):
        c = np.asarray(pb, np.float64) + 0.5
        return all(np.linalg.norm(c - np.full(3, q)) > r_big_bins + reach for q in BIG_AT)

    cells = [(cx, cy, cz) for cx in range(20) for cy in range(20) for cz in range(20)
             if clear_of_big((PITCH * cx + 2, PITCH * cy + 2, PITCH * cz + 2), 4.0)]
    cells = [cells[i] for i in rng.permutation(len(cells))]
    edge2d = {}  # (class) -> free (c1, c2) cells of the face of the grid the class lives on

    def next_bin(cls):
        if cls[:-1] in ("first_", "last_"):
            ax = "xyz".index(cls[-1])
            if cls not in edge2d:
                edge2d[cls] = [(a, c) for a in range(19) for c in range(19)]
                edge2d[cls] = [edge2d[cls][i] for i in rng.permutation(361)]
            while True:
                a, c = edge2d[cls].pop()
                pb = [PITCH * a + 5, PITCH * c + 5]  # between the cells of the other classes: 3 bins from them along two axes
                pb.insert(ax, 0 if cls.startswith("first") else last[ax])
                if clear_of_big(pb, 3.0):
                    return np.array(pb, np.int64)
        return PITCH * np.array(cells.pop(), np.int64) + 2

    def unit(v):
        return v / np.linalg.norm(v)

    owners = []  # dict(t, G, m, fam, cls, k, pair)
    pairs = []   # dict(cls, k, listed (by design, with the families on), owners)

    def add(t, G, m, fam, cls, k, pair):
        owners.append(dict(t=t, G=np.asarray(G, np.int64), m=m, fam=fam, cls=cls, k=k, pair=pair))
        return len(owners) - 1

    def place(cls, k, Pu, u, tA, tB, mA=0.0, mB=0.0, fA=0, fB=0, thres=0.0, symmetric=False, never=False):
        """a pair whose contact point (as the engine computes it, from B's side) is the lattice point Pu and whose depth is
        thres + k grey bands; the first sphere is XB + D u"""
        RA, RB = radii[tA] + f32(mA), radii[tB] + f32(mB)
        depth = thres + k * d64.BAND * (RA + RB)
        D = RA + RB - depth
        if symmetric:
            w = np.rint(0.5 * D * u / l).astype(np.int64)
            GA, GB = Pu + w, Pu - w
        else:
            GB = np.rint(Pu - (RB - 0.5 * depth) * u / l).astype(np.int64)
            GA = GB + np.rint(D * u / l).astype(np.int64)
        pi = len(pairs)
        ia, ib = add(tA, GA, mA, fA, cls, k, pi), add(tB, GB, mB, fB, cls, k, pi)
        pairs.append(dict(cls=cls, k=k, listed=(k > 0 and not never), owners=(ia, ib)))
        return ia, ib

    for cls in G_CLASSES:
        for i in range(N_G):
            k = K6[i % 6]
            if cls == "ratio_300":
                continue
            pb = next_bin(cls)
            frac = rng.uniform(0.3, 0.7, 3)
            u = unit(rng.normal(size=3))
            kw = {}
            tA = tB = 0
            if cls in ("cross1", "cross2", "cross3", "face"):
                nax = {"cross1": 1, "cross2": 2, "cross3": 3, "face": 1}[cls]
                axes = rng.permutation(3)[:nax]
                u = 0.1 * rng.normal(size=3)
                u[axes] = rng.choice([-1.0, 1.0], nax)
                u = unit(u)
                frac[axes] = 0.0 if cls == "face" else 0.02
                kw["symmetric"] = cls == "face"
            elif cls[:-1] in ("first_", "last_"):
                ax = "xyz".index(cls[-1])
                if cls.startswith("last"):
                    frac[ax] = rng.uniform(0.1, 0.2)
                    u[ax] *= 0.2
                    u = unit(u)
            elif cls == "voxel":
                u = np.array([rng.choice([-1.0, 1.0]), 0.0, 0.0])
            elif cls == "corner":  # the far corner of the bin: the largest fp32 coordinates the pre-filter sees, along the diagonal
                frac = rng.uniform(0.86, 0.93, 3)
                u = unit(rng.choice([-1.0, 1.0]) * np.ones(3) + 0.15 * rng.normal(size=3))
            elif cls == "ratio_3":
                tA, tB = (0, 1) if i % 2 else (1, 0)
            elif cls == "ratio_12":
                tA, tB = (0, 2) if i % 2 else (2, 0)
            elif cls == "margin_owner":
                kw.update(dict(zip(("mA", "mB"), [(2e-5, 7e-5), (1.3e-4, 0.0), (5e-5, 1.1e-4), (0.0, 9e-5)][(i // 6) % 4])))
            elif cls == "extra_fam":
                fA, fB = (1, 2) if (i // 6) % 2 else (2, 1)
                kw.update(mA=1e-4, mB=1e-4, fA=fA, fB=fB, thres=f32(EXTRA[1]))
            elif cls == "masked":
                kw.update(fA=3, fB=4, never=True)
                k = 1000 * 300  # 0.3 mm deep
            elif cls == "big":
                tA = tB = 4
            Pu = pb * M + np.rint(frac * M).astype(np.int64)
            if cls == "same_owner":
                pairs.append(dict(cls=cls, k=0, listed=False, owners=(add(5, Pu, 0.0, 0, cls, 0, len(pairs)),)))
                continue
            ia, ib = place(cls, k, Pu, u, tA, tB, **kw)
            if cls == "voxel":  # codec fields at the ends of their range; the pair's axis is x, so the distance is untouched
                for o in (owners[ia], owners[ib]):
                    o["G"][1] = (o["G"][1] // 65536) * 65536 + 65535
                    o["G"][2] = (o["G"][2] // 65536) * 65536
                shift = 65535 - owners[ia]["G"][0] % 65536
                owners[ia]["G"][0] += shift
                owners[ib]["G"][0] += shift
    # the two 0.3 m spheres and their 48 small partners each, spread evenly over the surface
    big_owner = []
    for q in BIG_AT:
        Cb = np.rint(np.full(3, q) * M).astype(np.int64)
        ib = add(3, Cb, 0.0, 0, "ratio_300", 0, -1)
        big_owner.append(ib)
        for j in range(N_G // 2):
            k = K6[j % 6]
            zc = 1.0 - 2.0 * (j + 0.5) / (N_G // 2)
            ph = j * np.pi * (3.0 - np.sqrt(5.0))
            w = np.array([np.sqrt(1 - zc * zc) * np.cos(ph), np.sqrt(1 - zc * zc) * np.sin(ph), zc])
            Rs = radii[3] + radii[0]
            D = Rs - k * d64.BAND * Rs
            ia = add(0, Cb + np.rint(D * w / l).astype(np.int64), 0.0, 0, "ratio_300", k, len(pairs))
            pairs.append(dict(cls="ratio_300", k=k, listed=k > 0, owners=(ia, ib)))
    # ---- numbering: a permutation of the scene, one big sphere first and one last
    n = len(owners)
    rest = [i for i in rng.permutation(n) if i not in big_owner]
    order = [big_owner[0]] + rest + [big_owner[1]]
    new_id = np.zeros(n, np.int64)
    new_id[order] = np.arange(n)
    ow = [owners[i] for i in order]
    batch = b.AddClumps([tmpl[o["t"]] for o in ow], _placeholder(n))
    batch.SetFamily(np.array([o["fam"] for o in ow], np.uint8))
    z = _finish(pkg, b, np.array([o["G"] for o in ow]), np.array([o["m"] for o in ow], np.float32), n, M, l)
    z.pairs = [dict(q, owners=tuple(int(new_id[i]) for i in q["owners"])) for q in pairs]
    z.owner_cls = [o["cls"] for o in ow]
    z.families = families
    return z


@functools.lru_cache(maxsize=None)
def statement_g(families):
    return _statement(_pkg(), scene_g(families))


# ------------------------------------------------------------------------------------------------------------ scene A
N_PLANES, DZ, Z0 = 130, 4e-3, 0.3
CYL_AT = {1: ("post", (0.40, 0.75), 0.010), 63: ("drum", (0.60, 0.60), 0.50), 64: ("post", (0.80, 0.75), 0.020), 129: ("drum", (0.61, 0.60), 0.53)}
N_ANAL_ALL = N_PLANES + len(CYL_AT)
N_ANAL = (64, 65, 130, N_ANAL_ALL)


@functools.lru_cache(maxsize=None)
def scene_a(n_anal):
    """positions below are relative to the corner of the bin grid (user coordinates + 0.1 m); the objects' own records are read back
    from the scene arrays, so the spheres are designed against the fp32 values the engine gets"""
    pkg = _pkg()
    b, M, l, _ = _builder(pkg, 120.7)
    t = b.LoadSphereType(1e-3, R1, 0)
    b.SetFamilyExtraMargin(1, 2e-5)
    b.SetFamilyExtraMargin(2, 1e-5)
    f32 = lambda x: float(np.float32(x))
    lbf = -0.1
    objs = []  # (kind, data) in list order
    jp = 0
    for i in range(N_ANAL_ALL):
        if i in CYL_AT:
            kind, xy, rad = CYL_AT[i]
            o = b.AddExternalObject()
            o.AddCylinder((xy[0] + lbf, xy[1] + lbf, 0.0), (0, 0, 1), rad, 0, normal_inward=(kind == "drum"))
            objs.append((kind, o))
        else:
            o = b.AddBCPlane((0.5, 0.5, Z0 + DZ * jp + lbf), (0, 0, 1), 0)
            if jp % 3 == 0:
                o.SetFamily(2)
            objs.append(("plane", o))
            jp += 1
    obj_margin = [(0.0, 5e-5, 1.2e-4)[i % 3] for i in range(N_ANAL_ALL)]
    # object positions as the engine has them: the owner's lattice point + the fp32 offset.  Every object owner starts at the
    # user's origin, whose lattice point is that of (0 - lbf) in fp32 arithmetic, truncated: read from a probe scene.
    probe, *_ = _builder(pkg, 120.7)
    probe.LoadSphereType(1e-3, R1, 0)
    probe.AddBCPlane((0, 0, 0), (0, 0, 1), 0)
    pp, _ = probe.Initialize()
    origin = d64.lattice_of(probe.arrays, pp)[0].astype(np.float64) * l  # metres from the grid's corner
    G, margins, fams, design = [], [], [], []
    n_sph = 0
    for i, (kind, o) in enumerate(objs):
        mo = f32(obj_margin[i])
        fam_o = o.family
        for j, k in enumerate(K6):
            ms = (0.0, 3e-5)[(i + j) % 2]
            R = f32(R1) + f32(ms)
            thres = min(f32(2e-5), f32(1e-5) if fam_o == 2 else 0.0)
            if kind == "plane":
                pz = origin[2] + float(np.float32(o.comps[0][1][2]))
                dist = R + mo - thres                       # where depth = threshold; the band is 2^-22 (R + |dist|)
                dist -= k * d64.BAND * (R + dist)
                q = n_sph
                X = np.array([0.32 + 0.015 * (q % 40), 0.32 + 0.015 * (q // 40), pz + dist])
            else:
                _, xy, rad = CYL_AT[i]
                ax = origin[:2] + np.array([float(np.float32(xy[0] + lbf)), float(np.float32(xy[1] + lbf))])
                rad = f32(rad)
                sgn = 1.0 if kind == "drum" else -1.0
                # depth = R + mo - sgn (rad - dr) = thres + k band, band = 2^-22 (R + rad + dr)
                dr = rad - sgn * (R + mo - thres)
                dr += sgn * k * d64.BAND * (R + rad + dr)
                th = 2 * np.pi * (j + 0.37 * (i % 7)) / 6.0
                X = np.array([ax[0] + dr * np.cos(th), ax[1] + dr * np.sin(th), 0.95 + 0.004 * j])
            G.append(np.rint(X / l).astype(np.int64))
            margins.append(ms)
            fams.append(1)
            design.append((i, k))
            n_sph += 1
    # keep the first n_anal objects only (the spheres stay: those of a missing object touch nothing of it)
    b.ext_objs = [o for _, o in objs[:n_anal]]
    batch = b.AddClumps(t, _placeholder(n_sph))
    batch.SetFamily(np.array(fams, np.uint8))
    z = _finish(pkg, b, np.array(G), np.array(margins, np.float32), n_sph, M, l)
    z.margins[n_sph:n_sph + n_anal] = obj_margin[:n_anal]
    z.design, z.n_anal = design, n_anal
    assert int(b.counts["nAnal"]) == n_anal
    return z


@functools.lru_cache(maxsize=None)
def statement_a(n_anal):
    return _statement(_pkg(), scene_a(n_anal))


# ------------------------------------------------------------------------------------------------------------ history
N_H = 3000
MEMBERS = {"none": lambda i: i < 0, "all": lambda i: i >= 0, "one": lambda i: i == N_H // 2, "tenth": lambda i: i % 10 == 3,
           "upper": lambda i: i >= N_H, "lower": lambda i: i < N_H, "not0": lambda i: i % 3 != 0, "not1": lambda i: i % 3 != 1}
HISTORY = {  # name -> (pairs of the universe, previous set, new set, nPrev, nNew)
    "0->n": (N_H, "none", "all", 0, N_H),
    "n->0": (N_H, "all", "none", N_H, 0),
    "1->n": (N_H, "one", "all", 1, N_H),
    "n->1": (N_H, "all", "one", N_H, 1),
    "n->10n": (10 * N_H, "tenth", "all", N_H, 10 * N_H),
    "10n->n": (10 * N_H, "all", "tenth", 10 * N_H, N_H),
    "identical": (N_H, "all", "all", N_H, N_H),
    "new below": (2 * N_H, "upper", "lower", N_H, N_H),
    "new above": (2 * N_H, "lower", "upper", N_H, N_H),
    "interleaved": (N_H + N_H // 2, "not0", "not1", N_H, N_H),
}
_H_STATEMENTS = {}  # (universe, set) -> the all-pairs statement of that state, shared by the cases that use it


@functools.lru_cache(maxsize=None)
def scene_h(case, n_wild):
    """pairs (2 i, 2 i + 1) on a grid of pitch 3 bins; a pair of a set touches (centres 1.8 r apart), any other is 3 r apart.  Returns
    the scene in the PREVIOUS state and the codec fields of the new one"""
    pkg = _pkg()
    n_pairs, in_prev, in_new = HISTORY[case][0], MEMBERS[HISTORY[case][1]], MEMBERS[HISTORY[case][2]]
    b, M, l, _ = _builder(pkg, 120.7)
    if n_wild == 2:
        from tests.test_force_hook import PLAIN
        b.DefineContactForceModel(PLAIN)
        b.SetPerContactWildcards(["zoo_a", "zoo_b"])
    t = b.LoadSphereType(1e-3, R1, 0)
    i = np.arange(n_pairs)
    side = 36
    assert n_pairs <= side ** 3
    C = (np.stack([i % side, (i // side) % side, i // (side * side)], 1) * 3 + 2) * M + M // 3
    r_u = R1 / l

    def lattice(member):
        gap = np.where(member(i), 1.8, 3.0) * r_u
        G = np.zeros((2 * n_pairs, 3), np.int64)
        G[0::2], G[1::2] = C, C
        G[1::2, 0] += np.rint(gap).astype(np.int64)
        return G
    b.AddClumps(t, _placeholder(2 * n_pairs))
    z = _finish(pkg, b, lattice(in_prev), np.zeros(2 * n_pairs, np.float32), 2 * n_pairs, M, l)
    assert int(z.params.nContactWildcards) == n_wild
    z.new_state = {k: np.array(b.arrays[k], copy=True) for k in
                   ("voxelID", "locX", "locY", "locZ", "oriQw", "oriQx", "oriQy", "oriQz", "vX", "vY", "vZ", "omgBarX", "omgBarY", "omgBarZ")}
    Gn = lattice(in_new)
    vox = Gn // 65536
    p = z.params
    z.new_state["voxelID"][:2 * n_pairs] = (vox[:, 0] + (vox[:, 1] << p.nvXp2) + (vox[:, 2] << (p.nvXp2 + p.nvYp2))).astype(np.uint64)
    for k, name in enumerate(("locX", "locY", "locZ")):
        z.new_state[name][:2 * n_pairs] = (Gn[:, k] % 65536).astype(np.uint16)

    def designed(member):
        j = np.nonzero(member(i))[0]
        return (2 * j).astype(np.uint32), (2 * j + 1).astype(np.uint32), np.full(len(j), 1, np.uint8)
    z.prev_list, z.new_list = designed(in_prev), designed(in_new)
    z.n_wild = n_wild
    return z


def _row_codes(n, w):
    """wildcard w of row c: a value that names (c, w), exact in fp32, never zero"""
    return (np.arange(n, dtype=np.float32) * np.float32(4.0) + np.float32(w + 1)).astype(np.float32)


def _run_history(z, side, compile_into=None):
    """two detections around upload_state; returns (previous list, new list with the map, wildcards after migrate)"""
    side.set_margins(z.margins)
    side.detect()
    side.migrate()
    prev = side.contacts()
    n = len(prev[0])
    for w in range(z.n_wild):
        side.set_wildcard(w, _row_codes(n, w))
    side.upload_state(z.new_state)
    side.detect()
    new = side.contacts()
    side.migrate()
    wild = [side.wildcard(w) for w in range(z.n_wild)]
    return prev, new, wild


def _check_history(z, prev, new, wild):
    assert all(np.array_equal(a, b) for a, b in zip(prev[:3], z.prev_list)), "previous list"
    assert all(np.array_equal(a, b) for a, b in zip(new[:3], z.new_list)), "new list"
    want = d64.history_map(prev, new)
    assert np.array_equal(new[3], want)
    mapped = want != NULL
    for w in range(z.n_wild):
        codes = _row_codes(len(prev[0]), w)
        expect = np.zeros(len(want), np.float32)
        expect[mapped] = codes[want[mapped]]
        assert np.array_equal(wild[w].view(np.uint32), expect.view(np.uint32)), ("wildcard", w)


# ------------------------------------------------------------------------------------------------------------ CPU tests
def _oracle_list(pkg, orc, z):
    sim = orc.make_sim(pkg, z.params, z.scene)
    sim.set_margins(z.margins)
    sim.detect()
    out = sim.contacts(), sim.bin_incidence(), (int(sim.counts().nActiveBins), int(sim.counts().maxSpheresInBin))
    sim.close()
    return out


_oracle_cached = functools.lru_cache(maxsize=None)(lambda kind, *key: _oracle_list(_pkg(), __import__("__graft_entry__").load_oracle(),
                                                                                 {"p": scene_p, "g": scene_g, "a": scene_a}[kind](*key)))


def _same_list(got, want):
    assert len(got[0]) == len(want[0]), f"{len(got[0])} contacts, the statement has {len(want[0])}"
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)


def _strictly_increasing(lst):
    a, b, t = (np.asarray(x).astype(np.uint64) for x in lst[:3])
    cls = np.where(t == 1, 0, 2).astype(np.uint64)
    key = (a << np.uint64(33)) | (cls << np.uint64(31)) | b
    assert (key[1:] > key[:-1]).all()


@pytest.mark.parametrize("numbering", ["cluster", "scattered"])
@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_population_rows_design(pkg, orc, row, numbering):
    """grey band empty; the list is every unordered pair of every cluster, once; bin c starts at the running sum of the populations
    before it and holds exactly its cluster (the oracle's bin_incidence); the oracle's list is the statement's"""
    z = scene_p(row, numbering)
    want, grey = statement_p(row, numbering)
    assert grey == 0
    assert len(want[0]) == sum(n * (n - 1) // 2 for n in row)
    assert (z.cluster[want[0]] == z.cluster[want[1]]).all() and (want[0] < want[1]).all() and (want[2] == 1).all()
    _strictly_increasing(want)
    got, (bins, sph), (active, largest) = _oracle_cached("p", row, numbering)
    assert len(bins) == sum(row)  # one incidence per sphere
    start = 0
    for c, n in enumerate(row):
        assert (bins[start:start + n] == c).all()
        assert np.array_equal(sph[start:start + n], np.nonzero(z.cluster == c)[0])  # in sphere order: the sort by bin is stable
        start += n
    assert active == len(row) and largest == max(row, default=0)
    _same_list(got, want)


@pytest.mark.parametrize("families", [True, False], ids=["families", "trivial"])
def test_pair_geometry_design(pkg, orc, families):
    """grey band empty; 96 pairs per class; the statement lists exactly the pairs designed inside their threshold (+2, +8, +1000
    bands), never the same-owner clumps, the masked pairs only without the masks; the centres of the cross classes lie across one, two
    and three bin planes, the face class has its contact point on a face, the first / last classes sit in the first / last bin; the
    oracle's list is the statement's"""
    z = scene_g(families)
    want, grey = statement_g(families)
    assert grey == 0
    by_cls = {c: [q for q in z.pairs if q["cls"] == c] for c in G_CLASSES}
    assert all(len(v) == N_G for v in by_cls.values()), {c: len(v) for c, v in by_cls.items()}
    A = z.builder.arrays
    own = np.asarray(A["ownerClumpBody"], np.int64)
    got_pairs = set(zip(own[want[0]].tolist(), own[want[1]].tolist()))
    assert len(got_pairs) == len(want[0]) and (want[2] == 1).all()
    designed = set()
    for q in z.pairs:
        # (without the families the masked pairs are listed, and so is every extra_fam pair: its depth is within 1000 bands of 3e-5 m)
        if len(q["owners"]) == 2 and (q["listed"] or (q["cls"] in ("masked", "extra_fam") and not families)):
            designed.add((min(q["owners"]), max(q["owners"])))
    assert got_pairs == designed
    for c in G_CLASSES:  # both sides of the threshold in every class that has one
        if c not in ("same_owner", "masked"):
            assert sorted(set(q["k"] for q in by_cls[c])) == sorted(K6) and sum(q["listed"] for q in by_cls[c]) == N_G // 2
    assert (A["familyMasks"] != 0).any() == families and (A["familyExtraMarginSize"] != 0).any() == families
    # positions against the grid
    G = d64.lattice_of(A, z.params)
    M = z.M
    for c, nax in (("cross1", 1), ("cross2", 2), ("cross3", 3), ("interior", 0)):
        for q in by_cls[c]:
            ia, ib = q["owners"]
            assert int((G[ia] // M != G[ib] // M).sum()) == nax, (c, q)
    for q in by_cls["face"]:
        ia, ib = q["owners"]
        assert ((G[ia] + G[ib]) % (2 * M) == 0).any()
    last = [(1 << (16 + nv)) // M for nv in (z.params.nvXp2, z.params.nvYp2, z.params.nvZp2)]
    assert (int(z.params.nbX) - 1, int(z.params.nbY) - 1, int(z.params.nbZ) - 1) == tuple(last)
    for ax, name in enumerate("xyz"):
        for q in by_cls["first_" + name]:
            assert all(G[i][ax] // M == 0 for i in q["owners"])
        for q in by_cls["last_" + name]:
            assert all(G[i][ax] // M == last[ax] for i in q["owners"])
    for q in by_cls["voxel"]:
        assert all(G[i][0] % 65536 == 65535 or G[i][1] % 65536 == 65535 for i in q["owners"]) and all(G[i][2] % 65536 == 0 for i in q["owners"])
    big = [i for i, c in enumerate(z.owner_cls) if c == "ratio_300" and A["Radii"][A["clumpComponentOffset"][np.nonzero(own == i)[0][0]]] > 0.1]
    assert big == [0, z.n_clumps - 1]
    got, _, _ = _oracle_cached("g", families)
    _same_list(got, want)


@pytest.mark.parametrize("n_anal", N_ANAL)
def test_analytical_objects_design(pkg, orc, n_anal):
    """grey band empty (with the plane rows' band 2^-22 (R + |distance|)); every object present lists its three spheres inside the
    threshold and none of its three outside; the oracle's list is the statement's"""
    z = scene_a(n_anal)
    want, grey = statement_a(n_anal)
    assert grey == 0
    listed = set(zip(want[0].tolist(), want[1].tolist()))
    assert len(z.design) == 6 * N_ANAL_ALL
    for s, (obj, k) in enumerate(z.design):
        if obj < n_anal:
            assert ((s, obj) in listed) == (k > 0), (s, obj, k)
    types = {int(o): int(t) for o, t in zip(want[1], want[2])}
    assert all(types[o] == (13 if o in CYL_AT else 11) for o in types) and len(types) == n_anal
    got, _, _ = _oracle_cached("a", n_anal)
    _same_list(got, want)


@pytest.mark.parametrize("case", list(HISTORY))
def test_history_design(pkg, orc, case):
    """the designed lists are the all-pairs statement's in both states (grey band empty), and the oracle's history map and migrated
    wildcards are the dict's"""
    z = scene_h(case, 4)
    n_pairs, prev_key, new_key, n_prev, n_new = HISTORY[case]
    for key, state, lst in ((prev_key, None, z.prev_list), (new_key, z.new_state, z.new_list)):
        if (n_pairs, key) not in _H_STATEMENTS:
            arrays = dict(z.builder.arrays)
            if state is not None:
                arrays.update(state)
            _H_STATEMENTS[(n_pairs, key)] = d64.expected(d64.inputs_of(arrays, z.params, z.margins, pkg.model.mask_pair))
        want, grey = _H_STATEMENTS[(n_pairs, key)]
        assert grey == 0
        _same_list(want, lst)
    assert (len(z.prev_list[0]), len(z.new_list[0])) == (n_prev, n_new)
    for n_wild in (4, 2):
        zz = scene_h(case, n_wild)
        sim = orc.make_sim(pkg, zz.params, zz.scene)
        _check_history(zz, *_run_history(zz, sim))
        sim.close()


# ------------------------------------------------------------------------------------------------------------ GPU tests
VARIANTS = ("caller order", "engine order", "segmented arena")


def _context(pkg, z, variant, monkeypatch):
    if variant == "segmented arena":
        monkeypatch.setenv("DEME_KEY_SEG_MIN", "4096")
    ctx = pkg.Context(0)
    if variant == "engine order":
        ctx.set_arith_mode("fast")  # (the exact mode keeps the caller's order)
    else:
        ctx.set_reorder(False)
    ctx.set_params(z.params), ctx.upload_scene(z.scene)
    assert ctx.engine_order()[0] == (variant == "engine order"), ctx.engine_order()
    return ctx


def _check_detection(ctx, z, want, oracle):
    got_o, _, (active, largest) = oracle
    ctx.set_margins(z.margins)
    ctx.detect()
    got = ctx.contacts()
    _same_list(got, want)
    _same_list(got, got_o)
    _strictly_increasing(got)
    c = ctx.counts()
    assert int(c.nContacts) == len(want[0])
    assert (int(c.nActiveBins), int(c.maxSpheresInBin)) == (active, largest)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,row", [(v, r) for v in VARIANTS for r in (ROWS_REORDERED if v == "engine order" else ROWS)],
                         ids=lambda x: x if isinstance(x, str) else _row_id(x))
def test_population_rows(pkg, orc, monkeypatch, variant, row):
    numbering = "scattered" if variant == "engine order" else "cluster"
    z = scene_p(row, numbering)
    ctx = _context(pkg, z, variant, monkeypatch)
    _check_detection(ctx, z, statement_p(row, numbering)[0], _oracle_cached("p", row, numbering))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("families", [True, False], ids=["families", "trivial"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_pair_geometry(pkg, orc, monkeypatch, variant, families):
    z = scene_g(families)
    ctx = _context(pkg, z, variant, monkeypatch)
    _check_detection(ctx, z, statement_g(families)[0], _oracle_cached("g", families))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_anal", N_ANAL)
def test_analytical_objects(pkg, orc, monkeypatch, n_anal):
    z = scene_a(n_anal)
    ctx = _context(pkg, z, "caller order", monkeypatch)
    _check_detection(ctx, z, statement_a(n_anal)[0], _oracle_cached("a", n_anal))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_wild", [4, 2], ids=["builtin-4", "custom-2"])
@pytest.mark.parametrize("case", list(HISTORY))
def test_history_map_and_migration(pkg, orc, monkeypatch, case, n_wild):
    z = scene_h(case, n_wild)
    ctx = _context(pkg, z, "caller order", monkeypatch)
    if n_wild == 2:
        z.builder.compile_into(ctx)
    _check_history(z, *_run_history(z, ctx))
    ctx.close()
