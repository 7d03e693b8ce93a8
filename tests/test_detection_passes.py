"""The small passes of a contact detection (run with -m gpu on an MI355X): the two-level scan of the per-sphere bin counts (a sum per
workgroup of 256 spheres, one workgroup over the sums, the counts again in k_fill_incidence), the counters cleared by one fill or on
the side of the kernel before them, the read-backs that bring the counters in one copy, and the radix sort at its tile edges.

Everything here is integer work with one right answer: the comparisons are for equality.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R_SMALL, BIN = 0.001, 0.01


def _spheres(pkg, xyz, radii=None, cd_freq=0):
    """single spheres at xyz (metres, inside a 0.6 m box), bins of 1 cm, no margin beyond the owners' own speed (zero)"""
    import math
    b = pkg.model.SceneBuilder()
    mat = b.LoadMaterial({"E": 1e8, "nu": 0.3, "CoR": 0.6, "mu": 0.2, "Crr": 0.0})
    b.InstructBoxDomainDimension((0.0, 0.6), (0.0, 0.6), (0.0, 0.6))
    radii = np.full(len(xyz), R_SMALL) if radii is None else np.asarray(radii, float)
    tm = {float(r): b.LoadSphereType(2.6e3 * 4.0 / 3.0 * math.pi * r ** 3, float(r), mat) for r in np.unique(radii)}
    b.AddClumps([tm[float(r)] for r in radii], np.asarray(xyz, np.float32))
    b.SetInitTimeStep(5e-6)
    b.SetGravitationalAcceleration((0, 0, -9.81))
    b.SetCDUpdateFreq(cd_freq)
    b.SetInitBinSize(BIN)
    b.SetExpandSafetyAdder(0.0)
    b.SetMaxVelocity(5.0)
    b.SetErrorOutVelocity(1e3)
    return b


def _grid(n, pitch, origin=0.0205):
    """n points of a cubic grid, x fastest"""
    side = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    i = np.arange(n)
    return origin + pitch * np.stack([i % side, (i // side) % side, i // (side * side)], 1).astype(np.float64)


def _context(pkg, builder):
    p, sc = builder.Initialize()
    ctx = pkg.Context(0)
    ctx.set_params(p)
    ctx.upload_scene(sc)
    return ctx, p, sc


def _incidence_statement(ctx, p):
    """the (bin, sphere) list as numpy states it: every sphere's bins in z-y-x order, sphere-major (np.repeat), then a stable sort
    by bin id.  The spans are bin_range() of the kernels in the same fp64 operations, from the geometry the device computed; with
    zero margins the binning radius is the sweep radius."""
    X, Y, Z, R = ctx.sphere_geometry()
    bs = float(p.binSize)

    def span(pos, nb):
        b, s = pos / bs, R.astype(np.float64) / bs
        hi = np.where(b + s < float(nb), np.floor(b + s), nb - 1).astype(np.int64)
        lo = np.floor(np.maximum(b - s, 0.0)).astype(np.int64)
        return lo, hi - lo + 1

    (lx, nx), (ly, ny), (lz, nz) = span(X, p.nbX), span(Y, p.nbY), span(Z, p.nbZ)
    cnt = nx * ny * nz
    sph = np.repeat(np.arange(len(X), dtype=np.int64), cnt)
    k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)  # index inside the sphere's box
    i, j, kk = k % nx[sph], (k // nx[sph]) % ny[sph], k // (nx[sph] * ny[sph])
    bins = (lx[sph] + i) + (ly[sph] + j) * int(p.nbX) + (lz[sph] + kk) * int(p.nbX) * int(p.nbY)
    order = np.argsort(bins, kind="stable")
    return bins[order].astype(np.uint32), sph[order].astype(np.uint32), cnt


def _check_incidence(pkg, xyz, radii=None):
    ctx, p, sc = _context(pkg, _spheres(pkg, xyz, radii))
    try:
        ctx.compute_margins(0)
        ctx.detect()
        eb, es, cnt = _incidence_statement(ctx, p)
        gb, gs = ctx.bin_incidence()
        assert int(ctx.counts().nBinSphereTouches) == len(gb) == len(eb)  # the total the scan leaves = the list's length
        assert np.array_equal(gb, eb) and np.array_equal(gs, es)
        return cnt
    finally:
        ctx.close()


# 1 / 255 / 256 / 257: around one workgroup of k_sphere_prep; 65 537 = 256 * 256 + 1: 257 sums, the last of one sphere, past a wavefront
# of k_scan_small's threads (4 sums each).  A pitch of 3.3 mm puts some spheres across bin faces: counts of 1, 2, 4 and 8 mixed.
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_two_level_scan_sizes(pkg, n):
    cnt = _check_incidence(pkg, _grid(n, 0.0033))
    assert n < 255 or len(np.unique(cnt)) > 1


def test_two_level_scan_uneven_counts(pkg):
    """300 spheres (the second workgroup is partial) at bin centres, one bin each -- but the last sphere of the first workgroup
    reaches into 27: its neighbours' offsets, in its workgroup and in the next, move by 26"""
    xyz = _grid(300, BIN, origin=0.025)
    radii = np.full(300, R_SMALL)
    radii[255] = 0.008
    cnt = _check_incidence(pkg, xyz, radii)
    assert cnt[255] == 27 and (np.delete(cnt, 255) == 1).all()


def test_incidence_arena_grows_after_early_fill(pkg):
    """600 spheres of 8 mm at bin centres, 3 cm apart: every one reaches into 27 bins, 16 200 incidences against the arena of
    max(8 x 600, 4096) = 4800 slots the upload made.  k_fill_incidence has gone out before the host knows the total and stopped
    at the arena's end; the list must be the one filled again into the grown arena"""
    n = 600
    cnt = _check_incidence(pkg, _grid(n, 0.03, origin=0.025), np.full(n, 0.008))
    assert (cnt == 27).all() and int(cnt.sum()) == 16200 > max(8 * n, 4096)


def _dense(pkg, n=800, cd_freq=0):
    return pkg.model.packed_bed(n, seed=23, cd_freq=cd_freq, spacing_mult=1.5)  # (test_contact_arena_growth's scene: > 6 contacts a sphere)


def _snapshot(ctx):
    c = ctx.counts()
    return (int(c.nContacts), int(c.nBinSphereTouches), int(c.nActiveBins), int(c.maxSpheresInBin)), ctx.contacts()[:3], ctx.bin_incidence()


def _same(s1, s2):
    assert s1[0] == s2[0]
    for a, b in zip(s1[1] + s1[2], s2[1] + s2[2]):
        assert np.array_equal(a, b)


def test_folded_clears_two_detections(pkg):
    """nothing of the first detection is left in a counter the second one adds to; the first one here also grows the contact
    arena (the retry clears again)"""
    ctx, p, sc = _context(pkg, _dense(pkg))
    ctx.detect()
    one = _snapshot(ctx)
    assert one[0][0] > 6 * sc.nSpheres and one[0][0] == len(one[1][0])
    ctx.detect()
    _same(one, _snapshot(ctx))
    ctx.detect()
    _same(one, _snapshot(ctx))
    ctx.close()
    ctx2, *_ = _context(pkg, _dense(pkg))  # a fresh context: one detection alone
    ctx2.detect()
    _same(one, _snapshot(ctx2))
    ctx2.close()


# (spheres, pitch, safety adder, D, detections checked, pairs per sphere the list must exceed, pairs of the first list if stated)
ASYNC_BEDS = {
    # spheres 0.2 mm apart, margins of 0.15 mm from the safety velocity over K + D = 30 steps: the near pairs along the grid's axes
    "axis_pairs": (3000, 0.0022, 1.0, 10, 3, 1, None),
    # 10 x 10 x 10 spheres 0.02 mm apart.  A resting owner's margin is adder x h x drift (k_margins) = 3 x 5e-6 x drift: twice
    # that is 0.6 mm over the K steps of the first, lock-step detection -- the 2700 axis pairs, inside the 6 x 1000 slots the
    # upload gave the contact arena -- and 1.05 mm over K + D = 35, which takes in the face diagonals (gap 0.857 mm; the body
    # diagonals at 1.499 mm stay out): 7560 pairs (both counts from tests/_detect64.py), so the arena grows in part 1 of the
    # first asynchronous detection, beside the steps
    "arena_grows_beside_the_steps": (1000, 0.00202, 3.0, 15, 2, 6, 2700),
}


@pytest.mark.parametrize("bed_name", list(ASYNC_BEDS))
def test_folded_clears_async_detection(pkg, bed_name):
    """detections beside the steps (two lists, a stream of their own) on a bed that does not move (no gravity, no overlap).
    Every asynchronous detection must build the list that one lock-step detection with the same margins builds -- nothing left
    over from the detection before it"""
    K = 20
    n, pitch, adder, D, rounds, per_sphere, first = ASYNC_BEDS[bed_name]

    def bed():
        b = _spheres(pkg, _grid(n, pitch), cd_freq=K)
        b.SetGravitationalAcceleration((0, 0, 0))
        b.SetExpandSafetyAdder(adder)
        return b

    ref, *_ = _context(pkg, bed())
    ref.compute_margins(K + D)
    ref.detect()
    want = ref.contacts()[:3]
    nb, mx = int(ref.counts().nActiveBins), int(ref.counts().maxSpheresInBin)
    ref.close()
    assert len(want[0]) > per_sphere * n
    ctx, *_ = _context(pkg, bed())
    ctx.set_async_detection(D)
    ctx.set_timing(1)
    ctx.step(1)  # the first detection, in lock-step with margins for K steps
    assert first is None or int(ctx.counts().nContacts) == first < 6 * n
    for steps in (2 * K,) + (K,) * (rounds - 1):  # after the second, third ... detection
        ctx.step(steps)
        c = ctx.counts()
        got = ctx.contacts()[:3]
        assert int(c.nContacts) == len(got[0]) == len(want[0])
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert (int(c.nActiveBins), int(c.maxSpheresInBin)) == (nb, mx)
    assert int(ctx.counts().nDetections) >= rounds + 1
    assert ctx.kernel_time_ms("detect_async_part1")[1] >= 1  # (the asynchronous path really served)
    ctx.close()


@pytest.mark.parametrize("seg_min", ["4096", "0"])
def test_merged_readbacks_both_arenas(pkg, monkeypatch, seg_min):
    """the contact count comes back with the counters in one copy: from the 64 segment counts (segmented arena, forced onto this
    small scene) or from the single counter"""
    monkeypatch.setenv("DEME_KEY_SEG_MIN", seg_min)
    ctx, p, sc = _context(pkg, _dense(pkg, 1200))
    ctx.detect()
    ctx.detect()
    snap = _snapshot(ctx)
    ctx.close()
    monkeypatch.delenv("DEME_KEY_SEG_MIN")
    ref, *_ = _context(pkg, _dense(pkg, 1200))
    ref.detect()
    _same(snap, _snapshot(ref))
    assert snap[0][0] == len(snap[1][0]) > 6 * sc.nSpheres
    ref.close()


def _digit_order(keys, b0, b1):
    return np.argsort((keys.astype(np.uint64) >> np.uint64(b0)) & np.uint64((1 << (b1 - b0)) - 1), kind="stable")


def _patterns(n, b0, b1, dtype):
    bits = b1 - b0
    top = max(bits - 8, 0)  # the last pass's digit
    span = np.uint64(1) << np.uint64(bits)
    i = np.arange(n, dtype=np.uint64)
    noise = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(3)  # bits outside the range travel with the key
    outside = noise & ~(((span - np.uint64(1)) << np.uint64(b0)))
    if dtype == np.uint32:
        outside &= np.uint64(0xFFFFFFFF)
    yield "equal", np.full(n, (np.uint64(0x5A5A5) & (span - np.uint64(1))) << np.uint64(b0), np.uint64) | outside
    yield "descending", (((np.uint64(n) - i) % span) << np.uint64(b0)) | outside
    yield "top digit", (((i * np.uint64(7)) % (span >> np.uint64(top))) << np.uint64(b0 + top)) | outside


@pytest.mark.parametrize("b0,b1,wide", [(0, 20, False), (0, 21, False), (0, 22, False), (31, 55, True)])
def test_sort_tile_edges(pkg, b0, b1, wide):
    """the project's sort (force_own) at the edges of its tile, against numpy's stable argsort by the same bits"""
    T = pkg.abi.sort_tile_keys()
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 17):
        for name, k64 in _patterns(n, b0, b1, np.uint64 if wide else np.uint32):
            if wide:
                out = pkg.abi.sort_keys_u64(k64, b0, b1, force_own=True)
                assert np.array_equal(out, k64[_digit_order(k64, b0, b1)]), (name, n)
            else:
                keys, vals = k64.astype(np.uint32), np.arange(n, dtype=np.uint32)[::-1].copy()
                ko, vo = pkg.abi.sort_pairs_u32(keys, vals, b0, b1, force_own=True)
                order = _digit_order(keys, b0, b1)
                assert np.array_equal(ko, keys[order]) and np.array_equal(vo, vals[order]), (name, n)
