"""deme_tri_wear_enable / _sample / _read / _reset (Context.tri_wear_*): contact impulse, normal impulse, sliding work and shear work
of every mesh triangle, summed from sample to sample on the device, against tests/_tri_wear64.py applied to the whole-list downloads
and the owners' state as it stands.

The beds are those of tests/test_tri_loads.py.  Tolerance of a triangle's lane: |got - model| <= 1e-10 * abs_scale, abs_scale the sum
over the triangle's counted rows of the magnitudes before any cancellation (w |f| for lanes 0 to 3, w |f| (|v_A| + |w_A| |r_A| + |v_B|
+ |w_B| |r_B|) for lanes 4 and 5).  It is derived, not measured: both sides add the same fp64 terms in different orders, a sum of n
terms differs by at most n * 1.1e-16 of abs_scale with n < 1e5 (asserted by the model), and a term's own rounding is a few ulps of
its uncancelled magnitude.  The row counts are compared for equality."""
import ctypes as C

import numpy as np
import pytest

from tests._tri_wear64 import REL, tri_wear
from tests.test_mesh import mesh_bed
from tests.test_owner_contacts import _bed_scene, _stepped, _whole_list
from tests.test_tri_loads import STATE_KEYS, flat_bed, runs_of, stepped_mesh_bed, two_triangle_bed

THR = 1e-12  # what the shell passes (DEME_TINY_FLOAT_HOST)
SYMBOLS = tuple(f"deme_{m}tri_wear_{c}" for m in ("", "multi_") for c in ("enable", "sample", "read", "reset"))
LANES = ("impulse", "normalImpulse", "slidingWork", "shearWork")


def test_tri_wear_is_exported_and_bound(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in SYMBOLS:
        assert n in names and hasattr(lib, n), n
    for cls in (pkg.Context, pkg.abi.Multi):
        for meth in ("tri_wear_enable", "tri_wear_sample", "tri_wear_read", "tri_wear_reset"):
            assert hasattr(cls, meth), (cls.__name__, meth)
    assert len(lib.deme_tri_wear_sample.argtypes) == 4 and len(lib.deme_tri_wear_read.argtypes) == 9
    assert len(lib.deme_multi_tri_wear_sample.argtypes) == 4 and len(lib.deme_multi_tri_wear_read.argtypes) == 9
    assert pkg.abi.TRI_WEAR_COLUMNS == LANES + ("rows",)


def test_the_model_on_a_hand_written_list():
    """Four rows, one a triangle; w = 0.25.  Owners: 0 to 2 the spheres', 3 a resting face owner, 4 one moving along at 2 m/s.
    Triangles 0 to 2 lie in the z plane with the normal +z, triangle 3 is degenerate (n3 = n1).  f = (0.3, 0, -1) on the sphere, so
    g = (-0.3, 0, 1): Fn = 1, |gt| = 0.3.
      row 0  the sphere slides at 2 m/s along x over triangle 0: lanes 3, 4, 5 = w, 2 w, 0.6 w
      row 1  the same over triangle 1, whose owner moves along: lanes 4 and 5 are zero
      row 2  a sphere at rest spinning at 5 rad/s about y with its contact point 0.1 below its centre: |ut| = |w_A| |r_A| = 0.5
      row 3  the degenerate triangle: the impulse is counted, lanes 3 to 5 are zero"""
    w = 0.25
    f = np.array([[0.3, 0, -1]] * 4, np.float32)
    whole = {"idA": [0, 1, 2, 0], "idB": [0, 1, 2, 3], "type": [2, 2, 2, 2], "ownerA": [0, 1, 2, 0], "force": f,
             "cpA": np.array([[0, 0, -0.1]] * 4, np.float32), "cpB": np.zeros((4, 3), np.float32)}
    z = np.zeros(5, np.float32)
    state = {"oriQw": z + 1, "oriQx": z, "oriQy": z, "oriQz": z, "vX": np.array([2, 2, 0, 0, 2], np.float32), "vY": z, "vZ": z,
             "omgBarX": z, "omgBarY": np.array([0, 0, 5, 0, 0], np.float32), "omgBarZ": z}
    n1 = np.zeros((4, 3), np.float32)
    n2 = np.array([[1, 0, 0]] * 4, np.float32)
    n3 = np.array([[0, 1, 0]] * 3 + [[0, 0, 0]], np.float32)
    m = tri_wear(whole, state, (n1, n2, n3), [3, 4, 3, 3], None, 4, 0.0, w)
    g = -f[0].astype(np.float64)
    assert m["counted"].all() and m["rows"].tolist() == [1, 1, 1, 1] and m["rows"].dtype == np.uint64
    assert np.array_equal(m["lanes"][:, :3], np.tile(w * g, (4, 1)))
    assert np.allclose(m["lanes"][0, 3:], [w, 2 * w, 0.6 * w], rtol=1e-7, atol=0)  # (0.3 is its fp32 neighbour)
    assert m["lanes"][1, 3] == m["lanes"][0, 3] and m["lanes"][1, 4] == 0 and m["lanes"][1, 5] == 0
    assert np.allclose(m["lanes"][2, 3:], [w, 0.5 * w, 0.5 * 0.3 * w], rtol=1e-7, atol=0)
    assert (m["lanes"][3, 3:] == 0).all() and np.array_equal(m["lanes"][3, :3], w * g)
    fm = np.sqrt((g * g).sum())
    assert np.allclose(m["abs_scale"][0], [w * fm] * 4 + [w * fm * 2.0] * 2, rtol=1e-15)
    assert np.allclose(m["abs_scale"][1, 4:], w * fm * 4.0, rtol=1e-15) and np.allclose(m["abs_scale"][2, 4:], w * fm * 0.5, rtol=1e-15)
    assert abs(m["u_max"] - 2.0) < 1e-15
    # the threshold, a ghost's sphere and a triangle id past the mesh: not counted, as tests/_tri_loads64.py
    assert tri_wear(whole, state, (n1, n2, n3), [3, 4, 3, 3], None, 4, 2.0, w)["rows"].sum() == 0
    assert tri_wear(whole, state, (n1, n2, n3), [3, 4, 3, 3], [True, False, False, False, False], 4, 0.0, w)["rows"].tolist() == [0, 1, 1, 0]
    assert tri_wear(whole, state, (n1[:3], n2[:3], n3[:3]), [3, 4, 3], None, 3, 0.0, w)["rows"].tolist() == [1, 1, 1]


def model_of(ctx, sc, thr, w):
    k = sc._keep
    return tri_wear(_whole_list(ctx, sc), ctx.download_state(), (k["triNode1"], k["triNode2"], k["triNode3"]), k["ownerMesh"], None,
                    int(sc.nTri), thr, w)


def lanes_of(got):
    return np.concatenate([got["impulse"]] + [got[k][:, None] for k in LANES[1:]], 1)


def check(got, want_lanes, want_rows, scale, what):
    lanes = lanes_of(got)
    err = np.abs(lanes - want_lanes)
    ratio = (err / np.maximum(scale, 1e-300)).max(0)
    print(f"{what}: counted rows {int(want_rows.sum())}, loaded triangles {int((want_rows > 0).sum())}, worst |got - model| / abs_scale "
          f"per lane {np.array2string(ratio, precision=2)} (bound {REL:g})")
    assert got["rows"].dtype == np.uint64 and np.array_equal(got["rows"], want_rows), what
    assert lanes.dtype == np.float64 and lanes.shape == want_lanes.shape and (err <= REL * scale).all(), (what, ratio)


def scatter_motion(ctx, sc, seed=20):
    """drawn velocities and angular velocities on every owner, the mesh's included: a sample is a pure function of the records and
    the state as it stands, and a scatter leaves the records alone"""
    rng = np.random.default_rng(seed)
    n = int(sc.nOwners)
    rows = {k: rng.normal(0.0, 0.5, n).astype(np.float32) for k in ("vX", "vY", "vZ")}
    rows.update({k: rng.normal(0.0, 20.0, n).astype(np.float32) for k in ("omgBarX", "omgBarY", "omgBarZ")})
    ctx.scatter_owner_state(np.arange(n, dtype=np.uint32), rows)


@pytest.fixture(scope="module", params=["fast", "exact"])
def bed(pkg, request):
    ctx, p, sc = stepped_mesh_bed(pkg, mesh_bed(pkg, 1500), request.param)
    ctx.tri_wear_enable()
    yield {"ctx": ctx, "p": p, "sc": sc, "mode": request.param}
    ctx.close()


@pytest.mark.gpu
def test_one_sample_equals_the_model(bed):
    """mesh_bed after 180 steps with scattered motion: one sample each at thr 0 and at the shell's threshold, w = 0.25"""
    ctx, sc = bed["ctx"], bed["sc"]
    scatter_motion(ctx, sc)
    assert sc.nTri == 800
    for thr in (0.0, THR):
        want = model_of(ctx, sc, thr, 0.25)
        ctx.tri_wear_reset()
        assert ctx.tri_wear_sample(thr, 0.25) is True
        got = ctx.tri_wear_read()
        check(got, want["lanes"], want["rows"], want["abs_scale"], f"{bed['mode']}, thr {thr:g}")
        assert got["sampledTime"] == 0.25
        assert (got["slidingWork"] != 0).any() and (got["shearWork"] != 0).any() and (got["normalImpulse"] > 0).any()
        idle = got["rows"] == 0
        assert idle.any() and (~idle).any() and (lanes_of(got)[idle] == 0).all() and not np.signbit(lanes_of(got)[idle]).any()
    assert 10 <= int(want["rows"].sum()) < int(model_of(ctx, sc, 0.0, 0.25)["rows"].sum())


@pytest.mark.gpu
def test_samples_add_up_and_reset_clears(bed):
    """three samples of weights 0.5, 0.125 and 2.0 with 20 steps between them: the model's three results added in that order, within
    the bound of the summed scales; rows their exact integer sum; then the sub-range reads and the reset"""
    ctx, sc = bed["ctx"], bed["sc"]
    ctx.tri_wear_reset()
    lanes, scale, rows = np.zeros((800, 6)), np.zeros((800, 6)), np.zeros(800, np.uint64)
    for k, w in enumerate((0.5, 0.125, 2.0)):
        if k:
            ctx.step(20)
        want = model_of(ctx, sc, THR, w)
        assert ctx.tri_wear_sample(THR, w)
        lanes, scale, rows = lanes + want["lanes"], scale + want["abs_scale"], rows + want["rows"]
    got = ctx.tri_wear_read()
    check(got, lanes, rows, scale, f"{bed['mode']}, three samples")
    assert got["sampledTime"] == 2.625 and rows.sum() >= 10
    part = ctx.tri_wear_read(first=137, count=300)
    assert part["impulse"].shape == (300, 3) and part["rows"].shape == (300,) and part["rows"].any()
    for k in LANES + ("rows",):
        assert part[k].tobytes() == got[k][137:437].tobytes(), k
    last = ctx.tri_wear_read(first=799)
    assert all(last[k].tobytes() == got[k][799:].tobytes() and len(last[k]) == 1 for k in LANES + ("rows",))
    none = ctx.tri_wear_read(first=137, count=0)
    assert none["impulse"].shape == (0, 3) and none["rows"].shape == (0,) and none["sampledTime"] == 2.625
    ctx.tri_wear_reset()
    got = ctx.tri_wear_read()
    assert got["sampledTime"] == 0.0 and not got["rows"].any()
    assert all(got[k].tobytes() == bytes(got[k].nbytes) for k in LANES)  # exact zeros, +0.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_runs_that_span_workgroups_add_onto_the_sums(pkg, mode):
    """Two triangles under the whole bed, thr = 0: runs of about 1 100 rows, each summed by several workgroups, one closed by the
    final pass.  Sampled twice, so that the second sample adds onto non-zero sums through WearOut from both passes."""
    ctx, p, sc = stepped_mesh_bed(pkg, two_triangle_bed(pkg), mode)
    block = pkg.abi.tri_loads_block_rows()
    ctx.tri_wear_enable()
    scatter_motion(ctx, sc)
    want = model_of(ctx, sc, 0.0, 0.75)
    starts, ends, straddles = runs_of({"counts": want["rows"].astype(np.int64)}, block)
    print(f"{mode}: runs {want['rows'].tolist()}, blocks of {block}")
    assert sc.nTri == 2 and want["rows"].max() >= 3 * block and straddles
    assert ctx.tri_wear_sample(0.0, 0.75)
    first = ctx.tri_wear_read()
    check(first, want["lanes"], want["rows"], want["abs_scale"], f"{mode}, two triangles, one sample")
    assert (lanes_of(first) != 0).all()
    assert ctx.tri_wear_sample(0.0, 0.75)
    second = ctx.tri_wear_read()
    check(second, want["lanes"] + want["lanes"], want["rows"] * np.uint64(2), 2 * want["abs_scale"], f"{mode}, two triangles, two samples")
    assert lanes_of(second).tobytes() == (lanes_of(first) + lanes_of(first)).tobytes()  # acc + the same sample's sum, added once
    ctx.close()


@pytest.mark.gpu
def test_more_partials_than_one_round_of_the_last_pass_takes(pkg):
    """flat_bed(1, 40000) at thr 0: more than 128 workgroups with counted rows, so k_seg_final carries an open run from one round of
    256 partials into the next before WearOut adds it"""
    ctx, p, sc = stepped_mesh_bed(pkg, flat_bed(pkg, 1, 40000), "fast")
    block = pkg.abi.tri_loads_block_rows()
    ctx.tri_wear_enable()
    scatter_motion(ctx, sc)
    want = model_of(ctx, sc, 0.0, 0.5)
    counted = int(want["rows"].sum())
    print(f"two-triangle plate under 40 000 clumps: {counted} counted rows, runs {want['rows'].tolist()}")
    assert counted > 128 * block
    for k in (1, 2):
        assert ctx.tri_wear_sample(0.0, 0.5)
        check(ctx.tri_wear_read(), k * want["lanes"], want["rows"] * np.uint64(k), k * want["abs_scale"], f"flat bed, {k} sample(s)")
    ctx.close()


def _sequence(pkg, mode, wear):
    ctx, p, sc = stepped_mesh_bed(pkg, mesh_bed(pkg, 600, cd_freq=20), mode, steps=120)
    if wear:
        ctx.tri_wear_enable()
    return ctx, p, sc


@pytest.mark.gpu
def test_the_same_sequence_gives_the_same_bits(pkg):
    reads = []
    for _ in range(2):
        ctx, p, sc = _sequence(pkg, "fast", True)
        for w in (0.5, 0.25, 0.125, 1.0):
            ctx.step(7)
            assert ctx.tri_wear_sample(THR, w)
        reads.append(ctx.tri_wear_read())
        ctx.close()
    assert reads[0]["rows"].sum() > 0 and np.abs(reads[0]["impulse"]).max() > 0
    for k in LANES + ("rows",):
        assert reads[0][k].tobytes() == reads[1][k].tobytes(), k
    assert reads[0]["sampledTime"] == reads[1]["sampledTime"] == 1.875


def _assert_twins(ctx, ref, p, sc, what):
    a, r = ctx.download_state(), ref.download_state()
    for k in STATE_KEYS:
        assert np.array_equal(a[k], r[k]), (what, k)
    la, lr = _whole_list(ctx, sc), _whole_list(ref, sc)
    for k in la:
        assert np.array_equal(la[k].view(np.uint32) if la[k].dtype == np.float32 else la[k],
                              lr[k].view(np.uint32) if lr[k].dtype == np.float32 else lr[k]), (what, k)
    for w in range(int(p.nContactWildcards)):
        assert np.array_equal(ctx.wildcard(w).view(np.uint32), ref.wildcard(w).view(np.uint32)), (what, w)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_sampling_changes_nothing(pkg, mode):
    """40 rounds of (step 5, sample) beside a twin that never enabled wear: the state, the list, its records and its history are
    bit-equal at the end, and no detection was added (the fast mode keeps the engine's order, the exact mode the caller's)"""
    ctx, p, sc = _sequence(pkg, mode, True)
    ref, _, _ = _sequence(pkg, mode, False)
    assert ctx.engine_order()[0] == (mode == "fast")
    for _ in range(40):
        ctx.step(5), ref.step(5)
        assert ctx.tri_wear_sample(0.0, 5 * float(p.h))
    ctx.sync(), ref.sync()
    assert ctx.counts().nDetections == ref.counts().nDetections and ctx.counts().nSteps == ref.counts().nSteps == 320
    _assert_twins(ctx, ref, p, sc, mode)
    got = ctx.tri_wear_read()
    assert got["rows"].sum() > 100 and abs(got["sampledTime"] - 200 * float(p.h)) <= 1e-12 * got["sampledTime"]
    assert got["impulse"][:, 2].sum() < 0  # the plate carries the bed: the impulse on it points down
    ctx.close(), ref.close()


@pytest.mark.gpu
def test_sampling_beside_an_asynchronous_detection(pkg):
    """the same trajectory as the twin with deme_set_async_detection on: a sample reads the list in force, never the one being built"""
    ctxs = []
    for wear in (True, False):
        b = mesh_bed(pkg, 600, cd_freq=20)
        b.SetExpandSafetyAdder(1.0)
        p, sc = b.Initialize()
        c = pkg.Context(0)
        c.set_arith_mode("fast")
        c.set_params(p), c.upload_scene(sc)
        c.set_record_contacts(True)
        c.step(120)
        c.set_async_detection(6)
        c.set_timing(1)
        if wear:
            c.tri_wear_enable()
        ctxs.append(c)
    ctx, ref = ctxs
    flags = []
    for _ in range(12):
        ctx.step(25), ref.step(25)
        flags.append(ctx.tri_wear_sample(0.0, 1.0))
    ctx.step(1), ref.step(1)  # (a cycle that ends with a call leaves records of the list before: one more step evaluates the new one)
    ctx.sync(), ref.sync()
    print(f"sampled: {flags}")
    assert ctx.kernel_time_ms("detect_async_part1")[1] >= 8  # (the asynchronous path really served)
    assert ctx.counts().nDetections == ref.counts().nDetections
    _assert_twins(ctx, ref, p, sc, "async detection")
    got = ctx.tri_wear_read()
    assert sum(flags) >= 6 and got["sampledTime"] == float(sum(flags)) and got["rows"].sum() > 100
    # the list in force has been evaluated now: a sample of it is the model's
    ctx.tri_wear_reset()
    assert ctx.tri_wear_sample(0.0, 0.5) is True
    want = model_of(ctx, sc, 0.0, 0.5)
    check(ctx.tri_wear_read(), want["lanes"], want["rows"], want["abs_scale"], "beside an asynchronous detection")
    ctx.close(), ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_a_list_that_was_not_evaluated_is_not_sampled(pkg, mode):
    """deme_detect_contacts puts a new list in force while the records in memory are those of the list before -- what the end of an
    asynchronous detection cycle leaves too: sampled == 0, nothing added; one step later the sample is the model's"""
    ctx, p, sc = _sequence(pkg, mode, True)
    assert ctx.tri_wear_sample(0.0, 0.5)
    before = ctx.tri_wear_read()
    ctx.detect()
    assert ctx.tri_wear_sample(0.0, 3.0) is False
    after = ctx.tri_wear_read()
    assert after["sampledTime"] == 0.5 and all(after[k].tobytes() == before[k].tobytes() for k in LANES + ("rows",))
    ctx.step(1)
    ctx.tri_wear_reset()
    assert ctx.tri_wear_sample(0.0, 3.0) is True
    want = model_of(ctx, sc, 0.0, 3.0)
    check(ctx.tri_wear_read(), want["lanes"], want["rows"], want["abs_scale"], f"{mode}, the step after a detection")
    assert want["rows"].sum() > 20
    ctx.close()


@pytest.mark.gpu
def test_bytes_that_come_to_the_host(bed):
    ctx, lib = bed["ctx"], bed["ctx"].lib
    before = ctx.query_host_bytes()
    ctx.tri_wear_enable()
    ctx.tri_wear_reset()
    assert ctx.tri_wear_sample(THR, 0.5) and ctx.tri_wear_sample(0.0, 0.0)
    assert ctx.query_host_bytes() == before
    ctx.tri_wear_read()
    assert ctx.query_host_bytes() - before == 56 * 800
    ctx.tri_wear_read(first=137, count=300)
    assert ctx.query_host_bytes() - before == 56 * 800 + 56 * 300
    before = ctx.query_host_bytes()
    work = ctx.tri_wear_read(first=137, count=300, columns=("slidingWork",))
    assert ctx.query_host_bytes() - before == 8 * 300 and set(work) == {"slidingWork", "sampledTime"}
    ctx.tri_wear_read(first=0, count=10, columns=("impulse", "rows"))
    assert ctx.query_host_bytes() - before == 8 * 300 + 32 * 10
    t = C.c_double(-1.0)
    assert lib.deme_tri_wear_read(ctx.h, 137, 0, None, None, None, None, None, C.byref(t)) == 0 and t.value == 0.5
    ctx.tri_wear_reset()
    assert ctx.query_host_bytes() - before == 8 * 300 + 32 * 10


def _seed_again(ctx, p):
    a, b, t, _ = ctx.contacts()
    W = np.stack([ctx.wildcard(w) for w in range(int(p.nContactWildcards))], 1) if p.nContactWildcards else None
    ctx.seed_contacts(a, b, t, W)


@pytest.mark.gpu
def test_a_seeded_list_is_not_sampled(pkg):
    ctx, p, sc = _sequence(pkg, "fast", True)
    assert ctx.tri_wear_sample(0.0, 0.5)
    before = ctx.tri_wear_read()
    _seed_again(ctx, p)
    with pytest.raises(pkg.abi.DemeError):
        ctx.contact_records()
    assert ctx.tri_wear_sample(0.0, 3.0) is False
    assert ctx.lib.deme_tri_wear_sample(ctx.h, 0.0, 3.0, None) == 0
    after = ctx.tri_wear_read()
    assert after["sampledTime"] == 0.5 and before["rows"].sum() > 0
    assert all(after[k].tobytes() == before[k].tobytes() for k in LANES + ("rows",))
    ctx.step(1)
    assert ctx.tri_wear_sample(0.0, 3.0) is True
    after = ctx.tri_wear_read()
    assert after["sampledTime"] == 3.5 and after["rows"].sum() > before["rows"].sum()
    ctx.close()


@pytest.mark.gpu
def test_a_scene_upload_keeps_or_clears_the_sums(pkg):
    ctx, p, sc = _sequence(pkg, "fast", True)
    assert ctx.tri_wear_sample(0.0, 0.5)
    before = ctx.tri_wear_read()
    assert before["rows"].sum() > 0
    ctx.tri_wear_enable()  # twice: the sums stay
    ctx.upload_scene(sc)   # the same mesh: the sums stay
    same = ctx.tri_wear_read()
    assert same["sampledTime"] == 0.5 and all(same[k].tobytes() == before[k].tobytes() for k in LANES + ("rows",))
    p2, sc2 = two_triangle_bed(pkg, 300).Initialize()
    ctx.set_params(p2), ctx.upload_scene(sc2)
    fresh = ctx.tri_wear_read()
    assert fresh["rows"].shape == (2,) and fresh["sampledTime"] == 0.0 and not fresh["rows"].any()
    assert all(fresh[k].tobytes() == bytes(fresh[k].nbytes) for k in LANES)
    ctx.set_record_contacts(True)
    ctx.step(60)
    assert ctx.tri_wear_sample(0.0, 1.0) and ctx.tri_wear_read()["sampledTime"] == 1.0
    ctx.tri_wear_enable(False)  # freed: the calls refuse, and enabling again starts from zeros
    with pytest.raises(pkg.abi.DemeError, match="not enabled"):
        ctx.tri_wear_read()
    ctx.tri_wear_enable()
    assert not ctx.tri_wear_read()["rows"].any() and ctx.tri_wear_read()["sampledTime"] == 0.0
    ctx.close()


@pytest.mark.gpu
def test_refusals(pkg, bed):
    ctx, lib, mode = bed["ctx"], bed["ctx"].lib, bed["mode"]
    ctx.tri_wear_reset()
    assert ctx.tri_wear_sample(THR, 0.5)
    kept = ctx.tri_wear_read()

    def unchanged(c, ref):
        now = c.tri_wear_read()
        return now["sampledTime"] == ref["sampledTime"] and all(now[k].tobytes() == ref[k].tobytes() for k in LANES + ("rows",))

    def sample(c, thr, w):
        flag = C.c_int(77)
        rc = lib.deme_tri_wear_sample(c.h, thr, w, C.byref(flag))
        return rc, flag.value, lib.deme_last_error(c.h).decode()

    # in the order listed: not enabled comes before the threshold, the threshold before the weight, the weight before recording
    off, p, sc2 = stepped_mesh_bed(pkg, mesh_bed(pkg, 600), mode, steps=120)
    off.set_record_contacts(False)
    for call in ("sample", "read", "reset"):
        rc = {"sample": lambda: lib.deme_tri_wear_sample(off.h, -1.0, -1.0, None),
              "read": lambda: lib.deme_tri_wear_read(off.h, 0, 900, None, None, None, None, None, None),
              "reset": lambda: lib.deme_tri_wear_reset(off.h)}[call]()
        msg = lib.deme_last_error(off.h).decode()
        assert rc == 1 and "not enabled" in msg and f"deme_tri_wear_{call}" in msg, (call, msg)
    off.tri_wear_enable()
    for what, thr, w in (("threshold", -1.0, -1.0), ("threshold", float("nan"), 0.5), ("threshold", float("inf"), float("nan")),
                         ("weight", THR, -0.5), ("weight", THR, float("nan")), ("weight", THR, float("inf")), ("recording is off", THR, 0.5)):
        rc, flag, msg = sample(off, thr, w)
        assert rc == 1 and flag == 77 and what in msg and "deme_tri_wear_sample" in msg, (what, thr, w, msg)
        assert ("threshold" in msg) == (what == "threshold") and ("weight" in msg) == (what == "weight"), msg
    zero = off.tri_wear_read()
    assert zero["sampledTime"] == 0.0 and not zero["rows"].any()
    off.set_record_contacts(True)
    off.step(1)
    # a weight of 0 counts rows and adds zeros
    assert off.tri_wear_sample(0.0, 0.0) is True
    got = off.tri_wear_read()
    assert got["rows"].sum() > 0 and got["sampledTime"] == 0.0 and not lanes_of(got).any()
    off.close()
    # the bed: every refusal leaves its sums as they were, and the caller's arrays untouched
    for thr, w in ((-1.0, 0.5), (THR, -0.5)):
        assert sample(ctx, thr, w)[0] == 1
    for what, first, count, null in (("range past the last triangle", 1, 800, False), ("range that begins past the last triangle", 801, 0, False),
                                     ("range that wraps", 0xFFFFFFFF, 2, False), ("every output null", 0, 800, True)):
        buf = np.full((max(count, 1) + 2, 3), 7.5)
        rc = lib.deme_tri_wear_read(ctx.h, first, count, None if null else buf.ctypes.data, None, None, None, None, None)
        msg = lib.deme_last_error(ctx.h).decode()
        assert rc == 1 and (buf == 7.5).all() and "deme_tri_wear_read" in msg, (what, msg)
        assert ("triangles" in msg) == ("range" in what) and ("null" in msg) == ("null" in what), (what, msg)
    assert lib.deme_tri_wear_read(ctx.h, 800, 0, None, None, None, None, None, None) == 0
    assert unchanged(ctx, kept)
    with pytest.raises(pkg.abi.DemeError, match="threshold"):
        ctx.tri_wear_sample(-1.0, 0.5)
    # a context without triangles: every call does nothing, a triangle asked for is refused
    p, sc, _ = _bed_scene(pkg)
    plain = _stepped(pkg, p, sc, mode)
    assert sc.nTri == 0
    plain.tri_wear_enable()
    assert plain.tri_wear_sample(THR, 0.5) is True
    got = plain.tri_wear_read()
    assert got["rows"].shape == (0,) and got["impulse"].shape == (0, 3) and got["sampledTime"] == 0.5
    buf = np.full(3, 7.5)
    assert lib.deme_tri_wear_read(plain.h, 0, 1, buf.ctypes.data, None, None, None, None, None) == 1 and (buf == 7.5).all()
    assert "deme_tri_wear_read" in lib.deme_last_error(plain.h).decode()
    plain.tri_wear_reset()
    plain.close()
    # no scene uploaded
    bare = pkg.Context(0)
    assert lib.deme_tri_wear_enable(bare.h, 1) == 1
    bare.close()
