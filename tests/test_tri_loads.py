"""deme_inspect_tri_loads (Context.inspect_tri_loads): the contact force and the contact count of every mesh triangle, summed over
the current list on the device, against tests/_tri_loads64.py applied to the whole-list downloads.

The bed is that of tests/test_mesh.py: 1500 three-sphere clumps falling onto a wavy 20 x 20 plate (800 triangles), stepped 3 x 60
times as test_mesh_contacts_and_forces_match_oracle steps it, with recording on.

Tolerance of a triangle's force: |force - model| <= 1e-10 * abs_sum per component, abs_sum = sum |f_j| over the triangle's counted
rows.  It is derived, not measured: both sides add the same fp32 terms in fp64, in different orders; a sum of n terms differs by at
most n * 1.1e-16 of abs_sum, and n < 1e4 here.  The counts are compared for equality."""
import ctypes as C

import numpy as np
import pytest

from tests._tri_loads64 import tri_loads
from tests.test_mesh import mesh_bed
from tests.test_owner_contacts import _bed_scene, _owner_tables, _stepped, _whole_list

THR = 1e-12  # what the shell passes (DEME_TINY_FLOAT_HOST)
REL = 1e-10
SYMBOLS = ("deme_inspect_tri_loads", "deme_multi_inspect_tri_loads", "deme_tri_loads_block_rows")
STATE_KEYS = ("voxelID", "locX", "locY", "locZ", "oriQw", "oriQx", "oriQy", "oriQz", "vX", "vY", "vZ", "omgBarX", "omgBarY", "omgBarZ")


def test_tri_loads_are_exported_and_bound(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in SYMBOLS:
        assert n in names and hasattr(lib, n), n
    for cls in (pkg.Context, pkg.abi.Multi):
        assert hasattr(cls, "inspect_tri_loads"), cls.__name__
    assert lib.deme_inspect_tri_loads.argtypes is not None and len(lib.deme_inspect_tri_loads.argtypes) == 6
    assert len(lib.deme_multi_inspect_tri_loads.argtypes) == 6
    assert pkg.abi.tri_loads_block_rows() >= 64


def test_the_model_on_a_hand_written_list():
    """five rows: sphere-sphere, sphere-plane, two on triangle 1, one on triangle 2 below the threshold; a sixth of a ghost's sphere"""
    idA = [0, 1, 2, 3, 4, 5]
    idB = [1, 0, 1, 1, 2, 0]
    ctype = [1, 3, 2, 2, 2, 2]
    force = np.array([[9, 9, 9], [8, 8, 8], [1, 2, 3], [0.5, -1, 0.25], [1e-3, 0, 0], [7, 7, 7]], np.float32)
    sphere_owner = [0, 0, 1, 2, 2, 3]
    ghost = [False, False, False, True]
    m = tri_loads(idA, idB, ctype, force, sphere_owner, ghost, 3, 0.01)
    assert m["counted"].tolist() == [False, False, True, True, False, False]
    assert m["counts"].tolist() == [0, 2, 0] and m["counts"].dtype == np.uint32
    assert np.array_equal(m["force"], [[0, 0, 0], [-1.5, -1, -3.25], [0, 0, 0]])
    assert np.array_equal(m["abs_sum"][1], [1.5, 3, 3.25])
    m0 = tri_loads(idA[:5], idB[:5], ctype[:5], force[:5], sphere_owner, None, 3, 0.0)
    assert m0["counts"].tolist() == [0, 2, 1] and m0["force"][2, 0] == -float(np.float32(1e-3))
    z = np.zeros((5, 3), np.float32)
    assert tri_loads(idA[:5], idB[:5], ctype[:5], z, sphere_owner, None, 3, 0.0)["counts"].tolist() == [0, 2, 1]  # zero force counts at 0
    assert tri_loads(idA[:5], idB[:5], ctype[:5], force[:5], sphere_owner, None, 2, 0.0)["counts"].tolist() == [0, 2]  # B >= n_tri: not counted


def model_of(ctx, sc, thr):
    whole = _whole_list(ctx, sc)
    return whole, tri_loads(whole["idA"], whole["idB"], whole["type"], whole["force"], _owner_tables(sc)[0], None, int(sc.nTri), thr)


def check(force, counts, want, what):
    err = np.abs(force - want["force"])
    bound = REL * want["abs_sum"]
    print(f"{what}: counted rows {int(counts.sum())}, loaded triangles {int((counts > 0).sum())}, max |force - model| {err.max():.3e}, "
          f"max abs_sum {want['abs_sum'].max():.3e}, worst ratio {(err / np.maximum(want['abs_sum'], 1e-300)).max():.3e}")
    assert counts.dtype == np.uint32 and np.array_equal(counts, want["counts"]), what
    assert force.dtype == np.float64 and force.shape == want["force"].shape and (err <= bound).all(), (what, err.max())


def stepped_mesh_bed(pkg, builder, mode, steps=180, reorder=None):
    p, sc = builder.Initialize()
    c = pkg.Context(0)
    c.set_arith_mode(mode)
    if reorder is not None:
        c.set_reorder(reorder)
    c.set_params(p)
    c.upload_scene(sc)
    c.set_record_contacts(True)
    for _ in range(steps // 60):
        c.step(60)
    if steps % 60:
        c.step(steps % 60)
    c.sync()
    return c, p, sc


@pytest.fixture(scope="module", params=["fast", "exact"])
def bed(pkg, request):
    ctx, p, sc = stepped_mesh_bed(pkg, mesh_bed(pkg, 1500), request.param)
    whole, want = model_of(ctx, sc, THR)
    _, want0 = model_of(ctx, sc, 0.0)
    yield {"ctx": ctx, "p": p, "sc": sc, "mode": request.param, "whole": whole, "want": want, "want0": want0}
    ctx.close()


@pytest.mark.gpu
def test_bed_list_exercises_what_it_should(bed):
    """After 180 steps the bed is still bouncing on the plate: the list holds some 640 sphere-mesh rows (every triangle a sphere's
    box reaches), of which 17 carry a force at that instant.  So the list is asked twice: with a threshold
    of 0, where every listed sphere-mesh row counts -- the 50 rows, the triangles with several and with none are asserted there
    -- and with the shell's threshold, where only the rows with a force do."""
    whole, want, want0, sc = bed["whole"], bed["want"], bed["want0"], bed["sc"]
    assert sc.nTri == 800
    assert int(want0["counted"].sum()) >= 50 and int(want0["counted"].sum()) == int((whole["type"] == 2).sum())
    assert (want0["counts"] >= 2).any() and (want0["counts"] == 0).any()
    assert (whole["type"] == 1).any()
    assert 10 <= int(want["counted"].sum()) < int(want0["counted"].sum()) and (want["counts"] == 0).any()
    assert bed["ctx"].engine_order()[0] == (bed["mode"] == "fast")
    f = np.sqrt((whole["force"][whole["type"] == 2].astype(np.float64) ** 2).sum(1))
    assert not ((f > THR / 2) & (f < 2 * THR)).any()  # no row a rounding could move across the shell's threshold


@pytest.mark.gpu
def test_forces_and_counts_equal_the_model(bed):
    for thr, want in ((0.0, bed["want0"]), (THR, bed["want"])):
        force, counts = bed["ctx"].inspect_tri_loads(thr)
        check(force, counts, want, f"{bed['mode']}, whole mesh, threshold {thr:g}")
        assert np.abs(force).max() > 0 and (force[counts == 0] == 0).all()
        # the plate carries the bed: the load on it points down
        assert force[:, 2].sum() < 0


@pytest.mark.gpu
def test_a_threshold_above_the_median_force(bed):
    """The decision is exact on both sides (the squares of fp32 values are exact in fp64 and the three are added in the same
    order); the threshold is put between two neighbours of the sorted |f| all the same, and no row lies within rounding of it."""
    ctx, whole = bed["ctx"], bed["whole"]
    sm = whole["type"] == 2
    f = np.sort(np.sqrt((whole["force"][sm].astype(np.float64) ** 2).sum(1)))
    f = f[f > 0]
    k = int(0.6 * len(f))
    thr = float(np.float32(0.5 * (f[k] + f[k + 1])))
    assert thr > np.median(f) and f[k] < thr < f[k + 1]
    assert not (np.abs(f - thr) <= 1e-6 * thr).any()  # (an fp32 rounding is 6e-8 of the value)
    _, want = model_of(ctx, bed["sc"], thr)
    force, counts = ctx.inspect_tri_loads(thr)
    check(force, counts, want, f"{bed['mode']}, threshold {thr:.3e}")
    assert 0 < counts.sum() < bed["want"]["counts"].sum()


@pytest.mark.gpu
def test_a_sub_range_is_the_slice_of_the_whole_answer(pkg, bed):
    ctx, lib = bed["ctx"], bed["ctx"].lib
    force, counts = ctx.inspect_tri_loads(THR)
    f, n = ctx.inspect_tri_loads(THR, first=137, count=300)
    assert f.shape == (300, 3) and n.shape == (300,)
    assert f.tobytes() == force[137:437].tobytes() and np.array_equal(n, counts[137:437]) and n.any()
    f, n = ctx.inspect_tri_loads(THR, first=799)  # to the last one
    assert f.tobytes() == force[799:].tobytes() and np.array_equal(n, counts[799:])
    assert lib.deme_inspect_tri_loads(ctx.h, THR, 137, 0, None, None) == 0
    assert lib.deme_inspect_tri_loads(ctx.h, THR, 800, 0, None, None) == 0
    f, n = ctx.inspect_tri_loads(THR, first=137, count=0)
    assert f.shape == (0, 3) and n.shape == (0,)
    # a context without triangles answers nTris = 0, and nothing else
    p, sc, _ = _bed_scene(pkg)
    plain = _stepped(pkg, p, sc, bed["mode"])
    assert sc.nTri == 0
    f, n = plain.inspect_tri_loads(THR)
    assert f.shape == (0, 3) and n.shape == (0,)
    buf = np.full(3, 7.5)
    assert lib.deme_inspect_tri_loads(plain.h, THR, 0, 1, buf.ctypes.data, None) == 1 and (buf == 7.5).all()
    assert "deme_inspect_tri_loads" in lib.deme_last_error(plain.h).decode()
    plain.close()


def two_triangle_bed(pkg, n=1500):
    """the bed of mesh_bed laid out flat (a third of its height, so three times the footprint) over a plate of two triangles"""
    b = pkg.model.packed_bed(n, seed=3, cd_freq=0, spacing_mult=2.8, init_vz=-1.0, aspect=(1.0, 1.0, 0.15))
    lo, hi = b.user_box_min, b.user_box_max
    v, f = pkg.model.plate_mesh(1, 1, float(hi[0] - lo[0]) * 0.9, float(hi[1] - lo[1]) * 0.9, z=0.0, wavy=0.0)
    m = b.AddMeshObject(v, f, 0)
    m.SetInitPos(((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, 0.0195))
    m.SetMass(0.5)
    m.SetMOI((1e-3, 1e-3, 2e-3))
    return b


def runs_of(want, block):
    """(start, end) of every triangle's run in the sorted counted rows, and whether some run starts inside one workgroup's
    entries and ends in another's"""
    lengths = want["counts"].astype(np.int64)
    ends = np.cumsum(lengths)
    starts = ends - lengths
    live = lengths > 0
    straddles = live & (starts % block != 0) & (starts // block != (ends - 1) // block)
    return starts, ends, bool(straddles.any())


def test_the_two_triangle_bed_has_runs_that_span_workgroups(pkg, orc):
    """The oracle's list of the scene the GPU test below steps: 1500 clumps, 2238 rows, 2201 of them sphere-mesh, 1099 on triangle 0
    and 1102 on triangle 1 -- each more than 3 x 256, and triangle 1's run begins at entry 1099 = 4 * 256 + 75."""
    p, sc = two_triangle_bed(pkg).Initialize()
    sim = orc.make_sim(pkg, p, sc)
    sim.step(180)
    a, b, t, _ = sim.contacts()
    sm = t == 2
    lengths = np.bincount(b[sm], minlength=2)
    print(f"two-triangle bed: {len(a)} rows, {int(sm.sum())} sphere-mesh, runs {lengths.tolist()}")
    block = 256  # (deme_tri_loads_block_rows() of the library as built; the GPU test asks the library)
    assert sc.nTri == 2 and lengths.max() >= 3 * block
    assert runs_of({"counts": lengths}, block)[2]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_runs_that_span_workgroups(pkg, mode):
    """Two triangles under the whole bed, thr = 0: every listed sphere-mesh row counts.  n = 1500 clumps is enough (the CPU test
    above: runs of 1099 and 1102 rows, blocks of 256)."""
    ctx, p, sc = stepped_mesh_bed(pkg, two_triangle_bed(pkg), mode)
    block = pkg.abi.tri_loads_block_rows()
    whole, want = model_of(ctx, sc, 0.0)
    sm = whole["type"] == 2
    assert sc.nTri == 2 and int(want["counted"].sum()) == int(sm.sum())
    starts, ends, straddles = runs_of(want, block)
    print(f"{mode}: runs {want['counts'].tolist()}, blocks of {block}")
    assert want["counts"].max() >= 3 * block and straddles
    force, counts = ctx.inspect_tri_loads(0.0)
    check(force, counts, want, f"{mode}, two triangles")
    again, _ = ctx.inspect_tri_loads(0.0)
    assert again.tobytes() == force.tobytes()
    ctx.close()


def flat_bed(pkg, cells, n):
    """n clumps of mesh_bed's recipe laid out a few layers high (aspect 1 : 1 : 0.03) over a plate of cells x cells x 2 triangles.
    With the oracle's list after 180 steps: 40 000 clumps on the two-triangle plate give 47 660 sphere-mesh rows of 48 652 (runs of
    23 846 and 23 814); 80 000 clumps on the 20 x 20 plate 54 550 of 57 680, the longest run 91 rows, one run across row 32 768
    (40 000 clumps give 25 983 there: too few)"""
    b = pkg.model.packed_bed(n, seed=3, cd_freq=0, spacing_mult=2.8, init_vz=-1.0, aspect=(1.0, 1.0, 0.03))
    lo, hi = b.user_box_min, b.user_box_max
    v, f = pkg.model.plate_mesh(cells, cells, float(hi[0] - lo[0]) * 0.9, float(hi[1] - lo[1]) * 0.9, z=0.0, wavy=0.0 if cells == 1 else 0.003)
    m = b.AddMeshObject(v, f, 0)
    m.SetInitPos(((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, 0.0195))
    m.SetMass(0.5)
    m.SetMOI((1e-3, 1e-3, 2e-3))
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("cells,n", [(1, 40000), (20, 80000)])
def test_more_partials_than_one_round_of_the_last_pass_takes(pkg, cells, n):
    """k_seg_final (deme_seg_sum.h) takes the blocks' partials 256 at a round and carries the open run from one round to the next: that needs
    more than 128 blocks with counted rows, more than 32 768 counted rows.  A bed a few layers high, asked with thr = 0:
    on the two-triangle plate both runs span dozens of blocks and the second one crosses from the first round into the second; on
    the 20 x 20 plate the rounds meet in the middle of the list, among runs of a few dozen rows.  The same list at the shell's
    threshold has more than 50 rows that carry a force and triangles that sum several of them."""
    ctx, p, sc = stepped_mesh_bed(pkg, flat_bed(pkg, cells, n), "fast")
    block = pkg.abi.tri_loads_block_rows()
    per_round = 128 * block  # sorted rows behind one round of 256 partials (two a block)
    whole, want0 = model_of(ctx, sc, 0.0)
    starts, ends, straddles = runs_of(want0, block)
    counted = int(want0["counts"].sum())
    live = want0["counts"] > 0
    crosses = live & (starts // per_round != (ends - 1) // per_round)
    print(f"{cells} x {cells} plate: {len(whole['idA'])} rows, {counted} counted at thr 0, longest run {int(want0['counts'].max())}, "
          f"{-(-counted // block)} blocks with counted rows, runs that cross a round: {int(crosses.sum())}")
    assert counted > per_round and straddles and crosses.any()
    force, counts = ctx.inspect_tri_loads(0.0)
    check(force, counts, want0, f"{cells} x {cells} plate, thr 0")
    _, want = model_of(ctx, sc, THR)
    nonzero = int(want["counts"].sum())
    print(f"rows that carry a force: {nonzero}, triangles that sum two or more: {int((want['counts'] >= 2).sum())}")
    assert nonzero >= 50 and (want["counts"] >= 2).any()
    force, counts = ctx.inspect_tri_loads(THR)
    check(force, counts, want, f"{cells} x {cells} plate, thr {THR:g}")
    assert np.abs(force).max() > 0
    ctx.close()


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(bed):
    a, na = bed["ctx"].inspect_tri_loads(THR)
    b, nb = bed["ctx"].inspect_tri_loads(THR)
    assert a.tobytes() == b.tobytes() and a.any() and np.array_equal(na, nb)


@pytest.mark.gpu
def test_engine_order_on_and_off_agree(pkg):
    """The bed's state, list and history handed to two fresh contexts, one keeping an order of its own and one the caller's; one
    step each.  (The fast mode: the exact mode keeps the caller's order whatever deme_set_reorder says.)  Both evaluate the same
    contacts of the same state; the triangles' sums are taken in different orders."""
    src, p, sc = stepped_mesh_bed(pkg, mesh_bed(pkg, 1500), "fast")
    st = src.download_state()
    la, lb, lt, _ = src.contacts()
    W = np.stack([src.wildcard(w) for w in range(int(p.nContactWildcards))], 1) if p.nContactWildcards else None
    got = {}
    for reorder in (True, False):
        c = pkg.Context(0)
        c.set_arith_mode("fast")
        c.set_reorder(reorder)
        c.set_params(p), c.upload_scene(sc)
        c.set_record_contacts(True)
        assert c.engine_order()[0] == reorder
        c.upload_state({k: st[k] for k in STATE_KEYS})
        c.seed_contacts(la, lb, lt, W)
        c.step(1)
        c.sync()
        whole, want = model_of(c, sc, THR)
        force, counts = c.inspect_tri_loads(THR)
        check(force, counts, want, f"engine order {'on' if reorder else 'off'}")
        got[reorder] = (force, counts, want, whole)
        c.close()
    src.close()
    rows_differ = np.abs(got[True][3]["force"].astype(np.float64) - got[False][3]["force"]).max() if len(got[True][3]["force"]) == len(got[False][3]["force"]) else np.nan
    print(f"largest difference of a recorded force between the two contexts: {rows_differ:.3e}")
    assert np.array_equal(got[True][1], got[False][1]) and got[True][1].sum() >= 10
    assert (np.abs(got[True][0] - got[False][0]) <= REL * got[True][2]["abs_sum"]).all()


@pytest.mark.gpu
def test_bytes_that_come_to_the_host(bed):
    ctx, lib = bed["ctx"], bed["ctx"].lib
    before = ctx.query_host_bytes()
    ctx.inspect_tri_loads(THR)
    assert ctx.query_host_bytes() - before == 28 * 800
    ctx.inspect_tri_loads(THR, first=137, count=300)
    assert ctx.query_host_bytes() - before == 28 * 800 + 28 * 300
    before = ctx.query_host_bytes()
    f, n = np.zeros((300, 3)), np.zeros(300, np.uint32)
    assert lib.deme_inspect_tri_loads(ctx.h, THR, 137, 300, f.ctypes.data, None) == 0
    assert ctx.query_host_bytes() - before == 24 * 300
    assert lib.deme_inspect_tri_loads(ctx.h, THR, 137, 300, None, n.ctypes.data) == 0
    assert ctx.query_host_bytes() - before == 24 * 300 + 4 * 300
    assert f.any() and n.any()
    assert lib.deme_inspect_tri_loads(ctx.h, THR, 137, 0, None, None) == 0
    assert ctx.query_host_bytes() - before == 28 * 300


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_the_call_changes_nothing(pkg, mode):
    """step, ask, step -- the state and the list afterwards are those of a twin context that never asked, and the question has
    launched no detection"""
    b = mesh_bed(pkg, 600, cd_freq=20)
    ctx, p, sc = stepped_mesh_bed(pkg, b, mode, steps=150)
    ref, _, _ = stepped_mesh_bed(pkg, mesh_bed(pkg, 600, cd_freq=20), mode, steps=151)
    detections = ctx.counts().nDetections
    ctx.inspect_tri_loads(THR)
    force, counts = ctx.inspect_tri_loads(0.0)
    ctx.inspect_tri_loads(0.0, first=3, count=17)
    assert counts.sum() > 20
    ctx.step(1)
    ctx.sync()
    assert ctx.counts().nDetections == ref.counts().nDetections and ctx.counts().nDetections - detections <= 1 and ctx.counts().nSteps == 151
    a, r = ctx.download_state(), ref.download_state()
    assert all(np.array_equal(a[k], r[k]) for k in a)
    ctx.inspect_tri_loads(THR)
    la, lr = _whole_list(ctx, sc), _whole_list(ref, sc)
    for k in la:
        assert np.array_equal(la[k].view(np.uint32) if la[k].dtype == np.float32 else la[k],
                              lr[k].view(np.uint32) if lr[k].dtype == np.float32 else lr[k]), k
    for w in range(int(p.nContactWildcards)):
        assert np.array_equal(ctx.wildcard(w).view(np.uint32), ref.wildcard(w).view(np.uint32)), w
    ctx.step(1), ref.step(1)
    ctx.sync(), ref.sync()
    a, r = ctx.download_state(), ref.download_state()
    assert all(np.array_equal(a[k], r[k]) for k in a)
    ctx.close(), ref.close()


@pytest.mark.gpu
def test_refusals(pkg, bed):
    ctx, sc, lib = bed["ctx"], bed["sc"], bed["ctx"].lib

    def ask(c, thr, first, count, null=(False, False)):
        f = np.full((max(count, 1) + 2, 3), 7.5)
        n = np.full(max(count, 1) + 2, 0xABABABAB, np.uint32)
        rc = lib.deme_inspect_tri_loads(c.h, thr, first, count, None if null[0] else f.ctypes.data, None if null[1] else n.ctypes.data)
        return rc, bool((f == 7.5).all() and (n == 0xABABABAB).all()), lib.deme_last_error(c.h).decode()

    for what, thr, first, count, null in (("negative threshold", -1.0, 0, 800, (False, False)), ("NaN threshold", float("nan"), 0, 800, (False, False)),
                                          ("infinite threshold", float("inf"), 0, 800, (False, False)),
                                          ("range past the last triangle", THR, 1, 800, (False, False)),
                                          ("range that begins past the last triangle", THR, 801, 0, (False, False)),
                                          ("range that wraps", THR, 0xFFFFFFFF, 2, (False, False)),
                                          ("both outputs null", THR, 0, 800, (True, True))):
        rc, untouched, msg = ask(ctx, thr, first, count, null)
        assert rc == 1 and untouched and "deme_inspect_tri_loads" in msg, (what, rc, msg)
        assert ("threshold" in msg) == ("threshold" in what) and ("triangles" in msg) == ("range" in what) and ("null" in msg) == ("null" in what), (what, msg)
    rc, untouched, _ = ask(ctx, THR, 0, 800)
    assert rc == 0 and not untouched
    with pytest.raises(pkg.abi.DemeError, match="threshold"):
        ctx.inspect_tri_loads(-1.0)
    # recording off, and a seeded list: the refusals of deme_download_contact_records
    off, p, sc2 = stepped_mesh_bed(pkg, mesh_bed(pkg, 600), bed["mode"], steps=150)
    off.set_record_contacts(False)
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    assert "recording is off" in lib.deme_last_error(off.h).decode()
    rc, untouched, msg = ask(off, THR, 0, 800)
    assert rc == 1 and untouched and "recording is off" in msg and "deme_inspect_tri_loads" in msg
    off.set_record_contacts(True)
    a, b, t, _ = off.contacts()
    W = np.stack([off.wildcard(w) for w in range(int(p.nContactWildcards))], 1) if p.nContactWildcards else None
    off.seed_contacts(a, b, t, W)
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    assert "seed" in lib.deme_last_error(off.h).decode()
    rc, untouched, msg = ask(off, THR, 0, 800)
    assert rc == 1 and untouched and "seed" in msg and "deme_inspect_tri_loads" in msg
    off.step(1)
    off.sync()
    assert off.inspect_tri_loads(0.0)[1].sum() > 0  # evaluated again: it answers
    off.close()
