"""deme_scatter_owner_state / deme_multi_scatter_owner_state: position code, orientation, velocity, angular velocity and family of
a few owners, written on the device.  Every case is held against a twin context: the same scene and steps, where the same change
is made by download_state -> edit rows -> upload_state of the same columns only.  The values are copied, never computed, so every
comparison is np.array_equal on bit patterns."""
import numpy as np
import pytest

from tests.test_owner_contacts import _bed_scene, _stepped
from tests.test_owner_contacts_multi import HALO, STEPS, bed_scene, built

pytestmark = pytest.mark.gpu
PER_ID = 4 + 64  # bytes a scattered owner takes to the device: its slot (or global id) and its record
POS = ("voxelID", "locX", "locY", "locZ")
VEL = ("vX", "vY", "vZ")
ORI_ANGVEL = ("oriQw", "oriQx", "oriQy", "oriQz", "omgBarX", "omgBarY", "omgBarZ")
FAM = ("familyID",)
TILT = np.float32(0.01)  # half the angle of the orientation written: a small tilt about y (a large one would push packed clumps into each other)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same(a, b, what, cols=None):
    for k in (cols or sorted(a)):
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _new_rows(whole, ids, cols, l_units=3, families=None):
    """row i: what owner ids[i] is to hold in the columns `cols`, derived from the state `whole` so that every value differs from
    what is there: the position nudged by l_units sub-voxel units, the velocity halved and shifted, a fixed quaternion, an
    angular velocity that depends on the row, family 1 (or `families`)"""
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    rows = {}
    for k in cols:
        cur = whole[k][ids]
        if k == "voxelID":
            rows[k] = cur.copy()
        elif k in ("locX", "locY", "locZ"):
            rows[k] = np.where(cur < 60000, cur + l_units, cur - l_units).astype(np.uint16)
        elif k in VEL:
            rows[k] = (np.float32(0.5) * cur + np.float32(0.0125) * np.arange(1, n + 1, dtype=np.float32)).astype(np.float32)
        elif k.startswith("oriQ"):
            rows[k] = np.full(n, {"oriQw": np.cos(TILT), "oriQx": 0.0, "oriQy": np.sin(TILT), "oriQz": 0.0}[k], np.float32)
        elif k.startswith("omgBar"):
            rows[k] = (np.float32(0.125) * np.arange(1, n + 1, dtype=np.float32)).astype(np.float32)
        elif k == "familyID":
            rows[k] = np.full(n, 1, np.uint8) if families is None else np.asarray(families, np.uint8)
    return rows


def _whole_upload(ctx, ids, rows):
    """the twin's write: the whole state to the host, the rows edited, the same columns back"""
    st = ctx.download_state()
    for k, v in rows.items():
        st[k][np.asarray(ids, np.int64)] = v
    ctx.upload_state({k: st[k] for k in rows})


def _list_of(ctx):
    return dict(zip(("idA", "idB", "type", "map"), ctx.contacts()))


def test_scatter_is_exported_and_bound(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in ("deme_scatter_owner_state", "deme_multi_scatter_owner_state"):
        assert n in names and hasattr(lib, n), n
    assert hasattr(pkg.Context, "scatter_owner_state") and hasattr(pkg.abi.Multi, "scatter_owner_state")


@pytest.mark.parametrize("cols", [POS, VEL, ORI_ANGVEL, FAM, POS + VEL + ORI_ANGVEL + FAM], ids=["pos", "vel", "ori+angvel", "family", "all15"])
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_scatter_equals_the_whole_upload_on_a_bed(pkg, mode, cols):
    """twin equality right after the write and past the next detection; rows not asked for and columns not given keep
    the bits of the download taken before the call"""
    p, sc, mid = _bed_scene(pkg)
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    ids = [nC - 1, mid, nC, 3]  # unsorted: the last clump, a clump in the middle, the first owner behind the clumps
    ctx, twin = _stepped(pkg, p, sc, mode, steps=30), _stepped(pkg, p, sc, mode, steps=30)
    assert ctx.engine_order()[0] == (mode == "fast")  # the fast mode keeps an order of its own: ids go through the slot map
    before, before_twin = ctx.download_state(), twin.download_state()
    _assert_same(before, before_twin, "the twins start alike")
    fam_now = before["familyID"][ids]
    rows = _new_rows(before, ids, cols, families=np.where(np.asarray(ids) < nC, 1, fam_now))  # (the box keeps its family)
    ctx.scatter_owner_state(ids, rows)
    _whole_upload(twin, ids, rows)
    after, after_twin = ctx.download_state(), twin.download_state()
    _assert_same(after, after_twin, f"{mode}: after the write")
    others = np.setdiff1d(np.arange(nO), ids)
    # nothing else moved.  (a / alpha are not the records': a download after a write reads them without the replay of the last
    # step that a download before it launches, as after an upload -- they are held against the twin's above)
    for k in pkg.abi.QUERY_STATE_COLUMNS:
        if k in cols:
            assert np.array_equal(_bits(after[k][ids]), _bits(rows[k])), k
            assert np.array_equal(_bits(after[k][others]), _bits(before[k][others])), k
        else:
            assert np.array_equal(_bits(after[k]), _bits(before[k])), k
    assert any(not np.array_equal(_bits(after[k]), _bits(before[k])) for k in cols)  # the write wrote
    ctx.step(25), twin.step(25)
    ctx.sync(), twin.sync()
    _assert_same(ctx.download_state(), twin.download_state(), f"{mode}: 25 steps later", pkg.abi.QUERY_STATE_COLUMNS)
    _assert_same(_list_of(ctx), _list_of(twin), f"{mode}: the list 25 steps later")
    assert ctx.counts().nDetections == twin.counts().nDetections >= 3
    ctx.close(), twin.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_scatter_to_a_mesh_owner(pkg, mode):
    """pose and velocity of the mesh owner; 40 steps later the twins agree, so the triangles followed"""
    from tests.test_mesh import mesh_bed
    p, sc = mesh_bed(pkg, 600).Initialize()
    nO = int(sc.nOwners)
    ctx, twin = _stepped(pkg, p, sc, mode, steps=10), _stepped(pkg, p, sc, mode, steps=10)
    before = ctx.download_state()
    twin.download_state()
    ids = [nO - 1, 5]
    rows = _new_rows(before, ids, POS + VEL + ("oriQw", "oriQx", "oriQy", "oriQz"), l_units=40)
    ctx.scatter_owner_state(ids, rows)
    _whole_upload(twin, ids, rows)
    _assert_same(ctx.download_state(), twin.download_state(), f"{mode}: after the write")
    ctx.step(40), twin.step(40)
    ctx.sync(), twin.sync()
    _assert_same(ctx.download_state(), twin.download_state(), f"{mode}: 40 steps later", pkg.abi.QUERY_STATE_COLUMNS)
    _assert_same(_list_of(ctx), _list_of(twin), f"{mode}: the list 40 steps later")
    ctx.close(), twin.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_scatter_sets_the_flags_of_an_upload(pkg, mode):
    """a velocity write makes the next step detect; an empty write changes nothing"""
    b = pkg.model.packed_bed(300, seed=11, cd_freq=20, spacing_mult=2.4)
    p, sc = b.Initialize()
    ctx = _stepped(pkg, p, sc, mode, steps=1)
    assert ctx.counts().nDetections == 1
    ctx.scatter_owner_state([7], {"vZ": np.array([-0.3], np.float32)})
    ctx.step(1)
    ctx.sync()
    assert ctx.counts().nDetections == 2
    ctx.close()
    ctx, ref = _stepped(pkg, p, sc, mode, steps=1), _stepped(pkg, p, sc, mode, steps=2)
    ctx.scatter_owner_state([], {"vZ": np.zeros(0, np.float32)})
    ctx.scatter_owner_state([], {})
    ctx.step(1)
    ctx.sync()
    assert ctx.counts().nDetections == 1 and ctx.counts().nSteps == 2
    _assert_same(ctx.download_state(), ref.download_state(), "two uninterrupted steps", pkg.abi.QUERY_STATE_COLUMNS)
    ctx.close(), ref.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_scatter_of_a_family_acts_on_the_next_step(pkg, mode):
    """a clump written into a fixed family stops, one written into a family with a prescribed velocity takes
    it -- in the step after the write, as in the twin"""
    b = pkg.model.packed_bed(300, seed=11, cd_freq=20, spacing_mult=2.4, init_vz=-0.3)
    b.SetFamilyFixed(5)
    b.SetFamilyPrescribedLinVel(7, "0.0125f", "none", "none")
    p, sc = b.Initialize()
    ctxs = []
    for _ in range(3):
        c = pkg.Context(0)
        c.set_arith_mode(mode)
        c.set_params(p), c.upload_scene(sc)
        b.compile_into(c)
        c.step(3)
        c.sync()
        ctxs.append(c)
    ctx, twin, untouched = ctxs
    for c in ctxs:
        c.download_state()
    ids, rows = [11, 200], {"familyID": np.array([5, 7], np.uint8)}
    ctx.scatter_owner_state(ids, rows)
    _whole_upload(twin, ids, rows)
    for c in ctxs:
        c.step(2)
        c.sync()
    after, plain = ctx.download_state(), untouched.download_state()
    _assert_same(after, twin.download_state(), mode, pkg.abi.QUERY_STATE_COLUMNS)
    assert list(after["familyID"][ids]) == [5, 7] and list(plain["familyID"][ids]) == [0, 0]
    # the families act from the step after the write: the prescribed velocity is there, and the clump of the fixed family no
    # longer takes the acceleration the same clump takes in a run without the write
    assert after["vX"][200] == np.float32(0.0125) and plain["vX"][200] != np.float32(0.0125)
    assert after["vZ"][11] != plain["vZ"][11]
    for c in ctxs:
        c.close()


def _refusals(pkg, target, n_owners):
    """the refused calls on a Context or a Multi, each with a message that names its cause"""
    one = np.array([0.5], np.float32)
    with pytest.raises(pkg.abi.DemeError, match="out of range"):
        target.scatter_owner_state([0, n_owners], {"vX": np.array([1, 2], np.float32)})
    with pytest.raises(pkg.abi.DemeError, match="given twice"):
        target.scatter_owner_state([4, 9, 4], {"vX": np.array([1, 2, 3], np.float32)})
    for k in ("aX", "alphaZ"):
        with pytest.raises(pkg.abi.DemeError, match="deme_upload_owner_state"):
            target.scatter_owner_state([2], {"vX": one, k: one})
    with pytest.raises(pkg.abi.DemeError, match="null owner id array"):
        target.scatter_owner_state(None, {"vX": one}, n=1)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_scatter_refusals_change_nothing(pkg, mode):
    """afterwards the whole state is the download before, and one more step does not detect: the flags are untouched"""
    b = pkg.model.packed_bed(300, seed=11, cd_freq=20, spacing_mult=2.4)
    p, sc = b.Initialize()
    ctx = _stepped(pkg, p, sc, mode, steps=1)
    before = ctx.download_state()
    bytes_before = ctx.query_host_bytes()
    _refusals(pkg, ctx, int(sc.nOwners))
    _assert_same(ctx.download_state(), before, "after the refusals")
    assert ctx.query_host_bytes() == bytes_before
    ctx.step(1)
    ctx.sync()
    assert ctx.counts().nDetections == 1 and ctx.counts().nSteps == 2
    ctx.close()


def test_scatter_bytes_do_not_depend_on_the_bed(pkg):
    """68 bytes per id (the header's formula), at 300 and at 1 200 clumps"""
    moved = []
    for n_clumps in (300, 1200):
        p, sc = pkg.model.packed_bed(n_clumps, seed=11, cd_freq=20, spacing_mult=2.4).Initialize()
        ctx = _stepped(pkg, p, sc, "fast", steps=1)
        ids = [5, 250, int(sc.nOwnerClumps), 17, 1]
        rows = _new_rows(ctx.download_state(), ids, VEL + FAM, families=ctx.download_state()["familyID"][ids])
        at = ctx.query_host_bytes()
        ctx.scatter_owner_state(ids, rows)
        moved.append(ctx.query_host_bytes() - at)
        ctx.scatter_owner_state([], {})
        assert ctx.query_host_bytes() - at == moved[-1]
        ctx.close()
    assert moved == [PER_ID * 5, PER_ID * 5]


@pytest.mark.parametrize("n_slabs", [3, 2])
def test_multi_scatter_equals_the_whole_upload(pkg, n_slabs):
    """by global id on a decomposed run; every copy is written -- the owning slab's, the ghost in the neighbour, the
    replicated owners on every slab -- so every slab's own context holds what the twin's holds"""
    p, sc = bed_scene(pkg)
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    m, twin = built(pkg, p, sc, n_slabs), built(pkg, p, sc, n_slabs)
    for r in (m, twin):
        r.step(STEPS)
        r.sync()
    before = m.download_state()
    _assert_same(before, twin.download_state(), "the twins start alike")
    plan, parts = pkg.decomp.decompose_lib(p, sc, n_slabs, HALO, axis=0, snap=True, spatial_order=True)
    ghost = int(parts[1]["ghost_left_g"][0])  # slab 0's clump inside slab 1's halo: two slabs hold a copy
    x = pkg.model.decode_positions(before["voxelID"], before["locX"], before["locY"], before["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)[:nC, 0] + p.LBFX
    own = parts[n_slabs - 1]["global_ids"]
    deep = int(own[np.argmax(x[own])])  # the clump of the last slab farthest from its cut
    plan.close()
    ids = list(dict.fromkeys([ghost, deep, nC, nO - 1]))  # (nC: the box, replicated -- in this scene also the last owner)
    assert len(ids) >= 3
    rows = _new_rows(before, ids, POS + VEL + ("oriQw", "oriQx", "oriQy", "oriQz"), l_units=1)
    # A slab's ghost copies are refreshed at the start of a step, so after the last step they lag their owners by that step.  The
    # whole upload writes every copy of EVERY owner and so brings all ghosts up to date; the scatter writes the copies of the asked
    # owners only and leaves the rest to the next step's exchange.  Both runs therefore start from a round trip of the same columns,
    # unchanged: from there on every slab's context must hold the same bits, ghosts of owners not asked for included.
    for r in (m, twin):
        st0 = r.download_state()
        r.upload_state({k: st0[k] for k in rows})
    _assert_same(m.download_state(), before, "the round trip changes no owner")
    _refusals(pkg, m, nO)
    _assert_same(m.download_state(), before, "after the refusals")
    at = m.query_host_bytes()
    m.scatter_owner_state(ids, rows)
    assert m.query_host_bytes() - at == PER_ID * len(ids) * n_slabs
    st = twin.download_state()
    for k, v in rows.items():
        st[k][ids] = v
    twin.upload_state({k: st[k] for k in rows})
    after = m.download_state()
    _assert_same(after, twin.download_state(), f"{n_slabs} slabs: after the write")
    for k, v in rows.items():
        assert np.array_equal(_bits(after[k][ids]), _bits(v)), k
    copies = 0
    for s in range(n_slabs):  # ghost and replicated copies too
        a, b = m.slab_ctx(s).download_state(), twin.slab_ctx(s).download_state()
        _assert_same(a, b, f"slab {s} of {n_slabs}", pkg.abi.QUERY_STATE_COLUMNS)
        copies += int(np.sum(_bits(a["vZ"]) == _bits(rows["vZ"])[0]))  # the ghost clump's new vZ, wherever a copy of it lives
    assert copies >= 2
    m.step(STEPS), twin.step(STEPS)
    m.sync(), twin.sync()
    _assert_same(m.download_state(), twin.download_state(), f"{n_slabs} slabs: {STEPS} steps later", pkg.abi.QUERY_STATE_COLUMNS)
    _assert_same(dict(zip("abt", m.contacts())), dict(zip("abt", twin.contacts())), f"{n_slabs} slabs: the merged list")
    m.close(), twin.close()


@pytest.mark.parametrize("n_slabs", [3, 2])
def test_multi_scatter_sets_the_flags_on_every_slab(pkg, n_slabs):
    """no upload anywhere in this run, so only the scatter can mark the lists stale: with a detection every 7 steps, a step after
    the refused calls detects on no slab, and a step after one velocity written to one clump detects on every slab"""
    p, sc = bed_scene(pkg)
    m = built(pkg, p, sc, n_slabs)
    per_slab = lambda: [int(m.slab_ctx(s).counts().nDetections) for s in range(n_slabs)]
    m.step(1)
    m.sync()
    assert per_slab() == [1] * n_slabs
    _refusals(pkg, m, int(sc.nOwners))
    m.scatter_owner_state([], {"vZ": np.zeros(0, np.float32)})
    m.step(1)
    m.sync()
    assert per_slab() == [1] * n_slabs
    m.scatter_owner_state([5], {"vZ": np.array([-0.3], np.float32)})
    m.step(1)
    m.sync()
    assert per_slab() == [2] * n_slabs
    m.close()


def _pattern(pkg, name, n, salt):
    """n values of column `name` with a bit pattern of their own per owner and per salt (the family has 251 of them to give)"""
    i = np.arange(n, dtype=np.uint64)
    dt = pkg.abi.STATE_DTYPES[name]
    if dt == np.float32:  # finite, positive, none of them a value a scene would hold
        return (np.uint64(0x3C000000 + 0x10000 * salt + 1) + np.uint64(7) * i).astype(np.uint32).view(np.float32)
    if dt == np.uint64:
        return np.uint64(0x0000000100000003) * (i + np.uint64(1)) + np.uint64(salt)
    if dt == np.uint16:
        return (np.uint64(1000 * salt + 1) + np.uint64(5) * i).astype(np.uint16)
    return ((np.uint64(7) * i + np.uint64(salt)) % np.uint64(251)).astype(np.uint8)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_every_column_lands_in_its_own_field(pkg, mode):
    """Column by column at the ABI, on 300 clumps in random order, a box and a mesh owner, with no step taken (a / alpha are plain
    storage then): one column uploaded alone reads back bit for bit and leaves the other 20 as they were -- a column paired with
    its neighbour's field would pass every twin test above.  Then the 15 pose columns through the scatter, on a few ids.  (300
    clumps, not fewer: the engine keeps an order of its own only beyond two tiles of 128, and the fast leg is to go through it.)"""
    b = pkg.model.packed_bed(300, seed=3, cd_freq=0, spacing_mult=2.8, order="random")
    lo, hi = b.user_box_min, b.user_box_max
    v, f = pkg.model.plate_mesh(4, 4, float(hi[0] - lo[0]) * 0.9, float(hi[1] - lo[1]) * 0.9, z=0.0, wavy=0.003)
    m = b.AddMeshObject(v, f, 0)
    m.SetInitPos(((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, 0.0195))
    m.SetMass(0.5), m.SetMOI((1e-3, 1e-3, 2e-3))
    p, sc = b.Initialize()
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    assert nC == 300 and nO == nC + 2 and int(sc.nTri) > 0 and int(sc.nAnal) > 0
    ctx = pkg.Context(0)
    ctx.set_arith_mode(mode)
    ctx.set_params(p), ctx.upload_scene(sc)
    assert ctx.engine_order()[0] == (mode == "fast")
    cols = list(pkg.abi.STATE_DTYPES)
    assert len(cols) == 21
    for salt, k in enumerate(cols):
        before = ctx.download_state()
        new = _pattern(pkg, k, nO, salt)
        ctx.upload_state({k: new})
        after = ctx.download_state()
        assert np.array_equal(_bits(after[k]), _bits(new)), (mode, "upload", k)
        for other in cols:
            if other != k:
                assert np.array_equal(_bits(after[other]), _bits(before[other])), (mode, "upload of", k, "moved", other)
    ids = np.array([nO - 1, 7, nC, 130, nC - 1, 0], np.int64)  # unsorted: the mesh owner, the box, clumps of both tiles
    rest = np.setdiff1d(np.arange(nO), ids)
    assert pkg.abi.QUERY_STATE_COLUMNS == tuple(c for c in cols if not c.startswith(("a", "alpha")))
    for salt, k in enumerate(pkg.abi.QUERY_STATE_COLUMNS, start=len(cols)):
        before = ctx.download_state()
        new = _pattern(pkg, k, len(ids), salt)
        ctx.scatter_owner_state(ids, {k: new})
        after = ctx.download_state()
        assert np.array_equal(_bits(after[k][ids]), _bits(new)), (mode, "scatter", k)
        assert np.array_equal(_bits(after[k][rest]), _bits(before[k][rest])), (mode, "scatter", k, "other owners")
        for other in cols:
            if other != k:
                assert np.array_equal(_bits(after[other]), _bits(before[other])), (mode, "scatter of", k, "moved", other)
    ctx.close()
