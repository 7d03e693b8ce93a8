"""deme_query_owner_contacts / Context.owner_contacts: the rows of the contact list that touch a few owners, selected on the
device.  Every value is copied, never recomputed, so every comparison is np.array_equal against the numpy filter of the whole-list
downloads (contacts() + contact_records()) and the scene's sphere / triangle / component owner tables.

The bed: 300 three-sphere clumps (more than two tiles of 128 owners, so the fast mode keeps an order of its own) lowered onto the
floor of their box so that the list holds sphere--plane rows at the first detection; the last clump stays where the lattice put
it, clear of the others, as the owner without contacts.  With seed 11 the CPU oracle lists 573 rows after the first step (64 of
them against the box): three workgroups, a partial last wavefront."""
import ctypes as C

import numpy as np
import pytest

COUNTS = ("nOwners", "nOwnerClumps", "nSpheres", "nAnal", "nTri", "nMat", "nComp", "nMassProps")
N_BED, SEED = 300, 11
FIELDS = ("idA", "idB", "type", "ownerA", "ownerB", "side")
RECORDS = ("force", "torqueOnly", "cpA", "cpB")
_cache = {}


def test_owner_query_is_exported_and_bound(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in ("deme_query_owner_contacts", "deme_query_host_bytes"):
        assert n in names and hasattr(lib, n), n
    assert hasattr(pkg.Context, "owner_contacts") and hasattr(pkg.Context, "query_host_bytes")


def _bed_scene(pkg):
    if "bed" not in _cache:
        b = pkg.model.packed_bed(N_BED, seed=SEED, cd_freq=20, spacing_mult=2.4)
        p, sc = b.Initialize()
        arr = {k: np.array(v, copy=True) for k, v in sc._keep.items()}
        counts = {k: int(getattr(sc, k)) for k in COUNTS}
        nC = counts["nOwnerClumps"]
        X = pkg.model.decode_positions(arr["voxelID"], arr["locX"], arr["locY"], arr["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
        # the lowest clump centre 4.5 mm above the floor (z = 0 of the box; sphere radius 4 mm); the last clump is left behind
        X[:nC - 1, 2] -= (X[:nC, 2].min() + p.LBFZ) - 0.0045
        arr["voxelID"], arr["locX"], arr["locY"], arr["locZ"] = pkg.model.encode_positions(X, p.nvXp2, p.nvYp2, p.voxelSize, p.l)
        centre = X[:nC - 1].mean(0)
        _cache["bed"] = (p, pkg.abi.make_scene_struct(arr, counts), int(np.argmin(((X[:nC - 1] - centre) ** 2).sum(1))))
    return _cache["bed"]


def _owner_tables(sc):
    keep = sc._keep
    return (np.asarray(keep["ownerClumpBody"], np.uint32), np.asarray(keep.get("ownerMesh", np.zeros(0)), np.uint32),
            np.asarray(keep.get("objOwner", np.zeros(0)), np.uint32))


def _stepped(pkg, p, sc, mode, steps=1, record=True):
    c = pkg.Context(0)
    c.set_arith_mode(mode)
    c.set_params(p)
    c.upload_scene(sc)
    c.set_record_contacts(record)
    c.step(steps)
    c.sync()
    return c


def _whole_list(ctx, sc):
    """the list, its records and both owners of every row: what the filter below selects from"""
    a, b, t, _ = ctx.contacts()
    rec = ctx.contact_records()
    sph, tri, obj = _owner_tables(sc)
    oB = np.zeros(len(a), np.uint32)
    for cls, table in ((t == 1, sph), (t == 2, tri), (t > 2, obj)):
        oB[cls] = table[b[cls]]
    return {"idA": a, "idB": b, "type": t, "ownerA": sph[a], "ownerB": oB, **dict(zip(RECORDS, rec))}


def _filter(whole, ids, n_owners):
    mark = np.zeros(n_owners, bool)
    mark[np.asarray(ids, np.int64)] = True
    mA, mB = mark[whole["ownerA"]], mark[whole["ownerB"]]
    hit = mA | mB
    out = {k: v[hit] for k, v in whole.items()}
    out["side"] = np.where(mA[hit], 0, 1).astype(np.uint8)
    return out


def _same(got, want, what):
    for k in FIELDS + RECORDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k} {got[k].shape} vs {want[k].shape}"
        assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                              want[k].view(np.uint32) if want[k].dtype == np.float32 else want[k]), f"{what}: {k} differs"


@pytest.fixture(scope="module", params=["fast", "exact"])
def bed(pkg, request):
    p, sc, mid = _bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, request.param)
    yield {"ctx": ctx, "sc": sc, "mid": mid, "mode": request.param, "whole": _whole_list(ctx, sc)}
    ctx.close()


@pytest.mark.gpu
def test_bed_list_exercises_what_it_should(bed):
    n = len(bed["whole"]["idA"])
    print(f"{bed['mode']}: {n} rows, engine order {bed['ctx'].engine_order()}")
    assert n > 256 and n % 64 != 0
    # the fast mode keeps an order of its own for this bed (otherwise its leg tests no translation), the exact mode the caller's
    assert bed["ctx"].engine_order()[0] == (bed["mode"] == "fast")
    assert (bed["whole"]["type"] == 1).any() and (bed["whole"]["type"] == 11).any()
    assert np.abs(bed["whole"]["force"]).max() > 0


def _cases(bed):
    sc, whole = bed["sc"], bed["whole"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    rng = np.random.default_rng(5)
    return nO, nC, {
        "a: one clump in the middle": [bed["mid"]],
        "b: the box (B side only)": [nC],
        "c: every owner": list(range(nO)),
        "d: an owner without contacts": [nC - 1],
        "e: no owner": [],
        "g: 65 scattered clumps": sorted(rng.choice(nC, 65, replace=False).tolist()),
    }


@pytest.mark.gpu
def test_owner_contacts_equal_the_filtered_whole_list(bed):
    ctx, whole = bed["ctx"], bed["whole"]
    nO, nC, cases = _cases(bed)
    for what, ids in cases.items():
        want = _filter(whole, ids, nO)
        got = ctx.owner_contacts(ids, records=True)
        print(f"{bed['mode']} {what}: {len(got['idA'])} rows")
        _same(got, want, f"{bed['mode']}, {what}")
        bare = ctx.owner_contacts(ids)  # without records: the same rows, no record arrays
        assert set(bare) == set(FIELDS) and all(np.array_equal(bare[k], want[k]) for k in FIELDS), what
    n = len(whole["idA"])
    assert len(_filter(whole, cases["a: one clump in the middle"], nO)["idA"]) > 0
    assert (_filter(whole, [nC], nO)["side"] == 1).all() and len(_filter(whole, [nC], nO)["idA"]) > 32
    assert len(_filter(whole, list(range(nO)), nO)["idA"]) == n
    assert len(_filter(whole, [nC - 1], nO)["idA"]) == 0
    # (f) repeated ids are the de-duplicated question
    ids = cases["g: 65 scattered clumps"]
    twice = ctx.owner_contacts(ids + ids[::-1] + [ids[0]] * 3, records=True)
    _same(twice, _filter(whole, ids, nO), f"{bed['mode']}, f: repeated ids")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_first_query_grows_its_scratch_and_moves_only_the_hits(pkg, mode):
    """A context that has answered no question yet -- no scratch, no cached caller's view of the list.  Every owner at once is
    more rows than the first scratch holds: the selection runs twice (two 4-byte count read-backs) and no row is lost.  Then one
    clump: what comes to the host (deme_query_host_bytes: the count read-back and the hit rows; the answer fits the buffers
    owner_contacts starts with, so it is one call) against the bytes of the list itself -- 8 of key and 48 of records a row,
    what a whole-list answer moves once -- must stay below 1 %."""
    p, sc, mid = _bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, mode)
    nO = int(sc.nOwners)
    n = int(ctx.counts().nContacts)
    assert n > 256
    lib, cnt = ctx.lib, C.c_size_t(0)
    ids = np.arange(nO, dtype=np.uint32)
    rc = lib.deme_query_owner_contacts(ctx.h, ids.ctypes.data, ids.size, 1, *([None] * 10), 0, C.byref(cnt))
    assert rc == 1 and cnt.value == n and ctx.query_host_bytes() == 8
    everything = ctx.owner_contacts(ids, records=True)
    before = ctx.query_host_bytes()
    one = ctx.owner_contacts([mid], records=True)
    moved = ctx.query_host_bytes() - before
    hits = len(one["idA"])
    print(f"{mode}: {hits} of {n} rows, {moved} bytes to the host, list {56 * n} bytes, ratio {moved / (56 * n):.4f}")
    assert 0 < hits <= 64 and moved == 4 + 72 * hits
    assert moved < 0.01 * 56 * n
    # only now is the whole list brought over, to check both answers
    whole = _whole_list(ctx, sc)
    _same(everything, _filter(whole, ids, nO), f"{mode}, every owner on a fresh context")
    _same(one, _filter(whole, [mid], nO), f"{mode}, one clump on a fresh context")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_mesh_owner_gets_the_rows_of_its_triangles(pkg, mode):
    """600 clumps on a plate: in the fast mode the engine keeps an order of its own, so the triangle's owner goes through the
    owner translation while the triangle id in the key stays as it is"""
    from tests.test_mesh import mesh_bed
    b = mesh_bed(pkg, 600)
    p, sc = b.Initialize()
    ctx = _stepped(pkg, p, sc, mode, steps=150)
    assert ctx.engine_order()[0] == (mode == "fast")
    whole = _whole_list(ctx, sc)
    nO = int(sc.nOwners)
    mesh = nO - 1
    sm = whole["type"] == 2
    assert sm.sum() > 20 and (whole["ownerB"][sm] == mesh).all()
    got = ctx.owner_contacts([mesh], records=True)
    _same(got, _filter(whole, [mesh], nO), f"{mode}, mesh owner")
    assert len(got["idA"]) == sm.sum() and (got["type"] == 2).all() and (got["side"] == 1).all()
    assert np.array_equal(got["idB"], whole["idB"][sm]) and np.abs(got["force"]).max() > 0
    # a clump resting on the plate: its rows include sphere--triangle rows, A side
    clump = int(whole["ownerA"][sm][0])
    _same(ctx.owner_contacts([clump], records=True), _filter(whole, [clump], nO), f"{mode}, a clump on the mesh")
    ctx.close()


def _raw_query(ctx, ids, records, cap, fill=0xAB):
    ids = np.ascontiguousarray(ids, np.uint32)
    bufs = [np.full(max(cap, 4), fill, dt) for dt in (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint8)]
    bufs += [np.full((max(cap, 4), 3), np.float32(7.5), np.float32) for _ in range(4)]
    n = C.c_size_t(12345)
    rc = ctx.lib.deme_query_owner_contacts(ctx.h, ids.ctypes.data, ids.size, int(records), *[x.ctypes.data for x in bufs], cap, C.byref(n))
    untouched = all((x == fill).all() for x in bufs[:6]) and all((x == np.float32(7.5)).all() for x in bufs[6:])
    return rc, int(n.value), untouched, ctx.lib.deme_last_error(ctx.h).decode()


@pytest.mark.gpu
def test_owner_query_refusals(pkg, bed):
    ctx, sc = bed["ctx"], bed["sc"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    rc, n, untouched, msg = _raw_query(ctx, [bed["mid"], nO], True, 4096)
    assert rc == 1 and n == 12345 and untouched and "out of range" in msg
    with pytest.raises(pkg.abi.DemeError, match="out of range"):
        ctx.owner_contacts([nO + 7])
    # a buffer that is too small: the count comes back, no row does
    want = len(_filter(bed["whole"], [nC], nO)["idA"])
    rc, n, untouched, msg = _raw_query(ctx, [nC], True, want - 1)
    assert rc == 1 and n == want and untouched and str(want) in msg
    rc, n, untouched, _ = _raw_query(ctx, [nC], True, want)
    assert rc == 0 and n == want and not untouched
    # records while recording is off: the message of deme_download_contact_records
    p, sc2, mid = _bed_scene(pkg)
    off = _stepped(pkg, p, sc2, bed["mode"], record=False)
    with pytest.raises(pkg.abi.DemeError) as whole_list:
        off.contact_records()
    want_msg = off.lib.deme_last_error(off.h).decode()
    assert "recording is off" in want_msg and want_msg in str(whole_list.value)
    rc, n, untouched, msg = _raw_query(off, [mid], True, 4096)
    assert rc == 1 and n == 12345 and untouched and msg == want_msg
    assert len(off.owner_contacts([mid])["idA"]) == len(_filter(bed["whole"], [mid], nO)["idA"])  # without records it answers
    off.close()
