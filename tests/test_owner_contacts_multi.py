"""deme_multi_query_owner_contacts / Multi.owner_contacts: the rows of a decomposed run's merged contact list that touch a few
owners, selected on every slab's device.  Every value is copied (a flipped row's force negated, its contact points swapped, as
deme_multi_download_contact_records does), never recomputed, so every comparison is np.array_equal on bit patterns against the
numpy filter of the whole-list downloads (Multi.contacts() + Multi.contact_records()) and the scene's owner tables.

The bed is that of tests/test_multi.py (1600 three-sphere clumps, a detection every 7 steps) lowered onto the floor of its box so
that the list holds sphere--plane rows; the last clump stays where the lattice put it, as the owner without contacts.  With the
CPU oracle and the library's plan (decompose_lib, spatial_order=True) the list after 60 steps has 2 881 rows (2 726 sphere--sphere,
155 sphere--plane; 1 856 carry a force); in 3 slabs 347 reported rows are flipped, 129 straddle a cut and all three slabs report
plane rows (55 / 48 / 52); in 2 slabs 367 are flipped and 70 straddle the cut; no clump has more than 10 rows."""
import ctypes as C

import numpy as np
import pytest

from tests.test_decomp import _sheared_bed

COUNTS = ("nOwners", "nOwnerClumps", "nSpheres", "nAnal", "nTri", "nMat", "nComp", "nMassProps")
FIELDS = ("idA", "idB", "type", "ownerA", "ownerB", "side")
RECORDS = ("force", "torqueOnly", "cpA", "cpB")
HALO, STEPS = 0.03, 60
_cache = {}


def test_multi_owner_queries_are_exported_and_bound(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in ("deme_multi_query_owner_contacts", "deme_multi_query_host_bytes", "deme_query_owner_state", "deme_multi_query_owner_state"):
        assert n in names and hasattr(lib, n), n
    for cls, methods in ((pkg.abi.Multi, ("owner_contacts", "query_host_bytes", "owner_state")), (pkg.Context, ("owner_state",))):
        for meth in methods:
            assert hasattr(cls, meth), (cls.__name__, meth)


def bed_scene(pkg):
    """(params, scene): the bed of tests/test_multi.py::_bed with cd_freq 7, every clump but the last lowered onto the floor"""
    if "bed" not in _cache:
        b = pkg.model.packed_bed(1600, seed=4, cd_freq=7, spacing_mult=2.5, init_vz=-0.4, aspect=(2.0, 1.0, 0.5))
        b.SetExpandSafetyAdder(0.5)
        p, sc = b.Initialize()
        arr = {k: np.array(v, copy=True) for k, v in sc._keep.items()}
        counts = {k: int(getattr(sc, k)) for k in COUNTS}
        nC = counts["nOwnerClumps"]
        X = pkg.model.decode_positions(arr["voxelID"], arr["locX"], arr["locY"], arr["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
        X[:nC - 1, 2] -= (X[:nC, 2].min() + p.LBFZ) - 0.0045  # the lowest clump centre 4.5 mm above the floor (z = 0)
        arr["voxelID"], arr["locX"], arr["locY"], arr["locZ"] = pkg.model.encode_positions(X, p.nvXp2, p.nvYp2, p.voxelSize, p.l)
        _cache["bed"] = (p, pkg.abi.make_scene_struct(arr, counts))
    return _cache["bed"]


def built(pkg, p, sc, n_slabs, halo=HALO, record=True, arith="exact", migration=0):
    m = pkg.abi.Multi(devices=(0,))
    m.build(p, sc, slabs_per_device=n_slabs, axis=0, halo=halo, arith=arith)
    if migration:
        m.set_migration(migration)
    for s in range(n_slabs):
        m.slab_ctx(s).set_record_contacts(record)
    return m


def owner_tables(sc):
    keep = sc._keep
    return (np.asarray(keep["ownerClumpBody"], np.uint32), np.asarray(keep.get("ownerMesh", np.zeros(0)), np.uint32),
            np.asarray(keep.get("objOwner", np.zeros(0)), np.uint32))


def whole_list(m, sc, records=True):
    """the merged list, its records and both (global) owners of every row: what the filter below selects from"""
    a, b, t = m.contacts()
    sph, tri, obj = owner_tables(sc)
    oB = np.zeros(len(a), np.uint32)
    for cls, table in ((t == 1, sph), (t == 2, tri), (t > 2, obj)):
        oB[cls] = table[b[cls]]
    out = {"idA": a, "idB": b, "type": t, "ownerA": sph[a], "ownerB": oB}
    if records:
        out.update(dict(zip(RECORDS, m.contact_records())))
    return out


def filtered(whole, ids, n_owners):
    mark = np.zeros(n_owners, bool)
    mark[np.asarray(ids, np.int64)] = True
    mA, mB = mark[whole["ownerA"]], mark[whole["ownerB"]]
    hit = mA | mB
    out = {k: v[hit] for k, v in whole.items()}
    out["side"] = np.where(mA[hit], 0, 1).astype(np.uint8)
    return out


def same(got, want, what, keys=FIELDS + RECORDS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k} {got[k].shape} vs {want[k].shape}"
        assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                              want[k].view(np.uint32) if want[k].dtype == np.float32 else want[k]), f"{what}: {k} differs"


def plan_facts(pkg, p, sc, n_slabs, whole):
    """from the library's plan (what deme_multi_build cuts): per row of the merged list the slab that reports it, whether that slab
    holds the pair the other way round, and whether the two clumps belong to different slabs"""
    plan, parts = pkg.decomp.decompose_lib(p, sc, n_slabs, HALO, axis=0, snap=True, spatial_order=True)
    nC, nS = int(sc.nOwnerClumps), int(sc.nSpheres)
    slab_of = np.full(int(sc.nOwners), -1, np.int64)
    local = np.full((n_slabs, nS), -1, np.int64)  # global sphere id -> the slab's own id
    for r, pt in enumerate(parts):
        slab_of[pt["global_ids"]] = r
        local[r, pt["sphere_global"]] = np.arange(len(pt["sphere_global"]))
    assert (slab_of[:nC] >= 0).all()
    ss = whole["type"] == 1
    rep = slab_of[whole["ownerA"]]
    la, lb = local[rep, whole["idA"]], local[rep[ss], whole["idB"][ss]]
    assert (la >= 0).all() and (lb >= 0).all()  # the reporting slab holds both spheres
    flipped = np.zeros(len(rep), bool)
    flipped[ss] = la[ss] > lb
    cross = np.zeros(len(rep), bool)
    cross[ss] = slab_of[whole["ownerB"][ss]] != rep[ss]
    plan.close()
    return rep, flipped, cross, slab_of


@pytest.fixture(scope="module", params=[3, 2])
def run(pkg, request):
    p, sc = bed_scene(pkg)
    m = built(pkg, p, sc, request.param)
    m.step(STEPS)
    m.sync()
    whole = whole_list(m, sc)
    yield {"m": m, "p": p, "sc": sc, "n_slabs": request.param, "whole": whole}
    m.close()


def cut_clump(whole, slab_of, cross):
    """a clump with sphere--sphere rows whose other clump is in another slab and rows whose other clump is in its own"""
    ss = whole["type"] == 1
    for o in np.unique(whole["ownerA"][cross]):
        mine = ss & ((whole["ownerA"] == o) | (whole["ownerB"] == o))
        others = np.where(whole["ownerA"][mine] == o, whole["ownerB"][mine], whole["ownerA"][mine])
        if len(set(slab_of[others].tolist())) > 1:
            return int(o)
    raise AssertionError("no clump with neighbours in two slabs")


@pytest.mark.gpu
def test_bed_list_exercises_what_it_should(pkg, run):
    whole, n_slabs = run["whole"], run["n_slabs"]
    n = len(whole["idA"])
    rep, flipped, cross, slab_of = plan_facts(pkg, run["p"], run["sc"], n_slabs, whole)
    plane = whole["type"] > 2
    per_clump = np.bincount(np.concatenate([whole["ownerA"], whole["ownerB"][whole["type"] == 1]]))
    print(f"{n_slabs} slabs: {n} rows, {(whole['type'] == 1).sum()} sphere-sphere, {plane.sum()} plane, {(np.abs(whole['force']).max(1) > 0).sum()} with "
          f"a force, {flipped.sum()} flipped, {cross.sum()} across a cut, plane rows per slab {np.bincount(rep[plane], minlength=n_slabs)}, "
          f"most rows of one clump {per_clump[:int(run['sc'].nOwnerClumps)].max()}")
    assert n > 256
    assert (whole["type"] == 1).any() and plane.any()
    assert np.abs(whole["force"]).max() > 0
    assert flipped.sum() > 0 and cross.sum() > 0
    assert len(np.unique(rep[plane])) > 1


@pytest.mark.gpu
def test_rows_equal_the_filtered_merged_list(pkg, run):
    m, sc, whole = run["m"], run["sc"], run["whole"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    rep, flipped, cross, slab_of = plan_facts(pkg, run["p"], sc, run["n_slabs"], whole)
    rng = np.random.default_rng(5)
    scattered = sorted(rng.choice(nC, 65, replace=False).tolist())
    cases = {
        "a: one clump with neighbours in two slabs": [cut_clump(whole, slab_of, cross)],
        "b: the box (B side only, a replicated owner)": [nC],
        "c: every owner": list(range(nO)),
        "d: the contact-free last clump": [nC - 1],
        "e: no owner": [],
        "g: 65 scattered clumps": scattered,
        "f: repeated ids": scattered + scattered[::-1] + [scattered[0]] * 3,
    }
    for what, ids in cases.items():
        want = filtered(whole, ids, nO)
        got = m.owner_contacts(ids, records=True)
        print(f"{run['n_slabs']} slabs, {what}: {len(got['idA'])} rows")
        same(got, want, f"{run['n_slabs']} slabs, {what}")
        bare = m.owner_contacts(ids)  # without records: the same rows, no record arrays
        assert set(bare) == set(FIELDS) and all(np.array_equal(bare[k], want[k]) for k in FIELDS), what
    one = filtered(whole, cases["a: one clump with neighbours in two slabs"], nO)
    assert len(one["idA"]) > 1
    box = filtered(whole, [nC], nO)
    assert (box["side"] == 1).all() and len(box["idA"]) > 32
    assert len(filtered(whole, list(range(nO)), nO)["idA"]) == len(whole["idA"])
    assert len(filtered(whole, [nC - 1], nO)["idA"]) == 0
    # the flipped rows are among the answers checked above: the scattered clumps alone touch some
    hit = np.isin(whole["ownerA"], scattered) | np.isin(whole["ownerB"], scattered)
    assert (hit & flipped).any() and (hit & cross).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n_slabs", [3, 2])
def test_first_query_grows_its_scratch_and_moves_only_the_hits(pkg, n_slabs):
    """A run that has answered no question yet and has never merged its list.  Every owner at once is more rows than the first
    scratch of a slab holds (256): those slabs select twice and no row is lost.  Then one clump: the counter's increase is the
    header's formula -- 4 bytes per slab (one pass each) and 72 per hit row with records -- and stays below 1 % of the list's own
    56 bytes a row (at most 10 rows a clump on this bed: 80 bytes a row and 12 of counts are about 0.5 %)."""
    p, sc = bed_scene(pkg)
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    m = built(pkg, p, sc, n_slabs)
    m.step(STEPS)
    m.sync()
    per_slab = [int(m.slab_ctx(s).counts().nContacts) for s in range(n_slabs)]
    assert all(k > 256 for k in per_slab)
    assert m.query_host_bytes() == 0
    ids = np.arange(nO, dtype=np.uint32)
    cnt = C.c_size_t(0)
    _argtypes(m)
    rc = m.lib.deme_multi_query_owner_contacts(m.h, ids.ctypes.data, ids.size, 1, *([None] * 10), 0, C.byref(cnt))
    n = int(cnt.value)
    assert rc == 1 and n > 256 and m.query_host_bytes() == 8 * n_slabs  # two passes on every slab, no row moved
    everything = m.owner_contacts(ids, records=True)
    # (the scratch is kept: one pass a call now; owner_contacts asks twice, its first buffers hold 64 rows)
    assert m.query_host_bytes() == 8 * n_slabs + 2 * 4 * n_slabs + 72 * n
    clump = nC // 2
    before = m.query_host_bytes()
    one = m.owner_contacts([clump], records=True)
    moved = m.query_host_bytes() - before
    hits = len(one["idA"])
    print(f"{n_slabs} slabs: {hits} of {n} rows, {moved} bytes to the host, list {56 * n} bytes, ratio {moved / (56 * n):.4f}")
    assert moved == 4 * n_slabs + 72 * hits
    assert moved < 0.01 * 56 * n
    # only now is the merged list built, to check both answers
    whole = whole_list(m, sc)
    assert len(whole["idA"]) == n
    same(everything, filtered(whole, ids, nO), f"{n_slabs} slabs, every owner on a fresh run")
    same(one, filtered(whole, [clump], nO), f"{n_slabs} slabs, one clump on a fresh run")
    assert 0 < hits <= 10
    m.close()


@pytest.mark.gpu
def test_rows_follow_the_clumps_after_a_migration(pkg):
    """the sheared bed of test_multi_migrates_a_drifting_bed: clumps change slabs every 50 steps, the device books follow them and
    so does the selection; step 151 follows the last migration, so its contacts are evaluated and recorded.  Directly after a
    migrating step the lists are seeds: records are refused with the whole-list call's words."""
    b, p, sc, x = _sheared_bed(pkg, 20_000, 6)
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    m = built(pkg, p, sc, 3, halo=0.035, migration=50)
    m.step(150)
    m.sync()
    with pytest.raises(pkg.abi.DemeError) as whole_call:
        m.contact_records()
    want_msg = m.lib.deme_multi_last_error(m.h).decode()
    assert "seed" in want_msg and want_msg in str(whole_call.value)
    with pytest.raises(pkg.abi.DemeError) as query_call:
        m.owner_contacts([nC], records=True)
    assert m.lib.deme_multi_last_error(m.h).decode() == want_msg and want_msg in str(query_call.value)
    seeded = whole_list(m, sc, records=False)  # without records the seeded lists answer
    same(m.owner_contacts([nC]), filtered(seeded, [nC], nO), "the box, seeded lists", keys=FIELDS)
    m.step(1)
    m.sync()
    cnt, moved = m.counts()
    assert moved > 20, moved
    whole = whole_list(m, sc)
    rng = np.random.default_rng(7)
    scattered = sorted(rng.choice(nC, 65, replace=False).tolist())
    assert len(whole["idA"]) > 0 and np.abs(whole["force"]).max() > 0
    for what, ids in (("65 scattered clumps", scattered), ("the box", [nC]), ("every owner", list(range(nO)))):
        want = filtered(whole, ids, nO)
        print(f"after {moved} clumps migrated, {what}: {len(want['idA'])} of {len(whole['idA'])} rows")
        same(m.owner_contacts(ids, records=True), want, f"after {moved} clumps migrated, {what}")
    m.close()


def _argtypes(m):
    m.lib.deme_multi_query_owner_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 10 + [C.c_size_t, C.POINTER(C.c_size_t)]


def _raw_query(m, ids, records, cap, fill=0xAB):
    ids = np.ascontiguousarray(ids, np.uint32)
    bufs = [np.full(max(cap, 4), fill, dt) for dt in (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint8)]
    bufs += [np.full((max(cap, 4), 3), np.float32(7.5), np.float32) for _ in range(4)]
    n = C.c_size_t(12345)
    _argtypes(m)
    rc = m.lib.deme_multi_query_owner_contacts(m.h, ids.ctypes.data, ids.size, int(records), *[x.ctypes.data for x in bufs], cap, C.byref(n))
    untouched = all((x == fill).all() for x in bufs[:6]) and all((x == np.float32(7.5)).all() for x in bufs[6:])
    return rc, int(n.value), untouched, m.lib.deme_multi_last_error(m.h).decode()


@pytest.mark.gpu
def test_multi_owner_query_refusals(pkg, run):
    m, sc, whole = run["m"], run["sc"], run["whole"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    rc, n, untouched, msg = _raw_query(m, [nC // 2, nO], True, 8192)
    assert rc == 1 and n == 12345 and untouched and "out of range" in msg and str(nO) in msg
    with pytest.raises(pkg.abi.DemeError, match="out of range"):
        m.owner_contacts([nO + 7])
    # a buffer that is one row short: the count comes back, no row does
    want = len(filtered(whole, [nC], nO)["idA"])
    rc, n, untouched, msg = _raw_query(m, [nC], True, want - 1)
    assert rc == 1 and n == want and untouched and str(want) in msg
    rc, n, untouched, _ = _raw_query(m, [nC], True, want)
    assert rc == 0 and n == want and not untouched
    # records while recording is off on one slab: the message of deme_multi_download_contact_records
    p, sc2 = bed_scene(pkg)
    off = built(pkg, p, sc2, run["n_slabs"])
    off.slab_ctx(run["n_slabs"] - 1).set_record_contacts(False)
    off.step(STEPS)
    off.sync()
    with pytest.raises(pkg.abi.DemeError) as whole_call:
        off.contact_records()
    want_msg = off.lib.deme_multi_last_error(off.h).decode()
    assert "recording is off" in want_msg and want_msg in str(whole_call.value)
    rc, n, untouched, msg = _raw_query(off, [nC], True, 8192)
    assert rc == 1 and n == 12345 and untouched and msg == want_msg
    assert len(off.owner_contacts([nC])["idA"]) == want  # without records it answers
    off.close()
