"""deme_multi_inspect_contacts / deme_multi_inspect_contact_counts (Multi.inspect_contacts, .inspect_contact_counts) on 2 and 3
slabs of one device, exact mode, the bed of tests/test_owner_contacts_multi.py after 60 steps.

The model is the sum over slabs of tests/_contact_sums64.py: applied to each slab context's own downloads (its list, its records,
its owner state) with the slab scene's owner tables, restricted to sides whose owner is an own clump of the slab (the first nOwn
owners: Multi.slab_counts), added in slab order in fp64 and scattered to global ids with the slab's owner book.  No clump changes
slabs in this run (no migration is set), so the books are those of the library's plan (decompose_lib, as the other tests of the
merged list take them).  The tensor is held to the bound derived in tests/test_contact_inspect.py."""
import ctypes as C

import numpy as np
import pytest

from tests._contact_sums64 import contact_sums
from tests.test_contact_inspect import REL, THR, centres, no_force_near
from tests.test_decomp import _sheared_bed
from tests.test_owner_contacts_multi import HALO, STEPS, bed_scene, built

pytestmark = pytest.mark.gpu
RECORDS = ("force", "torqueOnly", "cpA", "cpB")


def _table(sc, name, n):
    ptr = getattr(sc, name)
    if not n or not ptr:
        return np.zeros(0, np.uint32)
    return np.ctypeslib.as_array(C.cast(C.c_void_p(ptr), C.POINTER(C.c_uint32)), shape=(int(n),)).copy()


def slab_model(pkg, m, p, sc, n_slabs, in_region, thr):
    """in_region: bool per GLOBAL owner.  Returns the model's dict with counts by global id, and the number of own clumps in the
    region summed over the slabs."""
    plan, parts = pkg.decomp.decompose_lib(p, sc, n_slabs, HALO, axis=0, snap=True, spatial_order=True)
    nOG = int(sc.nOwners)
    total = {"virial": np.zeros((3, 3)), "abs_sum": np.zeros((3, 3)), "sides": 0, "counts": np.zeros(nOG, np.uint32)}
    clumps, rows = 0, 0
    for s, pt in enumerate(parts):
        ctx, ssc = m.slab_ctx(s), pt["scene"]
        n_own = m.slab_counts(s)[0][0]
        assert n_own == pt["n_own"] and int(ssc.nOwners) == len(pt["owner_global"])
        a, b, t, _ = ctx.contacts()
        whole = {"idA": a, "idB": b, "type": t, **dict(zip(RECORDS, ctx.contact_records()))}
        tables = (_table(ssc, "ownerClumpBody", ssc.nSpheres), _table(ssc, "ownerMesh", ssc.nTri), _table(ssc, "objOwner", ssc.nAnal))
        gid = pt["owner_global"]
        mask = (np.arange(int(ssc.nOwners)) < n_own) & in_region[gid]
        one = contact_sums(whole, tables, ctx.download_state(), mask, thr)
        total["virial"] += one["virial"]
        total["abs_sum"] += one["abs_sum"]
        total["sides"] += one["sides"]
        np.add.at(total["counts"], gid, one["counts"])
        clumps += int(mask.sum())
        rows += len(a)
    plan.close()
    return total, clumps, rows


@pytest.fixture(scope="module", params=[3, 2])
def run(pkg, request):
    p, sc = bed_scene(pkg)
    m = built(pkg, p, sc, request.param)
    m.step(STEPS)
    m.sync()
    yield {"m": m, "p": p, "sc": sc, "n_slabs": request.param}
    m.close()


@pytest.fixture(scope="module")
def single(pkg):
    """the same bed undivided, exact mode: its integers are what the slabs must add up to"""
    from tests.test_owner_contacts import _owner_tables, _stepped, _whole_list
    p, sc = bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, "exact", steps=STEPS)
    whole = _whole_list(ctx, sc)
    assert no_force_near(whole, THR)
    out = {"sums": ctx.inspect_contacts(-1, THR), "counts": ctx.inspect_contact_counts(-1, THR), "X": centres(pkg, p, ctx.download_state())}
    ctx.close()
    return out


def test_slabs_add_up_to_the_model_and_to_the_undivided_run(pkg, run, single):
    m, p, sc, n_slabs = run["m"], run["p"], run["sc"], run["n_slabs"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    X = centres(pkg, p, m.download_state())
    z = np.sort(X[:nC - 1, 2].astype(np.float64))
    third = z[len(z) // 3: 2 * len(z) // 3 + 1]
    k = int(np.argmax(np.diff(third)))
    gap, cut = float(third[k + 1] - third[k]), float(0.5 * (third[k] + third[k + 1]))
    assert gap > 1e-5 * (z[-1] - z[0]), gap
    clump = np.arange(nO) < nC
    cases = {"everywhere": (None, clump), "blank": ("  ", clump), "the lower half": (f"return Z < {cut!r};", clump & (X[:, 2].astype(np.float64) < cut)),
             "an empty region": ("return Z > 1.0e30f;", np.zeros(nO, bool))}
    for what, (code, in_region) in cases.items():
        want, clumps, rows = slab_model(pkg, m, p, sc, n_slabs, in_region, THR)
        got = m.inspect_contacts(code, THR)
        counts = m.inspect_contact_counts(code, THR)
        err = np.abs(got["virial"] - want["virial"])
        print(f"{n_slabs} slabs, {what}: {rows} rows on the slabs, sides {got['sides']}, clumps {got['clumps']}, max |virial - model| {err.max():.3e}, "
              f"max abs_sum {want['abs_sum'].max():.3e}")
        assert rows < 2e5
        assert got["sides"] == want["sides"] and np.array_equal(counts, want["counts"]) and int(counts.sum()) == got["sides"], what
        assert (err <= REL * want["abs_sum"]).all(), (what, err)
        assert got["clumps"] == clumps == int(in_region.sum()), what  # every clump in the region once: no ghost is counted
        assert (counts[~in_region] == 0).all()
        if what in ("everywhere", "blank"):
            assert want["abs_sum"].max() > 0 and got["virial"][2, 2] < 0
            # the integers of the undivided run (no row of it is near the threshold: the fixture asserts it)
            assert got["sides"] == single["sums"]["sides"] and got["clumps"] == single["sums"]["clumps"] == nC
            assert np.array_equal(counts, single["counts"])
        if what == "the lower half":
            assert 0 < got["sides"] < single["sums"]["sides"]
    a, b = m.inspect_contacts(None, THR), m.inspect_contacts(None, THR)
    assert a["virial"].tobytes() == b["virial"].tobytes()


def test_bytes_and_refusals(pkg, run):
    m, sc, n_slabs = run["m"], run["sc"], run["n_slabs"]
    nO = int(sc.nOwners)
    before = m.query_host_bytes()
    m.inspect_contacts(None, THR)
    assert m.query_host_bytes() - before == 88 * n_slabs
    m.inspect_contact_counts(None, THR)
    assert m.query_host_bytes() - before == 88 * n_slabs + 4 * nO * n_slabs
    lib = m.lib
    out = pkg.abi.DemeContactSums()
    out.sides = 123
    for thr in (-1.0, float("nan")):
        assert lib.deme_multi_inspect_contacts(m.h, None, thr, C.byref(out)) == 1 and out.sides == 123
        assert "threshold" in lib.deme_multi_last_error(m.h).decode()
    assert lib.deme_multi_inspect_contacts(m.h, None, THR, None) == 1
    buf = np.full(nO, 0xABABABAB, np.uint32)
    assert lib.deme_multi_inspect_contact_counts(m.h, None, THR, buf.ctypes.data, nO - 1) == 1 and (buf == 0xABABABAB).all()
    assert str(nO) in lib.deme_multi_last_error(m.h).decode()
    with pytest.raises(pkg.abi.DemeError):
        m.inspect_contacts("return 1 > 0;", THR)  # no region: it does not look at X, Y or Z
    # recording off on one slab: the message of deme_multi_download_contact_records
    p, sc2 = bed_scene(pkg)
    off = built(pkg, p, sc2, n_slabs)
    off.slab_ctx(n_slabs - 1).set_record_contacts(False)
    off.step(STEPS)
    off.sync()
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    want_msg = lib.deme_multi_last_error(off.h).decode()
    assert "recording is off" in want_msg
    assert lib.deme_multi_inspect_contacts(off.h, None, THR, C.byref(out)) == 1 and out.sides == 123
    assert lib.deme_multi_last_error(off.h).decode() == want_msg
    assert lib.deme_multi_inspect_contact_counts(off.h, None, THR, buf.ctypes.data, nO) == 1 and (buf == 0xABABABAB).all()
    assert lib.deme_multi_last_error(off.h).decode() == want_msg
    off.close()


def test_refused_on_the_step_after_a_migration(pkg):
    """the sheared bed of tests/test_owner_contacts_multi.py: directly after a migrating step the slabs' lists are seeds, and the
    inspectors are refused with the words of the records call; one step later they answer"""
    b, p, sc, x = _sheared_bed(pkg, 20_000, 6)
    nC = int(sc.nOwnerClumps)
    m = built(pkg, p, sc, 3, halo=0.035, migration=50)
    m.step(150)
    m.sync()
    with pytest.raises(pkg.abi.DemeError) as whole_call:
        m.contact_records()
    want_msg = m.lib.deme_multi_last_error(m.h).decode()
    assert "seed" in want_msg and want_msg in str(whole_call.value)
    for call in (m.inspect_contacts, m.inspect_contact_counts):
        with pytest.raises(pkg.abi.DemeError) as refused:
            call(None, THR)
        assert m.lib.deme_multi_last_error(m.h).decode() == want_msg and want_msg in str(refused.value)
    m.step(1)
    m.sync()
    got = m.inspect_contacts(None, THR)
    counts = m.inspect_contact_counts(None, THR)
    assert got["clumps"] == nC and got["sides"] == int(counts.sum()) > 0
    m.close()
