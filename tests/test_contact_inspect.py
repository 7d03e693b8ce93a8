"""deme_inspect_contacts / deme_inspect_contact_counts (Context.inspect_contacts, .inspect_contact_counts): the virial sum and the
counted sides of the current contact list, summed on the device, against tests/_contact_sums64.py applied to the whole-list
downloads, the scene's owner tables and the downloaded owner state.

The bed is that of tests/test_owner_contacts.py: 300 three-sphere clumps lowered onto the floor of their box, the last clump left
where the lattice put it as the owner without contacts; 573 rows after the first step, 64 of them against the box.

Tolerance of the tensor: |virial - model| <= 1e-10 * abs_sum per component, abs_sum = sum |r_i| |f_j| over the counted sides.  It is
derived, not measured: both sides do the same fp64 arithmetic on the same fp32 inputs; a term carries a few dozen roundings of
1.1e-16, and a sum of n < 2e5 terms adds at most n * 1.1e-16 ~ 2e-11 of abs_sum.  The integers are compared for equality."""
import ctypes as C

import numpy as np
import pytest

from tests._contact_sums64 import contact_sums
from tests.test_owner_contacts import _bed_scene, _owner_tables, _stepped, _whole_list

THR = 1e-12  # what the shell passes (DEME_TINY_FLOAT_HOST)
REL = 1e-10
SYMBOLS = ("deme_inspect_contacts", "deme_inspect_contact_counts", "deme_multi_inspect_contacts", "deme_multi_inspect_contact_counts")


def test_contact_inspectors_are_exported_and_bound(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in SYMBOLS:
        assert n in names and hasattr(lib, n), n
    for cls in (pkg.Context, pkg.abi.Multi):
        assert hasattr(cls, "inspect_contacts") and hasattr(cls, "inspect_contact_counts"), cls.__name__
    assert C.sizeof(pkg.abi.DemeContactSums) == 88


def centres(pkg, p, state):
    """owner centres of mass as the region filter sees them: float32 of the decoded position plus the domain's corner"""
    X = pkg.model.decode_positions(state["voxelID"], state["locX"], state["locY"], state["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    return (X + np.array([p.LBFX, p.LBFY, p.LBFZ], np.float64)).astype(np.float32)


def no_force_near(whole, thr):
    """no row's |f| within a factor 2 of the threshold: the rows a rounding could move across it"""
    f = np.sqrt((whole["force"].astype(np.float64) ** 2).sum(1))
    return not ((f > thr / 2) & (f < 2 * thr)).any()


def check(got, counts, want, what):
    err = np.abs(got["virial"] - want["virial"])
    bound = REL * want["abs_sum"]
    print(f"{what}: sides {got['sides']}, clumps {got['clumps']}, max |virial - model| {err.max():.3e}, max abs_sum {want['abs_sum'].max():.3e}, "
          f"worst ratio {(err / np.maximum(want['abs_sum'], 1e-300)).max():.3e}")
    assert got["sides"] == want["sides"], what
    assert counts.dtype == np.uint32 and np.array_equal(counts, want["counts"]), what
    assert int(counts.sum()) == got["sides"], what
    assert (err <= bound).all(), (what, err, bound)


@pytest.fixture(scope="module", params=["fast", "exact"])
def bed(pkg, request):
    p, sc, mid = _bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, request.param)
    state = ctx.download_state()
    yield {"ctx": ctx, "p": p, "sc": sc, "mode": request.param, "whole": _whole_list(ctx, sc), "state": state, "X": centres(pkg, p, state)}
    ctx.close()


def regions(bed):
    """name -> (region string or None, boolean owner mask of the model)"""
    sc, X = bed["sc"], bed["X"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    clump = np.arange(nO) < nC
    # the lower half: a cut in the middle of the largest gap among the central third of the sorted clump centres, so that the
    # region's float comparison cannot fall on a rounding (an fp32 coordinate is good to 1e-7 of the bed's height)
    z = np.sort(X[:nC - 1, 2].astype(np.float64))
    third = z[len(z) // 3: 2 * len(z) // 3 + 1]
    k = int(np.argmax(np.diff(third)))
    gap, cut = float(third[k + 1] - third[k]), float(0.5 * (third[k] + third[k + 1]))
    assert gap > 1e-5 * (z[-1] - z[0]), gap
    # the last clump alone: a ball around its centre of half the distance to its nearest neighbour
    last = [float(v) for v in X[nC - 1]]
    d = float(np.sqrt(((X[:nC - 1].astype(np.float64) - np.array(last)) ** 2).sum(1)).min())
    assert d > 1e-3
    ball = (f"return (X - {last[0]!r}) * (X - {last[0]!r}) + (Y - {last[1]!r}) * (Y - {last[1]!r}) + (Z - {last[2]!r}) * (Z - {last[2]!r}) "
            f"< {(0.5 * d) ** 2!r};")
    only_last = np.zeros(nO, bool)
    only_last[nC - 1] = True
    return {
        "everywhere (-1)": (None, clump),
        "all clumps": ("return Z > -1.0e30f;", clump),
        "the lower half": (f"return Z < {cut!r};", clump & (X[:, 2].astype(np.float64) < cut)),
        "an empty region": ("return Z > 1.0e30f;", np.zeros(nO, bool)),
        "the last clump": (ball, only_last),
    }


@pytest.mark.gpu
def test_bed_list_exercises_what_it_should(bed):
    whole, sc = bed["whole"], bed["sc"]
    n = len(whole["idA"])
    assert n > 256 and n % 64 != 0
    assert (whole["type"] == 1).any() and (whole["type"] == 11).any()
    # the fast mode keeps an order of its own (its per-owner output goes through o2e), the exact mode the caller's
    assert bed["ctx"].engine_order()[0] == (bed["mode"] == "fast")
    assert no_force_near(whole, THR)


@pytest.mark.gpu
def test_sums_and_counts_equal_the_model(bed):
    ctx, sc, whole = bed["ctx"], bed["sc"], bed["whole"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    tables = _owner_tables(sc)
    for what, (code, mask) in regions(bed).items():
        rid = -1 if code is None else ctx.compile_region(code)
        want = contact_sums(whole, tables, bed["state"], mask, THR)
        got = ctx.inspect_contacts(rid, THR)
        counts = ctx.inspect_contact_counts(rid, THR)
        check(got, counts, want, f"{bed['mode']}, {what}")
        assert got["clumps"] == int(mask.sum()), what
        assert (counts[nC:] == 0).all() and len(counts) == nO  # the box's sides are never counted
        if what in ("everywhere (-1)", "all clumps"):
            assert want["abs_sum"].max() > 0 and got["clumps"] == nC
            assert got["virial"][2, 2] < 0  # a bed lying on its floor is in compression
            plane = whole["type"] > 2
            f2 = (whole["force"][plane].astype(np.float64) ** 2).sum(1)
            assert (f2 >= THR * THR).any()  # counted sphere--plane rows: their A sides are in, the plane's never
        if what == "the lower half":
            assert 0 < got["clumps"] < nC - 1 and 0 < got["sides"] < contact_sums(whole, tables, bed["state"], np.arange(nO) < nC, THR)["sides"]
        if what in ("an empty region", "the last clump"):
            assert got["sides"] == 0 and not got["virial"].any() and got["clumps"] == (1 if what == "the last clump" else 0)


@pytest.mark.gpu
def test_a_threshold_above_the_median_force(bed):
    """The decision is exact on both sides -- the squares of fp32 values are exact in fp64 and the three are added in the same
    order -- so the threshold may lie anywhere; it is put between two neighbours of the sorted |f| all the same."""
    ctx, sc, whole = bed["ctx"], bed["sc"], bed["whole"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    f = np.sort(np.sqrt((whole["force"].astype(np.float64) ** 2).sum(1)))
    f = f[f > 0]
    k = int(0.6 * len(f))
    thr = float(np.float32(0.5 * (f[k] + f[k + 1])))
    assert thr > np.median(f) and f[k] < thr < f[k + 1]
    clump = np.arange(nO) < nC
    want = contact_sums(whole, _owner_tables(sc), bed["state"], clump, thr)
    low = contact_sums(whole, _owner_tables(sc), bed["state"], clump, THR)
    got = ctx.inspect_contacts(-1, thr)
    check(got, ctx.inspect_contact_counts(-1, thr), want, f"{bed['mode']}, threshold {thr:.3e}")
    assert 0 < got["sides"] < low["sides"]


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(bed):
    a = bed["ctx"].inspect_contacts(-1, THR)
    b = bed["ctx"].inspect_contacts(-1, THR)
    assert a["virial"].tobytes() == b["virial"].tobytes() and a["virial"].any()


@pytest.mark.gpu
def test_bytes_that_come_to_the_host(bed):
    ctx, nO = bed["ctx"], int(bed["sc"].nOwners)
    before = ctx.query_host_bytes()
    ctx.inspect_contacts(-1, THR)
    assert ctx.query_host_bytes() - before == 88
    ctx.inspect_contact_counts(-1, THR)
    assert ctx.query_host_bytes() - before == 88 + 4 * nO


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_the_inspectors_change_nothing(pkg, mode):
    """a detection every 20 steps: step, ask, step -- the question must not make the second step detect again, and the state and
    the list afterwards are those of a twin context that never asked"""
    p, sc, mid = _bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, mode, steps=1)
    ref = _stepped(pkg, p, sc, mode, steps=2)
    assert ctx.counts().nDetections == 1
    rid = ctx.compile_region("return Z < 0.02;")
    ctx.inspect_contacts(-1, THR), ctx.inspect_contacts(rid, THR), ctx.inspect_contact_counts(rid, THR)
    ctx.step(1)
    ctx.sync()
    assert ctx.counts().nDetections == 1 and ctx.counts().nSteps == 2
    a, r = ctx.download_state(), ref.download_state()
    assert all(np.array_equal(a[k], r[k]) for k in pkg.abi.QUERY_STATE_COLUMNS)
    ctx.inspect_contacts(rid, THR), ctx.inspect_contact_counts(-1, THR)
    la, lr = _whole_list(ctx, sc), _whole_list(ref, sc)
    for k in la:
        assert np.array_equal(la[k].view(np.uint32) if la[k].dtype == np.float32 else la[k],
                              lr[k].view(np.uint32) if lr[k].dtype == np.float32 else lr[k]), k
    for w in range(int(p.nContactWildcards)):
        assert np.array_equal(ctx.wildcard(w).view(np.uint32), ref.wildcard(w).view(np.uint32)), w
    a, r = ctx.download_state(), ref.download_state()
    assert all(np.array_equal(a[k], r[k]) for k in a)
    ctx.close(), ref.close()


@pytest.mark.gpu
def test_refusals(pkg, bed):
    ctx, sc, lib = bed["ctx"], bed["sc"], bed["ctx"].lib
    nO = int(sc.nOwners)

    def sums(c, region, thr, null=False):
        out = pkg.abi.DemeContactSums()
        out.virial[0], out.sides, out.clumps = 7.5, 123, 456
        rc = lib.deme_inspect_contacts(c.h, region, thr, None if null else C.byref(out))
        return rc, (out.virial[0], out.sides, out.clumps) == (7.5, 123, 456), lib.deme_last_error(c.h).decode()

    def counts(c, region, thr, cap, null=False):
        buf = np.full(nO + 4, 0xABABABAB, np.uint32)
        rc = lib.deme_inspect_contact_counts(c.h, region, thr, None if null else buf.ctypes.data, cap)
        return rc, bool((buf == 0xABABABAB).all()), lib.deme_last_error(c.h).decode()

    n_regions = ctx.compile_region("return Z > 0;") + 1
    for what, region, thr in (("negative threshold", -1, -1.0), ("NaN threshold", -1, float("nan")), ("infinite threshold", -1, float("inf")),
                              ("region past the last", n_regions, THR), ("region below -1", -2, THR)):
        rc, untouched, msg = sums(ctx, region, thr)
        assert rc == 1 and untouched and msg, what
        assert ("threshold" in msg) == ("threshold" in what) and ("region" in msg) == ("region" in what), (what, msg)
        rc, untouched, msg = counts(ctx, region, thr, nO)
        assert rc == 1 and untouched, what
    assert sums(ctx, -1, THR, null=True)[0] == 1 and counts(ctx, -1, THR, nO, null=True)[0] == 1
    rc, untouched, msg = counts(ctx, -1, THR, nO - 1)
    assert rc == 1 and untouched and str(nO) in msg
    rc, untouched, _ = counts(ctx, -1, THR, nO)
    assert rc == 0 and not untouched
    with pytest.raises(pkg.abi.DemeError, match="threshold"):
        ctx.inspect_contacts(-1, -1.0)
    # recording off, and a seeded list: the messages of deme_download_contact_records
    p, sc2, mid = _bed_scene(pkg)
    off = _stepped(pkg, p, sc2, bed["mode"], record=False)
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    want_msg = lib.deme_last_error(off.h).decode()
    assert "recording is off" in want_msg
    for rc, untouched, msg in (sums(off, -1, THR), counts(off, -1, THR, nO)):
        assert rc == 1 and untouched and msg == want_msg
    off.set_record_contacts(True)
    a, b, t, _ = off.contacts()
    W = np.stack([off.wildcard(w) for w in range(int(p.nContactWildcards))], 1) if p.nContactWildcards else None
    off.seed_contacts(a, b, t, W)
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    want_msg = lib.deme_last_error(off.h).decode()
    assert "seed" in want_msg
    for rc, untouched, msg in (sums(off, -1, THR), counts(off, -1, THR, nO)):
        assert rc == 1 and untouched and msg == want_msg
    off.step(1)
    off.sync()
    assert off.inspect_contacts(-1, THR)["sides"] > 0  # evaluated again: it answers
    off.close()


@pytest.mark.gpu
def test_more_partials_than_the_second_stage_has_threads(pkg):
    """50 000 clumps of the packed bed of tests/test_owner_contacts_multi.py, at the lattice spacing of the small bed above (its
    clumps overlap from the start, so the list carries forces after a few steps): more than 65 536 rows, so the first stage leaves
    more than 256 partials and threads of the second stage add several before the tree"""
    COUNTS = ("nOwners", "nOwnerClumps", "nSpheres", "nAnal", "nTri", "nMat", "nComp", "nMassProps")
    b = pkg.model.packed_bed(50_000, seed=4, cd_freq=7, spacing_mult=2.4, init_vz=-0.4, aspect=(2.0, 1.0, 0.5))
    b.SetExpandSafetyAdder(0.5)
    p, sc = b.Initialize()
    arr = {k: np.array(v, copy=True) for k, v in sc._keep.items()}
    counts = {k: int(getattr(sc, k)) for k in COUNTS}
    nO, nC = counts["nOwners"], counts["nOwnerClumps"]
    X = pkg.model.decode_positions(arr["voxelID"], arr["locX"], arr["locY"], arr["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    X[:nC - 1, 2] -= (X[:nC, 2].min() + p.LBFZ) - 0.0045
    arr["voxelID"], arr["locX"], arr["locY"], arr["locZ"] = pkg.model.encode_positions(X, p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    sc = pkg.abi.make_scene_struct(arr, counts)
    ctx = _stepped(pkg, p, sc, "exact", steps=5)
    assert ctx.counts().nDetections == 1
    whole = _whole_list(ctx, sc)
    n = len(whole["idA"])
    assert n > 65536 and n < 2e5 and no_force_near(whole, THR)
    state = ctx.download_state()
    clump = np.arange(nO) < nC
    want = contact_sums(whole, _owner_tables(sc), state, clump, THR)
    got = ctx.inspect_contacts(-1, THR)
    check(got, ctx.inspect_contact_counts(-1, THR), want, f"{n} rows")
    assert got["clumps"] == nC and want["abs_sum"].max() > 0 and got["sides"] > 0
    again = ctx.inspect_contacts(-1, THR)
    assert again["virial"].tobytes() == got["virial"].tobytes()
    ctx.close()
