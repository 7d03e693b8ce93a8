"""deme_multi_inspect_fields (Multi.inspect_fields) on 2 and 3 slabs of one device, exact mode, the bed of
tests/test_owner_contacts_multi.py after 60 steps, and the sheared bed of tests/test_contact_inspect_multi.py for the step after a
migration.

The model is the sum over slabs of tests/_fields64.py: applied to each slab context's own downloads (its owner state, its list, its
records) with the slab scene's tables, restricted to the slab's own clumps (its first nOwn owners), added in slab order in fp64.
The doubles are held to the bound derived in tests/test_fields.py (the slabs' sums add once more per slab: n stays below 1e5 per
cell); the integers must equal those of the undivided run."""
import ctypes as C

import numpy as np
import pytest

from tests._fields64 import fields, positions
from tests.test_decomp import _sheared_bed
from tests.test_fields import BYTES, CONTACT_COLUMNS, OWNER_COLUMNS, REL, THR, _raw_call
from tests.test_owner_contacts_multi import HALO, STEPS, bed_scene, built

pytestmark = pytest.mark.gpu
RECORDS = ("force", "torqueOnly", "cpA", "cpB")
ALL = OWNER_COLUMNS + CONTACT_COLUMNS


def _table(sc, name, n, dtype=np.uint32):
    ptr = getattr(sc, name)
    if not n or not ptr:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(C.cast(C.c_void_p(ptr), C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(int(n),)).copy()


def _volumes(n_props):
    return (1e-7 * (1.0 + np.arange(int(n_props)))).astype(np.float32)


def slab_model(pkg, m, p, sc, n_slabs, grid, thr, contacts=True):
    plan, parts = pkg.decomp.decompose_lib(p, sc, n_slabs, HALO, axis=0, snap=True, spatial_order=True)
    total, rows = None, 0
    for s, pt in enumerate(parts):
        ctx, ssc = m.slab_ctx(s), pt["scene"]
        n_own = m.slab_counts(s)[0][0]
        assert n_own == pt["n_own"] and int(ssc.nOwners) == len(pt["owner_global"])
        state = ctx.download_state()
        whole = None
        if contacts:
            a, b, t, _ = ctx.contacts()
            whole = {"idA": a, "idB": b, "type": t, **dict(zip(RECORDS, ctx.contact_records()))}
            rows += len(a)
        tables = (_table(ssc, "ownerClumpBody", ssc.nSpheres), _table(ssc, "ownerMesh", ssc.nTri), _table(ssc, "objOwner", ssc.nAnal))
        off = _table(ssc, "inertiaPropOffsets", ssc.nOwners, np.uint16).astype(np.int64)
        mass = _table(ssc, "MassProperties", ssc.nMassProps, np.float32)[off]
        volume = _volumes(ssc.nMassProps)[off]
        own = np.arange(int(ssc.nOwners)) < n_own
        one = fields(positions(pkg.model.decode_positions, p, state), state, own, mass, volume, *grid, whole, tables, thr)
        one.pop("cell_of"), one.pop("side_cells", None)
        total = one if total is None else {k: total[k] + one[k] for k in total}
    plan.close()
    return total, rows


def grid_of(pkg, p, state, n_clumps, shape=(5, 3, 2)):
    X = positions(pkg.model.decode_positions, p, state)[:n_clumps]
    lo, hi = X.min(0) - 1.2345e-4, X.max(0) + 2.3456e-4
    u = (X - lo) / ((hi - lo) / shape)
    assert np.abs(u - np.round(u)).min() > 1e-9
    return lo, (hi - lo) / shape, shape


@pytest.fixture(scope="module", params=[3, 2])
def run(pkg, request):
    p, sc = bed_scene(pkg)
    m = built(pkg, p, sc, request.param)
    for s in range(request.param):
        m.slab_ctx(s).upload_volumes(_volumes(sc.nMassProps))
    m.step(STEPS)
    m.sync()
    yield {"m": m, "p": p, "sc": sc, "n_slabs": request.param, "grid": grid_of(pkg, p, m.download_state(), int(sc.nOwnerClumps))}
    m.close()


@pytest.fixture(scope="module")
def single(pkg):
    """the same bed undivided, exact mode: its integers are what the slabs must add up to"""
    from tests.test_owner_contacts import _stepped
    p, sc = bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, "exact", steps=STEPS)
    ctx.upload_volumes(_volumes(sc.nMassProps))
    f = np.sqrt((ctx.contact_records()[0].astype(np.float64) ** 2).sum(1))
    assert not ((f > THR / 2) & (f < 2 * THR)).any()  # no row a rounding could move across the threshold
    yield ctx
    ctx.close()


def test_slabs_add_up_to_the_model_and_to_the_undivided_run(pkg, run, single):
    m, p, sc, n_slabs, grid = run["m"], run["p"], run["sc"], run["n_slabs"], run["grid"]
    nC = int(sc.nOwnerClumps)
    undivided = single.inspect_fields(*grid, force_threshold=THR)
    want, rows = slab_model(pkg, m, p, sc, n_slabs, grid, THR)
    got = m.inspect_fields(*grid, force_threshold=THR)
    assert tuple(got) == ALL
    for k in ALL:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if got[k].dtype == np.uint32:
            assert np.array_equal(got[k], want[k]) and np.array_equal(got[k], undivided[k]), k
            continue
        err = np.abs(got[k] - want[k])
        print(f"{n_slabs} slabs, {rows} rows on the slabs, {k}: max |got - model| {err.max():.3e}, max abs_sum {want['abs_' + k].max():.3e}")
        assert (err <= REL * want["abs_" + k]).all(), (k, float(err.max()))
    assert want["terms_owner"].max() + n_slabs < 1e5 and want["terms_side"].max() + n_slabs < 1e5
    assert int(got["clumps"].sum()) == nC and int(got["sides"].sum()) > 0  # every clump once: no ghost is counted
    assert (got["clumps"] > 1).any() and np.abs(got["virial"]).max() > 0 and got["virial"][:, 8].min() < 0
    again = m.inspect_fields(*grid, force_threshold=THR)
    assert all(again[k].tobytes() == got[k].tobytes() for k in ALL)


def test_bytes_and_refusals(pkg, run):
    m, sc, n_slabs, grid = run["m"], run["sc"], run["n_slabs"], run["grid"]
    n_cells = int(np.prod(grid[2]))
    for columns in (("clumps",), ("virial",), ("mass", "momentum", "sides"), ALL):
        before = m.query_host_bytes()
        m.inspect_fields(*grid, columns=columns, force_threshold=THR)
        assert m.query_host_bytes() - before == n_slabs * n_cells * sum(BYTES[k] for k in columns), columns
    lib = m.lib
    base = {"origin": (0.0, 0.0, 0.0), "cell": (1.0, 1.0, 1.0), "n": (2, 2, 2), "thr": THR, "ask": ALL}

    def call(mm, **over):
        return _raw_call(pkg, lib.deme_multi_inspect_fields, mm.h, lib.deme_multi_last_error, **{**base, **over})

    rc, untouched, _ = call(m)
    assert rc == 0 and not untouched
    for what, word, over in (("a null grid", "grid", {"null_grid": True}), ("null columns", "columns", {"null_columns": True}),
                             ("an origin that is not finite", "finite", {"origin": (0.0, float("inf"), 0.0)}),
                             ("a negative edge", "> 0", {"cell": (1.0, -1.0, 1.0)}), ("no cells", "cells", {"n": (2, 2, 0)}),
                             ("too many cells", "at most", {"n": (2048, 2048, 1)}), ("every column null", "null output", {"ask": ()}),
                             ("a negative threshold", "threshold", {"thr": -1.0}), ("a NaN threshold", "threshold", {"thr": float("nan")})):
        rc, untouched, msg = call(m, **over)
        assert rc == 1 and untouched and word in msg and "deme_multi_inspect_fields" in msg, (what, msg)
    # no volumes on the slabs, and recording off on one slab: the owner columns answer, the others are refused
    p, sc2 = bed_scene(pkg)
    off = built(pkg, p, sc2, n_slabs)
    off.slab_ctx(n_slabs - 1).set_record_contacts(False)
    off.step(STEPS)
    off.sync()
    rc, untouched, msg = call(off)
    assert rc == 1 and untouched and "deme_upload_volumes" in msg
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    want_msg = lib.deme_multi_last_error(off.h).decode()
    assert "recording is off" in want_msg
    for ask in (("clumps", "sides"), ("virial",)):
        rc, untouched, msg = call(off, ask=ask)
        assert rc == 1 and untouched and msg == want_msg
    rc, untouched, _ = call(off, ask=("clumps", "mass", "momentum", "kinetic"))
    assert rc == 0 and not untouched
    off.close()


def test_a_contact_column_is_refused_on_the_step_after_a_migration(pkg):
    """the sheared bed of tests/test_contact_inspect_multi.py: directly after a migrating step the slabs' lists are seeds; a contact
    column is refused with the words of the records call, the owner columns answer; one step later all do"""
    b, p, sc, x = _sheared_bed(pkg, 20_000, 6)
    nC = int(sc.nOwnerClumps)
    m = built(pkg, p, sc, 3, halo=0.035, migration=50)
    m.step(150)
    m.sync()
    grid = grid_of(pkg, p, m.download_state(), nC, (6, 4, 3))
    with pytest.raises(pkg.abi.DemeError) as whole_call:
        m.contact_records()
    want_msg = m.lib.deme_multi_last_error(m.h).decode()
    assert "seed" in want_msg and want_msg in str(whole_call.value)
    for columns in (("sides",), ("clumps", "virial")):
        with pytest.raises(pkg.abi.DemeError) as refused:
            m.inspect_fields(*grid, columns=columns, force_threshold=THR)
        assert m.lib.deme_multi_last_error(m.h).decode() == want_msg and want_msg in str(refused.value)
    owner = m.inspect_fields(*grid, columns=("clumps", "mass", "momentum", "kinetic"))
    assert int(owner["clumps"].sum()) == nC and owner["mass"].min() >= 0  # every clump once, wherever it migrated to
    m.step(1)
    m.sync()
    grid = grid_of(pkg, p, m.download_state(), nC, (6, 4, 3))
    got = m.inspect_fields(*grid, columns=("clumps", "mass", "momentum", "kinetic", "sides", "virial"), force_threshold=THR)
    assert int(got["clumps"].sum()) == nC and int(got["sides"].sum()) == m.inspect_contacts(None, THR)["sides"] > 0
    m.close()
