"""deme_multi_tri_wear_* (Multi.tri_wear_*) on 2 and 3 slabs of one device, exact mode: the bed, the plate and the slabs of
tests/test_tri_loads_multi.py (1500 clumps over a fixed plate of 7 x 7 x 2 triangles, triangles with rows from both sides of a cut).

The model is the sum over slabs of tests/_tri_wear64.py applied to each slab context's own downloads -- its list, its records, its
owners' state -- with the slab scene's tables and the slab's ghost copies flagged, added in slab order; no clump changes slabs there
(no migration is set), so the tables are those of the library's plan.  The slabs' sum is held to it within REL * abs_scale, the bound
derived in tests/test_tri_wear.py; rows are held to equality with the model and with the undivided run.

Against the undivided run REL cannot be the bound: a decomposed run follows the undivided one within a tolerance, not bit for bit.
tests/test_tri_loads_multi.py derives PER_ROW, the most one listed row's recorded force differs between the two runs, from the bounds
tests/test_decomp.py holds positions and velocities to.  A sample of weight w multiplies a row's force by w (lanes 0 to 3: |d(w g)| <=
w PER_ROW, and | |Fn| - |Fn'| | <= |g - g'|) and lanes 4 and 5 by the sliding speed as well, which is at most the largest |u| of the
scene, U: | |Fn| |ut| - |Fn'| |ut'| | <= PER_ROW U to first order in the force.  (The speed differs between the runs too, by DV of
that file; U is taken from the float64 model of the undivided run's downloads and widened by DV, never from the accumulators.)  A
triangle's lane may differ by that times its listed rows, the total by that times all listed sphere-mesh rows."""
import ctypes as C

import numpy as np
import pytest

from tests._tri_wear64 import REL, tri_wear
from tests.test_contact_inspect_multi import _table
from tests.test_fields_multi import _table as _typed_table
from tests.test_owner_contacts import _stepped
from tests.test_owner_contacts_multi import HALO, built
from tests.test_tri_loads_multi import DV, PER_ROW, STEPS, bed_scene
from tests.test_tri_wear import LANES, THR, lanes_of, model_of

pytestmark = pytest.mark.gpu
W = 0.25
COLS = LANES + ("rows",)


@pytest.fixture(scope="module", params=[3, 2])
def run(pkg, request):
    p, sc = bed_scene(pkg)
    m = built(pkg, p, sc, request.param)
    m.step(STEPS)
    m.sync()
    m.tri_wear_enable()
    yield {"m": m, "p": p, "sc": sc, "n_slabs": request.param}
    m.close()


@pytest.fixture(scope="module")
def single(pkg):
    """the same bed undivided, exact mode: the float64 model of its downloads (rows, lanes, listed rows per triangle, U)"""
    p, sc = bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, "exact", steps=STEPS)
    out = {thr: model_of(ctx, sc, thr, W) for thr in (THR, 0.0)}
    ctx.close()
    return out


def slab_model(pkg, m, p, sc, n_slabs, thr, w):
    plan, parts = pkg.decomp.decompose_lib(p, sc, n_slabs, HALO, axis=0, snap=True, spatial_order=True)
    nT = int(sc.nTri)
    total = {"lanes": np.zeros((nT, 6)), "abs_scale": np.zeros((nT, 6)), "rows": np.zeros(nT, np.uint64)}
    per_slab = []
    for s, pt in enumerate(parts):
        ctx, ssc = m.slab_ctx(s), pt["scene"]
        own, below, above = m.slab_counts(s)[0][:3]
        assert own == pt["n_own"] and int(ssc.nTri) == nT
        ghost = np.zeros(int(ssc.nOwners), bool)
        ghost[own:own + below + above] = True
        a, b, t, _ = ctx.contacts()
        rec = ctx.contact_records()
        whole = {"idA": a, "idB": b, "type": t, "ownerA": _table(ssc, "ownerClumpBody", ssc.nSpheres)[a], "force": rec[0], "cpA": rec[2],
                 "cpB": rec[3]}
        nodes = tuple(_typed_table(ssc, f"triNode{k}", 3 * nT, np.float32).reshape(-1, 3) for k in (1, 2, 3))
        one = tri_wear(whole, ctx.download_state(), nodes, _table(ssc, "ownerMesh", nT), ghost, nT, thr, w)
        for k in total:
            total[k] = total[k] + one[k]
        per_slab.append(one["rows"])
    plan.close()
    return total, per_slab


def test_slabs_add_up_to_the_model_and_to_the_undivided_run(pkg, run, single):
    m, p, sc, n_slabs = run["m"], run["p"], run["sc"], run["n_slabs"]
    listed = single[0.0]["rows"].astype(np.float64)  # listed sphere-mesh rows per triangle (threshold 0: every one counts)
    for thr in (THR, 0.0):
        want, per_slab = slab_model(pkg, m, p, sc, n_slabs, thr, W)
        m.tri_wear_reset()
        assert m.tri_wear_sample(thr, W) is True
        got = m.tri_wear_read()
        lanes = lanes_of(got)
        err = np.abs(lanes - want["lanes"])
        print(f"{n_slabs} slabs, thr {thr:g}: counted rows per slab {[int(c.sum()) for c in per_slab]}, worst |got - model| / abs_scale per lane "
              f"{np.array2string((err / np.maximum(want['abs_scale'], 1e-300)).max(0), precision=2)} (bound {REL:g})")
        assert got["rows"].dtype == np.uint64 and np.array_equal(got["rows"], want["rows"]) and got["sampledTime"] == W
        assert (err <= REL * want["abs_scale"]).all()
        if thr == 0.0:  # the cut leaves sphere-mesh rows on at least two slabs, and some triangle gets rows from two
            assert sum(1 for c in per_slab if c.sum() > 0) >= 2
            assert (sum((c > 0).astype(np.int64) for c in per_slab) >= 2).any()
        # the undivided run: every sphere-triangle pair once
        one = single[thr]
        assert np.array_equal(got["rows"], one["rows"]) and got["rows"].sum() >= (50 if thr == 0.0 else 5)
        U = single[0.0]["u_max"] + DV
        per_row = W * PER_ROW * np.array([1, 1, 1, 1, U, U])
        dev = np.abs(lanes - one["lanes"])
        dev_total = np.abs(lanes.sum(0) - one["lanes"].sum(0))
        print(f"{n_slabs} slabs, thr {thr:g}: against the undivided run worst |lane - its| per lane {np.array2string(dev.max(0), precision=3)}, "
              f"worst ratio to the bound {np.array2string((dev / np.maximum(per_row * listed[:, None], 1e-300)).max(0), precision=2)}, totals "
              f"{np.array2string(dev_total, precision=3)} of {np.array2string(np.abs(one['lanes'].sum(0)), precision=3)}, U {U:.3f} m/s, "
              f"w PER_ROW {W * PER_ROW:.3e} N s")
        assert (dev <= per_row * listed[:, None]).all()
        assert (dev_total <= per_row * listed.sum()).all() and np.abs(one["lanes"].sum(0)).min() > 0
        assert (got["slidingWork"] != 0).any() and (got["shearWork"] != 0).any()
    # a second sample adds onto every slab's sums; a sub-range is the slice
    before = m.tri_wear_read()
    assert m.tri_wear_sample(THR, 2 * W)
    after = m.tri_wear_read()
    assert after["sampledTime"] == 3 * W and np.array_equal(after["rows"], before["rows"] + single[THR]["rows"])
    part = m.tri_wear_read(first=37, count=50)
    assert all(part[k].tobytes() == after[k][37:87].tobytes() for k in COLS) and part["rows"].shape == (50,)
    again = m.tri_wear_read()
    assert all(again[k].tobytes() == after[k].tobytes() for k in COLS)


def test_bytes_and_refusals(pkg, run):
    m, sc, n_slabs, lib = run["m"], run["sc"], run["n_slabs"], run["m"].lib
    nT = int(sc.nTri)
    assert nT == 98
    before = m.query_host_bytes()
    m.tri_wear_enable()
    m.tri_wear_reset()
    assert m.tri_wear_sample(THR, W)
    assert m.query_host_bytes() == before
    m.tri_wear_read()
    assert m.query_host_bytes() - before == 56 * nT * n_slabs
    m.tri_wear_read(first=37, count=50, columns=("slidingWork",))
    assert m.query_host_bytes() - before == (56 * nT + 8 * 50) * n_slabs
    t = C.c_double(-1.0)
    assert lib.deme_multi_tri_wear_read(m.h, 5, 0, None, None, None, None, None, C.byref(t)) == 0 and t.value == W
    assert m.query_host_bytes() - before == (56 * nT + 8 * 50) * n_slabs
    kept = m.tri_wear_read()
    f = np.full((50, 3), 7.5)
    flag = C.c_int(77)
    for what, thr, w in (("threshold", -1.0, W), ("threshold", float("nan"), -1.0), ("weight", THR, -1.0), ("weight", THR, float("inf"))):
        rc = lib.deme_multi_tri_wear_sample(m.h, thr, w, C.byref(flag))
        msg = lib.deme_multi_last_error(m.h).decode()
        assert rc == 1 and flag.value == 77 and what in msg and "deme_multi_tri_wear_sample" in msg, (what, msg)
    for what, first, count, pf in (("triangles", 49, 50, f), ("null", 0, 50, None)):
        rc = lib.deme_multi_tri_wear_read(m.h, first, count, None if pf is None else pf.ctypes.data, None, None, None, None, None)
        msg = lib.deme_multi_last_error(m.h).decode()
        assert rc == 1 and (f == 7.5).all() and what in msg and "deme_multi_tri_wear_read" in msg, (what, msg)
    now = m.tri_wear_read()
    assert now["sampledTime"] == kept["sampledTime"] and all(now[k].tobytes() == kept[k].tobytes() for k in COLS)
    # not enabled, and recording off on one slab
    p, sc2 = bed_scene(pkg)
    off = built(pkg, p, sc2, n_slabs)
    off.slab_ctx(n_slabs - 1).set_record_contacts(False)
    off.step(STEPS)
    off.sync()
    for rc in (lib.deme_multi_tri_wear_sample(off.h, THR, W, None), lib.deme_multi_tri_wear_read(off.h, 0, 50, f.ctypes.data, None, None, None, None, None),
               lib.deme_multi_tri_wear_reset(off.h)):
        assert rc == 1
    assert "not enabled" in lib.deme_multi_last_error(off.h).decode() and (f == 7.5).all()
    off.tri_wear_enable()
    assert lib.deme_multi_tri_wear_sample(off.h, THR, W, C.byref(flag)) == 1 and flag.value == 77
    msg = lib.deme_multi_last_error(off.h).decode()
    assert "recording is off" in msg and "deme_multi_tri_wear_sample" in msg
    got = off.tri_wear_read()
    assert got["sampledTime"] == 0.0 and not got["rows"].any()  # no slab added anything
    off.close()


def test_a_sample_on_the_step_after_a_migration_adds_nothing(pkg):
    """The bed with neighbouring clumps sheared along x (2 and 1 m/s), migrating every 100 steps (a migrating step re-assembles and re-seeds every slab whether or not a clump crossed a cut): directly after a migrating step every slab's list
    is a seed, so the sample reports sampled == 0 and no accumulator of any slab has moved; one step later it samples."""
    p, sc = bed_scene(pkg)
    arr = {k: np.array(v, copy=True) for k, v in sc._keep.items()}
    counts = {k: int(getattr(sc, k)) for k in ("nOwners", "nOwnerClumps", "nSpheres", "nAnal", "nTri", "nMat", "nComp", "nMassProps")}
    nc = counts["nOwnerClumps"]
    arr["vX"] = np.array(arr["vX"], np.float32)
    arr["vX"][:nc] = np.where(np.arange(nc) % 2 == 0, 2.0, 1.0).astype(np.float32)
    sheared = pkg.abi.make_scene_struct(arr, counts)
    m = built(pkg, p, sheared, 3, migration=100)
    m.tri_wear_enable()
    m.step(199)
    assert m.tri_wear_sample(0.0, 0.5) is True
    before = m.tri_wear_read()
    slabs_before = [m.slab_ctx(s).tri_wear_read(0, counts["nTri"]) for s in range(3)]
    assert before["rows"].sum() > 0 and before["sampledTime"] == 0.5
    m.step(1)  # step 200 migrates
    m.sync()
    with pytest.raises(pkg.abi.DemeError):
        m.contact_records()
    assert "seed" in m.lib.deme_multi_last_error(m.h).decode()
    assert m.tri_wear_sample(0.0, 3.0) is False
    assert m.lib.deme_multi_tri_wear_sample(m.h, 0.0, 3.0, None) == 0
    after = m.tri_wear_read()
    assert after["sampledTime"] == 0.5 and all(after[k].tobytes() == before[k].tobytes() for k in COLS)
    for s in range(3):
        now = m.slab_ctx(s).tri_wear_read(0, counts["nTri"])
        assert now["sampledTime"] == slabs_before[s]["sampledTime"] and all(now[k].tobytes() == slabs_before[s][k].tobytes() for k in COLS), s
    m.step(1)
    assert m.tri_wear_sample(0.0, 3.0) is True
    after = m.tri_wear_read()
    assert after["sampledTime"] == 3.5 and after["rows"].sum() > before["rows"].sum()
    print(f"{m.counts()[1]} clumps migrated; rows before {int(before['rows'].sum())}, after {int(after['rows'].sum())}")
    m.close()
