"""deme_multi_inspect_tri_loads (Multi.inspect_tri_loads) on 2 and 3 slabs of one device, exact mode, built as
tests/test_contact_inspect_multi.py builds its slabs: the bed of tests/test_mesh.py (1500 clumps, a detection every 5 steps) on a
fixed plate of 7 x 7 x 2 triangles after 120 steps.  The plate's cells are wider than a few spheres and no cut falls on a line of its
grid, so triangles get rows from the slabs on both sides of a cut (the oracle's list with the plan's ownership: 11 such triangles
with 2 slabs, 22 with 3; with the 20 x 20 plate the middle cut runs along a grid line and there is none).  The run is asked with a
threshold of 0, where every listed sphere-mesh row counts, and with the shell's, where only the few rows that carry a force do.

The model is the sum over slabs of tests/_tri_loads64.py applied to each slab context's own downloads with the slab scene's
sphere-to-owner table and the slab's ghost copies (the clump owners behind its own ones) flagged, added in slab order.  The plate is
replicated with the same triangle ids on every slab, and no clump changes slabs (no migration is set), so the tables are those of
the library's plan.  Forces are held to the model within the bound derived in tests/test_tri_loads.py.  Counts are held to equality
with the model and with the undivided run.

The forces are also held to the undivided run's, per triangle and in total.  REL cannot be the bound there: a decomposed run follows
the undivided one within a tolerance, not bit for bit -- tests/test_decomp.py holds clump centres to 2e-7 m and velocities to
2e-3 m/s per component -- so one row's recorded force differs between the two runs by what those differences do to a Hertzian
contact.  The bound per listed row, PER_ROW below, is derived from them and from the scene, not from the answer:
  sphere centres and velocities: DX = 2 sqrt(3) * 2e-7 m, DV = 2 sqrt(3) * 2e-3 m/s (the vector norm of the per-component
    tolerance, doubled for the clump's rotation about its centre, which test_decomp.py does not bound by itself);
  stiffness: k = 2 E* sqrt(R d) with E* = E / (2 (1 - nu^2)) = 5.49e7 Pa, R = 4 mm, and d no deeper than the overlap that stops a
    clump (1.816 g) arriving at 2 m/s, twice the bed's initial speed: (8/15) E* sqrt(R) d^2.5 = m v^2 / 2, d = 3.3e-4 m, k = 1.26e5 N/m;
  damping: c = 2 sqrt(5/6) |beta| sqrt(k m), beta = ln CoR / sqrt(ln^2 CoR + pi^2) = -0.16 for CoR 0.6: c = 4.4 N s/m;
  a row's force changes by at most k DX + c DV along the normal and by as much again along the tangent (the tangential spring is no
    stiffer, its stretch differs by the integral of DV over a contact, which is below DX): PER_ROW = 2 (k DX + c DV) = 0.24 N.
A triangle's force may differ by PER_ROW times its listed rows, the total by PER_ROW times all listed sphere-mesh rows.  Measured
(MI355X, printed by the test): with 3 slabs the largest difference of a triangle's force is 2.4e-7 N -- one fp32 step of a 2 N
force, 1e-7 of the bound -- and the total differs by 1.2e-7 N of 80 N; with 2 slabs the two runs agree to the last bit."""
import numpy as np
import pytest

from tests._tri_loads64 import tri_loads
from tests.test_contact_inspect_multi import _table
from tests.test_owner_contacts import _stepped
from tests.test_owner_contacts_multi import HALO, built
from tests.test_tri_loads import REL, THR

pytestmark = pytest.mark.gpu
STEPS = 120
# the bound of one row's force between a decomposed and the undivided run (the module's docstring)
E_STAR = 1e8 / (2 * (1 - 0.3 ** 2))
RADIUS, CLUMP_MASS, V_MAX = 0.8 * 0.005, 2.6e3 * 5.5886717 * 0.005 ** 3, 2.0
DX, DV = 2 * np.sqrt(3.0) * 2e-7, 2 * np.sqrt(3.0) * 2e-3
D_MAX = (0.5 * CLUMP_MASS * V_MAX ** 2 / ((8.0 / 15.0) * E_STAR * np.sqrt(RADIUS))) ** 0.4
K_MAX = 2 * E_STAR * np.sqrt(RADIUS * D_MAX)
BETA = np.log(0.6) / np.sqrt(np.log(0.6) ** 2 + np.pi ** 2)
C_MAX = 2 * np.sqrt(5.0 / 6.0) * abs(BETA) * np.sqrt(K_MAX * CLUMP_MASS)
PER_ROW = 2 * (K_MAX * DX + C_MAX * DV)
_cache = {}


def bed_scene(pkg):
    if "bed" not in _cache:
        b = pkg.model.packed_bed(1500, seed=3, cd_freq=5, spacing_mult=2.8, init_vz=-1.0)  # (mesh_bed's, under a coarser plate)
        lo, hi = b.user_box_min, b.user_box_max
        v, f = pkg.model.plate_mesh(7, 7, float(hi[0] - lo[0]) * 0.9, float(hi[1] - lo[1]) * 0.9, z=0.0, wavy=0.003)
        m = b.AddMeshObject(v, f, 0)
        m.SetInitPos(((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, 0.0195))
        m.SetMass(0.5)
        m.SetMOI((1e-3, 1e-3, 2e-3))
        _cache["bed"] = b.Initialize()
    return _cache["bed"]


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
    """the same bed undivided, exact mode"""
    p, sc = bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, "exact", steps=STEPS)
    out = {thr: ctx.inspect_tri_loads(thr) for thr in (THR, 0.0)}
    a, b, t, _ = ctx.contacts()
    f = np.sqrt((ctx.contact_records()[0][t == 2].astype(np.float64) ** 2).sum(1))
    assert not ((f > THR / 2) & (f < 2 * THR)).any()  # no row a rounding could move across the threshold
    ctx.close()
    return out


def slab_model(pkg, m, p, sc, n_slabs, thr):
    plan, parts = pkg.decomp.decompose_lib(p, sc, n_slabs, HALO, axis=0, snap=True, spatial_order=True)
    nT = int(sc.nTri)
    total = {"force": np.zeros((nT, 3)), "abs_sum": np.zeros((nT, 3)), "counts": np.zeros(nT, np.uint32)}
    per_slab = []
    for s, pt in enumerate(parts):
        ctx, ssc = m.slab_ctx(s), pt["scene"]
        own, below, above = m.slab_counts(s)[0][:3]
        assert own == pt["n_own"] and int(ssc.nTri) == nT
        ghost = np.zeros(int(ssc.nOwners), bool)
        ghost[own:own + below + above] = True
        a, b, t, _ = ctx.contacts()
        one = tri_loads(a, b, t, ctx.contact_records()[0], _table(ssc, "ownerClumpBody", ssc.nSpheres), ghost, nT, thr)
        for k in total:
            total[k] += one[k]
        per_slab.append(one["counts"])
    plan.close()
    return total, per_slab


def test_slabs_add_up_to_the_model_and_to_the_undivided_run(pkg, run, single):
    m, p, sc, n_slabs = run["m"], run["p"], run["sc"], run["n_slabs"]
    for thr in (THR, 0.0):
        want, per_slab = slab_model(pkg, m, p, sc, n_slabs, thr)
        force, counts = m.inspect_tri_loads(thr)
        err = np.abs(force - want["force"])
        print(f"{n_slabs} slabs, thr {thr:g}: counted rows per slab {[int(c.sum()) for c in per_slab]}, max |force - model| {err.max():.3e}, "
              f"max abs_sum {want['abs_sum'].max():.3e}")
        assert counts.dtype == np.uint32 and np.array_equal(counts, want["counts"])
        assert (err <= REL * want["abs_sum"]).all()
        if thr == 0.0:  # the cut leaves sphere-mesh rows on at least two slabs, and some triangle gets rows from two
            assert sum(1 for c in per_slab if c.sum() > 0) >= 2
            assert (sum((c > 0).astype(np.int64) for c in per_slab) >= 2).any()
        # the undivided run: every sphere-triangle pair once
        one_force, one_counts = single[thr]
        assert np.array_equal(counts, one_counts) and counts.sum() >= (50 if thr == 0.0 else 5)
        listed = single[0.0][1].astype(np.float64)  # listed sphere-mesh rows per triangle (threshold 0: every one counts)
        dev = np.abs(force - one_force)
        dev_total = np.abs(force.sum(0) - one_force.sum(0))
        print(f"{n_slabs} slabs, thr {thr:g}: against the undivided run max |force - its| {dev.max():.3e} N "
              f"(bound there {PER_ROW * listed[np.unravel_index(dev.argmax(), dev.shape)[0]]:.3e}), "
              f"worst ratio to the bound {(dev / np.maximum(PER_ROW * listed[:, None], 1e-300)).max():.3e}, total {dev_total.max():.3e} N of "
              f"{np.abs(one_force.sum(0)).max():.3e} N (bound {PER_ROW * listed.sum():.3e}), PER_ROW {PER_ROW:.3e} N")
        assert (dev <= PER_ROW * listed[:, None]).all()
        assert (dev_total <= PER_ROW * listed.sum()).all() and np.abs(one_force.sum(0)).max() > 0
    a, _ = m.inspect_tri_loads(THR)
    b, _ = m.inspect_tri_loads(THR)
    assert a.tobytes() == b.tobytes() and a.any()
    f, n = m.inspect_tri_loads(THR, first=37, count=50)
    assert f.tobytes() == a[37:87].tobytes() and n.shape == (50,)


def test_bytes_and_refusals(pkg, run):
    m, sc, n_slabs, lib = run["m"], run["sc"], run["n_slabs"], run["m"].lib
    nT = int(sc.nTri)
    assert nT == 98
    before = m.query_host_bytes()
    m.inspect_tri_loads(THR)
    assert m.query_host_bytes() - before == 28 * nT * n_slabs
    f, n = np.full((50, 3), 7.5), np.full(50, 0xABABABAB, np.uint32)
    assert lib.deme_multi_inspect_tri_loads(m.h, THR, 37, 50, f.ctypes.data, None) == 0 and not (f == 7.5).all()
    assert m.query_host_bytes() - before == (28 * nT + 24 * 50) * n_slabs
    assert lib.deme_multi_inspect_tri_loads(m.h, THR, 5, 0, None, None) == 0
    assert m.query_host_bytes() - before == (28 * nT + 24 * 50) * n_slabs
    f[:] = 7.5
    for what, thr, first, count, pf, pn in (("threshold", -1.0, 0, 50, f, n), ("threshold", float("nan"), 0, 50, f, n),
                                           ("triangles", THR, 49, 50, f, n), ("null", THR, 0, 50, None, None)):
        rc = lib.deme_multi_inspect_tri_loads(m.h, thr, first, count, None if pf is None else pf.ctypes.data, None if pn is None else pn.ctypes.data)
        msg = lib.deme_multi_last_error(m.h).decode()
        assert rc == 1 and (f == 7.5).all() and (n == 0xABABABAB).all() and what in msg and "deme_multi_inspect_tri_loads" in msg, (what, msg)
    # recording off on one slab
    p, sc2 = bed_scene(pkg)
    off = built(pkg, p, sc2, n_slabs)
    off.slab_ctx(n_slabs - 1).set_record_contacts(False)
    off.step(STEPS)
    off.sync()
    assert lib.deme_multi_inspect_tri_loads(off.h, THR, 0, 50, f.ctypes.data, n.ctypes.data) == 1
    msg = lib.deme_multi_last_error(off.h).decode()
    assert (f == 7.5).all() and (n == 0xABABABAB).all() and "recording is off" in msg and "deme_multi_inspect_tri_loads" in msg
    off.close()
