"""deme_multi_change_owner_sizes: a decomposed run resized by GLOBAL owner id -- own clumps and ghost copies on every slab, one
component table for all slabs (migration carries component indices), a halo that no longer fits refused with nothing changed.
The single-domain resized run is the yardstick, within the bounds tests/test_multi.py holds slabs to against the single domain."""
import numpy as np
import pytest

from tests.test_decomp import GKEYS, _sheared_bed
from tests.test_multi import _bed, _positions

pytestmark = pytest.mark.gpu


def _third(nc, f1=1.05, f2=0.95):
    ids = np.arange(0, nc, 3, dtype=np.uint32)
    return ids, np.where((np.arange(ids.size) % 2) == 0, f1, f2).astype(np.float32)


def _single(pkg, p, sc, ids, fac):
    c = pkg.Context(0)
    c.set_arith_mode("exact"), c.set_params(p), c.upload_scene(sc)
    c.change_owner_sizes(ids, fac)
    return c


def _same_tables(m, n_slabs):
    t0 = m.slab_ctx(0).components()
    for s in range(1, n_slabs):
        assert np.array_equal(m.slab_ctx(s).components(), t0), f"slab {s} holds another component table"
    return t0


def _same_geometry(m, n_slabs, one, n_spheres):
    """every sphere (by global id) has the single domain's relative position and radius, bit for bit"""
    t = _same_tables(m, n_slabs)
    g = t[m.sphere_components(n_spheres)]
    w = one.components()[one.sphere_components()]
    assert np.array_equal(g, w)


@pytest.mark.parametrize("n_slabs", [2, 4])
def test_multi_resize_equals_the_single_domain_resize(pkg, n_slabs):
    b, p, sc = _bed(pkg, cd_freq=7)
    nc, ns = int(sc.nOwnerClumps), int(sc.nSpheres)
    ids, fac = _third(nc)
    m = pkg.abi.Multi(devices=(0,))
    m.build(p, sc, slabs_per_device=n_slabs, axis=0, halo=0.03, arith="exact")
    one = pkg.Context(0)
    one.set_arith_mode("exact"), one.set_params(p), one.upload_scene(sc)
    m.step(20), one.step(20)
    m.sync()
    m.change_owner_sizes(ids, fac)
    one.change_owner_sizes(ids, fac)
    _same_geometry(m, n_slabs, one, ns)
    m.step(60), one.step(60)
    m.sync()
    g, o = m.download_state(), one.download_state()
    dx = np.abs(_positions(pkg, p, g, nc) - _positions(pkg, p, o, nc)).max()
    dv = max(np.abs(g[k][:nc] - o[k][:nc]).max() for k in ("vX", "vY", "vZ"))
    assert dx < 5e-9 and dv < 1e-4, (dx, dv)
    ga, gb, gt = m.contacts()
    oa, ob, ot, _ = one.contacts()
    assert len(ga) == len(oa) > 500 and np.array_equal(ga, oa) and np.array_equal(gb, ob)
    m.close()


def test_migrated_resized_clumps_keep_their_geometry(pkg):
    b, p, sc, x = _sheared_bed(pkg, 20_000, 6)
    nc, ns = int(sc.nOwnerClumps), int(sc.nSpheres)
    ids, fac = _third(nc)
    m = pkg.abi.Multi(devices=(0,))
    m.build(p, sc, slabs_per_device=3, axis=0, halo=0.035, arith="exact")
    m.set_migration(50)
    one = _single(pkg, p, sc, ids, fac)
    m.change_owner_sizes(ids, fac)
    m.step(151), one.step(151)
    m.sync()
    cnt, moved = m.counts()
    assert moved > 20, moved
    _same_geometry(m, 3, one, ns)
    g, o = m.download_state(), one.download_state()
    assert np.abs(_positions(pkg, p, g, nc) - _positions(pkg, p, o, nc)).max() < 1e-4
    m.close()


def test_growth_past_the_halo_is_refused_and_changes_nothing(pkg):
    b, p, sc = _bed(pkg, cd_freq=7)
    nc = int(sc.nOwnerClumps)
    m = pkg.abi.Multi(devices=(0,))
    m.build(p, sc, slabs_per_device=2, axis=0, halo=0.03, arith="exact")
    m.step(10)
    m.sync()
    st = m.download_state()
    t0 = m.slab_ctx(0).components()
    with pytest.raises(pkg.abi.DemeError, match="halo of 0.03"):
        m.change_owner_sizes(np.arange(0, nc, 5, dtype=np.uint32), np.full(len(range(0, nc, 5)), 3.0, np.float32))
    assert np.array_equal(m.slab_ctx(0).components(), t0) and np.array_equal(m.slab_ctx(1).components(), t0)
    back = m.download_state()
    assert all(np.array_equal(back[k], st[k]) for k in GKEYS)
    m.step(10)  # and the run goes on
    m.close()
