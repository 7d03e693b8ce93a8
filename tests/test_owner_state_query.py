"""deme_query_owner_state / deme_multi_query_owner_state: position code, orientation, velocity, angular velocity and family of a
few owners, gathered on the device.  The values are copies of the owner records, so every comparison is np.array_equal on bit
patterns against download_state() indexed by the ids."""
import ctypes as C

import numpy as np
import pytest

from tests.test_owner_contacts import _bed_scene, _stepped
from tests.test_owner_contacts_multi import HALO, STEPS, bed_scene, built

pytestmark = pytest.mark.gpu
REC = 64  # bytes a gathered owner record brings to the host


def _same_state(got, whole, ids, what):
    ids = np.asarray(ids, np.int64)
    assert set(got) == set(whole) - {"aX", "aY", "aZ", "alphaX", "alphaY", "alphaZ"}, what
    for k, v in got.items():
        want = whole[k][ids]
        assert v.dtype == want.dtype and v.shape == want.shape, (what, k, v.shape, want.shape)
        assert np.array_equal(v.view(np.uint32) if v.dtype == np.float32 else v, want.view(np.uint32) if want.dtype == np.float32 else want), (what, k)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_owner_state_equals_the_indexed_download(pkg, mode):
    p, sc, mid = _bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, mode, steps=30)
    assert ctx.engine_order()[0] == (mode == "fast")  # the fast mode keeps an order of its own: ids go through the slot map
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    whole = ctx.download_state()
    assert np.abs(whole["vZ"][:nC]).max() > 0 and len(np.unique(whole["oriQw"][:nC])) > 1  # the bed has moved and turned
    before = ctx.query_host_bytes()
    cases = {
        "unsorted and repeated": [mid, nC - 1, 0, mid, 257, 131, nC, 131, mid],
        "the box": [nC],
        "every owner backwards": list(range(nO))[::-1],
        "empty": [],
    }
    moved = 0
    for what, ids in cases.items():
        _same_state(ctx.owner_state(ids), whole, ids, f"{mode}, {what}")
        moved += REC * len(ids)
    assert ctx.query_host_bytes() - before == moved
    two = ctx.owner_state([nC, 3], columns=("vZ", "familyID"))
    assert set(two) == {"vZ", "familyID"} and np.array_equal(two["vZ"], whole["vZ"][[nC, 3]]) and np.array_equal(two["familyID"], whole["familyID"][[nC, 3]])
    # refusals: an id out of range; a non-null acceleration column
    with pytest.raises(pkg.abi.DemeError, match="out of range"):
        ctx.owner_state([0, nO])
    with pytest.raises(pkg.abi.DemeError, match="reduction"):
        ctx.owner_state([0], columns=("vX", "aX"))
    st = pkg.abi.DemeOwnerState()
    ids = np.array([0], np.uint32)
    acc = np.full(1, 7.5, np.float32)
    st.alphaZ = acc.ctypes.data
    assert ctx.lib.deme_query_owner_state(ctx.h, ids.ctypes.data, 1, C.byref(st)) == 1 and acc[0] == 7.5
    ctx.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_owner_state_of_a_mesh_owner(pkg, mode):
    from tests.test_mesh import mesh_bed
    p, sc = mesh_bed(pkg, 600).Initialize()
    ctx = _stepped(pkg, p, sc, mode, steps=40)
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    whole = ctx.download_state()
    ids = [nO - 1, 5, nC, nO - 1, nC - 1]  # the mesh, a clump, the first owner behind the clumps
    _same_state(ctx.owner_state(ids), whole, ids, f"{mode}, mesh bed")
    ctx.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_owner_state_query_changes_nothing(pkg, mode):
    """a detection every 20 steps: step, ask, step -- the question must not make the second step detect again (as an upload of
    the same state would: it marks the list stale)"""
    b = pkg.model.packed_bed(300, seed=11, cd_freq=20, spacing_mult=2.4)
    p, sc = b.Initialize()
    ctx = _stepped(pkg, p, sc, mode, steps=1)
    assert ctx.counts().nDetections == 1
    ref = _stepped(pkg, p, sc, mode, steps=2)
    ctx.owner_state([0, 7, int(sc.nOwnerClumps)])
    ctx.step(1)
    ctx.sync()
    assert ctx.counts().nDetections == 1 and ctx.counts().nSteps == 2
    a, r = ctx.download_state(), ref.download_state()
    assert all(np.array_equal(a[k], r[k]) for k in pkg.abi.QUERY_STATE_COLUMNS)  # the trajectory of two uninterrupted steps
    ctx.close(), ref.close()


@pytest.mark.parametrize("n_slabs", [3, 2])
def test_multi_owner_state_equals_the_indexed_download(pkg, n_slabs):
    p, sc = bed_scene(pkg)
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    m = built(pkg, p, sc, n_slabs)
    m.step(STEPS)
    m.sync()
    whole = m.download_state()
    plan, parts = pkg.decomp.decompose_lib(p, sc, n_slabs, HALO, axis=0, snap=True, spatial_order=True)
    ghost = int(parts[1]["ghost_left_g"][0])  # slab 0's clump inside slab 1's halo: two slabs hold a copy, one answers
    x = pkg.model.decode_positions(whole["voxelID"], whole["locX"], whole["locY"], whole["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)[:nC, 0] + p.LBFX
    own = parts[n_slabs - 1]["global_ids"]
    deep = int(own[np.argmax(x[own])])  # the clump of the last slab farthest from its cut
    plan.close()
    assert np.abs(whole["vZ"][:nC]).max() > 0
    before = m.query_host_bytes()
    ids = [ghost, deep, nC, deep, nO - 1, 0]
    got = m.owner_state(ids)
    _same_state(got, whole, ids, f"{n_slabs} slabs")
    distinct = len(set(ids))
    assert m.query_host_bytes() - before == 4 * n_slabs + REC * distinct  # per-slab counts and per-hit bytes only
    every = list(range(nO))[::-1]
    _same_state(m.owner_state(every), whole, every, f"{n_slabs} slabs, every owner")
    assert m.owner_state([])["vX"].shape == (0,)
    with pytest.raises(pkg.abi.DemeError, match="out of range"):
        m.owner_state([nO])
    with pytest.raises(pkg.abi.DemeError, match="reduction"):
        m.owner_state([0], columns=("alphaX",))
    m.close()
