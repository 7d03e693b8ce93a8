"""deme_change_owner_sizes (the reference's ChangeClumpSizes): clumps of a running simulation grow or shrink.  The oracle cannot
resize, so every check compares a resized run against a scene BUILT pre-scaled -- components np.float32(c) * np.float32(f), the
same masses and MOIs -- which in the exact arithmetic mode is the same arithmetic, bit for bit."""
import ctypes as C

import numpy as np
import pytest

KEYS = ("voxelID", "locX", "locY", "locZ", "oriQw", "oriQx", "oriQy", "oriQz", "vX", "vY", "vZ", "omgBarX", "omgBarY", "omgBarZ")
COUNTS = ("nOwners", "nOwnerClumps", "nSpheres", "nAnal", "nTri", "nMat", "nComp", "nMassProps")


def test_resize_entry_points_are_exported(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in ("deme_change_owner_sizes", "deme_num_components", "deme_download_components", "deme_download_sphere_components"):
        assert n in names and hasattr(lib, n), n
    assert hasattr(pkg.Context, "change_owner_sizes") and hasattr(pkg.Context, "num_components")


def _bed(pkg, n, K=20, seed=31):
    b = pkg.model.packed_bed(n, seed=seed, cd_freq=K, spacing_mult=3.0, init_vz=-1.0)
    b.SetExpandSafetyAdder(1.0)
    return b.Initialize()


def _prescaled(pkg, sc, ids, factors):
    """the scene with owner ids[i]'s components multiplied by factors[i] (one derived entry per distinct (component, factor))"""
    arr = {k: np.array(v, copy=True) for k, v in sc._keep.items()}
    counts = {k: int(getattr(sc, k)) for k in COUNTS}
    comp = arr["clumpComponentOffset"].astype(np.int64)
    owner = arr["ownerClumpBody"]
    tab = [arr[k].astype(np.float32) for k in ("CDRelPosX", "CDRelPosY", "CDRelPosZ", "Radii")]
    fac = np.zeros(counts["nOwners"], np.float32)
    fac[np.asarray(ids, np.int64)] = np.asarray(factors, np.float32)
    new = {}
    cols = [list(t) for t in tab]
    for s in range(counts["nSpheres"]):
        f = fac[owner[s]]
        if f == 0:
            continue
        key = (int(comp[s]), float(f))
        if key not in new:
            new[key] = len(cols[0])
            for j in range(4):
                cols[j].append(np.float32(tab[j][comp[s]]) * np.float32(f))
        comp[s] = new[key]
    for j, k in enumerate(("CDRelPosX", "CDRelPosY", "CDRelPosZ", "Radii")):
        arr[k] = np.asarray(cols[j], np.float32)
    arr["clumpComponentOffset"] = comp.astype(np.uint16)
    counts["nComp"] = len(cols[0])
    return pkg.abi.make_scene_struct(arr, counts)


def _ctx(pkg, p, sc, mode="exact"):
    c = pkg.Context(0)
    c.set_arith_mode(mode)
    c.set_params(p)
    c.upload_scene(sc)
    return c


def _third(sc, f1=1.25, f2=0.8):
    nc = int(sc.nOwnerClumps)
    ids = np.arange(0, nc, 3, dtype=np.uint32)
    fac = np.where((np.arange(ids.size) % 2) == 0, f1, f2).astype(np.float32)
    return ids, fac


def _same_run(x, y, what, lists=True):
    """lists=False: an asynchronous detection's list holds extra near-pairs (zero history) beside the lock-step one"""
    if lists:
        xa, xb, xt, _ = x.contacts()
        ya, yb, yt, _ = y.contacts()
        assert np.array_equal(xa, ya) and np.array_equal(xb, yb) and np.array_equal(xt, yt), f"{what}: contact lists differ"
        for w in range(x.n_wildcards):
            assert np.array_equal(x.wildcard(w), y.wildcard(w)), f"{what}: history wildcard {w} differs"
    sx, sy = x.download_state(), y.download_state()
    for k in KEYS:
        assert np.array_equal(sx[k], sy[k]), f"{what}: {k} differs"


def _same_as_oracle(c, sim, what, lists=True):
    if lists:
        a, b, t, _ = c.contacts()
        oa, ob, ot, _ = sim.contacts()
        assert np.array_equal(a, oa) and np.array_equal(b, ob) and np.array_equal(t, ot), f"{what}: contact set differs from the oracle"
    gs, os_ = c.download_state(), sim.download_state()
    for k in KEYS:
        assert np.array_equal(gs[k], os_[k]), f"{what}: {k} differs from the oracle"


@pytest.mark.gpu
def test_resize_at_step_zero_matches_prescaled_scene(pkg, orc):
    p, sc = _bed(pkg, 20000)
    ids, fac = _third(sc)
    pre = _prescaled(pkg, sc, ids, fac)
    g = _ctx(pkg, p, sc)
    g.change_owner_sizes(ids, fac)
    g.step(200)  # K = 20: ten detections
    sim = orc.make_sim(pkg, p, pre)
    sim.step(200)
    ref = _ctx(pkg, p, pre)
    ref.step(200)
    assert len(g.contacts()[0]) > 1000
    _same_run(g, ref, "exact, resized at step 0 vs pre-scaled")
    _same_as_oracle(g, sim, "exact, resized at step 0")
    # fast mode: within the bound test_fast_mode.py holds the fast path to against the oracle
    gf, rf = _ctx(pkg, p, sc, "fast"), _ctx(pkg, p, pre, "fast")
    gf.change_owner_sizes(ids, fac)
    gf.step(200), rf.step(200)
    assert gf.force_kernel()[0] == "k_tile_forces<0, false>"
    S, O = gf.download_state(), sim.download_state()
    X = pkg.model.decode_positions(S["voxelID"], S["locX"], S["locY"], S["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    Y = pkg.model.decode_positions(O["voxelID"], O["locX"], O["locY"], O["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    assert float(np.abs(X - Y).max()) <= 5e-8
    assert max(float(np.abs(S[k] - O[k]).max()) for k in ("vX", "vY", "vZ")) <= 1e-3


def _restart_from(pkg, p, scene, src, mode="exact"):
    """a context of `scene` seeded with src's state, contact list and history (the restart path)"""
    c = _ctx(pkg, p, scene, mode)
    c.upload_state(src.download_state())
    a, b, t, _ = src.contacts()
    W = np.stack([src.wildcard(w) for w in range(src.n_wildcards)], axis=1) if src.n_wildcards else None
    c.seed_contacts(a, b, t, W)
    return c


def _restart_oracle(orc, pkg, p, scene, src):
    sim = orc.make_sim(pkg, p, scene)
    sim.upload_state(src.download_state())
    a, b, t, _ = src.contacts()
    W = np.stack([src.wildcard(w) for w in range(src.n_wildcards)], axis=1) if src.n_wildcards else None
    sim.seed_contacts(a, b, t, W)
    return sim


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 6])
def test_resize_mid_run_matches_restarted_prescaled_scene(pkg, orc, lead):
    """k steps, resize, m steps; lead > 0: with the asynchronous detection on, a list detected with the old sizes is never used"""
    p, sc = _bed(pkg, 20000)
    # (with the asynchronous detection, gentle factors: a 25 % growth in a packed bed starts an explosion whose speeds outrun margins
    # sized D steps ahead -- the limit of that mode, resized or not)
    ids, fac = _third(sc, *((1.02, 0.98) if lead else (1.25, 0.8)))
    pre = _prescaled(pkg, sc, ids, fac)
    g = _ctx(pkg, p, sc)
    if lead:
        g.set_async_detection(lead)
    g.step(130)  # (mid-way between two detections)
    ref = _restart_from(pkg, p, pre, g)
    sim = _restart_oracle(orc, pkg, p, pre, g)
    X0, Y0, Z0, R0 = g.sphere_geometry()
    g.change_owner_sizes(ids, fac)
    X1, Y1, Z1, R1 = g.sphere_geometry()
    resized = np.isin(sc._keep["ownerClumpBody"], ids)
    assert np.array_equal(R0[~resized], R1[~resized]) and not np.any(R0[resized] == R1[resized])
    r = sc._keep["Radii"][sc._keep["clumpComponentOffset"]]
    f = np.zeros(int(sc.nOwners), np.float32)
    f[ids] = fac
    fs = f[sc._keep["ownerClumpBody"]]
    assert np.allclose(R1[resized] - R0[resized], r[resized] * (fs[resized] - 1.0), rtol=1e-4, atol=1e-9)
    g.step(150)
    if not lead:
        ref.step(150), sim.step(150)
        _same_run(g, ref, "exact, resized mid-run vs restarted pre-scaled")
        _same_as_oracle(g, sim, "exact, resized mid-run")
    else:  # the lock-step resized run is the same trajectory, and every pair both lists hold carries the same history
        h = _ctx(pkg, p, sc)
        h.step(130)
        h.change_owner_sizes(ids, fac)
        h.step(150)
        _same_run(g, h, "asynchronous vs lock-step resized run", lists=False)
        wg = {q: w for q, w in zip(zip(*[x.tolist() for x in g.contacts()[:3]]), g.wildcard(g.n_wildcards - 1).tolist())}
        wh = {q: w for q, w in zip(zip(*[x.tolist() for x in h.contacts()[:3]]), h.wildcard(h.n_wildcards - 1).tolist())}
        common = [q for q in wh if q in wg]
        assert len(common) > 100 and all(wg[q] == wh[q] for q in common)
        assert all(wh[q] == 0.0 for q in wh if q not in wg)


@pytest.mark.gpu
def test_repeated_uniform_growth_keeps_the_table_compact(pkg):
    p, sc = _bed(pkg, 6000)
    nT = int(sc.nComp)
    g = _ctx(pkg, p, sc, "fast")
    ids = np.arange(int(sc.nOwnerClumps), dtype=np.uint32)
    total = np.float32(1.0)
    for _ in range(10):
        g.change_owner_sizes(ids, np.full(ids.size, 1.01, np.float32))
        total = total * np.float32(1.01)
        assert g.num_components() <= 2 * nT
        g.step(20)
    assert g.force_kernel()[0] == "k_tile_forces<0, false>"
    tab = g.components()
    assert np.array_equal(tab[:nT, 3], sc._keep["Radii"])  # the templates stay
    comp = g.sphere_components()
    assert comp.min() >= nT  # every sphere is on a derived entry
    # compounding: ten fp32 multiplies of the current value
    want = sc._keep["Radii"][sc._keep["clumpComponentOffset"]].copy()
    for _ in range(10):
        want = want * np.float32(1.01)
    assert np.array_equal(tab[comp, 3], want)


@pytest.mark.gpu
def test_per_clump_factors_take_the_general_path_and_stay_exact(pkg, orc):
    p, sc = _bed(pkg, 2000)
    nc = int(sc.nOwnerClumps)
    ids = np.arange(nc, dtype=np.uint32)
    fac = (1.0 + 0.1 * np.random.default_rng(3).random(nc)).astype(np.float32)
    pre = _prescaled(pkg, sc, ids, fac)
    g, ref = _ctx(pkg, p, sc), _ctx(pkg, p, pre)
    g.change_owner_sizes(ids, fac)
    assert g.num_components() == int(sc.nComp) + 3 * np.unique(fac).size  # (equal factors share their entries)
    g.step(120), ref.step(120)
    _same_run(g, ref, "per-clump factors")
    gf = _ctx(pkg, p, sc, "fast")
    gf.change_owner_sizes(ids, fac)
    gf.step(40)
    assert gf.force_kernel()[0] != "k_tile_forces<0, false>"  # the table is past the tile path's limit
    sim = orc.make_sim(pkg, p, pre)  # ... and the general fast path computes the pre-scaled scene within the fast mode's bounds
    sim.step(40)
    S, O = gf.download_state(), sim.download_state()
    X = pkg.model.decode_positions(S["voxelID"], S["locX"], S["locY"], S["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    Y = pkg.model.decode_positions(O["voxelID"], O["locX"], O["locY"], O["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    assert float(np.abs(X - Y).max()) <= 5e-8
    assert max(float(np.abs(S[k] - O[k]).max()) for k in ("vX", "vY", "vZ")) <= 1e-3


@pytest.mark.gpu
def test_a_re_upload_that_names_its_templates_keeps_the_table_compact(pkg):
    """resize, then re-upload the scene with the effective geometry (what the shell's UpdateClumps does) and name the true template
    count: ten such cycles keep the table within twice the templates"""
    p, sc = _bed(pkg, 3000)
    nT = int(sc.nComp)
    g = _ctx(pkg, p, sc)
    ids = np.arange(int(sc.nOwnerClumps), dtype=np.uint32)
    for _ in range(10):
        g.change_owner_sizes(ids, np.full(ids.size, 1.01, np.float32))
        assert g.num_components() <= 2 * nT
        tab, comp, st = g.components(), g.sphere_components(), g.download_state()
        arr = {k: np.array(v, copy=True) for k, v in sc._keep.items()}
        counts = {k: int(getattr(sc, k)) for k in COUNTS}
        for j, k in enumerate(("CDRelPosX", "CDRelPosY", "CDRelPosZ", "Radii")):
            arr[k] = tab[:, j].copy()
        arr["clumpComponentOffset"] = comp
        counts["nComp"] = tab.shape[0]
        for k in KEYS:
            arr[k] = st[k]
        scene = pkg.abi.make_scene_struct(arr, counts)
        g.upload_scene(scene)
        g.set_template_components(nT)
        g.step(10)
    assert g.num_components() <= 2 * nT
    with pytest.raises(pkg.abi.DemeError):
        g.set_template_components(g.num_components() + 1)


def _snapshot(c):
    a, b, t, _ = c.contacts()
    return c.num_components(), c.components(), c.sphere_components(), c.download_state(), (a, b, t)


def _unchanged(c, before):
    n, tab, comp, st, (a, b, t) = before
    assert c.num_components() == n and np.array_equal(c.components(), tab) and np.array_equal(c.sphere_components(), comp)
    s2 = c.download_state()
    assert all(np.array_equal(s2[k], st[k]) for k in KEYS)
    a2, b2, t2, _ = c.contacts()
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(t, t2)


@pytest.mark.gpu
def test_a_table_past_65535_components_is_refused(pkg):
    p, sc = _bed(pkg, 22000)
    g = _ctx(pkg, p, sc)
    g.step(10)
    before = _snapshot(g)
    nc = int(sc.nOwnerClumps)
    assert 3 * nc + int(sc.nComp) > 65535
    fac = (1.0 + np.arange(nc, dtype=np.float32) * np.float32(1e-6)).astype(np.float32)
    with pytest.raises(pkg.abi.DemeError, match="65535"):
        g.change_owner_sizes(np.arange(nc, dtype=np.uint32), fac)
    _unchanged(g, before)
    g.step(10)  # and the run goes on


@pytest.mark.gpu
def test_bad_requests_are_refused_and_change_nothing(pkg):
    p, sc = _bed(pkg, 2000)
    g = _ctx(pkg, p, sc)
    g.step(30)
    before = _snapshot(g)
    n = int(sc.nOwners)
    lib = pkg.abi.load_library()
    for ids, fac, what in (([0, n], [1.1, 1.1], "out of range"), ([4, 5, 4], [1.1, 1.2, 1.3], "twice"),
                           ([1], [0.0], "> 0"), ([1], [-2.0], "> 0"), ([1], [float("nan")], "finite"), ([1], [float("inf")], "finite")):
        with pytest.raises(pkg.abi.DemeError, match=what):
            g.change_owner_sizes(ids, fac)
        _unchanged(g, before)
    with pytest.raises(pkg.abi.DemeError):
        g.change_owner_sizes([1, 2], [1.1])
    _unchanged(g, before)
    # owners without spheres (the walls are owners behind the clumps) are a silent no-op
    assert n > int(sc.nOwnerClumps)  # (the bed's walls)
    g.change_owner_sizes([n - 1], [2.0])
    _unchanged(g, before)
    # before a scene is uploaded: refused
    c = pkg.Context(0)
    x = np.array([0], np.uint32)
    f = np.array([1.1], np.float32)
    assert lib.deme_change_owner_sizes(c.h, x.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), 1) != 0
