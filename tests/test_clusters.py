"""deme_inspect_clusters (Context.inspect_clusters): the connected components of the contact network -- labels, summary and the
cluster table -- labelled on the device, against tests/_clusters64.py applied to the whole-list downloads, the scene's owner tables
and the downloaded owner state.

Scenes:
  the bed of tests/test_owner_contacts.py: 300 three-sphere clumps on the floor of their box, the last clump left hanging; 573 rows;
  a chain: 2311 single-sphere clumps in one line along x, each overlapping its neighbour and nobody else, the caller ids a fixed
    random permutation of the positions -- 2310 rows, more than 8 workgroups of the link kernel, the longest find path and the most
    contention the algorithm can meet at this size, one cluster of 2311 sorted entries (2311 % 256 != 0: its table row goes through
    the partials of the final pass); the same chain with the overlap removed at three places is four clusters with known minima;
  many small clusters: 324 cells of a grid holding one, two or three overlapping spheres each, ids permuted.

Tolerance of a double: |got - model| <= 1e-10 * abs_sum per entry, abs_sum the sum of |term| over the cluster's terms: the
derivation of tests/test_contact_inspect.py -- both sides add the same fp64 terms (each product m * P is one rounding of the same
two fp64 factors) in different orders, so the difference is at most n * 1.1e-16 * abs_sum, and n < 1e5 is asserted.  The integers
are compared for equality."""
import ctypes as C
import math

import numpy as np
import pytest

from tests._clusters64 import NONE, clusters, edges_of, union_find
from tests._fields64 import positions
from tests.test_contact_inspect import no_force_near
from tests.test_owner_contacts import _bed_scene, _owner_tables, _stepped, _whole_list

THR = 1e-12  # what the shell passes (DEME_TINY_FLOAT_HOST)
REL = 1e-10
SYMBOLS = ("deme_inspect_clusters", "deme_multi_inspect_clusters", "deme_clusters_link_retries")
SUMMARY = ("vertices", "edges", "clusters", "singletons", "largestSize", "largestLabel")
COLUMNS = ("label", "size", "mass", "moment")
ROW_BYTES = {"label": 4, "size": 4, "mass": 8, "moment": 24}
HEAD_BYTES, SUMMARY_BYTES = 16, 48
R = 2.0e-4       # sphere radius of the chain and of the small clusters
PITCH = 1.8 * R  # neighbours overlap by 0.2 R; the next but one is 3.6 R away
N_CHAIN, CUTS = 2311, (500, 1203, 1900)  # the chain is cut in front of these positions


def test_cluster_inspector_is_exported_and_bound(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in SYMBOLS:
        assert n in names and hasattr(lib, n), n
    for cls in (pkg.Context, pkg.abi.Multi):
        assert hasattr(cls, "inspect_clusters"), cls.__name__
    assert len(lib.deme_inspect_clusters.argtypes) == 8 and len(lib.deme_multi_inspect_clusters.argtypes) == 8
    assert C.sizeof(pkg.abi.DemeClusterSummary) == 48 and C.sizeof(pkg.abi.DemeClusterColumns) == 32
    assert tuple(n for n, _ in pkg.abi.DemeClusterSummary._fields_) == SUMMARY
    assert pkg.abi.CLUSTER_COLUMNS == COLUMNS and pkg.abi.CLUSTER_NONE == NONE


def test_the_model_on_a_hand_written_graph():
    """seven owners: clumps 0..4, a ghost copy 5 (no vertex here), a mesh owner 6.  Rows: 3-1, 1-4 (two rows), 2-2 (one clump's own
    spheres), 0-5 (a ghost), 3-6 (the mesh), 0-2 below the threshold, a sphere-plane row of 0"""
    tables = (np.array([0, 1, 2, 2, 3, 4, 5], np.uint32), np.array([6], np.uint32), np.array([6], np.uint32))
    whole = {"idA": np.array([4, 1, 1, 2, 0, 4, 0, 0], np.uint32), "idB": np.array([1, 5, 5, 3, 6, 0, 2, 0], np.uint32),
             "type": np.array([1, 1, 1, 1, 1, 2, 1, 3], np.uint8),
             "force": np.array([[1, 0, 0], [0, 2, 0], [0, 0, 4], [8, 0, 0], [1, 1, 1], [0, 0, 16], [1e-3, 0, 0], [5, 0, 0]], np.float32)}
    vertex = np.array([True] * 5 + [False, False])
    X = np.arange(21, dtype=np.float64).reshape(7, 3)
    mass = np.array([1, 2, 4, 8, 16, 32, 64], np.float32)
    m = clusters(X, mass, vertex, whole, tables, 0.01)
    assert m["labels"].tolist() == [0, 1, 2, 1, 1, NONE, NONE] and m["labels"].dtype == np.uint32
    assert m["summary"] == {"vertices": 5, "edges": 3, "clusters": 3, "singletons": 2, "largestSize": 3, "largestLabel": 1}
    assert m["label"].tolist() == [0, 1, 2] and m["size"].tolist() == [1, 3, 1] and m["mass"].tolist() == [1, 26, 4]
    assert m["moment"][1].tolist() == [2 * 3 + 8 * 9 + 16 * 12, 2 * 4 + 8 * 10 + 16 * 13, 2 * 5 + 8 * 11 + 16 * 14]
    m0 = clusters(X, mass, vertex, whole, tables, 0.0)  # the row 0-2 now counts
    assert m0["labels"].tolist() == [0, 1, 0, 1, 1, NONE, NONE] and m0["summary"]["edges"] == 4 and m0["summary"]["singletons"] == 0
    # a slab: the ghost copy links (0-5 joins them) and is never counted
    s = clusters(X, mass, np.array([True] * 6 + [False]), whole, tables, 0.01, counted=vertex)
    assert s["labels"].tolist() == [0, 1, 2, 1, 1, 0, NONE] and s["size"].tolist() == [1, 3, 1] and s["mass"].tolist() == [1, 26, 4]
    assert union_find(6, [5, 3, 1], [4, 5, 2]).tolist() == [0, 1, 1, 3, 3, 3]


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def spheres_scene(pkg, X_by_id, box):
    """single-sphere clumps of radius R at the given centres (row = caller id) in a box without walls, no gravity; two templates of
    different mass alternate, so that the table's masses are no multiples of one number"""
    b = pkg.SceneBuilder()
    mat = b.LoadMaterial({"E": 1e7, "nu": 0.3, "CoR": 0.6, "mu": 0.2, "Crr": 0.0})
    b.InstructBoxDomainDimension((0.0, box[0]), (0.0, box[1]), (0.0, box[2]))
    b.InstructBoxDomainBoundingBC("none", mat)
    vol = 4.0 / 3.0 * math.pi * R ** 3
    types = [b.LoadSphereType(rho * vol, R, mat) for rho in (2.6e3, 7.8e3)]
    b.AddClumps([types[i % 2] for i in range(len(X_by_id))], np.asarray(X_by_id, np.float32))
    b.SetInitTimeStep(1e-7)
    b.SetGravitationalAcceleration((0, 0, 0))
    b.SetCDUpdateFreq(0)
    b.SetInitBinSizeAsMultipleOfSmallestSphere(4.0)
    b.SetExpandSafetyAdder(0.0)
    b.SetMaxVelocity(5.0)
    b.SetErrorOutVelocity(1e3)
    return b.Initialize()


def chain_positions(n=N_CHAIN, cuts=(), seed=17):
    """(X by caller id, the permutation: perm[j] is the id of the j-th sphere along x).  A cut widens the gap in front of position
    c to 2.5 R: no overlap there."""
    x = np.zeros(n)
    gap = np.full(n, PITCH)
    gap[0] = 0.0
    for c in cuts:
        gap[c] = 2.5 * R
    x = 0.01 + np.cumsum(gap)
    perm = np.random.default_rng(seed).permutation(n)
    X = np.zeros((n, 3))
    X[perm, 0] = x
    X[:, 1] = X[:, 2] = 0.01
    assert x[-1] < 0.99
    return X, perm


def chain_scene(pkg, cuts=()):
    X, perm = chain_positions(cuts=cuts)
    p, sc = spheres_scene(pkg, X, (1.0, 0.02, 0.02))
    return p, sc, perm


def small_clusters_positions(side=18, seed=23):
    """side x side cells of pitch 8 R in the plane z = 0.01: cell c holds 1 + c % 3 spheres in a row along x.  Returns (X by caller
    id, the cell of every id)"""
    pts, cell = [], []
    for c in range(side * side):
        for k in range(1 + c % 3):
            pts.append((0.01 + 8 * R * (c % side) + PITCH * k, 0.01 + 8 * R * (c // side), 0.01))
            cell.append(c)
    pts, cell = np.array(pts), np.array(cell)
    perm = np.random.default_rng(seed).permutation(len(pts))
    X, cells = np.zeros_like(pts), np.zeros(len(pts), np.int64)
    X[perm], cells[perm] = pts, cell
    return X, cells


def owner_mass(sc):
    keep = sc._keep
    return np.asarray(keep["MassProperties"], np.float32).reshape(int(sc.nMassProps), -1)[:, 0][np.asarray(keep["inertiaPropOffsets"], np.int64)]


def setup(pkg, ctx, p, sc, mode):
    state = ctx.download_state()
    return {"ctx": ctx, "p": p, "sc": sc, "mode": mode, "whole": _whole_list(ctx, sc), "state": state, "mass": owner_mass(sc),
            "X": positions(pkg.model.decode_positions, p, state)}


def model(s, thr=THR):
    sc = s["sc"]
    vertex = np.arange(int(sc.nOwners)) < int(sc.nOwnerClumps)
    return clusters(s["X"], s["mass"], vertex, s["whole"], _owner_tables(sc), thr)


def check(got, want, what, max_terms=1e5):
    print(f"{what}: summary {got['summary']}")
    assert got["summary"] == want["summary"], (what, got["summary"], want["summary"])
    assert got["labels"].dtype == np.uint32 and np.array_equal(got["labels"], want["labels"]), what
    for k in ("label", "size"):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), (what, k)
    assert (np.diff(got["label"].astype(np.int64)) > 0).all()  # labels ascending
    assert int(got["size"].sum()) == got["summary"]["vertices"] and len(got["label"]) == got["summary"]["clusters"]
    abs_mass = want["mass"]  # (every term is positive)
    for k, abs_sum in (("mass", abs_mass), ("moment", want["abs_moment"])):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, (what, k)
        err = np.abs(got[k] - want[k])
        if err.size:
            print(f"{what}, {k}: max |got - model| {err.max():.3e}, max abs_sum {abs_sum.max():.3e}, "
                  f"worst ratio {(err / np.maximum(abs_sum, 1e-300)).max():.3e}")
        assert (err <= REL * abs_sum).all(), (what, k)
    assert want["size"].max(initial=0) < max_terms


@pytest.fixture(scope="module", params=["fast", "exact"])
def bed(pkg, request):
    p, sc, mid = _bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, request.param)
    yield setup(pkg, ctx, p, sc, request.param)
    ctx.close()


@pytest.fixture(scope="module", params=["fast", "exact"])
def chain(pkg, request):
    p, sc, perm = chain_scene(pkg)
    ctx = _stepped(pkg, p, sc, request.param)
    s = setup(pkg, ctx, p, sc, request.param)
    s["perm"] = perm
    yield s
    ctx.close()


def threshold_gap(whole):
    """a threshold inside the widest gap of the sorted |f| of the sphere-sphere rows: if the gap is a factor 4 or more, no row's
    |f| is within a factor 2 of it (no_force_near)"""
    f = np.sort(np.sqrt((whole["force"][whole["type"] == 1].astype(np.float64) ** 2).sum(1)))
    f = f[f > 0]
    k = int(np.argmax(f[1:] / f[:-1]))
    return float(np.float32(math.sqrt(f[k] * f[k + 1])))


def threshold_at(whole, q):
    """a threshold between two neighbours of the sorted |f| of the sphere-sphere rows at the q-quantile: the fp32 number nearest to
    their mean.  Returns (thr, the smallest |f| / thr - 1 in magnitude over the rows)"""
    f = np.sort(np.sqrt((whole["force"][whole["type"] == 1].astype(np.float64) ** 2).sum(1)))
    k = int(q * len(f))
    while f[k + 1] < f[k] * (1 + 1e-3):  # (neighbours too close to put an fp32 number well between them: the next pair)
        k += 1
    thr = float(np.float32(0.5 * (f[k] + f[k + 1])))
    every = np.sqrt((whole["force"].astype(np.float64) ** 2).sum(1))
    return thr, float(np.abs(every / thr - 1.0).min())


# ---- the bed ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bed_equals_the_model(pkg, bed):
    ctx, sc, whole = bed["ctx"], bed["sc"], bed["whole"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    assert no_force_near(whole, THR) and ctx.engine_order()[0] == (bed["mode"] == "fast")
    want = model(bed)
    got = ctx.inspect_clusters(THR)
    check(got, want, f"{bed['mode']}, the shell's threshold")
    # the floor rows join nothing: the box is no vertex, and without the sphere-sphere rows every clump is alone
    assert (whole["type"] > 2).any() and (got["labels"][nC:] == NONE).all() and (got["labels"][:nC] < nC).all()
    only_floor = {k: v[whole["type"] > 2] for k, v in whole.items()}
    assert clusters(bed["X"], bed["mass"], np.arange(nO) < nC, only_floor, _owner_tables(sc), THR)["summary"]["clusters"] == nC
    # the lone last clump is a singleton
    assert got["labels"][nC - 1] == nC - 1 and got["size"][got["label"] == nC - 1].tolist() == [1]
    assert got["summary"]["vertices"] == nC and 0 < got["summary"]["edges"] <= int((whole["type"] == 1).sum())
    total = bed["mass"][:nC].astype(np.float64).sum()
    assert abs(got["mass"].sum() - total) <= REL * total
    assert abs(got["mass"].sum() - ctx.inspect("clump_mass")) <= 1e-5 * total  # (the fp32 inspector)


@pytest.mark.gpu
def test_bed_at_thresholds_inside_the_force_distribution(pkg, bed):
    """Thresholds between two neighbours of the sorted |f| at the 60th and the 90th percentile.  One step after the bed was lowered
    its 509 sphere-sphere forces lie between 6.6 N and 546 N without a gap: no threshold in there keeps every |f| a factor 2 away
    (no_force_near).  What that rule protects still holds and is asserted: the device and the model make the same fp64 comparison
    of the same fp32 records with the same fp32 threshold, and no |f| is within 1e-5 of it (an fp32 rounding is 6e-8).  The
    factor-2 rule is asserted where the bed allows it: at a threshold in the widest gap of the distribution."""
    ctx, whole = bed["ctx"], bed["whole"]
    all_edges = model(bed)["summary"]["edges"]
    seen = []
    for q in (0.6, 0.9):
        thr, nearest = threshold_at(whole, q)
        assert nearest > 1e-5, (q, thr, nearest)
        want = model(bed, thr)
        seen.append(want["summary"])
        check(ctx.inspect_clusters(thr), want, f"{bed['mode']}, threshold {thr:.4e} at the {q:.0%} quantile")
        assert abs(want["summary"]["edges"] - (1 - q) * all_edges) < 0.05 * all_edges
    print(seen)
    for s in seen:  # no trivial partition: several clusters, one of them larger than 1
        assert s["clusters"] > 1 and s["largestSize"] > 1 and s["singletons"] > 0, s
    thr = threshold_gap(whole)
    if no_force_near(whole, thr):
        check(ctx.inspect_clusters(thr), model(bed, thr), f"{bed['mode']}, threshold {thr:.4e} in the widest gap")
    else:
        print(f"{bed['mode']}: the widest gap of the forces is narrower than a factor 4; no threshold with every |f| a factor 2 away")


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_is_one_cluster_labelled_zero(pkg, chain):
    ctx, sc, perm = chain["ctx"], chain["sc"], chain["perm"]
    n = int(sc.nOwnerClumps)
    assert n == N_CHAIN and n % 256 != 0 and int(sc.nOwners) == n
    a, b = edges_of(chain["whole"], _owner_tables(sc), np.ones(n, bool), THR)
    assert len(a) == n - 1 > 8 * 256  # more than 8 workgroups of the link kernel
    along = np.argsort(perm)  # position of every id
    assert (np.abs(along[a] - along[b]) == 1).all()  # neighbours only: a path
    got = ctx.inspect_clusters(THR)
    check(got, model(chain), f"{chain['mode']}, the chain")
    assert (got["labels"] == 0).all()
    assert got["summary"] == {"vertices": n, "edges": n - 1, "clusters": 1, "singletons": 0, "largestSize": n, "largestLabel": 0}
    assert got["label"].tolist() == [0] and got["size"].tolist() == [n]  # one row out of the final pass's partials
    print(f"{chain['mode']}: {ctx.clusters_link_retries()} compare-and-swaps lost in the link pass")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_cut_chain_is_four_clusters_with_known_minima(pkg, mode):
    p, sc, perm = chain_scene(pkg, CUTS)
    ctx = _stepped(pkg, p, sc, mode)
    s = setup(pkg, ctx, p, sc, mode)
    got = ctx.inspect_clusters(THR)
    check(got, model(s), f"{mode}, the cut chain")
    segments = np.split(perm, CUTS)
    minima = sorted(int(seg.min()) for seg in segments)
    assert got["label"].tolist() == minima and sorted(got["size"].tolist()) == sorted(len(seg) for seg in segments)
    for seg in segments:
        assert (got["labels"][seg] == seg.min()).all()
    assert got["summary"]["edges"] == N_CHAIN - 4 and got["summary"]["clusters"] == 4 and got["summary"]["largestSize"] == max(map(len, segments))
    ctx.close()


# ---- many small clusters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_many_small_clusters_and_the_row_count_protocol(pkg, mode):
    X, cells = small_clusters_positions()
    p, sc = spheres_scene(pkg, X, (0.1, 0.1, 0.02))
    ctx = _stepped(pkg, p, sc, mode)
    s = setup(pkg, ctx, p, sc, mode)
    got = ctx.inspect_clusters(THR)
    check(got, model(s), f"{mode}, small clusters")
    n_cells = int(cells.max()) + 1
    want_labels = np.array([np.flatnonzero(cells == c).min() for c in range(n_cells)])[cells]
    assert np.array_equal(got["labels"], want_labels)
    assert got["summary"]["clusters"] == n_cells == 324 and got["summary"]["singletons"] == 108 and got["summary"]["largestSize"] == 3
    assert got["summary"]["largestLabel"] == int(np.sort(np.unique(want_labels[np.bincount(cells)[cells] == 3]))[0])
    assert sorted(np.bincount(got["size"]).tolist()) == [0, 108, 108, 108]
    # the protocol: room for no row -- the count comes back, nothing is written, DEME_ERR_INVALID; the exact room succeeds
    lib = ctx.lib
    rows = C.c_size_t(12345)
    arrays = {k: np.full(n_cells * w, 0xAB, np.uint8).repeat(np.dtype(dt).itemsize) for k, (dt, w) in pkg.abi.CLUSTER_COLUMN_SHAPES.items()}
    cols = pkg.abi.DemeClusterColumns(*[arrays[k].ctypes.data for k in COLUMNS])
    before = ctx.query_host_bytes()
    assert lib.deme_inspect_clusters(ctx.h, THR, None, None, 0, C.byref(cols), 0, C.byref(rows)) == 1
    assert rows.value == n_cells and all((a == 0xAB).all() for a in arrays.values()) and "rows" in lib.deme_last_error(ctx.h).decode()
    assert ctx.query_host_bytes() - before == HEAD_BYTES
    rows = C.c_size_t(0)
    assert lib.deme_inspect_clusters(ctx.h, THR, None, None, 0, None, 0, C.byref(rows)) == 0 and rows.value == n_cells  # the count alone
    assert lib.deme_inspect_clusters(ctx.h, THR, None, None, 0, C.byref(cols), n_cells - 1, C.byref(rows)) == 1
    assert all((a == 0xAB).all() for a in arrays.values())
    assert lib.deme_inspect_clusters(ctx.h, THR, None, None, 0, C.byref(cols), n_cells, C.byref(rows)) == 0 and rows.value == n_cells
    for k, (dt, w) in pkg.abi.CLUSTER_COLUMN_SHAPES.items():
        assert arrays[k].view(dt).reshape(got[k].shape).tobytes() == got[k].tobytes(), k
    ctx.close()


# ---- determinism, bytes, read-only, refusals ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_calls_give_the_same_bits(bed, chain):
    for s in (bed, chain):
        a, b = s["ctx"].inspect_clusters(THR), s["ctx"].inspect_clusters(THR)
        assert a["summary"] == b["summary"]
        for k in ("labels",) + COLUMNS:
            assert a[k].tobytes() == b[k].tobytes() and a[k].size, k


@pytest.mark.gpu
def test_bytes_that_come_to_the_host(pkg, bed):
    ctx, nO = bed["ctx"], int(bed["sc"].nOwners)
    rows = ctx.inspect_clusters(THR)["summary"]["clusters"]
    for summary, labels, table in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        before = ctx.query_host_bytes()
        ctx.inspect_clusters(THR, summary=summary, labels=labels, table=table)
        want = HEAD_BYTES + (SUMMARY_BYTES if summary else 0) + (4 * nO if labels else 0) + (rows * sum(ROW_BYTES.values()) if table else 0)
        assert ctx.query_host_bytes() - before == want, (summary, labels, table)
    # one column of the table
    mass = np.zeros(rows)
    cols = pkg.abi.DemeClusterColumns()
    cols.mass = mass.ctypes.data
    n = C.c_size_t(0)
    before = ctx.query_host_bytes()
    assert ctx.lib.deme_inspect_clusters(ctx.h, THR, None, None, 0, C.byref(cols), rows, C.byref(n)) == 0
    assert ctx.query_host_bytes() - before == HEAD_BYTES + 8 * rows and mass.min() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_the_inspector_changes_nothing(pkg, mode):
    """step, ask, step, 40 times: the state and the list afterwards are those of a twin context that never asked"""
    p, sc, mid = _bed_scene(pkg)
    ctx, ref = _stepped(pkg, p, sc, mode, steps=1), _stepped(pkg, p, sc, mode, steps=1)
    for k in range(40):
        got = ctx.inspect_clusters(THR if k % 2 else 1e-3)
        assert got["summary"]["vertices"] == int(sc.nOwnerClumps)
        for c in (ctx, ref):
            c.step(1)
    ctx.sync(), ref.sync()
    assert ctx.counts().nDetections == ref.counts().nDetections and ctx.counts().nSteps == 41
    a, r = ctx.download_state(), ref.download_state()
    assert all(np.array_equal(a[k], r[k]) for k in a)
    la, lr = _whole_list(ctx, sc), _whole_list(ref, sc)
    for k in la:
        assert np.array_equal(la[k].view(np.uint32) if la[k].dtype == np.float32 else la[k],
                              lr[k].view(np.uint32) if lr[k].dtype == np.float32 else lr[k]), k
    for w in range(int(p.nContactWildcards)):
        assert np.array_equal(ctx.wildcard(w).view(np.uint32), ref.wildcard(w).view(np.uint32)), w
    ctx.close(), ref.close()


def raw_call(pkg, fn, handle, last_error, n_owners, thr, ask=("summary", "labels", "table", "rows"), label_cap=None):
    """the C call with sentinel-filled outputs: (rc, every output untouched, message)"""
    summ = np.full(48, 0xAB, np.uint8)
    labels = np.full(4 * max(n_owners, 1), 0xAB, np.uint8)
    arrays = {k: np.full(max(n_owners, 1) * w, 0xAB, np.uint8).repeat(np.dtype(dt).itemsize) for k, (dt, w) in pkg.abi.CLUSTER_COLUMN_SHAPES.items()}
    cols = pkg.abi.DemeClusterColumns(*[arrays[k].ctypes.data for k in COLUMNS])
    rows = np.full(8, 0xAB, np.uint8)
    rc = fn(handle, thr, C.cast(summ.ctypes.data, C.POINTER(pkg.abi.DemeClusterSummary)) if "summary" in ask else None,
            labels.ctypes.data if "labels" in ask else None, n_owners if label_cap is None else label_cap,
            C.byref(cols) if "table" in ask else None, n_owners, C.cast(rows.ctypes.data, C.POINTER(C.c_size_t)) if "rows" in ask else None)
    untouched = all(bool((a == 0xAB).all()) for a in (summ, labels, rows, *arrays.values()))
    return rc, untouched, last_error(handle).decode()


@pytest.mark.gpu
def test_refusals(pkg, bed):
    """every refusal of the header in its order, nothing written and no byte counted -- but the last one: a list of 2^31 rows does
    not fit a device.  Each case also breaks every later rule it can."""
    ctx, lib, nO = bed["ctx"], bed["ctx"].lib, int(bed["sc"].nOwners)

    def call(c, **over):
        before = c.query_host_bytes()
        rc, untouched, msg = raw_call(pkg, lib.deme_inspect_clusters, c.h, lib.deme_last_error, nO, **{"thr": THR, **over})
        return rc, untouched, msg, c.query_host_bytes() - before

    rc, untouched, _, nbytes = call(ctx)
    assert rc == 0 and not untouched and nbytes > 0
    for what, word, over in (("every output null", "null output", {"ask": (), "label_cap": 0, "thr": -1.0}),
                             ("too few labels", "too small", {"label_cap": nO - 1, "thr": float("nan")}),
                             ("a negative threshold", "threshold", {"thr": -1.0}),
                             ("a threshold that is not finite", "threshold", {"thr": float("inf")})):
        rc, untouched, msg, nbytes = call(ctx, **over)
        assert rc == 1 and untouched and word in msg and nbytes == 0, (what, msg)
    assert call(ctx, ask=("summary",), label_cap=0)[0] == 0  # labelCap is looked at only when labels are asked
    # recording off, then a seeded list: the messages of the records download; the arguments are refused before the context is
    p, sc2, mid = _bed_scene(pkg)
    off = _stepped(pkg, p, sc2, bed["mode"], record=False)
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    want_msg = lib.deme_last_error(off.h).decode()
    assert "recording is off" in want_msg
    for ask in (("summary",), ("labels",), ("rows",), ("summary", "labels", "table", "rows")):
        rc, untouched, msg, nbytes = call(off, ask=ask)
        assert rc == 1 and untouched and msg == want_msg and nbytes == 0, ask
    rc, untouched, msg, nbytes = call(off, thr=-1.0)
    assert rc == 1 and untouched and "threshold" in msg
    off.set_record_contacts(True)
    a, b, t, _ = off.contacts()
    W = np.stack([off.wildcard(w) for w in range(int(p.nContactWildcards))], 1) if p.nContactWildcards else None
    off.seed_contacts(a, b, t, W)
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    want_msg = lib.deme_last_error(off.h).decode()
    assert "seed" in want_msg
    rc, untouched, msg, nbytes = call(off)
    assert rc == 1 and untouched and msg == want_msg and nbytes == 0
    off.step(1)
    off.sync()
    assert call(off)[0] == 0  # evaluated again: it answers
    off.close()
