"""deme_inspect_fields (Context.inspect_fields): per-cell sums on a grid -- clumps, mass, volume, momentum, the kinetic tensor, the
counted sides and the virial -- summed on the device, against tests/_fields64.py applied to the downloaded owner state, the
whole-list downloads and the scene's tables.

The bed is that of tests/test_owner_contacts.py, stepped as tests/test_contact_inspect.py steps it: 300 three-sphere clumps lowered
onto the floor of their box, the last clump left where the lattice put it.

Tolerance of a double: |got - model| <= 1e-10 * abs_sum per entry, abs_sum the sum of |term| over the cell's terms.  It is derived,
as in tests/test_tri_loads.py: both sides add the same fp64 terms in different orders, so the difference is at most
n * 1.1e-16 * abs_sum, and the tests assert n < 1e5 terms per cell (the one-cell grid of the 40 000-clump bed holds more and
asserts n * 1.1e-16 <= 1e-10 instead: see there).  (A term itself has the same bits on both sides up to the few
roundings of the rotation, each 1.1e-16 of the term.)  The integers are compared for equality."""
import ctypes as C

import numpy as np
import pytest

from tests._contact_sums64 import contact_sums
from tests._fields64 import cells_of, fields, positions
from tests.test_owner_contacts import _bed_scene, _owner_tables, _stepped, _whole_list

THR = 1e-12  # what the shell passes (DEME_TINY_FLOAT_HOST)
REL = 1e-10
SYMBOLS = ("deme_inspect_fields", "deme_multi_inspect_fields", "deme_fields_block_rows")
OWNER_COLUMNS = ("clumps", "mass", "volume", "momentum", "kinetic")
CONTACT_COLUMNS = ("sides", "virial")
BYTES = {"clumps": 4, "mass": 8, "volume": 8, "momentum": 24, "kinetic": 48, "sides": 4, "virial": 72}
MAX_CELLS = 1 << 21


def test_field_inspector_is_exported_and_bound(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in SYMBOLS:
        assert n in names and hasattr(lib, n), n
    for cls in (pkg.Context, pkg.abi.Multi):
        assert hasattr(cls, "inspect_fields"), cls.__name__
    assert len(lib.deme_inspect_fields.argtypes) == 4 and len(lib.deme_multi_inspect_fields.argtypes) == 4
    assert C.sizeof(pkg.abi.DemeFieldGrid) == 64 and C.sizeof(pkg.abi.DemeFieldColumns) == 56
    assert pkg.abi.FIELD_COLUMNS == OWNER_COLUMNS + CONTACT_COLUMNS
    assert pkg.abi.fields_block_rows() == 256


class _Params:  # positions are multiples of 2^-10: every face below is met exactly
    nvXp2, nvYp2, voxelSize, l = 4, 4, 64.0, 2.0 ** -10
    LBFX = LBFY = LBFZ = 0.0


def test_the_model_on_a_hand_written_state(pkg):
    """five owners -- a clump inside cell 0, one exactly on the lower face of cell 1, one exactly on the grid's upper face, a ghost
    copy beside the first, a mesh owner -- and six rows, one of them below the threshold"""
    P = np.array([[0.25, 0.25, 0.25], [0.5, 0.25, 0.25], [1.0, 0.25, 0.25], [0.25, 0.25, 0.25], [0.25, 0.25, 0.25]])
    vid, lx, ly, lz = pkg.model.encode_positions(P, 4, 4, 64.0, 2.0 ** -10)
    one, zero = np.ones(5, np.float32), np.zeros(5, np.float32)
    state = {"voxelID": vid, "locX": lx, "locY": ly, "locZ": lz, "oriQw": one, "oriQx": zero, "oriQy": zero, "oriQz": zero,
             "vX": np.array([1, 2, 3, 4, 5], np.float32), "vY": np.array([0, -1, 0, 0, 0], np.float32), "vZ": zero}
    X = positions(pkg.model.decode_positions, _Params, state)
    assert np.array_equal(X, P)
    own = np.array([True, True, True, False, False])  # the ghost and the mesh owner are no own clumps
    mass = np.array([2, 3, 5, 7, 11], np.float32)
    vol = np.array([0.5, 0.25, 1, 1, 1], np.float32)
    # spheres 0..3 belong to owners 0..3, triangle 0 and component 0 to owner 4
    tables = (np.arange(4, dtype=np.uint32), np.array([4], np.uint32), np.array([4], np.uint32))
    whole = {"idA": np.array([0, 0, 1, 0, 1, 1], np.uint32), "idB": np.array([1, 2, 3, 0, 0, 0], np.uint32),
             "type": np.array([1, 1, 1, 2, 1, 3], np.uint8),
             "force": np.array([[1, 0, 0], [0, 2, 0], [0, 0, 4], [8, 0, 0], [1e-3, 0, 0], [0, 0, 16]], np.float32),
             "cpA": np.array([[1, 2, 3]] * 6, np.float32), "cpB": np.array([[-1, 0, 1]] * 6, np.float32)}
    m = fields(X, state, own, mass, vol, (0, 0, 0), (0.5, 0.5, 0.5), (2, 2, 2), whole, tables, 0.01)
    assert m["cell_of"].tolist() == [0, 1, 8, 8, 8]  # lower face: in the cell; the grid's upper face, the ghost, the mesh: out
    assert m["clumps"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and m["clumps"].dtype == np.uint32
    assert m["mass"][:2].tolist() == [2, 3] and m["volume"][:2].tolist() == [0.5, 0.25] and not m["mass"][2:].any()
    assert m["momentum"][:2].tolist() == [[2, 0, 0], [6, -3, 0]]
    assert m["kinetic"][1].tolist() == [12, 3, 0, -6, 0, 0] and m["abs_kinetic"][1].tolist() == [12, 3, 0, 6, 0, 0]
    # rows 0, 1, 3 carry owner 0 on side A; row 0 owner 1 on side B, rows 2 and 5 on side A; row 4 is below the threshold; the
    # sides of owners 2 (outside), 3 (ghost) and 4 (mesh, plane) are never counted
    assert m["sides"].tolist() == [3, 3, 0, 0, 0, 0, 0, 0]
    assert [s.tolist() for s in m["side_cells"]] == [[0, 0, 1, 0, 8, 1], [1, 8, 8, 8, 8, 8]]
    assert m["virial"][0].reshape(3, 3).tolist() == [[9, 2, 0], [18, 4, 0], [27, 6, 0]]  # (1, 2, 3) (x) (1 + 8, 2, 0)
    assert m["virial"][1].reshape(3, 3).tolist() == [[1, 0, 20], [0, 0, 40], [-1, 0, 60]]  # (-1, 0, 1) (x) (-1, 0, 0) + (1, 2, 3) (x) (0, 0, 20)
    assert m["abs_virial"][1].reshape(3, 3).tolist() == [[1, 0, 20], [0, 0, 40], [1, 0, 60]]
    m0 = fields(X, state, own, mass, None, (0, 0, 0), (0.5, 0.5, 0.5), (2, 2, 2), whole, tables, 0.0)
    assert m0["sides"].tolist() == [4, 4, 0, 0, 0, 0, 0, 0] and "volume" not in m0
    nan = X.copy()
    nan[0, 1] = np.nan
    assert cells_of(nan, (0, 0, 0), (0.5, 0.5, 0.5), (2, 2, 2))[0].tolist() == [False, True, False, True, True]  # (geometry alone)


# ---- the bed on the device ------------------------------------------------------------------------------------------------------------
def _tables_of(sc):
    """per owner: mass of its mass-property entry; the volume table the tests upload (distinct values, one per entry)"""
    keep = sc._keep
    off = np.asarray(keep["inertiaPropOffsets"], np.int64)
    volumes = (1e-7 * (1.0 + np.arange(int(sc.nMassProps)))).astype(np.float32)
    return np.asarray(keep["MassProperties"], np.float32)[off], volumes[off], volumes


def _model(pkg, bed, grid, thr=THR, contacts=True):
    sc = bed["sc"]
    own = np.arange(int(sc.nOwners)) < int(sc.nOwnerClumps)
    return fields(bed["X"], bed["state"], own, bed["mass"], bed["volume"], *grid, bed["whole"] if contacts else None, _owner_tables(sc), thr)


def _setup(pkg, ctx, p, sc, mode):
    mass, volume, table = _tables_of(sc)
    ctx.upload_volumes(table)
    state = ctx.download_state()
    return {"ctx": ctx, "p": p, "sc": sc, "mode": mode, "whole": _whole_list(ctx, sc), "state": state, "mass": mass, "volume": volume,
            "X": positions(pkg.model.decode_positions, p, state)}


@pytest.fixture(scope="module", params=["fast", "exact"])
def bed(pkg, request):
    p, sc, mid = _bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, request.param)
    yield _setup(pkg, ctx, p, sc, request.param)
    ctx.close()


def grids(bed):
    """name -> (origin, cell, n).  The pads are no round numbers of the position grid, so that no centre falls on a face."""
    nC = int(bed["sc"].nOwnerClumps)
    X = bed["X"][:nC]
    lo, hi = X.min(0) - 1.2345e-4, X.max(0) + 2.3456e-4
    settled = X[:nC - 1]  # (the last clump hangs above the bed)
    blo, bhi = settled.min(0) - 1.2345e-4, settled.max(0) + 2.3456e-4
    zmid = float(np.median(settled[:, 2])) + 1.0e-7
    return {
        "one cell around everything": (lo, hi - lo, (1, 1, 1)),
        "4 x 4 x 3 over the bed": (blo, (bhi - blo) / (4, 4, 3), (4, 4, 3)),
        "16 x 16 x 16": (lo, (hi - lo) / 16, (16, 16, 16)),
        "the lower half": (blo, np.array([bhi[0] - blo[0], bhi[1] - blo[1], zmid - blo[2]]) / (3, 3, 2), (3, 3, 2)),
        "beside the bed": (hi + 1.0, (hi - lo) / 4, (4, 4, 4)),
    }


def check(got, want, what, columns=OWNER_COLUMNS + CONTACT_COLUMNS, max_terms=1e5):
    for k in columns:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        if got[k].dtype == np.uint32:
            assert np.array_equal(got[k], want[k]), (what, k)
            continue
        err, bound = np.abs(got[k] - want[k]), REL * want["abs_" + k]
        print(f"{what}, {k}: max |got - model| {err.max():.3e}, max abs_sum {want['abs_' + k].max():.3e}, "
              f"worst ratio {(err / np.maximum(want['abs_' + k], 1e-300)).max():.3e}")
        assert (err <= bound).all(), (what, k, float(err.max()))
    assert want["terms_owner"].max() < max_terms and ("terms_side" not in want or want["terms_side"].max() < max_terms)


@pytest.mark.gpu
def test_every_column_equals_the_model(pkg, bed):
    ctx = bed["ctx"]
    for what, grid in grids(bed).items():
        want = _model(pkg, bed, grid)
        got = ctx.inspect_fields(*grid, force_threshold=THR)
        assert tuple(got) == OWNER_COLUMNS + CONTACT_COLUMNS
        check(got, want, f"{bed['mode']}, {what}")
        if what == "beside the bed":
            assert not any(v.any() for v in got.values())
        else:
            assert got["clumps"].sum() > 0 and got["sides"].sum() > 0 and np.abs(got["virial"]).max() > 0 and got["kinetic"].max() > 0
            assert (got["volume"][got["clumps"] > 0] > 0).all() and not got["mass"][got["clumps"] == 0].any()


@pytest.mark.gpu
def test_grids_exercise_what_they_should(pkg, bed):
    sc, whole = bed["sc"], bed["whole"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    all_grids = grids(bed)
    for what, (origin, cell, n) in all_grids.items():
        u = (bed["X"][:nC] - origin) / cell
        assert np.abs(u - np.round(u)).min() > 1e-9, what  # no centre within 1e-9 of a cell of a face
    f = np.sqrt((whole["force"].astype(np.float64) ** 2).sum(1))
    assert not ((f > THR / 2) & (f < 2 * THR)).any()  # no row a rounding could move across the threshold
    coarse, fine, half = (_model(pkg, bed, all_grids[k]) for k in ("4 x 4 x 3 over the bed", "16 x 16 x 16", "the lower half"))
    assert coarse["clumps"].max() > 1  # some cell has several clumps; some cell of the fine grid has none
    assert int(coarse["clumps"].sum()) == nC - 1  # the hanging clump is outside the bed's box
    assert (fine["clumps"] == 0).any() and (fine["clumps"] <= 1).mean() > 0.5  # most cells hold no clump or one
    assert int(fine["clumps"].sum()) == nC
    assert 0 < int(half["clumps"].sum()) < nC - 1 and 0 < int(half["sides"].sum()) < int(coarse["sides"].sum())
    # some counted side's partner lies in another cell; sphere--plane rows are counted on side A only
    a, b = coarse["side_cells"]
    n_cells = len(coarse["clumps"])
    assert ((a < n_cells) & (b < n_cells) & (a != b)).any()
    plane = whole["type"] > 2
    assert plane.any() and (a[plane] < n_cells).any() and (b[plane] == n_cells).all()
    assert bed["ctx"].engine_order()[0] == (bed["mode"] == "fast")


@pytest.mark.gpu
def test_one_cell_agrees_with_the_merged_inspectors(pkg, bed):
    ctx, sc = bed["ctx"], bed["sc"]
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    grid = grids(bed)["one cell around everything"]
    got = ctx.inspect_fields(*grid, force_threshold=THR)
    sums = ctx.inspect_contacts(-1, THR)
    assert int(got["clumps"][0]) == sums["clumps"] == nC and int(got["sides"][0]) == sums["sides"] > 0
    model = contact_sums(bed["whole"], _owner_tables(sc), bed["state"], np.arange(nO) < nC, THR)
    assert (np.abs(got["virial"][0].reshape(3, 3) - sums["virial"]) <= REL * model["abs_sum"]).all() and sums["sides"] < 1e5
    total = bed["mass"][:nC].astype(np.float64).sum()
    assert abs(got["mass"][0] - total) <= REL * total
    assert abs(got["mass"][0] - ctx.inspect("clump_mass")) <= 1e-5 * total  # (the fp32 inspector)


@pytest.mark.gpu
def test_the_face_rule_on_the_device(pkg, bed):
    """a grid of one cell whose origin is clump P's centre and whose x edge is Q_x - P_x: u is 0.0 for P -- in -- and exactly 1.0
    for Q -- out; with the next double as the edge, Q is in"""
    ctx, nC = bed["ctx"], int(bed["sc"].nOwnerClumps)
    X = bed["X"][:nC - 1]
    pair = None
    for i in np.argsort(X.sum(1)):
        j = np.flatnonzero((X[:, 0] > X[i, 0]) & (X[:, 1] >= X[i, 1]) & (X[:, 2] >= X[i, 2]))
        if len(j):
            pair = (int(i), int(j[0]))
            break
    assert pair is not None
    P, Q = X[pair[0]], X[pair[1]]
    edge = np.array([Q[0] - P[0], Q[1] - P[1] + 1.0, Q[2] - P[2] + 1.0])
    assert (P + edge)[1] > Q[1] and (P + edge)[2] > Q[2] and (Q[0] - P[0]) / edge[0] == 1.0
    for what, e0, q_in in (("the face", edge[0], False), ("one ulp wider", np.nextafter(edge[0], np.inf), True)):
        grid = (P, np.array([e0, edge[1], edge[2]]), (1, 1, 1))
        want = _model(pkg, bed, grid)
        assert want["cell_of"][pair[0]] == 0 and (want["cell_of"][pair[1]] == 0) == q_in, what
        got = ctx.inspect_fields(*grid, columns=("clumps", "mass"), force_threshold=THR)
        check(got, want, f"{bed['mode']}, {what}", ("clumps", "mass"))
        assert int(got["clumps"][0]) >= (2 if q_in else 1)


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(bed):
    grid = grids(bed)["4 x 4 x 3 over the bed"]
    a = bed["ctx"].inspect_fields(*grid, force_threshold=THR)
    b = bed["ctx"].inspect_fields(*grid, force_threshold=THR)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() and a[k].any(), k


@pytest.mark.gpu
def test_bytes_that_come_to_the_host(bed):
    ctx = bed["ctx"]
    grid = grids(bed)["4 x 4 x 3 over the bed"]
    for columns in [(k,) for k in BYTES] + [("clumps", "virial"), tuple(BYTES)]:
        before = ctx.query_host_bytes()
        ctx.inspect_fields(*grid, columns=columns, force_threshold=THR)
        assert ctx.query_host_bytes() - before == 48 * sum(BYTES[k] for k in columns), columns


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_owner_columns_alone_need_no_records(pkg, mode):
    p, sc, mid = _bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, mode, record=False)
    # (the whole list cannot be downloaded: recording is off)
    mass, volume, table = _tables_of(sc)
    ctx.upload_volumes(table)
    state = ctx.download_state()
    bed = {"sc": sc, "X": positions(pkg.model.decode_positions, p, state), "state": state, "mass": mass, "volume": volume, "whole": None}
    grid = grids(bed)["4 x 4 x 3 over the bed"]
    got = ctx.inspect_fields(*grid, columns=OWNER_COLUMNS)
    check(got, _model(pkg, bed, grid, contacts=False), f"{mode}, recording off", OWNER_COLUMNS)
    assert got["clumps"].sum() == int(sc.nOwnerClumps) - 1
    for k in CONTACT_COLUMNS:
        with pytest.raises(pkg.abi.DemeError, match="recording is off"):
            ctx.inspect_fields(*grid, columns=("clumps", k))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_the_inspector_changes_nothing(pkg, mode):
    """step, ask, step 40 times: the state and the list afterwards are those of a twin context that never asked"""
    p, sc, mid = _bed_scene(pkg)
    ctx, ref = _stepped(pkg, p, sc, mode, steps=1), _stepped(pkg, p, sc, mode, steps=1)
    bed = _setup(pkg, ctx, p, sc, mode)
    for grid in grids(bed).values():
        ctx.inspect_fields(*grid, force_threshold=THR)
    for c in (ctx, ref):
        c.step(40)
        c.sync()
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


def _raw_call(pkg, fn, handle, last_error, origin, cell, n, thr, ask, null_grid=False, null_columns=False):
    """the C call with sentinel-filled arrays of 8 cells: (rc, every array untouched, message)"""
    grid = pkg.abi.DemeFieldGrid((C.c_double * 3)(*origin), (C.c_double * 3)(*cell), (C.c_uint32 * 3)(*n))
    cols, arrays = pkg.abi.DemeFieldColumns(), {}
    for k in ask:
        dtype, width = pkg.abi.FIELD_COLUMN_SHAPES[k]
        arrays[k] = np.full(8 * width, 0xAB, np.uint8).repeat(np.dtype(dtype).itemsize)
        setattr(cols, k, arrays[k].ctypes.data)
    rc = fn(handle, None if null_grid else C.byref(grid), thr, None if null_columns else C.byref(cols))
    return rc, all(bool((a == 0xAB).all()) for a in arrays.values()), last_error(handle).decode()


REFUSALS = (  # what, message word, overrides -- in the order of the header; each also breaks every later rule it can
    ("a null grid", "grid", {"null_grid": True, "cell": (0.0, 1.0, 1.0)}),
    ("null columns", "columns", {"null_columns": True, "n": (0, 1, 1)}),
    ("an origin that is not finite", "finite", {"origin": (float("nan"), 0.0, 0.0), "cell": (-1.0, 1.0, 1.0)}),
    ("an infinite cell edge", "finite", {"cell": (1.0, float("inf"), 1.0), "n": (0, 2, 2)}),
    ("a cell edge of zero", "> 0", {"cell": (1.0, 1.0, 0.0), "n": (2, 0, 2)}),
    ("a negative cell edge", "> 0", {"cell": (-1.0, 1.0, 1.0), "n": (4096, 4096, 4096)}),
    ("no cells along y", "cells", {"n": (2, 0, 2), "ask": ()}),
    ("more than 2^21 cells", "at most", {"n": (128, 128, 129), "ask": ()}),
    ("counts whose product overflows", "at most", {"n": (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), "thr": -1.0}),
    ("every column null", "null output", {"ask": (), "thr": -1.0}),
    ("a negative threshold", "threshold", {"thr": -1.0}),
    ("a threshold that is not finite", "threshold", {"thr": float("nan")}),
)


@pytest.mark.gpu
def test_refusals(pkg, bed):
    """every refusal of the header in its order, the arrays left as they were -- but the last one: a list of 2^31 rows does not fit
    a device"""
    ctx, lib = bed["ctx"], bed["ctx"].lib
    base = {"origin": (0.0, 0.0, 0.0), "cell": (1.0, 1.0, 1.0), "n": (2, 2, 2), "thr": THR, "ask": tuple(BYTES)}

    def call(c, **over):
        return _raw_call(pkg, lib.deme_inspect_fields, c.h, lib.deme_last_error, **{**base, **over})

    rc, untouched, _ = call(ctx)
    assert rc == 0 and not untouched
    for what, word, over in REFUSALS:
        rc, untouched, msg = call(ctx, **over)
        assert rc == 1 and untouched and word in msg, (what, msg)
    rc, untouched, _ = call(ctx, n=(128, 128, 128), cell=(1e-3, 1e-3, 1e-3), ask=())  # 2^21 cells: not the cap's refusal
    assert rc == 1 and "null output" in lib.deme_last_error(ctx.h).decode()
    with pytest.raises(pkg.abi.DemeError, match="at most"):
        ctx.inspect_fields((0, 0, 0), (1, 1, 1), (4096, 4096, 4096))
    with pytest.raises(ValueError):
        ctx.inspect_fields((0, 0, 0), (1, 1, 1), (2, 2, 2), columns=("pressure",))
    # volume without uploaded volumes (the message of clump_volume), then recording off and a seeded list (records_refused)
    p, sc2, mid = _bed_scene(pkg)
    off = _stepped(pkg, p, sc2, bed["mode"], record=False)
    with pytest.raises(pkg.abi.DemeError):
        off.inspect("clump_volume")
    want_msg = lib.deme_last_error(off.h).decode()
    assert "deme_upload_volumes" in want_msg
    rc, untouched, msg = call(off)  # (volume is refused before the records are)
    assert rc == 1 and untouched and msg == want_msg
    rc, untouched, msg = call(off, ask=("clumps", "mass"))
    assert rc == 0 and not untouched
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    want_msg = lib.deme_last_error(off.h).decode()
    assert "recording is off" in want_msg
    for ask in (("clumps", "sides"), ("virial",)):
        rc, untouched, msg = call(off, ask=ask)
        assert rc == 1 and untouched and msg == want_msg
    off.set_record_contacts(True)
    a, b, t, _ = off.contacts()
    W = np.stack([off.wildcard(w) for w in range(int(p.nContactWildcards))], 1) if p.nContactWildcards else None
    off.seed_contacts(a, b, t, W)
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    want_msg = lib.deme_last_error(off.h).decode()
    assert "seed" in want_msg
    rc, untouched, msg = call(off, ask=("clumps", "sides", "virial"))
    assert rc == 1 and untouched and msg == want_msg
    assert call(off, ask=("clumps", "kinetic"))[0] == 0  # the owner columns do not look at the list
    off.step(1)
    off.sync()
    assert call(off, ask=("sides",))[0] == 0  # evaluated again: it answers
    off.close()


@pytest.mark.gpu
def test_more_partials_than_the_second_stage_has_threads(pkg):
    """40 000 clumps of the packed bed of tests/test_contact_inspect.py's larger case: more than 32 768 owners and more than
    16 384 rows, so both final passes see more than 256 partials -- in one cell, a single run through every block, and on 8 x 8 x 4.
    This bed lists 89 641 rows after 5 steps and its one cell holds 168 319 counted sides: more than the 1e5 terms a cell the other
    tests assert, so the one-cell grid asserts what the bound's derivation needs, n * 1.1e-16 <= 1e-10 (n <= 909 090); the
    8 x 8 x 4 grid keeps n < 1e5.  The bound itself is the same 1e-10 * abs_sum."""
    COUNTS = ("nOwners", "nOwnerClumps", "nSpheres", "nAnal", "nTri", "nMat", "nComp", "nMassProps")
    b = pkg.model.packed_bed(40_000, seed=4, cd_freq=7, spacing_mult=2.4, init_vz=-0.4, aspect=(2.0, 1.0, 0.5))
    b.SetExpandSafetyAdder(0.5)
    p, sc = b.Initialize()
    arr = {k: np.array(v, copy=True) for k, v in sc._keep.items()}
    counts = {k: int(getattr(sc, k)) for k in COUNTS}
    nC = counts["nOwnerClumps"]
    X = pkg.model.decode_positions(arr["voxelID"], arr["locX"], arr["locY"], arr["locZ"], p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    X[:nC - 1, 2] -= (X[:nC, 2].min() + p.LBFZ) - 0.0045
    arr["voxelID"], arr["locX"], arr["locY"], arr["locZ"] = pkg.model.encode_positions(X, p.nvXp2, p.nvYp2, p.voxelSize, p.l)
    sc = pkg.abi.make_scene_struct(arr, counts)
    ctx = _stepped(pkg, p, sc, "exact", steps=5)
    bed = _setup(pkg, ctx, p, sc, "exact")
    rows = pkg.abi.fields_block_rows()
    assert nC > 32768 and 2 * ((nC + rows - 1) // rows) > 256
    n = len(bed["whole"]["idA"])
    assert n > 16384 and 2 * ((2 * n + rows - 1) // rows) > 256
    lo, hi = bed["X"][:nC].min(0) - 1.2345e-4, bed["X"][:nC].max(0) + 2.3456e-4
    for what, shape, max_terms in (("one cell", (1, 1, 1), REL / 1.1e-16), ("8 x 8 x 4", (8, 8, 4), 1e5)):
        grid = (lo, (hi - lo) / shape, shape)
        u = (bed["X"][:nC] - grid[0]) / grid[1]
        assert np.abs(u - np.round(u)).min() > 1e-9
        want = _model(pkg, bed, grid)
        print(f"{what}: most terms in a cell: {int(want['terms_owner'].max())} owners, {int(want['terms_side'].max())} sides")
        got = ctx.inspect_fields(*grid, force_threshold=THR)
        check(got, want, f"{nC} clumps, {n} rows, {what}", max_terms=max_terms)
        assert int(got["clumps"].sum()) == nC and int(got["sides"].sum()) > 0
        again = ctx.inspect_fields(*grid, force_threshold=THR)
        assert all(again[k].tobytes() == got[k].tobytes() for k in got)
    ctx.close()
