"""deme_multi_inspect_clusters (Multi.inspect_clusters) on 2 and 3 slabs of one device, exact mode: the bed of
tests/test_owner_contacts_multi.py after 60 steps, and the chain of tests/test_clusters.py laid along the decomposition axis, where
the one cluster crosses every cut and only the host's merge of the slabs' local trees can make it one.

The labels, the summary and the table's integers must equal the undivided run's.  The doubles are held to the bound of
tests/test_fields_multi.py against the per-slab model: tests/_clusters64.py applied to each slab context's own downloads (its owner
state, its list, its records) with the slab scene's tables -- the slab's clumps and ghost copies as vertices, its own clumps counted
--, the slabs' local trees united by global id and their rows added in slab order in fp64: |got - model| <= 1e-10 * abs_sum with
fewer than 1e5 terms per cluster."""
import ctypes as C

import numpy as np
import pytest

from tests._clusters64 import NONE, clusters, union_find
from tests._fields64 import positions
from tests.test_clusters import COLUMNS, HEAD_BYTES, REL, SUMMARY_BYTES, THR, chain_scene, raw_call, N_CHAIN
from tests.test_fields_multi import RECORDS, _table
from tests.test_owner_contacts import _stepped
from tests.test_owner_contacts_multi import HALO, STEPS, bed_scene, built

pytestmark = pytest.mark.gpu
CHAIN_HALO = 2.0e-3  # ten sphere radii of the chain


def slab_model(pkg, m, p, sc, n_slabs, halo, thr):
    """(the merged model: labels per global owner and the table with abs_moment; per slab (local owners, rows of its table))"""
    plan, parts = pkg.decomp.decompose_lib(p, sc, n_slabs, halo, axis=0, snap=True, spatial_order=True)
    nOG = int(sc.nOwners)
    pairs_a, pairs_b, slabs, vertex = [], [], [], np.zeros(nOG, bool)
    for s, pt in enumerate(parts):
        ctx, ssc = m.slab_ctx(s), pt["scene"]
        n_own = m.slab_counts(s)[0][0]
        gid = pt["owner_global"]
        assert n_own == pt["n_own"] and int(ssc.nOwners) == len(gid)
        state = ctx.download_state()
        a, b, t, _ = ctx.contacts()
        whole = {"idA": a, "idB": b, "type": t, **dict(zip(RECORDS, ctx.contact_records()))}
        tables = (_table(ssc, "ownerClumpBody", ssc.nSpheres), _table(ssc, "ownerMesh", ssc.nTri), _table(ssc, "objOwner", ssc.nAnal))
        off = _table(ssc, "inertiaPropOffsets", ssc.nOwners, np.uint16).astype(np.int64)
        mass = _table(ssc, "MassProperties", ssc.nMassProps, np.float32)[off]
        local = np.arange(int(ssc.nOwners))
        one = clusters(positions(pkg.model.decode_positions, p, state), mass, local < int(ssc.nOwnerClumps), whole, tables, thr,
                       counted=local < n_own)
        v = np.flatnonzero(one["labels"] != NONE)
        pairs_a.append(gid[v]), pairs_b.append(gid[one["labels"][v].astype(np.int64)])
        vertex[gid[v]] = True
        one["root_gid"] = gid[one["label"].astype(np.int64)]
        slabs.append(one)
    plan.close()
    root = union_find(nOG, np.concatenate(pairs_a), np.concatenate(pairs_b))
    labels = np.where(vertex, root, NONE).astype(np.uint32)
    size, mass = np.zeros(nOG, np.int64), np.zeros(nOG)
    moment, abs_moment = np.zeros((nOG, 3)), np.zeros((nOG, 3))
    for one in slabs:  # slab order, local roots ascending
        for k, g in enumerate(one["root_gid"]):
            l = root[g]
            size[l] += one["size"][k]
            mass[l] += one["mass"][k]
            moment[l] += one["moment"][k]
            abs_moment[l] += one["abs_moment"][k]
    rows = np.flatnonzero(size > 0)
    merged = {"labels": labels, "label": rows.astype(np.uint32), "size": size[rows].astype(np.uint32), "mass": mass[rows],
              "moment": moment[rows], "abs_moment": abs_moment[rows]}
    return merged, [(len(one["labels"]), len(one["label"])) for one in slabs]


def check(got, want, undivided, what, n_slabs):
    print(f"{what}: summary {got['summary']}")
    assert got["summary"] == undivided["summary"], (what, got["summary"], undivided["summary"])
    for k in ("labels", "label", "size"):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]) and np.array_equal(got[k], undivided[k]), (what, k)
    for k, abs_sum in (("mass", want["mass"]), ("moment", want["abs_moment"])):
        err = np.abs(got[k] - want[k])
        print(f"{what}, {k}: max |got - model| {err.max():.3e}, max abs_sum {abs_sum.max():.3e}, "
              f"worst ratio {(err / np.maximum(abs_sum, 1e-300)).max():.3e}")
        assert got[k].shape == want[k].shape and (err <= REL * abs_sum).all(), (what, k)
    assert int(want["size"].max()) + n_slabs < 1e5


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
    """the same bed undivided, exact mode: its integers are what the merged answer must equal"""
    p, sc = bed_scene(pkg)
    ctx = _stepped(pkg, p, sc, "exact", steps=STEPS)
    f = np.sqrt((ctx.contact_records()[0].astype(np.float64) ** 2).sum(1))
    assert not ((f > THR / 2) & (f < 2 * THR)).any()  # no row a rounding could move across the threshold
    yield ctx
    ctx.close()


def test_bed_equals_the_undivided_run_and_the_per_slab_model(pkg, run, single):
    m, p, sc, n_slabs = run["m"], run["p"], run["sc"], run["n_slabs"]
    nC = int(sc.nOwnerClumps)
    undivided = single.inspect_clusters(THR)
    want, per_slab = slab_model(pkg, m, p, sc, n_slabs, HALO, THR)
    before = m.query_host_bytes()
    got = m.inspect_clusters(THR)
    nbytes = m.query_host_bytes() - before
    check(got, want, undivided, f"the bed in {n_slabs} slabs", n_slabs)
    s = got["summary"]
    assert s["vertices"] == nC and s["clusters"] > 1 and s["largestSize"] > nC // 2 and s["singletons"] >= 1 and s["edges"] > 0
    assert got["labels"][nC - 1] == nC - 1 and (got["labels"][nC:] == NONE).all()  # the hanging clump; the box
    # a cluster reaches over every cut: some slab's local tree is smaller than the cluster it belongs to
    assert all(n_loc < int(sc.nOwners) for n_loc, _ in per_slab)
    assert nbytes == sum(HEAD_BYTES + SUMMARY_BYTES + 8 * n_loc + 40 * rows for n_loc, rows in per_slab)
    before = m.query_host_bytes()
    m.inspect_clusters(THR, summary=False, table=False)
    assert m.query_host_bytes() - before == sum(HEAD_BYTES + 8 * n_loc for n_loc, _ in per_slab)
    again = m.inspect_clusters(THR)
    assert again["summary"] == got["summary"] and all(again[k].tobytes() == got[k].tobytes() for k in ("labels",) + COLUMNS)


@pytest.mark.parametrize("n_slabs", [2, 3])
def test_chain_across_every_cut_is_one_cluster(pkg, n_slabs):
    p, sc, perm = chain_scene(pkg)
    single = _stepped(pkg, p, sc, "exact")
    undivided = single.inspect_clusters(THR)
    single.close()
    m = built(pkg, p, sc, n_slabs, halo=CHAIN_HALO)
    m.step(1)
    m.sync()
    want, per_slab = slab_model(pkg, m, p, sc, n_slabs, CHAIN_HALO, THR)
    got = m.inspect_clusters(THR)
    check(got, want, undivided, f"the chain in {n_slabs} slabs", n_slabs)
    n = N_CHAIN
    assert got["summary"] == {"vertices": n, "edges": n - 1, "clusters": 1, "singletons": 0, "largestSize": n, "largestLabel": 0}
    assert (got["labels"] == 0).all() and got["size"].tolist() == [n]
    # the chain crosses every cut: every slab owns a part of it and sees less than all of it
    for s in range(n_slabs):
        own = m.slab_counts(s)[0][0]
        assert 0 < own < n and per_slab[s][0] < n, (s, own)
    assert sum(m.slab_counts(s)[0][0] for s in range(n_slabs)) == n
    m.close()


def test_refusals(pkg, run):
    m, sc, n_slabs = run["m"], run["sc"], run["n_slabs"]
    lib, nO = m.lib, int(sc.nOwners)

    def call(mm, **over):
        before = mm.query_host_bytes()
        rc, untouched, msg = raw_call(pkg, lib.deme_multi_inspect_clusters, mm.h, lib.deme_multi_last_error, nO, **{"thr": THR, **over})
        return rc, untouched, msg, mm.query_host_bytes() - before

    rc, untouched, _, nbytes = call(m)
    assert rc == 0 and not untouched and nbytes > 0
    for what, word, over in (("every output null", "null output", {"ask": (), "label_cap": 0, "thr": -1.0}),
                             ("too few labels", "too small", {"label_cap": nO - 1, "thr": float("nan")}),
                             ("a negative threshold", "threshold", {"thr": -1.0}), ("a NaN threshold", "threshold", {"thr": float("nan")})):
        rc, untouched, msg, nbytes = call(m, **over)
        assert rc == 1 and untouched and word in msg and "deme_multi_inspect_clusters" in msg and nbytes == 0, (what, msg)
    # the table's protocol in global rows
    rows = C.c_size_t(0)
    assert lib.deme_multi_inspect_clusters(m.h, THR, None, None, 0, None, 0, C.byref(rows)) == 0
    assert rows.value == m.inspect_clusters(THR)["summary"]["clusters"]
    cols = pkg.abi.DemeClusterColumns()
    size = np.full(rows.value, 0xABABABAB, np.uint32)
    cols.size = size.ctypes.data
    assert lib.deme_multi_inspect_clusters(m.h, THR, None, None, 0, C.byref(cols), rows.value - 1, C.byref(rows)) == 1
    assert (size == 0xABABABAB).all() and "rows" in lib.deme_multi_last_error(m.h).decode()
    assert lib.deme_multi_inspect_clusters(m.h, THR, None, None, 0, C.byref(cols), rows.value, C.byref(rows)) == 0
    assert int(size.sum()) == int(sc.nOwnerClumps)
    # recording off on one slab: the words of the records call
    p, sc2 = bed_scene(pkg)
    off = built(pkg, p, sc2, n_slabs)
    off.slab_ctx(n_slabs - 1).set_record_contacts(False)
    off.step(STEPS)
    off.sync()
    with pytest.raises(pkg.abi.DemeError):
        off.contact_records()
    want_msg = lib.deme_multi_last_error(off.h).decode()
    assert "recording is off" in want_msg
    rc, untouched, msg, nbytes = call(off)
    assert rc == 1 and untouched and "recording is off" in msg and nbytes == 0
    off.close()
