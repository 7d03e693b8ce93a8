"""clusters_bench.py -- what one deme_inspect_clusters call costs beside the only other way to the same answer.

The scene is bench.py's flagship bed (bench.build_bed), fast mode, `settle` steps with contact recording on.  Two thresholds: the
shell's (1e-12) and the median |f| of the sphere-sphere rows.  Then, per threshold, with the host clock around each, a warm-up and 5
timed repeats of
  device   Context.inspect_clusters()                      (16 + 48 bytes, 4 an owner, 40 a cluster to the host)
  host     deme_download_owner_state + deme_download_contacts + deme_download_contact_records: what a script has to bring to the
           host today before it can unite anything (64 bytes an owner and 56 a row on the device's side)
and the median with min - max is printed in ms, with the time of the call's three passes from the library's event timers
(deme_kernel_time_ms), the compare-and-swaps the link pass lost, and, once, the host's union-find and sums (tests/_clusters64.py)
on the downloads with the comparison of the two answers.

  python tools/clusters_bench.py [n = 1000000] [settle = 200]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402
from tests._clusters64 import clusters  # noqa: E402
from tests._fields64 import positions  # noqa: E402


def report(what, v):
    v = sorted(v)
    print(f"{what} median {v[len(v) // 2]:.3f} ms ({v[0]:.3f} - {v[-1]:.3f})", flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    settle = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    pkg = entry.load_package()
    p, sc = bench.build_bed(pkg, n, 2024, 40).Initialize()
    ctx = pkg.Context(0)
    ctx.set_arith_mode("fast")
    ctx.set_params(p)
    ctx.upload_scene(sc)
    ctx.set_record_contacts(True)
    t0 = time.perf_counter()
    ctx.step(settle)
    ctx.sync()
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    rows = int(ctx.counts().nContacts)
    print(f"BED clumps={nC} settle_steps={settle} settle_s={time.perf_counter() - t0:.1f} contacts={rows}", flush=True)
    a, bb, t, _ = ctx.contacts()
    f = np.sqrt((ctx.contact_records()[0][t == 1].astype(np.float64) ** 2).sum(1))
    median = float(np.float32(np.median(f))) if len(f) else 0.0
    keep = sc._keep
    off = np.asarray(keep["inertiaPropOffsets"], np.int64)
    mass = np.asarray(keep["MassProperties"], np.float32).reshape(int(sc.nMassProps), -1)[:, 0][off]
    tables = (np.asarray(keep["ownerClumpBody"], np.uint32), np.asarray(keep.get("ownerMesh", np.zeros(0)), np.uint32),
              np.asarray(keep.get("objOwner", np.zeros(0)), np.uint32))
    ok = True
    for what, thr in (("the shell's threshold", 1e-12), ("the median force", median)):
        dev, dl = [], []
        got = whole = state = None
        for rep in range(6):
            before = ctx.query_host_bytes()
            t0 = time.perf_counter()
            got = ctx.inspect_clusters(thr)
            t1 = time.perf_counter()
            dev_bytes = ctx.query_host_bytes() - before
            state = ctx.download_state()
            a, bb, t, _ = ctx.contacts()
            rec = ctx.contact_records()
            t2 = time.perf_counter()
            whole = {"idA": a, "idB": bb, "type": t, "force": rec[0]}
            if rep:  # (the first repeat is the warm-up: scratch allocations, the caller's view of the list)
                dev.append(1e3 * (t1 - t0)), dl.append(1e3 * (t2 - t1))
        print(f"THRESHOLD {thr:.6g} ({what}): {got['summary']}, link retries {ctx.clusters_link_retries()}", flush=True)
        report("device inspect_clusters, summary + labels + table", dev)
        report("host downloads (owner state, list, records)", dl)
        print(f"bytes to the host: device {dev_bytes}, host road {nO * 64 + rows * (8 + 48)}")
        t0 = time.perf_counter()
        want = clusters(positions(pkg.model.decode_positions, p, state), mass, np.arange(nO) < nC, whole, tables, thr)
        print(f"host union-find and fp64 sums (numpy + a Python loop over the edges): {1e3 * (time.perf_counter() - t0):.1f} ms")
        same = got["summary"] == want["summary"] and all(np.array_equal(got[k], want[k]) for k in ("labels", "label", "size"))
        worst = 0.0
        if same and len(want["label"]):
            worst = max(float((np.abs(got["mass"] - want["mass"]) / want["mass"]).max()),
                        float((np.abs(got["moment"] - want["moment"]) / np.maximum(want["abs_moment"], 1e-300)).max()))
        # (the largest cluster of a settled bed holds nearly every clump: 1e6 terms * 1.1e-16)
        ok = ok and same and worst <= max(1e-10, 1.1e-16 * max(int(want["size"].max(initial=0)), 1))
        print(f"integers equal: {same}; max |device - host| / abs_sum {worst:.3e}")
        ctx.set_timing(True)
        ctx.kernel_time_reset()
        for _ in range(3):
            ctx.inspect_clusters(thr)
        for name in ("clusters_label", "clusters_sort", "clusters_sums"):
            ms, launches = ctx.kernel_time_ms(name)
            print(f"pass {name}: {ms:.4f} ms (mean of {launches})")
        ctx.set_timing(False)
    print("BENCH_OK" if ok else "BENCH_MISMATCH", flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
