"""tri_loads_bench.py -- what one deme_inspect_tri_loads call costs beside the only other way to the same numbers.

The scene is bench.py's BASELINE configs[3] flavour (bench.build_bed with a wavy fixed plate of about `triangles` triangles under the
bed: python bench.py --mesh-triangles), fast mode, `settle` steps with contact recording on.  Then, with the host clock around
each, a warm-up and 5 timed repeats of
  device   Context.inspect_tri_loads()                      (28 bytes a triangle to the host)
  host     deme_download_contacts + deme_download_contact_records, then the fp64 sum per triangle in numpy
           (tests/_tri_loads64.py); the downloads and the sum are timed separately
and the median with min - max is printed in ms, with the bytes either road brings to the host, the longest run of rows on one
triangle, the largest difference between the two answers relative to a triangle's sum |f_j|, and the time of the call's three
passes from the library's event timers (deme_kernel_time_ms).  `thr` is the force threshold (0: every listed sphere-mesh row
counts).

  python tools/tri_loads_bench.py [n = 2000000] [triangles = 40000] [settle = 2000] [thr = 1e-12]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402
from tests._tri_loads64 import tri_loads  # noqa: E402


def report(what, v):
    v = sorted(v)
    print(f"{what} median {v[len(v) // 2]:.3f} ms ({v[0]:.3f} - {v[-1]:.3f})", flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    triangles = int(sys.argv[2]) if len(sys.argv) > 2 else 40_000
    settle = int(sys.argv[3]) if len(sys.argv) > 3 else 2_000
    thr = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-12
    pkg = entry.load_package()
    b = bench.build_bed(pkg, n, 2024, 40)
    lo, hi = b.user_box_min, b.user_box_max
    n_side = max(2, int(round((triangles / 2) ** 0.5)))
    v, f = pkg.model.plate_mesh(n_side, n_side, float(hi[0] - lo[0]) * 0.98, float(hi[1] - lo[1]) * 0.98, z=0.0, wavy=0.002)
    m = b.AddMeshObject(v, f, 0)
    m.SetInitPos(((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, 0.021))
    p, sc = b.Initialize()
    ctx = pkg.Context(0)
    ctx.set_arith_mode("fast")
    ctx.set_params(p)
    ctx.upload_scene(sc)
    ctx.set_record_contacts(True)
    t0 = time.perf_counter()
    ctx.step(settle)
    ctx.sync()
    nT = int(sc.nTri)
    rows = int(ctx.counts().nContacts)
    print(f"BED clumps={int(sc.nOwnerClumps)} triangles={nT} settle_steps={settle} settle_s={time.perf_counter() - t0:.1f} contacts={rows} "
          f"block_rows={pkg.abi.tri_loads_block_rows()}", flush=True)
    sphere_owner = np.asarray(sc._keep["ownerClumpBody"], np.uint32)

    dev, dl, hsum = [], [], []
    got = want = None
    for rep in range(6):
        before = ctx.query_host_bytes()
        t0 = time.perf_counter()
        got = ctx.inspect_tri_loads(thr)
        t1 = time.perf_counter()
        dev_bytes = ctx.query_host_bytes() - before
        a, bb, t, _ = ctx.contacts()
        frc = ctx.contact_records()[0]
        t2 = time.perf_counter()
        want = tri_loads(a, bb, t, frc, sphere_owner, None, nT, thr)
        t3 = time.perf_counter()
        if rep:  # (the first repeat is the warm-up: scratch allocations, the caller's view of the list)
            dev.append(1e3 * (t1 - t0)), dl.append(1e3 * (t2 - t1)), hsum.append(1e3 * (t3 - t2))
    report("device inspect_tri_loads", dev)
    report("host downloads", dl)
    report("host fp64 sum per triangle (numpy)", hsum)
    report("host downloads + sum", [x + y for x, y in zip(dl, hsum)])
    # what deme_download_contacts and deme_download_contact_records move: 8 bytes of key and 4 records of 12 bytes a row
    print(f"bytes to the host: device {dev_bytes}, host road {rows * (8 + 48)}")
    force, counts = got
    err = np.abs(force - want["force"]) / np.maximum(want["abs_sum"], 1e-300)
    sm = int((t == 2).sum())
    ok = np.array_equal(counts, want["counts"]) and err.max() <= 1e-14 + 1.1e-16 * max(int(counts.max(initial=0)), 1)
    print(f"sphere-mesh rows {sm} counted {int(counts.sum())} loaded triangles {int((counts > 0).sum())} longest run {int(counts.max(initial=0))} "
          f"Fz {force[:, 2].sum():.6e} max |device - host| / abs_sum {err.max():.3e}")
    # the passes by themselves: three more calls with the library's event timers on (kept out of the host clock's repeats above)
    ctx.set_timing(True)
    ctx.kernel_time_reset()
    for _ in range(3):
        ctx.inspect_tri_loads(thr)
    for name in ("tri_loads_select", "tri_loads_sort", "tri_loads_sums"):
        ms, launches = ctx.kernel_time_ms(name)
        print(f"pass {name}: {ms:.4f} ms (mean of {launches})")
    ctx.set_timing(False)
    print("BENCH_OK" if ok else "BENCH_MISMATCH", flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
