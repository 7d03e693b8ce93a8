"""fields_bench.py -- what one deme_inspect_fields call costs beside the only other way to the same numbers.

The scene is bench.py's flagship bed (bench.build_bed), fast mode, `settle` steps with contact recording on; the grid has `cells`
cells a side over the clumps' bounding box and every column is asked.  Then, with the host clock around each, a warm-up and 5 timed
repeats of
  device   Context.inspect_fields()                        (168 bytes a cell to the host)
  host     deme_download_owner_state + deme_download_contacts + deme_download_contact_records: what a script has to bring to the
           host today before it can sum anything (64 bytes an owner and 56 a row on the device's side)
and the median with min - max is printed in ms, with the time of the call's three passes from the library's event timers
(deme_kernel_time_ms) and, once, the largest difference to the fp64 statement in numpy (tests/_fields64.py) relative to a cell's
sum of |term|.

  python tools/fields_bench.py [n = 1000000] [cells = 64] [settle = 200] [thr = 1e-12]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402
from tests._fields64 import fields, positions  # noqa: E402


def report(what, v):
    v = sorted(v)
    print(f"{what} median {v[len(v) // 2]:.3f} ms ({v[0]:.3f} - {v[-1]:.3f})", flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    cells = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    settle = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    thr = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-12
    pkg = entry.load_package()
    p, sc = bench.build_bed(pkg, n, 2024, 40).Initialize()
    ctx = pkg.Context(0)
    ctx.set_arith_mode("fast")
    ctx.set_params(p)
    ctx.upload_scene(sc)
    ctx.set_record_contacts(True)
    volumes = (1e-7 * (1.0 + np.arange(int(sc.nMassProps)))).astype(np.float32)
    ctx.upload_volumes(volumes)
    t0 = time.perf_counter()
    ctx.step(settle)
    ctx.sync()
    nO, nC = int(sc.nOwners), int(sc.nOwnerClumps)
    rows = int(ctx.counts().nContacts)
    print(f"BED clumps={nC} settle_steps={settle} settle_s={time.perf_counter() - t0:.1f} contacts={rows} grid={cells}^3 "
          f"block_rows={pkg.abi.fields_block_rows()}", flush=True)
    state = ctx.download_state()
    X = positions(pkg.model.decode_positions, p, state)
    lo, hi = X[:nC].min(0) - 1.2345e-4, X[:nC].max(0) + 2.3456e-4
    grid = (lo, (hi - lo) / cells, (cells, cells, cells))

    dev, dl = [], []
    got = whole = None
    for rep in range(6):
        before = ctx.query_host_bytes()
        t0 = time.perf_counter()
        got = ctx.inspect_fields(*grid, force_threshold=thr)
        t1 = time.perf_counter()
        dev_bytes = ctx.query_host_bytes() - before
        state = ctx.download_state()
        a, bb, t, _ = ctx.contacts()
        rec = ctx.contact_records()
        t2 = time.perf_counter()
        whole = {"idA": a, "idB": bb, "type": t, "force": rec[0], "cpA": rec[2], "cpB": rec[3]}
        if rep:  # (the first repeat is the warm-up: scratch allocations, the caller's view of the list)
            dev.append(1e3 * (t1 - t0)), dl.append(1e3 * (t2 - t1))
    report("device inspect_fields, every column", dev)
    report("host downloads (owner state, list, records)", dl)
    print(f"bytes to the host: device {dev_bytes}, host road {nO * 64 + rows * (8 + 48)}")

    keep = sc._keep
    off = np.asarray(keep["inertiaPropOffsets"], np.int64)
    tables = (np.asarray(keep["ownerClumpBody"], np.uint32), np.asarray(keep.get("ownerMesh", np.zeros(0)), np.uint32),
              np.asarray(keep.get("objOwner", np.zeros(0)), np.uint32))
    t0 = time.perf_counter()
    want = fields(positions(pkg.model.decode_positions, p, state), state, np.arange(nO) < nC, np.asarray(keep["MassProperties"], np.float32)[off],
                  volumes[off], *grid, whole, tables, thr)
    print(f"host fp64 sums per cell (numpy): {1e3 * (time.perf_counter() - t0):.1f} ms")
    ok = np.array_equal(got["clumps"], want["clumps"]) and np.array_equal(got["sides"], want["sides"])
    worst = 0.0
    for k in ("mass", "volume", "momentum", "kinetic", "virial"):
        worst = max(worst, float((np.abs(got[k] - want[k]) / np.maximum(want["abs_" + k], 1e-300)).max()))
    ok = ok and worst <= 1e-10
    print(f"clumps in the grid {int(got['clumps'].sum())}, most in a cell {int(got['clumps'].max())}, counted sides {int(got['sides'].sum())}, "
          f"most in a cell {int(got['sides'].max())}, max |device - host| / abs_sum {worst:.3e}")
    # the passes by themselves: three more calls with the library's event timers on (kept out of the host clock's repeats above)
    ctx.set_timing(True)
    ctx.kernel_time_reset()
    for _ in range(3):
        ctx.inspect_fields(*grid, force_threshold=thr)
    for name in ("fields_cells", "fields_sort", "fields_sums"):
        ms, launches = ctx.kernel_time_ms(name)
        print(f"pass {name}: {ms:.4f} ms (mean of {launches})")
    ctx.set_timing(False)
    print("BENCH_OK" if ok else "BENCH_MISMATCH", flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
