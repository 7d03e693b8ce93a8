"""contact_inspect_bench.py -- what one deme_inspect_contacts call costs beside the only other way to the same numbers.

The bed is the recipe of tools/tracker_frame_bench.cpp built through the Python model: n three-sphere clumps on a jittered lattice
of spacing 3 r with random orientations, aspect 1 : 1 : 0.45, in an open-top box, a detection every 40 steps, fast mode, `settle`
settling steps with contact recording on.  Then, with the host clock around each, a warm-up and 5 timed repeats of
  device   Context.inspect_contacts()                      (88 bytes to the host)
  counts   Context.inspect_contact_counts()                (4 bytes an owner)
  host     deme_download_contacts + deme_download_contact_records + deme_download_owner_state, then the fp64 sum in numpy
           (tests/_contact_sums64.py); the downloads and the sum are timed separately
and the median with min - max is printed in ms, with the largest difference between the two tensors relative to sum |r_i| |f_j|.

  python tools/contact_inspect_bench.py [n = 1000000] [settle = 30000]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from tests._contact_sums64 import contact_sums  # noqa: E402

THR = 1e-12


def report(what, v):
    v = sorted(v)
    print(f"{what} median {v[len(v) // 2]:.3f} ms ({v[0]:.3f} - {v[-1]:.3f})", flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    settle = int(sys.argv[2]) if len(sys.argv) > 2 else 30_000
    pkg = entry.load_package()
    b = pkg.model.packed_bed(n, seed=2024, cd_freq=40, spacing_mult=3.0, aspect=(1.0, 1.0, 0.45), bin_multiple=5.0)
    p, sc = b.Initialize()
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

    dev, cnt, dl, hsum = [], [], [], []
    got = want = None
    for rep in range(6):
        t0 = time.perf_counter()
        got = ctx.inspect_contacts(-1, THR)
        t1 = time.perf_counter()
        counts = ctx.inspect_contact_counts(-1, THR)
        t2 = time.perf_counter()
        a, bb, t, _ = ctx.contacts()
        f, _, cpA, cpB = ctx.contact_records()
        state = ctx.download_state()
        t3 = time.perf_counter()
        keep = sc._keep
        tables = (np.asarray(keep["ownerClumpBody"], np.uint32), np.asarray(keep.get("ownerMesh", np.zeros(0)), np.uint32),
                  np.asarray(keep.get("objOwner", np.zeros(0)), np.uint32))
        want = contact_sums({"idA": a, "idB": bb, "type": t, "force": f, "cpA": cpA, "cpB": cpB}, tables, state, np.arange(nO) < nC, THR)
        t4 = time.perf_counter()
        if rep:  # (the first repeat is the warm-up: scratch allocations, the caller's view of the list)
            dev.append(1e3 * (t1 - t0)), cnt.append(1e3 * (t2 - t1)), dl.append(1e3 * (t3 - t2)), hsum.append(1e3 * (t4 - t3))
    report("device inspect_contacts", dev)
    report("device inspect_contact_counts", cnt)
    report("host downloads", dl)
    report("host fp64 sum (numpy)", hsum)
    report("host downloads + sum", [x + y for x, y in zip(dl, hsum)])
    err = np.abs(got["virial"] - want["virial"]) / np.maximum(want["abs_sum"], 1e-300)
    # (the bound of a sum of this many terms: every side's few dozen roundings and the additions, 1.1e-16 each)
    ok = got["sides"] == want["sides"] and np.array_equal(counts, want["counts"]) and err.max() <= 1e-14 + 1.1e-16 * max(want["sides"], 1)
    print(f"sides {got['sides']} clumps {got['clumps']} coordination {got['sides'] / max(got['clumps'], 1):.4f} zz {got['virial'][2, 2]:.6e} "
          f"max |device - host| / abs_sum {err.max():.3e}")
    print("BENCH_OK" if ok else "BENCH_MISMATCH", flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
