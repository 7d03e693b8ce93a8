"""tri_wear_bench.py -- what a mesh-wear sample (deme_tri_wear_sample) costs beside the steps and beside the host road to the same
integrals.

The scene is that of tools/tri_loads_bench.py: bench.py's BASELINE configs[3] flavour (bench.build_bed with a wavy fixed plate of about
`triangles` triangles under the bed), fast mode, `settle` steps with contact recording on.  Then
  passes    the three event timers of one sample (deme_kernel_time_ms: tri_wear_select, tri_wear_sort, tri_wear_sums), mean of three
  run       ms per step of 400 steps taken 10 at a call, host clock from the first call to the end of a sync, with a sample after
            every call and with wear disabled: alternating runs in one session, two each, every figure printed
  host      the host road's downloads alone (deme_download_contacts + deme_download_contact_records + the owners' state): what one
            sample costs a script that integrates on the host, 5 repeats, median with min - max
  read      one deme_tri_wear_read of the whole mesh, 5 repeats

  python tools/tri_wear_bench.py [n = 2000000] [triangles = 40000] [settle = 2000] [thr = 1e-12]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402


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
    print(f"BED clumps={int(sc.nOwnerClumps)} triangles={int(sc.nTri)} settle_steps={settle} settle_s={time.perf_counter() - t0:.1f} "
          f"contacts={int(ctx.counts().nContacts)}", flush=True)

    ctx.tri_wear_enable()
    ctx.tri_wear_sample(thr, 0.0)  # (the warm-up: the pair list and the sort's scratch are allocated)
    ctx.sync()
    ctx.set_timing(True)
    ctx.kernel_time_reset()
    for _ in range(3):
        ctx.tri_wear_sample(thr, 0.0)
    ctx.sync()
    total = 0.0
    for name in ("tri_wear_select", "tri_wear_sort", "tri_wear_sums"):
        ms, launches = ctx.kernel_time_ms(name)
        total += ms
        print(f"pass {name}: {ms:.4f} ms (mean of {launches})")
    print(f"passes of one sample: {total:.4f} ms")
    ctx.set_timing(False)

    h = float(p.h)
    for rep in range(2):
        for wear in (True, False):
            ctx.tri_wear_enable(wear)
            ctx.step(10)  # (the first call after a switch: allocations)
            if wear:
                ctx.tri_wear_sample(thr, 10 * h)
            ctx.sync()
            skipped = 0
            t0 = time.perf_counter()
            for _ in range(40):
                ctx.step(10)
                if wear:
                    skipped += not ctx.tri_wear_sample(thr, 10 * h)
            ctx.sync()
            ms = 1e3 * (time.perf_counter() - t0) / 400
            print(f"run {rep}: 400 steps, {'a sample every 10 steps' if wear else 'wear disabled'}: {ms:.5f} ms a step"
                  + (f" ({skipped} samples found an unevaluated list)" if wear else ""), flush=True)
    ctx.tri_wear_enable(True)
    ctx.tri_wear_sample(thr, 10 * h)

    dl, rd = [], []
    for rep in range(6):
        t0 = time.perf_counter()
        ctx.contacts()
        ctx.contact_records()
        ctx.download_state()
        t1 = time.perf_counter()
        before = ctx.query_host_bytes()
        got = ctx.tri_wear_read()
        t2 = time.perf_counter()
        if rep:
            dl.append(1e3 * (t1 - t0)), rd.append(1e3 * (t2 - t1))
    report("host road: downloads of one sample", dl)
    report("tri_wear_read, the whole mesh", rd)
    print(f"bytes of a read {ctx.query_host_bytes() - before}; counted rows of the last sample's mesh {int(got['rows'].sum())}, loaded triangles "
          f"{int((got['rows'] > 0).sum())}, sliding work {got['slidingWork'].sum():.6e} J, normal impulse {got['normalImpulse'].sum():.6e} N s")
    print("BENCH_OK", flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
