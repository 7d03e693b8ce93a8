"""The tracker getters and setters of the C++ shell (tests/clients/demo_tracker_io.cpp): ten frames of stepping, reading the pose,
velocity and family of a tracked clump, the plane and every owner of a batch tracker, and writing some of them back in the single
and the vector forms.  The getters gather the tracked owners' records on the device and the setters scatter to them;
DEME_TRACKER_HOST=1 keeps the paths that move the whole state, and the two must print the same -- the floats are printed with %a."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dem-engine_amd", "host")
CLIENT = os.path.join(ROOT, "tests", "clients", "demo_tracker_io")
BYTE_LINES = ("BATCH_GET_BYTES", "TOTAL_BYTES")
FRAMES = 10
_runs = {}


def _make():
    subprocess.check_call(["make", "-C", HOST, "demo_tracker_io"], stdout=subprocess.DEVNULL)


def test_demo_tracker_io_builds():
    """the client links against the shell whose setters scatter: DEMTracker's vector setters and GetOwnerQueryHostBytes"""
    _make()
    assert os.access(CLIENT, os.X_OK)
    lib = subprocess.run(["nm", "-D", os.path.join(ROOT, "dem-engine_amd", "csrc", "libdeme_hip.so")], capture_output=True, text=True).stdout
    assert "deme_scatter_owner_state" in lib and "deme_multi_scatter_owner_state" in lib


def _run(**env):
    key = tuple(sorted(env.items()))
    if key not in _runs:
        _make()
        e = dict(os.environ)
        for k in ("DEME_TRACKER_HOST", "DEME_QUERY_HOST", "DEME_SLABS_PER_DEVICE"):
            e.pop(k, None)
        e.update(env)
        out = subprocess.run([CLIENT, str(FRAMES)], capture_output=True, text=True, timeout=600, env=e)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "DEMO_OK" in out.stdout, out.stdout
        _runs[key] = out.stdout
    return _runs[key]


def _split(stdout):
    """(the lines apart from the byte lines, the bytes of the batch tracker's getter loop per frame, the run's bytes)"""
    rest, per_frame, total = [], [], None
    for line in stdout.splitlines():
        w = line.split()
        if w and w[0] == "BATCH_GET_BYTES":
            per_frame.append(int(w[2]))
        elif w and w[0] == "TOTAL_BYTES":
            total = int(w[1])
        else:
            rest.append(line)
    return rest, per_frame, total


@pytest.mark.gpu
@pytest.mark.parametrize("slabs", [None, "2", "3"])
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_device_path_prints_what_the_whole_state_path_prints(slabs, arith):
    env = {"DEME_ARITH": arith}
    if slabs:
        env["DEME_SLABS_PER_DEVICE"] = slabs
    dev, dev_frames, dev_total = _split(_run(**env))
    host, host_frames, host_total = _split(_run(DEME_TRACKER_HOST="1", **env))
    head = {w[0]: w[1] for w in (l.split() for l in dev) if len(w) == 2 and w[0] in ("SLABS", "NBATCH")}  # (a decomposed run prints RCCL's banner first)
    n_slabs, n_batch = int(head["SLABS"]), int(head["NBATCH"])
    assert n_slabs == (int(slabs) if slabs else 1) and n_batch >= 20
    for i, (a, b) in enumerate(zip(dev, host)):
        assert a == b, (slabs, arith, i, a, b)
    assert len(dev) == len(host) > FRAMES * n_batch
    # the writes and the steps both show: the tracked clump's printed state changes from frame to frame and across the setters
    clump = [l.split(None, 2)[2] for l in dev if l.startswith("CLUMP ") and "twins" not in l]
    clump_set = [l.split(None, 2)[2] for l in dev if l.startswith("CLUMP_SET ")]
    assert len(clump) == len(clump_set) == FRAMES and len(set(clump)) == FRAMES and all(a != b for a, b in zip(clump, clump_set))
    fams = [l.split()[2:] for l in dev if l.startswith("FAMILIES ")]
    assert set(fams[0]) == {"0"} and set(fams[5]) == {"1"} and fams[7][3] == "3" and fams[7].count("1") == n_batch - 1
    # the path that ran: nothing is counted on the whole-state path; on the device path the loop over the batch tracker's offsets
    # (six getters each) is ONE gather of its owners per frame -- 64 bytes per owner, and the count read-back of every slab
    assert host_total == 0 and host_frames == [0] * FRAMES
    one_gather = 64 * n_batch + (4 * n_slabs if slabs else 0)
    assert dev_frames == [one_gather] * FRAMES and dev_total > sum(dev_frames)
    print(f"{n_slabs} slab(s), {arith}: {dev_total} bytes over {FRAMES} frames, {one_gather} per batch read")
