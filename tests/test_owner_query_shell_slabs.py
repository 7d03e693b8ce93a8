"""The by-owner contact questions of the C++ shell on a DECOMPOSED run (tests/clients/demo_owner_query_slabs.cpp): a bed cut
into 2 and 3 slabs on one GPU, the tracked clump next to the first cut, the plane tracked.  GetOwnerContactForces,
GetOwnerContactClumps and DEMTracker::GetContactClumps select on the slabs' devices; DEME_QUERY_HOST=1 keeps the paths that
download the merged list, and the two must print the same -- the floats are printed with %a."""
import collections
import os
import subprocess

import pytest

from tests import test_contact_query_shell as one_domain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dem-engine_amd", "host")
CLIENT = os.path.join(ROOT, "tests", "clients", "demo_owner_query_slabs")
BYTE_LINES = ("LIST_BYTES", "CLUMP_BYTES")
_runs = {}


def _make():
    subprocess.check_call(["make", "-C", HOST, "demo_owner_query_slabs"], stdout=subprocess.DEVNULL)


def test_demo_owner_query_slabs_builds():
    """the client calls GetOwnerQueryHostBytes: it does not compile without it"""
    _make()
    assert os.access(CLIENT, os.X_OK)


def _run(**env):
    key = tuple(sorted(env.items()))
    if key not in _runs:
        _make()
        e = dict(os.environ)
        e.pop("DEME_QUERY_HOST", None), e.pop("DEME_SLABS_PER_DEVICE", None)
        e.update(env)
        out = subprocess.run([CLIENT], capture_output=True, text=True, timeout=600, env=e)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "DEMO_OK" in out.stdout, out.stdout
        _runs[key] = out.stdout
    return _runs[key]


def _split(stdout):
    """(the lines apart from the byte lines, {byte line tag: value})"""
    rest, nbytes = [], {}
    for line in stdout.splitlines():
        w = line.split()
        if w and w[0] in BYTE_LINES:
            nbytes[w[0]] = int(w[1])
        else:
            rest.append(line)
    return rest, nbytes


@pytest.mark.gpu
@pytest.mark.parametrize("slabs", ["2", "3"])
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_device_path_prints_what_the_whole_list_path_prints(slabs, arith):
    dev, dev_bytes = _split(_run(DEME_ARITH=arith, DEME_SLABS_PER_DEVICE=slabs))
    host, host_bytes = _split(_run(DEME_ARITH=arith, DEME_SLABS_PER_DEVICE=slabs, DEME_QUERY_HOST="1"))
    d = one_domain._parse("\n".join(dev))
    assert d["SLABS"] == int(slabs)  # the run really is decomposed
    assert [l for l in dev if l.startswith("FORCES")] == [l for l in host if l.startswith("FORCES")], (slabs, arith)
    assert dev == host, (slabs, arith)
    # the answers are not empty: the clump has neighbours and lies on the plane, both carry forces
    clump, plane = d["CLUMP_ID"], d["PLANE_ID"]
    want = [b if a == clump else a for a, b in d["PAIRS"] if clump in (a, b)]
    assert len(want) > 0 and collections.Counter(d["CLUMP"]) == collections.Counter(want) and d["TRACKER_CLUMP"] == d["CLUMP"]
    assert len(d["PLANE"]) > 0 and d["PLANE"] == d["TRACKER_PLANE"] and clump in d["PLANE"]
    for who in ("clump", "plane"):
        for flavour in ("plain", "global", "local"):
            w = d[f"FORCES {who} {flavour}"]
            assert int(w[0]) > 0 and any(float.fromhex(x) != 0.0 for x in w[4:7]), (who, flavour)
    print(f"{slabs} slabs, {arith}: list {dev_bytes['LIST_BYTES']} bytes, the clump's questions {dev_bytes['CLUMP_BYTES']} bytes "
          f"({dev_bytes['CLUMP_BYTES'] / dev_bytes['LIST_BYTES']:.4f})")
    assert host_bytes["CLUMP_BYTES"] == 0
    assert dev_bytes["LIST_BYTES"] == host_bytes["LIST_BYTES"] > 0
    assert 0 < dev_bytes["CLUMP_BYTES"] < 0.05 * dev_bytes["LIST_BYTES"]


@pytest.mark.gpu
def test_demo_contact_query_in_two_slabs_prints_what_it_printed():
    """the unchanged client of the one-domain test in 2 slabs: its decomposed run now takes the device path, and prints what the
    whole-list path (what it took before) prints"""
    dev = one_domain._run(DEME_ARITH="exact", DEME_SLABS_PER_DEVICE="2")
    host = one_domain._run(DEME_ARITH="exact", DEME_SLABS_PER_DEVICE="2", DEME_QUERY_HOST="1")
    assert one_domain._parse(dev)["SLABS"] == 2
    assert dev == host
