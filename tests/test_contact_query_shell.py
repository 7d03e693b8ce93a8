"""DEMSolver::GetOwnerContactClumps, DEMTracker::GetContactClumps and the GetContactForces family on the device-side owner query,
through the C++ shell (tests/clients/demo_contact_query.cpp): a small bed pressed onto a plane, one clump and the plane tracked."""
import collections
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dem-engine_amd", "host")
CLIENT = os.path.join(ROOT, "tests", "clients", "demo_contact_query")
_runs = {}


def _make():
    subprocess.check_call(["make", "-C", HOST, "demo_contact_query"], stdout=subprocess.DEVNULL)


def test_demo_contact_query_builds():
    """the client calls GetOwnerContactClumps and GetContactClumps: it does not compile without them"""
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


def _parse(stdout):
    """tag -> list of ints for the id lines, 'FORCES who flavour' -> the rest of the line, PAIRS -> list of (a, b)"""
    d = {}
    for line in stdout.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "PAIRS":
            d["PAIRS"] = [tuple(int(x) for x in pr.split(":")) for pr in w[1:]]
        elif w[0] in ("CLUMP", "PLANE"):
            d[w[0] + "_ID"], d[w[0]] = int(w[1]), [int(x) for x in w[3:]]
        elif w[0] in ("TRACKER_PLANE", "TRACKER_CLUMP"):
            d[w[0]] = [int(x) for x in w[2:]]
        elif w[0] == "SLABS":
            d["SLABS"] = int(w[1])
        elif w[0] == "FORCES":
            d[f"FORCES {w[1]} {w[2]}"] = w[3:]
    return d


@pytest.mark.gpu
def test_contact_clumps_and_forces_of_the_tracked_owners():
    stdout = _run(DEME_ARITH="exact")
    d = _parse(stdout)
    assert "THROW_OUT_OF_RANGE" in stdout and "THROW_OFFSET tracker offset is out of range" in stdout and "NO_THROW" not in stdout
    clump, plane = d["CLUMP_ID"], d["PLANE_ID"]
    # the clump: one entry per listed pair it is on, the other side's owner (GetClumpContacts lists owner pairs of the
    # sphere--sphere rows in list order, so the sequence follows too)
    want = [b if a == clump else a for a, b in d["PAIRS"] if clump in (a, b)]
    assert len(want) > 0 and d["CLUMP"] == want
    assert collections.Counter(d["CLUMP"]) == collections.Counter(want)
    assert d["TRACKER_CLUMP"] == d["CLUMP"]
    # the plane: every entry is a clump; the tracked clump lies on it
    assert len(d["PLANE"]) > 0 and d["PLANE"] == d["TRACKER_PLANE"]
    assert all(o < plane for o in d["PLANE"]) and clump in d["PLANE"]
    for who in ("clump", "plane"):
        for flavour in ("plain", "global", "local"):
            w = d[f"FORCES {who} {flavour}"]
            assert int(w[0]) > 0, (who, flavour)
            sums = [float.fromhex(x) for x in w[1:]]
            assert any(s != 0.0 for s in sums[3:6]), (who, flavour, "force sum")
    print("\n".join(l for l in stdout.splitlines() if l.startswith(("FORCES", "FRAMES", "CLUMP", "DEMO_OK"))))


@pytest.mark.gpu
def test_device_path_prints_what_the_whole_list_path_prints():
    """DEME_QUERY_HOST=1 keeps GetOwnerContactForces on the path that downloads the whole list; the floats are printed with %a"""
    for arith in ("exact", "fast"):  # (324 clumps: in the fast mode the engine keeps an order of its own)
        dev, host = _run(DEME_ARITH=arith), _run(DEME_ARITH=arith, DEME_QUERY_HOST="1")
        assert [l for l in dev.splitlines() if l.startswith("FORCES")] == [l for l in host.splitlines() if l.startswith("FORCES")], arith
        assert dev == host, arith


@pytest.mark.gpu
def test_two_slabs_print_the_same_contact_clumps():
    one, two = _parse(_run(DEME_ARITH="exact")), _parse(_run(DEME_ARITH="exact", DEME_SLABS_PER_DEVICE="2"))
    assert one["SLABS"] == 1 and two["SLABS"] == 2  # the second run really is decomposed
    assert one["CLUMP_ID"] == two["CLUMP_ID"] and one["PLANE_ID"] == two["PLANE_ID"]
    for tag in ("CLUMP", "PLANE", "TRACKER_PLANE", "TRACKER_CLUMP"):
        assert collections.Counter(one[tag]) == collections.Counter(two[tag]), tag
    assert len(two["CLUMP"]) > 0 and len(two["PLANE"]) > 0
