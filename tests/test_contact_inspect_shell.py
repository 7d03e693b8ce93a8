"""DEMInspector("clump_virial") / ("clump_coordination") through the C++ shell (tests/clients/demo_contact_inspect.cpp): a small bed
pressed onto a plane, the two inspectors with and without a region, beside the same sums the client computes from
GetContactDetailedInfo() and the trackers' positions.

The coordination must match exactly.  The tensor is held to a derived bound.  The inspector's own error is the 1e-10 * abs_sum of
tests/test_contact_inspect.py.  The client's arm is (contact point - centre of mass), both fp32 numbers in the global frame of a
0.2 m box, where half an ulp is 7.5e-9 m: the point carries the rounding of the centre, of the sum (centre + rotated local point)
and ~2e-9 m of the fp32 rotation of a 4 mm local point, the centre its own rounding, and on the B side the two bodies' local
points of one contact agree to a few 1e-9 m.  That is below 4e-8 m per component of the arm, so
|tensor_ij - own_ij| <= 4e-8 m * sum |f_j| + 1e-10 * abs_sum_ij, with both sums printed by the client."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dem-engine_amd", "host")
CLIENT = os.path.join(ROOT, "tests", "clients", "demo_contact_inspect")
ARM_ERR, REL = 4e-8, 1e-10
_runs = {}


def _make():
    subprocess.check_call(["make", "-C", HOST, "demo_contact_inspect"], stdout=subprocess.DEVNULL)


def test_demo_contact_inspect_builds():
    """the client calls DEMInspector::GetTensor: it does not compile without it"""
    _make()
    assert os.access(CLIENT, os.X_OK)


def _run(**env):
    key = tuple(sorted(env.items()))
    if key not in _runs:
        _make()
        e = dict(os.environ)
        e.pop("DEME_SLABS_PER_DEVICE", None)
        e.update(env)
        out = subprocess.run([CLIENT], capture_output=True, text=True, timeout=600, env=e)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "DEMO_OK" in out.stdout, out.stdout
        _runs[key] = out.stdout
    return _runs[key]


def _parse(stdout):
    d = {}
    for line in stdout.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] in ("VIRIAL", "OWN_VIRIAL", "OWN_ABS", "COORD", "OWN_COORD"):
            d[(w[0], w[1])] = [float.fromhex(x) if "0x" in x else float(x) for x in w[2:]]
        elif w[0] == "SLABS":
            d["SLABS"] = int(w[1])
        elif w[0] in ("THROW_VALUE", "THROW_TENSOR"):
            d[w[0]] = line[len(w[0]) + 1:]
    return d


def _check(stdout, slabs):
    d = _parse(stdout)
    print("\n".join(l for l in stdout.splitlines() if l.startswith(("FRAMES", "SLABS", "CUT", "COORD", "OWN_COORD", "THROW"))))
    assert d["SLABS"] == slabs and "NO_THROW" not in stdout
    assert "GetTensor()" in d["THROW_VALUE"] and "clump_virial" in d["THROW_VALUE"]
    assert "GetTensor()" in d["THROW_TENSOR"] and "clump_virial" in d["THROW_TENSOR"]
    for which in ("all", "low"):
        got, own = np.array(d[("VIRIAL", which)]), np.array(d[("OWN_VIRIAL", which)])
        abs_sum, fsum = np.array(d[("OWN_ABS", which)][:9]), np.array(d[("OWN_ABS", which)][9:])
        bound = ARM_ERR * np.tile(fsum, 3) + REL * abs_sum
        err = np.abs(got - own)
        print(f"{slabs} slab(s), {which}: max |tensor - own| {err.max():.3e}, bound there {bound[err.argmax()]:.3e}, zz {got[8]:.6e}")
        assert abs_sum.max() > 0 and (err <= bound).all(), (which, err, bound)
        coord, own_coord = d[("COORD", which)], d[("OWN_COORD", which)]
        assert coord[0] == own_coord[0] and coord[1] == own_coord[1] > 0, which  # the value, and the sides summed over GetValues()
        assert got[8] < 0  # pressed onto its floor: compression
    assert d[("COORD", "low")][1] < d[("COORD", "all")][1]
    return d


@pytest.mark.gpu
def test_inspectors_equal_the_sums_of_the_contact_list():
    _check(_run(DEME_ARITH="exact"), 1)


@pytest.mark.gpu
def test_two_slabs_equal_the_sums_of_the_contact_list():
    _check(_run(DEME_ARITH="exact", DEME_SLABS_PER_DEVICE="2"), 2)
