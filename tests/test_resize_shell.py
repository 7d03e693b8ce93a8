"""DEMSolver::ChangeClumpSizes / DEMTracker::ChangeClumpSizes through the C++ shell (host/demo_grow.cpp): a radius-expansion loop,
a tracker-relative resize, and UpdateClumps afterwards."""
import csv
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dem-engine_amd", "host")
R_TEMPLATE = np.float32(0.8) * np.float32(0.004)  # demo_grow's template radius, after Scale
N_BED, N_FEW = 600, 2


def test_demo_grow_builds():
    subprocess.check_call(["make", "-C", HOST, "demo_grow"], stdout=subprocess.DEVNULL)
    assert os.access(os.path.join(HOST, "demo_grow"), os.X_OK)


def _radii(path):
    with open(path) as f:
        return np.array([np.float32(float(r["r"])) for r in csv.DictReader(f)], np.float32)


def _xyz(path):
    with open(path) as f:
        return np.array([[float(r["X"]), float(r["Y"]), float(r["Z"])] for r in csv.DictReader(f)])


def _run(out_dir, rounds, env=None):
    import os as _os
    e = dict(_os.environ)
    e.update(env or {})
    out = subprocess.run([os.path.join(HOST, "demo_grow"), str(rounds), str(out_dir)], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.mark.gpu
def test_demo_grow_resizes_and_keeps_geometry_through_update_clumps(tmp_path):
    subprocess.check_call(["make", "-C", HOST, "demo_grow"], stdout=subprocess.DEVNULL)
    rounds = 5
    stdout = _run(tmp_path, rounds)
    assert "THROW_BEFORE_INIT ChangeClumpSizes operates on device-side arrays directly" in stdout, stdout
    assert "DEMO_OK" in stdout
    grown = _radii(tmp_path / "spheres_grown.csv")
    assert grown.size == 3 * (N_BED + N_FEW)
    # compounding fp32 multiplies of the current radius (the csv holds 6 significant digits)
    want = R_TEMPLATE
    for _ in range(rounds):
        want = want * np.float32(1.02)
    np.testing.assert_allclose(grown[:3 * N_BED], want, rtol=5e-6)
    # the tracker's id 1 is the small batch's second clump, not the bed's
    few = grown[3 * N_BED:]
    np.testing.assert_allclose(few[:3], R_TEMPLATE, rtol=5e-6)
    np.testing.assert_allclose(few[3:], R_TEMPLATE * np.float32(1.5), rtol=5e-6)
    # UpdateClumps: the grown clumps keep their radii, the appended clump joins at template size
    upd = _radii(tmp_path / "spheres_updated.csv")
    assert upd.size == grown.size + 3
    assert np.array_equal(upd[:grown.size], grown)
    np.testing.assert_allclose(upd[grown.size:], R_TEMPLATE, rtol=5e-6)
    # ResortClumps renumbers the clumps: every one keeps its spheres' radii
    res = _radii(tmp_path / "spheres_resorted.csv")
    assert np.array_equal(np.sort(res), np.sort(upd))


@pytest.mark.gpu
def test_demo_grow_on_two_slabs_prints_what_one_domain_prints(tmp_path):
    """the same script decomposed into two slabs, with a halo the growth outgrows after the second round: the shell re-plans with a
    halo that fits and carries the grown geometry over; radii equal the single domain's, positions within the slab bound"""
    subprocess.check_call(["make", "-C", HOST, "demo_grow"], stdout=subprocess.DEVNULL)
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir(), two.mkdir()
    _run(one, 5)
    # (the clump reaches 5.62 mm from its centre: a 11.5 mm halo holds two reaches up to a growth of 2.3 %)
    _run(two, 5, {"DEME_SLABS_PER_DEVICE": "2", "DEME_SLAB_HALO": "0.0115"})
    for name in ("spheres_grown.csv", "spheres_updated.csv"):
        assert np.array_equal(_radii(one / name), _radii(two / name)), name
        assert np.abs(_xyz(one / name) - _xyz(two / name)).max() < 1e-3, name
