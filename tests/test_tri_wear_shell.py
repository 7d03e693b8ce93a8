"""DEMSolver::EnableMeshWearAccumulation, the trackers' GetMeshFace... wear getters and the wear arrays of WriteMeshFile through the C++
shell (dem-engine_amd/host/demo_wear.cpp): two layers of spheres, held in x and y by a prescribed zero velocity, settle on a flat plate
of 128 triangles that is then moved at a prescribed VX = 0.5 m/s for 1200 steps, with a sample every 10 steps.

Every contact slides at VX apart from the spheres' spin, so the total sliding work is held against VX times the total normal impulse.
The bound of |ratio - 1| is not taken from the accumulators: the oracle exposes no contact records, so it comes from the float64 model
on the downloaded records -- the client's host road, which fetches the whole list after every interval and adds w |f_z| and
w |f_z| |u_t| in double from the trackers' state -- as the ratio that reaches and its deviation from 1, doubled.  The two roads are also
held to each other within 1e-4 of the totals: they add the same fp32 forces; the host road takes the arm of the spin term from fp32
world coordinates (1.5e-8 m of a 4 mm arm, 4e-6 of that term) and the angular velocity from an fp32 rotation (1e-7), ten times which is
1e-4 with room for the order of the additions.
Measured (MI355X, exact mode): one slab ratio 0.953911 on the device and 0.953911 on the host road (deviation 4.61e-2, bound 9.22e-2), the
two roads' normal impulse agrees to 2.5e-8 and their sliding work to 1.2e-8; two slabs 0.953905 on both roads, the same agreement."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dem-engine_amd", "host")
CLIENT = os.path.join(HOST, "demo_wear")
FACES, VX, K_OVER_H, H = 128, float(np.float32(0.5)), 1e-13, 5e-6
_runs = {}


def _make():
    subprocess.check_call(["make", "-C", HOST, "demo_wear"], stdout=subprocess.DEVNULL)


def test_demo_wear_builds():
    """the client calls EnableMeshWearAccumulation, ResetMeshWear, GetMeshWearSampledTime and the six tracker getters: it does not
    compile without them"""
    _make()
    assert os.access(CLIENT, os.X_OK)


def _run(tmp_path_factory, **env):
    key = tuple(sorted(env.items()))
    if key not in _runs:
        _make()
        out_dir = tmp_path_factory.mktemp("wear")
        e = dict(os.environ)
        e.pop("DEME_SLABS_PER_DEVICE", None)
        e.update(env)
        out = subprocess.run([CLIENT, str(out_dir)], capture_output=True, text=True, timeout=600, env=e)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "DEMO_OK" in out.stdout, out.stdout
        _runs[key] = (out.stdout, out_dir)
    return _runs[key]


def _parse(stdout):
    d, faces = {}, []
    for line in stdout.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "THROW":
            d["THROW"] = line[6:]
        elif w[0] == "FACE":
            faces.append([float.fromhex(x) for x in w[2:]])
        elif w[0] in ("SLABS", "INTERVALS", "TOTALS", "HOST", "RATIO", "FORCE_Z"):
            d[w[0]] = [float.fromhex(x) if "0x" in x else float(x) for x in w[1:]]
    d["FACE"] = np.array(faces)
    return d


def _check(stdout, out_dir, slabs):
    d = _parse(stdout)
    print("\n".join(l for l in stdout.splitlines() if not l.startswith("FACE ")))
    assert d["SLABS"] == [slabs] and "NO_THROW" not in stdout
    assert "GetMeshFaceSlidingWork" in d["THROW"] and "mesh" in d["THROW"]
    # 37 + 3 + 60 steps with a sample every 10: ten intervals, 100 h
    assert abs(d["INTERVALS"][0] - 100.0) <= 1e-5
    ix, iy, iz, normal, sliding, shear, t = d["TOTALS"]
    host_normal, host_sliding = d["HOST"]
    ratio, host_ratio = d["RATIO"]
    assert abs(t - 1200 * H) <= 1e-6 * t and normal > 0 and sliding > 0 and shear > 0 and iz < 0
    # the sliding plate: work against VX times the normal impulse, the bound from the host road's float64 model
    bound = 2 * abs(host_ratio - 1.0)
    print(f"{slabs} slab(s): sliding work / (VX * normal impulse) {ratio:.6f} on the device, {host_ratio:.6f} on the host road; |ratio - 1| "
          f"{abs(ratio - 1):.3e}, bound {bound:.3e}; device / host normal {normal / host_normal - 1:+.3e}, sliding {sliding / host_sliding - 1:+.3e}")
    assert ratio == sliding / (VX * normal) and bound > 0
    assert abs(ratio - 1.0) <= bound
    assert abs(normal - host_normal) <= 1e-4 * host_normal and abs(sliding - host_sliding) <= 1e-4 * host_sliding
    fz_t, iz2 = d["FORCE_Z"]
    assert iz2 == iz and fz_t < 0
    # per face
    area, work, depth, pressure = d["FACE"].T
    assert len(area) == FACES and np.abs(area / (0.5 * (0.14 / 8) ** 2) - 1).max() < 1e-5
    assert np.array_equal(depth, K_OVER_H * work / area) and (work > 0).any() and (work >= 0).all()
    assert abs(work.sum() - sliding) <= 1e-12 * sliding
    assert np.isfinite(pressure).all() and (pressure >= 0).all() and abs((pressure * area * t).sum() - normal) <= 1e-12 * normal
    # the VTK files: the grid is what it is without the feature, the three wear arrays follow it
    plain = open(os.path.join(out_dir, "mesh_plain.vtk"), "rb").read()
    wear = open(os.path.join(out_dir, "mesh_wear.vtk"), "rb").read()
    assert b"CELL_DATA" not in plain and b"CELL_TYPES" in plain
    assert wear.startswith(plain) and len(wear) > len(plain)
    tail = [l for l in wear[len(plain):].decode().split("\n") if l.strip()]
    assert tail[0] == f"CELL_DATA {FACES}" and tail[1] == "VECTORS wear_impulse float"
    vec = np.array([[float(x) for x in l.split()] for l in tail[2:2 + FACES]])
    assert vec.shape == (FACES, 3)
    assert tail[2 + FACES] == "SCALARS wear_sliding_work float 1" and tail[3 + FACES] == "LOOKUP_TABLE default"
    vtk_work = np.array([float(l) for l in tail[4 + FACES:4 + 2 * FACES]])
    assert tail[4 + 2 * FACES] == "SCALARS wear_shear_work float 1" and tail[5 + 2 * FACES] == "LOOKUP_TABLE default"
    vtk_shear = np.array([float(l) for l in tail[6 + 2 * FACES:6 + 3 * FACES]])
    assert len(tail) == 6 + 3 * FACES
    assert np.abs(vtk_work - work).max() <= 1e-5 * work.max()  # (six printed digits a value)
    assert abs(vtk_shear.sum() - shear) <= 1e-4 * shear and np.abs(vec.sum(0) - [ix, iy, iz]).max() <= 1e-4 * abs(iz)


@pytest.mark.gpu
def test_sliding_work_on_a_sliding_plate(tmp_path_factory):
    _check(*_run(tmp_path_factory, DEME_ARITH="exact"), 1)


@pytest.mark.gpu
def test_sliding_work_on_a_sliding_plate_in_two_slabs(tmp_path_factory):
    _check(*_run(tmp_path_factory, DEME_ARITH="exact", DEME_SLABS_PER_DEVICE="2"), 2)
