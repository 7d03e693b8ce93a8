"""bench.py's one-line JSON contract (driver-facing), on a small bed so that it runs in seconds."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_fields():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "24", "--warmup", "4", "--clumps",
                          "30000", "--presettle", "3000", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == "clump*steps/s" and d["unit"] == "clump*steps/s" and d["n_gpus"] == 1 and d["steps"] == 24 and d["warmup"] == 4
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"] and d["config"]["clumps_total"] == 30000
    assert abs(d["value"] - 30000 * 24 / (d["ms_per_step"] * 24e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["launches"] > 0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0 < r["frac"] < 1
    assert r["traffic"] is None  # the PMC figure in profiles/ belongs to the 1e6-clump workload, not to this small bed
    assert d["cpu_baseline"] is None  # switched off here; a --full run fills it (kind, cores, sample)


def _load_bench():
    """bench.py as a module, without leaving its process-wide environment default behind in the test process"""
    key = "HSA_ENABLE_IPC_MODE_LEGACY"
    saved = os.environ.get(key)
    import bench
    if saved is None:
        os.environ.pop(key, None)
    return bench


class _FakeCtx:
    """the two read-backs dump_outputs makes, on a bed larger than its sample, contact list in a given order"""

    def __init__(self, abi, n_owners, n_contacts, n_w, perm_seed):
        rng = np.random.default_rng(5)
        self.st = {k: (rng.integers(0, 1 << 16, n_owners).astype(dt) if np.dtype(dt).kind == "u" else rng.standard_normal(n_owners).astype(dt))
                   for k, dt in abi.STATE_DTYPES.items()}
        a = rng.integers(0, n_owners, n_contacts).astype(np.uint32)
        b = (a + 1 + rng.integers(0, 50, n_contacts)).astype(np.uint32)
        t = rng.integers(0, 3, n_contacts).astype(np.uint8)
        _, first = np.unique(np.stack([a, b, t], 1), axis=0, return_index=True)  # a contact list holds each pair once
        wc = rng.standard_normal((len(a), n_w)).astype(np.float32)
        perm = np.random.default_rng(perm_seed).permutation(len(first))
        keep = first[perm]
        self.c = (a[keep], b[keep], t[keep], np.zeros(len(keep), np.uint32))
        self.wc = wc[keep]

    def download_state(self):
        return {k: v.copy() for k, v in self.st.items()}

    def contacts(self):
        return self.c

    def wildcard(self, w):
        return self.wc[:, w].copy()


def test_dump_outputs_float_files_bounded_and_independent_of_the_list_order(pkg, tmp_path):
    """--dump-outputs writes float32 / float64 .npy files within 64 MB, a fixed sample of a larger output, and the same files
    whatever order the engine keeps its contact list in"""
    bench = _load_bench()
    p = types.SimpleNamespace(nvXp2=22, nvYp2=21, voxelSize=1.28e-7, l=1.95e-12, nContactWildcards=4)
    n_o, n_c = bench.DUMP_SAMPLE + 40_000, bench.DUMP_SAMPLE + 90_000
    sizes = bench.dump_outputs(pkg, _FakeCtx(pkg.abi, n_o, n_c, 4, 1), p, str(tmp_path / "a"))
    bench.dump_outputs(pkg, _FakeCtx(pkg.abi, n_o, n_c, 4, 2), p, str(tmp_path / "b"))
    assert sum(sizes.values()) <= 64 << 20
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in sizes)
    for n in sizes:
        x, y = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert len(x) == bench.DUMP_SAMPLE, n
        assert x.shape == y.shape and (x == y).all(), n
    ids = np.load(tmp_path / "a" / "contact_ids.npy")
    assert (np.diff(ids[:, 0]) >= 0).all()  # canonical order: ascending A id first
    # a full-size bed (10^6 owners, 4.3 M contacts) writes the same sample sizes: within the limit by construction
    assert bench.DUMP_SAMPLE * (24 + 16 + 4 * 12) + bench.DUMP_SAMPLE * (24 + 4 * 4) <= 64 << 20


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_outputs_repeat(tmp_path):
    """a plain run (no --full) takes no side measurement, and two runs with the same arguments dump the same outputs bit for bit"""
    outs = []
    for d in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3", "--clumps",
                              "30000", "--presettle", "3000", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        outs.append(json.loads(lines[0]))
    for js in outs:
        assert js["steps"] == 12 and js["warmup"] == 3 and js["ms_per_step"] > 0
        assert js["cpu_baseline"] is None and js["roofline"]["attainable_copy_GBs"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names and names == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and (x == y).all(), n
    assert np.load(tmp_path / "a" / "owner_pos.npy").shape == (outs[0]["config"]["owners_this_rank"], 3)  # below the sample size: every owner
