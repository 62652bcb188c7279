"""bench.py --dump-outputs: what the timed path computed in its last step, written as float64 .npy files within 64 MB, the same cells
on every run.  The CPU tests drive bench.dump_outputs with host stand-ins for the driver's multifabs; the GPU test runs bench.py twice."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostFab:
    """stand-in for boxlib.MultiFab: a[i, j, k, c] = the fab's code + position, so a written value names the cell it came from"""

    def __init__(self, sizes, nc, ng, nodal, code):
        self.nc, self.ng, self.sizes, self.nodal, self.code = nc, ng, sizes, nodal, code

    def to_numpy(self, i=0):
        sh = tuple(self.sizes[i][d] + self.nodal + 2 * self.ng for d in range(3))
        I, J, K, Cc = np.meshgrid(*[np.arange(x) - self.ng for x in sh], np.arange(self.nc), indexing="ij")
        return np.asfortranarray(self.code + I + 1e3 * J + 1e6 * K + 1e9 * Cc, dtype=np.float64)


class HostSim:
    def __init__(self, boxes, local, amr):
        levels = boxes if amr else [boxes]
        loc = local if amr else [local]
        sizes = [[tuple(b[1][d] - b[0][d] + 1 for d in range(3)) for b in [lb[g] for g in loc[n]]] for n, lb in enumerate(levels)]
        self.boxes, self.local = boxes, local
        self.uold = [HostFab(s, 3, 3, 0, 0.0) for s in sizes]
        self.sold = [HostFab(s, 2, 3, 0, 0.25) for s in sizes]
        self.gp = [HostFab(s, 3, 1, 0, 0.5) for s in sizes]
        self.p = [HostFab(s, 1, 1, 1, 0.75) for s in sizes]
        self.dt, self.time = 1.25e-3, 0.5


def box(lo, n):
    return (tuple(lo), tuple(x + n - 1 for x in lo))


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_fields_are_written_whole(tmp_path):
    G = HostSim([box((0, 0, 0), 8), box((8, 0, 0), 8)], [0, 1], amr=False)
    files, nbytes, sampled = bench.dump_outputs(G, str(tmp_path), False, 0)
    got = load_dir(str(tmp_path))
    assert not sampled and files == len(got) == 2 * 4 + 2
    assert nbytes == sum(a.nbytes for a in got.values())
    for name, a in got.items():
        assert a.dtype == np.float64, name
    assert got["dt"].tolist() == [1.25e-3] and got["time"].tolist() == [0.5]
    u = got["lev0_box1_u"]
    assert u.shape == (8, 8, 8, 3)
    # the valid cells only: (i, j, k, c) of the box, no ghost cell
    assert u[2, 3, 4, 1] == 2 + 3e3 + 4e6 + 1e9
    assert got["lev0_box0_p"].shape == (9, 9, 9, 1) and got["lev0_box0_p"][8, 8, 8, 0] == 0.75 + 8 + 8e3 + 8e6
    assert got["lev0_box0_gp"][0, 0, 0, 2] == 0.5 + 2e9


def test_large_fields_are_sampled_within_the_budget_and_repeat(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40000)
    boxes = [[box((0, 0, 0), 16)], [box((4, 4, 4), 8), box((12, 4, 4), 12)]]        # two levels, boxes of different sizes
    runs = []
    for tag in ("a", "b"):
        G = HostSim(boxes, [[0], [0, 1]], amr=True)
        d = str(tmp_path / tag)
        files, nbytes, sampled = bench.dump_outputs(G, d, True, 0)
        assert sampled and nbytes <= bench.DUMP_BUDGET_BYTES
        runs.append(load_dir(d))
    a, b = runs
    assert sorted(a) == sorted(b) and len(a) == 3 * 4 + 2
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
    # a box's share follows its size; every field of a box holds the same cells, distinct, inside the valid region
    assert a["lev1_box1_u"].shape[0] > a["lev1_box0_u"].shape[0] > 0
    for lev, bi, n in ((0, 0, 16), (1, 0, 8), (1, 1, 12)):
        u = a["lev%d_box%d_u" % (lev, bi)]
        cell = u[:, 0]
        i, j, k = cell % 1e3, (cell // 1e3) % 1e3, cell // 1e6
        assert len(set(cell.tolist())) == len(cell) and i.max() < n and j.max() < n and k.max() < n and min(i.min(), j.min(), k.min()) >= 0
        assert np.array_equal(a["lev%d_box%d_s" % (lev, bi)][:, 1], cell + 0.25 + 1e9)
        assert np.array_equal(a["lev%d_box%d_p" % (lev, bi)][:, 0], cell + 0.75)


def test_each_rank_writes_its_own_boxes(tmp_path):
    boxes = [box((x, 0, 0), 8) for x in (0, 8, 16, 24)]
    for rank, local in ((0, [0, 2]), (1, [1, 3])):
        bench.dump_outputs(HostSim(boxes, local, amr=False), str(tmp_path), False, rank)
    got = load_dir(str(tmp_path))
    assert sorted(got) == sorted(["dt", "time"] + ["lev0_box%d_%s" % (b, f) for b in range(4) for f in ("u", "s", "gp", "p")])


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_on_every_run(gpu, tmp_path):
    """two bench.py processes with the same arguments: the line reports the requested number of timed steps and their time per step, and
    the dumped state of the last timed step is the same bit for bit"""
    lines = []
    for tag in ("a", "b"):
        d = str(tmp_path / tag)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--box", "32", "--skip-cpu",
                              "--dump-outputs", d], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1, out.stdout
        lines.append(json.loads(js[0]))
    for ln in lines:
        assert ln["steps"] == 3 and ln["ms_per_step"] > 0
        assert ln["outputs_dumped"]["files"] == 6 and not ln["outputs_dumped"]["sampled"]
    a, b = load_dir(str(tmp_path / "a")), load_dir(str(tmp_path / "b"))
    assert sorted(a) == sorted(b) == sorted(["dt", "time", "lev0_box0_u", "lev0_box0_s", "lev0_box0_gp", "lev0_box0_p"])
    assert a["lev0_box0_u"].shape == (32, 32, 32, 3) and a["lev0_box0_p"].shape == (33, 33, 33, 1)
    for k in a:
        assert a[k].dtype == np.float64 and np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    assert np.abs(a["lev0_box0_u"]).max() > 0 and a["dt"][0] > 0
