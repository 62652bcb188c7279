#!/usr/bin/env python
"""What one call of the run diagnostics costs (vdn_diagnostics, csrc/diag.hip), wall-clock per call (every call ends in its one read-back), on

  one      a 256^3 level in one box
  amr3     the three-level hierarchy of tests/golden/amr_grids_256_l3.json (a 256^3 base in one box, 263 and 997 boxes above it)

next to two other ways to look at the same fields:

  (a) diagnostics, vort=False      the composite integrals, extrema and the finite check
  (b) diagnostics, vort=True       ... with enstrophy and the vorticity's extrema
  (c) norm_inf of u and of s       the library's plain max |f| passes (k_absmax) over every level: the same bytes, one quantity, no mask
  (d) host copy + numpy            what the long-run tools do: to_numpy() of every box, then min, max, sum and isfinite().all() of the valid cells per component

The bytes a call must read are (dm + nscal) * 8 B per composite cell; the table gives them per second and as a fraction of the 8 TB/s HBM peak the README uses.
The fields are constants set on the device: the time of none of the four depends on the values.

    python tools/diag_probe.py [--repeats 5] [--grids one,amr3] [--no-host] [--out profiles/diag_probe.txt]
    python tools/diag_probe.py --lib <libvarden_amd.so of another build> --only-host      # (c), (d) on a build without the entry, e.g. the parent commit's"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grids", default="one,amr3")
    ap.add_argument("--lib", default=None, help="another build of libvarden_amd.so")
    ap.add_argument("--only-host", action="store_true", help="(c) and (d) only: a build without vdn_diagnostics")
    ap.add_argument("--no-host", action="store_true", help="leave (d) out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from varden_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    if a.only_host:
        for name in ("vdn_diagnostics", "vdn_diag_sizeof"):
            capi.SIGNATURES.pop(name)
    from varden_amd import advance as adv, boxlib as bl
    prm = capi.default_params()
    dm, ns = prm.dm, prm.nscal
    bl.initialize(prm, 0, 1, 0)
    walls = [[bl.NO_SLIP_WALL] * 2] * 3
    n = 256
    text = []
    for grid in a.grids.split(","):
        boxes = [[((0, 0, 0), (n - 1,) * 3)]]
        if grid == "amr3":
            boxes += [[(tuple(b[0]), tuple(b[1])) for b in lev] for lev in json.load(open(os.path.join(ROOT, "tests", "golden", "amr_grids_256_l3.json")))]
        NL = len(boxes)
        mla = bl.MLLayout([((0, 0, 0), ((n << l) - 1,) * 3) for l in range(NL)], boxes, rr=[(2, 2, 2)] * (NL - 1))
        bct = bl.BCTower(mla, walls)
        dx = [[1.0 / (n << l)] * 3 for l in range(NL)]
        u, s = [bl.MultiFab(mla, l, dm, 1) for l in range(NL)], [bl.MultiFab(mla, l, ns, 1) for l in range(NL)]
        for l in range(NL):
            for c in range(dm):
                u[l].setval(0.25 * (c + 1) - 0.5, c, 1, all=True)
            for c in range(ns):
                s[l].setval(1.0 + 0.5 * c, c, 1, all=True)

        def host():
            out = []
            for mfs in (u, s):
                for mf in mfs:
                    for i in range(mf.nfabs()):
                        v = mf.to_numpy(i)[1:-1, 1:-1, 1:-1]
                        out.append([(v[..., c].min(), v[..., c].max(), v[..., c].sum()) for c in range(mf.nc)] + [np.isfinite(v).all()])
            return out
        runs = []
        if not a.only_host:
            runs += [("(a) diagnostics, vort=False", lambda: adv.diagnostics(mla, u, s, dx, bct, vort=False)),
                     ("(b) diagnostics, vort=True", lambda: adv.diagnostics(mla, u, s, dx, bct, vort=True))]
        runs += [("(c) norm_inf of u and s, every level", lambda: [m.norm_inf() for m in u + s])]
        if not a.no_host:
            runs += [("(d) to_numpy of every box + numpy", host)]
        res = {name: fn() for name, fn in runs}                                           # warm-up (and the results)
        times = {name: [] for name, _ in runs}
        for r in range(a.repeats):
            for name, fn in runs[r % len(runs):] + runs[:r % len(runs)]:
                capi.check(capi.load().vdn_device_synchronize())
                t0 = time.perf_counter()
                fn()
                times[name].append(1e3 * (time.perf_counter() - t0))
        if a.only_host:                                                                   # the composite cells from the box lists
            cells = sum(int(np.prod([hi[k] - lo[k] + 1 for k in range(3)])) for lev in boxes for lo, hi in lev)
            cells -= sum(int(np.prod([hi[k] - lo[k] + 1 for k in range(3)])) // 8 for lev in boxes[1:] for lo, hi in lev)
        else:
            d = res[runs[0][0]]
            cells = d["cells"]
            assert d["nonfinite"] == 0 and abs(d["volume"] - 1.0) < 1e-9 and res[runs[1][0]]["cells"] == cells
        nbytes = (dm + ns) * 8 * cells
        text += ["diag_probe %s: %d level(s), boxes %s, %d composite cells, (dm + nscal) * 8 B * cells = %.1f MB; %d timed calls each after a warm-up; library %s (%s)"
                 % (grid, NL, [len(b) for b in boxes], cells, nbytes / 1e6, a.repeats, os.path.relpath(capi.LIB_PATH, ROOT), capi.load().vdn_build_flavour().decode()),
                 "%-40s %9s %9s %9s %9s %9s" % ("", "median ms", "min ms", "max ms", "GB/s", "of peak")]
        for name, _ in runs:
            t = times[name]
            gbs = nbytes / (1e-3 * statistics.median(t)) / 1e9
            text.append("%-40s %9.3f %9.3f %9.3f %9.1f %9.4f" % (name, statistics.median(t), min(t), max(t), gbs, gbs * 1e9 / HBM_PEAK))
        text.append("")
        for m in u + s:
            m.destroy()
        bct.destroy()
        mla.destroy()
    print("\n".join(text))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
