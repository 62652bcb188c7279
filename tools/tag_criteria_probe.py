#!/usr/bin/env python
"""What tagging by criteria costs: make_new_grids on ONE 256^3 level in one box (walls), wall-clock per call (every call ends in a stream synchronise and the
host clustering), `--repeats` timed calls of each after one warm-up, the four measurements taking turns round by round in a rotating order:

  (a) vdn_make_new_grids                  the reference rule of prob_type 1 (rho > 1.01), kk_tag
  (b) vdn_make_new_grids_by, scalar       the same rule as a criterion, kk_tag_by<scalar>: the same boxes
  (c) vdn_make_new_grids_by, vorticity    |curl u| > threshold evaluated inside the tagging pass
  (d) the unfused route to (c)            vdn_make_vorticity into a multifab, then a scalar criterion on it: the same boxes as (c)

    python tools/tag_criteria_probe.py [--n 256] [--repeats 5] [--out profiles/tag_criteria_probe.txt]
    python tools/tag_criteria_probe.py --lib <libvarden_amd.so of another build> --only-a      # (a) on a build without the two entries, e.g. the parent commit's

Prints one table (median, min, max in ms; boxes and tagged cells) and, with --out, appends it to that file."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libvarden_amd.so for (a)")
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from varden_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    if a.only_a:                                   # a build from before the two entries existed
        for name in ("vdn_tag_boxes_by", "vdn_make_new_grids_by"):
            capi.SIGNATURES.pop(name)
    from varden_amd import advance as adv, boxlib as bl
    from varden_amd.driver import initdata_numpy
    n, h = a.n, 1.0 / a.n
    bl.initialize(capi.default_params(), 0, 1, 0)
    walls = [[bl.NO_SLIP_WALL] * 2] * 3
    mla = bl.MLLayout([((0, 0, 0), (n - 1,) * 3)], [[((0, 0, 0), (n - 1,) * 3)]])
    bct = bl.BCTower(mla, walls)
    s, u, w = bl.MultiFab(mla, 0, 2, 0), bl.MultiFab(mla, 0, 3, 1), bl.MultiFab(mla, 0, 1, 0)
    s.from_numpy(initdata_numpy((n,) * 3, [h] * 3, 1, 3, 2)[1][3:-3, 3:-3, 3:-3])           # the bubble's density
    ax = h * (np.arange(n + 2) - 0.5)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    ua = np.zeros(X.shape + (3,), order="F")
    ua[..., 0] = np.tanh((Y - 0.5 - 0.1 * np.sin(2.0 * np.pi * Z)) / 0.05)            # a bent shear layer: a sheet of vorticity
    ua[..., 1] = 0.1 * np.sin(2.0 * np.pi * X)
    u.from_numpy(ua)
    del X, Y, Z, ua
    cl = dict(buf_wid=2, nest=0, min_eff=0.9, min_width=4, blocking=4, max_grid_size=128, maxboxes=65536)
    rho_rule = [dict(field="scalar", comp=1, gt=1.01)]
    vort_rule = [dict(field="vorticity", gt=10.0)]
    vort_as_scalar = [dict(field="scalar", comp=1, gt=10.0)]
    rho_rule, vort_rule, vort_as_scalar = (adv.tag_criteria(c)[0] for c in (rho_rule, vort_rule, vort_as_scalar))      # converted once, as the drivers do

    def unfused():
        adv.make_vorticity(w, 0, u, [h] * 3, bct)
        return adv.make_new_grids_by(w, None, None, None, 1, vort_as_scalar, **cl)
    runs = [("(a) make_new_grids, reference rule", lambda: adv.make_new_grids(s, 1, **cl))]
    if not a.only_a:
        runs += [("(b) make_new_grids_by, scalar criterion", lambda: adv.make_new_grids_by(s, None, None, None, 1, rho_rule, **cl)),
                 ("(c) make_new_grids_by, vorticity criterion", lambda: adv.make_new_grids_by(s, u, [h] * 3, bct, 1, vort_rule, **cl)),
                 ("(d) make_vorticity + scalar criterion on it", unfused)]
    res = {name: fn() for name, fn in runs}                                            # warm-up (and the results)
    times = {name: [] for name, _ in runs}
    for r in range(a.repeats):
        for name, fn in runs[r % len(runs):] + runs[:r % len(runs)]:                   # the order rotates: every measurement follows every other one
            capi.check(capi.load().vdn_device_synchronize())
            t0 = time.perf_counter()
            fn()
            times[name].append(1e3 * (time.perf_counter() - t0))
    if not a.only_a:
        assert res[runs[1][0]] == res[runs[0][0]], "(b) differs from (a)"
        assert res[runs[3][0]] == res[runs[2][0]], "(d) differs from (c)"
    lines = ["tag_criteria_probe: one %d^3 level in one box, %d timed calls each after a warm-up, ms per call; library %s (%s)"
             % (n, a.repeats, os.path.relpath(capi.LIB_PATH, ROOT), capi.load().vdn_build_flavour().decode()),
             "%-46s %9s %9s %9s %7s %10s" % ("", "median", "min", "max", "boxes", "tagged")]
    for name, _ in runs:
        t = times[name]
        lines.append("%-46s %9.3f %9.3f %9.3f %7d %10d" % (name, statistics.median(t), min(t), max(t), len(res[name][0]), res[name][1]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n\n")
    for m in (s, u, w):
        m.destroy()
    bct.destroy()
    mla.destroy()


if __name__ == "__main__":
    main()
