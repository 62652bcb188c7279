#!/usr/bin/env python
"""Time a plot file and a checkpoint of the two-level 256^3 hierarchy (tests/golden/amr_grids_256_l2.json, 24 M cells) after two steps, written
  (a) by the library (plotfile.write_plotfile / write_checkfile on one rank: vdn_fabio_ml_multifab_write_d, vdn_checkpoint_write -- kk_fab_pack, one copy per range), and
  (b) by the Python reference path (_gather: one synchronous copy per box and source, np.concatenate, tobytes; write_ml_multifab) -- what ran before the library wrote.

    python tools/io_probe.py <output directory> [--rounds 3] [--library-only]

The two writers alternate in one process, one warm-up round and `--rounds` timed rounds each; medians and the spread are printed, everything written is
deleted.  --library-only (for a rocprofv3 --kernel-trace --stats run of its own: kk_fab_pack's time against 16 B per value) skips the Python path."""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reference_plotfile(sim, name):
    from varden_amd import advance as adv
    from varden_amd import boxlib as bl
    from varden_amd import plotfile as pf
    dm, ns = sim.dm, sim.nscal
    pd, nl = pf._domain(sim)
    ncomp = 2 * dm + ns + 2
    plot = [bl.MultiFab(sim.mla, n, ncomp, 0) for n in range(nl)]
    try:
        for n in range(nl):
            plot[n].copy_c(0, sim.uold[n], 0, dm)
            plot[n].copy_c(dm, sim.sold[n], 0, ns)
            adv.make_magvel(plot[n], dm + ns, sim.uold[n])
            adv.make_vorticity(plot[n], dm + ns + 1, sim.uold[n], sim.dx[n], sim.bct)
            plot[n].copy_c(dm + ns + 2, sim.gp[n], 0, dm)
        levels = pf._gather(sim, [plot])
    finally:
        for m in plot:
            m.destroy()
    dx0 = list(sim.dx[0][:dm])
    pf.write_ml_multifab(name, levels, [2] * (nl - 1), dm, pf.plot_names(dm, ns), pd, [0.0] * dm, [dx0[d] * (pd[1][d] + 1) for d in range(dm)], sim.time, dx0, nc=ncomp)
    pf.write_job_info(name, sim)


def reference_checkfile(sim, name):
    from varden_amd import plotfile as pf
    pd, nl = pf._domain(sim)
    os.makedirs(name)
    pf.write_ml_multifab(os.path.join(name, "State"), pf._gather(sim, [sim.uold, sim.sold, sim.gp]), [2] * (nl - 1), sim.dm, pd=pd, nc=2 * sim.dm + sim.nscal)
    pf.write_ml_multifab(os.path.join(name, "Pressure"), pf._gather(sim, [sim.p], (1, 1, 1)), [2] * (nl - 1), sim.dm, pd=pd, nc=1)
    with open(os.path.join(name, "Header"), "w") as f:
        f.write("&CHKPOINT\n TIME=%s,\n DT=%s,\n NLEVS=%d,\n /\n" % (pf._es(sim.time).strip(), pf._es(sim.dt).strip(), nl))
        for _ in range(nl - 1):
            f.write("%12d\n" % 2)


def tree_bytes(path):
    return sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(path) for f in fs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--library-only", action="store_true")
    args = ap.parse_args()
    from varden_amd import boxlib as bl
    from varden_amd import driver, plotfile
    from varden_amd.capi import default_params
    fine = [(tuple(b[0]), tuple(b[1])) for b in json.load(open(os.path.join(ROOT, "tests", "golden", "amr_grids_256_l2.json")))[0]]
    walls = [[15, 15]] * 3
    G = driver.VardenAMR(256, fine, walls, params=default_params(), init_shrink=0.1, init_iter=1, do_initial_projection=1, max_grid_size=256)
    G.step(); G.step()
    cells = [sum((h[0] - l[0] + 1) * (h[1] - l[1] + 1) * (h[2] - l[2] + 1) for l, h in lb) for lb in G.boxes]
    print("io_probe: two-level hierarchy, boxes per level %r, cells per level %r, after step %d" % ([len(b) for b in G.boxes], cells, G.istep))
    work = os.path.join(args.outdir, "io_probe_%d" % os.getpid())
    os.makedirs(work)
    writers = {"library": (lambda d: plotfile.write_plotfile(G, base=os.path.join(d, "plt")), lambda d: plotfile.write_checkfile(G, base=os.path.join(d, "chk")))}
    if not args.library_only:
        writers["python"] = (lambda d: reference_plotfile(G, os.path.join(d, "plt%05d" % G.istep)), lambda d: reference_checkfile(G, os.path.join(d, "chk%05d" % G.istep)))
    times = {(w, k): [] for w in writers for k in ("plotfile", "checkpoint")}
    size = {}
    try:
        for rnd in range(args.rounds + 1):                       # round 0 warms up (pinned buffer, page cache, imports)
            for w, (plt, chk) in writers.items():
                d = os.path.join(work, "%s_%d" % (w, rnd))
                os.makedirs(d)
                for kind, fn in (("plotfile", plt), ("checkpoint", chk)):
                    bl.capi.load().vdn_device_synchronize()
                    t0 = time.perf_counter()
                    fn(d)
                    dt = time.perf_counter() - t0
                    print("io_probe: round %d %-8s %-10s %8.3f s%s" % (rnd, w, kind, dt, "" if rnd else "   (warm-up)"), flush=True)
                    if rnd:
                        times[(w, kind)].append(dt)
                    size[kind] = tree_bytes(d) - (size["plotfile"] if kind == "checkpoint" else 0)
                shutil.rmtree(d)
        for kind in ("plotfile", "checkpoint"):
            row = {}
            for w in writers:
                t = times[(w, kind)]
                row[w] = statistics.median(t)
                print("io_probe: %-10s %-8s median %8.3f s   min %8.3f   max %8.3f   (%d rounds, %.2f GB, %.2f GB/s at the median)"
                      % (kind, w, row[w], min(t), max(t), len(t), size[kind] / 1e9, size[kind] / 1e9 / row[w]))
            if "python" in row:
                print("io_probe: %-10s python / library = %.2f" % (kind, row["python"] / row["library"]))
    finally:
        shutil.rmtree(work, ignore_errors=True)
        G.close()


if __name__ == "__main__":
    main()
