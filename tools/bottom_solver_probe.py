"""What do the Krylov bottom solvers (vdn_params.mg_bottom_solver / hg_bottom_solver, csrc/krylov_wg.h and csrc/krylov_grid.h) buy on sizes that are no power of two?
Ten advance steps of the inviscid bubble after two warm-up steps, on one box of 200^3 (multigrid bottom 25^3 cells / 26^3 nodes), 100^3 (the same bottom, one
level fewer) and 256^3 (the control: bottom 2^3, where the bottom solve is 8 sweeps of 8 cells), each with the bottom sweeps (-1 / -1) and with CG (2 / 2):
wall time and phase times per step, V-cycles of the step's MAC and HG solves, the bottom statistics of the last solves and the form their bottom took
(vdn_last_bottom_form: 0 sweeps, 1 one workgroup, 2 the whole GPU; "-" on a library older than that entry point).
dm = 2 (csrc/dim2.hip): the same on one box of 200^2 (bottom 25^2 cells / 26^2 nodes, which the sweeps visit with two to four launches per sweep), 100^2 and
the control 128^2 (bottom 2^2).
Large bottom levels (profiles/bottom_solver_probe_wide.txt): sizes 150 and 300 (bottom 75^3 cells), 250 (125^3), with rows = cg -- the bottom sweeps take
max(8, N^2) = 5625 sweeps of 75^3 cells per V-cycle there, minutes per step.  The crossover between the two Krylov forms: sizes 34, 50, 66, 90 (bottoms 17^3,
25^3, 33^3, 45^3 cells), rows = cg, once with a library built with -DVDN_KRYLOV_GRID_MIN_POINTS=1073741824 (always one workgroup) and once with
-DVDN_KRYLOV_GRID_MIN_POINTS=0 (always the whole GPU); `lib` names the library to load instead of the package's.
Large bottom levels, dm = 2 (profiles/bottom_solver_probe_2d_wide.txt): sizes 150, 300 (bottom 75^2 cells), 1000 (125^2), 3000 (375^2) and the controls 128
and 200, dm = 2, rows = cg, this build and the parent commit's library in turn.  Their crossover: sizes 102, 142, 154, 162, 170, 182, 202, 282 (bottoms 51^2
.. 141^2 cells), the library built with -DVDN_KRYLOV_GRID_MIN_POINTS_2D=1073741824 and with =0.
usage: python tools/bottom_solver_probe.py [sizes, default 200,100,256 -- dm = 2: 200,100,128] [nsteps=10] [dm=3] [rows=both|cg|sweeps] [lib]
       (output: profiles/bottom_solver_probe.txt; dm = 2: profiles/bottom_solver_probe_2d.txt)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from varden_amd import advance as adv, capi, driver              # noqa: E402
from varden_amd.capi import default_params                       # noqa: E402

dm = int(sys.argv[3]) if len(sys.argv) > 3 else 3
sizes = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 and sys.argv[1] else ([200, 100, 256] if dm == 3 else [200, 100, 128])
ns = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rows = {"both": ((-1, -1), (2, 2)), "cg": ((2, 2),), "sweeps": ((-1, -1),)}[sys.argv[4] if len(sys.argv) > 4 else "both"]
if len(sys.argv) > 5:
    capi.LIB_PATH = os.path.abspath(sys.argv[5])
form = (lambda w: str(adv.last_bottom_form(w))) if hasattr(adv, "last_bottom_form") else (lambda w: "-")
W = [[15, 15]] * dm + [[0, 0]] * (3 - dm)
print("bottom_solver_probe: dm = %d, inviscid bubble, walls, one box, %d timed steps after 2 warm-up steps; times in ms per step; library %s" % (dm, ns, os.path.basename(capi.LIB_PATH)), flush=True)
for n in sizes:
    res = {}
    for mg, hg in rows:
        G = driver.Varden(n, W, default_params(dm=dm, cflfac=0.9, mg_bottom_solver=mg, hg_bottom_solver=hg), prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1, swap_state=True)
        for _ in range(2):
            G.step()
        capi.check(capi.load().vdn_device_synchronize())
        t0 = time.perf_counter()
        ph = dict(scalar=0.0, velocity=0.0, mac=0.0, hg=0.0, total=0.0)
        cyc = dict(mac=[], hg=[])
        bot, its = {}, dict(mac=[], hg=[])
        for _ in range(ns):
            G.step()
            for k, v in adv.last_step_timing().items():
                ph[k] += v
            for w in ("mac", "hg"):
                cyc[w].append(adv.last_solver_stats(w)[0])
                bot[w] = adv.last_bottom_stats(w)
                its[w].append(bot[w]["iters"] / max(bot[w]["calls"], 1))
        capi.check(capi.load().vdn_device_synchronize())
        el = time.perf_counter() - t0
        res[(mg, hg)] = 1e3 * el / ns
        print("n %4d  mg/hg_bottom_solver %2d/%2d : %9.2f ms per step | phases %s | V-cycles mac %s hg %s | bottom (last solve) mac %s hg %s | iterations per visit mac %.1f hg %.1f | form mac %s hg %s"
              % (n, mg, hg, 1e3 * el / ns, " ".join("%s %.2f" % (k, 1e3 * v / ns) for k, v in ph.items()),
                 ",".join(str(c) for c in cyc["mac"]), ",".join(str(c) for c in cyc["hg"]),
                 " ".join("%s %d" % kv for kv in bot["mac"].items()), " ".join("%s %d" % kv for kv in bot["hg"].items()),
                 sum(its["mac"]) / ns, sum(its["hg"]) / ns, form("mac"), form("hg")), flush=True)
        G.close()
    if len(rows) == 2:
        print("n %4d  CG / sweeps: %.3f" % (n, res[(2, 2)] / res[(-1, -1)]), flush=True)
