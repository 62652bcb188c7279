"""What do the Krylov bottom solvers (vdn_params.mg_bottom_solver / hg_bottom_solver, csrc/krylov_wg.h) buy on sizes that are no power of two?
Ten advance steps of the inviscid bubble after two warm-up steps, on one box of 200^3 (multigrid bottom 25^3 cells / 26^3 nodes), 100^3 (the same bottom, one
level fewer) and 256^3 (the control: bottom 2^3, where the bottom solve is 8 sweeps of 8 cells), each with the bottom sweeps (-1 / -1) and with CG (2 / 2):
wall time and phase times per step, V-cycles of the step's MAC and HG solves, the bottom statistics of the last solves.
dm = 2 (csrc/dim2.hip): the same on one box of 200^2 (bottom 25^2 cells / 26^2 nodes, which the sweeps visit with two to four launches per sweep), 100^2 and
the control 128^2 (bottom 2^2).
usage: python tools/bottom_solver_probe.py [sizes, default 200,100,256 -- dm = 2: 200,100,128] [nsteps=10] [dm=3]
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
W = [[15, 15]] * dm + [[0, 0]] * (3 - dm)
print("bottom_solver_probe: dm = %d, inviscid bubble, walls, one box, %d timed steps after 2 warm-up steps; times in ms per step" % (dm, ns), flush=True)
for n in sizes:
    res = {}
    for mg, hg in ((-1, -1), (2, 2)):
        G = driver.Varden(n, W, default_params(dm=dm, cflfac=0.9, mg_bottom_solver=mg, hg_bottom_solver=hg), prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1, swap_state=True)
        for _ in range(2):
            G.step()
        capi.check(capi.load().vdn_device_synchronize())
        t0 = time.perf_counter()
        ph = dict(scalar=0.0, velocity=0.0, mac=0.0, hg=0.0, total=0.0)
        cyc = dict(mac=[], hg=[])
        bot = {}
        for _ in range(ns):
            G.step()
            for k, v in adv.last_step_timing().items():
                ph[k] += v
            for w in ("mac", "hg"):
                cyc[w].append(adv.last_solver_stats(w)[0])
                bot[w] = adv.last_bottom_stats(w)
        capi.check(capi.load().vdn_device_synchronize())
        el = time.perf_counter() - t0
        res[(mg, hg)] = 1e3 * el / ns
        print("n %4d  mg/hg_bottom_solver %2d/%2d : %9.2f ms per step | phases %s | V-cycles mac %s hg %s | bottom (last solve) mac %s hg %s"
              % (n, mg, hg, 1e3 * el / ns, " ".join("%s %.2f" % (k, 1e3 * v / ns) for k, v in ph.items()),
                 ",".join(str(c) for c in cyc["mac"]), ",".join(str(c) for c in cyc["hg"]),
                 " ".join("%s %d" % kv for kv in bot["mac"].items()), " ".join("%s %d" % kv for kv in bot["hg"].items())), flush=True)
        G.close()
    print("n %4d  CG / sweeps: %.3f" % (n, res[(2, 2)] / res[(-1, -1)]), flush=True)
