"""dm = 2 on box lists: the 1024^2 bubble (walls, inviscid) cut into nb x nb boxes, the start-up sequence and one step, then three timed steps.
Run plain for the step time, under `rocprofv3 --kernel-trace --stats -- python tools/probes/dim2_boxlists_probe.py nb` for the launches per step
(profiles/dim2_boxlists_1024.txt).  argv: nb (boxes per direction, default 1)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from varden_amd import driver  # noqa: E402
from varden_amd.capi import default_params  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 1
n = 1024
G = driver.Varden(n, [[15, 15], [15, 15], [0, 0]], default_params(dm=2, cflfac=0.9), prob_type=1, init_shrink=0.1, init_iter=1, decomp=(nb, nb, 1))
G.step()
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    G.step()
    ts.append(time.perf_counter() - t0)
print("boxes %d: step %.2f ms (min of 3), steps %s" % (nb * nb, 1e3 * min(ts), ["%.2f" % (1e3 * t) for t in ts]))
G.close()
