#!/usr/bin/env python
"""bench.py -- cells*steps/sec of advance_timestep on the MI355X-native hot path.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config 256|512|amr2|amr3] [--scaling weak|strong] [--dump-outputs DIR] [--full]

A plain run sets the workload up, runs W warm-up and K timed steps, writes --dump-outputs and prints the line: `value` and `ms_per_step`
are the timed steps, `config` their phase split, V-cycle counts and transport traffic.  Everything else the bench measures runs with
`--full` only (the line's `roofline`, `cpu_baseline`, `extra_workloads` and `config.one_box_512` are null / empty without it).

`--gpus N` with N > 1 STARTS ITS OWN N RANKS: the parent process touches neither torch.cuda nor HIP, spawns N children (one per
GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in their environment), waits for them and exits with their code;
rank 0 prints the one JSON line.  Under torchrun (WORLD_SIZE already set) the process is one of the ranks and spawns nothing.

Workloads (BASELINE.json `configs`; every run: variable-density bubble of src/initdata.f90:212-238, no-slip walls, gravity -9.8,
cflfac 0.9, init_shrink 0.1, init_iter 1, MAC + HG projection every step, exec/test/inputs_bubble_3d with visc_coef = 0):
  256  (default)  configs[1]: 3-D 256^3, one level, one 256^3 box per GPU.  N > 1: weak scaling, the domain grows 2x1x1 / 2x2x1 /
                  2x2x2 (N = 8 is the 512^3 case of configs[2]).
  512             configs[2] / the north star's single-GPU case: 512^3, one level, max_grid_size 256 => eight 256^3 boxes dealt
                  round-robin to the N ranks (N = 1: all eight on one GPU).  `--scaling strong` selects it for any N: the global
                  problem is fixed, so the per-N values give the strong-scaling curve.
  amr2            configs[3]: 256^3 base + one refined level over the cells tagged rho > 1.01 (tag_boxes.f90:65-75), grids built
                  once and fixed (initialize.f90:93-150); boxes dealt to the ranks by cell count.
  amr3            configs[4]: 256^3 base + two refined levels (rho > 1.01, rho > 1.1); N > 1: the base level is cut into 128^3
                  boxes so that every level can be dealt to the ranks.
A "step" = one pass of the reference's time-loop body (src/varden.f90:291-328): ghost fills, estdt, advance_timestep, uold<-unew.
All state is resident in HBM before the timed region.

With `--full`: `roofline` is the MAC-multigrid red-black Gauss-Seidel colour pass on the finest level (48 algorithmic B/cell/pass; round 5: the level by colour),
timed with HIP events on the launch stream inside the library, its HBM bytes per launch measured in the same run by two rocprofv3 --pmc child passes; `cpu_baseline` is the CPU oracle (a port, OpenMP) on a bounded
sample of the same workload, with the survey's per-core timing of the reference's own Godunov kernels quoted next to it.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

def measure_pass_traffic(kernel_substr, timeout_s=240):
    """HBM bytes per launch of the roofline kernel, MEASURED NOW: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE as two child runs of tools/smoother_probe.py
    (the same kernel on the same 256^3 data as the timed probe; counters in passes of their own, as MI355X_MICROARCH.md prescribes), per-launch means over its
    24 dispatches, bytes = (2 x FETCH_SIZE + WRITE_SIZE) KB (the guide's gfx950 correction for streaming reads).  None when rocprofv3 is missing or a pass fails."""
    import csv, glob, shutil, tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    # under an outer profiler (rocprofv3 ... -- python3 bench.py) the child passes would inherit its preloaded tool library and contend with its trace: skip
    if any(k.startswith("ROCP") or k.startswith("ROCPROF") for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        print("bench: running under a profiler -- roofline.traffic is not measured in this run", file=sys.stderr)
        return None
    out = tempfile.mkdtemp(prefix="vdn_pmc_", dir="/tmp")
    means = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(out, ctr)
            # the pass in a session of its own: on a timeout the whole process group goes (rocprofv3 AND the probe it started -- an orphaned probe would keep
            # the GPU busy under the timings that follow)
            pr = subprocess.Popen([exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--",
                                   sys.executable, os.path.join(ROOT, "tools", "smoother_probe.py"), "256", "20"],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=dict(os.environ, TMPDIR="/tmp"), start_new_session=True)
            try:
                _, err_ = pr.communicate(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                import signal
                os.killpg(pr.pid, signal.SIGKILL)          # the exact group this call started
                pr.communicate()
                raise
            if pr.returncode != 0:
                raise RuntimeError("rocprofv3 --pmc %s failed (%d): %s" % (ctr, pr.returncode, (err_ or "")[-200:]))
            tot = cnt = 0
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if kernel_substr in r["Kernel_Name"] and r["Counter_Name"] == ctr:
                        tot += float(r["Counter_Value"]); cnt += 1
            if cnt == 0:
                return None
            means[ctr] = tot / cnt
        return int(round((2.0 * means["FETCH_SIZE"] + means["WRITE_SIZE"]) * 1024)), means
    except Exception as e:                                   # (a missing profiler or a failed pass must not fail the bench line)
        print("bench: traffic not measured in this run (%s)" % (str(e)[:200],), file=sys.stderr)
        return None
    finally:
        shutil.rmtree(out, ignore_errors=True)


HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# the reference's own velpred + mkflux (scalars, velocity) + update, flang -O2, ONE core, 128^3: 2.91 s per
# step of advection alone => 0.72 Mcells/s/core (no forcing, no ghost fills, no multigrid): an upper bound on the reference's
# per-core advance_timestep rate
REF_GODUNOV_MCELLS_PER_CORE = 0.72


def godunov_calibration(vo, n=128):
    """BASELINE.md 1b on the oracle: velpred (3 comps) + mkflux (scalars, velocity) + update (u + s) on ONE box of n^3, interior
    (periodic) BCs, smooth velocity + the bubble density, dt = 0.4 dx, ONE thread -- the calls the survey timed in the reference's own
    Fortran kernels (2.91 s at 128^3 on one core of the survey container).  Returns the seconds per call (second call of each: the first
    one pays the page faults of the work arrays)."""
    import ctypes as C
    import numpy as np
    from varden_amd.capi import default_params
    try:
        C.CDLL("libgomp.so.1").omp_set_num_threads(1)
    except OSError:
        pass
    L = vo.lib()
    prm = default_params()
    phys = [[vo.PERIODIC, vo.PERIODIC]] * 3
    bc, pm = vo.make_bc(phys, 3, 2), vo.ivec([1, 1, 1])
    lo, hi = (0, 0, 0), (n - 1,) * 3
    dx = vo.dvec([1.0 / n] * 3)
    u, s = vo.Fab(lo, hi, 3, 3), vo.Fab(lo, hi, 3, 2)
    x = (np.arange(-3, n + 3) + 0.5) / n
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    u.a[..., 0] = np.sin(2 * np.pi * X) * np.cos(2 * np.pi * Y)
    u.a[..., 1] = -np.cos(2 * np.pi * X) * np.sin(2 * np.pi * Y) * np.cos(2 * np.pi * Z)
    u.a[..., 2] = 0.3 * np.sin(2 * np.pi * Z)
    r = np.sqrt((X - .5) ** 2 + (Y - .5) ** 2 + (Z - .5) ** 2)
    s.a[..., 0] = 1 + 0.5 * 9 * (1 - np.tanh(30 * (r - 0.1)))
    s.a[..., 1] = s.a[..., 0]

    def faces(ng, nc, val=0.0):
        return [vo.Fab(lo, hi, ng, nc, tuple(1 if t == d else 0 for t in range(3)), val) for d in range(3)]
    fu, fs, mac_rhs = vo.Fab(lo, hi, 1, 3), vo.Fab(lo, hi, 1, 2), vo.Fab(lo, hi, 1, 1)
    um, se, fl, ue, uf = faces(1, 1, 1e20), faces(0, 2), faces(0, 2), faces(0, 3), faces(0, 3)
    un, sn = vo.Fab(lo, hi, 3, 3), vo.Fab(lo, hi, 3, 2)
    dt = C.c_double(0.4 / n)
    P = vo.fab_ptr_array
    calls = {
        "velpred": lambda: L.vo_velpred(u.ref, P(um), fu.ref, dx, dt, C.byref(bc), C.byref(prm)),
        "mkflux_scalars": lambda: L.vo_mkflux(s.ref, P(se), P(fl), P(um), fs.ref, mac_rhs.ref, dx, dt, 0, vo.ivec([1, 0]), 3, C.byref(bc), C.byref(prm)),
        "mkflux_velocity": lambda: L.vo_mkflux(u.ref, P(ue), P(uf), P(um), fu.ref, mac_rhs.ref, dx, dt, 1, vo.ivec([0, 0, 0]), 0, C.byref(bc), C.byref(prm)),
        "update": lambda: (L.vo_update(s.ref, P(um), P(se), P(fl), fs.ref, sn.ref, dx, dt, 0, vo.ivec([1, 0])),
                           L.vo_update(u.ref, P(um), P(ue), P(uf), fu.ref, un.ref, dx, dt, 1, vo.ivec([0, 0, 0]))),
    }
    out = {}
    for name, f in calls.items():
        f()
        if name == "velpred":
            for m in um:
                L.vo_fill_boundary(m.ref, pm)
        t0 = time.perf_counter()
        f()
        out[name] = round(time.perf_counter() - t0, 3)
    return out


DUMP_BUDGET_BYTES = 60 << 20     # what --dump-outputs writes in all (ranks included), below 64 MB with room for the .npy headers and dt / time


def dump_outputs(G, outdir, amr, rank):
    """--dump-outputs: the state the timed path hands its caller after the last timed step -- new velocity `u`, new scalars `s`
    (rho, tracer), pressure gradient `gp` on the valid cells, nodal pressure `p`, and `dt` / `time` -- as float64 .npy files
    lev<L>_box<B>_<field>.npy (B: the box's global index on level L; every rank writes the boxes it owns, rank 0 dt.npy and time.npy).
    When the whole valid region of every box fits in DUMP_BUDGET_BYTES the fields are written whole, shape (nx, ny, nz, nc) (p: its
    valid nodes, (nx+1, ny+1, nz+1, 1)).  Otherwise each box contributes a share of a fixed number of cells proportional to its size,
    drawn without replacement by a generator seeded with (level, box) and sorted, shape (k, nc), p at each sampled cell's low node:
    the same cells on every run with the same arguments.  Returns (files, bytes, sampled) of this rank."""
    import numpy as np
    levels = G.boxes if amr else [G.boxes]
    local = G.local if amr else [G.local]
    fields = (("u", G.uold), ("s", G.sold), ("gp", G.gp), ("p", G.p))     # (after a swap_state step uold / sold hold the new state)
    ncc = sum(mfs[0].nc for name, mfs in fields if name != "p")        # cell-centred components per cell
    size = [[tuple(b[1][d] - b[0][d] + 1 for d in range(3)) for b in lb] for lb in levels]
    cells = sum(int(np.prod(sz)) for ls in size for sz in ls)
    nodes = sum(int(np.prod([x + 1 for x in sz])) for ls in size for sz in ls)
    budget = DUMP_BUDGET_BYTES - 16                                      # (dt and time)
    whole = 8 * (ncc * cells + nodes) <= budget
    npoints = budget // (8 * (ncc + 1))                                  # sampled cells in all (one p value per cell)
    os.makedirs(outdir, exist_ok=True)
    files = nbytes = 0

    def save(name, a):
        nonlocal files, nbytes
        a = np.ascontiguousarray(a, dtype=np.float64)
        np.save(os.path.join(outdir, name + ".npy"), a)
        files, nbytes = files + 1, nbytes + a.nbytes

    for lev in range(len(levels)):
        for li, gi in enumerate(local[lev]):
            sz = size[lev][gi]
            ncell = int(np.prod(sz))
            idx = None
            if not whole:
                k = min(ncell, npoints * ncell // cells)
                idx = np.unravel_index(np.sort(np.random.default_rng([lev, gi]).choice(ncell, k, replace=False)), sz)
            for name, mfs in fields:
                mf = mfs[lev]
                a = mf.to_numpy(li)
                g = mf.ng
                if whole:
                    v = a[g:a.shape[0] - g, g:a.shape[1] - g, g:a.shape[2] - g]
                else:
                    v = a[idx[0] + g, idx[1] + g, idx[2] + g]
                save("lev%d_box%d_%s" % (lev, gi, name), v)
    if rank == 0:
        save("dt", np.array([G.dt]))
        save("time", np.array([G.time]))
    return files, nbytes, not whole


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default=os.environ.get("VDN_BENCH_CONFIG", "256"), choices=["256", "512", "amr2", "amr3"])
    ap.add_argument("--scaling", default=os.environ.get("VDN_BENCH_SCALING", "weak"), choices=["weak", "strong"])
    ap.add_argument("--box", dest="n", type=int, default=256, help="box width (256/512) or base-level width (amr2/amr3)")
    ap.add_argument("--full", action="store_true", help="after the timed steps also run the CPU baseline against the oracle, the roofline probe, the extra workloads "
                    "and the 512 config's one-box companion (--cpu-box, --cpu-steps, --skip-cpu, --no-calib, --no-cpu256, --no-pmc and --no-extra shape these legs)")
    ap.add_argument("--cpu-box", dest="cpu_n", type=int, default=0, help="width of the CPU sample (0: 128, or 64 for amr)")
    ap.add_argument("--cpu-steps", dest="cpu_steps", type=int, default=3, help="timed oracle steps of the cpu_baseline leg (the median is reported; each is compared with the GPU)")
    ap.add_argument("--skip-cpu", dest="no_cpu", action="store_true")
    ap.add_argument("--hg-fmg", dest="hg_fmg", type=int, default=1, choices=[0, 1], help="nested-iteration start of the nodal solve (vdn_params.hg_fmg; 0: the zero guess of rounds 1-2)")
    ap.add_argument("--mac-fmg", dest="mac_fmg", type=int, default=1, choices=[0, 1], help="nested-iteration start of the MAC solve (vdn_params.mac_fmg; 0: the zero guess)")
    ap.add_argument("--hg-pre-pair", dest="hg_pre_pair", type=int, default=1, choices=[0, 1], help="two-step damping of the nodal V-cycle's pre-smoothing sweeps (vdn_params.hg_omega_pre1 / 2; 0: hg_omega for both)")
    ap.add_argument("--no-calib", dest="no_calib", action="store_true", help="skip the one-thread Godunov calibration of the cpu_baseline leg")
    ap.add_argument("--no-cpu256", dest="no_cpu256", action="store_true", help="skip cpu_baseline.sample_256 (one oracle step at the headline size, about 20 s with its start-up)")
    ap.add_argument("--no-pmc", dest="no_pmc", action="store_true", help="do not measure roofline.traffic in this run (two rocprofv3 --pmc child passes on tools/smoother_probe.py); "
                    "the committed counter summary is quoted instead.  Needed when bench.py itself runs under rocprofv3")
    ap.add_argument("--no-extra", dest="no_extra", action="store_true", help="skip the extra_workloads (512^3 in eight boxes and in one box, tagged two- and three-level hierarchies, the viscous 256^3 step, the viscous three-level run with regridding) of the --full N = 1 line")
    ap.add_argument("--dump-outputs", dest="dump_dir", default=None, metavar="DIR",
                    help="after the timed steps write the state the last one computed (u, s, gp, p, dt, time) to DIR/<name>.npy, float64, at most 64 MB in all "
                         "(a fixed, seeded sample of cells when the fields are larger): two builds run with the same arguments can be compared output for output.  "
                         "bench_outputs/ inside the tree is git-ignored")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def spawn_ranks(args):
    """start one child per GPU; this process never initialises the GPU (no torch import, no HIP call)"""
    n = args.gpus
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                r = p.poll()
                if r is None:
                    continue
                pending.remove(p)
                if r != 0 and rc == 0:
                    rc = r
                    for q in pending:          # a rank died: the others would wait in a collective forever
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:                        # exact PIDs of the children started above
            if p.poll() is None:
                p.kill()
    return rc


def main():
    args = parse_args()
    # the one-GPU rehearsals of the N > 1 transport (packed buffers through a 1-rank RCCL communicator; every rank on GPU 0 over the RCCL test double) are switches
    # of the TESTING build of the library; a plain run loads the product, which reads no environment variable
    if os.environ.get("VDN_FORCE_PACKED") or os.environ.get("VDN_BENCH_ONE_DEVICE") == "1" or os.environ.get("VDN_RCCL_LIB"):
        os.environ.setdefault("VDN_LIB_FLAVOUR", "testing")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args))
    if args.scaling == "strong" and args.config == "256":
        args.config = "512"
    if args.config == "512":
        args.scaling = "strong"

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert args.gpus in (1, world), "--gpus %d but WORLD_SIZE=%d" % (args.gpus, world)
    one_dev = os.environ.get("VDN_BENCH_ONE_DEVICE") == "1"     # debugging aid: every rank on GPU 0, gloo control plane, RCCL test double
    if one_dev:
        local_rank = 0
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if one_dev:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    assert torch.cuda.is_available(), "bench.py needs a GPU: the product path has no CPU fallback"

    import numpy as np
    from varden_amd import advance as adv
    from varden_amd import boxlib as bl
    from varden_amd import driver
    from varden_amd.capi import default_params

    n = args.n
    walls = [[bl.NO_SLIP_WALL] * 2] * 3
    prm = default_params(cflfac=0.9, hg_fmg=args.hg_fmg, mac_fmg=args.mac_fmg)
    if not args.hg_pre_pair:
        prm.hg_omega_pre1 = prm.hg_omega_pre2 = 0.0
        prm.hg_omega_fac1 = prm.hg_omega_fac2 = prm.hg_omega_fac3 = 0.0
    comm_id = None
    if world > 1:                                          # RCCL unique id: rank 0 creates it, everybody receives it
        bl.initialize(prm, rank, world, local_rank)
        idt = torch.zeros(128, dtype=torch.uint8, device="cpu" if one_dev else "cuda")
        if rank == 0:
            idt.copy_(torch.tensor(list(bl.comm_get_unique_id()), dtype=torch.uint8))
        dist.broadcast(idt, 0)
        comm_id = bytes(idt.cpu().tolist())

    if world == 1 and os.environ.get("VDN_FORCE_PACKED") == "2":
        # one-GPU rehearsal of the N > 1 transport: a 1-rank RCCL communicator, every box-to-box copy packed and sent to the rank itself
        bl.initialize(prm, 0, 1, local_rank)
        bl.comm_init(bl.comm_get_unique_id())

    def build_workload(config, n):
        """the driver object of one BASELINE.json config: (G, cells, workload, parallelism, is_amr)"""
        amr = config in ("amr2", "amr3")
        if amr:
            max_levs = 2 if config == "amr2" else 3
            base_boxes = None
            if world > 1:                                      # cut the base level so that it can be dealt to the ranks
                hb = n // 2
                base_boxes = [((i * hb, j * hb, k * hb), ((i + 1) * hb - 1, (j + 1) * hb - 1, (k + 1) * hb - 1))
                              for k in range(2) for j in range(2) for i in range(2)]
            mgs = min(256, n)
            levels = driver.VardenAMR.tagged_grids(n, walls, prm, max_levs=max_levs, max_grid_size=mgs, device=local_rank, rank=rank, nranks=world,
                                                   comm_id=comm_id, base_boxes=base_boxes)
            assert len(levels) == max_levs - 1, "tagging produced %d refined levels, %d wanted" % (len(levels), max_levs - 1)
            G = driver.VardenAMR(n, levels[0], walls, params=prm, finer_levels=levels[1:], init_shrink=0.1, init_iter=1, do_initial_projection=1,
                                 device=local_rank, rank=rank, nranks=world, comm_id=comm_id, base_boxes=base_boxes, max_grid_size=mgs, swap_state=True)
            lev_cells = [n ** 3] + [sum(int(np.prod([b[1][d] - b[0][d] + 1 for d in range(3)])) for b in lb) for lb in levels]
            cells = sum(lev_cells)
            workload = ("3D %d-level AMR, base %d^3, refined levels tagged rho > 1.01%s (tag_boxes.f90:65-84), fixed grids: %s boxes, %s cells per level; "
                        "composite MAC + HG solves each step (BASELINE.json configs[%d])"
                        % (max_levs, n, " / rho > 1.1" if max_levs == 3 else "", [1 if base_boxes is None else 8] + [len(lb) for lb in levels], lev_cells,
                           3 if max_levs == 2 else 4))
            par = "single GPU" if world == 1 else "boxes of every level dealt to %d ranks by cell count (knapsack), RCCL p2p ghost / coarse-fine exchange + allreduce" % world
        else:
            if config == "512":                                # fixed global problem: 2x2x2 boxes of n^3, dealt round-robin
                decomp = (2, 2, 2)
                assert 8 % world == 0, "the 8 boxes of the 512 config need 1, 2, 4 or 8 ranks"
            else:
                decomp = {1: (1, 1, 1), 2: (2, 1, 1), 4: (2, 2, 1), 8: (2, 2, 2)}.get(world)
                assert decomp is not None, "bench.py supports 1, 2, 4 or 8 GPUs"
            nglob = tuple(n * decomp[d] for d in range(3))
            h = 1.0 / (n * max(decomp))                        # dx = dy = dz; 2x2x2 gives the unit cube
            prob_hi = tuple(nglob[d] * h for d in range(3))
            G = driver.Varden(nglob, walls, prm, prob_type=1, grav=-9.8, prob_hi=prob_hi, init_shrink=0.1, init_iter=1,
                              device=local_rank, decomp=decomp, rank=rank, nranks=world, comm_id=comm_id,
                              swap_state=True)     # uold <- unew as a handle exchange (tests/test_advance_gpu.py::test_handle_swap_equals_copy)
            cells = nglob[0] * nglob[1] * nglob[2]
            nb = decomp[0] * decomp[1] * decomp[2]
            workload = ("3D %dx%dx%d single-level variable-density bubble, %d box(es) of %d^3, MAC+HG projection each step (BASELINE.json configs[%d]%s)"
                        % (nglob + (nb, n, 1 if nb == 1 else 2, "" if (nb > 1 or n == 256) else " at north_star's single-GPU box size" if n == 512 else " at another box size")))
            par = "single GPU" if world == 1 else ("domain decomposition %dx%dx%d, %d box(es) of %d^3 per GPU, RCCL p2p ghost exchange + allreduce"
                                                   % (decomp + (nb // world, n)))
        return G, cells, workload, par, amr

    G, cells, workload, par, amr = build_workload(args.config, n)
    rccl_nranks = bl.comm_nranks()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    import ctypes as C
    from varden_amd import capi
    for _ in range(args.warmup):
        G.step()
    barrier()
    cst = (C.c_long * 24)()
    capi.load().vdn_comm_stats(cst, 1)                     # traffic counters of the timed steps only
    t0 = time.perf_counter()
    phases = dict(scalar=0.0, velocity=0.0, mac=0.0, hg=0.0, total=0.0)
    cyc = dict(mac=0, hg=0)
    for _ in range(args.steps):
        G.step()
        for k, v in adv.last_step_timing().items():
            phases[k] += v
        cyc["mac"] += adv.last_solver_stats("mac")[0]
        cyc["hg"] += adv.last_solver_stats("hg")[0]
    barrier()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], device="cpu" if one_dev else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())

    value = cells * args.steps / el
    capi.load().vdn_comm_stats(cst, 0)
    transport = capi.load().vdn_comm_transport().decode()
    comm = None
    if cst[0] or cst[3] or cst[4] or cst[6]:               # what this rank asked of the transport per step (include/varden_amd.h: vdn_comm_stats)
        k = float(args.steps)
        comm = {"ghost_exchanges": cst[0] / k, "view_refreshes": cst[6] / k, "sends": cst[1] / k, "MB_sent": (cst[2] + cst[7]) * 8e-6 / k,
                "allreduces": cst[3] / k, "allgathers": cst[4] / k,
                "exchanges_by_log2_bytes": {str(10 + b): cst[8 + b] / k for b in range(16) if cst[8 + b]}}
    dumped = None
    if args.dump_dir:                                      # (after the clock stopped: the copies to the host are not timed)
        dumped = dump_outputs(G, args.dump_dir, amr, rank)
    rho = None
    if args.full and rank == 0 and not amr:
        rho = G.sold[0].to_numpy()[..., 0]                  # rank 0's first box, for the smoother probe's coefficients
    G.close()                                              # also tears the RCCL communicator down

    # ---- strong scaling's N = 1 point is the eight-box run; the same 512^3 domain as ONE box on this GPU beside it (the best one-GPU time: speed-ups read against
    #      the eight-box point are flattered by what the decomposition itself costs) ----------
    one_box_512 = None
    if args.full and world == 1 and args.config == "512" and n == 256 and not args.no_extra:
        G1, cells1, wl1, _, _ = build_workload("256", 512)
        G1.step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            G1.step()
        torch.cuda.synchronize()
        el1 = time.perf_counter() - t1
        G1.close()
        one_box_512 = {"workload": wl1, "ms_per_step": round(1e3 * el1 / args.steps, 3), "value": round(cells1 * args.steps / el1, 1), "unit": "cells*steps/s",
                       "eight_boxes_over_one_box": round((el / args.steps) / (el1 / args.steps), 3),
                       "note": "strong-scaling speed-ups should be read against THIS time: the N = 1 point of the curve (eight boxes on one GPU) carries the cost of the decomposition"}

    # ---- the other single-GPU workloads of BASELINE.json, a few timed steps each (the headline stays configs[1]) ----------
    extra = []
    if args.full and world == 1 and args.config == "256" and n == 256 and not args.no_extra:
        XS = 10                                            # timed steps of every extra workload (one warm-up step before)
        # 512^3 as eight boxes (configs[2] on one GPU), 512^3 as ONE box (north_star's single-GPU size), the tagged hierarchies of configs[3] and configs[4]
        for cfg, n2 in (("512", 256), ("256", 512), ("amr2", 256), ("amr3", 256)):
            tb = time.perf_counter()
            G2, cells2, wl2, _, _ = build_workload(cfg, n2)
            G2.step()                                       # warm-up
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            cyc2 = dict(mac=0, hg=0)
            for _ in range(XS):
                G2.step()
                cyc2["mac"] += adv.last_solver_stats("mac")[0]
                cyc2["hg"] += adv.last_solver_stats("hg")[0]
            torch.cuda.synchronize()
            el2 = time.perf_counter() - t1
            G2.close()
            extra.append({"workload": wl2, "cells": cells2, "steps": XS, "warmup": 1, "ms_per_step": round(1e3 * el2 / XS, 3),
                          "value": round(cells2 * XS / el2, 1), "unit": "cells*steps/s",
                          "solver_iterations_per_step": {k: round(v / float(XS), 2) for k, v in cyc2.items()}, "wall_s_incl_setup": round(time.perf_counter() - tb, 1)})
        # the shape of the reference's own 3-D inputs, which the inviscid headline leaves out: visc_coef = 0.001 (exec/test/inputs_bubble_3d: three Crank-Nicolson
        # velocity solves per step) on one 256^3 box, and on the three-level hierarchy with the grids rebuilt every second step (exec/test/inputs_3d-regt: regrid_int = 2)
        vprm = default_params(cflfac=0.9, hg_fmg=args.hg_fmg, mac_fmg=args.mac_fmg, visc_coef=0.001)
        tb = time.perf_counter()
        Gv = driver.Varden((256,) * 3, walls, vprm, prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1, device=local_rank, swap_state=True)
        Gv.step(); torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(XS):
            Gv.step()
        torch.cuda.synchronize()
        elv = time.perf_counter() - t1
        Gv.close()
        extra.append({"workload": "3D 256x256x256 single-level bubble with visc_coef = 0.001 (exec/test/inputs_bubble_3d's value; the headline is the same run with visc_coef = 0)", "cells": 256 ** 3,
                      "steps": XS, "warmup": 1, "ms_per_step": round(1e3 * elv / XS, 3), "value": round(256 ** 3 * XS / elv, 1), "unit": "cells*steps/s", "wall_s_incl_setup": round(time.perf_counter() - tb, 1)})
        tb = time.perf_counter()
        lv = driver.VardenAMR.tagged_grids(256, walls, vprm, max_levs=3, max_grid_size=256, device=local_rank)
        Gr = driver.VardenAMR(256, lv[0], walls, params=vprm, finer_levels=lv[1:], init_shrink=0.1, init_iter=1, do_initial_projection=1, device=local_rank, max_grid_size=256, swap_state=True,
                              regrid_int=2, max_levs=3)
        Gr.step(); torch.cuda.synchronize()
        tsr, cells_r = [], 0
        for _ in range(XS):
            t1 = time.perf_counter(); nreg = Gr.nregrids
            Gr.step(); torch.cuda.synchronize()
            tsr.append((time.perf_counter() - t1, Gr.nregrids > nreg))
            cells_r += sum(int(np.prod([b[1][d] - b[0][d] + 1 for d in range(3)])) for lb in Gr.boxes for b in lb)
        boxes_r = [len(lb) for lb in Gr.boxes]
        Gr.close()
        elr = sum(t for t, _ in tsr)
        t_reg, t_plain = [t for t, r in tsr if r], [t for t, r in tsr if not r]
        extra.append({"workload": "3D 3-level AMR, base 256^3, visc_coef = 0.001, the grids rebuilt every second step (regrid_int = 2 as exec/test/inputs_3d-regt: tag_boxes + make_new_grids + "
                                  "fillpatch of the new levels inside the timed steps); %s boxes per level at the end" % boxes_r,
                      "cells": int(cells_r / XS), "steps": XS, "warmup": 1, "ms_per_step": round(1e3 * elr / XS, 3), "value": round(cells_r / elr, 1), "unit": "cells*steps/s",
                      "ms_per_step_with_a_regrid": round(1e3 * sum(t_reg) / max(1, len(t_reg)), 1), "ms_per_step_without": round(1e3 * sum(t_plain) / max(1, len(t_plain)), 1),
                      "regrids": len(t_reg), "wall_s_incl_setup": round(time.perf_counter() - tb, 1)})

    # ---- roofline of the dominant kernel: one colour pass of the MAC-MG smoother at 256^3 ----------
    roof = None
    if args.full and rank == 0:
        bl.initialize(prm, 0, 1, local_rank)               # the probe is a single-rank, single-box measurement
        pn = n if not amr else 256
        if rho is None:                                     # amr: the same bubble density on one 256^3 box
            rho = driver.initdata_numpy((pn,) * 3, [1.0 / pn] * 3, 1, 3, 2)[1][..., 0]
        lo0, hi0 = (0, 0, 0), (pn - 1,) * 3
        mla = bl.MLLayout([(lo0, hi0)], [[(lo0, hi0)]])
        rh, phi = bl.MultiFab(mla, 0, 1, 0), bl.MultiFab(mla, 0, 1, 1)
        beta = [bl.MultiFab(mla, 0, 1, 0, tuple(1 if t == d else 0 for t in range(3))) for d in range(3)]
        for d in range(3):      # beta = 2/(rho_i + rho_{i-1})  (macproject.f90:376-394), built on the host for the probe
            sl_hi = [slice(3, -3)] * 3
            sl_lo = [slice(3, -3)] * 3
            sl_hi[d] = slice(3, rho.shape[d] - 2)
            sl_lo[d] = slice(2, rho.shape[d] - 3)
            beta[d].from_numpy((2.0 / (rho[tuple(sl_hi)] + rho[tuple(sl_lo)]))[..., None])
        rng = np.random.default_rng(0)
        r = rng.standard_normal((pn, pn, pn, 1))
        rh.from_numpy(r - r.mean())
        bc = [[bl.BC_NEU] * 2] * 3
        rho_mf = bl.MultiFab(mla, 0, 1, 3)
        rho_mf.from_numpy(rho[..., None])
        # the pass macproject runs on its finest level (face coefficients recomputed from rho), and the stored-coefficient pass next to it
        ms, ncell = adv.bench_cc_smoother(rh, phi, beta, [1.0 / pn] * 3, bc, 200, rho=rho_mf)
        level_form = capi.load().vdn_last_mac_level_form()      # which kernel the probe timed: 1 the level by colour (kk_cc_gsrb_rho_split), 0 interleaved (kk_cc_gsrb_rho_pair)
        ms_stored, _ = adv.bench_cc_smoother(rh, phi, beta, [1.0 / pn] * 3, bc, 200)
        # the same passes launched as a solve launches them: sweeps of nu1 + nu2 = 4 sweeps time-skewed over plane slabs, a slab served from the Infinity Cache
        ms_in_solve, nc_in = adv.bench_cc_smoother_in_solve(rh, phi, beta, [1.0 / pn] * 3, bc, 4, 200, rho_mf)
        rho_mf.destroy()
        alg_bytes = 48.0 * ncell
        model_rate = alg_bytes / (ms * 1e-3) / 1e9
        # HBM bytes per launch: PMC passes (FETCH_SIZE x2 + WRITE_SIZE, MI355X_MICROARCH.md) collected with `rocprofv3 --pmc` on
        # tools/smoother_probe.py in a separate run and committed; not measured in THIS run, and said so in traffic_source
        traffic, traffic_source = None, None
        # which form ran: the level by colour (kk_cc_gsrb_rho_split, from 2^23 cells on one box; the default) or interleaved (kk_cc_gsrb_rho_pair)
        split = level_form == 1
        names = (["r06_smoother_split_pmc.json", "r05_smoother_split_pmc.json"] if split else
                 ["r05_smoother_rho_pmc.json", "r04_smoother_rho_pmc.json", "r03_smoother_rho_pmc.json", "r02_smoother_rho_pmc.json", "r01_smoother_rho_pmc.json"])
        if pn == 256 and world == 1 and not args.no_pmc:
            got = measure_pass_traffic("kk_cc_gsrb_rho_split<0, false>" if split else "kk_cc_gsrb_rho_pair(")
            if got:
                traffic = got[0]
                traffic_source = ("measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE, one child run of tools/smoother_probe.py 256 20 each (the timed probe's "
                                  "kernel and data), per-launch means %.1f / %.1f KB, bytes = 2 x FETCH_SIZE + WRITE_SIZE (MI355X_MICROARCH.md)" % (got[1]["FETCH_SIZE"], got[1]["WRITE_SIZE"]))
        for name in ([] if traffic else names):
            pmc = os.path.join(ROOT, "profiles", name)
            if pn == 256 and os.path.exists(pmc):
                traffic = json.load(open(pmc))["hbm_bytes_per_launch"]
                traffic_source = "profiles/%s (committed rocprofv3 --pmc passes of the same kernel; not measured in this run)" % name
                break
        # the bytes of the entries a pass touches in this layout: phi own r + w, rhs own, rho both colours, phi other colour = 48 B per UPDATED cell
        # = 24 B per cell of the level (split); the interleaved pass cannot avoid whole lines of phi and rhs: 34 B per cell of the level
        touched = (24.0 if split else 34.0) * ncell
        kname = ("kk_cc_gsrb_rho_split<0, false> (MAC-MG red-black GS colour pass, %d^3, the level stored BY COLOUR; beta recomputed from rho, two cells per thread. "
                 "`achieved` / `frac` are BANDWIDTH: the HBM bytes the counters saw per launch / launch time (/ peak); without counters the bytes of the entries the pass "
                 "touches, 24 B per cell of the level.  SURVEY section 8(d)'s 48 B per cell of the level (stored face coefficients, whole lines of phi and rhs) is what "
                 "an interleaved stored-coefficient pass would move for the same work: `model_48B_rate` / `frac_model` price the pass that way -- a work rate, NOT bandwidth, "
                 "it may exceed the peak.  Interleaved stored-beta pass kk_cc_gsrb_pair: %.5f ms)" % (pn, ms_stored)) if split else \
                ("kk_cc_gsrb_rho_pair (MAC-MG red-black GS colour pass, %d^3, the level interleaved; beta recomputed from rho, 2x2 cells per thread: ~34 B per cell of the level "
                 "touched; `achieved` / `frac`: counter bytes (else the touched bytes) / time; `model_48B_rate`: SURVEY 8(d)'s 48 B/cell model, a work rate.  Stored-beta pass kk_cc_gsrb_pair: %.5f ms)" % (pn, ms_stored))
        phys_bytes = float(traffic) if traffic else touched
        achieved = phys_bytes / (ms * 1e-3) / 1e9
        assert achieved <= HBM_PEAK_GBS, "roofline.achieved %.1f GB/s above the HBM peak: the byte count is wrong" % achieved
        roof = {"bound": "hbm", "kernel": kname,
                "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                "bytes_priced": ("counters (2 x FETCH_SIZE + WRITE_SIZE)" if traffic else "touched entries (no counters in this run)"),
                "touched_bytes_per_launch": touched, "frac_touched": round(touched / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "avg_launch_ms": round(ms, 5),
                # inside a solve the passes of a cycle run time-skewed over plane slabs (cc_split_run): per pass over the whole level, mostly cache-served
                "in_solve_ms_per_level_pass": (round(ms_in_solve, 5) if nc_in else None),
                "in_solve_note": ("sweeps of 4 time-skewed over plane slabs as cc_solve launches them; a slab's second to eighth pass is served from the 256 MB Infinity Cache, "
                                  "so bytes / this time is not an HBM rate" if nc_in else None),
                # the survey's model of the pass (48 B per cell of the level): a work rate for continuity with rounds 1-4, not bandwidth
                "alg_bytes_per_launch": alg_bytes, "model_48B_rate": round(model_rate, 1), "frac_model": round(model_rate / HBM_PEAK_GBS, 4),
                "model_note": "48 B/cell is what SURVEY 8(d) prices a pass at (stored coefficients, whole lines); the kernel moves fewer bytes for the same pass, so this rate is not bandwidth"}
        for m in [rh, phi] + beta:
            m.destroy()

    # ---- CPU baseline: the oracle (a port of the same algorithm, OpenMP) on a bounded sample ------
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu:      # reported at N = 1 only
        nthreads = min(16, os.cpu_count() or 1)
        os.environ["OMP_NUM_THREADS"] = str(nthreads)
        from oracle import voracle as vo
        vo.lib(); vo.set_threads(nthreads)          # (torch's libgomp is in the process already and has read its environment: set the count directly)

        def single_level_sample(cn, ncpu, gpu_timed=True):
            """the oracle on one cn^3 box of the same bubble, `ncpu` timed steps after the start-up sequence; the GPU on the SAME sample, from the same initial data
            through the same start-up sequence, stepped next to it: the new state, dt and both solvers' cycle counts are compared after EVERY timed CPU step"""
            O = vo.Sim(cn, walls, default_params(cflfac=0.9), prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1)
            bl.initialize(prm, 0, 1, local_rank)
            Gs = driver.Varden((cn,) * 3, walls, default_params(cflfac=0.9), prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1, device=local_rank, swap_state=True)
            tsteps, phase_runs = [], []
            par_u = par_s = par_p = par_dt = 0.0
            cyc_o, cyc_g = [], []
            for _ in range(ncpu):
                tc = time.perf_counter()
                O.step()
                tsteps.append(time.perf_counter() - tc)
                phase_runs.append([float(O.phase[i]) for i in range(4)])
                Gs.step()
                gsz = 3
                ug = Gs.uold[0].to_numpy()[gsz:-gsz, gsz:-gsz, gsz:-gsz]     # after the step uold / sold hold the new state on both sides
                sg = Gs.sold[0].to_numpy()[gsz:-gsz, gsz:-gsz, gsz:-gsz]
                pg = Gs.p[0].to_numpy()[1:-1, 1:-1, 1:-1]
                uo, so, po = O.uold.valid(), O.sold.valid(), O.p.valid()
                par_u = max(par_u, float(np.abs(ug - uo).max() / max(np.abs(uo).max(), 1e-300)))
                par_s = max(par_s, float(np.abs(sg - so).max() / max(np.abs(so).max(), 1e-300)))
                pg, po = pg - pg.mean(), po - po.mean()                        # the pressure is fixed up to a constant
                par_p = max(par_p, float(np.abs(pg - po).max() / max(np.abs(po).max(), 1e-300)))
                par_dt = max(par_dt, abs(Gs.dt - O.dt) / O.dt)
                cyc_o.append([int(O.mgstat[0].cycles), int(O.mgstat[1].cycles)])
                cyc_g.append([int(adv.last_solver_stats("mac")[0]), int(adv.last_solver_stats("hg")[0])])
            tmed = sorted(tsteps)[len(tsteps) // 2]                # median
            parity = {"steps_compared": ncpu, "max_rel_u": par_u, "max_rel_s": par_s, "max_rel_p": par_p, "max_rel_dt": par_dt,
                      "cycles_equal": cyc_o == cyc_g, "cycles_mac_hg_oracle": cyc_o, "cycles_mac_hg_gpu": cyc_g,
                      "tolerance": {"u": 1e-9, "s": 1e-9, "p": 1e-6}}
            pr = phase_runs[tsteps.index(tmed)]                    # the oracle's own split of the median step (advance_timestep.f90:159-166)
            phase_s = {k: round(pr[i], 3) for i, k in enumerate(("scalar_advance", "velocity_advance", "mac_project", "hg_project"))}
            phase_s["other (forces, velpred, ghost fills, estdt)"] = round(tmed - sum(phase_s.values()), 3)
            gpu_ms = None
            if gpu_timed:                                          # the GPU's time on the SAME sample (like for like with `value` of this object)
                for _ in range(5):                                 # the card idled through the CPU legs: untimed steps first
                    Gs.step()
                torch.cuda.synchronize()
                tg = time.perf_counter()
                for _ in range(5):
                    Gs.step()
                torch.cuda.synchronize()
                gpu_ms = round(1e3 * (time.perf_counter() - tg) / 5, 3)
            Gs.close()
            del O
            return tmed, tsteps, parity, phase_s, gpu_ms

        parity = phase_s = gpu_same_ms = None
        if amr:
            cn = args.cpu_n or 64
            # the oracle's hierarchies hold one box per level: the sample refines the bounding box of the tagged region
            flo, fhi = [cn], [0]
            for b in driver.VardenAMR.tagged_grids(cn, walls, default_params(cflfac=0.9), max_levs=2, max_grid_size=256, device=local_rank)[0]:
                flo.append(min(b[0])); fhi.append(max(b[1]))
            flo, fhi = (min(flo) // 2 * 2,) * 3, ((max(fhi) + 1) // 2 * 2 - 1,) * 3
            O = vo.Sim2L(cn, flo, fhi, walls, prm=default_params(cflfac=0.9), init_shrink=0.1, init_iter=1, do_initial_projection=1)
            ccells = cn ** 3 + (fhi[0] - flo[0] + 1) ** 3
            sample = "%d^3 base + one refined box %s..%s (bounding box of the rho > 1.01 tags), composite solves" % (cn, flo, fhi)
            ncpu = 1
            tc = time.perf_counter()
            O.step()
            tsteps = [time.perf_counter() - tc]
            tcpu = tsteps[0]
        else:
            cn = args.cpu_n or 128
            ccells = cn ** 3
            sample = "%d^3 bubble (same problem, smaller box)" % cn
            ncpu = max(1, args.cpu_steps)
            tcpu, tsteps, parity, phase_s, gpu_same_ms = single_level_sample(cn, ncpu)
        # calibration against the reference's own kernels: the four Godunov calls of a step on one thread, beside the
        # 2.91 s the survey measured for the reference's Fortran on one core (that was the survey container's CPU, this is
        # the bench host's: a cross-machine ratio -- DESIGN.md quotes the same-machine one)
        cal = godunov_calibration(vo, 128) if not args.no_calib else None
        vo.set_threads(nthreads)                              # (the calibration ran on one thread)
        # ONE oracle step at the headline size itself (256^3, configs[1]) with the GPU stepped beside it: the GPU / CPU ratio at the size `value` is quoted on,
        # timed by this run (about 7 s for the step + the start-up sequence before it)
        sample_256 = None
        if not amr and args.config == "256" and n == 256 and cn != 256 and not args.no_cpu256:
            t256, ts256, par256, ph256, _ = single_level_sample(256, 1, gpu_timed=False)
            sample_256 = {"value": round(256 ** 3 / t256, 1), "unit": "cells*steps/s", "cores": nthreads, "cpu_s_per_step": round(t256, 2),
                          "gpu_ms_per_step": round(1e3 * el / args.steps, 3), "gpu_over_cpu": round(t256 / (el / args.steps), 1),
                          "sample": "the headline workload itself: one timed oracle step at 256^3 after the start-up sequence, the GPU stepped beside it and compared",
                          "parity": par256, "phase_s": ph256}
        cpu = {"value": round(ccells / tcpu, 1), "unit": "cells*steps/s", "cores": nthreads, "kind": "port",
               "sample": "%s, median of %d timed step(s) (%s s) after the start-up sequence; gcc -O2 -fopenmp, OMP_NUM_THREADS=%d"
                         % (sample, ncpu, "/".join("%.1f" % t for t in tsteps), nthreads),
               "parity": parity, "phase_s": phase_s,
               "gpu_same_sample_ms": gpu_same_ms,
               "gpu_over_cpu_same_sample": (round(1e3 * tcpu / gpu_same_ms, 1) if gpu_same_ms else None),
               "sample_256": sample_256,
               "godunov_1thread_128_s": cal,
               "calibration_vs_reference_godunov": (round(sum(cal.values()) / 2.91, 2) if cal else None),
               "reference_godunov_mcells_per_s_per_core": REF_GODUNOV_MCELLS_PER_CORE,
               "reference_note": "BASELINE.md 1b: the reference's own velpred+mkflux+update (flang -O2, 1 core, 128^3) = 0.72 Mcells/s/core for advection "
                                 "alone (no multigrid): x%d cores = %.2e cells*steps/s is an upper bound on the reference's advance_timestep on this host"
                                 % (nthreads, REF_GODUNOV_MCELLS_PER_CORE * 1e6 * nthreads)}

    if rank == 0:
        out = {
            "metric": "cells*steps/sec on advance_timestep",
            "value": round(value, 1), "unit": "cells*steps/s",
            "n_gpus": world, "rccl_nranks": rccl_nranks, "transport": transport, "library": capi.load().vdn_build_flavour().decode(), "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * el / args.steps, 3),
            "higher_is_better": True, "scaling": args.scaling if not amr else "strong", "vs_baseline": None, "full": args.full,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": workload, "parallelism": par, "cells": cells,
                       "phase_ms_per_step": {k: round(1e3 * v / args.steps, 3) for k, v in phases.items()},
                       "vcycles_per_step": {k: round(v / args.steps, 2) for k, v in cyc.items()},
                       "comm_per_step_rank0": comm, "one_box_512": one_box_512,
                       "note": ("the timed steps are steps %d-%d of the inviscid run (exec/test/inputs_bubble_3d with visc_coef = 0).  Run to the end, this configuration does NOT "
                                "complete at 256^3: the blob reaches the floor near t = 0.34, rho undershoots to 0.06 and the nodal solve diverges at step 275 "
                                "(profiles/r05_long_inviscid_256.txt; the scheme without viscosity at this resolution -- GPU and oracle agree through the same impact at 128^3)"
                                % (args.warmup + 1, args.warmup + args.steps)) if (not amr and args.config == "256") else None},
            "roofline": roof, "cpu_baseline": cpu, "extra_workloads": extra,
        }
        if dumped:                                         # (rank 0's files; the other ranks wrote their own boxes next to them)
            out["outputs_dumped"] = {"dir": os.path.abspath(args.dump_dir), "files": dumped[0], "bytes": dumped[1], "sampled": dumped[2]}
        print(json.dumps(out), flush=True)
        for prt in ((cpu or {}).get("parity"), ((cpu or {}).get("sample_256") or {}).get("parity")):
            if prt:                                        # the bench FAILS when the GPU and the oracle disagree on a sample they both stepped
                assert prt["max_rel_u"] <= 1e-9 and prt["max_rel_s"] <= 1e-9 and prt["max_rel_p"] <= 1e-6 and prt["cycles_equal"], \
                    "cpu_baseline.parity out of tolerance: %r" % (prt,)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
