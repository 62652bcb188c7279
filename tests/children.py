"""Every child process the suite starts on the GPU, in one place.

The library reads its launch-form switches once per process (varden_amd/csrc/vdn_switches.h), so a test that compares launch forms runs each form in a child:
run_variant / run_variants.  Several ranks on one GPU are processes too (or threads of a process, tests/_rank_threads.py), with the RCCL test double
tests/fake_rccl as their transport and a file as their rendezvous: launch_ranks on the test's side, rendezvous / save_rank on the worker's.

A child sees NO VDN_* variable of the outer environment except the ones that choose the library and steer bench.py and the workers themselves
(variant_env): what a variant runs is what its dictionary says, whatever the shell that started pytest had set."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
TAGS = ("HASH", "FORM", "CASE", "RESULT")
MAX_CHILDREN = 4          # the most processes one call starts next to each other (eight ranks run as 4 x 2 threads)


def variant_env(switches, keep=()):
    """os.environ without any VDN_* variable -- but VDN_LIB_FLAVOUR, VDN_BENCH_*, VDN_WORKER_* and the names in `keep` --, then `switches` on top"""
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("VDN_") or k == "VDN_LIB_FLAVOUR" or k.startswith(("VDN_BENCH_", "VDN_WORKER_")) or k in keep}
    env.update(switches)
    return env


def run_variant(cmd, switches, timeout, cwd=ROOT):
    """one child `python cmd...` (a worker's path with its arguments, or "-c", code, arguments) under `switches`; fails with the end of its stderr on a
    non-zero status or the time limit; returns {tag: [tokens of every stdout line that starts with the tag, the tag first]} for HASH / FORM / CASE / RESULT"""
    try:
        r = subprocess.run([sys.executable] + [str(c) for c in cmd], env=variant_env(switches), capture_output=True, text=True, timeout=timeout, cwd=cwd)
    except subprocess.TimeoutExpired as e:          # (subprocess.run has killed the child)
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        raise AssertionError("%r: no end after %d s\n%s" % (switches, timeout, err[-2000:]))
    assert r.returncode == 0, "%r: status %d\n%s" % (switches, r.returncode, r.stderr[-2000:])
    out = {}
    for ln in r.stdout.splitlines():
        tok = ln.split()
        if tok and tok[0] in TAGS:
            out.setdefault(tok[0], []).append(tok)
    return out


def run_variants(cmd, variants, timeout):
    """run_variant for each of `variants` in turn, the results in their order; a child that fails, is killed by a signal or runs into the time limit
    raises there, so nothing is started after it"""
    return [run_variant(cmd, switches, timeout) for switches in variants]


def line(result, tag):
    """the first line of a run_variant result that carries `tag`, as the child printed it (single blanks)"""
    return " ".join(result[tag][0])


def fake_rccl():
    """the RCCL test double, built when it is not there yet"""
    if not os.path.exists(FAKE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(FAKE)])
    return FAKE


def rank_groups(nranks, per_proc):
    """the ranks each worker process hosts, as its first argument: "0,1", "2,3", ..."""
    return [",".join(str(r) for r in range(a, min(a + per_proc, nranks))) for a in range(0, nranks, per_proc)]


def launch_ranks(worker, nranks, tmp_path, tag, args, per_proc=1, real_rccl=False, agree=("dt",), switches=None, timeout=400, overlap="1"):
    """`nranks` ranks of tests/<worker> (argv: ranks nranks idfile outprefix args...), `per_proc` rank threads per process; waits for all of them, kills what
    is left of the processes it started, wants every status zero and merges the ranks' <prefix>.<rank>.npz files (the keys in `agree` equal on all ranks).
    overlap: VDN_OVERLAP of the ranks unless `switches` says otherwise ("1": halo exchange on the second stream + shell kernels on every level -- by default
    only boxes of >= 2^20 cells do; None: unset).  real_rccl: one GPU per rank, the RCCL torch ships (dlopen of librccl.so.1)"""
    groups = rank_groups(nranks, per_proc)
    assert len(groups) <= MAX_CHILDREN, "%d ranks as %d processes: at most %d next to each other on a shared card (raise per_proc)" % (nranks, len(groups), MAX_CHILDREN)
    idfile, prefix = str(tmp_path / (tag + ".id")), str(tmp_path / tag)
    if real_rccl:
        env = variant_env(dict(switches or {}, VDN_WORKER_DEVICE_PER_RANK="1", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    else:
        env = variant_env(dict({} if overlap is None else {"VDN_OVERLAP": overlap}, **(switches or {})))
        env.update(VDN_RCCL_LIB=fake_rccl() if nranks > 1 else FAKE, VDN_TESTING="1", FAKE_RCCL_DIR=str(tmp_path))
        if nranks >= 8:
            env["FAKE_RCCL_MAXMSG_MB"] = "8"     # 64 mailboxes: keep the memory-mapped file small (the messages of 32^3 boxes are a few hundred KB)
    procs = []
    try:
        for g in groups:
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", worker), g, str(nranks), idfile, prefix] + [str(a) for a in args], env=env, cwd=ROOT))
        end = time.time() + timeout
        rcs = [p.wait(timeout=max(0.0, end - time.time())) for p in procs]
    finally:
        for p in procs:                          # exactly the children started here
            if p.poll() is None:
                p.kill()
                p.wait()
    assert rcs == [0] * len(procs), rcs
    out = {}
    for r in range(nranks):
        with np.load(prefix + ".%d.npz" % r) as z:
            for k in z.files:
                if k in agree:
                    out.setdefault(k, z[k])
                    assert np.array_equal(out[k], z[k]), "ranks disagree on " + k
                else:
                    out[k] = z[k]
    return out


# ---- the worker's side -----------------------------------------------------------------------------------------------------------------------
def rendezvous(bl, prm, rank, nranks, idfile, dev=0):
    """the communicator id of a run of several ranks (None for one rank): rank 0 publishes it in `idfile` (written under another name, then renamed),
    the others wait for the file, two minutes at the most.  bl: the rank's boxlib module (its own copy of the package under rank threads)"""
    if nranks == 1:
        return None
    bl.initialize(prm, rank, nranks, dev)
    if rank == 0:
        with open(idfile + ".tmp", "wb") as f:
            f.write(bl.comm_get_unique_id())
        os.rename(idfile + ".tmp", idfile)
    t0 = time.time()
    while not os.path.exists(idfile):
        time.sleep(0.01)
        assert time.time() - t0 < 120, "rendezvous timed out"
    with open(idfile, "rb") as f:
        return f.read()


def save_rank(outprefix, rank, out):
    """one rank's results, where launch_ranks reads them"""
    np.savez(outprefix + ".%d.npz" % rank, **out)
