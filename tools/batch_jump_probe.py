"""Batched trajectories with one-site jump channels: aggregate time steps per second of a batch (a) with no channel,
(b) with a jump channel on site 5 and (c) with jump channels on every site, at the shapes of profiles/batch_probe.txt:
L = 10, d = 4, M = 6, D = 16 and D = 32, B = 128.   python tools/batch_jump_probe.py [--only none|one|all] [--D 16]

One JSON line per measurement.  Every measurement runs in a child process of its own under a time limit (a run that sits
is ended and reported, nothing more is started then); a warm-up, then three timed repeats with a device synchronisation on
both sides, minimum reported.  The condition on the kernel (k_batch_channel's mean duration at most k_batch_sweep's at the
same shape and B) is read from a `rocprofv3 --kernel-trace --stats -- python tools/batch_jump_probe.py --child all D` run
of its own, without counter collection."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, DT, B, SITE, K = 10, 4, 6, 0.5, 128, 5, 4
NSTEP, REPEATS, LIMIT_S = 5, 3, 240
KINDS = ("none", "one", "all")


def kraus_set(rng):
    """K random d x d matrices rescaled to sum B^+ B = 1"""
    import numpy as np

    G = rng.standard_normal((K, d, d)) + 1j * rng.standard_normal((K, d, d))
    w, V = np.linalg.eigh(sum(g.conj().T @ g for g in G))
    return G @ ((V / np.sqrt(w)) @ V.conj().T)


def measure(kind, D):
    import numpy as np

    import pytdscf_amd as P
    from pytdscf_amd import synthetic as syn
    from pytdscf_amd.engine import device_sync

    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    bt = P.TDVPBatch(B, L)
    for r, e in enumerate(bt.engines):
        e.set_mpo(mpo)
        e.init_random([d] * L, D, seed=1 + r)
    rng = np.random.default_rng(0)
    sites = {"none": [], "one": [SITE], "all": list(range(L))}[kind]
    if sites:
        bt.set_jumps({p: kraus_set(rng) for p in sites}, seed=1)
    bt.propagate(DT, 2)  # warm-up: Krylov memories, workspaces, clocks
    for e in bt.engines:
        e.counters_reset()
    best = None
    for _ in range(REPEATS):
        device_sync(0)
        t0 = time.perf_counter()
        bt.propagate(DT, NSTEP)
        device_sync(0)
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    launches = bt.launches() / (REPEATS * NSTEP)
    jumps = int(bt.jump_counts().sum()) if sites else 0
    rec = dict(probe="batch_jump_probe", kind=kind, B=B, L=L, d=d, D=D, M=M, K=K, dt=DT, jump_sites=len(sites), steps=NSTEP,
               repeats=REPEATS, seconds_min=round(best, 6), ms_per_step=round(1e3 * best / NSTEP, 3),
               aggregate_steps_per_s=round(B * NSTEP / best, 1), launches_per_step=round(launches, 2), jumps_counted=jumps,
               norm0=round(float(bt[0].norm()), 12))
    bt.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=KINDS)
    ap.add_argument("--D", type=int, choices=(16, 32))
    ap.add_argument("--child", nargs=2, metavar=("KIND", "D"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child[0], int(a.child[1]))), flush=True)
        return 0
    rc = 0
    for D in (16, 32):
        if a.D and D != a.D:
            continue
        for kind in KINDS:
            if a.only and kind != a.only:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, str(D)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(probe="batch_jump_probe", kind=kind, D=D, error=f"no result within {LIMIT_S} s")), flush=True)
                return 1  # nothing more is started on a device that may be in trouble
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(json.dumps(dict(probe="batch_jump_probe", kind=kind, D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
                if p.returncode < 0 or p.returncode in (134, 139):
                    return 1
                rc = 1
                continue
            print(line, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
