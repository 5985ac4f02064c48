"""Observed batched trajectories: time per step of (a) the unobserved batch step, (b) the recorded run (one site reduced
density of every replica and its ensemble mean at every step, formed on the device: mitdvp_batch_run) and (c) the way
without it, TDVPBatch.propagate(dt) followed by reduced_density over all engines, at L = 10, d = 4, M = 6, D = 16 and
D = 32, B = 128, one interior site.   python tools/batch_observe_probe.py [--only step|run|run_all|loop]

One JSON line per measurement ("run": the means only, the cheap default; "run_all": every replica's density comes back as
well).  Every measurement runs in a child process of its own under a time limit (a run that sits is ended and reported,
nothing more is started then); a warm-up, then three timed repeats with a device synchronisation on both sides, minimum
reported."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, DT, B, SITE = 10, 4, 6, 0.5, 128, 5
NSTEP, REPEATS, LIMIT_S = 5, 3, 240
KINDS = ("step", "run", "run_all", "loop")


def measure(kind, D):
    import pytdscf_amd as P
    from pytdscf_amd import synthetic as syn
    from pytdscf_amd.engine import device_sync

    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    bt = P.TDVPBatch(B, L)
    for r, e in enumerate(bt.engines):
        e.set_mpo(mpo)
        e.init_random([d] * L, D, seed=1 + r)
    legs = [0] * SITE + [2]
    last = {}

    def run(n):
        if kind == "step":
            bt.propagate(DT, n)
        elif kind in ("run", "run_all"):
            rec = bt.propagate(DT, n, observe=dict(sites=[SITE], norm=False, per_replica=kind == "run_all"), every=1)
            last["trace"] = float(np_trace(rec["mean_rdm"][0][-1]))
        else:
            for _ in range(n):
                rho = sum(e.reduced_density(legs) for e in bt.engines) / B
                bt.propagate(DT)
            last["trace"] = float(np_trace(rho))

    run(2)  # warm-up: Krylov memories, workspaces, clocks
    for e in bt.engines:
        e.counters_reset()
    best = None
    for _ in range(REPEATS):
        device_sync(0)
        t0 = time.perf_counter()
        run(NSTEP)
        device_sync(0)
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    launches = sum(e.counters()["n_launch"] for e in bt.engines) / (REPEATS * NSTEP)
    rec = dict(probe="batch_observe_probe", kind=kind, B=B, L=L, d=d, D=D, M=M, dt=DT, site=SITE, steps=NSTEP, repeats=REPEATS,
               seconds_min=round(best, 6), ms_per_step=round(1e3 * best / NSTEP, 3), launches_per_step=round(launches, 2),
               mean_trace=round(last.get("trace", float("nan")), 12))
    bt.close()
    return rec


def np_trace(rho):
    import numpy as np

    return np.trace(rho).real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=KINDS)
    ap.add_argument("--child", nargs=2, metavar=("KIND", "D"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child[0], int(a.child[1]))), flush=True)
        return 0
    rc = 0
    for D in (16, 32):
        for kind in KINDS:
            if a.only and kind != a.only:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, str(D)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(probe="batch_observe_probe", kind=kind, D=D, error=f"no result within {LIMIT_S} s")), flush=True)
                return 1  # nothing more is started on a device that may be in trouble
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(json.dumps(dict(probe="batch_observe_probe", kind=kind, D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
                if p.returncode < 0 or p.returncode in (134, 139):
                    return 1
                rc = 1
                continue
            print(line, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
