"""Batched trajectories against the ensemble mode and one full-device engine: aggregate half-sweeps per second at
L = 10, d = 4, M = 6, D = 16 and D = 32.   python tools/batch_probe.py [--only batch|ensemble|engine]

One JSON line per measurement.  TDVPBatch at B = 16, 64, 128, 256 (one launch per half-sweep for the whole batch),
TDVPEnsemble at B = 16 (an engine, a host thread and a compute-unit range per replica), one engine on the whole device.
Every measurement runs in a child process of its own under a time limit (a run that sits is ended and reported, the
others still run); a warm-up, then three timed repeats with a device synchronisation on both sides, minimum reported."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, DT = 10, 4, 6, 0.5
NSTEP, REPEATS, LIMIT_S = 5, 3, 240


def measure(kind, B, D):
    import pytdscf_amd as P
    from pytdscf_amd.engine import device_sync
    from pytdscf_amd import synthetic as syn

    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    if kind == "batch":
        obj = P.TDVPBatch(B, L)
        engines = obj.engines
    elif kind == "ensemble":
        obj = P.TDVPEnsemble(B, L)
        engines = obj.engines
    else:
        obj = None
        engines = [P.TDVPEngine(L)]
    for r, e in enumerate(engines):
        e.set_mpo(mpo)
        e.init_random([d] * L, D, seed=1 + r)

    def run(n):
        if kind == "engine":
            for _ in range(n):
                engines[0].propagate(DT)
        else:
            obj.propagate(DT, n)

    run(2)  # warm-up: Krylov memories, workspaces, clocks
    for e in engines:
        e.counters_reset()
    best = None
    for _ in range(REPEATS):
        device_sync(0)
        t0 = time.perf_counter()
        run(NSTEP)
        device_sync(0)
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    launches = sum(e.counters()["n_launch"] for e in engines) / (REPEATS * NSTEP)
    rec = dict(probe="batch_probe", kind=kind, B=B, L=L, d=d, D=D, M=M, dt=DT, steps=NSTEP, repeats=REPEATS,
               seconds_min=round(best, 6), sweeps_per_s=round(B * 2 * NSTEP / best, 1),
               launches_per_step=round(launches, 2), norm0=round(engines[0].norm(), 12))
    if obj is None:
        engines[0].close()
    else:
        obj.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["batch", "ensemble", "engine"])
    ap.add_argument("--child", nargs=3, metavar=("KIND", "B", "D"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child[0], int(a.child[1]), int(a.child[2]))), flush=True)
        return 0
    jobs = []
    for D in (16, 32):
        jobs += [("batch", B, D) for B in (16, 64, 128, 256)] + [("ensemble", 16, D), ("engine", 1, D)]
    rc = 0
    for kind, B, D in jobs:
        if a.only and kind != a.only:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, str(B), str(D)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(probe="batch_probe", kind=kind, B=B, D=D, error=f"no result within {LIMIT_S} s")), flush=True)
            return 1  # nothing more is started on a device that may be in trouble
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
        if p.returncode != 0 or line is None:
            print(json.dumps(dict(probe="batch_probe", kind=kind, B=B, D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
            if p.returncode < 0 or p.returncode in (134, 139):
                return 1
            rc = 1
            continue
        print(line, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
