"""Expectation values of MPO observables of batched trajectories: time per step of (a) the unobserved batch step ("step"),
(b) a recorded run with the expect request alone, three observables at every step, on the device (k_batch_expect:
"expect"), and (c) the host route the request replaces ("host"): TDVPBatch.propagate(dt) followed by
TDVPEngine.expectation(k) for the three observables on every engine -- a fresh right-environment walk per engine and
operator -- at L = 10, d = 4, M = 6, D = 16 and D = 32, B = 128.   python tools/batch_expect_probe.py [--only step|expect|host]

The condition is (b) <= (c) at both bond dimensions, on the same box.  One JSON line per measurement.  Every measurement
runs in a child process of its own under a time limit (a run that sits is ended and reported, nothing more is started
then); a warm-up, then three timed repeats with a device synchronisation on both sides, minimum reported.
`--child KIND D` is one measurement in this process: the form to put behind a profiler (kernel trace and statistics on
their own, no counter collection, the program behind `--`), to read the mean duration of k_batch_expect next to
k_batch_sweep's."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, DT, B = 10, 4, 6, 0.5, 128
NOBS = 3
NSTEP, REPEATS, LIMIT_S = 5, 3, 240
KINDS = ("step", "expect", "host")


def measure(kind, D):
    import numpy as np

    import pytdscf_amd as P
    from pytdscf_amd import synthetic as syn
    from pytdscf_amd.engine import device_sync

    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    obs = [syn.synthetic_mpo(L, d, M, seed=10 + k) for k in range(NOBS)]  # three observables with the Hamiltonian's MPO bonds
    ids = list(range(1, NOBS + 1))
    bt = P.TDVPBatch(B, L)
    for r, e in enumerate(bt.engines):
        e.set_mpo(mpo)
        for k, cores in zip(ids, obs):
            e.set_mpo(cores, k)
        e.init_random([d] * L, D, seed=1 + r)
    if kind == "expect":
        bt.set_expect(ids)
    last = {}

    def run(n):
        if kind == "step":
            bt.propagate(DT, n)
            last["value"] = 0.0
        elif kind == "expect":
            rec = bt.propagate(DT, n, observe=dict(norm=False, per_replica=False, expect=True), every=1)
            last["value"] = float(rec["mean_expect"][-1, 0].real)
        else:
            for _ in range(n):
                bt.propagate(DT)
                vals = np.mean([[e.expectation(k) for k in ids] for e in bt.engines], axis=0)
            last["value"] = float(vals[0].real)

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
    rec = dict(probe="batch_expect_probe", kind=kind, B=B, observables=NOBS, L=L, d=d, D=D, M=M, dt=DT, steps=NSTEP, repeats=REPEATS,
               seconds_min=round(best, 6), ms_per_step=round(1e3 * best / NSTEP, 3), launches_per_step=round(launches, 2),
               last_mean_first_observable=round(last["value"], 12))
    bt.close()
    return rec


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
                print(json.dumps(dict(probe="batch_expect_probe", kind=kind, D=D, error=f"no result within {LIMIT_S} s")), flush=True)
                return 1  # nothing more is started on a device that may be in trouble
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(json.dumps(dict(probe="batch_expect_probe", kind=kind, D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
                if p.returncode < 0 or p.returncode in (134, 139):
                    return 1
                rc = 1
                continue
            print(line, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
