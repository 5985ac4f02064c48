"""Cross overlaps of batched trajectories: time per step of a recorded run that evaluates P = 128 plain-overlap pairs
<psi_r(0)|psi_r(t)> (snapshot bra, replica ket) at every step on the device (k_batch_cross: "cross"), of the same run
recording the t/2-trick autocorrelation only (k_batch_observe: "autocorr"), and of the way without either,
TDVPBatch.propagate(dt) followed by overlap_reference over all engines ("walk"), at L = 10, d = 4, M = 6, D = 16 and
D = 32, B = 128.   python tools/batch_cross_probe.py [--only cross|autocorr|walk]

One JSON line per measurement.  Every measurement runs in a child process of its own under a time limit (a run that sits
is ended and reported, nothing more is started then); a warm-up, then three timed repeats with a device synchronisation
on both sides, minimum reported.  `--child KIND D` is one measurement in this process: the form to put behind a profiler."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, DT, B = 10, 4, 6, 0.5, 128
NSTEP, REPEATS, LIMIT_S = 5, 3, 240
KINDS = ("cross", "autocorr", "walk")


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
    if kind == "cross":
        bt.snapshot()
        bt.set_cross([(bt.snap(r), r) for r in range(B)])
    if kind == "walk":
        for e in bt.engines:
            e.save_reference()
    last = {}

    def run(n):
        if kind == "cross":
            rec = bt.propagate(DT, n, observe=dict(norm=False, per_replica=False, cross=True), every=1)
            last["value"] = complex(rec["mean_cross"][-1])
        elif kind == "autocorr":
            rec = bt.propagate(DT, n, observe=dict(norm=False, autocorr=True, per_replica=False), every=1)
            last["value"] = complex(rec["mean_autocorr"][-1])
        else:
            for _ in range(n):
                c = np.mean([e.overlap_reference() for e in bt.engines])
                bt.propagate(DT)
            last["value"] = complex(c)

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
    v = last["value"]
    rec = dict(probe="batch_cross_probe", kind=kind, B=B, P=B, L=L, d=d, D=D, M=M, dt=DT, steps=NSTEP, repeats=REPEATS,
               seconds_min=round(best, 6), ms_per_step=round(1e3 * best / NSTEP, 3), launches_per_step=round(launches, 2),
               last_mean=[round(v.real, 12), round(v.imag, 12)])
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
                print(json.dumps(dict(probe="batch_cross_probe", kind=kind, D=D, error=f"no result within {LIMIT_S} s")), flush=True)
                return 1  # nothing more is started on a device that may be in trouble
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(json.dumps(dict(probe="batch_cross_probe", kind=kind, D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
                if p.returncode < 0 or p.returncode in (134, 139):
                    return 1
                rc = 1
                continue
            print(line, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
