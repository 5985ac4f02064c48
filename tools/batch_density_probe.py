"""Batched trajectories with multi-site reduced densities: time per time step of a batch (a) unobserved, (b) in a recorded
run with the pair keys (4, 4, 5, 5) and (2, 2, 7, 7) observed every step (k_batch_density: one more launch per record) and
(c) the only way to the same numbers without it: TDVPBatch.propagate(dt) followed by TDVPEngine.reduced_density(legs) over
all engines, at the shapes of profiles/batch_probe.txt: L = 10, d = 4, M = 6, D = 16 and D = 32, B = 128.
    python tools/batch_density_probe.py [--only step|keys|walk] [--D 16]

One JSON line per measurement and a verdict line per shape.  Every measurement runs in a child process of its own under a
time limit, and the first one that fails, faults or sits ends the script: nothing more is started then.  A warm-up, then
three timed repeats with a device synchronisation on both sides, minimum reported.  Condition: (b) <= (c) at both shapes
((c) pays a stream synchronisation per replica and key that (b) does not have).  The mean duration of k_batch_density is
read from a `rocprofv3 --kernel-trace --stats -- python tools/batch_density_probe.py --child keys D` run of its own,
without counter collection."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, DT, B = 10, 4, 6, 0.5, 128
KEYS = [(4, 4, 5, 5), (2, 2, 7, 7)]
NSTEP, REPEATS, LIMIT_S = 5, 3, 300
KINDS = ("step", "keys", "walk")


def measure(kind, D):
    import numpy as np

    import pytdscf_amd as P
    from pytdscf_amd import synthetic as syn
    from pytdscf_amd.engine import density_key_legs, device_sync

    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    bt = P.TDVPBatch(B, L)
    for r, e in enumerate(bt.engines):
        e.set_mpo(mpo)
        e.init_random([d] * L, D, seed=1 + r)
    legs = [density_key_legs(k, L) for k in KEYS]

    def walk():
        return [np.mean([e.reduced_density(lg) for e in bt.engines], axis=0) for lg in legs]

    def run():
        if kind == "step":
            bt.propagate(DT, NSTEP)
        elif kind == "keys":
            bt.propagate(DT, NSTEP, observe=dict(norm=False, keys=KEYS), every=1)
        else:
            walk()
            for _ in range(NSTEP):
                bt.propagate(DT)
                walk()

    bt.propagate(DT, 2)  # warm-up: Krylov memories, workspaces, clocks
    run()
    for e in bt.engines:
        e.counters_reset()
    best = None
    for _ in range(REPEATS):
        device_sync(0)
        t0 = time.perf_counter()
        run()
        device_sync(0)
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    launches = bt.launches() / (REPEATS * NSTEP)
    rec = dict(probe="batch_density_probe", kind=kind, B=B, L=L, d=d, D=D, M=M, dt=DT, keys=[list(k) for k in KEYS], steps=NSTEP,
               records=NSTEP + 1 if kind != "step" else 0, repeats=REPEATS, seconds_min=round(best, 6),
               ms_per_step=round(1e3 * best / NSTEP, 3), launches_per_step=round(launches, 2))
    if kind == "keys":  # outside the timed region: the batch's means against the walk over the engines, same state
        got = bt.densities(KEYS, per_replica=False)["mean_density"]
        rec["defect_vs_engines"] = float(max(np.abs(g - w).max() for g, w in zip(got, walk())))
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
        ms = {}
        for kind in KINDS:
            if a.only and kind != a.only:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, str(D)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(probe="batch_density_probe", kind=kind, D=D, error=f"no result within {LIMIT_S} s")), flush=True)
                return 1  # nothing more is started on a device that may be in trouble
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(json.dumps(dict(probe="batch_density_probe", kind=kind, D=D, error=(p.stderr or p.stdout)[-400:],
                                      rc=p.returncode)), flush=True)
                return 1
            print(line, flush=True)
            ms[kind] = json.loads(line)["ms_per_step"]
        if "keys" in ms and "walk" in ms:
            ok = ms["keys"] <= ms["walk"]
            print(json.dumps(dict(probe="batch_density_probe", D=D, condition="recorded run with keys <= walk over the engines",
                                  keys_ms_per_step=ms["keys"], walk_ms_per_step=ms["walk"], met=ok)), flush=True)
            rc = rc or (0 if ok else 1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
