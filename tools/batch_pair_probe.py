"""Batched trajectories with nearest-neighbour (pair) channels: aggregate time steps per second of a batch (a) with no
channel, (b) with a pair jump channel (K = 4) on bond (4, 5) and (c) with pair gates on every bond, at the shapes of
profiles/batch_probe.txt: L = 10, d = 4, M = 6, D = 16 and D = 32, B = 128; (b) and (c) also as a ratio to (a) of the same
run.   python tools/batch_pair_probe.py [--only none|jump|gates] [--D 16]

One JSON line per measurement.  Every measurement runs in a child process of its own under a time limit (a run that sits
is ended and reported, nothing more is started then); a warm-up, then three timed repeats with a device synchronisation on
both sides, minimum reported.  Nothing else does this work, so there is no bar to meet; the mean duration of k_batch_pair
is read from a `rocprofv3 --kernel-trace --stats -- python tools/batch_pair_probe.py --child gates D` run of its own,
without counter collection."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, DT, B, BOND, K = 10, 4, 6, 0.5, 128, (4, 5), 4
NSTEP, REPEATS, LIMIT_S = 5, 3, 240
KINDS = ("none", "jump", "gates")


def kraus_set(rng, n):
    """K random n x n matrices rescaled to sum B^+ B = 1"""
    import numpy as np

    G = rng.standard_normal((K, n, n)) + 1j * rng.standard_normal((K, n, n))
    w, V = np.linalg.eigh(sum(g.conj().T @ g for g in G))
    return G @ ((V / np.sqrt(w)) @ V.conj().T)


def unitary(rng, n):
    import numpy as np

    Q, R = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return Q * (np.diag(R) / np.abs(np.diag(R)))


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
    if kind == "jump":
        bt.set_jumps({BOND: kraus_set(rng, d * d)}, seed=1)
    elif kind == "gates":
        bt.set_gates({(q, q + 1): unitary(rng, d * d) for q in range(L - 1)})
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
    rec = dict(probe="batch_pair_probe", kind=kind, B=B, L=L, d=d, D=D, M=M, K=K, dt=DT, steps=NSTEP, repeats=REPEATS,
               seconds_min=round(best, 6), ms_per_step=round(1e3 * best / NSTEP, 3), aggregate_steps_per_s=round(B * NSTEP / best, 1),
               launches_per_step=round(launches, 2), pair_jumps_counted=int(bt.pair_jump_counts().sum()),
               discarded_weight_max=float(bt.discarded_weight().max()), norm0=round(float(bt[0].norm()), 12))
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
        base = None
        for kind in KINDS:
            if a.only and kind != a.only:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, str(D)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(probe="batch_pair_probe", kind=kind, D=D, error=f"no result within {LIMIT_S} s")), flush=True)
                return 1  # nothing more is started on a device that may be in trouble
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(json.dumps(dict(probe="batch_pair_probe", kind=kind, D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
                return 1  # whatever failed, nothing more is started
            rec = json.loads(line)
            if kind == "none":
                base = rec["aggregate_steps_per_s"]
            elif base:
                rec["ratio_to_none"] = round(rec["aggregate_steps_per_s"] / base, 4)
            print(json.dumps(rec), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
