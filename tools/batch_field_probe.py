"""Batched trajectories with time-dependent one-site fields: milliseconds per time step of a batch (a) with no field,
(b) with a field on every site (k_batch_field: the unitaries in place, the left blocks rebuilt), (c) with the SAME
unitaries set once as gates (k_batch_channel's walk: two gauge moves per site besides) and (d) with set_gates called
before every single step, which is the only way the gate route can follow a pulse: it gives up the run's single host wait.
L = 10, d = 4, M = 6, D = 16 and D = 32, B = 128.   python tools/batch_field_probe.py [--D 16] [--out FILE]

One JSON line per shape.  Each shape runs in a child process of its own under a time limit (a run that sits is ended and
reported, nothing more is started then).  In the child the four batches live side by side and are timed in turn, repeat
after repeat, so that what else the box does falls on all of them alike; a warm-up, then REPEATS windows of NSTEP steps,
a host clock around calls that end in the batch's host wait, device synchronised on both sides; the median is reported,
with the smallest and largest window."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, DT, B, AMP = 10, 4, 6, 0.5, 128, 0.7
NSTEP, REPEATS, LIMIT_S = 10, 7, 420
KINDS = ("none", "field", "gates_once", "gates_every_step")


def measure(D):
    import numpy as np

    import pytdscf_amd as P
    from pytdscf_amd import synthetic as syn
    from pytdscf_amd.engine import device_sync

    rng = np.random.default_rng(0)
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    G = []
    for _ in range(L):
        X = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        G.append((X + X.conj().T) / 2)
    gates = {}
    for p in range(L):  # exp(-i dt a G) of the decomposition the field route is given
        g, V = np.linalg.eigh(G[p])
        gates[p] = (V * np.exp(-1j * DT * AMP * g)) @ V.conj().T
    fields = {p: dict(G=G[p], pulse=np.full(4 + NSTEP * (REPEATS + 1), AMP)) for p in range(L)}

    def make(kind):
        bt = P.TDVPBatch(B, L)
        for r, e in enumerate(bt.engines):
            e.set_mpo(mpo)
            e.init_random([d] * L, D, seed=1 + r)
        if kind == "field":
            bt.set_fields(fields)
        elif kind != "none":
            bt.set_gates(gates)
        return bt

    def run(kind, bt, n):
        if kind == "gates_every_step":
            for _ in range(n):
                bt.set_gates(gates)
                bt.propagate(DT, 1)
        else:
            bt.propagate(DT, n)

    batches = {k: make(k) for k in KINDS}
    for k, bt in batches.items():
        run(k, bt, 2)  # warm-up: Krylov memories, workspaces, clocks
    l0 = {k: bt.launches() for k, bt in batches.items()}
    times = {k: [] for k in KINDS}
    for _ in range(REPEATS):
        for k, bt in batches.items():
            device_sync(0)
            t0 = time.perf_counter()
            run(k, bt, NSTEP)
            device_sync(0)
            times[k].append(1e3 * (time.perf_counter() - t0) / NSTEP)
    rec = dict(probe="batch_field_probe", B=B, L=L, d=d, D=D, M=M, dt=DT, steps=NSTEP, repeats=REPEATS)
    for k, bt in batches.items():
        rec[k] = dict(ms_per_step_median=round(statistics.median(times[k]), 3), ms_min=round(min(times[k]), 3),
                      ms_max=round(max(times[k]), 3), launches_per_step=round((bt.launches() - l0[k]) / (REPEATS * NSTEP), 2))
    # the two routes apply the same unitaries: the states agree
    a, b = batches["field"], batches["gates_once"]
    T = np.ones((1, 1), dtype=np.complex128)
    for x, y in zip(a[0].get_mps(), b[0].get_mps()):
        T = np.einsum("ab,ajs,bjt->st", T, np.conj(x), y)
    rec["norm_field"], rec["norm_gates"] = round(float(a[0].norm()), 12), round(float(b[0].norm()), 12)
    rec["fidelity_defect_field_vs_gates"] = float(1 - abs(T[0, 0]) / (rec["norm_field"] * rec["norm_gates"]))
    base = rec["none"]["ms_per_step_median"]
    rec["field_launch_ms"] = round(rec["field"]["ms_per_step_median"] - base, 3)
    rec["gate_walk_ms"] = round(rec["gates_once"]["ms_per_step_median"] - base, 3)
    for bt in batches.values():
        bt.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, choices=(16, 32))
    ap.add_argument("--out", help="also append the JSON lines to this file")
    ap.add_argument("--child", type=int, metavar="D")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child)), flush=True)
        return 0
    rc = 0
    for D in (16, 32):
        if a.D and D != a.D:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(D)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(probe="batch_field_probe", D=D, error=f"no result within {LIMIT_S} s")), flush=True)
            return 1  # nothing more is started on a device that may be in trouble
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
        if p.returncode != 0 or line is None:
            print(json.dumps(dict(probe="batch_field_probe", D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
            return 1
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
