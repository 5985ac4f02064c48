"""An MPO applied to the replicas of a batch: time per call of (a) TDVPBatch.operate over all B replicas (k_batch_operate,
ONE launch and one host wait: "batch") and (b) the route it replaces ("engines"): the loop of TDVPEngine.operate over the
same B engines, dozens of launches per site and one host wait per site and sweep each -- in the same process on the same
box, at the shapes of profiles/batch_probe.txt, L = 10, d = 4, M = 6, D = 16 and D = 32, B = 128, with a dipole-like
synthetic MPO (sum_p mu_p, its bond padded with zeros to M), maxstep = 4 and conv_tol = 0, so that both sides run the same
four double sweeps.   python tools/batch_operate_probe.py [--only batch|engines]

The condition is batch <= engines at both shapes.  One JSON line per measurement.  Every shape runs in a child process of
its own under a time limit (a run that sits is ended and reported, nothing more is started then).  Every repeat starts from
the same states (set again before the clock starts); a warm-up, then three timed repeats with a device synchronisation on
both sides, minimum reported.  `--child KIND D` is one shape in this process (KIND batch, engines or both): `--child batch D`
is the form to put behind a profiler (kernel trace and statistics on their own, no counter collection, the program behind
`--`) to read the mean duration of k_batch_operate."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, B = 10, 4, 6, 128
MAXSTEP, TOL = 4, 0.0
REPEATS, LIMIT_S = 3, 400
KINDS = ("batch", "engines")


def dipole_mpo(seed=5):
    """sum_p mu_p with a ladder-like mu of its own per site, as an MPO whose bond is padded with zeros from 2 to M"""
    import numpy as np

    rng = np.random.default_rng(seed)
    cores = []
    for p in range(L):
        mu = np.diag(np.sqrt(np.arange(1.0, d)), 1)
        mu = (mu + mu.T) * (1.0 + 0.1 * rng.standard_normal())
        w = np.zeros((1 if p == 0 else M, d, d, 1 if p == L - 1 else M), dtype=np.complex128)
        eye = np.eye(d)
        if p == 0:
            w[0, :, :, 0], w[0, :, :, 1] = eye, mu
        elif p == L - 1:
            w[0, :, :, 0], w[1, :, :, 0] = mu, eye
        else:
            w[0, :, :, 0], w[0, :, :, 1], w[1, :, :, 1] = eye, mu, eye
        cores.append(w)
    return cores


def measure(kind, D):
    import numpy as np

    import pytdscf_amd as P
    from pytdscf_amd.engine import device_sync

    mpo = dipole_mpo()
    bt = P.TDVPBatch(B, L)
    for r, e in enumerate(bt.engines):
        e.set_mpo(mpo)
        e.init_random([d] * L, D, seed=1 + r)
    starts = [e.get_mps() for e in bt.engines]
    last = {}

    def reset():
        for e, s in zip(bt.engines, starts):
            e.set_mps(s)

    def run(which):
        if which == "batch":
            got = bt.operate(0, maxstep=MAXSTEP, conv_tol=TOL)
            last["norm"], last["iters"] = float(got["norms"].mean()), int(got["iterations"].max())
        else:
            res = [e.operate(0, maxstep=MAXSTEP, conv_tol=TOL) for e in bt.engines]
            last["norm"], last["iters"] = float(np.mean([r[0] for r in res])), max(r[1] for r in res)

    out = []
    for which in (KINDS if kind == "both" else (kind,)):
        reset()
        run(which)  # warm-up: buffers, tables, clocks
        best, launches = None, 0
        for _ in range(REPEATS):
            reset()
            for e in bt.engines:
                e.counters_reset()
            device_sync(0)
            t0 = time.perf_counter()
            run(which)
            device_sync(0)
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
            launches = sum(e.counters()["n_launch"] for e in bt.engines)
        out.append(dict(probe="batch_operate_probe", kind=which, B=B, L=L, d=d, D=D, M=M, maxstep=MAXSTEP, conv_tol=TOL, repeats=REPEATS,
                        ms_per_call=round(1e3 * best, 3), launches_per_call=launches, mean_norm=round(last["norm"], 12),
                        iterations=last["iters"]))
    bt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=KINDS)
    ap.add_argument("--child", nargs=2, metavar=("KIND", "D"))
    a = ap.parse_args()
    if a.child:
        for rec in measure(a.child[0], int(a.child[1])):
            print(json.dumps(rec), flush=True)
        return 0
    for D in (16, 32):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", a.only or "both", str(D)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(probe="batch_operate_probe", D=D, error=f"no result within {LIMIT_S} s")), flush=True)
            return 1  # nothing more is started on a device that may be in trouble
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            print(json.dumps(dict(probe="batch_operate_probe", D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
            return 1
        print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
