"""MPO matrix elements between the replicas of a batch: time per call of (a) TDVPBatch.cross_mpo() over the B diagonal
entries (r, r, 0) of operator 0 (k_batch_cross_mpo: "cross_mpo"), (b) TDVPBatch.expect() of operator 0 for the B replicas
(k_batch_expect: "expect"), and (c) the host route the request replaces ("host"): get_mps() of both states of every entry
plus the NumPy walk of the left block per entry -- at the shapes of profiles/batch_probe.txt, L = 10, d = 4, M = 6, D = 16
and D = 32, B = 128.   python tools/batch_cross_mpo_probe.py [--only cross_mpo|expect|host]

(a) and (b) do the same three products per site at the same sizes -- (a) from the left over all L sites with two tensors,
(b) from the right to bond 1 and one H_eff apply -- so their kernels should cost about the same; (c) only has to lose to
(a).  One JSON line per measurement.  Every measurement runs in a child process of its own under a time limit (a run that
sits is ended and reported, nothing more is started then); a warm-up, then three timed repeats with a device
synchronisation on both sides, minimum reported.
`--child KIND D` is one measurement in this process; `--child both D` runs leg (a) and then leg (b) in ONE process: the
form to put behind a profiler (kernel trace and statistics on their own, no counter collection, the program behind `--`),
to read the mean duration of k_batch_cross_mpo next to k_batch_expect's in the same run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d, M, DT, B = 10, 4, 6, 0.5, 128
NCALL, REPEATS, LIMIT_S = 5, 3, 240
KINDS = ("cross_mpo", "expect", "host")


def host_walk(bra, ket, mpo):
    """<bra| O |ket> by the walk of the left block (bra bond, MPO bond, ket bond) in the kernel's three stages"""
    import numpy as np

    T = np.ones((1, 1, 1), dtype=np.complex128)
    for b, k, W in zip(bra, ket, mpo):
        X = np.einsum("bca,bps->caps", np.conj(b), T)
        Y = np.einsum("pctq,caps->aqts", W, X)
        T = np.einsum("aqts,str->aqr", Y, k)
    return complex(T[0, 0, 0])


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
    bt.propagate(DT, 1)  # the state a batch step leaves: centre at site 0
    bt.set_cross_mpo([(r, r, 0) for r in range(B)])
    bt.set_expect([0])
    w = np.full(B, 1.0 / B)
    last = {}

    def run(which, n):
        for _ in range(n):
            if which == "cross_mpo":
                last["value"] = bt.cross_mpo()["mean"]
            elif which == "expect":
                last["value"] = complex(bt.expect(per_replica=False)["mean"][0])
            else:
                vals = []
                for e in bt.engines:
                    bra, ket = e.get_mps(), e.get_mps()  # the two states of an entry come off the device separately
                    vals.append(host_walk(bra, ket, mpo))
                last["value"] = complex(w @ np.array(vals))

    out = []
    for which in (("cross_mpo", "expect") if kind == "both" else (kind,)):
        run(which, 2)  # warm-up: buffers, tables, clocks
        for e in bt.engines:
            e.counters_reset()
        best = None
        for _ in range(REPEATS):
            device_sync(0)
            t0 = time.perf_counter()
            run(which, NCALL)
            device_sync(0)
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
        launches = sum(e.counters()["n_launch"] for e in bt.engines) / (REPEATS * NCALL)
        out.append(dict(probe="batch_cross_mpo_probe", kind=which, B=B, entries=B, L=L, d=d, D=D, M=M, calls=NCALL, repeats=REPEATS,
                        seconds_min=round(best, 6), ms_per_call=round(1e3 * best / NCALL, 3), launches_per_call=round(launches, 2),
                        mean_re=round(last["value"].real, 12), mean_im=round(last["value"].imag, 12)))
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
    rc = 0
    for D in (16, 32):
        for kind in KINDS:
            if a.only and kind != a.only:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, str(D)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(probe="batch_cross_mpo_probe", kind=kind, D=D, error=f"no result within {LIMIT_S} s")), flush=True)
                return 1  # nothing more is started on a device that may be in trouble
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(json.dumps(dict(probe="batch_cross_mpo_probe", kind=kind, D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)),
                      flush=True)
                if p.returncode < 0 or p.returncode in (134, 139):
                    return 1
                rc = 1
                continue
            print(line, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
