"""Excited states by deflation: what the stored states cost a relaxation step of the batch.  The time of one relaxation
step (TDVPBatch(relax="improved").propagate(0, 1): two launches) with 0, 1 and 4 slots of the deflation set filled
(k_batch_relax against k_batch_relax_defl), on the disordered spin-3/2 Heisenberg chain of tools/batch_relax_probe.py,
L = 10, d = 4, MPO bond 5, D = 16 and D = 32, B = 128, one disorder realisation per replica.
    python tools/batch_deflate_probe.py

Three batches of B replicas each live in one process, one per slot count; a window times one step of each of them in
turn (0, 1, 4, 0, 1, 4, ...), every time from the same states, set again before the clock starts; the median of 7
windows is reported, with the H_eff applies per replica and step from the counters the kernels keep (a penalised
operator has another spectrum, so the solves take another number of vectors: time per apply is the comparable figure).
As in batch_relax_probe the step that is timed is the SECOND one: every replica's first step from its random start is
made beforehand, untimed, by an engine with max_diag_krylov = 256.  The stored states are random normalised states of
the replicas' shapes with weight 4; local solves may restart (set_relax_restarts(16)) in all three batches alike.

There is no pass bar.  One JSON line per measurement.  Every shape runs in a child process of its own under a time
limit (a run that sits is ended and reported, nothing more is started then): at most two processes at a time.
`--child D` is one shape in this process."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from batch_relax_probe import L, d, heisenberg_mpo  # noqa: E402

B = 128
SLOTS = (0, 1, 4)
WINDOWS, LIMIT_S = 7, 420
WEIGHT = 4.0


def measure(D):
    import pytdscf_amd as P
    from pytdscf_amd.engine import device_sync

    prep = P.TDVPEngine(L, relax="improved", max_diag_krylov=256)
    starts = []
    for r in range(B):  # the first step, untimed
        prep.set_mpo(heisenberg_mpo(r))
        prep.init_random([d] * L, D, seed=1 + r)
        prep.propagate(0.0)
        starts.append(prep.get_mps())
    prep.close()

    batches = {}
    for K in SLOTS:
        bt = P.TDVPBatch(B, L, relax="improved")
        for r, e in enumerate(bt.engines):
            e.set_mpo(heisenberg_mpo(r))
        bt.set_relax_restarts(16)
        for k in range(K):
            for r, e in enumerate(bt.engines):
                e.init_random([d] * L, D, seed=100000 * (k + 1) + r)
            bt.deflate_push(WEIGHT)
        assert bt.deflate_count() == K
        batches[K] = bt

    def one(bt):
        for e, s in zip(bt.engines, starts):
            e.set_mps(s)
        for e in bt.engines:
            e.counters_reset()
        device_sync(0)
        t0 = time.perf_counter()
        bt.propagate(0.0, 1)
        device_sync(0)
        el = time.perf_counter() - t0
        cs = [e.counters() for e in bt.engines]
        return el, sum(c["n_heff"] for c in cs), sum(c["n_launch"] for c in cs), sum(c["heff_flops"] for c in cs)

    for K in SLOTS:
        one(batches[K])  # warm-up: buffers, tables, the right blocks' buffers, clocks
    times = {K: [] for K in SLOTS}
    last = {}
    for _ in range(WINDOWS):
        for K in SLOTS:
            el, applies, launches, flops = one(batches[K])
            times[K].append(el)
            last[K] = (applies, launches, flops)
    base = statistics.median(times[0])
    for K in SLOTS:
        med = statistics.median(times[K])
        applies, launches, flops = last[K]
        yield dict(probe="batch_deflate_probe", slots=K, B=B, L=L, d=d, D=D, windows=WINDOWS, ms_per_step=round(1e3 * med, 3),
                   ms_min=round(1e3 * min(times[K]), 3), ms_max=round(1e3 * max(times[K]), 3), against_no_slots=round(med / base, 3),
                   heff_applies_per_replica_and_step=round(applies / B, 1), us_per_heff_apply=round(1e6 * med / (applies / B), 2),
                   launches_per_step=launches, counted_gflop_per_step=round(flops / 1e9, 2))
    for bt in batches.values():
        bt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="D")
    a = ap.parse_args()
    if a.child:
        for rec in measure(int(a.child)):
            print(json.dumps(rec), flush=True)
        return 0
    for D in (16, 32):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(D)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(probe="batch_deflate_probe", D=D, error=f"no result within {LIMIT_S} s")), flush=True)
            return 1  # nothing more is started on a device that may be in trouble
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            print(json.dumps(dict(probe="batch_deflate_probe", D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
            return 1
        print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
