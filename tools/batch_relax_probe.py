"""Ground states of an ensemble by improved relaxation: aggregate relaxation steps per second of (a) the batch
(TDVPBatch(relax="improved"): k_batch_relax, two launches per step whatever B, the Lanczos eigen-solve on the device:
"batch") and (b) the only route there was before it ("engines"): B TDVPEngine(relax="improved") stepped one after
another, each local solve reading partial sums back and solving the tridiagonal problem on the host after every Lanczos
vector -- in the same process on the same box, alternating, on the disordered spin-3/2 Heisenberg chain, L = 10, d = 4,
MPO bond 5, D = 16 and D = 32, B = 16 / 64 / 128 / 256, one disorder realisation per replica.
    python tools/batch_relax_probe.py [--only batch|engines]

What is timed is the SECOND relaxation step.  From a random start the first step's local solves at this shape take up to
about 60 Krylov vectors for most realisations and more than the default cap of 64 (max_diag_krylov) for some, which both
routes refuse in the same words; so every replica's first step is made beforehand, untimed, by an engine with
max_diag_krylov = 256, and both routes start from the states it leaves.

The condition is batch >= engines in aggregate steps per second at B = 128 at both shapes.  One JSON line per
measurement.  Every shape runs in a child process of its own under a time limit (a run that sits is ended and reported,
nothing more is started then).  Every repeat starts from the same states (set again before the clock starts); a warm-up,
then three timed repeats of NSTEP steps between device synchronisations, minimum reported.  Also recorded, without a
condition: launches per step, and the time per H_eff apply of a relaxation half-sweep against that of a real-time
half-sweep (k_batch_sweep) of the same shape and B = 128, from the apply counts the kernels keep -- what the inner
eigen-solve costs.  `--child KIND D` is one shape in this process (KIND batch, engines or both)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, d = 10, 4
BS = (16, 64, 128, 256)
NSTEP = 1
REPEATS, LIMIT_S = 3, 900
KINDS = ("batch", "engines")


def heisenberg_mpo(seed):
    """H = sum_p [(S+S- + S-S+)/2 + SzSz]_{p,p+1} + sum_p (h_p Sz + g_p Sx), spin (d - 1) / 2, h ~ U(-1, 1), g ~ U(-0.5, 0.5)"""
    import numpy as np

    rng = np.random.default_rng(seed)
    h, g = rng.uniform(-1.0, 1.0, L), rng.uniform(-0.5, 0.5, L)
    s = (d - 1) / 2.0
    m = s - np.arange(d)
    sz = np.diag(m).astype(np.complex128)
    sp = np.zeros((d, d), dtype=np.complex128)
    for k in range(1, d):
        sp[k - 1, k] = np.sqrt(s * (s + 1) - m[k] * (m[k] + 1))
    sm = sp.conj().T.copy()
    eye = np.eye(d, dtype=np.complex128)
    cores = []
    for p in range(L):
        w = np.zeros((5, d, d, 5), dtype=np.complex128)
        w[0, :, :, 0], w[1, :, :, 0], w[2, :, :, 0], w[3, :, :, 0] = eye, sm, sp, sz
        w[4, :, :, 0] = h[p] * sz + g[p] * 0.5 * (sp + sm)
        w[4, :, :, 1], w[4, :, :, 2], w[4, :, :, 3], w[4, :, :, 4] = 0.5 * sp, 0.5 * sm, sz, eye
        if p == 0:
            w = w[4:5]
        if p == L - 1:
            w = w[:, :, :, 0:1]
        cores.append(np.ascontiguousarray(w))
    return cores


def measure(kind, D):
    import pytdscf_amd as P
    from pytdscf_amd.engine import device_sync

    bmax = max(BS)
    bt_all = P.TDVPBatch(bmax, L, relax="improved")
    for r, e in enumerate(bt_all.engines):
        e.set_mpo(heisenberg_mpo(r))
        e.init_random([d] * L, D, seed=1 + r)
        e.set_small_kernels(False)
    prep = P.TDVPEngine(L, relax="improved", max_diag_krylov=256)
    starts = []
    for r, e in enumerate(bt_all.engines):  # the first step, untimed
        prep.set_mpo(heisenberg_mpo(r))
        prep.set_mps(e.get_mps())
        prep.propagate(0.0)
        starts.append(prep.get_mps())
    yield dict(probe="batch_relax_probe", kind="first_step", D=D, largest_krylov_dimension_of_replica_255=max(prep.krylov_memory(p) for p in range(L)))
    prep.close()

    def timed(engines, run):
        def reset():
            for e, s in zip(engines, starts):
                e.set_mps(s)

        reset()
        run()  # warm-up: buffers, tables, the right blocks' buffers, clocks
        best, launches, applies = None, 0, 0
        for _ in range(REPEATS):
            reset()
            for e in engines:
                e.counters_reset()
            device_sync(0)
            t0 = time.perf_counter()
            run()
            device_sync(0)
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
            cs = [e.counters() for e in engines]
            launches = sum(c["n_launch"] for c in cs)
            applies = sum(c["n_heff"] for c in cs)
        return best, launches, applies

    for B in BS:
        engines = bt_all.engines[:B]
        bt = P.TDVPBatch.from_engines(engines)
        for which in (KINDS if kind == "both" else (kind,)):  # alternating: batch, engines, batch, ... over B
            def loop():
                for e in engines:
                    for _ in range(NSTEP):
                        e.propagate(0.0)

            try:
                best, launches, applies = timed(engines, (lambda: bt.propagate(0.0, NSTEP)) if which == "batch" else loop)
            except ValueError as ex:  # a local solve that needs more than max_diag_krylov vectors: no figure for this row
                yield dict(probe="batch_relax_probe", kind=which, B=B, L=L, d=d, D=D, error=str(ex))
                continue
            yield dict(probe="batch_relax_probe", kind=which, B=B, L=L, d=d, D=D, nstep=NSTEP, repeats=REPEATS,
                       ms_per_call=round(1e3 * best, 3), steps_per_s=round(B * NSTEP / best, 2),
                       launches_per_step=round(launches / NSTEP, 1), heff_applies=int(applies))
        bt.close()
    if kind in ("both", "batch"):  # what the inner eigen-solve costs: a relaxation half-sweep against a real-time one
        B = 128
        engines = bt_all.engines[:B]
        bt = P.TDVPBatch.from_engines(engines)
        t_rx, _, a_rx = timed(engines, lambda: bt.sweep(0.0, True))
        bt.close()
        rt = P.TDVPBatch(B, L)
        for r, e in enumerate(rt.engines):
            e.set_mpo(heisenberg_mpo(r))
        t_rt, _, a_rt = timed(rt.engines, lambda: rt.sweep(0.01, True))
        c_rt = sum(e.counters()["n_keff"] for e in rt.engines)
        rt.close()
        yield dict(probe="batch_relax_probe", kind="apply_cost", B=B, L=L, d=d, D=D,
                   relax_half_sweep_ms=round(1e3 * t_rx, 3), relax_heff_applies_per_replica=round(a_rx / B, 1),
                   relax_us_per_heff_apply=round(1e6 * t_rx / (a_rx / B), 2),
                   realtime_half_sweep_ms=round(1e3 * t_rt, 3), realtime_heff_applies_per_replica=round(a_rt / B, 1),
                   realtime_keff_applies_per_replica=round(c_rt / B, 1),
                   realtime_us_per_heff_apply=round(1e6 * t_rt / (a_rt / B), 2))
    for e in bt_all.engines:
        e.close()


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
            print(json.dumps(dict(probe="batch_relax_probe", D=D, error=f"no result within {LIMIT_S} s")), flush=True)
            return 1  # nothing more is started on a device that may be in trouble
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            print(json.dumps(dict(probe="batch_relax_probe", D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
            return 1
        print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
