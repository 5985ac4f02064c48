"""Thick restarts of the batched improved relaxation's local Lanczos solve (TDVPBatch.set_relax_restarts): what they
cost when no solve needs one, the row of tools/batch_relax_probe.py that had no figure, and what a small max_diag_krylov
costs in applies.  The method is that of tools/batch_relax_probe.py: the disordered spin-3/2 Heisenberg chain, L = 10,
d = 4, MPO bond 5, one realisation per replica; the SECOND relaxation step is timed (the first, from a random start, is made
beforehand, untimed, by an engine with max_diag_krylov = 256); the settings alternate in one process; every repeat starts
from the same states; a warm-up, then the minimum of three repeats between device synchronisations.
    python tools/batch_relax_restart_probe.py [--tree DIR] [--parent]

Rows, one JSON line each:
  unused      B = 128, max_diag_krylov = 64, the setter never called ("none") against max_restarts = 8, twice each,
              alternating: no solve restarts there, so the two must cost the same.
  no_figure   B = 256, max_restarts = 4: at D = 32 a realisation needs more than 64 vectors in its second step.
  small_cap   B = 128, max_diag_krylov = 16 and 32 with max_restarts = 64: steps per second, H_eff applies and restarts
              next to those of the 64-vector solve -- what a 4 x / 2 x smaller Krylov carve costs.
--tree DIR imports the package from another checkout (the parent commit, built beside this one) and --parent measures the
"none" rows only, which is all the parent has: run parent, branch, parent in one session; the parent's two runs give its
own run-to-run spread, the allowed shortfall of the branch.  Every shape runs in a child process of its own under a time
limit; a run that sits is ended and reported, and nothing more is started then.  `--child D` is one shape in this process."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L, d = 10, 4
NSTEP = 1
REPEATS, LIMIT_S = 3, 900


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


def measure(D, parent):
    import pytdscf_amd as P
    from pytdscf_amd.engine import device_sync

    bmax = 128 if parent else 256
    mpos = [heisenberg_mpo(r) for r in range(bmax)]
    seedling = P.TDVPEngine(L, relax="improved")
    prep = P.TDVPEngine(L, relax="improved", max_diag_krylov=256)
    starts, kmax = [], 0
    for r in range(bmax):  # the first step, untimed
        seedling.set_mpo(mpos[r])
        seedling.init_random([d] * L, D, seed=1 + r)
        prep.set_mpo(mpos[r])
        prep.set_mps(seedling.get_mps())
        prep.propagate(0.0)
        kmax = max(kmax, max(prep.krylov_memory(p) for p in range(L)))
        starts.append(prep.get_mps())
    seedling.close()
    prep.close()
    yield dict(probe="batch_relax_restart_probe", kind="first_step", D=D, replicas=bmax, largest_krylov_dimension=kmax)

    def batch_of(B, kcap):
        bt = P.TDVPBatch(B, L, relax="improved", **({"max_diag_krylov": kcap} if kcap else {}))
        for r, e in enumerate(bt.engines):
            e.set_mpo(mpos[r])
            e.set_mps(starts[r])
            e.set_small_kernels(False)
        return bt

    def timed(bt, B, max_restarts):
        def reset():
            for e, s in zip(bt.engines, starts):
                e.set_mps(s)

        reset()
        if max_restarts is not None:
            bt.set_relax_restarts(max_restarts)
        bt.propagate(0.0, NSTEP)  # warm-up: buffers, tables, the right blocks' buffers, clocks
        best, applies, restarts, most = None, 0, 0, 0
        for _ in range(REPEATS):
            reset()
            for e in bt.engines:
                e.counters_reset()
            if max_restarts is not None:
                bt.set_relax_restarts(max_restarts)  # clears the counters
            device_sync(0)
            t0 = time.perf_counter()
            bt.propagate(0.0, NSTEP)
            device_sync(0)
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
            applies = sum(e.counters()["n_heff"] for e in bt.engines)
            if max_restarts is not None:
                rr = bt.relax_restarts()
                restarts, most = int(rr["total"].sum()), int(rr["most"].max())
        return dict(ms_per_step=round(1e3 * best / NSTEP, 3), steps_per_s=round(B * NSTEP / best, 2), heff_applies=int(applies),
                    restarts=restarts, most_restarts_of_one_solve=most)

    def row(kind, bt, B, kcap, max_restarts):
        base = dict(probe="batch_relax_restart_probe", kind=kind, B=B, L=L, d=d, D=D, max_diag_krylov=kcap or 64,
                    max_restarts="none" if max_restarts is None else max_restarts)
        try:
            return dict(base, **timed(bt, B, max_restarts))
        except ValueError as ex:  # a local solve that did not converge: no figure for this row
            return dict(base, error=str(ex))

    bt = batch_of(128, 0)
    for _ in range(2):
        for mr in ((None,) if parent else (None, 8)):
            yield row("unused", bt, 128, 0, mr)
    bt.close()
    if parent:
        return
    bt = batch_of(256, 0)
    yield row("no_figure", bt, 256, 0, 0)
    yield row("no_figure", bt, 256, 0, 4)
    bt.close()
    for kcap in (16, 32, 64):
        bt = batch_of(128, kcap)
        yield row("small_cap", bt, 128, kcap, 64)
        bt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the checkout to import pytdscf_amd from")
    ap.add_argument("--parent", action="store_true", help="the rows a build without restarts has")
    ap.add_argument("--child", metavar="D")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if a.child:
        sys.path.insert(0, tree)
        for rec in measure(int(a.child), a.parent):
            print(json.dumps(dict(rec, tree="parent" if a.parent else "branch")), flush=True)
        return 0
    for D in (16, 32):
        cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--child", str(D)] + (["--parent"] if a.parent else [])
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S, cwd=tree)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(probe="batch_relax_restart_probe", D=D, error=f"no result within {LIMIT_S} s")), flush=True)
            return 1  # nothing more is started on a device that may be in trouble
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            print(json.dumps(dict(probe="batch_relax_restart_probe", D=D, error=(p.stderr or p.stdout)[-400:], rc=p.returncode)), flush=True)
            return 1
        print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
