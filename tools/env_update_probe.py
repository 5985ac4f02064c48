"""Environment updates at the centre of a CANONICAL chain under the bench's generators, exactly as a sweep issues them: the
check of a local solve (mitdvp_heff_apply_center), the QR split and the update of the next block (mitdvp_split_center),
then the bond matrix goes back into the site so the same update runs again -- reps times after one warm-up, in both
directions.  Device ms per update from the engine's phase timer 1 (env_ms / n_env); n_env_fold tells which form ran:
the structured one (Gram matrix + folded operator) or, with MITDVP_FOLD_ENV=0, the M-fold chain; n_env_reuse how many of
those took the operator from the solve's Strassen factors (MITDVP_FOLD_ENV_REUSE=0: none).  groups > 1 repeats the timed
round and prints one line per group: the spread of repeated timings.
    [MITDVP_FOLD_ENV=0|1] [MITDVP_FOLD_ENV_REUSE=0] python tools/env_update_probe.py C3|C5|C4|L,d,D,M [reps] [groups]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytdscf_amd import TDVPEngine, synthetic as syn

name = sys.argv[1] if len(sys.argv) > 1 else "C3"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
groups = int(sys.argv[3]) if len(sys.argv) > 3 else 1
cfgs = {"C3": (6, 32, 128, 16, False), "C5": (14, 4, 512, 16, True), "C4": (7, 16, 1024, 32, False)}
cfg = cfgs[name] if name in cfgs else tuple(int(v) for v in name.split(",")) + (False,)
L, d, D, M, liou = cfg
mpo = syn.synthetic_liouvillian_mpo(L, M, seed=0, gamma=0.002) if liou else syn.synthetic_mpo(L, d, M, seed=0)
eng = TDVPEngine(L, integrator="arnoldi" if liou else "lanczos", conserve_norm=not liou)
eng.set_mpo(mpo)
eng.init_random([d] * L, D, seed=1)
c = L // 2
eng.build_envs(1)
for _ in range(c):
    eng.split_center(True)
    eng.absorb_bond(True)
shape = eng.get_site_shape(c)[:3]
for forward in (True, False):
    for timed in [False] + [True] * groups:  # one warm-up round (builds the cached cores), then the timed ones
        eng.set_profiling(timed)
        eng.counters_reset()
        for _ in range(reps if timed else 1):
            eng.heff_apply_center()
            eng.split_center(forward)
            eng.absorb_bond(not forward)
        if not timed:
            continue
        k = eng.counters()
        print(f"ENV_PROBE {name} site {c} shape {shape} {'->' if forward else '<-'} FOLD_ENV={os.environ.get('MITDVP_FOLD_ENV', 'def')}: "
              f"{k['env_ms'] / max(k['n_env'], 1):.3f} ms per update (device), {k['n_env']} updates, {k['n_env_fold']:.0f} structured, "
              f"{k.get('n_env_reuse', 0):.0f} with the solve's operator", flush=True)
eng.close()
