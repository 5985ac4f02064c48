"""H_eff applies at the centre of a CANONICAL chain under the bench's generators (identity blocks in the environments, the
finite-state-machine / direct-sum MPO cores): exactly the kernels a local exponential issues (mitdvp_heff_apply_center),
reps times after one warm-up, for rocprofv3 kernel-trace / PMC passes.  Every call chooses the forms again, so with the
folded variant of the edge form it builds the folded operators once and applies them once: the device timers printed at
the end give both (stage 1 = the build, or the transpose of an unfolded L side; stages 0 / 2 = the L / R side products).
With MITDVP_FOLD_STRASSEN=1 the build also packs the seven factors of each folded operator and stages 0 / 2 are the seven
half-size products with their two small kernels (MITDVP_STRASSEN_BATCH=1: one batched launch); with =2 the build packs 49
factors per operator and the stages are 49 quarter-size products with their four small kernels.  PROBE_BEGIN names the
Strassen levels the two sides took.  groups > 1 repeats the timed loop and prints one PROBE_END line per group: the
spread of repeated timings.
    [MITDVP_EDGE_APPLY=0|1] [MITDVP_FOLD_APPLY=0|1] [MITDVP_FOLD_STRASSEN=0|1|2] [MITDVP_STRASSEN_BATCH=1]
        python tools/heff_center_probe.py C3|C5|C4|L,d,D,M [reps] [groups]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pytdscf_amd import TDVPEngine, synthetic as syn

name = sys.argv[1] if len(sys.argv) > 1 else "C3"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 6
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
x = eng.get_site(c)
_, flags = eng.heff_apply_center(x)  # warm-up (also builds the cached reduced cores of the edge form)
levels = [2 if flags & hi else 1 if flags & lo else 0 for lo, hi in ((0x100, 0x400), (0x80, 0x200))]
print(f"PROBE_BEGIN {name} site {c} shape {shape} flags {flags} Strassen levels L {levels[0]} R {levels[1]} reps {reps}", flush=True)
eng.set_profiling(True)
for _ in range(groups):
    eng.counters_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.heff_apply_center(x)
    wall = (time.perf_counter() - t0) / reps * 1e3
    k = eng.counters()
    st = [v / reps for v in k["heff_stage_ms"]]
    print(f"PROBE_END {wall:.3f} ms per call (with host copies); device ms per call: L side {st[0]:.3f}  "
          f"build/transpose {st[1]:.3f}  R side {st[2]:.3f}  sum {sum(st):.3f}", flush=True)
eng.close()
