"""The cases of tests/test_gpu_small_chain.py: chains of the one-launch small-bond kernel (k_small_site) with the slice of
the chip and the launch plan each is meant to run under, and the references in extended precision.  A case names its
regime as a set of words; ``regime_of`` derives the same words from a plan, so that a test can assert that the kernel ran
what the case is named after (tests/test_small_plan_host.py checks the table against the planner on the CPU)."""

from __future__ import annotations

import numpy as np

SS_THREADS = 512  # threads of a workgroup: the operand prefetch takes 1 / 2 / 4 trips of it for A / R / W


def crandn(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def extents(kind, dims):
    """(slabs na, contracted right index ns, elements of a resident A slab, R rows per chunk column, W elements)"""
    if kind == "heff":
        dl, d, dr, ml, mr = dims
        return dict(na=dl, ns=dr, a_slab=ml * dl, r_per_cs=mr * dr, nw=d * mr * ml * d)
    if kind == "keff":
        d1, d2, m = dims
        return dict(na=d1, ns=d2, a_slab=m * d1, r_per_cs=m * d2, nw=0)
    din, min_, d, dout, mout = dims
    return dict(na=dout, ns=din, a_slab=d * din, r_per_cs=d * dout, nw=mout * d * d * min_)


def regime_of(kind, dims, plan):
    """the words that describe a plan (a dict with nsc, cs, spw, a_resident, sg_aliases_x)"""
    e = extents(kind, dims)
    nsc, cs, spw, res = plan["nsc"], plan["cs"], plan["spw"], plan["a_resident"]
    w = {f"nsc{nsc}"}
    if nsc * cs > e["ns"]:
        w.add("ragged_chunk")  # the last chunk is narrower than cs
    if spw > 1:
        w.add("spw")
        w.add("resident" if res else "restaged")
        if e["na"] % spw:
            w.add("short_group")  # the last workgroup of a chunk has fewer than spw slabs
    w.add("sg_aliases_x" if plan["sg_aliases_x"] else "sg_apart")
    if res and e["a_slab"] * min(spw, e["na"]) > SS_THREADS:
        w.add("tail_A")
    if e["r_per_cs"] * cs > 2 * SS_THREADS:
        w.add("tail_R")
    if e["nw"] > 4 * SS_THREADS:
        w.add("tail_W")
    return w


class ApplyCase:
    """kind "heff" (dl, d, dr, ml, mr), "keff" (d1, d2, m) or "env" (din, min, d, dout, mout; ``left``: the -> update);
    ``cu``: compute units of the slice (0: the whole chip, 256 on MI355X); ``plan``: (nsc, cs, spw, a_resident) expected;
    ``regime``: words that must be among ``regime_of`` the plan that ran"""

    def __init__(self, kind, dims, cu, plan, regime, shift=0.0, left=True):
        self.kind, self.dims, self.cu, self.plan, self.regime, self.shift, self.left = kind, dims, cu, plan, set(regime), shift, left
        self.id = (f"{kind}{'' if kind != 'env' else ('-left' if left else '-right')}-" + "x".join(map(str, dims)) +
                   f"-cu{cu or 'all'}" + ("-shift" if shift else ""))

    @property
    def n_cu(self):
        return self.cu or 256


SHIFT = 0.7 - 1.3j

# the starting points are those of a port of the planner; each is verified against the planner itself
APPLY_CASES = [
    # chunks over s: 1, 2 (ragged), 4 (ragged), 8
    ApplyCase("heff", (5, 3, 4, 3, 2), 0, (1, 4, 1, 1), {"nsc1", "sg_aliases_x"}),
    ApplyCase("heff", (7, 10, 21, 6, 6), 0, (2, 11, 1, 1), {"nsc2", "ragged_chunk", "tail_R", "tail_W"}),
    ApplyCase("heff", (7, 10, 21, 6, 6), 0, (2, 11, 1, 1), {"nsc2", "ragged_chunk"}, shift=SHIFT),
    ApplyCase("heff", (37, 10, 21, 6, 6), 0, (4, 6, 1, 1), {"nsc4", "ragged_chunk"}),
    ApplyCase("keff", (80, 80, 6), 64, (8, 10, 16, 0), {"nsc8", "spw", "restaged", "sg_apart", "tail_R"}),
    # several slabs per workgroup, the last group short: A resident, A re-staged, and with ragged chunks as well
    ApplyCase("heff", (7, 10, 21, 6, 6), 8, (2, 11, 2, 1), {"spw", "resident", "short_group", "ragged_chunk"}),
    ApplyCase("heff", (13, 10, 21, 6, 6), 16, (2, 11, 2, 1), {"nsc2", "spw", "resident", "short_group", "ragged_chunk"}),
    ApplyCase("heff", (37, 10, 21, 6, 6), 64, (4, 6, 4, 1), {"nsc4", "spw", "resident", "short_group", "ragged_chunk", "tail_A"},
              shift=SHIFT),
    ApplyCase("heff", (37, 10, 21, 6, 6), 16, (4, 6, 16, 0), {"nsc4", "spw", "restaged", "short_group", "ragged_chunk"}),
    ApplyCase("heff", (21, 10, 13, 6, 6), 16, (1, 13, 2, 0), {"nsc1", "spw", "restaged", "short_group"}, shift=SHIFT),
    ApplyCase("heff", (40, 6, 33, 7, 5), 64, (4, 9, 4, 1), {"spw", "resident", "ragged_chunk", "tail_A", "tail_R"}),
    # K_eff: no W stage, Sg never aliases X
    ApplyCase("keff", (37, 37, 6), 0, (2, 19, 1, 1), {"nsc2", "ragged_chunk", "sg_apart", "tail_R"}, shift=SHIFT),
    ApplyCase("keff", (37, 37, 6), 16, (2, 19, 8, 1), {"spw", "resident", "short_group", "ragged_chunk", "sg_apart", "tail_A"},
              shift=SHIFT),
    ApplyCase("keff", (37, 37, 6), 8, (2, 19, 16, 1), {"spw", "resident", "short_group", "sg_apart", "tail_A"}),
    ApplyCase("keff", (13, 29, 5), 8, (1, 29, 2, 1), {"nsc1", "spw", "resident", "short_group", "sg_apart"}),
    # environment updates, both directions; (33, 5, 6, 40, 7): a W stage whose Sg does not fit into X
    ApplyCase("env", (21, 6, 10, 13, 6), 16, (2, 11, 2, 1), {"nsc2", "spw", "resident", "short_group", "ragged_chunk"}, left=True),
    ApplyCase("env", (13, 6, 10, 21, 6), 16, (1, 13, 2, 0), {"spw", "restaged", "short_group", "tail_R"}, left=False),
    ApplyCase("env", (33, 5, 6, 40, 7), 0, (4, 9, 1, 1), {"nsc4", "ragged_chunk", "sg_apart"}, left=True),
    ApplyCase("env", (33, 5, 6, 40, 7), 8, (4, 9, 32, 0), {"nsc4", "spw", "restaged", "short_group", "ragged_chunk", "sg_apart"},
              left=False),
    # bond dimension 1 on either side, on the smallest slice
    ApplyCase("heff", (1, 4, 6, 1, 5), 8, (1, 6, 1, 1), {"nsc1"}),
    ApplyCase("heff", (7, 2, 1, 4, 1), 8, (1, 1, 1, 1), {"nsc1"}),
]

# every regime the kernel has must be named by at least one case
REQUIRED = [
    {"nsc1"}, {"nsc2", "ragged_chunk"}, {"nsc4", "ragged_chunk"}, {"nsc8"},
    {"spw", "short_group", "resident"}, {"spw", "short_group", "restaged"},
    {"spw", "short_group", "ragged_chunk"},
    {"sg_apart"}, {"tail_A"}, {"tail_R"}, {"tail_W"},
]


# ---------------------------------------------------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------------------------------------------------
def operands(case, seed=0):
    """the operands of ``engine.small_apply`` for a case, complex normal"""
    rng = np.random.default_rng(4100 + seed)
    if case.kind == "heff":
        dl, d, dr, ml, mr = case.dims
        return crandn(rng, dl, ml, dl), crandn(rng, ml, d, d, mr), crandn(rng, dr, mr, dr), crandn(rng, dl, d, dr)
    if case.kind == "keff":
        d1, d2, m = case.dims
        return crandn(rng, d1, m, d1), crandn(rng, d2, m, d2), crandn(rng, d1, d2)
    din, min_, d, dout, mout = case.dims
    if case.left:  # env (din, min, din), site (din, d, dout), W (min, d, d, mout) -> (dout, mout, dout)
        return crandn(rng, din, min_, din), crandn(rng, din, d, dout), crandn(rng, min_, d, d, mout)
    # env (din, min, din) right of the site (dout, d, din), W (mout, d, d, min) -> (dout, mout, dout)
    return crandn(rng, din, min_, din), crandn(rng, dout, d, din), crandn(rng, mout, d, d, min_)


def _ld(x):
    return np.asarray(x, dtype=np.clongdouble)


def _chain(*steps):
    """pairwise einsum contractions in the precision of the operands (a four-operand einsum would walk every index at once)"""
    x = steps[0]
    for spec, y in steps[1:]:
        x = np.einsum(spec, x, y)
    return x


def reference(case, ops, dtype=np.clongdouble):
    """the formulas of csrc/small_site.h, evaluated in ``dtype``:
      H_eff  sigma[a,i,r] = sum L[a,c,b] W[c,i,j,t] R[r,t,s] psi[b,j,s] + shift psi
      K_eff  sigma'[a,r]  = sum L[a,c,b] sigma[b,s] R[r,c,s] + shift sigma
      env -> out[a,q,r] = sum conj(T)[b,i,a] env[b,c,s] W[c,i,j,q] T[s,j,r]
      env <- out[a,c,r] = sum conj(T)[a,i,b] env[b,q,s] W[c,i,j,q] T[r,j,s]"""
    ops = [np.asarray(x, dtype=dtype) for x in ops]
    shift = dtype(case.shift)
    if case.kind == "heff":
        L, W, R, psi = ops
        return _chain(L, ("acb,bjs->acjs", psi), ("acjs,cijt->aits", W), ("aits,rts->air", R)) + shift * psi
    if case.kind == "keff":
        L, R, sig = ops
        return _chain(L, ("acb,bs->acs", sig), ("acs,rcs->ar", R)) + shift * sig
    env, T, W = ops
    if case.left:
        return _chain(np.conj(T), ("bia,bcs->iacs", env), ("iacs,cijq->asjq", W), ("asjq,sjr->aqr", T))
    return _chain(np.conj(T), ("aib,bqs->aiqs", env), ("aiqs,cijq->asjc", W), ("asjc,rjs->acr", T))


def oracle(case, ops):
    """the same through the project's oracle, complex128 (a cross-check of the formulas above)"""
    from oracle import tdvp_oracle as orc

    if case.kind == "heff":
        L, W, R, psi = ops
        return orc.heff_apply(L, W, R, psi) + case.shift * psi
    if case.kind == "keff":
        L, R, sig = ops
        return orc.keff_apply(L, R, sig) + case.shift * sig
    env, T, W = ops
    return orc.env_update_left(env, T, W) if case.left else orc.env_update_right(env, T, W)


# ---------------------------------------------------------------------------------------------------------------------
# EXP mode: one-site problems (helpers.local_exp.Seam) whose site or bond solve the planner lays out differently on
# slices of 8, 16 and 64 compute units and on the whole chip (0)
# ---------------------------------------------------------------------------------------------------------------------
ALL_CONFIGS = ("lanczos-reference", "lanczos-orthodox", "arnoldi", "lanczos-reference-shift100", "lanczos-orthodox-shift100",
               "arnoldi-shift100", "lanczos-reference-relax", "lanczos-orthodox-relax", "arnoldi-relax",
               "lanczos-reference-shift100-relax", "lanczos-orthodox-shift100-relax", "arnoldi-shift100-relax")
PLAIN_CONFIGS = ("lanczos-reference", "lanczos-orthodox", "arnoldi")
# Bond solves of a relaxation with the offset 100 are exp(+(100 + k) / 2): approximants of norm 5e21 whose differences stall
# where the projected exponential rounds, so whether twenty vectors "converge" is decided by rounding (the reference
# raises; test_gpu_local_exp.test_bond_solve holds the device to either verdict with a dense exp at n = 64).  At n = 1369
# there is no dense reference to hold the other verdict against: those three configurations are left to that test.
BOND_CONFIGS = tuple(c for c in ALL_CONFIGS if not c.endswith("shift100-relax"))


class ExpCase:
    """``shape``: (dl, d, dr, m) of the seam; ``kind`` "heff": the site solve, "keff": the bond solve right of the site
    after a forward split; ``slices``: (compute units, plan expected in EXP mode, words of its regime)"""

    def __init__(self, kind, shape, slices, configs):
        dl, d, dr, m = shape
        self.kind, self.shape, self.slices, self.configs = kind, shape, slices, configs
        self.chain_dims = (dl, d, dr, m, m) if kind == "heff" else (dr, dr, m)
        self.n = dl * d * dr if kind == "heff" else dr * dr
        self.id = ("site-" if kind == "heff" else "bond-") + "x".join(map(str, shape))


EXP_SITE = [
    ExpCase("heff", (13, 10, 21, 6), [
        (8, (2, 11, 4, 0), {"nsc2", "spw", "restaged", "short_group", "ragged_chunk"}),
        (16, (2, 11, 2, 1), {"nsc2", "spw", "resident", "short_group", "ragged_chunk"}),
        (64, (2, 11, 1, 1), {"nsc2", "ragged_chunk"}),
        (0, (2, 11, 1, 1), {"nsc2", "ragged_chunk"})], ALL_CONFIGS),
    ExpCase("heff", (37, 10, 21, 6), [
        (8, (4, 6, 32, 0), {"nsc4", "spw", "restaged", "short_group", "ragged_chunk"}),
        (16, (4, 6, 16, 0), {"nsc4", "spw", "restaged", "short_group", "ragged_chunk"}),
        (64, (4, 6, 4, 1), {"nsc4", "spw", "resident", "short_group", "ragged_chunk", "tail_A"}),
        (0, (4, 6, 1, 1), {"nsc4", "ragged_chunk"})], PLAIN_CONFIGS),
]
EXP_BOND = [
    ExpCase("keff", (13, 4, 37, 6), [
        (8, (2, 19, 16, 0), {"nsc2", "spw", "restaged", "short_group", "ragged_chunk", "sg_apart"}),
        (16, (2, 19, 8, 1), {"nsc2", "spw", "resident", "short_group", "ragged_chunk", "sg_apart", "tail_A"}),
        (64, (2, 19, 2, 1), {"nsc2", "spw", "resident", "short_group", "ragged_chunk", "sg_apart"}),
        (0, (2, 19, 1, 1), {"nsc2", "ragged_chunk", "sg_apart"})], BOND_CONFIGS),
]


def exp_config(cfg_id):
    from helpers import local_exp as lx

    return next(c for c in lx.ENGINE_CONFIGS if c.id == cfg_id)


def heff_ld(sm):
    """the seam's H_eff with the contraction in np.clongdouble, the result rounded to complex128"""
    L, W, R = _ld(sm.L), _ld(sm.W), _ld(sm.R)

    def mv(x):
        x = _ld(x)
        y = _chain(L, ("acb,bjs->acjs", x), ("acjs,cijt->aits", W), ("aits,rts->air", R))
        return (y + np.clongdouble(sm.shift) * x).astype(np.complex128)

    return mv


def keff_ld(sm, Lp):
    L, R = _ld(Lp), _ld(sm.R)

    def mv(s):
        s = _ld(s)
        return (_chain(L, ("acb,bs->acs", s), ("acs,rcs->ar", R)) + np.clongdouble(sm.shift) * s).astype(np.complex128)

    return mv


_BOND_REFS: dict = {}


def bond_problem(case, cfg):
    """the seam of a bond case, the oracle's forward split of its centre (A, sigma) and the threshold placed for two
    chained bond solves from sigma (the device's QR may pick another gauge: a unitarily equivalent problem)"""
    from helpers import local_exp as lx
    from oracle import tdvp_oracle as orc

    key = (case.id, cfg.id)
    if key not in _BOND_REFS:
        sm = lx.seam_for(case.shape, cfg)
        A0, sig0 = orc.qr_psi2Asigma(sm.psi)
        mv = sm.keff(sm.keff_blocks(A0)[0])
        thresh = lx.placed_thresh(cfg.integrator, cfg.variant, cfg.bond_scale(), mv, sig0, 0, cfg.cn, chained=True)
        _BOND_REFS[key] = (sm, A0, sig0, thresh)
    return _BOND_REFS[key]


def bond_reference(sm, cfg, A, sigma, thresh):
    """two bond solves in a row by the statement-level reference from the split (A, sigma): the second from the first's
    result with the first's k as memory.  No dense K_eff."""
    from helpers import local_exp as lx

    Lp, _ = sm.keff_blocks(A)
    s, mv = cfg.bond_scale(), sm.keff(Lp)
    r = lx.Ref()
    r.Lp, r.raises = Lp, None
    try:
        r.y1, r.k1, r.d1 = lx.sil(cfg.integrator, cfg.variant, s, mv, sigma, thresh, 0, cfg.cn)
        r.y2, r.k2, r.d2 = lx.sil(cfg.integrator, cfg.variant, s, mv, r.y1, thresh, r.k1, cfg.cn)
    except ValueError as e:
        r.raises = str(e)
    return r


def eligibility(case, cfg):
    """CPU-side numbers behind the use of lx.PARITY at a new shape: the reference's two solves (k, the margins of its last
    two differences against the placed threshold) and how far the same solves with an extended-precision matvec land from
    them.  Returns a dict; ``ok``: well separated and the two precisions within PARITY / 10."""
    from helpers import local_exp as lx

    if case.kind == "heff":
        r = lx.site_reference(case.shape, cfg, dense=False)
        sm, x0, s, mv_ld = r.seam, r.seam.psi, cfg.site_scale(), heff_ld(r.seam)
        thresh = r.thresh
    else:
        sm, A0, x0, thresh = bond_problem(case, cfg)
        r = bond_reference(sm, cfg, A0, x0, thresh)
        s, mv_ld = cfg.bond_scale(), keff_ld(sm, r.Lp)
    out = dict(case=case.id, cfg=cfg.id, thresh=thresh, raises=r.raises)
    if r.raises:
        out["ok"] = False
        return out
    z1, kz1, _ = lx.sil(cfg.integrator, cfg.variant, s, mv_ld, x0, thresh, 0, cfg.cn)
    z2, kz2, _ = lx.sil(cfg.integrator, cfg.variant, s, mv_ld, r.y1, thresh, r.k1, cfg.cn)
    out.update(k=(r.k1, r.k2), k_ld=(kz1, kz2), margins=(lx.margins(r.d1, thresh), lx.margins(r.d2, thresh)),
               separated=lx.well_separated(r.d1, thresh) and lx.well_separated(r.d2, thresh),
               precision=max(lx.err(z1, r.y1), lx.err(z2, r.y2)))
    out["ok"] = bool(out["separated"] and out["k"] == out["k_ld"] and out["precision"] <= lx.PARITY / 10)
    return out
