"""The stepwise seam the tests of the edge / folded H_eff apply and of the structured environment update share
(tests/test_gpu_fold_apply.py, tests/test_gpu_env_fold.py, tests/test_gpu_fold_range.py): an engine created under chosen
MITDVP_* variables, moved to an interior site without any check behind its updates, then probed or solved there and
compared with the oracle's plain contractions."""

import os

import numpy as np

EDGE, FOLD_R, FOLD_L = 0x10, 0x20, 0x40
TOL = 1e-12  # relative, max norm: one complex128 contraction with the same summation lengths in another order


def crandn(rng, *s):
    a = rng.standard_normal(s + (2,))
    return a.view(np.complex128).reshape(s)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def engine_under(L, variables, **kw):
    """an engine with the given environment variables set while it is created (value None: the variable unset; a
    variable not named: left as it is), and without the one-launch small-bond kernels, which would take the shortest of
    the tests' shapes before any form is chosen"""
    from pytdscf_amd import TDVPEngine

    want = dict(variables)
    want["MITDVP_SMALL_KERNELS"] = "0"
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return TDVPEngine(L, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def to_site(eng, c):
    eng.build_envs(1)
    for _ in range(c):
        eng.split_center(True)
        eng.absorb_bond(True)
    assert eng.counters()["n_env_fold"] == 0  # no check ran before any of these updates


def check_center(orc, eng, mpo, c, rng, want_flags, tol=TOL):
    got, flags = eng.heff_apply_center()
    assert flags & 0x70 == want_flags, hex(flags)
    if flags & EDGE:
        assert flags & 7 == 0, hex(flags)
    Lb, Rb, psi = eng.get_env(0, c), eng.get_env(1, c + 1), eng.get_site(c)
    r = rel(got, orc.heff_apply(Lb, mpo[c], Rb, psi))
    print(f"site {c} shape {psi.shape} flags {flags:#x}: rel err {r:.3e}")
    assert r < tol
    x = crandn(rng, *psi.shape)  # a second vector through the same operators
    got, flags2 = eng.heff_apply_center(x)
    assert flags2 & 0x70 == flags & 0x70, hex(flags2)
    r = rel(got, orc.heff_apply(Lb, mpo[c], Rb, x))
    print(f"site {c} random vector: rel err {r:.3e}")
    assert r < tol


def split(orc, eng, mpo, c, forward):
    """split the centre c and return (block the library built, the oracle's update of the same inputs)"""
    if forward:
        env_in = eng.get_env(0, c)
        eng.split_center(True)
        return eng.get_env(0, c + 1), orc.env_update_left(env_in, eng.get_site(c), mpo[c])
    env_in = eng.get_env(1, c + 1)
    eng.split_center(False)
    return eng.get_env(1, c), orc.env_update_right(env_in, eng.get_site(c), mpo[c])


def solve_update_check(orc, eng, mpo, c, forward, want_fold, dt=0.1):
    n0 = eng.counters()["n_env_fold"]
    eng.site_exp(dt)  # the local solve: its check of the two blocks is what the update may rely on
    got, ref = split(orc, eng, mpo, c, forward)
    took = eng.counters()["n_env_fold"] - n0
    r = rel(got, ref)
    print(f"site {c} {'->' if forward else '<-'} block {got.shape}: structured {took:.0f}, rel err {r:.3e}")
    assert took == want_fold
    assert r < TOL
