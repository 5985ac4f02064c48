"""GPU: thick restarts of the local Lanczos solve of the batched improved relaxation (TDVPBatch.set_relax_restarts /
relax_restarts, mitdvp_batch_set_relax_restarts: a solve of k_batch_relax that has not converged after max_diag_krylov
vectors keeps its lowest Ritz vector and the next Lanczos vector and goes on) and relax_trajectories(max_restarts=...).

The inputs are the chains of helpers/relax_cases; the references are the oracle's unrestarted solve (up to 3000 vectors) and
the restarted solve restated in NumPy (helpers/relax_restart_oracle, held against the oracle on the CPU by
tests/test_batch_relax_restart_host.py).  The bars are those of tests/test_gpu_batch_relax.py: fidelity defect < 1e-10,
energy within 1e-8 |E|, |norm - 1| < 1e-12.  Restart counts are printed, never compared: the solver stops on
rounding-level quantities once a site has converged."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FID, ENE, NRM = 1e-10, 1e-8, 1e-12
MOTIVE = ((4,) * 10, 16)  # with seed 3 the first step has a local solve of more than 64 vectors


def _engine(mpo, cores, shift=0.0, **kw):
    from pytdscf_amd import TDVPEngine

    e = TDVPEngine(len(mpo), relax="improved", **kw)
    e.set_mpo(mpo, shift=shift)
    e.set_mps(cores)
    return e


def _batch(items, restarts=None, **kw):
    from pytdscf_amd import TDVPBatch

    bt = TDVPBatch.from_engines([_engine(*it, **kw) for it in items])
    if restarts is not None:
        bt.set_relax_restarts(restarts)
    return bt


def _close(bt):
    engines = list(bt.engines)
    bt.close()
    for e in engines:
        e.close()


def _heis(dims, D, seeds):
    from helpers import relax_cases as rc

    return [(rc.heisenberg_mpo(dims, s), rc.start(dims, D, s)) for s in seeds]


def _tensors(bt):
    return [e.get_mps() for e in bt.engines]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check(got, ref_cores, ref_energy, what):
    from helpers import relax_cases as rc

    fid = rc.fidelity_defect(ref_cores, got["cores"])
    print(f"{what}: fidelity defect {fid:.2e}, energy {got['energy']:.12f} against {ref_energy:.12f}, |norm - 1| {abs(got['norm'] - 1):.2e}")
    assert fid < FID
    assert abs(got["energy"] - ref_energy) < ENE * abs(ref_energy)
    assert abs(got["norm"] - 1) < NRM


def _state(e):
    return dict(cores=e.get_mps(), energy=e.expectation().real, norm=e.norm())


def _mixed_items():
    """dims (3,) * 5, D = 4: field-only replicas 0 and 2 from product starts, Heisenberg replicas 1 and 3 from full-rank ones"""
    from helpers import relax_cases as rc

    dims, D = (3,) * 5, 4
    items = []
    for r in range(4):
        if r % 2 == 0:
            items.append((rc.field_mpo_wide(dims, r), rc.product_start(dims, D, r)))
        else:
            items.append((rc.heisenberg_mpo(dims, r), rc.start(dims, D, r)))
    return dims, items


# ---- 1. off is bitwise off ----
def test_off_is_bitwise_off():
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L6d3D6"]
    items = _heis(dims, D, seeds[:2])
    plain, zero, unused = _batch(items), _batch(items, 0), _batch(items, 8, max_diag_krylov=64)
    try:
        for bt in (plain, zero, unused):
            bt.propagate(0.0, 2)
            assert bt.statuses == [0, 0]
        for x, y, z in zip(_tensors(plain), _tensors(zero), _tensors(unused)):
            assert _same(x, y)
            assert _same(x, z)
        for bt in (plain, zero, unused):  # no solve of this case needs more than 64 vectors
            out = bt.relax_restarts()
            assert out["total"].dtype == np.int64 and out["most"].dtype == np.int32
            assert list(out["total"]) == [0, 0] and list(out["most"]) == [0, 0]
    finally:
        _close(plain)
        _close(zero)
        _close(unused)


def test_the_setter_refuses_what_the_header_says():
    from helpers import relax_cases as rc
    from pytdscf_amd import TDVPBatch, TDVPEngine

    dims, D = rc.MANY
    bt = _batch(_heis(dims, D, (0, 1)), 3)
    try:
        for bad in (-1, 4097):
            with pytest.raises(ValueError, match=rf"mitdvp_batch_set_relax_restarts: max_restarts = {bad}, .* 0 to 4096"):
                bt.set_relax_restarts(bad)
        bt.propagate(0.0, 1)  # the setting before a refused call is still in place: nothing here needs it, nothing breaks
        assert bt.statuses == [0, 0]
    finally:
        _close(bt)
    e = TDVPEngine(len(dims))  # real time
    e.set_mpo(rc.heisenberg_mpo(dims, 0))
    e.set_mps(rc.start(dims, D, 0))
    rt = TDVPBatch.from_engines([e])
    try:
        with pytest.raises(ValueError, match="mitdvp_batch_set_relax_restarts: the replicas have relax = 0"):
            rt.set_relax_restarts(4)
    finally:
        rt.close()
        e.close()


# ---- 2., 3. small caps against the oracle and against the NumPy model ----
@pytest.fixture(scope="module", params=[(4, 64), (8, 32)], ids=["kcap4", "kcap8"])
def small_cap(request):
    from helpers import relax_cases as rc

    kcap, max_restarts = request.param
    dims, D, seeds = rc.PARITY["L6d3D6"]
    bt = _batch(_heis(dims, D, seeds[:2]), max_restarts, max_diag_krylov=kcap)
    try:
        bt.propagate(0.0, 3)  # without restarts: "not converged in 4 basis"
        return dict(kcap=kcap, max_restarts=max_restarts, statuses=list(bt.statuses), restarts=bt.relax_restarts(),
                    states=[_state(e) for e in bt.engines])
    finally:
        _close(bt)


def test_small_caps_against_the_oracle(small_cap):
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L6d3D6"]
    assert small_cap["statuses"] == [0, 0]
    print("restarts", small_cap["restarts"])
    for r, s in enumerate(seeds[:2]):
        energies, kmax, _, cores = rc.oracle_relax("heis", dims, D, s, 3)
        print("oracle largest k per step", kmax)
        _check(small_cap["states"][r], cores, energies[-1], f"kcap {small_cap['kcap']} seed {s} against the oracle")
        assert small_cap["restarts"]["total"][r] > 0
        assert 0 < small_cap["restarts"]["most"][r] <= small_cap["max_restarts"]


def test_small_caps_against_the_numpy_model(small_cap):
    from helpers import relax_cases as rc
    from helpers import relax_restart_oracle as rro

    dims, D, seeds = rc.PARITY["L6d3D6"]
    for r, s in enumerate(seeds[:2]):
        m = rro.model_relax("heis", dims, D, s, 3, small_cap["kcap"], small_cap["max_restarts"])
        print(f"seed {s}: restarts, device {small_cap['restarts']['total'][r]} (most {small_cap['restarts']['most'][r]}), "
              f"model {m['total']} (most per step {m['most']})")
        _check(small_cap["states"][r], m["cores"], m["energies"][-1], f"kcap {small_cap['kcap']} seed {s} against the model")


# ---- 4. the default cap where it fails without restarts ----
def test_the_default_cap_with_and_without_restarts():
    from helpers import relax_cases as rc
    from pytdscf_amd import _lib

    dims, D = MOTIVE
    seeds = (0, 3)
    off, on = _batch(_heis(dims, D, seeds)), _batch(_heis(dims, D, seeds), 4)
    try:
        with pytest.raises(ValueError, match="Lanczos Diagonalization is not converged in 64 basis$"):
            off.propagate(0.0, 1)
        assert off.statuses == [0, _lib.ENOTCONV]
        on.propagate(0.0, 1)
        assert on.statuses == [0, 0]
        out = on.relax_restarts()
        print("restarts", out)
        for r, s in enumerate(seeds):
            energies, kmax, _, cores = rc.oracle_relax("heis", dims, D, s, 1)
            print("oracle largest k of the step", kmax)
            _check(_state(on[r]), cores, energies[-1], f"L10 d4 D16 seed {s}")
        assert out["most"][1] >= 1
    finally:
        _close(off)
        _close(on)


# ---- 5. exhaustion is a status ----
def test_restarts_that_run_out_are_a_status():
    from helpers import relax_cases as rc
    from pytdscf_amd import _lib

    dims, items = _mixed_items()
    bt = _batch(items, 2, max_diag_krylov=4)
    try:
        with pytest.raises(ValueError, match="Lanczos Diagonalization is not converged in 4 basis after 2 restarts$"):
            bt.relax(2)
        print("statuses", bt.statuses, "energies", bt.relaxed["energy"], "restarts", bt.relax_restarts())
        assert bt.statuses == [0, _lib.ENOTCONV, 0, _lib.ENOTCONV]
        for r in (0, 2):
            assert abs(bt.relaxed["energy"][r] - rc.field_ground_energy(dims, r)) < 1e-12
            assert bt.relaxed["steps"][r] == 2
    finally:
        _close(bt)


# ---- 6. a replica's bits do not depend on the batch ----
def test_a_replicas_bits_do_not_depend_on_the_batch():
    from helpers import relax_cases as rc

    dims, D = rc.MANY
    B = 70
    items = [(rc.heisenberg_mpo(dims, s % 7), rc.start(dims, D, s)) for s in range(B)]
    pick = [0, 33, 69]
    big, small = _batch(items, 64, max_diag_krylov=4), _batch([items[r] for r in pick], 64, max_diag_krylov=4)
    try:
        big.relax(2)
        small.relax(2)
        assert big.statuses == [0] * B
        rb, rs = big.relax_restarts(), small.relax_restarts()
        print("restarts of the three", [int(rb["total"][r]) for r in pick])
        for j, r in enumerate(pick):
            assert _same(big[r].get_mps(), small[j].get_mps())
            assert rb["total"][r] == rs["total"][j] and rb["most"][r] == rs["most"][j]
        assert sum(int(rb["total"][r]) for r in pick) > 0
    finally:
        _close(big)
        _close(small)


# ---- 7. one launch equals single steps ----
def test_one_launch_equals_single_steps_and_the_launch_count_stays():
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L8d2D4"]
    items = _heis(dims, D, seeds[:3])
    a, b = _batch(items, 32, max_diag_krylov=8), _batch(items, 32, max_diag_krylov=8)
    try:
        a.propagate(0.0, 1)  # builds the right blocks with the engines' own launches
        n0 = a.launches()
        a.propagate(0.0, 1)
        a.propagate(0.0, 1)
        assert a.launches() - n0 == 4  # two per step, whatever the restarts
        out = b.relax(3, 0.0)
        assert list(out["steps"]) == [3, 3, 3]
        for x, y in zip(_tensors(a), _tensors(b)):
            assert _same(x, y)
        ra, rb = a.relax_restarts(), b.relax_restarts()
        print("restarts", ra)
        assert np.array_equal(ra["total"], rb["total"]) and np.array_equal(ra["most"], rb["most"])
        assert (ra["total"] > 0).all()
        b.set_relax_restarts(32)  # the call clears the counters
        assert list(b.relax_restarts()["total"]) == [0, 0, 0] and list(b.relax_restarts()["most"]) == [0, 0, 0]
    finally:
        _close(a)
        _close(b)


# ---- 8. signed off-diagonals in the projected eigen-solve ----
def _restart_shaped_cases():
    """[(name, alpha, beta)] of the shape a restart leaves: alpha[0] a previous theta (the lowest eigenvalue of the matrix
    the rest is cut from), beta[0] of either sign from 1e-12 |T| to |T|, the rest random or recorded from a Lanczos run"""
    import scipy.linalg

    from helpers import relax_cases as rc

    recorded = max(rc.recorded_T(), key=lambda t: len(t[1]))
    out = []
    for k in (2, 3, 17, 64):
        rng = np.random.default_rng(500 + k)
        bases = [("random", rng.standard_normal(k), np.abs(rng.standard_normal(k - 1)) + 0.05)]
        if len(recorded[1]) >= k:
            bases.append(("recorded", recorded[1][:k].copy(), recorded[2][: k - 1].copy()))
        for kind, a0, b0 in bases:
            theta_prev = float(scipy.linalg.eigh_tridiagonal(a0, b0, eigvals_only=True)[0])
            tn = max(float(np.max(np.abs(a0))), abs(theta_prev))
            for sign in (1.0, -1.0):
                for f in (1e-12, 1e-6, 1e-3, 1.0):
                    a, b = a0.copy(), b0.copy()
                    a[0] = theta_prev
                    b[0] = sign * f * tn
                    out.append((f"{kind}-k{k}-{'+' if sign > 0 else '-'}{f:g}", a, b))
    return out


def _bars(a, b):
    """as helpers/relax_cases.tridiag_table derives them: 8 x the reference's own error (|theta_LAPACK - theta_longdouble|,
    the residual of LAPACK's pair), floored at k eps |T|_1; the vector bar is (residual bar) / gap where the gap exceeds
    1e-6 |T|_1, none otherwise"""
    import scipy.linalg

    from helpers import relax_cases as rc

    k = len(a)
    T = np.diag(a) + np.diag(b, 1) + np.diag(b, -1)
    t1 = float(np.max(np.sum(np.abs(T), axis=0)))
    w, v = scipy.linalg.eigh_tridiagonal(a, b)
    c = v[:, 0] * (-1.0 if v[0, 0] < 0 else 1.0)
    theta_err = float(abs(np.longdouble(w[0]) - rc._sturm_lowest_longdouble(a, b)))
    res = float(np.linalg.norm(T @ c - w[0] * c))
    floor = k * rc.EPS * t1
    gap = float(w[1] - w[0])
    bar_res = max(8.0 * res, floor)
    return dict(T=T, theta=float(w[0]), vec=c, bar_theta=max(8.0 * theta_err, floor), bar_res=bar_res,
                bar_vec=bar_res / gap if gap > 1e-6 * t1 else None)


def test_the_eigen_solve_takes_off_diagonals_of_either_sign():
    from pytdscf_amd import engine

    cases = _restart_shaped_cases()
    assert {len(a) for _, a, _ in cases} == {2, 3, 17, 64}
    assert any(b[0] < 0 for _, _, b in cases) and any(name.startswith("recorded-k64") for name, _, _ in cases)
    theta, vecs = engine.tridiag_lowest([a for _, a, _ in cases], [b for _, _, b in cases])
    misses = []
    for (name, a, b), th, c in zip(cases, theta, vecs):
        r = _bars(a, b)
        d_theta = abs(th - r["theta"])
        res = float(np.linalg.norm(r["T"] @ c - th * c))
        d_vec = float(np.linalg.norm(c - r["vec"]))
        print("%-22s |dtheta| %.2e (bar %.2e)  resid %.2e (bar %.2e)  |dvec| %.2e (bar %s)" % (
            name, d_theta, r["bar_theta"], res, r["bar_res"], d_vec, "-" if r["bar_vec"] is None else "%.2e" % r["bar_vec"]))
        ok = (len(c) == len(a) and d_theta <= r["bar_theta"] and res <= r["bar_res"] and c[0] >= 0 and
              abs(np.linalg.norm(c) - 1) <= 4 * len(a) * 2.3e-16 and (r["bar_vec"] is None or d_vec <= r["bar_vec"]))
        if not ok:
            misses.append(name)
    assert not misses


# ---- 9. relax_trajectories ----
def test_relax_trajectories_with_restarts():
    from helpers import relax_cases as rc
    from pytdscf_amd import Exciton, Model, relax_trajectories

    dims, D = rc.FULL_BOND
    seeds = (0, 1)
    models = [Model([Exciton(nstate=2) for _ in range(len(dims))], operators={"hamiltonian": rc.heisenberg_mpo(dims, s)}, bond_dim=D)
              for s in seeds]
    starts = [rc.start(dims, D, s) for s in seeds]
    plain = relax_trajectories(models, starts=starts, maxstep=6, conv_tol=1e-11)
    assert set(plain) == {"energy", "steps", "history", "states"}
    out = relax_trajectories(models, starts=starts, maxstep=6, conv_tol=1e-11, max_diag_krylov=8, max_restarts=32)
    print("energies", plain["energy"], out["energy"], "restarts", out["restarts"])
    assert set(out) == {"energy", "steps", "history", "states", "restarts"}
    assert out["restarts"].shape == (2,) and out["restarts"].dtype == np.int64 and (out["restarts"] > 0).all()
    for r in range(2):
        assert abs(out["energy"][r] - plain["energy"][r]) < ENE * abs(plain["energy"][r])
