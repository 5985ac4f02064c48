"""CPU: the batched operator application (TDVPBatch.operate, mitdvp_batch_operate, k_batch_operate) without a GPU -- the
entry point is declared, exported and documented; the carve of the request's buffer and its cap
(csrc/batch_operate_plan.h, compiled with g++ into a throw-away shim); the NumPy twin of the kernel's walk against the
oracle and the reference's golden result; the conditioning of every case the GPU test uses; the iteration-count cases and
their gaps; the argument checks of the Python front end, raised before any engine exists; and the oracle route of the
correlated-start correlation function against dense expm."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_entry_point_is_declared_and_bound():
    from pytdscf_amd import _lib

    header = open(os.path.join(ROOT, "include", "mitdvp.h")).read()
    assert "int mitdvp_batch_operate(mitdvp_batch* b, int op_id, int maxstep, double conv_tol, const int* replicas, int nsel," in header
    assert "mitdvp_batch_operate" in _lib.declared_symbols()
    assert "mitdvp_batch_operate(" in open(os.path.join(ROOT, "pytdscf_amd", "csrc", "capi.hip")).read()
    assert "batch_operate_plan.h" in open(os.path.join(ROOT, "pytdscf_amd", "csrc", "Makefile")).read()
    from pytdscf_amd import TDVPBatch

    assert callable(TDVPBatch.operate)


# ---- the carve and the cap, through a g++ shim ----
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("bop_shim") / "libbop_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "helpers", "operate_plan_shim.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    lib.bop_plan.restype = C.c_char_p
    lib.bop_plan.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_longlong)]
    lib.bop_fits.restype = C.c_char_p
    lib.bop_fits.argtypes = [C.c_ulonglong, C.c_ulonglong]
    lib.bop_max_bytes.restype = C.c_ulonglong
    return lib


NAMES = ("ket", "prev", "mix", "ov", "x", "y", "work", "spare", "h", "sig", "t0", "t1", "id", "total")


def _rows(name, label):
    """[L][5]: the site shapes of the shape with the operator's MPO bonds"""
    from helpers import expect_cases as ec
    from helpers import operate_cases as oc
    from oracle import tdvp_oracle as orc

    dims, D = oc.SHAPES[name]
    _, _, mpo = ec.case(name, label)
    return [[dl, d, dr, w.shape[0], w.shape[3]] for (dl, dr), d, w in zip(orc.bond_dims(list(dims), D), dims, mpo)]


def _plan(shim, rows, op_id=0):
    L = len(rows)
    arr = np.ascontiguousarray(rows, dtype=np.int32)
    out = (C.c_ulonglong * 14)()
    tabs = (C.c_longlong * (3 * (L + 1)))()
    msg = shim.bop_plan(arr.ctypes.data_as(C.POINTER(C.c_int)), op_id, L, out, tabs)
    t = np.array(list(tabs)).reshape(3, L + 1)
    return (None if msg is None else msg.decode()), dict(zip(NAMES, out)), t


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_the_carve_has_room_for_everything_and_nothing_overlaps(shim, name):
    from helpers import operate_cases as oc

    assert shim.bop_max_mpo() == 16 and shim.bop_max_bytes() == 1 << 32
    for label in oc.LABELS:
        rows = _rows(name, label)
        L = len(rows)
        msg, o, (site, mix, ov) = _plan(shim, rows)
        assert msg is None
        n = [dl * d * dr for dl, d, dr, _, _ in rows]
        # the ragged regions: site tensors and blocks at their true sizes, block b left of site b, block L the boundary
        assert list(np.diff(site)) == n and site[0] == 0
        assert list(np.diff(mix)) == [dl * ml * dl for dl, _, _, ml, _ in rows] and mix[0] == 0
        assert list(np.diff(ov)) == [dl * dl for dl, _, _, _, _ in rows] and ov[0] == 0
        assert len(set(np.diff(mix))) > 1  # ragged indeed
        nxy = max(k * max(r[3], r[4]) for k, r in zip(n, rows))
        nb = max(max(r[0], r[2]) for r in rows) ** 2
        need = {"ket": site[L], "prev": site[L], "mix": mix[L] + 1, "ov": ov[L] + 1, "x": nxy, "y": nxy, "work": max(n), "spare": max(n),
                "h": max(n), "sig": nb, "t0": nb, "t1": nb, "id": max(r[1] for r in rows) ** 2}
        order = NAMES[:-1]
        assert o["ket"] == 0
        for a, b in zip(order, order[1:] + ("total",)):  # every region ends where the next begins, or before
            assert o[a] + need[a] <= o[b], (a, b)
        assert o["total"] % 16 == 0 and o["total"] - o["id"] - need["id"] < 16


def test_the_plan_refuses_bad_mpo_bonds(shim):
    ok = _rows("mixed", "local")
    assert _plan(shim, ok, 5)[0] is None
    bad = [list(r) for r in ok]
    bad[1][4] = bad[2][3] = 17
    assert "operator 5, site 1: MPO bonds (%d, 17): the batched kernel takes MPO bonds of 1 to 16" % ok[1][3] in _plan(shim, bad, 5)[0]
    bad = [list(r) for r in ok]
    bad[2][3] += 1
    assert "the core of site 2 has the left MPO bond %d" % bad[2][3] in _plan(shim, bad, 5)[0]
    bad = [list(r) for r in ok]
    bad[-1][4] = 2
    assert "operator 5: the outer MPO bonds are (1, 2), they must be 1" in _plan(shim, bad, 5)[0]
    bad = [list(r) for r in ok]
    bad[0][3] = 0
    assert "MPO bonds of 1 to 16" in _plan(shim, bad, 5)[0]


def test_the_buffer_cap_names_both_figures_and_what_fits(shim):
    _, o, _ = _plan(shim, _rows("wide", "longrange"))
    total = o["total"]
    fit = (1 << 32) // (16 * total)
    assert shim.bop_fits(fit, total) is None and shim.bop_fits(1, total) is None
    msg = shim.bop_fits(fit + 1, total).decode()
    assert f"{fit + 1} replicas of {16 * total} bytes each need a buffer of {(fit + 1) * 16 * total} bytes" in msg
    assert f"the limit is {1 << 32} bytes: at most {fit} replicas fit" in msg
    assert fit > 1000  # the envelope of the trajectory workflows


# ---- the NumPy twin of the kernel's walk ----
@pytest.mark.parametrize("maxstep", [1, 10])
def test_the_twin_gives_the_golden_state(maxstep):
    from helpers import jump_oracle as jo
    from helpers import operate_cases as oc
    from oracle import tdvp_oracle as orc

    mpo, start, res = oc.golden()
    ref_norm, ref_state = res[maxstep]
    nrm, bra, it, status = oc.twin(start, mpo, 0.0, maxstep, 1e-8, seed=maxstep)
    assert it == maxstep and status == 0
    assert abs(nrm - ref_norm) < 1e-10 * ref_norm
    assert oc.state_defect(jo.dense_state(bra), ref_state) < 1e-10
    n_o, b_o, it_o = orc.operate(start, mpo, maxstep=maxstep)
    assert it_o == maxstep and oc.state_defect(jo.dense_state(bra), jo.dense_state(b_o)) < 1e-10
    # centre at site 0, sites 1 .. L-1 in gauge B
    for c in bra[1:]:
        m = c.reshape(c.shape[0], -1)
        assert np.abs(m @ m.conj().T - np.eye(c.shape[0])).max() < 1e-13
    assert abs(np.linalg.norm(bra[0]) - 1) < 1e-14


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_the_twin_gives_the_oracle_state_whatever_the_qr_phases(name):
    from helpers import expect_cases as ec
    from helpers import jump_oracle as jo
    from helpers import operate_cases as oc

    worst = 0.0
    for label in oc.LABELS:
        _, shift, mpo = ec.case(name, label)
        for r in range(oc.NSTATES):
            nrm, pin, it = oc.oracle_case(name, label, r)
            n2, bra, it2, status = oc.twin(oc.states(name)[r], mpo, shift, oc.MAXSTEP, 0.0, seed=7 + r)
            assert it2 == it == oc.MAXSTEP and status == 0
            worst = max(worst, oc.state_defect(jo.dense_state(bra), pin) / 1e-10, abs(n2 - nrm) / (1e-10 * nrm))
    print(f"{name}: worst |twin - oracle| = {worst:.3e} of 1e-10")
    assert worst < 1


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_the_bars_have_room(name):
    """a 1e-13 relative perturbation of the inputs moves the oracle's dense result by less than a tenth of the bars, for
    every case the GPU test uses"""
    from helpers import expect_cases as ec
    from helpers import jump_oracle as jo
    from helpers import operate_cases as oc
    from oracle import tdvp_oracle as orc

    rng = np.random.default_rng(11)
    jig = lambda a: a * (1.0 + 1e-13 * rng.standard_normal(a.shape))
    worst = 0.0
    for label in oc.LABELS:
        _, shift, mpo = ec.case(name, label)
        for r in range(oc.NSTATES):
            nrm, pin, _ = oc.oracle_case(name, label, r)
            n2, bra, _ = orc.operate([jig(c) for c in oc.states(name)[r]], [jig(w) for w in mpo], maxstep=oc.MAXSTEP, conv_tol=0.0,
                                     shift=shift)
            worst = max(worst, oc.state_defect(jo.dense_state(bra), pin) / (0.1 * oc.BAR_STATE), abs(n2 - nrm) / (0.1 * oc.BAR_NORM * nrm))
    print(f"{name}: a 1e-13 perturbation moves the oracle by {worst:.3e} of a tenth of the bars")
    assert worst < 1


def test_the_golden_case_is_well_conditioned_too():
    from helpers import jump_oracle as jo
    from helpers import operate_cases as oc
    from oracle import tdvp_oracle as orc

    rng = np.random.default_rng(12)
    jig = lambda a: a * (1.0 + 1e-13 * rng.standard_normal(a.shape))
    mpo, start, res = oc.golden()
    for ns in (1, 10):
        n2, bra, _ = orc.operate([jig(c) for c in start], [jig(w) for w in mpo], maxstep=ns)
        assert oc.state_defect(jo.dense_state(bra), res[ns][1]) < 0.1 * oc.BAR_STATE
        assert abs(n2 - res[ns][0]) < 0.1 * oc.BAR_NORM * res[ns][0]


def test_the_iteration_count_cases_have_a_gap():
    """the oracle's defect is at least a factor 2 above conv_tol at the last sweep that does not stop and at least a factor
    2 below it at the sweep that stops: a last-bit difference of the device does not move the count"""
    from helpers import operate_cases as oc
    from oracle import tdvp_oracle as orc

    for key, (cores, mpo, shift, tol, stop) in oc.stop_cases().items():
        seq = oc.defects(cores, mpo, shift, stop)
        print(f"{key}: conv_tol {tol:g}, defects " + ", ".join(f"{x:.3e}" for x in seq))
        assert all(x >= 2 * tol for x in seq[:stop - 1]) and seq[stop - 1] <= tol / 2
        assert orc.operate(cores, mpo, maxstep=10, conv_tol=tol, shift=shift)[2] == stop
        assert oc.twin(cores, mpo, shift, 10, tol)[2] == stop


def test_the_twin_stops_an_annihilated_state():
    from helpers import operate_cases as oc

    dims, _ = oc.SHAPES["odd"]
    st = [c.copy() for c in oc.states("odd")[1]]
    st[0][:, 1:, :] = 0.0
    proj = np.zeros((3, 3))
    proj[1, 1] = 1.0
    mpo = [m[None, :, :, None].astype(np.complex128) for m in [proj] + [np.eye(d) for d in dims[1:]]]
    nrm, _, it, status = oc.twin(st, mpo, 0.0, 3, 0.0)
    assert nrm == 0.0 and status == 3 and it == 1


# ---- the Python front end, before any engine exists ----
def test_operate_request_validates_and_creates_nothing():
    from pytdscf_amd.engine import operate_request

    assert operate_request(4) == (0, 10, 1e-8, None)
    assert operate_request(4, np.int64(2), 3, 0, replicas=[3, np.int32(0)]) == (2, 3, 0.0, [3, 0])
    assert operate_request(4, replicas=2) == (0, 10, 1e-8, [2])
    assert operate_request(4, replicas=range(1, 4, 2))[3] == [1, 3]
    for kw, msg in ((dict(maxstep=0), "maxstep = 0, it must be >= 1"), (dict(maxstep=2.0), "maxstep = 2.0 is not a whole number"),
                    (dict(maxstep=True), "not a whole number"), (dict(maxstep=2**31), "does not fit an int"),
                    (dict(op_id=-1), "op_id = -1 is negative"), (dict(op_id="0"), "op_id = '0' is not a whole number"),
                    (dict(conv_tol=-1e-9), "conv_tol = -1e-09, it must be finite and >= 0"), (dict(conv_tol=float("nan")), "conv_tol = nan"),
                    (dict(conv_tol=float("inf")), "conv_tol = inf"), (dict(conv_tol="1e-8"), "conv_tol = '1e-8' is not a number"),
                    (dict(replicas=[0, 4]), "replica 4 is outside 0 .. 3"), (dict(replicas=[-1]), "replica -1 is outside 0 .. 3"),
                    (dict(replicas=[1, 2, 1]), "replica 1 is listed twice"), (dict(replicas=[]), "replicas is empty"),
                    (dict(replicas=[0.0]), "replica = 0.0 is not a whole number"), (dict(replicas=3.5), "a list of replica indices")):
        with pytest.raises(ValueError, match="operate: .*" + msg.replace("(", "\\(").replace(")", "\\)")):
            operate_request(4, **kw)


def test_batch_operate_refuses_before_a_handle_exists():
    from pytdscf_amd import TDVPBatch

    bt = TDVPBatch.__new__(TDVPBatch)  # no engine, no library call: the request is checked first
    bt.engines, bt._b = [None, None], None
    for kw, msg in ((dict(maxstep=0), "maxstep = 0"), (dict(conv_tol=-1.0), "conv_tol"), (dict(replicas=[2]), "replica 2 is outside 0 .. 1"),
                    (dict(replicas=[1, 1]), "listed twice")):
        with pytest.raises(ValueError, match=msg):
            bt.operate(**kw)
    assert bt._b is None
    bt.engines = []  # nothing for __del__ to close


def test_correlation_function_checks_core_starts_before_any_engine_exists(monkeypatch):
    from helpers import cross_cases as cc
    from helpers import operate_cases as oc
    from pytdscf_amd import trajectories as tr
    from pytdscf_amd import units

    def no_batch(*a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(tr, "TDVPBatch", no_batch)
    m = cc.model()
    good = oc.corr_start()
    kw = dict(maxstep=3, stepsize=cc.DT * units.au_in_fs, A=cc.A_OP, B=cc.B_OP)
    bad = [c.copy() for c in good]
    bad[1] = bad[1][0]  # rank 2
    with pytest.raises(ValueError, match="start 0, site 1: an MPS core is \\(dl, d, dr\\), got an array of rank 2"):
        tr.correlation_function(m, [bad], **kw)
    with pytest.raises(ValueError, match="start 1, site 0: an MPS core is \\(dl, d, dr\\), got an array of rank 1"):
        tr.correlation_function(m, [good, cc.START], **kw)
    wide = [np.zeros((1, 2, 2)), np.zeros((2, 2, 5)), np.zeros((5, 2, 2)), np.zeros((2, 2, 1))]
    with pytest.raises(ValueError, match="start 0: bond 5 between sites 1 and 2 is above 4, what model.m_aux_max = 4 allows there"):
        tr.correlation_function(m, [wide], **kw)
    dbad = [np.zeros((1, 2, 2)), np.zeros((2, 3, 4)), np.zeros((4, 2, 2)), np.zeros((2, 2, 1))]
    with pytest.raises(ValueError, match="start 0, site 1: the core has physical dimension 3, the model's is 2"):
        tr.correlation_function(m, [dbad], **kw)
    misfit = [np.zeros((1, 2, 2)), np.zeros((1, 2, 4)), np.zeros((4, 2, 2)), np.zeros((2, 2, 1))]
    with pytest.raises(ValueError, match="start 0, site 1: the core has the left bond 1, expected 2"):
        tr.correlation_function(m, [misfit], **kw)
    with pytest.raises(ValueError, match="start 0 has 3 cores, the chain has 4 sites"):
        tr.correlation_function(m, [good[:3]], **kw)
    with pytest.raises(ValueError, match="operate: maxstep = 0"):
        tr.correlation_function(m, [good], operate_maxstep=0, **kw)
    with pytest.raises(ValueError, match="operate: conv_tol"):
        tr.correlation_function(m, [good], operate_tol=-1.0, **kw)
    # narrower cores are padded to the model's bonds; Hartree products are not touched by the check
    assert tr.core_starts([cc.START], m.dims, cc.D) is None
    thin = [np.ones((1, 2, 1)) for _ in range(cc.L)]
    padded = tr.core_starts([thin], m.dims, cc.D)[0]
    assert [c.shape for c in padded] == [c.shape for c in good] and all(c[0, :, 0].tolist() == [1, 1] and abs(c).sum() == 2 for c in padded)
    # for Hartree products the MPO wider than the bond is still refused, in the same words
    with pytest.raises(ValueError, match="B has MPO bond .* the state's bond there is .*B psi does not fit"):
        tr.correlation_function(_narrow_model(), [cc.START], maxstep=3, stepsize=1.0, A=cc.A_OP, B=_sum_sx())


def _sum_sx():
    from helpers import cross_mpo_cases as xc

    return xc.b_mpo()


def _narrow_model():
    from helpers import cross_cases as cc
    from helpers import pair_cases as pc
    from pytdscf_amd import Exciton, Model

    return Model([Exciton(nstate=2) for _ in range(cc.L)], operators={"hamiltonian": pc._spin_chain_mpo(cc.L)}, bond_dim=1)


def test_the_oracle_route_of_the_correlated_start_against_dense_expm():
    """delta, the oracle route's own deviation from dense expm: the GPU test holds the device within ten times it"""
    from helpers import operate_cases as oc

    out = {}
    for b_form in ("mpo", "site"):
        o, d = oc.corr_oracle(b_form), oc.corr_dense(b_form)
        assert np.abs(d[-1] - d[0]) > 1e-2 and np.abs(d).min() > 1e-6  # C(t) moves, and is never a zero
        out[b_form] = np.abs(o - d).max()
    print("oracle route vs dense expm: " + ", ".join(f"B {k}: {v:.2e}" for k, v in out.items()))
    assert max(out.values()) < 1e-10
    # the start is correlated: its middle bond carries more than one Schmidt value
    c = oc.corr_start()
    s = np.linalg.svd(np.einsum("ajb,bkc->ajkc", c[0], c[1]).reshape(4, -1), compute_uv=False)
    assert s[1] > 1e-3
