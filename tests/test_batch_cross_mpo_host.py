"""CPU: MPO matrix elements between the replicas of a batch -- the C surface is declared, exported and bound; the walk of
k_batch_cross_mpo, restated in NumPy, equals the dense pin on every (shape, operator, pair of states) inside a tenth of
the bar of the device tests, and no value compared there is a zero against a zero; the host-built ``B psi`` of
correlation_function is the MPO applied to the dense product; its refusals are raised before any engine exists; the plan
and the refusal logic of the library (csrc/batch_cross_mpo_plan.h, compiled with g++ into a throw-away shim); and the
physics case's oracle against dense expm."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["mitdvp_batch_set_cross_mpo", "mitdvp_batch_cross_mpo", "mitdvp_batch_cross_mpo_records"]


def test_cross_mpo_symbols_are_declared_exported_and_refuse_a_null_batch():
    from pytdscf_amd import _lib

    declared = _lib.declared_symbols()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(_lib.__file__), "_lib.py")) as f:
        binding = f.read()
    for n in NAMES:
        assert n in declared and n in header
        assert f'"{n}"' in binding
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    lib = _lib.load()
    assert lib.mitdvp_batch_set_cross_mpo(None, 0, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_set_cross_mpo" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_cross_mpo(None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_cross_mpo:" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_cross_mpo_records(None, None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_cross_mpo_records" in lib.mitdvp_last_error(None)


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_the_twin_equals_the_dense_pin_and_no_value_is_a_zero(name):
    """three random states of norms 0.7, 0.9, 1.1; every operator; every ordered pair (a, b), a = b included.  The defect is
    printed as a fraction of the device tests' bar 1e-12 SCALE |a| |b| and must stay inside a tenth of it; every value is
    above 1e-6 SCALE |a| |b|, so no device comparison is one of two zeros."""
    from helpers import cross_mpo_cases as xc

    states = xc.random_states(name, 3)
    norms = [xc.norm_of(s) for s in states]
    assert np.allclose(norms, [0.7, 0.9, 1.1], atol=1e-12)
    worst = {"same": 0.0, "other": 0.0}
    small = np.inf
    for label in xc.LABELS:
        _, shift, mpo = xc.case(name, label)
        S = xc.scale(name, label)
        for a in range(3):
            for b in range(3):
                pin, twin = xc.dense_value(states[a], states[b], mpo, shift), xc.walk(states[a], states[b], mpo, shift)
                unit = S * norms[a] * norms[b]
                assert abs(pin) <= unit * (1 + 1e-12), (label, a, b, pin, unit)  # SCALE bounds the value: the bar is a relative one
                key = "same" if a == b else "other"
                worst[key] = max(worst[key], abs(twin - pin) / (xc.BAR * unit))
                small = min(small, abs(twin) / (1e-6 * unit))
    print(f"{name}: worst |twin - dense pin| = {worst['same']:.3e} (a = b), {worst['other']:.3e} (a != b) of 1e-12 SCALE |a| |b|; "
          f"smallest |value| = {small:.3e} of 1e-6 SCALE |a| |b|")
    assert max(worst.values()) <= 0.1
    assert small > 1


def test_the_twin_conjugates_and_reduces_to_its_neighbours():
    """(a, b) is the conjugate of (b, a) for the Hermitian operators; a = b is expect_cases.walk's value; an operator of MPO
    bond 1 on one site is cross_cases.walk with that matrix; the shift adds shift times the overlap"""
    from helpers import cross_cases as cc
    from helpers import cross_mpo_cases as xc
    from helpers import expect_cases as ec
    from helpers import spin_bath as sb

    name = "odd"
    dims, _ = xc.SHAPES[name]
    a, b = xc.random_states(name, 2)
    for label in xc.LABELS:
        _, shift, mpo = xc.case(name, label)
        unit = xc.scale(name, label) * xc.norm_of(a) * xc.norm_of(b)
        ab, ba = xc.walk(a, b, mpo, shift), xc.walk(b, a, mpo, shift)
        if label in xc.HERMITIAN:
            assert abs(ab - np.conj(ba)) < 1e-13 * unit
        else:
            assert abs(ab - np.conj(ba)) > 1e-3 * unit
        assert abs(xc.walk(a, a, mpo, shift) - ec.walk(a, mpo, shift)) < 1e-13 * xc.scale(name, label) * xc.norm_of(a) ** 2
        assert abs(xc.walk(a, b, mpo, shift) - xc.walk(a, b, mpo) - shift * cc.walk(a, b)) < 1e-15 * unit
    O = cc.random_op(dims[2], 9)
    one = [np.ascontiguousarray(w, dtype=np.complex128) for w in sb.sop_mpo([(1.0, {2: O})], list(dims))]
    assert max(w.shape[3] for w in one) == 1
    assert abs(xc.walk(a, b, one) - cc.walk(a, b, 2, O)) < 1e-13 * np.linalg.norm(O, 2) * xc.norm_of(a) * xc.norm_of(b)


def test_host_built_b_psi_is_the_mpo_on_the_dense_product():
    """phi_p[c, i, t] = sum_j W_p[c, i, j, t] v_p[j] against apply_mpo on the dense product, 1e-14 relative: bare, and padded
    to the bond dimensions and brought to the canonical form as the front end sets it"""
    import functools

    from helpers import cross_cases as cc
    from helpers import cross_mpo_cases as xc
    from helpers import expect_cases as ec
    from helpers import jump_oracle as jo
    from pytdscf_amd.trajectories import mpo_on_product

    psi0 = functools.reduce(np.kron, cc.start_vectors())
    for mpo in (xc.b_mpo(), xc.a_mpo()):
        want = ec.apply_mpo(mpo, psi0)
        bare = mpo_on_product(mpo, cc.START)  # the raw vectors: normalised inside
        assert [c.shape for c in bare] == [(w.shape[0], w.shape[1], w.shape[3]) for w in mpo]
        assert np.abs(jo.dense_state(bare) - want).max() <= 1e-14 * np.abs(want).max()
        padded = xc.phi_cores(mpo)
        assert np.abs(jo.dense_state(padded) - want).max() <= 1e-14 * np.abs(want).max() * 10  # the QR sweep's roundings
        assert abs(xc.norm_of(padded) - np.linalg.norm(want)) <= 1e-14 * np.linalg.norm(want)
    # a ragged chain with a non-Hermitian operator of bond 3 .. 5
    name = "mixed"
    dims, _ = xc.SHAPES[name]
    rng = np.random.default_rng(3)
    vecs = [rng.standard_normal(d) + 1j * rng.standard_normal(d) for d in dims]
    mpo = xc.case(name, "complex")[2]
    want = ec.apply_mpo(mpo, functools.reduce(np.kron, [v / np.linalg.norm(v) for v in vecs]))
    assert np.abs(jo.dense_state(mpo_on_product(mpo, vecs)) - want).max() <= 1e-14 * np.abs(want).max()


def test_correlation_function_refuses_before_any_engine_exists(monkeypatch):
    from helpers import cross_cases as cc
    from helpers import cross_mpo_cases as xc
    from helpers import spin_bath as sb
    import pytdscf_amd.trajectories as tr

    def _no_batch(*a, **k):
        raise AssertionError("a batch was constructed")

    monkeypatch.setattr(tr, "TDVPBatch", _no_batch)
    m = xc.model()
    kw = dict(maxstep=3, stepsize=0.1)
    with pytest.raises(ValueError, match=r"A = 'dipole' is not in model.observables \(it has \['sx_total', 'sz_total'\]\)"):
        tr.correlation_function(m, [cc.START], A="dipole", B="sx_total", **kw)
    with pytest.raises(ValueError, match=r"B = 'current' is not in model.observables"):
        tr.correlation_function(m, [cc.START], A=cc.A_OP, B="current", **kw)
    # an MPO of bond 3 between sites 0 and 1, where a chain of d = 2 has a bond of 2
    wide = [np.ascontiguousarray(w) for w in sb.sop_mpo([(1.0, {0: sb.SX, 1: sb.SX}), (1.0, {0: sb.SY, 1: sb.SY}), (1.0, {0: sb.SZ, 1: sb.SZ})],
                                                         [2] * cc.L)]
    assert wide[0].shape[3] == 3
    with pytest.raises(ValueError, match=r"B has MPO bond 3 between sites 0 and 1, the state's bond there is 2"):
        tr.correlation_function(m, [cc.START], A="sz_total", B=wide, **kw)
    # a start that B annihilates: every site in the kernel of the lowering operator
    low = np.array([[0, 1], [0, 0]], dtype=complex)
    lower = sb.sop_mpo([(1.0, {p: low}) for p in range(cc.L)], [2] * cc.L)
    with pytest.raises(ValueError, match="B annihilates start 1"):
        tr.correlation_function(m, [cc.START, [[1, 0]] * cc.L], A="sz_total", B=lower, **kw)
    with pytest.raises(ValueError, match=r"A has 3 MPO cores, the chain has 4 sites"):
        tr.correlation_function(m, [cc.START], A=xc.a_mpo()[:3], B="sx_total", **kw)
    with pytest.raises(ValueError, match=r"A: the MPO core of site 1 has shape"):
        tr.correlation_function(m, [cc.START], A=[xc.a_mpo()[0]] * 4, B="sx_total", **kw)
    with pytest.raises(ValueError, match="A acts on site 7"):
        tr.correlation_function(m, [cc.START], A=(7, sb.SZ), B="sx_total", **kw)
    with pytest.raises(ValueError, match="give both A and B"):
        tr.correlation_function(m, [cc.START], A="sz_total", **kw)
    # and the forms are told apart as stated
    assert tr._operator_form("A", cc.A_OP, m, m.dims)[0] == "site"
    assert tr._operator_form("A", "sz_total", m, m.dims)[0] == "mpo" and tr._operator_form("B", xc.b_mpo(), m, m.dims)[0] == "mpo"


def test_set_cross_mpo_entries_on_the_python_side():
    from pytdscf_amd import TDVPBatch

    bt = TDVPBatch.__new__(TDVPBatch)  # no engine, no library call: the checks in front of them
    bt._cross_mpo = None
    for bad in ([(0, 1)], [(0, 1, 2, 3)], [(0, 1, 0.5)], [(0, "1", 0)], [(0, 1, 2**40)]):
        with pytest.raises(ValueError, match="set_cross_mpo: entry 0"):
            bt.set_cross_mpo(bad)
    with pytest.raises(ValueError, match="no cross request of MPOs is set"):
        bt._request_weights("cross_mpo", "entry", None)
    bt._cross_mpo = ([0, 1], [1, 0], [1, 1])
    with pytest.raises(ValueError, match="cross_mpo weights must be 2 numbers, one per entry"):
        bt._request_weights("cross_mpo", "entry", [1.0])
    bt._b = None  # what __del__ looks at
    bt.engines, bt._own = [], False


# ---- the plan and the refusal logic of the library, through a g++ shim ----
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("xm_shim") / "libxm_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "helpers", "cross_mpo_plan_shim.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    lib.xm_plan.restype = lib.xm_fits.restype = lib.xm_entries.restype = C.c_char_p
    lib.xm_max_bytes.restype = C.c_ulonglong
    lib.xm_fits.argtypes = [C.c_ulonglong, C.c_ulonglong]
    return lib


def _plan(shim, shapes, op_ids):
    """shapes: [nops][L] of (dl, d, dr, ml, mr) -> (message or None, (o_e1, o_x, o_y, total))"""
    arr = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32))
    nops, L = arr.shape[:2]
    out = (C.c_ulonglong * 4)()
    ids = (C.c_int * nops)(*op_ids)
    msg = shim.xm_plan(arr.ctypes.data_as(C.POINTER(C.c_int)), ids, L, nops, out)
    return (msg.decode() if msg else None), tuple(int(x) for x in out)


def _shapes(dims, D, mpo):
    from pytdscf_amd.mps import bond_dims

    return [(dl, d, dr, w.shape[0], w.shape[3]) for (dl, dr), d, w in zip(bond_dims(list(dims), D), dims, mpo)]


def test_the_plan_sizes_the_carve_from_the_shapes(shim):
    from helpers import cross_mpo_cases as xc

    assert shim.xm_max_mpo() == 16 and shim.xm_max_entries() == 65536 and shim.xm_max_bytes() == 1 << 32
    assert shim.xm_sizeof_entry() == 16
    # the figure of the design: d = 4, D = 32, M = 16 in the middle of a long chain, about 2.6 MB a carve
    L = 10
    big = [[(1 if p == 0 else 32 if p > 2 else 4 ** p, 4, 1 if p == L - 1 else 32 if p < L - 3 else 4 ** (L - 1 - p),
             1 if p == 0 else 16, 1 if p == L - 1 else 16) for p in range(L)]]
    msg, (o_e1, o_x, o_y, total) = _plan(shim, big, [0])
    assert msg is None
    assert (o_e1, o_x - o_e1, o_y - o_x, total - o_y) == (32 * 16 * 32, 32 * 16 * 32, 4096 * 16, 4096 * 16)
    assert total * 16 == 2621440
    # every test shape and operator, alone and together: the carve is the largest block twice, the largest X and the largest Y
    for name, (dims, D) in xc.SHAPES.items():
        rows = [_shapes(dims, D, xc.case(name, label)[2]) for label in xc.LABELS]
        msg, (o_e1, o_x, o_y, total) = _plan(shim, rows, [xc.OP_ID[x] for x in xc.LABELS])
        assert msg is None
        flat = [s for row in rows for s in row]
        ne = max(dr * mr * dr for dl, d, dr, ml, mr in flat)
        nx = max(dl * d * dr * ml for dl, d, dr, ml, mr in flat)
        ny = max(dl * d * dr * mr for dl, d, dr, ml, mr in flat)
        assert (o_e1, o_x, o_y) == (ne, 2 * ne, 2 * ne + nx) and total == -(-(2 * ne + nx + ny) // 16) * 16
        # the overlap walk of the scalar term fits the same carve: its T in a block, its U in X
        assert ne >= max(max(dl * dl, dr * dr) for dl, d, dr, ml, mr in flat) and nx >= max(dl * d * dr for dl, d, dr, ml, mr in flat)
        alone = _plan(shim, rows[:1], [1])[1]
        assert alone[3] <= total


def test_the_plan_refuses_what_the_expect_plan_refuses(shim):
    ok = [(1, 2, 2, 1, 3), (2, 2, 2, 3, 3), (2, 2, 1, 3, 1)]
    assert _plan(shim, [ok], [5])[0] is None
    bad = [([(1, 2, 2, 1, 17), (2, 2, 2, 17, 3), ok[2]], r"operator 5, site 0: MPO bonds (1, 17): the batched kernel takes MPO bonds of 1 to 16"),
           ([(1, 2, 2, 1, 0), (2, 2, 2, 0, 3), ok[2]], r"operator 5, site 0: MPO bonds (1, 0): the batched kernel takes MPO bonds of 1 to 16"),
           ([ok[0], (2, 2, 2, 4, 3), ok[2]], r"operator 5, site 0: MPO bonds (1, 3): the core of site 1 has the left MPO bond 4"),
           ([(1, 2, 2, 2, 3), ok[1], ok[2]], r"operator 5: the outer MPO bonds are (2, 1), they must be 1"),
           ([ok[0], ok[1], (2, 2, 1, 3, 2)], r"operator 5: the outer MPO bonds are (1, 2), they must be 1")]
    for shapes, want in bad:
        msg, _ = _plan(shim, [ok, shapes], [4, 5])
        assert msg == want, msg


def test_the_buffer_cap_names_the_figure_and_what_fits(shim):
    carve = 163840  # d = 4, D = 32, M = 16: 2 621 440 bytes
    fit = (1 << 32) // (carve * 16)
    assert fit == 1638
    assert shim.xm_fits(fit, carve) is None and shim.xm_fits(1, carve) is None
    msg = shim.xm_fits(fit + 1, carve).decode()
    assert msg == (f"{fit + 1} entries of 2621440 bytes each need a buffer of {(fit + 1) * 2621440} bytes, the limit is 4294967296 bytes: "
                   f"at most {fit} entries fit")
    assert shim.xm_fits(65536, 4096) is None  # exactly 2^32 bytes
    assert b"at most 65280 entries fit" in shim.xm_fits(65536, 4112)  # (1 << 32) // (4112 * 16)


def test_the_entries_are_checked_as_the_cross_request_checks_its_pairs(shim):
    ia = lambda v: (C.c_int * max(len(v), 1))(*v)

    def check(B, snap, bra, ket, op):
        msg = shim.xm_entries(B, int(snap), len(bra), ia(bra), ia(ket), ia(op))
        return msg.decode() if msg else None

    assert check(3, False, [0, 2, 1], [1, 2, 0], [0, 7, 7]) is None
    assert check(3, True, [3, 5], [0, 4], [0, 0]) is None
    assert check(3, False, [], [], []) is None
    assert check(3, False, [0, 6], [1, 0], [0, 0]) == ("entry 1: bra index 6 is outside 0 .. 5 (the batch has 3 replicas; 3 + r names the snapshot "
                                                        "of replica r)")
    assert check(3, True, [0], [-1], [0]).startswith("entry 0: ket index -1 is outside 0 .. 5")
    assert check(3, False, [0, 1], [1, 4], [0, 0]) == ("entry 1: ket index 4 names the snapshot of replica 1, and no snapshot was taken yet "
                                                        "(mitdvp_batch_snapshot)")
    assert check(3, False, [0, 1], [1, 2], [0, -2]) == "entry 1: operator -2 is negative (operator ids are >= 0)"
    n = 65537
    assert check(3, False, [0] * n, [1] * n, [0] * n) == "65537 entries, a request takes at most 65536"
    assert check(3, False, [0] * 65536, [1] * 65536, [0] * 65536) is None
    assert shim.xm_entries(3, 0, -1, None, None, None) == b"nentries must be >= 0"
    assert shim.xm_entries(3, 0, 2, None, None, None) == b"null list of bra, ket or operator indices"


# ---- the physics case ----
def test_the_oracle_follows_dense_expm_on_the_physics_case():
    """C(t) = <psi| A(t) B |psi> with A = sum_p SZ_p, B = sum_p SX_p on cross_cases' L = 4, D = 4 chain: OracleMPS runs of psi
    and phi = B psi, then the twin, against dense expm.  The deviation is printed (it is recorded in the helper's docstring);
    the GPU test holds the device within ten times the deviation it computes from the same two references.  The mixed forms
    too: A one-site with B an MPO, A an MPO with B one-site."""
    from helpers import cross_cases as cc
    from helpers import cross_mpo_cases as xc

    out = {}
    for forms in (("mpo", "mpo"), ("site", "mpo"), ("mpo", "site")):
        oc, de = xc.oracle_corr(*forms), xc.dense_corr(*forms)
        assert oc.shape == de.shape == (cc.NSTEPS + 1,)
        assert np.abs(de[-1] - de[0]) > 1e-2 and np.abs(de).min() > 1e-6  # C(t) moves, and is never a zero
        out[forms] = np.abs(oc - de).max()
    print("oracle vs dense expm: " + ", ".join(f"A {a} / B {b}: {v:.2e}" for (a, b), v in out.items()))
    assert max(out.values()) < 1e-10
    # at t = 0 the value is <psi| A B |psi> of the dense product
    import functools

    from helpers import jump_oracle as jo

    psi0 = functools.reduce(np.kron, cc.start_vectors())
    want = np.vdot(psi0, jo.dense_operator(xc.a_mpo()) @ (jo.dense_operator(xc.b_mpo()) @ psi0))
    assert abs(xc.oracle_corr()[0] - want) < 1e-14
