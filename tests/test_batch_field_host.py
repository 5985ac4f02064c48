"""CPU: time-dependent one-site fields of the batched trajectories -- the C surface is declared, exported and mirrored;
the pure-Python refusals; the noise generator restated in Python and its statistics; the in-place step equals the gate
walk it replaces; the splitting is of second order against the dense time-ordered evolution."""

import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

NAMES = ["mitdvp_batch_set_field", "mitdvp_batch_field_values"]


def test_field_symbols_are_declared_exported_and_mirrored():
    from pytdscf_amd import _lib

    declared = _lib.declared_symbols()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(_lib.__file__), "_lib.py")) as f:
        binding = f.read()
    for n in NAMES:
        assert n in declared and n in header
        assert f'"{n}"' in binding
    assert "#define MITDVP_FIELD_TABLE 1" in header and "#define MITDVP_FIELD_OU 2" in header
    assert (_lib.FIELD_TABLE, _lib.FIELD_OU, _lib.MAX_FIELD_D) == (1, 2, 64)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    lib = _lib.load()  # the signatures load
    assert lib.mitdvp_batch_set_field.argtypes is not None and len(lib.mitdvp_batch_set_field.argtypes) == 11
    assert len(lib.mitdvp_batch_field_values.argtypes) == 2


def test_null_handle_is_refused_with_the_entry_point_named():
    from pytdscf_amd import _lib

    lib = _lib.load()
    g = np.zeros(2)
    V = np.eye(2, dtype=np.complex128)
    dp = C.POINTER(C.c_double)
    assert lib.mitdvp_batch_set_field(None, 0, 2, V.ctypes.data_as(dp), g.ctypes.data_as(dp), _lib.FIELD_OU, None, 0, 0, 1.0, 1.0) == _lib.EINVAL
    assert lib.mitdvp_last_error(None).decode() == "mitdvp_batch_set_field: null handle"
    out = np.zeros(4)
    assert lib.mitdvp_batch_field_values(None, out.ctypes.data_as(dp)) == _lib.EINVAL
    assert lib.mitdvp_last_error(None).decode() == "mitdvp_batch_field_values: null handle"


SX = np.array([[0, 1], [1, 0]], dtype=complex)


def test_field_request_refuses_in_pure_python():
    from pytdscf_amd import _lib
    from pytdscf_amd.engine import field_request

    dims, B = [2, 3, 2], 4
    G3 = np.diag([1.0, 0.0, -1.0])

    def refused(fields, match):
        with pytest.raises(ValueError, match=match):
            field_request(fields, dims, B)

    refused({3: dict(G=SX, pulse=[1.0])}, "site 3 is out of range")
    refused({-1: dict(G=SX, pulse=[1.0])}, "out of range")
    refused({0: dict(G=np.ones((2, 3)), pulse=[1.0])}, r"fields\[0\].*square")
    refused({0: dict(G=np.array([[0, 1], [0, 0]]), pulse=[1.0])}, r"fields\[0\].*not Hermitian")
    refused({0: dict(G=SX + 1e-9j * np.eye(2), pulse=[1.0])}, "not Hermitian")
    refused({1: dict(G=SX, pulse=[1.0])}, r"fields\[1\].*order 2.*dimension is 3")
    refused({0: dict(G=SX, pulse=[1.0], sigma=0.5, tau=1.0)}, "not both")
    refused({0: dict(G=SX)}, "one of them")
    refused({0: dict(G=SX, pulse=np.zeros((3, 5)))}, r"\(n,\) or \(4, n\)")
    refused({0: dict(G=SX, pulse=np.zeros(0))}, "n >= 1")
    refused({0: dict(G=SX, pulse=[1.0, np.nan])}, "finite")
    refused({0: dict(G=SX, pulse=[1.0j])}, "real")
    refused({0: dict(G=SX, sigma=-1.0, tau=1.0)}, "finite and >= 0")
    refused({0: dict(G=SX, sigma=1.0, tau=np.inf)}, "finite and >= 0")
    refused({0: dict(G=SX, pulse=[1.0], width=3)}, "unknown key 'width'")
    refused({0: SX}, "must be dict")

    assert field_request(None, dims, B) == {} and field_request({}, dims, B) == {}
    out = field_request({0: dict(G=SX, pulse=[0.5, 0.25]), 1: dict(G=G3, sigma=0.5, tau=2.0), 2: dict(G=SX, pulse=np.ones((4, 3)))}, dims, B)
    V, g, kind, tab, sigma, tau = out[0]
    assert kind == _lib.FIELD_TABLE and tab.shape == (2,) and tab.dtype == np.float64
    assert np.abs((V * g) @ V.conj().T - SX).max() < 1e-15 and np.all(np.diff(g) >= 0)  # numpy.linalg.eigh
    assert out[1][2:] == (_lib.FIELD_OU, None, 0.5, 2.0)
    assert out[2][3].shape == (4, 3) and out[2][3].flags.c_contiguous


class _Stop(Exception):
    pass


def test_the_drivers_refuse_before_any_engine_is_created(monkeypatch):
    from helpers import spin_bath as sb
    from pytdscf_amd import Exciton, Model
    from pytdscf_amd import trajectories as tr

    def no_engine(*a, **k):
        raise _Stop("an engine was created")

    monkeypatch.setattr(tr, "TDVPBatch", no_engine)
    case = sb.case_trajectories()
    m = Model([Exciton(nstate=d) for d in case["dims"]], operators={"hamiltonian": case["mpo"]}, bond_dim=64)
    args = dict(maxstep=3, stepsize=0.1, reduced_density=([(1, 1)], 1))
    with pytest.raises(ValueError, match=r"fields\[1\].*order 2.*dimension is 3"):
        tr.propagate_trajectories(m, case["starts"], fields={1: dict(G=SX, pulse=[1.0])}, **args)
    with pytest.raises(ValueError, match="not both"):
        tr.propagate_trajectories(m, case["starts"], fields={0: dict(G=SX, pulse=lambda t: 1.0, sigma=1.0)}, **args)
    with pytest.raises(ValueError, match=r"\(n,\) or \(4, n\)"):
        tr.propagate_trajectories(m, case["starts"], fields={0: dict(G=SX, pulse=np.zeros((3, 2)))}, **args)
    with pytest.raises(ValueError, match="not Hermitian"):
        tr.correlation_function(m, case["starts"], 3, 0.1, fields={0: dict(G=np.array([[0, 1], [0, 0]]), sigma=1.0, tau=1.0)})
    # a run that is accepted reaches the engine: a callable pulse, and noise
    with pytest.raises(_Stop):
        tr.propagate_trajectories(m, case["starts"], fields={0: dict(G=SX, pulse=lambda t: math.sin(t))}, **args)
    with pytest.raises(_Stop):
        tr.correlation_function(m, case["starts"], 3, 0.1, fields={2: dict(G=SX, sigma=0.3, tau=0.0)})


def test_field_normal_and_pulse_table_are_their_definitions():
    from pytdscf_amd.trajectories import field_noise_path, field_normal, jump_uniform, pulse_table

    for seed, tid, step, site, nsite in [(0, 0, 0, 0, 1), (7, 3, 2, 1, 2), (2**64 - 1, 2**63, 10**6, 4, 5), (12345, 2047, 3, 0, 9)]:
        u1 = jump_uniform(seed, tid, step, 2 * nsite + 2 * site)
        u2 = jump_uniform(seed, tid, step, 2 * nsite + 2 * site + 1)
        z = math.sqrt(-2.0 * math.log1p(-u1)) * math.cos(2.0 * math.pi * u2)
        assert field_normal(seed, tid, step, site, nsite) == z, (seed, tid, step, site, nsite)
    # the keys of the noise lie above the one-site jump keys 0 .. L-1 and the pair keys L .. 2L-2
    L = 5
    assert min(2 * L + 2 * p for p in range(L)) > 2 * L - 2
    # the recursion, white noise, and the first step of the batch's counter
    dts = [0.1, 0.1, 0.2, 0.05]
    z = [field_normal(9, 4, 10 + n, 1, 3) for n in range(4)]
    path = field_noise_path(9, 4, 1, 3, 0.8, 0.25, dts, first_step=10)
    want = [0.8 * z[0]]
    for n in range(1, 4):
        a = math.exp(-dts[n] / 0.25)
        want.append(a * want[-1] + 0.8 * math.sqrt(1 - a * a) * z[n])
    assert np.array_equal(path, np.array(want))
    assert np.array_equal(field_noise_path(9, 4, 1, 3, 0.8, 0.0, dts, first_step=10), 0.8 * np.array(z))

    tab = pulse_table(lambda t: 3.0 * t, 0.5, 4, t0=1.0)
    assert np.array_equal(tab, 3.0 * (1.0 + (np.arange(4) + 0.5) * 0.5)) and tab.dtype == np.float64
    with pytest.raises(ValueError):
        pulse_table(lambda t: t, 0.5, 0)


def test_noise_statistics():
    """Seed 7, trajectories 0 .. 4095, L = 2, sigma = 0.8, tau = 0.25, dt = 0.1, 8 steps: every per-step mean, variance,
    lag-1 covariance (against a sigma^2) and the cross-site covariance within 4 standard errors -- sigma / sqrt(N) for a
    mean, sigma^2 sqrt(2 / (N - 1)) for a variance, sigma^2 sqrt((1 + a^2) / N) for the lag-1 covariance and sigma^2 /
    sqrt(N) for the cross-site covariance of two independent Gaussians.  The worst of the 46 figures is 1.7."""
    from pytdscf_amd.trajectories import field_noise_path

    N, L, sigma, tau, dt, nsteps = 4096, 2, 0.8, 0.25, 0.1, 8
    x = np.array([[field_noise_path(7, t, p, L, sigma, tau, [dt] * nsteps) for p in range(L)] for t in range(N)])  # (N, L, n)
    a, s2 = math.exp(-dt / tau), sigma * sigma
    worst = 0.0
    for p in range(L):
        for n in range(nsteps):
            worst = max(worst, abs(x[:, p, n].mean()) / (sigma / math.sqrt(N)))
            worst = max(worst, abs(x[:, p, n].var(ddof=1) - s2) / (s2 * math.sqrt(2.0 / (N - 1))))
        for n in range(1, nsteps):
            worst = max(worst, abs(np.mean(x[:, p, n] * x[:, p, n - 1]) - a * s2) / (s2 * math.sqrt((1 + a * a) / N)))
    for n in range(nsteps):
        worst = max(worst, abs(np.mean(x[:, 0, n] * x[:, 1, n])) / (s2 / math.sqrt(N)))
    print(f"worst deviation {worst:.2f} standard errors")
    assert worst < 4.0


@functools.lru_cache(maxsize=None)
def _case(D):
    from helpers import field_oracle as fo

    return fo.driven_chain(D=D)


@pytest.mark.parametrize("D", [4, 2])
def test_in_place_step_equals_the_gate_walk(D):
    """the L = 4 driven chain, 4 steps of 0.05 around the pulse's rise: unitaries in place + rebuilt left blocks against
    the same unitaries as gates of jump_oracle's walk; D = 2 truncates"""
    from helpers import field_oracle as fo
    from helpers import jump_oracle as jo
    from oracle import tdvp_oracle as orc

    case = _case(D)
    a = fo.run_numpy(case, 0.05, 4, step=fo.field_step)
    b = fo.run_numpy(case, 0.05, 4, step=fo.walk_step)
    diff = np.abs(jo.dense_state(a.cores) - jo.dense_state(b.cores)).max()
    print(f"D = {D}: max |in place - walk| = {diff:.2e}")
    assert diff < 1e-12
    # the site tensors stay isometries without a gauge move: after one forward half-sweep and the unitaries, gauge A
    st = orc.OracleMPS([c.copy() for c in case["start"]], case["mpo"], integrator="arnoldi", conserve_norm=False, thresh=1e-13)
    st.build_right_envs()
    st.sweep(0.05, True)
    fo.apply_fields_in_place(st, 0.05, [0.7] * 4, case["fields"])
    for p in range(3):
        c = st.cores[p]
        assert np.abs(np.einsum("ajs,ajt->st", c.conj(), c) - np.eye(c.shape[2])).max() < 1e-13
        assert np.abs(st.left[p + 1] - orc.env_update_left(st.left[p], c, st.mpo[p])).max() == 0
    assert abs(np.sqrt(abs(orc.overlap(a.cores, a.cores))) - 1) < 1e-12


def test_second_order_against_the_time_ordered_evolution():
    """error of the state at T = 1 against the dense time-ordered evolution at dt = 0.05, 0.025, 0.0125: a factor between
    3.5 and 4.5 per halving (D = 4 is the chain's full bond, so one-site TDVP of H0 alone is exact and the error is the
    splitting's)"""
    from helpers import field_oracle as fo
    from helpers import jump_oracle as jo

    case = _case(4)
    exact = fo.dense_time_ordered(jo.dense_state(case["start"]), case["H0"], fo.pulse, case["G"], 0.0, fo.T_END)
    errs = []
    for dt in (0.05, 0.025, 0.0125):
        st = fo.run_numpy(case, dt, round(fo.T_END / dt))
        errs.append(np.linalg.norm(jo.dense_state(st.cores) - exact))
    ratios = [errs[i] / errs[i + 1] for i in range(2)]
    print(f"errors {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e}, ratios {ratios[0]:.3f} {ratios[1]:.3f}")
    assert all(3.5 < r < 4.5 for r in ratios)
