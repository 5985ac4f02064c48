"""GPU: the records of the five batch requests -- cross, spectra, samples, expect, cross_mpo -- live in one store
(csrc/engine_batch.h, RecordStore, laid out by csrc/batch_records.h), and each request keeps the promises of that store:
a call on the current state after a recorded run writes the slot behind the run's records and loses none of them or of
their means; means under weights given later are formed from the records on the device, into a region of their own, so
the run's own means are still there afterwards; and the call on the state the run ended in is bitwise the run's last
record.

The shape is the smallest of the spectra tests, "mixed": dims (2, 3, 2, 4, 2), D = 6, B = 3 replicas of norms 0.7, 0.9,
1.1 that carry the five operators of helpers/expect_cases; cross and cross_mpo are given four entries, so that their
number of rows is not the number of replicas.  The means under given weights are compared with ``w @ R`` formed on the
host to 1e-13 max|R|, the bar of test_a_recorded_run in tests/test_gpu_batch_spectra.py: at most four terms of size
max|R| are summed, each rounded once."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAME = "mixed"
DT = 0.2
B = 3
REQUESTS = ("cross", "spectra", "samples", "expect", "cross_mpo")


def _batch():
    """three replicas carrying the five operators, a snapshot of the start and one step behind it"""
    from helpers import cross_mpo_cases as xc
    from pytdscf_amd import TDVPBatch

    dims, _ = xc.SHAPES[NAME]
    bt = TDVPBatch(B, len(dims), integrator="arnoldi", conserve_norm=False)
    for e, cores in zip(bt.engines, xc.random_states(NAME, B)):
        for label in xc.LABELS:
            _, shift, mpo = xc.case(NAME, label)
            e.set_mpo(mpo, xc.OP_ID[label], shift=shift)
        e.set_mps(cores)
    bt.snapshot()
    bt.propagate(DT, 1)
    return bt


def _cat(parts):
    return np.concatenate([np.asarray(p) for p in parts], axis=-1)


def _set(bt, request):
    """sets the request; returns the number of weights it takes"""
    from helpers import cross_cases as cc
    from helpers import cross_mpo_cases as xc

    dims, _ = xc.SHAPES[NAME]
    s = bt.snap
    if request == "cross":
        bt.set_cross([(0, 1), (2, s(1), 3, cc.random_op(dims[3], 14)), (s(0), 0), (1, 2, 1, cc.random_op(dims[1], 12))])
        return 4
    if request == "spectra":
        bt.set_spectra([0, 2, 3])
    if request == "samples":
        bt.set_samples(5, seed=3)
    if request == "expect":
        bt.set_expect([xc.OP_ID[x] for x in xc.LABELS])
    if request == "cross_mpo":
        bt.set_cross_mpo([(0, 1, xc.OP_ID["local"]), (2, s(1), xc.OP_ID["complex"]), (s(0), 0, xc.OP_ID["energy"]),
                          (1, 1, xc.OP_ID["longrange"])])
        return 4
    return B


def _flat_spectra(d):
    """the entries of spectra() / _spectra_records as (values [.., B, len], mean [.., len])"""
    names = ("norm2", "entropy", "renyi2", "min_weight")
    return _cat([d[k] for k in names] + d["weights"]), _cat([d["mean_" + k] for k in names] + d["mean_weights"])


def _records(bt, request, w):
    """X_records under the weights w (None: the run's own means): the averaged values [nrec, rows, len], their means
    [nrec, len], and what else the request records per row"""
    if request in ("cross", "cross_mpo"):
        vals, mean = (bt._cross_records if request == "cross" else bt._cross_mpo_records)(w)
        return vals[:, :, None], mean[:, None], []
    if request == "spectra":
        return _flat_spectra(bt._spectra_records(w)) + ([],)
    if request == "samples":
        d = bt._samples_records(w)
        return _cat(d["freq"]), _cat(d["mean_freq"]), [d["configs"], d["prob"]]
    d = bt._expect_records(w)
    return d["expect"], d["mean_expect"], []


def _now(bt, request):
    """X() on the current state: the values [rows, len] and what else the request gives per row"""
    if request in ("cross", "cross_mpo"):
        return (bt.cross() if request == "cross" else bt.cross_mpo())["values"][:, None], []
    if request == "spectra":
        return _flat_spectra(bt.spectra())[0], []
    if request == "samples":
        d = bt.samples()
        return _cat(d["freq"]), [d["configs"], d["prob"]]
    return bt.expect()["values"], []


@pytest.mark.parametrize("request_name", REQUESTS)
def test_a_call_and_new_weights_leave_the_records_of_the_run_as_they_are(request_name):
    bt = _batch()
    nw = _set(bt, request_name)
    bt.propagate(DT, 2, observe={request_name: True}, every=1)
    R, M, more = _records(bt, request_name, None)
    assert R.shape[:2] == (3, nw) and M.shape == (3, R.shape[2]) and np.abs(R).max() > 0
    assert all(x.shape[:2] == (3, B) for x in more)

    now, more_now = _now(bt, request_name)  # writes the slot behind the three records

    R1, M1, more1 = _records(bt, request_name, None)
    assert np.array_equal(R1, R) and np.array_equal(M1, M)
    assert all(np.array_equal(a, b) for a, b in zip(more1, more))

    w = np.array([0.5, 0.2, 0.3]) if nw == B else np.array([0.4, 0.1, 0.3, 0.2])
    R2, M2, more2 = _records(bt, request_name, w)
    assert np.array_equal(R2, R) and all(np.array_equal(a, b) for a, b in zip(more2, more))
    ref = np.einsum("r,qre->qe", w, R)
    defect = np.abs(M2 - ref).max() / (1e-13 * np.abs(R).max())
    print(f"{request_name}: |means under given weights - w @ R| = {defect:.3e} of the bar 1e-13 max|R|; "
          f"|they - the run's means| = {np.abs(M2 - M).max() / np.abs(R).max():.3e} max|R|")
    assert np.abs(M2 - M).max() > 1e-6 * np.abs(R).max()  # the weights are not the default: another answer was formed
    assert defect < 1

    R3, M3, _ = _records(bt, request_name, None)  # the re-weighted means went to a region of their own
    assert np.array_equal(M3, M) and np.array_equal(R3, R)

    assert np.array_equal(now, R[-1])  # the run ended in this state: the call is its last record, bit for bit
    assert all(np.array_equal(a, b[-1]) for a, b in zip(more_now, more))
    bt.close()
