"""CPU: where the records of a batch request and their means lie (csrc/batch_records.h, compiled with g++ into a
throw-away shim): for every (rows, len, nrec) with rows in 1..3, len in 1..4 and nrec in 0..3 the nrec + 1 record slots
tile the record buffer, the three regions of the mean buffer are disjoint, in order and end at the stated size, and the
sizes are the products the host code wrote out per request before the layout had a place of its own."""

import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = list(itertools.product(range(1, 4), range(1, 5), range(0, 4)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("br_shim") / "libbr_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "helpers", "batch_records_shim.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    ull = C.c_ulonglong
    lib.br_layout.argtypes = [ull, ull, ull, C.POINTER(ull)]
    lib.br_layout.restype = None
    lib.br_rec_slot.argtypes = [ull, ull, ull, ull]
    lib.br_rec_slot.restype = ull
    return lib


def _layout(shim, rows, length, nrec):
    out = (C.c_ulonglong * 7)()
    shim.br_layout(rows, length, nrec, out)
    names = ("rec_elems", "slot_elems", "rec_now", "mean_elems", "mean_run", "mean_now", "mean_reweighted")
    return dict(zip(names, (int(x) for x in out)))


def test_the_cases_are_the_whole_grid():
    assert len(CASES) == 3 * 4 * 4 and len(set(CASES)) == len(CASES)


@pytest.mark.parametrize("rows,length,nrec", CASES)
def test_the_record_slots_tile_the_record_buffer(shim, rows, length, nrec):
    l = _layout(shim, rows, length, nrec)
    starts = [int(shim.br_rec_slot(rows, length, nrec, q)) for q in range(nrec + 1)]
    assert l["slot_elems"] > 0
    assert starts[0] == 0
    assert all(b - a == l["slot_elems"] for a, b in zip(starts, starts[1:]))  # back to back, no gap and no overlap
    assert starts[-1] + l["slot_elems"] == l["rec_elems"]                     # the last one ends the buffer
    assert l["rec_now"] == starts[nrec]                                       # the call's own slot is the one behind the run's


@pytest.mark.parametrize("rows,length,nrec", CASES)
def test_the_three_mean_regions_are_disjoint_in_order_and_end_at_the_size(shim, rows, length, nrec):
    l = _layout(shim, rows, length, nrec)
    # the run's means [nrec][len], the slot's mean [len], the re-weighted means of the records [nrec][len]
    regions = [(l["mean_run"], nrec * length), (l["mean_now"], length), (l["mean_reweighted"], nrec * length)]
    assert regions[0][0] == 0
    for (a, na), (b, _) in zip(regions, regions[1:]):
        assert a + na <= b
    assert regions[0][0] + regions[0][1] == regions[1][0] and regions[1][0] + regions[1][1] == regions[2][0]
    last, nlast = regions[-1]
    assert last + nlast <= l["mean_elems"]
    assert last + (nrec + 1) * length == l["mean_elems"]  # the third region is given nrec + 1 rows, as before


@pytest.mark.parametrize("rows,length,nrec", CASES)
def test_the_sizes_are_the_formulas_of_the_requests(shim, rows, length, nrec):
    l = _layout(shim, rows, length, nrec)
    assert l["rec_elems"] == (nrec + 1) * rows * length
    assert l["mean_elems"] == 2 * (nrec + 1) * length
    assert l["rec_now"] == nrec * rows * length         # slot * rows * len of X()
    assert l["mean_now"] == nrec * length               # slot * len of X()
    assert l["mean_reweighted"] == (nrec + 1) * length  # (nrec + 1) * len of X_records
