// batch_records.h -- where the records of a batch request and their means lie (RecordStore, engine_batch.h).  Nothing here
// includes a HIP header, so that a test can compile it with a plain C++ compiler (tests/helpers/batch_records_shim.cpp).
#pragma once
#include <cstddef>

namespace mitdvp {

// A request keeps nrec records of a run, each [rows][len] doubles, and ONE more slot behind them for the call on the
// current state (slot q = nrec), so that such a call overwrites no record of the run.  The mean buffer has three regions:
// the means of the run's records [nrec][len], the mean of the slot [len], and the records' means under weights given
// later [nrec + 1][len] -- re-weighting overwrites neither of the first two.  All offsets and counts are in elements;
// these are the only place the products are written.
struct BatchRecords {
  size_t rows = 0, len = 0, nrec = 0;

  size_t slot_elems() const { return rows * len; }
  size_t rec_elems() const { return (nrec + 1) * slot_elems(); }
  size_t rec_slot(size_t q) const { return q * slot_elems(); }
  size_t rec_now() const { return rec_slot(nrec); }

  size_t mean_elems() const { return 2 * (nrec + 1) * len; }
  size_t mean_run() const { return 0; }
  size_t mean_now() const { return nrec * len; }
  size_t mean_reweighted() const { return (nrec + 1) * len; }
};

}  // namespace mitdvp
