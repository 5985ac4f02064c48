// Throw-away C shim over csrc/batch_records.h for tests/test_batch_records_host.py (compiled with g++, no HIP).
#include "../../pytdscf_amd/csrc/batch_records.h"

using namespace mitdvp;

extern "C" {
// out: rec_elems, slot_elems, rec_now, mean_elems, mean_run, mean_now, mean_reweighted
void br_layout(unsigned long long rows, unsigned long long len, unsigned long long nrec, unsigned long long* out) {
  const BatchRecords l{(size_t)rows, (size_t)len, (size_t)nrec};
  out[0] = l.rec_elems(); out[1] = l.slot_elems(); out[2] = l.rec_now();
  out[3] = l.mean_elems(); out[4] = l.mean_run(); out[5] = l.mean_now(); out[6] = l.mean_reweighted();
}
unsigned long long br_rec_slot(unsigned long long rows, unsigned long long len, unsigned long long nrec, unsigned long long q) {
  return BatchRecords{(size_t)rows, (size_t)len, (size_t)nrec}.rec_slot((size_t)q);
}
}
