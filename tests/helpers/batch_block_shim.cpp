// Throw-away C shim over csrc/batch_block_check.h for tests/test_batch_blocks_host.py (compiled with g++, no HIP).
#include "../../pytdscf_amd/csrc/batch_block_check.h"

using namespace mitdvp;

extern "C" {
int bb_sizeof_args() { return (int)sizeof(mitdvp_batch_block_args); }
int bb_offsetof_ncopies() { return (int)offsetof(mitdvp_batch_block_args, ncopies); }
int bb_offsetof_scl() { return (int)offsetof(mitdvp_batch_block_args, scl); }
// MAX_SITE, MAX_MPO, MAX_BOND, PAIR_MAX_DIM, MAX_COPIES, MAX_CHAIN
void bb_limits(long out[6]) {
  out[0] = BATCH_MAX_SITE; out[1] = BATCH_MAX_MPO; out[2] = BATCH_MAX_BOND; out[3] = BATCH_PAIR_MAX_DIM;
  out[4] = BATCH_BLOCK_MAX_COPIES; out[5] = BATCH_BLOCK_MAX_CHAIN;
}
// the shape check alone; out: in[4], out0, out1, info, work[3].  nullptr = accepted
const char* bb_shape(const mitdvp_batch_block_args* a, size_t out[10]) {
  BatchBlockFoot f;
  const char* bad = batch_block_shape_check(a, &f);
  if (bad) return bad;
  for (int k = 0; k < 4; ++k) out[k] = f.in[k];
  out[4] = f.out0; out[5] = f.out1; out[6] = f.info;
  for (int k = 0; k < 3; ++k) out[7 + k] = f.work[k];
  return nullptr;
}
// the whole check on buffers of the given sizes (a size of 0 passes a null pointer); nullptr = accepted
const char* bb_check(const mitdvp_batch_block_args* a, const size_t nin[4], size_t nout0, size_t nout1, size_t ninfo) {
  static const char one = 0;
  const void* in[4];
  for (int k = 0; k < 4; ++k) in[k] = nin[k] ? &one : nullptr;
  return batch_block_check(a, in, nin, nout0 ? &one : nullptr, nout0, nout1 ? &one : nullptr, nout1, ninfo ? &one : nullptr, ninfo, nullptr);
}
}
