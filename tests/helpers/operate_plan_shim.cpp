// Throw-away C shim over csrc/batch_operate_plan.h for tests/test_batch_operate_host.py (compiled with g++, no HIP).
#include <cstring>

#include "../../pytdscf_amd/csrc/batch_operate_plan.h"

using namespace mitdvp;

namespace {
const char* keep(const std::string& why) {
  static std::string msg;
  msg = why;
  return msg.c_str();
}
}  // namespace

extern "C" {
int bop_max_mpo() { return BATCH_MAX_MPO; }
unsigned long long bop_max_bytes() { return BATCH_OPERATE_MAX_BYTES; }
// shapes: [L][5] ints (dl, d, dr, ml, mr); out: the 14 offsets in the order of BatchOperatePlan; tabs: [3][L + 1] the
// prefix sums site, mix, ov; nullptr = accepted, else the message
const char* bop_plan(const int* shapes, int op_id, int L, unsigned long long* out, long long* tabs) {
  static_assert(sizeof(BatchShape) == 5 * sizeof(int), "BatchShape is five ints");
  BatchOperatePlan p;
  std::string why;
  if (!batch_operate_plan(reinterpret_cast<const BatchShape*>(shapes), op_id, L, p, why)) return keep(why);
  const size_t o[14] = {p.o_ket, p.o_prev, p.o_mix, p.o_ov, p.o_x, p.o_y, p.o_work, p.o_spare, p.o_h, p.o_sig, p.o_t0, p.o_t1, p.o_id, p.total};
  for (int k = 0; k < 14; ++k) out[k] = o[k];
  for (int b = 0; b <= L; ++b) {
    tabs[b] = p.site[(size_t)b];
    tabs[(L + 1) + b] = p.mix[(size_t)b];
    tabs[2 * (L + 1) + b] = p.ov[(size_t)b];
  }
  return nullptr;
}
const char* bop_fits(unsigned long long nsel, unsigned long long total) {
  BatchOperatePlan plan;
  plan.total = (size_t)total;
  std::string why;
  return batch_operate_fits((size_t)nsel, plan, why) ? nullptr : keep(why);
}
}
