// Throw-away C shim over csrc/batch_cross_mpo_plan.h for tests/test_batch_cross_mpo_host.py (compiled with g++, no HIP).
#include <cstring>

#include "../../pytdscf_amd/csrc/batch_cross_mpo_plan.h"

using namespace mitdvp;

namespace {
const char* keep(const std::string& why) {
  static std::string msg;
  msg = why;
  return msg.c_str();
}
}  // namespace

extern "C" {
int xm_max_mpo() { return BATCH_MAX_MPO; }
int xm_max_entries() { return BATCH_CROSS_MAX_PAIRS; }
unsigned long long xm_max_bytes() { return BATCH_CROSS_MPO_MAX_BYTES; }
int xm_sizeof_entry() { return (int)sizeof(BatchCrossMpoEntry); }
// shapes: [nops][L][5] ints (dl, d, dr, ml, mr); out: o_e1, o_x, o_y, total; nullptr = accepted, else the message
const char* xm_plan(const int* shapes, const int* op_ids, int L, int nops, unsigned long long* out) {
  static_assert(sizeof(BatchShape) == 5 * sizeof(int), "BatchShape is five ints");
  BatchCrossMpoPlan plan;
  std::string why;
  if (!batch_cross_mpo_plan(reinterpret_cast<const BatchShape*>(shapes), op_ids, L, nops, plan, why)) return keep(why);
  out[0] = plan.o_e1; out[1] = plan.o_x; out[2] = plan.o_y; out[3] = plan.total;
  return nullptr;
}
const char* xm_fits(unsigned long long nentries, unsigned long long total) {
  BatchCrossMpoPlan plan;
  plan.total = (size_t)total;
  std::string why;
  return batch_cross_mpo_fits((size_t)nentries, plan, why) ? nullptr : keep(why);
}
const char* xm_entries(int B, int has_snap, int nentries, const int* bra, const int* ket, const int* op_id) {
  std::string why;
  return batch_cross_mpo_entries_ok(B, has_snap != 0, nentries, bra, ket, op_id, why) ? nullptr : keep(why);
}
}
