// Throw-away C shim over csrc/batch_deflate_plan.h for tests/test_batch_deflate_host.py (compiled with g++, no HIP).
#include <string>
#include <vector>

#include "../../pytdscf_amd/csrc/batch_deflate_plan.h"

using namespace mitdvp;

namespace {
std::vector<BatchShape> shapes(const int* dl, const int* d, const int* dr, int L) {
  std::vector<BatchShape> s((size_t)L);
  for (int p = 0; p < L; ++p) s[(size_t)p] = BatchShape{dl[p], d[p], dr[p], 1, 1};
  return s;
}
}  // namespace

extern "C" {
int bdp_max_deflate() { return BATCH_MAX_DEFLATE; }
unsigned long long bdp_max_bytes() { return BATCH_DEFLATE_MAX_BYTES; }
// nullptr = accepted, else the message
const char* bdp_room(int count) {
  static std::string msg;
  return batch_deflate_room(count, msg) ? nullptr : msg.c_str();
}
const char* bdp_weights_ok(const double* w, int n) {
  static std::string msg;
  return batch_deflate_weights_ok(w, n, msg) ? nullptr : msg.c_str();
}
// out: blk_len, max_site, o_q, per
void bdp_plan(const int* dl, const int* d, const int* dr, int L, int slots, unsigned long long* out) {
  const std::vector<BatchShape> s = shapes(dl, d, dr, L);
  const BatchDeflatePlan pl = batch_deflate_plan(s.data(), L, slots);
  out[0] = pl.blk_len;
  out[1] = pl.max_site;
  out[2] = pl.o_q;
  out[3] = pl.per;
}
const char* bdp_fits(const int* dl, const int* d, const int* dr, int L, int slots, unsigned long long nrep) {
  static std::string msg;
  const std::vector<BatchShape> s = shapes(dl, d, dr, L);
  return batch_deflate_fits(s.data(), L, slots, (size_t)nrep, msg) ? nullptr : msg.c_str();
}
}
