// Throw-away C shim over csrc/batch_relax_plan.h for tests/test_batch_relax_host.py (compiled with g++, no HIP).
#include <string>

#include "../../pytdscf_amd/csrc/batch_relax_plan.h"

using namespace mitdvp;

extern "C" {
int brx_max_krylov() { return BATCH_RELAX_MAX_KRYLOV; }
int brx_exp_slots() { return BATCH_EXP_KRYLOV_SLOTS; }
unsigned long long brx_carve(long max_site, long max_bond, int relax, int max_diag_krylov) {
  return (unsigned long long)batch_krylov_carve(max_site, max_bond, relax, max_diag_krylov);
}
// nullptr = accepted, else the message
const char* brx_kcap_ok(int max_diag_krylov) {
  static std::string msg;
  return batch_relax_kcap_ok(max_diag_krylov, msg) ? nullptr : msg.c_str();
}
}
