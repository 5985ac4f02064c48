// Throw-away C shim over batch_relax_restarts_ok (csrc/batch_relax_plan.h) for tests/test_batch_relax_restart_host.py
// (compiled with g++, no HIP).
#include <string>

#include "../../pytdscf_amd/csrc/batch_relax_plan.h"

using namespace mitdvp;

extern "C" {
int brr_max_restarts() { return BATCH_RELAX_MAX_RESTARTS; }
// nullptr = accepted, else the message
const char* brr_restarts_ok(int max_restarts) {
  static std::string msg;
  return batch_relax_restarts_ok(max_restarts, msg) ? nullptr : msg.c_str();
}
}
