// Throw-away C shim over csrc/zgemm_reduce_args_check.h for tests/test_zgemm_reduce_host.py (compiled with g++, no HIP).
#include "../../pytdscf_amd/csrc/zgemm_reduce_args_check.h"

using namespace mitdvp;

extern "C" {
int zr_shape_ok(int xm, int yn, int di) { return zgemm_reduce_shape_ok(xm, yn, di) ? 1 : 0; }
int zr_full_shape(int xm, int yn, int di) { return zgemm_reduce_full_shape(xm, yn, di) ? 1 : 0; }
int zr_variant(int xm, int yn, int di, int b4, int full) { return zgemm_reduce_variant(xm, yn, di, b4, full); }
int zr_sizeof_args() { return (int)sizeof(mitdvp_zgemm_reduce_args); }
int zr_offsetof_mode3m() { return (int)offsetof(mitdvp_zgemm_reduce_args, mode3m); }
// the footprint check on buffers of the given sizes (the pointers only have to be non-null); nullptr = accepted
const char* zr_check(const mitdvp_zgemm_reduce_args* a, size_t nA, size_t nB, size_t nW, size_t nC) {
  static const char one = 0;
  return zgemm_reduce_args_check(a, &one, nA, &one, nB, &one, nW, &one, nC);
}
}
