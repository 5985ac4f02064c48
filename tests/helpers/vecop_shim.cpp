// Throw-away C shim over csrc/vecop_check.h for tests/test_vecops_host.py (compiled with g++, no HIP).
#include "../../pytdscf_amd/csrc/vecop_check.h"

#include <cstddef>
#include <cstdint>

extern "C" {
int vo_sizeof_args() { return (int)sizeof(mitdvp_vecop_args); }
int vo_offsetof_strides() { return (int)offsetof(mitdvp_vecop_args, strides); }
int vo_offsetof_eps() { return (int)offsetof(mitdvp_vecop_args, eps); }
int vo_offsetof_f() { return (int)offsetof(mitdvp_vecop_args, f); }
void vo_limits(long out[7]) {
  out[0] = mitdvp::VECOP_NPART; out[1] = mitdvp::VECOP_MAXK; out[2] = mitdvp::VECOP_SMALL_VEC_N; out[3] = mitdvp::VECOP_MAX_BLOCKS;
  out[4] = mitdvp::VECOP_MAX_BATCH; out[5] = mitdvp::VECOP_MAX_DIM; out[6] = (long)mitdvp::VECOP_MAX_BYTES;
}
// out: zin[3], rin, idx, zio[2], rio, zwr[2], rwr, empty, own_return
const char* vo_shape(const mitdvp_vecop_args* a, const int* idx, size_t nidx, size_t out[13]) {
  mitdvp::VecopFoot f;
  const char* bad = mitdvp::vecop_shape_check(a, idx, nidx, &f);
  if (bad) return bad;
  const size_t v[13] = {f.zin[0], f.zin[1], f.zin[2], f.rin, f.idx, f.zio[0], f.zio[1], f.rio, f.zwr[0], f.zwr[1], f.rwr,
                        (size_t)f.empty, (size_t)f.own_return};
  for (int k = 0; k < 13; ++k) out[k] = v[k];
  return nullptr;
}
// n: zin[3], rin, zio[2], rio in elements; the buffers are addresses one after the other (never dereferenced; only idx,
// which the check reads, is real); alias >= 0: complex result 0 is laid over complex input `alias` instead
const char* vo_check(const mitdvp_vecop_args* a, const size_t n[7], const int* idx, size_t nidx, int alias) {
  uintptr_t p = (uintptr_t)1 << 20;
  const void* zin[3];
  const void* zio[2];
  const size_t nzin[3] = {n[0], n[1], n[2]}, nzio[2] = {n[4], n[5]};
  for (int k = 0; k < 3; ++k) { zin[k] = n[k] ? (const void*)p : nullptr; p += n[k] * 16; }
  const void* rin = n[3] ? (const void*)p : nullptr; p += n[3] * 8;
  for (int k = 0; k < 2; ++k) { zio[k] = n[4 + k] ? (const void*)p : nullptr; p += n[4 + k] * 16; }
  const void* rio = n[6] ? (const void*)p : nullptr;
  if (alias >= 0 && alias < 3) zio[0] = zin[alias];
  return mitdvp::vecop_check(a, zin, nzin, rin, n[3], idx, nidx, zio, nzio, rio, n[6], nullptr);
}
}
