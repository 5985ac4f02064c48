// zgemm_reduce_args_check.h -- the host side of the reducing product (zgemm_reduce, ZgemmDesc::epi_w) that needs no HIP:
// which shapes it serves, which of its thirteen epilogue bodies a shape runs, and the check of a
// mitdvp_zgemm_reduce_args descriptor (see mitdvp_zgemm_reduce).  Nothing here includes a HIP header, so that a test
// can compile it with a plain C++ compiler (tests/helpers/zgemm_reduce_shim.cpp).
#pragma once
#include <cstddef>

#include "../../include/mitdvp.h"

namespace mitdvp {

// the block shapes reduce_epilogue is instantiated for (3 row blocks run as 4, 3 column blocks as 4)
inline bool zgemm_reduce_shape_ok(int xm, int yn, int di) {
  if (xm < 1 || yn < 1 || di < 1 || xm > 64 || yn > 64 || di > 64) return false;
  const int rb = (di + 15) / 16, cb = ((64 / xm) * (64 / yn) + 15) / 16;
  return (cb == 1) || (cb == 2 && rb <= 2) || (cb <= 4 && rb == 1);
}

// the shapes the unguarded 4 x 4 x 4 epilogue serves (the shape part of zgemm_reduce_full_ok)
inline bool zgemm_reduce_full_shape(int xm, int yn, int di) {
  if (xm < 1 || yn < 1 || xm > 64 || yn > 64) return false;
  const int kp = xm * yn, npair = (64 / xm) * (64 / yn);
  return (di == 16 || di == 32) && npair == 8 && yn % 4 == 0 && kp % 128 == 0 && !(xm & (xm - 1)) && !(yn & (yn - 1)) &&
         8 * (kp + 4) <= 2 * (64 * 17 + 16 * 64);
}

// Which epilogue body the EPI branch of zgemm_kernel runs for a shape -- that branch restated on the host, statement by
// statement (b4 = ZgemmDesc::epi_b4; full = epi_full set AND a fragment-ordered core epi_wf passed):
//    1  reduce_epilogue_b4<1, 2, ., true>       2  reduce_epilogue_b4<2, 2, ., true>      (the unguarded pair)
//    3  reduce_epilogue_b4<1, 1, ., false>      4  reduce_epilogue_b4<1, 2, ., false>
//    5  reduce_epilogue_b4<2, 1, ., false>      6  reduce_epilogue_b4<2, 2, ., false>
//    7  reduce_epilogue_b4w                     8  reduce_epilogue<1, 1>                  9  reduce_epilogue<2, 1>
//   10  reduce_epilogue_blocks<4, 1>           11  reduce_epilogue<1, 2>                 12  reduce_epilogue_blocks<2, 2>
//   13  reduce_epilogue_blocks<1, 4>            0  a shape zgemm_reduce refuses
inline int zgemm_reduce_variant(int xm, int yn, int di, int b4, int full) {
  if (!zgemm_reduce_shape_ok(xm, yn, di)) return 0;
  constexpr int STAGE = 64 * 17 + 16 * 64;  // the smaller of the NN and the NT K loop's LDS stages
  const int rbn = (di + 15) / 16;
  const int npair = (64 / xm) * (64 / yn);
  const int cbn = (npair + 15) / 16;
  if (b4 && !(di <= 4 && npair <= 64) && npair <= 8 && di <= 32) {
    const int kp = xm * yn;
    const bool f = full && yn % 4 == 0 && kp % 128 == 0 && !(xm & (xm - 1)) && !(yn & (yn - 1)) && 8 * (kp + 4) <= 2 * STAGE;
    if (di == 16 && npair == 8 && f) return 1;
    if (di == 32 && npair == 8 && f) return 2;
    if (di <= 16) return npair <= 4 ? 3 : 4;
    return npair <= 4 ? 5 : 6;
  }
  if (b4 && di <= 4 && npair <= 64) return 7;
  if (cbn == 1) return rbn == 1 ? 8 : (rbn == 2 ? 9 : 10);
  if (cbn == 2) return rbn == 1 ? 11 : 12;
  return 13;
}

// The descriptor of mitdvp_zgemm_reduce, checked before any HIP call: every index the operation may touch lies inside the
// caller's buffers -- A and B as dense views, the core as di rows of xm * yn elements ldw apart, C at its (nu, nv, di)
// corners -- and the kernel serves the shape.  Returns nullptr, or what is wrong.
inline const char* zgemm_reduce_args_check(const mitdvp_zgemm_reduce_args* a, const void* A, size_t nA, const void* B, size_t nB,
                                           const void* W, size_t nW, const void* C, size_t nC) {
  typedef __int128 wide;
  if (!a) return "zgemm_reduce: null descriptor";
  if (a->m < 0 || a->n < 0 || a->k < 1) return "zgemm_reduce: negative m or n, or k < 1";
  if (a->transB < 0 || a->transB > 1 || a->acc < 0 || a->acc > 1) return "zgemm_reduce: transB and acc must be 0 or 1";
  if (a->mode3m < -1 || a->mode3m > 1) return "zgemm_reduce: mode3m must be -1, 0 or 1";
  if (a->epi_b4 < -1 || a->epi_b4 > 0 || a->epi_full < -1 || a->epi_full > 0)
    return "zgemm_reduce: epi_b4 and epi_full must be -1 (the library decides) or 0 (off): a form cannot be forced on";
  const long nonneg[] = {a->lda, a->ldb, a->offA, a->offB, a->ldw, a->offW, a->su, a->sv, a->si, a->offC};
  for (long v : nonneg)
    if (v < 0) return "zgemm_reduce: negative leading dimension, stride or offset";
  if (!zgemm_reduce_shape_ok(a->xm, a->yn, a->di)) return "zgemm_reduce: (xm, yn, di) outside the reducing epilogue's range";
  if (a->m % a->xm || a->n % a->yn) return "zgemm_reduce: m, n must be whole groups of xm, yn";
  if (a->m == 0 || a->n == 0) return nullptr;  // nothing is read or written
  if (!A || !B || !W || !C) return "zgemm_reduce: null operand";
  const wide m1 = a->m - 1, n1 = a->n - 1, k1 = a->k - 1;
  const wide nu1 = a->m / a->xm - 1, nv1 = a->n / a->yn - 1, di1 = a->di - 1;
  if ((wide)a->offA + m1 * a->lda + k1 >= (wide)nA) return "zgemm_reduce: the view of A leaves its buffer";
  if ((wide)a->offB + (a->transB ? n1 * a->ldb + k1 : k1 * a->ldb + n1) >= (wide)nB) return "zgemm_reduce: the view of B leaves its buffer";
  if ((wide)a->offW + di1 * a->ldw + (wide)a->xm * a->yn - 1 >= (wide)nW) return "zgemm_reduce: the view of W leaves its buffer";
  if ((wide)a->offC + nu1 * a->su + nv1 * a->sv + di1 * a->si >= (wide)nC) return "zgemm_reduce: the view of C leaves its buffer";
  return nullptr;
}

}  // namespace mitdvp
