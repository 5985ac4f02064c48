// zgemm_args_check.h -- host-side check of a mitdvp_zgemm_args descriptor (no HIP call; see mitdvp_zgemm_desc)
#pragma once
#include <algorithm>
#include <cstddef>

#include "../../include/mitdvp.h"
#include "common.h"

namespace mitdvp {
// The descriptor of mitdvp_zgemm_desc, checked on the host before any HIP call: every index the logical operation may
// touch must lie inside the caller's buffers, so that no descriptor -- a test's mistake included -- sends the kernel
// outside an allocation.  Footprints: A and B as dense views (a K-tile list only ever leaves tiles out), the stored rows
// of A through the arow_skip map, the rows of C through ldc or the row map, the list as ntm whole rows of klist_stride.
inline void zgemm_args_check(const mitdvp_zgemm_args* a, const void* A, size_t nA, const void* B, size_t nB, const void* C,
                             size_t nC, const int* klist, size_t nklist) {
  typedef __int128 wide;
  if (!a) throw ArgError("zgemm_desc: null descriptor");
  if (a->m < 0 || a->n < 0 || a->k < 0 || a->batch < 0) throw ArgError("zgemm_desc: negative m, n, k or batch");
  if (a->batch > 65535) throw ArgError("zgemm_desc: batch > 65535");
  if (a->tile_cfg < -1 || a->tile_cfg > 2) throw ArgError("zgemm_desc: tile_cfg must be -1, 0, 1 or 2");
  if (a->mode3m < -1 || a->mode3m > 1) throw ArgError("zgemm_desc: mode3m must be -1, 0 or 1");
  const long nonneg[] = {a->lda, a->ldb, a->ldc, a->strideA, a->strideB, a->strideC, a->offA, a->offB, a->offC,
                         a->rowmap_s1, a->rowmap_s2, (long)a->rowmap_p, (long)a->rowmap_r0, (long)a->klist_stride};
  for (long v : nonneg)
    if (v < 0) throw ArgError("zgemm_desc: negative leading dimension, stride, offset or row-map parameter");
  if (a->arow_skip && (a->arow_skip < 2 || a->transA || klist))
    throw ArgError("zgemm_desc: arow_skip must be >= 2 and needs a plain, untransposed A");
  if (a->m == 0 || a->n == 0 || a->batch == 0) return;  // nothing is read or written
  if ((!A && a->k > 0) || (!B && a->k > 0) || !C) throw ArgError("zgemm_desc: null operand");
  const wide bm1 = a->batch - 1, m1 = a->m - 1, n1 = a->n - 1, k1 = a->k - 1;
  if (a->k > 0) {
    const wide srow = a->arow_skip > 1 ? m1 + m1 / (a->arow_skip - 1) + 1 : m1;  // stored row of the last logical row
    const wide lastA = (wide)a->offA + bm1 * a->strideA + (a->transA ? k1 * a->lda + m1 : srow * a->lda + k1);
    const wide lastB = (wide)a->offB + bm1 * a->strideB + (a->transB ? n1 * a->ldb + k1 : k1 * a->ldb + n1);
    if (lastA >= (wide)nA) throw ArgError("zgemm_desc: the view of A leaves its buffer");
    if (lastB >= (wide)nB) throw ArgError("zgemm_desc: the view of B leaves its buffer");
  }
  wide rowC = m1 * a->ldc;
  if (a->rowmap_p > 0) {
    rowC = 0;
    for (long r = a->rowmap_r0; r < (long)a->rowmap_r0 + a->m; ++r)
      rowC = std::max(rowC, (wide)(r % a->rowmap_p) * a->rowmap_s1 + (wide)(r / a->rowmap_p) * a->rowmap_s2);
  }
  if ((wide)a->offC + bm1 * a->strideC + rowC + n1 >= (wide)nC) throw ArgError("zgemm_desc: the view of C leaves its buffer");
  if (klist) {
    if (a->transA || a->transB || a->k % 16 != 0 || a->k < 16 || a->tile_cfg != 1)
      throw ArgError("zgemm_desc: a K-tile list needs NN operands, K % 16 == 0, K >= 16 and tile_cfg 1");
    const int nkt = a->k / 16, ntm = (a->m + 63) / 64;
    if (a->klist_stride < 1 + nkt) throw ArgError("zgemm_desc: klist_stride < 1 + K / 16");
    if ((wide)ntm * a->klist_stride > (wide)nklist) throw ArgError("zgemm_desc: the K-tile list leaves its buffer");
    for (int tm = 0; tm < ntm; ++tm) {
      const int* row = klist + (size_t)tm * a->klist_stride;
      if (row[0] < 0 || row[0] > nkt) throw ArgError("zgemm_desc: K-tile count out of range");
      for (int q = 1; q <= row[0]; ++q)
        if (row[q] < 0 || row[q] >= nkt || (q > 1 && row[q] <= row[q - 1]))
          throw ArgError("zgemm_desc: K-tile indices must be ascending and below K / 16");
    }
  }
}

}  // namespace mitdvp
