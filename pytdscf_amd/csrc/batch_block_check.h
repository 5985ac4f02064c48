// batch_block_check.h -- the host side of the test hook of the batch kernels' building blocks (k_batch_block in
// batch_site.hip, mitdvp_batch_block) that needs no HIP: the footprint of an operation -- what it reads, writes and needs
// as work space, per copy -- and the check of a mitdvp_batch_block_args descriptor against the kernels' own envelope and
// the caller's buffers.  Nothing here includes a HIP header, so that a test can compile it with a plain C++ compiler
// (tests/helpers/batch_block_shim.cpp).
#pragma once
#include <cstddef>

#include "../../include/mitdvp.h"
#include "batch_shape.h"

namespace mitdvp {

constexpr int BATCH_BLOCK_MAX_COPIES = 16;
constexpr int BATCH_BLOCK_MAX_CHAIN = 6;  // sites of the OVERLAP chain: dims = (L, d, the L - 1 inner bonds)

// Complex elements per copy of the four operands, the two results and the three work areas; doubles of the info record.
//   op       dims                      in0         in1        in2        in3      out0          out1     work
//   MATMUL   M, N, K                   A  M x K    B  K x N   -          -        A B           -        tmp; -; -
//   HEFF     dl, d, dr, ml, mr         L  a,c,b    w2l        R  r,t,s   v a,j,s  H v           -        X; Y; -
//   KEFF     dim, m                    L  a,c,b    -          R  r,c,s   sigma    K sigma       -        X; -; -
//   ENV      din, min, d, dout, mout   env b,p,s   w2el/w2er  bra        ket      env' a,q,r    -        X; Y; -
//   OVERLAP  L, d, b_1 .. b_(L-1)      ket sites   bra sites  -          -        <bra|ket>     -        T; T'; U
//   QR       m, n                      A (layout of the variant)  -      -        Q, as A       R / R^T  work matrix; -; -
//   SPLIT    m, n, r                   theta m x n -          -          -        B  r x n      C' m x r work copy; -; -
// info: [0] the return code (SS_OK = 0); SPLIT also [1] kept weight, [2] discarded fraction, [3 .. 3 + m) the squared row
// norms in descending order.
struct BatchBlockFoot {
  size_t in[4] = {0, 0, 0, 0}, out0 = 0, out1 = 0, info = 1, work[3] = {0, 0, 0};
  size_t work_total() const { return in[0] + in[1] + in[2] + in[3] + work[0] + work[1] + work[2]; }
};

// nullptr and the footprint, or what is wrong: an unknown op or variant, a dimension below 1, a shape outside the
// envelope of the kernels that call the function (batch_shape.h, BATCH_PAIR_MAX_DIM), ncopies outside 1 .. 16
inline const char* batch_block_shape_check(const mitdvp_batch_block_args* a, BatchBlockFoot* foot) {
  if (!a) return "batch_block: null descriptor";
  if (a->ncopies < 1 || a->ncopies > BATCH_BLOCK_MAX_COPIES) return "batch_block: ncopies outside 1 .. 16";
  const int* q = a->dims;
  BatchBlockFoot f;
  int ndims = 0, nvariants = 1;
  switch (a->op) {
    case MITDVP_BLOCK_MATMUL: ndims = 3; nvariants = 3; break;
    case MITDVP_BLOCK_HEFF: ndims = 5; break;
    case MITDVP_BLOCK_KEFF: ndims = 2; break;
    case MITDVP_BLOCK_ENV: ndims = 5; nvariants = 3; break;
    case MITDVP_BLOCK_OVERLAP:
      if (q[0] < 1 || q[0] > BATCH_BLOCK_MAX_CHAIN) return "batch_block: the chain of an overlap has 1 .. 6 sites";
      ndims = 1 + q[0];
      break;
    case MITDVP_BLOCK_QR: ndims = 2; nvariants = 2; break;
    case MITDVP_BLOCK_SPLIT: ndims = 3; break;
    default: return "batch_block: unknown op";
  }
  if (a->variant < 0 || a->variant >= nvariants) return "batch_block: unknown variant of this op";
  for (int k = 0; k < ndims; ++k)
    if (q[k] < 1) return "batch_block: a dimension below 1";
  const char* site = "batch_block: more than BATCH_MAX_SITE elements in a tensor";
  const char* bond = "batch_block: a bond above BATCH_MAX_BOND";
  const char* mpo = "batch_block: an MPO bond above BATCH_MAX_MPO";
  switch (a->op) {
    case MITDVP_BLOCK_MATMUL: {
      const long M = q[0], N = q[1], K = q[2];
      if (M * K > BATCH_MAX_SITE || K * N > BATCH_MAX_SITE || M * N > BATCH_MAX_SITE) return site;
      if (a->variant == 1 && N != K) return "batch_block: dst = A needs N = K";
      if (a->variant == 2 && M != K) return "batch_block: dst = B needs M = K";
      f.in[0] = M * K; f.in[1] = K * N; f.out0 = M * N; f.work[0] = M * N;
      break;
    }
    case MITDVP_BLOCK_HEFF: {
      const long dl = q[0], d = q[1], dr = q[2], ml = q[3], mr = q[4];
      if (dl > BATCH_MAX_BOND || dr > BATCH_MAX_BOND) return bond;
      if (ml > BATCH_MAX_MPO || mr > BATCH_MAX_MPO) return mpo;
      if (dl * d * dr > BATCH_MAX_SITE) return site;
      f.in[0] = dl * ml * dl; f.in[1] = d * mr * ml * d; f.in[2] = dr * mr * dr; f.in[3] = dl * d * dr;
      f.out0 = dl * d * dr; f.work[0] = dl * ml * d * dr; f.work[1] = dl * d * mr * dr;
      break;
    }
    case MITDVP_BLOCK_KEFF: {
      const long dim = q[0], m = q[1];
      if (dim > BATCH_MAX_BOND) return bond;
      if (m > BATCH_MAX_MPO) return mpo;
      f.in[0] = f.in[2] = dim * m * dim; f.in[3] = f.out0 = dim * dim; f.work[0] = dim * m * dim;
      break;
    }
    case MITDVP_BLOCK_ENV: {
      const long din = q[0], mi = q[1], d = q[2], dout = q[3], mo = q[4];
      if (din > BATCH_MAX_BOND || dout > BATCH_MAX_BOND) return bond;
      if (mi > BATCH_MAX_MPO || mo > BATCH_MAX_MPO) return mpo;
      if (din * d * dout > BATCH_MAX_SITE) return site;
      f.in[0] = din * mi * din; f.in[1] = mo * d * d * mi; f.in[2] = f.in[3] = din * d * dout;
      f.out0 = dout * mo * dout; f.work[0] = d * dout * mi * din; f.work[1] = dout * mo * d * din;
      break;
    }
    case MITDVP_BLOCK_OVERLAP: {
      const int L = q[0];
      const long d = q[1];
      long tot = 0, mb = 1, ms = 1;
      for (int p = 0; p < L; ++p) {
        const long dl = p == 0 ? 1 : q[1 + p], dr = p == L - 1 ? 1 : q[2 + p];
        if (dl > BATCH_MAX_BOND || dr > BATCH_MAX_BOND) return bond;
        if (dl * d * dr > BATCH_MAX_SITE) return site;
        tot += dl * d * dr;
        if (dl * d * dr > ms) ms = dl * d * dr;
        if (dr * dr > mb) mb = dr * dr;
      }
      f.in[0] = f.in[1] = tot; f.out0 = 1; f.work[0] = f.work[1] = mb; f.work[2] = ms;
      break;
    }
    case MITDVP_BLOCK_QR: {
      const long m = q[0], n = q[1];
      if (m < n) return "batch_block: a thin QR needs m >= n";
      if (n > BATCH_MAX_BOND) return bond;
      if (m * n > BATCH_MAX_SITE) return site;
      f.in[0] = f.out0 = f.work[0] = m * n; f.out1 = n * n;
      break;
    }
    default: {  // MITDVP_BLOCK_SPLIT
      const long m = q[0], n = q[1], r = q[2];
      if (m > BATCH_PAIR_MAX_DIM || n > BATCH_PAIR_MAX_DIM) return "batch_block: split m or n above BATCH_PAIR_MAX_DIM";
      if (r > m || r > n || r > BATCH_MAX_BOND) return "batch_block: split r above min(m, n, BATCH_MAX_BOND)";
      f.in[0] = f.work[0] = m * n; f.out0 = r * n; f.out1 = m * r; f.info = 3 + m;
      break;
    }
  }
  if (foot) *foot = f;
  return nullptr;
}

// The descriptor of mitdvp_batch_block and the caller's buffers, checked before any HIP call: nin / nout0 / nout1 in
// complex elements, ninfo in doubles; the operands hold one copy, the results ncopies.
inline const char* batch_block_check(const mitdvp_batch_block_args* a, const void* const in[4], const size_t nin[4], const void* out0,
                                     size_t nout0, const void* out1, size_t nout1, const void* info, size_t ninfo, BatchBlockFoot* foot) {
  BatchBlockFoot f;
  if (const char* bad = batch_block_shape_check(a, &f)) return bad;
  static const char* const short_in[4] = {"batch_block: operand 0 is shorter than the operation's footprint",
                                          "batch_block: operand 1 is shorter than the operation's footprint",
                                          "batch_block: operand 2 is shorter than the operation's footprint",
                                          "batch_block: operand 3 is shorter than the operation's footprint"};
  for (int k = 0; k < 4; ++k)
    if (f.in[k] && (!in[k] || nin[k] < f.in[k])) return short_in[k];
  const size_t nc = (size_t)a->ncopies;
  if (!out0 || nout0 < nc * f.out0) return "batch_block: result 0 is shorter than the operation's footprint";
  if (f.out1 && (!out1 || nout1 < nc * f.out1)) return "batch_block: result 1 is shorter than the operation's footprint";
  if (!info || ninfo < nc * f.info) return "batch_block: the info record is shorter than the operation's footprint";
  if (foot) *foot = f;
  return nullptr;
}

}  // namespace mitdvp
