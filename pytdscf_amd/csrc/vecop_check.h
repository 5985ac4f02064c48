// vecop_check.h -- the host side of the test hook of the Krylov vector and layout kernels (vecops.hip, mitdvp_vecop) that
// needs no HIP: the footprint of every op -- one past the last element read and written, per buffer -- and the check of a
// mitdvp_vecop_args descriptor against the caller's buffers.  Nothing here includes a HIP header, so that a test can
// compile it with a plain C++ compiler (tests/helpers/vecop_shim.cpp).  The op table is the comment in include/mitdvp.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mitdvp.h"

namespace mitdvp {

// vecops.h's constants, repeated because that header needs HIP (capi.hip asserts that they agree)
constexpr int VECOP_NPART = 256;
constexpr int VECOP_MAXK = 21;
constexpr long VECOP_SMALL_VEC_N = 16384;
constexpr int VECOP_MAX_BLOCKS = 64;        // BlockList, and the blocks of ident_deviation_multi's mask
constexpr long VECOP_MAX_BATCH = 65535;     // grid z of the transpose
constexpr long VECOP_MAX_DIM = 1L << 28;    // any one dimension or stride
constexpr size_t VECOP_MAX_BYTES = 128u << 20;  // all buffers of one call together

// Elements (complex for zin / zio, doubles for rin / rio, ints for idx) each buffer must hold = one past the last element
// the op reads or writes there; zwr / rwr: one past the last element WRITTEN (<= zio / rio; 0: the buffer is only read or
// not taken).  empty: a zero-size call, nothing is launched and the outputs stay as they are; own_return: the wrapper has
// its own zero-size return, so the hook still calls it.
struct VecopFoot {
  size_t zin[3] = {0, 0, 0}, rin = 0, idx = 0, zio[2] = {0, 0}, rio = 0, zwr[2] = {0, 0}, rwr = 0;
  bool empty = false, own_return = false;
};

namespace vecop_detail {
constexpr long SAT = 1L << 40;  // products saturate here: far above any buffer the byte cap lets through
inline long mul(long a, long b) {
  if (a == 0 || b == 0) return 0;
  return (a >= SAT || b >= SAT || a > SAT / b) ? SAT : a * b;
}
inline long add(long a, long b) { return a + b >= SAT ? SAT : a + b; }
// one past the last element of a rows x cols matrix with leading dimension ld (0 if it has no element)
inline long mat(long rows, long cols, long ld) { return rows > 0 && cols > 0 ? add(mul(rows - 1, ld), cols) : 0; }
inline bool overlap(const void* p, size_t pb, const void* q, size_t qb) {
  if (!p || !q || !pb || !qb) return false;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qb && b < a + pb;
}
}  // namespace vecop_detail

// nullptr and the footprint, or what is wrong with the descriptor alone.  idx: the caller's int array (host), needed for
// the footprints that depend on its values (map2, block indices); nidx its length.
inline const char* vecop_shape_check(const mitdvp_vecop_args* a, const int* idx, size_t nidx, VecopFoot* foot) {
  using namespace vecop_detail;
  if (!a) return "vecop: null descriptor";
  int nd = 0, ns = 0, nvar = 1;
  switch (a->op) {
    case MITDVP_VECOP_DOT: nd = 1; nvar = 2; break;
    case MITDVP_VECOP_SUMSQ: nd = 1; break;
    case MITDVP_VECOP_LANCZOS_UPDATE: nd = 1; nvar = 2; break;
    case MITDVP_VECOP_LANCZOS_UPDATE_DEF: nd = 2; nvar = 4; break;
    case MITDVP_VECOP_LANCZOS_STEP_SMALL: nd = 1; nvar = 4; break;
    case MITDVP_VECOP_SCALE_INV_NORM: nd = 1; break;
    case MITDVP_VECOP_MULTI_DOT: nd = 2; ns = 1; break;
    case MITDVP_VECOP_ARNOLDI_UPDATE: nd = 2; ns = 1; break;
    case MITDVP_VECOP_LINCOMB: nd = 2; ns = 1; nvar = 4; break;
    case MITDVP_VECOP_AXPBY: nd = 1; break;
    case MITDVP_VECOP_SCALE: nd = 1; break;
    case MITDVP_VECOP_TRANSPOSE: nd = 3; ns = 4; break;
    case MITDVP_VECOP_TRANSPOSE_REV3: nd = 3; break;
    case MITDVP_VECOP_PERMUTE_0213: nd = 4; break;
    case MITDVP_VECOP_PERMUTE5: nd = 5; ns = 5; nvar = 2; break;
    case MITDVP_VECOP_PHYS_DIAG: nd = 3; nvar = 2; break;
    case MITDVP_VECOP_COPY2D: nd = 3; ns = 2; nvar = 2; break;
    case MITDVP_VECOP_COPY_RAW: nd = 1; break;
    case MITDVP_VECOP_IDENTITY: nd = 2; ns = 1; break;
    case MITDVP_VECOP_SCALE_COLS: nd = 2; ns = 1; break;
    case MITDVP_VECOP_GATHER_BLOCKS: nd = 5; break;
    case MITDVP_VECOP_FILL_SCALED_BLOCKS: nd = 4; ns = 1; break;
    case MITDVP_VECOP_ACCUM_SCALED_BLOCKS: nd = 3; ns = 1; break;
    case MITDVP_VECOP_COL_SUMSQ: nd = 2; break;
    case MITDVP_VECOP_ROW_SUMSQ: nd = 2; break;
    case MITDVP_VECOP_SHELL_SUMSQ: nd = 1; break;
    case MITDVP_VECOP_IDENT_DEV: nd = 1; ns = 1; break;
    case MITDVP_VECOP_IDENT_DEV_MULTI: nd = 2; ns = 2; nvar = 2; break;
    default: return "vecop: unknown op";
  }
  if (a->variant < 0 || a->variant >= nvar) return "vecop: unknown variant of this op";
  const long* d = a->dims;
  const long* s = a->strides;
  for (int k = 0; k < nd; ++k) {
    if (d[k] < 0) return "vecop: a negative dimension";
    if (d[k] > VECOP_MAX_DIM) return "vecop: a dimension above 2^28";
  }
  for (int k = 0; k < ns; ++k) {
    if (s[k] < 0) return "vecop: a negative stride";
    if (s[k] > VECOP_MAX_DIM) return "vecop: a stride above 2^28";
  }
  VecopFoot f;
  const int v = a->variant;
  const size_t NP = VECOP_NPART;
  const char* lead = "vecop: a leading dimension below the row length";
  const char* toomany = "vecop: more than 64 blocks in a list";
  const char* noidx = "vecop: the int array is shorter than the operation's footprint";
  switch (a->op) {
    case MITDVP_VECOP_DOT:
      f.zin[0] = f.zin[1] = d[0]; f.zio[0] = f.zwr[0] = NP; f.empty = d[0] == 0;
      break;
    case MITDVP_VECOP_SUMSQ:
      f.zin[0] = d[0]; f.rio = f.rwr = NP; f.empty = d[0] == 0;
      break;
    case MITDVP_VECOP_LANCZOS_UPDATE:
      f.zio[0] = f.zwr[0] = f.zin[0] = d[0]; f.zin[2] = NP; f.rio = f.rwr = NP; f.empty = d[0] == 0;
      if (v & 1) { f.zin[1] = d[0]; f.rin = NP; }
      break;
    case MITDVP_VECOP_LANCZOS_UPDATE_DEF:
      if (d[1] >= VECOP_MAXK) return "vecop: l >= MAXK";
      f.zio[0] = f.zwr[0] = f.zin[0] = d[0]; f.zin[2] = NP; f.rin = (size_t)d[1] * NP; f.rio = f.rwr = NP; f.empty = d[0] == 0;
      if (v & 1) f.zin[1] = d[0];
      break;
    case MITDVP_VECOP_LANCZOS_STEP_SMALL:
      if (d[0] > VECOP_SMALL_VEC_N) return "vecop: n > SMALL_VEC_N for the one-workgroup step";
      f.zio[0] = f.zwr[0] = f.zin[0] = d[0]; f.zio[1] = f.zwr[1] = NP; f.rio = f.rwr = NP; f.empty = d[0] == 0;
      if (v & 2) f.zin[1] = d[0];
      if (v & 1) { f.zin[2] = d[0]; f.rin = NP; }
      break;
    case MITDVP_VECOP_SCALE_INV_NORM:
      f.zio[0] = f.zwr[0] = d[0]; f.rin = NP; f.empty = d[0] == 0;
      break;
    case MITDVP_VECOP_MULTI_DOT:
    case MITDVP_VECOP_ARNOLDI_UPDATE:
    case MITDVP_VECOP_LINCOMB:
      if (d[1] > VECOP_MAXK) return "vecop: k > MAXK";
      if (d[1] > 1 && s[0] < d[0]) return lead;
      // k = 0 is empty for the dots only: the update still writes v and its norm, the combination zeros
      f.zin[0] = mat(d[1], d[0], s[0]); f.empty = d[0] == 0;
      if (a->op == MITDVP_VECOP_MULTI_DOT) {
        f.zin[1] = d[0]; f.zio[0] = f.zwr[0] = (size_t)d[1] * NP; f.empty = d[0] == 0 || d[1] == 0;
      } else if (a->op == MITDVP_VECOP_ARNOLDI_UPDATE) {
        f.zin[1] = (size_t)d[1] * NP; f.zio[0] = f.zwr[0] = d[0]; f.rio = f.rwr = NP;
      } else {
        if (v & 1) f.zio[0] = f.zwr[0] = d[0];
        if (v & 2) f.rio = f.rwr = NP;
        if (!v) f.empty = true;  // neither the vector nor the norm: nothing to write
      }
      break;
    case MITDVP_VECOP_AXPBY:
      f.zin[0] = f.zio[0] = f.zwr[0] = d[0]; f.empty = d[0] == 0;
      break;
    case MITDVP_VECOP_SCALE:
      f.zio[0] = f.zwr[0] = d[0]; f.empty = d[0] == 0;
      break;
    case MITDVP_VECOP_TRANSPOSE: {
      const long rows = d[0], cols = d[1], batch = d[2];
      if (batch > VECOP_MAX_BATCH) return "vecop: batch > 65535 for the transpose";
      f.empty = rows == 0 || cols == 0 || batch == 0; f.own_return = true;
      if (f.empty) break;
      if (rows > 1 && s[0] < cols) return lead;
      if (cols > 1 && s[1] < rows) return lead;
      const long ein = mat(rows, cols, s[0]), eout = mat(cols, rows, s[1]);
      if (batch > 1) {  // the batches of the destination lie one after the other, or interleaved inside a row stride
        const bool apart = s[3] >= eout;
        const bool inter = s[3] >= rows && (cols == 1 || s[1] >= add(mul(batch - 1, s[3]), rows));
        if (!apart && !inter) return "vecop: the batches of the transpose's destination overlap";
      }
      f.zin[0] = add(mul(batch - 1, s[2]), ein); f.zio[0] = f.zwr[0] = add(mul(batch - 1, s[3]), eout);
      break;
    }
    case MITDVP_VECOP_TRANSPOSE_REV3:
      if (d[1] > VECOP_MAX_BATCH) return "vecop: batch > 65535 for the transpose";
      f.zin[0] = f.zio[0] = f.zwr[0] = mul(mul(d[0], d[1]), d[2]); f.empty = f.zin[0] == 0; f.own_return = true;
      break;
    case MITDVP_VECOP_PERMUTE_0213:
      f.zin[0] = f.zio[0] = f.zwr[0] = mul(mul(d[0], d[1]), mul(d[2], d[3])); f.empty = f.zin[0] == 0; f.own_return = true;
      break;
    case MITDVP_VECOP_PERMUTE5: {
      const long tot = mul(mul(mul(d[0], d[1]), mul(d[2], d[3])), d[4]);
      f.empty = tot == 0; f.own_return = true;
      if (f.empty) break;
      long last2 = d[2] - 1;
      if (v & 1) {
        if (!idx || nidx < (size_t)d[2]) return noidx;
        f.idx = d[2]; last2 = 0;
        for (long k = 0; k < d[2]; ++k) {
          if (idx[k] < 0) return "vecop: a negative entry in map2";
          if (idx[k] > last2) last2 = idx[k];
        }
      }
      long e = 1;
      for (int k = 0; k < 5; ++k) e = add(e, mul(k == 2 ? last2 : d[k] - 1, s[k]));
      f.zin[0] = e; f.zio[0] = f.zwr[0] = tot;
      break;
    }
    case MITDVP_VECOP_PHYS_DIAG:
      f.zio[0] = f.zwr[0] = (v & 1) ? mul(d[0], d[2]) : mul(mul(d[0], d[1]), d[2]);
      f.zin[0] = mul(mul(d[0], d[1]), mul(d[1], d[2])); f.empty = f.zio[0] == 0; f.own_return = true;
      break;
    case MITDVP_VECOP_COPY2D: {
      const long w = d[2] > d[1] ? d[2] : d[1];
      f.empty = d[0] == 0 || w == 0; f.own_return = true;
      if (f.empty) break;
      if (d[0] > 1 && (s[0] < w || s[1] < d[1])) return lead;
      f.zin[0] = mat(d[0], d[1], s[1]); f.zio[0] = f.zwr[0] = mat(d[0], w, s[0]);
      break;
    }
    case MITDVP_VECOP_COPY_RAW:
      f.zin[0] = f.zio[0] = f.zwr[0] = d[0]; f.empty = d[0] == 0; f.own_return = true;
      break;
    case MITDVP_VECOP_IDENTITY:
      if (d[0] > 1 && s[0] < d[1]) return lead;
      f.zio[0] = f.zwr[0] = mat(d[0], d[1], s[0]); f.empty = f.zio[0] == 0;
      break;
    case MITDVP_VECOP_SCALE_COLS:
      if (d[0] > 1 && s[0] < d[1]) return lead;
      f.zio[0] = f.zwr[0] = mat(d[0], d[1], s[0]); f.rin = d[1]; f.empty = f.zio[0] == 0; f.own_return = true;
      break;
    case MITDVP_VECOP_GATHER_BLOCKS: {  // rows, cols, bl.n, n_dst, m_src
      if (d[2] > VECOP_MAX_BLOCKS) return toomany;
      if (d[3] < d[2]) return "vecop: n_dst < bl.n";
      if (!idx && d[2]) return noidx;
      if (nidx < (size_t)d[2]) return noidx;
      for (long k = 0; k < d[2]; ++k)
        if (idx[k] < 0 || idx[k] >= d[4]) return "vecop: a block index outside the source";
      f.idx = d[2]; f.empty = d[0] == 0 || d[1] == 0; f.own_return = true;  // bl.n = 0 is the wrapper's own return
      f.zin[0] = mul(mul(d[0], d[4]), d[1]); f.zio[0] = mul(mul(d[0], d[3]), d[1]);
      f.zwr[0] = d[2] ? add(mul(mul(d[0] - 1, d[3]), d[1]), mul(d[2], d[1])) : 0;
      if (f.empty) f.zwr[0] = 0;
      break;
    }
    case MITDVP_VECOP_FILL_SCALED_BLOCKS: {  // rows, cols, bl.n, pos0; ldx
      if (d[2] > VECOP_MAX_BLOCKS) return toomany;
      const long w = mul(add(d[3], d[2]), d[1]);
      f.empty = d[0] == 0 || d[1] == 0; f.own_return = true;
      if (f.empty) break;
      if (d[0] > 1 && s[0] < w) return lead;
      f.zin[0] = mul(d[0], d[1]); f.zio[0] = mat(d[0], w, s[0]); f.zwr[0] = d[2] ? f.zio[0] : 0;
      break;
    }
    case MITDVP_VECOP_ACCUM_SCALED_BLOCKS: {  // rows, cols, bl.n; ldx
      if (d[2] > VECOP_MAX_BLOCKS) return toomany;
      if (!idx && d[2]) return noidx;
      if (nidx < (size_t)d[2]) return noidx;
      long top = -1;
      for (long k = 0; k < d[2]; ++k) {
        if (idx[k] < 0) return "vecop: a block index outside the source";
        if (idx[k] > top) top = idx[k];
      }
      f.idx = d[2]; f.empty = d[0] == 0 || d[1] == 0; f.own_return = true;
      if (f.empty) break;
      const long w = mul(top + 1, d[1]);
      if (d[0] > 1 && s[0] < w) return lead;
      f.zin[0] = mat(d[0], w, s[0]); f.zin[1] = f.zio[0] = f.zwr[0] = mul(d[0], d[1]);
      break;
    }
    case MITDVP_VECOP_COL_SUMSQ:
      f.zin[0] = mul(d[0], d[1]); f.rio = f.rwr = d[1]; f.empty = f.zin[0] == 0;
      break;
    case MITDVP_VECOP_ROW_SUMSQ:
      f.zin[0] = mul(d[0], d[1]); f.rio = f.rwr = d[0]; f.empty = f.zin[0] == 0;
      break;
    case MITDVP_VECOP_SHELL_SUMSQ:
      f.zin[0] = mul(d[0], d[0]); f.rio = f.rwr = d[0]; f.empty = d[0] == 0;
      break;
    case MITDVP_VECOP_IDENT_DEV:
      if (d[0] > 1 && s[0] < d[0]) return lead;
      f.zin[0] = mat(d[0], d[0], s[0]); f.rio = f.rwr = 1; f.empty = d[0] == 0;
      break;
    default: {  // MITDVP_VECOP_IDENT_DEV_MULTI: n, nblk; ld, blk_stride
      if (d[1] > VECOP_MAX_BLOCKS) return toomany;
      if (d[0] > 1 && s[0] < d[0]) return lead;
      f.empty = d[0] == 0 || d[1] == 0;
      if (f.empty) break;
      f.zin[0] = add(mul(d[1] - 1, s[1]), mat(d[0], d[0], s[0])); f.rio = f.rwr = d[1]; f.zio[1] = f.zwr[1] = d[1];
      break;
    }
  }
  if (f.empty) {  // nothing is read or written
    VecopFoot e;
    e.empty = true; e.own_return = f.own_return;
    f = e;
  }
  if (foot) *foot = f;
  return nullptr;
}

// The descriptor of mitdvp_vecop and the caller's buffers, checked before any HIP call.  zin / zio count complex elements,
// rin / rio doubles, idx ints.  Every kernel takes its pointers as __restrict__: no source may overlap a destination, and
// the destinations may not overlap each other (the one sanctioned alias, x = vl of the one-workgroup step, is a variant).
inline const char* vecop_check(const mitdvp_vecop_args* a, const void* const zin[3], const size_t nzin[3], const void* rin, size_t nrin,
                               const int* idx, size_t nidx, const void* const zio[2], const size_t nzio[2], const void* rio,
                               size_t nrio, VecopFoot* foot) {
  using vecop_detail::overlap;
  VecopFoot f;
  if (const char* bad = vecop_shape_check(a, idx, nidx, &f)) return bad;
  static const char* const short_in[3] = {"vecop: complex input 0 is shorter than the operation's footprint",
                                          "vecop: complex input 1 is shorter than the operation's footprint",
                                          "vecop: complex input 2 is shorter than the operation's footprint"};
  static const char* const short_io[2] = {"vecop: complex result 0 is shorter than the operation's footprint",
                                          "vecop: complex result 1 is shorter than the operation's footprint"};
  for (int k = 0; k < 3; ++k)
    if (f.zin[k] && (!zin[k] || nzin[k] < f.zin[k])) return short_in[k];
  if (f.rin && (!rin || nrin < f.rin)) return "vecop: the real input is shorter than the operation's footprint";
  for (int k = 0; k < 2; ++k)
    if (f.zio[k] && (!zio[k] || nzio[k] < f.zio[k])) return short_io[k];
  if (f.rio && (!rio || nrio < f.rio)) return "vecop: the real result is shorter than the operation's footprint";
  const size_t z = 16, r = 8;
  const size_t cap = VECOP_MAX_BYTES;
  size_t total = 0;
  const size_t parts[8] = {nzin[0], nzin[1], nzin[2], nzio[0], nzio[1], (nrin + 1) / 2, (nrio + 1) / 2, (nidx + 3) / 4};
  for (size_t p : parts) {
    if (p > cap / z) return "vecop: more than 128 MB in one call";
    total += p * z;
  }
  if (total > cap) return "vecop: more than 128 MB in one call";
  const void* dst[3] = {f.zio[0] ? zio[0] : nullptr, f.zio[1] ? zio[1] : nullptr, f.rio ? rio : nullptr};
  const size_t dstb[3] = {nzio[0] * z, nzio[1] * z, nrio * r};
  const void* src[5] = {f.zin[0] ? zin[0] : nullptr, f.zin[1] ? zin[1] : nullptr, f.zin[2] ? zin[2] : nullptr, f.rin ? rin : nullptr,
                        f.idx ? idx : nullptr};
  const size_t srcb[5] = {nzin[0] * z, nzin[1] * z, nzin[2] * z, nrin * r, nidx * sizeof(int)};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 5; ++j)
      if (overlap(dst[i], dstb[i], src[j], srcb[j])) return "vecop: a source overlaps a destination";
    for (int j = i + 1; j < 3; ++j)
      if (overlap(dst[i], dstb[i], dst[j], dstb[j])) return "vecop: two destinations overlap";
  }
  if (foot) *foot = f;
  return nullptr;
}

}  // namespace mitdvp
