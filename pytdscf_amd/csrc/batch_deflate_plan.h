// batch_deflate_plan.h -- the host side of the deflation set of a batch (excited states by the penalty method,
// k_batch_relax_defl / k_batch_defl_overlaps in batch_site.hip) that needs no HIP: the number of slots, the check of the
// weights and the size of the kernel's work buffer.  Nothing here includes a HIP header, so that a test can compile it
// with a plain C++ compiler (tests/helpers/deflate_plan_shim.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <string>

#include "batch_shape.h"

namespace mitdvp {

// Stored states one batch keeps: each slot is a copy of every replica's site tensors and one weight per replica.  The
// rank-one terms of a local solve are reduced four slots at a time (two doubles per slot in the eight of the workgroup
// reduction), so eight slots are two rounds per apply.
constexpr int BATCH_MAX_DEFLATE = 8;
// the kernel's work buffer, all replicas together
constexpr unsigned long long BATCH_DEFLATE_MAX_BYTES = 1ull << 32;

// false + a message naming the count and the limit when the set is full
inline bool batch_deflate_room(int count, std::string& why) {
  if (count >= 0 && count < BATCH_MAX_DEFLATE) return true;
  why = "the set holds " + std::to_string(count) + " states, a batch keeps at most " + std::to_string(BATCH_MAX_DEFLATE);
  return false;
}

// false + a message naming the replica and its weight when one of the n weights is not finite or not > 0, or the list
// is null.  The penalty is w |<phi|psi>|^2: a weight that is zero or negative does not push a state up.
inline bool batch_deflate_weights_ok(const double* weights, int n, std::string& why) {
  if (!weights) {
    why = "weights is NULL, the call takes one weight per replica";
    return false;
  }
  for (int r = 0; r < n; ++r)
    if (!std::isfinite(weights[r]) || !(weights[r] > 0.0)) {
      why = "replica " + std::to_string(r) + " has weight " + std::to_string(weights[r]) + ", a weight must be finite and > 0";
      return false;
    }
  return true;
}

// A replica's part of the work buffer, complex elements, for `slots` stored states:
//   per slot the overlap blocks at their actual bond sizes, one (dl_p x dl_p) block per bond left of site p, p = 0 .. L-1
//   (the block of bond p is the left block while the centre is at or right of site p and the right block otherwise; the
//   1 x 1 blocks of the two ends are both the number 1 and share element 0);
//   then per slot one projected vector q_k as long as the largest site tensor.
struct BatchDeflatePlan {
  size_t blk_len = 0;  // sum_p dl_p^2
  size_t max_site = 0; // max_p dl_p d_p dr_p
  size_t o_q = 0;      // where the projected vectors start: slots * blk_len
  size_t per = 0;      // slots * (blk_len + max_site)
};
inline BatchDeflatePlan batch_deflate_plan(const BatchShape* shp, int L, int slots) {
  BatchDeflatePlan pl;
  for (int p = 0; p < L; ++p) {
    pl.blk_len += (size_t)shp[p].dl * shp[p].dl;
    const size_t n = (size_t)shp[p].dl * shp[p].d * shp[p].dr;
    if (n > pl.max_site) pl.max_site = n;
  }
  pl.o_q = (size_t)slots * pl.blk_len;
  pl.per = (size_t)slots * (pl.blk_len + pl.max_site);
  return pl;
}

// false + a message naming both figures and the largest number of slots that fits when nrep replicas with `slots` stored
// states need a work buffer above BATCH_DEFLATE_MAX_BYTES
inline bool batch_deflate_fits(const BatchShape* shp, int L, int slots, size_t nrep, std::string& why) {
  const BatchDeflatePlan one = batch_deflate_plan(shp, L, 1);
  const unsigned long long per_slot = 16ull * one.per * nrep;  // bytes one slot adds, all replicas together
  const unsigned long long need = per_slot * (unsigned long long)slots;
  if (need <= BATCH_DEFLATE_MAX_BYTES) return true;
  const unsigned long long most = per_slot ? BATCH_DEFLATE_MAX_BYTES / per_slot : (unsigned long long)BATCH_MAX_DEFLATE;
  why = "the work buffer of " + std::to_string(slots) + " stored states takes " + std::to_string(need) + " bytes (" +
        std::to_string(nrep) + " replicas x " + std::to_string(slots) + " x " + std::to_string(one.per) +
        " elements x 16), the limit is " + std::to_string(BATCH_DEFLATE_MAX_BYTES) + ": at most " + std::to_string(most) +
        " states fit";
  return false;
}

}  // namespace mitdvp
