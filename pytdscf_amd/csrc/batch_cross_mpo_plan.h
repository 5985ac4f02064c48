// batch_cross_mpo_plan.h -- the host side of the MPO matrix elements between replicas (k_batch_cross_mpo, batch_site.hip)
// that needs no HIP: the check of a request's entries, the carve of the request's buffer and its cap.  Nothing here
// includes a HIP header, so that a test can compile it with a plain C++ compiler (tests/helpers/cross_mpo_plan_shim.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>

#include "batch_shape.h"

namespace mitdvp {

constexpr unsigned long long BATCH_CROSS_MPO_MAX_BYTES = 1ull << 32;  // the request's buffer, entries x carve x 16 bytes
struct BatchCrossMpoEntry {
  int bra, ket;  // state indices: 0 .. B-1 a replica, B + r the snapshot of replica r
  int op;        // index into the request's list of distinct operators
  int pad;
};
// One entry's carve of the request's buffer, offsets in complex elements: the two left blocks the walk writes alternately
// (T0 at 0, T1 at o_e1: the largest chi_q m_q chi_q over the bonds each) and X, Y of the update (the largest n ml / n mr
// over the sites, n = dl d dr).  The maxima run over all listed operators: every entry has the same carve.  The overlap
// walk of the scalar term lives in the same carve (its T and successor in the blocks, its U in X).
struct BatchCrossMpoPlan {
  size_t o_e1 = 0, o_x = 0, o_y = 0, total = 0;
};

// The entries of a request against the batch: false + a message naming the entry and the limit for more than
// BATCH_CROSS_MAX_PAIRS entries, an index outside 0 .. 2B-1, a snapshot index while there is no snapshot, a negative
// op_id.  B: the number of replicas.
inline bool batch_cross_mpo_entries_ok(int B, bool has_snap, int nentries, const int* bra, const int* ket, const int* op_id,
                                       std::string& why) {
  if (nentries < 0) { why = "nentries must be >= 0"; return false; }
  if (nentries > BATCH_CROSS_MAX_PAIRS) {
    why = std::to_string(nentries) + " entries, a request takes at most " + std::to_string(BATCH_CROSS_MAX_PAIRS);
    return false;
  }
  if (nentries > 0 && (!bra || !ket || !op_id)) { why = "null list of bra, ket or operator indices"; return false; }
  for (int q = 0; q < nentries; ++q) {
    const std::string who = "entry " + std::to_string(q) + ": ";
    const int idx[2] = {bra[q], ket[q]};
    for (int k = 0; k < 2; ++k) {
      const std::string name = std::string(k ? "ket" : "bra") + " index " + std::to_string(idx[k]);
      if (idx[k] < 0 || idx[k] >= 2 * B) {
        why = who + name + " is outside 0 .. " + std::to_string(2 * B - 1) + " (the batch has " + std::to_string(B) + " replicas; " +
              std::to_string(B) + " + r names the snapshot of replica r)";
        return false;
      }
      if (idx[k] >= B && !has_snap) {
        why = who + name + " names the snapshot of replica " + std::to_string(idx[k] - B) +
              ", and no snapshot was taken yet (mitdvp_batch_snapshot)";
        return false;
      }
    }
    if (op_id[q] < 0) {
      why = who + "operator " + std::to_string(op_id[q]) + " is negative (operator ids are >= 0)";
      return false;
    }
  }
  return true;
}

// shp: [nops][L], the site shapes with operator k's MPO bonds; op_ids: [nops], the names of the operators.  false + a
// message naming the operator, the site and the limit when an MPO bond is outside 1 .. BATCH_MAX_MPO, the bonds of
// neighbouring cores differ or the outer ones are not 1: the conditions of batch_expect_plan, for the forward roles.
inline bool batch_cross_mpo_plan(const BatchShape* shp, const int* op_ids, int L, int nops, BatchCrossMpoPlan& plan, std::string& why) {
  plan = BatchCrossMpoPlan{};
  size_t ne = 1, nx = 1, ny = 1;
  for (int k = 0; k < nops; ++k) {
    const BatchShape* s = shp + (size_t)k * L;
    for (int p = 0; p < L; ++p) {
      const std::string at = "operator " + std::to_string(op_ids[k]) + ", site " + std::to_string(p) + ": MPO bonds (" +
                             std::to_string(s[p].ml) + ", " + std::to_string(s[p].mr) + "): ";
      if (s[p].ml < 1 || s[p].mr < 1 || s[p].ml > BATCH_MAX_MPO || s[p].mr > BATCH_MAX_MPO) {
        why = at + "the batched kernel takes MPO bonds of 1 to " + std::to_string(BATCH_MAX_MPO);
        return false;
      }
      if (p + 1 < L && s[p].mr != s[p + 1].ml) {
        why = at + "the core of site " + std::to_string(p + 1) + " has the left MPO bond " + std::to_string(s[p + 1].ml);
        return false;
      }
      // the update of the left block: X (d dr) x (ml dl), Y dr x (mr d) x dl, T (dr, mr, dr)
      const size_t n = (size_t)s[p].dl * s[p].d * s[p].dr;
      nx = std::max(nx, n * s[p].ml);
      ny = std::max(ny, n * s[p].mr);
      ne = std::max(ne, (size_t)s[p].dr * s[p].mr * s[p].dr);
    }
    if (s[0].ml != 1 || s[L - 1].mr != 1) {
      why = "operator " + std::to_string(op_ids[k]) + ": the outer MPO bonds are (" + std::to_string(s[0].ml) + ", " +
            std::to_string(s[L - 1].mr) + "), they must be 1";
      return false;
    }
  }
  size_t o = 0;
  o += ne;
  plan.o_e1 = o; o += ne;
  plan.o_x = o; o += nx;
  plan.o_y = o; o += ny;
  plan.total = (o + 15) / 16 * 16;
  return true;
}

// false + a message with the figure and the largest number of entries that fits when nentries x plan.total x 16 bytes
// exceeds BATCH_CROSS_MPO_MAX_BYTES
inline bool batch_cross_mpo_fits(size_t nentries, const BatchCrossMpoPlan& plan, std::string& why) {
  const unsigned long long per = (unsigned long long)plan.total * 16ull;
  const unsigned long long fit = per ? BATCH_CROSS_MPO_MAX_BYTES / per : 0;
  if ((unsigned long long)nentries <= fit) return true;
  why = std::to_string(nentries) + " entries of " + std::to_string(per) + " bytes each need a buffer of " +
        std::to_string((unsigned long long)nentries * per) + " bytes, the limit is " + std::to_string(BATCH_CROSS_MPO_MAX_BYTES) +
        " bytes: at most " + std::to_string(fit) + " entries fit";
  return false;
}

}  // namespace mitdvp
