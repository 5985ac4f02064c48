// batch_operate_plan.h -- the host side of the batched operator application (k_batch_operate, batch_site.hip) that needs
// no HIP: the carve of the request's buffer, the checks of the operator's bonds and the buffer's cap.  Nothing here
// includes a HIP header, so that a test can compile it with a plain C++ compiler (tests/helpers/operate_plan_shim.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "batch_shape.h"

namespace mitdvp {

constexpr unsigned long long BATCH_OPERATE_MAX_BYTES = 1ull << 32;  // the request's buffer, selected replicas x carve x 16 bytes

// One selected replica's carve of the request's buffer, offsets in complex elements.  Everything of tensor size that the
// fit needs besides the replica's own site tensors (which hold the bra, phi) lies here:
//   ket   the copy of the replica's tensors the operator is applied to, site after site: site p at o_ket + site[p]
//   prev  phi as it was before the double sweep in progress, the same layout at o_prev
//   mix   the L + 1 mixed blocks (bra bond, MPO bond, ket bond) at their true sizes: block b at o_mix + mix[b], b = 0 and
//         b = L the 1 x 1 x 1 boundaries; block b is the LEFT block while the centre is at a site >= b, the RIGHT block
//         otherwise -- a half-sweep overwrites a block exactly when its other role is spent
//   ov    the L + 1 overlap blocks (bra bond, ket bond) of the scalar term, block b at o_ov + ov[b]
//   x, y  the two intermediates of an apply or a block update (the largest n max(ml, mr), n = dl d dr, each)
//   work  the QR work matrix, spare the target of an absorb, h the overlap-block apply of the scalar term (largest n each)
//   sig   the R factor of a gauge move, t0 / t1 the transfer matrices of the convergence overlap (largest bond squared)
//   id    the d x d identity, the core of the scalar term's bond-1 operator (largest d squared)
struct BatchOperatePlan {
  size_t o_ket = 0, o_prev = 0, o_mix = 0, o_ov = 0, o_x = 0, o_y = 0, o_work = 0, o_spare = 0, o_h = 0, o_sig = 0, o_t0 = 0,
         o_t1 = 0, o_id = 0, total = 0;
  std::vector<long long> site, mix, ov;  // [L + 1] prefix sums: the last entry is the length of the region
};

// shp: [L], the site shapes with the operator's MPO bonds.  false + a message naming the operator, the site and the limit
// when an MPO bond is outside 1 .. BATCH_MAX_MPO, the bonds of neighbouring cores differ or the outer ones are not 1.
inline bool batch_operate_plan(const BatchShape* shp, int op_id, int L, BatchOperatePlan& plan, std::string& why) {
  plan = BatchOperatePlan{};
  const std::string op = "operator " + std::to_string(op_id);
  size_t nmax = 1, nxy = 1, nb = 1, nd = 1;
  plan.site.assign((size_t)L + 1, 0);
  plan.mix.assign((size_t)L + 1, 0);
  plan.ov.assign((size_t)L + 1, 0);
  for (int p = 0; p < L; ++p) {
    const BatchShape& s = shp[p];
    const std::string at = op + ", site " + std::to_string(p) + ": MPO bonds (" + std::to_string(s.ml) + ", " + std::to_string(s.mr) + "): ";
    if (s.ml < 1 || s.mr < 1 || s.ml > BATCH_MAX_MPO || s.mr > BATCH_MAX_MPO) {
      why = at + "the batched kernel takes MPO bonds of 1 to " + std::to_string(BATCH_MAX_MPO);
      return false;
    }
    if (p + 1 < L && s.mr != shp[p + 1].ml) {
      why = at + "the core of site " + std::to_string(p + 1) + " has the left MPO bond " + std::to_string(shp[p + 1].ml);
      return false;
    }
    const size_t n = (size_t)s.dl * s.d * s.dr;
    nmax = std::max(nmax, n);
    nxy = std::max(nxy, n * (size_t)std::max(s.ml, s.mr));
    nb = std::max(nb, std::max((size_t)s.dl * s.dl, (size_t)s.dr * s.dr));
    nd = std::max(nd, (size_t)s.d * s.d);
    plan.site[p + 1] = plan.site[p] + (long long)n;
    // block p is left of site p: (dl, ml, dl); block L is the right boundary, 1 x 1 x 1
    plan.mix[p + 1] = plan.mix[p] + (long long)s.dl * s.ml * s.dl;
    plan.ov[p + 1] = plan.ov[p] + (long long)s.dl * s.dl;
  }
  if (shp[0].ml != 1 || shp[L - 1].mr != 1) {
    why = op + ": the outer MPO bonds are (" + std::to_string(shp[0].ml) + ", " + std::to_string(shp[L - 1].mr) + "), they must be 1";
    return false;
  }
  const size_t nsite = (size_t)plan.site[L], nmix = (size_t)plan.mix[L] + 1, nov = (size_t)plan.ov[L] + 1;
  size_t o = 0;
  plan.o_ket = o; o += nsite;
  plan.o_prev = o; o += nsite;
  plan.o_mix = o; o += nmix;
  plan.o_ov = o; o += nov;
  plan.o_x = o; o += nxy;
  plan.o_y = o; o += nxy;
  plan.o_work = o; o += nmax;
  plan.o_spare = o; o += nmax;
  plan.o_h = o; o += nmax;
  plan.o_sig = o; o += nb;
  plan.o_t0 = o; o += nb;
  plan.o_t1 = o; o += nb;
  plan.o_id = o; o += nd;
  plan.total = (o + 15) / 16 * 16;
  return true;
}

// false + a message with both figures and the largest number of replicas that fits when nsel x plan.total x 16 bytes
// exceeds BATCH_OPERATE_MAX_BYTES
inline bool batch_operate_fits(size_t nsel, const BatchOperatePlan& plan, std::string& why) {
  const unsigned long long per = (unsigned long long)plan.total * 16ull;
  const unsigned long long fit = per ? BATCH_OPERATE_MAX_BYTES / per : 0;
  if ((unsigned long long)nsel <= fit) return true;
  why = std::to_string(nsel) + " replicas of " + std::to_string(per) + " bytes each need a buffer of " +
        std::to_string((unsigned long long)nsel * per) + " bytes, the limit is " + std::to_string(BATCH_OPERATE_MAX_BYTES) +
        " bytes: at most " + std::to_string(fit) + " replicas fit in one call";
  return false;
}

}  // namespace mitdvp
