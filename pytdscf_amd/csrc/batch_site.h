// batch_site.h -- batched trajectories (batch_site.hip): ONE workgroup owns one replica's whole chain and walks a
// half-sweep of it inside one launch; the replica index is blockIdx.x, so any number of replicas runs in one grid.
#pragma once
#include <string>

#include "common.h"
#include "small_site.h"

namespace mitdvp {

// shapes of one site of the chain (identical across the replicas of a batch)
struct BatchShape {
  int dl, d, dr;  // site tensor (dl, d, dr)
  int ml, mr;     // MPO core (ml, d, d, mr)
};

// Qualifying envelope of k_batch_sweep, decided on the host (the twin of small_chain_plan for this kernel):
//   * dl * d * dr <= BATCH_MAX_SITE elements per site tensor (the kernel keeps nothing of that size in LDS, so the
//     bound is one of scratch memory and time per replica rather than of the hardware: 4096 is d = 4, D = 32),
//   * MPO bonds ml, mr <= BATCH_MAX_MPO,
//   * bonds dl, dr <= BATCH_MAX_BOND (the Householder scalars of a gauge move live in LDS),
//   * dl * d >= dr and d * dr >= dl (a thin QR needs at least as many rows as columns; the sweep requires the same).
constexpr long BATCH_MAX_SITE = 8192;
constexpr int BATCH_MAX_MPO = 16;
constexpr int BATCH_MAX_BOND = 64;

struct BatchPlan {
  long max_site = 1;  // largest site tensor, elements
  long max_bond = 1;  // largest bond matrix, elements
  long nx = 1, ny = 1;  // largest M-fold intermediates X, Y of an apply or environment update, elements
  // per-replica scratch carve, offsets in complex elements
  size_t o_sig = 0, o_spare = 0, o_work = 0, o_x = 0, o_y = 0, o_u = 0, total = 0;
};
// false + a message naming the offending site and the limit when the chain is outside the envelope
bool batch_plan(const BatchShape* shp, int L, BatchPlan& plan, std::string& why);

struct BatchArgs {
  int L, forward;
  const BatchShape* shp;    // [L], device
  // per-replica pointer table, ptr_stride = 6 L + 3 entries each: [site tensors L][left blocks L + 1, bond b left of
  // site b][right blocks L + 1][MpoSite::w2l L (H_eff W stage)][w2el L (environment update ->)][w2er L (<-)]
  // [scratch 1: sigma, spare tensor, QR work matrix, X, Y, Krylov basis -- the BatchPlan carve]
  void* const* ptrs;
  int ptr_stride;
  const zc* shift;          // [B] scalar term of each replica's operator
  int* kprev;               // [B * L] Krylov memory per site (site and bond exponential of site p share kprev[p])
  int* status;              // [B] SS_OK / SS_ENOTCONV / SS_EZERO; a replica whose word is set does no more work
  long long* stats;         // [B * 4] applies inside site / bond exponentials, and their flops
  BatchPlan plan;
  SmallExp e;               // integrator, variant, conserve_norm, max_krylov, thresh (scale / site / slot set per solve)
  double site_re, site_im, bond_re, bond_im;  // scale of the site / bond exponentials
};

// one launch: grid = nrep workgroups, a half-sweep of every replica
void batch_sweep_launch(hipStream_t st, const BatchArgs& a, int nrep);

}  // namespace mitdvp
