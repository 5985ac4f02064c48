// batch_shape.h -- the shapes and limits of the batched trajectories that the host-side plans share (batch_site.h).
// Nothing here includes a HIP header, so that a test can compile the plans with a plain C++ compiler.
#pragma once

namespace mitdvp {

// shapes of one site of the chain (identical across the replicas of a batch)
struct BatchShape {
  int dl, d, dr;  // site tensor (dl, d, dr)
  int ml, mr;     // MPO core (ml, d, d, mr)
};

// the envelope of k_batch_sweep (batch_site.h has the reasons)
constexpr long BATCH_MAX_SITE = 8192;
constexpr int BATCH_MAX_MPO = 16;
constexpr int BATCH_MAX_BOND = 64;
// pairs of one cross request (k_batch_cross), entries of one cross request of MPOs (k_batch_cross_mpo)
constexpr int BATCH_CROSS_MAX_PAIRS = 65536;
// rows and columns of the two-site tensor of a pair channel (k_batch_pair; batch_site.h has the reasons)
constexpr int BATCH_PAIR_MAX_DIM = 128;

}  // namespace mitdvp
