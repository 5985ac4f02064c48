// batch_relax_plan.h -- the host side of the batched improved relaxation (k_batch_relax, batch_site.hip) that needs no
// HIP: the cap of the Lanczos eigen-solver's Krylov space, the range of its restarts and the size of a replica's
// Krylov-basis carve.  Nothing here includes a HIP header, so that a test can compile it with a plain C++ compiler
// (tests/helpers/relax_plan_shim.cpp, relax_restart_shim.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>

namespace mitdvp {

// Krylov vectors of one local eigen-solve (bt_diag): one lane of a wave per row of the projected tridiagonal matrix
constexpr int BATCH_RELAX_MAX_KRYLOV = 64;
constexpr int BATCH_EXP_KRYLOV_SLOTS = 21;  // MAXK (vecops.h), the slots the exponential's basis takes

// Config::max_diag_krylov as the engine reads it: 0 (or less) means 64
inline int batch_relax_kcap_of(int max_diag_krylov) { return max_diag_krylov > 0 ? max_diag_krylov : BATCH_RELAX_MAX_KRYLOV; }

// false + a message naming the value and the limit when the cap is outside 2 .. BATCH_RELAX_MAX_KRYLOV
inline bool batch_relax_kcap_ok(int max_diag_krylov, std::string& why) {
  const int k = batch_relax_kcap_of(max_diag_krylov);
  if (k >= 2 && k <= BATCH_RELAX_MAX_KRYLOV) return true;
  why = "max_diag_krylov = " + std::to_string(k) + ", the batched improved relaxation takes 2 to " +
        std::to_string(BATCH_RELAX_MAX_KRYLOV) + " (one lane of a wave per row of the projected matrix)";
  return false;
}

// Thick restarts one local solve may take (BatchRelaxArgs::max_restarts): after min(N, max_diag_krylov) vectors without
// convergence the basis is folded into its lowest Ritz vector and the next Lanczos vector, and the solve goes on.  0: none.
constexpr int BATCH_RELAX_MAX_RESTARTS = 4096;

// false + a message naming the value and the range when max_restarts is outside 0 .. BATCH_RELAX_MAX_RESTARTS
inline bool batch_relax_restarts_ok(int max_restarts, std::string& why) {
  if (max_restarts >= 0 && max_restarts <= BATCH_RELAX_MAX_RESTARTS) return true;
  why = "max_restarts = " + std::to_string(max_restarts) + ", the batched improved relaxation takes 0 to " +
        std::to_string(BATCH_RELAX_MAX_RESTARTS) + " restarts of a local solve";
  return false;
}

// Complex elements of a replica's Krylov-basis carve (BatchPlan::o_u .. total).  relax 0 / 1: the MAXK slots of the local
// exponential, as ever.  relax 2: the eigen-solver keeps kcap + 1 vectors of a site tensor, kcap = min(N, max_diag_krylov)
// at a site of N elements, so min(max_site, max_diag_krylov) + 1 slots bound every site.  A slot is as long as the largest
// site tensor or bond matrix (the pair channels park the two-site tensor in the same carve).
inline size_t batch_krylov_carve(long max_site, long max_bond, int relax, int max_diag_krylov) {
  const size_t slot = (size_t)std::max(max_site, max_bond);
  if (relax != 2) return (size_t)BATCH_EXP_KRYLOV_SLOTS * slot;
  const long kcap = std::min<long>(max_site, batch_relax_kcap_of(max_diag_krylov));
  return (size_t)(kcap + 1) * slot;
}

}  // namespace mitdvp
