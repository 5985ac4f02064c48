// Throw-away C shim over csrc/small_chain_plan.h for tests/test_small_plan_host.py (compiled with g++, no HIP).
// -DSSP_HEADER='"path"' compiles it over another copy of the header (the test's deliberately broken planners).
#ifndef SSP_HEADER
#define SSP_HEADER "../../pytdscf_amd/csrc/small_chain_plan.h"
#endif
#include SSP_HEADER

using namespace mitdvp;

namespace {
// what the planner and the carve read of a chain: the extents, "is there a W stage", the plan
struct ShimChain {
  const void* W2 = nullptr;
  int na = 0, nb = 0, nc = 0, nj = 0, ni = 0, nt = 0, ns = 0, nr = 0;
  int nsc = 0, cs = 0, spw = 0, a_resident = 0;
};
const int w_stage = 0;

// kind 0 H_eff (dl, d, dr, ml, mr), 1 K_eff (d1, d2, m), 2 env update (din, min, d, dout, mout)
bool chain_of(ShimChain& c, int kind, const int* q) {
  c = ShimChain{};
  if (kind == 0) { small_extents_heff(c, q[0], q[1], q[2], q[3], q[4]); c.W2 = &w_stage; }
  else if (kind == 1) small_extents_keff(c, q[0], q[1], q[2]);
  else if (kind == 2) { small_extents_env(c, q[0], q[1], q[2], q[3], q[4]); c.W2 = &w_stage; }
  else return false;
  return true;
}
}  // namespace

extern "C" {
// consts[6]: SS_MAXG, SS_THREADS, SS_WAVES, SS_PAYMAX, MAXK, SS_LDS_PLAN
void ssp_consts(int* out) {
  out[0] = SS_MAXG; out[1] = SS_THREADS; out[2] = SS_WAVES; out[3] = SS_PAYMAX; out[4] = MAXK; out[5] = SS_LDS_PLAN;
}
// ext[8]: na nb nc nj ni nt ns nr
int ssp_extents(int kind, const int* dims, int* ext) {
  ShimChain c;
  if (!chain_of(c, kind, dims)) return -1;
  const int e[8] = {c.na, c.nb, c.nc, c.nj, c.ni, c.nt, c.ns, c.nr};
  for (int k = 0; k < 8; ++k) ext[k] = e[k];
  return c.W2 ? 1 : 0;
}
// plan[4]: nsc cs spw a_resident; returns 1 planned, 0 refused, -1 bad kind
int ssp_plan(int kind, const int* dims, int exp_mode, int n_cu, int* plan) {
  ShimChain c;
  if (!chain_of(c, kind, dims)) return -1;
  const bool ok = small_chain_plan_of(c, exp_mode != 0, n_cu);
  plan[0] = c.nsc; plan[1] = c.cs; plan[2] = c.spw; plan[3] = c.a_resident;
  return ok ? 1 : 0;
}
// the carve of a chain under a GIVEN plan; off[9]: As Rs Ws Bs Xs Ys Sg misc total (complex elements)
int ssp_carve(int kind, const int* dims, int exp_mode, const int* plan, unsigned long long* off) {
  ShimChain c;
  if (!chain_of(c, kind, dims)) return -1;
  c.nsc = plan[0]; c.cs = plan[1]; c.spw = plan[2]; c.a_resident = plan[3];
  const Carve k = ss_carve(c, exp_mode != 0);
  const size_t o[9] = {k.As, k.Rs, k.Ws, k.Bs, k.Xs, k.Ys, k.Sg, k.misc, k.total};
  for (int i = 0; i < 9; ++i) off[i] = o[i];
  return 0;
}
}
