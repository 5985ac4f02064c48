// small_chain_plan.h -- the part of the small-bond kernel family (k_small_site, small_site.hip) that is plain integer
// arithmetic: the extents of the three contraction chains, the LDS carve of a workgroup and the launch plan (chunks over
// the contracted index, slabs per workgroup, resident or re-staged A).  The kernel carves its LDS with ss_carve, the host
// sizes the launch and picks the plan with the same function.  Nothing here includes a HIP header or names a HIP type, so
// that a test can compile it with a plain C++ compiler (tests/helpers/small_plan_shim.cpp): the functions are templates
// over the chain record, of which they read the extents, W2 (as "is there a W stage") and the plan fields.
#pragma once
#include <algorithm>
#include <cstddef>

#if defined(__HIPCC__)
#define SS_PLAN_HD __host__ __device__
#else
#define SS_PLAN_HD
#endif

namespace mitdvp {

constexpr int MAXK = 21;  // Krylov vectors kept: ndim (<= 20) + 1

// Threads per workgroup.  Rounds 2-4 ran 1024 (16 waves: "four per SIMD hide the LDS / L2 latencies of the short dependent
// chains") -- at a register budget of 128 per thread, which this kernel exceeds: 125 VGPRs spilled, 380 B of scratch per
// lane (hipcc -Rpass-analysis=kernel-resource-usage).  With 512 threads (8 waves, 256 registers each: 233 used, no scratch)
// the same code runs C2 at 237 instead of 208 sweeps/s and the ensembles at 468 / 806 / 882 / 1134 instead of 407 / 693 /
// 782 / 995 (2 / 4 / 8 / 16 replicas, same box: profiles/r05_ss_threads_ab.txt).  make variantf DEFS=-DMITDVP_SS_THREADS=1024
// builds the old form for A/B runs.
#ifndef MITDVP_SS_THREADS
#define MITDVP_SS_THREADS 512
#endif
constexpr int SS_THREADS = MITDVP_SS_THREADS;
static_assert(SS_THREADS == 1024 || SS_THREADS == 512, "small-site workgroups have 16 or 8 waves");
constexpr int SS_WAVES = SS_THREADS / 64;
constexpr int SS_PAYMAX = 2 * MAXK + 2;  // doubles one workgroup contributes to an exchange
constexpr int SS_MAXG = 256;             // workgroups of one persistent launch at the most
constexpr int SS_LDS_PLAN = 155 * 1024;  // bytes of LDS a plan may take

// The extents of the three chains (small_site.h: out[a][i][r] = sum A(a;c,b) B(b,j,s) W2[(i,t)][(c,j)] R(r,t,s)); the
// engine adds the operand views (Engine::chain_heff / chain_keff / chain_env).
// H_eff  sigma[a,i,r] = sum L[a,c,b] W[c,i,j,t] R[r,t,s] psi[b,j,s]
template <class Chain>
inline void small_extents_heff(Chain& c, int dl, int d, int dr, int ml, int mr) {
  c.na = dl; c.nb = dl; c.nc = ml; c.nj = d; c.ni = d; c.nt = mr; c.ns = dr; c.nr = dr;
}
// K_eff  sigma'[a,r] = sum L[a,c,b] sigma[b,s] R[r,c,s]   (no W stage)
template <class Chain>
inline void small_extents_keff(Chain& c, int d1, int d2, int m) {
  c.na = d1; c.nb = d1; c.nc = m; c.nj = 1; c.ni = 1; c.nt = m; c.ns = d2; c.nr = d2;
}
// environment update  env'[i,q,j] = sum conj(T)[m,r,i] env[m,p,n] W2[(r,q),(p,s)] T[n,s,j]
template <class Chain>
inline void small_extents_env(Chain& c, int din, int min_, int d, int dout, int mout) {
  c.na = dout; c.nb = din; c.nc = d; c.nj = min_; c.ni = mout; c.nt = d; c.ns = din; c.nr = dout;
}

// LDS carve (units: 16-byte complex elements unless noted); the same arithmetic runs on the host in small_chain_lds
struct Carve {
  size_t As, Rs, Ws, Bs, Xs, Ys, Sg, misc, total;  // offsets in complex elements
};
template <class Chain>
SS_PLAN_HD inline Carve ss_carve(const Chain& c, bool exp_mode) {
  Carve k{};
  size_t o = 0;
  // A_a of the workgroup's slabs: all of them when they fit (a_resident), else one slot re-staged per slab
  k.As = o; o += (size_t)c.nc * c.nb * (c.a_resident && c.spw > 1 ? c.spw : 1);
  k.Rs = o; o += (size_t)c.nt * c.cs * c.nr;
  k.Ws = o; o += c.W2 ? (size_t)c.ni * c.nt * c.nc * c.nj : 0;
  k.Bs = o;
  size_t bs = (size_t)c.nb * c.nj * c.cs;
  if (exp_mode) bs = bs > (size_t)6 * MAXK * MAXK ? bs : (size_t)6 * MAXK * MAXK;  // also the k x k exponential's scratch
  o += bs;
  k.Xs = o; o += (size_t)c.nc * c.nj * c.cs;
  k.Ys = o; o += c.W2 ? (size_t)c.ni * c.nt * c.cs : 0;
  // this chunk's partial of the output slab; with a W stage it may reuse X's space (stage 3 reads Y and R only)
  if (c.W2 && (size_t)c.ni * c.nr <= (size_t)c.nc * c.nj * c.cs) k.Sg = k.Xs;
  else { k.Sg = o; o += (size_t)c.ni * c.nr; }
  k.misc = o;
  // misc: pay[SS_PAYMAX] red[SS_PAYMAX] wsh[SS_WAVES*SS_PAYMAX] (doubles) + alpha[MAXK] coef[MAXK] cprev[MAXK] (zc)
  //       + hess[(MAXK+1)*MAXK] (zc) + beta[MAXK] invb[MAXK+1] (doubles) + ints
  o += (size_t)((2 + SS_WAVES) * SS_PAYMAX + 1) / 2 + 3 * MAXK + (size_t)(MAXK + 1) * MAXK + (2 * MAXK + 2) / 2 + 8;
  k.total = o;
  return k;
}

// LDS bytes the chain needs under its plan fields
template <class Chain>
inline size_t small_chain_lds_of(const Chain& c, bool exp_mode) { return ss_carve(c, exp_mode).total * 16; }

// choose nsc / cs / spw / a_resident for a chain whose extents are set; false when the chain does not qualify
template <class Chain>
inline bool small_chain_plan_of(Chain& c, bool exp_mode, int n_cu) {
  if (c.na < 1 || c.ns < 1 || c.nr < 1 || c.nb < 1) return false;
  const int gmax = std::min(n_cu, SS_MAXG);
  c.spw = 1;
  c.a_resident = 1;
  // chunks over s: enough workgroups that one holds about 0.4 Mflop of the chain (beyond that the exchanges
  // between workgroups, not the arithmetic, set the pace), at least 4 columns per chunk, LDS permitting
  const double flops = 8.0 * c.na * ((double)c.nc * c.nb * c.nj * c.ns + (c.W2 ? (double)c.ni * c.nt * c.nc * c.nj * c.ns : 0.0) +
                                     (double)c.ni * c.nt * c.ns * c.nr);
  int want = 1;
  while (want < 8 && flops / ((double)c.na * want) > 0.6e6) want *= 2;
  if (c.na <= gmax) {
    for (int nsc = want; nsc <= 8; nsc *= 2) {
      if (c.na * nsc > gmax) break;
      const int cs = (c.ns + nsc - 1) / nsc;
      if (nsc > 1 && cs < 4) break;
      if ((nsc - 1) * cs >= c.ns) continue;  // every chunk must be non-empty
      c.nsc = nsc;
      c.cs = cs;
      if (small_chain_lds_of(c, exp_mode) <= (size_t)SS_LDS_PLAN) return true;
    }
    // fewer chunks than wanted: an engine confined to part of the chip (ensemble mode) has fewer compute units than the
    // chain would like workgroups
    for (int nsc = want / 2; nsc >= 1; nsc /= 2) {
      if (c.na * nsc > gmax) continue;
      const int cs = (c.ns + nsc - 1) / nsc;
      if ((nsc - 1) * cs >= c.ns) continue;
      c.nsc = nsc;
      c.cs = cs;
      if (small_chain_lds_of(c, exp_mode) <= (size_t)SS_LDS_PLAN) return true;
    }
  }
  // Still not placed: one slab per workgroup wants more workgroups, or more LDS per workgroup (wide chunks), than the
  // slice offers.  Several slabs per workgroup (round 5): narrow chunks keep B / R / X / Y small, the grid is
  // ceil(na / spw) * nsc <= gmax.  Fewest slabs per workgroup first, then the most chunks that fit; A resident if it fits.
  // (only for slices of at most 64 compute units -- four or more replicas: on larger grids a chain that does not fit with
  // one slab per workgroup is better served by the general multi-launch kernels, which is what it got before)
  if (n_cu > 64) return false;
  for (int spw = 2; spw <= 64 && spw <= 2 * c.na; spw *= 2) {
    const int ngrp = (c.na + spw - 1) / spw;
    if (ngrp > gmax) continue;
    for (int nsc = 8; nsc >= 1; nsc /= 2) {
      if (ngrp * nsc > gmax) continue;
      const int cs = (c.ns + nsc - 1) / nsc;
      if (nsc > 1 && cs < 4) continue;
      if ((nsc - 1) * cs >= c.ns) continue;
      c.nsc = nsc;
      c.cs = cs;
      c.spw = spw;
      for (int res = 1; res >= 0; --res) {
        c.a_resident = res;
        if (small_chain_lds_of(c, exp_mode) <= (size_t)SS_LDS_PLAN) return true;
      }
    }
  }
  c.spw = 1;
  c.a_resident = 1;
  return false;
}

}  // namespace mitdvp
