// small_site.hip -- the small-bond kernel family (SURVEY 8d "C2 and small-D": a site is a few hundred KB,
// every step of the reference is latency bound; north_star: "SIL local propagator fused into one kernel
// launch per site").
//
// Reference functions replaced (paths relative to /root/reference/pytdscf):
//   multiplyH_MPS_direct_MPO._op_lcr_dot / .dot     _contraction.py:1038-1243   (H_eff apply)
//   multiplyK_MPS_direct_MPO._op_lr_dot / .dot      _contraction.py:1297-1407   (K_eff apply)
//   contract_with_site_mpo                          _contraction.py:148-397     (environment update)
//   short_iterative_lanczos / short_iterative_arnoldi  _integrator.py:453-655, :287-432
//     incl. the host work the reference does per iteration: two device->host syncs (:553-554),
//     eigh_tridiagonal / eig + solve of the projected matrix (:590, :618, :402-408), vstack (:568).
//
// ONE kernel, k_small_site:
//   * a workgroup owns (slab a, chunk sc of the contracted right index s); the three stages of the
//     contraction chain run out of LDS (operands A_a, W2, R staged once per launch, X and Y never leave
//     LDS); the chunk partials of a slab are summed in a fixed order by the owners of the output range;
//   * EXP mode wraps the Krylov loop around it: per iteration TWO grid-wide exchanges of a few doubles
//     per workgroup (the projections <v_j|H v_l>, which are linear in the chunk partials and therefore
//     travel with them; then the norm of the new vector), the k x k exponential (scaling and squaring,
//     degree-20 Taylor: the algorithm of small_linalg.h::expm_col0) evaluated redundantly by every
//     workgroup, the reference's convergence test and the final linear combination -- no host involvement.
//     The basis is kept unnormalised (u_j) with the factors 1/beta_j applied on the fly: v_j = u_j * invb_j
//     is the same floating-point number wherever it is formed, so results equal the multi-launch path's.
//
// Inter-workgroup protocol (MI355X_MICROARCH.md, "Workgroup dispatch ... visibility", valid forms, row 1):
// every byte another workgroup reads is stored with an agent-scope (sc1) store and read with an agent-scope
// (sc1) load; every storing wave drains (s_waitcnt vmcnt(0)) before the workgroup barrier that precedes the
// ONE arrival atomic per workgroup; one lane polls the counter and the other waves proceed behind a
// workgroup barrier.  The grid never exceeds the CU count and a workgroup takes more than half a CU's LDS,
// so all workgroups are resident; every poll loop is bounded (2 s) and raises a sticky error instead of
// hanging.  Reductions are summed in a fixed order: all workgroups obtain bit-identical scalars and take
// identical branches.
#include "small_site.h"
#include "krylov_dev.h"
#include "small_exp_dev.h"

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/mitdvp.h"

namespace mitdvp {
namespace {

constexpr int SS_NGR = 2 * SS_PAYMAX;  // granules per workgroup and exchange

#define SS_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ double ld_sh(const double* p) { return __hip_atomic_load(p, SS_RLX); }
__device__ __forceinline__ void st_sh(double* p, double v) { __hip_atomic_store(p, v, SS_RLX); }
__device__ __forceinline__ zc ldz_sh(const zc* p) {
  const double* q = reinterpret_cast<const double*>(p);
  return make_double2(ld_sh(q), ld_sh(q + 1));
}
__device__ __forceinline__ void stz_sh(zc* p, zc v) {
  double* q = reinterpret_cast<double*>(p);
  st_sh(q, v.x);
  st_sh(q + 1, v.y);
}

struct SsArgs {
  SmallChain c;
  int mode;
  const zc* v;  // APPLY: input vector
  zc* out;      // APPLY: output (contiguous (na, ni, nr))
  zc* x;        // EXP: in/out vector
  zc* U;        // EXP: unnormalised Krylov vectors, U[j] at j*N (j >= 1; vector 0 is x)
  zc* P;        // chunk partials [nsc][N]
  zc shift;
  int add_shift;
  SmallExp e;
  unsigned epoch0;  // tags of this launch's exchanges are epoch0 + 1, + 2, ...
  unsigned* abort_w;
  unsigned* err_w;
  unsigned long long* gran;
  long long* stats;
  int* kprev;
  long long* trace;  // debugging: workgroup 0 stamps s_memrealtime at its phase boundaries (nullptr = off)
};

struct Sync {
  unsigned long long* gran;
  unsigned* abort_w;
  int G, wg;
  unsigned epoch;
};


// Grid-wide exchange: every workgroup contributes pay[0..npay) (LDS), every workgroup receives the
// element-wise sums over all workgroups in red[0..npay) (LDS), summed in the same order everywhere.
// Also orders all sc1 stores issued before it against all sc1 loads issued after it, grid-wide.
//
// The data is the flag (MI355X_MICROARCH.md price list, "allgather"; cdna_hip_programming.md Guideline 16 R2):
// every double travels as two 8-byte granules {tag = epoch, 32 payload bits}, each written by ONE
// agent-scope store; thread t reads the granules of workgroup t until all carry this epoch's tag.  No
// counter, no separate flag: one store->load round trip.  Granules are laid out [index][workgroup] so a
// wave's poll is one coalesced request; two buffers alternate (a writer can be at most one epoch ahead of
// the slowest reader).  Returns false (uniformly) when a wait timed out or the abort flag was raised.
__device__ bool ss_exchange(Sync& s, const double* pay, int npay, double* red, double* wsh /*[SS_WAVES*SS_PAYMAX]*/) {
  s.epoch += 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ng = npay > 0 ? 2 * npay : 1;
  unsigned long long* base = s.gran + (size_t)(s.epoch & 1u) * SS_NGR * SS_MAXG;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its sc1 stores of vector data have landed
  __syncthreads();
  if (tid < ng) {
    unsigned half = 0u;
    if (npay > 0) {
      const unsigned long long b = (unsigned long long)__double_as_longlong(pay[tid >> 1]);
      half = (tid & 1) ? (unsigned)(b >> 32) : (unsigned)b;
    }
    __hip_atomic_store(base + (size_t)tid * SS_MAXG + s.wg, ((unsigned long long)s.epoch << 32) | half, SS_RLX);
  }
  int ok = 1;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();  // 100 MHz
  for (int g0 = 0; g0 < ng; g0 += 8) {
    unsigned long long x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = 0ull;
    if (tid < s.G && ok) {
      unsigned spins = 0;
      for (;;) {
        bool ready = true;
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (g0 + q < ng) {
            x[q] = __hip_atomic_load(base + (size_t)(g0 + q) * SS_MAXG + tid, SS_RLX);
            ready = ready && (unsigned)(x[q] >> 32) == s.epoch;
          }
        if (ready) break;
        __builtin_amdgcn_s_sleep(1);
        if ((++spins & 255u) == 0u) {
          if (__hip_atomic_load(s.abort_w, SS_RLX) != 0u) { ok = 0; break; }
          if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) {  // 2 s: a workgroup is not resident
            __hip_atomic_store(s.abort_w, 1u, SS_RLX);
            ok = 0;
            break;
          }
        }
      }
    }
    if (npay > 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (g0 + 2 * q < ng) {
          double v = 0.0;
          if (tid < s.G) v = __longlong_as_double((long long)((x[2 * q] & 0xffffffffull) | (x[2 * q + 1] << 32)));
          v = wave_sum64(v);
          if (lane == 0 && w < 4) wsh[(g0 / 2 + q) * 4 + w] = v;  // G <= 256: waves 0..3 hold the workgroups
        }
    }
  }
  if (!__syncthreads_and(ok)) return false;
  if (npay > 0) {
    if (tid < npay) red[tid] = (wsh[tid * 4 + 0] + wsh[tid * 4 + 1]) + (wsh[tid * 4 + 2] + wsh[tid * 4 + 3]);
    __syncthreads();
  }
  return true;
}


// ---------------------------------------------------------------------------
// krylov_dev.h: the Ritz step of the MULTI-launch Krylov loop on the device (one workgroup).  Reference semantics:
// _iter_info warm-up (_integrator.py:178-186) is applied by the host (it decides WHICH iterations are inspected, a
// function of k_prev only); here: the scalars of iterations [q0, l], exhaustion (:569 / :392), the projected exponential
// (:581-637 / :397-409; real alpha -> the symmetric tridiagonal T, :617-621), and the bookkeeping of the previous Ritz
// coefficients for the convergence test (:638-651) that kry_diff finishes.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double kr_sum256(const double* __restrict__ p, int stride, int lane) {
  // one wave: fixed-order sum of NPART = 256 partials (stride in doubles between consecutive partials)
  const double v = (p[(size_t)lane * stride] + p[(size_t)(lane + 64) * stride]) +
                   (p[(size_t)(lane + 128) * stride] + p[(size_t)(lane + 192) * stride]);
  return wave_sum64(v);  // lane 0
}

__global__ __launch_bounds__(SS_THREADS) void k_kry_ritz(KryRitzArgs a) {
  static_assert(NPART == 256, "kr_sum256 is written for 256 partials");
  __shared__ zc mats[6 * MAXK * MAXK];
  __shared__ zc coef_s[MAXK];
  __shared__ double wsh[SS_WAVES * SS_PAYMAX];
  __shared__ int ctl[4];
  KryDev* st = a.st;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (!a.first && st->state != KRY_RUNNING) return;  // closed by an earlier check: the host has queued one iteration too many
  for (int q = a.q0; q <= a.l; ++q) {
    const int nz = a.lanczos ? 1 : q + 1;
    for (int j = w; j <= nz; j += SS_WAVES) {
      if (j < nz) {
        const double* p = reinterpret_cast<const double*>(a.lanczos ? a.alpha_p + (size_t)q * NPART
                                                                   : a.h_p + ((size_t)q * MAXK + j) * NPART);
        const double re = kr_sum256(p, 2, lane), im = kr_sum256(p + 1, 2, lane);
        if (lane == 0) {
          if (a.lanczos) st->alpha[q] = make_double2(re, im);
          else st->hess[j * MAXK + q] = make_double2(re, im);
        }
      } else {
        const double s = kr_sum256(a.nrm_p + (size_t)q * NPART, 1, lane);
        if (lane == 0) st->beta[q] = sqrt(s);
      }
    }
  }
  if (a.first && w == SS_WAVES - 1) {
    const double s = a.beta0_p ? kr_sum256(a.beta0_p, 1, lane) : 1.0;
    if (lane == 0) st->beta0 = a.beta0_p ? sqrt(s) : 1.0;
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    st->deferred = a.deferred;
    if (a.deferred) {  // unnormalised basis: invb_q = 1 / beta_{q-1} (1 below eps), alpha_q = invb_q (^2) * raw dot
      if (a.first) st->invb[0] = 1.0;
      for (int q = a.q0; q <= a.l; ++q) {
        const double f = st->invb[q];
        const double fa = a.orthodox ? f * f : f;
        st->alpha[q].x *= fa;
        st->alpha[q].y *= fa;
        const double b = st->beta[q];
        if (q + 1 < MAXK) st->invb[q + 1] = b >= a.eps ? 1.0 / b : 1.0;
      }
    }
    int ld = a.l, exhausted = 0;
    for (int q = a.q0; q <= a.l; ++q) {
      const double b = st->beta[q];
      if (!a.lanczos && b > a.eps) st->hess[(q + 1) * MAXK + q] = make_double2(b, 0.0);
      if (b < a.eps || q + 1 == a.nsize) { ld = q; exhausted = 1; break; }
    }
    int real_alpha = 1;
    if (a.lanczos)
      for (int q = 0; q <= ld; ++q)
        if (fabs(st->alpha[q].y) > 1e-10) real_alpha = 0;
    ctl[0] = ld + 1;
    ctl[1] = exhausted;
    ctl[2] = real_alpha;
  }
  __threadfence_block();
  __syncthreads();
  const int k = ctl[0];
  const bool exhausted = ctl[1] != 0, real_alpha = ctl[2] != 0;
  zc* Tm = mats;
  zc* M2 = Tm + MAXK * MAXK;
  zc* M3 = M2 + MAXK * MAXK;
  zc* M4 = M3 + MAXK * MAXK;
  zc* Pm = M4 + MAXK * MAXK;
  zc* Qm = Pm + MAXK * MAXK;
  bool vec_done = false;
  if (a.lanczos && k > 1) {  // tridiagonal: vector form in one wave (wave_expm_tridiag)
    zc cq;
    const int sq_ = wave_expm_tridiag(st->alpha, st->beta, a.scale, k, real_alpha, cq, tid < 64);
    if (sq_ <= SS_VEC_SMAX) {
      if (tid < k) coef_s[tid] = cq;
      __syncthreads();
      vec_done = true;
    }
  }
  if (!vec_done) {
    for (int t = tid; t < k * k; t += SS_THREADS) {
      const int i = t / k, j = t - i * k;
      zc z = make_double2(0.0, 0.0);
      if (a.lanczos) {
        if (i == j) { z = st->alpha[i]; if (real_alpha) z.y = 0.0; }
        else if (i == j + 1) z = make_double2(st->beta[j], 0.0);
        else if (j == i + 1) z = make_double2(st->beta[i], 0.0);
      } else {
        if (i <= j + 1) z = st->hess[i * MAXK + j];
      }
      Tm[t] = make_double2(a.scale.x * z.x - a.scale.y * z.y, a.scale.x * z.y + a.scale.y * z.x);
    }
    __syncthreads();
    ss_expm_col0(Tm, M2, M3, M4, Pm, Qm, k, coef_s, wsh);
  }
  const int have_prev = a.first ? 0 : st->have_prev;
  const int prev_len = a.first ? 0 : st->prev_len;
  if (tid < k) {
    const zc c = coef_s[tid];
    st->coef[tid] = c;
    if (!exhausted) {
      if (have_prev) {
        zc d = c;
        if (tid < prev_len) { const zc o = st->cprev[tid]; d.x -= o.x; d.y -= o.y; }
        if (a.deferred) { const double f = st->invb[tid]; d.x *= f; d.y *= f; }  // kry_diff combines the STORED vectors
        st->dcoef[tid] = d;
      } else {
        st->cprev[tid] = c;
      }
    }
  }
  if (tid == 0) {
    st->k = k;
    if (a.first) { st->ticket = 0u; st->err = -1.0; }
    if (exhausted) {
      st->state = KRY_EXHAUSTED;
      st->need_diff = 0;
    } else {
      st->state = KRY_RUNNING;
      st->need_diff = have_prev ? 1 : 0;
      if (!have_prev) { st->have_prev = 1; st->prev_len = k; }
    }
  }
}

// (the LDS carve ss_carve: small_chain_plan.h -- the same arithmetic runs on the host in small_chain_lds)
__global__ __launch_bounds__(SS_THREADS) void k_small_site(SsArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  zc* sm = reinterpret_cast<zc*>(smem);
  const SmallChain& c = g.c;
  const bool exp_mode = g.mode == SS_MODE_EXP;
  const Carve cv = ss_carve(c, exp_mode);
  zc* As = sm + cv.As;
  zc* Rs = sm + cv.Rs;
  zc* Ws = sm + cv.Ws;
  zc* Bs = sm + cv.Bs;
  zc* Xs = sm + cv.Xs;
  zc* Ys = c.W2 ? sm + cv.Ys : Xs;
  zc* Sg = sm + cv.Sg;
  double* pay = reinterpret_cast<double*>(sm + cv.misc);
  double* red = pay + SS_PAYMAX;
  double* wsh = red + SS_PAYMAX;
  zc* alpha = reinterpret_cast<zc*>(wsh + SS_WAVES * SS_PAYMAX);
  zc* coef = alpha + MAXK;
  zc* cprev = coef + MAXK;
  zc* hess = cprev + MAXK;  // (MAXK+1) x MAXK, row-major, ld = MAXK
  double* beta = reinterpret_cast<double*>(hess + (MAXK + 1) * MAXK);
  double* invb = beta + MAXK;
  int* ctl = reinterpret_cast<int*>(invb + MAXK + 1);  // [0] exchange verdict, [1] action, [2] kdim, [3] next_unread

  const int tid = threadIdx.x;
  const int nsc = c.nsc, cs = c.cs;
  // a workgroup owns chunk sc of the contracted index for spw consecutive slabs (spw = 1: one slab -- the layout of a
  // full-size grid; spw > 1: an engine confined to a slice of the chip, ensemble mode): R, W and the stage-1 operand B of
  // the chunk are shared by its slabs, A_a is per slab (all resident in LDS when they fit, else re-staged per slab)
  const int spw = c.spw > 1 ? c.spw : 1;
  const int ag = blockIdx.x / nsc, sc = blockIdx.x - ag * nsc;
  const int a_first = ag * spw;
  const int nsl = min(spw, c.na - a_first);  // >= 1 by construction of the plan
  const int s0 = sc * cs;
  const int csl = min(cs, c.ns - s0);  // >= 1 by construction of the plan
  const int slab = c.ni * c.nr;
  const long N = (long)c.na * slab;
  const int rg = (slab + nsc - 1) / nsc;
  const int r_lo = min(sc * rg, slab), r_hi = min((sc + 1) * rg, slab);  // this chunk's share of an output slab
  const int nAone = c.nc * c.nb;

  Sync sy{g.gran, g.abort_w, (int)gridDim.x, (int)blockIdx.x, g.epoch0};
  int ntr = 1;
  auto stamp = [&](int label) {
    if (g.trace && blockIdx.x == 0 && tid == 0 && ntr < 250) {
      g.trace[2 * ntr] = (long long)__builtin_amdgcn_s_memrealtime();
      g.trace[2 * ntr + 1] = label;
      g.trace[512 + ntr] = (long long)__builtin_amdgcn_s_memtime();
      ntr += 1;
      g.trace[0] = ntr;
    }
  };
  stamp(0);

  // ---- operands that do not change during the launch -> LDS -------------------------------
  // Every thread's first elements of the three operands are loaded before any of them is stored: one exposed L2 latency
  // at the start of a launch instead of one per loop trip (As 1, Rs 2, Ws 4 trips at C2: ~4 of the ~10 us a launch
  // spent before its first product in the MITDVP_SS_TRACE timelines).  Longer operands finish in the plain loops below.
  {
    const int nA = c.a_resident ? nAone * nsl : 0, kk = c.nt * cs, nR = kk * c.nr, nW = c.W2 ? c.ni * c.nt * c.nc * c.nj : 0;
    auto ldA = [&](int t) __attribute__((always_inline)) -> zc {
      const int q = t / nAone, tt = t - q * nAone;
      const int cc = tt / c.nb, b = tt - cc * c.nb;
      zc z = c.A[(long)(a_first + q) * c.sAa + (long)cc * c.sAc + (long)b * c.sAb];
      if (c.conjA) z.y = -z.y;
      return z;
    };
    auto ldR = [&](int t) __attribute__((always_inline)) -> zc {
      // r fastest in LDS; pick the global order that keeps loads coalesced for the common layouts
      const int k = t / c.nr, r = t - k * c.nr;
      const int tt = k / cs, sl = k - tt * cs;
      zc z = make_double2(0.0, 0.0);
      if (sl < csl) z = c.R[(long)r * c.sRr + (long)tt * c.sRt + (long)(s0 + sl) * c.sRs];
      return z;
    };
    zc za = make_double2(0.0, 0.0), zr[2], zw[4];
    if (tid < nA) za = ldA(tid);
#pragma unroll
    for (int u = 0; u < 2; ++u) { zr[u] = make_double2(0.0, 0.0); if (tid + u * SS_THREADS < nR) zr[u] = ldR(tid + u * SS_THREADS); }
#pragma unroll
    for (int u = 0; u < 4; ++u) { zw[u] = make_double2(0.0, 0.0); if (tid + u * SS_THREADS < nW) zw[u] = c.W2[tid + u * SS_THREADS]; }
    if (tid < nA) As[tid] = za;
#pragma unroll
    for (int u = 0; u < 2; ++u) if (tid + u * SS_THREADS < nR) Rs[tid + u * SS_THREADS] = zr[u];
#pragma unroll
    for (int u = 0; u < 4; ++u) if (tid + u * SS_THREADS < nW) Ws[tid + u * SS_THREADS] = zw[u];
    for (int t = tid + SS_THREADS; t < nA; t += SS_THREADS) As[t] = ldA(t);
    for (int t = tid + 2 * SS_THREADS; t < nR; t += SS_THREADS) Rs[t] = ldR(t);
    for (int t = tid + 4 * SS_THREADS; t < nW; t += SS_THREADS) Ws[t] = c.W2[t];
  }
  stamp(3);

  // stage-1 operand of this chunk: Bs[b][(j, sl)] = scale * vec(b, j, s0 + sl)
  auto load_B = [&](const zc* vec, bool shared, double scl) {
    const int ncol = c.nj * cs, total = c.nb * ncol;
    for (int t0 = 0; t0 < total; t0 += 4 * SS_THREADS) {  // all loads of a batch in flight before the first use
      zc z[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * SS_THREADS + tid;
        z[u] = make_double2(0.0, 0.0);
        if (t < total) {
          const int b = t / ncol, q = t - b * ncol;
          const int j = q / cs, sl = q - j * cs;
          if (sl < csl) {
            const zc* p = vec + (long)b * c.sBb + (long)j * c.sBj + (long)(s0 + sl) * c.sBs;
            z[u] = shared ? ldz_sh(p) : *p;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * SS_THREADS + tid;
        if (t < total) Bs[t] = make_double2(z[u].x * scl, z[u].y * scl);
      }
    }
  };

  // the three stages; this chunk's partial of out[a][:][:] ends up in Sg (LDS)
  auto chain = [&](int q) {
    const zc* Aq = As + (c.a_resident ? (size_t)q * nAone : 0);
    if (!c.a_resident) {  // A of this slab -> LDS (the previous slab's stage 1 is long over: two barriers ago)
      // (round 5, measured and dropped: requesting slab q + 1's A into registers before this slab's stages and storing it
      // into a second slot afterwards -- the registers held across the three stages added spills to a kernel that is
      // already spill-bound: 8 x 32 CUs 812 -> 634 sweeps/s, 16 x 16 CUs 998 -> 756, profiles/r05_ensemble_probe.txt)
      for (int t = tid; t < nAone; t += SS_THREADS) {
        const int cc = t / c.nb, b = t - cc * c.nb;
        zc z = c.A[(long)(a_first + q) * c.sAa + (long)cc * c.sAc + (long)b * c.sAb];
        if (c.conjA) z.y = -z.y;
        As[t] = z;
      }
    }
    __syncthreads();
    stamp(20);
    lds_gemm(Aq, c.nb, Bs, c.nj * cs, Xs, c.nj * cs, c.nc, c.nj * cs, c.nb, 1.0);
    __syncthreads();
    stamp(21);
    if (c.W2) {
      lds_gemm(Ws, c.nc * c.nj, Xs, cs, Ys, cs, c.ni * c.nt, cs, c.nc * c.nj, 1.0);
      __syncthreads();
    }
    stamp(22);
    lds_gemm(Ys, c.nt * cs, Rs, c.nr, Sg, c.nr, c.ni, c.nr, c.nt * cs, 1.0);
    __syncthreads();
    stamp(23);
  };

  zc* Pchunk = g.P + (size_t)sc * N;  // this chunk's partials; slab a at + a * slab

  if (!exp_mode) {
    load_B(g.v, false, 1.0);
    stamp(1);
    for (int sl = 0; sl < nsl; ++sl) {
      const long a = a_first + sl;
      chain(sl);
      for (int q = tid; q < slab; q += SS_THREADS) {
        zc v = Sg[q];
        if (g.add_shift && sc == 0) {  // the scalar term (coupleJ * ovlp, _contraction.py:1200-1216) rides on chunk 0
          const zc x = g.v[a * slab + q];
          v.x += g.shift.x * x.x - g.shift.y * x.y;
          v.y += g.shift.x * x.y + g.shift.y * x.x;
        }
        stz_sh(Pchunk + a * slab + q, v);
      }
    }
    stamp(2);
    if (!ss_exchange(sy, pay, 0, red, wsh)) {
      if (blockIdx.x == 0 && tid == 0) atomicMax(g.err_w, (unsigned)SS_ETIMEOUT);
      return;
    }
    for (int sl = 0; sl < nsl; ++sl) {
      const long eb = (long)(a_first + sl) * slab;
      for (long e = eb + r_lo + tid; e < eb + r_hi; e += SS_THREADS) {
        zc s = make_double2(0.0, 0.0);
        for (int q = 0; q < nsc; ++q) {
          const zc p = ldz_sh(g.P + (size_t)q * N + e);
          s.x += p.x; s.y += p.y;
        }
        g.out[e] = s;
      }
    }
    return;
  }

  // =====================================================================================
  // EXP mode: x <- exp(scale * Op) x   (short_iterative_lanczos / _arnoldi)
  // =====================================================================================
  const SmallExp& ex = g.e;
  const bool lanczos = ex.integrator == MITDVP_LANCZOS;
  const bool cn = ex.conserve_norm != 0;
  const long nsize = N;
  const int ndim = (int)min((long)ex.max_krylov, nsize);
  const int k_prev = g.kprev[ex.site];
  const int n_warm = ss_n_warm(k_prev, nsize);
  const zc scale = make_double2(ex.scale_re, ex.scale_im);

  // basis vector j at element e: v_j(e) = u_j(e) * invb[j], u_0 = x (input, plain loads)
  auto basis = [&](int j, long e) -> zc {
    zc z = j == 0 ? g.x[e] : ldz_sh(g.U + (size_t)j * N + e);
    const double f = invb[j];
    z.x *= f; z.y *= f;
    return z;
  };
  auto fail = [&](int code) {
    if (blockIdx.x == 0 && tid == 0) atomicMax(g.err_w, (unsigned)code);
  };

  // the elements this workgroup owns in the assembled vectors: its chunk's share [r_lo, r_hi) of each of its slabs
  auto own = [&](auto&& body) __attribute__((always_inline)) {
    for (int sl = 0; sl < nsl; ++sl) {
      const long eb = (long)(a_first + sl) * slab;
      for (long e = eb + r_lo + tid; e < eb + r_hi; e += SS_THREADS) body(e);
    }
  };

  // ---- _normalize (_integrator.py:189-203) ---------------------------------------------
  double beta0 = 1.0;
  if (!cn) {
    double s = 0.0;
    own([&](long e) { const zc z = g.x[e]; s += z.x * z.x + z.y * z.y; });
    s = wave_sum64(s);
    if ((tid & 63) == 0) wsh[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) pay[0] = wtree(wsh);
    __syncthreads();
    if (!ss_exchange(sy, pay, 1, red, wsh)) { fail(SS_ETIMEOUT); return; }
    beta0 = sqrt(red[0]);
    if (beta0 == 0.0) { fail(SS_EZERO); return; }
  }
  stamp(4);
  if (tid == 0) {
    invb[0] = 1.0 / beta0;
    ctl[3] = 0;  // next_unread
  }
  __syncthreads();
  stamp(5);

  bool have_prev = false;
  int prev_len = 0;
  int napply = 0;
  for (int l = 0; l < ndim; ++l) {
    // ---- sigma = Op v_l : chunk partials + the projections that are linear in them ----------
    stamp(10);
    load_B(l == 0 ? g.x : g.U + (size_t)l * N, l != 0, invb[l]);
    stamp(11);
    const int jlo = lanczos ? (ex.variant == 0 ? 0 : l) : 0;
    const int jhi = lanczos ? jlo : l;
    const int nd = jhi - jlo + 1;
    {
      const int lane = tid & 63, w = tid >> 6;
      // per-wave sums of the projections accumulate over the workgroup's slabs in wsh (each slot has ONE writer: lane 0
      // of its wave, which also clears it here)
      if (lane == 0)
        for (int j = 0; j < 2 * nd; ++j) wsh[j * SS_WAVES + w] = 0.0;
      for (int sl = 0; sl < nsl; ++sl) {
        const long ab = (long)(a_first + sl) * slab;
        chain(sl);
        // store this chunk's partial (with the scalar term on chunk 0) and keep the shifted values in Sg
        for (int q = tid; q < slab; q += SS_THREADS) {
          zc v = Sg[q];
          const long e = ab + q;
          if (g.add_shift && sc == 0) {  // (H + shift) v_l: the projections below must see the scalar term too
            const zc vl = basis(l, e);
            v.x += g.shift.x * vl.x - g.shift.y * vl.y;
            v.y += g.shift.x * vl.y + g.shift.y * vl.x;
            Sg[q] = v;
          }
          stz_sh(Pchunk + e, v);
        }
        // projections <v_j | partial>, four basis vectors per pass (registers: four accumulator pairs at a time)
        for (int j0 = 0; j0 < nd; j0 += 4) {
          double dre[4] = {0.0, 0.0, 0.0, 0.0}, dim_[4] = {0.0, 0.0, 0.0, 0.0};
          for (int q = tid; q < slab; q += SS_THREADS) {
            const zc v = Sg[q];
            const long e = ab + q;
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j0 + j < nd) {
                const zc b = basis(jlo + j0 + j, e);  // conj(b) * v
                dre[j] += b.x * v.x + b.y * v.y;
                dim_[j] += b.x * v.y - b.y * v.x;
              }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j0 + j < nd) {
              const double r1 = wave_sum64(dre[j]), r2 = wave_sum64(dim_[j]);
              if (lane == 0) { wsh[(2 * (j0 + j)) * SS_WAVES + w] += r1; wsh[(2 * (j0 + j) + 1) * SS_WAVES + w] += r2; }
            }
        }
      }
      stamp(12);
      napply += 1;
      __syncthreads();
      if (tid < 2 * nd) pay[tid] = wtree(wsh + tid * SS_WAVES);
      __syncthreads();
      stamp(13);
      if (!ss_exchange(sy, pay, 2 * nd, red, wsh)) { fail(SS_ETIMEOUT); return; }
      stamp(14);
      if (tid == 0) {
        if (lanczos) alpha[l] = make_double2(red[0], red[1]);
        else
          for (int j = 0; j <= l; ++j) hess[j * MAXK + l] = make_double2(red[2 * j], red[2 * j + 1]);
      }
      __syncthreads();
    }
    // ---- own range: assemble sigma, orthogonalise, norm ---------------------------------------
    {
      double s = 0.0;
      const double bprev = l > 0 ? beta[l - 1] : 0.0;
      own([&](long e) {
        // v_l and v_{l-1} are requested before the chunk partials: their latencies overlap the partial loop's
        zc vl = l == 0 ? g.x[e] : ldz_sh(g.U + (size_t)l * N + e);
        zc vm = make_double2(0.0, 0.0);
        if (lanczos && l > 0) vm = l == 1 ? g.x[e] : ldz_sh(g.U + (size_t)(l - 1) * N + e);
        zc u = make_double2(0.0, 0.0);
        for (int q = 0; q < nsc; ++q) {
          const zc p = ldz_sh(g.P + (size_t)q * N + e);
          u.x += p.x; u.y += p.y;
        }
        { const double f = invb[l]; vl.x *= f; vl.y *= f; }
        if (lanczos) {  // _integrator.py:556-562
          const zc al = alpha[l];
          u.x -= al.x * vl.x - al.y * vl.y;
          u.y -= al.x * vl.y + al.y * vl.x;
          if (l > 0) {
            const double f = invb[l - 1];
            vm.x *= f; vm.y *= f;
            u.x -= bprev * vm.x;
            u.y -= bprev * vm.y;
          }
        } else {  // classical Gram-Schmidt against all vectors, _orth_step_np (:247-260)
          for (int j = 0; j <= l; ++j) {
            const zc h = hess[j * MAXK + l];
            const zc vj = j == l ? vl : basis(j, e);
            u.x -= h.x * vj.x - h.y * vj.y;
            u.y -= h.x * vj.y + h.y * vj.x;
          }
        }
        stz_sh(g.U + (size_t)(l + 1) * N + e, u);
        s += u.x * u.x + u.y * u.y;
      });
      s = wave_sum64(s);
      __syncthreads();
      if ((tid & 63) == 0) wsh[tid >> 6] = s;
      __syncthreads();
      if (tid == 0) pay[0] = wtree(wsh);
      __syncthreads();
      stamp(15);
      if (!ss_exchange(sy, pay, 1, red, wsh)) { fail(SS_ETIMEOUT); return; }
      stamp(16);
    }
    // ---- scalars; decide what this iteration inspects (_integrator.py:569-652, :392-430) --------
    if (tid == 0) ss_decide(l, nsize, ndim, n_warm, lanczos, red[0], beta, invb, hess, ctl);
    __syncthreads();
    int act = ctl[1];
    const int k = ctl[2];
    if (act == 0) continue;

    // ---- coef = exp(scale * T_k) e_0 ------------------------------------------------------------
    bool vec_done = false;
    stamp(30);
    vec_done = ss_try_tridiag(lanczos, k, alpha, beta, scale, coef);  // tridiagonal: one wave, vector form
    if (!vec_done) {
      zc* Tm = Bs;
      zc* M2 = Tm + MAXK * MAXK;
      zc* M3 = M2 + MAXK * MAXK;
      zc* M4 = M3 + MAXK * MAXK;
      zc* Pm = M4 + MAXK * MAXK;
      zc* Qm = Pm + MAXK * MAXK;
      ss_fill_T(Tm, k, lanczos, alpha, beta, hess, scale);
      stamp(17);
      ss_expm_col0(Tm, M2, M3, M4, Pm, Qm, k, coef, wsh);
      stamp(18);
    }
    stamp(31);
    if (act == 1) {
      if (have_prev) {  // || psi_k - psi_{k-1} ||  (:644-652)
        // (round 4, measured and dropped: issuing the k agent-scope loads of an element in batches of eight before their
        // first use, here, in the closing combination and in the own-range assembly -- C2 204 -> 201 sweeps/s on one box,
        // the wider live ranges spill in the per-iteration loops)
        double s = 0.0;
        own([&](long e) {
          double re = 0.0, im = 0.0;
          for (int j = 0; j < k; ++j) {
            zc d = coef[j];
            if (j < prev_len) { d.x -= cprev[j].x; d.y -= cprev[j].y; }
            const zc vj = basis(j, e);
            re += d.x * vj.x - d.y * vj.y;
            im += d.x * vj.y + d.y * vj.x;
          }
          s += re * re + im * im;
        });
        s = wave_sum64(s);
        __syncthreads();
        if ((tid & 63) == 0) wsh[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) pay[0] = wtree(wsh);
        __syncthreads();
        stamp(32);
        if (!ss_exchange(sy, pay, 1, red, wsh)) { fail(SS_ETIMEOUT); return; }
        stamp(33);
        if (sqrt(red[0]) < ex.thresh) act = 2;
      }
      if (act == 1) {
        __syncthreads();
        if (tid < k) cprev[tid] = coef[tid];
        __syncthreads();
        have_prev = true;
        prev_len = k;
        continue;
      }
    }
    // ---- act == 2: psi = sum_j c_j v_j, renormalised or rescaled (_rescale, :206-213) ------------
    // x is read by OTHER workgroups only before this iteration's exchanges; from here on every
    // workgroup touches its own range only.  With conserve_norm the new vector waits in the unused
    // slot 0 of the basis buffer until its norm is known.
    {
      const double cs_ = cn ? 1.0 : beta0;
      double s = 0.0;
      own([&](long e) {
        double re = 0.0, im = 0.0;
        for (int j = 0; j < k; ++j) {
          const zc d = make_double2(coef[j].x * cs_, coef[j].y * cs_);
          const zc vj = basis(j, e);
          re += d.x * vj.x - d.y * vj.y;
          im += d.x * vj.y + d.y * vj.x;
        }
        if (cn) g.U[e] = make_double2(re, im);
        else g.x[e] = make_double2(re, im);
        s += re * re + im * im;
      });
      if (cn) {
        s = wave_sum64(s);
        __syncthreads();
        if ((tid & 63) == 0) wsh[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) pay[0] = wtree(wsh);
        __syncthreads();
        if (!ss_exchange(sy, pay, 1, red, wsh)) { fail(SS_ETIMEOUT); return; }
        const double inv = 1.0 / sqrt(red[0]);
        own([&](long e) {  // same thread wrote g.U[e] above
          zc z = g.U[e];
          z.x *= inv; z.y *= inv;
          g.x[e] = z;
        });
      }
      if (blockIdx.x == 0 && tid == 0) {
        g.kprev[ex.site] = k;
        atomicAdd(reinterpret_cast<unsigned long long*>(g.stats + ex.stat_slot), (unsigned long long)napply);
        atomicAdd(reinterpret_cast<unsigned long long*>(g.stats + 2 + ex.stat_slot),
                  (unsigned long long)napply * (unsigned long long)ex.flops_per_apply);
      }
      return;
    }
  }
  fail(SS_ENOTCONV);  // "... is not converged in N basis. Try shorter time interval." (:430, :653)
  if (blockIdx.x == 0 && tid == 0) {
    g.kprev[ex.site] = ndim;
    atomicAdd(reinterpret_cast<unsigned long long*>(g.stats + ex.stat_slot), (unsigned long long)napply);
    atomicAdd(reinterpret_cast<unsigned long long*>(g.stats + 2 + ex.stat_slot),
              (unsigned long long)napply * (unsigned long long)ex.flops_per_apply);
  }
}

}  // namespace

void kry_ritz(hipStream_t st, const KryRitzArgs& a) {
  hipLaunchKernelGGL(k_kry_ritz, dim3(1), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// the carve and the planner themselves: small_chain_plan.h (host arithmetic, tested on the CPU)
size_t small_chain_lds(const SmallChain& c, bool exp_mode) { return small_chain_lds_of(c, exp_mode); }

bool small_chain_plan(SmallChain& c, bool exp_mode, int n_cu) { return small_chain_plan_of(c, exp_mode, n_cu); }

// ---- persistent launches of several engines on one GPU ---------------------------------------------------------
// k_small_site exchanges data BETWEEN its workgroups inside one launch, so all workgroups of a launch
// must be resident together.  Two such grids from two engines (an ensemble of trajectories on one GPU, host threads)
// could each get part of the chip and wait for the rest of themselves until the 2 s timeout.  Per device, process
// wide, while more than one engine uses the family: every persistent launch is entered in a list with an event and
// its grid size (one workgroup per compute unit: each takes more than half a CU's LDS), and a new launch is issued only
// once "grids of other engines that may run beside it + its own grid <= compute units" holds (the launching host thread
// waits for the oldest foreign launch otherwise).  Launches that fit beside
// each other still overlap (two C2 local exponentials use 64-128 of the 256 compute units each); any set of launches
// that can be running at the same time fits the chip as a whole, so none can starve another.
namespace {
struct PEvent {  // one recorded launch; shared so that a waiter keeps it alive while it is being retired elsewhere
  hipEvent_t ev = nullptr;
  ~PEvent() { if (ev) (void)hipEventDestroy(ev); }
};
struct PersistentChain {
  std::mutex mu;
  struct InFlight { std::shared_ptr<PEvent> e; int grid; hipStream_t st; };
  std::vector<InFlight> fl;
  int users = 0;
  int n_cu = 0;
};
PersistentChain g_pchain[64];
inline int current_device_slot() {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  return dev >= 0 && dev < 64 ? dev : 63;
}
}  // namespace

void persistent_register(int delta) {
  PersistentChain& c = g_pchain[current_device_slot()];
  std::lock_guard<std::mutex> lk(c.mu);
  c.users += delta;
  if (delta > 0 && c.users == 2) {
    // the engine that was alone so far recorded nothing: let its launches drain once, from now on the list orders them
    HIP_CHECK(hipDeviceSynchronize());
  }
}

// Admission on the HOST: the launching thread waits (hipEventSynchronize, lock released) for the oldest foreign launch
// still in flight until its own grid fits beside the rest.  (Making the STREAM wait instead -- hipStreamWaitEvent on the
// other engine's event -- was measured first: 8 engines fell from ~370 to 43 sweeps/s in aggregate, a cross-stream
// dependency costs far more than the 20-140 us kernels it orders.)
PersistentLaunch::PersistentLaunch(hipStream_t st, int grid, bool partitioned)
    : st_(st), slot_(partitioned ? -1 : current_device_slot()), grid_(grid) {
  if (slot_ < 0) return;  // a stream confined to its own compute units: nobody to wait for
  PersistentChain& c = g_pchain[slot_];
  c.mu.lock();
  chained_ = c.users > 1;
  if (!chained_) return;
  try {
    if (!c.n_cu) {
      int dev = 0;
      HIP_CHECK(hipGetDevice(&dev));
      HIP_CHECK(hipDeviceGetAttribute(&c.n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    }
    for (;;) {
      size_t keep = 0;  // forget what has completed
      for (size_t k = 0; k < c.fl.size(); ++k)
        if (hipEventQuery(c.fl[k].e->ev) != hipSuccess) c.fl[keep++] = c.fl[k];
      c.fl.resize(keep);
      (void)hipGetLastError();  // hipEventQuery reports "not ready" through the error state
      int beside = 0;
      std::shared_ptr<PEvent> oldest;
      for (const auto& f : c.fl)
        if (f.st != st) {  // stream order already puts this stream's own launches before the new one
          beside += f.grid;
          if (!oldest) oldest = f.e;
        }
      if (beside + grid <= c.n_cu || !oldest) break;
      c.mu.unlock();
      const hipError_t rc = hipEventSynchronize(oldest->ev);
      c.mu.lock();
      if (rc != hipSuccess) throw HipError("persistent launch admission: hipEventSynchronize failed");
    }
  } catch (...) {
    c.mu.unlock();
    throw;
  }
}

PersistentLaunch::~PersistentLaunch() {
  if (slot_ < 0) return;
  PersistentChain& c = g_pchain[slot_];
  if (chained_) {
    auto e = std::make_shared<PEvent>();
    if (hipEventCreateWithFlags(&e->ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(e->ev, st_) == hipSuccess)
      c.fl.push_back({e, grid_, st_});
  }
  c.mu.unlock();
}

void small_sync_alloc(SmallSync& s, int nsite, hipStream_t st) {
  if (s.words) return;
  persistent_register(+1);
  HIP_CHECK(hipMalloc(&s.words, 16 * sizeof(unsigned)));
  HIP_CHECK(hipMalloc(&s.slots, (size_t)2 * SS_MAXG * SS_NGR * sizeof(unsigned long long)));
  HIP_CHECK(hipMalloc(&s.stats, 4 * sizeof(long long)));
  HIP_CHECK(hipMalloc(&s.kprev, (size_t)std::max(nsite, 1) * sizeof(int)));
  HIP_CHECK(hipMemsetAsync(s.words, 0, 16 * sizeof(unsigned), st));
  HIP_CHECK(hipMemsetAsync(s.slots, 0, (size_t)2 * SS_MAXG * SS_NGR * sizeof(unsigned long long), st));
  HIP_CHECK(hipMemsetAsync(s.stats, 0, 4 * sizeof(long long), st));
  HIP_CHECK(hipMemsetAsync(s.kprev, 0, (size_t)std::max(nsite, 1) * sizeof(int), st));
  HIP_CHECK(hipStreamSynchronize(st));
  s.launches = 0;
}

void small_sync_free(SmallSync& s) {
  if (s.words) {
    try { persistent_register(-1); } catch (...) {}
  }
  if (s.words) (void)hipFree(s.words);
  if (s.slots) (void)hipFree(s.slots);
  if (s.stats) (void)hipFree(s.stats);
  if (s.kprev) (void)hipFree(s.kprev);
  s = SmallSync{};
}

static void ss_launch(hipStream_t st, SmallSync& sy, SsArgs& g, bool exp_mode) {
  const SmallChain& c = g.c;
  // validate what the kernel's indexing assumes before anything is launched
  if (c.nsc < 1 || c.cs < 1 || (c.nsc - 1) * c.cs >= c.ns || c.nsc * c.cs < c.ns) throw ArgError("small_site: bad chunking");
  const int spw_ = c.spw > 1 ? c.spw : 1;
  const int grid_ = ((c.na + spw_ - 1) / spw_) * c.nsc;
  if (grid_ > SS_MAXG || (sy.max_grid > 0 && grid_ > sy.max_grid)) throw ArgError("small_site: grid exceeds the resident-workgroup bound");
  if (!c.W2 && (c.ni != 1 || c.nj != 1 || c.nt != c.nc)) throw ArgError("small_site: chain without W stage needs ni = nj = 1, nt = nc");
  size_t lds = small_chain_lds(c, exp_mode);
  if (lds > 156 * 1024) throw ArgError("small_site: chain does not fit LDS");
  lds = std::max<size_t>(lds, 84 * 1024);  // > half a CU's LDS: at most one workgroup per CU
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  static bool attr_set[64] = {};  // the attribute is per device
  static std::mutex attr_mu;
  std::lock_guard<std::mutex> lk(attr_mu);
  if (dev >= 64 || !attr_set[dev]) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_small_site), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  156 * 1024));  // the kernel's few static LDS words come out of the same 160 KiB
    if (dev < 64) attr_set[dev] = true;
  }
  // exchange tags are unique per launch: 4096 epochs each (a launch needs at most 4 * MAXK + 2)
  sy.launches += 1;
  if ((sy.launches & 0xFFFFFu) == 0u) {  // tag space wraps: forget the old granules
    HIP_CHECK(hipMemsetAsync(sy.slots, 0, (size_t)2 * SS_MAXG * SS_NGR * sizeof(unsigned long long), st));
    sy.launches += 1;
  }
  g.epoch0 = (sy.launches & 0xFFFFFu) << 12;
  g.abort_w = sy.words + 2;
  g.err_w = sy.words + 3;
  g.gran = reinterpret_cast<unsigned long long*>(sy.slots);
  g.stats = sy.stats;
  g.kprev = sy.kprev;
  static const bool tracing = std::getenv("MITDVP_SS_TRACE") != nullptr;
  static long long* trace_buf = nullptr;
  if (tracing && !trace_buf) {
    HIP_CHECK(hipMalloc(&trace_buf, 1024 * sizeof(long long)));
  }
  g.trace = tracing ? trace_buf : nullptr;
  if (tracing) HIP_CHECK(hipMemsetAsync(trace_buf, 0, 1024 * sizeof(long long), st));
  {  // what is being launched, for the unit seam that reports it (mitdvp_small_apply)
    const Carve cv = ss_carve(c, exp_mode);
    sy.last.mode = g.mode; sy.last.nsc = c.nsc; sy.last.cs = c.cs; sy.last.spw = spw_; sy.last.a_resident = c.a_resident;
    sy.last.grid = grid_; sy.last.lds = cv.total * sizeof(zc); sy.last.sg_aliases_x = cv.Sg == cv.Xs ? 1 : 0;
  }
  {
    PersistentLaunch chain(st, grid_, sy.partitioned);  // admitted only when it fits beside the persistent launches in flight
    hipLaunchKernelGGL(k_small_site, dim3(grid_), dim3(SS_THREADS), lds, st, g);
  }
  HIP_CHECK(hipGetLastError());
  if (tracing) {  // debugging aid: phase timeline of workgroup 0, microseconds since its first stamp
    long long h[1024];
    HIP_CHECK(hipMemcpyAsync(h, trace_buf, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    fprintf(stderr, "[ss_trace] mode=%d G=%d (na=%d nsc=%d cs=%d spw=%d res=%d) lds=%zu:", g.mode, grid_, c.na, c.nsc, c.cs, spw_, c.a_resident, lds);
    for (int i = 1; i < (int)h[0] && i < 250; ++i) fprintf(stderr, " %lld:%.2f", h[2 * i + 1], (double)(h[2 * i] - h[2]) * 0.01);
    const int nn = (int)h[0];
    if (nn > 2)
      fprintf(stderr, " | shader clock %.0f MHz", (double)(h[512 + nn - 1] - h[512 + 1]) / ((double)(h[2 * (nn - 1)] - h[2]) * 0.01));
    fprintf(stderr, "\n");
  }
}

void small_apply(hipStream_t st, SmallSync& sy, const SmallChain& c, const zc* v, zc* out, zc* partials, zc shift,
                 bool add_shift) {
  SsArgs g{};
  g.c = c;
  g.mode = SS_MODE_APPLY;
  g.v = v;
  g.out = out;
  g.P = partials;
  g.shift = shift;
  g.add_shift = add_shift ? 1 : 0;
  ss_launch(st, sy, g, false);
}

void small_exp(hipStream_t st, SmallSync& sy, const SmallChain& c, const SmallExp& e, zc* x, zc* basis, zc* partials,
               zc shift) {
  if ((long)c.na * c.ni * c.nr != (long)c.nb * c.nj * c.ns) throw ArgError("small_exp: the operator must be square");
  SsArgs g{};
  g.c = c;
  g.mode = SS_MODE_EXP;
  g.x = x;
  g.U = basis;
  g.P = partials;
  g.shift = shift;
  g.add_shift = (shift.x != 0.0 || shift.y != 0.0) ? 1 : 0;
  g.e = e;
  ss_launch(st, sy, g, true);
}

}  // namespace mitdvp
