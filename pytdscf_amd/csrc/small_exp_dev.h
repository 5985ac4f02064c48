// small_exp_dev.h -- device functions shared by the kernels that run a whole local exponential inside one launch
// (k_small_site in small_site.hip: a grid of workgroups per engine; k_batch_sweep in batch_site.hip: one workgroup per
// replica): the workgroup size, the fixed-order reductions, the small in-LDS product, the k x k projected exponential
// (ss_expm_col0 / wave_expm_tridiag) and the scalar logic of short_iterative_lanczos / _arnoldi (_integrator.py:287-655:
// the warm-up memory _iter_info, the exhausted Krylov space, which iterations are inspected).  Both kernels call these
// very functions, so the two paths cannot drift apart.  Device code only; include from a .hip file.
#pragma once
#include "common.h"
#include "small_chain_plan.h"
#include "vecops.h"

namespace mitdvp {
namespace {

// (the workgroup size SS_THREADS, SS_WAVES and SS_PAYMAX: small_chain_plan.h, which the host-side planner shares)
constexpr double SS_EPS = 1e-12;  // _integrator.py:22

// fixed-order sum of the SS_WAVES per-wave partials p[0..SS_WAVES)
__device__ __forceinline__ double wtree(const double* p) {
  // written out (halving tree: i += i + 8, then 4, 2, 1): as loops over a local array hipcc kept the array in scratch
  double b0, b1, b2, b3, b4, b5, b6, b7;
  if constexpr (SS_WAVES == 16) {
    b0 = p[0] + p[8]; b1 = p[1] + p[9]; b2 = p[2] + p[10]; b3 = p[3] + p[11];
    b4 = p[4] + p[12]; b5 = p[5] + p[13]; b6 = p[6] + p[14]; b7 = p[7] + p[15];
  } else {
    b0 = p[0]; b1 = p[1]; b2 = p[2]; b3 = p[3]; b4 = p[4]; b5 = p[5]; b6 = p[6]; b7 = p[7];
  }
  const double c0 = b0 + b4, c1 = b1 + b5, c2 = b2 + b6, c3 = b3 + b7;
  const double d0 = c0 + c2, d1 = c1 + c3;
  return d0 + d1;
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// C(M x N) = A(M x K) * B(K x N), all row-major in LDS.  The operands are tiny (a few hundred outputs,
// K of a few dozen): the time goes into the dependent chain of K multiply-adds behind LDS latency, so K is
// split over KS adjacent lanes (KS = the largest power of two that still leaves every thread an output)
// and the KS partial sums are combined with cross-lane adds in a fixed order.
// all-reduce over groups of KS (<= 16) adjacent lanes with DPP moves (a cross-lane add costs one VALU
// issue; the LDS-crossbar shuffle would cost a round trip per step); the pairing order is fixed
template <int CTRL>
__device__ __forceinline__ double dpp_add(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double ks_allreduce(double v, int KS) {
  if (KS >= 2) v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
  if (KS >= 4) v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
  if (KS >= 8) v = dpp_add<0x141>(v);  // row_half_mirror: the other quad of the same 8 lanes
  if (KS >= 16) v = dpp_add<0x140>(v); // row_mirror: the other half of the same 16 lanes
  return v;
}

// C = scl * A B.  (Measured and dropped, round 2: a 2 x 2 block of outputs per thread -- half the LDS reads per
// multiply-add, but four times the cross-lane reduction work: the stages got 25 % slower.  At 16 waves per CU this
// kernel is bound by VALU issue slots, ~500 instructions per wave and stage of which the multiply-adds are a quarter.
// The same products as 16 x 16 MFMA tiles (one wave per tile, zero-padded edges): equal stage times (2.8 / 3.2 / 2.5 us) --
// four or five tiles keep four or five of the sixteen waves busy on a dependent read -> MFMA chain -- and the second code
// path cost the kernel 6 % through register spills: dropped as well.)
__device__ __forceinline__ void lds_gemm(const zc* __restrict__ A, int lda, const zc* __restrict__ B, int ldb,
                                         zc* __restrict__ C, int ldc, int M, int N, int K, double scl) {
  const int mn = M * N;
  int KS = 1, lg = 0;
  while (KS < 16 && mn * KS * 2 <= SS_THREADS && KS * 2 <= K) { KS *= 2; ++lg; }
  const int per = SS_THREADS >> lg;
  const int ks = threadIdx.x & (KS - 1);
  const int npass = (mn + per - 1) / per;
  for (int ps = 0; ps < npass; ++ps) {
    const int o = ps * per + (threadIdx.x >> lg);
    const bool valid = o < mn;
    const int oo = valid ? o : mn - 1;
    const int m = oo / N, n = oo - m * N;
    const zc* ap = A + m * lda;
    const zc* bp = B + n;
    // four k-steps per batch: all eight LDS reads are issued before the first multiply-add (hipcc otherwise
    // waits for every pair), and the four products feed independent accumulators
    double r0 = 0.0, r1 = 0.0, i0 = 0.0, i1 = 0.0;
    int k = ks;
    for (; k + 3 * KS < K; k += 4 * KS) {
      zc av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { av[u] = ap[k + u * KS]; bv[u] = bp[(k + u * KS) * ldb]; }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        r0 = fma(av[u].x, bv[u].x, r0); r1 = fma(-av[u].y, bv[u].y, r1);
        i0 = fma(av[u].x, bv[u].y, i0); i1 = fma(av[u].y, bv[u].x, i1);
      }
    }
    for (; k < K; k += KS) {
      const zc a = ap[k], b = bp[k * ldb];
      r0 = fma(a.x, b.x, r0); r1 = fma(-a.y, b.y, r1);
      i0 = fma(a.x, b.y, i0); i1 = fma(a.y, b.x, i1);
    }
    const double re = ks_allreduce(r0 + r1, KS), im = ks_allreduce(i0 + i1, KS);
    if (valid && ks == 0) C[m * ldc + n] = make_double2(re * scl, im * scl);
  }
}

// first column of exp(T) for the k x k matrix T (LDS, row-major, ld = k), by the whole workgroup:
// scaling and squaring (|T / 2^s|_1 <= 1/2) around the degree-16 Taylor polynomial, remainder
// 0.5^17 / 17! = 2e-20 (small_linalg.h::expm_col0 is the host twin, summed to degree 20), evaluated in
// Paterson-Stockmeyer form with the powers A^2, A^3, A^4:
//   p(A) = B0 + A^4 (B1 + A^4 (B2 + A^4 (B3 + A^4 / 16!))),  Bi = sum_{r<4} A^r / (4i + r)!
// = 3 + 4 products instead of 16.  Tm is destroyed; M2, M3, M4, Pm, Qm are k x k scratch.
__device__ void ss_expm_col0(zc* Tm, zc* M2, zc* M3, zc* M4, zc* Pm, zc* Qm, int k, zc* coef, double* wsh) {
  const int tid = threadIdx.x, kk = k * k;
  if (k == 1) {
    if (tid == 0) {
      const zc z = Tm[0];
      const double e = exp(z.x);
      coef[0] = make_double2(e * cos(z.y), e * sin(z.y));
    }
    __syncthreads();
    return;
  }
  if (tid < k) {  // 1-norm: max column sum
    double s = 0.0;
    for (int i = 0; i < k; ++i) { const zc z = Tm[i * k + tid]; s += sqrt(z.x * z.x + z.y * z.y); }
    wsh[tid] = s;
  }
  __syncthreads();
  double nrm = 0.0;
  for (int j = 0; j < k; ++j) nrm = fmax(nrm, wsh[j]);
  int sq = 0;
  while (nrm > 0.5 && sq < 60) { nrm *= 0.5; ++sq; }
  const double sc = ldexp(1.0, -sq);
  for (int t = tid; t < kk; t += SS_THREADS) { zc z = Tm[t]; z.x *= sc; z.y *= sc; Tm[t] = z; }
  __syncthreads();
  lds_gemm(Tm, k, Tm, k, M2, k, k, k, k, 1.0);
  __syncthreads();
  lds_gemm(M2, k, Tm, k, M3, k, k, k, k, 1.0);
  lds_gemm(M2, k, M2, k, M4, k, k, k, k, 1.0);
  __syncthreads();
  // inverse factorials 1/n!, n = 0..16
  constexpr double F[17] = {1.0, 1.0, 0.5, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880,
                            1.0 / 3628800, 1.0 / 39916800, 1.0 / 479001600, 1.0 / 6227020800.0, 1.0 / 87178291200.0,
                            1.0 / 1307674368000.0, 1.0 / 20922789888000.0};
  auto bcoef = [&](int i, int t) -> zc {  // element t of B_i
    const zc a1 = Tm[t], a2 = M2[t], a3 = M3[t];
    const double one = (t / k == t % k) ? 1.0 : 0.0;
    return make_double2(F[4 * i] * one + F[4 * i + 1] * a1.x + F[4 * i + 2] * a2.x + F[4 * i + 3] * a3.x,
                        F[4 * i + 1] * a1.y + F[4 * i + 2] * a2.y + F[4 * i + 3] * a3.y);
  };
  for (int t = tid; t < kk; t += SS_THREADS) {  // P = B3 + A^4 / 16!
    const zc b = bcoef(3, t), a4 = M4[t];
    Pm[t] = make_double2(b.x + F[16] * a4.x, b.y + F[16] * a4.y);
  }
  __syncthreads();
  for (int i = 2; i >= 0; --i) {  // P <- B_i + A^4 P
    lds_gemm(M4, k, Pm, k, Qm, k, k, k, k, 1.0);
    __syncthreads();
    for (int t = tid; t < kk; t += SS_THREADS) {
      const zc b = bcoef(i, t), q = Qm[t];
      Pm[t] = make_double2(b.x + q.x, b.y + q.y);
    }
    __syncthreads();
  }
  for (int s = 0; s < sq; ++s) {  // E <- E E
    lds_gemm(Pm, k, Pm, k, Qm, k, k, k, k, 1.0);
    __syncthreads();
    for (int t = tid; t < kk; t += SS_THREADS) Pm[t] = Qm[t];
    __syncthreads();
  }
  if (tid < k) coef[tid] = Pm[tid * k];
  __syncthreads();
}

// coef = first column of exp(scale * T_k) for the TRIDIAGONAL T of a Lanczos recurrence (diagonal alpha, off-diagonal
// beta), by ONE WAVE with the vector in registers: lane q holds row q of T / 2^s and entry q of the vector, a product
// T p is two wave shifts and three complex multiply-adds, exp(T / 2^s) e_0 is the degree-20 Taylor sum (|T / 2^s|_1 <= 1:
// remainder 1 / 21! = 2e-20) applied 2^s times.  No LDS, no barrier, no k x k products: 20 dependent steps of ~50 cycles
// where ss_expm_col0 takes seven k x k products behind workgroup barriers (measured in k_small_site at C2: 14.2 us per
// inspected iteration, two per local exponential).  Every wave of the workgroup may run it redundantly (same
// instructions, same bits): all then know s, which decides uniformly whether this form is used (s <= SS_VEC_SMAX; for
// larger norms the 2^s repetitions cost more than squaring the matrix).  Returns s; coef is written by the caller's wave 0.
constexpr int SS_VEC_SMAX = 3;
__device__ __forceinline__ double wave_shr1(double v) {  // lane q <- lane q - 1 (lane 0 <- 0)
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_shl1(double v) {  // lane q <- lane q + 1 (lane 63 <- 0)
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_max64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// compute: only the wave(s) that pass true run the Taylor sum (the scaling exponent is returned to every caller).  All 16
// waves of a workgroup running it side by side shared four SIMDs: ~8 us per call in the MITDVP_SS_TRACE timelines, 2.4 us
// with one wave (the others wait at the barrier that follows anyway) and 1 / n as literals of the unrolled sum.
__device__ __forceinline__ int wave_expm_tridiag(const zc* alpha, const double* beta, zc scale, int k, bool real_alpha,
                                                 zc& out, bool compute = true) {
  const int q = threadIdx.x & 63;
  zc a = make_double2(0.0, 0.0), bl = a, bu = a;
  if (q < k) {
    zc al = alpha[q];
    if (real_alpha) al.y = 0.0;
    a = make_double2(scale.x * al.x - scale.y * al.y, scale.x * al.y + scale.y * al.x);
    if (q + 1 < k) { const double b = beta[q]; bu = make_double2(scale.x * b, scale.y * b); }
    if (q > 0) { const double b = beta[q - 1]; bl = make_double2(scale.x * b, scale.y * b); }
  }
  // column q of T: T[q][q] = a, T[q-1][q] = b_{q-1}, T[q+1][q] = b_q
  double nrm = wave_max64(sqrt(a.x * a.x + a.y * a.y) + sqrt(bl.x * bl.x + bl.y * bl.y) + sqrt(bu.x * bu.x + bu.y * bu.y));
  int s = 0;
  while (nrm > 1.0 && s < 60) { nrm *= 0.5; ++s; }
  if (s > SS_VEC_SMAX || !compute) return s;
  const double sc = ldexp(1.0, -s);
  a.x *= sc; a.y *= sc; bl.x *= sc; bl.y *= sc; bu.x *= sc; bu.y *= sc;
  zc y = make_double2(q == 0 ? 1.0 : 0.0, 0.0);
  for (int rep = 0; rep < (1 << s); ++rep) {
    zc p = y, acc = y;
#pragma unroll
    for (int n = 1; n <= 20; ++n) {
      const zc pm = make_double2(wave_shr1(p.x), wave_shr1(p.y));  // p_{q-1}
      const zc pp = make_double2(wave_shl1(p.x), wave_shl1(p.y));  // p_{q+1}
      // (T p)_q = T[q][q-1] p_{q-1} + T[q][q] p_q + T[q][q+1] p_{q+1}, T[q][q-1] = b_{q-1}, T[q][q+1] = b_q
      double re = a.x * p.x - a.y * p.y, im = a.x * p.y + a.y * p.x;
      re = fma(bl.x, pm.x, re); re = fma(-bl.y, pm.y, re);
      im = fma(bl.x, pm.y, im); im = fma(bl.y, pm.x, im);
      re = fma(bu.x, pp.x, re); re = fma(-bu.y, pp.y, re);
      im = fma(bu.x, pp.y, im); im = fma(bu.y, pp.x, im);
      const double inv = 1.0 / (double)n;
      p = make_double2(re * inv, im * inv);
      acc.x += p.x; acc.y += p.y;
    }
    y = acc;
  }
  out = y;
  return s;
}

// ---- scalar logic of a local exponential (one thread; the arrays live in LDS) -------------------------------------------
// _iter_info, _integrator.py:178-186: how many iterations pass without an inspection, from the previous solve's dimension
__device__ __forceinline__ int ss_n_warm(int k_prev, long nsize) {
  return (int)min(nsize, (long)min(max(0, k_prev - 2), 15));
}

// After iteration l (nrm2 = |u_{l+1}|^2): records beta_l and the factor of the next basis vector, and decides what this
// iteration inspects (_integrator.py:569-652, :392-430): ctl[1] = 0 nothing, 1 the convergence test, 2 the space is
// exhausted (close with what there is); ctl[2] = dimension of the projected problem; ctl[3] = first beta not yet looked at.
__device__ __forceinline__ void ss_decide(int l, long nsize, int ndim, int n_warm, bool lanczos, double nrm2, double* beta,
                                          double* invb, zc* hess, int* ctl) {
  const double b = sqrt(nrm2);
  beta[l] = b;
  invb[l + 1] = b >= SS_EPS ? 1.0 / b : 1.0;  // exhausted Krylov space: the vector is left as it is
  if (!lanczos && b > SS_EPS) hess[(l + 1) * MAXK + l] = make_double2(b, 0.0);
  int act = 0, kd = 0;
  const bool last_possible = (l + 1 == nsize);
  if (!(l < n_warm && !last_possible && l + 1 < ndim)) {
    int ld = l;
    bool exhausted = false;
    for (int q = ctl[3]; q <= l; ++q)
      if (beta[q] < SS_EPS || q + 1 == nsize) { ld = q; exhausted = true; break; }
    ctl[3] = l + 1;
    if (!(ld < n_warm && !exhausted)) { kd = ld + 1; act = exhausted ? 2 : 1; }
  }
  ctl[1] = act;
  ctl[2] = kd;
}

// coef = exp(scale * T_k) e_0 of a Lanczos recurrence in the one-wave vector form, when its scaling exponent allows
// (every wave calls it: the decision is uniform); false: the caller takes ss_fill_T + ss_expm_col0
__device__ __forceinline__ bool ss_try_tridiag(bool lanczos, int k, const zc* alpha, const double* beta, zc scale, zc* coef) {
  if (!(lanczos && k > 1)) return false;
  zc cq;
  const int sq_ = wave_expm_tridiag(alpha, beta, scale, k, false, cq, threadIdx.x < 64);
  if (sq_ > SS_VEC_SMAX) return false;
  if (threadIdx.x < k) coef[threadIdx.x] = cq;
  __syncthreads();
  return true;
}

// Tm (k x k, LDS) = scale * (the tridiagonal T of a Lanczos recurrence | the Hessenberg matrix of an Arnoldi one)
__device__ __forceinline__ void ss_fill_T(zc* Tm, int k, bool lanczos, const zc* alpha, const double* beta, const zc* hess,
                                          zc scale) {
  for (int t = threadIdx.x; t < k * k; t += SS_THREADS) {
    const int i = t / k, j = t - i * k;
    zc z = make_double2(0.0, 0.0);
    if (lanczos) {
      if (i == j) z = alpha[i];
      else if (i == j + 1) z = make_double2(beta[j], 0.0);
      else if (j == i + 1) z = make_double2(beta[i], 0.0);
    } else {
      if (i <= j + 1) z = hess[i * MAXK + j];
    }
    Tm[t] = make_double2(scale.x * z.x - scale.y * z.y, scale.x * z.y + scale.y * z.x);
  }
  __syncthreads();
}

}  // namespace
}  // namespace mitdvp
