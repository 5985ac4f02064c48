// batch_site.hip -- batched trajectories: k_batch_sweep, ONE workgroup per replica, a whole half-sweep per launch.
// (Further down: k_batch_observe / k_batch_mean, the observables of every replica and their ensemble means, one launch each;
// k_batch_channel, one-site gates and quantum-jump channels between the two half-sweeps of a time step, one launch;
// k_batch_field, time-dependent one-site fields (pulses, noise) as unitaries applied in place in the same slot, one launch;
// k_batch_pair, the same walk with nearest-neighbour gates and jump channels: merge, apply, truncated re-split;
// k_batch_cross / k_batch_snapshot, overlaps and one-site matrix elements between two replicas or their snapshots, one
// workgroup per pair; k_batch_spectra, the Schmidt spectra of the requested bonds; k_batch_sample, configurations drawn
// from every replica's state, one workgroup per replica; k_batch_expect, expectation values of MPO observables, one
// workgroup per replica and operator; k_batch_cross_mpo, matrix elements of MPOs between two replicas or snapshots, one
// workgroup per entry; k_batch_operate, an MPO applied to the replicas; k_batch_relax, right behind k_batch_sweep, the same
// sweep with the lowest eigenvector of H_eff in place of the exponential: improved relaxation; k_batch_relax_defl, the same
// text with rank-one penalties on stored states added to every local solve: excited states by deflation, and
// k_batch_defl_overlaps, the overlaps with the stored states.)
//
// At trajectory shapes (d = 2..4, D <= 32, M <= 16) a local problem is a few tens of kilobytes, so one workgroup can own
// one replica completely: the replica index is blockIdx.x, nothing is exchanged between workgroups, and therefore there is
// no spin wait, no residency requirement, no compute-unit mask and no admission control -- the hardware schedules the B
// workgroups as compute units free up, for any B.  For p = begin .. end the workgroup runs what Engine::sweep_part runs
// with a launch per item:
//   1. exp(scale * H_eff) on the centre tensor        (three-stage chain of small_site.h, stages as workgroup GEMMs)
//   2. the gauge move Psi -> A sigma / sigma B         (Householder thin QR inside the workgroup; the gauge is free)
//   3. the environment update L[p + 1] / R[p]          (operand roles of Engine::chain_env)
//   4. exp(scale * K_eff) on sigma                     (Engine::chain_keff)
//   5. the absorb Psi(p + 1) = sigma B / Psi(p - 1) = A sigma
// The scalar logic of a local exponential (Lanczos alpha variants, Arnoldi, _iter_info warm-up, conserve_norm rescale,
// exhausted Krylov space, the projected exponential, the |psi_k - psi_{k-1}| test) is small_exp_dev.h: the same functions
// k_small_site calls.
//
// What is resident where:
//   * LDS, 56 544 bytes static per workgroup: the two operand tiles of the running product (16 x 32 complex each, rows
//     padded to 33; aliased with the 6 k x k matrices of the projected exponential, which never run at the same time), the
//     Krylov scalars (alpha, beta, 1 / beta, Hessenberg matrix, Ritz coefficients), the Householder scalars of a gauge
//     move and the reduction partials.  LDS would allow two workgroups per compute unit; the register file does not (256
//     VGPRs x 8 waves = 2 waves per SIMD): ONE workgroup, i.e. one replica, is resident per compute unit, 256 at a time.
//   * global memory, per replica, L2-resident at these sizes: the tensors and blocks of the engine, and a scratch area with
//     sigma, a spare tensor, the QR work matrix, the M-fold intermediates X and Y of an apply and the Krylov basis.
//     Everything in it is written and re-read by the SAME workgroup only and ordered by workgroup-scope barriers
//     (__syncthreads: release / acquire fences at workgroup scope around s_barrier).  No device-scope atomic, no flag.
// Every loop is bounded: the Krylov loop by max_krylov, the projected exponential by its fixed caps, the rest by the shapes.
//
// Arithmetic: complex128 FMA products out of LDS tiles; every reduction is a wave tree followed by a fixed order over the
// waves, and every element of every intermediate is computed by the same thread in the same order whatever the grid: a
// replica's result depends neither on B nor on the compute unit it ran on.
//
// Resources: see the figures next to k_batch_sweep below.
#include "batch_site.h"
#include "small_exp_dev.h"

#include <algorithm>

#include "../../include/mitdvp.h"

namespace mitdvp {
namespace {

constexpr int BT_TM = 32, BT_TN = 32, BT_TK = 16;  // output tile and K step of the workgroup product
constexpr int BT_LD = 33;                          // padded leading dimension of the LDS tiles (bank spread)
static_assert(SS_THREADS == 512, "k_batch_sweep: a 32 x 32 tile is two outputs per thread of 512");
static_assert(2 * BT_TK * BT_LD <= 6 * MAXK * MAXK, "the tiles alias the projected exponential's scratch");

struct BtSh {  // pointers into the workgroup's LDS
  zc* mats;      // [6 * MAXK * MAXK]  projected exponential; the product tiles alias it
  double* wsh;   // [SS_WAVES * SS_PAYMAX]
  double* red;   // [8]
  zc *alpha, *coef, *cprev, *hess;
  double *beta, *invb;
  int* ctl;
  zc *udiag, *rdiag;  // [BATCH_MAX_BOND] Householder: diagonal entry of u_j, diagonal of R
  double* gam;        // [BATCH_MAX_BOND] 2 / (u_j^H u_j), 0: no reflection
};

// element-wise sums of NV values per thread over the workgroup -> sh.red[0 .. NV), the same bits in every thread
template <int NV>
__device__ __forceinline__ void wg_reduce(const double (&v)[NV], const BtSh& sh) {
  static_assert(NV <= 8, "red holds 8 values");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const double r = wave_sum64(v[q]);
    if (lane == 0) sh.wsh[q * SS_WAVES + w] = r;
  }
  __syncthreads();
  if (tid < NV) sh.red[tid] = wtree(sh.wsh + tid * SS_WAVES);
  __syncthreads();
}

// C(m, n) = sum_k a(m, k) b(k, n) by the whole workgroup: fa / fb fetch an operand element (global memory, any layout),
// fc stores a result.  32 x 32 output tiles, thread t owns column t % 32 of rows t / 32 and t / 32 + 16; K in steps of 16
// through two LDS tiles.  AK / BK: k is the fast index of the operand in memory (the tile is fetched k-fastest then).
// The k order of every output is fixed; ends with a barrier (the results are visible to the workgroup).
template <bool AK, bool BK, class FA, class FB, class FC>
__device__ __forceinline__ void wg_gemm(int M, int N, int K, zc* tiles, FA&& fa, FB&& fb, FC&& fc) {
  zc* As = tiles;                   // [BT_TK][BT_LD]: As[kk][mm]
  zc* Bs = tiles + BT_TK * BT_LD;   // [BT_TK][BT_LD]: Bs[kk][nn]
  const int tid = threadIdx.x;
  const int tn = tid & 31, tm = tid >> 5;
  const int a_kk = AK ? (tid & 15) : (tid >> 5), a_mm = AK ? (tid >> 4) : (tid & 31);
  const int b_kk = BK ? (tid & 15) : (tid >> 5), b_nn = BK ? (tid >> 4) : (tid & 31);
  for (int m0 = 0; m0 < M; m0 += BT_TM)
    for (int n0 = 0; n0 < N; n0 += BT_TN) {
      double c0r = 0.0, c0i = 0.0, c1r = 0.0, c1i = 0.0;
      for (int k0 = 0; k0 < K; k0 += BT_TK) {
        zc za = make_double2(0.0, 0.0), zb = za;
        if (m0 + a_mm < M && k0 + a_kk < K) za = fa(m0 + a_mm, k0 + a_kk);
        if (n0 + b_nn < N && k0 + b_kk < K) zb = fb(k0 + b_kk, n0 + b_nn);
        As[a_kk * BT_LD + a_mm] = za;
        Bs[b_kk * BT_LD + b_nn] = zb;
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < BT_TK; ++kk) {
          const zc a0 = As[kk * BT_LD + tm], a1 = As[kk * BT_LD + tm + 16], b = Bs[kk * BT_LD + tn];
          c0r = fma(a0.x, b.x, c0r); c0r = fma(-a0.y, b.y, c0r);
          c0i = fma(a0.x, b.y, c0i); c0i = fma(a0.y, b.x, c0i);
          c1r = fma(a1.x, b.x, c1r); c1r = fma(-a1.y, b.y, c1r);
          c1i = fma(a1.x, b.y, c1i); c1i = fma(a1.y, b.x, c1i);
        }
        __syncthreads();
      }
      if (n0 + tn < N) {
        if (m0 + tm < M) fc(m0 + tm, n0 + tn, make_double2(c0r, c0i));
        if (m0 + tm + 16 < M) fc(m0 + tm + 16, n0 + tn, make_double2(c1r, c1i));
      }
    }
  __syncthreads();
}

// The two products of one site of an overlap walk, T (dl x dl) -> T' (dr x dr) between a ket tensor K and a bra tensor:
//   U[m][(j,s)] = sum_n T[m][n] K[n][(j,s)]
__device__ __forceinline__ void wg_walk_u(const zc* T, const zc* Kt, zc* U, int dl, int ddr, zc* tiles) {
  wg_gemm<true, false>(dl, ddr, dl, tiles,
      [&](int m, int kk) { return T[(long)m * dl + kk]; },
      [&](int kk, int n) { return Kt[(long)kk * ddr + n]; },
      [&](int m, int n, zc z) { U[(long)m * ddr + n] = z; });
}
//   T'[i][j] = sum_(m,s) conj(Bra[(m,s)][i]) U[(m,s)][j], K = dl d; CONJ = false: Bra as it stands (the autocorrelation)
template <bool CONJ>
__device__ __forceinline__ void wg_walk_t(const zc* Bt, const zc* U, zc* T2, int dr, int K, zc* tiles) {
  wg_gemm<false, false>(dr, dr, K, tiles,
      [&](int m, int kk) { const zc z = Bt[(long)kk * dr + m]; return CONJ ? make_double2(z.x, -z.y) : z; },
      [&](int kk, int n) { return U[(long)kk * dr + n]; },
      [&](int m, int n, zc z) { T2[(long)m * dr + n] = z; });
}
// The plain overlap <bra | ket> over all L sites: T starts as [1]; ket(p, soff) / bra(p, soff) give the tensors of site
// p, soff being the sum of the sizes of the sites before it.  Returns the block that holds the 1 x 1 result.
template <class FK, class FB>
__device__ __forceinline__ const zc* wg_overlap(int L, const BatchShape* shp, FK&& ket, FB&& bra, zc* T, zc* T2, zc* U, zc* tiles) {
  if (threadIdx.x == 0) T[0] = make_double2(1.0, 0.0);
  __syncthreads();
  size_t soff = 0;
  for (int p = 0; p < L; ++p) {
    const BatchShape s = shp[p];
    const int dl = s.dl, d = s.d, dr = s.dr, ddr = d * dr;
    wg_walk_u(T, ket(p, soff), U, dl, ddr, tiles);
    wg_walk_t<true>(bra(p, soff), U, T2, dr, dl * d, tiles);
    zc* t = T; T = T2; T2 = t;
    soff += (size_t)dl * ddr;
  }
  return T;
}

// A state of a cross request: index i < B is replica i, whose tensors come through its row of the pointer table; index
// i >= B is snapshot i - B, whose tensors lie site after site in the batch's buffer.
struct BtState {
  const zc* const* tab;  // the replica's row, nullptr for a snapshot
  const zc* snap;        // the snapshot's base, nullptr for a replica
  __device__ BtState(int i, int B, void* const* ptrs, int ptr_stride, const zc* snaps, size_t snap_len)
      : tab(i < B ? reinterpret_cast<const zc* const*>(ptrs + (size_t)i * ptr_stride) : nullptr),
        snap(i < B ? nullptr : snaps + (size_t)(i - B) * snap_len) {}
  // the tensor of site p; soff: the sum of the sizes of the sites before p
  __device__ const zc* at(int p, size_t soff) const { return tab ? tab[p] : snap + soff; }
  // a replica that failed in an earlier launch; a snapshot is never dead
  __device__ static bool dead(int i, int B, const int* status) { return i < B && status[i] != SS_OK; }
};

// out[a,i,r] = sum L[a,c,b] W[c,i,j,t] R[r,t,s] (scl * v)[b,j,s]   (small_site.h stages 1-3; Engine::chain_heff)
__device__ __noinline__ void bt_heff(const BatchShape& s, const zc* Lb, const zc* W2, const zc* Rb, const zc* v, double scl, zc* X,
                        zc* Y, zc* out, zc* tiles) {
  const int dl = s.dl, d = s.d, dr = s.dr, ml = s.ml, mr = s.mr;
  const int ddr = d * dr;
  // X[(a,c)][(j,s)] = sum_b L[(a,c)][b] v[b][(j,s)]
  wg_gemm<true, false>(dl * ml, ddr, dl, tiles,
      [&](int m, int k) { return Lb[(long)m * dl + k]; },
      [&](int k, int n) { const zc z = v[(long)k * ddr + n]; return make_double2(z.x * scl, z.y * scl); },
      [&](int m, int n, zc z) { X[(long)m * ddr + n] = z; });
  // Y[a][(i,t)][s] = sum_(c,j) W2[(i,t)][(c,j)] X[a][(c,j)][s]
  const int kw = ml * d, mw = d * mr;
  wg_gemm<true, false>(mw, dl * dr, kw, tiles,
      [&](int m, int k) { return W2[(long)m * kw + k]; },
      [&](int k, int n) { const int a = n / dr, ss = n - a * dr; return X[((long)a * kw + k) * dr + ss]; },
      [&](int m, int n, zc z) { const int a = n / dr, ss = n - a * dr; Y[((long)a * mw + m) * dr + ss] = z; });
  // out[(a,i)][r] = sum_(t,s) Y[(a,i)][(t,s)] R[r][(t,s)]
  const int kr = mr * dr;
  wg_gemm<true, true>(dl * d, dr, kr, tiles,
      [&](int m, int k) { return Y[(long)m * kr + k]; },
      [&](int k, int n) { return Rb[(long)n * kr + k]; },
      [&](int m, int n, zc z) { out[(long)m * dr + n] = z; });
}

// out[a,r] = sum L[a,c,b] (scl * sigma)[b,s] R[r,c,s]   (Engine::chain_keff; no W stage)
__device__ __noinline__ void bt_keff(int dim, int m, const zc* Lb, const zc* Rb, const zc* v, double scl, zc* X, zc* out, zc* tiles) {
  wg_gemm<true, false>(dim * m, dim, dim, tiles,
      [&](int mm, int k) { return Lb[(long)mm * dim + k]; },
      [&](int k, int n) { const zc z = v[(long)k * dim + n]; return make_double2(z.x * scl, z.y * scl); },
      [&](int mm, int n, zc z) { X[(long)mm * dim + n] = z; });
  const int kr = m * dim;
  wg_gemm<true, true>(dim, dim, kr, tiles,
      [&](int mm, int k) { return X[(long)mm * kr + k]; },
      [&](int k, int n) { return Rb[(long)n * kr + k]; },
      [&](int mm, int n, zc z) { out[(long)mm * dim + n] = z; });
}

// The tiles of a product function are LDS, whoever calls it.  The compiler works that out by itself only while EVERY
// caller hands over a __shared__ array directly; k_batch_operate hands it over through BopCtx, and then the product loops
// of bt_env and bt_matmul read the tiles through flat loads instead of LDS loads: 3-4 % of a whole batch step
// (profiles/batch_shared_products.txt).  So those two say it.
__device__ __forceinline__ void assume_lds(const zc* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_assume(__builtin_amdgcn_is_shared(p));
#endif
}

// env'[a,q,r] = sum conj(Bra)(b,c,a) env[b,p,s] W2e[(q,t)][(c,p)] Ket(s,t,r)   (Engine::chain_env), T(in, phys, out) =
// T[in * sTi + phys * sTd + out * sTo] for both tensors: the site tensor itself (->) or its mirror image (<-) without a
// copy.  env (din, min, din) -> env' (dout, mout, dout).  The block update of a sweep passes the site tensor twice.
// This is the one text of the three products; bt_env below is the function the kernels call.
__device__ __forceinline__ void bt_env_body(const zc* env, const zc* Tb, const zc* Tk, long sTi, long sTd, long sTo, const zc* W2e,
                                            int din, int min_, int d, int dout, int mout, zc* X, zc* Y, zc* out, zc* tiles) {
  assume_lds(tiles);
  const int nx = min_ * din;
  // X[(c,a)][(p,s)] = sum_b conj(Bra(b,c,a)) env[b][(p,s)]
  wg_gemm<false, false>(d * dout, nx, din, tiles,
      [&](int m, int k) { const int c = m / dout, a = m - c * dout; const zc z = Tb[k * sTi + c * sTd + a * sTo]; return make_double2(z.x, -z.y); },
      [&](int k, int n) { return env[(long)k * nx + n]; },
      [&](int m, int n, zc z) { X[(long)m * nx + n] = z; });
  // Y[a][(q,t)][s] = sum_(c,p) W2e[(q,t)][(c,p)] X[c][a][p][s]
  const int kw = d * min_, mw = mout * d;
  wg_gemm<true, false>(mw, dout * din, kw, tiles,
      [&](int m, int k) { return W2e[(long)m * kw + k]; },
      [&](int k, int n) {
        const int c = k / min_, p = k - c * min_, a = n / din, ss = n - a * din;
        return X[(((long)c * dout + a) * min_ + p) * din + ss];
      },
      [&](int m, int n, zc z) { const int a = n / din, ss = n - a * din; Y[((long)a * mw + m) * din + ss] = z; });
  // out[(a,q)][r] = sum_(t,s) Y[(a,q)][(t,s)] Ket(s,t,r)
  const int kr = d * din;
  wg_gemm<true, false>(dout * mout, dout, kr, tiles,
      [&](int m, int k) { return Y[(long)m * kr + k]; },
      [&](int k, int n) { const int t = k / din, ss = k - t * din; return Tk[ss * sTi + t * sTd + n * sTo]; },
      [&](int m, int n, zc z) { out[(long)m * dout + n] = z; });
}
__device__ __noinline__ void bt_env(const zc* env, const zc* Tb, const zc* Tk, long sTi, long sTd, long sTo, const zc* W2e, int din,
                                    int min_, int d, int dout, int mout, zc* X, zc* Y, zc* out, zc* tiles) {
  bt_env_body(env, Tb, Tk, sTi, sTd, sTo, W2e, din, min_, d, dout, mout, X, Y, out, tiles);
}
// k_batch_cross_mpo's own instance, the forward roles only: with the strides (d dout, dout, 1) known at compile time its
// walk measured faster than through bt_env (profiles/batch_shared_products.txt)
__device__ __noinline__ void bt_env_fwd(const zc* env, const zc* Tb, const zc* Tk, const zc* W2e, int din, int min_, int d, int dout,
                                        int mout, zc* X, zc* Y, zc* out, zc* tiles) {
  bt_env_body(env, Tb, Tk, (long)d * dout, dout, 1, W2e, din, min_, d, dout, mout, X, Y, out, tiles);
}
// k_batch_block's instance of the same: a second caller of bt_env_fwd moved the registers of k_batch_cross_mpo (180 -> 184
// VGPRs: the tile address stops being a constant of the one caller)
__device__ __noinline__ void bt_env_fwd_blk(const zc* env, const zc* Tb, const zc* Tk, const zc* W2e, int din, int min_, int d, int dout,
                                            int mout, zc* X, zc* Y, zc* out, zc* tiles) {
  bt_env_body(env, Tb, Tk, (long)d * dout, dout, 1, W2e, din, min_, d, dout, mout, X, Y, out, tiles);
}

// dst = A (M x K) . B (K x N), all row-major, by way of tmp (dst may be A or B): the absorb of a sweep
__device__ __noinline__ void bt_matmul(const zc* A, const zc* B, zc* tmp, zc* dst, int M, int N, int K, zc* tiles) {
  assume_lds(tiles);
  wg_gemm<true, false>(M, N, K, tiles,
      [&](int m, int k) { return A[(long)m * K + k]; },
      [&](int k, int n) { return B[(long)k * N + n]; },
      [&](int m, int n, zc z) { tmp[(long)m * N + n] = z; });
  for (long e = threadIdx.x; e < (long)M * N; e += SS_THREADS) dst[e] = tmp[e];
  __syncthreads();
}

// Thin QR of the m x n matrix a(i, j) = src[i * si + j * sj] (m >= n): Q(i, j) -> qdst[i * si + j * sj] (qdst may be src),
// R(i, j) -> rdst[i * ri + j * rj].  Householder reflections H_j = 1 - gam u u^H with u = x + phase(x_j) |x| e_j, so
// R_jj = -phase |x|: no sign convention on diag(R) (the gauge of the sweep is free, qr_thin(..., gauge_free)); a zero
// column gives H_j = 1, so Q is an isometry for rank-deficient input as well.  Wk is the (m x n, row-major) work matrix.
// Element (i, c) belongs to lane i % 64 of wave c % 8 from the first copy to the last store: besides the column of the
// current reflector, published by one barrier per column, a thread reads only what it wrote itself.
__device__ __noinline__ void bt_qr(const zc* src, zc* qdst, long si, long sj, zc* rdst, long ri, long rj, int m, int n, zc* Wk,
                      const BtSh& sh) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int c = w; c < n; c += SS_WAVES)
    for (int i = lane; i < m; i += 64) Wk[(long)i * n + c] = src[i * si + c * sj];
  for (int j = 0; j < n; ++j) {
    if (w == j % SS_WAVES) {  // the owner wave of column j: its norm below the diagonal, the reflector's scalars
      double s = 0.0;
      zc ajj = make_double2(0.0, 0.0);
      for (int i = lane; i < m; i += 64)
        if (i >= j) {
          const zc z = Wk[(long)i * n + j];
          s += z.x * z.x + z.y * z.y;
          if (i == j) ajj = z;
        }
      s = __shfl(wave_sum64(s), 0, 64);
      ajj.x = __shfl(ajj.x, j & 63, 64);
      ajj.y = __shfl(ajj.y, j & 63, 64);
      const double nx = sqrt(s), aa = sqrt(ajj.x * ajj.x + ajj.y * ajj.y);
      zc ph = make_double2(1.0, 0.0);
      if (aa > 0.0) ph = make_double2(ajj.x / aa, ajj.y / aa);
      if (lane == 0) {
        if (nx > 1e-150) {
          sh.udiag[j] = make_double2(ajj.x + ph.x * nx, ajj.y + ph.y * nx);
          sh.gam[j] = 1.0 / (nx * (nx + aa));
          sh.rdiag[j] = make_double2(-ph.x * nx, -ph.y * nx);
        } else {
          sh.udiag[j] = ajj;
          sh.gam[j] = 0.0;
          sh.rdiag[j] = ajj;
        }
      }
    }
    __syncthreads();
    const double gam = sh.gam[j];
    if (gam == 0.0) continue;
    const zc ud = sh.udiag[j];
    int c = j + 1 + ((w - (j + 1)) % SS_WAVES + SS_WAVES) % SS_WAVES;  // first column right of j that this wave owns
    for (; c < n; c += SS_WAVES) {
      double dr_ = 0.0, di_ = 0.0;
      for (int i = lane; i < m; i += 64)
        if (i >= j) {
          const zc u = i == j ? ud : Wk[(long)i * n + j];
          const zc x = Wk[(long)i * n + c];
          dr_ += u.x * x.x + u.y * x.y;  // conj(u) x
          di_ += u.x * x.y - u.y * x.x;
        }
      dr_ = __shfl(wave_sum64(dr_), 0, 64) * gam;
      di_ = __shfl(wave_sum64(di_), 0, 64) * gam;
      for (int i = lane; i < m; i += 64)
        if (i >= j) {
          const zc u = i == j ? ud : Wk[(long)i * n + j];
          zc x = Wk[(long)i * n + c];
          x.x -= u.x * dr_ - u.y * di_;
          x.y -= u.x * di_ + u.y * dr_;
          Wk[(long)i * n + c] = x;
        }
    }
  }
  __syncthreads();
  // Q e_c = H_0 ... H_c e_c (H_j e_c = e_c for j > c), column c in place in qdst
  for (int c = w; c < n; c += SS_WAVES) {
    for (int i = lane; i < m; i += 64) qdst[i * si + c * sj] = make_double2(i == c ? 1.0 : 0.0, 0.0);
    for (int j = c; j >= 0; --j) {
      const double gam = sh.gam[j];
      if (gam == 0.0) continue;
      const zc ud = sh.udiag[j];
      double dr_ = 0.0, di_ = 0.0;
      for (int i = lane; i < m; i += 64)
        if (i >= j) {
          const zc u = i == j ? ud : Wk[(long)i * n + j];
          const zc x = qdst[i * si + c * sj];
          dr_ += u.x * x.x + u.y * x.y;
          di_ += u.x * x.y - u.y * x.x;
        }
      dr_ = __shfl(wave_sum64(dr_), 0, 64) * gam;
      di_ = __shfl(wave_sum64(di_), 0, 64) * gam;
      for (int i = lane; i < m; i += 64)
        if (i >= j) {
          const zc u = i == j ? ud : Wk[(long)i * n + j];
          zc x = qdst[i * si + c * sj];
          x.x -= u.x * dr_ - u.y * di_;
          x.y -= u.x * di_ + u.y * dr_;
          qdst[i * si + c * sj] = x;
        }
    }
  }
  for (int t = tid; t < n * n; t += SS_THREADS) {
    const int i = t / n, c = t - i * n;
    zc z = make_double2(0.0, 0.0);
    if (c > i) z = Wk[(long)i * n + c];
    else if (c == i) z = sh.rdiag[i];
    rdst[i * ri + c * rj] = z;
  }
  __syncthreads();
}

// the operator of a local exponential: H_eff of a site (W2 != nullptr) or K_eff of a bond (dim x dim, MPO bond m)
struct BtOp {
  BatchShape s;
  const zc *Lb, *W2, *Rb;
  int dim, m;
  zc *X, *Y, *tiles;
};
__device__ __forceinline__ void bt_apply(const BtOp& o, const zc* vin, double scl, zc* out) {
  if (o.W2) bt_heff(o.s, o.Lb, o.W2, o.Rb, vin, scl, o.X, o.Y, out, o.tiles);
  else bt_keff(o.dim, o.m, o.Lb, o.Rb, vin, scl, o.X, out, o.tiles);
}
// x <- exp(scale * Op) x for the operator op (bt_apply: out = Op (scl * vin), ends with a barrier):
// short_iterative_lanczos / _arnoldi as k_small_site's EXP mode runs them, with one workgroup owning the whole vector.
// The basis is kept unnormalised (u_j, factors 1 / beta_j applied on the fly) in U[j * N ...), j >= 1; slot 0 of U holds
// the new vector until its norm is known (conserve_norm).  Element e belongs to thread e % 512 throughout.
__device__ __noinline__ int bt_exp(const BtOp& op, zc* x, zc* U, long N, int* kprev_p, zc scale, zc shift, const SmallExp& ex,
                                   const BtSh& sh, long long* stats, int stat_slot, long long flops_per_apply) {
  const int tid = threadIdx.x;
  const bool lanczos = ex.integrator == MITDVP_LANCZOS;
  const bool cn = ex.conserve_norm != 0;
  const bool add_shift = shift.x != 0.0 || shift.y != 0.0;
  const long nsize = N;
  const int ndim = (int)min((long)ex.max_krylov, nsize);
  const int k_prev = __hip_atomic_load(kprev_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  const int n_warm = ss_n_warm(k_prev, nsize);
  zc* alpha = sh.alpha; zc* coef = sh.coef; zc* cprev = sh.cprev; zc* hess = sh.hess;
  double* beta = sh.beta; double* invb = sh.invb; int* ctl = sh.ctl;

  auto basis = [&](int j, long e) -> zc {
    zc z = j == 0 ? x[e] : U[(size_t)j * N + e];
    const double f = invb[j];
    z.x *= f; z.y *= f;
    return z;
  };
  auto account = [&](int k, int napply) {
    if (tid == 0) {
      __hip_atomic_store(kprev_p, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      stats[stat_slot] += napply;
      stats[2 + stat_slot] += (long long)napply * flops_per_apply;
    }
  };

  // ---- _normalize (_integrator.py:189-203) ---------------------------------------------
  double beta0 = 1.0;
  if (!cn) {
    double s[1] = {0.0};
    for (long e = tid; e < N; e += SS_THREADS) { const zc z = x[e]; s[0] += z.x * z.x + z.y * z.y; }
    wg_reduce(s, sh);
    beta0 = sqrt(sh.red[0]);
    if (beta0 == 0.0) return SS_EZERO;
  }
  __syncthreads();
  if (tid == 0) {
    invb[0] = 1.0 / beta0;
    ctl[3] = 0;  // next_unread
  }
  __syncthreads();

  bool have_prev = false;
  int prev_len = 0;
  int napply = 0;
  for (int l = 0; l < ndim; ++l) {
    zc* un = U + (size_t)(l + 1) * N;
    bt_apply(op, l == 0 ? x : U + (size_t)l * N, invb[l], un);
    napply += 1;
    if (add_shift)  // (Op + shift) v_l: the projections below see the scalar term too
      for (long e = tid; e < N; e += SS_THREADS) {
        zc v = un[e];
        const zc vl = basis(l, e);
        v.x += shift.x * vl.x - shift.y * vl.y;
        v.y += shift.x * vl.y + shift.y * vl.x;
        un[e] = v;
      }
    // ---- projections <v_j | Op v_l>: Lanczos one (j = 0 reference, j = l orthodox), Arnoldi j = 0 .. l ----
    const int jlo = lanczos ? (ex.variant == 0 ? 0 : l) : 0;
    const int jhi = lanczos ? jlo : l;
    const int nd = jhi - jlo + 1;
    for (int j0 = 0; j0 < nd; j0 += 4) {
      double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (long e = tid; e < N; e += SS_THREADS) {
        const zc v = un[e];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j0 + j < nd) {
            const zc b = basis(jlo + j0 + j, e);  // conj(b) * v
            acc[2 * j] += b.x * v.x + b.y * v.y;
            acc[2 * j + 1] += b.x * v.y - b.y * v.x;
          }
      }
      wg_reduce(acc, sh);
      if (tid == 0)
        for (int j = 0; j < 4 && j0 + j < nd; ++j) {
          const zc z = make_double2(sh.red[2 * j], sh.red[2 * j + 1]);
          if (lanczos) alpha[l] = z;
          else hess[(j0 + j) * MAXK + l] = z;
        }
      __syncthreads();
    }
    // ---- orthogonalise, norm (_integrator.py:556-562; _orth_step_np :247-260) ---------------------
    {
      double s[1] = {0.0};
      const double bprev = l > 0 ? beta[l - 1] : 0.0;
      for (long e = tid; e < N; e += SS_THREADS) {
        const zc vl = basis(l, e);
        zc u = un[e];
        if (lanczos) {
          const zc al = alpha[l];
          u.x -= al.x * vl.x - al.y * vl.y;
          u.y -= al.x * vl.y + al.y * vl.x;
          if (l > 0) {
            const zc vm = basis(l - 1, e);
            u.x -= bprev * vm.x;
            u.y -= bprev * vm.y;
          }
        } else {
          for (int j = 0; j <= l; ++j) {
            const zc h = hess[j * MAXK + l];
            const zc vj = j == l ? vl : basis(j, e);
            u.x -= h.x * vj.x - h.y * vj.y;
            u.y -= h.x * vj.y + h.y * vj.x;
          }
        }
        un[e] = u;
        s[0] += u.x * u.x + u.y * u.y;
      }
      wg_reduce(s, sh);
    }
    if (tid == 0) ss_decide(l, nsize, ndim, n_warm, lanczos, sh.red[0], beta, invb, hess, ctl);
    __syncthreads();
    int act = ctl[1];
    const int k = ctl[2];
    if (act == 0) continue;

    // ---- coef = exp(scale * T_k) e_0 ------------------------------------------------------------
    if (!ss_try_tridiag(lanczos, k, alpha, beta, scale, coef)) {
      zc* Tm = sh.mats;
      zc* M2 = Tm + MAXK * MAXK;
      zc* M3 = M2 + MAXK * MAXK;
      zc* M4 = M3 + MAXK * MAXK;
      zc* Pm = M4 + MAXK * MAXK;
      zc* Qm = Pm + MAXK * MAXK;
      ss_fill_T(Tm, k, lanczos, alpha, beta, hess, scale);
      ss_expm_col0(Tm, M2, M3, M4, Pm, Qm, k, coef, sh.wsh);
    }
    if (act == 1) {
      if (have_prev) {  // || psi_k - psi_{k-1} ||  (:644-652)
        double s[1] = {0.0};
        for (long e = tid; e < N; e += SS_THREADS) {
          double re = 0.0, im = 0.0;
          for (int j = 0; j < k; ++j) {
            zc dd = coef[j];
            if (j < prev_len) { dd.x -= cprev[j].x; dd.y -= cprev[j].y; }
            const zc vj = basis(j, e);
            re += dd.x * vj.x - dd.y * vj.y;
            im += dd.x * vj.y + dd.y * vj.x;
          }
          s[0] += re * re + im * im;
        }
        wg_reduce(s, sh);
        if (sqrt(sh.red[0]) < ex.thresh) act = 2;
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
    {
      const double cs_ = cn ? 1.0 : beta0;
      double s[1] = {0.0};
      for (long e = tid; e < N; e += SS_THREADS) {
        double re = 0.0, im = 0.0;
        for (int j = 0; j < k; ++j) {
          const zc dd = make_double2(coef[j].x * cs_, coef[j].y * cs_);
          const zc vj = basis(j, e);
          re += dd.x * vj.x - dd.y * vj.y;
          im += dd.x * vj.y + dd.y * vj.x;
        }
        if (cn) U[e] = make_double2(re, im);
        else x[e] = make_double2(re, im);
        s[0] += re * re + im * im;
      }
      if (cn) {
        wg_reduce(s, sh);
        const double inv = 1.0 / sqrt(sh.red[0]);
        for (long e = tid; e < N; e += SS_THREADS) {  // the same thread wrote U[e] above
          zc z = U[e];
          z.x *= inv; z.y *= inv;
          x[e] = z;
        }
      }
      account(k, napply);
      __syncthreads();
      return SS_OK;
    }
  }
  account(ndim, napply);  // "... is not converged in N basis. Try shorter time interval." (:430, :653)
  __syncthreads();
  return SS_ENOTCONV;
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 256 VGPRs, occupancy 2 waves
// per SIMD (one workgroup per compute unit), 56 544 bytes of LDS, and 816 bytes of private memory per lane: the kernel
// body SPILLS 93 vector and 31 scalar registers around the calls of its stage functions (a few times per site of the
// sweep), and the argument blocks those functions take by reference live there too.  The stages are separate
// (non-inlined) device functions because inlined into one body the spills sat inside the product loops (119 VGPRs, 928
// bytes); the product functions bt_heff / bt_keff / bt_env / bt_matmul themselves use 194 / 178 / 196 / 136 VGPRs and no private
// memory, bt_exp 254 VGPRs and 16 bytes.  This misses the "no spills" aim; what it costs is measured, not guessed:
// profiles/batch_probe.txt and DESIGN.md section 7.3.
// The batch kernels SHARE these product functions (and wg_walk_u / wg_walk_t / wg_overlap above): there is one text per
// product, so a new caller may move the register figures of the kernels that already call it.  What a feature is held to
// is: no new vector or scalar spills, no new private memory inside a product loop, unchanged occupancy, and measured time
// (profiles/batch_shared_products.txt has the figures of every kernel and the old-against-new timings of the merge).  A
// kernel that measures slower through a shared function gets a non-inlined instance of the same text, as bt_env_fwd.
__global__ __launch_bounds__(SS_THREADS) void k_batch_sweep(BatchArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_mats[6 * MAXK * MAXK];
  __shared__ zc s_z[3 * MAXK + (MAXK + 1) * MAXK + 2 * BATCH_MAX_BOND];
  __shared__ double s_d[SS_WAVES * SS_PAYMAX + 8 + 2 * MAXK + 1 + BATCH_MAX_BOND];
  __shared__ int s_ctl[4];
  BtSh sh;
  sh.mats = s_mats;
  sh.alpha = s_z; sh.coef = sh.alpha + MAXK; sh.cprev = sh.coef + MAXK; sh.hess = sh.cprev + MAXK;
  sh.udiag = sh.hess + (MAXK + 1) * MAXK; sh.rdiag = sh.udiag + BATCH_MAX_BOND;
  sh.wsh = s_d; sh.red = sh.wsh + SS_WAVES * SS_PAYMAX; sh.beta = sh.red + 8; sh.invb = sh.beta + MAXK;
  sh.gam = sh.invb + MAXK + 1;
  sh.ctl = s_ctl;

  const int r = blockIdx.x, tid = threadIdx.x, L = g.L;
  if (g.status[r] != SS_OK) return;  // a replica that failed in an earlier launch of the call does no more work
  void* const* tab = g.ptrs + (size_t)r * g.ptr_stride;
  zc* const* site = reinterpret_cast<zc* const*>(tab);
  zc* const* envL = reinterpret_cast<zc* const*>(tab + L);
  zc* const* envR = reinterpret_cast<zc* const*>(tab + 2 * L + 1);
  const zc* const* w2l = reinterpret_cast<const zc* const*>(tab + 3 * L + 2);
  const zc* const* w2el = reinterpret_cast<const zc* const*>(tab + 4 * L + 2);
  const zc* const* w2er = reinterpret_cast<const zc* const*>(tab + 5 * L + 2);
  zc* scr = reinterpret_cast<zc*>(tab[6 * L + 2]);
  zc* sig = scr + g.plan.o_sig;
  zc* spare = scr + g.plan.o_spare;
  zc* work = scr + g.plan.o_work;
  zc* X = scr + g.plan.o_x;
  zc* Y = scr + g.plan.o_y;
  zc* U = scr + g.plan.o_u;
  int* kprev = g.kprev + (size_t)r * L;
  long long* stats = g.stats + (size_t)r * 4;
  const zc shift = g.shift[r];
  const zc sc_site = make_double2(g.site_re, g.site_im), sc_bond = make_double2(g.bond_re, g.bond_im);
  const bool fwd = g.forward != 0;
  zc* tiles = sh.mats;

  int rc = SS_OK;
  for (int step = 0; step < L; ++step) {
    const int p = fwd ? step : L - 1 - step;
    const BatchShape s = g.shp[p];
    const int dl = s.dl, d = s.d, dr = s.dr;
    const long N = (long)dl * d * dr;
    {  // 1. exp(scale * H_eff) on the centre tensor
      const zc* Lb = envL[p];
      const zc* Rb = envR[p + 1];
      const zc* W2 = w2l[p];
      const long long fl = (long long)(8.0 * ((double)dl * dl * s.ml * d * dr + (double)dl * dr * s.ml * s.mr * d * d +
                                              (double)dl * dr * dr * s.mr * d));
      const BtOp op{s, Lb, W2, Rb, 0, 0, X, Y, tiles};
      rc = bt_exp(op, site[p], U, N, kprev + p, sc_site, shift, g.e, sh, stats, 0, fl);
    }
    if (rc != SS_OK || step == L - 1) break;
    if (fwd) {
      // 2. Psi2Asigma: A in place of Psi, sigma (dr x dr)
      bt_qr(site[p], site[p], dr, 1, sig, dr, 1, dl * d, dr, work, sh);
      // 3. L[p + 1]
      bt_env(envL[p], site[p], site[p], (long)d * dr, dr, 1, w2el[p], dl, s.ml, d, dr, s.mr, X, Y, envL[p + 1], tiles);
      // 4. exp(scale * K_eff) on sigma
      const zc* Lb = envL[p + 1];
      const zc* Rb = envR[p + 1];
      const int m = s.mr;
      const BtOp op{s, Lb, nullptr, Rb, dr, m, X, Y, tiles};
      rc = bt_exp(op, sig, U, (long)dr * dr, kprev + p, sc_bond, shift, g.e, sh, stats, 1, (long long)(16.0 * (double)m * dr * dr * dr));
      if (rc != SS_OK) break;
      // 5. Psi(p + 1) = sigma . B(p + 1)
      const BatchShape q = g.shp[p + 1];
      const int nn = q.d * q.dr;
      zc* nxt = site[p + 1];
      bt_matmul(sig, nxt, spare, nxt, dr, nn, dr, tiles);
    } else {
      // 2. Psi2sigmaB: Psi^T = Q R  ->  B = Q^T in place of Psi, sigma = R^T (dl x dl)
      const int mq = d * dr;
      bt_qr(site[p], site[p], 1, mq, sig, 1, dl, mq, dl, work, sh);
      // 3. R[p] from the mirror image of B (dr, d, dl), read in place
      bt_env(envR[p + 1], site[p], site[p], 1, dr, (long)d * dr, w2er[p], dr, s.mr, d, dl, s.ml, X, Y, envR[p], tiles);
      // 4. exp(scale * K_eff) on sigma
      const zc* Lb = envL[p];
      const zc* Rb = envR[p];
      const int m = s.ml;
      const BtOp op{s, Lb, nullptr, Rb, dl, m, X, Y, tiles};
      rc = bt_exp(op, sig, U, (long)dl * dl, kprev + p, sc_bond, shift, g.e, sh, stats, 1, (long long)(16.0 * (double)m * dl * dl * dl));
      if (rc != SS_OK) break;
      // 5. Psi(p - 1) = A(p - 1) . sigma
      const BatchShape q = g.shp[p - 1];
      const int mm_ = q.dl * q.d;
      zc* prv = site[p - 1];
      bt_matmul(prv, sig, spare, prv, mm_, dl, dl, tiles);
    }
  }
  if (rc != SS_OK && tid == 0) g.status[r] = rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// Improved relaxation: k_batch_relax, ONE workgroup per replica as above, any number of half-sweeps per launch.  At every
// site the centre tensor is replaced by the lowest eigenvector of H_eff + shift (bt_diag: matrix_diagonalize_lanczos,
// _integrator.py:74-138, as Engine::krylov_diag restates it); the gauge move, the block update and the absorb are those of
// k_batch_sweep, and the bond matrix is left alone (_mps_cls.py:1159-1160).
// What is resident where: LDS holds the two operand tiles of wg_gemm, the reduction partials, the Householder scalars of
// a gauge move and the scalars of the eigen-solve -- alpha, beta, the Ritz coefficients c and c_prev and the two pivot
// sequences of the twisted factorisation, 64 doubles each (23 120 bytes in all).  The Lanczos basis, up to
// min(N, kcap) + 1 NORMALISED vectors, lives in the replica's Krylov carve (BatchPlan::o_u, sized by batch_krylov_carve),
// written and re-read by this workgroup only.
// The projected problem: after every new vector wave 0 finds the lowest eigenpair of T_k (bt_trilow), the other seven
// waves wait at the barrier that publishes the result.  Every loop is bounded: the Lanczos loop by (max_restarts + 1) kcap,
// kcap <= 64 and max_restarts <= BATCH_RELAX_MAX_RESTARTS, the multisection by BT_TRI_ROUNDS, the rest by k.

struct BrSh {  // the eigen-solve's own LDS, 64 doubles each
  double *alpha, *beta, *c, *cprev, *dp, *dm;
  double* out;  // [2]: the lowest Ritz value, |c_k - pad(c_{k-1})|
  int max_restarts;      // thick restarts one local solve may take (BatchRelaxArgs::max_restarts)
  long long* rst_total;  // the replica's counters: restarts taken,
  int* rst_most;         // the most of any one local solve
};

__device__ __forceinline__ double wave_min64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
// (wave_max64: small_exp_dev.h)

constexpr int BT_TRI_ROUNDS = 24;  // multisection rounds: 9 shrink the Gershgorin interval by 63^9 > 2^53, a refused hint costs one

// Lowest eigenpair of the real symmetric tridiagonal T_k (diagonal alpha[0 .. k), off-diagonal beta[0 .. k-1), both in
// LDS), 1 <= k <= 64, by ONE WAVE, all 64 lanes of it: returns the eigenvalue (the same bits in every lane) and leaves the
// unit eigenvector, first component non-negative, in c[0 .. k) and zeros in c[k .. 64).  dp, dm: 64 doubles of LDS each.
//   eigenvalue   multisection on Sturm counts (the pivots q_i = (alpha_i - x) - beta_{i-1}^2 / q_{i-1} of T - x, negative
//                ones counted, tiny ones replaced by -pivmin as LAPACK's dstebz does): every round the lanes count at 64
//                points that span the interval, both ends included, and the interval becomes the one gap in which the
//                count goes from 0 to >= 1.  Since the ends are counted too, a bracket is VERIFIED each round: the first one
//                is the caller's hint [hint - slack, hint + tiny] when it gives one (interlacing: the lowest eigenvalue
//                of T_k is not above that of T_{k-1}; the slack is a residual bound that usually, not always, holds), and
//                a hint that does not bracket falls back to the Gershgorin interval.  Ends at a width of eps |T|.
//   eigenvector  twisted factorisation (Fernando; Parlett & Dhillon): the pivots of T - theta from the top (lane 0) and
//                from the bottom (lane 1), the twist at the smallest |gamma_r|, gamma_r = d+_r + d-_r - (alpha_r - theta),
//                z_r = 1 and the two recurrences away from r.  The residual is |gamma_r| / |z|, small whatever the gap.
__device__ __noinline__ double bt_trilow(const double* alpha, const double* beta, int k, double* c, double* dp, double* dm, bool has_hint,
                                         double hint, double slack) {
  const int lane = threadIdx.x & 63;
  if (k <= 1) {
    c[lane] = lane == 0 ? 1.0 : 0.0;
    return alpha[0];
  }
  const double eps = 2.220446049250313e-16;
  const double a = lane < k ? alpha[lane] : 0.0;
  const double bl = lane > 0 && lane < k ? fabs(beta[lane - 1]) : 0.0;
  const double br = lane + 1 < k ? fabs(beta[lane]) : 0.0;
  double glo = wave_min64(lane < k ? a - bl - br : 1.0e300);
  double ghi = wave_max64(lane < k ? a + bl + br : -1.0e300);
  const double tnorm = fmax(fabs(glo), fabs(ghi));
  const double bmax = wave_max64(fmax(bl, br));
  const double pivmin = 2.2250738585072014e-308 * fmax(1.0, bmax * bmax);
  const double wide = 2.0 * tnorm * eps * k + 2.0 * pivmin;
  glo -= wide;
  ghi += wide;
  const double tol = eps * tnorm;

  double lo = glo, hi = ghi;
  bool on_hint = false;
  if (has_hint && hint == hint && slack == slack) {  // NaN: no hint
    const double l2 = hint - slack - 16.0 * tol, h2 = hint + 16.0 * tol;
    if (l2 > glo && h2 < ghi) { lo = l2; hi = h2; on_hint = true; }
  }
  for (int round = 0; round < BT_TRI_ROUNDS; ++round) {
    const double w = hi - lo;
    double x = lo + w * ((double)lane * (1.0 / 63.0));
    if (lane == 63) x = hi;
    double q = alpha[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int cnt = q < 0.0 ? 1 : 0;
    for (int i = 1; i < k; ++i) {
      const double b = beta[i - 1];
      q = (alpha[i] - x) - b * b / q;
      if (fabs(q) < pivmin) q = -pivmin;
      cnt += q < 0.0 ? 1 : 0;
    }
    const unsigned long long m = __ballot(cnt >= 1);
    if (m == 0ull || (m & 1ull)) {  // no eigenvalue below hi, or one below lo: not a bracket
      if (!on_hint) break;          // the widened Gershgorin interval always is one; keep what there is
      on_hint = false;
      lo = glo;
      hi = ghi;
      continue;
    }
    on_hint = false;  // verified
    const int j = __ffsll((long long)m) - 1;  // 1 .. 63: the first point with an eigenvalue below it
    const double nlo = __shfl(x, j - 1, 64), nhi = __shfl(x, j, 64);
    const bool stall = !(nlo > lo || nhi < hi);
    lo = nlo;
    hi = nhi;
    if (stall || hi - lo <= tol) break;
  }
  const double theta = 0.5 * (lo + hi);

  // ---- the eigenvector ----
  const double pivv = fmax(eps * tnorm, pivmin);
  if (lane < 2) {  // the same text for both directions: lane 0 runs rows 0 .. k-1, lane 1 rows k-1 .. 0
    const bool up = lane == 0;
    double* d = up ? dp : dm;
    int row = up ? 0 : k - 1;
    double q = alpha[row] - theta;
    if (fabs(q) < pivv) q = -pivv;
    d[row] = q;
    for (int i = 1; i < k; ++i) {
      const double b = up ? beta[i - 1] : beta[k - 1 - i];
      row = up ? i : k - 1 - i;
      q = (alpha[row] - theta) - b * b / q;
      if (fabs(q) < pivv) q = -pivv;
      d[row] = q;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const double gam = lane < k ? fabs(dp[lane] + dm[lane] - (a - theta)) : 1.0e300;
  const double gmin = wave_min64(gam);
  const int r = __ffsll((long long)__ballot(gam == gmin)) - 1;
  if (lane == 0) c[r] = 1.0;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  if (lane < 2) {  // lane 0 walks from the twist up to row 0, lane 1 down to row k-1
    const bool up = lane == 0;
    const int n = up ? r : k - 1 - r;
    double z = 1.0;
    for (int i = 1; i <= n; ++i) {
      const int row = up ? r - i : r + i;
      const double b = up ? beta[row] : beta[row - 1];
      const double piv = up ? dp[row] : dm[row];
      z = -(b / piv) * z;
      c[row] = z;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const double z = lane < k ? c[lane] : 0.0;
  const double n2 = __shfl(wave_sum64(z * z), 0, 64);
  const double z0 = __shfl(z, 0, 64);
  const double inv = (z0 < 0.0 ? -1.0 : 1.0) / sqrt(n2);
  c[lane] = z * inv;
  return theta;
}

// x <- the lowest eigenvector of Op + shift, Op the H_eff of BtOp (bt_apply ends with a barrier): orthodox Lanczos,
// alpha_l = Re <v_l | (Op + shift) v_l>, with one workgroup owning the whole vector; the basis is kept NORMALISED in
// U[j * N ...), j = 0 .. kcap, slot 0 a copy of x as it came (the reference does not normalise its start either).
// Element e belongs to thread e % 512 throughout.  After every new vector the lowest eigenpair of T_k; converged when
// |c_k - pad(c_{k-1})| < thresh in coefficient space, or beta_k < SS_EPS, or k == N; then x = sum_j c_j v_j, renormalised.
// After kcap vectors without convergence: a thick restart (below) while rs.max_restarts allows one, else SS_ENOTCONV; with
// rs.max_restarts == 0 the loop is the one it always was.  *kprev_p <- k of the last cycle; stats count the applies of all
// cycles; the lowest Ritz value is left in rs.out[0] (behind a barrier).
// DEFL: the operator is Op + shift + sum_k w_k |q_k><q_k| with the df.K projected stored states of BtDefl (k_batch_relax_defl);
// the rank-one terms are added to un right behind the apply, element e by its owning thread, so nothing else changes.
// This is the one text of the solve; bt_diag and bt_diag_defl below are the functions the kernels call.
struct BtDefl {
  int K;            // stored states, 1 .. BATCH_MAX_DEFLATE
  const zc* q;      // q_k at q + k * qs: phi_k in the replica's basis at this site, N elements each
  size_t qs;
  const double* w;  // w_k at w[k * ws]
  size_t ws;
};
// un += sum_k w_k q_k <q_k | v>, four slots per round (red holds 8 doubles).  Element e of un is read and written by its
// owning thread e % 512 only, which is also the one that reads it next in the solve; the apply before ended with a barrier.
__device__ __noinline__ void bt_defl_add(const BtDefl& df, const zc* vi, zc* un, long N, const BtSh& sh) {
  const int tid = threadIdx.x;
  for (int k0 = 0; k0 < df.K; k0 += 4) {
    const int nk = min(4, df.K - k0);
    const zc* q0 = df.q + (size_t)k0 * df.qs;
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long e = tid; e < N; e += SS_THREADS) {
      const zc v = vi[e];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nk) {
          const zc q = q0[(size_t)j * df.qs + e];
          s[2 * j] += q.x * v.x + q.y * v.y;  // conj(q) v
          s[2 * j + 1] += q.x * v.y - q.y * v.x;
        }
    }
    wg_reduce(s, sh);
    double cr[4], ci[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double w = j < nk ? df.w[(size_t)(k0 + j) * df.ws] : 0.0;
      cr[j] = w * sh.red[2 * j];
      ci[j] = w * sh.red[2 * j + 1];
    }
    for (long e = tid; e < N; e += SS_THREADS) {  // un[e] is read next by this thread only
      zc u = un[e];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nk) {
          const zc q = q0[(size_t)j * df.qs + e];
          u.x += q.x * cr[j] - q.y * ci[j];
          u.y += q.x * ci[j] + q.y * cr[j];
        }
      un[e] = u;
    }
  }
}
template <bool DEFL>
__device__ __forceinline__ int bt_diag_body(const BtOp& op, zc* x, zc* U, long N, int kcap_in, double thresh, zc shift, const BtSh& sh,
                                            const BrSh& rs, int* kprev_p, long long* stats, long long flops_per_apply, const BtDefl& df) {
  const int tid = threadIdx.x;
  const bool add_shift = shift.x != 0.0 || shift.y != 0.0;
  const int kcap = (int)min((long)kcap_in, N);
  for (long e = tid; e < N; e += SS_THREADS) U[e] = x[e];
  __syncthreads();
  int napply = 0, nrest = 0;
  int rc = SS_ENOTCONV, kdone = kcap;
  for (int i = 0; i < kcap; ++i) {  // a restart at the end of the body sets i back: at most (max_restarts + 1) kcap passes
    const zc* vi = U + (size_t)i * N;
    const zc* vm = U + (size_t)(i > 0 ? i - 1 : 0) * N;
    zc* un = U + (size_t)(i + 1) * N;
    bt_apply(op, vi, 1.0, un);
    napply += 1;
    if (DEFL) bt_defl_add(df, vi, un, N, sh);
    {  // (Op + shift) v_i, and alpha_i
      double s[1] = {0.0};
      for (long e = tid; e < N; e += SS_THREADS) {
        zc v = un[e];
        const zc b = vi[e];
        if (add_shift) {
          v.x += shift.x * b.x - shift.y * b.y;
          v.y += shift.x * b.y + shift.y * b.x;
          un[e] = v;
        }
        s[0] += b.x * v.x + b.y * v.y;
      }
      wg_reduce(s, sh);
    }
    const double al = sh.red[0];
    const double bprev = i > 0 ? rs.beta[i - 1] : 0.0;
    {
      double s[1] = {0.0};
      for (long e = tid; e < N; e += SS_THREADS) {
        zc u = un[e];
        const zc b = vi[e];
        u.x -= al * b.x;
        u.y -= al * b.y;
        if (i > 0) {
          const zc m = vm[e];
          u.x -= bprev * m.x;
          u.y -= bprev * m.y;
        }
        un[e] = u;
        s[0] += u.x * u.x + u.y * u.y;
      }
      wg_reduce(s, sh);
    }
    const double be = sqrt(sh.red[0]);
    if (be >= SS_EPS) {
      const double inv = 1.0 / be;
      for (long e = tid; e < N; e += SS_THREADS) {  // the same thread wrote un[e] above
        zc u = un[e];
        u.x *= inv; u.y *= inv;
        un[e] = u;
      }
    }
    if (tid == 0) {
      rs.alpha[i] = al;
      rs.beta[i] = be;
    }
    __syncthreads();
    const int k = i + 1;
    if (tid < 64) {  // wave 0: the lowest eigenpair of T_k and the change of the Ritz coefficients
      const bool hint = i > 0;
      const double slack = hint ? fabs(rs.beta[i - 1] * rs.cprev[i - 1]) * 1.0625 : 0.0;
      const double th = bt_trilow(rs.alpha, rs.beta, k, rs.c, rs.dp, rs.dm, hint, hint ? rs.out[0] : 0.0, slack);
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      const double dlt = tid < k ? rs.c[tid] - (tid < i ? rs.cprev[tid] : 0.0) : 0.0;
      const double err = wave_sum64(dlt * dlt);
      if (tid == 0) {
        rs.out[0] = th;
        rs.out[1] = sqrt(err);
      }
    }
    __syncthreads();
    bool done = be < SS_EPS || (long)k == N;
    if (!done && i > 0) done = rs.out[1] < thresh;
    if (done) {
      rc = SS_OK;
      kdone = k;
      break;
    }
    if (k < kcap || nrest >= rs.max_restarts) {
      if (tid < 64) rs.cprev[tid] = rs.c[tid];
      __syncthreads();
      continue;
    }
    // Thick restart with the one retained Ritz vector: u_0 = sum_j c_j v_j renormalised, u_1 = v_kcap.  H u_0 = theta u_0 +
    // s u_1 with s = beta_{kcap-1} c_{kcap-1}, so T stays tridiagonal with alpha_0 = theta and beta_0 = s (signed), and the
    // recurrence goes on at i = 1.  c_prev = e_1 is the old c in the old basis: the stop rule carries across, and so does
    // the hint of bt_trilow (out[0] = theta, slack |s|, the exact residual of u_0).  No apply, no new LDS: one pass over
    // the basis.  Element e is read in every slot and then written in slots 0 and 1 by its owning thread, so there is no
    // barrier between the combination (summed in the order of the final one below) and the copy.
    {
      const zc* vk = U + (size_t)kcap * N;
      zc* u1 = U + (size_t)N;
      double s[1] = {0.0};
      for (long e = tid; e < N; e += SS_THREADS) {
        double re = 0.0, im = 0.0;
        for (int j = 0; j < kcap; ++j) {
          const double cj = rs.c[j];
          const zc v = U[(size_t)j * N + e];
          re += cj * v.x;
          im += cj * v.y;
        }
        const zc nx = vk[e];
        U[e] = make_double2(re, im);
        u1[e] = nx;
        s[0] += re * re + im * im;
      }
      const double sb = rs.beta[kcap - 1] * rs.c[kcap - 1];
      wg_reduce(s, sh);  // its first barrier stands behind every read of c and beta above
      const double inv = 1.0 / sqrt(sh.red[0]);
      for (long e = tid; e < N; e += SS_THREADS) {  // the same thread wrote U[e] above
        zc z = U[e];
        z.x *= inv; z.y *= inv;
        U[e] = z;
      }
      if (tid < 64) rs.cprev[tid] = tid == 0 ? 1.0 : 0.0;
      if (tid == 0) {
        rs.alpha[0] = rs.out[0];
        rs.beta[0] = sb;
      }
      __syncthreads();
    }
    nrest += 1;
    i = 0;  // the loop's ++i makes it 1
  }
  if (rc == SS_OK) {  // x = sum_j c_j v_j, renormalised (get_C_sval_states_norm, _mps_cls.py:1083-1084)
    double s[1] = {0.0};
    for (long e = tid; e < N; e += SS_THREADS) {
      double re = 0.0, im = 0.0;
      for (int j = 0; j < kdone; ++j) {
        const double cj = rs.c[j];
        const zc v = U[(size_t)j * N + e];
        re += cj * v.x;
        im += cj * v.y;
      }
      x[e] = make_double2(re, im);
      s[0] += re * re + im * im;
    }
    wg_reduce(s, sh);
    const double inv = 1.0 / sqrt(sh.red[0]);
    for (long e = tid; e < N; e += SS_THREADS) {  // the same thread wrote x[e] above
      zc z = x[e];
      z.x *= inv; z.y *= inv;
      x[e] = z;
    }
  }
  if (tid == 0) {
    __hip_atomic_store(kprev_p, kdone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    stats[0] += napply;
    stats[2] += (long long)napply * flops_per_apply;
    if (nrest > 0) {
      *rs.rst_total += nrest;
      if (nrest > *rs.rst_most) *rs.rst_most = nrest;
    }
  }
  __syncthreads();
  return rc;
}
__device__ __noinline__ int bt_diag(const BtOp& op, zc* x, zc* U, long N, int kcap_in, double thresh, zc shift, const BtSh& sh,
                                    const BrSh& rs, int* kprev_p, long long* stats, long long flops_per_apply) {
  return bt_diag_body<false>(op, x, U, N, kcap_in, thresh, shift, sh, rs, kprev_p, stats, flops_per_apply, BtDefl{});
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 248 VGPRs, 106 SGPRs, no vector
// register spills, 46 scalar registers spilled around the calls of the stage functions, 320 bytes of private memory per
// lane (the argument blocks the stage functions take by reference: none of it inside a product loop), 23 120 bytes of
// LDS; occupancy 2 waves per SIMD, i.e. one workgroup (replica) per compute unit.  The other kernels compile to the figures
// they had (profiles/batch_relax_resources.txt, batch_relax_restart_resources.txt have the listings).
//
// Excited states by deflation (DEFL, k_batch_relax_defl): with dg.count stored states phi_k (copies of all site tensors,
// the snapshot's layout) and weights w_k per replica, every local solve runs on H_eff + shift + sum_k w_k |q_k><q_k|, q_k
// being phi_k in the replica's current basis at the site: q_k = OL_k[p] . phi_k[p] . OR_k[p + 1]^T with the overlap
// blocks OL_k[b][a][a'] = <replica's left basis state a | phi_k's a'> of bond b (and OR_k the same from the right).  One
// block per slot and bond lives in the replica's part of dg.work: the left block while the centre is at or right of the
// bond, the right block otherwise.  At the start of a launch the workgroup builds the blocks of the side the first
// half-sweep looks at from the tensors as they stand (nothing persists between launches); after every gauge move the
// block of the bond the centre crossed is rewritten from the new A (or B), beside the H block's bt_env.  The stop rule,
// the restarts and the status words are those above; E_n, the lowest Ritz value at site 0, is then the energy PLUS
// sum_k w_k |<phi_k|psi>|^2.
// The overlap products of the deflation, each by the whole workgroup through wg_gemm; U / V: N elements of scratch.
//   left:  T2 (dr x dr) = sum conj(Bra) T Ket, the step of wg_overlap
__device__ __noinline__ void bdf_left(const zc* T, const zc* Ket, const zc* Bra, zc* U, zc* T2, int dl, int d, int dr, zc* tiles) {
  assume_lds(tiles);
  wg_walk_u(T, Ket, U, dl, d * dr, tiles);
  wg_walk_t<true>(Bra, U, T2, dr, dl * d, tiles);
}
//   V[(a,s)][t] = sum_t' A[(a,s)][t'] R[t][t']
__device__ __forceinline__ void wg_mul_rt(const zc* A, const zc* R, zc* V, int rows, int dr, zc* tiles) {
  wg_gemm<true, true>(rows, dr, dr, tiles,
      [&](int m, int k) { return A[(long)m * dr + k]; },
      [&](int k, int n) { return R[(long)n * dr + k]; },
      [&](int m, int n, zc z) { V[(long)m * dr + n] = z; });
}
//   right: T2[r][r'] (dl x dl) = sum_(s,t) conj(Bra[r][(s,t)]) V[r'][(s,t)], V = Ket . T^T; Bra in gauge B, (dl, d, dr) as it lies
__device__ __noinline__ void bdf_right(const zc* T, const zc* Ket, const zc* Bra, zc* V, zc* T2, int dl, int d, int dr, zc* tiles) {
  assume_lds(tiles);
  wg_mul_rt(Ket, T, V, dl * d, dr, tiles);
  const int ddr = d * dr;
  wg_gemm<true, true>(dl, dl, ddr, tiles,
      [&](int m, int k) { const zc z = Bra[(long)m * ddr + k]; return make_double2(z.x, -z.y); },
      [&](int k, int n) { return V[(long)n * ddr + k]; },
      [&](int m, int n, zc z) { T2[(long)m * dl + n] = z; });
}
//   q = OL . phi . OR^T: two products, as bt_keff arranges its own
__device__ __noinline__ void bdf_project(const zc* OL, const zc* OR, const zc* phi, zc* tmp, zc* q, int dl, int d, int dr, zc* tiles) {
  assume_lds(tiles);
  wg_walk_u(OL, phi, tmp, dl, d * dr, tiles);
  wg_mul_rt(tmp, OR, q, dl * d, dr, tiles);
}
// where the block of bond b starts in a slot's blocks (bond L shares the 1 of bond 0), and site p in a stored state
__device__ __forceinline__ size_t bdf_boff(const BatchShape* shp, int L, int b) {
  size_t o = 0;
  if (b < L)
    for (int j = 0; j < b; ++j) o += (size_t)shp[j].dl * shp[j].dl;
  return o;
}
__device__ __forceinline__ size_t bdf_soff(const BatchShape* shp, int p) {
  size_t o = 0;
  for (int j = 0; j < p; ++j) o += (size_t)shp[j].dl * shp[j].d * shp[j].dr;
  return o;
}
// The helpers below take the launch's arguments and work out the replica's own pointers themselves: every value the
// kernel body keeps across their calls costs it registers.  Each counts its flops into the replica's stats.
struct BdfCtx {
  const BatchShape* shp;
  int L, r;
  zc* const* site;
  zc* X;             // N elements of scratch: the X carve of the sweep, free between the applies
  zc* dwork;         // the replica's blocks [count][blk_len], then q_k [count][max_site]
  long long* stats;
};
__device__ __forceinline__ BdfCtx bdf_ctx(const BatchRelaxDeflArgs& gg) {
  const int r = blockIdx.x, L = gg.r.L;
  void* const* tab = gg.r.ptrs + (size_t)r * gg.r.ptr_stride;
  return BdfCtx{gg.r.shp, L, r, reinterpret_cast<zc* const*>(tab), reinterpret_cast<zc*>(tab[6 * L + 2]) + gg.r.plan.o_x,
                gg.d.work + (size_t)r * gg.d.plan.per, gg.r.stats + (size_t)r * 4};
}
// the blocks a launch starts from: right blocks of bonds L-1 .. 1 before a forward half-sweep (sites 1 .. L-1 in gauge
// B), left blocks of bonds 1 .. L-1 before a backward one (sites 0 .. L-2 in gauge A)
__device__ __noinline__ void bdf_build(const BatchRelaxDeflArgs& gg, bool fwd, zc* tiles) {
  const BatchDeflArgs& dg = gg.d;
  const BdfCtx c = bdf_ctx(gg);
  const BatchShape* shp = c.shp;
  const int L = c.L, r = c.r;
  zc* const* site = c.site;
  zc* V = c.X;
  zc* dwork = c.dwork;
  long long* stats = c.stats;
  double fl = 0.0;
  for (int k = 0; k < dg.count; ++k) {
    const zc* phi = dg.slot[k] + (size_t)r * dg.snap_len;
    zc* blk = dwork + (size_t)k * dg.plan.blk_len;
    if (threadIdx.x == 0) blk[0] = make_double2(1.0, 0.0);
    __syncthreads();
    for (int step = 0; step + 1 < L; ++step) {
      const int p = fwd ? L - 1 - step : step;
      const BatchShape s = shp[p];
      const zc* ket = phi + bdf_soff(shp, p);
      if (fwd) bdf_right(blk + bdf_boff(shp, L, p + 1), ket, site[p], V, blk + bdf_boff(shp, L, p), s.dl, s.d, s.dr, tiles);
      else bdf_left(blk + bdf_boff(shp, L, p), ket, site[p], V, blk + bdf_boff(shp, L, p + 1), s.dl, s.d, s.dr, tiles);
      fl += 8.0 * (double)s.dl * s.d * s.dr * (s.dl + s.dr);
    }
  }
  if (threadIdx.x == 0) stats[2] += (long long)fl;
}
// q_k of every slot at site p, into the replica's projected vectors
__device__ __forceinline__ void bdf_site(const BatchRelaxDeflArgs& gg, int p, zc* tiles) {
  const BatchDeflArgs& dg = gg.d;
  const BdfCtx c = bdf_ctx(gg);
  const BatchShape* shp = c.shp;
  const int L = c.L, r = c.r;
  zc* tmp = c.X;
  zc* dwork = c.dwork;
  long long* stats = c.stats;
  const BatchShape s = shp[p];
  const size_t bo = bdf_boff(shp, L, p), bn = bdf_boff(shp, L, p + 1), so = bdf_soff(shp, p);
  for (int k = 0; k < dg.count; ++k) {
    const zc* blk = dwork + (size_t)k * dg.plan.blk_len;
    bdf_project(blk + bo, blk + bn, dg.slot[k] + (size_t)r * dg.snap_len + so, tmp, dwork + dg.plan.o_q + (size_t)k * dg.plan.max_site,
                s.dl, s.d, s.dr, tiles);
  }
  if (threadIdx.x == 0) stats[2] += (long long)dg.count * (long long)(8.0 * (double)s.dl * s.d * s.dr * (s.dl + s.dr));
}
// the deflated solve at site p: q_k of every slot first (op.X is free until the first apply), then bt_diag's text with the
// rank-one terms; 16 N flops per slot and apply come on top of the apply's own
__device__ __noinline__ int bt_diag_defl(const BtOp& op, zc* x, zc* U, long N, int kcap_in, double thresh, zc shift, const BtSh& sh,
                                         const BrSh& rs, int* kprev_p, long long* stats, long long flops_per_apply,
                                         const BatchRelaxDeflArgs& gg, int p) {
  const BatchDeflArgs& dg = gg.d;
  const int r = blockIdx.x;
  bdf_site(gg, p, op.tiles);
  const BtDefl df{dg.count, dg.work + (size_t)r * dg.plan.per + dg.plan.o_q, dg.plan.max_site, dg.w + r, (size_t)gridDim.x};
  return bt_diag_body<true>(op, x, U, N, kcap_in, thresh, shift, sh, rs, kprev_p, stats, flops_per_apply + 16LL * N * dg.count, df);
}
// the block of the bond the centre crossed, of every slot, from the new A (forward: OL_k[p + 1]) or B (backward: OR_k[p])
__device__ __noinline__ void bdf_move(const BatchRelaxDeflArgs& gg, int p, bool fwd, zc* tiles) {
  const BatchDeflArgs& dg = gg.d;
  const BdfCtx c = bdf_ctx(gg);
  const BatchShape* shp = c.shp;
  const int L = c.L, r = c.r;
  const zc* sp = c.site[p];
  zc* V = c.X;
  zc* dwork = c.dwork;
  long long* stats = c.stats;
  const BatchShape s = shp[p];
  const size_t bo = bdf_boff(shp, L, p), bn = bdf_boff(shp, L, p + 1), so = bdf_soff(shp, p);
  for (int k = 0; k < dg.count; ++k) {
    zc* blk = dwork + (size_t)k * dg.plan.blk_len;
    const zc* ket = dg.slot[k] + (size_t)r * dg.snap_len + so;
    if (fwd) bdf_left(blk + bo, ket, sp, V, blk + bn, s.dl, s.d, s.dr, tiles);
    else bdf_right(blk + bn, ket, sp, V, blk + bo, s.dl, s.d, s.dr, tiles);
  }
  if (threadIdx.x == 0) stats[2] += (long long)dg.count * (long long)(8.0 * (double)s.dl * s.d * s.dr * (s.dl + s.dr));
}

template <bool DEFL>
__device__ __forceinline__ void batch_relax_body(const BatchRelaxArgs& g, const BatchRelaxDeflArgs* gg) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ zc s_z[2 * BATCH_MAX_BOND];
  __shared__ double s_d[SS_WAVES * 8 + 8 + BATCH_MAX_BOND + 6 * BATCH_RELAX_MAX_KRYLOV + 2];
  BtSh sh{};
  sh.mats = s_tiles;
  sh.wsh = s_d;
  sh.red = s_d + SS_WAVES * 8;
  sh.gam = sh.red + 8;
  sh.udiag = s_z;
  sh.rdiag = s_z + BATCH_MAX_BOND;
  BrSh rs;
  rs.alpha = sh.gam + BATCH_MAX_BOND;
  rs.beta = rs.alpha + BATCH_RELAX_MAX_KRYLOV;
  rs.c = rs.beta + BATCH_RELAX_MAX_KRYLOV;
  rs.cprev = rs.c + BATCH_RELAX_MAX_KRYLOV;
  rs.dp = rs.cprev + BATCH_RELAX_MAX_KRYLOV;
  rs.dm = rs.dp + BATCH_RELAX_MAX_KRYLOV;
  rs.out = rs.dm + BATCH_RELAX_MAX_KRYLOV;

  const int r = blockIdx.x, tid = threadIdx.x, L = g.L;
  rs.max_restarts = g.max_restarts;
  rs.rst_total = g.total + r;
  rs.rst_most = g.most + r;
  if (g.status[r] != SS_OK) return;  // a replica that failed in an earlier launch of the call does no more work
  void* const* tab = g.ptrs + (size_t)r * g.ptr_stride;
  zc* const* site = reinterpret_cast<zc* const*>(tab);
  zc* const* envL = reinterpret_cast<zc* const*>(tab + L);
  zc* const* envR = reinterpret_cast<zc* const*>(tab + 2 * L + 1);
  const zc* const* w2l = reinterpret_cast<const zc* const*>(tab + 3 * L + 2);
  const zc* const* w2el = reinterpret_cast<const zc* const*>(tab + 4 * L + 2);
  const zc* const* w2er = reinterpret_cast<const zc* const*>(tab + 5 * L + 2);
  zc* scr = reinterpret_cast<zc*>(tab[6 * L + 2]);
  zc* sig = scr + g.plan.o_sig;
  zc* spare = scr + g.plan.o_spare;
  zc* work = scr + g.plan.o_work;
  zc* X = scr + g.plan.o_x;
  zc* Y = scr + g.plan.o_y;
  zc* U = scr + g.plan.o_u;
  int* kprev = g.kprev + (size_t)r * L;
  long long* stats = g.stats + (size_t)r * 4;
  const zc shift = g.shift[r];
  zc* tiles = s_tiles;

  int rc = SS_OK;
  int nstep = 0;
  double e_prev = 0.0;
  bool fwd = g.forward != 0;
  if (DEFL) bdf_build(*gg, fwd, tiles);
  for (int h = 0; h < g.nhalf && rc == SS_OK; ++h, fwd = !fwd) {
    double theta = 0.0;
    for (int step = 0; step < L; ++step) {
      const int p = fwd ? step : L - 1 - step;
      const BatchShape s = g.shp[p];
      const int dl = s.dl, d = s.d, dr = s.dr;
      const long N = (long)dl * d * dr;
      {  // 1. the lowest eigenvector of H_eff + shift in place of the centre tensor
        const long long fl = (long long)(8.0 * ((double)dl * dl * s.ml * d * dr + (double)dl * dr * s.ml * s.mr * d * d +
                                                (double)dl * dr * dr * s.mr * d));
        const BtOp op{s, envL[p], w2l[p], envR[p + 1], 0, 0, X, Y, tiles};
        if (DEFL) {
          rc = bt_diag_defl(op, site[p], U, N, g.kcap, g.thresh, shift, sh, rs, kprev + p, stats, fl, *gg, p);
        } else {
          rc = bt_diag(op, site[p], U, N, g.kcap, g.thresh, shift, sh, rs, kprev + p, stats, fl);
        }
        theta = rs.out[0];
      }
      if (rc != SS_OK || step == L - 1) break;
      if (fwd) {
        // 2. Psi2Asigma, 3. L[p + 1], 5. Psi(p + 1) = sigma . B(p + 1)
        bt_qr(site[p], site[p], dr, 1, sig, dr, 1, dl * d, dr, work, sh);
        bt_env(envL[p], site[p], site[p], (long)d * dr, dr, 1, w2el[p], dl, s.ml, d, dr, s.mr, X, Y, envL[p + 1], tiles);
        if (DEFL) bdf_move(*gg, p, true, tiles);  // OL_k[p + 1] from the new A
        const BatchShape q = g.shp[p + 1];
        zc* nxt = site[p + 1];
        bt_matmul(sig, nxt, spare, nxt, dr, q.d * q.dr, dr, tiles);
      } else {
        // 2. Psi2sigmaB, 3. R[p] from the mirror image of B, 5. Psi(p - 1) = A(p - 1) . sigma
        const int mq = d * dr;
        bt_qr(site[p], site[p], 1, mq, sig, 1, dl, mq, dl, work, sh);
        bt_env(envR[p + 1], site[p], site[p], 1, dr, (long)d * dr, w2er[p], dr, s.mr, d, dl, s.ml, X, Y, envR[p], tiles);
        if (DEFL) bdf_move(*gg, p, false, tiles);  // OR_k[p] from the new B
        const BatchShape q = g.shp[p - 1];
        zc* prv = site[p - 1];
        bt_matmul(prv, sig, spare, prv, q.dl * q.d, dl, dl, tiles);
      }
    }
    if (rc != SS_OK) break;
    if (!fwd && h > 0) {  // a full step ends here; theta is the Ritz value of the solve at site 0, workgroup-uniform
      nstep += 1;
      if (g.energy && tid == 0) {
        g.energy[r] = theta;
        g.steps[r] = nstep;
        if (nstep <= g.hist_len) g.history[(size_t)r * g.hist_len + nstep - 1] = theta;
      }
      const bool stop = g.conv_tol > 0.0 && nstep > 1 && fabs(theta - e_prev) <= g.conv_tol;
      e_prev = theta;
      if (stop) break;
    }
  }
  if (rc != SS_OK && tid == 0) g.status[r] = rc;
}
__global__ __launch_bounds__(SS_THREADS) void k_batch_relax(BatchRelaxArgs g) { batch_relax_body<false>(g, nullptr); }
// Resources of the deflated instance (profiles/batch_deflate_resources.txt): 256 VGPRs, 106 SGPRs, 23 120 bytes of LDS,
// occupancy 2 waves per SIMD as above, 704 bytes of private memory per lane -- and 6 vector and 2 scalar registers spilled
// in this body around the calls of the stage functions, none inside a loop over elements (those are all in functions of
// their own: bdf_left / bdf_right / bdf_project 136 .. 148 VGPRs, bt_defl_add 102, bt_diag_defl 248, no private memory
// beyond their argument blocks).
__global__ __launch_bounds__(SS_THREADS) void k_batch_relax_defl(BatchRelaxDeflArgs g) { batch_relax_body<true>(g.r, &g); }

// <phi_k | psi_r> for every slot k and replica r: workgroup k * B + r walks wg_overlap with the replica as ket and the
// stored state as bra; T, its successor and U lie in the request's own buffer.  Replicas and slots are only read.
__global__ __launch_bounds__(SS_THREADS) void k_batch_defl_overlaps(BatchDeflOvArgs g) {
  __shared__ __attribute__((aligned(16))) zc tiles[2 * BT_TK * BT_LD];
  const int B = g.nrep, k = blockIdx.x / B, r = blockIdx.x - k * B;
  const zc* const* tab = reinterpret_cast<const zc* const*>(g.ptrs + (size_t)r * g.ptr_stride);
  const zc* phi = g.slot[k] + (size_t)r * g.snap_len;
  zc* T = g.buf + (size_t)blockIdx.x * g.buf_len;
  const zc* res = wg_overlap(g.L, g.shp,
      [&](int p, size_t) { return tab[p]; },
      [&](int, size_t soff) { return phi + soff; }, T, T + g.o_t2, T + g.o_u, tiles);
  if (threadIdx.x == 0) {
    const zc z = res[0];
    g.rec[2 * (size_t)blockIdx.x] = z.x;
    g.rec[2 * (size_t)blockIdx.x + 1] = z.y;
  }
}

// test hook: bt_trilow alone, one workgroup of one wave per case
__global__ __launch_bounds__(64) void k_batch_trilow(const double* __restrict__ alpha, const double* __restrict__ beta,
                                                     const int* __restrict__ kk, double* __restrict__ theta, double* __restrict__ vec) {
  __shared__ double s_d[5 * BATCH_RELAX_MAX_KRYLOV];
  const int q = blockIdx.x, lane = threadIdx.x;
  double* a = s_d;
  double* b = a + BATCH_RELAX_MAX_KRYLOV;
  double* c = b + BATCH_RELAX_MAX_KRYLOV;
  a[lane] = alpha[(size_t)q * BATCH_RELAX_MAX_KRYLOV + lane];
  b[lane] = beta[(size_t)q * BATCH_RELAX_MAX_KRYLOV + lane];
  c[lane] = 0.0;
  __syncthreads();
  const double th = bt_trilow(a, b, kk[q], c, c + BATCH_RELAX_MAX_KRYLOV, c + 2 * BATCH_RELAX_MAX_KRYLOV, false, 0.0, 0.0);
  __syncthreads();
  if (lane == 0) theta[q] = th;
  vec[(size_t)q * BATCH_RELAX_MAX_KRYLOV + lane] = c[lane];
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched observables: k_batch_observe, ONE workgroup per replica as above, one record per replica and launch
// (BatchObsArgs in batch_site.h has the record's layout).  The state is the one a batch step leaves: centre at site 0,
// sites 1 .. L-1 right-canonical.
//   norm^2           sum of squares of the centre tensor                                     (Engine::norm)
//   site RDMs        one left-to-right pass of the transfer matrix T (dl x dl, starts as 1) up to the last listed site:
//                    U = T^T C; at a listed site rho[j][j'] = sum_{a',s} U[a'][j][s] conj(C[a'][j'][s]); then
//                    T'[s][s'] = sum_{a',j} U[a'][j][s] conj(C[a'][j][s'])                    (Engine::site_rdm)
//   autocorrelation  the same pass without the conjugate over all L sites: U = T C, T' = C^T U (Engine::autocorr)
//   energy           <C | H_eff C> + shift <C | C> with bt_heff at site 0                     (Engine::expect)
// What is resident where: LDS holds the two operand tiles of wg_gemm and the reduction partials (17 472 bytes); T, its
// successor, U and the X / Y / H C of the H_eff apply live in the observation's own carve of the replica's scratch area
// (global memory, L2-resident), written and re-read by this workgroup only and ordered by workgroup barriers.  The T / U
// products are wg_gemm; the d x d output of a site RDM is NOT (its K = dl dr is up to 4096 and d^2 may be 4): there K
// is split over all 512 threads, four outputs at a time, and wg_reduce finishes in its fixed order.  Every element has
// one owner thread and every sum one order: a record depends neither on B nor on the compute unit.  No atomics.
__device__ __noinline__ void bo_rdm(const zc* U, const zc* C, int dl, int d, int dr, double* out, const BtSh& sh) {
  const int tid = threadIdx.x, K = dl * dr, nout = d * d;
  for (int e0 = 0; e0 < nout; e0 += 4) {
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k < K; k += SS_THREADS) {
      const int a = k / dr, s = k - a * dr;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e0 + q < nout) {
          const int e = e0 + q, j = e / d, jp = e - j * d;
          const zc u = U[((long)a * d + j) * dr + s], c = C[((long)a * d + jp) * dr + s];
          acc[2 * q] += u.x * c.x + u.y * c.y;  // u conj(c)
          acc[2 * q + 1] += u.y * c.x - u.x * c.y;
        }
    }
    wg_reduce(acc, sh);
    if (tid < 8 && 2 * e0 + tid < 2 * nout) out[2 * e0 + tid] = sh.red[tid];
  }
  __syncthreads();
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 194 VGPRs -- those of bt_heff, the
// non-inlined product function shared with k_batch_sweep -- so occupancy 2 waves per SIMD (one workgroup per compute
// unit); no vector or scalar register spills; 128 bytes of private memory per lane (the argument blocks of the calls of
// bo_rdm and bt_heff); 17 472 bytes of LDS.  The aim of 128 VGPRs (two workgroups per compute unit) is missed; the aim of
// no spills inside the product loops is met.  k_batch_mean: 13 VGPRs, no LDS, no private memory.
__global__ __launch_bounds__(SS_THREADS) void k_batch_observe(BatchObsArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ double s_d[SS_WAVES * 8 + 8];
  BtSh sh{};
  sh.mats = s_tiles;
  sh.wsh = s_d;
  sh.red = s_d + SS_WAVES * 8;
  zc* tiles = s_tiles;

  const int r = blockIdx.x, tid = threadIdx.x, L = g.L;
  double* rec = g.rec + (size_t)r * g.rec_len;
  for (long e = tid; e < g.rec_len; e += SS_THREADS) rec[e] = 0.0;
  __syncthreads();
  if (g.status[r] != SS_OK) return;  // a replica that failed: zeros
  void* const* tab = g.ptrs + (size_t)r * g.ptr_stride;
  const zc* const* site = reinterpret_cast<const zc* const*>(tab);
  const zc* const* envL = reinterpret_cast<const zc* const*>(tab + L);
  const zc* const* envR = reinterpret_cast<const zc* const*>(tab + 2 * L + 1);
  const zc* const* w2l = reinterpret_cast<const zc* const*>(tab + 3 * L + 2);
  zc* scr = reinterpret_cast<zc*>(tab[6 * L + 2]) + g.carve;
  zc* T = scr + g.plan.o_t;
  zc* T2 = scr + g.plan.o_t2;
  zc* U = scr + g.plan.o_u;

  const BatchShape s0 = g.shp[0];
  const long N0 = (long)s0.dl * s0.d * s0.dr;
  double n2 = 0.0;
  if (g.what & (BOBS_NORM | BOBS_ENERGY)) {
    const zc* C = site[0];
    double s[1] = {0.0};
    for (long e = tid; e < N0; e += SS_THREADS) { const zc z = C[e]; s[0] += z.x * z.x + z.y * z.y; }
    wg_reduce(s, sh);
    n2 = sh.red[0];
    if ((g.what & BOBS_NORM) && tid == 0) rec[0] = n2;
  }

  if (g.what & BOBS_RDM) {
    if (tid == 0) T[0] = make_double2(1.0, 0.0);
    __syncthreads();
    const int last = g.sites[g.nsites - 1];
    int k = 0;
    long off = BOBS_HEAD;
    for (int p = 0; p <= last; ++p) {
      const BatchShape s = g.shp[p];
      const int dl = s.dl, d = s.d, dr = s.dr, ddr = d * dr;
      const zc* C = site[p];
      // U[a'][(j,s)] = sum_a T[a][a'] C[a][(j,s)]
      wg_gemm<false, false>(dl, ddr, dl, tiles,
          [&](int m, int kk) { return T[(long)kk * dl + m]; },
          [&](int kk, int n) { return C[(long)kk * ddr + n]; },
          [&](int m, int n, zc z) { U[(long)m * ddr + n] = z; });
      if (g.sites[k] == p) {
        bo_rdm(U, C, dl, d, dr, rec + off, sh);
        off += 2L * d * d;
        ++k;
      }
      if (p < last) {
        // T'[s][s'] = sum_(a',j) U[(a',j)][s] conj(C[(a',j)][s'])
        wg_gemm<false, false>(dr, dr, dl * d, tiles,
            [&](int m, int kk) { return U[(long)kk * dr + m]; },
            [&](int kk, int n) { const zc z = C[(long)kk * dr + n]; return make_double2(z.x, -z.y); },
            [&](int m, int n, zc z) { T2[(long)m * dr + n] = z; });
        zc* t = T; T = T2; T2 = t;
      }
    }
  }

  if (g.what & BOBS_AUTOCORR) {
    if (tid == 0) T[0] = make_double2(1.0, 0.0);
    __syncthreads();
    for (int p = 0; p < L; ++p) {
      const BatchShape s = g.shp[p];
      const int dl = s.dl, d = s.d, dr = s.dr, ddr = d * dr;
      const zc* C = site[p];
      // U = T C, T' = C^T U: the overlap walk with bra = conj(ket)
      wg_walk_u(T, C, U, dl, ddr, tiles);
      wg_walk_t<false>(C, U, T2, dr, dl * d, tiles);
      zc* t = T; T = T2; T2 = t;
    }
    if (tid == 0) { const zc z = T[0]; rec[2] = z.x; rec[3] = z.y; }
    __syncthreads();
  }

  if (g.what & BOBS_ENERGY) {
    zc* H = scr + g.plan.o_h;
    const zc* C = site[0];
    bt_heff(s0, envL[0], w2l[0], envR[1], C, 1.0, scr + g.plan.o_x, scr + g.plan.o_y, H, tiles);
    double acc[2] = {0.0, 0.0};
    for (long e = tid; e < N0; e += SS_THREADS) {
      const zc c = C[e], h = H[e];
      acc[0] += c.x * h.x + c.y * h.y;  // conj(c) h
      acc[1] += c.x * h.y - c.y * h.x;
    }
    wg_reduce(acc, sh);
    if (tid == 0) {
      const zc sft = g.shift[r];
      rec[4] = sh.red[0] + sft.x * n2;
      rec[5] = sh.red[1] + sft.y * n2;
    }
  }
}

__global__ __launch_bounds__(256) void k_batch_mean(const double* __restrict__ rec, const double* __restrict__ w,
                                                    double* __restrict__ mean, int nrep, long rec_len, long nrec) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nrec * rec_len) return;
  const long q = idx / rec_len, e = idx - q * rec_len;
  const double* src = rec + (size_t)q * nrep * rec_len + e;
  double acc = 0.0;
  for (int r = 0; r < nrep; ++r) acc += w[r] * src[(size_t)r * rec_len];  // index order: deterministic by construction
  mean[idx] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched multi-site reduced densities: k_batch_density, ONE workgroup per replica as above, every key of the request
// for every replica in one launch (BatchDensArgs in batch_site.h has the envelope and the record's layout).  The state
// is k_batch_observe's: centre at site 0, sites 1 .. L-1 right-canonical, so everything right of a key's last kept site
// drops out.  Per key the arithmetic of Engine::reduced_density: the open physical legs collected so far form an index o
// (row-major over the earlier kept legs), T_o[a][a'] (ket bond, bra bond) is the transfer block of o, T = 1 before site
// 0.  At site p, for each o in turn, U = T_o^T C (bd_tu), then by the key's leg count n at p
//   n = 0            T'_o[s][s'] = sum_(a',j) U[a'][j][s] conj(C[a'][j][s'])                  as the one-site pass
//   n = 2, p < last  T'_(o,j,j')[s][s'] = sum_a' U[a'][j][s] conj(C[a'][j'][s'])               ONE product (d dr) x (d dr)
//                    over K = dl whose store scatters to the (o, j, j', s, s') order -- no permutation pass
//   n = 1, p < last  the same with j' = j only: d products dr x dr over K = dl
//   p = last         rho_o[j][j'] = sum_(a',s) U[a'][j][s] conj(C[a'][j'][s]) by bo_rdm's K-split reduction (n = 2), its
//                    diagonal alone by bd_diag (n = 1), written straight into the record.
// All three T' forms are ONE non-inlined product function, bd_uc, with one wg_gemm in it.
// What is resident where: LDS holds the two operand tiles of wg_gemm and the reduction partials (17 472 bytes, as
// k_batch_observe); U is the observation carve's U buffer (one o at a time); the T_o of a replica and their successors
// are the batch's own device buffer [B][2][need], need = the largest (open legs x bond matrix) a key of the request
// reaches.  Everything is written and re-read by this workgroup only and ordered by workgroup barriers.  Every element
// has one owner thread and every sum one order: a replica's densities depend neither on B nor on the compute unit.  No
// atomics, and every loop is bounded by the shapes and the keys.
//
// U[a'][n] = sum_a T[a][a'] C[a][n], n = (j, s)
__device__ __noinline__ void bd_tu(const zc* T, const zc* C, zc* U, int dl, int ddr, zc* tiles) {
  wg_gemm<false, false>(dl, ddr, dl, tiles,
      [&](int m, int kk) { return T[(long)kk * dl + m]; },
      [&](int kk, int n) { return C[(long)kk * ddr + n]; },
      [&](int m, int n, zc z) { U[(long)m * ddr + n] = z; });
}

// out(m, n) = sum_k U[k * ldk + m] conj(C[k * ldk + n]) for m, n < mn; with m = (jm, sm), n = (jn, sn) in blocks of blk
// the result goes to out[((jm * nb + jn) * blk + sm) * blk + sn]: blk = mn, nb = 1 is a plain row-major mn x mn matrix.
__device__ __noinline__ void bd_uc(const zc* U, const zc* C, zc* out, int mn, int K, long ldk, int blk, int nb, zc* tiles) {
  wg_gemm<false, false>(mn, mn, K, tiles,
      [&](int m, int kk) { return U[kk * ldk + m]; },
      [&](int kk, int n) { const zc z = C[kk * ldk + n]; return make_double2(z.x, -z.y); },
      [&](int m, int n, zc z) {
        const int jm = m / blk, sm = m - jm * blk, jn = n / blk, sn = n - jn * blk;
        out[(((long)jm * nb + jn) * blk + sm) * blk + sn] = z;
      });
}

// out[j] = sum_(a',s) U[a'][j][s] conj(C[a'][j][s]): the diagonal of bo_rdm's matrix, K split the same way
__device__ __noinline__ void bd_diag(const zc* U, const zc* C, int dl, int d, int dr, double* out, const BtSh& sh) {
  const int tid = threadIdx.x, K = dl * dr;
  for (int j0 = 0; j0 < d; j0 += 4) {
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k < K; k += SS_THREADS) {
      const int a = k / dr, s = k - a * dr;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (j0 + q < d) {
          const long at = ((long)a * d + j0 + q) * dr + s;
          const zc u = U[at], c = C[at];
          acc[2 * q] += u.x * c.x + u.y * c.y;  // u conj(c)
          acc[2 * q + 1] += u.y * c.x - u.x * c.y;
        }
    }
    wg_reduce(acc, sh);
    if (tid < 8 && 2 * j0 + tid < 2 * d) out[2 * j0 + tid] = sh.red[tid];
  }
  __syncthreads();
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 148 VGPRs, occupancy 3 waves per
// SIMD (still one workgroup per compute unit); no vector register spills, 13 scalar registers spilled to vector lanes
// around the calls; 112 bytes of private memory per lane (the argument blocks of the calls of the stage functions, none
// of it inside a product loop); 17 472 bytes of LDS.  The aim of no scalar spills is missed; DESIGN.md section 7.3.
__global__ __launch_bounds__(SS_THREADS) void k_batch_density(BatchDensArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ double s_d[SS_WAVES * 8 + 8];
  BtSh sh{};
  sh.mats = s_tiles;
  sh.wsh = s_d;
  sh.red = s_d + SS_WAVES * 8;
  zc* tiles = s_tiles;

  const int r = blockIdx.x, tid = threadIdx.x, L = g.L;
  double* rec = g.rec + (size_t)r * g.rec_len;
  for (long e = (g.zero_head ? 0 : g.dens_off) + tid; e < g.rec_len; e += SS_THREADS) rec[e] = 0.0;
  __syncthreads();
  if (g.status[r] != SS_OK) return;  // a replica that failed: zeros
  void* const* tab = g.ptrs + (size_t)r * g.ptr_stride;
  const zc* const* site = reinterpret_cast<const zc* const*>(tab);
  zc* U = reinterpret_cast<zc*>(tab[6 * L + 2]) + g.carve + g.plan.o_u;
  zc* Ta = g.tbuf + (size_t)r * 2 * g.need;
  zc* Tb = Ta + g.need;
  double* out = rec + g.dens_off;

  for (int k = 0; k < g.nkeys; ++k) {
    const int* legs = g.legs + (size_t)k * L;
    int last = 0;
    for (int p = 0; p < L; ++p)
      if (legs[p]) last = p;
    zc *T = Ta, *T2 = Tb;
    if (tid == 0) T[0] = make_double2(1.0, 0.0);
    __syncthreads();
    long no = 1;
    for (int p = 0; p <= last; ++p) {
      const BatchShape s = g.shp[p];
      const int dl = s.dl, d = s.d, dr = s.dr, ddr = d * dr, n = legs[p];
      const long tl = (long)dl * dl, tr = (long)dr * dr;
      const zc* C = site[p];
      for (long o = 0; o < no; ++o) {
        bd_tu(T + o * tl, C, U, dl, ddr, tiles);
        if (p < last) {
          if (n == 0) bd_uc(U, C, T2 + o * tr, dr, dl * d, dr, dr, 1, tiles);
          else if (n == 2) bd_uc(U, C, T2 + o * d * d * tr, ddr, dl, ddr, dr, d, tiles);
          else
            for (int j = 0; j < d; ++j) bd_uc(U + (long)j * dr, C + (long)j * dr, T2 + (o * d + j) * tr, dr, dl, ddr, dr, 1, tiles);
        } else if (n == 2) {
          bo_rdm(U, C, dl, d, dr, out + o * 2 * d * d, sh);
        } else {
          bd_diag(U, C, dl, d, dr, out + o * 2 * d, sh);
        }
      }
      if (p < last) {
        no *= n == 2 ? d * d : (n == 1 ? d : 1);
        zc* t = T; T = T2; T2 = t;
      } else {
        out += 2 * no * (n == 2 ? d * d : d);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// One-site channels between the two half-sweeps of a time step: k_batch_channel, ONE workgroup per replica as above, one
// launch per time step (the slot of Engine::step's gates: forward half-sweep, maps with the centre at L-1, backward
// half-sweep).  Precondition: the state a forward half-sweep leaves (centre at L-1, sites 0 .. L-2 in gauge A).
//   downward walk  p = L-1 .. lo (the lowest site with a channel): the site's channel acts on the CENTRE tensor; then, for
//                  p > lo, Psi -> sigma B (bt_qr in the backward sweep's roles) and Psi(p-1) = A(p-1) sigma.  No
//                  environment work: the backward half-sweep rebuilds every right block itself.
//   upward walk    p = lo .. L-2: Psi -> A sigma, L[p+1] by bt_env in the forward sweep's roles, Psi(p+1) = sigma B(p+1):
//                  the centre is back at L-1 and every left block is valid.
// A gate is C[a,i,s] = sum_j U[i,j] C[a,j,s], as is.  A jump channel {B_k} picks ONE k per visit: w_k = |B_k C|^2 (the
// centre tensor carries the whole norm, so these are the branch weights of the state), W = sum_k w_k in index order, u
// from the counter generator below, the smallest k whose running sum exceeds u W (if rounding leaves none: the last k
// with w_k > 0), C <- B_k C sqrt(|C|^2 / w_k).  W == 0 is SS_EZERO for that replica.  The Krylov memories are not touched.
// What is resident where: LDS holds the two operand tiles of wg_gemm, the Householder scalars of a gauge move, the
// reduction partials and the K + 1 weights (20 168 bytes); the operators are read from the batch's device array
// (L2-resident, a few hundred bytes a site); sigma, the spare tensor, the QR work matrix and X / Y of the environment
// update are the sweep's carve of the replica's scratch area.  Every element has one owner thread and every sum one order.
__device__ __forceinline__ unsigned long long bc_mix(unsigned long long z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
  z ^= z >> 27; z *= 0x94D049BB133111EBULL;
  z ^= z >> 31;
  return z;
}
// u in [0, 1): a function of (seed, trajectory, step, site) only -- no generator state anywhere
__device__ __forceinline__ double bc_uniform(unsigned long long seed, unsigned long long traj, unsigned long long step, unsigned long long site) {
  const unsigned long long key = bc_mix(bc_mix(bc_mix(seed ^ traj) + step) + site);
  return (double)(key >> 11) * 0x1.0p-53;
}

// C[a,i,s] <- scl * sum_j Bm[i][j] C[a,j,s] by way of tmp; element e belongs to thread e % 512 in both passes
__device__ __noinline__ void bc_apply(const zc* Bm, double scl, zc* C, zc* tmp, int dl, int d, int dr) {
  const int ddr = d * dr;
  const long N = (long)dl * ddr;
  for (long e = threadIdx.x; e < N; e += SS_THREADS) {
    const int a = (int)(e / ddr), rem = (int)(e - (long)a * ddr), i = rem / dr, s = rem - i * dr;
    const zc* col = C + (long)a * ddr + s;
    const zc* row = Bm + (long)i * d;
    double re = 0.0, im = 0.0;
    for (int j = 0; j < d; ++j) {
      const zc b = row[j], c = col[(long)j * dr];
      re = fma(b.x, c.x, re); re = fma(-b.y, c.y, re);
      im = fma(b.x, c.y, im); im = fma(b.y, c.x, im);
    }
    tmp[e] = make_double2(re * scl, im * scl);
  }
  __syncthreads();
  for (long e = threadIdx.x; e < N; e += SS_THREADS) C[e] = tmp[e];
  __syncthreads();
}

// wk[k] = |B_k C|^2 for k < K, wk[BATCH_MAX_JUMP] = |C|^2: the same bits in every thread after the closing barrier.
// Only the norms are kept: B_k C of the picked k is formed a second time by bc_apply (d multiply-adds per element, at
// d <= 16 cheaper than a K-fold copy of the centre tensor in the scratch area).
__device__ __noinline__ void bc_weights(const zc* ops, int K, const zc* C, int dl, int d, int dr, double* wk, const BtSh& sh) {
  const int tid = threadIdx.x, ddr = d * dr;
  const long N = (long)dl * ddr;
  for (int k0 = 0; k0 < K; k0 += 4) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long e = tid; e < N; e += SS_THREADS) {
      const int a = (int)(e / ddr), rem = (int)(e - (long)a * ddr), i = rem / dr, s = rem - i * dr;
      const zc* col = C + (long)a * ddr + s;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (k0 + q < K) {
          const zc* row = ops + ((long)(k0 + q) * d + i) * d;
          double re = 0.0, im = 0.0;
          for (int j = 0; j < d; ++j) {
            const zc b = row[j], c = col[(long)j * dr];
            re = fma(b.x, c.x, re); re = fma(-b.y, c.y, re);
            im = fma(b.x, c.y, im); im = fma(b.y, c.x, im);
          }
          acc[q] += re * re + im * im;
        }
    }
    wg_reduce(acc, sh);
    if (tid < 4 && k0 + tid < K) wk[k0 + tid] = sh.red[tid];
  }
  double s[1] = {0.0};
  for (long e = tid; e < N; e += SS_THREADS) { const zc z = C[e]; s[0] += z.x * z.x + z.y * z.y; }
  wg_reduce(s, sh);
  if (tid == 0) wk[BATCH_MAX_JUMP] = sh.red[0];
  __syncthreads();
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 196 VGPRs -- those of the
// non-inlined bt_env shared with k_batch_sweep -- so occupancy 2 waves per SIMD (one workgroup per compute unit); 98
// SGPRs; no vector or scalar register spills; 160 bytes of private memory per lane (the argument blocks of the calls);
// 20 168 bytes of LDS.
__global__ __launch_bounds__(SS_THREADS) void k_batch_channel(BatchChanArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ zc s_z[2 * BATCH_MAX_BOND];
  __shared__ double s_d[SS_WAVES * 8 + 8 + BATCH_MAX_BOND + BATCH_MAX_JUMP + 1];
  BtSh sh{};
  sh.mats = s_tiles;
  sh.udiag = s_z; sh.rdiag = s_z + BATCH_MAX_BOND;
  sh.wsh = s_d; sh.red = sh.wsh + SS_WAVES * 8; sh.gam = sh.red + 8;
  double* wk = sh.gam + BATCH_MAX_BOND;  // [BATCH_MAX_JUMP + 1]
  zc* tiles = s_tiles;

  const int r = blockIdx.x, tid = threadIdx.x, L = g.L;
  if (g.status[r] != SS_OK) return;  // a replica that failed in an earlier launch of the call does no more work
  void* const* tab = g.ptrs + (size_t)r * g.ptr_stride;
  zc* const* site = reinterpret_cast<zc* const*>(tab);
  zc* const* envL = reinterpret_cast<zc* const*>(tab + L);
  const zc* const* w2el = reinterpret_cast<const zc* const*>(tab + 4 * L + 2);
  zc* scr = reinterpret_cast<zc*>(tab[6 * L + 2]);
  zc* sig = scr + g.plan.o_sig;
  zc* spare = scr + g.plan.o_spare;
  zc* work = scr + g.plan.o_work;
  zc* X = scr + g.plan.o_x;
  zc* Y = scr + g.plan.o_y;
  const int lo = g.lo;

  int rc = SS_OK;
  for (int p = L - 1; p >= lo; --p) {
    const BatchShape s = g.shp[p];
    const int dl = s.dl, d = s.d, dr = s.dr;
    const BatchChanSite ch = g.chan[p];
    const zc* ops = g.ops + ch.off;
    if (ch.kind == BCH_GATE) {
      bc_apply(ops, 1.0, site[p], spare, dl, d, dr);
    } else if (ch.kind == BCH_JUMP) {
      const int K = ch.nops;
      bc_weights(ops, K, site[p], dl, d, dr, wk, sh);
      double W = 0.0;
      for (int k = 0; k < K; ++k) W += wk[k];
      if (!(W > 0.0)) { rc = SS_EZERO; break; }
      const double u = bc_uniform(g.seed, g.ids[r], (unsigned long long)g.step, (unsigned long long)p);
      const double thr = u * W;
      int pick = -1, lastpos = 0;
      double run = 0.0;
      for (int k = 0; k < K; ++k) {
        run += wk[k];
        if (wk[k] > 0.0) lastpos = k;
        if (pick < 0 && run > thr) pick = k;
      }
      if (pick < 0) pick = lastpos;
      const double scl = sqrt(wk[BATCH_MAX_JUMP] / wk[pick]);
      bc_apply(ops + (long)pick * d * d, scl, site[p], spare, dl, d, dr);  // its barriers order the reads of wk above
      if (tid == 0) g.counts[((size_t)r * L + p) * BATCH_MAX_JUMP + pick] += 1;
    }
    if (p > lo) {
      // Psi2sigmaB and Psi(p - 1) = A(p - 1) . sigma, as the backward sweep
      const int mq = d * dr;
      bt_qr(site[p], site[p], 1, mq, sig, 1, dl, mq, dl, work, sh);
      const BatchShape q = g.shp[p - 1];
      zc* prv = site[p - 1];
      bt_matmul(prv, sig, spare, prv, q.dl * q.d, dl, dl, tiles);
    }
  }
  if (rc == SS_OK)
    for (int p = lo; p < L - 1; ++p) {
      const BatchShape s = g.shp[p];
      const int dl = s.dl, d = s.d, dr = s.dr;
      // Psi2Asigma, L[p + 1], Psi(p + 1) = sigma . B(p + 1), as the forward sweep
      bt_qr(site[p], site[p], dr, 1, sig, dr, 1, dl * d, dr, work, sh);
      bt_env(envL[p], site[p], site[p], (long)d * dr, dr, 1, w2el[p], dl, s.ml, d, dr, s.mr, X, Y, envL[p + 1], tiles);
      const BatchShape q = g.shp[p + 1];
      zc* nxt = site[p + 1];
      bt_matmul(sig, nxt, spare, nxt, dr, q.d * q.dr, dr, tiles);
    }
  if (rc != SS_OK && tid == 0) g.status[r] = rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// Time-dependent one-site fields: k_batch_field, ONE workgroup per replica, one launch per time step while at least one
// field is set, between the forward half-sweep and the channel launch.  H(t) = H0 + sum_p a_p(t) G_p with G_p = V diag(g) V^+
// Hermitian (decomposed on the host: the device holds V and g and nothing else) and a_p real: in the symmetric splitting
// of a time step the term is the one-site unitary exp(-i dt a_p G_p) with a_p taken at the step's midpoint.
// Precondition and result: the state a forward half-sweep leaves (centre at L-1, sites 0 .. L-2 in gauge A, left blocks
// valid).  A unitary on the physical index of an isometry leaves it an isometry, so there is NO gauge move -- no QR, no
// sigma, no absorb: for every site p with a field, ascending,
//   amplitude  thread 0: a table entry (entry `clock` of the site's table, shared or the replica's own row; 0 past its end)
//              or the site's Ornstein-Uhlenbeck value xi (xi = sigma z when clock == 0, else decay xi + innov z with
//              z = sqrt(-2 log1p(-u1)) cos(2 pi u2), u1 / u2 = bc_uniform(seed, id, step, 2L + 2p / 2L + 2p + 1): the keys
//              from 2L on meet neither the one-site jump keys 0 .. L-1 nor the pair keys L .. 2L-2); it stores xi and
//              the applied amplitude -- both written by this workgroup only -- and publishes a through LDS
//   phases     phi_k = exp(-i dt a g_k), thread k < d, in LDS
//   unitary    T[a,k,s] = phi_k sum_j conj(V[j][k]) C[a,j,s] into the spare tensor, then C[a,i,s] = sum_k V[i][k] T[a,k,s]:
//              j, then k, ascending, fused multiply-adds; element e belongs to thread e % 512 in both passes; no d x d
//              matrix per replica is ever formed
// and then L[p+1] for p = lo .. L-2 (lo: the lowest site with a field) by bt_env in the forward sweep's roles, as the
// upward walk of k_batch_channel.  An amplitude that is exactly 0 (a table past its end, sigma = 0) skips its site: exp(0)
// is the identity, the tensor keeps its bits, and lo is the lowest site whose amplitude was not 0 -- none: no block is
// rebuilt.  The amplitude is the replica's own number, the same in every thread, so the branch is uniform.  No atomics, nothing waits on another workgroup, every loop is bounded by the shapes.
__device__ __noinline__ void bf_rotate(const zc* V, const zc* phi, zc* C, zc* tmp, int dl, int d, int dr) {
  const int ddr = d * dr;
  const long N = (long)dl * ddr;
  for (long e = threadIdx.x; e < N; e += SS_THREADS) {
    const int a = (int)(e / ddr), rem = (int)(e - (long)a * ddr), k = rem / dr, s = rem - k * dr;
    const zc* col = C + (long)a * ddr + s;
    double re = 0.0, im = 0.0;
    for (int j = 0; j < d; ++j) {  // conj(V[j][k]) C[a,j,s]
      const zc v = V[(long)j * d + k], c = col[(long)j * dr];
      re = fma(v.x, c.x, re); re = fma(v.y, c.y, re);
      im = fma(v.x, c.y, im); im = fma(-v.y, c.x, im);
    }
    const zc f = phi[k];
    tmp[e] = make_double2(fma(f.x, re, -f.y * im), fma(f.x, im, f.y * re));
  }
  __syncthreads();
  for (long e = threadIdx.x; e < N; e += SS_THREADS) {
    const int a = (int)(e / ddr), rem = (int)(e - (long)a * ddr), i = rem / dr, s = rem - i * dr;
    const zc* col = tmp + (long)a * ddr + s;
    const zc* row = V + (long)i * d;
    double re = 0.0, im = 0.0;
    for (int k = 0; k < d; ++k) {
      const zc v = row[k], c = col[(long)k * dr];
      re = fma(v.x, c.x, re); re = fma(-v.y, c.y, re);
      im = fma(v.x, c.y, im); im = fma(v.y, c.x, im);
    }
    C[e] = make_double2(re, im);
  }
  __syncthreads();
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 196 VGPRs -- those of the
// non-inlined bt_env shared with k_batch_sweep -- so occupancy 2 waves per SIMD (one workgroup per compute unit); 106
// SGPRs; no vector or scalar register spills; no private memory; 17 928 bytes of LDS (the tiles of bt_env, d phases, the
// amplitude).  This caller of bt_env moved no figure of k_batch_sweep, k_batch_channel, k_batch_pair or any other kernel
// of this file (profiles/batch_field_probe.txt), so it needs no instance of its own.
__global__ __launch_bounds__(SS_THREADS) void k_batch_field(BatchFieldArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ zc s_phi[BATCH_FIELD_MAX_D];
  __shared__ double s_amp;
  zc* tiles = s_tiles;

  const int r = blockIdx.x, tid = threadIdx.x, L = g.L;
  if (g.status[r] != SS_OK) return;  // a replica that failed in an earlier launch of the call does no more work
  void* const* tab = g.ptrs + (size_t)r * g.ptr_stride;
  zc* const* site = reinterpret_cast<zc* const*>(tab);
  zc* const* envL = reinterpret_cast<zc* const*>(tab + L);
  const zc* const* w2el = reinterpret_cast<const zc* const*>(tab + 4 * L + 2);
  zc* scr = reinterpret_cast<zc*>(tab[6 * L + 2]);
  zc* spare = scr + g.plan.o_spare;
  zc* X = scr + g.plan.o_x;
  zc* Y = scr + g.plan.o_y;
  int lo = -1;  // the lowest site this replica rotated in this step (>= g.lo)

  for (int p = 0; p < L; ++p) {
    const BatchFieldSite f = g.fld[p];
    if (f.kind == BFLD_NONE) {
      if (tid == 0) g.amp[(size_t)r * L + p] = 0.0;
      continue;
    }
    const BatchShape s = g.shp[p];
    if (tid == 0) {
      double a = 0.0;
      if (f.kind == BFLD_TABLE) {
        if (g.clock < f.ntab) a = g.tables[f.off_t + (f.per_replica ? (long long)r * f.ntab : 0LL) + g.clock];
      } else {
        const unsigned long long key = 2ULL * (unsigned long long)L + 2ULL * (unsigned long long)p;
        const double u1 = bc_uniform(g.seed, g.ids[r], (unsigned long long)g.step, key);
        const double u2 = bc_uniform(g.seed, g.ids[r], (unsigned long long)g.step, key + 1);
        const double z = sqrt(-2.0 * log1p(-u1)) * cos(6.283185307179586 * u2);
        double* xi = g.xi + (size_t)r * L + p;
        a = g.clock == 0 ? f.sigma * z : fma(g.decay[2 * p], *xi, g.decay[2 * p + 1] * z);
        *xi = a;
      }
      g.amp[(size_t)r * L + p] = a;
      s_amp = a;
    }
    __syncthreads();
    const double a = s_amp;
    __syncthreads();  // every thread has its copy: thread 0 may publish the next site's
    if (a == 0.0) continue;  // exp(0) is the identity exactly: the tensor keeps its bits (a pulse that is over costs nothing)
    if (lo < 0) lo = p;
    if (tid < f.d) {
      const double th = -g.dt * a * g.evals[f.off_g + tid];
      double sn, cs;
      sincos(th, &sn, &cs);
      s_phi[tid] = make_double2(cs, sn);
    }
    __syncthreads();
    bf_rotate(g.vecs + f.off_v, s_phi, site[p], spare, s.dl, s.d, s.dr);  // its closing barrier frees s_phi
  }
  if (lo < 0) return;  // nothing was rotated: every left block is still valid
  for (int p = lo; p < L - 1; ++p) {
    const BatchShape s = g.shp[p];
    bt_env(envL[p], site[p], site[p], (long)s.d * s.dr, s.dr, 1, w2el[p], s.dl, s.ml, s.d, s.dr, s.mr, X, Y, envL[p + 1], tiles);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same walk with nearest-neighbour (pair) channels: k_batch_pair, ONE workgroup per replica, one launch per time step
// in the place of k_batch_channel whenever a pair channel is set (k_batch_channel itself is untouched and stays in use
// otherwise).  Walking down with the centre at p the one-site channel of p acts as above; then, if bond (p-1, p) carries
// a pair channel, it takes the place of that step's bt_qr + absorb:
//   merge   theta[(a,i)][(j,s)] = sum_b A(p-1)[(a,i)][b] C(p)[b][(j,s)]                       (wg_gemm; m x n, m = dl d_{p-1},
//           n = d_p dr, both <= BATCH_PAIR_MAX_DIM)
//   apply   theta <- Op theta on (i, j); a jump channel first picks its operator by the rule of the one-site channel, with
//           w_k = |B_k theta|^2 computed directly and the uniform of "site" L + (p-1)         (bp_weights / bp_apply)
//   split   theta ~ C'(p-1) . B(p), B(p) with r = dl(p) orthonormal rows (the bond keeps its dimension): a one-sided
//           (Hestenes) Jacobi SVD on the ROWS of a work copy of theta -- pairs of rows in a fixed round-robin order are
//           rotated until all are mutually orthogonal (|<x, y>|^2 <= BP_TOL2 |x|^2 |y|^2); the rows are then sigma_j v_j^+,
//           the r of largest norm, normalised, are B(p), and C'(p-1) = theta B(p)^+ from the kept copy: no U, no V.
//           Rows whose norm^2 is <= BP_TINY |theta|^2 (|theta|^2 lies between the largest sigma^2 and m times it; a
//           rank-deficient theta: a product start padded to D) are rounding noise: those among the selected r are
//           replaced by an orthonormal completion (bp_select), so B(p) B(p)^+ = 1 whatever the rank.  A row is left out
//           of the ROTATIONS only at or below BP_FREEZE |theta|^2, the unit roundoff of |theta| itself (with more rows
//           than columns the surplus rows shrink towards 0 and would rotate for ever).  The two floors are apart on
//           purpose: a row frozen at 1e-14 |theta| may still carry a part of a direction whose sigma lies just above,
//           and some eighty such rows hid 3e-14 |theta| of a singular value at 127 x 65 and 128 x 128
//           (tests/test_gpu_batch_blocks.py); at the roundoff floor all of them together hold 1e-15 |theta| at most.
// After a jump C' is rescaled so that the norm after the split is the norm before the jump (operator and truncation
// together); after a gate nothing is rescaled and the discarded weight sum_{j>r} sigma_j^2 / sum_j sigma_j^2 of every
// split is added to disc[replica] by thread 0.  A split that does not converge in BATCH_PAIR_MAX_SWEEPS sweeps is
// SS_ENOTCONV for that replica only.
// What is resident where: theta and its work copy are the first 2 m n elements of the Krylov-basis carve of the scratch
// area (idle during the walk; global memory, L2-resident), written and re-read by this workgroup only between workgroup
// barriers.  LDS: the operand tiles of wg_gemm, the Householder scalars, the reduction partials and weights of
// k_batch_channel, and for the split the rotation scalars of a round (c, s, phase per pair), the row norms, their ranks,
// the selection and the coefficients of the completion.  A round is two phases with a barrier each: the wave that owns
// a pair forms its three inner products (lane l holds columns l and l + 64; wave tree) and publishes the rotation, then
// element (pair, column) is rotated by thread (pair * n + column) % 512.  Every element has one owner per phase and
// every sum one order; no atomics; the loops are bounded by the shapes and BATCH_PAIR_MAX_SWEEPS.
constexpr double BP_TOL2 = 1.6e-29;  // (4e-15)^2: sqrt(128) eps = 2.5e-15 is what a 128-term inner product carries
constexpr double BP_TINY = 1e-28;    // (1e-14)^2: a row this small against |theta| is rounding noise, not a direction
constexpr double BP_FREEZE = 1e-32;  // (1e-16)^2: a row this small against |theta| takes no part in the rotations

struct BpSh {
  double* rot;   // [4 * BATCH_PAIR_MAX_DIM / 2]  c, s, phase (re, im) of the round's pairs; s == 0: no rotation
  double* nrm;   // [BATCH_PAIR_MAX_DIM] squared row norms after the last sweep
  double* res;   // [BATCH_PAIR_MAX_DIM] completion: 1 - sum_k |B_k[c]|^2
  double* scal;  // [3] kept weight sum_{j<=r} sigma_j^2, discarded fraction, BP_TINY |theta|^2
  zc* h;         // [BATCH_MAX_BOND] completion: <B_k | v>
  int* rank;     // [BATCH_PAIR_MAX_DIM]
  int* sel;      // [BATCH_MAX_BOND] rows in descending order of norm
  int* flag;     // [2] a rotation happened in this sweep; number of selected rows that are kept as they are
};

// the selection rule of a jump channel on the weights wk[0 .. K): W in index order, the smallest k whose running sum
// exceeds u W, else the last k with w_k > 0; -1 when W == 0
__device__ __forceinline__ int bc_pick(const double* wk, int K, double u) {
  double W = 0.0;
  for (int k = 0; k < K; ++k) W += wk[k];
  if (!(W > 0.0)) return -1;
  const double thr = u * W;
  int pick = -1, lastpos = 0;
  double run = 0.0;
  for (int k = 0; k < K; ++k) {
    run += wk[k];
    if (wk[k] > 0.0) lastpos = k;
    if (pick < 0 && run > thr) pick = k;
  }
  return pick < 0 ? lastpos : pick;
}

// the pair of round t that slot k of the round-robin (circle) schedule over mp = 2 np players holds
__device__ __forceinline__ void bp_pair(int k, int t, int mp, int& i, int& j) {
  const int ring = mp - 1;
  if (k == 0) { i = ring; j = t; return; }
  i = t + k; if (i >= ring) i -= ring;
  j = t - k; if (j < 0) j += ring;
}

// T[(a,i)][(j,s)] = sum_b A[(a,i)][b] C[b][(j,s)]
__device__ __noinline__ void bp_merge(const zc* A, const zc* C, zc* T, int m, int n, int r, zc* tiles) {
  wg_gemm<true, false>(m, n, r, tiles,
      [&](int mm, int k) { return A[(long)mm * r + k]; },
      [&](int k, int nn) { return C[(long)k * n + nn]; },
      [&](int mm, int nn, zc z) { T[(long)mm * n + nn] = z; });
}

// wk[k] = |B_k T|^2 for k < K, wk[BATCH_MAX_JUMP] = |T|^2, B_k (d0 d1) x (d0 d1) on the legs (i, j) of T[a][i][j][s]:
// bc_weights with d0 d1 in the place of d
__device__ __noinline__ void bp_weights(const zc* ops, int K, const zc* T, int dl, int d0, int d1, int dr, double* wk, const BtSh& sh) {
  const int tid = threadIdx.x, n = d1 * dr, dd = d0 * d1;
  const long N = (long)dl * d0 * n;
  for (int k0 = 0; k0 < K; k0 += 4) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long e = tid; e < N; e += SS_THREADS) {
      const int row = (int)(e / n), col = (int)(e - (long)row * n), a = row / d0, i = row - a * d0, j = col / dr, s = col - j * dr;
      const zc* src = T + (long)a * d0 * n + s;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (k0 + q < K) {
          const zc* oprow = ops + ((long)(k0 + q) * dd + i * d1 + j) * dd;
          double re = 0.0, im = 0.0;
          for (int ip = 0; ip < d0; ++ip)
            for (int jp = 0; jp < d1; ++jp) {
              const zc b = oprow[ip * d1 + jp], c = src[(long)ip * n + jp * dr];
              re = fma(b.x, c.x, re); re = fma(-b.y, c.y, re);
              im = fma(b.x, c.y, im); im = fma(b.y, c.x, im);
            }
          acc[q] += re * re + im * im;
        }
    }
    wg_reduce(acc, sh);
    if (tid < 4 && k0 + tid < K) wk[k0 + tid] = sh.red[tid];
  }
  double s1[1] = {0.0};
  for (long e = tid; e < N; e += SS_THREADS) { const zc z = T[e]; s1[0] += z.x * z.x + z.y * z.y; }
  wg_reduce(s1, sh);
  if (tid == 0) wk[BATCH_MAX_JUMP] = sh.red[0];
  __syncthreads();
}

// T1[a,i,j,s] = sum_(i',j') Op[(i,j)][(i',j')] T0[a,i',j',s], then T0 <- T1 (the work copy of the split); element e
// belongs to thread e % 512 in both passes
__device__ __noinline__ void bp_apply(const zc* Op, zc* T0, zc* T1, int dl, int d0, int d1, int dr) {
  const int n = d1 * dr, dd = d0 * d1;
  const long N = (long)dl * d0 * n;
  for (long e = threadIdx.x; e < N; e += SS_THREADS) {
    const int row = (int)(e / n), col = (int)(e - (long)row * n), a = row / d0, i = row - a * d0, j = col / dr, s = col - j * dr;
    const zc* src = T0 + (long)a * d0 * n + s;
    const zc* oprow = Op + (long)(i * d1 + j) * dd;
    double re = 0.0, im = 0.0;
    for (int ip = 0; ip < d0; ++ip)
      for (int jp = 0; jp < d1; ++jp) {
        const zc b = oprow[ip * d1 + jp], c = src[(long)ip * n + jp * dr];
        re = fma(b.x, c.x, re); re = fma(-b.y, c.y, re);
        im = fma(b.x, c.y, im); im = fma(b.y, c.x, im);
      }
    T1[e] = make_double2(re, im);
  }
  __syncthreads();
  for (long e = threadIdx.x; e < N; e += SS_THREADS) T0[e] = T1[e];
  __syncthreads();
}

// One-sided Jacobi on the rows of T (m x n, row-major, in place): on return (SS_OK) the rows are mutually orthogonal and
// ps.nrm[i] = |row i|^2.  With g = <x, y> = sum_c x[c] conj(y[c]) = |g| e^(i phi), a = |x|^2, b = |y|^2 the rotation is
// x' = c x + s e^(i phi) y, y' = -s x + c e^(i phi) y, t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), zeta = (a - b) / 2|g|.
__device__ __noinline__ int bp_jacobi(zc* T, int m, int n, const BpSh& ps, const BtSh& sh) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int mp = (m + 1) & ~1, np = mp >> 1;
  double tiny;
  {  // |T|^2 is invariant under the rotations: the scale of "zero" for the whole split
    double s1[1] = {0.0};
    for (long e = tid; e < (long)m * n; e += SS_THREADS) { const zc z = T[e]; s1[0] += z.x * z.x + z.y * z.y; }
    wg_reduce(s1, sh);
    tiny = BP_FREEZE * sh.red[0];
    if (tid == 0) ps.scal[2] = BP_TINY * sh.red[0];  // bp_select's floor
  }
  int rc = SS_ENOTCONV;
  for (int sweep = 0; sweep < BATCH_PAIR_MAX_SWEEPS; ++sweep) {
    if (tid == 0) ps.flag[0] = 0;
    __syncthreads();
    for (int t = 0; t < mp - 1; ++t) {
      for (int k = w; k < np; k += SS_WAVES) {  // the wave that owns slot k: inner products, rotation scalars
        int i, j;
        bp_pair(k, t, mp, i, j);
        double c = 1.0, s = 0.0, px = 1.0, py = 0.0;
        if (i < m && j < m) {  // m odd: the slot with the padding player rests
          const zc* x = T + (long)i * n;
          const zc* y = T + (long)j * n;
          double a = 0.0, b = 0.0, gr = 0.0, gi = 0.0;
          for (int cc = lane; cc < n; cc += 64) {
            const zc zx = x[cc], zy = y[cc];
            a += zx.x * zx.x + zx.y * zx.y;
            b += zy.x * zy.x + zy.y * zy.y;
            gr += zx.x * zy.x + zx.y * zy.y;  // x conj(y)
            gi += zx.y * zy.x - zx.x * zy.y;
          }
          a = __shfl(wave_sum64(a), 0, 64);
          b = __shfl(wave_sum64(b), 0, 64);
          gr = __shfl(wave_sum64(gr), 0, 64);
          gi = __shfl(wave_sum64(gi), 0, 64);
          const double g2 = gr * gr + gi * gi;
          if (g2 > BP_TOL2 * a * b && a > tiny && b > tiny) {  // a row at the roundoff of |theta| takes no part
            const double ag = sqrt(g2), zeta = (a - b) / (2.0 * ag);
            const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            c = 1.0 / sqrt(1.0 + tt * tt);
            s = c * tt;
            px = gr / ag;
            py = gi / ag;
          }
        }
        if (lane == 0) {
          ps.rot[4 * k] = c; ps.rot[4 * k + 1] = s; ps.rot[4 * k + 2] = px; ps.rot[4 * k + 3] = py;
          if (s != 0.0) ps.flag[0] = 1;  // the same value from every writer
        }
      }
      __syncthreads();
      for (int e = tid; e < np * n; e += SS_THREADS) {  // element (slot, column): both rows of the slot at that column
        const int k = e / n, cc = e - k * n;
        const double s = ps.rot[4 * k + 1];
        if (s == 0.0) continue;
        const double c = ps.rot[4 * k], px = ps.rot[4 * k + 2], py = ps.rot[4 * k + 3];
        int i, j;
        bp_pair(k, t, mp, i, j);
        const zc zx = T[(long)i * n + cc], zy = T[(long)j * n + cc];
        const double yr = px * zy.x - py * zy.y, yi = px * zy.y + py * zy.x;
        T[(long)i * n + cc] = make_double2(c * zx.x + s * yr, c * zx.y + s * yi);
        T[(long)j * n + cc] = make_double2(c * yr - s * zx.x, c * yi - s * zx.y);
      }
      __syncthreads();
    }
    const int any = ps.flag[0];
    __syncthreads();  // everyone has read the flag before the next sweep resets it
    if (!any) { rc = SS_OK; break; }
  }
  for (int i = w; i < m; i += SS_WAVES) {
    double a = 0.0;
    for (int cc = lane; cc < n; cc += 64) { const zc z = T[(long)i * n + cc]; a += z.x * z.x + z.y * z.y; }
    a = wave_sum64(a);
    if (lane == 0) ps.nrm[i] = a;
  }
  __syncthreads();
  return rc;
}

// Bp (r x n) from the orthogonal rows of T (m x n, squared norms ps.nrm): the r rows of largest norm (ties: the lower
// index first), normalised; those of them at or below BP_TINY |theta|^2 (ps.scal[2]) are replaced one after the other by
// the unit vector e_c furthest from the span so far (largest 1 - sum_k |B_k[c]|^2 >= 1 / n, the lowest c on a tie),
// orthogonalised against it twice (classical Gram-Schmidt) and normalised.  ps.scal: kept weight, discarded fraction.
// This is the one text of the selection; bp_select below is the function k_batch_pair calls.
__device__ __forceinline__ void bp_select_body(const zc* T, zc* Bp, int m, int n, int r, const BpSh& ps, const BtSh& sh) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < r) ps.sel[tid] = tid;  // in range whatever the norms are (NaN compares false everywhere)
  __syncthreads();
  if (tid < m) {
    const double mine = ps.nrm[tid];
    int rk = 0;
    for (int j = 0; j < m; ++j) {
      const double v = ps.nrm[j];
      rk += (v > mine || (v == mine && j < tid)) ? 1 : 0;
    }
    ps.rank[tid] = rk;
    if (rk < r) ps.sel[rk] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0, disc = 0.0, kept = 0.0;
    for (int i = 0; i < m; ++i) {
      tot += ps.nrm[i];
      if (ps.rank[i] >= r) disc += ps.nrm[i];
    }
    const double tiny = ps.scal[2];
    int nz = 0;
    for (int k = 0; k < r; ++k) {
      const double v = ps.nrm[ps.sel[k]];
      kept += v;
      if (v > tiny) nz = k + 1;  // descending: the kept rows are the first nz
    }
    ps.scal[0] = kept;
    ps.scal[1] = tot > 0.0 ? disc / tot : 0.0;
    ps.flag[1] = nz;
  }
  __syncthreads();
  const int nz = ps.flag[1];
  for (int e = tid; e < r * n; e += SS_THREADS) {
    const int k = e / n, cc = e - k * n;
    zc z = make_double2(0.0, 0.0);
    if (k < nz) {
      const int i = ps.sel[k];
      const double inv = 1.0 / sqrt(ps.nrm[i]);
      z = T[(long)i * n + cc];
      z.x *= inv; z.y *= inv;
    }
    Bp[e] = z;
  }
  __syncthreads();
  for (int k = nz; k < r; ++k) {  // the orthonormal completion, one row at a time (r <= n: there is always room)
    if (tid < n) {
      double acc = 1.0;
      for (int kk = 0; kk < k; ++kk) { const zc z = Bp[(long)kk * n + tid]; acc -= z.x * z.x + z.y * z.y; }
      ps.res[tid] = acc;
    }
    __syncthreads();
    int cs = 0;
    double best = ps.res[0];
    for (int cc = 1; cc < n; ++cc) {
      const double v = ps.res[cc];
      if (v > best) { best = v; cs = cc; }
    }
    if (tid < n) {  // v = e_cs - sum_kk B_kk conj(B_kk[cs])
      double re = tid == cs ? 1.0 : 0.0, im = 0.0;
      for (int kk = 0; kk < k; ++kk) {
        const zc b = Bp[(long)kk * n + tid], q = Bp[(long)kk * n + cs];
        re -= b.x * q.x + b.y * q.y;
        im -= b.y * q.x - b.x * q.y;
      }
      Bp[(long)k * n + tid] = make_double2(re, im);
    }
    __syncthreads();
    for (int kk = w; kk < k; kk += SS_WAVES) {  // h_kk = <B_kk | v>
      double hr = 0.0, hi = 0.0;
      for (int cc = lane; cc < n; cc += 64) {
        const zc b = Bp[(long)kk * n + cc], v = Bp[(long)k * n + cc];
        hr += b.x * v.x + b.y * v.y;
        hi += b.x * v.y - b.y * v.x;
      }
      hr = wave_sum64(hr);
      hi = wave_sum64(hi);
      if (lane == 0) ps.h[kk] = make_double2(hr, hi);
    }
    __syncthreads();
    zc v = make_double2(0.0, 0.0);
    double s1[1] = {0.0};
    if (tid < n) {
      v = Bp[(long)k * n + tid];
      for (int kk = 0; kk < k; ++kk) {
        const zc hh = ps.h[kk], b = Bp[(long)kk * n + tid];
        v.x -= hh.x * b.x - hh.y * b.y;
        v.y -= hh.x * b.y + hh.y * b.x;
      }
      s1[0] = v.x * v.x + v.y * v.y;
    }
    wg_reduce(s1, sh);
    const double inv = 1.0 / sqrt(sh.red[0]);
    if (tid < n) Bp[(long)k * n + tid] = make_double2(v.x * inv, v.y * inv);
    __syncthreads();
  }
}
__device__ __noinline__ void bp_select(const zc* T, zc* Bp, int m, int n, int r, const BpSh& ps, const BtSh& sh) {
  bp_select_body(T, Bp, m, n, r, ps, sh);
}
// k_batch_block's instance of the same text, as bt_env_fwd_blk: with a second caller the LDS addresses in ps and sh stop being
// constants of bp_select, and k_batch_pair spilled 25 scalar registers around its calls instead of 15
__device__ __noinline__ void bp_select_blk(const zc* T, zc* Bp, int m, int n, int r, const BpSh& ps, const BtSh& sh) {
  bp_select_body(T, Bp, m, n, r, ps, sh);
}

// Cp[(a,i)][b] = scl * sum_c T[(a,i)][c] conj(Bp[b][c])
// (one text; bp_cprime is the function k_batch_pair calls, bp_cprime_blk k_batch_block's instance, as bp_select_blk)
__device__ __forceinline__ void bp_cprime_body(const zc* T, const zc* Bp, zc* Cp, int m, int n, int r, double scl, zc* tiles) {
  wg_gemm<true, true>(m, r, n, tiles,
      [&](int mm, int k) { return T[(long)mm * n + k]; },
      [&](int k, int nn) { const zc z = Bp[(long)nn * n + k]; return make_double2(z.x, -z.y); },
      [&](int mm, int nn, zc z) { Cp[(long)mm * r + nn] = make_double2(z.x * scl, z.y * scl); });
}
__device__ __noinline__ void bp_cprime(const zc* T, const zc* Bp, zc* Cp, int m, int n, int r, double scl, zc* tiles) {
  bp_cprime_body(T, Bp, Cp, m, n, r, scl, tiles);
}
__device__ __noinline__ void bp_cprime_blk(const zc* T, const zc* Bp, zc* Cp, int m, int n, int r, double scl, zc* tiles) {
  bp_cprime_body(T, Bp, Cp, m, n, r, scl, tiles);
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 196 VGPRs -- those of the
// non-inlined bt_env shared with k_batch_sweep -- 106 SGPRs, no vector register spills, 15 scalar registers spilled around
// the calls of the stage functions, 224 bytes of private memory per lane (the argument blocks of those calls, none of it
// inside a product, QR or Jacobi loop), 26 088 bytes of LDS; occupancy 2 waves per SIMD, i.e. one workgroup (replica) per
// compute unit.  DESIGN.md section 7.3.
__global__ __launch_bounds__(SS_THREADS) void k_batch_pair(BatchPairArgs gp) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ zc s_z[3 * BATCH_MAX_BOND];
  __shared__ double s_d[SS_WAVES * 8 + 8 + BATCH_MAX_BOND + BATCH_MAX_JUMP + 1 + 2 * BATCH_PAIR_MAX_DIM + 2 * BATCH_PAIR_MAX_DIM + 3];
  __shared__ int s_i[BATCH_PAIR_MAX_DIM + BATCH_MAX_BOND + 2];
  BtSh sh{};
  sh.mats = s_tiles;
  sh.udiag = s_z; sh.rdiag = s_z + BATCH_MAX_BOND;
  sh.wsh = s_d; sh.red = sh.wsh + SS_WAVES * 8; sh.gam = sh.red + 8;
  double* wk = sh.gam + BATCH_MAX_BOND;  // [BATCH_MAX_JUMP + 1]
  BpSh ps;
  ps.rot = wk + BATCH_MAX_JUMP + 1; ps.nrm = ps.rot + 2 * BATCH_PAIR_MAX_DIM; ps.res = ps.nrm + BATCH_PAIR_MAX_DIM;
  ps.scal = ps.res + BATCH_PAIR_MAX_DIM;  // [3]
  ps.h = s_z + 2 * BATCH_MAX_BOND;
  ps.rank = s_i; ps.sel = s_i + BATCH_PAIR_MAX_DIM; ps.flag = ps.sel + BATCH_MAX_BOND;
  zc* tiles = s_tiles;

  const BatchChanArgs& g = gp.c;
  const int r = blockIdx.x, tid = threadIdx.x, L = g.L;
  if (g.status[r] != SS_OK) return;  // a replica that failed in an earlier launch of the call does no more work
  void* const* tab = g.ptrs + (size_t)r * g.ptr_stride;
  zc* const* site = reinterpret_cast<zc* const*>(tab);
  zc* const* envL = reinterpret_cast<zc* const*>(tab + L);
  const zc* const* w2el = reinterpret_cast<const zc* const*>(tab + 4 * L + 2);
  zc* scr = reinterpret_cast<zc*>(tab[6 * L + 2]);
  zc* sig = scr + g.plan.o_sig;
  zc* spare = scr + g.plan.o_spare;
  zc* work = scr + g.plan.o_work;
  zc* X = scr + g.plan.o_x;
  zc* Y = scr + g.plan.o_y;
  zc* T0 = scr + g.plan.o_u;  // the work copy of theta; theta itself follows it
  const int lo = g.lo;

  int rc = SS_OK;
  for (int p = L - 1; p >= lo; --p) {
    const BatchShape s = g.shp[p];
    const int dl = s.dl, d = s.d, dr = s.dr;
    const BatchChanSite ch = g.chan[p];
    const zc* ops = g.ops + ch.off;
    // the one-site channel of p, as k_batch_channel applies it
    if (ch.kind == BCH_GATE) {
      bc_apply(ops, 1.0, site[p], spare, dl, d, dr);
    } else if (ch.kind == BCH_JUMP) {
      bc_weights(ops, ch.nops, site[p], dl, d, dr, wk, sh);
      const int pick = bc_pick(wk, ch.nops, bc_uniform(g.seed, g.ids[r], (unsigned long long)g.step, (unsigned long long)p));
      if (pick < 0) { rc = SS_EZERO; break; }
      const double scl = sqrt(wk[BATCH_MAX_JUMP] / wk[pick]);
      bc_apply(ops + (long)pick * d * d, scl, site[p], spare, dl, d, dr);  // its barriers order the reads of wk above
      if (tid == 0) g.counts[((size_t)r * L + p) * BATCH_MAX_JUMP + pick] += 1;
    }
    if (p == lo) break;
    const BatchShape q = g.shp[p - 1];
    const BatchChanSite pc = gp.pair[p - 1];
    if (pc.kind == BCH_NONE) {
      // Psi2sigmaB and Psi(p - 1) = A(p - 1) . sigma, as the backward sweep
      const int mq = d * dr;
      bt_qr(site[p], site[p], 1, mq, sig, 1, dl, mq, dl, work, sh);
      bt_matmul(site[p - 1], sig, spare, site[p - 1], q.dl * q.d, dl, dl, tiles);
      continue;
    }
    // the pair channel of bond (p - 1, p): merge, apply, split
    const int m = q.dl * q.d, n = d * dr, dd = q.d * d;
    zc* T1 = T0 + (long)m * n;
    const zc* pops = g.ops + pc.off;
    bp_merge(site[p - 1], site[p], T0, m, n, dl, tiles);
    int pick = 0;
    double before = 0.0;
    if (pc.kind == BCH_JUMP) {
      bp_weights(pops, pc.nops, T0, q.dl, q.d, d, dr, wk, sh);
      pick = bc_pick(wk, pc.nops, bc_uniform(g.seed, g.ids[r], (unsigned long long)g.step, (unsigned long long)(L + p - 1)));
      if (pick < 0) { rc = SS_EZERO; break; }
      before = wk[BATCH_MAX_JUMP];
    }
    bp_apply(pops + (long)pick * dd * dd, T0, T1, q.dl, q.d, d, dr);  // its barriers order the reads of wk above
    rc = bp_jacobi(T0, m, n, ps, sh);
    if (rc != SS_OK) break;
    bp_select(T0, site[p], m, n, dl, ps, sh);
    const double scl = pc.kind == BCH_JUMP ? sqrt(before / ps.scal[0]) : 1.0;
    bp_cprime(T1, site[p], site[p - 1], m, n, dl, scl, tiles);  // its barriers order the reads of ps.scal
    if (tid == 0) {
      gp.disc[r] += ps.scal[1];
      if (pc.kind == BCH_JUMP) gp.pcounts[((size_t)r * L + p - 1) * BATCH_MAX_JUMP + pick] += 1;
    }
  }
  if (rc == SS_OK)
    for (int p = lo; p < L - 1; ++p) {
      const BatchShape s = g.shp[p];
      const int dl = s.dl, d = s.d, dr = s.dr;
      // Psi2Asigma, L[p + 1], Psi(p + 1) = sigma . B(p + 1), as the forward sweep
      bt_qr(site[p], site[p], dr, 1, sig, dr, 1, dl * d, dr, work, sh);
      bt_env(envL[p], site[p], site[p], (long)d * dr, dr, 1, w2el[p], dl, s.ml, d, dr, s.mr, X, Y, envL[p + 1], tiles);
      const BatchShape q = g.shp[p + 1];
      zc* nxt = site[p + 1];
      bt_matmul(sig, nxt, spare, nxt, dr, q.d * q.dr, dr, tiles);
    }
  if (rc != SS_OK && tid == 0) g.status[r] = rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// Cross overlaps and one-site matrix elements between two states of a batch: k_batch_cross, ONE workgroup per PAIR (the
// pair index is blockIdx.x), every requested pair in one launch.  A state is a replica or the snapshot of one
// (BatchCrossPair in batch_site.h).  Two different states share no canonical form, so the walk runs over all L sites:
//   T (dl x dl, index order (bra bond, ket bond)) starts as 1
//   U[a'][(j,s)] = sum_a T[a'][a] K[a][(j,s)]                                  K: the ket tensor
//   at the pair's site the T' product reads  sum_j O[i][j] U[a'][(j,s)]  in the place of U[a'][(i,s)]  (the arithmetic
//     of bc_apply: j ascending, fused multiply-adds; formed in the operand fetch, so U needs no second buffer)
//   T'[s'][s] = sum_(a',j) conj(Bra[a'][j][s']) U[a'][j][s]
// and the value is the 1 x 1 T after site L-1.  The products are wg_gemm, as in the autocorrelation pass of
// k_batch_observe, which this walk equals when bra = conj(ket).
// What is resident where: LDS holds the two operand tiles of wg_gemm (16 896 bytes); T, its successor and U live in
// the batch's own buffer, indexed by PAIR -- several pairs may read one replica at the same time, so nothing of a walk
// may sit in a replica's scratch area -- written and re-read by this workgroup only and ordered by workgroup barriers.
// Replicas, snapshots and operators are only read.  Every element has one owner thread and every sum one order: a value
// depends on its two states and its operator only, not on the number of pairs, its place in the list, B or the compute
// unit.  No atomics, nothing waits for another workgroup, every loop is bounded by the shapes.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 86 VGPRs, 76 SGPRs, no vector
// or scalar register spills, NO private memory (0 bytes per lane: nothing is called out of line, so no access to it can
// sit inside a product loop), 16 896 bytes of LDS; occupancy 5 waves per SIMD, i.e. TWO workgroups (pairs) per compute
// unit where k_batch_observe (194 VGPRs through bt_heff) has one.  k_batch_snapshot, one workgroup of 256 threads per
// (replica, site): 10 VGPRs, no LDS, no private memory.
__global__ __launch_bounds__(256) void k_batch_snapshot(const BatchShape* __restrict__ shp, void* const* __restrict__ ptrs, int ptr_stride,
                                                        zc* __restrict__ snap, size_t snap_len) {
  const int r = blockIdx.x, p = blockIdx.y;
  size_t off = 0;
  for (int k = 0; k < p; ++k) off += (size_t)shp[k].dl * shp[k].d * shp[k].dr;
  const long N = (long)shp[p].dl * shp[p].d * shp[p].dr;
  const zc* src = reinterpret_cast<const zc*>(ptrs[(size_t)r * ptr_stride + p]);
  zc* dst = snap + (size_t)r * snap_len + off;
  for (long e = threadIdx.x; e < N; e += 256) dst[e] = src[e];
}

__global__ __launch_bounds__(SS_THREADS) void k_batch_cross(BatchCrossArgs g) {
  __shared__ __attribute__((aligned(16))) zc tiles[2 * BT_TK * BT_LD];
  const int q = blockIdx.x, tid = threadIdx.x, L = g.L, B = g.nrep;
  const BatchCrossPair pr = g.pairs[q];
  double* rec = g.rec + 2 * (size_t)q;
  if (BtState::dead(pr.bra, B, g.status) || BtState::dead(pr.ket, B, g.status)) {  // the same decision in every thread
    if (tid == 0) { rec[0] = 0.0; rec[1] = 0.0; }
    return;
  }
  const BtState bra(pr.bra, B, g.ptrs, g.ptr_stride, g.snap, g.snap_len), ket(pr.ket, B, g.ptrs, g.ptr_stride, g.snap, g.snap_len);
  const zc* O = g.ops + pr.off;
  zc* T = g.buf + (size_t)q * g.buf_len;
  zc* T2 = T + g.o_t2;
  zc* U = T + g.o_u;

  if (tid == 0) T[0] = make_double2(1.0, 0.0);
  __syncthreads();
  size_t soff = 0;
  for (int p = 0; p < L; ++p) {
    const BatchShape s = g.shp[p];
    const int dl = s.dl, d = s.d, dr = s.dr, ddr = d * dr;
    const zc* Kt = ket.at(p, soff);
    const zc* Bt = bra.at(p, soff);
    wg_walk_u(T, Kt, U, dl, ddr, tiles);
    // T'[i][j] = sum_(m,s) conj(Bra[(m,s)][i]) U[(m,s)][j], U with the operator on its physical index at the pair's site
    if (p == pr.site)
      wg_gemm<false, false>(dr, dr, dl * d, tiles,
          [&](int m, int kk) { const zc z = Bt[(long)kk * dr + m]; return make_double2(z.x, -z.y); },
          [&](int kk, int n) {
            const int a = kk / d, i = kk - a * d;
            const zc* col = U + (long)a * ddr + n;
            const zc* row = O + (long)i * d;
            double re = 0.0, im = 0.0;
            for (int j = 0; j < d; ++j) {
              const zc b = row[j], c = col[(long)j * dr];
              re = fma(b.x, c.x, re); re = fma(-b.y, c.y, re);
              im = fma(b.x, c.y, im); im = fma(b.y, c.x, im);
            }
            return make_double2(re, im);
          },
          [&](int m, int n, zc z) { T2[(long)m * dr + n] = z; });
    else
      wg_walk_t<true>(Bt, U, T2, dr, dl * d, tiles);
    zc* t = T; T = T2; T2 = t;
    soff += (size_t)dl * ddr;
  }
  if (tid == 0) { const zc z = T[0]; rec[0] = z.x; rec[1] = z.y; }
}

// ---------------------------------------------------------------------------------------------------------------------
// Bond spectra and entanglement entropies: k_batch_spectra, ONE workgroup per replica as above, every requested bond of
// every replica in one launch (BatchSpecArgs in batch_site.h has the record's layout).  The state is k_batch_observe's:
// centre at site 0, sites 1 .. L-1 right-canonical, so the Schmidt values of bond q are the singular values of the
// centre tensor once the centre stands at site q.  The walk moves the centre on WORK BUFFERS only:
//   X = C_0 (read in place)
//   q = 0 .. the highest requested bond:
//     X seen as (dl d) x dr  ->  R (dr x dr) by bt_qr, the sweep's Householder QR (its Q goes to X, which is free by then)
//     bp_jacobi on the rows of R: afterwards they are mutually orthogonal, |row i|^2 are the sigma^2 of bond q
//     a requested bond: its record from the row norms (bs_record)
//     q below the last: X = R' B_{q+1} with the rotated R' (bp_merge); R' is R up to a unitary on the left index, which
//       no later spectrum sees.  No U and no V is formed; sites right of the last requested bond are not touched.
// The record of a bond (bs_record): the squared row norms ranked by counting as bp_select does (ties: the lower index
// first) and stored in descending order; W, S1, S2 and pmin formed by ONE thread in that order.
// A Jacobi that does not converge zeroes the replica's record and sets the request's own word fail[replica]; the
// replica's status word is not touched -- an observation never changes a replica.
// What is resident where: LDS holds the two operand tiles of wg_gemm, the Householder scalars, the rotation scalars of a
// Jacobi round, the row norms, their ranks, the sorted weights and the reduction partials (22 376 bytes); X, the QR work
// matrix and R live in the request's own buffer [B][buf_len] (global memory, L2-resident), written and re-read by this
// workgroup only between workgroup barriers.  The replicas are only read.  Every element has one owner thread and every
// sum one order: a record depends neither on B nor on the replica's place in the batch nor on the compute unit.  No
// atomics, nothing waits for another workgroup, every loop is bounded by the shapes and BATCH_PAIR_MAX_SWEEPS.
__device__ __noinline__ void bs_record(int chi, const BpSh& ps, double* srt, double* out) {
  const int tid = threadIdx.x;
  if (tid < chi) srt[tid] = 0.0;  // every slot is defined whatever the norms are (NaN compares false everywhere)
  __syncthreads();
  if (tid < chi) {
    const double mine = ps.nrm[tid];
    int rk = 0;
    for (int j = 0; j < chi; ++j) {
      const double v = ps.nrm[j];
      rk += (v > mine || (v == mine && j < tid)) ? 1 : 0;
    }
    ps.rank[tid] = rk;
    srt[rk] = mine;
  }
  __syncthreads();
  if (tid < chi) out[BSPEC_HEAD + tid] = srt[tid];
  if (tid == 0) {
    double W = 0.0;
    for (int k = 0; k < chi; ++k) W += srt[k];
    double s1 = 0.0, s2 = 0.0, pmin = 0.0;
    if (W > 0.0) {
      double p2 = 0.0;
      for (int k = 0; k < chi; ++k) {
        const double p = srt[k] / W;
        if (p > 0.0) s1 -= p * log(p);
        p2 += p * p;
      }
      s2 = -log(p2);
      pmin = srt[chi - 1] / W;
    }
    out[0] = W; out[1] = s1; out[2] = s2; out[3] = pmin;
  }
  __syncthreads();
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 136 VGPRs -- those of the
// non-inlined stage functions it shares with k_batch_pair (bt_qr, bp_jacobi, bp_merge) -- 106 SGPRs, no vector or scalar
// register spills, 224 bytes of private memory per lane (the argument blocks of the calls of the stage functions, none of
// it inside a QR, Jacobi or product loop), 22 376 bytes of LDS; occupancy 3 waves per SIMD, i.e. one workgroup per
// compute unit.  DESIGN.md section 7.3.
__global__ __launch_bounds__(SS_THREADS) void k_batch_spectra(BatchSpecArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ zc s_z[2 * BATCH_MAX_BOND];
  __shared__ double s_d[SS_WAVES * 8 + 8 + BATCH_MAX_BOND + 2 * BATCH_MAX_BOND + BATCH_MAX_BOND + BATCH_MAX_BOND + 3];
  __shared__ int s_i[BATCH_MAX_BOND + 2];
  BtSh sh{};
  sh.mats = s_tiles;
  sh.udiag = s_z; sh.rdiag = s_z + BATCH_MAX_BOND;
  sh.wsh = s_d; sh.red = sh.wsh + SS_WAVES * 8; sh.gam = sh.red + 8;
  BpSh ps{};  // what bp_jacobi uses of it, sized for BATCH_MAX_BOND rows: the rotations of a round, the row norms, the scale
  ps.rot = sh.gam + BATCH_MAX_BOND; ps.nrm = ps.rot + 2 * BATCH_MAX_BOND;
  double* srt = ps.nrm + BATCH_MAX_BOND;  // [BATCH_MAX_BOND] the weights of a bond in descending order
  ps.scal = srt + BATCH_MAX_BOND;         // [3]
  ps.rank = s_i; ps.flag = s_i + BATCH_MAX_BOND;
  zc* tiles = s_tiles;

  const int r = blockIdx.x, tid = threadIdx.x;
  double* rec = g.rec + (size_t)r * g.rec_len;
  for (long e = tid; e < g.rec_len; e += SS_THREADS) rec[e] = 0.0;
  __syncthreads();
  if (g.status[r] != SS_OK) return;  // a replica that failed: zeros
  const zc* const* site = reinterpret_cast<const zc* const*>(g.ptrs + (size_t)r * g.ptr_stride);
  zc* X = g.buf + (size_t)r * g.buf_len;
  zc* work = X + g.o_work;
  zc* R = X + g.o_r;

  const int last = g.bonds[g.nbonds - 1];
  int k = 0, rc = SS_OK, q = 0;
  long off = 0;
  for (; q <= last; ++q) {
    const BatchShape s = g.shp[q];
    const int m = s.dl * s.d, n = s.dr;
    bt_qr(q == 0 ? site[0] : X, X, n, 1, R, n, 1, m, n, work, sh);
    rc = bp_jacobi(R, n, n, ps, sh);
    if (rc != SS_OK) break;  // the same decision in every thread of the workgroup
    if (g.bonds[k] == q) {
      bs_record(n, ps, srt, rec + off);
      off += BSPEC_HEAD + n;
      ++k;
    }
    if (q < last) {
      const BatchShape t = g.shp[q + 1];
      bp_merge(R, site[q + 1], X, n, t.d * t.dr, n, tiles);
    }
  }
  if (rc != SS_OK) {
    __syncthreads();
    for (long e = tid; e < g.rec_len; e += SS_THREADS) rec[e] = 0.0;
    if (tid == 0) g.fail[r] = q + 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Sampled configurations: k_batch_sample, ONE workgroup per replica, nshots configurations of every replica in one launch
// (BatchSampleArgs in batch_site.h has the arithmetic).  The state is k_batch_observe's: centre at site 0, sites 1 .. L-1
// right-canonical, so the weight of outcome j at site p given the outcomes left of it is |v C_p[:, j, :]|^2 with v the
// normalised left boundary vector of the shot: one walk from left to right, no environment.  Shots go through the walk
// BATCH_SAMPLE_CHUNK at a time; per site of a chunk:
//   product    W (chunk x d dr) = V (chunk x dl) C_p (dl x d dr): ONE wg_gemm
//   weights    g[t][j] = sum_s |W[t][j dr + s]|^2: (shot, outcome) q of a round of 64 belongs to lanes 8 (q % 64) ..
//              8 (q % 64) + 7; lane l of them adds s = l, l + 8, .. in that order, then a three-level xor tree over the 8
//   selection  thread t owns shot t of the chunk: G in index order, bc_pick on the shot's uniform, the int32 outcome and
//              the running probability
//   normalise  V[t][s] = W[t][j_t dr + s] / sqrt(g[t][j_t]), element e by thread e % 512
// A row of the product takes its K terms in the order of wg_gemm whatever the other rows are, so a shot's bits depend on
// (replica state, seed, id, step, shot) only: not on the chunk, nshots, B or the compute unit.  The frequencies are counted
// at the end over the replica's finished configurations, (site, outcome) f by thread f % 512.
// What is resident where: LDS holds the two operand tiles of wg_gemm, a chunk's weights while d <= BATCH_SAMPLE_LDS_D
// (otherwise they go to the request's buffer), and per shot of the chunk the running probability, the outcome and
// sqrt(g); V and W live in the request's own buffer [B][buf_len] (global memory, L2-resident), written and re-read by
// this workgroup only between workgroup barriers.  The replicas are only read.  No atomics, nothing waits for another
// workgroup, every loop is bounded by the shapes and nshots.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 110 VGPRs, 82 SGPRs, no vector
// or scalar register spills, no private memory (wg_gemm is inlined: there is no call and no argument block), 26 368 bytes
// of LDS; occupancy 4 waves per SIMD, i.e. two workgroups per compute unit.  DESIGN.md section 7.3.
__device__ __forceinline__ double bsm_uniform(unsigned long long base, unsigned long long site, unsigned long long shot) {
  // base = mix(mix(seed ^ trajectory) + step): key = mix(mix(base + site) + shot)
  const unsigned long long key = bc_mix(bc_mix(base + site) + shot);
  return (double)(key >> 11) * 0x1.0p-53;
}

__global__ __launch_bounds__(SS_THREADS) void k_batch_sample(BatchSampleArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ double s_g[BATCH_SAMPLE_CHUNK * BATCH_SAMPLE_LDS_D];
  __shared__ double s_prob[BATCH_SAMPLE_CHUNK], s_nrm[BATCH_SAMPLE_CHUNK];
  __shared__ int s_pick[BATCH_SAMPLE_CHUNK];
  zc* tiles = s_tiles;

  const int r = blockIdx.x, tid = threadIdx.x, L = g.L, nshots = g.nshots;
  int* cfg = g.configs + (size_t)r * nshots * L;
  double* prob = g.prob + (size_t)r * nshots;
  double* freq = g.freq + (size_t)r * g.F;
  if (g.status[r] != SS_OK) {  // a replica that failed: -1 everywhere and zeros
    for (long e = tid; e < (long)nshots * L; e += SS_THREADS) cfg[e] = -1;
    for (long e = tid; e < nshots; e += SS_THREADS) prob[e] = 0.0;
    for (long e = tid; e < g.F; e += SS_THREADS) freq[e] = 0.0;
    return;
  }
  const zc* const* site = reinterpret_cast<const zc* const*>(g.ptrs + (size_t)r * g.ptr_stride);
  zc* V = g.buf + (size_t)r * g.buf_len;
  zc* W = V + g.o_w;
  double* gbuf = reinterpret_cast<double*>(V + g.o_g);
  const unsigned long long base = bc_mix(bc_mix(g.seed ^ g.ids[r]) + (unsigned long long)g.step);
  const int sub = tid & 7, grp = tid >> 3;

  for (int c0 = 0; c0 < nshots; c0 += BATCH_SAMPLE_CHUNK) {
    const int nc = min(BATCH_SAMPLE_CHUNK, nshots - c0);
    if (tid < nc) {
      V[tid] = make_double2(1.0, 0.0);
      s_prob[tid] = 1.0;
      s_pick[tid] = 0;
    }
    __syncthreads();
    for (int p = 0; p < L; ++p) {
      const BatchShape s = g.shp[p];
      const int dl = s.dl, d = s.d, dr = s.dr, ddr = d * dr;
      const zc* C = site[p];
      wg_gemm<true, false>(nc, ddr, dl, tiles,
                           [&](int m, int k) { return V[m * dl + k]; },
                           [&](int k, int n) { return C[(long)k * ddr + n]; },
                           [&](int m, int n, zc z) { W[m * ddr + n] = z; });
      double* gw = d <= BATCH_SAMPLE_LDS_D ? s_g : gbuf;
      const int total = nc * d;
      for (int q0 = 0; q0 < total; q0 += SS_THREADS / 8) {
        const int q = q0 + grp;
        double acc = 0.0;
        if (q < total) {
          const int t = q / d, j = q - t * d;
          const zc* row = W + t * ddr + j * dr;
          for (int k = sub; k < dr; k += 8) {
            const zc z = row[k];
            acc = fma(z.x, z.x, acc); acc = fma(z.y, z.y, acc);
          }
        }
        acc += __shfl_xor(acc, 4, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 1, 64);
        if (q < total && sub == 0) gw[q] = acc;
      }
      __syncthreads();
      if (tid < nc) {
        int pick = -1;
        double nrm = 1.0;
        if (s_pick[tid] >= 0) {  // a shot that met G == 0 stays at -1
          const double* w = gw + tid * d;
          pick = bc_pick(w, d, bsm_uniform(base, (unsigned long long)p, (unsigned long long)(c0 + tid)));
          if (pick >= 0) {
            double G = 0.0;
            for (int j = 0; j < d; ++j) G += w[j];
            s_prob[tid] *= w[pick] / G;
            nrm = sqrt(w[pick]);
          } else {
            s_prob[tid] = 0.0;
          }
        }
        s_pick[tid] = pick;
        s_nrm[tid] = nrm;
        cfg[(size_t)(c0 + tid) * L + p] = pick;
      }
      __syncthreads();
      for (int e = tid; e < nc * dr; e += SS_THREADS) {
        const int t = e / dr, k = e - t * dr, pk = s_pick[t];
        zc z = make_double2(0.0, 0.0);
        if (pk >= 0) {
          const zc w = W[t * ddr + pk * dr + k];
          const double nr = s_nrm[t];
          z = make_double2(w.x / nr, w.y / nr);
        }
        V[e] = z;
      }
      __syncthreads();
    }
    if (tid < nc) prob[c0 + tid] = s_prob[tid];
    __syncthreads();
  }
  for (long f = tid; f < g.F; f += SS_THREADS) {
    int p = 0;
    long j = f;
    while (j >= g.shp[p].d) { j -= g.shp[p].d; ++p; }  // f < F = sum d_p: p stays below L
    long cnt = 0;
    for (int t = 0; t < nshots; ++t) cnt += cfg[(size_t)t * L + p] == (int)j ? 1 : 0;
    freq[f] = (double)cnt / (double)nshots;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Expectation values of MPO observables: k_batch_expect, ONE workgroup per (replica, operator) pair, workgroup index
// r * nops + k, every listed operator of every replica in one launch (BatchExpectArgs in batch_site.h).  The state is
// k_batch_observe's: centre at site 0, sites 1 .. L-1 right-canonical.  The walk is the arithmetic of Engine::expect for an
// operator whose right blocks nobody has cached:
//   E = the right boundary block (1 x 1 x 1, the engine's own)
//   p = L-1 .. 1:  E <- bt_env(E, site p in its mirror-image strides, w2er of operator k at p), the form k_batch_sweep
//                  uses on its way back, with operator k's ml / mr; written alternately into the pair's two blocks
//   H = bt_heff(left block 0, w2l of operator k at site 0, E, C_0)
//   value = <C_0 | H> + shift_k <C_0 | C_0>, not normalised: the three sums split over the 512 threads in one fixed order
//           and finished by wg_reduce, as the energy of k_batch_observe
// L = 1 skips the walk.  What is resident where: LDS holds the two operand tiles of wg_gemm and the reduction partials
// (17 472 bytes); the two blocks, X, Y and H C live in the pair's carve of the request's own buffer [B][nops][carve]
// (global memory, L2-resident), written and re-read by this workgroup only between workgroup barriers.  Replicas, operators
// and status words are only read.  Every element has one owner thread and every sum one order: a value depends on its
// replica and its operator only, not on B, nops, the operator's place in the list or the compute unit.  No atomics, nothing
// waits for another workgroup, every loop is bounded by the shapes.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 196 VGPRs -- those of the
// non-inlined product function bt_env it shares with k_batch_sweep -- 83 SGPRs, no vector or scalar register spills, 32
// bytes of private memory per lane (the shape block bt_heff takes by reference, none of it inside a product loop), 17 472
// bytes of LDS; occupancy 2 waves per SIMD, i.e. one workgroup per compute unit.  DESIGN.md section 7.3.
__global__ __launch_bounds__(SS_THREADS) void k_batch_expect(BatchExpectArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ double s_d[SS_WAVES * 8 + 8];
  BtSh sh{};
  sh.mats = s_tiles;
  sh.wsh = s_d;
  sh.red = s_d + SS_WAVES * 8;
  zc* tiles = s_tiles;

  const int wg = blockIdx.x, tid = threadIdx.x, L = g.L;
  const int r = wg / g.nops, k = wg - r * g.nops;
  double* rec = g.rec + (size_t)wg * 2;
  if (g.status[r] != SS_OK) {  // a replica that failed: zeros
    if (tid < 2) rec[tid] = 0.0;
    return;
  }
  void* const* tab = g.ptrs + (size_t)r * g.ptr_stride;
  const zc* const* site = reinterpret_cast<const zc* const*>(tab);
  const zc* envL0 = reinterpret_cast<const zc*>(tab[L]);
  const zc* cur = reinterpret_cast<const zc*>(tab[3 * L + 1]);  // right block L, the boundary
  const zc* const* w2l = reinterpret_cast<const zc* const*>(g.ops + (size_t)wg * 3 * L);
  const zc* const* w2er = w2l + 2 * L;
  const BatchShape* shp = g.shp + (size_t)k * L;
  zc* buf = g.buf + (size_t)wg * g.plan.total;
  zc* Ea = buf;
  zc* Eb = buf + g.plan.o_e1;
  zc* X = buf + g.plan.o_x;
  zc* Y = buf + g.plan.o_y;
  zc* H = buf + g.plan.o_h;

  for (int p = L - 1; p >= 1; --p) {
    const BatchShape s = shp[p];
    bt_env(cur, site[p], site[p], 1, s.dr, (long)s.d * s.dr, w2er[p], s.dr, s.mr, s.d, s.dl, s.ml, X, Y, Ea, tiles);
    cur = Ea;
    zc* t = Ea; Ea = Eb; Eb = t;
  }
  const BatchShape s0 = shp[0];
  const long N0 = (long)s0.dl * s0.d * s0.dr;
  const zc* C = site[0];
  bt_heff(s0, envL0, w2l[0], cur, C, 1.0, X, Y, H, tiles);
  double acc[3] = {0.0, 0.0, 0.0};
  for (long e = tid; e < N0; e += SS_THREADS) {
    const zc c = C[e], h = H[e];
    acc[0] += c.x * h.x + c.y * h.y;  // conj(c) h
    acc[1] += c.x * h.y - c.y * h.x;
    acc[2] += c.x * c.x + c.y * c.y;
  }
  wg_reduce(acc, sh);
  if (tid == 0) {
    const zc sft = g.shift[wg];
    const double n2 = sh.red[2];
    rec[0] = sh.red[0] + sft.x * n2;
    rec[1] = sh.red[1] + sft.y * n2;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// MPO matrix elements between two states of a batch: k_batch_cross_mpo, ONE workgroup per ENTRY (the entry index is
// blockIdx.x), every entry of the request in one launch (BatchCrossMpoArgs in batch_site.h).  An entry is (bra, ket,
// operator); the states are named as in k_batch_cross, the operator's cores and scalar term are those of the ket's owner,
// replica ket mod B.  Two different states share no canonical form, so the walk runs over all L sites, left to right:
//   T (bra bond, MPO bond, ket bond) = the 1 x 1 x 1 block [1]
//   p = 0 .. L-1:  T <- bt_env_fwd(T, Bra_p, Ket_p, w2el of the operator at p): the three products of bt_env in the roles
//                  of the forward sweep, strides (d dr, dr, 1); stage 1 reads conj of the BRA tensor, stage 3 the KET
//                  tensor; written alternately into the entry's two blocks
//   value = the 1 x 1 x 1 block after site L-1, <bra | O | ket>, not normalised
// With a non-zero scalar term the same workgroup then runs the plain-overlap walk (wg_overlap: the products of
// k_batch_cross with site = -1) and adds shift * <bra | ket>; the decision is the same in every thread.
// What is resident where: LDS holds the two operand tiles of wg_gemm (16 896 bytes); the two blocks, X and Y live in the
// ENTRY's carve of the request's own buffer [P][carve] -- several entries may read one replica at the same time, so
// nothing of a walk may sit in a replica's scratch area -- written and re-read by this workgroup only between workgroup
// barriers; the overlap walk reuses them (T and its successor in the blocks, U in X).  Replicas, snapshots, operators and
// status words are only read.  Every element has one owner thread and every sum one order: a value depends on its two
// states and its operator only, not on the number of entries, its place in the list, B or the compute unit.  No atomics,
// nothing waits for another workgroup, every loop is bounded by the shapes.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 180 VGPRs -- those of bt_env_fwd
// -- 82 SGPRs, no vector or scalar register spills, NO private memory (0 bytes per lane: bt_env_fwd takes its arguments in
// registers, so no access to private memory can sit inside a product loop), 16 896 bytes of LDS; occupancy 2 waves per
// SIMD, i.e. one workgroup (entry) per compute unit.
__global__ __launch_bounds__(SS_THREADS) void k_batch_cross_mpo(BatchCrossMpoArgs g) {
  __shared__ __attribute__((aligned(16))) zc tiles[2 * BT_TK * BT_LD];
  const int q = blockIdx.x, tid = threadIdx.x, L = g.L, B = g.nrep;
  const BatchCrossMpoEntry en = g.entries[q];
  double* rec = g.rec + 2 * (size_t)q;
  if (BtState::dead(en.bra, B, g.status) || BtState::dead(en.ket, B, g.status)) {  // the same decision in every thread
    if (tid == 0) { rec[0] = 0.0; rec[1] = 0.0; }
    return;
  }
  const int owner = en.ket < B ? en.ket : en.ket - B;
  const BtState bra(en.bra, B, g.ptrs, g.ptr_stride, g.snap, g.snap_len), ket(en.ket, B, g.ptrs, g.ptr_stride, g.snap, g.snap_len);
  const zc* const* w2el = reinterpret_cast<const zc* const*>(g.ops + ((size_t)owner * g.nops + en.op) * L);
  const BatchShape* shp = g.shp + (size_t)en.op * L;
  const zc sft = g.shift[(size_t)owner * g.nops + en.op];
  zc* buf = g.buf + (size_t)q * g.plan.total;
  zc* Ea = buf;
  zc* Eb = buf + g.plan.o_e1;
  zc* X = buf + g.plan.o_x;
  zc* Y = buf + g.plan.o_y;

  if (tid == 0) Ea[0] = make_double2(1.0, 0.0);
  __syncthreads();
  size_t soff = 0;
  for (int p = 0; p < L; ++p) {
    const BatchShape s = shp[p];
    bt_env_fwd(Ea, bra.at(p, soff), ket.at(p, soff), w2el[p], s.dl, s.ml, s.d, s.dr, s.mr, X, Y, Eb, tiles);
    zc* t = Ea; Ea = Eb; Eb = t;
    soff += (size_t)s.dl * s.d * s.dr;
  }
  const zc val = Ea[0];
  if (sft.x == 0.0 && sft.y == 0.0) {  // uniform: the scalar term is the entry's
    if (tid == 0) { rec[0] = val.x; rec[1] = val.y; }
    return;
  }
  __syncthreads();  // every thread has read the value before the blocks are used again
  // the plain overlap <bra | ket>, T and its successor in the two blocks, U in X
  const zc* T = wg_overlap(L, shp, [&](int p, size_t so) { return ket.at(p, so); }, [&](int p, size_t so) { return bra.at(p, so); },
                           Ea, Eb, X, tiles);
  if (tid == 0) {
    const zc ov = T[0];
    rec[0] = val.x + (sft.x * ov.x - sft.y * ov.y);
    rec[1] = val.y + (sft.x * ov.y + sft.y * ov.x);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// An MPO applied to the replicas: k_batch_operate, ONE workgroup per SELECTED replica (workgroup j owns replica
// replicas[j]), the whole variational fit of Engine::operate / oracle.operate in one launch (BatchOperateArgs in
// batch_site.h): phi ~ O|psi> / |O|psi>| in the bond dimensions of psi.  The bra, phi, lives in the replica's own site
// tensors, which the kernel WRITES; the ket is a copy of them in the replica's carve of the request's buffer.
//   setup      ket <- the replica's tensors (centre at site 0); blocks 0 and L of the mixed and of the overlap chain <- [1];
//              p = L-1 .. 1: block p <- bt_env(block p+1, bra_p, ket_p, w2er at p) in the mirror-image strides of the
//              backward sweep (bra = ket here)
//   double sweep it = 1 .. maxstep:
//     prev <- bra
//     p = 0 .. L-1:   bra_p <- bt_heff(block p, w2l at p, block p+1, ket_p)  [+ shift * the same apply of the overlap
//                     blocks with the identity core]; nrm = |bra_p|; bra_p /= nrm; unless p = L-1: thin QR of bra_p (R
//                     dropped: the next site is replaced) and of ket_p (R absorbed into ket_{p+1}), block p+1 <-
//                     bt_env(block p, bra_p, ket_p, w2el at p)  [and the overlap block with the identity core]
//     p = L-1 .. 0:   the mirror image: QR of the transposes, R^T absorbed into ket_{p-1}, block p <- bt_env(block p+1, ..,
//                     w2er at p)
//     ov = <bra | prev> by the plain-overlap walk (wg_overlap); stop when |1 - |ov|| < conv_tol
//   norms[j] = nrm of the last apply at site 0, iters[j] = double sweeps run.  A norm that is not > 0 stops the replica:
//   SS_EZERO in its status word, norms[j] = 0; the decision is formed from a workgroup reduction, the same in every thread.
// One array of L + 1 blocks serves both directions: block b is the left block while the centre is at a site >= b and the
// right block otherwise, and a half-sweep overwrites it exactly when its other role is spent.  The scalar term goes
// through the overlap blocks as the engine does it: the identity core of MPO bond 1 (written into the carve for the
// site's d before each use) through the same bt_heff / bt_env.  L = 1: one apply per half-sweep, no QR.
// What is resident where: LDS holds the two operand tiles of wg_gemm, the Householder scalars of a gauge move and the
// reduction partials (20 032 bytes); everything of tensor size lives in the replica's carve of the REQUEST's own buffer
// (BatchOperatePlan: ket, prev, the blocks, X, Y, the QR work matrix, ...), written and re-read by this workgroup only
// between workgroup barriers.  Every element has one owner thread and every sum one order: a replica's result depends on
// its tensors, its operator, maxstep and conv_tol only -- not on the selection, B or the compute unit.  No atomics, nothing
// waits for another workgroup, every loop is bounded by the shapes and maxstep.  The stages are non-inlined functions that
// take what they need by value, so that no private-memory access sits inside a product loop.
struct BopCtx {
  int L;
  zc sft;
  const BatchShape* shp;
  zc* const* site;
  const zc* const* w2l;
  const zc* const* w2el;
  const zc* const* w2er;
  const long long *soff, *moff, *voff;
  zc *ket, *mix, *ov, *X, *Y, *work, *spare, *H, *sig, *Id, *tiles;
};

// the d x d identity: the core (1, d, d, 1) of the scalar term's operator in all three of its forms
__device__ __noinline__ void bop_ident(zc* Id, int d) {
  for (int e = threadIdx.x; e < d * d; e += SS_THREADS) Id[e] = make_double2(e / d == e % d ? 1.0 : 0.0, 0.0);
  __syncthreads();
}

// bra_p <- (mixed blocks) W ket_p [+ shift (overlap blocks) ket_p], normalised; returns the norm, the same bits in every
// thread; a norm that is not > 0 leaves bra_p unscaled
__device__ __noinline__ double bop_apply(const BopCtx& c, int p, const BtSh& sh) {
  const BatchShape s = c.shp[p];
  const long N = (long)s.dl * s.d * s.dr;
  const zc* kt = c.ket + c.soff[p];
  zc* out = c.site[p];
  zc* X = c.X;
  zc* Y = c.Y;
  zc* tiles = c.tiles;
  bt_heff(s, c.mix + c.moff[p], c.w2l[p], c.mix + c.moff[p + 1], kt, 1.0, X, Y, out, tiles);
  const zc sft = c.sft;
  const bool hs = sft.x != 0.0 || sft.y != 0.0;
  zc* H = c.H;
  if (hs) {
    const BatchShape si{s.dl, s.d, s.dr, 1, 1};
    zc* Id = c.Id;
    bop_ident(Id, s.d);
    bt_heff(si, c.ov + c.voff[p], Id, c.ov + c.voff[p + 1], kt, 1.0, X, Y, H, tiles);
  }
  double acc[1] = {0.0};
  for (long e = threadIdx.x; e < N; e += SS_THREADS) {
    zc z = out[e];
    if (hs) {
      const zc h = H[e];
      z.x += sft.x * h.x - sft.y * h.y;
      z.y += sft.x * h.y + sft.y * h.x;
      out[e] = z;
    }
    acc[0] += z.x * z.x + z.y * z.y;
  }
  wg_reduce(acc, sh);
  const double nrm = sqrt(sh.red[0]);
  if (nrm > 0.0)
    for (long e = threadIdx.x; e < N; e += SS_THREADS) {  // the same thread read or wrote out[e] above
      zc z = out[e];
      z.x /= nrm; z.y /= nrm;
      out[e] = z;
    }
  __syncthreads();
  return nrm;
}

// the centre of bra and ket moves from site p to p + 1 (fwd) or p - 1, and the block between them is renewed
__device__ __noinline__ void bop_move(const BopCtx& c, int p, bool fwd, const BtSh& sh) {
  const BatchShape s = c.shp[p];
  const int dl = s.dl, d = s.d, dr = s.dr;
  const bool hs = c.sft.x != 0.0 || c.sft.y != 0.0;
  zc* bra = c.site[p];
  zc* kt = c.ket + c.soff[p];
  zc *X = c.X, *Y = c.Y, *sig = c.sig, *work = c.work, *spare = c.spare, *tiles = c.tiles, *Id = c.Id;
  if (fwd) {
    bt_qr(bra, bra, dr, 1, sig, dr, 1, dl * d, dr, work, sh);  // phi: Psi -> A, its R goes into a tensor that is replaced next
    bt_qr(kt, kt, dr, 1, sig, dr, 1, dl * d, dr, work, sh);    // psi: Psi -> A sigma
    const BatchShape q = c.shp[p + 1];
    zc* nxt = c.ket + c.soff[p + 1];
    bt_matmul(sig, nxt, spare, nxt, dr, q.d * q.dr, dr, tiles);
    bt_env(c.mix + c.moff[p], bra, kt, (long)d * dr, dr, 1, c.w2el[p], dl, s.ml, d, dr, s.mr, X, Y, c.mix + c.moff[p + 1], tiles);
    if (hs) {
      bop_ident(Id, d);
      bt_env(c.ov + c.voff[p], bra, kt, (long)d * dr, dr, 1, Id, dl, 1, d, dr, 1, X, Y, c.ov + c.voff[p + 1], tiles);
    }
  } else {
    const int mq = d * dr;
    bt_qr(bra, bra, 1, mq, sig, 1, dl, mq, dl, work, sh);  // Psi^T = Q R: B = Q^T in place
    bt_qr(kt, kt, 1, mq, sig, 1, dl, mq, dl, work, sh);    // sigma = R^T (dl x dl)
    const BatchShape q = c.shp[p - 1];
    zc* prv = c.ket + c.soff[p - 1];
    bt_matmul(prv, sig, spare, prv, q.dl * q.d, dl, dl, tiles);
    bt_env(c.mix + c.moff[p + 1], bra, kt, 1, dr, (long)d * dr, c.w2er[p], dr, s.mr, d, dl, s.ml, X, Y, c.mix + c.moff[p], tiles);
    if (hs) {
      bop_ident(Id, d);
      bt_env(c.ov + c.voff[p + 1], bra, kt, 1, dr, (long)d * dr, Id, dr, 1, d, dl, 1, X, Y, c.ov + c.voff[p], tiles);
    }
  }
}

// <bra | prev> over all sites (wg_overlap), T and its successor in the two transfer blocks; the same bits in every thread
__device__ __noinline__ zc bop_overlap(int L, const BatchShape* shp, zc* const* site, const zc* prev, const long long* soff, zc* T,
                                       zc* T2, zc* U, zc* tiles) {
  const zc ov = wg_overlap(L, shp, [&](int p, size_t) { return prev + soff[p]; }, [&](int p, size_t) { return site[p]; },
                           T, T2, U, tiles)[0];
  __syncthreads();  // every thread has read the value before the blocks are used again
  return ov;
}

// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 512 threads = 8 waves): 246 VGPRs, 106 SGPRs, no vector
// register spills, 22 scalar registers spilled around the calls of the stage functions, 384 bytes of private memory per lane
// (BopCtx, which the stage functions take by reference and read BEFORE their products, and the shape blocks bt_heff takes
// by reference: none of it inside a product loop), 20 032 bytes of LDS; occupancy 2 waves per SIMD, i.e. one workgroup
// (replica) per compute unit.  DESIGN.md section 7.3.
__global__ __launch_bounds__(SS_THREADS) void k_batch_operate(BatchOperateArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ zc s_z[2 * BATCH_MAX_BOND];
  __shared__ double s_d[SS_WAVES * 8 + 8 + BATCH_MAX_BOND];
  BtSh sh{};
  sh.mats = s_tiles;
  sh.wsh = s_d;
  sh.red = s_d + SS_WAVES * 8;
  sh.gam = sh.red + 8;
  sh.udiag = s_z;
  sh.rdiag = s_z + BATCH_MAX_BOND;

  const int j = blockIdx.x, tid = threadIdx.x, L = g.L;
  const int r = g.replicas[j];
  zc* buf = g.buf + (size_t)j * g.carve.total;
  BopCtx c;
  c.L = L;
  c.sft = g.shift[j];
  c.shp = g.shp;
  c.site = reinterpret_cast<zc* const*>(g.ptrs + (size_t)r * g.ptr_stride);
  c.w2l = reinterpret_cast<const zc* const*>(g.ops + (size_t)j * 3 * L);
  c.w2el = c.w2l + L;
  c.w2er = c.w2l + 2 * L;
  c.soff = g.offs;
  c.moff = g.offs + (L + 1);
  c.voff = g.offs + 2 * (L + 1);
  c.ket = buf + g.carve.o_ket;
  c.mix = buf + g.carve.o_mix;
  c.ov = buf + g.carve.o_ov;
  c.X = buf + g.carve.o_x;
  c.Y = buf + g.carve.o_y;
  c.work = buf + g.carve.o_work;
  c.spare = buf + g.carve.o_spare;
  c.H = buf + g.carve.o_h;
  c.sig = buf + g.carve.o_sig;
  c.Id = buf + g.carve.o_id;
  c.tiles = s_tiles;
  zc* prev = buf + g.carve.o_prev;
  zc* T0 = buf + g.carve.o_t0;
  zc* T1 = buf + g.carve.o_t1;
  const bool hs = c.sft.x != 0.0 || c.sft.y != 0.0;  // uniform: the scalar term is the replica's

  // setup: the ket, the boundary blocks, the right blocks of the initial bra = ket pair
  for (int p = 0; p < L; ++p) {
    const long N = c.soff[p + 1] - c.soff[p];
    const zc* src = c.site[p];
    zc* dst = c.ket + c.soff[p];
    for (long e = tid; e < N; e += SS_THREADS) dst[e] = src[e];
  }
  if (tid == 0) {
    const zc one = make_double2(1.0, 0.0);
    c.mix[c.moff[0]] = one; c.mix[c.moff[L]] = one;
    c.ov[c.voff[0]] = one; c.ov[c.voff[L]] = one;
  }
  __syncthreads();
  for (int p = L - 1; p >= 1; --p) {
    const BatchShape s = c.shp[p];
    const zc* kt = c.ket + c.soff[p];
    bt_env(c.mix + c.moff[p + 1], c.site[p], kt, 1, s.dr, (long)s.d * s.dr, c.w2er[p], s.dr, s.mr, s.d, s.dl, s.ml, c.X, c.Y,
           c.mix + c.moff[p], c.tiles);
    if (hs) {
      bop_ident(c.Id, s.d);
      bt_env(c.ov + c.voff[p + 1], c.site[p], kt, 1, s.dr, (long)s.d * s.dr, c.Id, s.dr, 1, s.d, s.dl, 1, c.X, c.Y, c.ov + c.voff[p],
             c.tiles);
    }
  }

  double nrm = 0.0;
  bool dead = false;
  int it = 1;
  for (; it <= g.maxstep; ++it) {
    for (int p = 0; p < L; ++p) {
      const long N = c.soff[p + 1] - c.soff[p];
      const zc* src = c.site[p];
      zc* dst = prev + c.soff[p];
      for (long e = tid; e < N; e += SS_THREADS) dst[e] = src[e];
    }
    __syncthreads();
    for (int p = 0; p < L && !dead; ++p) {  // ->
      nrm = bop_apply(c, p, sh);
      dead = !(nrm > 0.0);
      if (!dead && p < L - 1) bop_move(c, p, true, sh);
    }
    for (int p = L - 1; p >= 0 && !dead; --p) {  // <-
      nrm = bop_apply(c, p, sh);
      dead = !(nrm > 0.0);
      if (!dead && p > 0) bop_move(c, p, false, sh);
    }
    if (dead) break;
    const zc ov = bop_overlap(L, c.shp, c.site, prev, c.soff, T0, T1, c.X, c.tiles);
    // _is_converged: |1 - |<phi_i | phi_{i-1}>|| < conv_tol
    if (fabs(1.0 - sqrt(ov.x * ov.x + ov.y * ov.y)) < g.conv_tol || it == g.maxstep) break;
  }
  if (tid == 0) {
    if (dead) g.status[r] = SS_EZERO;
    g.norms[j] = dead ? 0.0 : nrm;
    g.iters[j] = it;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Test hook: k_batch_block, ONE building block of the kernels above in one workgroup (mitdvp_batch_block; the shapes,
// operands and footprints are batch_block_check.h's, and the host has checked them).  Workgroup b copies the operands to
// its own part of g.work and runs the block there -- the function the kernels call, not a restatement of it -- with the
// LDS of k_batch_pair: the tile array handed over directly (assume_lds above says why), BtSh and BpSh carved the same
// way.  Everything a workgroup reads after the copy it wrote itself; nothing is shared between workgroups.
__global__ __launch_bounds__(SS_THREADS) void k_batch_block(BatchBlockArgs g) {
  __shared__ __attribute__((aligned(16))) zc s_tiles[2 * BT_TK * BT_LD];
  __shared__ zc s_z[3 * BATCH_MAX_BOND];
  __shared__ double s_d[SS_WAVES * 8 + 8 + BATCH_MAX_BOND + 2 * BATCH_PAIR_MAX_DIM + 2 * BATCH_PAIR_MAX_DIM + 3];
  __shared__ int s_i[BATCH_PAIR_MAX_DIM + BATCH_MAX_BOND + 2];
  __shared__ BatchShape s_shp[BATCH_BLOCK_MAX_CHAIN];
  BtSh sh{};
  sh.mats = s_tiles;
  sh.udiag = s_z; sh.rdiag = s_z + BATCH_MAX_BOND;
  sh.wsh = s_d; sh.red = sh.wsh + SS_WAVES * 8; sh.gam = sh.red + 8;
  BpSh ps;
  ps.rot = sh.gam + BATCH_MAX_BOND; ps.nrm = ps.rot + 2 * BATCH_PAIR_MAX_DIM; ps.res = ps.nrm + BATCH_PAIR_MAX_DIM;
  ps.scal = ps.res + BATCH_PAIR_MAX_DIM;  // [3]
  ps.h = s_z + 2 * BATCH_MAX_BOND;
  ps.rank = s_i; ps.sel = s_i + BATCH_PAIR_MAX_DIM; ps.flag = ps.sel + BATCH_MAX_BOND;

  const int b = blockIdx.x, tid = threadIdx.x;
  const BatchBlockFoot& f = g.foot;
  zc* c[4];  // this workgroup's copies of the operands
  zc* w[3];  // and its work areas
  {
    zc* p = g.work + (size_t)b * (f.in[0] + f.in[1] + f.in[2] + f.in[3] + f.work[0] + f.work[1] + f.work[2]);  // work_total()
    for (int k = 0; k < 4; ++k) {
      c[k] = p;
      for (size_t e = tid; e < f.in[k]; e += SS_THREADS) p[e] = g.in[k][e];
      p += f.in[k];
    }
    for (int k = 0; k < 3; ++k) { w[k] = p; p += f.work[k]; }
  }
  zc* out0 = g.out0 + (size_t)b * f.out0;
  zc* out1 = g.out1 + (size_t)b * f.out1;
  double* info = g.info + (size_t)b * f.info;
  __syncthreads();

  const int* q = g.dims;
  int rc = SS_OK;
  switch (g.op) {
    case MITDVP_BLOCK_MATMUL: {
      const int M = q[0], N = q[1], K = q[2];
      zc* dst = g.variant == 1 ? c[0] : g.variant == 2 ? c[1] : out0;
      bt_matmul(c[0], c[1], w[0], dst, M, N, K, s_tiles);
      if (dst != out0)
        for (long e = tid; e < (long)M * N; e += SS_THREADS) out0[e] = dst[e];
      break;
    }
    case MITDVP_BLOCK_HEFF: {
      const BatchShape s{q[0], q[1], q[2], q[3], q[4]};
      bt_heff(s, c[0], c[1], c[2], c[3], g.scl, w[0], w[1], out0, s_tiles);
      break;
    }
    case MITDVP_BLOCK_KEFF:
      bt_keff(q[0], q[1], c[0], c[2], c[3], g.scl, w[0], out0, s_tiles);
      break;
    case MITDVP_BLOCK_ENV: {
      const int din = q[0], mi = q[1], d = q[2], dout = q[3], mo = q[4];
      if (g.variant == 0) bt_env(c[0], c[2], c[3], (long)d * dout, dout, 1, c[1], din, mi, d, dout, mo, w[0], w[1], out0, s_tiles);
      else if (g.variant == 1) bt_env(c[0], c[2], c[3], 1, din, (long)d * din, c[1], din, mi, d, dout, mo, w[0], w[1], out0, s_tiles);
      else bt_env_fwd_blk(c[0], c[2], c[3], c[1], din, mi, d, dout, mo, w[0], w[1], out0, s_tiles);
      break;
    }
    case MITDVP_BLOCK_OVERLAP: {
      const int L = q[0];
      if (tid < L) s_shp[tid] = BatchShape{tid == 0 ? 1 : q[1 + tid], q[1], tid == L - 1 ? 1 : q[2 + tid], 1, 1};
      __syncthreads();
      const zc* res = wg_overlap(L, s_shp, [&](int, size_t soff) { return c[0] + soff; }, [&](int, size_t soff) { return c[1] + soff; },
                                 w[0], w[1], w[2], s_tiles);
      if (tid == 0) out0[0] = res[0];
      break;
    }
    case MITDVP_BLOCK_QR: {
      const int m = q[0], n = q[1];
      if (g.variant == 0) bt_qr(c[0], c[0], n, 1, out1, n, 1, m, n, w[0], sh);  // Psi2Asigma
      else bt_qr(c[0], c[0], 1, m, out1, 1, n, m, n, w[0], sh);                 // Psi2sigmaB, on the transpose
      for (long e = tid; e < (long)m * n; e += SS_THREADS) out0[e] = c[0][e];
      break;
    }
    case MITDVP_BLOCK_SPLIT: {
      const int m = q[0], n = q[1], r = q[2];
      for (long e = tid; e < (long)m * n; e += SS_THREADS) w[0][e] = c[0][e];  // the work copy, as bp_apply leaves it
      __syncthreads();
      rc = bp_jacobi(w[0], m, n, ps, sh);
      if (rc != SS_OK) break;
      bp_select_blk(w[0], out0, m, n, r, ps, sh);
      bp_cprime_blk(c[0], out0, out1, m, n, r, 1.0, s_tiles);  // its barriers order the reads of ps below
      if (tid < m) info[3 + ps.rank[tid]] = ps.nrm[tid];
      if (tid == 0) { info[1] = ps.scal[0]; info[2] = ps.scal[1]; }
      break;
    }
    default: break;
  }
  if (tid == 0) info[0] = (double)rc;
}

}  // namespace

void batch_block_launch(hipStream_t st, const BatchBlockArgs& a, int ncopies) {
  if (ncopies < 1 || ncopies > BATCH_BLOCK_MAX_COPIES) throw ArgError("batch_block: ncopies outside 1 .. 16");
  if (!a.out0 || !a.info || !a.work || (a.foot.out1 && !a.out1)) throw ArgError("batch_block: the hook has no buffers");
  for (int k = 0; k < 4; ++k)
    if (a.foot.in[k] && !a.in[k]) throw ArgError("batch_block: an operand is missing");
  hipLaunchKernelGGL(k_batch_block, dim3(ncopies), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_operate_launch(hipStream_t st, const BatchOperateArgs& a, int nsel) {
  if (nsel < 1 || a.L < 1 || a.maxstep < 1) throw ArgError("batch: no replica to apply the operator to");
  if (!a.shp || !a.ptrs || !a.replicas || !a.ops || !a.shift || !a.offs || !a.buf || !a.status || !a.norms || !a.iters ||
      a.carve.total < 1)
    throw ArgError("batch: the operator application has no buffers");
  hipLaunchKernelGGL(k_batch_operate, dim3(nsel), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_cross_mpo_launch(hipStream_t st, const BatchCrossMpoArgs& a, int nentries) {
  if (nentries < 1 || nentries > BATCH_CROSS_MAX_PAIRS || a.L < 1 || a.nrep < 1 || a.nops < 1)
    throw ArgError("batch: no cross entry of an MPO to observe");
  if (!a.entries || !a.shp || !a.ops || !a.shift || !a.buf || !a.rec || a.plan.total < 1)
    throw ArgError("batch: the cross request of MPOs has no buffers");
  hipLaunchKernelGGL(k_batch_cross_mpo, dim3(nentries), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

bool batch_expect_plan(const BatchShape* shp, const int* op_ids, int L, int nops, BatchExpectPlan& plan, std::string& why) {
  plan = BatchExpectPlan{};
  size_t ne = 1, nx = 1, ny = 1, nh = 1;
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
      const size_t n = (size_t)s[p].dl * s[p].d * s[p].dr;
      if (p == 0) {  // the H_eff apply: X (dl ml) x (d dr), Y dl x (d mr) x dr, H C
        nx = std::max(nx, n * s[p].ml);
        ny = std::max(ny, n * s[p].mr);
        nh = std::max(nh, n);
      } else {       // the update of the right block: X (d dl) x (mr dr), Y dl x (ml d) x dr, E (dl, ml, dl)
        nx = std::max(nx, n * s[p].mr);
        ny = std::max(ny, n * s[p].ml);
        ne = std::max(ne, (size_t)s[p].dl * s[p].ml * s[p].dl);
      }
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
  plan.o_h = o; o += nh;
  plan.total = (o + 15) / 16 * 16;
  return true;
}

void batch_expect_launch(hipStream_t st, const BatchExpectArgs& a, int nrep) {
  if (nrep < 1 || a.L < 1) throw ArgError("batch: nothing to launch");
  if (a.nops < 1 || a.nops > BATCH_EXPECT_MAX_OPS || !a.shp || !a.ops || !a.shift || !a.buf || !a.rec || a.plan.total < 1)
    throw ArgError("batch: no operator to take the expectation value of");
  hipLaunchKernelGGL(k_batch_expect, dim3((unsigned)nrep * (unsigned)a.nops), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_sample_launch(hipStream_t st, const BatchSampleArgs& a, int nrep) {
  if (nrep < 1 || a.L < 1) throw ArgError("batch: nothing to launch");
  if (a.nshots < 1 || a.nshots > BATCH_SAMPLE_MAX_SHOTS || (long)a.nshots * a.L > BATCH_SAMPLE_MAX_CONFIG || !a.buf || !a.configs || !a.prob ||
      !a.freq || !a.ids || a.F < a.L)
    throw ArgError("batch: no configurations to sample");
  hipLaunchKernelGGL(k_batch_sample, dim3(nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_spectra_launch(hipStream_t st, const BatchSpecArgs& a, int nrep) {
  if (nrep < 1 || a.L < 2) throw ArgError("batch: nothing to launch");
  if (a.nbonds < 1 || a.nbonds > a.L - 1 || !a.bonds || !a.buf || !a.fail || !a.rec || a.rec_len < 1)
    throw ArgError("batch: no bond spectrum to observe");
  hipLaunchKernelGGL(k_batch_spectra, dim3(nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_cross_launch(hipStream_t st, const BatchCrossArgs& a, int npairs) {
  if (npairs < 1 || npairs > BATCH_CROSS_MAX_PAIRS || a.L < 1 || a.nrep < 1) throw ArgError("batch: no cross pair to observe");
  if (!a.pairs || !a.buf || !a.rec || !a.ops) throw ArgError("batch: the cross request has no buffers");
  hipLaunchKernelGGL(k_batch_cross, dim3(npairs), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_snapshot_launch(hipStream_t st, const BatchShape* shp, void* const* ptrs, int ptr_stride, zc* snap, size_t snap_len, int L,
                           int nrep) {
  if (nrep < 1 || L < 1 || !snap) throw ArgError("batch: nothing to snapshot");
  hipLaunchKernelGGL(k_batch_snapshot, dim3(nrep, L), dim3(256), 0, st, shp, ptrs, ptr_stride, snap, snap_len);
  HIP_CHECK(hipGetLastError());
}

bool batch_pair_fits(const BatchShape* shp, int L, const BatchPlan& plan, int q, std::string& why) {
  const std::string at = "batch: pair channel on bond (" + std::to_string(q) + ", " + std::to_string(q + 1) + "): ";
  if (q < 0 || q + 1 >= L) {
    why = at + "out of range (the chain has " + std::to_string(L) + " sites, bonds (0, 1) to (" + std::to_string(L - 2) + ", " +
          std::to_string(L - 1) + "))";
    return false;
  }
  const long m = (long)shp[q].dl * shp[q].d, n = (long)shp[q + 1].d * shp[q + 1].dr;
  if (m > BATCH_PAIR_MAX_DIM || n > BATCH_PAIR_MAX_DIM) {
    why = at + "the two-site tensor is " + std::to_string(m) + " x " + std::to_string(n) + " (dl d_q x d_{q+1} dr), the split takes at most " +
          std::to_string(BATCH_PAIR_MAX_DIM) + " rows and " + std::to_string(BATCH_PAIR_MAX_DIM) + " columns";
    return false;
  }
  const long room = (long)MAXK * std::max(plan.max_site, plan.max_bond);
  if (2 * m * n > room) {
    why = at + "the two-site tensor and its copy take " + std::to_string(2 * m * n) + " elements, the Krylov-basis carve of the scratch area has " +
          std::to_string(room);
    return false;
  }
  return true;
}

void batch_pair_launch(hipStream_t st, const BatchPairArgs& a, int nrep) {
  if (nrep < 1 || a.c.L < 2) throw ArgError("batch: nothing to launch");
  if (a.c.lo < 0 || a.c.lo >= a.c.L - 1 || !a.pair || !a.pcounts || !a.disc) throw ArgError("batch: no pair channel is set");
  hipLaunchKernelGGL(k_batch_pair, dim3(nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

bool batch_plan(const BatchShape* shp, int L, BatchPlan& plan, std::string& why, int relax, int max_diag_krylov) {
  plan = BatchPlan{};
  for (int p = 0; p < L; ++p) {
    const BatchShape& s = shp[p];
    const long n = (long)s.dl * s.d * s.dr;
    const std::string at = "batch: site " + std::to_string(p) + " (" + std::to_string(s.dl) + ", " + std::to_string(s.d) + ", " +
                           std::to_string(s.dr) + "), MPO bonds (" + std::to_string(s.ml) + ", " + std::to_string(s.mr) + "): ";
    if (s.dl < 1 || s.d < 1 || s.dr < 1 || s.ml < 1 || s.mr < 1) { why = at + "bad shape"; return false; }
    if (n > BATCH_MAX_SITE) {
      why = at + "the site tensor has " + std::to_string(n) + " elements, the batched kernel takes at most " + std::to_string(BATCH_MAX_SITE);
      return false;
    }
    if (s.ml > BATCH_MAX_MPO || s.mr > BATCH_MAX_MPO) {
      why = at + "the batched kernel takes MPO bonds of at most " + std::to_string(BATCH_MAX_MPO);
      return false;
    }
    if (s.dl > BATCH_MAX_BOND || s.dr > BATCH_MAX_BOND) {
      why = at + "the batched kernel takes bonds of at most " + std::to_string(BATCH_MAX_BOND);
      return false;
    }
    if ((p + 1 < L && (long)s.dl * s.d < s.dr) || (p > 0 && (long)s.d * s.dr < s.dl)) {
      why = at + "a bond is wider than the row space it is split from (the gauge move needs dl * d >= dr and d * dr >= dl)";
      return false;
    }
    const long mm = std::max(s.ml, s.mr), dd = std::max(s.dl, s.dr);
    plan.max_site = std::max(plan.max_site, n);
    plan.max_bond = std::max(plan.max_bond, dd * dd);
    // X / Y of an H_eff apply (ml N, mr N), of a K_eff apply (m D^2) and of an environment update (d D^2 m each)
    plan.nx = std::max(plan.nx, std::max(mm * n, mm * dd * dd));
    plan.ny = std::max(plan.ny, mm * n);
  }
  size_t o = 0;
  plan.o_sig = o; o += (size_t)plan.max_bond;
  plan.o_spare = o; o += (size_t)plan.max_site;
  plan.o_work = o; o += (size_t)plan.max_site;
  plan.o_x = o; o += (size_t)plan.nx;
  plan.o_y = o; o += (size_t)plan.ny;
  static_assert(BATCH_EXP_KRYLOV_SLOTS == MAXK, "batch_relax_plan.h repeats vecops.h");
  plan.o_u = o; o += batch_krylov_carve(plan.max_site, plan.max_bond, relax, max_diag_krylov);
  plan.total = o;
  return true;
}

void batch_sweep_launch(hipStream_t st, const BatchArgs& a, int nrep) {
  if (nrep < 1 || a.L < 1) throw ArgError("batch: nothing to launch");
  if (a.e.max_krylov < 1 || a.e.max_krylov > MAXK - 1) throw ArgError("batch: max_krylov must be in [1, 20]");
  hipLaunchKernelGGL(k_batch_sweep, dim3(nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

static void batch_relax_args_ok(const BatchRelaxArgs& a, int nrep) {
  if (nrep < 1 || a.L < 1 || a.nhalf < 1) throw ArgError("batch: nothing to launch");
  if (a.kcap < 2 || a.kcap > BATCH_RELAX_MAX_KRYLOV) throw ArgError("batch: max_diag_krylov must be in [2, 64]");
  if (a.max_restarts < 0 || a.max_restarts > BATCH_RELAX_MAX_RESTARTS) throw ArgError("batch: max_restarts must be in [0, 4096]");
  if (!a.total || !a.most) throw ArgError("batch: the relaxation needs its restart counters");
  if (a.plan.total - a.plan.o_u < batch_krylov_carve(a.plan.max_site, a.plan.max_bond, 2, a.kcap))
    throw ArgError("batch: the Krylov carve is too small for the improved relaxation");
  if ((a.energy != nullptr) != (a.steps != nullptr) || (a.energy != nullptr) != (a.history != nullptr) || (a.energy && a.hist_len < 1))
    throw ArgError("batch: the relaxation's outputs go together");
}

void batch_relax_launch(hipStream_t st, const BatchRelaxArgs& a, int nrep) {
  batch_relax_args_ok(a, nrep);
  hipLaunchKernelGGL(k_batch_relax, dim3(nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_relax_defl_launch(hipStream_t st, const BatchRelaxArgs& a, const BatchDeflArgs& d, int nrep) {
  batch_relax_args_ok(a, nrep);
  if (d.count < 1 || d.count > BATCH_MAX_DEFLATE || !d.w || !d.work) throw ArgError("batch: the deflated relaxation needs its stored states");
  for (int k = 0; k < d.count; ++k)
    if (!d.slot[k]) throw ArgError("batch: a stored state of the deflation set is missing");
  if (d.plan.o_q != (size_t)d.count * d.plan.blk_len || d.plan.per != (size_t)d.count * (d.plan.blk_len + d.plan.max_site) ||
      d.plan.max_site < (size_t)a.plan.max_site)
    throw ArgError("batch: the deflation's work buffer is not laid out for its stored states");
  const BatchRelaxDeflArgs g{a, d};
  hipLaunchKernelGGL(k_batch_relax_defl, dim3(nrep), dim3(SS_THREADS), 0, st, g);
  HIP_CHECK(hipGetLastError());
}

void batch_defl_overlaps_launch(hipStream_t st, const BatchDeflOvArgs& a) {
  if (a.count < 1 || a.count > BATCH_MAX_DEFLATE || a.nrep < 1 || a.L < 1 || !a.buf || !a.rec) throw ArgError("batch: no stored state to overlap with");
  for (int k = 0; k < a.count; ++k)
    if (!a.slot[k]) throw ArgError("batch: a stored state of the deflation set is missing");
  hipLaunchKernelGGL(k_batch_defl_overlaps, dim3(a.count * a.nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_trilow_launch(hipStream_t st, const double* alpha, const double* beta, const int* k, int ncases, double* theta, double* vec) {
  if (ncases < 1 || !alpha || !beta || !k || !theta || !vec) throw ArgError("batch_trilow: nothing to launch");
  hipLaunchKernelGGL(k_batch_trilow, dim3(ncases), dim3(64), 0, st, alpha, beta, k, theta, vec);
  HIP_CHECK(hipGetLastError());
}

void batch_channel_launch(hipStream_t st, const BatchChanArgs& a, int nrep) {
  if (nrep < 1 || a.L < 1) throw ArgError("batch: nothing to launch");
  if (a.lo < 0 || a.lo >= a.L) throw ArgError("batch: no channel is set");
  hipLaunchKernelGGL(k_batch_channel, dim3(nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_field_launch(hipStream_t st, const BatchFieldArgs& a, int nrep) {
  if (nrep < 1 || a.L < 1) throw ArgError("batch: nothing to launch");
  if (a.lo < 0 || a.lo >= a.L || !a.fld || !a.vecs || !a.evals || !a.tables || !a.decay || !a.xi || !a.amp)
    throw ArgError("batch: no field is set");
  hipLaunchKernelGGL(k_batch_field, dim3(nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_observe_plan(const BatchPlan& plan, BatchObsPlan& obs) {
  size_t o = 0;
  obs.o_t = o; o += (size_t)plan.max_bond;
  obs.o_t2 = o; o += (size_t)plan.max_bond;
  obs.o_u = o; o += (size_t)plan.max_site;
  obs.o_x = o; o += (size_t)plan.nx;
  obs.o_y = o; o += (size_t)plan.ny;
  obs.o_h = o; o += (size_t)plan.max_site;
  obs.total = o;
}

void batch_observe_launch(hipStream_t st, const BatchObsArgs& a, int nrep) {
  if (nrep < 1 || a.L < 1) throw ArgError("batch: nothing to launch");
  if (!(a.what & BOBS_ALL) || ((a.what & BOBS_RDM) != 0) != (a.nsites > 0)) throw ArgError("batch: nothing to observe");
  hipLaunchKernelGGL(k_batch_observe, dim3(nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

bool batch_density_plan(const BatchShape* shp, int L, const int* legs, int nkeys, long nrdm, BatchDensPlan& plan, std::string& why) {
  plan = BatchDensPlan{};
  if (nkeys < 0 || (nkeys > 0 && !legs)) { why = "batch: bad list of density keys"; return false; }
  if (nkeys > BATCH_DENS_MAX_KEYS) {
    why = "batch: " + std::to_string(nkeys) + " density keys, one call takes at most " + std::to_string(BATCH_DENS_MAX_KEYS);
    return false;
  }
  for (int k = 0; k < nkeys; ++k) {
    const int* lg = legs + (size_t)k * L;
    std::string name = "batch: density key " + std::to_string(k) + " (legs";
    for (int p = 0; p < L; ++p) name += " " + std::to_string(lg[p]);
    name += "): ";
    int last = -1;
    for (int p = 0; p < L; ++p) {
      if (lg[p] < 0 || lg[p] > 2) { why = name + "the number of legs of site " + std::to_string(p) + " must be 0, 1 or 2"; return false; }
      if (lg[p]) last = p;
    }
    if (last < 0) { why = name + "it keeps no leg (the number of legs must be greater than 0 at one site at least)"; return false; }
    long no = 1;
    for (int p = 0; p <= last; ++p) {
      const long dd = std::max(shp[p].dl, shp[p].dr), d = shp[p].d;
      if (no * dd * dd > BATCH_OBS_MAX_OPEN) {
        why = name + std::to_string(no) + " open legs reach site " + std::to_string(p) + " (bonds " + std::to_string(shp[p].dl) + ", " +
              std::to_string(shp[p].dr) + "): " + std::to_string(no * dd * dd) + " elements of transfer blocks, the batched kernel takes at most " +
              std::to_string(BATCH_OBS_MAX_OPEN);
        return false;
      }
      plan.need = std::max(plan.need, (size_t)(no * dd * dd));
      no *= lg[p] == 2 ? d * d : (lg[p] == 1 ? d : 1);  // <= 65536 * 64 * 64: no overflow
    }
    plan.ndens += no;
    if (nrdm + plan.ndens > BATCH_OBS_MAX_RDM) {
      why = name + "the site RDMs and the keys up to this one have more than " + std::to_string(BATCH_OBS_MAX_RDM) + " elements per replica";
      return false;
    }
  }
  return true;
}

void batch_density_launch(hipStream_t st, const BatchDensArgs& a, int nrep) {
  if (nrep < 1 || a.L < 1) throw ArgError("batch: nothing to launch");
  if (a.nkeys < 1 || !a.legs || !a.tbuf || a.need < 1 || a.dens_off < BOBS_HEAD || a.dens_off >= a.rec_len)
    throw ArgError("batch: no density key to observe");
  hipLaunchKernelGGL(k_batch_density, dim3(nrep), dim3(SS_THREADS), 0, st, a);
  HIP_CHECK(hipGetLastError());
}

void batch_mean_launch(hipStream_t st, const double* rec, const double* w, double* mean, int nrep, long rec_len, long nrec) {
  const long total = nrec * rec_len;
  if (nrep < 1 || total < 1) throw ArgError("batch: nothing to average");
  hipLaunchKernelGGL(k_batch_mean, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, rec, w, mean, nrep, rec_len, nrec);
  HIP_CHECK(hipGetLastError());
}

}  // namespace mitdvp
