// batch_site.h -- batched trajectories (batch_site.hip): ONE workgroup owns one replica's whole chain and walks a
// half-sweep of it inside one launch; the replica index is blockIdx.x, so any number of replicas runs in one grid.
#pragma once
#include <string>

#include "batch_block_check.h"
#include "batch_cross_mpo_plan.h"
#include "batch_deflate_plan.h"
#include "batch_operate_plan.h"
#include "batch_relax_plan.h"
#include "batch_shape.h"
#include "common.h"
#include "small_site.h"

namespace mitdvp {

// Qualifying envelope of k_batch_sweep, decided on the host (the twin of small_chain_plan for this kernel):
//   * dl * d * dr <= BATCH_MAX_SITE elements per site tensor (the kernel keeps nothing of that size in LDS, so the
//     bound is one of scratch memory and time per replica rather than of the hardware: 4096 is d = 4, D = 32),
//   * MPO bonds ml, mr <= BATCH_MAX_MPO,
//   * bonds dl, dr <= BATCH_MAX_BOND (the Householder scalars of a gauge move live in LDS),
//   * dl * d >= dr and d * dr >= dl (a thin QR needs at least as many rows as columns; the sweep requires the same).
// (the three constants BATCH_MAX_SITE = 8192, BATCH_MAX_MPO = 16, BATCH_MAX_BOND = 64 and BatchShape itself are in
// batch_shape.h, which needs no HIP)

struct BatchPlan {
  long max_site = 1;  // largest site tensor, elements
  long max_bond = 1;  // largest bond matrix, elements
  long nx = 1, ny = 1;  // largest M-fold intermediates X, Y of an apply or environment update, elements
  // per-replica scratch carve, offsets in complex elements
  size_t o_sig = 0, o_spare = 0, o_work = 0, o_x = 0, o_y = 0, o_u = 0, total = 0;
};
// false + a message naming the offending site and the limit when the chain is outside the envelope.  relax /
// max_diag_krylov size the Krylov-basis carve (batch_krylov_carve, batch_relax_plan.h): for relax 0 or 1 the plan does not
// depend on them.
bool batch_plan(const BatchShape* shp, int L, BatchPlan& plan, std::string& why, int relax = 0, int max_diag_krylov = 0);

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

// ---- improved relaxation (k_batch_relax) ----
// nhalf half-sweeps of every replica in one launch, the first in direction `forward`, the directions alternating: at every
// site the lowest eigenvector of H_eff + shift by Lanczos (bt_diag; Engine::krylov_diag), then the gauge move, the block
// update and the absorb of k_batch_sweep -- the bond matrix is left alone.  After every backward half-sweep that follows a
// forward one (a full step) the Ritz value of the solve at site 0 is the replica's energy E_n; with conv_tol > 0 a replica
// stops once |E_n - E_{n-1}| <= conv_tol, the others go on.
struct BatchRelaxArgs {
  int L, forward, nhalf;
  int kcap;                 // max_diag_krylov, 2 .. BATCH_RELAX_MAX_KRYLOV; a solve at a site of N elements takes min(N, kcap)
  int max_restarts;         // 0 .. BATCH_RELAX_MAX_RESTARTS thick restarts of one local solve (bt_diag); 0: none, as ever
  double thresh, conv_tol;  // of the local solve (coefficient space); of the energy, 0: never stop early
  const BatchShape* shp;    // [L], device
  void* const* ptrs;        // the pointer table of BatchArgs
  int ptr_stride;
  const zc* shift;          // [B]
  int* kprev;               // [B * L]: the Krylov dimension of the last solve at every site
  int* status;              // [B]: SS_ENOTCONV when a solve did not converge in min(N, kcap) vectors and max_restarts restarts
  long long* stats;         // [B * 4] as BatchArgs: [0] applies (over all cycles of a restarted solve), [2] their flops
  long long* total;         // [B]: restarts taken, added up over the launches
  int* most;                // [B]: the most restarts of any one local solve
  BatchPlan plan;           // sized with relax = 2
  double* energy;           // [B]: the last E_n; null (with steps and history): not recorded
  int* steps;               // [B]: full steps run
  double* history;          // [B][hist_len]: E_1 .. E_n, the rest is left as the host set it (NaN)
  int hist_len;
};
void batch_relax_launch(hipStream_t st, const BatchRelaxArgs& a, int nrep);

// ---- excited states by deflation against stored states (k_batch_relax_defl, k_batch_defl_overlaps) ----
// The same sweep with every local solve on H_eff + shift + sum_k w_k |q_k><q_k|, q_k the stored state phi_k projected
// into the replica's basis at the site (the penalty method).  A stored state is a copy of all site tensors of every
// replica in the snapshot's layout [B][snap_len]; the overlap blocks that give q_k are built at the start of the launch
// and carried through the sweep in `work` (BatchDeflatePlan, batch_deflate_plan.h, which needs no HIP).  E_n is then the
// energy plus sum_k w_k |<phi_k|psi>|^2.  BATCH_MAX_DEFLATE = 8 stored states.
struct BatchDeflArgs {
  int count;                            // stored states, 1 .. BATCH_MAX_DEFLATE
  const zc* slot[BATCH_MAX_DEFLATE];    // [B][snap_len] each, device
  size_t snap_len;                      // sum of the site sizes, complex elements
  const double* w;                      // [count][B]: the weights
  zc* work;                             // [B][plan.per]: blocks [count][blk_len], then q_k [count][max_site]
  BatchDeflatePlan plan;                // for `count` slots
};
struct BatchRelaxDeflArgs {
  BatchRelaxArgs r;
  BatchDeflArgs d;
};
// one launch: grid = nrep workgroups, as batch_relax_launch; the stored states are only read
void batch_relax_defl_launch(hipStream_t st, const BatchRelaxArgs& a, const BatchDeflArgs& d, int nrep);
struct BatchDeflOvArgs {
  int L, nrep, count;
  const BatchShape* shp;                // [L], device
  void* const* ptrs;                    // the pointer table of BatchArgs (only its site tensors are read)
  int ptr_stride;
  const zc* slot[BATCH_MAX_DEFLATE];
  size_t snap_len;
  zc* buf;                              // [count * B][buf_len]: T, its successor and U of each workgroup
  size_t o_t2, o_u, buf_len;            // as BatchCrossArgs
  double* rec;                          // [count][B][2]: (re, im) of <phi_k | psi_r>
};
// one launch: grid = count * nrep workgroups; replicas and stored states are only read
void batch_defl_overlaps_launch(hipStream_t st, const BatchDeflOvArgs& a);
// test hook (k_batch_trilow): the eigen-solve of bt_diag alone, one workgroup of one wave per case.  alpha / beta:
// [ncases][64] diagonal and off-diagonal, k: [ncases] in 1 .. 64; theta: [ncases] the lowest eigenvalue, vec: [ncases][64]
// its unit eigenvector with a non-negative first component, zeros behind k.  All device pointers.
void batch_trilow_launch(hipStream_t st, const double* alpha, const double* beta, const int* k, int ncases, double* theta, double* vec);

// ---- one-site channels between the half-sweeps (k_batch_channel) ----
constexpr int BATCH_MAX_JUMP = 16;  // operators of one jump channel
enum { BCH_NONE = 0, BCH_GATE = 1, BCH_JUMP = 2 };  // the values of MITDVP_CHANNEL_* (include/mitdvp.h)
struct BatchChanSite {
  int kind, nops;   // BCH_*; 1 for a gate, 2 .. BATCH_MAX_JUMP for a jump channel
  long long off;    // first operator in BatchChanArgs::ops, complex elements; nops matrices d x d, row-major, follow
};
struct BatchChanArgs {
  int L, lo;                  // lo: the lowest site that carries a channel
  const BatchShape* shp;      // [L], device
  void* const* ptrs;          // the pointer table of BatchArgs
  int ptr_stride;
  int* status;                // [B]; W == 0 at a jump sets SS_EZERO on that replica
  BatchPlan plan;
  const BatchChanSite* chan;  // [L], device
  const zc* ops;              // device, the operators of all channels
  unsigned long long seed;
  long long step;             // completed time steps of the batch since the seed was set
  const unsigned long long* ids;  // [B] trajectory ids
  long long* counts;          // [B][L][BATCH_MAX_JUMP]: how often operator k of site p was picked
};
// one launch: grid = nrep workgroups.  Precondition: centre at site L - 1, sites 0 .. L-2 in gauge A with valid left
// blocks (the state a forward half-sweep leaves); the same state is left, with the channels applied.
void batch_channel_launch(hipStream_t st, const BatchChanArgs& a, int nrep);

// ---- time-dependent one-site fields between the half-sweeps (k_batch_field) ----
// H(t) = H0 + sum_p a_p(t) G_p, G_p = V diag(g) V^+ Hermitian and a_p real: the one-site unitary exp(-i dt a_p G_p) applied
// IN PLACE to the site tensor (no gauge move), then the left blocks above the lowest field site rebuilt.
constexpr int BATCH_FIELD_MAX_D = 64;  // physical dimension of a site with a field (its d phases live in LDS)
enum { BFLD_NONE = 0, BFLD_TABLE = 1, BFLD_OU = 2 };  // the values of MITDVP_FIELD_* (include/mitdvp.h)
struct BatchFieldSite {
  int kind, d;            // BFLD_*; the order of G
  int ntab, per_replica;  // BFLD_TABLE: entries of the table; 0: one row for all replicas, 1: [B][ntab]
  long long off_v;        // V in BatchFieldArgs::vecs, complex elements: d x d, row-major V[i][k], column k the k-th eigenvector
  long long off_g;        // g in BatchFieldArgs::evals, doubles: d eigenvalues
  long long off_t;        // the table in BatchFieldArgs::tables, doubles
  double sigma;           // BFLD_OU: stationary standard deviation
};
struct BatchFieldArgs {
  int L, lo;                    // lo: the lowest site that carries a field
  const BatchShape* shp;        // [L], device
  void* const* ptrs;            // the pointer table of BatchArgs
  int ptr_stride;
  const int* status;            // [B]: a replica whose word is set does nothing
  BatchPlan plan;
  const BatchFieldSite* fld;    // [L], device
  const zc* vecs;               // device, V of all fields
  const double* evals;          // device, g of all fields
  const double* tables;         // device, the tables of all table fields
  const double* decay;          // [L][2], device: exp(-|dt| / tau) and sigma sqrt(1 - that^2) of the call's dt (BFLD_OU)
  double dt;
  unsigned long long seed;
  long long step;               // completed time steps of the batch since the seed was set (the generator's counter)
  long long clock;              // completed time steps since a field or the seed was last set: the table index; 0 draws xi afresh
  const unsigned long long* ids;  // [B] trajectory ids
  double* xi;                   // [B][L]: the Ornstein-Uhlenbeck values, the generator's only state
  double* amp;                  // [B][L]: the amplitudes applied in this step, 0 where the site carries no field
};
// one launch: grid = nrep workgroups; precondition and result as batch_channel_launch
void batch_field_launch(hipStream_t st, const BatchFieldArgs& a, int nrep);

// ---- nearest-neighbour (pair) channels in the same walk (k_batch_pair) ----
// A pair channel sits on a bond (q, q+1): a gate (one matrix) or a jump channel (2 .. BATCH_MAX_JUMP matrices), each
// (d_q d_{q+1}) x (d_q d_{q+1}), row-major over (i_q, i_{q+1}).  Envelope, decided on the host (batch_pair_fits): the
// two-site tensor theta, seen as (dl d_q) x (d_{q+1} dr), has at most BATCH_PAIR_MAX_DIM rows and columns (row norms,
// ranks and rotation scalars of the split live in LDS), and theta and its copy fit the Krylov-basis carve of the
// replica's scratch area (BatchPlan::o_u), which is idle during the walk.
// (BATCH_PAIR_MAX_DIM = 128: batch_shape.h, which needs no HIP)
// Jacobi sweeps of one split; a replica that reaches it gets SS_ENOTCONV.  The cyclic sweeps run on the rows of theta as
// they are (no preconditioning), so the count grows with the rows and with the spread of the spectrum: up to 60 rows 12
// sweeps were the most seen, but 128 x 128 with singular values graded over 12 decades, or 128 of them 0.8 apart, takes 32
// (tests/test_gpu_batch_blocks.py; the limit was 30 and such a split was SS_ENOTCONV).  A sweep that rotates nothing ends
// the loop, so the limit costs nothing where fewer are needed.
constexpr int BATCH_PAIR_MAX_SWEEPS = 64;
// false + a message naming the bond and the limit
bool batch_pair_fits(const BatchShape* shp, int L, const BatchPlan& plan, int q, std::string& why);
struct BatchPairArgs {
  BatchChanArgs c;            // the walk's own arguments; c.lo: the lowest site that ANY channel touches (a pair on
                              // (q, q+1) touches q); c.ops holds the pair operators too
  const BatchChanSite* pair;  // [L], device: entry q is the channel of bond (q, q+1); entry L-1 is BCH_NONE
  long long* pcounts;         // [B][L][BATCH_MAX_JUMP]: how often operator k of bond (q, q+1) was picked, row q
  double* disc;               // [B]: discarded weight sum_{j>r} sigma_j^2 / sum_j sigma_j^2, added up over the splits
};
// one launch: grid = nrep workgroups; precondition and result as batch_channel_launch
void batch_pair_launch(hipStream_t st, const BatchPairArgs& a, int nrep);

// ---- batched observables (k_batch_observe, k_batch_mean) ----
// what is wanted of an observation: the values of MITDVP_OBS_* (include/mitdvp.h)
enum { BOBS_NORM = 1, BOBS_AUTOCORR = 2, BOBS_ENERGY = 4, BOBS_RDM = 8, BOBS_ALL = 15 };
// One replica's record, in doubles: [0] norm^2, [1] 0, [2, 3] autocorrelation, [4, 5] energy, then the site RDMs of the
// listed sites in list order, d_p * d_p complex numbers each (row = ket, column = bra).  What was not asked is 0.
constexpr int BOBS_HEAD = 6;
constexpr long BATCH_OBS_MAX_RDM = 65536;  // complex elements of all observed RDMs of one replica together

// The observation's own carve of a replica's scratch area, offsets in complex elements from the START OF THE CARVE (the
// carve lies behind the sweep's, BatchPlan::total, which it leaves as it is): the transfer matrix T and its successor
// (max_bond each), U = T C (max_site), and X, Y, H C of the energy's H_eff apply (nx, ny, max_site).
struct BatchObsPlan {
  size_t o_t = 0, o_t2 = 0, o_u = 0, o_x = 0, o_y = 0, o_h = 0, total = 0;
};
void batch_observe_plan(const BatchPlan& plan, BatchObsPlan& obs);

struct BatchObsArgs {
  int L, what, nsites;
  const BatchShape* shp;    // [L], device
  void* const* ptrs;        // the pointer table of BatchArgs
  int ptr_stride;
  const zc* shift;          // [B]
  const int* status;        // [B]: a replica whose word is set does no work, its record is zeros
  const int* sites;         // [nsites], device, strictly ascending
  size_t carve;             // offset of the observation's carve in a replica's scratch area, complex elements
  BatchObsPlan plan;
  double* rec;              // [B][rec_len]: this observation's records
  long rec_len;             // BOBS_HEAD + 2 * sum d_p^2
};
// one launch: grid = nrep workgroups, one record per replica.  Precondition: centre at site 0, sites 1 .. L-1 in gauge B,
// and for BOBS_ENERGY valid right blocks.
void batch_observe_launch(hipStream_t st, const BatchObsArgs& a, int nrep);
// one launch: mean[q][e] = sum_r w[r] rec[q][r][e], r in index order, one thread per (q, e)
void batch_mean_launch(hipStream_t st, const double* rec, const double* w, double* mean, int nrep, long rec_len, long nrec);

// ---- batched multi-site reduced densities (k_batch_density) ----
// A key keeps, per site, both legs (2: ket and bra), the diagonal (1) or nothing (0), as Engine::reduced_density takes
// it.  Its values follow the site RDMs in the replica's record (rec_len = BOBS_HEAD + 2 nrdm + 2 ndens), key after key in
// list order; within a key: kept sites ascending, (ket, bra) per two-leg site, not symmetrised, not normalised.
// Envelope, decided on the host: at most BATCH_DENS_MAX_KEYS keys; legs 0 .. 2, at least one kept; for every key and
// every site up to its last kept one, (open physical legs collected before the site) x (the wider bond of the site)^2
// <= BATCH_OBS_MAX_OPEN complex elements (1 MB per replica and buffer: a pair of two-leg sites at d = 4, D = 32 is
// 16 x 1024; at d = 8, D = 32 it is on the limit; three at d = 4, D = 32 are refused); site RDMs and keys together at
// most BATCH_OBS_MAX_RDM elements per replica.
constexpr int BATCH_DENS_MAX_KEYS = 64;
constexpr long BATCH_OBS_MAX_OPEN = 65536;
struct BatchDensPlan {
  long ndens = 0;   // complex elements of all keys of one replica together
  size_t need = 1;  // largest (open legs x bond matrix) any key reaches: one transfer buffer, complex elements
};
// false + a message naming the key and the limit; legs: [nkeys][L]; nrdm: what the site RDMs of the same record take
bool batch_density_plan(const BatchShape* shp, int L, const int* legs, int nkeys, long nrdm, BatchDensPlan& plan, std::string& why);

struct BatchDensArgs {
  int L, nkeys, zero_head;  // zero_head: no k_batch_observe ran on this record, its head and site RDMs are zeroed here
  const BatchShape* shp;    // [L], device
  void* const* ptrs;        // the pointer table of BatchArgs
  int ptr_stride;
  const int* status;        // [B]: a replica whose word is set does no work, its densities are zeros
  const int* legs;          // [nkeys][L], device
  size_t carve;             // offset of the observation's carve in a replica's scratch area (U = T^T C lives there)
  BatchObsPlan plan;
  zc* tbuf;                 // [B][2][need]: the transfer blocks T_o of a replica and their successors
  size_t need;
  double* rec;              // [B][rec_len]: this observation's records
  long rec_len, dens_off;   // dens_off = BOBS_HEAD + 2 nrdm: where the first key starts
};
// one launch: grid = nrep workgroups.  Precondition: centre at site 0, sites 1 .. L-1 in gauge B.  On the stream of
// batch_observe_launch and behind it when both write one record (k_batch_observe zeroes the whole record first).
void batch_density_launch(hipStream_t st, const BatchDensArgs& a, int nrep);

// ---- cross overlaps and one-site matrix elements between replicas (k_batch_cross, k_batch_snapshot) ----
// A state index 0 .. B-1 names a replica, B .. 2B-1 the snapshot of replica (index - B): the copy of all its site tensors
// that the last batch_snapshot_launch left in the batch's snapshot buffer, [B][sum of site sizes], site after site.
// at most BATCH_CROSS_MAX_PAIRS (batch_shape.h: 65536) pairs in one request
struct BatchCrossPair {
  int bra, ket;   // state indices
  int site;       // site of the operator, -1: the plain overlap <bra | ket>
  int pad;
  long long off;  // the operator in BatchCrossArgs::ops, complex elements: d_site x d_site, row-major [out][in]
};
struct BatchCrossArgs {
  int L, nrep;                 // nrep = B: where the snapshot indices start
  const BatchShape* shp;       // [L], device
  void* const* ptrs;           // the pointer table of BatchArgs (only its site tensors are read)
  int ptr_stride;
  const int* status;           // [B]: a pair that names a replica whose word is set writes zeros
  const zc* snap;              // [B][snap_len], null while no snapshot was taken (no pair may name one then)
  size_t snap_len;             // sum of the site sizes, complex elements
  const BatchCrossPair* pairs; // [P], device
  const zc* ops;               // device, the operators of all pairs
  zc* buf;                     // [P][buf_len]: T, its successor and U of each pair
  size_t o_t2, o_u, buf_len;   // T at 0, its successor at o_t2 (max_bond each), U at o_u (max_site)
  double* rec;                 // [P][2]: (re, im) of each pair's value
};
// one launch: grid = npairs workgroups, replicas and snapshots are only read
void batch_cross_launch(hipStream_t st, const BatchCrossArgs& a, int npairs);
// one launch: grid = (nrep, L), site p of replica r copied to snap[r][offset of site p]
void batch_snapshot_launch(hipStream_t st, const BatchShape* shp, void* const* ptrs, int ptr_stride, zc* snap, size_t snap_len, int L,
                           int nrep);

// ---- bond spectra and entanglement entropies (k_batch_spectra) ----
// The request is a strictly ascending list of bonds q in 0 .. L-2; bond q lies between sites q and q+1 (named by its left
// site, as the pair channels are) and has dimension chi_q = dr of site q.  One replica's record, in doubles, for every
// listed bond in list order: [0] W = sum sigma^2 (summed in descending order of sigma^2; the replica's norm^2), [1] S1 =
// -sum p ln p with p = sigma^2 / W (a term with p <= 0 counts as 0), [2] S2 = -ln sum p^2, [3] pmin = the smallest p, then
// the chi_q values sigma^2, descending, not normalised.  W == 0 gives S1 = S2 = pmin = 0.
constexpr int BSPEC_HEAD = 4;
struct BatchSpecArgs {
  int L, nbonds;
  const BatchShape* shp;    // [L], device
  void* const* ptrs;        // the pointer table of BatchArgs (only its site tensors are read)
  int ptr_stride;
  const int* status;        // [B]: a replica whose word is set does no work, its record is zeros
  const int* bonds;         // [nbonds], device, strictly ascending
  zc* buf;                  // [B][buf_len]: the walk's tensor X, the QR work matrix and R of each replica
  size_t o_work, o_r, buf_len;  // X at 0 and the work matrix at o_work (max_site each), R at o_r (max_bond)
  int* fail;                // [B]: 1 + the bond whose Jacobi sweeps did not converge; the kernel only ever sets it
  double* rec;              // [B][rec_len]: this observation's records
  long rec_len;             // sum over the listed bonds of BSPEC_HEAD + chi_q
};
// one launch: grid = nrep workgroups, the replicas are only read.  Precondition: centre at site 0, sites 1 .. L-1 in
// gauge B.
void batch_spectra_launch(hipStream_t st, const BatchSpecArgs& a, int nrep);

// ---- sampled configurations (k_batch_sample) ----
// A configuration is one basis index per site, drawn with probability |<j_0 .. j_{L-1}|psi>|^2 / <psi|psi>.  Shot t of a
// replica walks the chain once, left to right: v = [1]; at site p, w[j][s] = sum_a v[a] C_p[a][j][s], g_j = sum_s
// |w[j][s]|^2, the outcome j by the selection rule of the jump channels (bc_pick) on the uniform of (seed, trajectory id,
// step, site, shot), v <- w[j][:] / sqrt(g_j), prob <- prob g_j / G.  G == 0 gives -1 from that site on and prob = 0.
// Shots are processed BATCH_SAMPLE_CHUNK at a time; a shot's bits depend neither on the chunk it fell into nor on nshots.
constexpr int BATCH_SAMPLE_CHUNK = 64;
constexpr int BATCH_SAMPLE_MAX_SHOTS = 65536;     // shots of one request
constexpr long BATCH_SAMPLE_MAX_CONFIG = 1L << 22;  // nshots * L, the int32 entries of one replica's configurations
constexpr int BATCH_SAMPLE_LDS_D = 16;  // up to this physical dimension (that of the channels' operators) a chunk's weights live in LDS
struct BatchSampleArgs {
  int L, nshots;
  const BatchShape* shp;    // [L], device
  void* const* ptrs;        // the pointer table of BatchArgs (only its site tensors are read)
  int ptr_stride;
  const int* status;        // [B]: a replica whose word is set writes -1 and zeros
  unsigned long long seed;  // the request's own seed
  long long step;           // completed time steps of the batch since the seed was set (the jump channels' counter)
  const unsigned long long* ids;  // [B] trajectory ids
  zc* buf;                  // [B][buf_len]: V (chunk x widest bond), W (chunk x widest d dr), then a chunk's weights
  size_t o_w, o_g, buf_len; // V at 0, W at o_w, the weights (doubles, chunk x widest d) at o_g; complex elements
  int* configs;             // [B][nshots][L]
  double* prob;             // [B][nshots]
  double* freq;             // [B][F], F = sum d_p: entry (p, j) is count / nshots
  long F;
};
// one launch: grid = nrep workgroups, the replicas are only read.  Precondition: centre at site 0, sites 1 .. L-1 in
// gauge B.
void batch_sample_launch(hipStream_t st, const BatchSampleArgs& a, int nrep);

// ---- expectation values of MPO observables (k_batch_expect) ----
// The request is a list of operator ids; every replica carries each of them as a whole MPO (Engine::set_mpo_core packs
// w2l / w2el / w2er for every id).  The value of (replica r, operator k) is <psi_r | O_k | psi_r> + shift_k <psi_r | psi_r>,
// not normalised, by the arithmetic of Engine::expect: a fresh walk of the right blocks of O_k from the right boundary to
// bond 1 and one H_eff apply at site 0.  One replica's record, in doubles: (re, im) of every listed operator in list order.
constexpr int BATCH_EXPECT_MAX_OPS = 64;
// One (replica, operator) pair's carve of the request's buffer, offsets in complex elements: the two right blocks the
// walk writes alternately (E0 at 0, E1 at o_e1: the largest dl * ml_k * dl of sites 1 .. L-1 each), X and Y (the largest
// either bt_env or the site-0 bt_heff needs) and H C (the site-0 tensor).  The maxima run over all listed operators: every
// pair has the same carve.
struct BatchExpectPlan {
  size_t o_e1 = 0, o_x = 0, o_y = 0, o_h = 0, total = 0;
};
// shp: [nops][L], the site shapes with operator k's MPO bonds; op_ids: [nops], the names of the operators.  false + a
// message naming the operator, the site and the limit when an MPO bond is outside 1 .. BATCH_MAX_MPO, the bonds of
// neighbouring cores differ or the outer ones are not 1.
bool batch_expect_plan(const BatchShape* shp, const int* op_ids, int L, int nops, BatchExpectPlan& plan, std::string& why);
struct BatchExpectArgs {
  int L, nops;
  const BatchShape* shp;    // [nops][L], device: operator k's ml / mr at every site
  void* const* ptrs;        // the pointer table of BatchArgs (its site tensors, left block 0 and right block L are read)
  int ptr_stride;
  void* const* ops;         // [B][nops][3 L], device: w2l, w2el (not read), w2er of operator k of replica r
  const zc* shift;          // [B][nops]
  const int* status;        // [B]: a replica whose word is set does no work, its values are zeros
  zc* buf;                  // [B][nops][plan.total]
  BatchExpectPlan plan;
  double* rec;              // [B][2 nops]: this observation's records
};
// one launch: grid = nrep * nops workgroups, workgroup r * nops + k; replicas and operators are only read.  Precondition:
// centre at site 0, sites 1 .. L-1 in gauge B.
void batch_expect_launch(hipStream_t st, const BatchExpectArgs& a, int nrep);

// ---- MPO matrix elements between replicas (k_batch_cross_mpo) ----
// An entry is (bra, ket, operator): the state indices are BatchCrossPair's (0 .. B-1 a replica, B + r the snapshot of
// replica r), the operator is an index into the request's list of distinct operator ids, which every replica carries as
// a whole MPO.  The cores and the scalar term used are those of the ket's owner, replica ket mod B.  The value is
// <psi_bra | O | psi_ket> + shift <psi_bra | psi_ket>, not normalised: a walk of the left block T (bra bond, MPO bond,
// ket bond) over all L sites in the three stages of the forward environment update, conj of the bra tensor in stage 1
// and the ket tensor in stage 3; then, for a non-zero shift, k_batch_cross's plain-overlap walk.
// BATCH_CROSS_MPO_MAX_BYTES, BatchCrossMpoEntry, BatchCrossMpoPlan, batch_cross_mpo_plan, batch_cross_mpo_fits and the check
// of a request's entries, batch_cross_mpo_entries_ok: batch_cross_mpo_plan.h, which needs no HIP.
struct BatchCrossMpoArgs {
  int L, nrep, nops;                  // nrep = B: where the snapshot indices start; nops distinct operators
  const BatchShape* shp;              // [nops][L], device: operator k's ml / mr at every site
  void* const* ptrs;                  // the pointer table of BatchArgs (only its site tensors are read)
  int ptr_stride;
  const int* status;                  // [B]: an entry that names a replica whose word is set writes zeros
  const zc* snap;                     // [B][snap_len], null while no snapshot was taken (no entry may name one then)
  size_t snap_len;                    // sum of the site sizes, complex elements
  const BatchCrossMpoEntry* entries;  // [P], device
  void* const* ops;                   // [B][nops][L], device: w2el of operator k of replica r at every site
  const zc* shift;                    // [B][nops]
  zc* buf;                            // [P][plan.total]
  BatchCrossMpoPlan plan;
  double* rec;                        // [P][2]: (re, im) of each entry's value
};
// one launch: grid = nentries workgroups; replicas, snapshots and operators are only read
void batch_cross_mpo_launch(hipStream_t st, const BatchCrossMpoArgs& a, int nentries);

// ---- an MPO applied to the replicas: the variational fit of Engine::operate (k_batch_operate) ----
// phi ~ O|psi> / |O|psi>| in the bond dimensions of psi, for every SELECTED replica, the whole fit in one launch: up to
// maxstep double sweeps in which every site tensor of the bra (the replica's own tensors) is replaced by the mixed-block
// apply on the ket (a copy of the replica's tensors in the request's buffer), each replica stopping on its own when
// |1 - |<phi_i | phi_{i-1}>|| < conv_tol.  The kernel WRITES the replica: on return its tensors are phi, normalised,
// centre at site 0, sites 1 .. L-1 in gauge B.  BATCH_OPERATE_MAX_BYTES, BatchOperatePlan, batch_operate_plan and
// batch_operate_fits: batch_operate_plan.h, which needs no HIP.
struct BatchOperateCarve {  // the offsets of BatchOperatePlan, complex elements
  size_t o_ket, o_prev, o_mix, o_ov, o_x, o_y, o_work, o_spare, o_h, o_sig, o_t0, o_t1, o_id, total;
};
struct BatchOperateArgs {
  int L, maxstep;
  double conv_tol;
  const BatchShape* shp;   // [L], device: the site shapes with the operator's ml / mr
  void* const* ptrs;       // the pointer table of BatchArgs (only its site tensors are used: read AND written)
  int ptr_stride;
  const int* replicas;     // [nsel], device: workgroup j owns replica replicas[j]
  void* const* ops;        // [nsel][3][L], device: w2l, w2el, w2er of the operator on workgroup j's replica
  const zc* shift;         // [nsel]: the operator's scalar term
  const long long* offs;   // [3][L + 1], device: BatchOperatePlan::site, mix, ov
  zc* buf;                 // [nsel][carve.total]
  BatchOperateCarve carve;
  int* status;             // [B], by replica: SS_EZERO when an apply gave a norm that is not > 0
  double* norms;           // [nsel]: the norm of the last apply at site 0; 0 for a replica that stopped
  int* iters;              // [nsel]: double sweeps run
};
// one launch: grid = nsel workgroups
void batch_operate_launch(hipStream_t st, const BatchOperateArgs& a, int nsel);

// ---- test hook: one building block of the kernels above in one workgroup (k_batch_block) ----
// Workgroup b copies the operands into its own part of work, runs the block on that copy with the LDS carve of
// k_batch_pair, and writes its own copy of the results.  The shapes and footprints are batch_block_check.h's; the caller
// has checked them (batch_block_check) -- the kernel itself checks nothing.
struct BatchBlockArgs {
  int op, variant;          // MITDVP_BLOCK_*
  int dims[8];
  double scl;
  const zc* in[4];          // one copy of each operand, foot.in[k] elements
  zc *out0, *out1;          // [ncopies][foot.out0], [ncopies][foot.out1]
  double* info;             // [ncopies][foot.info]
  zc* work;                 // [ncopies][foot.work_total()]: the operands' copies, then the three work areas
  BatchBlockFoot foot;
};
// one launch: grid = ncopies workgroups
void batch_block_launch(hipStream_t st, const BatchBlockArgs& a, int ncopies);

}  // namespace mitdvp
