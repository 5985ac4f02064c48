/*
 * mitdvp.h -- C ABI of the MI355X-native one-site TDVP sweep engine.
 *
 * This is the drop-in boundary for PyTDSCF's hot path.  Every entry point
 * names the reference interface it replaces (paths relative to
 * /root/reference/pytdscf).  The coarse seam is
 *     MPSCoef.propagate(stepsize_au, ints_spf, matH)      _mps_cls.py:452-503
 * called once per time step from WFunc.propagate_SM        wavefunction.py:408-412
 * plus the observables MPSCoef.expectation / autocorr / norm / pop_states
 * (_mps_cls.py:540-716, wavefunction.py:226-257).
 *
 * Conventions
 *   - all tensors are complex128, C order, passed as interleaved (re, im)
 *     doubles; host buffers are copied in/out, the handle owns device memory;
 *   - site tensor psi[b][j][s]      shape (D_l, d, D_r)   _site_cls.py:27-60
 *   - MPO core    W[c][i][j][t]     shape (M_l, d, d, M_r) _mpo_cls.py:166-198
 *   - every function returns 0 on success, a negative MITDVP_E* code on error;
 *     mitdvp_last_error() gives the message.  The Python shell maps
 *     MITDVP_ENOTCONV to ValueError like _integrator.py:430,653.
 *   - a handle is bound to one GPU and one HIP stream and is not thread safe.
 */
#ifndef MITDVP_H
#define MITDVP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mitdvp_engine mitdvp_engine;

enum {
  MITDVP_OK = 0,
  MITDVP_EINVAL = -1,   /* bad argument / shape                        */
  MITDVP_EHIP = -2,     /* HIP runtime error                           */
  MITDVP_ENOTCONV = -3, /* Krylov not converged in 20 vectors          */
  MITDVP_ESTATE = -4,   /* call sequence error (e.g. missing tensors)  */
  MITDVP_ENOMEM = -5
};

enum { MITDVP_LANCZOS = 0, MITDVP_ARNOLDI = 1 };
enum { MITDVP_GAUGE_C = -1 /* no gauge */, MITDVP_GAUGE_PSI = 0, MITDVP_GAUGE_A = 1, MITDVP_GAUGE_B = 2 };

/* const.set_runtype(...) flags that reach the sweep (_const_cls.py:102-252). */
typedef struct {
  int nsite;            /* chain length L                                   */
  int device;           /* HIP device ordinal                               */
  int integrator;       /* MITDVP_LANCZOS | MITDVP_ARNOLDI  (:integrator)   */
  int conserve_norm;    /* const.conserve_norm, _integrator.py:189-213      */
  int relax;            /* 0 real time; 1 imaginary time (const.doRelax = True);
                           2 improved relaxation (doRelax = "improved": Lanczos
                           ground state of H_eff per site, _integrator.py:74-138) */
  double thresh;        /* const.thresh_exp, default 1e-9                   */
  int max_krylov;       /* 20, _integrator.py:182                           */
  int lanczos_variant;  /* 0: reference alpha_l=<v0|H|v_l> (_integrator.py:556)
                           1: orthodox alpha_l=<v_l|H|v_l>                  */
  int max_diag_krylov;  /* Krylov vectors kept by the improved-relaxation solver
                           (0 = default 64; the reference allows up to 3000)   */
  int cu_first, cu_count; /* > 0: the engine's stream is confined to cu_count compute units starting at cu_first
                             (hipExtStreamCreateWithCUMask; unit u = CU u / 8 of XCD u % 8, so a range of 8 k units is
                             k CUs on every XCD): several engines of one process with DISJOINT ranges run side by side
                             without ever competing for a compute unit -- an ensemble of trajectories in the small-bond
                             regime (mitdvp_ensemble_step).  0 = the whole device.                                     */
  int reserved[5];
} mitdvp_config;

/* -- lifetime ----------------------------------------------------------
 * Threading: a handle owns one HIP stream and all its device memory and must be driven by one host
 * thread at a time; different handles are independent and may be driven concurrently from different
 * threads (an ensemble of trajectories on one GPU). */
int mitdvp_create(const mitdvp_config* cfg, mitdvp_engine** out);
void mitdvp_destroy(mitdvp_engine* h);
const char* mitdvp_last_error(const mitdvp_engine* h); /* h may be NULL */
const char* mitdvp_version(void);
/* Number of HIP devices visible to this process (0 without a GPU; no engine needed).  Lets a launcher map
 * ranks to devices (rank % count) without importing a second GPU runtime. */
int mitdvp_device_count(int* count);
int mitdvp_device_cu_count(int device, int* count); /* compute units of a device (256 on MI355X): what cu_first / cu_count divide */
/* hipDeviceSynchronize on `device`: the fence bench.py puts on both sides of its timed region (the engine's
 * stream is private, so a foreign runtime's "current stream" synchronise would not see its work). */
int mitdvp_device_sync(int device);

/* -- state: superblock_states[0][isite] (SiteCoef), _site_cls.py:27-60 --- */
int mitdvp_set_site(mitdvp_engine* h, int isite, const double* reim, int l, int n, int r, int gauge);
int mitdvp_get_site_shape(mitdvp_engine* h, int isite, int* l, int* n, int* r, int* gauge);
int mitdvp_get_site(mitdvp_engine* h, int isite, double* reim_out);
/* Device-side full-rank random MPS with LatticeInfo.get_bond_dim bond
 * dimensions (_mps_cls.py:2616-2631), canonicalised right->left like
 * alloc_superblock_random (:2684-2699).  For workloads too large to stage
 * through the host. */
int mitdvp_init_random(mitdvp_engine* h, const int* dims, int bond_dim, uint64_t seed);
/* The raw (not canonicalised) tensors mitdvp_init_random draws for sites [first, first + nsite) of an nsite_total-site
 * chain (shapes and seeds follow the GLOBAL site index; h holds nsite sites): one block of a site-range sharded state
 * (MPSCoefParallel keeps one block per rank, _mps_parallel.py:64-118) without the whole chain on every rank; the ranks
 * then canonicalise in a pipeline with mitdvp_split_center / mitdvp_absorb_bond.  balance != 0: each tensor times the
 * largest power of two <= 1 / sqrt(d_l d), so the weight handed along the chain stays O(1). */
int mitdvp_init_random_block(mitdvp_engine* h, const int* dims, int nsite_total, int first, int bond_dim, uint64_t seed, int balance);
/* alloc_superblock_random's C2sigmaB sweep for tensors given by set_site
 * with gauge "C": site 0 becomes "Psi", scaled to norm `scale`; scale <= 0 keeps
 * the state's own normalisation (Liouville space: trace-normalised start,
 * _mps_cls.py:2695-2699). */
int mitdvp_canonicalize(mitdvp_engine* h, double scale);

/* -- operators: TensorHamiltonian.mpo[0][0] after reduction to one
 *    full-chain 4-leg MPO (hamiltonian_cls.py:618-752, _mpo_cls.py:44-234).
 *    op_id 0 is the Hamiltonian used by mitdvp_step; others are observables. */
int mitdvp_set_mpo_core(mitdvp_engine* h, int op_id, int isite, const double* reim,
                        int ml, int d_out, int d_in, int mr);
/* coupleJ[0][0] * ovlp term (_contraction.py:1200-1216): adds shift*psi. */
int mitdvp_set_shift(mitdvp_engine* h, int op_id, double re, double im);

/* -- the hot path ------------------------------------------------------- */
/* MPSCoef.propagate: forward + backward half-sweep with dt/2 each
 * (_mps_cls.py:482-500).  First call builds all right environments
 * (:835-843); the cache is reused afterwards (:848-861). */
int mitdvp_step(mitdvp_engine* h, double dt_au);
/* nsteps time steps of n independent engines at once (independent trajectories / replicas of one model: SURVEY 7 step 6,
 * 8e "fallback"; the reference averages trajectories in a Python loop, tests/test_mixedstate.py:269-308): every engine is
 * driven by its own host thread inside this call.  Meant for engines created with disjoint cu_first / cu_count ranges (see
 * mitdvp_config): their launches then overlap on the chip without any admission control.  Returns the first non-zero
 * status (that engine's mitdvp_last_error holds the message); statuses[i] (may be NULL) receives each engine's own. */
int mitdvp_ensemble_step(mitdvp_engine** hs, int n, double dt_au, int nsteps, int* statuses);

/* Batched trajectories: any number of replicas of one chain shape stepped by ONE kernel launch per half-sweep for the whole
 * batch (k_batch_sweep: one workgroup owns one replica, the replica index is the workgroup index; no host threads, no
 * compute-unit ranges, no limit of 16).  Replicas are ordinary engine handles -- each owns its tensors and its own MPO, so
 * per-replica Hamiltonians work -- which the batch borrows; it owns the pointer tables, status words and scratch only, and
 * must be destroyed before the engines.  mitdvp_batch_create returns MITDVP_EINVAL (message: mitdvp_last_error(NULL)) and
 * leaves every engine untouched unless: all handles are distinct and on one device, none is confined to a compute-unit
 * range (cu_count == 0), each is a single electronic state, none is adaptive, a segment or bond-sharded, relax is 0, 1
 * or 2 (with 2, improved relaxation, max_diag_krylov -- 0 means 64 -- is in 2 .. 64 and identical across the replicas),
 * no gates or Kraus maps are set, site and MPO shapes are identical across the replicas at every site, integrator,
 * lanczos_variant, conserve_norm, thresh, max_krylov and relax are identical, and the shapes are inside the kernel's
 * envelope: dl*d*dr <= 8192 per site (d = 4, D = 32 is 4096), MPO bonds <= 16, bonds <= 64, dl*d >= dr and d*dr >= dl; the
 * message names the offending site and the limit.  The same checks run again at every step: engines may be used on their
 * own (setters, propagate, observables) between batch calls.
 *   mitdvp_batch_step : nsteps time steps (forward and backward half-sweep each) of every replica; all engines must have
 *                       their centre at site 0, as for mitdvp_step.  Two launches per time step, whatever n and nsite.
 *   mitdvp_batch_sweep: one half-sweep.
 * Afterwards every engine is an ordinary consistent engine (centre, gauges, environment cache, Krylov memories, counters;
 * n_launch counts the batch's launches once, on replica 0).  statuses[i] (may be NULL) receives replica i's own status; the
 * call returns the first non-zero one.  A replica that fails (MITDVP_ENOTCONV: its local exponential did not converge in
 * max_krylov vectors) stops working, the others finish; its message is in mitdvp_last_error(hs[i]), and its state was left
 * in the middle of a half-sweep: the caller must set its tensors again (set_site / init_random + canonicalize) before
 * using it further. */
typedef struct mitdvp_batch mitdvp_batch;
int mitdvp_batch_create(mitdvp_engine** hs, int n, mitdvp_batch** out);
int mitdvp_batch_step(mitdvp_batch* b, double dt_au, int nsteps, int* statuses);
int mitdvp_batch_sweep(mitdvp_batch* b, double dt_au, int forward, int* statuses);
void mitdvp_batch_destroy(mitdvp_batch* b);
/* Observables of a batch without a walk over its engines (k_batch_observe: one workgroup per replica, ONE launch observes
 * every replica; k_batch_mean: ONE launch forms the ensemble means on the device, replica after replica in index order).
 * `what` is a non-empty set of MITDVP_OBS_* bits; MITDVP_OBS_RDM goes with a strictly ascending list `sites` of nsites
 * sites (one-site reduced densities, d x d, row = ket, column = bra, not symmetrised, as mitdvp_site_rdm), and only with
 * it.  All replicas must have their centre at site 0 with the chain canonical around it (the state mitdvp_batch_step
 * leaves); for MITDVP_OBS_ENERGY (operator 0, as mitdvp_expect) the right environment blocks are built once with the
 * engines' own launches when no step has built them yet.  weights: n doubles or NULL (1 / n each).
 * Every pointer of `out` may be NULL.  Per replica, record-major ([record][replica]...): norm (the root, as mitdvp_norm),
 * autocorr[..][2], energy[..][2], rdm[..][nrdm][2] with nrdm = the sum of d_p * d_p over the listed sites, in list order.
 * Means over the replicas ([record]...): mean_norm2 (the mean of the SQUARED norms), mean_autocorr, mean_energy, mean_rdm.
 * counts (may be NULL) receives {records, replicas, nrdm}; with out == NULL the call only validates what does not depend
 * on the engines' state and returns the counts, like mitdvp_reduced_density.
 *   mitdvp_batch_observe: one observation of the current state: two launches, one host wait.
 *   mitdvp_batch_run    : nsteps time steps as mitdvp_batch_step, recording the state before step 0 and after every
 *                         `every`-th step (nsteps must be a multiple of every; nsteps / every + 1 records).  The records
 *                         stay on the device until the end: the call has the one host wait of mitdvp_batch_step, and
 *                         2 nsteps + records + 1 launches, whatever n and nsites.  Asking for the means only is the cheap
 *                         form.  A replica that fails to converge behaves as in mitdvp_batch_step; its records from then
 *                         on are zeros, the call returns its status, and the MEANS of such a call are not usable.
 * A refused request (MITDVP_EINVAL, message: mitdvp_last_error(NULL)) leaves every engine untouched. */
#define MITDVP_OBS_NORM 1
#define MITDVP_OBS_AUTOCORR 2
#define MITDVP_OBS_ENERGY 4
#define MITDVP_OBS_RDM 8
typedef struct mitdvp_batch_out {
  double *norm, *autocorr, *energy, *rdm;
  double *mean_norm2, *mean_autocorr, *mean_energy, *mean_rdm;
} mitdvp_batch_out;
int mitdvp_batch_observe(mitdvp_batch* b, const int* sites, int nsites, int what, const double* weights,
                         const mitdvp_batch_out* out, size_t counts[3]);
int mitdvp_batch_run(mitdvp_batch* b, double dt_au, int nsteps, int every, const int* sites, int nsites, int what,
                     const double* weights, const mitdvp_batch_out* out, size_t counts[3], int* statuses);
/* Multi-site reduced densities of a batch (k_batch_density: one workgroup per replica, ONE launch forms every key of every
 * replica; the one k_batch_mean launch of the call averages them with everything else).  A key is a row of nsite leg
 * counts as mitdvp_reduced_density takes it -- 2: ket and bra leg kept, 1: the diagonal, 0: traced out -- and its values
 * have that call's layout bit for bit: kept sites ascending, (ket, bra) per two-leg site, not symmetrised, not normalised.
 * remain_nleg is [nkeys][nsite]; the keys' values are concatenated in list order, ndens complex numbers per replica:
 * density[record][replica][ndens][2], mean_density[record][ndens][2]; either may be NULL.  sites / what / weights / out are
 * those of mitdvp_batch_run, except that `what` may be 0 (and out NULL) when nkeys > 0; with nkeys == 0 the two calls ARE
 * mitdvp_batch_observe / mitdvp_batch_run: the same bits, the same refusals.  counts (may be NULL) receives {records,
 * replicas, nrdm, ndens}; with out == NULL && density == NULL && mean_density == NULL the call only validates what does
 * not depend on the engines' state and returns the counts.  The state required is that of mitdvp_batch_observe (centre at
 * site 0).  Launches: per record one more than without keys, and k_batch_observe is skipped when what == 0, so a record
 * costs at most two; mitdvp_batch_run_keys makes at most 2 nsteps + 2 records + 1.  A replica that failed has zeros.
 * MITDVP_EINVAL (message: mitdvp_last_error(NULL), naming the key and the limit; every engine untouched) when a leg count
 * is outside 0 .. 2, a key keeps no leg, there are more than 64 keys, for some key and site (open physical legs collected
 * before the site) x (the wider bond of the site)^2 exceeds 65536 complex elements (1 MB per replica and buffer: two
 * two-leg sites at d = 4, D = 32 are 16 x 1024; at d = 8, D = 32 they are on the limit; three at d = 4 are refused), the
 * site RDMs and all keys together exceed 65536 elements per replica, or the centre is not at site 0. */
int mitdvp_batch_observe_keys(mitdvp_batch* b, const int* sites, int nsites, const int* remain_nleg, int nkeys, int what,
                              const double* weights, const mitdvp_batch_out* out, double* density, double* mean_density,
                              size_t counts[4]);
int mitdvp_batch_run_keys(mitdvp_batch* b, double dt_au, int nsteps, int every, const int* sites, int nsites,
                          const int* remain_nleg, int nkeys, int what, const double* weights, const mitdvp_batch_out* out,
                          double* density, double* mean_density, size_t counts[4], int* statuses);
/* One-site channels of a batch, applied between the two half-sweeps of every time step -- the slot of the reference's
 * one_gate_to_apply (_mps_cls.py:489-492) -- by ONE more launch per step for the whole batch (k_batch_channel: one workgroup
 * per replica walks the centre from site L-1 down to the lowest site with a channel, applying each site's channel to the
 * centre tensor, and back up, rebuilding the left blocks).  While at least one channel is set a time step of
 * mitdvp_batch_step / mitdvp_batch_run is three launches; with none set nothing changes.
 *   mitdvp_batch_set_channel: `ops_reim` holds nops matrices d x d (row-major [k][out][in], interleaved re / im) for `site`;
 *       NULL removes the site's channel.  MITDVP_CHANNEL_GATE (nops == 1): C[a,i,s] = sum_j U[i,j] C[a,j,s], as is -- U need
 *       not be unitary.  MITDVP_CHANNEL_JUMP (2 <= nops <= 16): a Kraus channel {B_k} unravelled into quantum jumps: with
 *       the centre at the site, w_k = |B_k C|^2, W = sum_k w_k in index order, one uniform u in [0, 1), the smallest k
 *       whose running sum exceeds u W (if rounding leaves none, the last k with w_k > 0), and C <- B_k C sqrt(|C|^2 / w_k):
 *       the norm before the jump is kept.  W == 0 stops that replica only (MITDVP_EINVAL in its status, "zero norm" in
 *       its message; its tensors must be set again, as after MITDVP_ENOTCONV).  MITDVP_EINVAL (message:
 *       mitdvp_last_error(NULL), nothing changed, every engine untouched) when the site is out of range, d is not the
 *       site's physical dimension, nops is out of range for the kind, or the replicas run in imaginary time (relax == 1);
 *       the message names the site and the limit.  mitdvp_batch_sweep (a single half-sweep) refuses while a channel is set.
 *   mitdvp_batch_set_seed: the generator is counter-based, no state is stored: with mix(z) = { z ^= z >> 30;
 *       z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 } on 64-bit unsigned integers,
 *       key = mix(mix(mix(seed ^ trajectory_id) + step) + site) and u = (key >> 11) * 2^-53, where step counts the batch's
 *       completed time steps since this call (or creation: seed 0) -- the batch's count, advanced by every
 *       mitdvp_batch_step / mitdvp_batch_run whether or not a channel is set and whatever the replicas' statuses are; it
 *       does not say how far a replica that failed got.  trajectory_ids: n numbers, NULL = 0 .. n-1; a
 *       replica's draws depend on its id only, not on n or its place in the batch.  Resets the step counter and the jump
 *       counters.
 *   mitdvp_batch_jump_counts: counts[n][nsite][16] (long long), how often operator k of a site's jump channel was picked
 *       since the last mitdvp_batch_set_seed; sites without a jump channel are zeros.  One host wait. */
#define MITDVP_CHANNEL_GATE 1
#define MITDVP_CHANNEL_JUMP 2
int mitdvp_batch_set_channel(mitdvp_batch* b, int site, int kind, const double* ops_reim, int nops, int d);
int mitdvp_batch_set_seed(mitdvp_batch* b, unsigned long long seed, const unsigned long long* trajectory_ids);
int mitdvp_batch_jump_counts(mitdvp_batch* b, long long* counts);
/* Nearest-neighbour (pair) channels of a batch, in the same walk between the two half-sweeps: while at least one is set
 * the walk is run by k_batch_pair in the place of k_batch_channel -- still ONE more launch per step for the whole batch;
 * with none set nothing changes.  A pair channel sits on the bond (site, site + 1), 0 <= site < nsite - 1.  Walking
 * down with the centre at p, the one-site channel of p acts first; then, if bond (p-1, p) carries a pair channel, it
 * takes the place of that step's gauge move: merge theta[a,i,j,s] = sum_b A_{p-1}[a,i,b] C_p[b,j,s], apply the operator
 * on (i, j), split theta ~ C'_{p-1} B_p with B_p of r orthonormal rows, r the bond's dimension as it is (shapes never
 * change; one-sided Jacobi SVD inside the workgroup), C'_{p-1} = theta B_p^+.  The walk goes down to the lowest site
 * that any channel touches (a pair on (q, q+1) touches q).
 *   mitdvp_batch_set_pair_channel: `ops_reim` holds nops matrices (d0 d1) x (d0 d1), row-major over (i_site, i_site+1)
 *       for rows and columns alike, [k][out][in], interleaved re / im; NULL removes the bond's channel.
 *       MITDVP_CHANNEL_GATE (nops == 1): applied as it is, no rescale: what the truncation removes is lost and reported
 *       by mitdvp_batch_discarded_weight.  MITDVP_CHANNEL_JUMP (2 <= nops <= 16): the selection rule of the one-site
 *       jump channel bit for bit, on w_k = |B_k theta|^2, with the uniform of "site" nsite + site (distinct from every
 *       one-site draw); afterwards C' is rescaled so that the norm after the split equals the norm before the jump.
 *       W == 0 stops that replica only, as for a one-site channel; so does a split that does not converge in 64 sweeps
 *       (MITDVP_ENOTCONV in its status).  MITDVP_EINVAL (message: mitdvp_last_error(NULL), naming the bond and the limit;
 *       nothing changed, every engine untouched) when the bond is out of range, d0 / d1 are not the two sites' physical
 *       dimensions, nops is out of range for the kind, dl d0 or d1 dr exceeds 128, theta and its copy do not fit the
 *       Krylov-basis part of the replica's scratch area, or the replicas run in imaginary time (relax == 1).
 *   mitdvp_batch_pair_jump_counts: counts[n][nsite][16] (long long), row q for the bond (q, q + 1), since the last
 *       mitdvp_batch_set_seed.  One host wait.
 *   mitdvp_batch_discarded_weight: weights[n], per replica the sum over its splits of
 *       sum_{j>r} sigma_j^2 / sum_j sigma_j^2 since the seed or a channel was last set.  One host wait. */
int mitdvp_batch_set_pair_channel(mitdvp_batch* b, int site, int kind, const double* ops_reim, int nops, int d0, int d1);
int mitdvp_batch_pair_jump_counts(mitdvp_batch* b, long long* counts);
int mitdvp_batch_discarded_weight(mitdvp_batch* b, double* weights);
/* Time-dependent one-site fields of a batch: H(t) = H0 + sum_p a_p(t) G_p with G_p Hermitian on site p and a_p real -- a
 * laser pulse E(t) on the dipoles, or dynamic disorder xi_p(t) per trajectory.  In the symmetric splitting of a time step
 * (forward half-sweep dt/2, maps, backward half-sweep dt/2) the term is the one-site unitary exp(-i dt a_p G_p) with a_p at
 * the step's midpoint: ONE more launch per step for the whole batch while at least one field is set (k_batch_field: one
 * workgroup per replica), after the forward half-sweep and before the channels' launch; the step is accurate to O(dt^2).
 * A unitary on the physical index keeps gauge A, so it is applied in place -- no gauge move -- and only the left blocks
 * above the lowest field site are rebuilt.  With no field set nothing changes.
 *   mitdvp_batch_set_field: G = V diag(g) V^+ arrives decomposed: `vecs_reim` is V, d x d, row-major [i][k] with column
 *       k the k-th eigenvector, interleaved re / im; `evals` the d eigenvalues g.  NULL vecs_reim removes the site's
 *       field.  MITDVP_FIELD_TABLE: the amplitude of the n-th time step of the FIELD CLOCK -- the time steps the batch
 *       has completed since the last mitdvp_batch_set_field or mitdvp_batch_set_seed -- is table[n] (per_replica == 0:
 *       ntab doubles shared by all replicas; otherwise [n replicas][ntab], one row each), and 0 from step ntab on; the
 *       caller supplies midpoint values.  MITDVP_FIELD_OU: a stationary Ornstein-Uhlenbeck process per (trajectory, site),
 *       constant over a step: xi_0 = sigma z_0, xi_n = a xi_{n-1} + sigma sqrt(1 - a^2) z_n with a = exp(-|dt| / tau)
 *       (tau == 0: a = 0, white noise; tau in the unit of dt) and z = sqrt(-2 log1p(-u1)) cos(2 pi u2), u1 / u2 the
 *       uniforms of mitdvp_batch_set_seed for "site" 2 nsite + 2 p and 2 nsite + 2 p + 1 (distinct from every jump draw)
 *       at the batch's step counter: a trajectory's noise depends on seed, id, site and the sequence of dt only.  ANY
 *       call resets the field clock and the noise of all sites.  MITDVP_EINVAL (message: mitdvp_last_error(NULL), naming
 *       the site and the limit; nothing changed, every engine untouched) when the site is out of range, d is not the
 *       site's physical dimension or above 64, the kind is unknown, ntab < 1 or table is NULL for a table field, sigma or
 *       tau is negative or not finite, or the replicas run in imaginary time (relax != 0).  mitdvp_batch_sweep refuses
 *       while a field is set.
 *   mitdvp_batch_field_values: values[n][nsite], the amplitudes a_p applied in the last time step, 0 where none was.
 *       One host wait. */
#define MITDVP_FIELD_TABLE 1
#define MITDVP_FIELD_OU 2
int mitdvp_batch_set_field(mitdvp_batch* b, int site, int d, const double* vecs_reim, const double* evals, int kind,
                           const double* table, int ntab, int per_replica, double sigma, double tau);
int mitdvp_batch_field_values(mitdvp_batch* b, double* values);
/* Cross overlaps and one-site matrix elements between two states of a batch (k_batch_cross: one workgroup per PAIR, the
 * pair index is the workgroup index, ONE launch forms every requested pair; k_batch_mean averages them on the device,
 * pair after pair in index order).  A state index 0 .. n-1 names replica i as it is now, n + r names the snapshot of
 * replica r.  An entry (bra, ket, site, O) has the value <psi_bra| O_site |psi_ket>; site = -1 is the plain overlap
 * <psi_bra|psi_ket>.  The walk runs over all nsite sites (two different states share no canonical form): the transfer
 * matrix T (index order (bra bond, ket bond)) starts as 1, U = T K with the ket tensor K, the operator acts on the
 * physical index of U at the entry's site, T' = sum conj(Bra) U, and the value is the 1 x 1 T after the last site.  It
 * depends on its two states and its operator only: not on the number of pairs, its place in the list, n or the compute
 * unit.  The replicas are only read; T and U live in a buffer of the batch indexed by pair.  A pair that names a
 * replica that failed in the same call is zeros.
 *   mitdvp_batch_snapshot: ONE launch (k_batch_snapshot) copies every site tensor of every replica into the batch's
 *       snapshot buffer; one host wait.  The centre may be at site 0 or at site nsite-1 (where a batch call leaves it):
 *       overlaps do not depend on the gauge.  Shapes never change in a batch, so a snapshot stays valid until the next.
 *   mitdvp_batch_set_cross: registers npairs entries: bra[], ket[], site[] (npairs each); the entries with site >= 0
 *       take, in list order, the matrices of ops_reim (row-major [out][in], interleaved re / im, one after the other)
 *       whose orders are op_dims[].  npairs = 0 removes the request.  No launch, no wait.  MITDVP_EINVAL when an index is
 *       outside 0 .. 2n-1, a snapshot index is used before any snapshot exists, a site is outside -1 .. nsite-1, an
 *       operator's order is not that site's physical dimension, or there are more than 65536 pairs.
 *   mitdvp_batch_cross: the request on the current state: TWO launches (k_batch_cross, k_batch_mean), one host wait.
 *       weights: npairs doubles or NULL (1 / npairs each); values[npairs][2] and mean[2] may each be NULL.
 *   While a request is set, every record of mitdvp_batch_run / _run_keys and every call of mitdvp_batch_observe /
 *       _observe_keys records the request too: ONE more launch per record and ONE more k_batch_mean launch per call
 *       (mitdvp_batch_run: 2 nsteps + 2 records + 2), no further host wait; `what` may then be 0 with out pointing at a
 *       mitdvp_batch_out of NULLs: the request alone is recorded, by 2 nsteps + records + 1 launches.  With no request set
 *       nothing changes: the same launches, the same bits, the same refusals.
 *   mitdvp_batch_cross_records: what the last such call recorded: values[records][npairs][2], mean[records][2],
 *       counts = {records, npairs}; each may be NULL.  weights NULL: the means under 1 / npairs, formed by that call, no
 *       launch and no wait here; weights given (npairs doubles): ONE k_batch_mean launch over the records, which are
 *       still on the device, and one host wait.  A new request or no recording call yet: records = 0.
 * Every refusal is MITDVP_EINVAL with a message in mitdvp_last_error(NULL) that names the entry point and the limit, and
 * leaves the request, the snapshot, the records and every engine as they were. */
int mitdvp_batch_snapshot(mitdvp_batch* b);
int mitdvp_batch_set_cross(mitdvp_batch* b, int npairs, const int* bra, const int* ket, const int* site, const double* ops_reim,
                           const int* op_dims);
int mitdvp_batch_cross(mitdvp_batch* b, const double* weights, double* values, double* mean);
int mitdvp_batch_cross_records(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[2]);
/* Bond spectra and entanglement entropies of a batch (k_batch_spectra: one workgroup per replica, ONE launch forms every
 * requested bond of every replica; k_batch_mean averages the records on the device, replica after replica in index
 * order).  Bond q, 0 <= q <= nsite-2, lies between sites q and q+1 and has dimension chi_q.  With the centre at site 0
 * and sites 1 .. nsite-1 right-canonical (the state mitdvp_batch_step leaves) the walk runs on work buffers only: X is
 * the centre tensor; for q = 0 .. the highest requested bond, X seen as (dl d) x dr is QR-factorised (Householder, inside
 * the workgroup), the rows of R are made mutually orthogonal by one-sided Jacobi rotations -- their squared norms are the
 * squared Schmidt values sigma^2 of bond q -- and X <- R' B_{q+1} with the rotated R'.  No U and no V is formed; sites
 * right of the last requested bond are not touched; the replicas are only read.  A replica's record holds, for every
 * requested bond in list order, 4 + chi_q doubles: W = sum sigma^2 (the replica's squared norm; summed in descending
 * order), S1 = -sum p ln p with p = sigma^2 / W (the von Neumann entropy, natural logarithm; a term with p <= 0 counts
 * as 0), S2 = -ln sum p^2 (the second Renyi entropy), pmin = the smallest p (how close the bond is to being too narrow),
 * then the chi_q values sigma^2, descending, not normalised.  rec_len is the sum of 4 + chi_q over the requested bonds.  A
 * record depends on its replica only: not on n, its place in the batch or the compute unit.  A replica that failed in
 * the same call is zeros.
 *   mitdvp_batch_set_spectra: registers the strictly ascending list bonds[nbonds]; nbonds = 0 removes the request.  No
 *       launch, no wait.  MITDVP_EINVAL when a bond is outside 0 .. nsite-2, the list is not strictly ascending, or
 *       rec_len exceeds 65536 doubles.
 *   mitdvp_batch_spectra: the request on the current state: TWO launches (k_batch_spectra, k_batch_mean), one host wait.
 *       weights: n doubles or NULL (1 / n each); values[n][rec_len], mean[rec_len]; counts (may be NULL) receives {n,
 *       rec_len}; with values == NULL && mean == NULL the call only returns the counts.  MITDVP_EINVAL without a request
 *       or when a replica's centre is not at site 0.
 *   While a request is set, every record of mitdvp_batch_run / _run_keys and every call of mitdvp_batch_observe /
 *       _observe_keys records the request too: ONE more launch per record and ONE more k_batch_mean launch per call
 *       (weights 1 / n), no further host wait; `what` may then be 0 with out pointing at a mitdvp_batch_out of NULLs: the
 *       request alone is recorded, by 2 nsteps + records + 1 launches.  A cross request that is set as well adds its own
 *       launches.  With no request set nothing changes: the same launches, the same bits, the same refusals.
 *   mitdvp_batch_spectra_records: what the last such call recorded: values[records][n][rec_len], mean[records][rec_len],
 *       counts = {records, n, rec_len}; each may be NULL.  weights NULL: the means under 1 / n, formed by that call, no
 *       launch and no wait here; weights given (n doubles): ONE k_batch_mean launch over the records, which are still on
 *       the device, and one host wait.  A new request or no recording call yet: records = 0.
 * Jacobi sweeps that do not converge within 64 sweeps zero that replica's record; its status and its tensors stay as
 * they are (an observation never changes a replica), and the call returns MITDVP_ENOTCONV with a message in
 * mitdvp_last_error(NULL) naming the replica and the bond.  Every refusal is MITDVP_EINVAL with a message in
 * mitdvp_last_error(NULL) that names the entry point and the limit, and leaves the request, the records and every engine
 * as they were. */
int mitdvp_batch_set_spectra(mitdvp_batch* b, const int* bonds, int nbonds);
int mitdvp_batch_spectra(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[2]);
int mitdvp_batch_spectra_records(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[3]);
/* Sampled configurations of a batch (k_batch_sample: one workgroup per replica, ONE launch draws nshots configurations of
 * every replica; k_batch_mean averages the frequencies on the device, replica after replica in index order).  A
 * configuration is one basis index per site, drawn with probability |<j_0 .. j_{nsite-1}|psi>|^2 / <psi|psi>.  With the
 * centre at site 0 and sites 1 .. nsite-1 right-canonical (the state mitdvp_batch_step leaves) shot t of replica r walks
 * the chain once from left to right, on work buffers only: v = [1]; at site p, w[j][s] = sum_a v[a] C_p[a][j][s] and
 * g_j = sum_s |w[j][s]|^2; the outcome is picked by the rule of the jump channels -- G = sum_j g_j in index order, the
 * smallest j whose running sum exceeds u G, else the last j with g_j > 0 -- then v <- w[j][:] / sqrt(g_j) and
 * prob <- prob g_j / G.  The uniform is counter-based, u = (key >> 11) 2^-53 with
 * key = mix(mix(mix(mix(seed ^ trajectory_id) + step) + site) + shot): mix, trajectory_id and step are those of the jump
 * channels (mitdvp_batch_set_seed; step counts the batch's completed time steps), seed is the request's own.  A shot
 * therefore depends on (state, seed, id, step, shot) only: not on n, the replica's place in the batch, nshots or the
 * compute unit.  G == 0 at a site gives that shot -1 from that site on and prob = 0; a replica that failed in the same
 * call writes -1 everywhere and zeros.  The replicas are only read.  Per replica: configs[nshots][nsite] (int),
 * prob[nshots] (the product of the conditionals), freq[F] with F = sum_p d_p, entry (p, j) = count / nshots of outcome j
 * at site p; mean_freq[F] is the weighted sum of freq over the replicas.
 *   mitdvp_batch_set_samples: registers the request; nshots = 0 removes it.  No launch, no wait.  MITDVP_EINVAL when
 *       nshots is outside 0 .. 65536 or nshots * nsite exceeds 2^22.
 *   mitdvp_batch_samples: the request on the current state: TWO launches (k_batch_sample, k_batch_mean), one host wait.
 *       weights: n doubles or NULL (1 / n each); configs[n][nshots][nsite], prob[n][nshots], freq[n][F], mean_freq[F], each
 *       may be NULL; counts (may be NULL) receives {n, nshots, nsite, F}; with all four NULL the call only returns the
 *       counts.  MITDVP_EINVAL without a request or when a replica's centre is not at site 0.
 *   While a request is set, every record of mitdvp_batch_run / _run_keys and every call of mitdvp_batch_observe /
 *       _observe_keys records the request too: ONE more launch per record and ONE more k_batch_mean launch per call
 *       (weights 1 / n), no further host wait; `what` may then be 0 with out pointing at a mitdvp_batch_out of NULLs: the
 *       request alone is recorded, by 2 nsteps + records + 1 launches.  With no request set nothing changes: the same
 *       launches, the same bits, the same refusals.
 *   mitdvp_batch_samples_records: what the last such call recorded, the arrays of mitdvp_batch_samples with a leading
 *       record axis; counts = {records, n, nshots, nsite, F}; each may be NULL.  weights NULL: the means under 1 / n,
 *       formed by that call, no launch and no wait here; weights given (n doubles): ONE k_batch_mean launch over the
 *       records, which are still on the device, and one host wait.  A new request, other shapes or no recording call
 *       yet: records = 0.
 * Every refusal is MITDVP_EINVAL with a message in mitdvp_last_error(NULL) that names the entry point and the limit, and
 * leaves the request, the records and every engine as they were. */
int mitdvp_batch_set_samples(mitdvp_batch* b, int nshots, unsigned long long seed);
int mitdvp_batch_samples(mitdvp_batch* b, const double* weights, int* configs, double* prob, double* freq, double* mean_freq,
                         size_t counts[4]);
int mitdvp_batch_samples_records(mitdvp_batch* b, const double* weights, int* configs, double* prob, double* freq,
                                 double* mean_freq, size_t counts[5]);
/* Expectation values of MPO observables of a batch (k_batch_expect: one workgroup per (replica, operator) pair, ONE
 * launch walks every listed operator over every replica; k_batch_mean averages the records on the device, replica after
 * replica in index order).  An operator is named by the op_id under which mitdvp_set_mpo_core gave its cores to every
 * replica (and mitdvp_set_shift its scalar term): total dipole, site-energy sums, currents, bath energies, any sum of
 * products over the chain.  With the centre at site 0 and sites 1 .. nsite-1 right-canonical (the state mitdvp_batch_step
 * leaves) the value of (replica r, operator k) is what mitdvp_expect(engine r, k) returns, <psi | O_k | psi> + shift_k
 * <psi | psi>, not normalised, by the same arithmetic: the right blocks of O_k are walked afresh from the right boundary
 * to bond 1 on work buffers of the request, then one H_eff apply at site 0.  op_id 0 is allowed and gives the energy by a
 * fresh walk, whether or not the sweep's right blocks are valid.  The replicas may carry different cores under one
 * op_id, of equal shapes.  A replica's record holds (re, im) of every listed operator in list order.  A value depends
 * on its replica and its operator only: not on n, nops, the operator's place in the list or the compute unit.  A
 * replica that failed in the same call is zeros.  Replicas, operators and status words are only read.
 *   mitdvp_batch_set_expect: registers the list op_ids[nops]; nops = 0 removes the request.  No launch, no wait.
 *       MITDVP_EINVAL when nops is outside 0 .. 64, an op_id is negative or listed twice, a replica has no core of a
 *       listed operator at some site, the core shapes differ between replicas or their physical dimension is not the
 *       site's, an MPO bond exceeds 16, neighbouring cores do not fit, or the outer MPO bonds are not 1.
 *   mitdvp_batch_expect: the request on the current state: TWO launches (k_batch_expect, k_batch_mean), one host wait.
 *       weights: n doubles or NULL (1 / n each); values[n][nops][2], mean[nops][2]; counts (may be NULL) receives {n,
 *       nops}; with values == NULL && mean == NULL the call only returns the counts.  MITDVP_EINVAL without a request,
 *       when the cores the replicas carry now are refused as above, or when a replica's centre is not at site 0 (the
 *       message names the replica).
 *   While a request is set, every record of mitdvp_batch_run / _run_keys and every call of mitdvp_batch_observe /
 *       _observe_keys records the request too: ONE more launch per record and ONE more k_batch_mean launch per call
 *       (weights 1 / n), no further host wait; `what` may then be 0 with out pointing at a mitdvp_batch_out of NULLs: the
 *       request alone is recorded, by 2 nsteps + records + 1 launches.  With no request set nothing changes: the same
 *       launches, the same bits, the same refusals.
 *   mitdvp_batch_expect_records: what the last such call recorded: values[records][n][nops][2], mean[records][nops][2],
 *       counts = {records, n, nops}; each may be NULL.  weights NULL: the means under 1 / n, formed by that call, no
 *       launch and no wait here; weights given (n doubles): ONE k_batch_mean launch over the records, which are still on
 *       the device, and one host wait.  A new request, other shapes of the chain or of the cores, or no recording call
 *       yet: records = 0.
 * Every refusal is MITDVP_EINVAL with a message in mitdvp_last_error(NULL) that names the entry point, the operator, the
 * site and the limit, and leaves the request, the records and every engine as they were. */
int mitdvp_batch_set_expect(mitdvp_batch* b, const int* op_ids, int nops);
int mitdvp_batch_expect(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[2]);
int mitdvp_batch_expect_records(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[3]);
/* MPO matrix elements between two states of a batch (k_batch_cross_mpo: one workgroup per entry, ONE launch forms every
 * entry; k_batch_mean sums the values on the device, entry after entry in index order).  An entry is (bra, ket, op_id):
 * the state indices are those of mitdvp_batch_set_cross (0 .. n-1 a replica, n + r the snapshot of replica r), op_id names
 * an operator that every replica carries at every site (mitdvp_set_mpo_core, its scalar term from mitdvp_set_shift), as for
 * mitdvp_batch_set_expect.  The cores and the scalar term used are those of the ket's owner, replica ket mod n.  The value
 * is <psi_bra | O | psi_ket> + shift <psi_bra | psi_ket>, not normalised.  Two different states share no canonical form, so
 * the walk runs over all nsite sites, left to right: a left block (bra bond, MPO bond, ket bond) starts as [1] and takes
 * the three products of the forward environment update at every site, conj of the bra tensor in the first and the ket
 * tensor in the third; with a non-zero scalar term the same workgroup then walks the plain overlap by the arithmetic of
 * mitdvp_batch_cross and adds shift times it.  A value depends on its two states and its operator only: not on nentries,
 * its place in the list, n or the compute unit.  An entry that names a replica which failed in the same call is zeros.
 * Replicas, snapshots, operators and status words are only read.
 *   mitdvp_batch_set_cross_mpo: registers nentries entries; nentries = 0 removes the request.  No launch, no wait.
 *       MITDVP_EINVAL when an index is outside 0 .. 2n-1, a snapshot is named before any was taken, an op_id is negative,
 *       a replica has no core of a named operator at some site, the core shapes differ between replicas, an MPO bond is
 *       outside 1 .. 16, neighbouring cores do not fit, the outer MPO bonds are not 1, nentries exceeds 65536, or the
 *       request's work buffer (nentries x carve x 16 bytes, carve = 2 max chi m chi + max n ml + max n mr complex numbers,
 *       n = dl d dr) would exceed 2^32 bytes: the message names the figure and the largest nentries that fits.
 *   mitdvp_batch_cross_mpo: the request on the current state: TWO launches (k_batch_cross_mpo, k_batch_mean), one host
 *       wait.  The centre may be at site 0 or at site nsite-1.  weights: nentries doubles or NULL (1 / nentries each);
 *       values[nentries][2], mean[2]; each may be NULL.  MITDVP_EINVAL without a request, or when the cores the replicas
 *       carry now are refused as above.  Cores may be replaced between calls; cores of other shapes drop the records.
 *   While a request is set, every record of mitdvp_batch_run / _run_keys and every call of mitdvp_batch_observe /
 *       _observe_keys records the request too: ONE more launch per record and ONE more k_batch_mean launch per call
 *       (weights 1 / nentries), no further host wait; the cross and expect requests may be set beside it.  With no request
 *       set nothing changes: the same launches, the same bits, the same refusals.
 *   mitdvp_batch_cross_mpo_records: what the last such call recorded: values[records][nentries][2], mean[records][2],
 *       counts = {records, nentries}; each may be NULL.  weights NULL: the means under 1 / nentries, formed by that call,
 *       no launch and no wait here; weights given (nentries doubles): ONE k_batch_mean launch over the records, which are
 *       still on the device, and one host wait.  A new request, other shapes, or no recording call yet: records = 0.
 * Every refusal is MITDVP_EINVAL with a message in mitdvp_last_error(NULL) that names the entry point, the entry, the
 * operator, the site and the limit, and leaves the request, the records, the snapshot and every engine as they were. */
int mitdvp_batch_set_cross_mpo(mitdvp_batch* b, int nentries, const int* bra, const int* ket, const int* op_id);
int mitdvp_batch_cross_mpo(mitdvp_batch* b, const double* weights, double* values, double* mean);
int mitdvp_batch_cross_mpo_records(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[2]);
/* An MPO applied to replicas of a batch (k_batch_operate: one workgroup per selected replica, ONE launch and one host
 * wait for the whole fit of all of them): mitdvp_operate for every selected replica.  phi ~ O|psi> / |O|psi>| is fitted in
 * the bond dimensions of psi by up to maxstep double sweeps of mixed-block applies, O the operator the replica carries under
 * op_id (mitdvp_set_mpo_core; its scalar term, mitdvp_set_shift, goes through the overlap blocks); a replica stops on its
 * own when |1 - |<phi_i|phi_{i-1}>|| < conv_tol, and reaching maxstep unconverged is not an error.  The fit is exact only
 * where O psi fits the bonds.  replicas: nsel distinct replica indices, or NULL for all.  The selected replicas are WRITTEN:
 * on return their tensors are phi, normalised, centre at site 0, gauge Psi B B ..., their blocks invalid.  norms, iters and
 * statuses (each n entries, indexed by replica, each may be NULL) are written for the selected replicas only: the norm of
 * the last apply at site 0, the double sweeps run, and MITDVP_OK or MITDVP_EINVAL.  An apply whose norm is not > 0 (the
 * operator annihilates the state) stops that replica -- norm 0, MITDVP_EINVAL in its status, its message in
 * mitdvp_last_error(its engine), its chain to be set again -- while the others finish; the call then returns MITDVP_EINVAL.
 * Krylov memories, the jump generator's step counter and counters, channels, the snapshot, every request and the records
 * of the last run are untouched; the call is allowed with channels set and in either relax mode.
 * Refused with MITDVP_EINVAL before the GPU is touched, everything left as it was, the message naming the entry point, the
 * replica / operator / site and the limit: maxstep < 1; conv_tol negative or not finite; a replica index out of range or
 * repeated; a selected replica whose centre is not at site 0; an operator that a selected replica does not carry at every
 * site; core shapes that differ between the selected replicas; MPO bonds outside 1 .. 16; outer MPO bonds that are not 1;
 * neighbouring cores that do not fit; a work buffer (selected replicas x carve x 16 bytes) above 2^32 bytes: the message
 * names both figures and the largest number of replicas that fits. */
int mitdvp_batch_operate(mitdvp_batch* b, int op_id, int maxstep, double conv_tol, const int* replicas, int nsel, double* norms,
                         int* iters, int* statuses);
/* Ground states of a batch by improved relaxation (k_batch_relax: one workgroup per replica; at every site the lowest
 * eigenvector of H_eff + shift by Lanczos with the projected tridiagonal problem solved on the device, then the gauge move,
 * the block update and the absorb; no bond step).  Replicas created with relax = 2 take mitdvp_batch_step / _sweep / _run /
 * _run_keys like any others: a half-sweep is one launch, dt_au is ignored, a replica whose local solve does not converge in
 * max_diag_krylov vectors gets MITDVP_ENOTCONV ("Lanczos Diagonalization is not converged in N basis") and stops, the others
 * finish.  mitdvp_batch_relax runs up to maxstep steps (forward + backward half-sweep) of every replica in ONE launch and one
 * host wait; the right blocks are built first where no step has built them.  E_n, a replica's energy after step n, is the
 * lowest Ritz value of its last local solve (site 0; the scalar term included).  With conv_tol > 0 a replica stops on its
 * own once |E_n - E_{n-1}| <= conv_tol, the others go on; conv_tol = 0 runs maxstep steps.  energies [n]: the last E_n;
 * steps [n]: the steps run; history [n][maxstep]: E_1 .. E_n of each replica, NaN behind its stop; statuses [n]; each of
 * the four may be NULL.  Afterwards every engine is an ordinary consistent engine, centre at site 0.  The jump generator's
 * step counter, channels, the snapshot, every request and the records of the last run are untouched.
 * Refused with MITDVP_EINVAL before the GPU is touched, everything left as it was, the message naming the entry point and
 * the limit: maxstep outside 1 .. 2^20; conv_tol negative or not finite; replicas whose relax is not 2; a replica whose
 * centre is not at site 0. */
int mitdvp_batch_relax(mitdvp_batch* b, int maxstep, double conv_tol, double* energies, int* steps, double* history, int* statuses);
/* Thick restarts of the local Lanczos solve of a relax = 2 batch.  A local solve takes at most min(N, max_diag_krylov)
 * <= 64 Krylov vectors at a site of N elements (one lane of a wave per row of the projected matrix).  With max_restarts > 0
 * a solve that has not converged by then keeps its lowest Ritz vector u_0 = sum_j c_j v_j and the next Lanczos vector
 * u_1 = v_m, on which the projected matrix is tridiagonal again (alpha_0 = theta, beta_0 = beta_{m-1} c_{m-1}), and goes on
 * from there: no apply of H_eff and no memory beyond the max_diag_krylov + 1 slots the solve has anyway, so that a small
 * max_diag_krylov (a small scratch area per replica) becomes usable.  The stop rule is unchanged and carries across a
 * restart.  A solve that is not converged after max_restarts restarts gives its replica MITDVP_ENOTCONV ("Lanczos
 * Diagonalization is not converged in N basis after R restarts"); the others finish.  max_restarts = 0, the default, is
 * the solve without restarts: a batch that never calls this launches and computes what it always did, bit for bit.  The
 * setting holds for mitdvp_batch_relax and for mitdvp_batch_step / _sweep / _run / _run_keys alike, until it is set again.
 * The call clears the counters below.  MITDVP_EINVAL before the GPU is touched, the message naming the entry point and the
 * limit: a NULL handle, replicas whose relax is not 2, max_restarts outside 0 .. 4096. */
int mitdvp_batch_set_relax_restarts(mitdvp_batch* b, int max_restarts);
/* The restart counters since the last mitdvp_batch_set_relax_restarts (or the creation of the batch).  total [n]: the
 * restarts replica i has taken; most [n]: the most restarts of any one of its local solves.  Either may be NULL.  One host
 * wait.  (The applies of H_eff of all cycles are counted in the engines' counters as ever.) */
int mitdvp_batch_relax_restarts(mitdvp_batch* b, long long* total, int* most);
/* Excited states of a relax = 2 batch by deflation against stored states (the penalty method).  A batch owns up to 8
 * slots; each holds a copy of every replica's site tensors and one weight per replica.  While the set is not empty,
 * mitdvp_batch_relax and the relax = 2 paths of mitdvp_batch_step / _sweep / _run / _run_keys solve every local problem on
 *   H_eff + shift + sum_k w_k |q_k><q_k|,
 * q_k being the stored state phi_k projected into the replica's current site basis: the same number of launches, one
 * workgroup per replica (k_batch_relax_defl); the overlap blocks that give q_k are built at the start of every launch from
 * the tensors as they stand and carried through the sweep, nothing of them persists between launches.  The stop rule, the
 * restarts, the Krylov memories and the status words are those of mitdvp_batch_relax; E_n, the lowest Ritz value at site
 * 0, is then the energy PLUS sum_k w_k |<phi_k|psi>|^2 (use the energy observable for <psi|H|psi>).  With an empty set
 * the batch launches the kernel it always launched and computes the same bits.
 * The method finds state k only if every w exceeds the gap to it from the stored states below: a weight that is too small
 * lets the solve fall back onto a stored state.  A fresh start must not BE a stored state: that is an exact eigenvector of
 * the penalised operator (eigenvalue E + w) and the Lanczos solve stops on it at once.
 * mitdvp_batch_deflate_push copies the present state of every replica into the next free slot (ONE launch, one host wait).
 * The centre must be at site 0 and the chain canonical around it, the state mitdvp_batch_relax leaves.  weights: n doubles,
 * one per replica, each finite and > 0.  The states are stored as they are: the penalty is w |<phi|psi>|^2, so the caller
 * pushes normalised states (mitdvp_batch_relax leaves them normalised).  Refused with MITDVP_EINVAL before the GPU is
 * touched, everything left as it was, the message naming the entry point and the limit: a NULL handle; replicas whose
 * relax is not 2; a replica whose centre is not at site 0; a ninth push; NULL weights; a weight that is not finite or not
 * > 0 (the message names the replica); a work buffer (replicas x slots x (sum_p dl_p^2 + max_p N_p) x 16 bytes) above 2^32
 * bytes: the message names both figures and the largest number of slots that fits.
 * mitdvp_batch_deflate_clear empties the set; mitdvp_batch_deflate_count reports how many slots are filled.  The set is
 * also dropped when the replicas' shapes change (where the snapshot is dropped); it is independent of the snapshot, of
 * the cross / expect / spectra / samples requests, of channels and of fields.
 * mitdvp_batch_deflate_overlaps: reim [count][n][2] receives <phi_k|psi_r> for every slot k and replica r (ONE launch,
 * one workgroup per (slot, replica), one host wait; an empty set: no launch, nothing written).  The centre may be at site
 * 0 or at site nsite-1.  Neither the replicas nor the slots are written. */
int mitdvp_batch_deflate_push(mitdvp_batch* b, const double* weights);
int mitdvp_batch_deflate_clear(mitdvp_batch* b);
int mitdvp_batch_deflate_count(mitdvp_batch* b, int* count);
int mitdvp_batch_deflate_overlaps(mitdvp_batch* b, double* reim);
/* propagate_along_sweep (_mps_cls.py:798-1014), one direction only. */
int mitdvp_sweep(mitdvp_engine* h, double dt_au, int forward);
/* The same half-sweep in parts: the next `nsites` local updates of the half-sweep in progress (one is started when none
 * is), through the code of mitdvp_sweep, which is this call with nsites = nsite.  *left (may be NULL) receives the
 * sites still to go, 0 when the half-sweep is complete.  While one is in progress only observables, other parts in
 * the same direction and mitdvp_close are allowed; mitdvp_sweep / mitdvp_step refuse. */
int mitdvp_sweep_part(mitdvp_engine* h, double dt_au, int forward, int nsites, int* left);
/* op_sys_sites = None (_mps_cls.py:2311,2371,2417, wavefunction.py:64-65). */
int mitdvp_invalidate_env(mitdvp_engine* h);

/* -- multi-GPU: bond-sharded (tensor-parallel) applies ------------------- */
/* One process per GPU, every rank holds the replicated state and calls the
 * same sequence of entry points.  H_eff / K_eff applies and environment
 * updates are computed for this rank's slice of the bra-side bond index and
 * combined by ONE collective each, issued through `fn` (RCCL via
 * torch.distributed in pytdscf_amd/dist.py; gloo in the tests):
 *   op 0: in-place all-gather  (rank r owns bytes [r*nbytes/N, (r+1)*nbytes/N))
 *   op 1: in-place all-reduce  (sum, float64)
 * `fn` is called with the engine's stream drained and must return after the
 * collective has completed on the device.  The reference's only parallel path
 * is the approximate mpi4py real-space scheme (_mps_parallel.py:106-268); this
 * one is exact (same results as 1 GPU up to summation order). */
typedef int (*mitdvp_collective_fn)(void* user, int op, void* dev_ptr, size_t nbytes);
int mitdvp_set_parallel(mitdvp_engine* h, int nranks, int rank, mitdvp_collective_fn fn, void* user);

/* The same bond-sharded mode with the collectives issued by the library itself: RCCL
 * (librccl, resolved with dlopen on first use) on the engine's own HIP stream, stream-ordered,
 * no host synchronisation per collective.  One rank creates the 128-byte ncclUniqueId with
 * mitdvp_rccl_unique_id and distributes it out of band (torch.distributed, MPI, a file);
 * every rank then calls mitdvp_set_parallel_rccl.  mitdvp_rccl_selftest runs one all-gather and
 * one all-reduce on a small device buffer and returns the number of wrong values. */
int mitdvp_rccl_unique_id(char out[128]);
int mitdvp_set_parallel_rccl(mitdvp_engine* h, int nranks, int rank, const char id[128]);
int mitdvp_rccl_selftest(mitdvp_engine* h, int* mismatches);

/* -- several electronic states (MPS-SM, nstate > 1) -------------------------
 * The reference keeps one MPS per electronic state (superblock_states[istate][isite],
 * _mps_cls.py:84-118; the SURVEY's istate / ibra / iket arguments) and one MPO block plus one
 * scalar per (bra, ket) state pair (TensorHamiltonian.mpo[i][j], .coupleJ[i][j],
 * hamiltonian_cls.py:618-752).  The local solves act on all states' centre tensors stacked into
 * one Krylov vector (SplitStack, _contraction.py:479-608; multiplyH_MPS_direct_MPO.dot, :1182-1243),
 * environment blocks are kept per state pair (renormalize_op_psite, _mps_mpo.py:421-696) and the
 * gauge move is one QR per state (_mps_cls.py:1798-1850).  mitdvp_ms_configure switches a handle
 * to this mode; states share the physical dimensions, bond dimensions may differ per state;
 * every MPO block spans all sites (4-leg cores).  mitdvp_krylov_stats and mitdvp_counters apply
 * unchanged.  Not available in this mode: adaptive bonds, gates, Kraus maps (single-state only in
 * the reference too).  mitdvp_set_parallel* shards this mode like the single-state one. */
int mitdvp_ms_configure(mitdvp_engine* h, int nstate);
int mitdvp_ms_set_site(mitdvp_engine* h, int istate, int isite, const double* reim, int l, int n, int r, int gauge);
int mitdvp_ms_get_site_shape(mitdvp_engine* h, int istate, int isite, int* l, int* n, int* r, int* gauge);
int mitdvp_ms_get_site(mitdvp_engine* h, int istate, int isite, double* out);
/* right-to-left QR of one state, site 0 scaled to `scale` = sqrt(weight of the state) >= 0
 * (alloc_superblock_random, _mps_cls.py:2684-2699; _mps_mpo.py:88-94) */
int mitdvp_ms_canonicalize(mitdvp_engine* h, int istate, double scale);
int mitdvp_ms_set_mpo_core(mitdvp_engine* h, int op_id, int ibra, int iket, int isite, const double* reim, int ml, int d_out,
                           int d_in, int mr);
int mitdvp_ms_set_coupleJ(mitdvp_engine* h, int op_id, int ibra, int iket, double re, double im);
int mitdvp_ms_step(mitdvp_engine* h, double dt_au);                   /* MPSCoef.propagate, _mps_cls.py:452-503 */
int mitdvp_ms_expect(mitdvp_engine* h, int op_id, double out[2]);     /* sum over state pairs, _mps_cls.py:540-612 */
int mitdvp_ms_autocorr(mitdvp_engine* h, double out[2]);              /* sum over states, wavefunction.py:226-257 */
/* Simulator.operate with several states (apply_dipole_along_sweep, _mps_cls.py:718-796): every state must
 * be fed by at least one block or scalar term (the reference fails otherwise, _contraction.py:555) */
int mitdvp_ms_operate(mitdvp_engine* h, int op_id, int maxstep, double conv_tol, double* norm_out, int* iters_out);
int mitdvp_ms_pops(mitdvp_engine* h, double* out /* [nstate] */);      /* pop_states, _mps_cls.py:682-703 */

/* -- one block of a site-range sharded chain ----------------------------------
 * Real-space parallel one-site TDVP (MPSCoefParallel.propagate, _mps_parallel.py:106-268): every rank owns a
 * contiguous range of sites as an engine whose outer bonds are wider than 1.  The environment blocks at its
 * two ends come from the neighbours (send_op_block / recv_op_block, :1610-1635), and a half-sweep is driven
 * through the pieces of propagate_along_sweep (_mps_cls.py:798-1014) so that the end site can be left to the
 * joint update of two ranks (skip_end_site, :876-877; propagate_joint_two_sites, _mps_parallel.py:270-470).
 * Host side: pytdscf_amd/parallel_sites.py.
 *   side 0: block left of site 0, L[a][c][b] (d, m, d); side 1: block right of the last site, R[r][t][s]. */
int mitdvp_set_boundary_env(mitdvp_engine* h, int side, const double* reim, int d, int m);
/* new values for a site tensor of unchanged shape; the environment cache is kept (mitdvp_set_site drops it) */
int mitdvp_replace_site(mitdvp_engine* h, int isite, const double* reim, int gauge);
/* environment block left (side 0) / right (side 1) of bond `bond` (the bond left of site `bond`); reim_out may be
 * NULL to query the shape (d, m, d) */
int mitdvp_get_env(mitdvp_engine* h, int side, int bond, double* reim_out, int* d, int* m);
/* construct_op_sites (_mps_cls.py:1738-1796): all blocks on one side of the centre (0: left, 1: right) */
int mitdvp_build_envs(mitdvp_engine* h, int side);
int mitdvp_site_exp(mitdvp_engine* h, double dt_au);      /* exp_superH_propagation_direct, _mps_cls.py:1016-1100 */
/* ONE H_eff apply at the centre site, sigma = H_eff x (multiplyH_MPS_direct_MPO.dot, _contraction.py:1182-1243), issued
 * exactly as the local exponential issues its applies: identity blocks of the environments short-circuited when the
 * numerical check finds them (the reference's eye shortcut, _mps_mpo.py:510-523), zero blocks of the MPO core skipped.
 * reim_in NULL: x = the centre tensor.  *flags (may be NULL): bit 0 first stage trimmed, bit 1 third stage trimmed,
 * bit 2 block-sparse W stage, bit 3 the one-launch small-bond kernel, bit 4 the two-product form of an edge-structured
 * core (reducing epilogue, no intermediates; then bits 0-2 are clear); with bit 4, bit 5 (0x20) = its R side and bit 6
 * (0x40) = its L side ran the folded variant (the reduced core contracted into the environment block once per local
 * solve, the side one plain GEMM; MITDVP_FOLD_APPLY=0 never, 1 wherever valid); bit 7 (0x80) / bit 8 (0x100) = that folded
 * R / L side ran as seven half-size products (one Strassen level; MITDVP_FOLD_STRASSEN=0 never, 1 wherever its sizes are
 * even); bit 9 (0x200) / bit 10 (0x400), set together with 0x80 / 0x100 = each of those seven ran as seven quarter-size
 * products (two levels, 49 products in one launch; MITDVP_FOLD_STRASSEN=2 wherever the side's sizes are divisible by 4, else
 * as 1).  For parity tests of the kernels a sweep runs. */
int mitdvp_heff_apply_center(mitdvp_engine* h, const double* reim_in, double* reim_out, int* flags);
/* trans_next_psite_AsigmaB (:1798-1850): centre -> A sigma (forward) or sigma B; the block through the site is built,
 * sigma stays in the engine as the pending bond matrix */
int mitdvp_split_center(mitdvp_engine* h, int forward);
int mitdvp_bond_exp(mitdvp_engine* h, double dt_au);      /* exp_superK_propagation_direct, :1102-1170 */
int mitdvp_absorb_bond(mitdvp_engine* h, int forward);    /* trans_next_psite_APsiB, :1172-1206 */
int mitdvp_get_bond(mitdvp_engine* h, double* reim_out, int* dim);   /* the pending bond matrix (joint_sigvec) */
int mitdvp_set_bond(mitdvp_engine* h, int bond, const double* reim, int dim);
/* Where the tensor arguments of mitdvp_set_site / replace_site / set_boundary_env / set_bond / fold_block (sources) and
 * mitdvp_get_site / get_env / get_bond / fold_block (destinations) live: MITDVP_POINTER_HOST (default) or
 * MITDVP_POINTER_DEVICE = device memory on the handle's GPU (the halo messages of the site-sharded sweep go from
 * engine to RCCL and back without touching the host: the reference pickles NumPy arrays through mpi4py,
 * _mps_parallel.py:541-807).  Device operands are copied by a kernel on the handle's stream, so they may have been
 * allocated by another HIP runtime instance of the process (torch's); every call returns after the copy completed. */
#define MITDVP_POINTER_HOST 0
#define MITDVP_POINTER_DEVICE 1
int mitdvp_set_pointer_mode(mitdvp_engine* h, int mode);
/* Observables of a site-sharded state without gathering it (MPSCoefParallel.ovlp, _mps_parallel.py:855-983;
 * expectation, :1210-1302): a boundary block is carried through ALL sites of this engine.  from_left: reim_in sits
 * left of site 0, reim_out right of the last site (shape from the last site / MPO core); else the other way round.
 * op_id >= 0: environment block (d, m, d) of that operator, bra conjugated; op_id < 0: transfer block (d, 1, d),
 * conj_bra = 0 gives <Psi*|Psi> (the autocorrelation of the t/2 trick). */
int mitdvp_fold_block(mitdvp_engine* h, int op_id, int conj_bra, int from_left, const double* reim_in, int d, int m,
                      double* reim_out);
/* the same through the sites [first, first + count) only (count = 0: the block is copied) */
int mitdvp_fold_block_range(mitdvp_engine* h, int op_id, int conj_bra, int from_left, int first, int count, const double* reim_in,
                            int d, int m, double* reim_out);
/* Reduced density of ONE site of a site-sharded state (MPSCoefParallel.get_reduced_densities, _mps_parallel.py:1035-1208):
 * rho[j][j'] from the site tensor and the transfer blocks of everything left / right of it, left[bra][ket] (D_l x D_l),
 * right[bra][ket] (D_r x D_r) as mitdvp_fold_block (op_id < 0, conj_bra = 1) produces them.  reim_out: d x d, host. */
int mitdvp_site_rdm_blocks(mitdvp_engine* h, int isite, const double* left, const double* right, double* reim_out);

/* -- one RANK of the site-range sharded sweep, driven natively -------------------------------------
 * MPSCoefParallel.propagate (_mps_parallel.py:106-268) as ONE call per time step: the block's two half-sweeps, the
 * joint update of the two sites facing each other across a rank boundary (propagate_joint_two_sites, :270-470:
 * psi_L X^+ psi_R -> A X' B through the pseudo-inverse of the joint matrix, multiply_sigvec_pinv _site_cls.py:709-754)
 * and the neighbour messages around it -- the reference's mpi4py send / recv pairs send_Psi_to_left (:698-707),
 * send_op_sys_to_left (:761-807), send_B_to_right (:728-740), send_joint_sigvec_to_right (:541-597),
 * send_op_sys_to_right (:612-628) -- as grouped ncclSend / ncclRecv of device buffers between chain neighbours on the
 * block engine's stream (RCCL over xGMI, librccl resolved with dlopen).  A shard owns two engines: its block
 * (nsite_block sites, outer bonds wider than 1) and, except on the last rank, the two-site engine of the junction to
 * its right; mitdvp_shard_engine hands them out (borrowed: never mitdvp_destroy them) so that set-up -- MPO cores,
 * site tensors, boundary blocks, mitdvp_build_envs -- uses the entry points above.  State between steps as in the
 * reference's diagram (:115-122): even ranks [Psi B .. B], odd ranks [A .. A Psi], every block's junction-side end
 * site carrying the weight of the joint matrix X (held by the LEFT rank of each junction: joint_sigvec_not_pinv). */
typedef struct mitdvp_shard mitdvp_shard;
/* dr_next: right bond dimension of the first site of rank + 1 (ignored on the last rank) */
int mitdvp_shard_create(const mitdvp_config* cfg, int rank, int world, int nsite_block, int dr_next, mitdvp_shard** out);
void mitdvp_shard_destroy(mitdvp_shard* h);
const char* mitdvp_shard_last_error(const mitdvp_shard* h); /* h may be NULL */
int mitdvp_shard_engine(mitdvp_shard* h, int which /* 0 block, 1 junction engine, 2 left junction engine (pair mode) */, mitdvp_engine** out);
/* the reference's treatment of small singular values at a junction: regularize != 0 lifts singular values below
 * SQRT_EPSRHO = 1e-4 to s + eps exp(-s / eps) -- in the (D_l D_r x d) unfolding of the left junction site before its
 * QR (SiteCoef.gauge_trf(regularize=True), _site_cls.py:207-246) and in the new joint matrix; p_svd >= 0 replaces
 * the new joint matrix by truncate_sigvec(p = p_svd, keepdim = True) (:586-690: SVD, cumulative-weight cut, zeros on
 * the cut values, A <- A U, B <- Vh B, blocks rebuilt).  The reference runs with both (regularize = 1, p_svd =
 * const.p_svd, default 1e-7; _mps_parallel.py:369, :437-444); defaults here: 0, -1 (off). */
int mitdvp_shard_set_options(mitdvp_shard* h, int regularize, double p_svd);
/* Pair mode (call on EVERY rank before the first step, after the transport is attached): both ranks of a junction run
 * its update on identical copies of the two facing sites, bond-sharded over the pair -- every apply and environment
 * update of the two-site engine contracts half of the bra-side bond index on each GPU (the engine's exact tensor
 * parallelism), combined by two-rank all-gathers / all-reduces over the same point-to-point transport -- instead of
 * the right rank waiting while the left one works (in the reference the partner of propagate_joint_two_sites sits in
 * comm.recv, _mps_parallel.py:196-203).  A rank > 0 gets a second two-site engine for the junction to its LEFT
 * (mitdvp_shard_engine(h, 2, ...): give it the MPO cores of sites (first - 1, first)); dl_prev = left bond dimension of
 * the left neighbour's last site (ignored on rank 0).  Same results as the default mode to rounding. */
int mitdvp_shard_enable_pair(mitdvp_shard* h, int dl_prev);
int mitdvp_shard_set_joint(mitdvp_shard* h, const double* reim, int dim);       /* host, (dim, dim) */
int mitdvp_shard_get_joint(mitdvp_shard* h, double* reim_out, int* dim);        /* reim_out may be NULL */
/* Transport.  Production: every rank calls mitdvp_shard_attach_rccl with the 128-byte id one rank got from
 * mitdvp_rccl_unique_id (distributed out of band), one rank per GPU.  Ranks SHARING a GPU (one-GPU test boxes; RCCL
 * refuses two ranks on one device) install a callback instead: op 0 sends / op 1 receives nbytes of host memory
 * to / from rank `peer`, blocking, 0 on success; the shard stages the device buffers through it. */
typedef int (*mitdvp_p2p_fn)(void* user, int op, int peer, void* host_buf, size_t nbytes);
int mitdvp_shard_set_transport(mitdvp_shard* h, mitdvp_p2p_fn fn, void* user);
int mitdvp_shard_attach_rccl(mitdvp_shard* h, const char id[128]);
/* neighbour ping over every junction, both directions (collective over the ranks); number of wrong values */
int mitdvp_shard_selftest(mitdvp_shard* h, int* mismatches);
/* one grouped ncclSend + ncclRecv of `elems` complex numbers from this rank to itself (needs attach_rccl) */
int mitdvp_shard_self_sendrecv(mitdvp_shard* h, size_t elems, int* mismatches);
int mitdvp_shard_step(mitdvp_shard* h, double dt_au);                            /* MPSCoefParallel.propagate */
/* the pieces of a step (tests, other schedules): propagate_along_sweep over the block with skip_end_site (:147-175),
 * and the joint updates of the junctions whose LEFT rank has parity `parity` (0: (3)->(4), 1: (2)->(1) of :115-122) */
int mitdvp_shard_sweep(mitdvp_shard* h, double dt_au, int forward, int skip_end);
int mitdvp_shard_junctions(mitdvp_shard* h, double dt_au, int parity);
int mitdvp_shard_traffic(mitdvp_shard* h, double* bytes, long* messages);        /* halo traffic sent so far */
/* host wall time this rank has spent in its block half-sweeps / in (and waiting for) the junction updates, over `steps`
 * mitdvp_shard_step calls: the load balance of the site-sharded sweep */
int mitdvp_shard_phase_times(mitdvp_shard* h, double* block_ms, double* junction_ms, long* steps);
/* Panel factorisation of the QR gauge move (SiteCoef.gauge_trf, _site_cls.py:138-292 = LAPACK zgeqrf + zungqr):
 * 1 (default) = CholeskyQR2 of each 32-column panel + reconstruction of LAPACK's Householder vectors / T / tau / signs
 * of diag(R) from the orthonormal panel, falling back to 0 = one Householder step per launch (unconditionally stable)
 * when a conditioning check on the device fails.  Process-wide, like mitdvp_set_gemm_mode. */
int mitdvp_set_qr_fast(int on);
int mitdvp_get_qr_fast(void);
/* device time (HIP events) of one m x n factorisation with Q and R formed, random full-rank input */
int mitdvp_bench_qr(int device, int m, int n, int reps, double* ms_out, long* launches);
/* The thin factorisation as the SWEEP issues it (csrc/qr.h qr_thin): gauge_free != 0 = the sign convention of LAPACK's
 * diag(R) is not asked for (SiteCoef.gauge_trf's Q R = psi and Q^H Q = 1 are all a gauge move needs, _site_cls.py:264-282;
 * SURVEY appendix B item 6) -> block Gram-Schmidt over Cholesky factors of 128-column blocks, R with a positive diagonal;
 * falls back to the Householder panels when a conditioning check on the device fails.  a: m x n row-major complex128 on
 * the host, or NULL = a random full-rank matrix generated on the device (timing); q_out (m x n), r_out (n x n) may be
 * NULL.  *ms_out = device time per factorisation over `reps`, *launches per factorisation, *path_out = 1 when the
 * gauge-free path delivered the result, 0 when the Householder panels did. */
int mitdvp_qr_thin(int device, const double* a, int m, int n, int gauge_free, double* q_out, double* r_out, int reps,
                   double* ms_out, long* launches, int* path_out);
/* warm-up memory of the local solves at a site (_Debug.niter_krylov[isite], _integrator.py:178-186) */
int mitdvp_get_krylov_memory(mitdvp_engine* h, int isite, int* k);
int mitdvp_set_krylov_memory(mitdvp_engine* h, int isite, int k);
/* the one-launch small-bond kernels need all their workgroups resident: switch them off (0) for engines that share
 * their GPU with other processes; default on (or MITDVP_SMALL_KERNELS) */
int mitdvp_set_small_kernels(mitdvp_engine* h, int on);

/* -- observables -------------------------------------------------------- */
int mitdvp_expect(mitdvp_engine* h, int op_id, double out[2]);       /* _mps_cls.py:540-612 */
int mitdvp_autocorr(mitdvp_engine* h, double out[2]);                /* wavefunction.py:226-257, conj=False */
/* Autocorrelation without the t/2 trick (Simulator(t2_trick=False): Properties._get_autocorr,
 * properties.py:222-232, wf_zero._ints_wf_ovlp_mpo): keep a device copy of the current state, later
 * return <copy|current state> (bra conjugated). */
int mitdvp_save_reference(mitdvp_engine* h);
int mitdvp_overlap_reference(mitdvp_engine* h, double out[2]);
int mitdvp_norm(mitdvp_engine* h, double* out);                      /* _mps_cls.py:706-716 */
int mitdvp_site_rdm(mitdvp_engine* h, int isite, double* reim_out);  /* _mps_cls.py:1208-1436, key (isite,isite) */
/* General reduced density, MPSCoef.get_reduced_densities / _get_pure_reduced_density
 * (_mps_cls.py:1208-1283, :1628-1678): remain_nleg[isite] in {0,1,2} legs kept per site
 * (2 = ket and bra, 1 = diagonal).  Two calls: with out == NULL the number of complex
 * elements is returned in *n_out; then with a buffer of that size.  Axes: kept sites
 * ascending, (ket, bra) per 2-leg site. */
int mitdvp_reduced_density(mitdvp_engine* h, const int* remain_nleg, int nlen, double* reim_out, size_t* n_out);
/* SVD truncation of the bond right of the centre ("Psi") site, truncate_sigvec
 * (_site_cls.py:586-690): keep the leading singular values whose cumulative weight
 * sum s_k / sum s reaches 1 - p (at most max_dim if max_dim > 0); the kept values,
 * normalised to unit 2-norm, are written to svals_out (may be NULL) and their number
 * to *new_dim.  The engine's one-sided Jacobi SVD kernel does the decomposition. */
int mitdvp_truncate_bond(mitdvp_engine* h, double p, int max_dim, int* new_dim, double* svals_out);
/* One-site gates, Model(one_gate_to_apply=TensorHamiltonian of single-site operators):
 *   mitdvp_set_gate    : register U[d_out][d_in] (d x d, row-major, interleaved re/im) for a
 *                        site; NULL removes it.  While gates are registered mitdvp_step applies
 *                        them between its two half-sweeps with the last site as
 *                        re-orthogonalisation centre (MPSCoef.propagate, _mps_cls.py:489-490).
 *   mitdvp_apply_gates : MPSCoef.apply_one_gate (_mps_cls.py:2314-2373, :2420-2451) now, with
 *                        the current centre site as reorth_center (WFunc.apply_one_gate,
 *                        wavefunction.py:588-598, uses the resting centre 0): U on the physical
 *                        leg, canonicalizeB / canonicalizeA over the touched span (:3539-3598),
 *                        environment blocks that saw a touched site dropped (op_sys_sites = None). */
int mitdvp_set_gate(mitdvp_engine* h, int isite, const double* U_reim, int d);
int mitdvp_apply_gates(mitdvp_engine* h);
/* Kraus maps on purified states, Model(kraus_op={(site,): B} or {(site, site+1): B}) with
 * B (k, d, d) = the Kraus operators B_q[x][d'] (kraus.py:17-123):
 *   mitdvp_set_kraus   : register B for `isite` (NULL removes it).  two_site = 0: the site's
 *                        physical index is (system d, ancilla K), K = dim / d
 *                        (_kraus_contract_single_site_np, kraus.py:146-228); two_site = 1: system
 *                        site `isite` (dimension d) and ancilla site `isite + 1`
 *                        (_kraus_contract_two_site_np, :281-358; the bond between them is
 *                        re-split by the engine's Jacobi SVD).  mitdvp_step applies the maps after
 *                        the gates, between its half-sweeps (MPSCoef.propagate, _mps_cls.py:491-492).
 *   mitdvp_apply_kraus : MPSCoef.apply_kraus (_mps_cls.py:2375-2418) now, re-orthogonalising
 *                        towards the current centre site. */
int mitdvp_set_kraus(mitdvp_engine* h, int isite, int two_site, const double* B_reim, int k, int d);
int mitdvp_apply_kraus(mitdvp_engine* h);
/* Simulator.operate (simulator_cls.py:286-331, :356-360): variational application of operator
 * op_id to the state, WFunc.apply_dipole (wavefunction.py:303-351) -> MPSCoef.apply_dipole
 * (_mps_cls.py:421-450, :718-796, :2733-2778): at most maxstep double sweeps in which every site
 * tensor is replaced by the mixed-environment apply (bra = new state, ket = initial state),
 * stopped when |1 - |<phi_i|phi_{i-1}>|| < conv_tol (1e-8 in the reference).  On return the
 * engine holds phi ~ O|psi> / ||O|psi>|| (site-0 centred); *norm_out is the norm of the last
 * apply (the value Simulator.operate returns), *iters_out the number of double sweeps done. */
int mitdvp_operate(mitdvp_engine* h, int op_id, int maxstep, double conv_tol, double* norm_out, int* iters_out);
/* Adaptive bond dimension (a1TDVP), Simulator.propagate(adaptive=True, adaptive_Dmax,
 * adaptive_dD, adaptive_p_proj) -> const.adaptive / Dmax / dD / p_proj
 * (_const_cls.py:120-124, :212-216).  While enabled, every half-sweep widens the
 * neighbour tensors by up to dD orthogonal-complement vectors (get_superblock_full,
 * _mps_cls.py:3699-3755), picks each bond's new rank from the projection-error
 * functional (get_rank_and_projection_error, :1985-2105; stop when the relative
 * increment falls below p_proj, never above Dmax) and propagates the zero-padded
 * centre tensor (propagate_along_sweep, :863-987).  Real-time propagation only. */
int mitdvp_set_adaptive(mitdvp_engine* h, int enable, int dmax, int dd, double p_proj);
/* SiteCoef.thin_to_full (_site_cls.py:294-405) on caller data: gauge 0 = "A": site
 * (l, c, r) isometric over (l c) x r -> out (l, c, r + extra); gauge 1 = "B": isometric
 * over l x (c r) -> out (l + extra, c, r).  The added vectors are the leading ones of
 * the orthogonal complement in LAPACK's full-mode QR of the isometry. */
int mitdvp_thin_to_full(int device, int gauge, const double* site, int l, int c, int r, int extra, double* out);
/* kernel-level hook: A (r x c) = U diag(S) Vh with the engine's Jacobi SVD */
int mitdvp_svd(int device, const double* A, int r, int c, double* U, double* S, double* Vh, int* sweeps);

/* Liouville space (Model(space="liouville")): the MPS is a vectorised density matrix with
 * site dimension n*n, physical index = row*n + col (_mps_mpo.py:135-194).
 *   mitdvp_set_trace_op_core : core O[a][out][in][f] (M_l, n, n, M_r) of a full-chain
 *                              observable acting on the n-dimensional Hilbert-space legs
 *   mitdvp_expect_trace      : Tr(O rho), _exp_liouville (_mps_cls.py:3769-3838)
 *   mitdvp_partial_trace     : get_partial_trace (_mps_cls.py:1438-1510); size query with
 *                              out == NULL like mitdvp_reduced_density; the right-most kept
 *                              site always keeps both legs */
int mitdvp_set_trace_op_core(mitdvp_engine* h, int op_id, int isite, const double* reim, int ml, int n, int mr);
int mitdvp_expect_trace(mitdvp_engine* h, int op_id, double out[2]);
int mitdvp_partial_trace(mitdvp_engine* h, const int* remain_nleg, int nlen, double* reim_out, size_t* n_out);
/* Subspace projection of a Liouville-space site (Model(subspace_inds={site: P_inds}), model_cls.py:110-118,
 * MPSCoefMPO.project_subspace / define_reshape_mat, _mps_mpo.py:135-220): the site's physical leg holds the entries
 * inds[0..ninds) of the n*n vectorised density matrix.  The caller hands over MPO cores and site tensors with the
 * shorter leg (TensorHamiltonian.project_subspace, hamiltonian_cls.py:852-880); this call tells the trace
 * observables how to embed the leg back into n x n.  Call it BEFORE mitdvp_set_trace_op_core for that site
 * (those cores are gathered on arrival); ninds = 0 removes the projection. */
int mitdvp_set_subspace(mitdvp_engine* h, int isite, int n, const int* inds, int ninds);
/* MPSCoef.hermitise (_mps_cls.py:2289-2312, svd_conj_mpdo :2516-2562): rho <- (rho + rho^dagger) / 2 of a
 * Liouville-space chain as a direct sum, re-truncated bond by bond to the old bond dimensions by two-site SVDs,
 * left in the site-0-centred canonical form with its normalisation untouched. */
int mitdvp_hermitise(mitdvp_engine* h);
int mitdvp_krylov_stats(mitdvp_engine* h, int* per_site);            /* _Debug.niter_krylov, _helper.py:29 */

/* -- counters: _ElpTime / _NFlops equivalents (_helper.py:33-101) ------- */
typedef struct {
  double heff_flops;     /* algorithmic flops in H_eff applies (SURVEY 8d F_H)  */
  double heff_ms;        /* HIP-event time of those applies (profiling on)      */
  double env_flops, env_ms;
  double keff_flops, keff_ms;
  double qr_flops, qr_ms;
  double krylov_vec_ms;  /* Krylov vector kernels                               */
  long long n_heff, n_keff, n_env, n_qr;
  long long n_exp_site, n_exp_bond;
  long long n_launch;    /* kernel launches issued                              */
  double heff_stage_ms[3]; /* L.psi, W., .R stages of the H_eff applies (profiling on) */
  double n_collectives;    /* collectives issued (bond-sharded mode)                   */
  double collective_bytes; /* sum of the collective buffer sizes                       */
  double heff_flops_skipped; /* part of heff_flops NOT executed: zero blocks of W skipped by the block-sparse W stage */
  double n_host_waits;     /* device->host records the host waited for inside local exponentials (multi-launch regime) */
  double n_heff_edge;      /* H_eff applies that took the two-product "edge" form (the others ran the three-stage chain or the one-launch kernel) */
  double heff_stage_flops[3]; /* 8-flop-per-complex-MAC count of what the three stages EXECUTE (trimmed identity blocks,
                                 skipped zero blocks and tile padding of the W stage accounted; the 3M product's 6 / 8 is
                                 applied by the reader): with heff_stage_ms the roofline of each stage's kernel */
  double n_env_fold;       /* environment updates that took the structured form (Gram matrix of the site tensor + folded
                              operator of the general MPO-bond states) instead of the M-fold chain */
  double n_env_reuse;      /* those of them that took the general states' operator from the Strassen factors the local
                              solve had packed, instead of building it again and applying it as one plain product */
} mitdvp_counters;
int mitdvp_counters_get(mitdvp_engine* h, mitdvp_counters* out);
int mitdvp_counters_reset(mitdvp_engine* h);
int mitdvp_set_profiling(mitdvp_engine* h, int on); /* HIP-event timing per phase */

/* -- fine seam for unit-level parity tests (SURVEY 8b "internal seam 1"):
 *    one H_eff / K_eff apply and one environment update on caller data.
 *    contract_with_site_mpo (_contraction.py:148-397),
 *    multiplyH_MPS_direct_MPO._op_lcr_dot (:1038-1173),
 *    multiplyK_MPS_direct_MPO._op_lr_dot (:1297-1352). */
int mitdvp_heff_apply(int device, const double* L, const double* W, const double* R, const double* psi,
                      int dl, int d, int dr, int ml, int mr, double* sigma_out, int reps, double* ms_out);
int mitdvp_keff_apply(int device, const double* L, const double* R, const double* sval,
                      int dl, int dr, int m, double* out);
int mitdvp_env_update(int device, int left, const double* env, const double* site, const double* W,
                      int dl, int d, int dr, int ml, int mr, double* out);
/* -- the one-launch small-bond kernel (k_small_site) under a chosen launch plan.
 *    kind and dims name one of its three contraction chains:
 *      MITDVP_SMALL_HEFF  dims = (dl, d, dr, ml, mr)
 *      MITDVP_SMALL_KEFF  dims = (d1, d2, m)
 *      MITDVP_SMALL_ENV   dims = (din, min, d, dout, mout): block (din, min, din) -> (dout, mout, dout)
 *    mitdvp_small_plan: the plan an engine with n_cu compute units gives that chain, APPLY (exp_mode 0) or EXP mode
 *    (the engine plans environment updates in APPLY mode only).  Host arithmetic, no device call.  ok = 0: the chain does
 *    not qualify for the family there (the other fields are then 0).  grid = ceil(slabs / spw) * nsc workgroups,
 *    lds_bytes what the plan carves (the launch asks for at least 84 KiB), sg_aliases_x: the chunk partial reuses X's LDS. */
enum { MITDVP_SMALL_HEFF = 0, MITDVP_SMALL_KEFF = 1, MITDVP_SMALL_ENV = 2 };
typedef struct {
  int ok, nsc, cs, spw, a_resident, grid, lds_bytes, sg_aliases_x;
} mitdvp_small_plan_t;
int mitdvp_small_plan(int kind, const int* dims, int exp_mode, int n_cu, mitdvp_small_plan_t* out);
/*    mitdvp_small_apply: one H_eff / K_eff apply or environment update through Engine::heff_apply / keff_apply /
 *    env_update (the production dispatch) on an engine confined to the compute units [0, cu_count) -- 0: the whole
 *    device, else a multiple of 8 -- with a complex shift (out += shift * v; H_eff and K_eff only).
 *      HEFF  a = L (dl, ml, dl), w = W (ml, d, d, mr), r = R (dr, mr, dr), v = psi (dl, d, dr), out (dl, d, dr)
 *      KEFF  a = L (d1, m, d1), r = R (d2, m, d2), v = sigma (d1, d2), out (d1, d2); w unused
 *      ENV   dims = (dl, d, dr, ml, mr) of the SITE and its core, as mitdvp_env_update: v = site (dl, d, dr), w = W;
 *            left != 0: a = env (dl, ml, dl) -> out (dr, mr, dr); left == 0: a = env (dr, mr, dr) -> out (dl, ml, dl)
 *            through the mirrored tensor; r unused.  The plan's dims are (dl, ml, d, dr, mr) / (dr, mr, d, dl, ml).
 *    info: n_launch = launches the call issued (1: the one-launch family served it; plan is then the plan it ran,
 *    as launched), plan.ok = 0 otherwise. */
typedef struct {
  int n_launch;
  mitdvp_small_plan_t plan;
} mitdvp_small_info;
int mitdvp_small_apply(int device, int cu_count, int kind, int left, const int* dims, const double* a, const double* w,
                       const double* r, const double* v, double shift_re, double shift_im, double* out,
                       mitdvp_small_info* info);
/* SiteCoef.gauge_trf (_site_cls.py:138-292): key 0 "Psi2Asigma", 1 "Psi2sigmaB". */
int mitdvp_gauge_trf(int device, int key, const double* psi, int dl, int d, int dr,
                     double* site_out, double* sigma_out);
/* short_iterative_lanczos / _arnoldi on a dense operator (_integrator.py:287-655). */
int mitdvp_expm_dense(int device, int integrator, int conserve_norm, int lanczos_variant,
                      const double* mat, int n, const double* x, double scale_re, double scale_im,
                      double thresh, int k_prev, double* y_out, int* k_out);
/* The same, and the counters of the engine that ran it (n_launch: the launches of the Krylov loop, the operator's
 * own GEMM not counted; n_host_waits): which vector-step kernels the solve took is read off them. */
int mitdvp_expm_dense_counted(int device, int integrator, int conserve_norm, int lanczos_variant,
                              const double* mat, int n, const double* x, double scale_re, double scale_im,
                              double thresh, int k_prev, double* y_out, int* k_out,
                              mitdvp_counters* counters_out);

/* -- kernel-level test / bench hooks (no reference counterpart) --------- */
/* C = alpha*op(A)*op(B) + beta*C on the MFMA zgemm kernel, row-major. */
int mitdvp_zgemm(int device, int transA, int conjA, int transB, int conjB, int m, int n, int k,
                 const double* A, const double* B, double* C, const double alpha[2], const double beta[2],
                 int tile_cfg, int reps, double* ms_out);
/* The same kernel through its whole descriptor (ZgemmDesc), one call, no timing:
 *   C[b] = alpha * op(A[b]) * op(B[b]) + beta * C[b],  b < batch, row-major, operand b at off + b * stride elements
 * of its buffer.  A, B, C are WHOLE buffers of nA, nB, nC complex elements: all three are copied to the device, the
 * product runs once, and all of C comes back (so that what lies around the view can be checked too).
 *   arow_skip (0 = off, else >= 2; A untransposed): logical row r of A is stored at row r + r / (arow_skip - 1) + 1;
 *   rowmap_p > 0: row r of C is stored at ((r + r0) % p) * s1 + ((r + r0) / p) * s2 instead of r * ldc;
 *   klist (NULL = dense; NN operands, K % 16 == 0, tile_cfg 1): for each 64-row tile tm, klist[tm * klist_stride] =
 *   number of 16-wide K tiles to visit, then their ascending indices; klist_stride >= 1 + K / 16; the other tiles of A
 *   count as zero.
 * Before any HIP call the footprint of the descriptor is computed on the host -- first and last element the operation
 * may touch in A, B (dense views, the arow_skip map included), C (ldc or the row map) and the list (ntm rows of
 * klist_stride) -- and MITDVP_EINVAL is returned if any index falls outside nA / nB / nC / nklist, or if the kernel
 * does not serve the combination (batch > 65535, arow_skip 1 or with transA or a list, a list with a transpose or
 * K % 16 != 0, tile_cfg outside -1..2).  m, n or batch of 0: success, C unchanged.  k = 0: C = beta * C. */
typedef struct mitdvp_zgemm_args {
  int m, n, k, batch;
  int transA, conjA, transB, conjB;
  long lda, ldb, ldc;             /* leading dimensions, complex elements */
  long strideA, strideB, strideC; /* batch strides (0 = shared operand) */
  long offA, offB, offC;          /* first operand element inside its buffer */
  double alpha[2], beta[2];
  int tile_cfg, mode3m;           /* -1 = library default */
  int arow_skip;
  int rowmap_p;
  long rowmap_s1, rowmap_s2;
  int rowmap_r0;
  int klist_stride;
} mitdvp_zgemm_args;
int mitdvp_zgemm_desc(int device, const mitdvp_zgemm_args* a, const double* A, size_t nA, const double* B, size_t nB,
                      double* C, size_t nC, const int* klist, size_t nklist);
/* The same kernel with its REDUCING epilogue (the call each side of the edge form of an H_eff apply makes), one call:
 *   C[offC + u*su + v*sv + i*si] (+)= sum_{x < xm, y < yn} W[offW + i*ldw + x*yn + y] * T[u*xm + x][v*yn + y],  i < di,
 *   T = A * op(B)  (m x n, never stored),  u < m / xm,  v < n / yn;  acc = 1 adds to C, acc = 0 overwrites it.
 * A (m x k, rows lda apart), B (transB = 0: k x n, 1: n x k; rows ldb apart), W and C are WHOLE buffers of nA, nB, nW,
 * nC complex elements: all are copied to the device, the product runs once, all of C comes back.  The fragment-ordered
 * copy of the core is built as the engine builds it whenever the shape runs the unguarded epilogue.
 *   epi_b4 / epi_full: -1 = as the library decides, 0 = the 4 x 4 x 4 form / its unguarded variant off for this call
 *   (1 is refused: a form cannot be forced on);  the timing bits of MITDVP_ZGEMM_TUNE are not honoured.
 *   variant_out (may be NULL): the epilogue body the call ran, 1..13 (numbering: csrc/zgemm_reduce_args_check.h).
 * Before any HIP call MITDVP_EINVAL is returned if the last element of A, B, W ((di-1)*ldw + xm*yn - 1) or C
 * ((m/xm-1)*su + (n/yn-1)*sv + (di-1)*si) falls outside its buffer, a stride or offset is negative, m % xm or n % yn is
 * non-zero, k < 1, the kernel does not serve (xm, yn, di), or epi_b4 / epi_full is 1.  m or n of 0: success, C unchanged. */
typedef struct mitdvp_zgemm_reduce_args {
  int m, n, k;                 /* m = nu * xm, n = nv * yn */
  int transB;                  /* 0: NN (the L side's form), 1: NT (the R side's) */
  long lda, ldb, offA, offB;
  int xm, yn, di, acc;
  long ldw, offW;              /* w[i * ldw + x * yn + y] */
  long su, sv, si, offC;
  int mode3m;                  /* -1 library default, 0 = 4M, 1 = 3M */
  int epi_b4, epi_full;        /* -1 = as the library decides; 0 = off */
} mitdvp_zgemm_reduce_args;
int mitdvp_zgemm_reduce(int device, const mitdvp_zgemm_reduce_args* a, const double* A, size_t nA, const double* B, size_t nB,
                        const double* W, size_t nW, double* C, size_t nC, int* variant_out);
/* One building block of the batched-trajectory kernels (csrc/batch_site.hip) in ONE workgroup, as those kernels call it:
 * the workgroup product behind the absorb, the H_eff / K_eff applies, the environment update and the overlap walk, the
 * in-workgroup Householder thin QR, and the Jacobi split of a two-site tensor.  Workgroup b of a grid of ncopies takes its
 * own copy of the operands and writes its own copy of the results (a result may not depend on the grid).
 *   op / variant / dims (all tensors row-major, complex128 as (re, im)):
 *   MATMUL   (M, N, K)                 out0 = in0 (M x K) in1 (K x N); variant 0: into a buffer of its own, 1: in place of
 *                                      in0 (N = K), 2: in place of in1 (M = K)
 *   HEFF     (dl, d, dr, ml, mr)       out0[a,i,r] = sum in0[a,c,b] W[c,i,j,t] in2[r,t,s] scl in3[b,j,s]; in1 = W as
 *                                      [(i,t)][(c,j)]
 *   KEFF     (dim, m)                  out0[a,r] = sum in0[a,c,b] scl in3[b,s] in2[r,c,s]
 *   ENV      (din, min, d, dout, mout) out0[a,q,r] = sum conj(bra)(b,i,a) in0[b,p,s] W[p,i,j,q] ket(s,j,r), in2 = bra,
 *                                      in3 = ket; variant 0: tensors stored (in, phys, out), in1 = W as [(q,j)][(i,p)];
 *                                      variant 1: tensors stored (out, phys, in), the mirror image a backward sweep reads
 *                                      (W[p,i,j,q] is then core[q,i,j,p] of the MPO core); variant 2: as 0 through the
 *                                      forward-only instance.  (in1 of HEFF / ENV 0, 2 / ENV 1 is the packing w2l / w2el /
 *                                      w2er of a core (ml, d, d, mr): csrc/engine.h)
 *   OVERLAP  (L, d, b_1 .. b_(L-1))    out0[0] = <bra | ket>, in0 / in1 = the L <= 6 site tensors of ket / bra one after
 *                                      the other, site p of shape (b_p, d, b_(p+1)), b_0 = b_L = 1
 *   QR       (m, n), m >= n            variant 0: in0 = A (m x n), out0 = Q (m x n), out1 = R (n x n); variant 1: in0 =
 *                                      A^T (n x m), out0 = Q^T, out1 = R^T; no sign convention on diag(R)
 *   SPLIT    (m, n, r)                 in0 = theta (m x n); out0 = B (r x n, orthonormal rows), out1 = C' = theta B^H
 *                                      (m x r)
 *   info, doubles, per copy: [0] the block's return code (0 = ok, 1 = not converged within the 64 Jacobi sweeps); SPLIT also [1] the kept
 *   weight, [2] the discarded fraction, [3 .. 3 + m) the squared row norms (sigma^2) in descending order.
 * n0 .. n3, nout0, nout1 count complex elements, ninfo doubles; the results hold ncopies copies one after the other.
 * Before any HIP call MITDVP_EINVAL is returned for an unknown op or variant, a dimension below 1, a shape outside the
 * kernels' own envelope (more than 8192 elements in a tensor, a bond above 64, an MPO bond above 16, QR with m < n, SPLIT
 * with m or n above 128 or r above min(m, n, 64)), a buffer shorter than the operation's footprint
 * (csrc/batch_block_check.h) or ncopies outside 1 .. 16. */
#define MITDVP_BLOCK_MATMUL 0
#define MITDVP_BLOCK_HEFF 1
#define MITDVP_BLOCK_KEFF 2
#define MITDVP_BLOCK_ENV 3
#define MITDVP_BLOCK_OVERLAP 4
#define MITDVP_BLOCK_QR 5
#define MITDVP_BLOCK_SPLIT 6
typedef struct mitdvp_batch_block_args {
  int op, variant;
  int dims[8];
  int ncopies;
  double scl; /* HEFF, KEFF: the factor on the vector */
} mitdvp_batch_block_args;
/* Test hook: the projected eigen-solve of k_batch_relax alone (the same device function, one workgroup of one wave per
 * case): the lowest eigenpair of ncases real symmetric tridiagonal matrices.  Case q has order k[q] in 1 .. 64, diagonal
 * alpha[64 q .. 64 q + k) and off-diagonal beta[64 q .. 64 q + k - 1); the rest of a row is not read.  theta[q]: the lowest
 * eigenvalue; vec[64 q ..): its unit eigenvector, first component non-negative, zeros behind k.  MITDVP_EINVAL before the
 * GPU is touched for ncases outside 1 .. 65536, a NULL pointer, or a k outside 1 .. 64 (the message names the case). */
int mitdvp_batch_trilow(int device, const double* alpha, const double* beta, const int* k, int ncases, double* theta, double* vec);
int mitdvp_batch_block(int device, const mitdvp_batch_block_args* a, const double* in0, size_t n0, const double* in1, size_t n1,
                       const double* in2, size_t n2, const double* in3, size_t n3, double* out0, size_t nout0, double* out1,
                       size_t nout1, double* info, size_t ninfo);
/* One call of ONE host wrapper of csrc/vecops.h -- the Krylov vector algebra, the leg shuffles, the block lists of the
 * K_eff apply, the norm profiles and the identity tests -- on a stream of its own, exactly as the engine calls it (the
 * wrapper's grid choice included).  All tensors row-major, complex128 as (re, im).  Buffers: z0 z1 z2 complex inputs, r0 a
 * real input, idx an int array, mask 64 bits; zo0 zo1 complex and ro real RESULTS, which are in-out: the caller's contents
 * go to the device first and the whole buffer comes back, so what lies between the written elements must be as it was.
 * P = 256 partial sums (NPART); "v & 1": bit 0 of variant.
 *   op                   dims; strides          buffers and what is computed
 *   DOT                  n                      zo0[P] = partials of sum conj(z0) z1 (variant 1) or sum z0 z1 (variant 0)
 *   SUMSQ                n                      ro[P] = partials of sum |z0|^2
 *   LANCZOS_UPDATE       n                      zo0 = v -= alpha z0 (+ beta z1 if v & 1); alpha = sum z2[P], beta =
 *                                               sqrt(sum r0[P]); ro[P] = partials of |v|^2
 *   LANCZOS_UPDATE_DEF   n, l                   zo0 = H u_l -> u_(l+1), z0 = u_l, z1 = u_(l-1) (if v & 1), z2[P] = partials
 *                                               of the raw dot, r0[l][P] = nrm_all, orthodox = v & 2, eps; ro[P]
 *   LANCZOS_STEP_SMALL   n <= 16384             zo0 = w, z0 = vl, z1 = x (if v & 2; else x is vl itself), z2 = vm2 and r0[P]
 *                                               = betaprev (if v & 1), eps; zo1[P] = alpha, ro[P] = |w|^2, each [0] = value
 *   SCALE_INV_NORM       n                      zo0 /= sqrt(sum r0[P]) unless that is below eps
 *   MULTI_DOT            n, k; ldv              zo0[k][P] = partials of <z0_j | z1>, z0 = V (k rows, ldv apart)
 *   ARNOLDI_UPDATE       n, k; ldv              zo0 = v -= sum_j h_j V_j, z0 = V, z1[k][P] = partials of h; ro[P]
 *   LINCOMB              n, k; ldv              zo0 = sum_j coef_j V_j (if v & 1), ro[P] = partials of its norm (if v & 2)
 *   AXPBY                n                      zo0 = a z0 + b zo0
 *   SCALE                n                      zo0 *= a
 *   TRANSPOSE            rows, cols, batch;     zo0_b[c][r] = z0_b[r][c]; batches in_bs / out_bs apart, apart or interleaved
 *                        ldi, ldo, in_bs, out_bs
 *   TRANSPOSE_REV3       na, nj, ns             zo0[s][j][a] = z0[a][j][s]
 *   PERMUTE_0213         n0, n1, n2, n3         zo0[i0][i2][i1][i3] = z0[i0][i1][i2][i3]
 *   PERMUTE5             d0 .. d4; s0 .. s4     zo0 (C order) = z0 gathered with the strides; v & 1: idx = map2 replaces i2
 *   PHYS_DIAG            dl, n, dr              zo0[b][c][e] = z0[b][c n + c][e]; variant 1: the trace over c
 *   COPY2D               rows, cols, zero_to;   zo0[r][c] = a z0[r][c] (+ zo0[r][c] if v & 1), columns cols .. zero_to - 1
 *                        ldd, lds               zeroed
 *   COPY_RAW             n                      zo0 = z0
 *   IDENTITY             rows, cols; ld         zo0 = the rows x cols identity
 *   SCALE_COLS           rows, cols; ld         zo0[r][c] *= r0[c]
 *   GATHER_BLOCKS        rows, cols, nbl,       zo0[a][k][:] = z0[a][idx[k]][:], k < nbl <= 64
 *                        n_dst, m_src
 *   FILL_SCALED_BLOCKS   rows, cols, nbl, pos0; zo0[a][pos0 + k][:] = f[k] z0[a][:]
 *                        ldx
 *   ACCUM_SCALED_BLOCKS  rows, cols, nbl; ldx   zo0[a][:] += sum_k f[k] z0[a][idx[k]][:] + both z1[a][:]
 *   COL_SUMSQ            rows, cols             ro[c] = sum_r |z0[r][c]|^2
 *   ROW_SUMSQ            rows, cols             ro[r] = sum_c |z0[r][c]|^2
 *   SHELL_SUMSQ          n                      ro[t] = sum over max(i, j) = t of |z0[i][j]|^2
 *   IDENT_DEV            n; ld                  ro[0] = max |z0 - 1|, 1e308 if an element is not finite
 *   IDENT_DEV_MULTI      n, nblk; ld, blk_stride  ro[c] = max |block c - lam 1|, zo1[c] = lam, blocks of mask only;
 *                                               variant 1 = clear, variant 0 = the maximum with what ro held
 * Left out: fold_env_core, gram_env_core, gram_mirror_lower and strassen_* (tested with their own files), kry_diff (needs
 * the device Krylov state), vec_randn, the clock and CU probes.
 * Before any HIP call MITDVP_EINVAL is returned for an unknown op or variant, a negative dimension or stride, a buffer
 * shorter than the footprint (csrc/vecop_check.h), a source that overlaps a result, k > 21, n > 16384 for the one-workgroup
 * step, batch > 65535 for the transposes, more than 64 blocks, or more than 128 MB in all.  A zero-size call returns
 * MITDVP_OK with the results untouched (k = 0 is zero-size for MULTI_DOT only: ARNOLDI_UPDATE still writes v and its norm,
 * LINCOMB zeros).  After any other error code the contents of the results are undefined. */
#define MITDVP_VECOP_DOT 0
#define MITDVP_VECOP_SUMSQ 1
#define MITDVP_VECOP_LANCZOS_UPDATE 2
#define MITDVP_VECOP_LANCZOS_UPDATE_DEF 3
#define MITDVP_VECOP_LANCZOS_STEP_SMALL 4
#define MITDVP_VECOP_SCALE_INV_NORM 5
#define MITDVP_VECOP_MULTI_DOT 6
#define MITDVP_VECOP_ARNOLDI_UPDATE 7
#define MITDVP_VECOP_LINCOMB 8
#define MITDVP_VECOP_AXPBY 9
#define MITDVP_VECOP_SCALE 10
#define MITDVP_VECOP_TRANSPOSE 11
#define MITDVP_VECOP_TRANSPOSE_REV3 12
#define MITDVP_VECOP_PERMUTE_0213 13
#define MITDVP_VECOP_PERMUTE5 14
#define MITDVP_VECOP_PHYS_DIAG 15
#define MITDVP_VECOP_COPY2D 16
#define MITDVP_VECOP_COPY_RAW 17
#define MITDVP_VECOP_IDENTITY 18
#define MITDVP_VECOP_SCALE_COLS 19
#define MITDVP_VECOP_GATHER_BLOCKS 20
#define MITDVP_VECOP_FILL_SCALED_BLOCKS 21
#define MITDVP_VECOP_ACCUM_SCALED_BLOCKS 22
#define MITDVP_VECOP_COL_SUMSQ 23
#define MITDVP_VECOP_ROW_SUMSQ 24
#define MITDVP_VECOP_SHELL_SUMSQ 25
#define MITDVP_VECOP_IDENT_DEV 26
#define MITDVP_VECOP_IDENT_DEV_MULTI 27
typedef struct mitdvp_vecop_args {
  int op, variant;
  long dims[5];
  long strides[5];
  double a[2], b[2], both[2], eps; /* complex scalars as (re, im) */
  double coef[42];                 /* LINCOMB: 21 complex coefficients */
  double f[128];                   /* block lists: 64 complex factors */
} mitdvp_vecop_args;
int mitdvp_vecop(int device, const mitdvp_vecop_args* a, const double* z0, size_t nz0, const double* z1, size_t nz1,
                 const double* z2, size_t nz2, const double* r0, size_t nr0, const int* idx, size_t nidx,
                 unsigned long long mask, double* zo0, size_t nzo0, double* zo1, size_t nzo1, double* ro, size_t nro);
/* Complex-product form of the MFMA zgemm kernel for everything that follows:
 * 0 = "4M" (textbook, 4 real MFMA products), 1 = "3M" (Karatsuba, 3 products,
 * normwise stable); the library default is 1 unless MITDVP_ZGEMM=4m is set. */
int mitdvp_set_gemm_mode(int mode3m);
int mitdvp_get_gemm_mode(void);
/* Device-resident timing of the three-stage H_eff apply at a given shape
 * with random operands (bench roofline leg).  Returns avg ms per apply. */
int mitdvp_bench_heff(int device, int dl, int d, int dr, int ml, int mr, int reps, int warmup, double* ms_out);
/* Size-independent self checks of the H_eff apply on device-resident random
 * operands at a given (possibly full BASELINE) shape, without host copies:
 *   out[0] = ||H_3m(x) - H_4m(x)|| / ||H_4m(x)||        (two complex-product forms agree)
 *   out[1] = ||H(x + 2i y) - H(x) - 2i H(y)|| / ||H(x + 2i y)||   (linearity)
 *   out[2] = ||H(x)||, out[3] = ms of the last apply */
int mitdvp_heff_selfcheck(int device, int dl, int d, int dr, int ml, int mr, double out[4]);
/* raw v_mfma_f64_16x16x4_f64 issue-rate probe: returns TFLOP/s */
int mitdvp_mfma_peak_probe(int device, double* tflops_out);
/* dumps the C/D lane map of v_mfma_f64_16x16x4_f64: out[64*4*2] = (row, col) */
/* shader-clock probe: out[0] = shader cycles, out[1] = 100 MHz reference ticks spent by a
 * single-wavefront dependent-FMA loop of `iters` iterations (clock in MHz = 100 * out[0] / out[1]). */
int mitdvp_clock_probe(int device, long iters, double* cycles_ticks_out);
/* Where the workgroups of a launch on a stream created with a CU mask run (hipExtStreamCreateWithCUMask; mask NULL: an
 * ordinary stream): out[b] = XCC id (bits 3:0) | CU / shader-array / shader-engine id (bits 15:8) of workgroup b.  Every
 * workgroup holds lds_bytes of LDS for spin_us microseconds.  Used to find the mask bits of one XCD (ensemble mode). */
int mitdvp_cu_mask_probe(int device, const unsigned* mask, int nwords, int nblocks, size_t lds_bytes, int spin_us, int* out);
int mitdvp_mfma_layout_probe(int device, int* out);

#ifdef __cplusplus
}
#endif
#endif /* MITDVP_H */
