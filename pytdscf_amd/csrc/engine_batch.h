// engine_batch.h -- batched trajectories (engine_batch.hip): B borrowed engines stepped by one launch per half-sweep.
// One-site and nearest-neighbour gates and quantum-jump channels set on the batch act between the two half-sweeps of a
// time step: one more launch.  Time-dependent one-site fields (pulse tables, Ornstein-Uhlenbeck noise) act in the same
// slot, before the channels: one more launch of their own (k_batch_field).
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "batch_records.h"
#include "batch_site.h"
#include "engine.h"

namespace mitdvp {

// An owning device array of the batch: move-only, freed in the destructor.  reserve grows only, does not preserve the
// contents and allocates at least one element, so an array that was reserved is never null; fits says whether reserve
// would leave the array where it is.  Whoever lets one grow waits first for the work queued on it (Batch::reserve_synced).
template <class T>
struct DevArr {
  T* p = nullptr;
  size_t n = 0;  // elements asked for

  DevArr() = default;
  DevArr(DevArr&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevArr& operator=(DevArr&& o) noexcept {
    std::swap(p, o.p);
    std::swap(n, o.n);
    return *this;
  }
  ~DevArr() { if (p) (void)hipFree(p); }

  bool fits(size_t need) const { return p && need <= n; }
  void reserve(size_t need) {
    if (fits(need)) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    HIP_CHECK(hipMalloc((void**)&p, std::max<size_t>(need, 1) * sizeof(T)));
    n = need;
  }
  operator T*() const { return p; }
};

// The records of ONE request of the batch (cross, spectra, samples, expect, cross_mpo) and their means, laid out by
// BatchRecords (batch_records.h): rec holds the nrec records [rows][len] of the last run() and, behind them, the slot of
// the call on the current state, which therefore overwrites none of them; mean holds the run's means, the slot's mean and
// the records' means under weights given later.  h_rec / h_mean mirror what the last run() copied back, h_now the slot
// and its mean.  The stream and the launch counter are the batch's, and so is every host wait.
struct RecordStore {
  DevArr<double> rec, mean, w;
  std::vector<double> h_rec, h_mean, h_w, h_now;
  size_t rows = 0, len = 0;  // as last reserved
  long nrec = 0;             // the records of the last run() that rec and h_rec hold
  BatchRecords lay() const { return BatchRecords{rows, len, (size_t)nrec}; }

  void drop() { nrec = 0; }  // the records are another request's, or of other shapes
  // Room for l.nrec records and the slot behind them.  While records are held they must stay where they are, since
  // X_records still reads them on the device: X() reserves for the run's own count, which fits; run() drops them first.
  // A reserve for another count, other rows or len, or one that would move them throws std::logic_error and changes
  // nothing.  reserve also takes rows and len from l, so it is called whether or not everything fits.
  bool fits(const BatchRecords& l) const { return rec.fits(l.rec_elems()) && mean.fits(l.mean_elems()) && w.fits(l.rows); }
  void reserve(const BatchRecords& l);
  double* slot(long q) const { return rec.p + lay().rec_slot((size_t)q); }  // where the request's kernel writes record q
  void weights(hipStream_t st, const double* weights);                      // rows doubles, null: 1 / rows each
  // the end of a run of nrec records: ONE k_batch_mean over all of them (the weights are set first), then the copies back
  void mean_of_run(hipStream_t st, long nrec, long long& n_launch);
  void fetch_run(hipStream_t st);
  // the call on the current state, once the request's kernel wrote slot(nrec): ONE k_batch_mean over the slot, the
  // copies back and, after the host wait, the hand-out (null: not wanted)
  void mean_of_slot(hipStream_t st, long long& n_launch);
  void fetch_slot(hipStream_t st, bool values = true, bool mean = true);
  void slot_out(double* values, double* mean) const;
  // X_records: values from the mirror; mean from the mirror (weights null; false: nothing was queued) or by ONE
  // k_batch_mean under the given weights into the third region of the mean buffer, copied straight to mean (true: the
  // caller waits once)
  bool records(hipStream_t st, const double* weights, double* values, double* mean, long long& n_launch);
};

constexpr int BATCH_RELAX_MAX_STEPS = 1 << 20;   // full steps of one relax() call
constexpr int BATCH_TRILOW_MAX_CASES = 65536;    // cases of one batch_trilow call
// test hook: the lowest eigenpair of ncases tridiagonal matrices by the eigen-solve of k_batch_relax (bt_trilow), one
// workgroup per case.  Host pointers; alpha / beta / vec [ncases][64], k / theta [ncases].  ArgError before the GPU is
// touched for ncases outside 1 .. BATCH_TRILOW_MAX_CASES, a null argument, or a k outside 1 .. 64.
void batch_trilow(int device, const double* alpha, const double* beta, const int* k, int ncases, double* theta, double* vec);

class Batch {
 public:
  // validates (ArgError otherwise, every engine untouched): one device, distinct engines, no CU mask, single electronic
  // state, not adaptive, not a segment, not bond-sharded, no gates / Kraus maps, identical site and MPO shapes
  // and identical integrator settings across the replicas, shapes inside the envelope of batch_plan; with relax == 2
  // (improved relaxation) also max_diag_krylov in 2 .. 64 and equal across the replicas
  explicit Batch(const std::vector<Engine*>& engines);
  ~Batch();
  Batch(const Batch&) = delete;
  Batch& operator=(const Batch&) = delete;

  void step(double dt, int nsteps, int* statuses);        // statuses[i]: SS_OK / SS_ENOTCONV / SS_EZERO of replica i
  void sweep(double dt, bool forward, int* statuses);  // refused while a channel or a field is set

  // One-site channels applied between the two half-sweeps of every time step (k_batch_channel, one more launch per step
  // while at least one is set).  kind: BCH_GATE (nops == 1) or BCH_JUMP (2 <= nops <= BATCH_MAX_JUMP); ops_reim: nops
  // matrices d x d, row-major, interleaved re / im; null removes the site's channel.  ArgError (nothing changed) when the
  // site is out of range, d is not the site's physical dimension, nops is out of range or the replicas run in imaginary time.
  void set_channel(int site, int kind, const double* ops_reim, int nops, int d);
  // seed and trajectory ids (null: 0 .. B-1) of the jump generator; resets the step counter and the jump counters
  void set_seed(unsigned long long seed, const unsigned long long* ids);
  void jump_counts(long long* counts);  // [B][L][BATCH_MAX_JUMP], zeros where no jump channel acted
  bool has_channels() const { return chan_lo_ >= 0; }
  // Pair channels on the bond (site, site + 1), in the same walk (k_batch_pair takes the place of k_batch_channel while
  // at least one is set: still one more launch per step).  ops_reim: nops matrices (d0 d1) x (d0 d1), row-major over
  // (i_site, i_site+1), interleaved re / im; null removes the bond's channel.  ArgError naming the bond and the limit
  // (nothing changed) when the bond is out of range, d0 / d1 are not the two physical dimensions, nops is out of range,
  // the two-site tensor is outside batch_pair_fits, or the replicas run in imaginary time.
  void set_pair_channel(int site, int kind, const double* ops_reim, int nops, int d0, int d1);
  void pair_jump_counts(long long* counts);  // [B][L][BATCH_MAX_JUMP], row q: bond (q, q + 1)
  // [B]: sum over the splits since the seed or a channel was last set of the weight each split discarded
  void discarded_weight(double* out);
  bool has_pairs() const { return npair_ > 0; }

  // Time-dependent one-site fields H(t) = H0 + sum_p a_p(t) G_p, applied between the forward half-sweep and the channels
  // of every time step (k_batch_field, one more launch per step while at least one is set).  G = V diag(g) V^+ arrives
  // decomposed: vecs_reim is V, d x d, row-major [i][k] with column k the k-th eigenvector, interleaved re / im; evals its
  // d eigenvalues; null vecs_reim removes the site's field.  kind BFLD_TABLE: the amplitude of the n-th time step of the
  // field clock is table[n] (per_replica 0: ntab doubles for all replicas; 1: [B][ntab]), 0 past the end; the caller
  // supplies midpoint values.  kind BFLD_OU: a stationary Ornstein-Uhlenbeck process per (trajectory, site) of standard
  // deviation sigma and correlation time tau (the unit of dt; 0: white noise), piecewise constant over a step.  The field
  // clock counts the time steps completed since the last set_field or set_seed call; ANY call of set_field resets it and
  // the noise state of all sites.  ArgError naming the site and the limit (nothing changed) when the site is out of
  // range, d is not the site's physical dimension or above BATCH_FIELD_MAX_D, the kind is unknown, ntab < 1 or the table
  // is null for a table field, sigma or tau is negative or not finite, or the replicas run in imaginary time.
  void set_field(int site, int d, const double* vecs_reim, const double* evals, int kind, const double* table, int ntab,
                 int per_replica, double sigma, double tau);
  void field_values(double* out);  // [B][L]: the amplitudes applied in the last time step, 0 where none was applied
  bool has_fields() const { return fld_lo_ >= 0; }

  // Host destinations of the observables, every one may be null; nrec records on the leading axis (mitdvp_batch_out).
  struct ObsOut {
    double *norm = nullptr, *autocorr = nullptr, *energy = nullptr, *rdm = nullptr;  // [nrec][B], [nrec][B][2], .., [nrec][B][nrdm][2]
    double *mean_norm2 = nullptr, *mean_autocorr = nullptr, *mean_energy = nullptr, *mean_rdm = nullptr;
  };
  // validates the request (ArgError otherwise, every engine untouched): what non-empty (it may be empty when density keys
  // are asked: with_keys), the RDM bit and the site list go together, sites in range and strictly ascending; returns
  // sum d_p^2 over the listed sites
  long observe_sizes(const int* sites, int nsites, int what, bool with_keys = false);
  // Multi-site reduced densities (k_batch_density): nkeys rows of L leg counts (2: ket and bra, 1: diagonal, 0: traced
  // out), as Engine::reduced_density takes one.  density_sizes validates the keys against the envelope of
  // batch_density_plan (ArgError naming the key and the limit otherwise, every engine untouched) and returns the complex
  // elements of all keys of one replica together; nrdm: what observe_sizes returned for the same request.
  struct DensOut {
    const int* legs = nullptr;  // [nkeys][L]
    int nkeys = 0;
    double *density = nullptr, *mean_density = nullptr;  // [nrec][B][ndens][2], [nrec][ndens][2]; each may be null
  };
  long density_sizes(const int* legs, int nkeys, long nrdm);
  // records the state before step 0 and after every `every`-th of nsteps steps (nsteps = 0: one observation of the
  // current state): one k_batch_observe launch per record, ONE k_batch_mean launch for all of them, records on the device
  // until the end, one host wait.  weights: B doubles or null (1 / B).  With density keys (dens.nkeys > 0) one
  // k_batch_density launch per record follows k_batch_observe on the same stream, and k_batch_observe is skipped when
  // `what` is empty; the keys' values lie behind the site RDMs in the record and are averaged by the same k_batch_mean.
  void run(double dt, int nsteps, int every, const int* sites, int nsites, int what, const double* weights, const ObsOut& out,
           int* statuses, const DensOut& dens);
  void run(double dt, int nsteps, int every, const int* sites, int nsites, int what, const double* weights, const ObsOut& out,
           int* statuses) {
    run(dt, nsteps, every, sites, nsites, what, weights, out, statuses, DensOut());
  }

  // ---- the five requests: cross, spectra, samples, expect, cross_mpo ----
  // What they share, X standing for the request and a row being what a weight multiplies (a pair or an entry for cross and
  // cross_mpo, a replica for the others):
  // set_X registers the request, an empty one removes it; either way the records of the request before are dropped.  No
  // launch, no wait.
  // X() is the request on the current state: the request's kernel and k_batch_mean, TWO launches, one host wait.  weights:
  // one double per row or null (1 / rows each); every output may be null.
  // While a request is set every record of run() records it too: ONE more launch per record (the request's kernel behind
  // the record's other launches) and ONE more k_batch_mean launch per call (weights 1 / rows); values and means are copied
  // with the rest, no further host wait.  X_records returns what the last run() recorded: the arrays of X() with a leading
  // record axis, each may be null, and counts with the number of records in front.  weights null: the means of the run,
  // no launch and no wait; weights given: ONE k_batch_mean launch over the records, which are still on the device, and
  // one host wait.  X() after a run leaves the run's records and means as they are, and so does X_records.
  // Every refusal is an ArgError that names the entry point and the limit and leaves the request, the records, the
  // snapshot and every engine as they were.

  // ---- cross overlaps and one-site matrix elements between replicas (k_batch_cross, k_batch_snapshot) ----
  // A state index 0 .. B-1 names replica i, B + r the snapshot of replica r.
  // snapshot: ONE launch copies every site tensor of every replica into the batch's snapshot buffer; one host wait.  The
  // centre may be at site 0 or at site L-1 (where a batch call leaves it).
  void snapshot();
  // set_cross: registers npairs entries (bra, ket, site, operator); site -1 is the plain overlap, otherwise the entry
  // takes the next matrix of ops_reim (row-major [out][in], interleaved re / im) whose order is the next of op_dims.
  // Refused: an index outside 0 .. 2B-1, a snapshot index before any snapshot, a site outside -1 .. L-1, an order that is
  // not the site's d, more than BATCH_CROSS_MAX_PAIRS pairs.
  void set_cross(int npairs, const int* bra, const int* ket, const int* site, const double* ops_reim, const int* op_dims);
  bool has_cross() const { return !cross_.empty(); }
  // weights: npairs doubles; values [npairs][2], mean [2]; counts {records, npairs}
  void cross(const double* weights, double* values, double* mean);
  void cross_records(const double* weights, double* values, double* mean, size_t* counts);

  // ---- bond spectra and entanglement entropies (k_batch_spectra) ----
  // The request is a strictly ascending list of bonds q in 0 .. L-2 (bond q lies between sites q and q+1); a replica's
  // record is, per listed bond, BSPEC_HEAD + chi_q doubles (batch_site.h).
  // set_spectra refuses: a bond outside 0 .. L-2, a list that is not strictly ascending, a record of more than
  // BATCH_OBS_MAX_RDM doubles.
  void set_spectra(const int* bonds, int nbonds);
  bool has_spectra() const { return !spec_bonds_.empty(); }
  // centre at site 0.  weights: B doubles; values [B][rec_len], mean [rec_len]; counts {B, rec_len} and {records, B,
  // rec_len}; with all outputs null only the counts are returned.  NotConverged, naming the replica and the bond, when a
  // Jacobi sweep did not converge (that replica's record is zeros; its status word and its tensors stay as they are).
  void spectra(const double* weights, double* values, double* mean, size_t* counts);
  void spectra_records(const double* weights, double* values, double* mean, size_t* counts);

  // ---- sampled configurations (k_batch_sample) ----
  // The request is a number of shots and a seed of its own; a replica's record is configs [nshots][L] (int32), prob
  // [nshots] and freq [F], F = sum d_p (batch_site.h); freq is what is averaged.
  // set_samples refuses: nshots outside 0 .. BATCH_SAMPLE_MAX_SHOTS, nshots * L above BATCH_SAMPLE_MAX_CONFIG.
  void set_samples(int nshots, unsigned long long seed);
  bool has_samples() const { return smp_nshots_ > 0; }
  // centre at site 0.  weights: B doubles; configs [B][nshots][L], prob [B][nshots], freq [B][F], mean_freq [F]; counts
  // {B, nshots, L, F} and {records, B, nshots, L, F}; with all outputs null only the counts are returned.
  void samples(const double* weights, int* configs, double* prob, double* freq, double* mean_freq, size_t* counts);
  void samples_records(const double* weights, int* configs, double* prob, double* freq, double* mean_freq, size_t* counts);

  // ---- expectation values of MPO observables (k_batch_expect) ----
  // The request is a list of operator ids that every replica carries at every site (Engine::set_mpo_core); a replica's
  // record is 2 nops doubles, (re, im) of <psi | O_k | psi> + shift_k <psi | psi> in list order, not normalised.  A
  // refusal names the operator and the site too.
  // set_expect refuses: nops outside 0 .. BATCH_EXPECT_MAX_OPS, a repeated or negative id, an operator that a replica does
  // not carry at every site, core shapes that differ between replicas or whose physical dimension is not the site's, MPO
  // bonds above BATCH_MAX_MPO, outer MPO bonds that are not 1.
  void set_expect(const int* op_ids, int nops);
  bool has_expect() const { return !exp_ops_.empty(); }
  // centre at site 0.  weights: B doubles; values [B][nops][2], mean [nops][2]; counts {B, nops} and {records, B, nops};
  // with all outputs null only the counts are returned.
  void expect(const double* weights, double* values, double* mean, size_t* counts);
  void expect_records(const double* weights, double* values, double* mean, size_t* counts);

  // ---- MPO matrix elements between replicas (k_batch_cross_mpo) ----
  // An entry is (bra, ket, op_id): state indices as for set_cross, op_id an operator every replica carries at every site
  // (Engine::set_mpo_core); its value is <psi_bra | O | psi_ket> + shift <psi_bra | psi_ket> with the cores and the scalar
  // term of the ket's owner (replica ket mod B), not normalised.  A refusal names the entry, the operator and the site too.
  // set_cross_mpo refuses: an index outside 0 .. 2B-1, a snapshot index before any snapshot, a negative op_id, an operator
  // that a replica does not carry at every site, core shapes that differ between replicas, MPO bonds outside
  // 1 .. BATCH_MAX_MPO, neighbouring cores that do not fit, outer MPO bonds that are not 1, more than
  // BATCH_CROSS_MAX_PAIRS entries, a buffer above BATCH_CROSS_MPO_MAX_BYTES.
  void set_cross_mpo(int nentries, const int* bra, const int* ket, const int* op_id);
  bool has_cross_mpo() const { return !xm_.empty(); }
  // centre at site 0 or L-1.  weights: nentries doubles; values [nentries][2], mean [2]; counts {records, nentries}
  void cross_mpo(const double* weights, double* values, double* mean);
  void cross_mpo_records(const double* weights, double* values, double* mean, size_t* counts);

  // ---- an MPO applied to the replicas (k_batch_operate) ----
  // Engine::operate for every selected replica in ONE launch and one host wait: phi ~ O|psi> / |O|psi>| in the bond
  // dimensions of psi, O the operator every selected replica carries under op_id (its scalar term included), up to maxstep
  // double sweeps, each replica stopping on its own when |1 - |<phi_i | phi_{i-1}>|| < conv_tol; reaching maxstep is not
  // an error.  replicas: nsel distinct replica indices, null: all of them.  The selected replicas are WRITTEN: on return
  // their tensors are phi, normalised, centre at site 0, gauge Psi B B ..., every block invalid.  norms [B], iters [B] and
  // statuses [B] are indexed by replica and may each be null; entries of replicas that are not selected are left as given.
  // norms[r]: the norm of the last apply at site 0; iters[r]: double sweeps run; statuses[r]: SS_OK, or SS_EZERO when an
  // apply gave a norm that is not > 0 -- that replica stops (norms[r] = 0, gauge C, centre -1, as a replica that stopped in
  // a step), the others finish.  Krylov memories, the jump generator, channels, the snapshot, every request and the records
  // of the last run() are untouched.  Refused before the GPU is touched, with an ArgError that names the entry point, the
  // replica / operator / site and the limit and leaves everything as it was: maxstep < 1, conv_tol negative or not finite,
  // a replica index out of range or repeated, a selected replica whose centre is not at site 0, an operator that a selected
  // replica does not carry at every site, core shapes that differ between the selected replicas, MPO bonds outside
  // 1 .. BATCH_MAX_MPO, outer MPO bonds that are not 1, neighbouring cores that do not fit, a buffer (selected replicas x
  // carve x 16 bytes, batch_operate_plan.h) above BATCH_OPERATE_MAX_BYTES.
  void operate(int op_id, int maxstep, double conv_tol, const int* replicas, int nsel, double* norms, int* iters, int* statuses);

  // ---- ground states by improved relaxation (k_batch_relax) ----
  // Replicas with relax == 2 take step / sweep / run like the others: a half-sweep is one launch of k_batch_relax, dt is
  // ignored, there is no bond step.  relax() runs up to maxstep full steps (forward + backward half-sweep) of every replica
  // in ONE launch and one host wait.  E_n, the energy of a replica after step n, is the Ritz value of its last local solve
  // (site 0); with conv_tol > 0 a replica stops once |E_n - E_{n-1}| <= conv_tol, the others go on.  energies [B]: the last
  // E_n; steps [B]: steps run; history [B][maxstep]: E_1 .. E_n, NaN behind the stop; statuses [B]: SS_OK, or SS_ENOTCONV
  // when a local solve did not converge in max_diag_krylov vectors (that replica stops as in a step, the others finish).
  // Every output may be null.  The jump generator's step counter, channels, the snapshot, every request and the records of
  // the last run() are untouched.  Refused before the GPU is touched, with an ArgError that names the entry point and the
  // limit and leaves everything as it was: maxstep outside 1 .. BATCH_RELAX_MAX_STEPS, conv_tol negative or not finite,
  // replicas whose relax != 2, a replica whose centre is not at site 0.
  void relax(int maxstep, double conv_tol, double* energies, int* steps, double* history, int* statuses);
  // Thick restarts of the local Lanczos solve (bt_diag): a solve that has not converged after min(N, max_diag_krylov)
  // vectors folds its basis into the lowest Ritz vector and the next Lanczos vector and goes on, up to max_restarts times;
  // only then the replica gets SS_ENOTCONV.  0, the default: no restart.  The setting holds for relax(), step, sweep and
  // run alike.  The call clears the counters.  Refused before the GPU is touched, with an ArgError that names the entry
  // point and the limit: replicas whose relax != 2, max_restarts outside 0 .. BATCH_RELAX_MAX_RESTARTS.
  void set_relax_restarts(int max_restarts);
  // total [B]: the restarts every replica has taken since the setting was made; most [B]: the most of any one of its local
  // solves.  Either may be null.  One host wait.
  void relax_restarts(long long* total, int* most);

  // ---- excited states by deflation against stored states (k_batch_relax_defl, k_batch_defl_overlaps) ----
  // The batch owns up to BATCH_MAX_DEFLATE slots, each a copy of every replica's site tensors (the snapshot's layout,
  // copied by k_batch_snapshot) and one weight per replica.  While the set is not empty, relax() and the relax == 2 paths
  // of step / sweep / run solve every local problem on H_eff + shift + sum_k w_k |q_k><q_k|, q_k the stored state k in the
  // replica's current site basis: the same launches, one workgroup per replica, and E_n is then the energy plus
  // sum_k w_k |<phi_k|psi>|^2.  With an empty set the batch launches k_batch_relax as ever.  The states are stored as they
  // are: the penalty is w |<phi|psi>|^2, so the caller pushes normalised states (relax() leaves them normalised).  The set
  // is dropped where the snapshot is (the replicas' shapes changed); it is independent of the snapshot, of every request,
  // of channels and of fields.
  // deflate_push: ONE launch and one host wait; weights: B doubles.  Refused before the GPU is touched, with an ArgError
  // that names the entry point and the limit and leaves everything as it was: replicas whose relax != 2, a replica whose
  // centre is not at site 0 (or whose chain is not canonical around it), a full set, a null list, a weight that is not
  // finite or not > 0 (the replica is named), a work buffer (batch_deflate_plan.h) above BATCH_DEFLATE_MAX_BYTES (both
  // figures and the largest number of slots that fits are named).
  void deflate_push(const double* weights);
  void deflate_clear() { defl_count_ = 0; }
  int deflate_count();  // validates first: a set that other shapes have dropped counts as empty
  // reim [count][B][2]: <phi_k | psi_r>; ONE launch, one workgroup per (slot, replica), one host wait; with an empty set
  // no launch.  The centre may be at site 0 or at site L-1.  Neither the replicas nor the slots are written.
  void deflate_overlaps(double* reim);

  std::string status_message(int code) const;
  int size() const { return (int)eng_.size(); }
  int device() const { return device_; }
  long long launches() const { return n_launch_; }

 private:
  std::vector<Engine*> eng_;
  int device_ = 0, L_ = 0;
  hipStream_t st_ = nullptr;
  std::vector<hipEvent_t> ev_;
  std::vector<BatchShape> shp_;
  bool shapes_dirty_ = true;
  BatchPlan plan_;
  // reserve(need) of every (array, need) pair given; when one of them has to grow, ONE wait for the stream comes first:
  // work queued on st_ may still use the buffer that is freed.  An array is a DevArr or a RecordStore.
  template <class... A>
  void reserve_synced(A&&... a) {
    if (!all_fit(a...)) HIP_CHECK(hipStreamSynchronize(st_));
    reserve_all(a...);  // a no-op for a DevArr that fits; a RecordStore takes its rows and len from it either way
  }
  static bool all_fit() { return true; }
  template <class A, class N, class... R>
  static bool all_fit(const A& a, const N& need, const R&... r) { return a.fits(need) && all_fit(r...); }
  static void reserve_all() {}
  template <class A, class N, class... R>
  static void reserve_all(A& a, const N& need, R&... r) { a.reserve(need); reserve_all(r...); }
  // device tables; per replica [site L][envL L+1][envR L+1][w2l L][w2el L][w2er L][scratch 1]
  size_t ptrs_per_replica() const { return (size_t)6 * L_ + 3; }
  DevArr<void*> d_ptrs_;
  std::vector<void*> h_ptrs_;
  DevArr<BatchShape> d_shp_;
  DevArr<zc> d_shift_;
  DevArr<int> d_kprev_, d_status_;
  DevArr<long long> d_stats_;
  DevArr<zc> d_scratch_;
  std::vector<zc> h_shift_;
  std::vector<int> h_kprev_;
  long long n_launch_ = 0;

  // observables: the carve behind the sweep's in a replica's scratch area, and the device buffers of a recorded run
  BatchObsPlan obs_plan_;
  size_t carve_ = 0;            // offset of the observation's carve, complex elements
  DevArr<double> d_rec_;        // [nrec][B][rec_len]
  DevArr<double> d_mean_;       // [nrec][rec_len]
  DevArr<double> d_w_;          // [B]
  DevArr<int> d_sites_;         // [L]
  std::vector<double> h_w_, h_rec_, h_mean_;
  std::vector<int> h_sites_;
  // density keys: the leg table and the transfer blocks [B][2][need] of k_batch_density (both grow only)
  BatchDensPlan dens_plan_;
  DevArr<int> d_legs_;
  DevArr<zc> d_tbuf_;
  std::vector<int> h_legs_;

  // channels: the table and the operators (host copies and their device images), the generator's seed, ids and step
  // counter, the jump counters
  std::vector<BatchChanSite> chan_;        // [L]
  std::vector<std::vector<zc>> chan_ops_;  // [L] operators of a site's channel
  int chan_lo_ = -1;                       // lowest site with a channel, -1: none
  bool chan_dirty_ = false;
  std::vector<BatchChanSite> h_chan_;
  std::vector<zc> h_ops_;
  DevArr<BatchChanSite> d_chan_;
  DevArr<zc> d_ops_;
  unsigned long long seed_ = 0;
  // The BATCH's count of time steps launched since the seed was set, the `step` of the generator: it advances by nsteps
  // in every step / run call, with or without channels and whatever the replicas' statuses are -- it says nothing about
  // how far a replica that failed got (its status word does, and it draws nothing more).
  long long steps_done_ = 0;
  std::vector<unsigned long long> h_ids_;
  DevArr<unsigned long long> d_ids_;
  DevArr<long long> d_counts_;
  // pair channels: entry q is bond (q, q + 1); their operators follow the one-site ones in h_ops_ / d_ops_
  std::vector<BatchChanSite> pair_, h_pair_;  // [L]
  std::vector<std::vector<zc>> pair_ops_;     // [L]
  int npair_ = 0;
  DevArr<BatchChanSite> d_pair_;
  DevArr<long long> d_pcounts_;
  DevArr<double> d_disc_;

  // fields: the table per site with V, g and the amplitude tables (host copies and their device images), the
  // Ornstein-Uhlenbeck coefficients of the dt they were last computed for, the field clock, the noise state and the
  // amplitudes of the last step
  std::vector<BatchFieldSite> fld_, h_fld_;    // [L]
  std::vector<std::vector<zc>> fld_vecs_;      // [L]
  std::vector<std::vector<double>> fld_evals_, fld_tabs_;  // [L]
  std::vector<double> fld_tau_;                // [L]
  int fld_lo_ = -1;                            // lowest site with a field, -1: none
  bool fld_dirty_ = false;
  bool fld_decay_set_ = false;
  double fld_decay_dt_ = 0.0;
  long long field_clock_ = 0;
  std::vector<zc> h_fvecs_;
  std::vector<double> h_fevals_, h_ftabs_, h_fdecay_;
  DevArr<BatchFieldSite> d_fld_;
  DevArr<zc> d_fvecs_;
  DevArr<double> d_fevals_, d_ftabs_, d_fdecay_, d_fxi_, d_famp_;
  void check_fields() const;
  void upload_fields(double dt);
  void launch_field(double dt, long long step, long long clock);

  // What the five requests share lies in their RecordStore; the tail of X_records is one function for all of them.
  void records_of(RecordStore& s, const double* weights, double* values, double* mean);

  // cross request: the pairs and their operators (host copies and device images), the transfer buffers [P][buf_len] of
  // k_batch_cross, the records (rows = P, len = 2), the snapshot [B][snap_len]
  std::vector<BatchCrossPair> cross_;
  std::vector<zc> cross_ops_;
  bool cross_dirty_ = false, has_snap_ = false;
  DevArr<BatchCrossPair> d_cross_pairs_;
  DevArr<zc> d_cross_ops_, d_cross_buf_, d_snap_;
  RecordStore cross_rec_;
  size_t snap_len() const;
  size_t cross_buf_len() const { return 2 * (size_t)plan_.max_bond + (size_t)plan_.max_site; }
  void check_cross(const char* entry) const;  // the request against the shapes and the snapshot as they are now
  void prepare_observing();                   // prepare() for a call that only reads the state: centre at 0 or at L-1
  void upload_cross(long nrec);               // device images of the request, room for nrec records and cross()'s slot
  void launch_cross(long record);

  // spectra request: the bonds (host copy and device image), the walk's buffers [B][buf_len], the word per replica that a
  // Jacobi sweep without convergence sets, the records (rows = B, len = spec_rec_len())
  std::vector<int> spec_bonds_;
  bool spec_dirty_ = false;
  DevArr<int> d_spec_bonds_, d_spec_fail_;
  DevArr<zc> d_spec_buf_;
  RecordStore spec_rec_;
  std::vector<int> h_spec_fail_;
  long spec_rec_len() const;
  size_t spec_buf_len() const { return 2 * (size_t)plan_.max_site + (size_t)plan_.max_bond; }
  void check_spectra(const char* entry) const;  // the request against the shapes as they are now
  void upload_spectra(long nrec);               // device image of the request, room for nrec records and spectra()'s slot
  void launch_spectra(long record);
  void spectra_failed(const char* entry) const;  // NotConverged when h_spec_fail_ names a replica

  // samples request: shots and seed, the walk's buffers [B][buf_len], the records: the frequencies, the one averaged
  // array, in the store (rows = B, len = F); configurations and probabilities beside it, sliced by smp_cfg_lay() and
  // smp_prob_lay() with the store's count of records
  int smp_nshots_ = 0;
  unsigned long long smp_seed_ = 0;
  DevArr<zc> d_smp_buf_;
  DevArr<int> d_smp_cfg_;
  DevArr<double> d_smp_prob_;
  RecordStore smp_rec_;
  std::vector<int> h_smp_cfg_, h_smp_cfg_now_;
  std::vector<double> h_smp_prob_, h_smp_prob_now_;
  BatchRecords smp_cfg_lay(long nrec) const { return BatchRecords{eng_.size(), (size_t)smp_nshots_ * L_, (size_t)nrec}; }
  BatchRecords smp_prob_lay(long nrec) const { return BatchRecords{eng_.size(), (size_t)smp_nshots_, (size_t)nrec}; }
  long smp_F() const;           // sum of the physical dimensions
  size_t smp_o_w() const;       // offsets of W and of the weights in a replica's part of d_smp_buf_, and its length
  size_t smp_o_g() const;
  size_t smp_buf_len() const;
  void check_samples(const char* entry) const;  // the request against the shapes as they are now
  void upload_samples(long nrec);               // room for nrec records and samples()'s slot
  void launch_samples(long record, long long step);

  // expect request: the operator ids, the shapes [nops][L] with each operator's MPO bonds and the carve they give, the
  // device tables (operator blocks [B][nops][3 L], shapes, shifts [B][nops]; refreshed with the batch's own tables, since
  // engines may be given new cores between calls), the walk's buffer [B][nops][carve], the records (rows = B, len = 2 nops)
  std::vector<int> exp_ops_;
  std::vector<BatchShape> exp_shp_;
  BatchExpectPlan exp_plan_;
  bool exp_shp_dirty_ = false;
  DevArr<void*> d_exp_ptrs_;
  DevArr<BatchShape> d_exp_shp_;
  DevArr<zc> d_exp_shift_, d_exp_buf_;
  RecordStore exp_rec_;
  std::vector<void*> h_exp_ptrs_;
  std::vector<zc> h_exp_shift_;
  // the shapes of the listed operators on the engines as they are now; ArgError naming the entry point otherwise
  void expect_shapes(const char* entry, const int* op_ids, int nops, std::vector<BatchShape>& shp, BatchExpectPlan& plan) const;
  void check_expect(const char* entry);  // the request against the engines as they are now; new shapes drop the records
  void upload_expect(long nrec);         // the device tables, room for nrec records and expect()'s slot
  void launch_expect(long record);
  // the shapes [nops][L] of the listed operators on the engines as they are now (the gathering half of expect_shapes);
  // ArgError naming the entry point, the operator, the site and the replica otherwise
  // only: the replicas to look at (nonly of them), null: all
  void operator_shapes(const char* entry, const int* op_ids, int nops, std::vector<BatchShape>& shp, const int* only = nullptr,
                       int nonly = 0) const;

  // operate(): the tables of one call (grow only): the selected replicas [nsel], w2l / w2el / w2er of the operator
  // [nsel][3][L], its scalar terms [nsel], the shapes [L] with its MPO bonds, the carve's prefix sums [3][L + 1], the
  // carves [nsel][total], the norms and sweep counts [nsel]
  DevArr<int> d_op_rep_, d_op_iters_;
  DevArr<void*> d_op_ptrs_;
  DevArr<zc> d_op_shift_, d_op_buf_;
  DevArr<BatchShape> d_op_shp_;
  DevArr<long long> d_op_offs_;
  DevArr<double> d_op_norms_;

  // cross request of MPOs: the entries (op = index into xm_ops_, the distinct operator ids in order of first use), the
  // shapes [nops][L] and the carve they give, the device tables (w2el [B][nops][L], shapes, shifts [B][nops]; refreshed
  // with the batch's own tables, since engines may be given new cores between calls), the walk's buffer [P][carve], the
  // records (rows = P, len = 2)
  std::vector<BatchCrossMpoEntry> xm_;
  std::vector<int> xm_ops_;
  std::vector<BatchShape> xm_shp_;
  BatchCrossMpoPlan xm_plan_;
  bool xm_dirty_ = false;
  DevArr<BatchCrossMpoEntry> d_xm_ent_;
  DevArr<void*> d_xm_ptrs_;
  DevArr<BatchShape> d_xm_shp_;
  DevArr<zc> d_xm_shift_, d_xm_buf_;
  RecordStore xm_rec_;
  std::vector<void*> h_xm_ptrs_;
  std::vector<zc> h_xm_shift_;
  // shapes and carve of the listed operators on the engines as they are now, and the buffer cap for nentries entries
  void cross_mpo_shapes(const char* entry, const int* op_ids, int nops, size_t nentries, std::vector<BatchShape>& shp,
                        BatchCrossMpoPlan& plan) const;
  void check_cross_mpo(const char* entry);  // the request against the engines and the snapshot as they are now
  void upload_cross_mpo(long nrec);         // the device tables, room for nrec records and cross_mpo()'s slot
  void launch_cross_mpo(long record);

  static std::vector<BatchShape> shapes_of(Engine& e);
  void check_channels() const;
  void upload_channels();
  void channels_changed();  // chan_lo_, npair_, the dirty flag, and the discarded weights back to zero
  void launch_channel(long long step);
  void reset_generator(unsigned long long seed, const unsigned long long* ids);  // set_seed without its wait for the stream
  void validate();
  void prepare(bool forward, bool build_envs = true);
  void launch(double dt, bool forward);
  void launch_relax(bool forward, int nhalf, double conv_tol, double* energies, int* steps, double* history, int hist_len);
  DevArr<double> d_rx_energy_, d_rx_hist_;  // relax(): [B], [B][maxstep]
  DevArr<int> d_rx_steps_;                  // [B]
  int rx_restarts_ = 0;                     // set_relax_restarts()
  DevArr<long long> d_rx_rst_total_;        // [B] restarts taken; made and zeroed by the first launch_relax
  DevArr<int> d_rx_rst_most_;               // [B] the most of one local solve
  // the deflation set: the filled slots [B][snap_len] each, their weights [BATCH_MAX_DEFLATE][B] (host copy and device
  // image), the kernel's work buffer [B][plan.per] and the buffers of deflate_overlaps
  int defl_count_ = 0;
  DevArr<zc> d_defl_slot_[BATCH_MAX_DEFLATE];
  std::vector<double> h_defl_w_;
  DevArr<double> d_defl_w_, d_defl_ov_;
  DevArr<zc> d_defl_work_, d_defl_ovbuf_;
  void launch_observe(int what, int nsites, long record, long rec_len);
  void launch_density(int nkeys, bool zero_head, long record, long rec_len, long dens_off);
  void finish(bool ends_forward, int half_sweeps, int* statuses, int other_launches = 0, int channel_passes = 0, int field_passes = 0);
  void finish_observe(int launches, int* statuses);
};

}  // namespace mitdvp
