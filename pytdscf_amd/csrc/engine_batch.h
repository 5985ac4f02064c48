// engine_batch.h -- batched trajectories (engine_batch.hip): B borrowed engines stepped by one launch per half-sweep.
// One-site and nearest-neighbour gates and quantum-jump channels set on the batch act between the two half-sweeps of a
// time step: one more launch.
#pragma once
#include <string>
#include <vector>

#include "batch_site.h"
#include "engine.h"

namespace mitdvp {

class Batch {
 public:
  // validates (ArgError otherwise, every engine untouched): one device, distinct engines, no CU mask, single electronic
  // state, not adaptive, not a segment, not bond-sharded, relax 0 or 1, no gates / Kraus maps, identical site and MPO shapes
  // and identical integrator settings across the replicas, shapes inside the envelope of batch_plan
  explicit Batch(const std::vector<Engine*>& engines);
  ~Batch();
  Batch(const Batch&) = delete;
  Batch& operator=(const Batch&) = delete;

  void step(double dt, int nsteps, int* statuses);        // statuses[i]: SS_OK / SS_ENOTCONV / SS_EZERO of replica i
  void sweep(double dt, bool forward, int* statuses);  // refused while a channel is set

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
  // ---- cross overlaps and one-site matrix elements between replicas (k_batch_cross, k_batch_snapshot) ----
  // A state index 0 .. B-1 names replica i, B + r the snapshot of replica r.  Every refusal is an ArgError that names the
  // entry point and the limit and leaves the request, the snapshot and every engine as they were.
  // snapshot: ONE launch copies every site tensor of every replica into the batch's snapshot buffer; one host wait.  The
  // centre may be at site 0 or at site L-1 (where a batch call leaves it).
  void snapshot();
  // set_cross: registers npairs entries (bra, ket, site, operator); site -1 is the plain overlap, otherwise the entry
  // takes the next matrix of ops_reim (row-major [out][in], interleaved re / im) whose order is the next of op_dims.
  // npairs = 0 removes the request.  Refused: an index outside 0 .. 2B-1, a snapshot index before any snapshot, a site
  // outside -1 .. L-1, an order that is not the site's d, more than BATCH_CROSS_MAX_PAIRS pairs.  No launch, no wait.
  void set_cross(int npairs, const int* bra, const int* ket, const int* site, const double* ops_reim, const int* op_dims);
  bool has_cross() const { return !cross_.empty(); }
  // cross: the request on the current state: k_batch_cross and k_batch_mean, TWO launches, one host wait.  weights:
  // npairs doubles or null (1 / npairs); values [npairs][2] and mean [2] may each be null.
  void cross(const double* weights, double* values, double* mean);
  // While a request is set every record of run() records it too: ONE more launch per record (k_batch_cross behind the
  // record's other launches) and ONE more k_batch_mean launch per call (weights 1 / npairs); values and means are copied
  // with the rest, no further host wait.  cross_records returns what the last run() recorded: values
  // [records][npairs][2], mean [records][2], counts {records, npairs}; each may be null.  weights null: the means of the
  // run, no launch and no wait; weights given (npairs doubles): ONE k_batch_mean launch over the records, which are still
  // on the device, and one host wait.
  void cross_records(const double* weights, double* values, double* mean, size_t* counts);

  // ---- bond spectra and entanglement entropies (k_batch_spectra) ----
  // The request is a strictly ascending list of bonds q in 0 .. L-2 (bond q lies between sites q and q+1); a replica's
  // record is, per listed bond, BSPEC_HEAD + chi_q doubles (batch_site.h).  Every refusal is an ArgError that names the
  // entry point and the limit and leaves the request, the records and every engine as they were.
  // set_spectra: nbonds = 0 removes the request.  Refused: a bond outside 0 .. L-2, a list that is not strictly ascending,
  // a record of more than BATCH_OBS_MAX_RDM doubles.  No launch, no wait.
  void set_spectra(const int* bonds, int nbonds);
  bool has_spectra() const { return !spec_bonds_.empty(); }
  // spectra: the request on the current state (centre at site 0): k_batch_spectra and k_batch_mean, TWO launches, one host
  // wait.  weights: B doubles or null (1 / B); values [B][rec_len] and mean [rec_len] may each be null; counts {B,
  // rec_len}; with all outputs null only the counts are returned.  NotConverged, naming the replica and the bond, when a
  // Jacobi sweep did not converge (that replica's record is zeros; its status word and its tensors stay as they are).
  void spectra(const double* weights, double* values, double* mean, size_t* counts);
  // While a request is set every record of run() records it too: ONE more launch per record (k_batch_spectra behind the
  // record's other launches) and ONE more k_batch_mean launch per call (weights 1 / B); values and means are copied with
  // the rest, no further host wait.  spectra_records returns what the last run() recorded: values
  // [records][B][rec_len], mean [records][rec_len], counts {records, B, rec_len}; each may be null.  weights null: the
  // means of the run, no launch and no wait; weights given (B doubles): ONE k_batch_mean launch over the records, which
  // are still on the device, and one host wait.
  void spectra_records(const double* weights, double* values, double* mean, size_t* counts);

  // ---- sampled configurations (k_batch_sample) ----
  // The request is a number of shots and a seed of its own; a replica's record is configs [nshots][L] (int32), prob
  // [nshots] and freq [F], F = sum d_p (batch_site.h).  Every refusal is an ArgError that names the entry point and the
  // limit and leaves the request, the records and every engine as they were.
  // set_samples: nshots = 0 removes the request.  Refused: nshots outside 0 .. BATCH_SAMPLE_MAX_SHOTS, nshots * L above
  // BATCH_SAMPLE_MAX_CONFIG.  No launch, no wait.
  void set_samples(int nshots, unsigned long long seed);
  bool has_samples() const { return smp_nshots_ > 0; }
  // samples: the request on the current state (centre at site 0): k_batch_sample and k_batch_mean, TWO launches, one host
  // wait.  weights: B doubles or null (1 / B); configs [B][nshots][L], prob [B][nshots], freq [B][F] and mean_freq [F]
  // may each be null; counts {B, nshots, L, F}; with all outputs null only the counts are returned.
  void samples(const double* weights, int* configs, double* prob, double* freq, double* mean_freq, size_t* counts);
  // While a request is set every record of run() records it too: ONE more launch per record (k_batch_sample behind the
  // record's other launches) and ONE more k_batch_mean launch per call (weights 1 / B); values and means are copied with
  // the rest, no further host wait.  samples_records returns what the last run() recorded, the arrays of samples() with a
  // leading record axis, counts {records, B, nshots, L, F}; each may be null.  weights null: the means of the run, no
  // launch and no wait; weights given (B doubles): ONE k_batch_mean launch over the records, which are still on the
  // device, and one host wait.
  void samples_records(const double* weights, int* configs, double* prob, double* freq, double* mean_freq, size_t* counts);

  // ---- expectation values of MPO observables (k_batch_expect) ----
  // The request is a list of operator ids that every replica carries at every site (Engine::set_mpo_core); a replica's
  // record is 2 nops doubles, (re, im) of <psi | O_k | psi> + shift_k <psi | psi> in list order, not normalised.  Every
  // refusal is an ArgError that names the entry point, the operator, the site and the limit and leaves the request, the
  // records and every engine as they were.
  // set_expect: nops = 0 removes the request.  Refused: nops outside 0 .. BATCH_EXPECT_MAX_OPS, a repeated or negative id,
  // an operator that a replica does not carry at every site, core shapes that differ between replicas or whose physical
  // dimension is not the site's, MPO bonds above BATCH_MAX_MPO, outer MPO bonds that are not 1.  No launch, no wait.
  void set_expect(const int* op_ids, int nops);
  bool has_expect() const { return !exp_ops_.empty(); }
  // expect: the request on the current state (centre at site 0): k_batch_expect and k_batch_mean, TWO launches, one host
  // wait.  weights: B doubles or null (1 / B); values [B][nops][2] and mean [nops][2] may each be null; counts {B, nops};
  // with all outputs null only the counts are returned.
  void expect(const double* weights, double* values, double* mean, size_t* counts);
  // While a request is set every record of run() records it too: ONE more launch per record (k_batch_expect behind the
  // record's other launches) and ONE more k_batch_mean launch per call (weights 1 / B); values and means are copied with
  // the rest, no further host wait.  expect_records returns what the last run() recorded: values [records][B][nops][2],
  // mean [records][nops][2], counts {records, B, nops}; each may be null.  weights null: the means of the run, no launch
  // and no wait; weights given (B doubles): ONE k_batch_mean launch over the records, which are still on the device, and
  // one host wait.
  void expect_records(const double* weights, double* values, double* mean, size_t* counts);

  // ---- MPO matrix elements between replicas (k_batch_cross_mpo) ----
  // An entry is (bra, ket, op_id): state indices as for set_cross, op_id an operator every replica carries at every site
  // (Engine::set_mpo_core); its value is <psi_bra | O | psi_ket> + shift <psi_bra | psi_ket> with the cores and the scalar
  // term of the ket's owner (replica ket mod B), not normalised.  Every refusal is an ArgError that names the entry point,
  // the entry, the operator, the site and the limit and leaves the request, the records, the snapshot and every engine as
  // they were.
  // set_cross_mpo: nentries = 0 removes the request.  Refused: an index outside 0 .. 2B-1, a snapshot index before any
  // snapshot, a negative op_id, an operator that a replica does not carry at every site, core shapes that differ between
  // replicas, MPO bonds outside 1 .. BATCH_MAX_MPO, neighbouring cores that do not fit, outer MPO bonds that are not 1,
  // more than BATCH_CROSS_MAX_PAIRS entries, a buffer above BATCH_CROSS_MPO_MAX_BYTES.  No launch, no wait.
  void set_cross_mpo(int nentries, const int* bra, const int* ket, const int* op_id);
  bool has_cross_mpo() const { return !xm_.empty(); }
  // cross_mpo: the request on the current state (centre at site 0 or L-1): k_batch_cross_mpo and k_batch_mean, TWO
  // launches, one host wait.  weights: nentries doubles or null (1 / nentries); values [nentries][2] and mean [2] may each
  // be null.
  void cross_mpo(const double* weights, double* values, double* mean);
  // While a request is set every record of run() records it too: ONE more launch per record and ONE more k_batch_mean
  // launch per call (weights 1 / nentries), no further host wait.  cross_mpo_records returns what the last run() recorded:
  // values [records][nentries][2], mean [records][2], counts {records, nentries}; each may be null.  weights null: the
  // means of the run, no launch and no wait; weights given: ONE k_batch_mean launch over the records and one host wait.
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
  // device tables; per replica [site L][envL L+1][envR L+1][w2l L][w2el L][w2er L][scratch 1]
  size_t ptrs_per_replica() const { return (size_t)6 * L_ + 3; }
  void** d_ptrs_ = nullptr;
  std::vector<void*> h_ptrs_;
  BatchShape* d_shp_ = nullptr;
  zc* d_shift_ = nullptr;
  int* d_kprev_ = nullptr;
  int* d_status_ = nullptr;
  long long* d_stats_ = nullptr;
  zc* d_scratch_ = nullptr;
  size_t scratch_elems_ = 0;
  std::vector<zc> h_shift_;
  std::vector<int> h_kprev_;
  long long n_launch_ = 0;

  // observables: the carve behind the sweep's in a replica's scratch area, and the device buffers of a recorded run
  BatchObsPlan obs_plan_;
  size_t carve_ = 0;            // offset of the observation's carve, complex elements
  double* d_rec_ = nullptr;     // [nrec][B][rec_len]
  double* d_mean_ = nullptr;    // [nrec][rec_len]
  double* d_w_ = nullptr;       // [B]
  int* d_sites_ = nullptr;      // [L]
  size_t rec_elems_ = 0, mean_elems_ = 0;
  std::vector<double> h_w_, h_rec_, h_mean_;
  std::vector<int> h_sites_;
  // density keys: the leg table and the transfer blocks [B][2][need] of k_batch_density (both grow only)
  BatchDensPlan dens_plan_;
  int* d_legs_ = nullptr;
  zc* d_tbuf_ = nullptr;
  size_t legs_elems_ = 0, tbuf_elems_ = 0;
  std::vector<int> h_legs_;

  // channels: the table and the operators (host copies and their device images), the generator's seed, ids and step
  // counter, the jump counters
  std::vector<BatchChanSite> chan_;        // [L]
  std::vector<std::vector<zc>> chan_ops_;  // [L] operators of a site's channel
  int chan_lo_ = -1;                       // lowest site with a channel, -1: none
  bool chan_dirty_ = false;
  std::vector<BatchChanSite> h_chan_;
  std::vector<zc> h_ops_;
  BatchChanSite* d_chan_ = nullptr;
  zc* d_ops_ = nullptr;
  size_t ops_elems_ = 0;
  unsigned long long seed_ = 0;
  // The BATCH's count of time steps launched since the seed was set, the `step` of the generator: it advances by nsteps
  // in every step / run call, with or without channels and whatever the replicas' statuses are -- it says nothing about
  // how far a replica that failed got (its status word does, and it draws nothing more).
  long long steps_done_ = 0;
  std::vector<unsigned long long> h_ids_;
  unsigned long long* d_ids_ = nullptr;
  long long* d_counts_ = nullptr;
  // pair channels: entry q is bond (q, q + 1); their operators follow the one-site ones in h_ops_ / d_ops_
  std::vector<BatchChanSite> pair_, h_pair_;  // [L]
  std::vector<std::vector<zc>> pair_ops_;     // [L]
  int npair_ = 0;
  BatchChanSite* d_pair_ = nullptr;
  long long* d_pcounts_ = nullptr;
  double* d_disc_ = nullptr;

  // cross request: the pairs and their operators (host copies and device images), the transfer buffers [P][buf_len] of
  // k_batch_cross, the records [nrec + 1][P][2] (the slot behind a run's records is cross()'s own) and their means, the
  // snapshot [B][snap_len]
  std::vector<BatchCrossPair> cross_;
  std::vector<zc> cross_ops_;
  bool cross_dirty_ = false, has_snap_ = false;
  BatchCrossPair* d_cross_pairs_ = nullptr;
  zc *d_cross_ops_ = nullptr, *d_cross_buf_ = nullptr, *d_snap_ = nullptr;
  double *d_cross_rec_ = nullptr, *d_cross_mean_ = nullptr, *d_cross_w_ = nullptr;
  size_t cross_pairs_elems_ = 0, cross_ops_elems_ = 0, cross_buf_elems_ = 0, cross_rec_slots_ = 0,
         cross_mean_slots_ = 0, snap_elems_ = 0;  // cross_rec_slots_ / cross_mean_slots_: doubles
  long cross_nrec_ = 0;  // records of the last run() held in d_cross_rec_ / h_cross_rec_
  std::vector<double> h_cross_rec_, h_cross_mean_, h_cross_w_, h_cross_now_;
  size_t snap_len() const;
  size_t cross_buf_len() const { return 2 * (size_t)plan_.max_bond + (size_t)plan_.max_site; }
  void check_cross(const char* entry) const;  // the request against the shapes and the snapshot as they are now
  void prepare_observing();                   // prepare() for a call that only reads the state: centre at 0 or at L-1
  void upload_cross(long nrec);               // device images of the request, room for nrec records and cross()'s slot
  void launch_cross(long record);
  void cross_weights(const double* weights);

  // spectra request: the bonds (host copy and device image), the walk's buffers [B][buf_len], the word per replica that a
  // Jacobi sweep without convergence sets, the records [nrec + 1][B][rec_len] (the slot behind a run's records is
  // spectra()'s own) and their means
  std::vector<int> spec_bonds_;
  bool spec_dirty_ = false;
  int *d_spec_bonds_ = nullptr, *d_spec_fail_ = nullptr;
  zc* d_spec_buf_ = nullptr;
  double *d_spec_rec_ = nullptr, *d_spec_mean_ = nullptr, *d_spec_w_ = nullptr;
  size_t spec_buf_elems_ = 0, spec_rec_slots_ = 0, spec_mean_slots_ = 0;  // the last two: doubles
  long spec_nrec_ = 0;  // records of the last run() held in d_spec_rec_ / h_spec_rec_
  std::vector<double> h_spec_rec_, h_spec_mean_, h_spec_w_, h_spec_now_;
  std::vector<int> h_spec_fail_;
  long spec_rec_len() const;
  size_t spec_buf_len() const { return 2 * (size_t)plan_.max_site + (size_t)plan_.max_bond; }
  void check_spectra(const char* entry) const;  // the request against the shapes as they are now
  void upload_spectra(long nrec);               // device image of the request, room for nrec records and spectra()'s slot
  void launch_spectra(long record);
  void spectra_weights(const double* weights);
  void spectra_failed(const char* entry) const;  // NotConverged when h_spec_fail_ names a replica

  // samples request: shots and seed, the walk's buffers [B][buf_len], the records [nrec + 1] of configurations,
  // probabilities and frequencies (the slot behind a run's records is samples()'s own) and the frequencies' means
  int smp_nshots_ = 0;
  unsigned long long smp_seed_ = 0;
  zc* d_smp_buf_ = nullptr;
  int* d_smp_cfg_ = nullptr;
  double *d_smp_prob_ = nullptr, *d_smp_freq_ = nullptr, *d_smp_mean_ = nullptr, *d_smp_w_ = nullptr;
  size_t smp_buf_elems_ = 0, smp_cfg_slots_ = 0, smp_prob_slots_ = 0, smp_freq_slots_ = 0, smp_mean_slots_ = 0;
  long smp_nrec_ = 0;  // records of the last run() held in d_smp_* / h_smp_*
  std::vector<int> h_smp_cfg_, h_smp_cfg_now_;
  std::vector<double> h_smp_prob_, h_smp_freq_, h_smp_mean_, h_smp_w_, h_smp_now_;
  long smp_F() const;           // sum of the physical dimensions
  size_t smp_o_w() const;       // offsets of W and of the weights in a replica's part of d_smp_buf_, and its length
  size_t smp_o_g() const;
  size_t smp_buf_len() const;
  void check_samples(const char* entry) const;  // the request against the shapes as they are now
  void upload_samples(long nrec);               // room for nrec records and samples()'s slot
  void launch_samples(long record, long long step);
  void samples_weights(const double* weights);

  // expect request: the operator ids, the shapes [nops][L] with each operator's MPO bonds and the carve they give, the
  // device tables (operator blocks [B][nops][3 L], shapes, shifts [B][nops]; refreshed with the batch's own tables, since
  // engines may be given new cores between calls), the walk's buffer [B][nops][carve], the records [nrec + 1][B][2 nops]
  // (the slot behind a run's records is expect()'s own) and their means
  std::vector<int> exp_ops_;
  std::vector<BatchShape> exp_shp_;
  BatchExpectPlan exp_plan_;
  bool exp_shp_dirty_ = false;
  void** d_exp_ptrs_ = nullptr;
  BatchShape* d_exp_shp_ = nullptr;
  zc *d_exp_shift_ = nullptr, *d_exp_buf_ = nullptr;
  double *d_exp_rec_ = nullptr, *d_exp_mean_ = nullptr, *d_exp_w_ = nullptr;
  size_t exp_ptrs_elems_ = 0, exp_shp_elems_ = 0, exp_shift_elems_ = 0, exp_buf_elems_ = 0, exp_rec_slots_ = 0,
         exp_mean_slots_ = 0;  // the last two: doubles
  long exp_nrec_ = 0;  // records of the last run() held in d_exp_rec_ / h_exp_rec_
  std::vector<void*> h_exp_ptrs_;
  std::vector<zc> h_exp_shift_;
  std::vector<double> h_exp_rec_, h_exp_mean_, h_exp_w_, h_exp_now_;
  // the shapes of the listed operators on the engines as they are now; ArgError naming the entry point otherwise
  void expect_shapes(const char* entry, const int* op_ids, int nops, std::vector<BatchShape>& shp, BatchExpectPlan& plan) const;
  void check_expect(const char* entry);  // the request against the engines as they are now; new shapes drop the records
  void upload_expect(long nrec);         // the device tables, room for nrec records and expect()'s slot
  void launch_expect(long record);
  void expect_weights(const double* weights);
  // the shapes [nops][L] of the listed operators on the engines as they are now (the gathering half of expect_shapes);
  // ArgError naming the entry point, the operator, the site and the replica otherwise
  // only: the replicas to look at (nonly of them), null: all
  void operator_shapes(const char* entry, const int* op_ids, int nops, std::vector<BatchShape>& shp, const int* only = nullptr,
                       int nonly = 0) const;

  // operate(): the tables of one call (grow only): the selected replicas [nsel], w2l / w2el / w2er of the operator
  // [nsel][3][L], its scalar terms [nsel], the shapes [L] with its MPO bonds, the carve's prefix sums [3][L + 1], the
  // carves [nsel][total], the norms and sweep counts [nsel]
  int* d_op_rep_ = nullptr;
  void** d_op_ptrs_ = nullptr;
  zc *d_op_shift_ = nullptr, *d_op_buf_ = nullptr;
  BatchShape* d_op_shp_ = nullptr;
  long long* d_op_offs_ = nullptr;
  double* d_op_norms_ = nullptr;
  int* d_op_iters_ = nullptr;
  size_t op_rep_elems_ = 0, op_ptrs_elems_ = 0, op_shift_elems_ = 0, op_buf_elems_ = 0, op_shp_elems_ = 0, op_offs_elems_ = 0,
         op_norms_elems_ = 0, op_iters_elems_ = 0;

  // cross request of MPOs: the entries (op = index into xm_ops_, the distinct operator ids in order of first use), the
  // shapes [nops][L] and the carve they give, the device tables (w2el [B][nops][L], shapes, shifts [B][nops]; refreshed
  // with the batch's own tables, since engines may be given new cores between calls), the walk's buffer [P][carve], the
  // records [nrec + 1][P][2] (the slot behind a run's records is cross_mpo()'s own) and their means, the weights [P]
  std::vector<BatchCrossMpoEntry> xm_;
  std::vector<int> xm_ops_;
  std::vector<BatchShape> xm_shp_;
  BatchCrossMpoPlan xm_plan_;
  bool xm_dirty_ = false;
  BatchCrossMpoEntry* d_xm_ent_ = nullptr;
  void** d_xm_ptrs_ = nullptr;
  BatchShape* d_xm_shp_ = nullptr;
  zc *d_xm_shift_ = nullptr, *d_xm_buf_ = nullptr;
  double *d_xm_rec_ = nullptr, *d_xm_mean_ = nullptr, *d_xm_w_ = nullptr;
  size_t xm_ent_elems_ = 0, xm_ptrs_elems_ = 0, xm_shp_elems_ = 0, xm_shift_elems_ = 0, xm_buf_elems_ = 0, xm_rec_slots_ = 0,
         xm_mean_slots_ = 0, xm_w_elems_ = 0;  // xm_rec_slots_ / xm_mean_slots_: doubles
  long xm_nrec_ = 0;  // records of the last run() held in d_xm_rec_ / h_xm_rec_
  std::vector<void*> h_xm_ptrs_;
  std::vector<zc> h_xm_shift_;
  std::vector<double> h_xm_rec_, h_xm_mean_, h_xm_w_, h_xm_now_;
  // shapes and carve of the listed operators on the engines as they are now, and the buffer cap for nentries entries
  void cross_mpo_shapes(const char* entry, const int* op_ids, int nops, size_t nentries, std::vector<BatchShape>& shp,
                        BatchCrossMpoPlan& plan) const;
  void check_cross_mpo(const char* entry);  // the request against the engines and the snapshot as they are now
  void upload_cross_mpo(long nrec);         // the device tables, room for nrec records and cross_mpo()'s slot
  void launch_cross_mpo(long record);
  void cross_mpo_weights(const double* weights);

  static std::vector<BatchShape> shapes_of(Engine& e);
  void check_channels() const;
  void upload_channels();
  void channels_changed();  // chan_lo_, npair_, the dirty flag, and the discarded weights back to zero
  void launch_channel(long long step);
  void reset_generator(unsigned long long seed, const unsigned long long* ids);  // set_seed without its wait for the stream
  void validate();
  void prepare(bool forward, bool build_envs = true);
  void launch(double dt, bool forward);
  void launch_observe(int what, int nsites, long record, long rec_len);
  void launch_density(int nkeys, bool zero_head, long record, long rec_len, long dens_off);
  void finish(bool ends_forward, int half_sweeps, int* statuses, int other_launches = 0, int channel_passes = 0);
  void finish_observe(int launches, int* statuses);
};

}  // namespace mitdvp
