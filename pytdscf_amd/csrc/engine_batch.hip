// engine_batch.hip -- batched trajectories on the host side: a Batch borrows B ordinary engines (each owns its tensors and
// its own MPO), owns the pointer tables, the status words and the per-replica scratch of k_batch_sweep (batch_site.hip),
// and steps all replicas with ONE launch per half-sweep (and, while one-site channels are set on the batch -- gates,
// quantum-jump channels: the table, the operators, the generator's seed / ids / step counter and the jump counters are the
// batch's -- ONE launch of k_batch_channel between the two half-sweeps of a time step, or of k_batch_pair in its place
// while a nearest-neighbour channel is set: its table, counters and discarded weights are the batch's too).  No host threads, no compute-unit masks, no persistent-launch
// admission: the kernel's workgroups never wait for each other.  Host waits of a call: ONE stream synchronisation, behind
// the copy of the status words at its end (plain hipStreamSynchronize: the library's wait helper, wait_published, spins on
// a mapped word, which this path has none of); besides it only what the engines' own preparation does on first use
// (right-environment build, workspace growth) and one synchronisation when the scratch area has to grow.
#include "engine_batch.h"
#include "capi_internal.h"

#include <map>
#include <algorithm>
#include <cmath>
#include <cstring>

mitdvp_batch::mitdvp_batch() = default;
mitdvp_batch::~mitdvp_batch() = default;

namespace mitdvp {

// ---- the records of one request (RecordStore, engine_batch.h) ----
void RecordStore::reserve(const BatchRecords& l) {
  if (nrec > 0 && ((long)l.nrec != nrec || l.rows != rows || l.len != len || !rec.fits(l.rec_elems()) || !mean.fits(l.mean_elems())))
    throw std::logic_error("batch: the records of the last run are still held, and room is asked for others");
  rec.reserve(l.rec_elems());
  mean.reserve(l.mean_elems());
  w.reserve(l.rows);
  rows = l.rows;
  len = l.len;
}

void RecordStore::weights(hipStream_t st, const double* weights) {
  h_w.assign(rows, 1.0 / (double)rows);
  if (weights) h_w.assign(weights, weights + rows);
  HIP_CHECK(hipMemcpyAsync(w, h_w.data(), rows * sizeof(double), hipMemcpyHostToDevice, st));
}

void RecordStore::mean_of_run(hipStream_t st, long nrec_run, long long& n_launch) {
  weights(st, nullptr);
  nrec = nrec_run;
  batch_mean_launch(st, rec, w, mean + lay().mean_run(), (int)rows, (long)len, nrec);
  n_launch += 1;
}

void RecordStore::fetch_run(hipStream_t st) {
  const BatchRecords l = lay();
  h_rec.resize(l.rec_now());                  // the slots in front of the call's own
  h_mean.resize(l.mean_now() - l.mean_run());  // the first region
  HIP_CHECK(hipMemcpyAsync(h_rec.data(), rec, h_rec.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_mean.data(), mean + l.mean_run(), h_mean.size() * sizeof(double), hipMemcpyDeviceToHost, st));
}

void RecordStore::mean_of_slot(hipStream_t st, long long& n_launch) {
  const BatchRecords l = lay();
  batch_mean_launch(st, rec + l.rec_now(), w, mean + l.mean_now(), (int)rows, (long)len, 1);
  n_launch += 1;
}

void RecordStore::fetch_slot(hipStream_t st, bool values, bool mean_too) {
  const BatchRecords l = lay();
  h_now.resize(l.slot_elems() + len);
  if (values) HIP_CHECK(hipMemcpyAsync(h_now.data(), rec + l.rec_now(), l.slot_elems() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mean_too) HIP_CHECK(hipMemcpyAsync(h_now.data() + l.slot_elems(), mean + l.mean_now(), len * sizeof(double), hipMemcpyDeviceToHost, st));
}

void RecordStore::slot_out(double* values, double* mean_out) const {
  const size_t ne = lay().slot_elems();
  if (values) std::memcpy(values, h_now.data(), ne * sizeof(double));
  if (mean_out) std::memcpy(mean_out, h_now.data() + ne, len * sizeof(double));
}

bool RecordStore::records(hipStream_t st, const double* weights_in, double* values, double* mean_out, long long& n_launch) {
  const BatchRecords l = lay();
  if (values) std::memcpy(values, h_rec.data(), l.rec_now() * sizeof(double));
  if (!mean_out) return false;
  if (!weights_in) {
    std::memcpy(mean_out, h_mean.data(), (l.mean_now() - l.mean_run()) * sizeof(double));
    return false;
  }
  weights(st, weights_in);
  double* dst = mean + l.mean_reweighted();  // behind the run's own means and the slot's: both stay as they are
  batch_mean_launch(st, rec, w, dst, (int)rows, (long)len, nrec);
  n_launch += 1;
  HIP_CHECK(hipMemcpyAsync(mean_out, dst, (l.mean_now() - l.mean_run()) * sizeof(double), hipMemcpyDeviceToHost, st));
  return true;
}

std::vector<BatchShape> Batch::shapes_of(Engine& e) {
  std::vector<BatchShape> s((size_t)e.L_);
  auto it = e.ops_.find(0);
  for (int p = 0; p < e.L_; ++p) {
    if (!e.site_[p].p) throw ArgError("batch: a replica has no tensor at site " + std::to_string(p));
    if (it == e.ops_.end() || !it->second.sites[p].set) throw ArgError("batch: a replica has no MPO core at site " + std::to_string(p));
    const MpoSite& w = it->second.sites[p];
    if (w.d != e.dd_[p]) throw ArgError("MPO physical dimension differs from the site tensor's");
    s[p] = BatchShape{e.dl_[p], e.dd_[p], e.dr_[p], w.ml, w.mr};
  }
  return s;
}

// everything mitdvp_batch_create promises to check; touches no engine state
void Batch::validate() {
  const int n = (int)eng_.size();
  Engine& e0 = *eng_[0];
  for (int i = 0; i < n; ++i) {
    Engine& e = *eng_[i];
    const std::string who = "batch: replica " + std::to_string(i) + " ";
    for (int k = 0; k < i; ++k)
      if (eng_[k] == eng_[i]) throw ArgError("batch: the same engine is listed twice");
    if (e.cfg.device != e0.cfg.device) throw ArgError(who + "is on another device");
    if (e.cfg.cu_count != 0) throw ArgError(who + "is confined to a compute-unit range (cu_count != 0): the batched kernel runs on the whole device");
    if (e.ms_) throw ArgError(who + "has several electronic states");
    if (e.adaptive_) throw ArgError(who + "has an adaptive bond dimension");
    if (e.segment_) throw ArgError(who + "is a segment of a site-sharded chain");
    if (e.nranks_ != 1) throw ArgError(who + "is bond-sharded over several GPUs");
    if (e.cfg.relax < 0 || e.cfg.relax > 2) throw ArgError(who + "has relax = " + std::to_string(e.cfg.relax) + " (relax must be 0, 1 or 2)");
    if (!e.gates_.empty() || !e.kraus_.empty()) throw ArgError(who + "has gates or Kraus maps set");
    if (e.sw_next_ >= 0) throw ArgError(who + "has a half-sweep in parts in progress");
    if (e.L_ != e0.L_) throw ArgError(who + "has another number of sites");
    if (e.cfg.integrator != e0.cfg.integrator || e.cfg.lanczos_variant != e0.cfg.lanczos_variant ||
        e.cfg.conserve_norm != e0.cfg.conserve_norm || e.cfg.thresh != e0.cfg.thresh || e.cfg.max_krylov != e0.cfg.max_krylov ||
        e.cfg.relax != e0.cfg.relax)
      throw ArgError(who + "differs from replica 0 in integrator, lanczos_variant, conserve_norm, thresh, max_krylov or relax");
  }
  if (e0.cfg.max_krylov < 1 || e0.cfg.max_krylov > MAXK - 1) throw ArgError("batch: max_krylov must be in [1, 20]");
  if (e0.cfg.relax == 2) {  // improved relaxation: one cap of the eigen-solver's Krylov space for all replicas, 2 .. 64
    for (int i = 1; i < n; ++i)
      if (eng_[i]->max_diag_krylov_ != e0.max_diag_krylov_)
        throw ArgError("batch: replica " + std::to_string(i) + " differs from replica 0 in max_diag_krylov (" +
                       std::to_string(eng_[i]->max_diag_krylov_) + " against " + std::to_string(e0.max_diag_krylov_) + ")");
    std::string bad;
    if (!batch_relax_kcap_ok(e0.max_diag_krylov_, bad)) throw ArgError("batch: " + bad);
  }
  std::vector<BatchShape> s0 = shapes_of(e0);
  for (int i = 1; i < n; ++i) {
    std::vector<BatchShape> s = shapes_of(*eng_[i]);
    for (int p = 0; p < e0.L_; ++p) {
      if (s[p].dl != s0[p].dl || s[p].d != s0[p].d || s[p].dr != s0[p].dr)
        throw ArgError("batch: replica " + std::to_string(i) + " differs from replica 0 in the shape of site " + std::to_string(p));
      if (s[p].ml != s0[p].ml || s[p].mr != s0[p].mr)
        throw ArgError("batch: replica " + std::to_string(i) + " differs from replica 0 in the MPO bonds of site " + std::to_string(p));
    }
  }
  for (int p = 0; p + 1 < e0.L_; ++p)
    if (s0[p].dr != s0[p + 1].dl) throw ArgError("bond dimension mismatch between neighbouring sites");
  for (int p = 0; p + 1 < e0.L_; ++p)  // the kernel writes block p + 1 with mr[p]; the buffer is sized with ml[p + 1]
    if (s0[p].mr != s0[p + 1].ml)
      throw ArgError("batch: MPO bond mismatch between sites " + std::to_string(p) + " and " + std::to_string(p + 1));
  if (s0[0].ml != 1 || s0[e0.L_ - 1].mr != 1) throw ArgError("batch: the outer MPO bonds must be 1");
  if (s0[0].dl != 1 || s0[e0.L_ - 1].dr != 1) throw ArgError("open boundary bonds must be 1");
  BatchPlan pl;
  std::string why;
  if (!batch_plan(s0.data(), e0.L_, pl, why, e0.cfg.relax, e0.max_diag_krylov_)) throw ArgError(why);
  if (s0.size() != shp_.size() || std::memcmp(s0.data(), shp_.data(), s0.size() * sizeof(BatchShape)) != 0) {
    shp_ = s0;
    shapes_dirty_ = true;
    has_snap_ = false;  // a snapshot of other shapes names nothing any more
    defl_count_ = 0;    // nor do the stored states of the deflation set
    spec_rec_.drop();   // nor do spectra records of other bond dimensions
    smp_rec_.drop();    // nor sampled configurations of other shapes
    exp_rec_.drop();    // nor expectation values walked over other bonds
    xm_rec_.drop();     // nor MPO matrix elements between states of other bonds
  }
  plan_ = pl;
  batch_observe_plan(plan_, obs_plan_);
  carve_ = (plan_.total + 15) / 16 * 16;
}

Batch::Batch(const std::vector<Engine*>& engines) : eng_(engines) {
  if (eng_.empty()) throw ArgError("batch: no replicas");
  for (Engine* e : eng_)
    if (!e) throw ArgError("batch: null engine");
  validate();
  device_ = eng_[0]->cfg.device;
  L_ = eng_[0]->L_;
  HIP_CHECK(hipSetDevice(device_));
  HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
  const size_t n = eng_.size();
  ev_.assign(n, nullptr);
  for (size_t i = 0; i < n; ++i) HIP_CHECK(hipEventCreateWithFlags(&ev_[i], hipEventDisableTiming));
  d_ptrs_.reserve(n * ptrs_per_replica());
  d_shp_.reserve((size_t)L_);
  d_shift_.reserve(n);
  d_kprev_.reserve(n * L_);
  d_status_.reserve(n);
  d_stats_.reserve(n * 4);
  d_w_.reserve(n);
  d_sites_.reserve((size_t)L_);
  d_chan_.reserve((size_t)L_);
  d_ids_.reserve(n);
  d_counts_.reserve(n * L_ * BATCH_MAX_JUMP);
  d_pair_.reserve((size_t)L_);
  d_pcounts_.reserve(n * L_ * BATCH_MAX_JUMP);
  d_disc_.reserve(n);
  d_spec_bonds_.reserve((size_t)L_);
  d_spec_fail_.reserve(n);
  chan_.assign((size_t)L_, BatchChanSite{BCH_NONE, 0, 0});
  chan_ops_.assign((size_t)L_, {});
  pair_.assign((size_t)L_, BatchChanSite{BCH_NONE, 0, 0});
  pair_ops_.assign((size_t)L_, {});
  d_fld_.reserve((size_t)L_);
  d_fdecay_.reserve((size_t)2 * L_);
  d_fxi_.reserve(n * L_);
  d_famp_.reserve(n * L_);
  fld_.assign((size_t)L_, BatchFieldSite{BFLD_NONE, 0, 0, 0, 0, 0, 0, 0.0});
  fld_vecs_.assign((size_t)L_, {});
  fld_evals_.assign((size_t)L_, {});
  fld_tabs_.assign((size_t)L_, {});
  fld_tau_.assign((size_t)L_, 0.0);
  HIP_CHECK(hipMemsetAsync(d_famp_, 0, n * L_ * sizeof(double), st_));
  reset_generator(0, nullptr);  // nothing is queued on the new stream: no wait; a batch without channels pays two small async operations
}

Batch::~Batch() {
  (void)hipSetDevice(device_);
  if (st_) (void)hipStreamSynchronize(st_);
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
  if (st_) (void)hipStreamDestroy(st_);
}  // the device arrays free themselves behind this, with nothing queued on them any more

// Brings every engine to the state a half-sweep in direction `forward` starts from, makes the block buffers of every
// bond exist, and rebuilds the device tables when a shape or a buffer moved since the last call.
void Batch::prepare(bool forward, bool build_envs) {
  const size_t n = eng_.size();
  const int begin = forward ? 0 : L_ - 1;
  // what depends on the engines' state is checked for ALL of them before any of them is touched
  for (size_t i = 0; i < n; ++i) {
    const Engine& e = *eng_[i];
    const std::string who = "batch: replica " + std::to_string(i) + ": ";
    if (e.center_ != begin) throw ArgError(who + "sweep must start at the centre (Psi) site");
    for (int p = 0; p < L_; ++p) {
      const int want = p < begin ? MITDVP_GAUGE_A : (p == begin ? MITDVP_GAUGE_PSI : MITDVP_GAUGE_B);
      if (e.gauge_[p] != want) throw ArgError(who + "the chain is not canonical around the centre site");
    }
  }
  for (size_t i = 0; i < n; ++i) {
    Engine& e = *eng_[i];
    e.require_ready();
    e.ss_check();
    if (L_ > 1 && build_envs) {
      if (forward) e.build_right_envs();
      else e.build_left_envs();
    }
    for (int b = 1; b < L_; ++b) {  // bond b is left of site b: blocks (dl[b], ml[b], dl[b])
      const size_t need = (size_t)shp_[b].dl * shp_[b].ml * shp_[b].dl;
      if (!e.envL_[b].p || e.envL_[b].n < need) { e.pool_put(std::move(e.envL_[b])); e.envL_[b] = e.pool_get(need); e.envL_ok_[b] = 0; }
      if (!e.envR_[b].p || e.envR_[b].n < need) { e.pool_put(std::move(e.envR_[b])); e.envR_[b] = e.pool_get(need); e.envR_ok_[b] = 0; }
    }
    e.ss_pull_kprev();
  }
  // scratch (grows only when the shapes or the number of replicas grew: the one other synchronisation)
  const size_t per = carve_ + (obs_plan_.total + 15) / 16 * 16;  // the sweep's carve, then the observation's
  reserve_synced(d_scratch_, per * n);
  // tables: [site L][envL L+1][envR L+1][w2l L][w2el L][w2er L][scratch 1] per replica
  const size_t ppr = ptrs_per_replica();
  std::vector<void*> h(n * ppr);
  std::vector<zc> shift(n);
  std::vector<int> kp(n * L_);
  for (size_t i = 0; i < n; ++i) {
    Engine& e = *eng_[i];
    void** q = h.data() + i * ppr;
    const Operator& o = e.ops_.find(0)->second;
    for (int p = 0; p < L_; ++p) q[p] = e.site_[p].p;
    for (int b = 0; b <= L_; ++b) { q[L_ + b] = e.envL_[b].p; q[2 * L_ + 1 + b] = e.envR_[b].p; }
    for (int p = 0; p < L_; ++p) {
      q[3 * L_ + 2 + p] = o.sites[p].w2l.p;
      q[4 * L_ + 2 + p] = o.sites[p].w2el.p;
      q[5 * L_ + 2 + p] = o.sites[p].w2er.p;
    }
    q[6 * L_ + 2] = d_scratch_ + i * per;
    shift[i] = make_double2(o.shift.real(), o.shift.imag());
    for (int p = 0; p < L_; ++p) kp[i * L_ + p] = e.kprev_[p];
  }
  if (h != h_ptrs_) {
    h_ptrs_ = h;
    HIP_CHECK(hipMemcpyAsync(d_ptrs_, h_ptrs_.data(), h_ptrs_.size() * sizeof(void*), hipMemcpyHostToDevice, st_));
  }
  if (shapes_dirty_) {
    HIP_CHECK(hipMemcpyAsync(d_shp_, shp_.data(), shp_.size() * sizeof(BatchShape), hipMemcpyHostToDevice, st_));
    shapes_dirty_ = false;
  }
  h_shift_ = shift;
  h_kprev_ = kp;
  HIP_CHECK(hipMemcpyAsync(d_shift_, h_shift_.data(), n * sizeof(zc), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(d_kprev_, h_kprev_.data(), h_kprev_.size() * sizeof(int), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemsetAsync(d_status_, 0, n * sizeof(int), st_));
  HIP_CHECK(hipMemsetAsync(d_stats_, 0, n * 4 * sizeof(long long), st_));
  // what the engines have queued on their own streams comes first
  for (size_t i = 0; i < n; ++i) {
    HIP_CHECK(hipEventRecord(ev_[i], eng_[i]->st_));
    HIP_CHECK(hipStreamWaitEvent(st_, ev_[i], 0));
  }
}

// improved relaxation: nhalf half-sweeps of k_batch_relax in one launch; energies / steps / history null: not recorded
void Batch::launch_relax(bool forward, int nhalf, double conv_tol, double* energies, int* steps, double* history, int hist_len) {
  Engine& e0 = *eng_[0];
  const size_t n = eng_.size();
  if (!d_rx_rst_total_.fits(n) || !d_rx_rst_most_.fits(n)) {  // once in the life of a batch
    reserve_synced(d_rx_rst_total_, n, d_rx_rst_most_, n);
    HIP_CHECK(hipMemsetAsync(d_rx_rst_total_, 0, n * sizeof(long long), st_));
    HIP_CHECK(hipMemsetAsync(d_rx_rst_most_, 0, n * sizeof(int), st_));
  }
  BatchRelaxArgs a{};
  a.L = L_;
  a.forward = forward ? 1 : 0;
  a.nhalf = nhalf;
  a.kcap = e0.max_diag_krylov_;
  a.max_restarts = rx_restarts_;
  a.thresh = e0.cfg.thresh;
  a.conv_tol = conv_tol;
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.shift = d_shift_;
  a.kprev = d_kprev_;
  a.status = d_status_;
  a.stats = d_stats_;
  a.total = d_rx_rst_total_;
  a.most = d_rx_rst_most_;
  a.plan = plan_;
  a.energy = energies;
  a.steps = steps;
  a.history = history;
  a.hist_len = hist_len;
  if (defl_count_ > 0) {  // the deflated instance of the same kernel: still one launch
    BatchDeflArgs d{};
    d.count = defl_count_;
    for (int k = 0; k < defl_count_; ++k) d.slot[k] = d_defl_slot_[k];
    d.snap_len = snap_len();
    d.w = d_defl_w_;
    d.plan = batch_deflate_plan(shp_.data(), L_, defl_count_);
    reserve_synced(d_defl_work_, n * d.plan.per);
    d.work = d_defl_work_;
    batch_relax_defl_launch(st_, a, d, (int)n);
  } else {
    batch_relax_launch(st_, a, (int)n);
  }
  n_launch_ += 1;
}

void Batch::launch(double dt, bool forward) {
  const size_t n = eng_.size();
  Engine& e0 = *eng_[0];
  if (e0.cfg.relax == 2) {  // dt means nothing to the eigen-solver, as in Engine::local_site_exp
    launch_relax(forward, 1, 0.0, nullptr, nullptr, nullptr, 0);
    return;
  }
  BatchArgs a{};
  a.L = L_;
  a.forward = forward ? 1 : 0;
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.shift = d_shift_;
  a.kprev = d_kprev_;
  a.status = d_status_;
  a.stats = d_stats_;
  a.plan = plan_;
  a.e = SmallExp{};
  a.e.integrator = e0.cfg.integrator; a.e.variant = e0.cfg.lanczos_variant; a.e.conserve_norm = e0.cfg.conserve_norm;
  a.e.max_krylov = e0.cfg.max_krylov; a.e.thresh = e0.cfg.thresh;
  const hzc ss = e0.scale_site(dt), sb = e0.scale_bond(dt);
  a.site_re = ss.real(); a.site_im = ss.imag(); a.bond_re = sb.real(); a.bond_im = sb.imag();
  batch_sweep_launch(st_, a, (int)n);
  n_launch_ += 1;
}

// after the launches of a call: statuses, Krylov memories, counters, and the engines' own bookkeeping
void Batch::finish(bool ends_forward, int half_sweeps, int* statuses, int other_launches, int channel_passes, int field_passes) {
  const size_t n = eng_.size();
  std::vector<int> st(n), kp(n * L_);
  std::vector<long long> stats(n * 4);
  HIP_CHECK(hipMemcpyAsync(st.data(), d_status_, n * sizeof(int), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(kp.data(), d_kprev_, kp.size() * sizeof(int), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(stats.data(), d_stats_, stats.size() * sizeof(long long), hipMemcpyDeviceToHost, st_));
  for (size_t i = 0; i < n; ++i) {  // the device copy of an engine's own one-launch exponentials, on the batch's stream
    Engine& e = *eng_[i];
    if (e.ss_.kprev && !e.exp_small_.empty())
      HIP_CHECK(hipMemcpyAsync(e.ss_.kprev, d_kprev_ + i * L_, (size_t)L_ * sizeof(int), hipMemcpyDeviceToDevice, st_));
  }
  HIP_CHECK(hipStreamSynchronize(st_));  // the one host wait of the call
  for (size_t i = 0; i < n; ++i) {
    Engine& e = *eng_[i];
    for (int p = 0; p < L_; ++p) e.kprev_[p] = kp[i * L_ + p];
    e.cnt_.n_heff += stats[i * 4 + 0];
    e.cnt_.n_keff += stats[i * 4 + 1];
    e.cnt_.heff_flops += (double)stats[i * 4 + 2];
    e.cnt_.keff_flops += (double)stats[i * 4 + 3];
    if (st[i] == SS_OK) {  // a replica that stopped part-way did less: only what the device counted is added for it
      e.cnt_.n_exp_site += (long long)half_sweeps * L_;
      if (e.cfg.relax != 2) e.cnt_.n_exp_bond += (long long)half_sweeps * (L_ - 1);  // improved relaxation has no bond step
      e.cnt_.n_qr += (long long)half_sweeps * (L_ - 1);
      e.cnt_.n_env += (long long)half_sweeps * (L_ - 1);
      if (channel_passes) {  // a channel pass: two gauge moves and one left block per site above the lowest channel
        e.cnt_.n_qr += (long long)channel_passes * 2 * (L_ - 1 - chan_lo_);
        e.cnt_.n_env += (long long)channel_passes * (L_ - 1 - chan_lo_);
      }
      if (field_passes) e.cnt_.n_env += (long long)field_passes * (L_ - 1 - fld_lo_);  // a field pass: left blocks only
    }
    if (i == 0) e.cnt_.n_launch += half_sweeps + other_launches + channel_passes + field_passes;  // the batch's launches are counted once
    const int centre = ends_forward ? L_ - 1 : 0;
    for (int p = 0; p < L_; ++p) e.gauge_[p] = p < centre ? MITDVP_GAUGE_A : (p == centre ? MITDVP_GAUGE_PSI : MITDVP_GAUGE_B);
    e.center_ = centre;
    for (int b = 1; b < L_; ++b) {
      e.envL_ok_[b] = ends_forward ? 1 : 0;
      e.envR_ok_[b] = ends_forward ? 0 : 1;
    }
    (void)e.take_env_checked();  // the blocks its sets described are gone
    if (st[i] != SS_OK) {  // the replica stopped in the middle of a half-sweep: its chain must be set up again
      for (int b = 1; b < L_; ++b) { e.envL_ok_[b] = 0; e.envR_ok_[b] = 0; }
      for (int p = 0; p < L_; ++p) e.gauge_[p] = MITDVP_GAUGE_C;
      e.center_ = -1;
    }
    if (statuses) statuses[i] = st[i];
  }
}

void Batch::step(double dt, int nsteps, int* statuses) {
  if (nsteps < 0) throw ArgError("batch: nsteps must be >= 0");
  HIP_CHECK(hipSetDevice(device_));
  validate();
  if (nsteps == 0) {
    for (size_t i = 0; statuses && i < eng_.size(); ++i) statuses[i] = SS_OK;
    return;
  }
  check_channels();
  check_fields();
  prepare(true);
  const bool chan = has_channels();  // without a channel: the two launches per step of before, nothing else
  const bool fld = has_fields();     // nor without a field
  if (chan) upload_channels();
  if (fld) upload_fields(dt);
  for (int s = 0; s < nsteps; ++s) {
    launch(dt, true);
    if (fld) launch_field(dt, steps_done_ + s, field_clock_ + s);
    if (chan) launch_channel(steps_done_ + s);
    launch(dt, false);
  }
  steps_done_ += nsteps;
  field_clock_ += nsteps;
  finish(false, nsteps * 2, statuses, 0, chan ? nsteps : 0, fld ? nsteps : 0);
}

void Batch::sweep(double dt, bool forward, int* statuses) {
  HIP_CHECK(hipSetDevice(device_));
  validate();
  if (has_channels())
    throw ArgError("batch: a single half-sweep is refused while channels are set (site " + std::to_string(chan_lo_) +
                   (chan_[chan_lo_].kind != BCH_NONE ? " carries one" : " is the lower end of a pair channel") +
                   "): they act between the two half-sweeps of a time step");
  if (has_fields())
    throw ArgError("batch: a single half-sweep is refused while fields are set (site " + std::to_string(fld_lo_) +
                   " carries one): they act between the two half-sweeps of a time step");
  prepare(forward);
  launch(dt, forward);
  finish(L_ > 1 ? forward : false, 1, statuses);
}

// ---- one-site channels between the half-sweeps (k_batch_channel) ----
void Batch::set_channel(int site, int kind, const double* ops_reim, int nops, int d) {
  HIP_CHECK(hipSetDevice(device_));
  validate();
  if (site < 0 || site >= L_) throw ArgError("batch: channel site " + std::to_string(site) + " is out of range (the chain has " + std::to_string(L_) + " sites)");
  const std::string at = "batch: channel on site " + std::to_string(site) + ": ";
  if (ops_reim) {
    if (kind != BCH_GATE && kind != BCH_JUMP) throw ArgError(at + "kind must be MITDVP_CHANNEL_GATE or MITDVP_CHANNEL_JUMP");
    if (kind == BCH_GATE && nops != 1) throw ArgError(at + "a gate is one matrix (got " + std::to_string(nops) + ")");
    if (kind == BCH_JUMP && (nops < 2 || nops > BATCH_MAX_JUMP))
      throw ArgError(at + "a jump channel has 2 to " + std::to_string(BATCH_MAX_JUMP) + " operators (got " + std::to_string(nops) + ")");
    if (d != shp_[site].d)
      throw ArgError(at + "the operators are " + std::to_string(d) + " x " + std::to_string(d) + ", the site's physical dimension is " +
                     std::to_string(shp_[site].d));
    if (eng_[0]->cfg.relax != 0) throw ArgError(at + "channels do not go with imaginary time (relax must be 0)");
    const size_t ne = (size_t)nops * d * d;
    std::vector<zc> ops(ne);
    for (size_t e = 0; e < ne; ++e) ops[e] = make_double2(ops_reim[2 * e], ops_reim[2 * e + 1]);
    chan_ops_[site] = std::move(ops);
    chan_[site] = BatchChanSite{kind, nops, 0};
  } else {
    chan_ops_[site].clear();
    chan_[site] = BatchChanSite{BCH_NONE, 0, 0};
  }
  channels_changed();
}

void Batch::channels_changed() {
  chan_lo_ = -1;
  npair_ = 0;
  for (int p = L_ - 1; p >= 0; --p) {
    if (chan_[p].kind != BCH_NONE || pair_[p].kind != BCH_NONE) chan_lo_ = p;  // a pair on (p, p + 1) touches p
    if (pair_[p].kind != BCH_NONE) npair_ += 1;
  }
  chan_dirty_ = true;
  HIP_CHECK(hipMemsetAsync(d_disc_, 0, eng_.size() * sizeof(double), st_));
}

void Batch::set_pair_channel(int site, int kind, const double* ops_reim, int nops, int d0, int d1) {
  HIP_CHECK(hipSetDevice(device_));
  validate();
  if (site < 0 || site + 1 >= L_ || ops_reim) {  // removing a channel needs a bond in range, setting one the whole envelope
    std::string why;
    if (!batch_pair_fits(shp_.data(), L_, plan_, site, why)) throw ArgError(why);
  }
  const std::string at = "batch: pair channel on bond (" + std::to_string(site) + ", " + std::to_string(site + 1) + "): ";
  if (ops_reim) {
    if (kind != BCH_GATE && kind != BCH_JUMP) throw ArgError(at + "kind must be MITDVP_CHANNEL_GATE or MITDVP_CHANNEL_JUMP");
    if (kind == BCH_GATE && nops != 1) throw ArgError(at + "a gate is one matrix (got " + std::to_string(nops) + ")");
    if (kind == BCH_JUMP && (nops < 2 || nops > BATCH_MAX_JUMP))
      throw ArgError(at + "a jump channel has 2 to " + std::to_string(BATCH_MAX_JUMP) + " operators (got " + std::to_string(nops) + ")");
    if (d0 != shp_[site].d || d1 != shp_[site + 1].d)
      throw ArgError(at + "the operators act on dimensions " + std::to_string(d0) + " x " + std::to_string(d1) + " (matrices of order " +
                     std::to_string((long)d0 * d1) + "), the sites' physical dimensions are " + std::to_string(shp_[site].d) + " x " +
                     std::to_string(shp_[site + 1].d) + " (order " + std::to_string((long)shp_[site].d * shp_[site + 1].d) + ")");
    if (eng_[0]->cfg.relax != 0) throw ArgError(at + "channels do not go with imaginary time (relax must be 0)");
    const size_t dd = (size_t)d0 * d1, ne = (size_t)nops * dd * dd;
    std::vector<zc> ops(ne);
    for (size_t e = 0; e < ne; ++e) ops[e] = make_double2(ops_reim[2 * e], ops_reim[2 * e + 1]);
    pair_ops_[site] = std::move(ops);
    pair_[site] = BatchChanSite{kind, nops, 0};
  } else {
    pair_ops_[site].clear();
    pair_[site] = BatchChanSite{BCH_NONE, 0, 0};
  }
  channels_changed();
}

// what may have changed on the engines since the channels were set (validate() has just refreshed shp_)
void Batch::check_channels() const {
  if (!has_channels()) return;
  if (eng_[0]->cfg.relax != 0) throw ArgError("batch: channels do not go with imaginary time (relax must be 0)");
  for (int p = 0; p < L_; ++p)
    if (chan_[p].kind != BCH_NONE && chan_ops_[p].size() != (size_t)chan_[p].nops * shp_[p].d * shp_[p].d)
      throw ArgError("batch: channel on site " + std::to_string(p) + ": the operators no longer match the site's physical dimension " +
                     std::to_string(shp_[p].d));
  for (int q = 0; q + 1 < L_; ++q) {
    if (pair_[q].kind == BCH_NONE) continue;
    std::string why;
    if (!batch_pair_fits(shp_.data(), L_, plan_, q, why)) throw ArgError(why);
    const size_t dd = (size_t)shp_[q].d * shp_[q + 1].d;
    if (pair_ops_[q].size() != (size_t)pair_[q].nops * dd * dd)
      throw ArgError("batch: pair channel on bond (" + std::to_string(q) + ", " + std::to_string(q + 1) +
                     "): the operators no longer match the sites' physical dimensions " + std::to_string(shp_[q].d) + " x " +
                     std::to_string(shp_[q + 1].d));
  }
}

void Batch::upload_channels() {
  if (!chan_dirty_) return;
  h_chan_ = chan_;
  h_ops_.clear();
  for (int p = 0; p < L_; ++p) {
    h_chan_[p].off = (long long)h_ops_.size();
    h_ops_.insert(h_ops_.end(), chan_ops_[p].begin(), chan_ops_[p].end());
  }
  h_pair_ = pair_;
  for (int q = 0; q < L_; ++q) {
    h_pair_[q].off = (long long)h_ops_.size();
    h_ops_.insert(h_ops_.end(), pair_ops_[q].begin(), pair_ops_[q].end());
  }
  reserve_synced(d_ops_, h_ops_.size());
  HIP_CHECK(hipMemcpyAsync(d_chan_, h_chan_.data(), h_chan_.size() * sizeof(BatchChanSite), hipMemcpyHostToDevice, st_));
  if (npair_) HIP_CHECK(hipMemcpyAsync(d_pair_, h_pair_.data(), h_pair_.size() * sizeof(BatchChanSite), hipMemcpyHostToDevice, st_));
  if (!h_ops_.empty()) HIP_CHECK(hipMemcpyAsync(d_ops_, h_ops_.data(), h_ops_.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
  chan_dirty_ = false;
}

void Batch::launch_channel(long long step) {
  BatchChanArgs a{};
  a.L = L_;
  a.lo = chan_lo_;
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.status = d_status_;
  a.plan = plan_;
  a.chan = d_chan_;
  a.ops = d_ops_;
  a.seed = seed_;
  a.step = step;
  a.ids = d_ids_;
  a.counts = d_counts_;
  if (npair_) {  // the walk with pair channels is a kernel of its own; without one k_batch_channel runs as before
    BatchPairArgs pa{};
    pa.c = a;
    pa.pair = d_pair_;
    pa.pcounts = d_pcounts_;
    pa.disc = d_disc_;
    batch_pair_launch(st_, pa, (int)eng_.size());
  } else {
    batch_channel_launch(st_, a, (int)eng_.size());
  }
  n_launch_ += 1;
}

// ---- time-dependent one-site fields between the half-sweeps (k_batch_field) ----
void Batch::set_field(int site, int d, const double* vecs_reim, const double* evals, int kind, const double* table, int ntab,
                      int per_replica, double sigma, double tau) {
  HIP_CHECK(hipSetDevice(device_));
  validate();
  if (site < 0 || site >= L_) throw ArgError("batch: field site " + std::to_string(site) + " is out of range (the chain has " + std::to_string(L_) + " sites)");
  const std::string at = "batch: field on site " + std::to_string(site) + ": ";
  const size_t n = eng_.size();
  if (vecs_reim) {
    if (kind != BFLD_TABLE && kind != BFLD_OU) throw ArgError(at + "kind must be MITDVP_FIELD_TABLE or MITDVP_FIELD_OU");
    if (d != shp_[site].d)
      throw ArgError(at + "the generator is " + std::to_string(d) + " x " + std::to_string(d) + ", the site's physical dimension is " +
                     std::to_string(shp_[site].d));
    if (d > BATCH_FIELD_MAX_D)
      throw ArgError(at + "the physical dimension is " + std::to_string(d) + ", a field takes at most " + std::to_string(BATCH_FIELD_MAX_D));
    if (!evals) throw ArgError(at + "null eigenvalues");
    if (kind == BFLD_TABLE && (ntab < 1 || !table))
      throw ArgError(at + "a table field takes a table of at least 1 entry (got " + (table ? std::to_string(ntab) + " entries" : std::string("a null table")) + ")");
    if (kind == BFLD_OU && (!std::isfinite(sigma) || sigma < 0.0 || !std::isfinite(tau) || tau < 0.0))
      throw ArgError(at + "sigma and tau must be finite and >= 0 (got " + std::to_string(sigma) + ", " + std::to_string(tau) + ")");
    if (eng_[0]->cfg.relax != 0) throw ArgError(at + "fields do not go with imaginary time (relax must be 0)");
    std::vector<zc> v((size_t)d * d);
    for (size_t e = 0; e < v.size(); ++e) v[e] = make_double2(vecs_reim[2 * e], vecs_reim[2 * e + 1]);
    fld_vecs_[site] = std::move(v);
    fld_evals_[site].assign(evals, evals + d);
    BatchFieldSite f{kind, d, 0, 0, 0, 0, 0, 0.0};
    if (kind == BFLD_TABLE) {
      f.ntab = ntab;
      f.per_replica = per_replica ? 1 : 0;
      fld_tabs_[site].assign(table, table + (size_t)ntab * (per_replica ? n : 1));
      fld_tau_[site] = 0.0;
    } else {
      f.sigma = sigma;
      fld_tabs_[site].clear();
      fld_tau_[site] = tau;
    }
    fld_[site] = f;
  } else {
    fld_vecs_[site].clear();
    fld_evals_[site].clear();
    fld_tabs_[site].clear();
    fld_tau_[site] = 0.0;
    fld_[site] = BatchFieldSite{BFLD_NONE, 0, 0, 0, 0, 0, 0, 0.0};
  }
  fld_lo_ = -1;
  for (int p = L_ - 1; p >= 0; --p)
    if (fld_[p].kind != BFLD_NONE) fld_lo_ = p;
  fld_dirty_ = true;
  fld_decay_set_ = false;
  field_clock_ = 0;  // any call: the tables start again and the noise of all sites is drawn afresh
  HIP_CHECK(hipMemsetAsync(d_fxi_, 0, n * L_ * sizeof(double), st_));
  HIP_CHECK(hipMemsetAsync(d_famp_, 0, n * L_ * sizeof(double), st_));
}

void Batch::field_values(double* out) {
  if (!out) throw ArgError("batch: null destination for the field amplitudes");
  HIP_CHECK(hipSetDevice(device_));
  HIP_CHECK(hipMemcpyAsync(out, d_famp_, eng_.size() * L_ * sizeof(double), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}

// what may have changed on the engines since the fields were set (validate() has just refreshed shp_)
void Batch::check_fields() const {
  if (!has_fields()) return;
  if (eng_[0]->cfg.relax != 0) throw ArgError("batch: fields do not go with imaginary time (relax must be 0)");
  for (int p = 0; p < L_; ++p)
    if (fld_[p].kind != BFLD_NONE && fld_[p].d != shp_[p].d)
      throw ArgError("batch: field on site " + std::to_string(p) + ": the generator no longer matches the site's physical dimension " +
                     std::to_string(shp_[p].d));
}

// the device images of the fields, and the Ornstein-Uhlenbeck coefficients of this call's dt
void Batch::upload_fields(double dt) {
  if (fld_dirty_) {
    h_fld_ = fld_;
    h_fvecs_.clear();
    h_fevals_.clear();
    h_ftabs_.clear();
    for (int p = 0; p < L_; ++p) {
      h_fld_[p].off_v = (long long)h_fvecs_.size();
      h_fld_[p].off_g = (long long)h_fevals_.size();
      h_fld_[p].off_t = (long long)h_ftabs_.size();
      h_fvecs_.insert(h_fvecs_.end(), fld_vecs_[p].begin(), fld_vecs_[p].end());
      h_fevals_.insert(h_fevals_.end(), fld_evals_[p].begin(), fld_evals_[p].end());
      h_ftabs_.insert(h_ftabs_.end(), fld_tabs_[p].begin(), fld_tabs_[p].end());
    }
    reserve_synced(d_fvecs_, h_fvecs_.size(), d_fevals_, h_fevals_.size(), d_ftabs_, h_ftabs_.size());
    HIP_CHECK(hipMemcpyAsync(d_fld_, h_fld_.data(), h_fld_.size() * sizeof(BatchFieldSite), hipMemcpyHostToDevice, st_));
    if (!h_fvecs_.empty()) HIP_CHECK(hipMemcpyAsync(d_fvecs_, h_fvecs_.data(), h_fvecs_.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
    if (!h_fevals_.empty()) HIP_CHECK(hipMemcpyAsync(d_fevals_, h_fevals_.data(), h_fevals_.size() * sizeof(double), hipMemcpyHostToDevice, st_));
    if (!h_ftabs_.empty()) HIP_CHECK(hipMemcpyAsync(d_ftabs_, h_ftabs_.data(), h_ftabs_.size() * sizeof(double), hipMemcpyHostToDevice, st_));
    fld_dirty_ = false;
  }
  if (!fld_decay_set_ || dt != fld_decay_dt_) {  // a = exp(-|dt| / tau) (tau = 0: 0, white noise) and sigma sqrt(1 - a^2)
    h_fdecay_.assign((size_t)2 * L_, 0.0);
    for (int p = 0; p < L_; ++p) {
      if (fld_[p].kind != BFLD_OU) continue;
      const double a = fld_tau_[p] > 0.0 ? std::exp(-std::fabs(dt) / fld_tau_[p]) : 0.0;
      h_fdecay_[2 * p] = a;
      h_fdecay_[2 * p + 1] = fld_[p].sigma * std::sqrt(1.0 - a * a);
    }
    HIP_CHECK(hipMemcpyAsync(d_fdecay_, h_fdecay_.data(), h_fdecay_.size() * sizeof(double), hipMemcpyHostToDevice, st_));
    fld_decay_set_ = true;
    fld_decay_dt_ = dt;
  }
}

void Batch::launch_field(double dt, long long step, long long clock) {
  BatchFieldArgs a{};
  a.L = L_;
  a.lo = fld_lo_;
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.status = d_status_;
  a.plan = plan_;
  a.fld = d_fld_;
  a.vecs = d_fvecs_;
  a.evals = d_fevals_;
  a.tables = d_ftabs_;
  a.decay = d_fdecay_;
  a.dt = dt;
  a.seed = seed_;
  a.step = step;
  a.clock = clock;
  a.ids = d_ids_;
  a.xi = d_fxi_;
  a.amp = d_famp_;
  batch_field_launch(st_, a, (int)eng_.size());
  n_launch_ += 1;
}

void Batch::set_seed(unsigned long long seed, const unsigned long long* ids) {
  HIP_CHECK(hipSetDevice(device_));
  HIP_CHECK(hipStreamSynchronize(st_));  // h_ids_ may still be the source of an earlier copy
  reset_generator(seed, ids);
}

void Batch::reset_generator(unsigned long long seed, const unsigned long long* ids) {
  const size_t n = eng_.size();
  seed_ = seed;
  steps_done_ = 0;
  field_clock_ = 0;  // the noise of the fields is drawn afresh, their tables start again
  h_ids_.resize(n);
  for (size_t i = 0; i < n; ++i) h_ids_[i] = ids ? ids[i] : (unsigned long long)i;
  HIP_CHECK(hipMemcpyAsync(d_ids_, h_ids_.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemsetAsync(d_counts_, 0, n * L_ * BATCH_MAX_JUMP * sizeof(long long), st_));
  HIP_CHECK(hipMemsetAsync(d_pcounts_, 0, n * L_ * BATCH_MAX_JUMP * sizeof(long long), st_));
  HIP_CHECK(hipMemsetAsync(d_disc_, 0, n * sizeof(double), st_));
}

void Batch::jump_counts(long long* counts) {
  if (!counts) throw ArgError("batch: null destination for the jump counters");
  HIP_CHECK(hipSetDevice(device_));
  HIP_CHECK(hipMemcpyAsync(counts, d_counts_, eng_.size() * L_ * BATCH_MAX_JUMP * sizeof(long long), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}

void Batch::pair_jump_counts(long long* counts) {
  if (!counts) throw ArgError("batch: null destination for the pair jump counters");
  HIP_CHECK(hipSetDevice(device_));
  HIP_CHECK(hipMemcpyAsync(counts, d_pcounts_, eng_.size() * L_ * BATCH_MAX_JUMP * sizeof(long long), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}

void Batch::discarded_weight(double* out) {
  if (!out) throw ArgError("batch: null destination for the discarded weights");
  HIP_CHECK(hipSetDevice(device_));
  HIP_CHECK(hipMemcpyAsync(out, d_disc_, eng_.size() * sizeof(double), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}

// ---- observables (k_batch_observe, k_batch_mean) ----
long Batch::observe_sizes(const int* sites, int nsites, int what, bool with_keys) {
  validate();
  if ((!(what & BOBS_ALL) && !(with_keys && what == 0)) || (what & ~BOBS_ALL)) throw ArgError("batch: nothing to observe (what must be a non-empty set of MITDVP_OBS_* bits)");
  if (nsites < 0 || (nsites > 0 && !sites)) throw ArgError("batch: bad list of observed sites");
  if (((what & BOBS_RDM) != 0) != (nsites > 0)) throw ArgError("batch: MITDVP_OBS_RDM and a non-empty list of sites go together");
  long nrdm = 0;
  for (int k = 0; k < nsites; ++k) {
    if (sites[k] < 0 || sites[k] >= L_) throw ArgError("batch: observed site " + std::to_string(sites[k]) + " is out of range");
    if (k > 0 && sites[k] <= sites[k - 1]) throw ArgError("batch: the observed sites must be strictly ascending");
    nrdm += (long)shp_[sites[k]].d * shp_[sites[k]].d;
    if (nrdm > BATCH_OBS_MAX_RDM)
      throw ArgError("batch: the observed site RDMs have more than " + std::to_string(BATCH_OBS_MAX_RDM) + " elements per replica");
  }
  return nrdm;
}

long Batch::density_sizes(const int* legs, int nkeys, long nrdm) {
  std::string why;
  if (!batch_density_plan(shp_.data(), L_, legs, nkeys, nrdm, dens_plan_, why)) throw ArgError(why);
  return dens_plan_.ndens;
}

void Batch::launch_density(int nkeys, bool zero_head, long record, long rec_len, long dens_off) {
  BatchDensArgs a{};
  a.L = L_;
  a.nkeys = nkeys;
  a.zero_head = zero_head ? 1 : 0;
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.status = d_status_;
  a.legs = d_legs_;
  a.carve = carve_;
  a.plan = obs_plan_;
  a.tbuf = d_tbuf_;
  a.need = dens_plan_.need;
  a.rec = d_rec_ + (size_t)record * eng_.size() * rec_len;
  a.rec_len = rec_len;
  a.dens_off = dens_off;
  batch_density_launch(st_, a, (int)eng_.size());
  n_launch_ += 1;
}

void Batch::launch_observe(int what, int nsites, long record, long rec_len) {
  BatchObsArgs a{};
  a.L = L_;
  a.what = what;
  a.nsites = nsites;
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.shift = d_shift_;
  a.status = d_status_;
  a.sites = d_sites_;
  a.carve = carve_;
  a.plan = obs_plan_;
  a.rec = d_rec_ + (size_t)record * eng_.size() * rec_len;
  a.rec_len = rec_len;
  batch_observe_launch(st_, a, (int)eng_.size());
  n_launch_ += 1;
}

// the end of a call that only observed: the one host wait; the engines keep their bookkeeping as it is
void Batch::finish_observe(int launches, int* statuses) {
  HIP_CHECK(hipStreamSynchronize(st_));
  eng_[0]->cnt_.n_launch += launches;
  for (size_t i = 0; statuses && i < eng_.size(); ++i) statuses[i] = SS_OK;
}

void Batch::run(double dt, int nsteps, int every, const int* sites, int nsites, int what, const double* weights, const ObsOut& out,
                int* statuses, const DensOut& dens) {
  if (nsteps < 0) throw ArgError("batch: nsteps must be >= 0");
  if (every < 1) throw ArgError("batch: every must be >= 1");
  if (nsteps % every != 0) throw ArgError("batch: nsteps must be a multiple of every");
  HIP_CHECK(hipSetDevice(device_));
  const int nkeys = dens.nkeys;
  const bool cx = has_cross();  // a cross request rides on every record; it may be all that is recorded
  const bool sp = has_spectra();  // so does a spectra request
  const bool sm = has_samples();  // and a samples request
  const bool ex = has_expect();   // and an expect request
  const bool xm = has_cross_mpo();  // and a cross request of MPOs
  const long nrdm = observe_sizes(sites, nsites, what, nkeys > 0 || cx || sp || sm || ex || xm);
  const long ndens = density_sizes(dens.legs, nkeys, nrdm);
  if (cx) check_cross("mitdvp_batch_run");
  if (sp) check_spectra("mitdvp_batch_run");
  if (sm) check_samples("mitdvp_batch_run");
  if (ex) check_expect("mitdvp_batch_run");
  if (xm) check_cross_mpo("mitdvp_batch_run");
  const bool own = what != 0 || nkeys > 0;  // false: only the cross request is recorded, no record of the replicas
  const size_t n = eng_.size();
  const long nrec = nsteps / every + 1, dens_off = BOBS_HEAD + 2 * nrdm, rec_len = dens_off + 2 * ndens;
  const int per_rec = (what ? 1 : 0) + (nkeys ? 1 : 0);  // launches per record
  const bool chan = has_channels() && nsteps > 0;
  if (chan) check_channels();
  const bool fld = has_fields() && nsteps > 0;
  if (fld) check_fields();
  prepare(true, nsteps > 0 || (what & BOBS_ENERGY));
  if (chan) upload_channels();
  if (fld) upload_fields(dt);
  // nothing refuses from here on: the run replaces the records of the last one, so their buffers may now grow
  if (cx) { cross_rec_.drop(); upload_cross(nrec); }
  if (sp) { spec_rec_.drop(); upload_spectra(nrec); }
  if (sm) { smp_rec_.drop(); upload_samples(nrec); }
  if (ex) { exp_rec_.drop(); upload_expect(nrec); }
  if (xm) { xm_rec_.drop(); upload_cross_mpo(nrec); }
  // buffers of the records and their means (grow only), the site list and the weights
  const size_t need_rec = (size_t)nrec * n * rec_len, need_mean = (size_t)nrec * rec_len;
  const size_t need_legs = (size_t)nkeys * L_, need_tbuf = nkeys ? n * 2 * dens_plan_.need : 0;
  reserve_synced(d_legs_, need_legs, d_tbuf_, need_tbuf, d_rec_, need_rec, d_mean_, need_mean);
  h_sites_.assign(sites, sites + nsites);
  h_w_.assign(n, 1.0 / (double)n);
  if (weights) h_w_.assign(weights, weights + n);
  if (nsites) HIP_CHECK(hipMemcpyAsync(d_sites_, h_sites_.data(), (size_t)nsites * sizeof(int), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(d_w_, h_w_.data(), n * sizeof(double), hipMemcpyHostToDevice, st_));
  if (nkeys) {
    h_legs_.assign(dens.legs, dens.legs + need_legs);
    HIP_CHECK(hipMemcpyAsync(d_legs_, h_legs_.data(), need_legs * sizeof(int), hipMemcpyHostToDevice, st_));
  }
  auto record = [&](long q, long long step) {
    if (what) launch_observe(what, nsites, q, rec_len);
    if (nkeys) launch_density(nkeys, what == 0, q, rec_len, dens_off);
    if (cx) launch_cross(q);
    if (sp) launch_spectra(q);
    if (sm) launch_samples(q, step);
    if (ex) launch_expect(q);
    if (xm) launch_cross_mpo(q);
  };

  record(0, steps_done_);
  for (int s = 0; s < nsteps; ++s) {
    launch(dt, true);
    if (fld) launch_field(dt, steps_done_ + s, field_clock_ + s);
    if (chan) launch_channel(steps_done_ + s);
    launch(dt, false);
    if ((s + 1) % every == 0) record((s + 1) / every, steps_done_ + s + 1);
  }
  if (own) {
    batch_mean_launch(st_, d_rec_, d_w_, d_mean_, (int)n, rec_len, nrec);
    n_launch_ += 1;
  }
  const bool per_replica = own && (out.norm || out.autocorr || out.energy || out.rdm || dens.density);
  h_mean_.assign(need_mean, 0.0);
  if (own) HIP_CHECK(hipMemcpyAsync(h_mean_.data(), d_mean_, need_mean * sizeof(double), hipMemcpyDeviceToHost, st_));
  // every request that is set: ONE k_batch_mean over its records (weights 1 / rows); they and their means come back with
  // the rest and are the request's records from here on
  auto end_run = [&](RecordStore& s) {
    s.mean_of_run(st_, nrec, n_launch_);
    s.fetch_run(st_);
  };
  if (cx) end_run(cross_rec_);
  if (sp) {
    end_run(spec_rec_);
    HIP_CHECK(hipMemcpyAsync(h_spec_fail_.data(), d_spec_fail_, n * sizeof(int), hipMemcpyDeviceToHost, st_));
  }
  if (sm) {  // the frequencies are what is averaged; configurations and probabilities are copied beside them
    smp_rec_.mean_of_run(st_, nrec, n_launch_);
    h_smp_cfg_.resize(smp_cfg_lay(nrec).rec_now());
    h_smp_prob_.resize(smp_prob_lay(nrec).rec_now());
    HIP_CHECK(hipMemcpyAsync(h_smp_cfg_.data(), d_smp_cfg_, h_smp_cfg_.size() * sizeof(int), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(h_smp_prob_.data(), d_smp_prob_, h_smp_prob_.size() * sizeof(double), hipMemcpyDeviceToHost, st_));
    smp_rec_.fetch_run(st_);
  }
  if (ex) end_run(exp_rec_);
  if (xm) end_run(xm_rec_);
  if (per_replica) {
    h_rec_.resize(need_rec);
    HIP_CHECK(hipMemcpyAsync(h_rec_.data(), d_rec_, need_rec * sizeof(double), hipMemcpyDeviceToHost, st_));
  }
  steps_done_ += nsteps;
  field_clock_ += nsteps;
  const int nreq = (int)cx + (int)sp + (int)sm + (int)ex + (int)xm;  // each: its kernel per record and ONE k_batch_mean
  const int other = (int)nrec * per_rec + (own ? 1 : 0) + nreq * ((int)nrec + 1);
  if (nsteps > 0) finish(false, nsteps * 2, statuses, other, chan ? nsteps : 0, fld ? nsteps : 0);
  else finish_observe(other, statuses);

  for (long q = 0; q < nrec; ++q) {
    const double* m = h_mean_.data() + (size_t)q * rec_len;
    if (out.mean_norm2) out.mean_norm2[q] = m[0];
    if (out.mean_autocorr) { out.mean_autocorr[2 * q] = m[2]; out.mean_autocorr[2 * q + 1] = m[3]; }
    if (out.mean_energy) { out.mean_energy[2 * q] = m[4]; out.mean_energy[2 * q + 1] = m[5]; }
    if (out.mean_rdm && nrdm) std::memcpy(out.mean_rdm + (size_t)q * 2 * nrdm, m + BOBS_HEAD, (size_t)2 * nrdm * sizeof(double));
    if (dens.mean_density && ndens) std::memcpy(dens.mean_density + (size_t)q * 2 * ndens, m + dens_off, (size_t)2 * ndens * sizeof(double));
    for (size_t i = 0; per_replica && i < n; ++i) {
      const double* r = h_rec_.data() + ((size_t)q * n + i) * rec_len;
      const size_t at = (size_t)q * n + i;
      if (out.norm) out.norm[at] = std::sqrt(r[0]);
      if (out.autocorr) { out.autocorr[2 * at] = r[2]; out.autocorr[2 * at + 1] = r[3]; }
      if (out.energy) { out.energy[2 * at] = r[4]; out.energy[2 * at + 1] = r[5]; }
      if (out.rdm && nrdm) std::memcpy(out.rdm + at * 2 * nrdm, r + BOBS_HEAD, (size_t)2 * nrdm * sizeof(double));
      if (dens.density && ndens) std::memcpy(dens.density + at * 2 * ndens, r + dens_off, (size_t)2 * ndens * sizeof(double));
    }
  }
  if (sp) spectra_failed("mitdvp_batch_run");
}

// ---- cross overlaps and one-site matrix elements between replicas (k_batch_cross, k_batch_snapshot) ----
size_t Batch::snap_len() const {
  size_t len = 0;
  for (const BatchShape& s : shp_) len += (size_t)s.dl * s.d * s.dr;
  return len;
}

void Batch::prepare_observing() {
  const bool at_end = L_ > 1 && eng_[0]->center_ == L_ - 1;  // where a forward half-sweep leaves the centre
  prepare(!at_end, false);
}

void Batch::snapshot() {
  HIP_CHECK(hipSetDevice(device_));
  validate();
  prepare_observing();
  const size_t need = eng_.size() * snap_len();
  reserve_synced(d_snap_, need);
  batch_snapshot_launch(st_, d_shp_, d_ptrs_, (int)ptrs_per_replica(), d_snap_, snap_len(), L_, (int)eng_.size());
  n_launch_ += 1;
  finish_observe(1, nullptr);
  has_snap_ = true;
}

void Batch::set_cross(int npairs, const int* bra, const int* ket, const int* site, const double* ops_reim, const int* op_dims) {
  const std::string at = "mitdvp_batch_set_cross: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  const int B = (int)eng_.size();
  if (npairs < 0) throw ArgError(at + "npairs must be >= 0");
  if (npairs > BATCH_CROSS_MAX_PAIRS)
    throw ArgError(at + std::to_string(npairs) + " pairs, a request takes at most " + std::to_string(BATCH_CROSS_MAX_PAIRS));
  if (npairs > 0 && (!bra || !ket || !site)) throw ArgError(at + "null list of bra, ket or site indices");
  std::vector<BatchCrossPair> pairs((size_t)npairs);
  std::vector<zc> ops;
  int nop = 0;
  for (int q = 0; q < npairs; ++q) {
    const std::string who = at + "pair " + std::to_string(q) + ": ";
    const int idx[2] = {bra[q], ket[q]};
    for (int k = 0; k < 2; ++k) {
      const std::string name = std::string(k ? "ket" : "bra") + " index " + std::to_string(idx[k]);
      if (idx[k] < 0 || idx[k] >= 2 * B)
        throw ArgError(who + name + " is outside 0 .. " + std::to_string(2 * B - 1) + " (the batch has " + std::to_string(B) +
                       " replicas; " + std::to_string(B) + " + r names the snapshot of replica r)");
      if (idx[k] >= B && !has_snap_)
        throw ArgError(who + name + " names the snapshot of replica " + std::to_string(idx[k] - B) +
                       ", and no snapshot was taken yet (mitdvp_batch_snapshot)");
    }
    if (site[q] < -1 || site[q] >= L_)
      throw ArgError(who + "site " + std::to_string(site[q]) + " is out of range (-1: the plain overlap, or 0 .. " + std::to_string(L_ - 1) + ")");
    pairs[q] = BatchCrossPair{bra[q], ket[q], site[q], 0, 0};
    if (site[q] < 0) continue;
    if (!ops_reim || !op_dims) throw ArgError(who + "it has an operator on site " + std::to_string(site[q]) + ", and ops_reim or op_dims is null");
    const int d = op_dims[nop++];
    if (d != shp_[site[q]].d)
      throw ArgError(who + "the operator is " + std::to_string(d) + " x " + std::to_string(d) + ", the physical dimension of site " +
                     std::to_string(site[q]) + " is " + std::to_string(shp_[site[q]].d));
    pairs[q].off = (long long)ops.size();
    const size_t ne = (size_t)d * d;
    for (size_t e = 0; e < ne; ++e) ops.push_back(make_double2(ops_reim[2 * e], ops_reim[2 * e + 1]));
    ops_reim += 2 * ne;
  }
  cross_ = std::move(pairs);
  cross_ops_ = std::move(ops);
  cross_dirty_ = true;
  cross_rec_.drop();  // records of another request are not this one's
}

void Batch::check_cross(const char* entry) const {
  const std::string at = std::string(entry) + ": ";
  if (cross_.empty()) throw ArgError(at + "no cross request is set (mitdvp_batch_set_cross)");
  const int B = (int)eng_.size();
  for (size_t q = 0; q < cross_.size(); ++q) {
    const BatchCrossPair& c = cross_[q];
    if ((c.bra >= B || c.ket >= B) && !has_snap_)
      throw ArgError(at + "pair " + std::to_string(q) + " of the cross request names a snapshot, and the shapes changed since it was taken");
    if (c.site < 0) continue;
    // the operators lie in list order: this one ends where the next one starts, or at the end of the array
    size_t end = cross_ops_.size();
    for (size_t k = q + 1; k < cross_.size(); ++k)
      if (cross_[k].site >= 0) { end = (size_t)cross_[k].off; break; }
    if (end - (size_t)c.off != (size_t)shp_[c.site].d * shp_[c.site].d)
      throw ArgError(at + "pair " + std::to_string(q) + " of the cross request: the operator no longer matches the physical dimension " +
                     std::to_string(shp_[c.site].d) + " of site " + std::to_string(c.site));
  }
}

void Batch::upload_cross(long nrec) {
  const size_t np = cross_.size();
  reserve_synced(cross_rec_, BatchRecords{np, 2, (size_t)nrec}, d_cross_pairs_, np, d_cross_ops_, cross_ops_.size(), d_cross_buf_,
                 np * cross_buf_len());
  if (cross_dirty_) {
    HIP_CHECK(hipMemcpyAsync(d_cross_pairs_, cross_.data(), np * sizeof(BatchCrossPair), hipMemcpyHostToDevice, st_));
    if (!cross_ops_.empty())
      HIP_CHECK(hipMemcpyAsync(d_cross_ops_, cross_ops_.data(), cross_ops_.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
    cross_dirty_ = false;
  }
}

void Batch::launch_cross(long record) {
  BatchCrossArgs a{};
  a.L = L_;
  a.nrep = (int)eng_.size();
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.status = d_status_;
  a.snap = has_snap_ ? d_snap_ : nullptr;
  a.snap_len = snap_len();
  a.pairs = d_cross_pairs_;
  a.ops = d_cross_ops_;
  a.buf = d_cross_buf_;
  a.o_t2 = (size_t)plan_.max_bond;
  a.o_u = 2 * (size_t)plan_.max_bond;
  a.buf_len = cross_buf_len();
  a.rec = cross_rec_.slot(record);
  batch_cross_launch(st_, a, (int)cross_.size());
  n_launch_ += 1;
}

void Batch::cross(const double* weights, double* values, double* mean) {
  HIP_CHECK(hipSetDevice(device_));
  validate();
  check_cross("mitdvp_batch_cross");
  prepare_observing();
  upload_cross(cross_rec_.nrec);  // the slot behind the records of the last run, which stay
  cross_rec_.weights(st_, weights);
  launch_cross(cross_rec_.nrec);
  cross_rec_.mean_of_slot(st_, n_launch_);
  cross_rec_.fetch_slot(st_);
  finish_observe(2, nullptr);
  cross_rec_.slot_out(values, mean);
}

// the tail of every X_records: nothing without records or without a destination; one host wait when a mean was launched
void Batch::records_of(RecordStore& s, const double* weights, double* values, double* mean) {
  if (s.nrec == 0 || (!values && !mean)) return;
  if (mean && weights) HIP_CHECK(hipSetDevice(device_));
  if (s.records(st_, weights, values, mean, n_launch_)) finish_observe(1, nullptr);
}

void Batch::cross_records(const double* weights, double* values, double* mean, size_t* counts) {
  if (counts) { counts[0] = (size_t)cross_rec_.nrec; counts[1] = cross_.size(); }
  records_of(cross_rec_, weights, values, mean);
}

// ---- bond spectra and entanglement entropies (k_batch_spectra) ----
long Batch::spec_rec_len() const {
  long len = 0;
  for (int q : spec_bonds_) len += BSPEC_HEAD + shp_[q].dr;
  return len;
}

void Batch::set_spectra(const int* bonds, int nbonds) {
  const std::string at = "mitdvp_batch_set_spectra: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  if (nbonds < 0 || (nbonds > 0 && !bonds)) throw ArgError(at + "bad list of bonds (nbonds must be >= 0, and the list not null)");
  long len = 0;
  for (int k = 0; k < nbonds; ++k) {
    if (bonds[k] < 0 || bonds[k] > L_ - 2)
      throw ArgError(at + "bond " + std::to_string(bonds[k]) + " is out of range (the chain has " + std::to_string(L_) + " sites, bonds 0 .. " +
                     std::to_string(L_ - 2) + "; bond q lies between sites q and q + 1)");
    if (k > 0 && bonds[k] <= bonds[k - 1])
      throw ArgError(at + "the bonds must be strictly ascending (bond " + std::to_string(bonds[k]) + " follows bond " + std::to_string(bonds[k - 1]) + ")");
    len += BSPEC_HEAD + shp_[bonds[k]].dr;
  }
  if (len > BATCH_OBS_MAX_RDM)
    throw ArgError(at + "a replica's record would have " + std::to_string(len) + " doubles (4 + the bond's dimension per bond), a request takes at most " +
                   std::to_string(BATCH_OBS_MAX_RDM));
  spec_bonds_.assign(bonds, bonds + nbonds);
  spec_dirty_ = true;
  spec_rec_.drop();  // records of another request are not this one's
}

void Batch::check_spectra(const char* entry) const {
  const std::string at = std::string(entry) + ": ";
  if (spec_bonds_.empty()) throw ArgError(at + "no spectra request is set (mitdvp_batch_set_spectra)");
  if (spec_bonds_.back() > L_ - 2) throw ArgError(at + "the spectra request names bond " + std::to_string(spec_bonds_.back()) + ", which the chain no longer has");
  if (spec_rec_len() > BATCH_OBS_MAX_RDM)
    throw ArgError(at + "a replica's spectra record has " + std::to_string(spec_rec_len()) + " doubles at the bond dimensions as they are now, a request takes at most " +
                   std::to_string(BATCH_OBS_MAX_RDM));
}

void Batch::upload_spectra(long nrec) {
  const size_t n = eng_.size();
  reserve_synced(spec_rec_, BatchRecords{n, (size_t)spec_rec_len(), (size_t)nrec}, d_spec_buf_, n * spec_buf_len());
  if (spec_dirty_) {
    HIP_CHECK(hipMemcpyAsync(d_spec_bonds_, spec_bonds_.data(), spec_bonds_.size() * sizeof(int), hipMemcpyHostToDevice, st_));
    spec_dirty_ = false;
  }
  h_spec_fail_.assign(n, 0);
  HIP_CHECK(hipMemsetAsync(d_spec_fail_, 0, n * sizeof(int), st_));
}

void Batch::launch_spectra(long record) {
  BatchSpecArgs a{};
  a.L = L_;
  a.nbonds = (int)spec_bonds_.size();
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.status = d_status_;
  a.bonds = d_spec_bonds_;
  a.buf = d_spec_buf_;
  a.o_work = (size_t)plan_.max_site;
  a.o_r = 2 * (size_t)plan_.max_site;
  a.buf_len = spec_buf_len();
  a.fail = d_spec_fail_;
  a.rec_len = spec_rec_len();
  a.rec = spec_rec_.slot(record);
  batch_spectra_launch(st_, a, (int)eng_.size());
  n_launch_ += 1;
}

void Batch::spectra_failed(const char* entry) const {
  for (size_t i = 0; i < h_spec_fail_.size(); ++i)
    if (h_spec_fail_[i] != 0) {
      const int q = h_spec_fail_[i] - 1;
      throw NotConverged(std::string(entry) + ": replica " + std::to_string(i) + ": the Jacobi rotations of bond " + std::to_string(q) + " (between sites " +
                         std::to_string(q) + " and " + std::to_string(q + 1) + ") are not converged in " + std::to_string(BATCH_PAIR_MAX_SWEEPS) +
                         " sweeps; its spectra record is zeros, the replica itself is as it was");
    }
}

void Batch::spectra(const double* weights, double* values, double* mean, size_t* counts) {
  const std::string at = "mitdvp_batch_spectra: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  check_spectra("mitdvp_batch_spectra");
  const size_t n = eng_.size(), len = (size_t)spec_rec_len();
  if (counts) { counts[0] = n; counts[1] = len; }
  if (!values && !mean) return;
  for (size_t i = 0; i < n; ++i)
    if (eng_[i]->center_ != 0)
      throw ArgError(at + "replica " + std::to_string(i) + " has its centre at site " + std::to_string(eng_[i]->center_) +
                     "; the walk starts from the centre at site 0 (the state a batch step leaves)");
  prepare(true, false);
  upload_spectra(spec_rec_.nrec);  // the slot behind the records of the last run, which stay
  spec_rec_.weights(st_, weights);
  launch_spectra(spec_rec_.nrec);
  spec_rec_.mean_of_slot(st_, n_launch_);
  spec_rec_.fetch_slot(st_);
  HIP_CHECK(hipMemcpyAsync(h_spec_fail_.data(), d_spec_fail_, n * sizeof(int), hipMemcpyDeviceToHost, st_));
  finish_observe(2, nullptr);
  spec_rec_.slot_out(values, mean);
  spectra_failed("mitdvp_batch_spectra");
}

void Batch::spectra_records(const double* weights, double* values, double* mean, size_t* counts) {
  if (counts) { counts[0] = (size_t)spec_rec_.nrec; counts[1] = eng_.size(); counts[2] = spec_bonds_.empty() ? 0 : (size_t)spec_rec_len(); }
  records_of(spec_rec_, weights, values, mean);
}

// ---- sampled configurations (k_batch_sample) ----
long Batch::smp_F() const {
  long F = 0;
  for (const BatchShape& s : shp_) F += s.d;
  return F;
}

size_t Batch::smp_o_w() const {
  int b = 1;
  for (const BatchShape& s : shp_) b = std::max(b, std::max(s.dl, s.dr));
  return (size_t)BATCH_SAMPLE_CHUNK * b;
}

size_t Batch::smp_o_g() const {
  long ddr = 1;
  for (const BatchShape& s : shp_) ddr = std::max(ddr, (long)s.d * s.dr);
  return smp_o_w() + (size_t)BATCH_SAMPLE_CHUNK * ddr;
}

size_t Batch::smp_buf_len() const {
  int d = 1;
  for (const BatchShape& s : shp_) d = std::max(d, s.d);
  return smp_o_g() + ((size_t)BATCH_SAMPLE_CHUNK * d + 1) / 2;  // the weights are doubles: two to a complex element
}

void Batch::set_samples(int nshots, unsigned long long seed) {
  const std::string at = "mitdvp_batch_set_samples: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  if (nshots < 0 || nshots > BATCH_SAMPLE_MAX_SHOTS)
    throw ArgError(at + "nshots = " + std::to_string(nshots) + " is outside 0 .. " + std::to_string(BATCH_SAMPLE_MAX_SHOTS) + " (0 removes the request)");
  if ((long)nshots * L_ > BATCH_SAMPLE_MAX_CONFIG)
    throw ArgError(at + std::to_string(nshots) + " shots of " + std::to_string(L_) + " sites are " + std::to_string((long)nshots * L_) +
                   " outcomes per replica, a request takes at most " + std::to_string(BATCH_SAMPLE_MAX_CONFIG));
  smp_nshots_ = nshots;
  smp_seed_ = seed;
  smp_rec_.drop();  // records of another request are not this one's
}

void Batch::check_samples(const char* entry) const {
  const std::string at = std::string(entry) + ": ";
  if (smp_nshots_ < 1) throw ArgError(at + "no samples request is set (mitdvp_batch_set_samples)");
  if ((long)smp_nshots_ * L_ > BATCH_SAMPLE_MAX_CONFIG)
    throw ArgError(at + "the samples request has " + std::to_string((long)smp_nshots_ * L_) + " outcomes per replica, a request takes at most " +
                   std::to_string(BATCH_SAMPLE_MAX_CONFIG));
}

void Batch::upload_samples(long nrec) {
  // configurations and probabilities grow with the frequencies: only with a new request, other shapes or in run()
  const size_t n = eng_.size();
  reserve_synced(smp_rec_, BatchRecords{n, (size_t)smp_F(), (size_t)nrec}, d_smp_cfg_, smp_cfg_lay(nrec).rec_elems(), d_smp_prob_,
                 smp_prob_lay(nrec).rec_elems(), d_smp_buf_, n * smp_buf_len());
}

void Batch::launch_samples(long record, long long step) {
  BatchSampleArgs a{};
  a.L = L_;
  a.nshots = smp_nshots_;
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.status = d_status_;
  a.seed = smp_seed_;
  a.step = step;
  a.ids = d_ids_;
  a.buf = d_smp_buf_;
  a.o_w = smp_o_w();
  a.o_g = smp_o_g();
  a.buf_len = smp_buf_len();
  a.F = smp_F();
  a.configs = d_smp_cfg_ + smp_cfg_lay(smp_rec_.nrec).rec_slot((size_t)record);
  a.prob = d_smp_prob_ + smp_prob_lay(smp_rec_.nrec).rec_slot((size_t)record);
  a.freq = smp_rec_.slot(record);
  batch_sample_launch(st_, a, (int)eng_.size());
  n_launch_ += 1;
}

void Batch::samples(const double* weights, int* configs, double* prob, double* freq, double* mean_freq, size_t* counts) {
  const std::string at = "mitdvp_batch_samples: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  check_samples("mitdvp_batch_samples");
  const size_t n = eng_.size(), ns = (size_t)smp_nshots_, F = (size_t)smp_F();
  if (counts) { counts[0] = n; counts[1] = ns; counts[2] = (size_t)L_; counts[3] = F; }
  if (!configs && !prob && !freq && !mean_freq) return;
  for (size_t i = 0; i < n; ++i)
    if (eng_[i]->center_ != 0)
      throw ArgError(at + "replica " + std::to_string(i) + " has its centre at site " + std::to_string(eng_[i]->center_) +
                     "; the walk starts from the centre at site 0 (the state a batch step leaves)");
  prepare(true, false);
  const long slot = smp_rec_.nrec;  // behind the records of the last run, which stay
  const BatchRecords cl = smp_cfg_lay(slot), pl = smp_prob_lay(slot);
  upload_samples(slot);
  smp_rec_.weights(st_, weights);
  launch_samples(slot, steps_done_);
  smp_rec_.mean_of_slot(st_, n_launch_);
  h_smp_cfg_now_.resize(cl.slot_elems());
  h_smp_prob_now_.resize(pl.slot_elems());
  if (configs) HIP_CHECK(hipMemcpyAsync(h_smp_cfg_now_.data(), d_smp_cfg_ + cl.rec_now(), cl.slot_elems() * sizeof(int), hipMemcpyDeviceToHost, st_));
  if (prob) HIP_CHECK(hipMemcpyAsync(h_smp_prob_now_.data(), d_smp_prob_ + pl.rec_now(), pl.slot_elems() * sizeof(double), hipMemcpyDeviceToHost, st_));
  smp_rec_.fetch_slot(st_, freq != nullptr, mean_freq != nullptr);
  finish_observe(2, nullptr);
  if (configs) std::memcpy(configs, h_smp_cfg_now_.data(), cl.slot_elems() * sizeof(int));
  if (prob) std::memcpy(prob, h_smp_prob_now_.data(), pl.slot_elems() * sizeof(double));
  smp_rec_.slot_out(freq, mean_freq);
}

void Batch::samples_records(const double* weights, int* configs, double* prob, double* freq, double* mean_freq, size_t* counts) {
  const long nrec = smp_rec_.nrec;
  if (counts) {
    counts[0] = (size_t)nrec; counts[1] = eng_.size(); counts[2] = (size_t)smp_nshots_; counts[3] = (size_t)L_;
    counts[4] = smp_nshots_ > 0 ? (size_t)smp_F() : 0;
  }
  if (nrec == 0) return;
  if (configs) std::memcpy(configs, h_smp_cfg_.data(), smp_cfg_lay(nrec).rec_now() * sizeof(int));
  if (prob) std::memcpy(prob, h_smp_prob_.data(), smp_prob_lay(nrec).rec_now() * sizeof(double));
  records_of(smp_rec_, weights, freq, mean_freq);
}

// ---- expectation values of MPO observables (k_batch_expect) ----
void Batch::expect_shapes(const char* entry, const int* op_ids, int nops, std::vector<BatchShape>& shp, BatchExpectPlan& plan) const {
  operator_shapes(entry, op_ids, nops, shp);
  std::string why;
  if (!batch_expect_plan(shp.data(), op_ids, L_, nops, plan, why)) throw ArgError(std::string(entry) + ": " + why);
}

void Batch::operator_shapes(const char* entry, const int* op_ids, int nops, std::vector<BatchShape>& shp, const int* only,
                            int nonly) const {
  const std::string at = std::string(entry) + ": ";
  shp.assign((size_t)nops * L_, BatchShape{});
  const size_t nlook = only ? (size_t)nonly : eng_.size();
  const size_t first = only && nonly > 0 ? (size_t)only[0] : 0;
  for (int k = 0; k < nops; ++k) {
    const std::string op = "operator " + std::to_string(op_ids[k]) + " ";
    for (size_t ii = 0; ii < nlook; ++ii) {
      const size_t i = only ? (size_t)only[ii] : ii;
      const Engine& e = *eng_[i];
      auto it = e.ops_.find(op_ids[k]);
      for (int p = 0; p < L_; ++p) {
        if (it == e.ops_.end() || !it->second.sites[p].set)
          throw ArgError(at + op + "has no core at site " + std::to_string(p) + " of replica " + std::to_string(i) +
                         " (every replica must carry every listed operator at all " + std::to_string(L_) + " sites)");
        const MpoSite& w = it->second.sites[p];
        if (w.d != shp_[p].d)
          throw ArgError(at + op + "has physical dimension " + std::to_string(w.d) + " at site " + std::to_string(p) + " of replica " +
                         std::to_string(i) + ", the site's is " + std::to_string(shp_[p].d));
        BatchShape& s = shp[(size_t)k * L_ + p];
        if (ii == 0) s = BatchShape{shp_[p].dl, shp_[p].d, shp_[p].dr, w.ml, w.mr};
        else if (w.ml != s.ml || w.mr != s.mr)
          throw ArgError(at + op + "has MPO bonds (" + std::to_string(w.ml) + ", " + std::to_string(w.mr) + ") at site " + std::to_string(p) +
                         " of replica " + std::to_string(i) + ", replica " + std::to_string(first) + " has (" + std::to_string(s.ml) + ", " + std::to_string(s.mr) +
                         "): the core shapes must be equal across the replicas");
      }
    }
  }
}

void Batch::set_expect(const int* op_ids, int nops) {
  const std::string at = "mitdvp_batch_set_expect: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  if (nops < 0 || nops > BATCH_EXPECT_MAX_OPS || (nops > 0 && !op_ids))
    throw ArgError(at + "bad list of operators (" + std::to_string(nops) + " given; a request takes 0 to " + std::to_string(BATCH_EXPECT_MAX_OPS) +
                   ", and the list must not be null)");
  for (int k = 0; k < nops; ++k) {
    if (op_ids[k] < 0) throw ArgError(at + "operator " + std::to_string(op_ids[k]) + " is negative (operator ids are >= 0)");
    for (int j = 0; j < k; ++j)
      if (op_ids[j] == op_ids[k]) throw ArgError(at + "operator " + std::to_string(op_ids[k]) + " is listed twice");
  }
  std::vector<BatchShape> shp;
  BatchExpectPlan plan;
  expect_shapes("mitdvp_batch_set_expect", op_ids, nops, shp, plan);
  exp_ops_.assign(op_ids, op_ids + nops);
  exp_shp_ = std::move(shp);
  exp_plan_ = plan;
  exp_shp_dirty_ = true;
  h_exp_ptrs_.clear();
  exp_rec_.drop();  // records of another request are not this one's
}

void Batch::check_expect(const char* entry) {
  if (exp_ops_.empty()) throw ArgError(std::string(entry) + ": no expect request is set (mitdvp_batch_set_expect)");
  std::vector<BatchShape> shp;
  BatchExpectPlan plan;
  expect_shapes(entry, exp_ops_.data(), (int)exp_ops_.size(), shp, plan);
  if (shp.size() != exp_shp_.size() || std::memcmp(shp.data(), exp_shp_.data(), shp.size() * sizeof(BatchShape)) != 0) {
    exp_shp_ = std::move(shp);
    exp_shp_dirty_ = true;
    exp_rec_.drop();  // the engines were given cores of other shapes: records walked over the old ones are dropped
  }
  exp_plan_ = plan;
}

void Batch::upload_expect(long nrec) {
  const size_t n = eng_.size(), nops = exp_ops_.size();
  const size_t need_ptrs = n * nops * 3 * L_, need_shp = nops * L_, need_shift = n * nops;
  if (!d_exp_ptrs_.fits(need_ptrs)) h_exp_ptrs_.clear();  // a table that moves is uploaded again
  if (!d_exp_shp_.fits(need_shp)) exp_shp_dirty_ = true;
  reserve_synced(exp_rec_, BatchRecords{n, 2 * nops, (size_t)nrec}, d_exp_ptrs_, need_ptrs, d_exp_shp_, need_shp, d_exp_shift_, need_shift,
                 d_exp_buf_, n * nops * exp_plan_.total);
  // tables: [w2l L][w2el L][w2er L] per (replica, operator); the engines may have been given new cores since the last call
  std::vector<void*> h(need_ptrs);
  h_exp_shift_.resize(need_shift);
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < nops; ++k) {
      const Operator& o = eng_[i]->ops_.find(exp_ops_[k])->second;
      void** q = h.data() + (i * nops + k) * 3 * L_;
      for (int p = 0; p < L_; ++p) {
        q[p] = o.sites[p].w2l.p;
        q[L_ + p] = o.sites[p].w2el.p;
        q[2 * L_ + p] = o.sites[p].w2er.p;
      }
      h_exp_shift_[i * nops + k] = make_double2(o.shift.real(), o.shift.imag());
    }
  if (h != h_exp_ptrs_) {
    h_exp_ptrs_ = h;
    HIP_CHECK(hipMemcpyAsync(d_exp_ptrs_, h_exp_ptrs_.data(), need_ptrs * sizeof(void*), hipMemcpyHostToDevice, st_));
  }
  if (exp_shp_dirty_) {
    HIP_CHECK(hipMemcpyAsync(d_exp_shp_, exp_shp_.data(), need_shp * sizeof(BatchShape), hipMemcpyHostToDevice, st_));
    exp_shp_dirty_ = false;
  }
  HIP_CHECK(hipMemcpyAsync(d_exp_shift_, h_exp_shift_.data(), need_shift * sizeof(zc), hipMemcpyHostToDevice, st_));
}

void Batch::launch_expect(long record) {
  BatchExpectArgs a{};
  a.L = L_;
  a.nops = (int)exp_ops_.size();
  a.shp = d_exp_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.ops = d_exp_ptrs_;
  a.shift = d_exp_shift_;
  a.status = d_status_;
  a.buf = d_exp_buf_;
  a.plan = exp_plan_;
  a.rec = exp_rec_.slot(record);
  batch_expect_launch(st_, a, (int)eng_.size());
  n_launch_ += 1;
}

void Batch::expect(const double* weights, double* values, double* mean, size_t* counts) {
  const std::string at = "mitdvp_batch_expect: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  check_expect("mitdvp_batch_expect");
  const size_t n = eng_.size();
  if (counts) { counts[0] = n; counts[1] = exp_ops_.size(); }
  if (!values && !mean) return;
  for (size_t i = 0; i < n; ++i)
    if (eng_[i]->center_ != 0)
      throw ArgError(at + "replica " + std::to_string(i) + " has its centre at site " + std::to_string(eng_[i]->center_) +
                     "; the walk ends at the centre at site 0 (the state a batch step leaves)");
  prepare(true, false);
  upload_expect(exp_rec_.nrec);  // the slot behind the records of the last run, which stay
  exp_rec_.weights(st_, weights);
  launch_expect(exp_rec_.nrec);
  exp_rec_.mean_of_slot(st_, n_launch_);
  exp_rec_.fetch_slot(st_);
  finish_observe(2, nullptr);
  exp_rec_.slot_out(values, mean);
}

void Batch::expect_records(const double* weights, double* values, double* mean, size_t* counts) {
  if (counts) { counts[0] = (size_t)exp_rec_.nrec; counts[1] = eng_.size(); counts[2] = exp_ops_.size(); }
  records_of(exp_rec_, weights, values, mean);
}

// ---- MPO matrix elements between replicas (k_batch_cross_mpo) ----
void Batch::cross_mpo_shapes(const char* entry, const int* op_ids, int nops, size_t nentries, std::vector<BatchShape>& shp,
                             BatchCrossMpoPlan& plan) const {
  const std::string at = std::string(entry) + ": ";
  operator_shapes(entry, op_ids, nops, shp);
  std::string why;
  if (!batch_cross_mpo_plan(shp.data(), op_ids, L_, nops, plan, why)) throw ArgError(at + why);
  if (!batch_cross_mpo_fits(nentries, plan, why)) throw ArgError(at + why);
}

void Batch::set_cross_mpo(int nentries, const int* bra, const int* ket, const int* op_id) {
  const std::string at = "mitdvp_batch_set_cross_mpo: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  const int B = (int)eng_.size();
  std::string bad;
  if (!batch_cross_mpo_entries_ok(B, has_snap_, nentries, bra, ket, op_id, bad)) throw ArgError(at + bad);
  std::vector<BatchCrossMpoEntry> ent((size_t)nentries);
  std::vector<int> ops;  // the distinct operators in order of first use
  std::map<int, int> slot;
  for (int q = 0; q < nentries; ++q) {
    auto it = slot.find(op_id[q]);
    if (it == slot.end()) {
      it = slot.emplace(op_id[q], (int)ops.size()).first;
      ops.push_back(op_id[q]);
    }
    ent[q] = BatchCrossMpoEntry{bra[q], ket[q], it->second, 0};
  }
  std::vector<BatchShape> shp;
  BatchCrossMpoPlan plan;
  cross_mpo_shapes("mitdvp_batch_set_cross_mpo", ops.data(), (int)ops.size(), (size_t)nentries, shp, plan);
  xm_ = std::move(ent);
  xm_ops_ = std::move(ops);
  xm_shp_ = std::move(shp);
  xm_plan_ = plan;
  xm_dirty_ = true;
  h_xm_ptrs_.clear();
  xm_rec_.drop();  // records of another request are not this one's
}

void Batch::check_cross_mpo(const char* entry) {
  const std::string at = std::string(entry) + ": ";
  if (xm_.empty()) throw ArgError(at + "no cross request of MPOs is set (mitdvp_batch_set_cross_mpo)");
  const int B = (int)eng_.size();
  for (size_t q = 0; q < xm_.size(); ++q)
    if ((xm_[q].bra >= B || xm_[q].ket >= B) && !has_snap_)
      throw ArgError(at + "entry " + std::to_string(q) + " of the cross request of MPOs names a snapshot, and the shapes changed since it was taken");
  std::vector<BatchShape> shp;
  BatchCrossMpoPlan plan;
  cross_mpo_shapes(entry, xm_ops_.data(), (int)xm_ops_.size(), xm_.size(), shp, plan);
  if (shp.size() != xm_shp_.size() || std::memcmp(shp.data(), xm_shp_.data(), shp.size() * sizeof(BatchShape)) != 0) {
    xm_shp_ = std::move(shp);
    xm_dirty_ = true;
    xm_rec_.drop();  // the engines were given cores of other shapes: records walked over the old ones are dropped
  }
  xm_plan_ = plan;
}

void Batch::upload_cross_mpo(long nrec) {
  const size_t n = eng_.size(), np = xm_.size(), nops = xm_ops_.size();
  const size_t need_ptrs = n * nops * L_, need_shp = nops * L_, need_shift = n * nops;
  if (!d_xm_ent_.fits(np) || !d_xm_shp_.fits(need_shp)) xm_dirty_ = true;  // a table that moves is uploaded again
  if (!d_xm_ptrs_.fits(need_ptrs)) h_xm_ptrs_.clear();
  reserve_synced(xm_rec_, BatchRecords{np, 2, (size_t)nrec}, d_xm_ent_, np, d_xm_ptrs_, need_ptrs, d_xm_shp_, need_shp, d_xm_shift_, need_shift,
                 d_xm_buf_, np * xm_plan_.total);
  // tables: w2el of every site per (replica, operator); the engines may have been given new cores since the last call
  std::vector<void*> h(need_ptrs);
  h_xm_shift_.resize(need_shift);
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < nops; ++k) {
      const Operator& o = eng_[i]->ops_.find(xm_ops_[k])->second;
      void** q = h.data() + (i * nops + k) * L_;
      for (int p = 0; p < L_; ++p) q[p] = o.sites[p].w2el.p;
      h_xm_shift_[i * nops + k] = make_double2(o.shift.real(), o.shift.imag());
    }
  if (h != h_xm_ptrs_) {
    h_xm_ptrs_ = h;
    HIP_CHECK(hipMemcpyAsync(d_xm_ptrs_, h_xm_ptrs_.data(), need_ptrs * sizeof(void*), hipMemcpyHostToDevice, st_));
  }
  if (xm_dirty_) {
    HIP_CHECK(hipMemcpyAsync(d_xm_ent_, xm_.data(), np * sizeof(BatchCrossMpoEntry), hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(d_xm_shp_, xm_shp_.data(), need_shp * sizeof(BatchShape), hipMemcpyHostToDevice, st_));
    xm_dirty_ = false;
  }
  HIP_CHECK(hipMemcpyAsync(d_xm_shift_, h_xm_shift_.data(), need_shift * sizeof(zc), hipMemcpyHostToDevice, st_));
}

void Batch::launch_cross_mpo(long record) {
  BatchCrossMpoArgs a{};
  a.L = L_;
  a.nrep = (int)eng_.size();
  a.nops = (int)xm_ops_.size();
  a.shp = d_xm_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.status = d_status_;
  a.snap = has_snap_ ? d_snap_ : nullptr;
  a.snap_len = snap_len();
  a.entries = d_xm_ent_;
  a.ops = d_xm_ptrs_;
  a.shift = d_xm_shift_;
  a.buf = d_xm_buf_;
  a.plan = xm_plan_;
  a.rec = xm_rec_.slot(record);
  batch_cross_mpo_launch(st_, a, (int)xm_.size());
  n_launch_ += 1;
}

void Batch::cross_mpo(const double* weights, double* values, double* mean) {
  HIP_CHECK(hipSetDevice(device_));
  validate();
  check_cross_mpo("mitdvp_batch_cross_mpo");
  prepare_observing();
  upload_cross_mpo(xm_rec_.nrec);  // the slot behind the records of the last run, which stay
  xm_rec_.weights(st_, weights);
  launch_cross_mpo(xm_rec_.nrec);
  xm_rec_.mean_of_slot(st_, n_launch_);
  xm_rec_.fetch_slot(st_);
  finish_observe(2, nullptr);
  xm_rec_.slot_out(values, mean);
}

void Batch::cross_mpo_records(const double* weights, double* values, double* mean, size_t* counts) {
  if (counts) { counts[0] = (size_t)xm_rec_.nrec; counts[1] = xm_.size(); }
  records_of(xm_rec_, weights, values, mean);
}

// ---- an MPO applied to the replicas (k_batch_operate) ----
void Batch::operate(int op_id, int maxstep, double conv_tol, const int* replicas, int nsel, double* norms, int* iters, int* statuses) {
  const std::string at = "mitdvp_batch_operate: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  const int B = (int)eng_.size();
  if (maxstep < 1) throw ArgError(at + "maxstep = " + std::to_string(maxstep) + ", it must be >= 1");
  if (!(conv_tol >= 0.0) || !std::isfinite(conv_tol))
    throw ArgError(at + "conv_tol = " + std::to_string(conv_tol) + ", it must be finite and >= 0");
  if (op_id < 0) throw ArgError(at + "operator " + std::to_string(op_id) + " is negative (operator ids are >= 0)");
  std::vector<int> sel;
  if (replicas) {
    if (nsel < 1) throw ArgError(at + "the list of replicas is empty (null selects all " + std::to_string(B) + ")");
    std::vector<char> seen((size_t)B, 0);
    for (int k = 0; k < nsel; ++k) {
      const int r = replicas[k];
      if (r < 0 || r >= B)
        throw ArgError(at + "replica " + std::to_string(r) + " (entry " + std::to_string(k) + " of the list) is outside 0 .. " +
                       std::to_string(B - 1));
      if (seen[(size_t)r]) throw ArgError(at + "replica " + std::to_string(r) + " is listed twice (entry " + std::to_string(k) + ")");
      seen[(size_t)r] = 1;
    }
    sel.assign(replicas, replicas + nsel);
  } else {
    sel.resize((size_t)B);
    for (int r = 0; r < B; ++r) sel[(size_t)r] = r;
  }
  const size_t ns = sel.size();
  for (int r : sel)
    if (eng_[(size_t)r]->center_ != 0)
      throw ArgError(at + "replica " + std::to_string(r) + " has its centre at site " + std::to_string(eng_[(size_t)r]->center_) +
                     "; the fit starts from the centre at site 0 (the state a batch step leaves)");
  std::vector<BatchShape> shp;
  operator_shapes("mitdvp_batch_operate", &op_id, 1, shp, sel.data(), (int)ns);
  BatchOperatePlan plan;
  std::string why;
  if (!batch_operate_plan(shp.data(), op_id, L_, plan, why)) throw ArgError(at + why);
  if (!batch_operate_fits(ns, plan, why)) throw ArgError(at + why);

  prepare(true, false);  // canonical chains around site 0; the pointer table, zeroed status words, the engines' streams
  const size_t need_ptrs = ns * 3 * L_, need_offs = (size_t)3 * (L_ + 1), need_buf = ns * plan.total;
  reserve_synced(d_op_rep_, ns, d_op_ptrs_, need_ptrs, d_op_shift_, ns, d_op_buf_, need_buf, d_op_shp_, (size_t)L_, d_op_offs_, need_offs,
                 d_op_norms_, ns, d_op_iters_, ns);
  std::vector<void*> h_ptrs(need_ptrs);
  std::vector<zc> h_shift(ns);
  std::vector<long long> h_offs(need_offs);
  for (size_t k = 0; k < ns; ++k) {
    const Operator& o = eng_[(size_t)sel[k]]->ops_.find(op_id)->second;
    void** q = h_ptrs.data() + k * 3 * L_;
    for (int p = 0; p < L_; ++p) {
      q[p] = o.sites[p].w2l.p;
      q[L_ + p] = o.sites[p].w2el.p;
      q[2 * L_ + p] = o.sites[p].w2er.p;
    }
    h_shift[k] = make_double2(o.shift.real(), o.shift.imag());
  }
  for (int b = 0; b <= L_; ++b) {
    h_offs[(size_t)b] = plan.site[(size_t)b];
    h_offs[(size_t)(L_ + 1) + b] = plan.mix[(size_t)b];
    h_offs[(size_t)2 * (L_ + 1) + b] = plan.ov[(size_t)b];
  }
  // the sources are locals: they live until the host wait below
  HIP_CHECK(hipMemcpyAsync(d_op_rep_, sel.data(), ns * sizeof(int), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(d_op_ptrs_, h_ptrs.data(), need_ptrs * sizeof(void*), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(d_op_shift_, h_shift.data(), ns * sizeof(zc), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(d_op_shp_, shp.data(), (size_t)L_ * sizeof(BatchShape), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(d_op_offs_, h_offs.data(), need_offs * sizeof(long long), hipMemcpyHostToDevice, st_));

  BatchOperateArgs a{};
  a.L = L_;
  a.maxstep = maxstep;
  a.conv_tol = conv_tol;
  a.shp = d_op_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  a.replicas = d_op_rep_;
  a.ops = d_op_ptrs_;
  a.shift = d_op_shift_;
  a.offs = d_op_offs_;
  a.buf = d_op_buf_;
  a.carve = BatchOperateCarve{plan.o_ket, plan.o_prev, plan.o_mix, plan.o_ov, plan.o_x, plan.o_y, plan.o_work, plan.o_spare,
                              plan.o_h, plan.o_sig, plan.o_t0, plan.o_t1, plan.o_id, plan.total};
  a.status = d_status_;
  a.norms = d_op_norms_;
  a.iters = d_op_iters_;
  batch_operate_launch(st_, a, (int)ns);
  n_launch_ += 1;

  std::vector<int> st((size_t)B), h_iters(ns);
  std::vector<double> h_norms(ns);
  HIP_CHECK(hipMemcpyAsync(st.data(), d_status_, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(h_norms.data(), d_op_norms_, ns * sizeof(double), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(h_iters.data(), d_op_iters_, ns * sizeof(int), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));  // the one host wait of the call
  eng_[0]->cnt_.n_launch += 1;           // the batch's launches are counted once
  for (size_t k = 0; k < ns; ++k) {
    const int r = sel[k];
    Engine& e = *eng_[(size_t)r];
    const bool ok = st[(size_t)r] == SS_OK;
    for (int p = 0; p < L_; ++p) e.gauge_[p] = !ok ? MITDVP_GAUGE_C : (p == 0 ? MITDVP_GAUGE_PSI : MITDVP_GAUGE_B);
    e.center_ = ok ? 0 : -1;
    for (int b = 1; b < L_; ++b) { e.envL_ok_[b] = 0; e.envR_ok_[b] = 0; }  // the blocks describe the state before the fit
    (void)e.take_env_checked();
    if (norms) norms[r] = h_norms[k];
    if (iters) iters[r] = h_iters[k];
    if (statuses) statuses[r] = st[(size_t)r];
  }
}

// ---- ground states by improved relaxation (k_batch_relax) ----
void Batch::relax(int maxstep, double conv_tol, double* energies, int* steps, double* history, int* statuses) {
  const std::string at = "mitdvp_batch_relax: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  const size_t n = eng_.size();
  if (maxstep < 1) throw ArgError(at + "maxstep = " + std::to_string(maxstep) + ", it must be >= 1");
  if (maxstep > BATCH_RELAX_MAX_STEPS)
    throw ArgError(at + "maxstep = " + std::to_string(maxstep) + ", one call takes at most " + std::to_string(BATCH_RELAX_MAX_STEPS));
  if (!(conv_tol >= 0.0) || !std::isfinite(conv_tol))
    throw ArgError(at + "conv_tol = " + std::to_string(conv_tol) + ", it must be finite and >= 0");
  if (eng_[0]->cfg.relax != 2)
    throw ArgError(at + "the replicas have relax = " + std::to_string(eng_[0]->cfg.relax) + ", the call needs improved relaxation (relax must be 2)");
  for (size_t i = 0; i < n; ++i)
    if (eng_[i]->center_ != 0)
      throw ArgError(at + "replica " + std::to_string(i) + " has its centre at site " + std::to_string(eng_[i]->center_) +
                     "; a relaxation step starts from the centre at site 0 (the state a batch step leaves)");
  prepare(true);  // the right blocks, where no step has built them
  const size_t nh = n * (size_t)maxstep;
  reserve_synced(d_rx_energy_, n, d_rx_steps_, n, d_rx_hist_, nh);
  std::vector<double> h_e(n, std::nan("")), h_hist(nh, std::nan(""));
  std::vector<int> h_steps(n, 0);
  // the sources are locals: they live until the host wait in finish()
  HIP_CHECK(hipMemcpyAsync(d_rx_energy_, h_e.data(), n * sizeof(double), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(d_rx_hist_, h_hist.data(), nh * sizeof(double), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemsetAsync(d_rx_steps_, 0, n * sizeof(int), st_));
  launch_relax(true, 2 * maxstep, conv_tol, d_rx_energy_, d_rx_steps_, d_rx_hist_, maxstep);
  std::vector<double> o_e(n), o_hist(nh);
  HIP_CHECK(hipMemcpyAsync(o_e.data(), d_rx_energy_, n * sizeof(double), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(o_hist.data(), d_rx_hist_, nh * sizeof(double), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipMemcpyAsync(h_steps.data(), d_rx_steps_, n * sizeof(int), hipMemcpyDeviceToHost, st_));
  // the one host wait of the call; the counters take the half-sweeps of the replica that ran the most, then each
  // replica's own count is put right below (a replica that stopped early ran fewer)
  finish(false, 0, statuses, 1);
  for (size_t i = 0; i < n; ++i) {
    Engine& e = *eng_[i];
    const long long hs = 2LL * h_steps[i];
    e.cnt_.n_exp_site += hs * L_;
    e.cnt_.n_qr += hs * (L_ - 1);
    e.cnt_.n_env += hs * (L_ - 1);
  }
  if (energies) std::memcpy(energies, o_e.data(), n * sizeof(double));
  if (steps) std::memcpy(steps, h_steps.data(), n * sizeof(int));
  if (history) std::memcpy(history, o_hist.data(), nh * sizeof(double));
}

void Batch::set_relax_restarts(int max_restarts) {
  const std::string at = "mitdvp_batch_set_relax_restarts: ";
  if (eng_[0]->cfg.relax != 2)
    throw ArgError(at + "the replicas have relax = " + std::to_string(eng_[0]->cfg.relax) + ", restarts belong to improved relaxation (relax must be 2)");
  std::string bad;
  if (!batch_relax_restarts_ok(max_restarts, bad)) throw ArgError(at + bad);
  rx_restarts_ = max_restarts;
  const size_t n = eng_.size();
  if (d_rx_rst_total_.fits(n) && d_rx_rst_most_.fits(n)) {  // behind the launches queued so far; before the first launch there is nothing to clear
    HIP_CHECK(hipSetDevice(device_));
    HIP_CHECK(hipMemsetAsync(d_rx_rst_total_, 0, n * sizeof(long long), st_));
    HIP_CHECK(hipMemsetAsync(d_rx_rst_most_, 0, n * sizeof(int), st_));
  }
}

void Batch::relax_restarts(long long* total, int* most) {
  const size_t n = eng_.size();
  std::vector<long long> t(n, 0);
  std::vector<int> m(n, 0);
  if (d_rx_rst_total_.fits(n) && d_rx_rst_most_.fits(n)) {
    HIP_CHECK(hipSetDevice(device_));
    HIP_CHECK(hipMemcpyAsync(t.data(), d_rx_rst_total_, n * sizeof(long long), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(m.data(), d_rx_rst_most_, n * sizeof(int), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  if (total) std::memcpy(total, t.data(), n * sizeof(long long));
  if (most) std::memcpy(most, m.data(), n * sizeof(int));
}

// ---- excited states by deflation against stored states (k_batch_relax_defl, k_batch_defl_overlaps) ----
void Batch::deflate_push(const double* weights) {
  const std::string at = "mitdvp_batch_deflate_push: ";
  HIP_CHECK(hipSetDevice(device_));
  validate();
  const size_t n = eng_.size();
  if (eng_[0]->cfg.relax != 2)
    throw ArgError(at + "the replicas have relax = " + std::to_string(eng_[0]->cfg.relax) +
                   ", stored states deflate the improved relaxation (relax must be 2)");
  for (size_t i = 0; i < n; ++i) {
    const Engine& e = *eng_[i];
    if (e.center_ != 0)
      throw ArgError(at + "replica " + std::to_string(i) + " has its centre at site " + std::to_string(e.center_) +
                     "; a state is stored with the centre at site 0 (the state mitdvp_batch_relax leaves)");
    for (int p = 0; p < L_; ++p)
      if (e.gauge_[p] != (p == 0 ? MITDVP_GAUGE_PSI : MITDVP_GAUGE_B))
        throw ArgError(at + "replica " + std::to_string(i) + ": the chain is not canonical around site 0");
  }
  std::string bad;
  if (!batch_deflate_room(defl_count_, bad)) throw ArgError(at + bad);
  if (!batch_deflate_weights_ok(weights, (int)n, bad)) throw ArgError(at + bad);
  if (!batch_deflate_fits(shp_.data(), L_, defl_count_ + 1, n, bad)) throw ArgError(at + bad);
  prepare(true, false);
  const int k = defl_count_;
  if (h_defl_w_.size() != n * BATCH_MAX_DEFLATE) h_defl_w_.assign(n * BATCH_MAX_DEFLATE, 0.0);
  reserve_synced(d_defl_slot_[k], n * snap_len(), d_defl_w_, n * BATCH_MAX_DEFLATE);
  std::memcpy(h_defl_w_.data() + (size_t)k * n, weights, n * sizeof(double));
  HIP_CHECK(hipMemcpyAsync(d_defl_w_, h_defl_w_.data(), h_defl_w_.size() * sizeof(double), hipMemcpyHostToDevice, st_));
  batch_snapshot_launch(st_, d_shp_, d_ptrs_, (int)ptrs_per_replica(), d_defl_slot_[k], snap_len(), L_, (int)n);
  n_launch_ += 1;
  finish_observe(1, nullptr);
  defl_count_ = k + 1;
}

int Batch::deflate_count() {
  validate();
  return defl_count_;
}

void Batch::deflate_overlaps(double* reim) {
  HIP_CHECK(hipSetDevice(device_));
  validate();
  if (defl_count_ == 0) return;
  const size_t n = eng_.size(), rows = (size_t)defl_count_ * n;
  prepare_observing();
  reserve_synced(d_defl_ovbuf_, rows * cross_buf_len(), d_defl_ov_, 2 * rows);
  BatchDeflOvArgs a{};
  a.L = L_;
  a.nrep = (int)n;
  a.count = defl_count_;
  a.shp = d_shp_;
  a.ptrs = d_ptrs_;
  a.ptr_stride = (int)ptrs_per_replica();
  for (int k = 0; k < defl_count_; ++k) a.slot[k] = d_defl_slot_[k];
  a.snap_len = snap_len();
  a.buf = d_defl_ovbuf_;
  a.o_t2 = (size_t)plan_.max_bond;
  a.o_u = 2 * (size_t)plan_.max_bond;
  a.buf_len = cross_buf_len();
  a.rec = d_defl_ov_;
  batch_defl_overlaps_launch(st_, a);
  n_launch_ += 1;
  std::vector<double> h(2 * rows);
  HIP_CHECK(hipMemcpyAsync(h.data(), d_defl_ov_, h.size() * sizeof(double), hipMemcpyDeviceToHost, st_));
  finish_observe(1, nullptr);
  if (reim) std::memcpy(reim, h.data(), h.size() * sizeof(double));
}

// the eigen-solve of the improved relaxation alone (k_batch_trilow), for tests
void batch_trilow(int device, const double* alpha, const double* beta, const int* k, int ncases, double* theta, double* vec) {
  const std::string at = "mitdvp_batch_trilow: ";
  if (ncases < 1 || ncases > BATCH_TRILOW_MAX_CASES)
    throw ArgError(at + "ncases = " + std::to_string(ncases) + ", it must be in 1 .. " + std::to_string(BATCH_TRILOW_MAX_CASES));
  if (!alpha || !beta || !k || !theta || !vec) throw ArgError(at + "null argument");
  for (int q = 0; q < ncases; ++q)
    if (k[q] < 1 || k[q] > BATCH_RELAX_MAX_KRYLOV)
      throw ArgError(at + "case " + std::to_string(q) + " has k = " + std::to_string(k[q]) + ", it must be in 1 .. " +
                     std::to_string(BATCH_RELAX_MAX_KRYLOV));
  HIP_CHECK(hipSetDevice(device));
  hipStream_t st;
  HIP_CHECK(hipStreamCreate(&st));
  {
    const size_t nv = (size_t)ncases * BATCH_RELAX_MAX_KRYLOV;
    // T of case q: its k diagonal and k - 1 off-diagonal entries, the rest of the row zeros
    std::vector<double> ha(nv, 0.0), hb(nv, 0.0);
    for (int q = 0; q < ncases; ++q)
      for (int i = 0; i < k[q]; ++i) {
        ha[(size_t)q * BATCH_RELAX_MAX_KRYLOV + i] = alpha[(size_t)q * BATCH_RELAX_MAX_KRYLOV + i];
        if (i + 1 < k[q]) hb[(size_t)q * BATCH_RELAX_MAX_KRYLOV + i] = beta[(size_t)q * BATCH_RELAX_MAX_KRYLOV + i];
      }
    DevArr<double> da, db, dth, dv;
    DevArr<int> dk;
    da.reserve(nv); db.reserve(nv); dv.reserve(nv); dth.reserve((size_t)ncases); dk.reserve((size_t)ncases);
    HIP_CHECK(hipMemcpyAsync(da, ha.data(), nv * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(db, hb.data(), nv * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dk, k, (size_t)ncases * sizeof(int), hipMemcpyHostToDevice, st));
    batch_trilow_launch(st, da, db, dk, ncases, dth, dv);
    HIP_CHECK(hipMemcpyAsync(theta, dth, (size_t)ncases * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(vec, dv, nv * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
  HIP_CHECK(hipStreamDestroy(st));
}

std::string Batch::status_message(int code) const {
  const Engine& e0 = *eng_[0];
  if (code == SS_ENOTCONV && e0.cfg.relax == 2)  // Engine::krylov_diag's words; a site of fewer elements than the cap stops at k = N
    return "Lanczos Diagonalization is not converged in " + std::to_string(e0.max_diag_krylov_) + " basis" +
           (rx_restarts_ > 0 ? " after " + std::to_string(rx_restarts_) + " restarts" : std::string());
  if (code == SS_ENOTCONV)
    return std::string(has_pairs() ? "The split of a pair channel is not converged in " + std::to_string(BATCH_PAIR_MAX_SWEEPS) + " Jacobi sweeps, or " : "") +
           std::string(e0.cfg.integrator == MITDVP_LANCZOS ? "Short Iterative Lanczos" : "Short Iterative Arnoldi") +
           " is not converged in " + std::to_string(e0.cfg.max_krylov) + " basis. Try shorter time interval.";
  if (code == SS_EZERO)
    return has_channels() ? "Initial psi has zero norm, or every operator of a jump channel gave it zero weight." : "Initial psi has zero norm.";
  return "batch: unknown status " + std::to_string(code);
}

}  // namespace mitdvp
