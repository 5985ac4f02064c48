// engine.hip -- host orchestration of the device-resident one-site TDVP sweep.
//
// Reference path being replaced (paths relative to /root/reference/pytdscf):
//   MPSCoef.propagate / propagate_along_sweep      _mps_cls.py:452-503, :798-1014
//   exp_superH/K_propagation_direct                _mps_cls.py:1016-1170
//   trans_next_psite_AsigmaB / APsiB               _mps_cls.py:1798-1850, :1172-1206
//   renormalize_op_psite / contract_with_site_mpo  _mps_mpo.py:421-696, _contraction.py:148-397
//   multiplyH/K_MPS_direct_MPO.dot                 _contraction.py:1182-1243, :1358-1407
//   short_iterative_lanczos / _arnoldi             _integrator.py:453-655, :287-432
//   SiteCoef.gauge_trf                             _site_cls.py:138-292
//
// All tensors live in HBM for the whole run; one HIP stream; the host only sees
// the O(k) Krylov scalars (k <= 20) at the points where the reference evaluates
// its convergence test.
#include "engine_internal.h"
#include "engine_krylov.inc"
#include "rccl_dyn.h"

namespace mitdvp {

Engine::Engine(const mitdvp_config& c) : cfg(c), L_(c.nsite) {
  if (c.nsite < 1) throw ArgError("nsite must be >= 1");
  if (c.max_krylov < 1 || c.max_krylov > MAXK - 1) throw ArgError("max_krylov must be in [1, 20]");
  if (c.integrator != MITDVP_LANCZOS && c.integrator != MITDVP_ARNOLDI) throw ArgError("bad integrator");
  if (c.relax < 0 || c.relax > 2) throw ArgError("relax must be 0, 1 or 2");
  max_diag_krylov_ = c.max_diag_krylov > 0 ? c.max_diag_krylov : 64;
  if (const char* e = std::getenv("MITDVP_SMALL_KERNELS")) small_kernels_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("MITDVP_SPARSE_W")) sparse_w_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("MITDVP_TRIM_IDENTITY")) trim_identity_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("MITDVP_EDGE_APPLY")) edge_mode_ = std::atoi(e);
  if (const char* e = std::getenv("MITDVP_FOLD_APPLY")) fold_mode_ = std::atoi(e);
  if (const char* e = std::getenv("MITDVP_FOLD_STRASSEN")) strassen_mode_ = std::atoi(e);
  if (const char* e = std::getenv("MITDVP_STRASSEN_BATCH")) strassen_batched_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("MITDVP_STRASSEN_FUSE")) strassen_fuse_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("MITDVP_FOLD_ENV")) fold_env_mode_ = std::atoi(e);
  if (const char* e = std::getenv("MITDVP_FOLD_ENV_REUSE")) env_reuse_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("MITDVP_CORE_LISTS")) core_lists_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("MITDVP_QR_GAUGE_FREE")) qr_gauge_free_ = std::atoi(e) != 0;
  if (const char* e = std::getenv("MITDVP_KEFF_IDENT")) keff_ident_ = std::atoi(e) != 0;
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  if (ndev < 1) throw HipError("no HIP device visible: the MI355X engine has no CPU fallback");
  if (c.device < 0 || c.device >= ndev) throw ArgError("bad device ordinal");
  HIP_CHECK(hipSetDevice(c.device));
  HIP_CHECK(hipDeviceGetAttribute(&n_cu_, hipDeviceAttributeMultiprocessorCount, c.device));
  if (c.cu_count > 0) {
    // a stream confined to the compute units [cu_first, cu_first + cu_count): mask bit u = CU u / 8 of XCD u % 8 (measured,
    // tools/cu_mask_probe.py); every XCD must keep at least one unit or the hardware falls back to units of its own choice
    if (c.cu_first < 0 || c.cu_first + c.cu_count > n_cu_ || c.cu_count % 8 != 0 || c.cu_first % 8 != 0)
      throw ArgError("cu_first / cu_count: a multiple of 8 compute units inside the device (8 k units = k CUs on every XCD)");
    std::vector<uint32_t> mask((size_t)(n_cu_ + 31) / 32, 0u);
    for (int u = c.cu_first; u < c.cu_first + c.cu_count; ++u) mask[(size_t)u / 32] |= 1u << (u % 32);
    cu_range_claim(c.device, c.cu_first, c.cu_count);  // refuses a range that overlaps another engine's
    cu_claim_.dev = c.device; cu_claim_.first = c.cu_first; cu_claim_.count = c.cu_count;
    HIP_CHECK(hipExtStreamCreateWithCUMask(&st_, (uint32_t)mask.size(), mask.data()));
    n_cu_ = c.cu_count;
    ss_.max_grid = c.cu_count;
    ss_.partitioned = true;
  } else {
    HIP_CHECK(hipStreamCreate(&st_));
  }
  qr_hist_ = qr_history_new();
  dl_.assign(L_, 0); dd_.assign(L_, 0); dr_.assign(L_, 0); gauge_.assign(L_, -1);
  site_.resize(L_);
  sub_.assign(L_, {}); subn_.assign(L_, 0);
  envL_.resize(L_ + 1); envR_.resize(L_ + 1);
  envL_ok_.assign(L_ + 1, 0); envR_ok_.assign(L_ + 1, 0);
  kprev_.assign(L_, 0);
  red_.reserve(RED_TOTAL);
  red_elems_ = RED_TOTAL;
  h_red_.alloc(RED_TOTAL * sizeof(zc));
  h_seq_.alloc(64);
  HIP_CHECK(hipMalloc((void**)&kst_, sizeof(KryDev)));
  HIP_CHECK(hipMemsetAsync(kst_, 0, sizeof(KryDev), st_));
  h_kpub_.alloc(sizeof(KryPub));
  // trivial boundary blocks, construct_op_zerosite (_mps_mpo.py:364-419)
  const zc one = make_double2(1.0, 0.0);
  envL_[0].reserve(1); envR_[L_].reserve(1);
  HIP_CHECK(hipMemcpyAsync(envL_[0].p, &one, sizeof(zc), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(envR_[L_].p, &one, sizeof(zc), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  envL_ok_[0] = 1; envR_ok_[L_] = 1;
}

Engine::~Engine() {
  if (st_) (void)hipStreamSynchronize(st_);
  small_sync_free(ss_);
  qr_history_free(qr_hist_);
  if (rccl_comm_) (void)RcclApi::get().comm_destroy(static_cast<ncclComm_t>(rccl_comm_));
  for (auto& t : pending_) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
  for (auto& e : evpool_) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  if (kst_) (void)hipFree(kst_);
  if (st_) { zgemm_release_stream(st_); (void)hipStreamDestroy(st_); }
}

// ---------------------------------------------------------------------------
DevBuf Engine::pool_get(size_t elems) {
  for (size_t i = 0; i < pool_.size(); ++i)
    if (pool_[i].n >= elems && pool_[i].n <= elems + elems / 2 + 64) {
      DevBuf b = std::move(pool_[i]);
      pool_.erase(pool_.begin() + i);
      return b;
    }
  DevBuf b;
  b.reserve(elems);
  return b;
}
void Engine::pool_put(DevBuf&& b) {
  if (b.p) pool_.push_back(std::move(b));
  if (pool_.size() > pool_cap_) pool_.erase(pool_.begin());  // adaptive ranks: block sizes drift, drop the oldest
}

void Engine::timer_begin(int kind) {
  if (!profiling_) return;
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (!evpool_.empty()) { ev = evpool_.back(); evpool_.pop_back(); }
  else { HIP_CHECK(hipEventCreate(&ev.first)); HIP_CHECK(hipEventCreate(&ev.second)); }
  HIP_CHECK(hipEventRecord(ev.first, st_));
  pending_.push_back(PhaseTimer{ev.first, ev.second, kind, false});
  cur_timer_ = (int)pending_.size() - 1;
}
void Engine::timer_end() {
  if (!profiling_ || cur_timer_ < 0) return;
  HIP_CHECK(hipEventRecord(pending_[cur_timer_].b, st_));
  pending_[cur_timer_].closed = true;
  cur_timer_ = -1;
  if (pending_.size() > 8192) resolve_timers();
}
void Engine::resolve_timers() {
  if (pending_.empty()) return;
  HIP_CHECK(hipStreamSynchronize(st_));
  for (auto& t : pending_) {
    float ms = 0;
    if (!t.closed) {  // unwound between begin and end: nothing to read, the events go back to the pool
      evpool_.emplace_back(t.a, t.b);
      continue;
    }
    HIP_CHECK(hipEventElapsedTime(&ms, t.a, t.b));
    switch (t.kind) {
      case 0: cnt_.heff_ms += ms; break;
      case 1: cnt_.env_ms += ms; break;
      case 2: cnt_.keff_ms += ms; break;
      case 3: cnt_.qr_ms += ms; break;
      case 10: case 11: case 12:
        cnt_.heff_stage_ms[t.kind - 10] += ms;
        cnt_.heff_ms += ms;
        break;
      default: cnt_.krylov_vec_ms += ms; break;
    }
    evpool_.emplace_back(t.a, t.b);
  }
  pending_.clear();
  cur_timer_ = -1;
}
void Engine::counters_get(mitdvp_counters* out) {
  ss_dirty_ = ss_dirty_ || ss_.words != nullptr;
  ss_check();  // merges the apply counts kept on the device
  resolve_timers();
  *out = cnt_;
}
void Engine::counters_reset() {
  ss_dirty_ = ss_dirty_ || ss_.words != nullptr;
  ss_check();
  resolve_timers();
  std::memset(&cnt_, 0, sizeof(cnt_));
}

// A Krylov iteration's scalars on their way to the host.  hipMemcpyAsync + hipStreamSynchronize costs ~15 us per round
// trip on this stack; a one-workgroup kernel that copies the values into the (host-coherent, device-mapped) pinned buffer
// and then bumps a sequence word the host spins on costs ~7 us (tools/probes/sync_latency.hip).  Local exponentials of the
// mid-size regime wait for three or four such round trips each.  Reads of more than 16384 elements keep the copy + synchronise form.
__global__ __launch_bounds__(256) void k_publish(const zc* __restrict__ src, zc* __restrict__ dst, size_t count,
                                                 volatile unsigned* seq, unsigned tag) {
  for (size_t e = threadIdx.x; e < count; e += 256) dst[e] = src[e];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) *seq = tag;
}

void Engine::read_partials(size_t off, size_t count) {
  cnt_.n_host_waits += 1;
  if (count <= 16384) {
    const unsigned tag = ++seq_tag_;
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(256), 0, st_, red_.p + off, h_red_.d + off, count, h_seq_.d, tag);
    HIP_CHECK(hipGetLastError());
    wait_published(st_, h_seq_.h, tag, "read_partials: the publish kernel did not deliver");
    return;
  }
  HIP_CHECK(hipMemcpyAsync(h_red_.h + off, red_.p + off, count * sizeof(zc), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}

void Engine::wait_pub(unsigned tag) {
  wait_published(st_, &h_kpub_.h->seq, tag, "wait_pub: the Krylov record was not published");
}

// ---------------------------------------------------------------------------
// state
// ---------------------------------------------------------------------------
void Engine::set_site(int i, const double* reim, int l, int n, int r, int gauge) {
  if (i < 0 || i >= L_) throw ArgError("set_site: bad site index");
  if (l < 1 || n < 1 || r < 1) throw ArgError("set_site: bad shape");
  const size_t e = (size_t)l * n * r;
  site_[i].reserve(e);
  copy_in(site_[i].p, reim, e);
  dl_[i] = l; dd_[i] = n; dr_[i] = r; gauge_[i] = gauge;
  if (gauge == MITDVP_GAUGE_PSI) center_ = i;
  invalidate_env();
}
void Engine::get_site_shape(int i, int* l, int* n, int* r, int* gauge) const {
  if (i < 0 || i >= L_) throw ArgError("get_site_shape: bad site index");
  *l = dl_[i]; *n = dd_[i]; *r = dr_[i]; *gauge = gauge_[i];
}
void Engine::get_site(int i, double* out) {
  if (i < 0 || i >= L_ || !site_[i].p) throw ArgError("get_site: bad or unset site");
  const size_t e = (size_t)dl_[i] * dd_[i] * dr_[i];
  copy_out(out, site_[i].p, e);
}

void Engine::set_pointer_mode(int mode) {
  if (mode != 0 && mode != 1) throw ArgError("set_pointer_mode: 0 (host) or 1 (device)");
  ptr_mode_ = mode;
}
void Engine::copy_in(zc* dst, const double* src, size_t elems) {
  if (ptr_mode_ == 0) HIP_CHECK(hipMemcpyAsync(dst, src, elems * sizeof(zc), hipMemcpyHostToDevice, st_));
  else vec_copy_raw(st_, dst, reinterpret_cast<const zc*>(src), elems);
  HIP_CHECK(hipStreamSynchronize(st_));
}
void Engine::copy_out(double* dst, const zc* src, size_t elems) {
  if (ptr_mode_ == 0) HIP_CHECK(hipMemcpyAsync(dst, src, elems * sizeof(zc), hipMemcpyDeviceToHost, st_));
  else vec_copy_raw(st_, reinterpret_cast<zc*>(dst), src, elems);
  HIP_CHECK(hipStreamSynchronize(st_));
}

Operator& Engine::op(int id) {
  auto it = ops_.find(id);
  if (it == ops_.end()) {
    Operator o;
    o.sites.resize(L_);
    it = ops_.emplace(id, std::move(o)).first;
  }
  return it->second;
}
const MpoSite& Engine::mpo(int op_id, int isite) {
  auto it = ops_.find(op_id);
  if (it == ops_.end() || !it->second.sites[isite].set) throw ArgError("operator core not set for this site");
  return it->second.sites[isite];
}

void Engine::upload_mpo_core(MpoSite& s, const double* reim, int ml, int dout, int din, int mr) {
  if (ml < 1 || mr < 1 || dout < 1 || dout != din) throw ArgError("set_mpo_core: need a square 4-leg core");
  const int d = dout;
  const hzc* W = reinterpret_cast<const hzc*>(reim);
  std::vector<hzc> w2l((size_t)d * mr * ml * d), w2r((size_t)d * ml * mr * d);
  std::vector<hzc> w2el(w2l.size()), w2er(w2r.size());
  for (int c = 0; c < ml; ++c)
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < d; ++j)
        for (int t = 0; t < mr; ++t) {
          const hzc v = W[(((size_t)c * d + i) * d + j) * mr + t];
          w2l[((size_t)i * mr + t) * ((size_t)ml * d) + (size_t)c * d + j] = v;
          w2r[((size_t)i * ml + c) * ((size_t)mr * d) + (size_t)t * d + j] = v;
          w2el[((size_t)t * d + j) * ((size_t)d * ml) + (size_t)i * ml + c] = v;
          w2er[((size_t)c * d + j) * ((size_t)d * mr) + (size_t)i * mr + t] = v;
        }
  s.ml = ml; s.d = d; s.mr = mr;
  s.w2l.reserve(w2l.size());
  s.w2r.reserve(w2r.size());
  HIP_CHECK(hipMemcpyAsync(s.w2l.p, w2l.data(), w2l.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(s.w2r.p, w2r.data(), w2r.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
  // block-sparse forms: rows (t, i) for W2L, (c, i) for W2R; K-tile lists on the 64 x 16 tile grid
  auto sparse_form = [&](const std::vector<hzc>& w2, int mo, int mi, DevBuf& wt, DevBuf& kl, int& stride, double& frac,
                         std::vector<MpoSite::SpSeg>& segs) {
    // w2: rows (i, q) with q in [0, mo), cols (p, j) with p in [0, mi); permuted rows (q, i)
    const int M = d * mo, K = mi * d;
    frac = 1.0; stride = 0; segs.clear();
    if (K % 16 != 0) return;
    std::vector<hzc> p((size_t)M * K);
    for (int i = 0; i < d; ++i)
      for (int q = 0; q < mo; ++q)
        std::memcpy(&p[((size_t)q * d + i) * K], &w2[((size_t)i * mo + q) * K], (size_t)K * sizeof(hzc));
    const int nkt = K / 16;
    stride = nkt + 1;
    // per bond state q (rows [q d, (q + 1) d)): the K tiles that hold a non-zero
    std::vector<std::vector<char>> need(mo, std::vector<char>(nkt, 0));
    std::vector<int> cntq(mo, 0);
    for (int q = 0; q < mo; ++q) {
      for (int kt = 0; kt < nkt; ++kt) {
        bool nz = false;
        for (int r = q * d; r < (q + 1) * d && !nz; ++r)
          for (int k = kt * 16; k < kt * 16 + 16; ++k)
            if (p[(size_t)r * K + k] != hzc(0.0, 0.0)) { nz = true; break; }
        need[q][kt] = nz;
        cntq[q] += nz;
      }
    }
    std::vector<int> list;
    long executed = 0;  // in units of (row, K tile), padding rows of the tiles included: the flop the hardware runs
    for (int q0 = 0; q0 < mo;) {
      const bool dense = 2 * cntq[q0] > nkt;
      int q1 = q0 + 1;
      while (q1 < mo && (2 * cntq[q1] > nkt) == dense) ++q1;
      MpoSite::SpSeg sg{q0 * d, q1 * d, dense, 0};
      if (dense) {
        // what the matrix cores execute: whole tiles (32 rows for a range of <= 32 rows, else 64: w_stage's choice)
        const int rows = sg.r1 - sg.r0, tile = rows <= 32 ? 32 : 64;
        executed += (long)((rows + tile - 1) / tile) * tile * nkt;
      } else {
        sg.tile0 = (int)(list.size() / stride);
        for (int r = sg.r0; r < sg.r1; r += 64) {  // this range's own grid of 64-row tiles
          const size_t o = list.size();
          list.resize(o + stride, 0);
          int cnt = 0;
          for (int kt = 0; kt < nkt; ++kt) {
            bool nz = false;
            for (int q = r / d; q <= (std::min(r + 64, sg.r1) - 1) / d && !nz; ++q) nz = need[q][kt];
            if (nz) list[o + 1 + cnt++] = kt;
          }
          list[o] = cnt;
          executed += 64L * cnt;  // a tile runs all its 64 rows through every listed K tile
        }
      }
      segs.push_back(sg);
      q0 = q1;
    }
    if (list.empty()) list.assign(stride, 0);
    frac = (double)executed / ((double)M * nkt);
    wt.reserve(p.size());
    kl.reserve((list.size() * sizeof(int) + sizeof(zc) - 1) / sizeof(zc));
    HIP_CHECK(hipMemcpyAsync(wt.p, p.data(), p.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(kl.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipStreamSynchronize(st_));  // the host vectors go out of scope
  };
  sparse_form(w2l, mr, ml, s.w2lt, s.kl_l, s.kl_stride_l, s.sp_frac_l, s.seg_l);
  sparse_form(w2r, ml, mr, s.w2rt, s.kl_r, s.kl_stride_r, s.sp_frac_r, s.seg_r);
  // what the edge form of an apply needs (heff_apply_edge): the core itself and the map of its non-zero blocks
  s.whost.clear(); s.nzblk.clear(); s.edge.valid = false; s.edge.skip = 0;
  if (ml <= 64 && mr <= 64) {
    s.whost.assign(W, W + (size_t)ml * d * d * mr);
    s.nzblk.assign((size_t)ml * mr, 0);
    for (int c = 0; c < ml; ++c)
      for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j)
          for (int t = 0; t < mr; ++t)
            if (W[(((size_t)c * d + i) * d + j) * mr + t] != hzc(0.0, 0.0)) s.nzblk[(size_t)c * mr + t] = 1;
  }
  s.w2el.reserve(w2el.size());
  s.w2er.reserve(w2er.size());
  HIP_CHECK(hipMemcpyAsync(s.w2el.p, w2el.data(), w2el.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipMemcpyAsync(s.w2er.p, w2er.data(), w2er.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  s.set = true;
}

void Engine::set_mpo_core(int op_id, int isite, const double* reim, int ml, int dout, int din, int mr) {
  if (isite < 0 || isite >= L_) throw ArgError("set_mpo_core: bad site index");
  upload_mpo_core(op(op_id).sites[isite], reim, ml, dout, din, mr);
  if (op_id == 0) invalidate_env();
}
void Engine::set_shift(int op_id, double re, double im) { op(op_id).shift = hzc(re, im); }

void Engine::invalidate_env() {
  (void)take_env_checked();  // the blocks a check described go back to the pool: their addresses may come back with other contents
  for (int b = 1; b < L_; ++b) {
    envL_ok_[b] = 0; envR_ok_[b] = 0;
    pool_put(std::move(envL_[b]));
    pool_put(std::move(envR_[b]));
  }
}

void Engine::ensure_work(long max_site, long max_x, long max_y, int max_qr_m, int max_qr_n, int qr_next) {
  X_.reserve(max_x);
  Y_.reserve(max_y);
  V_.reserve((size_t)MAXK * max_site);
  tmp1_.reserve(max_site);
  tmp2_.reserve(max_site);
  const size_t dd = (size_t)max_qr_n * max_qr_n;
  sig_.reserve(std::max<size_t>(dd, 1));
  sig2_.reserve(std::max<size_t>(dd, 1));
  qrwork_.reserve(qr_work_elems(max_qr_m, max_qr_n, qr_next));
}

void Engine::size_workspaces() {
  long ms = 1, mx = 1, my = 1;
  int qm = 1, qn = 1;
  for (int p = 0; p < L_; ++p) {
    const long s = (long)dl_[p] * dd_[p] * dr_[p];
    ms = std::max(ms, s);
    qm = std::max(qm, std::max(dl_[p], dr_[p]) * dd_[p]);
    qn = std::max(qn, std::max(dl_[p], dr_[p]));
    for (auto& kv : ops_) {
      const MpoSite& w = kv.second.sites[p];
      if (!w.set) continue;
      const long mm = std::max(w.ml, w.mr);
      mx = std::max(mx, (long)dl_[p] * dr_[p] * dd_[p] * mm);
      my = std::max(my, (long)dl_[p] * dr_[p] * dd_[p] * mm);
    }
  }
  ensure_work(ms, mx, my, qm, qn);
  // site buffers are exchanged with a spare of capacity max_site during the
  // sweep (QR / absorb write into the spare, then swap): give all of them that
  // capacity so that any of them can play the spare's role afterwards.
  for (int p = 0; p < L_; ++p)
    if (site_[p].p) site_[p].grow_preserve((size_t)ms, (size_t)dl_[p] * dd_[p] * dr_[p], st_);
}

void Engine::require_ready(bool open_ends) {
  for (int p = 0; p < L_; ++p) {
    if (!site_[p].p) throw ArgError("site tensor not set");
    if (p + 1 < L_ && dr_[p] != dl_[p + 1]) throw ArgError("bond dimension mismatch between neighbouring sites");
  }
  if (!segment_) {
    if (!open_ends && (dl_[0] != 1 || dr_[L_ - 1] != 1)) throw ArgError("open boundary bonds must be 1");
  } else if ((envL_ok_[0] && bnd_dl_ != dl_[0]) || (envR_ok_[L_] && bnd_dr_ != dr_[L_ - 1])) {
    throw ArgError("segment: the outer bonds differ from the boundary blocks' dimension");
  }
  size_workspaces();
  ss_refresh_plan();
}

// ---------------------------------------------------------------------------
// bond-sharded execution over several GPUs (one process per GPU)
//
// The three contractions of an apply / environment update are independent for
// every value of the leading (bra-side) bond index of the environment block, so
// rank r computes the rows a in [r*n/N, (r+1)*n/N) from replicated operands and
// the ranks exchange results with ONE collective per contraction chain:
//   H_eff / K_eff apply : in-place all-gather of the result vector
//   environment update  : in-place all-reduce (sum over the sharded bra index)
// Everything else (Krylov vector algebra, QR, absorption) is computed
// redundantly on identical data, so all ranks take identical control-flow
// decisions without exchanging scalars.  The collective itself is a callback
// (RCCL through torch.distributed in production, gloo in the 1-GPU tests).
// ---------------------------------------------------------------------------
void Engine::set_parallel(int nranks, int rank, CollFn fn, void* user) {
  if (nranks < 1 || rank < 0 || rank >= nranks) throw ArgError("set_parallel: bad rank / nranks");
  if (nranks > 1 && !fn) throw ArgError("set_parallel: a collective callback is required for nranks > 1");
  if (rccl_comm_) { (void)RcclApi::get().comm_destroy(static_cast<ncclComm_t>(rccl_comm_)); rccl_comm_ = nullptr; }
  nranks_ = nranks; rank_ = rank; coll_ = fn; coll_user_ = user;
}

bool Engine::shard_range(int n, int& a0, int& a1) const {
  a0 = 0; a1 = n;
  if (nranks_ <= 1 || n % nranks_ != 0 || n < 8 * nranks_) return false;  // small / ragged bonds stay replicated
  const int c = n / nranks_;
  a0 = rank_ * c; a1 = a0 + c;
  return true;
}

void Engine::collective(int op, zc* p, size_t elems) {
  if (rccl_comm_) {
    // native path: stream-ordered RCCL collectives on the engine's own stream -- no host
    // synchronisation, the Krylov loop stays asynchronous between its convergence checks
    const RcclApi& r = RcclApi::get();
    ncclComm_t comm = static_cast<ncclComm_t>(rccl_comm_);
    const size_t n = elems * 2;  // float64 values
    if (op == COLL_ALLGATHER) {
      const size_t chunk = n / nranks_;
      double* base = reinterpret_cast<double*>(p);
      rccl_check(r.all_gather(base + (size_t)rank_ * chunk, base, chunk, ncclDouble, comm, st_), "ncclAllGather");
    } else {
      rccl_check(r.all_reduce(p, p, n, ncclDouble, ncclSum, comm, st_), "ncclAllReduce");
    }
  } else {
    HIP_CHECK(hipStreamSynchronize(st_));
    const int rc = coll_(coll_user_, op, p, elems * sizeof(zc));
    if (rc != 0) throw HipError("collective callback failed (rc=" + std::to_string(rc) + ")");
  }
  cnt_.n_collectives += 1;
  cnt_.collective_bytes += (double)(elems * sizeof(zc));
}

// RCCL communicator owned by the engine (one process per GPU; `id` = the 128 bytes of an
// ncclUniqueId created on one rank by rccl_unique_id() and distributed out of band)
void Engine::rccl_unique_id(char out[128]) {
  ncclUniqueId id;
  rccl_check(RcclApi::get().get_unique_id(&id), "ncclGetUniqueId");
  static_assert(sizeof(id.internal) == 128, "ncclUniqueId size");
  std::memcpy(out, id.internal, 128);
}

void Engine::set_parallel_rccl(int nranks, int rank, const char id_bytes[128]) {
  if (nranks < 1 || rank < 0 || rank >= nranks) throw ArgError("set_parallel_rccl: bad rank / nranks");
  const RcclApi& r = RcclApi::get();
  if (rccl_comm_) { (void)r.comm_destroy(static_cast<ncclComm_t>(rccl_comm_)); rccl_comm_ = nullptr; }
  ncclUniqueId id;
  std::memcpy(id.internal, id_bytes, 128);
  ncclComm_t comm = nullptr;
  rccl_check(r.comm_init_rank(&comm, nranks, id, rank), "ncclCommInitRank");
  rccl_comm_ = comm;
  nranks_ = nranks; rank_ = rank; coll_ = nullptr; coll_user_ = nullptr;
}

// both collectives on a small device buffer: returns 0 when the gathered / reduced values are right
int Engine::rccl_selftest() {
  if (!rccl_comm_) throw ArgError("rccl_selftest: no RCCL communicator (call set_parallel_rccl)");
  const int per = 8;
  std::vector<hzc> h((size_t)nranks_ * per, hzc(-1.0, -1.0));
  for (int i = 0; i < per; ++i) h[(size_t)rank_ * per + i] = hzc(rank_ + 1.0, 0.5);
  DevBuf b = pool_get(h.size());
  HIP_CHECK(hipMemcpyAsync(b.p, h.data(), h.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
  collective(COLL_ALLGATHER, b.p, h.size());
  HIP_CHECK(hipMemcpyAsync(h.data(), b.p, h.size() * sizeof(zc), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  int bad = 0;
  for (int r = 0; r < nranks_; ++r)
    for (int i = 0; i < per; ++i) bad += h[(size_t)r * per + i] != hzc(r + 1.0, 0.5);
  for (auto& x : h) x = hzc(rank_ + 1.0, 1.0);
  HIP_CHECK(hipMemcpyAsync(b.p, h.data(), h.size() * sizeof(zc), hipMemcpyHostToDevice, st_));
  collective(COLL_ALLREDUCE, b.p, h.size());
  HIP_CHECK(hipMemcpyAsync(h.data(), b.p, h.size() * sizeof(zc), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  const hzc want(nranks_ * (nranks_ + 1) / 2.0, (double)nranks_);
  for (auto& x : h) bad += x != want;
  pool_put(std::move(b));
  return bad;
}

// ---------------------------------------------------------------------------
// gauge moves
// ---------------------------------------------------------------------------
void Engine::gauge_qr_left(const zc* psi, int dl, int d, int dr, zc* A_out, zc* sigma_out) {
  const long n = (long)dl * d * dr;
  HIP_CHECK(hipMemcpyAsync(tmp1_.p, psi, n * sizeof(zc), hipMemcpyDeviceToDevice, st_));
  timer_begin(3);
  long nl = 0;
  qr_thin(st_, tmp1_.p, dl * d, dr, A_out, sigma_out, qrwork_.p, &nl, qr_hist_, qr_gauge_free_);
  timer_end();
  cnt_.n_launch += nl;
  cnt_.n_qr += 1;
  const double m = (double)dl * d, nn = dr;
  cnt_.qr_flops += 4.0 * (4.0 * m * nn * nn - 4.0 * nn * nn * nn / 3.0);
}

void Engine::gauge_qr_right(const zc* psi, int dl, int d, int dr, zc* B_out, zc* Bt_out, zc* sigma_out) {
  timer_begin(3);
  long nl = 0;
  transpose_rev3(st_, psi, tmp1_.p, dl, d, dr);  // (dr, d, dl)
  qr_thin(st_, tmp1_.p, dr * d, dl, Bt_out, sig2_.p, qrwork_.p, &nl, qr_hist_, qr_gauge_free_);
  transpose_batched(st_, sig2_.p, sigma_out, dl, dl, dl, dl, 1, 0, 0);  // sigma = R^T
  if (B_out) transpose_rev3(st_, Bt_out, B_out, dr, d, dl);             // (dl, d, dr)
  timer_end();
  cnt_.n_launch += nl + 3;
  cnt_.n_qr += 1;
  const double m = (double)dr * d, nn = dl;
  cnt_.qr_flops += 4.0 * (4.0 * m * nn * nn - 4.0 * nn * nn * nn / 3.0);
}

// ---------------------------------------------------------------------------
// initial state
// ---------------------------------------------------------------------------
void Engine::init_random(const int* dims, int D, uint64_t seed) {
  if (D < 1) throw ArgError("bond_dim must be >= 1");
  // LatticeInfo.get_bond_dim (_mps_cls.py:2616-2631), products saturated at D
  auto satprod = [&](int lo, int hi) {
    double p = 1;
    for (int i = lo; i < hi; ++i) { p *= dims[i]; if (p > D) return (long)D + 1; }
    return (long)p;
  };
  for (int i = 0; i < L_; ++i) {
    if (dims[i] < 1) throw ArgError("bad physical dimension");
    const long left = i == 0 ? 1 : std::min<long>(D, satprod(0, i));
    const long right = i == L_ - 1 ? 1 : std::min<long>(D, satprod(i + 1, L_));
    const long dc = dims[i];
    dl_[i] = (int)std::min({left, dc * right, (long)D});
    dr_[i] = (int)std::min({left * dc, right, (long)D});
    dd_[i] = dims[i];
    const size_t e = (size_t)dl_[i] * dd_[i] * dr_[i];
    site_[i].reserve(e);
    vec_randn(st_, site_[i].p, (long)e, seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1));
    gauge_[i] = -1;
  }
  invalidate_env();
  canonicalize(1.0);
}

// The raw (not canonicalised) random tensors of sites [first, first + L_) of an ntot-site chain: shapes and seeds by the
// GLOBAL site index, i.e. what init_random draws for those sites before it canonicalises -- a rank of a site-sharded
// state fills only its own block and the ranks canonicalise in a pipeline (parallel_sites.py).  balance: every tensor is
// multiplied by the largest power of two <= 1 / sqrt(d_l d) (exact in floating point; the right-canonical factors do not
// change, the weight passed on along the chain stays O(1) instead of growing by ~sqrt(D d D) per site).
void Engine::init_random_block(const int* dims, int ntot, int first, int D, uint64_t seed, bool balance) {
  if (D < 1) throw ArgError("bond_dim must be >= 1");
  if (first < 0 || first + L_ > ntot) throw ArgError("init_random_block: the block lies outside the chain");
  auto satprod = [&](int lo, int hi) {
    double p = 1;
    for (int i = lo; i < hi; ++i) { p *= dims[i]; if (p > D) return (long)D + 1; }
    return (long)p;
  };
  for (int q = 0; q < L_; ++q) {
    const int i = first + q;
    if (dims[i] < 1) throw ArgError("bad physical dimension");
    const long left = i == 0 ? 1 : std::min<long>(D, satprod(0, i));
    const long right = i == ntot - 1 ? 1 : std::min<long>(D, satprod(i + 1, ntot));
    const long dc = dims[i];
    dl_[q] = (int)std::min({left, dc * right, (long)D});
    dr_[q] = (int)std::min({left * dc, right, (long)D});
    dd_[q] = dims[i];
    const size_t e = (size_t)dl_[q] * dd_[q] * dr_[q];
    site_[q].reserve(e);
    vec_randn(st_, site_[q].p, (long)e, seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1));
    if (balance) {
      int ex = 0;
      (void)std::frexp(1.0 / std::sqrt((double)dl_[q] * dd_[q]), &ex);  // 1 / sqrt = m 2^ex, m in [0.5, 1)
      vec_scale(st_, site_[q].p, (long)e, make_double2(std::ldexp(1.0, ex - 1), 0.0));
    }
    gauge_[q] = -1;
  }
  center_ = -1;
  bond_ = -1;
  invalidate_env();
}

void Engine::canonicalize(double scale) {
  require_ready();
  DevBuf spare = pool_get(V_.n / MAXK);
  double log_scale = 0.0;
  for (int p = L_ - 1; p > 0; --p) {
    const int dl = dl_[p], d = dd_[p], dr = dr_[p];
    // C2sigmaB (_mps_cls.py:2684-2693)
    gauge_qr_right(site_[p].p, dl, d, dr, spare.p, tmp2_.p, sig_.p);
    std::swap(site_[p], spare);
    gauge_[p] = MITDVP_GAUGE_B;
    // sigma is rescaled to unit Frobenius norm on the device (unnormalised, e.g.
    // random, cores would otherwise grow geometrically along a long chain and
    // overflow); the factors are accumulated on the host for scale <= 0 (keep the
    // state's own normalisation: Liouville space, _mps_cls.py:2695-2699)
    {
      double* nrm = reinterpret_cast<double*>(red_.p + RED_MISC);
      vec_sumsq(st_, sig_.p, (long)dl * dl, nrm);
      vec_scale_inv_norm(st_, sig_.p, (long)dl * dl, nrm, 1e-300);
      if (scale <= 0.0) {
        read_partials(RED_MISC, NPART / 2);
        const double* hp = reinterpret_cast<const double*>(h_red_.h + RED_MISC);
        double t = 0;
        for (int i = 0; i < NPART; ++i) t += hp[i];
        if (t > 0) log_scale += 0.5 * std::log(t);
      }
    }
    // site[p-1] <- site[p-1] . sigma
    const int m = dl_[p - 1] * dd_[p - 1];
    ZgemmDesc g = zgemm_desc(site_[p - 1].p, sig_.p, spare.p, m, dl, dl);
    zgemm(st_, g);
    std::swap(site_[p - 1], spare);
    cnt_.n_launch += 1;
  }
  pool_put(std::move(spare));
  const long n0 = (long)dl_[0] * dd_[0] * dr_[0];
  vec_sumsq(st_, site_[0].p, n0, reinterpret_cast<double*>(red_.p + RED_MISC));
  read_partials(RED_MISC, NPART / 2);
  const double* hp = reinterpret_cast<const double*>(h_red_.h + RED_MISC);
  double s = 0;
  for (int i = 0; i < NPART; ++i) s += hp[i];
  if (s == 0.0) throw ArgError("canonicalize: zero state");
  if (scale > 0.0)
    vec_scale(st_, site_[0].p, n0, make_double2(scale / std::sqrt(s), 0.0));
  else
    vec_scale(st_, site_[0].p, n0, make_double2(std::exp(log_scale), 0.0));
  gauge_[0] = MITDVP_GAUGE_PSI;
  center_ = 0;
  invalidate_env();
}

// ---------------------------------------------------------------------------
// sweep
// ---------------------------------------------------------------------------
hzc Engine::scale_site(double dt) const { return cfg.relax ? hzc(-dt / 2, 0.0) : hzc(0.0, -dt / 2); }  // :1070 / :1088
hzc Engine::scale_bond(double dt) const { return cfg.relax ? hzc(+dt / 2, 0.0) : hzc(0.0, +dt / 2); }

void Engine::build_right_envs() {
  // construct_op_sites(begin=L-1, end=0) (_mps_cls.py:835-843, :1738-1796)
  for (int p = L_ - 1; p >= 1; --p) {
    if (envR_ok_[p]) continue;
    if (!envR_ok_[p + 1]) throw ArgError("internal: right environment chain broken");
    if (gauge_[p] != MITDVP_GAUGE_B) throw ArgError("sites right of the centre must be in gauge B");
    const MpoSite& w = mpo(0, p);
    transpose_rev3(st_, site_[p].p, tmp1_.p, dl_[p], dd_[p], dr_[p]);
    envR_[p] = pool_get((size_t)dl_[p] * w.ml * dl_[p]);
    env_update(envR_[p + 1].p, tmp1_.p, w.w2r.p, envR_[p].p, dr_[p], w.mr, dd_[p], dl_[p], w.ml, w.w2er.p, &w, 1);
    envR_ok_[p] = 1;
  }
}

void Engine::build_left_envs() {
  // construct_op_sites(begin=0, end=L-1): needed when a gate / Kraus map re-orthogonalised
  // sites after the forward half-sweep (op_sys_sites = None, _mps_cls.py:2370)
  for (int p = 0; p < L_ - 1; ++p) {
    if (envL_ok_[p + 1]) continue;
    if (!envL_ok_[p]) throw ArgError("internal: left environment chain broken");
    if (gauge_[p] != MITDVP_GAUGE_A) throw ArgError("sites left of the centre must be in gauge A");
    const MpoSite& w = mpo(0, p);
    pool_put(std::move(envL_[p + 1]));
    envL_[p + 1] = pool_get((size_t)dr_[p] * w.mr * dr_[p]);
    env_update(envL_[p].p, site_[p].p, w.w2l.p, envL_[p + 1].p, dl_[p], w.ml, dd_[p], dr_[p], w.mr, w.w2el.p, &w, 0);
    envL_ok_[p + 1] = 1;
  }
}

void Engine::local_site_exp(int p, double dt) {
  const MpoSite& w = mpo(0, p);
  if (dd_[p] != w.d) throw ArgError("MPO physical dimension differs from the site tensor's");
  if (small_site_exp(p, dt)) return;  // one launch, no host round trip
  const int dl = dl_[p], d = dd_[p], dr = dr_[p];
  const zc* Lb = envL_[p].p;
  const zc* Rb = envR_[p + 1].p;
  const hzc shift = op(0).shift;
  // large bonds: one check per site (two tiny launches and a synchronisation) buys 1 / M_r of stage S3 in every apply
  const ApplyPlan plan = choose_apply_forms(Lb, w, Rb, dl, d, dr);
  auto mv = [&](const zc* in, zc* out) { heff_apply(Lb, w, Rb, in, out, dl, d, dr, shift, plan); };
  if (cfg.relax == 2)  // improved relaxation, _mps_cls.py:1078-1084
    kprev_[p] = krylov_diag(mv, site_[p].p, (long)dl * d * dr);
  else
    kprev_[p] = krylov_exp(scale_site(dt), mv, site_[p].p, (long)dl * d * dr, kprev_[p]);
  cnt_.n_exp_site += 1;
}

void Engine::sweep(double dt, bool forward) {
  if (sw_next_ >= 0) throw ArgError("sweep: a half-sweep in parts is in progress");
  sweep_part(dt, forward, L_);
}

// The half-sweep's loop, resumable: a call runs the next `nsites` sites of the half-sweep in progress (starting one when
// none is) and returns how many are left; sweep() is one call over all L sites.
int Engine::sweep_part(double dt, bool forward, int nsites) {
  if (nsites < 1) throw ArgError("sweep_part: nsites must be >= 1");
  const int begin = forward ? 0 : L_ - 1, end = forward ? L_ - 1 : 0;
  if (sw_next_ < 0) {
    require_ready();
    if (L_ == 1) {
      if (center_ != 0) throw ArgError("no centre site");
      local_site_exp(0, dt);
      ss_check();
      return 0;
    }
    if (center_ != begin) throw ArgError("sweep must start at the centre (Psi) site");
    if (forward) build_right_envs();
    else build_left_envs();
    if (adaptive_) {
      if (cfg.relax) throw ArgError("adaptive bond dimension is implemented for real-time propagation only");
      adaptive_prepare();
      build_superblock_full(forward);
    }
    sw_spare_ = pool_get(V_.n / MAXK);
    sw_next_ = begin;
    sw_fwd_ = forward;
  } else if (forward != sw_fwd_ || center_ != sw_next_) {
    throw ArgError("sweep_part: the half-sweep in progress runs the other way or its state has moved");
  }
  const hzc shift = op(0).shift;
  DevBuf& spare = sw_spare_;
  const int stop = forward ? std::min(end, sw_next_ + nsites - 1) : std::max(end, sw_next_ - nsites + 1);
  try {
  for (int p = sw_next_; forward ? p <= stop : p >= stop; p += forward ? 1 : -1) {
    if (adaptive_ && p != end && adaptive_site(p, dt, forward, spare)) continue;
    local_site_exp(p, dt);  // exp_superH_propagation_direct
    if (p == end) break;
    const MpoSite& w = mpo(0, p);
    const int dl = dl_[p], d = dd_[p], dr = dr_[p];
    if (forward) {
      // Psi2Asigma: site[p] (destroyed) -> A in spare, sigma in sig_
      timer_begin(3);
      long nl = 0;
      qr_thin(st_, site_[p].p, dl * d, dr, spare.p, sig_.p, qrwork_.p, &nl, qr_hist_, qr_gauge_free_);
      timer_end();
      cnt_.n_launch += nl; cnt_.n_qr += 1;
      cnt_.qr_flops += 4.0 * (4.0 * (double)dl * d * dr * dr - 4.0 * (double)dr * dr * dr / 3.0);
      std::swap(site_[p], spare);
      gauge_[p] = MITDVP_GAUGE_A;
      // renormalize_op_psite: L_{p+1}
      envL_[p + 1] = pool_get((size_t)dr * w.mr * dr);
      env_update(envL_[p].p, site_[p].p, w.w2l.p, envL_[p + 1].p, dl, w.ml, d, dr, w.mr, w.w2el.p, &w, 0);
      envL_ok_[p + 1] = 1;
      // exp(+i K dt/2) on the bond matrix
      const zc* Lb = envL_[p + 1].p;
      const zc* Rb = envR_[p + 1].p;
      const int m = w.mr;
      if (cfg.relax != 2 && !small_bond_exp(p, Lb, Rb, dr, m, dt)) {  // improved relaxation leaves the bond matrix alone (_mps_cls.py:1159-1160)
        const KeffCompact* kc = keff_prepare(Lb, Rb, dr, dr, m);  // identity states of the two blocks: skipped in every apply of this solve
        auto mk = [&](const zc* in, zc* out) { keff_apply(Lb, Rb, in, out, dr, dr, m, shift, kc); };
        kprev_[p] = krylov_exp(scale_bond(dt), mk, sig_.p, (long)dr * dr, kprev_[p]);
        cnt_.n_exp_bond += 1;
      }
      envR_ok_[p + 1] = 0;
      pool_put(std::move(envR_[p + 1]));
      // trans_next_psite_APsiB: Psi(p+1) = sigma . B(p+1)
      ZgemmDesc g = zgemm_desc(sig_.p, site_[p + 1].p, spare.p, dr, dd_[p + 1] * dr_[p + 1], dr);
      zgemm(st_, g);
      cnt_.n_launch += 1;
      std::swap(site_[p + 1], spare);
      gauge_[p + 1] = MITDVP_GAUGE_PSI;
      center_ = p + 1;
    } else {
      // Psi2sigmaB: B in spare, mirrored B~ (dr,d,dl) in tmp2_, sigma (dl x dl) in sig_
      gauge_qr_right(site_[p].p, dl, d, dr, spare.p, tmp2_.p, sig_.p);
      std::swap(site_[p], spare);
      gauge_[p] = MITDVP_GAUGE_B;
      envR_[p] = pool_get((size_t)dl * w.ml * dl);
      env_update(envR_[p + 1].p, tmp2_.p, w.w2r.p, envR_[p].p, dr, w.mr, d, dl, w.ml, w.w2er.p, &w, 1, site_[p].p);
      envR_ok_[p] = 1;
      const zc* Lb = envL_[p].p;
      const zc* Rb = envR_[p].p;
      const int m = w.ml;
      if (cfg.relax != 2 && !small_bond_exp(p, Lb, Rb, dl, m, dt)) {
        const KeffCompact* kc = keff_prepare(Lb, Rb, dl, dl, m);
        auto mk = [&](const zc* in, zc* out) { keff_apply(Lb, Rb, in, out, dl, dl, m, shift, kc); };
        kprev_[p] = krylov_exp(scale_bond(dt), mk, sig_.p, (long)dl * dl, kprev_[p]);
        cnt_.n_exp_bond += 1;
      }
      envL_ok_[p] = 0;
      pool_put(std::move(envL_[p]));
      // Psi(p-1) = A(p-1) . sigma
      ZgemmDesc g = zgemm_desc(site_[p - 1].p, sig_.p, spare.p, dl_[p - 1] * dd_[p - 1], dl, dl);
      zgemm(st_, g);
      cnt_.n_launch += 1;
      std::swap(site_[p - 1], spare);
      gauge_[p - 1] = MITDVP_GAUGE_PSI;
      center_ = p - 1;
    }
  }
  } catch (...) {  // a failed local update ends the half-sweep, as it did when the loop was one call
    sw_next_ = -1;
    DevBuf drop = std::move(sw_spare_);
    throw;
  }
  if (stop != end) {
    sw_next_ = stop + (forward ? 1 : -1);
    return forward ? end - sw_next_ + 1 : sw_next_ - end + 1;
  }
  sw_next_ = -1;
  pool_put(std::move(sw_spare_));
  ss_check();  // the one host synchronisation of a small-bond sweep: errors raised on the device
  return 0;
}

void Engine::step(double dt) {
  sweep(dt, true);
  apply_gates();  // Model(one_gate_to_apply=...), _mps_cls.py:489-490 (reorth_center = nsite - 1)
  apply_kraus();  // Model(kraus_op=...), :491-492
  sweep(dt, false);
}

}  // namespace mitdvp
