// capi.hip -- extern "C" surface declared in include/mitdvp.h.
#include <mutex>
#include <thread>
#include <vector>

#include "capi_internal.h"
#include "engine_batch.h"
#include "engine_internal.h"
#include "engine_krylov.inc"
#include "vecop_check.h"
#include "zgemm_args_check.h"
#include "zgemm_reduce_args_check.h"

namespace {
thread_local std::string g_err;

template <class F>
int guard(mitdvp_engine* h, F&& f) {
  std::string* dst = h ? &h->err : &g_err;
  try {
    if (h) {
      hipError_t e = hipSetDevice(h->device);
      if (e != hipSuccess) { *dst = hipGetErrorString(e); return MITDVP_EHIP; }
    }
    f();
    return MITDVP_OK;
  } catch (const mitdvp::NotConverged& ex) {
    *dst = ex.what();
    return MITDVP_ENOTCONV;
  } catch (const mitdvp::ArgError& ex) {
    *dst = ex.what();
    return MITDVP_EINVAL;
  } catch (const mitdvp::HipError& ex) {
    *dst = ex.what();
    return MITDVP_EHIP;
  } catch (const std::bad_alloc&) {
    *dst = "out of host memory";
    return MITDVP_ENOMEM;
  } catch (const std::exception& ex) {
    *dst = ex.what();
    return MITDVP_ESTATE;
  } catch (...) {  // nothing may leave an extern "C" entry point or a worker thread of mitdvp_ensemble_step
    *dst = "unknown exception";
    return MITDVP_ESTATE;
  }
}

mitdvp_config unit_cfg(int device) {
  mitdvp_config c{};
  c.nsite = 1;
  c.device = device;
  c.integrator = MITDVP_LANCZOS;
  c.conserve_norm = 1;
  c.thresh = 1e-9;
  c.max_krylov = 20;
  return c;
}

struct Dev {
  mitdvp::DevBuf b;
  Dev(hipStream_t st, const double* host, size_t elems) {
    b.reserve(std::max<size_t>(elems, 1));
    if (host && elems) HIP_CHECK(hipMemcpyAsync(b.p, host, elems * sizeof(mitdvp::zc), hipMemcpyHostToDevice, st));
  }
  explicit Dev(size_t elems) { b.reserve(std::max<size_t>(elems, 1)); }
  mitdvp::zc* p() { return b.p; }
};

void to_host(hipStream_t st, double* dst, const mitdvp::zc* src, size_t elems) {
  HIP_CHECK(hipMemcpyAsync(dst, src, elems * sizeof(mitdvp::zc), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
}
}  // namespace

extern "C" {

const char* mitdvp_version(void) { return "mitdvp 0.2 (gfx950)"; }

int mitdvp_device_count(int* count) {
  if (!count) { g_err = "null argument"; return MITDVP_EINVAL; }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;  // no driver / no GPU: 0 devices, not an error
  (void)hipGetLastError();
  *count = n;
  return MITDVP_OK;
}

int mitdvp_device_cu_count(int device, int* count) {
  return guard(nullptr, [&] {
    if (!count) throw mitdvp::ArgError("null pointer argument");
    HIP_CHECK(hipDeviceGetAttribute(count, hipDeviceAttributeMultiprocessorCount, device));
  });
}

int mitdvp_device_sync(int device) {
  return guard(nullptr, [&] {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int mitdvp_create(const mitdvp_config* cfg, mitdvp_engine** out) {
  if (!cfg || !out) { g_err = "null argument"; return MITDVP_EINVAL; }
  *out = nullptr;
  auto* h = new mitdvp_engine();
  h->device = cfg->device;
  int rc = guard(nullptr, [&] { h->e.reset(new mitdvp::Engine(*cfg)); });
  if (rc != MITDVP_OK) { delete h; return rc; }
  *out = h;
  return MITDVP_OK;
}
void mitdvp_destroy(mitdvp_engine* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  delete h;
}
const char* mitdvp_last_error(const mitdvp_engine* h) { return h ? h->err.c_str() : g_err.c_str(); }

#define ENG_CALL(h, body)                                   \
  if (!(h) || !(h)->e) { g_err = "null handle"; return MITDVP_EINVAL; } \
  return guard((h), [&] { body; (h)->e->check_device_errors(); })
// argument pointers that must not be NULL (reported as MITDVP_EINVAL instead of a crash)
#define NEED(...)                                                       \
  do {                                                                  \
    const void* ptrs_[] = {__VA_ARGS__};                                \
    for (const void* q_ : ptrs_)                                        \
      if (!q_) throw mitdvp::ArgError("null pointer argument");         \
  } while (0)

int mitdvp_set_site(mitdvp_engine* h, int isite, const double* reim, int l, int n, int r, int gauge) {
  ENG_CALL(h, { NEED(reim); h->e->set_site(isite, reim, l, n, r, gauge); });
}
int mitdvp_get_site_shape(mitdvp_engine* h, int isite, int* l, int* n, int* r, int* gauge) {
  ENG_CALL(h, { NEED(l, n, r, gauge); h->e->get_site_shape(isite, l, n, r, gauge); });
}
int mitdvp_get_site(mitdvp_engine* h, int isite, double* out) { ENG_CALL(h, { NEED(out); h->e->get_site(isite, out); }); }
int mitdvp_init_random(mitdvp_engine* h, const int* dims, int bond_dim, uint64_t seed) {
  ENG_CALL(h, { NEED(dims); h->e->init_random(dims, bond_dim, seed); });
}
int mitdvp_init_random_block(mitdvp_engine* h, const int* dims, int nsite_total, int first, int bond_dim, uint64_t seed, int balance) {
  ENG_CALL(h, { NEED(dims); h->e->init_random_block(dims, nsite_total, first, bond_dim, seed, balance != 0); });
}
int mitdvp_canonicalize(mitdvp_engine* h, double scale) { ENG_CALL(h, h->e->canonicalize(scale)); }
int mitdvp_set_mpo_core(mitdvp_engine* h, int op_id, int isite, const double* reim, int ml, int d_out, int d_in,
                        int mr) {
  ENG_CALL(h, { NEED(reim); h->e->set_mpo_core(op_id, isite, reim, ml, d_out, d_in, mr); });
}
int mitdvp_set_shift(mitdvp_engine* h, int op_id, double re, double im) { ENG_CALL(h, h->e->set_shift(op_id, re, im)); }
int mitdvp_step(mitdvp_engine* h, double dt) { ENG_CALL(h, h->e->step(dt)); }
int mitdvp_sweep(mitdvp_engine* h, double dt, int forward) { ENG_CALL(h, h->e->sweep(dt, forward != 0)); }
int mitdvp_sweep_part(mitdvp_engine* h, double dt, int forward, int nsites, int* left) {
  ENG_CALL(h, {
    const int r = h->e->sweep_part(dt, forward != 0, nsites);
    if (left) *left = r;
  });
}
int mitdvp_ensemble_step(mitdvp_engine** hs, int n, double dt, int nsteps, int* statuses) {
  if (!hs || n < 1 || nsteps < 0) { g_err = "mitdvp_ensemble_step: bad arguments"; return MITDVP_EINVAL; }
  for (int i = 0; i < n; ++i)
    if (!hs[i] || !hs[i]->e) { g_err = "mitdvp_ensemble_step: null engine"; return MITDVP_EINVAL; }
  for (int i = 0; i < n; ++i)  // a handle is driven by one host thread at a time
    for (int k = 0; k < i; ++k)
      if (hs[k] == hs[i]) { g_err = "mitdvp_ensemble_step: the same engine is listed twice"; return MITDVP_EINVAL; }
  std::vector<int> rc((size_t)n, MITDVP_OK);
  std::vector<std::thread> th;
  th.reserve((size_t)n);
  auto run = [&](int i) {
    mitdvp_engine* h = hs[i];
    rc[(size_t)i] = guard(h, [&] {
      for (int s = 0; s < nsteps; ++s) h->e->step(dt);
      h->e->check_device_errors();
      HIP_CHECK(hipStreamSynchronize(h->e->stream()));
    });
  };
  for (int i = 0; i < n; ++i) {
    try {
      th.emplace_back(run, i);
    } catch (const std::exception&) {  // no more host threads: this replica runs on the caller's thread, after the others
      for (auto& t : th) t.join();
      th.clear();
      for (int k = i; k < n; ++k) run(k);
      break;
    }
  }
  for (auto& t : th) t.join();
  int first = MITDVP_OK;
  for (int i = 0; i < n; ++i) {
    if (statuses) statuses[i] = rc[(size_t)i];
    if (first == MITDVP_OK && rc[(size_t)i] != MITDVP_OK) first = rc[(size_t)i];
  }
  return first;
}
// ---- batched trajectories (engine_batch.hip, batch_site.hip) ----
namespace {
int batch_finish(mitdvp_batch* b, const std::vector<int>& st, int* statuses) {
  int first = MITDVP_OK;
  for (size_t i = 0; i < st.size(); ++i) {
    int rc = MITDVP_OK;
    if (st[i] != mitdvp::SS_OK) {
      rc = st[i] == mitdvp::SS_ENOTCONV ? MITDVP_ENOTCONV : MITDVP_EINVAL;
      b->hs[i]->err = b->b->status_message(st[i]);
      if (first == MITDVP_OK) first = rc;
    }
    if (statuses) statuses[i] = rc;
  }
  return first;
}
}  // namespace
int mitdvp_batch_create(mitdvp_engine** hs, int n, mitdvp_batch** out) {
  if (!hs || !out || n < 1) { g_err = "mitdvp_batch_create: bad arguments"; return MITDVP_EINVAL; }
  *out = nullptr;
  for (int i = 0; i < n; ++i)
    if (!hs[i] || !hs[i]->e) { g_err = "mitdvp_batch_create: null engine"; return MITDVP_EINVAL; }
  auto* b = new mitdvp_batch();
  const int rc = guard(nullptr, [&] {
    std::vector<mitdvp::Engine*> es;
    for (int i = 0; i < n; ++i) { es.push_back(hs[i]->e.get()); b->hs.push_back(hs[i]); }
    b->b.reset(new mitdvp::Batch(es));
  });
  if (rc != MITDVP_OK) { delete b; return rc; }
  *out = b;
  return MITDVP_OK;
}
int mitdvp_batch_step(mitdvp_batch* b, double dt_au, int nsteps, int* statuses) {
  if (!b || !b->b) { g_err = "null handle"; return MITDVP_EINVAL; }
  std::vector<int> st((size_t)b->b->size(), 0);
  const int rc = guard(nullptr, [&] { b->b->step(dt_au, nsteps, st.data()); });
  if (rc != MITDVP_OK) return rc;
  return batch_finish(b, st, statuses);
}
int mitdvp_batch_sweep(mitdvp_batch* b, double dt_au, int forward, int* statuses) {
  if (!b || !b->b) { g_err = "null handle"; return MITDVP_EINVAL; }
  std::vector<int> st((size_t)b->b->size(), 0);
  const int rc = guard(nullptr, [&] { b->b->sweep(dt_au, forward != 0, st.data()); });
  if (rc != MITDVP_OK) return rc;
  return batch_finish(b, st, statuses);
}
int mitdvp_batch_run_keys(mitdvp_batch* b, double dt_au, int nsteps, int every, const int* sites, int nsites,
                          const int* remain_nleg, int nkeys, int what, const double* weights, const mitdvp_batch_out* out,
                          double* density, double* mean_density, size_t counts[4], int* statuses) {
  if (!b || !b->b) { g_err = "null handle"; return MITDVP_EINVAL; }
  std::vector<int> st((size_t)b->b->size(), 0);
  const int rc = guard(nullptr, [&] {
    if (nsteps < 0 || every < 1 || nsteps % every != 0)
      throw mitdvp::ArgError("batch: nsteps must be >= 0 and a multiple of every >= 1");
    if (nkeys < 0 || (nkeys > 0 && !remain_nleg)) throw mitdvp::ArgError("batch: bad list of density keys");
    HIP_CHECK(hipSetDevice(b->b->device()));
    const long nrdm = b->b->observe_sizes(sites, nsites, what, nkeys > 0 || b->b->has_cross() || b->b->has_spectra() || b->b->has_samples() ||
                                                                         b->b->has_expect() || b->b->has_cross_mpo());
    const long ndens = b->b->density_sizes(remain_nleg, nkeys, nrdm);
    if (counts) {
      counts[0] = (size_t)(nsteps / every + 1); counts[1] = (size_t)b->b->size(); counts[2] = (size_t)nrdm; counts[3] = (size_t)ndens;
    }
    if (!out && !density && !mean_density) return;  // size query
    mitdvp::Batch::ObsOut o;
    if (out) {
      o.norm = out->norm; o.autocorr = out->autocorr; o.energy = out->energy; o.rdm = out->rdm;
      o.mean_norm2 = out->mean_norm2; o.mean_autocorr = out->mean_autocorr; o.mean_energy = out->mean_energy; o.mean_rdm = out->mean_rdm;
    }
    mitdvp::Batch::DensOut dn;
    dn.legs = remain_nleg; dn.nkeys = nkeys; dn.density = density; dn.mean_density = mean_density;
    b->b->run(dt_au, nsteps, every, sites, nsites, what, weights, o, st.data(), dn);
  });
  if (rc != MITDVP_OK) return rc;
  return batch_finish(b, st, statuses);
}
int mitdvp_batch_observe_keys(mitdvp_batch* b, const int* sites, int nsites, const int* remain_nleg, int nkeys, int what,
                              const double* weights, const mitdvp_batch_out* out, double* density, double* mean_density,
                              size_t counts[4]) {
  return mitdvp_batch_run_keys(b, 0.0, 0, 1, sites, nsites, remain_nleg, nkeys, what, weights, out, density, mean_density, counts, nullptr);
}
// the nkeys = 0 case of mitdvp_batch_run_keys
int mitdvp_batch_run(mitdvp_batch* b, double dt_au, int nsteps, int every, const int* sites, int nsites, int what,
                     const double* weights, const mitdvp_batch_out* out, size_t counts[3], int* statuses) {
  size_t c4[4] = {0, 0, 0, 0};
  const int rc = mitdvp_batch_run_keys(b, dt_au, nsteps, every, sites, nsites, nullptr, 0, what, weights, out, nullptr, nullptr, c4, statuses);
  if (counts && (rc == MITDVP_OK || c4[1] != 0)) { counts[0] = c4[0]; counts[1] = c4[1]; counts[2] = c4[2]; }
  return rc;
}
int mitdvp_batch_observe(mitdvp_batch* b, const int* sites, int nsites, int what, const double* weights,
                         const mitdvp_batch_out* out, size_t counts[3]) {
  return mitdvp_batch_run(b, 0.0, 0, 1, sites, nsites, what, weights, out, counts, nullptr);
}
int mitdvp_batch_set_channel(mitdvp_batch* b, int site, int kind, const double* ops_reim, int nops, int d) {
  if (!b || !b->b) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_channel(site, kind, ops_reim, nops, d); });
}
int mitdvp_batch_set_seed(mitdvp_batch* b, unsigned long long seed, const unsigned long long* trajectory_ids) {
  if (!b || !b->b) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_seed(seed, trajectory_ids); });
}
int mitdvp_batch_jump_counts(mitdvp_batch* b, long long* counts) {
  if (!b || !b->b) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->jump_counts(counts); });
}
int mitdvp_batch_set_pair_channel(mitdvp_batch* b, int site, int kind, const double* ops_reim, int nops, int d0, int d1) {
  if (!b || !b->b) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_pair_channel(site, kind, ops_reim, nops, d0, d1); });
}
int mitdvp_batch_pair_jump_counts(mitdvp_batch* b, long long* counts) {
  if (!b || !b->b) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->pair_jump_counts(counts); });
}
int mitdvp_batch_discarded_weight(mitdvp_batch* b, double* weights) {
  if (!b || !b->b) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->discarded_weight(weights); });
}
int mitdvp_batch_set_field(mitdvp_batch* b, int site, int d, const double* vecs_reim, const double* evals, int kind,
                           const double* table, int ntab, int per_replica, double sigma, double tau) {
  if (!b || !b->b) { g_err = "mitdvp_batch_set_field: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_field(site, d, vecs_reim, evals, kind, table, ntab, per_replica, sigma, tau); });
}
int mitdvp_batch_field_values(mitdvp_batch* b, double* values) {
  if (!b || !b->b) { g_err = "mitdvp_batch_field_values: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->field_values(values); });
}
int mitdvp_batch_snapshot(mitdvp_batch* b) {
  if (!b || !b->b) { g_err = "mitdvp_batch_snapshot: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->snapshot(); });
}
int mitdvp_batch_set_cross(mitdvp_batch* b, int npairs, const int* bra, const int* ket, const int* site, const double* ops_reim,
                           const int* op_dims) {
  if (!b || !b->b) { g_err = "mitdvp_batch_set_cross: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_cross(npairs, bra, ket, site, ops_reim, op_dims); });
}
int mitdvp_batch_cross(mitdvp_batch* b, const double* weights, double* values, double* mean) {
  if (!b || !b->b) { g_err = "mitdvp_batch_cross: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->cross(weights, values, mean); });
}
int mitdvp_batch_cross_records(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[2]) {
  if (!b || !b->b) { g_err = "mitdvp_batch_cross_records: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->cross_records(weights, values, mean, counts); });
}
int mitdvp_batch_set_spectra(mitdvp_batch* b, const int* bonds, int nbonds) {
  if (!b || !b->b) { g_err = "mitdvp_batch_set_spectra: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_spectra(bonds, nbonds); });
}
int mitdvp_batch_spectra(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[2]) {
  if (!b || !b->b) { g_err = "mitdvp_batch_spectra: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->spectra(weights, values, mean, counts); });
}
int mitdvp_batch_spectra_records(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[3]) {
  if (!b || !b->b) { g_err = "mitdvp_batch_spectra_records: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->spectra_records(weights, values, mean, counts); });
}
int mitdvp_batch_set_samples(mitdvp_batch* b, int nshots, unsigned long long seed) {
  if (!b || !b->b) { g_err = "mitdvp_batch_set_samples: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_samples(nshots, seed); });
}
int mitdvp_batch_samples(mitdvp_batch* b, const double* weights, int* configs, double* prob, double* freq, double* mean_freq,
                         size_t counts[4]) {
  if (!b || !b->b) { g_err = "mitdvp_batch_samples: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->samples(weights, configs, prob, freq, mean_freq, counts); });
}
int mitdvp_batch_samples_records(mitdvp_batch* b, const double* weights, int* configs, double* prob, double* freq, double* mean_freq,
                                 size_t counts[5]) {
  if (!b || !b->b) { g_err = "mitdvp_batch_samples_records: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->samples_records(weights, configs, prob, freq, mean_freq, counts); });
}
int mitdvp_batch_set_expect(mitdvp_batch* b, const int* op_ids, int nops) {
  if (!b || !b->b) { g_err = "mitdvp_batch_set_expect: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_expect(op_ids, nops); });
}
int mitdvp_batch_expect(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[2]) {
  if (!b || !b->b) { g_err = "mitdvp_batch_expect: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->expect(weights, values, mean, counts); });
}
int mitdvp_batch_expect_records(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[3]) {
  if (!b || !b->b) { g_err = "mitdvp_batch_expect_records: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->expect_records(weights, values, mean, counts); });
}
int mitdvp_batch_set_cross_mpo(mitdvp_batch* b, int nentries, const int* bra, const int* ket, const int* op_id) {
  if (!b || !b->b) { g_err = "mitdvp_batch_set_cross_mpo: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_cross_mpo(nentries, bra, ket, op_id); });
}
int mitdvp_batch_cross_mpo(mitdvp_batch* b, const double* weights, double* values, double* mean) {
  if (!b || !b->b) { g_err = "mitdvp_batch_cross_mpo: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->cross_mpo(weights, values, mean); });
}
int mitdvp_batch_cross_mpo_records(mitdvp_batch* b, const double* weights, double* values, double* mean, size_t counts[2]) {
  if (!b || !b->b) { g_err = "mitdvp_batch_cross_mpo_records: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->cross_mpo_records(weights, values, mean, counts); });
}
int mitdvp_batch_operate(mitdvp_batch* b, int op_id, int maxstep, double conv_tol, const int* replicas, int nsel, double* norms,
                         int* iters, int* statuses) {
  if (!b || !b->b) { g_err = "mitdvp_batch_operate: null handle"; return MITDVP_EINVAL; }
  const size_t n = (size_t)b->b->size();
  std::vector<int> st(n, -1);  // -1: not selected, left as given
  const int rc = guard(nullptr, [&] { b->b->operate(op_id, maxstep, conv_tol, replicas, nsel, norms, iters, st.data()); });
  if (rc != MITDVP_OK) return rc;
  int first = MITDVP_OK;
  for (size_t i = 0; i < n; ++i) {
    if (st[i] < 0) continue;
    int code = MITDVP_OK;
    if (st[i] != mitdvp::SS_OK) {
      code = MITDVP_EINVAL;
      b->hs[i]->err = "mitdvp_batch_operate: the operator annihilates the state of replica " + std::to_string(i) +
                      " (an apply gave a norm that is not > 0)";
      if (first == MITDVP_OK) first = code;
    }
    if (statuses) statuses[i] = code;
  }
  return first;
}
int mitdvp_batch_relax(mitdvp_batch* b, int maxstep, double conv_tol, double* energies, int* steps, double* history, int* statuses) {
  if (!b || !b->b) { g_err = "mitdvp_batch_relax: null handle"; return MITDVP_EINVAL; }
  std::vector<int> st((size_t)b->b->size(), 0);
  const int rc = guard(nullptr, [&] { b->b->relax(maxstep, conv_tol, energies, steps, history, st.data()); });
  if (rc != MITDVP_OK) return rc;
  return batch_finish(b, st, statuses);
}
int mitdvp_batch_set_relax_restarts(mitdvp_batch* b, int max_restarts) {
  if (!b || !b->b) { g_err = "mitdvp_batch_set_relax_restarts: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->set_relax_restarts(max_restarts); });
}
int mitdvp_batch_relax_restarts(mitdvp_batch* b, long long* total, int* most) {
  if (!b || !b->b) { g_err = "mitdvp_batch_relax_restarts: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->relax_restarts(total, most); });
}
int mitdvp_batch_deflate_push(mitdvp_batch* b, const double* weights) {
  if (!b || !b->b) { g_err = "mitdvp_batch_deflate_push: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->deflate_push(weights); });
}
int mitdvp_batch_deflate_clear(mitdvp_batch* b) {
  if (!b || !b->b) { g_err = "mitdvp_batch_deflate_clear: null handle"; return MITDVP_EINVAL; }
  b->b->deflate_clear();
  return MITDVP_OK;
}
int mitdvp_batch_deflate_count(mitdvp_batch* b, int* count) {
  if (!b || !b->b) { g_err = "mitdvp_batch_deflate_count: null handle"; return MITDVP_EINVAL; }
  if (!count) { g_err = "mitdvp_batch_deflate_count: count is NULL"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { *count = b->b->deflate_count(); });
}
int mitdvp_batch_deflate_overlaps(mitdvp_batch* b, double* reim) {
  if (!b || !b->b) { g_err = "mitdvp_batch_deflate_overlaps: null handle"; return MITDVP_EINVAL; }
  return guard(nullptr, [&] { b->b->deflate_overlaps(reim); });
}
int mitdvp_batch_trilow(int device, const double* alpha, const double* beta, const int* k, int ncases, double* theta, double* vec) {
  return guard(nullptr, [&] { mitdvp::batch_trilow(device, alpha, beta, k, ncases, theta, vec); });
}
void mitdvp_batch_destroy(mitdvp_batch* b) { delete b; }
int mitdvp_invalidate_env(mitdvp_engine* h) { ENG_CALL(h, h->e->invalidate_env()); }
int mitdvp_replace_site(mitdvp_engine* h, int isite, const double* reim, int gauge) {
  ENG_CALL(h, { NEED(reim); h->e->replace_site(isite, reim, gauge); });
}
int mitdvp_set_boundary_env(mitdvp_engine* h, int side, const double* reim, int d, int m) {
  ENG_CALL(h, { NEED(reim); h->e->set_boundary_env(side, reim, d, m); });
}
int mitdvp_get_env(mitdvp_engine* h, int side, int bond, double* reim_out, int* d, int* m) {
  ENG_CALL(h, { NEED(d, m); h->e->env_shape(side, bond, d, m); if (reim_out) h->e->get_env(side, bond, reim_out); });
}
int mitdvp_build_envs(mitdvp_engine* h, int side) { ENG_CALL(h, h->e->build_envs(side)); }
int mitdvp_site_exp(mitdvp_engine* h, double dt) { ENG_CALL(h, h->e->site_exp(dt)); }
int mitdvp_split_center(mitdvp_engine* h, int forward) { ENG_CALL(h, h->e->split_center(forward != 0)); }
int mitdvp_bond_exp(mitdvp_engine* h, double dt) { ENG_CALL(h, h->e->bond_exp(dt)); }
int mitdvp_absorb_bond(mitdvp_engine* h, int forward) { ENG_CALL(h, h->e->absorb_bond(forward != 0)); }
int mitdvp_get_bond(mitdvp_engine* h, double* reim_out, int* dim) { ENG_CALL(h, { NEED(dim); h->e->get_bond(reim_out, dim); }); }
int mitdvp_set_bond(mitdvp_engine* h, int bond, const double* reim, int dim) {
  ENG_CALL(h, { NEED(reim); h->e->set_bond(bond, reim, dim); });
}
int mitdvp_fold_block_range(mitdvp_engine* h, int op_id, int conj_bra, int from_left, int first, int count, const double* reim_in,
                            int d, int m, double* reim_out) {
  ENG_CALL(h, { NEED(reim_in, reim_out); h->e->fold_block(op_id, conj_bra != 0, from_left != 0, reim_in, d, m, reim_out, first, count); });
}
int mitdvp_site_rdm_blocks(mitdvp_engine* h, int isite, const double* left, const double* right, double* reim_out) {
  ENG_CALL(h, { NEED(left, right, reim_out); h->e->site_rdm_blocks(isite, left, right, reim_out); });
}
int mitdvp_set_qr_fast(int on) { mitdvp::qr_set_fast(on); return MITDVP_OK; }
int mitdvp_get_qr_fast(void) { return mitdvp::qr_get_fast(); }
int mitdvp_heff_apply_center(mitdvp_engine* h, const double* reim_in, double* reim_out, int* flags) {
  ENG_CALL(h, { NEED(reim_out); h->e->heff_apply_center(reim_in, reim_out, flags); });
}
int mitdvp_get_krylov_memory(mitdvp_engine* h, int isite, int* k) { ENG_CALL(h, { NEED(k); *k = h->e->kprev_get(isite); }); }
int mitdvp_set_krylov_memory(mitdvp_engine* h, int isite, int k) { ENG_CALL(h, h->e->kprev_set(isite, k)); }
int mitdvp_set_small_kernels(mitdvp_engine* h, int on) { ENG_CALL(h, h->e->set_small_kernels(on != 0)); }
int mitdvp_set_pointer_mode(mitdvp_engine* h, int mode) { ENG_CALL(h, h->e->set_pointer_mode(mode)); }
int mitdvp_fold_block(mitdvp_engine* h, int op_id, int conj_bra, int from_left, const double* reim_in, int d, int m,
                      double* reim_out) {
  ENG_CALL(h, { NEED(reim_in, reim_out); h->e->fold_block(op_id, conj_bra != 0, from_left != 0, reim_in, d, m, reim_out); });
}
int mitdvp_expect(mitdvp_engine* h, int op_id, double out[2]) {
  ENG_CALL(h, { NEED(out); auto v = h->e->expect(op_id); out[0] = v.real(); out[1] = v.imag(); });
}
int mitdvp_autocorr(mitdvp_engine* h, double out[2]) {
  ENG_CALL(h, { NEED(out); auto v = h->e->autocorr(); out[0] = v.real(); out[1] = v.imag(); });
}
int mitdvp_norm(mitdvp_engine* h, double* out) { ENG_CALL(h, { NEED(out); *out = h->e->norm(); }); }
int mitdvp_site_rdm(mitdvp_engine* h, int isite, double* out) { ENG_CALL(h, { NEED(out); h->e->site_rdm(isite, out); }); }
int mitdvp_reduced_density(mitdvp_engine* h, const int* remain_nleg, int nlen, double* out, size_t* n_out) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] {
    if (!n_out || !remain_nleg) throw mitdvp::ArgError("null argument");
    if (!out) {  // size query: product of the kept physical dimensions
      size_t n = 1;
      for (int p = 0; p < nlen; ++p) {
        int l = 0, d = 0, r = 0, g = 0;
        h->e->get_site_shape(p, &l, &d, &r, &g);
        for (int q = 0; q < remain_nleg[p]; ++q) n *= (size_t)d;
      }
      *n_out = n;
      return;
    }
    std::vector<mitdvp::hzc> v;
    std::vector<int> shp;
    h->e->reduced_density(remain_nleg, nlen, v, shp);
    if (v.size() > *n_out) throw mitdvp::ArgError("output buffer too small");
    std::memcpy(out, v.data(), v.size() * sizeof(mitdvp::hzc));
    *n_out = v.size();
  });
}
int mitdvp_truncate_bond(mitdvp_engine* h, double p, int max_dim, int* new_dim, double* svals_out) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] {
    std::vector<double> sv;
    const int n = h->e->truncate_bond(p, max_dim, sv);
    if (new_dim) *new_dim = n;
    if (svals_out) std::memcpy(svals_out, sv.data(), sv.size() * sizeof(double));
  });
}
int mitdvp_set_gate(mitdvp_engine* h, int isite, const double* U_reim, int d) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] { h->e->set_gate(isite, U_reim, d); });
}
int mitdvp_apply_gates(mitdvp_engine* h) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] { h->e->apply_gates(); });
}
int mitdvp_set_kraus(mitdvp_engine* h, int isite, int two_site, const double* B_reim, int k, int d) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] { h->e->set_kraus(isite, two_site, B_reim, k, d); });
}
int mitdvp_apply_kraus(mitdvp_engine* h) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] { h->e->apply_kraus(); });
}
int mitdvp_rccl_unique_id(char out[128]) {
  return guard(nullptr, [&] { NEED(out); mitdvp::Engine::rccl_unique_id(out); });
}
int mitdvp_set_parallel_rccl(mitdvp_engine* h, int nranks, int rank, const char id[128]) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] { NEED(id); h->e->set_parallel_rccl(nranks, rank, id); });
}
int mitdvp_rccl_selftest(mitdvp_engine* h, int* mismatches) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] { NEED(mismatches); *mismatches = h->e->rccl_selftest(); });
}
int mitdvp_save_reference(mitdvp_engine* h) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] { h->e->save_reference(); });
}
int mitdvp_overlap_reference(mitdvp_engine* h, double out[2]) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] {
    NEED(out);
    const mitdvp::hzc v = h->e->overlap_reference();
    out[0] = v.real(); out[1] = v.imag();
  });
}
int mitdvp_operate(mitdvp_engine* h, int op_id, int maxstep, double conv_tol, double* norm_out, int* iters_out) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] {
    const double n = h->e->operate(op_id, maxstep, conv_tol, iters_out);
    if (norm_out) *norm_out = n;
  });
}
// ---- several electronic states (engine_multi.hip) ---------------------------------------------
int mitdvp_ms_configure(mitdvp_engine* h, int nstate) { ENG_CALL(h, { h->e->ms_configure(nstate); }); }
int mitdvp_ms_set_site(mitdvp_engine* h, int istate, int isite, const double* reim, int l, int n, int r, int gauge) {
  ENG_CALL(h, { NEED(reim); h->e->ms_set_site(istate, isite, reim, l, n, r, gauge); });
}
int mitdvp_ms_get_site_shape(mitdvp_engine* h, int istate, int isite, int* l, int* n, int* r, int* gauge) {
  ENG_CALL(h, { NEED(l, n, r, gauge); h->e->ms_get_site_shape(istate, isite, l, n, r, gauge); });
}
int mitdvp_ms_get_site(mitdvp_engine* h, int istate, int isite, double* out) {
  ENG_CALL(h, { NEED(out); h->e->ms_get_site(istate, isite, out); });
}
int mitdvp_ms_canonicalize(mitdvp_engine* h, int istate, double scale) { ENG_CALL(h, { h->e->ms_canonicalize(istate, scale); }); }
int mitdvp_ms_set_mpo_core(mitdvp_engine* h, int op_id, int ibra, int iket, int isite, const double* reim, int ml, int d_out,
                           int d_in, int mr) {
  ENG_CALL(h, { NEED(reim); h->e->ms_set_mpo_core(op_id, ibra, iket, isite, reim, ml, d_out, d_in, mr); });
}
int mitdvp_ms_set_coupleJ(mitdvp_engine* h, int op_id, int ibra, int iket, double re, double im) {
  ENG_CALL(h, { h->e->ms_set_couplej(op_id, ibra, iket, re, im); });
}
int mitdvp_ms_step(mitdvp_engine* h, double dt_au) { ENG_CALL(h, { h->e->ms_step(dt_au); }); }
int mitdvp_ms_expect(mitdvp_engine* h, int op_id, double out[2]) {
  ENG_CALL(h, { NEED(out); auto v = h->e->ms_expect(op_id); out[0] = v.real(); out[1] = v.imag(); });
}
int mitdvp_ms_autocorr(mitdvp_engine* h, double out[2]) {
  ENG_CALL(h, { NEED(out); auto v = h->e->ms_autocorr(); out[0] = v.real(); out[1] = v.imag(); });
}
int mitdvp_ms_operate(mitdvp_engine* h, int op_id, int maxstep, double conv_tol, double* norm_out, int* iters_out) {
  ENG_CALL(h, {
    const double n = h->e->ms_operate(op_id, maxstep, conv_tol, iters_out);
    if (norm_out) *norm_out = n;
  });
}
int mitdvp_ms_pops(mitdvp_engine* h, double* out) { ENG_CALL(h, { NEED(out); h->e->ms_pops(out); }); }

int mitdvp_set_adaptive(mitdvp_engine* h, int enable, int dmax, int dd, double p_proj) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] { h->e->set_adaptive(enable != 0, dmax, dd, p_proj); });
}
int mitdvp_thin_to_full(int device, int gauge, const double* site, int l, int c, int r, int extra, double* out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    if (l < 1 || c < 1 || r < 1 || extra < 0) throw ArgError("thin_to_full: bad shape");
    const long room = gauge == 0 ? (long)l * c - r : (long)c * r - l;
    if (room < 0) throw ArgError("thin_to_full: the tensor cannot be an isometry in that gauge");
    if (extra > room) throw ArgError("thin_to_full: extra exceeds the dimension of the orthogonal complement");
    Engine e(unit_cfg(device));
    hipStream_t st = e.stream();
    const long ns = (long)l * c * r;
    const long nf = gauge == 0 ? (long)l * c * (r + extra) : (long)(l + extra) * c * r;
    e.ensure_work(nf, 1, 1, gauge == 0 ? l * c : c * r, gauge == 0 ? r : l, extra + 1);
    Dev din(st, site, ns), dout(nf);
    if (gauge == 0) e.thin_to_full_A(din.p(), l, c, r, extra, dout.p());
    else e.thin_to_full_B(din.p(), l, c, r, extra, dout.p());
    to_host(st, out, dout.p(), nf);
  });
}
int mitdvp_svd(int device, const double* A, int r, int c, double* U, double* S, double* Vh, int* sweeps) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    HIP_CHECK(hipSetDevice(device));
    hipStream_t st;
    HIP_CHECK(hipStreamCreate(&st));
    {
      const int k = std::min(r, c);
      Dev dA(st, A, (size_t)r * c), dU((size_t)r * k), dV((size_t)k * c), work(svd_work_elems(r, c));
      svd_jacobi(st, dA.p(), r, c, dU.p(), S, dV.p(), work.p(), sweeps);
      to_host(st, U, dU.p(), (size_t)r * k);
      to_host(st, Vh, dV.p(), (size_t)k * c);
    }
    HIP_CHECK(hipStreamDestroy(st));
  });
}
int mitdvp_set_trace_op_core(mitdvp_engine* h, int op_id, int isite, const double* reim, int ml, int n, int mr) {
  ENG_CALL(h, { NEED(reim); h->e->set_trace_op_core(op_id, isite, reim, ml, n, mr); });
}
int mitdvp_expect_trace(mitdvp_engine* h, int op_id, double out[2]) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] {
    NEED(out);
    const auto v = h->e->expect_trace(op_id);
    out[0] = v.real();
    out[1] = v.imag();
  });
}
int mitdvp_partial_trace(mitdvp_engine* h, const int* remain_nleg, int nlen, double* out, size_t* n_out) {
  if (!h || !h->e) { g_err = "null handle"; return MITDVP_EINVAL; }
  return guard(h, [&] {
    if (!n_out || !remain_nleg) throw mitdvp::ArgError("null argument");
    if (!out) {
      int center = -1;
      for (int p = 0; p < nlen; ++p)
        if (remain_nleg[p]) center = p;
      size_t n = 1;
      for (int p = 0; p <= center; ++p) {
        int l = 0, d = 0, r = 0, g = 0;
        h->e->get_site_shape(p, &l, &d, &r, &g);
        (void)d;
        const size_t nn = (size_t)h->e->liouville_n(p);
        const int k = p == center ? 2 : remain_nleg[p];
        for (int q = 0; q < k; ++q) n *= nn;
      }
      *n_out = n;
      return;
    }
    std::vector<mitdvp::hzc> v;
    h->e->partial_trace(remain_nleg, nlen, v);
    if (v.size() > *n_out) throw mitdvp::ArgError("output buffer too small");
    std::memcpy(out, v.data(), v.size() * sizeof(mitdvp::hzc));
    *n_out = v.size();
  });
}
int mitdvp_set_subspace(mitdvp_engine* h, int isite, int n, const int* inds, int ninds) {
  ENG_CALL(h, h->e->set_subspace(isite, n, inds, ninds));
}
int mitdvp_hermitise(mitdvp_engine* h) { ENG_CALL(h, h->e->hermitise()); }
int mitdvp_krylov_stats(mitdvp_engine* h, int* per_site) { ENG_CALL(h, { NEED(per_site); h->e->krylov_stats(per_site); }); }
int mitdvp_counters_get(mitdvp_engine* h, mitdvp_counters* out) { ENG_CALL(h, { NEED(out); h->e->counters_get(out); }); }
int mitdvp_counters_reset(mitdvp_engine* h) { ENG_CALL(h, h->e->counters_reset()); }
int mitdvp_set_profiling(mitdvp_engine* h, int on) { ENG_CALL(h, h->e->set_profiling(on != 0)); }
int mitdvp_set_parallel(mitdvp_engine* h, int nranks, int rank, mitdvp_collective_fn fn, void* user) {
  ENG_CALL(h, h->e->set_parallel(nranks, rank, fn, user));
}

// ---- unit-level seam ------------------------------------------------------
int mitdvp_heff_apply(int device, const double* L, const double* W, const double* R, const double* psi, int dl,
                      int d, int dr, int ml, int mr, double* sigma_out, int reps, double* ms_out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    Engine e(unit_cfg(device));
    hipStream_t st = e.stream();
    e.set_mpo_core(0, 0, W, ml, d, d, mr);
    const long ns = (long)dl * d * dr, mm = std::max(ml, mr);
    e.ensure_work(ns, (long)dl * dr * d * mm, (long)dl * dr * d * mm, 1, 1);
    Dev dL(st, L, (size_t)dl * ml * dl), dR(st, R, (size_t)dr * mr * dr), dpsi(st, psi, ns), dout(ns);
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    const MpoSite& w = e.mpo(0, 0);
    e.heff_apply(dL.p(), w, dR.p(), dpsi.p(), dout.p(), dl, d, dr, hzc(0, 0));
    HIP_CHECK(hipEventRecord(a, st));
    for (int i = 0; i < reps; ++i) e.heff_apply(dL.p(), w, dR.p(), dpsi.p(), dout.p(), dl, d, dr, hzc(0, 0));
    HIP_CHECK(hipEventRecord(b, st));
    HIP_CHECK(hipEventSynchronize(b));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    if (ms_out) *ms_out = reps > 0 ? ms / reps : 0.0;
    HIP_CHECK(hipEventDestroy(a));
    HIP_CHECK(hipEventDestroy(b));
    to_host(st, sigma_out, dout.p(), ns);
  });
}

int mitdvp_keff_apply(int device, const double* L, const double* R, const double* sval, int dl, int dr, int m,
                      double* out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    Engine e(unit_cfg(device));
    hipStream_t st = e.stream();
    e.ensure_work((long)dl * dr, (long)dl * m * dr, 1, 1, 1);
    Dev dL(st, L, (size_t)dl * m * dl), dR(st, R, (size_t)dr * m * dr), ds(st, sval, (size_t)dl * dr),
        dout((size_t)dl * dr);
    e.keff_apply(dL.p(), dR.p(), ds.p(), dout.p(), dl, dr, m, hzc(0, 0));
    to_host(st, out, dout.p(), (size_t)dl * dr);
  });
}

int mitdvp_env_update(int device, int left, const double* env, const double* site, const double* W, int dl, int d,
                      int dr, int ml, int mr, double* out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    Engine e(unit_cfg(device));
    hipStream_t st = e.stream();
    e.set_mpo_core(0, 0, W, ml, d, d, mr);
    const long ns = (long)dl * d * dr, mm = std::max(ml, mr);
    e.ensure_work(ns, (long)dl * dr * d * mm, (long)dl * dr * d * mm, 1, 1);
    const MpoSite& w = e.mpo(0, 0);
    Dev dsite(st, site, ns);
    if (left) {
      // contract_with_site_mpo, gauge "A": env (dl, ml, dl) -> (dr, mr, dr)
      Dev denv(st, env, (size_t)dl * ml * dl), dout((size_t)dr * mr * dr);
      e.env_update(denv.p(), dsite.p(), w.w2l.p, dout.p(), dl, ml, d, dr, mr);
      to_host(st, out, dout.p(), (size_t)dr * mr * dr);
    } else {
      // gauge "B": env (dr, mr, dr) -> (dl, ml, dl), through the mirrored tensor
      Dev denv(st, env, (size_t)dr * mr * dr), dout((size_t)dl * ml * dl), dbt(ns);
      transpose_rev3(st, dsite.p(), dbt.p(), dl, d, dr);
      e.env_update(denv.p(), dbt.p(), w.w2r.p, dout.p(), dr, mr, d, dl, ml);
      to_host(st, out, dout.p(), (size_t)dl * ml * dl);
    }
  });
}

// ---- the one-launch small-bond kernel under a chosen launch plan ------------
namespace {
// the unplanned chain of a kind (operands null: only "is there a W stage" matters to the plan)
void small_chain_of(mitdvp::SmallChain& c, int kind, const int* q) {
  using namespace mitdvp;
  static const zc w_stage{};  // any non-null address: the plan reads W2 as a flag
  if (!q) throw ArgError("null argument");
  const int n = kind == MITDVP_SMALL_KEFF ? 3 : 5;
  for (int k = 0; k < n; ++k)
    if (q[k] < 1) throw ArgError("small chain: every extent must be at least 1");
  if (kind == MITDVP_SMALL_HEFF) small_chain_heff(c, nullptr, &w_stage, nullptr, q[0], q[1], q[2], q[3], q[4]);
  else if (kind == MITDVP_SMALL_KEFF) small_chain_keff(c, nullptr, nullptr, q[0], q[1], q[2]);
  else if (kind == MITDVP_SMALL_ENV) small_chain_env(c, nullptr, &w_stage, q[0], q[1], q[2], q[3], q[4]);
  else throw ArgError("small chain: kind is MITDVP_SMALL_HEFF, _KEFF or _ENV");
}
}  // namespace

int mitdvp_small_plan(int kind, const int* dims, int exp_mode, int n_cu, mitdvp_small_plan_t* out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    NEED(out);
    if (n_cu < 1) throw ArgError("mitdvp_small_plan: n_cu must be at least 1");
    *out = mitdvp_small_plan_t{};
    SmallChain c;
    small_chain_of(c, kind, dims);
    if (!small_chain_plan(c, exp_mode != 0, n_cu)) return;
    const Carve cv = ss_carve(c, exp_mode != 0);
    out->ok = 1;
    out->nsc = c.nsc; out->cs = c.cs; out->spw = c.spw; out->a_resident = c.a_resident;
    out->grid = ((c.na + c.spw - 1) / c.spw) * c.nsc;
    out->lds_bytes = (int)small_chain_lds(c, exp_mode != 0);
    out->sg_aliases_x = cv.Sg == cv.Xs ? 1 : 0;
  });
}

int mitdvp_small_apply(int device, int cu_count, int kind, int left, const int* dims, const double* a, const double* w,
                       const double* r, const double* v, double shift_re, double shift_im, double* out,
                       mitdvp_small_info* info) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    NEED(dims); NEED(a); NEED(v); NEED(out); NEED(info);
    *info = mitdvp_small_info{};
    const hzc shift(shift_re, shift_im);
    mitdvp_config cfg = unit_cfg(device);
    cfg.cu_first = 0;
    cfg.cu_count = cu_count;  // Engine: a multiple of 8 inside the device
    Engine e(cfg);
    hipStream_t st = e.stream();
    mitdvp_counters c0{}, c1{};
    if (kind == MITDVP_SMALL_KEFF) {
      NEED(r);
      const int d1 = dims[0], d2 = dims[1], m = dims[2];
      if (d1 < 1 || d2 < 1 || m < 1) throw ArgError("mitdvp_small_apply: every extent must be at least 1");
      e.ensure_work((long)d1 * d2, (long)d1 * m * d2, 1, 1, 1);
      Dev dL(st, a, (size_t)d1 * m * d1), dR(st, r, (size_t)d2 * m * d2), ds(st, v, (size_t)d1 * d2), dout((size_t)d1 * d2);
      e.counters_get(&c0);
      e.keff_apply(dL.p(), dR.p(), ds.p(), dout.p(), d1, d2, m, shift);
      e.counters_get(&c1);
      to_host(st, out, dout.p(), (size_t)d1 * d2);
    } else if (kind == MITDVP_SMALL_HEFF || kind == MITDVP_SMALL_ENV) {
      NEED(w);
      const int dl = dims[0], d = dims[1], dr = dims[2], ml = dims[3], mr = dims[4];
      if (dl < 1 || d < 1 || dr < 1 || ml < 1 || mr < 1) throw ArgError("mitdvp_small_apply: every extent must be at least 1");
      e.set_mpo_core(0, 0, w, ml, d, d, mr);
      const long ns = (long)dl * d * dr, mm = std::max(ml, mr);
      e.ensure_work(ns, (long)dl * dr * d * mm, (long)dl * dr * d * mm, 1, 1);
      const MpoSite& ws = e.mpo(0, 0);
      Dev dv(st, v, ns);
      if (kind == MITDVP_SMALL_HEFF) {
        NEED(r);
        Dev dL(st, a, (size_t)dl * ml * dl), dR(st, r, (size_t)dr * mr * dr), dout(ns);
        e.counters_get(&c0);
        e.heff_apply(dL.p(), ws, dR.p(), dv.p(), dout.p(), dl, d, dr, shift);
        e.counters_get(&c1);
        to_host(st, out, dout.p(), ns);
      } else {
        if (shift != hzc(0.0, 0.0)) throw ArgError("mitdvp_small_apply: an environment update takes no shift");
        if (left) {  // as Engine's -> sweep issues it: the small-site core w2el beside the general one
          Dev denv(st, a, (size_t)dl * ml * dl), dout((size_t)dr * mr * dr);
          e.counters_get(&c0);
          e.env_update(denv.p(), dv.p(), ws.w2l.p, dout.p(), dl, ml, d, dr, mr, ws.w2el.p);
          e.counters_get(&c1);
          to_host(st, out, dout.p(), (size_t)dr * mr * dr);
        } else {  // <- sweep: the mirrored tensor and w2r / w2er
          Dev denv(st, a, (size_t)dr * mr * dr), dout((size_t)dl * ml * dl), dbt(ns);
          transpose_rev3(st, dv.p(), dbt.p(), dl, d, dr);
          e.counters_get(&c0);
          e.env_update(denv.p(), dbt.p(), ws.w2r.p, dout.p(), dr, mr, d, dl, ml, ws.w2er.p);
          e.counters_get(&c1);
          to_host(st, out, dout.p(), (size_t)dl * ml * dl);
        }
      }
    } else {
      throw ArgError("mitdvp_small_apply: kind is MITDVP_SMALL_HEFF, _KEFF or _ENV");
    }
    e.check_device_errors();  // a launch that gave up (an exchange timed out) is an error of this call
    info->n_launch = (int)(c1.n_launch - c0.n_launch);
    const SmallSync::Last& p = e.small_last();
    if (info->n_launch == 1 && p.mode == SS_MODE_APPLY) {
      info->plan.ok = 1;
      info->plan.nsc = p.nsc; info->plan.cs = p.cs; info->plan.spw = p.spw; info->plan.a_resident = p.a_resident;
      info->plan.grid = p.grid; info->plan.lds_bytes = (int)p.lds; info->plan.sg_aliases_x = p.sg_aliases_x;
    }
  });
}

int mitdvp_gauge_trf(int device, int key, const double* psi, int dl, int d, int dr, double* site_out,
                     double* sigma_out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    Engine e(unit_cfg(device));
    hipStream_t st = e.stream();
    const long ns = (long)dl * d * dr;
    e.ensure_work(ns, 1, 1, std::max(dl, dr) * d, std::max(dl, dr));
    e.set_qr_gauge_free(false);  // SiteCoef.gauge_trf as LAPACK returns it (signs of diag(R) included)
    Dev dpsi(st, psi, ns), dsite(ns), dbt(ns);
    if (key == 0) {
      Dev dsig((size_t)dr * dr);
      e.gauge_qr_left(dpsi.p(), dl, d, dr, dsite.p(), dsig.p());
      to_host(st, site_out, dsite.p(), ns);
      to_host(st, sigma_out, dsig.p(), (size_t)dr * dr);
    } else {
      Dev dsig((size_t)dl * dl);
      e.gauge_qr_right(dpsi.p(), dl, d, dr, dsite.p(), dbt.p(), dsig.p());
      to_host(st, site_out, dsite.p(), ns);
      to_host(st, sigma_out, dsig.p(), (size_t)dl * dl);
    }
  });
}

int mitdvp_expm_dense_counted(int device, int integrator, int conserve_norm, int lanczos_variant, const double* mat, int n,
                              const double* x, double scale_re, double scale_im, double thresh, int k_prev, double* y_out,
                              int* k_out, mitdvp_counters* counters_out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    mitdvp_config c = unit_cfg(device);
    c.integrator = integrator;
    c.conserve_norm = conserve_norm;
    c.lanczos_variant = lanczos_variant;
    c.thresh = thresh;
    Engine e(c);
    hipStream_t st = e.stream();
    e.ensure_work(n, 1, 1, 1, 1);
    Dev dm(st, mat, (size_t)n * n), dx(st, x, n);
    auto mv = [&](const zc* in, zc* out) {  // not counted: n_launch holds the launches of the Krylov loop alone
      ZgemmDesc g = zgemm_desc(dm.p(), in, out, n, 1, n);
      zgemm(st, g);
    };
    const int k = e.krylov_exp(hzc(scale_re, scale_im), mv, dx.p(), n, k_prev);
    if (k_out) *k_out = k;
    if (counters_out) e.counters_get(counters_out);
    to_host(st, y_out, dx.p(), n);
  });
}

int mitdvp_expm_dense(int device, int integrator, int conserve_norm, int lanczos_variant, const double* mat, int n,
                      const double* x, double scale_re, double scale_im, double thresh, int k_prev, double* y_out,
                      int* k_out) {
  return mitdvp_expm_dense_counted(device, integrator, conserve_norm, lanczos_variant, mat, n, x, scale_re, scale_im, thresh,
                                   k_prev, y_out, k_out, nullptr);
}

// ---- kernel-level hooks ---------------------------------------------------
int mitdvp_zgemm(int device, int transA, int conjA, int transB, int conjB, int m, int n, int k, const double* A,
                 const double* B, double* C, const double alpha[2], const double beta[2], int tile_cfg, int reps,
                 double* ms_out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    HIP_CHECK(hipSetDevice(device));
    hipStream_t st;
    HIP_CHECK(hipStreamCreate(&st));
    {
      Dev dA(st, A, (size_t)m * k), dB(st, B, (size_t)k * n), dC(st, C, (size_t)m * n), dC0(st, C, (size_t)m * n);
      ZgemmDesc g = zgemm_desc(dA.p(), dB.p(), dC.p(), m, n, k);
      g.transA = transA; g.conjA = conjA; g.transB = transB; g.conjB = conjB;
      g.lda = transA ? m : k;
      g.ldb = transB ? k : n;
      g.alpha = make_double2(alpha[0], alpha[1]);
      g.beta = make_double2(beta[0], beta[1]);
      g.tile_cfg = tile_cfg;
      zgemm(st, g);
      to_host(st, C, dC.p(), (size_t)m * n);
      if (reps > 0) {
        hipEvent_t a, b;
        HIP_CHECK(hipEventCreate(&a));
        HIP_CHECK(hipEventCreate(&b));
        g.C = dC0.p();
        g.beta = make_double2(0.0, 0.0);
        zgemm(st, g);
        HIP_CHECK(hipEventRecord(a, st));
        for (int i = 0; i < reps; ++i) zgemm(st, g);
        HIP_CHECK(hipEventRecord(b, st));
        HIP_CHECK(hipEventSynchronize(b));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        if (ms_out) *ms_out = ms / reps;
        HIP_CHECK(hipEventDestroy(a));
        HIP_CHECK(hipEventDestroy(b));
      }
    }
    HIP_CHECK(hipStreamDestroy(st));
  });
}

// one product through the whole descriptor on the caller's whole buffers (zgemm_args_check.h refuses, before any HIP
// call, whatever would leave them); all of C comes back
int mitdvp_zgemm_desc(int device, const mitdvp_zgemm_args* a, const double* A, size_t nA, const double* B, size_t nB,
                      double* C, size_t nC, const int* klist, size_t nklist) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    zgemm_args_check(a, A, nA, B, nB, C, nC, klist, nklist);
    HIP_CHECK(hipSetDevice(device));
    hipStream_t st;
    HIP_CHECK(hipStreamCreate(&st));
    {
      Dev dA(st, A, nA), dB(st, B, nB), dC(st, C, nC), dK((nklist * sizeof(int) + sizeof(zc) - 1) / sizeof(zc));
      if (klist && nklist) HIP_CHECK(hipMemcpyAsync(dK.p(), klist, nklist * sizeof(int), hipMemcpyHostToDevice, st));
      ZgemmDesc g = zgemm_desc(dA.p() + a->offA, dB.p() + a->offB, dC.p() + a->offC, a->m, a->n, a->k);
      g.transA = a->transA; g.conjA = a->conjA; g.transB = a->transB; g.conjB = a->conjB;
      g.lda = a->lda; g.ldb = a->ldb; g.ldc = a->ldc;
      g.strideA = a->strideA; g.strideB = a->strideB; g.strideC = a->strideC;
      g.batch = a->batch;
      g.alpha = make_double2(a->alpha[0], a->alpha[1]);
      g.beta = make_double2(a->beta[0], a->beta[1]);
      g.tile_cfg = a->tile_cfg;
      g.mode3m = a->mode3m;
      g.arow_skip = a->arow_skip;
      g.rowmap_p = a->rowmap_p; g.rowmap_s1 = a->rowmap_s1; g.rowmap_s2 = a->rowmap_s2; g.rowmap_r0 = a->rowmap_r0;
      if (klist) { g.klist = reinterpret_cast<const int*>(dK.p()); g.klist_stride = a->klist_stride; }
      zgemm(st, g);
      if (nC) to_host(st, C, dC.p(), nC);
      else HIP_CHECK(hipStreamSynchronize(st));
    }
    zgemm_release_stream(st);
    HIP_CHECK(hipStreamDestroy(st));
  });
}

// one reducing product (zgemm_reduce) on the caller's whole buffers, as a side of the edge apply issues it: the core also in
// fragment order whenever the shape runs the unguarded epilogue; zgemm_reduce_args_check.h refuses, before any HIP call,
// whatever would leave a buffer.  The timing bits of MITDVP_ZGEMM_TUNE are not honoured (tune = 0).
int mitdvp_zgemm_reduce(int device, const mitdvp_zgemm_reduce_args* a, const double* A, size_t nA, const double* B, size_t nB,
                        const double* W, size_t nW, double* C, size_t nC, int* variant_out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    if (const char* bad = zgemm_reduce_args_check(a, A, nA, B, nB, W, nW, C, nC)) throw ArgError(bad);
    if (a->m == 0 || a->n == 0) {  // nothing to do: C stays as it is, no device is touched
      if (variant_out) *variant_out = 0;
      return;
    }
    HIP_CHECK(hipSetDevice(device));
    hipStream_t st;
    HIP_CHECK(hipStreamCreate(&st));
    {
      const int kp = a->xm * a->yn;
      Dev dA(st, A, nA), dB(st, B, nB), dW(st, W, nW), dC(st, C, nC), dWf((size_t)a->di * kp);
      const int b4 = a->epi_b4 != 0 && zgemm_reduce_b4_available(st) != 0;
      // the engine's rule (MpoSite::EdgeCache::rebuild, heff_apply_edge): zgemm_reduce_full_ok decides, zgemm_reduce_pack_core packs
      const bool wf = b4 && a->epi_full != 0 && zgemm_reduce_full_ok(st, a->xm, a->yn, a->di) &&
                      zgemm_reduce_pack_core(st, dW.p() + a->offW, a->ldw, a->di, kp, dWf.p());
      ZgemmDesc g = zgemm_desc(dA.p() + a->offA, dB.p() + a->offB, dC.p() + a->offC, a->m, a->n, a->k);
      g.transB = a->transB;
      g.lda = a->lda; g.ldb = a->ldb;
      g.mode3m = a->mode3m;
      g.tune = 0;
      g.epi_w = dW.p() + a->offW; g.epi_ldw = a->ldw; g.epi_xm = a->xm; g.epi_yn = a->yn; g.epi_di = a->di;
      g.epi_wf = wf ? dWf.p() : nullptr;
      g.epi_su = a->su; g.epi_sv = a->sv; g.epi_si = a->si; g.epi_acc = a->acc;
      zgemm_reduce(st, g, a->epi_b4, a->epi_full);
      to_host(st, C, dC.p(), nC);
      if (variant_out) *variant_out = zgemm_reduce_variant(a->xm, a->yn, a->di, b4, wf ? 1 : 0);
    }
    zgemm_release_stream(st);
    HIP_CHECK(hipStreamDestroy(st));
  });
}

// one building block of the batch kernels in one workgroup per copy (k_batch_block): batch_block_check.h refuses, before
// any HIP call, what lies outside the kernels' envelope or the caller's buffers
int mitdvp_batch_block(int device, const mitdvp_batch_block_args* a, const double* in0, size_t n0, const double* in1, size_t n1,
                       const double* in2, size_t n2, const double* in3, size_t n3, double* out0, size_t nout0, double* out1,
                       size_t nout1, double* info, size_t ninfo) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    const void* const in[4] = {in0, in1, in2, in3};
    const size_t nin[4] = {n0, n1, n2, n3};
    BatchBlockFoot f;
    if (const char* bad = batch_block_check(a, in, nin, out0, nout0, out1, nout1, info, ninfo, &f)) throw ArgError(bad);
    HIP_CHECK(hipSetDevice(device));
    hipStream_t st;
    HIP_CHECK(hipStreamCreate(&st));
    {
      const size_t nc = (size_t)a->ncopies;
      Dev d0(st, in0, f.in[0]), d1(st, in1, f.in[1]), d2(st, in2, f.in[2]), d3(st, in3, f.in[3]);
      Dev dout0(nc * f.out0), dout1(nc * f.out1), dwork(nc * f.work_total()), dinfo((nc * f.info + 1) / 2);
      HIP_CHECK(hipMemsetAsync(dout0.p(), 0, nc * f.out0 * sizeof(zc), st));
      if (f.out1) HIP_CHECK(hipMemsetAsync(dout1.p(), 0, nc * f.out1 * sizeof(zc), st));
      HIP_CHECK(hipMemsetAsync(dinfo.p(), 0, (nc * f.info + 1) / 2 * sizeof(zc), st));
      BatchBlockArgs g{};
      g.op = a->op; g.variant = a->variant; g.scl = a->scl;
      for (int k = 0; k < 8; ++k) g.dims[k] = a->dims[k];
      g.in[0] = f.in[0] ? d0.p() : nullptr; g.in[1] = f.in[1] ? d1.p() : nullptr;
      g.in[2] = f.in[2] ? d2.p() : nullptr; g.in[3] = f.in[3] ? d3.p() : nullptr;
      g.out0 = dout0.p(); g.out1 = dout1.p(); g.info = reinterpret_cast<double*>(dinfo.p()); g.work = dwork.p();
      g.foot = f;
      batch_block_launch(st, g, a->ncopies);
      HIP_CHECK(hipMemcpyAsync(info, dinfo.p(), nc * f.info * sizeof(double), hipMemcpyDeviceToHost, st));
      if (f.out1) HIP_CHECK(hipMemcpyAsync(out1, dout1.p(), nc * f.out1 * sizeof(zc), hipMemcpyDeviceToHost, st));
      to_host(st, out0, dout0.p(), nc * f.out0);
    }
    HIP_CHECK(hipStreamDestroy(st));
  });
}

// one call of one host wrapper of vecops.h on a stream of its own, on the caller's whole buffers (the results are in-out:
// up first, the whole buffer back); vecop_check.h refuses, before any HIP call, whatever would leave a buffer
int mitdvp_vecop(int device, const mitdvp_vecop_args* a, const double* z0, size_t nz0, const double* z1, size_t nz1,
                 const double* z2, size_t nz2, const double* r0, size_t nr0, const int* idx, size_t nidx,
                 unsigned long long mask, double* zo0, size_t nzo0, double* zo1, size_t nzo1, double* ro, size_t nro) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    static_assert(VECOP_NPART == NPART && VECOP_MAXK == MAXK && VECOP_SMALL_VEC_N == SMALL_VEC_N, "vecop_check.h repeats vecops.h");
    static_assert(VECOP_MAX_BLOCKS == sizeof(BlockList::idx) / sizeof(int), "vecop_check.h repeats BlockList");
    const void* const zin[3] = {z0, z1, z2};
    const size_t nzin[3] = {nz0, nz1, nz2};
    const void* const zio[2] = {zo0, zo1};
    const size_t nzio[2] = {nzo0, nzo1};
    VecopFoot f;
    if (const char* bad = vecop_check(a, zin, nzin, r0, nr0, idx, nidx, zio, nzio, ro, nro, &f)) throw ArgError(bad);
    if (f.empty && !f.own_return) return;  // nothing to do: the results stay as they are, no device is touched
    HIP_CHECK(hipSetDevice(device));
    struct Stream {  // destroyed also when a wrapper or a HIP call throws
      hipStream_t s = nullptr;
      Stream() { HIP_CHECK(hipStreamCreate(&s)); }
      ~Stream() { (void)hipStreamDestroy(s); }
    } stream;
    hipStream_t st = stream.s;
    {
      // a buffer the op does not take is not passed on: the wrapper gets a null pointer, as from the engine
      Dev d0(st, z0, f.zin[0] ? nz0 : 0), d1(st, z1, f.zin[1] ? nz1 : 0), d2(st, z2, f.zin[2] ? nz2 : 0);
      Dev dr(f.rin ? (nr0 + 1) / 2 : 0), di(f.idx ? (nidx + 3) / 4 : 0);
      Dev o0(st, zo0, f.zio[0] ? nzo0 : 0), o1(st, zo1, f.zio[1] ? nzo1 : 0), dro(f.rio ? (nro + 1) / 2 : 0);
      if (f.rin) HIP_CHECK(hipMemcpyAsync(dr.p(), r0, nr0 * sizeof(double), hipMemcpyHostToDevice, st));
      if (f.idx) HIP_CHECK(hipMemcpyAsync(di.p(), idx, nidx * sizeof(int), hipMemcpyHostToDevice, st));
      if (f.rio) HIP_CHECK(hipMemcpyAsync(dro.p(), ro, nro * sizeof(double), hipMemcpyHostToDevice, st));
      const zc* x0 = f.zin[0] ? d0.p() : nullptr;
      const zc* x1 = f.zin[1] ? d1.p() : nullptr;
      const zc* x2 = f.zin[2] ? d2.p() : nullptr;
      const double* xr = f.rin ? reinterpret_cast<const double*>(dr.p()) : nullptr;
      const int* xi = f.idx ? reinterpret_cast<const int*>(di.p()) : nullptr;
      zc* y0 = f.zio[0] ? o0.p() : nullptr;
      zc* y1 = f.zio[1] ? o1.p() : nullptr;
      double* yr = f.rio ? reinterpret_cast<double*>(dro.p()) : nullptr;
      const long* d = a->dims;
      const long* s = a->strides;
      const int v = a->variant;
      BlockList bl{};
      switch (a->op) {
        case MITDVP_VECOP_DOT: vec_dot(st, x0, x1, d[0], v != 0, y0); break;
        case MITDVP_VECOP_SUMSQ: vec_sumsq(st, x0, d[0], yr); break;
        case MITDVP_VECOP_LANCZOS_UPDATE: vec_lanczos_update(st, y0, x0, x1, d[0], x2, xr, yr); break;
        case MITDVP_VECOP_LANCZOS_UPDATE_DEF:
          vec_lanczos_update_deferred(st, y0, x0, x1, d[0], x2, xr, (int)d[1], (v & 2) != 0, a->eps, yr);
          break;
        case MITDVP_VECOP_LANCZOS_STEP_SMALL: vec_lanczos_step_small(st, y0, (v & 2) ? x1 : x0, x0, x2, d[0], y1, xr, yr, a->eps); break;
        case MITDVP_VECOP_SCALE_INV_NORM: vec_scale_inv_norm(st, y0, d[0], xr, a->eps); break;
        case MITDVP_VECOP_MULTI_DOT: vec_multi_dot(st, x0, s[0], (int)d[1], x1, d[0], y0); break;
        case MITDVP_VECOP_ARNOLDI_UPDATE: vec_arnoldi_update(st, y0, x0, s[0], (int)d[1], d[0], x1, yr); break;
        case MITDVP_VECOP_LINCOMB: {
          Coefs c{};
          for (int j = 0; j < MAXK; ++j) c.c[j] = make_double2(a->coef[2 * j], a->coef[2 * j + 1]);
          vec_lincomb(st, y0, x0, s[0], (int)d[1], c, d[0], yr);
          break;
        }
        case MITDVP_VECOP_AXPBY: vec_axpby(st, y0, x0, d[0], make_double2(a->a[0], a->a[1]), make_double2(a->b[0], a->b[1])); break;
        case MITDVP_VECOP_SCALE: vec_scale(st, y0, d[0], make_double2(a->a[0], a->a[1])); break;
        case MITDVP_VECOP_TRANSPOSE: transpose_batched(st, x0, y0, (int)d[0], (int)d[1], s[0], s[1], (int)d[2], s[2], s[3]); break;
        case MITDVP_VECOP_TRANSPOSE_REV3: transpose_rev3(st, x0, y0, (int)d[0], (int)d[1], (int)d[2]); break;
        case MITDVP_VECOP_PERMUTE_0213: permute_0213(st, x0, y0, d[0], (int)d[1], (int)d[2], (int)d[3]); break;
        case MITDVP_VECOP_PERMUTE5: {
          const int dims[5] = {(int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4]};
          permute5(st, x0, y0, dims, s, (v & 1) ? xi : nullptr);
          break;
        }
        case MITDVP_VECOP_PHYS_DIAG: phys_diag(st, x0, y0, (int)d[0], (int)d[1], (int)d[2], (v & 1) != 0); break;
        case MITDVP_VECOP_COPY2D:
          copy2d(st, y0, s[0], x0, s[1], d[0], (int)d[1], (int)d[2], make_double2(a->a[0], a->a[1]), (v & 1) != 0);
          break;
        case MITDVP_VECOP_COPY_RAW: vec_copy_raw(st, y0, x0, (size_t)d[0]); break;
        case MITDVP_VECOP_IDENTITY: set_identity(st, y0, (int)d[0], (int)d[1], s[0]); break;
        case MITDVP_VECOP_SCALE_COLS: scale_cols(st, y0, d[0], (int)d[1], s[0], xr); break;
        case MITDVP_VECOP_GATHER_BLOCKS:
        case MITDVP_VECOP_FILL_SCALED_BLOCKS:
        case MITDVP_VECOP_ACCUM_SCALED_BLOCKS:
          bl.n = (int)d[2];
          for (int k = 0; k < bl.n; ++k) {
            bl.idx[k] = f.idx ? idx[k] : 0;
            bl.f[k] = make_double2(a->f[2 * k], a->f[2 * k + 1]);
          }
          if (a->op == MITDVP_VECOP_GATHER_BLOCKS) gather_blocks(st, y0, (int)d[3], x0, (int)d[4], d[0], (int)d[1], bl);
          else if (a->op == MITDVP_VECOP_FILL_SCALED_BLOCKS) fill_scaled_blocks(st, y0, s[0], (int)d[3], x0, d[0], (int)d[1], bl);
          else accum_scaled_blocks(st, y0, x0, s[0], x1, d[0], (int)d[1], bl, make_double2(a->both[0], a->both[1]));
          break;
        case MITDVP_VECOP_COL_SUMSQ: col_sumsq(st, x0, d[0], (int)d[1], yr); break;
        case MITDVP_VECOP_ROW_SUMSQ: row_sumsq(st, x0, (int)d[0], d[1], yr); break;
        case MITDVP_VECOP_SHELL_SUMSQ: shell_sumsq(st, x0, (int)d[0], yr); break;
        case MITDVP_VECOP_IDENT_DEV: ident_deviation(st, x0, s[0], (int)d[0], yr); break;
        default: ident_deviation_multi(st, x0, (int)d[1], s[1], s[0], (int)d[0], yr, y1, mask, (v & 1) != 0); break;
      }
      if (f.rio) HIP_CHECK(hipMemcpyAsync(ro, dro.p(), nro * sizeof(double), hipMemcpyDeviceToHost, st));
      if (f.zio[1]) HIP_CHECK(hipMemcpyAsync(zo1, o1.p(), nzo1 * sizeof(zc), hipMemcpyDeviceToHost, st));
      if (f.zio[0]) HIP_CHECK(hipMemcpyAsync(zo0, o0.p(), nzo0 * sizeof(zc), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
    }
  });
}

int mitdvp_bench_heff(int device, int dl, int d, int dr, int ml, int mr, int reps, int warmup, double* ms_out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    Engine e(unit_cfg(device));
    hipStream_t st = e.stream();
    const long ns = (long)dl * d * dr, mm = std::max(ml, mr);
    e.ensure_work(ns, (long)dl * dr * d * mm, (long)dl * dr * d * mm, 1, 1);
    std::vector<double> w((size_t)ml * d * d * mr * 2);
    uint64_t s = 88172645463325252ull;
    for (auto& v : w) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v = ((double)(s >> 11) / 9007199254740992.0 - 0.5) * 0.1; }
    e.set_mpo_core(0, 0, w.data(), ml, d, d, mr);
    const MpoSite& ws = e.mpo(0, 0);
    Dev dL((size_t)dl * ml * dl), dR((size_t)dr * mr * dr), dpsi(ns), dout(ns);
    vec_randn(st, dL.p(), (long)dl * ml * dl, 11);
    vec_randn(st, dR.p(), (long)dr * mr * dr, 12);
    vec_randn(st, dpsi.p(), ns, 13);
    for (int i = 0; i < warmup; ++i) e.heff_apply(dL.p(), ws, dR.p(), dpsi.p(), dout.p(), dl, d, dr, hzc(0, 0));
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    HIP_CHECK(hipEventRecord(a, st));
    for (int i = 0; i < reps; ++i) e.heff_apply(dL.p(), ws, dR.p(), dpsi.p(), dout.p(), dl, d, dr, hzc(0, 0));
    HIP_CHECK(hipEventRecord(b, st));
    HIP_CHECK(hipEventSynchronize(b));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    *ms_out = ms / std::max(reps, 1);
    HIP_CHECK(hipEventDestroy(a));
    HIP_CHECK(hipEventDestroy(b));
  });
}

int mitdvp_qr_thin(int device, const double* a, int m, int n, int gauge_free, double* q_out, double* r_out, int reps,
                   double* ms_out, long* launches, int* path_out) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    if (m < n || n < 1 || reps < 1) throw ArgError("qr_thin: need m >= n >= 1, reps >= 1");
    Engine e(unit_cfg(device));
    hipStream_t st = e.stream();
    Dev A((size_t)m * n), A0(st, a, (size_t)m * n), Q((size_t)m * n), R((size_t)n * n), work(qr_work_elems(m, n));
    if (!a) vec_randn(st, A0.p(), (long)m * n, 21);
    QrHistory* hist = qr_history_new();
    long nl = 0;
    bool used = false;
    auto once = [&] {
      HIP_CHECK(hipMemcpyAsync(A.p(), A0.p(), (size_t)m * n * sizeof(zc), hipMemcpyDeviceToDevice, st));
      qr_thin(st, A.p(), m, n, Q.p(), R.p(), work.p(), &nl, hist, gauge_free != 0, &used);
    };
    try {
      once();
      if (path_out) *path_out = used ? 1 : 0;
      nl = 0;
      hipEvent_t ea, eb;
      HIP_CHECK(hipEventCreate(&ea));
      HIP_CHECK(hipEventCreate(&eb));
      HIP_CHECK(hipEventRecord(ea, st));
      for (int i = 0; i < reps; ++i) once();
      HIP_CHECK(hipEventRecord(eb, st));
      HIP_CHECK(hipEventSynchronize(eb));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, ea, eb));
      if (ms_out) *ms_out = ms / reps;
      if (launches) *launches = nl / reps;
      HIP_CHECK(hipEventDestroy(ea));
      HIP_CHECK(hipEventDestroy(eb));
      if (q_out) to_host(st, q_out, Q.p(), (size_t)m * n);
      if (r_out) to_host(st, r_out, R.p(), (size_t)n * n);
    } catch (...) {
      qr_history_free(hist);
      throw;
    }
    qr_history_free(hist);
  });
}

// device time of one (m x n) QR (Q and R formed), averaged over reps; launches per factorisation in *launches
int mitdvp_bench_qr(int device, int m, int n, int reps, double* ms_out, long* launches) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    NEED(ms_out);
    if (m < n || n < 1 || reps < 1) throw ArgError("bench_qr: need m >= n >= 1, reps >= 1");
    Engine e(unit_cfg(device));
    hipStream_t st = e.stream();
    Dev A((size_t)m * n), A0((size_t)m * n), Q((size_t)m * n), R((size_t)n * n), work(qr_work_elems(m, n));
    vec_randn(st, A0.p(), (long)m * n, 21);
    long nl = 0;
    auto once = [&] {
      HIP_CHECK(hipMemcpyAsync(A.p(), A0.p(), (size_t)m * n * sizeof(zc), hipMemcpyDeviceToDevice, st));
      qr_householder(st, A.p(), m, n, Q.p(), R.p(), work.p(), &nl);
    };
    once();
    nl = 0;
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    HIP_CHECK(hipEventRecord(a, st));
    for (int i = 0; i < reps; ++i) once();
    HIP_CHECK(hipEventRecord(b, st));
    HIP_CHECK(hipEventSynchronize(b));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    *ms_out = ms / reps;
    if (launches) *launches = nl / reps;
    HIP_CHECK(hipEventDestroy(a));
    HIP_CHECK(hipEventDestroy(b));
  });
}

int mitdvp_heff_selfcheck(int device, int dl, int d, int dr, int ml, int mr, double out[4]) {
  return guard(nullptr, [&] {
    using namespace mitdvp;
    Engine e(unit_cfg(device));
    hipStream_t st = e.stream();
    const long ns = (long)dl * d * dr, mm = std::max(ml, mr);
    e.ensure_work(ns, (long)dl * dr * d * mm, (long)dl * dr * d * mm, 1, 1);
    std::vector<double> w((size_t)ml * d * d * mr * 2);
    uint64_t s = 0x2545F4914F6CDD1Dull;
    for (auto& v : w) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v = ((double)(s >> 11) / 9007199254740992.0 - 0.5); }
    e.set_mpo_core(0, 0, w.data(), ml, d, d, mr);
    const MpoSite& ws = e.mpo(0, 0);
    Dev dL((size_t)dl * ml * dl), dR((size_t)dr * mr * dr), x(ns), y(ns), z(ns), hx(ns), hy(ns), hz(ns), h4(ns);
    vec_randn(st, dL.p(), (long)dl * ml * dl, 21);
    vec_randn(st, dR.p(), (long)dr * mr * dr, 22);
    vec_randn(st, x.p(), ns, 23);
    vec_randn(st, y.p(), ns, 24);
    const zc one = make_double2(1.0, 0.0), mone = make_double2(-1.0, 0.0), twoi = make_double2(0.0, 2.0),
             mtwoi = make_double2(0.0, -2.0);
    HIP_CHECK(hipMemcpyAsync(z.p(), x.p(), ns * sizeof(zc), hipMemcpyDeviceToDevice, st));
    vec_axpby(st, z.p(), y.p(), ns, twoi, one);  // z = x + 2i y
    const int saved = zgemm_default_mode();
    Dev red(NPART);
    double* rp = reinterpret_cast<double*>(red.p());
    auto nrm = [&](zc* v) {
      std::vector<double> h(NPART);
      vec_sumsq(st, v, ns, rp);
      HIP_CHECK(hipMemcpyAsync(h.data(), rp, NPART * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      double t = 0;
      for (double q : h) t += q;
      return std::sqrt(t);
    };
    zgemm_set_default_mode(0);
    e.heff_apply(dL.p(), ws, dR.p(), x.p(), h4.p(), dl, d, dr, hzc(0, 0));
    zgemm_set_default_mode(1);
    e.heff_apply(dL.p(), ws, dR.p(), x.p(), hx.p(), dl, d, dr, hzc(0, 0));
    zgemm_set_default_mode(saved);
    const double n4 = nrm(h4.p());
    vec_axpby(st, h4.p(), hx.p(), ns, mone, one);  // h4 - hx
    out[0] = nrm(h4.p()) / n4;
    e.heff_apply(dL.p(), ws, dR.p(), y.p(), hy.p(), dl, d, dr, hzc(0, 0));
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    HIP_CHECK(hipEventRecord(a, st));
    e.heff_apply(dL.p(), ws, dR.p(), z.p(), hz.p(), dl, d, dr, hzc(0, 0));
    HIP_CHECK(hipEventRecord(b, st));
    const double nz = nrm(hz.p());
    vec_axpby(st, hz.p(), hx.p(), ns, mone, one);
    vec_axpby(st, hz.p(), hy.p(), ns, mtwoi, one);
    out[1] = nrm(hz.p()) / nz;
    out[2] = nrm(hx.p());
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    out[3] = ms;
    HIP_CHECK(hipEventDestroy(a));
    HIP_CHECK(hipEventDestroy(b));
  });
}

int mitdvp_set_gemm_mode(int mode3m) {
  mitdvp::zgemm_set_default_mode(mode3m);
  return MITDVP_OK;
}
int mitdvp_get_gemm_mode(void) { return mitdvp::zgemm_default_mode(); }

int mitdvp_mfma_peak_probe(int device, double* tflops_out) {
  return guard(nullptr, [&] {
    HIP_CHECK(hipSetDevice(device));
    *tflops_out = mitdvp::mfma_peak_probe(nullptr);
  });
}
int mitdvp_clock_probe(int device, long iters, double* cycles_ticks_out) {
  return guard(nullptr, [&] {
    HIP_CHECK(hipSetDevice(device));
    double o[3];
    mitdvp::clock_probe(nullptr, iters, o);
    cycles_ticks_out[0] = o[0];
    cycles_ticks_out[1] = o[1];
  });
}
int mitdvp_cu_mask_probe(int device, const unsigned* mask, int nwords, int nblocks, size_t lds_bytes, int spin_us, int* out) {
  return guard(nullptr, [&] {
    HIP_CHECK(hipSetDevice(device));
    mitdvp::where_probe(mask, nwords, nblocks, lds_bytes, spin_us, out);
  });
}
int mitdvp_mfma_layout_probe(int device, int* out) {
  return guard(nullptr, [&] {
    HIP_CHECK(hipSetDevice(device));
    mitdvp::mfma_layout_probe(nullptr, out);
  });
}

}  // extern "C"
