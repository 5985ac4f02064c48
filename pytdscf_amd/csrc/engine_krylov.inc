// engine_krylov.inc -- bodies of the Engine member templates (local propagators); included by
// every translation unit that instantiates them with its own matvec lambda.
#pragma once
#include "engine_internal.h"

namespace mitdvp {

// ---------------------------------------------------------------------------
// local propagator: x <- exp(scale*Op) x, with the Ritz step and the convergence test on the device (krylov_dev.h;
// small_linalg.h keeps their host twins, which the tests pin the device forms against).  Which iterations
// are inspected is the reference's rule (_iter_info, _integrator.py:178-186; :578-579) and depends on k_prev only, so the
// host queues the inspections without looking at any result; convergence needs two consecutive Ritz vectors (:638-651),
// i.e. cannot come before iteration n_warm + 1 unless the Krylov space is exhausted: that is the first record the host
// waits for.  In the steady state (the count equals the one remembered for this site) a local exponential costs ONE
// host read; every further iteration one more.
// ---------------------------------------------------------------------------
template <class MV>
int Engine::krylov_exp(hzc scale, MV&& matvec, zc* x, long n, int k_prev, long nsize) {
  // nsize: element count of the UNPADDED input tensor (adaptive rank: x is zero-padded to
  // the output shape but _iter_info still counts psi_states, _integrator.py:178-186, :524)
  if (nsize <= 0) nsize = n;
  const int ndim = (int)std::min<long>(nsize, cfg.max_krylov);
  const int n_warm = (int)std::min<long>(nsize, std::min(std::max(0, k_prev - 2), 15));
  const bool lanczos = cfg.integrator == MITDVP_LANCZOS;
  const bool cn = cfg.conserve_norm != 0;
  zc* V = V_.p;
  const long ldv = n;
  zc* alpha_p = red_.p + RED_ALPHA;
  double* nrm_p = reinterpret_cast<double*>(red_.p + RED_NRM);
  zc* h_p = red_.p + RED_H;
  double* misc_d = reinterpret_cast<double*>(red_.p + RED_MISC);
  double* b0_d = misc_d + 2 * NPART;  // |x|^2 partials of _normalize (:189-203), kept until the first inspection

  HIP_CHECK(hipMemcpyAsync(V, x, n * sizeof(zc), hipMemcpyDeviceToDevice, st_));
  if (!cn) {
    vec_sumsq(st_, x, n, b0_d);
    vec_scale_inv_norm(st_, V, n, b0_d, 1e-300);  // a zero vector stays zero and is reported below
    cnt_.n_launch += 2;
  }
  // the first iteration whose record the host reads
  const int l_sync = (int)std::min<long>(std::min(n_warm + 1, ndim - 1), nsize - 1);
  bool first = true;
  int q0 = 0;
  // deferred normalisation (Lanczos, vectors too long for the one-workgroup step kernel): the basis stays unnormalised
  // and every consumer applies 1 / beta on the fly -- one launch and one pass over the vector less per iteration
  const bool small_step = lanczos && n <= SMALL_VEC_N && small_kernels_;
  const bool deferred = lanczos && !small_step;
  for (int l = 0; l < ndim; ++l) {
    zc* vl = V + (size_t)l * ldv;
    zc* vn = V + (size_t)(l + 1) * ldv;
    matvec(vl, vn);
    timer_begin(4);
    if (deferred) {
      vec_dot(st_, cfg.lanczos_variant == 0 ? V : vl, vn, n, true, alpha_p + (size_t)l * NPART);
      vec_lanczos_update_deferred(st_, vn, vl, l > 0 ? V + (size_t)(l - 1) * ldv : nullptr, n, alpha_p + (size_t)l * NPART, nrm_p, l,
                                  cfg.lanczos_variant != 0, KRYLOV_EPS, nrm_p + (size_t)l * NPART);
      cnt_.n_launch += 2;
    } else if (small_step) {
      vec_lanczos_step_small(st_, vn, cfg.lanczos_variant == 0 ? V : vl, vl, l > 0 ? V + (size_t)(l - 1) * ldv : nullptr, n,
                             alpha_p + (size_t)l * NPART, l > 0 ? nrm_p + (size_t)(l - 1) * NPART : nullptr,
                             nrm_p + (size_t)l * NPART, KRYLOV_EPS);
      cnt_.n_launch += 1;
    } else {  // Arnoldi
      vec_multi_dot(st_, V, ldv, l + 1, vn, n, h_p + (size_t)l * MAXK * NPART);
      vec_arnoldi_update(st_, vn, V, ldv, l + 1, n, h_p + (size_t)l * MAXK * NPART, nrm_p + (size_t)l * NPART);
      vec_scale_inv_norm(st_, vn, n, nrm_p + (size_t)l * NPART, KRYLOV_EPS);
      cnt_.n_launch += 3;
    }
    const bool last_possible = (l + 1 == nsize);
    if (l < n_warm && !last_possible && l + 1 < ndim) {  // warm-up: not inspected (:578-579)
      timer_end();
      continue;
    }
    KryRitzArgs a{};
    a.st = kst_;
    a.alpha_p = alpha_p; a.nrm_p = nrm_p; a.h_p = h_p;
    a.beta0_p = cn ? nullptr : b0_d;
    a.l = l; a.q0 = q0; a.n_warm = n_warm; a.ndim = ndim; a.nsize = nsize;
    a.lanczos = lanczos ? 1 : 0;
    a.first = first ? 1 : 0;
    a.scale = make_double2(scale.real(), scale.imag());
    a.eps = KRYLOV_EPS;
    a.deferred = deferred ? 1 : 0;
    a.orthodox = cfg.lanczos_variant != 0 ? 1 : 0;
    kry_ritz(st_, a);
    const unsigned tag = ++kry_tag_;
    kry_diff(st_, kst_, V, ldv, n, cfg.thresh, h_kpub_.d, tag);
    cnt_.n_launch += 2;
    timer_end();
    first = false;
    q0 = l + 1;
    if (l < l_sync) continue;
    wait_pub(tag);
    cnt_.n_host_waits += 1;
    if (h_kpub_.h->state == KRY_RUNNING) continue;
    const int k = h_kpub_.h->k;
    const double beta0 = h_kpub_.h->beta0;
    if (!cn && !(beta0 > 0.0)) throw ArgError("Initial psi has zero norm.");
    Coefs c{};
    for (int j = 0; j < k; ++j) {
      const zc v = h_kpub_.h->coef[j];
      c.c[j] = cn ? v : make_double2(v.x * beta0, v.y * beta0);  // _rescale, :206-213
    }
    if (cn) {
      vec_lincomb(st_, x, V, ldv, k, c, n, misc_d);
      vec_scale_inv_norm(st_, x, n, misc_d, 0.0);
    } else {
      vec_lincomb(st_, x, V, ldv, k, c, n, nullptr);
    }
    cnt_.n_launch += 2;
    return k;
  }
  throw NotConverged(std::string(lanczos ? "Short Iterative Lanczos" : "Short Iterative Arnoldi") +
                     " is not converged in " + std::to_string(ndim) + " basis. Try shorter time interval.");
}

// ---------------------------------------------------------------------------
// improved relaxation: lowest eigenvector of H_eff by Lanczos
// (matrix_diagonalize_lanczos, _integrator.py:74-138): orthodox Lanczos
// (alpha_l = Re <v_l|H|v_l>), the projected tridiagonal problem is solved on the
// host after every new vector, convergence on the change of the Ritz vector.
// The Ritz vector's sign is fixed by a non-negative overlap with the start
// vector (LAPACK leaves it arbitrary; only the global phase of the state is
// affected).  The change ||psi_k - psi_{k-1}|| is evaluated in the Lanczos
// coefficient space (the basis is orthonormal to working accuracy).
// ---------------------------------------------------------------------------
template <class MV>
int Engine::krylov_diag(MV&& matvec, zc* x, long n) {
  const int kcap = (int)std::min<long>(n, max_diag_krylov_);
  Vdiag_.reserve((size_t)(kcap + 1) * n);
  zc* V = Vdiag_.p;
  zc* alpha_p = red_.p + RED_ALPHA;
  double* nrm_p = reinterpret_cast<double*>(red_.p + RED_NRM);
  HIP_CHECK(hipMemcpyAsync(V, x, n * sizeof(zc), hipMemcpyDeviceToDevice, st_));
  std::vector<double> alpha, beta;  // beta[i] = norm of vector i+1 before normalisation
  std::vector<double> prev;
  auto finalize = [&](const std::vector<double>& c) {
    const int k = (int)c.size();
    double* misc_d = reinterpret_cast<double*>(red_.p + RED_MISC);
    for (int c0 = 0; c0 < k; c0 += MAXK) {  // sum_j c_j V_j in chunks of MAXK vectors
      const int kc = std::min(MAXK, k - c0);
      Coefs cf{};
      for (int j = 0; j < kc; ++j) cf.c[j] = make_double2(c[c0 + j], 0.0);
      if (c0 == 0) {
        vec_lincomb(st_, x, V, n, kc, cf, n, nullptr);
      } else {
        vec_lincomb(st_, tmp1_.p, V + (size_t)c0 * n, n, kc, cf, n, nullptr);
        vec_axpby(st_, x, tmp1_.p, n, make_double2(1.0, 0.0), make_double2(1.0, 0.0));
      }
    }
    vec_sumsq(st_, x, n, misc_d);  // renormalise (get_C_sval_states_norm, _mps_cls.py:1083-1084)
    vec_scale_inv_norm(st_, x, n, misc_d, 0.0);
  };
  for (int i = 0; i < kcap; ++i) {
    zc* vi = V + (size_t)i * n;
    zc* vn = V + (size_t)(i + 1) * n;
    matvec(vi, vn);
    const int slot = i % MAXK;  // scalar slots are recycled; they are read every iteration
    vec_dot(st_, vi, vn, n, true, alpha_p + (size_t)slot * NPART);
    const int pslot = (i + MAXK - 1) % MAXK;
    vec_lanczos_update(st_, vn, vi, i > 0 ? V + (size_t)(i - 1) * n : nullptr, n, alpha_p + (size_t)slot * NPART,
                       i > 0 ? nrm_p + (size_t)pslot * NPART : nullptr, nrm_p + (size_t)slot * NPART);
    vec_scale_inv_norm(st_, vn, n, nrm_p + (size_t)slot * NPART, KRYLOV_EPS);
    cnt_.n_launch += 3;
    read_partials(RED_ALPHA + (size_t)slot * NPART, NPART);
    read_partials(RED_NRM, (size_t)MAXK * NPART / 2 + 1);
    double a = 0, b2 = 0;
    for (int q = 0; q < NPART; ++q) a += h_red_.h[RED_ALPHA + (size_t)slot * NPART + q].x;
    const double* np_ = reinterpret_cast<const double*>(h_red_.h + RED_NRM) + (size_t)slot * NPART;
    for (int q = 0; q < NPART; ++q) b2 += np_[q];
    alpha.push_back(a);
    beta.push_back(std::sqrt(b2));
    const int k = i + 1;
    std::vector<double> c = tridiag_eigvec(alpha, beta, k, 0, nullptr);
    if (c.empty()) throw NotConverged("tridiagonal eigen-solver did not converge");
    bool done = beta.back() < KRYLOV_EPS || k == n;
    if (!done && i > 0) {
      double err = 0;
      for (int j = 0; j < k; ++j) {
        const double dlt = c[j] - (j < (int)prev.size() ? prev[j] : 0.0);
        err += dlt * dlt;
      }
      done = std::sqrt(err) < cfg.thresh;
    }
    if (done) {
      finalize(c);
      return k;
    }
    prev = c;
  }
  throw NotConverged("Lanczos Diagonalization is not converged in " + std::to_string(kcap) + " basis");
}

}  // namespace mitdvp
