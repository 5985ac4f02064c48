// engine_apply.hip -- the contractions of the large-bond hot path: H_eff / K_eff applies in all their forms, the
// environment update, and the identity checks of the environment blocks that choose between the forms.
#include "engine_internal.h"
#include "core_lists.h"

namespace mitdvp {

// 64 x 64 tiles each product of a Strassen level must have for a folded side to take that level by default
// (choose_apply_forms): one whole round on the 256 compute units, seven or 49 in the batched launch.  Measured per apply
// (profiles/fold_strassen_ab.txt): 1024 tiles (C4, 1024 x 16 x 1024) -12.5 %, 256 tiles (512 x 16 x 512) -11 %, 64 tiles
// (C5, 512 x 4 x 512) +1 % and the factors to pack on top; nothing between 64 and 256 has been measured.  The second level
// (profiles/fold_strassen2_ab.txt): 256 tiles per quarter-size product (C4) -9.5 % per apply on top of the first and +2.8 ms
// of packing per solve; 64 tiles (512 x 16 x 512) -1.7 % per apply, which the 0.52 ms of extra packing takes back.
constexpr long STRASSEN_MIN_TILES = 256;

// W stage: Y_b[(i,q)][n] = W2[(i,q)][(p,j)] X_b[(p,j)][n] for nbatch slabs b (X_, Y_ workspaces).  With a
// finite-state-machine MPO most (p, q) blocks of W are zero: rows of W2 ordered (q, i), per 64-row tile the list of
// 16-wide K tiles that hold a non-zero; row ranges that need most K tiles go through the plain kernel, the others
// through the list kernel, Y's rows are mapped back to (i, q).  Skipping exact zeros leaves Y bit-identical.
double Engine::w_stage(const MpoSite* sp, int side, const zc* w2, int d, int mout, int min_, int ncol, int nbatch) {
  ZgemmDesc g = zgemm_desc(w2, X_.p, Y_.p, d * mout, ncol, min_ * d);
  g.batch = nbatch; g.strideA = 0; g.strideB = (long)min_ * d * ncol; g.strideC = (long)d * mout * ncol;
  const bool use = sp && sparse_w_ && ncol >= 64 && (side == 0 ? sp->kl_l.p : sp->kl_r.p) &&
                   (side == 0 ? sp->sp_frac_l : sp->sp_frac_r) <= 0.6;
  if (!use) {
    zgemm(st_, g);
    return 1.0;
  }
  const zc* wt = side == 0 ? sp->w2lt.p : sp->w2rt.p;
  const int* kl = reinterpret_cast<const int*>(side == 0 ? sp->kl_l.p : sp->kl_r.p);
  const int stride = side == 0 ? sp->kl_stride_l : sp->kl_stride_r;
  const auto& segs = side == 0 ? sp->seg_l : sp->seg_r;
  const int K = min_ * d;
  // heavy ranges first: they are the long-running workgroups
  for (int pass = 0; pass < 2; ++pass)
    for (const auto& sgm : segs) {
      if (sgm.dense != (pass == 0)) continue;
      ZgemmDesc h = g;
      h.A = wt + (size_t)sgm.r0 * K;
      h.M = sgm.r1 - sgm.r0;
      h.rowmap_p = d; h.rowmap_s1 = (long)mout * ncol; h.rowmap_s2 = ncol; h.rowmap_r0 = sgm.r0;
      if (!sgm.dense) { h.klist = kl + (size_t)sgm.tile0 * stride; h.klist_stride = stride; }
      h.tile_cfg = (sgm.dense && h.M <= 32) ? 2 : 1;  // a dense state of <= 32 rows: the 32 x 32 tile, no rows wasted
      zgemm(st_, h);
      cnt_.n_launch += 1;
    }
  cnt_.n_launch -= 1;  // the caller counts one launch for this stage
  return side == 0 ? sp->sp_frac_l : sp->sp_frac_r;
}

// The blocks may be rectangular (bra bond != ket bond): L (dlo, ml, dli), R (dro, mr, dri),
// psi (dli, d, dri) -> out (dlo, d, dro).  That is the adaptive-rank case
// (tensor_shapes_out, _contraction.py:455-477); the plain sweep has dlo == dli, dro == dri.
void Engine::heff_apply_rect(const zc* L, const MpoSite& w, const zc* R, const zc* psi, zc* out, int dlo, int dli,
                             int d, int dro, int dri, const ApplyPlan& plan) {
  const int ml = w.ml, mr = w.mr;
  int a0, a1;
  const bool sharded = shard_range(dlo, a0, a1);
  const int na = a1 - a0;
  timer_begin(10);
  const bool triml = plan.trim_l && !sharded && dlo == dli && ml > 1;
  if (triml) {
    // L[:, 0, :] is the identity: rows (a, c = 0) of X are psi itself, the GEMM runs over the other ml - 1 rows of
    // every slab (A rows gathered, C rows scattered with the same map)
    const zc one = make_double2(1.0, 0.0);
    const long row = (long)d * dri;
    copy2d(st_, X_.p, (long)ml * row, psi, row, na, (int)row, 0, one, false);
    ZgemmDesc g = zgemm_desc(L, psi, X_.p + row, na * (ml - 1), d * dri, dli);
    g.arow_skip = ml;
    g.rowmap_p = ml - 1; g.rowmap_s1 = row; g.rowmap_s2 = (long)ml * row; g.rowmap_r0 = 0;
    g.tile_cfg = 1;
    zgemm(st_, g);
    cnt_.n_launch += 1;
    cnt_.heff_flops_skipped += 8.0 * (double)na * dli * d * dri;
  } else {  // X[(a,c)][(j,s)] = L[(a,c)][b] psi[b][(j,s)]
    ZgemmDesc g = zgemm_desc(L + (size_t)a0 * ml * dli, psi, X_.p, na * ml, d * dri, dli);
    zgemm(st_, g);
  }
  timer_end();
  timer_begin(11);
  // Y_a[(i,t)][s] = W2L[(i,t)][(c,j)] X_a[(c,j)][s]
  const double s2_frac = w_stage(&w, 0, w.w2l.p, d, mr, ml, dri, na);
  timer_end();
  timer_begin(12);
  const bool trim = plan.trim_r && !sharded && dro == dri && mr > 1;
  if (trim) {
    // R[:, mr-1, :] is the identity: its K block of the contraction is a strided copy of Y, the GEMM runs over the
    // other mr - 1 blocks and adds to it
    const zc one = make_double2(1.0, 0.0);
    copy2d(st_, out + (size_t)a0 * d * dro, dro, Y_.p + (size_t)(mr - 1) * dri, (long)mr * dri, (long)na * d, dro, 0, one, false);
    ZgemmDesc g = zgemm_desc(Y_.p, R, out + (size_t)a0 * d * dro, na * d, dro, (mr - 1) * dri);
    g.lda = (long)mr * dri; g.transB = 1; g.ldb = (long)mr * dri; g.beta = one;
    zgemm(st_, g);
    cnt_.n_launch += 1;
    cnt_.heff_flops_skipped += 8.0 * (double)na * d * dro * dri;
  } else {  // out[(a,i)][r] = Y[(a,i)][(t,s)] R[r][(t,s)]
    ZgemmDesc g = zgemm_desc(Y_.p, R, out + (size_t)a0 * d * dro, na * d, dro, mr * dri);
    g.transB = 1; g.ldb = (long)mr * dri;
    zgemm(st_, g);
  }
  timer_end();
  if (sharded) collective(COLL_ALLGATHER, out, (size_t)dlo * d * dro);
  cnt_.n_launch += 3;
  cnt_.n_heff += 1;
  cnt_.heff_flops += 8.0 * ((double)na * dli * ml * d * dri + (double)na * dri * ml * mr * d * d + (double)na * dro * dri * mr * d);
  cnt_.heff_flops_skipped += 8.0 * (1.0 - s2_frac) * ((double)na * dri * ml * mr * d * d);
  cnt_.heff_stage_flops[0] += 8.0 * (double)na * (triml ? ml - 1 : ml) * dli * d * dri;
  cnt_.heff_stage_flops[1] += 8.0 * s2_frac * ((double)na * dri * ml * mr * d * d);
  cnt_.heff_stage_flops[2] += 8.0 * (double)na * d * dro * (trim ? mr - 1 : mr) * dri;
}

bool Engine::try_reserve(DevBuf& b, size_t elems) {
  if (elems <= b.n) return true;
  zc* q = nullptr;  // the new buffer first: a refusal leaves the old one, which an earlier side's plan may count on
  if (hipMalloc(&q, elems * sizeof(zc)) != hipSuccess) { (void)hipGetLastError(); return false; }
  b.release();
  b.p = q; b.n = elems;
  return true;
}

// One folded side of an apply as seven half-size products (ApplyPlan::strassen_l / strassen_r; the formulas: vecops.h).
// out ((2 hm) x (2 hn), leading dimension ldpsi) (+)= A B with the contraction 2 hk long.  fixed: the operator's seven
// packed factors, the left ones of GL (fixed_is_a; psi is B, (2 hk) x (2 hn)) or the right ones of GR^T as stored, each
// hn x hk for a transB product (psi is A, (2 hm) x (2 hk)).  Every summation order is fixed: the same bits every run.
//
// level 2: each of the seven is itself seven quarter-size products.  fixed then holds the operator's 49 quarter-size factors,
// (k1, k2) at (7 k1 + k2) quarter-size matrices; psi's seven level-1 factors go to the head of str_v_ and their 49 factors
// behind them (one batched packing launch over the seven); the 49 products go behind the level-1 area of str_m_, one batched
// pass combines them into the seven half-size products at its head (written, never added to), and the level-1 pass ends.
// That is the two-pass form (the R side; MITDVP_STRASSEN_FUSE=0).  By default a level-2 L side packs psi's 49 factors in one launch from
// psi's 16 blocks (strassen_operands2) and combines the 49 products into out in one launch (strassen_combine2), both with
// the sums of the two passes in their order (the same bits): neither the seven factors nor the seven products are written.
void Engine::strassen_side(const zc* fixed, bool fixed_is_a, const zc* psi, long ldpsi, zc* out, long hm, long hn, long hk,
                           bool accumulate, int level) {
  const long vr = fixed_is_a ? hk : hm, vc = fixed_is_a ? hn : hk;  // psi's level-1 factors: vr x vc
  const int vset = fixed_is_a ? STRASSEN_B : STRASSEN_A;
  // (the L side only: measured on the R side, the one-pass kernels' gain stayed under ten spreads of repeated groups --
  // profiles/env_reuse_ab.txt -- so that side keeps the two passes)
  const bool fused = level == 2 && strassen_fuse_ && fixed_is_a;
  int np = 7;
  long pm = hm, pn = hn, pk = hk;
  const zc* V = str_v_.p;
  zc* Mp = str_m_.p;
  if (fused) {  // psi's 49 straight from its 16 blocks, the products at the head of str_m_: no level-1 area in either buffer
    strassen_operands2(st_, psi, ldpsi, vr / 2, vc / 2, str_v_.p, vset);
    np = 49; pm = hm / 2; pn = hn / 2; pk = hk / 2;
  } else {
    strassen_operands(st_, psi, ldpsi, vr, vc, str_v_.p, vset);
    if (level == 2) {
      zc* v2 = str_v_.p + 7 * vr * vc;
      strassen_operands(st_, str_v_.p, vc, vr / 2, vc / 2, v2, vset, 7, vr * vc, 7 * (vr / 2) * (vc / 2));
      np = 49; pm = hm / 2; pn = hn / 2; pk = hk / 2;
      V = v2;
      Mp = str_m_.p + 7 * hm * hn;
    }
  }
  const zc* A = fixed_is_a ? fixed : V;
  const zc* B = fixed_is_a ? V : fixed;
  ZgemmDesc g = zgemm_desc(A, B, Mp, (int)pm, (int)pn, (int)pk);
  if (!fixed_is_a) { g.transB = 1; g.ldb = pk; }
  if (strassen_batched_) {
    g.batch = np; g.strideA = pm * pk; g.strideB = pk * pn; g.strideC = pm * pn;
    zgemm(st_, g);
  } else {
    for (int k = 0; k < np; ++k) {
      ZgemmDesc h = g;
      h.A = A + k * pm * pk; h.B = B + k * pk * pn; h.C = Mp + k * pm * pn;
      zgemm(st_, h);
    }
  }
  if (fused) {
    strassen_combine2(st_, Mp, pm, pn, out, ldpsi, accumulate);
  } else {
    if (level == 2) strassen_combine(st_, Mp, pm, pn, str_m_.p, hn, false, 7, 7 * pm * pn, hm * hn);
    strassen_combine(st_, str_m_.p, hm, hn, out, ldpsi, accumulate);
  }
  cnt_.n_launch += (fused ? 2 : level == 2 ? 4 : 2) + (strassen_batched_ ? 1 : np);
}

// The apply for an edge-structured core between canonical environments (MpoSite::EdgeCache; L[:, 0, :] = R[:, mr-1, :] = 1,
// verified numerically by choose_apply_forms).  All terms with c = 0 see X_0 = psi, all terms with t = mr - 1 see the
// identity on the right, and there are no others:
//   sigma[a,i,r] = sum_{j,t} W[0,i,j,t] T[(a,j)][(r,t)],        T = psi[(a,j)][s] R[(r,t)][s]^T        ("R side")
//                + sum_{c>=1,j} W[c,i,j,mr-1] X[(a,c)][(r,j)],  X = L[(a,c)][b] psiT[b][(r,j)]        ("L side")
// Both are GEMMs of the size of stages S1 / S3 whose 64 x 64 tiles hold whole (j, t) / (c, j) groups and are contracted
// with the d x (d M) reduced core in the epilogue (zgemm_reduce): the M-fold intermediates X and Y of the three-stage
// chain ("must be tiled / fused") are never written.  psiT = psi with its last two indices swapped.
//
// The folded variant (ApplyPlan::fold_r / fold_l, per side, chosen and built by choose_apply_forms): the M-fold product of a side
// is not needed when its MPO bond is wider than d.  With the reduced core contracted into the block once per local solve,
//   GR[(i,r)][(j,s)] = sum_t wr[i,j,t] R[r,t,s]   (in Y_),      GL[(a,i)][(b,j)] = sum_c wl[i,c,j] L[a,c,b]   (in X_),
// the side is one plain GEMM, sigma[a][(i,r)] = psi[a][(j,s)] GR^T resp. sigma[(a,i)][r] += GL psi[(b,j)][r]: mr / d
// resp. ml / d times fewer products, no transpose, no epilogue.
void Engine::heff_apply_edge(const zc* L, const MpoSite& w, const zc* R, const zc* psi, zc* out, int dl, int d, int dr,
                             const ApplyPlan& plan) {
  const int ml = w.ml, mr = w.mr;
  const MpoSite::EdgeCache& c = w.edge;
  bool first = true;
  double exe = 0.0;
  if (c.has_r && plan.fold_r && plan.strassen_r) {  // sigma[a][(i,r)] = psi GR^T: psi's factors per apply, GR's in str_r_
    timer_begin(12);
    const bool two = plan.strassen_r == 2;
    strassen_side(str_r_.p, false, psi, (long)d * dr, out, dl / 2, (long)d * dr / 2, (long)d * dr / 2, false,
                  plan.strassen_r);
    timer_end();
    first = false;
    const double f = (two ? 49.0 / 8.0 : 7.0) * (double)dl * d * dr * d * dr;
    exe += f;
    cnt_.heff_stage_flops[2] += f;
  } else if (c.has_r && plan.fold_r) {
    timer_begin(12);
    ZgemmDesc g = zgemm_desc(psi, Y_.p, out, dl, d * dr, d * dr);
    g.transB = 1; g.ldb = (long)d * dr;
    zgemm(st_, g);
    timer_end();
    first = false;
    cnt_.n_launch += 1;
    exe += 8.0 * (double)dl * d * dr * d * dr;
    cnt_.heff_stage_flops[2] += 8.0 * (double)dl * d * dr * d * dr;
  } else if (c.has_r) {  // R side: rows (a, j), columns (r, t)
    timer_begin(12);
    ZgemmDesc g = zgemm_desc(psi, R, out, dl * d, dr * mr, dr);
    g.transB = 1; g.ldb = dr;
    g.epi_w = c.w_r.p; g.epi_ldw = (long)d * mr; g.epi_xm = d; g.epi_yn = mr; g.epi_di = d;
    g.epi_wf = c.rf_ok ? c.w_rf.p : nullptr;
    g.epi_su = (long)d * dr; g.epi_sv = 1; g.epi_si = dr; g.epi_acc = 0;
    zgemm_reduce(st_, g);
    timer_end();
    first = false;
    cnt_.n_launch += 1;
    exe += 8.0 * ((double)dl * d * dr * mr * dr + (double)dl * dr * d * d * mr);
    cnt_.heff_stage_flops[2] += 8.0 * ((double)dl * d * dr * mr * dr + (double)dl * dr * d * d * mr);
  }
  if (c.has_l && plan.fold_l && plan.strassen_l) {  // sigma[(a,i)][r] (+)= GL psi: GL's factors in str_l_, psi's per apply;
    timer_begin(10);                                 // the combining pass adds to what the R side wrote
    const bool two = plan.strassen_l == 2;
    strassen_side(str_l_.p, true, psi, dr, out, (long)dl * d / 2, dr / 2, (long)dl * d / 2, !first, plan.strassen_l);
    timer_end();
    first = false;
    const double f = (two ? 49.0 / 8.0 : 7.0) * (double)dl * d * dl * d * dr;
    exe += f;
    cnt_.heff_stage_flops[0] += f;
  } else if (c.has_l && plan.fold_l) {
    timer_begin(10);
    ZgemmDesc g = zgemm_desc(X_.p, psi, out, dl * d, dr, dl * d);
    if (!first) g.beta = make_double2(1.0, 0.0);
    zgemm(st_, g);
    timer_end();
    first = false;
    cnt_.n_launch += 1;
    exe += 8.0 * (double)dl * d * dl * d * dr;
    cnt_.heff_stage_flops[0] += 8.0 * (double)dl * d * dl * d * dr;
  } else if (c.has_l) {
    timer_begin(11);
    transpose_batched(st_, psi, X_.p, d, dr, dr, d, dl, (long)d * dr, (long)d * dr);  // psiT[b][s][j]
    timer_end();
    timer_begin(10);
    // L side: rows (a, c), columns (s, j)
    ZgemmDesc g = zgemm_desc(L, X_.p, out, dl * ml, dr * d, dl);
    g.epi_w = c.w_l.p; g.epi_ldw = (long)ml * d; g.epi_xm = ml; g.epi_yn = d; g.epi_di = d;
    g.epi_wf = c.lf_ok ? c.w_lf.p : nullptr;
    g.epi_su = (long)d * dr; g.epi_sv = 1; g.epi_si = dr; g.epi_acc = first ? 0 : 1;
    zgemm_reduce(st_, g);
    timer_end();
    first = false;
    cnt_.n_launch += 2;
    exe += 8.0 * ((double)dl * ml * dl * d * dr + (double)dl * dr * d * ml * d);
    cnt_.heff_stage_flops[0] += 8.0 * ((double)dl * ml * dl * d * dr + (double)dl * dr * d * ml * d);
  }
  if (first) HIP_CHECK(hipMemsetAsync(out, 0, (size_t)dl * d * dr * sizeof(zc), st_));  // a zero core
  cnt_.n_heff += 1;
  cnt_.n_heff_edge += 1;
  const double alg = 8.0 * ((double)dl * dl * ml * d * dr + (double)dl * dr * ml * mr * d * d + (double)dl * dr * dr * mr * d);
  cnt_.heff_flops += alg;
  cnt_.heff_flops_skipped += alg - exe;
}

// One look at the MPO-bond states ms / me of the two blocks: one clear, two launches, and the record back through the
// pinned mirror of the reduction area (read_partials: ~10 us; a copy into pageable host memory followed by a stream
// synchronisation measured ~120 us of idle GPU per site, 9 % of a C3 sweep).  Valid until that area's next use.
const Engine::IdentRecord& Engine::identity_sets(const zc* L, int ml, int dl, unsigned long long ms, const zc* R, int mr, int dr,
                                                 unsigned long long me) {
  double* dev = reinterpret_cast<double*>(red_.p + RED_MISC);
  zc* lam_dev = red_.p + RED_MISC + 64;  // behind the 128 deviations
  HIP_CHECK(hipMemsetAsync(dev, 0, 128 * sizeof(double), st_));  // both sides' deviations: one clear
  ident_deviation_multi(st_, L, ml, dl, (long)ml * dl, dl, dev, lam_dev, ms, false);
  ident_deviation_multi(st_, R, mr, dr, (long)mr * dr, dr, dev + 64, lam_dev + 64, me, false);
  read_partials(RED_MISC, sizeof(IdentRecord) / sizeof(zc));
  cnt_.n_launch += 2;
  return *reinterpret_cast<const IdentRecord*>(h_red_.h + RED_MISC);
}

void MpoSite::EdgeCache::rebuild(hipStream_t st, const MpoSite& w, unsigned long long S, unsigned long long E,
                                 const std::vector<hzc>& lam, const std::vector<hzc>& mu) {
  const int ml = w.ml, d = w.d, mr = w.mr;
  bool same = valid && s == S && e == E;
  if (same) {  // the multiples are +-1 or weights that do not change along a run -- up to the rounding of the block's first
    // diagonal element (1 +- 2e-16 from sweep to sweep): compared to the tolerance of the identity test itself, so that the
    // reduced cores are not rebuilt on the host and uploaded again for every site of every sweep
    for (int c = 0; c < ml && same; ++c) if (((S >> c) & 1ull) && std::abs(this->lam[c] - lam[c]) > 1e-13) same = false;
    for (int t = 0; t < mr && same; ++t) if (((E >> t) & 1ull) && std::abs(this->mu[t] - mu[t]) > 1e-13) same = false;
  }
  if (std::getenv("MITDVP_EDGE_TRACE")) fprintf(stderr, "[mitdvp] edge cores of a site: %s\n", same ? "kept" : "rebuilt");
  if (same) return;
  const hzc* W = w.whost.data();
  std::vector<hzc> wl((size_t)d * ml * d, hzc(0, 0)), wr((size_t)d * d * mr, hzc(0, 0));
  valid = has_l = has_r = false;  // until the new cores are in place
  for (int c = 0; c < ml; ++c)
    for (int t = 0; t < mr; ++t) {
      if (!w.nzblk[(size_t)c * mr + t]) continue;
      const bool in_s = (S >> c) & 1ull;
      const hzc f = in_s ? lam[c] : mu[t];
      if (f == hzc(0.0, 0.0)) continue;  // a zero block of the environment: the term vanishes
      for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
          const hzc v = f * W[(((size_t)c * d + i) * d + j) * mr + t];
          if (in_s) wr[(size_t)i * d * mr + (size_t)j * mr + t] += v;
          else wl[(size_t)i * ml * d + (size_t)c * d + j] += v;
        }
      (in_s ? has_r : has_l) = true;
    }
  w_l.reserve(wl.size());
  w_r.reserve(wr.size());
  HIP_CHECK(hipMemcpyAsync(w_l.p, wl.data(), wl.size() * sizeof(zc), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(w_r.p, wr.data(), wr.size() * sizeof(zc), hipMemcpyHostToDevice, st));
  // the lists of the same cores (core_lists.h), for the strides choose_apply_forms folds them with; they live and die with
  // the cores.  (the blobs are whole 16-byte words; each copy is waited for: its host blob goes out of scope)
  auto upload_list = [&](DevBuf& b, const std::vector<unsigned char>& blob, size_t at = 0) {
    HIP_CHECK(hipMemcpyAsync(reinterpret_cast<unsigned char*>(b.p) + at, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
  };
  {
    const std::vector<unsigned char> ll = build_fold_list(wl.data(), d, ml, (long)ml * d, 1, d);
    const std::vector<unsigned char> lr = build_fold_list(wr.data(), d, mr, (long)d * mr, mr, 1);
    w_l_list.reserve(ll.size() / sizeof(zc));
    w_r_list.reserve(lr.size() / sizeof(zc));
    upload_list(w_l_list, ll);
    upload_list(w_r_list, lr);
  }
  w_lf.reserve(wl.size());
  w_rf.reserve(wr.size());
  lf_ok = zgemm_reduce_pack_core(st, w_l.p, (long)ml * d, d, ml * d, w_lf.p);
  rf_ok = zgemm_reduce_pack_core(st, w_r.p, (long)d * mr, d, d * mr, w_rf.p);
  // the cores of the structured environment update (env_update_fold), both directions: the blocks out of an identity
  // state summed with its multiple (all out states), and, per out state a general state feeds, those blocks unweighted
  for (int side = 0; side < 2; ++side) {
    const int mi = side == 0 ? ml : mr, mo = side == 0 ? mr : ml;
    const unsigned long long I = side == 0 ? S : E;
    const std::vector<hzc>& wt = side == 0 ? lam : mu;
    auto blk = [&](int in, int out) { return side == 0 ? (size_t)in * mr + out : (size_t)out * mr + in; };
    auto Wel = [&](int in, int i, int j, int out) {
      return side == 0 ? W[(((size_t)in * d + i) * d + j) * mr + out] : W[(((size_t)out * d + i) * d + j) * mr + in];
    };
    EnvFold& f = envf[side];
    f.t0.clear();
    for (int out = 0; out < mo; ++out)
      for (int in = 0; in < mi; ++in)
        if (!((I >> in) & 1ull) && w.nzblk[blk(in, out)]) { f.t0.push_back(out); break; }
    std::vector<hzc> ws((size_t)d * d * mo, hzc(0, 0)), wg(std::max<size_t>(f.t0.size(), 1) * d * mi * d, hzc(0, 0));
    for (int in = 0; in < mi; ++in) {
      if (!((I >> in) & 1ull)) continue;
      for (int out = 0; out < mo; ++out) {
        if (!w.nzblk[blk(in, out)]) continue;
        for (int i = 0; i < d; ++i)
          for (int j = 0; j < d; ++j) ws[((size_t)i * d + j) * mo + out] += wt[in] * Wel(in, i, j, out);
      }
    }
    for (size_t k = 0; k < f.t0.size(); ++k)
      for (int in = 0; in < mi; ++in) {
        if (((I >> in) & 1ull) || !w.nzblk[blk(in, f.t0[k])]) continue;
        for (int i = 0; i < d; ++i)
          for (int j = 0; j < d; ++j) wg[((k * d + i) * mi + in) * d + j] = Wel(in, i, j, f.t0[k]);
      }
    f.ws.reserve(ws.size());
    f.wg.reserve(wg.size());
    HIP_CHECK(hipMemcpyAsync(f.ws.p, ws.data(), ws.size() * sizeof(zc), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(f.wg.p, wg.data(), wg.size() * sizeof(zc), hipMemcpyHostToDevice, st));
    {
      const std::vector<unsigned char> gl = build_gram_list(ws.data(), d, mo, gram_list_tu(mo));
      f.ws_list.reserve(gl.size() / sizeof(zc));
      upload_list(f.ws_list, gl);
      // a dense wg[k] bounds every list: one stride for all k
      f.wg_list_stride = (fold_list_head(d) + (size_t)d * ((d + 3) / 4) * mi * sizeof(FoldEntry)) / sizeof(zc);
      f.wg_list.reserve(std::max<size_t>(f.t0.size(), 1) * f.wg_list_stride);
      for (size_t k = 0; k < f.t0.size(); ++k)
        upload_list(f.wg_list, build_fold_list(wg.data() + k * (size_t)d * mi * d, d, mi, (long)mi * d, 1, d),
                    k * f.wg_list_stride * sizeof(zc));
    }
    // whether the update may take the general states' operator from the solve's packed factors (EnvFold, engine.h).  The
    // directions differ because every block out of a state of S went to the R-side core wr above, whatever its out state
    f.reuse = false;
    std::vector<hzc> ws2;
    if (f.t0.size() == 1) {
      const int o = f.t0[0];
      const hzc wo = side == 0 ? mu[o] : lam[o];
      bool ok = (((side == 0 ? E : S) >> o) & 1ull) && wo != hzc(0.0, 0.0);
      if (side == 1)  // no other state of S may have put a block into GR (a zero multiple put none)
        for (int c = 0; c < ml && ok; ++c) {
          if (c == o || !((S >> c) & 1ull) || lam[c] == hzc(0.0, 0.0)) continue;
          for (int t = 0; t < mr && ok; ++t) if (w.nzblk[(size_t)c * mr + t]) ok = false;
        }
      if (ok) {
        f.reuse = true;
        f.reuse_alpha = hzc(1.0, 0.0) / wo;
        ws2 = ws;
        if (side == 1) for (int ij = 0; ij < d * d; ++ij) ws2[(size_t)ij * mo + o] = hzc(0.0, 0.0);
        f.ws_reuse.reserve(ws2.size());
        HIP_CHECK(hipMemcpyAsync(f.ws_reuse.p, ws2.data(), ws2.size() * sizeof(zc), hipMemcpyHostToDevice, st));
        const std::vector<unsigned char> gl2 = build_gram_list(ws2.data(), d, mo, gram_list_tu(mo));
        f.ws_reuse_list.reserve(gl2.size() / sizeof(zc));
        upload_list(f.ws_reuse_list, gl2);
      }
    }
    HIP_CHECK(hipStreamSynchronize(st));  // the host vectors go out of scope
  }
  HIP_CHECK(hipStreamSynchronize(st));
  s = S; e = E; this->lam = lam; this->mu = mu; valid = true;
}

// Which forms the applies of the local solve between these blocks take.  The three-stage chain may trim the identity
// blocks L[:, 0, :] and R[:, mr-1, :] (checked from D = 256 on, where one check per site buys 1 / M of stages S1 / S3 in
// every apply); the edge form needs the identity states of both bonds (all blocks checked: two launches, one copy).
ApplyPlan Engine::choose_apply_forms(const zc* Lb, const MpoSite& w, const zc* Rb, int dl, int d, int dr) {
  ApplyPlan plan;
  (void)take_env_checked();  // an earlier solve's sets describe other blocks
  int a0, a1;
  const bool sharded = shard_range(dl, a0, a1);
  const int ml = w.ml, mr = w.mr;
  // The folded variant of a side (heff_apply_edge), should the core turn out edge-structured.  The rule: a side's GEMM
  // shrinks by m / d, so it is folded when its MPO bond is wider than d; building the operator is d^2 m D^2 products and
  // one write of (d D)^2 elements per local solve, against (m - d) d D^3 products saved in every apply (measured:
  // profiles/fold_apply_ab.txt).  The operators live in the chain form's workspaces, which the edge form leaves idle and
  // nothing else writes during a local solve (Y_: GR; X_: GL, or psiT of an unfolded L side): (d D)^2 <= D M d D whenever
  // d <= M, so a side whose operator does not fit is not folded and no memory is ever allocated for one.
  const bool can_fold_r = fold_mode_ != 0 && !sharded && (fold_mode_ > 0 || mr > d) && (size_t)d * dr * d * dr <= Y_.n;
  const bool can_fold_l = fold_mode_ != 0 && !sharded && (fold_mode_ > 0 || ml > d) && (size_t)dl * d * dl * d <= X_.n;
  // (a folded side has no reducing epilogue: its group shapes need not be among those zgemm_reduce is built for)
  const bool edge_cand = edge_mode_ != 0 && trim_identity_ && !w.whost.empty() && !sharded && dl >= 32 && dr >= 32 &&
                         (can_fold_r || zgemm_reduce_ok(d, mr, d)) && (can_fold_l || zgemm_reduce_ok(ml, d, d)) && (long)d * dr < (1L << 20) &&
                         // the size rule: the epilogue streams the d x (d M) reduced core once per tile -- cheap beside a
                         // tile's K loop only while d M is small (measured: profiles/r04_edge_apply_ab.txt)
                         // round 5: with the 4 x 4 x 4 epilogue (no padded products at d M = 512) the form also wins where the
                         // W stage is a large share of the chain, i.e. at short bonds: C3 (D = 128) heff -9 %, C4 (D = 1024) +2 %
                         // (both sides folded: no epilogue at all, two plain GEMMs m / d times smaller than the chain's outer stages)
                         (edge_mode_ > 0 || (can_fold_r && can_fold_l) || ((long)d * std::max(ml, mr) <= 64 && (long)dl * dr <= 512L * 512L) ||
                          // (later in round 5: with the cores in fragment order and the unguarded epilogue the form is level with
                          // the chain at C4 too -- 0.02064 against 0.02058 sweeps/s, H_eff frac 0.899 against 0.875, a ninth of the
                          // chain's intermediate traffic -- so shapes that run that variant take it at any bond)
                          ((long)d * std::max(ml, mr) <= 512 && zgemm_reduce_b4_available(st_) != 0 &&
                           ((long)dl * dr <= 256L * 256L || (zgemm_reduce_full_ok(st_, d, mr, d) && zgemm_reduce_full_ok(st_, ml, d, d)))));
  const bool skip = edge_cand && w.edge.skip > 0;  // a core that failed the structure check recently: no look at all blocks
  if (skip) w.edge.skip -= 1;
  if (!edge_cand || skip) {  // the plain checks
    identity_blocks(trim_identity_ && dl >= 256 && ml > 1 ? Lb : nullptr, dl, ml,
                    trim_identity_ && dr >= 256 && mr > 1 ? Rb : nullptr, dr, mr, &plan.trim_l, &plan.trim_r);
    return plan;
  }
  // The identity states of a site do not change from sweep to sweep (they follow from the MPO's structure and the
  // canonical form): first only the blocks that were identity multiples last time are looked at (3 of 16 at C5); all of
  // them again when one of those has stopped being one, or when there is no previous answer.
  unsigned long long S = 0, E = 0;
  std::vector<hzc> lam(ml), mu(mr);
  for (int attempt = (w.edge.valid ? 0 : 1); attempt < 2; ++attempt) {
    const unsigned long long ms = attempt == 0 ? w.edge.s : ~0ull, me = attempt == 0 ? w.edge.e : ~0ull;
    const IdentRecord& h = identity_sets(Lb, ml, dl, ms, Rb, mr, dr, me);
    S = E = 0;
    for (int c = 0; c < ml; ++c) { lam[c] = h.lam[c]; if (((ms >> c) & 1ull) && h.dev[c] < 1e-13) S |= 1ull << c; }
    for (int t = 0; t < mr; ++t) { mu[t] = h.lam[64 + t]; if (((me >> t) & 1ull) && h.dev[64 + t] < 1e-13) E |= 1ull << t; }
    if (attempt == 0 && (S != w.edge.s || E != w.edge.e)) continue;  // something changed: look at every block
    break;
  }
  // the trimmed three-stage chain wants the plain identity in state 0 / mr - 1
  plan.trim_l = ml > 1 && (S & 1ull) && std::abs(lam[0] - 1.0) < 1e-13;
  plan.trim_r = mr > 1 && ((E >> (mr - 1)) & 1ull) && std::abs(mu[mr - 1] - 1.0) < 1e-13;
  for (int c = 0; c < ml; ++c)
    for (int t = 0; t < mr; ++t)
      if (w.nzblk[(size_t)c * mr + t] && !((S >> c) & 1ull) && !((E >> t) & 1ull)) {  // a block between general states
        w.edge.skip = 16;  // not an edge-structured core (or not between canonical blocks): ask again in a while
        return plan;
      }
  w.edge.rebuild(st_, w, S, E, lam, mu);
  plan.edge = true;
  // S / E describe exactly these two blocks of this site: the next environment update may rely on them (env_fold_ok)
  env_chk_ = EnvChecked{&w, {Lb, Rb}, {dl, dr}};
  plan.fold_r = w.edge.has_r && can_fold_r;
  plan.fold_l = w.edge.has_l && can_fold_l;
  if (plan.fold_r || plan.fold_l) {  // once per local solve, on the stream, no synchronisation
    timer_begin(11);
    if (plan.fold_r)
      fold_env_core(st_, Rb, w.edge.w_r.p, Y_.p, dr, mr, d, (long)d * mr, mr, 1, (long)dr * d * dr, (long)d * dr, dr, 1,
                    core_lists_ ? w.edge.w_r_list.p : nullptr);
    if (plan.fold_l)
      fold_env_core(st_, Lb, w.edge.w_l.p, X_.p, dl, ml, d, (long)ml * d, 1, d, (long)dl * d, (long)d * dl * d, 1, d,
                    core_lists_ ? w.edge.w_l_list.p : nullptr);
    // Strassen levels over a folded side.  One level: its rows, columns and contraction length even, and (the rule) the
    // half-size products still at least one whole round of 64 x 64 tiles on the device -- STRASSEN_MIN_TILES per product,
    // measured: profiles/fold_strassen_ab.txt.  Two levels: all three divisible by 4 and the same of the quarter-size
    // products.  The operator's seven or 49 factors are packed here, once per local solve, from GL / GR, which stay where
    // they are; both levels use the same table (a level-1 factor of GR is an untransposed sum of GR's quadrants and stands
    // for the transposed B factor just as GR does), and a side with two levels never writes its seven.  Buffers that cannot
    // be had drop the side a level.
    const size_t quarter = (size_t)dl * d * dr / 4;
    auto tiles_fill = [](long pm, long pn) { return ((pm + 63) / 64) * ((pn + 63) / 64) >= STRASSEN_MIN_TILES; };
    auto level_of = [&](long rows, long cols, long klen) {  // the levels the sizes and the switch allow
      if (strassen_mode_ == 0 || rows % 2 || cols % 2 || klen % 2) return 0;
      const bool four = rows % 4 == 0 && cols % 4 == 0 && klen % 4 == 0;
      if (strassen_mode_ > 0) return strassen_mode_ >= 2 && four ? 2 : 1;
      if (four && tiles_fill(rows / 4, cols / 4)) return 2;
      return tiles_fill(rows / 2, cols / 2) ? 1 : 0;
    };
    auto pack = [&](const zc* op, long n, DevBuf& f, int which, int want) {  // the n x n operator's factors, 49 or seven, in f
      const long h = n / 2, q = n / 4;
      // (the contents of str_v_ / str_m_ are per-apply scratch: growing them here loses nothing)
      // (a fused side -- the L side, strassen_side -- has no level-1 area)
      const size_t two = (strassen_fuse_ && which == STRASSEN_A ? 0 : 7 * quarter) + 49 * (quarter / 4);
      if (want == 2 && try_reserve(f, 49 * (size_t)q * q) && try_reserve(str_v_, two) && try_reserve(str_m_, two)) {
        strassen_operands2(st_, op, n, q, q, f.p, which);  // the 49 straight from the operator's 16 blocks
        cnt_.n_launch += 1;
        return 2;
      }
      if (want == 0 || !try_reserve(f, 7 * (size_t)h * h) || !try_reserve(str_v_, 7 * quarter) || !try_reserve(str_m_, 7 * quarter))
        return 0;
      strassen_operands(st_, op, n, h, h, f.p, which);
      cnt_.n_launch += 1;
      return 1;
    };
    if (plan.fold_r) plan.strassen_r = pack(Y_.p, (long)d * dr, str_r_, STRASSEN_BT, level_of(dl, (long)d * dr, (long)d * dr));
    if (plan.fold_l) plan.strassen_l = pack(X_.p, (long)dl * d, str_l_, STRASSEN_A, level_of((long)dl * d, dr, (long)dl * d));
    env_chk_.lvl[0] = plan.strassen_l;  // what str_l_ / str_r_ hold of these blocks until the next call of this function
    env_chk_.lvl[1] = plan.strassen_r;
    timer_end();
    cnt_.n_launch += (plan.fold_r ? 1 : 0) + (plan.fold_l ? 1 : 0);
    if (std::getenv("MITDVP_EDGE_TRACE"))
      fprintf(stderr, "[mitdvp] folded sides of a site: R %s, L %s\n",
              plan.strassen_r == 2 ? "49 quarter-size products" : plan.strassen_r ? "seven half-size products" : plan.fold_r ? "plain product" : "not folded",
              plan.strassen_l == 2 ? "49 quarter-size products" : plan.strassen_l ? "seven half-size products" : plan.fold_l ? "plain product" : "not folded");
  }
  return plan;
}

void Engine::heff_apply(const zc* L, const MpoSite& w, const zc* R, const zc* psi, zc* out, int dl, int d, int dr,
                        hzc shift, const ApplyPlan& plan) {
  SmallChain sc;
  if (small_ok() && chain_heff(sc, L, w, R, dl, d, dr, false)) {  // one launch, X / Y in LDS
    timer_begin(10);
    small_apply(st_, ss_, sc, psi, out, ss_partials(sc), make_double2(shift.real(), shift.imag()), shift != hzc(0.0, 0.0));
    timer_end();
    cnt_.n_launch += 1;
    cnt_.n_heff += 1;
    cnt_.heff_flops += 8.0 * ((double)dl * dl * w.ml * d * dr + (double)dl * dr * w.ml * w.mr * d * d + (double)dl * dr * dr * w.mr * d);
    return;
  }
  if (plan.edge) heff_apply_edge(L, w, R, psi, out, dl, d, dr, plan);
  else heff_apply_rect(L, w, R, psi, out, dl, dl, d, dr, dr, plan);
  if (shift != hzc(0.0, 0.0))
    vec_axpby(st_, out, psi, (long)dl * d * dr, make_double2(shift.real(), shift.imag()), make_double2(1.0, 0.0));
}

// L (dlo, m, dli), R (dro, m, dri), sig (dli, dri) -> out (dlo, dro)
void Engine::keff_apply_rect(const zc* L, const zc* R, const zc* sig, zc* out, int dlo, int dli, int dro, int dri,
                             int m) {
  int a0, a1;
  const bool sharded = shard_range(dlo, a0, a1);
  const int na = a1 - a0;
  timer_begin(2);
  {  // X[(a,c)][s] = L[(a,c)][b] sig[b][s]
    ZgemmDesc g = zgemm_desc(L + (size_t)a0 * m * dli, sig, X_.p, na * m, dri, dli);
    zgemm(st_, g);
  }
  {  // out[a][r] = X[a][(c,s)] R[r][(c,s)]
    ZgemmDesc g = zgemm_desc(X_.p, R, out + (size_t)a0 * dro, na, dro, m * dri);
    g.transB = 1; g.ldb = (long)m * dri;
    zgemm(st_, g);
  }
  timer_end();
  if (sharded) collective(COLL_ALLGATHER, out, (size_t)dlo * dro);
  cnt_.n_launch += 2;
  cnt_.n_keff += 1;
  cnt_.keff_flops += 8.0 * ((double)na * dli * m * dri + (double)na * dro * dri * m);
}

// Which MPO-bond states of the two blocks of a bond are multiples of the identity (one look at all blocks: two launches,
// one copy, one synchronisation per bond exponential), the compact copies of the blocks that are not, and the lists of
// scaled copies.  nullptr when nothing, or too little, can be skipped; else the form for the applies of this bond solve.
const Engine::KeffCompact* Engine::keff_prepare(const zc* L, const zc* R, int d1, int d2, int m) {
  int a0, a1;
  if (!keff_ident_ || !trim_identity_ || d1 != d2 || d1 < 256 || m < 2 || m > 64 || shard_range(d1, a0, a1)) return nullptr;
  const IdentRecord& h = identity_sets(L, m, d1, ~0ull, R, m, d2, ~0ull);
  BlockList gl{}, gr{};  // blocks gathered into Lc ([E \ S | general]) and Rc ([general | S \ E])
  KeffCompact& k = kc_;
  k.fillS.n = k.accE.n = 0;
  hzc both(0.0, 0.0);
  std::vector<int> onlyE, gen, onlyS;
  for (int c = 0; c < m; ++c) {
    const bool inS = h.dev[c] < 1e-13, inE = h.dev[64 + c] < 1e-13;
    if (inS && inE) both += h.lam[c] * h.lam[64 + c];
    else if (inS) onlyS.push_back(c);
    else if (inE) onlyE.push_back(c);
    else gen.push_back(c);
  }
  const int skipped = 2 * (m - (int)gen.size()) - (int)onlyS.size() - (int)onlyE.size();  // block products saved, of 2 m
  if (skipped * 16 < 2 * m) return nullptr;  // less than 1 / 16 of the apply: not worth the extra launches
  k.nE = (int)onlyE.size(); k.nG = (int)gen.size(); k.nS = (int)onlyS.size();
  k.n1 = k.nE + k.nG;
  for (int c : onlyE) gl.idx[gl.n++] = c;
  for (int c : gen) { gl.idx[gl.n++] = c; gr.idx[gr.n++] = c; }
  for (int c : onlyS) gr.idx[gr.n++] = c;
  for (int q = 0; q < k.nS; ++q) { const hzc l = h.lam[onlyS[q]]; k.fillS.f[k.fillS.n++] = make_double2(l.real(), l.imag()); }
  for (int q = 0; q < k.nE; ++q) {
    const hzc mu = h.lam[64 + onlyE[q]];
    k.accE.idx[k.accE.n] = q;  // position of the block in X's row layout
    k.accE.f[k.accE.n++] = make_double2(mu.real(), mu.imag());
  }
  k.both = make_double2(both.real(), both.imag());
  k.m = m;
  k.Lc.reserve((size_t)d1 * std::max(k.n1, 1) * d1);
  k.Rc.reserve((size_t)d2 * std::max(k.nG + k.nS, 1) * d2);
  gather_blocks(st_, k.Lc.p, k.n1, L, m, d1, d1, gl);
  gather_blocks(st_, k.Rc.p, k.nG + k.nS, R, m, d2, d2, gr);
  cnt_.n_launch += 2;
  return &k;
}

void Engine::keff_apply_compact(const KeffCompact& k, const zc* sig, zc* out, int d1, int d2, hzc shift) {
  const int nx = k.nE + k.nG + k.nS;
  const long ldx = (long)nx * d2;
  timer_begin(2);
  if (k.n1 > 0) {  // X[a][ci][s] = Lc[(a, ci)][b] sig[b][s], ci over [E \ S | general]
    ZgemmDesc g = zgemm_desc(k.Lc.p, sig, X_.p, d1 * k.n1, d2, d1);
    g.rowmap_p = k.n1; g.rowmap_s1 = d2; g.rowmap_s2 = ldx; g.rowmap_r0 = 0;
    zgemm(st_, g);
    cnt_.n_launch += 1;
  }
  fill_scaled_blocks(st_, X_.p, ldx, k.n1, sig, d1, d2, k.fillS);  // X[a][n1 + q][:] = lam_q sig[a][:]
  if (k.fillS.n) cnt_.n_launch += 1;
  const int n2 = k.nG + k.nS;
  if (n2 > 0) {  // out[a][r] = X[a][(cj, s)] Rc[r][(cj, s)], cj over [general | S \ E]
    ZgemmDesc g = zgemm_desc(X_.p + (size_t)k.nE * d2, k.Rc.p, out, d1, d2, n2 * d2);
    g.lda = ldx; g.transB = 1; g.ldb = (long)n2 * d2;
    zgemm(st_, g);
    cnt_.n_launch += 1;
  } else {
    HIP_CHECK(hipMemsetAsync(out, 0, (size_t)d1 * d2 * sizeof(zc), st_));
  }
  const hzc tot = hzc(k.both.x, k.both.y) + shift;  // the scalar term of the operator rides on the same pass
  accum_scaled_blocks(st_, out, X_.p, ldx, sig, d1, d2, k.accE, make_double2(tot.real(), tot.imag()));
  cnt_.n_launch += 1;
  timer_end();
  cnt_.n_keff += 1;
  // (algorithmic count: all m blocks, as SURVEY 8d F_K)
  cnt_.keff_flops += 8.0 * ((double)d1 * d1 * k.m * d2 + (double)d1 * d2 * d2 * k.m);
}

void Engine::keff_apply(const zc* L, const zc* R, const zc* sig, zc* out, int d1, int d2, int m, hzc shift,
                        const KeffCompact* kc) {
  if (kc) { keff_apply_compact(*kc, sig, out, d1, d2, shift); return; }
  SmallChain sc;
  if (small_ok() && chain_keff(sc, L, R, d1, d2, m, false)) {
    timer_begin(2);
    small_apply(st_, ss_, sc, sig, out, ss_partials(sc), make_double2(shift.real(), shift.imag()), shift != hzc(0.0, 0.0));
    timer_end();
    cnt_.n_launch += 1;
    cnt_.n_keff += 1;
    cnt_.keff_flops += 8.0 * ((double)d1 * d1 * m * d2 + (double)d1 * d2 * d2 * m);
    return;
  }
  keff_apply_rect(L, R, sig, out, d1, d1, d2, d2, m);
  if (shift != hzc(0.0, 0.0))
    vec_axpby(st_, out, sig, (long)d1 * d2, make_double2(shift.real(), shift.imag()), make_double2(1.0, 0.0));
}

// env_in (dbi, min, dki), ket tensor Tk (dki, d, dko), bra tensor Tb (dbi, d, dbo),
// W2 ((d*mout) x (min*d)) -> env_out (dbo, mout, dko).  Tb != Tk is the adaptive-rank
// "bra" block (superblock_states_bra, _mps_cls.py:1950-1963).
void Engine::env_update_rect(const zc* env_in, const zc* Tk, const zc* Tb, const zc* w2, zc* env_out, int dbi, int dki,
                             int min_, int d, int dbo, int dko, int mout, const MpoSite* sp, int sp_side) {
  int m0, m1;
  const bool sharded = shard_range(dbi, m0, m1);
  const int nm = m1 - m0;
  timer_begin(1);
  {  // X[(m,p)][(s,j)] = env[(m,p)][n] Tk[n][(s,j)]
    ZgemmDesc g = zgemm_desc(env_in + (size_t)m0 * min_ * dki, Tk, X_.p, nm * min_, d * dko, dki);
    zgemm(st_, g);
  }
  // Y_m[(r,q)][j] = W2[(r,q)][(p,s)] X_m[(p,s)][j]
  (void)w_stage(sp, sp_side, w2, d, mout, min_, dko, nm);
  {  // env'[i][(q,j)] = conj(Tb)[(m,r)][i] Y[(m,r)][(q,j)]   (sum over this rank's m)
    ZgemmDesc g = zgemm_desc(Tb + (size_t)m0 * d * dbo, Y_.p, env_out, dbo, mout * dko, nm * d);
    g.transA = 1; g.conjA = 1; g.lda = dbo;
    zgemm(st_, g);
  }
  timer_end();
  if (sharded) collective(COLL_ALLREDUCE, env_out, (size_t)dbo * mout * dko);
  cnt_.n_launch += 3;
  cnt_.n_env += 1;
  cnt_.env_flops += 8.0 * ((double)nm * dki * min_ * d * dko + (double)nm * dko * min_ * mout * d * d +
                           (double)nm * dbo * dko * mout * d);
}

// The structured update.  With I the states of the consumed block's MPO bond whose blocks env_in[:, c, :] are multiples
// lam_c of the identity (found by choose_apply_forms for this very block), the sum over c splits:
//   c in I:      env_in drops out.  G[(i,a')][(j,r)] = sum_a conj(T[a,i,a']) T[a,j,r]  (the site tensor's Gram matrix, Hermitian:
//                its upper block half by block rows, d (d + 1) / 2 D^3 products, the lower half mirrored) and env_out[a',t,r] = sum_{i,j} ws[i,j,t] G[(i,a')][(j,r)] for every t
//                (gram_env_core: d^2 M D^2 products);
//   c not in I:  only the few out states t0 a general state feeds (one per summand of a finite-state-machine MPO).  With
//                GL_t0[(a,i)][(b,j)] = sum_{c not in I} W[c,i,j,t0] env_in[a,c,b]  (fold_env_core),
//                env_out[:, t0, :] += T^H (GL_t0 T): d^2 D^3 + d D^3 products.
// (d (d + 1) / 2 + |t0| d^2) D^3 + |t0| d D^3 products against the chain's 2 M d D^3.  The Gram matrix and then GL_t0 T live in Y_,
// GL_t0 in X_: the chain's own workspaces, (d D)^2 <= D M d D whenever d <= M; nothing is allocated.
bool Engine::env_fold_ok(const zc* env_in, int din, int min_, int d, int dout, int mout, const MpoSite* sp, int sp_side,
                         int* reuse_level) {
  const EnvChecked chk = take_env_checked();  // whatever this update does, the sets have had their one use
  *reuse_level = 0;
  int a0, a1;
  if (fold_env_mode_ == 0 || !sp || adaptive_ || shard_range(din, a0, a1)) return false;
  if (chk.w != sp || chk.blk[sp_side] != env_in || chk.n[sp_side] != din || !sp->edge.valid || sp->d != d) return false;
  if (min_ != (sp_side == 0 ? sp->ml : sp->mr) || mout != (sp_side == 0 ? sp->mr : sp->ml)) return false;
  if (min_ > 64 || mout > 64 || d > 64 || din > 65535 || dout > 65535) return false;  // the two kernels' ranges
  const MpoSite::EnvFold& f = sp->edge.envf[sp_side];
  const double nt = (double)f.t0.size();
  if ((size_t)d * dout * d * dout > Y_.n || (size_t)din * d * dout > Y_.n || (nt > 0 && (size_t)din * d * din * d > X_.n)) return false;
  // the solve behind this record packed the consumed side's operator (the record matches block, width and site): the one
  // general out state's operator is that one up to a factor
  if (env_reuse_ && f.reuse) *reuse_level = chk.lvl[sp_side];
  if (fold_env_mode_ > 0) return true;
  // the rule: the consumed side's MPO bond wider than d (as for the folded apply), and at most three quarters of the
  // chain's products left (one general out state always passes; a direct sum with several is taken while it pays)
  const double fresh = (double)d * d * dout * dout * din + nt * ((double)d * d * din * din * dout + (double)d * din * dout * dout);
  const double chain = (double)min_ * d * din * din * dout + (double)mout * d * din * dout * dout;
  return min_ > d && 4.0 * fresh <= 3.0 * chain;
}

// The structured update itself (the formulas: above env_fold_ok).
// reuse_level >= 1 (one t0; EnvFold::reuse and the record of the solve agree): the operator of the general states is the one
// the solve packed into str_l_ / str_r_, up to the factor 1 / reuse_alpha.  fold_env_core is skipped and the product with
// it runs as the solve's applies do (strassen_side; str_v_ / str_m_ are idle between applies), into Y_:
//   ->  Z[(a,i)][r] = GL T, closed by T^H Z as below;
//   <-  the R-side product takes the unmirrored tensor B[a][(j,s)] (T_plain; T is its mirror image) and gives
//       Z'[a][(i,r)] = B GR^T; block c0 += conj(B)[a'][(i,r)] Z'[a][(i,r)], a conjugated, untransposed A against a transposed B.
//       GR also holds the identity states' blocks out of c0, so the Gram core ran without them (ws_reuse).
void Engine::env_update_fold(const zc* env_in, const zc* T, zc* env_out, int din, int min_, int d, int dout, int mout,
                             const MpoSite::EnvFold& f, int sp_side, int reuse_level, const zc* T_plain) {
  const bool reuse = reuse_level >= 1;
  timer_begin(1);
  // G[(i,a')][(j,r)] = conj(T)[a][(i,a')] T[a][(j,r)] is Hermitian: block row i of the product is formed from its diagonal
  // block on (j >= i: d (d + 1) / 2 of the d^2 blocks, the diagonal ones whole), the blocks below the diagonal are the
  // conjugate transposes of those above (gram_mirror_lower: one read and one write of that half)
  const long ldg = (long)d * dout;
  for (int i = 0; i < d; ++i) {
    ZgemmDesc g = zgemm_desc(T + (size_t)i * dout, T + (size_t)i * dout, Y_.p + (size_t)i * dout * ldg + (size_t)i * dout, dout,
                             (d - i) * dout, din);
    g.transA = 1; g.conjA = 1; g.lda = ldg; g.ldb = ldg; g.ldc = ldg;
    zgemm(st_, g);
  }
  gram_mirror_lower(st_, Y_.p, dout, d);
  gram_env_core(st_, Y_.p, reuse ? f.ws_reuse.p : f.ws.p, env_out, dout, mout, d,
                !core_lists_ ? nullptr : reuse ? f.ws_reuse_list.p : f.ws_list.p);
  const zc alpha = make_double2(f.reuse_alpha.real(), f.reuse_alpha.imag());
  if (reuse && sp_side == 0) {
    strassen_side(str_l_.p, true, T, dout, Y_.p, (long)din * d / 2, dout / 2, (long)din * d / 2, false, reuse_level);
    ZgemmDesc h = zgemm_desc(T, Y_.p, env_out + (size_t)f.t0[0] * dout, dout, dout, din * d);
    h.transA = 1; h.conjA = 1; h.lda = dout; h.ldc = (long)mout * dout; h.alpha = alpha; h.beta = make_double2(1.0, 0.0);
    zgemm(st_, h);
  } else if (reuse) {
    strassen_side(str_r_.p, false, T_plain, (long)d * din, Y_.p, dout / 2, (long)d * din / 2, (long)d * din / 2, false, reuse_level);
    ZgemmDesc h = zgemm_desc(T_plain, Y_.p, env_out + (size_t)f.t0[0] * dout, dout, dout, d * din);
    h.conjA = 1; h.transB = 1; h.ldb = (long)d * din; h.ldc = (long)mout * dout; h.alpha = alpha; h.beta = make_double2(1.0, 0.0);
    zgemm(st_, h);
  }
  for (size_t k = 0; !reuse && k < f.t0.size(); ++k) {
    // GL[(a,i)][(b,j)] (in X_), Z[(a,i)][r] = GL T[(b,j)][r] (in Y_: the Gram matrix has been consumed), block t0 += T^H Z
    fold_env_core(st_, env_in, f.wg.p + k * (size_t)d * min_ * d, X_.p, din, min_, d, (long)min_ * d, 1, d, (long)din * d,
                  (long)d * din * d, 1, d, core_lists_ ? f.wg_list.p + k * f.wg_list_stride : nullptr);
    ZgemmDesc g = zgemm_desc(X_.p, T, Y_.p, din * d, dout, din * d);
    zgemm(st_, g);
    ZgemmDesc h = zgemm_desc(T, Y_.p, env_out + (size_t)f.t0[k] * dout, dout, dout, din * d);
    h.transA = 1; h.conjA = 1; h.lda = dout; h.ldc = (long)mout * dout; h.beta = make_double2(1.0, 0.0);
    zgemm(st_, h);
  }
  timer_end();
  // (strassen_side counts its own launches: the packing, the products and the combining)
  cnt_.n_launch += d + (d > 1 ? 1 : 0) + 1 + (reuse ? 1 : 3 * (long long)f.t0.size());
  cnt_.n_env += 1;
  cnt_.n_env_fold += 1;
  if (reuse) cnt_.n_env_reuse += 1;
  // (algorithmic count, as heff_flops: the chain's)
  cnt_.env_flops += 8.0 * ((double)din * din * min_ * d * dout + (double)din * dout * min_ * mout * d * d +
                           (double)din * dout * dout * mout * d);
}

void Engine::env_update(const zc* env_in, const zc* T, const zc* w2, zc* env_out, int din, int min_, int d, int dout,
                        int mout, const zc* w2e, const MpoSite* sp, int sp_side, const zc* T_plain) {
  SmallChain sc;
  if (w2e && small_ok() && chain_env(sc, T, w2e, din, min_, d, dout, mout)) {
    timer_begin(1);
    small_apply(st_, ss_, sc, env_in, env_out, ss_partials(sc), make_double2(0.0, 0.0), false);
    timer_end();
    cnt_.n_launch += 1;
    cnt_.n_env += 1;
    cnt_.env_flops += 8.0 * ((double)din * din * min_ * d * dout + (double)din * dout * min_ * mout * d * d +
                             (double)din * dout * dout * mout * d);
    (void)take_env_checked();
    return;
  }
  int reuse_level = 0;
  if (env_fold_ok(env_in, din, min_, d, dout, mout, sp, sp_side, &reuse_level)) {
    if (sp_side == 1 && !T_plain) reuse_level = 0;
    env_update_fold(env_in, T, env_out, din, min_, d, dout, mout, sp->edge.envf[sp_side], sp_side, reuse_level, T_plain);
    return;
  }
  env_update_rect(env_in, T, T, w2, env_out, din, din, min_, d, dout, dout, mout, sp, sp_side);
}

// Block L[:, 0, :] / R[:, mr-1, :] == the identity to 1e-13 (the tensors on that side are canonical, to rounding):
// both checks of a site with ONE host synchronisation (two small reduction launches, one 16-byte copy); a null block
// is not checked
void Engine::identity_blocks(const zc* L, int dl, int ml, const zc* R, int dr, int mr, bool* left, bool* right) {
  double* dev = reinterpret_cast<double*>(red_.p + RED_MISC);
  const double* h = reinterpret_cast<const double*>(h_red_.h + RED_MISC);
  if (L) ident_deviation(st_, L, (long)ml * dl, dl, dev);
  if (R) ident_deviation(st_, R + (size_t)(mr - 1) * dr, (long)mr * dr, dr, dev + 1);
  if (L || R) read_partials(RED_MISC, 1);
  *left = L && h[0] < 1e-13;
  *right = R && h[1] < 1e-13;
}

}  // namespace mitdvp
