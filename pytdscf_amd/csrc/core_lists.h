// The coefficient lists of the two core contractions (vecops.hip: k_fold_env_core_list, k_gram_env_core_list): plain C++,
// no HIP, so that the host test compiles it alone (tests/test_core_lists_host.py).  A reduced MPO core is the same for
// every workgroup of a launch; the lists hold, once per upload of the core (MpoSite::EdgeCache::rebuild), exactly the
// coefficients the dense kernels would pick out of it, in the order they use them, so that the kernels fetch them with
// wave-uniform addresses.  Both blobs are whole multiples of 16 bytes.
#pragma once
#include <complex>
#include <cstdint>
#include <cstring>
#include <vector>

namespace mitdvp {

// --- fold list -------------------------------------------------------------------------------------------------------
// Items (i, j-group of four), item = i * njb + j0 / 4, njb = (d + 3) / 4.  CSR: int32 off[d * njb + 1], padded to 16 bytes,
// then the entries.  Entry = bond state c and the four coefficients w[i][min(j0 + u, d - 1)][c], u = 0..3, for ascending c,
// for exactly the c at which one of the four is non-zero (the dense kernel's test).
struct FoldEntry {
  int32_t c;
  int32_t pad[3];
  double f[8];  // (re, im) of u = 0..3
};
static_assert(sizeof(FoldEntry) == 80, "FoldEntry is five 16-byte words");

inline size_t fold_list_head(int d) {  // bytes before the first entry
  const size_t nitem = (size_t)d * ((d + 3) / 4);
  return ((nitem + 1) * sizeof(int32_t) + 15) / 16 * 16;
}

inline std::vector<unsigned char> build_fold_list(const std::complex<double>* w, int d, int m, long wi, long wj, long wm) {
  const int njb = (d + 3) / 4, nitem = d * njb;
  std::vector<int32_t> off(nitem + 1, 0);
  std::vector<FoldEntry> ent;
  for (int item = 0; item < nitem; ++item) {
    const int i = item / njb, j0 = (item % njb) * 4;
    for (int c = 0; c < m; ++c) {
      FoldEntry e;
      std::memset(&e, 0, sizeof e);
      e.c = c;
      bool any = false;
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u < d - 1 ? j0 + u : d - 1;
        const std::complex<double> v = w[i * wi + j * wj + c * wm];
        e.f[2 * u] = v.real();
        e.f[2 * u + 1] = v.imag();
        any = any || v.real() != 0.0 || v.imag() != 0.0;
      }
      if (any) ent.push_back(e);
    }
    off[item + 1] = (int32_t)ent.size();
  }
  const size_t head = fold_list_head(d);
  std::vector<unsigned char> blob(head + ent.size() * sizeof(FoldEntry), 0);
  std::memcpy(blob.data(), off.data(), off.size() * sizeof(int32_t));
  if (!ent.empty()) std::memcpy(blob.data() + head, ent.data(), ent.size() * sizeof(FoldEntry));
  return blob;
}

// --- Gram list -------------------------------------------------------------------------------------------------------
// For the instantiation TU the launcher takes at this m (gram_list_tu), UC = min(TU, 8) blocks at a time: one record per
// (i, wave v, j, chunk ch), record = ((i * 4 + v) * d + j) * (TU / UC) + ch (a wave walks j: its records are contiguous), of the coefficients ws[i][j][t],
// t = v + 4 * (UC * ch + u), u = 0..UC-1 (zero where t >= m), and a mask whose bit u says that coefficient u is non-zero.
// Layout: uint32 mask[records], padded to 16 bytes, then records x UC coefficients (re, im).
inline int gram_list_tu(int m) { return m <= 16 ? 4 : m <= 32 ? 8 : 16; }
inline int gram_list_uc(int tu) { return tu < 8 ? tu : 8; }
inline size_t gram_list_records(int d, int tu) { return (size_t)d * d * 4 * (tu / gram_list_uc(tu)); }
inline size_t gram_list_head(int d, int tu) { return (gram_list_records(d, tu) * sizeof(uint32_t) + 15) / 16 * 16; }

inline std::vector<unsigned char> build_gram_list(const std::complex<double>* ws, int d, int m, int tu) {
  const int uc = gram_list_uc(tu), nch = tu / uc;
  const size_t nrec = gram_list_records(d, tu), head = gram_list_head(d, tu);
  std::vector<unsigned char> blob(head + nrec * uc * 2 * sizeof(double), 0);
  uint32_t* mask = reinterpret_cast<uint32_t*>(blob.data());
  double* cf = reinterpret_cast<double*>(blob.data() + head);
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j)
      for (int v = 0; v < 4; ++v)
        for (int ch = 0; ch < nch; ++ch) {
          const size_t rec = (((size_t)i * 4 + v) * d + j) * nch + ch;
          uint32_t mk = 0;
          for (int u = 0; u < uc; ++u) {
            const int t = v + 4 * (uc * ch + u);
            const std::complex<double> x = t < m ? ws[((size_t)i * d + j) * m + t] : std::complex<double>(0.0, 0.0);
            cf[(rec * uc + u) * 2] = x.real();
            cf[(rec * uc + u) * 2 + 1] = x.imag();
            if (x.real() != 0.0 || x.imag() != 0.0) mk |= 1u << u;
          }
          mask[rec] = mk;
        }
  return blob;
}

}  // namespace mitdvp
