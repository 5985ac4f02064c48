// Throw-away C shim over csrc/core_lists.h for tests/test_core_lists_host.py (compiled with g++, no HIP).
#include "../../pytdscf_amd/csrc/core_lists.h"

using namespace mitdvp;

static size_t give(const std::vector<unsigned char>& blob, unsigned char* out, size_t cap) {
  if (out && cap >= blob.size()) std::memcpy(out, blob.data(), blob.size());
  return blob.size();
}

extern "C" {
// the blob's size; it is copied to out when cap is large enough
size_t cl_fold_list(const double* w, int d, int m, long wi, long wj, long wm, unsigned char* out, size_t cap) {
  return give(build_fold_list(reinterpret_cast<const std::complex<double>*>(w), d, m, wi, wj, wm), out, cap);
}
size_t cl_gram_list(const double* ws, int d, int m, int tu, unsigned char* out, size_t cap) {
  return give(build_gram_list(reinterpret_cast<const std::complex<double>*>(ws), d, m, tu), out, cap);
}
size_t cl_fold_head(int d) { return fold_list_head(d); }
size_t cl_gram_head(int d, int tu) { return gram_list_head(d, tu); }
size_t cl_gram_records(int d, int tu) { return gram_list_records(d, tu); }
int cl_gram_tu(int m) { return gram_list_tu(m); }
int cl_fold_entry_bytes() { return (int)sizeof(FoldEntry); }
}
