// engine_batch.h -- batched trajectories (engine_batch.hip): B borrowed engines stepped by one launch per half-sweep.
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
  void sweep(double dt, bool forward, int* statuses);
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

  static std::vector<BatchShape> shapes_of(Engine& e);
  void validate();
  void prepare(bool forward);
  void launch(double dt, bool forward);
  void finish(bool ends_forward, int half_sweeps, int* statuses);
};

}  // namespace mitdvp
