// capi_internal.h -- the opaque handle of include/mitdvp.h as the translation units of the C surface see it
// (capi.hip, shard.hip).
#pragma once
#include <memory>
#include <string>

#include <vector>

#include "engine.h"

struct mitdvp_engine {
  std::unique_ptr<mitdvp::Engine> e;
  std::string err;
  int device = 0;
};

namespace mitdvp { class Batch; }
struct mitdvp_batch {
  std::unique_ptr<mitdvp::Batch> b;
  std::vector<mitdvp_engine*> hs;  // borrowed: the replicas' handles (their err strings receive per-replica messages)
  mitdvp_batch();
  ~mitdvp_batch();
};
