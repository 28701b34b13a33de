// policy_act_rows.h — argument block and launcher of k_policy_act_rows (csrc/policy_act_rows.hip): N observation rows
// through a net's row-major master weights, 16 rows per workgroup; obs / out are host-mapped.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace oprl {

constexpr int kActRowsMax = 256;     // OPRL_ACT_ROWS_MAX
constexpr int kActRowsTile = 16;     // rows per workgroup (one MFMA tile)
constexpr int kActRowsWidth = 512;   // widest layer (= kPolicyActMaxWidth): the LDS row of a tile

struct PolicyActRowsArgs {
  int n_layers;
  int dims[kMaxLayers + 1];
  const float* w[kMaxLayers];
  const float* b[kMaxLayers];
  const float* obs;                    // [n_rows][dims[0]]
  unsigned long long* out;             // [n_rows][dims[n_layers]] {ticket, value}
  int n_rows;
  unsigned ticket_value;
};
hipError_t launch_policy_act_rows(const PolicyActRowsArgs& a, hipStream_t st);

}  // namespace oprl
