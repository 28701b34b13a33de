// per_seed.h — the argument block of k_td_weighted_seed (per_seed.hip): the importance-weighted MSE-TD seed of a
// critic step that trains from prioritized replay ("Training from it").
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace oprl {

struct TdSeedArgs {
  SeedArgs s;                    // the target operands exactly as SEED_MSE_TD takes them: p0, p1, p2, log_alpha / alpha_const, r, d, gamma, cval = 1/B, y_out / q_out (critic 0)
  const float* q; long q_stride; // the online critics' outputs q[j * q_stride + b] (the forward-only launches' `out`)
  const float* w;                // importance weights [B]
  float* seed; long seed_stride; // out: seed[j * seed_stride + b] = ((2 (q_j - y)) cval) w_b — what SEED_PTR reads with ld0 = 1
  float* td_abs;                 // out: [B] (sum_j |q_j - y|) / nc
  float* partials;               // out: [nc][n_slices][4] per-slice sums of w (q - y)^2, q, y (launch_reduce_partials' layout)
  int nc, B, n_slices;
};

hipError_t launch_td_weighted_seed(const TdSeedArgs& a, hipStream_t st);

}  // namespace oprl
