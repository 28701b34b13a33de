// iql_seed.h — the argument blocks of k_iql_value_seed / k_iql_actor_seed (iql_seed.hip): the implicit-Q-learning mode of a
// TD3 learner (Kostrikov et al. 2021).  The first sits between the value net's forward-only launch on s and
// its backward-only launch from SEED_PTR, the second between the actor's forward and its backward (learner_modes.hip
// iql_critic_phase / iql_action_grads).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace oprl {

constexpr int kIqlThreads = 256;       // both kernels: one lane per minibatch row, 16 slices of 16 rows per workgroup

struct IqlValueArgs {
  const float* q1;       // target critic 0 on (s, a) [B]
  const float* q2;       // target critic 1 on (s, a) [B]
  const float* v;        // V(s) [B]
  float tau, omtau;      // the expectile and 1 - expectile, each rounded from double on the host
  float beta, clip;      // inverse temperature (>= 0), advantage-weight clip (> 0)
  float inv_B;           // 1 / B
  int B, n_slices;       // rows; (B + kR - 1) / kR
  float* u;              // out [B]: min(q1, q2) - v
  float* seed;           // out [B]: ((2 (v - qt)) (1/B)) omega, what SEED_PTR reads with ld0 = 1
  float* w;              // out [B]: min(exp(beta u), clip)
  float* part_v;         // out [n_slices][4]: per slice (sum omega u^2, sum v, sum u) — launch_reduce_partials' layout
  float* part_w;         // out [n_slices][4]: per slice (0, sum w, rows at the clip)
};

struct IqlActorArgs {
  const float* pi;       // pi(s) [B][A]
  const float* a;        // the minibatch's actions [B][A]
  const float* w;        // the rows' weights [B] (k_iql_value_seed)
  float two_inv_B;       // 2 / B
  int B, A, n_slices;
  float* da;             // out [B][A]: (2/B) w_b (pi - a), written in full
  float* part;           // out [n_slices][4]: per slice (0, sum_b w_b sum_k (pi - a)^2, 0)
};

hipError_t launch_iql_value_seed(const IqlValueArgs& a, hipStream_t st);
hipError_t launch_iql_actor_seed(const IqlActorArgs& a, hipStream_t st);

}  // namespace oprl
