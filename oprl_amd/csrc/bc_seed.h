// bc_seed.h — the argument blocks of k_bc_seed / k_bc_mix (bc_seed.hip): the behaviour-cloning mode of a TD3 learner's
// actor step (TD3+BC, Fujimoto & Gu 2021), between critic 0's forward-only launch on (s, pi) and its backward-only launch
// from SEED_PTR, and between that backward and the actor's (learner_modes.hip bc_action_grads).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace oprl {

constexpr int kBcSeedThreads = 1024;   // k_bc_seed: ONE workgroup, whatever B is
constexpr int kBcMixThreads = 256;     // k_bc_mix: one lane per element of pi
constexpr int kBcSlice = kR;           // k_bc_mix: adjacent lanes (elements) per partial sum

struct BcSeedArgs {
  const float* q;        // Q1(s, pi(s)) [B]
  float alpha;           // bc_alpha (> 0)
  int B, n_slices;       // rows; (B + kR - 1) / kR
  float* seed;           // out [B]: -(lambda (1/B)), what SEED_PTR reads with ld0 = 1
  float* scal;           // out [0] = lambda = alpha / mean |q|, [1] = mean |q|  ([2], [3] are not written)
  float* partials;       // out or null: [n_slices][4] per-slice (0, sum q, 0) — launch_reduce_partials' layout
};

struct BcMixArgs {
  const float* pi;       // pi(s) [B][A]
  const float* a;        // the minibatch's actions [B][A]
  float* da;             // in / out [B][A]: da += (2 / (B A)) (pi - a)
  float* part;           // out: [(B A + kBcSlice - 1) / kBcSlice] sums of (pi - a)^2 over kBcSlice adjacent elements
  int B, A;
};

inline int bc_mix_slices(int B, int A) { return (B * A + kBcSlice - 1) / kBcSlice; }

hipError_t launch_bc_seed(const BcSeedArgs& a, hipStream_t st);
hipError_t launch_bc_mix(const BcMixArgs& a, hipStream_t st);

}  // namespace oprl
