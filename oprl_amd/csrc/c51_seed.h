// c51_seed.h — the argument block of k_c51_critic_seed / k_c51_actor_seed (c51_seed.hip): the loss-gradient seeds of
// D4PG's categorical critic, between the critic's forward-only launch and its backward-only launch from SEED_PTR
// (learner_modes.hip c51_critic_step, c51_action_grads).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace oprl {

constexpr int kC51MaxAtoms = kNarrowMax;   // one lane per atom, and the critic's output is a narrow one

struct C51Args {
  const float* z;        // online logits [B][ld]
  const float* zt;       // critic seed: target logits Zbar(s', a') [B][ld]
  const float* r;        // critic seed: [B]
  const float* d;        // critic seed: [B]
  float gamma, v_min, v_max;
  float inv_B;           // 1 / B: the mean over the minibatch
  int N, B, ld;          // atoms (2 .. kC51MaxAtoms), rows, row stride of z / zt / seed / m (>= N, <= 64)
  float* seed;           // out [B][ld]: dL / dlogit, pad columns N .. ld - 1 zero
  float* m;              // critic seed, out or null: the projected target distribution [B][ld] (pad columns zero)
  float* loss_row;       // critic seed, out or null: [B] the row's cross-entropy
  float* q_out;          // critic seed, out or null: [B] sum_j z_j p_j
  float* y_out;          // critic seed, out or null: [B] sum_j z_j m_j
  float* partials;       // out or null: [n_slices][4] per-slice sums — critic: loss, q, y; actor: 0, Q, 0
  int n_slices;
};

hipError_t launch_c51_critic_seed(const C51Args& a, hipStream_t st);
hipError_t launch_c51_actor_seed(const C51Args& a, hipStream_t st);

}  // namespace oprl
