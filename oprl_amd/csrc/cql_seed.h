// cql_seed.h — the argument blocks of k_cql_rows / k_cql_seed (cql_seed.hip): the conservative-Q-learning mode of a SAC
// learner (Kumar et al. 2020, CQL(H) with a fixed penalty weight).  The first builds the WIDE rows of the
// critic step — the minibatch's (s, a) and 3 N sampled actions per state — the second sits between the critics'
// forward-only launch on those rows and their backward-only launch from SEED_PTR (learner_modes.hip cql_critic_step).
//
// The wide rows, Bw = B (1 + 3 N) of them:
//   row b, b < B:                      (s_b, a_b), the data rows: the first (B + 15) / 16 slices are theirs;
//   row B + b 3N + e, e = kind N + k:  (s_b, x_bk) with  kind 0: x = u_bk uniform in [-1, 1]^A,
//                                      kind 1: x = p_bk ~ pi(.|s_b),  kind 2: x = n_bk ~ pi(.|s'_b)
// — all three kinds at s_b, and a row's 3 N entries next to each other.  logd[b][e] is the log-density the action was drawn
// with: -A log 2, log pi(p_bk|s_b), log pi(n_bk|s'_b).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace oprl {

constexpr int kCqlThreads = 256;       // both kernels; k_cql_seed: one lane per minibatch row, 16 slices of 16 rows per workgroup
constexpr int kCqlMaxActions = 16;     // N at most: 3 N <= 48 entries per row

struct CqlRowsArgs {
  const float* s;        // the minibatch's states [B][S]
  const float* a;        // ... and actions [B][A]
  const float* raw_s;    // the online actor's raw head rows on s [B][2A] (means | log-stds)
  const float* raw_s2;   // ... and on s'
  const float* eps;      // N(0,1) draws [B][2N][A] ([b][(kind - 1) N + k][col]); null: Philox, key_eps
  const float* uni;      // the uniform actions [B][N][A], clamped to [-1, 1]; null: Philox, key_uni
  unsigned long long key_eps, key_uni, ctr;   // Philox keys of the two streams and the counter (the learner's update count)
  int B, S, A, N;
  float* ws;             // out [Bw][S]: the wide states
  float* wa;             // out [Bw][A]: the wide actions
  float* logd;           // out [B][3N]: the log-densities
};

struct CqlSeedArgs {
  SeedArgs s;                    // the TD target's operands exactly as SEED_MSE_TD / k_td_weighted_seed take them; cval = 1/B; y_out / q_out (critic 0)
  const float* q; long q_stride; // the online critics on the wide rows, q[j * q_stride + row]
  const float* logd;             // [B][3N] (k_cql_rows)
  float ca;                      // cql_alpha (>= 0)
  float* seed; long seed_stride; // out: seed[j * seed_stride + row], what SEED_PTR reads with ld0 = 1 —
                                 //   data row b: ((2 (q - y)) - ca) (1/B);  sampled row (b, e): (ca softmax(c_jb.)_e) (1/B)
  float* partials;               // out [nc][n_slices][4]: per slice of 16 data rows (sum (q - y)^2, sum q, sum y) — launch_reduce_partials' layout
  float* part_cql;               // out [nc][n_slices][4]: per slice (sum (lse - q), sum_b sum_k q on the uniform actions, ... on the kind-1 policy actions)
  int nc, B, N, n_slices;        // critics, minibatch rows, sampled actions per kind, (B + kR - 1) / kR
  const float* g;                // the calibrated form only (Cal-QL): the rows' returns-to-go [B], the lower bound of
                                 //   q at the policy entries e in [N, 3N); part_cql[..][3] then takes the count of bounded entries
};

hipError_t launch_cql_rows(const CqlRowsArgs& a, hipStream_t st);
hipError_t launch_cql_seed(const CqlSeedArgs& a, hipStream_t st);      // a.g null: the plain kernel; else the calibrated one

}  // namespace oprl
