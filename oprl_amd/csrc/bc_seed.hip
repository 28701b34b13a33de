// bc_seed.hip — k_bc_seed / k_bc_mix: the behaviour-cloning mode of a TD3 learner's actor step (TD3+BC, Fujimoto & Gu
// 2021).  The actor minimises  -lambda mean_b Q1(s_b, pi(s_b)) + mean_{b,k} (pi(s_b)_k - a_bk)^2  with
// lambda = alpha / mean_b |Q1(s_b, pi(s_b))| held constant for the gradient (no epsilon in the denominator, as in the
// authors' code).  k_bc_seed sits between critic 0's forward-only launch on (s, pi), which leaves q [B] in memory, and its
// backward-only launch from SEED_PTR; k_bc_mix adds the cloning term's gradient to the action gradients that backward
// leaves, before the actor's own backward reads them.
//
// Plain C++: vector stores only, no atomics, fixed summation orders, nothing written for rows >= B.
#include "bc_seed.h"

namespace oprl {

static_assert(kBcSeedThreads == 1024 && kR == 16 && kBcSlice == 16, "16 waves of 64 lanes; a slice is 16 adjacent lanes of one wave");

// ONE workgroup: the mean of |q| couples all rows, and with one grid its bits do not depend on how many workgroups ran.
// Thread t sums |q| over rows t, t + 1024, ... in that order; a 64-lane xor butterfly; the 16 wave sums through LDS in
// wave order.  The per-slice sums of q (16 rows = 16 adjacent lanes) take k_td_weighted_seed's slice butterfly.
__global__ __launch_bounds__(kBcSeedThreads) void k_bc_seed(const BcSeedArgs A) {
#pragma clang fp contract(off)
  __shared__ float red[kBcSeedThreads / 64];
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  const int n_pass = (A.B + kBcSeedThreads - 1) / kBcSeedThreads;      // (uniform: the shuffles need whole waves)
  float acc = 0.f;
  for (int k = 0; k < n_pass; ++k) {
    const int row = k * kBcSeedThreads + t;
    const bool ok = row < A.B;
    const float q = ok ? A.q[row] : 0.f;
    acc += fabsf(q);
    float v = q;
#pragma unroll
    for (int m = 1; m < kR; m <<= 1) v += __shfl_xor(v, m);
    const int slice = row / kR;
    if ((t & (kR - 1)) == 0 && ok && slice < A.n_slices && A.partials != nullptr) {
      float* p = A.partials + (size_t)slice * 4;
      p[0] = 0.f; p[1] = v; p[2] = 0.f;
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  float total = 0.f;
  for (int w = 0; w < kBcSeedThreads / 64; ++w) total += red[w];
  const float mean_abs = total / (float)A.B;
  const float lambda = A.alpha / mean_abs;
  const float sv = -(lambda * (1.f / (float)A.B));
  for (int k = 0; k < n_pass; ++k) {
    const int row = k * kBcSeedThreads + t;
    if (row < A.B) A.seed[row] = sv;
  }
  if (t == 0) { A.scal[0] = lambda; A.scal[1] = mean_abs; }
}

// One lane per element e = b A + k of pi: da += (2 / (B A)) (pi - a), and the sums of (pi - a)^2 over 16 adjacent
// elements (the slice butterfly again; the lanes past B A hold zeros), which oprl_learner_read_bc adds up in slice order.
__global__ __launch_bounds__(kBcMixThreads) void k_bc_mix(const BcMixArgs A) {
#pragma clang fp contract(off)
  const int n = A.B * A.A;
  const int e = (int)blockIdx.x * kBcMixThreads + (int)threadIdx.x;
  const bool ok = e < n;
  float sq = 0.f;
  if (ok) {
    const float diff = A.pi[e] - A.a[e];
    const float c = 2.f / ((float)A.B * (float)A.A);
    A.da[e] = A.da[e] + c * diff;
    sq = diff * diff;
  }
#pragma unroll
  for (int m = 1; m < kBcSlice; m <<= 1) sq += __shfl_xor(sq, m);
  if ((threadIdx.x & (kBcSlice - 1)) == 0 && ok) A.part[e / kBcSlice] = sq;
}

hipError_t launch_bc_seed(const BcSeedArgs& a, hipStream_t st) {
  if (a.B < 1 || !(a.alpha > 0.f) || a.q == nullptr || a.seed == nullptr || a.scal == nullptr) return hipErrorInvalidValue;
  if (a.partials != nullptr && a.n_slices != (a.B + kR - 1) / kR) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bc_seed, dim3(1), dim3(kBcSeedThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_bc_mix(const BcMixArgs& a, hipStream_t st) {
  if (a.B < 1 || a.A < 1 || (long)a.B * a.A > (1L << 30) || a.pi == nullptr || a.a == nullptr || a.da == nullptr || a.part == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bc_mix, dim3((a.B * a.A + kBcMixThreads - 1) / kBcMixThreads), dim3(kBcMixThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace oprl
