// per_seed.hip — k_td_weighted_seed: the loss-gradient seed of the MSE-TD critics (DDPG, TD3 / SAC, REDQ) under
// importance weights, between the critics' forward-only launches and their backward-only launches from SEED_PTR
// (learner_per.hip; DESIGN.md §11, "Training from it").  One lane per minibatch row; a workgroup is 16 slices of 16
// rows, the slices of the slice kernels, so the per-slice sums land where launch_reduce_partials reads them.
#include "per_seed.h"
#include "slice_head.h"

namespace oprl {

constexpr int kSeedThreads = 256;
static_assert(kSeedThreads % kR == 0 && kR == 16, "a slice is 16 adjacent lanes of one wave");

__global__ __launch_bounds__(kSeedThreads) void k_td_weighted_seed(const TdSeedArgs A) {
  const SeedArgs& S = A.s;
  const int gr = (int)blockIdx.x * kSeedThreads + (int)threadIdx.x, slice = gr / kR;
  const bool ok = gr < A.B;
  float y = 0.f, w = 0.f;
  if (ok) {
    // the TD target, in the words of slice_seed's SEED_MSE_TD case (slice_head.h): the same contraction, the same bits
    float qn = S.p0[gr];
    if (S.p1 != nullptr) qn = fminf(qn, S.p1[gr]);
    if (S.p2 != nullptr) qn -= alpha_of(S) * S.p2[gr];
    y = S.r[gr] + ((1.f - S.d[gr]) * S.gamma) * qn;
    w = A.w[gr];
  }
  float td = 0.f;
  for (int j = 0; j < A.nc; ++j) {       // (uniform trip count: the shuffles below need whole slices)
    float v[3] = {0.f, 0.f, 0.f};
    if (ok) {
      const float q = A.q[(size_t)j * A.q_stride + gr];
      A.seed[(size_t)j * A.seed_stride + gr] = 2.f * (q - y) * S.cval * w;
      if (j == 0 && S.y_out != nullptr) S.y_out[gr] = y;
      if (j == 0 && S.q_out != nullptr) S.q_out[gr] = q;
      td += fabsf(q - y);
      v[0] = w * ((q - y) * (q - y));
      v[1] = q;
      v[2] = y;
    }
    // a slice's sums over its 16 lanes in the slice kernels' order (slice_seed's butterfly, whose other lanes hold zeros)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int m = 1; m < kR; m <<= 1) v[k] += __shfl_xor(v[k], m);
    }
    if ((threadIdx.x & (kR - 1)) == 0 && slice < A.n_slices && A.partials != nullptr) {
      float* p = A.partials + ((size_t)j * A.n_slices + slice) * 4;
      p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
    }
  }
  if (ok) A.td_abs[gr] = td / (float)A.nc;
}

hipError_t launch_td_weighted_seed(const TdSeedArgs& a, hipStream_t st) {
  if (a.B < 1 || a.nc < 1 || a.n_slices != (a.B + kR - 1) / kR || a.q == nullptr || a.w == nullptr || a.seed == nullptr ||
      a.td_abs == nullptr || a.s.p0 == nullptr || a.s.r == nullptr || a.s.d == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_td_weighted_seed, dim3((a.B + kSeedThreads - 1) / kSeedThreads), dim3(kSeedThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace oprl
