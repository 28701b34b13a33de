// iql_seed.hip — k_iql_value_seed / k_iql_actor_seed: the implicit-Q-learning mode of a TD3 learner (Kostrikov, Nair &
// Levine 2021).  With qt = min of the two TARGET critics on the dataset's (s, a) and u = qt - V(s):
//   the value net minimises the expectile loss  (1/B) sum_b omega_b u_b^2,  omega_b = 1 - tau where u_b < 0, else tau;
//   the actor minimises  (1/B) sum_b w_b sum_k (pi(s_b)_k - a_bk)^2,  w_b = min(exp(beta u_b), clip) a constant.
// k_iql_value_seed sits between the value net's forward-only launch on s, which leaves V(s) [B] in memory, and its
// backward-only launch from SEED_PTR; k_iql_actor_seed between the actor's forward and its backward (SEED_TANH).
//
// One lane per minibatch row; a workgroup is 16 slices of 16 rows, the slices of the slice kernels, so the per-slice sums
// land where launch_reduce_partials reads them.  Plain C++: vector stores only, no atomics, fixed summation orders (the
// slice butterfly of per_seed.hip, whose lanes past B hold zeros), nothing written for rows >= B; a row's results depend on
// that row's operands alone, so they are the same bits for every B, position and grid.
#include "iql_seed.h"

namespace oprl {

static_assert(kIqlThreads % kR == 0 && kR == 16, "a slice is 16 adjacent lanes of one wave");

// In this order:  qt = fminf(q1, q2);  u = qt - v;  omega = u < 0 ? omtau : tau;  seed = ((2 (v - qt)) (1/B)) omega;
// e = expf(beta u);  w = fminf(e, clip)  (e = +inf gives clip, e = 0 gives 0);  at the clip: e >= clip.
// The loss term is omega (u u).
__global__ __launch_bounds__(kIqlThreads) void k_iql_value_seed(const IqlValueArgs A) {
#pragma clang fp contract(off)
  const int gr = (int)blockIdx.x * kIqlThreads + (int)threadIdx.x, slice = gr / kR;
  const bool ok = gr < A.B;
  float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {
    const float v = A.v[gr];
    const float qt = fminf(A.q1[gr], A.q2[gr]);
    const float u = qt - v;
    const float omega = u < 0.f ? A.omtau : A.tau;
    const float e = expf(A.beta * u);
    const float w = fminf(e, A.clip);
    A.u[gr] = u;
    A.seed[gr] = ((2.f * (v - qt)) * A.inv_B) * omega;
    A.w[gr] = w;
    s[0] = omega * (u * u);
    s[1] = v;
    s[2] = u;
    s[3] = w;
    s[4] = e >= A.clip ? 1.f : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
#pragma unroll
    for (int m = 1; m < kR; m <<= 1) s[k] += __shfl_xor(s[k], m);
  }
  if ((threadIdx.x & (kR - 1)) == 0 && ok && slice < A.n_slices) {
    float* p = A.part_v + (size_t)slice * 4;
    p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
    float* q = A.part_w + (size_t)slice * 4;
    q[0] = 0.f; q[1] = s[3]; q[2] = s[4];
  }
}

// Row b, columns k = 0 .. A - 1 in order:  diff = pi - a;  da = (two_inv_B w_b) diff;  sq += diff diff;  the row's loss
// term is w_b sq.  da is WRITTEN: nothing else feeds the action gradients in this mode.
__global__ __launch_bounds__(kIqlThreads) void k_iql_actor_seed(const IqlActorArgs A) {
#pragma clang fp contract(off)
  const int gr = (int)blockIdx.x * kIqlThreads + (int)threadIdx.x, slice = gr / kR;
  const bool ok = gr < A.B;
  float term = 0.f;
  if (ok) {
    const float w = A.w[gr];
    const float c = A.two_inv_B * w;
    const size_t row = (size_t)gr * A.A;
    float sq = 0.f;
    for (int k = 0; k < A.A; ++k) {
      const float diff = A.pi[row + k] - A.a[row + k];
      A.da[row + k] = c * diff;
      sq += diff * diff;
    }
    term = w * sq;
  }
#pragma unroll
  for (int m = 1; m < kR; m <<= 1) term += __shfl_xor(term, m);
  if ((threadIdx.x & (kR - 1)) == 0 && ok && slice < A.n_slices) {
    float* p = A.part + (size_t)slice * 4;
    p[0] = 0.f; p[1] = term; p[2] = 0.f;
  }
}

hipError_t launch_iql_value_seed(const IqlValueArgs& a, hipStream_t st) {
  if (a.B < 1 || a.n_slices != (a.B + kR - 1) / kR || a.q1 == nullptr || a.q2 == nullptr || a.v == nullptr || a.u == nullptr ||
      a.seed == nullptr || a.w == nullptr || a.part_v == nullptr || a.part_w == nullptr || !(a.clip > 0.f) || !(a.beta >= 0.f))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_iql_value_seed, dim3((a.B + kIqlThreads - 1) / kIqlThreads), dim3(kIqlThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_iql_actor_seed(const IqlActorArgs& a, hipStream_t st) {
  if (a.B < 1 || a.A < 1 || (long)a.B * a.A > (1L << 30) || a.n_slices != (a.B + kR - 1) / kR || a.pi == nullptr || a.a == nullptr ||
      a.w == nullptr || a.da == nullptr || a.part == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_iql_actor_seed, dim3((a.B + kIqlThreads - 1) / kIqlThreads), dim3(kIqlThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace oprl
