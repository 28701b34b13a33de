// c51_seed.hip — k_c51_critic_seed / k_c51_actor_seed: the loss-gradient seeds of D4PG's categorical critic (Bellemare et
// al. 2017; Barth-Maron et al. 2018), between the critic's forward-only launch, which leaves the logits [B][ld] in
// memory, and its backward-only launch from SEED_PTR (learner_modes.hip).
//
// One wave per minibatch row, lane j = atom j (N <= 48 < 64; the lanes past N hold the neutral element of every
// reduction).  A workgroup is 16 waves = one slice of kR = 16 rows, the slice of the slice kernels, so the per-slice sums
// land where launch_reduce_partials reads them.  A row's results depend on that row's operands only: the wave reductions
// are butterflies over all 64 lanes, the projection is a fixed-order loop, nothing is accumulated across rows except the
// diagnostics, which are combined in wave order.  No atomics, vector stores only, nothing written for rows >= B.
#include "c51_seed.h"

namespace oprl {

constexpr int kC51Waves = kR;                 // rows per workgroup
constexpr int kC51Threads = 64 * kC51Waves;
static_assert(kC51MaxAtoms <= 64 && kC51Threads <= 1024, "one lane per atom, one workgroup per slice");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) v += __shfl_xor(v, k);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) v = fmaxf(v, __shfl_xor(v, k));
  return v;
}

// max-subtracted softmax of a row of logits, lane j = atom j: p_j and, where asked for, log p_j (dead lanes: 0 and 0)
__device__ __forceinline__ float row_softmax(float z, bool act, float* logp = nullptr) {
#pragma clang fp contract(off)
  const float mx = wave_max(act ? z : -INFINITY);
  const float e = act ? expf(z - mx) : 0.f;
  const float s = wave_sum(e);
  if (logp != nullptr) *logp = act ? (z - mx) - logf(s) : 0.f;
  return e / s;
}

// the slice's sums of up to three per-row values (every lane of a wave holds its row's), in wave order through LDS
__device__ __forceinline__ void slice_sums(float v0, float v1, float v2, float* partials, int n_slices) {
  __shared__ float red[kC51Waves][4];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  if (lane == 0) { red[wave][0] = v0; red[wave][1] = v1; red[wave][2] = v2; }
  __syncthreads();
  if (threadIdx.x < 3 && partials != nullptr && (int)blockIdx.x < n_slices) {
    float s = 0.f;
    for (int w = 0; w < kC51Waves; ++w) s += red[w][threadIdx.x];
    partials[(size_t)blockIdx.x * 4 + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(kC51Threads) void k_c51_critic_seed(const C51Args A) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int row = (int)blockIdx.x * kC51Waves + wave;
  const bool ok = row < A.B;                       // (wave-uniform)
  const bool act = ok && lane < A.N;
  float loss = 0.f, q = 0.f, y = 0.f;
  if (ok) {
#pragma clang fp contract(off)
    const size_t o = (size_t)row * A.ld + lane;
    const float delta = (A.v_max - A.v_min) / (float)(A.N - 1);
    const float atom = A.v_min + (float)lane * delta;
    // 1. p' = softmax(Zbar(s', a')), p = softmax(Z(s, a))
    float lp;
    const float pt = row_softmax(act ? A.zt[o] : 0.f, act);
    const float p = row_softmax(act ? A.z[o] : 0.f, act, &lp);
    // 2. Tz_i = clamp(r + ((1 - d) gamma) z_i, v_min, v_max), b_i = (Tz_i - v_min) / delta — formed as the OFFSET from the
    // atom's own index, b_i - i = (r - (1 - g) v_min) / delta - (1 - g) i with g = (1 - d) gamma, clamped to [-i, N - 1 - i]:
    // the same number, but for g near 1 every term is small, so float32 keeps the fractional part to ~1e-7 where
    // (Tz_i - v_min) / delta loses it to the size of Tz_i (~4e-6 at 41 atoms: DESIGN.md §15, "Arithmetic")
    const float g = (1.f - A.d[row]) * A.gamma;
    const float omg = 1.f - g;
    const float c0 = (A.r[row] - omg * A.v_min) / delta;
    const float fl = (float)lane;
    const float off = fminf(fmaxf(c0 - omg * fl, -fl), (float)(A.N - 1) - fl);
    // 3. m_j = sum_i p'_i max(0, 1 - |b_i - j|), i in index order (p'_i and b_i - i from lane i; i - j is exact)
    float mj = 0.f;
    for (int i = 0; i < A.N; ++i) {
      const float pi = __shfl(pt, i), oi = __shfl(off, i);
      mj += pi * fmaxf(0.f, 1.f - fabsf(oi + (float)(i - lane)));
    }
    if (!act) mj = 0.f;
    // 4. the row's cross-entropy and its gradient with respect to the logits
    loss = wave_sum(-(mj * lp));
    q = wave_sum(act ? atom * p : 0.f);
    y = wave_sum(act ? atom * mj : 0.f);
    if (lane < A.ld) {
      A.seed[o] = act ? (p - mj) * A.inv_B : 0.f;
      if (A.m != nullptr) A.m[o] = mj;
    }
    if (lane == 0) {
      if (A.loss_row != nullptr) A.loss_row[row] = loss;
      if (A.q_out != nullptr) A.q_out[row] = q;
      if (A.y_out != nullptr) A.y_out[row] = y;
    }
  }
  slice_sums(loss, q, y, A.partials, A.n_slices);
}

// the actor step through the critic: loss -(1/B) sum_b Q_b, Q = sum_j z_j p_j; dQ / dlogit_j = p_j (z_j - Q)
__global__ __launch_bounds__(kC51Threads) void k_c51_actor_seed(const C51Args A) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int row = (int)blockIdx.x * kC51Waves + wave;
  const bool ok = row < A.B;
  const bool act = ok && lane < A.N;
  float q = 0.f;
  if (ok) {
#pragma clang fp contract(off)
    const size_t o = (size_t)row * A.ld + lane;
    const float delta = (A.v_max - A.v_min) / (float)(A.N - 1);
    const float atom = A.v_min + (float)lane * delta;
    const float p = row_softmax(act ? A.z[o] : 0.f, act);
    q = wave_sum(act ? atom * p : 0.f);
    if (lane < A.ld) A.seed[o] = act ? -(A.inv_B * (p * (atom - q))) : 0.f;
  }
  slice_sums(0.f, q, 0.f, A.partials, A.n_slices);
}

static bool c51_args_ok(const C51Args& a, bool critic) {
  if (a.B < 1 || a.N < 2 || a.N > kC51MaxAtoms || a.ld < a.N || a.ld > 64 || !(a.v_max > a.v_min)) return false;
  if (a.z == nullptr || a.seed == nullptr) return false;
  if (a.partials != nullptr && a.n_slices != (a.B + kR - 1) / kR) return false;
  if (critic && (a.zt == nullptr || a.r == nullptr || a.d == nullptr)) return false;
  return true;
}

hipError_t launch_c51_critic_seed(const C51Args& a, hipStream_t st) {
  if (!c51_args_ok(a, true)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_c51_critic_seed, dim3((a.B + kC51Waves - 1) / kC51Waves), dim3(kC51Threads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_c51_actor_seed(const C51Args& a, hipStream_t st) {
  if (!c51_args_ok(a, false)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_c51_actor_seed, dim3((a.B + kC51Waves - 1) / kC51Waves), dim3(kC51Threads), 0, st, a);
  return hipGetLastError();
}

}  // namespace oprl
