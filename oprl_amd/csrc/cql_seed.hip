// cql_seed.hip — k_cql_rows / k_cql_seed: the conservative-Q-learning mode of a SAC learner (Kumar et al. 2020, CQL(H) with
// a fixed penalty weight).  Per critic j the loss is
//   (1/B) sum_b (Q_j(s_b, a_b) - y_b)^2  +  cql_alpha (1/B) sum_b [ logsumexp_e c_jbe - Q_j(s_b, a_b) ],
//   c_jbe = Q_j(s_b, x_be) - logdensity(x_be)   over the 3 N sampled actions x_be of row b (cql_seed.h: uniform, pi(.|s_b),
//   pi(.|s'_b), all evaluated at s_b),
// so the critic step runs on the wide rows k_cql_rows builds, and k_cql_seed turns the critics' outputs on them into the
// seed rows their backward-only launch reads (SEED_PTR).
//
// Plain C++: vector stores only, no atomics, fixed summation orders, nothing written for rows past an extent.  A row's
// results depend on that row's operands and 1/B alone — the same bits at every B, position and grid, the seeds up to their
// last multiplication by the float32 1/B.
#include "cql_seed.h"
#include "slice_head.h"

namespace oprl {

static_assert(kCqlThreads % kR == 0 && kR == 16, "a slice is 16 adjacent lanes of one wave");

constexpr float kLog2 = 0.69314718055994530942f;

// uniform in (-1, 1) addressed by (stream ctr, row, col): 24 bits of one Philox word
__device__ __forceinline__ float philox_uniform_pm1(unsigned long long seed, unsigned long long ctr, uint32_t row, uint32_t col) {
#pragma clang fp contract(off)
  const u32x4 r = philox4x32_10(u32x4{(uint32_t)ctr, (uint32_t)(ctr >> 32), row, col}, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float u = ((float)(r.x >> 8) + 0.5f) * (1.0f / 16777216.0f);      // (0, 1)
  return 2.f * u - 1.f;
}

// One thread per wide row (cql_seed.h has the layout).  A data row is a copy; a sampled row copies s_b and, column by
// column in order, draws its action: kind 0 the uniform one (log-density -A log 2), kinds 1 / 2 the tanh-Gaussian sample of
// the raw head row at s_b / s'_b with gauss_elem (slice_head.h) — ACT_GAUSS's formula, clamp and tanh correction — whose
// terms are added in column order.  The thread of a row's entry e writes logd[b][e].
__global__ __launch_bounds__(kCqlThreads) void k_cql_rows(const CqlRowsArgs A) {
#pragma clang fp contract(off)
  const int B = A.B, S = A.S, Ad = A.A, N = A.N, E = 3 * N;
  const int row = (int)blockIdx.x * kCqlThreads + (int)threadIdx.x;
  if (row >= B * (1 + E)) return;
  int b = row, e = -1;
  if (row >= B) {
    const int idx = row - B;
    b = idx / E;
    e = idx - b * E;
  }
  const float* sb = A.s + (size_t)b * S;
  float* so = A.ws + (size_t)row * S;
  for (int i = 0; i < S; ++i) so[i] = sb[i];
  float* ao = A.wa + (size_t)row * Ad;
  if (e < 0) {
    const float* ab = A.a + (size_t)b * Ad;
    for (int col = 0; col < Ad; ++col) ao[col] = ab[col];
    return;
  }
  const int kind = e / N, k = e - kind * N;
  float lp;
  if (kind == 0) {
    const int ur = b * N + k;
    for (int col = 0; col < Ad; ++col) {
      const float u = A.uni != nullptr ? fminf(fmaxf(A.uni[(size_t)ur * Ad + col], -1.f), 1.f)
                                       : philox_uniform_pm1(A.key_uni, A.ctr, (uint32_t)ur, (uint32_t)col);
      ao[col] = u;
    }
    lp = -((float)Ad * kLog2);
  } else {
    const float* raw = (kind == 1 ? A.raw_s : A.raw_s2) + (size_t)b * 2 * Ad;
    const int er = b * 2 * N + (kind - 1) * N + k;
    lp = 0.f;
    for (int col = 0; col < Ad; ++col) {
      const float eps = A.eps != nullptr ? A.eps[(size_t)er * Ad + col] : philox_normal(A.key_eps, A.ctr, (uint32_t)er, (uint32_t)col);
      float act;
      lp += gauss_elem(raw[col], raw[Ad + col], eps, &act);
      ao[col] = act;
    }
  }
  A.logd[(size_t)b * E + e] = lp;
}

// The TD target of row gr in the words of slice_seed's SEED_MSE_TD case (slice_head.h) and of k_td_weighted_seed, under the
// same contraction rules as they are: the same bits.
__device__ __forceinline__ float cql_td_target(const SeedArgs& S, int gr) {
  float qn = S.p0[gr];
  if (S.p1 != nullptr) qn = fminf(qn, S.p1[gr]);
  if (S.p2 != nullptr) qn -= alpha_of(S) * S.p2[gr];
  return S.r[gr] + ((1.f - S.d[gr]) * S.gamma) * qn;
}

// One lane per minibatch row; per critic j, over the row's entries e = 0 .. 3N - 1 in order, three passes:
//   m = max_e c_e;   z = sum_e expf(c_e - m);   lse = m + logf(z);   p_e = expf(c_e - m) / z   (the max-subtracted softmax)
//   seed(b, e) = (ca p_e) (1/B);   seed(b) = ((2 (q - y)) - ca) (1/B)
// and the slice sums over 16 adjacent lanes in the slice kernels' order (k_td_weighted_seed's butterfly, lanes past B hold
// zeros).  The entries are re-read in each pass (3 N <= 48 floats per row and critic, from L2) instead of kept in an
// indexed register array.
//
// kCal, the calibrated form (Cal-QL, Nakamoto et al. 2023): at the policy entries e in [N, 3N) the critic's
// value is bounded below by the row's return-to-go g_b — c_e = max(q_e, g_b) - logd_e in all three passes — and the bound
// passes no gradient: seed(b, e) = (ca p_e)(1/B) if q_e >= g_b, else 0 (written, as 0).  The uniform entries are not
// bounded.  Everything else is formed as in the plain form, from c; the sums of q stay sums of the critic's own q.  Slot 3
// of part_cql takes the count of bounded entries (exact in float: at most 512 per slice).  The plain instantiation reads
// no g and leaves slot 3 alone.
template <bool kCal>
__global__ __launch_bounds__(kCqlThreads) void k_cql_seed(const CqlSeedArgs A) {
#pragma clang fp contract(off)
  const SeedArgs& S = A.s;
  const int gr = (int)blockIdx.x * kCqlThreads + (int)threadIdx.x, slice = gr / kR;
  const bool ok = gr < A.B;
  const int N = A.N, E = 3 * N;
  const float y = ok ? cql_td_target(S, gr) : 0.f;
  for (int j = 0; j < A.nc; ++j) {       // (uniform trip count: the shuffles below need whole slices)
    constexpr int kV = kCal ? 7 : 6;
    float v[kV] = {};
    if (ok) {
      const float* qj = A.q + (size_t)j * A.q_stride;
      float* sj = A.seed + (size_t)j * A.seed_stride;
      const float q = qj[gr];
      const float* qe = qj + (size_t)A.B + (size_t)gr * E;
      float* se = sj + (size_t)A.B + (size_t)gr * E;
      const float* ld = A.logd + (size_t)gr * E;
      const float gb = kCal ? A.g[gr] : 0.f;
      // the entry's value as the penalty sees it: the critic's, or in the calibrated form at a policy entry max(q_e, g_b)
      auto qt = [&](int e) { return kCal && e >= N ? fmaxf(qe[e], gb) : qe[e]; };
      float m = qt(0) - ld[0];
      for (int e = 1; e < E; ++e) m = fmaxf(m, qt(e) - ld[e]);
      float z = 0.f, q_uni = 0.f, q_pi = 0.f;
      for (int e = 0; e < E; ++e) {
        z += expf((qt(e) - ld[e]) - m);
        if (e < N) q_uni += qe[e];
        else if (e < 2 * N) q_pi += qe[e];
      }
      const float lse = m + logf(z);
      float n_bound = 0.f;
      for (int e = 0; e < E; ++e) {
        const float p = expf((qt(e) - ld[e]) - m) / z;
        float sd = (A.ca * p) * S.cval;
        if (kCal && e >= N && !(qe[e] >= gb)) sd = 0.f;
        if (kCal && e >= N && qe[e] < gb) n_bound += 1.f;
        se[e] = sd;
      }
      sj[gr] = ((2.f * (q - y)) - A.ca) * S.cval;
      if (j == 0 && S.y_out != nullptr) S.y_out[gr] = y;
      if (j == 0 && S.q_out != nullptr) S.q_out[gr] = q;
      v[0] = (q - y) * (q - y);
      v[1] = q;
      v[2] = y;
      v[3] = lse - q;
      v[4] = q_uni;
      v[5] = q_pi;
      if constexpr (kCal) v[6] = n_bound;
    }
#pragma unroll
    for (int k = 0; k < kV; ++k) {
#pragma unroll
      for (int mm = 1; mm < kR; mm <<= 1) v[k] += __shfl_xor(v[k], mm);
    }
    if ((threadIdx.x & (kR - 1)) == 0 && ok && slice < A.n_slices) {
      float* p = A.partials + ((size_t)j * A.n_slices + slice) * 4;
      p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
      float* c = A.part_cql + ((size_t)j * A.n_slices + slice) * 4;
      c[0] = v[3]; c[1] = v[4]; c[2] = v[5];
      if constexpr (kCal) c[3] = v[6];
    }
  }
}

hipError_t launch_cql_rows(const CqlRowsArgs& a, hipStream_t st) {
  if (a.B < 1 || a.S < 1 || a.A < 1 || a.N < 1 || a.N > kCqlMaxActions || a.s == nullptr || a.a == nullptr || a.raw_s == nullptr ||
      a.raw_s2 == nullptr || a.ws == nullptr || a.wa == nullptr || a.logd == nullptr)
    return hipErrorInvalidValue;
  const long Bw = (long)a.B * (1 + 3 * a.N);
  if (Bw * (a.S > a.A ? a.S : a.A) > (1L << 30)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cql_rows, dim3((unsigned)((Bw + kCqlThreads - 1) / kCqlThreads)), dim3(kCqlThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_cql_seed(const CqlSeedArgs& a, hipStream_t st) {
  if (a.B < 1 || a.nc < 1 || a.N < 1 || a.N > kCqlMaxActions || a.n_slices != (a.B + kR - 1) / kR || (long)a.B * (1 + 3 * a.N) > (1L << 30) ||
      a.q == nullptr || a.logd == nullptr || a.seed == nullptr || a.partials == nullptr || a.part_cql == nullptr || a.s.p0 == nullptr ||
      a.s.r == nullptr || a.s.d == nullptr || !(a.ca >= 0.f))
    return hipErrorInvalidValue;
  const dim3 grid((a.B + kCqlThreads - 1) / kCqlThreads);
  if (a.g != nullptr) hipLaunchKernelGGL(k_cql_seed<true>, grid, dim3(kCqlThreads), 0, st, a);
  else hipLaunchKernelGGL(k_cql_seed<false>, grid, dim3(kCqlThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace oprl
