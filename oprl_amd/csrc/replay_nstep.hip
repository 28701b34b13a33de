// replay_nstep.hip — n-step returns out of the HBM episodic replay: the uniform sampler's gather with the reward, the
// done flag and the next state replaced by their multi-step forms.
//
// Reference: none (the reference samples one-step transitions only, buffers/episodic_buffer.py:123-133; its unused
// `gamma` field is what this sampler reads).  Every TD target of the learners has the form y = r + ((1 - d) γ) q'(s'),
// with d read as a float, so a sampler that writes
//   r  <- R = Σ_{k<m} γ^k r_{t+k}
//   d  <- 1 - γ^{m-1} (1 - d_{t+m-1})
//   s' <- s_{t+m}
// makes them compute R + γ^m (1 - d_last) q'(s_{t+m}) without a change to their device code.  m counts the steps
// taken: at most n, never past the episode's stored steps, and none after the first step whose done is not 0.
//
// The shape is k_replay_gather's (replay.hip): 256 threads, 16 samples per workgroup, the episode table staged in LDS,
// rows staged in LDS and written coalesced.  states[E, L+1, S] keeps s_{t+m} in the same episode row as s_t, m rows on.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/oprl_amd.h"
#include "philox.h"
#include "replay_index.h"
#include "replay_internal.h"

namespace oprl {
void set_err(const char* fmt, ...);
void prof_begin(int kind, hipStream_t st);
void prof_end(hipStream_t st);
}
using oprl::set_err;

#define HIPC(x)                                                              \
  do {                                                                       \
    hipError_t _e = (x);                                                     \
    if (_e != hipSuccess) {                                                  \
      set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
      return OPRL_ERR_HIP;                                                   \
    }                                                                        \
  } while (0)

namespace {

constexpr int kGatherThreads = 256;
constexpr int kSamplesPerWg = 16;
constexpr int kMaxEndsLds = 2048;                 // as k_replay_gather: episode-end table entries staged in LDS
constexpr int kMaxN = oprl::kNstepMax;            // one lane per (sample, step): kSamplesPerWg * kMaxN = kGatherThreads
static_assert(kSamplesPerWg * kMaxN == kGatherThreads, "one (sample, step) pair per lane");

// Single IEEE operations, round to nearest, never contracted to FMA: the numpy oracle (tests/nstep_oracle.py) reproduces
// the sums bit for bit.  (__fmul_rn / __fadd_rn are plain operators in hipcc's headers and contract once inlined; the
// pragma takes the `contract` flag off these operations.)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

struct NstepArgs {
  const float *states, *actions, *rewards, *dones;
  const int* ends;  // cumulative episode ends, [n_eps]
  int n_eps, L, S, A, B, n;
  long n_transitions;
  const long long* idx;  // or null
  unsigned long long seed, counter;
  float pw[kMaxN + 1];   // (float)pow((double)γ, k), formed on the host
  float *out_s, *out_a, *out_r, *out_d, *out_s2;
  int *out_ep, *out_step, *out_m;
};

__global__ __launch_bounds__(kGatherThreads) void k_replay_gather_nstep(const NstepArgs G) {
  extern __shared__ float stage[];  // [kSamplesPerWg][2S + A]: s | a | s_{t+m}
  __shared__ int s_ep[kSamplesPerWg], s_t[kSamplesPerWg], s_mmax[kSamplesPerWg], s_m[kSamplesPerWg];
  __shared__ float s_r[kSamplesPerWg * kMaxN], s_d[kSamplesPerWg * kMaxN];
  __shared__ float s_R[kSamplesPerWg], s_D[kSamplesPerWg], s_pw[kMaxN + 1];
  __shared__ int s_ends[kMaxEndsLds];
  const int tid = threadIdx.x;
  const oprl::EndsLds ET = oprl::stage_ends(G.ends, G.n_eps, s_ends, kMaxEndsLds, tid, kGatherThreads);
  if (tid <= kMaxN) s_pw[tid] = G.pw[tid];          // (the scan indexes the powers by a per-lane step count)
  __syncthreads();
  const int base = blockIdx.x * kSamplesPerWg;
  const int S = G.S, A = G.A, W = 2 * S + A, SA = S + A;
  if (tid < kSamplesPerWg) {
    const int i = base + tid;
    int e = 0, t = 0, mmax = 1;
    if (i < G.B) {
      long ind;
      if (G.idx != nullptr) {
        ind = (long)G.idx[i];
      } else {
        // the uniform sampler's draw, word for word: the same (seed, counter) picks the same (e, t)
        const oprl::u32x4 r = oprl::philox4x32_10(
            oprl::u32x4{(uint32_t)G.counter, (uint32_t)(G.counter >> 32), (uint32_t)i, 0x5a17u},
            (uint32_t)G.seed, (uint32_t)(G.seed >> 32));
        ind = (long)oprl::bounded_u32(r.x, (uint32_t)G.n_transitions);
      }
      long start = 0;
      e = oprl::find_episode(G.ends, G.n_eps, ET, ind, &start);
      t = (int)(ind - start);
      const long end = ET.stride == 1 ? (long)ET.lds[e] : (long)G.ends[e];
      // steps of this episode from t on; an index past every end (the all-True argmin: e = 0, t = ind) gets one step,
      // which is what the plain gather reads for it
      const long left = end - start - (long)t;
      mmax = (int)max(1L, min((long)G.n, left));
      if (G.out_ep != nullptr) G.out_ep[i] = e;
      if (G.out_step != nullptr) G.out_step[i] = t;
    }
    s_ep[tid] = e;
    s_t[tid] = t;
    s_mmax[tid] = mmax;
  }
  __syncthreads();
  const int n_here = min(kSamplesPerWg, G.B - base);
  // Round 1, every load issued before the first LDS store (branch-free sources, as in k_replay_gather): lane
  // (sample, k) takes r and d of step t + min(k, m_max - 1) — nothing past the episode's stored steps is read — and
  // the s | a rows, which do not depend on m, travel in the same round.
  constexpr int kU = 2;
  {
    const int smp = tid / kMaxN, k = min(tid % kMaxN, s_mmax[smp] - 1);
    const long o = (long)s_ep[smp] * G.L + s_t[smp] + k;
    const float rk = G.rewards[o], dk = G.dones[o];
    for (int i0 = 0; i0 < n_here * SA; i0 += kU * kGatherThreads) {
      float v[kU];
#pragma unroll
      for (int j = 0; j < kU; ++j) {
        const int idx = min(i0 + j * kGatherThreads + tid, n_here * SA - 1);
        const int q = idx / SA, c = idx - q * SA;
        const long e = s_ep[q], t = s_t[q];
        const float* src = G.states + (e * (G.L + 1) + t) * S + c;
        if (c >= S) src = G.actions + (e * G.L + t) * A + (c - S);
        v[j] = *src;
      }
#pragma unroll
      for (int j = 0; j < kU; ++j) {
        const int idx = i0 + j * kGatherThreads + tid;
        if (idx < n_here * SA) { const int q = idx / SA; stage[q * W + (idx - q * SA)] = v[j]; }
      }
    }
    s_r[tid] = rk;
    s_d[tid] = dk;
  }
  __syncthreads();
  // One lane per sample scans its row in a fixed order (mul_rn / add_rn: no FMA).
  if (tid < kSamplesPerWg) {
    const float* r = s_r + tid * kMaxN;
    const float* d = s_d + tid * kMaxN;
    const int mmax = s_mmax[tid];
    float R = r[0];
    int m = 1;
    while (m < mmax && d[m - 1] == 0.f) {
      R = add_rn(R, mul_rn(s_pw[m], r[m]));
      ++m;
    }
    const float dl = d[m - 1];
    s_m[tid] = m;
    s_R[tid] = R;
    s_D[tid] = m == 1 ? dl : add_rn(1.f, -mul_rn(s_pw[m - 1], add_rn(1.f, -dl)));
  }
  __syncthreads();
  // Round 2: s_{t+m}, the one load that waits for the scan
  for (int i0 = 0; i0 < n_here * S; i0 += kU * kGatherThreads) {
    float v[kU];
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      const int idx = min(i0 + j * kGatherThreads + tid, n_here * S - 1);
      const int q = idx / S, c = idx - q * S;
      const long e = s_ep[q], t = s_t[q] + s_m[q];
      v[j] = G.states[(e * (G.L + 1) + t) * S + c];
    }
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      const int idx = i0 + j * kGatherThreads + tid;
      if (idx < n_here * S) { const int q = idx / S; stage[q * W + SA + (idx - q * S)] = v[j]; }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < n_here * S; idx += kGatherThreads) {
    const int smp = idx / S, c = idx - smp * S;
    G.out_s[(size_t)(base + smp) * S + c] = stage[smp * W + c];
    G.out_s2[(size_t)(base + smp) * S + c] = stage[smp * W + SA + c];
  }
  for (int idx = tid; idx < n_here * A; idx += kGatherThreads) {
    const int smp = idx / A, c = idx - smp * A;
    G.out_a[(size_t)(base + smp) * A + c] = stage[smp * W + S + c];
  }
  if (tid < n_here) {
    G.out_r[base + tid] = s_R[tid];
    G.out_d[base + tid] = s_D[tid];
    if (G.out_m != nullptr) G.out_m[base + tid] = s_m[tid];
  }
}

}  // namespace

extern "C" int oprl_replay_set_nstep(oprl_replay* h, int32_t n, double gamma) {
  if (!h) { set_err("oprl_replay_set_nstep: null replay handle"); return OPRL_ERR_INVALID; }
  if (n < 1 || n > oprl::kNstepMax || !(gamma > 0.0) || !(gamma <= 1.0)) {
    set_err("oprl_replay_set_nstep: need 1 <= n <= %d and 0 < gamma <= 1 (got n = %d, gamma = %g)", oprl::kNstepMax, (int)n, gamma);
    return OPRL_ERR_INVALID;
  }
  if (h->prio && n > 1) {
    set_err("oprl_replay_set_nstep: this replay is prioritized; n-step returns over the sum tree are not supported");
    return OPRL_ERR_STATE;
  }
  if (h->her.G > 0 && n > 1) {
    set_err("oprl_replay_set_nstep: this replay relabels goals in hindsight (oprl_replay_set_her); n-step returns over relabelled rows are not supported");
    return OPRL_ERR_STATE;
  }
  h->nstep = n;
  h->nstep_gamma = gamma;
  return OPRL_OK;
}

extern "C" int oprl_replay_sample_nstep(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed, uint64_t counter,
                                        float* out_s, float* out_a, float* out_r, float* out_d, float* out_s2,
                                        int32_t* out_ep, int32_t* out_step, int32_t* out_m, void* stream) {
  if (!h || B < 1 || !out_s || !out_a || !out_r || !out_d || !out_s2) {
    set_err("oprl_replay_sample_nstep: invalid argument");
    return OPRL_ERR_INVALID;
  }
  if (h->n_transitions <= 0 || h->n_eps <= 0) {
    set_err("oprl_replay_sample_nstep: buffer is empty");
    return OPRL_ERR_STATE;
  }
  int rc = oprl_replay_flush(h, stream);
  if (rc != OPRL_OK) return rc;
  NstepArgs G;
  G.states = h->states; G.actions = h->actions; G.rewards = h->rewards; G.dones = h->dones;
  G.ends = h->ends_dev; G.n_eps = h->n_eps; G.L = h->L; G.S = h->S; G.A = h->A; G.B = B; G.n = h->nstep;
  G.n_transitions = h->n_transitions;
  G.idx = (const long long*)idx; G.seed = seed; G.counter = counter;
  for (int k = 0; k <= kMaxN; ++k) G.pw[k] = (float)pow(h->nstep_gamma, (double)k);
  G.out_s = out_s; G.out_a = out_a; G.out_r = out_r; G.out_d = out_d; G.out_s2 = out_s2;
  G.out_ep = out_ep; G.out_step = out_step; G.out_m = out_m;
  const int grid = (B + kSamplesPerWg - 1) / kSamplesPerWg;
  const size_t lds = sizeof(float) * kSamplesPerWg * (2 * h->S + h->A);
  oprl::prof_begin(2, (hipStream_t)stream);
  hipLaunchKernelGGL(k_replay_gather_nstep, dim3(grid), dim3(kGatherThreads), lds, (hipStream_t)stream, G);
  oprl::prof_end((hipStream_t)stream);
  HIPC(hipGetLastError());
  return OPRL_OK;
}
