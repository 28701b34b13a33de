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
// The shape is the gather kernels' (replay_gather.h): the slot phase and the write-back are the shared ones; the two
// load rounds are this kernel's.  states[E, L+1, S] keeps s_{t+m} in the same episode row as s_t, m rows on.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/oprl_amd.h"
#include "replay_gather.h"

using namespace oprl;

namespace {

constexpr int kMaxN = kNstepMax;                  // one lane per (sample, step): kSamplesPerWg * kMaxN = kGatherThreads
static_assert(kSamplesPerWg * kMaxN == kGatherThreads, "one (sample, step) pair per lane");

struct NstepArgs {
  GatherSrc src;
  int n;
  float pw[kMaxN + 1];   // (float)pow((double)γ, k), formed on the host
  GatherOut out;
  int* out_m;
};

__global__ __launch_bounds__(kGatherThreads) void k_replay_gather_nstep(const NstepArgs K) {
  extern __shared__ float stage[];  // [kSamplesPerWg][2S + A]: s | a | s_{t+m}
  __shared__ int s_ep[kSamplesPerWg], s_t[kSamplesPerWg], s_mmax[kSamplesPerWg], s_m[kSamplesPerWg];
  __shared__ float s_r[kSamplesPerWg * kMaxN], s_d[kSamplesPerWg * kMaxN];
  __shared__ float s_R[kSamplesPerWg], s_D[kSamplesPerWg], s_pw[kMaxN + 1];
  __shared__ int s_ends[kMaxEndsLds];
  const GatherSrc& G = K.src;
  const int tid = threadIdx.x;
  const EndsLds ET = stage_ends(G.ends, G.n_eps, s_ends, kMaxEndsLds, tid, kGatherThreads);
  if (tid <= kMaxN) s_pw[tid] = K.pw[tid];          // (the scan indexes the powers by a per-lane step count)
  __syncthreads();
  const int base = blockIdx.x * kSamplesPerWg;
  const int S = G.S, A = G.A, W = 2 * S + A, SA = S + A;
  gather_slots(G, K.out, ET, base, s_ep, s_t, [&](int, bool live, const Slot& sl) {
    // steps of this episode from t on; an index past every end (the all-True argmin: e = 0, t = ind) gets one step,
    // which is what the plain gather reads for it
    s_mmax[tid] = live ? (int)max(1L, min((long)K.n, sl.end - sl.start - (long)sl.t)) : 1;
  });
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
  gather_write_rows(K.out, S, A, base, n_here, stage, W, SA, S);
  gather_write_rd(K.out, base, n_here, s_R, s_D, 1);
  if (tid < n_here && K.out_m != nullptr) K.out_m[base + tid] = s_m[tid];
}

}  // namespace

extern "C" int oprl_replay_set_nstep(oprl_replay* h, int32_t n, double gamma) {
  if (!h) { set_err("oprl_replay_set_nstep: null replay handle"); return OPRL_ERR_INVALID; }
  if (n < 1 || n > kNstepMax || !(gamma > 0.0) || !(gamma <= 1.0)) {
    set_err("oprl_replay_set_nstep: need 1 <= n <= %d and 0 < gamma <= 1 (got n = %d, gamma = %g)", kNstepMax, (int)n, gamma);
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
  if (h->prior && n > 1) {
    set_err("oprl_replay_set_nstep: this replay mixes prior data into its batches (oprl_replay_set_prior); n-step returns over mixed batches are not supported");
    return OPRL_ERR_STATE;
  }
  h->nstep = n;
  h->nstep_gamma = gamma;
  return OPRL_OK;
}

extern "C" int oprl_replay_sample_nstep(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed, uint64_t counter,
                                        float* out_s, float* out_a, float* out_r, float* out_d, float* out_s2,
                                        int32_t* out_ep, int32_t* out_step, int32_t* out_m, void* stream) {
  RC(gather_check("oprl_replay_sample_nstep", h, B, out_s, out_a, out_r, out_d, out_s2));
  NstepArgs K;
  gather_fill(h, B, idx, seed, counter, out_s, out_a, out_r, out_d, out_s2, out_ep, out_step, &K.src, &K.out);
  K.n = h->nstep;
  for (int k = 0; k <= kMaxN; ++k) K.pw[k] = (float)pow(h->nstep_gamma, (double)k);
  K.out_m = out_m;
  return gather_launch("oprl_replay_sample_nstep: buffer is empty", k_replay_gather_nstep, K, 2 * h->S + h->A, h, stream);
}
