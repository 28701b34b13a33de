// replay_her.hip — hindsight experience replay out of the HBM episodic replay: the uniform sampler's gather with the
// desired goal of a share of the rows replaced by a goal the same episode achieved later, and their reward recomputed
// (DESIGN.md §18).
//
// Reference: none (the reference samples stored transitions only, buffers/episodic_buffer.py:123-133).  Andrychowicz et
// al., "Hindsight Experience Replay", NeurIPS 2017: strategies `future` and `final`.  A flat state row carries the
// achieved goal at [ag_off, ag_off + G) and the desired goal at [g_off, g_off + G).  For a drawn slot (e, t) of an
// episode with len_e stored steps, c = len_e - 1 - t later rows states[e, t' + 1], t <= t' <= len_e - 2, are always
// written (the row behind the last stored step is not).  A row is relabelled iff c >= 1 and U < ratio:
//   g'   = ag(states[e, t' + 1])           t' = t + bounded_u32(r.z, c) (future) | len_e - 2 (final)
//   s, s' <- the stored rows with the desired-goal columns replaced by g';  a, d verbatim
//   r    <- dist2 <= thr2 ? 0 : -1 (sparse) | -sqrtf(dist2) (dense),  dist2 = Σ_k (ag(s')_k - g'_k)^2, k in order
// with (r.x, r.y, r.z) the words of the ONE Philox call that draws the slot.  Every other row is k_replay_gather's.
//
// The shape is k_replay_gather's (replay.hip): 256 threads, 16 samples per workgroup, the episode table staged in LDS,
// rows staged in LDS and written coalesced.  t' is known from the draw, so there is no dependent second round of loads.
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
constexpr int kMaxG = oprl::kHerMaxGoal;          // one lane per (sample, goal element)
static_assert(kSamplesPerWg * kMaxG == kGatherThreads, "one (sample, goal element) pair per lane");

// Single IEEE operations, round to nearest, never contracted to FMA: the numpy oracle (tests/her_oracle.py) reproduces
// the distance bit for bit (replay_nstep.hip records why the pragma and not __fmul_rn).
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

struct HerArgs {
  const float *states, *actions, *rewards, *dones;
  const int* ends;  // cumulative episode ends, [n_eps]
  int n_eps, L, S, A, B;
  long n_transitions;
  const long long* idx;  // or null
  unsigned long long seed, counter;
  int ag_off, g_off, G, strategy, reward;
  float ratio, thr2;     // (float)ratio; (float)(threshold * threshold), squared on the host in double
  float *out_s, *out_a, *out_r, *out_d, *out_s2;
  int *out_ep, *out_step, *out_future;
};

__global__ __launch_bounds__(kGatherThreads) void k_replay_gather_her(const HerArgs G) {
  extern __shared__ float stage[];  // [kSamplesPerWg][2S + A + 2]: s | s' | a | r | d, k_replay_gather's layout
  __shared__ int s_ep[kSamplesPerWg], s_t[kSamplesPerWg], s_tp[kSamplesPerWg];   // s_tp: t', or -1 = not relabelled
  __shared__ float s_sq[kSamplesPerWg * kMaxG];     // fl(δ_k δ_k) of lane (sample, k)
  __shared__ int s_ends[kMaxEndsLds];
  const int tid = threadIdx.x;
  const oprl::EndsLds ET = oprl::stage_ends(G.ends, G.n_eps, s_ends, kMaxEndsLds, tid, kGatherThreads);
  __syncthreads();
  const int base = blockIdx.x * kSamplesPerWg;
  const int S = G.S, A = G.A, W = 2 * S + A + 2;
  if (tid < kSamplesPerWg) {
    const int i = base + tid;
    int e = 0, t = 0, tp = -1;
    if (i < G.B) {
      // the uniform sampler's draw, word for word: r.x picks the slot; r.y and r.z decide the relabelling, also when
      // the index is injected
      const oprl::u32x4 r = oprl::philox4x32_10(
          oprl::u32x4{(uint32_t)G.counter, (uint32_t)(G.counter >> 32), (uint32_t)i, 0x5a17u},
          (uint32_t)G.seed, (uint32_t)(G.seed >> 32));
      const long ind = G.idx != nullptr ? (long)G.idx[i] : (long)oprl::bounded_u32(r.x, (uint32_t)G.n_transitions);
      long start = 0;
      e = oprl::find_episode(G.ends, G.n_eps, ET, ind, &start);
      t = (int)(ind - start);
      const long end = ET.stride == 1 ? (long)ET.lds[e] : (long)G.ends[e];
      // later rows of this episode that are always written; an index past every end (the all-True argmin: e = 0,
      // t = ind >= every end) has c < 0 and stays the plain gather's row
      const long c = end - start - 1 - (long)t;
      const float U = (float)(r.y >> 8) * (1.0f / 16777216.0f);
      if (c >= 1 && U < G.ratio)
        tp = G.strategy == 0 ? t + (int)oprl::bounded_u32(r.z, (uint32_t)c) : (int)(end - start) - 2;
      if (G.out_ep != nullptr) G.out_ep[i] = e;
      if (G.out_step != nullptr) G.out_step[i] = t;
      if (G.out_future != nullptr) G.out_future[i] = tp;
    }
    s_ep[tid] = e;
    s_t[tid] = t;
    s_tp[tid] = tp;
  }
  __syncthreads();
  const int n_here = min(kSamplesPerWg, G.B - base);
  // Every load issued before the first LDS store, sources selected without branches (as in k_replay_gather).  Lane
  // (sample, k) takes element min(k, G - 1) of the achieved goals of s' and of states[e, t' + 1]; a row that is not
  // relabelled reads its own s' twice, so nothing outside the rows the plain gather reads is touched.
  const int smp_g = tid / kMaxG, k_g = min(tid % kMaxG, G.G - 1);
  const int tp_g = s_tp[smp_g];
  float ag, gp;
  {
    const long e = s_ep[smp_g], t = s_t[smp_g], tq = tp_g >= 0 ? tp_g : t;
    ag = G.states[(e * (G.L + 1) + t + 1) * S + G.ag_off + k_g];
    gp = G.states[(e * (G.L + 1) + tq + 1) * S + G.ag_off + k_g];
  }
  constexpr int kU = 4;
  for (int i0 = 0; i0 < n_here * W; i0 += kU * kGatherThreads) {
    float v[kU];
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      const int idx = min(i0 + j * kGatherThreads + tid, n_here * W - 1);
      const int smp = idx / W, c = idx - smp * W;
      const long e = s_ep[smp], t = s_t[smp];
      const float* src = G.states + (e * (G.L + 1) + t) * S + c;                       // s | s' contiguous
      if (c >= 2 * S) src = G.actions + (e * G.L + t) * A + (c - 2 * S);
      if (c == 2 * S + A) src = G.rewards + e * G.L + t;
      if (c == 2 * S + A + 1) src = G.dones + e * G.L + t;
      v[j] = *src;
    }
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      const int idx = i0 + j * kGatherThreads + tid;
      if (idx < n_here * W) stage[idx] = v[j];
    }
  }
  {
    const float dlt = sub_rn(ag, gp);
    s_sq[tid] = mul_rn(dlt, dlt);
  }
  __syncthreads();
  // Relabelled rows: lane (sample, k < G) puts g'_k over the desired goal of s and of s' in the stage, and one lane
  // per sample sums the squares in a fixed order and writes the reward over the stored one.
  if (smp_g < n_here && tp_g >= 0 && tid % kMaxG < G.G) {
    stage[smp_g * W + G.g_off + k_g] = gp;
    stage[smp_g * W + S + G.g_off + k_g] = gp;
  }
  if (tid < n_here && s_tp[tid] >= 0) {
    const float* sq = s_sq + tid * kMaxG;
    float dist2 = 0.f;
    for (int k = 0; k < G.G; ++k) dist2 = add_rn(dist2, sq[k]);
    stage[tid * W + 2 * S + A] = G.reward == 0 ? (dist2 <= G.thr2 ? 0.f : -1.f) : -sqrtf(dist2);
  }
  __syncthreads();
  for (int idx = tid; idx < n_here * S; idx += kGatherThreads) {
    const int smp = idx / S, c = idx - smp * S;
    G.out_s[(size_t)(base + smp) * S + c] = stage[smp * W + c];
    G.out_s2[(size_t)(base + smp) * S + c] = stage[smp * W + S + c];
  }
  for (int idx = tid; idx < n_here * A; idx += kGatherThreads) {
    const int smp = idx / A, c = idx - smp * A;
    G.out_a[(size_t)(base + smp) * A + c] = stage[smp * W + 2 * S + c];
  }
  if (tid < n_here) {
    G.out_r[base + tid] = stage[tid * W + 2 * S + A];
    G.out_d[base + tid] = stage[tid * W + 2 * S + A + 1];
  }
}

}  // namespace

namespace oprl {
int replay_her(const oprl_replay* h) { return h->her.G; }
}

extern "C" int oprl_replay_set_her(oprl_replay* h, int32_t ag_off, int32_t g_off, int32_t G, double ratio,
                                   int32_t strategy, int32_t reward, double threshold) {
  if (!h) { set_err("oprl_replay_set_her: null replay handle"); return OPRL_ERR_INVALID; }
  if (G == 0) { h->her = oprl::HerMode{}; return OPRL_OK; }      // the mode off: the other arguments are not read
  if (G < 1 || G > oprl::kHerMaxGoal) {
    set_err("oprl_replay_set_her: the goal dimension must lie in 1 .. %d, or be 0 to switch the mode off (got %d)", oprl::kHerMaxGoal, (int)G);
    return OPRL_ERR_INVALID;
  }
  const long S = h->S, a0 = ag_off, g0 = g_off;
  if (a0 < 0 || a0 + G > S || g0 < 0 || g0 + G > S) {
    set_err("oprl_replay_set_her: the achieved goal [%d, %d) and the desired goal [%d, %d) must lie inside the state row [0, %d)",
            (int)ag_off, (int)(a0 + G), (int)g_off, (int)(g0 + G), (int)S);
    return OPRL_ERR_INVALID;
  }
  if (a0 < g0 + G && g0 < a0 + G) {
    set_err("oprl_replay_set_her: the achieved goal [%d, %d) and the desired goal [%d, %d) overlap", (int)ag_off, (int)(a0 + G),
            (int)g_off, (int)(g0 + G));
    return OPRL_ERR_INVALID;
  }
  if (!(ratio >= 0.0) || !(ratio <= 1.0)) { set_err("oprl_replay_set_her: the relabelled share must lie in [0, 1] (got %g)", ratio); return OPRL_ERR_INVALID; }
  if (!(threshold >= 0.0) || !(threshold <= 1.7976931348623157e308)) {
    set_err("oprl_replay_set_her: the distance threshold must be finite and >= 0 (got %g)", threshold);
    return OPRL_ERR_INVALID;
  }
  if (strategy != 0 && strategy != 1) { set_err("oprl_replay_set_her: unknown strategy %d (0 = future, 1 = final)", (int)strategy); return OPRL_ERR_INVALID; }
  if (reward != 0 && reward != 1) { set_err("oprl_replay_set_her: unknown reward kind %d (0 = sparse, 1 = dense)", (int)reward); return OPRL_ERR_INVALID; }
  if (h->nstep > 1) {
    set_err("oprl_replay_set_her: this replay samples %d-step returns (oprl_replay_set_nstep); hindsight goals over n-step rows are not supported", h->nstep);
    return OPRL_ERR_STATE;
  }
  if (h->prio) {
    set_err("oprl_replay_set_her: this replay is prioritized; hindsight goals over the sum tree are not supported");
    return OPRL_ERR_STATE;
  }
  h->her = oprl::HerMode{(int)ag_off, (int)g_off, (int)G, (int)strategy, (int)reward, ratio, threshold};
  return OPRL_OK;
}

extern "C" int oprl_replay_sample_her(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed, uint64_t counter,
                                      float* out_s, float* out_a, float* out_r, float* out_d, float* out_s2,
                                      int32_t* out_ep, int32_t* out_step, int32_t* out_future, void* stream) {
  if (!h || B < 1 || !out_s || !out_a || !out_r || !out_d || !out_s2) {
    set_err("oprl_replay_sample_her: invalid argument");
    return OPRL_ERR_INVALID;
  }
  if (h->her.G < 1) {
    set_err("oprl_replay_sample_her: this replay has no goal layout (oprl_replay_set_her)");
    return OPRL_ERR_STATE;
  }
  if (h->n_transitions <= 0 || h->n_eps <= 0) {
    set_err("oprl_replay_sample_her: buffer is empty");
    return OPRL_ERR_STATE;
  }
  int rc = oprl_replay_flush(h, stream);
  if (rc != OPRL_OK) return rc;
  const oprl::HerMode& m = h->her;
  HerArgs G;
  G.states = h->states; G.actions = h->actions; G.rewards = h->rewards; G.dones = h->dones;
  G.ends = h->ends_dev; G.n_eps = h->n_eps; G.L = h->L; G.S = h->S; G.A = h->A; G.B = B;
  G.n_transitions = h->n_transitions;
  G.idx = (const long long*)idx; G.seed = seed; G.counter = counter;
  G.ag_off = m.ag_off; G.g_off = m.g_off; G.G = m.G; G.strategy = m.strategy; G.reward = m.reward;
  G.ratio = (float)m.ratio;
  G.thr2 = (float)(m.threshold * m.threshold);
  G.out_s = out_s; G.out_a = out_a; G.out_r = out_r; G.out_d = out_d; G.out_s2 = out_s2;
  G.out_ep = out_ep; G.out_step = out_step; G.out_future = out_future;
  const int grid = (B + kSamplesPerWg - 1) / kSamplesPerWg;
  const size_t lds = sizeof(float) * kSamplesPerWg * (2 * h->S + h->A + 2);
  oprl::prof_begin(2, (hipStream_t)stream);
  hipLaunchKernelGGL(k_replay_gather_her, dim3(grid), dim3(kGatherThreads), lds, (hipStream_t)stream, G);
  oprl::prof_end((hipStream_t)stream);
  HIPC(hipGetLastError());
  return OPRL_OK;
}
