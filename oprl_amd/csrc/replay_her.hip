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
// The shape is the gather kernels' (replay_gather.h): the slot phase, the stage copy and the write-back are the shared
// ones.  t' is known from the draw, so there is no dependent second round of loads.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/oprl_amd.h"
#include "replay_gather.h"

using namespace oprl;

namespace {

constexpr int kMaxG = kHerMaxGoal;                // one lane per (sample, goal element)
static_assert(kSamplesPerWg * kMaxG == kGatherThreads, "one (sample, goal element) pair per lane");

struct HerArgs {
  GatherSrc src;
  int ag_off, g_off, G, strategy, reward;
  float ratio, thr2;     // (float)ratio; (float)(threshold * threshold), squared on the host in double
  GatherOut out;
  int* out_future;
};

__global__ __launch_bounds__(kGatherThreads) void k_replay_gather_her(const HerArgs K) {
  extern __shared__ float stage[];  // [kSamplesPerWg][2S + A + 2]: s | s' | a | r | d, k_replay_gather's layout
  __shared__ int s_ep[kSamplesPerWg], s_t[kSamplesPerWg], s_tp[kSamplesPerWg];   // s_tp: t', or -1 = not relabelled
  __shared__ float s_sq[kSamplesPerWg * kMaxG];     // fl(δ_k δ_k) of lane (sample, k)
  __shared__ int s_ends[kMaxEndsLds];
  const GatherSrc& G = K.src;
  const int tid = threadIdx.x;
  const EndsLds ET = stage_ends(G.ends, G.n_eps, s_ends, kMaxEndsLds, tid, kGatherThreads);
  __syncthreads();
  const int base = blockIdx.x * kSamplesPerWg;
  const int S = G.S, A = G.A, W = 2 * S + A + 2;
  // r.x picked the slot; r.y and r.z decide the relabelling, also when the index is injected (kAlwaysDraw)
  gather_slots<true>(G, K.out, ET, base, s_ep, s_t, [&](int i, bool live, const Slot& sl) {
    int tp = -1;
    if (live) {
      // later rows of this episode that are always written; an index past every end (the all-True argmin: e = 0,
      // t = ind >= every end) has c < 0 and stays the plain gather's row
      const long c = sl.end - sl.start - 1 - (long)sl.t;
      const float U = (float)(sl.r.y >> 8) * (1.0f / 16777216.0f);
      if (c >= 1 && U < K.ratio)
        tp = K.strategy == 0 ? sl.t + (int)bounded_u32(sl.r.z, (uint32_t)c) : (int)(sl.end - sl.start) - 2;
      if (K.out_future != nullptr) K.out_future[i] = tp;
    }
    s_tp[tid] = tp;
  });
  __syncthreads();
  const int n_here = min(kSamplesPerWg, G.B - base);
  // Every load issued before the first LDS store, sources selected without branches (as in k_replay_gather).  Lane
  // (sample, k) takes element min(k, G - 1) of the achieved goals of s' and of states[e, t' + 1]; a row that is not
  // relabelled reads its own s' twice, so nothing outside the rows the plain gather reads is touched.
  const int smp_g = tid / kMaxG, k_g = min(tid % kMaxG, K.G - 1);
  const int tp_g = s_tp[smp_g];
  float ag, gp;
  {
    const long e = s_ep[smp_g], t = s_t[smp_g], tq = tp_g >= 0 ? tp_g : t;
    ag = G.states[(e * (G.L + 1) + t + 1) * S + K.ag_off + k_g];
    gp = G.states[(e * (G.L + 1) + tq + 1) * S + K.ag_off + k_g];
  }
  gather_stage_rows(G, n_here, s_ep, s_t, stage);
  {
    const float dlt = sub_rn(ag, gp);
    s_sq[tid] = mul_rn(dlt, dlt);
  }
  __syncthreads();
  // Relabelled rows: lane (sample, k < G) puts g'_k over the desired goal of s and of s' in the stage, and one lane
  // per sample sums the squares in a fixed order and writes the reward over the stored one.
  if (smp_g < n_here && tp_g >= 0 && tid % kMaxG < K.G) {
    stage[smp_g * W + K.g_off + k_g] = gp;
    stage[smp_g * W + S + K.g_off + k_g] = gp;
  }
  if (tid < n_here && s_tp[tid] >= 0) {
    const float* sq = s_sq + tid * kMaxG;
    float dist2 = 0.f;
    for (int k = 0; k < K.G; ++k) dist2 = add_rn(dist2, sq[k]);
    stage[tid * W + 2 * S + A] = K.reward == 0 ? (dist2 <= K.thr2 ? 0.f : -1.f) : -sqrtf(dist2);
  }
  __syncthreads();
  gather_write_rows(K.out, S, A, base, n_here, stage, W, S, 2 * S);
  gather_write_rd(K.out, base, n_here, stage + 2 * S + A, stage + 2 * S + A + 1, W);
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
  if (h->prior) {
    set_err("oprl_replay_set_her: this replay mixes prior data into its batches (oprl_replay_set_prior); hindsight goals over mixed batches are not supported");
    return OPRL_ERR_STATE;
  }
  h->her = oprl::HerMode{(int)ag_off, (int)g_off, (int)G, (int)strategy, (int)reward, ratio, threshold};
  return OPRL_OK;
}

extern "C" int oprl_replay_sample_her(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed, uint64_t counter,
                                      float* out_s, float* out_a, float* out_r, float* out_d, float* out_s2,
                                      int32_t* out_ep, int32_t* out_step, int32_t* out_future, void* stream) {
  RC(gather_check("oprl_replay_sample_her", h, B, out_s, out_a, out_r, out_d, out_s2));
  if (h->her.G < 1) {
    set_err("oprl_replay_sample_her: this replay has no goal layout (oprl_replay_set_her)");
    return OPRL_ERR_STATE;
  }
  const HerMode& m = h->her;
  HerArgs K;
  gather_fill(h, B, idx, seed, counter, out_s, out_a, out_r, out_d, out_s2, out_ep, out_step, &K.src, &K.out);
  K.ag_off = m.ag_off; K.g_off = m.g_off; K.G = m.G; K.strategy = m.strategy; K.reward = m.reward;
  K.ratio = (float)m.ratio;
  K.thr2 = (float)(m.threshold * m.threshold);
  K.out_future = out_future;
  return gather_launch("oprl_replay_sample_her: buffer is empty", k_replay_gather_her, K, 2 * h->S + h->A + 2, h, stream);
}
