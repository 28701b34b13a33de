// replay_returns.hip — discounted returns-to-go of sampled slots out of the HBM episodic replay: the one
// per-row quantity beyond (s, a, r, d, s') that calibrated Q-learning needs (Nakamoto et al., "Cal-QL: Calibrated Offline
// RL Pre-Training for Efficient Online Fine-Tuning", NeurIPS 2023).
//
// Reference: none (the reference's buffer stores no returns).  For row i with the slot (e, t) = (ep[i], step[i]) inside
// the row's source — the handle, or for i < B_p its prior (replay_mix.hip: the split is by row index) —
//   len_e = the episode's stored steps from the source's ends table, the in-progress tail included
//   T     = the first k >= t with dones[e, k] != 0, or len_e - 1 if there is none
//   G_i   = sum_{k = t .. T} gamma^(k - t) rewards[e, k]
// with no bootstrap at a truncation (a timeout, a dataset piece cut at L, an episode still running): the sum ends at the
// last stored step.  t >= len_e (the sampler's one corner) gives the single term rewards[e, t]; a slot
// outside [0, E) x [0, L) reads nothing and gives 0.
//
// One wave per row.  The wave sweeps the tail [t, len_e) in chunks of 64 steps: coalesced loads of rewards and dones, the
// first non-zero done by ballot, lane l's term pw[l] r_l (pw[l] = (float)pow((double)gamma, l), formed on the host as
// replay_nstep.hip forms its table), the chunk's sum by the xor butterfly of the seed kernels (masks 1, 2, .. 32), and
//   G <- G + f_c S_c,   f_0 = 1,  f_{c+1} = f_c pw[64]
// chunk after chunk, every operation a single mul_rn / add_rn (replay_gather.h): the order is the definition, and
// tests/calql_oracle.py restates it in numpy float32 bit for bit.  Plain C++: vector stores only, no atomics, no inline
// assembly, nothing written for rows >= B.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/oprl_amd.h"
#include "replay_gather.h"

using namespace oprl;

namespace {

constexpr int kWave = 64;
constexpr int kReturnsWaves = 4;                      // rows per workgroup
constexpr int kReturnsThreads = kWave * kReturnsWaves;
constexpr int kAhead = 4;                             // chunks whose loads are in flight together

struct ReturnsSrc {
  const float *rewards, *dones;
  const int* ends;      // cumulative episode ends, [n_eps]
  int n_eps, E, L;
};

struct ReturnsArgs {
  ReturnsSrc prior, own;  // rows [0, Bp) read `prior`, rows [Bp, B) read `own`
  int Bp, B;
  const int *ep, *step;   // [B] the rows' slots inside their sources
  float pw[kWave + 1];    // (float)pow((double)gamma, l), l = 0 .. 64
  float* out_g;           // [B]
};

__global__ __launch_bounds__(kReturnsThreads) void k_replay_returns(const ReturnsArgs K) {
  __shared__ float s_pw[kWave + 1];                   // (a lane indexes the powers by its own number)
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  if (tid <= kWave) s_pw[tid] = K.pw[tid];
  __syncthreads();
  const int row = (int)blockIdx.x * kReturnsWaves + tid / kWave;      // uniform in the wave
  if (row >= K.B) return;
  const bool p = row < K.Bp;
  const float* rewards = p ? K.prior.rewards : K.own.rewards;
  const float* dones = p ? K.prior.dones : K.own.dones;
  const int* ends = p ? K.prior.ends : K.own.ends;
  const int n_eps = p ? K.prior.n_eps : K.own.n_eps, E = p ? K.prior.E : K.own.E, L = p ? K.prior.L : K.own.L;
  const int e = K.ep[row], t = K.step[row];
  if (e < 0 || e >= E || t < 0 || t >= L) {           // caller-supplied: nothing is read for it
    if (lane == 0) K.out_g[row] = 0.f;
    return;
  }
  int len = 0;
  if (e < n_eps) len = ends[e] - (e > 0 ? ends[e - 1] : 0);
  len = min(max(len, 0), L);
  const int n = max(len - t, 1);                      // the tail's steps; t >= len_e: the one stored at (e, t)
  const long base = (long)e * L + t;
  const float pwl = s_pw[lane], pw64 = s_pw[kWave];
  float g = 0.f, f = 1.f;
  bool over = false;
  // kAhead chunks' loads are issued before the first of them is summed: the sweep is a chain of dependent round trips
  // (load, ballot, butterfly), 16 of them at a full tail of 1000 steps, and a chunk behind the done costs two loads nobody
  // reads.  The sums keep the chunks' order.
  for (int c0 = 0; c0 < n && !over; c0 += kAhead * kWave) {
    float r[kAhead], d[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {                // (branch-free, a clamped index: a load under a condition is a load and
      const int k = min(c0 + j * kWave + lane, n - 1);    //  a wait of its own; what a lane past the tail loads is not used)
      r[j] = rewards[base + k];
      d[j] = dones[base + k];
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      // a chunk behind the done or past the tail is not `live`: it is summed like the others — no branch, or the
      // compiler sinks its loads into it — and G keeps its bits
      const bool live = !over && c0 + j * kWave < n;  // (uniform in the wave)
      const bool in = live && c0 + j * kWave + lane < n;
      const unsigned long long ended = __ballot(in && d[j] != 0.f);
      const int last = ended != 0ull ? __ffsll((long long)ended) - 1 : kWave - 1;    // the chunk's last lane that counts
      float v = in && lane <= last ? mul_rn(pwl, r[j]) : 0.f;
#pragma unroll
      for (int mm = 1; mm < kWave; mm <<= 1) v = add_rn(v, __shfl_xor(v, mm));
      const float g1 = add_rn(g, mul_rn(f, v));
      g = live ? g1 : g;
      over = over || ended != 0ull;
      f = mul_rn(f, pw64);
    }
  }
  if (lane == 0) K.out_g[row] = g;
}

// what keeps a source's stored rewards from meaning a return; null: nothing
const char* no_returns(const oprl_replay* r) {
  if (r->her.G > 0) return "relabels goals in hindsight (oprl_replay_set_her): its rewards are relabelled per sample, a stored return means nothing";
  return nullptr;
}

ReturnsSrc returns_src(const oprl_replay* r) { return ReturnsSrc{r->rewards, r->dones, r->ends_dev, r->n_eps, r->E, r->L}; }

}  // namespace

extern "C" int oprl_replay_returns(oprl_replay* h, int32_t B, const int32_t* ep, const int32_t* step, double gamma,
                                   float* out_g, void* stream) {
  if (!h || !ep || !step || !out_g) { set_err("oprl_replay_returns: null argument"); return OPRL_ERR_INVALID; }
  if (B < 1 || !(gamma > 0.0) || !(gamma <= 1.0)) {
    set_err("oprl_replay_returns: need B >= 1 and 0 < gamma <= 1 (got B = %d, gamma = %g)", (int)B, gamma);
    return OPRL_ERR_INVALID;
  }
  oprl_replay* p = h->prior;
  const int Bp = p ? prior_rows(B, h->prior_share) : 0;
  if (const char* why = no_returns(h)) { set_err("oprl_replay_returns: this replay %s", why); return OPRL_ERR_STATE; }
  if (p)
    if (const char* why = no_returns(p)) { set_err("oprl_replay_returns: the prior replay %s", why); return OPRL_ERR_STATE; }
  if (Bp > 0 && (p->n_transitions <= 0 || p->n_eps <= 0)) {
    set_err("oprl_replay_returns: the prior replay is empty and has to supply %d of the %d rows", Bp, (int)B);
    return OPRL_ERR_STATE;
  }
  if (Bp < B && (h->n_transitions <= 0 || h->n_eps <= 0)) {
    set_err("oprl_replay_returns: this replay is empty and has to supply %d of the %d rows", (int)B - Bp, (int)B);
    return OPRL_ERR_STATE;
  }
  ReturnsArgs K;
  K.own = returns_src(h);
  K.prior = p ? returns_src(p) : K.own;
  K.Bp = Bp; K.B = B;
  K.ep = ep; K.step = step;
  for (int l = 0; l <= kWave; ++l) K.pw[l] = (float)pow(gamma, (double)l);
  K.out_g = out_g;
  if (p) RC(oprl_replay_flush(p, stream));
  RC(oprl_replay_flush(h, stream));
  prof_begin(2, (hipStream_t)stream);
  hipLaunchKernelGGL(k_replay_returns, dim3((B + kReturnsWaves - 1) / kReturnsWaves), dim3(kReturnsThreads), 0,
                     (hipStream_t)stream, K);
  prof_end((hipStream_t)stream);
  HIPC(hipGetLastError());
  return OPRL_OK;
}
