// replay.hip — HBM-resident episodic replay: batched transition writes and the
// uniform sampler as a gather kernel.
//
// Reference: buffers/episodic_buffer.py
//   storage layout              :29-55   (states[E,L+1,S] actions[E,L,A] rewards/dones[E,L,1])
//   add_transition data movement:81-96
//   flat index -> (episode,step):114-121 (first episode whose cumulative end > index)
//   sample                      :123-133 (5 advanced-index gathers)
//
// Because states is [E, L+1, S], state (e,t) and next_state (e,t+1) are ADJACENT
// rows: one sample reads a single contiguous 2·S-float run, plus A + 1 + 1 floats.
// A workgroup stages 16 samples' rows in LDS and writes the five output arrays
// fully coalesced (the shape and its pieces: replay_gather.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/oprl_amd.h"
#include "replay_gather.h"

using namespace oprl;

namespace {

constexpr int kStageRows = 4096;      // transitions staged on the host between flushes

struct GatherArgs {
  GatherSrc src;
  GatherOut out;
};

__global__ __launch_bounds__(kGatherThreads) void k_replay_gather(const GatherArgs G) {
  extern __shared__ float stage[];  // [kSamplesPerWg][2S + A + 2]
  __shared__ int s_ep[kSamplesPerWg], s_t[kSamplesPerWg];
  __shared__ int s_ends[kMaxEndsLds];
  const int tid = threadIdx.x;
  // the episode table goes to LDS in one coalesced pass (whole, or every stride-th end: replay_index.h); a
  // binary search over global memory is 10+ dependent round trips to L2/HBM (measured 7.4 us for this kernel)
  const EndsLds ET = stage_ends(G.src.ends, G.src.n_eps, s_ends, kMaxEndsLds, tid, kGatherThreads);
  __syncthreads();
  const int base = blockIdx.x * kSamplesPerWg;
  const int S = G.src.S, A = G.src.A, W = 2 * S + A + 2;
  gather_slots(G.src, G.out, ET, base, s_ep, s_t, [](int, bool, const Slot&) {});
  __syncthreads();
  const int n_here = min(kSamplesPerWg, G.src.B - base);
  gather_stage_rows(G.src, n_here, s_ep, s_t, stage);
  __syncthreads();
  gather_write_rows(G.out, S, A, base, n_here, stage, W, S, 2 * S);
  gather_write_rd(G.out, base, n_here, stage + 2 * S + A, stage + 2 * S + A + 1, W);
}

// staged row: [ep, t] as two ints bit-cast into floats, then s[S], a[A], r, d
__device__ __forceinline__ void scatter_rows(const float* rows, int n, int rowlen, float* states, float* actions,
                                             float* rewards, float* dones, int L, int S, int A) {
  for (int rix = blockIdx.x; rix < n; rix += gridDim.x) {
    const float* row = rows + (size_t)rix * rowlen;
    const long e = __float_as_int(row[0]), t = __float_as_int(row[1]);
    for (int c = threadIdx.x; c < S + A + 2; c += blockDim.x) {
      const float v = row[2 + c];
      if (c < S) states[(e * (L + 1) + t) * S + c] = v;
      else if (c < S + A) actions[(e * L + t) * A + (c - S)] = v;
      else if (c == S + A) rewards[e * L + t] = v;
      else dones[e * L + t] = v;
    }
  }
}

__global__ void k_replay_scatter(const float* rows, int n, int rowlen, float* states,
                                 float* actions, float* rewards, float* dones, int L, int S,
                                 int A) {
  scatter_rows(rows, n, rowlen, states, actions, rewards, dones, L, S, A);
}

// The per-env-step form of the same (the trainer loop adds ONE transition between two updates): rows AND the changed
// tail of the episode-ends table straight from the pinned staging buffers (host-mapped: a few hundred bytes over the
// link inside the kernel) — one launch instead of two H2D copies and a scatter launch.
__global__ void k_replay_ingest(const float* rows, int n, int rowlen, float* states, float* actions, float* rewards,
                                float* dones, int L, int S, int A, const int* ends_src, int* ends_dst, int ends_first,
                                int ends_n) {
  scatter_rows(rows, n, rowlen, states, actions, rewards, dones, L, S, A);
  for (int i = ends_first + (int)(blockIdx.x * blockDim.x + threadIdx.x); i < ends_n; i += (int)(gridDim.x * blockDim.x))
    ends_dst[i] = ends_src[i];
}

}  // namespace

// (struct oprl_replay: replay_internal.h)

extern "C" int oprl_replay_create(int32_t n_episodes, int32_t max_ep_len, int32_t state_dim,
                                  int32_t action_dim, float* states, float* actions,
                                  float* rewards, float* dones, oprl_replay** out) {
  if (!out || n_episodes < 1 || max_ep_len < 1 || state_dim < 1 || action_dim < 1 || !states ||
      !actions || !rewards || !dones) {
    set_err("oprl_replay_create: invalid argument");
    return OPRL_ERR_INVALID;
  }
  auto* h = new oprl_replay();
  h->E = n_episodes; h->L = max_ep_len; h->S = state_dim; h->A = action_dim;
  h->states = states; h->actions = actions; h->rewards = rewards; h->dones = dones;
  h->rowlen = 2 + state_dim + action_dim + 2;
  HIPC(hipMalloc(&h->ends_dev, sizeof(int) * n_episodes));
  for (int i = 0; i < 2; ++i) {
    HIPC(hipHostMalloc(&h->stage_host[i], sizeof(float) * h->rowlen * kStageRows));
    HIPC(hipMalloc(&h->stage_dev[i], sizeof(float) * h->rowlen * kStageRows));
    HIPC(hipHostMalloc(&h->ends_host[i], sizeof(int) * n_episodes));
    HIPC(hipEventCreateWithFlags(&h->stage_ev[i], hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&h->ends_ev[i], hipEventDisableTiming));
    if (hipHostGetDevicePointer((void**)&h->stage_map[i], h->stage_host[i], 0) != hipSuccess) h->stage_map[i] = nullptr;
    if (hipHostGetDevicePointer((void**)&h->ends_map[i], h->ends_host[i], 0) != hipSuccess) h->ends_map[i] = nullptr;
  }
  (void)hipGetLastError();
  *out = h;
  return OPRL_OK;
}

extern "C" int oprl_replay_destroy(oprl_replay* h) {
  if (!h) return OPRL_OK;
  (void)hipDeviceSynchronize();
  oprl::prio_free(h->prio);
  oprl::rows_free(h);
  (void)hipFree(h->ends_dev);
  for (int i = 0; i < 2; ++i) {
    (void)hipHostFree(h->stage_host[i]);
    (void)hipFree(h->stage_dev[i]);
    (void)hipHostFree(h->ends_host[i]);
    (void)hipEventDestroy(h->stage_ev[i]);
    (void)hipEventDestroy(h->ends_ev[i]);
  }
  delete h;
  return OPRL_OK;
}

extern "C" int oprl_replay_flush(oprl_replay* h, void* stream) {
  if (!h) { set_err("null replay handle"); return OPRL_ERR_INVALID; }
  if (h->n_staged == 0 && !h->ends_pending && !(h->prio && h->prio->n_eps != h->n_eps)) return OPRL_OK;
  hipStream_t st = (hipStream_t)stream;
  const int c = h->cur, n = h->n_staged, ec = h->ends_cur;
  const PendingEnds pe = pending_ends(h, n, h->stage_map[c], h->ends_map[ec]);
  const int e_first = pe.first, e_n = pe.n;
  const bool direct = pe.direct;
  if (direct) {
    const int wgs = n > 0 ? n : 1;
    hipLaunchKernelGGL(k_replay_ingest, dim3(wgs), dim3(64), 0, st, h->stage_map[c], n, h->rowlen, h->states, h->actions,
                       h->rewards, h->dones, h->L, h->S, h->A, h->ends_map[ec], h->ends_dev, e_first, e_n);
    HIPC(hipGetLastError());
  } else {
    if (n > 0) {
      HIPC(hipMemcpyAsync(h->stage_dev[c], h->stage_host[c], sizeof(float) * h->rowlen * n, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_replay_scatter, dim3(n < 1024 ? n : 1024), dim3(64), 0, st,
                         h->stage_dev[c], n, h->rowlen, h->states, h->actions, h->rewards, h->dones,
                         h->L, h->S, h->A);
      HIPC(hipGetLastError());
    }
    if (e_n > e_first)
      HIPC(hipMemcpyAsync(h->ends_dev + e_first, h->ends_host[ec] + e_first, sizeof(int) * (e_n - e_first),
                          hipMemcpyHostToDevice, st));
  }
  if (h->prio) {       // the sum tree of prioritized replay follows the rows and the table (replay_prio.hip)
    const float* rows = n > 0 ? (direct ? h->stage_map[c] : h->stage_dev[c]) : nullptr;
    int rc = oprl::prio_flush(h, rows, n, h->rowlen, e_first, e_n, st);
    if (rc != OPRL_OK) return rc;
  }
  if (n > 0) {
    HIPC(hipEventRecord(h->stage_ev[c], st));
    h->stage_busy[c] = true;
    h->cur ^= 1;
    h->n_staged = 0;
    if (h->stage_busy[h->cur]) {  // the other buffer must have drained before we refill it
      HIPC(hipEventSynchronize(h->stage_ev[h->cur]));
      h->stage_busy[h->cur] = false;
    }
  }
  return oprl::ends_sent(h, st);
}

namespace oprl {
PendingEnds pending_ends(const oprl_replay* h, int n_rows, const float* rows_map, const int* ends_map) {
  PendingEnds p;
  p.first = h->ends_pending ? h->ends_first : 0;
  p.n = h->ends_pending ? h->ends_n : 0;
  p.direct = n_rows <= kDirectRows && p.n - p.first <= kDirectEnds && rows_map != nullptr && ends_map != nullptr;
  return p;
}

int ends_sent(oprl_replay* h, hipStream_t st) {
  if (h->ends_pending) {
    const int ec = h->ends_cur;
    HIPC(hipEventRecord(h->ends_ev[ec], st));
    h->ends_busy[ec] = true;
    h->ends_cur ^= 1;
    h->ends_pending = false;
  }
  return OPRL_OK;
}

int check_lens(const oprl_replay* h, const int32_t* ep_lens_host, int32_t episodes_counter, const char* who) {
  if (!h || !ep_lens_host || episodes_counter < 0 || episodes_counter > h->E) {
    set_err("%s: invalid argument", who);
    return OPRL_ERR_INVALID;
  }
  for (int i = 0; i < episodes_counter; ++i)
    if (ep_lens_host[i] < 0 || ep_lens_host[i] > h->L) { set_err("ep_lens[%d]=%d out of range", i, ep_lens_host[i]); return OPRL_ERR_INVALID; }
  return OPRL_OK;
}
}  // namespace oprl

extern "C" int oprl_replay_write(oprl_replay* h, int32_t ep, int32_t t, const float* state_host,
                                 const float* action_host, float reward, float done) {
  if (!h || !state_host || !action_host) { set_err("oprl_replay_write: null argument"); return OPRL_ERR_INVALID; }
  if (ep < 0 || ep >= h->E || t < 0 || t >= h->L) {
    set_err("oprl_replay_write: slot (%d,%d) outside [%d,%d)", ep, t, h->E, h->L);
    return OPRL_ERR_INVALID;
  }
  if (h->n_staged == kStageRows) {
    // staging is full and this entry point has no stream argument: the scatter goes on the null stream and is
    // WAITED for — no stream handle of an earlier call is kept (it may have been destroyed, or not be the stream of the
    // next sample), and whatever stream that sample runs on finds the rows in HBM.  Once per kStageRows writes.
    int rc = oprl_replay_flush(h, nullptr);
    if (rc != OPRL_OK) return rc;
    HIPC(hipStreamSynchronize(nullptr));
  }
  float* row = h->stage_host[h->cur] + (size_t)h->n_staged * h->rowlen;
  memcpy(row, &ep, 4);
  memcpy(row + 1, &t, 4);
  memcpy(row + 2, state_host, sizeof(float) * h->S);
  memcpy(row + 2 + h->S, action_host, sizeof(float) * h->A);
  row[2 + h->S + h->A] = reward;
  row[3 + h->S + h->A] = done;
  ++h->n_staged;
  return OPRL_OK;
}

// The trainer loop's add_transition as ONE call: stage the row, take the episode table, and put both on their way
// (oprl_replay_write + oprl_replay_set_lens + oprl_replay_flush).
extern "C" int oprl_replay_write_flush(oprl_replay* h, int32_t ep, int32_t t, const float* state_host,
                                       const float* action_host, float reward, float done, const int32_t* ep_lens_host,
                                       int32_t episodes_counter, void* stream) {
  int rc = oprl_replay_write(h, ep, t, state_host, action_host, reward, done);
  if (rc != OPRL_OK) return rc;
  rc = oprl_replay_set_lens(h, ep_lens_host, episodes_counter, stream);
  if (rc != OPRL_OK) return rc;
  return oprl_replay_flush(h, stream);
}

// n consecutive steps [t0, t0 + n) of episode `ep` from host records [s (S) | a (A) | r | d | ...] that are
// `row_stride` floats apart — a whole episode (or a drained ring segment) in ONE call instead of n
// oprl_replay_write calls (the learner ranks of the distributed setup take in tens of thousands of
// transitions per second).  Staging that fills up is flushed on `stream`.
extern "C" int oprl_replay_write_block(oprl_replay* h, int32_t ep, int32_t t0, int32_t n, const float* rows_host,
                                       int32_t row_stride, void* stream) {
  if (!h || !rows_host || n < 0) { set_err("oprl_replay_write_block: invalid argument"); return OPRL_ERR_INVALID; }
  if (ep < 0 || ep >= h->E || t0 < 0 || t0 + n > h->L || row_stride < h->S + h->A + 2) {
    set_err("oprl_replay_write_block: steps [%d,%d) of episode %d outside [%d,%d) x [0,%d) or stride %d too small",
            t0, t0 + n, ep, 0, h->E, h->L, row_stride);
    return OPRL_ERR_INVALID;
  }
  for (int i = 0; i < n; ++i) {
    if (h->n_staged == kStageRows) {
      int rc = oprl_replay_flush(h, stream);
      if (rc != OPRL_OK) return rc;
    }
    float* row = h->stage_host[h->cur] + (size_t)h->n_staged * h->rowlen;
    const int t = t0 + i;
    memcpy(row, &ep, 4);
    memcpy(row + 1, &t, 4);
    memcpy(row + 2, rows_host + (size_t)i * row_stride, sizeof(float) * (h->S + h->A + 2));
    ++h->n_staged;
  }
  return OPRL_OK;
}

extern "C" int oprl_replay_set_lens(oprl_replay* h, const int32_t* ep_lens_host,
                                    int32_t episodes_counter, void* stream) {
  (void)stream;      // (the table goes up with the next flush — every reader flushes first — on ITS stream)
  // validate the whole table BEFORE touching the mirrors: a bad entry midway must not leave ends_last ahead of what
  // the device holds (the next valid call would then see "no difference" and never upload those entries)
  const int ok = oprl::check_lens(h, ep_lens_host, episodes_counter, "oprl_replay_set_lens");
  if (ok != OPRL_OK) return ok;
  const int c = h->ends_cur;
  if (!h->ends_pending && h->ends_busy[c]) { HIPC(hipEventSynchronize(h->ends_ev[c])); h->ends_busy[c] = false; }
  long acc = 0;
  int first = -1;
  if ((int)h->ends_last.size() < episodes_counter) h->ends_last.resize(episodes_counter, -1);
  for (int i = 0; i < episodes_counter; ++i) {
    acc += ep_lens_host[i];
    h->ends_host[c][i] = (int)acc;
    if (h->ends_last[i] != (int)acc) {
      if (first < 0) first = i;
      h->ends_last[i] = (int)acc;
    }
  }
  if (first >= 0) {
    h->ends_first = h->ends_pending ? (first < h->ends_first ? first : h->ends_first) : first;
    h->ends_n = h->ends_pending ? (episodes_counter > h->ends_n ? episodes_counter : h->ends_n) : episodes_counter;
    h->ends_pending = true;
  }
  h->n_eps = episodes_counter;
  h->n_transitions = acc;
  return OPRL_OK;
}

extern "C" int oprl_replay_sample(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed,
                                  uint64_t counter, float* out_s, float* out_a, float* out_r,
                                  float* out_d, float* out_s2, int32_t* out_ep, int32_t* out_step,
                                  void* stream) {
  RC(gather_check("oprl_replay_sample", h, B, out_s, out_a, out_r, out_d, out_s2));
  if (h->nstep > 1)      // n-step mode (oprl_replay_set_nstep): the same draw, n-step rows (replay_nstep.hip)
    return oprl_replay_sample_nstep(h, B, idx, seed, counter, out_s, out_a, out_r, out_d, out_s2, out_ep, out_step, nullptr, stream);
  if (h->her.G > 0)      // hindsight mode (oprl_replay_set_her): the same draw, relabelled rows (replay_her.hip)
    return oprl_replay_sample_her(h, B, idx, seed, counter, out_s, out_a, out_r, out_d, out_s2, out_ep, out_step, nullptr, stream);
  if (h->prior)          // prior-data mode (oprl_replay_set_prior): the same draw, over two replays (replay_mix.hip)
    return oprl_replay_sample_mix(h, B, idx, seed, counter, out_s, out_a, out_r, out_d, out_s2, out_ep, out_step, nullptr, stream);
  GatherArgs G;
  gather_fill(h, B, idx, seed, counter, out_s, out_a, out_r, out_d, out_s2, out_ep, out_step, &G.src, &G.out);
  return gather_launch("oprl_replay_sample: buffer is empty (np.random.randint(0, 0) raises in the reference)",
                       k_replay_gather, G, 2 * h->S + h->A + 2, h, stream);
}

// used by the learner's fused step_n
namespace oprl {
int replay_dims(const oprl_replay* h, int* S, int* A) { *S = h->S; *A = h->A; return 0; }
// raw view for kernels that gather in-place (fused_ddpg.hip)
int replay_view(const oprl_replay* h, const float** states, const float** actions,
                const float** rewards, const float** dones, const int** ends, int* n_eps, int* L,
                long* n_transitions) {
  *states = h->states; *actions = h->actions; *rewards = h->rewards; *dones = h->dones;
  *ends = h->ends_dev; *n_eps = h->n_eps; *L = h->L; *n_transitions = h->n_transitions;
  return 0;
}
// n-step mode of the handle (replay_nstep.hip): *n > 1 when oprl_replay_sample gathers n-step rows with *gamma
int replay_nstep(const oprl_replay* h, int* n, double* gamma) { *n = h->nstep; *gamma = h->nstep_gamma; return 0; }
}
