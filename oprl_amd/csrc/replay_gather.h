// replay_gather.h — what the gather kernels of the replay sampler share: k_replay_gather (replay.hip),
// k_replay_gather_nstep (replay_nstep.hip), k_replay_gather_her (replay_her.hip) and k_replay_gather_mix (replay_mix.hip).
//
// One shape for all of them: 256 threads and 16 samples per workgroup; the episode table staged in LDS
// (replay_index.h); lanes < 16 draw their sample's slot (e, t) into s_ep / s_t; the rows go to an LDS stage and from
// there, coalesced, to the five outputs.  The pieces below are that shape — every one __forceinline__, so a kernel is
// the code it would be with the pieces written out — and the host side of it: the kernels' common arguments, the
// argument check, and the launcher (empty-buffer refusal, flush, grid and LDS sizing, profiled launch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "replay_index.h"
#include "replay_internal.h"

namespace oprl {

constexpr int kGatherThreads = 256;
constexpr int kSamplesPerWg = 16;     // more workgroups, one copy round per thread at walker dims
constexpr int kMaxEndsLds = 2048;     // episode-end table entries staged in LDS by the gather

struct GatherSrc {
  const float *states, *actions, *rewards, *dones;
  const int* ends;  // cumulative episode ends, [n_eps]
  int n_eps, L, S, A, B;
  long n_transitions;
  const long long* idx;  // or null
  unsigned long long seed, counter;
};
struct GatherOut {
  float *s, *a, *r, *d, *s2;
  int *ep, *step;        // or null
};

// The kernels' common arguments from the handle.  The entry points call this before gather_launch flushes: a flush
// moves rows and table entries to the device and must not change ends_dev, n_eps or n_transitions (set_lens does).
inline void gather_fill(const oprl_replay* h, int B, const int64_t* idx, uint64_t seed, uint64_t counter, float* out_s,
                        float* out_a, float* out_r, float* out_d, float* out_s2, int32_t* out_ep, int32_t* out_step,
                        GatherSrc* src, GatherOut* out) {
  *src = GatherSrc{h->states, h->actions, h->rewards, h->dones, h->ends_dev, h->n_eps, h->L, h->S, h->A, B,
                   h->n_transitions, (const long long*)idx, seed, counter};
  *out = GatherOut{out_s, out_a, out_r, out_d, out_s2, out_ep, out_step};
}

// Single IEEE operations, round to nearest, never contracted to FMA: the numpy oracles (tests/nstep_oracle.py,
// tests/her_oracle.py) reproduce the sums bit for bit.  (__fmul_rn / __fadd_rn are plain operators in hipcc's headers
// and contract once inlined; the pragma takes the `contract` flag off these operations.)
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

// The slot phase, after stage_ends' barrier: lane tid < kSamplesPerWg draws row base + tid (replay_index.h draw_slot),
// leaves (e, t) in s_ep / s_t and in the optional ep / step outputs, and hands the slot to mode(i, live, slot) for what
// the kernel's mode derives from it.  A lane past the batch (live = false) gets the all-zero slot.
template <bool kAlwaysDraw = false, class Mode>
__device__ __forceinline__ void gather_slots(const GatherSrc& G, const GatherOut& O, const EndsLds& ET, int base,
                                             int* s_ep, int* s_t, Mode&& mode) {
  const int tid = threadIdx.x;
  if (tid >= kSamplesPerWg) return;
  const int i = base + tid;
  const bool live = i < G.B;
  Slot sl{};
  if (live) {
    sl = draw_slot<kAlwaysDraw>(G.ends, ET, G.n_eps, G.n_transitions, G.seed, G.counter, i, G.idx);
    if (O.ep != nullptr) O.ep[i] = sl.e;
    if (O.step != nullptr) O.step[i] = sl.t;
  }
  s_ep[tid] = sl.e;
  s_t[tid] = sl.t;
  mode(i, live, sl);
}

// Rows -> LDS: stage[kSamplesPerWg][W = 2S + A + 2] = s | s' | a | r | d of the n_here slots in s_ep / s_t (s and s'
// are adjacent rows of states[E, L+1, S]).  Branch-free source selection and all of a thread's loads issued before its
// LDS stores: an if/else per kind (s|s', a, r, d) diverges inside a wave and turns the copy into several serialised
// load -> wait -> store round trips (the kernel is pure latency: 8.5 us at B = 256 before).
__device__ __forceinline__ void gather_stage_rows(const GatherSrc& G, int n_here, const int* s_ep, const int* s_t,
                                                  float* stage) {
  const int tid = threadIdx.x, S = G.S, A = G.A, W = 2 * S + A + 2;
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
}

// The same copy for a workgroup whose samples [0, split) lie in P and [split, n_here) in O (k_replay_gather_mix,
// replay_mix.hip): the sample's source selects the base pointers and L — selects, no branch — and S and A are common
// to the two.  Beside gather_stage_rows, not in it: the three kernels above keep their code.
__device__ __forceinline__ void gather_stage_rows_mix(const GatherSrc& P, const GatherSrc& O, int split, int n_here,
                                                      const int* s_ep, const int* s_t, float* stage) {
  const int tid = threadIdx.x, S = O.S, A = O.A, W = 2 * S + A + 2;
  constexpr int kU = 4;
  for (int i0 = 0; i0 < n_here * W; i0 += kU * kGatherThreads) {
    float v[kU];
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      const int idx = min(i0 + j * kGatherThreads + tid, n_here * W - 1);
      const int smp = idx / W, c = idx - smp * W;
      const bool p = smp < split;
      const long e = s_ep[smp], t = s_t[smp], L = p ? P.L : O.L;
      const float* src = (p ? P.states : O.states) + (e * (L + 1) + t) * S + c;         // s | s' contiguous
      if (c >= 2 * S) src = (p ? P.actions : O.actions) + (e * L + t) * A + (c - 2 * S);
      if (c == 2 * S + A) src = (p ? P.rewards : O.rewards) + e * L + t;
      if (c == 2 * S + A + 1) src = (p ? P.dones : O.dones) + e * L + t;
      v[j] = *src;
    }
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      const int idx = i0 + j * kGatherThreads + tid;
      if (idx < n_here * W) stage[idx] = v[j];
    }
  }
}

// Stage -> outputs, coalesced: s at column 0 of a W-float stage row, s' at off_s2, a at off_a ...
__device__ __forceinline__ void gather_write_rows(const GatherOut& O, int S, int A, int base, int n_here,
                                                  const float* stage, int W, int off_s2, int off_a) {
  const int tid = threadIdx.x;
  for (int idx = tid; idx < n_here * S; idx += kGatherThreads) {
    const int smp = idx / S, c = idx - smp * S;
    O.s[(size_t)(base + smp) * S + c] = stage[smp * W + c];
    O.s2[(size_t)(base + smp) * S + c] = stage[smp * W + off_s2 + c];
  }
  for (int idx = tid; idx < n_here * A; idx += kGatherThreads) {
    const int smp = idx / A, c = idx - smp * A;
    O.a[(size_t)(base + smp) * A + c] = stage[smp * W + off_a + c];
  }
}
// ... and r / d of sample j from r[j * stride] / d[j * stride]: the stage row's last two columns, or per-sample arrays
__device__ __forceinline__ void gather_write_rd(const GatherOut& O, int base, int n_here, const float* r,
                                                const float* d, int stride) {
  const int tid = threadIdx.x;
  if (tid < n_here) {
    O.r[base + tid] = r[tid * stride];
    O.d[base + tid] = d[tid * stride];
  }
}

// ---- host: the front and the back of oprl_replay_sample / _sample_nstep / _sample_her --------------------------------
inline int gather_check(const char* who, const oprl_replay* h, int32_t B, const float* out_s, const float* out_a,
                        const float* out_r, const float* out_d, const float* out_s2) {
  if (!h || B < 1 || !out_s || !out_a || !out_r || !out_d || !out_s2) {
    set_err("%s: invalid argument", who);
    return OPRL_ERR_INVALID;
  }
  return OPRL_OK;
}

// G: filled (gather_fill() and the mode's own fields); `empty`: what an empty buffer is refused with; row_floats: the width
// of a sample's row in the kernel's LDS stage
template <class Args>
int gather_launch(const char* empty, void (*kernel)(const Args), const Args& G, int row_floats, oprl_replay* h,
                  void* stream) {
  if (h->n_transitions <= 0 || h->n_eps <= 0) {
    set_err("%s", empty);
    return OPRL_ERR_STATE;
  }
  RC(oprl_replay_flush(h, stream));
  const int grid = (G.src.B + kSamplesPerWg - 1) / kSamplesPerWg;
  const size_t lds = sizeof(float) * kSamplesPerWg * row_floats;
  prof_begin(2, (hipStream_t)stream);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kGatherThreads), lds, (hipStream_t)stream, G);
  prof_end((hipStream_t)stream);
  HIPC(hipGetLastError());
  return OPRL_OK;
}

}  // namespace oprl
