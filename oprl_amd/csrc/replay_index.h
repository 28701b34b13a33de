// replay_index.h — the uniform sampler's draw, and flat transition index -> (episode, step), for every device-side
// sampler: the gather kernels (replay_gather.h: k_replay_gather in replay.hip, k_replay_gather_nstep in
// replay_nstep.hip, k_replay_gather_her in replay_her.hip, k_replay_gather_mix in replay_mix.hip, which draws each
// row over the table of the row's own replay) and the in-kernel gathers of the fused and layer-by-layer
// launches (batch_rows.h: load_batch, prefetch_rows_direct).  All of them pick the same slot for the same
// (seed, counter, row): the gather kernels call draw_slot; batch_rows.h's two sites carry its no-index path written
// out (kUniformWord, bounded_u32 of r.x, find_episode), because the call moves an instruction selection inside the
// benchmarked launches.  A change to the draw is a change here and at those two sites.
//
// Reference: EpisodicReplayBuffer._inds_to_episodic (buffers/episodic_buffer.py:114-121): the episode of flat
// index `ind` is the first slot whose cumulative end exceeds it (np.argmin over the >= mask; if none does,
// argmin of an all-True mask = slot 0).  A binary search over the table in global memory is ~log2(E)
// dependent round trips; the table is staged in LDS instead — whole when it fits (the reference's 1000
// episodes), otherwise as a COARSE table of every stride-th end, finished by <= log2(stride) + 1 global probes
// (a replay of 200-step episodes has 5000 of them: 5.4 us -> 1.x us for the sampling chain).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace oprl {

struct EndsLds { const int* lds; int stride, n_blocks; };

// all threads of the workgroup; a barrier must follow before find_episode
__device__ __forceinline__ EndsLds stage_ends(const int* __restrict__ ends, int n_eps, int* lds, int lds_cap,
                                              int tid, int n_threads) {
  EndsLds t;
  t.lds = lds;
  t.stride = (n_eps + lds_cap - 1) / lds_cap;
  if (t.stride < 1) t.stride = 1;
  t.n_blocks = (n_eps + t.stride - 1) / t.stride;
  for (int j = tid; j < t.n_blocks; j += n_threads) {
    const int last = min(n_eps, (j + 1) * t.stride) - 1;
    lds[j] = ends[last];
  }
  return t;
}

// first episode e with ends[e] > ind (0 if none); *start = ends[e - 1] (0 for e = 0)
__device__ __forceinline__ int find_episode(const int* __restrict__ ends, int n_eps, const EndsLds& T, long ind,
                                            long* start) {
  int lo = 0, hi = T.n_blocks;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long)T.lds[mid] > ind) hi = mid; else lo = mid + 1;
  }
  int e;
  if (lo >= T.n_blocks) {
    e = 0;                                            // every end <= ind: the all-True argmin
  } else if (T.stride == 1) {
    e = lo;
  } else {
    int a = lo * T.stride, b = min(n_eps, a + T.stride) - 1;   // ends[b] > ind is known
    while (a < b) {
      const int mid = (a + b) >> 1;
      if ((long)ends[mid] > ind) b = mid; else a = mid + 1;
    }
    e = a;
  }
  if (e == 0) *start = 0;
  else *start = T.stride == 1 ? (long)T.lds[e - 1] : (long)ends[e - 1];
  return e;
}

// fourth Philox counter word of the uniform draw (the prioritized sampler has its own: replay_prio.hip kSampleWord)
constexpr uint32_t kUniformWord = 0x5a17u;

struct Slot {
  int e, t;          // episode and step of the drawn transition
  long start, end;   // ends[e - 1] (0 for e = 0) and ends[e]: the episode holds end - start steps
  u32x4 r;           // the draw's Philox words (r.x picked the slot); zeros where the draw was skipped
};

// Row i of the sample (seed, counter): flat index bounded_u32(r.x, n_transitions), or idx[i] when indices are
// injected, as (episode, step).  An injected index skips the Philox call unless kAlwaysDraw (hindsight reads r.y and
// r.z of injected rows too).  After stage_ends' barrier.
template <bool kAlwaysDraw = false>
__device__ __forceinline__ Slot draw_slot(const int* ends, const EndsLds& ET, int n_eps, long n_transitions,
                                          unsigned long long seed, unsigned long long counter, int i,
                                          const long long* idx) {
  Slot s;
  s.r = u32x4{0u, 0u, 0u, 0u};
  if (kAlwaysDraw || idx == nullptr)
    s.r = philox4x32_10(u32x4{(uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)i, kUniformWord}, (uint32_t)seed,
                        (uint32_t)(seed >> 32));
  const long ind = idx != nullptr ? (long)idx[i] : (long)bounded_u32(s.r.x, (uint32_t)n_transitions);
  // first episode with ends[e] > ind  (np.argmin over the >= mask; all-True -> 0)
  s.e = find_episode(ends, n_eps, ET, ind, &s.start);
  s.t = (int)(ind - s.start);
  // (a global load when the table is coarse; k_replay_gather never reads `end` or `r`, and both are dead code there)
  s.end = ET.stride == 1 ? (long)ET.lds[s.e] : (long)ends[s.e];
  return s;
}

}  // namespace oprl
