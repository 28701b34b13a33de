// replay_mix.hip — a batch out of two HBM episodic replays: the first B_p rows from a fixed dataset (the handle's
// `prior`), the rest from the handle itself.  Offline-to-online fine-tuning and online RL with prior
// data (Ball et al., "Efficient Online Reinforcement Learning with Offline Data", ICML 2023: symmetric sampling).
//
// Reference: none (the reference samples one buffer, buffers/episodic_buffer.py:123-133).  For a batch of B rows
//   B_p = min(B, max(0, (int)floor(share * B + 0.5)))        (double arithmetic)
// and row i is the uniform sampler's row i — the one Philox call (counter lo, counter hi, i, 0x5a17) under `seed`,
// bounded_u32(r.x, n_transitions), or the injected idx[i] — over the episode table, the n_transitions and the storage of
// ITS source: `prior` for i < B_p, the handle for i >= B_p.  So rows [0, B_p) are rows [0, B_p) of oprl_replay_sample(prior)
// and rows [B_p, B) are rows [B_p, B) of oprl_replay_sample of a plain handle, both with the same (B, seed, counter), bit
// for bit.  S and A are common to the two sources; E and L are each source's own.
//
// The shape is the gather kernels' (replay_gather.h).  A workgroup's 16 rows are prior rows [0, split) and own rows
// [split, n_here); split is uniform in the workgroup, and all workgroups but the one B_p falls into have split = 0 or
// split = n_here: they stage one episode table and do the plain gather's work.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/oprl_amd.h"
#include "replay_gather.h"

using namespace oprl;

namespace {

struct MixArgs {
  GatherSrc prior, own;  // B, idx, seed and counter are the call's in both
  int Bp;                // rows [0, Bp) from prior, rows [Bp, B) from own
  GatherOut out;
  int* out_src;          // or null: 1 for a prior row, 0 for an own row
};

__global__ __launch_bounds__(kGatherThreads) void k_replay_gather_mix(const MixArgs K) {
  extern __shared__ float stage[];  // [kSamplesPerWg][2S + A + 2]: s | s' | a | r | d, k_replay_gather's layout
  __shared__ int s_ep[kSamplesPerWg], s_t[kSamplesPerWg];
  __shared__ int s_ends_p[kMaxEndsLds], s_ends_o[kMaxEndsLds];
  const GatherSrc &P = K.prior, &O = K.own;
  const int tid = threadIdx.x;
  const int base = blockIdx.x * kSamplesPerWg;
  const int n_here = min(kSamplesPerWg, O.B - base);
  const int split = min(max(K.Bp - base, 0), n_here);
  // only the tables this workgroup's rows are drawn over (uniform in blockIdx): a source that supplies no row of the
  // batch may be empty, and its table is never read
  EndsLds ETp{s_ends_p, 1, 0}, ETo{s_ends_o, 1, 0};
  if (split > 0) ETp = stage_ends(P.ends, P.n_eps, s_ends_p, kMaxEndsLds, tid, kGatherThreads);
  if (split < n_here) ETo = stage_ends(O.ends, O.n_eps, s_ends_o, kMaxEndsLds, tid, kGatherThreads);
  __syncthreads();
  // The slot phase (gather_slots' with the source chosen per row): the values are selected, not the structs, so the
  // lanes of the one straddling workgroup run one draw_slot together.
  if (tid < kSamplesPerWg) {
    const int i = base + tid;
    Slot sl{};
    if (tid < n_here) {
      const bool p = tid < split;
      const EndsLds ET{p ? ETp.lds : ETo.lds, p ? ETp.stride : ETo.stride, p ? ETp.n_blocks : ETo.n_blocks};
      sl = draw_slot(p ? P.ends : O.ends, ET, p ? P.n_eps : O.n_eps, p ? P.n_transitions : O.n_transitions, O.seed,
                     O.counter, i, O.idx);
      if (K.out.ep != nullptr) K.out.ep[i] = sl.e;
      if (K.out.step != nullptr) K.out.step[i] = sl.t;
      if (K.out_src != nullptr) K.out_src[i] = p ? 1 : 0;
    }
    s_ep[tid] = sl.e;
    s_t[tid] = sl.t;
  }
  __syncthreads();
  const int S = O.S, A = O.A, W = 2 * S + A + 2;
  gather_stage_rows_mix(P, O, split, n_here, s_ep, s_t, stage);
  __syncthreads();
  gather_write_rows(K.out, S, A, base, n_here, stage, W, S, 2 * S);
  gather_write_rd(K.out, base, n_here, stage + 2 * S + A, stage + 2 * S + A + 1, W);
}

// what keeps a handle from being one side of a mixed batch; null: it is plain
const char* not_plain(const oprl_replay* r) {
  if (r->nstep > 1) return "samples n-step returns (oprl_replay_set_nstep)";
  if (r->her.G > 0) return "relabels goals in hindsight (oprl_replay_set_her)";
  if (r->prio) return "is prioritized (oprl_replay_prio_enable)";
  return nullptr;
}

}  // namespace

namespace oprl {
int replay_prior(const oprl_replay* h) { return h->prior != nullptr ? 1 : 0; }
}

extern "C" int oprl_replay_set_prior(oprl_replay* h, oprl_replay* prior, double share) {
  if (!h) { set_err("oprl_replay_set_prior: null replay handle"); return OPRL_ERR_INVALID; }
  if (!prior) { h->prior = nullptr; h->prior_share = 0.0; return OPRL_OK; }      // the mode off: the share is not read
  if (!(share >= 0.0) || !(share <= 1.0)) {
    set_err("oprl_replay_set_prior: the prior share of a batch must lie in [0, 1] (got %g)", share);
    return OPRL_ERR_INVALID;
  }
  if (prior == h) { set_err("oprl_replay_set_prior: a replay cannot be the prior of itself"); return OPRL_ERR_INVALID; }
  if (prior->S != h->S || prior->A != h->A) {
    set_err("oprl_replay_set_prior: the prior's dims (%d,%d) are not this replay's (%d,%d)", prior->S, prior->A, h->S, h->A);
    return OPRL_ERR_INVALID;
  }
  if (const char* why = not_plain(h)) {
    set_err("oprl_replay_set_prior: this replay %s; mixed batches take plain rows on both sides", why);
    return OPRL_ERR_STATE;
  }
  if (const char* why = not_plain(prior)) {
    set_err("oprl_replay_set_prior: the prior replay %s; mixed batches take plain rows on both sides", why);
    return OPRL_ERR_STATE;
  }
  if (prior->prior) {
    set_err("oprl_replay_set_prior: the prior replay has a prior of its own (one prior per batch)");
    return OPRL_ERR_STATE;
  }
  h->prior = prior;
  h->prior_share = share;
  return OPRL_OK;
}

extern "C" int oprl_replay_sample_mix(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed, uint64_t counter,
                                      float* out_s, float* out_a, float* out_r, float* out_d, float* out_s2,
                                      int32_t* out_ep, int32_t* out_step, int32_t* out_src, void* stream) {
  RC(gather_check("oprl_replay_sample_mix", h, B, out_s, out_a, out_r, out_d, out_s2));
  oprl_replay* p = h->prior;
  if (!p) {
    set_err("oprl_replay_sample_mix: this replay has no prior (oprl_replay_set_prior)");
    return OPRL_ERR_STATE;
  }
  // nothing tracks the handles that are priors: whatever mode the prior took on since set_prior is found here
  if (const char* why = not_plain(p)) {
    set_err("oprl_replay_sample_mix: the prior replay %s since oprl_replay_set_prior; mixed batches take plain rows on both sides", why);
    return OPRL_ERR_STATE;
  }
  MixArgs K;
  GatherOut unused;
  gather_fill(p, B, idx, seed, counter, out_s, out_a, out_r, out_d, out_s2, out_ep, out_step, &K.prior, &unused);
  gather_fill(h, B, idx, seed, counter, out_s, out_a, out_r, out_d, out_s2, out_ep, out_step, &K.own, &K.out);
  K.Bp = prior_rows(B, h->prior_share);
  K.out_src = out_src;
  if (K.Bp > 0 && (p->n_transitions <= 0 || p->n_eps <= 0)) {
    set_err("oprl_replay_sample_mix: the prior replay is empty and has to supply %d of the %d rows", K.Bp, (int)B);
    return OPRL_ERR_STATE;
  }
  if (K.Bp < B && (h->n_transitions <= 0 || h->n_eps <= 0)) {
    set_err("oprl_replay_sample_mix: this replay is empty and has to supply %d of the %d rows (its prior supplies %d)",
            (int)B - K.Bp, (int)B, K.Bp);
    return OPRL_ERR_STATE;
  }
  RC(oprl_replay_flush(p, stream));          // (fill_replay leaves staged rows)
  RC(oprl_replay_flush(h, stream));
  const int grid = (B + kSamplesPerWg - 1) / kSamplesPerWg;
  const size_t lds = sizeof(float) * kSamplesPerWg * (2 * h->S + h->A + 2);
  prof_begin(2, (hipStream_t)stream);
  hipLaunchKernelGGL(k_replay_gather_mix, dim3(grid), dim3(kGatherThreads), lds, (hipStream_t)stream, K);
  prof_end((hipStream_t)stream);
  HIPC(hipGetLastError());
  return OPRL_OK;
}
