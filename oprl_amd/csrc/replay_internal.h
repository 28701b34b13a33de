// replay_internal.h — the replay handle (struct oprl_replay) and what the replay's translation units share: the writes,
// the flush and the uniform sampler (replay.hip), the sum tree of prioritized replay (replay_prio.hip), the n-step and
// hindsight samplers (replay_nstep.hip, replay_her.hip; their kernels' common shape is replay_gather.h), the sampler
// over two replays (replay_mix.hip), the returns-to-go of sampled slots (replay_returns.hip) and the many-episodes write
// (replay_rows.hip).  learner_per.hip reads the handle's sum tree too.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/oprl_amd.h"
#include "host_err.h"

namespace oprl {

// Sum tree of prioritized replay.  Level 0 holds one leaf per slot (e, t) at e·L + t; level k + 1
// holds one node per kPrioFan nodes of level k; the top level holds the root alone.  Every level is padded with zeros
// to a multiple of kPrioFan, so a node's children are one aligned run of kPrioFan floats.  All levels live in `tree`,
// level k at `off[k]`, the leaves first.
constexpr int kPrioFan = 256;       // children per node: four per lane of one wave
constexpr int kPrioMaxLevels = 8;
struct PrioTree {
  int n_levels = 0;                     // levels including the leaves (>= 2); the root is level n_levels - 1
  long count[kPrioMaxLevels] = {};      // nodes per level before padding
  long off[kPrioMaxLevels + 1] = {};    // offsets of the levels in `tree`; off[n_levels] = floats allocated
  float* tree = nullptr;
  int* dirty = nullptr;                 // one flag per node of levels >= 1 (level k at off[k] - off[1]): recompute it
  int* lens = nullptr;                  // [E] the episode lengths the leaves stand for (0 = dead episode)
  float* p_max = nullptr;               // device scalar: the largest priority ever assigned (1 before any update)
  int* owner = nullptr;                 // [E·L] the batch row that sets a slot in a priority update, -1 between updates
  int n_eps = 0;                        // the episodes_counter the leaves stand for
  double alpha = 0.6, eps = 1e-6;
  long long* idx = nullptr;             // sampler scratch: one flat transition index per row
  int idx_cap = 0;
};

constexpr int kNstepMax = 16;       // largest n of the n-step sampler (replay_nstep.hip: one lane per (sample, step))

// Hindsight mode of a replay (oprl_replay_set_her, replay_her.hip).  G = 0: off.
constexpr int kHerMaxGoal = 16;     // largest goal dimension (replay_her.hip: one lane per (sample, goal element))
struct HerMode {
  int ag_off = 0, g_off = 0, G = 0;     // achieved goal [ag_off, ag_off + G), desired goal [g_off, g_off + G) of a state row
  int strategy = 0, reward = 0;         // 0 future | 1 final;  0 sparse | 1 dense
  double ratio = 0.8, threshold = 0.0;  // relabelled share of the eligible rows; the sparse reward's distance bound
};

// Keep the leaves in step with a flush: the staged rows `rows` (n_rows records of `rowlen` floats, [ep, t] as int
// bits first; device-readable) and the episode-table entries [ends_first, ends_n) it uploaded (ends_n = 0: none).
// Called by oprl_replay_flush and oprl_replay_write_rows after their copies, on their stream.
int prio_flush(oprl_replay* h, const float* rows, int n_rows, int rowlen, int ends_first, int ends_n, hipStream_t st);
void prio_free(PrioTree* p);

// staged rows / changed table entries up to which an ingest kernel reads the pinned buffers itself (replay.hip,
// replay_rows.hip); beyond them the rows are copied to device staging first
constexpr int kDirectRows = 16;
constexpr int kDirectEnds = 2048;
constexpr int kRowsMax = 256;       // records of one oprl_replay_write_rows call (replay_rows.hip)
// What an ingest launch of n_rows staged rows has to take along: the pending range [first, n) of the episode-ends
// table (n = 0: none), and `direct`: its kernel may read the pinned row buffer and ends_host[ends_cur] through their
// device mappings rows_map / ends_map (null: not mapped) instead of waiting for copies to device staging.
struct PendingEnds { int first, n; bool direct; };
PendingEnds pending_ends(const oprl_replay* h, int n_rows, const float* rows_map, const int* ends_map);

// B_p: the prior rows of a batch of B over a replay in prior-data mode, rows [0, B_p) of the batch
inline int prior_rows(int B, double share) {
  const double x = floor(share * (double)B + 0.5);
  return x > 0.0 ? (x < (double)B ? (int)x : B) : 0;
}

// what oprl_replay_set_lens refuses, without touching the handle (`who` names the caller in the message)
int check_lens(const oprl_replay* h, const int32_t* ep_lens_host, int32_t episodes_counter, const char* who);
// the table range a launch or copy on `st` just took from ends_host[ends_cur]: event, buffer switch, nothing pending
int ends_sent(oprl_replay* h, hipStream_t st);
void rows_free(oprl_replay* h);     // the staging of oprl_replay_write_rows, if it was ever allocated

}  // namespace oprl

struct oprl_replay {
  int E, L, S, A;
  float *states, *actions, *rewards, *dones;
  int* ends_dev = nullptr;
  int n_eps = 0;
  long n_transitions = 0;
  // double-buffered pinned staging for add_transition rows and for ends uploads
  int rowlen = 0;
  float* stage_host[2] = {nullptr, nullptr};
  float* stage_dev[2] = {nullptr, nullptr};
  int* ends_host[2] = {nullptr, nullptr};
  hipEvent_t stage_ev[2], ends_ev[2];
  bool stage_busy[2] = {false, false}, ends_busy[2] = {false, false};
  int cur = 0, ends_cur = 0, n_staged = 0;
  // the device copies of the pinned buffers' addresses, and the ends-table upload oprl_replay_set_lens left for the
  // next flush: entries [first, n) of ends_host[ends_cur] differ from what the device holds (ends_last = its mirror)
  float* stage_map[2] = {nullptr, nullptr};
  int* ends_map[2] = {nullptr, nullptr};
  std::vector<int> ends_last;
  bool ends_pending = false;
  int ends_first = 0, ends_n = 0;
  oprl::PrioTree* prio = nullptr;       // the sum tree once oprl_replay_prio_enable ran, else null
  // n-step mode (oprl_replay_set_nstep): with nstep > 1 oprl_replay_sample gathers n-step rows
  int nstep = 1;
  double nstep_gamma = 1.0;
  // hindsight mode (oprl_replay_set_her): with her.G > 0 oprl_replay_sample gathers relabelled rows
  oprl::HerMode her;
  // prior-data mode (oprl_replay_set_prior): with prior non-null oprl_replay_sample gathers the first
  // floor(prior_share · B + 0.5) rows of a batch from `prior` (the caller keeps it alive) and the rest from this replay
  oprl_replay* prior = nullptr;
  double prior_share = 0.0;
  // oprl_replay_write_rows (replay_rows.hip): double-buffered pinned staging of its own for up to kRowsMax
  // records of reclen floats, allocated by the first call
  bool rows_ready = false;
  int reclen = 0, rows_cur = 0;
  float* rows_host[2] = {nullptr, nullptr};
  float* rows_dev[2] = {nullptr, nullptr};
  float* rows_map[2] = {nullptr, nullptr};
  hipEvent_t rows_ev[2];
  bool rows_ev_made[2] = {false, false}, rows_busy[2] = {false, false};
};
