// learner_internal.h — what the host-side translation units share: the learner's state (struct oprl_learner), the
// launchers' declarations, small layout helpers, and the internals of learner.hip that learner_create.hip,
// learner_dp.hip, learner_group.hip, learner_misc.hip and net_rounds.hip call (namespace oprl_host; defined in learner.hip).
#pragma once
#include <algorithm>
#include <chrono>
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/oprl_amd.h"
#include "host_err.h"
#include "kernels.h"
#include "ln_slice.h"
#include "p2p.h"

namespace oprl {

void prof_fold();      // (the profiler of host_err.h's prof_begin / prof_end: learner.hip)

// (Learners that share a GPU: the fused phase kernels contain bounded cross-workgroup waits that rely on a launch's
// workgroups becoming resident together.  An event chain that serialised the phase launches of all learners of a process
// was measured in round 1 — 8 packed learners 45k -> 17.7k steps/s — and removed in round 3; what protects such runs is
// the clusters-of-four setting (oprl_learner_set_cluster, runners/train.py) and bench.py's verified multi_learner run.)
size_t mlp_slice_lds_bytes(int width, int n_layers);
hipError_t launch_mlp_slice(const MlpArgs& a, int width, hipStream_t st);
hipError_t launch_mlp_slice_multi(const MlpArgs* a, int n, int width, hipStream_t st);
bool mlp_layerwise_ok(const MlpArgs* a, int n, int width);
hipError_t launch_mlp_layerwise(const MlpArgs* a, int n, int width, int n_cus, hipStream_t st, int prec, const TqcJob* job,
                                const MlpArgs* rider, bool first_done, const MlpArgs* tail, int tail_n, int tail0, int tail_prec,
                                const PrefetchJob* prefetch, const LwPairBuf* pairs, bool second_done = false, bool* second_rode = nullptr,
                                const MlpArgs* bwd_rider = nullptr, bool* bwd_rode = nullptr, const DwKArgs* bwd_tiles = nullptr,
                                int bwd_tile_wgs = 0, bool* tiles_rode = nullptr);
bool mlp_layerwise_fin_ok(const MlpArgs* a, int n, int width);
int mlp_layerwise_fin_fit(const MlpArgs* a, int n, int host_wgs, int n_cus);
hipError_t launch_slice_tp_with_fin(const MlpArgs& host, const MlpArgs* a, int n, int n_ride, int width, int n_cus, hipStream_t st,
                                    int prec);
hipError_t launch_mlp_layerwise_first(const MlpArgs* t, int t_n, int t0, int width, int n_cus, hipStream_t st, int prec);
bool mlp_layerwise_rider_ok(const MlpArgs* a, int n, const MlpArgs& rider, int n_cus);
hipError_t init_layerwise_attrs();
hipError_t launch_mlp_slice_tp(const MlpArgs& a, hipStream_t st);
hipError_t launch_mlp_slice_tp2(const MlpArgs& a0, const MlpArgs& a1, int n_cus, hipStream_t st);
hipError_t init_slice_tp_attrs();
bool mlp_slice_tp_shape_ok(const MlpArgs& a, int width);
hipError_t init_kernel_attrs();
hipError_t launch_dw_adam(const DwArgs& a, hipStream_t st);
hipError_t launch_repack(const RepackItem* items_dev, int n_items, int total_blocks, hipStream_t st);
hipError_t launch_adam_flat(float* th, float* m, float* v, float* tt, const float* g, long n,
                            const AdamScalars& ad, hipStream_t st);
hipError_t launch_polyak_flat(float* tt, const float* th, long n, double tau, hipStream_t st);
hipError_t launch_alpha_step(double* log_alpha, double* m, double* v, const float* logp, int B,
                             float target_entropy, double lr, double beta1, double beta2, double eps,
                             int step, double* grad_out, const double* grad_in, float grad_scale,
                             hipStream_t st);
hipError_t launch_reduce_partials(const float* partials, int n_slices, float* out, int out_off,
                                  float scale_loss, float scale_mean, hipStream_t st);
hipError_t launch_sum(const float* x, int n, float* out, int out_off, float scale, hipStream_t st);
hipError_t launch_tqc_target(const float* z, long net_stride, int ldz, int n_nets, int Q, int drop,
                             const float* r, const float* d, const float* logp,
                             const double* log_alpha, float gamma, int B, float* target,
                             hipStream_t st);
hipError_t launch_redq_min(const float* q, long net_stride, int ldq, int M, int B, float* out, hipStream_t st);
int replay_dims(const oprl_replay* h, int* S, int* A);
int replay_nstep(const oprl_replay* h, int* n, double* gamma);
int replay_her(const oprl_replay* h);     // the goal dimension of a replay in hindsight mode (replay_her.hip), else 0
int replay_prior(const oprl_replay* h);   // 1 for a replay that mixes prior data into its batches (replay_mix.hip), else 0
int replay_view(const oprl_replay* h, const float** states, const float** actions,
                const float** rewards, const float** dones, const int** ends, int* n_eps, int* L,
                long* n_transitions);
hipError_t launch_debug_normal(unsigned long long seed, unsigned long long ctr, int rows, int cols, float* out,
                               hipStream_t st);
hipError_t init_fused_attrs();
bool xcd_map_ok();
bool fused_tile64_all();
size_t fused_xbuf_granules_per_cluster(int nc);
hipError_t launch_ddpg_phase1(const DdpgArgs& a, hipStream_t st);
hipError_t launch_ddpg_phase1_dw(const DdpgArgs& a, const DwKArgs& d, hipStream_t st);
bool fused_ddpg_is_lean(int nc, int no_lean, int S, int A, bool sac);
hipError_t launch_ddpg_phase2(const DdpgArgs& a, hipStream_t st);
hipError_t launch_ddpg_phase2_dw(const DdpgArgs& a, const DwKArgs& d, hipStream_t st);
hipError_t launch_ddpg_chain(const DdpgArgs& a, const DwKArgs4& dc, const DwKArgs4& da, const ChainArgs& c, hipStream_t st);
hipError_t launch_ddpg_phase1_group(const DdpgArgs& a0, const DdpgArgs* batch_dev, int n, hipStream_t st);
hipError_t launch_ddpg_phase2_group(const DdpgArgs& a0, const DdpgArgs* batch_dev, int n, hipStream_t st);
int fill_dw_kargs(const DwArgs& a, DwKArgs* k, int tile_k = 32);
bool fused_x2_tiles();
hipError_t launch_dw_adam_group(const void* batch_dev, int ni, int n, int tiles, hipStream_t st);
int compact_dw_kargs(const DwKArgs& k, void* o, int ni);
size_t dw_group_block_bytes(int ni);

}  // namespace oprl

using namespace oprl;

// ---- minimal run-time binding of RCCL (NCCL API; enum values are the API's) ----
namespace oprl_host {
struct NcclId { char internal[OPRL_COMM_ID_BYTES]; };
typedef int (*fn_get_unique_id)(NcclId*);
typedef int (*fn_comm_init_rank)(void**, int, NcclId, int);
typedef int (*fn_all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_comm_destroy)(void*);
typedef const char* (*fn_get_error_string)(int);
constexpr int kNcclFloat32 = 7, kNcclFloat64 = 8, kNcclSum = 0;

struct Rccl {
  void* lib = nullptr;
  fn_get_unique_id get_unique_id = nullptr;
  fn_comm_init_rank comm_init_rank = nullptr;
  fn_all_reduce all_reduce = nullptr;
  fn_broadcast broadcast = nullptr;
  fn_comm_destroy comm_destroy = nullptr;
  fn_get_error_string err_str = nullptr;
  void* comm = nullptr;
  int rank = 0, world = 1;
};

inline int rccl_bind(Rccl& r, const char* path) {
  if (r.lib) return OPRL_OK;
  r.lib = dlopen(path && path[0] ? path : "librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!r.lib) { set_err("dlopen(%s) failed: %s", path ? path : "librccl.so", dlerror()); return OPRL_ERR_INVALID; }
  r.get_unique_id = (fn_get_unique_id)dlsym(r.lib, "ncclGetUniqueId");
  r.comm_init_rank = (fn_comm_init_rank)dlsym(r.lib, "ncclCommInitRank");
  r.all_reduce = (fn_all_reduce)dlsym(r.lib, "ncclAllReduce");
  r.broadcast = (fn_broadcast)dlsym(r.lib, "ncclBroadcast");
  r.comm_destroy = (fn_comm_destroy)dlsym(r.lib, "ncclCommDestroy");
  r.err_str = (fn_get_error_string)dlsym(r.lib, "ncclGetErrorString");
  if (!r.get_unique_id || !r.comm_init_rank || !r.all_reduce) {
    set_err("%s does not export the NCCL API", path ? path : "librccl.so");
    return OPRL_ERR_INVALID;
  }
  return OPRL_OK;
}
inline long net_param_count(const oprl_net& n) {
  long c = 0;
  for (int l = 0; l < n.n_layers; ++l) c += (long)n.dims[l + 1] * n.dims[l] + n.dims[l + 1];
  return c;
}

inline long w_off(const oprl_net& n, int l) {
  long c = 0;
  for (int j = 0; j < l; ++j) c += (long)n.dims[j + 1] * n.dims[j] + n.dims[j + 1];
  return c;
}
inline long b_off(const oprl_net& n, int l) { return w_off(n, l) + (long)n.dims[l + 1] * n.dims[l]; }

inline int check_net(const oprl_net& n, const char* name, int* width) {
  if (n.n_layers < 2 || n.n_layers > OPRL_MAX_LAYERS) {
    set_err("%s: n_layers=%d unsupported (2..%d)", name, n.n_layers, OPRL_MAX_LAYERS);
    return OPRL_ERR_INVALID;
  }
  const int w = n.dims[1];
  if (w != 256 && w != 512) { set_err("%s: hidden width %d unsupported (256 or 512)", name, w); return OPRL_ERR_INVALID; }
  for (int l = 1; l < n.n_layers; ++l)
    if (n.dims[l] != w) { set_err("%s: hidden widths must be equal", name); return OPRL_ERR_INVALID; }
  if (n.dims[0] < 1 || n.dims[0] > 96) { set_err("%s: input dim %d unsupported (1..96)", name, n.dims[0]); return OPRL_ERR_INVALID; }
  if (n.dims[n.n_layers] < 1 || n.dims[n.n_layers] > kNarrowMax) {
    set_err("%s: output dim %d unsupported (1..%d)", name, n.dims[n.n_layers], kNarrowMax);
    return OPRL_ERR_INVALID;
  }
  if (!n.theta) { set_err("%s: theta is null", name); return OPRL_ERR_INVALID; }
  if (!n.pack) { set_err("%s: pack buffer is null (see oprl_net_pack_floats)", name); return OPRL_ERR_INVALID; }
  if (n.theta_target && !n.pack_target) { set_err("%s: pack_target is null", name); return OPRL_ERR_INVALID; }
  *width = w;
  return OPRL_OK;
}

// offsets (floats) of layer l's forward / backward pack inside a pack buffer
inline long pack_off_fwd(const oprl_net& n, int l) {
  long c = 0;
  for (int j = 0; j < l; ++j) c += 2 * pack_floats(n.dims[j + 1], n.dims[j]);
  return c;
}
inline long pack_off_bwd(const oprl_net& n, int l) { return pack_off_fwd(n, l) + pack_floats(n.dims[l + 1], n.dims[l]); }
inline long net_pack_floats(const oprl_net& n) { return pack_off_fwd(n, n.n_layers); }

// the same for the bf16 packs (library-owned, oprl_learner::pack16 / pack16_t), in floats (16-byte fragments)
// (pl = fp16 / bf16 planes per block: 1 for the bf16 packs, 2 for the PrecX2 packs — hi | lo)
inline long pack16_off_fwd(const oprl_net& n, int l, int pl = 1) {
  long c = 0;
  for (int j = 0; j < l; ++j) c += pl * (pack16_floats(n.dims[j + 1], n.dims[j]) + pack16_floats(n.dims[j], n.dims[j + 1]));
  return c;
}
inline long pack16_off_bwd(const oprl_net& n, int l, int pl = 1) { return pack16_off_fwd(n, l, pl) + pl * pack16_floats(n.dims[l + 1], n.dims[l]); }
inline long net_pack16_floats(const oprl_net& n, int pl = 1) { return pack16_off_fwd(n, n.n_layers, pl); }

inline Net net_view(const oprl_net& n, bool target) {
  Net v;
  memset(&v, 0, sizeof v);
  v.n_layers = n.n_layers;
  for (int l = 0; l <= n.n_layers; ++l) v.dims[l] = n.dims[l];
  const float* base = target ? n.theta_target : n.theta;
  const float* pk = target ? n.pack_target : n.pack;
  for (int l = 0; l < n.n_layers; ++l) {
    v.b[l] = base + b_off(n, l);
    v.pf[l] = pk + pack_off_fwd(n, l);
    v.pb[l] = pk + pack_off_bwd(n, l);
  }
  return v;
}

// per-net activation / gradient exchange buffers (HBM, sized for max_batch rows)
constexpr int kMaxCluster = 4;   // CUs per tensor-parallel slice cluster (csrc/tp3.h)

// a Net whose pf / pb point at the bf16 packs (for the PrecBF16 kernels only)
inline Net net_view16(const oprl_net& n, bool target, const float* pk16, int pl = 1) {
  Net v = net_view(n, target);
  for (int l = 0; l < n.n_layers; ++l) {
    v.pf[l] = pk16 + pack16_off_fwd(n, l, pl);
    v.pb[l] = pk16 + pack16_off_bwd(n, l, pl);
  }
  return v;
}

struct NetWs {
  float* X[kMaxLayers] = {nullptr, nullptr, nullptr, nullptr};
  float* dY[kMaxLayers] = {nullptr, nullptr, nullptr, nullptr};
  int ldx0 = 0, lddo = 0, width = 0;
  long dY0_stride = 0;   // dY[0] is kMaxCluster buffers this many floats apart (dz1 partials)
};

inline int n_slices(int B) { return (B + kR - 1) / kR; }   // row slices of kR rows: the grid of a net pass, the rows of a partials table

struct Pool {  // one hipMalloc, bump allocated
  char* base = nullptr;
  size_t cap = 0, used = 0;
  template <class T>
  T* take(size_t n) {
    used = (used + 255) & ~(size_t)255;
    T* p = reinterpret_cast<T*>(base + used);
    used += n * sizeof(T);
    return p;
  }
};

// Every OPRL_AMD_* switch that shapes a learner's launches, read once at oprl_learner_create (read_switches), never
// written afterwards.  Each NO_* turns one form or rider off (tests / A-B: bit-identical to what it replaces).
struct Switches {
  int cluster = kMaxCluster;   // OPRL_AMD_CLUSTER=1 / 2 / 4: CUs per slice cluster in the fused path (ncl's start value)
  // OPRL_AMD_FORM: "chain" (default: the whole update, several per launch), "two" (no_whole: merged phase launches, phase 1
  // + the critic's tiles | phase 2 + the actor's), "p2" (+ no_merge2: phase 2 and the actor's dW as launches of their own),
  // "plain" (+ no_merge: the critic's dW as a launch of its own)
  bool no_whole = false, no_merge2 = false, no_merge = false;
  int chain_max = kChainMax;   // OPRL_AMD_CHAIN=n: at most n updates per k_ddpg_chain launch
  int chain_order = 0;         // OPRL_AMD_CHAIN_ORDER: dispatch order of an update's role rows (ChainArgs::order)
  // OPRL_AMD_NO_RIDE, bit by bit: 1 TQC's TD target on the target heads, 2 its actor forward on the critic heads, 4 the
  // online critics' first hidden launch behind that forward, 8 the next rows on k_lw_dact, 16 the 64 x 64-tile dW kernel
  // of the 512 x 512 layers (DwArgs::no_wide), 32 hidden-layer pairs, 64 TD3's twin tiles on merged phase 1, 128 the
  // critics' second hidden layer behind the tail on the target heads (r06-12), 256 the actor's backward on k_lw_dact
  // (r06-16), 512 its dW + Adam tiles behind it (r06-18)
  bool no_tqc_ride = false, no_af_ride = false, no_fin_ride = false, no_gather_ride = false, no_wide_dw = false;
  bool no_lw_pairs = false, no_merge_twin = false, no_l2_ride = false, no_bwd_ride = false, no_bwd_tiles = false;
  bool no_layerwise = false;   // OPRL_AMD_NO_LAYERWISE: wide nets stay on the single-CU slice kernel
  bool no_p1_rows = false;     // OPRL_AMD_NO_P1_ROWS: TD3's exact-fp32 / bf16 merged launches carry no next-rows row (r06-15)
  bool no_dp_inline = false;   // OPRL_AMD_NO_DP_INLINE: peer-window exchanges as separate launches
  bool no_side_by_side = false;   // OPRL_AMD_NO_SIDE_BY_SIDE: the twin critics back to back (role A, SAC's phase 2)
  int no_lean = 0;             // OPRL_AMD_NO_LEAN: the generic tp3.h passes, never tp4.h's (DdpgArgs::no_lean)
  bool no_wide = false;        // OPRL_AMD_NO_WIDE: never run role A / phase 2's critic pass on clusters of eight
  int no_rt2 = 0;              // OPRL_AMD_NO_RT2: 1 one row tile everywhere; 2 the B roles' two tiles, SAC's role C a role
  bool no_xcd_local = false;   // OPRL_AMD_NO_XCD_LOCAL: cluster exchanges at agent scope
  bool no_bf16_chain = false;  // OPRL_AMD_NO_BF16_CHAIN (set at all): bf16 DDPG learners without k_ddpg_chain<PrecBF16>
};
Switches read_switches();

// The launch form of a fused DDPG / TD3 / SAC update (fused_form, learner.hip; the fields as in DdpgArgs)
struct FusedForm {
  bool lean = false;           // tp4.h's passes (fused_ddpg_is_lean); false: the generic tp3.h passes (DDPG)
  int x2 = 0, bf16 = 0, nc = 1, xnc = 1, wide = 0, twin_split = 0, p2_pair = 0, merged = 0, whole = 0, rt2 = 0;
  int chain_max = 1;           // updates per k_ddpg_chain launch at most (1 unless `whole`)
};

// The rows of one update — or of one chain launch — as the launch builders see them.  It travels down
// from the entry point as an argument; nothing of it is kept on the learner.
struct StepRows {
  enum Stage { kNone, kPhase1, kPhase2 };
  BatchSrc cur;                // the update's rows: the caller's (gather 0), or the kernels' own gather with its counter
  BatchSrc next;               // what the staging launch gathers (counter + 1), s .. s2: the set the rows go to
  Stage stage = kNone;         // which of the update's launches carries the next update's rows
  int n_upd = 1;               // chain launch: the updates it runs (at most the form's chain_max) ...
  bool stage_after_last = false;   // ... whether its last update stages the rows of the update after it ...
  const float* other_set[5] = {};  // ... and the other staging set (cur's s .. s2 are set 0 of the launch)
  bool staged = false;         // out: a launch that stages the next update's rows has gone out
  // training from prioritized replay (oprl_learner_update_weighted): the rows' importance weights [B] and where their
  // |TD| goes [B]; null: the plain update.  Generic launch sequence only (generic_critic_phase).
  const float* w = nullptr;
  float* td_abs = nullptr;
  // calibrated Q-learning (oprl_learner_update_calql): the rows' returns-to-go [B], the lower bound of the
  // conservative penalty's policy entries; null: the plain penalty.  Read by cql_critic_step alone.
  const float* g = nullptr;
};
inline StepRows plain_rows(const float* s, const float* a, const float* r, const float* d, const float* s2) {
  StepRows rows{};
  rows.cur.s = s; rows.cur.a = a; rows.cur.r = r; rows.cur.d = d; rows.cur.s2 = s2;
  return rows;
}

}  // namespace oprl_host

using namespace oprl_host;

#include "learner_modes.h"

struct oprl_learner {
  Switches sw;                 // the environment switches, read by oprl_learner_create
  oprl_learner_config cfg;
  int S, A, Bmax, nc;
  int w_actor = 0, w_critic = 0;
  Pool pool;
  NetWs ws_actor, ws_critic[OPRL_MAX_CRITICS];
  std::vector<DwItem> items_host;  // [critic items..., actor items...] (travel in the kernel arguments)
  int n_items_critic = 0, n_items_actor = 0, tiles_critic = 0, tiles_actor = 0;
  // batch-sized scratch
  float *a2 = nullptr, *logp2 = nullptr, *qn = nullptr /*[nc][B][ldq]*/, *pi = nullptr,
        *raw = nullptr, *logp = nullptr, *da = nullptr /*[nc][B][A]*/, *qpi = nullptr /*[nc][B]*/,
        *target = nullptr, *ydbg = nullptr, *qdbg = nullptr;
  int ldq = 0;
  float *part_c = nullptr /*[nc][slices][4]*/, *part_a = nullptr, *scalars = nullptr;
  double* alpha_grad = nullptr;
  // step_n batch buffers
  float *bs = nullptr, *ba = nullptr, *br = nullptr, *bd = nullptr, *bs2 = nullptr;
  int64_t update_count = 0;
  int redq_subset[OPRL_MAX_CRITICS] = {};   // REDQ: the target critics of the current update (oprl_redq_subset), slot j of qn = net redq_subset[j]
  int opt_step_critic = 0, opt_step_actor = 0, opt_step_alpha = 0;
  int last_B = 0;
  bool actor_updated_last = false;
  long long* trace = nullptr;
  int trace_slot = 0;
  Rccl rccl;
  long n_critic_params = 0, n_actor_params = 0;
  // side streams: independent per-net launches (twin / quantile critics) run concurrently
  hipStream_t side[OPRL_MAX_CRITICS] = {};
  hipEvent_t ev_fork = nullptr, ev_join[OPRL_MAX_CRITICS] = {};
  bool have_side = false;
  bool fused = false;          // DDPG / TD3 / SAC two-kernel path (csrc/fused_ddpg.hip) is built for this learner
  const float* noise1_pending = nullptr;   // update()'s injected actor-phase draws: SAC's role C runs in phase 1
  bool tp_generic_on = false;  // the generic per-net launches may run on clusters of 4 (csrc/slice_tp.hip)
  unsigned tp_tag = 0;         // launch-unique tag source of the cluster exchanges (fused and generic)
  P2pState p2p;                // one-shot all-reduce windows (csrc/p2p.hip); used when p2p_ok
  bool p2p_ok = false, p2p_tested = false, p2p_inline = false;
  int p2p_max_tiles = 0;
  bool dp_inline = false;      // this data-parallel update exchanges inside the dW launches (k_dw_adam<true>)
  DwXchg dw_xchg;
  PrefetchJob prefetch;        // step_n on the generic path (TQC): the next update's rows as riders of this update's k_lw_dact launch
  bool prefetch_pending = false, prefetch_done = false;
  // the modes (learner_modes.h): prioritized weights, D4PG, TD3 + BC, implicit Q-learning, (calibrated) conservative Q-learning, LayerNorm critics
  PerMode per;
  C51Mode c51;
  BcMode bc;
  IqlMode iql;
  CqlMode cql;
  LnMode ln;
  float* batch_alt = nullptr;  // the second set of batch rows [Bmax x (2 S + A + 2)] the riders fill while an update reads the first
  MlpArgs fin_args[OPRL_MAX_CRITICS];   // TQC: the online critics' first-launch arguments of this update (generic_critic_phase step 1) ...
  int fin_tail0 = -1;          // ... of which [fin_tail0, nc) did not fit beside the actor's forward: offered to the target pass's head launch (-1: none pending)
  bool fin16 = false;
  bool fin_l2_done = false;    // ... and the second hidden layer's forward rode on the target pass's heads behind the tail (r06-12); step 3 skips it too
  bool fin_done = false;       // TQC: the online critics' first hidden launch rode on the actor's forward on s' (generic_critic_phase step 1); step 3 skips it
  LwPairBuf lw_pairs = {nullptr, 0, 1u, 1 << 20, nullptr, 3, 0};   // k_lw_mid_pair: flags (own allocation), tags; OPRL_AMD_LW_PAIR: bit 0 forward, bit 1 backward pairs (default 3)
  float* lw_scratch = nullptr; // [critics][layers 1 .. L-1][Bmax x 512]: activations of forward-only layer-by-layer launches (the target pass) — not the nets' dW exchange buffers, which the early first launch has already filled
  MlpArgs rider;               // TQC: the actor's forward on s, prepared in generic_critic_phase to ride on the critic step's head launch ...
  bool rider_pending = false;  // ... offered to the next round (launch_layerwise_round); taken: rider_done, and generic_actor_phase skips its step 5
  bool rider_done = false;
  MlpArgs bwd_rider;           // TQC: the actor's backward, prepared in generic_actor_phase to ride on the k_lw_dact launch whose rows it consumes (r06-16) ...
  bool bwd_rider_pending = false;   // ... offered to the round with the action gradients; taken: bwd_rider_done, and step 8 is skipped
  bool bwd_rider_done = false;
  DwKArgs bwd_tiles;           // ... and its dW + Adam tiles (the actor's step 9) behind it (r06-18): offered with the rider; taken: bwd_tiles_done
  int bwd_tile_wgs = 0;
  bool bwd_tiles_pending = false, bwd_tiles_done = false;
  TqcJob tqc_job;              // TQC: the TD target as the tail of the target critics' head launch (kernels.h) ...
  bool tqc_job_pending = false; // ... offered to the next round; still set afterwards: k_tqc_target as a launch of its own
  unsigned long long* tqc_counter = nullptr;   // [slices at Bmax] arrival counters, zeroed once
  unsigned long long* y_granules = nullptr;   // [Bmax] TD-target hand-off (fused DDPG)
  unsigned epoch = 0;          // monotonically increasing, never reset
  int ncl = 1;                 // CUs per slice cluster in the fused path (csrc/tp3.h)
  int n_cus = 256;
  bool shared_chip = false;    // oprl_learner_set_cluster(< 8): this learner is one of several on the GPU (no clusters of eight either)
  bool group_member = false;   // oprl_group_create took it (and it stays so): no side-by-side twin forms, whose clusters wait for each other
  // merged phase 2 (DdpgArgs::merged bit 1): du granules [Bm][kDuLd], the first layer's dz1 granules [16][Bm][16] and the
  // snapshot of the actor's output layer (Bm = min(max_batch, 256))
  // oprl_learner_step_act: host-mapped pinned block [obs 512 floats | out 512 granules {ticket, value}] and the ticket of the pending row
  float* act_pin = nullptr;
  float* act_map = nullptr;
  unsigned act_ticket = 0;
  bool act_pending = false;
  // oprl_learner_act_rows / step_act_rows (csrc/policy_act_rows.hip): a pinned area of its own, allocated by the first such
  // call [obs OPRL_ACT_ROWS_MAX x S floats | out OPRL_ACT_ROWS_MAX x n_out granules], its ticket and the pending rows (0: none)
  float* rows_pin = nullptr;
  float* rows_map = nullptr;
  unsigned rows_ticket = 0;
  int rows_pending = 0;
  unsigned long long* du_granules = nullptr;
  unsigned long long* g1_granules = nullptr;
  float* w3_snap = nullptr;
  bool xcd_local = false;      // XCD-local cluster exchanges (DdpgArgs::xcd_local): probed dispatcher, not OPRL_AMD_NO_XCD_LOCAL, cleared by an expired wait
  int xnc = kMaxCluster;       // members an exchange area of xbuf is laid out for
  unsigned long long* xbuf = nullptr;
  size_t xbuf_granules = 0;
  // Largest cluster size for which ONE role's clusters (c x slices workgroups, one per CU) fit on the
  // chip.  Phase 1's grid may then exceed the CU count (B > 256): workgroups are dispatched in block
  // order — role A's clusters, then B's, then C's — role A waits for nobody, the members of a cluster
  // are dispatched together, and a B workgroup only ever waits for an A workgroup dispatched before it,
  // so later roles simply start as earlier workgroups retire.
  // Measured (profiles/r01g_batch_sweep.txt): worth it for the lean clusters of 4 (B = 512: 76 -> 51 us
  // per DDPG update); the generic passes on smaller clusters do better fully co-resident.
  int nc_cluster(int B) const {
    const int slices = n_slices(B);
    if (ncl == 4 && 4 * slices <= n_cus) return 4;
    const int roles = 2 + nc;
    int c = ncl;
    while (c > 1 && roles * c * slices > n_cus) c >>= 1;
    return c;
  }
  // key of the in-update noise streams (TD3 smoothing, SAC / TQC reparameterisation draws): the run
  // seed and, in a data-parallel job, the rank — every seed and every rank draws its own eps
  uint64_t noise_seed = 0;
  int noise_rank = 0;
  // OPRL_PREC_BF16: bf16 fragment packs of every net (online: forward + backward, target: forward),
  // derived state owned by the library and written by the dW + Adam epilogues / k_repack; index 0 = actor,
  // 1 + j = critic j
  // Bounded cross-workgroup waits (cluster all-reduce, TD-target hand-off, twin exchanges, gradient tile /
  // window exchanges) REPORT an expiry here besides poisoning their result with NaN: one word of
  // host-mapped memory, written by the device only on that error path (tp3.h report_expired), read by
  // the host at the start of every update / step_n / apply / read_scalars call — no copy, no sync.
  unsigned* err_host = nullptr;
  unsigned* err_dev = nullptr;
  int debug_expire = 0;        // test hook (oprl_learner_debug_expire): this wait site gives up at once
  bool bf16 = false;
  bool x2 = false;             // OPRL_PREC_X2: the lean fused kernels run PrecX2 (engine.h) from packs of two fp16 planes, kept in pack16 / pack16_t
  int planes = 1;              // fp16 / bf16 planes per block of those packs
  // PrecX2 learners: the fused updates do not write the fp32 packs (nothing of theirs reads them); whoever does —
  // the nets' own forward (oprl_mlp_forward / act / backward), a generic launch sequence — gets them rebuilt from the
  // master first (fresh32): [0] the critics' (online + target), [1] the actor's
  bool stale32[2] = {false, false};
  bool lazy_wide = false;      // this learner is in g_lazy and its wide layers' fp32 packs may be left stale (16-bit TQC)
  bool stale_wide = false;     // ... and are: only the critics' 512 x 512 layers' fp32 packs (the narrow layers' are current)
  float* uc_base = nullptr;    // the fp16 packs' uncached allocation (PrecX2 learners)
  bool uc_pool = false;        // the workspace pool is uncached memory as well
  // exact-fp32 DDPG learners (fchain): the fused kernels' fp32 fragment packs are library-owned UNCACHED mirrors of the
  // caller's pack arenas (same layout) — what k_ddpg_chain<PrecF32>'s tiles write, the next update's roles read without a
  // kernel boundary; the caller's packs are rebuilt from the masters when something outside reads them (fresh32).
  // fnet[0] = the actor, fnet[1] = the critic with pack / pack_target -> the mirrors (uc_base holds them)
  bool fchain = false;
  // bf16 DDPG learners (bchain, round 5): whole updates per launch as well — k_ddpg_chain<PrecBF16>: the passes on the bf16
  // packs (coherent loads), the tiles with the exact-fp32 product writing both pack sets, the actor's unit-seed rows in
  // exact fp32 from the fp32 W^T pack; the workspace in uncached memory like the other chain learners'
  bool bchain = false;
  oprl_net fnet[2];
  // k_ddpg_chain (the whole update, several per launch): role C's / the critic tiles' flags, the critic's uncached bias copies
  unsigned long long* w_flags = nullptr;
  float* critic_b16 = nullptr;
  // k_ddpg_chain (several updates per launch): the tiles' FIN flags, the prefetch flags, the uncached bias copies of all
  // four nets ([0] actor, [1] actor target, [2] critic = critic_b16, [3] critic target) and the output layer's two buffers
  unsigned long long* chain_flags = nullptr;   // [ct_fin 192 | at_fin 192 | pf_done 64 | gu_flags 128 | partial q 1024]
  float* gu = nullptr;                         // [kDuLd][Bm][256] the actor's unit-seed dz1 rows (DwGate kind 3)
  float* chain_b16 = nullptr;                  // [4][kMaxLayers][256]
  float* w3buf1 = nullptr;                     // (w3buf[0] = w3_snap)
  bool whole_done = false;     // this update's actor phase was part of the critic phase's launch
  float* pack16[OPRL_MAX_CRITICS + 1] = {};
  float* pack16_t[OPRL_MAX_CRITICS + 1] = {};
  // prebuilt device repack tables: [0] critics online, [1] critics online+target, [2] actor (+target)
  RepackItem* rp_dev[3] = {nullptr, nullptr, nullptr};
  int rp_n[3] = {0, 0, 0}, rp_blocks[3] = {0, 0, 0};
};

// ---- internals of learner.hip, learner_generic.hip and learner_modes.hip that cross units
namespace oprl_host {
const double* alpha_ptr(const oprl_learner* h);
void dev_free(void* p);
bool actor_due(const oprl_learner* h);
bool critic_targets_due(const oprl_learner* h);
bool gauss_actor(const oprl_learner* h);
hipError_t uc_alloc(void** out, size_t bytes);
size_t net_ws_floats(const oprl_net& n, int B);
int fresh32(const oprl_net* net, hipStream_t st);
FusedForm fused_form(const oprl_learner* h, int B, bool dp_inline);
DdpgArgs ddpg_args(oprl_learner* h, const StepRows& rows, int B);
int chain_rows(const oprl_learner* h, int B);
void build_repack_items(const oprl_net* const* nets, int n_nets, int which,
                        std::vector<RepackItem>& items, int* blocks_out,
                        float* const* pk16 = nullptr, float* const* pk16_t = nullptr, int pl = 1);
void alloc_net_ws(Pool& p, const oprl_net& n, int B, NetWs* ws);
bool use_fused(const oprl_learner* h, int B);
void set_step(AdamScalars& ad, int step);
void set_adam(AdamScalars& ad, double lr, double beta1, double beta2, double eps, double tau);
int next_tp_tag(unsigned* counter, unsigned long long* xbuf, size_t xbuf_bytes, hipStream_t st, unsigned* out);
const oprl_net& eff(const oprl_learner* h, const oprl_net& n);
int check_device_error(const oprl_learner* h);
unsigned long long noise_key(uint64_t seed, int rank, uint64_t stream_id);      // Philox key of a noise stream (1 .. 3: the update's and REDQ's; 4, 5: the CQL mode's; 6: the LN critics' dropout masks)
constexpr uint64_t kDropStream = 6;
inline unsigned long long noise_key(const oprl_learner* h, uint64_t stream_id) { return noise_key(h->noise_seed, h->noise_rank, stream_id); }
void redq_subset(uint64_t seed, int rank, uint64_t counter, int n, int m, int* out);
bool tp_generic(const oprl_learner* h, const oprl_net& n, int B);
AdamScalars adam_scalars(const oprl_learner* h, double lr, int step, bool polyak, float grad_scale);
int dw_step(oprl_learner* h, bool critic, int B, hipStream_t st, const PrefetchJob* prefetch = nullptr);
int temperature_step(oprl_learner* h, int B, hipStream_t st);
// learner_generic.hip: the generic (per-net) launch sequence of an update, and the launch builders it shares with the modes
int generic_critic_phase(oprl_learner* h, StepRows& rows, int B, const float* noise0, hipStream_t st);
int generic_actor_phase(oprl_learner* h, StepRows& rows, int B, const float* noise1, hipStream_t st);
MlpArgs base_args(oprl_learner* h, const oprl_net& n, bool target, int B);
void with_store(MlpArgs& a, const NetWs& ws, bool x, bool dy);
MlpArgs critic_sa_args(oprl_learner* h, int j, const float* s, const float* a, int B, bool bwd);
SeedArgs mse_td_seed(const oprl_learner* h, const float* r, const float* d, int B, int n_min);
// net n forward only on the rows (x0 | x1; x1 null: x0 alone) with the activations kept in ws (store_dy: its dY rows
// bound as well), the output to out [B][ldo]; and its counterpart, backward only from those activations with the seed rows
// read from memory (SEED_PTR, ld0)
MlpArgs forward_args(oprl_learner* h, const oprl_net& n, const NetWs& ws, bool store_dy, const float* x0, const float* x1, int B,
                     float* out, int ldo);
MlpArgs backward_args(oprl_learner* h, const oprl_net& n, const NetWs& ws, bool store_dy, int B, const float* seed, int ld0);
void dact_to(MlpArgs& f, const oprl_learner* h, int j);      // the action columns' gradient of critic j's backward -> da[j]
// learner_modes.hip: the modes' allocations, their steps of the generic sequence, and the wide rows' fit
int per_alloc(oprl_learner* h);
void free_modes(oprl_learner* h);
int cql_rows_fit(const oprl_learner* h, const char* who, int B);
int weighted_critic_step(oprl_learner* h, const StepRows& rows, int B, int n_min, hipStream_t st);
int c51_critic_step(oprl_learner* h, const StepRows& rows, int B, hipStream_t st);
int cql_critic_step(oprl_learner* h, const StepRows& rows, int B, hipStream_t st);
int iql_critic_phase(oprl_learner* h, const StepRows& rows, int B, hipStream_t st);
int c51_action_grads(oprl_learner* h, const StepRows& rows, int B, hipStream_t st);
int iql_action_grads(oprl_learner* h, const StepRows& rows, int B, hipStream_t st);
int bc_action_grads(oprl_learner* h, const StepRows& rows, int B, hipStream_t st);
int ln_adam_step(oprl_learner* h, int B, hipStream_t st);      // the LN parameters' step of the critic optimiser (k_ln_adam), at the step count of the dW launch beside it
hipError_t launch_dw_prof(const oprl_learner* h, DwArgs a, hipStream_t st);
void fill_items(const oprl_net& n, const NetWs& ws, std::vector<DwItem>& v, int* tiles, bool small_partial_tiles = false,
                float* pk16 = nullptr, float* pk16_t = nullptr, int pl = 1);
DwArgs dw_args(const oprl_learner* h, bool critic, int B, int step);
void dw_commit(oprl_learner* h, bool critic, const DwArgs& dw, int steps);
bool alpha_rides(const oprl_learner* h);
AlphaJob alpha_job(const oprl_learner* h, int B, int step);
hipError_t alpha_step(const oprl_learner* h, int B, int step, float grad_scale, hipStream_t st);
int fresh32_tables(oprl_learner* h, int which /* bit 0 critics, bit 1 actor */, hipStream_t st, bool wide_too = false);
// net_rounds.hip: one net pass as a launch of its own (a cluster launch with a fresh tag where the shape takes one), and a
// round of them — the n equal nets of one pass — from their finished arguments (tags and borrowed buffers are written into a[])
int launch(const MlpArgs& a, int width, hipStream_t st);
int launch_round(oprl_learner* h, MlpArgs* a, int n, int width, hipStream_t st);
// One round of the generic launch sequence: make_j(j) builds the arguments of net j in [0, n), and launch_round decides
// from the list how they go out.
template <class F>
int for_each_net(oprl_learner* h, int n, int width, hipStream_t st, F&& make_j) {
  MlpArgs a[OPRL_MAX_CRITICS];
  if (n > OPRL_MAX_CRITICS) { set_err("internal: a round of %d nets", n); return OPRL_ERR_STATE; }
  for (int j = 0; j < n; ++j) a[j] = make_j(j);
  return launch_round(h, a, n, width, st);
}
// learners with lazily maintained fp32 packs (fresh32)
extern std::mutex g_lazy_mu;
extern std::vector<oprl_learner*> g_lazy;
int repack_nets(const oprl_net* const* nets, int n_nets, int which, hipStream_t st,
                float* const* pk16 = nullptr, float* const* pk16_t = nullptr, int pl = 1);
// oprl_learner_update_phase / oprl_learner_update on a given plan of rows (the C entry points pass plain_rows)
int learner_update_phase(oprl_learner* h, int phase, StepRows& rows, int B, const float* noise0, const float* noise1, void* stream);
int learner_update(oprl_learner* h, StepRows& rows, int B, const float* noise0, const float* noise1, void* stream);

// The row protocol of a K-loop over a replay whose rows the fused kernels gather themselves: the replay's
// view and the seed, the two staging sets, which of them the coming update reads and whether its rows are already there.
// open() is the loops' shared set-up; plan() yields the coming update's (chain launch's) StepRows, done() takes its
// `staged` and moves on.  It lives on the entry point's stack: a refused or failed call leaves nothing behind.
struct RowStager {
  StepRows rows;               // the plan under way (built in place, handed out by reference)
  float* set[2][5];            // {s, a, r, d, s2}: the learner's own batch rows and batch_alt (the own ones again without it)
  int cur = 0;                 // the set the coming update reads
  bool staged = false;         // ... which a launch of the previous update has already filled
  int flip = 0;                // sets done() moves on by: 1 after phase-1 staging, U after a chain launch, else 0
  // do the replay and K / B fit (dims; K / B; an n-step replay's gamma; packed learners: one-step, no hindsight, no prior data)?  *nstep > 1, replay_her(replay) > 0 or replay_prior(replay): no in-kernel gather
  static int check(const char* who, const oprl_learner* h, const oprl_replay* replay, bool packed, int K, int B, int* nstep);
  int open(const char* who, const oprl_learner* h, oprl_replay* replay, uint64_t seed, void* stream);
  void bind(const oprl_learner* h, uint64_t seed);     // the seed and staging sets of (another) learner over the opened view
  // K_left > 0: a chain launch.  (TQC's rider loop takes a kPhase1 plan for the set alternation and the `next` rows only:
  // its generic launches read plain rows, and it sets `staged` itself from the riders' prefetch_done.)
  StepRows& plan(const oprl_learner* h, StepRows::Stage stage, int K_left = 0);
  void done() { staged = rows.staged; cur = (cur + flip) & 1; }
};
// step_n's K-loop as launches of several updates each (k_ddpg_chain); also the inline data-parallel loop
int chain_loop(oprl_learner* h, RowStager& stg, int K, int B, void* stream);
bool chain_ok(oprl_learner* h, int B);
}  // namespace oprl_host
using namespace oprl_host;

