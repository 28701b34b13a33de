// learner.hip — host orchestration of update() for DDPG / TD3 / SAC / TQC and the
// C-ABI of include/oprl_amd.h.  Each update() is a short fixed sequence of
// k_mlp_slice / k_dw_adam launches on the caller's stream; no host sync inside.
// Here: the fused launch forms, the dW + Adam launch, the update's entry points and step_n; critic_phase / actor_phase
// dispatch to the fused branches or to the generic per-net sequence (learner_generic.hip; the modes: learner_modes.hip).
//
// Order of operations follows the reference exactly (it matters: the actor
// loss sees the post-Adam critic, Polyak sees both updated nets):
//   DDPG  algos/ddpg.py:61-107      TD3  algos/td3.py:71-146
//   SAC   algos/sac.py:75-155       TQC  algos/tqc.py:116-189
#include "learner_internal.h"
#include "philox.h"

namespace oprl {

static thread_local std::string g_err;
void set_err(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
}

// ---- HIP-event profiler (off by default; zero cost when off) ----------------
struct Prof {
  bool on = false;
  std::vector<hipEvent_t> ev;      // pairs
  std::vector<int> kind;
  long counts[OPRL_PROFILE_KINDS] = {0, 0, 0, 0, 0, 0};
  double ms[OPRL_PROFILE_KINDS] = {0, 0, 0, 0, 0, 0};
};
static Prof g_prof;
static const size_t kProfMaxPairs = 1 << 16;

void prof_fold() {
  if (g_prof.ev.empty()) return;
  (void)hipDeviceSynchronize();
  for (size_t i = 0; i + 1 < g_prof.ev.size(); i += 2) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_prof.ev[i], g_prof.ev[i + 1]) == hipSuccess) {
      g_prof.counts[g_prof.kind[i / 2]] += 1;
      g_prof.ms[g_prof.kind[i / 2]] += t;
    }
    (void)hipEventDestroy(g_prof.ev[i]);
    (void)hipEventDestroy(g_prof.ev[i + 1]);
  }
  g_prof.ev.clear();
  g_prof.kind.clear();
}

void prof_begin(int kind, hipStream_t st) {
  if (!g_prof.on) return;
  if (g_prof.ev.size() >= 2 * kProfMaxPairs) prof_fold();
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
  g_prof.ev.push_back(a);
  g_prof.ev.push_back(b);
  g_prof.kind.push_back(kind);
  (void)hipEventRecord(a, st);
}

void prof_end(hipStream_t st) {
  if (!g_prof.on || g_prof.ev.empty()) return;
  (void)hipEventRecord(g_prof.ev.back(), st);
}

}  // namespace oprl

namespace oprl_host {

// learners with lazily maintained fp32 packs, by pack pointer (oprl_mlp_* know a net, not its learner)
// Whole-update launches (k_ddpg_chain) take the whole chip for up to 32 updates.  Learners of one process that launch them
// from DIFFERENT STREAMS (one host thread per learner: the multi-seed layout) take TURNS: a launch waits for the event
// behind the last whole-update launch of another stream — two such launches side by side would only hold each other's
// compute units with waiting workgroups (bounded waits would expire).  Nothing is recorded until a second stream shows
// up (a process whose learners share one stream — the headline path, bench.py's blocks — pays no event, no barrier
// packet); the first launch from a second stream drains the device on the host, once.
// Limits (deliberate): only the WHOLE-UPDATE launches take turns — another learner's merged / phase launches, or
// any other kernel of the process on a second stream, can still hold compute units while a chain launch waits for its
// own workgroups: the bounded wait then expires, the call reports it, and after clear_error the learner runs the
// shared-chip forms (tested: tests/test_gpu_errors.py); a learner that is KNOWN to share the GPU says so up front
// (set_cluster(4), OPRL_AMD_FORM=plain).  Streams are told apart by handle and devices by id & 15; the one
// hipDeviceSynchronize (the first launch from a second stream) runs under the mutex, once per process and device.
struct ChipTurn {
  std::mutex mu;
  hipEvent_t ev[16] = {};
  hipStream_t stream[16] = {};
  bool any[16] = {}, multi[16] = {}, rec[16] = {};
};
ChipTurn g_turn;

hipError_t chip_turn_begin(hipStream_t st, int* dev_out) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  dev &= 15;
  *dev_out = dev;
  if (!g_turn.any[dev] || g_turn.stream[dev] == st) return hipSuccess;
  if (!g_turn.multi[dev]) {                       // the second stream of this process: from now on events
    g_turn.multi[dev] = true;
    return hipDeviceSynchronize();                // (once; the other stream's handle may be gone by now)
  }
  return g_turn.rec[dev] ? hipStreamWaitEvent(st, g_turn.ev[dev], 0) : hipSuccess;
}
void chip_turn_end(hipStream_t st, int dev) {
  g_turn.any[dev] = true;
  g_turn.stream[dev] = st;
  g_turn.rec[dev] = false;
  if (!g_turn.multi[dev]) return;
  if (g_turn.ev[dev] == nullptr && hipEventCreateWithFlags(&g_turn.ev[dev], hipEventDisableTiming) != hipSuccess) { g_turn.ev[dev] = nullptr; return; }
  if (hipEventRecord(g_turn.ev[dev], st) == hipSuccess) g_turn.rec[dev] = true;
}

// the net the fused kernels of `h` see (fchain: the one with the mirrored packs)
const oprl_net& eff(const oprl_learner* h, const oprl_net& n) {
  if (h->fchain) {
    if (&n == &h->cfg.actor) return h->fnet[0];
    if (&n == &h->cfg.critics[0]) return h->fnet[1];
  }
  return n;
}

std::mutex g_lazy_mu;
std::vector<oprl_learner*> g_lazy;

// Uncached device memory (hipDeviceMallocUncached) is never handed back to the runtime: a block a destroyed learner
// owned waits here for the next PrecX2 learner.  Measured (tools/sac_probe2.py, r03 log): after hipFree of such a block,
// later ordinary allocations of the same process — another learner's workspace — lost flag granules in the fused
// kernels (bounded waits expired) until the process ended; with the blocks kept, 0 failures in the same churn.
struct UcBlock { void* p; size_t bytes; bool used; };
std::mutex g_uc_mu;
std::vector<UcBlock> g_uc;
hipError_t uc_alloc(void** out, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_uc_mu);
  for (UcBlock& b : g_uc)
    if (!b.used && b.bytes >= bytes && b.bytes <= 2 * bytes + (1u << 20)) { b.used = true; *out = b.p; return hipSuccess; }
  // a process that cycles learners of ever different shapes must not grow without bound: once more than 64 MB of
  // blocks lie idle, ANY idle block that is large enough serves (the smallest such), whatever its size
  size_t idle = 0;
  for (const UcBlock& b : g_uc) if (!b.used) idle += b.bytes;
  if (idle > ((size_t)64 << 20)) {
    UcBlock* best = nullptr;
    for (UcBlock& b : g_uc)
      if (!b.used && b.bytes >= bytes && (best == nullptr || b.bytes < best->bytes)) best = &b;
    if (best != nullptr) { best->used = true; *out = best->p; return hipSuccess; }
  }
  void* p = nullptr;
  hipError_t e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) return e;
  g_uc.push_back(UcBlock{p, bytes, true});
  *out = p;
  return hipSuccess;
}
void dev_free(void* p);
bool uc_release(void* p) {       // true: the block was one of these (and is NOT freed)
  std::lock_guard<std::mutex> lk(g_uc_mu);
  for (UcBlock& b : g_uc)
    if (b.p == p) { b.used = false; return true; }
  return false;
}
void dev_free(void* p) {
  if (p != nullptr && !uc_release(p)) (void)hipFree(p);
}

// (wide_too: also when only the wide layers' packs are stale — the launch about to run reads THOSE)
int fresh32_tables(oprl_learner* h, int which /* bit 0 critics, bit 1 actor */, hipStream_t st, bool wide_too) {
  if ((which & 1) && (h->stale32[0] || (wide_too && h->stale_wide))) {
    HIPC(launch_repack(h->rp_dev[1], h->rp_n[1], h->rp_blocks[1], st));
    h->stale32[0] = false;
    h->stale_wide = false;
  }
  if ((which & 2) && h->stale32[1]) {
    HIPC(launch_repack(h->rp_dev[2], h->rp_n[2], h->rp_blocks[2], st));
    h->stale32[1] = false;
  }
  return OPRL_OK;
}

// before a launch that reads `net`'s fp32 packs outside its learner's fused kernels
int fresh32(const oprl_net* net, hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_lazy_mu);
  for (oprl_learner* h : g_lazy) {
    if (!h->stale32[0] && !h->stale32[1] && !h->stale_wide) continue;
    // (a target module of the Python host is a net of its own whose pack IS the learner's target pack)
    auto same = [&](const oprl_net& n) {
      return net->pack == n.pack || (n.pack_target != nullptr && (net->pack == n.pack_target || net->pack_target == n.pack_target));
    };
    if (same(h->cfg.actor)) return fresh32_tables(h, 2, st);
    for (int j = 0; j < h->nc; ++j)
      if (same(h->cfg.critics[j])) return fresh32_tables(h, 1, st, true);
  }
  return OPRL_OK;
}

void fill_items(const oprl_net& n, const NetWs& ws, std::vector<DwItem>& v, int* tiles, bool small_partial_tiles,
                float* pk16, float* pk16_t, int pl) {
  for (int l = 0; l < n.n_layers; ++l) {
    DwItem it;
    memset(&it, 0, sizeof it);
    it.K = n.dims[l];
    it.N = n.dims[l + 1];
    it.X = ws.X[l];
    it.ldx = (l == 0) ? ws.ldx0 : ws.width;
    it.dY = ws.dY[l];
    it.ldy = (l == n.n_layers - 1) ? ws.lddo : ws.width;
    const long wo = w_off(n, l), bo = b_off(n, l);
    it.w = n.theta + wo;                       it.b = n.theta + bo;
    it.w_t = n.theta_target ? n.theta_target + wo : nullptr;
    it.b_t = n.theta_target ? n.theta_target + bo : nullptr;
    it.w_m = n.adam_m ? n.adam_m + wo : nullptr; it.b_m = n.adam_m ? n.adam_m + bo : nullptr;
    it.w_v = n.adam_v ? n.adam_v + wo : nullptr; it.b_v = n.adam_v ? n.adam_v + bo : nullptr;
    it.w_g = n.grad ? n.grad + wo : nullptr;     it.b_g = n.grad ? n.grad + bo : nullptr;
    it.pf = n.pack + pack_off_fwd(n, l);
    it.pb = n.pack + pack_off_bwd(n, l);
    it.tpf = n.pack_target ? n.pack_target + pack_off_fwd(n, l) : nullptr;
    it.pf16 = pk16 ? pk16 + pack16_off_fwd(n, l, pl) : nullptr;
    it.pb16 = pk16 ? pk16 + pack16_off_bwd(n, l, pl) : nullptr;
    it.tpf16 = (pk16_t && n.theta_target) ? pk16_t + pack16_off_fwd(n, l, pl) : nullptr;
    it.x2 = pl == 2 ? 1 : 0;
    it.dY_part_stride = (l == 0 && n.n_layers > 1) ? ws.dY0_stride : 0;
    it.scaled = (l < n.n_layers - 1) ? 1 : 0;
    it.rs = ws.dY[n.n_layers - 1];
    it.rs_ld = ws.lddo;
    // (8-row tiles for this layer were measured: no difference — profiles/r01b_experiments.txt)
    it.tile_n = kDwTileN;
    const int tn = (it.N + it.tile_n - 1) / it.tile_n;
    it.tiles_k = (it.K + kDwTile - 1) / kDwTile;
    it.tile_begin = *tiles;
    *tiles += tn * it.tiles_k;
    it.tile_end = *tiles;
    v.push_back(it);
  }
}

size_t net_ws_floats(const oprl_net& n, int B) {
  size_t f = 0;
  f += (size_t)B * round_up(n.dims[0], 4) + 64;
  for (int l = 1; l < n.n_layers; ++l) f += (size_t)B * n.dims[1] + 64;
  for (int l = 0; l < n.n_layers - 1; ++l) f += ((size_t)B * n.dims[1] + 1088) * (l == 0 ? kMaxCluster : 1) + 64;
  f += (size_t)B * round_up(n.dims[n.n_layers], 4) + 64;
  return f + 64 * 8;
}

void alloc_net_ws(Pool& p, const oprl_net& n, int B, NetWs* ws) {
  ws->width = n.dims[1];
  ws->ldx0 = round_up(n.dims[0], 4);
  ws->lddo = round_up(n.dims[n.n_layers], 4);
  ws->X[0] = p.take<float>((size_t)B * ws->ldx0);
  for (int l = 1; l < n.n_layers; ++l) ws->X[l] = p.take<float>((size_t)B * ws->width);
  // the dz1 partial buffers are read together (k_dw_adam sums them on load): an odd multiple
  // of 4 KB + 256 B between them keeps the four loads of one element off the same HBM channel
  ws->dY0_stride = (long)B * ws->width + 1088;
  for (int l = 0; l < n.n_layers - 1; ++l)
    ws->dY[l] = p.take<float>(l == 0 ? (size_t)ws->dY0_stride * kMaxCluster : (size_t)B * ws->width);
  ws->dY[n.n_layers - 1] = p.take<float>((size_t)B * ws->lddo);
}

void set_adam(AdamScalars& ad, double lr, double beta1, double beta2, double eps, double tau) {
  ad.lr = (float)lr; ad.beta1 = (float)beta1; ad.beta2 = (float)beta2; ad.eps = (float)eps;
  ad.tau = (float)tau;
  ad.omb1 = (float)(1.0 - beta1);
  ad.omb2 = (float)(1.0 - beta2);
  ad.omtau = (float)(1.0 - tau);
  ad.lr_d = lr; ad.beta1_d = beta1; ad.beta2_d = beta2;
}

void set_step(AdamScalars& ad, int step) {
  ad.step_base = step; ad.step_dev = nullptr;
  ad.step_size_host = (float)(ad.lr_d / (1.0 - pow(ad.beta1_d, (double)step)));
  ad.bc2_sqrt_host = (float)sqrt(1.0 - pow(ad.beta2_d, (double)step));
}

AdamScalars adam_scalars(const oprl_learner* h, double lr, int step, bool polyak, float grad_scale) {
  AdamScalars ad;
  memset(&ad, 0, sizeof ad);
  const oprl_hparams& hp = h->cfg.hp;
  set_adam(ad, lr, hp.beta1, hp.beta2, hp.adam_eps, hp.tau);
  set_step(ad, step);
  ad.do_polyak = polyak ? 1 : 0;
  ad.do_adam = h->cfg.export_grads ? 0 : 1;
  ad.grad_scale = grad_scale;
  return ad;
}

// Does a slice launch of net `n` at batch B run on tensor-parallel clusters (slice_tp.hip)?  One
// predicate for the launch and for the dW kernel that has to sum the dz1 partials it leaves.
bool tp_generic(const oprl_learner* h, const oprl_net& n, int B) {
  if (!h->tp_generic_on || h->xbuf == nullptr) return false;
  if (h->ln.on && &n != &h->cfg.actor) return false;            // (critics with LN run the single-CU LN kernels, ln_slice.hip)
  if (n.n_layers != 3 || n.dims[1] != 256 || n.dims[2] != 256) return false;
  if (n.dims[0] > 96 || n.dims[3] > kNarrowMax) return false;
  if (((h->S & 15) + h->A - 1) / 16 >= 4) return false;          // input-gradient column span
  const int slices = n_slices(B);
  return slices * 4 <= h->n_cus;
}

hipError_t launch_dw_prof(const oprl_learner* h, DwArgs a, hipStream_t st) {
  if (h != nullptr) a.no_wide = h->sw.no_wide_dw ? 1 : 0;
  prof_begin(1, st);
  hipError_t e = launch_dw_adam(a, st);
  prof_end(st);
  return e;
}

const double* alpha_ptr(const oprl_learner* h) {
  const bool learned = h->cfg.algo == OPRL_TQC || ((h->cfg.algo == OPRL_SAC || h->cfg.algo == OPRL_REDQ) && h->cfg.hp.tune_alpha);
  return learned ? h->cfg.log_alpha : nullptr;
}

// the tanh-Gaussian actor (output 2A, reparameterised draws, entropy term): SAC, TQC, REDQ
bool gauss_actor(const oprl_learner* h) {
  return h->cfg.algo == OPRL_SAC || h->cfg.algo == OPRL_TQC || h->cfg.algo == OPRL_REDQ;
}

// Philox key of noise stream `stream_id` (1: next-state draw / TD3 smoothing, 2: actor-step draw, 3: REDQ's target subset;
// 4, 5: the CQL mode's draws; 6: the dropout masks of the LN critics, kDropStream).
// Seed 0 on rank 0 is the bare stream constant; anything else is mixed in (splitmix64 finaliser).
unsigned long long noise_key(uint64_t seed, int rank, uint64_t stream_id) {
  uint64_t x = seed ^ ((uint64_t)rank * 0x9E3779B97F4A7C15ULL);
  if (x != 0) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    x ^= x >> 31;
  }
  return 0x0b5e55edULL + stream_id + x;
}

// REDQ's target subset (include/oprl_amd.h oprl_redq_subset): a partial Fisher-Yates shuffle of 0 .. n-1 driven by the
// words of Philox blocks (stream 3, counter `counter`, block index in the third counter word)
void redq_subset(uint64_t seed, int rank, uint64_t counter, int n, int m, int* out) {
  const unsigned long long key = noise_key(seed, rank, 3);
  int perm[OPRL_MAX_CRITICS];
  for (int i = 0; i < n; ++i) perm[i] = i;
  u32x4 blk = {0, 0, 0, 0};
  for (int i = 0; i < m; ++i) {
    if ((i & 3) == 0)
      blk = philox4x32_10(u32x4{(uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)(i >> 2), 0u}, (uint32_t)key,
                          (uint32_t)(key >> 32));
    const uint32_t w = (i & 3) == 0 ? blk.x : (i & 3) == 1 ? blk.y : (i & 3) == 2 ? blk.z : blk.w;
    const int j = i + (int)bounded_u32(w, (uint32_t)(n - i));
    const int t = perm[i]; perm[i] = perm[j]; perm[j] = t;
    out[i] = perm[i];
  }
}

// ------------------------------------------------------------ fused DDPG / TD3
bool actor_due(const oprl_learner* h);

// grid rows of one update of k_ddpg_chain at batch B: 16 role rows + the tile-only rows of small batches (16 x 64 tiles)
int chain_rows(const oprl_learner* h, int B) {
  int tiles64[2] = {0, 0};
  for (size_t i = 0; i < h->items_host.size(); ++i)
    tiles64[(int)i < h->n_items_critic ? 0 : 1] += ((h->items_host[i].N + 15) / 16) * ((h->items_host[i].K + 63) / 64);
  const int sl = n_slices(B), mt = tiles64[0] > tiles64[1] ? tiles64[0] : tiles64[1];
  return 16 + chain_tile_rows(mt, sl);
}

// The launch form of a fused update of batch B, read off the learner (dp_inline: this update's gradient exchange runs
// inside the dW tiles — debug_form also asks it of a learner not set up for that).  Each condition is named once, in order.
FusedForm fused_form(const oprl_learner* h, int B, bool dp_inline) {
  const oprl_learner_config& c = h->cfg;
  const Switches& sw = h->sw;
  const int slices = n_slices(B);
  const bool sac = c.algo == OPRL_SAC;
  FusedForm f;
  f.nc = h->nc_cluster(B);
  f.xnc = h->xnc;
  f.lean = fused_ddpg_is_lean(f.nc, sw.no_lean, h->S, h->A, sac);
  f.x2 = h->x2 && f.lean;       // the PrecX2 instances: every net through its packs of two fp16 planes
  f.bf16 = h->bf16 && f.lean;   // the PrecBF16 instances of the (lean) phase kernels: every net through its bf16 packs
  const bool side_by_side = !sw.no_side_by_side && !h->group_member;
  // role A and the role-C cluster wait for each other: only with all four roles of a slice resident
  f.twin_split = (h->nc == 2 && f.nc == 4 && !sw.no_lean && side_by_side && (2 + h->nc) * 4 * slices <= h->n_cus) ? 1 : 0;
  // (SAC) both phase-2 clusters of a slice must be co-resident: cluster 0 waits for cluster 1's result
  f.p2_pair = (sac && h->ncl == 4 && 2 * 4 * slices <= h->n_cus && side_by_side) ? 1 : 0;
  if (!f.lean) return f;
  const bool x2_tiles = f.x2 && fused_x2_tiles();   // the 16 x 64 PrecX2 tiles
  // (one update's workgroups wait for each other in the whole-update launch: all must fit the chip)
  const bool fits = chain_rows(h, B) * slices <= h->n_cus;

  // clusters of EIGHT for role A (DDPG: the roles then fill the chip exactly at B = 256) and for phase 2's
  // critic pass (DDPG / TD3), while the launch still fits the chip; exact-fp32 lean passes only
  // A property of the LEARNER (oprl_learner_set_cluster(h, 8) = the default / (h, 4) = never), not of the
  // moment: results differ in the last bits between cluster sizes (summation order of the exchanges).  A wide
  // launch wants the whole chip; FOUR such launches each cut in the middle of role A (64 members resident, 64
  // waiting for a CU) fill it with workgroups that spin for each other — measured with eight learners on eight
  // streams: every wait ran into its bound and was reported.  Learners that share a GPU with more than two
  // others (packed seeds on streams, one process per seed on one GPU) turn it off: set_cluster(h, 4) or
  // OPRL_AMD_NO_WIDE=1; up to three cannot dead-lock (the B roles always finish and free their CUs).
  const bool wide_ok = h->xnc >= 8 && !h->shared_chip && !sw.no_wide && !sac && (!f.bf16 || h->bchain) && h->A <= 8;   // (narrow exchanges)
  const bool wide_a = wide_ok && h->nc == 1 && (f.nc + 8 + f.nc) * slices <= h->n_cus;
  const bool wide_p2 = wide_ok && (8 + 1) * slices <= h->n_cus;

  // the whole update per launch with the exact-fp32 tiles (learners with mirrored packs: k_ddpg_chain<PrecF32>) or the
  // bf16 ones (k_ddpg_chain<PrecBF16>: learner_internal.h bchain), when that form is possible at all (a gradient-exporting
  // learner takes it only when its tiles exchange the gradients themselves: dp_inline)
  const bool whole_ok = fused_x2_tiles() && !sw.no_whole && !sw.no_merge && !sw.no_merge2 && !h->shared_chip &&
                        (!c.export_grads || dp_inline) && B <= 256 && wide_a && wide_p2 && h->chain_flags != nullptr &&
                        h->du_granules != nullptr && fits;
  const bool whole_f32 = whole_ok && h->fchain && !f.x2 && !f.bf16;
  const bool whole_bf16 = whole_ok && h->bchain && f.bf16;
  const bool own_tiles = x2_tiles || whole_f32 || whole_bf16;     // tiles that take role A on eight beside them

  // (dp_inline: the gradient exchange inside the dW tiles — the 16 x 32 tiles of k_dw_adam<true> as launches of their own,
  // or the 16 x 64 tiles of the merged / whole-update launches themselves: dw_tile_x2.h — PrecX2 learners in both forms,
  // exact-fp32 and bf16 learners in the whole-update form, round 6)
  const bool inline_tiles = dp_inline && fused_x2_tiles() && h->nc == 1 && (f.x2 || whole_f32 || whole_bf16);
  const bool dp_ok = !dp_inline || inline_tiles;

  // merged phase 1 (DDPG, lean passes, one 256-row chunk, this rank's own Adam step): the critic's dW tiles ride on phase
  // 1 — whose role A then stays on a cluster of four unless the tiles are the 16 x 64 ones: 64 CUs must be free for tile
  // workgroups from the start (a gradient-exporting learner — data parallel over RCCL — merges only with the PrecX2
  // tiles, which know how to leave dW in the gradient arena instead of running Adam: four launches per data-parallel
  // update instead of six).  TD3: both critics' tiles ride — roles A | B1 | B2 | C are the whole chip at B = 256, the
  // 2 x 84 / 2 x 152 tiles take the compute units the roles leave; this rank's own Adam step only
  const bool merge_twin = h->nc == 2 && c.algo == OPRL_TD3 && !c.export_grads && !dp_inline && !sw.no_merge_twin;
  const bool xport_ok = !c.export_grads || x2_tiles || inline_tiles;
  const bool merged1 = !sw.no_merge && !h->shared_chip && (h->nc == 1 || merge_twin) && !sac && B <= 256 && xport_ok && dp_ok;
  // merged phase 2: the ACTOR's tiles on phase 2 (DDPG / TD3: the tanh head, action_dim <= kDuLd): the tiles form their
  // dY from du, the first layer's comes from one more backward step of the critic pass's members (csrc/fused_ddpg.hip);
  // the pass on clusters of eight.  PrecX2 learners, or inside the whole form: with the exact-fp32 tiles on its own the
  // merged form measured no faster than the two launches (34.9 vs 34.7 us)
  const bool merged2 = !sw.no_merge2 && !h->shared_chip && own_tiles && h->du_granules != nullptr && !sac && B <= 256 &&
                       dp_ok && c.actor.theta_target != nullptr && wide_p2;

  // the whole update as ONE launch: both merged forms, role A and the critic pass on eight, the 16 x 64 tiles, and
  // everything the roles hand to each other in uncached memory
  f.whole = (!sw.no_whole && (!c.export_grads || inline_tiles) && own_tiles && h->nc == 1 && merged1 && merged2 &&
             wide_a && wide_p2 && h->uc_pool && (h->uc_base != nullptr || h->bchain) && h->w_flags != nullptr &&
             h->chain_flags != nullptr && fits) ? 1 : 0;
  const bool merged2_on = merged2 && (f.x2 || f.whole);           // (exact fp32: no merged phase 2 outside the whole form)
  // (an exchanging rank outside PrecX2 has the in-tile exchange in the whole-update form only: whatever kept that form
  // away, its merged phase launch — 16 x 32 tiles that exchange nothing — must not run either)
  const bool merges = !dp_inline || f.x2 || f.whole;
  f.merged = merges ? ((merged1 ? 1 : 0) | (merged2_on ? 2 : 0)) : 0;
  // (outside the whole form a bf16 learner's passes stay on clusters of four, as before; role A stays on four beside
  // tiles other than the 16 x 64 ones, and beside the exact-fp32 tiles outside the whole form)
  const bool wide_on = !h->bchain || whole_bf16;
  const bool a_on_four = (merged1 && !own_tiles) || (merged2 && !merged2_on);
  f.wide = wide_on ? ((wide_a && !a_on_four ? 1 : 0) | (wide_p2 ? 2 : 0)) : 0;
  f.chain_max = f.whole ? sw.chain_max : 1;

  // Over-subscribed plain phase-1 launches (B >= 512: the roles' clusters need more compute units than the chip has, the
  // launch is several dispatch rounds): the B roles carry TWO row tiles per cluster — half the workgroups, one fetch of the
  // critic's fragments per 32 rows (tp4.h tp4_scalar_fb2; bit-identical to the one-tile form).  Slices a multiple of 16: a
  // cluster's members then sit on one XCD (fused_ddpg.hip role_b2).
  // (twin critics only — TD3, SAC: their two B roles then share the first dispatch round; measured, r06-6: SAC humanoid
  // B = 1024 - 3.7 us per update in every mode, TD3 B = 512 - 4.7, SAC B = 512 - 5; a single critic's one B role on half the
  // workgroups only lengthens the wait of role A behind it: DDPG B = 512 + 1.8 us, B = 1024 + 2.4 .. 4)
  f.rt2 = (sw.no_rt2 != 1 && h->nc == 2 && f.merged == 0 && (f.wide & 1) == 0 && f.nc == 4 && (slices & 15) == 0 &&
           (2 + h->nc) * 4 * slices > h->n_cus) ? 1 : 0;
  // SAC there: role A's first pass — the online actor on s' — also carries role C's pass, the same actor on s (tp4_forward2;
  // bit-identical): role C's dispatch round is not launched (r06-13; OPRL_AMD_NO_RT2=2 keeps role C)
  // (where role A alone fills the chip — humanoid B = 1024: -3.1 us x2, -2.1 f32 / bf16 per update; at B = 512 role C ran
  // beside role A's second half and the merged pass is 3.5 us SLOWER: a tile's pass is bound by instruction issue, not by
  // its fragments, so the second tile costs a pass's 6.4 us, not the 2 - 3 us the B roles' shared fragments suggested)
  if (f.rt2 == 1 && sac && !f.twin_split && sw.no_rt2 == 0 && 4 * slices >= h->n_cus) f.rt2 = 2;
  return f;
}

// The kernel's arguments of a fused update of batch B: the form (fused_form) and the pointers and scalars it needs.
DdpgArgs ddpg_args(oprl_learner* h, const StepRows& rows, int B) {
  const oprl_learner_config& c = h->cfg;
  const FusedForm f = fused_form(h, B, h->dp_inline);
  DdpgArgs a;
  memset(&a, 0, sizeof a);
  a.actor = net_view(eff(h, c.actor), false);
  a.actor_t = net_view(eff(h, c.actor), true);
  a.critic = net_view(eff(h, c.critics[0]), false);
  a.critic_t = net_view(eff(h, c.critics[0]), true);
  a.n_critics = h->nc;
  a.do_actor = 1;
  if (h->nc == 2) {      // TD3 / SAC: twin critic
    a.critic2 = net_view(c.critics[1], false);
    a.critic2_t = net_view(c.critics[1], true);
    for (int l = 0; l < kMaxLayers; ++l) { a.c2X[l] = h->ws_critic[1].X[l]; a.c2dY[l] = h->ws_critic[1].dY[l]; }
    a.rng_seed = noise_key(h, 1);                         // the streams seed_rng() gives the generic path
    a.rng_ctr = (unsigned long long)h->update_count;
  }
  if (c.algo == OPRL_TD3) {   // target-policy smoothing (td3.py:83-93), delayed actor steps
    a.smooth = 1;
    a.policy_noise = (float)c.hp.policy_noise;
    a.noise_clip = (float)c.hp.noise_clip;
    a.max_action = (float)c.hp.max_action;
    a.do_actor = actor_due(h) ? 1 : 0;
  }
  if (c.algo == OPRL_SAC) {   // tanh-Gaussian actor, entropy term (sac.py:90-141)
    a.sac = 1;
    a.noise_pi = h->noise1_pending;
    a.rng_seed_pi = noise_key(h, 2);
    a.log_alpha = alpha_ptr(h);
    a.alpha_const = (float)c.hp.alpha_init;
    a.raw = h->raw;
    a.logp = h->logp;
  }
  a.B = B; a.S = h->S; a.A = h->A;
  a.src = rows.cur;
  a.next = rows.next;
  a.gamma = (float)c.hp.gamma;
  a.inv_B = 1.0f / (float)B;
  for (int l = 0; l < kMaxLayers; ++l) {
    a.cX[l] = h->ws_critic[0].X[l]; a.cdY[l] = h->ws_critic[0].dY[l];
    a.aX[l] = h->ws_actor.X[l];     a.adY[l] = h->ws_actor.dY[l];
  }
  a.cldx0 = h->ws_critic[0].ldx0; a.clddo = h->ws_critic[0].lddo;
  a.aldx0 = h->ws_actor.ldx0;     a.alddo = h->ws_actor.lddo;
  a.pi = h->pi;
  a.y_out = h->ydbg; a.q_out = h->qdbg;
  a.y_granules = h->y_granules; a.gran_stride = h->Bmax;
  a.gate_flags = h->y_granules + (size_t)3 * h->Bmax;   // 256 flag granules behind the TD / q granules
  a.seed2_granules = h->y_granules + (size_t)3 * h->Bmax + 256;
  a.epoch = h->epoch;
  a.no_lean = h->sw.no_lean;
  a.xcd_local = h->xcd_local ? 1 : 0;
  a.xbuf = h->xbuf;
  a.cdY0_stride = h->ws_critic[0].dY0_stride;
  a.adY0_stride = h->ws_actor.dY0_stride;
  a.partials_c = h->part_c; a.partials_a = h->part_a;
  a.err = h->err_dev;
  a.debug_expire = h->debug_expire;
  a.w3_src = c.actor.theta + w_off(c.actor, c.actor.n_layers - 1);
  a.nc = f.nc; a.xnc = f.xnc; a.x2 = f.x2; a.bf16 = f.bf16; a.wide = f.wide; a.twin_split = f.twin_split;
  a.p2_pair = f.p2_pair; a.merged = f.merged; a.whole = f.whole; a.rt2 = f.rt2;
  if (f.x2 || f.bf16) {     // every net through its 16-bit packs (x2: two fp16 planes per block)
    const int pl = f.x2 ? 2 : 1;
    a.actor = net_view16(c.actor, false, h->pack16[0], pl);
    if (c.actor.theta_target) a.actor_t = net_view16(c.actor, true, h->pack16_t[0], pl);
    a.critic = net_view16(c.critics[0], false, h->pack16[1], pl);
    a.critic_t = net_view16(c.critics[0], true, h->pack16_t[1], pl);
    if (h->nc == 2) {
      a.critic2 = net_view16(c.critics[1], false, h->pack16[2], pl);
      a.critic2_t = net_view16(c.critics[1], true, h->pack16_t[2], pl);
    }
  }
  if (f.whole && f.bf16) a.actor_pb1_f32 = net_view(c.actor, false).pb[1];
  if ((f.merged & 2) != 0) {
    a.du_granules = h->du_granules;
    a.g1_granules = h->g1_granules;
    a.w3_snap = h->w3_snap;
  }
  if (f.whole) {
    a.w_flags = h->w_flags;
    a.ct_done = h->w_flags + 64;
    for (int l = 0; l < c.critics[0].n_layers; ++l) a.critic_b16[l] = h->critic_b16 + 256 * l;
  }
  return a;
}

// DDPG runs fused for every batch size (generic tp3.h passes when the lean ones do not fit);
// TD3's and SAC's fused kernels exist in the lean form only, otherwise the generic launch sequence is used
bool use_fused(const oprl_learner* h, int B) {
  if (!h->fused) return false;
  if (h->cfg.algo == OPRL_DDPG) return true;
  return fused_form(h, B, h->dp_inline).lean;
}

// The temperature step of this update as a job for the actor's dW launch (one more workgroup), when nothing
// but this rank's own Adam step is wanted of it; otherwise (gradient export, exchange inside the dW launch)
// the caller launches k_alpha_step itself (alpha_step).
bool alpha_rides(const oprl_learner* h) {
  return alpha_ptr(h) != nullptr && !h->cfg.export_grads && !h->dp_inline;
}
AlphaJob alpha_job(const oprl_learner* h, int B, int step) {
  const oprl_learner_config& c = h->cfg;
  AlphaJob j;
  j.log_alpha = c.log_alpha; j.m = c.log_alpha_m; j.v = c.log_alpha_v; j.logp = h->logp; j.B = B;
  j.target_entropy = (float)c.hp.target_entropy;
  j.lr = c.hp.lr_alpha; j.beta1 = c.hp.beta1; j.beta2 = c.hp.beta2; j.eps = c.hp.adam_eps;
  j.bc1 = 1.0 - std::pow(c.hp.beta1, (double)step);
  j.bc2_sqrt = std::sqrt(1.0 - std::pow(c.hp.beta2, (double)step));
  return j;
}

// The temperature's Adam step as a launch of its own (k_alpha_step), step `step`: B > 0 from this update's log pi
// (a gradient-exporting learner also leaves the gradient in alpha_grad), B = 0 from the all-reduced gradient in alpha_grad
hipError_t alpha_step(const oprl_learner* h, int B, int step, float grad_scale, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  const bool from_grad = B == 0;
  return launch_alpha_step(c.log_alpha, c.log_alpha_m, c.log_alpha_v, from_grad ? nullptr : h->logp, from_grad ? 1 : B,
                           (float)c.hp.target_entropy, c.hp.lr_alpha, c.hp.beta1, c.hp.beta2, c.hp.adam_eps, step,
                           !from_grad && c.export_grads ? h->alpha_grad : nullptr, from_grad ? h->alpha_grad : nullptr,
                           grad_scale, st);
}

// this update's temperature step where it did not ride on the actor's dW launch
int temperature_step(oprl_learner* h, int B, hipStream_t st) {
  if (alpha_ptr(h) == nullptr || alpha_rides(h)) return OPRL_OK;
  HIPC(alpha_step(h, B, h->opt_step_alpha + 1, 1.0f, st));
  h->opt_step_alpha += 1;
  return OPRL_OK;
}

// The dW + Adam (+ Polyak) launch of the critic(s) or the actor at batch B as the optimiser's step `step`.  Reads the
// learner only: the caller commits the step (dw_commit) once the launch that carries it is out.  B = 0: the data-parallel
// apply, fed from the all-reduced gradient arena (w_g / b_g) instead of the GEMM.
// The critic's targets move when critic_targets_due (TD3: on actor steps only, td3.py:135-146), the actor's when it has any.
DwArgs dw_args(const oprl_learner* h, bool critic, int B, int step) {
  const oprl_learner_config& c = h->cfg;
  DwArgs dw;
  dw.items = h->items_host.data() + (critic ? 0 : h->n_items_critic);
  dw.n_items = critic ? h->n_items_critic : h->n_items_actor;
  dw.total_tiles = critic ? h->tiles_critic : h->tiles_actor;
  dw.ad = adam_scalars(h, critic ? c.hp.lr_critic : c.hp.lr_actor, step,
                       critic ? critic_targets_due(h) : c.actor.theta_target != nullptr, 1.0f);
  dw.B = B;
  if (B == 0) {
    dw.apply_only = 1;
    return dw;
  }
  dw.trace = h->trace != nullptr ? h->trace + (size_t)(critic ? 4 : 5) * 64 * kTraceStamps * 2 : nullptr;   // slot 4 / 5
  if (use_fused(h, B)) {
    // the lean phase 1 leaves unit-seed dz rows (tp4_scalar_fb): each critic's TD-error seed, dY of its output layer, is
    // applied per row (DwItem::rs); the lean passes leave tile-major dz1 partials
    const bool lean = fused_form(h, B, h->dp_inline).lean;
    dw.n_part = h->nc_cluster(B);
    dw.use_row_scale = (critic && lean) ? 1 : 0;
    dw.dy_tiled = (lean && dw.n_part > 1) ? 1 : 0;
    dw.skip32 = (h->x2 && lean && !c.export_grads) ? 1 : 0;     // the PrecX2 kernels read the fp16 packs only (fresh32)
  } else {
    dw.n_part = tp_generic(h, critic ? c.critics[0] : c.actor, B) ? 4 : 1;
    dw.dy_tiled = dw.n_part > 1 ? 1 : 0;               // k_mlp_slice_tp runs the tp4 passes
    // TQC in a 16-bit mode: the critics' 512 x 512 layers run through the 16-bit packs (layerwise.hip); their fp32
    // packs — a third of the wide dW launch's stores — are left stale and rebuilt by whoever reads them (fresh32)
    dw.skip32_wide = (critic && c.algo == OPRL_TQC && (h->x2 || h->bf16) && h->lazy_wide && !c.export_grads &&
                      !h->sw.no_layerwise) ? 1 : 0;
  }
  return dw;
}

// The launch of `dw` is out: its optimiser has taken `steps` steps (and the temperature's one, if it rode), and the fp32
// packs it did not write (skip32, skip32_wide) or wrote the uncached mirrors of (fchain) fall behind the masters
void dw_commit(oprl_learner* h, bool critic, const DwArgs& dw, int steps) {
  (critic ? h->opt_step_critic : h->opt_step_actor) += steps;
  if (dw.alpha.log_alpha != nullptr) h->opt_step_alpha += 1;
  if (dw.skip32 || h->fchain) h->stale32[critic ? 0 : 1] = true;
  if (dw.skip32_wide) h->stale_wide = true;
}

// the peer-window exchange of a data-parallel dW launch whose (first) exchange has sequence number `seq`
DwXchg xchg_args(const oprl_learner* h, unsigned long long seq) {
  const P2pState& P = h->p2p;
  DwXchg X;
  memset((void*)&X, 0, sizeof X);
  for (int r = 0; r < kDwXchgMaxWorld; ++r) X.peer[r] = r < P.world ? P.peer[r] + P.tile_off : nullptr;
  X.window = P.window + P.tile_off;
  X.world = P.world; X.rank = P.rank; X.max_tiles = h->p2p_max_tiles;
  X.seq = seq; X.parity = (int)(seq & 1);
  X.err = h->err_dev;
  return X;
}

// one dW + Adam launch of its own (the actor's carries the temperature step where it rides)
int dw_step(oprl_learner* h, bool critic, int B, hipStream_t st, const PrefetchJob* prefetch) {
  DwArgs dw = dw_args(h, critic, B, (critic ? h->opt_step_critic : h->opt_step_actor) + 1);
  if (!critic && alpha_rides(h)) dw.alpha = alpha_job(h, B, h->opt_step_alpha + 1);
  dw.prefetch = prefetch;
  const unsigned long long seq = h->p2p.tile_seq + 1;
  if (h->dp_inline) {
    // data-parallel on peer windows: this launch all-reduces its tiles itself and runs Adam on the mean
    h->dw_xchg = xchg_args(h, seq);
    dw.xchg = &h->dw_xchg;
    dw.ad.do_adam = 1;
    dw.ad.grad_scale = 1.0f / (float)h->p2p.world;
  }
  if (dw.n_items > kDwMaxItems) {
    // (REDQ's ensemble: more layers than one launch's table holds — launches of at most kDwMaxItems layers, each with the
    // same step count and so the same Adam scalars; a riding job goes with the last)
    if (h->dp_inline || dw.prefetch != nullptr) { set_err("internal: a split dW table with an exchange or riders"); return OPRL_ERR_STATE; }
    DwArgs part = dw;
    for (int i0 = 0; i0 < dw.n_items; i0 += kDwMaxItems) {
      part.items = dw.items + i0;
      part.n_items = std::min(kDwMaxItems, dw.n_items - i0);
      part.alpha = i0 + kDwMaxItems >= dw.n_items ? dw.alpha : AlphaJob{};
      HIPC(launch_dw_prof(h, part, st));
    }
  } else {
    HIPC(launch_dw_prof(h, dw, st));
  }
  dw_commit(h, critic, dw, 1);
  if (h->dp_inline) h->p2p.tile_seq = seq;
  return OPRL_OK;
}

// ------------------------------------------------------------ critic phase
// The gates of the dW tiles that ride on a phase launch (DwGate): the common fields of the critic's tiles (phase 1's
// roles flag their rows, the TD-error seeds come as granules, one per row) ...
void critic_gate(const oprl_learner* h, const DdpgArgs& fa, int B, DwGate& g) {
  const int slices = n_slices(B);
  g.rows = fa.gate_flags; g.n_rows = 4 * slices * h->nc;
  g.seed = fa.y_granules; g.n_seed = B;
  g.late_dY = h->ws_critic[0].dY[h->cfg.critics[0].n_layers - 1];
  g.tag = h->epoch; g.spin = h->debug_expire == 7 ? 0 : (1 << 20);
  g.err = h->err_dev; g.err_code = (1u << 8) | 7u;      // KERN_PHASE1, SITE_DW_GATE (csrc/tp3.h)
}
// ... and of the actor's tiles (they wait for the du granules; items = the actor's layers 0, 1, 2)
void actor_gate(const oprl_learner* h, const DdpgArgs& fa, int B, DwGate& g) {
  g.seed = fa.du_granules; g.n_seed = B;
  g.tag = h->epoch; g.spin = h->debug_expire == 7 ? 0 : (1 << 20);
  g.err = h->err_dev; g.err_code = (2u << 8) | 7u;      // KERN_PHASE2, SITE_DW_GATE (csrc/tp3.h)
  g.kind[0] = 2; g.kind[1] = 1; g.kind[2] = 0; g.kind[3] = 0;
  g.h2 = h->ws_actor.X[2];
  g.w3 = fa.w3_snap;
  g.g1 = fa.g1_granules;
  g.n_act = h->A;
}

// The whole update as k_ddpg_chain launches: phase 1's roles, the critic's tiles, role U + the actor's tiles, the critic
// pass, of U updates (rows.n_upd) per launch.  What the launch advances — the optimisers' step counts, the epochs,
// the exchange tags and, data parallel, this rank's tile sequence — is committed once it is out: after an error return
// Adam's bias corrections and the peers' sequence numbers are where they were.
int whole_update(oprl_learner* h, StepRows& rows, DdpgArgs& fa, const FusedForm& form, int B, hipStream_t st) {
  const int slices = n_slices(B);
  const int U = rows.n_upd < form.chain_max ? rows.n_upd : form.chain_max;
  const int step_c = h->opt_step_critic + 1, step_a = h->opt_step_actor + 1;     // update 0's
  fa.prefetch_next = 0;
  DwKArgs kd;
  DwKArgs4 kc, ka;
  auto compact = [&](const DwKArgs& k, DwKArgs4* o) {
    for (int j = 0; j < kDwFusedItems; ++j) { o->tile_end[j] = k.tile_end[j]; o->items[j] = k.items[j]; }
    o->n_items = k.n_items; o->B = k.B; o->n_part = k.n_part; o->dy_tiled = k.dy_tiled; o->ad = k.ad; o->trace = k.trace;
    o->gate = k.gate;
    memset((void*)&o->xchg, 0, sizeof o->xchg);
  };
  const DwArgs dc = dw_args(h, true, B, step_c);
  if (fill_dw_kargs(dc, &kd, 64) < 0 || dc.n_items > kDwFusedItems) { set_err("whole update: bad critic dW table"); return OPRL_ERR_INVALID; }
  critic_gate(h, fa, B, kd.gate);
  kd.gate.done = fa.ct_done; kd.gate.what_if = h->debug_expire;
  fa.n_ct = kd.tile_end[kDwMaxItems - 1];
  if (fa.n_ct > 192 - 64) { set_err("whole update: too many critic tiles"); return OPRL_ERR_INVALID; }
  compact(kd, &kc);
  const DwArgs da = dw_args(h, false, B, step_a);
  if (fill_dw_kargs(da, &kd, 64) < 0 || da.n_items != 3) { set_err("whole update: bad actor dW table"); return OPRL_ERR_INVALID; }
  actor_gate(h, fa, B, kd.gate);
  kd.gate.what_if = h->debug_expire;
  compact(kd, &ka);
  // (every tile must find a role-B / role-C workgroup to be the continuation of: 8 per slice)
  const int max_tiles = kc.tile_end[kDwFusedItems - 1] > ka.tile_end[kDwFusedItems - 1] ? kc.tile_end[kDwFusedItems - 1] : ka.tile_end[kDwFusedItems - 1];
  const int t_rows = chain_tile_rows(max_tiles, slices);
  // (the form's fit test counted the same 16 x 64 tiles from the learner's item table: chain_rows)
  if (16 + t_rows != chain_rows(h, B)) { set_err("internal: whole update of %d grid rows, the form counted %d", 16 + t_rows, chain_rows(h, B)); return OPRL_ERR_STATE; }
  const unsigned long long seq = h->p2p.tile_seq + 1;
  if (h->dp_inline) {
    // data parallel on peer windows: the tiles of this launch all-reduce their gradients themselves and run Adam on
    // the mean (dw_tile_x2.h): exchange sequence numbers seq + 2 u (critic) / + 1 (actor) for update u of the launch
    if (max_tiles > h->p2p_max_tiles) { set_err("data-parallel whole update: the windows hold %d tiles, the launch has %d", h->p2p_max_tiles, max_tiles); return OPRL_ERR_STATE; }
    kc.xchg = xchg_args(h, seq);
    kc.xchg.parity = 0;           // (parity = the exchange's sequence number & 1, formed in the tile)
    ka.xchg = kc.xchg;
    kc.ad.do_adam = 1; ka.ad.do_adam = 1;
    kc.ad.grad_scale = 1.0f / (float)h->p2p.world; ka.ad.grad_scale = 1.0f / (float)h->p2p.world;
  }
  // SEVERAL updates as one launch (k_ddpg_chain): the tables above are update 0's; what changes per update — Adam's
  // bias-correction terms, epochs, exchange tags, the staging set — is in ChainArgs
  ChainArgs ca;
  memset((void*)&ca, 0, sizeof ca);
  ca.n_upd = U;
  ca.first_gather = fa.src.gather;
  ca.pf_last = rows.stage_after_last ? 1 : 0;
  ca.trace_u = U - 1;
  ca.rows = 16 + t_rows;
  ca.order = h->sw.chain_order;
  ca.mS = row_div_magic(fa.S); ca.mA = row_div_magic(fa.A); ca.mSA = row_div_magic(fa.S + fa.A);      // (idiv.h)
  // (the optimisers' step counts advance once per update and net: only Adam's bias-correction terms change from update
  // to update — a table build per update and net was 8 of the 17 us a step_n(20) call took to enqueue)
  AdamScalars sc_ = kc.ad, sa_ = ka.ad;
  for (int u = 0; u < U; ++u) {
    set_step(sc_, step_c + u);
    set_step(sa_, step_a + u);
    ca.c_step[u] = sc_.step_size_host; ca.c_bc2[u] = sc_.bc2_sqrt_host;
    ca.a_step[u] = sa_.step_size_host; ca.a_bc2[u] = sa_.bc2_sqrt_host;
  }
  ca.set0[0] = fa.src.s; ca.set0[1] = fa.src.a; ca.set0[2] = fa.src.r; ca.set0[3] = fa.src.d; ca.set0[4] = fa.src.s2;
  for (int i = 0; i < 5; ++i) ca.set1[i] = rows.other_set[i];
  if ((U > 1 || ca.pf_last) && ca.set1[0] == nullptr) { set_err("chain launch: no second staging set"); return OPRL_ERR_STATE; }
  ca.ct_fin = h->chain_flags; ca.at_fin = h->chain_flags + 192; ca.pf_done = h->chain_flags + 384;
  for (int w = 0; w < 4; ++w)
    for (int l = 0; l < kMaxLayers; ++l) ca.b16[w][l] = h->chain_b16 + ((size_t)w * kMaxLayers + l) * 256;
  ca.w3buf[0] = h->w3_snap; ca.w3buf[1] = h->w3buf1;
  // the first hidden layer's dY from the unit-seed rows the pass's members leave before the pass (DwGate kind 3)
  ca.qp = h->chain_flags + 576;
  fa.gu = h->gu; fa.gu_flags = h->chain_flags + 448;
  ka.gate.kind[0] = 3; ka.gate.gu = h->gu; ka.gate.gu_flags = fa.gu_flags; ka.gate.n_gu_flags = 8 * slices;
  if (kc.tile_end[kDwFusedItems - 1] > 192 || ka.tile_end[kDwFusedItems - 1] > 192 || slices > 64) { set_err("chain launch: too many tiles"); return OPRL_ERR_INVALID; }
  // exchange tags: two per update (the roles', the critic pass's), consecutive: cluster_tag = the first
  unsigned tag = h->tp_tag;
  if ((tag & 0x03FFFFFFu) + 2u * (unsigned)U + 2u >= 0x03FFFFFFu) {      // (would wrap inside the launch: wrap now)
    tag = (tag | 0x03FFFFFFu) + 1u;
    HIPC(hipMemsetAsync(h->xbuf, 0, h->xbuf_granules * sizeof(unsigned long long), st));
  }
  fa.cluster_tag = (tag + 1u) & 0x03FFFFFFu;
  fa.prefetch_p1 = 0;
  fa.trace2 = fa.trace != nullptr ? h->trace + (size_t)3 * 64 * kTraceStamps * 2 : nullptr;   // slot 3
  prof_begin(4, st);
  hipError_t e;
  {
    std::lock_guard<std::mutex> lk(g_turn.mu);
    int dev = 0;
    e = chip_turn_begin(st, &dev);
    if (e == hipSuccess) e = launch_ddpg_chain(fa, kc, ka, ca, st);
    if (e == hipSuccess) chip_turn_end(st, dev);
  }
  prof_end(st);
  HIPC(e);
  dw_commit(h, true, dc, U);
  dw_commit(h, false, da, U);
  if (h->dp_inline) {
    h->p2p.tile_seq += 2ull * (unsigned long long)U;
    h->stale32[0] = true; h->stale32[1] = true;  // (the tiles write the fp16 packs only)
  }
  h->tp_tag = tag + 2u * (unsigned)U;
  h->epoch += (unsigned)(U - 1);
  h->whole_done = true;
  rows.staged = rows.stage_after_last;                 // the launch's last update staged the next rows: set (cur + U) & 1
  return OPRL_OK;
}

// phase 1 of a fused update — or the whole update, or phase 1 with the critic's dW tiles — and the critic's dW + Adam
static int fused_critic_phase(oprl_learner* h, StepRows& rows, int B, const float* noise0, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  h->epoch += 1;
  if (h->epoch == 0 || h->epoch > 0xFFFFFFFFu - (unsigned)kChainMax) {   // the TD-target tag wrapped (or would inside a chain launch): retire every stale granule
    h->epoch = 1;
    HIPC(hipMemsetAsync(h->y_granules, 0, ((size_t)4 * h->Bmax + 256) * sizeof(unsigned long long), st));
    if (h->du_granules != nullptr) {
      HIPC(hipMemsetAsync(h->du_granules, 0, (size_t)(h->Bmax < 256 ? h->Bmax : 256) * kDuLd * sizeof(unsigned long long), st));
      HIPC(hipMemsetAsync(h->g1_granules, 0, (size_t)16 * (h->Bmax < 256 ? h->Bmax : 256) * 16 * sizeof(unsigned long long), st));
      HIPC(hipMemsetAsync(h->w_flags, 0, 256 * sizeof(unsigned long long), st));
      HIPC(hipMemsetAsync(h->chain_flags, 0, (192 + 192 + 64 + 128 + 1024) * sizeof(unsigned long long), st));
    }
  }
  const FusedForm form = fused_form(h, B, h->dp_inline);
  DdpgArgs fa = ddpg_args(h, rows, B);
  if (h->x2 && !fa.x2) RC(fresh32_tables(h, 3, st));     // (a batch the lean kernels do not take: fp32 packs)
  fa.noise = noise0;
  if (rows.stage == StepRows::kPhase1) {
    // (step_n asks phase 1 to stage only for a form with merged bits, which the rt2 form never has)
    if (fa.rt2 != 0) { set_err("internal: phase 1 asked to stage the next rows in the rt2 form"); return OPRL_ERR_STATE; }
    fa.prefetch_p1 = 1;
    rows.staged = true;
  }
  if (h->trace != nullptr) fa.trace = h->trace;   // roles use slots 0 .. 1 + n_critics
  h->whole_done = false;
  if (form.whole) return whole_update(h, rows, fa, form, B, st);
  RC(next_tp_tag(&h->tp_tag, h->xbuf, h->xbuf_granules * sizeof(unsigned long long), st, &fa.cluster_tag));
  if ((fa.merged & 1) != 0) {
    // phase 1 and the critic's dW + Adam tiles as ONE launch: the tiles wait for the roles' flag granules
    const DwArgs dw = dw_args(h, true, B, h->opt_step_critic + 1);
    DwKArgs kd;
    if (fill_dw_kargs(dw, &kd, ((fa.x2 && fused_x2_tiles()) || (h->nc == 2 && fused_tile64_all())) ? 64 : 32) < 0) { set_err("merged phase 1: bad dW table"); return OPRL_ERR_INVALID; }
    critic_gate(h, fa, B, kd.gate);
    if (h->nc == 2) {      // (twin critics: the second one's items, seeds and output-layer dY)
      kd.gate.item_split = c.critics[0].n_layers;
      kd.gate.seed2 = fa.seed2_granules;
      kd.gate.late_dY2 = h->ws_critic[1].dY[c.critics[1].n_layers - 1];
    }
    RC(profiled(4, st, [&] { return launch_ddpg_phase1_dw(fa, kd, st); }));
    dw_commit(h, true, dw, 1);
    return OPRL_OK;
  }
  RC(profiled(4, st, [&] { return launch_ddpg_phase1(fa, st); }));
  return dw_step(h, true, B, st);
}

// The two phases of an update: the fused launches where the learner has them at this batch (use_fused), else the generic
// launch sequence (learner_generic.hip)
int critic_phase(oprl_learner* h, StepRows& rows, int B, const float* noise0, hipStream_t st) {
  if (rows.w != nullptr && (use_fused(h, B) || h->cfg.algo == OPRL_TQC || h->cfg.algo == OPRL_D4PG)) {      // (the entry point refuses all three)
    set_err("internal: importance weights reached a launch form that does not apply them");
    return OPRL_ERR_STATE;
  }
  return use_fused(h, B) ? fused_critic_phase(h, rows, B, noise0, st) : generic_critic_phase(h, rows, B, noise0, st);
}

// ------------------------------------------------------------- actor phase
// phase 2 of a fused update (with the actor's dW tiles where they ride), the actor's dW + Adam and the temperature step
static int fused_actor_phase(oprl_learner* h, StepRows& rows, int B, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  DdpgArgs fa = ddpg_args(h, rows, B);
  if (h->x2 && !fa.x2) RC(fresh32_tables(h, 3, st));
  RC(next_tp_tag(&h->tp_tag, h->xbuf, h->xbuf_granules * sizeof(unsigned long long), st, &fa.cluster_tag));
  if (h->trace != nullptr && c.algo == OPRL_DDPG) fa.trace = h->trace + (size_t)3 * 64 * kTraceStamps * 2;   // slot 3
  else if (h->trace != nullptr && h->nc == 2) fa.trace = h->trace + (size_t)6 * 64 * kTraceStamps * 2;      // twin critics: roles 0 .. 3 are phase 1's, slot 6
  fa.prefetch_next = rows.stage == StepRows::kPhase2 ? 1 : 0;
  // Where phase 2's own workgroups already fill the chip (SAC at B = 1024: 4 x 64), its prefetch row is a round of
  // its own; the actor's dW launch, which follows and leaves 40 % of the chip idle, carries the row instead
  // (prefetch_rows_direct, the same rows).
  bool pf_on_dw = false;
  PrefetchJob pj;
  {
    const int slices = n_slices(B);
    const int grid_rows = (fa.wide & 2) != 0 ? 8 : fa.nc * ((fa.sac && fa.p2_pair) ? 2 : 1);
    if (fa.prefetch_next && (grid_rows + 1) * slices > h->n_cus && !h->dp_inline) {
      pf_on_dw = true;
      fa.prefetch_next = 0;
      memset((void*)&pj, 0, sizeof pj);
      pj.next = fa.next; pj.S = h->S; pj.A = h->A; pj.B = B; pj.z0 = -1;
    }
  }
  if (rows.stage == StepRows::kPhase2) rows.staged = true;
  if ((fa.merged & 2) != 0 && !pf_on_dw) {
    // phase 2 and the actor's dW + Adam tiles as ONE launch: the tiles wait for the du (first layer: dz1) granules
    const DwArgs dw = dw_args(h, false, B, h->opt_step_actor + 1);
    DwKArgs kd;
    if (fill_dw_kargs(dw, &kd, (fa.x2 && fused_x2_tiles()) ? 64 : 32) < 0 || dw.n_items != 3) { set_err("merged phase 2: bad dW table"); return OPRL_ERR_INVALID; }
    actor_gate(h, fa, B, kd.gate);
    RC(profiled(5, st, [&] { return launch_ddpg_phase2_dw(fa, kd, st); }));
    dw_commit(h, false, dw, 1);
    return OPRL_OK;
  }
  RC(profiled(5, st, [&] { return launch_ddpg_phase2(fa, st); }));
  RC(dw_step(h, false, B, st, pf_on_dw ? &pj : nullptr));
  return temperature_step(h, B, st);      // SAC temperature (sac.py:129-141), from role C's log pi
}

int actor_phase(oprl_learner* h, StepRows& rows, int B, const float* noise1, hipStream_t st) {
  if (h->whole_done) {          // (this update's actor step ran inside the critic phase's launch: k_ddpg_update)
    h->whole_done = false;
    return OPRL_OK;
  }
  return use_fused(h, B) ? fused_actor_phase(h, rows, B, st) : generic_actor_phase(h, rows, B, noise1, st);
}

// master -> packs for a list of nets (which: bit0 online, bit1 target).  The item
// table goes through a small device scratch; synchronous on `st` only.
void build_repack_items(const oprl_net* const* nets, int n_nets, int which,
                        std::vector<RepackItem>& items, int* blocks_out,
                        float* const* pk16, float* const* pk16_t, int pl) {
  int blocks = 0;
  for (int i = 0; i < n_nets; ++i) {
    const oprl_net& n = *nets[i];
    for (int pass = 0; pass < 2; ++pass) {
      if (!(which & (1 << pass))) continue;
      const float* base = pass == 0 ? n.theta : n.theta_target;
      float* pk = pass == 0 ? n.pack : n.pack_target;
      if (!base || !pk) continue;
      for (int l = 0; l < n.n_layers; ++l) {
        RepackItem it;
        it.w = base + w_off(n, l);
        it.N = n.dims[l + 1]; it.K = n.dims[l];
        it.pf = pk + pack_off_fwd(n, l);
        it.pb = pass == 0 ? pk + pack_off_bwd(n, l) : nullptr;
        float* p16 = pass == 0 ? (pk16 ? pk16[i] : nullptr) : (pk16_t ? pk16_t[i] : nullptr);
        it.pf16 = p16 ? p16 + pack16_off_fwd(n, l, pl) : nullptr;
        it.pb16 = (p16 && pass == 0) ? p16 + pack16_off_bwd(n, l, pl) : nullptr;
        it.x2 = pl == 2 ? 1 : 0;
        it.blk_begin = blocks;
        blocks += (int)(((long)it.N * it.K + 255) / 256);
        it.blk_end = blocks;
        items.push_back(it);
      }
    }
  }
  *blocks_out = blocks;
}

int repack_nets(const oprl_net* const* nets, int n_nets, int which, hipStream_t st,
                float* const* pk16, float* const* pk16_t, int pl) {
  std::vector<RepackItem> items;
  int blocks = 0;
  build_repack_items(nets, n_nets, which, items, &blocks, pk16, pk16_t, pl);
  if (items.empty()) return OPRL_OK;
  RepackItem* dev = nullptr;
  HIPC(hipMalloc(&dev, sizeof(RepackItem) * items.size()));
  hipError_t e = hipMemcpyAsync(dev, items.data(), sizeof(RepackItem) * items.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_repack(dev, (int)items.size(), blocks, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(dev);
  HIPC(e);
  return OPRL_OK;
}

// Does this update take an actor step?  TD3: on every policy_freq-th, counted from the first (td3.py:135); REDQ: on the
// last of every G = policy_freq updates, (u + 1) % G == 0
bool actor_due(const oprl_learner* h) {
  if (h->cfg.algo == OPRL_REDQ) return (h->update_count + 1) % h->cfg.hp.policy_freq == 0;
  return h->cfg.algo != OPRL_TD3 || (h->update_count % h->cfg.hp.policy_freq == 0);
}

// Do the critic targets take their Polyak step in this update?  TD3: with the actor (td3.py:135-146); REDQ: on every update
bool critic_targets_due(const oprl_learner* h) {
  return h->cfg.algo == OPRL_REDQ || actor_due(h);
}

int check_batch(const oprl_learner* h, const void* s, const void* a, const void* r, const void* d,
                const void* s2, int B) {
  if (!h) { set_err("null learner handle"); return OPRL_ERR_INVALID; }
  if (!s || !a || !r || !d || !s2) { set_err("update: null batch pointer"); return OPRL_ERR_INVALID; }
  if (B < 1 || B > h->Bmax) { set_err("update: batch %d outside [1, max_batch=%d]", B, h->Bmax); return OPRL_ERR_INVALID; }
  return OPRL_OK;
}

// Has a kernel of this learner reported an expired wait?  (Sticky until oprl_learner_clear_error.)

int check_device_error(const oprl_learner* h) {
  if (h == nullptr || h->err_host == nullptr) return OPRL_OK;
  const unsigned code = *(volatile const unsigned*)h->err_host;
  if (code == 0) return OPRL_OK;
  static const char* kern[] = {"?", "k_ddpg_phase1", "k_ddpg_phase2", "k_mlp_slice_tp", "k_dw_adam<exchange>", "peer-window all-reduce", "k_lw_mid_pair"};
  static const char* site[] = {"?", "cluster all-reduce (a member of a 4-CU slice cluster never published its partial)",
                               "TD-target hand-off (role B never received y from role A)",
                               "twin-target exchange between role A and the role-C cluster",
                               "SAC phase 2 pair exchange (critic 2's cluster never delivered)",
                               "gradient tile exchange with another rank", "peer-window flag of another rank",
                               "gate of the dW tiles riding on a phase launch (a role never flagged its rows / seeds)",
                               "hand-over inside a layer-by-layer launch (a producing workgroup — first hidden layer, riding tail, action-gradient rows — never flagged its rows)"};
  const unsigned k = (code >> 8) & 0xff, w = code & 0xff;
  if (w == 9) {     // SITE_X2_RANGE (csrc/tp3.h): not a wait
    set_err("device error 0x%x: an activation left the range of the split-fp16 mode (precision='x2': |x| < 4094 for observations and "
            "hidden activations, |w| < 256 for weights) in %s; the results of that update (and everything after it) are poisoned.  "
            "Normalise the observations or create the learner with precision='f32' (exact fp32, no such range).  Restore a "
            "checkpoint, then oprl_learner_clear_error().", code, k < 7 ? kern[k] : "?");
    return OPRL_ERR_STATE;
  }
  set_err("device error 0x%x: a bounded cross-workgroup wait expired in %s at the %s; the results of that "
          "update (and everything after it) are poisoned with NaN.  Typical causes: the launch's workgroups were "
          "not co-resident (another process or learner held the GPU's compute units for longer than the wait bound), "
          "or a data-parallel peer died.  Restore a checkpoint, then oprl_learner_clear_error() — after which this learner "
          "runs the launch forms for a shared GPU (set_cluster(4): no workgroup waits for another role of its own launch).",
          code, k < 7 ? kern[k] : "?", w < 9 ? site[w] : "?");
  return OPRL_ERR_STATE;
}

}  // namespace oprl_host

// =========================================================================== C-ABI
extern "C" const char* oprl_last_error(void) { return g_err.c_str(); }

extern "C" int oprl_learner_check(oprl_learner* h) {
  if (!h) { set_err("null learner handle"); return OPRL_ERR_INVALID; }
  return check_device_error(h);
}

extern "C" int oprl_learner_clear_error(oprl_learner* h) {
  if (!h) { set_err("null learner handle"); return OPRL_ERR_INVALID; }
  if (h->err_host) {
    // A bounded wait that expired inside a launch whose workgroups wait for each other ACROSS roles (the whole-update
    // and merged launches: tiles for roles, the critic pass for tiles) means those workgroups were not running side by
    // side — the chip is shared (another process, an eval / actor process on the same GPU, a partitioned device).  The
    // learner then goes on, after the caller's restore, with the forms that cross a kernel boundary instead:
    // set_cluster(< 8) semantics, as for learners that share a GPU by design.
    const unsigned code = *(volatile unsigned*)h->err_host, w = code & 0xff;
    if (code != 0 && w != 9 /* SITE_X2_RANGE */ && w != 5 && w != 6 /* data-parallel peers */ && !h->debug_expire && !h->shared_chip) {
      h->shared_chip = true;     // (and so: no merged or whole-update form, no clusters of eight)
    }
    // (an expired wait of any kind: the cluster exchanges go back to agent-scope publishes as well — if a member sat on an
    // XCD the others did not expect, the demoted forms must not repeat it)
    if (code != 0 && w != 9 && !h->debug_expire) h->xcd_local = false;
    *(volatile unsigned*)h->err_host = 0;
  }
  return OPRL_OK;
}

extern "C" int oprl_redq_subset(uint64_t seed, int32_t rank, uint64_t counter, int32_t n, int32_t m, int32_t* out_host) {
  if (!out_host || rank < 0 || m < 1 || n < m || n > OPRL_MAX_CRITICS) {
    set_err("oprl_redq_subset: need 1 <= m <= n <= %d (n=%d, m=%d), rank >= 0 and an output array", OPRL_MAX_CRITICS, n, m);
    return OPRL_ERR_INVALID;
  }
  int out[OPRL_MAX_CRITICS];
  redq_subset(seed, rank, counter, n, m, out);
  for (int i = 0; i < m; ++i) out_host[i] = out[i];
  return OPRL_OK;
}

extern "C" int oprl_debug_noise(oprl_learner* h, int32_t stream_id, uint64_t counter, int32_t rows, int32_t cols,
                                float* out_dev, void* stream) {
  if (!h || stream_id < 1 || stream_id > 2 || rows < 1 || cols < 1 || !out_dev) { set_err("oprl_debug_noise: invalid argument"); return OPRL_ERR_INVALID; }
  HIPC(launch_debug_normal(noise_key(h, (uint64_t)stream_id), counter, rows, cols, out_dev, (hipStream_t)stream));
  return OPRL_OK;
}

extern "C" int oprl_learner_debug_expire(oprl_learner* h, int32_t site) {
  if (!h || site < 0 || (site > 8 && (site < 101 || site > 106 || site == 103))) { set_err("oprl_learner_debug_expire: invalid argument"); return OPRL_ERR_INVALID; }
  // (101 .. 106 are TIMING experiments — a cross-workgroup wait counts as satisfied, the update computes wrong parameters and
  // reports nothing: refused unless the process opted in, tools/what_if.py sets the variable)
  if (site > 8) {
    const char* e = getenv("OPRL_AMD_WHAT_IF");
    if (e == nullptr || atoi(e) == 0) { set_err("oprl_learner_debug_expire: sites 101..106 are timing experiments that corrupt the update; set OPRL_AMD_WHAT_IF=1 to allow them"); return OPRL_ERR_STATE; }
  }
  h->debug_expire = site;
  h->lw_pairs.spin = site == 8 ? 0 : (1 << 20);      // (8: the hand-over inside k_lw_mid_pair)
  return OPRL_OK;
}


extern "C" int oprl_profile_enable(int32_t on) {
  if (!on) prof_fold();
  g_prof.on = on != 0;
  return OPRL_OK;
}

extern "C" int oprl_profile_read(int64_t* counts_host, double* ms_host, int32_t reset) {
  if (!counts_host || !ms_host) { set_err("oprl_profile_read: null argument"); return OPRL_ERR_INVALID; }
  prof_fold();
  for (int k = 0; k < OPRL_PROFILE_KINDS; ++k) {
    counts_host[k] = g_prof.counts[k];
    ms_host[k] = g_prof.ms[k];
    if (reset) { g_prof.counts[k] = 0; g_prof.ms[k] = 0; }
  }
  return OPRL_OK;
}
extern "C" int oprl_abi_version(void) { return OPRL_ABI_VERSION; }

namespace oprl_host {
int learner_update_phase(oprl_learner* h, int phase, StepRows& rows, int B, const float* noise0, const float* noise1, void* stream) {
  RC(check_batch(h, rows.cur.s, rows.cur.a, rows.cur.r, rows.cur.d, rows.cur.s2, B));
  if (h->cql.cal_on && rows.g == nullptr) {
    set_err("update: the learner's calibrated mode is on (oprl_learner_set_calql) and these rows carry no returns-to-go; "
            "oprl_learner_update_calql takes them, oprl_learner_step_n computes them");
    return OPRL_ERR_STATE;
  }
  if (!h->cql.cal_on && rows.g != nullptr) {
    set_err("update: returns-to-go for a learner whose calibrated mode is off (oprl_learner_set_calql)");
    return OPRL_ERR_STATE;
  }
  RC(cql_rows_fit(h, "update", B));
  RC(check_device_error(h));      // an expired wait of an earlier launch (asynchronous: whatever has run by now)
  hipStream_t st = (hipStream_t)stream;
  h->last_B = B;
  if (phase == 0) h->trace_slot = 0;
  h->noise1_pending = noise1;
  if (phase == 0) return critic_phase(h, rows, B, noise0, st);
  if (phase == 1) {
    h->actor_updated_last = actor_due(h);
    int rc = OPRL_OK;
    if (h->actor_updated_last) rc = actor_phase(h, rows, B, noise1, st);
    if (rc == OPRL_OK) h->update_count += 1;
    return rc;
  }
  set_err("phase must be 0 or 1");
  return OPRL_ERR_INVALID;
}

int learner_update(oprl_learner* h, StepRows& rows, int B, const float* noise0, const float* noise1, void* stream) {
  RC(learner_update_phase(h, 0, rows, B, noise0, noise1, stream));
  return learner_update_phase(h, 1, rows, B, noise0, noise1, stream);
}
}  // namespace oprl_host

extern "C" int oprl_learner_update_phase(oprl_learner* h, int32_t phase, const float* s, const float* a, const float* r, const float* d,
                                         const float* s2, int32_t B, const float* noise0, const float* noise1, void* stream) {
  StepRows rows = plain_rows(s, a, r, d, s2);
  return learner_update_phase(h, phase, rows, B, noise0, noise1, stream);
}

extern "C" int oprl_learner_update(oprl_learner* h, const float* s, const float* a, const float* r, const float* d,
                                   const float* s2, int32_t B, const float* noise0, const float* noise1, void* stream) {
  StepRows rows = plain_rows(s, a, r, d, s2);
  return learner_update(h, rows, B, noise0, noise1, stream);
}

// The two-call path of the calibrated mode (oprl_learner_set_calql): g[B] are the rows' returns-to-go
// (oprl_replay_returns), which cql_critic_step hands to the calibrated seed kernel.
extern "C" int oprl_learner_update_calql(oprl_learner* h, const float* s, const float* a, const float* r, const float* d,
                                         const float* s2, const float* g, int32_t B, const float* noise0, const float* noise1,
                                         void* stream) {
  if (!h) { set_err("oprl_learner_update_calql: null learner handle"); return OPRL_ERR_INVALID; }
  if (!g) { set_err("oprl_learner_update_calql: null returns-to-go pointer"); return OPRL_ERR_INVALID; }
  StepRows rows = plain_rows(s, a, r, d, s2);
  rows.g = g;
  return learner_update(h, rows, B, noise0, noise1, stream);
}

extern "C" int oprl_learner_apply(oprl_learner* h, int32_t phase, double grad_scale, void* stream) {
  if (!h) { set_err("null learner handle"); return OPRL_ERR_INVALID; }
  if (!h->cfg.export_grads) { set_err("oprl_learner_apply: learner was not created with export_grads"); return OPRL_ERR_STATE; }
  RC(check_device_error(h));
  if (phase != 0 && phase != 1) { set_err("phase must be 0 or 1"); return OPRL_ERR_INVALID; }
  const bool critic = phase == 0;
  if (!critic && !h->actor_updated_last) return OPRL_OK;
  hipStream_t st = (hipStream_t)stream;
  // one launch: k_dw_adam's epilogue (Adam, Polyak, packs written in pack order) fed from the all-reduced gradient arena
  // instead of the GEMM — replaces k_adam_flat + k_repack — at the step update_phase counted when it took the gradient
  // (dw_args' Polyak test for the critic: update_count is not advanced before phase 1)
  DwArgs dw = dw_args(h, critic, 0, critic ? h->opt_step_critic : h->opt_step_actor);
  dw.ad.do_adam = 1;
  dw.ad.grad_scale = (float)grad_scale;
  HIPC(launch_dw_prof(h, dw, st));
  dw_commit(h, critic, dw, 0);
  if (!critic && alpha_ptr(h) != nullptr) HIPC(alpha_step(h, 0, h->opt_step_alpha, (float)grad_scale, st));
  return OPRL_OK;
}

namespace oprl_host {
int RowStager::check(const char* who, const oprl_learner* h, const oprl_replay* replay, bool packed, int K, int B, int* nstep) {
  int S = 0, A = 0;
  replay_dims(replay, &S, &A);
  if (S != h->S || A != h->A) { set_err("replay dims (%d,%d) != %s dims (%d,%d)", S, A, packed ? "group" : "learner", h->S, h->A); return OPRL_ERR_INVALID; }
  if (K < 0 || B < 1 || B > h->Bmax) { set_err("%s: bad K/B", who); return OPRL_ERR_INVALID; }
  // An n-step replay (oprl_replay_set_nstep): the in-kernel gathers read one-step rows, so such a replay
  // goes through the callers' sample + update loops; the update still takes its fused form on the sampled rows.
  double gamma = 0.0;
  replay_nstep(replay, nstep, &gamma);
  if (*nstep > 1 && packed) {     // the members gather their rows inside the group's launches, one step at a time
    set_err("%s: the replay samples %d-step returns (oprl_replay_set_nstep); packed learners take one-step replays only", who, *nstep);
    return OPRL_ERR_STATE;
  }
  if (*nstep > 1 && gamma != h->cfg.hp.gamma) {
    set_err("%s: the replay's %d-step gamma %.17g is not the learner's %.17g (the sampler's gamma^(m-1) multiplies the learner's gamma)",
            who, *nstep, gamma, h->cfg.hp.gamma);
    return OPRL_ERR_INVALID;
  }
  // A hindsight replay (oprl_replay_set_her) is read through its own gather in the same way.
  if (replay_her(replay) > 0 && packed) {
    set_err("%s: the replay relabels goals in hindsight (oprl_replay_set_her); packed learners take plain replays only", who);
    return OPRL_ERR_STATE;
  }
  // A replay with prior data (oprl_replay_set_prior) likewise: its rows come from two storages.
  if (replay_prior(replay) != 0 && packed) {
    set_err("%s: the replay mixes prior data into its batches (oprl_replay_set_prior); packed learners take plain replays only", who);
    return OPRL_ERR_STATE;
  }
  return OPRL_OK;
}

// The kernels gather their own rows (same Philox draw / index map as k_replay_gather): the first update in its slice
// kernels, every later one from a staging set that a launch of the update before it has filled.
int RowStager::open(const char* who, const oprl_learner* h, oprl_replay* replay, uint64_t seed, void* stream) {
  RC(oprl_replay_flush(replay, stream));
  rows = StepRows{};
  BatchSrc& v = rows.cur;
  long n_tr = 0;
  replay_view(replay, &v.states, &v.actions, &v.rewards, &v.dones, &v.ends, &v.n_eps, &v.L, &n_tr);
  if (n_tr <= 0 || v.n_eps <= 0) { set_err("%s: replay buffer is empty", who); return OPRL_ERR_STATE; }
  v.n_transitions = n_tr;
  v.gather = 1;
  rows.next = v;
  bind(h, seed);
  return OPRL_OK;
}

void RowStager::bind(const oprl_learner* h, uint64_t seed) {
  rows.cur.seed = rows.next.seed = seed;
  const size_t Bm = (size_t)h->Bmax;
  const size_t off[5] = {0, Bm * h->S, Bm * (h->S + h->A), Bm * (h->S + h->A + 1), Bm * (h->S + h->A + 2)};
  float* const own[5] = {h->bs, h->ba, h->br, h->bd, h->bs2};
  for (int i = 0; i < 5; ++i) { set[0][i] = own[i]; set[1][i] = h->batch_alt != nullptr ? h->batch_alt + off[i] : own[i]; }
}

// The coming update reads set[cur]: staged there, else gathered by its own kernels.  Phase-1 staging fills the other set,
// whose rows the update's own roles are not reading, and the sets alternate; phase-2 staging fills the set it has read.
// K_left > 0: a k_ddpg_chain launch of U = min(K_left, chain_max) updates instead — update u of the launch stages the rows
// of update u + 1 into the other set, the last one only when updates are left; the next launch reads set (cur + U) & 1.
StepRows& RowStager::plan(const oprl_learner* h, StepRows::Stage stage, int K_left) {
  const int U = K_left < h->sw.chain_max ? K_left : h->sw.chain_max;      // (0: not a chain launch)
  const bool other = stage == StepRows::kPhase1 || U > 0;
  float* const* b = set[cur];
  float* const* nb = set[other ? cur ^ 1 : cur];
  BatchSrc &c = rows.cur, &n = rows.next;
  c.s = b[0]; c.a = b[1]; c.r = b[2]; c.d = b[3]; c.s2 = b[4];
  n.s = nb[0]; n.a = nb[1]; n.r = nb[2]; n.d = nb[3]; n.s2 = nb[4];
  c.counter = (unsigned long long)h->update_count;
  n.counter = c.counter + 1;
  c.gather = staged ? 0 : 1;
  rows.stage = stage;
  rows.n_upd = U > 0 ? U : 1;
  rows.stage_after_last = U > 0 && U < K_left;
  for (int i = 0; i < 5; ++i) rows.other_set[i] = U > 0 ? set[cur ^ 1][i] : nullptr;
  rows.staged = false;
  flip = other ? rows.n_upd : 0;
  return rows;
}

// step_n's K-loop as launches of up to chain_max updates each (k_ddpg_chain).  Also the data-parallel loop when the gradient
// exchange is inside the tiles.
int chain_loop(oprl_learner* h, RowStager& stg, int K, int B, void* stream) {
  for (int k = 0; k < K;) {
    StepRows& rows = stg.plan(h, StepRows::kNone, K - k);
    RC(learner_update(h, rows, B, nullptr, nullptr, stream));
    h->update_count += rows.n_upd - 1;                  // (learner_update() counted one)
    k += rows.n_upd;
    stg.done();
  }
  return OPRL_OK;
}

// does step_n at this batch run as chain launches?
bool chain_ok(oprl_learner* h, int B) {
  return fused_form(h, B, h->dp_inline).whole && h->batch_alt != nullptr;
}
}  // namespace oprl_host

extern "C" int oprl_learner_step_n(oprl_learner* h, oprl_replay* replay, int32_t K, int32_t B,
                                   uint64_t seed, void* stream) {
  if (!h || !replay) { set_err("oprl_learner_step_n: null handle"); return OPRL_ERR_INVALID; }
  if (h->cfg.export_grads) { set_err("step_n is the single-GPU fused path; export_grads learners use update_phase/apply"); return OPRL_ERR_STATE; }
  int nstep = 1;
  RC(RowStager::check("step_n", h, replay, false, K, B, &nstep));
  RC(cql_rows_fit(h, "step_n", B));
  if (h->cql.cal_on && replay_her(replay) > 0) {      // (before anything is launched; oprl_replay_returns would say the same after the sample)
    set_err("step_n: the learner's calibrated mode is on (oprl_learner_set_calql) and the replay relabels goals in hindsight "
            "(oprl_replay_set_her): its rewards are relabelled per sample, so its slots have no returns-to-go");
    return OPRL_ERR_STATE;
  }
  RowStager stg;
  // else (n-step, hindsight or prior-data rows): the sample + update loop at the end
  const bool plain = nstep == 1 && replay_her(replay) == 0 && replay_prior(replay) == 0;
  if (plain && use_fused(h, B)) {
    RC(stg.open("step_n", h, replay, seed, stream));
    // k_ddpg_chain: up to chain_max updates per launch, the rows of update u + 1 staged by update u inside the launch
    if (chain_ok(h, B)) return chain_loop(h, stg, K, B, stream);
    // Otherwise phase 2 of every update that has one gathers the next update's rows into the set it has read.  With the
    // merged phase 2 (whose roles fill the chip) PHASE 1 carries them — every update, TD3's critic-only ones included — into
    // the other of the two sets, since its own roles are still reading theirs ...
    const FusedForm probe = fused_form(h, B, h->dp_inline);
    // (... and TD3's merged twin launches in every arithmetic, r06-15: without the merged phase 2 — exact fp32, bf16 — a
    // critic-only update had no launch that staged the next rows, and the update behind it gathered its own inside the roles'
    // first stage: 4.8 us against 2.9 before the first barrier of every role of every second launch)
    const bool td3_p1 = h->cfg.algo == OPRL_TD3 && (probe.merged & 1) != 0 && !h->sw.no_p1_rows;
    const bool p1 = h->batch_alt != nullptr && ((probe.merged & 2) != 0 || td3_p1);
    for (int k = 0; k < K; ++k) {
      RC(learner_update(h, stg.plan(h, k + 1 == K ? StepRows::kNone : p1 ? StepRows::kPhase1 : StepRows::kPhase2), B, nullptr, nullptr, stream));
      stg.done();
    }
    return OPRL_OK;
  }
  if (plain && h->cfg.algo == OPRL_TQC && h->batch_alt != nullptr && !h->sw.no_gather_ride && K > 1) {
    // the rows of update k + 1 are gathered by riders of update k's k_lw_dact launch (same draw as k_replay_gather)
    // into the other of two sets of batch rows; only the first update's rows are a launch
    RC(stg.open("step_n", h, replay, seed, stream));
    int rc = OPRL_OK;
    for (int k = 0; k < K && rc == OPRL_OK; ++k) {
      StepRows& rows = stg.plan(h, StepRows::kPhase1);    // (the sets alternate as under phase-1 staging)
      float* const* b = stg.set[stg.cur];
      if (rows.cur.gather)
        rc = oprl_replay_sample(replay, B, nullptr, seed, (uint64_t)h->update_count, b[0], b[1], b[2], b[3], b[4], nullptr, nullptr, stream);
      h->prefetch_done = false;
      h->prefetch_pending = false;
      if (rc == OPRL_OK && k + 1 < K) {
        memset((void*)&h->prefetch, 0, sizeof h->prefetch);
        h->prefetch.next = rows.next;
        h->prefetch.S = h->S; h->prefetch.A = h->A; h->prefetch.B = B; h->prefetch.z0 = -1;
        h->prefetch_pending = true;
      }
      rows.cur.gather = 0;                                // the generic launches read plain rows and know no stage:
      rows.stage = StepRows::kNone;                       // the next rows travel as the offer above
      if (rc == OPRL_OK) rc = learner_update(h, rows, B, nullptr, nullptr, stream);
      h->prefetch_pending = false;
      rows.staged = h->prefetch_done;
      h->prefetch_done = false;
      stg.done();
    }
    return rc;
  }
  for (int k = 0; k < K; ++k) {
    if (h->cql.cal_on) {      // the sampler's slots -> their returns-to-go with the learner's gamma -> the calibrated update
      RC(oprl_replay_sample(replay, B, nullptr, seed, (uint64_t)h->update_count, h->bs, h->ba, h->br,
                            h->bd, h->bs2, h->cql.ep, h->cql.step, stream));
      RC(oprl_replay_returns(replay, B, h->cql.ep, h->cql.step, h->cfg.hp.gamma, h->cql.g, stream));
      RC(oprl_learner_update_calql(h, h->bs, h->ba, h->br, h->bd, h->bs2, h->cql.g, B, nullptr, nullptr, stream));
      continue;
    }
    RC(oprl_replay_sample(replay, B, nullptr, seed, (uint64_t)h->update_count, h->bs, h->ba, h->br,
                          h->bd, h->bs2, nullptr, nullptr, stream));
    RC(oprl_learner_update(h, h->bs, h->ba, h->br, h->bd, h->bs2, B, nullptr, nullptr, stream));
  }
  return OPRL_OK;
}

// ===================================================================== the trainer loop's step
extern "C" int oprl_learner_step_act(oprl_learner* h, oprl_replay* replay, int32_t B, uint64_t seed,
                                     const float* obs_host, void* stream) {
  if (!h || !replay || !obs_host) { set_err("oprl_learner_step_act: null argument"); return OPRL_ERR_INVALID; }
  const oprl_net& n = h->cfg.actor;
  if (n.n_layers < 1 || n.n_layers > kMaxLayers) { set_err("oprl_learner_step_act: bad actor"); return OPRL_ERR_INVALID; }
  for (int l = 0; l <= n.n_layers; ++l)
    if (n.dims[l] > kPolicyActMaxWidth) { set_err("oprl_learner_step_act: layer width %d > %d", n.dims[l], kPolicyActMaxWidth); return OPRL_ERR_INVALID; }
  if (h->act_pin == nullptr) {
    HIPC(hipHostMalloc((void**)&h->act_pin, (3 * kPolicyActMaxWidth + 16) * sizeof(float), hipHostMallocMapped));
    HIPC(hipHostGetDevicePointer((void**)&h->act_map, h->act_pin, 0));
    memset(h->act_pin, 0, (3 * kPolicyActMaxWidth + 16) * sizeof(float));
  }
  RC(oprl_learner_step_n(h, replay, 1, B, seed, stream));
  memcpy(h->act_pin, obs_host, sizeof(float) * n.dims[0]);
  PolicyActArgs a;
  memset(&a, 0, sizeof a);
  a.n_layers = n.n_layers;
  for (int l = 0; l <= n.n_layers; ++l) a.dims[l] = n.dims[l];
  for (int l = 0; l < n.n_layers; ++l) { a.w[l] = n.theta + w_off(n, l); a.b[l] = n.theta + b_off(n, l); }
  a.obs = h->act_map;
  a.out = reinterpret_cast<unsigned long long*>(h->act_map + kPolicyActMaxWidth);
  h->act_ticket += 1;
  if (h->act_ticket == 0) h->act_ticket = 1;
  a.ticket_value = h->act_ticket;
  HIPC(launch_policy_act(a, (hipStream_t)stream));
  h->act_pending = true;
  return OPRL_OK;
}

extern "C" int oprl_learner_act_wait(oprl_learner* h, float* out_host, int32_t n_out, int64_t timeout_us) {
  if (!h || !out_host) { set_err("oprl_learner_act_wait: null argument"); return OPRL_ERR_INVALID; }
  if (!h->act_pending) { set_err("oprl_learner_act_wait: no row is pending (oprl_learner_step_act first)"); return OPRL_ERR_STATE; }
  const oprl_net& n = h->cfg.actor;
  if (n_out != n.dims[n.n_layers]) { set_err("oprl_learner_act_wait: n_out %d != the actor's %d outputs", n_out, n.dims[n.n_layers]); return OPRL_ERR_INVALID; }
  const unsigned long long* g = reinterpret_cast<const unsigned long long*>(h->act_pin + kPolicyActMaxWidth);
  const auto t0 = std::chrono::steady_clock::now();
  long spins = 0;
  for (int i = 0; i < n_out; ++i) {
    unsigned long long x;
    while ((unsigned)((x = __atomic_load_n(g + i, __ATOMIC_ACQUIRE)) >> 32) != h->act_ticket) {
      if ((++spins & 1023) == 0 &&
          std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_us) {
        set_err("oprl_learner_act_wait: the policy row did not arrive within %lld us", (long long)timeout_us);
        return OPRL_ERR_STATE;
      }
      __builtin_ia32_pause();
    }
    const unsigned bits = (unsigned)x;
    memcpy(out_host + i, &bits, 4);
  }
  h->act_pending = false;
  return OPRL_OK;
}

