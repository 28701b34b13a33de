// learner_group.hip — packed learners (oprl_group_*): N independent learners stepped by one launch sequence.
// Split from learner.hip (round 4).
#include "learner_internal.h"

// ===================================================================== packed learners
// The reference trains several seeds as several processes (runners/train.py:36-50).  One DDPG learner at B = 256
// is a chain of four latency-bound launches that keeps a fraction of the chip busy; a GROUP steps N independent
// learners (own weights, own replay keys) with FOUR launches per update for all of them: grid.z = learner, the
// argument blocks in device memory.  Group members run the single-CU-per-slice passes (cluster size 1): no
// workgroup of such a launch waits for a later one, so the N x 48 phase-1 workgroups may simply queue behind
// each other on the 256 CUs, and a learner's result does not depend on who else is in the launch.
struct oprl_group {
  std::vector<oprl_learner*> L;
  // The argument blocks of kGroupChunk updates — per update [N x DdpgArgs phase 1][N x DdpgArgs phase 2][N x DwKArgsN<ni_c>
  // critic(s)][N x DwKArgsG actor] — are built ahead on the host and go up in ONE copy per chunk (four copies per update
  // of the 5 KB blocks stood for 56 of 424 us per group update of 32 members).
  char* dev = nullptr;                         // [kGroupChunk][bytes]
  char* stage[2] = {nullptr, nullptr};         // pinned host staging (double buffered), the same layout
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  bool stage_busy[2] = {false, false};
  int cur = 0;
  size_t bytes = 0;                            // one update's blocks
  int span = 1;                                // XCDs a member's slices are dealt out to (generic passes: 1)
  int ni_c = kDwGroupItems;                    // layers per critic-step dW block (twin critics: kDwGroupItems2)
  int device = 0;                              // the device the group's buffers (and its members) live on
};
constexpr int kGroupChunk = 4;

static void group_free(oprl_group* g) {
  if (g->dev) (void)hipFree(g->dev);
  for (int i = 0; i < 2; ++i) {
    if (g->stage[i]) (void)hipHostFree(g->stage[i]);
    if (g->stage_ev[i]) (void)hipEventDestroy(g->stage_ev[i]);
  }
  delete g;
}

extern "C" int oprl_group_create(oprl_learner** learners, int32_t n, oprl_group** out) {
  if (!learners || !out || n < 1 || n > 64) { set_err("oprl_group_create: invalid argument"); return OPRL_ERR_INVALID; }
  const int algo0 = learners[0] ? learners[0]->cfg.algo : -1;
  for (int i = 0; i < n; ++i) {
    oprl_learner* h = learners[i];
    if (h && h->bc.alpha > 0.0) {
      set_err("oprl_group_create: member %d has the behaviour-cloning mode on (oprl_learner_set_bc); packed learners run the fused launches, which have no BC step", i);
      return OPRL_ERR_STATE;
    }
    if (h && h->ln.on) {
      set_err("oprl_group_create: member %d has layer normalisation in its critics (oprl_learner_set_layernorm); packed learners run the fused launches, which have none", i);
      return OPRL_ERR_STATE;
    }
    if (h && h->iql.on) {
      set_err("oprl_group_create: member %d has the implicit-Q-learning mode on (oprl_learner_set_iql); packed learners run the fused launches, which have no value net", i);
      return OPRL_ERR_STATE;
    }
    if (!h || (algo0 != OPRL_DDPG && algo0 != OPRL_TD3 && algo0 != OPRL_SAC) || h->cfg.algo != algo0 || !h->fused || h->cfg.export_grads ||
        h->bf16 != learners[0]->bf16 || h->x2 != learners[0]->x2 || h->S != learners[0]->S || h->A != learners[0]->A ||
        h->Bmax != learners[0]->Bmax || h->cfg.hp.policy_freq != learners[0]->cfg.hp.policy_freq ||
        (alpha_ptr(h) != nullptr) != (alpha_ptr(learners[0]) != nullptr)) {
      set_err("oprl_group_create: member %d is not a fused DDPG / TD3 / SAC learner of the group's algorithm, shape and precision", i);
      return OPRL_ERR_INVALID;
    }
  }
  // The members' launch form.  Exact fp32: the generic single-CU-per-slice passes (cluster size 1) — no workgroup of such
  // a launch waits for another, and 32 members measure 71k updates/s against 58k on clusters of four.  bf16 / x2: the
  // lean passes on clusters of four (the only form these precisions exist in).  TD3 / SAC members (fused in the lean form
  // only): clusters of four in every precision.
  int group_nc = 4;
  {
    oprl_learner* h0 = learners[0];
    // (the lean passes on clusters of four, as the members will run them: nc_cluster with ncl = 4)
    const bool lean = 4 * n_slices(h0->Bmax) <= h0->n_cus && fused_ddpg_is_lean(4, h0->sw.no_lean, h0->S, h0->A, algo0 == OPRL_SAC);
    if (!lean || (algo0 == OPRL_DDPG && !h0->bf16 && !h0->x2)) group_nc = 1;
    if (group_nc == 1 && (h0->bf16 || h0->x2 || algo0 != OPRL_DDPG)) {
      set_err("oprl_group_create: TD3 / SAC members and the bf16 / x2 modes need nets the lean passes take (256-wide hidden layers, narrow inputs)");
      return OPRL_ERR_INVALID;
    }
  }
  auto* g = new oprl_group();
  g->L.assign(learners, learners + n);
  (void)hipGetDevice(&g->device);
  g->ni_c = learners[0]->nc == 2 ? kDwGroupItems2 : kDwGroupItems;
  g->span = 1;        // (a member's slices on one XCD: 2 / 4 / 8 measured slower, r03-39)
  g->bytes = (size_t)n * (2 * sizeof(DdpgArgs) + dw_group_block_bytes(g->ni_c) + dw_group_block_bytes(kDwGroupItems));
  bool ok = hipMalloc((void**)&g->dev, g->bytes * kGroupChunk) == hipSuccess;
  for (int i = 0; i < 2 && ok; ++i) {
    ok = hipHostMalloc((void**)&g->stage[i], g->bytes * kGroupChunk) == hipSuccess &&
         hipEventCreateWithFlags(&g->stage_ev[i], hipEventDisableTiming) == hipSuccess;
  }
  if (!ok) {      // (nothing is kept of a failed create: the partial allocations go, the members stay as they were)
    group_free(g);
    set_err("oprl_group_create: allocation failed");
    return OPRL_ERR_NOMEM;
  }
  // (a solo run for comparison: oprl_learner_set_cluster(h, 4) — the un-merged lean launches — or (h, 1))
  // (the twin critics' side-by-side forms want all of a slice's clusters resident at once: not in a queue of members)
  for (oprl_learner* h : g->L) { h->ncl = group_nc; h->shared_chip = true; h->group_member = true; }
  *out = g;
  return OPRL_OK;
}

extern "C" int oprl_group_destroy(oprl_group* g) {
  if (!g) return OPRL_OK;
  // the group's OWN device, whatever the caller's current one is: launches that read the argument blocks may be in flight
  int cur = 0;
  const int dev = g->device;
  (void)hipGetDevice(&cur);
  if (cur != dev) (void)hipSetDevice(dev);
  (void)hipDeviceSynchronize();
  group_free(g);
  if (cur != dev) (void)hipSetDevice(cur);
  return OPRL_OK;
}

extern "C" int oprl_learner_set_cluster(oprl_learner* h, int32_t nc) {
  if (!h || (nc != 1 && nc != 2 && nc != 4 && nc != 8)) { set_err("oprl_learner_set_cluster: cluster size must be 1, 2, 4 or 8"); return OPRL_ERR_INVALID; }
  // 8 = clusters of four, and of eight where the fused kernels have them (the default); 4 = never eight
  h->ncl = nc == 8 ? 4 : nc;
  // ... and a learner that shares the chip (anything but 8) keeps to the launch forms whose workgroups only wait within
  // their cluster: no clusters of eight, no tile workgroups riding on the phase launches (measured: 8 learners on 8
  // streams 47k -> 60k aggregate); with 8, clusters of eight unless h->sw.no_wide (fused_form)
  h->shared_chip = nc != 8;
  return OPRL_OK;
}

// K updates of every member: per update one H2D copy of the N x 4 argument blocks and four launches.
extern "C" int oprl_group_step_n(oprl_group* g, oprl_replay* replay, int32_t K, int32_t B, const uint64_t* seeds,
                                 void* stream) {
  if (!g || !replay || !seeds || K < 0) { set_err("oprl_group_step_n: invalid argument"); return OPRL_ERR_INVALID; }
  const int n = (int)g->L.size();
  oprl_learner* h0 = g->L[0];
  if (B < 1 || B > h0->Bmax) { set_err("oprl_group_step_n: bad batch %d", B); return OPRL_ERR_INVALID; }
  int nstep = 1;
  RC(RowStager::check("oprl_group_step_n", h0, replay, true, K, B, &nstep));
  hipStream_t st = (hipStream_t)stream;
  // everything that can be refused is checked BEFORE any member's counters move: the members advance together, so
  // being in phase now is being in phase for all K updates
  for (int l = 0; l < n; ++l) {
    RC(check_device_error(g->L[l]));
    if (actor_due(g->L[l]) != actor_due(h0) || g->L[l]->cfg.hp.policy_freq != h0->cfg.hp.policy_freq) {
      set_err("oprl_group_step_n: the members' delayed actor steps are out of phase (update counts differ modulo policy_freq)");
      return OPRL_ERR_STATE;
    }
  }
  // (what is left — an internal inconsistency of the launch tables — rolls the members' counters back to here)
  struct Snap { unsigned epoch, tp_tag; long long update_count; int oc, oa, oal; bool aul, s0, s1; };
  std::vector<Snap> snap(n);
  auto take = [&]() {
    for (int l = 0; l < n; ++l) {
      const oprl_learner* h = g->L[l];
      snap[l] = Snap{h->epoch, h->tp_tag, (long long)h->update_count, (int)h->opt_step_critic, (int)h->opt_step_actor, (int)h->opt_step_alpha,
                     h->actor_updated_last, h->stale32[0], h->stale32[1]};
    }
  };
  auto roll_back = [&](int rc) {
    for (int l = 0; l < n; ++l) {
      oprl_learner* h = g->L[l];
      const Snap& q = snap[l];
      h->epoch = q.epoch; h->tp_tag = q.tp_tag; h->update_count = q.update_count; h->opt_step_critic = q.oc; h->opt_step_actor = q.oa;
      h->opt_step_alpha = q.oal; h->actor_updated_last = q.aul; h->stale32[0] = q.s0; h->stale32[1] = q.s1;
    }
    return rc;
  };
  // every member's rows: the replay's one view under the member's own seed; phase 2 stages into the one set it reads
  std::vector<RowStager> rows_of(1);
  RC(rows_of[0].open("oprl_group_step_n", h0, replay, seeds[0], stream));
  rows_of.resize(n, rows_of[0]);
  for (int l = 0; l < n; ++l) {
    rows_of[l].bind(g->L[l], seeds[l]);
    g->L[l]->last_B = B;
  }
  static_assert(sizeof(DdpgArgs) % 8 == 0 && sizeof(DwKArgsG) % 8 == 0 && sizeof(DwKArgsG2) % 8 == 0, "the blocks of an update lie back to back");
  const size_t dc_bytes = dw_group_block_bytes(g->ni_c), da_bytes = dw_group_block_bytes(kDwGroupItems);
  for (oprl_learner* h : g->L) h->noise1_pending = nullptr;
  for (int k0 = 0; k0 < K; k0 += kGroupChunk) {
    const int m = K - k0 < kGroupChunk ? K - k0 : kGroupChunk;
    const int c = g->cur;
    if (g->stage_busy[c]) { HIPC(hipEventSynchronize(g->stage_ev[c])); g->stage_busy[c] = false; }
    take();                                   // nothing of this chunk has been launched until its blocks are complete
    int tiles_c = 0, tiles_a = 0;
    DdpgArgs first[kGroupChunk][2];           // member 0's blocks of each update (for the grids)
    bool due[kGroupChunk];                    // TD3: the actor steps every policy_freq updates — of ALL members at once
    for (int j = 0; j < m; ++j) {
      const int k = k0 + j;
      DdpgArgs* p1 = reinterpret_cast<DdpgArgs*>(g->stage[c] + (size_t)j * g->bytes);
      DdpgArgs* p2 = p1 + n;
      char* dc = reinterpret_cast<char*>(p2 + n);
      char* da = dc + (size_t)n * dc_bytes;
      due[j] = actor_due(g->L[0]);
      for (int l = 0; l < n; ++l) {
        oprl_learner* h = g->L[l];
        if (actor_due(h) != due[j]) { set_err("oprl_group_step_n: the members' delayed actor steps are out of phase (update counts differ modulo policy_freq)"); return roll_back(OPRL_ERR_STATE); }
        const bool prefetch = k + 1 < K && due[j];              // (the row of phase 2's launch: actor steps only)
        StepRows& rows = rows_of[l].plan(h, prefetch ? StepRows::kPhase2 : StepRows::kNone);
        h->epoch += 1;
        if (h->epoch == 0) {      // (the TD-target tag wrapped)
          h->epoch = 1;
          const hipError_t e = hipMemsetAsync(h->y_granules, 0, ((size_t)4 * h->Bmax + 256) * sizeof(unsigned long long), st);
          if (e != hipSuccess) { set_err("oprl_group_step_n: hipMemsetAsync failed: %s", hipGetErrorString(e)); return roll_back(OPRL_ERR_HIP); }
        }
        p1[l] = ddpg_args(h, rows, B);
        p1[l].group_span = g->span;
        int rc = next_tp_tag(&h->tp_tag, h->xbuf, h->xbuf_granules * sizeof(unsigned long long), st, &p1[l].cluster_tag);
        if (rc != OPRL_OK) return roll_back(rc);
        DwKArgs kd;
        // (as the un-merged launches of a solo learner; the step counts move with the blocks, roll_back puts them back)
        DwArgs dw = dw_args(h, true, B, h->opt_step_critic + 1);
        const int tc = fill_dw_kargs(dw, &kd) < 0 ? -1 : compact_dw_kargs(kd, dc + (size_t)l * dc_bytes, g->ni_c);
        dw_commit(h, true, dw, 1);
        int ta = tiles_a;
        if (due[j]) {
          p2[l] = ddpg_args(h, rows, B);
          p2[l].group_span = g->span;
          rc = next_tp_tag(&h->tp_tag, h->xbuf, h->xbuf_granules * sizeof(unsigned long long), st, &p2[l].cluster_tag);   // (a launch, a tag)
          if (rc != OPRL_OK) return roll_back(rc);
          p2[l].prefetch_next = prefetch ? 1 : 0;
          rows.staged = prefetch;
          dw = dw_args(h, false, B, h->opt_step_actor + 1);
          if (alpha_rides(h)) dw.alpha = alpha_job(h, B, h->opt_step_alpha + 1);    // (SAC: the temperature step rides)
          ta = fill_dw_kargs(dw, &kd) < 0 ? -1 : compact_dw_kargs(kd, da + (size_t)l * da_bytes, kDwGroupItems);
          dw_commit(h, false, dw, 1);
          if (l == 0 && tiles_a == 0) tiles_a = ta;
          if (ta < 0 || ta != tiles_a || p2[l].nc != p1[l].nc || p2[l].merged || p2[l].wide || p2[l].whole || p2[l].p2_pair) ta = -1;
        }
        if (l == 0 && j == 0) tiles_c = tc;
        if (tc < 0 || ta < 0 || tc != tiles_c || p1[l].nc != p1[0].nc || p1[l].merged || p1[l].wide || p1[l].whole || p1[l].twin_split) {
          set_err("oprl_group_step_n: internal: bad launch arguments");
          return roll_back(OPRL_ERR_INVALID);
        }
        h->actor_updated_last = due[j];
        h->update_count += 1;
        rows_of[l].done();
      }
      first[j][0] = p1[0];
      if (due[j]) first[j][1] = p2[0];
    }
    HIPC(hipMemcpyAsync(g->dev, g->stage[c], g->bytes * m, hipMemcpyHostToDevice, st));
    HIPC(hipEventRecord(g->stage_ev[c], st));
    g->stage_busy[c] = true;
    g->cur ^= 1;
    for (int j = 0; j < m; ++j) {
      const DdpgArgs* p1 = reinterpret_cast<const DdpgArgs*>(g->dev + (size_t)j * g->bytes);
      const DdpgArgs* p2 = p1 + n;
      const char* dc = reinterpret_cast<const char*>(p2 + n);
      const char* da = dc + (size_t)n * dc_bytes;
      HIPC(launch_ddpg_phase1_group(first[j][0], p1, n, st));
      HIPC(launch_dw_adam_group(dc, g->ni_c, n, tiles_c, st));
      if (!due[j]) continue;
      HIPC(launch_ddpg_phase2_group(first[j][1], p2, n, st));
      HIPC(launch_dw_adam_group(da, kDwGroupItems, n, tiles_a, st));
    }
  }
  return OPRL_OK;
}

