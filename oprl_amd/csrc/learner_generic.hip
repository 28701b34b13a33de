// learner_generic.hip — the generic (per-net) launch sequence of an update: the critic phase's steps 1 - 4 and the actor
// phase's steps 5 - 10 with TQC's rider offers and REDQ's subset, and the launch builders they share with the modes'
// steps (learner_modes.hip).  Host code only; learner.hip's critic_phase / actor_phase dispatch here.
#include "learner_internal.h"

namespace oprl_host {

MlpArgs base_args(oprl_learner* h, const oprl_net& n, bool target, int B) {
  MlpArgs a;
  memset(&a, 0, sizeof a);
  if (tp_generic(h, n, B)) {
    a.tp_xbuf = h->xbuf;
    a.tp_tag_counter = &h->tp_tag;
    a.tp_xbuf_bytes = h->xbuf_granules * sizeof(unsigned long long);
  }
  if (h->trace != nullptr && h->trace_slot < OPRL_TRACE_SLOTS)
    a.trace = h->trace + (size_t)(h->trace_slot++) * 64 * kTraceStamps * 2;
  a.net = net_view(eff(h, n), target);
  a.err = h->err_dev;
  if (h->bf16 || h->x2) {     // (the 16-bit packs of the net's layers: bf16, or two fp16 planes per block)
    int idx = -1;                                      // 0 = actor, 1 + j = critic j
    if (&n == &h->cfg.actor) idx = 0;
    for (int j = 0; j < h->nc; ++j) if (&n == &h->cfg.critics[j]) idx = 1 + j;
    const float* pk16 = idx < 0 ? nullptr : (target ? h->pack16_t[idx] : h->pack16[idx]);
    for (int l = 0; pk16 != nullptr && l < n.n_layers; ++l) {
      a.pf16[l] = pk16 + pack16_off_fwd(n, l, h->planes);
      a.pb16[l] = target ? nullptr : pk16 + pack16_off_bwd(n, l, h->planes);
    }
  }
  if (h->ln.on)                      // (a critic of a learner with LN: its view goes with the launch, net_rounds.hip)
    for (int j = 0; j < h->nc; ++j) if (&n == &h->cfg.critics[j]) {
      LnView& v = target ? h->ln.target[j] : h->ln.online[j];
      if (v.drop_thresh != 0) {      // dropout: the key, and the stream T = (u 4 + k) 16 + j of this pass of critic j in this
        v.drop_key = noise_key(h, kDropStream);        // update (a backward-only launch of the same phase draws the same)
        v.drop_stream = ((unsigned long long)h->update_count * 4 + (target ? 0 : h->ln.drop_pass)) * 16 + j;
      }
      a.reserved = &v;
    }
  a.B = B;
  a.action_dim = h->A;
  a.policy_noise = (float)h->cfg.hp.policy_noise;
  a.noise_clip = (float)h->cfg.hp.noise_clip;
  a.max_action = (float)h->cfg.hp.max_action;
  return a;
}

void with_store(MlpArgs& a, const NetWs& ws, bool x, bool dy) {
  for (int l = 0; l < kMaxLayers; ++l) {
    a.Xg[l] = x ? ws.X[l] : nullptr;
    a.dYg[l] = dy ? ws.dY[l] : nullptr;
  }
  a.ldx0 = ws.ldx0;
  a.lddo = ws.lddo;
  a.dY0_stride = ws.dY0_stride;
}

MlpArgs forward_args(oprl_learner* h, const oprl_net& n, const NetWs& ws, bool store_dy, const float* x0, const float* x1, int B,
                     float* out, int ldo) {
  MlpArgs f = base_args(h, n, false, B);
  f.do_fwd = 1;
  f.x0 = x0; f.k0 = h->S; f.x1 = x1; f.k1 = x1 != nullptr ? h->A : 0;
  with_store(f, ws, true, store_dy);
  f.out = out; f.ldo = ldo;
  return f;
}

MlpArgs backward_args(oprl_learner* h, const oprl_net& n, const NetWs& ws, bool store_dy, int B, const float* seed, int ld0) {
  MlpArgs f = base_args(h, n, false, B);
  f.do_bwd = 1;
  with_store(f, ws, true, store_dy);
  f.seed_mode = SEED_PTR;
  f.seed.p0 = seed; f.seed.ld0 = ld0;
  return f;
}

void dact_to(MlpArgs& f, const oprl_learner* h, int j) {
  f.dact_col0 = h->S; f.dact_cols = h->A; f.dact = h->da + (size_t)j * h->Bmax * h->A; f.lddact = h->A;
}

static void seed_rng(MlpArgs& a, const oprl_learner* h, const float* noise, uint64_t stream_id) {
  a.noise = noise;
  a.rng_seed = noise_key(h, stream_id);
  a.rng_ctr = (unsigned long long)h->update_count;
}

// the actor's forward on s with the activations kept for its backward (step 5)
static MlpArgs actor_forward_args(oprl_learner* h, const float* s, int B, const float* noise1) {
  MlpArgs f = forward_args(h, h->cfg.actor, h->ws_actor, false, s, nullptr, B, h->pi, h->A);
  if (gauss_actor(h)) {
    f.out_act = ACT_GAUSS; f.raw_out = h->raw; f.ldraw = 2 * h->A; f.logp = h->logp;
    seed_rng(f, h, noise1, 2);
  } else {
    f.out_act = ACT_TANH;
  }
  return f;
}

// the actor's backward from those activations and the action gradients in da (step 8)
static MlpArgs actor_backward_args(oprl_learner* h, int B, int n_q, const float* noise1) {
  const oprl_learner_config& c = h->cfg;
  MlpArgs f = base_args(h, c.actor, false, B);
  f.do_bwd = 1;
  with_store(f, h->ws_actor, true, true);
  SeedArgs& sd = f.seed;
  if (gauss_actor(h)) {
    f.seed_mode = SEED_GAUSS;
    sd.p0 = h->da; sd.ld0 = h->A; sd.n_da = n_q; sd.da_stride = (long)h->Bmax * h->A;
    sd.p1 = h->raw;
    seed_rng(f, h, noise1, 2);   // backward re-reads (or re-draws) the forward's eps
    sd.log_alpha = alpha_ptr(h); sd.alpha_const = (float)c.hp.alpha_init;
    sd.cval = 1.0f / (float)B;
  } else {
    f.seed_mode = SEED_TANH;
    sd.p0 = h->da; sd.ld0 = h->A; sd.p1 = h->pi;
  }
  return f;
}

// online critic j on (s, a), activations and dY stored for its dW launch: the critic step's forward, with the backward or not
MlpArgs critic_sa_args(oprl_learner* h, int j, const float* s, const float* a, int B, bool bwd) {
  MlpArgs f = base_args(h, h->cfg.critics[j], false, B);
  f.do_fwd = 1; f.do_bwd = bwd ? 1 : 0;
  f.x0 = s; f.k0 = h->S; f.x1 = a; f.k1 = h->A;
  with_store(f, h->ws_critic[j], true, true);
  return f;
}

// SEED_MSE_TD's operands, all but the debug rows y_out / q_out.  n_min: REDQ's target critics (else unused)
SeedArgs mse_td_seed(const oprl_learner* h, const float* r, const float* d, int B, int n_min) {
  const oprl_learner_config& c = h->cfg;
  const bool redq = c.algo == OPRL_REDQ;
  SeedArgs sd;
  memset((void*)&sd, 0, sizeof sd);
  sd.p0 = h->qn;
  sd.p1 = h->nc > 1 ? h->qn + (size_t)h->Bmax * h->ldq : nullptr;
  if (redq) {      // the minimum over the subset's slots: one or two rows here, else k_redq_min's row
    sd.p0 = n_min > 2 ? h->target : h->qn;
    sd.p1 = n_min == 2 ? h->qn + (size_t)h->Bmax * h->ldq : nullptr;
  }
  sd.p2 = (c.algo == OPRL_SAC || redq) ? h->logp2 : nullptr;
  sd.log_alpha = alpha_ptr(h); sd.alpha_const = (float)c.hp.alpha_init;
  sd.r = r; sd.d = d; sd.gamma = (float)c.hp.gamma;
  sd.cval = 1.0f / (float)B;
  return sd;
}

// ------------------------------------------------------------ critic phase
// 1. the next action: the (target) actor on s' — TQC: with the online critics' first hidden launch riding behind it
static int next_action_step(oprl_learner* h, const StepRows& rows, int B, const float* noise0, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  const float *s = rows.cur.s, *a = rows.cur.a;
  const int nc = h->nc, algo = c.algo;
  const bool use_target_actor = (algo == OPRL_DDPG || algo == OPRL_TD3 || algo == OPRL_D4PG);
  MlpArgs f = base_args(h, c.actor, use_target_actor, B);
  f.do_fwd = 1;
  f.x0 = rows.cur.s2; f.k0 = h->S;
  f.out = h->a2; f.ldo = h->A;
  if (algo == OPRL_DDPG || algo == OPRL_D4PG) f.out_act = ACT_TANH;
  else if (algo == OPRL_TD3) { f.out_act = ACT_TANH_SMOOTH; seed_rng(f, h, noise0, 1); }
  else { f.out_act = ACT_GAUSS; f.logp = h->logp2; seed_rng(f, h, noise0, 1); }
  if (h->cql.n > 0) { f.raw_out = h->cql.raw_s2; f.ldraw = 2 * h->A; }      // (the CQL mode samples from this head row too: cql_critic_step)
  // TQC: this launch is 64 workgroups on 256 CUs, and the online critics' first two layers on (s, a) — the
  // first launch of step 3 — depend on nothing of it: they ride behind it (k_slice_tp_fin, layerwise.hip)
  bool fin_ride = false, fin16 = false;
  MlpArgs* fin_args = h->fin_args;
  h->fin_done = false;
  h->fin_l2_done = false;
  h->fin_tail0 = -1;
  if (algo == OPRL_TQC && !h->sw.no_fin_ride && !h->sw.no_layerwise && nc > 2 && nc <= kMaxMulti &&
      h->lw_scratch != nullptr && h->w_critic == 512 && f.tp_xbuf != nullptr) {
    fin16 = h->bf16 || h->x2;
    for (int j = 0; j < nc; ++j) {
      MlpArgs g = critic_sa_args(h, j, s, a, B, true);
      for (int l = 1; l + 1 < g.net.n_layers; ++l) fin16 = fin16 && g.pf16[l] != nullptr && g.pb16[l] != nullptr;
      fin_args[j] = g;
    }
    if (fin16)
      for (int j = 0; j < nc; ++j)
        for (int l = 1; l + 1 < fin_args[j].net.n_layers; ++l) fin_args[j].net.pf[l] = fin_args[j].pf16[l];
    fin_ride = mlp_layerwise_fin_ok(fin_args, nc, h->w_critic);
  }
  // as many nets as fit beside the forward's 4 x slices workgroups with everything resident at once (4 of TQC's 5)
  const int n_ride = fin_ride ? mlp_layerwise_fin_fit(fin_args, nc, 4 * n_slices(B), h->n_cus) : 0;
  if (!fin_ride || n_ride < 1) return launch(f, h->w_actor, st);
  RC(next_tp_tag(f.tp_tag_counter, f.tp_xbuf, f.tp_xbuf_bytes, st, &f.tp_tag));
  RC(profiled(0, st, [&] { return launch_slice_tp_with_fin(f, fin_args, nc, n_ride, h->w_critic, h->n_cus, st, fin16 ? (h->x2 ? 2 : 1) : 0); }));
  h->fin_done = true;
  h->fin16 = fin16;
  if (n_ride < nc) h->fin_tail0 = n_ride;
  return OPRL_OK;
}

// 3. the online critics as every algorithm without a mode runs them: forward + loss seed + backward in one launch per grouping
static int plain_critic_step(oprl_learner* h, const StepRows& rows, int B, int n_min, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  const int nc = h->nc, algo = c.algo;
  // TQC: the actor step's forward on s depends on nothing of the critic step: offered as a rider of this launch's
  // heads (k_lw_head: 80 workgroups on 256 CUs), with the noise and the counter the actor phase would give it
  if (algo == OPRL_TQC && !h->sw.no_af_ride && !c.export_grads && actor_due(h)) {
    MlpArgs f = actor_forward_args(h, rows.cur.s, B, h->noise1_pending);
    if (f.tp_xbuf != nullptr) {
      RC(next_tp_tag(f.tp_tag_counter, f.tp_xbuf, f.tp_xbuf_bytes, st, &f.tp_tag));
      h->rider = f;
      h->rider_pending = true;
    }
  }
  RC(for_each_net(h, nc, h->w_critic, st, [&](int j) {
    MlpArgs f = critic_sa_args(h, j, rows.cur.s, rows.cur.a, B, true);
    f.partials = h->part_c + (size_t)j * n_slices(B) * 4;
    SeedArgs& sd = f.seed;
    if (algo == OPRL_TQC) {
      const int Q = c.hp.n_quantiles, M = nc * Q - c.hp.top_quantiles_to_drop;
      f.seed_mode = SEED_QHUBER;
      sd.p0 = h->target; sd.M = M; sd.Q = Q;
      sd.cval = 1.0f / ((float)B * (float)nc * (float)Q * (float)M);
    } else {
      f.seed_mode = SEED_MSE_TD;
      sd = mse_td_seed(h, rows.cur.r, rows.cur.d, B, n_min);
      if (j == 0) { sd.y_out = h->ydbg; sd.q_out = h->qdbg; }
    }
    return f;
  }));
  h->rider_pending = false;          // (not taken: the actor phase launches the forward itself)
  if (h->fin_done) {                 // the early first launch was not picked up: step 3 did not run layer by layer
    h->fin_done = false;
    set_err("TQC critic step: the online critics' early first launch has no layer-by-layer continuation");
    return OPRL_ERR_STATE;
  }
  return OPRL_OK;
}

int generic_critic_phase(oprl_learner* h, StepRows& rows, int B, const float* noise0, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  const float *r = rows.cur.r, *d = rows.cur.d;
  RC(fresh32_tables(h, 3, st));      // (a PrecX2 learner's generic launches read the fp32 packs)
  h->ln.drop_pass = 1;
  const int nc = h->nc, algo = c.algo;
  if (h->iql.on) return iql_critic_phase(h, rows, B, st);      // the implicit-Q-learning mode: its own sequence
  RC(next_action_step(h, rows, B, noise0, st));
  // 2. target critics on (s', a')   (independent: one stream each)
  if (algo == OPRL_TQC && h->tqc_counter != nullptr && !h->sw.no_tqc_ride) {
    TqcJob& J = h->tqc_job;
    J.counter = h->tqc_counter;
    J.z = h->qn; J.net_stride = (long)h->Bmax * h->ldq; J.ldz = h->ldq;
    J.n_nets = nc; J.Q = c.hp.n_quantiles; J.drop = c.hp.top_quantiles_to_drop;
    J.r = r; J.d = d; J.logp = h->logp2; J.log_alpha = c.log_alpha; J.gamma = (float)c.hp.gamma;
    J.target = h->target;
    h->tqc_job_pending = true;
  }
  // REDQ: only the M target critics of this update's subset run, net redq_subset[j] into slot j of qn
  const bool redq = algo == OPRL_REDQ;
  const int n_min = redq ? c.hp.n_min : 0;
  if (redq) redq_subset(h->noise_seed, h->noise_rank, (uint64_t)h->update_count, nc, n_min, h->redq_subset);
  RC(for_each_net(h, redq ? n_min : nc, h->w_critic, st, [&](int j) {
    MlpArgs f = base_args(h, c.critics[redq ? h->redq_subset[j] : j], true, B);
    f.do_fwd = 1;
    f.x0 = rows.cur.s2; f.k0 = h->S; f.x1 = h->a2; f.k1 = h->A;
    f.out = h->qn + (size_t)j * h->Bmax * h->ldq; f.ldo = h->ldq;
    return f;
  }));
  // (M > 2: their minimum as one row, k_redq_min, into the TQC target's buffer, which REDQ does not use)
  if (redq && n_min > 2) HIPC(launch_redq_min(h->qn, (long)h->Bmax * h->ldq, h->ldq, n_min, B, h->target, st));
  if (h->fin_tail0 >= 0) {                           // (the rest of the early first launch found no head launch to ride on)
    RC(profiled(0, st, [&] { return launch_mlp_layerwise_first(h->fin_args, nc, h->fin_tail0, h->w_critic, h->n_cus, st, h->fin16 ? (h->x2 ? 2 : 1) : 0); }));
    h->fin_tail0 = -1;
  }
  // (the job did not ride — not the layer-by-layer path — or was never offered)
  if (algo == OPRL_TQC && (h->tqc_job_pending || h->tqc_counter == nullptr || h->sw.no_tqc_ride)) {
    h->tqc_job_pending = false;
    HIPC(launch_tqc_target(h->qn, (long)h->Bmax * h->ldq, h->ldq, nc, c.hp.n_quantiles, c.hp.top_quantiles_to_drop, r, d, h->logp2,
                           c.log_alpha, (float)c.hp.gamma, B, h->target, st));
  }
  // 3. online critics (independent: one stream each): the mode's step, or forward + loss seed + backward as one launch
  h->rider_pending = false;
  h->rider_done = false;
  int rows_dw = B;                   // the conservative-Q-learning mode's step 4 runs on the wide rows
  if (h->cql.n > 0) { RC(cql_critic_step(h, rows, B, st)); rows_dw = B * (1 + 3 * h->cql.n); }
  else if (rows.w != nullptr) RC(weighted_critic_step(h, rows, B, n_min, st));
  else if (algo == OPRL_D4PG) RC(c51_critic_step(h, rows, B, st));
  else RC(plain_critic_step(h, rows, B, n_min, st));
  // 4. dW + Adam (+ Polyak where the reference does it every step); the LN parameters' step beside it, at the same step count
  // (in front of dw_step, whose dw_commit moves the count once BOTH launches are out.  Should the dW launch itself fail — a hard
  // error, the update is lost — gamma / beta have taken a step the weights and the count have not)
  if (h->ln.on) RC(ln_adam_step(h, B, st));
  return dw_step(h, true, rows_dw, st);
}

// ------------------------------------------------------------- actor phase
// 6./7. SAC: the critics on (s, pi), both q's before either seed (min), then the gradient wrt the action columns
static int minq_action_grads(oprl_learner* h, const float* s, int B, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  RC(for_each_net(h, h->nc, h->w_critic, st, [&](int j) {
    return forward_args(h, c.critics[j], h->ws_critic[j], false, s, h->pi, B, h->qpi + (size_t)j * h->Bmax, 1);
  }));
  return for_each_net(h, h->nc, h->w_critic, st, [&](int j) {
    MlpArgs f = base_args(h, c.critics[j], false, B);
    f.do_bwd = 1;
    with_store(f, h->ws_critic[j], true, false);
    f.seed_mode = SEED_MINQ;
    f.seed.p0 = h->qpi; f.seed.p1 = h->qpi + h->Bmax; f.seed.which = j;
    f.seed.cval = 1.0f / (float)B;
    dact_to(f, h, j);
    if (j == 0) f.partials = h->part_a;
    return f;
  });
}

// 6./7. every other algorithm without a mode: forward + constant seed + backward in one launch per grouping.  TQC: the
// actor's backward (step 8) and its dW tiles (step 9, *actor_dw) are offered as riders of the launch sequence's end
static int const_action_grads(oprl_learner* h, const float* s, int B, int n_q, const float* noise1, DwArgs* actor_dw, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  const int nc = h->nc, algo = c.algo;
  // TQC: the actor's backward (step 8) consumes the action gradients the launch sequence below ends with (k_lw_dact):
  // offered as a rider of that launch (r06-16; the tag its launch would draw, now)
  h->bwd_rider_pending = false;
  h->bwd_rider_done = false;
  if (algo == OPRL_TQC && gauss_actor(h) && !c.export_grads && !h->sw.no_bwd_ride) {
    MlpArgs f = actor_backward_args(h, B, n_q, noise1);
    if (f.tp_xbuf != nullptr && mlp_slice_tp_shape_ok(f, h->w_actor)) {
      RC(next_tp_tag(f.tp_tag_counter, f.tp_xbuf, f.tp_xbuf_bytes, st, &f.tp_tag));
      h->bwd_rider = f;
      h->bwd_rider_pending = true;
      // ... and step 9's tiles behind it (the 16 x 32 tiles of k_dw_adam, the temperature's step as the workgroup one past
      // them): built with THIS update's step counts, committed once they have ridden; if the launch does not take them,
      // step 9 launches the same table
      h->bwd_tiles_pending = false;
      h->bwd_tiles_done = false;
      if (!h->sw.no_bwd_tiles && alpha_rides(h) && h->n_items_actor <= kDwMaxItems) {
        *actor_dw = dw_args(h, false, B, h->opt_step_actor + 1);
        actor_dw->alpha = alpha_job(h, B, h->opt_step_alpha + 1);
        const int total = fill_dw_kargs(*actor_dw, &h->bwd_tiles, 32);
        if (total > 0) {
          h->bwd_tile_wgs = total + (actor_dw->alpha.log_alpha != nullptr ? 1 : 0);
          h->bwd_tiles_pending = true;
        }
      }
    }
  }
  return for_each_net(h, n_q, h->w_critic, st, [&](int j) {
    MlpArgs f = base_args(h, c.critics[j], false, B);
    f.do_fwd = 1; f.do_bwd = 1;
    f.x0 = s; f.k0 = h->S; f.x1 = h->pi; f.k1 = h->A;
    f.seed_mode = SEED_CONST;
    f.seed.cval = (algo == OPRL_TQC) ? -1.0f / ((float)B * (float)nc * (float)c.hp.n_quantiles)
                  : (algo == OPRL_REDQ) ? -1.0f / ((float)B * (float)nc)      // the mean over the ensemble
                                        : -1.0f / (float)B;
    dact_to(f, h, j);
    if (j == 0) f.partials = h->part_a;
    if (algo == OPRL_REDQ) f.partials = h->part_a + (size_t)j * n_slices(B) * 4;   // (read_scalars: mean over all N)
    return f;
  });
}

int generic_actor_phase(oprl_learner* h, StepRows& rows, int B, const float* noise1, hipStream_t st) {
  const float* s = rows.cur.s;
  RC(fresh32_tables(h, 3, st));
  h->ln.drop_pass = 2;
  const int algo = h->cfg.algo;
  const int n_q = (algo == OPRL_TD3 || algo == OPRL_DDPG || algo == OPRL_D4PG) ? 1 : h->nc;   // TD3 uses Q1 only
  // (the offers to the riding launches below never outlive this update: after an error return the next must not find one)
  struct ClearOffers {
    oprl_learner* h;
    ~ClearOffers() { h->bwd_rider_pending = false; h->bwd_rider_done = false; h->bwd_tiles_pending = false; h->bwd_tiles_done = false; }
  } clear_offers{h};
  DwArgs actor_dw;                        // step 9's table where it rides (built with this update's step counts)
  // 5. actor forward (activations kept for its backward) — unless it rode on the critic step's heads (the critic phase)
  if (h->rider_done) h->rider_done = false;
  else RC(launch(actor_forward_args(h, s, B, noise1), h->w_actor, st));
  // 6./7. the gradient wrt the action columns into da: the mode's step, or the critics on (s, pi)
  if (algo == OPRL_SAC) RC(minq_action_grads(h, s, B, st));
  else if (algo == OPRL_D4PG) RC(c51_action_grads(h, rows, B, st));
  else if (h->iql.on) RC(iql_action_grads(h, rows, B, st));
  else if (h->bc.alpha > 0.0) RC(bc_action_grads(h, rows, B, st));
  else RC(const_action_grads(h, s, B, n_q, noise1, &actor_dw, st));
  // 8. actor backward from the stored activations — unless it rode on the k_lw_dact launch above
  h->bwd_rider_pending = false;
  if (h->bwd_rider_done) h->bwd_rider_done = false;
  else RC(launch(actor_backward_args(h, B, n_q, noise1), h->w_actor, st));
  // 9. dW + Adam (+ Polyak of the actor target for DDPG / TD3) — unless the tiles rode behind the riding backward
  h->bwd_tiles_pending = false;
  if (h->bwd_tiles_done) dw_commit(h, false, actor_dw, 1);
  else RC(dw_step(h, false, B, st));
  // 10. temperature (when it did not ride on the actor's dW launch)
  return temperature_step(h, B, st);
}

}  // namespace oprl_host
