// learner_per.hip — training from prioritized replay ("Training from it"): the entry points
// oprl_learner_update_weighted and oprl_learner_step_n_prio.  Host code only.  The update itself is the generic sequence's: the
// weights travel down in the update's StepRows and its step 3 becomes forward | k_td_weighted_seed | backward
// (learner_modes.hip weighted_critic_step, which also holds per_alloc); everything else of the update is untouched.
#include "learner_internal.h"
#include "replay_internal.h"

namespace {

// may this learner run a weighted update?  Nothing is changed by the test.
int per_check(const oprl_learner* h, const char* who) {
  if (h->cfg.algo == OPRL_TQC) {
    set_err("%s: TQC's quantile-Huber seed takes no per-row weight yet (a follow-up); DDPG, TD3, SAC and REDQ train from prioritized replay", who);
    return OPRL_ERR_INVALID;
  }
  if (h->cfg.algo == OPRL_D4PG) {
    set_err("%s: D4PG's cross-entropy seed takes no per-row weight yet (a follow-up: the per-row cross-entropy as priority)", who);
    return OPRL_ERR_INVALID;
  }
  if (h->bf16 || h->x2) {
    set_err("%s: prioritized training runs the exact-fp32 generic launch sequence only (precision f32)", who);
    return OPRL_ERR_INVALID;
  }
  if (h->cfg.export_grads || h->rccl.comm != nullptr || h->p2p_ok) {
    set_err("%s: gradient-exporting / data-parallel learners do not train from prioritized replay", who);
    return OPRL_ERR_STATE;
  }
  if (h->group_member) { set_err("%s: the learner is a member of a group (packed learners gather their own rows)", who); return OPRL_ERR_STATE; }
  if (h->iql.on) {
    set_err("%s: the learner's implicit-Q-learning mode is on (oprl_learner_set_iql), whose value and actor steps take no importance weights", who);
    return OPRL_ERR_STATE;
  }
  if (h->cql.n > 0) {
    set_err("%s: the learner's conservative-Q-learning mode is on (oprl_learner_set_cql), whose penalty takes no importance weights", who);
    return OPRL_ERR_STATE;
  }
  if (h->ln.on) {
    set_err("%s: the learner's critics carry layer normalisation (oprl_learner_set_layernorm), whose kernels take no importance weights", who);
    return OPRL_ERR_STATE;
  }
  if (h->fused) {
    set_err("%s: the learner's fused launch form is on, which applies no importance weights; create it with no_fuse", who);
    return OPRL_ERR_STATE;
  }
  return OPRL_OK;
}

int weighted_update(oprl_learner* h, const float* s, const float* a, const float* r, const float* d, const float* s2,
                    const float* w, int B, const float* noise0, const float* noise1, float* td_abs, void* stream) {
  StepRows rows = plain_rows(s, a, r, d, s2);
  rows.w = w;
  rows.td_abs = td_abs;
  return learner_update(h, rows, B, noise0, noise1, stream);
}

}  // namespace

extern "C" int oprl_learner_update_weighted(oprl_learner* h, const float* s, const float* a, const float* r, const float* d,
                                            const float* s2, const float* w, int32_t B, const float* noise0,
                                            const float* noise1, float* td_abs_out, void* stream) {
  if (!h) { set_err("oprl_learner_update_weighted: null learner handle"); return OPRL_ERR_INVALID; }
  RC(per_check(h, "oprl_learner_update_weighted"));
  if (!s || !a || !r || !d || !s2 || !w || !td_abs_out) { set_err("oprl_learner_update_weighted: null batch, weight or td_abs pointer"); return OPRL_ERR_INVALID; }
  if (B < 1 || B > h->Bmax) { set_err("oprl_learner_update_weighted: batch %d outside [1, max_batch=%d]", B, h->Bmax); return OPRL_ERR_INVALID; }
  RC(check_device_error(h));
  RC(per_alloc(h));
  return weighted_update(h, s, a, r, d, s2, w, B, noise0, noise1, td_abs_out, stream);
}

extern "C" int oprl_learner_step_n_prio(oprl_learner* h, oprl_replay* replay, int32_t K, int32_t B, uint64_t seed,
                                        double beta0, double beta_steps, void* stream) {
  if (!h || !replay) { set_err("oprl_learner_step_n_prio: null handle"); return OPRL_ERR_INVALID; }
  RC(per_check(h, "oprl_learner_step_n_prio"));
  if (replay->prio == nullptr) {
    set_err("oprl_learner_step_n_prio: the replay has no sum tree (oprl_replay_prio_enable); oprl_learner_step_n samples it uniformly");
    return OPRL_ERR_STATE;
  }
  int nstep = 1;
  RC(RowStager::check("oprl_learner_step_n_prio", h, replay, false, K, B, &nstep));
  if (!(beta0 >= 0.0 && beta0 <= 1.0) || !(beta_steps > 0.0)) {
    set_err("oprl_learner_step_n_prio: need 0 <= beta0 <= 1 and beta_steps > 0 (beta0=%g, beta_steps=%g)", beta0, beta_steps);
    return OPRL_ERR_INVALID;
  }
  RC(check_device_error(h));
  RC(oprl_replay_flush(replay, stream));
  if (replay->n_transitions <= 0 || replay->n_eps <= 0) { set_err("oprl_learner_step_n_prio: replay buffer is empty"); return OPRL_ERR_STATE; }
  RC(per_alloc(h));
  for (int k = 0; k < K; ++k) {
    const uint64_t u = (uint64_t)h->update_count;
    const double beta = std::min(1.0, beta0 + (1.0 - beta0) * (double)u / beta_steps);
    RC(oprl_replay_prio_sample(replay, B, seed, u, beta, h->bs, h->ba, h->br, h->bd, h->bs2, h->per.slots, h->per.w, stream));
    RC(weighted_update(h, h->bs, h->ba, h->br, h->bd, h->bs2, h->per.w, B, nullptr, nullptr, h->per.td, stream));
    RC(oprl_replay_prio_update(replay, B, h->per.slots, h->per.td, stream));
  }
  return OPRL_OK;
}
