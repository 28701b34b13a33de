// learner_misc.hip — scalars, counters, traces and debug views of a learner, and the stand-alone building blocks of
// the C-ABI (oprl_mlp_forward / act / backward, oprl_adam_step, oprl_polyak).  Split from learner.hip (round 4).
#include "learner_internal.h"
#include "c51_seed.h"
#include "bc_seed.h"
#include "iql_seed.h"
#include "cql_seed.h"

#include <cmath>
#include <vector>

extern "C" int oprl_learner_read_scalars(oprl_learner* h, float* out_host, int32_t n, void* stream) {
  if (!h || !out_host || n < 1) { set_err("oprl_learner_read_scalars: invalid argument"); return OPRL_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  const int B = h->last_B > 0 ? h->last_B : 1;
  const int n_slices = (B + kR - 1) / kR;
  const oprl_learner_config& c = h->cfg;
  float loss_scale = 1.0f / (float)B;
  if (c.algo == OPRL_TQC) {
    const int Q = c.hp.n_quantiles, M = h->nc * Q - c.hp.top_quantiles_to_drop;
    loss_scale = 1.0f / ((float)B * (float)h->nc * (float)Q * (float)M);
  }
  // critic partials of all critics are contiguous: loss sums over critics (td1 + td2)
  HIPC(launch_reduce_partials(h->part_c, n_slices * h->nc, h->scalars, 0, loss_scale,
                              1.0f / ((float)B * (float)h->nc), st));
  // (REDQ: the actor-step sums of every critic, -mean over the ensemble)
  const int n_qa = c.algo == OPRL_REDQ ? h->nc : 1;
  // (the implicit-Q-learning mode: k_iql_actor_seed's sums of w (pi - a)^2, the loss itself and not -q)
  HIPC(launch_reduce_partials(h->part_a, n_slices * n_qa, h->scalars, 4, 0.f, (h->iql_on ? 1.0f : -1.0f) / ((float)B * (float)n_qa), st));
  // critic 0 alone (the reference logs q1, not the twin mean) and the mean log-density of the actor step
  HIPC(launch_reduce_partials(h->part_c, n_slices, h->scalars, 8, loss_scale, 1.0f / (float)B, st));
  const bool gauss = gauss_actor(h);
  if (gauss) HIPC(launch_sum(h->logp, B, h->scalars, 12, 1.0f / (float)B, st));
  float host[16] = {0};
  HIPC(hipMemcpyAsync(host, h->scalars, sizeof(float) * 13, hipMemcpyDeviceToHost, st));
  double la = 0.0;
  const double* lap = alpha_ptr(h);
  if (lap) HIPC(hipMemcpyAsync(&la, lap, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  RC(check_device_error(h));      // after the synchronisation: definitive for everything launched so far
  float res[6];
  res[0] = host[0];                 // critic loss
  res[1] = host[5];                 // actor loss (-mean q part)
  res[2] = host[1];                 // mean q
  res[3] = host[2];                 // mean TD target
  res[4] = lap ? (float)exp(la) : (float)c.hp.alpha_init;
  res[5] = (float)h->update_count;
  float res2[4];
  res2[0] = host[9];                                  // mean q of critic 0 (the reference's "q1")
  res2[1] = gauss ? host[12] : 0.f;                   // mean log pi(a|s) of the last actor step
  // SAC / TQC actor loss as the reference forms it: alpha * mean(log pi) - mean(min q)   (sac.py:124-126)
  res2[2] = gauss ? res[4] * res2[1] + res[1] : res[1];
  // temperature loss -log_alpha * (target_entropy + mean log pi)   (sac.py:133-135; with the CURRENT log_alpha)
  res2[3] = lap ? (float)(-la * (c.hp.target_entropy + (double)res2[1])) : 0.f;
  for (int i = 0; i < n && i < 6; ++i) out_host[i] = res[i];
  for (int i = 6; i < n && i < 10; ++i) out_host[i] = res2[i - 6];
  return OPRL_OK;
}

extern "C" int oprl_learner_set_trace(oprl_learner* h, int64_t* buf) {
  if (!h) { set_err("null learner handle"); return OPRL_ERR_INVALID; }
  h->trace = (long long*)buf;
  return OPRL_OK;
}

extern "C" int oprl_learner_update_count(oprl_learner* h, int64_t* out_host) {
  if (!h || !out_host) { set_err("null argument"); return OPRL_ERR_INVALID; }
  *out_host = h->update_count;
  return OPRL_OK;
}

extern "C" int oprl_learner_set_update_count(oprl_learner* h, int64_t count) {
  if (!h || count < 0) { set_err("invalid argument"); return OPRL_ERR_INVALID; }
  h->update_count = count;
  return OPRL_OK;
}

extern "C" int oprl_learner_set_seed(oprl_learner* h, uint64_t seed, int32_t rank) {
  if (!h || rank < 0) { set_err("oprl_learner_set_seed: invalid argument"); return OPRL_ERR_INVALID; }
  h->noise_seed = seed;
  h->noise_rank = rank;
  return OPRL_OK;
}

extern "C" int oprl_learner_get_counters(oprl_learner* h, int64_t out_host[OPRL_N_COUNTERS]) {
  if (!h || !out_host) { set_err("null argument"); return OPRL_ERR_INVALID; }
  out_host[0] = h->update_count;
  out_host[1] = h->opt_step_critic;
  out_host[2] = h->opt_step_actor;
  out_host[3] = h->opt_step_alpha;
  return OPRL_OK;
}

extern "C" int oprl_learner_set_counters(oprl_learner* h, const int64_t in_host[OPRL_N_COUNTERS]) {
  if (!h || !in_host) { set_err("null argument"); return OPRL_ERR_INVALID; }
  for (int k = 0; k < OPRL_N_COUNTERS; ++k)
    if (in_host[k] < 0 || in_host[k] > 0x7fffffffLL) { set_err("counter %d out of range", k); return OPRL_ERR_INVALID; }
  h->update_count = in_host[0];
  h->opt_step_critic = (int)in_host[1];
  h->opt_step_actor = (int)in_host[2];
  h->opt_step_alpha = (int)in_host[3];
  return OPRL_OK;
}

extern "C" int oprl_learner_debug_ptrs(oprl_learner* h, const float** q, const float** y) {
  if (!h) { set_err("null learner handle"); return OPRL_ERR_INVALID; }
  if (q) *q = h->qdbg;
  if (y) *y = h->ydbg;
  return OPRL_OK;
}

// (debug) device views of the workspace a fused DDPG update leaves behind: tools/race_hunt.py compares them between a
// chain learner and a one-update-per-launch learner.  which: 0..2 the actor's X rows, 3 pi, 4 unit-seed rows, 5 du granules
// (8 bytes each), 6..8 the critic's X rows, 9 / 10 the critic's dY rows (first hidden partials | second hidden), 11 the TD
// seed granules, 12 the batch rows of the last update's set (s), 13 the other set
extern "C" int oprl_learner_debug_view(oprl_learner* h, int32_t which, const void** ptr, int64_t* n_bytes) {
  if (!h || !ptr || !n_bytes) { set_err("oprl_learner_debug_view: invalid argument"); return OPRL_ERR_INVALID; }
  const size_t B = (size_t)h->Bmax;
  const void* p = nullptr;
  size_t n = 0;
  switch (which) {
    case 0: p = h->ws_actor.X[0]; n = B * h->ws_actor.ldx0 * 4; break;
    case 1: p = h->ws_actor.X[1]; n = B * h->ws_actor.width * 4; break;
    case 2: p = h->ws_actor.X[2]; n = B * h->ws_actor.width * 4; break;
    case 3: p = h->pi; n = B * h->A * 4; break;
    case 4: p = h->gu; n = h->gu ? (size_t)h->A * (B < 256 ? B : 256) * 256 * 4 : 0; break;
    case 5: p = h->du_granules; n = h->du_granules ? (B < 256 ? B : 256) * kDuLd * 8 : 0; break;
    case 6: p = h->ws_critic[0].X[0]; n = B * h->ws_critic[0].ldx0 * 4; break;
    case 7: p = h->ws_critic[0].X[1]; n = B * h->ws_critic[0].width * 4; break;
    case 8: p = h->ws_critic[0].X[2]; n = B * h->ws_critic[0].width * 4; break;
    case 9: p = h->ws_critic[0].dY[0]; n = B * h->ws_critic[0].width * 4; break;
    case 10: p = h->ws_critic[0].dY[1]; n = B * h->ws_critic[0].width * 4; break;
    case 11: p = h->y_granules; n = B * 8; break;
    case 12: p = h->bs; n = B * h->S * 4; break;
    case 13: p = h->batch_alt; n = h->batch_alt ? B * h->S * 4 : 0; break;
    default: set_err("oprl_learner_debug_view: no such view"); return OPRL_ERR_INVALID;
  }
  *ptr = p; *n_bytes = (int64_t)n;
  return OPRL_OK;
}

// Which LAUNCH FORM would an update of batch size B take right now?  The decision (learner.hip fused_form: a dozen
// interacting conditions — precision, algorithm, batch size, cluster size, gradient export, the data-parallel exchange, a
// shared chip, the environment switches) as numbers a test can hold against a table (tests/test_gpu_forms.py), so that a
// mode falling off its fast form is a red test and not a line in a benchmark.  Reads the learner only.
//   out[0]  fused: 1 the fused phase kernels (DDPG / TD3 / SAC), 0 the generic launch sequence (TQC, no_fuse, odd shapes)
//   out[1]  lean: 1 tp4.h's passes, 0 the generic tp3.h passes
//   out[2]  form: 4 whole updates per launch (k_ddpg_chain), 3 both merged launches (phase 1 + critic tiles | phase 2 +
//           actor tiles), 2 merged phase 1 only, 1 the plain phase launches + dW launches, 0 not fused
//   out[3]  updates per chain launch step_n may run (1 unless form 4)
//   out[4]  wide bits (1: role A on clusters of eight, 2: the critic pass)      out[5]  cluster size of the other roles
//   out[6]  twin_split    out[7]  p2_pair    out[8]  arithmetic of the kernels: 0 exact fp32, 1 bf16, 2 x2
//   out[9]  XCD-local cluster exchanges    out[10] the learner was demoted to the shared-chip forms
//   out[11] gradient-exporting learners: the form (as out[2]) of a data-parallel update whose exchange runs inside the dW
//           tiles (peer windows, level 2) — 4 = the rank runs the single-GPU whole-update launch; others: 0
//   out[12] rt2: 1 phase 1's B roles carry two row tiles per cluster, 2 ... and SAC's role A carries role C's pass, 0 neither
extern "C" int oprl_learner_debug_form(oprl_learner* h, int32_t B, int32_t* out) {
  if (!h || !out || B < 1 || B > h->Bmax) { set_err("oprl_learner_debug_form: invalid argument"); return OPRL_ERR_INVALID; }
  auto form_code = [](const FusedForm& f) { return f.whole ? 4 : ((f.merged & 3) == 3 ? 3 : ((f.merged & 1) ? 2 : 1)); };
  for (int i = 0; i < 13; ++i) out[i] = 0;
  out[10] = h->shared_chip ? 1 : 0;
  out[8] = h->x2 ? 2 : (h->bf16 ? 1 : 0);
  if (!use_fused(h, B)) return OPRL_OK;
  const FusedForm f = fused_form(h, B, h->dp_inline);
  out[0] = 1;
  out[1] = f.lean ? 1 : 0;
  out[2] = form_code(f);
  out[3] = f.chain_max;
  out[4] = f.wide; out[5] = f.nc; out[6] = f.twin_split; out[7] = f.p2_pair;
  out[8] = f.x2 ? 2 : (f.bf16 ? 1 : 0);
  out[9] = h->xcd_local ? 1 : 0;
  if (h->cfg.export_grads) out[11] = form_code(fused_form(h, B, true));
  out[12] = f.rt2;
  return OPRL_OK;
}

// D4PG's critic seed on the caller's rows (include/oprl_amd.h): the kernel and the launch checks of the learner's critic step
extern "C" int oprl_c51_seed(const float* zt, const float* z, const float* r, const float* d, double gamma, double v_min,
                             double v_max, int32_t N, int32_t B, int32_t ld, float* seed_out, float* m_out, float* loss_out,
                             void* stream) {
  if (!zt || !z || !r || !d || !seed_out) { set_err("oprl_c51_seed: null argument"); return OPRL_ERR_INVALID; }
  if (N < 2 || N > kC51MaxAtoms || ld < N || ld > 64 || B < 1 || !((float)v_max > (float)v_min)) {
    set_err("oprl_c51_seed: need 2 <= N <= %d atoms (N=%d), N <= ld <= 64 (ld=%d), B >= 1 (B=%d) and v_max > v_min (%g, %g)",
            kC51MaxAtoms, N, ld, B, v_max, v_min);
    return OPRL_ERR_INVALID;
  }
  C51Args a;
  memset((void*)&a, 0, sizeof a);
  a.z = z; a.zt = zt; a.r = r; a.d = d;
  a.gamma = (float)gamma; a.v_min = (float)v_min; a.v_max = (float)v_max;
  a.inv_B = 1.0f / (float)B;
  a.N = N; a.B = B; a.ld = ld;
  a.seed = seed_out; a.m = m_out; a.loss_row = loss_out;
  HIPC(launch_c51_critic_seed(a, (hipStream_t)stream));
  return OPRL_OK;
}

// ---------------------------------------------------------------- TD3 + BC
// The behaviour-cloning mode of a TD3 learner's actor step (learner.hip actor_phase).  Every refusal comes before any GPU
// work and changes nothing.
extern "C" int oprl_learner_set_bc(oprl_learner* h, double alpha) {
  if (!h) { set_err("oprl_learner_set_bc: null learner handle"); return OPRL_ERR_INVALID; }
  if (h->cfg.algo != OPRL_TD3) {
    set_err("oprl_learner_set_bc: the behaviour-cloning actor step is a mode of TD3 learners (algo %d); DDPG shares the branch and is a follow-up", h->cfg.algo);
    return OPRL_ERR_INVALID;
  }
  if (h->bf16 || h->x2) { set_err("oprl_learner_set_bc: the BC step runs the exact-fp32 generic launch sequence only (precision f32)"); return OPRL_ERR_INVALID; }
  // (as the kernel sees it, a float: neither overflowing nor flushed to zero)
  if (!std::isfinite(alpha) || alpha < 0.0 || !std::isfinite((float)alpha) || (alpha > 0.0 && !((float)alpha > 0.f))) {
    set_err("oprl_learner_set_bc: alpha=%g is not a finite number >= 0 (0 turns the mode off)", alpha);
    return OPRL_ERR_INVALID;
  }
  // (a member of a group is a fused learner: said first, so that the message names the reason that cannot be lifted)
  if (h->group_member) { set_err("oprl_learner_set_bc: the learner is a member of a group (packed learners run the fused launches, which have no BC step)"); return OPRL_ERR_STATE; }
  if (h->fused) {
    set_err("oprl_learner_set_bc: the learner's fused launch form is on, which has no BC step; create it with no_fuse");
    return OPRL_ERR_STATE;
  }
  if (h->cfg.export_grads || h->rccl.comm != nullptr || h->p2p_ok) {
    set_err("oprl_learner_set_bc: gradient-exporting (export_grads) / data-parallel learners have no BC step");
    return OPRL_ERR_STATE;
  }
  if (h->iql_on) { set_err("oprl_learner_set_bc: the learner's implicit-Q-learning mode is on (oprl_learner_set_iql), whose actor step runs no critic"); return OPRL_ERR_STATE; }
  if (alpha > 0.0 && h->bc_seed == nullptr) {      // the mode's rows, once: no update allocates
    const size_t n = (size_t)h->Bmax + 4 + (size_t)bc_mix_slices(h->Bmax, h->A);
    float* p = nullptr;
    if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) { set_err("hipMalloc(%zu) failed (behaviour-cloning rows)", n * sizeof(float)); return OPRL_ERR_NOMEM; }
    hipError_t e = hipMemset(p, 0, n * sizeof(float));
    if (e != hipSuccess) { (void)hipFree(p); HIPC(e); }
    h->bc_seed = p;
    h->bc_scal = p + h->Bmax;
    h->bc_part = h->bc_scal + 4;
  }
  h->bc_alpha = alpha;
  return OPRL_OK;
}

extern "C" int oprl_learner_read_bc(oprl_learner* h, float out_host[4], void* stream) {
  if (!h || !out_host) { set_err("oprl_learner_read_bc: null argument"); return OPRL_ERR_INVALID; }
  if (h->bc_seed == nullptr) { set_err("oprl_learner_read_bc: the behaviour-cloning mode was never on (oprl_learner_set_bc)"); return OPRL_ERR_STATE; }
  hipStream_t st = (hipStream_t)stream;
  const int n = h->bc_parts;
  std::vector<float> host(4 + (size_t)n, 0.f);
  HIPC(hipMemcpyAsync(host.data(), h->bc_scal, sizeof(float) * (4 + (size_t)n), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  RC(check_device_error(h));
  double sq = 0.0;                                  // k_bc_mix's partial sums, in slice order
  for (int i = 0; i < n; ++i) sq += (double)host[4 + i];
  out_host[0] = host[0];                            // lambda
  out_host[1] = host[1];                            // mean |Q1(s, pi(s))|
  out_host[2] = n > 0 ? (float)(sq / ((double)h->bc_B * (double)h->A)) : 0.f;   // mean (pi - a)^2
  out_host[3] = 0.f;
  return OPRL_OK;
}

extern "C" int oprl_bc_seed(const float* q, const float* pi, const float* a, float* da, double alpha, int32_t B, int32_t A,
                            float* seed_out, float* scal_out, float* part_q_out, float* part_sq_out, void* stream) {
  if (!q || !pi || !a || !da || !seed_out || !scal_out || !part_q_out || !part_sq_out) { set_err("oprl_bc_seed: null argument"); return OPRL_ERR_INVALID; }
  if (B < 1 || A < 1 || (int64_t)B * A > (1 << 30) || !std::isfinite(alpha) || !((float)alpha > 0.f) || !std::isfinite((float)alpha)) {
    set_err("oprl_bc_seed: need B >= 1 (B=%d), A >= 1 (A=%d), B A <= 2^30 and a finite alpha > 0 (%g)", B, A, alpha);
    return OPRL_ERR_INVALID;
  }
  BcSeedArgs t;
  memset((void*)&t, 0, sizeof t);
  t.q = q; t.alpha = (float)alpha; t.B = B; t.n_slices = (B + kR - 1) / kR;
  t.seed = seed_out; t.scal = scal_out; t.partials = part_q_out;
  HIPC(launch_bc_seed(t, (hipStream_t)stream));
  BcMixArgs m;
  memset((void*)&m, 0, sizeof m);
  m.pi = pi; m.a = a; m.da = da; m.part = part_sq_out; m.B = B; m.A = A;
  HIPC(launch_bc_mix(m, (hipStream_t)stream));
  return OPRL_OK;
}

// ---------------------------------------------------------------- implicit Q-learning
// The IQL mode of a TD3 learner (learner.hip iql_critic_phase / actor_phase).  Every refusal comes before any GPU work and
// changes nothing.
namespace {
// (as the kernels see them, floats: neither overflowing nor flushed to zero)
bool iql_hparams_ok(const char* who, double expectile, double beta, double adv_clip) {
  if (!std::isfinite(expectile) || !(expectile > 0.0 && expectile < 1.0) || !((float)expectile > 0.f) || !((float)(1.0 - expectile) > 0.f)) {
    set_err("%s: expectile=%g is not a number inside (0, 1)", who, expectile);
    return false;
  }
  if (!std::isfinite(beta) || beta < 0.0 || !std::isfinite((float)beta)) { set_err("%s: beta=%g is not a finite number >= 0", who, beta); return false; }
  if (!std::isfinite(adv_clip) || !((float)adv_clip > 0.f) || !std::isfinite((float)adv_clip)) {
    set_err("%s: adv_clip=%g is not a finite number > 0", who, adv_clip);
    return false;
  }
  return true;
}
}  // namespace

extern "C" int oprl_learner_set_iql(oprl_learner* h, const oprl_net* value, double expectile, double beta, double adv_clip,
                                    double lr_value) {
  if (!h) { set_err("oprl_learner_set_iql: null learner handle"); return OPRL_ERR_INVALID; }
  if (value == nullptr) {          // off: plain TD3 again (the rows stay for the next turn-on; V's step count is kept)
    h->iql_on = false;
    return OPRL_OK;
  }
  if (h->cfg.algo != OPRL_TD3) {
    set_err("oprl_learner_set_iql: implicit Q-learning is a mode of TD3 learners (algo %d): twin critics and a tanh actor", h->cfg.algo);
    return OPRL_ERR_INVALID;
  }
  if (h->bf16 || h->x2) { set_err("oprl_learner_set_iql: the mode runs the exact-fp32 generic launch sequence only (precision f32)"); return OPRL_ERR_INVALID; }
  if (h->cfg.hp.policy_freq != 1) {
    set_err("oprl_learner_set_iql: policy_freq=%d; implicit Q-learning takes its actor step and the critics' Polyak step on every update (policy_freq 1)", h->cfg.hp.policy_freq);
    return OPRL_ERR_INVALID;
  }
  if (!iql_hparams_ok("oprl_learner_set_iql", expectile, beta, adv_clip)) return OPRL_ERR_INVALID;
  if (!std::isfinite(lr_value) || !(lr_value > 0.0) || !((float)lr_value > 0.f) || !std::isfinite((float)lr_value)) {
    set_err("oprl_learner_set_iql: lr_value=%g is not a finite number > 0", lr_value);
    return OPRL_ERR_INVALID;
  }
  int wv = 0;
  RC(check_net(*value, "oprl_learner_set_iql: value net", &wv));      // (layer count, widths, theta, pack: what the generic path takes)
  if (value->dims[0] != h->S || value->dims[value->n_layers] != 1) {
    set_err("oprl_learner_set_iql: the value net maps %d inputs to %d outputs; V(s) takes the learner's state_dim=%d and has one output",
            value->dims[0], value->dims[value->n_layers], h->S);
    return OPRL_ERR_INVALID;
  }
  if (!value->adam_m || !value->adam_v) { set_err("oprl_learner_set_iql: the value net has no Adam moments (adam_m / adam_v)"); return OPRL_ERR_INVALID; }
  if (value->theta_target != nullptr || value->grad != nullptr) {
    set_err("oprl_learner_set_iql: the value net has a target or a gradient arena; V has no target net and the mode exports no gradients");
    return OPRL_ERR_INVALID;
  }
  // (a member of a group is a fused learner: said first, so that the message names the reason that cannot be lifted)
  if (h->group_member) { set_err("oprl_learner_set_iql: the learner is a member of a group (packed learners run the fused launches, which have no value net)"); return OPRL_ERR_STATE; }
  if (h->fused) {
    set_err("oprl_learner_set_iql: the learner's fused launch form is on, which has no value net; create it with no_fuse");
    return OPRL_ERR_STATE;
  }
  if (h->cfg.export_grads || h->rccl.comm != nullptr || h->p2p_ok) {
    set_err("oprl_learner_set_iql: gradient-exporting (export_grads) / data-parallel learners have no implicit-Q-learning step");
    return OPRL_ERR_STATE;
  }
  if (h->bc_alpha > 0.0) { set_err("oprl_learner_set_iql: the learner's behaviour-cloning mode is on (oprl_learner_set_bc); turn it off first"); return OPRL_ERR_STATE; }
  // the mode's rows, once per shape of V: no update allocates
  bool same = h->iql_base != nullptr && h->iql_value.n_layers == value->n_layers;
  for (int l = 0; same && l <= value->n_layers; ++l) same = h->iql_value.dims[l] == value->dims[l];
  if (!same) {
    const size_t Bm = (size_t)h->Bmax, slices = (Bm + kR - 1) / kR;
    // (Pool::take rounds every block up to 256 bytes: 64 floats of slack for each of the 7 blocks behind the workspace)
    const size_t n = net_ws_floats(*value, h->Bmax) + 5 * Bm + 2 * slices * 4 + 8 * 64;
    float* p = nullptr;
    if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) { set_err("hipMalloc(%zu) failed (implicit-Q-learning rows)", n * sizeof(float)); return OPRL_ERR_NOMEM; }
    hipError_t e = hipMemset(p, 0, n * sizeof(float));
    if (e != hipSuccess) { (void)hipFree(p); HIPC(e); }
    if (h->iql_base != nullptr) (void)hipFree(h->iql_base);
    h->iql_base = p;
    Pool pool;
    pool.base = reinterpret_cast<char*>(p); pool.cap = n * sizeof(float);
    h->ws_value = NetWs{};
    alloc_net_ws(pool, *value, h->Bmax, &h->ws_value);
    h->iql_vn = pool.take<float>(Bm);
    h->iql_vs = pool.take<float>(Bm);
    h->iql_u = pool.take<float>(Bm);
    h->iql_w = pool.take<float>(Bm);
    h->iql_seed = pool.take<float>(Bm);
    h->iql_part_v = pool.take<float>(slices * 4);
    h->iql_part_w = pool.take<float>(slices * 4);
    if (pool.used > pool.cap) { set_err("internal: the implicit-Q-learning rows overran their allocation"); h->iql_on = false; return OPRL_ERR_STATE; }
    h->iql_B = 0;
  }
  h->iql_value = *value;
  h->iql_items.clear();
  h->iql_tiles = 0;
  fill_items(h->iql_value, h->ws_value, h->iql_items, &h->iql_tiles);
  h->iql_tau = expectile; h->iql_beta = beta; h->iql_clip = adv_clip; h->iql_lr = lr_value;
  h->iql_on = true;
  return OPRL_OK;
}

extern "C" int oprl_learner_read_iql(oprl_learner* h, float out_host[8], void* stream) {
  if (!h || !out_host) { set_err("oprl_learner_read_iql: null argument"); return OPRL_ERR_INVALID; }
  if (h->iql_base == nullptr) { set_err("oprl_learner_read_iql: the implicit-Q-learning mode was never on (oprl_learner_set_iql)"); return OPRL_ERR_STATE; }
  hipStream_t st = (hipStream_t)stream;
  const int B = h->iql_B, n = B > 0 ? (B + kR - 1) / kR : 0;
  std::vector<float> pv((size_t)n * 4, 0.f), pw((size_t)n * 4, 0.f), pa((size_t)n * 4, 0.f);
  if (n > 0) {
    HIPC(hipMemcpyAsync(pv.data(), h->iql_part_v, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(pw.data(), h->iql_part_w, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(pa.data(), h->part_a, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, st));
  }
  HIPC(hipStreamSynchronize(st));
  RC(check_device_error(h));
  double s[6] = {0, 0, 0, 0, 0, 0};                 // the per-slice sums, in slice order
  for (int i = 0; i < n; ++i) {
    s[0] += (double)pv[4 * i]; s[1] += (double)pv[4 * i + 1]; s[2] += (double)pv[4 * i + 2];
    s[3] += (double)pw[4 * i + 1]; s[4] += (double)pw[4 * i + 2];
    s[5] += (double)pa[4 * i + 1];
  }
  // V loss | mean V(s) | mean u | mean w | share of rows at the clip | the weighted cloning loss | two spares
  for (int k = 0; k < 6; ++k) out_host[k] = n > 0 ? (float)(s[k] / (double)B) : 0.f;
  out_host[6] = out_host[7] = 0.f;
  return OPRL_OK;
}

// V's Adam step count (get_counters / set_counters carry four numbers and stay as they are)
extern "C" int oprl_learner_get_iql_step(oprl_learner* h, int64_t* out_host) {
  if (!h || !out_host) { set_err("oprl_learner_get_iql_step: null argument"); return OPRL_ERR_INVALID; }
  *out_host = h->opt_step_value;
  return OPRL_OK;
}

extern "C" int oprl_learner_set_iql_step(oprl_learner* h, int64_t step) {
  if (!h) { set_err("oprl_learner_set_iql_step: null learner handle"); return OPRL_ERR_INVALID; }
  if (step < 0 || step > 0x7fffffffLL) { set_err("oprl_learner_set_iql_step: step %lld out of range", (long long)step); return OPRL_ERR_INVALID; }
  h->opt_step_value = (int)step;
  return OPRL_OK;
}

extern "C" int oprl_iql_seed(const float* q1, const float* q2, const float* v, const float* pi, const float* a, double expectile,
                             double beta, double adv_clip, int32_t B, int32_t A, float* u_out, float* seed_out, float* w_out,
                             float* da_out, float* part_v_out, float* part_w_out, float* part_a_out, void* stream) {
  if (!q1 || !q2 || !v || !pi || !a || !u_out || !seed_out || !w_out || !da_out || !part_v_out || !part_w_out || !part_a_out) {
    set_err("oprl_iql_seed: null argument");
    return OPRL_ERR_INVALID;
  }
  if (B < 1 || A < 1 || (int64_t)B * A > (1 << 30)) {
    set_err("oprl_iql_seed: need B >= 1 (B=%d), A >= 1 (A=%d) and B A <= 2^30", B, A);
    return OPRL_ERR_INVALID;
  }
  if (!iql_hparams_ok("oprl_iql_seed", expectile, beta, adv_clip)) return OPRL_ERR_INVALID;
  IqlValueArgs t;
  memset((void*)&t, 0, sizeof t);
  t.q1 = q1; t.q2 = q2; t.v = v;
  t.tau = (float)expectile; t.omtau = (float)(1.0 - expectile);
  t.beta = (float)beta; t.clip = (float)adv_clip;
  t.inv_B = 1.0f / (float)B;
  t.B = B; t.n_slices = (B + kR - 1) / kR;
  t.u = u_out; t.seed = seed_out; t.w = w_out; t.part_v = part_v_out; t.part_w = part_w_out;
  HIPC(launch_iql_value_seed(t, (hipStream_t)stream));
  IqlActorArgs m;
  memset((void*)&m, 0, sizeof m);
  m.pi = pi; m.a = a; m.w = w_out;
  m.two_inv_B = 2.0f / (float)B;
  m.B = B; m.A = A; m.n_slices = t.n_slices;
  m.da = da_out; m.part = part_a_out;
  HIPC(launch_iql_actor_seed(m, (hipStream_t)stream));
  return OPRL_OK;
}

// ---------------------------------------------------------------- conservative Q-learning
// The CQL mode of a SAC learner (learner.hip cql_critic_step).  Every refusal comes before any GPU work and changes nothing.
namespace {
bool cql_alpha_ok(const char* who, double cql_alpha) {
  if (!std::isfinite(cql_alpha) || cql_alpha < 0.0 || !std::isfinite((float)cql_alpha)) {
    set_err("%s: cql_alpha=%g is not a finite number >= 0", who, cql_alpha);
    return false;
  }
  return true;
}
}  // namespace

extern "C" int oprl_learner_set_cql(oprl_learner* h, double cql_alpha, int32_t n_actions) {
  if (!h) { set_err("oprl_learner_set_cql: null learner handle"); return OPRL_ERR_INVALID; }
  if (n_actions < 0 || n_actions > kCqlMaxActions) {
    set_err("oprl_learner_set_cql: n_actions=%d outside 0..%d (0 turns the mode off; 3 n_actions entries per row)", n_actions, kCqlMaxActions);
    return OPRL_ERR_INVALID;
  }
  if (n_actions == 0) {            // off: plain SAC again (the rows stay for the next turn-on), the calibrated form with it
    h->cql_n = 0;
    h->calql_on = false;
    return OPRL_OK;
  }
  if (h->cfg.algo != OPRL_SAC) {
    set_err("oprl_learner_set_cql: conservative Q-learning is a mode of SAC learners (algo %d): twin critics, a tanh-Gaussian actor and a temperature", h->cfg.algo);
    return OPRL_ERR_INVALID;
  }
  if (h->bf16 || h->x2) { set_err("oprl_learner_set_cql: the mode runs the exact-fp32 generic launch sequence only (precision f32)"); return OPRL_ERR_INVALID; }
  if (!cql_alpha_ok("oprl_learner_set_cql", cql_alpha)) return OPRL_ERR_INVALID;
  // (a member of a group is a fused learner: said first, so that the message names the reason that cannot be lifted)
  if (h->group_member) { set_err("oprl_learner_set_cql: the learner is a member of a group (packed learners run the fused launches, which have no wide critic step)"); return OPRL_ERR_STATE; }
  if (h->fused) {
    set_err("oprl_learner_set_cql: the learner's fused launch form is on, which has no wide critic step; create it with no_fuse");
    return OPRL_ERR_STATE;
  }
  if (h->cfg.export_grads || h->rccl.comm != nullptr || h->p2p_ok) {
    set_err("oprl_learner_set_cql: gradient-exporting (export_grads) / data-parallel learners have no conservative-Q-learning step");
    return OPRL_ERR_STATE;
  }
  if (h->cql_base == nullptr) {      // the mode's rows, once: no update allocates
    const size_t Bm = (size_t)h->Bmax, slices = (Bm + kR - 1) / kR, A = (size_t)h->A, S = (size_t)h->S, nc = (size_t)h->nc;
    // (Pool::take rounds every block up to 256 bytes: 64 floats of slack for each of the 7 blocks)
    const size_t n = 2 * Bm * 2 * A + Bm * S + Bm * A + Bm + nc * Bm + nc * slices * 4 + 8 * 64;
    float* p = nullptr;
    if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) { set_err("hipMalloc(%zu) failed (conservative-Q-learning rows)", n * sizeof(float)); return OPRL_ERR_NOMEM; }
    hipError_t e = hipMemset(p, 0, n * sizeof(float));
    if (e != hipSuccess) { (void)hipFree(p); HIPC(e); }
    Pool pool;
    pool.base = reinterpret_cast<char*>(p); pool.cap = n * sizeof(float);
    h->cql_raw_s = pool.take<float>(Bm * 2 * A);
    h->cql_raw_s2 = pool.take<float>(Bm * 2 * A);
    h->cql_ws = pool.take<float>(Bm * S);
    h->cql_wa = pool.take<float>(Bm * A);
    h->cql_logd = pool.take<float>(Bm);
    h->cql_seed = pool.take<float>(nc * Bm);
    h->cql_part = pool.take<float>(nc * slices * 4);
    if (pool.used > pool.cap) { (void)hipFree(p); set_err("internal: the conservative-Q-learning rows overran their allocation"); return OPRL_ERR_STATE; }
    h->cql_base = p;
    h->cql_B = 0;
  }
  h->cql_alpha = cql_alpha;
  h->cql_n = n_actions;
  return OPRL_OK;
}

// The calibrated form of the mode (Cal-QL): the updates then need the rows' returns-to-go.
extern "C" int oprl_learner_set_calql(oprl_learner* h, int32_t on) {
  if (!h) { set_err("oprl_learner_set_calql: null learner handle"); return OPRL_ERR_INVALID; }
  if (!on) { h->calql_on = false; return OPRL_OK; }
  if (h->cql_n == 0) {
    set_err("oprl_learner_set_calql: the conservative-Q-learning mode is off (oprl_learner_set_cql first): the calibrated bound is a form of its penalty");
    return OPRL_ERR_STATE;
  }
  if (h->calql_ep == nullptr) {      // step_n's slots and returns-to-go, once: no update allocates
    const size_t Bm = (size_t)h->Bmax;
    int* p = nullptr;
    if (hipMalloc(&p, 3 * Bm * sizeof(int)) != hipSuccess) { set_err("hipMalloc(%zu) failed (calibrated-Q-learning rows)", 3 * Bm * sizeof(int)); return OPRL_ERR_NOMEM; }
    hipError_t e = hipMemset(p, 0, 3 * Bm * sizeof(int));
    if (e != hipSuccess) { (void)hipFree(p); HIPC(e); }
    h->calql_ep = p;
    h->calql_step = p + Bm;
    h->calql_g = reinterpret_cast<float*>(p + 2 * Bm);
  }
  h->calql_on = true;
  return OPRL_OK;
}

extern "C" int oprl_learner_set_cql_noise(oprl_learner* h, const float* eps, const float* uni) {
  if (!h) { set_err("oprl_learner_set_cql_noise: null learner handle"); return OPRL_ERR_INVALID; }
  h->cql_eps = eps;
  h->cql_uni = uni;
  return OPRL_OK;
}

extern "C" int oprl_learner_read_cql(oprl_learner* h, float out_host[8], void* stream) {
  if (!h || !out_host) { set_err("oprl_learner_read_cql: null argument"); return OPRL_ERR_INVALID; }
  if (h->cql_base == nullptr) { set_err("oprl_learner_read_cql: the conservative-Q-learning mode was never on (oprl_learner_set_cql)"); return OPRL_ERR_STATE; }
  hipStream_t st = (hipStream_t)stream;
  const int B = h->cql_B, n = B > 0 ? (B + kR - 1) / kR : 0, nc = h->nc < 2 ? h->nc : 2;
  std::vector<float> pc((size_t)nc * n * 4, 0.f);
  if (n > 0) HIPC(hipMemcpyAsync(pc.data(), h->cql_part, sizeof(float) * 4 * n * nc, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  RC(check_device_error(h));
  for (int k = 0; k < 8; ++k) out_host[k] = 0.f;
  if (n == 0) return OPRL_OK;
  const double N = (double)h->cql_last_n;
  double bound = 0;                                   // the calibrated form's count of bounded entries, over the critics
  for (int j = 0; j < nc; ++j) {
    double s[3] = {0, 0, 0};                          // the per-slice sums, in slice order
    for (int i = 0; i < n; ++i) {
      for (int k = 0; k < 3; ++k) s[k] += (double)pc[((size_t)j * n + i) * 4 + k];
      if (h->cql_last_cal) bound += (double)pc[((size_t)j * n + i) * 4 + 3];
    }
    // per critic: mean (lse - q) | mean q on the uniform actions | mean q on the actions drawn from pi(.|s)
    out_host[j] = (float)(s[0] / (double)B);
    out_host[2 + j] = (float)(s[1] / ((double)B * N));
    out_host[4 + j] = (float)(s[2] / ((double)B * N));
  }
  out_host[6] = (float)(h->cql_alpha * ((double)out_host[0] + (double)out_host[1]));     // the penalty term of the summed critic loss
  if (h->cql_last_cal) out_host[7] = (float)(bound / ((double)nc * (double)B * 2.0 * N));   // the share of policy entries at the bound
  return OPRL_OK;
}

extern "C" int oprl_cql_rows(const float* s, const float* a, const float* raw_s, const float* raw_s2, const float* eps, const float* uni,
                             uint64_t seed, uint64_t counter, int32_t B, int32_t S, int32_t A, int32_t N, float* ws_out, float* wa_out,
                             float* logd_out, void* stream) {
  if (!s || !a || !raw_s || !raw_s2 || !ws_out || !wa_out || !logd_out) { set_err("oprl_cql_rows: null argument"); return OPRL_ERR_INVALID; }
  if (B < 1 || S < 1 || A < 1 || N < 1 || N > kCqlMaxActions || (int64_t)B * (1 + 3 * N) * (S > A ? S : A) > (1 << 30)) {
    set_err("oprl_cql_rows: need B >= 1 (B=%d), S >= 1 (S=%d), A >= 1 (A=%d), n_actions in 1..%d (%d) and B (1 + 3 n_actions) max(S, A) <= 2^30",
            B, S, A, kCqlMaxActions, N);
    return OPRL_ERR_INVALID;
  }
  CqlRowsArgs g;
  memset((void*)&g, 0, sizeof g);
  g.s = s; g.a = a; g.raw_s = raw_s; g.raw_s2 = raw_s2; g.eps = eps; g.uni = uni;
  g.key_eps = noise_key(seed, 0, 4); g.key_uni = noise_key(seed, 0, 5); g.ctr = counter;
  g.B = B; g.S = S; g.A = A; g.N = N;
  g.ws = ws_out; g.wa = wa_out; g.logd = logd_out;
  HIPC(launch_cql_rows(g, (hipStream_t)stream));
  return OPRL_OK;
}

namespace {
// k_cql_seed on caller-supplied rows; g null: the plain kernel, else the calibrated one
int cql_seed_rows(const char* who, const float* q, const float* qn1, const float* qn2, const float* logp2, const float* r, const float* d,
                  const float* logd, const float* g, double alpha, double gamma, double cql_alpha, int32_t nc, int32_t B, int32_t N,
                  float* seed_out, float* y_out, float* part_out, float* part_cql_out, void* stream) {
  if (!q || !qn1 || !r || !d || !logd || !seed_out || !part_out || !part_cql_out) { set_err("%s: null argument", who); return OPRL_ERR_INVALID; }
  if (nc < 1 || nc > OPRL_MAX_CRITICS || B < 1 || N < 1 || N > kCqlMaxActions || (int64_t)B * (1 + 3 * N) > (1 << 30)) {
    set_err("%s: need critics in 1..%d (%d), B >= 1 (B=%d), n_actions in 1..%d (%d) and B (1 + 3 n_actions) <= 2^30",
            who, OPRL_MAX_CRITICS, nc, B, kCqlMaxActions, N);
    return OPRL_ERR_INVALID;
  }
  if (!cql_alpha_ok(who, cql_alpha)) return OPRL_ERR_INVALID;
  const long Bw = (long)B * (1 + 3 * N);
  CqlSeedArgs t;
  memset((void*)&t, 0, sizeof t);
  t.s.p0 = qn1; t.s.p1 = qn2; t.s.p2 = logp2;
  t.s.alpha_const = (float)alpha; t.s.r = r; t.s.d = d; t.s.gamma = (float)gamma;
  t.s.cval = 1.0f / (float)B;
  t.s.y_out = y_out;
  t.q = q; t.q_stride = Bw; t.logd = logd;
  t.ca = (float)cql_alpha;
  t.seed = seed_out; t.seed_stride = Bw;
  t.partials = part_out; t.part_cql = part_cql_out;
  t.nc = nc; t.B = B; t.N = N; t.n_slices = (B + kR - 1) / kR;
  t.g = g;
  HIPC(launch_cql_seed(t, (hipStream_t)stream));
  return OPRL_OK;
}
}  // namespace

extern "C" int oprl_cql_seed(const float* q, const float* qn1, const float* qn2, const float* logp2, const float* r, const float* d,
                             const float* logd, double alpha, double gamma, double cql_alpha, int32_t nc, int32_t B, int32_t N,
                             float* seed_out, float* y_out, float* part_out, float* part_cql_out, void* stream) {
  return cql_seed_rows("oprl_cql_seed", q, qn1, qn2, logp2, r, d, logd, nullptr, alpha, gamma, cql_alpha, nc, B, N, seed_out, y_out,
                       part_out, part_cql_out, stream);
}

extern "C" int oprl_cql_seed_cal(const float* q, const float* qn1, const float* qn2, const float* logp2, const float* r, const float* d,
                                 const float* logd, double alpha, double gamma, double cql_alpha, int32_t nc, int32_t B, int32_t N,
                                 float* seed_out, float* y_out, float* part_out, float* part_cql_out, const float* g, void* stream) {
  if (!g) { set_err("oprl_cql_seed_cal: null returns-to-go pointer"); return OPRL_ERR_INVALID; }
  return cql_seed_rows("oprl_cql_seed_cal", q, qn1, qn2, logp2, r, d, logd, g, alpha, gamma, cql_alpha, nc, B, N, seed_out, y_out,
                       part_out, part_cql_out, stream);
}

// ---------------------------------------------------------------- building blocks
namespace {
struct TmpBuf {  // small per-thread device scratch for the stand-alone MLP calls
  float* p = nullptr;
  size_t cap = 0;
  float* get(size_t floats) {
    if (floats > cap) {
      if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); p = nullptr; cap = 0; }
      if (hipMalloc(&p, floats * sizeof(float)) != hipSuccess) return nullptr;
      cap = floats;
    }
    return p;
  }
};
thread_local TmpBuf g_tmp;
bool g_attrs_done = false;
}  // namespace

extern "C" int oprl_mlp_forward(const oprl_net* net, int32_t use_target, const float* x0, int32_t k0,
                                const float* x1, int32_t k1, int32_t B, int32_t out_act, float* out,
                                void* stream) {
  if (!net || !x0 || !out || B < 1) { set_err("oprl_mlp_forward: invalid argument"); return OPRL_ERR_INVALID; }
  int width = 0;
  RC(check_net(*net, "net", &width));
  if (use_target && !net->theta_target) { set_err("oprl_mlp_forward: no target arena"); return OPRL_ERR_INVALID; }
  if (k0 + (x1 ? k1 : 0) != net->dims[0]) { set_err("oprl_mlp_forward: k0+k1=%d != input dim %d", k0 + (x1 ? k1 : 0), net->dims[0]); return OPRL_ERR_INVALID; }
  if (out_act != ACT_NONE && out_act != ACT_TANH && out_act != ACT_GAUSS_MEAN) { set_err("oprl_mlp_forward: out_act %d unsupported here", out_act); return OPRL_ERR_INVALID; }
  if (!g_attrs_done) { HIPC(init_kernel_attrs()); g_attrs_done = true; }
  RC(fresh32(net, (hipStream_t)stream));
  MlpArgs a;
  memset(&a, 0, sizeof a);
  a.net = net_view(*net, use_target != 0);
  a.B = B; a.do_fwd = 1;
  a.x0 = x0; a.k0 = k0; a.x1 = x1; a.k1 = x1 ? k1 : 0;
  a.out_act = out_act;
  const int nout = net->dims[net->n_layers];
  a.action_dim = nout / 2;
  a.out = out; a.ldo = (out_act == ACT_GAUSS_MEAN) ? nout / 2 : nout;
  return launch(a, width, (hipStream_t)stream);
}

// One observation in HOST memory -> one output row in HOST memory: what a policy's explore() /
// exploit() does once per environment step (reference nn_models.py:138-150, 180-195: as_tensor ->
// forward -> .cpu()).  Pinned staging rows on both sides, one H2D copy, one slice launch, one D2H
// copy and a stream sync — four runtime calls instead of the dozen torch dispatches around
// oprl_mlp_forward (37 us for as_tensor alone).
namespace {
struct ActStage {
  std::mutex mu;
  float* host = nullptr;   // pinned: [0, 256) observation, [256, 512) output
  float* dev = nullptr;    // device: same layout
};
ActStage g_act;
}  // namespace

extern "C" int oprl_mlp_act(const oprl_net* net, const float* obs_host, int32_t k0, int32_t out_act,
                            float* out_host, int32_t n_out, void* stream) {
  if (!net || !obs_host || !out_host) { set_err("oprl_mlp_act: invalid argument"); return OPRL_ERR_INVALID; }
  int width = 0;
  RC(check_net(*net, "net", &width));
  const int nout = net->dims[net->n_layers];
  const int want = (out_act == ACT_GAUSS_MEAN) ? nout / 2 : nout;
  if (k0 != net->dims[0] || k0 > 256 || n_out != want || want > 256) {
    set_err("oprl_mlp_act: dims (%d in, %d out) do not match the net (%d in, %d out)", k0, n_out, net->dims[0], want);
    return OPRL_ERR_INVALID;
  }
  if (out_act != ACT_NONE && out_act != ACT_TANH && out_act != ACT_GAUSS_MEAN) { set_err("oprl_mlp_act: out_act %d unsupported here", out_act); return OPRL_ERR_INVALID; }
  if (!g_attrs_done) { HIPC(init_kernel_attrs()); g_attrs_done = true; }
  hipStream_t st = (hipStream_t)stream;
  RC(fresh32(net, st));
  std::lock_guard<std::mutex> lk(g_act.mu);
  if (g_act.host == nullptr) {
    HIPC(hipHostMalloc((void**)&g_act.host, 512 * sizeof(float), hipHostMallocDefault));
    HIPC(hipMalloc((void**)&g_act.dev, 512 * sizeof(float)));
  }
  memcpy(g_act.host, obs_host, sizeof(float) * k0);
  HIPC(hipMemcpyAsync(g_act.dev, g_act.host, sizeof(float) * k0, hipMemcpyHostToDevice, st));
  MlpArgs a;
  memset(&a, 0, sizeof a);
  a.net = net_view(*net, false);
  a.B = 1; a.do_fwd = 1;
  a.x0 = g_act.dev; a.k0 = k0;
  a.out_act = out_act;
  a.action_dim = nout / 2;
  a.out = g_act.dev + 256; a.ldo = want;
  RC(launch(a, width, st));
  HIPC(hipMemcpyAsync(g_act.host + 256, g_act.dev + 256, sizeof(float) * want, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  memcpy(out_host, g_act.host + 256, sizeof(float) * want);
  return OPRL_OK;
}

extern "C" int oprl_mlp_backward(const oprl_net* net, const float* x0, int32_t k0, const float* x1,
                                 int32_t k1, int32_t B, const float* dout, float* dx, void* stream) {
  if (!net || !x0 || !dout || B < 1 || !net->grad) { set_err("oprl_mlp_backward: invalid argument (grad arena required)"); return OPRL_ERR_INVALID; }
  int width = 0;
  RC(check_net(*net, "net", &width));
  if (k0 + (x1 ? k1 : 0) != net->dims[0]) { set_err("oprl_mlp_backward: input dims mismatch"); return OPRL_ERR_INVALID; }
  if (!g_attrs_done) { HIPC(init_kernel_attrs()); g_attrs_done = true; }
  hipStream_t st = (hipStream_t)stream;
  RC(fresh32(net, st));
  NetWs ws;
  float* base = g_tmp.get(net_ws_floats(*net, B) + sizeof(DwItem) * kMaxLayers / sizeof(float) + 2048);
  if (!base) { set_err("oprl_mlp_backward: scratch allocation failed"); return OPRL_ERR_NOMEM; }
  Pool p; p.base = (char*)base; p.cap = (size_t)-1;
  alloc_net_ws(p, *net, B, &ws);
  std::vector<DwItem> items;
  int tiles = 0;
  fill_items(*net, ws, items, &tiles);
  MlpArgs a;
  memset(&a, 0, sizeof a);
  a.net = net_view(*net, false);
  a.B = B; a.do_fwd = 1; a.do_bwd = 1;
  a.x0 = x0; a.k0 = k0; a.x1 = x1; a.k1 = x1 ? k1 : 0;
  with_store(a, ws, true, true);
  a.seed_mode = SEED_PTR;
  const int nout = net->dims[net->n_layers];
  a.seed.p0 = dout; a.seed.ld0 = nout;
  if (dx) { a.dact_col0 = 0; a.dact_cols = net->dims[0]; a.dact = dx; a.lddact = net->dims[0]; }
  if (dx && net->dims[0] > kNarrowMax) { set_err("oprl_mlp_backward: dx supported for input dim <= %d", kNarrowMax); return OPRL_ERR_INVALID; }
  RC(launch(a, width, st));
  DwArgs dw;
  dw.items = items.data(); dw.n_items = (int)items.size(); dw.total_tiles = tiles; dw.B = B;
  set_adam(dw.ad, 0.0, 0.9, 0.999, 1e-8, 0.0);
  set_step(dw.ad, 1); dw.ad.grad_scale = 1.0f; dw.ad.do_adam = 0;
  HIPC(launch_dw_prof(nullptr, dw, st));
  return OPRL_OK;
}

extern "C" int oprl_adam_step(float* theta, float* m, float* v, const float* grad, int64_t n,
                              int32_t step, double lr, double beta1, double beta2, double eps,
                              double grad_scale, void* stream) {
  if (!theta || !m || !v || !grad || n < 1 || step < 1) { set_err("oprl_adam_step: invalid argument"); return OPRL_ERR_INVALID; }
  AdamScalars ad;
  memset(&ad, 0, sizeof ad);
  set_adam(ad, lr, beta1, beta2, eps, 0.0);
  set_step(ad, step); ad.do_adam = 1; ad.grad_scale = (float)grad_scale;
  HIPC(launch_adam_flat(theta, m, v, nullptr, grad, (long)n, ad, (hipStream_t)stream));
  return OPRL_OK;
}

extern "C" int oprl_polyak(float* target, const float* source, int64_t n, double tau, void* stream) {
  if (!target || !source || n < 1) { set_err("oprl_polyak: invalid argument"); return OPRL_ERR_INVALID; }
  HIPC(launch_polyak_flat(target, source, (long)n, tau, (hipStream_t)stream));
  return OPRL_OK;
}

