// learner_modes.hip — the modes of the generic learner (state: learner_modes.h), one section each: the state's allocation,
// the set_* / read_* entry points and the stand-alone seed calls of the C-ABI, and the mode's step of the generic launch
// sequence (learner_generic.hip picks it in its step-3 and step-6/7 chains).  Host code only.
// Every step has one form: a net forward with the activations stored | the mode's seed kernel | the net backward from the
// seed rows (SEED_PTR), so that the dW + Adam launch behind it reads what it always reads.
#include "learner_internal.h"
#include "per_seed.h"
#include "c51_seed.h"
#include "bc_seed.h"
#include "iql_seed.h"
#include "cql_seed.h"

#include <cmath>
#include <vector>

// One zeroed allocation of a mode's own, made when the mode is first turned on: no update allocates
static int mode_block(const char* what, size_t bytes, void** out) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) { set_err("hipMalloc(%zu) failed (%s rows)", bytes, what); return OPRL_ERR_NOMEM; }
  const hipError_t e = hipMemset(p, 0, bytes);
  if (e != hipSuccess) { (void)hipFree(p); HIPC(e); }
  *out = p;
  return OPRL_OK;
}

void oprl_host::free_modes(oprl_learner* h) {
  void* const blocks[6] = {h->per.seed, h->bc.seed, h->iql.base, h->cql.base, h->cql.ep, h->ln.base};
  for (void* p : blocks)
    if (p != nullptr) (void)hipFree(p);
}

// What set_bc, set_iql and set_cql refuse alike, in this order (a member of a group is a fused learner: said first, so that
// the message names the reason that cannot be lifted): the fused launches lack `fused_lacks`, the data-parallel learners `dp_lacks`
static int refuse_fused_or_dp(const oprl_learner* h, const char* who, const char* fused_lacks, const char* dp_lacks) {
  if (h->group_member) { set_err("%s: the learner is a member of a group (packed learners run the fused launches, which have no %s)", who, fused_lacks); return OPRL_ERR_STATE; }
  if (h->fused) { set_err("%s: the learner's fused launch form is on, which has no %s; create it with no_fuse", who, fused_lacks); return OPRL_ERR_STATE; }
  if (h->cfg.export_grads || h->rccl.comm != nullptr || h->p2p_ok) {
    set_err("%s: gradient-exporting (export_grads) / data-parallel learners have no %s", who, dp_lacks);
    return OPRL_ERR_STATE;
  }
  return OPRL_OK;
}

// ---------------------------------------------------------------- prioritized weights (entry points: learner_per.hip)
// the weighted seeds [nc][Bmax] | step_n_prio's weights [Bmax] | |TD| [Bmax] | slots [Bmax]: one allocation, on first use
int oprl_host::per_alloc(oprl_learner* h) {
  if (h->per.seed != nullptr) return OPRL_OK;
  const size_t Bm = (size_t)h->Bmax;
  RC(mode_block("prioritized training", ((size_t)h->nc + 3) * Bm * sizeof(float), (void**)&h->per.seed));
  h->per.w = h->per.seed + (size_t)h->nc * Bm;
  h->per.td = h->per.w + Bm;
  h->per.slots = reinterpret_cast<int*>(h->per.td + Bm);
  return OPRL_OK;
}

// Step 3 of the generic critic phase under importance weights (rows.w; oprl_learner_update_weighted): the launch that is
// forward + seed + backward there, as three — q into qpi (idle until the actor phase), k_td_weighted_seed (per_seed.hip) on
// those q and the target operands SEED_MSE_TD takes.  The same rounds (for_each_net) and the same stores.
int oprl_host::weighted_critic_step(oprl_learner* h, const StepRows& rows, int B, int n_min, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  const int nc = h->nc;
  if (h->per.seed == nullptr || rows.td_abs == nullptr) { set_err("internal: weighted critic step without its buffers"); return OPRL_ERR_STATE; }
  RC(for_each_net(h, nc, h->w_critic, st, [&](int j) {
    return forward_args(h, c.critics[j], h->ws_critic[j], true, rows.cur.s, rows.cur.a, B, h->qpi + (size_t)j * h->Bmax, 1);
  }));
  TdSeedArgs t;
  memset((void*)&t, 0, sizeof t);
  t.s = mse_td_seed(h, rows.cur.r, rows.cur.d, B, n_min);
  t.s.y_out = h->ydbg; t.s.q_out = h->qdbg;
  t.q = h->qpi; t.q_stride = h->Bmax;
  t.w = rows.w;
  t.seed = h->per.seed; t.seed_stride = h->Bmax;
  t.td_abs = rows.td_abs;
  t.partials = h->part_c;
  t.nc = nc; t.B = B; t.n_slices = n_slices(B);
  RC(profiled(0, st, [&] { return launch_td_weighted_seed(t, st); }));
  return for_each_net(h, nc, h->w_critic, st, [&](int j) {
    return backward_args(h, c.critics[j], h->ws_critic[j], true, B, h->per.seed + (size_t)j * h->Bmax, 1);
  });
}

// ---------------------------------------------------------------- D4PG's categorical critic
// the seed operands: the atoms, the row count and the logits / seed rows of this learner (c51_seed.h)
static C51Args c51_args(const oprl_learner* h, int B) {
  const oprl_net& q = h->cfg.critics[0];
  C51Args a;
  memset((void*)&a, 0, sizeof a);
  a.z = h->c51.logits;
  a.seed = h->c51.seed;
  a.gamma = (float)h->cfg.hp.gamma; a.v_min = (float)h->cfg.hp.v_min; a.v_max = (float)h->cfg.hp.v_max;
  a.inv_B = 1.0f / (float)B;
  a.N = q.dims[q.n_layers]; a.B = B; a.ld = h->ldq;
  a.n_slices = n_slices(B);
  return a;
}

// Step 3 of the generic critic phase: the critic's logits into c51.logits | k_c51_critic_seed (c51_seed.hip) on those
// logits and the target critic's (qn) | the critic's backward from the seed rows (ld0 = ldq)
int oprl_host::c51_critic_step(oprl_learner* h, const StepRows& rows, int B, hipStream_t st) {
  const oprl_net& q = h->cfg.critics[0];
  if (h->c51.logits == nullptr || h->c51.seed == nullptr) { set_err("internal: categorical critic step without its buffers"); return OPRL_ERR_STATE; }
  RC(for_each_net(h, 1, h->w_critic, st, [&](int) { return forward_args(h, q, h->ws_critic[0], true, rows.cur.s, rows.cur.a, B, h->c51.logits, h->ldq); }));
  C51Args t = c51_args(h, B);
  t.zt = h->qn;
  t.r = rows.cur.r; t.d = rows.cur.d;
  t.q_out = h->qdbg; t.y_out = h->ydbg;
  t.partials = h->part_c;
  RC(profiled(3, st, [&] { return launch_c51_critic_seed(t, st); }));
  return for_each_net(h, 1, h->w_critic, st, [&](int) { return backward_args(h, q, h->ws_critic[0], true, B, h->c51.seed, h->ldq); });
}

// Steps 6/7 of the generic actor phase: the critic on (s, pi), its logits | the seed -(1/B) p_j (z_j - Q) of the loss
// -(1/B) sum_b Q_b (k_c51_actor_seed) | the backward that leaves the action gradients
int oprl_host::c51_action_grads(oprl_learner* h, const StepRows& rows, int B, hipStream_t st) {
  const oprl_net& q = h->cfg.critics[0];
  if (h->c51.logits == nullptr || h->c51.seed == nullptr) { set_err("internal: categorical actor step without its buffers"); return OPRL_ERR_STATE; }
  RC(for_each_net(h, 1, h->w_critic, st, [&](int) { return forward_args(h, q, h->ws_critic[0], false, rows.cur.s, h->pi, B, h->c51.logits, h->ldq); }));
  C51Args t = c51_args(h, B);
  t.partials = h->part_a;
  RC(profiled(3, st, [&] { return launch_c51_actor_seed(t, st); }));
  return for_each_net(h, 1, h->w_critic, st, [&](int) {
    MlpArgs f = backward_args(h, q, h->ws_critic[0], false, B, h->c51.seed, h->ldq);
    dact_to(f, h, 0);
    return f;
  });
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
// The behaviour-cloning mode of a TD3 learner's actor step.  Every refusal comes before any GPU work and changes nothing.
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
  RC(refuse_fused_or_dp(h, "oprl_learner_set_bc", "BC step", "BC step"));
  if (h->iql.on) { set_err("oprl_learner_set_bc: the learner's implicit-Q-learning mode is on (oprl_learner_set_iql), whose actor step runs no critic"); return OPRL_ERR_STATE; }
  if (alpha > 0.0 && h->bc.seed == nullptr) {
    const size_t n = (size_t)h->Bmax + 4 + (size_t)bc_mix_slices(h->Bmax, h->A);
    RC(mode_block("behaviour-cloning", n * sizeof(float), (void**)&h->bc.seed));
    h->bc.scal = h->bc.seed + h->Bmax;
    h->bc.part = h->bc.scal + 4;
  }
  h->bc.alpha = alpha;
  return OPRL_OK;
}

extern "C" int oprl_learner_read_bc(oprl_learner* h, float out_host[4], void* stream) {
  if (!h || !out_host) { set_err("oprl_learner_read_bc: null argument"); return OPRL_ERR_INVALID; }
  if (h->bc.seed == nullptr) { set_err("oprl_learner_read_bc: the behaviour-cloning mode was never on (oprl_learner_set_bc)"); return OPRL_ERR_STATE; }
  hipStream_t st = (hipStream_t)stream;
  const int n = h->bc.parts;
  std::vector<float> host(4 + (size_t)n, 0.f);
  HIPC(hipMemcpyAsync(host.data(), h->bc.scal, sizeof(float) * (4 + (size_t)n), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  RC(check_device_error(h));
  double sq = 0.0;                                  // k_bc_mix's partial sums, in slice order
  for (int i = 0; i < n; ++i) sq += (double)host[4 + i];
  out_host[0] = host[0];                            // lambda
  out_host[1] = host[1];                            // mean |Q1(s, pi(s))|
  out_host[2] = n > 0 ? (float)(sq / ((double)h->bc.B * (double)h->A)) : 0.f;   // mean (pi - a)^2
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
  t.q = q; t.alpha = (float)alpha; t.B = B; t.n_slices = n_slices(B);
  t.seed = seed_out; t.scal = scal_out; t.partials = part_q_out;
  HIPC(launch_bc_seed(t, (hipStream_t)stream));
  BcMixArgs m;
  memset((void*)&m, 0, sizeof m);
  m.pi = pi; m.a = a; m.da = da; m.part = part_sq_out; m.B = B; m.A = A;
  HIPC(launch_bc_mix(m, (hipStream_t)stream));
  return OPRL_OK;
}

// Steps 6/7 of the generic actor phase: where TD3 runs one forward + backward launch of critic 0 from SEED_CONST -1/B, the
// seed is -lambda/B with lambda = alpha / mean |Q1(s, pi)|, which needs every row's q first — so critic 0's q into qpi (idle
// since the critic step) | k_bc_seed | critic 0's backward from the seed rows (ld0 = 1), and k_bc_mix, which adds
// (2 / (B A)) (pi - a) to the action gradients
int oprl_host::bc_action_grads(oprl_learner* h, const StepRows& rows, int B, hipStream_t st) {
  const oprl_net& q = h->cfg.critics[0];
  if (h->cfg.algo != OPRL_TD3 || h->bc.seed == nullptr) { set_err("internal: behaviour-cloning actor step without its buffers"); return OPRL_ERR_STATE; }
  RC(for_each_net(h, 1, h->w_critic, st, [&](int) { return forward_args(h, q, h->ws_critic[0], false, rows.cur.s, h->pi, B, h->qpi, 1); }));
  BcSeedArgs t;
  memset((void*)&t, 0, sizeof t);
  t.q = h->qpi; t.alpha = (float)h->bc.alpha;
  t.B = B; t.n_slices = n_slices(B);
  t.seed = h->bc.seed; t.scal = h->bc.scal; t.partials = h->part_a;
  RC(profiled(3, st, [&] { return launch_bc_seed(t, st); }));
  RC(for_each_net(h, 1, h->w_critic, st, [&](int) {
    MlpArgs f = backward_args(h, q, h->ws_critic[0], false, B, h->bc.seed, 1);
    dact_to(f, h, 0);
    return f;
  }));
  BcMixArgs m;
  memset((void*)&m, 0, sizeof m);
  m.pi = h->pi; m.a = rows.cur.a; m.da = h->da; m.part = h->bc.part;
  m.B = B; m.A = h->A;
  RC(profiled(3, st, [&] { return launch_bc_mix(m, st); }));
  h->bc.parts = bc_mix_slices(B, h->A); h->bc.B = B;
  return OPRL_OK;
}

// ---------------------------------------------------------------- implicit Q-learning
// The IQL mode of a TD3 learner.  Every refusal comes before any GPU work and changes nothing.
// (as the kernels see them, floats: neither overflowing nor flushed to zero)
static bool iql_hparams_ok(const char* who, double expectile, double beta, double adv_clip) {
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

extern "C" int oprl_learner_set_iql(oprl_learner* h, const oprl_net* value, double expectile, double beta, double adv_clip,
                                    double lr_value) {
  if (!h) { set_err("oprl_learner_set_iql: null learner handle"); return OPRL_ERR_INVALID; }
  IqlMode& m = h->iql;
  if (value == nullptr) {          // off: plain TD3 again (the rows stay for the next turn-on; V's step count is kept)
    m.on = false;
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
  RC(refuse_fused_or_dp(h, "oprl_learner_set_iql", "value net", "implicit-Q-learning step"));
  if (h->bc.alpha > 0.0) { set_err("oprl_learner_set_iql: the learner's behaviour-cloning mode is on (oprl_learner_set_bc); turn it off first"); return OPRL_ERR_STATE; }
  // the mode's rows, once per shape of V
  bool same = m.base != nullptr && m.value.n_layers == value->n_layers;
  for (int l = 0; same && l <= value->n_layers; ++l) same = m.value.dims[l] == value->dims[l];
  if (!same) {
    const size_t Bm = (size_t)h->Bmax, slices = (size_t)n_slices(h->Bmax);
    // (Pool::take rounds every block up to 256 bytes: 64 floats of slack for each of the 7 blocks behind the workspace)
    const size_t n = net_ws_floats(*value, h->Bmax) + 5 * Bm + 2 * slices * 4 + 8 * 64;
    float* p = nullptr;
    RC(mode_block("implicit-Q-learning", n * sizeof(float), (void**)&p));
    if (m.base != nullptr) (void)hipFree(m.base);
    m.base = p;
    Pool pool;
    pool.base = reinterpret_cast<char*>(p); pool.cap = n * sizeof(float);
    m.ws = NetWs{};
    alloc_net_ws(pool, *value, h->Bmax, &m.ws);
    m.vn = pool.take<float>(Bm);
    m.vs = pool.take<float>(Bm);
    m.u = pool.take<float>(Bm);
    m.w = pool.take<float>(Bm);
    m.seed = pool.take<float>(Bm);
    m.part_v = pool.take<float>(slices * 4);
    m.part_w = pool.take<float>(slices * 4);
    if (pool.used > pool.cap) { set_err("internal: the implicit-Q-learning rows overran their allocation"); m.on = false; return OPRL_ERR_STATE; }
    m.B = 0;
  }
  m.value = *value;
  m.items.clear();
  m.tiles = 0;
  fill_items(m.value, m.ws, m.items, &m.tiles);
  m.tau = expectile; m.beta = beta; m.clip = adv_clip; m.lr = lr_value;
  m.on = true;
  return OPRL_OK;
}

extern "C" int oprl_learner_read_iql(oprl_learner* h, float out_host[8], void* stream) {
  if (!h || !out_host) { set_err("oprl_learner_read_iql: null argument"); return OPRL_ERR_INVALID; }
  if (h->iql.base == nullptr) { set_err("oprl_learner_read_iql: the implicit-Q-learning mode was never on (oprl_learner_set_iql)"); return OPRL_ERR_STATE; }
  hipStream_t st = (hipStream_t)stream;
  const int B = h->iql.B, n = B > 0 ? n_slices(B) : 0;
  std::vector<float> pv((size_t)n * 4, 0.f), pw((size_t)n * 4, 0.f), pa((size_t)n * 4, 0.f);
  if (n > 0) {
    HIPC(hipMemcpyAsync(pv.data(), h->iql.part_v, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(pw.data(), h->iql.part_w, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, st));
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
  *out_host = h->iql.opt_step;
  return OPRL_OK;
}

extern "C" int oprl_learner_set_iql_step(oprl_learner* h, int64_t step) {
  if (!h) { set_err("oprl_learner_set_iql_step: null learner handle"); return OPRL_ERR_INVALID; }
  if (step < 0 || step > 0x7fffffffLL) { set_err("oprl_learner_set_iql_step: step %lld out of range", (long long)step); return OPRL_ERR_INVALID; }
  h->iql.opt_step = (int)step;
  return OPRL_OK;
}

// k_iql_value_seed's operands but for the rows it reads and writes
static IqlValueArgs iql_value_args(double expectile, double beta, double adv_clip, int B) {
  IqlValueArgs t;
  memset((void*)&t, 0, sizeof t);
  t.tau = (float)expectile; t.omtau = (float)(1.0 - expectile);
  t.beta = (float)beta; t.clip = (float)adv_clip;
  t.inv_B = 1.0f / (float)B;
  t.B = B; t.n_slices = n_slices(B);
  return t;
}

// k_iql_actor_seed: the action gradients (2/B) w_b (pi - a), written in full, and the sums of w (pi - a)^2
static hipError_t iql_actor_seed(const float* pi, const float* a, const float* w, int B, int A, float* da, float* part, hipStream_t st) {
  IqlActorArgs m;
  memset((void*)&m, 0, sizeof m);
  m.pi = pi; m.a = a; m.w = w;
  m.two_inv_B = 2.0f / (float)B;
  m.B = B; m.A = A; m.n_slices = n_slices(B);
  m.da = da; m.part = part;
  return launch_iql_actor_seed(m, st);
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
  IqlValueArgs t = iql_value_args(expectile, beta, adv_clip, B);
  t.q1 = q1; t.q2 = q2; t.v = v;
  t.u = u_out; t.seed = seed_out; t.w = w_out; t.part_v = part_v_out; t.part_w = part_w_out;
  HIPC(launch_iql_value_seed(t, (hipStream_t)stream));
  HIPC(iql_actor_seed(pi, a, w_out, B, A, da_out, part_a_out, (hipStream_t)stream));
  return OPRL_OK;
}

// The critic phase of a TD3 learner with the mode on.  No action outside the batch is evaluated: V on s' where TD3 runs the
// target actor and the target critics on (s', a'), the target critics on the batch's own (s, a), V's expectile step as
// forward | k_iql_value_seed | backward from SEED_PTR with a dW + Adam launch of its own (its item table, its learning rate,
// its step count; no target, no Polyak), then TD3's critic launch with the one target row V(s') — taken BEFORE V's step —
// and the critics' unchanged dW + Adam + Polyak: 8 launches.
int oprl_host::iql_critic_phase(oprl_learner* h, const StepRows& rows, int B, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  const float *s = rows.cur.s, *a = rows.cur.a;
  IqlMode& m = h->iql;
  const oprl_net& V = m.value;
  if (rows.w != nullptr) { set_err("internal: importance weights reached the implicit-Q-learning critic step"); return OPRL_ERR_STATE; }
  if (c.algo != OPRL_TD3 || h->nc != 2 || m.base == nullptr) { set_err("internal: implicit-Q-learning critic step without its buffers"); return OPRL_ERR_STATE; }
  const int wv = V.dims[1];
  // 1. V(s'), from V as it is before this update's step
  {
    MlpArgs f = base_args(h, V, false, B);
    f.do_fwd = 1;
    f.x0 = rows.cur.s2; f.k0 = h->S;
    f.out = m.vn; f.ldo = 1;
    RC(launch(f, wv, st));
  }
  // 2. the target critics on (s, a)
  RC(for_each_net(h, 2, h->w_critic, st, [&](int j) {
    MlpArgs f = base_args(h, c.critics[j], true, B);
    f.do_fwd = 1;
    f.x0 = s; f.k0 = h->S; f.x1 = a; f.k1 = h->A;
    f.out = h->qn + (size_t)j * h->Bmax * h->ldq; f.ldo = h->ldq;
    return f;
  }));
  // 3. V's step: forward on s with the activations stored | the seed rows, u and w | backward from the seed rows
  RC(launch(forward_args(h, V, m.ws, true, s, nullptr, B, m.vs, 1), wv, st));
  IqlValueArgs t = iql_value_args(m.tau, m.beta, m.clip, B);
  t.q1 = h->qn; t.q2 = h->qn + (size_t)h->Bmax * h->ldq; t.v = m.vs;
  t.u = m.u; t.seed = m.seed; t.w = m.w;
  t.part_v = m.part_v; t.part_w = m.part_w;
  RC(profiled(3, st, [&] { return launch_iql_value_seed(t, st); }));
  m.B = B;
  RC(launch(backward_args(h, V, m.ws, true, B, m.seed, 1), wv, st));
  // 4. V's dW + Adam, committed to V's counter only
  {
    DwArgs dw;
    dw.items = m.items.data();
    dw.n_items = (int)m.items.size();
    dw.total_tiles = m.tiles;
    dw.ad = adam_scalars(h, m.lr, m.opt_step + 1, false, 1.0f);
    dw.B = B;
    dw.n_part = tp_generic(h, V, B) ? 4 : 1;
    dw.dy_tiled = dw.n_part > 1 ? 1 : 0;
    HIPC(launch_dw_prof(h, dw, st));
    m.opt_step += 1;
  }
  // 5. the online critics: TD3's launch, y = r + ((1 - d) gamma) V(s'); 6. their dW + Adam + Polyak
  RC(for_each_net(h, 2, h->w_critic, st, [&](int j) {
    MlpArgs f = critic_sa_args(h, j, s, a, B, true);
    f.partials = h->part_c + (size_t)j * n_slices(B) * 4;
    f.seed_mode = SEED_MSE_TD;
    f.seed = mse_td_seed(h, rows.cur.r, rows.cur.d, B, 0);
    f.seed.p0 = m.vn; f.seed.p1 = nullptr; f.seed.p2 = nullptr;
    if (j == 0) { f.seed.y_out = h->ydbg; f.seed.q_out = h->qdbg; }
    return f;
  }));
  return dw_step(h, true, B, st);
}

// Steps 6/7 of the generic actor phase: no critic runs on (s, pi).  The action gradients come from the weights the critic
// phase's k_iql_value_seed left (the sums go to part_a)
int oprl_host::iql_action_grads(oprl_learner* h, const StepRows& rows, int B, hipStream_t st) {
  if (h->cfg.algo != OPRL_TD3 || h->iql.base == nullptr) { set_err("internal: implicit-Q-learning actor step without its buffers"); return OPRL_ERR_STATE; }
  return profiled(3, st, [&] { return iql_actor_seed(h->pi, rows.cur.a, h->iql.w, B, h->A, h->da, h->part_a, st); });
}

// ---------------------------------------------------------------- conservative Q-learning
// The CQL mode of a SAC learner and its calibrated form.  Every refusal comes before any GPU work and changes nothing.
static bool cql_alpha_ok(const char* who, double cql_alpha) {
  if (!std::isfinite(cql_alpha) || cql_alpha < 0.0 || !std::isfinite((float)cql_alpha)) {
    set_err("%s: cql_alpha=%g is not a finite number >= 0", who, cql_alpha);
    return false;
  }
  return true;
}

extern "C" int oprl_learner_set_cql(oprl_learner* h, double cql_alpha, int32_t n_actions) {
  if (!h) { set_err("oprl_learner_set_cql: null learner handle"); return OPRL_ERR_INVALID; }
  CqlMode& m = h->cql;
  if (n_actions < 0 || n_actions > kCqlMaxActions) {
    set_err("oprl_learner_set_cql: n_actions=%d outside 0..%d (0 turns the mode off; 3 n_actions entries per row)", n_actions, kCqlMaxActions);
    return OPRL_ERR_INVALID;
  }
  if (n_actions == 0) {            // off: plain SAC again (the rows stay for the next turn-on), the calibrated form with it
    m.n = 0;
    m.cal_on = false;
    return OPRL_OK;
  }
  if (h->cfg.algo != OPRL_SAC) {
    set_err("oprl_learner_set_cql: conservative Q-learning is a mode of SAC learners (algo %d): twin critics, a tanh-Gaussian actor and a temperature", h->cfg.algo);
    return OPRL_ERR_INVALID;
  }
  if (h->bf16 || h->x2) { set_err("oprl_learner_set_cql: the mode runs the exact-fp32 generic launch sequence only (precision f32)"); return OPRL_ERR_INVALID; }
  if (!cql_alpha_ok("oprl_learner_set_cql", cql_alpha)) return OPRL_ERR_INVALID;
  RC(refuse_fused_or_dp(h, "oprl_learner_set_cql", "wide critic step", "conservative-Q-learning step"));
  if (h->ln.on) { set_err("oprl_learner_set_cql: the learner's critics carry layer normalisation (oprl_learner_set_layernorm), which the wide critic step does not run"); return OPRL_ERR_STATE; }
  if (m.base == nullptr) {
    const size_t Bm = (size_t)h->Bmax, slices = (size_t)n_slices(h->Bmax), A = (size_t)h->A, S = (size_t)h->S, nc = (size_t)h->nc;
    // (Pool::take rounds every block up to 256 bytes: 64 floats of slack for each of the 7 blocks)
    const size_t n = 2 * Bm * 2 * A + Bm * S + Bm * A + Bm + nc * Bm + nc * slices * 4 + 8 * 64;
    float* p = nullptr;
    RC(mode_block("conservative-Q-learning", n * sizeof(float), (void**)&p));
    Pool pool;
    pool.base = reinterpret_cast<char*>(p); pool.cap = n * sizeof(float);
    m.raw_s = pool.take<float>(Bm * 2 * A);
    m.raw_s2 = pool.take<float>(Bm * 2 * A);
    m.ws = pool.take<float>(Bm * S);
    m.wa = pool.take<float>(Bm * A);
    m.logd = pool.take<float>(Bm);
    m.seed = pool.take<float>(nc * Bm);
    m.part = pool.take<float>(nc * slices * 4);
    if (pool.used > pool.cap) { (void)hipFree(p); set_err("internal: the conservative-Q-learning rows overran their allocation"); return OPRL_ERR_STATE; }
    m.base = p;
    m.B = 0;
  }
  m.alpha = cql_alpha;
  m.n = n_actions;
  return OPRL_OK;
}

// The calibrated form of the mode (Cal-QL): the updates then need the rows' returns-to-go.
extern "C" int oprl_learner_set_calql(oprl_learner* h, int32_t on) {
  if (!h) { set_err("oprl_learner_set_calql: null learner handle"); return OPRL_ERR_INVALID; }
  CqlMode& m = h->cql;
  if (!on) { m.cal_on = false; return OPRL_OK; }
  if (h->ln.on) { set_err("oprl_learner_set_calql: the learner's critics carry layer normalisation (oprl_learner_set_layernorm), which the conservative penalty's step does not run"); return OPRL_ERR_STATE; }
  if (m.n == 0) {
    set_err("oprl_learner_set_calql: the conservative-Q-learning mode is off (oprl_learner_set_cql first): the calibrated bound is a form of its penalty");
    return OPRL_ERR_STATE;
  }
  if (m.ep == nullptr) {      // step_n's slots and returns-to-go
    const size_t Bm = (size_t)h->Bmax;
    RC(mode_block("calibrated-Q-learning", 3 * Bm * sizeof(int), (void**)&m.ep));
    m.step = m.ep + Bm;
    m.g = reinterpret_cast<float*>(m.ep + 2 * Bm);
  }
  m.cal_on = true;
  return OPRL_OK;
}

extern "C" int oprl_learner_set_cql_noise(oprl_learner* h, const float* eps, const float* uni) {
  if (!h) { set_err("oprl_learner_set_cql_noise: null learner handle"); return OPRL_ERR_INVALID; }
  h->cql.eps = eps;
  h->cql.uni = uni;
  return OPRL_OK;
}

extern "C" int oprl_learner_read_cql(oprl_learner* h, float out_host[8], void* stream) {
  if (!h || !out_host) { set_err("oprl_learner_read_cql: null argument"); return OPRL_ERR_INVALID; }
  const CqlMode& m = h->cql;
  if (m.base == nullptr) { set_err("oprl_learner_read_cql: the conservative-Q-learning mode was never on (oprl_learner_set_cql)"); return OPRL_ERR_STATE; }
  hipStream_t st = (hipStream_t)stream;
  const int B = m.B, n = B > 0 ? n_slices(B) : 0, nc = h->nc < 2 ? h->nc : 2;
  std::vector<float> pc((size_t)nc * n * 4, 0.f);
  if (n > 0) HIPC(hipMemcpyAsync(pc.data(), m.part, sizeof(float) * 4 * n * nc, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  RC(check_device_error(h));
  for (int k = 0; k < 8; ++k) out_host[k] = 0.f;
  if (n == 0) return OPRL_OK;
  const double N = (double)m.last_n;
  double bound = 0;                                   // the calibrated form's count of bounded entries, over the critics
  for (int j = 0; j < nc; ++j) {
    double s[3] = {0, 0, 0};                          // the per-slice sums, in slice order
    for (int i = 0; i < n; ++i) {
      for (int k = 0; k < 3; ++k) s[k] += (double)pc[((size_t)j * n + i) * 4 + k];
      if (m.last_cal) bound += (double)pc[((size_t)j * n + i) * 4 + 3];
    }
    // per critic: mean (lse - q) | mean q on the uniform actions | mean q on the actions drawn from pi(.|s)
    out_host[j] = (float)(s[0] / (double)B);
    out_host[2 + j] = (float)(s[1] / ((double)B * N));
    out_host[4 + j] = (float)(s[2] / ((double)B * N));
  }
  out_host[6] = (float)(m.alpha * ((double)out_host[0] + (double)out_host[1]));     // the penalty term of the summed critic loss
  if (m.last_cal) out_host[7] = (float)(bound / ((double)nc * (double)B * 2.0 * N));   // the share of policy entries at the bound
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

// k_cql_seed on caller-supplied rows; g null: the plain kernel, else the calibrated one
static int cql_seed_rows(const char* who, const float* q, const float* qn1, const float* qn2, const float* logp2, const float* r, const float* d,
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
  t.nc = nc; t.B = B; t.N = N; t.n_slices = n_slices(B);
  t.g = g;
  HIPC(launch_cql_seed(t, (hipStream_t)stream));
  return OPRL_OK;
}

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

// the mode's critic step runs on B (1 + 3 N) rows of the workspace
int oprl_host::cql_rows_fit(const oprl_learner* h, const char* who, int B) {
  if (h->cql.n == 0 || (long)B * (1 + 3 * h->cql.n) <= (long)h->Bmax) return OPRL_OK;
  set_err("%s: the conservative-Q-learning mode's critic step needs batch x (1 + 3 n_actions) = %d x %d = %ld rows of a workspace "
          "of max_batch=%d; create the learner with a larger max_batch or lower n_actions", who, B, 1 + 3 * h->cql.n,
          (long)B * (1 + 3 * h->cql.n), h->Bmax);
  return OPRL_ERR_INVALID;
}

// Step 3 of the generic critic phase at a wider row count: Bw = B (1 + 3 N) rows, the minibatch's (s, a) first and then N
// uniform actions, N from pi(.|s_b) and N from pi(.|s'_b) per state, all at s_b (cql_seed.h has the layout).  The actor's raw
// head row on s' is step 1's (raw_out); the one on s is a forward-only launch here: the actor does not run N times.  Then
// k_cql_rows | the critics' q on the wide rows into qpi | k_cql_seed | the critics' backward from the seed rows: 5 launches
// where SAC has 1, and step 4's dW + Adam + Polyak reads what it always reads, Bw rows of it.
int oprl_host::cql_critic_step(oprl_learner* h, const StepRows& rows, int B, hipStream_t st) {
  const oprl_learner_config& c = h->cfg;
  CqlMode& m = h->cql;
  const int S = h->S, A = h->A, nc = h->nc, N = m.n;
  const int Bw = B * (1 + 3 * N);
  if (rows.w != nullptr) { set_err("internal: importance weights reached the conservative-Q-learning critic step"); return OPRL_ERR_STATE; }
  if (c.algo != OPRL_SAC || m.base == nullptr || Bw > h->Bmax) { set_err("internal: conservative-Q-learning critic step without its buffers"); return OPRL_ERR_STATE; }
  {
    MlpArgs f = base_args(h, c.actor, false, B);
    f.do_fwd = 1;
    f.x0 = rows.cur.s; f.k0 = S;
    f.out = m.raw_s; f.ldo = 2 * A;
    f.out_act = ACT_NONE;
    RC(launch(f, h->w_actor, st));
  }
  CqlRowsArgs g;
  memset((void*)&g, 0, sizeof g);
  g.s = rows.cur.s; g.a = rows.cur.a;
  g.raw_s = m.raw_s; g.raw_s2 = m.raw_s2;
  g.eps = m.eps; g.uni = m.uni;
  g.key_eps = noise_key(h, 4); g.key_uni = noise_key(h, 5);       // (streams 1 .. 3: the update's two and REDQ's subset)
  g.ctr = (unsigned long long)h->update_count;
  g.B = B; g.S = S; g.A = A; g.N = N;
  g.ws = m.ws; g.wa = m.wa; g.logd = m.logd;
  RC(profiled(3, st, [&] { return launch_cql_rows(g, st); }));
  RC(for_each_net(h, nc, h->w_critic, st, [&](int j) {
    return forward_args(h, c.critics[j], h->ws_critic[j], true, m.ws, m.wa, Bw, h->qpi + (size_t)j * h->Bmax, 1);
  }));
  CqlSeedArgs t;
  memset((void*)&t, 0, sizeof t);
  t.s = mse_td_seed(h, rows.cur.r, rows.cur.d, B, 0);
  t.s.y_out = h->ydbg; t.s.q_out = h->qdbg;
  t.q = h->qpi; t.q_stride = h->Bmax;
  t.logd = m.logd;
  t.ca = (float)m.alpha;
  t.seed = m.seed; t.seed_stride = h->Bmax;
  t.partials = h->part_c; t.part_cql = m.part;
  t.nc = nc; t.B = B; t.N = N; t.n_slices = n_slices(B);
  t.g = rows.g;                    // the calibrated seed when the rows carry returns-to-go
  RC(profiled(3, st, [&] { return launch_cql_seed(t, st); }));
  m.B = B; m.last_n = N; m.last_cal = rows.g != nullptr;
  return for_each_net(h, nc, h->w_critic, st, [&](int j) {
    return backward_args(h, c.critics[j], h->ws_critic[j], true, Bw, m.seed + (size_t)j * h->Bmax, 1);
  });
}

// ---------------------------------------------------------------- LayerNorm critics (ln_slice.hip)
// Linear -> LayerNorm -> ReLU in both hidden layers of every critic of a SAC / REDQ learner (the RLPD / DroQ block).  The
// parameters are the caller's, outside the nets' arenas; the critics' passes go to the LN slice kernels (net_rounds.hip),
// and the parameters step with the critic optimiser (ln_adam_step, beside step 4 of the generic critic phase).
extern "C" int oprl_learner_set_layernorm(oprl_learner* h, const oprl_layernorm* ln) {
  const char* who = "oprl_learner_set_layernorm";
  if (!h) { set_err("%s: null learner handle", who); return OPRL_ERR_INVALID; }
  if (!ln) { set_err("%s: null oprl_layernorm", who); return OPRL_ERR_INVALID; }
  const oprl_learner_config& c = h->cfg;
  if (c.algo != OPRL_SAC && c.algo != OPRL_REDQ) {
    set_err("%s: layer normalisation is built for the critics of SAC and REDQ learners (algo %d)", who, c.algo);
    return OPRL_ERR_INVALID;
  }
  if (h->bf16 || h->x2) { set_err("%s: the LN slice kernels run exact fp32 only (precision f32)", who); return OPRL_ERR_INVALID; }
  for (int j = 0; j < h->nc; ++j) {
    const oprl_net& n = c.critics[j];
    if (n.n_layers != kLnHidden + 1 || n.dims[1] != kLnWidth || n.dims[2] != kLnWidth || n.dims[3] != 1) {
      set_err("%s: critic %d is not a three-layer net of hidden width %d with one output", who, j, kLnWidth);
      return OPRL_ERR_INVALID;
    }
  }
  if (!ln->theta || !ln->theta_target || !ln->adam_m || !ln->adam_v) { set_err("%s: null parameter array (theta, theta_target, adam_m, adam_v)", who); return OPRL_ERR_INVALID; }
  if (!std::isfinite(ln->eps) || !(ln->eps > 0.f)) { set_err("%s: eps=%g must be finite and positive", who, (double)ln->eps); return OPRL_ERR_INVALID; }
  RC(refuse_fused_or_dp(h, who, "LN kernels", "LN step"));
  if (h->cql.n > 0) { set_err("%s: the learner's conservative-Q-learning mode is on (oprl_learner_set_cql), whose wide critic step has no LN form", who); return OPRL_ERR_STATE; }
  LnMode& m = h->ln;
  if (m.on) { set_err("%s: the mode is already on (it is set once, before the first update)", who); return OPRL_ERR_STATE; }
  if (h->update_count > 0) { set_err("%s: the learner has run %lld updates; the mode is set before the first", who, (long long)h->update_count); return OPRL_ERR_STATE; }
  const size_t Bm = (size_t)h->Bmax, slices = (size_t)n_slices(h->Bmax), nc = (size_t)h->nc;
  const size_t n_zh = nc * kLnHidden * Bm * kLnWidth, n_rstd = nc * kLnHidden * Bm, n_sums = nc * kLnHidden * slices * 2 * kLnWidth;
  float* p = nullptr;
  RC(mode_block("layer-normalisation", (n_zh + n_rstd + n_sums + 3 * 64) * sizeof(float), (void**)&p));
  Pool pool;
  pool.base = reinterpret_cast<char*>(p); pool.cap = (n_zh + n_rstd + n_sums + 3 * 64) * sizeof(float);
  float* zh = pool.take<float>(n_zh);
  float* rstd = pool.take<float>(n_rstd);
  m.sums = pool.take<float>(n_sums);
  if (pool.used > pool.cap) { (void)hipFree(p); m.sums = nullptr; set_err("internal: the layer-normalisation rows overran their allocation"); return OPRL_ERR_STATE; }
  m.base = p;
  m.slices = (int)slices;
  m.theta = ln->theta; m.theta_target = ln->theta_target; m.adam_m = ln->adam_m; m.adam_v = ln->adam_v;
  m.eps = ln->eps;
  for (int j = 0; j < h->nc; ++j) {
    LnView v;
    memset((void*)&v, 0, sizeof v);
    v.eps = m.eps;
    v.gb = m.theta_target + (size_t)j * kLnNetFloats;
    m.target[j] = v;
    v.gb = m.theta + (size_t)j * kLnNetFloats;
    for (int l = 0; l < kLnHidden; ++l) {
      v.zh[l] = zh + ((size_t)j * kLnHidden + l) * Bm * kLnWidth;
      v.rstd[l] = rstd + ((size_t)j * kLnHidden + l) * Bm;
    }
    v.sums = m.sums + (size_t)j * kLnHidden * slices * 2 * kLnWidth;
    v.sum_slices = (int)slices;
    m.online[j] = v;
  }
  m.on = true;
  return OPRL_OK;
}

// ---------------------------------------------------------------- dropout in the LN critics
static bool drop_rate_ok(float rate) { return rate >= 0.f && rate < 1.f; }      // (NaN fails both)

// a view's dropout fields but the pass's stream: threshold (uint32)(rate 2^32) (0: off), scale 1 / (1 - rate) in float32
static void set_drop(LnView& v, float rate, uint64_t key) {
  v.drop_thresh = (uint32_t)((double)rate * 4294967296.0);
  v.drop_scale = v.drop_thresh != 0 ? 1.0f / (1.0f - rate) : 1.0f;
  v.drop_key = v.drop_thresh != 0 ? key : 0;
}

// Linear -> Dropout -> LayerNorm -> ReLU in every critic pass of a learner whose LN mode is on: the views get the key of
// threshold and the scale here, and the key of noise stream 6 and the pass's stream T before each launch (base_args).
extern "C" int oprl_learner_set_dropout(oprl_learner* h, float rate) {
  const char* who = "oprl_learner_set_dropout";
  if (!h) { set_err("%s: null learner handle", who); return OPRL_ERR_INVALID; }
  if (!drop_rate_ok(rate)) { set_err("%s: rate=%g must lie in [0, 1)", who, (double)rate); return OPRL_ERR_INVALID; }
  LnMode& m = h->ln;
  if (!m.on) { set_err("%s: the critics carry no layer normalisation (oprl_learner_set_layernorm comes first: dropout runs inside the LN kernels)", who); return OPRL_ERR_STATE; }
  if (m.drop_rate > 0.f) { set_err("%s: the mode is already on (it is set once, before the first update)", who); return OPRL_ERR_STATE; }
  if (h->update_count > 0) { set_err("%s: the learner has run %lld updates; the mode is set before the first", who, (long long)h->update_count); return OPRL_ERR_STATE; }
  LnView probe;
  memset((void*)&probe, 0, sizeof probe);
  set_drop(probe, rate, 0);
  if (probe.drop_thresh == 0) return OPRL_OK;      // (rate 0, or below 2^-32: the mode stays off)
  m.drop_rate = rate;
  // (the key follows the learner's seed, which may be set later: base_args writes it with the stream)
  for (int j = 0; j < h->nc; ++j) { set_drop(m.online[j], rate, 0); set_drop(m.target[j], rate, 0); }
  return OPRL_OK;
}

// k_ln_adam: every critic's per-slice dgamma / dbeta sums of this update's critic step, added in slice order, and the
// Adam (+ Polyak when critic_targets_due) step with lr_critic at the step count of the critics' dW launch — which the
// caller makes next and which commits the count (dw_commit)
int oprl_host::ln_adam_step(oprl_learner* h, int B, hipStream_t st) {
  const LnMode& m = h->ln;
  LnAdamArgs a;
  memset((void*)&a, 0, sizeof a);
  a.theta = m.theta; a.target = m.theta_target; a.m = m.adam_m; a.v = m.adam_v;
  a.sums = m.sums;
  a.n_nets = h->nc; a.n_slices = n_slices(B); a.sum_slices = m.slices;
  a.ad = adam_scalars(h, h->cfg.hp.lr_critic, h->opt_step_critic + 1, critic_targets_due(h), 1.0f);
  RC(profiled(1, st, [&] { return launch_ln_adam(a, st); }));
  return OPRL_OK;
}

// One packed three-layer net of width 256 with LN parameters ln_theta [2][gamma | beta][256] on caller rows [x0 | x1]:
// forward, and — given dout [B][n_out] — backward from those seed rows (SEED_PTR).  split = 0: one launch; 1: a
// forward-only launch that keeps x, zh and rstd, then a backward-only launch that reloads them.  Row arrays hold `rows`
// (>= B) rows per hidden layer: x / dz / zh [2][rows][256], rstd [2][rows]; dx1 [B][k1] the gradient over the x1 columns;
// dln [2][2][256] the reduced dgamma | dbeta.  The kernel tests' entry point (tests/test_gpu_ln_slice.py).
static int mlp_ln_run(const char* who, const oprl_net* net, const float* ln_theta, float eps, const float* x0, int32_t k0, const float* x1,
                      int32_t k1, int32_t B, int32_t rows, int32_t split, const float* dout, float* out, float* x_rows, float* dz_rows,
                      float* zh_rows, float* rstd_rows, float* dx1, float* dln, void* stream, float rate, uint64_t key, uint64_t stream_id) {
  if (!net || !ln_theta || !x0 || !out || !x_rows || !zh_rows || !rstd_rows) { set_err("%s: null argument", who); return OPRL_ERR_INVALID; }
  if (dout != nullptr && (!dz_rows || !dln)) { set_err("%s: a backward (dout) needs dz_rows and dln", who); return OPRL_ERR_INVALID; }
  int width = 0;
  RC(check_net(*net, "net", &width));
  if (net->n_layers != kLnHidden + 1 || width != kLnWidth) { set_err("%s: the LN kernels take a three-layer net of hidden width %d", who, kLnWidth); return OPRL_ERR_INVALID; }
  if (B < 1 || rows < B || rows > (1 << 22)) { set_err("%s: need 1 <= B (%d) <= rows (%d) <= 2^22", who, B, rows); return OPRL_ERR_INVALID; }
  if (k0 < 1 || k0 + (x1 ? k1 : 0) != net->dims[0] || (x1 && k1 < 1)) { set_err("%s: k0+k1=%d != input dim %d", who, k0 + (x1 ? k1 : 0), net->dims[0]); return OPRL_ERR_INVALID; }
  if (dx1 != nullptr && (!x1 || !dout || k1 > kNarrowMax)) { set_err("%s: dx1 needs x1 (k1 <= %d) and dout", who, kNarrowMax); return OPRL_ERR_INVALID; }
  if (!std::isfinite(eps) || !(eps > 0.f)) { set_err("%s: eps=%g must be finite and positive", who, (double)eps); return OPRL_ERR_INVALID; }
  if (!drop_rate_ok(rate)) { set_err("%s: rate=%g must lie in [0, 1)", who, (double)rate); return OPRL_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  HIPC(init_ln_attrs());
  RC(fresh32(net, st));
  const int slices = n_slices(B), nout = net->dims[net->n_layers];
  float* sums = nullptr;
  if (dout != nullptr) RC(mode_block(who, (size_t)kLnHidden * slices * 2 * kLnWidth * sizeof(float), (void**)&sums));
  MlpArgs a;
  memset(&a, 0, sizeof a);
  a.net = net_view(*net, false);
  a.B = B;
  a.x0 = x0; a.k0 = k0; a.x1 = x1; a.k1 = x1 ? k1 : 0;
  a.out = out; a.ldo = nout;
  LnView v;
  memset((void*)&v, 0, sizeof v);
  v.gb = ln_theta; v.eps = eps;
  set_drop(v, rate, key);
  v.drop_stream = stream_id;       // (the backward-only launch below carries the forward launch's)
  for (int l = 0; l < kLnHidden; ++l) {
    a.Xg[l + 1] = x_rows + (size_t)l * rows * kLnWidth;
    if (dout != nullptr) a.dYg[l] = dz_rows + (size_t)l * rows * kLnWidth;
    v.zh[l] = zh_rows + (size_t)l * rows * kLnWidth;
    v.rstd[l] = rstd_rows + (size_t)l * rows;
  }
  a.seed_mode = SEED_PTR;
  a.seed.p0 = dout; a.seed.ld0 = nout;
  if (dx1 != nullptr) { a.dact_col0 = k0; a.dact_cols = k1; a.dact = dx1; a.lddact = k1; }
  hipError_t e = hipSuccess;
  if (dout == nullptr || split) {
    MlpArgs f = a;
    f.do_fwd = 1;
    e = launch_mlp_slice_ln(f, v, st);
  }
  if (e == hipSuccess && dout != nullptr) {
    MlpArgs b = a;
    b.do_fwd = split ? 0 : 1; b.do_bwd = 1;
    if (split) b.out = nullptr;
    LnView vb = v;
    vb.sums = sums; vb.sum_slices = slices;
    e = launch_mlp_slice_ln(b, vb, st);
    if (e == hipSuccess) {
      LnAdamArgs r;
      memset((void*)&r, 0, sizeof r);
      r.theta = dln; r.m = dln; r.v = dln;          // (do_adam 0: only the reduced gradient is written, to gout)
      r.sums = sums; r.gout = dln;
      r.n_nets = 1; r.n_slices = slices; r.sum_slices = slices;
      set_adam(r.ad, 0.0, 0.9, 0.999, 1e-8, 0.0);
      set_step(r.ad, 1); r.ad.grad_scale = 1.0f; r.ad.do_adam = 0;
      e = launch_ln_adam(r, st);
    }
  }
  if (sums != nullptr) {
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(sums);
    if (e == hipSuccess) e = e2;
  }
  HIPC(e);
  return OPRL_OK;
}

extern "C" int oprl_mlp_ln(const oprl_net* net, const float* ln_theta, float eps, const float* x0, int32_t k0, const float* x1, int32_t k1,
                           int32_t B, int32_t rows, int32_t split, const float* dout, float* out, float* x_rows, float* dz_rows,
                           float* zh_rows, float* rstd_rows, float* dx1, float* dln, void* stream) {
  return mlp_ln_run("oprl_mlp_ln", net, ln_theta, eps, x0, k0, x1, k1, B, rows, split, dout, out, x_rows, dz_rows, zh_rows, rstd_rows,
                    dx1, dln, stream, 0.f, 0, 0);
}

// oprl_mlp_ln with dropout in front of both normalisations: the mask of (key, stream_id), b the row's index
// in the batch.  The kernel tests' entry point (tests/test_gpu_droq_slice.py).
extern "C" int oprl_mlp_ln_drop(const oprl_net* net, const float* ln_theta, float eps, const float* x0, int32_t k0, const float* x1,
                                int32_t k1, int32_t B, int32_t rows, int32_t split, const float* dout, float* out, float* x_rows,
                                float* dz_rows, float* zh_rows, float* rstd_rows, float* dx1, float* dln, void* stream, float rate,
                                uint64_t key, uint64_t stream_id) {
  return mlp_ln_run("oprl_mlp_ln_drop", net, ln_theta, eps, x0, k0, x1, k1, B, rows, split, dout, out, x_rows, dz_rows, zh_rows,
                    rstd_rows, dx1, dln, stream, rate, key, stream_id);
}
