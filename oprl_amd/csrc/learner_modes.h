// learner_modes.h — the state of the learner's modes, one plain struct each (included by learner_internal.h in front of
// struct oprl_learner, which holds one member of each).  Entry points, allocation and steps: learner_modes.hip.
#pragma once

// training from prioritized replay (learner_per.hip): one allocation of its own, made by the first weighted update —
// the weighted seeds [nc][Bmax], and step_n_prio's weights, |TD| and slots [Bmax] each; null on every other learner
struct PerMode {
  float *seed = nullptr, *w = nullptr, *td = nullptr;
  int* slots = nullptr;
};

// D4PG (c51_seed.hip): the online critic's logits [Bmax][ldq] between its forward-only and backward-only launches, and
// the seed rows SEED_PTR reads; in the learner's pool, null on every other learner
struct C51Mode {
  float *logits = nullptr, *seed = nullptr;
};

// the behaviour-cloning mode of a TD3 learner's actor step (oprl_learner_set_bc, bc_seed.hip): alpha (0:
// off), and one allocation of its own, made when the mode is first turned on — the seed rows [Bmax] | lambda, mean |Q|
// and two spares [4] | k_bc_mix's partial sums [bc_mix_slices(Bmax, A)]; parts: how many the last actor step wrote
struct BcMode {
  double alpha = 0.0;
  float *seed = nullptr, *scal = nullptr, *part = nullptr;
  int parts = 0, B = 0;
};

// the implicit-Q-learning mode of a TD3 learner (oprl_learner_set_iql, iql_seed.hip): the caller's value
// net V(s) (on: the mode), its hyper-parameters and its own Adam step count, and one allocation of its own, made when
// the mode is first turned on — V's workspace rows | V(s') | V(s) | u | w | the V seed [Bmax] each | the two tables of
// k_iql_value_seed's per-slice sums [slices at Bmax][4] each (the actor's go to part_a); V's dW items with their tiles
struct IqlMode {
  bool on = false;
  oprl_net value = {};
  double tau = 0.0, beta = 0.0, clip = 0.0, lr = 0.0;
  int opt_step = 0;
  float* base = nullptr;
  NetWs ws;
  float *vn = nullptr, *vs = nullptr, *u = nullptr, *w = nullptr, *seed = nullptr;
  float *part_v = nullptr, *part_w = nullptr;
  std::vector<DwItem> items;
  int tiles = 0, B = 0;
};

// the conservative-Q-learning mode of a SAC learner (oprl_learner_set_cql, cql_seed.hip): the penalty
// weight and the sampled actions per kind (n = 0: off), and one allocation of its own, made when the mode is first
// turned on — the actor's raw head rows on s and on s' [Bmax][2A] each | the wide states [Bmax][S] and actions [Bmax][A] |
// the log-densities and the seed rows [nc][Bmax] | k_cql_seed's own per-slice sums [nc][slices at Bmax][4]; the test
// hook's noise arrays (null: Philox) and the row count of the last update with the mode on
struct CqlMode {
  double alpha = 0.0;
  int n = 0, B = 0, last_n = 0;
  float* base = nullptr;
  float *raw_s = nullptr, *raw_s2 = nullptr, *ws = nullptr, *wa = nullptr, *logd = nullptr, *seed = nullptr;
  float* part = nullptr;
  const float *eps = nullptr, *uni = nullptr;
  // the calibrated form of that mode (oprl_learner_set_calql, Cal-QL): on only while n > 0; one
  // allocation of its own, made when it is first turned on — step_n's slots (episode | step, int32) and returns-to-go,
  // [Bmax] each; whether the last update with the CQL mode on was a calibrated one (read_cql's out[7])
  bool cal_on = false, last_cal = false;
  int *ep = nullptr, *step = nullptr;
  float* g = nullptr;
};

// layer normalisation in the critics of a SAC / REDQ learner (oprl_learner_set_layernorm, ln_slice.hip):
// the caller's four arrays [nc][2 hidden layers][gamma | beta][256] (parameters, target copy, Adam m and v), eps, and one
// allocation of its own, made when the mode is turned on — the zh rows [nc][2][Bmax][256] and rstd [nc][2][Bmax] a
// forward-only launch leaves for the backward-only one | the per-slice dgamma / dbeta sums [nc][2][slices at Bmax][2][256].
// online[j] / target[j]: critic j's views as MlpArgs::reserved carries them to the launchers (net_rounds.hip).
// Dropout in front of the normalisation (oprl_learner_set_dropout): drop_rate (0: off; the views hold the
// key, threshold and scale), and drop_pass, the pass k of the stream T = (u 4 + k) 16 + j that base_args writes into a
// view before each launch of critic j — 1 in the critic phase, 2 in the actor phase; a target critic's pass is 0
struct LnMode {
  bool on = false;
  float drop_rate = 0.f;
  int drop_pass = 1;
  float *theta = nullptr, *theta_target = nullptr, *adam_m = nullptr, *adam_v = nullptr;
  float eps = 0.f;
  float* base = nullptr;
  float* sums = nullptr;
  int slices = 0;
  oprl::LnView online[OPRL_MAX_CRITICS], target[OPRL_MAX_CRITICS];
};
