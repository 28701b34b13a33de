/* oprl_amd.h — C-ABI of the MI355X-native off-policy learner (liboprl_amd.so).
 *
 * The reference (schatty/oprl) has no FFI: its "operator API" for this path is
 * two Python Protocols.  Each entry point below names the reference interface
 * it sits under (paths relative to /root/reference/src/oprl):
 *
 *   oprl_learner_*   AlgorithmProtocol.update()           algos/protocols.py:21-41
 *                    DDPG/TD3/SAC/TQC.update()            algos/ddpg.py:61, td3.py:71, sac.py:75, tqc.py:116
 *   oprl_learner_set_bc / read_bc, oprl_bc_seed   no counterpart: TD3+BC's actor loss as a mode of a TD3 learner
 *                    (Fujimoto & Gu 2021), for training from a fixed dataset
 *   oprl_learner_set_iql / read_iql / get_iql_step / set_iql_step, oprl_iql_seed   no counterpart: implicit Q-learning
 *                    (Kostrikov et al. 2021) as a mode of a TD3 learner with a caller-owned value net
 *   oprl_learner_set_cql / read_cql / set_cql_noise, oprl_cql_rows, oprl_cql_seed   no counterpart: conservative Q-learning
 *                    (Kumar et al. 2020, CQL(H)) as a mode of a SAC learner
 *   oprl_learner_set_calql / update_calql, oprl_replay_returns, oprl_cql_seed_cal   no counterpart: calibrated Q-learning
 *                    (Nakamoto et al. 2023, Cal-QL), the calibrated form of that mode
 *   oprl_learner_set_layernorm, oprl_mlp_ln   no counterpart: layer normalisation in the critics of a SAC / REDQ learner
 *                    (the RLPD / DroQ critic block)
 *   oprl_learner_set_dropout, oprl_mlp_ln_drop   no counterpart: Philox dropout in front of that normalisation (Hiraoka
 *                    et al. 2022, DroQ)
 *   oprl_replay_*    ReplayBufferProtocol              buffers/protocols.py:6-26
 *                    EpisodicReplayBuffer.{add_transition,sample}  buffers/episodic_buffer.py:81-133
 *   oprl_mlp_*       MLP / Critic / policies forward      algos/nn_models.py:27-194
 *   oprl_adam_* / oprl_polyak   torch.optim.Adam.step / soft_update  algos/nn_functions.py:5-10
 *
 * Conventions: every function returns 0 on success or a negative oprl_status;
 * oprl_last_error() returns the text of the last failure on the calling
 * thread.  No exceptions cross the boundary.  All `float*`/`void*` data
 * pointers are DEVICE pointers (HBM) unless the name ends in `_host`.  `stream`
 * is a hipStream_t passed as void* (0 = default stream); all work is enqueued
 * asynchronously on it.  The library never frees caller memory; it allocates
 * only its own workspace in *_create and frees it in *_destroy.  A handle is
 * used from one host thread at a time; distinct handles are independent.
 */
#ifndef OPRL_AMD_H
#define OPRL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPRL_ABI_VERSION 4
#define OPRL_MAX_LAYERS 4   /* linear layers per MLP (TQC critic has 4) */
#define OPRL_MAX_CRITICS 10 /* TQC n_nets (5), REDQ ensemble (10) */

typedef enum oprl_status {
  OPRL_OK = 0,
  OPRL_ERR_INVALID = -1,   /* bad argument / unsupported shape */
  OPRL_ERR_HIP = -2,       /* a HIP runtime call failed */
  OPRL_ERR_STATE = -3,     /* handle not ready (e.g. empty replay) */
  OPRL_ERR_NOMEM = -4
} oprl_status;

/* OPRL_REDQ: an ensemble of n_critics scalar critics (<= OPRL_MAX_CRITICS) with SAC's tanh-Gaussian actor; the TD
 * target takes the minimum over hp.n_min target critics drawn afresh for every update (oprl_redq_subset), the critic
 * targets move on every update and the actor (+ temperature) steps on every hp.policy_freq-th (Chen et al., ICLR 2021;
 * DESIGN.md "REDQ").  F32 only, no gradient export, never a fused form.
 * OPRL_D4PG: DDPG with ONE categorical critic (Bellemare et al. 2017; Barth-Maron et al. 2018): the critic's
 * N = dims[n_layers] outputs (2 .. 48) are logits over the atoms z_i = hp.v_min + i (hp.v_max - hp.v_min) / (N - 1); the
 * critic loss is the cross-entropy against the projected target distribution, the actor ascends Q = sum_j z_j p_j.  F32
 * only, the generic launch sequence only, no gradient export, no group membership, no importance weights. */
typedef enum oprl_algo { OPRL_DDPG = 0, OPRL_TD3 = 1, OPRL_SAC = 2, OPRL_TQC = 3, OPRL_REDQ = 4, OPRL_D4PG = 5 } oprl_algo;

/* Arithmetic mode of the MLP GEMMs.
 *   F32  = exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), the parity mode: Q-values and gradients within
 *          1e-4 of the reference (measured <= 2e-6).  A fused single-critic DDPG learner (own Adam step) runs whole
 *          updates, up to 32 per launch, in this mode too (k_ddpg_chain<PrecF32>): its kernels read and write
 *          library-owned UNCACHED mirrors of the packs below, and the caller's `pack` / `pack_target` are then
 *          maintained like an X2 learner's fp32 packs — rebuilt from the masters by every entry point that reads
 *          them (oprl_mlp_forward / backward / act, oprl_net_repack), not by the updates.
 *   BF16 = v_mfma_f32_16x16x32_bf16 with fp32 accumulation (16x the matrix rate, half the weight
 *          bytes): both GEMM operands of the forward and backward passes of the fused update kernels
 *          (DDPG / TD3 / SAC phase kernels, TQC's layer-wise critic kernels) are rounded to bf16 on the
 *          way into the matrix cores — the weights once per Adam step, into bf16 fragment packs the
 *          library owns.  Master weights, Adam moments, Polyak targets, activations in LDS / HBM, the
 *          heads, losses and the dW GEMM stay fp32.  Outside the fused kernels (oprl_mlp_forward / act /
 *          backward, generic fall-back launches for shapes the fused kernels do not cover) a BF16
 *          learner computes in fp32 from the fp32 packs.  Deviation from the reference: ~1e-3..1e-2
 *          relative on Q (bf16 inputs cannot meet the 1e-4 gate; tests/test_gpu_bf16.py states and
 *          measures the tolerance).
 *   X2   = every fp32 operand as the sum of two fp16 numbers (hi + lo), three v_mfma_f32_16x16x32_f16 per product
 *          (lo*hi + hi*lo + hi*hi) with fp32 accumulation: 22 mantissa bits per operand at 3/16 of the exact-fp32
 *          MFMA time.  Weights are kept as fp16 pairs of 2^8 w (packs of two planes the library owns), activations
 *          and gradient tiles enter scaled by a power of two (csrc/engine.h, PrecX2); accumulators, master weights,
 *          Adam and Polyak are fp32.  A PARITY mode: held to the reference's golden vectors and the CPU oracle at the
 *          F32 mode's gates (tests/test_gpu_x2.py); measured rms error of a 256-deep dot product 1.45e-7 relative (the
 *          fp32 MFMA chain: 2.8e-7).  Covers the fused DDPG / TD3 / SAC kernels — DDPG's whole updates, up to 32 per
 *          launch (k_ddpg_chain; oprl_learner_step_n) — and the hidden layers of TQC's 512-wide critics; everything else
 *          runs exact fp32.  RANGE: observations and hidden activations below 4094 in magnitude, weights below 256;
 *          leaving it is reported through the error word (oprl_learner_check / the next update return OPRL_ERR_STATE,
 *          "split-fp16 range"), never silent; F32 has no such range and is the default of the Python classes.  The fp32
 *          packs of such a learner are not kept current by its updates: every entry point that reads them
 *          (oprl_mlp_forward / backward / act, the generic launches) rebuilds them first. */
typedef enum oprl_precision { OPRL_PREC_F32 = 0, OPRL_PREC_BF16 = 1, OPRL_PREC_X2 = 2 } oprl_precision;

/* One MLP (ReLU hidden layers, identity output), parameters laid out exactly
 * like the reference module's state_dict: W0[out0,in0] row-major, b0, W1, b1...
 * (algos/nn_models.py:84-107).  theta is the trainable master copy; the other
 * arenas use the same layout and may be NULL when the net has no target / is
 * not trained. */
typedef struct oprl_net {
  int32_t n_layers;                     /* number of Linear layers, 2..OPRL_MAX_LAYERS */
  int32_t dims[OPRL_MAX_LAYERS + 1];    /* dims[0]=input ... dims[n_layers]=output */
  float* theta;
  float* theta_target;
  float* adam_m;
  float* adam_v;
  float* grad;                          /* written when grads are exported (DP / tests) */
  /* Fragment-order weight packs (device, caller-owned, oprl_net_pack_floats()
   * floats each, zero-initialised by the caller): the layout the MFMA kernels
   * stream (csrc/engine.h).  The library keeps them in step with theta /
   * theta_target whenever IT changes those (update, apply) — or, for the
   * learners named under oprl_precision, rebuilds them when one of its entry
   * points reads them; after an outside change of the master
   * (load_state_dict ...) call oprl_learner_sync_params() (every pack of the
   * learner, the library-owned ones included) or, for a net no learner of a
   * BF16 / X2 / chain kind owns, oprl_net_repack(). */
  float* pack;
  float* pack_target;                   /* NULL when there is no target */
} oprl_net;

/* Doubles on purpose: the reference's hyper-parameters are python floats and
 * torch forms 1-beta1, 1-beta2, 1-tau, lr/(1-beta1^t) in double before rounding
 * to fp32 (1.f - 0.999f differs from (float)(1 - 0.999) by 1.3e-5 relative). */
typedef struct oprl_hparams {
  double gamma, tau;
  double lr_actor, lr_critic, lr_alpha;
  double beta1, beta2, adam_eps;         /* torch defaults .9 / .999 / 1e-8 */
  double policy_noise, noise_clip, max_action;   /* TD3 (td3.py:98-103) */
  double alpha_init;                             /* SAC fixed alpha (sac.py:64) */
  double target_entropy;                         /* -action_dim */
  int32_t policy_freq;                           /* TD3 (td3.py:81); REDQ: updates per actor step (G) */
  int32_t tune_alpha;                            /* SAC (sac.py:65-70); TQC always 1 */
  int32_t n_quantiles, top_quantiles_to_drop;    /* TQC (tqc.py:71-73) */
  int32_t n_min;                                 /* REDQ: target critics in the minimum (M, 1..n_critics) */
  double v_min, v_max;                           /* D4PG: the first and the last atom (v_max > v_min); read for OPRL_D4PG only */
} oprl_hparams;

typedef struct oprl_learner_config {
  int32_t abi_version;      /* OPRL_ABI_VERSION */
  int32_t algo;             /* oprl_algo */
  int32_t precision;        /* oprl_precision */
  int32_t state_dim, action_dim;
  int32_t max_batch;        /* workspace is sized for this many rows */
  int32_t n_critics;        /* 1 DDPG / D4PG, 2 TD3/SAC, n_nets TQC, the ensemble's size REDQ */
  int32_t no_fuse;          /* 1: always use the generic per-net launch sequence (DDPG
                               otherwise runs the fused two-kernel path, csrc/fused_ddpg.hip) */
  int32_t export_grads;     /* 1: update() stops before Adam and leaves grads in
                               net.grad (data-parallel learner reduces them, then
                               calls oprl_learner_apply); 0: fused dW+Adam+Polyak */
  oprl_net actor;
  oprl_net critics[OPRL_MAX_CRITICS];
  double* log_alpha;        /* device scalar (float64 like the reference), or NULL */
  double* log_alpha_m;      /* its Adam state (device), or NULL */
  double* log_alpha_v;
  double* log_alpha_grad;   /* export_grads: d(alpha loss)/d(log_alpha) lands here */
  oprl_hparams hp;
} oprl_learner_config;

typedef struct oprl_learner oprl_learner;
typedef struct oprl_replay oprl_replay;

const char* oprl_last_error(void);
int oprl_abi_version(void);

/* ---- learner: AlgorithmProtocol.update() ------------------------------- */
int oprl_learner_create(const oprl_learner_config* cfg, oprl_learner** out);
int oprl_learner_destroy(oprl_learner* h);

/* One reference-semantics update() on a caller-supplied minibatch (row-major
 * fp32: s[B,S] a[B,A] r[B] d[B] s2[B,S]).  noise0/noise1 are the N(0,1) draws
 * the reference takes inside update() (TD3: randn_like(action), td3.py:98;
 * SAC/TQC: next-state draw then actor-step draw, nn_models.py:213), each
 * [B,A]; NULL = draw on device (Philox, keyed by seed and the update counter).*/
int oprl_learner_update(oprl_learner* h, const float* s, const float* a, const float* r,
                        const float* d, const float* s2, int32_t B,
                        const float* noise0, const float* noise1, void* stream);

/* Second half of an export_grads update: Adam (+Polyak) from net.grad after the
 * caller has all-reduced it.  phase 0 = critic(s), 1 = actor (+alpha). */
int oprl_learner_apply(oprl_learner* h, int32_t phase, double grad_scale, void* stream);
/* In export_grads mode update() is split so the reduction can sit between the
 * halves exactly where the reference's optimizer.step() sits:
 *   oprl_learner_update_phase(h, 0, batch...) -> critic grads in net.grad
 *   <all-reduce> ; oprl_learner_apply(h, 0, 1/world)
 *   oprl_learner_update_phase(h, 1, ...)      -> actor grads
 *   <all-reduce> ; oprl_learner_apply(h, 1, 1/world)                        */
int oprl_learner_update_phase(oprl_learner* h, int32_t phase, const float* s, const float* a,
                              const float* r, const float* d, const float* s2, int32_t B,
                              const float* noise0, const float* noise1, void* stream);

/* K back-to-back sample()+update() iterations with the minibatch drawn on
 * device from `replay` (the 4000-update loop of
 * distrib/policy_update_worker.py:65-68 as one call). */
int oprl_learner_step_n(oprl_learner* h, oprl_replay* replay, int32_t K, int32_t B,
                        uint64_t seed, void* stream);

/* The trainer loop's step (trainers/base_trainer.py:38-74: one update, then actor.explore(next_state) opens the next
 * environment step): oprl_learner_step_n with K = 1 and, enqueued behind it in the same call, the ACTOR's forward
 * of one observation obs_host[0 .. state_dim) with the weights that update leaves (a 1-row GEMV over the master
 * weights, csrc/policy_act.hip).  Nothing is waited for: the raw output row of the actor's last layer (no tanh, no
 * Gaussian head — what oprl_mlp_act returns with out_act = none) is collected with oprl_learner_act_wait, which
 * spins on a ticket in host-mapped memory (bounded: OPRL_ERR_STATE after `timeout_us`).  One pending row per learner. */
int oprl_learner_step_act(oprl_learner* h, oprl_replay* replay, int32_t B, uint64_t seed,
                          const float* obs_host, void* stream);
int oprl_learner_act_wait(oprl_learner* h, float* out_host, int32_t n_out, int64_t timeout_us);

/* ---- acting for many environments per launch ----------------------------------------------------
 * The actor's forward of n_rows (1 .. OPRL_ACT_ROWS_MAX) observations in ONE launch (csrc/policy_act_rows.hip: a
 * workgroup per 16 rows, exact-fp32 MFMA over the row-major MASTER weights — no packs are read, so the rows are the
 * fp32 evaluation of the masters in every precision mode).  Observations are read from, and the raw last-layer rows
 * written to, host-mapped pinned memory the learner allocates on the first such call; a row's bits do not depend on
 * n_rows, its position or its neighbours.  The pending rows have their own area and ticket: a row of
 * oprl_learner_step_act may be pending at the same time; one pending row batch per learner.  OPRL_ERR_INVALID: null
 * arguments, n_rows outside 1 .. OPRL_ACT_ROWS_MAX, dims that are not the actor's, a bad K or B; OPRL_ERR_STATE:
 * act_rows_wait with nothing pending or another n_rows than the pending one, a pending device error (as step_n).  A
 * refused call changes nothing. */
#define OPRL_ACT_ROWS_MAX 256
/* enqueue the actor's forward of n_rows observations obs_host[n_rows][state_dim] with the weights as `stream` leaves them; nothing is waited for */
int oprl_learner_act_rows(oprl_learner* h, const float* obs_host, int32_t n_rows, void* stream);
/* oprl_learner_step_n(K) and, behind it in the same call, oprl_learner_act_rows */
int oprl_learner_step_act_rows(oprl_learner* h, oprl_replay* replay, int32_t K, int32_t B, uint64_t seed,
                               const float* obs_host, int32_t n_rows, void* stream);
/* collect the raw last-layer rows out_host[n_rows][n_out]; bounded spin on the tickets (OPRL_ERR_STATE after timeout_us) */
int oprl_learner_act_rows_wait(oprl_learner* h, float* out_host, int32_t n_rows, int32_t n_out, int64_t timeout_us);

/* ---- packed learners: the reference's --seeds fan-out (runners/train.py:24-50) on ONE GPU ----------------
 * A group steps N independent fused DDPG, TD3 or SAC learners of one algorithm, shape and precision (own weights, own sampler keys
 * seeds[i], one shared HBM replay) with FOUR launches per update for all of them (grid.z = learner; the
 * argument blocks of four updates travel to device memory in one copy).  OPRL_PREC_F32 members run on
 * single-CU slices (oprl_learner_set_cluster(h, 1) is applied to them), OPRL_PREC_X2 / OPRL_PREC_BF16 members on
 * clusters of four ((h, 4): the form those precisions exist in): a member's result is bit-identical to the same
 * learner stepped alone with that cluster size, whoever else is in the group.  TD3 / SAC members (fused in the lean
 * form only): clusters of four in every precision, the twin critics back to back (OPRL_AMD_NO_TWIN_SPLIT=1 /
 * OPRL_AMD_NO_P2_PAIR=1 give a solo learner the same form); TD3's delayed actor step is taken by all members at
 * once — members whose update counts differ modulo policy_freq are refused (OPRL_ERR_STATE); SAC's temperature
 * step rides on the actor's dW launch.  The members stay ordinary learners (update / step_n / checkpoints)
 * between group calls. */
typedef struct oprl_group oprl_group;
int oprl_group_create(oprl_learner** learners, int32_t n, oprl_group** out);
int oprl_group_destroy(oprl_group* g);
int oprl_group_step_n(oprl_group* g, oprl_replay* replay, int32_t K, int32_t B, const uint64_t* seeds, void* stream);
/* CUs per 16-row slice in the fused kernels.  8 (the default): tensor-parallel clusters of four, and of EIGHT
 * for the forward-only chains where that still fits the chip (DDPG's target chain, DDPG / TD3's critic pass of
 * the actor step; exact-fp32 mode, action_dim <= 8) — lowest latency for a learner that has the GPU (nearly) to
 * itself; such launches want every CU, so learners that share a GPU with more than two others (seeds packed on
 * streams, one process per seed on one GPU) use 4: clusters of four only (also OPRL_AMD_NO_WIDE=1), and the dW + Adam
 * tiles as launches of their own instead of workgroups riding on the phase launches.  2 or 1:
 * least CU time per update (what oprl_group uses).  Results differ in the last bits between settings (order of
 * the exchange sums); a setting is part of a run's configuration like the seed. */
int oprl_learner_set_cluster(oprl_learner* h, int32_t nc);
/* Diagnostics of the most recent update, read without forcing a sync inside
 * update(): out_host[0]=critic_loss, [1]=-mean q(s, pi) (DDPG / TD3 actor loss; min over twins for SAC; mean over the
 * ensemble for REDQ),
 * [2]=mean q over all critics, [3]=mean target, [4]=alpha, [5]=update_step, and (n up to 10) [6]=mean q of
 * critic 0 (the reference's "q1"), [7]=mean log pi of the actor step, [8]=SAC / TQC actor loss
 * alpha * mean(log pi) - mean(min q), [9]=temperature loss.  Synchronises `stream`. */
int oprl_learner_read_scalars(oprl_learner* h, float* out_host, int32_t n, void* stream);
/* Rebuild every pack of the learner's nets from their masters (after the caller
 * changed parameters from outside, e.g. load_state_dict). */
int oprl_learner_sync_params(oprl_learner* h, void* stream);
int oprl_learner_update_count(oprl_learner* h, int64_t* out_host);
int oprl_learner_set_update_count(oprl_learner* h, int64_t count);
/* Checkpoint / exact resume (reference: base_trainer.py:113-120 saves only the policy).  The
 * learner's host-side state beyond the caller-owned arenas: {update_count, Adam step of the
 * critics, of the actor, of log_alpha}.  Restoring the arenas (theta, theta_target, m, v,
 * log_alpha + its m, v), these four counters and calling oprl_learner_sync_params resumes a
 * run bit for bit (tests/test_gpu_callers.py). */
#define OPRL_N_COUNTERS 4
int oprl_learner_get_counters(oprl_learner* h, int64_t out_host[OPRL_N_COUNTERS]);
int oprl_learner_set_counters(oprl_learner* h, const int64_t in_host[OPRL_N_COUNTERS]);
/* Device-side failures.  The fused update kernels and the data-parallel exchanges contain BOUNDED waits
 * between workgroups (4-CU slice clusters, the TD-target hand-off between roles, gradient tiles between
 * ranks).  An expired wait poisons its result with NaN — it cannot hang the GPU — and is REPORTED: the
 * kernel stores (kernel << 8 | wait site) into a host-visible error word of the learner.  The word is
 * checked, without any synchronisation, at the start of every oprl_learner_update / update_phase / apply /
 * step_n / dp_* call and after the synchronisation inside oprl_learner_read_scalars; once set those calls
 * return OPRL_ERR_STATE with the kernel and wait site in oprl_last_error() until it is cleared.
 * oprl_learner_check polls it explicitly (synchronise the stream first for a definitive answer);
 * oprl_learner_debug_expire (tests) makes one wait site (2 = TD-target hand-off, 1 = cluster all-reduce, 7 = gate of the dW tiles riding on phase 1's launch;
 * 0 = off) give up immediately in subsequent launches.  Sites 101, 102, 104, 105, 106 are TIMING experiments
 * (tools/what_if.py): one cross-workgroup wait of k_ddpg_chain counts as satisfied — role B's q for role A's tail,
 * the critic's tiles for the critic pass, role A's seeds / the pass's du / role B's rows for the tiles — so that
 * the change of the update's period shows what that hand-over contributes; such a learner computes wrong numbers. */
int oprl_learner_check(oprl_learner* h);
int oprl_learner_clear_error(oprl_learner* h);
int oprl_learner_debug_expire(oprl_learner* h, int32_t site);
/* Which launch form an update of batch size B would take right now (tests/test_gpu_forms.py holds the decision —
 * csrc/learner.hip fused_form — against a table; the learner is only read).  out[13]: [0] 1 fused phase kernels / 0 the generic launch
 * sequence, [1] lean (tp4.h) passes, [2] form 4 whole updates per launch (k_ddpg_chain) / 3 both merged launches / 2 merged
 * phase 1 / 1 plain phase + dW launches / 0, [3] updates per chain launch, [4] wide bits (1 role A, 2 the critic pass on
 * clusters of eight), [5] cluster size of the other roles, [6] twin_split, [7] p2_pair, [8] arithmetic 0 exact fp32 /
 * 1 bf16 / 2 x2, [9] XCD-local cluster exchanges, [10] demoted to the shared-chip forms, [11] gradient-exporting
 * learners: the form (as [2]) of a data-parallel update whose exchange runs inside the dW tiles, others 0, [12] rt2 (1 phase
 * 1's B roles on two row tiles per cluster, 2 ... and SAC's role A carries role C's pass).  Reference: none (the
 * reference has one path, autograd). */
int oprl_learner_debug_form(oprl_learner* h, int32_t B, int32_t* out);
/* Key of the learner's device-side noise streams (TD3 target smoothing, the SAC / TQC
 * reparameterisation draws, drawn with Philox when update() gets no injected noise): `seed` is the
 * run seed (the reference seeds torch's generator in runners/train.py:14-21), `rank` the
 * data-parallel rank (oprl_comm_init / oprl_p2p_create set it too) so that every seed and every
 * rank draws its own eps.  Seed 0 on rank 0 is the default. */
int oprl_learner_set_seed(oprl_learner* h, uint64_t seed, int32_t rank);
/* Test / audit export of the device-side noise: out_dev[rows][cols] = the N(0,1) draws (Philox4x32-10 +
 * Box-Muller, csrc/philox.h) the update kernels of this learner take for noise stream `stream_id` (1: next-state
 * draw / TD3 target smoothing, 2: actor-step draw) at update counter `counter`, element (row, col) = (minibatch
 * row, action dimension), under the learner's current seed and rank (oprl_learner_set_seed). */
int oprl_debug_noise(oprl_learner* h, int32_t stream_id, uint64_t counter, int32_t rows, int32_t cols,
                     float* out_dev, void* stream);
/* REDQ's target subset of update `counter` (the learner's update_count before the update) under noise key (seed, rank)
 * as oprl_learner_set_seed takes them: m distinct indices in [0, n) into out_host[0 .. m).  Philox4x32-10 (csrc/philox.h)
 * keyed like the device noise's stream 3 (key = that stream's 64-bit key, low word first), counter words {counter low,
 * counter high, block, 0}: the four 32-bit words of block k are words 4k .. 4k+3, and a partial Fisher-Yates shuffle of 0 .. n-1
 * takes, for i < m, j = i + bounded_u32(word_i, n - i) (the high 32 bits of word_i * (n - i)) and swaps perm[i], perm[j].  Host only (no GPU needed); the learner calls the same function.
 * OPRL_ERR_INVALID unless 1 <= m <= n <= OPRL_MAX_CRITICS. */
int oprl_redq_subset(uint64_t seed, int32_t rank, uint64_t counter, int32_t n, int32_t m, int32_t* out_host);
/* device pointer to the per-row Q / TD-target of the last critic step ([B] each,
 * critic 0), for parity tests. */
int oprl_learner_debug_ptrs(oprl_learner* h, const float** q, const float** y);
/* (debug) device views of what a fused DDPG update leaves in the workspace; `which` as listed at the definition */
int oprl_learner_debug_view(oprl_learner* h, int32_t which, const void** ptr, int64_t* n_bytes);

/* ---- building blocks (nn_models.py forward; used by Module.__call__) ----- */
/* floats needed for ONE pack buffer of this net (dims only are read) */
int64_t oprl_net_pack_floats(const oprl_net* net);
/* rebuild pack from theta (which & 1) and/or pack_target from theta_target (which & 2) */
int oprl_net_repack(const oprl_net* net, int32_t which, void* stream);
/* out[B,dims[L]] = MLP([x0 | x1]) with x0[B,k0], x1[B,k1] (x1 may be NULL,
 * k0+k1 == dims[0]); out_act: 0 identity, 1 tanh.  use_target selects
 * theta_target. */
int oprl_mlp_forward(const oprl_net* net, int32_t use_target, const float* x0, int32_t k0,
                     const float* x1, int32_t k1, int32_t B, int32_t out_act, float* out,
                     void* stream);
/* The per-environment-step policy call (reference nn_models.py:138-150 explore / exploit and
 * :180-195: as_tensor(state) -> forward -> .cpu()): ONE observation obs_host[k0] in host memory ->
 * out_host[n_out] in host memory (n_out = dims[L], or dims[L]/2 with out_act 4 = tanh of the
 * Gaussian mean).  Synchronous on `stream`. */
int oprl_mlp_act(const oprl_net* net, const float* obs_host, int32_t k0, int32_t out_act,
                 float* out_host, int32_t n_out, void* stream);
/* oprl_mlp_act for n_rows (1 .. OPRL_ACT_ROWS_MAX) observations at once, stand-alone and synchronous: any net of up to
 * OPRL_MAX_LAYERS layers and widths <= 512 (a policy without a learner; theta alone is read), obs_host[n_rows][k0] ->
 * the raw last-layer rows out_host[n_rows][n_out], through library-owned pinned staging. */
int oprl_mlp_act_rows(const oprl_net* net, const float* obs_host, int32_t n_rows, int32_t k0,
                      float* out_host, int32_t n_out, void* stream);
/* Gradient of sum(out * dout) wrt every parameter (into net->grad) and, if
 * dx != NULL, wrt the concatenated input [B,dims[0]].  Test/debug entry that
 * exercises the same backward + dW kernels update() uses. */
int oprl_mlp_backward(const oprl_net* net, const float* x0, int32_t k0, const float* x1,
                      int32_t k1, int32_t B, const float* dout, float* dx, void* stream);
/* torch.optim.Adam.step over a flat arena of n floats; step = 1-based count. */
int oprl_adam_step(float* theta, float* m, float* v, const float* grad, int64_t n, int32_t step,
                   double lr, double beta1, double beta2, double eps, double grad_scale,
                   void* stream);
/* target <- (1-tau)*target + tau*source  (nn_functions.py:5-10) */
int oprl_polyak(float* target, const float* source, int64_t n, double tau, void* stream);

/* ---- data parallel over RCCL (xGMI) ---------------------------------------- */
/* One process per GPU.  The library binds RCCL at run time from `rccl_path`
 * (dlopen; e.g. torch's bundled librccl.so) — it does not link it.  Rank 0 obtains
 * a 128-byte unique id, the host distributes it (any side channel, e.g.
 * torch.distributed's store), every rank calls oprl_comm_init on a learner created
 * with export_grads = 1.  oprl_learner_dp_update / dp_step_n then run the
 * synchronous data-parallel update entirely in C: critic phase -> ncclAllReduce of
 * the critic gradient arena -> Adam with grads scaled by 1/world -> actor phase ->
 * ncclAllReduce of the actor gradient arena (and the temperature gradient) -> Adam.
 * New functionality (the reference has a single learner). */
#define OPRL_COMM_ID_BYTES 128
int oprl_comm_unique_id(const char* rccl_path, char id_out[OPRL_COMM_ID_BYTES]);
int oprl_comm_init(oprl_learner* h, const char* rccl_path, int32_t rank, int32_t world,
                   const char id[OPRL_COMM_ID_BYTES]);
/* Make every replica identical to rank `root` (ncclBroadcast of every net's theta / theta_target / Adam
 * moments and of the temperature with its moments; the packs are rebuilt).  Once, after oprl_comm_init. */
int oprl_comm_broadcast_params(oprl_learner* h, int32_t root, void* stream);
/* Optional: the two gradient exchanges as ONE-SHOT all-reduces over peer windows (csrc/p2p.hip)
 * instead of RCCL rings — every rank pushes its arena straight into a slot of every other rank's
 * window over the xGMI mesh and sums the slots in rank order.  oprl_p2p_create allocates this rank's
 * window and returns its IPC handle; the host gathers the `world` handles (any side channel) and
 * passes them, in rank order, to oprl_p2p_connect; oprl_p2p_selftest (all ranks together) exchanges
 * a known pattern and reports whether this rank's sums were exact; when every rank passed, every
 * rank calls oprl_p2p_enable(h, level): 1 = the two exchanges of dp_update / dp_step_n run as one
 * window kernel each; 2 = in addition the fused learners (DDPG / TD3 / SAC) all-reduce every gradient
 * tile INSIDE their dW + Adam launches (no separate exchange or apply launches at all; the caller should
 * check after a few updates that parameters are finite and replicas identical, and step down to 1
 * otherwise — bench.py does); 0 = back to RCCL.  Without RCCL
 * (oprl_comm_init never called) a connected learner runs dp_update / dp_step_n on the windows alone. */
#define OPRL_P2P_HANDLE_BYTES 64
int oprl_p2p_create(oprl_learner* h, int32_t rank, int32_t world, char handle_out[OPRL_P2P_HANDLE_BYTES]);
int oprl_p2p_connect(oprl_learner* h, const char* handles /* world x OPRL_P2P_HANDLE_BYTES */);
int oprl_p2p_selftest(oprl_learner* h, void* stream);
int oprl_p2p_enable(oprl_learner* h, int32_t on);
int oprl_learner_dp_update(oprl_learner* h, const float* s, const float* a, const float* r,
                           const float* d, const float* s2, int32_t B, const float* noise0,
                           const float* noise1, void* stream);
int oprl_learner_dp_step_n(oprl_learner* h, oprl_replay* replay, int32_t K, int32_t B,
                           uint64_t seed, void* stream);

/* ---- measurement --------------------------------------------------------- */
/* When enabled, every kernel launch of this library is bracketed by a pair of
 * hipEvents recorded on the launch stream.  oprl_profile_read synchronises the
 * device and returns, per kernel kind, the launch count and the summed
 * hipEventElapsedTime (ms).  Kinds: 0 k_mlp_slice, 1 k_dw_adam, 2 k_replay_gather,
 * 3 everything else, 4 k_ddpg_phase1 — and every launch that starts with phase 1's roles: the merged
 * k_ddpg_phase1_dw and k_ddpg_chain (whole updates, up to 32 per launch: one count per LAUNCH) —,
 * 5 k_ddpg_phase2 (and k_ddpg_phase2_dw).  bench.py's roofline uses this. */
#define OPRL_PROFILE_KINDS 6
int oprl_profile_enable(int32_t on);
int oprl_profile_read(int64_t* counts_host, double* ms_host, int32_t reset);

/* Debug tracing: when buf != NULL every k_mlp_slice launch of this learner writes
 * per-workgroup phase timestamps (shader cycle counter, 100 MHz realtime) to
 * buf[launch_slot][64 workgroups][OPRL_TRACE_STAMPS][2] (int64, device memory);
 * launch_slot restarts at 0 with each update().  NULL disables. */
#define OPRL_TRACE_STAMPS 24
#define OPRL_TRACE_SLOTS 24
int oprl_learner_set_trace(oprl_learner* h, int64_t* buf);

/* ---- replay: ReplayBufferProtocol --------------------------------------- */
/* Storage tensors are owned by the caller (torch) with the reference layout
 * (buffers/episodic_buffer.py:29-55): states[E,L+1,S] actions[E,L,A]
 * rewards[E,L,1] dones[E,L,1], fp32, HBM resident. */
int oprl_replay_create(int32_t n_episodes, int32_t max_ep_len, int32_t state_dim,
                       int32_t action_dim, float* states, float* actions, float* rewards,
                       float* dones, oprl_replay** out);
int oprl_replay_destroy(oprl_replay* h);
/* add_transition's data movement: stage one transition (host pointers) for slot
 * [ep, t]; staged rows reach HBM in one batched copy + scatter at the next
 * flush/sample.  Index bookkeeping stays with the caller (it is host logic). */
int oprl_replay_write(oprl_replay* h, int32_t ep, int32_t t, const float* state_host,
                      const float* action_host, float reward, float done);
/* oprl_replay_write, oprl_replay_set_lens and oprl_replay_flush as one call (the per-env-step caller:
 * trainers/base_trainer.py adds one transition between two updates; the row and the changed tail of the episode
 * table travel in one small launch that runs while the host goes on to the update call). */
int oprl_replay_write_flush(oprl_replay* h, int32_t ep, int32_t t, const float* state_host,
                            const float* action_host, float reward, float done, const int32_t* ep_lens_host,
                            int32_t episodes_counter, void* stream);
/* The same for n consecutive steps [t0, t0+n) of one episode from host records
 * [state (S) | action (A) | reward | done | ...], row_stride floats apart: add_episode / a drained actor
 * ring segment in one call.  Staging that fills up is flushed on `stream`. */
int oprl_replay_write_block(oprl_replay* h, int32_t ep, int32_t t0, int32_t n, const float* rows_host,
                            int32_t row_stride, void* stream);
int oprl_replay_flush(oprl_replay* h, void* stream);
/* One step of n <= 256 open episodes in one call and one ingest launch: record i is step t[i] of
 * episode ep[i] — state s[i], action a[i], reward r[i], done d[i] — and s2[i] the state it led to, stored as
 * states[ep[i], t[i] + 1], so the next state of the last stored step of a running or truncated episode is in storage.
 * All pointers are host pointers.  On `stream`, in this order: rows the other write entry points staged
 * (oprl_replay_flush), these records, the episode table (oprl_replay_set_lens(ep_lens_host, episodes_counter)) and, on a
 * prioritized replay, the leaves.  OPRL_ERR_INVALID, with nothing staged, launched or changed, for a null pointer, n
 * outside 1 .. 256, an ep outside [0, E), a t outside [0, L), two records with one ep, and whatever
 * oprl_replay_set_lens refuses. */
int oprl_replay_write_rows(oprl_replay* h, int32_t n, const int32_t* ep, const int32_t* t, const float* s,
                           const float* a, const float* r, const float* d, const float* s2,
                           const int32_t* ep_lens_host, int32_t episodes_counter, void* stream);
/* Upload ep_lens[0:episodes_counter] (episodic_buffer.py:114-116); the device
 * keeps the cumulative ends for the flat-index -> (episode, step) map. */
int oprl_replay_set_lens(oprl_replay* h, const int32_t* ep_lens_host, int32_t episodes_counter,
                         void* stream);
/* sample(): gather B transitions.  idx (device int64[B], flat indices as
 * np.random.randint would give, episodic_buffer.py:124) or NULL to draw them
 * on device from (seed, counter).  Outputs: s[B,S] a[B,A] r[B,1] d[B,1] s2[B,S].
 * If out_ep/out_step are non-NULL the (episode, step) pairs are written too. */
int oprl_replay_sample(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed,
                       uint64_t counter, float* out_s, float* out_a, float* out_r, float* out_d,
                       float* out_s2, int32_t* out_ep, int32_t* out_step, void* stream);

/* ---- n-step returns ---------------------------------------------------------------------------------
 * A replay in n-step mode samples, for a drawn slot (e, t), m = the steps taken: at most n, never past the episode's
 * stored steps, none after the first step whose done is not 0.  The row it writes is
 *   r = sum_{k<m} gamma^k r_{t+k},  d = 1 - gamma^(m-1) (1 - d_{t+m-1})  (d_t verbatim when m = 1),  s2 = s_{t+m},
 * so that a learner's one-step target r + gamma (1 - d) q'(s2) IS the n-step target when its gamma is this one.
 * set_nstep: 1 <= n <= 16, 0 < gamma <= 1 (else OPRL_ERR_INVALID); n = 1 switches the mode off.  With n > 1
 * oprl_replay_sample and the learners' step_n / dp_step_n gather n-step rows (step_n / dp_step_n: OPRL_ERR_INVALID
 * unless gamma equals the learner's hp.gamma; oprl_group_step_n refuses such a replay).  Not combined with prioritized
 * replay: set_nstep(n > 1) on a prioritized handle and oprl_replay_prio_enable on an n-step handle return
 * OPRL_ERR_STATE.  Host state only; replays that never call it are unchanged. */
int oprl_replay_set_nstep(oprl_replay* h, int32_t n, double gamma);
/* oprl_replay_sample with the handle's (n, gamma) through the n-step gather kernel — also at n = 1, where every output
 * equals oprl_replay_sample's bit for bit — and, when out_m is non-NULL, the steps taken per row (int32[B]).  The
 * index draw is oprl_replay_sample's: the same (seed, counter) picks the same (episode, step). */
int oprl_replay_sample_nstep(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed, uint64_t counter,
                             float* out_s, float* out_a, float* out_r, float* out_d, float* out_s2, int32_t* out_ep,
                             int32_t* out_step, int32_t* out_m, void* stream);

/* ---- hindsight experience replay (Andrychowicz et al., NeurIPS 2017) ---------------------------------
 * A flat state row carries the achieved goal at [ag_off, ag_off + G) and the desired goal at [g_off, g_off + G).  A
 * replay in hindsight mode draws the slot (e, t) as oprl_replay_sample does and, with c = len_e - 1 - t later rows of
 * the episode that are always written, relabels the row iff c >= 1 and U < (float)ratio, U = (r.y >> 8) 2^-24 of the
 * draw's own Philox output r:  t' = t + bounded(r.z, c) (strategy 0, future) or len_e - 2 (strategy 1, final),
 * g' = achieved goal of states[e, t' + 1];  s and s2 get g' as their desired goal, a and d are verbatim, and
 *   r = dist2 <= (float)(threshold^2) ? 0 : -1  (reward 0, sparse)   or   r = -sqrtf(dist2)  (reward 1, dense),
 * dist2 = the float32 sum over k = 0 .. G-1, in order, of (achieved(s2)_k - g'_k)^2, every operation rounded once.
 * Rows that are not relabelled are oprl_replay_sample's bit for bit.
 * set_her: 1 <= G <= 16, both ranges inside [0, state_dim) and disjoint, 0 <= ratio <= 1, threshold finite and >= 0,
 * strategy and reward 0 or 1 (else OPRL_ERR_INVALID); G = 0 switches the mode off (the other arguments are not read).
 * With the mode on oprl_replay_sample and the learners' step_n / step_act / dp_step_n gather relabelled rows;
 * oprl_group_step_n refuses such a replay.  Not combined with n-step returns or prioritized replay: set_her on such a
 * handle, and oprl_replay_set_nstep(n > 1) / oprl_replay_prio_enable on a hindsight handle, return OPRL_ERR_STATE.
 * Host state only; replays that never call it are unchanged. */
int oprl_replay_set_her(oprl_replay* h, int32_t ag_off, int32_t g_off, int32_t G, double ratio, int32_t strategy,
                        int32_t reward, double threshold);
/* oprl_replay_sample through the hindsight gather kernel (OPRL_ERR_STATE when the mode is off) and, when out_future is
 * non-NULL, t' per relabelled row and -1 per other row (int32[B]).  With idx given the slots are the caller's; the
 * relabelling still follows (seed, counter). */
int oprl_replay_sample_her(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed, uint64_t counter,
                           float* out_s, float* out_a, float* out_r, float* out_d, float* out_s2, int32_t* out_ep,
                           int32_t* out_step, int32_t* out_future, void* stream);

/* ---- prior data in the batch ------------------------------------------------------------------------
 * Reference: none.  A replay may name a second replay, `prior` (a fixed dataset), and a share in [0, 1].  Of a batch of B
 * rows the first B_p = min(B, max(0, (int)floor(share * B + 0.5))) (double arithmetic) come from `prior` and the rest
 * from the replay itself; row i is oprl_replay_sample's row i — the same Philox call for (seed, counter, i), or idx[i] —
 * over the episode table and storage of ITS source.  So rows [0, B_p) equal those rows of oprl_replay_sample(prior, B, ...)
 * and rows [B_p, B) those of oprl_replay_sample on a plain handle with this replay's contents, bit for bit.
 * set_prior: prior non-NULL switches the mode on (share 0 is allowed), prior NULL switches it off (the share is not
 * read).  Host state only; the caller keeps `prior` alive while it is set.  OPRL_ERR_INVALID: a null h, a share that is
 * not finite or outside [0, 1], prior == h, state or action dims that differ (episode slots and steps per episode may);
 * OPRL_ERR_STATE: either handle samples n-step returns, relabels in hindsight or is prioritized, or prior has a prior of
 * its own.  A refused call changes nothing.  With the mode on oprl_replay_sample and the learners' step_n / step_act /
 * dp_step_n gather mixed batches; oprl_group_step_n refuses such a replay, and oprl_replay_set_nstep(n > 1),
 * oprl_replay_set_her(G > 0) and oprl_replay_prio_enable on it return OPRL_ERR_STATE.  Replays that never call it are
 * unchanged. */
int oprl_replay_set_prior(oprl_replay* h, oprl_replay* prior, double share);
/* The mixed batch (OPRL_ERR_STATE when the mode is off) and, when out_src is non-NULL, 1 per prior row and 0 per own row
 * (int32[B]); out_ep / out_step are the slot inside the row's source, idx[i] a flat index into it.  Both handles are
 * flushed on `stream` first.  OPRL_ERR_STATE, with nothing launched, when prior is no longer plain, or when a source
 * that has to supply at least one row holds no transitions. */
int oprl_replay_sample_mix(oprl_replay* h, int32_t B, const int64_t* idx, uint64_t seed, uint64_t counter,
                           float* out_s, float* out_a, float* out_r, float* out_d, float* out_s2, int32_t* out_ep,
                           int32_t* out_step, int32_t* out_src, void* stream);

/* ---- returns-to-go of sampled slots -------------------------------------------------------------------
 * Reference: none.  ep[B], step[B] (device, int32) are the slots (e, t) of B rows inside each row's SOURCE, exactly what
 * the gathers write to out_ep / out_step: the source is h, and with h in prior-data mode rows i < B_p (the formula above,
 * from the share on the handle: the split is by row index) read h's prior.  With len_e the episode's stored steps from
 * the source's episode table (the in-progress tail included) and T the first k >= t with dones[e, k] != 0, or len_e - 1
 * when there is none,
 *   out_g[i] = sum_{k = t .. T} gamma^(k - t) rewards[e, k]
 * with NO bootstrap at a truncation (a timeout, a dataset piece cut at L, an episode still running end the sum at the last
 * stored step): an underestimate of the return for non-negative rewards.  t >= len_e gives the single term rewards[e, t];
 * a row with e outside [0, E) or t outside [0, L) of its source reads nothing and gives 0 (the arrays are the caller's
 * and cannot be checked on the host).  float32, a fixed summation order (csrc/replay_returns.hip): the same bits in every
 * run.  Nothing is written past out_g[B].  h is flushed on `stream` first, and its prior too.  n-step and prioritized
 * handles are fine: G depends on (e, t) only.  OPRL_ERR_INVALID: a null pointer, B < 1, gamma outside (0, 1];
 * OPRL_ERR_STATE, with nothing launched: a source in hindsight mode (its rewards are relabelled per sample), a source
 * that has to supply a row and holds no transitions. */
int oprl_replay_returns(oprl_replay* h, int32_t B, const int32_t* ep, const int32_t* step, double gamma, float* out_g,
                        void* stream);

/* ---- prioritized replay (Schaul et al., ICLR 2016, proportional variant) ------------------------------------------
 * A sum tree over the E·L slots of a replay, in HBM next to it: leaf e·L + t is the priority of slot
 * (e, t).  A slot is live when e < episodes_counter and t < ep_lens[e] (the set oprl_replay_sample draws from); every
 * dead leaf is 0.  Every flush gives the slots it writes, and the slots that become live, p_max (the largest priority
 * assigned so far, 1 before any update) and zeroes the slots that stop being live.  Every call below flushes first.
 * enable: allocate the tree (once per replay) and start every live slot at p_max = 1; priorities are then
 * (|delta| + eps)^alpha.  Replays that never call it are unchanged. */
int oprl_replay_prio_enable(oprl_replay* h, double alpha, double eps, void* stream);
/* B rows drawn with probability proportional to priority, stratified over B equal segments of the root's mass and
 * keyed by (seed, counter): s, a, r, d, s2 as oprl_replay_sample writes them, the slots e·L + t in out_slot[B] (int32)
 * and the importance weights (N·p_j / total)^-beta over their batch maximum in out_w[B].  The arithmetic of the draw is
 * DESIGN.md §11's; a tree whose root is 0 gives slot -1 and weight 0. */
int oprl_replay_prio_sample(oprl_replay* h, int32_t B, uint64_t seed, uint64_t counter, double beta, float* out_s,
                            float* out_a, float* out_r, float* out_d, float* out_s2, int32_t* out_slot, float* out_w,
                            void* stream);
/* New priorities of the B slots slot[B] (int32, device) from td_abs[B] (device): (max(td_abs, 0) + eps)^alpha; a slot
 * listed more than once takes the row with the largest index; p_max = max(p_max, the new priorities); slots that are no
 * longer live stay 0. */
int oprl_replay_prio_update(oprl_replay* h, int32_t B, const int32_t* slot, const float* td_abs, void* stream);
/* Checkpoints and tests: the whole tree (every level, leaves first; layout in DESIGN.md §11) into tree_out[0 .. n)
 * (device; NULL: none), its size in floats into *n_floats_host, p_max into *p_max_host (which synchronises `stream`);
 * either host pointer may be NULL. */
int oprl_replay_prio_read(oprl_replay* h, float* tree_out, int64_t n, int64_t* n_floats_host, float* p_max_host,
                          void* stream);
/* Restore leaves[E·L] (device; the entries of dead slots are taken as 0) and p_max (> 0); the nodes are rebuilt. */
int oprl_replay_prio_load(oprl_replay* h, const float* leaves, float p_max, void* stream);

/* ---- D4PG's categorical critic seed, stand-alone ---------------------------------------------------
 * k_c51_critic_seed (csrc/c51_seed.hip) on caller-supplied device rows, as the learner's critic step runs it: target
 * logits zt[B][ld] and online logits z[B][ld] over N atoms from v_min to v_max, r[B], d[B].  Out: seed[B][ld] =
 * (softmax(z) - m) / B with the pad columns N .. ld - 1 written as zero, m[B][ld] the target distribution projected onto
 * the atoms (Tz_i = clamp(r + ((1 - d) gamma) z_i, v_min, v_max); pad columns zero) and loss[B] = -sum_j m_j log
 * softmax(z)_j; m_out and loss_out may be NULL.  Nothing is written for rows >= B.  OPRL_ERR_INVALID: a null pointer,
 * N outside 2 .. 48, ld outside N .. 64, B < 1, v_max <= v_min.  Tests reach the kernel's corners through it. */
int oprl_c51_seed(const float* zt, const float* z, const float* r, const float* d, double gamma, double v_min,
                  double v_max, int32_t N, int32_t B, int32_t ld, float* seed_out, float* m_out, float* loss_out,
                  void* stream);

/* ---- training from prioritized replay ("Training from it") -----------------------------------------
 * One reference-semantics update whose critic loss is (1/B) sum_b w[b] (Q(s,a) - y)^2 per critic, w[B] on the device;
 * the actor and temperature losses are not weighted (Schaul et al.).  td_abs_out[B] (device) receives
 * (sum_j |Q_j(s,a) - y|) / n_critics.  With w = 1 everywhere the update is oprl_learner_update's on a no_fuse learner,
 * bit for bit.  The critic step runs the generic launch sequence as forward | k_td_weighted_seed | backward, so:
 * OPRL_ERR_STATE for a learner whose fused form is on (create it with no_fuse), for export_grads / data-parallel
 * learners and members of a group; OPRL_ERR_INVALID for TQC (its quantile-Huber seed takes no per-row weight yet), for
 * D4PG (its cross-entropy seed takes none either) and for a precision other than OPRL_PREC_F32.  A refused call changes nothing. */
int oprl_learner_update_weighted(oprl_learner* h, const float* s, const float* a, const float* r, const float* d,
                                 const float* s2, const float* w, int32_t B, const float* noise0, const float* noise1,
                                 float* td_abs_out, void* stream);
/* K times, with u the learner's update count before each update: oprl_replay_prio_sample(seed, counter = u,
 * beta = min(1, beta0 + (1 - beta0) u / beta_steps), formed in double), oprl_learner_update_weighted on those rows
 * and weights, oprl_replay_prio_update(the rows' slots, its td_abs).  Everything is enqueued on `stream`; the host
 * waits for nothing.  Refused like update_weighted, and: a replay without a sum tree or an empty one
 * (OPRL_ERR_STATE), dims that are not the learner's, K < 0, B outside [1, max_batch], beta0 outside [0, 1] or
 * beta_steps <= 0 (OPRL_ERR_INVALID). */
int oprl_learner_step_n_prio(oprl_learner* h, oprl_replay* replay, int32_t K, int32_t B, uint64_t seed, double beta0,
                             double beta_steps, void* stream);

/* ---- TD3 + BC: a behaviour-cloning term in a TD3 learner's actor loss (Fujimoto & Gu 2021) ----------
 * A MODE of a TD3 learner, not an algorithm of its own: with alpha > 0 every later actor step minimises
 *   -lambda (1/B) sum_b Q1(s_b, pi(s_b)) + (1/(B A)) sum_{b,k} (pi(s_b)_k - a_bk)^2,  lambda = alpha / ((1/B) sum_b |Q1(s_b, pi(s_b))|),
 * lambda a constant for the gradient and with NO epsilon in its denominator (the authors' code has none); a is the
 * minibatch's action.  The critic step, the target smoothing noise, policy_freq and the Polyak steps are TD3's, through
 * every entry point (update, update_weighted, step_n, step_n_prio).  alpha = 0 turns the mode off: TD3 again, bit for
 * bit.  The first call with alpha > 0 allocates the mode's rows; no update allocates.  The actor step runs the generic
 * launch sequence as actor forward | critic 0 forward | k_bc_seed | critic 0 backward (SEED_PTR) | k_bc_mix | actor
 * backward | dW + Adam + Polyak (csrc/bc_seed.hip), so: OPRL_ERR_INVALID for any algorithm but TD3 (DDPG shares the
 * branch: a follow-up), for a precision other than OPRL_PREC_F32, for a negative or non-finite alpha; OPRL_ERR_STATE for
 * a learner whose fused form is on (create it with no_fuse), for export_grads / data-parallel learners and members of a
 * group; oprl_group_create refuses a learner with the mode on.  A refused call changes nothing. */
int oprl_learner_set_bc(oprl_learner* h, double alpha);
/* Of the last actor step with the mode on: out_host[0] = lambda, [1] = (1/B) sum_b |Q1(s_b, pi(s_b))|, [2] =
 * (1/(B A)) sum (pi - a)^2 (k_bc_mix's partial sums added in slice order), [3] = 0 (spare).  Synchronises `stream`.
 * OPRL_ERR_STATE for a learner on which the mode was never on. */
int oprl_learner_read_bc(oprl_learner* h, float out_host[4], void* stream);
/* k_bc_seed and k_bc_mix on caller-supplied device rows, as the learner's actor step runs them: q[B], pi[B][A], a[B][A],
 * da[B][A] (in / out: da += (2 / (B A)) (pi - a)).  Out: seed_out[B] = -lambda / B; scal_out[0] = lambda, [1] = mean |q|
 * ([2], [3] are left alone); part_q_out[(B + 15) / 16][4] = (0, sum q, 0, untouched) per slice of 16 rows;
 * part_sq_out[(B A + 15) / 16] = the sums of (pi - a)^2 over 16 adjacent elements.  Nothing is written past those
 * extents.  OPRL_ERR_INVALID: a null pointer, B < 1, A < 1, B A > 2^30, alpha not finite or <= 0.  Tests reach the
 * kernels' corners through it. */
int oprl_bc_seed(const float* q, const float* pi, const float* a, float* da, double alpha, int32_t B, int32_t A,
                 float* seed_out, float* scal_out, float* part_q_out, float* part_sq_out, void* stream);

/* ---- Implicit Q-learning: an expectile value net and an advantage-weighted actor (Kostrikov et al. 2021)
 * A MODE of a TD3 learner, like the one above: a non-null `value` turns it on, NULL turns it off (TD3 again, bit for
 * bit).  `value` is a caller-owned net V(s) with dims [state_dim, ..., 1]: theta, Adam moments and fragment pack, no
 * target, no gradient arena.  With qt = min_j Qtarget_j(s, a) on the minibatch's own action, u = qt - V(s) and V(s')
 * both taken with V as it is BEFORE this update's V step, one update is
 *   V:       one Adam step (lr_value, its own step count) on (1/B) sum_b omega_b u_b^2, omega_b = 1 - expectile where
 *            u_b < 0 and expectile otherwise; V has no target net and takes no Polyak step;
 *   critics: TD3's step with y = r + ((1 - d) gamma) V(s'): no target actor, no smoothing noise;
 *   actor:   one Adam step on (1/B) sum_b w_b sum_k (pi(s_b)_k - a_bk)^2, w_b = min(exp(beta u_b), adv_clip) a constant;
 *   Polyak on the critic targets (and the actor's, which nothing reads), every update.
 * No action outside the minibatch is evaluated.  The call that turns the mode on allocates its rows (once per shape of
 * V); no update allocates.  oprl_learner_sync_params rebuilds V's pack too while the mode is on.  12 launches per update
 * on the generic launch sequence (csrc/iql_seed.hip holds the two new kernels), so: OPRL_ERR_INVALID for any algorithm but
 * TD3, a precision other than OPRL_PREC_F32, policy_freq != 1, expectile outside (0, 1), beta < 0, adv_clip <= 0, lr_value
 * <= 0, any of them non-finite, a value net whose dims[0] is not state_dim or whose output is not 1, whose layer count or
 * width the generic path does not take, or without moments or pack; OPRL_ERR_STATE for a learner whose fused form is on
 * (create it with no_fuse), for export_grads / data-parallel learners, members of a group and a learner with the
 * behaviour-cloning mode on.  With the mode on, oprl_learner_set_bc, oprl_group_create, oprl_learner_update_weighted and
 * oprl_learner_step_n_prio return OPRL_ERR_STATE.  A refused call changes nothing. */
int oprl_learner_set_iql(oprl_learner* h, const oprl_net* value, double expectile, double beta, double adv_clip,
                         double lr_value);
/* Of the last update with the mode on, the per-slice sums added in slice order: out_host[0] = the V loss, [1] = mean
 * V(s), [2] = mean u, [3] = mean w, [4] = the share of rows at the clip, [5] = the weighted cloning loss (what
 * oprl_learner_read_scalars reports as the actor loss in this mode), [6] = [7] = 0 (spares).  Synchronises `stream`.
 * OPRL_ERR_STATE for a learner on which the mode was never on. */
int oprl_learner_read_iql(oprl_learner* h, float out_host[8], void* stream);
/* V's Adam step count (oprl_learner_get_counters / set_counters carry their four numbers unchanged). */
int oprl_learner_get_iql_step(oprl_learner* h, int64_t* out_host);
int oprl_learner_set_iql_step(oprl_learner* h, int64_t step);
/* k_iql_value_seed and k_iql_actor_seed on caller-supplied device rows, as the learner's update runs them: q1[B], q2[B]
 * (the target critics), v[B], pi[B][A], a[B][A].  Out: u_out[B] = min(q1, q2) - v; seed_out[B] = ((2 (v - qt)) (1/B))
 * omega; w_out[B] = min(exp(beta u), adv_clip); da_out[B][A] = (2/B) w (pi - a); per slice of 16 rows, n = (B + 15) / 16:
 * part_v_out[n][4] = (sum omega u^2, sum v, sum u, untouched), part_w_out[n][4] = (0, sum w, rows at the clip,
 * untouched), part_a_out[n][4] = (0, sum_b w_b sum_k (pi - a)^2, 0, untouched).  Nothing is written past those extents.
 * OPRL_ERR_INVALID: a null pointer, B < 1, A < 1, B A > 2^30, expectile outside (0, 1), beta < 0, adv_clip <= 0 or any of
 * them non-finite.  Tests reach the kernels' corners through it. */
int oprl_iql_seed(const float* q1, const float* q2, const float* v, const float* pi, const float* a, double expectile,
                  double beta, double adv_clip, int32_t B, int32_t A, float* u_out, float* seed_out, float* w_out,
                  float* da_out, float* part_v_out, float* part_w_out, float* part_a_out, void* stream);

/* ---- Conservative Q-learning: a penalty on the critics' values of actions outside the dataset (Kumar et al. 2020, CQL(H)
 * with a fixed penalty weight).  A MODE of a SAC learner, like the two above: n_actions = N in 1 .. 16 turns
 * it on, 0 turns it off (SAC again, bit for bit).  With the mode on the critic step of an update on B rows runs on
 * Bw = B (1 + 3 N) rows: the minibatch's (s, a) and, per state s_b, N actions uniform in [-1, 1]^A (log-density -A log 2),
 * N drawn from pi(.|s_b) and N from pi(.|s'_b) with their log-probabilities — the tanh-Gaussian head's formula, from ONE
 * forward of the online actor on s and one on s' — all evaluated at s_b and all constants for every gradient.  Per critic j,
 * with c_jbe = Q_j(s_b, x_be) - logdensity(x_be) over the row's 3 N entries, the loss is
 *   (1/B) sum_b (Q_j(s_b, a_b) - y_b)^2 + cql_alpha (1/B) sum_b [ logsumexp_e c_jbe - Q_j(s_b, a_b) ]
 * with SAC's target y (so an n-step replay gives n-step CQL); the critics are summed as SAC sums them and take one Adam step.
 * The actor step, the temperature step and Polyak are SAC's.  The call that turns the mode on allocates its rows (once);
 * no update allocates.  Noise: Philox streams 4 (normal) and 5 (uniform) of the learner's seed, counter = the update count.
 * OPRL_ERR_INVALID: a learner that is not SAC, a precision other than OPRL_PREC_F32, cql_alpha < 0 or non-finite, n_actions
 * outside 0 .. 16.  OPRL_ERR_STATE: a learner whose fused form is on (create it with no_fuse), a member of a group, an
 * export_grads / data-parallel learner.  The workspace holds max_batch rows — oprl_learner_create sets no ceiling on it —
 * so with the mode on oprl_learner_update / update_phase / step_n return OPRL_ERR_INVALID for B (1 + 3 N) > max_batch, and
 * oprl_learner_update_weighted and oprl_learner_step_n_prio return OPRL_ERR_STATE.  A refused call changes nothing. */
int oprl_learner_set_cql(oprl_learner* h, double cql_alpha, int32_t n_actions);
/* Of the last update with the mode on, the per-slice sums added in slice order, as means: out_host[0], [1] = mean_b
 * (logsumexp_e c_jbe - Q_j(s_b, a_b)) of critic 0, 1; [2], [3] = their mean Q on the uniform actions; [4], [5] = on the actions
 * drawn from pi(.|s_b); [6] = cql_alpha ([0] + [1]), the penalty term of the summed loss; [7] = after a calibrated update
 * (oprl_learner_set_calql) the share of the policy entries at the bound, sum_j #{(b, e >= N) : q_jbe < g_b} / (nc B 2N), else
 * 0.  Synchronises `stream`.
 * OPRL_ERR_STATE for a learner on which the mode was never on. */
int oprl_learner_read_cql(oprl_learner* h, float out_host[8], void* stream);
/* Test hook, like noise0 / noise1 of oprl_learner_update: device arrays standing in for the mode's draws, read by every
 * later update until replaced — eps[B][2N][A] N(0,1) draws ([b][k] for pi(.|s_b), [b][N + k] for pi(.|s'_b)), uni[B][N][A]
 * the uniform actions themselves (clamped to [-1, 1]).  NULL: Philox. */
int oprl_learner_set_cql_noise(oprl_learner* h, const float* eps, const float* uni);
/* k_cql_rows on caller-supplied device rows, as the learner's update runs it: s[B][S], a[B][A], the actor's raw head rows
 * raw_s[B][2A], raw_s2[B][2A] (means | log-stds), eps / uni as above (NULL: Philox streams 4 / 5 of `seed`, rank 0, at
 * `counter`).  Out, Bw = B (1 + 3 N) rows: ws_out[Bw][S], wa_out[Bw][A] — row b < B is (s_b, a_b); row B + b 3N + e,
 * e = kind N + k, is (s_b, x) with kind 0 uniform, 1 from pi(.|s_b), 2 from pi(.|s'_b) — and logd_out[B][3N].  Nothing is
 * written past those extents.  OPRL_ERR_INVALID: a null pointer (eps, uni excepted), B, S, A < 1, N outside 1 .. 16,
 * B (1 + 3 N) max(S, A) > 2^30. */
int oprl_cql_rows(const float* s, const float* a, const float* raw_s, const float* raw_s2, const float* eps, const float* uni,
                  uint64_t seed, uint64_t counter, int32_t B, int32_t S, int32_t A, int32_t N, float* ws_out, float* wa_out,
                  float* logd_out, void* stream);
/* k_cql_seed on caller-supplied device rows: q[nc][Bw] the critics on the wide rows, the target's operands qn1[B], qn2[B]
 * (or NULL), logp2[B] (or NULL; then alpha is unused), r[B], d[B] — y = r + ((1 - d) gamma) (min(qn1, qn2) - alpha logp2)
 * as SEED_MSE_TD forms it — and logd[B][3N].  Out: seed_out[nc][Bw] — data row b: ((2 (q - y)) - cql_alpha) (1/B); sampled
 * row (b, e): (cql_alpha softmax(c_jb.)_e) (1/B), a max-subtracted softmax in entry order — y_out[B] (or NULL), and per
 * slice of 16 rows, n = (B + 15) / 16: part_out[nc][n][4] = (sum (q - y)^2, sum q, sum y, untouched),
 * part_cql_out[nc][n][4] = (sum (logsumexp - q), sum_b sum_k q on the uniform actions, ... on pi(.|s_b)'s, untouched).
 * Nothing is written past those extents.  OPRL_ERR_INVALID: a null pointer, nc outside 1 .. OPRL_MAX_CRITICS, B < 1, N
 * outside 1 .. 16, B (1 + 3 N) > 2^30, cql_alpha < 0 or non-finite. */
int oprl_cql_seed(const float* q, const float* qn1, const float* qn2, const float* logp2, const float* r, const float* d,
                  const float* logd, double alpha, double gamma, double cql_alpha, int32_t nc, int32_t B, int32_t N,
                  float* seed_out, float* y_out, float* part_out, float* part_cql_out, void* stream);
/* The calibrated kernel on the same rows: oprl_cql_seed's arguments and g[B] (before `stream`, which stays last), the rows'
 * returns-to-go.  At the policy entries e in [N, 3N) of row b — the actions from pi(.|s_b) and pi(.|s'_b); the uniform ones are
 * not bounded — c_e = max(q_e, g_b) - logd_e, and seed(b, e) = (cql_alpha softmax(c)_e) (1/B) if q_e >= g_b, else 0 (written).
 * Everything else is formed as oprl_cql_seed forms it, from c; the sums of q are sums of the critics' own q.  Slot 3 of
 * part_cql_out takes the slice's count of bounded entries, #{e >= N : q_e < g_b}.  g = -inf everywhere gives oprl_cql_seed's
 * outputs bit for bit (and counts 0).  OPRL_ERR_INVALID as oprl_cql_seed, and for a null g. */
int oprl_cql_seed_cal(const float* q, const float* qn1, const float* qn2, const float* logp2, const float* r, const float* d,
                      const float* logd, double alpha, double gamma, double cql_alpha, int32_t nc, int32_t B, int32_t N,
                      float* seed_out, float* y_out, float* part_out, float* part_cql_out, const float* g, void* stream);

/* ---- Calibrated Q-learning (Nakamoto et al. 2023, Cal-QL): the calibrated form of the mode above.  Inside the
 * conservative penalty the critics' values at the policy actions are bounded below by the rows' returns-to-go g
 * (oprl_replay_returns); the TD term, the actor step, the temperature step and Polyak do not change.  on != 0 needs the CQL
 * mode on (OPRL_ERR_STATE otherwise) and, the first time, allocates [max_batch] rows for step_n's slots and returns;
 * oprl_learner_set_cql(.., 0) turns this form off with the mode.  With it on: oprl_learner_step_n (and step_act /
 * step_act_rows through it) takes the sampler's slots, calls oprl_replay_returns with the learner's gamma and updates with
 * them, over a plain, an n-step, a prioritized and a prior-data replay alike — a hindsight replay is refused with
 * OPRL_ERR_STATE before anything is launched; oprl_learner_update / update_phase return OPRL_ERR_STATE (the rows carry no
 * returns); oprl_learner_update_weighted and oprl_learner_step_n_prio return OPRL_ERR_STATE as under the CQL mode.  A
 * refused call changes nothing. */
int oprl_learner_set_calql(oprl_learner* h, int32_t on);
/* oprl_learner_update with the rows' returns-to-go g[B]: the two-call path of the calibrated form.  OPRL_ERR_INVALID: a
 * null g; OPRL_ERR_STATE: the calibrated form is off. */
int oprl_learner_update_calql(oprl_learner* h, const float* s, const float* a, const float* r, const float* d, const float* s2,
                              const float* g, int32_t B, const float* noise0, const float* noise1, void* stream);

/* ---- LayerNorm critics (Ball et al. 2023, RLPD; Hiraoka et al. 2022, DroQ): Linear -> LayerNorm -> ReLU in
 * both hidden layers of every critic of a SAC or REDQ learner; the output layer stays plain.  Per hidden layer and row, over
 * the 256 columns: mu = mean z, var = mean (z - mu)^2 (biased, two passes), zh = (z - mu) / sqrt(var + eps),
 * x = relu(gamma zh + beta).  The four arrays are the CALLER's device arrays [n_critics][2 hidden layers][gamma | beta][256]
 * fp32 (gamma starts at 1, beta at 0; the target copy equal; m and v zero), outside the nets' arenas and packs, whose
 * layouts do not change.  They belong to the critic optimiser: every update steps them with lr_critic, the learner's betas
 * and eps and the step count of that update's critic dW launch, and the target copy takes its Polyak step when the
 * critics' targets do.  Target forwards read the target copy; the actor step propagates through LN and steps nothing.
 * Called once, before the first update.  OPRL_ERR_INVALID: an algorithm other than SAC / REDQ, a precision other than f32,
 * critics that are not three layers of hidden width 256 with one output, a null array, an eps that is not finite and
 * positive.  OPRL_ERR_STATE: the fused launch form is on (create the learner with no_fuse), a group member, export_grads /
 * data-parallel, the CQL mode on, a second call, a learner that has updated.  While the mode is on oprl_learner_set_cql /
 * set_calql, oprl_group_create, oprl_learner_update_weighted and oprl_learner_step_n_prio return OPRL_ERR_STATE.  A refused
 * call changes nothing. */
typedef struct oprl_layernorm {
  float* theta;             /* [n_critics][2][2][256] gamma | beta per hidden layer */
  float* theta_target;      /* the target critics' copy */
  float* adam_m;            /* Adam's first and second moments */
  float* adam_v;
  float eps;                /* 1e-5f: torch's default */
} oprl_layernorm;
int oprl_learner_set_layernorm(oprl_learner* h, const oprl_layernorm* ln);
/* One packed three-layer net of hidden width 256 with LN parameters ln_theta [2][gamma | beta][256] on caller rows
 * [x0 | x1] (x1 may be null): forward, and — given the seed rows dout [B][n_out] — backward.  split = 0: one launch;
 * 1: a forward-only launch that keeps the rows, then a backward-only launch that reloads them (the same bits).  The row
 * arrays hold `rows` >= B rows per hidden layer, of which rows >= B are not touched: x_rows / dz_rows / zh_rows
 * [2][rows][256] (the layer's output, the gradient wrt its pre-normalisation z, the normalised z), rstd_rows [2][rows];
 * out [B][n_out]; dx1 [B][k1] (or null) the gradient wrt the x1 columns; dln [2][2][256] dgamma | dbeta summed over the
 * batch in slice order.  dout null: forward only (dz_rows, dx1, dln unused).  With dout the call allocates its per-slice sums,
 * SYNCHRONISES the stream and frees them before it returns.  OPRL_ERR_INVALID: null arguments, a net that is not three layers
 * of hidden width 256, B < 1, rows < B or rows > 2^22, k0 + k1 != the net's input dim, an eps that is not finite and positive.
 * The kernel tests' entry point. */
int oprl_mlp_ln(const oprl_net* net, const float* ln_theta, float eps, const float* x0, int32_t k0, const float* x1, int32_t k1,
                int32_t B, int32_t rows, int32_t split, const float* dout, float* out, float* x_rows, float* dz_rows,
                float* zh_rows, float* rstd_rows, float* dx1, float* dln, void* stream);

/* ---- Dropout in the LayerNorm critics (Hiraoka et al. 2022, DroQ): Linear -> Dropout -> LayerNorm -> ReLU.
 * Per hidden layer l in {0, 1}, batch row b and column c: zd = keep(b, l, c) ? z scale : 0 with scale = 1.0f / (1.0f - rate)
 * in float32, and the LayerNorm above is taken of zd; backward, dL/dz = keep ? dL/dzd scale : 0.  The mask is
 *   keep = philox4x32_10(ctr = (lo32 T, hi32 T, b, l 64 + c / 4), key = (lo32 K, hi32 K))[c % 4] >= (uint32)((double)rate 2^32)
 * with K the learner's noise key of stream 6 and T = (u 4 + k) 16 + j: u the learner's update count before the update (the
 * counter of oprl_redq_subset), k the pass (0: target critics on (s', a'); 1: the critic step on (s, a); 2: the actor phase's
 * critics on (s, pi)), j the critic's index.  Dropout runs in every pass that evaluates a critic; nothing of the mask is
 * stored (a backward regenerates it), and a checkpoint needs nothing beyond the update count.
 * Called once, after oprl_learner_set_layernorm and before the first update.  rate 0, or a rate so small that its
 * threshold (uint32)(rate 2^32) is 0, leaves the mode off and is no error (it does not count as the one call).
 * OPRL_ERR_INVALID: a null handle; a rate that is NaN, negative or >= 1.  OPRL_ERR_STATE: the LN mode is off, a second
 * call, a learner that has updated.  Everything the LN mode refuses stays refused.  A refused call changes nothing. */
int oprl_learner_set_dropout(oprl_learner* h, float rate);
/* oprl_mlp_ln with that dropout at `rate` from the Philox key `key` and the stream `stream_id` (the T above; all 64 bits
 * count), b the row's index in the batch.  split = 1: the backward-only launch regenerates the forward launch's mask (the
 * same bits as split = 0).  rate 0 is oprl_mlp_ln.  OPRL_ERR_INVALID beyond oprl_mlp_ln's: a rate that is NaN, negative or
 * >= 1.  The kernel tests' entry point. */
int oprl_mlp_ln_drop(const oprl_net* net, const float* ln_theta, float eps, const float* x0, int32_t k0, const float* x1, int32_t k1,
                     int32_t B, int32_t rows, int32_t split, const float* dout, float* out, float* x_rows, float* dz_rows,
                     float* zh_rows, float* rstd_rows, float* dx1, float* dln, void* stream, float rate, uint64_t key,
                     uint64_t stream_id);

#ifdef __cplusplus
}
#endif
#endif /* OPRL_AMD_H */
