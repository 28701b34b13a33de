// ln_slice.h — layer normalisation inside the whole-MLP slice kernel (csrc/ln_slice.hip): what the host
// hands to k_mlp_slice_ln / k_mlp_slice_multi_ln beside a net's MlpArgs, and k_ln_adam's argument block.
//
// A critic MLP(S+A -> 256 -> 256 -> 1) with LN computes per hidden layer l and row, over the 256 columns,
//   z = W x + b;  mu = mean z;  var = mean (z - mu)^2  (two passes);  rstd = 1 / sqrt(var + eps);
//   zh = (z - mu) rstd;  n = gamma zh + beta;  x_l = relu(n)
// and backward from g = dL/dn (ReLU-masked)
//   dbeta += sum_b g;  dgamma += sum_b g zh;  gz = g gamma;  dz = rstd (gz - mean gz - zh mean(gz zh))
// dz is what the dW tiles read as dYg[l], x_l what they read as Xg[l + 1]: k_dw_adam does not change.
//
// Dropout (DroQ's Linear -> Dropout -> LayerNorm -> ReLU) sits between z and the row pass:
//   zd = keep(b, l, c) ? z scale : 0,  scale = 1 / (1 - rate) in float32;  the LayerNorm above is taken of zd,
//   and the backward's dz (now dL/dzd) becomes dL/dz = keep ? dz scale : 0 before it is written.
//   keep = philox4x32_10(ctr = (lo T, hi T, b, l 64 + c / 4), key = drop_key)[c % 4] >= drop_thresh
// b is the row's index in the batch.  Nothing of the mask is stored: a backward regenerates it from the same (key, T).
#pragma once
#include "kernels.h"

namespace oprl {

constexpr int kLnWidth = 256;     // the hidden width the LN kernels are built for
constexpr int kLnHidden = 2;      // hidden layers of a net with LN (three Linear layers)
constexpr int kLnNetFloats = kLnHidden * 2 * kLnWidth;   // one net's parameters: [layer][gamma | beta][256]

// One net of one launch.  MlpArgs::reserved of a launch that goes to the LN kernels points at one of these on the HOST
// (net_rounds.hip); the launchers pass it to the kernels by value.
struct LnView {
  const float* gb;                // this net's [2][gamma | beta][256]: the online parameters, or the target copy
  float* zh[kLnHidden];           // [B][256] zh rows of hidden layer l: a storing forward writes them, a backward-only
  float* rstd[kLnHidden];         //   launch reads them (and rstd [B]); null: nothing is kept
  float* sums;                    // [2][sum_slices][dgamma | dbeta][256] this launch's per-slice sums; null: none are
  int sum_slices;                 //   written (target nets, the actor phase's critic passes)
  float eps;
  unsigned long long drop_key;    // dropout: the Philox key, and the pass's stream T (a backward-only launch carries the
  unsigned long long drop_stream; //   T of the forward launch whose rows it reloads)
  uint32_t drop_thresh;           // (uint32)(rate 2^32): a word below it drops its column; 0: no dropout, no Philox call
  float drop_scale;               // 1 / (1 - rate)
};
static_assert(sizeof(LnView) == 80, "LnView's layout");

struct MlpMultiLnArgs { MlpArgs a[kMaxMulti]; LnView v[kMaxMulti]; };
static_assert(sizeof(MlpMultiLnArgs) <= 4096, "k_mlp_slice_multi_ln's argument block exceeds the 4 KB kernel-argument limit");

// k_ln_adam: one thread per (net, layer, gamma | beta, column) adds the per-slice sums in ascending slice order and takes
// the element's Adam (+ Polyak) step; gout (or null) receives the reduced gradient
struct LnAdamArgs {
  float *theta, *target, *m, *v;  // [n_nets][2][2][256] each; target null or ad.do_polyak 0: no Polyak step
  const float* sums;              // [n_nets][2][sum_slices][2][256]
  float* gout;
  int n_nets, n_slices, sum_slices;
  AdamScalars ad;                 // (the host knows the step: step_size_host / bc2_sqrt_host)
};

size_t mlp_slice_ln_lds_bytes();
hipError_t init_ln_attrs();       // the LN kernels' dynamic-LDS attribute on the current device (every learner create, oprl_mlp_ln)
hipError_t launch_mlp_slice_ln(const MlpArgs& a, const LnView& v, hipStream_t st);
hipError_t launch_mlp_slice_multi_ln(const MlpArgs* a, const LnView* v, int n, hipStream_t st);
hipError_t launch_ln_adam(const LnAdamArgs& a, hipStream_t st);

}  // namespace oprl
