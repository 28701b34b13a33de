// ln_slice.hip — the whole-MLP slice kernel with layer normalisation in the hidden layers.
//
//   k_mlp_slice_ln<256>        k_mlp_slice (kernels.hip) with Linear -> LayerNorm -> ReLU hidden layers: the same GEMMs
//                              (gemm_packed), head (slice_head), seeds (slice_seed) and input-gradient path; the hidden
//                              GEMMs' epilogue stores z, and a row pass follows each of them; with dropout
//                              the row pass first masks and scales z from one Philox call per lane, the backward row
//                              pass masks and scales dz from the same call
//   k_mlp_slice_multi_ln<256>  its grid (slices, nets <= kMaxMulti) form
//   k_ln_adam                  the per-slice dgamma / dbeta sums added in slice order + Adam + Polyak per element
//
// The row passes: a workgroup is 16 waves and a slice is 16 rows, so wave w owns row w; lane i holds the row's columns
// 4 i .. 4 i + 3 from one 16-byte LDS read (rows are lds_ld(256) = 264 floats apart: a wave's 64 reads are 1 KB in a
// row, conflict-free).  Mean, variance (two passes over the registers) and the backward's two means are wave reductions.
// The column sums of dgamma / dbeta cross the waves: they are read column-wise from the LDS tiles, rows in ascending order.
#include <cmath>
#include <cstring>
#include "ln_slice.h"
#include "philox.h"
#include "slice_head.h"

namespace oprl {

namespace {

// LDS map: SliceLds<256>'s (x0 | h[2] | out | aux | scr), then zh[2] [kR][WL] beside h, then rstd [2][kR]
struct LnLds {
  using LY = SliceLds<kLnWidth>;
  static constexpr int zh_off = LY::total(kLnHidden);
  static constexpr int rstd_off = zh_off + kLnHidden * LY::hbuf;
  static constexpr int total = rstd_off + kLnHidden * kR;
};
static_assert(LnLds::total * sizeof(float) <= 160 * 1024, "the LN slice kernel's LDS exceeds a compute unit's");
static_assert(LnLds::zh_off % 4 == 0, "16-byte alignment of the zh tiles");

// the sum over a wave's 64 lanes, in every lane: the DPP row sum, then the four rows
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// The dropout mask of this lane's four columns 4 lane .. 4 lane + 3 of batch row brow in hidden layer l, as bits 0 .. 3
// (set: kept).  One Philox call; it reads no memory, so the callers issue it in front of their LDS reads.
__device__ __forceinline__ uint32_t drop_keep4(const LnView& V, int l, int brow, int lane) {
  const u32x4 w = philox4x32_10(u32x4{(uint32_t)V.drop_stream, (uint32_t)(V.drop_stream >> 32), (uint32_t)brow, (uint32_t)(l * 64 + lane)},
                                (uint32_t)V.drop_key, (uint32_t)(V.drop_key >> 32));
  const uint32_t th = V.drop_thresh;
  return (w.x >= th ? 1u : 0u) | (w.y >= th ? 2u : 0u) | (w.z >= th ? 4u : 0u) | (w.w >= th ? 8u : 0u);
}

// Forward row pass over Hs [kR][WL] holding z: x = relu(gamma zh + beta) in place, zh to Zs, rstd to rs[row].
// With dropout (V.drop_thresh != 0, uniform over the launch's net) z becomes zd = keep ? z scale : 0 first.
// The caller has made z visible (barrier); the next GEMM's own barrier makes x visible.
__device__ __forceinline__ void ln_forward_rows(float* Hs, float* Zs, float* rs, const LnView& V, int l, int row0) {
  constexpr int WL = lds_ld(kLnWidth);
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
  const float* __restrict__ gb = V.gb + l * 2 * kLnWidth;
  const float eps = V.eps;
  const bool drop = __builtin_expect(V.drop_thresh != 0, 0);      // (off keeps the straight path)
  uint32_t keep = 0;
  if (drop) keep = drop_keep4(V, l, row0 + row, lane);
  const f32x4 gam = ld4(gb + 4 * lane), bet = ld4(gb + kLnWidth + 4 * lane);
  float* p = Hs + row * WL + 4 * lane;
  f32x4 z = ld4(p);
  if (drop) {
    const float scale = V.drop_scale;
#pragma unroll
    for (int t = 0; t < 4; ++t) z[t] = (keep >> t) & 1u ? z[t] * scale : 0.f;
  }
  const float mu = wave_sum((z[0] + z[1]) + (z[2] + z[3])) * (1.f / kLnWidth);
  const f32x4 d = z - mu;
  const float var = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.f / kLnWidth);
  const float rstd = 1.f / sqrtf(var + eps);
  const f32x4 zh = d * rstd;
  f32x4 x;
#pragma unroll
  for (int t = 0; t < 4; ++t) x[t] = fmaxf(__builtin_fmaf(gam[t], zh[t], bet[t]), 0.f);
  *reinterpret_cast<f32x4*>(p) = x;
  *reinterpret_cast<f32x4*>(Zs + row * WL + 4 * lane) = zh;
  if (lane == 0) rs[row] = rstd;
}

// Backward row pass over Gs [kR][WL] holding g = dL/dn (masked): dz in place.  Before that the slice's column sums over
// its `live` rows (< kR in the last slice of a ragged batch: rows >= B are never summed) go to sums [dgamma | dbeta][256].
// With dropout the dz written is dL/dz = keep ? dz scale : 0, the mask regenerated from the forward's (key, T).
// The caller has made g visible (barrier); contains the barrier between the column reads and the in-place writes.
__device__ __forceinline__ void ln_backward_rows(float* Gs, const float* Zs, const float* rs, const LnView& V, int l, int row0,
                                                 float* __restrict__ sums, int live) {
  constexpr int WL = lds_ld(kLnWidth);
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
  const float* __restrict__ gb = V.gb + l * 2 * kLnWidth;
  const bool drop = __builtin_expect(V.drop_thresh != 0, 0);      // (off keeps the straight path)
  uint32_t keep = 0;
  if (drop) keep = drop_keep4(V, l, row0 + row, lane);
  const f32x4 gam = ld4(gb + 4 * lane);
  float* p = Gs + row * WL + 4 * lane;
  const f32x4 g = ld4(p), zh = ld4(Zs + row * WL + 4 * lane);
  const float rstd = rs[row];
  if (sums != nullptr && threadIdx.x < 2 * kLnWidth) {
    const int c = threadIdx.x & (kLnWidth - 1);
    const bool is_gamma = threadIdx.x < kLnWidth;
    float acc = 0.f;
    for (int r = 0; r < live; ++r) {
      const float gv = Gs[r * WL + c];
      acc = is_gamma ? __builtin_fmaf(gv, Zs[r * WL + c], acc) : acc + gv;
    }
    sums[threadIdx.x] = acc;
  }
  __syncthreads();
  const f32x4 gz = g * gam;
  const float m1 = wave_sum((gz[0] + gz[1]) + (gz[2] + gz[3])) * (1.f / kLnWidth);
  const float m2 = wave_sum((gz[0] * zh[0] + gz[1] * zh[1]) + (gz[2] * zh[2] + gz[3] * zh[3])) * (1.f / kLnWidth);
  f32x4 dz;
#pragma unroll
  for (int t = 0; t < 4; ++t) dz[t] = rstd * ((gz[t] - m1) - zh[t] * m2);
  if (drop) {
    const float scale = V.drop_scale;
#pragma unroll
    for (int t = 0; t < 4; ++t) dz[t] = (keep >> t) & 1u ? dz[t] * scale : 0.f;
  }
  *reinterpret_cast<f32x4*>(p) = dz;
}

// mlp_slice_body (kernels.hip) for a three-layer net of width 256 with LN in both hidden layers
__device__ __forceinline__ void mlp_slice_ln_body(const MlpArgs& A, const LnView& V) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  using LY = SliceLds<kLnWidth>;
  constexpr int WL = lds_ld(kLnWidth);
  constexpr int HB = LY::hbuf;
  constexpr int NTW = kLnWidth / 16;
  constexpr int L = kLnHidden + 1;
  const Net& net = A.net;
  const int Nout = net.dims[L];
  float* x0s = smem;
  float* hb = smem + LY::h_off;
  float* outS = smem + LY::out_off(kLnHidden);
  float* auxS = smem + LY::aux_off(kLnHidden);
  float* scr = smem + LY::scr_off(kLnHidden);
  float* zhS = smem + LnLds::zh_off;
  float* rstdS = smem + LnLds::rstd_off;
  const int row0 = blockIdx.x * kR;
  const int B = A.B;
  const int tid = threadIdx.x;

  if (A.do_fwd) {
    lds_zero(x0s, kR * kX0Ld);
    __syncthreads();
    load_rows(x0s, kX0Ld, 0, A.x0, A.k0, A.k0, row0, B);
    if (A.x1 != nullptr) load_rows(x0s, kX0Ld, A.k0, A.x1, A.k1, A.k1, row0, B);
    gemm_packed(x0s, kX0Ld, net.pf[0], NTW, cdiv(net.dims[0], 16), scr, net.b[0], kLnWidth,
                [&](int row, int col, float v) { hb[row * WL + col] = v; });
    __syncthreads();
    ln_forward_rows(hb, zhS, rstdS, V, 0, row0);
    gemm_packed(hb, WL, net.pf[1], NTW, NTW, scr, net.b[1], kLnWidth,
                [&](int row, int col, float v) { hb[HB + row * WL + col] = v; });
    __syncthreads();
    ln_forward_rows(hb + HB, zhS + HB, rstdS + kR, V, 1, row0);
    gemm_packed(hb + HB, WL, net.pf[2], cdiv(Nout, 16), NTW, scr, net.b[2], Nout,
                [&](int row, int col, float v) { outS[row * kOutLd + col] = col < Nout ? v : 0.f; });
    // (the narrow GEMM ended with a barrier: h, zh and rstd are complete)
    if (A.Xg[0] != nullptr) store_rows(x0s, kX0Ld, A.Xg[0], A.ldx0, net.dims[0], row0, B);
#pragma unroll
    for (int l = 0; l < kLnHidden; ++l) {
      if (A.Xg[l + 1] != nullptr) store_rows4(hb + l * HB, WL, A.Xg[l + 1], kLnWidth, kLnWidth, row0, B);
      if (V.zh[l] != nullptr) {
        store_rows4(zhS + l * HB, WL, V.zh[l], kLnWidth, kLnWidth, row0, B);
        if (tid < kR && row0 + tid < B) V.rstd[l][row0 + tid] = rstdS[l * kR + tid];
      }
    }
    slice_head(A, outS, Nout, row0, true);
  } else if (A.do_bwd) {
#pragma unroll
    for (int l = 0; l < kLnHidden; ++l) {
      load_rows4(hb + l * HB, WL, A.Xg[l + 1], kLnWidth, kLnWidth, row0, B);
      load_rows4(zhS + l * HB, WL, V.zh[l], kLnWidth, kLnWidth, row0, B);
      if (tid < kR) rstdS[l * kR + tid] = row0 + tid < B ? V.rstd[l][row0 + tid] : 0.f;
    }
  }
  if (!A.do_bwd) return;

  slice_seed(A, outS, auxS, scr, Nout, L, row0, blockIdx.x, true);
  const int live = min(kR, B - row0);
  const float* dy = auxS;
  int ldy = kOutLd, ns = cdiv(Nout, 16);
#pragma unroll
  for (int l = kLnHidden; l >= 1; --l) {
    float* dx = hb + (l - 1) * HB;     // holds x (the ReLU mask) now, g and then dz afterwards
    gemm_packed(dy, ldy, net.pb[l], NTW, ns, scr, nullptr, 0, [&](int row, int col, float v) {
      float* p = dx + row * WL + col;
      *p = *p > 0.f ? v : 0.f;
    });
    __syncthreads();
    float* sums = V.sums != nullptr ? V.sums + ((size_t)(l - 1) * V.sum_slices + blockIdx.x) * (2 * kLnWidth) : nullptr;
    ln_backward_rows(dx, zhS + (l - 1) * HB, rstdS + (l - 1) * kR, V, l - 1, row0, sums, live);
    if (A.dYg[l - 1] != nullptr) {
      __syncthreads();
      store_rows4(dx, WL, A.dYg[l - 1], kLnWidth, kLnWidth, row0, B);
    }
    dy = dx;
    ldy = WL;
    ns = NTW;
  }
  if (A.dact_cols > 0) {
    const int dact_col0 = A.dact_col0, dact_cols = A.dact_cols;
    gemm_packed(dy, WL, net.pb[0], cdiv(net.dims[0], 16), NTW, scr, nullptr, 0, [&](int row, int col, float v) {
      const int c = col - dact_col0;
      if (c >= 0 && c < dact_cols) auxS[row * kOutLd + c] = v;
    });
    if (A.dact != nullptr) store_rows(auxS, kOutLd, A.dact, A.lddact, A.dact_cols, row0, B);
  }
}

}  // namespace

template <int WIDTH>
__global__ __launch_bounds__(kThreads) void k_mlp_slice_ln(const MlpArgs A, const LnView V) {
  static_assert(WIDTH == kLnWidth, "the LN slice kernels are built for width 256");
  mlp_slice_ln_body(A, V);
}

// grid (slices, nets): a workgroup addresses its own argument blocks through the kernarg segment pointer (scalar loads)
template <int WIDTH>
__global__ __launch_bounds__(kThreads) void k_mlp_slice_multi_ln(const MlpMultiLnArgs M) {
  static_assert(WIDTH == kLnWidth, "the LN slice kernels are built for width 256");
  const MlpMultiLnArgs* kp = (const MlpMultiLnArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  mlp_slice_ln_body(kp->a[blockIdx.y], kp->v[blockIdx.y]);
}

template __global__ void k_mlp_slice_ln<256>(const MlpArgs, const LnView);
template __global__ void k_mlp_slice_multi_ln<256>(const MlpMultiLnArgs);

__global__ __launch_bounds__(256) void k_ln_adam(const LnAdamArgs A) {
  const int e = blockIdx.x * 256 + threadIdx.x;              // (net, layer, gamma | beta, column)
  if (e >= A.n_nets * kLnNetFloats) return;
  const int net = e / kLnNetFloats, r = e - net * kLnNetFloats;
  const int l = r / (2 * kLnWidth), kc = r - l * (2 * kLnWidth);
  const float* sp = A.sums + ((size_t)(net * kLnHidden + l) * A.sum_slices) * (2 * kLnWidth) + kc;
  float g = 0.f;
  for (int s = 0; s < A.n_slices; ++s) g += sp[(size_t)s * (2 * kLnWidth)];
  float t0, t1;
  (void)adam_polyak_elem(g, A.theta + e, A.m + e, A.v + e, A.target != nullptr ? A.target + e : nullptr,
                         A.gout != nullptr ? A.gout + e : nullptr, A.ad, A.ad.step_size_host, A.ad.bc2_sqrt_host, &t0, &t1);
}

// ---------------------------------------------------------------------------
// host-visible launchers
// ---------------------------------------------------------------------------
size_t mlp_slice_ln_lds_bytes() { return sizeof(float) * LnLds::total; }

// the LN kernels' 97 920 B of dynamic LDS exceed the 64 KB default: per device, so on every oprl_learner_create (beside
// init_kernel_attrs) and in oprl_mlp_ln
hipError_t init_ln_attrs() {
  const void* ks[2] = {reinterpret_cast<const void*>(&k_mlp_slice_ln<256>), reinterpret_cast<const void*>(&k_mlp_slice_multi_ln<256>)};
  for (const void* k : ks) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// what the LN kernels are built for: three layers, 256 | 256 hidden, a narrow output; a backward-only launch needs the
// rows of a storing forward
static bool ln_launch_ok(const MlpArgs& a, const LnView& v) {
  const Net& n = a.net;
  if (n.n_layers != kLnHidden + 1 || n.dims[1] != kLnWidth || n.dims[2] != kLnWidth) return false;
  if (n.dims[0] < 1 || n.dims[0] > 96 || n.dims[3] < 1 || n.dims[3] > kNarrowMax) return false;
  if (a.B < 1 || v.gb == nullptr || a.tp_xbuf != nullptr) return false;
  if (a.do_fwd && a.k0 + (a.x1 != nullptr ? a.k1 : 0) != n.dims[0]) return false;
  if (a.dact_cols > 0 && (a.dact_cols > kNarrowMax || a.dact_col0 < 0 || a.dact_col0 + a.dact_cols > n.dims[0])) return false;
  if (v.sums != nullptr && v.sum_slices < (a.B + kR - 1) / kR) return false;
  for (int l = 0; l < kLnHidden; ++l) {
    if ((v.zh[l] == nullptr) != (v.rstd[l] == nullptr)) return false;
    if (!a.do_fwd && a.do_bwd && (v.zh[l] == nullptr || a.Xg[l + 1] == nullptr)) return false;
  }
  return a.do_fwd || a.do_bwd;
}

hipError_t launch_mlp_slice_ln(const MlpArgs& a, const LnView& v, hipStream_t st) {
  if (!ln_launch_ok(a, v)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mlp_slice_ln<256>, dim3((a.B + kR - 1) / kR), dim3(kThreads), mlp_slice_ln_lds_bytes(), st, a, v);
  return hipGetLastError();
}

// n <= kMaxMulti launches of equal batch as one
hipError_t launch_mlp_slice_multi_ln(const MlpArgs* a, const LnView* v, int n, hipStream_t st) {
  if (n < 1 || n > kMaxMulti) return hipErrorInvalidValue;
  for (int j = 0; j < n; ++j)
    if (!ln_launch_ok(a[j], v[j]) || a[j].B != a[0].B) return hipErrorInvalidValue;
  MlpMultiLnArgs m;
  for (int j = 0; j < kMaxMulti; ++j) { m.a[j] = a[j < n ? j : 0]; m.v[j] = v[j < n ? j : 0]; }
  const dim3 grid((a[0].B + kR - 1) / kR, n);
  hipLaunchKernelGGL(k_mlp_slice_multi_ln<256>, grid, dim3(kThreads), mlp_slice_ln_lds_bytes(), st, m);
  return hipGetLastError();
}

hipError_t launch_ln_adam(const LnAdamArgs& a, hipStream_t st) {
  if (a.n_nets < 1 || a.n_slices < 1 || a.n_slices > a.sum_slices || a.theta == nullptr || a.m == nullptr || a.v == nullptr ||
      a.sums == nullptr || a.ad.step_dev != nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ln_adam, dim3((a.n_nets * kLnNetFloats + 255) / 256), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace oprl
