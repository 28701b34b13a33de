// The policy call for MANY environments per launch: N <= 256 observation rows through the actor, as one
// launch that — like the single row of policy_act.hip — may be enqueued BEHIND the updates of the same C call
// (oprl_learner_step_act_rows) and talks to the host through host-mapped pinned memory: observations are read from
// there, the raw output rows are written there as {ticket, value} granules; no copies, no stream synchronise.
//
// k_policy_act_rows: one workgroup per tile of 16 rows, no waits between workgroups.  A tile goes through all layers with
// its activations in LDS; every product is v_mfma_f32_16x16x4_f32 (exact fp32, bitwise an fmaf chain) with the A operand
// from the LDS tile and the B operand straight from the row-major MASTER weights — no packs, so the result is the fp32
// evaluation of the masters in every precision mode and no learner needs a repack first.
//
// Operand mapping.  Lane l = 16 g + j feeds A[row j][k] and B[k][neuron n0 + j] with k = its k-group's index; which
// contraction index a lane carries is free as long as A and B agree, so in macro step q lane (g, j) takes the 16-byte
// run W[n0 + j][16 q + 4 g .. + 3] (one load instead of four strided dwords) and the same run of X[j] from LDS, and
// MFMA t of the step multiplies element t of both.  Output element (row i, neuron n) is therefore ONE chain in the fixed
// order q, t, g over row i's own activations — its bits do not depend on N, on the row's place in the batch or on its
// neighbours.  The accumulator of lane (g, j) holds rows 4 g .. 4 g + 3 of neuron n0 + j.
#include "policy_act_rows.h"

#include "learner_internal.h"

namespace oprl {

// LDS image of a tile: [16 rows][512], the 16-byte granule index XORed with the row — the 16 lanes of a k-group read the
// same columns of 16 different rows, which a plain 2 KB row stride would put into one bank group
__device__ __forceinline__ int rows_at(int i, int k) { return i * kActRowsWidth + ((((k >> 2) ^ i) << 2) | (k & 3)); }

__device__ __forceinline__ void rows_put(unsigned long long* p, unsigned ticket, float v) {
  // act_put's store (policy_act.hip): the value is its own flag
  __hip_atomic_store(p, ((unsigned long long)ticket << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}

// one 16-neuron tile of one layer: acc[r] = sum_k X[4 g + r][k] W[n][k] for this lane's neuron n.  kVec: rows of W are
// 16-byte aligned and K is a multiple of 4 (a run is whole or absent); otherwise four guarded dword loads.
template <bool kVec>
__device__ __forceinline__ f32x4 rows_tile(const float* x, const float* W, int K, int n, bool n_ok, int g, int j) {
  const float* wr = W + (size_t)(n_ok ? n : 0) * K;
  const int steps = (K + 15) >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // eight macro steps' weights are requested before the first is used (every load a trip to memory: the masters were
  // written by the update's tiles a moment ago); loads past the row's end go to a valid address and count as zeros
  for (int q0 = 0; q0 < steps; q0 += 8) {
    f32x4 b[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const int k = 16 * (q0 + d) + 4 * g;
      if (kVec) {
        const bool ok = n_ok && k < K;
        b[d] = ld4(ok ? wr + k : W);
        if (!ok) b[d] = f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const bool ok = n_ok && k + t < K;
          const float v = ok ? wr[k + t] : W[0];
          b[d][t] = ok ? v : 0.f;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      if (q0 + d < steps) {                 // (uniform; columns past the last step of the LDS tile are not zeros)
        const f32x4 a = ld4(x + rows_at(j, 16 * (q0 + d) + 4 * g));
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = mfma4(a[t], b[d][t], acc);
      }
    }
  }
  return acc;
}

__global__ __launch_bounds__(1024) void k_policy_act_rows(const PolicyActRowsArgs A) {
  __shared__ float xs[2][kActRowsTile * kActRowsWidth];      // 64 KB: the tile's activations, two layers
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15;
  const int row0 = blockIdx.x * kActRowsTile;
  const int live = A.n_rows - row0 < kActRowsTile ? A.n_rows - row0 : kActRowsTile;
  {
    // dead rows and the columns up to the next multiple of 16 are zeros (0 x garbage could be NaN)
    const int K0 = A.dims[0], K0p = (K0 + 15) & ~15;
    for (int e = tid; e < kActRowsTile * K0p; e += 1024) {
      const int i = e / K0p, k = e - i * K0p;
      xs[0][rows_at(i, k)] = (i < live && k < K0) ? A.obs[(size_t)(row0 + i) * K0 + k] : 0.f;
    }
  }
  __syncthreads();
  int cur = 0;
  for (int l = 0; l < A.n_layers; ++l) {
    const int K = A.dims[l], N = A.dims[l + 1];
    const float* W = A.w[l];
    const float* bias = A.b[l];
    const bool last = l == A.n_layers - 1;
    const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    const int tiles = (N + 15) >> 4;
    for (int tile = wave; tile < tiles; tile += 16) {
      const int n = 16 * tile + j;
      const bool n_ok = n < N;
      const f32x4 acc = vec ? rows_tile<true>(xs[cur], W, K, n, n_ok, g, j) : rows_tile<false>(xs[cur], W, K, n, n_ok, g, j);
      const float bv = n_ok ? bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * g + r;
        const float y = acc[r] + bv;
        if (last) {
          if (n_ok && i < live) rows_put(A.out + (size_t)(row0 + i) * N + n, A.ticket_value, y);   // raw row: the caller applies the head
        } else {
          xs[cur ^ 1][rows_at(i, n)] = (n_ok && y > 0.f) ? y : 0.f;      // (neurons past N: zeros up to the next multiple of 16)
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

hipError_t launch_policy_act_rows(const PolicyActRowsArgs& a, hipStream_t st) {
  const int grid = (a.n_rows + kActRowsTile - 1) / kActRowsTile;
  hipLaunchKernelGGL(k_policy_act_rows, dim3(grid), dim3(1024), 0, st, a);
  return hipGetLastError();
}

}  // namespace oprl

// ===================================================================== host side
namespace {

int rows_check_net(const oprl_net& n, const char* who) {
  if (n.n_layers < 1 || n.n_layers > kMaxLayers) { set_err("%s: n_layers=%d unsupported (1..%d)", who, n.n_layers, kMaxLayers); return OPRL_ERR_INVALID; }
  for (int l = 0; l <= n.n_layers; ++l)
    if (n.dims[l] < 1 || n.dims[l] > kActRowsWidth) { set_err("%s: layer width %d outside 1..%d", who, n.dims[l], kActRowsWidth); return OPRL_ERR_INVALID; }
  if (!n.theta) { set_err("%s: theta is null", who); return OPRL_ERR_INVALID; }
  return OPRL_OK;
}

int rows_check_n(int n_rows, const char* who) {
  if (n_rows < 1 || n_rows > kActRowsMax) { set_err("%s: n_rows %d outside 1..%d", who, n_rows, kActRowsMax); return OPRL_ERR_INVALID; }
  return OPRL_OK;
}

// a pinned, host-mapped area [obs: rows x S floats | out: rows x n_out granules] (the granules 8-byte aligned)
size_t rows_obs_floats(int rows, int S) { return ((size_t)rows * S + 1) & ~(size_t)1; }
size_t rows_area_bytes(int rows, int S, int n_out) { return rows_obs_floats(rows, S) * sizeof(float) + (size_t)rows * n_out * 8; }

int rows_enqueue(const oprl_net& n, float* pin, float* map, unsigned ticket, const float* obs_host, int n_rows, int cap_rows, hipStream_t st) {
  const int S = n.dims[0];
  memcpy(pin, obs_host, sizeof(float) * (size_t)n_rows * S);
  PolicyActRowsArgs a;
  memset(&a, 0, sizeof a);
  a.n_layers = n.n_layers;
  for (int l = 0; l <= n.n_layers; ++l) a.dims[l] = n.dims[l];
  for (int l = 0; l < n.n_layers; ++l) { a.w[l] = n.theta + w_off(n, l); a.b[l] = n.theta + b_off(n, l); }
  a.obs = map;
  a.out = reinterpret_cast<unsigned long long*>(map + rows_obs_floats(cap_rows, S));
  a.n_rows = n_rows;
  a.ticket_value = ticket;
  HIPC(launch_policy_act_rows(a, st));
  return OPRL_OK;
}

// bounded spin on the tickets of n granules; the values into out_host
int rows_collect(const float* pin, int cap_rows, int S, unsigned ticket, float* out_host, long n, int64_t timeout_us, const char* who) {
  const unsigned long long* gr = reinterpret_cast<const unsigned long long*>(pin + rows_obs_floats(cap_rows, S));
  const auto t0 = std::chrono::steady_clock::now();
  long spins = 0;
  for (long i = 0; i < n; ++i) {
    unsigned long long x;
    while ((unsigned)((x = __atomic_load_n(gr + i, __ATOMIC_ACQUIRE)) >> 32) != ticket) {
      if ((++spins & 1023) == 0 &&
          std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_us) {
        set_err("%s: the policy rows did not arrive within %lld us", who, (long long)timeout_us);
        return OPRL_ERR_STATE;
      }
      __builtin_ia32_pause();
    }
    const unsigned bits = (unsigned)x;
    memcpy(out_host + i, &bits, 4);
  }
  return OPRL_OK;
}

// the learner's area: allocated by the first call that acts in rows, for OPRL_ACT_ROWS_MAX rows at the actor's dims
int rows_area(oprl_learner* h) {
  if (h->rows_pin != nullptr) return OPRL_OK;
  const oprl_net& n = h->cfg.actor;
  const size_t bytes = rows_area_bytes(kActRowsMax, n.dims[0], n.dims[n.n_layers]);
  float* pin = nullptr;
  HIPC(hipHostMalloc((void**)&pin, bytes, hipHostMallocMapped));
  if (hipHostGetDevicePointer((void**)&h->rows_map, pin, 0) != hipSuccess) {
    (void)hipHostFree(pin);
    set_err("oprl_learner_act_rows: hipHostGetDevicePointer failed");
    return OPRL_ERR_HIP;
  }
  memset(pin, 0, bytes);
  h->rows_pin = pin;
  return OPRL_OK;
}

int rows_launch(oprl_learner* h, const float* obs_host, int n_rows, void* stream) {
  unsigned ticket = h->rows_ticket + 1;
  if (ticket == 0) ticket = 1;
  RC(rows_enqueue(h->cfg.actor, h->rows_pin, h->rows_map, ticket, obs_host, n_rows, kActRowsMax, (hipStream_t)stream));
  h->rows_ticket = ticket;
  h->rows_pending = n_rows;
  return OPRL_OK;
}

struct RowsStage {
  std::mutex mu;
  float* pin = nullptr;
  float* map = nullptr;
  size_t bytes = 0;
  int layout[3] = {0, 0, 0};   // (rows, in, out) the area was last laid out for
  unsigned ticket = 0;
};
RowsStage g_rows;

}  // namespace

extern "C" int oprl_learner_act_rows(oprl_learner* h, const float* obs_host, int32_t n_rows, void* stream) {
  if (!h || !obs_host) { set_err("oprl_learner_act_rows: null argument"); return OPRL_ERR_INVALID; }
  RC(rows_check_n(n_rows, "oprl_learner_act_rows"));
  RC(rows_check_net(h->cfg.actor, "oprl_learner_act_rows"));
  RC(check_device_error(h));
  RC(rows_area(h));
  return rows_launch(h, obs_host, n_rows, stream);
}

extern "C" int oprl_learner_step_act_rows(oprl_learner* h, oprl_replay* replay, int32_t K, int32_t B, uint64_t seed,
                                          const float* obs_host, int32_t n_rows, void* stream) {
  if (!h || !replay || !obs_host) { set_err("oprl_learner_step_act_rows: null argument"); return OPRL_ERR_INVALID; }
  RC(rows_check_n(n_rows, "oprl_learner_step_act_rows"));
  RC(rows_check_net(h->cfg.actor, "oprl_learner_step_act_rows"));
  // everything step_n refuses without having run an update is refused here as well, before anything changes
  if (h->cfg.export_grads) { set_err("oprl_learner_step_act_rows: step_n is the single-GPU fused path; export_grads learners use update_phase/apply"); return OPRL_ERR_STATE; }
  RC(check_device_error(h));
  int nstep = 1;
  RC(RowStager::check("step_act_rows", h, replay, false, K, B, &nstep));
  RC(rows_area(h));
  RC(oprl_learner_step_n(h, replay, K, B, seed, stream));
  return rows_launch(h, obs_host, n_rows, stream);
}

extern "C" int oprl_learner_act_rows_wait(oprl_learner* h, float* out_host, int32_t n_rows, int32_t n_out, int64_t timeout_us) {
  if (!h || !out_host) { set_err("oprl_learner_act_rows_wait: null argument"); return OPRL_ERR_INVALID; }
  if (h->rows_pending == 0) { set_err("oprl_learner_act_rows_wait: no rows are pending (oprl_learner_act_rows / step_act_rows first)"); return OPRL_ERR_STATE; }
  if (n_rows != h->rows_pending) { set_err("oprl_learner_act_rows_wait: n_rows %d != the %d pending rows", n_rows, h->rows_pending); return OPRL_ERR_STATE; }
  const oprl_net& n = h->cfg.actor;
  if (n_out != n.dims[n.n_layers]) { set_err("oprl_learner_act_rows_wait: n_out %d != the actor's %d outputs", n_out, n.dims[n.n_layers]); return OPRL_ERR_INVALID; }
  RC(rows_collect(h->rows_pin, kActRowsMax, n.dims[0], h->rows_ticket, out_host, (long)n_rows * n_out, timeout_us, "oprl_learner_act_rows_wait"));
  h->rows_pending = 0;
  return OPRL_OK;
}

extern "C" int oprl_mlp_act_rows(const oprl_net* net, const float* obs_host, int32_t n_rows, int32_t k0, float* out_host,
                                 int32_t n_out, void* stream) {
  if (!net || !obs_host || !out_host) { set_err("oprl_mlp_act_rows: null argument"); return OPRL_ERR_INVALID; }
  RC(rows_check_n(n_rows, "oprl_mlp_act_rows"));
  RC(rows_check_net(*net, "oprl_mlp_act_rows"));
  if (k0 != net->dims[0] || n_out != net->dims[net->n_layers]) {
    set_err("oprl_mlp_act_rows: dims (%d in, %d out) do not match the net (%d in, %d out)", k0, n_out, net->dims[0], net->dims[net->n_layers]);
    return OPRL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(g_rows.mu);
  const size_t bytes = rows_area_bytes(n_rows, k0, n_out);
  if (bytes > g_rows.bytes) {      // (synchronous calls: nothing in flight reads the old area)
    if (g_rows.pin) (void)hipHostFree(g_rows.pin);
    g_rows.pin = g_rows.map = nullptr;
    g_rows.bytes = 0;
    const size_t cap = std::max(bytes, (size_t)1 << 16);
    HIPC(hipHostMalloc((void**)&g_rows.pin, cap, hipHostMallocMapped));
    HIPC(hipHostGetDevicePointer((void**)&g_rows.map, g_rows.pin, 0));
    memset(g_rows.pin, 0, cap);
    g_rows.bytes = cap;
  }
  if (g_rows.layout[0] != n_rows || g_rows.layout[1] != k0 || g_rows.layout[2] != n_out) {
    // another layout: what lies where the granules go now is no ticket of this stage
    memset(g_rows.pin, 0, g_rows.bytes);
    g_rows.layout[0] = n_rows; g_rows.layout[1] = k0; g_rows.layout[2] = n_out;
  }
  g_rows.ticket += 1;
  if (g_rows.ticket == 0) g_rows.ticket = 1;
  RC(rows_enqueue(*net, g_rows.pin, g_rows.map, g_rows.ticket, obs_host, n_rows, n_rows, st));
  return rows_collect(g_rows.pin, n_rows, k0, g_rows.ticket, out_host, (long)n_rows * n_out, 10'000'000, "oprl_mlp_act_rows");
}
