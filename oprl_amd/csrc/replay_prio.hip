// replay_prio.hip — prioritized experience replay over the HBM replay (Schaul et al., ICLR 2016, proportional variant):
// a sum tree with one priority per slot (e, t), maintained, sampled and updated on the device.
//   k_prio_init     the leaves from the episode table (enable, checkpoint load)
//   k_prio_flush    the leaves of the rows and episodes one flush changed
//   k_prio_level    one level of internal nodes from their children (the flagged nodes, or all of them)
//   k_prio_sample   stratified descent, one wave per row; k_prio_weights the importance weights
//   k_prio_claim, k_prio_update   new priorities from |TD errors| (the largest batch index wins a slot listed twice)
// The rows themselves are gathered by k_replay_gather (oprl_replay_sample with the descent's flat indices).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "philox.h"
#include "replay_internal.h"

namespace {

constexpr int F = oprl::kPrioFan;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kSampleWord = 0x7e55u;  // the sampler's fourth Philox counter word (the uniform sampler's: replay_index.h kUniformWord)

__device__ __forceinline__ int ep_len(const int* ends, int e) { return ends[e] - (e > 0 ? ends[e - 1] : 0); }

// A node from its F children ch[0 .. F): lane l adds its four as (c0 + c1) + (c2 + c3), then the lanes fold by halves,
// v[l] = v[l] + v[l + h] for h = 32, 16, 8, 4, 2, 1; lane 0 ends with the node.  Every internal node is this function
// of its children, whichever kernel computes it.
__device__ __forceinline__ float node_sum(const float* ch, int lane) {
  const float4 c = reinterpret_cast<const float4*>(ch)[lane];
  float v = (c.x + c.y) + (c.z + c.w);
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) v += __shfl_down(v, h, 64);
  return v;
}

// leaf i = e·L + t: the loaded leaf src[i] (or pm when src is null) if the slot is live, else 0; the padding 0; lens[e]
// and *p_max as the tree's starting state
__global__ __launch_bounds__(kThreads) void k_prio_init(float* leaves, long n_pad, int* lens, float* p_max,
                                                       const int* ends, int n_eps, int E, int L, const float* src,
                                                       float pm) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_pad) return;
  float v = 0.f;
  if (i < (long)E * L) {
    const int e = (int)(i / L), t = (int)(i - (long)e * L);
    if (e < n_eps && t < ep_len(ends, e)) v = src != nullptr ? src[i] : pm;
  }
  leaves[i] = v;
  if (i < E) lens[i] = i < n_eps ? ep_len(ends, (int)i) : 0;
  if (i == 0) *p_max = pm;
}

struct FlushArgs {
  float* leaves;
  int* dirty1;                // the flags of level 1
  int* lens;
  const int* ends;
  const float* p_max;
  const float* rows;          // staged rows: [ep, t] as int bits, then the data
  int n_rows, rowlen, L, n_eps, ep_lo, row_blocks;
};

// Blocks [0, row_blocks): one staged row per thread.  The others: episode ep_lo + (block - row_blocks) each, whose
// leaves between its old and new length change.  A leaf both kinds write gets the same value from both: p_max if its
// slot is live under the new episode table, else 0.
__global__ __launch_bounds__(kThreads) void k_prio_flush(const FlushArgs a) {
  const float pm = *a.p_max;
  if ((int)blockIdx.x < a.row_blocks) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.n_rows) return;
    const float* row = a.rows + (size_t)r * a.rowlen;
    const int e = __float_as_int(row[0]), t = __float_as_int(row[1]);
    const int len = e < a.n_eps ? ep_len(a.ends, e) : 0;
    const long i = (long)e * a.L + t;
    a.leaves[i] = t < len ? pm : 0.f;
    a.dirty1[i / F] = 1;
    return;
  }
  const int e = a.ep_lo + ((int)blockIdx.x - a.row_blocks);
  const int len = e < a.n_eps ? ep_len(a.ends, e) : 0;
  const int old = a.lens[e];
  __syncthreads();            // (every thread has read lens[e] before it changes)
  if (len == old) return;
  if (threadIdx.x == 0) a.lens[e] = len;
  const int lo = min(len, old), hi = max(len, old);
  for (int t = lo + (int)threadIdx.x; t < hi; t += kThreads) {
    const long i = (long)e * a.L + t;
    a.leaves[i] = t < len ? pm : 0.f;
    a.dirty1[i / F] = 1;
  }
}

struct LevelArgs {
  float* tree;
  int* dirty;
  long child_off, node_off, n_nodes, flag_off, parent_flag_off;   // parent_flag_off < 0: this is the root's level
  int all;
};

// one wave per node of one level: the node from its children when it is flagged (or `all`); the flag is cleared and
// the parent's raised
__global__ __launch_bounds__(kThreads) void k_prio_level(const LevelArgs a) {
  const long node = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (node >= a.n_nodes) return;
  if (!a.all && a.dirty[a.flag_off + node] == 0) return;
  const float v = node_sum(a.tree + a.child_off + node * F, lane);
  if (lane == 0) {
    a.tree[a.node_off + node] = v;
    a.dirty[a.flag_off + node] = 0;
    if (a.parent_flag_off >= 0) a.dirty[a.parent_flag_off + node / F] = 1;
  }
}

struct SampleArgs {
  const float* tree;
  long off[oprl::kPrioMaxLevels];
  int n_levels;
  const int* ends;
  int L, B;
  unsigned long long seed, counter;
  int* out_slot;
  float* out_p;               // the rows' leaves (k_prio_weights turns them into weights in place)
  long long* idx;             // the rows' flat transition indices, for k_replay_gather
};

// One wave per row j.  u = (j + U) * (root / B), U uniform in [0, 1) from 24 Philox bits; at each level the children's
// running prefixes P (a lane's four in order, the lanes' totals by an inclusive Hillis-Steele scan) pick the first
// child with P > u and a nonzero value, else (rounding at the end of the last segment) the last nonzero child; u loses
// the chosen child's exclusive prefix, clamped at 0.  DESIGN.md §11 states the arithmetic; tests/per_oracle.py restates it.
__global__ __launch_bounds__(kThreads) void k_prio_sample(const SampleArgs a) {
  const int j = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= a.B) return;
  const float total = a.tree[a.off[a.n_levels - 1]];
  const float seg = (float)((double)total / (double)a.B);
  const oprl::u32x4 r = oprl::philox4x32_10(
      oprl::u32x4{(uint32_t)a.counter, (uint32_t)(a.counter >> 32), (uint32_t)j, kSampleWord},
      (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  const float U = (float)(r.x >> 8) * (1.0f / 16777216.0f);
  float u = ((float)j + U) * seg;
  long node = 0;
  for (int k = a.n_levels - 1; k >= 1; --k) {
    const float4 c = reinterpret_cast<const float4*>(a.tree + a.off[k - 1] + node * F)[lane];
    const float q0 = c.x, q1 = q0 + c.y, q2 = q1 + c.z, q3 = q2 + c.w;
    float x = q3;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float y = __shfl_up(x, d, 64);
      if (lane >= d) x = y + x;
    }
    float ex = __shfl_up(x, 1, 64);
    if (lane == 0) ex = 0.f;
    const float p0 = ex + q0, p1 = ex + q1, p2 = ex + q2, p3 = ex + q3;
    int pick = (c.x > 0.f && p0 > u) ? 0 : (c.y > 0.f && p1 > u) ? 1 : (c.z > 0.f && p2 > u) ? 2 : (c.w > 0.f && p3 > u) ? 3 : -1;
    unsigned long long m = __ballot(pick >= 0);
    int ls;
    if (m != 0ull) {
      ls = __builtin_ctzll(m);
    } else {
      pick = c.w > 0.f ? 3 : c.z > 0.f ? 2 : c.y > 0.f ? 1 : c.x > 0.f ? 0 : -1;
      m = __ballot(pick >= 0);
      if (m == 0ull) { node = -1; break; }      // a node without mass: the root is 0
      ls = 63 - __builtin_clzll(m);
    }
    const int ks = __shfl(pick, ls, 64);
    const float pe_l = ks == 0 ? ex : ks == 1 ? p0 : ks == 2 ? p1 : p2;
    const float pe = __shfl(pe_l, ls, 64);
    u = fmaxf(u - pe, 0.f);
    node = node * F + ls * 4 + ks;
  }
  if (lane == 0) {
    float p = 0.f;
    long long flat = 0;
    int slot = -1;
    if (node >= 0) {
      p = a.tree[a.off[0] + node];
      const int e = (int)(node / a.L), t = (int)(node - (long)e * a.L);
      flat = (long long)(e > 0 ? a.ends[e - 1] : 0) + t;
      slot = (int)node;
    }
    a.out_slot[j] = slot;
    a.out_p[j] = p;
    a.idx[j] = flat;
  }
}

// w[j] = (p_min / p_j)^beta, in double, rounded once: (N·p_j / total)^-beta over the batch's largest, with N and the
// total cancelled.  One workgroup; w holds the rows' leaves on entry (0 for a row of an empty tree, which stays 0).
__global__ __launch_bounds__(1024) void k_prio_weights(float* w, int B, double beta) {
  __shared__ float s_min[16];
  float m = INFINITY;
  for (int j = threadIdx.x; j < B; j += 1024) {
    const float p = w[j];
    if (p > 0.f) m = fminf(m, p);
  }
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) m = fminf(m, __shfl_xor(m, h, 64));
  if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = m;
  __syncthreads();
  m = s_min[0];
  for (int k = 1; k < 16; ++k) m = fminf(m, s_min[k]);
  for (int j = threadIdx.x; j < B; j += 1024) {
    const float p = w[j];
    w[j] = p > 0.f ? (float)pow((double)m / (double)p, beta) : 0.f;
  }
}

// Priority update, pass 1: every live row claims its slot, owner[slot] = max(owner[slot], j) (integer maximum: the
// largest batch index wins in any order), and p_max takes the maximum of the rows' priorities (an integer maximum of
// the non-negative floats' bits).  p = (max(td[j], 0) + eps)^alpha in double, rounded once.  Rows whose slot is no
// longer live (its episode was cut after the draw) take no part: the leaf stays 0.
__device__ __forceinline__ float prio_of(const float* td, int j, double alpha, double eps) {
  return (float)pow(fmax((double)td[j], 0.0) + eps, alpha);
}
__device__ __forceinline__ bool live_slot(const int* lens, int s, int L, long n_slots) {
  return s >= 0 && (long)s < n_slots && s - (s / L) * L < lens[s / L];
}
__global__ __launch_bounds__(kThreads) void k_prio_claim(int* owner, float* p_max, const int* lens, const int* slot,
                                                        const float* td, int B, int L, long n_slots, double alpha,
                                                        double eps) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= B) return;
  const int s = slot[j];
  if (!live_slot(lens, s, L, n_slots)) return;
  atomicMax(owner + s, j);
  atomicMax(reinterpret_cast<unsigned int*>(p_max), __float_as_uint(prio_of(td, j, alpha, eps)));
}
// pass 2: the row that owns its slot writes the leaf, flags the parent and releases the slot (owner -1 again; the
// other rows of that slot compare their own index and skip either way)
__global__ __launch_bounds__(kThreads) void k_prio_update(float* leaves, int* dirty1, int* owner, const int* lens,
                                                         const int* slot, const float* td, int B, int L, long n_slots,
                                                         double alpha, double eps) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= B) return;
  const int s = slot[j];
  if (!live_slot(lens, s, L, n_slots) || owner[s] != j) return;
  leaves[s] = prio_of(td, j, alpha, eps);
  dirty1[s / F] = 1;
  owner[s] = -1;
}

void prio_layout(oprl::PrioTree* p, long n_leaves) {
  long c = n_leaves;
  int k = 0;
  p->off[0] = 0;
  for (;;) {
    p->count[k] = c;
    p->off[k + 1] = p->off[k] + (c + F - 1) / F * F;
    ++k;
    if ((c == 1 && k >= 2) || k >= oprl::kPrioMaxLevels) break;
    c = (c + F - 1) / F;
  }
  p->n_levels = k;
}

// every internal level, root last: the flagged nodes (all = false) or all of them
int prio_levels(const oprl::PrioTree* p, bool all, hipStream_t st) {
  for (int k = 1; k < p->n_levels; ++k) {
    LevelArgs a;
    a.tree = p->tree; a.dirty = p->dirty;
    a.child_off = p->off[k - 1]; a.node_off = p->off[k]; a.n_nodes = p->count[k];
    a.flag_off = p->off[k] - p->off[1];
    a.parent_flag_off = k + 1 < p->n_levels ? p->off[k + 1] - p->off[1] : -1;
    a.all = all ? 1 : 0;
    hipLaunchKernelGGL(k_prio_level, dim3((unsigned)((a.n_nodes + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, a);
    HIPC(hipGetLastError());
  }
  return OPRL_OK;
}

// leaves from the device's episode table (src: loaded leaves, or null for pm on every live slot), then every node
int prio_init(oprl_replay* h, const float* src, float pm, hipStream_t st) {
  oprl::PrioTree* p = h->prio;
  HIPC(hipMemsetAsync(p->dirty, 0, sizeof(int) * (p->off[p->n_levels] - p->off[1]), st));
  const long n_pad = p->off[1];
  hipLaunchKernelGGL(k_prio_init, dim3((unsigned)((n_pad + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, p->tree,
                     n_pad, p->lens, p->p_max, (const int*)h->ends_dev, h->n_eps, h->E, h->L, src, pm);
  HIPC(hipGetLastError());
  p->n_eps = h->n_eps;
  return prio_levels(p, true, st);
}

int need_prio(const oprl_replay* h, const char* what) {
  if (!h) { set_err("%s: null replay handle", what); return OPRL_ERR_INVALID; }
  if (!h->prio) { set_err("%s: prioritized replay is not enabled (oprl_replay_prio_enable)", what); return OPRL_ERR_STATE; }
  return OPRL_OK;
}

}  // namespace

namespace oprl {

int prio_flush(oprl_replay* h, const float* rows, int n_rows, int rowlen, int ends_first, int ends_n, hipStream_t st) {
  PrioTree* p = h->prio;
  // the episodes whose length may have changed: the uploaded part of the table, and those that entered or left
  // [0, episodes_counter)
  int lo = h->E, hi = 0;
  if (ends_n > ends_first) { lo = ends_first; hi = ends_n; }
  if (h->n_eps != p->n_eps) {
    lo = std::min(lo, std::min(h->n_eps, p->n_eps));
    hi = std::max(hi, std::max(h->n_eps, p->n_eps));
  }
  hi = std::min(hi, h->E);
  if (hi < lo) hi = lo;
  p->n_eps = h->n_eps;
  const int row_blocks = (n_rows + kThreads - 1) / kThreads, grid = row_blocks + (hi - lo);
  if (grid == 0) return OPRL_OK;
  FlushArgs a;
  a.leaves = p->tree; a.dirty1 = p->dirty; a.lens = p->lens; a.ends = h->ends_dev; a.p_max = p->p_max;
  a.rows = rows; a.n_rows = n_rows; a.rowlen = rowlen; a.L = h->L; a.n_eps = h->n_eps; a.ep_lo = lo;
  a.row_blocks = row_blocks;
  hipLaunchKernelGGL(k_prio_flush, dim3(grid), dim3(kThreads), 0, st, a);
  HIPC(hipGetLastError());
  return prio_levels(p, false, st);
}

void prio_free(PrioTree* p) {
  if (!p) return;
  (void)hipFree(p->tree);
  (void)hipFree(p->dirty);
  (void)hipFree(p->lens);
  (void)hipFree(p->p_max);
  (void)hipFree(p->owner);
  (void)hipFree(p->idx);
  delete p;
}

}  // namespace oprl

extern "C" int oprl_replay_prio_enable(oprl_replay* h, double alpha, double eps, void* stream) {
  if (!h || !(alpha >= 0.0) || !(eps > 0.0)) {
    set_err("oprl_replay_prio_enable: invalid argument (need a handle, alpha >= 0, eps > 0)");
    return OPRL_ERR_INVALID;
  }
  if (h->nstep > 1) {
    set_err("oprl_replay_prio_enable: this replay samples %d-step returns (oprl_replay_set_nstep); the sum tree over n-step rows is not supported", h->nstep);
    return OPRL_ERR_STATE;
  }
  if (h->her.G > 0) {
    set_err("oprl_replay_prio_enable: this replay relabels goals in hindsight (oprl_replay_set_her); the sum tree over relabelled rows is not supported");
    return OPRL_ERR_STATE;
  }
  if (h->prior) {
    set_err("oprl_replay_prio_enable: this replay mixes prior data into its batches (oprl_replay_set_prior); the sum tree over mixed batches is not supported");
    return OPRL_ERR_STATE;
  }
  hipStream_t st = (hipStream_t)stream;
  int rc = oprl_replay_flush(h, stream);          // the episode table the leaves start from
  if (rc != OPRL_OK) return rc;
  if (!h->prio) {
    auto* p = new oprl::PrioTree();
    prio_layout(p, (long)h->E * h->L);
    if (p->count[p->n_levels - 1] != 1) { delete p; set_err("oprl_replay_prio_enable: replay too large for the sum tree"); return OPRL_ERR_INVALID; }
    const size_t n = (size_t)p->off[p->n_levels], nf = (size_t)(p->off[p->n_levels] - p->off[1]);
    hipError_t e = hipMalloc(&p->tree, sizeof(float) * n);
    if (e == hipSuccess) e = hipMalloc(&p->dirty, sizeof(int) * nf);
    if (e == hipSuccess) e = hipMalloc(&p->lens, sizeof(int) * h->E);
    if (e == hipSuccess) e = hipMalloc(&p->p_max, sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&p->owner, sizeof(int) * (size_t)h->E * h->L);
    if (e == hipSuccess) e = hipMemsetAsync(p->owner, 0xff, sizeof(int) * (size_t)h->E * h->L, st);   // every slot unclaimed (-1)
    if (e == hipSuccess) e = hipMemsetAsync(p->tree, 0, sizeof(float) * n, st);   // (the padding of the internal levels stays 0)
    if (e != hipSuccess) {     // the handle keeps no partial tree: it stays a uniform replay
      oprl::prio_free(p);
      set_err("oprl_replay_prio_enable: %s", hipGetErrorString(e));
      return OPRL_ERR_HIP;
    }
    h->prio = p;
  }
  h->prio->alpha = alpha;
  h->prio->eps = eps;
  return prio_init(h, nullptr, 1.0f, st);
}

extern "C" int oprl_replay_prio_sample(oprl_replay* h, int32_t B, uint64_t seed, uint64_t counter, double beta,
                                       float* out_s, float* out_a, float* out_r, float* out_d, float* out_s2,
                                       int32_t* out_slot, float* out_w, void* stream) {
  int rc = need_prio(h, "oprl_replay_prio_sample");
  if (rc != OPRL_OK) return rc;
  if (B < 1 || !out_s || !out_a || !out_r || !out_d || !out_s2 || !out_slot || !out_w || !(beta >= 0.0)) {
    set_err("oprl_replay_prio_sample: invalid argument");
    return OPRL_ERR_INVALID;
  }
  if (h->n_transitions <= 0 || h->n_eps <= 0) { set_err("oprl_replay_prio_sample: buffer is empty"); return OPRL_ERR_STATE; }
  hipStream_t st = (hipStream_t)stream;
  rc = oprl_replay_flush(h, stream);
  if (rc != OPRL_OK) return rc;
  oprl::PrioTree* p = h->prio;
  if (B > p->idx_cap) {
    if (p->idx) { HIPC(hipDeviceSynchronize()); HIPC(hipFree(p->idx)); p->idx = nullptr; p->idx_cap = 0; }
    HIPC(hipMalloc(&p->idx, sizeof(long long) * B));
    p->idx_cap = B;
  }
  SampleArgs a;
  a.tree = p->tree;
  for (int k = 0; k < oprl::kPrioMaxLevels; ++k) a.off[k] = p->off[k];
  a.n_levels = p->n_levels; a.ends = h->ends_dev; a.L = h->L; a.B = B; a.seed = seed; a.counter = counter;
  a.out_slot = out_slot; a.out_p = out_w; a.idx = p->idx;
  hipLaunchKernelGGL(k_prio_sample, dim3((B + kWaves - 1) / kWaves), dim3(kThreads), 0, st, a);
  HIPC(hipGetLastError());
  hipLaunchKernelGGL(k_prio_weights, dim3(1), dim3(1024), 0, st, out_w, (int)B, beta);
  HIPC(hipGetLastError());
  return oprl_replay_sample(h, B, (const int64_t*)p->idx, 0, 0, out_s, out_a, out_r, out_d, out_s2, nullptr, nullptr, stream);
}

extern "C" int oprl_replay_prio_update(oprl_replay* h, int32_t B, const int32_t* slot, const float* td_abs, void* stream) {
  int rc = need_prio(h, "oprl_replay_prio_update");
  if (rc != OPRL_OK) return rc;
  if (B < 1 || !slot || !td_abs) {
    set_err("oprl_replay_prio_update: invalid argument (B >= 1, slot and td_abs)");
    return OPRL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  rc = oprl_replay_flush(h, stream);
  if (rc != OPRL_OK) return rc;
  oprl::PrioTree* p = h->prio;
  const long n_slots = (long)h->E * h->L;
  const dim3 grid((B + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(k_prio_claim, grid, dim3(kThreads), 0, st, p->owner, p->p_max, (const int*)p->lens, slot, td_abs,
                     (int)B, h->L, n_slots, p->alpha, p->eps);
  HIPC(hipGetLastError());
  hipLaunchKernelGGL(k_prio_update, grid, dim3(kThreads), 0, st, p->tree, p->dirty, p->owner, (const int*)p->lens,
                     slot, td_abs, (int)B, h->L, n_slots, p->alpha, p->eps);
  HIPC(hipGetLastError());
  return prio_levels(p, false, st);
}

extern "C" int oprl_replay_prio_read(oprl_replay* h, float* tree_out, int64_t n, int64_t* n_floats_host,
                                     float* p_max_host, void* stream) {
  int rc = need_prio(h, "oprl_replay_prio_read");
  if (rc != OPRL_OK) return rc;
  oprl::PrioTree* p = h->prio;
  const int64_t size = p->off[p->n_levels];
  if (tree_out != nullptr && n < size) {
    set_err("oprl_replay_prio_read: the tree holds %lld floats, the output %lld", (long long)size, (long long)n);
    return OPRL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  rc = oprl_replay_flush(h, stream);
  if (rc != OPRL_OK) return rc;
  if (n_floats_host) *n_floats_host = size;
  if (tree_out) HIPC(hipMemcpyAsync(tree_out, p->tree, sizeof(float) * size, hipMemcpyDeviceToDevice, st));
  if (p_max_host) {
    HIPC(hipMemcpyAsync(p_max_host, p->p_max, sizeof(float), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
  }
  return OPRL_OK;
}

extern "C" int oprl_replay_prio_load(oprl_replay* h, const float* leaves, float p_max, void* stream) {
  int rc = need_prio(h, "oprl_replay_prio_load");
  if (rc != OPRL_OK) return rc;
  if (!leaves || !(p_max > 0.f)) { set_err("oprl_replay_prio_load: invalid argument (leaves, p_max > 0)"); return OPRL_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  rc = oprl_replay_flush(h, stream);
  if (rc != OPRL_OK) return rc;
  return prio_init(h, leaves, p_max, st);
}
