// replay_rows.hip — one step of up to 256 open episodes into the HBM replay in one call and one launch
// (oprl_replay_write_rows).  Record i of a call is the next step of ITS episode:
//   [ep, t] as two ints bit-cast into floats, then s[S] | s'[S] | a[A] | r | d
// and the kernel stores s | s' as ONE contiguous run of 2·S floats: states is [E, L+1, S], so (ep, t) and (ep, t+1)
// are adjacent rows — the next state of every stored step is in storage, the tail of a running episode and the last
// step of a truncated one included.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/oprl_amd.h"
#include "replay_internal.h"

namespace {

constexpr int kWave = 64;
constexpr int kU = 4;       // columns per lane and round: every load of a round is issued before its first store

// One wave per record; the lanes stride over its 2S + A + 2 data columns, so the loads (one record) and the stores (the
// 2·S run, the action row) are coalesced.  Column c goes to: c < 2S the run at states[e, t]; c < 2S + A actions[e, t];
// then rewards[e, t] and dones[e, t].  A record of up to kU·64 = 256 columns (2S + A + 2 <= 256) is one round, so all its
// loads precede its first store; wider records take further rounds.  The records of one launch name distinct episodes
// (the host refuses anything else): no two waves write one address and nothing depends on their order.  The same
// launch copies the changed range [ends_first, ends_n) of the episode-ends table, as k_replay_ingest does.
__global__ __launch_bounds__(kWave) void k_replay_ingest_rows(const float* recs, int n, int reclen, float* states,
                                                              float* actions, float* rewards, float* dones, int L, int S,
                                                              int A, const int* ends_src, int* ends_dst, int ends_first,
                                                              int ends_n) {
  const int lane = threadIdx.x, W = 2 * S + A + 2;
  for (int rix = blockIdx.x; rix < n; rix += gridDim.x) {
    const float* rec = recs + (size_t)rix * reclen;
    const long e = __float_as_int(rec[0]), t = __float_as_int(rec[1]);
    float* const run = states + (e * (L + 1) + t) * S;
    float* const act = actions + (e * L + t) * A;
    for (int c0 = 0; c0 < W; c0 += kU * kWave) {
      float v[kU];
#pragma unroll
      for (int j = 0; j < kU; ++j) v[j] = rec[2 + min(c0 + j * kWave + lane, W - 1)];
#pragma unroll
      for (int j = 0; j < kU; ++j) {
        const int c = c0 + j * kWave + lane;
        if (c >= W) continue;
        float* dst = run + min(c, 2 * S - 1);                  // (branch-free selection, as k_replay_gather's sources)
        if (c >= 2 * S) dst = act + min(c - 2 * S, A - 1);
        if (c == 2 * S + A) dst = rewards + e * L + t;
        if (c == 2 * S + A + 1) dst = dones + e * L + t;
        *dst = v[j];
      }
    }
  }
  for (int i = ends_first + (int)(blockIdx.x * blockDim.x + threadIdx.x); i < ends_n; i += (int)(gridDim.x * blockDim.x))
    ends_dst[i] = ends_src[i];
}

// the records' staging, allocated by the first oprl_replay_write_rows of a handle: two pinned, host-mapped areas of
// kRowsMax records and their device copies, guarded by events as stage_host / stage_ev are
int rows_area(oprl_replay* h) {
  if (h->rows_ready) return OPRL_OK;
  h->reclen = 2 + 2 * h->S + h->A + 2;
  const size_t bytes = sizeof(float) * h->reclen * oprl::kRowsMax;
  hipError_t e = hipSuccess;
  for (int i = 0; i < 2 && e == hipSuccess; ++i) {
    e = hipHostMalloc(&h->rows_host[i], bytes);
    if (e == hipSuccess) e = hipMalloc(&h->rows_dev[i], bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->rows_ev[i], hipEventDisableTiming);
    if (e != hipSuccess) break;
    h->rows_ev_made[i] = true;
    if (hipHostGetDevicePointer((void**)&h->rows_map[i], h->rows_host[i], 0) != hipSuccess) h->rows_map[i] = nullptr;
  }
  (void)hipGetLastError();
  if (e != hipSuccess) {      // the handle keeps no partial area
    oprl::rows_free(h);
    set_err("oprl_replay_write_rows: staging for %d records: %s", oprl::kRowsMax, hipGetErrorString(e));
    return OPRL_ERR_HIP;
  }
  h->rows_ready = true;
  return OPRL_OK;
}

}  // namespace

namespace oprl {
void rows_free(oprl_replay* h) {
  for (int i = 0; i < 2; ++i) {
    if (h->rows_host[i]) (void)hipHostFree(h->rows_host[i]);
    if (h->rows_dev[i]) (void)hipFree(h->rows_dev[i]);
    if (h->rows_ev_made[i]) (void)hipEventDestroy(h->rows_ev[i]);
    h->rows_host[i] = h->rows_dev[i] = h->rows_map[i] = nullptr;
    h->rows_ev_made[i] = false;
  }
  h->rows_ready = false;
}
}  // namespace oprl

extern "C" int oprl_replay_write_rows(oprl_replay* h, int32_t n, const int32_t* ep, const int32_t* t, const float* s,
                                      const float* a, const float* r, const float* d, const float* s2,
                                      const int32_t* ep_lens_host, int32_t episodes_counter, void* stream) {
  // 1. everything that can be refused is refused here, before anything is staged, launched or changed
  if (!h || !ep || !t || !s || !a || !r || !d || !s2 || !ep_lens_host) {
    set_err("oprl_replay_write_rows: null argument");
    return OPRL_ERR_INVALID;
  }
  if (n < 1 || n > oprl::kRowsMax) {
    set_err("oprl_replay_write_rows: n=%d outside 1 .. %d", n, oprl::kRowsMax);
    return OPRL_ERR_INVALID;
  }
  int sorted[oprl::kRowsMax];
  for (int i = 0; i < n; ++i) {
    if (ep[i] < 0 || ep[i] >= h->E || t[i] < 0 || t[i] >= h->L) {
      set_err("oprl_replay_write_rows: record %d: slot (%d,%d) outside [0,%d) x [0,%d)", i, ep[i], t[i], h->E, h->L);
      return OPRL_ERR_INVALID;
    }
    sorted[i] = ep[i];
  }
  std::sort(sorted, sorted + n);
  for (int i = 1; i < n; ++i)
    if (sorted[i] == sorted[i - 1]) {
      set_err("oprl_replay_write_rows: two records for episode %d (one step per episode and call)", sorted[i]);
      return OPRL_ERR_INVALID;
    }
  int rc = oprl::check_lens(h, ep_lens_host, episodes_counter, "oprl_replay_write_rows");
  if (rc != OPRL_OK) return rc;
  rc = rows_area(h);
  if (rc != OPRL_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  // 2. rows the classic entry points staged earlier go first: stream order is call order
  rc = oprl_replay_flush(h, stream);
  if (rc != OPRL_OK) return rc;
  // 3. the records
  const int c = h->rows_cur, S = h->S, A = h->A, reclen = h->reclen;
  if (h->rows_busy[c]) { HIPC(hipEventSynchronize(h->rows_ev[c])); h->rows_busy[c] = false; }
  for (int i = 0; i < n; ++i) {
    float* rec = h->rows_host[c] + (size_t)i * reclen;
    memcpy(rec, ep + i, 4);
    memcpy(rec + 1, t + i, 4);
    memcpy(rec + 2, s + (size_t)i * S, sizeof(float) * S);
    memcpy(rec + 2 + S, s2 + (size_t)i * S, sizeof(float) * S);
    memcpy(rec + 2 + 2 * S, a + (size_t)i * A, sizeof(float) * A);
    rec[2 + 2 * S + A] = r[i];
    rec[3 + 2 * S + A] = d[i];
  }
  // 4. the episode table
  rc = oprl_replay_set_lens(h, ep_lens_host, episodes_counter, stream);
  if (rc != OPRL_OK) return rc;
  // 5. one launch: the records and the table's changed range
  const int ec = h->ends_cur;
  const oprl::PendingEnds pe = oprl::pending_ends(h, n, h->rows_map[c], h->ends_map[ec]);
  const int e_first = pe.first, e_n = pe.n;
  const bool direct = pe.direct;
  const float* recs = direct ? h->rows_map[c] : h->rows_dev[c];
  if (!direct) HIPC(hipMemcpyAsync(h->rows_dev[c], h->rows_host[c], sizeof(float) * reclen * n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_replay_ingest_rows, dim3(n), dim3(kWave), 0, st, recs, (int)n, reclen, h->states, h->actions,
                     h->rewards, h->dones, h->L, S, A, direct ? h->ends_map[ec] : nullptr, h->ends_dev,
                     direct ? e_first : 0, direct ? e_n : 0);
  HIPC(hipGetLastError());
  if (!direct && e_n > e_first)
    HIPC(hipMemcpyAsync(h->ends_dev + e_first, h->ends_host[ec] + e_first, sizeof(int) * (e_n - e_first),
                        hipMemcpyHostToDevice, st));
  // 6. the sum tree follows the records and the table
  if (h->prio) {
    rc = oprl::prio_flush(h, recs, n, reclen, e_first, e_n, st);
    if (rc != OPRL_OK) return rc;
  }
  HIPC(hipEventRecord(h->rows_ev[c], st));
  h->rows_busy[c] = true;
  h->rows_cur ^= 1;
  return oprl::ends_sent(h, st);
}
