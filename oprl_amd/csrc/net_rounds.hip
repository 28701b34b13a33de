// net_rounds.hip — how the net passes of the generic (per-net) launch sequence go out.  Host code only.
// learner_generic.hip builds the arguments of a round — the n equal nets of one pass: twin critics, TQC's quantile critics, REDQ's
// ensemble or its target subset — and launch_round decides the launches from that list.  No state of an earlier call is
// read, except the offers TQC's riders make to the layer-by-layer round (learner_internal.h: *_pending / *_done).
#include "learner_internal.h"

namespace oprl_host {

// launch-unique 26-bit tag for the cluster exchanges of one learner; on wrap-around every stale
// granule is retired
int next_tp_tag(unsigned* counter, unsigned long long* xbuf, size_t xbuf_bytes, hipStream_t st, unsigned* out) {
  *counter += 1;
  if ((*counter & 0x03FFFFFFu) == 0) {
    *counter += 1;
    HIPC(hipMemsetAsync(xbuf, 0, xbuf_bytes, st));
  }
  *out = *counter & 0x03FFFFFFu;
  return OPRL_OK;
}

namespace {

// does this net pass run on tensor-parallel clusters (slice_tp.hip)?  Every cluster launch draws its tag, in net order
bool takes_cluster(const MlpArgs& a, int width) { return a.tp_xbuf != nullptr && mlp_slice_tp_shape_ok(a, width); }
int draw_tag(MlpArgs& a, hipStream_t st) { return next_tp_tag(a.tp_tag_counter, a.tp_xbuf, a.tp_xbuf_bytes, st, &a.tp_tag); }

// twin nets on the same slices: their cluster launches go out as ONE (k_mlp_slice_tp2) when the batches are equal; a net
// that takes no cluster launch goes out on its own
int launch_pair(oprl_learner* h, MlpArgs* a, int width, hipStream_t st) {
  MlpArgs* tp[2];
  int n_tp = 0;
  for (int k = 0; k < 2; ++k) {
    if (takes_cluster(a[k], width)) {
      RC(draw_tag(a[k], st));
      tp[n_tp++] = &a[k];
    } else {
      RC(launch(a[k], width, st));
    }
  }
  if (n_tp == 2 && tp[0]->B == tp[1]->B) {
    RC(profiled(0, st, [&] { return launch_mlp_slice_tp2(*tp[0], *tp[1], h->n_cus, st); }));
    return OPRL_OK;
  }
  for (int k = 0; k < n_tp; ++k) {
    RC(profiled(0, st, [&] { return launch_mlp_slice_tp(*tp[k], st); }));
  }
  return OPRL_OK;
}

// Three to five equal wide nets layer by layer over the whole chip (layerwise.hip), with whatever TQC's update has on
// offer for this launch: the TD-target job, the actor's forward and backward as riders, the tail of the early first
// launch, the next update's rows, the actor's dW tiles.  An offer that is taken is marked so on the learner.
int launch_layerwise_round(oprl_learner* h, MlpArgs* a, int n, int width, hipStream_t st) {
  // bf16 learners: the hidden layers (all but the first and the last) through their bf16 packs
  bool lw16 = h->bf16 || h->x2;
  for (int k = 0; k < n; ++k)
    for (int l = 1; l + 1 < a[k].net.n_layers; ++l)
      lw16 = lw16 && a[k].pf16[l] != nullptr && (!a[k].do_bwd || a[k].pb16[l] != nullptr);
  if (lw16)
    for (int k = 0; k < n; ++k)
      for (int l = 1; l + 1 < a[k].net.n_layers; ++l) { a[k].net.pf[l] = a[k].pf16[l]; if (a[k].pb16[l]) a[k].net.pb[l] = a[k].pb16[l]; }
  prof_begin(0, st);
  // a pending TD-target job (generic_critic_phase) rides on this launch's heads when it is the target critics' forward
  const TqcJob* job = nullptr;
  if (h->tqc_job_pending && !a[0].do_bwd && a[0].do_fwd && n == h->tqc_job.n_nets && a[0].out == h->tqc_job.z) {
    job = &h->tqc_job;
    h->tqc_job_pending = false;
  }
  // a pending rider (generic_critic_phase: the actor's forward on s) goes with the storing launch's heads
  const MlpArgs* rider = nullptr;
  if (h->rider_pending && a[0].do_bwd && a[0].do_fwd && mlp_layerwise_rider_ok(a, n, h->rider, h->n_cus)) {
    rider = &h->rider;
    h->rider_pending = false;
    h->rider_done = true;
  }
  const bool first_done = h->fin_done && a[0].do_bwd && a[0].do_fwd && a[0].Xg[0] != nullptr;
  if (first_done) h->fin_done = false;
  const bool second_done = first_done && h->fin_l2_done;
  if (first_done) h->fin_l2_done = false;
  // the part of the online critics' early first launch that did not fit beside the actor's forward rides on the
  // target pass's heads (forward-only launch, 80 workgroups)
  const MlpArgs* tail = nullptr;
  int tail0 = 0;
  if (h->fin_tail0 >= 0 && !a[0].do_bwd && a[0].do_fwd) {
    const int slices = n_slices(a[0].B);
    const int rest = h->nc - h->fin_tail0;
    if (mlp_layerwise_fin_fit(h->fin_args, h->nc, slices * n, h->n_cus) >= rest) {   // all resident at once
      tail = h->fin_args; tail0 = h->fin_tail0;
      h->fin_tail0 = -1;
    }
  }
  // step_n: the next update's rows ride on the launch sequence that ends in k_lw_dact (the actor step's critics)
  const PrefetchJob* pf = nullptr;
  if (h->prefetch_pending && a[0].do_bwd && a[0].dact_cols > 0 && h->prefetch.B == a[0].B) {
    pf = &h->prefetch;
    h->prefetch_pending = false;
    h->prefetch_done = true;
  }
  hipError_t e = launch_mlp_layerwise(a, n, width, h->n_cus, st, lw16 ? (h->x2 ? 2 : 1) : 0, job, rider, first_done,
                                      tail, h->nc, tail0, h->fin16 ? (h->x2 ? 2 : 1) : 0, pf, &h->lw_pairs, second_done,
                                      tail != nullptr ? &h->fin_l2_done : nullptr,
                                      (h->bwd_rider_pending && a[0].do_bwd && a[0].dact_cols > 0) ? &h->bwd_rider : nullptr,
                                      &h->bwd_rider_done, h->bwd_tiles_pending ? &h->bwd_tiles : nullptr, h->bwd_tile_wgs, &h->bwd_tiles_done);
  h->bwd_rider_pending = false;
  h->bwd_tiles_pending = false;
  // (a tag per pair launch; 2^32 launches on: every flag is retired before a tag can come round again)
  if (h->lw_pairs.next_tag + (unsigned)h->lw_pairs.used < h->lw_pairs.next_tag && h->lw_pairs.flags != nullptr)
    (void)hipMemsetAsync(h->lw_pairs.flags, 0, (size_t)h->lw_pairs.n_flags * sizeof(unsigned long long), st);
  h->lw_pairs.next_tag += (unsigned)h->lw_pairs.used;
  if (h->lw_pairs.next_tag == 0) h->lw_pairs.next_tag = 1;
  h->lw_pairs.used = 0;
  prof_end(st);
  HIPC(e);
  return OPRL_OK;
}

// Three to kMaxMulti nets on the same slices (TQC's quantile critics; REDQ's target subset): a cluster launch each, in order,
// or — the nets that take none; equal in shape, so all or none — layer by layer, else one k_mlp_slice_multi launch (grid (slices, nets))
int launch_few(oprl_learner* h, MlpArgs* a, int n, int width, hipStream_t st) {
  int m = 0;
  for (int j = 0; j < n; ++j) {
    if (takes_cluster(a[j], width)) { RC(launch(a[j], width, st)); continue; }
    if (m != j) a[m] = a[j];
    ++m;
  }
  if (m == 0) return OPRL_OK;
  bool same = true;
  for (int k = 1; k < m; ++k) same = same && a[k].B == a[0].B && a[k].net.n_layers == a[0].net.n_layers;
  const bool layerwise = same && !h->sw.no_layerwise;
  // wide nets go layer by layer over the whole chip (csrc/layerwise.hip); launches that keep no
  // activations (target nets, the actor phase's critics) borrow the nets' dW exchange buffers,
  // which nobody reads until the next storing launch overwrites them
  if (layerwise && width == 512 && m <= h->nc) {
    for (int k = 0; k < m; ++k) {
      const NetWs& ws = h->ws_critic[k];
      for (int l = 1; l < a[k].net.n_layers; ++l)
        if (a[k].Xg[l] == nullptr)
          a[k].Xg[l] = (!a[k].do_bwd && h->lw_scratch != nullptr)
                           ? h->lw_scratch + ((size_t)k * (kMaxLayers - 1) + (l - 1)) * (size_t)h->Bmax * 512
                           : ws.X[l];
      for (int l = 0; l + 1 < a[k].net.n_layers; ++l)
        if (a[k].dYg[l] == nullptr) a[k].dYg[l] = ws.dY[l];
    }
  }
  if (layerwise && mlp_layerwise_ok(a, m, width)) return launch_layerwise_round(h, a, m, width, st);
  // (these kernels read the fp32 packs: a 16-bit TQC learner's wide critics leave theirs stale)
  if (h->stale_wide && width == h->w_critic) RC(fresh32_tables(h, 1, st, true));
  if (!same) {
    for (int k = 0; k < m; ++k) RC(launch(a[k], width, st));
    return OPRL_OK;
  }
  RC(profiled(0, st, [&] { return launch_mlp_slice_multi(a, m, width, st); }));
  return OPRL_OK;
}

// A net pass that carries an LN view (MlpArgs::reserved: a critic of a learner with layer normalisation)
// goes to the LN kernels (ln_slice.hip).  What of the view this launch uses: the per-slice dgamma / dbeta sums only where
// the dW launch follows (forward + backward with the dY rows stored: the critic step), the zh / rstd rows only where the
// pass is split into a forward-only and a backward-only launch
LnView ln_view_of(const MlpArgs& a) {
  LnView v = *static_cast<const LnView*>(a.reserved);
  const bool whole = a.do_fwd && a.do_bwd;
  if (!whole || a.dYg[0] == nullptr) v.sums = nullptr;
  if (whole || (a.do_fwd && a.Xg[1] == nullptr))
    for (int l = 0; l < kLnHidden; ++l) { v.zh[l] = nullptr; v.rstd[l] = nullptr; }
  return v;
}

// a round of n LN nets: ceil(n / kMaxMulti) k_mlp_slice_multi_ln launches, whatever n
int launch_ln_round(MlpArgs* a, int n, int width, hipStream_t st) {
  if (width != kLnWidth) { set_err("internal: an LN net pass at width %d", width); return OPRL_ERR_STATE; }
  for (int j0 = 0; j0 < n; j0 += kMaxMulti) {
    const int m = std::min(kMaxMulti, n - j0);
    LnView v[kMaxMulti];
    for (int k = 0; k < m; ++k) {
      if (a[j0 + k].reserved == nullptr) { set_err("internal: a round of nets with and without LN"); return OPRL_ERR_STATE; }
      v[k] = ln_view_of(a[j0 + k]);
    }
    RC(profiled(0, st, [&] { return launch_mlp_slice_multi_ln(a + j0, v, m, st); }));
  }
  return OPRL_OK;
}

}  // namespace

int launch(const MlpArgs& a0, int width, hipStream_t st) {
  if (a0.reserved != nullptr) {
    if (width != kLnWidth) { set_err("internal: an LN net pass at width %d", width); return OPRL_ERR_STATE; }
    const LnView v = ln_view_of(a0);
    RC(profiled(0, st, [&] { return launch_mlp_slice_ln(a0, v, st); }));
    return OPRL_OK;
  }
  MlpArgs a = a0;
  const bool tp = takes_cluster(a, width);
  if (tp) RC(draw_tag(a, st));
  RC(profiled(0, st, [&] { return tp ? launch_mlp_slice_tp(a, st) : launch_mlp_slice(a, width, st); }));
  return OPRL_OK;
}

int launch_round(oprl_learner* h, MlpArgs* a, int n, int width, hipStream_t st) {
  // measured: the event fork/join costs more than it saves for 2 nets (TD3 8.8k -> 7.7k/s),
  // pays for the 5 quantile critics of TQC (673 -> 1206/s)
  if (n > 0 && a[0].reserved != nullptr) return launch_ln_round(a, n, width, st);
  if (n == 2) return launch_pair(h, a, width, st);
  if (n > 2 && n <= kMaxMulti) return launch_few(h, a, n, width, st);
  if (n > kMaxMulti && h->tp_generic_on) {
    // more nets than a multi launch takes (REDQ's ensemble): in pairs on the caller's stream, each pair one k_mlp_slice_tp2
    // launch (side by side, each net in its own exchange area, while both fit the chip).  Not on the side streams: every
    // cluster launch of a learner exchanges through the same area of xbuf, and two such launches running at once would
    // overwrite each other's granules
    for (int j0 = 0; j0 < n; j0 += 2) RC(j0 + 1 == n ? launch(a[j0], width, st) : launch_pair(h, a + j0, width, st));
    return OPRL_OK;
  }
  if (n <= 2 || !h->have_side) {
    for (int j = 0; j < n; ++j) RC(launch(a[j], width, st));
    return OPRL_OK;
  }
  // net 0 on the caller's stream, the others on side streams forked from / joined back into it, so independent nets
  // overlap on the GPU (each k_mlp_slice launch occupies only ceil(B/16) of the 256 CUs)
  HIPC(hipEventRecord(h->ev_fork, st));
  for (int j = 1; j < n; ++j) HIPC(hipStreamWaitEvent(h->side[j], h->ev_fork, 0));
  for (int j = 0; j < n; ++j) {
    hipStream_t sj = j == 0 ? st : h->side[j];
    RC(launch(a[j], width, sj));
    if (j > 0) HIPC(hipEventRecord(h->ev_join[j], sj));
  }
  for (int j = 1; j < n; ++j) HIPC(hipStreamWaitEvent(st, h->ev_join[j], 0));
  return OPRL_OK;
}

}  // namespace oprl_host
