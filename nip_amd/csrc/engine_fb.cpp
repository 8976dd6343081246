// engine_fb.cpp -- forward_backward_inference, forward_inference and mlss:
// the launch sites of the interface-chain kernels and of the derived
// marginals, and the hand-over to the operator chain and the general engine
// (engine_internal.h).
#include "engine_internal.h"

using namespace nipamd::eng;

namespace {

// the 16-state kernels' arguments (chain_kernels.hip, chain_mfma.hip, chain_ckpt.hip)
void fill_narrow(nipamd::ChainArgs& a, nipamd_model* mm, const Route& r, const ReqTables* rt,
                 const int32_t* d_obs, int n_obs, int B, int T) {
  const DevState* d = dev_of(mm);
  set_obs_view(a, d_obs, n_obs, T);
  if (r.pcol < 0) a.obs = nullptr;
  a.obs_col = r.pcol;
  a.B = B; a.T = T; a.H = T / 2; a.N = mm->m.chain.N; a.M = rt->M0;
  a.A = d->A; a.Etab = rt->Etab16; a.pi = d->pi; a.ts = rt->ts16; a.S = d->S;
}

// One launch of the chain kernel `kind` for route r: the interface
// variable's marginals (smoothed, or filtered) into dst rows (dbs / dts /
// doff), or only ll / status when dst is null.
int launch_cur(nipamd_model* mm, const Route& r, ReqTables* rt, int kind, const int32_t* d_obs,
               int n_obs, int B, int T, double* dst, long dbs, int dts, int doff,
               double* d_ll, uint32_t* d_status, void* stream, bool filt) {
  const auto& P = mm->m.chain;
  DevState* d = dev_of(mm);
  hipStream_t st = (hipStream_t)stream;
  if (kind == kMfmaWide) {
    // matrix-core interface chain: N <= 32, up to four observed children
    const int NT = P.N <= 16 ? 1 : 2;
    if (fb_ckw_ok(P, r, rt, filt, dst != nullptr)) {
      if (int rc = ensure_scratch(mm, nipamd::chain_estep_ckw_scratch_bytes(B, T))) return rc;
      nipamd::EMwArgs a{};
      set_obs_view(a, d_obs, n_obs, T);
      set_cols(a, P, r, rt->mtab, rt->mtab_off);
      set_post_view(a, dst, dbs, dts, doff);
      a.tab_rows = rt->mtab_rows;
      a.B = B; a.T = T; a.H = T / 2; a.N = P.N;
      a.A = d->A64; a.pi = d->pi64; a.w = rt->wv; a.S = d->S;
      a.ll = d_ll; a.status = d_status;
      const int lrc = nipamd::chain_fb_ckw_launch(a, chain_proper(P), fb_ckw_vl(), st);
      if (lrc != nipamd::kLaunchRefused) return launched(lrc, "chain_fb_ckw_kernel");
    }
    if (int rc = ensure_scratch(mm, filt ? 64 * sizeof(double) : nipamd::chain_mfma_wide_scratch_bytes(NT, B, T)))
      return rc;
    nipamd::WideMfmaArgs w{};
    set_obs_view(w, d_obs, n_obs, T);
    set_cols(w, P, r, rt->mtab, rt->mtab_off);
    set_post_view(w, dst, dbs, dts, doff);
    w.tab_rows = rt->mtab_rows;
    w.B = B; w.T = T; w.H = filt ? T : T / 2; w.N = P.N;
    w.A = d->A64; w.pi = d->pi64; w.w = rt->wv; w.S = d->S;
    w.ll = d_ll; w.status = d_status;
#ifdef NIPAMD_DIAGNOSTICS
    StampBuf stamps;                                   // [block][4 waves][4]
    const int nblk = (B + 15) / 16;
    if (int rc = stamps.attach(phase_times() && !filt, (size_t)nblk * 16, st, &w.diag)) return rc;
#endif
    if (int rc = nipamd::chain_mfma_wide_launch(w, NT, filt, st)) return launch_fail(rc, "chain_mfma_wide_kernel");
#ifdef NIPAMD_DIAGNOSTICS
    if (int rc = stamps.report(st, report_mfma_wide, nblk)) return rc;
#endif
    return 0;
  }
  if (kind == kWide64 || kind == kWide64Step) {
    // wide interface chain: N <= 64, up to four observed children
    // (kWide64Step: the kernel that rescales at every step, at 33..64 states too)
    if (int rc = ensure_scratch(mm, filt ? 64 * sizeof(double)
                                         : (size_t)(B + 2) * nipamd::chain_scratch_row64(T) * sizeof(double)))
      return rc;
    nipamd::WideArgs w{};
    w.filter = filt ? 1 : 0;
    set_obs_view(w, d_obs, n_obs, T);
    set_cols(w, P, r, *rt);
    set_post_view(w, dst, dbs, dts, doff);
    w.B = B; w.T = T; w.H = filt ? 0 : T / 2; w.N = P.N;
    w.A = d->A64; w.pi = d->pi64; w.s = d->sall64; w.S = d->S;
    w.ll = d_ll; w.status = d_status;
#ifdef NIPAMD_DIAGNOSTICS
    StampBuf stamps;                                   // chain_wide4: [block][16]
    if (int rc = stamps.attach(phase_times() && P.N > 32 && kind == kWide64, (size_t)B * 16, st, &w.diag)) return rc;
#endif
    if (int rc = nipamd::chain_wide_launch(w, st, kind == kWide64Step)) return launch_fail(rc, "wide chain kernel");
#ifdef NIPAMD_DIAGNOSTICS
    if (int rc = stamps.report(st, report_wide4, (long)B)) return rc;
#endif
    return 0;
  }
  if (kind != kNarrowMfma && kind != kNarrowDpp)
    return fail(NIPAMD_ERROR_UNSUPPORTED, "no interface-chain kernel fits this request");
  if (int rc = ensure_scratch(mm, nipamd::chain_scratch_bytes(B, T))) return rc;
  nipamd::ChainArgs a{};
  fill_narrow(a, mm, r, rt, d_obs, n_obs, B, T);
  set_post_view(a, dst, dbs, dts, doff);
  a.ll = d_ll;
  a.status = d_status;
#ifdef NIPAMD_DIAGNOSTICS
  StampBuf stamps, waves;             // [block][24]; chain_ckpt.hip's per-wave stamps [block][8 waves][5]
  const int nblk = (B + 15) / 16;
  const bool want = kind == kNarrowMfma && phase_times();
  unsigned long long* phases = nullptr;               // the kernel takes them in a.counts
  if (int rc = stamps.attach(want, (size_t)nblk * 24, st, &phases)) return rc;
  if (int rc = waves.attach(want, (size_t)nblk * 40, st, &a.diag)) return rc;
  a.counts = reinterpret_cast<double*>(phases);
#endif
  const int rc = kind == kNarrowMfma ? nipamd::chain_fb_mfma_launch(a, st) : nipamd::chain_fb_launch(a, st);
#ifdef NIPAMD_DIAGNOSTICS
  if (int frc = stamps.report(st, report_phases, nblk)) return frc;
  if (int frc = waves.report(st, report_ckpt_waves, nblk)) return frc;
#endif
  return launched(rc, kind == kNarrowMfma ? "chain_fb_mfma_kernel" : "chain_kernel");
}

// Joint interface, smoothing, every query one of the interface's current-slice
// variables: chain_fb_ckpt_kernel writes their marginals itself (digit sums of
// the normalised joint posterior, chain_ckpt.hip norm_store) instead of the
// joint posterior plus one project_kernel pass per variable.  *taken = false
// when the checkpoint kernel does not take the request (the caller falls back).
int launch_joint_marginals(nipamd_model* mm, const Route& r, ReqTables* rt, const int32_t* d_obs,
                           int n_obs, int B, int T, int n_query, const int* query, double* d_post,
                           double* d_ll, uint32_t* d_status, void* stream, bool* taken) {
  *taken = false;
  const auto& P = mm->m.chain;
  if (!P.joint || P.N > 16 || n_query < 1 || n_query > 4) return 0;
  nipamd::ChainArgs a{};
  int stride = 0;
  for (int i = 0; i < n_query; i++) {
    const int kind = query_kind(P, query[i]);
    if (kind < 700 || kind >= 1000) return 0;
    const int k = kind - 700;
    int st = 1;
    for (int j = 0; j < k; j++) st *= mm->m.vars[P.jcur[j]].card;
    const int card = mm->m.vars[P.jcur[k]].card;
    a.proj_off[i] = stride;
    a.proj_card[i] = card;
    for (int s = 0; s < 16; s++) a.proj_digit[i][s] = (signed char)(s < P.N ? (s / st) % card : -1);
    stride += card;
  }
  a.nproj = n_query;
  if (int rc = ensure_scratch(mm, nipamd::chain_scratch_bytes(B, T))) return rc;
  fill_narrow(a, mm, r, rt, d_obs, n_obs, B, T);
  set_post_view(a, d_post, (long)T * stride, stride, 0);
  a.ll = d_ll;
  a.status = d_status;
  const int rc = nipamd::chain_fb_ckpt_launch(a, (hipStream_t)stream);
  if (rc == -2) return 0;                            // not taken: the next kernel serves it
  if (rc) return launch_fail(rc, "chain_fb_ckpt_kernel");
  *taken = true;
  return 0;
}

// forward_backward_inference (filt = false) / forward_inference (filt = true).
// The interface variable's marginals come from the chain kernels; every
// other queried variable's are derived from them (derive.hip), with the
// forward messages of a filter pass when a hidden parent is smoothed.
int fb_impl(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
            int B, int T, int n_query, const int* query, double* d_post,
            double* d_ll, uint32_t* d_status, void* stream, bool filt) {
  if (!mm || B < 0 || T < 1 || (n_obs > 0 && (!d_obs || !obs_vars)) || (n_query > 0 && (!query || !d_post)))
    return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  for (int i = 0; i < n_query; i++)
    if (query[i] < 0 || query[i] >= (int)mm->m.vars.size()) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad query variable");
  if (B == 0) return 0;
  Route r;
  std::string why;
  ChainKernel kk = kNoChain;
  ReqTables* rt = nullptr;
  if (mm->engine != NIPAMD_ENGINE_JTREE && route_request(mm, n_obs, obs_vars, n_query, query, r, why)) {
    if (int rc = ensure_tables(mm)) return rc;
    if (int rc = ensure_req_tables(mm, r, &rt)) return rc;
    kk = pick_kernel(mm, r, rt, T, filt);
    // smoothed hidden parents also need the forward messages of a filter pass
    for (int i = 0; i < n_query && kk != kNoChain && !filt; i++)
      if (query_kind(mm->m.chain, query[i]) >= 1000 && pick_kernel(mm, r, rt, T, true) == kNoChain) kk = kNoChain;
    if (kk == kNoChain) why = "sequence too long for the interface-chain kernels' LDS-resident codes";
  }
  if (kk == kNoChain && mm->engine == NIPAMD_ENGINE_AUTO) {
    // the evidence-indexed interface chain (opchain.h): the slice as one K x K
    // operator per evidence combination, K <= 16 joint interface states
    // (automatic engine choice only: NIPAMD_ENGINE_CHAIN is the chain plan's
    // kernels, NIPAMD_ENGINE_JTREE the general engine)
    std::string why2;
    if (nipamd::op_supported(mm, n_obs, obs_vars, n_query, query, why2) &&
        nipamd::op_fits(mm, n_obs, obs_vars, T)) {
      if (int rc = ensure_device(mm)) return rc;
      const auto& out = mm->m.outgoing;
      std::string err;
      int K = 0;
      if (n_query == 1 && out.size() == 1) {           // the interface variable itself: straight into its rows
        const int card = mm->m.vars[query[0]].card;
        const int rc = nipamd::op_fb(mm, d_obs, n_obs, obs_vars, B, T, d_post, (long)T * card, card, 0, d_ll,
                                     d_status, stream, filt, &K, err);
        return rc ? fail(rc, err) : 0;
      }
      long stride = 0;
      for (int i = 0; i < n_query; i++) stride += mm->m.vars[query[i]].card;
      long Kj = 1;
      for (int v : out) Kj *= mm->m.vars[v].card;
      if (int rc = ensure_q(mm, (size_t)B * T * Kj * sizeof(double))) return rc;
      double* q = dev_of(mm)->Q;
      if (int rc = nipamd::op_fb(mm, d_obs, n_obs, obs_vars, B, T, q, (long)T * Kj, (int)Kj, 0, d_ll, d_status,
                                 stream, filt, &K, err))
        return fail(rc, err);
      long off = 0;
      for (int i = 0; i < n_query; i++) {
        nipamd::DeriveArgs g{};
        g.kind = nipamd::kDeriveProject;
        g.filter = filt ? 1 : 0;
        g.B = B; g.T = T; g.N = (int)Kj;
        g.cur = q; g.cur_bstride = (long)T * Kj; g.cur_tstride = (int)Kj;
        g.alpha = q; g.al_bstride = g.cur_bstride; g.al_tstride = g.cur_tstride;
        g.out = d_post; g.out_bstride = (long)T * stride; g.out_tstride = (int)stride; g.out_off = (int)off;
        g.prev_stride = 1;
        for (size_t j = 0; j < out.size() && out[j] != query[i]; j++) g.prev_stride *= mm->m.vars[out[j]].card;
        g.prev_card = mm->m.vars[query[i]].card;
        g.child_col = -1;
        if (int rc = nipamd::derive_launch(g, (hipStream_t)stream))
          return launch_fail(rc, "derive_kernel");
        off += g.prev_card;
      }
      return 0;
    }
  }
  if (kk == kNoChain) {
    // the general join-tree engine (jtree.hip): any slice, any T
    if (mm->engine == NIPAMD_ENGINE_CHAIN) return fail(NIPAMD_ERROR_UNSUPPORTED, why);
    return nipamd::jt_fb(mm, d_obs, n_obs, obs_vars, B, T, n_query, query, d_post, d_ll, d_status,
                         stream, filt);
  }
  if (!filt && kk == kNarrowMfma && mm->m.chain.joint) {
    bool taken = false;
    if (int rc = launch_joint_marginals(mm, r, rt, d_obs, n_obs, B, T, n_query, query, d_post, d_ll, d_status,
                                        stream, &taken))
      return rc;
    if (taken) return 0;
  }
  const auto& P = mm->m.chain;
  std::vector<int> kind(n_query), off(n_query);
  int stride = 0, first_cur = -1;
  bool derived = false, fwd_msgs = false;
  for (int i = 0; i < n_query; i++) {
    kind[i] = query_kind(P, query[i]);
    off[i] = stride;
    stride += mm->m.vars[query[i]].card;
    if (kind[i] == 0) { if (first_cur < 0) first_cur = i; }
    else { derived = true; fwd_msgs |= kind[i] >= 1000 && !filt; }
  }
  const long pbs = (long)T * stride;
  const int N = P.N;
  const size_t per = (size_t)B * T * N;
  // where the interface marginals live: the first query slot naming the
  // interface variable, or (derived queries only) the work buffer Q
  double* cur = nullptr;
  long cbs = 0;
  int cts = 0;
  double* fwd = nullptr;
  if (derived) {
    const size_t need = (first_cur < 0 ? per : 0) + (fwd_msgs ? per : 0);
    if (need) if (int rc = ensure_q(mm, need * sizeof(double))) return rc;
    double* q = dev_of(mm)->Q;
    if (first_cur < 0) { cur = q; cbs = (long)T * N; cts = N; q += per; }
    else { cur = d_post + off[first_cur]; cbs = pbs; cts = stride; }
    if (fwd_msgs) fwd = q;
  }
  bool first = true;
  for (int i = 0; i < n_query; i++) {
    if (kind[i] != 0) continue;
    if (int rc = launch_cur(mm, r, rt, kk, d_obs, n_obs, B, T, d_post, pbs, stride, off[i],
                            first ? d_ll : nullptr, first ? d_status : nullptr, stream, filt)) return rc;
    first = false;
  }
  if (first)       // no query slot names the interface variable
    if (int rc = launch_cur(mm, r, rt, kk, d_obs, n_obs, B, T, cur, cbs, cts, 0, d_ll, d_status, stream, filt)) return rc;
  if (fwd_msgs)    // the forward messages: a filter pass
    if (int rc = launch_cur(mm, r, rt, pick_kernel(mm, r, rt, T, true), d_obs, n_obs, B, T, fwd, (long)T * N, N, 0,
                            nullptr, nullptr, stream, true))
      return rc;
  if (!derived) return 0;
  DevState* d = dev_of(mm);
  for (int i = 0; i < n_query; i++) {
    if (kind[i] == 0) continue;
    nipamd::DeriveArgs g{};
    g.filter = filt ? 1 : 0;
    g.B = B; g.T = T; g.N = N;
    g.cur = cur; g.cur_bstride = cbs; g.cur_tstride = cts;
    if (fwd) { g.alpha = fwd; g.al_bstride = (long)T * N; g.al_tstride = N; }
    else { g.alpha = cur; g.al_bstride = cbs; g.al_tstride = cts; }
    g.out = d_post; g.out_bstride = pbs; g.out_tstride = stride; g.out_off = off[i];
    g.A = d->A64; g.pi = d->pi64;
    set_obs_view(g, d_obs, n_obs, T);
    set_cols(g, P, r, *rt);
    g.child_col = -1;
    if (kind[i] == 1) {
      g.kind = nipamd::kDerivePrev;
    } else if (kind[i] >= 500 && kind[i] < 1000) {
      // a joint interface's variable: its digit of the joint interface
      // marginal (current slice), or of the derived previous-interface one
      const bool is_prev = kind[i] < 700;
      const int k = kind[i] - (is_prev ? 500 : 700);
      const auto& vs = is_prev ? P.jprev : P.jcur;
      g.kind = is_prev ? nipamd::kDerivePrev : nipamd::kDeriveProject;
      g.prev_stride = 1;
      for (int j = 0; j < k; j++) g.prev_stride *= mm->m.vars[vs[j]].card;
      g.prev_card = mm->m.vars[vs[k]].card;
    } else if (kind[i] < 1000) {
      const int k = kind[i] - 2;
      g.kind = nipamd::kDeriveChild;
      g.child_M = P.emits[k].M;
      g.child_E = d->childE[k];
      for (int c = 0; c < r.ncol; c++) if (r.emit[c] == k) g.child_col = r.col[c];
    } else {
      const int j = kind[i] - 1000;
      if (int rc = ensure_hidden(mm, j)) return rc;
      g.kind = nipamd::kDeriveHidden;
      g.hid_card = mm->m.vars[P.hidden[j]].card;
      g.G = d->G[j];
    }
    if (int rc = nipamd::derive_launch(g, (hipStream_t)stream))
      return launch_fail(rc, "derive_kernel");
  }
  return 0;
}

// host-buffer form of fb_impl (PCIe-inclusive, synchronous)
int fb_host_impl(nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars,
                 int B, int T, int n_query, const int* query, double* post,
                 double* ll, uint32_t* status, bool filt) {
  if (!mm || B < 0 || T < 1 || n_query < 0 || (n_query > 0 && !query) || (n_obs > 0 && (!obs || !obs_vars)))
    return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  for (int i = 0; i < n_query; i++)
    if (query[i] < 0 || query[i] >= (int)mm->m.vars.size()) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad query variable");
  if (B == 0) return 0;
  int stride = 0;
  for (int i = 0; i < n_query; i++) stride += mm->m.vars[query[i]].card;
  const size_t nob = (size_t)B * T * (n_obs > 0 ? n_obs : 1);
  const size_t npo = (size_t)B * T * (stride > 0 ? stride : 1);
  return host_call(n_obs > 0 ? obs : nullptr, nob, stride > 0 ? post : nullptr, npo, false, ll, status, (size_t)B,
                   [&](int32_t* d_obs, double* d_post, double* d_ll, uint32_t* d_st) {
                     return fb_impl(mm, d_obs, n_obs, obs_vars, B, T, n_query, query, d_post, d_ll, d_st, nullptr, filt);
                   });
}

}  // namespace

// Sequences per chain_viterbi_kernel launch: the back-pointer scratch of a
// launch stays within kMlssScratch (8 bytes per sequence and step at N <= 16:
// a config-4 shard, 131072 x 1024, is one launch of exactly this size), and a
// longer batch runs as consecutive launches over the same scratch.  A multiple
// of 16, so every launch but the last fills its blocks.
long nipamd::eng::mlss_chunk(int N, int T) {
  constexpr size_t kMlssScratch = (size_t)1 << 30;
  const size_t per16 = nipamd::chain_viterbi_scratch_bytes(N, 16, T);
  const long c = (long)(kMlssScratch / per16) * 16;
  return c < 16 ? 16 : c;
}

namespace {

// mlss: the verdict on a request -- the arguments, then the scope -- decided on
// the host before anything touches the device.  obs / path: the caller's
// buffers (device or host), only tested for NULL.  Fills the query columns of a
// and the evidence route.
int mlss_check(nipamd_model* mm, const void* obs, int n_obs, const int* obs_vars, int B, int T, int n_query,
               const int* query, const void* path, nipamd::ViterbiArgs& a, Route& r) {
  if (int rc = check_var_lists("mlss", mm, !path || (n_obs > 0 && !obs), "NULL model, observations, variables or path",
                               B <= 0 || T <= 0, "bad arguments", n_obs, obs_vars, n_query, query))
    return rc;
  if (int rc = chain_scope(mm, "mlss", "the most likely state sequence", "")) return rc;
  if (int rc = interface_query("mlss", mm, n_query, query, &a.nq, a.qstride, a.qcard)) return rc;
  std::string why;
  if (!route_request(mm, n_obs, obs_vars, 0, nullptr, r, why)) return fail(NIPAMD_ERROR_UNSUPPORTED, "mlss: " + why);
  return 0;
}

// chain_viterbi_kernel over the chain plan's tables, asynchronous on stream
int mlss_impl(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars, int B, int T,
              int n_query, const int* query, int32_t* d_path, double* d_logp, uint32_t* d_status,
              void* stream) {
  nipamd::ViterbiArgs a{};
  Route r;
  if (int rc = mlss_check(mm, d_obs, n_obs, obs_vars, B, T, n_query, query, d_path, a, r)) return rc;
  const auto& P = mm->m.chain;
  if (int rc = ensure_tables(mm)) return rc;           // (the GPU fold of a fold_gpu plan included)
  ReqTables* rt = nullptr;
  if (int rc = ensure_req_tables(mm, r, &rt)) return rc;
  const int N = P.N;
  const long chunk = mlss_chunk(N, T);
  if (int rc = ensure_scratch(mm, nipamd::chain_viterbi_scratch_bytes(N, B < chunk ? B : chunk, T))) return rc;
  DevState* d = dev_of(mm);
  set_cols(a, P, r, *rt);
  a.A = d->A64; a.u0 = rt->u0;
  a.T = T; a.N = N;
  a.bp = reinterpret_cast<unsigned long long*>(d->S);
  a.path_bstride = (long)T * a.nq; a.path_tstride = a.nq;
  for (long b0 = 0; b0 < B; b0 += chunk) {
    a.B = B - b0 < chunk ? B - b0 : chunk;
    set_obs_view(a, d_obs, n_obs, T, b0);
    a.path = d_path + b0 * a.path_bstride;
    a.logp = d_logp ? d_logp + b0 : nullptr;
    a.status = d_status ? d_status + b0 : nullptr;
    if (int rc = nipamd::chain_viterbi_launch(a, (hipStream_t)stream)) return launch_fail(rc, "chain_viterbi_kernel");
  }
  return 0;
}

}  // namespace

extern "C" {

int nipamd_fb(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
              int B, int T, int n_query, const int* query, double* d_post,
              double* d_ll, uint32_t* d_status, void* stream) {
  return fb_impl(mm, d_obs, n_obs, obs_vars, B, T, n_query, query, d_post, d_ll, d_status, stream, false);
}

int nipamd_filter(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
                  int B, int T, int n_query, const int* query, double* d_post,
                  double* d_ll, uint32_t* d_status, void* stream) {
  return fb_impl(mm, d_obs, n_obs, obs_vars, B, T, n_query, query, d_post, d_ll, d_status, stream, true);
}

int nipamd_fb_host(nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars,
                   int B, int T, int n_query, const int* query, double* post,
                   double* ll, uint32_t* status) {
  return fb_host_impl(mm, obs, n_obs, obs_vars, B, T, n_query, query, post, ll, status, false);
}

int nipamd_filter_host(nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars,
                       int B, int T, int n_query, const int* query, double* post,
                       double* ll, uint32_t* status) {
  return fb_host_impl(mm, obs, n_obs, obs_vars, B, T, n_query, query, post, ll, status, true);
}

int nipamd_mlss(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars, int B, int T,
                int n_query, const int* query, int32_t* d_path, double* d_logp, uint32_t* d_status, void* stream) {
  return mlss_impl(mm, d_obs, n_obs, obs_vars, B, T, n_query, query, d_path, d_logp, d_status, stream);
}

// host-buffer form of nipamd_mlss (copies in and out, synchronous)
int nipamd_mlss_host(nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars, int B, int T,
                     int n_query, const int* query, int32_t* path, double* logp, uint32_t* status) {
  // the verdict on the request first: nothing is allocated for a refusal
  {
    nipamd::ViterbiArgs a{};
    Route r;
    if (int rc = mlss_check(mm, obs, n_obs, obs_vars, B, T, n_query, query, path, a, r)) return rc;
  }
  const size_t nob = (size_t)B * T * (n_obs > 0 ? n_obs : 1);
  const size_t npa = (size_t)B * T * (n_query > 0 ? n_query : 1);
  return host_call(n_obs > 0 ? obs : nullptr, nob, path, npa, false, logp, status, (size_t)B,
                   [&](int32_t* d_obs, int32_t* d_path, double* d_lp, uint32_t* d_st) {
                     return mlss_impl(mm, d_obs, n_obs, obs_vars, B, T, n_query, query, d_path, d_lp, d_st, nullptr);
                   });
}

}  // extern "C"
