// engine_soft.cpp -- batched soft (likelihood) evidence: the nipamd_fb_soft /
// nipamd_filter_soft entry points over chain_soft_kernel (soft.hip) and
// nipamd_mlss_soft over chain_viterbi_soft_kernel (viterbi_soft.hip).  The
// request's evidence columns are the hard ones (state codes) followed by the
// soft ones (likelihood vectors); the chain plan routes them together and the
// model's tables are looked up per call, as every entry point does
// (engine_internal.h).
#include "engine_internal.h"

using namespace nipamd::eng;

namespace {

static_assert(NIPAMD_STATUS_BAD_EVIDENCE == nipamd::kSoftBadEvidence, "include/nip_amd.h and chain_kernels.h disagree");

// The verdict on a request -- the arguments, then the scope -- decided on the
// host before anything touches the device (as stream_check and mlss_check;
// soft_columns holds what stream_check decides likewise).
// obs / lik / post: the caller's buffers (device or host), only tested for
// NULL.  Fills the route, the shape, the columns' roles and the query digits
// of a, and the rows' width.
int soft_check(const char* what, nipamd_model* mm, const void* obs, int n_obs, const int* obs_vars, const void* lik,
               int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query, const void* post,
               nipamd::SoftArgs& a, Route& r, int* width) {
  const bool null = !post || (n_obs > 0 && !obs) || (n_soft > 0 && (!lik || !soft_vars));
  if (int rc = check_var_lists(what, mm, null, "NULL model, observations, likelihoods, variables or rows",
                               B < 1 || T < 1 || n_soft < 0, "bad arguments (B >= 1, T >= 1)", n_obs, obs_vars, n_query,
                               query))
    return rc;
  if (int rc = soft_columns(what, mm, "soft evidence",
                            "the operator chain and the general engine take hard evidence only; ", n_obs, obs_vars,
                            n_soft, soft_vars, n_query, query, a, r, width))
    return rc;
  a.B = B; a.T = T;
  a.lik_bstride = (long)T * a.lik_tstride;
  a.post_bstride = (long)T * *width;
  const int rc = nipamd::chain_soft_prepare(a);
  if (rc == nipamd::kLaunchRefused)
    return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": the evidence tables, the transition and the staging "
                                              "rows need " + std::to_string(nipamd::chain_soft_lds_bytes(a)) +
                                              " bytes of LDS, more than a CU holds");
  if (rc) return launch_fail(rc, "chain_soft_kernel");
  return 0;
}

// chain_soft_kernel over the chain plan's tables, asynchronous on stream
int soft_impl(const char* what, nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
              const double* d_lik, int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query,
              double* d_post, double* d_ll, uint32_t* d_status, void* stream, bool filt) {
  nipamd::SoftArgs a{};
  Route r;
  int width = 0;
  if (int rc = soft_check(what, mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, n_query, query, d_post, a, r,
                          &width))
    return rc;
  const auto& P = mm->m.chain;
  if (int rc = ensure_tables(mm)) return rc;             // (the GPU fold of a fold_gpu plan included)
  ReqTables* rt = nullptr;
  if (int rc = ensure_req_tables(mm, r, &rt)) return rc;
  if (!filt)
    if (int rc = ensure_scratch(mm, nipamd::chain_soft_scratch_bytes(P.N, B, T))) return rc;
  const DevState* d = dev_of(mm);
  set_cols(a, P, r, *rt, n_obs);
  set_obs_view(a, n_obs > 0 ? d_obs : nullptr, n_obs, T);
  a.lik = n_soft > 0 ? d_lik : nullptr;
  a.A = d->A64; a.sall = d->sall64; a.pi = d->pi64;
  a.S = filt ? nullptr : d->S;
  a.post = d_post;
  a.ll = d_ll; a.status = d_status;
  a.filter = filt ? 1 : 0;
  return launched(nipamd::chain_soft_launch(a, (hipStream_t)stream), "chain_soft_kernel");
}

// host-buffer form: the verdict first (nothing is allocated for a refusal),
// then host_call with the likelihoods copied in around it
int soft_host_impl(const char* what, nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars,
                   const double* lik, int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query,
                   double* post, double* ll, uint32_t* status, bool filt) {
  int width = 0;
  size_t W = 0;
  {
    nipamd::SoftArgs a{};
    Route r;
    if (int rc = soft_check(what, mm, obs, n_obs, obs_vars, lik, n_soft, soft_vars, B, T, n_query, query, post, a, r,
                            &width))
      return rc;
    W = (size_t)a.lik_tstride;
  }
  const size_t nob = (size_t)B * T * (n_obs > 0 ? n_obs : 1);
  const size_t npo = (size_t)B * T * width;
  const size_t nli = (size_t)B * T * W;
  return host_call(n_obs > 0 ? obs : nullptr, nob, post, npo, false, ll, status, (size_t)B,
                   [&](int32_t* d_obs, double* d_post, double* d_ll, uint32_t* d_st) {
                     return with_lik(lik, nli, [&](const double* d_lik) {
                       return soft_impl(what, mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, n_query, query,
                                        d_post, d_ll, d_st, nullptr, filt);
                     });
                   });
}

// mlss_soft: the verdict on a request, as soft_check gives it with mlss's query
// rule (exactly the interface) in place of the rows' -- the arguments, the
// soft variables, the scope, a variable both hard and soft, the route, the
// query, the LDS.  Fills the route, the shape, the columns' roles and the
// path's columns of a.
int mlss_soft_check(nipamd_model* mm, const void* obs, int n_obs, const int* obs_vars, const void* lik, int n_soft,
                    const int* soft_vars, int B, int T, int n_query, const int* query, const void* path,
                    nipamd::ViterbiSoftArgs& a, Route& r) {
  const char* what = "mlss_soft";
  const bool null = !path || (n_obs > 0 && !obs) || (n_soft > 0 && (!lik || !soft_vars));
  if (int rc = check_var_lists(what, mm, null, "NULL model, observations, likelihoods, variables or path",
                               B < 1 || T < 1 || n_soft < 0, "bad arguments (B >= 1, T >= 1)", n_obs, obs_vars, n_query,
                               query))
    return rc;
  if (int rc = soft_evidence_columns(what, mm, "the most likely state sequence", "", n_obs, obs_vars, n_soft, soft_vars,
                                     a, r))
    return rc;
  if (int rc = interface_query(what, mm, n_query, query, &a.nq, a.qstride, a.qcard)) return rc;
  a.B = B; a.T = T;
  a.lik_bstride = (long)T * a.lik_tstride;
  a.path_bstride = (long)T * a.nq; a.path_tstride = a.nq;
  const int rc = nipamd::chain_viterbi_soft_prepare(a);
  if (rc == nipamd::kLaunchRefused)
    return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": the evidence tables and the staging rows need " +
                                              std::to_string(nipamd::chain_viterbi_soft_lds_bytes(a)) +
                                              " bytes of LDS, more than a CU holds");
  if (rc) return launch_fail(rc, "chain_viterbi_soft_kernel");
  return 0;
}

// chain_viterbi_soft_kernel over the chain plan's tables, asynchronous on
// stream: chunks of mlss_chunk sequences over the same back-pointer scratch
int mlss_soft_impl(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars, const double* d_lik,
                   int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query, int32_t* d_path,
                   double* d_logp, uint32_t* d_status, void* stream) {
  nipamd::ViterbiSoftArgs a{};
  Route r;
  if (int rc = mlss_soft_check(mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, n_query, query, d_path, a, r))
    return rc;
  const auto& P = mm->m.chain;
  if (int rc = ensure_tables(mm)) return rc;             // (the GPU fold of a fold_gpu plan included)
  ReqTables* rt = nullptr;
  if (int rc = ensure_req_tables(mm, r, &rt)) return rc;
  const long chunk = mlss_chunk(P.N, T);
  if (int rc = ensure_scratch(mm, nipamd::chain_viterbi_scratch_bytes(P.N, B < chunk ? B : chunk, T))) return rc;
  DevState* d = dev_of(mm);
  set_cols(a, P, r, *rt, n_obs);
  a.A = d->A64; a.u0 = rt->u0;
  a.bp = reinterpret_cast<unsigned long long*>(d->S);
  for (long b0 = 0; b0 < B; b0 += chunk) {
    a.B = B - b0 < chunk ? B - b0 : chunk;
    set_obs_view(a, n_obs > 0 ? d_obs : nullptr, n_obs, T, b0);
    a.lik = n_soft > 0 ? d_lik + b0 * a.lik_bstride : nullptr;
    a.path = d_path + b0 * a.path_bstride;
    a.logp = d_logp ? d_logp + b0 : nullptr;
    a.status = d_status ? d_status + b0 : nullptr;
    if (int rc = nipamd::chain_viterbi_soft_launch(a, (hipStream_t)stream))
      return launch_fail(rc, "chain_viterbi_soft_kernel");
  }
  return 0;
}

}  // namespace

extern "C" {

int nipamd_mlss_soft(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars, const double* d_lik,
                     int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query, int32_t* d_path,
                     double* d_logp, uint32_t* d_status, void* stream) {
  return mlss_soft_impl(mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, n_query, query, d_path, d_logp,
                        d_status, stream);
}

// host-buffer form: the verdict first (nothing is allocated for a refusal),
// then host_call with the likelihoods copied in around it
int nipamd_mlss_soft_host(nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars, const double* lik,
                          int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query,
                          int32_t* path, double* logp, uint32_t* status) {
  size_t W = 0, nq = 0;
  {
    nipamd::ViterbiSoftArgs a{};
    Route r;
    if (int rc = mlss_soft_check(mm, obs, n_obs, obs_vars, lik, n_soft, soft_vars, B, T, n_query, query, path, a, r))
      return rc;
    W = (size_t)a.lik_tstride;
    nq = (size_t)a.nq;
  }
  const size_t nob = (size_t)B * T * (n_obs > 0 ? n_obs : 1);
  const size_t npa = (size_t)B * T * nq;
  const size_t nli = (size_t)B * T * W;
  return host_call(n_obs > 0 ? obs : nullptr, nob, path, npa, false, logp, status, (size_t)B,
                   [&](int32_t* d_obs, int32_t* d_path, double* d_lp, uint32_t* d_st) {
                     return with_lik(lik, nli, [&](const double* d_lik) {
                       return mlss_soft_impl(mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, n_query, query,
                                             d_path, d_lp, d_st, nullptr);
                     });
                   });
}

int nipamd_fb_soft(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars, const double* d_lik,
                   int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query, double* d_post,
                   double* d_ll, uint32_t* d_status, void* stream) {
  return soft_impl("fb_soft", mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, n_query, query, d_post, d_ll,
                   d_status, stream, false);
}

int nipamd_filter_soft(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars, const double* d_lik,
                       int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query, double* d_post,
                       double* d_ll, uint32_t* d_status, void* stream) {
  return soft_impl("filter_soft", mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, n_query, query, d_post,
                   d_ll, d_status, stream, true);
}

int nipamd_fb_soft_host(nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars, const double* lik,
                        int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query, double* post,
                        double* ll, uint32_t* status) {
  return soft_host_impl("fb_soft", mm, obs, n_obs, obs_vars, lik, n_soft, soft_vars, B, T, n_query, query, post, ll,
                        status, false);
}

int nipamd_filter_soft_host(nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars, const double* lik,
                            int n_soft, const int* soft_vars, int B, int T, int n_query, const int* query, double* post,
                            double* ll, uint32_t* status) {
  return soft_host_impl("filter_soft", mm, obs, n_obs, obs_vars, lik, n_soft, soft_vars, B, T, n_query, query, post, ll,
                        status, true);
}

}  // extern "C"
