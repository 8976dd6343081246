// engine_soft.cpp -- batched soft (likelihood) evidence: the nipamd_fb_soft /
// nipamd_filter_soft entry points over chain_soft_kernel (soft.hip).  The
// request's evidence columns are the hard ones (state codes) followed by the
// soft ones (likelihood vectors); the chain plan routes them together and the
// model's tables are looked up per call, as every entry point does
// (engine_internal.h).
#include <algorithm>

#include "engine_internal.h"

using namespace nipamd::eng;

namespace {

static_assert(NIPAMD_STATUS_BAD_EVIDENCE == nipamd::kSoftBadEvidence, "include/nip_amd.h and chain_kernels.h disagree");

// The verdict on a request -- the arguments, then the scope -- decided on the
// host before anything touches the device (as stream_check and mlss_check).
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
  for (int i = 0; i < n_soft; i++)
    if (soft_vars[i] < 0 || soft_vars[i] >= (int)mm->m.vars.size())
      return fail(NIP_ERROR_INVALID_ARGUMENT, std::string(what) + ": bad soft-evidence variable");
  if (int rc = chain_scope(mm, what, "soft evidence",
                           "the operator chain and the general engine take hard evidence only; "))
    return rc;
  const auto& P = mm->m.chain;
  // the hard columns, then the soft ones: one evidence list for the plan
  std::vector<int> all(obs_vars, obs_vars + n_obs);
  all.insert(all.end(), soft_vars, soft_vars + n_soft);
  for (int i = 0; i < n_obs; i++)
    for (int j = 0; j < n_soft; j++)
      if (obs_vars[i] == soft_vars[j])
        return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": a variable is listed as hard and as soft evidence");
  std::string why;
  if (!route_request(mm, (int)all.size(), all.data(), 0, nullptr, r, why))
    return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": " + why);
  // the query: distinct current-slice interface variables, at least one
  bool is_if = n_query >= 1;
  if (!P.joint) {
    is_if = n_query == 1 && query[0] == P.v_cur;
    a.nq = 0;
    *width = P.N;
  } else {
    is_if = is_if && n_query <= nipamd::kViterbiMaxQuery &&
            interface_digits(mm, n_query, query, a.qstride, a.qcard, width);
    a.nq = n_query;
  }
  if (!is_if)
    return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": the query is not a non-empty list of distinct "
                                              "current-slice interface variables (at most " +
                                              std::to_string(nipamd::kViterbiMaxQuery) + ")");
  a.B = B; a.T = T; a.N = P.N;
  a.ncol = r.ncol; a.nhard = n_obs;
  int W = 0;
  for (int i = 0; i < r.ncol; i++) {
    a.M[i] = P.emit(r.emit[i]).M;
    a.col[i] = r.col[i];
    if (i >= n_obs) { a.col[i] = W; W += a.M[i]; }         // a soft column: where its weights start in a row
  }
  a.lik_tstride = W;
  a.lik_bstride = (long)T * W;
  a.post_tstride = *width;
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
  int col[4];
  std::copy(a.col, a.col + 4, col);
  set_cols(a, P, r, *rt);
  std::copy(col, col + 4, a.col);                        // the soft columns' offsets (soft_check)
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
                     DevBufs db;
                     double* d_lik = nullptr;
                     if (int rc = db.alloc(&d_lik, nli)) return rc;
                     if (nli) HIP_OK(hipMemcpy(d_lik, lik, nli * sizeof(double), hipMemcpyHostToDevice));
                     const int rc = soft_impl(what, mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, n_query,
                                              query, d_post, d_ll, d_st, nullptr, filt);
                     if (rc == 0) HIP_OK(hipDeviceSynchronize());   // d_lik is freed on return
                     return rc;
                   });
}

}  // namespace

extern "C" {

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
