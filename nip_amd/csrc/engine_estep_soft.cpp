// engine_estep_soft.cpp -- the batched e_step under soft (likelihood)
// evidence: nipamd_estep_soft_partial / nipamd_estep_soft /
// nipamd_estep_soft_host over chain_estep_soft_kernel (estep_soft.hip).  The
// evidence columns are nipamd_fb_soft's (engine_soft.cpp): the hard ones (state
// codes) followed by the soft ones (likelihood vectors).  The kernel writes
// one wide slab row per sequence; the fixed-order tree sums them into the wide
// route's partial (engine_estep.cpp run_slab_chunks, tag (0, 0, 1)), which
// nipamd_estep_finalize projects onto the em_learn layout unchanged.
//
// The reference has no e_step over uncertain series, so its verdict on a
// leading run of missing observations and its rejection of a positive ll are
// not applied here: weights above 1 make a positive ll legitimate.
#include <algorithm>

#include "engine_internal.h"

using namespace nipamd::eng;

namespace {

// The verdict on a request -- the arguments, then the scope -- decided on the
// host before anything touches the device, in the soft entry points' order
// (soft_check).  obs / lik / out: the caller's buffers (device or host), only
// tested for NULL.  Fills the route, the shape, the columns' roles and the
// count-table rows of a.
int estep_soft_check(const char* what, nipamd_model* mm, const void* obs, int n_obs, const int* obs_vars,
                     const void* lik, int n_soft, const int* soft_vars, int B, int T, const void* out,
                     nipamd::EstepSoftArgs& a, Route& r) {
  const bool null = !out || (n_obs > 0 && !obs) || (n_soft > 0 && (!lik || !soft_vars));
  if (int rc = check_var_lists(what, mm, null, "NULL model, observations, likelihoods, variables or counts",
                               B < 1 || T < 1 || n_soft < 0, "bad arguments (B >= 1, T >= 1)", n_obs, obs_vars, 0,
                               nullptr))
    return rc;
  if (int rc = soft_evidence_columns(what, mm, "the e_step under soft evidence",
                                     "the operator chain and the general engine take hard evidence only; ", n_obs,
                                     obs_vars, n_soft, soft_vars, a, r))
    return rc;
  const auto& P = mm->m.chain;
  if (P.joint)
    return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": the model has a joint interface (several interface "
                                              "variables); the e_step under soft evidence takes one interface "
                                              "variable");
  for (int i = 0; i < r.ncol; i++)
    if (r.emit[i] >= (int)P.emits.size())
      return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": evidence on the interface variable itself; the "
                                                "e_step under soft evidence takes evidence on its leaf children");
  if (!estep_wide_plan(mm->m))
    return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": no wide chain e_step plan for this model (one "
                                              "interface variable of at most 64 states, 1..4 leaf children, "
                                              "independent hidden parents)");
  a.B = B; a.T = T;
  a.lik_bstride = (long)T * a.lik_tstride;
  a.R = estep_rows(P);
  a.slab_size = nipamd::estep_wide_slab(P.N, a.R);
  a.n_unobs = 0;
  for_each_child(P, r, (int)P.emits.size(), [&](int k, int row, int slot) {
    if (slot >= 0) a.hrow[slot] = row;
    else a.urow[a.n_unobs++] = row + P.emits[k].M;
  });
  const int rc = nipamd::chain_estep_soft_prepare(a);
  if (rc == nipamd::kLaunchRefused)
    return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": the evidence tables, the transition, the staging "
                                              "rows and the count tables need " +
                                              std::to_string(nipamd::chain_estep_soft_lds_bytes(a)) +
                                              " bytes of LDS, more than a CU holds");
  if (rc) return launch_fail(rc, "chain_estep_soft_kernel");
  return 0;
}

// sequences per launch: a power of two (the chunk trees are subtrees of the
// batch's tree) whose slab rows and alpha^ scratch stay within ~4 GB
long estep_soft_chunk(int N, int S, int T) {
  const size_t per_seq = (size_t)S * sizeof(double) + nipamd::chain_soft_scratch_bytes(N, 1, T);
  return estep_pow2_chunk(per_seq, (size_t)4 << 30, 1, estep_chunk_limit());
}

int estep_soft_partial_impl(const char* what, nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
                            const double* d_lik, int n_soft, const int* soft_vars, int B, int T, double* d_partial,
                            double* d_ll, uint32_t* d_status, void* stream) {
  nipamd::EstepSoftArgs a{};
  Route r;
  if (int rc = estep_soft_check(what, mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, d_partial, a, r))
    return rc;
  const auto& P = mm->m.chain;
  const long chunk = std::min<long>(B, estep_soft_chunk(P.N, a.slab_size, T));
  ReqTables* rt = nullptr;
  auto prepare = [&] {
    if (int rc = ensure_tables(mm)) return rc;           // (the GPU fold of a fold_gpu plan included)
    return ensure_req_tables(mm, r, &rt);
  };
  return wide_slab_chunks(mm, a.slab_size, chunk, nipamd::chain_soft_scratch_bytes(P.N, chunk, T), B, d_partial,
                          (hipStream_t)stream, prepare, [&](long b0, long nb, double* slab) {
                            const DevState* d = dev_of(mm);
                            set_cols(a, P, r, *rt, n_obs);
                            set_obs_view(a, n_obs > 0 ? d_obs : nullptr, n_obs, T, b0);
                            a.lik = n_soft > 0 ? d_lik + b0 * a.lik_bstride : nullptr;
                            a.A = d->A64; a.sall = d->sall64; a.pi = d->pi64;
                            a.S = d->S;
                            a.B = nb;
                            a.slab = slab;
                            a.ll = d_ll ? d_ll + b0 : nullptr;
                            a.status = d_status ? d_status + b0 : nullptr;
                            return launched(nipamd::chain_estep_soft_launch(a, (hipStream_t)stream),
                                            "chain_estep_soft_kernel");
                          });
}

}  // namespace

extern "C" {

int nipamd_estep_soft_partial(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
                              const double* d_lik, int n_soft, const int* soft_vars, int B, int T, double* d_partial,
                              double* d_ll, uint32_t* d_status, void* stream) {
  return estep_soft_partial_impl("estep_soft_partial", mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T,
                                 d_partial, d_ll, d_status, stream);
}

int nipamd_estep_soft(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars, const double* d_lik,
                      int n_soft, const int* soft_vars, int B, int T, double* d_counts, double* d_ll,
                      uint32_t* d_status, void* stream) {
  {
    nipamd::EstepSoftArgs a{};
    Route r;
    if (int rc = estep_soft_check("estep_soft", mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, d_counts,
                                  a, r))
      return rc;
  }
  const int S = nipamd_estep_partial_size(mm);
  if (S < 0) return fail(NIPAMD_ERROR_UNSUPPORTED, "estep_soft: no e_step plan for this model under the selected engine");
  if (int rc = ensure_device(mm)) return rc;
  DevState* d = dev_of(mm);
  if (d->R_size < S) {
    (void)hipFree(d->R);
    d->R = nullptr;
    d->R_size = 0;
    HIP_OK(hipMalloc(&d->R, (size_t)S * sizeof(double)));
    d->R_size = S;
  }
  if (int rc = estep_soft_partial_impl("estep_soft", mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, d->R,
                                       d_ll, d_status, stream))
    return rc;
  return nipamd_estep_finalize(mm, d->R, d_counts, stream);
}

// host-buffer form: the verdict first (nothing is allocated for a refusal),
// then host_call with the likelihoods copied in around it
int nipamd_estep_soft_host(nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars, const double* lik,
                           int n_soft, const int* soft_vars, int B, int T, double* counts, double* ll,
                           uint32_t* status) {
  size_t W = 0;
  {
    nipamd::EstepSoftArgs a{};
    Route r;
    if (int rc = estep_soft_check("estep_soft", mm, obs, n_obs, obs_vars, lik, n_soft, soft_vars, B, T, counts, a, r))
      return rc;
    W = (size_t)a.lik_tstride;
  }
  const size_t P = (size_t)nipamd::param_size(mm->m);
  const size_t nob = (size_t)B * T * (n_obs > 0 ? n_obs : 1);
  const size_t nli = (size_t)B * T * W;
  return host_call(n_obs > 0 ? obs : nullptr, nob, counts, P, true, ll, status, (size_t)B,
                   [&](int32_t* d_obs, double* d_cnt, double* d_ll, uint32_t* d_st) {
                     return with_lik(lik, nli, [&](const double* d_lik) {
                       return nipamd_estep_soft(mm, d_obs, n_obs, obs_vars, d_lik, n_soft, soft_vars, B, T, d_cnt, d_ll,
                                                d_st, nullptr);
                     });
                   });
}

}  // extern "C"
