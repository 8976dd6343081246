// engine_stream.cpp -- online inference: the nipamd_stream_* entry points over
// chain_stream_kernel (stream.hip) and, for a stream with soft (likelihood)
// evidence columns, chain_stream_soft_kernel (stream_soft.hip).  A stream owns
// the per-sequence state on the device (forward messages, running totals, the
// ring of the pending steps: their raw codes, or their evaluated evidence
// under soft evidence) and the host counters n and pending; the model's tables
// are looked up per call, as every entry point does (engine_internal.h).
#include <algorithm>

#include "engine_internal.h"

using namespace nipamd::eng;

// The opaque handle of the C-ABI (include/nip_amd.h).
struct nipamd_stream {
  nipamd_model* mm = nullptr;
  std::vector<int> obs_vars;    // the hard columns
  std::vector<int> soft_vars;   // the soft columns (empty: chain_stream_kernel serves the stream)
  int B = 0, lag = 0, width = 0;
  int W = 0;                    // doubles of a step's likelihood vectors
  Route r;                      // of the hard columns followed by the soft ones
  nipamd::StreamSoftArgs a{};   // the launch arguments that never change: shape, columns, query digits, state
  void* state = nullptr;        // one device allocation behind a.base .. a.ring, a.ering
  long n = 0;                   // steps consumed
  int pending = 0;              // min(n, lag); 0 after a flush
  bool flushed = false;
};

namespace {

static_assert(NIPAMD_STREAM_CHUNK == nipamd::kStreamChunk && NIPAMD_STREAM_MAX_LAG == nipamd::kStreamMaxLag,
              "include/nip_amd.h and chain_kernels.h disagree");

// The verdict on a stream -- the arguments, then the scope -- decided on the
// host before anything touches the device (as mlss_check; soft_columns holds
// what soft_check decides likewise).  Fills the route, the columns' roles, the
// query digits and the shape of s.
int stream_check(nipamd_model* mm, int n_obs, const int* obs_vars, int n_soft, const int* soft_vars, int n_query,
                 const int* query, int B, int lag, nipamd_stream** out, nipamd_stream& s) {
  if (int rc = check_var_lists("stream", mm, !out || (n_soft > 0 && !soft_vars), "NULL model, variables or result",
                               B < 1 || lag < 0 || lag > NIPAMD_STREAM_MAX_LAG || n_soft < 0,
                               "bad arguments (B >= 1, 0 <= lag <= " + std::to_string(NIPAMD_STREAM_MAX_LAG) + ")",
                               n_obs, obs_vars, n_query, query))
    return rc;
  nipamd::StreamSoftArgs& a = s.a;
  if (int rc = soft_columns("stream", mm, "online inference",
                            "the operator chain and the general engine have no online form; ", n_obs, obs_vars,
                            n_soft, soft_vars, n_query, query, a, s.r, &s.width))
    return rc;
  a.B = B; a.lag = lag;
  s.W = a.lik_tstride;
  if (n_soft > 0) {
    const int rc = nipamd::chain_stream_soft_prepare(a);
    if (rc == nipamd::kLaunchRefused)
      return fail(NIPAMD_ERROR_UNSUPPORTED, "stream: the evidence tables, the transition and the staging rows need " +
                                                std::to_string(nipamd::chain_stream_soft_lds_bytes(a)) +
                                                " bytes of LDS, more than a CU holds");
    if (rc) return launch_fail(rc, "chain_stream_soft_kernel");
  } else {
    const int rc = nipamd::chain_stream_prepare(a);
    if (rc == nipamd::kLaunchRefused)
      return fail(NIPAMD_ERROR_UNSUPPORTED, "stream: the evidence tables, the transition and the window of lag " +
                                                std::to_string(lag) + " need " +
                                                std::to_string(nipamd::chain_stream_lds_bytes(a)) +
                                                " bytes of LDS, more than a CU holds");
    if (rc) return launch_fail(rc, "chain_stream_kernel");
  }
  s.mm = mm; s.B = B; s.lag = lag;
  s.obs_vars.assign(obs_vars, obs_vars + n_obs);
  s.soft_vars.assign(soft_vars, soft_vars + n_soft);
  return 0;
}

// the tables of this call into a (a push uses the model's tables as they are now)
template <typename Args>
int stream_tables(nipamd_stream* s, Args& a) {
  nipamd_model* mm = s->mm;
  if (int rc = ensure_tables(mm)) return rc;           // (the GPU fold of a fold_gpu plan included)
  ReqTables* rt = nullptr;
  if (int rc = ensure_req_tables(mm, s->r, &rt)) return rc;
  const DevState* d = dev_of(mm);
  set_cols(a, mm->m.chain, s->r, *rt, (int)s->obs_vars.size());
  a.A = d->A64; a.sall = d->sall64;
  return 0;
}

int stream_reset(nipamd_stream* s, void* stream) {
  nipamd::StreamArgs a = s->a;
  if (int rc = stream_tables(s, a)) return rc;
  if (int rc = nipamd::chain_stream_init_launch(a, dev_of(s->mm)->pi64, (hipStream_t)stream))
    return launch_fail(rc, "chain_stream_init_kernel");
  s->n = 0; s->pending = 0; s->flushed = false;
  return 0;
}

int rows_of_push(const nipamd_stream* s, int T) { return std::max(0L, (long)s->pending + T - s->lag); }

// the argument verdict of a push / flush (host or device buffers: only tested for NULL)
// soft: the call is a push_soft, which brings likelihood vectors
int push_check(const nipamd_stream* s, const void* obs, const void* lik, bool soft, int T, const void* post) {
  if (!s) return fail(NIP_ERROR_NULLPOINTER, "stream: NULL stream");
  if (!soft && !s->soft_vars.empty())
    return fail(NIP_ERROR_INVALID_ARGUMENT, "stream: the stream has soft evidence columns (nipamd_stream_push_soft "
                                            "brings their likelihood vectors)");
  if (T < 1) return fail(NIP_ERROR_INVALID_ARGUMENT, "stream: a push takes at least one step");
  if (s->flushed) return fail(NIP_ERROR_INVALID_ARGUMENT, "stream: push after flush (nipamd_stream_reset starts over)");
  if (!s->obs_vars.empty() && !obs) return fail(NIP_ERROR_NULLPOINTER, "stream: NULL observations");
  if (!s->soft_vars.empty() && !lik) return fail(NIP_ERROR_NULLPOINTER, "stream: NULL likelihood vectors");
  if (rows_of_push(s, T) > 0 && !post) return fail(NIP_ERROR_NULLPOINTER, "stream: NULL rows for a push that emits");
  return 0;
}
int flush_check(const nipamd_stream* s, const void* post) {
  if (!s) return fail(NIP_ERROR_NULLPOINTER, "stream: NULL stream");
  if (s->pending > 0 && !post) return fail(NIP_ERROR_NULLPOINTER, "stream: NULL rows for a flush that emits");
  return 0;
}

// T new steps (T = 0: the flush) as launches of at most kStreamChunk steps
int stream_run(nipamd_stream* s, const int32_t* d_obs, const double* d_lik, int T, double* d_post, double* d_ll,
               uint32_t* d_status, void* stream) {
  nipamd::StreamSoftArgs a = s->a;
  if (int rc = stream_tables(s, a)) return rc;
  const bool soft = !s->soft_vars.empty();
  const char* kernel = soft ? "chain_stream_soft_kernel" : "chain_stream_kernel";
  a.lik_bstride = (long)T * s->W;
  const long ocols = s->obs_vars.empty() ? 1 : (long)s->obs_vars.size();
  const long rows = T > 0 ? rows_of_push(s, T) : s->pending;
  a.obs_bstride = (long)T * ocols;
  a.obs_tstride = (int)ocols;
  a.post_bstride = rows * s->width;
  a.ll = d_ll; a.status = d_status;
  long done = 0;
  for (int c0 = 0; c0 < std::max(T, 1); c0 += nipamd::kStreamChunk) {
    a.T_new = std::min(nipamd::kStreamChunk, T - c0);
    a.final = T == 0;
    a.n = s->n; a.pending = s->pending;
    a.E = a.final ? s->pending : std::max(0, s->pending + a.T_new - s->lag);
    a.obs = d_obs ? d_obs + c0 * ocols : nullptr;
    a.lik = soft && d_lik ? d_lik + (long)c0 * s->W : nullptr;
    a.post = d_post ? d_post + done * s->width : nullptr;
    if (int rc = soft ? nipamd::chain_stream_soft_launch(a, (hipStream_t)stream)
                      : nipamd::chain_stream_launch(a, (hipStream_t)stream))
      return launch_fail(rc, kernel);
    done += a.E;
    s->n += a.T_new;
    s->pending = a.final ? 0 : (int)std::min<long>(s->n, s->lag);
  }
  if (T == 0) s->flushed = true;
  return 0;
}

}  // namespace

extern "C" {

int nipamd_stream_open_soft(nipamd_model* mm, int n_obs, const int* obs_vars, int n_soft, const int* soft_vars,
                            int n_query, const int* query, int B, int lag, nipamd_stream** out) {
  nipamd_stream* s = new nipamd_stream();
  if (int rc = stream_check(mm, n_obs, obs_vars, n_soft, soft_vars, n_query, query, B, lag, out, *s)) {
    delete s;
    return rc;
  }
  // only now the per-sequence state: base and head [B][NP], the ll's two mantissas and exponent, first dead
  // step, status, and the ring of the pending steps -- codes [B][lag][ncol], or under soft evidence the
  // evaluated evidence [B][lag + kStreamChunk][NP] (none at lag 0)
  const size_t NP = (size_t)nipamd::chain_stream_np(s->a.N), nb = (size_t)B;
  const bool soft = n_soft > 0;
  const size_t ring = soft ? 0 : nb * (size_t)lag * (size_t)s->a.ncol;
  const size_t ering = soft ? nb * nipamd::chain_stream_soft_ring_slots(lag) * NP : 0;
  const size_t fixed = (2 * nb * NP * sizeof(double) +
                        nb * (2 * sizeof(double) + 2 * sizeof(long) + sizeof(unsigned)) + ring * sizeof(int) + 7) &
                       ~(size_t)7;
  const size_t bytes = fixed + ering * sizeof(double);
  int rc = ensure_device(mm);
  if (!rc && hipMalloc(&s->state, bytes) != hipSuccess)
    rc = fail(NIPAMD_ERROR_DEVICE, "stream: device allocation of " + std::to_string(bytes) + " bytes failed");
  if (!rc) {
    nipamd::StreamArgs& a = s->a;
    a.base = static_cast<double*>(s->state);
    a.head = a.base + nb * NP;
    a.snum = a.head + nb * NP;
    a.sden = a.snum + nb;
    a.sexp = reinterpret_cast<long*>(a.sden + nb);
    a.sdead = a.sexp + nb;
    a.sstatus = reinterpret_cast<unsigned*>(a.sdead + nb);
    a.ring = reinterpret_cast<int*>(a.sstatus + nb);
    s->a.ering = ering ? reinterpret_cast<double*>(static_cast<char*>(s->state) + fixed) : nullptr;
    rc = stream_reset(s, nullptr);
    // the first push may come on any HIP stream
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(NIPAMD_ERROR_DEVICE, "stream: initialisation failed");
  }
  if (rc) { (void)hipFree(s->state); delete s; return rc; }
  *out = s;
  return 0;
}

int nipamd_stream_open(nipamd_model* mm, int n_obs, const int* obs_vars, int n_query, const int* query, int B,
                       int lag, nipamd_stream** out) {
  return nipamd_stream_open_soft(mm, n_obs, obs_vars, 0, nullptr, n_query, query, B, lag, out);
}

int nipamd_stream_push(nipamd_stream* s, const int32_t* d_obs, int T, double* d_post, double* d_ll,
                       uint32_t* d_status, void* stream) {
  if (int rc = push_check(s, d_obs, nullptr, false, T, d_post)) return rc;
  return stream_run(s, d_obs, nullptr, T, d_post, d_ll, d_status, stream);
}

int nipamd_stream_push_soft(nipamd_stream* s, const int32_t* d_obs, const double* d_lik, int T, double* d_post,
                            double* d_ll, uint32_t* d_status, void* stream) {
  if (int rc = push_check(s, d_obs, d_lik, true, T, d_post)) return rc;
  return stream_run(s, d_obs, d_lik, T, d_post, d_ll, d_status, stream);
}

int nipamd_stream_flush(nipamd_stream* s, double* d_post, double* d_ll, uint32_t* d_status, void* stream) {
  if (int rc = flush_check(s, d_post)) return rc;
  return stream_run(s, nullptr, nullptr, 0, d_post, d_ll, d_status, stream);
}

int nipamd_stream_reset(nipamd_stream* s, void* stream) {
  if (!s) return fail(NIP_ERROR_NULLPOINTER, "stream: NULL stream");
  return stream_reset(s, stream);
}

int nipamd_stream_pending(const nipamd_stream* s) { return s ? s->pending : -1; }

long nipamd_stream_steps(const nipamd_stream* s) { return s ? s->n : -1; }

void nipamd_stream_free(nipamd_stream* s) {
  if (!s) return;
  (void)hipFree(s->state);
  delete s;
}

int nipamd_stream_push_host(nipamd_stream* s, const int32_t* obs, int T, double* post, double* ll, uint32_t* status) {
  if (int rc = push_check(s, obs, nullptr, false, T, post)) return rc;
  const size_t nob = (size_t)s->B * T * s->obs_vars.size();
  const size_t npo = (size_t)s->B * rows_of_push(s, T) * s->width;
  return host_call(s->obs_vars.empty() ? nullptr : obs, nob, npo ? post : nullptr, npo, false, ll, status, (size_t)s->B,
                   [&](int32_t* d_obs, double* d_post, double* d_ll, uint32_t* d_st) {
                     return stream_run(s, d_obs, nullptr, T, d_post, d_ll, d_st, nullptr);
                   });
}

int nipamd_stream_push_soft_host(nipamd_stream* s, const int32_t* obs, const double* lik, int T, double* post,
                                 double* ll, uint32_t* status) {
  if (int rc = push_check(s, obs, lik, true, T, post)) return rc;
  const size_t nob = (size_t)s->B * T * s->obs_vars.size();
  const size_t npo = (size_t)s->B * rows_of_push(s, T) * s->width;
  const size_t nli = (size_t)s->B * T * (size_t)s->W;
  return host_call(s->obs_vars.empty() ? nullptr : obs, nob, npo ? post : nullptr, npo, false, ll, status, (size_t)s->B,
                   [&](int32_t* d_obs, double* d_post, double* d_ll, uint32_t* d_st) {
                     return with_lik(lik, nli, [&](const double* d_lik) {
                       return stream_run(s, d_obs, d_lik, T, d_post, d_ll, d_st, nullptr);
                     });
                   });
}

int nipamd_stream_flush_host(nipamd_stream* s, double* post, double* ll, uint32_t* status) {
  if (int rc = flush_check(s, post)) return rc;
  const size_t npo = (size_t)s->B * s->pending * s->width;
  return host_call((const int32_t*)nullptr, 0, npo ? post : nullptr, npo, false, ll, status, (size_t)s->B,
                   [&](int32_t*, double* d_post, double* d_ll, uint32_t* d_st) {
                     return stream_run(s, nullptr, nullptr, 0, d_post, d_ll, d_st, nullptr);
                   });
}

}  // extern "C"
