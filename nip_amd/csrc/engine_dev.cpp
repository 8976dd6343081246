// engine_dev.cpp -- the model's device state: the buffer pool, the uploads of
// the chain plan's tables and of a request's tables, scratch and work
// buffers, the fixed-order row reduction (engine_internal.h).
#include "engine_internal.h"

namespace nipamd::eng {

void* dalloc(DevState* d, size_t bytes) {
  for (size_t i = 0; i < d->pool.size(); i++)
    if (d->pool[i].second == bytes) {
      void* p = d->pool[i].first;
      d->pool[i] = d->pool.back();
      d->pool.pop_back();
      d->live[p] = bytes;
      return p;
    }
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  d->live[p] = bytes;
  return p;
}

// back to the pool (the caller has synchronised the device), or hipFree for
// buffers the pool did not hand out
void dfree(DevState* d, void* p) {
  if (!p) return;
  auto it = d->live.find(p);
  if (it == d->live.end()) { (void)hipFree(p); return; }
  d->pool.push_back(*it);
  d->live.erase(it);
}

DevState* dev_of(nipamd_model* mm) {
  if (!mm->m.dev) mm->m.dev = new DevState();
  return static_cast<DevState*>(mm->m.dev);
}

static void free_tables(DevState* d) {
  // queued kernels may still read the tables: they return to the pool only
  // once the device is idle (hipFree synchronised the same way)
  if (!d->live.empty()) (void)hipDeviceSynchronize();
  dfree(d, d->arena);
  d->A = d->pi = d->A64 = d->pi64 = d->sall64 = d->arena = nullptr;
  for (auto& r : d->reqs) dfree(d, r.arena);
  d->reqs.clear();
  for (double* p : d->G) dfree(d, p);
  d->childE.clear();
  d->G.clear();
  dfree(d, d->jm_ptr); dfree(d, d->jm_idx); dfree(d, d->jm_coef);
  d->jm_ptr = nullptr; d->jm_idx = nullptr; d->jm_coef = nullptr; d->jm_n = 0; d->jm_kind = 0;
  dfree(d, d->etab_all);
  d->etab_all = nullptr;
}

void dev_release(DevState* d) {
  if (!d) return;
  free_tables(d);
  for (auto& e : d->pool) (void)hipFree(e.first);
  d->pool.clear();
  (void)hipFree(d->S); (void)hipFree(d->W); (void)hipFree(d->R); (void)hipFree(d->Q);
  *d = DevState();
}

namespace {
// Several tables in one pool buffer with one host-to-device copy: every
// em_learn iteration re-uploads the model's tables after its m_step, and a
// synchronous copy per table kept the device idle for ~0.2 ms per iteration
// (profiles/r05/em_phases.py).  Each table starts on a 64-byte boundary.
struct Staged {
  std::vector<double> host;
  std::vector<std::pair<double**, size_t>> dst;
  template <typename V>
  void add(double** p, const V& v) {
    dst.push_back({p, host.size()});
    host.insert(host.end(), v.begin(), v.end());
    host.resize((host.size() + 8) & ~(size_t)7, 0.0);     // >= 1 double, 64-byte aligned
  }
  int commit(DevState* d, double** arena) {
    *arena = static_cast<double*>(dalloc(d, host.size() * sizeof(double)));
    if (!*arena) return fail(NIPAMD_ERROR_DEVICE, "device allocation failed");
    HIP_OK(hipMemcpy(*arena, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
    for (auto& e : dst) *e.first = *arena + e.second;
    return 0;
  }
};
}  // namespace

// Bind the model's device state to the current device (a different device
// drops every buffer of the old one).  Call before taking any DevState
// pointer that a later ensure_* must not free.
int ensure_device(nipamd_model* mm) {
  int dev = -1;
  HIP_OK(hipGetDevice(&dev));
  DevState* d = dev_of(mm);
  if (d->device != dev) { dev_release(d); d->device = dev; }
  return 0;
}

// Upload the chain plan's tables to the current device (once per version).
int ensure_tables(nipamd_model* mm) {
  if (int rc = ensure_device(mm)) return rc;
  DevState* d = dev_of(mm);
  if (d->version == mm->version && d->A64) return 0;
  if (int rc = nipamd::ensure_fold(mm)) return rc;
  const auto& P = mm->m.chain;
  free_tables(d);
  Staged sg;
  if (P.N <= 16) {
    sg.add(&d->A, P.A);
    sg.add(&d->pi, P.pi);
  }
  sg.add(&d->A64, P.A64);
  sg.add(&d->pi64, P.pi64);
  sg.add(&d->sall64, P.s_all64);
  d->childE.assign(P.emits.size(), nullptr);
  for (size_t k = 0; k < P.emits.size(); k++) {
    std::vector<double> t(P.emits[k].E);
    t.insert(t.end(), P.emits[k].s.begin(), P.emits[k].s.end());
    sg.add(&d->childE[k], t);
  }
  if (int rc = sg.commit(d, &d->arena)) return rc;
  d->G.assign(P.hidden.size(), nullptr);
  d->version = mm->version;
  return 0;
}

// G table of hidden parent j on the device (derived marginals)
int ensure_hidden(nipamd_model* mm, int j) {
  DevState* d = dev_of(mm);
  if (d->G[j]) return 0;
  std::vector<double> g;
  if (mm->m.chain.fold_gpu) {
    std::string err;
    double ms = 0, bytes = 0;
    if (nipamd::chain_fold_gpu(mm->m, j, g, &ms, &bytes, err)) return fail(NIPAMD_ERROR_DEVICE, "hidden fold: " + err);
  } else {
    nipamd::hidden_table(mm->m, j, g);
  }
  return upload(d, &d->G[j], g);
}

// Tables of a route (built and uploaded once per model version).
int ensure_req_tables(nipamd_model* mm, const Route& r, ReqTables** out) {
  DevState* d = dev_of(mm);
  const auto& P = mm->m.chain;
  std::string key;
  for (int i = 0; i < r.ncol; i++) key += std::to_string(r.emit[i]) + ",";
  key += "|" + std::to_string(r.primary);
  for (auto& t : d->reqs) if (t.key == key) { *out = &t; return 0; }
  ReqTables t;
  t.key = key;
  t.shrink = step_shrink(P, r);
  Staged sg;                                 // every table of the request, one upload
  const int N = P.N;
  if (N <= 16) {
    // narrow: the primary child's table times the other children's row sums
    std::vector<double> b(16, 0.0);
    for (int y = 0; y < N; y++) {
      double v = 1.0;
      for (size_t k = 0; k < P.emits.size(); k++) if ((int)k != r.primary) v *= P.emits[k].s[y];
      b[y] = v;
    }
    const int M = r.primary >= 0 ? P.emit(r.primary).M : 0;
    std::vector<double> E((size_t)(M + 2) * 16, 0.0);
    for (int y = 0; y < N; y++) {
      for (int m = 0; m < M; m++) E[(size_t)m * 16 + y] = P.emit(r.primary).E[(size_t)m * 64 + y] * b[y];
      E[(size_t)M * 16 + y] = (r.primary >= 0 ? P.emit(r.primary).s[y] : 1.0) * b[y];
    }
    std::vector<double> ts(16, 0.0);
    for (int x = 0; x < N; x++) {
      double acc = 0.0;
      for (int y = 0; y < N; y++) acc += P.A[x * 16 + y] * E[(size_t)M * 16 + y];
      ts[x] = acc;
    }
    t.M0 = M;
    sg.add(&t.Etab16, E);
    sg.add(&t.ts16, ts);
  }
  // wide: one unscaled table per observed child, the unobserved ones in ebase
  std::vector<double> W;
  for (int i = 0; i < r.ncol; i++) {
    const auto& em = P.emit(r.emit[i]);
    t.tabw_off.push_back(W.size());
    const size_t base = W.size();
    W.resize(base + (size_t)(em.M + 2) * 64, 0.0);
    for (int y = 0; y < N; y++) {
      for (int m = 0; m < em.M; m++) W[base + (size_t)m * 64 + y] = em.E[(size_t)m * 64 + y];
      W[base + (size_t)em.M * 64 + y] = em.s[y];
    }
  }
  std::vector<double> eb(64, 0.0);
  for (int y = 0; y < N; y++) {
    double v = 1.0;
    for (size_t k = 0; k < P.emits.size(); k++) {
      bool obs = false;
      for (int i = 0; i < r.ncol; i++) obs |= r.emit[i] == (int)k;
      if (!obs) v *= P.emits[k].s[y];
    }
    eb[y] = v;
  }
  sg.add(&t.tabw, W);
  sg.add(&t.ebase, eb);
  if (N <= 32) {
    const int NP = N <= 16 ? 16 : 32;
    std::vector<double> MT;
    const int nc = r.ncol > 0 ? r.ncol : 1;
    for (int i = 0; i < nc; i++) {
      const int M = r.ncol > 0 ? P.emit(r.emit[i]).M : 0;
      t.mtab_off[i] = (int)MT.size();
      const size_t base = MT.size();
      MT.resize(base + (size_t)(M + 2) * NP, 0.0);
      for (int y = 0; y < N; y++) {
        const double f = i == 0 ? eb[y] : 1.0;
        if (r.ncol > 0) {
          const auto& em = P.emit(r.emit[i]);
          for (int m = 0; m < M; m++) MT[base + (size_t)m * NP + y] = em.E[(size_t)m * 64 + y] * f;
          MT[base + (size_t)M * NP + y] = em.s[y] * f;
        } else {
          MT[base + y] = f;
        }
      }
    }
    t.mtab_rows = (int)(MT.size() / NP);
    std::vector<double> wv(64, 0.0);
    for (int x = 0; x < N; x++) {
      double acc = 0.0;
      for (int y = 0; y < N; y++) acc += P.A64[(size_t)x * 64 + y] * P.s_all64[y];
      wv[x] = acc;
    }
    sg.add(&t.mtab, MT);
    sg.add(&t.wv, wv);
  }
  // mlss only (chain_viterbi_kernel): slice -1 is summed out, not maximised (x
  // ascending).  Built for every route so that the request's tables stay one
  // upload and one cache entry; fb, filter and e_step never read these 64 doubles.
  std::vector<double> u0(64, 0.0);
  for (int y = 0; y < N; y++) {
    double acc = 0.0;
    for (int x = 0; x < N; x++) acc += P.pi64[x] * P.A64[(size_t)x * 64 + y];
    u0[y] = acc;
  }
  sg.add(&t.u0, u0);
  if (int rc = sg.commit(d, &t.arena)) return rc;
  d->reqs.push_back(std::move(t));
  *out = &d->reqs.back();
  return 0;
}

// a grow-only device buffer: nothing to do while it holds `bytes`
static int ensure_buf(double** p, size_t* have, size_t bytes) {
  if (*have >= bytes) return 0;
  (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  HIP_OK(hipMalloc(p, bytes));
  *have = bytes;
  return 0;
}
int ensure_scratch(nipamd_model* mm, size_t bytes) { DevState* d = dev_of(mm); return ensure_buf(&d->S, &d->S_bytes, bytes); }
int ensure_q(nipamd_model* mm, size_t bytes) { DevState* d = dev_of(mm); return ensure_buf(&d->Q, &d->Q_bytes, bytes); }
int ensure_work(nipamd_model* mm, size_t bytes) { DevState* d = dev_of(mm); return ensure_buf(&d->W, &d->W_bytes, bytes); }

// rows [n][S] -> out [S] by repeated radix-64 tree levels (ping-pong tA/tB)
int reduce_rows(const double* in, long n, int S, double* tA, double* tB, double* out, hipStream_t st) {
  const double* cur = in;
  while (n > 64) {
    double* dst = (cur == tA) ? tB : tA;
    if (nipamd::tree_reduce_launch(cur, n, S, dst, st)) return -1;
    cur = dst;
    n = (n + 63) / 64;
  }
  return nipamd::tree_reduce_launch(cur, n, S, out, st);
}

}  // namespace nipamd::eng

// A deferred fold (large in-clique, ChainPlan::fold_gpu): A64 on the GPU, then
// on the host for every host-side use (derived tables, likelihood, P.A).
int nipamd::ensure_fold(nipamd_model* mm) {
  using namespace nipamd::eng;
  auto& P = mm->m.chain;
  if (!P.valid || !P.fold_gpu || P.folded) return 0;
  if (int rc = ensure_device(mm)) return rc;
  std::vector<double> A;
  std::string err;
  if (nipamd::chain_fold_gpu(mm->m, -1, A, &mm->fold_ms, &mm->fold_bytes, err))
    return fail(NIPAMD_ERROR_DEVICE, "transition fold: " + err);
  P.A64 = std::move(A);
  if (P.N <= 16)
    for (int x = 0; x < P.N; x++)
      for (int y = 0; y < P.N; y++) P.A[x * 16 + y] = P.A64[x * 64 + y];
  P.folded = true;
  return 0;
}
