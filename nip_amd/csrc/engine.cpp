// engine.cpp -- C-ABI of the nip_amd engine (include/nip_amd.h): the error
// string, the model's lifecycle and its read accessors.
//
// The host side of the hot path is split by concern (engine_internal.h): it
// owns the compiled model, its device-resident tables and scratch
// (engine_dev.cpp), validates the request against the GPU execution plan and
// picks the kernel (engine_route.cpp) and launches the gfx950 kernels on the
// caller's stream (engine_fb.cpp, engine_estep.cpp).  There is no CPU
// fallback: a request the GPU plan does not cover fails with
// NIPAMD_ERROR_UNSUPPORTED, and a missing/unusable device with
// NIPAMD_ERROR_DEVICE.
#include <algorithm>
#include <cstring>
#include <fstream>
#include <sstream>

#include "engine_internal.h"

using namespace nipamd::eng;

namespace {
thread_local std::string g_err;
}

namespace nipamd {

int eng::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int eng::launch_fail(int rc, const char* what) {
  if (rc == kLaunchRefused)
    return fail(NIPAMD_ERROR_UNSUPPORTED, std::string(what) + ": the request does not fit the kernel (refused on the host)");
  return fail(NIPAMD_ERROR_DEVICE, std::string(what) + ": kernel launch failed: " + hipGetErrorString(hipGetLastError()));
}

int set_error(int code, const std::string& msg) { return eng::fail(code, msg); }
const char* g_last_kernel = "";

}  // namespace nipamd

extern "C" {

const char* nipamd_last_error(void) { return g_err.c_str(); }

const char* nipamd_last_kernel(void) { return nipamd::g_last_kernel; }

int nipamd_model_from_spec(int n_nodes, const char* const* symbols, const int* card,
                           const int* next, int n_pots, const int* pot_child,
                           const int* pot_nparents, const int* pot_parents,
                           const int* pot_ndata, const double* pot_data,
                           nipamd_model** out) {
  if (!out || !card || n_nodes <= 0) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  nipamd::NetSpec spec;
  for (int i = 0; i < n_nodes; i++) {
    spec.symbols.push_back(symbols && symbols[i] ? symbols[i] : ("V" + std::to_string(i)));
    spec.card.push_back(card[i]);
    spec.next.push_back(next ? next[i] : -1);
  }
  size_t po = 0, dof = 0;
  for (int p = 0; p < n_pots; p++) {
    nipamd::NetSpec::Pot q;
    q.child = pot_child[p];
    for (int k = 0; k < pot_nparents[p]; k++) q.parents.push_back(pot_parents[po++]);
    q.has_data = pot_ndata[p] > 0;
    q.data.assign(pot_data + dof, pot_data + dof + pot_ndata[p]);
    dof += pot_ndata[p];
    if (q.child < 0 || q.child >= n_nodes) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad child index");
    for (int v : q.parents) if (v < 0 || v >= n_nodes) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad parent index");
    spec.pots.push_back(std::move(q));
  }
  auto* mm = new nipamd_model();
  std::string err;
  int rc = nipamd::compile_model(spec, mm->m, err);
  if (rc) { delete mm; return fail(rc, err); }
  *out = mm;
  return 0;
}

int nipamd_model_from_net(const char* path, nipamd_model** out) {
  if (!path || !out) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  std::ifstream f(path);
  if (!f) return fail(NIP_ERROR_FILENOTFOUND, std::string("cannot open ") + path);
  std::stringstream ss;
  ss << f.rdbuf();
  nipamd::NetSpec spec;
  std::string err;
  int rc = nipamd::parse_net_file(ss.str(), spec, err);
  if (rc) return fail(rc, err);
  auto* mm = new nipamd_model();
  rc = nipamd::compile_model(spec, mm->m, err);
  if (rc) { delete mm; return fail(rc, err); }
  *out = mm;
  return 0;
}

void nipamd_model_free(nipamd_model* mm) {
  if (!mm) return;
  nipamd::generate_release(mm);
  nipamd::jt_release(mm);
  nipamd::op_release(mm);
  nipamd::likelihood_release(mm);
  DevState* d = static_cast<DevState*>(mm->m.dev);
  dev_release(d);
  delete d;
  delete mm;
}

int nipamd_model_num_vars(const nipamd_model* mm) { return mm ? (int)mm->m.vars.size() : -1; }

int nipamd_model_var_index(const nipamd_model* mm, const char* symbol) {
  if (!mm || !symbol) return -1;
  for (size_t i = 0; i < mm->m.vars.size(); i++)
    if (mm->m.vars[i].symbol == symbol) return (int)i;
  return -1;
}

int nipamd_model_var_card(const nipamd_model* mm, int v) {
  if (!mm || v < 0 || v >= (int)mm->m.vars.size()) return -1;
  return mm->m.vars[v].card;
}

int nipamd_model_desc_json(const nipamd_model* mm, char* buf, int cap) {
  if (!mm) return -1;
  std::string s = nipamd::model_desc_json(mm->m);
  if (buf && cap > 0) {
    size_t n = s.size() < (size_t)(cap - 1) ? s.size() : (size_t)(cap - 1);
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return (int)s.size();
}

int nipamd_model_param_size(const nipamd_model* mm) { return mm ? nipamd::param_size(mm->m) : -1; }

int nipamd_model_gpu_supported(const nipamd_model* mm, int n_obs, const int* obs_vars,
                               int n_query, const int* query) {
  if (!mm) return 0;
  Route r; std::string why;
  if (mm->engine != NIPAMD_ENGINE_JTREE && route_request(mm, n_obs, obs_vars, n_query, query, r, why)) return 1;
  if (mm->engine == NIPAMD_ENGINE_AUTO &&
      nipamd::op_supported(const_cast<nipamd_model*>(mm), n_obs, obs_vars, n_query, query, why))
    return 1;
  return mm->engine != NIPAMD_ENGINE_CHAIN && nipamd::jt_supported(mm, n_obs, obs_vars, n_query, query, why);
}

int nipamd_jt_plan_dump(const nipamd_model* mm, int n_obs, const int* obs_vars, int n_query,
                        const int* query, int estep, int* hdr, int hdr_cap, int* ip, long ip_cap,
                        double* dp, long dp_cap, long* sizes) {
  if (!mm || !hdr || !sizes || (n_obs > 0 && !obs_vars) || (n_query > 0 && !query))
    return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  return nipamd::jt_plan_dump(mm, n_obs, obs_vars, n_query, query, estep, hdr, hdr_cap, ip, ip_cap, dp,
                              dp_cap, sizes);
}

int nipamd_model_fold(nipamd_model* mm, int keep, double* out, long cap, double* kernel_ms, double* bytes) {
  if (!mm || !out) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  const auto& P = mm->m.chain;
  if (!P.valid || P.joint) return fail(NIPAMD_ERROR_UNSUPPORTED, "the model has no single-variable interface-chain plan");
  if (keep < -1 || keep >= (int)P.hidden.size()) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad hidden parent");
  const long need = (keep < 0 ? 1L : (long)mm->m.vars[P.hidden[keep]].card) * 64 * 64;
  if (cap < need) return fail(NIP_ERROR_INVALID_ARGUMENT, "output buffer too small");
  if (int rc = ensure_device(mm)) return rc;
  std::vector<double> v;
  std::string err;
  double ms = 0, by = 0;
  if (nipamd::chain_fold_gpu(mm->m, keep, v, &ms, &by, err)) return fail(NIPAMD_ERROR_DEVICE, "fold: " + err);
  std::copy(v.begin(), v.end(), out);
  if (kernel_ms) *kernel_ms = ms;
  if (bytes) *bytes = by;
  return 0;
}

int nipamd_model_set_engine(nipamd_model* mm, int engine) {
  if (!mm || engine < NIPAMD_ENGINE_AUTO || engine > NIPAMD_ENGINE_JTREE) return -1;
  const int prev = mm->engine;
  mm->engine = engine;
  return prev;
}

int nipamd_model_original(const nipamd_model* mm, int c, double* out, int cap) {
  if (!mm || c < 0 || c >= (int)mm->m.cliques.size()) return -1;
  const auto& o = mm->m.cliques[c].original;
  size_t n = o.size() < (size_t)cap ? o.size() : (size_t)cap;
  if (out) std::memcpy(out, o.data(), n * sizeof(double));
  return (int)o.size();
}

int nipamd_model_prior(const nipamd_model* mm, int v, double* out) {
  if (!mm || v < 0 || v >= (int)mm->m.vars.size()) return -1;
  const auto& var = mm->m.vars[v];
  if (!var.has_prior || !var.parents.empty()) return 0;
  if (out) std::memcpy(out, var.prior.data(), var.prior.size() * sizeof(double));
  return (int)var.prior.size();
}

int nipamd_model_num_cliques(const nipamd_model* mm) { return mm ? (int)mm->m.cliques.size() : -1; }
int nipamd_model_num_sepsets(const nipamd_model* mm) { return mm ? (int)mm->m.sepsets.size() : -1; }

int nipamd_model_clique(const nipamd_model* mm, int c, int* vars, int* n_vars, int* links, int* n_links) {
  if (!mm || c < 0 || c >= (int)mm->m.cliques.size()) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad clique");
  const auto& q = mm->m.cliques[c];
  if (n_vars) *n_vars = (int)q.vars.size();
  if (n_links) *n_links = (int)q.links.size();
  if (vars) std::copy(q.vars.begin(), q.vars.end(), vars);
  if (links) std::copy(q.links.begin(), q.links.end(), links);
  return NIP_NO_ERROR;
}

int nipamd_model_sepset(const nipamd_model* mm, int s, int* a, int* b, int* vars, int* n_vars) {
  if (!mm || s < 0 || s >= (int)mm->m.sepsets.size()) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad sepset");
  const auto& q = mm->m.sepsets[s];
  if (a) *a = q.a;
  if (b) *b = q.b;
  if (n_vars) *n_vars = (int)q.vars.size();
  if (vars) std::copy(q.vars.begin(), q.vars.end(), vars);
  return NIP_NO_ERROR;
}

int nipamd_model_interface_cliques(const nipamd_model* mm, int* in_clique, int* out_clique) {
  if (!mm) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad model");
  if (in_clique) *in_clique = mm->m.in_clique;
  if (out_clique) *out_clique = mm->m.out_clique;
  return NIP_NO_ERROR;
}

int nipamd_model_set_tables(nipamd_model* mm, int n_cliques, const double* const* originals,
                            int n_vars, const double* const* priors) {
  if (!mm || n_cliques != (int)mm->m.cliques.size() || n_vars != (int)mm->m.vars.size() ||
      (n_cliques > 0 && !originals) || (n_vars > 0 && !priors))
    return fail(NIP_ERROR_INVALID_ARGUMENT, "nipamd_model_set_tables: bad arguments");
  for (int c = 0; c < n_cliques; c++) {
    auto& o = mm->m.cliques[c].original;
    if (originals[c]) std::memcpy(o.data(), originals[c], o.size() * sizeof(double));
  }
  for (int v = 0; v < n_vars; v++) {
    auto& var = mm->m.vars[v];
    if (!priors[v] || !var.parents.empty()) continue;
    var.prior.assign(priors[v], priors[v] + var.card);
    var.has_prior = true;
  }
  nipamd::build_chain_plan(mm->m);
  mm->version++;
  return NIP_NO_ERROR;
}

int nipamd_graph_cliques(int n, const int* card, int n_edges, const int* edges,
                         int set_parents, int* clique_off, int* clique_vars, int cap) {
  if (n <= 0 || !card || (n_edges > 0 && !edges) || !clique_off) return -NIP_ERROR_INVALID_ARGUMENT;
  std::vector<int> cd(card, card + n);
  std::vector<std::pair<int, int>> e;
  for (int i = 0; i < n_edges; i++) e.emplace_back(edges[2 * i], edges[2 * i + 1]);
  std::vector<std::vector<int>> cl;
  std::string err;
  int nc = nipamd::compile_graph_only(n, cd, e, set_parents != 0, cl, err);
  if (nc < 0) { g_err = err; return -NIP_ERROR_GENERAL; }
  int pos = 0;
  clique_off[0] = 0;
  for (int c = 0; c < nc; c++) {
    for (int v : cl[c]) { if (clique_vars && pos < cap) clique_vars[pos] = v; pos++; }
    clique_off[c + 1] = pos;
  }
  return nc;
}

int nipamd_m_step(nipamd_model* mm, const double* params) {
  if (!mm || !params) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  int rc = nipamd::m_step(mm->m, params);
  mm->version++;
  return rc;
}

}  // extern "C"
