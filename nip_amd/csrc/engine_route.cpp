// engine_route.cpp -- which plan and which kernel serve a request: routing
// through the chain plan, the plan's predicates and the kernel pickers.
// Everything here reads host data only (engine_internal.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "engine_internal.h"

namespace nipamd::eng {

// Role of a query variable in the chain plan: 0 the interface variable, 1 its
// previous-slice copy, 2 + k leaf child k, 500 + i / 700 + i previous-slice /
// current interface variable i of a joint interface, 1000 + j hidden parent j;
// -1 none.
// Every variable of a single-variable plan has one (build_chain_plan accounts
// for all); a joint plan covers the interface variables, their previous-slice
// copies and the leaf children it factorises.
int query_kind(const ChainPlan& P, int v) {
  if (v == P.v_cur) return 0;
  if (v == P.v_prev) return 1;
  for (size_t i = 0; i < P.jprev.size(); i++) if (P.jprev[i] == v) return 500 + (int)i;
  for (size_t i = 0; i < P.jcur.size(); i++) if (P.jcur[i] == v) return 700 + (int)i;
  for (size_t k = 0; k < P.emits.size(); k++) if (P.emits[k].var == v) return 2 + (int)k;
  for (size_t j = 0; j < P.hidden.size(); j++) if (P.hidden[j] == v) return 1000 + (int)j;
  return -1;
}

// Which GPU plan (if any) covers this request.
int route_request(const nipamd_model* mm, int n_obs, const int* obs_vars, int n_query,
                  const int* query, Route& r, std::string& why) {
  const auto& P = mm->m.chain;
  if (!P.valid) {
    why = "model slice is not an interface chain (GPU plan: one interface variable, hidden "
          "independent parents, leaf children; see DESIGN.md)";
    return 0;
  }
  r = Route();
  for (int i = 0; i < n_obs; i++) {
    int k = -1;
    for (size_t e = 0; e < P.emits.size(); e++) if (P.emits[e].var == obs_vars[i]) k = (int)e;
    if (obs_vars[i] == P.v_cur) k = (int)P.emits.size();          // the interface variable itself
    if (k < 0) {
      why = "evidence on a variable that is neither the interface variable nor a leaf child of it";
      return 0;
    }
    for (int j = 0; j < r.ncol; j++) if (r.emit[j] == k) { why = "observed variable listed twice"; return 0; }
    if (r.ncol == 4) { why = "more than four observed children"; return 0; }
    r.col[r.ncol] = i; r.emit[r.ncol] = k; r.ncol++;
  }
  for (int i = 0; i < n_query; i++)
    if (query_kind(P, query[i]) < 0) { why = "query variable outside the chain plan"; return 0; }
  r.narrow = P.N <= 16 && r.ncol <= 1;
  if (r.ncol == 1) { r.primary = r.emit[0]; r.pcol = r.col[0]; }
  else if (!P.emits.empty()) { r.primary = 0; r.pcol = -1; }
  return 1;
}

// The argument verdict of a chain-plan entry point (`what`: "mlss", "stream"),
// in the order all of them give it: a NULL model or variable list, or the
// caller's own `null` -> NIP_ERROR_NULLPOINTER; a negative count, or the
// caller's own `bad` -> NIP_ERROR_INVALID_ARGUMENT; then every variable index
// against the model.  null_msg / bad_msg: the entry point's wording.
int check_var_lists(const std::string& what, const nipamd_model* mm, bool null, const char* null_msg, bool bad,
                    const std::string& bad_msg, int n_obs, const int* obs_vars, int n_query, const int* query) {
  if (!mm || null || (n_obs > 0 && !obs_vars) || (n_query > 0 && !query))
    return fail(NIP_ERROR_NULLPOINTER, what + ": " + null_msg);
  if (bad || n_obs < 0 || n_query < 0) return fail(NIP_ERROR_INVALID_ARGUMENT, what + ": " + bad_msg);
  const int nv = (int)mm->m.vars.size();
  for (int i = 0; i < n_obs; i++)
    if (obs_vars[i] < 0 || obs_vars[i] >= nv) return fail(NIP_ERROR_INVALID_ARGUMENT, what + ": bad observed variable");
  for (int i = 0; i < n_query; i++)
    if (query[i] < 0 || query[i] >= nv) return fail(NIP_ERROR_INVALID_ARGUMENT, what + ": bad query variable");
  return 0;
}

// The scope of an entry point that runs on the interface-chain plan only
// (`subject` runs ...; no_plan: what else the refusal of a model without a
// chain plan says).
int chain_scope(const nipamd_model* mm, const std::string& what, const char* subject, const char* no_plan) {
  if (mm->engine == NIPAMD_ENGINE_JTREE)
    return fail(NIPAMD_ERROR_UNSUPPORTED, what + ": the engine is set to NIPAMD_ENGINE_JTREE; " + subject +
                                              " runs on the interface-chain plan only");
  if (!mm->m.chain.valid)
    return fail(NIPAMD_ERROR_UNSUPPORTED, what + ": model slice is not an interface chain (no chain plan; " + no_plan +
                                              "see DESIGN.md)");
  return 0;
}

// query [n_query] as digits of a joint interface's state (the first variable
// fastest): false unless it lists distinct current-slice interface variables.
// qstride / qcard [n_query]: variable j is (state / qstride[j]) % qcard[j];
// *width: the sum of their cardinalities.
bool interface_digits(const nipamd_model* mm, int n_query, const int* query, int* qstride, int* qcard, int* width) {
  const auto& P = mm->m.chain;
  *width = 0;
  for (int j = 0; j < n_query; j++) {
    int k = -1, stride = 1;
    for (size_t i = 0; i < P.jcur.size(); i++) if (P.jcur[i] == query[j]) k = (int)i;
    for (int i = 0; i < j; i++) if (query[i] == query[j]) return false;
    if (k < 0) return false;
    for (int i = 0; i < k; i++) stride *= mm->m.vars[P.jcur[i]].card;
    qstride[j] = stride; qcard[j] = mm->m.vars[query[j]].card;
    *width += qcard[j];
  }
  return true;
}

// mlss's query rule (nipamd_mlss, nipamd_mlss_soft): the variables of interest
// are the interface, all of it and nothing else.  Fills the path's columns:
// *nq, qstride / qcard [*nq] (a single interface variable: one column).
int interface_query(const std::string& what, const nipamd_model* mm, int n_query, const int* query, int* nq,
                    int* qstride, int* qcard) {
  const auto& P = mm->m.chain;
  bool is_if = true;
  if (!P.joint) {
    is_if = n_query == 1 && query[0] == P.v_cur;
    *nq = 1; qstride[0] = 1; qcard[0] = P.N;
  } else {
    if ((int)P.jcur.size() > nipamd::kViterbiMaxQuery)
      return fail(NIPAMD_ERROR_UNSUPPORTED, what + ": the joint interface has " + std::to_string(P.jcur.size()) +
                                                " variables; the path holds at most " +
                                                std::to_string(nipamd::kViterbiMaxQuery) + " columns");
    int width = 0;
    is_if = n_query == (int)P.jcur.size() && interface_digits(mm, n_query, query, qstride, qcard, &width);
    *nq = n_query;
  }
  if (!is_if)
    return fail(NIPAMD_ERROR_UNSUPPORTED, what + ": the query is not exactly the interface (every outgoing-interface "
                                              "variable of the slice once, and no other variable)");
  return 0;
}

// What soft_check, stream_check and mlss_soft_check decide after
// check_var_lists, in this order: the soft variables, chain_scope (subject,
// no_plan), a variable both hard and soft, the route of the hard columns
// followed by the soft ones (soft_evidence_columns); then the query --
// soft_columns: any distinct current-slice interface variables; mlss_soft_check:
// interface_query.  soft_evidence_columns fills r and of a: N, ncol, nhard, M,
// col (a soft column's: where its weights start in a row of lik), lik_tstride;
// soft_columns the query digits and post_tstride = *width besides.
template <typename A>
int soft_evidence_columns(const std::string& what, nipamd_model* mm, const char* subject, const char* no_plan,
                          int n_obs, const int* obs_vars, int n_soft, const int* soft_vars, A& a, Route& r) {
  for (int i = 0; i < n_soft; i++)
    if (soft_vars[i] < 0 || soft_vars[i] >= (int)mm->m.vars.size())
      return fail(NIP_ERROR_INVALID_ARGUMENT, what + ": bad soft-evidence variable");
  if (int rc = chain_scope(mm, what, subject, no_plan)) return rc;
  const auto& P = mm->m.chain;
  std::vector<int> all(obs_vars, obs_vars + n_obs);
  all.insert(all.end(), soft_vars, soft_vars + n_soft);
  for (int i = 0; i < n_obs; i++)
    for (int j = 0; j < n_soft; j++)
      if (obs_vars[i] == soft_vars[j])
        return fail(NIPAMD_ERROR_UNSUPPORTED, what + ": a variable is listed as hard and as soft evidence");
  std::string why;
  if (!route_request(mm, (int)all.size(), all.data(), 0, nullptr, r, why))
    return fail(NIPAMD_ERROR_UNSUPPORTED, what + ": " + why);
  a.N = P.N;
  a.ncol = r.ncol; a.nhard = n_obs;
  a.lik_tstride = 0;
  for (int i = 0; i < r.ncol; i++) {
    a.M[i] = P.emit(r.emit[i]).M;
    a.col[i] = r.col[i];
    if (i >= n_obs) { a.col[i] = a.lik_tstride; a.lik_tstride += a.M[i]; }
  }
  return 0;
}
template int soft_evidence_columns(const std::string&, nipamd_model*, const char*, const char*, int, const int*, int,
                                   const int*, nipamd::ViterbiSoftArgs&, Route&);
template int soft_evidence_columns(const std::string&, nipamd_model*, const char*, const char*, int, const int*, int,
                                   const int*, nipamd::EstepSoftArgs&, Route&);

template <typename A>
int soft_columns(const std::string& what, nipamd_model* mm, const char* subject, const char* no_plan, int n_obs,
                 const int* obs_vars, int n_soft, const int* soft_vars, int n_query, const int* query, A& a, Route& r,
                 int* width) {
  if (int rc = soft_evidence_columns(what, mm, subject, no_plan, n_obs, obs_vars, n_soft, soft_vars, a, r)) return rc;
  const auto& P = mm->m.chain;
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
    return fail(NIPAMD_ERROR_UNSUPPORTED, what + ": the query is not a non-empty list of distinct current-slice "
                                              "interface variables (at most " +
                                              std::to_string(nipamd::kViterbiMaxQuery) + ")");
  a.post_tstride = *width;
  return 0;
}
template int soft_columns(const std::string&, nipamd_model*, const char*, const char*, int, const int*, int, const int*,
                          int, const int*, nipamd::SoftArgs&, Route&, int*);
template int soft_columns(const std::string&, nipamd_model*, const char*, const char*, int, const int*, int, const int*,
                          int, const int*, nipamd::StreamSoftArgs&, Route&, int*);

// The chain's transition rows and every child's rows sum to 1 within 1e-15
// (normalised CPTs; every m_step's output): the reference's per-step
// log m2 - log m1 then telescope to log P(obs) (m1_t is the previous step's
// mass), which chain_estep16_kernel's proper mode computes from the final
// forward mass -- the ll differs by the tables' rounding, <= T x 1e-15.
bool chain_proper(const ChainPlan& P) {
  if (P.N > 64) return false;
  for (int x = 0; x < P.N; x++) {
    double r = 0.0;
    for (int y = 0; y < P.N; y++) r += P.A64[x * 64 + y];
    if (!(std::fabs(r - 1.0) <= 1e-15)) return false;
  }
  for (const auto& E : P.emits)
    for (int y = 0; y < P.N; y++)
      if (!(std::fabs(E.s[y] - 1.0) <= 1e-15)) return false;
  return true;
}

// chain_estep16_kernel's proper mode may let the forward rows rescale every
// 4th step (as the backward rows do) when no step can shrink a vector's
// largest entry by more than 1e-30: then either direction's vector keeps its
// largest entry above 1e-120 between rescales and phase B's products
// alpha^ beta^ stay far above the subnormals.  Bound: for every previous
// state x and every code o (the missing row included), the largest entry of
// row x of A times the evidence column of o.  One child only (the HMM shape);
// otherwise every step rescales (tests/test_gpu_estep.py peaked models).
bool estep16_sparse_ok(const ChainPlan& P, int ne) {
  if (ne != 1 || P.emits.empty() || P.N > 64) return false;
  const auto& E = P.emits[0];
  for (int o = 0; o <= E.M; o++)
    for (int x = 0; x < P.N; x++) {
      double best = 0.0;
      for (int y = 0; y < P.N; y++)
        best = std::max(best, P.A64[x * 64 + y] * (o < E.M ? E.E[(size_t)o * 64 + y] : E.s[y]));
      if (!(best >= 1e-30)) return false;
    }
  return true;
}

// The observed columns' children: every one a leaf child of a plan of at most
// four, none twice.  seen[k]: child k is observed; *rows: the sum of their
// cardinalities M_k.
bool observed_children(const ChainPlan& P, const Route& r, bool (&seen)[4], int* rows) {
  for (bool& s : seen) s = false;
  *rows = 0;
  if (P.emits.size() > 4) return false;
  for (int i = 0; i < r.ncol; i++) {
    const int k = r.emit[i];
    if (k < 0 || k >= (int)P.emits.size() || seen[k]) return false;
    seen[k] = true;
    *rows += P.emits[k].M;
  }
  return true;
}

// How much one step can shrink a message: for every previous state x, the
// largest over y of A[x][y] times the smallest evidence any code combination
// gives y (per observed column the smallest of its rows, missing included;
// the unobserved children's row sums); the smallest of these over x.  A vector
// whose largest entry is m has one of at least m * step_shrink after a step
// (the bound of estep16_sparse_ok at several columns).  0 beyond 64 states.
double step_shrink(const ChainPlan& P, const Route& r) {
  if (P.N > 64) return 0.0;
  std::vector<double> ev(P.N, 1.0);
  for (int k = 0; k < (int)P.emits.size(); k++) {
    bool seen = false;
    for (int i = 0; i < r.ncol; i++) seen |= r.emit[i] == k;
    if (!seen)
      for (int y = 0; y < P.N; y++) ev[y] *= P.emits[k].s[y];
  }
  for (int i = 0; i < r.ncol; i++) {
    const auto& E = P.emit(r.emit[i]);
    for (int y = 0; y < P.N; y++) {
      double lo = E.s[y];
      for (int o = 0; o < E.M; o++) lo = std::min(lo, E.E[(size_t)o * 64 + y]);
      ev[y] *= lo;
    }
  }
  double shrink = 1.0;
  for (int x = 0; x < P.N; x++) {
    double best = 0.0;
    for (int y = 0; y < P.N; y++) best = std::max(best, P.A64[x * 64 + y] * ev[y]);
    shrink = std::min(shrink, best);
  }
  return shrink >= 0.0 ? shrink : 0.0;               // (a NaN table entry: no bound)
}

// The step-shrink bound, the one verdict that routes a request by its tables'
// values.  Kernels that rescale their messages every 4th step only
// (chain_fb_ckpt_kernel, chain_fb_mfma_kernel, chain_fb_ckw_kernel,
// chain_row64_kernel, chain_estep_ckw_kernel; chain_estep_ck_kernel through
// estep16_sparse_ok) take a request whose step_shrink is at least 1e-30:
// either direction's vector then keeps its largest entry above 1e-120 between
// rescales, the products of the two directions' vectors stay far above the
// subnormals, and so do the four-step products of step masses their ll
// mantissas hold.  Any other request goes to a kernel that rescales and
// renormalises at every step, as the reference does.
bool step_shrink_ok(double shrink) { return shrink >= kStepShrinkSparse; }

// A chain plan the general 16-state chain e_step takes: one interface
// variable of at most 16 states, 1..3 leaf children, hidden independent
// parents (their families follow from the xi sums, ensure_chain_map).
bool estep_general_plan(const ChainPlan& P) {
  return P.valid && !P.joint && !P.hmm && P.N <= 16 && !P.emits.empty() && P.emits.size() <= 3 &&
         !P.fold_gpu;
}
// the count-table rows of every child: sum_k (M_k + 2)
int estep_rows(const ChainPlan& P) {
  int R = 0;
  for (const auto& e : P.emits) R += e.M + 2;
  return R;
}

// the slab -> em_learn projection's structural preconditions (ensure_chain_map's checks)
bool chain_map_supported(const Model& m) {
  const auto& P = m.chain;
  if (!P.valid || P.joint || P.c_trans < 0) return false;
  for (int v : m.cliques[P.c_trans].vars)
    if (v != P.v_prev && v != P.v_cur && std::find(P.hidden.begin(), P.hidden.end(), v) == P.hidden.end())
      return false;
  if (!m.vars[P.v_prev].parents.empty()) return false;
  for (const auto& E : P.emits) {
    const auto& Vo = m.vars[E.var];
    if (Vo.parents.size() != 1 || Vo.parents[0] != P.v_cur) return false;
  }
  for (int v = 0; v < (int)m.vars.size(); v++) {
    const bool known = v == P.v_prev || v == P.v_cur ||
                       std::find(P.hidden.begin(), P.hidden.end(), v) != P.hidden.end() ||
                       std::any_of(P.emits.begin(), P.emits.end(), [&](const ChainEmit& e) { return e.var == v; });
    if (!known) return false;
  }
  return true;
}

// A chain plan the wide chain e_step takes (estep_wide.hip): one interface
// variable of at most 64 states, 1..4 leaf children, hidden independent
// parents, in-cliques folded on the GPU (config 3's and config 5's models).
bool estep_wide_plan(const Model& m) {
  const auto& P = m.chain;
  return P.valid && !P.joint && !P.emits.empty() && P.emits.size() <= 4 &&
         estep_wide_fits(P.N, estep_rows(P)) && chain_map_supported(m);
}

bool has_chain_estep(const Model& m) {
  const auto& P = m.chain;
  return P.valid && (P.hmm || P.jhmm || estep_general_plan(P) || estep_wide_plan(m));
}

// ---- kernel choice

// LDS limits of the kernels that do not raise theirs to the CU's (kLdsPerCU):
// chain_kernel (chain_kernels.hip, the round-2 16-lane DPP kernel) and
// chain_wide_kernel (chain_wide.hip, static LDS)
constexpr size_t kLdsDppKernel = 96 * 1024;
constexpr size_t kLdsWideKernel = 64 * 1024;

// fb kernel choice: the matrix-core kernels (chain_fb_ckpt_kernel for 16-wide
// posterior rows, NIPAMD_FB_KERNEL=scratch for chain_fb_mfma_kernel) unless NIPAMD_FB_KERNEL=dpp
// (the 16-lane DPP kernel, kept for the e_step and for A/B measurements)
static bool use_mfma() {
  static const bool v = [] {
    const char* e = diag_env("NIPAMD_FB_KERNEL");
    return !(e && std::string(e) == "dpp");
  }();
  return v;
}

ChainKernel pick_kernel(const nipamd_model* mm, const Route& r, const ReqTables* rt, int T, bool filt) {
  const auto& P = mm->m.chain;
  static const bool force_wide = [] {
    const char* e = diag_env("NIPAMD_FB_KERNEL");
    return e && std::string(e) == "wide";
  }();
  // below the step-shrink bound only kernels that rescale at every step:
  // chain_mfma_wide_kernel for the narrow requests too, chain_wide_kernel at
  // any width (kWide64Step), and the general engine where neither fits
  const bool sparse = step_shrink_ok(rt->shrink);
  if ((!r.narrow || filt || !sparse) && P.N <= 32 && !force_wide &&
      chain_mfma_wide_lds_bytes(P.N <= 16 ? 1 : 2, rt->mtab_rows, r.ncol, T) <= kLdsPerCU)
    return kMfmaWide;
  if (r.narrow && !filt && sparse) {
    if (use_mfma() && chain_mfma_lds_bytes(rt->M0, T) <= kLdsPerCU) return kNarrowMfma;
    if (chain_lds_bytes(rt->M0, T, false) <= kLdsDppKernel) return kNarrowDpp;
  }
  if (chain_wide_lds_bytes(r.ncol, T) <= kLdsWideKernel) return sparse ? kWide64 : kWide64Step;
  return kNoChain;
}

// kMfmaWide: chain_fb_ckw_kernel (round 6) before chain_mfma_wide_kernel --
// smoothing at 17..32 states with one or two observed columns where every
// recursion may rescale every 4th step (step_shrink_ok): checkpoints +
// recomputation, no message round trip.  NIPAMD_FB_WIDE_KERNEL=mw in
// diagnostics builds keeps chain_mfma_wide_kernel.  The launcher may still
// refuse (kLaunchRefused): then chain_mfma_wide_kernel serves the request.
bool fb_ckw_ok(const ChainPlan& P, const Route& r, const ReqTables* rt, bool filt, bool has_dst) {
  if (P.N <= 16 || filt || !has_dst || r.ncol < 1 || r.ncol > 2) return false;
  bool seen[4];
  int rows = 0;
  if (!observed_children(P, r, seen, &rows)) return false;
  const char* wk = diag_env("NIPAMD_FB_WIDE_KERNEL");
  return !(wk && std::string(wk) == "mw") && step_shrink_ok(rt->shrink);
}

#ifndef NIPAMD_FB_CKW_VL
#define NIPAMD_FB_CKW_VL 1          // A/B builds: 0 = the recomputed messages in registers, one wave per SIMD
#endif
bool fb_ckw_vl() {
  const char* vl = diag_env("NIPAMD_FB_CKW_VL");
  return vl ? std::atoi(vl) != 0 : NIPAMD_FB_CKW_VL != 0;
}

// e_step kernel of the chain route: kEstep16 = chain_estep16_kernel (16-lane
// DPP rows, direction-uniform waves, analytic phase-B normalisation; the
// default), kEstepDpp8 = chain_kernel<true> (the round-2 DPP kernel,
// mixed-direction waves; NIPAMD_ESTEP_KERNEL=dpp8 in diagnostics builds, or
// when the 16-seq block's LDS does not fit), kEstepMfma = the matrix-core
// kernel (NIPAMD_ESTEP_KERNEL=mfma).  Measured on config 4.
EstepKernel chain_estep_kernel(const nipamd_model* mm, int T) {
  const auto& P = mm->m.chain;
  if (estep_general_plan(P))                       // only chain_estep16_kernel takes several children
    return chain_estep16_lds_bytes(estep_rows(P) - 2, T, (int)P.emits.size()) <= kLdsPerCU ? kEstep16 : kEstepNone;
  const int M = P.emits[0].M;
  const char* ek = diag_env("NIPAMD_ESTEP_KERNEL");
  const std::string want = ek ? ek : "";
  // kEstepCk = chain_estep_ck_kernel (checkpoints + recomputation, round 6):
  // the default where both recursions may rescale every 4th step (the host's
  // underflow bound) and its count tables fit; NIPAMD_ESTEP_KERNEL=e16 in
  // diagnostics builds runs chain_estep16_kernel instead
  if (want != "mfma" && want != "dpp8" && want != "e16" && P.N <= 16 && P.hmm &&
      chain_estep_ck_lds_bytes(M) <= kLdsPerCU && estep16_sparse_ok(P, 1))
    return kEstepCk;
  if (want == "mfma" && P.N <= 16 && M <= 16 && chain_estep_mfma_lds_bytes(M, T) <= kLdsPerCU) return kEstepMfma;
  if (want != "dpp8" && P.N <= 16 && chain_estep16_lds_bytes(M, T, 1) <= kLdsPerCU) return kEstep16;
  if (chain_lds_bytes(M, T, true) <= kLdsDppKernel) return kEstepDpp8;
  return kEstepNone;
}

bool chain_estep_ok(const nipamd_model* mm, int n_obs, const int* obs_vars, int T, Route& r) {
  std::string why;
  const auto& P = mm->m.chain;
  const bool general = estep_general_plan(P);
  if (mm->engine == NIPAMD_ENGINE_JTREE || !P.valid || !(P.hmm || P.jhmm || general)) return false;
  if (!route_request(mm, n_obs, obs_vars, 0, nullptr, r, why)) return false;
  if (general) {                                   // evidence on leaf children only (not on the interface)
    for (int i = 0; i < r.ncol; i++) if (r.emit[i] >= (int)P.emits.size()) return false;
  } else if (r.ncol > 1 || (r.ncol == 1 && r.emit[0] != 0)) {
    return false;                                  // evidence on the child only
  }
  // below the step-shrink bound: chain_estep16_kernel in its every-step mode
  // (engine_estep.cpp) or nothing -- the other kernels of this route go four
  // steps between rescales whatever the tables, and the wide chain e_step or
  // the general engine serves the request (estep_partial_routes)
  const EstepKernel ek = chain_estep_kernel(mm, T);
  if (ek != kEstepNone && ek != kEstep16 && ek != kEstepCk && !step_shrink_ok(step_shrink(P, r))) return false;
  return ek != kEstepNone;
}

// the wide chain e_step: evidence on leaf children only
bool wide_estep_ok(const nipamd_model* mm, int n_obs, const int* obs_vars, Route& r) {
  std::string why;
  const auto& P = mm->m.chain;
  if (mm->engine == NIPAMD_ENGINE_JTREE || !estep_wide_plan(mm->m)) return false;
  if (!route_request(mm, n_obs, obs_vars, 0, nullptr, r, why)) return false;
  for (int i = 0; i < r.ncol; i++) if (r.emit[i] >= (int)P.emits.size()) return false;
  return true;
}

}  // namespace nipamd::eng
