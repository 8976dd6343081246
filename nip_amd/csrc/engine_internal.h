// engine_internal.h -- what the engine's translation units share: the host
// side of the hot path behind the C-ABI (include/nip_amd.h).
//   engine.cpp        error string, model lifecycle and read accessors
//   engine_dev.cpp    device state: buffer pool, table uploads, scratch
//   engine_route.cpp  request routing and kernel choice (host data only)
//   engine_fb.cpp     fb / filter / mlss launch sites
//   engine_estep.cpp  e_step partial routes, CSR maps, finalize
//   engine_estep_soft.cpp  the e_step under soft evidence
//   engine_diag.cpp   diagnostics builds: phase-stamp buffers and reports
#pragma once

#include <hip/hip_runtime.h>

#include <deque>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "chain_kernels.h"
#include "diag.h"
#include "model.h"
#include "nip_amd.h"

// internal to the library: nothing of nipamd::eng is exported
#pragma GCC visibility push(hidden)
namespace nipamd::eng {

// ---- engine.cpp
int fail(int code, const std::string& msg);
// A launcher's nonzero return (chain_kernels.h): kLaunchRefused -- the host
// refused the request before queueing anything (a shape or LDS budget the
// kernel does not take) -- is NIPAMD_ERROR_UNSUPPORTED; anything else is a
// failed HIP call, NIPAMD_ERROR_DEVICE with HIP's last error.
int launch_fail(int rc, const char* what);
inline int launched(int rc, const char* what) { return rc ? launch_fail(rc, what) : 0; }

#define HIP_OK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return ::nipamd::eng::fail(NIPAMD_ERROR_DEVICE, std::string(#expr) + ": " +        \
                                                          hipGetErrorString(e_));         \
  } while (0)

// Device tables that depend on which children a request observes.
struct ReqTables {
  std::string key;                // emit index per observed column
  int M0 = 0;                     // narrow kernels: rows of Etab16 are M0 + 2
  double* Etab16 = nullptr;       // [(M0+2)][16]
  double* ts16 = nullptr;         // [16] w = A s_all (matrix-core kernel's ll)
  double* tabw = nullptr;         // wide kernel: per column [(M_k+2)][64], concatenated
  std::vector<size_t> tabw_off;
  double* ebase = nullptr;        // [64] product of the unobserved children's row sums
  // matrix-core wide kernel: per column [(M_k+2)][NP], column 0 times ebase
  // (a single [2][NP] pseudo column = ebase when nothing is observed)
  double* mtab = nullptr;
  int mtab_rows = 0;
  int mtab_off[4] = {0, 0, 0, 0};
  double* wv = nullptr;           // [64] A s_all
  double* u0 = nullptr;           // [64] pi A: the first slice's prediction (mlss, viterbi.hip)
  double shrink = 0.0;            // step_shrink of the route (host: the kernel choice reads it per request)
  double* arena = nullptr;        // the pool buffer all of the above live in (one upload)
};

struct DevState {
  int device = -1;
  unsigned version = 0;
  double* A = nullptr;            // [16][16]  (N <= 16)
  double* pi = nullptr;           // [16]
  double* A64 = nullptr;          // [64][64]
  double* pi64 = nullptr;         // [64]
  double* sall64 = nullptr;       // [64]
  double* arena = nullptr;        // the pool buffer A .. sall64 and childE live in (one upload)
  std::deque<ReqTables> reqs;      // deque: pointers returned by ensure_req_tables stay valid
  double* S = nullptr;
  size_t S_bytes = 0;
  double* R = nullptr;     // E-step partial [nipamd_estep_partial_size] of nipamd_estep
  int R_size = 0;
  double* W = nullptr;     // E-step work: slabs + tree levels + chunk results + partial
  size_t W_bytes = 0;
  double* Q = nullptr;     // derived marginals: interface marginals / forward messages
  size_t Q_bytes = 0;
  std::vector<double*> childE;   // per leaf child [(M+1)][64]: E, then the row sums
  std::vector<double*> G;        // per hidden parent [card][64][64], built on first use
  // joint-interface e_step finalize: the slab -> em_learn layout map (CSR)
  int* jm_ptr = nullptr;
  int* jm_idx = nullptr;
  double* jm_coef = nullptr;
  int jm_n = 0;
  int jm_kind = 0;                // 1 joint map, 2 16-state chain slab, 3 wide chain slab
  // general chain e_step (several leaf children, hidden parents): every
  // child's table, rows M_k + 2 each (E, the row sums, zeros), 16 columns
  double* etab_all = nullptr;
  // model-table buffers of earlier versions, kept for the next version's
  // tables of the same sizes (an em_learn iteration re-uploads every table
  // after its m_step: no hipMalloc / hipFree pair per table and iteration)
  std::unordered_map<void*, size_t> live;        // pool-managed buffers in use -> bytes
  std::vector<std::pair<void*, size_t>> pool;     // free ones
};

// A request's routing through the chain plan: which emission child each
// observation column is, and which kernel family serves it.
struct Route {
  int ncol = 0;                   // observed emission children
  int col[4] = {-1, -1, -1, -1};  // their columns in obs
  int emit[4] = {-1, -1, -1, -1}; // their plan.emits index
  int primary = -1;               // narrow kernels: the child whose table is used
  int pcol = -1;                  // its column (or -1: never observed)
  bool narrow = false;            // N <= 16 and at most one observed child
};

// device buffers of a host-buffer call, freed on every return path
struct DevBufs {
  std::vector<void*> p;
  template <typename T> int alloc(T** out, size_t n) {
    *out = nullptr;
    HIP_OK(hipMalloc(out, (n ? n : 1) * sizeof(T)));
    p.push_back(*out);
    return 0;
  }
  ~DevBufs() { for (void* q : p) (void)hipFree(q); }
};

// The host-buffer form of a device call (PCIe-inclusive, synchronous): the
// observations in (obs null: none), run(d_obs, d_out, d_ll, d_status) on
// device buffers, then out [n_out], ll [B] and status [B] back (each may be
// null).  out_in: out is copied in first (the e_step adds to its counts).
template <typename Out, typename Run>
int host_call(const int32_t* obs, size_t n_obs_words, Out* out, size_t n_out, bool out_in, double* ll,
              uint32_t* status, size_t B, Run run) {
  DevBufs db;
  int32_t* d_obs = nullptr; Out* d_out = nullptr; double* d_ll = nullptr; uint32_t* d_st = nullptr;
  if (int rc = db.alloc(&d_obs, n_obs_words)) return rc;
  if (int rc = db.alloc(&d_out, n_out)) return rc;
  if (int rc = db.alloc(&d_ll, B)) return rc;
  if (int rc = db.alloc(&d_st, B)) return rc;
  if (obs && n_obs_words) HIP_OK(hipMemcpy(d_obs, obs, n_obs_words * sizeof(int32_t), hipMemcpyHostToDevice));
  if (out_in) HIP_OK(hipMemcpy(d_out, out, n_out * sizeof(Out), hipMemcpyHostToDevice));
  const int rc = run(d_obs, d_out, d_ll, d_st);
  if (rc == 0) {
    HIP_OK(hipDeviceSynchronize());
    if (out && n_out) HIP_OK(hipMemcpy(out, d_out, n_out * sizeof(Out), hipMemcpyDeviceToHost));
    if (ll && B) HIP_OK(hipMemcpy(ll, d_ll, B * sizeof(double), hipMemcpyDeviceToHost));
    if (status && B) HIP_OK(hipMemcpy(status, d_st, B * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return rc;
}

// ---- engine_dev.cpp
void* dalloc(DevState* d, size_t bytes);
void dfree(DevState* d, void* p);
DevState* dev_of(nipamd_model* mm);
void dev_release(DevState* d);
int ensure_device(nipamd_model* mm);
int ensure_tables(nipamd_model* mm);
int ensure_hidden(nipamd_model* mm, int j);
int ensure_req_tables(nipamd_model* mm, const Route& r, ReqTables** out);
int ensure_scratch(nipamd_model* mm, size_t bytes);   // DevState::S
int ensure_q(nipamd_model* mm, size_t bytes);         // DevState::Q
int ensure_work(nipamd_model* mm, size_t bytes);      // DevState::W
int reduce_rows(const double* in, long n, int S, double* tA, double* tB, double* out, hipStream_t st);

template <typename V>
int upload(DevState* d, double** dst, const V& v) {
  *dst = static_cast<double*>(dalloc(d, (v.size() ? v.size() : 1) * sizeof(double)));
  if (!*dst) return fail(NIPAMD_ERROR_DEVICE, "device allocation failed");
  if (v.size()) HIP_OK(hipMemcpy(*dst, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

// ---- engine_route.cpp: routing, plan predicates and kernel choice (host data only)
int query_kind(const ChainPlan& P, int v);
int route_request(const nipamd_model* mm, int n_obs, const int* obs_vars, int n_query, const int* query,
                  Route& r, std::string& why);
// the verdicts mlss and the streams share: arguments, scope, a joint interface's query
int check_var_lists(const std::string& what, const nipamd_model* mm, bool null, const char* null_msg, bool bad,
                    const std::string& bad_msg, int n_obs, const int* obs_vars, int n_query, const int* query);
int chain_scope(const nipamd_model* mm, const std::string& what, const char* subject, const char* no_plan);
bool interface_digits(const nipamd_model* mm, int n_query, const int* query, int* qstride, int* qcard, int* width);
// mlss's query rule: exactly the interface; the path's columns
int interface_query(const std::string& what, const nipamd_model* mm, int n_query, const int* query, int* nq,
                    int* qstride, int* qcard);
// the verdicts soft evidence and the streams share, and the columns' roles: the evidence columns alone
// (a: ViterbiSoftArgs), and with the rows' query (a: SoftArgs or StreamSoftArgs)
template <typename A>
int soft_evidence_columns(const std::string& what, nipamd_model* mm, const char* subject, const char* no_plan,
                          int n_obs, const int* obs_vars, int n_soft, const int* soft_vars, A& a, Route& r);
template <typename A>
int soft_columns(const std::string& what, nipamd_model* mm, const char* subject, const char* no_plan, int n_obs,
                 const int* obs_vars, int n_soft, const int* soft_vars, int n_query, const int* query, A& a, Route& r,
                 int* width);
bool chain_proper(const ChainPlan& P);
bool estep16_sparse_ok(const ChainPlan& P, int ne);
// the step-shrink bound (engine_route.cpp): kernels that rescale every 4th
// step take requests at or above kStepShrinkSparse
constexpr double kStepShrinkSparse = 1e-30;
double step_shrink(const ChainPlan& P, const Route& r);
bool step_shrink_ok(double shrink);
bool observed_children(const ChainPlan& P, const Route& r, bool (&seen)[4], int* rows);
bool estep_general_plan(const ChainPlan& P);
int estep_rows(const ChainPlan& P);
bool chain_map_supported(const Model& m);
bool estep_wide_plan(const Model& m);
bool has_chain_estep(const Model& m);

// ---- engine_estep.cpp, for the e_step under soft evidence (engine_estep_soft.cpp): the wide route's
// partial (tag (0, 0, 1)) from one slab row [S] per sequence -- run_slab_chunks with per_row = 1 --
// pow2_chunk, and the most sequences of a launch
int wide_slab_chunks(nipamd_model* mm, int S, long chunk, size_t scratch, long B, double* d_partial, hipStream_t st,
                     const std::function<int()>& prepare, const std::function<int(long, long, double*)>& launch);
long estep_pow2_chunk(size_t per_seq, size_t budget, long lo, long hi);
long estep_chunk_limit();

// ---- engine_fb.cpp: sequences per chain_viterbi_kernel / chain_viterbi_soft_kernel launch
long mlss_chunk(int N, int T);

// Interface-chain kernel for a route, in order of preference; each kernel
// stages the block's observation codes in LDS, so a long sequence may not fit
// one and falls through to the next (the 64-state kernel last).  kNoChain:
// no chain kernel fits -- the request goes to the general engine.
// kWide64Step: kWide64 for a request below the step-shrink bound -- the
// one-wave kernel (chain_wide_kernel, which rescales at every step) at 33..64
// states too, where kWide64 runs chain_row64_kernel.
enum ChainKernel { kNoChain = 0, kMfmaWide, kNarrowMfma, kNarrowDpp, kWide64, kWide64Step };
ChainKernel pick_kernel(const nipamd_model* mm, const Route& r, const ReqTables* rt, int T, bool filt);
// kMfmaWide: chain_fb_ckw_kernel before chain_mfma_wide_kernel, and its LDS variant
bool fb_ckw_ok(const ChainPlan& P, const Route& r, const ReqTables* rt, bool filt, bool has_dst);
bool fb_ckw_vl();

// e_step kernel of the 16-state chain route (kEstepNone: none fits)
enum EstepKernel { kEstepNone = 0, kEstepMfma, kEstepDpp8, kEstep16, kEstepCk };
EstepKernel chain_estep_kernel(const nipamd_model* mm, int T);
bool chain_estep_ok(const nipamd_model* mm, int n_obs, const int* obs_vars, int T, Route& r);
bool wide_estep_ok(const nipamd_model* mm, int n_obs, const int* obs_vars, Route& r);

// The first `ne` leaf children of the plan in order: f(k, first count-table row
// of child k (rows M_k + 2 each), slot) with slot the route's entry observing
// the child (its column is r.col[slot]) or -1.
template <typename F>
void for_each_child(const ChainPlan& P, const Route& r, int ne, F f) {
  for (int k = 0, row = 0; k < ne; k++) {
    int slot = -1;
    for (int i = 0; i < r.ncol; i++) if (r.emit[i] == k) slot = i;
    f(k, row, slot);
    row += P.emits[k].M + 2;
  }
}

// run(d_lik) with the likelihood vectors lik [nli] on the device around it (a host-buffer call's)
template <typename Run>
int with_lik(const double* lik, size_t nli, Run run) {
  DevBufs db;
  double* d_lik = nullptr;
  if (int rc = db.alloc(&d_lik, nli)) return rc;
  if (nli) HIP_OK(hipMemcpy(d_lik, lik, nli * sizeof(double), hipMemcpyHostToDevice));
  const int rc = run(d_lik);
  if (rc == 0) HIP_OK(hipDeviceSynchronize());           // d_lik is freed on return
  return rc;
}

// ---- the views and evidence columns of the kernels' argument structs
// (chain_kernels.h: the fields are same-named across the structs)
template <typename A>
void set_obs_view(A& a, const int32_t* d_obs, int n_obs, int T, long b0 = 0) {
  const long ocols = n_obs > 0 ? n_obs : 1;
  a.obs = d_obs ? d_obs + b0 * T * ocols : nullptr;
  a.obs_bstride = (long)T * ocols;
  a.obs_tstride = (int)ocols;
}
template <typename A>
void set_post_view(A& a, double* dst, long bstride, int tstride, int off) {
  a.post = dst; a.post_bstride = bstride; a.post_tstride = tstride; a.post_off = off;
}
// one [(M+2)][64] table pointer per observed column, and ebase; the columns
// from nhard on are soft and keep their col (a.col[nhard..] must hold what soft_columns filled)
constexpr int kAllHard = 4;   // the columns of Route::col
template <typename A>
void set_cols(A& a, const ChainPlan& P, const Route& r, const ReqTables& rt, int nhard = kAllHard) {
  a.ncol = r.ncol;
  for (int i = 0; i < r.ncol; i++) {
    if (i < nhard) a.col[i] = r.col[i];
    a.M[i] = P.emit(r.emit[i]).M;
    a.tab[i] = rt.tabw + rt.tabw_off[i];
  }
  a.ebase = rt.ebase;
}
// one table `tab` holding column i's rows at off[i] doubles
template <typename A, typename Off>
void set_cols(A& a, const ChainPlan& P, const Route& r, const double* tab, const Off& off) {
  a.ncol = r.ncol;
  a.tab = tab;
  for (int i = 0; i < 4; i++) {
    a.col[i] = i < r.ncol ? r.col[i] : 0;
    a.M[i] = i < r.ncol ? P.emit(r.emit[i]).M : 0;
    a.tab_off[i] = i < r.ncol ? (int)off[i] : 0;
  }
}

#ifdef NIPAMD_DIAGNOSTICS
// ---- engine_diag.cpp: per-block phase stamps (NIPAMD_PHASE_TIMES=1) and their reports
bool phase_times();
using Stamps = std::vector<unsigned long long>;
struct StampBuf {
  unsigned long long* dev = nullptr;
  size_t n = 0;
  // want: `words` stamps, zeroed on st, their address into the kernel's argument *slot
  int attach(bool want, size_t words, hipStream_t st, unsigned long long** slot);
  int fetch(hipStream_t st, Stamps& h);                // after a stream sync
  // attached: fetch, then report(stamps, count)
  template <typename Report, typename N>
  int report(hipStream_t st, Report rep, N count) {
    Stamps h;
    if (!dev) return 0;
    if (int rc = fetch(st, h)) return rc;
    rep(h, count);
    return 0;
  }
  StampBuf() = default;
  StampBuf(const StampBuf&) = delete;
  ~StampBuf() { (void)hipFree(dev); }
};
void report_phases(const Stamps& h, int nblk);          // chain_fb_mfma_kernel [block][24]
void report_ckpt_waves(const Stamps& w, int nblk);      // chain_fb_ckpt_kernel [block][8 waves][5]
void report_mfma_wide(const Stamps& h, int nblk);       // chain_mfma_wide_kernel [block][4 waves][4]
void report_wide4(const Stamps& h, long B);             // chain_wide4 [block][16]
// the 16-state e_step kernels' stamps of a launch of nb sequences (0 words: none)
size_t estep_stamp_words(EstepKernel ek, long nb);
void report_estep(const Stamps& h, std::pair<EstepKernel, long> ek_nb);
#endif

}  // namespace nipamd::eng
#pragma GCC visibility pop
