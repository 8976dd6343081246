// viterbi.hip -- most likely state sequence of an interface chain (mlss, the
// reference's declared and never implemented Viterbi / max-sum inference,
// src/nip.h:431-438, src/nip.c:1620-1699), batched over sequences.
//
// Over the chain plan's tables (compile.cpp; the wide request tables of
// engine.cpp ensure_req_tables) the marginal MAP of the interface sequence is
//
//   u0[y]      = sum_x pi[x] A[x][y]                     (host)
//   e_t[y]     = ebase[y] prod_k tab_k[code_k,t][y]      (code: state, M = missing, M + 1 = out of range)
//   delta_0[y] = u0[y] e_0[y]
//   delta_t[y] = (max_x delta_{t-1}[x] A[x][y]) e_t[y],  psi_t[y] = the lowest x attaining the max
//   x*_{T-1}   = the lowest y attaining max_y delta_{T-1}[y],  x*_{t-1} = psi_t[x*_t]
//   logp       = ln max_y delta_{T-1}[y]
//
// in the probability domain, fp64, multiplies and compares only.  delta is
// rescaled by an exact power of two every step -- the exponent of the row
// maximum of delta_{t-1} is taken out of delta_t, one step late, so that the
// reduction runs beside the products instead of ahead of them -- and the
// exponents are summed into logp.  A power of two changes no comparison, so
// ties (the lowest index wins) do not depend on the scaling or the lane layout.
//
// Layout: chain_group.h's lane groups (NP = 16, 32 or 64 padded states, one
// NP-lane group per sequence).  Column y of A stays in registers.
// delta_{t-1}[x] reaches every lane of its group through a 64-bit DPP
// row_newbcast operand at NP = 16 (dpp_row.h's
// v_fmac_f64_dpp onto a zero accumulator: fma(a, b, 0) is the rounded product)
// and through the wave's own LDS row above that.  The evidence tables are
// staged in LDS.  The raw observations of step t + 2 are loaded during step t
// and only turned into table rows (and e_{t+2} read from LDS) at the top of
// step t + 1, so each load has a whole step to land; the kernel is
// instantiated per column count so that these loads sit in no branch.
//
// Back-pointers: log2(NP) bit planes per step, plane k = the wave's ballot of
// bit k of psi_t -- one 64-bit word per plane covering all the wave's
// sequences, 4 bits per state at NP = 16 (8 bytes per sequence and step; 20 and
// 48 bytes at NP = 32 and 64).  A wave's words are contiguous in (t, plane)
// order, collected in registers (lane l holds word l of the current run of
// 64 / log2(NP) steps) and stored a run at a time.  The same wave backtracks:
// it reloads its words a run ahead of their use -- the addresses do not depend
// on the decoded states -- broadcasts each step's planes with v_readlane and
// extracts bit (group base + x*_t) of each.  The path is collected 16 steps
// per group and stored as int32, one column per queried variable (a joint
// interface's digits).  The max-product step and the words' geometry:
// viterbi_group.h, with chain_viterbi_soft_kernel (viterbi_soft.hip).
#include <hip/hip_runtime.h>

#include <cfloat>

#include "viterbi_group.h"

namespace nipamd {

namespace {

// NC = the observed columns (a.ncol): a constant, so that the observation loads
// are unconditional and stay in flight over a whole step
template <int NP, int NC>
__global__ __launch_bounds__(kGroupWaves * 64) void chain_viterbi_kernel(ViterbiArgs a) {
  constexpr int LOG = vit_log(NP), SPF = 64 / LOG, RUN = SPF * LOG, G = 64 / NP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* tabs = reinterpret_cast<double*>(smem);        // [rows][NP], ebase [NP], then [waves][64] (NP > 16)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.T;
  constexpr int NCA = NC > 0 ? NC : 1;
  // chain_group.h's stage_tables, written out: through the helper the compiler
  // schedules this kernel's step loops differently at every NP (it leaves
  // chain_stream_kernel's code as it is), and mlss measured up to 3.8 % slower
  // (64 states)
  int row0[NCA], rows = 0;
#pragma unroll
  for (int k = 0; k < NC; k++) {
    row0[k] = rows;
    const int n = (a.M[k] + 2) * NP;
    for (int i = tid; i < n; i += kGroupWaves * 64) tabs[rows * NP + i] = a.tab[k][(i / NP) * 64 + (i % NP)];
    rows += a.M[k] + 2;
  }
  double* eb = tabs + rows * NP;
  if (tid < NP) eb[tid] = a.ebase[tid];
  double* xch = eb + NP + wave * 64;
  __syncthreads();

  const int grp = lane / NP, y = lane % NP, gbase = grp * NP;
  const long gw = (long)blockIdx.x * kGroupWaves + wave; // the wave's sequences: gw G .. gw G + G - 1
  if (gw * G >= a.B) return;
  const long b = gw * G + grp;
  const bool live = b < a.B;
  const int* ob = a.obs + (live ? b : a.B - 1) * a.obs_bstride;

  double Ac[NP];
#pragma unroll
  for (int x = 0; x < NP; x++) Ac[x] = a.A[x * 64 + y];

  // Step t's raw observations (t clamped into the sequence): loads only, so
  // that nothing waits for them here.  evid turns them into table rows and e_t
  // a whole step later, where the wait for the loads lands.
  auto fetch = [&](int t, int (&o)[NCA]) {
    t = t < T ? t : T - 1;
#pragma unroll
    for (int k = 0; k < NC; k++) o[k] = ob[(long)t * a.obs_tstride + a.col[k]];
  };
  auto evid = [&](const int (&o)[NCA]) {
    double e = eb[y];
#pragma unroll
    for (int k = 0; k < NC; k++) e *= tabs[(row0[k] + code_of(o[k], a.M[k])) * NP + y];
    return e;
  };

  int on[NCA] = {};
  fetch(0, on);
  double d = a.u0[y] * evid(on);                          // delta_0
  fetch(1, on);
  double en = evid(on);                                   // e_1
  fetch(2, on);
  long esum = 0;
  unsigned long long* bpw = a.bp + gw * vit_wave_words(NP, T);
  const long nwords = (long)T * LOG;
  unsigned long long w = 0;                               // lane l: word l of the current run
  int slot = LOG;                                         // step t's first word within the run
  long wbase = 0;                                         // the run's first word
  for (int t = 1; t < T; t++) {
    const double e = en;
    en = evid(on);                                        // e_{t+1}, from the observations fetched a step ago
    fetch(t + 2, on);
    double m, best;
    int arg;
    vit_step<NP>(d, Ac, xch, lane, gbase, m, best, arg);
    int ex = 0;
    (void)frexp(m, &ex);                                  // 0 for m == 0
    d = ldexp(best * e, -ex);
    esum += ex;
#pragma unroll
    for (int k = 0; k < LOG; k++) {
      const unsigned long long bk = __ballot((arg >> k) & 1);
      if (lane == slot + k) w = bk;
    }
    slot += LOG;
    if (slot == RUN || t == T - 1) {
      if (lane < RUN && wbase + lane < nwords) bpw[wbase + lane] = w;
      wbase += RUN;
      slot = 0;
    }
  }

  // the final maximum, its lowest state, logp
  double m;
  if constexpr (NP == 16) {
    m = row_max(d);
  } else {
    xch[lane] = d;
    wave_lds_sync();
    m = 0.0;
#pragma unroll
    for (int x = 0; x < NP; x++) m = fmax(m, xch[gbase + x]);
  }
  const bool dead = !(m > 0.0);
  unsigned long long hit = __ballot(d == m) >> gbase;
  if (NP < 64) hit &= (1ull << (NP & 63)) - 1;
  int x = hit ? __builtin_ctzll(hit) : 0;
  if (live && y == 0) {
    if (a.logp) a.logp[b] = dead ? -DBL_MAX : log(m) + (double)esum * 0.693147180559945309417232121458;
    if (a.status) a.status[b] = dead ? 1u : 0u;
  }

  // backtrack: the wave's own words, read past the vector L1 (agent scope)
  // once its stores have been made visible
  __threadfence();
  auto run_load = [&](int c) -> unsigned long long {
    const long i = (long)c * RUN + lane;
    if (c < 0 || lane >= RUN || i >= nwords) return 0ull;
    return __hip_atomic_load(bpw + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  int c = (T - 1) / SPF;
  unsigned long long wc = run_load(c), wn = run_load(c - 1);
  int xs = 0;                                             // lane y < 16: x*_t of the step t = y (mod 16) in flight
  int* prow = a.path + (live ? b : 0) * a.path_bstride;
  for (int t = T - 1;; t--) {
    if (y == (t & 15)) xs = x;
    if ((t & 15) == 0 && live && y < 16 && t + y < T)
      for (int j = 0; j < a.nq; j++)
        prow[(long)(t + y) * a.path_tstride + j] = dead ? -1 : (xs / a.qstride[j]) % a.qcard[j];
    if (t == 0) break;
    if (t < c * SPF) {
      c--;
      wc = wn;
      wn = run_load(c - 1);
    }
    const int s = (t - c * SPF) * LOG;
    int xn = 0;
#pragma unroll
    for (int k = 0; k < LOG; k++) xn |= (int)((readlane64(wc, s + k) >> (gbase + x)) & 1) << k;
    x = xn;
  }
}

}  // namespace

size_t chain_viterbi_scratch_bytes(int N, long B, int T) {
  const int NP = group_np(N), G = 64 / NP;
  return (size_t)((B + G - 1) / G) * vit_wave_words(NP, T) * sizeof(unsigned long long);
}

size_t chain_viterbi_lds_bytes(const ViterbiArgs& a) {
  const int NP = group_np(a.N);
  return (evid_rows(a) * NP + (NP > 16 ? kGroupWaves * 64 : 0)) * sizeof(double);
}

int chain_viterbi_launch(const ViterbiArgs& a, hipStream_t stream) {
  if (!cols_shape_ok(a) || a.nq < 1 || a.T < 1) return kLaunchRefused;
  g_last_kernel = "chain_viterbi_kernel";
  return group_launch(a, chain_viterbi_lds_bytes(a), true, stream, [](auto np, auto nc) {
    return &chain_viterbi_kernel<decltype(np)::value, decltype(nc)::value>;
  });
}

}  // namespace nipamd
