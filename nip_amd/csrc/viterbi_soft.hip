// viterbi_soft.hip -- most likely state sequence of an interface chain under
// soft (likelihood) evidence (nipamd_mlss_soft, engine_soft.cpp), batched over
// sequences: viterbi.hip's recursion with soft.hip's step evidence,
//
//   e_t[y]     = ebase[y]  prod_hard E_k[o_{k,t}][y]  prod_soft sum_o w_{k,t}[o] E_k[o][y]
//   delta_0[y] = u0[y] e_0[y]
//   delta_t[y] = (max_x delta_{t-1}[x] A[x][y]) e_t[y],  psi_t[y] = the lowest x attaining the max
//   logp       = ln max_y delta_{T-1}[y]
//
// -- the marginal MAP of the interface sequence with the children summed out,
// a soft child under its weights.  Every soft vector is used at the scale of
// its largest valid weight (soft_evid: w 2^-ex, exact) and the exponents taken
// out are added to the recursion's own exponent sum before logp is formed:
// multiplying a step's vector by 2^k leaves e_t, every comparison and the path
// the same bits and adds k ln 2 to logp, for any finite non-negative vector
// with a positive entry (denormals to DBL_MAX).  All ones is the missing row,
// a one-hot vector a hard observation.  A weight that is negative, NaN or
// infinite leaves its step without evidence (e_t = 0): the sequence has no
// mass -- path -1, logp = -DBL_MAX -- and gets kSoftBadEvidence besides the
// zero-mass bit.
//
// Layout, recursion, back-pointers, backtrack and path stores are
// chain_viterbi_kernel's (viterbi.hip, whose body stays its own: its comments
// say what re-shaping it costs): chain_group.h's lane groups, column y of A in
// registers, delta_{t-1} through DPP row_newbcast operands at NP = 16 and the
// wave's LDS row above that, delta rescaled by the exact power of two of the
// previous row maximum, log2(NP) ballot bit planes per step, the same wave
// backtracking its own words.  The hard columns come first and their number is
// a template parameter (soft.hip).  Step t + 2's codes and weights (a vector's
// first NP; a longer vector's later pieces on demand, LONG) are loaded during
// step t and turned into e_{t+2} at the top of step t + 1, so each load has a
// whole step to land.  A sequence's results depend on its own inputs alone,
// bit for bit: every cross-lane operation stays inside the group.
//
// LDS: the evidence tables, ebase, and two [64] rows per wave -- the exchange
// row of the step (NP > 16) and the weight row of soft_evid.  No image of A.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "soft_group.h"
#include "viterbi_group.h"

namespace nipamd {

namespace {

template <int NP, int NC, int NH, bool LONG>
__global__ __launch_bounds__(kGroupWaves * 64) void chain_viterbi_soft_kernel(ViterbiSoftArgs a) {
  static_assert(NH >= 0 && NH <= NC, "the hard columns are the first of the columns");
  constexpr int LOG = vit_log(NP), SPF = 64 / LOG, RUN = SPF * LOG, G = 64 / NP;
  constexpr int NCA = NC > 0 ? NC : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [rows][NP] tables, ebase [NP], [waves][64] exchange rows, [waves][64] weight rows
  double* tabs = reinterpret_cast<double*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.T;
  int row0[NCA];
  double* eb = stage_tables<NP, NC>(a, tabs, tid, row0);
  double* xch = eb + NP + wave * 64;
  double* wrow = eb + NP + kGroupWaves * 64 + wave * 64;
  __syncthreads();

  const int grp = lane / NP, y = lane % NP, gbase = grp * NP;
  const long gw = (long)blockIdx.x * kGroupWaves + wave;   // the wave's sequences: gw G .. gw G + G - 1
  if (gw * G >= a.B) return;
  const long b = gw * G + grp;
  const bool live = b < a.B;
  const long bl = live ? b : a.B - 1;
  const int* orow = a.obs + bl * a.obs_bstride;
  const double* lrow = a.lik + bl * a.lik_bstride;

  double Ac[NP];
#pragma unroll
  for (int x = 0; x < NP; x++) Ac[x] = a.A[x * 64 + y];

  // Step t's loads (t clamped into the sequence) and, a whole step later, its
  // e_t.  The step's exponents and bad flag go to the totals once: a step past
  // the end is step T - 1 again and adds nothing.
  using Step = SoftStep<NCA>;
  long esum = 0;
  unsigned status = 0u;
  auto fetch = [&](int t, Step& s) { soft_fetch<NP, NC, NH>(a, orow, lrow, y, t < T ? t : T - 1, s); };
  auto evid = [&](int t, const Step& s) {
    bool bad;
    long exs;
    const double e =
        soft_evid<NP, NC, NH, LONG>(a, tabs, eb, row0, wrow, lrow, lane, gbase, y, t < T ? t : T - 1, s, bad, exs);
    if (t < T) {
      esum += exs;
      if (bad) status |= kSoftBadEvidence;
    }
    return e;
  };

  Step on;
  fetch(0, on);
  double d = a.u0[y] * evid(0, on);                        // delta_0
  fetch(1, on);
  double en = evid(1, on);                                 // e_1
  fetch(2, on);
  unsigned long long* bpw = a.bp + gw * vit_wave_words(NP, T);
  const long nwords = (long)T * LOG;
  unsigned long long w = 0;                                // lane l: word l of the current run
  int slot = LOG;                                          // step t's first word within the run
  long wbase = 0;                                          // the run's first word
  for (int t = 1; t < T; t++) {
    const double e = en;
    en = evid(t + 1, on);                                  // e_{t+1}, from the loads of a step ago
    fetch(t + 2, on);
    double m, best;
    int arg;
    vit_step<NP>(d, Ac, xch, lane, gbase, m, best, arg);
    int ex = 0;
    (void)frexp(m, &ex);                                   // 0 for m == 0
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
    if (a.status) a.status[b] = status | (dead ? 1u : 0u);
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
  int xs = 0;                                              // lane y < 16: x*_t of the step t = y (mod 16) in flight
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

bool viterbi_soft_shape_ok(const ViterbiSoftArgs& a) {
  return cols_shape_ok(a) && a.nq >= 1 && a.T >= 1 && a.nhard >= 0 && a.nhard <= a.ncol;
}

int viterbi_soft_dispatch(const ViterbiSoftArgs& a, bool launch, hipStream_t stream) {
  return soft_group_launch(
      a, launch, stream,
      [](auto np, auto nc, auto nh, auto lng) {
        return &chain_viterbi_soft_kernel<decltype(np)::value, decltype(nc)::value, decltype(nh)::value,
                                          decltype(lng)::value>;
      },
      chain_viterbi_soft_lds_bytes(a));
}

}  // namespace

size_t chain_viterbi_soft_lds_bytes(const ViterbiSoftArgs& a) {
  return (evid_rows(a) * group_np(a.N) + 2 * (size_t)kGroupWaves * 64) * sizeof(double);
}

int chain_viterbi_soft_prepare(const ViterbiSoftArgs& a) {
  if (!viterbi_soft_shape_ok(a)) return kLaunchRefused;
  return viterbi_soft_dispatch(a, false, nullptr);
}

int chain_viterbi_soft_launch(const ViterbiSoftArgs& a, hipStream_t stream) {
  if (!viterbi_soft_shape_ok(a) || !a.path || !a.bp || (a.nhard > 0 && !a.obs) || (a.nhard < a.ncol && !a.lik))
    return kLaunchRefused;
  g_last_kernel = "chain_viterbi_soft_kernel";
  return viterbi_soft_dispatch(a, true, stream);
}

}  // namespace nipamd
