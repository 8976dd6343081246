// estep_soft.hip -- the e_step's expected counts under soft (likelihood)
// evidence over an interface chain, batched over whole sequences
// (nipamd_estep_soft_partial, engine_estep_soft.cpp).
//
// The evidence is soft.hip's: hard columns pick a row of their child's table,
// a soft column enters as the weighted sum of the state rows, every vector at
// the scale of its largest weight (soft_group.h soft_evid).  The forward pass
// is chain_soft_kernel's fb form: alpha^_t to scratch [B][T][NP], the ll as two
// mantissa products and one exponent.  The backward pass recomputes e_t and,
// instead of writing rows, accumulates the three sums of the wide slab
// (estep_wide.hip: K [NP][NP], H [R][NP], P0 [NP]), one slab row per sequence.
// With g = e_t o beta_t (beta at any power-of-two scale) and v = A g, at step t
//
//   Z_t        = sum_x alpha^_{t-1}[x] v[x]               (alpha^_{-1} = prior)
//   K[x][y]   += alpha^_{t-1}[x] g[y] / Z_t               (no transition factor)
//   gamma_{t-1}[x] = alpha^_{t-1}[x] v[x] / Z_t           (gamma_{T-1} = alpha^_{T-1}; gamma_{-1} = P0)
//   H_k[code][y] += gamma_t[y]                            child k hard: code_of's row
//   H_k[o][y] += gamma_t[y] w[o] E_k[o][y] / sum_o' w[o'] E_k[o'][y]      child k soft
//   H_k[missing][y] += gamma_t[y]                         child k named by no column
//
// Z_t is the normaliser of gamma_{t-1} and comes from the backward step's
// un-rescaled output v, whose scale is g's: every quotient is free of beta's
// scale, and of the weights' (the ldexp-scaled weights are the same bits for w
// and 2^j w), so a partial is the same bits for both.  Each term w E / sum is at
// most 1 whatever the sizes of its parts.
//
// Layout: chain_group.h's lane groups (NP = 16, 32 or 64 padded states, one
// NP-lane group per sequence, lane y = state y).  Lane y keeps column y of K
// in NP registers, alpha^_{t-1} reaching it through the wave's LDS row; the H
// accumulators are indexed by data and live in LDS, R NP doubles per sequence,
// lane y reading and writing column y alone -- so they need no barrier.  The
// rows of children that no column names are one register sum, stored at the
// end.  Nothing is summed across sequences: a slab row depends on its own
// sequence's inputs alone, bit for bit; the fixed-order tree (engine_estep.cpp)
// sums the rows.
#include <hip/hip_runtime.h>

#include "soft_group.h"

namespace nipamd {

namespace {

// soft_evid's e_t of step t (the same operations in the same order: the same
// bits), which also adds the step's gamma = gamma_t[y] to the count tables Hl
// (this sequence's [R][NP], column y): a hard column's to row code_of of its
// child, a soft column's to the child's state rows in proportion w[o] E[o][y]
// (0 where their sum is 0).  A bad weight counts as 0, as in soft_evid: its
// sequence is dead by the forward pass and its slab all zero.
template <int NP, int NC, int NH, bool LONG>
__device__ __forceinline__ double soft_evid_counts(const EstepSoftArgs& a, double* const& tabs, double* const& eb,
                                                   const int (&row0)[NC > 0 ? NC : 1], double* const& wrow,
                                                   const double* const& lrow, double* const& Hl, const int& lane,
                                                   const int& gbase, const int& y, int t,
                                                   const SoftStep<(NC > 0 ? NC : 1)>& s, double gamma) {
  double e = eb[y];
#pragma unroll
  for (int k = 0; k < NC; k++) {
    if (k < NH) {
      const int c = code_of(s.code[k], a.M[k]);
      e *= tabs[(row0[k] + c) * NP + y];
      Hl[(a.hrow[k] + c) * NP] += gamma;
    } else {
      const int M = a.M[k];
      const double* tk = tabs + row0[k] * NP + y;
      double* hk = Hl + a.hrow[k] * NP;
      auto valid = [&](double w) { return !(w >= 0.0 && w <= DBL_MAX) ? 0.0 : w; };
      auto later = [&](int c0) {
        return lrow[(long)t * a.lik_tstride + a.col[k] + (c0 + y < M ? c0 + y : 0)];
      };
      const double w0 = valid(s.w[k]);
      double mx = w0;
      if constexpr (LONG)
        for (int c0 = NP; c0 < M; c0 += NP) mx = fmax(mx, valid(later(c0)));
      int ex = 0;
      (void)frexp(group_max<NP>(mx), &ex);               // 0 for a maximum of 0
      double acc = 0.0;
      // the weights o = c0 .. c0 + n - 1, this lane's being w: their sum (counts false), then their shares
      auto piece = [&](double w, int c0, bool counts) {
        wrow[lane] = ldexp(w, -ex);
        wave_lds_sync();
        const int n = M - c0 < NP ? M - c0 : NP;
        if (!counts) {
          for (int o = 0; o < n; o++) acc = fma(wrow[gbase + o], tk[(c0 + o) * NP], acc);
        } else if (acc > 0.0) {
          for (int o = 0; o < n; o++) hk[(c0 + o) * NP] += gamma * (wrow[gbase + o] * tk[(c0 + o) * NP] / acc);
        }
        wave_lds_sync();
      };
      if constexpr (LONG) {
        piece(w0, 0, false);
        for (int c0 = NP; c0 < M; c0 += NP) piece(valid(later(c0)), c0, false);
        piece(w0, 0, true);
        for (int c0 = NP; c0 < M; c0 += NP) piece(valid(later(c0)), c0, true);
      } else {
        // one piece: the shares from the weights already in the row
        wrow[lane] = ldexp(w0, -ex);
        wave_lds_sync();
        const int n = M < NP ? M : NP;
        for (int o = 0; o < n; o++) acc = fma(wrow[gbase + o], tk[o * NP], acc);
        if (acc > 0.0)
          for (int o = 0; o < n; o++) hk[o * NP] += gamma * (wrow[gbase + o] * tk[o * NP] / acc);
        wave_lds_sync();
      }
      e *= acc;
    }
  }
  return e;
}

// doubles of the count tables of a block: [waves][64 / NP sequences][R][NP]
inline size_t estep_soft_h_doubles(const EstepSoftArgs& a) { return (size_t)kGroupWaves * 64 * (size_t)a.R; }

template <int NP, int NC, int NH, bool LONG>
__global__ __launch_bounds__(kGroupWaves * 64) void chain_estep_soft_kernel(EstepSoftArgs a) {
  static_assert(NH >= 0 && NH <= NC, "the hard columns are the first of the columns");
  constexpr int NCA = NC > 0 ? NC : 1;
  constexpr int G = 64 / NP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // chain_soft_kernel's [rows][NP] tables, ebase [NP], A and A^T [NP][NP] (NP > 16), [waves][64] exchange
  // rows, [waves][64] weight rows; then the count tables [waves][G][R][NP]
  double* tabs = reinterpret_cast<double*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int row0[NCA];
  double* eb = stage_tables<NP, NC>(a, tabs, tid, row0);
  double* Af = eb + NP;                                    // Af[x][y] = A[x][y]
  double* Ab = Af + (NP > 16 ? NP * NP : 0);               // Ab[y][x] = A[x][y]
  if constexpr (NP > 16) {
    for (int i = tid; i < NP * NP; i += kGroupWaves * 64) {
      const double v = a.A[(i / NP) * 64 + (i % NP)];
      Af[i] = v;
      Ab[(i % NP) * NP + (i / NP)] = v;
    }
  }
  double* xch0 = Ab + (NP > 16 ? NP * NP : 0);
  double* xch = xch0 + wave * 64;
  double* wrow = xch0 + kGroupWaves * 64 + wave * 64;
  double* H0 = xch0 + 2 * kGroupWaves * 64;
  const int R = a.R;
  const int grp = lane / NP, y = lane % NP, gbase = grp * NP;
  double* Hl = H0 + ((size_t)(wave * G + grp) * R) * NP + y;   // this sequence's [R][NP], column y
  for (int r = 0; r < R; r++) Hl[r * NP] = 0.0;
  __syncthreads();

  const long gw = (long)blockIdx.x * kGroupWaves + wave;   // the wave's sequences: gw G .. gw G + G - 1
  if (gw * G >= a.B) return;
  const long b = gw * G + grp;
  const bool live = b < a.B;
  const long bl = live ? b : a.B - 1;
  const int T = a.T;
  double Ac[16], Ar[16];                                   // column y and row y of A (NP = 16)
  if constexpr (NP == 16) {
#pragma unroll
    for (int k = 0; k < 16; k++) {
      Ac[k] = a.A[k * 64 + y];
      Ar[k] = a.A[y * 64 + k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) Ac[k] = Ar[k] = 0.0;
  }
  const double sall = a.sall[y];

  using Step = SoftStep<NCA>;
  const int* orow = a.obs + bl * a.obs_bstride;
  const double* lrow = a.lik + bl * a.lik_bstride;
  auto fetch = [&](int t, Step& s) { soft_fetch<NP, NC, NH>(a, orow, lrow, y, t, s); };

  // forward, as chain_soft_kernel's fb form: the steps' loads run one step ahead, the stores one step behind
  Totals tot{1.0, 1.0, 0, 0u, kStreamAlive};
  const double prior = a.pi[y];
  double hd = prior;
  double* srow = a.S + bl * (long)T * NP + y;
  Step cur, nxt;
  fetch(0, cur);
  double owed = 0.0;
  for (int t = 0; t < T; t++) {
    fetch(t + 1 < T ? t + 1 : t, nxt);
    if (t > 0 && live) srow[(long)(t - 1) * NP] = owed;
    bool bad;
    long exs;
    const double e = soft_evid<NP, NC, NH, LONG>(a, tabs, eb, row0, wrow, lrow, lane, gbase, y, t, cur, bad, exs);
    hd = fwd_step<NP, true>(hd, e, sall, Ac, Af, xch, lane, gbase, y, t, tot);
    tot.ex += exs;                                         // m2 of the weights as given is 2^exs times fwd_step's
    if (bad) tot.status |= kSoftBadEvidence;
    owed = hd;
    if (t + 1 < T) cur = nxt;
  }
  const bool zero = tot.dead != kStreamAlive;
  if (zero) tot.status |= 3u;                              // ZERO_MASS | BAD_LUCK, as nipamd_estep
  if (live && y == 0) {
    if (a.ll) a.ll[b] = totals_ll(tot);
    if (a.status) a.status[b] = tot.status;
  }

  // backward: cur holds step T - 1, gamma_{T-1} = alpha^_{T-1}, beta = 1 there
  double K[NP];
#pragma unroll
  for (int x = 0; x < NP; x++) K[x] = 0.0;
  double gsum = 0.0;                                       // sum_t gamma_t[y]: the rows of the unnamed children
  double gamma = hd, beta = 1.0;
  double al = T > 1 ? srow[(long)(T - 2) * NP] : prior;    // alpha^_{t-1}
  for (int t = T - 1; t >= 0; t--) {
    if (t > 0) fetch(t - 1, nxt);
    const double aln = t > 1 ? srow[(long)(t - 2) * NP] : prior;
    const double e =
        soft_evid_counts<NP, NC, NH, LONG>(a, tabs, eb, row0, wrow, lrow, Hl, lane, gbase, y, t, cur, gamma);
    gsum += gamma;
    const double g = e * beta;
    const double v = matvec<NP>(g, Ar, Ab, xch, lane, gbase, y);
    const double av = al * v;
    const double Z = group_sum<NP>(av);
    const bool ok = Z > 0.0;
    const double c = ok ? g / Z : 0.0;
    xch[lane] = al;
    wave_lds_sync();
#pragma unroll
    for (int x = 0; x < NP; x++) K[x] = fma(xch[gbase + x], c, K[x]);
    wave_lds_sync();
    gamma = ok ? av / Z : 0.0;
    int ex = 0;
    (void)frexp(group_max<NP>(v), &ex);                    // 0 for a maximum of 0
    beta = ldexp(v, -ex);
    if (t > 0) cur = nxt;
    al = aln;
  }

  // the slab row: K [NP][NP], H [R][NP], P0 [NP] (gamma is gamma_{-1} now); all zero without mass
  if (!live) return;
  double* out = a.slab + b * (long)a.slab_size + y;
#pragma unroll
  for (int x = 0; x < NP; x++) out[x * NP] = zero ? 0.0 : K[x];
  out += NP * NP;
  for (int u = 0; u < a.n_unobs; u++) Hl[a.urow[u] * NP] = gsum;
  for (int r = 0; r < R; r++) out[r * NP] = zero ? 0.0 : Hl[r * NP];
  out[R * NP] = zero ? 0.0 : gamma;
}

bool estep_soft_shape_ok(const EstepSoftArgs& a) {
  if (!(cols_shape_ok(a) && a.T >= 1 && a.nhard >= 0 && a.nhard <= a.ncol && a.R >= 1 && a.n_unobs >= 0 &&
        a.n_unobs <= 4 && a.slab_size == group_np(a.N) * group_np(a.N) + a.R * group_np(a.N) + group_np(a.N)))
    return false;
  for (int k = 0; k < a.ncol; k++)
    if (a.hrow[k] < 0 || a.hrow[k] + a.M[k] + 2 > a.R) return false;
  for (int u = 0; u < a.n_unobs; u++)
    if (a.urow[u] < 0 || a.urow[u] >= a.R) return false;
  return true;
}

int estep_soft_dispatch(const EstepSoftArgs& a, bool launch, hipStream_t stream) {
  return soft_group_launch(
      a, launch, stream,
      [](auto np, auto nc, auto nh, auto lng) {
        return &chain_estep_soft_kernel<decltype(np)::value, decltype(nc)::value, decltype(nh)::value,
                                        decltype(lng)::value>;
      },
      chain_estep_soft_lds_bytes(a));
}

}  // namespace

size_t chain_estep_soft_lds_bytes(const EstepSoftArgs& a) {
  return (group_lds_doubles(a, a.N, 2) + estep_soft_h_doubles(a)) * sizeof(double);
}

int chain_estep_soft_prepare(const EstepSoftArgs& a) {
  if (!estep_soft_shape_ok(a)) return kLaunchRefused;
  return estep_soft_dispatch(a, false, nullptr);
}

int chain_estep_soft_launch(const EstepSoftArgs& a, hipStream_t stream) {
  if (!estep_soft_shape_ok(a) || !a.slab || !a.S || (a.nhard > 0 && !a.obs) || (a.nhard < a.ncol && !a.lik))
    return kLaunchRefused;
  g_last_kernel = "chain_estep_soft_kernel";
  return estep_soft_dispatch(a, true, stream);
}

}  // namespace nipamd
