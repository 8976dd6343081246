// soft_group.h -- what chain_stream_kernel (stream.hip), chain_soft_kernel
// (soft.hip) and chain_stream_soft_kernel (stream_soft.hip) share beyond
// chain_group.h, one definition each: a step's soft evidence, the row value
// and store, the backward step, the ll, the stream state's write-back and the
// NH x LONG launch ladder.  The kernels' staging, lane geometry and A rows stay
// written out in each: as routines they leave the compiler other LDS read
// merging and register counts.  chain_viterbi_soft_kernel (viterbi_soft.hip)
// takes the step's soft evidence and the ladder from here.  Included as
// chain_group.h is.
#pragma once
#include <cfloat>

#include "chain_group.h"
#include "store_pol.h"

namespace nipamd {
namespace {

// doubles of LDS of the tables, A / A^T and wave_rows [64] rows per wave (the exchange row included)
inline size_t group_lds_doubles(const EvidenceArgs& a, int N, int wave_rows) {
  const int NP = group_np(N);
  return evid_rows(a) * NP + (NP > 16 ? 2 * (size_t)NP * NP : 0) + (size_t)wave_rows * kGroupWaves * 64;
}

// what a step reads from memory: the hard columns' codes, and this lane's
// weight of the first NP of every soft column (past the vector's end: its first weight again, unused)
template <int NCA>
struct SoftStep {
  int code[NCA];
  double w[NCA];
};
// orow / lrow: the sequence's rows (dereferenced with NH > 0 / NH < NC only), t: the step among them
template <int NP, int NC, int NH, typename Args>
__device__ __forceinline__ void soft_fetch(const Args& a, const int* orow, const double* lrow, int y, int t,
                                           SoftStep<(NC > 0 ? NC : 1)>& s) {
#pragma unroll
  for (int k = 0; k < NC; k++) {
    s.code[k] = 0;
    s.w[k] = 0.0;
    if (k < NH) s.code[k] = orow[(long)t * a.obs_tstride + a.col[k]];
    else s.w[k] = lrow[(long)t * a.lik_tstride + a.col[k] + (y < a.M[k] ? y : 0)];
  }
}
// e_t of this lane's state from the step's loads, every soft vector taken at
// the scale of its largest weight: w 2^-ex with 2^(ex-1) <= max w < 2^ex
// (frexp / ldexp: exact), so that a column's sum is of the size of its table's
// entries whatever the caller's scale, the product over the columns neither
// overflows nor underflows on the way, and the rows are the same bits for w
// and for 2^k w.  exs: the sum of the columns' ex, which the forward pass adds
// to the ll's exponent (a backward pass normalises and needs none).  bad: a
// weight of the group's sequence is negative, NaN or infinite (then e_t = 0);
// such a weight is 0 before the maximum is taken.  wrow: the wave's weight row
// in LDS.  LONG: some soft column has more than NP states -- only then the
// loads of a vector's later pieces (and the waits that come with loads inside
// a loop).  The kernel's locals come by reference, as the lambda it replaces captured them.
template <int NP, int NC, int NH, bool LONG, typename Args>
__device__ __forceinline__ double soft_evid(const Args& a, double* const& tabs, double* const& eb,
                                            const int (&row0)[NC > 0 ? NC : 1], double* const& wrow,
                                            const double* const& lrow, const int& lane, const int& gbase,
                                            const int& y, int t, const SoftStep<(NC > 0 ? NC : 1)>& s, bool& bad,
                                            long& exs) {
  double e = eb[y];
  bool mine = false;
  exs = 0;
#pragma unroll
  for (int k = 0; k < NC; k++) {
    if (k < NH) {
      e *= tabs[(row0[k] + code_of(s.code[k], a.M[k])) * NP + y];
    } else {
      const int M = a.M[k];
      const double* tk = tabs + row0[k] * NP + y;
      // this lane's weight of the piece from c0 on, a bad one as 0 (past the
      // vector's end: its first weight again, which cannot raise the maximum)
      auto valid = [&](double w, int c0) {
        const bool wb = !(w >= 0.0 && w <= DBL_MAX);
        mine |= wb && c0 + y < M;
        return wb ? 0.0 : w;
      };
      auto later = [&](int c0) {
        return lrow[(long)t * a.lik_tstride + a.col[k] + (c0 + y < M ? c0 + y : 0)];
      };
      const double w0 = valid(s.w[k], 0);
      double mx = w0;
      if constexpr (LONG)
        for (int c0 = NP; c0 < M; c0 += NP) mx = fmax(mx, valid(later(c0), c0));
      int ex = 0;
      (void)frexp(group_max<NP>(mx), &ex);               // 0 for a maximum of 0
      exs += ex;
      double acc = 0.0;
      // the weights o = c0 .. c0 + n - 1, this lane's being w
      auto piece = [&](double w, int c0) {
        wrow[lane] = ldexp(w, -ex);
        wave_lds_sync();
        const int n = M - c0 < NP ? M - c0 : NP;
        for (int o = 0; o < n; o++) acc = fma(wrow[gbase + o], tk[(c0 + o) * NP], acc);
        wave_lds_sync();
      };
      piece(w0, 0);
      if constexpr (LONG)
        for (int c0 = NP; c0 < M; c0 += NP) piece(valid(later(c0), c0), c0);
      e *= acc;
    }
  }
  constexpr unsigned long long gmask = NP == 64 ? ~0ull : (1ull << (NP & 63)) - 1ull;
  bad = ((__ballot(mine) >> gbase) & gmask) != 0ull;
  return bad ? 0.0 : e;
}

// A row's values: normalise(p) (norm; else p as it is: alpha^ is normalised),
// all zeros for a sequence without mass at the row's endpoint
template <int NP>
__device__ __forceinline__ double row_value(double p, bool norm, bool zero) {
  double v = p;
  if (norm) {
    const double s = group_sum<NP>(p);
    v = s > 0.0 ? p / s : 0.0;
  }
  return zero ? 0.0 : v;
}
// Row r of the rows prow (width = a.post_tstride apart, read once by the kernel) from
// its values: the interface state itself, or the queried variables' digit sums
template <int NP, typename Args>
__device__ __forceinline__ void row_put(const Args& a, double* prow, int width, double* xch, bool live, int lane,
                                        int gbase, int y, double v, int r) {
  double* dst = prow + (long)r * width;
  if (a.nq == 0) {
    if (live && y < a.N) store_pol<NIPAMD_POST_NT != 0>(dst + y, v);
    return;
  }
  xch[lane] = v;
  wave_lds_sync();
  for (int c = y; c < width; c += NP) {
    int j = 0, d = c;
    while (j < a.nq - 1 && d >= a.qcard[j]) { d -= a.qcard[j]; j++; }
    const int qs = a.qstride[j], qc = a.qcard[j];
    double acc = 0.0;
    for (int x = 0; x < a.N; x++) acc += (x / qs) % qc == d ? xch[gbase + x] : 0.0;
    if (live) store_pol<NIPAMD_POST_NT != 0>(dst + c, acc);
  }
  wave_lds_sync();
}

// beta <- A (e o beta), rescaled by the exact power of two of the group maximum (finite on unreached states)
template <int NP>
__device__ __forceinline__ double bwd_step(double e, double beta, const double (&Ar)[16], const double* Ab,
                                           double* xch, int lane, int gbase, int y) {
  beta = matvec<NP>(e * beta, Ar, Ab, xch, lane, gbase, y);
  int ex = 0;
  (void)frexp(group_max<NP>(beta), &ex);                   // 0 for a maximum of 0
  return ldexp(beta, -ex);
}

// the ll of the totals: a function of the state alone
__device__ __forceinline__ double totals_ll(const Totals& tot) {
  return tot.dead != kStreamAlive ? -DBL_MAX
                                  : log(tot.num) - log(tot.den) + (double)tot.ex * 0.69314718055994530942;
}

// the state a stream's launch leaves of sequence b (a: StreamArgs), with ll and status out
template <int NP>
__device__ __forceinline__ void stream_state_store(const StreamArgs& a, long b, bool live, int y, double hd,
                                                   const Totals& tot) {
  if (live) {
    a.head[b * NP + y] = hd;
    if (y == 0) {
      a.snum[b] = tot.num;
      a.sden[b] = tot.den;
      a.sexp[b] = tot.ex;
      a.sstatus[b] = tot.status;
      a.sdead[b] = tot.dead;
      if (a.ll) a.ll[b] = totals_ll(tot);
      if (a.status) a.status[b] = tot.status;
    }
  }
}

// LDS of the two soft kernels: an exchange row and a weight row per wave
template <typename Args>
size_t soft_lds_bytes(const Args& a) { return group_lds_doubles(a, a.N, 2) * sizeof(double); }

// group_launch over NH (a.nhard) and LONG (a soft column longer than NP) besides, named by
// kernel_of(np, nc, nh, long); one per (NH, LONG): its dynamic-LDS bookkeeping is per kernel_of.
// lds: the kernel's bytes, kSoftLds for soft_lds_bytes(a)
constexpr size_t kSoftLds = ~(size_t)0;
template <typename Args, typename KernelOf>
int soft_group_launch(const Args& a, bool launch, hipStream_t stream, KernelOf kernel_of, size_t lds = kSoftLds) {
  if (lds == kSoftLds) lds = soft_lds_bytes(a);
  auto variant = [&](auto nh, auto lng) {
    return group_launch(a, lds, launch, stream, [kernel_of](auto np, auto nc) {
      constexpr int NC = decltype(nc)::value, NH = decltype(nh)::value < NC ? decltype(nh)::value : NC;
      return kernel_of(np, nc, std::integral_constant<int, NH>{},
                       std::integral_constant<bool, decltype(lng)::value && NH < NC>{});
    });
  };
  bool lng = false;
  for (int k = a.nhard; k < a.ncol; k++) lng |= a.M[k] > group_np(a.N);
  auto hard = [&](auto nh) { return lng ? variant(nh, std::true_type{}) : variant(nh, std::false_type{}); };
  switch (a.nhard) {
    case 0: return hard(std::integral_constant<int, 0>{});
    case 1: return hard(std::integral_constant<int, 1>{});
    case 2: return hard(std::integral_constant<int, 2>{});
    case 3: return hard(std::integral_constant<int, 3>{});
    default: return hard(std::integral_constant<int, 4>{});
  }
}

}  // namespace
}  // namespace nipamd
