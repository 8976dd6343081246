// soft.hip -- filtering and smoothing under soft (likelihood) evidence over an
// interface chain, batched over whole sequences (nipamd_fb_soft,
// nipamd_filter_soft, engine_soft.cpp).
//
// The chain kernels take a step's evidence as a product of table rows: a hard
// observation of child k picks row o of its table E_k.  A soft observation is
// a likelihood vector w over the child's states and enters as the weighted sum
// of the state rows,
//
//   e_t[y] = ebase[y]  prod_hard E_k[o_{k,t}][y]  prod_soft sum_o w_{k,t}[o] E_k[o][y]
//
// -- all ones gives the "missing" row, a one-hot vector a hard observation, and
// scaling a step's vector by c adds log c to the ll and moves no row, for any
// finite non-negative vector with a positive entry (denormals to DBL_MAX): a
// vector is used at the scale of its largest weight and the power of two taken
// out goes to the ll's exponent (evid below), so e_t is a product of factors of
// ordinary size.  Everything else is stream.hip's recursion on a whole sequence
// (DESIGN.md 2):
//
//   forward   alpha^_t = fwd_step(alpha^_{t-1}, e_t), alpha^_{-1} = prior; the ll as
//             two mantissa products and one exponent (chain_group.h)
//   filter    row t = alpha^_t
//   fb        alpha^_t goes to scratch [B][T][NP]; then beta = 1 at T - 1,
//             beta <- A (e_{t+1} o beta) rescaled by the exact power of two of
//             the group maximum at every step (finite on states the forward
//             pass never reaches), row t = normalise(alpha^_t o beta)
//
// with rows summed into the queried variables' digits.  A weight that is
// negative, NaN or infinite leaves its step without evidence (e_t = 0): the
// sequence has no mass from that step on and gets kSoftBadEvidence besides the
// zero-mass bit.  A dead sequence has ll = -DBL_MAX; its fb rows are all zero,
// its filtered rows from the dead step on.
//
// The backward pass recomputes e_t from the weights instead of storing it next
// to alpha^_t (W doubles read again against NP written and read).
//
// Layout: chain_group.h's lane groups (NP = 16, 32 or 64 padded states, one
// NP-lane group per sequence, kGroupWaves independent waves per block), one
// block barrier after the tables are staged.  The hard columns come first
// (nhard of the NC columns, uniform over the launch) and their number is a
// template parameter: the unrolled column loop has no branch.  A step's
// weights are loaded by the group's lanes, NP at a time, one step ahead of
// their use (their first NP; a longer vector's remaining pieces on demand), put
// into the wave's own LDS row and summed by every lane in the order of o.  A
// sequence's results depend on its own inputs alone, bit for bit: every
// cross-lane operation stays inside the group.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "chain_group.h"
#include "store_pol.h"

namespace nipamd {

namespace {

// NH: the hard columns, the first NH of the NC (a.nhard).  LONG: some soft
// column has more than NP states -- only then the step loop holds the loads of
// a vector's later pieces (and the waits that come with loads inside a loop).
template <int NP, int NC, int NH, bool LONG>
__global__ __launch_bounds__(kGroupWaves * 64) void chain_soft_kernel(SoftArgs a) {
  static_assert(NH >= 0 && NH <= NC, "the hard columns are the first of the columns");
  constexpr int G = 64 / NP;
  constexpr int NCA = NC > 0 ? NC : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [rows][NP] tables, ebase [NP], A and A^T [NP][NP] (NP > 16), [waves][64] exchange rows,
  // [waves][64] weight rows
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
  __syncthreads();

  const int grp = lane / NP, y = lane % NP, gbase = grp * NP;
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

  // what a step reads from memory: the hard columns' codes, and this lane's
  // weight of the first NP of every soft column (past the vector's end: its first weight again, unused)
  struct Step {
    int code[NCA];
    double w[NCA];
  };
  const int* orow = a.obs + bl * a.obs_bstride;            // dereferenced with NH > 0 only
  const double* lrow = a.lik + bl * a.lik_bstride;         // dereferenced with NH < NC only
  auto fetch = [&](int t, Step& s) {
#pragma unroll
    for (int k = 0; k < NC; k++) {
      s.code[k] = 0;
      s.w[k] = 0.0;
      if (k < NH) s.code[k] = orow[(long)t * a.obs_tstride + a.col[k]];
      else s.w[k] = lrow[(long)t * a.lik_tstride + a.col[k] + (y < a.M[k] ? y : 0)];
    }
  };
  // e_t of this lane's state from the step's loads, every soft vector taken at
  // the scale of its largest weight: w 2^-ex with 2^(ex-1) <= max w < 2^ex
  // (frexp / ldexp: exact), so that a column's sum is of the size of its table's
  // entries whatever the caller's scale, the product over the columns neither
  // overflows nor underflows on the way, and the rows are the same bits for w
  // and for 2^k w.  exs: the sum of the columns' ex, which the forward pass adds
  // to the ll's exponent (the backward pass normalises and needs none).  bad: a
  // weight of the group's sequence is negative, NaN or infinite (then e_t = 0);
  // such a weight is 0 before the maximum is taken.
  auto evid = [&](int t, const Step& s, bool& bad, long& exs) {
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
  };

  const int width = a.post_tstride;
  double* prow = a.post + bl * a.post_bstride;
  // A row's values and its store are two steps: the store of row r is issued
  // one loop iteration late, right after the next step's loads, so that a wait
  // for those loads never waits for a store just issued.
  // value: normalise(p) (norm; else p as it is: alpha^ is normalised), all
  // zeros for a sequence without mass
  auto value = [&](double p, bool norm, bool zero) {
    double v = p;
    if (norm) {
      const double s = group_sum<NP>(p);
      v = s > 0.0 ? p / s : 0.0;
    }
    return zero ? 0.0 : v;
  };
  // row r from its values: the interface state itself, or the queried
  // variables' digit sums (as chain_stream_kernel's rows)
  auto put = [&](double v, int r) {
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
  };

  // forward: the steps' loads run one step ahead, the stores one step behind
  Totals tot{1.0, 1.0, 0, 0u, kStreamAlive};
  double hd = a.pi[y];
  double* srow = a.filter ? nullptr : a.S + bl * (long)T * NP + y;
  Step cur, nxt;
  fetch(0, cur);
  double owed = 0.0;                                       // the values of the row (scratch row) not yet stored
  auto forward = [&](auto filter) {
    auto store = [&](int t) {
      if constexpr (decltype(filter)::value) put(owed, t);
      else if (live) srow[(long)t * NP] = owed;
    };
    for (int t = 0; t < T; t++) {
      fetch(t + 1 < T ? t + 1 : t, nxt);
      if (t > 0) store(t - 1);
      bool bad;
      long exs;
      const double e = evid(t, cur, bad, exs);
      hd = fwd_step<NP, true>(hd, e, sall, Ac, Af, xch, lane, gbase, y, t, tot);
      tot.ex += exs;                                       // m2 of the weights as given is 2^exs times fwd_step's
      if (bad) tot.status |= kSoftBadEvidence;
      owed = decltype(filter)::value ? value(hd, false, tot.dead != kStreamAlive) : hd;
      cur = nxt;
    }
    store(T - 1);
  };
  if (a.filter) forward(std::true_type{});
  else forward(std::false_type{});
  if (live && y == 0) {
    if (a.ll)
      a.ll[b] = tot.dead != kStreamAlive ? -DBL_MAX
                                         : log(tot.num) - log(tot.den) + (double)tot.ex * 0.69314718055994530942;
    if (a.status) a.status[b] = tot.status;
  }
  if (a.filter) return;

  // backward: cur holds step T - 1; beta = 1 there
  const bool zero = tot.dead != kStreamAlive;
  owed = value(hd, true, zero);
  double beta = 1.0;
  double al = T > 1 ? srow[(long)(T - 2) * NP] : 0.0;
  for (int t = T - 2; t >= 0; t--) {
    fetch(t, nxt);
    const double aln = t > 0 ? srow[(long)(t - 1) * NP] : 0.0;
    put(owed, t + 1);
    bool bad;
    long exs;
    const double e = evid(t + 1, cur, bad, exs);
    beta = matvec<NP>(e * beta, Ar, Ab, xch, lane, gbase, y);
    int ex = 0;
    (void)frexp(group_max<NP>(beta), &ex);                 // 0 for a maximum of 0
    beta = ldexp(beta, -ex);
    owed = value(al * beta, true, zero);
    cur = nxt;
    al = aln;
  }
  put(owed, 0);
}

bool soft_shape_ok(const SoftArgs& a) {
  return cols_shape_ok(a) && a.T >= 1 && a.nhard >= 0 && a.nhard <= a.ncol;
}

int soft_dispatch(const SoftArgs& a, bool launch, hipStream_t stream) {
  // one group_launch per (NH, LONG): its dynamic-LDS bookkeeping is per kernel_of
  auto variant = [&](auto nh, auto lng) {
    return group_launch(a, chain_soft_lds_bytes(a), launch, stream, [](auto np, auto nc) {
      constexpr int NC = decltype(nc)::value, NH = decltype(nh)::value < NC ? decltype(nh)::value : NC;
      return &chain_soft_kernel<decltype(np)::value, NC, NH, decltype(lng)::value && NH < NC>;
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

size_t chain_soft_scratch_bytes(int N, long B, int T) {
  return (size_t)B * (size_t)T * group_np(N) * sizeof(double);
}

size_t chain_soft_lds_bytes(const SoftArgs& a) {
  const int NP = group_np(a.N);
  const size_t dbl = evid_rows(a) * NP + (NP > 16 ? 2 * (size_t)NP * NP : 0) + 2 * kGroupWaves * 64;
  return dbl * sizeof(double);
}

int chain_soft_prepare(const SoftArgs& a) {
  if (!soft_shape_ok(a)) return kLaunchRefused;
  return soft_dispatch(a, false, nullptr);
}

int chain_soft_launch(const SoftArgs& a, hipStream_t stream) {
  if (!soft_shape_ok(a) || !a.post || (!a.filter && !a.S) || (a.nhard > 0 && !a.obs) ||
      (a.nhard < a.ncol && !a.lik))
    return kLaunchRefused;
  g_last_kernel = "chain_soft_kernel";
  return soft_dispatch(a, true, stream);
}

}  // namespace nipamd
