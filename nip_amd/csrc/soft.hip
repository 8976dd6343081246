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
// out goes to the ll's exponent (soft_evid), so e_t is a product of factors of
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
// cross-lane operation stays inside the group.  The step's loads and evidence, the
// rows, the backward step and the ladder: soft_group.h, with the stream kernels.
#include <hip/hip_runtime.h>

#include "soft_group.h"

namespace nipamd {

namespace {

// NH: the hard columns, the first NH of the NC (a.nhard).  LONG: some soft
// column has more than NP states -- only then the step loop holds the loads of
// a vector's later pieces (and the waits that come with loads inside a loop).
template <int NP, int NC, int NH, bool LONG>
__global__ __launch_bounds__(kGroupWaves * 64) void chain_soft_kernel(SoftArgs a) {
  static_assert(NH >= 0 && NH <= NC, "the hard columns are the first of the columns");
  constexpr int NCA = NC > 0 ? NC : 1;
  constexpr int G = 64 / NP;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [rows][NP] tables, ebase [NP], A and A^T [NP][NP] (NP > 16), [waves][64] exchange rows,
  // [waves][64] weight rows (staging and lane geometry stay written out: soft_group.h says why)
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

  using Step = SoftStep<NCA>;
  const int* orow = a.obs + bl * a.obs_bstride;
  const double* lrow = a.lik + bl * a.lik_bstride;
  auto fetch = [&](int t, Step& s) { soft_fetch<NP, NC, NH>(a, orow, lrow, y, t, s); };
  auto evid = [&](int t, const Step& s, bool& bad, long& exs) {
    return soft_evid<NP, NC, NH, LONG>(a, tabs, eb, row0, wrow, lrow, lane, gbase, y, t, s, bad, exs);
  };
  // A row's values (row_value) and its store are two steps: the store of row r
  // is issued one loop iteration late, right after the next step's loads, so
  // that a wait for those loads never waits for a store just issued.
  const int width = a.post_tstride;
  double* prow = a.post + bl * a.post_bstride;
  auto put = [&](double v, int r) { row_put<NP>(a, prow, width, xch, live, lane, gbase, y, v, r); };

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
      owed = decltype(filter)::value ? row_value<NP>(hd, false, tot.dead != kStreamAlive) : hd;
      cur = nxt;
    }
    store(T - 1);
  };
  if (a.filter) forward(std::true_type{});
  else forward(std::false_type{});
  if (live && y == 0) {
    if (a.ll) a.ll[b] = totals_ll(tot);
    if (a.status) a.status[b] = tot.status;
  }
  if (a.filter) return;

  // backward: cur holds step T - 1; beta = 1 there
  const bool zero = tot.dead != kStreamAlive;
  owed = row_value<NP>(hd, true, zero);
  double beta = 1.0;
  double al = T > 1 ? srow[(long)(T - 2) * NP] : 0.0;
  for (int t = T - 2; t >= 0; t--) {
    fetch(t, nxt);
    const double aln = t > 0 ? srow[(long)(t - 1) * NP] : 0.0;
    put(owed, t + 1);
    bool bad;
    long exs;
    beta = bwd_step<NP>(evid(t + 1, cur, bad, exs), beta, Ar, Ab, xch, lane, gbase, y);
    owed = row_value<NP>(al * beta, true, zero);
    cur = nxt;
    al = aln;
  }
  put(owed, 0);
}

bool soft_shape_ok(const SoftArgs& a) {
  return cols_shape_ok(a) && a.T >= 1 && a.nhard >= 0 && a.nhard <= a.ncol;
}

int soft_dispatch(const SoftArgs& a, bool launch, hipStream_t stream) {
  return soft_group_launch(a, launch, stream, [](auto np, auto nc, auto nh, auto lng) {
    return &chain_soft_kernel<decltype(np)::value, decltype(nc)::value, decltype(nh)::value, decltype(lng)::value>;
  });
}

}  // namespace

size_t chain_soft_scratch_bytes(int N, long B, int T) {
  return (size_t)B * (size_t)T * group_np(N) * sizeof(double);
}

size_t chain_soft_lds_bytes(const SoftArgs& a) { return soft_lds_bytes(a); }

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
