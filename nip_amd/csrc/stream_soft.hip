// stream_soft.hip -- online inference under soft (likelihood) evidence:
// resumable filtering and fixed-lag smoothing of sequences whose step evidence
// holds likelihood vectors (nipamd_stream_open_soft / nipamd_stream_push_soft,
// engine_stream.cpp).
//
// Rows, the emission schedule and the ll are stream.hip's, the step evidence
// e_t is soft.hip's:
//
//   e_t[y] = ebase[y]  prod_hard E_k[o_{k,t}][y]  prod_soft sum_o w_{k,t}[o] E_k[o][y]
//
// with every soft vector taken at the scale of its largest weight and the power
// of two taken out added to the ll's exponent by the head.  What differs from
// chain_stream_kernel is what a pending step keeps.  A likelihood vector has no
// code, and a window of vectors does not fit LDS, so the state holds the
// evaluated evidence itself: a ring of e_t[y], NP doubles per step, step t in
// slot t % R with R = lag + kStreamChunk.  One launch
//
//   head   evaluates e_t of every new step once, stores it to its slot and
//          takes the head's forward step with it (the totals, the exponents,
//          the bad-weight bit)
//   row t  base <- one forward step with e_t from the ring; beta = 1 at the
//          row's endpoint, beta <- A (e_j o beta) with e_j from the ring
//
// so a row costs L + 2 mat-vecs and one evidence evaluation, where
// chain_soft_kernel (each e_t used twice) recomputes it.  The window -- the
// pending steps, then the new ones -- is W <= R consecutive steps, so its slots
// are distinct and nothing is copied when the launch ends.  Lane y reads only
// what lane y wrote (in this launch or an earlier one): no fence inside a
// launch.  The backward pass normalises, so no exponent is kept with e_t; a
// step that is bad or leaves the sequence without mass is stored as zeros.
// Lag 0 has no ring: the row of a step is the head itself.
//
// Consequence: a pending step keeps the evidence of the model's tables as they
// were at the push that consumed it; chain_stream_kernel keeps raw codes and
// reads them against the tables of every later push.
//
// Every step of every sequence runs through the same routines with the same
// operands, whatever the split into launches and the place in the batch: rows,
// ll and status are bit-identical across splits.
//
// Layout: chain_group.h's lane groups, as soft.hip -- tables, A / A^T above 16
// states, the waves' exchange and weight rows in LDS (no code window), one
// block barrier after the staging, template parameters NP x NC x NH x LONG.
// The new steps' codes and weights are loaded one step ahead of their use, the
// base's e_t too, and the ring's e_j of the backward recursion in blocks of
// four, a block ahead: their addresses do not depend on the recursion, and a
// backward step is too short to cover a load from L2 by itself.  The step's
// loads and evidence are soft.hip's and the rows, the backward step and the
// state's write-back stream.hip's: one definition each, in soft_group.h.
#include <hip/hip_runtime.h>

#include "soft_group.h"

namespace nipamd {

namespace {

// NH: the hard columns, the first NH of the NC (a.nhard).  LONG: some soft
// column has more than NP states (the loads of a vector's later pieces).
template <int NP, int NC, int NH, bool LONG>
__global__ __launch_bounds__(kGroupWaves * 64) void chain_stream_soft_kernel(StreamSoftArgs a) {
  static_assert(NH >= 0 && NH <= NC, "the hard columns are the first of the columns");
  constexpr int NCA = NC > 0 ? NC : 1;
  constexpr int G = 64 / NP;
  constexpr int kAhead = 4;                                // the backward pass's e_j are loaded in blocks of four
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

  const int L = a.lag, P = a.pending, Tn = a.T_new, W = P + Tn;
  const int R = L + kStreamChunk;                          // the ring's slots (L > 0)
  const long s0 = a.n - P;                                 // the step of window index 0
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

  using Step = SoftStep<NCA>;                              // of new step t, t among the launch's
  const int* orow = a.obs + bl * a.obs_bstride;
  const double* lrow = a.lik + bl * a.lik_bstride;
  auto fetch = [&](int t, Step& s) { soft_fetch<NP, NC, NH>(a, orow, lrow, y, t, s); };
  auto evid = [&](int t, const Step& s, bool& bad, long& exs) {
    return soft_evid<NP, NC, NH, LONG>(a, tabs, eb, row0, wrow, lrow, lane, gbase, y, t, s, bad, exs);
  };

  Totals tot{a.snum[bl], a.sden[bl], a.sexp[bl], a.sstatus[bl], a.sdead[bl]};
  Totals none{};                                           // the base's steps carry no totals
  double hd = a.head[bl * NP + y];
  const int width = a.post_tstride;
  double* prow = a.post ? a.post + bl * a.post_bstride : nullptr;
  auto emit = [&](double p, bool norm, bool zero, int r) {
    row_put<NP>(a, prow, width, xch, live, lane, gbase, y, row_value<NP>(p, norm, zero), r);
  };

  // this lane's e of window index w (step s0 + w) in the ring
  double* ring = a.ering + bl * (long)R * NP + y;          // dereferenced with L > 0 only
  const int slot0 = (int)(s0 % R);
  auto slot = [&](int w) {                                 // w < W <= R
    const int s = slot0 + w;
    return (long)(s >= R ? s - R : s) * NP;
  };

  // the head: one evaluation of e_t and one forward step per new step, the
  // step's loads one step ahead.  Lag 0: the row of step t is alpha^_t itself.
  Step cur, nxt;
  if (Tn > 0) fetch(0, cur);
  for (int i = 0; i < Tn; i++) {
    fetch(i + 1 < Tn ? i + 1 : i, nxt);
    bool bad;
    long exs;
    const double e = evid(i, cur, bad, exs);
    hd = fwd_step<NP, true>(hd, e, sall, Ac, Af, xch, lane, gbase, y, a.n + i, tot);
    tot.ex += exs;                                         // m2 of the weights as given is 2^exs times fwd_step's
    if (bad) tot.status |= kSoftBadEvidence;
    if (L == 0) emit(hd, false, tot.dead != kStreamAlive, i);
    else if (live) ring[slot(P + i)] = tot.dead != kStreamAlive ? 0.0 : e;
    cur = nxt;
  }

  if (L > 0) {
    double bs = a.base[bl * NP + y];
    double enext = a.E > 0 ? ring[slot(0)] : 0.0;          // e of the base's next step
    for (int r = 0; r < a.E; r++) {                        // row t = s0 + r
      const int endw = a.final ? W - 1 : r + L;            // the row's endpoint min(t + L, n_end - 1)
      const double er = enext;
      enext = ring[slot(r + 1 < W ? r + 1 : r)];
      // the backward steps' e_j in blocks of kAhead, a block ahead of their use (an index
      // below r: r, in the window, unused)
      auto back = [&](int j) { return ring[slot(j > r ? j : r)]; };
      double e0 = back(endw), e1 = back(endw - 1), e2 = back(endw - 2), e3 = back(endw - 3);
      bs = fwd_step<NP, false>(bs, er, sall, Ac, Af, xch, lane, gbase, y, s0 + r, none);
      double beta = 1.0;
      auto bwd = [&](double e) { beta = bwd_step<NP>(e, beta, Ar, Ab, xch, lane, gbase, y); };
      int j = endw;
      for (; j - r >= kAhead; j -= kAhead) {
        const double c0 = e0, c1 = e1, c2 = e2, c3 = e3;
        e0 = back(j - 4); e1 = back(j - 5); e2 = back(j - 6); e3 = back(j - 7);
        // the loop has no store: without this the compiler carries the indices and loads
        // each e_j where it is used, the load's whole latency in every step
        asm volatile("" ::: "memory");
        bwd(c0); bwd(c1); bwd(c2); bwd(c3);
      }
      if (j > r) bwd(e0);
      if (j - 1 > r) bwd(e1);
      if (j - 2 > r) bwd(e2);
      emit(bs * beta, true, s0 + endw >= tot.dead, r);
    }
    if (live) a.base[b * NP + y] = bs;
  }

  stream_state_store<NP>(a, b, live, y, hd, tot);                   // (the new steps' e_t are in the ring already)
}

bool sstr_shape_ok(const StreamSoftArgs& a) {
  return cols_shape_ok(a) && a.lag >= 0 && a.lag <= kStreamMaxLag && a.nhard >= 0 && a.nhard <= a.ncol;
}

int sstr_dispatch(const StreamSoftArgs& a, bool launch, hipStream_t stream) {
  return soft_group_launch(a, launch, stream, [](auto np, auto nc, auto nh, auto lng) {
    return &chain_stream_soft_kernel<decltype(np)::value, decltype(nc)::value, decltype(nh)::value,
                                     decltype(lng)::value>;
  });
}

}  // namespace

size_t chain_stream_soft_lds_bytes(const StreamSoftArgs& a) { return soft_lds_bytes(a); }

int chain_stream_soft_prepare(const StreamSoftArgs& a) {
  if (!sstr_shape_ok(a)) return kLaunchRefused;
  return sstr_dispatch(a, false, nullptr);
}

int chain_stream_soft_launch(const StreamSoftArgs& a, hipStream_t stream) {
  if (!sstr_shape_ok(a) || a.T_new < 0 || a.T_new > kStreamChunk || a.pending < 0 || a.pending > a.lag ||
      a.E < 0 || a.E > a.pending + a.T_new || (a.E > 0 && !a.post) || (a.lag > 0 && !a.ering) ||
      (a.T_new > 0 && ((a.nhard > 0 && !a.obs) || (a.nhard < a.ncol && !a.lik))))
    return kLaunchRefused;
  g_last_kernel = "chain_stream_soft_kernel";
  return sstr_dispatch(a, true, stream);
}

}  // namespace nipamd
