// stream.hip -- online inference over an interface chain: resumable filtering
// and fixed-lag smoothing, batched over sequences that advance in lockstep
// (nipamd_stream_*, engine_stream.cpp).
//
// The chain plan's forward recursion enters the start of a
// sequence only through alpha_{-1} = prior, so a forward message kept on the
// device between calls resumes it at any step.  Per sequence the state holds
//
//   head  = alpha^_{n-1}   n = the steps consumed so far
//   base  = alpha^_{s-1}   s = n - pending, the oldest step whose row is still owed
//   the ll's two running products (below), status, the first step without mass,
//   and the raw codes of steps s .. n-1
//
// and one launch consumes T_new <= kStreamChunk new steps.  With lag L, row t
// is the marginal of the interface at step t given y_0 .. y_{t+L} (a flush:
// .. y_{n-1}); it is emitted by the launch that consumes step t + L:
//
//   one step      u = A^T alpha^,  m1 = sum u s_all,  a = u o e_t,  m2 = sum a,
//                 alpha^ = a / m2,  ll += log m2 - log m1      (m2 = 0: dead from t on)
//                 -- the ll as chain_wide_kernel carries it: the products of the m2 and of
//                 the m1 as a mantissa in [0.5, 1) each and one exponent sum, multiplied
//                 up step by step in the state (two multiplies and two frexp per step
//                 instead of two logarithms); the ll written out,
//                 log num - log den + ex ln 2, is a function of the state alone
//   head          one step per new step
//   row t         base <- one step (alpha^_t again, the same routine: the same bits);
//                 beta = 1 at the row's endpoint, beta <- A (e_j o beta) for j = endpoint .. t+1,
//                 rescaled by an exact power of two every step;
//                 row = normalise(alpha^_t o beta), summed into the queried variables' digits
//
// so a row costs L + 2 mat-vecs (one forward step of the head, one of the base,
// L backward).  Every step of every sequence runs through the same routine and
// the ll is summed step by step in the state, so rows, ll and status do not
// depend on how the steps were split into launches or the batch into streams:
// they are bit-identical.
//
// Layout: chain_group.h's lane groups (NP = 16, 32 or 64 padded states, one
// NP-lane group per sequence), one block barrier after the tables are staged.
// At NP = 16 column y and row y of A stay in registers and both mat-vecs are
// dpp_row.h's dot_bcast; above that the operand goes through the wave's own
// LDS row and A / A^T sit in LDS.  The evidence tables and the window's codes
// (the pending ring, then the new steps), as table rows, are staged in LDS.
// Every cross-lane sum starts from a materialised value (row_sum).  Rows, the
// backward step and the state's write-back: soft_group.h, with the soft kernels.
#include <hip/hip_runtime.h>

#include "soft_group.h"

namespace nipamd {

namespace {

template <int NP, int NC>
__global__ __launch_bounds__(kGroupWaves * 64) void chain_stream_kernel(StreamArgs a) {
  constexpr int G = 64 / NP;
  constexpr int NCA = NC > 0 ? NC : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [rows][NP] tables, ebase [NP], A and A^T [NP][NP] (NP > 16), [waves][64] exchange rows,
  // then the waves' codes [G][lag + kStreamChunk][NC] (int); written out: soft_group.h says why
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
  const int Wmax = a.lag + kStreamChunk;
  int* codes = reinterpret_cast<int*>(xch0 + kGroupWaves * 64) + wave * (G * Wmax * NC);
  __syncthreads();

  const int grp = lane / NP, y = lane % NP, gbase = grp * NP;
  const long gw = (long)blockIdx.x * kGroupWaves + wave;   // the wave's sequences: gw G .. gw G + G - 1
  if (gw * G >= a.B) return;
  const long b = gw * G + grp;
  const bool live = b < a.B;
  const long bl = live ? b : a.B - 1;

  const int L = a.lag, P = a.pending, Tn = a.T_new, W = P + Tn;
  const long s0 = a.n - P;                                 // the step of window index 0

  // the window's codes as table rows: the ring's pending steps, then the new ones
  if constexpr (NC > 0) {
    for (int i = lane; i < G * W * NC; i += 64) {
      const int k = i % NC, w = (i / NC) % W, g = i / (NC * W);
      long bb = gw * G + g;
      bb = bb < a.B ? bb : a.B - 1;
      int M = 0, r0 = 0, col = 0;
#pragma unroll
      for (int kk = 0; kk < NC; kk++)
        if (k == kk) { M = a.M[kk]; r0 = row0[kk]; col = a.col[kk]; }
      int raw;
      if (w < P) raw = a.ring[(bb * L + (s0 + w) % L) * NC + k];
      else raw = a.obs[bb * a.obs_bstride + (long)(w - P) * a.obs_tstride + col];
      codes[i] = r0 + code_of(raw, M);
    }
    wave_lds_sync();
  }
  auto evid = [&](int w) {
    double e = eb[y];
#pragma unroll
    for (int k = 0; k < NC; k++) e *= tabs[codes[(grp * W + w) * NC + k] * NP + y];
    return e;
  };

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

  Totals tot{a.snum[bl], a.sden[bl], a.sexp[bl], a.sstatus[bl], a.sdead[bl]};
  Totals none{};                                           // the base's steps carry no totals
  double hd = a.head[bl * NP + y];
  const int width = a.post_tstride;
  double* prow = a.post ? a.post + bl * a.post_bstride : nullptr;
  auto emit = [&](double p, bool norm, bool zero, int r) {
    row_put<NP>(a, prow, width, xch, live, lane, gbase, y, row_value<NP>(p, norm, zero), r);
  };
  if (L == 0) {
    // filtering: the row of step t is alpha^_t itself
    for (int w = 0; w < Tn; w++) {
      hd = fwd_step<NP, true>(hd, evid(w), sall, Ac, Af, xch, lane, gbase, y, s0 + w, tot);
      emit(hd, false, tot.dead != kStreamAlive, w);
    }
  } else {
    for (int w = P; w < W; w++)
      hd = fwd_step<NP, true>(hd, evid(w), sall, Ac, Af, xch, lane, gbase, y, s0 + w, tot);
    double bs = a.base[bl * NP + y];
    for (int r = 0; r < a.E; r++) {                        // row t = s0 + r
      bs = fwd_step<NP, false>(bs, evid(r), sall, Ac, Af, xch, lane, gbase, y, s0 + r, none);
      const int endw = a.final ? W - 1 : r + L;            // the row's endpoint min(t + L, n_end - 1)
      double beta = 1.0;
      for (int j = endw; j > r; j--) beta = bwd_step<NP>(evid(j), beta, Ar, Ab, xch, lane, gbase, y);
      emit(bs * beta, true, s0 + endw >= tot.dead, r);
    }
    if (live) a.base[b * NP + y] = bs;
  }

  // the state, and the new steps that stay pending into the ring
  stream_state_store<NP>(a, b, live, y, hd, tot);
  if constexpr (NC > 0) {
    const long nend = a.n + Tn;
    const long keep = nend < L ? nend : L;                 // pending after this launch
    const long t0 = a.n > nend - keep ? a.n : nend - keep; // the first new step that stays
    const int cnt = (int)(nend - t0);
    for (int i = lane; i < G * cnt * NC; i += 64) {
      const int k = i % NC, q = (i / NC) % cnt, g = i / (NC * cnt);
      const long bb = gw * G + g;
      if (bb >= a.B) continue;
      int col = 0;
#pragma unroll
      for (int kk = 0; kk < NC; kk++)
        if (k == kk) col = a.col[kk];
      const long t = t0 + q;
      a.ring[(bb * L + t % L) * NC + k] = a.obs[bb * a.obs_bstride + (t - a.n) * a.obs_tstride + col];
    }
  }
}

__global__ void chain_stream_init_kernel(StreamArgs a, const double* pi64, int NP) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.B * NP) {
    const double v = pi64[i % NP];
    a.base[i] = v;
    a.head[i] = v;
  }
  if (i < a.B) {
    a.snum[i] = 1.0;
    a.sden[i] = 1.0;
    a.sexp[i] = 0;
    a.sstatus[i] = 0u;
    a.sdead[i] = kStreamAlive;
  }
}

bool str_shape_ok(const StreamArgs& a) { return cols_shape_ok(a) && a.lag >= 0 && a.lag <= kStreamMaxLag; }

int str_dispatch(const StreamArgs& a, bool launch, hipStream_t stream) {
  return group_launch(a, chain_stream_lds_bytes(a), launch, stream, [](auto np, auto nc) {
    return &chain_stream_kernel<decltype(np)::value, decltype(nc)::value>;
  });
}

}  // namespace

int chain_stream_np(int N) { return group_np(N); }

size_t chain_stream_lds_bytes(const StreamArgs& a) {
  const size_t ints = (size_t)kGroupWaves * (64 / group_np(a.N)) * (a.lag + kStreamChunk) * a.ncol;
  return group_lds_doubles(a, a.N, 1) * sizeof(double) + ints * sizeof(int);
}

int chain_stream_prepare(const StreamArgs& a) {
  if (!str_shape_ok(a)) return kLaunchRefused;
  return str_dispatch(a, false, nullptr);
}

int chain_stream_launch(const StreamArgs& a, hipStream_t stream) {
  if (!str_shape_ok(a) || a.T_new < 0 || a.T_new > kStreamChunk || a.pending < 0 || a.pending > a.lag ||
      a.E < 0 || a.E > a.pending + a.T_new || (a.E > 0 && !a.post))
    return kLaunchRefused;
  g_last_kernel = "chain_stream_kernel";
  return str_dispatch(a, true, stream);
}

int chain_stream_init_launch(const StreamArgs& a, const double* pi64, hipStream_t stream) {
  const int NP = group_np(a.N);
  const long n = a.B * NP;
  hipLaunchKernelGGL(chain_stream_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, pi64, NP);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace nipamd
