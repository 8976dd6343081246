// viterbi_group.h -- what chain_viterbi_kernel (viterbi.hip) and
// chain_viterbi_soft_kernel (viterbi_soft.hip) share beyond chain_group.h, one
// definition each: the back-pointer words' geometry, the max-product step and
// the 64-bit lane read of the backtrack.  The kernels' bodies stay written out
// in each (viterbi.hip says why).  Included as chain_group.h is.
#pragma once
#include "chain_group.h"

namespace nipamd {
namespace {

__host__ __device__ constexpr int vit_log(int NP) { return NP == 16 ? 4 : NP == 32 ? 5 : 6; }
// words of one wave: T steps of log2(NP) planes, padded to whole 128-byte lines
__host__ __device__ inline long vit_wave_words(int NP, int T) { return ((long)T * vit_log(NP) + 15) & ~15L; }

// acc[k] = fma(value of lane K0 + k of this row, c[K0 + k], acc[k]), k = 0..7.
// One statement, so that the VALU -> DPP read hazard of v (2 wait states,
// which hipcc does not pad inside asm) is covered once by the leading s_nop.
template <int K0>
__device__ __forceinline__ void fmac_bcast8(double (&p)[16], double v, const double (&c)[16]) {
  asm("s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %8, %9 row_newbcast:%17 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %1, %8, %10 row_newbcast:%18 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %2, %8, %11 row_newbcast:%19 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %3, %8, %12 row_newbcast:%20 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %4, %8, %13 row_newbcast:%21 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %5, %8, %14 row_newbcast:%22 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %6, %8, %15 row_newbcast:%23 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %7, %8, %16 row_newbcast:%24 row_mask:0xf bank_mask:0xf"
      : "+v"(p[K0]), "+v"(p[K0 + 1]), "+v"(p[K0 + 2]), "+v"(p[K0 + 3]), "+v"(p[K0 + 4]), "+v"(p[K0 + 5]),
        "+v"(p[K0 + 6]), "+v"(p[K0 + 7])
      : "v"(v), "v"(c[K0]), "v"(c[K0 + 1]), "v"(c[K0 + 2]), "v"(c[K0 + 3]), "v"(c[K0 + 4]), "v"(c[K0 + 5]),
        "v"(c[K0 + 6]), "v"(c[K0 + 7]), "n"(K0), "n"(K0 + 1), "n"(K0 + 2), "n"(K0 + 3), "n"(K0 + 4),
        "n"(K0 + 5), "n"(K0 + 6), "n"(K0 + 7));
}

// max and lowest argmax of p[0..NP): four chains over ascending quarters,
// merged in ascending order with a strict compare, so the lowest index wins
template <int NP>
__device__ __forceinline__ void argmax_low(const double (&p)[NP], double& best, int& arg) {
  constexpr int Q = NP / 4;
  double b[4];
  int a[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    b[c] = p[c * Q];
    a[c] = c * Q;
#pragma unroll
    for (int i = 1; i < Q; i++) {
      const bool g = p[c * Q + i] > b[c];
      a[c] = g ? c * Q + i : a[c];
      b[c] = g ? p[c * Q + i] : b[c];
    }
  }
  const bool g01 = b[1] > b[0], g23 = b[3] > b[2];
  const double b01 = g01 ? b[1] : b[0], b23 = g23 ? b[3] : b[2];
  const int a01 = g01 ? a[1] : a[0], a23 = g23 ? a[3] : a[2];
  const bool g = b23 > b01;
  best = g ? b23 : b01;
  arg = g ? a23 : a01;
}

// One step for this lane's state y: m = the group's max of delta_{t-1} (d in
// lane x = delta_{t-1}[x]), best / arg = max_x and lowest argmax_x of
// delta_{t-1}[x] A[x][y].  xch: the wave's 64 doubles of LDS (NP > 16).
template <int NP>
__device__ __forceinline__ void vit_step(double d, const double (&Ac)[NP], double* xch, int lane, int gbase,
                                         double& m, double& best, int& arg) {
  double p[NP];
  if constexpr (NP == 16) {
#pragma unroll
    for (int x = 0; x < 16; x++) p[x] = 0.0;
    fmac_bcast8<0>(p, d, Ac);
    fmac_bcast8<8>(p, d, Ac);
    m = row_max(d);
  } else {
    xch[lane] = d;
    wave_lds_sync();
    m = 0.0;
#pragma unroll
    for (int x = 0; x < NP; x++) {
      const double dx = xch[gbase + x];
      m = fmax(m, dx);
      p[x] = dx * Ac[x];
    }
    wave_lds_sync();
  }
  argmax_low<NP>(p, best, arg);
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long w, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)w, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(w >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

}  // namespace
}  // namespace nipamd
