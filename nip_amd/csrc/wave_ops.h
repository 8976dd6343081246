// wave_ops.h -- what crosses the 16-lane rows of a wave, one definition each:
// the permlane-swap pair sums, the sums over 16, 32 or 64 lanes built on
// dpp_row.h's row_sum, the 16-state blocks of a sequence, the integer
// max-exponent rescale, the reciprocal of a normaliser and the LDS barrier.
// What stays inside a row is in dpp_row.h, the matrix-core register layout in
// mfma_layout.h.  (chain_group.h's group_sum / group_max go through
// __shfl_xor: the same bits, other code; viterbi.hip and stream.hip keep
// them.)  Included once per translation unit (namespace nipamd, anonymous).
#pragma once
#include <hip/hip_runtime.h>

#include "dpp_row.h"

namespace nipamd {
namespace {

// x[l] + x[l ^ 16] (xor16_sum) / x[l] + x[l ^ 32] (xor32_sum) in every lane:
// the pair's sum, identical bits in both lanes (IEEE addition commutes).  The
// swap's second operand is a copy of x made as a whole double (one v_mov_b64
// instead of two v_mov_b32); the swap works in place, so its two results come
// back in the register pairs of the two operands.
__device__ __forceinline__ double xor16_sum(double x) {
  double xc = x;
  asm("" : "+v"(xc));
  const auto rl = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(xc), false, false);
  const auto rh = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(xc), false, false);
  return __hiloint2double((int)rh[0], (int)rl[0]) + __hiloint2double((int)rh[1], (int)rl[1]);
}
__device__ __forceinline__ double xor32_sum(double x) {
  double xc = x;
  asm("" : "+v"(xc));
  const auto rl = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(xc), false, false);
  const auto rh = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(xc), false, false);
  return __hiloint2double((int)rh[0], (int)rl[0]) + __hiloint2double((int)rh[1], (int)rl[1]);
}

// Fixed-order sum over aligned groups of L lanes (16, 32 or 64; 64 is the
// whole wave): row_sum, then one pair sum per doubling.  Every level pairs
// equal partial sums, so all L lanes end with the same bits.  row_sum keeps
// the first add from being contracted into an fma (see there).
template <int L>
__device__ __forceinline__ double lanes_sum(double x) {
  static_assert(L == 16 || L == 32 || L == 64, "lanes_sum");
  x = row_sum(x);
  if (L >= 32) x = xor16_sum(x);
  if (L >= 64) x = xor32_sum(x);
  return x;
}

// lanes_sum<64> of n independent values, stage by stage so that their
// dependency chains interleave.  Unlike lanes_sum this has no contraction
// guard (the asm("" : "+v"(x)) of row_sum), on purpose: the partners of
// chain_wide4.hip pass fresh products, the compiler contracts each lane's
// term of the first add into an fma, and with the guard their kernels compile
// to other code (48 v_fmac_f64 become v_add_f64, 32 more v_mov_b64 per
// kernel).  So the lanes of one sum may disagree in the last bit here.  That
// is harmless for those callers and only for such: no scale exponent shared
// between lanes is taken from these sums -- every lane normalises its own
// posterior entry by its own sum, and the ll is one lane's own product of
// mantissas and exponents.  A caller that takes a common exponent from the
// sum needs lanes_sum.
template <int n>
__device__ __forceinline__ void wave_sum_n(double (&x)[n]) {
#pragma unroll
  for (int i = 0; i < n; i++) x[i] += row_ror<8>(x[i]);
#pragma unroll
  for (int i = 0; i < n; i++) x[i] += row_ror<4>(x[i]);
#pragma unroll
  for (int i = 0; i < n; i++) x[i] += row_ror<2>(x[i]);
#pragma unroll
  for (int i = 0; i < n; i++) x[i] += row_ror<1>(x[i]);
#pragma unroll
  for (int i = 0; i < n; i++) x[i] = xor16_sum(x[i]);
#pragma unroll
  for (int i = 0; i < n; i++) x[i] = xor32_sum(x[i]);
}

// The NB = NP / 16 blocks of 16 states of this lane's sequence (lane y holds
// x(y)), each in every lane of the sequence's rows and in canonical order:
// xb[b](lane 16 r + j) = x(state 16 b + j).  One row per sequence (NB 1): x
// itself; two rows (NB 2): one v_permlane16_swap per half ([0]: the pair's
// even row, [1]: its odd row); four rows (NB 4): a v_permlane32_swap level on
// both results (blocks 0, 2 from the first value's swap, 1, 3 from the
// second's).  The copies the in-place swaps need are made as whole doubles
// (one v_mov_b64 each instead of two v_mov_b32, as in xor16_sum).
template <int NB>
__device__ __forceinline__ void seq_blocks(double x, double (&xb)[NB]) {
  static_assert(NB == 1 || NB == 2 || NB == 4, "seq_blocks");
  if constexpr (NB == 1) {
    xb[0] = x;
  } else {
    double xc = x;
    asm("" : "+v"(xc));
    const auto pl = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(xc), false, false);
    const auto ph = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(xc), false, false);
    if constexpr (NB == 2) {
      xb[0] = __hiloint2double((int)ph[0], (int)pl[0]);
      xb[1] = __hiloint2double((int)ph[1], (int)pl[1]);
    } else {
      double p0 = __hiloint2double((int)ph[0], (int)pl[0]), p1 = __hiloint2double((int)ph[1], (int)pl[1]);
      double p0c = p0, p1c = p1;
      asm("" : "+v"(p0c));
      asm("" : "+v"(p1c));
      const auto q0l = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(p0), (unsigned)__double2loint(p0c), false, false);   // blocks 0, 2
      const auto q0h = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(p0), (unsigned)__double2hiint(p0c), false, false);
      const auto q1l = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(p1), (unsigned)__double2loint(p1c), false, false);   // blocks 1, 3
      const auto q1h = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(p1), (unsigned)__double2hiint(p1c), false, false);
      xb[0] = __hiloint2double((int)q0h[0], (int)q0l[0]);
      xb[2] = __hiloint2double((int)q0h[1], (int)q0l[1]);
      xb[1] = __hiloint2double((int)q1h[0], (int)q1l[0]);
      xb[3] = __hiloint2double((int)q1h[1], (int)q1l[1]);
    }
  }
}

// The rescale exponent from the largest element instead of the sum: minus the
// largest binary exponent over the sequence's NP lanes (16, 32 or 64).  Any
// power of two serves (the stored vectors and the partners' sums carry it
// exactly, posteriors and ll are scale-free), and an integer max over the
// wave is 32-bit DPP / permlane work (about 16 instructions) where the f64
// wave sum was 43.  Zeros do not count; an all-zero vector keeps the scale
// (-> 0).
template <int NP>
__device__ __forceinline__ int max_exp_rescale(double p) {
  static_assert(NP == 16 || NP == 32 || NP == 64, "max_exp_rescale");
  int e = row_max_exp(p);
  if (NP >= 32) {
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)e, (unsigned)e, false, false);
    e = max((int)r[0], (int)r[1]);
  }
  if (NP >= 64) {
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)e, (unsigned)e, false, false);
    e = max((int)r[0], (int)r[1]);
  }
  return rescale_of_max_exp(e);
}

// 1/c (v_rcp_f64 + two Newton steps); 0 when c == 0 so that an all-zero
// array stays zero (nip_normalise_array, nippotential.c:354)
__device__ __forceinline__ double recip(double c) {
  double r = __builtin_amdgcn_rcp(c);
  r = __builtin_fma(r, __builtin_fma(-c, r, 1.0), r);
  r = __builtin_fma(r, __builtin_fma(-c, r, 1.0), r);
  return c != 0.0 ? r : 0.0;
}

// recip of n values, staged like mirror_sum_n so the n chains interleave
template <int n>
__device__ __forceinline__ void recip_n(const double (&c)[n], double (&r)[n]) {
#pragma unroll
  for (int i = 0; i < n; i++) r[i] = __builtin_amdgcn_rcp(c[i]);
#pragma unroll
  for (int i = 0; i < n; i++) r[i] = __builtin_fma(r[i], __builtin_fma(-c[i], r[i], 1.0), r[i]);
#pragma unroll
  for (int i = 0; i < n; i++) r[i] = __builtin_fma(r[i], __builtin_fma(-c[i], r[i], 1.0), r[i]);
#pragma unroll
  for (int i = 0; i < n; i++) r[i] = c[i] != 0.0 ? r[i] : 0.0;   // all-zero rows stay zero
}

// The block barrier that hands LDS data from one wave to another: this
// wave's LDS operations complete, then s_barrier.  (Global memory is not
// waited for: estep_mw.hip's barrier_phase and the phase barrier of
// chain_mfma_core.h add vmcnt(0).)
__device__ __forceinline__ void barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace
}  // namespace nipamd
