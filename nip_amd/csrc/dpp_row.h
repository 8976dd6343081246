// dpp_row.h -- what lives inside one 16-lane DPP row, one definition each:
// row rotations and DPP moves of a double, the two 16-lane sum trees, the row
// maximum, the broadcast multiply-adds (v_fmac_f64_dpp row_newbcast) and the
// dots built from them, and the row's integer max-exponent rescale.  One row
// holds 16 states, lane y state y.  What crosses rows is in wave_ops.h, the
// matrix-core register layout in mfma_layout.h.  Included once per
// translation unit (namespace nipamd, anonymous).
#pragma once
#include <hip/hip_runtime.h>

namespace nipamd {
namespace {

// DPP row_ror:K -- every lane of a 16-lane row has a source, so no "old"
// operand is needed (mov_dpp with bound_ctrl)
template <int K>
__device__ __forceinline__ double row_ror(double v) {
  static_assert(K > 0 && K < 16, "row_ror");
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int rl = __builtin_amdgcn_mov_dpp(lo, 0x120 + K, 0xF, 0xF, true);
  const int rh = __builtin_amdgcn_mov_dpp(hi, 0x120 + K, 0xF, 0xF, true);
  return __hiloint2double(rh, rl);
}

// DPP move of a double within a 16-lane row by any control word (32-bit
// halves; full row mask): 0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1],
// 0x141 row_half_mirror, 0x140 row_mirror
template <int CTRL>
__device__ __forceinline__ double dpp64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}


// acc += (value of lane K of this row) * c   -- one v_fmac_f64 with a 64-bit
// DPP row_newbcast source (gfx950 DP-ALU DPP); the broadcast costs nothing
// extra.  hipcc neither pads nor schedules inside asm, so the VALU->DPP read
// hazard (2 wait states) is covered by the s_nop in the first term (NOP_FIRST).
template <int K, bool NOP_FIRST>
__device__ __forceinline__ void fmac_bcast(double& acc, double v, double c) {
  if (NOP_FIRST)
    asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
        : "+v"(acc) : "v"(v), "v"(c), "n"(K));
  else
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
        : "+v"(acc) : "v"(v), "v"(c), "n"(K));
}

// sum_k x[lane k] * c[k] over the 16 lanes of the row, x read by broadcast;
// the result is identical in every lane (fixed k order).  Four accumulators:
// rounds differently from dot2_bcast, so a kernel keeps the one it has.
__device__ __forceinline__ double dot_bcast(double x, const double (&c)[16]) {
#ifdef NIPAMD_ABLATE_NO_DOT      // timing-only ablation build (wrong results)
  return x * c[0];
#endif
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  fmac_bcast<0, true>(a0, x, c[0]);   fmac_bcast<1, false>(a1, x, c[1]);
  fmac_bcast<2, false>(a2, x, c[2]);  fmac_bcast<3, false>(a3, x, c[3]);
  fmac_bcast<4, false>(a0, x, c[4]);  fmac_bcast<5, false>(a1, x, c[5]);
  fmac_bcast<6, false>(a2, x, c[6]);  fmac_bcast<7, false>(a3, x, c[7]);
  fmac_bcast<8, false>(a0, x, c[8]);  fmac_bcast<9, false>(a1, x, c[9]);
  fmac_bcast<10, false>(a2, x, c[10]); fmac_bcast<11, false>(a3, x, c[11]);
  fmac_bcast<12, false>(a0, x, c[12]); fmac_bcast<13, false>(a1, x, c[13]);
  fmac_bcast<14, false>(a2, x, c[14]); fmac_bcast<15, false>(a3, x, c[15]);
  return (a0 + a1) + (a2 + a3);
}

// sum_k x[lane k] * c[k] with two accumulators (dot_bcast has four): two
// zeroing moves and one add per mat-vec instead of four and three; the
// other wave on the SIMD covers the longer fma chains.  c[k] = 0 past the
// chain's last state (opchain.hip).
__device__ __forceinline__ double dot2_bcast(double x, const double (&c)[16]) {
  double a0 = 0.0, a1 = 0.0;
  fmac_bcast<0, true>(a0, x, c[0]);   fmac_bcast<1, false>(a1, x, c[1]);
  fmac_bcast<2, false>(a0, x, c[2]);  fmac_bcast<3, false>(a1, x, c[3]);
  fmac_bcast<4, false>(a0, x, c[4]);  fmac_bcast<5, false>(a1, x, c[5]);
  fmac_bcast<6, false>(a0, x, c[6]);  fmac_bcast<7, false>(a1, x, c[7]);
  fmac_bcast<8, false>(a0, x, c[8]);  fmac_bcast<9, false>(a1, x, c[9]);
  fmac_bcast<10, false>(a0, x, c[10]); fmac_bcast<11, false>(a1, x, c[11]);
  fmac_bcast<12, false>(a0, x, c[12]); fmac_bcast<13, false>(a1, x, c[13]);
  fmac_bcast<14, false>(a0, x, c[14]); fmac_bcast<15, false>(a1, x, c[15]);
  return a0 + a1;
}

// acc[j & 3] += x(lane j of the row) * Ac[j], j = 0..15: one 16-state block
// of a wider mat-vec, the caller adds the four accumulators at the end
// (sixteen accumulators measured slower: 139K vs 128K cycles per block of
// chain_row64_kernel, the extra zeroing and adds cost more issue slots than
// the shorter chains save; a single wave per SIMD issues f64 VALU work every
// ~6.3 cycles)
__device__ __forceinline__ void fmac16(double (&acc)[4], double xb, const double (&Ac)[16]) {
  fmac_bcast<0, true>(acc[0], xb, Ac[0]);    fmac_bcast<1, false>(acc[1], xb, Ac[1]);
  fmac_bcast<2, false>(acc[2], xb, Ac[2]);   fmac_bcast<3, false>(acc[3], xb, Ac[3]);
  fmac_bcast<4, false>(acc[0], xb, Ac[4]);   fmac_bcast<5, false>(acc[1], xb, Ac[5]);
  fmac_bcast<6, false>(acc[2], xb, Ac[6]);   fmac_bcast<7, false>(acc[3], xb, Ac[7]);
  fmac_bcast<8, false>(acc[0], xb, Ac[8]);   fmac_bcast<9, false>(acc[1], xb, Ac[9]);
  fmac_bcast<10, false>(acc[2], xb, Ac[10]); fmac_bcast<11, false>(acc[3], xb, Ac[11]);
  fmac_bcast<12, false>(acc[0], xb, Ac[12]); fmac_bcast<13, false>(acc[1], xb, Ac[13]);
  fmac_bcast<14, false>(acc[2], xb, Ac[14]); fmac_bcast<15, false>(acc[3], xb, Ac[15]);
}

// K[k] += (value of lane k of this row) * w, k = 0..15 (E-step outer products)
__device__ __forceinline__ void acc_bcast(double (&K)[16], double x, double w) {
  fmac_bcast<0, true>(K[0], x, w);    fmac_bcast<1, false>(K[1], x, w);
  fmac_bcast<2, false>(K[2], x, w);   fmac_bcast<3, false>(K[3], x, w);
  fmac_bcast<4, false>(K[4], x, w);   fmac_bcast<5, false>(K[5], x, w);
  fmac_bcast<6, false>(K[6], x, w);   fmac_bcast<7, false>(K[7], x, w);
  fmac_bcast<8, false>(K[8], x, w);   fmac_bcast<9, false>(K[9], x, w);
  fmac_bcast<10, false>(K[10], x, w); fmac_bcast<11, false>(K[11], x, w);
  fmac_bcast<12, false>(K[12], x, w); fmac_bcast<13, false>(K[13], x, w);
  fmac_bcast<14, false>(K[14], x, w); fmac_bcast<15, false>(K[15], x, w);
}

// Sum over the 16 lanes of the row by the row_ror tree (8, 4, 2, 1);
// identical bits in every lane (each level pairs lanes whose partial sums are
// equal, and IEEE addition commutes).  The mirror tree below is another
// summation order: a kernel keeps the one it has.
// The ablation switch covers every user of this sum, opchain.hip and the
// wider sums of wave_ops.h (lanes_sum, wave_sum_n) included; default builds
// are unaffected.
__device__ __forceinline__ double row_sum(double x) {
#ifdef NIPAMD_ABLATE_NO_REDUCE   // timing-only ablation build (wrong results)
  return x;
#endif
  // x must be one rounded value in every lane: if x is a fresh product the
  // compiler may contract this lane's term of the first add into an fma
  // (x = a*b; x += ror(x) -> fma(a, b, ror(x))), the lanes then disagree in
  // the last bit, and a scale exponent taken from the sum can differ by one
  // between lanes (a sum of probabilities sits right at 1.0)
  asm("" : "+v"(x));
  x += row_ror<8>(x);
  x += row_ror<4>(x);
  x += row_ror<2>(x);
  x += row_ror<1>(x);
  return x;
}

// the maximum over the 16 lanes of the row, in every lane
__device__ __forceinline__ double row_max(double x) {
  x = fmax(x, row_ror<8>(x));
  x = fmax(x, row_ror<4>(x));
  x = fmax(x, row_ror<2>(x));
  x = fmax(x, row_ror<1>(x));
  return x;
}

// Sums over aligned groups of L = 8 or 16 lanes by the mirror tree (quad
// swaps, row_half_mirror, then row_mirror for L = 16), of n independent values
// level by level so that the n dependency chains interleave (one wave per
// SIMD: nothing else hides the f64 latency).  Every level pairs equal partial
// sums (or adds a value to its mirror), so all L lanes get identical bits.
template <int L, int n>
__device__ __forceinline__ void mirror_sum_n(double (&x)[n]) {
  static_assert(L == 8 || L == 16, "mirror_sum_n");
#pragma unroll
  for (int i = 0; i < n; i++) asm("" : "+v"(x[i]));   // one rounded value per lane: no fma contraction (row_sum)
#pragma unroll
  for (int i = 0; i < n; i++) x[i] += dpp64<0xB1>(x[i]);     // quad_perm [1,0,3,2]
#pragma unroll
  for (int i = 0; i < n; i++) x[i] += dpp64<0x4E>(x[i]);     // quad_perm [2,3,0,1]
#pragma unroll
  for (int i = 0; i < n; i++) x[i] += dpp64<0x141>(x[i]);    // row_half_mirror
  if (L == 16) {
#pragma unroll
    for (int i = 0; i < n; i++) x[i] += dpp64<0x140>(x[i]);  // row_mirror
  }
}
template <int L>
__device__ __forceinline__ double mirror_sum(double x) {
  double v[1] = {x};
  mirror_sum_n<L, 1>(v);
  return v[0];
}

// The largest binary exponent over the row's lanes, zeros excluded (kNoExp
// when all 16 are zero): 32-bit integer DPP work
constexpr int kNoExp = -0x40000;
__device__ __forceinline__ int row_max_exp(double p) {
  int e = p != 0.0 ? __builtin_amdgcn_frexp_exp(p) : kNoExp;
  e = max(e, __builtin_amdgcn_mov_dpp(e, 0x128, 0xF, 0xF, true));   // row_ror:8
  e = max(e, __builtin_amdgcn_mov_dpp(e, 0x124, 0xF, 0xF, true));   // row_ror:4
  e = max(e, __builtin_amdgcn_mov_dpp(e, 0x122, 0xF, 0xF, true));   // row_ror:2
  e = max(e, __builtin_amdgcn_mov_dpp(e, 0x121, 0xF, 0xF, true));   // row_ror:1
  return e;
}
// the scale that takes the largest element's exponent to 0; an all-zero
// vector keeps its scale (-> 0)
__device__ __forceinline__ int rescale_of_max_exp(int e) { return e > kNoExp ? -e : 0; }

// The rescale exponent from the largest element instead of the sum, 16-lane
// case (max_exp_rescale<NP> of wave_ops.h for wider groups): the rescale
// exponent of a proper model's forward rows, every step -- four DPP integer
// ops where the row's f64 sum was twelve.  Any power of two serves: the ll no
// longer reads the step masses, posteriors and xi are scale-free.
__device__ __forceinline__ int row_max_exp_rescale(double p) { return rescale_of_max_exp(row_max_exp(p)); }

}  // namespace
}  // namespace nipamd
