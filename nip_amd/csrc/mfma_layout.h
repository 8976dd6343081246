// mfma_layout.h -- the matrix-core (v_mfma_f64_16x16x4) register layout the
// chain kernels share, one definition each: the accumulator vector types, the
// state a register of a lane holds, loading and scaling such a vector, the
// one-instruction MFMA, the XOR-swizzled LDS piece offset and the packed
// code byte.  What lives inside a 16-lane row is in dpp_row.h, what crosses
// rows in wave_ops.h.  Included once per translation unit (namespace nipamd,
// anonymous).
#pragma once
#include <hip/hip_runtime.h>

namespace nipamd {
namespace {

typedef double v4d __attribute__((ext_vector_type(4)));   // an f64 MFMA accumulator
typedef double v2d __attribute__((ext_vector_type(2)));

// One 16x16x4 f64 MFMA: D += A (16 x 4) B (4 x 16); lane l supplies
// A[l & 15][l >> 4] and B[l >> 4][l & 15], and holds D[(l >> 4) + 4 r][l & 15].
__device__ __forceinline__ v4d mfma(double a, double b, v4d d) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, d, 0, 0, 0);
}

// The filters permute A's rows so that lane (g, j) = lane 16 g + j holds, of
// chain j's 16 states, two 16-byte pieces: states 2g, 2g + 1 and 2g + 8,
// 2g + 9.  state_of: the actual state held by register r of lane group g.
__host__ __device__ constexpr int state_of(int g, int r) { return r < 2 ? 2 * g + r : 6 + 2 * g + r; }

// This lane's four states of a 16-state row (tile q of a wider one);
// p = row + 16q + 2g.  Two forms of the same two 16-byte loads, because the
// compiler sees them differently: load4 reads HIP's double2 (a struct of
// doubles, so the loads alias plain double stores by type), load4v the vector
// type v2d, as those kernels' other LDS accesses do.  Each kernel schedules
// around the form it was written with, and the other form moves its
// s_waitcnt placement (and, in estep_ckw.hip, its register allocation): the
// narrow kernels and estep_ckw.hip use load4, chain_mfma_wide.hip and
// estep_mw.hip load4v.
__device__ __forceinline__ v4d load4(const double* p) {
  const double2 a = *reinterpret_cast<const double2*>(p);
  const double2 b = *reinterpret_cast<const double2*>(p + 8);
  v4d r;
  r.x = a.x; r.y = a.y; r.z = b.x; r.w = b.y;
  return r;
}
__device__ __forceinline__ v4d load4v(const double* p) {
  const v2d a = *reinterpret_cast<const v2d*>(p);
  const v2d b = *reinterpret_cast<const v2d*>(p + 8);
  return v4d{a.x, a.y, b.x, b.y};
}

__device__ __forceinline__ v4d ldexp4(v4d v, int k) {
  v4d r;
  r.x = __builtin_ldexp(v.x, k); r.y = __builtin_ldexp(v.y, k);
  r.z = __builtin_ldexp(v.z, k); r.w = __builtin_ldexp(v.w, k);
  return r;
}

// v with the entries zeroed whose entry of m is 0 (a select, never a product:
// v may hold inf)
__device__ __forceinline__ v4d zero_where_zero(v4d v, const v4d& m) {
  v.x = m.x != 0.0 ? v.x : 0.0; v.y = m.y != 0.0 ? v.y : 0.0;
  v.z = m.z != 0.0 ? v.z : 0.0; v.w = m.w != 0.0 ? v.w : 0.0;
  return v;
}

// LDS layout of one step's (or one transpose buffer's) rows, STRIDE doubles
// each: row j's states at j * STRIDE, its 16-byte piece p (states 2p, 2p + 1)
// XOR-swizzled by j & 7, so that the filter-layout writes (lane (g, j):
// pieces g and g + 4 of row j) and the partners' / sequence-major reads (a
// row's 16 doubles per 16 lanes) are bank-conflict free.
template <int STRIDE>
__device__ __forceinline__ int piece_off(int j, int p) { return j * STRIDE + ((p ^ (j & 7)) << 1); }

// byte k of a word of four packed observation codes
__device__ __forceinline__ unsigned byte_of(unsigned w, int k) { return (w >> (8 * k)) & 0xFFu; }

}  // namespace
}  // namespace nipamd
