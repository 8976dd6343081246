// chain_group.h -- the lane-group layout of chain_viterbi_kernel (viterbi.hip),
// chain_stream_kernel (stream.hip), chain_soft_kernel (soft.hip) and
// chain_stream_soft_kernel (stream_soft.hip): device helpers, the forward step
// of the latter three, and the launch ladder.  What only those three share is
// soft_group.h's.
//
// NP = 16, 32 or 64 padded states, one NP-lane group per sequence, lane y =
// state y, 64 / NP sequences per wave, kGroupWaves independent waves per block:
// after the evidence tables are staged in LDS (one block barrier) no wave waits
// for another.  Above 16 states a value reaches the other lanes of its group
// through the wave's own row of a [kGroupWaves][64] LDS exchange area.  The
// kernels are instantiated over NP x the observed columns (0..4), so that the
// observation loads sit in no branch.  Included inside an anonymous namespace
// user, as dpp_row.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "chain_kernels.h"
#include "dpp_row.h"

namespace nipamd {
namespace {

constexpr int kGroupWaves = 4;

__host__ __device__ constexpr int group_np(int N) { return N <= 16 ? 16 : N <= 32 ? 32 : 64; }

// LDS operations of one wave complete in issue order: the wave's own rows
// need no barrier, only the compiler kept from reordering the accesses
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Sum / maximum over the NP lanes of a group, the same bits in every lane (each
// level pairs lanes whose partial results are equal).
template <int NP>
__device__ __forceinline__ double group_sum(double x) {
  x = row_sum(x);
  if constexpr (NP >= 32) x += __shfl_xor(x, 16, 64);
  if constexpr (NP == 64) x += __shfl_xor(x, 32, 64);
  return x;
}
template <int NP>
__device__ __forceinline__ double group_max(double x) {
  x = row_max(x);
  if constexpr (NP >= 32) x = fmax(x, __shfl_xor(x, 16, 64));
  if constexpr (NP == 64) x = fmax(x, __shfl_xor(x, 32, 64));
  return x;
}

// sum_k v[lane k of the group] c_k for this lane: c = this lane's 16 coefficients
// in registers (NP = 16), or column `y` of the LDS image Al [k][NP] above that,
// v passing through the wave's LDS row xch.  A fixed k order.
template <int NP>
__device__ __forceinline__ double matvec(double v, const double (&c)[16], const double* Al, double* xch, int lane,
                                         int gbase, int y) {
  if constexpr (NP == 16) {
    return dot_bcast(v, c);
  } else {
    xch[lane] = v;
    wave_lds_sync();
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
    for (int k = 0; k < NP; k += 4) {
      a0 = fma(xch[gbase + k], Al[k * NP + y], a0);
      a1 = fma(xch[gbase + k + 1], Al[(k + 1) * NP + y], a1);
      a2 = fma(xch[gbase + k + 2], Al[(k + 2) * NP + y], a2);
      a3 = fma(xch[gbase + k + 3], Al[(k + 3) * NP + y], a3);
    }
    wave_lds_sync();
    return (a0 + a1) + (a2 + a3);
  }
}

// the running totals of one sequence (the same values in every lane of its group)
struct Totals {
  double num, den;   // mantissas in [0.5, 1) of the products of the m2 and of the m1
  long ex;           // the products' exponents, num's minus den's
  unsigned status;
  long dead;      // the first step without mass, kStreamAlive while there is none
};

// One forward step at step t: al = alpha^_{t-1} -> alpha^_t under the evidence e.
// LL: the head's step, which also carries the totals.
template <int NP, bool LL>
__device__ __forceinline__ double fwd_step(double al, double e, double sall, const double (&Ac)[16], const double* Af,
                                           double* xch, int lane, int gbase, int y, long t, Totals& tot) {
  const double u = matvec<NP>(al, Ac, Af, xch, lane, gbase, y);
  const double a = u * e;
  const double m2 = group_sum<NP>(a);
  const bool ok = m2 > 0.0;
  if constexpr (LL) {
    const double m1 = group_sum<NP>(u * sall);
    if (ok) {
      int e2 = 0, e1 = 0;
      tot.num = frexp(tot.num * m2, &e2);
      tot.den = frexp(tot.den * m1, &e1);
      tot.ex += e2 - e1;
    } else {
      if (tot.dead == kStreamAlive) tot.dead = t;
      tot.status |= 1u;
    }
  }
  return ok ? a / m2 : 0.0;
}

// The block stages the NC evidence tables into tabs as [rows][NP] -- column k's
// M_k + 2 rows from row0[k] on -- and ebase as the row after them; returns that
// row (tabs + rows NP; evid_rows(a) rows with it).  The caller's block barrier
// makes them visible.  chain_viterbi_kernel has the same loop written out
// (viterbi.hip says why).
template <int NP, int NC>
__device__ __forceinline__ double* stage_tables(const EvidenceArgs& a, double* tabs, int tid,
                                                int (&row0)[NC > 0 ? NC : 1]) {
  int rows = 0;
#pragma unroll
  for (int k = 0; k < NC; k++) {
    row0[k] = rows;
    const int n = (a.M[k] + 2) * NP;
    for (int i = tid; i < n; i += kGroupWaves * 64) tabs[rows * NP + i] = a.tab[k][(i / NP) * 64 + (i % NP)];
    rows += a.M[k] + 2;
  }
  double* eb = tabs + rows * NP;
  if (tid < NP) eb[tid] = a.ebase[tid];
  return eb;
}

// rows of the staged tables, ebase included
inline size_t evid_rows(const EvidenceArgs& a) {
  size_t rows = 1;
  for (int k = 0; k < a.ncol; k++) rows += (size_t)a.M[k] + 2;
  return rows;
}

// the shapes every launcher refuses (a: ViterbiArgs, StreamArgs, SoftArgs or StreamSoftArgs)
template <typename Args>
bool cols_shape_ok(const Args& a) {
  if (a.N < 1 || a.N > 64 || a.ncol < 0 || a.ncol > 4 || a.nq < 0 || a.nq > kViterbiMaxQuery || a.B < 1 ||
      a.B > 0x7fffffffL)
    return false;
  for (int k = 0; k < a.ncol; k++) if (a.M[k] < 1) return false;
  for (int j = 0; j < a.nq; j++) if (a.qstride[j] < 1 || a.qcard[j] < 1) return false;
  return true;
}

// The instantiation that serves a (NP = group_np(a.N), NC = a.ncol), as
// kernel_of(integral_constant NP, integral_constant NC) names it: its
// dynamic-LDS limit raised to lds bytes (ensure_dyn_lds) and, if launch, one
// group per sequence queued on stream.
template <typename Args, typename KernelOf>
int group_launch(const Args& a, size_t lds, bool launch, hipStream_t stream, KernelOf kernel_of) {
  lds = (lds + 15) & ~(size_t)15;
  auto run = [&](auto np, auto nc) -> int {
    constexpr int G = 64 / decltype(np)::value;
    static size_t lds_set[kMaxDevices] = {};               // of this instantiation
    void (*const kernel)(Args) = kernel_of(np, nc);
    if (const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), lds, lds_set)) return rc;
    if (!launch) return 0;
    const long waves = (a.B + G - 1) / G;
    const dim3 grid((unsigned)((waves + kGroupWaves - 1) / kGroupWaves)), block(kGroupWaves * 64);
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  };
  auto columns = [&](auto np) -> int {
    switch (a.ncol) {
      case 0: return run(np, std::integral_constant<int, 0>{});
      case 1: return run(np, std::integral_constant<int, 1>{});
      case 2: return run(np, std::integral_constant<int, 2>{});
      case 3: return run(np, std::integral_constant<int, 3>{});
      default: return run(np, std::integral_constant<int, 4>{});
    }
  };
  if (a.N <= 16) return columns(std::integral_constant<int, 16>{});
  if (a.N <= 32) return columns(std::integral_constant<int, 32>{});
  return columns(std::integral_constant<int, 64>{});
}

}  // namespace
}  // namespace nipamd
