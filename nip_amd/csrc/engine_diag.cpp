// engine_diag.cpp -- diagnostics builds only (-DNIPAMD_DIAGNOSTICS, diag.h):
// the kernels' per-block phase stamps (NIPAMD_PHASE_TIMES=1), fetched after
// the launch and printed as summaries.  The product build compiles none of it.
#ifdef NIPAMD_DIAGNOSTICS
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "engine_internal.h"

namespace nipamd::eng {

bool phase_times() {
  static const bool v = std::getenv("NIPAMD_PHASE_TIMES") != nullptr;
  return v;
}

int StampBuf::attach(bool want, size_t words, hipStream_t st, unsigned long long** slot) {
  if (!want || !words) return 0;
  HIP_OK(hipMalloc(&dev, words * sizeof(unsigned long long)));
  n = words;
  HIP_OK(hipMemsetAsync(dev, 0, n * sizeof(unsigned long long), st));
  *slot = dev;
  return 0;
}

int StampBuf::fetch(hipStream_t st, Stamps& h) {
  h.resize(n);
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipMemcpy(h.data(), dev, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
}

// per-block phase timestamps of the matrix-core fb kernel
void report_phases(const Stamps& hv, int nblk) {
  const unsigned long long* h = hv.data();
  double sa = 0, sb = 0, sc = 0;
  for (int k = 0; k < nblk; k++) {
    sa += (double)(h[k * 4 + 1] - h[k * 4 + 0]);
    sb += (double)(h[k * 4 + 2] - h[k * 4 + 1]);
    sc += (double)(h[k * 4 + 3] - h[k * 4 + 2]);
  }
  std::fprintf(stderr, "[nipamd] phase cycles (mean over %d blocks): A %.0f  barrier %.0f  B %.0f\n",
               nblk, sa / nblk, sb / nblk, sc / nblk);
  double w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < nblk; k++)
    for (int i = 0; i < 8; i++) w[i] += (double)h[(size_t)nblk * 4 + k * 8 + i];
  if (w[0] + w[4] > 0)
    std::fprintf(stderr, "[nipamd] barrier wait cycles A/B: fwd filter %.0f/%.0f  bwd filter %.0f/%.0f  "
                 "fwd partner %.0f/%.0f  bwd partner %.0f/%.0f\n", w[0] / nblk, w[4] / nblk, w[1] / nblk,
                 w[5] / nblk, w[2] / nblk, w[6] / nblk, w[3] / nblk, w[7] / nblk);
  double pp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < nblk; k++)
    for (int i = 0; i < 8; i++) pp[i] += (double)h[(size_t)nblk * 16 + k * 8 + i];
  if (pp[0] + pp[4] > 0)
    std::fprintf(stderr, "[nipamd] phase-B partner cycles (DMA wait / ll / drain): fwd %.0f/%.0f/%.0f  "
                 "bwd %.0f/%.0f/%.0f\n", pp[0] / nblk, pp[1] / nblk, pp[2] / nblk, pp[4] / nblk, pp[5] / nblk,
                 pp[6] / nblk);
  const unsigned long long* rt = h + (size_t)nblk * 12;   // s_memrealtime (100 MHz)
  unsigned long long t0 = ~0ull, e0 = 0, e1 = ~0ull, s1 = 0;
  double mhz = 0, me = 0, st0 = 0;
  for (int k = 0; k < nblk; k++) {
    t0 = std::min(t0, rt[k * 4 + 0]); s1 = std::max(s1, rt[k * 4 + 0]);
    e0 = std::max(e0, rt[k * 4 + 2]); e1 = std::min(e1, rt[k * 4 + 2]);
    me += (double)(rt[k * 4 + 2] - rt[k * 4 + 0]);
    st0 += (double)(h[k * 4] - rt[k * 4 + 1]);
    if (rt[k * 4 + 2] > rt[k * 4 + 0])
      mhz += 100.0 * (double)(rt[k * 4 + 3] - rt[k * 4 + 1]) / (double)(rt[k * 4 + 2] - rt[k * 4 + 0]);
  }
  std::fprintf(stderr, "[nipamd] wall us: last entry %.2f  first end %.2f  last end %.2f  mean block %.2f  "
               "clock %.0f MHz; entry->stamp0 cycles %.0f\n", (s1 - t0) / 100.0, (e1 - t0) / 100.0,
               (e0 - t0) / 100.0, me / nblk / 100.0, mhz / nblk, st0 / nblk);
}

void report_ckpt_waves(const Stamps& w, int nblk) {
  double m[40] = {0};
  for (int k = 0; k < nblk; k++)
    for (int i = 0; i < 40; i++) m[i] += (double)w[(size_t)k * 40 + i] / nblk;
  if (!(m[2] > 0)) return;
  std::fprintf(stderr, "[nipamd] ckpt kernel cycles per wave (phase A / phase-barrier wait / phase B / "
               "phase-B barrier waits / mean SIMD id; block 0's SIMD ids):\n");
  // a wave's phase-A role (row-form filters of chains 4q..4q+3; with
  // NIPAMD_CK_PHASEA=mfma the phase-B role's own phase A) / its phase-B role.
  // The filters' phase-B column includes their phase-barrier wait; with
  // NIPAMD_CK_PHASEA=mfma their columns are 0 / staging / whole kernel.
  static const char* names[8] = {"fwd rows 0 / fwd filter", "fwd rows 1 / bwd filter", "fwd rows 2 / fwd partner",
                                 "fwd rows 3 / bwd partner", "bwd rows 0 / bwd post 8-15",
                                 "bwd rows 1 / fwd post 8-15", "bwd rows 2 / beta recompute",
                                 "bwd rows 3 / alpha recompute"};
  for (int v = 0; v < 8; v++)
    std::fprintf(stderr, "[nipamd]   %-29s %9.0f %9.0f %9.0f %9.0f %5.2f %llu\n", names[v], m[v * 5], m[v * 5 + 1],
                 m[v * 5 + 2], m[v * 5 + 3], m[v * 5 + 4], w[v * 5 + 4]);
}

void report_mfma_wide(const Stamps& h, int nblk) {
  double m[16] = {0};
  for (int k = 0; k < nblk; k++)
    for (int i = 0; i < 16; i++) m[i] += (double)h[(size_t)k * 16 + i] / nblk;
  static const char* names[4] = {"fwd filter", "bwd filter", "fwd partner", "bwd partner"};
  std::fprintf(stderr, "[nipamd] mfma_wide cycles per wave (phase A / its barrier waits / phase B / its barrier waits):\n");
  for (int v = 0; v < 4; v++)
    std::fprintf(stderr, "[nipamd]   %-12s %9.0f %9.0f %9.0f %9.0f\n", names[v], m[v * 4], m[v * 4 + 1], m[v * 4 + 2],
                 m[v * 4 + 3]);
}

void report_wide4(const Stamps& h, long B) {
  double m[16] = {0};
  for (long b = 0; b < B; b++)
    for (int i = 0; i < 16; i++) m[i] += (double)h[(size_t)b * 16 + i] / B;
  std::fprintf(stderr, "[nipamd] wide4 cycles (total / wait / before / after barrier): fwd filter %.0f / %.0f / %.0f / %.0f  "
               "bwd filter %.0f / %.0f / %.0f / %.0f  partners %.0f %.0f  staging %.0f  block %.0f\n", m[0], m[1],
               m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[12], m[9], m[10]);
  unsigned long long e0 = ~0ull, e1 = 0, x0 = ~0ull, x1 = 0;
  for (long b = 0; b < B; b++) {
    e0 = std::min(e0, h[(size_t)b * 16 + 11]); e1 = std::max(e1, h[(size_t)b * 16 + 11]);
    x0 = std::min(x0, h[(size_t)b * 16 + 13]); x1 = std::max(x1, h[(size_t)b * 16 + 13]);
  }
  std::fprintf(stderr, "[nipamd] wide4 wall us: entries spread %.2f  first exit %.2f  last exit %.2f\n",
               (e1 - e0) / 100.0, (x0 - e0) / 100.0, (x1 - e0) / 100.0);
}

// chain_estep_ck_kernel [group][5]
static void report_estep_ck(const Stamps& h, long ngrp) {
  unsigned long long t0 = ~0ull, t1 = 0;
  double fw = 0, bw = 0, wall = 0;
  for (long k = 0; k < ngrp; k++) {
    const unsigned long long* r = h.data() + k * 5;
    t0 = std::min(t0, r[0]);
    t1 = std::max(t1, r[1]);
    fw += (double)r[2];
    bw += (double)r[3];
    wall += (double)(r[1] - r[0]);
  }
  std::fprintf(stderr, "[nipamd] estep_ck groups %ld, launch span %.1f us; per group: forward %.0f cycles, "
               "backward %.0f cycles, wall %.1f us\n", ngrp, (t1 - t0) / 100.0, fw / ngrp, bw / ngrp,
               wall / ngrp / 100.0);
}

// chain_estep16_kernel [block of 8 or 16 sequences: room for either][16 waves][4]
static void report_estep16(const Stamps& h, int nblk8) {
  double m[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  int nw[2] = {0, 0};
  for (int k = 0; k < nblk8; k++)
    for (int w = 0; w < 16; w++) {
      const unsigned long long* r = h.data() + ((size_t)k * 16 + w) * 4;
      if (r[0] + r[2] == 0) continue;
      const int dd = w < 8 ? 0 : 1;
      for (int i = 0; i < 4; i++) m[dd][i] += (double)r[i];
      nw[dd]++;
    }
  for (int dd = 0; dd < 2; dd++)
    if (nw[dd])
      std::fprintf(stderr, "[nipamd] estep16 %s waves: phase A %.0f  barrier wait %.0f  phase B %.0f  "
                   "block entry to exit %.0f cycles (mean of %d)\n", dd ? "backward" : "forward",
                   m[dd][0] / nw[dd], m[dd][1] / nw[dd], m[dd][2] / nw[dd], m[dd][3] / nw[dd], nw[dd]);
}

// the matrix-core e_step [block][24]
static void report_estep_mfma(const Stamps& h, int nblk) {
  unsigned long long t0 = ~0ull, tend = 0;
  double d[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < nblk; k++) {
    const unsigned long long* r = h.data() + (size_t)k * 24;
    t0 = std::min(t0, r[0]);
    for (int i = 1; i < 7; i++) { d[i] += (double)(r[i] - r[0]); tend = std::max(tend, r[i]); }
  }
  std::fprintf(stderr, "[nipamd] e_step blocks %d, launch span %.1f us; mean us from block entry: staged %.1f  "
               "phase A end %.1f  fwd filter end %.1f  bwd filter end %.1f  fwd partner end %.1f  "
               "bwd partner end %.1f\n", nblk, (tend - t0) / 100.0, d[1] / nblk / 100.0, d[2] / nblk / 100.0,
               d[3] / nblk / 100.0, d[4] / nblk / 100.0, d[5] / nblk / 100.0, d[6] / nblk / 100.0);
  double pcs[10] = {0};
  for (int k = 0; k < nblk; k++)
    for (int i = 0; i < 10; i++) pcs[i] += (double)h[(size_t)k * 24 + 8 + i];
  std::fprintf(stderr, "[nipamd] e_step partner phase-B cycles (wait / in-lane / xi / q / counts): "
               "fwd %.0f %.0f %.0f %.0f %.0f  bwd %.0f %.0f %.0f %.0f %.0f\n", pcs[0] / nblk, pcs[1] / nblk,
               pcs[2] / nblk, pcs[3] / nblk, pcs[4] / nblk, pcs[5] / nblk, pcs[6] / nblk, pcs[7] / nblk,
               pcs[8] / nblk, pcs[9] / nblk);
}

size_t estep_stamp_words(EstepKernel ek, long nb) {
  return ek == kEstepMfma ? (size_t)((nb + 15) / 16) * 24 : ek == kEstepCk ? (size_t)((nb + 15) / 16) * 5
       : ek == kEstep16 ? (size_t)((nb + 7) / 8) * 64 : 0;
}

void report_estep(const Stamps& h, std::pair<EstepKernel, long> ek_nb) {
  const EstepKernel ek = ek_nb.first;
  const long nb = ek_nb.second;
  if (ek == kEstepMfma) report_estep_mfma(h, (int)((nb + 15) / 16));
  if (ek == kEstepCk) report_estep_ck(h, (nb + 15) / 16);
  if (ek == kEstep16) report_estep16(h, (int)((nb + 7) / 8));
}

}  // namespace nipamd::eng
#endif  // NIPAMD_DIAGNOSTICS
