// engine_estep.cpp -- the batched e_step: the partial's size and routes (the
// chain kernels' slabs summed by the fixed-order tree, the operator chain,
// the general engine), the reference's prefix verdict, the slab -> em_learn
// maps and the finalize (engine_internal.h).
//
// The chain e_step kernels serve interface chains with evidence on their
// leaf children; every other e_step runs on the general engine, whose partial
// is the em_learn layout itself.  The partial is [body | route tag]: the body
// holds any layout the model's routes produce (the largest of the sizes), the
// three tag slots count the partials summed into it per route -- (1, 0, 0)
// the 16-state chain slab, (0, 1, 0) em_learn layout, (0, 0, 1) the wide
// chain slab (estep_wide.hip) -- so partials of different routes (another T,
// another engine setting, another rank) that were combined are detected by
// the finalize instead of being summed silently.
#include <algorithm>
#include <cstdlib>
#include <functional>

#include "engine_internal.h"

using namespace nipamd::eng;

namespace {

// Sequences per E-step launch: bounds the slab + scratch memory.  A power of
// two times 64^k, so chunk trees are subtrees of the one binary tree over the
// batch (see tree64_kernel).
#ifndef NIPAMD_ESTEP_SEQS
#define NIPAMD_ESTEP_SEQS 16384
#endif
constexpr long kEstepChunk = NIPAMD_ESTEP_SEQS;
// chain_estep_ck_kernel's launches: its scratch holds one checkpoint per four
// steps (~4.4 GB at 131072 x 1024), so a whole config-4 shard is one launch
constexpr long kEstepCkChunk = 131072;
constexpr int kTagSlots = 3;

// The body is the larger of the layouts this model's routes can produce,
// whatever the engine setting, so the tag sits at the same offset for every
// partial of a model version (a set_engine between partial and finalize
// cannot move it into the counts).
int estep_body_size(const nipamd_model* mm) {
  int body = nipamd::param_size(mm->m);
  const auto& P = mm->m.chain;
  if (P.valid && (P.hmm || P.jhmm)) body = std::max(body, nipamd::chain_estep_slab(P.emits[0].M));
  if (estep_general_plan(P)) body = std::max(body, nipamd::chain_estep_slab(estep_rows(P) - 2));
  if (estep_wide_plan(mm->m)) body = std::max(body, nipamd::estep_wide_slab(P.N, estep_rows(P)));
  return body;
}

// The request's route is the operator chain's e_step (the chain and wide
// routes decline it, the engine choice is automatic and the operator chain
// takes it): its partial carries a section after the route tag.
// capacity: the caller's partial in doubles (-1: unbounded, the size query).
// The operator chain's partial is larger than nipamd_estep_partial_size, so a
// partial of that size (nipamd_estep_partial, which takes no capacity) runs
// such requests on the general engine, whose partial fits.
bool op_estep_route(nipamd_model* mm, int n_obs, const int* obs_vars, int T, long capacity) {
  Route r;
  if (mm->engine != NIPAMD_ENGINE_AUTO || chain_estep_ok(mm, n_obs, obs_vars, T, r) ||
      wide_estep_ok(mm, n_obs, obs_vars, r))
    return false;
  std::string why;
  if (!nipamd::op_estep_supported(mm, n_obs, obs_vars, T, why)) return false;
  return capacity < 0 ||
         capacity >= (long)nipamd_estep_partial_size(mm) + (long)nipamd::op_estep_section(mm, n_obs, obs_vars);
}

// The reference's verdict on a leading run of missing observations
// (prefix.cpp), once per model version and T; -1: no step is rejected.
// prefix.cpp bounds its own work (entries x steps); models whose join tree
// holds more than kPrefixMaxEntries table entries are not simulated at all
// (-2: their leading missing runs are accepted).
constexpr long kPrefixMaxEntries = 1L << 26;

int prefix_first_bad(nipamd_model* mm, int T) {
  const int c = mm->pf_first_bad;
  // -1 holds for every shorter T, a step >= 0 for every T, -2 (the work bound
  // ran out) for every longer T
  const bool hit = mm->pf_version == mm->version &&
                   (c >= 0 || (c == -1 && T <= mm->pf_T) || (c == -2 && T >= mm->pf_T));
  if (!hit) {
    mm->pf_first_bad = nipamd::estep_prefix_entries(mm->m) > kPrefixMaxEntries
                           ? -2 : nipamd::estep_prefix_first_bad(mm->m, T, nullptr);
    mm->pf_version = mm->version;
    mm->pf_T = T;
  }
  const int k = mm->pf_first_bad;
  return k >= 0 && k < T ? k : -1;
}

// A route writes the first `written` doubles of the body; the rest (another
// route's larger layout) is zeroed, so every partial is fully defined and
// partials of one route combine and compare bit for bit.
int zero_tail(nipamd_model* mm, double* d_partial, int written, hipStream_t st) {
  const int body = estep_body_size(mm);
  if (written < body) HIP_OK(hipMemsetAsync(d_partial + written, 0, (size_t)(body - written) * sizeof(double), st));
  return 0;
}

// What the chain routes share: the kernels of a route write one slab row
// [S] per `per_row` sequences, `chunk` sequences per launch, and the
// fixed-order tree sums the rows (per chunk, then over the chunks) into the
// partial.  prepare() runs once before the first launch (table uploads; not
// for an empty batch); launch(b0, nb, slab) queues the kernels of sequences
// b0 .. b0 + nb and returns the engine's error code.  The scratch
// (DevState::S) and the work buffer are only valid from prepare() on.
struct SlabRun {
  int S;              // doubles per slab row = what the route writes of the body
  long chunk;         // sequences per launch, at most B
  int per_row;        // sequences per slab row
  size_t scratch;     // bytes of DevState::S one launch needs
  double tag[kTagSlots];
};

template <typename Prepare, typename Launch>
int run_slab_chunks(nipamd_model* mm, const SlabRun& s, long B, double* d_partial, hipStream_t st,
                    Prepare prepare, Launch launch) {
  if (nipamd::estep_tag_launch(d_partial + estep_body_size(mm), s.tag[0], s.tag[1], s.tag[2], st))
    return fail(NIPAMD_ERROR_DEVICE, "tag launch failed");
  if (int rc = zero_tail(mm, d_partial, s.S, st)) return rc;
  if (B == 0) { HIP_OK(hipMemsetAsync(d_partial, 0, (size_t)s.S * sizeof(double), st)); return 0; }
  if (int rc = prepare()) return rc;
  const long nchunks = (B + s.chunk - 1) / s.chunk;
  const long rows = (s.chunk + s.per_row - 1) / s.per_row;
  const long lvl = (rows + 63) / 64;
  const size_t work = ((size_t)rows + 2 * lvl + nchunks + 64) * s.S * sizeof(double);
  if (int rc = ensure_scratch(mm, s.scratch)) return rc;
  if (int rc = ensure_work(mm, work)) return rc;
  double* slab = dev_of(mm)->W;
  double* tA = slab + (size_t)rows * s.S;
  double* tB = tA + (size_t)lvl * s.S;
  double* cres = tB + (size_t)lvl * s.S;
  for (long c = 0; c < nchunks; c++) {
    const long b0 = c * s.chunk;
    const long nb = (B - b0) < s.chunk ? (B - b0) : s.chunk;
    if (int rc = launch(b0, nb, slab)) return rc;
    double* out = nchunks == 1 ? d_partial : cres + (size_t)c * s.S;
    if (reduce_rows(slab, (nb + s.per_row - 1) / s.per_row, s.S, tA, tB, out, st))
      return fail(NIPAMD_ERROR_DEVICE, "reduction launch failed");
  }
  if (nchunks > 1 && reduce_rows(cres, nchunks, s.S, tA, tB, d_partial, st))
    return fail(NIPAMD_ERROR_DEVICE, "reduction launch failed");
  return 0;
}

// sequences per launch: a power of two in [lo, hi] (the chunk trees are
// subtrees of the batch's tree) whose scratch stays within `budget` bytes
long pow2_chunk(size_t per_seq, size_t budget, long lo, long hi) {
  const size_t cap = std::min<size_t>(hi, std::max<size_t>(lo, budget / per_seq));
  long chunk = lo;
  while ((size_t)chunk * 2 <= cap) chunk *= 2;
  return chunk;
}

// the fused 17..32-state kernels: scratch within ~8 GB, config 3's 65,536 x 256 in one launch
long mw_chunk(bool ck, int T) {
  const size_t per_seq = ck ? nipamd::chain_estep_ckw_scratch_bytes(16, T) / 16 + 1
                            : nipamd::estep_mw_scratch_bytes(32, T) / 32 + 1;
  return pow2_chunk(per_seq, (size_t)8 << 30, 32, 65536);
}

// the two-kernel wide route: the messages of a chunk stay within ~4 GB of
// HBM, and the chunk is a power of two (>= 16), so power-of-two shards
// combine into exactly the whole batch's partial (nip_amd.h).
// NIPAMD_ESTEP_WIDE_BYTES lowers the byte budget in diagnostics builds (the
// multi-chunk shard-invariance test).
long wide_chunk(int N, int T) {
  size_t budget = (size_t)4 << 30;
  if (const char* wb = nipamd::diag_env("NIPAMD_ESTEP_WIDE_BYTES")) budget = (size_t)std::atoll(wb);
  return pow2_chunk(nipamd::estep_wide_scratch_bytes(N, 1, T), budget, 16, kEstepChunk);
}

// The fused matrix-core e_step (estep_mw.hip) for 17..32 states: the wide
// slab layout (K [32][32], H [R][32], P0 [32]), one row per 16 sequences.
// taken = false (nothing done) when the request does not fit the kernel: the
// caller takes the two-kernel route.
int estep_mw_partial(nipamd_model* mm, const Route& r, const int32_t* d_obs, int n_obs, int B, int T,
                     double* d_partial, double* d_ll, uint32_t* d_status, hipStream_t st, bool& taken) {
  const auto& P = mm->m.chain;
  taken = false;
  if (nipamd::estep_wide_np(P.N) != 32 || r.ncol > nipamd::estep_mw_max_cols()) return 0;
  if (nipamd::diag_env("NIPAMD_ESTEP_WIDE_TWO_KERNELS")) return 0;   // A/B: the round-4 route
  bool seen[4];
  int rows = 0;
  if (!observed_children(P, r, seen, &rows) || rows > 64) return 0;
  if (int rc = ensure_tables(mm)) return rc;
  ReqTables* rt = nullptr;
  if (int rc = ensure_req_tables(mm, r, &rt)) return rc;
  if (nipamd::estep_mw_lds_bytes(rt->mtab_rows) > nipamd::kLdsPerCU) return 0;
  taken = true;
  const int R = estep_rows(P);
  const int S = nipamd::estep_wide_slab(P.N, R);
  // chain_estep_ckw_kernel (checkpoints + recomputation, round 6): the
  // default where every step may rescale every 4th step (step_shrink_ok) and
  // its LDS fits; NIPAMD_ESTEP_WIDE_KERNEL=mw in diagnostics builds runs
  // chain_estep_mw_kernel instead
  const char* wk = nipamd::diag_env("NIPAMD_ESTEP_WIDE_KERNEL");
  const bool ck = !(wk && std::string(wk) == "mw") && r.ncol >= 1 && r.ncol <= 2 &&
                  nipamd::chain_estep_ckw_lds_bytes(rt->mtab_rows, rows + 2 * r.ncol) <= nipamd::kLdsPerCU &&
                  step_shrink_ok(rt->shrink);
  const long chunk = std::min<long>(B, mw_chunk(ck, T));
  const SlabRun run{S, chunk, 16, ck ? nipamd::chain_estep_ckw_scratch_bytes(chunk, T)
                                     : nipamd::estep_mw_scratch_bytes(chunk, T), {0.0, 0.0, 1.0}};
  DevState* d = dev_of(mm);
  nipamd::EMwArgs a{};
  set_cols(a, P, r, rt->mtab, rt->mtab_off);
  for (int i = 0, v = 0; i < 4; i++) {
    a.voff[i] = v;
    v += a.M[i];
  }
  for_each_child(P, r, (int)P.emits.size(), [&](int k, int row, int slot) {
    if (slot >= 0) {
      a.crow[slot] = row;
    } else {
      a.urow[a.n_unobs] = row;
      a.uM[a.n_unobs++] = P.emits[k].M;
    }
  });
  a.tab_rows = rt->mtab_rows;
  a.T = T; a.H = T / 2; a.N = P.N;
  a.A = d->A64; a.pi = d->pi64; a.w = rt->wv;
  a.slab_size = S; a.R = R;
  return run_slab_chunks(mm, run, B, d_partial, st, [] { return 0; }, [&](long b0, long nb, double* slab) {
    set_obs_view(a, d_obs, n_obs, T, b0);
    a.B = nb;
    a.S = d->S; a.slab = slab;
    a.ll = d_ll ? d_ll + b0 : nullptr;
    a.status = d_status ? d_status + b0 : nullptr;
    return ck ? launched(nipamd::chain_estep_ckw_launch(a, chain_proper(P), st), "chain_estep_ckw_kernel")
              : launched(nipamd::estep_mw_launch(a, st), "chain_estep_mw_kernel");
  });
}

// The wide chain e_step (estep_wide.hip): the filters store every message of
// a chunk of sequences, the statistics kernel writes one slab row per 16
// sequences.
int estep_wide_partial(nipamd_model* mm, const Route& r, const int32_t* d_obs, int n_obs, int B, int T,
                       double* d_partial, double* d_ll, uint32_t* d_status, hipStream_t st) {
  const auto& P = mm->m.chain;
  {
    bool taken = false;
    const int rc = estep_mw_partial(mm, r, d_obs, n_obs, B, T, d_partial, d_ll, d_status, st, taken);
    if (rc || taken) return rc;
  }
  const int R = estep_rows(P);
  const int S = nipamd::estep_wide_slab(P.N, R);
  const int NP = nipamd::estep_wide_np(P.N);
  const long chunk = std::min<long>(B, wide_chunk(P.N, T));
  const SlabRun run{S, chunk, 16, nipamd::estep_wide_scratch_bytes(P.N, chunk, T), {0.0, 0.0, 1.0}};
  ReqTables* rt = nullptr;
  auto prepare = [&] {
    if (int rc = ensure_tables(mm)) return rc;
    return ensure_req_tables(mm, r, &rt);
  };
  return run_slab_chunks(mm, run, B, d_partial, st, prepare, [&](long b0, long nb, double* slab) {
    const DevState* d = dev_of(mm);
    nipamd::EWideArgs a{};
    set_obs_view(a, d_obs, n_obs, T, b0);
    set_cols(a, P, r, rt->tabw, rt->tabw_off);
    a.ebase = rt->ebase; a.s = d->sall64; a.A = d->A64; a.pi = d->pi64;
    a.B = nb; a.T = T; a.N = P.N;
    a.Sa = d->S;
    a.Sb = a.Sa + (size_t)chunk * T * NP;
    a.Ea = reinterpret_cast<int*>(a.Sb + (size_t)chunk * (T + 1) * NP);
    a.ll = d_ll ? d_ll + b0 : nullptr;
    a.status = d_status ? d_status + b0 : nullptr;
    a.slab = slab; a.slab_size = S; a.R = R;
    a.proper = chain_proper(P) ? 1 : 0;
    a.nchild = (int)P.emits.size();
    for_each_child(P, r, a.nchild, [&](int k, int row, int slot) {
      a.ccol[k] = slot >= 0 ? r.col[slot] : -1;
      a.cM[k] = P.emits[k].M;
      a.erow[k] = row;
    });
    return launched(nipamd::estep_wide_launch(a, st), "wide chain e_step (chain_msgs_kernel + chain_stats_kernel)");
  });
}

// Every leaf child's evidence table for the general chain e_step: rows
// M_k + 2 per child (E_k[m][y], the row sums, an all-zero row for an
// out-of-range state), 16 columns, children in plan order.
int ensure_etab_all(nipamd_model* mm) {
  DevState* d = dev_of(mm);
  if (d->etab_all) return 0;
  const auto& P = mm->m.chain;
  std::vector<double> E;
  for (const auto& em : P.emits) {
    const size_t base = E.size();
    E.resize(base + (size_t)(em.M + 2) * 16, 0.0);
    for (int y = 0; y < P.N; y++) {
      for (int m = 0; m < em.M; m++) E[base + (size_t)m * 16 + y] = em.E[(size_t)m * 64 + y];
      E[base + (size_t)em.M * 16 + y] = em.s[y];
    }
  }
  return upload(d, &d->etab_all, E);
}

// The 16-state route's kernels (EstepKernel, engine_route.cpp chain_estep_kernel):
// the name for a launch failure, the launcher, the scratch of a launch and the
// sequences per slab row -- the matrix-core and checkpoint kernels' 16-sequence
// blocks, chain_estep16_kernel's blocks, the round-2 DPP kernel's sequences.
int seqs_per_row_1(int, int, int) { return 1; }
int seqs_per_row_16(int, int, int) { return 16; }
const struct {
  const char* name;
  int (*launch)(const nipamd::ChainArgs&, hipStream_t);
  size_t (*scratch_bytes)(long B, int T);
  int (*seqs_per_row)(int M, int T, int ne);
} kEstepKernels[] = {
    /* kEstepNone */ {"", nullptr, nullptr, nullptr},
    /* kEstepMfma */ {"chain_fb_mfma_kernel (e_step)", nipamd::chain_estep_mfma_launch, nipamd::chain_scratch_bytes,
                      seqs_per_row_16},
    /* kEstepDpp8 */ {"chain_kernel<true>", nipamd::chain_estep_launch, nipamd::chain_scratch_bytes, seqs_per_row_1},
    /* kEstep16 */ {"chain_estep16_kernel", nipamd::chain_estep16_launch, nipamd::chain_estep16_scratch_bytes,
                    nipamd::chain_estep16_seqs_per_row},
    /* kEstepCk */ {"chain_estep_ck_kernel", nipamd::chain_estep_ck_launch, nipamd::chain_estep_ck_scratch_bytes,
                    seqs_per_row_16},
};

// The 16-state chain e_step (an HMM, a joint interface's HMM, or the general
// plan with several leaf children): one slab (chain_estep_slab) per row.
int estep_chain_partial(nipamd_model* mm, const Route& r, const int32_t* d_obs, int n_obs, int B, int T,
                        double* d_partial, double* d_ll, uint32_t* d_status, hipStream_t st) {
  const auto& P = mm->m.chain;
  const bool general = estep_general_plan(P);
  const int col = r.pcol;
  const int ne = general ? (int)P.emits.size() : 1;            // chain_estep16_kernel's children
  const int Mo = general ? estep_rows(P) - 2 : P.emits[0].M;   // the slab's count-table rows - 2
  const int S = nipamd::chain_estep_slab(Mo);
  const EstepKernel ek = chain_estep_kernel(mm, T);
  const auto& K = kEstepKernels[ek];
  const long chunk = std::min<long>(B, ek == kEstepCk ? kEstepCkChunk : kEstepChunk);
  const SlabRun run{S, chunk, K.seqs_per_row(Mo, T, ne), K.scratch_bytes(chunk, T), {1.0, 0.0, 0.0}};
  ReqTables* rt = nullptr;
  auto prepare = [&] {
    if (int rc = ensure_tables(mm)) return rc;
    Route rh;
    rh.primary = 0;
    if (int rc = ensure_req_tables(mm, rh, &rt)) return rc;
    return general ? ensure_etab_all(mm) : 0;
  };
  return run_slab_chunks(mm, run, B, d_partial, st, prepare, [&](long b0, long nb, double* slab) {
    const DevState* d = dev_of(mm);
    nipamd::ChainArgs a{};
    set_obs_view(a, d_obs, n_obs, T, b0);
    if (!(general ? r.ncol > 0 : col >= 0)) a.obs = nullptr;
    a.obs_col = col;
    a.B = nb; a.T = T; a.H = T / 2; a.N = P.N; a.M = Mo;
    if (const char* hp = nipamd::diag_env("NIPAMD_ESTEP_H"))    // split point in % of T (A/B builds)
      if (ek == kEstep16) a.H = std::min(T - 1, std::max(0, (int)((long)T * std::atoi(hp) / 100)));
    a.A = d->A; a.Etab = general ? d->etab_all : rt->Etab16; a.pi = d->pi; a.ts = rt->ts16; a.S = d->S;
    // the HMM's one child (the primary table), or every leaf child
    a.ne = ne;
    for_each_child(P, r, ne, [&](int k, int row, int slot) {
      a.eM[k] = P.emits[k].M;
      a.erow[k] = row;
      a.ecol[k] = slot >= 0 ? r.col[slot] : -1;
    });
    a.ll = d_ll ? d_ll + b0 : nullptr;
    a.status = d_status ? d_status + b0 : nullptr;
    a.counts = slab;
    a.proper = ek == kEstepCk ? (chain_proper(P) ? 1 : 0)
                              : ek == kEstep16 && chain_proper(P) ? (estep16_sparse_ok(P, ne) ? 2 : 1) : 0;
    // below the step-shrink bound chain_estep16_kernel's backward rows rescale at every step too
    if (ek == kEstep16 && a.proper != 2 && !step_shrink_ok(step_shrink(P, r))) a.proper |= 4;
#ifdef NIPAMD_DIAGNOSTICS
    StampBuf stamps;                                   // the first launch's
    if (int rc = stamps.attach(phase_times() && b0 == 0, estep_stamp_words(ek, nb), st, &a.diag)) return rc;
#endif
    if (int rc = launched(K.launch(a, st), K.name)) return rc;
#ifdef NIPAMD_DIAGNOSTICS
    if (int rc = stamps.report(st, report_estep, std::make_pair(ek, nb))) return rc;
#endif
    return 0;
  });
}

int estep_partial_routes(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
                         int B, int T, double* d_partial, long capacity, double* d_ll,
                         uint32_t* d_status, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  Route r;
  if (chain_estep_ok(mm, n_obs, obs_vars, T, r))
    return estep_chain_partial(mm, r, d_obs, n_obs, B, T, d_partial, d_ll, d_status, st);
  if (wide_estep_ok(mm, n_obs, obs_vars, r))
    return estep_wide_partial(mm, r, d_obs, n_obs, B, T, d_partial, d_ll, d_status, st);
  if (mm->engine == NIPAMD_ENGINE_CHAIN)
    return fail(NIPAMD_ERROR_UNSUPPORTED, "chain e_step covers interface chains with evidence on their children");
  if (op_estep_route(mm, n_obs, obs_vars, T, capacity)) {
    // the operator chain (opchain.cpp): body zeros, the tag (-1, -1, -1)
    // that no other route's tag combines with, then its section
    const int body = estep_body_size(mm);
    HIP_OK(hipMemsetAsync(d_partial, 0, (size_t)body * sizeof(double), st));
    if (nipamd::estep_tag_launch(d_partial + body, -1.0, -1.0, -1.0, st))
      return fail(NIPAMD_ERROR_DEVICE, "tag launch failed");
    std::string err;
    if (int rc = nipamd::op_estep_partial(mm, d_obs, n_obs, obs_vars, B, T, d_partial + body + kTagSlots, d_ll,
                                          d_status, stream, err))
      return fail(rc, err);
    return 0;
  }
  std::string why;
  if (!nipamd::jt_supported(mm, n_obs, obs_vars, 0, nullptr, why)) return fail(NIPAMD_ERROR_UNSUPPORTED, why);
  if (int rc = nipamd::jt_estep_partial(mm, d_obs, n_obs, obs_vars, B, T, d_partial, d_ll, d_status, stream))
    return rc;
  // an operator-chain request on a partial too small for its section (the
  // capacity-free nipamd_estep_partial): say so in nipamd_last_kernel
  if (capacity >= 0 && op_estep_route(mm, n_obs, obs_vars, T, -1))
    nipamd::g_last_kernel =
        "jt_filter_kernel + jt_post_kernel (general engine: an operator-chain request on a partial without room "
        "for its section)";
  if (nipamd::estep_tag_launch(d_partial + estep_body_size(mm), 0.0, 1.0, 0.0, st))
    return fail(NIPAMD_ERROR_DEVICE, "tag launch failed");
  return zero_tail(mm, d_partial, nipamd::param_size(mm->m), st);
}

int estep_partial_cap(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
                      int B, int T, double* d_partial, long capacity, double* d_ll,
                      uint32_t* d_status, void* stream) {
  if (!mm || B < 0 || T < 1 || !d_partial || (n_obs > 0 && (!d_obs || !obs_vars)))
    return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  // The reference rejects series whose leading missing run reaches the
  // model's verdict step (BAD_LUCK): without d_status that verdict could not
  // be reported, and the partial would include counts the reference drops.
  if (!d_status && B > 0 && prefix_first_bad(mm, T) >= 0)
    return fail(NIP_ERROR_INVALID_ARGUMENT,
                "d_status is required: this model's e_step rejects series with a long leading missing run");
  if (int rc = estep_partial_routes(mm, d_obs, n_obs, obs_vars, B, T, d_partial, capacity, d_ll, d_status,
                                    stream))
    return rc;
  if (!d_status || B == 0) return 0;
  // the kernels are queued: this host work overlaps them
  const int k = prefix_first_bad(mm, T);
  if (k < 0) return 0;
  unsigned trivial = 0;                          // columns observing a one-state variable
  for (int c = 0; c < n_obs && c < 32; c++)
    if (obs_vars[c] >= 0 && obs_vars[c] < (int)mm->m.vars.size() && mm->m.vars[obs_vars[c]].card == 1)
      trivial |= 1u << c;
  if (nipamd::estep_prefix_flag_launch(d_obs, n_obs, B, T, k, trivial, d_status, (hipStream_t)stream))
    return fail(NIPAMD_ERROR_DEVICE, "prefix flag launch failed");
  return 0;
}

// the slab -> em_learn map (CSR) on the device
int upload_csr(DevState* d, const std::vector<int>& ptr, const std::vector<int>& idx,
               const std::vector<double>& coef, int n) {
  HIP_OK(hipMalloc(&d->jm_ptr, ptr.size() * sizeof(int)));
  HIP_OK(hipMemcpy(d->jm_ptr, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d->jm_idx, std::max<size_t>(1, idx.size()) * sizeof(int)));
  if (!idx.empty()) HIP_OK(hipMemcpy(d->jm_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
  if (int rc = upload(d, &d->jm_coef, coef)) return rc;
  d->jm_n = n;
  return 0;
}

// A joint interface's e_step counts (the HMM e_step kernel's slab over the
// joint states: xi sums Kf / Kb without the A factor, M1 tables of the
// observation, the t = 0 posterior P0) projected onto every family of the
// em_learn layout (child first, then its parents, nip.c:2101-2128): the
// family's value at a joint (x, y) is its variables' digits, previous-slice
// variables from x and interface variables from y.  Built on the host once
// per model version; each count is one fixed-order sum (CSR row).
int ensure_joint_map(nipamd_model* mm) {
  DevState* d = dev_of(mm);
  if (d->jm_ptr) return 0;
  const nipamd::Model& m = mm->m;
  const auto& P = m.chain;
  const int nv = (int)m.vars.size(), K = P.N, M = P.emits[0].M, ov = P.emits[0].var;
  const int Kb = nipamd::kSlabKb, Hf = nipamd::kSlabH, Hb = nipamd::kSlabH + (M + 2) * 16;
  const int p0 = nipamd::chain_slab_p0(M);
  std::vector<int> off(nv + 1, 0);
  for (int v = 0; v < nv; v++) {
    int sz = m.vars[v].card;
    for (int q : m.vars[v].parents) sz *= m.vars[q].card;
    off[v + 1] = off[v] + sz;
  }
  // value of variable w at joint (x, y): -1 if it is neither interface's
  auto value = [&](int w, int x, int y) {
    long sx = 1;
    for (size_t i = 0; i < P.jprev.size(); i++) {
      const int c = m.vars[P.jprev[i]].card;
      if (P.jprev[i] == w) return (int)((x / sx) % c);
      if (P.jcur[i] == w) return (int)((y / sx) % c);
      sx *= c;
    }
    return -1;
  };
  std::vector<std::vector<std::pair<int, double>>> rows(off[nv]);
  for (int v = 0; v < nv; v++) {
    const auto& V = m.vars[v];
    std::vector<int> U{v};
    U.insert(U.end(), V.parents.begin(), V.parents.end());
    auto family_index = [&](int x, int y, int first) {     // first: v's own value (child first)
      long idx = first, st = V.card;
      for (size_t k = 1; k < U.size(); k++) {
        const int u = value(U[k], x, y);
        if (u < 0) return -1L;
        idx += u * st;
        st *= m.vars[U[k]].card;
      }
      return idx;
    };
    const bool is_prev = std::find(P.jprev.begin(), P.jprev.end(), v) != P.jprev.end();
    const bool is_cur = std::find(P.jcur.begin(), P.jcur.end(), v) != P.jcur.end();
    if (is_prev) {
      if (U.size() != 1) return fail(NIPAMD_ERROR_UNSUPPORTED, "joint e_step: previous-slice variable with parents");
      for (int x = 0; x < K; x++) rows[off[v] + value(v, x, 0)].push_back({p0 + x, 1.0});
    } else if (is_cur) {
      for (int x = 0; x < K; x++)
        for (int y = 0; y < K; y++) {
          const long i = family_index(x, y, value(v, x, y));
          if (i < 0) return fail(NIPAMD_ERROR_UNSUPPORTED, "joint e_step: family outside the interfaces");
          const double a = P.A[x * 16 + y];
          rows[off[v] + i].push_back({x * 16 + y, a});
          rows[off[v] + i].push_back({Kb + x * 16 + y, a});
        }
    } else if (v == ov) {
      const auto& E = P.emits[0];
      for (int y = 0; y < K; y++)
        for (int o = 0; o < M; o++) {
          const long i = family_index(0, y, o);
          if (i < 0) return fail(NIPAMD_ERROR_UNSUPPORTED, "joint e_step: observation family outside the interface");
          rows[off[v] + i].push_back({Hf + o * 16 + y, 1.0});
          rows[off[v] + i].push_back({Hb + o * 16 + y, 1.0});
          if (E.s[y] != 0.0) {                   // missing observations, split as E(y, o) / s(y)
            const double w = E.E[(size_t)o * 64 + y] / E.s[y];
            rows[off[v] + i].push_back({Hf + M * 16 + y, w});
            rows[off[v] + i].push_back({Hb + M * 16 + y, w});
          }
        }
    } else {
      return fail(NIPAMD_ERROR_UNSUPPORTED, "joint e_step: variable outside the joint chain");
    }
  }
  std::vector<int> ptr{0}, idx;
  std::vector<double> coef;
  for (const auto& r : rows) {
    for (const auto& e : r) { idx.push_back(e.first); coef.push_back(e.second); }
    ptr.push_back((int)idx.size());
  }
  return upload_csr(d, ptr, idx, coef, off[nv]);
}

// the cached slab -> em_learn map serves one slab layout: drop it when a
// partial of another layout comes to be finalized
int ensure_map_kind(nipamd_model* mm, int kind) {
  DevState* d = dev_of(mm);
  if (d->jm_ptr && d->jm_kind != kind) {
    HIP_OK(hipDeviceSynchronize());
    dfree(d, d->jm_ptr); dfree(d, d->jm_idx); dfree(d, d->jm_coef);
    d->jm_ptr = nullptr; d->jm_idx = nullptr; d->jm_coef = nullptr; d->jm_n = 0;
  }
  d->jm_kind = kind;
  return 0;
}

struct SlabLayout {
  int ns;          // row stride of K and H
  int kf, kb;      // K sums (kb < 0: one sum)
  int hf, hb;      // count tables (hb < 0: one table)
  int p0;
};

// The general chain e_step's slab (xi sums without the transition, the
// children's count tables, the t = 0 posterior P0) projected onto every
// family of the em_learn layout (nip.c:2101-2128: child first, then its
// parents in v->parents order), as one fixed-order sum per count (CSR):
//   previous interface variable: P0
//   interface variable y | x, hidden parents h: in-clique(x, y, h)
//       x prod_j prior_j(h_j) x K(x, y)   (the joint posterior of the
//       in-clique's variables is alpha_{t-1}(x) P(y | x, h) prod prior(h)
//       e_t(y) beta_t(y) / Z; the xi sums K hold everything but the first factors)
//   hidden parent h_j: the same summed over everything but h_j
//   leaf child o_k | y: its count table, a missing observation split as
//       E_k(y, o) / s_k(y) (the child's posterior given y)
// Two slab layouts: the 16-state kernels' (Kf and Kb, two count tables, row
// stride 16) and estep_wide.hip's (one K, one table, row stride NP).  Built
// as (row, slab index, coefficient) triples in a fixed generation order, then
// grouped by row with a stable counting sort: the in-clique of config 5 has
// 16.7M entries, one CSR row each.
int ensure_chain_map(nipamd_model* mm, const SlabLayout& L) {
  DevState* d = dev_of(mm);
  if (d->jm_ptr) return 0;
  const nipamd::Model& m = mm->m;
  if (!chain_map_supported(m)) return fail(NIPAMD_ERROR_UNSUPPORTED, "chain e_step: slice outside the chain plan");
  const auto& P = m.chain;
  const int nv = (int)m.vars.size(), N = P.N;
  std::vector<long> off(nv + 1, 0);
  for (int v = 0; v < nv; v++) {
    long sz = m.vars[v].card;
    for (int q : m.vars[v].parents) sz *= m.vars[q].card;
    off[v + 1] = off[v] + sz;
  }
  struct Ent { long row; int idx; double coef; };
  std::vector<Ent> ents;
  auto kidx = [&](int base, int x, int y) { return base + x * L.ns + y; };
  // the in-clique's entries: (x, y, hidden values) -> coefficient
  const auto& cin = m.cliques[P.c_trans];
  const size_t nc = cin.vars.size();
  long total = 1;
  for (size_t i = 0; i < nc; i++) total *= m.vars[cin.vars[i]].card;
  ents.reserve((size_t)total * (L.kb >= 0 ? 2 : 1) + 4096);
  const int nh = (int)P.hidden.size();
  // hidden parent j, value d: sum over the in-clique entries of each (x, y),
  // in entry order, and the order in which the (x, y) first occur
  std::vector<std::vector<double>> hacc(nh);
  std::vector<std::vector<char>> hseen(nh);
  std::vector<std::vector<std::vector<int>>> horder(nh);
  for (int j = 0; j < nh; j++) {
    const int c = m.vars[P.hidden[j]].card;
    hacc[j].assign((size_t)c * N * N, 0.0);
    hseen[j].assign((size_t)c * N * N, 0);
    horder[j].resize(c);
  }
  std::vector<int> val(nv, 0);
  const auto& Vc = m.vars[P.v_cur];
  std::vector<int> cardc(nc);
  for (size_t k = 0; k < nc; k++) cardc[k] = m.vars[cin.vars[k]].card;
  std::vector<int> digit(nc, 0);
  for (long i = 0; i < total; i++) {
    for (size_t k = 0; k < nc; k++) val[cin.vars[k]] = digit[k];
    double coef = cin.original[(size_t)i];
    for (int h : P.hidden) coef *= m.vars[h].prior[val[h]];
    const int x = val[P.v_prev], y = val[P.v_cur];
    // the interface variable's family: y first, then its parents in order
    long idx = y, st = Vc.card;
    for (int q : Vc.parents) { idx += (long)val[q] * st; st *= m.vars[q].card; }
    ents.push_back({off[P.v_cur] + idx, kidx(L.kf, x, y), coef});
    if (L.kb >= 0) ents.push_back({off[P.v_cur] + idx, kidx(L.kb, x, y), coef});
    for (int j = 0; j < nh; j++) {
      const int dv = val[P.hidden[j]];
      const size_t c = ((size_t)dv * N + x) * N + y;
      if (!hseen[j][c]) { hseen[j][c] = 1; horder[j][dv].push_back(x * N + y); }
      hacc[j][c] += coef;
    }
    for (size_t k = 0; k < nc; k++) {                     // odometer, dimension 0 fastest
      if (++digit[k] < cardc[k]) break;
      digit[k] = 0;
    }
  }
  for (int j = 0; j < nh; j++) {
    const int h = P.hidden[j];
    for (int dv = 0; dv < m.vars[h].card; dv++) {
      for (int xy : horder[j][dv])
        ents.push_back({off[h] + dv, kidx(L.kf, xy / N, xy % N), hacc[j][((size_t)dv * N) * N + xy]});
      if (L.kb >= 0)
        for (int xy : horder[j][dv])
          ents.push_back({off[h] + dv, kidx(L.kb, xy / N, xy % N), hacc[j][((size_t)dv * N) * N + xy]});
    }
  }
  for (int x = 0; x < N; x++) ents.push_back({off[P.v_prev] + x, L.p0 + x, 1.0});
  for (size_t k = 0, row0 = 0; k < P.emits.size(); k++) {
    const auto& E = P.emits[k];
    for (int y = 0; y < N; y++)
      for (int o = 0; o < E.M; o++) {
        const long r = off[E.var] + o + (long)E.M * y;
        ents.push_back({r, L.hf + (int)(row0 + o) * L.ns + y, 1.0});
        if (L.hb >= 0) ents.push_back({r, L.hb + (int)(row0 + o) * L.ns + y, 1.0});
        if (E.s[y] != 0.0) {                   // missing observations, split as E(y, o) / s(y)
          const double w = E.E[(size_t)o * 64 + y] / E.s[y];
          ents.push_back({r, L.hf + (int)(row0 + E.M) * L.ns + y, w});
          if (L.hb >= 0) ents.push_back({r, L.hb + (int)(row0 + E.M) * L.ns + y, w});
        }
      }
    row0 += E.M + 2;
  }
  // CSR by a stable counting sort on the row
  const long nrows = off[nv];
  if ((long)ents.size() >= (1L << 31) || nrows >= (1L << 31))
    return fail(NIPAMD_ERROR_UNSUPPORTED, "chain e_step: projection beyond 2^31 entries");
  std::vector<int> ptr((size_t)nrows + 1, 0);
  for (const Ent& e : ents) ptr[(size_t)e.row + 1]++;
  for (long r = 0; r < nrows; r++) ptr[(size_t)r + 1] += ptr[(size_t)r];
  std::vector<int> fill(ptr.begin(), ptr.end() - 1), idx(ents.size());
  std::vector<double> coef(ents.size());
  for (const Ent& e : ents) {
    const int q = fill[(size_t)e.row]++;
    idx[(size_t)q] = e.idx;
    coef[(size_t)q] = e.coef;
  }
  return upload_csr(d, ptr, idx, coef, (int)nrows);
}

int map_finalize(const DevState* d, const double* d_partial, double* d_counts, void* stream) {
  if (nipamd::estep_map_finalize_launch(d_partial, d->jm_n, d->jm_ptr, d->jm_idx, d->jm_coef, d_counts,
                                        (hipStream_t)stream))
    return fail(NIPAMD_ERROR_DEVICE, "finalize launch failed");
  return 0;
}

}  // namespace

// ---- what engine_estep_soft.cpp takes of the above (engine_internal.h)
namespace nipamd::eng {

int wide_slab_chunks(nipamd_model* mm, int S, long chunk, size_t scratch, long B, double* d_partial, hipStream_t st,
                     const std::function<int()>& prepare,
                     const std::function<int(long, long, double*)>& launch) {
  const SlabRun run{S, chunk, 1, scratch, {0.0, 0.0, 1.0}};
  return run_slab_chunks(mm, run, B, d_partial, st, prepare, launch);
}

long estep_pow2_chunk(size_t per_seq, size_t budget, long lo, long hi) { return pow2_chunk(per_seq, budget, lo, hi); }

long estep_chunk_limit() { return kEstepChunk; }

}  // namespace nipamd::eng

extern "C" {

int nipamd_estep_partial_size(const nipamd_model* mm) {
  if (!mm) return -1;
  if (mm->engine == NIPAMD_ENGINE_CHAIN && !has_chain_estep(mm->m)) return -1;
  return estep_body_size(mm) + kTagSlots;
}

int nipamd_estep_partial_size_req(nipamd_model* mm, int n_obs, const int* obs_vars, int T) {
  if (!mm || T < 1 || (n_obs > 0 && !obs_vars)) return -1;
  const int base = nipamd_estep_partial_size(mm);
  if (base < 0 || !op_estep_route(mm, n_obs, obs_vars, T, -1)) return base;
  return base + (int)nipamd::op_estep_section(mm, n_obs, obs_vars);
}

int nipamd_estep_partial(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
                         int B, int T, double* d_partial, double* d_ll, uint32_t* d_status,
                         void* stream) {
  if (!mm) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  const int base = nipamd_estep_partial_size(mm);
  return estep_partial_cap(mm, d_obs, n_obs, obs_vars, B, T, d_partial, base > 0 ? base : 0, d_ll, d_status,
                           stream);
}

int nipamd_estep_partial_ex(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
                            int B, int T, double* d_partial, long capacity, double* d_ll,
                            uint32_t* d_status, void* stream) {
  if (!mm) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  const int base = nipamd_estep_partial_size(mm);
  if (base >= 0 && capacity < base)
    return fail(NIP_ERROR_INVALID_ARGUMENT, "partial capacity below nipamd_estep_partial_size");
  return estep_partial_cap(mm, d_obs, n_obs, obs_vars, B, T, d_partial, capacity, d_ll, d_status, stream);
}

int nipamd_tree_sum(const double* d_rows, long n, int S, double* d_work, double* d_out, void* stream) {
  if (n < 0 || S < 1 || !d_out || (n > 0 && !d_rows) || (n > 64 && !d_work))
    return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  if (n == 0) {
    HIP_OK(hipMemsetAsync(d_out, 0, (size_t)S * sizeof(double), (hipStream_t)stream));
    return 0;
  }
  double* tA = d_work;
  double* tB = d_work ? d_work + (size_t)((n + 63) / 64) * S : nullptr;
  if (reduce_rows(d_rows, n, S, tA, tB, d_out, (hipStream_t)stream))
    return fail(NIPAMD_ERROR_DEVICE, "tree launch failed");
  return 0;
}

int nipamd_estep_tail(const double* d_ll, const uint32_t* d_status, long B, double* d_work, double* d_out2,
                      void* stream) {
  if (B < 0 || !d_out2 || (B > 0 && (!d_ll || !d_status || !d_work)))
    return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  if (int rc = nipamd_tree_sum(d_ll, B, 1, d_work, d_out2, stream)) return rc;
  if (B == 0) {
    HIP_OK(hipMemsetAsync(d_out2 + 1, 0, sizeof(double), (hipStream_t)stream));
    return 0;
  }
  // the count's block parts after the tree's levels in the workspace
  double* cw = d_work + (B > 64 ? 2 * ((B + 63) / 64) : 0);
  if (nipamd::count_failed_launch(d_status, B, cw, d_out2 + 1, (hipStream_t)stream))
    return fail(NIPAMD_ERROR_DEVICE, "count launch failed");
  return 0;
}

int nipamd_estep_prefix_first_bad(nipamd_model* mm, int T) {
  if (!mm || T < 1) { fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments"); return -2; }
  if (nipamd::estep_prefix_entries(mm->m) > kPrefixMaxEntries) return -2;
  const int k = prefix_first_bad(mm, T);
  // -2: the simulation's work bound ran out (not simulated), not "no step"
  return k < 0 && mm->pf_first_bad == -2 ? -2 : k;
}

int nipamd_estep_finalize(nipamd_model* mm, const double* d_partial, double* d_counts, void* stream) {
  if (!mm || !d_partial || !d_counts) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  const int body = estep_body_size(mm);
  // the route tag (see nipamd_estep_partial_size): one 24-byte read, once per EM iteration
  double tag[kTagSlots] = {0.0, 0.0, 0.0};
  HIP_OK(hipMemcpyAsync(tag, d_partial + body, sizeof(tag), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  int route = -1, nz = 0;
  for (int k = 0; k < kTagSlots; k++)
    if (tag[k] != 0.0) { nz++; if (tag[k] >= 1.0) route = k; }
  if (tag[0] <= -1.0 && tag[1] == tag[0] && tag[2] == tag[0]) {
    // the operator chain's partial (its header names the request)
    std::string err;
    if (int rc = nipamd::op_estep_finalize(mm, d_partial + body + kTagSlots, d_counts, stream, err))
      return fail(rc, err);
    return 0;
  }
  if (nz != 1 || route < 0)
    return fail(NIP_ERROR_INVALID_ARGUMENT, "e_step partial: partials of different routes (chain slab / em_learn "
                                            "layout / wide chain slab) were combined, or the buffer is not an "
                                            "e_step partial");
  if (route == 1) return nipamd::jt_estep_finalize(mm, d_partial, d_counts, stream);
  const auto& P = mm->m.chain;
  if (!has_chain_estep(mm->m)) return fail(NIPAMD_ERROR_UNSUPPORTED, "no chain e_step plan for this model");
  if (int rc = ensure_tables(mm)) return rc;
  DevState* d = dev_of(mm);
  if (route == 2) {
    if (!estep_wide_plan(mm->m)) return fail(NIPAMD_ERROR_UNSUPPORTED, "no wide chain e_step plan for this model");
    const int NP = nipamd::estep_wide_np(P.N), R = estep_rows(P);
    const SlabLayout L{NP, 0, -1, NP * NP, -1, NP * NP + R * NP};
    if (int rc = ensure_map_kind(mm, 3)) return rc;
    if (int rc = ensure_chain_map(mm, L)) return rc;
    return map_finalize(d, d_partial, d_counts, stream);
  }
  Route rh;
  rh.primary = 0;
  ReqTables* rt = nullptr;
  if (int rc = ensure_req_tables(mm, rh, &rt)) return rc;
  if (P.jhmm || !P.hmm) {
    const int R = estep_rows(P);
    const SlabLayout L{16, nipamd::kSlabKf, nipamd::kSlabKb, nipamd::kSlabH, nipamd::kSlabH + R * 16,
                       nipamd::chain_slab_p0(R - 2)};
    if (int rc = ensure_map_kind(mm, P.jhmm ? 1 : 2)) return rc;
    if (int rc = P.jhmm ? ensure_joint_map(mm) : ensure_chain_map(mm, L)) return rc;
    return map_finalize(d, d_partial, d_counts, stream);
  }
  nipamd::ChainFinalize f{};
  f.N = P.N; f.M = P.emits[0].M;
  int off = 0;
  for (size_t v = 0; v < mm->m.vars.size(); v++) {
    if ((int)v == P.v_prev) f.off_prev = off;
    if ((int)v == P.v_cur) f.off_cur = off;
    if ((int)v == P.emits[0].var) f.off_obs = off;
    int s = mm->m.vars[v].card;
    for (int p : mm->m.vars[v].parents) s *= mm->m.vars[p].card;
    off += s;
  }
  f.A = d->A; f.Etab = rt->Etab16;
  if (nipamd::estep_finalize_launch(d_partial, f, d_counts, (hipStream_t)stream))
    return fail(NIPAMD_ERROR_DEVICE, "finalize launch failed");
  return 0;
}

int nipamd_estep(nipamd_model* mm, const int32_t* d_obs, int n_obs, const int* obs_vars,
                 int B, int T, double* d_counts, double* d_ll, uint32_t* d_status, void* stream) {
  if (!mm || !d_counts || T < 1) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  const int S = nipamd_estep_partial_size_req(mm, n_obs, obs_vars, T);
  if (S < 0) return fail(NIPAMD_ERROR_UNSUPPORTED, "no e_step plan for this model under the selected engine");
  if (int rc = ensure_device(mm)) return rc;
  DevState* d = dev_of(mm);
  if (d->R_size < S) {
    (void)hipFree(d->R);
    d->R = nullptr;
    d->R_size = 0;
    HIP_OK(hipMalloc(&d->R, (size_t)S * sizeof(double)));
    d->R_size = S;
  }
  double* part = d->R;
  int rc = nipamd_estep_partial_ex(mm, d_obs, n_obs, obs_vars, B, T, part, S, d_ll, d_status, stream);
  if (rc) return rc;
  return nipamd_estep_finalize(mm, part, d_counts, stream);
}

int nipamd_estep_host(nipamd_model* mm, const int32_t* obs, int n_obs, const int* obs_vars,
                      int B, int T, double* counts, double* ll, uint32_t* status) {
  if (!mm || B < 0 || T < 1 || !counts) return fail(NIP_ERROR_INVALID_ARGUMENT, "bad arguments");
  const int P = nipamd::param_size(mm->m);
  const size_t nob = (size_t)B * T * (n_obs > 0 ? n_obs : 1);
  return host_call(n_obs > 0 ? obs : nullptr, nob, counts, (size_t)P, true, ll, status, (size_t)B,
                   [&](int32_t* d_obs, double* d_cnt, double* d_ll, uint32_t* d_st) {
                     return nipamd_estep(mm, d_obs, n_obs, obs_vars, B, T, d_cnt, d_ll, d_st, nullptr);
                   });
}

}  // extern "C"
