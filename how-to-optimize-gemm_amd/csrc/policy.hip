// policy.hip -- sgemm_on(): argument checks, the empty contraction, and MMH_KERNEL_AUTO's tile choice (the
// reference's `NEW := MMult_xxx` makefile switch, cuda/makefile:1-3, as a run-time decision); call_on(): the same for
// mmh_sgemm_op / _ex / _batched / _batched_ex, one front end on the GemmArgs / BatchArgs the entry points pack (abi.hip); the plan
// entry points (plan_batched: both batched ones).  Pure host code; the kernels are launched by the launch_*.hip units.
#include <algorithm>

#include "internal.hpp"
#include "launch_common.hpp"   // streamk_wanted

namespace mmh {

namespace {
constexpr int kSliceK = 32;   // K-slice depth of the MFMA tiles (sgemm_tile.hpp BK)

// MMH_KERNEL_AUTO: a COST TABLE, not thresholds (round 4; rounds 1-3 had hand-set rules fitted to one chip's sweep).
// Every candidate -- a tile family as a plain launch or as a persistent stream-K launch -- is priced in microseconds
// from what the shape makes of it, per CU:
//     plain:     t = fix_p + cmax * nk * s_p[min(cmax, w)]      cmax = ceil(tiles / CUs): the tiles of the fullest CU
//     stream-K:  t = fix_s[w'] + (tiles * nk / CUs) * s_s[w']   w'   = persistent workgroups per CU
// nk = ceil(k / 32) K-slices per tile, w the family's co-residency; s_x[o] is what a CU takes per tile-slice with o
// tiles co-resident, fix_x everything that does not scale with K (launch, pipeline fill, C store, hand-over).  The
// numbers are FITTED (tools/policy_fit.py, least squares in relative error) to a measured set of shapes x candidates
// (tools/policy_shapes.py, tools/tile_sweep.py) and live in policy_table.inc; a plain launch of more than one round
// of workgroups with a ragged last round is priced at the fit's own 90th-percentile residual (MMH_POLICY_MULTIROUND_MARGIN).  Everything is
// per CU, so the table serves any CU count.  profiles/r04_auto_regret.md: regret against the best measured candidate
// on 500 held-out shapes.  tools/calibrate_policy.sh regenerates the table on another box.
struct Family {
  int kernel, bm, bn, w, has_sk;
  int skw;   // persistent workgroups per CU of the family's stream-K launches (<= w: the guarded chained kernel's registers)
  float fix_p, s_p[3], fix_s[3], s_s[3];
  float fix_p_whole, fix_s_whole[3];   // the fixed costs of the whole-tile instantiation (no guards: fast_shape)
  float tile_p[3], tile_s[3];          // per tile (on the fullest CU / per CU's share), by occupancy: pipeline fill, C store
};
#include "policy_table.inc"
const Family kFamilies[] = {MMH_POLICY_FAMILIES};

struct Plan {
  int kernel = -1;
  int form = 0;   // 1 plain, 2 persistent stream-K (GemmArgs::form)
  double us = 0.0;
  int sk_w = 0;   // form 2: the persistent workgroups per CU the price was taken for (GemmArgs::sk_w)
  int bm = 0, bn = 0;
};

bool is_k2w(int kernel) { return is_family(kernel, Launcher::K2W); }
// the tiles with op forms (launch_op.hip): where the NN table picks one of them the op plan is that very plan
bool has_op_forms(int kernel) { return k2w_tiles::with(kernel, [](auto t) { return (int)t.OPS; }, 0); }

// The price of a plain launch (one workgroup per tile) of `tiles` workgroups of the family, `full` of them not thin.
// The thin edge tiles cost MMH_POLICY_THIN of a round where they add a tile to the fullest CU (N = 1025 against 1024 on
// the 64x64 tile: 26.3 against 18.1 us; tools/policy_fit.py THIN).
double plain_us(const mmh_context *ctx, const Family &f, int k, long tiles, long full, bool whole) {
  const long cus = ctx && ctx->cu_count > 0 ? ctx->cu_count : 256;
  const double nk = (double)((k + kSliceK - 1) / kSliceK);
  const long cmax = (tiles + cus - 1) / cus;
  const int occ = (int)std::min<long>(cmax, f.w);
  double cmax_p = (double)cmax;
  if (full < tiles) {
    const long cfull = (full + cus - 1) / cus;
    cmax_p = (double)cfull + MMH_POLICY_THIN * (double)(cmax - cfull);
  }
  double t = (whole ? f.fix_p_whole : f.fix_p) + cmax_p * (nk * f.s_p[occ - 1] + f.tile_p[occ - 1]);
  if (cmax > f.w && tiles % ((long)f.w * cus) != 0) {   // a ragged last round
    // ... of between half a tile and one tile per CU: the dispatcher hands those out one per CU, or in pairs to the
    // CUs whose workgroups ended together -- a whole extra round (the same launch 142 and 110 TFLOP/s in two passes:
    // tools/policy_fit.py PAIRING); priced at the risk
    // (the launches launch_dma5.hpp splits -- one round and a last round of just under a tile per CU -- are out of that class)
    const long rem = tiles % ((long)f.w * cus);
    const bool split = is_k2w(f.kernel) && (!ctx || ctx->split_tail) && dma5_tail_split(tiles, f.w, cus, k);
    t *= (2 * rem > cus && rem <= cus && !split) ? std::max(MMH_POLICY_PAIRING_MARGIN, MMH_POLICY_MULTIROUND_MARGIN) : MMH_POLICY_MULTIROUND_MARGIN;
  }
  return t;
}

Plan auto_plan_for(const mmh_context *ctx, const GemmArgs &g) {
  const long cus = ctx && ctx->cu_count > 0 ? ctx->cu_count : 256;
  const double nk = (double)((g.k + kSliceK - 1) / kSliceK);
  Plan best;
  long tiles_rim = 0;
  bool any_dma5 = false;   // did any LDS-DMA family take the shape?
  for (const Family &f : kFamilies) {
    if ((g.ta || g.tb || g.ex) && !has_op_forms(f.kernel)) continue;   // op forms, and every epilogue call: the same table, restricted to their three tiles
    // (Rounds 2-3 kept K > 8192 -- B beyond the Infinity Cache, the config-4 panels -- on the 256x256 tile: K2L's small tiles
    // lost 1-6 % there.  K2W's do not: 2048 .. 4096 x 16384 x 16384 run 152.4-153.2 TFLOP/s on the 128x64 tile against
    // 150.2-150.3, and 2048 x 4096 x 16384 -- half a round of 256x256 tiles -- 151.5 against 74.8: the fence is gone, the
    // table decides; profiles/r04_big_k.md.)
    if (f.kernel != MMH_KERNEL_MFMA_256X256) {
      // (round 5: the K2L tiles are candidates too -- VERDICT r04 item 4: they shipped, AUTO never priced them, and on
      // small shapes their 256-thread workgroups and shorter preamble won by 5-8 %)
      if (is_k2w(f.kernel) ? !dma5_shape_ok(ctx, f.kernel, g) : !dma_shape_ok(ctx, f.kernel, g)) continue;
      any_dma5 = true;
    }
    long tiles = (long)((g.m + f.bm - 1) / f.bm) * ((g.n + f.bn - 1) / f.bn);
    {   // the 64x64 tile's RIM launch: one or two rows / columns past a 64-boundary cost no tiles of their own (plain only)
      int r_m = 0, r_n = 0;
      if (f.kernel == MMH_KERNEL_MFMA_64X64_DMA5 && ctx && ctx->rim5 && dma5_rim_dims(g.m, g.n, &r_m, &r_n))
        tiles_rim = (long)((g.m - r_m + 63) / 64) * ((g.n - r_n + 63) / 64);
      else
        tiles_rim = 0;
    }
    if (tiles_rim) tiles = tiles_rim;
    const bool whole = fast_shape(f.bm, f.bn, kSliceK, g);
    const double t = plain_us(ctx, f, g.k, tiles, is_k2w(f.kernel) && !tiles_rim ? full_tiles(g.m, g.n, f.bm, f.bn) : tiles, whole);
    if (best.kernel < 0 || t < best.us) best = Plan{f.kernel, 1, t, 0, f.bm, f.bn};
    if (f.has_sk && (!ctx || ctx->streamk) && !tiles_rim) {
      // the grid launch_streamk will launch: the largest w' <= skw workgroups per CU that leaves every one a whole tile
      // (round 4 took w' from the plain co-residency w and priced 768-tile launches that ran on 512)
      int wp = 0;
      for (int c = f.skw; c >= 1; --c)
        if (tiles >= (long)c * cus) { wp = c; break; }
      if (wp > 0 && tiles % ((long)wp * cus) != 0 && tiles <= (1L << 24)) {
        double ts = (whole ? f.fix_s_whole[wp - 1] : f.fix_s[wp - 1]) +
                    (double)tiles / (double)cus * (nk * f.s_s[wp - 1] + f.tile_s[wp - 1]);
        // the K2W 64x64 tile under stream-K: the one candidate whose rate moves 2-5 % from run to run (tools/policy_fit.py
        // T64SK): priced at the risk
        if (f.kernel == MMH_KERNEL_MFMA_64X64_DMA5 && wp >= 2) ts *= MMH_POLICY_T64SK_MARGIN;   // (two per CU: from 512 tiles)
        if (ts < best.us) best = Plan{f.kernel, 2, ts, wp, f.bm, f.bn};
      }
    }
  }
  // No LDS-DMA family takes the shape (operands beyond the 2 GiB descriptor window; MMH_OPT_DMA_EDGE = 0 on a ragged or
  // unaligned shape): the table's one remaining row -- the 256x256 tile, priced without rivals -- is not a choice.
  // fallback_kernel picks among the register-staged tiles by tile count (round 4 launched 16 workgroups of 256x256
  // for 1000^3 here).
  if (!any_dma5) return Plan{};
  return best;
}

// operands the descriptors cannot window (beyond 2 GiB), or the guarded LDS-DMA form switched off: the
// register-staged tiles, by how many tiles the shape has (rounds 1-2)
int fallback_kernel(const mmh_context *ctx, const GemmArgs &g) {
  const long cus = ctx && ctx->cu_count > 0 ? ctx->cu_count : 256;
  if (reg_tile_count(MMH_KERNEL_MFMA_256X256, g.m, g.n) >= cus) return MMH_KERNEL_MFMA_256X256;
  if (reg_tile_count(MMH_KERNEL_MFMA_128X64, g.m, g.n) * 2 <= cus) return MMH_KERNEL_MFMA_64X64;
  if (reg_tile_count(MMH_KERNEL_MFMA, g.m, g.n) * 10 < cus * 8) return MMH_KERNEL_MFMA_128X64;
  return MMH_KERNEL_MFMA;
}

// split-K's "auto" part count: fill two workgroups per CU, keep >= 8 K-slices per part, at most 8 parts
int splitk_auto_parts(long cus, long tiles, int k) {
  const int S = (int)((2 * cus) / (tiles > 0 ? tiles : 1));
  return std::min(std::min(S, k / (8 * kSliceK)), 8);
}

// The launcher of a catalogue row's family.  Split-K (K2s) runs on the row's fall-back tile, ctx->splitk parts (auto when
// <= 1).  MMH_OK, an error, or 1: the shape does not qualify.
int launch_family(mmh_context *ctx, const KernelRow &row, const GemmArgs &g) {
  switch (row.launcher) {
    case Launcher::Valu:
    case Launcher::Naive: return launch_valu(ctx, row.id, g);
    case Launcher::Reg: return launch_reg(ctx, row.id, g);
    case Launcher::K2L: return launch_dma(ctx, row.id, g);
    case Launcher::K2W: return launch_dma5(ctx, row.id, g);
#ifdef MMH_AB_BUILD
    case Launcher::K2M: return launch_dma32(ctx, row.id, g);
#endif
    case Launcher::SplitK: {
      int S = ctx ? ctx->splitk : 0;
      if (S <= 1) S = splitk_auto_parts(ctx && ctx->cu_count > 0 ? ctx->cu_count : 256, reg_tile_count(row.fallback, g.m, g.n), g.k);
      return launch_reg_splitk(ctx, row.fallback, S, g);
    }
    default: break;   // (MMH_KERNEL_AUTO: resolved by the caller)
  }
  set_last_error("unknown kernel variant");
  return MMH_ERR_INVALID_ARG;
}
}  // namespace

int sgemm_on(mmh_context *ctx, int kernel, int m, int n, int k, const float *dA, int lda, const float *dB, int ldb,
             float *dC, int ldc, int accumulate, hipStream_t s) {
  int rc = check_gemm_args(m, n, k, dA, lda, dB, ldb, dC, ldc);
  if (rc != MMH_OK) {
    set_last_error("invalid argument");
    return rc;
  }
  if (m == 0 || n == 0) return MMH_OK;
  if (k == 0) {
    // empty contraction: C = 0 (overwrite) or C unchanged (accumulate)
    if (!accumulate)
      HIP_TRY(hipMemset2DAsync(dC, (size_t)ldc * sizeof(float), 0, (size_t)n * sizeof(float), (size_t)m, s));
    return MMH_OK;
  }
  const GemmArgs g{m, n, k, dA, lda, dB, ldb, dC, ldc, accumulate ? 1 : 0, s};
  const long cus = ctx && ctx->cu_count > 0 ? ctx->cu_count : 256;
  if (kernel == MMH_KERNEL_AUTO) {
    const long tiles128 = reg_tile_count(MMH_KERNEL_MFMA, m, n);
    // OPT-IN split-K (default off: it gives up the one-chain-per-element bits, see sgemm_mfma.hpp K2s):
    // shapes with fewer 128x128 tiles than workgroup slots run their K ranges concurrently
    if (ctx && ctx->splitk > 0 && tiles128 < cus && reg_tile_count(MMH_KERNEL_MFMA_256X256, m, n) < cus) {
      int S = ctx->splitk;
      if (S == 1) S = splitk_auto_parts(cus, tiles128, k);
      if (S >= 2) {
        const int sk = launch_reg_splitk(ctx, MMH_KERNEL_MFMA, S, g);
        if (sk <= 0) return sk;
      }
    }
#ifdef MMH_AB_BUILD
    // MMH_OPT_RIM (tools build; measured, it does not pay -- profiles/r03_notes.md section 6): a few rows / columns past
    // a 64-boundary: the K2L tiles take the trimmed shape, the rim runs on the vector ALU in the same launch
    if (ctx && ctx->rim > 0) {
      const int rm = m % 64, rn = n % 64;
      if ((rm || rn) && rm <= ctx->rim && rn <= ctx->rim && m - rm >= 256 && n - rn >= 256 && k >= 64) {
        GemmArgs t = g;
        t.m = m - rm;
        t.n = n - rn;
        t.rim_m = m;
        t.rim_n = n;
        const long t64 = (long)(t.m / 64) * (t.n / 64);
        const int k0 = t64 <= 3 * cus ? MMH_KERNEL_MFMA_64X64_DMA : MMH_KERNEL_MFMA_128X64_DMA;
        const int d = launch_dma(ctx, k0, t);
        if (d <= 0) return d;
      }
    }
#endif
    const Plan plan = auto_plan_for(ctx, g);
    if (plan.kernel >= 0) {
      GemmArgs ga = g;
      ga.form = plan.form;
      ga.sk_w = plan.sk_w;
      const int d = launch_family(ctx, *kernel_row(plan.kernel), ga);   // (refused: fallback_kernel's tile, not the row's)
      if (d <= 0) return d;
    }
    kernel = fallback_kernel(ctx, g);
  }
  // a forced kernel (or AUTO's fall-back): its family's launcher, else the register-staged tile its row names
  const KernelRow *row = kernel_row(kernel);
  if (!row) {
    set_last_error("unknown kernel variant");
    return MMH_ERR_INVALID_ARG;
  }
  const int d = launch_family(ctx, *row, g);
  return (d <= 0 || row->fallback < 0) ? d : launch_reg(ctx, row->fallback, g);
}

// ---- mmh_sgemm_batched's plan; argument rules the call and the plan entry points share ----
namespace {
struct BatchPlan {
  int form = 0;      // MMH_BATCH_FORM_*
  int kernel = -1;   // one launch: the tile; fold / loop: the per-matrix (folded) plan's kernel, -1 = its fallback
  Plan per;          // fold / loop: the plan of the one GEMM mmh_sgemm_op runs (the folded one, or one matrix's)
};

// (mmh_sgemm_batched_ex: ... and the biases are ONE bias of the folded GEMM -- none, a column bias the whole batch shares, or
// row biases packed m apart: a row bias of batch x m floats)
bool fold_ok(const GemmArgs &g, const BatchArgs &b) {
  const bool bias_folds = g.bias_mode == MMH_BIAS_NONE || (g.bias_mode == MMH_BIAS_COL && b.sBias == 0) ||
                          (g.bias_mode == MMH_BIAS_ROW && b.sBias == g.m);
  return !g.ta && b.sB == 0 && b.sA == (long long)g.m * g.lda && b.sC == (long long)g.m * g.ldc &&
         (long long)b.batch * g.m <= 0x7fffffff && bias_folds;
}

// MMH_KERNEL_AUTO for a batch: fold where the matrices ARE one GEMM (B shared, A and C packed); else the cheaper of one
// batched launch on one of the three tiles -- the plain price of auto_plan_for with batch x tiles per matrix, thin edge
// tiles and ragged last round included -- and a loop of the per-matrix plan at batch x its price.  A batch of one is the
// per-matrix plan.  (g.ex, mmh_sgemm_batched_ex: the per-matrix plan is the `ex` call's, the tiles' plain price the same.)
BatchPlan batched_plan_for(const mmh_context *ctx, const GemmArgs &g, const BatchArgs &b) {
  BatchPlan bp;
  if (fold_ok(g, b)) {
    GemmArgs f = g;
    f.m = (int)(b.batch * g.m);
    bp.form = MMH_BATCH_FORM_FOLD;
    bp.per = auto_plan_for(ctx, f);
    bp.kernel = bp.per.kernel;
    return bp;
  }
  bp.form = MMH_BATCH_FORM_LOOP;
  bp.per = auto_plan_for(ctx, g);
  bp.kernel = bp.per.kernel;
  if (b.batch == 1) return bp;
  double best = bp.per.kernel >= 0 ? (double)b.batch * bp.per.us : 0.0;
  for (const Family &f : kFamilies) {
    if (!has_op_forms(f.kernel)) continue;
    const int form = dma5_form(ctx, f.bm, f.bn, g, b);
    if (form < 0) continue;
    const long per = (long)((g.m + f.bm - 1) / f.bm) * ((g.n + f.bn - 1) / f.bn);
    const double t = plain_us(ctx, f, g.k, b.batch * per, b.batch * full_tiles(g.m, g.n, f.bm, f.bn), form == 0);
    if (bp.kernel < 0 || t < best) {
      best = t;
      bp.form = MMH_BATCH_FORM_ONE_LAUNCH;
      bp.kernel = f.kernel;
    }
  }
  return bp;
}

bool op_flags_ok(int ta, int tb) { return (ta == MMH_OP_N || ta == MMH_OP_T) && (tb == MMH_OP_N || tb == MMH_OP_T); }

// the argument rules of mmh_sgemm_batched that need no pointer (mmh_auto_plan_batched shares them)
int check_batch_args(int ta, int tb, int m, int n, int ldc, long long sA, long long sB, long long sC, long batch) {
  if (!op_flags_ok(ta, tb)) return MMH_ERR_INVALID_ARG;
  if (batch < 0 || sA < 0 || sB < 0 || sC < 0) return MMH_ERR_INVALID_ARG;
  if (batch > 1 && m > 0 && n > 0 && ldc >= n && sC < (long long)(m - 1) * ldc + n) return MMH_ERR_INVALID_ARG;   // C matrices overlap
  return MMH_OK;
}

// What the plan entry points (mmh_auto_plan*) run the launch path's own functions on: a default handle of `cu_count` CUs and
// operands at addresses that are never dereferenced -- a 16-byte (or only 4-byte) aligned base each.  MMH_ERR_INVALID_ARG
// for a shape mmh_sgemm_op refuses.
int plan_inputs(int ta, int tb, int m, int n, int k, int lda, int ldb, int ldc, int base_align, int cu_count, mmh_context *ctx,
                GemmArgs *g) {
  if (!op_flags_ok(ta, tb)) return MMH_ERR_INVALID_ARG;
  if (m <= 0 || n <= 0 || k <= 0 || lda < (ta ? m : k) || ldb < (tb ? k : n) || ldc < n) return MMH_ERR_INVALID_ARG;
  ctx->cu_count = cu_count > 0 ? cu_count : 256;
  const uintptr_t base = (uintptr_t)1 << 32, off = base_align >= 16 ? 0 : 4;
  *g = op_args(ta, tb, m, n, k, reinterpret_cast<const float *>(base + off), lda, reinterpret_cast<const float *>(2 * base + off), ldb,
               reinterpret_cast<float *>(3 * base + off), ldc, 0, nullptr);
  return MMH_OK;
}

// ---- mmh_sgemm_op, mmh_sgemm_ex, mmh_sgemm_batched, mmh_sgemm_batched_ex: the call forms of the three K2W tiles with op forms ----
// They run on those tiles (AUTO: the table restricted to them; forced: 29 / 30 / 31) and on a naive kernel of their own; every
// other kernel, and operands beyond the 2 GiB descriptor window (the register-staged fallback is NN-only), are refused before
// anything is launched.  Split-K and MMH_OPT_STREAMK_CHAIN = 0 are NN A/B switches: these forms run the chained stream-K
// kernels, which keep the bits.  What differs between them: their own argument rules, the empty contraction, the naive
// kernel, AUTO's plan, the launcher -- and the subject of the two refusals.
struct CallText {
  const char *run, *need, *what, *why;
};
constexpr CallText kCallText[] = {
    {"transposed operands run", "transposed operands need", "an operand", " (the register-staged tiles take NN operands only)"},
    {"the fused epilogue runs", "the fused epilogue needs", "an operand", ""},
    {"batched GEMMs run", "batched GEMMs need", "a matrix", ""},
    {"batched GEMMs with the fused epilogue run", "batched GEMMs with the fused epilogue need", "a matrix", ""}};

int naive_call(Call call, const GemmArgs &g, const BatchArgs &b) {
  switch (call) {
    case Call::BatchedEx: return launch_naive_batched_ex(g, b);
    case Call::Batched: return launch_naive_batched(g, b);
    case Call::Ex: return launch_naive_ex(g);
    default: return launch_naive_op(g);
  }
}
// (1: not a tile with op forms -- AUTO found none --, or the shape does not qualify)
int tile_call(Call call, mmh_context *ctx, int kernel, const GemmArgs &g, const BatchArgs &b) {
  switch (call) {
    case Call::BatchedEx: return launch_dma5_batched_ex(ctx, kernel, g, b);
    case Call::Batched: return launch_dma5_batched(ctx, kernel, g, b);
    case Call::Ex: return launch_dma5_ex(ctx, kernel, g);
    default: return launch_dma5_op(ctx, kernel, g);
  }
}
// one GEMM of a batched call's fold or loop form: m rows at A, C (and bias), as the unbatched call of the same kind runs it
int one_gemm(mmh_context *ctx, GemmArgs g, int m, const float *A, const float *B, float *C, const float *bias) {
  g.m = m;
  g.A = A;
  g.B = B;
  g.C = C;
  g.bias = bias;
  return call_on(ctx, g.ex ? Call::Ex : Call::Op, MMH_KERNEL_AUTO, g);
}
}  // namespace

// g: the call's arguments as they came (ta / tb, bias and its mode unchecked; acc 0 / 1); b: a batched call's
int call_on(mmh_context *ctx, Call call, int kernel, GemmArgs g, const BatchArgs &b) {
  const CallText &text = kCallText[(int)call];
  const bool batched = call == Call::Batched || call == Call::BatchedEx, ex = call == Call::Ex || call == Call::BatchedEx;
  if (!op_flags_ok(g.ta, g.tb)) {
    set_last_error(batched ? "invalid argument" : "transa / transb must be MMH_OP_N or MMH_OP_T");
    return MMH_ERR_INVALID_ARG;
  }
  // NN is mmh_sgemm's own path -- but for an epilogue call, which is planned like an op call (auto_plan_for, g.ex)
  if (call == Call::Op && !g.ta && !g.tb) return sgemm_on(ctx, kernel, g.m, g.n, g.k, g.A, g.lda, g.B, g.ldb, g.C, g.ldc, g.acc, g.s);
  if (ex && (g.bias_mode < MMH_BIAS_NONE || g.bias_mode > MMH_BIAS_ROW || (g.act != MMH_ACT_NONE && g.act != MMH_ACT_RELU) ||
             (g.bias_mode != MMH_BIAS_NONE && !g.bias))) {
    set_last_error("bias_mode must be MMH_BIAS_NONE / _COL / _ROW (with a bias pointer), activation MMH_ACT_NONE / _RELU");
    return MMH_ERR_INVALID_ARG;
  }
  if (batched && g.bias_mode != MMH_BIAS_NONE && b.sBias < 0) {
    set_last_error("strideBias must not be negative");
    return MMH_ERR_INVALID_ARG;
  }
  if (g.bias_mode == MMH_BIAS_NONE) g.bias = nullptr;
  int rc = batched ? check_batch_args(g.ta, g.tb, g.m, g.n, g.ldc, b.sA, b.sB, b.sC, b.batch) : MMH_OK;
  if (rc == MMH_OK && b.batch > 0) rc = check_gemm_args(g.m, g.n, g.k, g.A, g.lda, g.B, g.ldb, g.C, g.ldc, g.ta, g.tb);
  if (rc != MMH_OK) {
    set_last_error("invalid argument");
    return rc;
  }
  if (b.batch == 0 || g.m == 0 || g.n == 0) return MMH_OK;
  if (kernel != MMH_KERNEL_AUTO && kernel != MMH_KERNEL_NAIVE && !has_op_forms(kernel)) {
    set_last_error(std::string(text.run) + " on MMH_KERNEL_AUTO, the 64x64 / 128x64 / 128x128 LDS-DMA tiles (29 / 30 / 31) and "
                   "MMH_KERNEL_NAIVE only");
    return MMH_ERR_UNSUPPORTED;
  }
  if (g.k == 0 && !ex) {
    // empty contraction: C = 0 (overwrite) or C unchanged (accumulate); a batch's zeros go out through the naive kernel,
    // matrix by matrix.  (ex: s = +0 through the naive kernel's epilogue, A and B are not read)
    if (g.acc) return MMH_OK;
    if (batched) return launch_naive_batched(g, b);
    HIP_TRY(hipMemset2DAsync(g.C, (size_t)g.ldc * sizeof(float), 0, (size_t)g.n * sizeof(float), (size_t)g.m, g.s));
    return MMH_OK;
  }
  if (g.k == 0 || kernel == MMH_KERNEL_NAIVE) return naive_call(call, g, b);
  if (kernel == MMH_KERNEL_AUTO && batched) {
    const BatchPlan bp = batched_plan_for(ctx, g, b);
    const int batch = (int)b.batch;
    if (bp.form == MMH_BATCH_FORM_FOLD) {
      rc = one_gemm(ctx, g, batch * g.m, g.A, g.B, g.C, g.bias);
      if (rc == MMH_OK)
        set_last_launch(last_launch_ref() + ", batch " + std::to_string(batch) + " folded into one " + std::to_string(batch * g.m) +
                        "-row GEMM");
      return rc;
    }
    if (bp.form == MMH_BATCH_FORM_LOOP) {
      for (int i = 0; i < batch && rc == MMH_OK; ++i)
        rc = one_gemm(ctx, g, g.m, g.A + i * b.sA, g.B + i * b.sB, g.C + i * b.sC, g.bias ? g.bias + i * b.sBias : nullptr);
      if (rc == MMH_OK)
        set_last_launch(last_launch_ref() + ", batch " + std::to_string(batch) + " as a loop of " + std::to_string(batch) +
                        " per-matrix launches");
      return rc;
    }
    kernel = bp.kernel;
  } else if (kernel == MMH_KERNEL_AUTO) {
    const Plan plan = auto_plan_for(ctx, g);
    if (plan.kernel >= 0) {
      g.form = plan.form;
      g.sk_w = plan.sk_w;
      kernel = plan.kernel;
    }
  }
  const int d = tile_call(call, ctx, kernel, g, b);
  if (d <= 0) return d;
  set_last_error(std::string(text.need) + " the LDS-DMA tiles: " + text.what + " lies beyond their 2 GiB descriptor window, or "
                 "MMH_OPT_DMA_EDGE keeps this shape off them" + text.why);
  return MMH_ERR_UNSUPPORTED;
}
// mmh_auto_plan_batched (ex = 0, no bias) and mmh_auto_plan_batched_ex: batched_plan_for on a default handle, as host arithmetic
int plan_batched(int ta, int tb, int m, int n, int k, int lda, int ldb, int ldc, long long sA, long long sB, long long sC,
                 long long sBias, int bias_mode, int ex, int batch, int base_align, int cu_count, int *kernel, int *form,
                 long *workgroups) {
  mmh_context ctx;
  GemmArgs g;
  if (bias_mode < MMH_BIAS_NONE || bias_mode > MMH_BIAS_ROW || (bias_mode != MMH_BIAS_NONE && sBias < 0)) return MMH_ERR_INVALID_ARG;
  if (check_batch_args(ta, tb, m, n, ldc, sA, sB, sC, batch) != MMH_OK || batch < 1) return MMH_ERR_INVALID_ARG;
  if (plan_inputs(ta, tb, m, n, k, lda, ldb, ldc, base_align, cu_count, &ctx, &g) != MMH_OK) return MMH_ERR_INVALID_ARG;
  g.ex = ex;
  g.bias_mode = bias_mode;
  const BatchArgs b{sA, sB, sC, batch, sBias};
  const BatchPlan bp = batched_plan_for(&ctx, g, b);
  if (form) *form = bp.form;
  if (bp.form == MMH_BATCH_FORM_ONE_LAUNCH) {
    if (kernel) *kernel = bp.kernel;
    if (workgroups)
      *workgroups = (long)batch * k2w_tiles::with(bp.kernel, [&](auto t) { return ((m + t.BM - 1) / t.BM) * ((n + t.BN - 1) / t.BN); }, 0);
    return MMH_OK;
  }
  // fold / loop: mmh_auto_plan_op on the one GEMM mmh_sgemm_op runs, times the launches
  const bool fold = bp.form == MMH_BATCH_FORM_FOLD;
  long tiles = 0;
  int grid = 0;
  const int rc = auto_plan_op(ta, tb, fold ? batch * m : m, n, k, lda, ldb, ldc, base_align, cu_count, kernel, &tiles, &grid, ex);
  if (rc != MMH_OK) return rc;
  if (workgroups) *workgroups = (fold ? 1L : (long)batch) * (grid > 0 ? grid : tiles);
  return MMH_OK;
}

// What MMH_KERNEL_AUTO would do with a shape, as host arithmetic (mmh_auto_plan: no device, no launch): the tile it
// picks and, for the tiles whose residency the LDS alone decides, whether the launch would be the persistent
// stream-K form.  Uses the very functions the launch path uses (auto_kernel, streamk_wanted) on a default handle.
int auto_plan(int m, int n, int k, int lda, int ldb, int ldc, int base_align, int cu_count, int *kernel, long *tiles,
              int *streamk_grid) {
  return auto_plan_op(MMH_OP_N, MMH_OP_N, m, n, k, lda, ldb, ldc, base_align, cu_count, kernel, tiles, streamk_grid);
}

// mmh_auto_plan_op: the same for C = op(A) op(B); an op form no tile with op forms takes is MMH_ERR_UNSUPPORTED
// (ex: mmh_auto_plan_ex -- an epilogue call is planned like an op form, NN too)
int auto_plan_op(int ta, int tb, int m, int n, int k, int lda, int ldb, int ldc, int base_align, int cu_count, int *kernel,
                 long *tiles, int *streamk_grid, int ex) {
  mmh_context ctx;
  GemmArgs g;
  if (plan_inputs(ta, tb, m, n, k, lda, ldb, ldc, base_align, cu_count, &ctx, &g) != MMH_OK) return MMH_ERR_INVALID_ARG;
  g.ex = ex;
  const Plan plan = auto_plan_for(&ctx, g);
  if ((ta || tb || ex) && plan.kernel < 0) return MMH_ERR_UNSUPPORTED;
  const int kern = plan.kernel >= 0 ? plan.kernel : fallback_kernel(&ctx, g);
  if (kernel) *kernel = kern;
  const long t = plan.kernel >= 0 ? (long)((m + plan.bm - 1) / plan.bm) * ((n + plan.bn - 1) / plan.bn)
                                  : reg_tile_count(kern, m, n);   // (the register-staged fall-back tiles)
  if (tiles) *tiles = t;
  if (streamk_grid) {
    *streamk_grid = -1;
    if (plan.kernel >= 0) {
      *streamk_grid = 0;
      if (plan.form == 2) {   // (the grid the price was taken for: plan.sk_w workgroups per CU, GemmArgs::sk_w)
        const int grid = mmh::streamk_grid(t, ctx.cu_count, plan.sk_w);
        *streamk_grid = (grid > 0 && t % grid != 0) ? grid : 0;   // (launch_streamk: a count the grid divides runs plain)
      }
    }
  }
  return MMH_OK;
}

}  // namespace mmh
