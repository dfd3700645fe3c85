// Host side of the filtered eigen-solver (filter.hip): workspace layout, descriptor construction and the launch
// sequence of one group of problems.  Used by the TT plan (plan.hip) for the eigen-problems whose kept rank is a
// fraction of their size, and by tadmm_eigh_top_f64 (tests).
#pragma once
#include <memory>
#include "host.h"

namespace tadmm {

// size of the iteration block for keeping r of N eigenvectors (0: not worth filtering -> full solve)
static inline int filter_block_size(int N, int r) {
  const char* e = getenv("TADMM_FILTER");            // 0 disables the filtered path (A/B measurements, tests)
  if (e && !atoi(e)) return 0;
  int min_n = 192;
  if (const char* m = getenv("TADMM_FILTER_MINN")) min_n = atoi(m);
  if (N < min_n || r < 16) return 0;
  double over = 1.45;     // (1.55 until round 3: 6.71 -> 6.52 ms per ResNet-50 iteration; 1.3 - 1.45 measure the same, 1.5 6.65, 1.65 8.9)
  if (const char* o = getenv("TADMM_FILTER_OVERSAMPLE")) over = atof(o);
  int rp = (int)align_up((size_t)(over * r + 0.999), 32);
  // The block is capped at 256 columns (register-resident Cholesky, chol.hip).  A kept rank whose preferred block would
  // be wider still takes the filter with the capped block while that leaves >= `min_over` of oversampling: the boundary
  // (lambda_r against lambda_{r'+1}) is closer, so the device-side planner spends more products, but a Rayleigh-Ritz
  // tournament over 256 columns instead of N = 480 / 512 is still the shorter chain (ResNet-18 layer4: r = 210 / 220).
  double min_over = 1.15;
  if (const char* o = getenv("TADMM_FILTER_MIN_OVERSAMPLE")) min_over = atof(o);
  if (rp > 256) {
    rp = 256;
    if ((double)rp < min_over * r) return 0;
  }
  if (rp * 100 > 56 * N || rp <= r) return 0;
  return rp;
}

// Guards of the filtered solve (filter.hip).  TADMM_FILTER_GUARD unset: the moments guard (in line, ~3 us); = n > 0: the
// moments guard AND n power steps on the deflated operator (side stream; 0.35 ms of the ResNet-50 iteration); = 0: none
// (A/B measurements, tests).
static inline int filter_guard_steps() {
  if (const char* e = getenv("TADMM_FILTER_GUARD")) return std::max(0, std::min(16, atoi(e)));
  return 0;
}
static inline bool filter_moments_on() {
  const char* e = getenv("TADMM_FILTER_GUARD");
  return !(e && atoi(e) == 0);
}

static inline int filter_tile_n() {
  const char* e = getenv("TADMM_FILTER_TN");
  return (e && atoi(e) == 64) ? 64 : 32;
}
// Rows of a product tile for a group of problems whose 64-row tiling has `tiles64` workgroups per product launch and whose
// widest block has rp_max columns: 32 (32 x 32 tiles, twice the workgroups, half the duration each) while the launch is
// latency-bound -- even the doubled count leaves the chip (256 CUs) about one workgroup per CU -- and the blocks are
// narrow (r' <= 192: at most 6 row tiles re-stream a 32-row panel of G); 64 otherwise.  A workgroup's duration is its
// share of ONE CU's fp64 matrix rate (a 64 x 32 x 480 tile is 2 MFLOP = 11 us at ~176 GFLOP/s), so halving the tile halves
// the launch as long as there are CUs to spare.  Measured (separate processes, one box): ResNet-50 (levels of 160 - 288
// tiles, r' = 160 / 192) 6.54 -> 6.27 ms per iteration with 32; ResNet-18 (256-column blocks, 120 - 380 tiles a level, the
// other lane saturated by full tournaments) 8.81 -> 9.16 with 32.  TADMM_FILTER_TM = 32 | 64 forces one.
static inline int filter_tile_m(int tiles64, int rp_max) {
  if (const char* e = getenv("TADMM_FILTER_TM")) return atoi(e) == 32 ? 32 : 64;
  if (filter_tile_n() != 32) return 64;
  int limit = 288;
  if (const char* e = getenv("TADMM_FILTER_TM_TILES")) limit = atoi(e);
  return (tiles64 <= limit && rp_max <= 192) ? 32 : 64;
}

struct FilterSpec {
  int N = 0, Npad = 0, ldg = 0, r = 0, rp = 0;
  const double* G = nullptr;        // [Npad][ldg] symmetric, zero padded (left untouched by the filter)
  int mode = 0, ldo = 0;            // output convention (EigDesc)
  float* out_a = nullptr; float* out_b = nullptr;
  double* sigma = nullptr;          // [r]
  int32_t* skip_slot = nullptr;     // device word in the skip array of the eig group that runs the Rayleigh-Ritz solve
  int32_t* fb_skip = nullptr;       // device word in the skip array of the fallback group
  // complement route (complement.hip): G above is the REFLECTED image G' (written by comp_prepare from g_orig), r the
  // number of DISCARDED vectors, comp_r the number of kept ones; mode is 4 (the filter itself emits nothing)
  int comp_r = 0;
  const double* g_orig = nullptr;
  double* sigma_layer = nullptr;
};

// Size of the filter block for the complement route, or 0: a rows-side step (Z-only mode) that keeps r <= 256 of N and
// discards k = N - r with 16 <= k <= 64 -- there the discarded subspace is the cheap one (DeiT-small proj / fc2: N = 288,
// keep 256).  OPT-IN (TADMM_COMPLEMENT=1): results are verified and parity-tested (tests/test_gpu_round3.py), but on
// the synthetic DeiT-small table 1-2 of the 22 problems per iteration fail their verification (the trailing end of a
// Wishart spectrum is dense: the Rayleigh-quotient bounds of the early stages mislead the stage planner), and ONE
// fallback -- a full N = 288 tournament queued behind the level's filter stages -- costs more than the route saves:
// 11.4 - 13.9 ms per iteration against 10.0 ms without it.
static inline int complement_block_size(int N, int r, bool trans, bool zonly) {
  const char* e = getenv("TADMM_COMPLEMENT");
  if (!e || !atoi(e)) return 0;
  const int k = N - r;
  if (!zonly || trans || r > 256 || (r % 32) || k < 16 || k > 64) return 0;
  return filter_block_size(N, k);
}

// instrumented runs only (tadmm_plan_enable_timing): the fp64 GEMM launches of the filter are timed one by one
struct FilterTiming {
  bool on = false;
  hipEvent_t a{}, b{};
  double gemm_ms = 0.0; int gemm_launches = 0; double gemm_flops = 0.0;
  double fast_ms = 0.0; int fast_launches = 0; double fast_flops = 0.0;      // dgemm3 launches (algorithmic flops)
};

// Side stream of the guard (filt_guard_kernel): it only needs the final orthonormal block, so it runs BESIDE the
// Rayleigh-Ritz solve (a chain of latency-bound launches on a handful of CUs) instead of in front of the verdict.
struct GuardSide {
  hipStream_t st = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  bool ok = false;
  GuardSide() {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    ok = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, lo) == hipSuccess &&
         hipEventCreateWithFlags(&fork, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&join, hipEventDisableTiming) == hipSuccess;
  }
  ~GuardSide() {
    if (fork) (void)hipEventDestroy(fork);
    if (join) (void)hipEventDestroy(join);
    if (st) (void)hipStreamDestroy(st);
  }
  GuardSide(const GuardSide&) = delete;
  GuardSide& operator=(const GuardSide&) = delete;
};

struct FilterGroup {
  int nf = 0;
  std::shared_ptr<GuardSide> side;           // created at the first run (on the plan's device)
  bool guard_forked = false;
  // complement route: problems whose FilterSpec carries comp_r
  int ncomp = 0, comp_npad_max = 0;
  size_t comp_off = 0;                       // CompDesc[ncomp]
  Phase cform, cgram, cemit;
  size_t cchol_off = 0, csolve_map_off = 0; int csolve_blocks = 0;
  int npad_max = 0, rp_max = 0;              // LDS of the guard kernel
  int max_degree = 8;
  int tile_m = 64;                           // rows of a product tile (filter_tile_m)
  size_t prob_off = 0;                       // FiltProb[nf]
  Phase init, stage0, p1, axpby, tfinal, hform, uform, verify, emit;
  std::vector<Phase> steps;                  // recurrence steps k = 2 .. max_degree
  Phase gramA, gramB;                        // Gram of the block: gated on "stage ran" / on "alive"
  size_t cholA_off = 0, cholB_off = 0;       // CholDesc[nf]
  size_t solve_map_off = 0; int solve_blocks = 0;
  size_t zero_off = 0, zero_bytes = 0;       // Rayleigh-Ritz images: padding must be zero (cleared at creation)
  // products at fp32 accuracy on the bf16 matrix cores (dgemm3.hip): planes of G + the same phases on 32 x 64 tiles
  Phase gplanes, stage0_f, p1_f;
  std::vector<Phase> steps_f;
  int fast_stages = -1;                      // stages 0 .. fast_stages-1 of the next run take the fast products
  // statistics of the last run (host)
  int last_stages = 0, last_bad = 0;
};

// How many leading filter stages run at fp32 accuracy: all but the last one the group needed in its previous run
// (the spectra of consecutive ADMM iterations are alike); none in a plan's first run.  OFF unless TADMM_FILTER_FAST=1
// (TADMM_FILTER_FAST_STAGES=n additionally forces n): numerically validated, but on MI355X a dgemm3 launch is bound by
// the same L2 -> CU operand traffic as the fp64 launch it replaces and is not faster yet.
static inline int filter_fast_stages(const FilterGroup& fg) {
  const char* on = getenv("TADMM_FILTER_FAST");
  if (!on || !atoi(on)) return 0;          // opt-in: see DESIGN.md 5 -- per launch the fast product is not yet faster
  if (const char* e = getenv("TADMM_FILTER_FAST_STAGES")) return std::max(0, atoi(e));
  return std::max(0, fg.fast_stages);
}

// Rayleigh-Ritz eigen-problem of filtered problem i (appended by the caller to its eig group)
struct FilterRR { EigDesc desc; int norm_blocks; int ext_blocks; };

// Lays out workspace + descriptors.  `dev(off)` turns an arena offset into a device pointer (null while sizing).
template <class DevFn>
static inline void filter_layout(FilterGroup& fg, const std::vector<FilterSpec>& specs, Arena& da, Arena& ar, DevFn dev,
                                 HostImage* img, std::vector<FilterRR>& rr_out) {
  const int nf = (int)specs.size();
  fg.nf = nf;
  rr_out.clear();
  if (nf == 0) return;
  fg.max_degree = 8;
  {
    // a level of complement problems filters the narrow trailing end of the spectrum: the boundary rate is small, the
    // growth of the block's condition number per step as well -- longer stages (fewer CholQRs) are safe and pay
    bool all_comp = true;
    for (const FilterSpec& f : specs) all_comp = all_comp && f.comp_r > 0;
    if (all_comp) fg.max_degree = 16;
    // blocks with the preferred oversampling (r' >= 1.4 r: every ResNet-50 problem) converge fast enough per step that the
    // stage count, not the step count, is what their chain pays for: stages of up to 12 steps (4 - 5 stages instead of
    // 6, the same products).  Measured, separate processes on one box: ResNet-50 6.91 -> 6.71 ms per iteration (10: 6.79,
    // 14: 6.75, 16: 6.8 - 7.3); the capped 256-column blocks of ResNet-18 (oversampling 1.16 - 1.22) lose 0.03 ms with
    // longer stages and keep 8.
    bool all_wide = !all_comp;
    for (const FilterSpec& f : specs) all_wide = all_wide && f.comp_r == 0 && 10 * f.rp >= 14 * f.r;
    if (all_wide) fg.max_degree = 12;
  }
  if (const char* e = getenv("TADMM_FILTER_DEGREE")) fg.max_degree = std::max(2, std::min(16, atoi(e)));
  {
    int tiles64 = 0, rp_max = 0;
    for (const FilterSpec& f : specs) {
      tiles64 += ((f.rp + 63) / 64) * ((f.Npad + filter_tile_n() - 1) / filter_tile_n());
      rp_max = std::max(rp_max, f.rp);
    }
    fg.tile_m = filter_tile_m(tiles64, rp_max);
  }
  const int D = fg.max_degree;
  std::vector<FiltProb> probs(nf);
  std::vector<DgemmDesc> d_stage0(nf), d_p1(nf), d_axpby(nf), d_tfinal(nf), d_hform(nf), d_uform(nf), d_verify(nf),
      d_gramA(nf), d_gramB(nf);
  std::vector<std::vector<DgemmDesc>> d_steps(std::max(0, D - 1), std::vector<DgemmDesc>(nf));
  std::vector<CholDesc> cA(nf), cB(nf);
  std::vector<BlockRef> m_init, m_stage0, m_axpby, m_hform, m_uform, m_verify, m_emit, m_gram, m_solve, m_fast, m_gp;
  std::vector<GPlaneDesc> d_gp(nf);
  std::vector<CompDesc> d_comp;
  std::vector<DgemmDesc> d_cgram;
  std::vector<CholDesc> c_comp;
  std::vector<BlockRef> m_cform, m_cgram, m_cemit, m_csolve;
  std::vector<TileProb> t_stage0, t_gram, t_verify, t_cgram;      // populations of the launch_dgemm_nt64 maps
  fg.ncomp = 0; fg.comp_npad_max = 0;
  const size_t zero_begin = align_up(ar.off, 256);
  std::vector<size_t> xth_off(nf), vh_offs(nf);
  for (int i = 0; i < nf; ++i) {   // images whose padding must be zero first, contiguous: one memset clears them
    const int ldh = (int)align_up(specs[i].rp, 128);
    xth_off[i] = ar.take((size_t)specs[i].rp * ldh * 8);                              // Rayleigh-Ritz image
    vh_offs[i] = ar.take(align_up(specs[i].r, 32) * (size_t)specs[i].rp * 8);         // Ritz vectors, rows >= r stay 0
  }
  fg.zero_off = zero_begin;
  fg.zero_bytes = ar.off - zero_begin;
  for (int i = 0; i < nf; ++i) {
    const FilterSpec& sp = specs[i];
    const int rp = sp.rp, Npad = sp.Npad, r32 = (int)align_up(sp.r, 32), ldy = Npad, ldh = (int)align_up(rp, 128);
    const int TNW = filter_tile_n();
    const int TMW = fg.tile_m;
    const int tn = (Npad + TNW - 1) / TNW;                                 // TMW x TNW tiles of the NT products with G
    size_t ring_off[3];
    for (auto& o : ring_off) o = ar.take((size_t)rp * ldy * 8);
    const size_t st_off = ar.take(sizeof(FiltState));
    const size_t c_off = ar.take((size_t)rp * rp * 8);
    const size_t r_off = ar.take((size_t)rp * rp * 8);
    const size_t w_off = ar.take((size_t)rp * 16 * 8);
    const size_t rq_off = ar.take((size_t)tn * rp * 8);
    const size_t vp_off = ar.take((size_t)tn * r32 * 8);
    const size_t vh_off = vh_offs[i];                            // Ritz vectors in the block basis, rows (zero beyond r)
    const int gnt = Npad / 16, gks = Npad / 32;                  // fragment-major bf16 planes of G (dgemm3.hip)
    const int64_t gplane = (int64_t)gnt * gks * 512;
    const size_t gp_off = ar.take((size_t)3 * gplane * 2);
    {
      GPlaneDesc& gd = d_gp[i];
      memset(&gd, 0, sizeof gd);
      gd.Gm = sp.G; gd.ldg = sp.ldg; gd.nt = gnt; gd.ks = gks; gd.out = (uint16_t*)dev(gp_off); gd.plane = gplane;
    }
    const size_t ut_off = ar.take((size_t)r32 * ldy * 8);
    const size_t th_off = ar.take((size_t)r32 * 8);
    const size_t lam_off = ar.take((size_t)rp * 8);
    const size_t ord_off = ar.take((size_t)rp * 4);
    const size_t off_off = ar.take(3 * 8);
    const size_t done_off = ar.take(4);
    const size_t sblk_off = ar.take((size_t)(rp / 16) * 256 * 8);
    FiltState* st = (FiltState*)dev(st_off);
    double* ring[3] = {(double*)dev(ring_off[0]), (double*)dev(ring_off[1]), (double*)dev(ring_off[2])};

    FiltProb& p = probs[i];
    memset(&p, 0, sizeof p);
    p.st = st;
    for (int k = 0; k < 3; ++k) p.ring[k] = ring[k];
    p.N = sp.N; p.Npad = Npad; p.rp = rp; p.r = sp.r; p.r32 = r32; p.ldy = ldy;
    p.rqpart = (const double*)dev(rq_off); p.rq_tiles = tn;
    p.vpart = (const double*)dev(vp_off); p.v_tiles = tn;
    p.lam = (const double*)dev(lam_off); p.order = (const int32_t*)dev(ord_off);
    p.sigma = sp.sigma; p.theta = (double*)dev(th_off); p.UT = (const double*)dev(ut_off);
    p.mode = sp.mode; p.ldo = sp.ldo; p.out_a = sp.out_a; p.out_b = sp.out_b;
    p.skip_slot = sp.skip_slot; p.fb_skip = sp.fb_skip;
    p.G = sp.G; p.ldg = sp.ldg;
    p.H = (const double*)dev(xth_off[i]); p.ldh = ldh;
    fg.npad_max = std::max(fg.npad_max, Npad); fg.rp_max = std::max(fg.rp_max, rp);
    auto base_desc = [&](int M, int N_, int K) {
      DgemmDesc g;
      memset(&g, 0, sizeof g);
      for (int k = 0; k < 3; ++k) g.ring[k] = ring[k];
      g.selA = g.selB = g.selC = g.selP = g.selQ = -1;
      g.M = M; g.N = N_; g.K = K;
      g.tiles_m = M / 32; g.tiles_n = N_ / 32;
      g.Gp = (const uint16_t*)dev(gp_off); g.g_plane = gplane;
      return g;
    };
    const int32_t* w_base = st ? &st->base : nullptr;
    const int32_t* w_res = st ? &st->res : nullptr;
    const int32_t* w_nsteps = st ? &st->nsteps : nullptr;
    const int32_t* w_active = st ? &st->active : nullptr;
    const int32_t* w_alive = st ? &st->alive : nullptr;
    // stage 0: ring[1] = G * ring[0]        (block images are [rp][ldy]: C[j][i] = sum_k Y[j][k] G[i][k])
    {
      DgemmDesc g = base_desc(rp, Npad, Npad);
      g.rot = w_base; g.selA = 0; g.selC = 1; g.B = sp.G;
      g.lda = ldy; g.ldb = sp.ldg; g.ldc = ldy; g.mode = 0;
      d_stage0[i] = g;
    }
    // first product of a stage: T = G Q  + Rayleigh quotients
    {
      DgemmDesc g = base_desc(rp, Npad, Npad);
      g.rot = w_base; g.selA = 0; g.selC = 1; g.selP = 0; g.B = sp.G;
      g.lda = ldy; g.ldb = sp.ldg; g.ldc = ldy; g.mode = 2; g.rowpart = (double*)dev(rq_off);
      g.gate = w_active; g.gate_min = 1;
      d_p1[i] = g;
    }
    {   // Y1 = coef1[0]*T + coef1[1]*Q in place of T
      DgemmDesc g = base_desc(rp, Npad, Npad);
      g.rot = w_base; g.selC = 1; g.selP = 0; g.ldc = ldy;
      g.coef = st ? st->coef1 : nullptr; g.gate = w_nsteps; g.gate_min = 1;
      d_axpby[i] = g;
    }
    for (int k = 2; k <= D; ++k) {     // Y_k = c0*G*Y_{k-1} + c1*Y_{k-1} + c2*Y_{k-2}, Y_j in ring[(base + j) % 3]
      DgemmDesc g = base_desc(rp, Npad, Npad);
      g.rot = w_base; g.selA = (k - 1) % 3; g.selP = (k - 1) % 3; g.selQ = (k - 2) % 3; g.selC = k % 3; g.B = sp.G;
      g.lda = ldy; g.ldb = sp.ldg; g.ldc = ldy; g.mode = 1;
      g.coef = st ? st->coefk : nullptr; g.gate = w_nsteps; g.gate_min = k;
      d_steps[k - 2][i] = g;
    }
    // Gram of the block that is about to be orthonormalised: C = Y^T Y
    {
      DgemmDesc g = base_desc(rp, rp, Npad);
      g.rot = w_res; g.selA = 0; g.selB = 0; g.C = (const double*)dev(c_off);
      g.lda = ldy; g.ldb = ldy; g.ldc = rp; g.mode = 0;
      g.gate = w_nsteps; g.gate_min = 1;
      d_gramA[i] = g;
      g.gate = w_alive; g.gate_min = 1;
      d_gramB[i] = g;
    }
    {
      CholDesc c;
      memset(&c, 0, sizeof c);
      c.C = (const double*)dev(c_off); c.ldc = rp; c.n = rp;
      c.R = (double*)dev(r_off); c.ldr = rp; c.Wd = (double*)dev(w_off);
      for (int k = 0; k < 3; ++k) c.ring[k] = ring[k];
      c.rot = w_res; c.sel = 0; c.ldy = ldy; c.ncols = Npad;
      c.bad = st ? &st->bad : nullptr;
      c.rot_out = st ? &st->base : nullptr;
      c.gate = w_nsteps; c.gate_min = 1;
      cA[i] = c;
      c.gate = w_alive; c.gate_min = 1;
      cB[i] = c;
    }
    {   // T = G Q (after the polish), then H = Q^T T
      DgemmDesc g = base_desc(rp, Npad, Npad);
      g.rot = w_base; g.selA = 0; g.selC = 1; g.B = sp.G;
      g.lda = ldy; g.ldb = sp.ldg; g.ldc = ldy; g.mode = 0; g.gate = w_alive; g.gate_min = 1;
      d_tfinal[i] = g;
      DgemmDesc hgm = base_desc(rp, rp, Npad);
      hgm.rot = w_base; hgm.selA = 0; hgm.selB = 1; hgm.C = (const double*)dev(xth_off[i]);
      hgm.lda = ldy; hgm.ldb = ldy; hgm.ldc = ldh; hgm.mode = 0; hgm.gate = w_alive; hgm.gate_min = 1;
      d_hform[i] = hgm;
    }
    {   // U^T[c][i] = sum_k VH^T[c][k] Q^T[k][i]   (NN), then residuals of the Ritz pairs
      DgemmDesc g = base_desc(r32, Npad, rp);
      g.rot = w_base; g.A = (const double*)dev(vh_off); g.selB = 0; g.C = (const double*)dev(ut_off);
      g.lda = rp; g.ldb = ldy; g.ldc = ldy; g.mode = 0; g.gate = w_alive; g.gate_min = 1;
      d_uform[i] = g;
      DgemmDesc v = base_desc(r32, Npad, Npad);
      v.A = (const double*)dev(ut_off); v.B = sp.G; v.P = (const double*)dev(ut_off);
      v.lda = ldy; v.ldb = sp.ldg; v.ldc = ldy; v.mode = 3; v.theta = (const double*)dev(th_off);
      v.rowpart = (double*)dev(vp_off); v.gate = w_alive; v.gate_min = 1;
      d_verify[i] = v;
    }
    if (sp.comp_r > 0) {       // complement route: descriptors of the kept basis (complement.hip + CholQR twice)
      const int cr = sp.comp_r, ci = fg.ncomp++;
      fg.comp_npad_max = std::max(fg.comp_npad_max, Npad);
      const size_t cimg_off = ar.take((size_t)cr * ldy * 8);
      const size_t cg_off = ar.take((size_t)cr * cr * 8);
      const size_t cr_off = ar.take((size_t)cr * cr * 8);
      const size_t cw_off = ar.take((size_t)cr * 16 * 8);
      const size_t cs_off = ar.take(8);
      CompDesc cd;
      memset(&cd, 0, sizeof cd);
      cd.st = st; cd.G = sp.g_orig; cd.Gc = (double*)sp.G; cd.N = sp.N; cd.Npad = Npad; cd.ldg = sp.ldg;
      cd.cshift = (double*)dev(cs_off);
      cd.UT = (const double*)dev(ut_off); cd.ldy = ldy; cd.k = sp.r;
      cd.Cimg = (double*)dev(cimg_off); cd.r = cr;
      cd.out_a = sp.out_a; cd.ldo = sp.ldo; cd.sigma_layer = sp.sigma_layer;
      d_comp.push_back(cd);
      DgemmDesc g = base_desc(cr, cr, Npad);
      g.A = (const double*)dev(cimg_off); g.B = (const double*)dev(cimg_off); g.C = (const double*)dev(cg_off);
      g.lda = ldy; g.ldb = ldy; g.ldc = cr; g.mode = 0; g.gate = w_alive; g.gate_min = 1;
      d_cgram.push_back(g);
      CholDesc c;
      memset(&c, 0, sizeof c);
      c.C = (const double*)dev(cg_off); c.ldc = cr; c.n = cr;
      c.R = (double*)dev(cr_off); c.ldr = cr; c.Wd = (double*)dev(cw_off);
      for (int k = 0; k < 3; ++k) c.ring[k] = (double*)dev(cimg_off);
      c.rot = nullptr; c.sel = 0; c.ldy = ldy; c.ncols = Npad;
      c.bad = st ? &st->bad : nullptr; c.rot_out = nullptr;
      c.gate = w_alive; c.gate_min = 1;
      c_comp.push_back(c);
      for (int b = 0; b < (cr + 3) / 4; ++b) { m_cform.push_back(BlockRef{ci, b}); m_cemit.push_back(BlockRef{ci, b}); }
      t_cgram.push_back(TileProb{cr, cr, Npad, TMW, TNW});
      for (int b = 0; b < Npad / kCholStrip; ++b) m_csolve.push_back(BlockRef{ci, b});
    }

    // Rayleigh-Ritz eigen-problem
    FilterRR rr;
    memset(&rr, 0, sizeof rr);
    EigDesc& e = rr.desc;
    e.XT = (double*)dev(xth_off[i]);
    e.N = rp; e.Npad = rp; e.ld = ldh; e.nb = rp / kJB;
    e.off = (double*)dev(off_off); e.done = (int32_t*)dev(done_off);
    e.lam = (double*)dev(lam_off); e.order = (int32_t*)dev(ord_off); e.sigma = sp.sigma;
    e.r = sp.r; e.mode = 2; e.evec_out = (double*)dev(vh_off); e.sblk = (double*)dev(sblk_off);
    if (eig_mid_direct_on() && eig_mid_direct_size(rp)) e.scratch = (double*)dev(ar.take(eig_mid_scratch_bytes(rp)));    // direct route (tridiag_mid.hip)
    rr.norm_blocks = (rp + 3) / 4; rr.ext_blocks = (sp.r + 3) / 4;
    rr_out.push_back(rr);
    // block maps
    const int el_blocks = (int)(((size_t)rp * ldy + 1023) / 1024);
    for (int b = 0; b < el_blocks; ++b) { m_init.push_back(BlockRef{i, b}); m_axpby.push_back(BlockRef{i, b}); }
    t_stage0.push_back(TileProb{rp, Npad, Npad, TMW, TNW});
    for (int b = 0; b < (rp / 32) * ((Npad + 63) / 64); ++b) m_fast.push_back(BlockRef{i, b});   // dgemm3: 32 x 64 tiles
    for (int b = 0; b < (gnt * gks + 3) / 4; ++b) m_gp.push_back(BlockRef{i, b});
    t_gram.push_back(TileProb{rp, rp, Npad, TMW, TNW});
    for (int b = 0; b < (r32 / 32) * (Npad / 32); ++b) m_uform.push_back(BlockRef{i, b});     // NN kernel: 32x32 tiles
    t_verify.push_back(TileProb{r32, Npad, Npad, TMW, TNW});
    for (int b = 0; b < (sp.r + 3) / 4; ++b) m_emit.push_back(BlockRef{i, b});
    for (int b = 0; b < Npad / kCholStrip; ++b) m_solve.push_back(BlockRef{i, b});
    (void)vh_off;
  }
  // the maps of the tile products, Grams and the verification: XCD-aware tile order (host.h: tile_map_build); the maps of
  // one population come out equal, so a panel of G is consumed next to the same L2 in every product launch of the level
  const bool by_problem = getenv("TADMM_FILTER_XCD") && atoi(getenv("TADMM_FILTER_XCD"));
  auto tile_map = [&](const std::vector<TileProb>& t) { return by_problem ? tile_map_plain(t) : tile_map_build(t); };
  m_stage0 = tile_map(t_stage0);
  m_gram = tile_map(t_gram);
  m_hform = m_gram;
  m_verify = tile_map(t_verify);
  m_cgram = tile_map(t_cgram);
  if (const char* e = getenv("TADMM_FILTER_XCD"); e && atoi(e)) {
    std::vector<double> wk(nf);
    for (int i = 0; i < nf; ++i) wk[i] = specs[i].Npad;          // cost of a block ~ its reduction length
    xcd_by_problem(m_stage0, wk);
    if (atoi(e) > 1) {
      xcd_by_problem(m_gram, wk);
      xcd_by_problem(m_hform, wk);
      xcd_by_problem(m_verify, wk);
      xcd_by_problem(m_solve, wk);
    }
  }
  {   // dgemm3 tiles that read the same slice of G (same problem, same column tile) go to one XCD / one L2
    std::vector<int> tn_of(nf);
    for (int i = 0; i < nf; ++i) tn_of[i] = (specs[i].Npad + 63) / 64;
    xcd_by_key(m_fast, [&](const BlockRef& b) { return b.prob * 3 + b.local % tn_of[b.prob]; });
  }
  fg.prob_off = da.take(probs.size() * sizeof(FiltProb));
  if (img) img->put(fg.prob_off, probs.data(), probs.size() * sizeof(FiltProb));
  auto place = [&](Phase& ph, const std::vector<DgemmDesc>& d, const std::vector<BlockRef>& m) {
    place_phase(ph, da, img, d.data(), d.size() * sizeof(DgemmDesc), nf, m);
  };
  place(fg.stage0, d_stage0, m_stage0);
  place(fg.p1, d_p1, m_stage0);
  place(fg.stage0_f, d_stage0, m_fast);
  place(fg.p1_f, d_p1, m_fast);
  fg.steps_f.assign(d_steps.size(), Phase());
  for (size_t k = 0; k < d_steps.size(); ++k) place(fg.steps_f[k], d_steps[k], m_fast);
  place_phase(fg.gplanes, da, img, d_gp.data(), d_gp.size() * sizeof(GPlaneDesc), nf, m_gp);
  place(fg.axpby, d_axpby, m_axpby);
  fg.steps.assign(d_steps.size(), Phase());
  for (size_t k = 0; k < d_steps.size(); ++k) place(fg.steps[k], d_steps[k], m_stage0);
  place(fg.gramA, d_gramA, m_gram);
  place(fg.gramB, d_gramB, m_gram);
  place(fg.tfinal, d_tfinal, m_stage0);
  place(fg.hform, d_hform, m_hform);
  place(fg.uform, d_uform, m_uform);
  place(fg.verify, d_verify, m_verify);
  fg.cholA_off = da.take(cA.size() * sizeof(CholDesc));
  fg.cholB_off = da.take(cB.size() * sizeof(CholDesc));
  fg.solve_map_off = da.take(m_solve.size() * sizeof(BlockRef));
  fg.solve_blocks = (int)m_solve.size();
  {   // init / emit phases carry no descriptor array of their own (they read FiltProb)
    fg.init.nprob = nf; fg.init.nblocks = (int)m_init.size();
    fg.init.map_off = da.take(m_init.size() * sizeof(BlockRef));
    fg.emit.nprob = nf; fg.emit.nblocks = (int)m_emit.size();
    fg.emit.map_off = da.take(std::max<size_t>(m_emit.size() * sizeof(BlockRef), 16));
  }
  if (fg.ncomp > 0) {
    fg.comp_off = da.take(d_comp.size() * sizeof(CompDesc));
    if (img) img->put(fg.comp_off, d_comp.data(), d_comp.size() * sizeof(CompDesc));
    place_phase(fg.cform, da, img, nullptr, 0, fg.ncomp, m_cform);
    place_phase(fg.cemit, da, img, nullptr, 0, fg.ncomp, m_cemit);
    place_phase(fg.cgram, da, img, d_cgram.data(), d_cgram.size() * sizeof(DgemmDesc), fg.ncomp, m_cgram);
    fg.cchol_off = da.take(c_comp.size() * sizeof(CholDesc));
    fg.csolve_map_off = da.take(m_csolve.size() * sizeof(BlockRef));
    fg.csolve_blocks = (int)m_csolve.size();
    if (img) {
      img->put(fg.cchol_off, c_comp.data(), c_comp.size() * sizeof(CholDesc));
      img->put(fg.csolve_map_off, m_csolve.data(), m_csolve.size() * sizeof(BlockRef));
    }
  }
  if (img) {
    img->put(fg.cholA_off, cA.data(), cA.size() * sizeof(CholDesc));
    img->put(fg.cholB_off, cB.data(), cB.size() * sizeof(CholDesc));
    img->put(fg.solve_map_off, m_solve.data(), m_solve.size() * sizeof(BlockRef));
    img->put(fg.init.map_off, m_init.data(), m_init.size() * sizeof(BlockRef));
    if (!m_emit.empty()) img->put(fg.emit.map_off, m_emit.data(), m_emit.size() * sizeof(BlockRef));
  }
}

static inline FiltParams filter_params(const FilterGroup& fg) {
  FiltParams prm;
  prm.max_degree = fg.max_degree;
  prm.log_target = log(2.0 / 1e-11);
  prm.cond_max = 1e6;
  prm.cond_first = 1e4;
  prm.sin_tol = 1e-5;
  prm.log_precise = log(100.0);
  // complement levels (trailing end of the spectrum: dense, tiny gaps behind the boundary) are held to a tighter target:
  // their verification figure divides the residuals by those gaps and sat at 1e-6 .. 8e-6 with the default
  if (fg.ncomp > 0 && fg.ncomp == fg.nf) prm.log_target = log(2.0 / 1e-13);
  if (const char* e = getenv("TADMM_FILTER_LOG_PRECISE")) prm.log_precise = atof(e);
  if (const char* e = getenv("TADMM_FILTER_EPS")) prm.log_target = log(2.0 / atof(e));
  if (const char* e = getenv("TADMM_FILTER_COND")) prm.cond_max = atof(e);
  if (const char* e = getenv("TADMM_FILTER_COND_FIRST")) prm.cond_first = atof(e);
  if (const char* e = getenv("TADMM_FILTER_SINTOL")) prm.sin_tol = atof(e);
  return prm;
}

// Part 1: filter + orthonormalise + form the Rayleigh-Ritz images.  One host wait per stage ("anyone still
// filtering?", a word per problem in pinned memory).
static inline int filter_run_pre(tadmm_handle h, FilterGroup& fg, char* ws, PollCtx& poll, hipStream_t s, bool debug,
                                 FilterTiming* tm = nullptr) {
  if (fg.nf == 0) return TADMM_OK;
  auto D = [&](size_t off) { return ws + off; };
  const FiltProb* probs = (const FiltProb*)D(fg.prob_off);
  const FiltParams prm = filter_params(fg);
  auto gemm = [&](const Phase& ph) {
    const bool t = tm && tm->on;
    if (t) (void)hipEventRecord(tm->a, s);
    launch_dgemm_nt64((const DgemmDesc*)D(ph.desc_off), (const BlockRef*)D(ph.map_off), ph.nblocks, s, filter_tile_n(), fg.tile_m);
    if (t) {
      float ms = 0.f;
      (void)hipEventRecord(tm->b, s);
      (void)hipEventSynchronize(tm->b);
      (void)hipEventElapsedTime(&ms, tm->a, tm->b);
      tm->gemm_ms += ms; tm->gemm_launches += 1;
    }
  };
  auto gemm3 = [&](const Phase& ph) {
    const bool t = tm && tm->on;
    if (t) (void)hipEventRecord(tm->a, s);
    launch_dgemm3((const DgemmDesc*)D(ph.desc_off), (const BlockRef*)D(ph.map_off), ph.nblocks, s);
    if (t) {
      float ms = 0.f;
      (void)hipEventRecord(tm->b, s);
      (void)hipEventSynchronize(tm->b);
      (void)hipEventElapsedTime(&ms, tm->a, tm->b);
      tm->fast_ms += ms; tm->fast_launches += 1;
    }
  };
  const int nfast = filter_fast_stages(fg);
  if (nfast > 0) launch_gplanes((const GPlaneDesc*)D(fg.gplanes.desc_off), (const BlockRef*)D(fg.gplanes.map_off), fg.gplanes.nblocks, s);
  auto cholqr = [&](const Phase& gram, size_t chol_off) {
    gemm(gram);
    launch_chol_factor((const CholDesc*)D(chol_off), fg.nf, s);
    launch_chol_solve((const CholDesc*)D(chol_off), (const BlockRef*)D(fg.solve_map_off), fg.solve_blocks, s);
  };
  if (fg.ncomp > 0) launch_comp_prepare((const CompDesc*)D(fg.comp_off), fg.ncomp, fg.comp_npad_max, 12, s);
  launch_filt_init(probs, (const BlockRef*)D(fg.init.map_off), fg.init.nblocks, fg.nf, s);
  if (nfast > 0) gemm3(fg.stage0_f); else gemm(fg.stage0);
  cholqr(fg.gramB, fg.cholB_off);
  int smax = 12;
  if (const char* e = getenv("TADMM_FILTER_STAGES")) smax = std::max(1, atoi(e));
  int stages = 0;
  // The stage logic runs on the device (gates); the host only has to stop launching.  A stage's plan already knows
  // whether its problem will want another stage (bit 1 of its verdict); the host reads the verdict of stage st-1 after
  // stage st's product + plan launches are queued, so it never waits for the GPU, and the price of the late read is
  // those two (gated, empty) launches at the end.
  for (int st = 0; st < smax; ++st) {
    const bool fast = st < nfast;
    if (fast) gemm3(fg.p1_f); else gemm(fg.p1);
    int* slot = poll.host + (size_t)(st & 1) * poll.stride;
    launch_filt_plan(probs, fg.nf, prm, st == smax - 1, (fast ? 1 : 0) | (nfast > 0 ? 2 : 0), slot, s);
    HIP_OK(h, hipEventRecord(poll.ev[st & 1], s));
    if (st > 0) {
      HIP_OK(h, hipEventSynchronize(poll.ev[(st - 1) & 1]));
      const int* prev = poll.host + (size_t)((st - 1) & 1) * poll.stride;
      bool ran = false, more = false;
      for (int q = 0; q < fg.nf; ++q) { ran = ran || (prev[1 + q] & 1); more = more || (prev[1 + q] & 2); }
      if (ran) ++stages;
      if (!more) break;            // nobody takes part in stage st: its product and plan above were gated off
    }
    launch_daxpby((const DgemmDesc*)D(fg.axpby.desc_off), (const BlockRef*)D(fg.axpby.map_off), fg.axpby.nblocks, s);
    if (fast) for (const Phase& ph : fg.steps_f) gemm3(ph);
    else for (const Phase& ph : fg.steps) gemm(ph);
    cholqr(fg.gramA, fg.cholA_off);
  }
  fg.last_stages = stages;
  fg.fast_stages = std::max(0, stages - 1);              // next run: every stage but the last one this run needed
  cholqr(fg.gramB, fg.cholB_off);        // second pass: orthonormal to rounding
  launch_filt_flags(probs, fg.nf, s);
  fg.guard_forked = false;
  if (filter_guard_steps() > 0 && !(getenv("TADMM_GUARD_INLINE") && atoi(getenv("TADMM_GUARD_INLINE")))) {
    // the guard reads the final block Q = ring[base] and G only: fork it here
    if (!fg.side) fg.side = std::make_shared<GuardSide>();
    if (fg.side->ok && hipEventRecord(fg.side->fork, s) == hipSuccess &&
        hipStreamWaitEvent(fg.side->st, fg.side->fork, 0) == hipSuccess) {
      launch_filt_guard(probs, fg.nf, fg.npad_max, fg.rp_max, filter_guard_steps(), fg.side->st);
      fg.guard_forked = hipEventRecord(fg.side->join, fg.side->st) == hipSuccess;
    }
  }
  gemm(fg.tfinal);
  gemm(fg.hform);
  if (filter_moments_on()) launch_filt_moments(probs, fg.nf, s);     // H is about to be overwritten by its own eigen-solve
  if (debug) fprintf(stderr, "[tadmm] filter: %d problems, %d stages of <= %d steps, product tiles %d x %d (%d blocks a launch)\n", fg.nf, stages,
                     fg.max_degree, fg.tile_m, filter_tile_n(), fg.p1.nblocks);
  return TADMM_OK;
}

// Part 2 (after the Rayleigh-Ritz solve + eig_norms/sort/extract of the group): Ritz vectors, verification, outputs.
// Returns the number of problems that must take the fallback solve in *nbad.
// `behind_verdict` (optional): queued behind the verdict's event and in front of the host's wait for it, so that the
// stream is not empty while the host wakes up -- the caller's next launch when no problem falls back (the usual case).
// It must be a launch that may simply be repeated after the fallback solve has replaced some of its inputs.
static inline int filter_run_post(tadmm_handle h, FilterGroup& fg, char* ws, PollCtx& poll, hipStream_t s, bool debug,
                                  int* nbad, FilterTiming* tm = nullptr,
                                  const std::function<void()>& behind_verdict = nullptr) {
  *nbad = 0;
  if (fg.nf == 0) return TADMM_OK;
  auto D = [&](size_t off) { return ws + off; };
  const FiltProb* probs = (const FiltProb*)D(fg.prob_off);
  const FiltParams prm = filter_params(fg);
  launch_filt_theta(probs, fg.nf, s);
  if (fg.guard_forked) HIP_OK(h, hipStreamWaitEvent(s, fg.side->join, 0));
  else launch_filt_guard(probs, fg.nf, fg.npad_max, fg.rp_max, filter_guard_steps(), s);     // (no side stream: in line)
  launch_dgemm((const DgemmDesc*)D(fg.uform.desc_off), (const BlockRef*)D(fg.uform.map_off), fg.uform.nblocks, false, s);
  {
    const bool t = tm && tm->on;
    if (t) (void)hipEventRecord(tm->a, s);
    launch_dgemm_nt64((const DgemmDesc*)D(fg.verify.desc_off), (const BlockRef*)D(fg.verify.map_off), fg.verify.nblocks, s, filter_tile_n(), fg.tile_m);
    if (t) {
      float ms = 0.f;
      (void)hipEventRecord(tm->b, s);
      (void)hipEventSynchronize(tm->b);
      (void)hipEventElapsedTime(&ms, tm->a, tm->b);
      tm->gemm_ms += ms; tm->gemm_launches += 1;
    }
  }
  if (fg.ncomp > 0) {     // kept basis = orthonormalised complement of the Ritz vectors; a Cholesky breakdown marks the
    const CompDesc* cd = (const CompDesc*)D(fg.comp_off);        // problem bad BEFORE the verdict is taken
    launch_comp_form(cd, (const BlockRef*)D(fg.cform.map_off), fg.cform.nblocks, s);
    for (int pass = 0; pass < 2; ++pass) {
      launch_dgemm_nt64((const DgemmDesc*)D(fg.cgram.desc_off), (const BlockRef*)D(fg.cgram.map_off), fg.cgram.nblocks, s, filter_tile_n(), fg.tile_m);
      launch_chol_factor((const CholDesc*)D(fg.cchol_off), fg.ncomp, s);
      launch_chol_solve((const CholDesc*)D(fg.cchol_off), (const BlockRef*)D(fg.csolve_map_off), fg.csolve_blocks, s);
    }
  }
  launch_filt_verdict(probs, fg.nf, prm, poll.host, s);
  launch_filt_emit(probs, (const BlockRef*)D(fg.emit.map_off), fg.emit.nblocks, s);
  if (fg.ncomp > 0) launch_comp_emit((const CompDesc*)D(fg.comp_off), (const BlockRef*)D(fg.cemit.map_off), fg.cemit.nblocks, s);
  HIP_OK(h, hipEventRecord(poll.ev[0], s));
  if (behind_verdict) behind_verdict();
  HIP_OK(h, hipEventSynchronize(poll.ev[0]));
  int bad = 0;
  for (int q = 0; q < fg.nf; ++q) bad += poll.host[1 + q] ? 0 : 1;
  *nbad = bad;
  fg.last_bad = bad;
  if (tm && tm->on) {     // executed FLOPs of the timed GEMM launches: products + Grams + projection + residuals
    std::vector<FiltProb> hp(fg.nf);
    if (hipMemcpy(hp.data(), probs, hp.size() * sizeof(FiltProb), hipMemcpyDeviceToHost) == hipSuccess) {
      for (int q = 0; q < fg.nf; ++q) {
        FiltState st;
        if (hipMemcpy(&st, hp[q].st, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) break;
        const double rp = hp[q].rp, np = hp[q].Npad, r32 = hp[q].r32;
        const double stages = st.stage;
        tm->fast_flops += 2.0 * rp * np * np * st.products_fast;     // block products at fp32 accuracy (algorithmic)
        tm->gemm_flops += 2.0 * rp * np * np * (st.products - st.products_fast)   // block products with G in fp64
                          + 2.0 * rp * rp * np * (stages + 2 + 1)    // Gram of every CholQR (+ stage 0, polish) and H
                          + 2.0 * r32 * np * np;                     // residuals of the Ritz pairs
      }
    }
  }
  if (debug) {
    fprintf(stderr, "[tadmm] filter: %d of %d problems fall back to the full solve\n", bad, fg.nf);
    std::vector<FiltProb> hp(fg.nf);
    if (hipMemcpy(hp.data(), probs, hp.size() * sizeof(FiltProb), hipMemcpyDeviceToHost) == hipSuccess) {
      for (int q = 0; q < fg.nf; ++q) {
        FiltState st;
        if (hipMemcpy(&st, hp[q].st, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) break;
        fprintf(stderr, "[tadmm]   filt %2d: N=%d r=%d rp=%d stages=%d logamp=%.1f crit=%.2e bad=%d b=%.4g lr=%.4g l1=%.4g\n", q,
                hp[q].N, hp[q].r, hp[q].rp, st.stage, st.logamp, st.crit, st.bad, st.b, st.lr, st.l1);
      }
    }
  }
  return TADMM_OK;
}

}  // namespace tadmm
