// The TT / SVD projection plan behind tadmm_plan_*: layer geometry, the phase scheduler that turns a set of layers
// into grouped launches, its run, the two-lane split, and the plan-scoped part of the C ABI of include/tadmm.h.
//
// One ADMM projection (reference ADMM.update, admm.py:42-78) over L layers runs as
//     unfold (1 launch)                                   T0 = unfold(W+U)
//     for TT step s = 0 .. max(d)-2, over every layer that has that step:
//         gram_partial, gram_reduce                       G = A A^T | A^T A              (fp64 MFMA)
//         jacobi_init, jacobi_tick x (sweeps*(nb-1))      eigen-decomposition of G       (fp64 MFMA)
//         eig_norms, eig_sort, eig_extract                top-r vectors, sigma
//         gemm                                            T_{s+1} = U_r^T A | core = A V S^-1 (fp32 MFMA)
//     gemm x (chain depth)                                Zmat = core_0 (core_1 (... T_{d-1}))
//     fold_update, resid_reduce                           Z, U += W-Z, ||W-Z||^2
// Layers are independent, so every launch is *grouped*: its blocks are mapped to
// (layer, local block) through a BlockRef table built once at plan creation.  All descriptors live in
// the caller-provided workspace; tadmm_plan_run allocates nothing.
#include "host.h"
#include "filter_host.h"

#include <cmath>
#include <condition_variable>
#include <mutex>
#include <thread>

using namespace tadmm;

// ------------------------------------------------------------------------------------------------
// layer geometry
// ------------------------------------------------------------------------------------------------
struct StepGeom : EigGeom {   // the unfolding of one TT step: m = r_s * n_s rows
  StepGeom() = default;
  explicit StepGeom(const EigGeom& g) : EigGeom(g) {}
  int r = 0;            // kept rank r_{s+1}
  bool skip = false;    // identity step (Z-only mode)
};

struct LayerGeom {
  tadmm_layer_desc desc;
  int64_t numel = 0;
  int O = 0, I = 0, K2 = 1;   // K2 > 1 -> conv permutation
  int d = 0;
  std::vector<StepGeom> steps;  // d-1 entries
};

static int clamp_ranks(tadmm_layer_desc* d) {
  int changed = 0;
  int64_t tail = 1;
  for (int i = 0; i < d->d; ++i) tail *= d->tt_shapes[i];
  // reference ttd.py:15-19: unfolding i is (r_i*n_i) x (tail / n_i ...) with the *already clamped* r_i
  int64_t rest = tail;
  for (int i = 0; i + 1 < d->d; ++i) {
    rest /= d->tt_shapes[i];
    const int64_t m = (int64_t)d->ranks[i] * d->tt_shapes[i];
    const int64_t ns = std::min<int64_t>(m, rest);
    if (ns < d->ranks[i + 1]) { d->ranks[i + 1] = (int32_t)ns; ++changed; }
  }
  return changed;
}

static int build_geom(tadmm_handle h, const tadmm_layer_desc& din, LayerGeom& g) {
  g.desc = din;
  tadmm_layer_desc& d = g.desc;
  if (d.ndim != 2 && d.ndim != 4) CTX_FAIL(h, TADMM_ERR_INVALID, "ndim must be 2 or 4 (got %d)", d.ndim);
  g.numel = 1;
  for (int i = 0; i < d.ndim; ++i) {
    if (d.dims[i] <= 0) CTX_FAIL(h, TADMM_ERR_INVALID, "non-positive dim");
    g.numel *= d.dims[i];
  }
  if (d.kind == TADMM_KIND_TUCKER2) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "Tucker layers use tadmm_tucker_* (not in a TT plan)");
  g.O = (int)d.dims[0];
  g.I = (int)d.dims[1];
  g.K2 = 1;
  if (d.kind == TADMM_KIND_TT_CONV) {
    if (d.ndim != 4) CTX_FAIL(h, TADMM_ERR_INVALID, "TT_CONV needs a 4-D weight");
    g.K2 = (int)(d.dims[2] * d.dims[3]);
  } else if (d.kind == TADMM_KIND_SVD) {
    // admm.py:129-149: squeeze to (O,I); a 4-D weight must be 1x1
    if (d.ndim == 4 && d.dims[2] * d.dims[3] != 1) CTX_FAIL(h, TADMM_ERR_INVALID, "SVD format needs a 1x1 kernel");
    d.d = 2;
    d.tt_shapes[0] = g.O; d.tt_shapes[1] = g.I;
    const int r = d.ranks[0];
    d.ranks[0] = 1; d.ranks[1] = r; d.ranks[2] = 1;
  }
  if (d.d < 2 || d.d > TADMM_MAX_MODES) CTX_FAIL(h, TADMM_ERR_INVALID, "number of TT modes must be in [2,%d]", TADMM_MAX_MODES);
  int64_t prod = 1;
  for (int i = 0; i < d.d; ++i) {
    if (d.tt_shapes[i] <= 0) CTX_FAIL(h, TADMM_ERR_INVALID, "non-positive tt_shape");
    prod *= d.tt_shapes[i];
  }
  if (prod != g.numel) CTX_FAIL(h, TADMM_ERR_INVALID, "prod(tt_shapes)=%lld != numel=%lld", (long long)prod, (long long)g.numel);
  if (d.ranks[0] != 1 || d.ranks[d.d] != 1) CTX_FAIL(h, TADMM_ERR_INVALID, "boundary TT ranks must be 1");
  for (int i = 0; i <= d.d; ++i) if (d.ranks[i] <= 0) CTX_FAIL(h, TADMM_ERR_INVALID, "non-positive rank");
  clamp_ranks(&d);
  g.d = d.d;
  g.steps.resize(d.d - 1);
  int64_t rest = g.numel;
  for (int s = 0; s + 1 < d.d; ++s) {
    StepGeom& st = g.steps[s];
    rest /= d.tt_shapes[s];
    st = StepGeom(eig_geom(d.ranks[s] * d.tt_shapes[s], rest, 64, true));
    st.r = d.ranks[s + 1];
    st.skip = (d.flags & TADMM_FLAG_SKIP_ROTATIONS) && !st.trans && st.r == st.m;
    if (!st.skip && !jacobi_size_supported(st.N))
      CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "TT step %d: eigen-problem of size %d exceeds the Jacobi kernels (max %d)", s,
               st.N, kJacobiMaxN);
  }
  return TADMM_OK;
}

// ------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------
struct StepPlan {
  Phase gram_p, gram_r, proj;
  // The eigen group of the level and, for the problems of it that the filtered eigen-solver serves (filter_host.h),
  // the fallback group: a filtered problem keeps its slot in `main`, where its r' x r' Rayleigh-Ritz problem replaces
  // the full N x N one; the full variants form `fb`.
  EigLayout main, fb;
  size_t off_off = 0, done_off = 0;   // contiguous [neig][3] doubles / [neig] ints
  std::vector<int> layer_of;      // problem -> layer
  FilterGroup fg;
  std::vector<int> filt_of;       // filtered problem -> problem of the level
  size_t skip_off = 0;            // [neig] ints: eig group (set for filtered problems that went bad)
  size_t fb_skip_off = 0;         // [nf] ints: fallback group (1 = filtered result accepted)
  // every projection of the level has beta == 0 and an output that overlaps neither operand: a second launch overwrites
  // the first, so the launch may be queued before the filter's verdict is known and repeated after a fallback solve
  bool proj_repeatable = false;
};

// the element range a strided M x N float matrix touches
static inline void gemm_span(const float* p, int64_t rows, int64_t cols, int64_t rs, int64_t cs, const float** lo, const float** hi) {
  *lo = p;
  *hi = p + (rows - 1) * rs + (cols - 1) * cs + 1;
}
static inline bool gemm_repeatable(const GemmDesc& g) {
  if (g.beta != 0.f || g.M <= 0 || g.N <= 0 || g.K <= 0) return false;
  if (g.a_rs < 0 || g.a_cs < 0 || g.b_rs < 0 || g.b_cs < 0 || g.c_rs < 0 || g.c_cs < 0) return false;
  const float *c0, *c1, *a0, *a1, *b0, *b1;
  gemm_span(g.C, g.M, g.N, g.c_rs, g.c_cs, &c0, &c1);
  gemm_span(g.A, g.M, g.K, g.a_rs, g.a_cs, &a0, &a1);
  gemm_span(g.B, g.K, g.N, g.b_rs, g.b_cs, &b0, &b1);
  return (c1 <= a0 || a1 <= c0) && (c1 <= b0 || b1 <= c0);
}

struct tadmm_plan_s {
  tadmm_handle h = nullptr;
  int n = 0;
  std::vector<LayerGeom> layers;
  char* ws = nullptr;
  size_t ws_bytes = 0;
  Phase unfold, fold;
  size_t sweep_desc_off = 0;
  size_t resid_partial_off = 0;
  int total_sweep_blocks = 0;
  std::vector<StepPlan> steps;
  std::vector<Phase> recon;       // chain levels
  // per layer / step bookkeeping for queries
  std::vector<std::vector<size_t>> sigma_off;   // [layer][step] -> offset of sigma doubles (or SIZE_MAX)
  // timing
  bool timing = false;
  hipEvent_t ev[16];
  bool ev_made = false;
  PollCtx poll;                   // pipelined convergence poll (host.h)
  double last_ms[8] = {0};
  int last_sweeps = 0;
  double tol = 1e-9;
  bool debug = false;
  int max_global_sweeps = 40;
  // filtered eigen-solver statistics of the last run
  int filt_problems = 0, filt_fallbacks = 0, filt_stages = 0;
  FilterTiming ftm;
  JacobiTiming jtm;
  const int32_t* resid_index = nullptr;   // device map local layer -> slot of the caller's residual array (lanes)
  struct Lanes* lanes = nullptr;          // set on a parent plan that runs its layers as two concurrent lanes
};

// ------------------------------------------------------------------------------------------------
// Lanes.  One eigen-solve is a chain of dependent launches, and the grouped launches of a plan put the short chains
// of most layers behind the few long ones (ResNet-50: the 3x3 kernels of layer3/layer4 need ~3/4 of the launches).
// A plan whose table has both kinds is therefore run as TWO sub-plans on two streams of the device: lane 0 holds the
// long chains and runs on a high-priority stream at the pace it would have alone, lane 1 (everything else) fills the
// CUs those launches leave idle.  Each sub-plan polls its own convergence words, so lane 1 is driven by a worker thread
// that lives as long as the plan.  Measured on MI355X, ResNet-50 table: 10.2 ms as one plan, 8.6 ms as two lanes.
// ------------------------------------------------------------------------------------------------
struct Lanes {
  tadmm_plan_s* sub[2] = {nullptr, nullptr};
  std::vector<int> lane_of, local_of;
  hipStream_t st[2] = {nullptr, nullptr};
  hipEvent_t ev_begin = nullptr, ev_end[2] = {nullptr, nullptr};
  std::thread worker;
  std::mutex mu;
  std::condition_variable cv;
  int job = 0;                 // 0 idle, 1 run posted, 2 quit
  bool done = true;
  int a_update_u = 0, a_use_u = 0;
  double* a_resid = nullptr;
  int rc = 0;
};

namespace {

struct Built {
  // per layer buffers (offsets in the arena)
  std::vector<size_t> tbuf0, tbuf1, xt, gpart, vs, cores_ws;
};

}  // namespace

// Lays out the whole plan.  If `img` is null only sizes are computed.
static int layout_plan(tadmm_plan_s* P, const float* const* W, float* const* U, float* const* Z, float* const* cores,
                       HostImage* img, size_t desc_region, size_t* desc_bytes, size_t* total_bytes) {
  tadmm_handle h = P->h;
  const int n = P->n;
  Arena da;                    // descriptors + block maps: [0, desc_region)
  Arena ar;                    // data buffers: [desc_region, ...)
  ar.off = desc_region;
  auto dev = [&](size_t off) -> char* { return P->ws ? P->ws + off : nullptr; };

  // ---- data buffers per layer ----
  std::vector<size_t> tb0(n), tb1(n), xt(n), gp(n), vs(n), cw(n);
  std::vector<std::vector<size_t>> core_off(n);     // float offsets (bytes) of core_s inside arena or user buf
  std::vector<std::vector<float*>> core_ptr(n);     // device pointers of cores (incl. last = T_{d-1} when user buf)
  P->sigma_off.assign(n, {});
  for (int l = 0; l < n; ++l) {
    const LayerGeom& g = P->layers[l];
    tb0[l] = ar.take((size_t)g.numel * 4);
    tb1[l] = ar.take((size_t)g.numel * 4);
    size_t xtb = 0, gpb = 0, vsb = 0, cb = 0;
    for (const StepGeom& st : g.steps) {
      if (st.skip) continue;
      xtb = std::max(xtb, (size_t)st.Npad * st.ld * 8);
      gpb = std::max(gpb, (size_t)st.ksplit * (st.nt * (st.nt + 1) / 2) * 1024 * 8);
      if (st.trans) vsb = std::max(vsb, (size_t)st.N * st.r * 4);
      cb += align_up((size_t)st.m * st.r * 4, 256);
    }
    xt[l] = ar.take(xtb ? xtb : 256);
    gp[l] = ar.take(gpb ? gpb : 256);
    vs[l] = ar.take(vsb ? vsb : 256);
    cw[l] = ar.take(cb ? cb : 256);
    P->sigma_off[l].assign(g.steps.size(), (size_t)-1);
  }

  // ---- sweep descriptors (unfold / fold_update) ----
  std::vector<SweepDesc> sd(n);
  std::vector<BlockRef> smap;
  // T pointer tracking: cur[l] = buffer holding T_s
  std::vector<float*> cur(n), other(n);
  for (int l = 0; l < n; ++l) {
    const LayerGeom& g = P->layers[l];
    SweepDesc& s = sd[l];
    memset(&s, 0, sizeof s);
    s.W = W ? W[l] : nullptr; s.U = U ? U[l] : nullptr; s.Z = Z ? Z[l] : nullptr;
    s.T0 = (float*)dev(tb0[l]);
    s.O = g.O; s.I = g.I; s.K2 = g.K2;
    s.numel = g.numel;
    if (g.K2 > 1) {
      int ich = std::min(g.I, 512);
      while ((int64_t)g.K2 * (ich + 4) > 12288 && ich > 1) ich /= 2;
      s.ichunk = ich;
      s.nchunk = (g.I + ich - 1) / ich;
      s.nblk = g.O * s.nchunk;
    } else {
      s.ichunk = 8192;
      s.nchunk = (int)((g.numel + s.ichunk - 1) / s.ichunk);
      s.nblk = s.nchunk;
    }
    s.blk_begin = (int)smap.size();
    for (int b = 0; b < s.nblk; ++b) smap.push_back(BlockRef{l, b});
    cur[l] = (float*)dev(tb0[l]);
    other[l] = (float*)dev(tb1[l]);
  }
  P->total_sweep_blocks = (int)smap.size();
  P->resid_partial_off = ar.take((size_t)smap.size() * 8);

  // ---- TT steps ----
  // Levels: layer l runs its TT step s at level s + lvl_off[l].  The longest chains fix the number of
  // levels; shorter chains are shifted so that their eigen-solves share a level with problems of at
  // least their size (a level costs ~ (nb_max - 1) ticks per sweep whatever its population), on the
  // least populated such level -- e.g. ResNet-50: the 1x1 convs' single N=256/512 solve runs beside the
  // 3x3 convs' N=480/512 steps instead of beside their N<=32 first step.
  int maxsteps = 0;
  for (const LayerGeom& g : P->layers) maxsteps = std::max(maxsteps, (int)g.steps.size());
  std::vector<int> lvl_off(n, 0);
  {
    std::vector<int> lvl_nb(maxsteps, 0);
    std::vector<long> lvl_wgs(maxsteps, 0);
    std::vector<int> order(n);
    for (int l = 0; l < n; ++l) order[l] = l;
    auto heavy = [&](int l) { int m = 0; for (const StepGeom& st : P->layers[l].steps) if (!st.skip) m = std::max(m, st.nb); return m; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
      const size_t ca = P->layers[a].steps.size(), cb = P->layers[b].steps.size();
      if (ca != cb) return ca > cb;
      return heavy(a) > heavy(b);
    });
    for (int l : order) {
      const LayerGeom& g = P->layers[l];
      const int len = (int)g.steps.size();
      int best = 0; double best_cost = 1e300;
      for (int off = 0; off + len <= maxsteps; ++off) {
        // cost = added ticks (levels whose nb_max grows) first, then population of the touched levels
        double cost = 0;
        for (int s = 0; s < len; ++s) {
          if (g.steps[s].skip) continue;
          const int lv = off + s;
          cost += 1e6 * std::max(0, g.steps[s].nb - lvl_nb[lv]) + (double)lvl_wgs[lv] * g.steps[s].nb;
        }
        if (cost < best_cost) { best_cost = cost; best = off; }
      }
      lvl_off[l] = best;
      for (int s = 0; s < len; ++s) {
        if (g.steps[s].skip) continue;
        lvl_nb[best + s] = std::max(lvl_nb[best + s], g.steps[s].nb);
        lvl_wgs[best + s] += g.steps[s].nb / 2;
      }
    }
  }
  P->steps.assign(maxsteps, StepPlan());
  // recon chain bookkeeping: for each layer the list of (core ptr, m, r, cols) of non-skipped steps
  struct RecOp { const float* core; int m, r; int64_t cols; };
  std::vector<std::vector<RecOp>> recops(n);
  std::vector<const float*> lastT(n, nullptr);

  for (int lev = 0; lev < maxsteps; ++lev) {
    StepPlan& sp = P->steps[lev];
    std::vector<GramDesc> gd;
    std::vector<EigDesc> ed;
    std::vector<GemmDesc> pd;
    std::vector<BlockRef> m_gp, m_gr, m_proj;
    std::vector<int> gp_cost;     // per problem: K chunk of its Gram workgroups (longest first in the block map)
    std::vector<int> layer_of;
    for (int l = 0; l < n; ++l) {
      const LayerGeom& g = P->layers[l];
      const int s = lev - lvl_off[l];
      if (s < 0 || s >= (int)g.steps.size()) continue;
      const StepGeom& st = g.steps[s];
      if (st.skip) {   // identity: T_{s+1} aliases T_s, no core
        if (cores && cores[l]) CTX_FAIL(h, TADMM_ERR_INVALID, "TADMM_FLAG_SKIP_ROTATIONS is incompatible with cores output");
        continue;
      }
      layer_of.push_back(l);
    }
    const int neig = (int)layer_of.size();
    sp.layer_of = layer_of;
    sp.off_off = ar.take((size_t)std::max(1, neig) * 3 * 8);
    sp.done_off = ar.take((size_t)std::max(1, neig) * 4);
    sp.main.prev_off = ar.take((size_t)std::max(1, neig) * 8);
    sp.skip_off = ar.take((size_t)std::max(1, neig) * 4);
    std::vector<FilterSpec> fspecs;
    sp.filt_of.clear();
    for (int p = 0; p < neig; ++p) {
      const int l = layer_of[p];
      const LayerGeom& g = P->layers[l];
      const int s = lev - lvl_off[l];
      const StepGeom& st = g.steps[s];
      const bool last_step = (s + 2 == g.d);
      // core storage
      float* core_dev;
      float* tnext;
      if (cores && cores[l]) {
        size_t off = 0;
        for (int j = 0; j < s; ++j) off += (size_t)g.steps[j].m * g.steps[j].r;
        core_dev = cores[l] + off;
        tnext = last_step ? (cores[l] + off + (size_t)st.m * st.r) : other[l];
      } else {
        size_t off = 0;
        for (int j = 0; j < s; ++j) if (!g.steps[j].skip) off += align_up((size_t)g.steps[j].m * g.steps[j].r * 4, 256);
        core_dev = (float*)dev(cw[l] + off);
        tnext = other[l];
      }
      const float* Tin = cur[l];
      // Gram
      GramDesc gdsc;
      memset(&gdsc, 0, sizeof gdsc);
      gdsc.A = Tin; gdsc.m = st.m; gdsc.n = (int)st.cols; gdsc.trans = st.trans ? 1 : 0;
      gdsc.N = st.N; gdsc.K = st.trans ? st.m : (int)st.cols;
      gdsc.nt = st.nt; gdsc.ksplit = st.ksplit; gdsc.kchunk = st.kchunk;
      gdsc.partial = (double*)dev(gp[l]);
      gdsc.G = (double*)dev(xt[l]);
      gdsc.Npad = st.Npad; gdsc.ld = st.ld;
      const int ntp = st.nt * (st.nt + 1) / 2;
      for (int b = 0; b < st.ksplit * ntp; ++b) m_gp.push_back(BlockRef{p, b});
      gp_cost.push_back(st.kchunk);
      const int64_t gtot = (int64_t)st.Npad * st.ld;
      if (st.ksplit > 1)
        for (int b = 0; b < (int)((gtot + 1023) / 1024); ++b) m_gr.push_back(BlockRef{p, b});
      gd.push_back(gdsc);
      // eig
      EigDesc e;
      memset(&e, 0, sizeof e);
      e.XT = (double*)dev(xt[l]);
      e.N = st.N; e.Npad = st.Npad; e.ld = st.ld; e.nb = st.nb;
      e.off = (double*)dev(sp.off_off) + 3 * p;
      e.done = (int32_t*)dev(sp.done_off) + p;
      const size_t lam_off = ar.take((size_t)st.Npad * 8);
      const size_t ord_off = ar.take((size_t)st.Npad * 4);
      const size_t sig_off = ar.take((size_t)st.r * 8);
      const size_t sblk_off = ar.take((size_t)(st.Npad / 16) * 256 * 8);
      P->sigma_off[l][s] = sig_off;
      e.lam = (double*)dev(lam_off);
      e.order = (int32_t*)dev(ord_off);
      e.sigma = (double*)dev(sig_off);
      e.r = st.r;
      e.mode = st.trans ? 1 : 0;
      e.out_a = st.trans ? (float*)dev(vs[l]) : core_dev;
      e.out_b = st.trans ? tnext : nullptr;
      e.evec_out = nullptr;
      e.sblk = (double*)dev(sblk_off);
      ed.push_back(e);
      const bool zonly = (g.desc.flags & TADMM_FLAG_SKIP_ROTATIONS) && !(cores && cores[l]);
      if (const int rp = filter_block_size(st.N, st.r)) {
        FilterSpec fs;
        fs.N = st.N; fs.Npad = st.Npad; fs.ldg = st.ld; fs.r = st.r; fs.rp = rp;
        fs.G = e.XT; fs.mode = e.mode; fs.ldo = e.ldo; fs.out_a = e.out_a; fs.out_b = e.out_b; fs.sigma = e.sigma;
        fs.skip_slot = (int32_t*)dev(sp.skip_off) + p;
        fspecs.push_back(fs);
        sp.filt_of.push_back(p);
      } else if (const int rpc = complement_block_size(st.N, st.r, st.trans, zonly)) {
        // complement route (complement.hip): the filter runs on the reflected image G' for the N - r DISCARDED vectors
        FilterSpec fs;
        const int kdis = st.N - st.r;
        fs.N = st.N; fs.Npad = st.Npad; fs.ldg = st.ld; fs.r = kdis; fs.rp = rpc;
        fs.G = (const double*)dev(ar.take((size_t)st.Npad * st.ld * 8));
        fs.g_orig = e.XT; fs.comp_r = st.r; fs.sigma_layer = e.sigma;
        fs.mode = 4; fs.ldo = e.ldo; fs.out_a = e.out_a; fs.out_b = nullptr;
        fs.sigma = (double*)dev(ar.take((size_t)align_up(kdis, 32) * 8));      // (Ritz values of G': scratch)
        fs.skip_slot = (int32_t*)dev(sp.skip_off) + p;
        fspecs.push_back(fs);
        sp.filt_of.push_back(p);
      }
      // projection GEMM
      GemmDesc pg;
      memset(&pg, 0, sizeof pg);
      pg.alpha = 1.f; pg.beta = 0.f;
      if (!st.trans) {   // T_{s+1}[r x cols] = Uf^T[r x m] * A[m x cols]
        pg.A = core_dev; pg.a_rs = 1; pg.a_cs = st.r;
        pg.B = Tin; pg.b_rs = st.cols; pg.b_cs = 1;
        pg.C = tnext; pg.c_rs = st.cols; pg.c_cs = 1;
        pg.M = st.r; pg.N = (int)st.cols; pg.K = st.m;
      } else {           // core[m x r] = A[m x n] * Vs[n x r]
        pg.A = Tin; pg.a_rs = st.cols; pg.a_cs = 1;
        pg.B = (const float*)dev(vs[l]); pg.b_rs = st.r; pg.b_cs = 1;
        pg.C = core_dev; pg.c_rs = st.r; pg.c_cs = 1;
        pg.M = st.m; pg.N = st.r; pg.K = (int)st.cols;
      }
      gemm_tiles(pg, p, m_proj);
      pd.push_back(pg);
      recops[l].push_back(RecOp{core_dev, st.m, st.r, st.cols});
      // advance the T chain
      if (tnext == other[l]) std::swap(cur[l], other[l]);
      else { cur[l] = tnext; }
    }
    std::stable_sort(m_gp.begin(), m_gp.end(),
                     [&](const BlockRef& a, const BlockRef& b) { return gp_cost[a.prob] > gp_cost[b.prob]; });
    place_phase(sp.gram_p, da, img, gd.data(), gd.size() * sizeof(GramDesc), neig, m_gp);
    place_map_like(sp.gram_r, sp.gram_p, da, img, m_gr);
    // ---- filtered problems: Rayleigh-Ritz problem in the eig group, full problem in the fallback group ----
    std::vector<EigDesc> ed_fb;
    {
      const int nf = (int)fspecs.size();
      sp.fb_skip_off = ar.take((size_t)std::max(1, nf) * 4);
      for (int i = 0; i < nf; ++i) fspecs[i].fb_skip = (int32_t*)dev(sp.fb_skip_off) + i;
      std::vector<FilterRR> rr;
      filter_layout(sp.fg, fspecs, da, ar, dev, img, rr);
      for (int i = 0; i < nf; ++i) {
        const int p = sp.filt_of[i];
        ed_fb.push_back(ed[p]);
        // the fallback problem needs convergence words of its own (the group's are used by the Rayleigh-Ritz solve)
        ed_fb.back().off = (double*)dev(ar.take(3 * 8));
        ed_fb.back().done = (int32_t*)dev(ar.take(4));
        EigDesc e = rr[i].desc;
        e.off = ed[p].off; e.done = ed[p].done;
        ed[p] = e;
      }
    }
    if (const int rc = build_eig_layout(h, sp.main, ed, true, da, img)) return rc;
    sp.fb.prev_off = ar.take((size_t)std::max<size_t>(1, ed_fb.size()) * 8);
    if (const int rc = build_eig_layout(h, sp.fb, ed_fb, true, da, img)) return rc;
    place_phase(sp.proj, da, img, pd.data(), pd.size() * sizeof(GemmDesc), neig, m_proj);
    sp.proj_repeatable = !pd.empty();
    for (const GemmDesc& g : pd) sp.proj_repeatable = sp.proj_repeatable && gemm_repeatable(g);
  }

  // ---- reconstruction chain, right to left:  R = T_{d-1};  R <- core_s * R ----
  for (int l = 0; l < n; ++l) lastT[l] = cur[l];
  size_t maxchain = 0;
  for (int l = 0; l < n; ++l) maxchain = std::max(maxchain, recops[l].size());
  P->recon.assign(maxchain, Phase());
  std::vector<const float*> rcur(n);
  std::vector<float*> rfree(n);
  for (int l = 0; l < n; ++l) {
    rcur[l] = lastT[l];
    // the "other" ping-pong buffer is free; if T_{d-1} lives in the user's cores buffer both are free
    float* b0 = (float*)dev(tb0[l]);
    float* b1 = (float*)dev(tb1[l]);
    rfree[l] = (rcur[l] == b0) ? b1 : b0;
  }
  for (size_t lev = 0; lev < maxchain; ++lev) {
    std::vector<GemmDesc> rd;
    std::vector<BlockRef> rmap;
    for (int l = 0; l < n; ++l) {
      if (lev >= recops[l].size()) continue;
      const RecOp& op = recops[l][recops[l].size() - 1 - lev];
      GemmDesc g;
      memset(&g, 0, sizeof g);
      g.alpha = 1.f;
      g.A = op.core; g.a_rs = op.r; g.a_cs = 1;
      g.B = rcur[l]; g.b_rs = op.cols; g.b_cs = 1;
      g.C = rfree[l]; g.c_rs = op.cols; g.c_cs = 1;
      g.M = op.m; g.N = (int)op.cols; g.K = op.r;
      gemm_tiles(g, (int)rd.size(), rmap);
      rd.push_back(g);
      // ping-pong: the old input buffer becomes free unless it is a user buffer
      float* b0 = (float*)dev(tb0[l]);
      float* b1 = (float*)dev(tb1[l]);
      const float* produced = rfree[l];
      rfree[l] = (produced == b0) ? b1 : b0;
      rcur[l] = produced;
    }
    place_phase(P->recon[lev], da, img, rd.data(), rd.size() * sizeof(GemmDesc), (int)rd.size(), rmap);
  }
  for (int l = 0; l < n; ++l) sd[l].Zmat = rcur[l];

  // ---- sweep phase descriptors ----
  P->sweep_desc_off = da.take(sd.size() * sizeof(SweepDesc));
  P->unfold.desc_off = P->sweep_desc_off;
  P->unfold.nprob = n;
  P->unfold.nblocks = (int)smap.size();
  P->unfold.map_off = da.take(smap.size() * sizeof(BlockRef));
  P->fold = P->unfold;
  if (img) {
    img->put(P->sweep_desc_off, sd.data(), sd.size() * sizeof(SweepDesc));
    img->put(P->unfold.map_off, smap.data(), smap.size() * sizeof(BlockRef));
  }
  *desc_bytes = align_up(da.off, 4096);
  *total_bytes = align_up(ar.off, 256);   // when desc_region == 0 this is the data size alone
  return TADMM_OK;
}

// a getter of four per-plan figures on a two-lane plan: the sum over the lanes (last slot: their maximum, if asked)
template <class T, class Get>
static bool sum_over_lanes(tadmm_plan p, T out[4], Get get, bool last_is_max = false) {
  if (!p->lanes) return false;
  T a[4], b[4];
  get(p->lanes->sub[0], a);
  get(p->lanes->sub[1], b);
  for (int i = 0; i < 4; ++i) out[i] = a[i] + b[i];
  if (last_is_max) out[3] = std::max(a[3], b[3]);
  return true;
}

// ------------------------------------------------------------------------------------------------
// plan-scoped C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int tadmm_tt_clamp_ranks(tadmm_layer_desc* desc) {
  if (!desc || desc->d < 2 || desc->d > TADMM_MAX_MODES) return TADMM_ERR_INVALID;
  return clamp_ranks(desc);
}

static int single_workspace_bytes(tadmm_handle h, int n_layers, const tadmm_layer_desc* descs, size_t* bytes) {
  if (!h || !descs || !bytes || n_layers <= 0) return TADMM_ERR_INVALID;
  tadmm_plan_s P;
  P.h = h;
  P.n = n_layers;
  P.layers.resize(n_layers);
  for (int l = 0; l < n_layers; ++l) {
    int rc = build_geom(h, descs[l], P.layers[l]);
    if (rc) return rc;
  }
  P.ws = nullptr;
  size_t db = 0, data = 0;
  int rc = layout_plan(&P, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &db, &data);
  if (rc) return rc;
  *bytes = db + data + 4096;
  return TADMM_OK;
}

static int single_create(tadmm_handle h, int n_layers, const tadmm_layer_desc* descs, const float* const* W,
                         float* const* U, float* const* Z, float* const* cores, void* workspace, size_t workspace_bytes,
                         tadmm_plan* out) {
  DeviceGuard device_guard(h);
  if (!h || !descs || !W || !U || !Z || !workspace || !out || n_layers <= 0) return TADMM_ERR_INVALID;
  tadmm_plan_s* P = new tadmm_plan_s();
  P->h = h;
  P->n = n_layers;
  P->layers.resize(n_layers);
  for (int l = 0; l < n_layers; ++l) {
    int rc = build_geom(h, descs[l], P->layers[l]);
    if (rc) { delete P; return rc; }
  }
  P->ws = (char*)workspace;
  P->ws_bytes = workspace_bytes;
  HostImage img;
  size_t need = 0, db = 0, data0 = 0;
  int rc = layout_plan(P, W, U, Z, cores, nullptr, 0, &db, &data0);      // pass 1: size of the descriptor region
  if (rc) { delete P; return rc; }
  rc = layout_plan(P, W, U, Z, cores, &img, db, &db, &need);             // pass 2: real offsets
  if (rc) { delete P; return rc; }
  if (need > workspace_bytes) {
    delete P;
    CTX_FAIL(h, TADMM_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
  }
  // descriptors were written at their arena offsets in the host image; upload the covered range
  if (!img.bytes.empty()) {
    hipError_t e = hipMemcpy(P->ws, img.bytes.data(), img.bytes.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { delete P; CTX_FAIL(h, TADMM_ERR_HIP, "descriptor upload failed: %s", hipGetErrorString(e)); }
  }
  for (const StepPlan& sp : P->steps) {      // Rayleigh-Ritz images / skip words start from zero
    hipError_t e = hipSuccess;
    if (sp.fg.zero_bytes) e = hipMemset(P->ws + sp.fg.zero_off, 0, sp.fg.zero_bytes);
    if (e == hipSuccess) e = hipMemset(P->ws + sp.skip_off, 0, (size_t)std::max(1, sp.main.neig) * 4);
    if (e == hipSuccess) e = hipMemset(P->ws + sp.fb_skip_off, 0, (size_t)std::max(1, sp.fg.nf) * 4);
    if (e != hipSuccess) { delete P; CTX_FAIL(h, TADMM_ERR_HIP, "workspace clear failed: %s", hipGetErrorString(e)); }
  }
  if (const char* e = getenv("TADMM_JACOBI_TOL")) P->tol = atof(e);
  if (getenv("TADMM_DEBUG")) P->debug = true;
  size_t maxe = 1;
  for (const StepPlan& sp : P->steps) maxe = std::max<size_t>(maxe, sp.main.neig);
  {
    const hipError_t e = P->poll.create(maxe);
    if (e != hipSuccess) { delete P; CTX_FAIL(h, TADMM_ERR_HIP, "poll buffers: %s", hipGetErrorString(e)); }
  }
  *out = P;
  return TADMM_OK;
}

static int single_run(tadmm_plan p, int update_u, int use_u, double* resid_sq_dev, void* stream_);

// ---- lanes: split rule, creation, the worker of lane 1 ----
// modelled latency (us) of one eigen-problem alone on the device; mirrors tadmm/sched.py problem_latency_us
static double step_latency_us_full_or_filtered(int N, int r) {
  const int npad = (int)align_up(N, 32);
  if (npad <= 64) return 100.0;
  const int rp = filter_block_size(N, r);
  if (rp) return 7.0 * (8 * 35.0 + 170.0) + (rp / 16 - 1) * 7.0 * (9.0 + 0.02 * (double)align_up(rp, 128));
  return (npad / 16 - 1) * 11.0 * (9.0 + 0.02 * (double)align_up(N, 128));
}

// lane 0 = layers whose chain of eigen-solves is at least `thr` of the longest; lane 1 = the rest.  One lane (return
// false) when either side would be (nearly) empty, when asked to (TADMM_LANES=1) or for small tables.
static bool lane_split(tadmm_handle h, int n, const tadmm_layer_desc* descs, std::vector<int>& lane_of) {
  lane_of.assign(n, 0);
  if (const char* e = getenv("TADMM_LANES")) if (atoi(e) == 1) return false;
  if (n < 4) return false;
  double thr = 0.6;
  if (const char* e = getenv("TADMM_LANE_THRESHOLD")) thr = atof(e);
  std::vector<double> lat(n, 0.0);
  std::vector<int> nfilt(n, 0);
  double lmax = 0.0;
  for (int l = 0; l < n; ++l) {
    LayerGeom g;
    if (build_geom(h, descs[l], g)) return false;
    for (const StepGeom& st : g.steps)
      if (!st.skip) {
        const bool zonly = (descs[l].flags & TADMM_FLAG_SKIP_ROTATIONS) != 0;
        const bool comp = !filter_block_size(st.N, st.r) && complement_block_size(st.N, st.r, st.trans, zonly) > 0;
        lat[l] += comp ? 1500.0 : step_latency_us_full_or_filtered(st.N, st.r);
        nfilt[l] += (filter_block_size(st.N, st.r) > 0 || comp) ? 1 : 0;
      }
    lmax = std::max(lmax, lat[l]);
  }
  int n0 = 0;
  double t1 = 0.0;
  // A level runs its filter stages BEFORE the Jacobi group that holds the Rayleigh-Ritz problems AND the level's full
  // solves (single_run), so a long chain of full solves sharing a plan with filtered chains waits for their filters at
  // every level (ResNet-18: layer4.0.conv1, N = 480 keep 236, beside the three filtered layer4 chains).  When the long
  // chains are of both kinds, the unfiltered ones go to lane 1: their tournaments then run beside the filter stages.
  bool long_filt = false, long_full = false;
  for (int l = 0; l < n; ++l)
    if (lat[l] >= thr * lmax) { if (nfilt[l] > 0) long_filt = true; else long_full = true; }
  const bool mixed = long_filt && long_full;
  // Long chains of FULL solves beside filtered / complement chains of any length (DeiT-small: the N = 384 solves of qkv /
  // fc1 beside the complement route of proj / fc2): a filtered chain is a few hundred SMALL dependent launches, a full
  // tournament a few hundred launches that fill the chip.  The small ones go to lane 0 -- the high-priority stream --
  // where each of them finds CUs at once and delays the big launches by next to nothing; as the low-priority lane they
  // waited for a whole tick launch every time (measured: 11.3 ms instead of 10.0 ms without the route).
  bool any_filt = false;
  for (int l = 0; l < n; ++l) any_filt = any_filt || nfilt[l] > 0;
  const bool by_kind = long_full && any_filt && !long_filt;
  for (int l = 0; l < n; ++l) {
    if (by_kind) lane_of[l] = nfilt[l] > 0 ? 0 : 1;
    else lane_of[l] = (lat[l] >= thr * lmax && !(mixed && nfilt[l] == 0)) ? 0 : 1;
  }
  if (by_kind) {
    // a tournament launch of lane 1 holds Npad / 32 workgroups per problem, one per CU (128 KiB of LDS each): one more
    // than the device has CUs and every tick of the lane takes two rounds.  The excess (shortest chains first) rides in
    // lane 0 behind that lane's filter stages.
    int ncu = 256;
    if (h) { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, h->device) == hipSuccess && pr.multiProcessorCount > 0) ncu = pr.multiProcessorCount; }
    std::vector<int> wgs(n, 0);
    long total = 0;
    for (int l = 0; l < n; ++l) {
      if (lane_of[l] != 1) continue;
      LayerGeom g;
      if (build_geom(h, descs[l], g)) return false;
      for (const StepGeom& st : g.steps) if (!st.skip) wgs[l] = std::max(wgs[l], st.Npad / 32);
      total += wgs[l];
    }
    std::vector<int> order;
    for (int l = 0; l < n; ++l) if (lane_of[l] == 1 && wgs[l] >= 4) order.push_back(l);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lat[a] < lat[b]; });
    for (int l : order) {
      if (total <= ncu) break;
      lane_of[l] = 0;
      total -= wgs[l];
    }
  }
  for (int l = 0; l < n; ++l) { if (lane_of[l] == 0) ++n0; else t1 += lat[l]; }
  if (n0 == 0 || n - n0 < 2 || t1 < 0.2 * lmax) {
    // no short side to hide behind the long chains.  A big table of like layers (DeiT-small: 48 layers, every chain
    // within 0.6 of the longest) still gains from two half tables on two streams -- one lane's GEMM phases fill the gaps
    // of the other's eigen-solves (12.3 -> 10.9 ms); small or short tables stay in one lane.
    if (n >= 16 && n0 >= n - 1 && lmax >= 2000.0) {
      for (int l = 0; l < n; ++l) lane_of[l] = l < n / 2 ? 0 : 1;
      return true;
    }
    lane_of.assign(n, 0);
    return false;
  }
  return true;
}

static void lane_worker(tadmm_plan_s* parent) {
  Lanes* L = parent->lanes;
  (void)hipSetDevice(parent->h->device);
  for (;;) {
    std::unique_lock<std::mutex> lk(L->mu);
    L->cv.wait(lk, [&] { return L->job != 0; });
    if (L->job == 2) return;
    const int uu = L->a_update_u, us = L->a_use_u;
    double* resid = L->a_resid;
    lk.unlock();
    const int rc = single_run(L->sub[1], uu, us, resid, L->st[1]);
    lk.lock();
    L->rc = rc;
    L->job = 0;
    L->done = true;
    lk.unlock();
    L->cv.notify_all();
  }
}

static void lanes_destroy(tadmm_plan_s* p);

int tadmm_plan_workspace_bytes(tadmm_handle h, int n_layers, const tadmm_layer_desc* descs, size_t* bytes) {
  if (!h || !descs || !bytes || n_layers <= 0) return TADMM_ERR_INVALID;
  std::vector<int> lane_of;
  if (!lane_split(h, n_layers, descs, lane_of)) return single_workspace_bytes(h, n_layers, descs, bytes);
  size_t total = 0;
  for (int lane = 0; lane < 2; ++lane) {
    std::vector<tadmm_layer_desc> sub;
    for (int l = 0; l < n_layers; ++l) if (lane_of[l] == lane) sub.push_back(descs[l]);
    size_t b = 0;
    const int rc = single_workspace_bytes(h, (int)sub.size(), sub.data(), &b);
    if (rc) return rc;
    total += align_up(b, 4096);
  }
  *bytes = total + align_up((size_t)n_layers * 4, 4096);
  return TADMM_OK;
}

int tadmm_plan_create(tadmm_handle h, int n_layers, const tadmm_layer_desc* descs, const float* const* W,
                      float* const* U, float* const* Z, float* const* cores, void* workspace, size_t workspace_bytes,
                      tadmm_plan* out) {
  DeviceGuard device_guard(h);
  if (!h || !descs || !W || !U || !Z || !workspace || !out || n_layers <= 0) return TADMM_ERR_INVALID;
  std::vector<int> lane_of;
  if (!lane_split(h, n_layers, descs, lane_of))
    return single_create(h, n_layers, descs, W, U, Z, cores, workspace, workspace_bytes, out);
  tadmm_plan_s* P = new tadmm_plan_s();
  P->h = h;
  P->n = n_layers;
  P->layers.resize(n_layers);
  for (int l = 0; l < n_layers; ++l) {
    const int rc = build_geom(h, descs[l], P->layers[l]);
    if (rc) { delete P; return rc; }
  }
  Lanes* L = new Lanes();
  P->lanes = L;
  L->lane_of = lane_of;
  L->local_of.assign(n_layers, 0);
  char* ws = (char*)workspace;
  size_t off = 0;
  std::vector<int32_t> index_host;                                   // [lane 0 layers | lane 1 layers] -> global slot
  size_t index_off[2] = {0, 0};
  for (int lane = 0; lane < 2; ++lane) {
    index_off[lane] = index_host.size();
    for (int l = 0; l < n_layers; ++l) if (lane_of[l] == lane) { L->local_of[l] = (int)(index_host.size() - index_off[lane]); index_host.push_back(l); }
  }
  int rc = TADMM_OK;
  size_t sub_bytes[2] = {0, 0};
  for (int lane = 0; lane < 2 && rc == TADMM_OK; ++lane) {
    std::vector<tadmm_layer_desc> sd;
    std::vector<const float*> sw;
    std::vector<float*> su, sz, sc;
    for (int l = 0; l < n_layers; ++l) if (lane_of[l] == lane) {
      sd.push_back(descs[l]); sw.push_back(W[l]); su.push_back(U[l]); sz.push_back(Z[l]); sc.push_back(cores ? cores[l] : nullptr);
    }
    rc = single_workspace_bytes(h, (int)sd.size(), sd.data(), &sub_bytes[lane]);
    if (rc) break;
    const size_t need = align_up(sub_bytes[lane], 4096);
    if (off + need > workspace_bytes) { rc = TADMM_ERR_WORKSPACE; h->err = "workspace too small for the two lanes"; break; }
    rc = single_create(h, (int)sd.size(), sd.data(), sw.data(), su.data(), sz.data(), cores ? sc.data() : nullptr, ws + off,
                       need, &L->sub[lane]);
    off += need;
  }
  if (rc == TADMM_OK && off + (size_t)n_layers * 4 > workspace_bytes) { rc = TADMM_ERR_WORKSPACE; h->err = "workspace too small for the lane index"; }
  if (rc == TADMM_OK) {
    if (hipMemcpy(ws + off, index_host.data(), index_host.size() * 4, hipMemcpyHostToDevice) != hipSuccess) rc = TADMM_ERR_HIP;
    for (int lane = 0; lane < 2; ++lane) L->sub[lane]->resid_index = (const int32_t*)(ws + off) + index_off[lane];
  }
  if (rc == TADMM_OK) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);                 // hi is the numerically smaller, more urgent one
    hipError_t e = hipStreamCreateWithPriority(&L->st[0], hipStreamNonBlocking, hi);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&L->st[1], hipStreamNonBlocking, lo);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L->ev_begin, hipEventDisableTiming);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&L->ev_end[i], hipEventDisableTiming);
    if (e != hipSuccess) { rc = TADMM_ERR_HIP; h->err = std::string("lane streams: ") + hipGetErrorString(e); }
  }
  if (rc != TADMM_OK) { lanes_destroy(P); delete P; return rc; }
  L->worker = std::thread(lane_worker, P);
  *out = P;
  return TADMM_OK;
}

int tadmm_plan_run(tadmm_plan p, int update_u, int use_u, double* resid_sq_dev, void* stream_) {
  if (!p) return TADMM_ERR_INVALID;
  if (!p->lanes) return single_run(p, update_u, use_u, resid_sq_dev, stream_);
  DeviceGuard device_guard(p->h);
  Lanes* L = p->lanes;
  hipStream_t s = (hipStream_t)stream_;
  HIP_OK(p->h, hipEventRecord(L->ev_begin, s));                      // both lanes start behind the caller's stream
  for (int i = 0; i < 2; ++i) HIP_OK(p->h, hipStreamWaitEvent(L->st[i], L->ev_begin, 0));
  {
    std::lock_guard<std::mutex> lk(L->mu);
    L->a_update_u = update_u; L->a_use_u = use_u; L->a_resid = resid_sq_dev;
    L->done = false;
    L->job = 1;
  }
  L->cv.notify_all();
  const int rc0 = single_run(L->sub[0], update_u, use_u, resid_sq_dev, L->st[0]);
  int rc1;
  {
    std::unique_lock<std::mutex> lk(L->mu);
    L->cv.wait(lk, [&] { return L->done; });
    rc1 = L->rc;
  }
  for (int i = 0; i < 2; ++i) {                                      // ... and the caller's stream continues behind both
    HIP_OK(p->h, hipEventRecord(L->ev_end[i], L->st[i]));
    HIP_OK(p->h, hipStreamWaitEvent(s, L->ev_end[i], 0));
  }
  for (int i = 0; i < 8; ++i) p->last_ms[i] = L->sub[0]->last_ms[i] + L->sub[1]->last_ms[i];
  p->last_sweeps = L->sub[0]->last_sweeps + L->sub[1]->last_sweeps;
  return rc0 != TADMM_OK ? rc0 : rc1;
}

static void lanes_destroy(tadmm_plan_s* p) {
  Lanes* L = p->lanes;
  if (!L) return;
  if (L->worker.joinable()) {
    { std::lock_guard<std::mutex> lk(L->mu); L->job = 2; }
    L->cv.notify_all();
    L->worker.join();
  }
  for (int i = 0; i < 2; ++i) {
    if (L->sub[i]) {
      if (L->sub[i]->ev_made) for (auto& e : L->sub[i]->ev) (void)hipEventDestroy(e);
      L->sub[i]->poll.destroy();
      delete L->sub[i];
    }
    if (L->st[i]) { (void)hipStreamSynchronize(L->st[i]); (void)hipStreamDestroy(L->st[i]); }
    if (L->ev_end[i]) (void)hipEventDestroy(L->ev_end[i]);
  }
  if (L->ev_begin) (void)hipEventDestroy(L->ev_begin);
  delete L;
  p->lanes = nullptr;
}

int tadmm_lane_split(int n_layers, const tadmm_layer_desc* descs, int32_t* lane_of_out) {
  if (!descs || n_layers <= 0) return TADMM_ERR_INVALID;
  std::vector<int> lane_of;
  const bool two = lane_split(nullptr, n_layers, descs, lane_of);
  if (lane_of_out) for (int l = 0; l < n_layers; ++l) lane_of_out[l] = lane_of[l];
  return two ? 2 : 1;
}

int tadmm_plan_lanes(tadmm_plan p, int32_t* lane_of_out) {
  if (!p) return TADMM_ERR_INVALID;
  if (!p->lanes) { if (lane_of_out) for (int l = 0; l < p->n; ++l) lane_of_out[l] = 0; return 1; }
  if (lane_of_out) for (int l = 0; l < p->n; ++l) lane_of_out[l] = p->lanes->lane_of[l];
  return 2;
}

int tadmm_plan_enable_timing(tadmm_plan p, int on) {
  DeviceGuard device_guard(p ? p->h : nullptr);
  if (!p) return TADMM_ERR_INVALID;
  if (p->lanes) {
    for (int i = 0; i < 2; ++i) { const int rc = tadmm_plan_enable_timing(p->lanes->sub[i], on); if (rc) return rc; }
    p->timing = on != 0;
    return TADMM_OK;
  }
  if (on && !p->ev_made) {
    for (auto& e : p->ev) if (hipEventCreate(&e) != hipSuccess) return TADMM_ERR_HIP;
    p->ev_made = true;
  }
  p->timing = on != 0;
  return TADMM_OK;
}

int tadmm_plan_last_timing(tadmm_plan p, double out_ms[8]) {
  if (!p || !out_ms) return TADMM_ERR_INVALID;
  for (int i = 0; i < 8; ++i) out_ms[i] = p->last_ms[i];
  out_ms[6] = p->last_sweeps;
  return TADMM_OK;
}

static int single_run(tadmm_plan p, int update_u, int use_u, double* resid_sq_dev, void* stream_) {
  DeviceGuard device_guard(p ? p->h : nullptr);
  if (!p) return TADMM_ERR_INVALID;
  tadmm_handle h = p->h;
  hipStream_t s = (hipStream_t)stream_;
  char* ws = p->ws;
  auto D = [&](size_t off) { return ws + off; };
  double acc_ms[8] = {0};
  int total_sweeps = 0;
  p->filt_problems = p->filt_fallbacks = p->filt_stages = 0;
  p->ftm.on = p->timing;
  p->ftm.gemm_ms = 0.0; p->ftm.gemm_launches = 0; p->ftm.gemm_flops = 0.0;
  p->ftm.fast_ms = 0.0; p->ftm.fast_launches = 0; p->ftm.fast_flops = 0.0;
  if (p->timing) { p->ftm.a = p->ev[14]; p->ftm.b = p->ev[15]; }
  p->jtm.on = p->timing;
  p->jtm.tick_ms = 0.0; p->jtm.tick_launches = 0; p->jtm.tick_flops = 0.0; p->jtm.tick_wgs = 0.0;
  if (p->timing) { p->jtm.a = p->ev[14]; p->jtm.b = p->ev[15]; }
  // timing helper: record a pair of events around a phase and accumulate after a sync
  auto tic = [&](int i) { if (p->timing) (void)hipEventRecord(p->ev[i], s); };
  auto toc = [&](int i, int slot) {
    if (!p->timing) return;
    (void)hipEventRecord(p->ev[i + 1], s);
    (void)hipEventSynchronize(p->ev[i + 1]);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, p->ev[i], p->ev[i + 1]);
    acc_ms[slot] += ms;
  };

  tic(0);
  launch_unfold((const SweepDesc*)D(p->sweep_desc_off), (const BlockRef*)D(p->unfold.map_off), p->unfold.nblocks,
                use_u, s);
  toc(0, 0);

  // one eigen group of a level: the tournament (or the single-launch solver) and its finalize launches
  // The finalize launches only read the X images and write outputs of their own, so the tournament may queue them
  // behind the sweep it expects to be the last, in front of its blocking read of that sweep's verdict (EigGroup::behind_last).
  auto solve_group = [&](EigLayout& L, EigGroup eg, bool* small_pending) -> int {
    int gs = 0;
    bool finalized = false;
    eg.behind_last = [&](hipStream_t st) { L.finalize(ws, st, eg.skip); };
    const int rc = run_eig_group(h, eg, p->poll, p->tol, p->max_global_sweeps, p->debug, s, &gs,
                                 small_pending, &p->jtm, &finalized);
    if (rc != TADMM_OK) return rc;
    L.last_sweeps = gs;     // main: the next run's `expected`; fallback: informational (its expected stays 0)
    total_sweeps += gs;
    if (!finalized) L.finalize(ws, s, eg.skip);
    return TADMM_OK;
  };

  for (StepPlan& sp : p->steps) {
    if (sp.main.neig == 0) continue;
    tic(0);
    launch_gram_partial((const GramDesc*)D(sp.gram_p.desc_off), (const BlockRef*)D(sp.gram_p.map_off),
                        sp.gram_p.nblocks, s);
    launch_gram_reduce((const GramDesc*)D(sp.gram_r.desc_off), (const BlockRef*)D(sp.gram_r.map_off),
                       sp.gram_r.nblocks, s);
    toc(0, 1);
    tic(0);
    const bool filtered = sp.fg.nf > 0;
    if (filtered) {
      const int rc = filter_run_pre(h, sp.fg, ws, p->poll, s, p->debug, &p->ftm);
      if (rc != TADMM_OK) return rc;
    }
    EigGroup eg = sp.main.group(ws, filtered ? (const int32_t*)D(sp.skip_off) : nullptr);
    eg.off_dev = (const double*)D(sp.off_off); eg.done_dev = (const int*)D(sp.done_off);
    eg.expected = sp.main.last_sweeps;
    bool small_pending = false;
    bool proj_queued = false;
    auto launch_proj = [&] {
      launch_gemm((const GemmDesc*)D(sp.proj.desc_off), (const BlockRef*)D(sp.proj.map_off), sp.proj.nblocks, s);
    };
    {
      const int rc = solve_group(sp.main, eg, &small_pending);
      if (rc != TADMM_OK) return rc;
    }
    if (filtered) {
      if (small_pending) {
        const int rc = check_small_group(h, eg, p->poll);
        if (rc != TADMM_OK) return rc;
        small_pending = false;
      }
      int nbad = 0;
      // The level's projection goes out behind the verdict's event, before the host waits for it; when a problem falls
      // back, the launch is repeated below on the fallback's outputs.  Instrumented runs keep the phases apart.
      std::function<void()> early_proj;
      if (sp.proj_repeatable && !p->timing)
        early_proj = [&] { launch_proj(); proj_queued = true; };
      int rc = filter_run_post(h, sp.fg, ws, p->poll, s, p->debug, &nbad, &p->ftm, early_proj);
      if (rc != TADMM_OK) return rc;
      if (nbad > 0) proj_queued = false;
      p->filt_problems += sp.fg.nf;
      p->filt_fallbacks += nbad;
      p->filt_stages = std::max(p->filt_stages, sp.fg.last_stages);
      if (nbad > 0) {       // the full Jacobi solve for the problems the filter could not certify
        const EigGroup fgp = sp.fb.group(ws, (const int32_t*)D(sp.fb_skip_off));
        bool fsmall = false;
        rc = solve_group(sp.fb, fgp, &fsmall);
        if (rc != TADMM_OK) return rc;
        if (fsmall) {
          rc = check_small_group(h, fgp, p->poll);
          if (rc != TADMM_OK) return rc;
        }
      }
    }
    toc(0, 2);
    tic(0);
    if (!proj_queued) launch_proj();
    toc(0, 3);
    if (small_pending) {      // the finalize + projection launches above are already queued behind it
      const int rc = check_small_group(h, eg, p->poll);
      if (rc != TADMM_OK) return rc;
    }
  }
  tic(0);
  for (Phase& ph : p->recon)
    launch_gemm((const GemmDesc*)D(ph.desc_off), (const BlockRef*)D(ph.map_off), ph.nblocks, s);
  toc(0, 4);
  tic(0);
  double* partial = (double*)D(p->resid_partial_off);
  launch_fold_update((const SweepDesc*)D(p->sweep_desc_off), (const BlockRef*)D(p->fold.map_off), p->fold.nblocks,
                     update_u, partial, s);
  if (resid_sq_dev)
    launch_resid_reduce((const SweepDesc*)D(p->sweep_desc_off), p->n, partial, resid_sq_dev, s, p->resid_index);
  toc(0, 5);
  HIP_OK(h, hipGetLastError());
  for (int i = 0; i < 8; ++i) p->last_ms[i] = acc_ms[i];
  p->last_sweeps = total_sweeps;
  if (p->debug) { (void)hipStreamSynchronize(s); dump_stamps(); }
  return TADMM_OK;
}

int tadmm_plan_singular_values(tadmm_plan p, int layer, int step, double* out_host, void* stream_) {
  DeviceGuard device_guard(p ? p->h : nullptr);
  if (!p || !out_host || layer < 0 || layer >= p->n) return TADMM_ERR_INVALID;
  if (p->lanes)
    return tadmm_plan_singular_values(p->lanes->sub[p->lanes->lane_of[layer]], p->lanes->local_of[layer], step, out_host, stream_);
  const LayerGeom& g = p->layers[layer];
  if (step < 0 || step >= (int)g.steps.size()) return TADMM_ERR_INVALID;
  const size_t off = p->sigma_off[layer][step];
  if (off == (size_t)-1) CTX_FAIL(p->h, TADMM_ERR_INVALID, "step %d of layer %d was skipped (identity)", step, layer);
  hipStream_t s = (hipStream_t)stream_;
  HIP_OK(p->h, hipMemcpyAsync(out_host, p->ws + off, (size_t)g.steps[step].r * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(p->h, hipStreamSynchronize(s));
  return TADMM_OK;
}

int tadmm_plan_filter_timing(tadmm_plan p, double out[4]) {
  if (!p || !out) return TADMM_ERR_INVALID;
  if (sum_over_lanes(p, out, tadmm_plan_filter_timing)) return TADMM_OK;
  out[0] = p->ftm.gemm_ms; out[1] = p->ftm.gemm_launches; out[2] = p->ftm.gemm_flops; out[3] = 0.0;
  return TADMM_OK;
}

int tadmm_plan_jacobi_timing(tadmm_plan p, double out[4]) {
  if (!p || !out) return TADMM_ERR_INVALID;
  if (sum_over_lanes(p, out, tadmm_plan_jacobi_timing)) return TADMM_OK;
  out[0] = p->jtm.tick_ms; out[1] = p->jtm.tick_launches; out[2] = p->jtm.tick_flops; out[3] = p->jtm.tick_wgs;
  return TADMM_OK;
}

int tadmm_plan_filter_timing_fast(tadmm_plan p, double out[4]) {
  if (!p || !out) return TADMM_ERR_INVALID;
  if (sum_over_lanes(p, out, tadmm_plan_filter_timing_fast)) return TADMM_OK;
  out[0] = p->ftm.fast_ms; out[1] = p->ftm.fast_launches; out[2] = p->ftm.fast_flops; out[3] = 0.0;
  return TADMM_OK;
}

int tadmm_plan_filter_stats(tadmm_plan p, int32_t out[4]) {
  if (!p || !out) return TADMM_ERR_INVALID;
  if (sum_over_lanes(p, out, tadmm_plan_filter_stats, true)) return TADMM_OK;   // stages: the deeper lane's
  int eligible = 0;
  for (const StepPlan& sp : p->steps) eligible += sp.fg.nf;
  out[0] = eligible; out[1] = p->filt_problems; out[2] = p->filt_fallbacks; out[3] = p->filt_stages;
  return TADMM_OK;
}

int tadmm_plan_destroy(tadmm_plan p) {
  DeviceGuard device_guard(p ? p->h : nullptr);
  if (!p) return TADMM_OK;
  lanes_destroy(p);
  if (p->ev_made) for (auto& e : p->ev) (void)hipEventDestroy(e);
  p->poll.destroy();
  delete p;
  return TADMM_OK;
}

int tadmm_plan_set_jacobi(tadmm_plan p, double tol, int inner_sweeps, int max_sweeps) {
  if (!p) return TADMM_ERR_INVALID;
  if (p->lanes) for (int i = 0; i < 2; ++i) tadmm_plan_set_jacobi(p->lanes->sub[i], tol, inner_sweeps, max_sweeps);
  if (tol > 0) p->tol = tol;
  (void)inner_sweeps;    // ignored: the 16x16 rotation solve is one cyclic sweep (include/tadmm.h)
  if (max_sweeps > 0) p->max_global_sweeps = max_sweeps;
  return TADMM_OK;
}

int tadmm_plan_ranks(tadmm_plan p, int layer, int32_t* ranks_out) {
  if (!p || !ranks_out || layer < 0 || layer >= p->n) return TADMM_ERR_INVALID;
  const tadmm_layer_desc& d = p->layers[layer].desc;
  for (int i = 0; i <= d.d; ++i) ranks_out[i] = d.ranks[i];
  return d.d + 1;
}

}  // extern "C"
