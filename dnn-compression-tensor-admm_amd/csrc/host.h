// Host-side pieces shared by the plan builders (plan.hip: TT / SVD projection, tucker_plan.hip: Tucker-2) and the
// stand-alone entries (abi_ops.hip): the context object behind tadmm_handle, error macros, the two-pass workspace
// arena and its placement helpers, the geometry of one eigen-problem, the XCD-aware block order of the Jacobi
// tournament and of the grouped tile products, and the layout and driver loop of one grouped eigen-solve.
#pragma once
#include "common.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

struct tadmm_ctx_s {
  int device = 0;
  std::string err;
};

#define CTX_FAIL(h, code, ...)                                   \
  do {                                                           \
    char _b[512];                                                \
    snprintf(_b, sizeof _b, __VA_ARGS__);                        \
    if (h) (h)->err = _b;                                        \
    return (code);                                               \
  } while (0)

#define HIP_OK(h, call)                                                                              \
  do {                                                                                               \
    hipError_t _e = (call);                                                                          \
    if (_e != hipSuccess) CTX_FAIL(h, TADMM_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
  } while (0)

namespace tadmm {

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Every C-ABI entry that launches or allocates runs on the handle's device, whatever device the calling thread
// has current (one process may drive several GPUs); the caller's choice is restored on exit.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(const tadmm_ctx_s* h) {
    if (!h) return;
    if (hipGetDevice(&prev) != hipSuccess) { prev = -1; return; }
    if (prev != h->device) switched = hipSetDevice(h->device) == hipSuccess;
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Raises a kernel's dynamic-LDS limit above the default 64 KiB, once per device (the attribute belongs to the device's
// code object).  A launcher keeps one static instance per kernel instantiation.  The flags are atomic: the two lanes of a
// projection plan launch from two host threads, and setting the attribute twice is harmless.  A failed call is returned
// and leaves the flag clear; every launcher hands it to the ABI caller as TADMM_ERR_HIP.
struct DynLdsOptIn {
  std::atomic<bool> done[64] = {};
  template <class K> hipError_t operator()(K kernel, size_t bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::atomic<bool>& flag = done[dev & 63];
    if (flag.load(std::memory_order_acquire)) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) flag.store(true, std::memory_order_release);
    else (void)hipGetLastError();      // reported through the return value: not left behind for the next HIP call
    return e;
  }
};

// core convolution (coreconv.hip): descriptor checks shared with its weight gradient (wgrad.hip), and the launch
int core_conv_check(tadmm_ctx_s* h, const tadmm_core_conv_desc* c, bool need_planes, int planes_rows, int planes_cols);
int launch_core_conv(tadmm_ctx_s* h, const tadmm_core_conv_desc* c, int transposed, hipStream_t s);

struct Phase {  // one grouped launch: descriptor array + block map inside the device arena
  size_t desc_off = 0, map_off = 0;
  int nprob = 0, nblocks = 0;
};

// A simple bump allocator of workspace offsets; a layout is run twice, once to size the workspace, once for real.
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes, size_t align = 256) {
    off = align_up(off, align);
    const size_t o = off;
    off += bytes;
    return o;
  }
};

struct HostImage {   // host copy of the descriptor part of the arena; it ends at the last non-empty array put into it
  std::vector<char> bytes;
  void put(size_t off, const void* src, size_t n) {
    if (!n) return;
    if (bytes.size() < off + n) bytes.resize(off + n);
    memcpy(bytes.data() + off, src, n);
  }
};

// descriptor array + block map of one grouped launch -> descriptor arena (and the host image when given)
static inline void place_phase(Phase& ph, Arena& da, HostImage* img, const void* descs, size_t dbytes, int nprob,
                               const std::vector<BlockRef>& map) {
  ph.nprob = nprob;
  ph.nblocks = (int)map.size();
  ph.desc_off = da.take(std::max<size_t>(dbytes, 16));
  ph.map_off = da.take(std::max<size_t>(map.size() * sizeof(BlockRef), 16));
  if (img) {
    img->put(ph.desc_off, descs, dbytes);
    img->put(ph.map_off, map.data(), map.size() * sizeof(BlockRef));
  }
}

// the descriptors of `like` under another block map (Gram reduce; self / norms / extract of an eigen group)
static inline void place_map_like(Phase& ph, const Phase& like, Arena& da, HostImage* img, const std::vector<BlockRef>& map) {
  ph = like;
  ph.nblocks = (int)map.size();
  ph.map_off = da.take(std::max<size_t>(map.size() * sizeof(BlockRef), 16));
  if (img) img->put(ph.map_off, map.data(), map.size() * sizeof(BlockRef));
}

// sets the tile counts of one fp32 GEMM and returns the number of its blocks
static inline size_t set_gemm_tiles(GemmDesc& g) {
  g.tiles_m = (g.M + kGemmBM - 1) / kGemmBM;
  g.tiles_n = (g.N + kGemmBN - 1) / kGemmBN;
  return (size_t)g.tiles_m * g.tiles_n;
}
// the same, appending the blocks to the map of the grouped launch as problem `prob`
static inline void gemm_tiles(GemmDesc& g, int prob, std::vector<BlockRef>& map) {
  const int nt = (int)set_gemm_tiles(g);
  for (int b = 0; b < nt; ++b) map.push_back(BlockRef{prob, b});
}

// Geometry of one eigen-problem: the N x N Gram of an m x cols matrix, taken on its smaller side, and the split-K
// shape of the launch that forms it.
struct EigGeom {
  int m = 0;            // rows of the matrix
  int64_t cols = 0;     // columns of the matrix
  bool trans = false;   // m > cols : eigen-solve on A^T A
  int N = 0, Npad = 0, nb = 0, ld = 0;
  int nt = 0, ksplit = 1, kchunk = 0;
};

// wg_target: Gram workgroups a problem should at least have; cap_chunk: no K chunk longer than 2048.  The plans pass
// (64, true), the stand-alone Gram (256, false).
static inline EigGeom eig_geom(int m, int64_t cols, int wg_target, bool cap_chunk) {
  EigGeom g;
  g.m = m; g.cols = cols;
  g.trans = (int64_t)m > cols;
  g.N = (int)std::min<int64_t>(m, cols);
  g.Npad = (int)align_up(g.N, 4 * kJB);     // whole super-pairs of 2 x 16 columns
  g.nb = g.Npad / kJB;
  // row length of the eigen-solver's X image: whole 1 KiB chunks (tick3 wants ld % 64 == 0)
  g.ld = eig_ld(g.N);
  g.nt = (g.N + 31) / 32;
  // (an empty problem, N <= 0, gets a valid split too: the size queries of the ABI are total, the entries refuse it)
  const int64_t K = std::max<int64_t>(1, g.trans ? m : cols);
  const int ntp = std::max(1, g.nt * (g.nt + 1) / 2);
  // split-K only where a problem has too few tiles to matter beside the others of its level (levels batch
  // 15-30 problems): >= 64 workgroups per problem in a plan; big problems (ks = 1) write G directly, no reduce pass
  int ks = (wg_target + ntp - 1) / ntp;
  const int maxks = (int)std::max<int64_t>(1, (K + 255) / 256);
  ks = std::max(1, std::min(ks, maxks));
  // a workgroup's duration grows with its K chunk and it shares the CU's matrix cores with its neighbours:
  // cap the chunk so that the long reductions (K = 4608 beside K = 512) do not form the tail of the launch
  if (cap_chunk) ks = std::max(ks, (int)((K + 2047) / 2048));
  g.kchunk = (int)align_up((K + ks - 1) / ks, 64);
  g.ksplit = (int)((K + g.kchunk - 1) / g.kchunk);
  return g;
}

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share one, MI355X_MICROARCH "Workgroup
// dispatch").  Re-order a block map so that CONSECUTIVE logical blocks land on the same XCD: the tournament
// hands a super-block from workgroup q to q+-1 between launches, so the next launch finds it in that XCD's L2.
static inline void xcd_group(std::vector<BlockRef>& m) {
  const char* e = getenv("TADMM_XCD_MAP");   // default on; 0 = plain order (for A/B measurements)
  if (e && !atoi(e)) return;
  const int G = (int)m.size();
  if (G < 16) return;
  std::vector<BlockRef> out(G);
  int i = 0;
  for (int x = 0; x < 8; ++x)
    for (int b = x; b < G; b += 8) out[b] = m[i++];
  m.swap(out);
}

// Grouped launches whose problems are re-read many times by their own blocks (the block products of the filtered
// eigen-solver: every 32x32 tile of a problem streams the problem's whole G and block image): give each PROBLEM to
// one XCD, so that its operands stay in that XCD's 4 MiB L2 instead of being fetched by all eight.  Blocks i, i+8, ..
// are observed to share an XCD; problems are dealt to the eight bins longest first, and a bin that runs dry steals
// from the fullest one (balance over locality).  Placement is a speed matter only.
static inline void xcd_by_problem(std::vector<BlockRef>& m, const std::vector<double>& weight) {
  const char* e = getenv("TADMM_XCD_MAP");
  if (e && !atoi(e)) return;
  const int G = (int)m.size();
  if (G < 64) return;
  const int np = (int)weight.size();
  std::vector<std::vector<BlockRef>> per(np);
  for (const BlockRef& b : m) per[b.prob].push_back(b);
  std::vector<int> order(np);
  for (int i = 0; i < np; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return weight[a] * per[a].size() > weight[b] * per[b].size();
  });
  std::vector<std::vector<BlockRef>> bin(8);
  double load[8] = {0};
  for (int p : order) {
    int best = 0;
    for (int x = 1; x < 8; ++x) if (load[x] < load[best]) best = x;
    load[best] += weight[p] * per[p].size();
    bin[best].insert(bin[best].end(), per[p].begin(), per[p].end());
  }
  size_t head[8] = {0};
  std::vector<BlockRef> out;
  out.reserve(G);
  for (int i = 0; (int)out.size() < G; ++i) {
    int x = i & 7;
    if (head[x] >= bin[x].size()) {         // dry: steal from the bin with the most blocks left
      int full = -1; size_t left = 0;
      for (int y = 0; y < 8; ++y) if (bin[y].size() - head[y] > left) { left = bin[y].size() - head[y]; full = y; }
      if (full < 0) break;
      x = full;
    }
    out.push_back(bin[x][head[x]++]);
  }
  m.swap(out);
}

// The same dealing with an arbitrary affinity key per block (blocks with equal key share an XCD and hence an L2): dgemm3
// keys its tiles by (problem, column tile), so the slice of G a column tile reads is fetched into ONE L2.
template <class KeyFn>
static inline void xcd_by_key(std::vector<BlockRef>& m, KeyFn key) {
  const char* e = getenv("TADMM_XCD_MAP");
  if (e && !atoi(e)) return;
  const int G = (int)m.size();
  if (G < 64) return;
  std::vector<std::vector<BlockRef>> bin(8);
  for (const BlockRef& b : m) bin[(size_t)(key(b) & 7)].push_back(b);
  size_t head[8] = {0};
  std::vector<BlockRef> out;
  out.reserve(G);
  for (int i = 0; (int)out.size() < G; ++i) {
    int x = i & 7;
    if (head[x] >= bin[x].size()) {
      int full = -1; size_t left = 0;
      for (int y = 0; y < 8; ++y) if (bin[y].size() - head[y] > left) { left = bin[y].size() - head[y]; full = y; }
      if (full < 0) break;
      x = full;
    }
    out.push_back(bin[x][head[x]++]);
  }
  m.swap(out);
}

// ---- Grouped NT tile products (dgemm_nt_tile_kernel): which tile runs next to which L2 ----
// One problem of a grouped launch: C[M][N] = A[M][K] * B[N][K]^T in TM x TN tiles.  A tile (tm, tn) streams one TM-row
// panel of A (the block image Y) and one TN-row panel of B (G); the plain map is problem-major with tn fastest, so with
// blocks dealt round-robin over the eight XCDs nearly every L2 fetches nearly every panel of a problem.
struct TileProb { int M, N, K, TM, TN; };
static inline int tile_rows(const TileProb& q) { return (q.M + q.TM - 1) / q.TM; }
static inline int tile_cols(const TileProb& q) { return (q.N + q.TN - 1) / q.TN; }

// TADMM_XCD_MAP=0: plain order (as for the other maps here).  TADMM_TILE_MAP: 0 plain order for these maps alone, 1 the
// band height with the smaller modelled traffic (default), 2 whole columns (h = tiles_m: one owner slot per G panel).
// TADMM_TILE_MAP_LONGEST=0: the runs of a slot queue in problem order instead of longest K first.  (A/B measurements.)
static inline int tile_map_mode() {
  const char* e = getenv("TADMM_XCD_MAP");
  if (e && !atoi(e)) return 0;
  const char* b = getenv("TADMM_TILE_MAP");
  return b ? std::max(0, std::min(2, atoi(b))) : 1;
}

static inline std::vector<BlockRef> tile_map_plain(const std::vector<TileProb>& probs) {
  std::vector<BlockRef> m;
  for (int p = 0; p < (int)probs.size(); ++p)
    for (int b = 0; b < tile_rows(probs[p]) * tile_cols(probs[p]); ++b) m.push_back(BlockRef{p, b});
  return m;
}

// Modelled operand traffic of one launch, bytes: position i of the map belongs to XCD slot i % 8, and every slot fetches
// each distinct (problem, A panel) and (problem, B panel) among its tiles once -- no reuse between slots, none lost
// inside one.
static inline double tile_map_cost(const std::vector<BlockRef>& map, const std::vector<TileProb>& probs) {
  std::vector<int> off(probs.size() + 1, 0);
  for (size_t p = 0; p < probs.size(); ++p) off[p + 1] = off[p] + tile_rows(probs[p]) + tile_cols(probs[p]);
  std::vector<char> seen((size_t)8 * off.back(), 0);
  double bytes = 0;
  for (size_t i = 0; i < map.size(); ++i) {
    const TileProb& q = probs[map[i].prob];
    const int tn = tile_cols(q), tr = tile_rows(q), r = map[i].local / tn, c = map[i].local - r * tn;
    char* s = seen.data() + (i & 7) * (size_t)off.back() + off[map[i].prob];
    if (!s[r]) { s[r] = 1; bytes += 8.0 * q.TM * q.K; }
    if (!s[tr + c]) { s[tr + c] = 1; bytes += 8.0 * q.TN * q.K; }
  }
  return bytes;
}

// A problem's tiles in bands of about h tile rows, column by column inside a band, the bands in alternating column
// direction: every stretch of the list is a compact patch of the (tm, tn) grid.
static inline std::vector<int> tile_band_order(int tr, int tn, int h) {
  std::vector<int> l;
  l.reserve((size_t)tr * tn);
  const int nb = (tr + h - 1) / h;
  for (int b = 0; b < nb; ++b) {
    const int r0 = b * tr / nb, r1 = (b + 1) * tr / nb;
    for (int k = 0; k < tn; ++k) {
      const int c = (b & 1) ? tn - 1 - k : k;
      for (int r = r0; r < r1; ++r) l.push_back(r * tn + c);
    }
  }
  return l;
}

// The map of a grouped launch, ordered so that position i belongs to XCD slot i % 8 (blocks i, i + 8, .. are observed to
// share an XCD; placement is a speed matter only, no result depends on it).  A permutation of the plain map.
//  - Every problem is cut into eight runs of its band order, run j for slot j: a slot sees a compact patch of every
//    problem (few distinct panels), every problem runs on all eight XCDs, and the slot of a patch depends on the
//    problem's own grid alone -- the panels of G meet the same L2 in every launch of a level.
//  - Runs differ by at most one tile; the odd tiles go to the slots after the one the previous problem stopped at, which
//    keeps the eight queues at the lengths the positions i % 8 give them (no padding entries).
//  - The band height of a problem is the one whose runs touch the fewest panel bytes (ties: the taller band).
//  - A slot's queue holds its runs longest K first: the short tiles fill in behind the long ones of the same XCD.
// The plain map is returned where the model says the order gains nothing.
static inline std::vector<BlockRef> tile_map_build(const std::vector<TileProb>& probs) {
  const int mode = tile_map_mode();
  std::vector<BlockRef> plain = tile_map_plain(probs);
  if (mode == 0) return plain;
  const int np = (int)probs.size();
  std::vector<std::vector<BlockRef>> run((size_t)np * 8);
  int fill = 0;                                  // slots [0, fill) are one tile ahead of the others
  for (int p = 0; p < np; ++p) {
    const TileProb& q = probs[p];
    const int tr = tile_rows(q), tn = tile_cols(q), n = tr * tn;
    int cnt[8];
    for (int x = 0; x < 8; ++x) cnt[x] = n / 8;
    for (int k = 0; k < n % 8; ++k) ++cnt[(fill + k) & 7];
    fill = (fill + n) & 7;
    std::vector<int> best;
    double best_cost = 0;
    for (int h = (mode == 2 ? tr : 1); h <= tr; ++h) {
      std::vector<int> l = tile_band_order(tr, tn, h);
      double cost = 0;
      for (int x = 0, i = 0; x < 8; i += cnt[x++]) {
        std::vector<char> seen((size_t)tr + tn, 0);
        for (int k = i; k < i + cnt[x]; ++k) {
          const int r = l[k] / tn, c = l[k] - r * tn;
          if (!seen[r]) { seen[r] = 1; cost += q.TM; }
          if (!seen[tr + c]) { seen[tr + c] = 1; cost += q.TN; }
        }
      }
      if (best.empty() || cost <= best_cost) { best.swap(l); best_cost = cost; }
    }
    for (int x = 0, i = 0; x < 8; i += cnt[x++])
      for (int k = i; k < i + cnt[x]; ++k) run[(size_t)p * 8 + x].push_back(BlockRef{p, best[k]});
  }
  std::vector<int> order(np);
  for (int p = 0; p < np; ++p) order[p] = p;
  if (const char* e = getenv("TADMM_TILE_MAP_LONGEST"); !(e && !atoi(e)))
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return probs[a].K > probs[b].K; });
  std::vector<BlockRef> queue[8];
  for (int x = 0; x < 8; ++x)
    for (int p : order) queue[x].insert(queue[x].end(), run[(size_t)p * 8 + x].begin(), run[(size_t)p * 8 + x].end());
  std::vector<BlockRef> out(plain.size());
  for (size_t i = 0; i < out.size(); ++i) out[i] = queue[i & 7][i >> 3];
  return tile_map_cost(out, probs) <= tile_map_cost(plain, probs) ? out : plain;
}

// Which tick kernel a group of problems uses.
enum class EigTick {
  Pairs,        // one workgroup per pair of 8-column blocks: jacobi_tick_kernel, or the streamed kernel for long rows
  SuperPairs,   // one workgroup per pair of 16-column super-blocks: jacobi_tick3_kernel, self pass in a sweep's first tick
};
// Super-pairs whenever 32 columns of the group's longest row fit the LDS (ld_max <= 512).  TADMM_JACOBI_MODE=0 asks for
// pairs (A/B measurements); any other value means the default.
static inline EigTick choose_eig_tick(int ld_max) {
  const char* em = getenv("TADMM_JACOBI_MODE");
  const bool want_pairs = em && atoi(em) == 0;
  return (!want_pairs && jacobi_tick3_fits(ld_max)) ? EigTick::SuperPairs : EigTick::Pairs;
}

// One sweep period for every problem of a tick3 group (EigDesc::period); TADMM_JACOBI_ALIGN=0 restores per-problem periods.
static inline bool align_sweeps_on() {
  static const bool on = !(getenv("TADMM_JACOBI_ALIGN") && !atoi(getenv("TADMM_JACOBI_ALIGN")));
  return on;
}

// Pinned verdict slots + events of the pipelined convergence poll (one per plan).
struct PollCtx {
  hipEvent_t ev[2];
  int* host = nullptr;      // 2 slots of `stride` ints, written by jacobi_conv_kernel
  size_t stride = 0;
  bool made = false;
  hipError_t create(size_t max_problems) {
    stride = (max_problems + 1 + 15) & ~(size_t)15;
    hipError_t e = hipHostMalloc((void**)&host, 2 * stride * sizeof(int), hipHostMallocDefault);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    made = e == hipSuccess;
    return e;
  }
  void destroy() {
    if (!made) return;
    for (auto& e : ev) (void)hipEventDestroy(e);
    (void)hipHostFree(host);
    made = false;
  }
};

// instrumented runs only (tadmm_plan_enable_timing): every jacobi_tick3 launch timed on its own
struct JacobiTiming {
  bool on = false;
  hipEvent_t a{}, b{};
  double tick_ms = 0.0; int tick_launches = 0; double tick_flops = 0.0; double tick_wgs = 0.0;
  double small_ms = 0.0; int small_launches = 0; double small_flops = 0.0;    // single-launch solver (<= 64 columns)
  const int* small_n = nullptr;       // per problem: N of its eigen-problem (8 N^3 model of the launch's work)
};

// One grouped eigen-solve: `neig` symmetric problems whose descriptors / block maps already sit on the device.
struct EigGroup {
  const EigDesc* ed = nullptr;
  int neig = 0;
  const int* players = nullptr;     // per problem: tournament players (super-blocks or blocks)
  int gsteps = 0;                   // ticks per global sweep = max(players - 1)
  EigTick kernel = EigTick::Pairs;
  int ld_max = 0;
  size_t tick_lds = 0;              // Pairs: dynamic LDS of the tick launches
  const BlockRef* tick_map = nullptr; int tick_blocks = 0;
  double* prev_dev = nullptr;       // [neig] scratch of the convergence kernel
  const int32_t* skip = nullptr;    // optional per-problem predicate (non-zero: the problem is dropped)
  int npad_max = 0;                 // largest padded problem size (<= 64: single-launch solver)
  int expected = 0;                 // sweeps the previous run of this group needed (0: unknown)
  bool aligned = false;             // every EigDesc carries period = gsteps: all sweeps start at the same tick
  bool warm = false;                // some EigDesc of the group carries a warm-start image (jacobi_small: second LDS image)
  const int* row_len = nullptr;     // per problem: ld of its X image (timing only: executed flops of a tick)
  const int* mid_sizes = nullptr;   // per problem: 128 / 192 when it may take the direct route (EigDesc::scratch set), else 0
  std::function<void(hipStream_t)> after_init;   // tick path only: queued right after jacobi_init (which takes the scale
                                                 // of a problem from X = G), e.g. the warm start X <- V G of big problems
  // tick path only, optional: launches that only read the X images and write outputs of their own (the group's finalize).
  // Queued behind every sweep whose verdict the host then blocks on -- the sweeps from `expected` on -- so that the
  // stream is not empty during that wait; run_eig_group reports whether they stand behind the final sweep.
  std::function<void(hipStream_t)> behind_last;
  // debug only
  const double* off_dev = nullptr; const int* done_dev = nullptr;
};

// Plan-time state of one grouped eigen-solve: where its descriptors and block maps sit in the workspace, and the
// kernel choice of the group.  tick carries the EigDesc array; norm / ext are further maps over it.
struct EigLayout {
  Phase tick, norm, ext;
  std::vector<int> players;       // per problem: tournament players
  std::vector<int> row_len;       // per problem: ld of the X image (instrumented runs)
  std::vector<int> mid;           // per problem: 128 / 192 when it may take the direct route of tridiag_mid.hip, else 0
  int neig = 0;
  int gsteps = 0;                 // ticks per global sweep = max(players - 1)
  EigTick kernel = EigTick::Pairs;
  int ld_max = 0, npad_max = 0;
  size_t tick_lds = 0;            // Pairs: dynamic LDS of the tick launches
  bool aligned = false;           // every EigDesc carries period = gsteps
  size_t prev_off = 0;            // [neig] doubles of the convergence kernel (taken by the caller)
  int last_sweeps = 0;            // global sweeps the previous run needed

  // The run-time view; the caller adds what is its own (off_dev / done_dev, warm, after_init, expected).
  // mid_sizes is always given: only Rayleigh-Ritz descriptors carry EigDesc::scratch (filter_layout), so the fallback and
  // Tucker groups have all-zero `mid` and stay off the direct route of tridiag_mid.hip -- setting `scratch` on their
  // descriptors would change their launch sequence.  row_len feeds the flop count of instrumented runs only.
  EigGroup group(char* ws, const int32_t* skip) const {
    EigGroup g;
    g.ed = (const EigDesc*)(ws + tick.desc_off); g.neig = neig;
    g.players = players.data(); g.row_len = row_len.data(); g.mid_sizes = mid.data();
    g.gsteps = gsteps; g.kernel = kernel; g.aligned = aligned;
    g.ld_max = ld_max; g.npad_max = npad_max; g.tick_lds = tick_lds;
    g.tick_map = (const BlockRef*)(ws + tick.map_off); g.tick_blocks = tick.nblocks;
    g.prev_dev = (double*)(ws + prev_off);
    g.skip = skip;
    return g;
  }
  // eigenvalues and their order; then the kept vectors and sigma (a caller may queue work on the sorted columns between)
  void sort(char* ws, hipStream_t s, const int32_t* skip) const {
    const EigDesc* ed = (const EigDesc*)(ws + tick.desc_off);
    launch_eig_norms(ed, (const BlockRef*)(ws + norm.map_off), norm.nblocks, s, skip);
    launch_eig_sort(ed, neig, s, skip, npad_max);
  }
  void extract(char* ws, hipStream_t s, const int32_t* skip) const {
    launch_eig_extract((const EigDesc*)(ws + tick.desc_off), (const BlockRef*)(ws + ext.map_off), ext.nblocks, s, skip);
  }
  void finalize(char* ws, hipStream_t s, const int32_t* skip) const { sort(ws, s, skip); extract(ws, s, skip); }
};

// Kernel choice, players and the three block maps of a group (counts go into the layout's phases, offsets do not).
// `align` (tick3 groups, unless TADMM_JACOBI_ALIGN=0): stamp one sweep period on every problem.
// Every eigen-solver descriptor of the library passes through here, so this is where the premise of the tick kernels'
// loader is checked: rows of whole 1 KiB pieces (eig_ld).
struct EigMaps { std::vector<BlockRef> tick, norm, ext; };
static inline int eig_maps(tadmm_handle h, EigLayout& l, std::vector<EigDesc>& descs, bool align, EigMaps& m) {
  for (const EigDesc& e : descs)
    if (e.ld <= 0 || e.ld % 128)
      CTX_FAIL(h, TADMM_ERR_INVALID, "internal: eigen-problem (N = %d) with rows of %d doubles; the Jacobi kernels need a "
               "multiple of 128", e.N, e.ld);
  l.neig = (int)descs.size();
  l.ld_max = l.npad_max = l.gsteps = 0;
  l.players.clear(); l.row_len.clear(); l.mid.clear();
  for (const EigDesc& e : descs) { l.ld_max = std::max(l.ld_max, e.ld); l.npad_max = std::max(l.npad_max, e.Npad); }
  // tick shape of the group: LDS-resident super-pairs when every problem fits, else plain pairs
  l.kernel = descs.empty() ? EigTick::Pairs : choose_eig_tick(l.ld_max);
  const bool super = l.kernel == EigTick::SuperPairs;
  l.tick_lds = jacobi_tick_lds_bytes(l.ld_max);
  for (int pq = 0; pq < l.neig; ++pq) {
    const EigDesc& e = descs[pq];
    const int units = super ? e.nb / 2 : e.nb;       // players of the tournament
    l.players.push_back(units);
    l.row_len.push_back(e.ld);
    l.mid.push_back((e.scratch && eig_mid_direct_size(e.N) && e.N == e.Npad) ? e.N : 0);
    l.gsteps = std::max(l.gsteps, units - 1);
    for (int b = 0; b < units / 2; ++b) m.tick.push_back(BlockRef{pq, b});
    for (int b = 0; b < (e.Npad + 3) / 4; ++b) m.norm.push_back(BlockRef{pq, b});
    for (int b = 0; b < (e.r + 3) / 4; ++b) m.ext.push_back(BlockRef{pq, b});
  }
  xcd_group(m.tick);
  l.aligned = super && align && align_sweeps_on();
  if (l.aligned) for (EigDesc& e : descs) e.period = l.gsteps;
  l.tick.nprob = l.norm.nprob = l.ext.nprob = l.neig;
  l.tick.nblocks = (int)m.tick.size();
  l.norm.nblocks = (int)m.norm.size(); l.ext.nblocks = (int)m.ext.size();
  return TADMM_OK;
}

// eig_maps + placement: descriptors and tick map, then the norm and ext maps, in that order from `da`
static inline int build_eig_layout(tadmm_handle h, EigLayout& l, std::vector<EigDesc>& descs, bool align, Arena& da,
                                   HostImage* img) {
  EigMaps m;
  const int rc = eig_maps(h, l, descs, align, m);
  if (rc != TADMM_OK) return rc;
  place_phase(l.tick, da, img, descs.data(), descs.size() * sizeof(EigDesc), l.neig, m.tick);
  place_map_like(l.norm, l.tick, da, img, m.norm);
  place_map_like(l.ext, l.tick, da, img, m.ext);
  return TADMM_OK;
}

// Runs jacobi_init + sweeps until every problem of the group has its `done` flag.
// Convergence is decided on the device after every sweep (jacobi_conv_kernel sets the sticky per-problem flags,
// so finished problems cost nothing in later launches).  The host only needs "all finished?" and reads that
// verdict one sweep late: the verdict of sweep g (written by the kernel straight into pinned host memory -- no
// copy in the stream) is consumed after sweep g+1 has been queued, so the GPU never idles on a poll; the price
// is one sweep of empty launches at the end.
// Small groups (every problem <= 64 columns) run in ONE launch (jacobi_small_kernel decides convergence itself);
// *small_pending is set and the caller, after queueing the group's finalize launches, calls check_small_group.
// *behind_last_stands (optional) is set when g.behind_last was queued behind the sweep that turned out to be the last:
// the caller then has nothing left to queue for the group.
static inline int run_eig_group(tadmm_handle h, const EigGroup& g, PollCtx& poll, double tol, int max_sweeps, bool debug,
                                hipStream_t s, int* sweeps_out, bool* small_pending, JacobiTiming* jt = nullptr,
                                bool* behind_last_stands = nullptr) {
  const bool super = g.kernel == EigTick::SuperPairs;
  *sweeps_out = 0;
  *small_pending = false;
  if (behind_last_stands) *behind_last_stands = false;
  bool stands = false;
  if (g.neig == 0) return TADMM_OK;
  {
    const char* e = getenv("TADMM_JACOBI_SMALL");     // 0: always use the tick kernels (A/B measurements)
    if (g.npad_max > 0 && jacobi_small_fits(g.npad_max) && !(e && !atoi(e))) {
      const bool timed = jt && jt->on;
      if (timed) (void)hipEventRecord(jt->a, s);
      // direct route first (tridiag.hip); the Jacobi launch behind it skips what that one solved and verified.  The flag
      // words live in the group's `prev` scratch (doubles of the tick path's convergence kernel, unused here).
      int32_t* fast = (g.prev_dev && eig_small_direct_on()) ? reinterpret_cast<int32_t*>(g.prev_dev) : nullptr;
      if (fast) HIP_OK(h, launch_eig_small_direct(g.ed, g.neig, g.skip, fast, poll.host, s));
      HIP_OK(h, launch_jacobi_small(g.ed, g.neig, g.npad_max, tol, std::max(max_sweeps, 60), g.skip, poll.host, s, g.warm, fast));
      if (timed) {
        float ms = 0.f;
        (void)hipEventRecord(jt->b, s);
        (void)hipEventSynchronize(jt->b);
        (void)hipEventElapsedTime(&ms, jt->a, jt->b);
        jt->small_ms += ms; jt->small_launches += 1;
        for (int q = 0; q < g.neig && jt->small_n; ++q) { const double nn = jt->small_n[q]; jt->small_flops += 8.0 * nn * nn * nn; }
      }
      HIP_OK(h, hipEventRecord(poll.ev[0], s));
      *small_pending = true;
      return TADMM_OK;
    }
  }
  launch_jacobi_init(g.ed, g.neig, s, g.skip, g.prev_dev);
  if (g.after_init) g.after_init(s);
  if (g.gsteps == 0) return TADMM_OK;      // every problem is a single block: nothing to rotate
  bool all_done = false;
  int tick = 0, gs = 0, pending = -1, needed = 0;
  std::vector<char> known_done(g.neig, 0);   // what the host has learnt so far (lags the device by a sweep)
  // Rayleigh-Ritz problems of 128 / 192 columns (EigDesc::scratch set by the filter layout): direct route first
  // (tridiag_mid.hip), ONE launch per size instead of ~80; what it solves and verifies has its `done` word set and the
  // tournament below skips it -- if that is every problem of the group the tournament is not queued at all.  The host has
  // to know, so this costs one stream round trip per group.
  if (super && g.mid_sizes && eig_mid_direct_on()) {
    bool any192 = false, any128 = false;
    for (int q = 0; q < g.neig; ++q) { any192 = any192 || g.mid_sizes[q] == 192; any128 = any128 || g.mid_sizes[q] == 128; }
    if (any192 || any128) {
      for (int q = 0; q <= g.neig; ++q) poll.host[q] = 0;
      if (any192) launch_eig_mid_direct(g.ed, g.neig, 192, g.skip, poll.host, s);
      if (any128) launch_eig_mid_direct(g.ed, g.neig, 128, g.skip, poll.host, s);
      HIP_OK(h, hipEventRecord(poll.ev[0], s));
      if (hipEventSynchronize(poll.ev[0]) != hipSuccess) CTX_FAIL(h, TADMM_ERR_HIP, "poll event failed");
      bool every = true;
      for (int q = 0; q < g.neig; ++q) {
        known_done[q] = poll.host[1 + q] != 0;
        every = every && (known_done[q] || g.players[q] < 2);
      }
      if (getenv("TADMM_MID_DEBUG")) {
        int ok = 0, cand = 0;
        for (int q = 0; q < g.neig; ++q) { ok += known_done[q] ? 1 : 0; cand += g.mid_sizes[q] ? 1 : 0; }
        fprintf(stderr, "[tadmm] direct RR route: %d of %d candidates solved (%d problems in the group)\n", ok, cand, g.neig);
      }
      if (every) { *sweeps_out = 0; return TADMM_OK; }
    }
  }
  std::vector<double> h_off;
  std::vector<int> h_done;
  auto consume = [&]() -> int {
    if (pending < 0) return TADMM_OK;
    if (hipEventSynchronize(poll.ev[pending & 1]) != hipSuccess) return TADMM_ERR_HIP;
    const int* v = poll.host + (size_t)(pending & 1) * poll.stride;
    if (v[0]) { all_done = true; needed = pending + 1; }
    for (int q = 0; q < g.neig; ++q) known_done[q] = v[1 + q] != 0;
    pending = -1;
    return TADMM_OK;
  };
  for (; gs < max_sweeps && !all_done; ++gs) {
    for (int t = 0; t < g.gsteps; ++t, ++tick) {
      if (super) {
        const bool timed = jt && jt->on;
        if (timed) (void)hipEventRecord(jt->a, s);
        HIP_OK(h, launch_jacobi_tick3(g.ed, g.tick_map, g.tick_blocks, tick, tol, g.ld_max, s));
        if (timed) {
          float ms = 0.f;
          (void)hipEventRecord(jt->b, s);
          (void)hipEventSynchronize(jt->b);
          (void)hipEventElapsedTime(&ms, jt->a, jt->b);
          jt->tick_ms += ms; jt->tick_launches += 1;
          // executed MFMA work of a workgroup (two 16-column super-blocks, rows of length ld): cross Gram 2*16*16*ld, two
          // rounds of column updates 2 * (2*16*16*ld) each -> 2560*ld; problems the host knows to be finished are left out,
          // workgroups of a padded schedule's idle ticks too
          for (int q = 0; q < g.neig; ++q) {
            if (known_done[q] || g.players[q] < 2) continue;
            const int own = g.players[q] - 1;
            if (g.aligned && (tick % g.gsteps) >= own) continue;
            const double ld = g.row_len ? g.row_len[q] : g.ld_max;
            jt->tick_flops += 2560.0 * ld * (g.players[q] / 2);
            jt->tick_wgs += g.players[q] / 2;
          }
        }
      } else {
        HIP_OK(h, launch_jacobi_tick(g.ed, g.tick_map, g.tick_blocks, tick, tol, g.tick_lds, s));
      }
    }
    launch_jacobi_conv(g.ed, g.neig, tick, tol, super, g.prev_dev, poll.host + (size_t)(gs & 1) * poll.stride, s);
    {   // a failed launch (LDS attribute not set on this device, bad configuration) must surface, not spin to max_sweeps
      const hipError_t le = hipGetLastError();
      if (le != hipSuccess) CTX_FAIL(h, TADMM_ERR_HIP, "Jacobi launch failed: %s", hipGetErrorString(le));
    }
    if (debug && g.off_dev) {
      h_off.resize((size_t)g.neig * 3); h_done.resize(g.neig);
      HIP_OK(h, hipMemcpyAsync(h_off.data(), g.off_dev, (size_t)g.neig * 3 * 8, hipMemcpyDeviceToHost, s));
      HIP_OK(h, hipMemcpyAsync(h_done.data(), g.done_dev, (size_t)g.neig * 4, hipMemcpyDeviceToHost, s));
      HIP_OK(h, hipStreamSynchronize(s));
      double mxo = 0; int nd = 0;
      for (int q = 0; q < g.neig; ++q) {
        const int steps = g.players[q] - 1;
        if (h_done[q]) ++nd;
        if (steps > 0 && tick % steps == 0) mxo = std::max(mxo, h_off[3 * q + ((tick / steps - 1) & 1)]);
      }
      fprintf(stderr, "[tadmm]   sweep %d: max observed off %.3e, done %d/%d\n", gs, mxo, nd, g.neig);
    }
    int rc = consume();                     // verdict of the previous sweep (long since on the host)
    if (rc != TADMM_OK) CTX_FAIL(h, rc, "poll event failed");
    if (all_done) break;
    // The verdict only matters near the end: with a sweep count to go by (the previous run's), the sweeps well before it
    // queue no event (a marker packet costs the chain ~5 us a sweep) and are not polled; a solve that finishes much
    // earlier than last time runs a few sweeps of gated (empty) launches before the host notices.
    static const bool lazy_poll = !(getenv("TADMM_POLL_EVERY_SWEEP") && atoi(getenv("TADMM_POLL_EVERY_SWEEP")));
    // (not in instrumented runs: their flop count leaves out the problems the host KNOWS to be finished)
    if (lazy_poll && !(jt && jt->on) && g.expected > 0 && gs + 3 < g.expected) continue;
    HIP_OK(h, hipEventRecord(poll.ev[gs & 1], s));
    pending = gs;
    if (g.expected > 0 && gs + 1 >= g.expected) {
      // Jacobi needs about the same number of sweeps from one ADMM iteration to the next: from the sweep that
      // was the last one last time, wait for the verdict (one short stall) instead of queueing a sweep of
      // launches that would most likely find every problem finished.  What the caller would queue after the group goes
      // out first (behind the event: the verdict is not delayed), so the GPU has work while the host wakes up; if the
      // verdict says "not all done" the tournament continues and those launches are simply queued again later.
      if (g.behind_last && behind_last_stands) { g.behind_last(s); stands = true; }
      rc = consume();
      if (rc != TADMM_OK) CTX_FAIL(h, rc, "poll event failed");
      if (!all_done) stands = false;
    }
  }
  if (!all_done) {
    const int rc = consume();
    if (rc != TADMM_OK) CTX_FAIL(h, rc, "poll event failed");
  }
  if (debug) {
    int pmax = 0;
    for (int q = 0; q < g.neig; ++q) pmax = std::max(pmax, g.players[q]);
    fprintf(stderr, "[tadmm] eig group: neig=%d players_max=%d ticks/sweep=%d wgs/tick=%d sweeps=%d ticks=%d kernel=%s\n",
            g.neig, pmax, g.gsteps, g.tick_blocks, all_done ? needed : gs, tick, super ? "super-pairs" : "pairs");
  }
  if (!all_done) CTX_FAIL(h, TADMM_ERR_NOCONVERGE, "Jacobi did not converge in %d sweeps", max_sweeps);
  *sweeps_out = needed;
  if (behind_last_stands) *behind_last_stands = stands;
  return TADMM_OK;
}

// The single-launch solver reports per-problem convergence through pinned memory: fail loudly if one hit the cap.
static inline int check_small_group(tadmm_handle h, const EigGroup& g, PollCtx& poll) {
  if (hipEventSynchronize(poll.ev[0]) != hipSuccess) CTX_FAIL(h, TADMM_ERR_HIP, "poll event failed");
  for (int q = 0; q < g.neig; ++q)
    if (!poll.host[1 + q]) CTX_FAIL(h, TADMM_ERR_NOCONVERGE, "Jacobi (small problems) did not converge, problem %d", q);
  return TADMM_OK;
}

}  // namespace tadmm
