// Gram matrix of a TT unfolding on the fp64 matrix cores.
//
//   G = A A^T  (m <= n, reduce over the n columns)      or      G = A^T A  (m > n, reduce over rows)
//
// A is float32; every product of two float32 values is exact in float64 (24+24 <= 53 mantissa
// bits), so v_mfma_f64_16x16x4_f64 gives an *exactly-rounded-per-add* fp64 accumulation of the
// Gram entries -- this is what keeps the Gram + eigen-solve route inside the 1e-5 parity bar
// (SURVEY.md section 7 "Accuracy of the Gram route").
//
// Work decomposition: 32x32 output tiles (upper triangle only, the matrix is symmetric) x split-K.
// One workgroup = 4 waves, each wave owns a quarter of the workgroup's K-chunk and a 2x2 grid of
// 16x16 MFMA tiles; partial tiles are reduced through LDS in a fixed order and written to a
// partial buffer; a second kernel sums the split-K partials (fixed order => deterministic),
// mirrors the triangle and zero-pads to the [Npad][ld] layout the Jacobi solver wants.
//
// MFMA operand maps (cdna_hip_programming.md section 3): A operand lane l holds A[i=l&15][k=l>>4],
// B operand lane l holds B[k=l>>4][j=l&15]; D: col = l&15, row = (l>>4) + 4*reg.
// For a Gram both operands are rows of the same matrix: B[k][j] = X[c0+j][k] has the *same* lane
// map as the A operand of row block c0, so one load serves both roles.
#include "common.h"
#include <type_traits>

namespace tadmm {

typedef double double4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double4_t mfma_f64(double a, double b, double4_t c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// tile-pair index -> (ti, tj), ti <= tj, row-major over the upper triangle
__device__ __forceinline__ void tile_pair(int tp, int nt, int& ti, int& tj) {
  int a = 0, rowlen = nt;
  while (tp >= rowlen) { tp -= rowlen; ++a; --rowlen; }
  ti = a; tj = a + tp;
}

__global__ __launch_bounds__(256) void gram_partial_kernel(const GramDesc* __restrict__ descs,
                                                           const BlockRef* __restrict__ map,
                                                           const int32_t* __restrict__ skip) {
  __shared__ double red[4][4][64 * 4];  // [wave][tile][lane*4+reg]  32 KB
  __shared__ double tile[32][33];       // summed 32x32 tile of the direct (ksplit == 1) path
  const BlockRef br = map[blockIdx.x];
  if (skip && skip[br.prob]) return;
  const GramDesc d = descs[br.prob];
  const int ntp = d.nt * (d.nt + 1) / 2;
  const int ks = br.local / ntp;
  const int tp = br.local - ks * ntp;
  int ti, tj;
  tile_pair(tp, d.nt, ti, tj);
  const bool diag = (ti == tj);
  // (the wave index in a scalar register: the K quarter, and with it every loop bound below, is wave-uniform)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;

  const int kbeg = ks * d.kchunk;
  const int kend = min(d.K, kbeg + d.kchunk);
  // each wave takes a contiguous quarter (multiple of 16) of [kbeg, kend)
  const int per = (((kend - kbeg + 3) / 4) + 15) & ~15;
  const int wk0 = min(kend, kbeg + wave * per);
  const int wk1 = min(kend, wk0 + per);

  double4_t acc00 = {0, 0, 0, 0}, acc01 = {0, 0, 0, 0}, acc10 = {0, 0, 0, 0}, acc11 = {0, 0, 0, 0};
  const G<const float>* A = gp(d.A);
  const int N = d.N;
  const int ra0 = ti * 32 + r, ra1 = ra0 + 16;   // G-rows of this lane for the A role
  const int rb0 = tj * 32 + r, rb1 = rb0 + 16;   // G-rows for the B role
  const float ma0 = ra0 < N ? 1.f : 0.f, ma1 = ra1 < N ? 1.f : 0.f;
  const float mb0 = rb0 < N ? 1.f : 0.f, mb1 = rb1 < N ? 1.f : 0.f;
  const int64_t ld = d.n;
  // G-indices beyond N are clamped to N - 1 (a valid row / column of A) and their values multiplied by 0
  const int ca0 = min(ra0, N - 1), ca1 = min(ra1, N - 1), cb0 = min(rb0, N - 1), cb1 = min(rb1, N - 1);

  struct Chunk { float a0[4], a1[4], b0[4], b1[4]; };   // this lane's 4 reduction indices of a 16-wide k chunk
  const int nfull =(wk1 - wk0) >> 4, rem = (wk1 - wk0) & 15;
  const int ktail = wk0 + 16 * nfull;
  // The wave's K range [wk0, wk1) is nfull whole chunks of 16 and a tail of rem < 16 (wk0 is a multiple of 16: kchunk is
  // one of 64).  Whole chunks are fetched by unconditional loads NPF chunks ahead of their MFMAs -- a wave's chunk is
  // far shorter than a round trip to L2 or HBM, and the plan's launches put one or two workgroups on a CU -- into a ring
  // of register sets with compile-time indices; chunk indices past the end are clamped to the last whole chunk (a few
  // repeated loads) instead of guarding the load, so that the same number of loads is in flight on every path and the
  // waits stay counted.  The tail is fetched first, by 4-byte loads whose k is clamped to wk1 - 1, and consumed last, with
  // +0 where k >= wk1 (selected where it is consumed: a select next to its load becomes a branch around the load).
  // Every address is inside A: a clamped row / column index is < N, and k < wk1 <= K.  A diagonal tile (block-uniform,
  // decided once, outside the loops) loads the A role only.
  auto body = [&](auto diag_tag, auto trans_tag) {
    constexpr bool kDiag = decltype(diag_tag)::value, kTrans = decltype(trans_tag)::value;
    constexpr int NPF = kTrans ? 3 : 4;          // trans: 16 loads per chunk, three chunks stay below the 63 a wave can count
    // 16 fp64 MFMAs per chunk
    auto mma = [&](const Chunk& c) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double da0 = c.a0[e], da1 = c.a1[e];
        const double db0 = kDiag ? da0 : (double)c.b0[e], db1 = kDiag ? da1 : (double)c.b1[e];
        acc00 = mfma_f64(da0, db0, acc00);
        acc01 = mfma_f64(da0, db1, acc01);
        if (!kDiag) acc10 = mfma_f64(da1, db0, acc10);
        acc11 = mfma_f64(da1, db1, acc11);
      }
    };
    // what the loads returned -> what the MFMAs see: rows beyond N times 0, the K tail +0 (applied when a chunk is
    // consumed, so that nothing waits for a load where it is issued).  lane k of element e: see fetch / fetch_tail
    auto cook = [&](const Chunk& c, bool tail) {
      Chunk o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = !tail || (ktail + (kTrans ? 4 * e + q : 4 * q + e)) < wk1;
        o.a0[e] = ok ? c.a0[e] * ma0 : 0.f;
        o.a1[e] = ok ? c.a1[e] * ma1 : 0.f;
        o.b0[e] = (ok && !kDiag) ? c.b0[e] * mb0 : 0.f;
        o.b1[e] = (ok && !kDiag) ? c.b1[e] * mb1 : 0.f;
      }
      return o;
    };
    const G<const float>* pa0 = A + (kTrans ? (int64_t)ca0 : (int64_t)ca0 * ld);
    const G<const float>* pa1 = A + (kTrans ? (int64_t)ca1 : (int64_t)ca1 * ld);
    const G<const float>* pb0 = A + (kTrans ? (int64_t)cb0 : (int64_t)cb0 * ld);
    const G<const float>* pb1 = A + (kTrans ? (int64_t)cb1 : (int64_t)cb1 * ld);
    auto ld4 = [&](float (&o)[4], const G<const float>* p) {
      const f4u t = *reinterpret_cast<const G<const f4u>*>(p);
      o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    };
    // a whole chunk at kk.  Row-contiguous: rows of A are G-indices and the reduction runs along the contiguous dimension;
    // lane (r,q) takes k = kk+4q .. +3 (a permutation of the MFMA k order that both operands share), one 16-byte load per
    // row.  trans: columns of A are G-indices, the reduction runs over rows: lane (r,q) reads A[kk+4e+q][col]
    auto fetch = [&](Chunk& c, int kk) {
      if (!kTrans) {
        const int k = kk + 4 * q;
        ld4(c.a0, pa0 + k); ld4(c.a1, pa1 + k);
        if (!kDiag) { ld4(c.b0, pb0 + k); ld4(c.b1, pb1 + k); }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t ro = (int64_t)(kk + 4 * e + q) * ld;
          c.a0[e] = pa0[ro]; c.a1[e] = pa1[ro];
          if (!kDiag) { c.b0[e] = pb0[ro]; c.b1[e] = pb1[ro]; }
        }
      }
    };
    auto fetch_tail = [&](Chunk& c) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kc = min(ktail + (kTrans ? 4 * e + q : 4 * q + e), wk1 - 1);
        const int64_t o = kTrans ? (int64_t)kc * ld : (int64_t)kc;
        c.a0[e] = pa0[o]; c.a1[e] = pa1[o];
        if (!kDiag) { c.b0[e] = pb0[o]; c.b1[e] = pb1[o]; }
      }
    };
    Chunk tail = {};
    if (rem) fetch_tail(tail);
    if (nfull > 0) {
      const int last = nfull - 1;
      Chunk R[NPF] = {};
#pragma unroll
      for (int u = 0; u < NPF; ++u) fetch(R[u], wk0 + 16 * min(u, last));
      int c = 0;
      for (; c + NPF <= nfull; c += NPF) {
#pragma unroll
        for (int u = 0; u < NPF; ++u) {
          const Chunk cur = cook(R[u], false);
          fetch(R[u], wk0 + 16 * min(c + u + NPF, last));
          __builtin_amdgcn_sched_barrier(0);   // the loads go out before the MFMAs
          mma(cur);
        }
      }
#pragma unroll
      for (int u = 0; u < NPF - 1; ++u)          // chunks c .. nfull - 1 sit in R[0], R[1], ...
        if (c + u < nfull) mma(cook(R[u], false));
    }
    if (rem) mma(cook(tail, true));
  };
  using T = std::true_type;
  using F = std::false_type;
  if (!d.trans) { if (diag) body(T(), F()); else body(F(), F()); }
  else          { if (diag) body(T(), T()); else body(F(), T()); }

  // cross-wave reduction in a fixed order
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[wave][0][lane * 4 + e] = acc00[e];
    red[wave][1][lane * 4 + e] = acc01[e];
    red[wave][2][lane * 4 + e] = acc10[e];
    red[wave][3][lane * 4 + e] = acc11[e];
  }
  __syncthreads();
  if (d.ksplit > 1) {
    double* out = d.partial + ((int64_t)ks * ntp + tp) * 1024;
    for (int idx = threadIdx.x; idx < 1024; idx += 256) {
      const int t = idx >> 8, le = idx & 255;        // tile, lane*4+reg
      const double v = (red[0][t][le] + red[1][t][le]) + (red[2][t][le] + red[3][t][le]);
      const int l = le >> 2, reg = le & 3;
      const int row = (t >> 1) * 16 + (l >> 4) + 4 * reg;
      const int col = (t & 1) * 16 + (l & 15);
      out[row * 32 + col] = v;
    }
    return;
  }
  // direct path (no split-K): this workgroup owns the whole reduction, so it writes the tile and its mirror
  // straight into the zero-padded [Npad][ld] image of the eigen-solver (Npad = 32*nt)
  for (int idx = threadIdx.x; idx < 1024; idx += 256) {
    const int t = idx >> 8, le = idx & 255;
    if (diag && t == 2) continue;                    // lower-left block of a diagonal tile = mirror of block 1
    const double v = (red[0][t][le] + red[1][t][le]) + (red[2][t][le] + red[3][t][le]);
    const int l = le >> 2, reg = le & 3;
    const int row = (t >> 1) * 16 + (l >> 4) + 4 * reg;
    const int col = (t & 1) * 16 + (l & 15);
    tile[row][col] = v;
    if (diag && t == 1) tile[col][row] = v;
  }
  __syncthreads();
  double* __restrict__ G = d.G;
  const int64_t gld = d.ld;
  for (int e = threadIdx.x; e < 1024; e += 256) {
    const int rr = e >> 5, cc = e & 31;
    G[(int64_t)(ti * 32 + rr) * gld + tj * 32 + cc] = tile[rr][cc];
    if (!diag) G[(int64_t)(tj * 32 + rr) * gld + ti * 32 + cc] = tile[cc][rr];
  }
  if (tj == d.nt - 1) {                              // zero the padding columns [Npad, ld) of row block ti
    const int padw = d.ld - d.Npad;
    for (int e = threadIdx.x; e < 32 * padw; e += 256) {
      const int rr = e / padw, cc = e - rr * padw;
      G[(int64_t)(ti * 32 + rr) * gld + d.Npad + cc] = 0.0;
    }
  }
}

// sum split-K partials, mirror, zero-pad.  local block = chunk of 1024 outputs of the [Npad][ld] image
__global__ __launch_bounds__(256) void gram_reduce_kernel(const GramDesc* __restrict__ descs,
                                                          const BlockRef* __restrict__ map,
                                                          const int32_t* __restrict__ skip) {
  const G<const BlockRef>* brp = gp(map + blockIdx.x);
  const int prob = brp->prob, local = brp->local;
  const G<const GramDesc>* d = gp(descs + prob);
  // (the descriptor goes out beside the skip word: both are scalar loads behind the map entry)
  const int nt = d->nt, N = d->N, Npad = d->Npad, ld = d->ld, ksplit = d->ksplit;
  const G<const double>* partial = gp((const double*)d->partial);
  G<double>* Gout = gp(d->G);
  if (skip && gp(skip)[prob]) return;
  const int ntp = nt * (nt + 1) / 2;
  const int64_t total = (int64_t)Npad * ld;
  const int64_t base = (int64_t)local * 1024;
  const int64_t stride = (int64_t)ntp * 1024;
  const bool small = total <= 0x7fffffff;            // uniform: split the index with 32-bit arithmetic
  // A thread's four outputs are independent: the partial loads of all four go out before the first add.  An output of
  // the padding (or past the image) reads the first partial instead and its adds are skipped.
  const G<const double>* p[4];
  bool live[4];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int64_t idx = base + threadIdx.x + 256 * o;
    const int j = small ? (int)((uint32_t)idx / (uint32_t)ld) : (int)(idx / ld);
    const int i = (int)(idx - (int64_t)j * ld);
    live[o] = idx < total && j < N && i < N;
    int a = j >> 5, b = i >> 5, jr = j & 31, ir = i & 31;
    if (a > b) { int s = a; a = b; b = s; s = jr; jr = ir; ir = s; }
    if (a == b && jr > ir) { const int s = jr; jr = ir; ir = s; }   // diagonal tiles: upper part only
    const int tp = a * nt - (a * (a - 1)) / 2 + (b - a);
    p[o] = live[o] ? partial + (int64_t)tp * 1024 + jr * 32 + ir : partial;
  }
  int ks = 0;
  for (; ks + 8 <= ksplit; ks += 8) {                // the order of the adds is fixed
    double t[4][8];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int u = 0; u < 8; ++u) t[o][u] = p[o][(ks + u) * stride];
#pragma unroll
    for (int o = 0; o < 4; ++o)
      v[o] += ((t[o][0] + t[o][1]) + (t[o][2] + t[o][3])) + ((t[o][4] + t[o][5]) + (t[o][6] + t[o][7]));
  }
  if (ks < ksplit) {                                 // up to seven more, one by one in order: loads on clamped chunks
    double t[4][7];
    const int n = ksplit - ks;
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int u = 0; u < 7; ++u) t[o][u] = p[o][(ks + min(u, n - 1)) * stride];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int u = 0; u < 7; ++u) v[o] = u < n ? v[o] + t[o][u] : v[o];
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int64_t idx = base + threadIdx.x + 256 * o;
    if (idx < total) Gout[idx] = live[o] ? v[o] : 0.0;
  }
}

void launch_gram_partial(const GramDesc* descs_dev, const BlockRef* map_dev, int nblocks, hipStream_t s,
                         const int32_t* skip) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(gram_partial_kernel, dim3(nblocks), dim3(256), 0, s, descs_dev, map_dev, skip);
}

void launch_gram_reduce(const GramDesc* descs_dev, const BlockRef* map_dev, int nblocks, hipStream_t s,
                        const int32_t* skip) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(nblocks), dim3(256), 0, s, descs_dev, map_dev, skip);
}

}  // namespace tadmm
