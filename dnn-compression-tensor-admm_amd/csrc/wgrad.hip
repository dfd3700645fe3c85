// Weight gradients of the factorised layers:  C[m][n] = alpha * sum_{t < T} A[t][m] * B[t][n],  fp32 result.
//
// m, n are a rank and a channel count (18 x 24 ... 256 x 2048), T is tokens or batch * pixels (10^4 ... 2 * 10^5): a
// small output and a very long reduction.  A and B are read IN PLACE, both fp32 or both bf16, both in one layout:
//   token rows          A (T, M) with row stride lda, B (T, N) with row stride ldb           (hw == 0)
//   channels-first      A (batch, M, hw pixels), B (batch, N, hw pixels), t = (batch, pixel)  (hw > 0)
//
// Matrix cores as in chain.hip: the reduction index t is the MFMA K index (v_mfma_f32_16x16x32_bf16), one plane for
// bf16 operands (bf16 x bf16 is exact in fp32), the exact three-plane split and the six kept plane pairs, smallest
// first, for fp32 operands (split2<3> / mma_step of chain_common.h).
//
// Grid = (output tiles) x (slices of T).  A workgroup (4 waves) owns one TM x TN tile (TM, TN in {16, 32, 64}) over one
// slice, walked in chunks of 128 tokens: global -> registers (the next chunk is requested before the MFMAs of this one)
// -> split into planes -> LDS image [plane][feature][128 tokens + pad], read back as MFMA fragments (8 consecutive
// tokens of one feature, one ds_read_b128).  In the image layout memory already lies that way (16-byte loads along the
// pixels); token rows are TURNED ON THE LDS WRITE: a thread loads the same 16 bytes of features for two consecutive
// tokens and writes one 32-bit (token, token + 1) pair per feature and plane, so that both layouts share one fragment
// read path and the split is done once per element.  Loads are 16 bytes where base and stride allow, 8 bytes where
// they allow that (rows of 10 floats, planes of 196 bf16 pixels), single elements otherwise; tiles may cross image
// boundaries.
// Waves split the tile's 16 x 16 subtiles and the chunk's four k-steps (WgradSplit): a wave holds at most four subtiles
// (2 x 2; 1 x 4 or 4 x 1 for the 16 x 64 and 64 x 16 tiles); tiles of up to four subtiles give every wave the whole tile
// and one k-step of four, 64 x 32 / 32 x 64 two waves per half and two k-steps each, 64 x 64 one quadrant per wave.  The
// k-split waves are summed through LDS in fixed order.  The MFMA accumulator is folded into a second
// register set every 8 chunks (1024 tokens of the slice) so that equal-signed products do not build a rounding bias.
//
// Deterministic, no atomics: with one slice the workgroup writes C; otherwise it writes its tile to the caller's
// workspace (plain 16-byte stores, every word of the workspace that is read was written by this call) and
// wgrad_reduce_kernel adds the slices of each entry in fixed order, in fp64, and rounds once.
#include "chain_common.h"
#include "host.h"

namespace tadmm {
namespace {

constexpr int kWgKC = 128;               // tokens per chunk
constexpr int kWgLD = kWgKC + kPad;      // LDS row of one feature: 68 words = 4 mod 64 banks
constexpr int kWgFold = 8;               // chunks between two folds of the MFMA accumulator
constexpr int kWgMinSlice = 256;         // a slice is never shorter than this many tokens
constexpr int kWgTargetWG = 512;         // two workgroups per CU
constexpr int kWgMaxTiles = 1 << 20;

struct WgradArgs {
  const void* A; const void* B; float* C; float* part;
  int64_t lda, ldb, ldc;
  int32_t T, M, N, hw;
  int32_t tiles_n, tiles, slices, nchunks;
  int32_t vec_a, vec_b;                  // 2: 16-byte loads, 1: 8-byte loads, 0: single elements
  float alpha;
};

__device__ __forceinline__ uint32_t word_of(const uint4& r, int j) { return j == 0 ? r.x : j == 1 ? r.y : j == 2 ? r.z : r.w; }
// element j of a 16-byte register image: raw bits of a float, or a bf16 in the low half
template <typename TIn> __device__ __forceinline__ uint32_t elem_of(const uint4& r, int j) {
  if constexpr (sizeof(TIn) == 4) return word_of(r, j);
  else return (word_of(r, j >> 1) >> (16 * (j & 1))) & 0xffffu;
}
// EPL elements gathered one by one (src(j) returns the raw bits of element j, 0 where it does not exist)
template <typename TIn, typename F> __device__ __forceinline__ uint4 gather(F src) {
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (sizeof(TIn) == 4) w[j] = src(j);
    else { const uint32_t lo = src(2 * j), hi = src(2 * j + 1); w[j] = lo | (hi << 16); }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ uint32_t raw_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t raw_bits(uint16_t v) { return v; }

// One operand's F features x 128 tokens of a chunk: global -> registers (load), registers -> planes -> LDS (store).
template <int P, int F, typename TIn, bool IMG> struct WgradLoader {
  static constexpr int EPL = 16 / sizeof(TIn);
  static constexpr int FV = F / EPL;                                       // 16-byte feature groups of a token row
  static constexpr int UNITS = IMG ? F * (kWgKC / EPL) : (kWgKC / 2) * FV;
  static constexpr int NU = (UNITS + 255) / 256;
  static constexpr int NR = IMG ? 1 : 2;                                   // rows: tokens t and t + 1
  uint4 regs[NU][NR];

  // EPL elements starting at p; `n` of them exist (the rest read as zero)
  static __device__ __forceinline__ uint4 fetch(const TIn* p, int vec, int n) {
    if (n >= EPL && vec == 2) return *reinterpret_cast<const uint4*>(p);
    if (n >= EPL && vec == 1) {
      const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + EPL / 2);
      return make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
    return gather<TIn>([&](int j) -> uint32_t { return j < n ? raw_bits(p[j]) : 0u; });
  }

  __device__ __forceinline__ void load(const TIn* X, int64_t ld, int hw, int nfeat, int f0, int t0, int tend, int vec,
                                       int tid) {
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int v = tid + 256 * i;
      if constexpr (IMG) {                                                 // EPL consecutive pixels of one channel
        const int c = f0 + v / (kWgKC / EPL);
        const int t = t0 + (v % (kWgKC / EPL)) * EPL;
        uint4 r = make_uint4(0, 0, 0, 0);
        if (c < nfeat && t < tend) {
          uint32_t b = (uint32_t)t / (uint32_t)hw, p = (uint32_t)t - b * (uint32_t)hw;
          const TIn* src = X + ((int64_t)b * nfeat + c) * hw + p;
          if (vec == 2) {                                                  // hw % EPL == 0: never leaves the plane
            r = *reinterpret_cast<const uint4*>(src);
          } else if (vec == 1) {                                           // hw % (EPL/2) == 0: two halves
            const uint2 lo = *reinterpret_cast<const uint2*>(src);
            uint2 hi = make_uint2(0, 0);
            if (t + EPL / 2 < tend) {
              p += EPL / 2;
              if (p >= (uint32_t)hw) { p = 0; ++b; }
              hi = *reinterpret_cast<const uint2*>(X + ((int64_t)b * nfeat + c) * hw + p);
            }
            r = make_uint4(lo.x, lo.y, hi.x, hi.y);
          } else {
            r = gather<TIn>([&](int j) -> uint32_t {           // called for j = 0, 1, .. in order
              const uint32_t e = (t + j < tend) ? raw_bits(X[((int64_t)b * nfeat + c) * hw + p]) : 0u;
              if (++p >= (uint32_t)hw) { p = 0; ++b; }
              return e;
            });
          }
        }
        regs[i][0] = r;
      } else {                                                             // EPL consecutive features of tokens t, t+1
        const int tp = (v / (8 * FV)) * 8 + (v & 7), fv = (v >> 3) % FV;
        const int c = f0 + fv * EPL;
        const int t = t0 + 2 * tp;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          uint4 r = make_uint4(0, 0, 0, 0);
          if (v < UNITS && c < nfeat && t + h < tend) r = fetch(X + (int64_t)(t + h) * ld + c, vec, nfeat - c);
          regs[i][h] = r;
        }
      }
    }
  }

  __device__ __forceinline__ void store(uint16_t* S, int tid) const {      // S: [P][F][kWgLD]
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int v = tid + 256 * i;
      if constexpr (IMG) {
        const int f = v / (kWgKC / EPL), tk = (v % (kWgKC / EPL)) * EPL;
        if constexpr (P == 1) {
          *reinterpret_cast<uint4*>(&S[f * kWgLD + tk]) = regs[i][0];
        } else {
          const uint4 v4 = regs[i][0];
          uint32_t s0[P], s1[P];
          split2<P>(__builtin_bit_cast(float, v4.x), __builtin_bit_cast(float, v4.y), s0);
          split2<P>(__builtin_bit_cast(float, v4.z), __builtin_bit_cast(float, v4.w), s1);
#pragma unroll
          for (int p = 0; p < P; ++p) *reinterpret_cast<uint2*>(&S[(p * F + f) * kWgLD + tk]) = make_uint2(s0[p], s1[p]);
        }
      } else {
        const int tp = (v / (8 * FV)) * 8 + (v & 7), fv = (v >> 3) % FV;
        if (v < UNITS) {
          if constexpr (P == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              *reinterpret_cast<uint32_t*>(&S[(fv * 8 + j) * kWgLD + 2 * tp]) =
                  elem_of<TIn>(regs[i][0], j) | (elem_of<TIn>(regs[i][1], j) << 16);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              uint32_t s[P];
              split2<P>(__builtin_bit_cast(float, word_of(regs[i][0], j)), __builtin_bit_cast(float, word_of(regs[i][1], j)), s);
#pragma unroll
              for (int p = 0; p < P; ++p) *reinterpret_cast<uint32_t*>(&S[(p * F + fv * 4 + j) * kWgLD + 2 * tp]) = s[p];
            }
          }
        }
      }
    }
  }
};

// fragments of S subtiles (16 features each, from subtile sub0) at k-step ks of an LDS image [P][F][kWgLD]
template <int P, int S, int F>
__device__ __forceinline__ void wgrad_frags(bf16x8_t (&f)[P][S], const uint16_t* img, int sub0, int ks, int r, int q) {
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int s = 0; s < S; ++s)
      f[p][s] = *reinterpret_cast<const bf16x8_t*>(&img[(p * F + 16 * (sub0 + s) + r) * kWgLD + 32 * ks + 8 * q]);
}

template <int TM, int TN> struct WgradSplit {
  static constexpr int SUB = (TM / 16) * (TN / 16);
  static constexpr int WM = (SUB >= 8 && TM == 64) ? 2 : 1;
  static constexpr int WN = (SUB == 16 || (SUB == 8 && TM != 64)) ? 2 : 1;
  static constexpr int WK = 4 / (WM * WN);
  static constexpr int MS = TM / 16 / WM, NS = TN / 16 / WN;
};

template <int P, int TM, int TN> constexpr size_t wgrad_lds_bytes() { return (size_t)P * (TM + TN) * kWgLD * 2; }

template <int P, int TM, int TN, typename TIn, bool IMG>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs d) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  using SP = WgradSplit<TM, TN>;
  constexpr int WM = SP::WM, WK = SP::WK, MS = SP::MS, NS = SP::NS, SUB = SP::SUB;
  static_assert(wgrad_lds_bytes<P, TM, TN>() >= (size_t)4 * MS * NS * 1024, "k-split reduction reuses the tile image");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int wk = wave % WK, wm = (wave / WK) % WM, wn = wave / (WK * WM);
  const int tile = blockIdx.x % d.tiles, slice = blockIdx.x / d.tiles;
  const int m0 = (tile / d.tiles_n) * TM, n0 = (tile % d.tiles_n) * TN;
  const int c_begin = (int)((int64_t)slice * d.nchunks / d.slices);
  const int c_end = (int)((int64_t)(slice + 1) * d.nchunks / d.slices);
  const int tend = min(d.T, c_end * kWgKC);
  const TIn* A = static_cast<const TIn*>(d.A);
  const TIn* B = static_cast<const TIn*>(d.B);
  uint16_t* As = lds;                                   // [P][TM][kWgLD]
  uint16_t* Bs = lds + P * TM * kWgLD;                  // [P][TN][kWgLD]

  float4v_t acc[NS][MS], tot[NS][MS];
#pragma unroll
  for (int ns = 0; ns < NS; ++ns)
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) acc[ns][ms] = tot[ns][ms] = float4v_t{0.f, 0.f, 0.f, 0.f};

  WgradLoader<P, TM, TIn, IMG> la;
  WgradLoader<P, TN, TIn, IMG> lb;
  if (c_begin < c_end) {
    la.load(A, d.lda, d.hw, d.M, m0, c_begin * kWgKC, tend, d.vec_a, tid);
    lb.load(B, d.ldb, d.hw, d.N, n0, c_begin * kWgKC, tend, d.vec_b, tid);
  }
  for (int c = c_begin; c < c_end; ++c) {
    __syncthreads();                                    // the fragment reads of the previous chunk are done
    la.store(As, tid);
    lb.store(Bs, tid);
    __syncthreads();
    if (c + 1 < c_end) {                                // workgroup-uniform: the last trip requests nothing
      la.load(A, d.lda, d.hw, d.M, m0, (c + 1) * kWgKC, tend, d.vec_a, tid);
      lb.load(B, d.ldb, d.hw, d.N, n0, (c + 1) * kWgKC, tend, d.vec_b, tid);
    }
#pragma unroll
    for (int ks = 0; ks < kWgKC / 32 / WK; ++ks) {
      bf16x8_t af[P][MS], bfr[P][NS];
      wgrad_frags<P, MS, TM>(af, As, wm * MS, ks * WK + wk, r, q);
      wgrad_frags<P, NS, TN>(bfr, Bs, wn * NS, ks * WK + wk, r, q);
      mma_step<P, NS, MS>(bfr, af, acc);                // acc[ns][ms][e] = C[16 ms + 4 q + e][16 ns + r]
    }
    if (((c - c_begin) & (kWgFold - 1)) == kWgFold - 1) {
#pragma unroll
      for (int ns = 0; ns < NS; ++ns)
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) {
          tot[ns][ms] += acc[ns][ms];
          acc[ns][ms] = float4v_t{0.f, 0.f, 0.f, 0.f};
        }
    }
  }
#pragma unroll
  for (int ns = 0; ns < NS; ++ns)
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) tot[ns][ms] += acc[ns][ms];

  if constexpr (WK > 1) {                               // k-split waves: summed by wave wk == 0 in the order 0, 1, ..
    __syncthreads();
    float4v_t* red = reinterpret_cast<float4v_t*>(lds);
    if (wk != 0) {
#pragma unroll
      for (int ns = 0; ns < NS; ++ns)
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) red[(wave * NS * MS + ns * MS + ms) * 64 + lane] = tot[ns][ms];
    }
    __syncthreads();
    if (wk != 0) return;
#pragma unroll
    for (int k = 1; k < WK; ++k)
#pragma unroll
      for (int ns = 0; ns < NS; ++ns)
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) tot[ns][ms] += red[((wave + k) * NS * MS + ns * MS + ms) * 64 + lane];
  }

#pragma unroll
  for (int ns = 0; ns < NS; ++ns)
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) {
      const int gms = wm * MS + ms, gns = wn * NS + ns;
      if (d.slices == 1) {
        const int n = n0 + 16 * gns + r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = m0 + 16 * gms + 4 * q + e;
          if (m < d.M && n < d.N) d.C[(int64_t)m * d.ldc + n] = d.alpha * tot[ns][ms][e];
        }
      } else {
        float4v_t* dst = reinterpret_cast<float4v_t*>(d.part) +
                         (((int64_t)slice * d.tiles + tile) * SUB + gms * (TN / 16) + gns) * 64 + lane;
        *dst = tot[ns][ms];
      }
    }
}

// C[m][n] = alpha * sum over the slices, in slice order within each of 8 lanes, the 8 lanes in a fixed tree; fp64.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const WgradArgs d, int TM, int TN) {
  const int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int j = threadIdx.x & 7;
  const int64_t total = (int64_t)d.M * d.N;
  const bool valid = idx < total;
  const int64_t id = valid ? idx : total - 1;
  const int m = (int)(id / d.N), n = (int)(id - (int64_t)m * d.N);
  const int sub_n = TN / 16, SUB = (TM / 16) * sub_n;
  const int tile = (m / TM) * d.tiles_n + n / TN;
  const int ml = m % TM, nl = n % TN;
  const int64_t off = ((int64_t)tile * SUB + (ml / 16) * sub_n + nl / 16) * 256 + (((ml & 15) >> 2) * 16 + (nl & 15)) * 4 + (ml & 3);
  const int64_t stride = (int64_t)d.tiles * SUB * 256;
  double s = 0.0;
  for (int sl = j; sl < d.slices; sl += 8) s += (double)d.part[sl * stride + off];
  s += __shfl_xor(s, 4, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 1, 64);
  if (valid && j == 0) d.C[(int64_t)m * d.ldc + n] = (float)((double)d.alpha * s);
}

struct WgradGeom {
  int TM = 16, TN = 16, tiles_m = 1, tiles_n = 1, tiles = 1, slices = 1, nchunks = 0;
  size_t ws_bytes = 0;
};

// Largest tile of {64, 32, 16} that pads the side by at most 1/8 more than 16-wide tiles would.
int wgrad_tile(int m) {
  const int64_t p16 = ((int64_t)m + 15) / 16 * 16;
  for (int t = 64; t >= 32; t /= 2) {
    const int64_t padded = ((int64_t)m + t - 1) / t * t;
    if (padded * 8 <= p16 * 9) return t;
  }
  return 16;
}

int wgrad_geom(tadmm_handle h, const tadmm_wgrad_desc* d, WgradGeom& g) {
  if (!d) CTX_FAIL(h, TADMM_ERR_INVALID, "wgrad: null descriptor");
  if (d->M <= 0 || d->N <= 0 || d->T < 0 || d->hw < 0)
    CTX_FAIL(h, TADMM_ERR_INVALID, "wgrad: M = %d, N = %d, T = %lld, hw = %d", d->M, d->N, (long long)d->T, d->hw);
  if (d->dtype != TADMM_CHAIN_F32 && d->dtype != TADMM_CHAIN_BF16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "wgrad: unknown dtype %d", d->dtype);
  const uintptr_t esz = d->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  if (d->T > 0 && (!d->A || !d->B)) CTX_FAIL(h, TADMM_ERR_INVALID, "wgrad: null operand");
  if (((uintptr_t)d->A | (uintptr_t)d->B) & (esz - 1)) CTX_FAIL(h, TADMM_ERR_INVALID, "wgrad: misaligned operand");
  if (d->hw > 0 && d->T % d->hw) CTX_FAIL(h, TADMM_ERR_INVALID, "wgrad: T = %lld is not whole images of %d pixels", (long long)d->T, d->hw);
  if (d->hw == 0 && d->T > 0 && (d->lda < d->M || d->ldb < d->N))
    CTX_FAIL(h, TADMM_ERR_INVALID, "wgrad: row stride below the feature count");
  if (d->T > INT32_MAX - 2 * kWgKC) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "wgrad: T = %lld exceeds the launch", (long long)d->T);
  g.TM = wgrad_tile(d->M);
  g.TN = wgrad_tile(d->N);
  g.tiles_m = (d->M + g.TM - 1) / g.TM;
  g.tiles_n = (d->N + g.TN - 1) / g.TN;
  const int64_t tiles = (int64_t)g.tiles_m * g.tiles_n;
  if (tiles > kWgMaxTiles) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "wgrad: %lld output tiles exceed the launch", (long long)tiles);
  g.tiles = (int)tiles;
  g.nchunks = (int)((d->T + kWgKC - 1) / kWgKC);
  // slices: enough to reach two workgroups per CU, none shorter than kWgMinSlice tokens; a function of (M, N, T) alone
  int64_t s = (kWgTargetWG + tiles - 1) / tiles;
  s = std::min<int64_t>(s, d->T / kWgMinSlice);
  g.slices = (int)std::max<int64_t>(s, 1);
  g.ws_bytes = g.slices > 1 ? (size_t)g.slices * g.tiles * g.TM * g.TN * sizeof(float) : 0;
  return TADMM_OK;
}

// Tiles above 64 KiB of LDS need the dynamic-LDS opt-in (host.h); a refusal is reported with the size.
template <int P, int TM, int TN, typename TIn, bool IMG>
hipError_t wgrad_launch(const WgradArgs& a, hipStream_t s, size_t* lds_out) {
  auto kern = wgrad_kernel<P, TM, TN, TIn, IMG>;
  constexpr size_t lds = wgrad_lds_bytes<P, TM, TN>();
  *lds_out = lds;
  if (lds > 64 * 1024) {
    static DynLdsOptIn allow_lds;
    const hipError_t e = allow_lds(kern, lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles * a.slices), dim3(256), lds, s, a);
  return hipGetLastError();
}

template <int P, typename TIn, bool IMG, int TM>
hipError_t wgrad_launch_tn(const WgradArgs& a, int TN, hipStream_t s, size_t* lds) {
  if (TN == 64) return wgrad_launch<P, TM, 64, TIn, IMG>(a, s, lds);
  if (TN == 32) return wgrad_launch<P, TM, 32, TIn, IMG>(a, s, lds);
  return wgrad_launch<P, TM, 16, TIn, IMG>(a, s, lds);
}
template <int P, typename TIn, bool IMG>
hipError_t wgrad_launch_tile(const WgradArgs& a, int TM, int TN, hipStream_t s, size_t* lds) {
  if (TM == 64) return wgrad_launch_tn<P, TIn, IMG, 64>(a, TN, s, lds);
  if (TM == 32) return wgrad_launch_tn<P, TIn, IMG, 32>(a, TN, s, lds);
  return wgrad_launch_tn<P, TIn, IMG, 16>(a, TN, s, lds);
}

// widest load the operand allows: 16 bytes, 8 bytes or single elements
int wgrad_vec(const void* p, int64_t step_elems, int esz) {
  const int epl = 16 / esz;
  if (((uintptr_t)p & 15) == 0 && step_elems % epl == 0) return 2;
  if (((uintptr_t)p & 7) == 0 && step_elems % (epl / 2) == 0) return 1;
  return 0;
}


// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient of the k x k core convolution (coreconv.hip):
//   dWc[r2][r1][ky][kx] = sum_{b, oy, ox} dY[b][r2][oy][ox] * X[b][r1][oy*sh - ph + ky*dh][ox*sw - pw + kx*dw]
// The scheme above with t = (b, oy, ox), A = dY read by the image loader and B = X read by a TAP-SHIFTED image loader
// (the pixel a tap reaches from output pixel t, zero outside the image); the tap is blockIdx.y, so every (tap, tile,
// slice) is one workgroup and the result goes to dWc + tap with column stride kh * kw.  Same slices, same fold of the
// accumulator every 1024 tokens, same fixed-order fp64 reduce.
struct CoreWgradArgs {
  WgradArgs g;                            // A = dY, B = X, C = dWc, M = R2, N = R1, hw = Ho * Wo, T = B * Ho * Wo
  int32_t H, W, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw;
};

template <int P, int F, typename TIn> struct TapLoader {
  using Base = WgradLoader<P, F, TIn, true>;
  static constexpr int EPL = Base::EPL;
  Base base;                              // its register image and its LDS store

  __device__ __forceinline__ void load(const TIn* X, const CoreWgradArgs& d, int ky, int kx, int f0, int t0, int tend, int tid) {
    const int nfeat = d.g.N;
    const int64_t plane = (int64_t)d.H * d.W;
#pragma unroll
    for (int i = 0; i < Base::NU; ++i) {
      const int v = tid + 256 * i;
      const int c = f0 + v / (kWgKC / EPL);
      const int t = t0 + (v % (kWgKC / EPL)) * EPL;
      uint4 r = make_uint4(0, 0, 0, 0);
      if (c < nfeat && t < tend) {
        uint32_t b = (uint32_t)t / (uint32_t)d.g.hw;
        const uint32_t p = (uint32_t)t - b * (uint32_t)d.g.hw;
        int oy = (int)(p / (uint32_t)d.Wo), ox = (int)p - oy * d.Wo;
        r = gather<TIn>([&](int j) -> uint32_t {                 // called for j = 0, 1, .. in order
          const int iy = oy * d.sh - d.ph + ky * d.dh, ix = ox * d.sw - d.pw + kx * d.dw;
          uint32_t e = 0u;
          if (t + j < tend && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W)
            e = raw_bits(X[((int64_t)b * nfeat + c) * plane + (int64_t)iy * d.W + ix]);
          if (++ox == d.Wo) { ox = 0; if (++oy == d.Ho) { oy = 0; ++b; } }
          return e;
        });
      }
      base.regs[i][0] = r;
    }
  }
  __device__ __forceinline__ void store(uint16_t* S, int tid) const { base.store(S, tid); }
};

template <int P, int TM, int TN, typename TIn>
__global__ __launch_bounds__(256) void core_wgrad_kernel(const CoreWgradArgs cd) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  using SP = WgradSplit<TM, TN>;
  constexpr int WM = SP::WM, WK = SP::WK, MS = SP::MS, NS = SP::NS, SUB = SP::SUB;
  static_assert(wgrad_lds_bytes<P, TM, TN>() >= (size_t)4 * MS * NS * 1024, "k-split reduction reuses the tile image");
  const WgradArgs& d = cd.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int wk = wave % WK, wm = (wave / WK) % WM, wn = wave / (WK * WM);
  const int tile = blockIdx.x % d.tiles, slice = blockIdx.x / d.tiles;
  const int tap = blockIdx.y, taps = cd.kh * cd.kw;
  const int ky = tap / cd.kw, kx = tap - ky * cd.kw;
  const int m0 = (tile / d.tiles_n) * TM, n0 = (tile % d.tiles_n) * TN;
  const int c_begin = (int)((int64_t)slice * d.nchunks / d.slices);
  const int c_end = (int)((int64_t)(slice + 1) * d.nchunks / d.slices);
  const int tend = min(d.T, c_end * kWgKC);
  const TIn* A = static_cast<const TIn*>(d.A);
  const TIn* B = static_cast<const TIn*>(d.B);
  uint16_t* As = lds;                                   // [P][TM][kWgLD]
  uint16_t* Bs = lds + P * TM * kWgLD;                  // [P][TN][kWgLD]

  float4v_t acc[NS][MS], tot[NS][MS];
#pragma unroll
  for (int ns = 0; ns < NS; ++ns)
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) acc[ns][ms] = tot[ns][ms] = float4v_t{0.f, 0.f, 0.f, 0.f};

  WgradLoader<P, TM, TIn, true> la;
  TapLoader<P, TN, TIn> lb;
  if (c_begin < c_end) {
    la.load(A, 0, d.hw, d.M, m0, c_begin * kWgKC, tend, d.vec_a, tid);
    lb.load(B, cd, ky, kx, n0, c_begin * kWgKC, tend, tid);
  }
  for (int c = c_begin; c < c_end; ++c) {
    __syncthreads();                                    // the fragment reads of the previous chunk are done
    la.store(As, tid);
    lb.store(Bs, tid);
    __syncthreads();
    if (c + 1 < c_end) {                                // workgroup-uniform: the last trip requests nothing
      la.load(A, 0, d.hw, d.M, m0, (c + 1) * kWgKC, tend, d.vec_a, tid);
      lb.load(B, cd, ky, kx, n0, (c + 1) * kWgKC, tend, tid);
    }
#pragma unroll
    for (int ks = 0; ks < kWgKC / 32 / WK; ++ks) {
      bf16x8_t af[P][MS], bfr[P][NS];
      wgrad_frags<P, MS, TM>(af, As, wm * MS, ks * WK + wk, r, q);
      wgrad_frags<P, NS, TN>(bfr, Bs, wn * NS, ks * WK + wk, r, q);
      mma_step<P, NS, MS>(bfr, af, acc);                // acc[ns][ms][e] = C[16 ms + 4 q + e][16 ns + r]
    }
    if (((c - c_begin) & (kWgFold - 1)) == kWgFold - 1) {
#pragma unroll
      for (int ns = 0; ns < NS; ++ns)
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) {
          tot[ns][ms] += acc[ns][ms];
          acc[ns][ms] = float4v_t{0.f, 0.f, 0.f, 0.f};
        }
    }
  }
#pragma unroll
  for (int ns = 0; ns < NS; ++ns)
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) tot[ns][ms] += acc[ns][ms];

  if constexpr (WK > 1) {                               // k-split waves: summed by wave wk == 0 in the order 0, 1, ..
    __syncthreads();
    float4v_t* red = reinterpret_cast<float4v_t*>(lds);
    if (wk != 0) {
#pragma unroll
      for (int ns = 0; ns < NS; ++ns)
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) red[(wave * NS * MS + ns * MS + ms) * 64 + lane] = tot[ns][ms];
    }
    __syncthreads();
    if (wk != 0) return;
#pragma unroll
    for (int k = 1; k < WK; ++k)
#pragma unroll
      for (int ns = 0; ns < NS; ++ns)
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) tot[ns][ms] += red[((wave + k) * NS * MS + ns * MS + ms) * 64 + lane];
  }

#pragma unroll
  for (int ns = 0; ns < NS; ++ns)
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) {
      const int gms = wm * MS + ms, gns = wn * NS + ns;
      if (d.slices == 1) {
        const int n = n0 + 16 * gns + r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = m0 + 16 * gms + 4 * q + e;
          if (m < d.M && n < d.N) d.C[((int64_t)m * d.N + n) * taps + tap] = tot[ns][ms][e];
        }
      } else {
        float4v_t* dst = reinterpret_cast<float4v_t*>(d.part) +
                         ((((int64_t)tap * d.slices + slice) * d.tiles + tile) * SUB + gms * (TN / 16) + gns) * 64 + lane;
        *dst = tot[ns][ms];
      }
    }
}

// wgrad_reduce_kernel with the tap as blockIdx.y: dWc[m][n][tap] = sum over the slices in the same fixed order, fp64.
__global__ __launch_bounds__(256) void core_wgrad_reduce_kernel(const WgradArgs d, int TM, int TN, int taps) {
  const int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int j = threadIdx.x & 7, tap = blockIdx.y;
  const int64_t total = (int64_t)d.M * d.N;
  const bool valid = idx < total;
  const int64_t id = valid ? idx : total - 1;
  const int m = (int)(id / d.N), n = (int)(id - (int64_t)m * d.N);
  const int sub_n = TN / 16, SUB = (TM / 16) * sub_n;
  const int tile = (m / TM) * d.tiles_n + n / TN;
  const int ml = m % TM, nl = n % TN;
  const int64_t off = ((int64_t)tile * SUB + (ml / 16) * sub_n + nl / 16) * 256 + (((ml & 15) >> 2) * 16 + (nl & 15)) * 4 + (ml & 3);
  const int64_t stride = (int64_t)d.tiles * SUB * 256;
  const float* part = d.part + (int64_t)tap * d.slices * stride;
  double s = 0.0;
  for (int sl = j; sl < d.slices; sl += 8) s += (double)part[sl * stride + off];
  s += __shfl_xor(s, 4, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 1, 64);
  if (valid && j == 0) d.C[((int64_t)m * d.N + n) * taps + tap] = (float)s;
}

template <int P, int TM, int TN, typename TIn>
hipError_t core_wgrad_launch(const CoreWgradArgs& a, hipStream_t s, size_t* lds_out) {
  auto kern = core_wgrad_kernel<P, TM, TN, TIn>;
  constexpr size_t lds = wgrad_lds_bytes<P, TM, TN>();
  *lds_out = lds;
  if (lds > 64 * 1024) {
    static DynLdsOptIn allow_lds;
    const hipError_t e = allow_lds(kern, lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)a.g.tiles * a.g.slices, (unsigned)(a.kh * a.kw)), dim3(256), lds, s, a);
  return hipGetLastError();
}
template <int P, typename TIn, int TM>
hipError_t core_wgrad_launch_tn(const CoreWgradArgs& a, int TN, hipStream_t s, size_t* lds) {
  if (TN == 64) return core_wgrad_launch<P, TM, 64, TIn>(a, s, lds);
  if (TN == 32) return core_wgrad_launch<P, TM, 32, TIn>(a, s, lds);
  return core_wgrad_launch<P, TM, 16, TIn>(a, s, lds);
}
template <int P, typename TIn>
hipError_t core_wgrad_launch_tile(const CoreWgradArgs& a, int TM, int TN, hipStream_t s, size_t* lds) {
  if (TM == 64) return core_wgrad_launch_tn<P, TIn, 64>(a, TN, s, lds);
  if (TM == 32) return core_wgrad_launch_tn<P, TIn, 32>(a, TN, s, lds);
  return core_wgrad_launch_tn<P, TIn, 16>(a, TN, s, lds);
}

// Tiles as for tadmm_wgrad; slices count the taps among the workgroups: a pure function of the descriptor's shapes.
int core_wgrad_geom(tadmm_handle h, const tadmm_core_conv_desc* d, WgradGeom& g) {
  const int rc = core_conv_check(h, d, false, 0, 0);
  if (rc != TADMM_OK) return rc;
  const int64_t T = (int64_t)d->B * d->Ho * d->Wo, taps = (int64_t)d->kh * d->kw;
  if (T > INT32_MAX - 2 * kWgKC) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "core conv wgrad: %lld output pixels exceed the launch", (long long)T);
  if (taps > 65535) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "core conv wgrad: %lld taps exceed the launch", (long long)taps);
  g.TM = wgrad_tile(d->R2);
  g.TN = wgrad_tile(d->R1);
  g.tiles_m = (d->R2 + g.TM - 1) / g.TM;
  g.tiles_n = (d->R1 + g.TN - 1) / g.TN;
  const int64_t tiles = (int64_t)g.tiles_m * g.tiles_n;
  if (tiles > kWgMaxTiles) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "core conv wgrad: %lld output tiles exceed the launch", (long long)tiles);
  g.tiles = (int)tiles;
  g.nchunks = (int)((T + kWgKC - 1) / kWgKC);
  int64_t s = (kWgTargetWG + tiles * taps - 1) / (tiles * taps);
  s = std::min<int64_t>(s, T / kWgMinSlice);
  g.slices = (int)std::max<int64_t>(s, 1);
  g.ws_bytes = g.slices > 1 ? (size_t)taps * g.slices * g.tiles * g.TM * g.TN * sizeof(float) : 0;
  return TADMM_OK;
}

}  // namespace
}  // namespace tadmm

using namespace tadmm;

extern "C" {

int tadmm_wgrad_desc_bytes(void) { return (int)sizeof(tadmm_wgrad_desc); }

int tadmm_wgrad_workspace_bytes(const tadmm_wgrad_desc* d, size_t* bytes, int* slices_out) {
  if (!bytes) return TADMM_ERR_INVALID;
  WgradGeom g;
  const int rc = wgrad_geom(nullptr, d, g);
  if (rc != TADMM_OK) return rc;
  *bytes = g.ws_bytes;
  if (slices_out) *slices_out = g.slices;
  return TADMM_OK;
}

int tadmm_wgrad(tadmm_handle h, const tadmm_wgrad_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  WgradGeom g;
  const int rc = wgrad_geom(h, d, g);
  if (rc != TADMM_OK) return rc;
  if (!d->C || ((uintptr_t)d->C & 3) || d->ldc < d->N) CTX_FAIL(h, TADMM_ERR_INVALID, "wgrad: C is null, misaligned or ldc < N");
  if (g.ws_bytes && (!workspace || workspace_bytes < g.ws_bytes))
    CTX_FAIL(h, TADMM_ERR_WORKSPACE, "wgrad workspace too small: need %zu bytes, got %zu", g.ws_bytes, workspace_bytes);
  if (g.ws_bytes && ((uintptr_t)workspace & 15)) CTX_FAIL(h, TADMM_ERR_INVALID, "wgrad: workspace must be 16-byte aligned");
  const int esz = d->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  WgradArgs a;
  a.A = d->A; a.B = d->B; a.C = d->C; a.part = (float*)workspace;
  a.lda = d->lda; a.ldb = d->ldb; a.ldc = d->ldc;
  a.T = (int32_t)d->T; a.M = d->M; a.N = d->N; a.hw = d->hw;
  a.tiles_n = g.tiles_n; a.tiles = g.tiles; a.slices = g.slices; a.nchunks = g.nchunks;
  a.vec_a = wgrad_vec(d->A, d->hw > 0 ? d->hw : d->lda, esz);
  a.vec_b = wgrad_vec(d->B, d->hw > 0 ? d->hw : d->ldb, esz);
  a.alpha = d->alpha;
  const hipStream_t s = (hipStream_t)stream;
  const bool img = d->hw > 0;
  size_t lds = 0;
  hipError_t e;
  if (d->dtype == TADMM_CHAIN_F32) {
    e = img ? wgrad_launch_tile<3, float, true>(a, g.TM, g.TN, s, &lds) : wgrad_launch_tile<3, float, false>(a, g.TM, g.TN, s, &lds);
  } else {
    e = img ? wgrad_launch_tile<1, uint16_t, true>(a, g.TM, g.TN, s, &lds)
            : wgrad_launch_tile<1, uint16_t, false>(a, g.TM, g.TN, s, &lds);
  }
  if (e != hipSuccess)
    CTX_FAIL(h, TADMM_ERR_HIP, "wgrad: launch of the %d x %d tile kernel (%zu bytes of LDS) failed: %s", g.TM, g.TN, lds,
             hipGetErrorString(e));
  if (g.slices > 1) {
    const int64_t nb = ((int64_t)d->M * d->N * 8 + 255) / 256;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, s, a, g.TM, g.TN);
  }
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_core_conv_wgrad_workspace_bytes(const tadmm_core_conv_desc* d, size_t* bytes, int* slices_out) {
  if (!bytes) return TADMM_ERR_INVALID;
  WgradGeom g;
  const int rc = core_wgrad_geom(nullptr, d, g);
  if (rc != TADMM_OK) return rc;
  *bytes = g.ws_bytes;
  if (slices_out) *slices_out = g.slices;
  return TADMM_OK;
}

int tadmm_core_conv_wgrad(tadmm_handle h, const tadmm_core_conv_desc* d, float* dW, void* workspace, size_t workspace_bytes,
                          void* stream) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  WgradGeom g;
  const int rc = core_wgrad_geom(h, d, g);
  if (rc != TADMM_OK) return rc;
  if (!dW || ((uintptr_t)dW & 3)) CTX_FAIL(h, TADMM_ERR_INVALID, "core conv wgrad: dW is null or misaligned");
  if (g.ws_bytes && (!workspace || workspace_bytes < g.ws_bytes))
    CTX_FAIL(h, TADMM_ERR_WORKSPACE, "core conv wgrad workspace too small: need %zu bytes, got %zu", g.ws_bytes, workspace_bytes);
  if (g.ws_bytes && ((uintptr_t)workspace & 15)) CTX_FAIL(h, TADMM_ERR_INVALID, "core conv wgrad: workspace must be 16-byte aligned");
  const int esz = d->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  const int hwo = d->Ho * d->Wo;
  CoreWgradArgs a;
  memset(&a, 0, sizeof a);
  a.g.A = d->Y; a.g.B = d->X; a.g.C = dW; a.g.part = (float*)workspace;
  a.g.T = (int32_t)((int64_t)d->B * hwo); a.g.M = d->R2; a.g.N = d->R1; a.g.hw = hwo; a.g.ldc = d->R1;
  a.g.tiles_n = g.tiles_n; a.g.tiles = g.tiles; a.g.slices = g.slices; a.g.nchunks = g.nchunks;
  a.g.vec_a = wgrad_vec(d->Y, hwo, esz);
  a.g.alpha = 1.f;
  a.H = d->H; a.W = d->W; a.Ho = d->Ho; a.Wo = d->Wo; a.kh = d->kh; a.kw = d->kw; a.sh = d->stride_h; a.sw = d->stride_w;
  a.ph = d->pad_h; a.pw = d->pad_w; a.dh = d->dil_h; a.dw = d->dil_w;
  const hipStream_t s = (hipStream_t)stream;
  const int taps = d->kh * d->kw;
  if (a.g.T == 0) {                                      // B == 0: the sum over nothing
    HIP_OK(h, hipMemsetAsync(dW, 0, (size_t)d->R2 * d->R1 * taps * sizeof(float), s));
    return TADMM_OK;
  }
  size_t lds = 0;
  const hipError_t e = d->dtype == TADMM_CHAIN_F32 ? core_wgrad_launch_tile<3, float>(a, g.TM, g.TN, s, &lds)
                                                   : core_wgrad_launch_tile<1, uint16_t>(a, g.TM, g.TN, s, &lds);
  if (e != hipSuccess)
    CTX_FAIL(h, TADMM_ERR_HIP, "core conv wgrad: launch of the %d x %d tile kernel (%zu bytes of LDS) failed: %s", g.TM, g.TN,
             lds, hipGetErrorString(e));
  if (g.slices > 1) {
    const int64_t nb = ((int64_t)d->R2 * d->R1 * 8 + 255) / 256;
    hipLaunchKernelGGL(core_wgrad_reduce_kernel, dim3((unsigned)nb, (unsigned)taps), dim3(256), 0, s, a.g, g.TM, g.TN, taps);
  }
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
