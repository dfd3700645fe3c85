// Grouped strided GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact-f32 fma chain).
//
//   C(i,j) = alpha * sum_k A(i,k) * B(k,j)  [+ beta * C(i,j)] [+ bias_n[j]] [+ bias_m[i]]
//
// Every operand is addressed with (row stride, col stride) so one kernel serves all contractions of
// the path without materialised transposes: U_r^T * T (TT projection), T * (V Sigma^-1) (core of a
// tall unfolding), the tt2ten chain (ttd.py:39-40), and the forward chains of the factorised layers
// (TTLinear.py:79-86, TTConv.py:133-147, TKConv.py:210-214, TKLinear.py:66-71).
//
// Tile: 64x64 per workgroup, 4 waves in a 2x2 grid, each wave one 32x32 MFMA accumulator; K in LDS stages of 32.
// LDS images are k-major (As[k][m], Bs[k][n]) so the MFMA operand reads (lane = row/col index) are
// conflict-free ds_read_b32; the global->LDS path picks its lane mapping from whichever stride is 1
// so global loads stay coalesced for both "N" and "T" operands.  That choice and the edge handling are made once
// per tile (TileLoader); inside the k loop every global load is unconditional, through a global-address-space
// pointer, and issued two stages before the LDS store that consumes it (counted prefetch, see gemm_tile_sum).
#include "common.h"

namespace tadmm {

typedef float float16_t __attribute__((ext_vector_type(16)));

constexpr int BM = kGemmBM, BN = kGemmBN;
constexpr int BK = 32;                          // k values per LDS stage: half of a 64-wide accumulation chunk
constexpr int LDA = BM + 4, LDB = BN + 4;
constexpr int kStage = BK * (LDA + LDB);        // floats per LDS stage (A image then B image)
constexpr int NPF = 2;                          // register sets: a stage's global loads are issued NPF stages before its LDS store (even)

// How a thread fetches its 8 elements of a (64 rows x 32 k) operand stage.  Every load is unconditional -- the
// compiler can then count them (a branch per load makes it drain vmcnt to 0 at each LDS store) -- and every address
// lies inside the operand:
//   kKc  the operand is contiguous along k: thread = (row tid>>2, k 4*(tid&3) + 16 j), one 16-byte load per j.  The row
//        is clamped to nrows - 1, and the main loop only runs stages with k0 + 32 <= K.
//   kRc  contiguous along rows, tile fully inside (row0 + 64 <= nrows): thread = (k tid>>4 + 16 j, rows 4*(tid&15) ..+3),
//        one 16-byte load per j.
//   kRe  the same map for an edge tile: four 4-byte loads per j, each row clamped to nrows - 1.
// A clamped row repeats the operand's last row.  Row i of A (column j of B) feeds output row i (column j) only, and
// the epilogue stores no row >= M or column >= N, so what such rows hold is immaterial.  The K tail (K % 32 values)
// is loaded by load_tail(): loads with k clamped to K - 1 (4-byte ones except for kRc), and zero_tail() replaces the values at k >= K by +0: they
// feed real outputs, and zero products leave an accumulator as it is.
enum : int { kKc = 0, kRc = 1, kRe = 2 };

struct Frag8 { float v[2][4]; };

template <int MODE>
struct TileLoader {
  const G<const float>* base;   // operand
  int64_t rowoff[4];            // kKc: [0] = clamped row * rs; kRc / kRe: the (clamped) rows, unit stride
  int64_t cs;                   // element stride of k (1 for kKc)
  int kk;                       // this thread's k inside a group of 16

  __device__ __forceinline__ void init(const float* P, int64_t rs, int64_t cs_, int row0, int nrows, int tid) {
    base = gp(P);
    if (MODE == kKc) {
      kk = (tid & 3) * 4; cs = 1;
      rowoff[0] = (int64_t)min(row0 + (tid >> 2), nrows - 1) * rs;
      rowoff[1] = rowoff[2] = rowoff[3] = 0;
    } else {
      kk = tid >> 4; cs = cs_;
      const int rr = (tid & 15) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) rowoff[e] = min(row0 + rr + e, nrows - 1);
    }
  }
  // a full stage: k0 + BK <= K
  __device__ __forceinline__ void load(Frag8& f, int k0) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + 16 * j + kk;
      if (MODE == kRe) {
#pragma unroll
        for (int e = 0; e < 4; ++e) f.v[j][e] = base[(int64_t)k * cs + rowoff[e]];
      } else {
        const G<const float>* p = (MODE == kKc) ? base + rowoff[0] + k : base + (int64_t)k * cs + rowoff[0];
        const f4u t = *reinterpret_cast<const G<const f4u>*>(p);
        f.v[j][0] = t.x; f.v[j][1] = t.y; f.v[j][2] = t.z; f.v[j][3] = t.w;
      }
    }
  }
  // the last, partial stage: k0 < K < k0 + BK
  __device__ __forceinline__ void load_tail(Frag8& f, int k0, int K) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (MODE == kRc) {                 // whole rows: still one 16-byte load, at the clamped k
        const f4u t = *reinterpret_cast<const G<const f4u>*>(base + (int64_t)min(k0 + 16 * j + kk, K - 1) * cs + rowoff[0]);
        f.v[j][0] = t.x; f.v[j][1] = t.y; f.v[j][2] = t.z; f.v[j][3] = t.w;
        continue;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 16 * j + kk + (MODE == kKc ? e : 0);
        const int kc = min(k, K - 1);
        f.v[j][e] = (MODE == kKc) ? base[rowoff[0] + kc] : base[(int64_t)kc * cs + rowoff[e]];
      }
    }
  }
  // ... and its values beyond K replaced by +0.  Kept apart from the loads, where the tail is consumed: a select next to
  // its load is turned into a branch around the load, which is then waited for on the spot.
  __device__ __forceinline__ void zero_tail(Frag8& f, int k0, int K) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 16 * j + kk + (MODE == kKc ? e : 0);
        f.v[j][e] = (k < K) ? f.v[j][e] : 0.f;
      }
    }
  }
  // registers -> k-major LDS image S[k][row]
  __device__ __forceinline__ void store(float* __restrict__ S, int ldS, const Frag8& f, int tid) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (MODE == kKc) {
        const int rr = tid >> 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) S[(16 * j + kk + e) * ldS + rr] = f.v[j][e];
      } else {
        const int rr = (tid & 15) * 4;
        *reinterpret_cast<float4*>(&S[(16 * j + kk) * ldS + rr]) = make_float4(f.v[j][0], f.v[j][1], f.v[j][2], f.v[j][3]);
      }
    }
  }
};

// The sum over K of one 64x64 output tile, 16 values per lane (MFMA D layout).  kComp: chunked accumulation with a second
// fp32 total (the product default); false = one fp32 accumulator over all of K (TADMM_GEMM_PLAIN=1: A/B measurements only).
//
// Accumulation.  One fp32 MFMA accumulator over all of K rounds K times; when every product is equal (constant or
// rank-1 weights: all partial sums round the same way) the error grows like K eps instead of sqrt(K) eps and reached
// 1.3e-5 of ||W|| at K = 4608 -- above the 1e-5 parity bar.  The K range is therefore accumulated in chunks of 64
// (32 MFMAs, k ascending); a finished chunk is added to a second set of 16 registers on the vector ALU and the accumulator
// restarts from zero: the rounding bias of a chunk is at most 64 eps / 2 of ITS sum, that of the K / 64 additions of chunks
// the same again -- two orders of magnitude below the single-accumulator figure at K = 4608 (measured: <= 4e-7).
//
// Data movement.  A chunk is two LDS stages of 32 k; stage i + 1 is written while stage i feeds the MFMAs (one barrier
// per stage), from registers whose global loads were issued NPF stages earlier, so the loop waits with a partial vmcnt
// only.  The fold sits between two stages of the unrolled loop: the accumulator stays in place.
template <bool kComp, int AMODE, int BMODE>
__device__ __forceinline__ float16_t gemm_tile_sum(const GemmDesc& d, int m0, int n0, float* __restrict__ smem) {
  static_assert(NPF % 2 == 0, "the fold follows the odd stages of the unrolled loop");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int K = d.K;
  const int nfull = K / BK, rem = K - nfull * BK;
  TileLoader<AMODE> la;
  TileLoader<BMODE> lb;
  la.init(d.A, d.a_rs, d.a_cs, m0, d.M, tid);
  // For B the "rows" of the tile loader are the N index: element (n,k) at B + k*b_rs + n*b_cs
  lb.init(d.B, d.b_cs, d.b_rs, n0, d.N, tid);

  const float16_t zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  float16_t acc0 = zero16, tot = zero16;
  const int ai = wm * 32 + (lane & 31), bj = wn * 32 + (lane & 31), kq = lane >> 5;
  auto sstore = [&](const Frag8& fa, const Frag8& fb, int stage) {
    float* As = smem + stage * kStage;
    la.store(As, LDA, fa, tid);
    lb.store(As + BK * LDA, LDB, fb, tid);
  };
  auto compute = [&](int stage) {
    const float* As = smem + stage * kStage;
    const float* Bs = As + BK * LDA;
    // all operands of the stage first (one burst of LDS reads), then the MFMAs back to back, k ascending
    float a[BK / 2], b[BK / 2];
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
      a[s] = As[(2 * s + kq) * LDA + ai];
      b[s] = Bs[(2 * s + kq) * LDB + bj];
    }
    __builtin_amdgcn_sched_barrier(0);     // (left alone the scheduler reads two operands, waits, issues two MFMAs, and so on)
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc0, 0, 0, 0);
  };
  auto compute_half = [&](int stage, int h) {   // the 16 k of half h of a stage (the K tail: whole 16-wide steps only)
    const float* As = smem + stage * kStage + 16 * h * LDA;
    const float* Bs = smem + stage * kStage + BK * LDA + 16 * h * LDB;
    float a[BK / 4], b[BK / 4];
#pragma unroll
    for (int s = 0; s < BK / 4; ++s) {
      a[s] = As[(2 * s + kq) * LDA + ai];
      b[s] = Bs[(2 * s + kq) * LDB + bj];
    }
#pragma unroll
    for (int s = 0; s < BK / 4; ++s) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc0, 0, 0, 0);
  };
  auto fold = [&]() {
#pragma unroll
    for (int e = 0; e < 16; ++e) tot[e] += acc0[e];
    acc0 = zero16;
  };

  // the K tail is fetched first: its registers are consumed after the loop
  Frag8 ta, tb;
  if (rem) {
    la.load_tail(ta, nfull * BK, K);
    lb.load_tail(tb, nfull * BK, K);
  }
  Frag8 ra[NPF], rb[NPF];
  if (nfull > 0) {
    // Stage indices past the end are clamped to the last stage (a few repeated loads at the end of the loop) instead of
    // guarding the load: with the same number of loads in flight on every path the waits below stay counted.
    const int last = nfull - 1;
#pragma unroll
    for (int u = 0; u < NPF; ++u) { la.load(ra[u], min(u, last) * BK); lb.load(rb[u], min(u, last) * BK); }
    sstore(ra[0], rb[0], 0);
    la.load(ra[0], min(NPF, last) * BK);
    lb.load(rb[0], min(NPF, last) * BK);
    __syncthreads();
    int c = 0;
    for (; c + NPF <= nfull; c += NPF) {
#pragma unroll
      for (int u = 0; u < NPF; ++u) {
        const int i = c + u;             // stage i sits in LDS buffer u & 1; it closes a chunk of 64 when u is odd
        if (i + 1 < nfull) sstore(ra[(u + 1) % NPF], rb[(u + 1) % NPF], (u + 1) & 1);
        la.load(ra[(u + 1) % NPF], min(i + 1 + NPF, last) * BK);
        lb.load(rb[(u + 1) % NPF], min(i + 1 + NPF, last) * BK);
        __builtin_amdgcn_sched_barrier(0);   // the loads are issued before the MFMAs, not after them
        compute(u & 1);
        if (kComp && (u & 1)) fold();
        __syncthreads();
      }
    }
    if (c < nfull) {                     // nfull odd: the last full stage (even index, buffer 0) was stored by the step before
      compute(0);
      __syncthreads();
    }
  }
  if (rem) {
    // buffer nfull & 1 was last read by stage nfull - 2, two barriers ago.  Whole 16-wide steps run, as they always did: the
    // zeros beyond K add nothing.  The chunk is complete (and folded, as every chunk of four 16-wide steps is) when the
    // tail reaches into its last 16.
    la.zero_tail(ta, nfull * BK, K);
    lb.zero_tail(tb, nfull * BK, K);
    sstore(ta, tb, nfull & 1);
    __syncthreads();
    compute_half(nfull & 1, 0);
    if (rem > 16) compute_half(nfull & 1, 1);
    if (kComp && (nfull & 1) && rem > 16) fold();
  }
  float16_t acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = kComp ? tot[e] + acc0[e] : acc0[e];
  return acc;
}

// one 64x64 output tile (`local` = tile index inside the problem)
template <bool kComp>
__device__ __forceinline__ void gemm_tile(const GemmDesc& d, int local, float* __restrict__ smem) {
  const int tm = local / d.tiles_n, tn = local - tm * d.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const bool a_k = (d.a_cs == 1), b_k = (d.b_rs == 1) && (d.b_cs != 1);
  // one block-uniform decision per tile, outside the k loop
  const int am = a_k ? kKc : (m0 + BM <= d.M ? kRc : kRe);
  const int bm = b_k ? kKc : (n0 + BN <= d.N ? kRc : kRe);
  float16_t acc;
#define TADMM_GEMM_CASE(A_, B_) case A_ * 3 + B_: acc = gemm_tile_sum<kComp, A_, B_>(d, m0, n0, smem); break;
  switch (am * 3 + bm) {
    TADMM_GEMM_CASE(kKc, kKc) TADMM_GEMM_CASE(kKc, kRc) TADMM_GEMM_CASE(kKc, kRe)
    TADMM_GEMM_CASE(kRc, kKc) TADMM_GEMM_CASE(kRc, kRc) TADMM_GEMM_CASE(kRc, kRe)
    TADMM_GEMM_CASE(kRe, kKc) TADMM_GEMM_CASE(kRe, kRc)
    default: acc = gemm_tile_sum<kComp, kRe, kRe>(d, m0, n0, smem); break;
  }
#undef TADMM_GEMM_CASE

  // epilogue: D row = (reg&3) + 8*(reg>>2) + 4*(lane>>5), col = lane&31
  const int col = n0 + wn * 32 + (lane & 31);
  if (col < d.N) {
    const float bn = d.bias_n ? d.bias_n[col] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = m0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      if (row < d.M) {
        float* c = d.C + (int64_t)row * d.c_rs + (int64_t)col * d.c_cs;
        float v = d.alpha * acc[reg] + bn;
        if (d.bias_m) v += d.bias_m[row];
        if (d.beta != 0.f) v += d.beta * (*c);
        *c = v;
      }
    }
  }
}

template <bool kComp>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmDesc* __restrict__ descs,
                                                   const BlockRef* __restrict__ map,
                                                   const int32_t* __restrict__ skip) {
  __shared__ __attribute__((aligned(16))) float smem[2 * kStage];   // two stages in ONE array
  const BlockRef br = map[blockIdx.x];
  if (skip && skip[br.prob]) return;
  const GemmDesc d = descs[br.prob];
  gemm_tile<kComp>(d, br.local, smem);
}

// A single GEMM whose descriptor travels as a kernel argument: no descriptor upload, no block map
// (the per-call path of the factorised layers' forward / backward products).
template <bool kComp>
__global__ __launch_bounds__(256) void gemm_one_kernel(const GemmDesc d) {
  __shared__ __attribute__((aligned(16))) float smem[2 * kStage];   // two stages in ONE array
  gemm_tile<kComp>(d, blockIdx.x, smem);
}

static bool gemm_plain() {
  static const bool plain = getenv("TADMM_GEMM_PLAIN") && atoi(getenv("TADMM_GEMM_PLAIN"));   // read once per process
  return plain;
}

void launch_gemm_one(const GemmDesc& d, hipStream_t s) {
  const int nblocks = d.tiles_m * d.tiles_n;
  if (nblocks <= 0) return;
  if (gemm_plain()) hipLaunchKernelGGL(gemm_one_kernel<false>, dim3(nblocks), dim3(256), 0, s, d);
  else hipLaunchKernelGGL(gemm_one_kernel<true>, dim3(nblocks), dim3(256), 0, s, d);
}

void launch_gemm(const GemmDesc* descs_dev, const BlockRef* map_dev, int nblocks, hipStream_t s, const int32_t* skip) {
  if (nblocks <= 0) return;
  if (gemm_plain()) hipLaunchKernelGGL(gemm_kernel<false>, dim3(nblocks), dim3(256), 0, s, descs_dev, map_dev, skip);
  else hipLaunchKernelGGL(gemm_kernel<true>, dim3(nblocks), dim3(256), 0, s, descs_dev, map_dev, skip);
}

}  // namespace tadmm
