// Self-attention of a BERT encoder layer (the reference's xcompression/transformer/compressed_modeling*.py:
// *BertSelfAttention.forward after the three projections): for q, k, v of shape (B, S, H*d), read in place by heads,
//     scores[b,h,i,j] = (Q[b,i,h,:] . K[b,j,h,:]) / sqrt(d) + mask[b,j]
//     P = softmax_j(scores),  Pd = P * keep / (1 - p)
//     context[b,i,h*d:(h+1)*d] = sum_j Pd[b,h,i,j] V[b,j,h,:]
// in ONE launch (scores and the row statistics optional), and its backward in two launches, for gradients of BOTH outputs:
//     dPd = (g_ctx V^T) keep / (1-p),  D_i = sum_j P_ij dPd_ij,  dS = g_sc + P (dPd - D)
//     dQ = dS K / sqrt(d),  dK = dS^T Q / sqrt(d),  dV = Pd^T g_ctx
// with P recomputed from Q, K, the mask and the saved row statistics (m_i = row maximum, l_i = sum_j exp(s_ij - m_i), so
// lse_i = m_i + log l_i) as exp(s - m) / l: the forward's own expression.  One rounded lse would put its half ulp (2.4e-7
// at lse in [4, 8)) on every probability of the row alike, more than float32 parity with the composed route allows.
//
// Layout.  A workgroup of four waves owns 64 rows of one (b, h); a wave owns 16 of them and keeps their operand
// fragments in registers for the whole launch.  The other side streams through LDS in tiles of TS rows, zero padded past
// S and d, once as it lies in memory ([row][feature], the B operand of own . stream^T) and, where it is the B operand of a
// product that reduces over the streamed rows, once transposed ([feature][row]).  Every product is of the form
// C[m][n] = sum_k A[m][k] B[n][k] with both operands contiguous in k, so one fragment rule serves them all: lane l reads
// 16 bytes at row (l & 15), k = chunk + (16 bytes) * (l >> 4).  For float32 these are four k values that feed four
// v_mfma_f32_16x16x4_f32 (exact float32 products; the k order inside a chunk is the same for A and B, which is all a
// dot product needs); for bfloat16 / binary16 they are the eight values of one v_mfma_f32_16x16x32_{bf16,f16}.
// Accumulators are float32 in the C layout row = 4 (l >> 4) + reg, col = l & 15.
//   attn_fwd_kernel   own = 64 queries, stream = keys, two sweeps.  Sweep 0: the scores of a tile, each lane's running
//                     maximum and (double) sum, then one butterfly over the 16 lanes that share a row: the row
//                     statistics.  Sweep 1: the scores again (stored from the accumulators if asked for),
//                     P = exp(s - max) / sum, the keep mask, P in the input type through a per-wave LDS image into the
//                     A operand of Pd V.  The score product is done twice and no score lives across tiles: the context
//                     accumulator is never rescaled, and no register array grows with S.
//   attn_bwd_kernel   <KV = false> own = 64 queries, stream = keys: sweep 0 forms D (stored for the other pass), sweep 1
//                     dS and dQ += dS K.  <KV = true> own = 64 keys, stream = queries: dS^T and Pd^T, dK += dS^T Q,
//                     dV += Pd^T g_ctx.  A block owns its output rows: no atomics, bitwise reproducible.
// The softmax and the backward's elementwise part run in double around a float32 expf (see attn_exp); a masked-out
// column (mask -inf, or past S) contributes an exact zero.
#include "host.h"

#include <type_traits>

namespace tadmm {

typedef float attn_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t attn_u4 __attribute__((ext_vector_type(4)));
typedef __bf16 attn_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 attn_f16x8 __attribute__((ext_vector_type(8)));

struct attn_bf16 { uint16_t x; };
struct attn_f16 { _Float16 x; };

__device__ __forceinline__ float attn_widen(float v) { return v; }
__device__ __forceinline__ float attn_widen(attn_bf16 v) { return __uint_as_float((uint32_t)v.x << 16); }
__device__ __forceinline__ float attn_widen(attn_f16 v) { return (float)v.x; }

template <typename T> __device__ __forceinline__ T attn_narrow(float v);
template <> __device__ __forceinline__ float attn_narrow<float>(float v) { return v; }
template <> __device__ __forceinline__ attn_bf16 attn_narrow<attn_bf16>(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return attn_bf16{(uint16_t)((u >> 16) | 0x40)};     // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                                          // nearest even
  return attn_bf16{(uint16_t)(u >> 16)};
}
template <> __device__ __forceinline__ attn_f16 attn_narrow<attn_f16>(float v) { return attn_f16{(_Float16)v}; }

// KC: k values per 16-byte fragment step over the four lane groups; FE: elements in a lane's 16 bytes; PAD: elements
// that keep LDS rows 16 bytes apart from a multiple of 128 bytes.
template <typename T> struct AttnT { static constexpr int KC = 32, FE = 8, PAD = 8; };
template <> struct AttnT<float> { static constexpr int KC = 16, FE = 4, PAD = 4; };

template <typename T>
__device__ __forceinline__ attn_f4 attn_mma(attn_u4 a, attn_u4 b, attn_f4 c) {
  if constexpr (std::is_same<T, float>::value) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[e]), __uint_as_float(b[e]), c, 0, 0, 0);
    return c;
  } else if constexpr (std::is_same<T, attn_bf16>::value) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(attn_bf16x8, a), __builtin_bit_cast(attn_bf16x8, b), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(attn_f16x8, a), __builtin_bit_cast(attn_f16x8, b), c, 0, 0, 0);
  }
}

// The elementwise arithmetic between two matrix products is double: x / sqrt(d) + mask is exact there (the stored score is
// its one rounding), a probability is expf of the exponent's float32 head times (1 + its tail) -- the softmax turns an
// absolute error of a score, or of score - maximum, into a relative error of the probability -- and dS keeps double until
// it is rounded for the next product.  What is left is expf's own error, the rounded row sum and the products'
// float32 accumulation.  A few dozen double operations per score against S*d/8 bytes of traffic: they do not show.
__device__ __forceinline__ double attn_score(float x, double scale, float mask) {
  return (double)x * scale + (double)mask;
}
// exp(diff) for diff <= ~0; 0 for -inf (and for the NaN of -inf - -inf)
__device__ __forceinline__ double attn_exp(double diff) {
  if (!(diff > -INFINITY)) return 0.0;
  const float hi = (float)diff;
  return (double)expf(hi) * (1.0 + (diff - (double)hi));
}

struct AttnArgs {
  const void* q; const void* k; const void* v;
  int64_t q_ld, k_ld, v_ld, q_bs, k_bs, v_bs;
  const float* mask;            // (B, S) or null
  const uint8_t* keep;          // (B, H, S, S) or null
  void* ctx; void* scores; float* stats;   // stats: (B, H, S, 2) = row maximum, row sum
  const void* g_ctx; const void* g_sc;
  void* dq; void* dk; void* dv;
  double* D;                    // (B, H, S)
  double scale;                 // 1 / sqrt(d)
  double keep_scale;            // 1 / (1 - p)
  int32_t H, S, d;
};

// A lane's fragments of one own row, straight from global memory: element by element (any element alignment), zeros
// past d and for a row past S (row == nullptr).
template <typename T, int NCH>
__device__ __forceinline__ void attn_own_frags(const T* __restrict__ row, int d, int lg, attn_u4 (&f)[NCH]) {
  using X = AttnT<T>;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    struct alignas(16) { T v[X::FE]; } t;
#pragma unroll
    for (int e = 0; e < X::FE; ++e) {
      const int kk = c * X::KC + X::FE * lg + e;
      t.v[e] = (row && kk < d) ? row[kk] : attn_narrow<T>(0.f);
    }
    f[c] = __builtin_bit_cast(attn_u4, t);
  }
}

// Rows row0 .. row0 + TS - 1 of one head (src = its row 0, ld = row stride) into LDS, zero padded to TS x DP:
// nat[r][c] (row stride DP + PAD) and / or tr[c][r] (row stride TS + PAD).  The whole workgroup calls it.
template <typename T, int TS, int DP>
__device__ __forceinline__ void attn_stage(const T* __restrict__ src, int64_t ld, int row0, int S, int d,
                                           T* __restrict__ nat, T* __restrict__ tr) {
  constexpr int LDN = DP + AttnT<T>::PAD, LDT = TS + AttnT<T>::PAD;
#pragma unroll 4
  for (int idx = threadIdx.x; idx < TS * DP; idx += 256) {
    const int r = idx / DP, c = idx % DP;
    T v = attn_narrow<T>(0.f);
    if (row0 + r < S && c < d) v = src[(int64_t)(row0 + r) * ld + c];
    if (nat) nat[r * LDN + c] = v;
    if (tr) tr[c * LDT + r] = v;
  }
}

// own (16 x DP, register fragments) . tile rows^T (16 rows of a [row][feature] LDS image): one 16 x 16 block.
template <typename T, int NCH, int LD>
__device__ __forceinline__ attn_f4 attn_nt(const attn_u4 (&a)[NCH], const T* __restrict__ rows, int lane) {
  using X = AttnT<T>;
  attn_f4 acc = {0.f, 0.f, 0.f, 0.f};
  const T* p = rows + (lane & 15) * LD + X::FE * (lane >> 4);
#pragma unroll
  for (int c = 0; c < NCH; ++c) acc = attn_mma<T>(a[c], *reinterpret_cast<const attn_u4*>(p + c * X::KC), acc);
  return acc;
}

// acc (16 x DP) += st (16 x TS, the wave's LDS image) . bt^T (bt: [feature][row] image, DP x TS)
template <typename T, int TS, int DP>
__device__ __forceinline__ void attn_acc(attn_f4 (&acc)[DP / 16], const T* __restrict__ st, const T* __restrict__ bt, int lane) {
  using X = AttnT<T>;
  constexpr int LDT = TS + X::PAD;
  const int off = (lane & 15) * LDT + X::FE * (lane >> 4);
#pragma unroll
  for (int c = 0; c < TS / X::KC; ++c) {
    const attn_u4 af = *reinterpret_cast<const attn_u4*>(st + off + c * X::KC);
#pragma unroll
    for (int n = 0; n < DP / 16; ++n)
      acc[n] = attn_mma<T>(af, *reinterpret_cast<const attn_u4*>(bt + n * 16 * LDT + off + c * X::KC), acc[n]);
  }
}

// the wave's 16 x DP accumulators, times mul, into rows row0.. of a contiguous (B, S, H*d) tensor (out = row 0, head h)
template <typename T, int DP>
__device__ __forceinline__ void attn_store_rows(T* __restrict__ out, int64_t ld, const attn_f4 (&acc)[DP / 16], double mul,
                                                int row0, int S, int d, int lane) {
#pragma unroll
  for (int n = 0; n < DP / 16; ++n) {
    const int c = n * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * (lane >> 4) + r;
      if (row < S && c < d) out[(int64_t)row * ld + c] = attn_narrow<T>((float)((double)acc[n][r] * mul));
    }
  }
}

constexpr int kAttnFwdTile = 64, kAttnBwdTile = 32;

template <typename T, int DP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const AttnArgs a) {
  using X = AttnT<T>;
  constexpr int TS = kAttnFwdTile, NCH = DP / X::KC, LDN = DP + X::PAD, LDT = TS + X::PAD, ND = DP / 16;
  __shared__ __attribute__((aligned(16))) T sK[TS * LDN];
  __shared__ __attribute__((aligned(16))) T sVt[DP * LDT];
  __shared__ __attribute__((aligned(16))) T sP[4 * 16 * LDT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
  const int S = a.S, d = a.d, H = a.H;
  const int nqb = (S + 63) / 64;
  const int qb = (int)(blockIdx.x % nqb);
  const int64_t bh = blockIdx.x / nqb;
  const int h = (int)(bh % H);
  const int64_t b = bh / H;
  const T* __restrict__ Q = (const T*)a.q + b * a.q_bs + (int64_t)h * d;
  const T* __restrict__ K = (const T*)a.k + b * a.k_bs + (int64_t)h * d;
  const T* __restrict__ V = (const T*)a.v + b * a.v_bs + (int64_t)h * d;
  const float* __restrict__ mask = a.mask ? a.mask + b * S : nullptr;
  const int row0 = qb * 64 + wave * 16;
  const double scale = a.scale;

  attn_u4 aq[NCH];
  attn_own_frags<T, NCH>(row0 + lr < S ? Q + (int64_t)(row0 + lr) * a.q_ld : nullptr, d, lg, aq);

  const int nt = (S + TS - 1) / TS;
  float m[4];
  double l[4];                                        // the row sum in double: rescaled whenever the maximum moves
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.0; }
  for (int t = 0; t < nt; ++t) {
    __syncthreads();
    attn_stage<T, TS, DP>(K, a.k_ld, t * TS, S, d, sK, nullptr);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < TS / 16; ++n) {
      const int col = t * TS + n * 16 + lr;
      const attn_f4 x = attn_nt<T, NCH, LDN>(aq, sK + n * 16 * LDN, lane);
      const float mk = col < S ? (mask ? mask[col] : 0.f) : -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double sd = col < S ? attn_score(x[r], scale, mk) : -(double)INFINITY;
        const float s = (float)sd;
        if (s > m[r]) { l[r] = l[r] * attn_exp((double)m[r] - (double)s) + attn_exp(sd - (double)s); m[r] = s; }
        else l[r] += attn_exp(sd - (double)m[r]);
      }
    }
  }
  float lf[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const float om = __shfl_xor(m[r], off, 64);
      const double ol = __shfl_xor(l[r], off, 64);
      const float M = fmaxf(m[r], om);
      l[r] = l[r] * attn_exp((double)m[r] - (double)M) + ol * attn_exp((double)om - (double)M);
      m[r] = M;
    }
    lf[r] = (float)l[r];
    const int row = row0 + 4 * lg + r;
    if (a.stats && lr == 0 && row < S) { a.stats[2 * (bh * S + row)] = m[r]; a.stats[2 * (bh * S + row) + 1] = lf[r]; }
  }

  attn_f4 acc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) acc[n] = attn_f4{0.f, 0.f, 0.f, 0.f};
  T* __restrict__ myP = sP + wave * 16 * LDT;
  T* __restrict__ sc = (T*)a.scores;
  const uint8_t* __restrict__ keep = a.keep;
  for (int t = 0; t < nt; ++t) {
    __syncthreads();
    attn_stage<T, TS, DP>(K, a.k_ld, t * TS, S, d, sK, nullptr);
    attn_stage<T, TS, DP>(V, a.v_ld, t * TS, S, d, nullptr, sVt);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < TS / 16; ++n) {
      const int col = t * TS + n * 16 + lr;
      const attn_f4 x = attn_nt<T, NCH, LDN>(aq, sK + n * 16 * LDN, lane);
      const float mk = col < S ? (mask ? mask[col] : 0.f) : -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * lg + r;
        const bool in = row < S && col < S;
        const double sd = col < S ? attn_score(x[r], scale, mk) : -(double)INFINITY;
        double p = attn_exp(sd - (double)m[r]) / (double)lf[r];
        if (in) {
          const int64_t e = (bh * S + row) * S + col;
          if (sc) sc[e] = attn_narrow<T>((float)sd);
          if (keep) p = keep[e] ? p * a.keep_scale : 0.0;
        }
        myP[(4 * lg + r) * LDT + n * 16 + lr] = attn_narrow<T>((float)p);
      }
    }
    __syncthreads();
    attn_acc<T, TS, DP>(acc, myP, sVt, lane);
  }
  const int64_t ldo = (int64_t)H * d;
  attn_store_rows<T, DP>((T*)a.ctx + b * S * ldo + (int64_t)h * d, ldo, acc, 1.0, row0, S, d, lane);
}

template <typename T, int DP, bool KV>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const AttnArgs a) {
  using X = AttnT<T>;
  constexpr int TS = kAttnBwdTile, NCH = DP / X::KC, LDN = DP + X::PAD, LDT = TS + X::PAD, ND = DP / 16;
  __shared__ __attribute__((aligned(16))) T sB1n[TS * LDN];
  __shared__ __attribute__((aligned(16))) T sB1t[DP * LDT];
  __shared__ __attribute__((aligned(16))) T sB2n[TS * LDN];
  __shared__ __attribute__((aligned(16))) T sB2t[KV ? DP * LDT : 8];
  __shared__ __attribute__((aligned(16))) T sS1[4 * 16 * LDT];
  __shared__ __attribute__((aligned(16))) T sS2[KV ? 4 * 16 * LDT : 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
  const int S = a.S, d = a.d, H = a.H;
  const int nob = (S + 63) / 64;
  const int ob = (int)(blockIdx.x % nob);
  const int64_t bh = blockIdx.x / nob;
  const int h = (int)(bh % H);
  const int64_t b = bh / H;
  const int64_t ldo = (int64_t)H * d;
  const T* __restrict__ Q = (const T*)a.q + b * a.q_bs + (int64_t)h * d;
  const T* __restrict__ K = (const T*)a.k + b * a.k_bs + (int64_t)h * d;
  const T* __restrict__ V = (const T*)a.v + b * a.v_bs + (int64_t)h * d;
  const T* __restrict__ G = a.g_ctx ? (const T*)a.g_ctx + b * S * ldo + (int64_t)h * d : nullptr;
  const T* __restrict__ gsc = (const T*)a.g_sc;
  const float* __restrict__ mask = a.mask ? a.mask + b * S : nullptr;
  const float* __restrict__ stats = a.stats + 2 * bh * S;
  double* __restrict__ Dv = a.D ? a.D + bh * S : nullptr;
  const uint8_t* __restrict__ keep = a.keep;
  const bool has_gc = G != nullptr;
  const double scale = a.scale;
  const double ks_on = a.keep_scale;
  const int row0 = ob * 64 + wave * 16;

  // own side: A1 (Q or K) and A2 (g_ctx or V); streamed side: B1 (K or Q) and B2 (V or g_ctx)
  const T* __restrict__ A1 = KV ? K : Q;  const int64_t lda1 = KV ? a.k_ld : a.q_ld;
  const T* __restrict__ A2 = KV ? V : G;  const int64_t lda2 = KV ? a.v_ld : ldo;
  const T* __restrict__ B1 = KV ? Q : K;  const int64_t ldb1 = KV ? a.q_ld : a.k_ld;
  const T* __restrict__ B2 = KV ? G : V;  const int64_t ldb2 = KV ? ldo : a.v_ld;
  attn_u4 a1[NCH], a2[NCH];
  attn_own_frags<T, NCH>(row0 + lr < S ? A1 + (int64_t)(row0 + lr) * lda1 : nullptr, d, lg, a1);
  attn_own_frags<T, NCH>(has_gc && row0 + lr < S ? A2 + (int64_t)(row0 + lr) * lda2 : nullptr, d, lg, a2);

  // per own row (registers): KV: the key's mask; else: the query's row maximum, row sum and D
  float own_mask[4], own_m[4], own_l[4];
  double own_D[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * lg + r;
    own_mask[r] = (KV && mask && row < S) ? mask[row] : 0.f;
    own_m[r] = (!KV && row < S) ? stats[2 * row] : 0.f;
    own_l[r] = (!KV && row < S) ? stats[2 * row + 1] : 1.f;
    own_D[r] = 0.0;
  }
  const int nt = (S + TS - 1) / TS;

  // p and the keep factor of element (own row r, streamed column col) from the score accumulator x
  auto prob = [&](float x, int r, int col, float col_mask, float col_m, float col_l, double& ksf) -> double {
    const int row = row0 + 4 * lg + r;
    ksf = 1.0;
    if (row >= S || col >= S) { ksf = 0.0; return 0.0; }
    const int i = KV ? col : row, j = KV ? row : col;
    if (keep) ksf = keep[(bh * S + i) * S + j] ? ks_on : 0.0;
    const double sd = attn_score(x, scale, KV ? own_mask[r] : col_mask);
    return attn_exp(sd - (double)(KV ? col_m : own_m[r])) / (double)(KV ? col_l : own_l[r]);
  };

  if (!KV && has_gc) {                                   // sweep 0: D_i = sum_j P_ij dPd_ij
    for (int t = 0; t < nt; ++t) {
      __syncthreads();
      attn_stage<T, TS, DP>(B1, ldb1, t * TS, S, d, sB1n, nullptr);
      attn_stage<T, TS, DP>(B2, ldb2, t * TS, S, d, sB2n, nullptr);
      __syncthreads();
#pragma unroll
      for (int n = 0; n < TS / 16; ++n) {
        const int col = t * TS + n * 16 + lr;
        const attn_f4 x = attn_nt<T, NCH, LDN>(a1, sB1n + n * 16 * LDN, lane);
        const attn_f4 y = attn_nt<T, NCH, LDN>(a2, sB2n + n * 16 * LDN, lane);
        const float cm = (mask && col < S) ? mask[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double ksf;
          const double p = prob(x[r], r, col, cm, 0.f, 1.f, ksf);
          own_D[r] += p * ((double)y[r] * ksf);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) own_D[r] += __shfl_xor(own_D[r], off, 64);
      const int row = row0 + 4 * lg + r;
      if (Dv && lr == 0 && row < S) Dv[row] = own_D[r];
    }
  }

  attn_f4 acc1[ND], acc2[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) { acc1[n] = attn_f4{0.f, 0.f, 0.f, 0.f}; acc2[n] = attn_f4{0.f, 0.f, 0.f, 0.f}; }
  T* __restrict__ my1 = sS1 + wave * 16 * LDT;
  T* __restrict__ my2 = sS2 + (KV ? wave * 16 * LDT : 0);
  for (int t = 0; t < nt; ++t) {
    __syncthreads();
    attn_stage<T, TS, DP>(B1, ldb1, t * TS, S, d, has_gc ? sB1n : nullptr, sB1t);
    if (has_gc) attn_stage<T, TS, DP>(B2, ldb2, t * TS, S, d, sB2n, KV ? sB2t : nullptr);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < TS / 16; ++n) {
      const int col = t * TS + n * 16 + lr;
      attn_f4 x = {0.f, 0.f, 0.f, 0.f}, y = {0.f, 0.f, 0.f, 0.f};
      float cm = 0.f, cx = 0.f, cl = 1.f;
      double cD = 0.0;
      if (has_gc) {
        x = attn_nt<T, NCH, LDN>(a1, sB1n + n * 16 * LDN, lane);
        y = attn_nt<T, NCH, LDN>(a2, sB2n + n * 16 * LDN, lane);
        if (col < S) {
          if (KV) { cx = stats[2 * col]; cl = stats[2 * col + 1]; cD = Dv[col]; }
          else if (mask) cm = mask[col];
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * lg + r;
        double ds = 0.0, pd = 0.0;
        if (row < S && col < S) {
          const int i = KV ? col : row, j = KV ? row : col;
          if (gsc) ds = (double)attn_widen(gsc[(bh * S + i) * S + j]);
          if (has_gc) {
            double ksf;
            const double p = prob(x[r], r, col, cm, cx, cl, ksf);
            ds += p * ((double)y[r] * ksf - (KV ? cD : own_D[r]));
            pd = p * ksf;
          }
        }
        my1[(4 * lg + r) * LDT + n * 16 + lr] = attn_narrow<T>((float)ds);
        if (KV) my2[(4 * lg + r) * LDT + n * 16 + lr] = attn_narrow<T>((float)pd);
      }
    }
    __syncthreads();
    attn_acc<T, TS, DP>(acc1, my1, sB1t, lane);
    if (KV && has_gc) attn_acc<T, TS, DP>(acc2, my2, sB2t, lane);
  }
  if (KV) {
    attn_store_rows<T, DP>((T*)a.dk + b * S * ldo + (int64_t)h * d, ldo, acc1, scale, row0, S, d, lane);
    attn_store_rows<T, DP>((T*)a.dv + b * S * ldo + (int64_t)h * d, ldo, acc2, 1.0, row0, S, d, lane);
  } else {
    attn_store_rows<T, DP>((T*)a.dq + b * S * ldo + (int64_t)h * d, ldo, acc1, scale, row0, S, d, lane);
  }
}

}  // namespace tadmm

using namespace tadmm;

namespace {

constexpr int kAttnMaxS = 512, kAttnMaxD = 64;

size_t attn_ws_bytes(int64_t B, int64_t H, int64_t S) { return align_up((size_t)(B * H * S) * sizeof(double), 256); }

// static LDS of the larger launch (the key-owning backward pass) for an element of es bytes and head width d
size_t attn_lds_bytes(size_t es, int d) {
  const size_t DP = d <= 32 ? 32 : 64, PAD = 16 / es, TSb = kAttnBwdTile, TSf = kAttnFwdTile;
  const size_t bwd = (2 * TSb * (DP + PAD) + 2 * DP * (TSb + PAD) + 2 * 64 * (TSb + PAD)) * es;
  const size_t fwd = (TSf * (DP + PAD) + DP * (TSf + PAD) + 64 * (TSf + PAD)) * es;
  return bwd > fwd ? bwd : fwd;
}

template <typename T>
void attn_launch_fwd(const AttnArgs& a, unsigned grid, hipStream_t s) {
  if (a.d <= 32) hipLaunchKernelGGL((attn_fwd_kernel<T, 32>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((attn_fwd_kernel<T, 64>), dim3(grid), dim3(256), 0, s, a);
}

template <typename T>
void attn_launch_bwd(const AttnArgs& a, unsigned grid, hipStream_t s) {
  if (a.d <= 32) {
    hipLaunchKernelGGL((attn_bwd_kernel<T, 32, false>), dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL((attn_bwd_kernel<T, 32, true>), dim3(grid), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((attn_bwd_kernel<T, 64, false>), dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL((attn_bwd_kernel<T, 64, true>), dim3(grid), dim3(256), 0, s, a);
  }
}

// The checks the two launches share.  Returns TADMM_OK with *skip set for an empty batch.
int attn_check(tadmm_handle h, const tadmm_attn_desc* d, const char* who, bool bwd, AttnArgs* a, unsigned* grid, bool* skip) {
  *skip = false;
  if (!d) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: the descriptor is NULL", who);
  if (d->S < 1 || d->d < 1 || d->H < 1 || d->B < 0)
    CTX_FAIL(h, TADMM_ERR_INVALID, "%s: S >= 1, d >= 1, H >= 1 and B >= 0 are required (got B %lld, H %d, S %d, d %d)", who,
             (long long)d->B, d->H, d->S, d->d);
  if (d->dtype != TADMM_CHAIN_F32 && d->dtype != TADMM_CHAIN_BF16 && d->dtype != TADMM_CHAIN_F16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "%s: unknown element type %d", who, d->dtype);
  if (bwd && d->dtype == TADMM_CHAIN_F16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "%s: binary16 is forward only (there is no binary16 training)", who);
  if (d->S > kAttnMaxS || d->d > kAttnMaxD)
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "%s: S %d > %d or d %d > %d: not a shape the launch takes", who, d->S, kAttnMaxS, d->d, kAttnMaxD);
  const size_t es = d->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  const int64_t Hd = (int64_t)d->H * d->d;
  struct { const char* name; const void* p; int64_t ld, bs; } in[3] = {
      {"q", d->q, d->q_ld, d->q_bs}, {"k", d->k, d->k_ld, d->k_bs}, {"v", d->v, d->v_ld, d->v_bs}};
  for (const auto& r : in) {
    if (!r.p) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: %s is NULL", who, r.name);
    if (((uintptr_t)r.p) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: %s is not aligned to its element", who, r.name);
    if (r.ld < Hd) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: row stride of %s %lld < H*d %lld", who, r.name, (long long)r.ld, (long long)Hd);
    if (r.bs < 0) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: batch stride of %s %lld < 0", who, r.name, (long long)r.bs);
  }
  if (((uintptr_t)d->mask) % 4) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: mask is not aligned to its element", who);
  if (!(d->p >= 0.0 && d->p < 1.0)) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: dropout p %g outside [0, 1)", who, d->p);
  if (d->p > 0.0 && !d->keep) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: dropout p %g > 0 without a keep tensor", who, d->p);
  if (!bwd) {
    if (!d->ctx || ((uintptr_t)d->ctx) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: ctx is NULL or misaligned", who);
    if (((uintptr_t)d->scores) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: scores is not aligned to its element", who);
    if (((uintptr_t)d->stats) % 4) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: stats is not aligned to its element", who);
  } else {
    if (!d->stats || ((uintptr_t)d->stats) % 4) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: stats is NULL or misaligned", who);
    if (((uintptr_t)d->g_ctx) % es || ((uintptr_t)d->g_sc) % es)
      CTX_FAIL(h, TADMM_ERR_INVALID, "%s: an upstream gradient is not aligned to its element", who);
    const void* outs[3] = {d->dq, d->dk, d->dv};
    for (const void* o : outs)
      if (!o || ((uintptr_t)o) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: dq / dk / dv are NULL or misaligned", who);
    if (d->g_ctx) {
      const size_t need = attn_ws_bytes(d->B, d->H, d->S);
      if (!d->workspace || ((uintptr_t)d->workspace) % 8 || d->workspace_bytes < need)
        CTX_FAIL(h, TADMM_ERR_WORKSPACE, "%s workspace too small or misaligned: need %zu bytes, got %zu", who, need, d->workspace_bytes);
    }
  }
  const int64_t blocks = d->B * d->H * (int64_t)((d->S + 63) / 64);
  if (blocks >= ((int64_t)1 << 31)) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "%s: %lld workgroups", who, (long long)blocks);
  if (d->B == 0) { *skip = true; return TADMM_OK; }
  *grid = (unsigned)blocks;
  a->q = d->q; a->k = d->k; a->v = d->v;
  a->q_ld = d->q_ld; a->k_ld = d->k_ld; a->v_ld = d->v_ld;
  a->q_bs = d->q_bs; a->k_bs = d->k_bs; a->v_bs = d->v_bs;
  a->mask = d->mask;
  a->keep = d->p > 0.0 ? d->keep : nullptr;
  a->ctx = d->ctx; a->scores = d->scores; a->stats = d->stats;
  a->g_ctx = d->g_ctx; a->g_sc = d->g_sc;
  a->dq = d->dq; a->dk = d->dk; a->dv = d->dv;
  a->D = (double*)d->workspace;
  a->scale = 1.0 / sqrt((double)d->d);
  a->keep_scale = 1.0 / (1.0 - d->p);
  a->H = d->H; a->S = d->S; a->d = d->d;
  return TADMM_OK;
}

}  // namespace

extern "C" {

int tadmm_attn_desc_bytes(void) { return (int)sizeof(tadmm_attn_desc); }

int tadmm_attn_fits(const tadmm_attn_desc* d, size_t* lds_bytes) {
  if (lds_bytes) *lds_bytes = 0;
  if (!d || d->S < 1 || d->d < 1 || d->H < 1) return TADMM_ERR_INVALID;
  if (d->S > kAttnMaxS || d->d > kAttnMaxD) return 0;
  if (lds_bytes) *lds_bytes = attn_lds_bytes(d->dtype == TADMM_CHAIN_F32 ? 4 : 2, d->d);
  return 1;
}

int tadmm_attn_workspace_bytes(const tadmm_attn_desc* d, size_t* bytes) {
  if (!d || !bytes || d->B < 0 || d->H < 1 || d->S < 1) return TADMM_ERR_INVALID;
  *bytes = attn_ws_bytes(d->B, d->H, d->S);
  return TADMM_OK;
}

int tadmm_attn_fwd(tadmm_handle h, const tadmm_attn_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  AttnArgs a;
  unsigned grid = 0;
  bool skip = false;
  const int rc = attn_check(h, d, "attn_fwd", false, &a, &grid, &skip);
  if (rc != TADMM_OK || skip) return rc;
  DeviceGuard device_guard(h);
  hipStream_t s = (hipStream_t)stream_;
  if (d->dtype == TADMM_CHAIN_F32) attn_launch_fwd<float>(a, grid, s);
  else if (d->dtype == TADMM_CHAIN_BF16) attn_launch_fwd<attn_bf16>(a, grid, s);
  else attn_launch_fwd<attn_f16>(a, grid, s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_attn_bwd(tadmm_handle h, const tadmm_attn_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  AttnArgs a;
  unsigned grid = 0;
  bool skip = false;
  const int rc = attn_check(h, d, "attn_bwd", true, &a, &grid, &skip);
  if (rc != TADMM_OK || skip) return rc;
  DeviceGuard device_guard(h);
  hipStream_t s = (hipStream_t)stream_;
  if (d->dtype == TADMM_CHAIN_F32) attn_launch_bwd<float>(a, grid, s);
  else attn_launch_bwd<attn_bf16>(a, grid, s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
