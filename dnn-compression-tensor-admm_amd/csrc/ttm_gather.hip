// Gathered TT-matrix chain: the lookup of the factorised embeddings (TTMEmbedding.py:96-129, TTEmbedding.py:91-118,
// SVDEmbedding.py:34-42) in ONE launch, and its core gradients in one launch per core.
//
// Cores G_j (r_j, n_j, m_j, r_{j+1}), j = 0 .. d-1, d <= 4, r_0 = 1, float32 contiguous.  Token t carries an index in
// [0, n_0 ... n_{d-1}), split into (i_0 .. i_{d-1}) with i_0 slowest.  With the slice S_j = G_j[:, i_j, :, :] and
// P_j = m_0 ... m_{j-1}, the running product A_j (P_j x r_j, A_0 = [1]) obeys
//     A_{j+1}[(p, jj), b] = sum_a A_j[p, a] * S_j[a, jj, b]
// and A_d (P_d x r_d) is the output row.  For fixed a the slice is m_j * r_{j+1} contiguous floats of the core, so
// lanes that walk (jj, b) load coalesced; the cores are small (KiB .. a few MiB) and live in L2.
//
// Forward: a workgroup of 256 threads takes a tile of tokens (ttm_geom: 1 .. 16, more tokens where a row is short),
// splits every index with integer arithmetic, keeps A_j of every token of the tile in LDS in two buffers used
// alternately (odd j / even j), and writes A_d straight to the output: no token-sized temporary in HBM.  A thread owns a
// column c = (jj, b) and kTtmRP rows p of the product: one global load of the slice feeds kTtmRP FMAs whose other
// operand is an LDS broadcast.  Plain fp32 FMAs (DESIGN.md section 16 has the reason).
//
// Backward, core j:  dS_j[a, jj, b] = sum_{p, q} L[p, a] * dY[p, jj, q] * R[b, q],  L = A_j, R = R_{j+1}, where the
// right products R_j (r_j x Q_j, Q_j = m_j ... m_{d-1} r_d, R_d = I) obey R_j[a, (jj, q)] = sum_b S_j[a, jj, b] R_{j+1}[b, q].
// The caller passes the tokens grouped by i_j (a stable sort: ascending token order inside a group) and the group
// offsets.  Workgroup i of the launch owns slice i of dG_j, all of it: it writes zeros, then for each token of its group,
// in order, recomputes L and R in LDS, forms V[p, jj, b] = sum_q dY[p, jj, q] R[b, q] in LDS and adds
// sum_p L[p, a] V[p, jj, b] to its slice (every element is read and written by one fixed thread).  No atomics, no
// memset, bitwise reproducible; slices that no token selects stay zero.
//
// An index outside [0, N) is never used as an address: the forward writes a zero row and adds 1 to *bad_count (the one
// atomic of this file), the backward skips the token.
#include "host.h"

namespace tadmm {
namespace {

constexpr int kTtmMaxD = 4;
constexpr int kTtmMaxTile = 16;             // tokens of a forward workgroup at most
constexpr int kTtmRP = 4;                   // rows of the running product per work item
constexpr int kTtmFwdThreads = 256;
constexpr int kTtmBwdThreads = 1024;
constexpr size_t kTtmMaxLds = 160 * 1024;   // dynamic LDS only: static LDS would come off the same 160 KiB
constexpr int kTtmFwdHeader = kTtmMaxD * kTtmMaxTile * 4;   // mode indices of the tile's tokens (int32), -1 = bad index

struct TtmGeom {
  int d = 0;
  int n[kTtmMaxD] = {1, 1, 1, 1}, m[kTtmMaxD] = {1, 1, 1, 1}, r[kTtmMaxD + 1] = {1, 1, 1, 1, 1};
  int P[kTtmMaxD + 1] = {1, 1, 1, 1, 1};    // P[j] = m_0 ... m_{j-1}
  int Q[kTtmMaxD + 1] = {1, 1, 1, 1, 1};    // Q[j] = m_j ... m_{d-1} * r_d
  int64_t stride[kTtmMaxD] = {1, 1, 1, 1};  // index stride of mode j
  int64_t N = 1;                            // n_0 ... n_{d-1}
  int s[2] = {0, 0};                        // floats per token of the two left buffers (states of even / odd j)
  int maxR = 0, maxV = 0;
  int row = 1;                              // P_d * r_d
  int tile = 0;                             // 0 with sized == false
  size_t fwd_lds = 0, bwd_lds = 0;
  bool sized = false;                       // false: a core or a product beyond 32-bit indexing, nothing was sized
  bool fits = false;
};

// TADMM_ERR_INVALID for what no route takes; otherwise g.fits says whether the launches take the shape, and g.sized
// whether the LDS figures mean anything (sizes beyond 32-bit indexing are refused before they are computed).
int ttm_geom(const tadmm_ttm_desc* c, TtmGeom& g) {
  if (!c || c->d < 1 || c->d > kTtmMaxD) return TADMM_ERR_INVALID;
  g.d = c->d;
  for (int j = 0; j < g.d; ++j) {
    if (c->n[j] <= 0 || c->m[j] <= 0 || c->r[j] <= 0) return TADMM_ERR_INVALID;
    g.n[j] = c->n[j]; g.m[j] = c->m[j]; g.r[j] = c->r[j];
  }
  if (c->r[g.d] <= 0 || c->r[0] != 1) return TADMM_ERR_INVALID;
  g.r[g.d] = c->r[g.d];
  const int64_t big = (int64_t)1 << 30;
  int64_t N = 1;
  for (int j = g.d - 1; j >= 0; --j) {
    g.stride[j] = N;
    if (N > ((int64_t)1 << 62) / g.n[j]) return TADMM_ERR_INVALID;
    N *= g.n[j];
  }
  g.N = N;
  g.fits = false;
  int64_t P = 1, maxE = 0, s[2] = {0, 0}, maxV = 0, maxR = 0;
  for (int j = 0; j < g.d; ++j) {
    if ((int64_t)g.r[j] * g.n[j] * g.m[j] * g.r[j + 1] >= ((int64_t)1 << 31)) return TADMM_OK;   // a core of 2^31 elements
    P *= g.m[j];
    if (P * g.r[j + 1] > big) return TADMM_OK;
    g.P[j + 1] = (int)P;
    const int64_t e = P * g.r[j + 1];
    maxE = std::max(maxE, e);
    maxV = std::max(maxV, e);
    if (j + 1 < g.d) s[(j + 1) & 1] = std::max(s[(j + 1) & 1], e);
  }
  int64_t Q = g.r[g.d];
  g.Q[g.d] = (int)Q;
  for (int j = g.d - 1; j >= 0; --j) {
    Q *= g.m[j];
    if (Q * g.r[j] > big) return TADMM_OK;
    g.Q[j] = (int)Q;
    if (j >= 1) maxR = std::max(maxR, Q * g.r[j]);
  }
  g.row = g.P[g.d] * g.r[g.d];
  g.s[0] = (int)s[0]; g.s[1] = (int)s[1]; g.maxR = (int)maxR; g.maxV = (int)maxV;
  const size_t per_token = 4 * (size_t)(s[0] + s[1]);
  int tile = (int)std::min<int64_t>(kTtmMaxTile, std::max<int64_t>(1, (2048 + maxE - 1) / maxE));
  while (tile > 1 && kTtmFwdHeader + tile * per_token > 64 * 1024) --tile;
  g.tile = tile;
  g.fwd_lds = kTtmFwdHeader + tile * per_token;
  g.bwd_lds = 16 + 4 * (size_t)(s[0] + s[1] + 2 * maxR + maxV);
  g.sized = true;
  g.fits = g.fwd_lds <= kTtmMaxLds && g.bwd_lds <= kTtmMaxLds;
  return TADMM_OK;
}

struct TtmArgs {
  const float* G[kTtmMaxD];
  int32_t n[kTtmMaxD], m[kTtmMaxD], r[kTtmMaxD + 1], P[kTtmMaxD + 1], Q[kTtmMaxD + 1];
  int64_t stride[kTtmMaxD];
  int64_t N, B;
  const void* index;
  int32_t idx64, d, tile;
  int32_t s[2];
  int32_t maxR;
  float* Y;                 // forward: (B, row)
  int32_t* bad;
  int32_t row;
  // backward, one core per launch
  int32_t k;
  const float* dY;
  float* dG;
  const int64_t* order;     // token positions grouped by i_k
  const int64_t* offs;      // n_k + 1 group offsets
};

__device__ __forceinline__ int64_t ttm_index(const TtmArgs& a, int64_t t) {
  return a.idx64 ? reinterpret_cast<const int64_t*>(a.index)[t] : (int64_t) reinterpret_cast<const int32_t*>(a.index)[t];
}

// One mode of the left chain for `ntok` tokens: dst[tok] = A_{j+1} from prev[tok] = A_j.  ik[tok] < 0 marks a bad index:
// nothing is computed for it, and a global destination gets zeros.
template <int NT, bool TO_GLOBAL>
__device__ __forceinline__ void ttm_left_step(const float* __restrict__ G, int nj, int mj, int rj, int rj1, int Pj, int ntok,
                                              const int* ik, const float* prev, int prev_stride, float* dst,
                                              int64_t dst_stride) {
  const int C = mj * rj1;
  const int PB = (Pj + kTtmRP - 1) / kTtmRP;
  const int per_tok = PB * C;
  const int total = ntok * per_tok;
  const int64_t astride = (int64_t)nj * C;
  for (int w = threadIdx.x; w < total; w += NT) {
    const int tok = w / per_tok;
    const int rem = w - tok * per_tok;
    const int pb = rem / C;
    const int c = rem - pb * C;
    const int p0 = pb * kTtmRP;
    const int i = ik[tok];
    float acc[kTtmRP];
#pragma unroll
    for (int u = 0; u < kTtmRP; ++u) acc[u] = 0.f;
    if (i >= 0) {
      const float* s = G + (int64_t)i * C + c;
      const float* pr = prev + (int64_t)tok * prev_stride;
      int rowof[kTtmRP];
#pragma unroll
      for (int u = 0; u < kTtmRP; ++u) rowof[u] = min(p0 + u, Pj - 1) * rj;
      if (prev == nullptr) {
        acc[0] = s[0];                       // A_0 = [1]
      } else {
        for (int aa = 0; aa < rj; ++aa) {
          const float sv = s[aa * astride];
#pragma unroll
          for (int u = 0; u < kTtmRP; ++u) acc[u] = fmaf(pr[rowof[u] + aa], sv, acc[u]);
        }
      }
    } else if (!TO_GLOBAL) {
      continue;
    }
    float* o = dst + (int64_t)tok * dst_stride + (int64_t)p0 * C + c;
#pragma unroll
    for (int u = 0; u < kTtmRP; ++u)
      if (p0 + u < Pj) o[(int64_t)u * C] = acc[u];
  }
}

__global__ __launch_bounds__(kTtmFwdThreads) void ttm_gather_fwd_kernel(TtmArgs a) {
  extern __shared__ __align__(16) unsigned char ttm_lds[];
  int* ik = reinterpret_cast<int*>(ttm_lds);                         // [mode][kTtmMaxTile]
  float* buf[2];
  buf[0] = reinterpret_cast<float*>(ttm_lds + kTtmFwdHeader);
  buf[1] = buf[0] + (size_t)a.tile * a.s[0];
  const int64_t t0 = (int64_t)blockIdx.x * a.tile;
  const int ntok = (int)min((int64_t)a.tile, a.B - t0);
  if ((int)threadIdx.x < ntok) {
    const int64_t idx = ttm_index(a, t0 + threadIdx.x);
    const bool ok = idx >= 0 && idx < a.N;
    if (!ok) atomicAdd(a.bad, 1);
    for (int j = 0; j < a.d; ++j) ik[j * kTtmMaxTile + threadIdx.x] = ok ? (int)((idx / a.stride[j]) % a.n[j]) : -1;
  }
  __syncthreads();
  for (int j = 0; j < a.d; ++j) {
    const float* prev = j == 0 ? nullptr : buf[j & 1];
    const int prev_stride = a.s[j & 1];
    if (j + 1 == a.d) {
      ttm_left_step<kTtmFwdThreads, true>(a.G[j], a.n[j], a.m[j], a.r[j], a.r[j + 1], a.P[j], ntok, ik + j * kTtmMaxTile, prev,
                                          prev_stride, a.Y + t0 * a.row, a.row);
    } else {
      ttm_left_step<kTtmFwdThreads, false>(a.G[j], a.n[j], a.m[j], a.r[j], a.r[j + 1], a.P[j], ntok, ik + j * kTtmMaxTile, prev,
                                           prev_stride, buf[(j + 1) & 1], a.s[(j + 1) & 1]);
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kTtmBwdThreads) void ttm_gather_bwd_kernel(TtmArgs a) {
  constexpr int NT = kTtmBwdThreads;
  extern __shared__ __align__(16) unsigned char ttm_lds[];
  int* ik = reinterpret_cast<int*>(ttm_lds);                         // [mode], one token at a time
  float* lbuf[2];
  lbuf[0] = reinterpret_cast<float*>(ttm_lds + 16);
  lbuf[1] = lbuf[0] + a.s[0];
  float* rbuf[2];
  rbuf[0] = lbuf[1] + a.s[1];
  rbuf[1] = rbuf[0] + a.maxR;
  float* V = rbuf[1] + a.maxR;

  const int k = a.k, d = a.d;
  const int slice = blockIdx.x;
  const int mk = a.m[k], rk = a.r[k], rk1 = a.r[k + 1], Pk = a.P[k], Qn = a.Q[k + 1];
  const int C = mk * rk1;
  const int E = rk * C;
  const int64_t astride = (int64_t)a.n[k] * C;
  float* dS = a.dG + (int64_t)slice * C;
  for (int w = threadIdx.x; w < E; w += NT) {
    const int aa = w / C;
    dS[aa * astride + (w - aa * C)] = 0.f;
  }
  const int64_t beg = max(a.offs[slice], (int64_t)0), end = min(a.offs[slice + 1], a.B);   // never past `order`
  for (int64_t pos = beg; pos < end; ++pos) {
    const int64_t t = a.order[pos];
    if (t < 0 || t >= a.B) continue;
    const int64_t idx = ttm_index(a, t);
    if (idx < 0 || idx >= a.N) continue;                  // uniform over the workgroup
    if ((int)threadIdx.x < d) ik[threadIdx.x] = (int)((idx / a.stride[threadIdx.x]) % a.n[threadIdx.x]);
    __syncthreads();
    if (ik[k] != slice) {                                 // a group the caller built wrongly adds nothing (uniform)
      __syncthreads();
      continue;
    }
    // left chain: A_k in lbuf[k & 1]
    for (int j = 0; j < k; ++j) {
      ttm_left_step<NT, false>(a.G[j], a.n[j], a.m[j], a.r[j], a.r[j + 1], a.P[j], 1, ik + j, j == 0 ? nullptr : lbuf[j & 1], 0,
                               lbuf[(j + 1) & 1], 0);
      __syncthreads();
    }
    // right chain: R_{k+1} in rbuf[(k + 1) & 1]  (R_d = I is never stored)
    for (int j = d - 1; j > k; --j) {
      const int mj = a.m[j], rj1 = a.r[j + 1], Qj1 = a.Q[j + 1];
      const int total = a.r[j] * mj * Qj1;
      const float* Rn = rbuf[(j + 1) & 1];
      float* Rc = rbuf[j & 1];
      const float* Gj = a.G[j];
      const int ij = ik[j], nj = a.n[j];
      for (int w = threadIdx.x; w < total; w += NT) {
        const int aa = w / (mj * Qj1);
        const int rem = w - aa * (mj * Qj1);
        const int jj = rem / Qj1;
        const int q = rem - jj * Qj1;
        const float* s = Gj + (((int64_t)aa * nj + ij) * mj + jj) * rj1;
        float acc;
        if (j == d - 1) {
          acc = s[q];
        } else {
          acc = 0.f;
          for (int b = 0; b < rj1; ++b) acc = fmaf(s[b], Rn[b * Qj1 + q], acc);
        }
        Rc[w] = acc;
      }
      __syncthreads();
    }
    // V[(p, jj), b] = sum_q dY[(p, jj), q] R[b, q]; the walk over q starts at b so that lanes of consecutive b hit
    // different banks when Q is a multiple of 32 (a fixed order per element all the same)
    const float* dy = a.dY + t * a.row;
    {
      const int total = Pk * C;
      const float* R = rbuf[(k + 1) & 1];
      for (int w = threadIdx.x; w < total; w += NT) {
        const int pj = w / rk1;
        const int b = w - pj * rk1;
        float acc;
        if (k == d - 1) {
          acc = dy[w];
        } else {
          acc = 0.f;
          const float* dyr = dy + (int64_t)pj * Qn;
          const float* Rr = R + b * Qn;
          int q = b % Qn;
          for (int it = 0; it < Qn; ++it) {
            acc = fmaf(dyr[q], Rr[q], acc);
            q = q + 1 == Qn ? 0 : q + 1;
          }
        }
        V[w] = acc;
      }
    }
    __syncthreads();
    {
      const float* L = lbuf[k & 1];
      for (int w = threadIdx.x; w < E; w += NT) {
        const int aa = w / C;
        const int c = w - aa * C;
        float acc = 0.f;
        if (k == 0) {
          acc = V[c];
        } else {
          for (int p = 0; p < Pk; ++p) acc = fmaf(L[p * rk + aa], V[p * C + c], acc);
        }
        float* o = dS + aa * astride + c;
        *o = *o + acc;
      }
    }
    __syncthreads();
  }
}

int ttm_args(tadmm_ctx_s* h, const tadmm_ttm_desc* c, TtmGeom& g, TtmArgs& a) {
  const int rc = ttm_geom(c, g);
  if (rc != TADMM_OK) CTX_FAIL(h, rc, "ttm_gather: 1 <= d <= 4, r_0 = 1 and positive sizes are required");
  if (!g.sized)
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "ttm_gather: a core of 2^31 elements or more, or a product of one token beyond 2^30 floats");
  if (!g.fits)
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "ttm_gather: a token needs %zu bytes of LDS (forward) / %zu (backward), a CU has %zu",
             g.fwd_lds, g.bwd_lds, kTtmMaxLds);
  if (c->B < 0 || c->B >= ((int64_t)1 << 31)) CTX_FAIL(h, TADMM_ERR_INVALID, "ttm_gather: 0 <= B < 2^31 tokens");
  if (c->index_dtype != 0 && c->index_dtype != 1) CTX_FAIL(h, TADMM_ERR_INVALID, "ttm_gather: index_dtype is 0 (int32) or 1 (int64)");
  if (c->B > 0 && (!c->index || ((uintptr_t)c->index & (c->index_dtype ? 7 : 3))))
    CTX_FAIL(h, TADMM_ERR_INVALID, "ttm_gather: index is null or misaligned");
  memset(&a, 0, sizeof a);
  for (int j = 0; j < g.d; ++j) {
    if (!c->cores[j] || ((uintptr_t)c->cores[j] & 3)) CTX_FAIL(h, TADMM_ERR_INVALID, "ttm_gather: core %d is null or misaligned", j);
    a.G[j] = c->cores[j];
    a.n[j] = g.n[j]; a.m[j] = g.m[j]; a.stride[j] = g.stride[j];
  }
  for (int j = 0; j <= kTtmMaxD; ++j) { a.r[j] = g.r[j]; a.P[j] = g.P[j]; a.Q[j] = g.Q[j]; }
  a.N = g.N; a.B = c->B; a.index = c->index; a.idx64 = c->index_dtype; a.d = g.d; a.tile = g.tile;
  a.s[0] = g.s[0]; a.s[1] = g.s[1]; a.maxR = g.maxR; a.row = g.row;
  return TADMM_OK;
}

}  // namespace
}  // namespace tadmm

using namespace tadmm;

extern "C" {

int tadmm_ttm_desc_bytes(void) { return (int)sizeof(tadmm_ttm_desc); }

int tadmm_ttm_gather_fits(const tadmm_ttm_desc* d, size_t* lds_bytes, int* tile) {
  TtmGeom g;
  const int rc = ttm_geom(d, g);
  if (rc != TADMM_OK) return rc;
  if (lds_bytes) *lds_bytes = std::max(g.fwd_lds, g.bwd_lds);
  if (tile) *tile = g.tile;
  return g.fits ? 1 : 0;
}

int tadmm_ttm_gather_fwd(tadmm_handle h, const tadmm_ttm_desc* d, void* stream) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  TtmGeom g;
  TtmArgs a;
  const int rc = ttm_args(h, d, g, a);
  if (rc != TADMM_OK) return rc;
  if (a.B == 0) return TADMM_OK;
  if (!d->Y || ((uintptr_t)d->Y & 3) || !d->bad_count || ((uintptr_t)d->bad_count & 3))
    CTX_FAIL(h, TADMM_ERR_INVALID, "ttm_gather_fwd: Y or bad_count is null or misaligned");
  a.Y = d->Y; a.bad = d->bad_count;
  static DynLdsOptIn allow_lds;
  if (g.fwd_lds > 64 * 1024) HIP_OK(h, allow_lds(ttm_gather_fwd_kernel, kTtmMaxLds));
  const int64_t blocks = (a.B + g.tile - 1) / g.tile;
  hipLaunchKernelGGL(ttm_gather_fwd_kernel, dim3((unsigned)blocks), dim3(kTtmFwdThreads), g.fwd_lds, (hipStream_t)stream, a);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_ttm_gather_bwd(tadmm_handle h, const tadmm_ttm_desc* d, void* stream) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  TtmGeom g;
  TtmArgs a;
  const int rc = ttm_args(h, d, g, a);
  if (rc != TADMM_OK) return rc;
  if (a.B > 0 && (!d->dY || ((uintptr_t)d->dY & 3))) CTX_FAIL(h, TADMM_ERR_INVALID, "ttm_gather_bwd: dY is null or misaligned");
  a.dY = d->dY;
  for (int j = 0; j < g.d; ++j) {
    if (!d->dcores[j]) continue;
    if (((uintptr_t)d->dcores[j] & 3) || !d->order[j] || !d->offsets[j] || ((uintptr_t)d->order[j] & 7) ||
        ((uintptr_t)d->offsets[j] & 7))
      CTX_FAIL(h, TADMM_ERR_INVALID, "ttm_gather_bwd: dcores / order / offsets of core %d are null or misaligned", j);
  }
  static DynLdsOptIn allow_lds;
  if (g.bwd_lds > 64 * 1024) HIP_OK(h, allow_lds(ttm_gather_bwd_kernel, kTtmMaxLds));
  for (int j = 0; j < g.d; ++j) {
    if (!d->dcores[j]) continue;
    a.k = j; a.dG = d->dcores[j]; a.order = d->order[j]; a.offs = d->offsets[j];
    hipLaunchKernelGGL(ttm_gather_bwd_kernel, dim3((unsigned)g.n[j]), dim3(kTtmBwdThreads), g.bwd_lds, (hipStream_t)stream, a);
  }
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
