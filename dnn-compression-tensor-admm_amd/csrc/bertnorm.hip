// The tail of every BERT sub-layer (xcompression/transformer/compressed_modeling*.py: *SelfOutput.forward,
// BertOutput.forward, BertEmbeddings, BertPredictionHeadTransform): LayerNorm(dropout(x) + res) with the reference's
// BertLayerNorm (epsilon inside the root), one launch forward, two backward.
//
//     s_ij   = x_ij * (keep_ij != 0) / (1 - p) + res_ij
//     mean_i = sum_j s_ij / hidden,  var_i = sum_j (s_ij - mean_i)^2 / hidden,  rstd_i = 1 / sqrt(var_i + eps)
//     y_ij   = gamma_j * (s_ij - mean_i) * rstd_i + beta_j
//
//   1. bertnorm_fwd_kernel<T, VEC, NV>   a wave owns a row, four waves to a workgroup, rows dealt round-robin over at
//                                        most 1024 workgroups.  Lane l holds columns (i * 64 + l) * VEC .. + VEC - 1 of
//                                        chunk i, NV values in all (rows of up to 64 * NV columns), from the one read of
//                                        x, keep and res to the one write of y.  Two sweeps over the registers: the sum
//                                        of s, then the sum of (s - mean)^2.  Elementwise arithmetic is float32; the two
//                                        row sums alone are added in double, so that mean and rstd are the exact values
//                                        rounded once: an element whose s and whose row mean are both small against the
//                                        row's spread sees the absolute error of the mean undamped (y is judged against
//                                        |gamma| (|s| + |mean|) rstd + |beta|), and a float32 sum of 312 unit-size terms
//                                        is off by some 1e-8, 20 units of such an element.  Row sums are wave
//                                        butterflies; no LDS.  gamma and beta are loaded once per wave.
//   2. bertnorm_bwd_kernel<T, VEC, NV>   the same ownership over at most 512 workgroups.  s and xhat = (s - mean) * rstd
//                                        are recomputed from x, keep, res and the saved (mean, rstd) with the forward's
//                                        own expressions.  a = g * gamma, dsum = rstd (a - mean_j a - xhat mean_j(a xhat)),
//                                        dres = dsum, dx = dsum keep / (1 - p).  A lane owns the same columns in every
//                                        row, so sum_i g xhat and sum_i g accumulate in its registers (float32); waves
//                                        1 .. 3 hand theirs to wave 0 through LDS, which adds them in that order and
//                                        writes the workgroup's partial (2, hidden) to the workspace.
//   3. bertnorm_param_kernel             16 columns x 16 slices to a workgroup: every slice adds its contiguous share
//                                        of the partials in double, in ascending order, slice 0 adds the 16 slice sums
//                                        in ascending order and writes dgamma and dbeta (float32).
// Grids and the row-to-workgroup map depend on (rows, hidden, dtype) alone; no atomics: bitwise reproducible.
// Accesses: VEC elements = 16 bytes when every base is 16-byte aligned, the row strides are whole 16-byte units and
// hidden is a multiple of VEC; one element otherwise.
#include "rownorm_common.h"

namespace tadmm {

struct BnArgs {
  const void* x; const void* res;
  int64_t ldx, ldr;
  const uint8_t* keep;
  const void* gamma; const void* beta;
  void* y; float* stats;
  const void* g; void* dx; void* dres;
  float* part;
  double eps;
  float q;                                   // 1 - p
  int64_t rows;
  int32_t hidden, hp, param_f32;
};

// s = x keep / (1 - p) + res of row r for the columns a lane owns (zeros beyond the row); bit (i * VEC + j) of `kept`
// is set where the element was kept (all ones without dropout).  The one expression of s, forward and backward.
template <typename T, int VEC, int CH>
__device__ __forceinline__ void bn_row(const BnArgs& a, int64_t r, int lane, float (&s)[CH][VEC], uint32_t& kept) {
  const T* __restrict__ xr = (const T*)a.x + r * a.ldx;
  const T* __restrict__ rr = a.res ? (const T*)a.res + r * a.ldr : nullptr;
  const uint8_t* __restrict__ kr = a.keep ? a.keep + r * (int64_t)a.hidden : nullptr;
  kept = 0xffffffffu;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (i * 64 + lane) * VEC;
    if (c < a.hidden) {
      bn_load<T, VEC>(xr + c, s[i]);
      if (kr) {
        BnPack<uint8_t, VEC> k;
        if constexpr (VEC == 1) k.v[0] = kr[c];
        else k = *reinterpret_cast<const BnPack<uint8_t, VEC>*>(kr + c);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          if (k.v[j]) s[i][j] = s[i][j] / a.q;
          else { s[i][j] = 0.f; kept &= ~(1u << (i * VEC + j)); }
        }
      }
      if (rr) {
        float t[VEC];
        bn_load<T, VEC>(rr + c, t);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[i][j] += t[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[i][j] = 0.f;
    }
  }
}

template <typename T, int VEC, int NV>
__global__ __launch_bounds__(256) void bertnorm_fwd_kernel(const BnArgs a) {
  static_assert(NV % VEC == 0 && NV <= 32, "a lane's values are whole chunks and fit the kept-bit word");
  constexpr int CH = NV / VEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hidden = a.hidden;
  const double dh = (double)hidden;
  float gam[CH][VEC], bet[CH][VEC];
  bn_load_param<T, VEC, CH>(a.gamma, a.param_f32 != 0, hidden, lane, gam);
  bn_load_param<T, VEC, CH>(a.beta, a.param_f32 != 0, hidden, lane, bet);
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < a.rows; r += (int64_t)gridDim.x * 4) {
    float s[CH][VEC];
    uint32_t kept;
    bn_row<T, VEC, CH>(a, r, lane, s, kept);
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
      for (int j = 0; j < VEC; ++j) t += (double)s[i][j];
    const float mean = (float)(bn_wave_sum(t) / dh);
    t = 0.0;
#pragma unroll
    for (int i = 0; i < CH; ++i)
      if ((i * 64 + lane) * VEC < hidden)
#pragma unroll
        for (int j = 0; j < VEC; ++j) { const double d = (double)s[i][j] - (double)mean; t += d * d; }
    const float rstd = (float)(1.0 / sqrt(bn_wave_sum(t) / dh + a.eps));
    T* __restrict__ yr = (T*)a.y + r * (int64_t)hidden;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (i * 64 + lane) * VEC;
      if (c < hidden) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = gam[i][j] * bn_xhat(s[i][j], mean, rstd) + bet[i][j];
        bn_store<T, VEC>(yr + c, o);
      }
    }
    if (a.stats && lane == 0) { a.stats[2 * r] = mean; a.stats[2 * r + 1] = rstd; }
  }
}

template <typename T, int VEC, int NV>
__global__ __launch_bounds__(256) void bertnorm_bwd_kernel(const BnArgs a) {
  static_assert(NV % VEC == 0 && NV <= 32, "a lane's values are whole chunks and fit the kept-bit word");
  constexpr int CH = NV / VEC;
  __shared__ float red[3][NV][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hidden = a.hidden;
  const float fh = (float)hidden;
  float gam[CH][VEC], ag[CH][VEC], ab[CH][VEC];
  bn_load_param<T, VEC, CH>(a.gamma, a.param_f32 != 0, hidden, lane, gam);
#pragma unroll
  for (int i = 0; i < CH; ++i)
#pragma unroll
    for (int j = 0; j < VEC; ++j) ag[i][j] = ab[i][j] = 0.f;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < a.rows; r += (int64_t)gridDim.x * 4) {
    float s[CH][VEC], gv[CH][VEC];
    uint32_t kept;
    bn_row<T, VEC, CH>(a, r, lane, s, kept);
    const T* __restrict__ gr = (const T*)a.g + r * (int64_t)hidden;
    const float mean = a.stats[2 * r], rstd = a.stats[2 * r + 1];
    float sa = 0.f, sax = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (i * 64 + lane) * VEC;
      if (c < hidden) {
        bn_load<T, VEC>(gr + c, gv[i]);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          // a is rounded once and kept: the row mean below and the difference a - mean_j a must see one value (a
          // product contracted into the subtraction would leave its rounding residual, times rstd, in a constant row)
          const float xh = bn_xhat(s[i][j], mean, rstd), av = __fmul_rn(gv[i][j], gam[i][j]);
          s[i][j] = xh;
          sa += av;
          sax += av * xh;
          ag[i][j] += gv[i][j] * xh;
          ab[i][j] += gv[i][j];
          gv[i][j] = av;
        }
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) gv[i][j] = 0.f;
      }
    }
    const float ma = bn_wave_sum(sa) / fh, max_ = bn_wave_sum(sax) / fh;
    T* __restrict__ dxr = a.dx ? (T*)a.dx + r * (int64_t)hidden : nullptr;
    T* __restrict__ drr = a.dres ? (T*)a.dres + r * (int64_t)hidden : nullptr;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (i * 64 + lane) * VEC;
      if (c < hidden) {
        float ds[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) ds[j] = rstd * ((gv[i][j] - ma) - s[i][j] * max_);
        if (drr) bn_store<T, VEC>(drr + c, ds);
        if (dxr) {
          if (a.keep) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) ds[j] = ((kept >> (i * VEC + j)) & 1u) ? ds[j] / a.q : 0.f;
          }
          bn_store<T, VEC>(dxr + c, ds);
        }
      }
    }
  }
  if (!a.part) return;
  // waves 1 .. 3 -> wave 0, which adds them in that order; first the sums of g xhat, then the sums of g
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (wave > 0) {
#pragma unroll
      for (int i = 0; i < CH; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) red[wave - 1][i * VEC + j][lane] = pass ? ab[i][j] : ag[i][j];
    }
    __syncthreads();
    if (wave == 0) {
      float* __restrict__ out = a.part + ((int64_t)blockIdx.x * 2 + pass) * a.hp;
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (i * 64 + lane) * VEC;
        if (c < hidden) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            float v = pass ? ab[i][j] : ag[i][j];
            v += red[0][i * VEC + j][lane];
            v += red[1][i * VEC + j][lane];
            v += red[2][i * VEC + j][lane];
            out[c + j] = v;
          }
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void bertnorm_param_kernel(const float* __restrict__ part, int nwg, int hidden, int hp,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double red[2][16][16];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const int per = (nwg + 15) / 16, lo = sl * per, hi = min(nwg, lo + per);
  double sg = 0.0, sb = 0.0;
  if (c < hidden) {
#pragma unroll 8
    for (int w = lo; w < hi; ++w) {
      sg += (double)part[(int64_t)(2 * w) * hp + c];
      sb += (double)part[(int64_t)(2 * w + 1) * hp + c];
    }
  }
  red[0][sl][cl] = sg;
  red[1][sl][cl] = sb;
  __syncthreads();
  if (sl != 0 || c >= hidden) return;
  double tg = 0.0, tb = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { tg += red[0][k][cl]; tb += red[1][k][cl]; }
  if (dgamma) dgamma[c] = (float)tg;
  if (dbeta) dbeta[c] = (float)tb;
}

void bn_param_launch(const float* part, int nwg, int hidden, int hp, float* dgamma, float* dbeta, hipStream_t s) {
  hipLaunchKernelGGL(bertnorm_param_kernel, dim3((unsigned)((hidden + 15) / 16)), dim3(256), 0, s, part, nwg, hidden, hp,
                     dgamma, dbeta);
}

}  // namespace tadmm

using namespace tadmm;

namespace {

template <typename T, bool BWD>
void bn_launch(const BnArgs& a, bool wide, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  const dim3 grid((unsigned)bn_grid(a.rows, BWD ? kBnBwdGrid : kBnFwdGrid)), block(256);
#define BN_GO(VV, NV)                                                                            \
  do {                                                                                           \
    if constexpr (BWD) hipLaunchKernelGGL((bertnorm_bwd_kernel<T, VV, NV>), grid, block, 0, s, a); \
    else hipLaunchKernelGGL((bertnorm_fwd_kernel<T, VV, NV>), grid, block, 0, s, a);             \
  } while (0)
#define BN_WIDTH(VV)                               \
  do {                                             \
    if (a.hidden <= 512) BN_GO(VV, 8);             \
    else if (a.hidden <= 1024) BN_GO(VV, 16);      \
    else BN_GO(VV, 32);                            \
  } while (0)
  if (wide) BN_WIDTH(V);
  else BN_WIDTH(1);
#undef BN_WIDTH
#undef BN_GO
}

// what the two launches share: returns TADMM_OK with *wide set, or the refusal
int bn_check(tadmm_ctx_s* h, const tadmm_bertnorm_desc* d, bool bwd, bool* wide) {
  if (!d) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: the descriptor is NULL");
  if (d->rows < 0 || d->hidden < 1)
    CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: rows >= 0 and hidden >= 1 are required (got %lld x %d)", (long long)d->rows,
             d->hidden);
  if (d->dtype != TADMM_CHAIN_F32 && d->dtype != TADMM_CHAIN_BF16 && d->dtype != TADMM_CHAIN_F16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: unknown element type %d", d->dtype);
  if (bwd && d->dtype == TADMM_CHAIN_F16) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: float16 is forward only");
  if (d->param_dtype != TADMM_CHAIN_F32 && d->param_dtype != d->dtype)
    CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: gamma and beta are float32 or of the type of x (got type %d)", d->param_dtype);
  const size_t es = d->dtype == TADMM_CHAIN_F32 ? 4 : 2, ps = d->param_dtype == TADMM_CHAIN_F32 ? 4 : 2;
  const int64_t H = d->hidden;
  if (!d->x) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: x is NULL");
  if (((uintptr_t)d->x) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: x is not aligned to its element");
  if (((uintptr_t)d->res) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: res is not aligned to its element");
  if (d->x_ld < H) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: row stride of x %lld < hidden %lld", (long long)d->x_ld, (long long)H);
  if (d->res && d->res_ld < H)
    CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: row stride of res %lld < hidden %lld", (long long)d->res_ld, (long long)H);
  if (!(d->p >= 0.0 && d->p < 1.0)) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: p %g outside [0, 1)", d->p);
  if (d->p > 0.0 && !d->keep) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: p > 0 without a keep tensor");
  if (!(d->eps >= 0.0) || !(d->eps < INFINITY)) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: eps %g must be finite and >= 0", d->eps);
  if (!d->gamma || ((uintptr_t)d->gamma) % ps) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: gamma is NULL or misaligned");
  if (!bwd && (!d->beta || ((uintptr_t)d->beta) % ps)) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: beta is NULL or misaligned");
  if (((uintptr_t)d->stats) % 4) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: stats is misaligned");
  bool w = ((uintptr_t)d->x) % 16 == 0 && ((uintptr_t)d->res) % 16 == 0 && ((size_t)d->x_ld * es) % 16 == 0 &&
           (!d->res || ((size_t)d->res_ld * es) % 16 == 0) && ((size_t)H * es) % 16 == 0 &&
           (d->p == 0.0 || ((uintptr_t)d->keep) % 8 == 0);
  if (!bwd) {
    if (!d->y || ((uintptr_t)d->y) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: y is NULL or misaligned");
    w = w && ((uintptr_t)d->y) % 16 == 0;
  } else {
    if (!d->stats) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: stats is NULL and the backward reads it");
    if (!d->g || ((uintptr_t)d->g) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: the upstream gradient g is NULL or misaligned");
    if (((uintptr_t)d->dx) % es || ((uintptr_t)d->dres) % es)
      CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: dx / dres are not aligned to their element");
    if (d->dx && d->dx == d->dres) CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: dx and dres are one buffer");
    if (((uintptr_t)d->dgamma) % 4 || ((uintptr_t)d->dbeta) % 4)
      CTX_FAIL(h, TADMM_ERR_INVALID, "bertnorm: dgamma / dbeta are misaligned");
    w = w && ((uintptr_t)d->g) % 16 == 0 && ((uintptr_t)d->dx) % 16 == 0 && ((uintptr_t)d->dres) % 16 == 0;
  }
  if (H > kBnHmax) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "bertnorm: hidden = %lld, the launch takes 1 <= hidden <= %d", (long long)H, kBnHmax);
  if (bwd && (d->dgamma || d->dbeta) && d->rows > 0) {
    const size_t need = bn_ws_bytes(d->rows, d->hidden);
    if (!d->workspace || ((uintptr_t)d->workspace) % 16 || d->workspace_bytes < need)
      CTX_FAIL(h, TADMM_ERR_WORKSPACE, "bertnorm workspace too small or misaligned: need %zu bytes, got %zu", need,
               d->workspace_bytes);
  }
  *wide = w;
  return TADMM_OK;
}

BnArgs bn_args(const tadmm_bertnorm_desc* d) {
  BnArgs a{};
  a.x = d->x; a.res = d->res; a.ldx = d->x_ld; a.ldr = d->res_ld;
  a.keep = d->p > 0.0 ? d->keep : nullptr;
  a.gamma = d->gamma; a.beta = d->beta;
  a.y = d->y; a.stats = d->stats; a.g = d->g; a.dx = d->dx; a.dres = d->dres;
  a.q = (float)(1.0 - d->p); a.eps = d->eps;
  a.rows = d->rows; a.hidden = d->hidden; a.hp = bn_hp(d->hidden);
  a.param_f32 = d->param_dtype == TADMM_CHAIN_F32;
  return a;
}

}  // namespace

extern "C" {

int tadmm_bertnorm_desc_bytes(void) { return (int)sizeof(tadmm_bertnorm_desc); }

int tadmm_bertnorm_fits(const tadmm_bertnorm_desc* d, int* hmax) {
  if (hmax) *hmax = kBnHmax;
  if (!d || d->hidden < 1) return TADMM_ERR_INVALID;
  return d->hidden <= kBnHmax ? 1 : 0;
}

int tadmm_bertnorm_workspace_bytes(const tadmm_bertnorm_desc* d, size_t* bytes) {
  if (!d || !bytes || d->rows < 0 || d->hidden < 1) return TADMM_ERR_INVALID;
  *bytes = d->rows == 0 ? 0 : bn_ws_bytes(d->rows, d->hidden);
  return TADMM_OK;
}

int tadmm_bertnorm_fwd(tadmm_handle h, const tadmm_bertnorm_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  const int rc = bn_check(h, d, false, &wide);
  if (rc != TADMM_OK) return rc;
  if (d->rows == 0) return TADMM_OK;
  DeviceGuard device_guard(h);
  const BnArgs a = bn_args(d);
  hipStream_t s = (hipStream_t)stream_;
  if (d->dtype == TADMM_CHAIN_F32) bn_launch<float, false>(a, wide, s);
  else if (d->dtype == TADMM_CHAIN_BF16) bn_launch<bn_bf16, false>(a, wide, s);
  else bn_launch<bn_f16, false>(a, wide, s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_bertnorm_bwd(tadmm_handle h, const tadmm_bertnorm_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  const int rc = bn_check(h, d, true, &wide);
  if (rc != TADMM_OK) return rc;
  if (d->rows == 0) return TADMM_OK;
  DeviceGuard device_guard(h);
  BnArgs a = bn_args(d);
  const bool params = d->dgamma || d->dbeta;
  a.part = params ? (float*)d->workspace : nullptr;
  hipStream_t s = (hipStream_t)stream_;
  if (d->dtype == TADMM_CHAIN_F32) bn_launch<float, true>(a, wide, s);
  else bn_launch<bn_bf16, true>(a, wide, s);
  if (params)
    bn_param_launch(a.part, bn_grid(d->rows, kBnBwdGrid), d->hidden, a.hp, d->dgamma, d->dbeta, s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
