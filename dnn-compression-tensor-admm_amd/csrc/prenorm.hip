// The tail of a pre-norm transformer branch (vit_tt.py: TTBlock, through timm's Block.forward): the residual stream takes
// the branch output behind its dropout and its per-sample DropPath, and the next branch reads the LayerNorm of the new
// stream (nn.LayerNorm: biased variance, epsilon inside the root).  Both are outputs: one launch forward, two backward.
//
//     scale_i = (path_keep[i / N] != 0) / (1 - p_path)                       (1 without DropPath; N rows to a sample)
//     s_ij    = x_ij + scale_i * b_ij * (keep_ij != 0) / (1 - p)             rounded to the type of x and written
//     mean_i  = sum_j s_ij / C,  var_i = sum_j (s_ij - mean_i)^2 / C,  rstd_i = 1 / sqrt(var_i + eps)    of s as written
//     y_ij    = gamma_j * (s_ij - mean_i) * rstd_i + beta_j
//
// The statistics are those of the stored s: the caller keeps s as the stream, the backward reads it back and recomputes
// xhat = (s - mean) rstd with the forward's expression, so neither x nor b is saved.
//
//   1. prenorm_fwd_kernel<T, VEC, NV>   ownership and arithmetic of bertnorm_fwd_kernel (rownorm_common.h holds what the
//                                       two share): a wave owns a row, four waves to a workgroup, rows dealt round-robin
//                                       over at most 1024 workgroups; lane l holds columns (i * 64 + l) * VEC .. + VEC - 1
//                                       of chunk i from the one read of x, b and keep; s is written as the chunk is
//                                       formed, y after the two register sweeps whose sums are added in double.  A row
//                                       of a dropped sample takes s = x without touching the value.
//   2. prenorm_bwd_kernel<T, VEC, NV>   the same ownership over at most 512 workgroups.  Reads s, stats, g_y and g_s:
//                                       a = g_y gamma, ds = g_s + rstd (a - mean_j a - xhat mean_j(a xhat)), dx = ds,
//                                       db = ds scale keep / (1 - p) (two stores, two buffers).  A missing g_y or g_s
//                                       is zero.  sum_i g_y xhat and sum_i g_y stay in a lane's registers across its
//                                       rows; waves 1 .. 3 hand theirs to wave 0 through LDS, which adds them in that
//                                       order and writes the workgroup's partial (2, C) to the workspace.
//   3. bertnorm_param_kernel            (bertnorm.hip) adds the partials in double in a fixed order.
// Grids and the row-to-workgroup map depend on (rows, C, dtype) alone; no atomics: bitwise reproducible.
// Accesses: VEC elements = 16 bytes when every base is 16-byte aligned, the row strides are whole 16-byte units and C
// is a multiple of VEC; one element otherwise.
#include "rownorm_common.h"

namespace tadmm {

struct PnArgs {
  const void* x; const void* b;
  int64_t ldx, ldb;
  const uint8_t* keep; const uint8_t* path_keep;
  const void* gamma; const void* beta;
  void* s; void* y; float* stats;
  const void* gy; const void* gs; void* dx; void* db;
  float* part;
  double eps;
  float q, qpath;                            // 1 - p, 1 - p_path
  int64_t rows, nper;                        // nper: rows of a sample
  int32_t hidden, hp, param_f32;
};

template <int VEC>
__device__ __forceinline__ void pn_load_keep(const uint8_t* __restrict__ p, BnPack<uint8_t, VEC>& k) {
  if constexpr (VEC == 1) k.v[0] = p[0];
  else k = *reinterpret_cast<const BnPack<uint8_t, VEC>*>(p);
}

// scale keep / (1 - p) applied to v, the one expression of forward (to b) and backward (to ds): the element's dropout,
// then the sample's DropPath (`alive`), each a division of what is kept and an exact zero for what is not
template <int VEC>
__device__ __forceinline__ void pn_gate(const PnArgs& a, const uint8_t* __restrict__ kr, int c, bool alive, float (&v)[VEC]) {
  if (kr) {
    BnPack<uint8_t, VEC> k;
    pn_load_keep<VEC>(kr + c, k);
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = k.v[j] ? v[j] / a.q : 0.f;
  }
  if (a.path_keep) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = alive ? v[j] / a.qpath : 0.f;
  }
}

template <typename T, int VEC, int NV>
__global__ __launch_bounds__(256) void prenorm_fwd_kernel(const PnArgs a) {
  static_assert(NV % VEC == 0 && NV <= kBnMaxNV, "a lane's values are whole chunks");
  constexpr int CH = NV / VEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hidden = a.hidden;
  const double dh = (double)hidden;
  float gam[CH][VEC], bet[CH][VEC];
  bn_load_param<T, VEC, CH>(a.gamma, a.param_f32 != 0, hidden, lane, gam);
  bn_load_param<T, VEC, CH>(a.beta, a.param_f32 != 0, hidden, lane, bet);
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < a.rows; r += (int64_t)gridDim.x * 4) {
    const T* __restrict__ xr = (const T*)a.x + r * a.ldx;
    const T* __restrict__ br = (const T*)a.b + r * a.ldb;
    const uint8_t* __restrict__ kr = a.keep ? a.keep + r * (int64_t)hidden : nullptr;
    const bool alive = a.path_keep ? a.path_keep[r / a.nper] != 0 : true;
    T* __restrict__ sr = (T*)a.s + r * (int64_t)hidden;
    float s[CH][VEC];
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (i * 64 + lane) * VEC;
      if (c < hidden) {
        bn_load<T, VEC>(xr + c, s[i]);
        if (alive) {
          float bv[VEC];
          bn_load<T, VEC>(br + c, bv);
          pn_gate<VEC>(a, kr, c, true, bv);
#pragma unroll
          for (int j = 0; j < VEC; ++j) s[i][j] = bn_widen(bn_narrow<T>(s[i][j] + bv[j]));   // s as stored
        }
        bn_store<T, VEC>(sr + c, s[i]);
#pragma unroll
        for (int j = 0; j < VEC; ++j) t += (double)s[i][j];
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[i][j] = 0.f;
      }
    }
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
__global__ __launch_bounds__(256) void prenorm_bwd_kernel(const PnArgs a) {
  static_assert(NV % VEC == 0 && NV <= kBnMaxNV, "a lane's values are whole chunks");
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
    const T* __restrict__ sr = (const T*)a.s + r * (int64_t)hidden;
    const T* __restrict__ gr = a.gy ? (const T*)a.gy + r * (int64_t)hidden : nullptr;
    const T* __restrict__ hr = a.gs ? (const T*)a.gs + r * (int64_t)hidden : nullptr;
    const uint8_t* __restrict__ kr = a.keep ? a.keep + r * (int64_t)hidden : nullptr;
    const bool alive = a.path_keep ? a.path_keep[r / a.nper] != 0 : true;
    float xh[CH][VEC], av[CH][VEC];
    float ma = 0.f, max_ = 0.f, rstd = 0.f;
    if (gr) {
      const float mean = a.stats[2 * r];
      rstd = a.stats[2 * r + 1];
      float sa = 0.f, sax = 0.f;
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (i * 64 + lane) * VEC;
        if (c < hidden) {
          float sv[VEC], gv[VEC];
          bn_load<T, VEC>(sr + c, sv);
          bn_load<T, VEC>(gr + c, gv);
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            // a is rounded once and kept: the row mean below and the difference a - mean_j a must see one value
            const float h = bn_xhat(sv[j], mean, rstd), v = __fmul_rn(gv[j], gam[i][j]);
            xh[i][j] = h;
            av[i][j] = v;
            sa += v;
            sax += v * h;
            ag[i][j] += gv[j] * h;
            ab[i][j] += gv[j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < VEC; ++j) xh[i][j] = av[i][j] = 0.f;
        }
      }
      ma = bn_wave_sum(sa) / fh;
      max_ = bn_wave_sum(sax) / fh;
    }
    T* __restrict__ dxr = a.dx ? (T*)a.dx + r * (int64_t)hidden : nullptr;
    T* __restrict__ dbr = a.db ? (T*)a.db + r * (int64_t)hidden : nullptr;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (i * 64 + lane) * VEC;
      if (c < hidden) {
        float ds[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) ds[j] = gr ? rstd * ((av[i][j] - ma) - xh[i][j] * max_) : 0.f;
        if (hr) {
          float hv[VEC];
          bn_load<T, VEC>(hr + c, hv);
#pragma unroll
          for (int j = 0; j < VEC; ++j) ds[j] += hv[j];
        }
        if (dxr) bn_store<T, VEC>(dxr + c, ds);
        if (dbr) {
          pn_gate<VEC>(a, kr, c, alive, ds);
          bn_store<T, VEC>(dbr + c, ds);
        }
      }
    }
  }
  if (!a.part) return;
  // waves 1 .. 3 -> wave 0, which adds them in that order; first the sums of g_y xhat, then the sums of g_y
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

}  // namespace tadmm

using namespace tadmm;

namespace {

template <typename T, bool BWD>
void pn_launch(const PnArgs& a, bool wide, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  const dim3 grid((unsigned)bn_grid(a.rows, BWD ? kBnBwdGrid : kBnFwdGrid)), block(256);
#define PN_GO(VV, NV)                                                                           \
  do {                                                                                          \
    if constexpr (BWD) hipLaunchKernelGGL((prenorm_bwd_kernel<T, VV, NV>), grid, block, 0, s, a); \
    else hipLaunchKernelGGL((prenorm_fwd_kernel<T, VV, NV>), grid, block, 0, s, a);             \
  } while (0)
#define PN_WIDTH(VV)                               \
  do {                                             \
    if (a.hidden <= 512) PN_GO(VV, 8);             \
    else if (a.hidden <= 1024) PN_GO(VV, 16);      \
    else PN_GO(VV, 32);                            \
  } while (0)
  if (wide) PN_WIDTH(V);
  else PN_WIDTH(1);
#undef PN_WIDTH
#undef PN_GO
}

// what the two launches share: returns TADMM_OK with *wide set, or the refusal
int pn_check(tadmm_ctx_s* h, const tadmm_prenorm_desc* d, bool bwd, bool* wide) {
  if (!d) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: the descriptor is NULL");
  if (d->rows < 0 || d->hidden < 1)
    CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: rows >= 0 and hidden >= 1 are required (got %lld x %d)", (long long)d->rows,
             d->hidden);
  if (d->rows_per_sample < 1 || d->rows % d->rows_per_sample)
    CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: rows %lld are not whole samples of rows_per_sample %lld", (long long)d->rows,
             (long long)d->rows_per_sample);
  if (d->dtype != TADMM_CHAIN_F32 && d->dtype != TADMM_CHAIN_BF16 && d->dtype != TADMM_CHAIN_F16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: unknown element type %d", d->dtype);
  if (bwd && d->dtype == TADMM_CHAIN_F16) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: float16 is forward only");
  if (d->param_dtype != TADMM_CHAIN_F32 && d->param_dtype != d->dtype)
    CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: gamma and beta are float32 or of the type of x (got type %d)", d->param_dtype);
  const size_t es = d->dtype == TADMM_CHAIN_F32 ? 4 : 2, ps = d->param_dtype == TADMM_CHAIN_F32 ? 4 : 2;
  const int64_t H = d->hidden;
  if (!(d->p >= 0.0 && d->p < 1.0)) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: p %g outside [0, 1)", d->p);
  if (!(d->p_path >= 0.0 && d->p_path < 1.0)) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: p_path %g outside [0, 1)", d->p_path);
  if (d->p > 0.0 && !d->keep) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: p > 0 without a keep tensor");
  if (d->p_path > 0.0 && !d->path_keep) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: p_path > 0 without a path_keep tensor");
  if (!(d->eps >= 0.0) || !(d->eps < INFINITY)) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: eps %g must be finite and >= 0", d->eps);
  if (!d->gamma || ((uintptr_t)d->gamma) % ps) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: gamma is NULL or misaligned");
  if (!d->s || ((uintptr_t)d->s) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: s is NULL or misaligned");
  if (((uintptr_t)d->stats) % 4) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: stats is misaligned");
  bool w = ((uintptr_t)d->s) % 16 == 0 && ((size_t)H * es) % 16 == 0 && (d->p == 0.0 || ((uintptr_t)d->keep) % 8 == 0);
  if (!bwd) {
    if (!d->x || ((uintptr_t)d->x) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: x is NULL or misaligned");
    if (!d->b || ((uintptr_t)d->b) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: b is NULL or misaligned");
    if (d->x_ld < H) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: row stride of x %lld < hidden %lld", (long long)d->x_ld, (long long)H);
    if (d->b_ld < H) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: row stride of b %lld < hidden %lld", (long long)d->b_ld, (long long)H);
    if (!d->beta || ((uintptr_t)d->beta) % ps) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: beta is NULL or misaligned");
    if (!d->y || ((uintptr_t)d->y) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: y is NULL or misaligned");
    if (d->y == d->s) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: s and y are one buffer");
    w = w && ((uintptr_t)d->x) % 16 == 0 && ((uintptr_t)d->b) % 16 == 0 && ((size_t)d->x_ld * es) % 16 == 0 &&
        ((size_t)d->b_ld * es) % 16 == 0 && ((uintptr_t)d->y) % 16 == 0;
  } else {
    if (!d->stats) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: stats is NULL and the backward reads it");
    if (!d->g_y && !d->g_s) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: the upstream gradients g_y and g_s are both NULL");
    if (((uintptr_t)d->g_y) % es || ((uintptr_t)d->g_s) % es)
      CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: the upstream gradients g_y / g_s are not aligned to their element");
    if (((uintptr_t)d->dx) % es || ((uintptr_t)d->db) % es)
      CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: dx / db are not aligned to their element");
    if (d->dx && d->dx == d->db) CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: dx and db are one buffer");
    if (((uintptr_t)d->dgamma) % 4 || ((uintptr_t)d->dbeta) % 4)
      CTX_FAIL(h, TADMM_ERR_INVALID, "prenorm: dgamma / dbeta are misaligned");
    w = w && ((uintptr_t)d->g_y) % 16 == 0 && ((uintptr_t)d->g_s) % 16 == 0 && ((uintptr_t)d->dx) % 16 == 0 &&
        ((uintptr_t)d->db) % 16 == 0;
  }
  if (H > kBnHmax) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "prenorm: hidden = %lld, the launch takes 1 <= hidden <= %d", (long long)H, kBnHmax);
  if (bwd && (d->dgamma || d->dbeta) && d->rows > 0) {
    const size_t need = bn_ws_bytes(d->rows, d->hidden);
    if (!d->workspace || ((uintptr_t)d->workspace) % 16 || d->workspace_bytes < need)
      CTX_FAIL(h, TADMM_ERR_WORKSPACE, "prenorm workspace too small or misaligned: need %zu bytes, got %zu", need,
               d->workspace_bytes);
  }
  *wide = w;
  return TADMM_OK;
}

PnArgs pn_args(const tadmm_prenorm_desc* d) {
  PnArgs a{};
  a.x = d->x; a.b = d->b; a.ldx = d->x_ld; a.ldb = d->b_ld;
  a.keep = d->p > 0.0 ? d->keep : nullptr;
  a.path_keep = d->p_path > 0.0 ? d->path_keep : nullptr;
  a.gamma = d->gamma; a.beta = d->beta;
  a.s = d->s; a.y = d->y; a.stats = d->stats;
  a.gy = d->g_y; a.gs = d->g_s; a.dx = d->dx; a.db = d->db;
  a.q = (float)(1.0 - d->p); a.qpath = (float)(1.0 - d->p_path); a.eps = d->eps;
  a.rows = d->rows; a.nper = d->rows_per_sample; a.hidden = d->hidden; a.hp = bn_hp(d->hidden);
  a.param_f32 = d->param_dtype == TADMM_CHAIN_F32;
  return a;
}

}  // namespace

extern "C" {

int tadmm_prenorm_desc_bytes(void) { return (int)sizeof(tadmm_prenorm_desc); }

int tadmm_prenorm_fits(const tadmm_prenorm_desc* d, int* hmax) {
  if (hmax) *hmax = kBnHmax;
  if (!d || d->hidden < 1) return TADMM_ERR_INVALID;
  return d->hidden <= kBnHmax ? 1 : 0;
}

int tadmm_prenorm_workspace_bytes(const tadmm_prenorm_desc* d, size_t* bytes) {
  if (!d || !bytes || d->rows < 0 || d->hidden < 1) return TADMM_ERR_INVALID;
  *bytes = d->rows == 0 ? 0 : bn_ws_bytes(d->rows, d->hidden);
  return TADMM_OK;
}

int tadmm_prenorm_fwd(tadmm_handle h, const tadmm_prenorm_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  const int rc = pn_check(h, d, false, &wide);
  if (rc != TADMM_OK) return rc;
  if (d->rows == 0) return TADMM_OK;
  DeviceGuard device_guard(h);
  const PnArgs a = pn_args(d);
  hipStream_t s = (hipStream_t)stream_;
  if (d->dtype == TADMM_CHAIN_F32) pn_launch<float, false>(a, wide, s);
  else if (d->dtype == TADMM_CHAIN_BF16) pn_launch<bn_bf16, false>(a, wide, s);
  else pn_launch<bn_f16, false>(a, wide, s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_prenorm_bwd(tadmm_handle h, const tadmm_prenorm_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  const int rc = pn_check(h, d, true, &wide);
  if (rc != TADMM_OK) return rc;
  if (d->rows == 0) return TADMM_OK;
  DeviceGuard device_guard(h);
  PnArgs a = pn_args(d);
  const bool params = d->dgamma || d->dbeta;
  a.part = params ? (float*)d->workspace : nullptr;
  hipStream_t s = (hipStream_t)stream_;
  if (d->dtype == TADMM_CHAIN_F32) pn_launch<float, true>(a, wide, s);
  else pn_launch<bn_bf16, true>(a, wide, s);
  if (params) bn_param_launch(a.part, bn_grid(d->rows, kBnBwdGrid), d->hidden, a.hp, d->dgamma, d->dbeta, s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
