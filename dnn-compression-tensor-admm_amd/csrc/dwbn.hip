// The middle of a MobileNetV2 inverted-residual block (mobilenetv2_cifar_tt.py: TTBaseBlock, mobilenetv2_tt.py:
// TTInvertedResidual): the depthwise 3x3 convolution (padding 1, stride s = 1 or 2, no bias), BatchNorm2d and ReLU6.
// x is (N, C, H, W), NCHW contiguous; w is (C, 1, 3, 3) float32; the output plane is Ho = (H - 1) / s + 1 by
// Wo = (W - 1) / s + 1 and a channel has M = N Ho Wo output values.
//
//     z[n,c,i,j] = sum_{a,b} w[c,a,b] x[n,c, i s + a - 1, j s + b - 1]          (zero outside the plane; float32, the
//                                                                                nine taps in the order a, b ascending)
//     y          = min(max(gamma_c (z - mean_c) rstd_c + beta_c, 0), 6)          (statistics of z as stored)
//
// Ownership.  A channel's work is cut into U units.  A plane that fits the staged tile (kDwTile floats with its halo)
// is taken whole and G images share a tile; a larger plane is cut into NB bands of RB output rows (G = 1).  Units are
// numbered (image group) * NB + band; workgroup (c, k) = blockIdx.x owns the `per` consecutive units from k * per, so it
// may own several bands of one image and several images.  G, RB, NB, U, S and per come from (N, C, H, W, s) alone
// (dw_plan).  Every unit stages its haloed input rows in LDS (zeros outside the plane), then each thread forms outputs
// from nine LDS reads.
//
//   1. dwbn_conv_kernel<T, VEC, STRIDE, false>  z, stored in the activation type; per-(channel, split) sums of z - K and
//                                               (z - K)^2 of z as stored, in double, K = z[0, c, 0, 0] (every workgroup
//                                               forms it from the same nine taps in the same order).
//   2. dwbn_apply_kernel<T, VEC>                the S partials added in one fixed order; y; split 0 writes stats (mean,
//                                               rstd rounded once), the running statistics and the batch counter.
//      dwbn_conv_kernel<T, VEC, STRIDE, true>   eval: a = gamma / sqrt(running_var + eps), b = beta - running_mean a
//                                               folded in double, y = clamp(a conv(x) + b); the one launch, no z.
//   3. dwbn_bwd_sum_kernel<T, VEC>              gz = g (0 < y < 6) from y as stored; sums of gz and gz xhat in double,
//                                               xhat from the stored z and stats (bn_xhat).
//   4. dwbn_bwd_dx_kernel<T, VEC, STRIDE>       the partials added as in 2; split 0 writes dgamma and dbeta;
//                                               dz = gamma rstd (gz - dbeta / M - xhat dgamma / M) is formed on a
//                                               haloed tile in LDS (one output row above and below the band, never
//                                               stored to memory); dx, the transposed convolution, from it; the nine
//                                               sums dz x of the unit's own outputs in double, one partial per
//                                               workgroup.
//   5. dwbn_dw_kernel                           dw[c, a, b]: the S partials in ascending order, in double.
// Three launches backward (two without dw).  No atomics; grids depend on the shape alone: bitwise reproducible.
// Accesses: 16 bytes when x, z, y (g, dx) are 16-byte aligned and W and Wo are whole numbers of 16-byte units; one
// element otherwise.
#include "rownorm_common.h"

namespace tadmm {

constexpr int kDwTile = 4096;                // floats of one staged tile (16 KiB)
constexpr int kDwTarget = 1024;              // workgroups the plan aims at
constexpr int kDwMaxSplit = 128;             // two partials per lane in the fixed-order sum
constexpr int kDwTileOut = 2048;             // outputs of a tile of whole planes
constexpr int kDwMaxW = kDwTile / 3 - 2;     // three haloed rows must fit
constexpr int64_t kDwMaxM = (int64_t(1) << 31) - 4096;

struct DwArgs {
  const void* x; const float* w; const float* gamma; const float* beta;
  float* rmean; float* rvar; int64_t* nbt;
  void* z; void* y; float* stats;
  const void* g; void* dx; float* dw; float* dgamma; float* dbeta;
  double* part;                              // (C, S, 2)
  double* wpart;                             // (C, S, 9)
  double eps, momentum;
  int32_t N, C, H, W, Ho, Wo, M;
  int32_t G, RB, NB, U, S, per;
};

// a unit: images [n0, n0 + gn) and output rows [i0, i0 + rows)
struct DwUnit { int n0, gn, i0, rows; };

__device__ __forceinline__ DwUnit dw_unit(const DwArgs& a, int u) {
  const int ng = u / a.NB, b = u - ng * a.NB;
  DwUnit q;
  q.n0 = ng * a.G;
  q.gn = min(a.G, a.N - q.n0);
  q.i0 = b * a.RB;
  q.rows = min(a.RB, a.Ho - q.i0);
  return q;
}

#define DW_OWN()                                                       \
  const int c = blockIdx.x / a.S, s = blockIdx.x - c * a.S;            \
  const int u0 = s * a.per, u1 = min(a.U, u0 + a.per)

// the nine taps in their one order
__device__ __forceinline__ float dw_conv9(const float (&w)[9], const float (&v)[9]) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) acc = fmaf(w[k], v[k], acc);
  return acc;
}

__device__ __forceinline__ float dw_clamp6(float o) {
  o = o < 0.f ? 0.f : o;                                                          // a NaN stays
  return o > 6.f ? 6.f : o;
}

// z[0, c, 0, 0] before rounding, from global memory
template <typename T, int STRIDE>
__device__ __forceinline__ float dw_first(const DwArgs& a, int c, const float (&w)[9]) {
  const T* __restrict__ xp = (const T*)a.x + (int64_t)c * a.H * a.W;
  float v[9];
#pragma unroll
  for (int ka = 0; ka < 3; ++ka)
#pragma unroll
    for (int kb = 0; kb < 3; ++kb) {
      const int h = ka - 1, ww = kb - 1;
      v[ka * 3 + kb] = (h >= 0 && h < a.H && ww >= 0 && ww < a.W) ? bn_widen(xp[h * a.W + ww]) : 0.f;
    }
  return dw_conv9(w, v);
}

// input rows [r0, r0 + rin) of the unit's images with one zero column on either side: xs[(g rin + r) (W + 2) + 1 + col]
template <typename T, int VEC>
__device__ __forceinline__ void dw_stage_x(const DwArgs& a, const DwUnit& q, int c, int r0, int rin, float* xs) {
  const int P = a.W + 2, R = q.gn * rin, wp = a.W / VEC;
  for (int rr = threadIdx.x; rr < R; rr += 256) {
    xs[rr * P] = 0.f;
    xs[rr * P + a.W + 1] = 0.f;
  }
  for (int idx = threadIdx.x; idx < R * wp; idx += 256) {
    const int rr = idx / wp, k = idx - rr * wp;
    const int g = rr / rin, h = r0 + (rr - g * rin);
    float v[VEC];
    if (h >= 0 && h < a.H) {
      bn_load<T, VEC>((const T*)a.x + (((int64_t)(q.n0 + g) * a.C + c) * a.H + h) * a.W + k * VEC, v);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) v[j] = 0.f;
    }
    float* __restrict__ d = xs + rr * P + 1 + k * VEC;
#pragma unroll
    for (int j = 0; j < VEC; ++j) d[j] = v[j];
  }
}

// both sums of the workgroup on thread 0: lanes by the butterfly, then waves 1 .. 3 in that order
__device__ __forceinline__ void dw_block_sum2(double& u, double& v) {
  __shared__ double red[3][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u = bn_wave_sum(u);
  v = bn_wave_sum(v);
  if (wave > 0 && lane == 0) { red[wave - 1][0] = u; red[wave - 1][1] = v; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w) { u += red[w][0]; v += red[w][1]; }
  }
}

// the channel's S partials added in one fixed order, the same value on every lane
__device__ __forceinline__ void dw_combine(const DwArgs& a, int c, double& u, double& v) {
  const int lane = threadIdx.x & 63;
  const double* __restrict__ p = a.part + (int64_t)c * a.S * 2;
  u = v = 0.0;
  if (lane < a.S) { u = p[2 * lane]; v = p[2 * lane + 1]; }
  if (lane + 64 < a.S) { u += p[2 * (lane + 64)]; v += p[2 * (lane + 64) + 1]; }
  u = bn_wave_sum(u);
  v = bn_wave_sum(v);
}

template <typename T, int VEC, int STRIDE, bool EVAL>
__global__ __launch_bounds__(256) void dwbn_conv_kernel(const DwArgs a) {
  __shared__ float xs[kDwTile];
  DW_OWN();
  float w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = a.w[c * 9 + k];
  float ea = 0.f, eb = 0.f;
  double K = 0.0;
  if constexpr (EVAL) {
    const double ad = (double)a.gamma[c] / sqrt((double)a.rvar[c] + a.eps);
    ea = (float)ad;
    eb = (float)((double)a.beta[c] - (double)a.rmean[c] * ad);
  } else {
    K = (double)bn_widen(bn_narrow<T>(dw_first<T, STRIDE>(a, c, w)));
  }
  const int P = a.W + 2, wpo = a.Wo / VEC, HoWo = a.Ho * a.Wo;
  T* __restrict__ out = EVAL ? (T*)a.y : (T*)a.z;
  double s1 = 0.0, s2 = 0.0;
  for (int u = u0; u < u1; ++u) {
    const DwUnit q = dw_unit(a, u);
    const int rin = (q.rows - 1) * STRIDE + 3;
    dw_stage_x<T, VEC>(a, q, c, q.i0 * STRIDE - 1, rin, xs);
    __syncthreads();
    const int total = q.gn * q.rows * wpo;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
      const int rr = idx / wpo, k = idx - rr * wpo;
      const int g = rr / q.rows, i = rr - g * q.rows;
      const float* __restrict__ t = xs + (g * rin + i * STRIDE) * P + k * VEC * STRIDE;
      float o[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float v[9];
#pragma unroll
        for (int ka = 0; ka < 3; ++ka)
#pragma unroll
          for (int kb = 0; kb < 3; ++kb) v[ka * 3 + kb] = t[ka * P + j * STRIDE + kb];
        o[j] = dw_conv9(w, v);
        if constexpr (EVAL) {
          o[j] = dw_clamp6(fmaf(ea, o[j], eb));
        } else {
          const double d = (double)bn_widen(bn_narrow<T>(o[j])) - K;
          s1 += d;
          s2 = fma(d, d, s2);
        }
      }
      bn_store<T, VEC>(out + ((int64_t)(q.n0 + g) * a.C + c) * HoWo + (q.i0 + i) * a.Wo + k * VEC, o);
    }
    __syncthreads();
  }
  if constexpr (!EVAL) {
    dw_block_sum2(s1, s2);
    if (threadIdx.x == 0) {
      a.part[(int64_t)blockIdx.x * 2] = s1;
      a.part[(int64_t)blockIdx.x * 2 + 1] = s2;
    }
  }
}

// the contiguous run of a unit's outputs in image g: rows [i0, i0 + rows) of plane (n0 + g, c), pack by pack at `at`
#define DW_PACKS_BEGIN                                                                                  \
  for (int u = u0; u < u1; ++u) {                                                                       \
    const DwUnit q = dw_unit(a, u);                                                                     \
    const int ppi = q.rows * a.Wo / VEC, total = q.gn * ppi;                                            \
    for (int idx = threadIdx.x; idx < total; idx += 256) {                                              \
      const int g = idx / ppi, r = idx - g * ppi;                                                       \
      const int64_t at = ((int64_t)(q.n0 + g) * a.C + c) * HoWo + q.i0 * a.Wo + r * VEC;
#define DW_PACKS_END                                                                                    \
    }                                                                                                   \
  }

template <typename T, int VEC>
__global__ __launch_bounds__(256) void dwbn_apply_kernel(const DwArgs a) {
  DW_OWN();
  const int HoWo = a.Ho * a.Wo;
  const float gam = a.gamma[c], bet = a.beta[c];
  const double K = (double)bn_widen(((const T*)a.z)[(int64_t)c * HoWo]);
  double s1, s2;
  dw_combine(a, c, s1, s2);
  const double dm = (double)a.M;
  const double mean = K + s1 / dm;
  const double var = fmax((s2 - s1 * s1 / dm) / dm, 0.0);
  const double rstd = 1.0 / sqrt(var + a.eps);
  if (s == 0 && threadIdx.x == 0) {
    if (a.stats) { a.stats[2 * c] = (float)mean; a.stats[2 * c + 1] = (float)rstd; }
    if (a.rmean) {
      a.rmean[c] = (float)((1.0 - a.momentum) * (double)a.rmean[c] + a.momentum * mean);
      a.rvar[c] = (float)((1.0 - a.momentum) * (double)a.rvar[c] + a.momentum * (var * dm / (dm - 1.0)));
    }
    if (a.nbt && c == 0) *a.nbt += 1;
  }
  DW_PACKS_BEGIN
    float v[VEC], o[VEC];
    bn_load<T, VEC>((const T*)a.z + at, v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = dw_clamp6(fmaf(gam, (float)(((double)v[j] - mean) * rstd), bet));
    bn_store<T, VEC>((T*)a.y + at, o);
  DW_PACKS_END
}

// gz of VEC values: the upstream gradient where the stored output is strictly inside (0, 6)
template <typename T, int VEC>
__device__ __forceinline__ void dw_load_gz(const T* __restrict__ gp, const T* __restrict__ yp, float (&gz)[VEC]) {
  float yv[VEC];
  bn_load<T, VEC>(gp, gz);
  bn_load<T, VEC>(yp, yv);
#pragma unroll
  for (int j = 0; j < VEC; ++j) gz[j] = (yv[j] > 0.f && yv[j] < 6.f) ? gz[j] : 0.f;
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void dwbn_bwd_sum_kernel(const DwArgs a) {
  DW_OWN();
  const int HoWo = a.Ho * a.Wo;
  const float mean = a.stats[2 * c], rstd = a.stats[2 * c + 1];
  double sg = 0.0, sgx = 0.0;
  DW_PACKS_BEGIN
    float gz[VEC], v[VEC];
    dw_load_gz<T, VEC>((const T*)a.g + at, (const T*)a.y + at, gz);
    bn_load<T, VEC>((const T*)a.z + at, v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      sg += (double)gz[j];
      sgx = fma((double)gz[j], (double)bn_xhat(v[j], mean, rstd), sgx);
    }
  DW_PACKS_END
  dw_block_sum2(sg, sgx);
  if (threadIdx.x == 0) {
    a.part[(int64_t)blockIdx.x * 2] = sg;
    a.part[(int64_t)blockIdx.x * 2 + 1] = sgx;
  }
}

template <typename T, int VEC, int STRIDE>
__global__ __launch_bounds__(256) void dwbn_bwd_dx_kernel(const DwArgs a) {
  __shared__ float xs[kDwTile];
  __shared__ float ds[kDwTile];
  __shared__ double wred[3][9];
  DW_OWN();
  if (!a.dx && !a.dw && s != 0) return;
  double sg, sgx;
  dw_combine(a, c, sg, sgx);
  if (s == 0 && threadIdx.x == 0) {
    if (a.dbeta) a.dbeta[c] = (float)sg;
    if (a.dgamma) a.dgamma[c] = (float)sgx;
  }
  if (!a.dx && !a.dw) return;
  const int HoWo = a.Ho * a.Wo, P = a.W + 2, Q = a.Wo + 2, wpo = a.Wo / VEC, wpi = a.W / VEC;
  const float mean = a.stats[2 * c], rstd = a.stats[2 * c + 1];
  const float k1 = (float)(sg / (double)a.M), k2 = (float)(sgx / (double)a.M), gr = a.gamma[c] * rstd;
  float w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = a.w[c * 9 + k];
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  for (int u = u0; u < u1; ++u) {
    const DwUnit q = dw_unit(a, u);
    const int rin = (q.rows - 1) * STRIDE + 3, rd = q.rows + 2;
    if (a.dw) dw_stage_x<T, VEC>(a, q, c, q.i0 * STRIDE - 1, rin, xs);
    // dz over output rows [i0 - 1, i0 + rows] and columns [-1, Wo]: ds[(g rd + r) Q + 1 + j], zero outside the plane
    const int R = q.gn * rd;
    for (int rr = threadIdx.x; rr < R; rr += 256) {
      ds[rr * Q] = 0.f;
      ds[rr * Q + a.Wo + 1] = 0.f;
    }
    for (int idx = threadIdx.x; idx < R * wpo; idx += 256) {
      const int rr = idx / wpo, k = idx - rr * wpo;
      const int g = rr / rd, i = q.i0 - 1 + (rr - g * rd);
      float o[VEC];
      if (i >= 0 && i < a.Ho) {
        const int64_t at = ((int64_t)(q.n0 + g) * a.C + c) * HoWo + i * a.Wo + k * VEC;
        float gz[VEC], v[VEC];
        dw_load_gz<T, VEC>((const T*)a.g + at, (const T*)a.y + at, gz);
        bn_load<T, VEC>((const T*)a.z + at, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = gr * ((gz[j] - k1) - bn_xhat(v[j], mean, rstd) * k2);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = 0.f;
      }
      float* __restrict__ d = ds + rr * Q + 1 + k * VEC;
#pragma unroll
      for (int j = 0; j < VEC; ++j) d[j] = o[j];
    }
    __syncthreads();
    if (a.dx) {
      // the band's input rows: [i0 s, (i0 + rows) s), the last band up to H
      const int h0 = q.i0 * STRIDE, h1 = (q.i0 + q.rows == a.Ho) ? a.H : (q.i0 + q.rows) * STRIDE;
      const int hr = h1 - h0, total = q.gn * hr * wpi;
      for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int rr = idx / wpi, k = idx - rr * wpi;
        const int g = rr / hr, h = h0 + (rr - g * hr);
        const float* __restrict__ t = ds + g * rd * Q;
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const int col = k * VEC + j;
          float sum = 0.f;
#pragma unroll
          for (int ka = 0; ka < 3; ++ka) {
            const int ti = h + 1 - ka;                     // i s: the output row this tap came from, times s
            if (STRIDE == 2 && (ti & 1)) continue;
            const int tr = ti / STRIDE - q.i0 + 1;         // ti = -1 (s = 1) is the zero row above the plane
#pragma unroll
            for (int kb = 0; kb < 3; ++kb) {
              const int tj = col + 1 - kb;
              if (STRIDE == 2 && (tj & 1)) continue;
              sum = fmaf(w[ka * 3 + kb], t[tr * Q + tj / STRIDE + 1], sum);
            }
          }
          o[j] = sum;
        }
        bn_store<T, VEC>((T*)a.dx + (((int64_t)(q.n0 + g) * a.C + c) * a.H + h) * a.W + k * VEC, o);
      }
    }
    if (a.dw) {
      const int total = q.gn * q.rows * a.Wo;
      for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int rr = idx / a.Wo, j = idx - rr * a.Wo;
        const int g = rr / q.rows, i = rr - g * q.rows;
        const double d = (double)ds[(g * rd + i + 1) * Q + j + 1];
        const float* __restrict__ t = xs + (g * rin + i * STRIDE) * P + j * STRIDE;
#pragma unroll
        for (int ka = 0; ka < 3; ++ka)
#pragma unroll
          for (int kb = 0; kb < 3; ++kb) acc[ka * 3 + kb] = fma(d, (double)t[ka * P + kb], acc[ka * 3 + kb]);
      }
    }
    __syncthreads();
  }
  if (!a.dw) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = bn_wave_sum(acc[k]);
  if (wave > 0 && lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) wred[wave - 1][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      double v = acc[k];
#pragma unroll
      for (int ww = 0; ww < 3; ++ww) v += wred[ww][k];
      a.wpart[(int64_t)blockIdx.x * 9 + k] = v;
    }
  }
}

#undef DW_PACKS_BEGIN
#undef DW_PACKS_END
#undef DW_OWN

// dw[c, k]: the channel's S partials in ascending order
__global__ __launch_bounds__(256) void dwbn_dw_kernel(const DwArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.C * 9) return;
  const int c = i / 9, k = i - c * 9;
  const double* __restrict__ p = a.wpart + (int64_t)c * a.S * 9 + k;
  double v = 0.0;
  for (int s = 0; s < a.S; ++s) v += p[s * 9];
  a.dw[i] = (float)v;
}

}  // namespace tadmm

using namespace tadmm;

namespace {

struct DwPlan { int G, RB, NB, U, S, per, cap; };

inline int dw_out(int n, int s) { return (n - 1) / s + 1; }
inline int64_t dw_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

// splits the workspace is sized for: from C alone, so the size cannot fall as N or the plane grows
inline int dw_cap(int C) { return (int)std::min<int64_t>(kDwMaxSplit, std::max<int64_t>(1, dw_ceil(kDwTarget, C))); }

// the ownership, from the shape alone (W <= kDwMaxW): bands of RB output rows so that the haloed input rows and the
// haloed dz rows each fit kDwTile floats, shorter (not below 4 rows) while N NB stays under the workgroups wanted per
// channel; whole planes G to a tile, at most kDwTileOut outputs; U units in S splits of `per`, none empty
DwPlan dw_plan(int N, int C, int H, int W, int s) {
  const int Ho = dw_out(H, s), Wo = dw_out(W, s);
  const int r1 = (kDwTile / (W + 2) - 3) / s + 1, r2 = kDwTile / (Wo + 2) - 2;
  const int rbmax = std::min(Ho, std::min(r1, r2));
  const int64_t want = std::max<int64_t>(1, dw_ceil(kDwTarget, C));
  const int64_t nbw = dw_ceil(want, N);
  const int rb = (int)std::max<int64_t>(dw_ceil(Ho, nbw), 4);
  DwPlan p;
  p.RB = std::min(rbmax, rb);
  p.NB = (int)dw_ceil(Ho, p.RB);
  p.G = 1;
  if (p.NB == 1) {
    const int64_t gl = std::min<int64_t>(kDwTile / ((int64_t)((Ho - 1) * s + 3) * (W + 2)),
                                         kDwTile / ((int64_t)(Ho + 2) * (Wo + 2)));
    const int64_t go = std::max<int64_t>(1, kDwTileOut / ((int64_t)Ho * Wo));
    const int64_t gp = std::max<int64_t>(1, N / want);
    p.G = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(N, gl), std::min(go, gp)));
  }
  const int64_t U = dw_ceil(N, p.G) * p.NB;
  p.U = (int)U;
  p.cap = dw_cap(C);
  const int64_t ns = std::min<int64_t>(U, p.cap);
  p.per = (int)dw_ceil(U, ns);
  p.S = (int)dw_ceil(U, p.per);
  return p;
}

size_t dw_ws_bytes(int C) { return align_up((size_t)C * dw_cap(C) * 11 * sizeof(double), 256); }

inline bool dw_dtype_ok(int dt) { return dt == TADMM_CHAIN_F32 || dt == TADMM_CHAIN_BF16 || dt == TADMM_CHAIN_F16; }
inline bool dw_shape_ok(const tadmm_dwbn_desc* d) {
  return d->N >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1 && (d->stride == 1 || d->stride == 2);
}
inline bool dw_shape_fits(const tadmm_dwbn_desc* d) {
  return d->W <= kDwMaxW && (int64_t)d->N * d->H * d->W <= kDwMaxM;
}

enum DwKernel { DW_CONV, DW_EVAL, DW_APPLY, DW_BWD_SUM, DW_BWD_DX };

template <typename T>
void dw_launch(const DwArgs& a, DwKernel k, bool wide, int stride, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr bool kBwd = !std::is_same<T, bn_f16>::value;        // float16 is forward only (dw_check refuses it)
  const dim3 grid((unsigned)((int64_t)a.C * a.S)), block(256);
#define DW_GO(VV, SS)                                                                                       \
  switch (k) {                                                                                              \
    case DW_CONV: hipLaunchKernelGGL((dwbn_conv_kernel<T, VV, SS, false>), grid, block, 0, s, a); break;    \
    case DW_EVAL: hipLaunchKernelGGL((dwbn_conv_kernel<T, VV, SS, true>), grid, block, 0, s, a); break;     \
    case DW_APPLY: hipLaunchKernelGGL((dwbn_apply_kernel<T, VV>), grid, block, 0, s, a); break;             \
    case DW_BWD_SUM:                                                                                        \
      if constexpr (kBwd) hipLaunchKernelGGL((dwbn_bwd_sum_kernel<T, VV>), grid, block, 0, s, a);           \
      break;                                                                                                \
    case DW_BWD_DX:                                                                                         \
      if constexpr (kBwd) hipLaunchKernelGGL((dwbn_bwd_dx_kernel<T, VV, SS>), grid, block, 0, s, a);        \
      break;                                                                                                \
  }
  if (wide) {
    if (stride == 1) DW_GO(V, 1) else DW_GO(V, 2)
  } else {
    if (stride == 1) DW_GO(1, 1) else DW_GO(1, 2)
  }
#undef DW_GO
}

void dw_launch_any(const tadmm_dwbn_desc* d, const DwArgs& a, DwKernel k, bool wide, hipStream_t s) {
  if (d->dtype == TADMM_CHAIN_F32) dw_launch<float>(a, k, wide, d->stride, s);
  else if (d->dtype == TADMM_CHAIN_BF16) dw_launch<bn_bf16>(a, k, wide, d->stride, s);
  else dw_launch<bn_f16>(a, k, wide, d->stride, s);
}

inline bool dw_mis(const void* p, size_t n) { return ((uintptr_t)p) % n != 0; }

// what the two entries share: TADMM_OK with *wide and the arguments set, or the refusal
int dw_check(tadmm_ctx_s* h, const tadmm_dwbn_desc* d, bool bwd, bool* wide, DwArgs* out) {
  if (!d) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: the descriptor is NULL");
  if (d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1)
    CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: N, C, H, W >= 1 are required (got %d, %d, %d, %d)", d->N, d->C, d->H, d->W);
  if (d->stride != 1 && d->stride != 2) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: stride is 1 or 2 (got %d)", d->stride);
  if (!dw_dtype_ok(d->dtype)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: unknown element type %d", d->dtype);
  if (bwd && d->dtype == TADMM_CHAIN_F16) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: float16 is forward only");
  const bool training = bwd || d->training != 0;
  const int Ho = dw_out(d->H, d->stride), Wo = dw_out(d->W, d->stride);
  const int64_t M = (int64_t)d->N * Ho * Wo;
  if (training && M < 2)
    CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: training needs more than one output value per channel (M = %lld)", (long long)M);
  if (!(d->eps >= 0.0) || !(d->eps < INFINITY)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: eps %g must be finite and >= 0", d->eps);
  if (!(d->momentum >= 0.0 && d->momentum <= 1.0))
    CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: momentum %g outside [0, 1]", d->momentum);
  const size_t es = d->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  const size_t V = 16 / es;
  if (!d->x || dw_mis(d->x, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: x is NULL or misaligned");
  if (!d->w || dw_mis(d->w, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: w is NULL or misaligned");
  if (!d->gamma || dw_mis(d->gamma, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: gamma is NULL or misaligned");
  if (dw_mis(d->stats, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: stats is misaligned");
  if (training && (!d->z || dw_mis(d->z, es))) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: z is NULL or misaligned in training mode");
  if (!d->y || dw_mis(d->y, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: y is NULL or misaligned");
  bool w = !dw_mis(d->x, 16) && !dw_mis(d->y, 16) && (size_t)d->W % V == 0 && (size_t)Wo % V == 0;
  if (training) w = w && !dw_mis(d->z, 16);
  if (!bwd) {
    if (!d->beta || dw_mis(d->beta, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: beta is NULL or misaligned");
    if (d->y == d->x || (training && (d->z == d->x || d->z == d->y)))
      CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: y, z and x must be three buffers");
    if (dw_mis(d->running_mean, 4) || dw_mis(d->running_var, 4))
      CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: the running statistics are misaligned");
    if (!training && (!d->running_mean || !d->running_var))
      CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: eval mode reads running_mean and running_var, one is NULL");
    if ((d->running_mean == nullptr) != (d->running_var == nullptr))
      CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: running_mean and running_var are given together or not at all");
    if (dw_mis(d->num_batches_tracked, 8)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: num_batches_tracked is misaligned");
  } else {
    if (!d->stats) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: stats is NULL and the backward reads it");
    if (!d->g || dw_mis(d->g, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: g is NULL or misaligned");
    if (dw_mis(d->dx, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: dx is not aligned to its element");
    if (d->dx && (d->dx == d->x || d->dx == d->g || d->dx == d->y || d->dx == d->z))
      CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: dx is one buffer with x, g, y or z");
    if (dw_mis(d->dw, 4) || dw_mis(d->dgamma, 4) || dw_mis(d->dbeta, 4))
      CTX_FAIL(h, TADMM_ERR_INVALID, "dwbn: dw / dgamma / dbeta are misaligned");
    w = w && !dw_mis(d->g, 16) && !dw_mis(d->dx, 16);
  }
  if (!dw_shape_fits(d))
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "dwbn: W = %d, N H W = %lld; the launch takes W <= %d and N H W <= %lld", d->W,
             (long long)((int64_t)d->N * d->H * d->W), kDwMaxW, (long long)kDwMaxM);
  const bool need_ws = bwd ? (d->dx || d->dw || d->dgamma || d->dbeta) : training;
  if (need_ws) {
    const size_t need = dw_ws_bytes(d->C);
    if (!d->workspace || dw_mis(d->workspace, 16) || d->workspace_bytes < need)
      CTX_FAIL(h, TADMM_ERR_WORKSPACE, "dwbn workspace too small or misaligned: need %zu bytes, got %zu", need,
               d->workspace_bytes);
  }
  const DwPlan plan = dw_plan(d->N, d->C, d->H, d->W, d->stride);
  DwArgs a{};
  a.x = d->x; a.w = d->w; a.gamma = d->gamma; a.beta = d->beta;
  a.rmean = d->running_mean; a.rvar = d->running_var; a.nbt = d->num_batches_tracked;
  a.z = d->z; a.y = d->y; a.stats = d->stats;
  a.g = d->g; a.dx = d->dx; a.dw = d->dw; a.dgamma = d->dgamma; a.dbeta = d->dbeta;
  a.part = need_ws ? (double*)d->workspace : nullptr;
  a.wpart = need_ws ? (double*)d->workspace + (size_t)d->C * plan.cap * 2 : nullptr;
  a.eps = d->eps; a.momentum = d->momentum;
  a.N = d->N; a.C = d->C; a.H = d->H; a.W = d->W; a.Ho = Ho; a.Wo = Wo; a.M = (int32_t)M;
  a.G = plan.G; a.RB = plan.RB; a.NB = plan.NB; a.U = plan.U; a.S = plan.S; a.per = plan.per;
  *wide = w;
  *out = a;
  return TADMM_OK;
}

}  // namespace

extern "C" {

int tadmm_dwbn_desc_bytes(void) { return (int)sizeof(tadmm_dwbn_desc); }

int tadmm_dwbn_fits(const tadmm_dwbn_desc* d, int32_t* max_w) {
  if (max_w) *max_w = kDwMaxW;
  if (!d || !dw_shape_ok(d)) return TADMM_ERR_INVALID;
  return dw_shape_fits(d) ? 1 : 0;
}

int tadmm_dwbn_plan(const tadmm_dwbn_desc* d, int32_t* plan6) {
  if (!d || !plan6 || !dw_shape_ok(d)) return TADMM_ERR_INVALID;
  if (!dw_shape_fits(d)) return TADMM_ERR_UNSUPPORTED;
  const DwPlan p = dw_plan(d->N, d->C, d->H, d->W, d->stride);
  plan6[0] = p.G; plan6[1] = p.RB; plan6[2] = p.NB; plan6[3] = p.U; plan6[4] = p.S; plan6[5] = p.per;
  return TADMM_OK;
}

int tadmm_dwbn_workspace_bytes(const tadmm_dwbn_desc* d, size_t* bytes) {
  if (!d || !bytes || !dw_shape_ok(d) || !dw_dtype_ok(d->dtype)) return TADMM_ERR_INVALID;
  if (!dw_shape_fits(d)) return TADMM_ERR_UNSUPPORTED;
  *bytes = dw_ws_bytes(d->C);
  return TADMM_OK;
}

int tadmm_dwbn_fwd(tadmm_handle h, const tadmm_dwbn_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  DwArgs a;
  const int rc = dw_check(h, d, false, &wide, &a);
  if (rc != TADMM_OK) return rc;
  DeviceGuard device_guard(h);
  hipStream_t s = (hipStream_t)stream_;
  if (d->training) {
    dw_launch_any(d, a, DW_CONV, wide, s);
    dw_launch_any(d, a, DW_APPLY, wide, s);
  } else {
    dw_launch_any(d, a, DW_EVAL, wide, s);
  }
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_dwbn_bwd(tadmm_handle h, const tadmm_dwbn_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  DwArgs a;
  const int rc = dw_check(h, d, true, &wide, &a);
  if (rc != TADMM_OK) return rc;
  if (!a.part) return TADMM_OK;                             // nothing is wanted
  DeviceGuard device_guard(h);
  hipStream_t s = (hipStream_t)stream_;
  dw_launch_any(d, a, DW_BWD_SUM, wide, s);
  dw_launch_any(d, a, DW_BWD_DX, wide, s);
  if (a.dw) hipLaunchKernelGGL(dwbn_dw_kernel, dim3((unsigned)((a.C * 9 + 255) / 256)), dim3(256), 0, s, a);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
