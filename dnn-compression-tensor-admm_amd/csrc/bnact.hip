// The tail of a ResNet block (resnet_cifar_tt.py: TTBasicBlock, resnet_inet_tt.py: TTBasicBlock / TTBottleneck):
// BatchNorm2d of the convolution's output, the shortcut added, ReLU -- relu(bn(conv(x))) and relu(bn(conv(x)) + shortcut).
// x is (N, C, H, W), NCHW contiguous; a channel's M = N H W values lie in N planes of HW elements.
//
//     mean_c = sum x / M,  var_c = sum (x - mean_c)^2 / M (biased),  rstd_c = 1 / sqrt(var_c + eps)        (training)
//     z      = gamma_c (x - mean_c) rstd_c + beta_c + [c0 <= c < c0 + Cr] res[n, c - c0, h, w]
//     y      = relu ? max(z, 0) : z
//
// res is read through four element strides: a plain tensor, or the option-A shortcut x_in[:, :, ::2, ::2] placed at
// channel offset c0 = planes / 4 (the zero padding of F.pad is the channels outside the window, which read nothing).
//
// Ownership.  A channel's values are numbered m = n HW + p and cut into S splits of `span` consecutive values, span a
// multiple of the trip 256 * (16 / sizeof(T)); workgroup (c, s) = blockIdx.x owns split s of channel c and walks it in
// trips of 256 * VEC values, lane t at m0 + trip * 256 * VEC + t * VEC, keeping (n, p) by addition (one division per
// lane and launch).  S comes from the shape alone (ba_plan): enough splits for about 2048 workgroups, at most 128, never
// more than there are trips -- C = 16 with M = 131072 gets 128 splits of one trip, C = 2048 with M = 98 one split.
//
//   1. bnact_stat_kernel<T, VEC>         sum (x - K) and sum (x - K)^2 in double with K = x[0, c, 0, 0], the shift all
//                                        splits of a channel share: the sums add across splits and a channel with
//                                        mean >> std keeps its variance (the differences are of the size of std).
//   2. bnact_apply_kernel<T, VEC, EVAL>  training: every workgroup adds its channel's S partials in one fixed order (two
//                                        per lane, then the butterfly of bn_wave_sum), so all splits of a channel hold
//                                        the same mean and rstd in double; y from them; split 0 writes stats (rounded
//                                        once), the running statistics (momentum, unbiased variance M / (M - 1)) and,
//                                        for channel 0, the batch counter.  Eval: a = gamma / sqrt(running_var + eps),
//                                        b = beta - running_mean a, y = act(a x + b + res); the one launch.
//   3. bnact_bwd_sum_kernel<T, VEC>      gz = g (y > 0) from y as stored; sum gz and sum gz xhat in double, xhat from
//                                        stats with the expression of the row norms (bn_xhat); dres = gz over the window.
//   4. bnact_bwd_dx_kernel<T, VEC>       the partials added as in 2; split 0 writes dgamma and dbeta;
//                                        dx = gamma rstd (gz - dbeta / M - xhat dgamma / M).  Without dx only split 0 works.
// No atomics; grids depend on (N, C, HW, dtype) alone: bitwise reproducible.  Accesses: VEC elements = 16 bytes when
// every contiguous base is 16-byte aligned and HW is a whole number of 16-byte units; one element otherwise.  The
// residual is loaded 16 bytes wide where it is plane-contiguous and aligned, else by element.
#include "rownorm_common.h"

namespace tadmm {

constexpr int kBaTarget = 2048;              // workgroups the split aims at
constexpr int kBaMaxSplit = 128;             // two partials per lane in the fixed-order sum
constexpr int64_t kBaMaxM = (int64_t(1) << 31) - 4096;

struct BaArgs {
  const void* x; const void* res;
  int64_t rs0, rs1, rs2, rs3;
  const float* gamma; const float* beta;
  float* rmean; float* rvar; int64_t* nbt;
  void* y; float* stats;
  const void* g; void* dx; void* dres; float* dgamma; float* dbeta;
  double* part;
  double eps, momentum;
  int32_t C, HW, W, c0, Cr, M, S, span;
  int32_t relu, res_wide, res_lin;
  int32_t step_q, step_r;                    // (256 * VEC) / HW and % HW: one trip in (n, p)
};

struct BaPos { int n, p; };

__device__ __forceinline__ void ba_next(BaPos& q, const BaArgs& a) {
  q.p += a.step_r;
  q.n += a.step_q;
  if (q.p >= a.HW) { q.p -= a.HW; ++q.n; }
}

// the residual of VEC values of plane (n, window channel cc) from p on
template <typename T, int VEC>
__device__ __forceinline__ void ba_load_res(const BaArgs& a, int n, int cc, int p, float (&r)[VEC]) {
  const T* __restrict__ base = (const T*)a.res + n * a.rs0 + cc * a.rs1;
  if (VEC > 1 && a.res_wide) {
    bn_load<T, VEC>(base + p, r);
    return;
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int pj = p + j;
    int64_t off;
    if (a.res_lin) {
      off = pj * a.rs3;
    } else {
      const int h = pj / a.W;
      off = h * a.rs2 + (pj - h * a.W) * a.rs3;
    }
    r[j] = bn_widen(base[off]);
  }
}

// both sums of the workgroup on thread 0: lanes by the butterfly, then waves 1 .. 3 in that order
__device__ __forceinline__ void ba_block_sum2(double& u, double& v) {
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
__device__ __forceinline__ void ba_combine(const BaArgs& a, int c, double& u, double& v) {
  const int lane = threadIdx.x & 63;
  const double* __restrict__ p = a.part + (int64_t)c * a.S * 2;
  u = v = 0.0;
  if (lane < a.S) { u = p[2 * lane]; v = p[2 * lane + 1]; }
  if (lane + 64 < a.S) { u += p[2 * (lane + 64)]; v += p[2 * (lane + 64) + 1]; }
  u = bn_wave_sum(u);
  v = bn_wave_sum(v);
}

#define BA_OWN()                                                       \
  const int c = blockIdx.x / a.S, s = blockIdx.x - c * a.S;            \
  const int m1 = min(a.M, (s + 1) * a.span);                           \
  int m = s * a.span + (int)threadIdx.x * VEC;                         \
  BaPos q;                                                             \
  q.n = m / a.HW;                                                      \
  q.p = m - q.n * a.HW
#define BA_AT(ptr) ((ptr) + ((int64_t)q.n * a.C + c) * a.HW + q.p)

template <typename T, int VEC>
__global__ __launch_bounds__(256) void bnact_stat_kernel(const BaArgs a) {
  BA_OWN();
  const double K = (double)bn_widen(((const T*)a.x)[(int64_t)c * a.HW]);
  double s1 = 0.0, s2 = 0.0;
  for (; m < m1; m += 256 * VEC, ba_next(q, a)) {
    float v[VEC];
    bn_load<T, VEC>(BA_AT((const T*)a.x), v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const double d = (double)v[j] - K;
      s1 += d;
      s2 = fma(d, d, s2);
    }
  }
  ba_block_sum2(s1, s2);
  if (threadIdx.x == 0) {
    a.part[(int64_t)blockIdx.x * 2] = s1;
    a.part[(int64_t)blockIdx.x * 2 + 1] = s2;
  }
}

template <typename T, int VEC, bool EVAL>
__global__ __launch_bounds__(256) void bnact_apply_kernel(const BaArgs a) {
  BA_OWN();
  const float gam = a.gamma[c], bet = a.beta[c];
  double mean = 0.0, rstd = 0.0;
  float ea = 0.f, eb = 0.f;
  if constexpr (EVAL) {
    const double ad = (double)gam / sqrt((double)a.rvar[c] + a.eps);
    ea = (float)ad;
    eb = (float)((double)bet - (double)a.rmean[c] * ad);
  } else {
    const double K = (double)bn_widen(((const T*)a.x)[(int64_t)c * a.HW]);
    double s1, s2;
    ba_combine(a, c, s1, s2);
    const double dm = (double)a.M;
    mean = K + s1 / dm;
    const double var = fmax((s2 - s1 * s1 / dm) / dm, 0.0);
    rstd = 1.0 / sqrt(var + a.eps);
    if (s == 0 && threadIdx.x == 0) {
      if (a.stats) { a.stats[2 * c] = (float)mean; a.stats[2 * c + 1] = (float)rstd; }
      if (a.rmean) {
        a.rmean[c] = (float)((1.0 - a.momentum) * (double)a.rmean[c] + a.momentum * mean);
        a.rvar[c] = (float)((1.0 - a.momentum) * (double)a.rvar[c] + a.momentum * (var * dm / (dm - 1.0)));
      }
      if (a.nbt && c == 0) *a.nbt += 1;
    }
  }
  const int cc = c - a.c0;
  const bool with_res = a.res && cc >= 0 && cc < a.Cr;
  for (; m < m1; m += 256 * VEC, ba_next(q, a)) {
    float v[VEC], o[VEC];
    bn_load<T, VEC>(BA_AT((const T*)a.x), v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if constexpr (EVAL) o[j] = fmaf(ea, v[j], eb);
      else o[j] = fmaf(gam, (float)(((double)v[j] - mean) * rstd), bet);
    }
    if (with_res) {
      float r[VEC];
      ba_load_res<T, VEC>(a, q.n, cc, q.p, r);
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] += r[j];
    }
    if (a.relu) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = o[j] < 0.f ? 0.f : o[j];             // a NaN stays
    }
    bn_store<T, VEC>(BA_AT((T*)a.y), o);
  }
}

// gz of VEC values: the upstream gradient where the stored output is positive
template <typename T, int VEC>
__device__ __forceinline__ void ba_load_gz(const BaArgs& a, const T* __restrict__ gp, const T* __restrict__ yp,
                                           float (&gz)[VEC]) {
  bn_load<T, VEC>(gp, gz);
  if (a.relu) {
    float yv[VEC];
    bn_load<T, VEC>(yp, yv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) gz[j] = yv[j] > 0.f ? gz[j] : 0.f;
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void bnact_bwd_sum_kernel(const BaArgs a) {
  BA_OWN();
  const float mean = a.stats[2 * c], rstd = a.stats[2 * c + 1];
  const int cc = c - a.c0;
  const bool with_dres = a.dres && cc >= 0 && cc < a.Cr;
  if (!a.part && !with_dres) return;
  double sg = 0.0, sgx = 0.0;
  for (; m < m1; m += 256 * VEC, ba_next(q, a)) {
    float gz[VEC], v[VEC];
    ba_load_gz<T, VEC>(a, BA_AT((const T*)a.g), BA_AT((const T*)a.y), gz);
    if (with_dres) bn_store<T, VEC>((T*)a.dres + ((int64_t)q.n * a.Cr + cc) * a.HW + q.p, gz);
    if (a.part) {
      bn_load<T, VEC>(BA_AT((const T*)a.x), v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        sg += (double)gz[j];
        sgx = fma((double)gz[j], (double)bn_xhat(v[j], mean, rstd), sgx);
      }
    }
  }
  if (!a.part) return;
  ba_block_sum2(sg, sgx);
  if (threadIdx.x == 0) {
    a.part[(int64_t)blockIdx.x * 2] = sg;
    a.part[(int64_t)blockIdx.x * 2 + 1] = sgx;
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void bnact_bwd_dx_kernel(const BaArgs a) {
  BA_OWN();
  if (!a.dx && s != 0) return;
  double sg, sgx;
  ba_combine(a, c, sg, sgx);
  if (s == 0 && threadIdx.x == 0) {
    if (a.dbeta) a.dbeta[c] = (float)sg;
    if (a.dgamma) a.dgamma[c] = (float)sgx;
  }
  if (!a.dx) return;
  const float mean = a.stats[2 * c], rstd = a.stats[2 * c + 1];
  const float k1 = (float)(sg / (double)a.M), k2 = (float)(sgx / (double)a.M), gr = a.gamma[c] * rstd;
  for (; m < m1; m += 256 * VEC, ba_next(q, a)) {
    float gz[VEC], v[VEC], o[VEC];
    ba_load_gz<T, VEC>(a, BA_AT((const T*)a.g), BA_AT((const T*)a.y), gz);
    bn_load<T, VEC>(BA_AT((const T*)a.x), v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = gr * ((gz[j] - k1) - bn_xhat(v[j], mean, rstd) * k2);
    bn_store<T, VEC>(BA_AT((T*)a.dx), o);
  }
}

#undef BA_AT
#undef BA_OWN

}  // namespace tadmm

using namespace tadmm;

namespace {

struct BaPlan { int S, span, cap; };

// the split of a channel, from (M, C, element size) alone: at most `cap` splits (what the workspace is sized for, so
// that its size never falls as M grows), evened out to S splits of `span` values, none of them empty
BaPlan ba_plan(int64_t M, int C, size_t es) {
  const int64_t trip = 256 * (16 / (int64_t)es);
  const int64_t trips = (M + trip - 1) / trip;
  const int64_t want = std::max<int64_t>(1, (kBaTarget + C - 1) / C);
  const int64_t cap = std::min<int64_t>(trips, std::min<int64_t>(kBaMaxSplit, want));
  const int64_t per = (trips + cap - 1) / cap;
  return BaPlan{(int)((trips + per - 1) / per), (int)(per * trip), (int)cap};
}

size_t ba_ws_bytes(int64_t M, int C, size_t es) {
  return align_up((size_t)C * ba_plan(M, C, es).cap * 2 * sizeof(double), 256);
}

enum BaKernel { BA_STAT, BA_TRAIN, BA_EVAL, BA_BWD_SUM, BA_BWD_DX };

template <typename T>
void ba_launch(BaArgs a, BaKernel k, bool wide, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr bool kBwd = !std::is_same<T, bn_f16>::value;        // float16 is forward only (ba_check refuses it)
  const int vec = wide ? V : 1;
  a.step_q = (256 * vec) / a.HW;
  a.step_r = (256 * vec) % a.HW;
  if (!wide) a.res_wide = 0;
  const dim3 grid((unsigned)((int64_t)a.C * a.S)), block(256);
#define BA_GO(VV)                                                                                         \
  switch (k) {                                                                                            \
    case BA_STAT: hipLaunchKernelGGL((bnact_stat_kernel<T, VV>), grid, block, 0, s, a); break;            \
    case BA_TRAIN: hipLaunchKernelGGL((bnact_apply_kernel<T, VV, false>), grid, block, 0, s, a); break;   \
    case BA_EVAL: hipLaunchKernelGGL((bnact_apply_kernel<T, VV, true>), grid, block, 0, s, a); break;     \
    case BA_BWD_SUM:                                                                                      \
      if constexpr (kBwd) hipLaunchKernelGGL((bnact_bwd_sum_kernel<T, VV>), grid, block, 0, s, a);        \
      break;                                                                                              \
    case BA_BWD_DX:                                                                                       \
      if constexpr (kBwd) hipLaunchKernelGGL((bnact_bwd_dx_kernel<T, VV>), grid, block, 0, s, a);         \
      break;                                                                                              \
  }
  if (wide) BA_GO(V) else BA_GO(1)
#undef BA_GO
}

void ba_launch_any(const tadmm_bnact_desc* d, const BaArgs& a, BaKernel k, bool wide, hipStream_t s) {
  if (d->dtype == TADMM_CHAIN_F32) ba_launch<float>(a, k, wide, s);
  else if (d->dtype == TADMM_CHAIN_BF16) ba_launch<bn_bf16>(a, k, wide, s);
  else ba_launch<bn_f16>(a, k, wide, s);
}

inline bool ba_mis(const void* p, size_t n) { return ((uintptr_t)p) % n != 0; }

// what the two entries share: TADMM_OK with *wide and the arguments set, or the refusal
int ba_check(tadmm_ctx_s* h, const tadmm_bnact_desc* d, bool bwd, bool* wide, BaArgs* out) {
  if (!d) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: the descriptor is NULL");
  if (d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1)
    CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: N, C, H, W >= 1 are required (got %d, %d, %d, %d)", d->N, d->C, d->H, d->W);
  if (d->dtype != TADMM_CHAIN_F32 && d->dtype != TADMM_CHAIN_BF16 && d->dtype != TADMM_CHAIN_F16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: unknown element type %d", d->dtype);
  if (bwd && d->dtype == TADMM_CHAIN_F16) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: float16 is forward only");
  const bool training = bwd || d->training != 0;
  const int64_t HW = (int64_t)d->H * d->W, M = HW * d->N;
  if (training && M < 2)
    CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: training needs more than one value per channel (M = %lld)", (long long)M);
  const bool has_res = bwd ? d->dres != nullptr : d->res != nullptr;
  if (has_res && (d->c0 < 0 || d->Cr < 1 || (int64_t)d->c0 + d->Cr > d->C))
    CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: the residual window [%d, %d + %d) is not inside the %d channels", d->c0, d->c0,
             d->Cr, d->C);
  if (!(d->eps >= 0.0) || !(d->eps < INFINITY)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: eps %g must be finite and >= 0", d->eps);
  if (!(d->momentum >= 0.0 && d->momentum <= 1.0))
    CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: momentum %g outside [0, 1]", d->momentum);
  const size_t es = d->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  if (!d->x || ba_mis(d->x, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: x is NULL or misaligned");
  if (!d->gamma || ba_mis(d->gamma, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: gamma is NULL or misaligned");
  if (ba_mis(d->stats, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: stats is misaligned");
  bool w = !ba_mis(d->x, 16) && ((size_t)HW * es) % 16 == 0;
  bool res_wide = false, res_lin = false;
  if (!bwd) {
    if (!d->beta || ba_mis(d->beta, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: beta is NULL or misaligned");
    if (!d->y || ba_mis(d->y, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: y is NULL or misaligned");
    if (ba_mis(d->res, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: res is misaligned");
    if (d->y == d->x || d->y == d->res) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: y and x or res are one buffer");
    if (ba_mis(d->running_mean, 4) || ba_mis(d->running_var, 4))
      CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: the running statistics are misaligned");
    if (!training && (!d->running_mean || !d->running_var))
      CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: eval mode reads running_mean and running_var, one is NULL");
    if ((d->running_mean == nullptr) != (d->running_var == nullptr))
      CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: running_mean and running_var are given together or not at all");
    if (ba_mis(d->num_batches_tracked, 8)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: num_batches_tracked is misaligned");
    w = w && !ba_mis(d->y, 16);
    if (d->res) {
      for (int i = 0; i < 4; ++i)
        if (d->res_stride[i] < 0) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: a stride of res is negative");
      res_lin = d->H == 1 || d->res_stride[2] == d->res_stride[3] * d->W;
      res_wide = res_lin && (d->res_stride[3] == 1 || HW == 1) && !ba_mis(d->res, 16) &&
                 ((size_t)d->res_stride[0] * es) % 16 == 0 && ((size_t)d->res_stride[1] * es) % 16 == 0;
    }
  } else {
    if (!d->stats) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: stats is NULL and the backward reads it");
    if (!d->g || ba_mis(d->g, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: g is NULL or misaligned");
    if (d->relu && (!d->y || ba_mis(d->y, es)))
      CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: y is NULL or misaligned and the ReLU mask reads it");
    if (ba_mis(d->dx, es) || ba_mis(d->dres, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: dx / dres are not aligned to their element");
    if (d->dx && d->dx == d->dres) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: dx and dres are one buffer");
    if (ba_mis(d->dgamma, 4) || ba_mis(d->dbeta, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "bnact: dgamma / dbeta are misaligned");
    w = w && !ba_mis(d->g, 16) && !ba_mis(d->dx, 16) && !ba_mis(d->dres, 16) && (!d->relu || !ba_mis(d->y, 16));
  }
  if (M > kBaMaxM)
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "bnact: N H W = %lld, the launch takes at most %lld values per channel", (long long)M,
             (long long)kBaMaxM);
  const bool need_ws = bwd ? (d->dx || d->dgamma || d->dbeta) : training;
  if (need_ws) {
    const size_t need = ba_ws_bytes(M, d->C, es);
    if (!d->workspace || ba_mis(d->workspace, 16) || d->workspace_bytes < need)
      CTX_FAIL(h, TADMM_ERR_WORKSPACE, "bnact workspace too small or misaligned: need %zu bytes, got %zu", need,
               d->workspace_bytes);
  }
  const BaPlan plan = ba_plan(M, d->C, es);
  BaArgs a{};
  a.x = d->x; a.res = d->res;
  a.rs0 = d->res_stride[0]; a.rs1 = d->res_stride[1]; a.rs2 = d->res_stride[2]; a.rs3 = d->res_stride[3];
  a.gamma = d->gamma; a.beta = d->beta;
  a.rmean = d->running_mean; a.rvar = d->running_var; a.nbt = d->num_batches_tracked;
  a.y = d->y; a.stats = d->stats;
  a.g = d->g; a.dx = d->dx; a.dres = d->dres; a.dgamma = d->dgamma; a.dbeta = d->dbeta;
  a.part = need_ws ? (double*)d->workspace : nullptr;
  a.eps = d->eps; a.momentum = d->momentum;
  a.C = d->C; a.HW = (int32_t)HW; a.W = d->W; a.c0 = d->c0; a.Cr = d->Cr; a.M = (int32_t)M;
  a.S = plan.S; a.span = plan.span;
  a.relu = d->relu != 0; a.res_wide = res_wide; a.res_lin = res_lin;
  *wide = w;
  *out = a;
  return TADMM_OK;
}

}  // namespace

extern "C" {

int tadmm_bnact_desc_bytes(void) { return (int)sizeof(tadmm_bnact_desc); }

int tadmm_bnact_fits(const tadmm_bnact_desc* d, int64_t* max_m) {
  if (max_m) *max_m = kBaMaxM;
  if (!d || d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1) return TADMM_ERR_INVALID;
  return (int64_t)d->N * d->H * d->W <= kBaMaxM ? 1 : 0;
}

int tadmm_bnact_workspace_bytes(const tadmm_bnact_desc* d, size_t* bytes) {
  if (!d || !bytes || d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1) return TADMM_ERR_INVALID;
  if (d->dtype != TADMM_CHAIN_F32 && d->dtype != TADMM_CHAIN_BF16 && d->dtype != TADMM_CHAIN_F16) return TADMM_ERR_INVALID;
  const int64_t M = (int64_t)d->N * d->H * d->W;
  if (M > kBaMaxM) return TADMM_ERR_UNSUPPORTED;
  *bytes = ba_ws_bytes(M, d->C, d->dtype == TADMM_CHAIN_F32 ? 4 : 2);
  return TADMM_OK;
}

int tadmm_bnact_plan(const tadmm_bnact_desc* d, int32_t* plan3) {
  if (!d || !plan3 || d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1) return TADMM_ERR_INVALID;
  if (d->dtype != TADMM_CHAIN_F32 && d->dtype != TADMM_CHAIN_BF16 && d->dtype != TADMM_CHAIN_F16) return TADMM_ERR_INVALID;
  const int64_t M = (int64_t)d->N * d->H * d->W;
  if (M > kBaMaxM) return TADMM_ERR_UNSUPPORTED;
  const BaPlan p = ba_plan(M, d->C, d->dtype == TADMM_CHAIN_F32 ? 4 : 2);
  plan3[0] = p.S; plan3[1] = p.span; plan3[2] = p.cap;
  return TADMM_OK;
}

int tadmm_bnact_fwd(tadmm_handle h, const tadmm_bnact_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  BaArgs a;
  const int rc = ba_check(h, d, false, &wide, &a);
  if (rc != TADMM_OK) return rc;
  DeviceGuard device_guard(h);
  hipStream_t s = (hipStream_t)stream_;
  if (d->training) {
    ba_launch_any(d, a, BA_STAT, wide, s);
    ba_launch_any(d, a, BA_TRAIN, wide, s);
  } else {
    a.stats = nullptr;
    ba_launch_any(d, a, BA_EVAL, wide, s);
  }
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_bnact_bwd(tadmm_handle h, const tadmm_bnact_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  BaArgs a;
  const int rc = ba_check(h, d, true, &wide, &a);
  if (rc != TADMM_OK) return rc;
  if (!a.part && !a.dres) return TADMM_OK;                  // nothing is wanted
  DeviceGuard device_guard(h);
  hipStream_t s = (hipStream_t)stream_;
  ba_launch_any(d, a, BA_BWD_SUM, wide, s);
  if (a.part) ba_launch_any(d, a, BA_BWD_DX, wide, s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
