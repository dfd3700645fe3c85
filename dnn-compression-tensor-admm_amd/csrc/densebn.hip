// The pre-activation of a DenseNet layer (densenet_cifar_tt.py: BasicBlock / BottleneckBlock / TransitionBlock,
// densenet_inet_tt.py: DenseLayer / DenseTransition): relu(bn(torch.cat(features, 1))) without the concatenation and
// without recomputing the batch statistics of channels an earlier layer of the block has already seen.
// Segment k is (N, C_k, H, W), NCHW contiguous; channel c of the concatenation is channel c - first_k of the segment
// with first_k <= c < first_k + C_k.  A channel's M = N H W values lie in N planes of HW elements.
//
//     stats_k[cl] = (mean, biased variance) of channel cl of segment k, double      (once per segment, densebn_stats)
//     rstd_c = 1 / sqrt(var_c + eps)                                                (per consuming layer: its own eps)
//     y[n, c, h, w] = act(gamma_c (x_k[n, c - first_k, h, w] - mean_c) rstd_c + beta_c)        (N, C, H, W) contiguous
//
// The segment table (data, stats, dx pointers and the first channels) travels in the kernel arguments; a workgroup
// finds its channel's segment by a bisection of the first channels, on scalar registers (the channel is uniform).
//
// Ownership is that of bnact.hip: a channel's values m = n HW + p are cut into S splits of `span` values, span a
// multiple of the trip 256 * (16 / sizeof(T)); workgroup (c, s) = blockIdx.x owns split s of channel c and walks it in
// trips, lane t at m0 + trip * 256 * VEC + t * VEC, keeping (n, p) by addition.  S comes from (M, C, dtype) alone.
//
//   1. densebn_stat_kernel<T, VEC>        one segment: sum (x - K) and sum (x - K)^2 in double, K = x[0, c, 0, 0].
//   2. densebn_finish_kernel              one lane per channel adds the S partials in ascending order: mean and variance.
//   3. densebn_apply_kernel<T, VEC, EVAL> y; training: split 0 updates the layer's running statistics (momentum, unbiased
//                                         variance M / (M - 1)) and channel 0 the batch counter.  Eval: a = gamma /
//                                         sqrt(running_var + eps), b = beta - running_mean a, y = act(a x + b).
//   4. densebn_bwd_sum_kernel<T, VEC>     gz = g (y > 0) from y as stored; sum gz and sum gz xhat in double.
//   5. densebn_bwd_dx_kernel<T, VEC>      the partials added in a fixed order; split 0 writes dgamma and dbeta;
//                                         dx_k = gamma rstd (gz - dbeta / M - xhat dgamma / M) into the segment's own
//                                         (N, C_k, H, W) output; a segment without one is only summed.
// No atomics; grids depend on the shapes and dtype alone: bitwise reproducible.  Accesses: VEC elements = 16 bytes when
// every base in use is 16-byte aligned and HW is a whole number of 16-byte units; one element otherwise.
#include "rownorm_common.h"

namespace tadmm {

constexpr int kDbTarget = 2048;              // workgroups the split aims at
constexpr int kDbMaxSplit = 128;             // two partials per lane in the fixed-order sum
constexpr int64_t kDbMaxM = (int64_t(1) << 31) - 4096;
constexpr int kDbMaxSeg = TADMM_DENSEBN_MAX_SEGMENTS;

struct DbArgs {
  const void* x[kDbMaxSeg];
  const double* stats[kDbMaxSeg];
  void* dx[kDbMaxSeg];
  int32_t first[kDbMaxSeg + 1];              // first[nseg] = C
  const float* gamma; const float* beta;
  float* rmean; float* rvar; int64_t* nbt;
  void* y; const void* g; float* dgamma; float* dbeta;
  double* part;
  double eps, momentum;
  int32_t C, HW, M, S, span, nseg, relu;
  int32_t step_q, step_r;                    // (256 * VEC) / HW and % HW: one trip in (n, p)
};

// the stats launches carry one segment
struct DbStatArgs {
  const void* x; double* stats; double* part;
  int32_t C, HW, M, S, span, step_q, step_r;
};

struct DbPos { int n, p; };

__device__ __forceinline__ void db_next(DbPos& q, int HW, int step_q, int step_r) {
  q.p += step_r;
  q.n += step_q;
  if (q.p >= HW) { q.p -= HW; ++q.n; }
}

// the segment of channel c: the last k with first[k] <= c
__device__ __forceinline__ int db_find(const DbArgs& a, int c) {
  int lo = 0, hi = a.nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.first[mid] <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// both sums of the workgroup on thread 0: lanes by the butterfly, then waves 1 .. 3 in that order
__device__ __forceinline__ void db_block_sum2(double& u, double& v) {
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
__device__ __forceinline__ void db_combine(const double* __restrict__ part, int S, int c, double& u, double& v) {
  const int lane = threadIdx.x & 63;
  const double* __restrict__ p = part + (int64_t)c * S * 2;
  u = v = 0.0;
  if (lane < S) { u = p[2 * lane]; v = p[2 * lane + 1]; }
  if (lane + 64 < S) { u += p[2 * (lane + 64)]; v += p[2 * (lane + 64) + 1]; }
  u = bn_wave_sum(u);
  v = bn_wave_sum(v);
}

#define DB_OWN()                                                       \
  const int c = blockIdx.x / a.S, s = blockIdx.x - c * a.S;            \
  const int m1 = min(a.M, (s + 1) * a.span);                           \
  int m = s * a.span + (int)threadIdx.x * VEC;                         \
  DbPos q;                                                             \
  q.n = m / a.HW;                                                      \
  q.p = m - q.n * a.HW
// the segment of the channel: k, the channel inside it and the segment's width
#define DB_SEG()                                                       \
  const int k = db_find(a, c);                                         \
  const int cl = c - a.first[k], Ck = a.first[k + 1] - a.first[k]
#define DB_AT(ptr) ((ptr) + ((int64_t)q.n * a.C + c) * a.HW + q.p)
#define DB_SEG_AT(ptr) ((ptr) + ((int64_t)q.n * Ck + cl) * a.HW + q.p)
#define DB_NEXT() m += 256 * VEC, db_next(q, a.HW, a.step_q, a.step_r)

template <typename T, int VEC>
__global__ __launch_bounds__(256) void densebn_stat_kernel(const DbStatArgs a) {
  DB_OWN();
  const double K = (double)bn_widen(((const T*)a.x)[(int64_t)c * a.HW]);
  double s1 = 0.0, s2 = 0.0;
  for (; m < m1; DB_NEXT()) {
    float v[VEC];
    bn_load<T, VEC>(DB_AT((const T*)a.x), v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const double d = (double)v[j] - K;
      s1 += d;
      s2 = fma(d, d, s2);
    }
  }
  db_block_sum2(s1, s2);
  if (threadIdx.x == 0) {
    a.part[(int64_t)blockIdx.x * 2] = s1;
    a.part[(int64_t)blockIdx.x * 2 + 1] = s2;
  }
}

// one lane per channel: the S partials in ascending order, (mean, biased variance) in double
template <typename T>
__global__ __launch_bounds__(256) void densebn_finish_kernel(const DbStatArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.C) return;
  const double* __restrict__ p = a.part + (int64_t)c * a.S * 2;
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < a.S; ++i) { s1 += p[2 * i]; s2 += p[2 * i + 1]; }
  const double K = (double)bn_widen(((const T*)a.x)[(int64_t)c * a.HW]);
  const double dm = (double)a.M;
  a.stats[2 * c] = K + s1 / dm;
  a.stats[2 * c + 1] = fmax((s2 - s1 * s1 / dm) / dm, 0.0);
}

template <typename T, int VEC, bool EVAL>
__global__ __launch_bounds__(256) void densebn_apply_kernel(const DbArgs a) {
  DB_OWN();
  DB_SEG();
  const float gam = a.gamma[c], bet = a.beta[c];
  double mean = 0.0, rstd = 0.0;
  float ea = 0.f, eb = 0.f;
  if constexpr (EVAL) {
    const double ad = (double)gam / sqrt((double)a.rvar[c] + a.eps);
    ea = (float)ad;
    eb = (float)((double)bet - (double)a.rmean[c] * ad);
  } else {
    const double* __restrict__ st = a.stats[k];
    mean = st[2 * cl];
    const double var = st[2 * cl + 1];
    rstd = 1.0 / sqrt(var + a.eps);
    if (s == 0 && threadIdx.x == 0) {
      if (a.rmean) {
        const double dm = (double)a.M;
        a.rmean[c] = (float)((1.0 - a.momentum) * (double)a.rmean[c] + a.momentum * mean);
        a.rvar[c] = (float)((1.0 - a.momentum) * (double)a.rvar[c] + a.momentum * (var * dm / (dm - 1.0)));
      }
      if (a.nbt && c == 0) *a.nbt += 1;
    }
  }
  const T* __restrict__ xk = (const T*)a.x[k];
  for (; m < m1; DB_NEXT()) {
    float v[VEC], o[VEC];
    bn_load<T, VEC>(DB_SEG_AT(xk), v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if constexpr (EVAL) o[j] = fmaf(ea, v[j], eb);
      else o[j] = fmaf(gam, (float)(((double)v[j] - mean) * rstd), bet);
      if (a.relu) o[j] = o[j] < 0.f ? 0.f : o[j];                               // a NaN stays
    }
    bn_store<T, VEC>(DB_AT((T*)a.y), o);
  }
}

// gz of VEC values: the upstream gradient where the stored output is positive
template <typename T, int VEC>
__device__ __forceinline__ void db_load_gz(int relu, const T* __restrict__ gp, const T* __restrict__ yp,
                                           float (&gz)[VEC]) {
  bn_load<T, VEC>(gp, gz);
  if (relu) {
    float yv[VEC];
    bn_load<T, VEC>(yp, yv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) gz[j] = yv[j] > 0.f ? gz[j] : 0.f;
  }
}

__device__ __forceinline__ float db_xhat(float v, double mean, double rstd) { return (float)(((double)v - mean) * rstd); }

template <typename T, int VEC>
__global__ __launch_bounds__(256) void densebn_bwd_sum_kernel(const DbArgs a) {
  DB_OWN();
  DB_SEG();
  if (!a.dx[k] && !a.dgamma && !a.dbeta) return;                                 // nobody reads this channel's sums
  const double* __restrict__ st = a.stats[k];
  const double mean = st[2 * cl], rstd = 1.0 / sqrt(st[2 * cl + 1] + a.eps);
  const T* __restrict__ xk = (const T*)a.x[k];
  double sg = 0.0, sgx = 0.0;
  for (; m < m1; DB_NEXT()) {
    float gz[VEC], v[VEC];
    db_load_gz<T, VEC>(a.relu, DB_AT((const T*)a.g), DB_AT((const T*)a.y), gz);
    bn_load<T, VEC>(DB_SEG_AT(xk), v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      sg += (double)gz[j];
      sgx = fma((double)gz[j], (double)db_xhat(v[j], mean, rstd), sgx);
    }
  }
  db_block_sum2(sg, sgx);
  if (threadIdx.x == 0) {
    a.part[(int64_t)blockIdx.x * 2] = sg;
    a.part[(int64_t)blockIdx.x * 2 + 1] = sgx;
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void densebn_bwd_dx_kernel(const DbArgs a) {
  DB_OWN();
  DB_SEG();
  T* __restrict__ dxk = (T*)a.dx[k];
  if (!dxk && (s != 0 || (!a.dgamma && !a.dbeta))) return;
  double sg, sgx;
  db_combine(a.part, a.S, c, sg, sgx);
  if (s == 0 && threadIdx.x == 0) {
    if (a.dbeta) a.dbeta[c] = (float)sg;
    if (a.dgamma) a.dgamma[c] = (float)sgx;
  }
  if (!dxk) return;
  const double* __restrict__ st = a.stats[k];
  const double mean = st[2 * cl], rstd = 1.0 / sqrt(st[2 * cl + 1] + a.eps);
  const float k1 = (float)(sg / (double)a.M), k2 = (float)(sgx / (double)a.M), gr = a.gamma[c] * (float)rstd;
  const T* __restrict__ xk = (const T*)a.x[k];
  for (; m < m1; DB_NEXT()) {
    float gz[VEC], v[VEC], o[VEC];
    db_load_gz<T, VEC>(a.relu, DB_AT((const T*)a.g), DB_AT((const T*)a.y), gz);
    bn_load<T, VEC>(DB_SEG_AT(xk), v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = gr * ((gz[j] - k1) - db_xhat(v[j], mean, rstd) * k2);
    bn_store<T, VEC>(DB_SEG_AT(dxk), o);
  }
}

#undef DB_NEXT
#undef DB_SEG_AT
#undef DB_AT
#undef DB_SEG
#undef DB_OWN

}  // namespace tadmm

using namespace tadmm;

namespace {

static_assert(sizeof(DbArgs) <= 4096, "the segment table must fit the kernel arguments");

struct DbPlan { int S, span, cap; };

// the split of a channel, from (M, C, element size) alone (bnact.hip: ba_plan): at most `cap` splits (what the
// workspace is sized for, so that its size never falls as M grows), evened out to S splits of `span` values, none empty
DbPlan db_plan(int64_t M, int64_t C, size_t es) {
  const int64_t trip = 256 * (16 / (int64_t)es);
  const int64_t trips = (M + trip - 1) / trip;
  const int64_t want = std::max<int64_t>(1, (kDbTarget + C - 1) / C);
  const int64_t cap = std::min<int64_t>(trips, std::min<int64_t>(kDbMaxSplit, want));
  const int64_t per = (trips + cap - 1) / cap;
  return DbPlan{(int)((trips + per - 1) / per), (int)(per * trip), (int)cap};
}

size_t db_ws_bytes(int64_t M, int64_t C, size_t es) {
  return align_up((size_t)C * db_plan(M, C, es).cap * 2 * sizeof(double), 256);
}

inline bool db_mis(const void* p, size_t n) { return ((uintptr_t)p) % n != 0; }
inline bool db_dtype_ok(int dt) { return dt == TADMM_CHAIN_F32 || dt == TADMM_CHAIN_BF16 || dt == TADMM_CHAIN_F16; }

// N, H, W >= 1, 1 <= nseg <= cap and every C_k >= 1: the total channel count, or -1
int64_t db_channels(const tadmm_densebn_desc* d) {
  if (!d || d->N < 1 || d->H < 1 || d->W < 1 || d->nseg < 1 || d->nseg > kDbMaxSeg) return -1;
  int64_t C = 0;
  for (int k = 0; k < d->nseg; ++k) {
    if (d->seg[k].C < 1) return -1;
    C += d->seg[k].C;
  }
  return C;
}

enum DbKernel { DB_TRAIN, DB_EVAL, DB_BWD_SUM, DB_BWD_DX };

template <typename T>
void db_launch(DbArgs a, DbKernel kn, bool wide, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr bool kBwd = !std::is_same<T, bn_f16>::value;        // float16 is forward only (db_check refuses it)
  const int vec = wide ? V : 1;
  a.step_q = (256 * vec) / a.HW;
  a.step_r = (256 * vec) % a.HW;
  const dim3 grid((unsigned)((int64_t)a.C * a.S)), block(256);
#define DB_GO(VV)                                                                                           \
  switch (kn) {                                                                                             \
    case DB_TRAIN: hipLaunchKernelGGL((densebn_apply_kernel<T, VV, false>), grid, block, 0, s, a); break;   \
    case DB_EVAL: hipLaunchKernelGGL((densebn_apply_kernel<T, VV, true>), grid, block, 0, s, a); break;     \
    case DB_BWD_SUM:                                                                                        \
      if constexpr (kBwd) hipLaunchKernelGGL((densebn_bwd_sum_kernel<T, VV>), grid, block, 0, s, a);        \
      break;                                                                                                \
    case DB_BWD_DX:                                                                                         \
      if constexpr (kBwd) hipLaunchKernelGGL((densebn_bwd_dx_kernel<T, VV>), grid, block, 0, s, a);         \
      break;                                                                                                \
  }
  if (wide) DB_GO(V) else DB_GO(1)
#undef DB_GO
}

void db_launch_any(int dtype, const DbArgs& a, DbKernel kn, bool wide, hipStream_t s) {
  if (dtype == TADMM_CHAIN_F32) db_launch<float>(a, kn, wide, s);
  else if (dtype == TADMM_CHAIN_BF16) db_launch<bn_bf16>(a, kn, wide, s);
  else db_launch<bn_f16>(a, kn, wide, s);
}

template <typename T>
void db_launch_stats(DbStatArgs a, bool wide, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(T);
  const int vec = wide ? V : 1;
  a.step_q = (256 * vec) / a.HW;
  a.step_r = (256 * vec) % a.HW;
  const dim3 grid((unsigned)((int64_t)a.C * a.S)), block(256);
  if (wide) hipLaunchKernelGGL((densebn_stat_kernel<T, V>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((densebn_stat_kernel<T, 1>), grid, block, 0, s, a);
  hipLaunchKernelGGL((densebn_finish_kernel<T>), dim3((unsigned)((a.C + 255) / 256)), block, 0, s, a);
}

// what every launching entry checks first: the shape, the type and the bound of _fits; *C_out and *es_out on TADMM_OK
int db_check_shape(tadmm_ctx_s* h, const tadmm_densebn_desc* d, bool training, bool bwd, int64_t* C_out, size_t* es_out) {
  if (!d) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: the descriptor is NULL");
  if (d->N < 1 || d->H < 1 || d->W < 1)
    CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: N, H, W >= 1 are required (got %d, %d, %d)", d->N, d->H, d->W);
  if (d->nseg < 1 || d->nseg > kDbMaxSeg)
    CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: %d segments, 1 .. %d are taken", d->nseg, kDbMaxSeg);
  const int64_t C = db_channels(d);
  if (C < 1) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: every segment needs at least one channel");
  if (!db_dtype_ok(d->dtype)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: unknown element type %d", d->dtype);
  if (bwd && d->dtype == TADMM_CHAIN_F16) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: float16 is forward only");
  const int64_t M = (int64_t)d->N * d->H * d->W;
  if (training && M < 2)
    CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: training needs more than one value per channel (M = %lld)", (long long)M);
  *C_out = C;                                                   // set before the bounds: the caller checks on
  *es_out = d->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  if (M > kDbMaxM)
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "densebn: N H W = %lld, the launch takes at most %lld values per channel",
             (long long)M, (long long)kDbMaxM);
  if (C * (int64_t)kDbMaxSplit > INT32_MAX)
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "densebn: %lld channels are more than the grid takes", (long long)C);
  return TADMM_OK;
}

int db_check_ws(tadmm_ctx_s* h, const tadmm_densebn_desc* d, size_t need) {
  if (!d->workspace || db_mis(d->workspace, 16) || d->workspace_bytes < need)
    CTX_FAIL(h, TADMM_ERR_WORKSPACE, "densebn workspace too small or misaligned: need %zu bytes, got %zu", need,
             d->workspace_bytes);
  return TADMM_OK;
}

// forward and backward: TADMM_OK with *wide and the arguments set, or the refusal
int db_check(tadmm_ctx_s* h, const tadmm_densebn_desc* d, bool bwd, bool* wide, DbArgs* out) {
  const bool training = bwd || (d && d->training != 0);
  int64_t C = 0;
  size_t es = 0;
  const int rc = db_check_shape(h, d, training, bwd, &C, &es);
  if (rc != TADMM_OK && rc != TADMM_ERR_UNSUPPORTED) return rc;
  if (!(d->eps >= 0.0) || !(d->eps < INFINITY)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: eps %g must be finite and >= 0", d->eps);
  if (!(d->momentum >= 0.0 && d->momentum <= 1.0))
    CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: momentum %g outside [0, 1]", d->momentum);
  const int64_t HW = (int64_t)d->H * d->W, M = HW * d->N;
  if (!d->gamma || db_mis(d->gamma, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: gamma is NULL or misaligned");
  bool w = ((size_t)HW * es) % 16 == 0;
  const char* y0 = (const char*)d->y;
  for (int k = 0; k < d->nseg; ++k) {
    const tadmm_densebn_seg& sg = d->seg[k];
    if (!sg.x || db_mis(sg.x, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: x of segment %d is NULL or misaligned", k);
    if (training && (!sg.stats || db_mis(sg.stats, 8)))
      CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: stats of segment %d is NULL or misaligned and training mode reads it", k);
    w = w && !db_mis(sg.x, 16);
    if (bwd) {
      if (db_mis(sg.dx, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: dx of segment %d is not aligned to its element", k);
      if (sg.dx && (sg.dx == sg.x || sg.dx == d->g || sg.dx == d->y))
        CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: dx of segment %d and x, g or y are one buffer", k);
      w = w && !db_mis(sg.dx, 16);
    } else if (y0 && rc == TADMM_OK) {                          // the byte ranges of a shape the launch takes
      const char* x0 = (const char*)sg.x;
      const size_t xb = (size_t)M * sg.C * es, yb = (size_t)M * (size_t)C * es;
      if (x0 < y0 + yb && y0 < x0 + xb) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: y overlaps segment %d", k);
    }
  }
  if (!bwd) {
    if (!d->beta || db_mis(d->beta, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: beta is NULL or misaligned");
    if (!d->y || db_mis(d->y, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: y is NULL or misaligned");
    if (db_mis(d->running_mean, 4) || db_mis(d->running_var, 4))
      CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: the running statistics are misaligned");
    if (!training && (!d->running_mean || !d->running_var))
      CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: eval mode reads running_mean and running_var, one is NULL");
    if ((d->running_mean == nullptr) != (d->running_var == nullptr))
      CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: running_mean and running_var are given together or not at all");
    if (db_mis(d->num_batches_tracked, 8)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: num_batches_tracked is misaligned");
    w = w && !db_mis(d->y, 16);
  } else {
    if (!d->g || db_mis(d->g, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: g is NULL or misaligned");
    if (d->relu && (!d->y || db_mis(d->y, es)))
      CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: y is NULL or misaligned and the ReLU mask reads it");
    if (db_mis(d->dgamma, 4) || db_mis(d->dbeta, 4)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn: dgamma / dbeta are misaligned");
    w = w && !db_mis(d->g, 16) && (!d->relu || !db_mis(d->y, 16));
  }
  if (rc != TADMM_OK) return rc;                                // TADMM_ERR_UNSUPPORTED; its message is set
  bool any_out = d->dgamma || d->dbeta;
  if (bwd) {
    for (int k = 0; k < d->nseg; ++k) any_out = any_out || d->seg[k].dx;
    if (any_out) {
      const int wrc = db_check_ws(h, d, db_ws_bytes(M, C, es));
      if (wrc != TADMM_OK) return wrc;
    }
  }
  const DbPlan plan = db_plan(M, C, es);
  DbArgs a{};
  int32_t first = 0;
  for (int k = 0; k < d->nseg; ++k) {
    a.x[k] = d->seg[k].x; a.stats[k] = d->seg[k].stats; a.dx[k] = bwd ? d->seg[k].dx : nullptr;
    a.first[k] = first;
    first += d->seg[k].C;
  }
  for (int k = d->nseg; k <= kDbMaxSeg; ++k) a.first[k] = first;
  a.gamma = d->gamma; a.beta = d->beta;
  a.rmean = d->running_mean; a.rvar = d->running_var; a.nbt = d->num_batches_tracked;
  a.y = d->y; a.g = d->g; a.dgamma = d->dgamma; a.dbeta = d->dbeta;
  a.part = bwd && any_out ? (double*)d->workspace : nullptr;
  a.eps = d->eps; a.momentum = d->momentum;
  a.C = (int32_t)C; a.HW = (int32_t)HW; a.M = (int32_t)M; a.S = plan.S; a.span = plan.span;
  a.nseg = d->nseg; a.relu = d->relu != 0;
  *wide = w;
  *out = a;
  return TADMM_OK;
}

}  // namespace

extern "C" {

int tadmm_densebn_desc_bytes(void) { return (int)sizeof(tadmm_densebn_desc); }

int tadmm_densebn_max_segments(void) { return kDbMaxSeg; }

int tadmm_densebn_fits(const tadmm_densebn_desc* d, int64_t* max_m) {
  if (max_m) *max_m = kDbMaxM;
  if (!d || d->N < 1 || d->H < 1 || d->W < 1 || d->nseg < 1) return TADMM_ERR_INVALID;
  if (d->nseg > kDbMaxSeg) return 0;
  const int64_t C = db_channels(d);
  if (C < 1) return TADMM_ERR_INVALID;
  return (int64_t)d->N * d->H * d->W <= kDbMaxM && C * (int64_t)kDbMaxSplit <= INT32_MAX ? 1 : 0;
}

int tadmm_densebn_workspace_bytes(const tadmm_densebn_desc* d, size_t* bytes) {
  if (!bytes || !d || !db_dtype_ok(d->dtype)) return TADMM_ERR_INVALID;
  const int64_t C = db_channels(d);
  if (C < 1) return TADMM_ERR_INVALID;
  const int64_t M = (int64_t)d->N * d->H * d->W;
  if (M > kDbMaxM || C * (int64_t)kDbMaxSplit > INT32_MAX) return TADMM_ERR_UNSUPPORTED;
  *bytes = db_ws_bytes(M, C, d->dtype == TADMM_CHAIN_F32 ? 4 : 2);
  return TADMM_OK;
}

int tadmm_densebn_plan(const tadmm_densebn_desc* d, int32_t* plan3) {
  if (!plan3 || !d || !db_dtype_ok(d->dtype)) return TADMM_ERR_INVALID;
  const int64_t C = db_channels(d);
  if (C < 1) return TADMM_ERR_INVALID;
  const int64_t M = (int64_t)d->N * d->H * d->W;
  if (M > kDbMaxM || C * (int64_t)kDbMaxSplit > INT32_MAX) return TADMM_ERR_UNSUPPORTED;
  const DbPlan p = db_plan(M, C, d->dtype == TADMM_CHAIN_F32 ? 4 : 2);
  plan3[0] = p.S; plan3[1] = p.span; plan3[2] = p.cap;
  return TADMM_OK;
}

int tadmm_densebn_stats(tadmm_handle h, const tadmm_densebn_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  int64_t C = 0;
  size_t es = 0;
  const int rc = db_check_shape(h, d, true, false, &C, &es);
  if (rc != TADMM_OK && rc != TADMM_ERR_UNSUPPORTED) return rc;
  if (d->nseg != 1) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn_stats: one segment per call (got %d)", d->nseg);
  const tadmm_densebn_seg& sg = d->seg[0];
  if (!sg.x || db_mis(sg.x, es)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn_stats: x is NULL or misaligned");
  if (!sg.stats || db_mis(sg.stats, 8)) CTX_FAIL(h, TADMM_ERR_INVALID, "densebn_stats: stats is NULL or misaligned");
  if (rc != TADMM_OK) return rc;
  const int64_t HW = (int64_t)d->H * d->W, M = HW * d->N;
  const int wrc = db_check_ws(h, d, db_ws_bytes(M, C, es));
  if (wrc != TADMM_OK) return wrc;
  const DbPlan plan = db_plan(M, C, es);
  DbStatArgs a{};
  a.x = sg.x; a.stats = sg.stats; a.part = (double*)d->workspace;
  a.C = (int32_t)C; a.HW = (int32_t)HW; a.M = (int32_t)M; a.S = plan.S; a.span = plan.span;
  const bool wide = !db_mis(sg.x, 16) && ((size_t)HW * es) % 16 == 0;
  DeviceGuard device_guard(h);
  hipStream_t s = (hipStream_t)stream_;
  if (d->dtype == TADMM_CHAIN_F32) db_launch_stats<float>(a, wide, s);
  else if (d->dtype == TADMM_CHAIN_BF16) db_launch_stats<bn_bf16>(a, wide, s);
  else db_launch_stats<bn_f16>(a, wide, s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_densebn_fwd(tadmm_handle h, const tadmm_densebn_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  DbArgs a;
  const int rc = db_check(h, d, false, &wide, &a);
  if (rc != TADMM_OK) return rc;
  DeviceGuard device_guard(h);
  db_launch_any(d->dtype, a, d->training ? DB_TRAIN : DB_EVAL, wide, (hipStream_t)stream_);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_densebn_bwd(tadmm_handle h, const tadmm_densebn_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  bool wide = false;
  DbArgs a;
  const int rc = db_check(h, d, true, &wide, &a);
  if (rc != TADMM_OK) return rc;
  if (!a.part) return TADMM_OK;                             // nothing is wanted
  DeviceGuard device_guard(h);
  hipStream_t s = (hipStream_t)stream_;
  db_launch_any(d->dtype, a, DB_BWD_SUM, wide, s);
  db_launch_any(d->dtype, a, DB_BWD_DX, wide, s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
