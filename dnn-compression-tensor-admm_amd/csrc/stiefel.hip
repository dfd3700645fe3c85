// Riemannian SGD on the Stiefel manifold (the reference's StfTKConv.py trained by geoopt.optim.RiemannianSGD): every
// factor of a model in ONE launch, one workgroup of 256 threads per factor, its tiles resident in LDS.
//
// Per factor X (n x p, n >= p, columns orthonormal), gradient G, momentum buffer M, sym(A) = (A + A^T) / 2:
//   1. g = G + weight_decay X
//   2. r = g - X sym(X^T g)                         tangent projection of the embedded metric
//   3. momentum > 0:  M <- momentum M + (1 - dampening) r,  d = nesterov ? r + momentum M : M;   else d = r
//   4. Y = X - lr d
//   5. X+ = Q factor of Y = Q R with diag(R) > 0    the QR retraction with geoopt's sign "unflip"
//   6. momentum > 0:  M+ = M - X+ sym(X+^T M)       vector transport by projection
// `project` mode is step 5 alone on an arbitrary full-rank X.
// Riemannian Adam (geoopt.optim.RiemannianAdam) is a second instantiation of the same body, `stiefel_adam_kernel`.  M is
// exp_avg; v (ONE float32 second moment per factor), vmax (its running maximum, amsgrad) and t (int32 counter) live in
// per-factor device arrays:
//   3'. t' = t + 1,  s = sum r^2,  M' = beta1 M + (1 - beta1) r,  v' = beta2 v + (1 - beta2) s,  u = amsgrad ? max(vmax, v') : v'
//   4'. Y = X - lr / ((1 - beta1^t') (sqrt(u / (1 - beta2^t')) + eps)) M'
// then steps 5 and 6.  The scale of step 4' needs s over the whole factor, so Y cannot be formed in the epilogue of the
// tangent-projection product as the SGD mode does: the epilogue stores M' and keeps per-thread fp64 partial sums of r^2,
// a fixed-order reduction follows (a butterfly inside each wave, the four waves' sums added in order from LDS that is
// idle at that point: the fp64 carves, 64 contiguous bytes even at p = 1), and one elementwise pass forms Y -- two
// barriers more than the SGD mode.  The bias corrections come from the factor's own counter, in fp64, on the device.
// v', u and t' are written by thread 0 in the last phase, like X and M, so a failed factor keeps all five.
//
// Arithmetic.  HBM is read once (X, G, M) and written once (X, M); everything between lives in LDS: three fp32 tiles
// (row pitch p|1) and two fp64 p x p matrices (row pitch p|1) plus two fp64 p-vectors.  Every inner product (X^T g, the
// Gram Y^T Y, the products with the p x p matrices) is accumulated in fp64 from the fp32 tiles on the vector ALU, in
// 4 x 4 register tiles per thread; every stored entry is rounded to fp32 once.  At p <= 64 the products are a latency
// matter (one workgroup, <= 2^18 multiply-adds each): the matrix cores would add operand shuffles to loops that are
// bound by the ~3 p barriers of the factorisation, so they are not used.
// Step 5 is a Cholesky QR: S = Y^T Y = R^T R factored in fp64 (right-looking, two barriers per column), W = R^-1 by
// back substitution (four lanes per column, one barrier per row), Q = Y W.  One pass leaves ||Q^T Q - I|| of the order
// of cond(S) * 2^-53; when the pivots spread by more than kStfSecondPass (a lower bound of cond(S)) a second pass runs
// on Q.  In a training step Y = X + O(lr), S = I + O(lr) and one pass is taken.
// A pivot that is not above kStfPivotFloor times its column's squared norm, or not finite, ends the factor: nothing of
// it is written back, its int32 status word is set with an ordinary store, the workgroup returns.  The decision is taken
// from LDS values every thread reads alike, so the barriers stay uniform.
// No atomics, fixed summation orders: a factor's result does not depend on what else is in the launch.
#include "host.h"

namespace tadmm {

constexpr size_t kStfMaxLds = 160 * 1024;
constexpr int kStfThreads = 256;
constexpr double kStfSecondPass = 1e4;
constexpr double kStfPivotFloor = 4e-14;

static inline __host__ __device__ size_t stf_align16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline __host__ __device__ size_t stf_tile_bytes(int n, int p) { return stf_align16((size_t)n * (p | 1) * 4); }
static inline __host__ __device__ size_t stf_mat_bytes(int p) { return stf_align16((size_t)p * (p | 1) * 8); }
static inline __host__ __device__ size_t stf_vec_bytes(int p) { return stf_align16((size_t)p * 8); }
// three fp32 tiles + two fp64 p x p matrices + two fp64 p-vectors
static inline size_t stf_lds_bytes(int n, int p) {
  return 3 * stf_tile_bytes(n, p) + 2 * stf_mat_bytes(p) + 2 * stf_vec_bytes(p);
}

// S[i][j] = sum_k a[k][i] b[k][j]   (i, j < p; k < n)
__device__ __forceinline__ void stf_atb(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ S,
                                        int n, int p, int pt, int ps) {
  const int tp = (p + 3) >> 2;
  for (int t = threadIdx.x; t < tp * tp; t += kStfThreads) {
    const int i0 = (t / tp) * 4, j0 = (t % tp) * 4;
    int ii[4], jj[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { ii[u] = min(i0 + u, p - 1); jj[u] = min(j0 + u, p - 1); }
    double acc[4][4] = {};
    for (int k = 0; k < n; ++k) {
      const float* ar = a + k * pt;
      const float* br = b + k * pt;
      double av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { av[u] = (double)ar[ii[u]]; bv[u] = (double)br[jj[u]]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fma(av[u], bv[v], acc[u][v]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (i0 + u < p && j0 + v < p) S[(i0 + u) * ps + j0 + v] = acc[u][v];
  }
}

// W = sym(S)
__device__ __forceinline__ void stf_sym(const double* __restrict__ S, double* __restrict__ W, int p, int ps) {
  for (int e = threadIdx.x; e < p * p; e += kStfThreads) {
    const int i = e / p, j = e - i * p;
    W[i * ps + j] = 0.5 * (S[i * ps + j] + S[j * ps + i]);
  }
}

// epi(i, j, sum_k a[i][k] W[k][j])   (i < n; j, k < p)
template <class Epi>
__device__ __forceinline__ void stf_aw(const float* __restrict__ a, const double* __restrict__ W, int n, int p, int pt,
                                       int ps, Epi epi) {
  const int tn = (n + 3) >> 2, tp = (p + 3) >> 2;
  for (int t = threadIdx.x; t < tn * tp; t += kStfThreads) {
    const int i0 = (t / tp) * 4, j0 = (t % tp) * 4;
    int ii[4], jj[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { ii[u] = min(i0 + u, n - 1) * pt; jj[u] = min(j0 + u, p - 1); }
    double acc[4][4] = {};
    for (int k = 0; k < p; ++k) {
      const double* wr = W + k * ps;
      double av[4], wv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { av[u] = (double)a[ii[u] + k]; wv[u] = wr[jj[u]]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fma(av[u], wv[v], acc[u][v]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (i0 + u < n && j0 + v < p) epi(i0 + u, j0 + v, acc[u][v]);
  }
}

// Q = Y R^-1 with Y^T Y = R^T R, diag(R) > 0.  Y and Q are distinct tiles.  Returns false (for every thread alike) when
// a pivot broke down; *spread = largest / smallest squared pivot.  Ends on a barrier.
__device__ bool stf_cholqr(const float* __restrict__ Y, float* __restrict__ Q, double* __restrict__ S,
                           double* __restrict__ W, double* __restrict__ d0, double* __restrict__ inv, int n, int p, int pt,
                           int ps, double* spread) {
  const int tid = threadIdx.x;
  stf_atb(Y, Y, S, n, p, pt, ps);
  __syncthreads();
  for (int k = tid; k < p; k += kStfThreads) d0[k] = S[k * ps + k];
  for (int e = tid; e < p * ps; e += kStfThreads) W[e] = 0.0;
  __syncthreads();
  double dmin = __builtin_huge_val(), dmax = 0.0;
  const int ti = tid >> 4, tj = tid & 15;
  for (int k = 0; k < p; ++k) {           // rows k of S become rows of R (strictly upper part; 1 / R[k][k] in inv)
    const double d = S[k * ps + k];
    if (!(d > d0[k] * kStfPivotFloor) || !(d < __builtin_huge_val())) return false;
    dmin = fmin(dmin, d);
    dmax = fmax(dmax, d);
    const double rinv = 1.0 / sqrt(d);
    for (int j = k + 1 + tid; j < p; j += kStfThreads) S[k * ps + j] *= rinv;
    if (tid == 0) inv[k] = rinv;
    __syncthreads();
    for (int i = k + 1 + ti; i < p; i += 16) {
      const double rki = S[k * ps + i];
      for (int j = k + 1 + tj; j < p; j += 16)
        if (j >= i) S[i * ps + j] = fma(-rki, S[k * ps + j], S[i * ps + j]);
    }
    __syncthreads();
  }
  // W = R^-1 (upper triangular, the rest stays zero), row by row from the bottom; four lanes share a column's sum
  const int col = tid >> 2, part = tid & 3;
  for (int i = p - 1; i >= 0; --i) {
    for (int jb = 0; jb < p; jb += kStfThreads / 4) {
      const int j = jb + col;
      double s = 0.0;
      if (j > i && j < p)
        for (int k = i + 1 + part; k <= j; k += 4) s = fma(S[i * ps + k], W[k * ps + j], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      if (part == 0 && j < p) {
        if (j == i) W[i * ps + i] = inv[i];
        else if (j > i) W[i * ps + j] = -inv[i] * s;
      }
    }
    __syncthreads();
  }
  stf_aw(Y, W, n, p, pt, ps, [&](int i, int j, double acc) { Q[i * pt + j] = (float)acc; });
  __syncthreads();
  *spread = dmax / dmin;
  return true;
}

// what the Adam instantiation needs on top of the SGD arguments; v, vmax, t hold one entry per factor in descriptor order
struct StfAdam {
  double b1, b2, eps;
  int amsgrad;
  float* v;
  float* vmax;
  int32_t* t;
};

// mode 0: one optimiser step, mode 1: project.  kAdam: the Adam step (always mode 0; mom, damp, nesterov unused).
template <bool kAdam>
__device__ __forceinline__ void stf_body(const tadmm_stiefel_desc* __restrict__ descs, int mode, double lr, double mom,
                                         double damp, double wd, int nesterov, const StfAdam& ad,
                                         int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const tadmm_stiefel_desc d = descs[blockIdx.x];
  const bool step = kAdam || mode == 0;
  if (step && !d.G) return;                 // no gradient this step: the factor is skipped
  const int tid = threadIdx.x;
  const int n = d.rows, p = d.cols, pt = p | 1, ps = p | 1;
  const int64_t ld = d.ld;
  float* tA = (float*)smem;
  float* tB = (float*)(smem + stf_tile_bytes(n, p));
  float* tC = (float*)(smem + 2 * stf_tile_bytes(n, p));
  double* S = (double*)(smem + 3 * stf_tile_bytes(n, p));
  double* W = (double*)((char*)S + stf_mat_bytes(p));
  double* d0 = (double*)((char*)W + stf_mat_bytes(p));
  double* inv = (double*)((char*)d0 + stf_vec_bytes(p));
  const bool use_m = kAdam || (step && mom > 0.0);
  // Adam: the factor's counter and bias corrections, read and computed while the tiles load
  int32_t tnew = 0;
  double c1 = 1.0, c2 = 1.0, vnew = 0.0, vtop = 0.0;
  if constexpr (kAdam) {
    tnew = ad.t[blockIdx.x] + 1;
    c1 = 1.0 - pow(ad.b1, (double)tnew);
    c2 = 1.0 - pow(ad.b2, (double)tnew);
  }

  float* Yt = tB;     // the matrix to orthonormalise
  float* Qt = tA;     // where its Q factor goes
  if (step) {
    for (int e = tid; e < n * p; e += kStfThreads) {
      const int i = e / p, j = e - i * p;
      const float x = d.X[i * ld + j];
      tA[i * pt + j] = x;
      tB[i * pt + j] = (float)fma(wd, (double)x, (double)d.G[i * ld + j]);
      if (use_m) tC[i * pt + j] = d.M[i * ld + j];
    }
    __syncthreads();
    stf_atb(tA, tB, S, n, p, pt, ps);
    __syncthreads();
    stf_sym(S, W, p, ps);
    __syncthreads();
    if constexpr (kAdam) {
      // the step's scale needs s = sum r^2 over the whole factor: the epilogue stores M' and keeps a partial sum, a
      // fixed-order reduction (butterfly in the wave, then the four waves in order) follows, one more pass forms Y
      const double keep = 1.0 - ad.b1;
      double part = 0.0;
      stf_aw(tA, W, n, p, pt, ps, [&](int i, int j, double acc) {
        const int o = i * pt + j;
        const double r = (double)tB[o] - acc;
        tC[o] = (float)fma(ad.b1, (double)tC[o], keep * r);
        part = fma(r, r, part);
      });
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
      __syncthreads();                      // W has been read: the four fp64 carves (>= 64 contiguous bytes) are free
      double* red = S;
      if ((tid & 63) == 0) red[tid >> 6] = part;
      __syncthreads();
      static_assert(kStfThreads == 4 * 64, "the reduction below adds four waves");
      const double s = ((red[0] + red[1]) + red[2]) + red[3];
      vnew = fma(ad.b2, (double)ad.v[blockIdx.x], (1.0 - ad.b2) * s);
      vtop = ad.amsgrad ? fmax((double)ad.vmax[blockIdx.x], vnew) : vnew;
      const double scale = lr / (c1 * (sqrt(vtop / c2) + ad.eps));
      for (int e = tid; e < n * p; e += kStfThreads) {
        const int o = (e / p) * pt + e % p;
        tB[o] = (float)fma(-scale, (double)tC[o], (double)tA[o]);
      }
      __syncthreads();
    } else {
      const double keep = 1.0 - damp;
      stf_aw(tA, W, n, p, pt, ps, [&](int i, int j, double acc) {
        const int o = i * pt + j;
        const double r = (double)tB[o] - acc;
        double dir = r;
        if (use_m) {
          const double m = fma(mom, (double)tC[o], keep * r);
          tC[o] = (float)m;
          dir = nesterov ? fma(mom, m, r) : m;
        }
        tB[o] = (float)fma(-lr, dir, (double)tA[o]);
      });
      __syncthreads();
    }
  } else {
    for (int e = tid; e < n * p; e += kStfThreads) {
      const int i = e / p, j = e - i * p;
      tB[i * pt + j] = d.X[i * ld + j];
    }
    __syncthreads();
  }

  double spread = 1.0;
  bool ok = stf_cholqr(Yt, Qt, S, W, d0, inv, n, p, pt, ps, &spread);
  if (ok && spread > kStfSecondPass) {
    ok = stf_cholqr(Qt, Yt, S, W, d0, inv, n, p, pt, ps, &spread);
    Qt = Yt;
  }
  if constexpr (kAdam) ok = ok && vnew >= 0.0 && vnew < __builtin_huge_val();     // a non-finite second moment fails too
  if (!ok) {
    if (tid == 0 && status) status[blockIdx.x] = 1;
    return;
  }
  if (use_m) {
    stf_atb(Qt, tC, S, n, p, pt, ps);
    __syncthreads();
    stf_sym(S, W, p, ps);
    __syncthreads();
    stf_aw(Qt, W, n, p, pt, ps, [&](int i, int j, double acc) {
      const int o = i * pt + j;
      tC[o] = (float)((double)tC[o] - acc);
    });
    __syncthreads();
  }
  for (int e = tid; e < n * p; e += kStfThreads) {
    const int i = e / p, j = e - i * p;
    d.X[i * ld + j] = Qt[i * pt + j];
    if (use_m) d.M[i * ld + j] = tC[i * pt + j];
  }
  if constexpr (kAdam) {
    if (tid == 0) {                         // written in the last phase, like X and M: a failed factor keeps them
      ad.v[blockIdx.x] = (float)vnew;
      if (ad.amsgrad) ad.vmax[blockIdx.x] = (float)vtop;
      ad.t[blockIdx.x] = tnew;
    }
  }
}

__global__ __launch_bounds__(kStfThreads) void stiefel_kernel(const tadmm_stiefel_desc* __restrict__ descs, int mode,
                                                              double lr, double mom, double damp, double wd, int nesterov,
                                                              int32_t* __restrict__ status) {
  stf_body<false>(descs, mode, lr, mom, damp, wd, nesterov, StfAdam{}, status);
}

__global__ __launch_bounds__(kStfThreads) void stiefel_adam_kernel(const tadmm_stiefel_desc* __restrict__ descs, double lr,
                                                                   double wd, StfAdam ad, int32_t* __restrict__ status) {
  stf_body<true>(descs, 0, lr, 0.0, 0.0, wd, 0, ad, status);
}

}  // namespace tadmm

using namespace tadmm;

struct tadmm_stiefel_plan_s {
  tadmm_handle h = nullptr;
  int n = 0;
  const tadmm_stiefel_desc* descs = nullptr;   // device copy, in the workspace
  size_t lds = 0;                               // of the largest factor
  bool has_m = true;                            // every factor carries a momentum buffer
};

namespace {

// checks every descriptor; *lds = dynamic LDS of the launch
int stiefel_check(tadmm_handle h, int n, const tadmm_stiefel_desc* descs, size_t* lds, bool* has_m) {
  if (n <= 0 || !descs) CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel: n = %d factors", n);
  size_t mx = 0;
  bool m = true;
  for (int i = 0; i < n; ++i) {
    const tadmm_stiefel_desc& d = descs[i];
    if (!d.X) CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel factor %d: X is NULL", i);
    if (d.cols <= 0 || d.rows < d.cols)
      CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel factor %d: shape %d x %d, need rows >= cols >= 1", i, d.rows, d.cols);
    if (d.ld < d.cols) CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel factor %d: ld %lld < cols %d", i, (long long)d.ld, d.cols);
    if ((((uintptr_t)d.X) | ((uintptr_t)d.G) | ((uintptr_t)d.M)) & 3)
      CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel factor %d: misaligned pointer", i);
    // (the fp64 matrices alone pass the budget beyond 100 columns: checked first, the sizes below cannot overflow)
    if (d.cols > 128 || d.rows > (1 << 20) || stf_lds_bytes(d.rows, d.cols) > kStfMaxLds)
      CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "stiefel factor %d: %d x %d does not fit the LDS-resident step (%zu bytes)", i,
               d.rows, d.cols, kStfMaxLds);
    mx = std::max(mx, stf_lds_bytes(d.rows, d.cols));
    m = m && d.M != nullptr;
  }
  *lds = mx;
  if (has_m) *has_m = m;
  return TADMM_OK;
}

int stiefel_launch(tadmm_stiefel_plan p, int mode, double lr, double mom, double damp, double wd, int nesterov,
                   int32_t* status, hipStream_t s) {
  tadmm_handle h = p->h;
  static DynLdsOptIn allow_lds;
  HIP_OK(h, allow_lds(stiefel_kernel, kStfMaxLds));
  hipLaunchKernelGGL(stiefel_kernel, dim3(p->n), dim3(kStfThreads), p->lds, s, p->descs, mode, lr, mom, damp, wd,
                     nesterov, status);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int stiefel_adam_launch(tadmm_stiefel_plan p, double lr, double wd, const StfAdam& ad, int32_t* status, hipStream_t s) {
  tadmm_handle h = p->h;
  static DynLdsOptIn allow_lds;
  HIP_OK(h, allow_lds(stiefel_adam_kernel, kStfMaxLds));
  hipLaunchKernelGGL(stiefel_adam_kernel, dim3(p->n), dim3(kStfThreads), p->lds, s, p->descs, lr, wd, ad, status);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // namespace

extern "C" {

int tadmm_stiefel_desc_bytes(void) { return (int)sizeof(tadmm_stiefel_desc); }

int tadmm_stiefel_workspace_bytes(int n, const tadmm_stiefel_desc* descs, size_t* bytes) {
  if (!bytes) return TADMM_ERR_INVALID;
  size_t lds = 0;
  const int rc = stiefel_check(nullptr, n, descs, &lds, nullptr);
  if (rc != TADMM_OK) return rc;
  *bytes = align_up((size_t)n * sizeof(tadmm_stiefel_desc), 256);
  return TADMM_OK;
}

int tadmm_stiefel_plan_create(tadmm_handle h, int n, const tadmm_stiefel_desc* descs, void* workspace,
                              size_t workspace_bytes, void* stream, tadmm_stiefel_plan* out) {
  DeviceGuard device_guard(h);
  if (!h || !out) return TADMM_ERR_INVALID;
  *out = nullptr;
  size_t lds = 0;
  bool has_m = true;
  const int rc = stiefel_check(h, n, descs, &lds, &has_m);
  if (rc != TADMM_OK) return rc;
  const size_t need = align_up((size_t)n * sizeof(tadmm_stiefel_desc), 256);
  if (!workspace || workspace_bytes < need)
    CTX_FAIL(h, TADMM_ERR_WORKSPACE, "stiefel workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
  // on the caller's stream, synchronous because the caller's array may die at return (as tadmm_orth_plan_create)
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(workspace, descs, (size_t)n * sizeof(tadmm_stiefel_desc), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) CTX_FAIL(h, TADMM_ERR_HIP, "stiefel table upload failed: %s", hipGetErrorString(e));
  tadmm_stiefel_plan_s* P = new tadmm_stiefel_plan_s;
  P->h = h; P->n = n; P->descs = (const tadmm_stiefel_desc*)workspace; P->lds = lds; P->has_m = has_m;
  *out = P;
  return TADMM_OK;
}

int tadmm_stiefel_step(tadmm_stiefel_plan p, double lr, double momentum, double dampening, double weight_decay,
                       int nesterov, int32_t* status_dev, void* stream) {
  if (!p) return TADMM_ERR_INVALID;
  tadmm_handle h = p->h;
  DeviceGuard device_guard(h);
  if (!(momentum >= 0.0)) CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel step: momentum %g < 0", momentum);
  if (momentum > 0.0 && !p->has_m)
    CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel step: momentum %g needs a momentum buffer for every factor", momentum);
  return stiefel_launch(p, 0, lr, momentum, dampening, weight_decay, nesterov ? 1 : 0, status_dev, (hipStream_t)stream);
}

int tadmm_stiefel_adam_step(tadmm_stiefel_plan p, double lr, double beta1, double beta2, double eps, double weight_decay,
                            int amsgrad, float* v_dev, float* vmax_dev, int32_t* step_dev, int32_t* status_dev,
                            void* stream) {
  if (!p) return TADMM_ERR_INVALID;
  tadmm_handle h = p->h;
  DeviceGuard device_guard(h);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
    CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel adam step: betas (%g, %g) outside [0, 1)", beta1, beta2);
  if (!(eps >= 0.0) || !(lr >= 0.0) || !(weight_decay >= 0.0))
    CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel adam step: eps %g, lr %g, weight_decay %g must not be negative", eps, lr,
             weight_decay);
  if (!v_dev || !step_dev) CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel adam step: v_dev or step_dev is NULL");
  if (amsgrad && !vmax_dev) CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel adam step: amsgrad needs vmax_dev");
  if (!p->has_m) CTX_FAIL(h, TADMM_ERR_INVALID, "stiefel adam step: every factor needs M (exp_avg)");
  const StfAdam ad = {beta1, beta2, eps, amsgrad ? 1 : 0, v_dev, vmax_dev, step_dev};
  return stiefel_adam_launch(p, lr, weight_decay, ad, status_dev, (hipStream_t)stream);
}

int tadmm_stiefel_project(tadmm_stiefel_plan p, int32_t* status_dev, void* stream) {
  if (!p) return TADMM_ERR_INVALID;
  DeviceGuard device_guard(p->h);
  return stiefel_launch(p, 1, 0.0, 0.0, 0.0, 0.0, 0, status_dev, (hipStream_t)stream);
}

int tadmm_stiefel_plan_destroy(tadmm_stiefel_plan p) {
  delete p;
  return TADMM_OK;
}

}  // extern "C"
