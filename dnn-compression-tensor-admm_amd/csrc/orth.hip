// Orthogonality regulariser of the Tucker / SVD factors (the reference's orthogonal.py: append_double_l2_loss).
//
// For every factor P_i (squeezed to a rows x cols matrix) with Gram G_i over its long side,
//     E_i = G_i - I,     loss += 0.5 * rho * ||E_i||_F^2,     grad_i = 2 rho E_i P_i   (G_i = P_i P_i^T)
//                                                              grad_i = 2 rho P_i E_i   (G_i = P_i^T P_i)
// One call covers every factor of a model in at most four grouped launches:
//   1. gram_partial_kernel (gram.hip)  exact fp32 products accumulated in fp64 on v_mfma_f64_16x16x4, split-K
//   2. gram_reduce_kernel  (gram.hip)  fixed-order sum of the split-K partials (only when some factor is split)
//   3. orth_tile_kernel                one workgroup per 32 x 32 tile of every grad_i: E = G - I in fp64, the E P /
//                                      P E product on the fp64 matrix cores, rounded to fp32 once; the workgroups of
//                                      the first long-side tile column also emit the fp64 sum of E^2 over their 32
//                                      rows of E (each entry of E is counted by exactly one workgroup)
//   4. orth_reduce_kernel              fixed-order sum of those row-block sums into loss_dev[0]
// Every table the launches read is uploaded once, when the plan is created; a call copies nothing.  No floating-point
// atomics anywhere: the results are bitwise reproducible from call to call.
//
// MFMA operand maps (cdna_hip_programming.md section 3; the f64 form as in gram.hip): A operand lane l holds
// A[i=l&15][k=l>>4], B operand lane l holds B[k=l>>4][j=l&15]; D: col = l&15, row = (l>>4) + 4*reg.
//   gram of rows (G = P P^T, P is N x K):  D[a][t] = sum_b E[a][b] P[b][t]   A = E, B = P
//   gram of cols (G = P^T P, P is K x N):  D[t][a] = sum_b P[t][b] E[b][a]   A = P, B = E
// E is symmetric, so in both cases the E operand of lane (r = l&15, q = l>>4) at step b0 is E[b0+q][a0+r]: a
// contiguous row segment of the Gram image.
#include "host.h"

namespace tadmm {

typedef double double4_t __attribute__((ext_vector_type(4)));

struct OrthProb {
  const float* P; int64_t ld;   // P[i * ld + j], i < rows, j < cols
  const double* G; int32_t ldg; // Gram image [Npad][ldg], zero padded beyond N
  int32_t rows, cols;           // squeezed shape; the gradient is contiguous rows x cols
  int32_t of_rows;              // 1: G = P P^T (N = rows, K = cols) ; 0: G = P^T P (N = cols, K = rows)
  int32_t N, K, nt, tk;         // Gram size, long side, 32-tiles along N, 32-tiles along K
  int32_t slot;                 // first of the nt row-block sums of ||E||^2
  int64_t goff;                 // element offset of the gradient in the call's buffer, < 0: none
};

__device__ __forceinline__ double orth_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void orth_tile_kernel(const OrthProb* __restrict__ probs,
                                                        const BlockRef* __restrict__ map, float* __restrict__ grad,
                                                        double rho, double* __restrict__ slots) {
  __shared__ double red[4];
  const BlockRef br = map[blockIdx.x];
  const OrthProb d = probs[br.prob];
  const int ta = br.local / d.tk, tb = br.local - ta * d.tk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;

  if (tb == 0) {   // ||E||^2 over rows [32 ta, 32 ta + 32) of E, fixed order
    const int a0 = ta * 32;
    const int na = min(32, d.N - a0);
    double acc = 0.0;
    for (int i = wave; i < na; i += 4) {
      const double* row = d.G + (int64_t)(a0 + i) * d.ldg;
      for (int j = lane; j < d.N; j += 64) {
        const double v = row[j] - (a0 + i == j ? 1.0 : 0.0);
        acc += v * v;
      }
    }
    acc = orth_wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) slots[d.slot + ta] = (red[0] + red[1]) + (red[2] + red[3]);
  }
  if (!grad || d.goff < 0) return;

  // this wave's 16 x 16 quadrant of the tile: Gram indices a0.., long-side indices t0..
  const int a0 = ta * 32 + (wave & 1) * 16;
  const int t0 = tb * 32 + (wave >> 1) * 16;
  const int Npad = d.nt * 32;
  const int N = d.N, K = d.K;
  const int64_t ld = d.ld;
  const int t = t0 + r;
  const bool tok = t < K;
  const int64_t tl = min(t, K - 1);
  const double* __restrict__ Ecol = d.G + a0 + r;   // E[b][a0+r] = G[b][a0+r] - delta
  const float* __restrict__ P = d.P;
  const bool rows = d.of_rows != 0;
  double4_t acc = {0, 0, 0, 0};
  // eight k-steps per round: the 16 loads of a round are independent and are issued before its MFMAs
  for (int b0 = 0; b0 < Npad; b0 += 32) {
    double e[8], p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = b0 + 4 * u + q;
      const int64_t bl = min(b, N - 1);
      e[u] = Ecol[(int64_t)b * d.ldg];
      const float v = rows ? P[bl * ld + tl] : P[tl * ld + bl];
      p[u] = (tok && b < N) ? (double)v : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = b0 + 4 * u + q;
      const double eu = e[u] - ((b == a0 + r && b < N) ? 1.0 : 0.0);
      acc = rows ? __builtin_amdgcn_mfma_f64_16x16x4f64(eu, p[u], acc, 0, 0, 0)
                 : __builtin_amdgcn_mfma_f64_16x16x4f64(p[u], eu, acc, 0, 0, 0);
    }
  }
  const double s = 2.0 * rho;
  float* __restrict__ g = grad + d.goff;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = q + 4 * reg;
    if (rows) {                                      // D[a][t] -> grad[a][t], N x K
      const int a = a0 + row, tt = t0 + r;
      if (a < N && tt < K) g[(int64_t)a * d.cols + tt] = (float)(s * acc[reg]);
    } else {                                         // D[t][a] -> grad[t][a], K x N
      const int tt = t0 + row, a = a0 + r;
      if (tt < K && a < N) g[(int64_t)tt * d.cols + a] = (float)(s * acc[reg]);
    }
  }
}

__global__ __launch_bounds__(64) void orth_reduce_kernel(int nslots, double rho, const double* __restrict__ slots,
                                                         double* __restrict__ loss) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nslots; i += 64) acc += slots[i];
  acc = orth_wave_sum(acc);
  if (threadIdx.x == 0) loss[0] += 0.5 * rho * acc;
}

}  // namespace tadmm

using namespace tadmm;

struct tadmm_orth_plan_s {
  tadmm_handle h = nullptr;
  int n = 0;
  const GramDesc* gram = nullptr;
  const BlockRef* map_p = nullptr; int nb_p = 0;
  const BlockRef* map_r = nullptr; int nb_r = 0;
  const OrthProb* probs = nullptr;
  const BlockRef* map_t = nullptr; int nb_t = 0;   // every tile of a factor with a gradient, column 0 of the others
  const BlockRef* map_n = nullptr; int nb_n = 0;   // column 0 of every factor: the calls without a gradient buffer
  double* slots = nullptr; int nslots = 0;
};

namespace {

struct OrthGeom {
  int N = 0, K = 0, Npad = 0, nt = 0, tk = 0, ksplit = 1, kchunk = 0;
};

int orth_geom(tadmm_handle h, int i, const tadmm_orth_desc& d, OrthGeom& g) {
  if (!d.P || d.rows <= 0 || d.cols <= 0)
    CTX_FAIL(h, TADMM_ERR_INVALID, "orth factor %d: null pointer or empty shape %d x %d", i, d.rows, d.cols);
  if (d.ld < d.cols || (((uintptr_t)d.P) & 3))
    CTX_FAIL(h, TADMM_ERR_INVALID, "orth factor %d: ld %lld < cols %d or misaligned pointer", i, (long long)d.ld,
             d.cols);
  if (d.ld > INT32_MAX || (int64_t)(d.rows - 1) * d.ld + d.cols > INT32_MAX)
    CTX_FAIL(h, TADMM_ERR_INVALID, "orth factor %d: spans more than 2^31 elements", i);
  g.N = d.gram_of_rows ? d.rows : d.cols;
  g.K = d.gram_of_rows ? d.cols : d.rows;
  if (g.N > kJacobiMaxN)
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "orth factor %d: Gram of size %d exceeds %d", i, g.N, kJacobiMaxN);
  g.nt = (g.N + 31) / 32;
  g.Npad = 32 * g.nt;
  g.tk = (g.K + 31) / 32;
  // split-K as the projection plans batch their Grams (plan.hip): >= 64 workgroups per factor where the reduction is
  // long enough, chunks of at most 2048
  const int ntp = g.nt * (g.nt + 1) / 2;
  int ks = (64 + ntp - 1) / ntp;
  ks = std::max(1, std::min(ks, (g.K + 255) / 256));
  ks = std::max(ks, (g.K + 2047) / 2048);
  g.kchunk = (int)align_up((g.K + ks - 1) / ks, 64);
  g.ksplit = (g.K + g.kchunk - 1) / g.kchunk;
  return TADMM_OK;
}

// Workspace layout, sized (base == nullptr) and filled by the same walk.  `img` receives the host image of the table
// part (everything below the first Gram buffer).
int orth_layout(tadmm_handle h, int n, const tadmm_orth_desc* descs, char* base, size_t* bytes,
                std::vector<char>* img, tadmm_orth_plan_s* P) {
  if (n <= 0 || !descs) CTX_FAIL(h, TADMM_ERR_INVALID, "orth: n = %d factors", n);
  std::vector<OrthGeom> geo(n);
  size_t np = 0, nr = 0, ntile = 0, nslots = 0;   // nslots: row blocks = tiles of the norm-only map
  for (int i = 0; i < n; ++i) {
    const int rc = orth_geom(h, i, descs[i], geo[i]);
    if (rc != TADMM_OK) return rc;
    const OrthGeom& g = geo[i];
    np += (size_t)g.ksplit * g.nt * (g.nt + 1) / 2;
    if (g.ksplit > 1) nr += ((size_t)g.Npad * g.Npad + 1023) / 1024;
    ntile += (size_t)g.nt * (descs[i].grad_offset >= 0 ? g.tk : 1);
    nslots += g.nt;
  }
  if (np > INT32_MAX / 2 || ntile > INT32_MAX / 2) CTX_FAIL(h, TADMM_ERR_INVALID, "orth: too many workgroups");
  Arena a;
  const size_t o_gram = a.take(n * sizeof(GramDesc));
  const size_t o_mp = a.take(np * sizeof(BlockRef));
  const size_t o_mr = a.take(nr * sizeof(BlockRef));
  const size_t o_pr = a.take(n * sizeof(OrthProb));
  const size_t o_mt = a.take(ntile * sizeof(BlockRef));
  const size_t o_mn = a.take(nslots * sizeof(BlockRef));
  const size_t table_end = a.off;
  const size_t o_sl = a.take(nslots * sizeof(double));
  std::vector<size_t> o_part(n), o_g(n);
  for (int i = 0; i < n; ++i) {
    const OrthGeom& g = geo[i];
    o_part[i] = g.ksplit > 1 ? a.take((size_t)g.ksplit * g.nt * (g.nt + 1) / 2 * 1024 * sizeof(double)) : 0;
    o_g[i] = a.take((size_t)g.Npad * g.Npad * sizeof(double));
  }
  *bytes = align_up(a.off, 256);
  if (!base) return TADMM_OK;

  img->assign(table_end, 0);
  char* I = img->data();
  GramDesc* gd = (GramDesc*)(I + o_gram);
  BlockRef* mp = (BlockRef*)(I + o_mp);
  BlockRef* mr = (BlockRef*)(I + o_mr);
  OrthProb* pr = (OrthProb*)(I + o_pr);
  BlockRef* mt = (BlockRef*)(I + o_mt);
  BlockRef* mn = (BlockRef*)(I + o_mn);
  size_t ip = 0, ir = 0, it = 0, in = 0;
  int slot = 0;
  for (int i = 0; i < n; ++i) {
    const OrthGeom& g = geo[i];
    const tadmm_orth_desc& d = descs[i];
    GramDesc& q = gd[i];
    q.A = d.P;
    q.m = d.rows;
    q.n = (int32_t)d.ld;           // the Gram kernels address A with a row stride of `n`
    q.trans = d.gram_of_rows ? 0 : 1;
    q.N = g.N; q.K = g.K; q.nt = g.nt; q.ksplit = g.ksplit; q.kchunk = g.kchunk;
    q.partial = g.ksplit > 1 ? (double*)(base + o_part[i]) : nullptr;
    q.G = (double*)(base + o_g[i]);
    q.Npad = g.Npad; q.ld = g.Npad;   // no padding columns: ld == Npad
    const int nblk_p = g.ksplit * g.nt * (g.nt + 1) / 2;
    for (int b = 0; b < nblk_p; ++b) mp[ip++] = BlockRef{i, b};
    if (g.ksplit > 1)
      for (int b = 0; b < (int)(((size_t)g.Npad * g.Npad + 1023) / 1024); ++b) mr[ir++] = BlockRef{i, b};
    OrthProb& o = pr[i];
    o.P = d.P; o.ld = d.ld; o.G = q.G; o.ldg = g.Npad;
    o.rows = d.rows; o.cols = d.cols; o.of_rows = d.gram_of_rows ? 1 : 0;
    o.N = g.N; o.K = g.K; o.nt = g.nt; o.tk = g.tk;
    o.slot = slot; slot += g.nt;
    o.goff = d.grad_offset;
    for (int ta = 0; ta < g.nt; ++ta) {          // local block = ta * tk + tb
      mn[in++] = BlockRef{i, ta * g.tk};
      for (int tb = 0; tb < (d.grad_offset >= 0 ? g.tk : 1); ++tb) mt[it++] = BlockRef{i, ta * g.tk + tb};
    }
  }
  P->n = n;
  P->gram = (const GramDesc*)(base + o_gram);
  P->map_p = (const BlockRef*)(base + o_mp); P->nb_p = (int)np;
  P->map_r = (const BlockRef*)(base + o_mr); P->nb_r = (int)nr;
  P->probs = (const OrthProb*)(base + o_pr);
  P->map_t = (const BlockRef*)(base + o_mt); P->nb_t = (int)ntile;
  P->map_n = (const BlockRef*)(base + o_mn); P->nb_n = (int)nslots;
  P->slots = (double*)(base + o_sl); P->nslots = (int)nslots;
  return TADMM_OK;
}

}  // namespace

extern "C" {

int tadmm_orth_desc_bytes(void) { return (int)sizeof(tadmm_orth_desc); }

int tadmm_orth_workspace_bytes(int n, const tadmm_orth_desc* descs, size_t* bytes) {
  if (!bytes) return TADMM_ERR_INVALID;
  return orth_layout(nullptr, n, descs, nullptr, bytes, nullptr, nullptr);
}

int tadmm_orth_plan_create(tadmm_handle h, int n, const tadmm_orth_desc* descs, void* workspace,
                           size_t workspace_bytes, void* stream, tadmm_orth_plan* out) {
  DeviceGuard device_guard(h);
  if (!h || !out) return TADMM_ERR_INVALID;
  *out = nullptr;
  size_t need = 0;
  int rc = orth_layout(h, n, descs, nullptr, &need, nullptr, nullptr);
  if (rc != TADMM_OK) return rc;
  if (!workspace || workspace_bytes < need)
    CTX_FAIL(h, TADMM_ERR_WORKSPACE, "orth workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
  tadmm_orth_plan_s* P = new tadmm_orth_plan_s;
  P->h = h;
  std::vector<char> img;
  rc = orth_layout(h, n, descs, (char*)workspace, &need, &img, P);
  if (rc != TADMM_OK) { delete P; return rc; }
  // on the caller's stream: the workspace may be memory that work queued there has just released; synchronous
  // because the host image dies at return
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(workspace, img.data(), img.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { delete P; CTX_FAIL(h, TADMM_ERR_HIP, "orth table upload failed: %s", hipGetErrorString(e)); }
  *out = P;
  return TADMM_OK;
}

int tadmm_orth_l2(tadmm_orth_plan p, double rho, float* grad, double* loss_dev, void* stream_) {
  if (!p) return TADMM_ERR_INVALID;
  tadmm_handle h = p->h;
  DeviceGuard device_guard(h);
  if (!loss_dev) CTX_FAIL(h, TADMM_ERR_INVALID, "orth: loss_dev is NULL");
  hipStream_t s = (hipStream_t)stream_;
  launch_gram_partial(p->gram, p->map_p, p->nb_p, s);
  launch_gram_reduce(p->gram, p->map_r, p->nb_r, s);   // no blocks (no launch) when no factor is split
  hipLaunchKernelGGL(orth_tile_kernel, dim3(grad ? p->nb_t : p->nb_n), dim3(256), 0, s, p->probs,
                     grad ? p->map_t : p->map_n, grad, rho, p->slots);
  hipLaunchKernelGGL(orth_reduce_kernel, dim3(1), dim3(64), 0, s, p->nslots, rho, (const double*)p->slots, loss_dev);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_orth_plan_destroy(tadmm_orth_plan p) {
  delete p;
  return TADMM_OK;
}

}  // extern "C"
