// BertAdam (the reference's xcompression/transformer/optimization.py:183-302, the optimiser of every xcompression
// training script): per-tensor gradient clipping, an Adam update without bias correction and decoupled weight decay, for
// ALL tensors of a param group in two launches.
//
// A plan holds a device table of n tensors (p, g, m, v, numel; float32, dense, 4-byte aligned) and a map that cuts them
// into chunks of kBaChunk elements, a chunk never spanning two tensors.  A workgroup takes chunks b, b + grid, ...
//   A. bertadam_norm_kernel     (only with max_grad_norm > 0)  partial[b] = sum of g^2 over chunk b: products and sums in
//                               double, per-lane sums, a wave butterfly, four wave sums through LDS, ONE double stored per
//                               chunk.  No atomics.
//   B. bertadam_update_kernel   a workgroup sums the partials of its chunk's tensor -- lane i takes partials i, i + 256,
//                               ... in ascending order, then the same butterfly: a fixed order that depends on the tensor
//                               alone, so every chunk of a tensor holds the same bits --, forms
//                                   norm = sqrt(sum),   c = (float) min(1, max_grad_norm / (norm + 1e-6))
//                               (c = 1 without clipping) and updates its chunk in float32, every operation rounded on its
//                               own as the reference's tensor operations are (no contraction into fma):
//                                   gc = g c;   m = b1 m + (1-b1) gc;   v = b2 v + (1-b2) gc gc
//                                   u = m / (sqrtf(v) + e);   u += weight_decay p  (weight_decay > 0);   p -= lr u
//                               m, v and p are stored once; g is only read (the reference scales .grad in place; this does
//                               not).  The first chunk of a tensor stores norm into the plan's per-tensor double array.
// The launches are ordered by the stream; no workgroup waits for another.  Non-finite values follow IEEE: an inf in g gives
// norm = inf, c = 0 and NaN at that element only; a NaN in g gives c = NaN (as torch's clamp) and a NaN tensor.  Nothing
// depends on the order workgroups run in: bitwise reproducible.
// Accesses: 16 bytes per lane where the tensor's four bases are 16-byte aligned (kBaChunk is a multiple of 4, so every
// chunk of such a tensor starts aligned), chosen per tensor on the host; single elements for the other tensors and for
// the last numel % 4 elements.
#include "host.h"

namespace tadmm {

constexpr int kBaThreads = 256;
constexpr int kBaChunk = 4096;        // elements: four 16-byte accesses per lane and array
constexpr int kBaGridCap = 2048;      // 8 workgroups per CU; the chunks beyond are taken by a stride loop

struct BaTensor {
  float* p; const float* g; float* m; float* v;
  int64_t n;
  int32_t first, nchunks;             // its chunks are first .. first + nchunks - 1 of the map
  int32_t g_vec, all_vec;             // g / all four bases are 16-byte aligned
};
struct BaChunkRef { int32_t tensor, index; };

struct BaHyper {
  float lr, b1, omb1, b2, omb2, e, wd;
  int32_t clip, decay;
  double max_norm;
};

__device__ __forceinline__ double ba_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the sum over the workgroup, the same bits in every lane; red: kBaThreads / 64 doubles, reusable after the call
__device__ __forceinline__ double ba_block_sum(double v, double* red) {
  v = ba_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kBaThreads) void bertadam_norm_kernel(const BaTensor* __restrict__ tens,
                                                                   const BaChunkRef* __restrict__ map, int nchunks,
                                                                   double* __restrict__ partial) {
  __shared__ double red[kBaThreads / 64];
  const int tid = threadIdx.x;
  for (int b = blockIdx.x; b < nchunks; b += gridDim.x) {
    const BaChunkRef r = map[b];
    const BaTensor t = tens[r.tensor];
    const int64_t off = (int64_t)r.index * kBaChunk;
    const int len = (int)min((int64_t)kBaChunk, t.n - off);
    const float* __restrict__ g = t.g + off;
    double acc = 0.0;
    int done = 0;
    if (t.g_vec) {
      done = len & ~3;
      for (int i = tid * 4; i < done; i += kBaThreads * 4) {
        const float4 x = *reinterpret_cast<const float4*>(g + i);
        acc += (double)x.x * (double)x.x;
        acc += (double)x.y * (double)x.y;
        acc += (double)x.z * (double)x.z;
        acc += (double)x.w * (double)x.w;
      }
    }
    for (int i = done + tid; i < len; i += kBaThreads) acc += (double)g[i] * (double)g[i];
    const double s = ba_block_sum(acc, red);
    if (tid == 0) partial[b] = s;
  }
}

__device__ __forceinline__ void ba_elem(float& p, float g, float& m, float& v, float c, const BaHyper& h) {
#pragma clang fp contract(off)
  const float gc = g * c;
  m = h.b1 * m + h.omb1 * gc;
  v = h.b2 * v + h.omb2 * gc * gc;
  float u = m / (sqrtf(v) + h.e);
  if (h.decay) u += h.wd * p;
  p -= h.lr * u;
}

__device__ __forceinline__ void ba_elem4(float4& p, const float4& g, float4& m, float4& v, float c, const BaHyper& h) {
  ba_elem(p.x, g.x, m.x, v.x, c, h);
  ba_elem(p.y, g.y, m.y, v.y, c, h);
  ba_elem(p.z, g.z, m.z, v.z, c, h);
  ba_elem(p.w, g.w, m.w, v.w, c, h);
}

__global__ __launch_bounds__(kBaThreads) void bertadam_update_kernel(const BaTensor* __restrict__ tens,
                                                                     const BaChunkRef* __restrict__ map, int nchunks,
                                                                     const double* __restrict__ partial,
                                                                     double* __restrict__ norms, BaHyper h) {
  __shared__ double red[kBaThreads / 64];
  const int tid = threadIdx.x;
  int last = -1;
  float c = 1.f;
  for (int b = blockIdx.x; b < nchunks; b += gridDim.x) {
    const BaChunkRef r = map[b];
    const BaTensor t = tens[r.tensor];
    if (h.clip && r.tensor != last) {      // (a workgroup meets a tensor's chunk 0 before any other chunk of it)
      last = r.tensor;
      double acc = 0.0;
      for (int i = tid; i < t.nchunks; i += kBaThreads) acc += partial[t.first + i];
      const double norm = sqrt(ba_block_sum(acc, red));
      const double x = h.max_norm / (norm + 1e-6);
      c = (float)(x > 1.0 ? 1.0 : x);      // a NaN stays a NaN
      if (r.index == 0 && tid == 0) norms[r.tensor] = norm;
    }
    const int64_t off = (int64_t)r.index * kBaChunk;
    const int len = (int)min((int64_t)kBaChunk, t.n - off);
    float* __restrict__ p = t.p + off;
    const float* __restrict__ g = t.g + off;
    float* __restrict__ m = t.m + off;
    float* __restrict__ v = t.v + off;
    int done = 0;
    if (t.all_vec && len == kBaChunk) {
      // a whole chunk: the sixteen loads of a lane go out before the first use
      constexpr int kIt = kBaChunk / (kBaThreads * 4);
      float4 P[kIt], G[kIt], M[kIt], V[kIt];
#pragma unroll
      for (int k = 0; k < kIt; ++k) {
        const int i = (k * kBaThreads + tid) * 4;
        G[k] = *reinterpret_cast<const float4*>(g + i);
        M[k] = *reinterpret_cast<const float4*>(m + i);
        V[k] = *reinterpret_cast<const float4*>(v + i);
        P[k] = *reinterpret_cast<const float4*>(p + i);
      }
#pragma unroll
      for (int k = 0; k < kIt; ++k) {
        const int i = (k * kBaThreads + tid) * 4;
        ba_elem4(P[k], G[k], M[k], V[k], c, h);
        *reinterpret_cast<float4*>(m + i) = M[k];
        *reinterpret_cast<float4*>(v + i) = V[k];
        *reinterpret_cast<float4*>(p + i) = P[k];
      }
      continue;
    }
    if (t.all_vec) {
      done = len & ~3;
      for (int i = tid * 4; i < done; i += kBaThreads * 4) {
        const float4 G = *reinterpret_cast<const float4*>(g + i);
        float4 M = *reinterpret_cast<const float4*>(m + i);
        float4 V = *reinterpret_cast<const float4*>(v + i);
        float4 P = *reinterpret_cast<const float4*>(p + i);
        ba_elem4(P, G, M, V, c, h);
        *reinterpret_cast<float4*>(m + i) = M;
        *reinterpret_cast<float4*>(v + i) = V;
        *reinterpret_cast<float4*>(p + i) = P;
      }
    }
    for (int i = done + tid; i < len; i += kBaThreads) {
      float P = p[i], M = m[i], V = v[i];
      ba_elem(P, g[i], M, V, c, h);
      m[i] = M;
      v[i] = V;
      p[i] = P;
    }
  }
}

}  // namespace tadmm

using namespace tadmm;

struct tadmm_bertadam_plan_s {
  tadmm_handle h = nullptr;
  int n = 0, nchunks = 0;
  const BaTensor* tens = nullptr;      // the four arrays live in the caller's workspace
  const BaChunkRef* map = nullptr;
  double* partial = nullptr;           // [nchunks]
  double* norms = nullptr;             // [n]
};

namespace {

struct BaLayout { size_t tens = 0, map = 0, partial = 0, norms = 0, bytes = 0; int64_t nchunks = 0; };

// checks every descriptor and places the four arrays
int bertadam_layout(tadmm_handle h, int n, const tadmm_bertadam_desc* descs, BaLayout* out) {
  if (n <= 0 || !descs) CTX_FAIL(h, TADMM_ERR_INVALID, "bertadam: n = %d tensors", n);
  int64_t nchunks = 0;
  for (int i = 0; i < n; ++i) {
    const tadmm_bertadam_desc& d = descs[i];
    if (!d.p || !d.g || !d.m || !d.v) CTX_FAIL(h, TADMM_ERR_INVALID, "bertadam tensor %d: NULL pointer", i);
    if ((((uintptr_t)d.p) | ((uintptr_t)d.g) | ((uintptr_t)d.m) | ((uintptr_t)d.v)) & 3)
      CTX_FAIL(h, TADMM_ERR_INVALID, "bertadam tensor %d: misaligned pointer", i);
    if (d.n <= 0) CTX_FAIL(h, TADMM_ERR_INVALID, "bertadam tensor %d: numel %lld", i, (long long)d.n);
    nchunks += (d.n + kBaChunk - 1) / kBaChunk;
    if (nchunks > INT32_MAX) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "bertadam: more than 2^31 chunks of %d elements", kBaChunk);
  }
  Arena a;
  out->tens = a.take((size_t)n * sizeof(BaTensor));
  out->map = a.take((size_t)nchunks * sizeof(BaChunkRef));
  out->partial = a.take((size_t)nchunks * sizeof(double));
  out->norms = a.take((size_t)n * sizeof(double));
  out->bytes = align_up(a.off, 256);
  out->nchunks = nchunks;
  return TADMM_OK;
}

}  // namespace

extern "C" {

int tadmm_bertadam_desc_bytes(void) { return (int)sizeof(tadmm_bertadam_desc); }

int tadmm_bertadam_chunk(void) { return kBaChunk; }

int tadmm_bertadam_workspace_bytes(int n, const tadmm_bertadam_desc* descs, size_t* bytes) {
  if (!bytes) return TADMM_ERR_INVALID;
  BaLayout l;
  const int rc = bertadam_layout(nullptr, n, descs, &l);
  if (rc != TADMM_OK) return rc;
  *bytes = l.bytes;
  return TADMM_OK;
}

int tadmm_bertadam_plan_create(tadmm_handle h, int n, const tadmm_bertadam_desc* descs, void* workspace,
                               size_t workspace_bytes, void* stream, tadmm_bertadam_plan* out) {
  DeviceGuard device_guard(h);
  if (!h || !out) return TADMM_ERR_INVALID;
  *out = nullptr;
  BaLayout l;
  const int rc = bertadam_layout(h, n, descs, &l);
  if (rc != TADMM_OK) return rc;
  if (!workspace || workspace_bytes < l.bytes)
    CTX_FAIL(h, TADMM_ERR_WORKSPACE, "bertadam workspace too small: need %zu bytes, got %zu", l.bytes, workspace_bytes);
  if ((uintptr_t)workspace & 15) CTX_FAIL(h, TADMM_ERR_INVALID, "bertadam workspace must be 16-byte aligned");
  // the table and the map, one host image, one upload
  const size_t image = l.map + (size_t)l.nchunks * sizeof(BaChunkRef);
  std::vector<char> img(image, 0);
  BaTensor* tens = reinterpret_cast<BaTensor*>(img.data() + l.tens);
  BaChunkRef* map = reinterpret_cast<BaChunkRef*>(img.data() + l.map);
  int32_t first = 0;
  for (int i = 0; i < n; ++i) {
    const tadmm_bertadam_desc& d = descs[i];
    BaTensor& t = tens[i];
    t.p = d.p; t.g = d.g; t.m = d.m; t.v = d.v; t.n = d.n;
    t.first = first;
    t.nchunks = (int32_t)((d.n + kBaChunk - 1) / kBaChunk);
    t.g_vec = (((uintptr_t)d.g) & 15) == 0;
    t.all_vec = ((((uintptr_t)d.p) | ((uintptr_t)d.g) | ((uintptr_t)d.m) | ((uintptr_t)d.v)) & 15) == 0;
    for (int32_t c = 0; c < t.nchunks; ++c) map[first + c] = BaChunkRef{i, c};
    first += t.nchunks;
  }
  // on the caller's stream, synchronous because the host image dies at return (as tadmm_stiefel_plan_create)
  const hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  hipError_t e = hipMemcpyAsync(ws, img.data(), image, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(ws + l.norms, 0, (size_t)n * sizeof(double), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) CTX_FAIL(h, TADMM_ERR_HIP, "bertadam table upload failed: %s", hipGetErrorString(e));
  tadmm_bertadam_plan_s* P = new tadmm_bertadam_plan_s;
  P->h = h; P->n = n; P->nchunks = (int)l.nchunks;
  P->tens = reinterpret_cast<const BaTensor*>(ws + l.tens);
  P->map = reinterpret_cast<const BaChunkRef*>(ws + l.map);
  P->partial = reinterpret_cast<double*>(ws + l.partial);
  P->norms = reinterpret_cast<double*>(ws + l.norms);
  *out = P;
  return TADMM_OK;
}

int tadmm_bertadam_step(tadmm_bertadam_plan p, double lr, double b1, double b2, double e, double weight_decay,
                        double max_grad_norm, void* stream) {
  if (!p) return TADMM_ERR_INVALID;
  tadmm_handle h = p->h;
  DeviceGuard device_guard(h);
  if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0))
    CTX_FAIL(h, TADMM_ERR_INVALID, "bertadam step: b1, b2 (%g, %g) outside [0, 1)", b1, b2);
  if (!(e >= 0.0) || !(lr >= 0.0)) CTX_FAIL(h, TADMM_ERR_INVALID, "bertadam step: e %g, lr %g must not be negative", e, lr);
  BaHyper hy;
  hy.lr = (float)lr; hy.b1 = (float)b1; hy.omb1 = (float)(1.0 - b1); hy.b2 = (float)b2; hy.omb2 = (float)(1.0 - b2);
  hy.e = (float)e; hy.wd = (float)weight_decay;
  hy.clip = max_grad_norm > 0.0 ? 1 : 0;
  hy.decay = weight_decay > 0.0 ? 1 : 0;
  hy.max_norm = max_grad_norm;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid(std::min(p->nchunks, kBaGridCap)), block(kBaThreads);
  if (hy.clip) hipLaunchKernelGGL(bertadam_norm_kernel, grid, block, 0, s, p->tens, p->map, p->nchunks, p->partial);
  hipLaunchKernelGGL(bertadam_update_kernel, grid, block, 0, s, p->tens, p->map, p->nchunks, p->partial, p->norms, hy);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_bertadam_norms(tadmm_bertadam_plan p, double** norms_dev) {
  if (!p || !norms_dev) return TADMM_ERR_INVALID;
  *norms_dev = p->norms;
  return TADMM_OK;
}

int tadmm_bertadam_plan_destroy(tadmm_bertadam_plan p) {
  delete p;
  return TADMM_OK;
}

}  // extern "C"
