// TinyBERT's intermediate-layer distillation losses (the reference's xcompression/task_distill.py:810-828, also
// task_distill1.py, task_distill2.py and general_distill.py): the mean squared error between student and teacher
// attention scores -- both with every entry <= a threshold (the additive -10000 of masked keys) replaced by zero -- and
// between student and teacher hidden states, for ALL pairs of one training step, with the students' gradients, from one
// call of two launches.
//
// A call carries a table of up to kLmMaxPairs pairs (s_i, t_i): n_i elements each, flat, of one type (float32, bfloat16
// or binary16, widened on load), a scale c_i, a group (0 attention, 1 hidden), a clamp flag and its threshold:
//     s' = (clamp && s <= thr) ? 0 : s     t' = (clamp && t <= thr) ? 0 : t     d = s' - t'
//     term_i = c_i sum_e d^2      g_i[e] = (clamp && s <= thr) ? 0 : 2 c_i d      loss[group] = sum of the group's terms
// `<=` on the widened value: -inf is clamped, a NaN compares false and propagates (torch.where does the same).
//   1. layer_mse_stream_kernel<T>  the host cuts every pair into chunks of kLmChunk elements (a chunk never spans two
//                                  pairs); workgroup w takes chunks w, w + grid, ... (grid <= kLmGridCap) and finds a
//                                  chunk's pair by a uniform scan of the prefix chunk counts, which sit in the kernel
//                                  arguments with the rest of the table (no upload, no device table).  d, d^2 and 2 c d are
//                                  formed in double from the widened values (d is exact), so g is rounded once.  A lane
//                                  sums d^2 in double over consecutive chunks of one pair; when the pair changes, and
//                                  at the end, the workgroup sums its lanes (butterfly, then four wave sums through LDS)
//                                  into the pair's accumulator in LDS.  At exit it stores its npairs accumulators to a
//                                  workspace column of its own: slots[pair][workgroup].
//   2. layer_mse_reduce_kernel     one workgroup of sixteen waves: wave v sums the slots of pairs v, v + 16 in a fixed
//                                  order (lane l takes workgroups l, l + 64, ..., then the butterfly), term_i = c_i sum;
//                                  thread 0 adds the terms of each group in pair order and writes terms[npairs],
//                                  loss[2] (double) and loss_f32[2].
// No floating-point atomics; which workgroup takes which chunk is fixed by the table alone and nothing depends on the
// order workgroups run in: bitwise reproducible.  Element offsets are int64.
// Accesses: 16-byte loads where both bases of a pair are 16-byte aligned (a chunk is a multiple of 16 bytes, so every chunk
// of such a pair starts aligned), element loads for the other pairs; 16-byte gradient stores where the pair's gradient base
// is 16-byte aligned; the last n % (16 / sizeof(T)) elements singly.  A whole chunk of an aligned pair issues all its loads
// before the first use.
#include "host.h"

namespace tadmm {

constexpr int kLmThreads = 256;
constexpr int kLmChunk = 4096;          // elements: four (float32) or two (16-bit) 16-byte loads per lane and tensor
constexpr int kLmGridCap = 2048;        // 8 workgroups per CU; the chunks beyond are taken by a stride loop
constexpr int kLmMaxPairs = TADMM_LAYER_MSE_MAX_PAIRS;
constexpr int kLmReduceThreads = 1024;

enum { kLmClamp = 1, kLmWideLoad = 2, kLmWideStore = 4 };

// The whole call, passed by value in the kernel arguments (1.7 KiB): every field is read with a workgroup-uniform index.
struct LmTable {
  const void* s[kLmMaxPairs];
  const void* t[kLmMaxPairs];
  float* g[kLmMaxPairs];
  double c[kLmMaxPairs];
  int64_t n[kLmMaxPairs];
  float thr[kLmMaxPairs];
  int32_t flags[kLmMaxPairs];
  int32_t first[kLmMaxPairs + 1];       // chunks of pair i: first[i] .. first[i + 1] - 1
  int32_t group[kLmMaxPairs];
  int32_t npairs;
};

struct lm_bf16 { uint16_t x; };
struct lm_f16 { _Float16 x; };
__device__ __forceinline__ float lm_widen(float v) { return v; }
__device__ __forceinline__ float lm_widen(lm_bf16 v) { return __uint_as_float((uint32_t)v.x << 16); }
__device__ __forceinline__ float lm_widen(lm_f16 v) { return (float)v.x; }

template <typename T> struct alignas(16) LmPack { T v[16 / sizeof(T)]; };

__device__ __forceinline__ double lm_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// one element: adds d^2 to acc, returns the gradient
__device__ __forceinline__ float lm_elem(float s, float t, bool clamp, float thr, double c2, double& acc) {
  const bool cs = clamp && s <= thr, ct = clamp && t <= thr;
  const double d = (cs ? 0.0 : (double)s) - (ct ? 0.0 : (double)t);
  acc += d * d;
  return cs ? 0.f : (float)(c2 * d);
}

template <typename T>
__device__ __forceinline__ void lm_pack(const LmPack<T>& ps, const LmPack<T>& pt, bool clamp, float thr, double c2,
                                        double& acc, float* __restrict__ g, bool wide_store) {
  constexpr int VEC = 16 / (int)sizeof(T);
  float o[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) o[j] = lm_elem(lm_widen(ps.v[j]), lm_widen(pt.v[j]), clamp, thr, c2, acc);
  if (!g) return;
  if (wide_store) {
#pragma unroll
    for (int j = 0; j < VEC; j += 4) *reinterpret_cast<float4*>(g + j) = make_float4(o[j], o[j + 1], o[j + 2], o[j + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) g[j] = o[j];
  }
}

template <typename T>
__global__ __launch_bounds__(kLmThreads) void layer_mse_stream_kernel(const LmTable tb, int nchunks,
                                                                      double* __restrict__ slots) {
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int kIt = kLmChunk / (kLmThreads * VEC);
  __shared__ double red[kLmThreads / 64];
  __shared__ double total[kLmMaxPairs];
  const int tid = threadIdx.x;
  if (tid < kLmMaxPairs) total[tid] = 0.0;
  __syncthreads();
  // the lanes' sums of pair `p` into total[p]; uniform, every lane calls it
  auto flush = [&](int p, double v) {
    v = lm_wave_sum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) total[p] += (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
  };
  double acc = 0.0;
  int p = 0, cur = -1;
  for (int b = blockIdx.x; b < nchunks; b += gridDim.x) {
    while (p + 1 < tb.npairs && b >= tb.first[p + 1]) ++p;       // b only grows: the scan resumes where it stopped
    if (p != cur) {
      if (cur >= 0) flush(cur, acc);
      cur = p;
      acc = 0.0;
    }
    const int flags = tb.flags[p];
    const bool clamp = flags & kLmClamp, wide_store = flags & kLmWideStore;
    const float thr = tb.thr[p];
    const double c2 = 2.0 * tb.c[p];
    const int64_t off = (int64_t)(b - tb.first[p]) * kLmChunk;
    const int len = (int)min((int64_t)kLmChunk, tb.n[p] - off);
    const T* __restrict__ s = (const T*)tb.s[p] + off;
    const T* __restrict__ t = (const T*)tb.t[p] + off;
    float* __restrict__ g = tb.g[p] ? tb.g[p] + off : nullptr;
    int done = 0;
    if (flags & kLmWideLoad) {
      if (len == kLmChunk) {
        LmPack<T> S[kIt], Tt[kIt];
#pragma unroll
        for (int k = 0; k < kIt; ++k) {
          const int i = (k * kLmThreads + tid) * VEC;
          S[k] = *reinterpret_cast<const LmPack<T>*>(s + i);
          Tt[k] = *reinterpret_cast<const LmPack<T>*>(t + i);
        }
#pragma unroll
        for (int k = 0; k < kIt; ++k) {
          const int i = (k * kLmThreads + tid) * VEC;
          lm_pack<T>(S[k], Tt[k], clamp, thr, c2, acc, g ? g + i : nullptr, wide_store);
        }
        continue;
      }
      done = len - len % VEC;
      for (int i = tid * VEC; i < done; i += kLmThreads * VEC) {
        const LmPack<T> ps = *reinterpret_cast<const LmPack<T>*>(s + i);
        const LmPack<T> pt = *reinterpret_cast<const LmPack<T>*>(t + i);
        lm_pack<T>(ps, pt, clamp, thr, c2, acc, g ? g + i : nullptr, wide_store);
      }
    }
    for (int i = done + tid; i < len; i += kLmThreads) {
      const float o = lm_elem(lm_widen(s[i]), lm_widen(t[i]), clamp, thr, c2, acc);
      if (g) g[i] = o;
    }
  }
  if (cur >= 0) flush(cur, acc);
  if (tid < tb.npairs) slots[(size_t)tid * gridDim.x + blockIdx.x] = total[tid];
}

__global__ __launch_bounds__(kLmReduceThreads) void layer_mse_reduce_kernel(const LmTable tb, int grid,
                                                                            const double* __restrict__ slots,
                                                                            double* __restrict__ terms,
                                                                            double* __restrict__ loss,
                                                                            float* __restrict__ loss32) {
  __shared__ double term[kLmMaxPairs];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = wave; p < tb.npairs; p += kLmReduceThreads / 64) {
    const double* __restrict__ col = slots + (size_t)p * grid;
    double v = 0.0;
    for (int w = lane; w < grid; w += 64) v += col[w];
    v = lm_wave_sum(v);
    if (lane == 0) term[p] = tb.c[p] * v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double att = 0.0, rep = 0.0;
  for (int p = 0; p < tb.npairs; ++p) {
    terms[p] = term[p];
    if (tb.group[p] == TADMM_LAYER_MSE_ATT) att += term[p];
    else rep += term[p];
  }
  loss[0] = att;
  loss[1] = rep;
  if (loss32) {
    loss32[0] = (float)att;
    loss32[1] = (float)rep;
  }
}

}  // namespace tadmm

using namespace tadmm;

namespace {

// checks the table part of a descriptor (what the workspace size depends on) and counts the chunks
int layer_mse_chunks(tadmm_handle h, const tadmm_layer_mse_desc* d, int64_t* nchunks) {
  if (!d) CTX_FAIL(h, TADMM_ERR_INVALID, "layer_mse: the descriptor is NULL");
  if (d->npairs < 1 || d->npairs > kLmMaxPairs)
    CTX_FAIL(h, TADMM_ERR_INVALID, "layer_mse: npairs %d outside [1, %d]", d->npairs, kLmMaxPairs);
  int64_t total = 0;
  for (int i = 0; i < d->npairs; ++i) {
    const int64_t n = d->pairs[i].n;
    if (n < 1) CTX_FAIL(h, TADMM_ERR_INVALID, "layer_mse pair %d: n = %lld elements", i, (long long)n);
    total += (n - 1) / kLmChunk + 1;
    if (total > INT32_MAX)
      CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "layer_mse: more than 2^31 - 1 chunks of %d elements", kLmChunk);
  }
  *nchunks = total;
  return TADMM_OK;
}

size_t layer_mse_ws_bytes(int npairs, int64_t nchunks) {
  const size_t grid = (size_t)std::min<int64_t>(nchunks, kLmGridCap);
  return align_up(grid * (size_t)npairs * sizeof(double), 256);
}

}  // namespace

extern "C" {

int tadmm_layer_mse_desc_bytes(void) { return (int)sizeof(tadmm_layer_mse_desc); }

int tadmm_layer_mse_max_pairs(void) { return kLmMaxPairs; }

int tadmm_layer_mse_geometry(int* chunk_elems, int* max_blocks) {
  if (!chunk_elems || !max_blocks) return TADMM_ERR_INVALID;
  *chunk_elems = kLmChunk;
  *max_blocks = kLmGridCap;
  return TADMM_OK;
}

int tadmm_layer_mse_workspace_bytes(const tadmm_layer_mse_desc* d, size_t* bytes) {
  if (!bytes) return TADMM_ERR_INVALID;
  int64_t nchunks = 0;
  const int rc = layer_mse_chunks(nullptr, d, &nchunks);
  if (rc != TADMM_OK) return rc;
  *bytes = layer_mse_ws_bytes(d->npairs, nchunks);
  return TADMM_OK;
}

int tadmm_layer_mse(tadmm_handle h, const tadmm_layer_mse_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  int64_t nchunks = 0;
  const int rc = layer_mse_chunks(h, d, &nchunks);
  if (rc != TADMM_OK) return rc;
  if (d->dtype != TADMM_CHAIN_F32 && d->dtype != TADMM_CHAIN_BF16 && d->dtype != TADMM_CHAIN_F16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "layer_mse: unknown element type %d", d->dtype);
  const size_t es = d->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  LmTable tb;
  memset(&tb, 0, sizeof tb);
  tb.npairs = d->npairs;
  int32_t first = 0;
  for (int i = 0; i < d->npairs; ++i) {
    const tadmm_layer_mse_pair& q = d->pairs[i];
    if (!q.s || !q.t) CTX_FAIL(h, TADMM_ERR_INVALID, "layer_mse pair %d: s or t is NULL", i);
    if (((uintptr_t)q.s) % es || ((uintptr_t)q.t) % es || ((uintptr_t)q.grad) % 4)
      CTX_FAIL(h, TADMM_ERR_INVALID, "layer_mse pair %d: a pointer is not aligned to its element", i);
    if (q.group != TADMM_LAYER_MSE_ATT && q.group != TADMM_LAYER_MSE_REP)
      CTX_FAIL(h, TADMM_ERR_INVALID, "layer_mse pair %d: unknown group %d", i, q.group);
    tb.s[i] = q.s; tb.t[i] = q.t; tb.g[i] = q.grad;
    tb.c[i] = q.scale; tb.n[i] = q.n; tb.thr[i] = q.thr; tb.group[i] = q.group;
    tb.flags[i] = (q.clamp ? kLmClamp : 0) | (((((uintptr_t)q.s) | ((uintptr_t)q.t)) & 15) == 0 ? kLmWideLoad : 0) |
                  ((q.grad && (((uintptr_t)q.grad) & 15) == 0) ? kLmWideStore : 0);
    tb.first[i] = first;
    first += (int32_t)((q.n - 1) / kLmChunk + 1);
  }
  for (int i = d->npairs; i <= kLmMaxPairs; ++i) tb.first[i] = first;
  if (!d->terms_dev || ((uintptr_t)d->terms_dev) % 8 || !d->loss_dev || ((uintptr_t)d->loss_dev) % 8 ||
      ((uintptr_t)d->loss_f32_dev) % 4)
    CTX_FAIL(h, TADMM_ERR_INVALID, "layer_mse: terms_dev / loss_dev are NULL or misaligned");
  const size_t need = layer_mse_ws_bytes(d->npairs, nchunks);
  if (!d->workspace || ((uintptr_t)d->workspace) % 8 || d->workspace_bytes < need)
    CTX_FAIL(h, TADMM_ERR_WORKSPACE, "layer_mse workspace too small or misaligned: need %zu bytes, got %zu", need,
             d->workspace_bytes);

  DeviceGuard device_guard(h);
  hipStream_t s = (hipStream_t)stream_;
  const int grid = (int)std::min<int64_t>(nchunks, kLmGridCap);
  double* slots = (double*)d->workspace;
  if (d->dtype == TADMM_CHAIN_F32)
    hipLaunchKernelGGL(layer_mse_stream_kernel<float>, dim3(grid), dim3(kLmThreads), 0, s, tb, (int)nchunks, slots);
  else if (d->dtype == TADMM_CHAIN_BF16)
    hipLaunchKernelGGL(layer_mse_stream_kernel<lm_bf16>, dim3(grid), dim3(kLmThreads), 0, s, tb, (int)nchunks, slots);
  else
    hipLaunchKernelGGL(layer_mse_stream_kernel<lm_f16>, dim3(grid), dim3(kLmThreads), 0, s, tb, (int)nchunks, slots);
  hipLaunchKernelGGL(layer_mse_reduce_kernel, dim3(1), dim3(kLmReduceThreads), 0, s, tb, grid, (const double*)slots,
                     d->terms_dev, d->loss_dev, d->loss_f32_dev);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
