// Distillation loss of the training step (the reference's losses.py: DistillationLoss around CrossEntropyLoss /
// LabelSmoothingCrossEntropy / SoftTargetCrossEntropy, and xcompression/task_distill.py: soft_cross_entropy): the base
// criterion, the knowledge-distillation term and the gradients of both logit tensors from one call, two launches.
//
// For row b of C logits, s = outputs, k = outputs_kd (may be s), t = the teacher's logits, all of one type (float32,
// bfloat16 or binary16), widened on load:
//     base_b = -sum_c q_bc log_softmax(s_b)_c     q_b = (1-eps) onehot(y_b) + eps/C          (INDEX)
//                                                 q_b = (1-eps) dense_b + eps/C               (DENSE)
//     kd_b   = sum_c p_t (log p_t - log p_k),  p = softmax(. / T)                             (SOFT_KL)
//            = -log_softmax(k_b)[first argmax_c t_bc]                                         (HARD)
//            = -sum_c softmax(t_b / T)_c log_softmax(k_b / T)_c                               (SOFT_CE)
//   1. distill_rows_kernel<T, VEC, RES>  a wave owns a row, four rows to a workgroup.  A row of up to 1024 classes is
//                                    read from global memory once and kept in registers (RES, 16 values per lane and
//                                    tensor); a wider one is streamed in chunks and re-read (from the cache) by every
//                                    sweep.  Three sweeps: maxima and the teacher's first argmax; the shifted sums; the
//                                    gradients.  Every logit is shifted by its row maximum BEFORE the division
//                                    by T and before expf.  expf is float32; differences, products and sums are double,
//                                    so a row's terms carry the rounding of expf and nothing else.  Row sums are wave
//                                    butterflies.  Lane 0 writes the row's two terms (double) and its label flags.
//   2. distill_reduce_kernel         one workgroup: fixed-order sum of the row terms and flags, the means, the mix
//                                    (1-alpha) base + alpha kd -> loss_dev[0] (double), loss_f32_dev[0], counts_dev[0..1].
// The gradient sweep needs the number of kept rows (the base term's denominator) before the reduce launch has run: every
// workgroup counts the labels itself (integers: the same count everywhere).  Labels are compared, never used as an
// address.  No floating-point atomics, nothing depends on the order workgroups run in: bitwise reproducible.
// Accesses: VEC elements (16 bytes, 8 bytes or one element) chosen on the host from the three bases and row strides; the
// last C % VEC elements of a row are read singly.  Gradient rows (float32, contiguous) take 16-byte stores where the row
// start allows and single stores elsewhere.
#include "host.h"

#include <type_traits>

namespace tadmm {

struct bf16_elem { uint16_t x; };
struct f16_elem { _Float16 x; };

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(bf16_elem v) { return __uint_as_float((uint32_t)v.x << 16); }
__device__ __forceinline__ float widen(f16_elem v) { return (float)v.x; }

template <typename T, int N> struct alignas(sizeof(T) * N) ElemPack { T v[N]; };
template <int N> struct alignas((N * 4 > 16) ? 16 : N * 4) FloatPack { float v[N]; };

struct DistillArgs {
  const void* s; const void* k; const void* t;
  int64_t lds, ldk, ldt;
  const int64_t* labels;
  const float* dense; int64_t ldd;
  int64_t ignore;
  double eps, alpha, tau;
  double* slots; int32_t* flags;
  float* gs; float* gk;
  int32_t B, C, base, kd;
};

__device__ __forceinline__ double distill_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float distill_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

template <typename T, int VEC, int N>
__device__ __forceinline__ void distill_load(const T* __restrict__ row, int c, float (&v)[VEC]) {
  if (!row) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = 0.f;
  } else if (N == 1) {
    v[0] = widen(row[c]);
  } else {
    const ElemPack<T, VEC> p = *reinterpret_cast<const ElemPack<T, VEC>*>(row + c);
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = widen(p.v[j]);
  }
}

constexpr int kDistillResident = 1024;   // widest row a wave keeps in registers: 16 values per lane and tensor

// One wave's view of row b of the three tensors.  sweep(f) calls f(c, integral_constant<N>, vs, vk, vt) for columns
// c .. c + N - 1 (zeros for a null row): whole VEC-chunks first, then the C % VEC last columns one by one; a lane's
// calls come in ascending c.  RES (C <= kDistillResident): load() reads the row from global memory once and every sweep
// runs on registers; otherwise every sweep streams the row in chunks (after the first from the cache).
template <typename T, int VEC, bool RES>
struct DistillRow {
  static constexpr int CH = RES ? kDistillResident / (64 * VEC) : 1;
  const T* __restrict__ rs; const T* __restrict__ rk; const T* __restrict__ rt;
  int C, lane;
  float vs[CH][VEC], vk[CH][VEC], vt[CH][VEC], ts[VEC], tk[VEC], tt[VEC];

  template <int N>
  __device__ __forceinline__ void fetch(int c, float (&a)[VEC], float (&b)[VEC], float (&d)[VEC]) const {
    distill_load<T, VEC, N>(rs, c, a);
    if (rk == rs) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) b[j] = a[j];
    } else {
      distill_load<T, VEC, N>(rk, c, b);
    }
    distill_load<T, VEC, N>(rt, c, d);
  }

  __device__ __forceinline__ void load() {
    if constexpr (RES) {
      const int Cv = C - C % VEC;
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (i * 64 + lane) * VEC;
        if (c < Cv) fetch<VEC>(c, vs[i], vk[i], vt[i]);
      }
      if (VEC > 1 && Cv + lane < C) fetch<1>(Cv + lane, ts, tk, tt);
    }
  }

  template <class F>
  __device__ __forceinline__ void sweep(F f) {
    const int Cv = C - C % VEC;
    if constexpr (RES) {
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (i * 64 + lane) * VEC;
        if (c < Cv) f(c, std::integral_constant<int, VEC>{}, vs[i], vk[i], vt[i]);
      }
      if (VEC > 1 && Cv + lane < C) f(Cv + lane, std::integral_constant<int, 1>{}, ts, tk, tt);
    } else {
      for (int c = lane * VEC; c < Cv; c += 64 * VEC) {
        fetch<VEC>(c, vs[0], vk[0], vt[0]);
        f(c, std::integral_constant<int, VEC>{}, vs[0], vk[0], vt[0]);
      }
      if (VEC > 1 && Cv + lane < C) {
        fetch<1>(Cv + lane, ts, tk, tt);
        f(Cv + lane, std::integral_constant<int, 1>{}, ts, tk, tt);
      }
    }
  }
};

template <int VEC, int N>
__device__ __forceinline__ void distill_store(float* __restrict__ grow, bool wide, int c, const float (&v)[VEC]) {
  if (N > 1 && wide) {
    FloatPack<VEC> p;
#pragma unroll
    for (int j = 0; j < VEC; ++j) p.v[j] = v[j];
    *reinterpret_cast<FloatPack<VEC>*>(grow + c) = p;
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) grow[c + j] = v[j];
  }
}

template <typename T, int VEC, bool RES>
__global__ __launch_bounds__(256) void distill_rows_kernel(const DistillArgs a) {
  __shared__ int cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.C, base = a.base, kd = a.kd;
  const bool grads = a.gs || a.gk;
  double inv_rows = 1.0 / (double)a.B;          // denominator of the base term: B rows (DENSE), the kept rows (INDEX)
  if (base == TADMM_DISTILL_BASE_INDEX && grads) {
    int n = 0;
    for (int i = threadIdx.x; i < a.B; i += 256) {
      const int64_t y = a.labels[i];
      n += (y != a.ignore && y >= 0 && y < C) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) cnt[wave] = n;
    __syncthreads();
    const int nk = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
    inv_rows = nk > 0 ? 1.0 / (double)nk : 0.0;
  }
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= a.B) return;

  int64_t y = -1;
  bool kept = base != TADMM_DISTILL_BASE_NONE, bad = false;
  if (base == TADMM_DISTILL_BASE_INDEX) {
    y = a.labels[b];
    kept = y != a.ignore && y >= 0 && y < C;
    bad = y != a.ignore && !kept;
  }
  const T* __restrict__ rs = kept ? (const T*)a.s + b * a.lds : nullptr;
  const T* __restrict__ rk = kd != TADMM_DISTILL_KD_NONE ? (const T*)a.k + b * a.ldk : nullptr;
  const T* __restrict__ rt = kd != TADMM_DISTILL_KD_NONE ? (const T*)a.t + b * a.ldt : nullptr;
  const float* __restrict__ rq = base == TADMM_DISTILL_BASE_DENSE ? a.dense + b * a.ldd : nullptr;
  const bool hard = kd == TADMM_DISTILL_KD_HARD, soft = kd == TADMM_DISTILL_KD_SOFT_KL || kd == TADMM_DISTILL_KD_SOFT_CE;
  const bool kl = kd == TADMM_DISTILL_KD_SOFT_KL;
  const double eps = a.eps, epsC = a.eps / (double)C, inv_tau = 1.0 / a.tau;

  DistillRow<T, VEC, RES> row;
  row.rs = rs; row.rk = rk; row.rt = rt; row.C = C; row.lane = lane;
  row.load();

  // sweep 1: row maxima, first index of the teacher's maximum
  float ms = -INFINITY, mk = -INFINITY, mt = -INFINITY;
  int arg = INT32_MAX;
  row.sweep([&](int c, auto n, const float(&vs)[VEC], const float(&vk)[VEC],
                     const float(&vt)[VEC]) {
#pragma unroll
    for (int j = 0; j < decltype(n)::value; ++j) {
      ms = fmaxf(ms, vs[j]);
      mk = fmaxf(mk, vk[j]);
      if (vt[j] > mt) { mt = vt[j]; arg = c + j; }
    }
  });
  ms = distill_wave_max(ms);
  mk = distill_wave_max(mk);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(mt, off, 64);
    const int oa = __shfl_xor(arg, off, 64);
    if (om > mt || (om == mt && oa < arg)) { mt = om; arg = oa; }
  }

  // sweep 2: the shifted sums
  double Zs = 0, Ss = 0, sy = 0, Q = 0, Sq = 0, Zk = 0, karg = 0, Za = 0, Zb = 0, S1 = 0;
  row.sweep([&](int c, auto n, const float(&vs)[VEC], const float(&vk)[VEC],
                     const float(&vt)[VEC]) {
#pragma unroll
    for (int j = 0; j < decltype(n)::value; ++j) {
      if (kept) {
        const double d = (double)vs[j] - (double)ms;
        Zs += (double)expf((float)d);
        if (base == TADMM_DISTILL_BASE_INDEX) {
          Ss += d;
          if (c + j == y) sy = d;
        } else {
          const double q = (1.0 - eps) * (double)rq[c + j] + epsC;
          Q += q;
          Sq += q * d;
        }
      }
      if (hard) {
        const double d = (double)vk[j] - (double)mk;
        Zk += (double)expf((float)d);
        if (c + j == arg) karg = d;
      } else if (soft) {
        const double da = ((double)vt[j] - (double)mt) * inv_tau, db = ((double)vk[j] - (double)mk) * inv_tau;
        const double ea = (double)expf((float)da);
        Za += ea;
        Zb += (double)expf((float)db);
        S1 += ea * (kl ? da - db : db);
      }
    }
  });
  double base_b = 0.0, kd_b = 0.0, Qrow = 1.0;
  if (kept) {
    Zs = distill_wave_sum(Zs);
    if (base == TADMM_DISTILL_BASE_INDEX) {
      Ss = distill_wave_sum(Ss);
      sy = distill_wave_sum(sy);
      base_b = log(Zs) - (1.0 - eps) * sy - epsC * Ss;
    } else {
      Qrow = distill_wave_sum(Q);
      Sq = distill_wave_sum(Sq);
      base_b = Qrow * log(Zs) - Sq;
    }
  }
  if (hard) {
    Zk = distill_wave_sum(Zk);
    karg = distill_wave_sum(karg);
    kd_b = log(Zk) - karg;
  } else if (soft) {
    Za = distill_wave_sum(Za);
    Zb = distill_wave_sum(Zb);
    S1 = distill_wave_sum(S1);
    kd_b = kl ? S1 / Za - log(Za) + log(Zb) : log(Zb) - S1 / Za;
  }
  if (lane == 0) {
    a.slots[2 * b] = base_b;
    a.slots[2 * b + 1] = kd_b;
    a.flags[b] = (kept || base == TADMM_DISTILL_BASE_NONE ? 1 : 0) | (bad ? 2 : 0);
  }
  if (!grads) return;

  // sweep 3: d loss / d s and d loss / d k of this row
  const double BC = (double)a.B * (double)C;
  const double cb = (kd == TADMM_DISTILL_KD_NONE ? 1.0 : 1.0 - a.alpha) * inv_rows;
  const double ck = a.alpha * (hard ? 1.0 / (double)a.B : kl ? a.tau / BC : 1.0 / (a.tau * BC));
  const double iZs = kept ? Qrow / Zs : 0.0, iZk = hard ? 1.0 / Zk : 0.0;
  const double iZa = soft ? 1.0 / Za : 0.0, iZb = soft ? 1.0 / Zb : 0.0;
  const bool sum = a.gs == a.gk;
  float* __restrict__ gsr = a.gs ? a.gs + b * (int64_t)C : nullptr;
  float* __restrict__ gkr = (a.gk && !sum) ? a.gk + b * (int64_t)C : nullptr;
  const uintptr_t mask = sizeof(FloatPack<VEC>) > 16 ? 15 : sizeof(FloatPack<VEC>) - 1;
  const bool wide_s = gsr && (((uintptr_t)gsr) & mask) == 0, wide_k = gkr && (((uintptr_t)gkr) & mask) == 0;
  row.sweep([&](int c, auto n, const float(&vs)[VEC], const float(&vk)[VEC],
                     const float(&vt)[VEC]) {
    constexpr int N = decltype(n)::value;
    float os[VEC], ok[VEC];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double g1 = 0.0, g2 = 0.0;
      if (kept) {
        const double d = (double)vs[j] - (double)ms;
        const double q = base == TADMM_DISTILL_BASE_INDEX ? (1.0 - eps) * (c + j == y ? 1.0 : 0.0) + epsC
                                                          : (1.0 - eps) * (double)rq[c + j] + epsC;
        g1 = cb * ((double)expf((float)d) * iZs - q);
      }
      if (hard) {
        const double d = (double)vk[j] - (double)mk;
        g2 = ck * ((double)expf((float)d) * iZk - (c + j == arg ? 1.0 : 0.0));
      } else if (soft) {
        const double da = ((double)vt[j] - (double)mt) * inv_tau, db = ((double)vk[j] - (double)mk) * inv_tau;
        g2 = ck * ((double)expf((float)db) * iZb - (double)expf((float)da) * iZa);
      }
      os[j] = sum ? (float)(g1 + g2) : (float)g1;
      ok[j] = (float)g2;
    }
    if (gsr) distill_store<VEC, N>(gsr, wide_s, c, os);
    if (gkr) distill_store<VEC, N>(gkr, wide_k, c, ok);
  });
}

__global__ __launch_bounds__(256) void distill_reduce_kernel(int B, int C, int base, int kd, double alpha, double tau,
                                                             const double* __restrict__ slots,
                                                             const int32_t* __restrict__ flags,
                                                             double* __restrict__ loss, float* __restrict__ loss32,
                                                             int64_t* __restrict__ counts) {
  __shared__ double rb[256], rd[256];
  __shared__ int nk[256], nb[256];
  const int tid = threadIdx.x;
  double sb = 0.0, sd = 0.0;
  int k = 0, bad = 0;
  for (int64_t i = tid; i < B; i += 256) {
    sb += slots[2 * i];
    sd += slots[2 * i + 1];
    const int f = flags[i];
    k += f & 1;
    bad += (f >> 1) & 1;
  }
  rb[tid] = sb; rd[tid] = sd; nk[tid] = k; nb[tid] = bad;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) { rb[tid] += rb[tid + w]; rd[tid] += rd[tid + w]; nk[tid] += nk[tid + w]; nb[tid] += nb[tid + w]; }
    __syncthreads();
  }
  if (tid != 0) return;
  const double BC = (double)B * (double)C;
  const double basev = base == TADMM_DISTILL_BASE_NONE ? 0.0 : rb[0] / (double)nk[0];   // no kept row: NaN, as torch
  const double kdv = kd == TADMM_DISTILL_KD_HARD ? rd[0] / (double)B
                   : kd == TADMM_DISTILL_KD_SOFT_KL ? rd[0] * tau * tau / BC : rd[0] / BC;
  const double v = kd == TADMM_DISTILL_KD_NONE ? basev : (1.0 - alpha) * basev + alpha * kdv;
  loss[0] = v;
  if (loss32) loss32[0] = (float)v;
  counts[0] = nk[0];
  counts[1] = nb[0];
}

}  // namespace tadmm

using namespace tadmm;

namespace {

size_t distill_slots_bytes(int64_t B) { return align_up((size_t)B * 2 * sizeof(double), 256); }
size_t distill_ws_bytes(int64_t B) { return distill_slots_bytes(B) + align_up((size_t)B * sizeof(int32_t), 256); }

template <typename T>
void distill_launch(const DistillArgs& a, int vec_bytes, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)a.B + 3) / 4)), block(256);
  constexpr int V16 = 16 / (int)sizeof(T), V8 = 8 / (int)sizeof(T);
  const bool res = a.C <= kDistillResident;
#define DISTILL_GO(V)                                                                          \
  do {                                                                                         \
    if (res) hipLaunchKernelGGL((distill_rows_kernel<T, V, true>), grid, block, 0, s, a);      \
    else hipLaunchKernelGGL((distill_rows_kernel<T, V, false>), grid, block, 0, s, a);         \
  } while (0)
  if (vec_bytes == 16) DISTILL_GO(V16);
  else if (vec_bytes == 8) DISTILL_GO(V8);
  else DISTILL_GO(1);
#undef DISTILL_GO
}

}  // namespace

extern "C" {

int tadmm_distill_desc_bytes(void) { return (int)sizeof(tadmm_distill_desc); }

int tadmm_distill_workspace_bytes(const tadmm_distill_desc* d, size_t* bytes) {
  if (!d || !bytes || d->B < 1) return TADMM_ERR_INVALID;
  *bytes = distill_ws_bytes(d->B);
  return TADMM_OK;
}

int tadmm_distill_loss(tadmm_handle h, const tadmm_distill_desc* d, void* stream_) {
  if (!h) return TADMM_ERR_INVALID;
  if (!d) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: the descriptor is NULL");
  if (d->B < 1 || d->C < 1) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: B >= 1 and C >= 1 are required (got %d x %d)", d->B, d->C);
  if (d->dtype != TADMM_CHAIN_F32 && d->dtype != TADMM_CHAIN_BF16 && d->dtype != TADMM_CHAIN_F16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "distill: unknown logit type %d", d->dtype);
  if (d->base_kind < TADMM_DISTILL_BASE_NONE || d->base_kind > TADMM_DISTILL_BASE_DENSE)
    CTX_FAIL(h, TADMM_ERR_INVALID, "distill: unknown base kind %d", d->base_kind);
  if (d->kd_kind < TADMM_DISTILL_KD_NONE || d->kd_kind > TADMM_DISTILL_KD_SOFT_CE)
    CTX_FAIL(h, TADMM_ERR_INVALID, "distill: unknown KD kind %d", d->kd_kind);
  const bool has_base = d->base_kind != TADMM_DISTILL_BASE_NONE, has_kd = d->kd_kind != TADMM_DISTILL_KD_NONE;
  if (!has_base && !has_kd) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: both kinds are NONE, nothing to compute");
  const size_t es = d->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  const int64_t C = d->C;
  struct { const char* name; const void* p; int64_t ld; bool used; } rows[3] = {
      {"s", d->s, d->s_ld, has_base}, {"k", d->k, d->k_ld, has_kd}, {"t", d->t, d->t_ld, has_kd}};
  int vec_bytes = 16;
  for (const auto& r : rows) {
    if (!r.used) continue;
    if (!r.p) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: %s is NULL and the chosen kinds read it", r.name);
    if (((uintptr_t)r.p) % es) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: %s is not aligned to its element", r.name);
    if (r.ld < C) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: row stride of %s %lld < C %lld", r.name, (long long)r.ld, (long long)C);
    while (vec_bytes > (int)es && (((uintptr_t)r.p) % vec_bytes || ((size_t)r.ld * es) % vec_bytes)) vec_bytes >>= 1;
  }
  if (vec_bytes < 8) vec_bytes = (int)es;
  if (d->base_kind == TADMM_DISTILL_BASE_INDEX && (!d->labels || ((uintptr_t)d->labels) % 8))
    CTX_FAIL(h, TADMM_ERR_INVALID, "distill: labels are NULL or misaligned");
  if (d->base_kind == TADMM_DISTILL_BASE_DENSE) {
    if (!d->dense || ((uintptr_t)d->dense) % 4) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: dense targets are NULL or misaligned");
    if (d->dense_ld < C) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: row stride of the dense targets %lld < C %lld", (long long)d->dense_ld, (long long)C);
  }
  if (!(d->eps >= 0.0 && d->eps <= 1.0)) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: eps %g outside [0, 1]", d->eps);
  const bool uses_tau = d->kd_kind == TADMM_DISTILL_KD_SOFT_KL || d->kd_kind == TADMM_DISTILL_KD_SOFT_CE;
  if (uses_tau && !(d->tau > 0.0)) CTX_FAIL(h, TADMM_ERR_INVALID, "distill: tau %g must be positive", d->tau);
  if (!d->loss_dev || ((uintptr_t)d->loss_dev) % 8 || !d->counts_dev || ((uintptr_t)d->counts_dev) % 8 ||
      ((uintptr_t)d->loss_f32_dev) % 4)
    CTX_FAIL(h, TADMM_ERR_INVALID, "distill: loss_dev / counts_dev are NULL or misaligned");
  if (((uintptr_t)d->grad_s) % 4 || ((uintptr_t)d->grad_k) % 4)
    CTX_FAIL(h, TADMM_ERR_INVALID, "distill: a gradient output is not aligned to its element");
  const size_t need = distill_ws_bytes(d->B);
  if (!d->workspace || ((uintptr_t)d->workspace) % 8 || d->workspace_bytes < need)
    CTX_FAIL(h, TADMM_ERR_WORKSPACE, "distill workspace too small or misaligned: need %zu bytes, got %zu", need,
             d->workspace_bytes);

  DeviceGuard device_guard(h);
  DistillArgs a;
  a.s = has_base ? d->s : nullptr; a.k = d->k; a.t = d->t;
  a.lds = d->s_ld; a.ldk = d->k_ld; a.ldt = d->t_ld;
  a.labels = d->labels; a.dense = d->dense; a.ldd = d->dense_ld;
  a.ignore = d->ignore_index;
  a.eps = has_base ? d->eps : 0.0; a.alpha = d->alpha; a.tau = uses_tau ? d->tau : 1.0;
  a.slots = (double*)d->workspace;
  a.flags = (int32_t*)((char*)d->workspace + distill_slots_bytes(d->B));
  a.gs = d->grad_s; a.gk = d->grad_k;
  a.B = d->B; a.C = d->C; a.base = d->base_kind; a.kd = d->kd_kind;
  hipStream_t s = (hipStream_t)stream_;
  if (d->dtype == TADMM_CHAIN_F32) distill_launch<float>(a, vec_bytes, s);
  else if (d->dtype == TADMM_CHAIN_BF16) distill_launch<bf16_elem>(a, vec_bytes, s);
  else distill_launch<f16_elem>(a, vec_bytes, s);
  hipLaunchKernelGGL(distill_reduce_kernel, dim3(1), dim3(256), 0, s, a.B, a.C, a.base, a.kd, a.alpha, a.tau,
                     (const double*)a.slots, (const int32_t*)a.flags, d->loss_dev, d->loss_f32_dev, d->counts_dev);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

}  // extern "C"
