// What the row-LayerNorm launches share (bertnorm.hip: LayerNorm(dropout(x) + res); prenorm.hip: the pre-norm block
// tail of a vision transformer): the 16-bit element types with their widen / narrow, the 16-byte pack, the row loads
// and stores, the wave sum, the one expression of xhat, the parameter loader, the geometry of the backward's
// per-workgroup partials and the launcher of the kernel that adds them (defined once, in bertnorm.hip).
#pragma once
#include "host.h"

namespace tadmm {

struct bn_bf16 { uint16_t x; };
struct bn_f16 { _Float16 x; };

__device__ __forceinline__ float bn_widen(float v) { return v; }
__device__ __forceinline__ float bn_widen(bn_bf16 v) { return __uint_as_float((uint32_t)v.x << 16); }
__device__ __forceinline__ float bn_widen(bn_f16 v) { return (float)v.x; }

template <typename T> __device__ __forceinline__ T bn_narrow(float v);
template <> __device__ __forceinline__ float bn_narrow<float>(float v) { return v; }
template <> __device__ __forceinline__ bn_bf16 bn_narrow<bn_bf16>(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return bn_bf16{(uint16_t)((u >> 16) | 0x40)};     // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                                       // nearest even
  return bn_bf16{(uint16_t)(u >> 16)};
}
template <> __device__ __forceinline__ bn_f16 bn_narrow<bn_f16>(float v) { return bn_f16{(_Float16)v}; }

template <typename T, int N> struct alignas(sizeof(T) * N) BnPack { T v[N]; };

constexpr int kBnMaxNV = 32;                 // values of a row a lane holds at most
constexpr int kBnHmax = 64 * kBnMaxNV;       // widest row
constexpr int kBnFwdGrid = 1024, kBnBwdGrid = 512;

template <typename F>
__device__ __forceinline__ F bn_wave_sum(F v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// xhat, the one expression of forward and backward: the difference of two float32 values is exact in double, so xhat
// carries the rounding of rstd and its own, nothing else (a float32 difference and product would add two more, which
// the sum over rows of g xhat amplifies where the terms cancel)
__device__ __forceinline__ float bn_xhat(float s, float mean, float rstd) {
  return (float)(((double)s - (double)mean) * (double)rstd);
}

template <typename T, int VEC>
__device__ __forceinline__ void bn_load(const T* __restrict__ p, float (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = bn_widen(p[0]);
  } else {
    const BnPack<T, VEC> t = *reinterpret_cast<const BnPack<T, VEC>*>(p);
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = bn_widen(t.v[j]);
  }
}

template <typename T, int VEC>
__device__ __forceinline__ void bn_store(T* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 1) {
    p[0] = bn_narrow<T>(v[0]);
  } else {
    BnPack<T, VEC> t;
#pragma unroll
    for (int j = 0; j < VEC; ++j) t.v[j] = bn_narrow<T>(v[j]);
    *reinterpret_cast<BnPack<T, VEC>*>(p) = t;
  }
}

// gamma or beta of the columns a lane owns: float32 or T, element loads (once per wave)
template <typename T, int VEC, int CH>
__device__ __forceinline__ void bn_load_param(const void* __restrict__ p, bool f32, int hidden, int lane,
                                              float (&v)[CH][VEC]) {
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (i * 64 + lane) * VEC;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float t = 0.f;
      if (c < hidden) t = f32 ? ((const float*)p)[c + j] : bn_widen(((const T*)p)[c + j]);
      v[i][j] = t;
    }
  }
}

// the backward's row launch: four rows to a workgroup and trip, at most `cap` workgroups; one float32 (2, hp) partial
// per workgroup
inline int bn_grid(int64_t rows, int cap) { return (int)std::min<int64_t>((rows + 3) / 4, cap); }
inline int bn_hp(int hidden) { return (hidden + 3) & ~3; }
inline size_t bn_ws_bytes(int64_t rows, int hidden) {
  return align_up((size_t)bn_grid(rows, kBnBwdGrid) * 2 * bn_hp(hidden) * sizeof(float), 256);
}

// bertnorm_param_kernel (bertnorm.hip): dgamma and dbeta (each nullable) from the nwg partials, in a fixed order
void bn_param_launch(const float* part, int nwg, int hidden, int hp, float* dgamma, float* dbeta, hipStream_t s);

}  // namespace tadmm
