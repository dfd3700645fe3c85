// The k x k core convolution of the factorised layers, forward and data gradient, on NCHW tensors in place:
//
//   forward   Y (B, R2, Ho, Wo) = conv(X (B, R1, H, W); Wc (R2, R1, kh, kw))       groups = 1, any stride / padding / dilation
//   dgrad     dX (B, R1, H, W)  = conv^T(dY (B, R2, Ho, Wo); Wc)
//
// Both are ONE kernel: a destination pixel gathers, for every tap, one source pixel's channel vector and multiplies it
// with that tap's (features x channels) weight block -- product 2 of convchain.hip, with the source image read from
// global memory instead of being built in LDS.  Only the tap -> source-pixel map differs:
//   forward   (oy, ox), tap (ky, kx)  ->  (oy*sh - ph + ky*dh, ox*sw - pw + kx*dw)
//   dgrad     (iy, ix), tap (ky, kx)  ->  ((iy + ph - ky*dh) / sh, (ix + pw - kx*dw) / sw) where both divisions are exact
// and a source outside its plane (or an inexact division) contributes zero.  The map is evaluated once per workgroup
// into an LDS table [tap][64 destination pixels] of halo-pixel indices (-1: zero), so the MFMA loop is the same for
// both modes and carries no division; the data gradient needs no flipped weights, only the planes of the transposed core
// (conv_core_planes(core.permute(1, 0, 2, 3))).  At stride 2 three quarters of the data gradient's gathered rows are zero
// rows: one code path for every stride is worth more here than the skipped products.
//
// A workgroup (4 waves) owns a tile of TR rows x TW <= 64 columns (at most 64 pixels) of one destination image and up
// to 4 * NBW * 16 destination features (blockIdx.y walks further feature groups: no bound on the feature count).  The
// tile's source halo is staged in LDS as bf16 planes [P][halo pixel][KC channels + kPad], KC channels at a time in two
// buffers (no bound on the channel count): fp32 through the exact three-plane split and the six kept plane pairs, smallest
// first; bf16 as one plane.  Halo rows are contiguous pixel runs (one run per channel when the tile spans the plane's
// width): 16-byte loads where base and run length allow, 8-byte or element loads otherwise; pixels outside the image are
// never stored and never gathered.  Stores go through a wave-private staging area (the halo buffers, free after the last
// chunk) in 16-byte or 8-byte units of whole destination rows, or directly when the runs are not aligned.
#include "chain_common.h"
#include "host.h"

namespace tadmm {
namespace {

constexpr int kCcTok = 64;               // destination pixels per workgroup
constexpr size_t kCcMaxLds = 96 * 1024;  // halo buffers + tap table: one workgroup never takes more

struct CoreConvArgs {
  const void* S; void* D;                 // source and destination images
  const uint16_t* Wp; int64_t w_plane;    // fragment-major planes of the (N x taps * Kp) tap-major weight
  int32_t B, K, N;                        // images, source channels (reduction), destination features
  int32_t Hs, Ws, Hd, Wd;
  int32_t kh, kw, sh, sw, ph, pw, dh, dw;
  int32_t transposed;                     // 0: forward map, 1: data-gradient map
  int32_t TR, TW, tiles_y, tiles_x, HP;   // tile, tiles per image, halo pixels the LDS image holds
  int32_t KSR, nt;                        // k-steps of 32 channels per tap, 16-feature tiles the planes hold
  int32_t s_align;                        // source base: 2 = 16-byte aligned, 1 = 8-byte, 0 = element
};

// EPL consecutive elements from p; `n` of them exist.  vec 2: one 16-byte load, 1: two 8-byte loads, 0: elements
template <typename T> __device__ __forceinline__ uint4 halo_fetch(const T* p, int vec, int n) {
  constexpr int EPL = 16 / sizeof(T);
  if (n >= EPL && vec == 2) return *reinterpret_cast<const uint4*>(p);
  if (n >= EPL && vec == 1) {
    const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + EPL / 2);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
  }
  alignas(16) T e[EPL];
#pragma unroll
  for (int j = 0; j < EPL; ++j) e[j] = j < n ? p[j] : T(0);
  return *reinterpret_cast<const uint4*>(e);
}

// Channels [k0, k0 + KC) of the halo -> LDS image [P][HP][KC + kPad].  The halo is `nrun` runs of `runlen` contiguous
// pixels, run i starting at plane pixel p0 + i * Ws; halo pixel index = i * runlen + offset.  Channels >= K are zeros
// (their weights are, too, but 0 x stale LDS bits must not become NaN).
template <int P, int KC, typename T>
__device__ __forceinline__ void halo_load(uint16_t* img, const T* S, int64_t img_chan0, int K, int64_t plane, int k0,
                                          int HP, int p0, int nrun, int runlen, int Ws, int vec, int tid) {
  constexpr int EPL = 16 / sizeof(T), LDK = KC + kPad;
  const uint32_t gpr = (uint32_t)(runlen + EPL - 1) / EPL, G = (uint32_t)nrun * gpr, units = KC * G;
  for (uint32_t v = tid; v < units; v += 256) {
    const uint32_t c = v / G, g = v - c * G;
    const uint32_t rr = nrun == 1 ? 0u : g / gpr;
    const int o = (int)(g - rr * gpr) * EPL;
    const int n = min(EPL, runlen - o);
    const int hp = (int)rr * runlen + o;
    uint4 rg = make_uint4(0, 0, 0, 0);
    if (k0 + (int)c < K) rg = halo_fetch<T>(S + (img_chan0 + k0 + c) * plane + p0 + (int64_t)rr * Ws + o, vec, n);
    alignas(16) T e[EPL];
    *reinterpret_cast<uint4*>(e) = rg;
#pragma unroll
    for (int j = 0; j < EPL; j += 2) {
      if constexpr (P == 1) {
        if (j < n && hp + j < HP) img[(hp + j) * LDK + c] = reinterpret_cast<const uint16_t*>(e)[j];
        if (j + 1 < n && hp + j + 1 < HP) img[(hp + j + 1) * LDK + c] = reinterpret_cast<const uint16_t*>(e)[j + 1];
      } else {
        uint32_t s[P];
        split2<P>(e[j], e[j + 1], s);
#pragma unroll
        for (int p = 0; p < P; ++p) {
          if (j < n && hp + j < HP) img[(p * HP + hp + j) * LDK + c] = (uint16_t)s[p];
          if (j + 1 < n && hp + j + 1 < HP) img[(p * HP + hp + j + 1) * LDK + c] = (uint16_t)(s[p] >> 16);
        }
      }
    }
  }
}

template <int P, int KC> constexpr int cc_buf_elems(int HP) { return P * HP * (KC + kPad); }

// NBW: feature tiles (16 wide) per wave; a workgroup covers 4 * NBW * 16 destination features
template <int P, int KC, int NBW, typename T>
__global__ __launch_bounds__(256) void core_conv_kernel(const CoreConvArgs d) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  constexpr int MT = kCcTok / 16, LDK = KC + kPad, SPC = KC / 32, SZ = sizeof(T), EPL = 16 / SZ;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int tpi = d.tiles_y * d.tiles_x;
  const int img = blockIdx.x / tpi, tile = blockIdx.x - img * tpi;
  const int tyi = tile / d.tiles_x, txi = tile - tyi * d.tiles_x;
  const int ty0 = tyi * d.TR, tx0 = txi * d.TW;
  const int trows = min(d.TR, d.Hd - ty0), tcols = min(d.TW, d.Wd - tx0), ntok = trows * tcols;
  int hy_lo, hy_hi, hx_lo, hx_hi;
  halo_range(d.transposed, ty0, trows, d.kh, d.sh, d.ph, d.dh, d.Hs, hy_lo, hy_hi);
  halo_range(d.transposed, tx0, tcols, d.kw, d.sw, d.pw, d.dw, d.Ws, hx_lo, hx_hi);
  const int hrows = max(0, hy_hi - hy_lo + 1), hcols = max(0, hx_hi - hx_lo + 1);
  const bool empty = hrows == 0 || hcols == 0;
  // the halo as runs of contiguous pixels: one run per channel when it spans the plane's width
  const bool whole = hcols == d.Ws;
  const int nrun = empty ? 0 : (whole ? 1 : hrows), runlen = whole ? hrows * d.Ws : hcols;
  const int p0 = hy_lo * d.Ws + hx_lo;
  const int64_t splane = (int64_t)d.Hs * d.Ws;
  int svec = 0;                                              // the `vec` test of conv_load, per run
  if (d.s_align == 2 && splane % EPL == 0 && p0 % EPL == 0 && (nrun <= 1 || d.Ws % EPL == 0)) svec = 2;
  else if (d.s_align >= 1 && splane % (EPL / 2) == 0 && p0 % (EPL / 2) == 0 && (nrun <= 1 || d.Ws % (EPL / 2) == 0)) svec = 1;

  const int buf = cc_buf_elems<P, KC>(d.HP);
  uint16_t* Xs = lds;                                        // [2][P][HP][LDK]
  int16_t* tab = reinterpret_cast<int16_t*>(lds + 2 * buf);  // [taps][64]
  const int taps = d.kh * d.kw;
  for (int i = tid; i < taps * kCcTok; i += 256) {
    const int tap = i >> 6, t = i & 63;
    int v = -1;
    if (t < ntok) {
      const int ly = t / tcols, lx = t - ly * tcols;
      const int ky = tap / d.kw, kx = tap - ky * d.kw;
      const int sy = tap_src(d.transposed, ty0 + ly, ky, d.sh, d.ph, d.dh, d.Hs);
      const int sx = tap_src(d.transposed, tx0 + lx, kx, d.sw, d.pw, d.dw, d.Ws);
      if (sy >= hy_lo && sy <= hy_hi && sx >= hx_lo && sx <= hx_hi) {
        v = whole ? (sy - hy_lo) * d.Ws + sx : (sy - hy_lo) * hcols + (sx - hx_lo);
        if (v >= d.HP) v = -1;
      }
    }
    tab[i] = (int16_t)v;
  }

  const T* S = static_cast<const T*>(d.S);
  const int64_t chan0 = (int64_t)img * d.K;
  const int f_wg = blockIdx.y * (4 * NBW * 16), f_base = f_wg + wave * NBW * 16;
  const bool active = f_base < d.N;                          // wave-uniform: idle waves still load and synchronise
  const int S_all = taps * d.KSR;                            // k-steps of a weight row
  gw_t w[NBW];
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    int ft = f_base / 16 + j;
    ft = ft < d.nt ? ft : d.nt - 1;
    w[j] = (gw_t)d.Wp + ((int64_t)ft * S_all * 64 + lane) * 8;
  }
  float4v_t acc[MT][NBW], lo[MT][NBW];                         // lo: float32's low-order pairs (mma_tile_split)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NBW; ++j) acc[mt][j] = lo[mt][j] = float4v_t{0.f, 0.f, 0.f, 0.f};

  const int nchunks = empty ? 0 : (d.K + KC - 1) / KC;
  if (nchunks > 0) halo_load<P, KC, T>(Xs, S, chan0, d.K, splane, 0, d.HP, p0, nrun, runlen, d.Ws, svec, tid);
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const uint16_t* Xc = Xs + (c & 1) * buf;
    if (c + 1 < nchunks)
      halo_load<P, KC, T>(Xs + ((c + 1) & 1) * buf, S, chan0, d.K, splane, (c + 1) * KC, d.HP, p0, nrun, runlen, d.Ws, svec, tid);
    if (active) {
      const int ks0 = c * SPC, nks = min(SPC, d.KSR - ks0), nsteps = taps * nks;
      // weight fragments one step ahead in a two-slot ring; the surplus step of an odd count multiplies zero rows
      bf16x8_t b[2][P][NBW];
      load_w<P, NBW>(b[0], w, d.w_plane, ks0);
      int tap = 0, ks = 0;
      for (int s = 0; s < nsteps; s += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bool live = s + u < nsteps;
          int ntap = tap, nk = ks + 1;                       // position of the next step (clamped to a valid one)
          if (nk == nks) { nk = 0; ntap = tap + 1; }
          if (ntap >= taps) { ntap = taps - 1; nk = nks - 1; }
          load_w<P, NBW>(b[(u + 1) & 1], w, d.w_plane, ntap * d.KSR + ks0 + nk);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const int row = live ? (int)tab[tap * kCcTok + 16 * mt + r] : -1;
            bf16x8_t a[P];
            gather_x<P>(a, Xc, d.HP, LDK, row, ks, q);
            mma_tile_split<P, NBW>(a, b[u], acc[mt], lo[mt]);
          }
          tap = ntap; ks = nk;
        }
      }
    }
    __syncthreads();
  }
  if (!active) return;
  if constexpr (P > 1) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < NBW; ++j) acc[mt][j] += lo[mt][j];
  }

  // ---- stores: features f_base .. f_base + nf of the tile's pixels; destination rows are runs of tcols pixels (one run
  // of ntok pixels per feature when the tile spans the plane's width)
  T* D = static_cast<T*>(d.D);
  const int nf = min(NBW * 16, d.N - f_base);
  const int64_t dplane = (int64_t)d.Hd * d.Wd;
  T* dblk = D + ((int64_t)img * d.N + f_base) * dplane + (int64_t)ty0 * d.Wd + tx0;
  const bool dwhole = tcols == d.Wd;
  const int nrd = dwhole ? 1 : trows, rld = dwhole ? ntok : tcols;
  const int stage_bytes = (2 * buf * 2 / 4) & ~15;           // per wave: a quarter of the halo buffers
  const bool fits = nf * ntok * SZ <= stage_bytes;
  auto units_ok = [&](int U) {
    return (((uintptr_t)dblk) % U) == 0 && (dplane * SZ) % U == 0 && (rld * SZ) % U == 0 && (nrd == 1 || (d.Wd * SZ) % U == 0);
  };
  const int U = !fits ? 0 : (units_ok(16) ? 16 : (units_ok(8) ? 8 : 0));
  if (U) {
    T* st = reinterpret_cast<T*>(reinterpret_cast<uint8_t*>(lds) + wave * stage_bytes);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int t = 16 * mt + r;
#pragma unroll
      for (int j = 0; j < NBW; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int fl = j * 16 + 4 * q + e;
          if (t < ntok && fl < nf) {
            if constexpr (SZ == 4) st[fl * ntok + t] = acc[mt][j][e];
            else st[fl * ntok + t] = bf16_rne(acc[mt][j][e]);
          }
        }
    }
    const int upr = rld * SZ / U, upf = nrd * upr, nunits = nf * upf;   // units per run, per feature, in all
    for (int i = lane; i < nunits; i += 64) {
      const int fl = i / upf, rem = i - fl * upf;
      const int rr = nrd == 1 ? 0 : rem / upr, u = rem - rr * upr;
      const uint8_t* src = reinterpret_cast<const uint8_t*>(st + fl * ntok + rr * rld) + u * U;
      uint8_t* dst = reinterpret_cast<uint8_t*>(dblk + (int64_t)fl * dplane + (int64_t)rr * d.Wd) + u * U;
      if (U == 16) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
      else *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(src);
    }
  } else {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int t = 16 * mt + r;
      if (t >= ntok) continue;
      const int ly = t / tcols, lx = t - ly * tcols;
#pragma unroll
      for (int j = 0; j < NBW; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int fl = j * 16 + 4 * q + e;
          if (fl >= nf) continue;
          T* p = dblk + (int64_t)fl * dplane + (int64_t)ly * d.Wd + lx;
          if constexpr (SZ == 4) *p = acc[mt][j][e];
          else *p = bf16_rne(acc[mt][j][e]);
        }
    }
  }
}

template <int P, int KC> size_t cc_lds_bytes(int HP, int taps) {
  return (size_t)2 * cc_buf_elems<P, KC>(HP) * 2 + (size_t)taps * kCcTok * 2;
}

template <int P, int KC, int NBW, typename T>
hipError_t cc_launch_nbw(const CoreConvArgs& a, hipStream_t s) {
  auto kern = core_conv_kernel<P, KC, NBW, T>;
  const size_t lds = cc_lds_bytes<P, KC>(a.HP, a.kh * a.kw);
  static DynLdsOptIn allow_lds;
  const hipError_t e = allow_lds(kern, kCcMaxLds);
  if (e != hipSuccess) return e;
  const unsigned gy = (unsigned)((a.N + 4 * NBW * 16 - 1) / (4 * NBW * 16));
  hipLaunchKernelGGL(kern, dim3((unsigned)a.B * a.tiles_y * a.tiles_x, gy), dim3(256), lds, s, a);
  return hipGetLastError();
}

template <int P, int KC, typename T>
hipError_t cc_launch(const CoreConvArgs& a, hipStream_t s) {
  const int tiles = (a.N + 15) / 16;                          // spread the feature tiles over the four waves
  if (tiles <= 4) return cc_launch_nbw<P, KC, 1, T>(a, s);
  if (tiles <= 8) return cc_launch_nbw<P, KC, 2, T>(a, s);
  return cc_launch_nbw<P, KC, 4, T>(a, s);
}

constexpr int kKcF32 = 32, kKcBf16 = 64;

// Tile of the destination plane: TW = ceil(Wd / n) columns for the smallest n that fits, TR = 64 / TW rows; among the
// candidates whose halo fits the LDS budget the one with the fewest workgroups per image, then the smallest halo.
bool cc_pick_tile(CoreConvArgs& a, int dtype) {
  const int taps = a.kh * a.kw;
  int64_t best_tiles = -1;
  int best_hp = 0;
  for (int n = (a.Wd + kCcTok - 1) / kCcTok; n <= a.Wd; ++n) {
    const int tw = (a.Wd + n - 1) / n, tr = std::min(a.Hd, kCcTok / tw);
    const int64_t hr = std::min<int64_t>(a.Hs, a.transposed ? (tr - 1 + (a.kh - 1) * a.dh) / a.sh + 1 : (int64_t)(tr - 1) * a.sh + (int64_t)(a.kh - 1) * a.dh + 1);
    const int64_t hc = std::min<int64_t>(a.Ws, a.transposed ? (tw - 1 + (a.kw - 1) * a.dw) / a.sw + 1 : (int64_t)(tw - 1) * a.sw + (int64_t)(a.kw - 1) * a.dw + 1);
    const int64_t hp = std::max<int64_t>(hr * hc, 16);
    if (hp > 32767) continue;
    const size_t lds = dtype == TADMM_CHAIN_F32 ? cc_lds_bytes<3, kKcF32>((int)hp, taps) : cc_lds_bytes<1, kKcBf16>((int)hp, taps);
    if (lds > kCcMaxLds) continue;
    const int64_t tiles = (int64_t)((a.Hd + tr - 1) / tr) * ((a.Wd + tw - 1) / tw);
    if (best_tiles < 0 || tiles < best_tiles || (tiles == best_tiles && hp < best_hp)) {
      best_tiles = tiles; best_hp = (int)hp;
      a.TR = tr; a.TW = tw; a.tiles_y = (a.Hd + tr - 1) / tr; a.tiles_x = (a.Wd + tw - 1) / tw; a.HP = (int)hp;
    }
  }
  return best_tiles > 0;
}

int align_class(const void* p) { return ((uintptr_t)p & 15) == 0 ? 2 : (((uintptr_t)p & 7) == 0 ? 1 : 0); }

}  // namespace

// Shapes, dtype, geometry and operands of a core-convolution descriptor (what forward, data gradient and weight
// gradient share); `need_planes`: the plane pointer is read.
int core_conv_check(tadmm_handle h, const tadmm_core_conv_desc* c, bool need_planes, int planes_rows, int planes_cols) {
  if (!c) CTX_FAIL(h, TADMM_ERR_INVALID, "core conv: null descriptor");
  if (c->B < 0 || c->R1 <= 0 || c->R2 <= 0 || c->H <= 0 || c->W <= 0 || c->kh <= 0 || c->kw <= 0 || c->stride_h <= 0 ||
      c->stride_w <= 0 || c->dil_h <= 0 || c->dil_w <= 0 || c->pad_h < 0 || c->pad_w < 0)
    CTX_FAIL(h, TADMM_ERR_INVALID, "core conv: bad geometry (B = %d, R1 = %d, R2 = %d, %d x %d, kernel %d x %d)", c->B, c->R1,
             c->R2, c->H, c->W, c->kh, c->kw);
  if (c->dtype != TADMM_CHAIN_F32 && c->dtype != TADMM_CHAIN_BF16) CTX_FAIL(h, TADMM_ERR_INVALID, "core conv: unknown dtype %d", c->dtype);
  const int64_t ho = ((int64_t)c->H + 2 * (int64_t)c->pad_h - (int64_t)c->dil_h * (c->kh - 1) - 1) / c->stride_h + 1;
  const int64_t wo = ((int64_t)c->W + 2 * (int64_t)c->pad_w - (int64_t)c->dil_w * (c->kw - 1) - 1) / c->stride_w + 1;
  if ((int64_t)c->H + 2 * (int64_t)c->pad_h < (int64_t)c->dil_h * (c->kh - 1) + 1 ||
      (int64_t)c->W + 2 * (int64_t)c->pad_w < (int64_t)c->dil_w * (c->kw - 1) + 1 || ho <= 0 || wo <= 0)
    CTX_FAIL(h, TADMM_ERR_INVALID, "core conv: empty output plane");
  if (ho != c->Ho || wo != c->Wo)
    CTX_FAIL(h, TADMM_ERR_INVALID, "core conv: output plane %d x %d does not match the geometry (%lld x %lld)", c->Ho, c->Wo,
             (long long)ho, (long long)wo);
  const uintptr_t esz = c->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  if (c->B > 0 && (!c->X || !c->Y)) CTX_FAIL(h, TADMM_ERR_INVALID, "core conv: null operand");
  if (((uintptr_t)c->X | (uintptr_t)c->Y) & (esz - 1)) CTX_FAIL(h, TADMM_ERR_INVALID, "core conv: misaligned operand");
  if (need_planes) {
    const int64_t kp = ((int64_t)planes_cols + 31) / 32, np = ((int64_t)planes_rows + 31) / 32 * 2;
    if (c->B > 0 && !c->Wc) CTX_FAIL(h, TADMM_ERR_INVALID, "core conv: null weight planes");
    if ((((uintptr_t)c->Wc) & 15) || (c->wc_plane & 7) || c->wc_plane < np * (int64_t)c->kh * c->kw * kp * 512)
      CTX_FAIL(h, TADMM_ERR_INVALID, "core conv: weight planes too small or misaligned (tadmm.ops.conv_core_planes builds them)");
  }
  const int64_t lim = INT32_MAX;
  if ((int64_t)c->H * c->W > lim || ho * wo > lim || (int64_t)c->kh * c->kw > 4096 || (int64_t)c->kh * c->dil_h > (1 << 20) ||
      (int64_t)c->kw * c->dil_w > (1 << 20) || c->pad_h > (1 << 20) || c->pad_w > (1 << 20) || c->stride_h > (1 << 20) ||
      c->stride_w > (1 << 20))
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "core conv: plane, kernel, padding or stride beyond the launch's index range");
  return TADMM_OK;
}

// transposed 0: Y = conv(X; Wc); 1: X = conv^T(Y; Wc) with the planes of the transposed core
int launch_core_conv(tadmm_handle h, const tadmm_core_conv_desc* c, int transposed, hipStream_t s) {
  const int rc = core_conv_check(h, c, true, transposed ? c->R1 : c->R2, transposed ? c->R2 : c->R1);
  if (rc != TADMM_OK) return rc;
  if (c->B == 0) return TADMM_OK;
  CoreConvArgs a;
  memset(&a, 0, sizeof a);
  a.Wp = (const uint16_t*)c->Wc; a.w_plane = c->wc_plane; a.B = c->B;
  a.kh = c->kh; a.kw = c->kw; a.sh = c->stride_h; a.sw = c->stride_w; a.ph = c->pad_h; a.pw = c->pad_w;
  a.dh = c->dil_h; a.dw = c->dil_w; a.transposed = transposed;
  if (!transposed) { a.S = c->X; a.D = c->Y; a.K = c->R1; a.N = c->R2; a.Hs = c->H; a.Ws = c->W; a.Hd = c->Ho; a.Wd = c->Wo; }
  else { a.S = c->Y; a.D = c->X; a.K = c->R2; a.N = c->R1; a.Hs = c->Ho; a.Ws = c->Wo; a.Hd = c->H; a.Wd = c->W; }
  a.KSR = (a.K + 31) / 32;
  a.nt = (a.N + 31) / 32 * 2;
  a.s_align = align_class(a.S);
  if (!cc_pick_tile(a, c->dtype)) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "core conv: no tile's halo fits the LDS");
  const int64_t wgs = (int64_t)a.B * a.tiles_y * a.tiles_x;
  if (wgs > INT32_MAX || (a.N + 63) / 64 > 65535) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "core conv: grid beyond the launch");
  const hipError_t e = c->dtype == TADMM_CHAIN_F32 ? cc_launch<3, kKcF32, float>(a, s) : cc_launch<1, kKcBf16, uint16_t>(a, s);
  if (e != hipSuccess) CTX_FAIL(h, TADMM_ERR_HIP, "core conv: launch failed: %s", hipGetErrorString(e));
  return TADMM_OK;
}

}  // namespace tadmm
