// TT-LSTM recurrence (ablation/tt_lstm_inference.py:44-77) as ONE launch for the whole sequence, and its backward
// through time as one launch.
//
// H = hidden size.  Xp (T, B, 4H) float32 holds the input pre-activations of every step, bias included (the TT input
// map produces it outside, one `linear_chain` launch for all T*B tokens).  Whh (4H, H), gate order z = [i | f | g | o]:
//     z_t = Xp[t] + h_{t-1} Whh^T,   i, f, o = S(z),  g = tanh(z),   c_t = f c_{t-1} + i g,   h_t = o tanh(c_t)
// with S = Hardsigmoid (the reference) or the logistic function (SIGMOID: a model trained as torch.nn.LSTM).
//
// Batch rows never interact, so a workgroup (4 waves) that owns 16 rows walks t = 0 .. T-1 alone: no grid barrier, no
// flags, no second launch.  The MFMA roles are the swapped ones of chain.hip (A = weight rows, B = batch rows): the D tile
// is 16 hidden units x 16 rows and a lane holds 4 consecutive units of one row.  A wave owns TPW consecutive 16-unit
// tiles and, for each, the FOUR gate tiles: the host packs Whh gate by gate (each gate's H rows padded to Hp = ceil16(H),
// `ops.lstm_planes`), so the four pre-activations of a (row, unit) pair sit in one lane at the same register index and the
// gate arithmetic needs no LDS and no cross-lane traffic.  h_{t-1} lives in LDS as three bf16 planes (the exact split of
// chain_common.h), double-buffered: one workgroup barrier per step.  c stays in float32 registers.  Whh fragments come from
// L2 every step (1.5 MB of planes at H = 256: they fit an XCD's L2, not the LDS), one k-step ahead of their use.
// Xp[t+1] is requested while step t computes; its values initialise the accumulators.
//
// Backward: same grid and (row, unit) ownership, t = T-1 .. 0.  dz follows lane-locally from the saved gate activations
// G[t] and cell states C[t], C[t-1]; it goes to HBM (dZ[t], which is also dXp[t]) and, as three planes, to LDS;
// dh_{t-1} = dz Whh (reduction over 4Hp) runs on the transposed planes with the output tiles dealt in the same ownership.
// dWhh, dbias and the TT cores' gradients are products over all T*B tokens and are left to `ops.wgrad` and the
// `linear_chain` backward.
//
// Rows beyond B and units beyond H are kept at exact zeros in LDS (they are written as zeros, never as what the
// arithmetic would give); nothing outside the tensors is read or written.  No atomics; bitwise reproducible.
#include "chain_common.h"
#include "host.h"

namespace tadmm {
namespace {

constexpr int kLstmRows = 16;               // batch rows of a workgroup
constexpr int kLstmWaves = 4;
constexpr int kLstmThreads = 64 * kLstmWaves;
constexpr int kLstmMaxTpw = 4;              // 16-unit tiles per wave at most: c, dc and dh of a lane are 16 registers each
constexpr int kLstmMaxH = 16 * kLstmWaves * kLstmMaxTpw;
constexpr size_t kLstmMaxLds = 160 * 1024;

struct LstmGeom {
  int H = 0, Hp = 0, Kp = 0, NT = 0, tpw = 0;
  size_t stage = 0, fwd_lds = 0, bwd_lds = 0;
  bool fits = false;
};

int lstm_geom(const tadmm_lstm_desc* c, LstmGeom& g) {
  if (!c || c->H < 1) return TADMM_ERR_INVALID;
  g.H = c->H;
  g.fits = false;
  if (c->H > kLstmMaxH) return TADMM_OK;     // not sized: the LDS figures stay 0
  g.Hp = (c->H + 15) / 16 * 16;
  g.Kp = (c->H + 31) / 32 * 32;
  g.NT = g.Hp / 16;
  const int need = (g.NT + kLstmWaves - 1) / kLstmWaves;
  g.tpw = need <= 1 ? 1 : need <= 2 ? 2 : 4;
  g.stage = (size_t)kLstmWaves * kLstmRows * (16 * g.tpw + 4) * 4;
  g.fwd_lds = (size_t)2 * 3 * kLstmRows * (g.Kp + kPad) * 2 + g.stage;
  g.bwd_lds = (size_t)3 * kLstmRows * (4 * g.Hp + kPad) * 2 + g.stage;
  g.fits = g.fwd_lds <= kLstmMaxLds && g.bwd_lds <= kLstmMaxLds;
  return TADMM_OK;
}

struct LstmArgs {
  const float* Xp; const void* W; const float* h0; const float* c0;
  float* Y; float* hT; float* cT; float* G; float* C;
  const float* dY; const float* dhT; const float* dcT;
  float* dZ; float* dh0; float* dc0;
  int64_t T, B, plane;
  int32_t H, Hp, Kp;
  int32_t vx, vy, vh0, vc0, vhT, vcT, vG, vC, vdY, vdhT, vdcT, vdZ, vdh0, vdc0;   // 16-byte paths allowed
};

template <bool SIGMOID> __device__ __forceinline__ float lstm_gate(float x) {
  if constexpr (SIGMOID) return 1.f / (1.f + expf(-x));
  else return fminf(fmaxf(x + 3.f, 0.f), 6.f) / 6.f;               // torch's Hardsigmoid: exactly 0 and 1 when saturated
}
template <bool SIGMOID> __device__ __forceinline__ float lstm_gate_grad(float a) {
  if constexpr (SIGMOID) return a * (1.f - a);
  else return (a > 0.f && a < 1.f) ? (1.f / 6.f) : 0.f;             // torch's rule, from the saved activation
}

// units [f, f+4) of one row (src points at the row's unit 0); zeros for a row or units outside the tensor
__device__ __forceinline__ float4v_t lstm_load4(const float* src, int f, int H, bool row_ok, bool vec) {
  float4v_t v = {0.f, 0.f, 0.f, 0.f};
  if (row_ok && f < H) {
    if (vec && f + 4 <= H) {
      const float4 t = *reinterpret_cast<const float4*>(src + f);
      v = float4v_t{t.x, t.y, t.z, t.w};
    } else {
      v[0] = src[f];
      if (f + 1 < H) v[1] = src[f + 1];
      if (f + 2 < H) v[2] = src[f + 2];
      if (f + 3 < H) v[3] = src[f + 3];
    }
  }
  return v;
}

// The staging area is exchanged between the lanes of ONE wave.  The hardware runs a wave's LDS instructions in order, but
// the compiler reasons per thread: without a convergent barrier it may sink the next write into a branch only some lanes
// take, ahead of the other lanes' reads.  All lanes of the wave reach this point together (wave-uniform control flow).
__device__ __forceinline__ void lstm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The TPW tiles of a wave -> rows [0, nrows) x units [u0, u0 + 16 TPW) below H of `dst` (points at row 0, unit 0; row
// stride ld), through the wave-private staging area: one instruction writes 64 / (4 TPW) rows of 64 TPW contiguous bytes,
// in whole 16-byte units with `vec`, element by element otherwise.
template <int TPW>
__device__ __forceinline__ void lstm_store_rows(float* stage, const float4v_t (&v)[TPW], float* dst, int64_t ld, int nrows,
                                                int u0, int H, bool vec, int lane) {
  constexpr int SLD = 16 * TPW + 4, UPR = 4 * TPW, RPI = 64 / UPR;
  const int r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int j = 0; j < TPW; ++j)
    *reinterpret_cast<float4*>(stage + r * SLD + 16 * j + 4 * q) = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
  const int rl = lane / UPR, u = lane - rl * UPR;
  const int f = u0 + 4 * u;
  lstm_wave_sync();                            // the rows are read by other lanes than wrote them
  float4 s[kLstmRows / RPI];
#pragma unroll
  for (int i = 0; i < kLstmRows / RPI; ++i) s[i] = *reinterpret_cast<const float4*>(stage + (i * RPI + rl) * SLD + 4 * u);
  lstm_wave_sync();                            // every lane has its rows before the area is written again
#pragma unroll
  for (int i = 0; i < kLstmRows / RPI; ++i) {
    const int row = i * RPI + rl;
    if (row < nrows && f < H) {
      float* g = dst + (int64_t)row * ld + f;
      if (vec && f + 4 <= H) *reinterpret_cast<float4*>(g) = s[i];
      else {
        g[0] = s[i].x;
        if (f + 1 < H) g[1] = s[i].y;
        if (f + 2 < H) g[2] = s[i].z;
        if (f + 3 < H) g[3] = s[i].w;
      }
    }
  }
}

// 4 units of one row -> three bf16 planes of an LDS image [3][16][ld] at column `col`
__device__ __forceinline__ void lstm_put_planes(uint16_t* img, int ld, int r, int col, const float4v_t v) {
  uint32_t s0[3], s1[3];
  split2<3>(v[0], v[1], s0);
  split2<3>(v[2], v[3], s1);
#pragma unroll
  for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2*>(&img[(p * kLstmRows + r) * ld + col]) = make_uint2(s0[p], s1[p]);
}

__device__ __forceinline__ void lstm_zero_lds(uint16_t* img, int elems, int tid) {
  uint32_t* w = reinterpret_cast<uint32_t*>(img);
  for (int i = tid; i < elems / 2; i += kLstmThreads) w[i] = 0u;
}

template <int TPW, bool SAVE, bool SIGMOID>
__global__ __launch_bounds__(kLstmThreads) void lstm_seq_kernel(const LstmArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int H = a.H, Hp = a.Hp, KS = a.Kp / 32, NT = Hp / 16;
  const int LDH = a.Kp + kPad;
  const int64_t b0 = (int64_t)blockIdx.x * kLstmRows;
  const int nrows = (int)min((int64_t)kLstmRows, a.B - b0);
  const bool row_ok = r < nrows;
  const int hbuf = 3 * kLstmRows * LDH;
  uint16_t* hs = lds;                                                       // [2][3][16][LDH]
  float* stage = reinterpret_cast<float*>(lds + 2 * hbuf) + wave * (kLstmRows * (16 * TPW + 4));
  const int u0 = wave * TPW * 16;                                           // first unit of this wave

  lstm_zero_lds(hs, 2 * hbuf, tid);
  __syncthreads();
  float4v_t c[TPW], hv[TPW], xn[TPW][4];
  const int64_t row = b0 + r;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int u = u0 + 16 * j + 4 * q;
    c[j] = a.c0 ? lstm_load4(a.c0 + row * H, u, H, row_ok, a.vc0) : float4v_t{0.f, 0.f, 0.f, 0.f};
    hv[j] = a.h0 ? lstm_load4(a.h0 + row * H, u, H, row_ok, a.vh0) : float4v_t{0.f, 0.f, 0.f, 0.f};
    if (wave * TPW + j < NT) lstm_put_planes(hs, LDH, r, u, hv[j]);
    const float* xr = a.Xp + row * 4 * H;
#pragma unroll
    for (int g = 0; g < 4; ++g) xn[j][g] = lstm_load4(xr + (int64_t)g * H, u, H, row_ok, a.vx);
  }
  __syncthreads();

  for (int64_t t = 0; t < a.T; ++t) {
    const uint16_t* hc = hs + (t & 1) * hbuf;
    uint16_t* hn = hs + ((t + 1) & 1) * hbuf;
    float4v_t ga[SAVE ? 4 : 1][TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int tile = wave * TPW + j;                                      // wave-uniform
      const int u = u0 + 16 * j + 4 * q;
      if (tile < NT) {
        float4v_t acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = xn[j][g];
        if (t + 1 < a.T) {                                                  // step t+1's pre-activations, under way while t computes
          const float* xr = a.Xp + ((t + 1) * a.B + row) * 4 * H;
#pragma unroll
          for (int g = 0; g < 4; ++g) xn[j][g] = lstm_load4(xr + (int64_t)g * H, u, H, row_ok, a.vx);
        }
        gw_t wb[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) wb[g] = (gw_t)a.W + ((int64_t)(g * NT + tile) * KS * 64 + lane) * 8;
        bf16x8_t bc[3][4], bn[3][4], av[3];
        load_w<3, 4>(bc, wb, a.plane, 0);
        // no data-dependent branch in here: the last trip re-reads its own fragments instead of branching
        for (int ks = 0; ks < KS; ++ks) {
          load_w<3, 4>(bn, wb, a.plane, min(ks + 1, KS - 1));
#pragma unroll
          for (int p = 0; p < 3; ++p)
            av[p] = *reinterpret_cast<const bf16x8_t*>(&hc[(p * kLstmRows + r) * LDH + 32 * ks + 8 * q]);
          constexpr int pa[6] = {2, 0, 1, 1, 0, 0}, pb[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
          for (int pr = 0; pr < 6; ++pr)
#pragma unroll
            for (int g = 0; g < 4; ++g)
              acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bc[pb[pr]][g], av[pa[pr]], acc[g], 0, 0, 0);
#pragma unroll
          for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int g = 0; g < 4; ++g) bc[p][g] = bn[p][g];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool ok = row_ok && u + e < H;
          const float ig = lstm_gate<SIGMOID>(acc[0][e]), fg = lstm_gate<SIGMOID>(acc[1][e]);
          const float gg = tanhf(acc[2][e]), og = lstm_gate<SIGMOID>(acc[3][e]);
          const float cn = fg * c[j][e] + ig * gg;
          c[j][e] = ok ? cn : 0.f;
          hv[j][e] = ok ? og * tanhf(cn) : 0.f;
          if constexpr (SAVE) { ga[0][j][e] = ig; ga[1][j][e] = fg; ga[2][j][e] = gg; ga[3][j][e] = og; }
        }
        lstm_put_planes(hn, LDH, r, u, hv[j]);
      } else {
        hv[j] = float4v_t{0.f, 0.f, 0.f, 0.f};
        if constexpr (SAVE) {
#pragma unroll
          for (int g = 0; g < 4; ++g) ga[g][j] = float4v_t{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    if (u0 < H) {
      const int64_t tb = t * a.B + b0;
      lstm_store_rows<TPW>(stage, hv, a.Y + tb * H, H, nrows, u0, H, a.vy, lane);
      if constexpr (SAVE) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          lstm_store_rows<TPW>(stage, ga[g], a.G + tb * 4 * H + (int64_t)g * H, 4 * (int64_t)H, nrows, u0, H, a.vG, lane);
        lstm_store_rows<TPW>(stage, c, a.C + tb * H, H, nrows, u0, H, a.vC, lane);
      }
    }
    __syncthreads();                           // h_t complete in `hn`, every read of h_{t-1} done
  }
  if (u0 < H) {
    lstm_store_rows<TPW>(stage, hv, a.hT + b0 * H, H, nrows, u0, H, a.vhT, lane);
    lstm_store_rows<TPW>(stage, c, a.cT + b0 * H, H, nrows, u0, H, a.vcT, lane);
  }
}

template <int TPW, bool SIGMOID>
__global__ __launch_bounds__(kLstmThreads) void lstm_seq_bwd_kernel(const LstmArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int H = a.H, Hp = a.Hp, NT = Hp / 16, KSB = Hp / 8;                 // reduction over 4 Hp
  const int LDZ = 4 * Hp + kPad;
  const int64_t b0 = (int64_t)blockIdx.x * kLstmRows;
  const int nrows = (int)min((int64_t)kLstmRows, a.B - b0);
  const bool row_ok = r < nrows;
  uint16_t* dzs = lds;                                                      // [3][16][LDZ]
  float* stage = reinterpret_cast<float*>(lds + 3 * kLstmRows * LDZ) + wave * (kLstmRows * (16 * TPW + 4));
  const int u0 = wave * TPW * 16;
  const int64_t row = b0 + r;

  lstm_zero_lds(dzs, 3 * kLstmRows * LDZ, tid);
  float4v_t dh[TPW], dc[TPW], gv[4][TPW], cc[TPW], cp[TPW], dy[TPW];
  gw_t wb[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int u = u0 + 16 * j + 4 * q;
    dh[j] = a.dhT ? lstm_load4(a.dhT + row * H, u, H, row_ok, a.vdhT) : float4v_t{0.f, 0.f, 0.f, 0.f};
    dc[j] = a.dcT ? lstm_load4(a.dcT + row * H, u, H, row_ok, a.vdcT) : float4v_t{0.f, 0.f, 0.f, 0.f};
    const int tile = min(wave * TPW + j, NT - 1);                           // surplus tiles compute and are dropped
    wb[j] = (gw_t)a.W + ((int64_t)tile * KSB * 64 + lane) * 8;
  }
  auto load_step = [&](int64_t t) {
    const int64_t tb = t * a.B + row;
    const float* cprev = t > 0 ? a.C + (tb - a.B) * H : (a.c0 ? a.c0 + row * H : nullptr);
    const bool vcp = t > 0 ? a.vC : a.vc0;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int u = u0 + 16 * j + 4 * q;
#pragma unroll
      for (int g = 0; g < 4; ++g) gv[g][j] = lstm_load4(a.G + tb * 4 * H + (int64_t)g * H, u, H, row_ok, a.vG);
      cc[j] = lstm_load4(a.C + tb * H, u, H, row_ok, a.vC);
      cp[j] = cprev ? lstm_load4(cprev, u, H, row_ok, vcp) : float4v_t{0.f, 0.f, 0.f, 0.f};
      dy[j] = a.dY ? lstm_load4(a.dY + tb * H, u, H, row_ok, a.vdY) : float4v_t{0.f, 0.f, 0.f, 0.f};
    }
  };
  load_step(a.T - 1);
  __syncthreads();

  for (int64_t t = a.T - 1; t >= 0; --t) {
    float4v_t dz[4][TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int u = u0 + 16 * j + 4 * q;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = row_ok && u + e < H;
        const float ig = gv[0][j][e], fg = gv[1][j][e], gg = gv[2][j][e], og = gv[3][j][e];
        const float tc = tanhf(cc[j][e]);
        const float dht = dy[j][e] + dh[j][e];
        const float dct = dc[j][e] + dht * og * (1.f - tc * tc);
        dz[0][j][e] = ok ? dct * gg * lstm_gate_grad<SIGMOID>(ig) : 0.f;
        dz[1][j][e] = ok ? dct * cp[j][e] * lstm_gate_grad<SIGMOID>(fg) : 0.f;
        dz[2][j][e] = ok ? dct * ig * (1.f - gg * gg) : 0.f;
        dz[3][j][e] = ok ? dht * tc * lstm_gate_grad<SIGMOID>(og) : 0.f;
        dc[j][e] = ok ? dct * fg : 0.f;
      }
      if (wave * TPW + j < NT) {
#pragma unroll
        for (int g = 0; g < 4; ++g) lstm_put_planes(dzs, LDZ, r, g * Hp + u, dz[g][j]);
      }
    }
    if (u0 < H) {
      const int64_t tb = t * a.B + b0;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        lstm_store_rows<TPW>(stage, dz[g], a.dZ + tb * 4 * H + (int64_t)g * H, 4 * (int64_t)H, nrows, u0, H, a.vdZ, lane);
    }
    __syncthreads();                           // dz_t complete in LDS
    if (t > 0) load_step(t - 1);               // does not depend on the recurrence: under way during the product
    float4v_t acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) acc[j] = float4v_t{0.f, 0.f, 0.f, 0.f};
    bf16x8_t bc[3][TPW], bn[3][TPW], av[3];
    load_w<3, TPW>(bc, wb, a.plane, 0);
    for (int ks = 0; ks < KSB; ++ks) {
      load_w<3, TPW>(bn, wb, a.plane, min(ks + 1, KSB - 1));
#pragma unroll
      for (int p = 0; p < 3; ++p)
        av[p] = *reinterpret_cast<const bf16x8_t*>(&dzs[(p * kLstmRows + r) * LDZ + 32 * ks + 8 * q]);
      constexpr int pa[6] = {2, 0, 1, 1, 0, 0}, pb[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
      for (int pr = 0; pr < 6; ++pr)
#pragma unroll
        for (int j = 0; j < TPW; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bc[pb[pr]][j], av[pa[pr]], acc[j], 0, 0, 0);
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int j = 0; j < TPW; ++j) bc[p][j] = bn[p][j];
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int u = u0 + 16 * j + 4 * q;
#pragma unroll
      for (int e = 0; e < 4; ++e) dh[j][e] = (row_ok && u + e < H) ? acc[j][e] : 0.f;
    }
    __syncthreads();                           // every read of dz_t done before dz_{t-1} is written
  }
  if (u0 < H) {
    if (a.dh0) lstm_store_rows<TPW>(stage, dh, a.dh0 + b0 * H, H, nrows, u0, H, a.vdh0, lane);
    if (a.dc0) lstm_store_rows<TPW>(stage, dc, a.dc0 + b0 * H, H, nrows, u0, H, a.vdc0, lane);
  }
}

template <int TPW, bool SAVE, bool SIGMOID> hipError_t lstm_launch_fwd(const LstmArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
  auto kern = lstm_seq_kernel<TPW, SAVE, SIGMOID>;
  static DynLdsOptIn allow_lds;
  const hipError_t e = lds > 64 * 1024 ? allow_lds(kern, kLstmMaxLds) : hipSuccess;
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(kLstmThreads), lds, s, a);
  return hipGetLastError();
}
template <int TPW, bool SIGMOID> hipError_t lstm_launch_bwd(const LstmArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
  auto kern = lstm_seq_bwd_kernel<TPW, SIGMOID>;
  static DynLdsOptIn allow_lds;
  const hipError_t e = lds > 64 * 1024 ? allow_lds(kern, kLstmMaxLds) : hipSuccess;
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(kLstmThreads), lds, s, a);
  return hipGetLastError();
}

template <bool SAVE, bool SIGMOID> hipError_t lstm_fwd_tpw(int tpw, const LstmArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
  if (tpw == 1) return lstm_launch_fwd<1, SAVE, SIGMOID>(a, blocks, lds, s);
  if (tpw == 2) return lstm_launch_fwd<2, SAVE, SIGMOID>(a, blocks, lds, s);
  return lstm_launch_fwd<4, SAVE, SIGMOID>(a, blocks, lds, s);
}
template <bool SIGMOID> hipError_t lstm_bwd_tpw(int tpw, const LstmArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
  if (tpw == 1) return lstm_launch_bwd<1, SIGMOID>(a, blocks, lds, s);
  if (tpw == 2) return lstm_launch_bwd<2, SIGMOID>(a, blocks, lds, s);
  return lstm_launch_bwd<4, SIGMOID>(a, blocks, lds, s);
}

inline bool lstm_bad_ptr(const void* p) { return !p || ((uintptr_t)p & 3); }
inline bool lstm_bad_opt(const void* p) { return p && ((uintptr_t)p & 3); }
// a 16-byte path needs the base on a 16-byte boundary and every row and gate offset a multiple of 4 elements
inline int32_t lstm_vec(const void* p, int H) { return (p && ((uintptr_t)p & 15) == 0 && H % 4 == 0) ? 1 : 0; }

// what all three entries check; fills the geometry and the shared part of the kernel arguments
int lstm_args(tadmm_ctx_s* h, const tadmm_lstm_desc* c, const char* who, LstmGeom& g, LstmArgs& a) {
  const int rc = lstm_geom(c, g);
  if (rc != TADMM_OK) CTX_FAIL(h, rc, "%s: a descriptor with H >= 1 is required", who);
  if (!g.fits) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "%s: H = %d, the launch takes 1 <= H <= %d", who, c->H, kLstmMaxH);
  if (c->T < 1 || c->B < 1) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: T >= 1 and B >= 1 are required (got T = %lld, B = %lld)", who,
                                     (long long)c->T, (long long)c->B);
  if (c->sigmoid != 0 && c->sigmoid != 1) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: sigmoid is 0 (Hardsigmoid) or 1 (logistic)", who);
  if (c->B > ((int64_t)1 << 31) * kLstmRows - kLstmRows || c->T > ((int64_t)1 << 40) / c->B / (4 * (int64_t)c->H))
    CTX_FAIL(h, TADMM_ERR_INVALID, "%s: T * B * 4H beyond 2^40 elements, or more than 2^31 workgroups", who);
  if (!c->W || ((uintptr_t)c->W & 15)) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: W (the weight planes) is null or not 16-byte aligned", who);
  if (lstm_bad_opt(c->c0)) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: c0 is misaligned", who);
  memset(&a, 0, sizeof a);
  a.W = c->W; a.c0 = c->c0; a.vc0 = lstm_vec(c->c0, c->H);
  a.T = c->T; a.B = c->B; a.H = g.H; a.Hp = g.Hp; a.Kp = g.Kp;
  return TADMM_OK;
}

int lstm_fwd(tadmm_ctx_s* h, const tadmm_lstm_desc* c, bool save, void* stream) {
  const char* who = save ? "lstm_seq_fwd_save" : "lstm_seq_fwd";
  LstmGeom g;
  LstmArgs a;
  const int rc = lstm_args(h, c, who, g, a);
  if (rc != TADMM_OK) return rc;
  if (lstm_bad_ptr(c->Xp) || lstm_bad_ptr(c->Y) || lstm_bad_ptr(c->hT) || lstm_bad_ptr(c->cT) || lstm_bad_opt(c->h0))
    CTX_FAIL(h, TADMM_ERR_INVALID, "%s: Xp, Y, hT or cT is null, or one of them or h0 is misaligned", who);
  if (save && (lstm_bad_ptr(c->G) || lstm_bad_ptr(c->C))) CTX_FAIL(h, TADMM_ERR_INVALID, "%s: G or C is null or misaligned", who);
  const int H = g.H;
  a.Xp = c->Xp; a.h0 = c->h0; a.Y = c->Y; a.hT = c->hT; a.cT = c->cT;
  a.vx = lstm_vec(c->Xp, H); a.vh0 = lstm_vec(c->h0, H); a.vy = lstm_vec(c->Y, H); a.vhT = lstm_vec(c->hT, H);
  a.vcT = lstm_vec(c->cT, H);
  if (save) { a.G = c->G; a.C = c->C; a.vG = lstm_vec(c->G, H); a.vC = lstm_vec(c->C, H); }
  a.plane = (int64_t)4 * g.Hp * g.Kp;
  const unsigned blocks = (unsigned)((c->B + kLstmRows - 1) / kLstmRows);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  if (save) e = c->sigmoid ? lstm_fwd_tpw<true, true>(g.tpw, a, blocks, g.fwd_lds, s) : lstm_fwd_tpw<true, false>(g.tpw, a, blocks, g.fwd_lds, s);
  else e = c->sigmoid ? lstm_fwd_tpw<false, true>(g.tpw, a, blocks, g.fwd_lds, s) : lstm_fwd_tpw<false, false>(g.tpw, a, blocks, g.fwd_lds, s);
  HIP_OK(h, e);
  return TADMM_OK;
}

}  // namespace
}  // namespace tadmm

using namespace tadmm;

extern "C" {

int tadmm_lstm_desc_bytes(void) { return (int)sizeof(tadmm_lstm_desc); }

int tadmm_lstm_fits(const tadmm_lstm_desc* d, size_t* lds_bytes, int* rows_per_wg) {
  LstmGeom g;
  const int rc = lstm_geom(d, g);
  if (rc != TADMM_OK) return rc;
  if (lds_bytes) *lds_bytes = std::max(g.fwd_lds, g.bwd_lds);
  if (rows_per_wg) *rows_per_wg = kLstmRows;
  return g.fits ? 1 : 0;
}

int tadmm_lstm_seq_fwd(tadmm_handle h, const tadmm_lstm_desc* d, void* stream) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  return lstm_fwd(h, d, false, stream);
}

int tadmm_lstm_seq_fwd_save(tadmm_handle h, const tadmm_lstm_desc* d, void* stream) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  return lstm_fwd(h, d, true, stream);
}

int tadmm_lstm_seq_bwd(tadmm_handle h, const tadmm_lstm_desc* d, void* stream) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  const char* who = "lstm_seq_bwd";
  LstmGeom g;
  LstmArgs a;
  const int rc = lstm_args(h, d, who, g, a);
  if (rc != TADMM_OK) return rc;
  if (lstm_bad_ptr(d->G) || lstm_bad_ptr(d->C) || lstm_bad_ptr(d->dZ))
    CTX_FAIL(h, TADMM_ERR_INVALID, "%s: G, C or dZ is null or misaligned", who);
  if (lstm_bad_opt(d->dY) || lstm_bad_opt(d->dhT) || lstm_bad_opt(d->dcT) || lstm_bad_opt(d->dh0) || lstm_bad_opt(d->dc0))
    CTX_FAIL(h, TADMM_ERR_INVALID, "%s: dY, dhT, dcT, dh0 or dc0 is misaligned", who);
  const int H = g.H;
  a.G = d->G; a.C = d->C; a.dY = d->dY; a.dhT = d->dhT; a.dcT = d->dcT; a.dZ = d->dZ; a.dh0 = d->dh0; a.dc0 = d->dc0;
  a.vG = lstm_vec(d->G, H); a.vC = lstm_vec(d->C, H); a.vdY = lstm_vec(d->dY, H); a.vdhT = lstm_vec(d->dhT, H);
  a.vdcT = lstm_vec(d->dcT, H); a.vdZ = lstm_vec(d->dZ, H); a.vdh0 = lstm_vec(d->dh0, H); a.vdc0 = lstm_vec(d->dc0, H);
  a.plane = (int64_t)g.Hp * 4 * g.Hp;
  const unsigned blocks = (unsigned)((d->B + kLstmRows - 1) / kLstmRows);
  const hipError_t e = d->sigmoid ? lstm_bwd_tpw<true>(g.tpw, a, blocks, g.bwd_lds, (hipStream_t)stream)
                                  : lstm_bwd_tpw<false>(g.tpw, a, blocks, g.bwd_lds, (hipStream_t)stream);
  HIP_OK(h, e);
  return TADMM_OK;
}

}  // extern "C"
