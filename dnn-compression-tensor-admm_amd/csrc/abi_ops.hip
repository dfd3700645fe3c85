// The C ABI entries of include/tadmm.h that belong to no plan: handle lifetime and size queries, and the stand-alone
// operators -- ADMM penalty, grouped / single / bf16 GEMM, the forward chains of the factorised layers, Gram and
// eigen-solve of one matrix, and the building blocks of the filtered eigen-solver that the tests call directly.
#include "host.h"

using namespace tadmm;

__global__ void square_copy_kernel(const double* __restrict__ in, double* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i] * in[i];
}

static GemmDesc to_gemm_desc(const tadmm_gemm_desc& s) {   // tile counts: set_gemm_tiles
  GemmDesc g;
  memset(&g, 0, sizeof g);
  g.A = s.A; g.B = s.B; g.C = s.C; g.M = s.M; g.N = s.N; g.K = s.K;
  g.a_rs = s.a_rs; g.a_cs = s.a_cs; g.b_rs = s.b_rs; g.b_cs = s.b_cs; g.c_rs = s.c_rs; g.c_cs = s.c_cs;
  g.alpha = s.alpha; g.beta = s.beta; g.bias_n = s.bias_n; g.bias_m = s.bias_m;
  return g;
}

extern "C" {

int tadmm_version(void) { return 100; }

int tadmm_abi_sizes(int* layer_desc_bytes, int* gemm_desc_bytes) {
  if (layer_desc_bytes) *layer_desc_bytes = (int)sizeof(tadmm_layer_desc);
  if (gemm_desc_bytes) *gemm_desc_bytes = (int)sizeof(tadmm_gemm_desc);
  return TADMM_OK;
}

int tadmm_chain_desc_bytes(void) { return (int)sizeof(tadmm_chain_desc); }

int tadmm_create(int device, tadmm_handle* out) {
  if (!out) return TADMM_ERR_INVALID;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  tadmm_handle h = new tadmm_ctx_s();
  h->device = device;
  *out = h;
  if (e != hipSuccess || device < 0 || device >= count) {
    h->err = std::string("no usable HIP device ") + std::to_string(device) + " (" + hipGetErrorString(e) + ")";
    return TADMM_ERR_HIP;
  }
  return TADMM_OK;
}

int tadmm_destroy(tadmm_handle h) {
  delete h;
  return TADMM_OK;
}

const char* tadmm_last_error(tadmm_handle h) { return h ? h->err.c_str() : "null handle"; }

// ---- penalty ----
int tadmm_penalty_scratch_doubles(void) { return kPenaltyBlocks; }

int tadmm_penalty(tadmm_handle h, int n, const void* const* ptrs_dev, const int64_t* numel_dev, int64_t total_numel,
                  float rho, float grad_scale, double* loss_dev, double* partial_dev, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || n <= 0 || !ptrs_dev || !numel_dev || !loss_dev || !partial_dev) return TADMM_ERR_INVALID;
  launch_penalty(n, ptrs_dev, numel_dev, total_numel, rho, grad_scale, loss_dev, partial_dev, (hipStream_t)stream_);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

// ---- grouped GEMM ----
static bool gemm_desc_valid(const tadmm_gemm_desc& s) {
  return s.M > 0 && s.N > 0 && s.K > 0 && ((s.a_rs == 1) || (s.a_cs == 1)) && ((s.b_rs == 1) || (s.b_cs == 1));
}

// 0 for a group that tadmm_gemm_pack refuses: a negative extent must not turn into a huge tile count
size_t tadmm_gemm_pack_bytes(int n, const tadmm_gemm_desc* descs) {
  if (n <= 0 || !descs) return 0;
  size_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    if (!gemm_desc_valid(descs[i])) return 0;
    GemmDesc g = to_gemm_desc(descs[i]);
    blocks += set_gemm_tiles(g);
  }
  return align_up((size_t)n * sizeof(GemmDesc), 256) + blocks * sizeof(BlockRef);
}

int tadmm_gemm_pack(int n, const tadmm_gemm_desc* descs, void* blob_host, size_t blob_bytes, int* nblocks_out) {
  if (n <= 0 || !descs || !blob_host || !nblocks_out) return TADMM_ERR_INVALID;
  for (int i = 0; i < n; ++i)       // shapes and strides first: the byte count of an invalid group means nothing
    if (!gemm_desc_valid(descs[i])) return TADMM_ERR_INVALID;
  if (blob_bytes < tadmm_gemm_pack_bytes(n, descs)) return TADMM_ERR_WORKSPACE;
  GemmDesc* gd = (GemmDesc*)blob_host;
  BlockRef* map = (BlockRef*)((char*)blob_host + align_up((size_t)n * sizeof(GemmDesc), 256));
  int nb = 0;
  for (int i = 0; i < n; ++i) {
    gd[i] = to_gemm_desc(descs[i]);
    const int nt = (int)set_gemm_tiles(gd[i]);
    for (int b = 0; b < nt; ++b) map[nb++] = BlockRef{i, b};
  }
  *nblocks_out = nb;
  return TADMM_OK;
}

int tadmm_gemm_run(tadmm_handle h, const void* blob_dev, int n, int nblocks, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !blob_dev || n <= 0 || nblocks <= 0) return TADMM_ERR_INVALID;
  const GemmDesc* gd = (const GemmDesc*)blob_dev;
  const BlockRef* map = (const BlockRef*)((const char*)blob_dev + align_up((size_t)n * sizeof(GemmDesc), 256));
  launch_gemm(gd, map, nblocks, (hipStream_t)stream_);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_gemm(tadmm_handle h, const tadmm_gemm_desc* sdesc, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !sdesc) return TADMM_ERR_INVALID;
  const tadmm_gemm_desc& s = *sdesc;
  if (s.M <= 0 || s.N <= 0 || s.K <= 0 || !s.A || !s.B || !s.C) CTX_FAIL(h, TADMM_ERR_INVALID, "tadmm_gemm: empty operand");
  if (!((s.a_rs == 1) || (s.a_cs == 1)) || !((s.b_rs == 1) || (s.b_cs == 1)))
    CTX_FAIL(h, TADMM_ERR_INVALID, "tadmm_gemm: each operand needs one unit stride");
  GemmDesc g = to_gemm_desc(s);
  set_gemm_tiles(g);
  launch_gemm_one(g, (hipStream_t)stream_);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_gemm_bf16_nt(tadmm_handle h, const void* A, const void* Bt, void* C, int M, int N, int K, int64_t lda,
                       int64_t ldb, int64_t ldc, const float* bias_n, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !A || !Bt || !C) return TADMM_ERR_INVALID;
  if (M <= 0 || N <= 0 || K <= 0 || lda < K || ldb < K || ldc < N) CTX_FAIL(h, TADMM_ERR_INVALID, "tadmm_gemm_bf16_nt: bad shape");
  launch_gemm_bf16_nt(A, Bt, C, M, N, K, lda, ldb, ldc, bias_n, (hipStream_t)stream_);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

// ---- forward chains of the factorised layers (chain.hip) ----
// `save`: the _save entries, which also store the true-rank columns [0, rt) of the middle-rank vector to h_out
static int chain_entry(tadmm_handle h, const tadmm_chain_desc* c, int fused, const char* who, void* stream_,
                       bool svdconv = false, bool save = false, int rt = 0, void* h_out = nullptr, int64_t ldh = 0) {
  DeviceGuard device_guard(h);
  if (!h || !c) return TADMM_ERR_INVALID;
  if (save) {
    if (c->dtype != TADMM_CHAIN_F32 && c->dtype != TADMM_CHAIN_BF16)
      CTX_FAIL(h, TADMM_ERR_INVALID, "chain save: float32 or bfloat16 only (binary16 is inference only: the weight gradients have no binary16 form)");
    if (!h_out) CTX_FAIL(h, TADMM_ERR_INVALID, "chain save: null h_out");
    if (rt <= 0 || rt > c->R) CTX_FAIL(h, TADMM_ERR_INVALID, "chain save: true rank %d outside (0, %d]", rt, c->R);
    if (ldh < rt) CTX_FAIL(h, TADMM_ERR_INVALID, "chain save: ldh %lld below the true rank %d", (long long)ldh, rt);
    if (((uintptr_t)h_out) % (c->dtype == TADMM_CHAIN_F32 ? 4 : 2))
      CTX_FAIL(h, TADMM_ERR_INVALID, "chain save: h_out must be aligned to its element");
  }
  if (svdconv) {   // 1x1 SVD convolution: NCHW in, NCHW out, one plane size, T = batch * plane
    if (c->x_hw <= 0 || c->y_hw != c->x_hw)
      CTX_FAIL(h, TADMM_ERR_INVALID, "svdconv: x_hw and y_hw must both equal the pixels of one image plane (H*W > 0)");
    if (c->T % c->x_hw) CTX_FAIL(h, TADMM_ERR_INVALID, "svdconv: T must be batch * H*W (a whole number of planes)");
    if (c->R % 64 || c->R > 256)
      CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "svdconv: middle rank must be padded to a multiple of 64, at most 256 (larger ranks take two tadmm_tucker_1x1 launches)");
  }
  if (!c->X || !c->Y || !c->Win || (fused && !c->Wout)) CTX_FAIL(h, TADMM_ERR_INVALID, "chain: null operand");
  if (c->T < 0 || c->Kin <= 0 || c->R <= 0 || (fused && c->Nout <= 0)) CTX_FAIL(h, TADMM_ERR_INVALID, "chain: bad shape");
  if (c->dtype != TADMM_CHAIN_F32 && c->dtype != TADMM_CHAIN_BF16 && c->dtype != TADMM_CHAIN_F16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "chain: bad dtype");
  const int epl = c->dtype == TADMM_CHAIN_F32 ? 4 : 8;          // elements per 16-byte load of X
  const int64_t ks1 = (c->Kin + 31) / 32, nt1 = (c->R + 15) / 16;
  if ((((uintptr_t)c->Win) & 15) || c->win_plane < nt1 * ks1 * 512 || (c->win_plane & 7))
    CTX_FAIL(h, TADMM_ERR_INVALID, "chain: Win planes must be 16-byte aligned fragment-major images of ceil(R/16) x ceil(Kin/32) KiB blocks");
  if (c->x_hw == 0 && (c->ldx < c->Kin || c->Kin % epl || c->ldx % epl || (((uintptr_t)c->X) & 15)))
    CTX_FAIL(h, TADMM_ERR_INVALID, "chain: X rows must be 16-byte aligned with Kin a whole number of 16-byte vectors");
  if (c->y_hw == 0 && c->ldy < (fused ? c->Nout : c->R)) CTX_FAIL(h, TADMM_ERR_INVALID, "chain: ldy too small");
  if (c->x_hw < 0 || c->y_hw < 0) CTX_FAIL(h, TADMM_ERR_INVALID, "chain: negative image size");
  // the vector image epilogue masks a 16-byte unit by its first pixel: a partial last plane would be overrun
  if ((c->x_hw > 0 && c->T % c->x_hw) || (c->y_hw > 0 && c->T % c->y_hw))
    CTX_FAIL(h, TADMM_ERR_INVALID, "chain: T must be a whole number of image planes (T % x_hw == 0 and T % y_hw == 0)");
  if (((uintptr_t)c->bias) & 15) CTX_FAIL(h, TADMM_ERR_INVALID, "chain: bias must be 16-byte aligned");
  if (fused) {
    if (c->R % 64 || c->R > 256) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "chain: fused middle rank must be a multiple of 64, at most 256");
    const int64_t nt2 = (c->Nout + 15) / 16;
    if ((((uintptr_t)c->Wout) & 15) || c->wout_plane < nt2 * (c->R / 32) * 512 || (c->wout_plane & 7))
      CTX_FAIL(h, TADMM_ERR_INVALID, "chain: Wout planes must be 16-byte aligned fragment-major images of ceil(Nout/16) x R/32 KiB blocks");
  }
  if (c->tile_tokens != 0 && c->tile_tokens != 32 && c->tile_tokens != 64) CTX_FAIL(h, TADMM_ERR_INVALID, "chain: tile_tokens");
  ChainDesc d;
  memset(&d, 0, sizeof d);
  d.X = c->X; d.Y = c->Y; d.Win = (const uint16_t*)c->Win; d.Wout = (const uint16_t*)c->Wout; d.bias = c->bias;
  d.T = c->T; d.Kin = c->Kin; d.R = c->R; d.Nout = c->Nout;
  d.ldx = c->ldx; d.ldy = c->ldy;
  d.win_plane = c->win_plane; d.wout_plane = c->wout_plane;
  d.x_hw = c->x_hw; d.y_hw = c->y_hw; d.fused = fused;
  d.x_vec = (c->x_hw > 0 && c->x_hw % epl == 0 && (((uintptr_t)c->X) & 15) == 0) ? 1 : 0;
  const int nfeat = fused ? c->Nout : c->R;
  if (c->y_hw > 0) d.y_vec = (c->y_hw % epl == 0 && (((uintptr_t)c->Y) & 15) == 0) ? 1 : 0;
  else d.y_vec = (c->ldy % epl == 0 && nfeat % epl == 0 && (((uintptr_t)c->Y) & 15) == 0) ? 1 : 0;
  if (save) {   // 16-byte stores where every unit is aligned and, on images, lies within one plane
    d.H = h_out; d.ldh = ldh; d.rt = rt;
    d.h_vec = ((svdconv ? c->x_hw % epl : ldh % epl) == 0 && (((uintptr_t)h_out) & 15) == 0) ? 1 : 0;
  }
  const int rc = svdconv ? launch_svdconv_chain(d, c->dtype, c->tile_tokens, (hipStream_t)stream_)
                         : launch_tt_chain(d, c->dtype, c->tile_tokens, (hipStream_t)stream_);
  if (rc > 0) CTX_FAIL(h, TADMM_ERR_HIP, "chain: dynamic-LDS opt-in failed: %s", hipGetErrorString((hipError_t)rc));
  if (rc != 0) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "chain: token tile does not fit the LDS");
  HIP_OK(h, hipGetLastError());
  (void)who;
  return TADMM_OK;
}
int tadmm_ttlinear_fwd(tadmm_handle h, const tadmm_chain_desc* d, void* s) { return chain_entry(h, d, 1, "ttlinear_fwd", s); }
int tadmm_ttlinear_bwd(tadmm_handle h, const tadmm_chain_desc* d, void* s) { return chain_entry(h, d, 1, "ttlinear_bwd", s); }
int tadmm_ttconv_chain_in(tadmm_handle h, const tadmm_chain_desc* d, void* s) { return chain_entry(h, d, 0, "ttconv_chain_in", s); }
int tadmm_ttconv_chain_out(tadmm_handle h, const tadmm_chain_desc* d, void* s) { return chain_entry(h, d, 0, "ttconv_chain_out", s); }
int tadmm_tucker_1x1(tadmm_handle h, const tadmm_chain_desc* d, void* s) { return chain_entry(h, d, 0, "tucker_1x1", s); }
int tadmm_svdconv_fwd(tadmm_handle h, const tadmm_chain_desc* d, void* s) { return chain_entry(h, d, 1, "svdconv_fwd", s, true); }
int tadmm_svdconv_bwd(tadmm_handle h, const tadmm_chain_desc* d, void* s) { return chain_entry(h, d, 1, "svdconv_bwd", s, true); }
int tadmm_ttlinear_fwd_save(tadmm_handle h, const tadmm_chain_desc* d, int r, void* h_out, int64_t ldh, void* s) {
  return chain_entry(h, d, 1, "ttlinear_fwd_save", s, false, true, r, h_out, ldh);
}
int tadmm_ttlinear_bwd_save(tadmm_handle h, const tadmm_chain_desc* d, int r, void* dh_out, int64_t ldh, void* s) {
  return chain_entry(h, d, 1, "ttlinear_bwd_save", s, false, true, r, dh_out, ldh);
}
int tadmm_svdconv_fwd_save(tadmm_handle h, const tadmm_chain_desc* d, int r, void* h_out, int64_t ldh, void* s) {
  return chain_entry(h, d, 1, "svdconv_fwd_save", s, true, true, r, h_out, ldh);
}
int tadmm_svdconv_bwd_save(tadmm_handle h, const tadmm_chain_desc* d, int r, void* dh_out, int64_t ldh, void* s) {
  return chain_entry(h, d, 1, "svdconv_bwd_save", s, true, true, r, dh_out, ldh);
}

int tadmm_conv_chain_desc_bytes(void) { return (int)sizeof(tadmm_conv_chain_desc); }

// Extents, geometry and tiling shared by the forward, the data gradient and the host-only plan.  Fills the kernel's
// descriptor in the roles of `mode` (forward: source = X on H x W, destination = Y on Ho x Wo; data gradient: source = dY
// on Ho x Wo, destination = dX on H x W, the ranks and channel counts swapped) without touching an operand.
static int conv_chain_shape(tadmm_handle h, const tadmm_conv_chain_desc* c, int mode, ConvChainDesc& d, size_t* lds) {
  if (c->dtype != TADMM_CHAIN_F32 && c->dtype != TADMM_CHAIN_BF16 && c->dtype != TADMM_CHAIN_F16)
    CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: bad dtype");
  if (c->B < 0 || c->C <= 0 || c->Nout <= 0 || c->H <= 0 || c->W <= 0 || c->kh <= 0 || c->kw <= 0 || c->stride_h <= 0 ||
      c->stride_w <= 0 || c->dil_h <= 0 || c->dil_w <= 0 || c->pad_h < 0 || c->pad_w < 0)
    CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: bad geometry");
  const int ho = (c->H + 2 * c->pad_h - c->dil_h * (c->kh - 1) - 1) / c->stride_h + 1;
  const int wo = (c->W + 2 * c->pad_w - c->dil_w * (c->kw - 1) - 1) / c->stride_w + 1;
  if (ho != c->Ho || wo != c->Wo) CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: output size does not match the geometry");
  if (mode == TADMM_CONV_CHAIN_FWD) {
    if (ho <= 0 || wo <= 0 || wo > 64) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "conv chain: output rows of more than 64 pixels take the three-launch path");
  } else {
    if (ho <= 0 || wo <= 0) CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: empty output plane");
    if (c->W > 64) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "conv chain: input rows of more than 64 pixels take the three data-gradient launches");
  }
  if (c->R1 <= 0 || c->R2 <= 0 || c->R1 % 32 || c->R2 % 32 || c->R1 > 256 || c->R2 > 256)
    CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "conv chain: ranks must be padded to multiples of 32 and at most 256");
  memset(&d, 0, sizeof d);
  d.B = c->B; d.kh = c->kh; d.kw = c->kw; d.sh = c->stride_h; d.sw = c->stride_w;
  d.ph = c->pad_h; d.pw = c->pad_w; d.dh = c->dil_h; d.dw = c->dil_w;
  if (mode == TADMM_CONV_CHAIN_FWD) {
    d.C = c->C; d.R1 = c->R1; d.R2 = c->R2; d.Nout = c->Nout; d.H = c->H; d.W = c->W; d.Ho = ho; d.Wo = wo;
  } else {
    d.C = c->Nout; d.R1 = c->R2; d.R2 = c->R1; d.Nout = c->C; d.H = ho; d.W = wo; d.Ho = c->H; d.Wo = c->W; d.transposed = 1;
  }
  if (!plan_tt_conv(d, c->dtype, lds)) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "conv chain: halo or intermediates do not fit the LDS");
  return TADMM_OK;
}

// weight planes of the kernel's three products, in the kernel's roles
static bool conv_chain_planes_ok(const tadmm_conv_chain_desc* c, const ConvChainDesc& d) {
  const int64_t taps = (int64_t)c->kh * c->kw;
  return !((((uintptr_t)c->W1) & 15) || (((uintptr_t)c->W2) & 15) || (((uintptr_t)c->W3) & 15) ||
           c->w1_plane < (int64_t)(d.R1 / 16) * ((d.C + 31) / 32) * 512 || c->w2_plane < (int64_t)(d.R2 / 16) * taps * (d.R1 / 32) * 512 ||
           c->w3_plane < (int64_t)((d.Nout + 15) / 16) * (d.R2 / 32) * 512);
}

static void conv_chain_operands(const tadmm_conv_chain_desc* c, ConvChainDesc& d) {
  d.X = c->X; d.Y = c->Y; d.W1 = (const uint16_t*)c->W1; d.W2 = (const uint16_t*)c->W2; d.W3 = (const uint16_t*)c->W3;
  d.w1_plane = c->w1_plane; d.w2_plane = c->w2_plane; d.w3_plane = c->w3_plane;
  const int epl = c->dtype == TADMM_CHAIN_F32 ? 4 : 8;
  d.x_vec = ((d.H * d.W) % epl == 0 && (((uintptr_t)c->X) & 15) == 0) ? 1 : 0;
}

static int conv_chain_launch(tadmm_handle h, const ConvChainDesc& d, int dtype, hipStream_t s) {
  const int rc = launch_tt_conv(d, dtype, s);
  if (rc > 0) CTX_FAIL(h, TADMM_ERR_HIP, "conv chain: dynamic-LDS opt-in failed: %s", hipGetErrorString((hipError_t)rc));
  if (rc != 0) CTX_FAIL(h, TADMM_ERR_UNSUPPORTED, "conv chain: the intermediates do not fit the LDS");
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_ttconv_fused(tadmm_handle h, const tadmm_conv_chain_desc* c, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !c) return TADMM_ERR_INVALID;
  if (!c->X || !c->Y || !c->W1 || !c->W2 || !c->W3) CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: null operand");
  ConvChainDesc d;
  const int rc = conv_chain_shape(h, c, TADMM_CONV_CHAIN_FWD, d, nullptr);
  if (rc != TADMM_OK) return rc;
  if (!conv_chain_planes_ok(c, d) || (((uintptr_t)c->bias) & 15))
    CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: weight planes too small or misaligned");
  conv_chain_operands(c, d);
  d.bias = c->bias;
  return conv_chain_launch(h, d, c->dtype, (hipStream_t)stream_);
}

// forward with saved intermediates (mode FWD) and data gradient (mode BWD): statuses as tadmm_core_conv_*
static int conv_chain_train(tadmm_handle h, const tadmm_conv_chain_desc* c, int mode, int r1, int r2, void* s1, void* s2,
                            void* stream_) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  if (!c) CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: null descriptor");
  if (c->dtype == TADMM_CHAIN_F16)   // these outputs feed the weight gradients, which take float32 and bfloat16 only
    CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: binary16 is inference only (tadmm_ttconv_fused)");
  ConvChainDesc d;
  const int rc = conv_chain_shape(h, c, mode, d, nullptr);
  if (rc != TADMM_OK) return rc;
  if (r1 <= 0 || r1 > c->R1 || r2 <= 0 || r2 > c->R2)
    CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: true ranks (%d, %d) outside (0, %d] x (0, %d]", r1, r2, c->R1, c->R2);
  const bool bwd = mode == TADMM_CONV_CHAIN_BWD;
  if (!bwd && (!s1 || !s2) && c->B > 0) CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: null intermediate (H1, H2)");
  if (bwd && (s1 == nullptr) != (s2 == nullptr)) CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: dH1 and dH2 are saved together or not at all");
  if (c->B > 0 && (!c->X || !c->Y || !c->W1 || !c->W2 || !c->W3)) CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: null operand");
  const uintptr_t esz = c->dtype == TADMM_CHAIN_F32 ? 4 : 2;
  if (((uintptr_t)c->X | (uintptr_t)c->Y | (uintptr_t)s1 | (uintptr_t)s2) & (esz - 1))
    CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: misaligned operand");
  if (!conv_chain_planes_ok(c, d) || (!bwd && (((uintptr_t)c->bias) & 15)))
    CTX_FAIL(h, TADMM_ERR_INVALID, "conv chain: weight planes too small or misaligned");
  if (c->B == 0) return TADMM_OK;
  conv_chain_operands(c, d);
  d.bias = bwd ? nullptr : c->bias;
  // S1 is product 1's tensor, S2 product 2's: H1, H2 forward; dH2, dH1 in the data gradient
  d.S1 = bwd ? s2 : s1; d.S2 = bwd ? s1 : s2;
  d.r1t = bwd ? r2 : r1; d.r2t = bwd ? r1 : r2;
  return conv_chain_launch(h, d, c->dtype, (hipStream_t)stream_);
}

int tadmm_ttconv_fused_save(tadmm_handle h, const tadmm_conv_chain_desc* d, int r1, int r2, void* H1, void* H2, void* stream) {
  return conv_chain_train(h, d, TADMM_CONV_CHAIN_FWD, r1, r2, H1, H2, stream);
}

int tadmm_ttconv_fused_bwd(tadmm_handle h, const tadmm_conv_chain_desc* d, int r1, int r2, void* dH1, void* dH2, void* stream) {
  return conv_chain_train(h, d, TADMM_CONV_CHAIN_BWD, r1, r2, dH1, dH2, stream);
}

int tadmm_ttconv_fused_plan(const tadmm_conv_chain_desc* c, int mode, int* tile_pixels, int* tile_rows, int* halo_tiles,
                            int* tiles_per_image, size_t* lds_bytes) {
  if (!c || (mode != TADMM_CONV_CHAIN_FWD && mode != TADMM_CONV_CHAIN_BWD)) return TADMM_ERR_INVALID;
  ConvChainDesc d;
  size_t lds = 0;
  const int rc = conv_chain_shape(nullptr, c, mode, d, &lds);
  if (rc != TADMM_OK) return rc;
  if (tile_pixels) *tile_pixels = d.TM;
  if (tile_rows) *tile_rows = d.TR;
  if (halo_tiles) *halo_tiles = d.NT;
  if (tiles_per_image) *tiles_per_image = d.tiles;
  if (lds_bytes) *lds_bytes = lds;
  return TADMM_OK;
}

// ---- k x k core convolution of the factorised layers (coreconv.hip; its weight gradient lives in wgrad.hip) ----
int tadmm_core_conv_desc_bytes(void) { return (int)sizeof(tadmm_core_conv_desc); }

int tadmm_core_conv_fwd(tadmm_handle h, const tadmm_core_conv_desc* d, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  return launch_core_conv(h, d, 0, (hipStream_t)stream_);
}

int tadmm_core_conv_dgrad(tadmm_handle h, const tadmm_core_conv_desc* d, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h) return TADMM_ERR_INVALID;
  return launch_core_conv(h, d, 1, (hipStream_t)stream_);
}

// ---- standalone Gram / eigh (tests, Tucker path) ----
// ~256 Gram workgroups for the one problem of a launch (the plans, whose levels batch 15-30 problems, ask for 64 each
// and cap the K chunk)
static EigGeom gram_geom(int m, int n) { return eig_geom(m, n, 256, false); }

size_t tadmm_gram_scratch_bytes(int m, int n) {
  const EigGeom st = gram_geom(m, n);
  const size_t ntp = (size_t)st.nt * (st.nt + 1) / 2;
  const size_t nblk_p = (size_t)st.ksplit * ntp;
  const size_t nblk_r = ((size_t)st.Npad * st.ld + 1023) / 1024;
  return align_up(st.ksplit * ntp * 1024 * 8, 256) + align_up(sizeof(GramDesc), 256) +
         align_up(nblk_p * sizeof(BlockRef), 256) + align_up(nblk_r * sizeof(BlockRef), 256);
}

int tadmm_gram_ld(int m, int n, int* Npad, int* ld) {
  const EigGeom st = gram_geom(m, n);
  if (Npad) *Npad = st.Npad;
  if (ld) *ld = st.ld;
  return st.N;
}

int tadmm_gram_f64(tadmm_handle h, const float* A, int m, int n, double* G, int ldg, void* scratch, size_t scratch_bytes,
                   void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !A || !G || !scratch || m <= 0 || n <= 0) return TADMM_ERR_INVALID;
  const EigGeom st = gram_geom(m, n);
  if (ldg != st.ld) CTX_FAIL(h, TADMM_ERR_INVALID, "ldg must be %d (tadmm_gram_ld)", st.ld);
  if (scratch_bytes < tadmm_gram_scratch_bytes(m, n)) CTX_FAIL(h, TADMM_ERR_WORKSPACE, "gram scratch too small");
  hipStream_t s = (hipStream_t)stream_;
  const size_t ntp = (size_t)st.nt * (st.nt + 1) / 2;
  char* base = (char*)scratch;
  size_t off = 0;
  double* partial = (double*)(base + off); off += align_up(st.ksplit * ntp * 1024 * 8, 256);
  GramDesc* gdev = (GramDesc*)(base + off); off += align_up(sizeof(GramDesc), 256);
  std::vector<BlockRef> mp, mr;
  for (int b = 0; b < (int)(st.ksplit * ntp); ++b) mp.push_back(BlockRef{0, b});
  if (st.ksplit > 1)   // ksplit == 1: the product kernel writes G itself
    for (int b = 0; b < (int)(((size_t)st.Npad * st.ld + 1023) / 1024); ++b) mr.push_back(BlockRef{0, b});
  BlockRef* mpd = (BlockRef*)(base + off); off += align_up(mp.size() * sizeof(BlockRef), 256);
  BlockRef* mrd = (BlockRef*)(base + off);
  GramDesc gd;
  memset(&gd, 0, sizeof gd);
  gd.A = A; gd.m = m; gd.n = n; gd.trans = st.trans; gd.N = st.N; gd.K = st.trans ? m : n; gd.nt = st.nt;
  gd.ksplit = st.ksplit; gd.kchunk = st.kchunk; gd.partial = partial; gd.G = G; gd.Npad = st.Npad; gd.ld = st.ld;
  HIP_OK(h, hipMemcpyAsync(gdev, &gd, sizeof gd, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(mpd, mp.data(), mp.size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(mrd, mr.data(), mr.size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
  HIP_OK(h, hipStreamSynchronize(s));   // host vectors die at return
  launch_gram_partial(gdev, mpd, (int)mp.size(), s);
  launch_gram_reduce(gdev, mrd, (int)mr.size(), s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

size_t tadmm_eigh_scratch_bytes(int N) {
  const EigGeom g = eig_geom(N, N, 64, true);
  const size_t Npad = g.Npad, ld = g.ld;
  return align_up(Npad * ld * 8, 256) + align_up(sizeof(EigDesc), 256) + 3 * align_up(Npad * sizeof(BlockRef), 256) +
         align_up(Npad * 8, 256) * 2 + align_up(Npad * 4, 256) + 1024 + align_up((Npad / 16) * 256 * 8, 256);
}

// The leading r pairs of G; *route_out (nullable): 0 direct route (tridiag.hip), 1 jacobi_small_kernel, 2 tournament.
static int eigh_leading(tadmm_handle h, const double* G, int N, int r, double* evals_out, double* evecs_out,
                        void* scratch, size_t scratch_bytes, int* sweeps_out, int* route_out, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !G || !evals_out || !evecs_out || !scratch || N <= 0 || r < 1 || r > N) return TADMM_ERR_INVALID;
  if (scratch_bytes < tadmm_eigh_scratch_bytes(N)) CTX_FAIL(h, TADMM_ERR_WORKSPACE, "eigh scratch too small");
  hipStream_t s = (hipStream_t)stream_;
  const EigGeom geo = eig_geom(N, N, 64, true);
  const int Npad = geo.Npad, ld = geo.ld;
  char* base = (char*)scratch;
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  double* XT = (double*)(base + carve((size_t)Npad * ld * 8));
  const size_t o_desc = carve(sizeof(EigDesc));
  EigDesc* edev = (EigDesc*)(base + o_desc);
  // the group layout of this one problem, with offsets into the scratch instead of a plan's workspace
  EigLayout L;
  Phase* phases[3] = {&L.tick, &L.norm, &L.ext};
  size_t o_map[3];
  for (size_t& o : o_map) o = carve(Npad * sizeof(BlockRef));
  double* lam = (double*)(base + carve((size_t)Npad * 8));
  double* sigma = (double*)(base + carve((size_t)Npad * 8));
  int32_t* order = (int32_t*)(base + carve((size_t)Npad * 4));
  double* offs = (double*)(base + off); off += 64;
  int32_t* done = (int32_t*)(base + off); off += 64;
  double* sblk = (double*)(base + off);
  HIP_OK(h, hipMemsetAsync(XT, 0, (size_t)Npad * ld * 8, s));
  HIP_OK(h, hipMemcpy2DAsync(XT, (size_t)ld * 8, G, (size_t)N * 8, (size_t)N * 8, N, hipMemcpyDeviceToDevice, s));
  std::vector<EigDesc> ev(1);
  EigDesc& e = ev[0];
  memset(&e, 0, sizeof e);
  e.XT = XT; e.N = N; e.Npad = Npad; e.ld = ld; e.nb = geo.nb; e.off = offs; e.done = done; e.lam = lam; e.order = order;
  e.sigma = sigma; e.r = r; e.mode = 2; e.out_a = nullptr; e.out_b = nullptr; e.evec_out = evecs_out;
  e.sblk = sblk;
  EigMaps maps;
  if (const int rc = eig_maps(h, L, ev, false, maps)) return rc;
  const std::vector<BlockRef>* mv[3] = {&maps.tick, &maps.norm, &maps.ext};
  HIP_OK(h, hipMemcpyAsync(edev, &e, sizeof e, hipMemcpyHostToDevice, s));
  for (int i = 0; i < 3; ++i) {
    phases[i]->desc_off = o_desc;
    phases[i]->map_off = o_map[i];
    HIP_OK(h, hipMemcpyAsync(base + o_map[i], mv[i]->data(), mv[i]->size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
  }
  HIP_OK(h, hipStreamSynchronize(s));
  const bool super = L.kernel == EigTick::SuperPairs;
  const int units = L.players[0];
  const BlockRef* m_tick = (const BlockRef*)(base + L.tick.map_off);
  const double tol = 1e-9;
  int tick = 0, gs = 0;
  bool conv = false;
  // problems of at most 64 columns take the route the plans take (run_eig_group): the direct solver of tridiag.hip, then
  // jacobi_small_kernel for whatever that one did not certify.  TADMM_EIGH_TICK=1 keeps them on the tournament kernels.
  if (jacobi_small_fits(Npad) && !(getenv("TADMM_EIGH_TICK") && atoi(getenv("TADMM_EIGH_TICK")))) {
    int32_t* fast = done + 4;                 // device words inside the 64-byte `done` slot: [4] direct-solver flag,
    int* verdict = (int*)(done + 8);          // [8..9] verdict of the single-launch solvers
    HIP_OK(h, hipMemsetAsync(done, 0, 64, s));
    const bool direct = eig_small_direct_on();
    if (direct) HIP_OK(h, launch_eig_small_direct(edev, 1, nullptr, fast, verdict, s));
    HIP_OK(h, launch_jacobi_small(edev, 1, Npad, tol, 60, nullptr, verdict, s, false, direct ? fast : nullptr));
    int hv[6] = {0, 0, 0, 0, 0, 0};
    HIP_OK(h, hipMemcpyAsync(hv, done + 4, sizeof hv, hipMemcpyDeviceToHost, s));
    HIP_OK(h, hipStreamSynchronize(s));
    conv = hv[5] != 0;                        // verdict[1]
    gs = hv[0] ? 0 : 1;                       // 0 sweeps: solved by the direct route
    if (sweeps_out) *sweeps_out = gs;
    if (route_out) *route_out = hv[0] ? 0 : 1;
    if (!conv) CTX_FAIL(h, TADMM_ERR_NOCONVERGE, "small eigen-solve did not converge");
  } else {
  if (route_out) *route_out = 2;
  launch_jacobi_init(edev, 1, s);
  double hoff[3];
  int hdone = 0;
  for (; gs < 40 && !conv; ++gs) {
    for (int t = 0; t < units - 1; ++t, ++tick) {
      if (super) {
        HIP_OK(h, launch_jacobi_tick3(edev, m_tick, L.tick.nblocks, tick, tol, ld, s));
      } else {
        HIP_OK(h, launch_jacobi_tick(edev, m_tick, L.tick.nblocks, tick, tol, L.tick_lds, s));
      }
    }
    HIP_OK(h, hipMemcpyAsync(hoff, offs, 24, hipMemcpyDeviceToHost, s));
    HIP_OK(h, hipMemcpyAsync(&hdone, done, 4, hipMemcpyDeviceToHost, s));
    HIP_OK(h, hipStreamSynchronize(s));
    conv = hdone || hoff[gs & 1] < tol;
  }
  if (sweeps_out) *sweeps_out = gs;
  if (getenv("TADMM_STAMPS_DUMP")) { (void)hipStreamSynchronize(s); dump_stamps(); }   // -DTADMM_STAMPS builds only
  if (!conv) CTX_FAIL(h, TADMM_ERR_NOCONVERGE, "Jacobi did not converge in 40 sweeps");
  }
  L.finalize(base, s, nullptr);
  HIP_OK(h, hipGetLastError());
  // eigenvalues in descending order = sigma^2, squared on the device to stay allocation-free
  hipLaunchKernelGGL(square_copy_kernel, dim3((r + 255) / 256), dim3(256), 0, s, sigma, evals_out, r);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

int tadmm_eigh_f64(tadmm_handle h, const double* G, int N, double* evals_out, double* evecs_out, void* scratch,
                   size_t scratch_bytes, int* sweeps_out, void* stream_) {
  return eigh_leading(h, G, N, N, evals_out, evecs_out, scratch, scratch_bytes, sweeps_out, nullptr, stream_);
}

int tadmm_eigh_partial_f64(tadmm_handle h, const double* G, int N, int r, double* evals_out, double* evecs_out,
                           void* scratch, size_t scratch_bytes, int* route_out, void* stream_) {
  return eigh_leading(h, G, N, r, evals_out, evecs_out, scratch, scratch_bytes, nullptr, route_out, stream_);
}

// ---- building blocks of the filtered eigen-solver, exposed for tests ----
size_t tadmm_dgemm_scratch_bytes(int M, int N) {
  return align_up(sizeof(DgemmDesc), 256) + align_up((size_t)(M / 32) * (N / 32) * sizeof(BlockRef), 256);
}

int tadmm_dgemm_f64(tadmm_handle h, const double* A, const double* B, double* C, int M, int N, int K, int lda, int ldb,
                    int ldc, int b_transposed, void* scratch, size_t scratch_bytes, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !A || !B || !C || !scratch) return TADMM_ERR_INVALID;
  if (M <= 0 || N <= 0 || K <= 0 || M % 32 || N % 32 || K % 16 || (lda & 1) || (ldb & 1) || (ldc & 1))
    CTX_FAIL(h, TADMM_ERR_INVALID, "tadmm_dgemm_f64: M, N multiples of 32, K of 16, even leading dimensions");
  if (scratch_bytes < tadmm_dgemm_scratch_bytes(M, N)) CTX_FAIL(h, TADMM_ERR_WORKSPACE, "dgemm scratch too small");
  hipStream_t s = (hipStream_t)stream_;
  DgemmDesc g;
  memset(&g, 0, sizeof g);
  g.A = A; g.B = B; g.C = C; g.selA = g.selB = g.selC = g.selP = g.selQ = -1;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.tiles_m = M / 32; g.tiles_n = N / 32;
  std::vector<BlockRef> map;
  for (int b = 0; b < g.tiles_m * g.tiles_n; ++b) map.push_back(BlockRef{0, b});
  DgemmDesc* gd = (DgemmDesc*)scratch;
  BlockRef* md = (BlockRef*)((char*)scratch + align_up(sizeof(DgemmDesc), 256));
  HIP_OK(h, hipMemcpyAsync(gd, &g, sizeof g, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(md, map.data(), map.size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
  HIP_OK(h, hipStreamSynchronize(s));
  if (b_transposed && K % 32 == 0 && !getenv("TADMM_DGEMM_OLD")) {        // the 64x64 LDS-staged kernel (what the filter uses)
    std::vector<BlockRef> m64;
    for (int b = 0; b < ((M + 63) / 64) * ((N + 63) / 64); ++b) m64.push_back(BlockRef{0, b});
    HIP_OK(h, hipMemcpyAsync(md, m64.data(), m64.size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
    HIP_OK(h, hipStreamSynchronize(s));
    launch_dgemm_nt64(gd, md, (int)m64.size(), s);
  } else {
    launch_dgemm(gd, md, (int)map.size(), b_transposed != 0, s);
  }
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

// C[M][N] = A[M][K] * G[N][K]^T at fp32 accuracy on the bf16 matrix cores (dgemm3.hip), the products the filter's early
// stages use: packs G into its three fragment-major planes, then one launch.  M % 32 == 0, N = K, N % 32 == 0.
size_t tadmm_dgemm3_scratch_bytes(int M, int N) {
  const size_t planes = (size_t)3 * (N / 16) * (N / 32) * 512 * 2;
  return align_up(sizeof(DgemmDesc), 256) + align_up(sizeof(GPlaneDesc), 256) + align_up(planes, 256) +
         2 * align_up(((size_t)(M / 32) * ((N + 63) / 64) + (size_t)(N / 16) * (N / 32) / 4 + 8) * sizeof(BlockRef), 256);
}

int tadmm_dgemm3_f64(tadmm_handle h, const double* A, const double* Gm, double* C, int M, int N, int lda, int ldg, int ldc,
                     int repeats, void* scratch, size_t scratch_bytes, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !A || !Gm || !C || !scratch) return TADMM_ERR_INVALID;
  if (M <= 0 || N <= 0 || M % 32 || N % 32 || lda < N || ldg < N || ldc < N || (lda & 1) || (ldg & 1) || (ldc & 1))
    CTX_FAIL(h, TADMM_ERR_INVALID, "tadmm_dgemm3_f64: M, N multiples of 32, even leading dimensions >= N");
  if (scratch_bytes < tadmm_dgemm3_scratch_bytes(M, N)) CTX_FAIL(h, TADMM_ERR_WORKSPACE, "dgemm3 scratch too small");
  hipStream_t s = (hipStream_t)stream_;
  char* base = (char*)scratch;
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off += align_up(b, 256); return o; };
  const size_t o_g = take(sizeof(DgemmDesc)), o_p = take(sizeof(GPlaneDesc));
  const int nt = N / 16, ks = N / 32;
  const int64_t plane = (int64_t)nt * ks * 512;
  const size_t o_planes = take((size_t)3 * plane * 2);
  std::vector<BlockRef> m_gp, m_fast;
  for (int b = 0; b < (nt * ks + 3) / 4; ++b) m_gp.push_back(BlockRef{0, b});
  const int tn = (N + 63) / 64;
  for (int b = 0; b < (M / 32) * tn; ++b) m_fast.push_back(BlockRef{0, b});
  xcd_by_key(m_fast, [&](const BlockRef& b) { return b.local % tn; });
  const size_t o_mgp = take(m_gp.size() * sizeof(BlockRef)), o_mf = take(m_fast.size() * sizeof(BlockRef));
  GPlaneDesc gd;
  memset(&gd, 0, sizeof gd);
  gd.Gm = Gm; gd.ldg = ldg; gd.nt = nt; gd.ks = ks; gd.out = (uint16_t*)(base + o_planes); gd.plane = plane;
  DgemmDesc g;
  memset(&g, 0, sizeof g);
  g.A = A; g.C = C; g.selA = g.selB = g.selC = g.selP = g.selQ = -1;
  g.M = M; g.N = N; g.K = N; g.lda = lda; g.ldb = ldg; g.ldc = ldc; g.tiles_m = M / 32; g.tiles_n = N / 32;
  g.Gp = (const uint16_t*)(base + o_planes); g.g_plane = plane;
  HIP_OK(h, hipMemcpyAsync(base + o_g, &g, sizeof g, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(base + o_p, &gd, sizeof gd, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(base + o_mgp, m_gp.data(), m_gp.size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(base + o_mf, m_fast.data(), m_fast.size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
  HIP_OK(h, hipStreamSynchronize(s));
  launch_gplanes((const GPlaneDesc*)(base + o_p), (const BlockRef*)(base + o_mgp), (int)m_gp.size(), s);
  for (int i = 0; i < std::max(1, repeats); ++i)
    launch_dgemm3((const DgemmDesc*)(base + o_g), (const BlockRef*)(base + o_mf), (int)m_fast.size(), s);
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

size_t tadmm_cholqr_scratch_bytes(int n, int ncols) {
  return align_up(sizeof(DgemmDesc), 256) + align_up(sizeof(CholDesc), 256) + 2 * align_up((size_t)n * n * 8, 256) +
         align_up((size_t)n * 16 * 8, 256) + align_up((size_t)(n / 32) * (n / 32) * sizeof(BlockRef), 256) +
         align_up((size_t)(ncols / kCholStrip) * sizeof(BlockRef), 256) + 256;
}

int tadmm_cholqr_f64(tadmm_handle h, double* YT, int n, int ncols, int ldy, void* scratch, size_t scratch_bytes,
                     int* bad_out_host, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !YT || !scratch || !bad_out_host) return TADMM_ERR_INVALID;
  if (n <= 0 || n > 256 || n % 32 || ncols <= 0 || ncols % 64 || ldy < ncols || (ldy & 1))
    CTX_FAIL(h, TADMM_ERR_INVALID, "tadmm_cholqr_f64: n multiple of 32 (<= 256), ncols multiple of 64, ldy >= ncols even");
  if (scratch_bytes < tadmm_cholqr_scratch_bytes(n, ncols)) CTX_FAIL(h, TADMM_ERR_WORKSPACE, "cholqr scratch too small");
  hipStream_t s = (hipStream_t)stream_;
  char* base = (char*)scratch;
  size_t off = 0;
  DgemmDesc* gd = (DgemmDesc*)(base + off); off += align_up(sizeof(DgemmDesc), 256);
  CholDesc* cd = (CholDesc*)(base + off); off += align_up(sizeof(CholDesc), 256);
  double* Cm = (double*)(base + off); off += align_up((size_t)n * n * 8, 256);
  double* Rm = (double*)(base + off); off += align_up((size_t)n * n * 8, 256);
  double* Wd = (double*)(base + off); off += align_up((size_t)n * 16 * 8, 256);
  BlockRef* mg = (BlockRef*)(base + off); off += align_up((size_t)(n / 32) * (n / 32) * sizeof(BlockRef), 256);
  BlockRef* ms = (BlockRef*)(base + off); off += align_up((size_t)(ncols / kCholStrip) * sizeof(BlockRef), 256);
  int32_t* bad = (int32_t*)(base + off);
  DgemmDesc g;
  memset(&g, 0, sizeof g);
  g.A = YT; g.B = YT; g.C = Cm; g.selA = g.selB = g.selC = g.selP = g.selQ = -1;
  g.M = n; g.N = n; g.K = ncols; g.lda = ldy; g.ldb = ldy; g.ldc = n; g.tiles_m = n / 32; g.tiles_n = n / 32;
  CholDesc c;
  memset(&c, 0, sizeof c);
  c.C = Cm; c.ldc = n; c.n = n; c.R = Rm; c.ldr = n; c.Wd = Wd;
  c.ring[0] = YT; c.ring[1] = YT; c.ring[2] = YT; c.rot = nullptr; c.sel = 0; c.ldy = ldy; c.ncols = ncols; c.bad = bad;
  std::vector<BlockRef> vg, vs;
  for (int b = 0; b < g.tiles_m * g.tiles_n; ++b) vg.push_back(BlockRef{0, b});
  for (int b = 0; b < ncols / kCholStrip; ++b) vs.push_back(BlockRef{0, b});
  HIP_OK(h, hipMemsetAsync(bad, 0, 4, s));
  HIP_OK(h, hipMemcpyAsync(gd, &g, sizeof g, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(cd, &c, sizeof c, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(mg, vg.data(), vg.size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(ms, vs.data(), vs.size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
  HIP_OK(h, hipStreamSynchronize(s));
  launch_dgemm(gd, mg, (int)vg.size(), true, s);     // (32x32 kernel: ncols is only required to be a multiple of 16)
  launch_chol_factor(cd, 1, s);
  launch_chol_solve(cd, ms, (int)vs.size(), s);
  HIP_OK(h, hipMemcpyAsync(bad_out_host, bad, 4, hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipStreamSynchronize(s));
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

// ---- the filter's tile product and daxpby, launched as the filter launches them (tests) ----
int tadmm_dgemm_tile_prob_bytes(void) { return (int)sizeof(tadmm_dgemm_tile_prob); }

static const char* dgemm_tile_refusal(int nprob, const tadmm_dgemm_tile_prob* p, int tile_m, int tile_n, int axpby) {
  if (nprob <= 0 || nprob > 64 || !p) return "1 .. 64 problems";
  if (!((tile_m == 32 && tile_n == 32) || (tile_m == 64 && (tile_n == 32 || tile_n == 64))))
    return "(tile_m, tile_n) is (32, 32), (64, 32) or (64, 64)";
  for (int i = 0; i < nprob; ++i) {
    const tadmm_dgemm_tile_prob& q = p[i];
    auto named = [&](int sel, const void* ptr) {
      if (sel < 0) return ptr != nullptr;
      return sel <= 2 && q.ring[0] && q.ring[1] && q.ring[2];
    };
    if (q.M <= 0 || q.N <= 0 || q.K <= 0 || q.M % 32 || q.N % 32 || q.K % 32) return "M, N, K positive multiples of 32";
    if ((q.lda & 1) || (q.ldb & 1) || (q.ldc & 1) || q.lda < q.K || q.ldb < q.K || q.ldc < q.N)
      return "even leading dimensions, lda, ldb >= K, ldc >= N";
    if (q.mode < 0 || q.mode > 3) return "mode 0 .. 3";
    if (!named(q.selC, q.C)) return "C is not named (explicit pointer, or sel 0 .. 2 with a full ring)";
    if (axpby) {
      if (!named(q.selP, q.P) || !q.coef) return "axpby needs P and coef";
    } else {
      if (!named(q.selA, q.A) || !named(q.selB, q.B)) return "A or B is not named";
      if (q.mode >= 1 && !named(q.selP, q.P)) return "modes 1 .. 3 need P";
      if (q.selQ > 2) return "selQ <= 2";
      if (q.selQ >= 0 && !(q.ring[0] && q.ring[1] && q.ring[2])) return "selQ >= 0 needs a full ring";
      if (q.mode == 1 && !q.coef) return "mode 1 needs coef";
      if (q.mode == 3 && !q.theta) return "mode 3 needs theta";
      if (q.mode >= 2 && !q.rowpart) return "modes 2, 3 need rowpart";
    }
  }
  return nullptr;
}

static size_t dgemm_tile_blocks(const tadmm_dgemm_tile_prob& q, int tile_m, int tile_n, int axpby) {
  if (axpby) return (size_t)(((int64_t)q.M * q.ldc + 1023) / 1024);
  return (size_t)((q.M + tile_m - 1) / tile_m) * (size_t)((q.N + tile_n - 1) / tile_n);
}

int tadmm_dgemm_tile_check(int nprob, const tadmm_dgemm_tile_prob* probs, int tile_m, int tile_n, int axpby) {
  return dgemm_tile_refusal(nprob, probs, tile_m, tile_n, axpby) ? TADMM_ERR_INVALID : TADMM_OK;
}

size_t tadmm_dgemm_tile_scratch_bytes(int nprob, const tadmm_dgemm_tile_prob* probs) {
  if (nprob <= 0 || !probs) return 0;
  size_t blocks = 0;
  for (int i = 0; i < nprob; ++i)
    blocks += std::max(dgemm_tile_blocks(probs[i], 32, 32, 0), dgemm_tile_blocks(probs[i], 32, 32, 1));
  return align_up((size_t)nprob * sizeof(DgemmDesc), 256) + align_up(blocks * sizeof(BlockRef), 256);
}

int tadmm_dgemm_tile_f64(tadmm_handle h, int nprob, const tadmm_dgemm_tile_prob* probs, int tile_m, int tile_n, int axpby,
                         void* scratch, size_t scratch_bytes, void* stream_) {
  DeviceGuard device_guard(h);
  if (!h || !scratch) return TADMM_ERR_INVALID;
  if (const char* why = dgemm_tile_refusal(nprob, probs, tile_m, tile_n, axpby))
    CTX_FAIL(h, TADMM_ERR_INVALID, "tadmm_dgemm_tile_f64: %s", why);
  if (scratch_bytes < tadmm_dgemm_tile_scratch_bytes(nprob, probs)) CTX_FAIL(h, TADMM_ERR_WORKSPACE, "dgemm tile scratch too small");
  hipStream_t s = (hipStream_t)stream_;
  std::vector<DgemmDesc> descs((size_t)nprob);
  std::vector<BlockRef> map;
  std::vector<TileProb> tiles;
  for (int i = 0; i < nprob; ++i) {
    const tadmm_dgemm_tile_prob& q = probs[i];
    DgemmDesc& g = descs[(size_t)i];
    memset(&g, 0, sizeof g);
    g.A = q.A; g.B = q.B; g.C = q.C; g.P = q.P; g.Q = q.Q;
    g.ring[0] = q.ring[0]; g.ring[1] = q.ring[1]; g.ring[2] = q.ring[2]; g.rot = q.rot;
    g.selA = q.selA; g.selB = q.selB; g.selC = q.selC; g.selP = q.selP; g.selQ = q.selQ;
    g.M = q.M; g.N = q.N; g.K = q.K; g.lda = q.lda; g.ldb = q.ldb; g.ldc = q.ldc;
    g.tiles_m = q.M / 32; g.tiles_n = q.N / 32; g.mode = q.mode;
    g.coef = q.coef; g.theta = q.theta; g.rowpart = q.rowpart; g.gate = q.gate; g.gate_min = q.gate_min;
    const int nb = (int)dgemm_tile_blocks(q, tile_m, tile_n, axpby);
    if (axpby) for (int b = 0; b < nb; ++b) map.push_back(BlockRef{i, b});
    else tiles.push_back(TileProb{q.M, q.N, q.K, tile_m, tile_n});
  }
  if (!axpby) map = tile_map_build(tiles);        // the order the filter gives these launches (host.h)
  DgemmDesc* gd = (DgemmDesc*)scratch;
  BlockRef* md = (BlockRef*)((char*)scratch + align_up((size_t)nprob * sizeof(DgemmDesc), 256));
  HIP_OK(h, hipMemcpyAsync(gd, descs.data(), descs.size() * sizeof(DgemmDesc), hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(md, map.data(), map.size() * sizeof(BlockRef), hipMemcpyHostToDevice, s));
  HIP_OK(h, hipStreamSynchronize(s));
  if (axpby) launch_daxpby(gd, md, (int)map.size(), s);
  else launch_dgemm_nt64(gd, md, (int)map.size(), s, tile_n, tile_m);
  HIP_OK(h, hipStreamSynchronize(s));
  HIP_OK(h, hipGetLastError());
  return TADMM_OK;
}

// The block map the filter and tadmm_dgemm_tile_f64 give a grouped tile product (host.h: tile_map_build), host only.
int64_t tadmm_tile_map(int nprob, const tadmm_tile_map_prob* probs, int32_t* map_out, int64_t capacity, double* cost_out) {
  if (nprob <= 0 || nprob > 4096 || !probs) return TADMM_ERR_INVALID;
  std::vector<TileProb> t((size_t)nprob);
  int64_t blocks = 0;
  for (int i = 0; i < nprob; ++i) {
    const tadmm_tile_map_prob& q = probs[i];
    if (q.M <= 0 || q.N <= 0 || q.K <= 0 || q.tile_m <= 0 || q.tile_n <= 0) return TADMM_ERR_INVALID;
    t[(size_t)i] = TileProb{q.M, q.N, q.K, q.tile_m, q.tile_n};
    blocks += (int64_t)tile_rows(t[(size_t)i]) * tile_cols(t[(size_t)i]);
    if (blocks > (1 << 24)) return TADMM_ERR_INVALID;
  }
  if (!map_out && !cost_out) return blocks;
  if (map_out && capacity < blocks) return TADMM_ERR_WORKSPACE;
  const std::vector<BlockRef> m = tile_map_build(t);
  if (map_out) memcpy(map_out, m.data(), m.size() * sizeof(BlockRef));
  if (cost_out) { cost_out[0] = tile_map_cost(m, t); cost_out[1] = tile_map_cost(tile_map_plain(t), t); }
  return blocks;
}

}  // extern "C"
