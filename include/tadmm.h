/*
 * tadmm.h -- C ABI of the MI355X-native ADMM low-rank projection path.
 *
 * The reference (miaoyin390/DNN-Compression-Tensor-ADMM) is pure Python and has
 * no FFI layer; its boundary for this path is the Python API of admm.py /
 * ttd.py / TT*.py / TK*.py.  This header is the C ABI
 * that sits *behind* that Python surface: plain pointers and sizes, no torch
 * types, extern "C".  Every entry point names the reference code it replaces.
 *
 * Conventions
 *   - all tensors are row-major contiguous DEVICE pointers (float32 unless said
 *     otherwise), owned by the caller;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every
 *     call is stream-ordered and asynchronous unless documented otherwise;
 *   - return value 0 = success, negative = tadmm_status; a human-readable
 *     message for the last failure of a handle is returned by
 *     tadmm_last_error();
 *   - no exceptions cross the boundary; a handle is not thread-safe.
 */
#ifndef TADMM_H_
#define TADMM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TADMM_MAX_MODES 8

typedef enum {
  TADMM_OK = 0,
  TADMM_ERR_INVALID = -1,     /* bad argument / inconsistent descriptor          */
  TADMM_ERR_WORKSPACE = -2,   /* caller workspace too small                      */
  TADMM_ERR_HIP = -3,         /* a HIP runtime call failed                       */
  TADMM_ERR_NOCONVERGE = -4,  /* Jacobi eigen-solver hit its sweep cap           */
  TADMM_ERR_UNSUPPORTED = -5
} tadmm_status;

typedef enum {
  TADMM_KIND_TT_CONV = 0,   /* admm.py:91-101  prune_conv_rank_tt  ((O,I,k2)->(O,k2,I) unfold) */
  TADMM_KIND_TT_LINEAR = 1, /* admm.py:103-111 prune_linear_rank_tt (no permutation)           */
  TADMM_KIND_SVD = 2,       /* admm.py:129-149 prune_{conv,linear}_rank_svd (2-mode TT)        */
  TADMM_KIND_TUCKER2 = 3    /* admm.py:113-127 prune_{conv,linear}_rank_tk (HOSVD + HOOI)      */
} tadmm_kind;

/* flags */
#define TADMM_FLAG_SKIP_ROTATIONS 1u /* Z-only mode: a TT step whose kept rank equals the row
                                        count of its unfolding is an orthogonal change of basis
                                        that cannot change Z; skip its eigen-solve.  Must be 0
                                        when cores are requested.                              */

/* Plain-old-data description of one compressed parameter. */
typedef struct {
  int32_t kind;                      /* tadmm_kind                                        */
  int32_t ndim;                      /* 2 or 4                                            */
  int64_t dims[4];                   /* weight shape: (O,I,kh,kw) or (out,in)             */
  int32_t d;                         /* number of TT modes (TT kinds); 2 for SVD          */
  int32_t tt_shapes[TADMM_MAX_MODES];/* n_0..n_{d-1}  (hp_dict.tt_shapes[name])           */
  int32_t ranks[TADMM_MAX_MODES + 1];/* r_0..r_d      (hp_dict.ranks[name]); Tucker: [r_out,r_in] */
  uint32_t flags;
  int32_t hooi_max_iter;             /* Tucker only (tensorly default 100)                */
  float hooi_tol;                    /* Tucker only (tensorly default 1e-4)               */
} tadmm_layer_desc;

typedef struct tadmm_ctx_s* tadmm_handle;
typedef struct tadmm_plan_s* tadmm_plan;

/* ---- library / handle ------------------------------------------------- */
int tadmm_version(void);
/* sizeof(tadmm_layer_desc) / sizeof(tadmm_gemm_desc) as compiled: lets a foreign binding verify its struct layout */
int tadmm_abi_sizes(int* layer_desc_bytes, int* gemm_desc_bytes);
int tadmm_create(int device, tadmm_handle* out);
int tadmm_destroy(tadmm_handle h);
const char* tadmm_last_error(tadmm_handle h);

/* ---- rank clamp (ttd.py:18-19) ---------------------------------------- */
/* The reference clamps r_{i+1} to the number of singular values of the i-th
 * unfolding, min(r_i*n_i, prod(n_{i+1..})) -- a pure function of the shapes.
 * Applies it to desc->ranks in place (host only, no device work); returns the
 * number of entries changed.  Rank selection is therefore bit-exact by
 * construction. */
int tadmm_tt_clamp_ranks(tadmm_layer_desc* desc);

/* ---- projection plan: Z <- proj(W+U), U += W-Z, ||W-Z||^2 -------------- */
/* Replaces ADMM.update (admm.py:42-78) for a set of layers that are processed
 * together, phase by phase, in grouped launches.  Pointers are captured at
 * creation; descriptors (with clamped ranks) are copied.
 *   W[i], U[i], Z[i] : device float32, prod(dims) elements each
 *   cores[i]         : NULL, or device float32 buffer receiving the TT cores
 *                      back to back (core_0 .. core_{d-1}, each (r_j,n_j,r_{j+1}));
 *                      for Tucker: core (r_out,r_in,k2...) then U_out (O,r_out)
 *                      then U_in (I,r_in)
 *   workspace        : device scratch of at least tadmm_plan_workspace_bytes */
int tadmm_plan_workspace_bytes(tadmm_handle h, int n_layers, const tadmm_layer_desc* descs, size_t* bytes);
int tadmm_plan_create(tadmm_handle h, int n_layers, const tadmm_layer_desc* descs,
                      const float* const* W, float* const* U, float* const* Z, float* const* cores,
                      void* workspace, size_t workspace_bytes, tadmm_plan* out);
/* Runs one ADMM projection over all layers of the plan.
 *   update_u     : 0 -> only Z is written (ADMM.__init__ + update(update_u=False), engines.py:245)
 *   use_u        : 0 -> project W alone (the --decompose path: TTConv.py:96-109, TTLinear.py:61-66)
 *   resid_sq_dev : NULL or device double[n_layers]  <- ||W-Z||_2^2 per layer (admm.py:73-76)
 * Convergence of the Jacobi sweeps is decided on the device; the host reads the verdict through pinned
 * memory one sweep late, so the call blocks only at the end of each eigen-solve level. */
int tadmm_plan_run(tadmm_plan p, int update_u, int use_u, double* resid_sq_dev, void* stream);
/* Singular values kept at TT step `step` of layer `layer` in the last run (device->host copy,
 * synchronous).  out must hold ranks[step+1] doubles. */
int tadmm_plan_singular_values(tadmm_plan p, int layer, int step, double* out_host, void* stream);
/* Per-phase device time of the last run in milliseconds:
 * [0]=unfold [1]=gram [2]=eig [3]=project [4]=reconstruct [5]=fold/update, [6]=jacobi sweeps (count) */
int tadmm_plan_last_timing(tadmm_plan p, double out_ms[8]);
int tadmm_plan_enable_timing(tadmm_plan p, int on);
/* Jacobi tunables: tol = largest relative off-diagonal a sweep may observe and still be the last one
 * (quadratic convergence leaves ~tol^2 afterwards; default 1e-9), inner_sweeps = ignored (the 16x16
 * sub-problems always get one cyclic sweep per visit; the argument stays for ABI compatibility), max_sweeps = cap
 * before TADMM_ERR_NOCONVERGE.  <=0 keeps a value. */
int tadmm_plan_set_jacobi(tadmm_plan p, double tol, int inner_sweeps, int max_sweeps);
/* Filtered eigen-solver statistics (csrc/filter.hip): out[0] = eigen-problems of the plan served by the Chebyshev-
 * filtered subspace path (those whose kept rank is a fraction of their size), and for the LAST run out[1] = filtered
 * solves performed, out[2] = how many of them failed their a-posteriori check and were redone by the full Jacobi
 * solve, out[3] = largest number of filter stages a level needed.  TADMM_FILTER=0 in the environment disables the
 * path (every problem takes the full solve). */
int tadmm_plan_filter_stats(tadmm_plan p, int32_t out[4]);
/* With timing enabled (tadmm_plan_enable_timing) the fp64 GEMM launches of the filtered eigen-solver
 * (dgemm_nt_tile_kernel: block products, Gram matrices, Rayleigh-Ritz projection, residuals) are timed one by one
 * with HIP events on the launch stream: out[0] = their summed duration in ms, out[1] = number of launches,
 * out[2] = floating-point operations they executed (2*M*N*K of every product that was not gated off). */
int tadmm_plan_filter_timing(tadmm_plan p, double out[4]);
/* The same for the block products that ran at fp32 accuracy on the bf16 matrix cores (dgemm3_kernel: every filter
 * stage but the last one a level needed in the previous run; TADMM_FILTER_FAST=0 keeps all products in fp64):
 * out[0] = ms, out[1] = launches, out[2] = ALGORITHMIC flops 2*M*N*K (six bf16 products are executed per flop pair). */
int tadmm_plan_filter_timing_fast(tadmm_plan p, double out[4]);
/* The same for the launches of jacobi_tick3_kernel (the block-Jacobi tournament of the Rayleigh-Ritz and full solves):
 * out[0] = ms, out[1] = launches, out[2] = matrix-core flops the launches executed (2560 * row length per workgroup of
 * a problem the host did not yet know to be finished: cross Gram + two rounds of column updates), out[3] = those
 * workgroups. */
int tadmm_plan_jacobi_timing(tadmm_plan p, double out[4]);
/* clamped ranks of a layer (r_0..r_d); returns d+1 */
int tadmm_plan_ranks(tadmm_plan p, int layer, int32_t* ranks_out);
/* Lanes.  A plan whose table mixes long chains of eigen-solves (e.g. the 3x3 kernels of ResNet layer3/layer4) with
 * short ones runs as two sub-plans on two device streams -- the long chains on a high-priority stream, the rest
 * filling the CUs they leave idle; the caller's stream is joined in front and behind, the second lane is driven by a
 * worker thread owned by the plan.  Returns the number of lanes (1 or 2) and, when lane_of_out is not NULL, each
 * layer's lane.  A big table of like layers (>= 16, every chain within the threshold of the longest) is split into two halves.
 * TADMM_LANES=1 in the environment keeps every plan in one lane; TADMM_LANE_THRESHOLD (default 0.6)
 * is the fraction of the longest modelled chain from which a layer counts as long. */
int tadmm_plan_lanes(tadmm_plan p, int32_t* lane_of_out);
/* The split rule alone (pure host function of the descriptors, no device needed): what tadmm_plan_create would do. */
int tadmm_lane_split(int n_layers, const tadmm_layer_desc* descs, int32_t* lane_of_out);
int tadmm_plan_destroy(tadmm_plan p);

/* ---- Tucker-2 projection plan (admm.py:113-127: tensorly partial_tucker + tucker_to_tensor) ---- */
/* All layers of kind TADMM_KIND_TUCKER2 (ranks[0] = r_out, ranks[1] = r_in; 4-D (O,I,kh,kw) or 2-D (out,in))
 * are processed together: HOSVD initialisation, then HOOI sweeps until each layer meets tensorly's stopping
 * rule (|err_it - err_{it-1}| < hooi_tol from the third sweep, at most hooi_max_iter sweeps; 0 selects the
 * tensorly defaults 1e-4 / 100), then Z = core x_0 U_out x_1 U_in, U += W-Z and ||W-Z||^2 as in tadmm_plan_run.
 * The stopping rule is evaluated on the device; layers that are finished drop out of the later grouped launches.
 * PARITY UNPINNED: tensorly is not vendored by the reference. */
typedef struct tadmm_tucker_plan_s* tadmm_tucker_plan;
int tadmm_tucker_workspace_bytes(tadmm_handle h, int n_layers, const tadmm_layer_desc* descs, size_t* bytes);
int tadmm_tucker_create(tadmm_handle h, int n_layers, const tadmm_layer_desc* descs, const float* const* W,
                        float* const* U, float* const* Z, void* workspace, size_t workspace_bytes,
                        tadmm_tucker_plan* out);
int tadmm_tucker_run(tadmm_tucker_plan p, int update_u, int use_u, double* resid_sq_dev, void* stream);
/* Device pointers (inside the workspace, valid after a run) of a layer's factors:
 * core (r_out, k2, r_in) row-major -- note the kernel-position axis in the middle --, U_out (O, r_out),
 * U_in (I, r_in).  Columns beyond the number of singular values of an unfolding are zero. */
int tadmm_tucker_factors(tadmm_tucker_plan p, int layer, const float** core, const float** u_out, const float** u_in);
/* HOOI sweeps each layer ran in the last call and its final relative reconstruction error (host arrays of
 * n_layers entries, either may be NULL); synchronises the stream. */
int tadmm_tucker_iterations(tadmm_tucker_plan p, int32_t* iters_out_host, double* errors_out_host, void* stream);
/* Jacobi sweeps summed over every eigen-solve group of the last run (HOSVD start + two per HOOI sweep): the figure the
 * warm start of the HOOI solves lowers; host-side counter, no synchronisation.  Negative on a null plan. */
int tadmm_tucker_jacobi_sweeps(tadmm_tucker_plan p);
/* Instrumented runs (bench.py): every launch of the eigen-solver is bracketed by HIP events on the launch stream (adds a
 * stream sync per launch).  last_timing: out[0] = summed ms of those launches in the last run, [1] = their number,
 * [2] = the 8 N^3 model FLOPs they stand for, [3] = ms of the whole run, [4] = HOOI sweeps (max over layers). */
int tadmm_tucker_enable_timing(tadmm_tucker_plan p, int on);
int tadmm_tucker_last_timing(tadmm_tucker_plan p, double out[8]);
int tadmm_tucker_destroy(tadmm_tucker_plan p);

/* ---- augmented-Lagrangian penalty (admm.py:80-85) ---------------------- */
/* loss_dev[0] += 0.5*rho*sum_i ||W_i - Z_i + U_i||^2 ; gradW[i] (nullable) = grad_scale*(W_i-Z_i+U_i)
 * (grad_scale = rho * upstream gradient of the scalar loss).
 * ptrs_dev: device array of 4*n pointers laid out [W_0..W_{n-1} | Z.. | U.. | gradW..] ;
 * numel_dev: device int64[n]; partial_dev: device double scratch >= tadmm_penalty_scratch_doubles(). */
int tadmm_penalty_scratch_doubles(void);
int tadmm_penalty(tadmm_handle h, int n, const void* const* ptrs_dev, const int64_t* numel_dev,
                  int64_t total_numel, float rho, float grad_scale, double* loss_dev, double* partial_dev,
                  void* stream);

/* ---- orthogonality regulariser of Tucker / SVD factors (orthogonal.py: append_double_l2_loss) ---------------------
 * For every factor P (a rows x cols float32 matrix, row stride ld >= cols, 4-byte aligned):
 *   gram_of_rows != 0:  E = P P^T - I,  grad = 2 rho E P        gram_of_rows == 0:  E = P^T P - I,  grad = 2 rho P E
 *   loss_dev[0] += 0.5 * rho * sum ||E||_F^2
 * The Grams are exact fp32 products accumulated in fp64 on v_mfma_f64_16x16x4_f64 (csrc/gram.hip), E P / P E run on
 * the fp64 matrix cores as well and each gradient entry is rounded to float32 once.  Fixed reduction orders, no
 * floating-point atomics: results are bitwise reproducible.
 * grad_offset: where the factor's gradient (contiguous rows x cols float32) starts, in elements, inside the gradient
 *   buffer given to each tadmm_orth_l2 call; negative: the factor adds to the loss but gets no gradient.
 * The plan captures the P pointers and uploads its tables into the workspace once, ordered on `stream` (the call waits
 * for the copy); each tadmm_orth_l2 call is then stream-ordered, copies nothing and launches at most four kernels
 * whatever the number of factors (a call with grad == NULL launches only the workgroups that sum ||E||^2).
 * tadmm_orth_plan_create returns TADMM_ERR_INVALID for n <= 0, an empty factor (rows * cols == 0), ld < cols or a
 * misaligned P, and TADMM_ERR_WORKSPACE when workspace_bytes < tadmm_orth_workspace_bytes. */
typedef struct {
  const float* P;
  int64_t grad_offset;
  int32_t rows, cols;
  int64_t ld;
  int32_t gram_of_rows;
  int32_t reserved;
} tadmm_orth_desc;
typedef struct tadmm_orth_plan_s* tadmm_orth_plan;
/* sizeof(tadmm_orth_desc) as the library was built */
int tadmm_orth_desc_bytes(void);
int tadmm_orth_workspace_bytes(int n, const tadmm_orth_desc* descs, size_t* bytes);
int tadmm_orth_plan_create(tadmm_handle h, int n, const tadmm_orth_desc* descs, void* workspace,
                           size_t workspace_bytes, void* stream, tadmm_orth_plan* out);
/* grad: device float32 buffer holding every factor's gradient at its grad_offset, or NULL (loss only). */
int tadmm_orth_l2(tadmm_orth_plan p, double rho, float* grad, double* loss_dev, void* stream);
int tadmm_orth_plan_destroy(tadmm_orth_plan p);

/* ---- Riemannian SGD on the Stiefel manifold (StfTKConv.py + geoopt.optim.RiemannianSGD) --------------------------
 * Every factor X (rows x cols float32, rows >= cols, row stride ld >= cols, 4-byte aligned, columns orthonormal) of a
 * model is updated in place by ONE launch, one workgroup per factor, its tiles resident in LDS (csrc/stiefel.hip).
 * With G the gradient and M the momentum buffer (both laid out like X), sym(A) = (A + A^T) / 2:
 *   g = G + weight_decay X;   r = g - X sym(X^T g);
 *   momentum > 0:  M <- momentum M + (1 - dampening) r,   d = nesterov ? r + momentum M : M;      else d = r
 *   X <- Q factor (positive diagonal of R) of X - lr d;   momentum > 0:  M <- M - X sym(X^T M)
 * Inner products are accumulated in fp64 from the fp32 tiles, the QR is a Cholesky QR in fp64 (a second pass when the
 * pivots spread by more than 1e4), every stored entry is rounded to fp32 once.
 * G == NULL: the factor is skipped by tadmm_stiefel_step (X and M untouched).  M may be NULL when momentum == 0 and
 * for plans used by tadmm_stiefel_project only, which replaces every X by the Q factor of X (any full-rank X).
 * A factor whose Cholesky pivot is not positive and finite (rank-deficient or non-finite input) keeps X and M and gets
 * status_dev[i] = 1 (int32 per factor, never cleared by the library, may be NULL); nothing synchronises.
 * tadmm_stiefel_workspace_bytes / _plan_create return TADMM_ERR_INVALID for n <= 0, rows < cols, cols <= 0, ld < cols,
 * a null or misaligned X, and TADMM_ERR_UNSUPPORTED for a factor whose tiles do not fit the LDS
 * (12 rows (cols|1) + 16 cols (cols|1) + 16 cols bytes <= 160 KiB; 64 x 64 and 123 x 64 fit).  The plan uploads its
 * table once, ordered on `stream` (the call waits for the copy); step / project copy nothing. */
typedef struct {
  float* X;
  const float* G;
  float* M;
  int32_t rows, cols;
  int64_t ld;
} tadmm_stiefel_desc;
typedef struct tadmm_stiefel_plan_s* tadmm_stiefel_plan;
/* sizeof(tadmm_stiefel_desc) as the library was built */
int tadmm_stiefel_desc_bytes(void);
int tadmm_stiefel_workspace_bytes(int n, const tadmm_stiefel_desc* descs, size_t* bytes);
int tadmm_stiefel_plan_create(tadmm_handle h, int n, const tadmm_stiefel_desc* descs, void* workspace,
                              size_t workspace_bytes, void* stream, tadmm_stiefel_plan* out);
int tadmm_stiefel_step(tadmm_stiefel_plan p, double lr, double momentum, double dampening, double weight_decay,
                       int nesterov, int32_t* status_dev, void* stream);
/* Riemannian Adam on the same plan (geoopt.optim.RiemannianAdam on Stiefel factors), one launch.  M of the descriptor is
 * exp_avg; v_dev (second moment, ONE float32 per factor), vmax_dev (its running maximum, amsgrad only, else may be NULL)
 * and step_dev (int32 step counter per factor) hold n entries each, in the plan's (descriptor) order:
 *   t' = t + 1;   g = G + weight_decay X;   r = g - X sym(X^T g);   s = sum_ij r_ij^2   (fp64, fixed summation order)
 *   M' = beta1 M + (1 - beta1) r;   v' = beta2 v + (1 - beta2) s;   u = amsgrad ? max(vmax, v') : v'
 *   X <- Q factor (positive diagonal of R) of X - lr / ((1 - beta1^t') (sqrt(u / (1 - beta2^t')) + eps)) M'
 *   M <- M' - X sym(X^T M');   v <- v', vmax <- u (amsgrad), t <- t'
 * The bias corrections are computed on the device from the factor's own counter; the host never reads it.  G == NULL
 * skips the factor: nothing of it is written.  A factor that fails (the rule above, or a non-finite second moment)
 * keeps X, M, v, vmax and t and gets status_dev[i] = 1.  Copies nothing, synchronises nothing.
 * Returns TADMM_ERR_INVALID and launches nothing for a NULL plan, beta1 or beta2 outside [0, 1), eps < 0, lr < 0,
 * weight_decay < 0, a NULL v_dev or step_dev, amsgrad with a NULL vmax_dev, and a plan in which some factor has no M. */
int tadmm_stiefel_adam_step(tadmm_stiefel_plan p, double lr, double beta1, double beta2, double eps,
                            double weight_decay, int amsgrad, float* v_dev, float* vmax_dev, int32_t* step_dev,
                            int32_t* status_dev, void* stream);
int tadmm_stiefel_project(tadmm_stiefel_plan p, int32_t* status_dev, void* stream);
int tadmm_stiefel_plan_destroy(tadmm_stiefel_plan p);

/* ---- BertAdam (xcompression/transformer/optimization.py:183-302) -------------------------------------------------
 * The optimiser of the reference's BERT training scripts, for ALL n tensors of a param group in two launches
 * (csrc/bertadam.hip).  Every tensor is float32, dense-contiguous, n elements, its four pointers 4-byte aligned; tensors
 * whose four pointers are 16-byte aligned take 16-byte accesses, the others single elements (chosen per tensor).
 * Work is cut into chunks of tadmm_bertadam_chunk() elements, a chunk never spanning two tensors.  With
 * max_grad_norm > 0 a first launch stores each chunk's sum of g^2 (double) into the workspace; the update launch adds a
 * tensor's partial sums in a fixed order that depends on the tensor alone (every chunk of it sees the same bits) and forms
 *   norm = sqrt(sum g^2),   c = (float) min(1, max_grad_norm / (norm + 1e-6))          (c = 1 with max_grad_norm <= 0)
 * then per element, in float32, each operation rounded on its own:
 *   gc = g c;   m <- b1 m + (1 - b1) gc;   v <- b2 v + (1 - b2) gc gc
 *   u = m / (sqrtf(v) + e);   u += weight_decay p  (only with weight_decay > 0);   p <- p - lr u
 * There is no bias correction; lr is the caller's scheduled rate.  g is read only (the reference scales .grad in place,
 * this does not).  Non-finite gradients follow IEEE as in the reference: an inf element gives norm = inf, c = 0 and a NaN
 * at that element only; there is no skipping and no status word.  No atomics, no inter-workgroup waiting: results are
 * bitwise reproducible.
 * tadmm_bertadam_workspace_bytes / _plan_create return TADMM_ERR_INVALID, with nothing launched, for n <= 0, a null or
 * misaligned (not 4-byte) pointer and a tensor with n <= 0; _plan_create returns TADMM_ERR_WORKSPACE for a workspace
 * that is null or too small and TADMM_ERR_INVALID for one that is not 16-byte aligned.  The plan uploads its table and
 * chunk map once, ordered on `stream` (the call waits for the copy), and clears the norms; the pointers of the
 * descriptors and the workspace must stay valid for the life of the plan.
 * tadmm_bertadam_step copies nothing and synchronises nothing; it returns TADMM_ERR_INVALID, with nothing launched, for a
 * NULL plan, b1 or b2 outside [0, 1), e < 0 and lr < 0 (NaN included).
 * tadmm_bertadam_norms hands out the device array of n doubles holding every tensor's gradient norm as the last step
 * with max_grad_norm > 0 computed it (zeros before the first); it lives in the workspace. */
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} tadmm_bertadam_desc;
typedef struct tadmm_bertadam_plan_s* tadmm_bertadam_plan;
/* sizeof(tadmm_bertadam_desc) as the library was built */
int tadmm_bertadam_desc_bytes(void);
/* elements per chunk (one workgroup's unit of work; a multiple of 4) */
int tadmm_bertadam_chunk(void);
int tadmm_bertadam_workspace_bytes(int n, const tadmm_bertadam_desc* descs, size_t* bytes);
int tadmm_bertadam_plan_create(tadmm_handle h, int n, const tadmm_bertadam_desc* descs, void* workspace,
                               size_t workspace_bytes, void* stream, tadmm_bertadam_plan* out);
int tadmm_bertadam_step(tadmm_bertadam_plan p, double lr, double b1, double b2, double e, double weight_decay,
                        double max_grad_norm, void* stream);
int tadmm_bertadam_norms(tadmm_bertadam_plan p, double** norms_dev);
int tadmm_bertadam_plan_destroy(tadmm_bertadam_plan p);

/* ---- building blocks (also used by the factorised layers) -------------- */
/* C[i,j] = alpha * sum_k A(i,k) B(k,j) (+ beta*C) with arbitrary element strides; one of the two
 * strides of each operand must be 1.  Replaces the torch.mm / F.linear chains of
 * TTLinear.py:79-86, TTConv.py:133-147, TKConv.py:210-214, TKLinear.py:66-71 and np.dot of
 * ttd.py:39-40.  fp32 in, fp32 MFMA accumulate. */
typedef struct {
  const float* A; const float* B; float* C;
  int32_t M, N, K;
  int64_t a_rs, a_cs, b_rs, b_cs, c_rs, c_cs;
  float alpha, beta;
  const float* bias_n;   /* nullable: added along N (C[i,j] += bias_n[j]) */
  const float* bias_m;   /* nullable: added along M */
} tadmm_gemm_desc;
/* pack: writes GemmDesc[n] + block map into a host blob the caller uploads (and may cache) itself;
 * run: launches one grouped kernel over the uploaded blob.
 * A descriptor with M, N or K <= 0 or an operand A / B without a unit stride is refused before anything is sized:
 * tadmm_gemm_pack returns TADMM_ERR_INVALID (TADMM_ERR_WORKSPACE only for a valid group in a short blob) and
 * tadmm_gemm_pack_bytes returns 0. */
size_t tadmm_gemm_pack_bytes(int n, const tadmm_gemm_desc* descs);
int tadmm_gemm_pack(int n, const tadmm_gemm_desc* descs, void* blob_host, size_t blob_bytes, int* nblocks_out);
int tadmm_gemm_run(tadmm_handle h, const void* blob_dev, int n, int nblocks, void* stream);
/* One GEMM, descriptor passed by value to the kernel (no upload): the per-call path of the layers' forward and
 * backward products (TTLinear.py:79-86, TTConv.py:133-147, TKConv.py:210-214, TKLinear.py:66-71). */
int tadmm_gemm(tadmm_handle h, const tadmm_gemm_desc* desc, void* stream);
/* bf16 inference path of the TT-linear chain (TTLinear.py:79-86; every product there is A * Bt^T with both
 * operands contiguous along K):  C[M][N] = A[M][K] * Bt[N][K]^T (+ bias_n[j]), bf16 in / bf16 out, fp32
 * accumulate on the matrix cores.  lda / ldb / ldc in elements. */
int tadmm_gemm_bf16_nt(tadmm_handle h, const void* A, const void* Bt, void* C, int M, int N, int K, int64_t lda,
                       int64_t ldb, int64_t ldc, const float* bias_n, void* stream);

/* ---- forward chains of the factorised layers (csrc/chain.hip) ---------------------------------------------------
 * One launch per chain on the bf16 matrix cores; the per-token intermediate stays in LDS.
 *   fused  : Y[t][:] = Wout (Win X[t][:]) + bias     TTLinearM (TTLinear.py:75-93); Win (R x Kin) / Wout (Nout x R)
 *            are the contracted input / output cores, R the middle TT rank (multiple of 64, <= 256; pad with zeros).
 *   single : Y[t][:] = Win X[t][:] + bias            N = R output features, any size.
 * dtype TADMM_CHAIN_F32: X, Y float32; weights as THREE bf16 planes (w = w1 + w2 + w3 exactly, plane p at
 *   W + p * plane_stride); six bf16 products per fp32 product, fp32 accumulate: fp32-GEMM accuracy.
 * dtype TADMM_CHAIN_BF16: X, Y bfloat16; one weight plane.
 * dtype TADMM_CHAIN_F16 (inference): X, Y IEEE binary16; the weights are ONE plane of binary16 in the same
 *   fragment-major order as a bf16 plane; fp32 accumulate, float32 bias; results round to nearest even and overflow to
 *   +-inf.  Every alignment, padding and size rule is TADMM_CHAIN_BF16's.  The library cannot tell a binary16 plane
 *   from a bfloat16 one: the caller pairs planes and dtype.  All seven entries below take all three dtypes (the _bwd
 *   entries are the forward kernels on transposed planes).
 * Layouts: x_hw / y_hw == 0: token rows of ldx / ldy elements.  x_hw / y_hw > 0: channels-first images
 *   (batch, channel, pixel) of that many pixels -- the NCHW tensors of TTConv.py:131 / TKConv.py:94 in place.  With an
 *   image on either side T must be a whole number of its planes (T % x_hw == 0, T % y_hw == 0): every entry returns
 *   TADMM_ERR_INVALID otherwise and launches nothing.
 * Weights are FRAGMENT-MAJOR (one MFMA operand = one contiguous KiB): element (row n, col k) of plane p of an
 *   N x K weight lives at W[p*plane + (((n/16)*KS + k/32)*64 + (k%32/8)*16 + n%16)*8 + k%8], KS = ceil(K/32), rows
 *   padded to 16 and columns to 32 with zeros (tadmm.ops.weight_planes builds it).  Token rows: Kin % 8 == 0
 *   (% 4 for float32) and 16-byte aligned rows.  bias: float32[N], 16-byte aligned, or NULL.  tile_tokens: 0 (default), 32 or 64. */
enum { TADMM_CHAIN_F32 = 0, TADMM_CHAIN_BF16 = 1, TADMM_CHAIN_F16 = 2 };
typedef struct {
  const void* X; void* Y;
  const void* Win; const void* Wout;          /* bf16 planes (binary16 for TADMM_CHAIN_F16) */
  const float* bias;
  int64_t T;                                   /* tokens (rows, or batch * pixels) */
  int32_t Kin, R, Nout;
  int64_t ldx, ldy, win_plane, wout_plane;   /* elements */
  int32_t x_hw, y_hw;
  int32_t dtype, tile_tokens;
} tadmm_chain_desc;
/* sizeof(tadmm_chain_desc) as the library was built (bindings check their struct layout against it) */
int tadmm_chain_desc_bytes(void);
/* TTLinearM forward (TTLinear.py:75-93), fused.  dtype: F32 | BF16 | F16. */
int tadmm_ttlinear_fwd(tadmm_handle h, const tadmm_chain_desc* d, void* stream);
/* TTLinearM data gradient dX = (dY Wout) Win: the same fused kernel with X = dY, Win = Wout^T planes (R x Nout),
 * Wout = Win^T planes (Kin x R); weight gradients are plain products (tadmm_gemm).  dtype: F32 | BF16 | F16. */
int tadmm_ttlinear_bwd(tadmm_handle h, const tadmm_chain_desc* d, void* stream);
/* TTConv2dM input-core chain (TTConv.py:131-137): image (B, C, H, W) -> (B, r, H, W), single product.
 * dtype: F32 | BF16 | F16. */
int tadmm_ttconv_chain_in(tadmm_handle h, const tadmm_chain_desc* d, void* stream);
/* TTConv2dM output-core chain + bias (TTConv.py:141-151): (B, r, H', W') -> (B, O, H', W'), single product.
 * dtype: F32 | BF16 | F16. */
int tadmm_ttconv_chain_out(tadmm_handle h, const tadmm_chain_desc* d, void* stream);
/* TKConv2dC first / last 1x1 stage (TKConv.py:93-98): per-pixel channel mixing, single product.
 * dtype: F32 | BF16 | F16. */
int tadmm_tucker_1x1(tadmm_handle h, const tadmm_chain_desc* d, void* stream);
/* SVDConv2dC / SVDConv2dM forward (SVDConv.py: two 1x1 convolutions / two per-pixel linears, padding 0):
 * y[b,:,p] = Wout (Win x[b,:,p]) + bias on NCHW images in place, one launch, the R-vector of a pixel in LDS.
 * x_hw = y_hw = H*W, T = B*H*W, Kin = C_in, Nout = C_out; Win (R x C_in) / Wout (C_out x R) planes with the rank padded
 * to R (multiple of 64, <= 256) as for tadmm_ttlinear_fwd.  Ranks above 256 are not served (two tadmm_tucker_1x1).
 * dtype: F32 | BF16 | F16. */
int tadmm_svdconv_fwd(tadmm_handle h, const tadmm_chain_desc* d, void* stream);
/* Its data gradient dX = Win^T (Wout^T dY): the same kernel with X = dY, Win = Wout^T planes (R x C_out),
 * Wout = Win^T planes (C_in x R), bias NULL.  dtype: F32 | BF16 | F16. */
int tadmm_svdconv_bwd(tadmm_handle h, const tadmm_chain_desc* d, void* stream);
/* Training on the fused chains: the four entries above that also store the middle-rank vector -- product 1, which the
 * plain entries keep in LDS and drop -- for the two weight gradients (tadmm_wgrad).  The descriptor is the plain
 * entry's; r in (0, R] is the true middle rank (R its padding), and only columns [0, r) are stored:
 *   _fwd_save : h_out  = H  = X Win^T          (dWout = dY^T H)
 *   _bwd_save : dh_out = dH = dY Wout          (dWin  = dH^T X), with the transposed planes of the _bwd entries.
 * The stored value is what product 2 reads: the bfloat16 rounding of the fp32 accumulator (TADMM_CHAIN_BF16), or the
 * accumulator itself (TADMM_CHAIN_F32).  Y is bit-identical to the plain entry's: the save adds stores, nothing else.
 * Layout, of the descriptor's dtype: tadmm_ttlinear_*: token rows (T, r) with row stride ldh >= r elements;
 * tadmm_svdconv_*: channels [0, r) of images (T / x_hw, ldh, x_hw), ldh >= r channels per image (ldh == r: one contiguous
 * NCHW tensor, the image layout of tadmm_wgrad).  Nothing else of the buffer is written.  Stores are 16-byte units where
 * h_out is 16-byte aligned and ldh (rows) or x_hw (images) is a whole number of them, single elements otherwise.
 * TADMM_ERR_INVALID, with nothing launched: TADMM_CHAIN_F16 (there is no binary16 weight gradient), a null h_out, r
 * outside (0, R], ldh < r, an h_out that is not aligned to its element; and whatever the plain entry refuses, with the
 * plain entry's status. */
int tadmm_ttlinear_fwd_save(tadmm_handle h, const tadmm_chain_desc* d, int r, void* h_out, int64_t ldh, void* stream);
int tadmm_ttlinear_bwd_save(tadmm_handle h, const tadmm_chain_desc* d, int r, void* dh_out, int64_t ldh, void* stream);
int tadmm_svdconv_fwd_save(tadmm_handle h, const tadmm_chain_desc* d, int r, void* h_out, int64_t ldh, void* stream);
int tadmm_svdconv_bwd_save(tadmm_handle h, const tadmm_chain_desc* d, int r, void* dh_out, int64_t ldh, void* stream);

/* ---- weight gradients of the factorised layers (csrc/wgrad.hip) ---------------------------------------------------
 * C[m][n] = alpha * sum_{t < T} A[t][m] * B[t][n], float32 C with row stride ldc: dW = dY^T X and its kin, a small
 * output (a rank times a channel count) over a long reduction (tokens or batch * pixels).  A and B are read in place,
 * both of `dtype` (TADMM_CHAIN_F32: exact three-plane bf16 split, six products per product, fp32-GEMM accuracy;
 * TADMM_CHAIN_BF16: one plane, products exact; TADMM_CHAIN_F16 is refused with TADMM_ERR_INVALID), both in one layout:
 *   hw == 0: token rows, A (T, M) with row stride lda >= M, B (T, N) with row stride ldb >= N (elements);
 *   hw  > 0: channels-first images, A contiguous (T / hw, M, hw), B contiguous (T / hw, N, hw); lda / ldb ignored.
 * Any alignment the element type allows: 16-byte loads where base and stride (lda / ldb, or hw) permit, 8-byte or
 * element loads otherwise.  The reduction is split over slices of T; the number of slices is a pure function of
 * (M, N, T).  With more than one slice every slice writes its tile to `workspace` (16-byte aligned, at least
 * tadmm_wgrad_workspace_bytes) and a second launch adds them in fixed order in fp64: no atomics, bitwise reproducible,
 * and independent of what workspace and C held before.  T == 0 writes zeros.
 * TADMM_ERR_INVALID: M <= 0, N <= 0, T < 0, unknown dtype, a null operand with T > 0, T not a multiple of hw, a row
 * stride below the feature count; TADMM_ERR_WORKSPACE: workspace too small (nothing is launched);
 * TADMM_ERR_UNSUPPORTED: T >= 2^31 - 256 or more than 2^20 output tiles. */
typedef struct {
  const void* A; const void* B; float* C;
  int64_t T;
  int32_t M, N;
  int64_t lda, ldb, ldc;                      /* elements */
  int32_t hw;                                 /* 0: token rows; > 0: NCHW images of hw pixels */
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16, for A and B alike */
  float alpha;
  int32_t reserved;
} tadmm_wgrad_desc;
/* sizeof(tadmm_wgrad_desc) as the library was built */
int tadmm_wgrad_desc_bytes(void);
/* Host only, no device needed: bytes of workspace tadmm_wgrad wants for this descriptor (0 when one slice serves it)
 * and, when slices_out is not NULL, the number of slices. */
int tadmm_wgrad_workspace_bytes(const tadmm_wgrad_desc* d, size_t* bytes, int* slices_out);
int tadmm_wgrad(tadmm_handle h, const tadmm_wgrad_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* The whole factorised convolution of a SMALL image in one launch (csrc/convchain.hip): y = W3 conv_kxk(W1 x; Wc) + bias
 * for NCHW tensors with output rows of at most 64 pixels: one workgroup per tile of output rows (<= 64 output pixels, a halo of
 * <= 192 input pixels); the two intermediates stay in LDS.  TTConv2dM
 * (TTConv.py:130-153), TKConv2dC / TKConv2dM (TKConv.py:93-98, :210-214).  W1 (R1 x C), W2 (R2 x kh*kw*R1, tap-major:
 * column (dy*kw + dx)*R1 + c) and W3 (Nout x R2) are fragment-major bf16 planes as for tadmm_chain_desc, R1 and R2
 * multiples of 32 (zero padded), both <= 256; groups = 1.  Returns TADMM_ERR_UNSUPPORTED when the image or the
 * intermediates do not fit (the caller then uses tadmm_ttconv_chain_in / conv2d / tadmm_ttconv_chain_out).
 * dtype: tadmm_ttconv_fused and tadmm_ttconv_fused_plan take F32 | BF16 | F16 (F16: one binary16 plane per weight, the
 * BF16 kernel with the f16 MFMA and conversions; its plan equals the BF16 plan field for field).  tadmm_ttconv_fused_save
 * and tadmm_ttconv_fused_bwd take F32 | BF16 and refuse F16 with TADMM_ERR_INVALID: what they store feeds the weight
 * gradients, which have no binary16 form. */
typedef struct {
  const void* X; void* Y;
  const void* W1; const void* W2; const void* W3;
  const float* bias;
  int64_t w1_plane, w2_plane, w3_plane;
  int32_t B, C, R1, R2, Nout;
  int32_t H, W, Ho, Wo, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 | TADMM_CHAIN_F16 (see above) */
} tadmm_conv_chain_desc;
int tadmm_conv_chain_desc_bytes(void);
int tadmm_ttconv_fused(tadmm_handle h, const tadmm_conv_chain_desc* d, void* stream);
/* Training on the one-launch path.  Both entries take the descriptor filled with the FORWARD geometry (H x W the input
 * plane, Ho x Wo the output plane, C / Nout the input / output channels, R1 / R2 the padded ranks) plus the true ranks
 * r1 in (0, R1], r2 in (0, R2] of the intermediates they store as contiguous NCHW tensors of `dtype`.
 *   _save : tadmm_ttconv_fused that also writes H1 (B, r1, H, W) = W1 x and H2 (B, r2, Ho, Wo) = conv(H1; Wc).  A pixel
 *           of H1 that no tap of any output pixel reads is written as zero (it contributes to no gradient).
 *   _bwd  : the data gradient dX = W1^T conv^T(W3^T dY; Wc) in one launch (transposed gather, nothing flipped):
 *           d->X = dY (B, Nout, Ho, Wo), d->Y = dX (B, C, H, W), d->W1 = planes of W3^T (R2 x Nout, rows padded to 32),
 *           d->W2 = planes of the transposed core (R1 x kh*kw*R2, tap-major as for tadmm_core_conv_dgrad), d->W3 =
 *           planes of W1^T (C x R1); d->bias is ignored.  Input pixels no tap reaches get exact zeros.  dH1 (B, r1, H, W)
 *           and dH2 (B, r2, Ho, Wo) receive the two intermediates (what the weight gradients read), or both are NULL.
 * Every element of the stored tensors is written by exactly one workgroup, chosen by the geometry alone: results are
 * bitwise reproducible, and nothing outside the tensors is written.
 * tadmm_ttconv_fused_plan is host only (no device): the tiling a launch of `mode` would use -- pixels and destination
 * rows per workgroup, 64- or 32-pixel tiles of its halo, workgroups per image, LDS bytes (any pointer may be NULL;
 * operand pointers of the descriptor are not read) -- and the one statement of the eligibility rule.
 * TADMM_ERR_INVALID: a non-positive extent, stride or dilation, negative padding or B, Ho / Wo that are not the output
 * size of the geometry, unknown dtype or mode, a null or misaligned operand with B > 0, weight planes too small or
 * misaligned, r1 / r2 outside (0, R1] / (0, R2], exactly one of dH1 / dH2 NULL.  TADMM_ERR_UNSUPPORTED: the
 * destination plane of the mode (Wo forward, W backward) wider than 64, a halo or intermediates beyond the LDS, a rank
 * above 256.  Nothing is launched in any of these cases; B == 0 succeeds with nothing launched. */
enum { TADMM_CONV_CHAIN_FWD = 0, TADMM_CONV_CHAIN_BWD = 1 };
int tadmm_ttconv_fused_save(tadmm_handle h, const tadmm_conv_chain_desc* d, int r1, int r2, void* H1, void* H2, void* stream);
int tadmm_ttconv_fused_bwd(tadmm_handle h, const tadmm_conv_chain_desc* d, int r1, int r2, void* dH1, void* dH2, void* stream);
int tadmm_ttconv_fused_plan(const tadmm_conv_chain_desc* d, int mode, int* tile_pixels, int* tile_rows, int* halo_tiles,
                            int* tiles_per_image, size_t* lds_bytes);

/* ---- k x k core convolution of the factorised layers (csrc/coreconv.hip, csrc/wgrad.hip) ---------------------------
 * The convolution between the two 1x1 stages of TTConv2dM (TTConv.py:130-153) and TKConv2dC / TKConv2dM
 * (TKConv.py:93-98, :210-214), groups = 1, on contiguous NCHW tensors in place; any plane size and any rank:
 *   fwd    Y (B, R2, Ho, Wo) = conv(X (B, R1, H, W); Wc (R2, R1, kh, kw))       reads X, Wc planes; writes Y
 *   dgrad  X (B, R1, H, W)   = the data gradient for Y = dY                      reads Y, Wc planes; writes X
 *   wgrad  dW (R2, R1, kh, kw) float32, contiguous = the weight gradient         reads X and Y = dY; Wc is ignored
 * X and Y are both of `dtype` (TADMM_CHAIN_F32: exact three-plane bf16 split, fp32-GEMM accuracy; TADMM_CHAIN_BF16: one
 * plane; TADMM_CHAIN_F16 is refused with TADMM_ERR_INVALID by all three), element aligned: 16-byte, 8-byte or element accesses as base and run length allow.
 * Wc: fragment-major bf16 planes (3 for float32, 1 for bfloat16; plane p at Wc + p * wc_plane elements, 16-byte aligned)
 * of the tap-major matrix, as for W2 of tadmm_conv_chain_desc: fwd takes the (R2 x kh*kw*R1p) matrix with column
 * (ky*kw + kx)*R1p + c, R1p = R1 rounded up to 32 and rows rounded up to 32; dgrad takes the same packing of the
 * transposed core (R1 x kh*kw*R2p) -- the kernel maps taps to source pixels itself, nothing is flipped
 * (tadmm.ops.conv_core_planes builds both).
 * wgrad splits the reduction over (batch, output pixel) into slices as tadmm_wgrad does, one workgroup per (tap, tile,
 * slice): no atomics, bitwise reproducible, independent of what workspace and dW held before.  The workspace (16-byte
 * aligned) is needed when there is more than one slice; tadmm_core_conv_wgrad_workspace_bytes is host only and a pure
 * function of the descriptor's shapes.
 * TADMM_ERR_INVALID: a non-positive extent, stride or dilation, negative padding or B, Ho / Wo that are not the output
 * size of the geometry or an empty output plane, unknown dtype, a null or misaligned operand with B > 0, weight planes
 * too small or misaligned (fwd, dgrad); TADMM_ERR_WORKSPACE: workspace too small; TADMM_ERR_UNSUPPORTED: planes of 2^31
 * pixels and more, more than 4096 taps, 2^31 - 256 output pixels in the batch (wgrad), a halo beyond the LDS.  Nothing
 * is launched in any of these cases.  B == 0 succeeds with nothing launched (wgrad writes zeros). */
typedef struct {
  void* X; void* Y;
  const void* Wc;                             /* bf16 planes; ignored by wgrad */
  int64_t wc_plane;                           /* elements */
  int32_t B, R1, R2;
  int32_t H, W, Ho, Wo, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 */
} tadmm_core_conv_desc;
int tadmm_core_conv_desc_bytes(void);
int tadmm_core_conv_fwd(tadmm_handle h, const tadmm_core_conv_desc* d, void* stream);
int tadmm_core_conv_dgrad(tadmm_handle h, const tadmm_core_conv_desc* d, void* stream);
int tadmm_core_conv_wgrad_workspace_bytes(const tadmm_core_conv_desc* d, size_t* bytes, int* slices_out);
int tadmm_core_conv_wgrad(tadmm_handle h, const tadmm_core_conv_desc* d, float* dW, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- gathered TT-matrix chain: the lookup of the factorised embeddings (csrc/ttm_gather.hip) ------------------------
 * TTMEmbedding.py:96-129, TTEmbedding.py:91-118 and SVDEmbedding.py:34-42 as one launch.  Cores G_j of shape
 * (r[j], n[j], m[j], r[j+1]), j < d, float32 contiguous, r[0] == 1.  Token t carries index[t] in [0, n[0] ... n[d-1]),
 * split into (i_0 .. i_{d-1}) with i_0 slowest; with S_j = G_j[:, i_j, :, :]
 *   Y[t][j_0 .. j_{d-1}, b] = sum_{a_1 .. a_{d-1}} S_0[0, j_0, a_1] S_1[a_1, j_1, a_2] ... S_{d-1}[a_{d-1}, j_{d-1}, b],
 * Y (B, m[0] ... m[d-1] * r[d]) float32 contiguous, j_0 slowest.  The running product of a token stays in LDS; every row
 * of Y is written once.  An index outside the range is never used as an address: its row of Y is zeros, it adds
 * nothing to the gradients, and the forward adds 1 to *bad_count (int32, device; the caller zeroes it when it likes).
 * tadmm_ttm_gather_bwd writes dcores[j] (shape of core j) = the gradient of sum(Y * dY) for every j with dcores[j] !=
 * NULL, one launch per core.  order[j] (B int64 token positions, grouped by i_j, ascending inside a group: a stable sort)
 * and offsets[j] (n[j] + 1 int64: group i is order[j][offsets[j][i] .. offsets[j][i+1])) come from the caller; bad
 * tokens may sit in any group.  Workgroup i owns slice i of dcores[j], writes all of it (zeros where no token selects
 * it) and adds its tokens in the order given: no atomics, no memset, bitwise reproducible.
 * tadmm_ttm_gather_fits is host only and reads d, n, m, r alone: 1 when the launches take the shape (a token's products
 * fit the 160 KiB of LDS of a CU, forward and backward), 0 when not, TADMM_ERR_INVALID for d < 1, d > 4, r[0] != 1 or a
 * size <= 0.  *lds_bytes (nullable): dynamic LDS of the larger launch; *tile (nullable): tokens per forward workgroup;
 * both 0 for a core of 2^31 elements or more or a product of one token beyond 2^30 floats (0 is returned, unsized).
 * The two launches return TADMM_ERR_UNSUPPORTED where _fits returns 0; B == 0 succeeds (the backward writes zeros). */
#define TADMM_TTM_MAX_D 4
typedef struct {
  const float* cores[TADMM_TTM_MAX_D];
  float* dcores[TADMM_TTM_MAX_D];             /* backward only; NULL: core skipped */
  const int64_t* order[TADMM_TTM_MAX_D];      /* backward only */
  const int64_t* offsets[TADMM_TTM_MAX_D];    /* backward only */
  const void* index;                          /* B indices, int32 or int64, contiguous */
  const float* dY;                            /* backward only */
  float* Y;                                   /* forward only */
  int32_t* bad_count;                         /* forward only */
  int64_t B;
  int32_t d;
  int32_t index_dtype;                        /* 0: int32, 1: int64 */
  int32_t n[TADMM_TTM_MAX_D], m[TADMM_TTM_MAX_D], r[TADMM_TTM_MAX_D + 1];
  int32_t reserved;
} tadmm_ttm_desc;
/* sizeof(tadmm_ttm_desc) as the library was built */
int tadmm_ttm_desc_bytes(void);
int tadmm_ttm_gather_fits(const tadmm_ttm_desc* d, size_t* lds_bytes, int* tile);
int tadmm_ttm_gather_fwd(tadmm_handle h, const tadmm_ttm_desc* d, void* stream);
int tadmm_ttm_gather_bwd(tadmm_handle h, const tadmm_ttm_desc* d, void* stream);

/* ---- LSTM recurrence over a whole sequence (csrc/lstm.hip) ------------------------------------------------------------
 * ablation/tt_lstm_inference.py:44-77 for all T steps in ONE launch.  H = hidden size, gate order z = [i | f | g | o]:
 *   z_t = Xp[t] + h_{t-1} Whh^T,  i, f, o = S(z),  g = tanh(z),  c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)
 * S = Hardsigmoid (sigmoid == 0) or the logistic function (sigmoid == 1).  Xp (T, B, 4H) holds the input pre-activations
 * with the bias in them; Y (T, B, H) = every h_t; hT, cT, h0, c0 (B, H); all float32 and contiguous, any 4-byte aligned
 * base (16-byte stores and loads where the base is 16-byte aligned and H % 4 == 0, single elements otherwise).  h0 / c0
 * NULL: zeros.  A workgroup owns 16 batch rows and walks the sequence alone; h stays in LDS, c in registers.
 *   forward  W = the three bf16 planes of Whh packed gate by gate, each gate's H rows padded to Hp = ceil16(H), columns
 *            to ceil32(H): (3, 4Hp/16, ceil32(H)/32, 64, 8) in the fragment-major order of the chain entries
 *            (tadmm.ops.lstm_planes builds it), 16-byte aligned.
 *   _save    also writes G (T, B, 4H), the four gate ACTIVATIONS, and C (T, B, H), every c_t; Y, hT, cT are bitwise
 *            those of the plain entry.
 *   backward W = the planes of the transposed padded weight, (3, Hp/16, 4Hp/32, 64, 8) (lstm_planes(transpose=True)).
 *            Reads G, C, c0 and the output gradients dY (T, B, H), dhT, dcT (B, H) (each NULL: zeros); writes dZ
 *            (T, B, 4H) -- the gradient of the pre-activations, which is also the gradient of Xp -- and dh0, dc0 (B, H;
 *            NULL: not written).  The Hardsigmoid derivative is 1/6 where the saved activation is strictly between 0
 *            and 1, else 0.  dWhh = dZ^T [h0, Y[0 .. T-2]] and dbias = sum dZ are left to the caller (tadmm_wgrad).
 * tadmm_lstm_fits is host only and reads H alone: 1 when the launches take it (1 <= H <= 256: four waves of at most four
 * 16-unit tiles; the backward's LDS image of dz would allow 368), 0 when not (*lds_bytes is then 0),
 * TADMM_ERR_INVALID for a NULL descriptor or H < 1.  *lds_bytes (nullable): dynamic LDS of the larger launch;
 * *rows_per_wg (nullable): 16.  The launches return TADMM_ERR_UNSUPPORTED where _fits returns 0 and TADMM_ERR_INVALID for
 * T < 1, B < 1, sigmoid outside {0, 1}, T * B * 4H beyond 2^40 or a required pointer that is NULL or misaligned; nothing
 * is launched in any of these cases.  No atomics; bitwise reproducible; rows never influence one another. */
typedef struct {
  const float* Xp;                            /* forward */
  const void* W;                              /* forward: planes of Whh; backward: planes of its transpose */
  const float* h0;                            /* forward; nullable */
  const float* c0;                            /* forward and backward; nullable */
  float* Y;                                   /* forward */
  float* hT;                                  /* forward */
  float* cT;                                  /* forward */
  float* G;                                   /* _save writes it, backward reads it */
  float* C;                                   /* _save writes it, backward reads it */
  const float* dY;                            /* backward; nullable */
  const float* dhT;                           /* backward; nullable */
  const float* dcT;                           /* backward; nullable */
  float* dZ;                                  /* backward */
  float* dh0;                                 /* backward; nullable */
  float* dc0;                                 /* backward; nullable */
  int64_t T, B;
  int32_t H;
  int32_t sigmoid;                            /* 0: Hardsigmoid, 1: logistic */
} tadmm_lstm_desc;
/* sizeof(tadmm_lstm_desc) as the library was built */
int tadmm_lstm_desc_bytes(void);
int tadmm_lstm_fits(const tadmm_lstm_desc* d, size_t* lds_bytes, int* rows_per_wg);
int tadmm_lstm_seq_fwd(tadmm_handle h, const tadmm_lstm_desc* d, void* stream);
int tadmm_lstm_seq_fwd_save(tadmm_handle h, const tadmm_lstm_desc* d, void* stream);
int tadmm_lstm_seq_bwd(tadmm_handle h, const tadmm_lstm_desc* d, void* stream);

/* ---- distillation loss: base criterion, KD term and logit gradients (csrc/distill.hip) -------------------------------
 * losses.py: DistillationLoss around CrossEntropyLoss / LabelSmoothingCrossEntropy / SoftTargetCrossEntropy, and
 * xcompression/task_distill.py:721-724 soft_cross_entropy, for B rows of C logits in two launches.  s = outputs, k =
 * outputs_kd (may be the same memory as s), t = the teacher's logits: all of `dtype` (TADMM_CHAIN_F32 / _BF16 / _F16),
 * unit column stride, row strides s_ld / k_ld / t_ld >= C in elements, any element-aligned base (16-byte, 8-byte or
 * element accesses are chosen from the bases and strides).
 *   base_b = -sum_c q_bc log_softmax(s_b)_c   INDEX: q_b = (1-eps) onehot(labels[b]) + eps/C, mean over the kept rows
 *                                             DENSE: q_b = (1-eps) dense[b] + eps/C (float32 rows, stride dense_ld >= C),
 *                                                    mean over B
 *   kd_b     SOFT_KL: sum_c p_t (log p_t - log p_k), p = softmax(. / tau); total scaled by tau^2 / (B*C)
 *            HARD:    -log_softmax(k_b)[argmax_c t_bc], first maximal index; mean over B
 *            SOFT_CE: -sum_c softmax(t_b / tau)_c log_softmax(k_b / tau)_c; mean over B*C
 *   loss   = base when kd_kind is NONE, else (1-alpha) base + alpha kd (base_kind NONE: alpha kd).
 * INDEX rows: labels[b] == ignore_index drops the row from the base term and its denominator; any other label outside
 * [0, C) does the same and is counted as bad; labels are compared, never used as an address.  No kept row: NaN.
 * Outputs: loss_dev[0] (double), loss_f32_dev[0] (nullable: the same value rounded once), counts_dev[0] = kept rows (B
 * unless INDEX), counts_dev[1] = bad labels; all three are overwritten.  grad_s / grad_k (nullable, float32, contiguous
 * B x C, 4-byte aligned): d loss / d s and d loss / d k; equal pointers receive the sum of the two (the caller's choice
 * when s and k are one tensor).  Rows that are not kept get exact zeros in grad_s.
 * workspace: tadmm_distill_workspace_bytes (host only, reads B alone) bytes, 8-byte aligned: two doubles and one int32
 * per row, each array rounded up to 256 bytes.  Every logit is shifted by its row maximum before exp; sums are double;
 * no floating-point atomics; bitwise reproducible; no host synchronisation.
 * TADMM_ERR_INVALID, with nothing launched: a NULL handle or descriptor, B < 1 or C < 1, an unknown kind or dtype, both
 * kinds NONE, a pointer the chosen kinds read that is NULL (s for a base kind; k, t for a KD kind; labels; dense;
 * loss_dev; counts_dev), a pointer not aligned to its element, a row stride below C, eps outside [0, 1], tau <= 0 where
 * tau is used (SOFT_KL, SOFT_CE).  TADMM_ERR_WORKSPACE: workspace NULL, misaligned or short. */
enum { TADMM_DISTILL_BASE_NONE = 0, TADMM_DISTILL_BASE_INDEX = 1, TADMM_DISTILL_BASE_DENSE = 2 };
enum { TADMM_DISTILL_KD_NONE = 0, TADMM_DISTILL_KD_SOFT_KL = 1, TADMM_DISTILL_KD_HARD = 2, TADMM_DISTILL_KD_SOFT_CE = 3 };
typedef struct {
  const void* s; const void* k; const void* t;
  int64_t s_ld, k_ld, t_ld;                   /* elements */
  const int64_t* labels;                      /* INDEX */
  const float* dense; int64_t dense_ld;       /* DENSE */
  void* workspace; size_t workspace_bytes;
  double* loss_dev;
  float* loss_f32_dev;                        /* nullable */
  int64_t* counts_dev;                        /* [kept rows, bad labels] */
  float* grad_s; float* grad_k;               /* nullable */
  int64_t ignore_index;
  double eps, alpha, tau;
  int32_t B, C;
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 | TADMM_CHAIN_F16 */
  int32_t base_kind, kd_kind;
  int32_t reserved;
} tadmm_distill_desc;
/* sizeof(tadmm_distill_desc) as the library was built */
int tadmm_distill_desc_bytes(void);
int tadmm_distill_workspace_bytes(const tadmm_distill_desc* d, size_t* bytes);
int tadmm_distill_loss(tadmm_handle h, const tadmm_distill_desc* d, void* stream);

/* ---- BERT self-attention: scores, softmax, dropout mask and context in one launch (csrc/attn.hip) -------------------
 * The body of xcompression/transformer/compressed_modeling*.py: *BertSelfAttention.forward after the projections.
 * q, k, v: (B, S, H*d) of `dtype`, read in place by heads: unit element stride, row strides q_ld / k_ld / v_ld >= H*d and
 * batch strides q_bs / k_bs / v_bs in elements (a slice of a packed (B, S, 3*H*d) tensor has ld = 3*H*d, bs = S*3*H*d),
 * any element-aligned base.
 *   scores[b,h,i,j] = (Q[b,i,h,:] . K[b,j,h,:]) / sqrt(d) + mask[b,j]      mask: float32 (B, S), nullable (zeros);
 *                                                                           -inf allowed in rows that keep a finite entry
 *   P = softmax_j(scores);  Pd = P * (keep != 0) / (1 - p)                  keep: bytes (B, H, S, S), read when p > 0
 *   ctx[b,i,h*d:(h+1)*d] = sum_j Pd[b,h,i,j] V[b,j,h,:]                     ctx: (B, S, H*d) contiguous, of `dtype`
 * tadmm_attn_fwd writes ctx, scores ((B, H, S, S) contiguous, of `dtype`; nullable: not written) and stats (float32
 * (B, H, S, 2): m = the row maximum and l = sum_j exp(score - m), so that lse = m + log l; nullable).  One launch.
 * tadmm_attn_bwd reads q, k, v, mask, keep, stats and the upstream gradients g_ctx (of ctx) and g_sc (of scores), both
 * contiguous, of `dtype`, each nullable (zeros), and writes dq, dk, dv ((B, S, H*d) contiguous, of `dtype`):
 *   dPd = (g_ctx V^T) keep / (1-p),  D_i = sum_j P_ij dPd_ij,  dS = g_sc + P (dPd - D)
 *   dQ = dS K / sqrt(d),  dK = dS^T Q / sqrt(d),  dV = Pd^T g_ctx
 * with P recomputed from q, k, mask and stats as exp(s - m) / l, the forward's own expression (a single rounded lse
 * would cost float32 parity).  Two launches (query-row blocks: D and dQ; key blocks: dK and dV); the
 * workspace (tadmm_attn_workspace_bytes: one double per (b, h, i), rounded up to 256 bytes; 8-byte aligned) carries D
 * from the first to the second and is needed when g_ctx is given.  No atomics; bitwise reproducible; no host
 * synchronisation.  float32 products are exact (v_mfma_f32_16x16x4_f32); the 16-bit types use
 * v_mfma_f32_16x16x32_{bf16,f16} with float32 accumulation; the softmax is float32.
 * tadmm_attn_fits is host only and reads H, S, d and dtype: 1 when the launches take the shape (1 <= S <= 512,
 * 1 <= d <= 64), 0 when not, TADMM_ERR_INVALID for a NULL descriptor or S < 1, d < 1, H < 1.  *lds_bytes (nullable): the
 * static LDS of the larger launch.  The launches return TADMM_ERR_UNSUPPORTED where _fits returns 0 and
 * TADMM_ERR_INVALID, with nothing launched, for: a NULL handle or descriptor; an unknown dtype; TADMM_CHAIN_F16 in _bwd;
 * q, k, v NULL or not element aligned; a row stride below H*d; any other pointer not aligned to its element; p outside
 * [0, 1); p > 0 without keep; ctx NULL (_fwd); stats, dq, dk or dv NULL (_bwd).  TADMM_ERR_WORKSPACE: g_ctx given and the
 * workspace NULL, misaligned or short.  B == 0 succeeds and launches nothing. */
typedef struct {
  const void* q; const void* k; const void* v;
  int64_t q_ld, k_ld, v_ld;                   /* row strides, elements */
  int64_t q_bs, k_bs, v_bs;                   /* batch strides, elements */
  const float* mask;                          /* (B, S); nullable */
  const uint8_t* keep;                        /* (B, H, S, S); required when p > 0 */
  void* ctx;                                  /* forward */
  void* scores;                               /* forward; nullable */
  float* stats;                               /* forward writes it (nullable), backward reads it */
  const void* g_ctx; const void* g_sc;        /* backward; each nullable */
  void* dq; void* dk; void* dv;               /* backward */
  void* workspace; size_t workspace_bytes;    /* backward with g_ctx */
  double p;                                   /* dropout probability, [0, 1) */
  int64_t B;
  int32_t H, S, d;
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 | TADMM_CHAIN_F16 (forward only) */
} tadmm_attn_desc;
/* sizeof(tadmm_attn_desc) as the library was built */
int tadmm_attn_desc_bytes(void);
int tadmm_attn_fits(const tadmm_attn_desc* d, size_t* lds_bytes);
int tadmm_attn_workspace_bytes(const tadmm_attn_desc* d, size_t* bytes);
int tadmm_attn_fwd(tadmm_handle h, const tadmm_attn_desc* d, void* stream);
int tadmm_attn_bwd(tadmm_handle h, const tadmm_attn_desc* d, void* stream);

/* ---- BERT sub-layer tail: dropout, residual add and LayerNorm in one launch (csrc/bertnorm.hip) ---------------------
 * xcompression/transformer/compressed_modeling*.py: LayerNorm(dropout(x) + res) of *SelfOutput, BertOutput, BertEmbeddings
 * and BertPredictionHeadTransform, with the reference's BertLayerNorm (epsilon inside the root).  x, res: (rows, hidden)
 * of `dtype`, read in place: unit element stride, row strides x_ld / res_ld >= hidden in elements, any element-aligned
 * base (16-byte accesses when every base is 16-byte aligned, the row strides are whole 16-byte units and hidden is a
 * multiple of 16 bytes of elements; element accesses otherwise).  res is nullable (zeros).
 *   s_ij   = x_ij * (keep_ij != 0) / (1 - p) + res_ij        keep: bytes (rows, hidden) contiguous, read when p > 0
 *   mean_i = sum_j s_ij / hidden,  var_i = sum_j (s_ij - mean_i)^2 / hidden,  rstd_i = 1 / sqrt(var_i + eps)
 *   y_ij   = gamma_j (s_ij - mean_i) rstd_i + beta_j         gamma, beta: (hidden) of `param_dtype`: float32 or `dtype`
 * Elementwise arithmetic is float32; the two row sums (of s, and of (s - mean)^2 over the row held in registers) are added
 * in double, so mean and rstd are exact values rounded once to float32.
 * tadmm_bertnorm_fwd writes y ((rows, hidden) contiguous, of `dtype`) and stats (float32 (rows, 2) = (mean, rstd);
 * nullable).  One launch.
 * tadmm_bertnorm_bwd reads x, res, keep, gamma, stats and g (the gradient of y: contiguous, of `dtype`), recomputes s and
 * xhat = (s - mean) rstd with the forward's expressions and writes, each nullable and contiguous of `dtype`,
 *   dres_ij = rstd_i (a_ij - mean_j a_i. - xhat_ij mean_j(a_i. xhat_i.)),  a = g gamma;    dx = dres keep / (1 - p)
 * (dx and dres must be two buffers) and, each nullable, float32 (hidden): dgamma_j = sum_i g_ij xhat_ij, dbeta_j =
 * sum_i g_ij.  Two launches: row blocks (per-workgroup partial sums to the workspace), then a fixed-order sum of the
 * partials in double; the second and the workspace (tadmm_bertnorm_workspace_bytes, reads rows and hidden; 16-byte
 * aligned) are needed only when dgamma or dbeta is given.  No atomics; grids depend on (rows, hidden, dtype) alone:
 * bitwise reproducible; no host synchronisation.
 * tadmm_bertnorm_fits is host only and reads hidden: 1 for 1 <= hidden <= HMAX (2048; *hmax, nullable, receives it), 0
 * above, TADMM_ERR_INVALID for a NULL descriptor or hidden < 1.  The launches return TADMM_ERR_UNSUPPORTED where _fits
 * returns 0 and TADMM_ERR_INVALID, with nothing launched, for: a NULL handle or descriptor; rows < 0 or hidden < 1; an
 * unknown dtype; TADMM_CHAIN_F16 in _bwd; a param_dtype that is neither float32 nor dtype; x NULL; a pointer not aligned
 * to its element; a row stride below hidden; p outside [0, 1); p > 0 without keep; eps negative or not finite; gamma NULL
 * (beta too in _fwd); y NULL (_fwd); stats or g NULL (_bwd); dx == dres.  TADMM_ERR_WORKSPACE: dgamma or dbeta given and
 * the workspace NULL, misaligned or short.  rows == 0 succeeds and launches nothing. */
typedef struct {
  const void* x; const void* res;             /* res nullable */
  int64_t x_ld, res_ld;                       /* row strides, elements */
  const uint8_t* keep;                        /* (rows, hidden); required when p > 0 */
  const void* gamma; const void* beta;        /* (hidden) of param_dtype */
  void* y;                                    /* forward */
  float* stats;                               /* forward writes it (nullable), backward reads it */
  const void* g;                              /* backward */
  void* dx; void* dres;                       /* backward; each nullable */
  float* dgamma; float* dbeta;                /* backward; each nullable */
  void* workspace; size_t workspace_bytes;    /* backward with dgamma or dbeta */
  double p;                                   /* dropout probability, [0, 1) */
  double eps;
  int64_t rows;
  int32_t hidden;
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 | TADMM_CHAIN_F16 (forward only) */
  int32_t param_dtype;                        /* TADMM_CHAIN_F32 | dtype */
  int32_t reserved;
} tadmm_bertnorm_desc;
/* sizeof(tadmm_bertnorm_desc) as the library was built */
int tadmm_bertnorm_desc_bytes(void);
int tadmm_bertnorm_fits(const tadmm_bertnorm_desc* d, int* hmax);
int tadmm_bertnorm_workspace_bytes(const tadmm_bertnorm_desc* d, size_t* bytes);
int tadmm_bertnorm_fwd(tadmm_handle h, const tadmm_bertnorm_desc* d, void* stream);
int tadmm_bertnorm_bwd(tadmm_handle h, const tadmm_bertnorm_desc* d, void* stream);

/* ---- Pre-norm block tail: branch dropout, DropPath, residual add and LayerNorm in one launch (csrc/prenorm.hip) --------
 * vit_tt.py: TTBlock through timm's Block.forward, x = x + drop_path(branch(norm(x))), where the next branch reads the
 * LayerNorm of the new stream: both the stream and its LayerNorm are outputs.  x (the stream), b (the branch output):
 * (rows, hidden) of `dtype`, read in place: unit element stride, row strides x_ld / b_ld >= hidden in elements, any
 * element-aligned base (16-byte accesses when every base is 16-byte aligned, the row strides are whole 16-byte units and
 * hidden is a multiple of 16 bytes of elements; element accesses otherwise).  rows = B * rows_per_sample.
 *   scale_i = (path_keep[i / rows_per_sample] != 0) / (1 - p_path)    path_keep: bytes (B), read when p_path > 0; else 1
 *   s_ij    = x_ij + scale_i b_ij (keep_ij != 0) / (1 - p)            keep: bytes (rows, hidden) contiguous, read when p > 0
 *   mean_i, rstd_i = 1 / sqrt(var_i + eps) of s_i as stored (rounded to `dtype`), biased variance, sums added in double
 *   y_ij    = gamma_j (s_ij - mean_i) rstd_i + beta_j                 gamma, beta: (hidden) of `param_dtype`
 * tadmm_prenorm_fwd writes s and y ((rows, hidden) contiguous, of `dtype`, two buffers) and stats (float32 (rows, 2) =
 * (mean, rstd); nullable).  One launch.  A row of a sample that DropPath drops has s == x bit for bit.
 * tadmm_prenorm_bwd reads s (as the forward wrote it), stats, gamma, keep, path_keep and the gradients g_y of y and g_s of
 * s (contiguous, of `dtype`; either may be NULL = zeros, not both) and writes, each nullable and contiguous of `dtype`,
 *   dx_ij = g_s_ij + rstd_i (a_ij - mean_j a_i. - xhat_ij mean_j(a_i. xhat_i.)),  a = g_y gamma,  xhat = (s - mean) rstd
 *   db_ij = dx_ij scale_i (keep_ij != 0) / (1 - p)                    (an exact zero in a dropped sample)
 * (dx and db must be two buffers) and, each nullable, float32 (hidden): dgamma_j = sum_i g_y_ij xhat_ij, dbeta_j =
 * sum_i g_y_ij.  Two launches: row blocks (per-workgroup partial sums to the workspace), then the fixed-order sum of the
 * partials in double that tadmm_bertnorm_bwd uses; the second and the workspace (tadmm_prenorm_workspace_bytes, reads rows
 * and hidden; 16-byte aligned) are needed only when dgamma or dbeta is given.  x, b, beta and y are not read.  No atomics;
 * grids depend on (rows, hidden, dtype) alone: bitwise reproducible; no host synchronisation.
 * tadmm_prenorm_fits is host only and reads hidden: 1 for 1 <= hidden <= HMAX (that of tadmm_bertnorm_fits; *hmax,
 * nullable, receives it), 0 above, TADMM_ERR_INVALID for a NULL descriptor or hidden < 1.  The launches return
 * TADMM_ERR_UNSUPPORTED where _fits returns 0 and TADMM_ERR_INVALID, with nothing launched, for: a NULL handle or
 * descriptor; rows < 0 or hidden < 1; rows_per_sample < 1 or rows not a multiple of it; an unknown dtype; TADMM_CHAIN_F16
 * in _bwd; a param_dtype that is neither float32 nor dtype; p or p_path outside [0, 1); p > 0 without keep; p_path > 0
 * without path_keep; eps negative or not finite; gamma or s NULL; a pointer not aligned to its element; in _fwd x, b, beta
 * or y NULL, a row stride below hidden, y == s; in _bwd stats NULL, g_y and g_s both NULL, dx == db.
 * TADMM_ERR_WORKSPACE: dgamma or dbeta given and the workspace NULL, misaligned or short.  rows == 0 succeeds and
 * launches nothing. */
typedef struct {
  const void* x; const void* b;               /* forward */
  int64_t x_ld, b_ld;                         /* row strides, elements */
  const uint8_t* keep;                        /* (rows, hidden); required when p > 0 */
  const uint8_t* path_keep;                   /* (rows / rows_per_sample); required when p_path > 0 */
  const void* gamma; const void* beta;        /* (hidden) of param_dtype */
  void* s;                                    /* forward writes it, backward reads it */
  void* y;                                    /* forward */
  float* stats;                               /* forward writes it (nullable), backward reads it */
  const void* g_y; const void* g_s;           /* backward; either nullable */
  void* dx; void* db;                         /* backward; each nullable */
  float* dgamma; float* dbeta;                /* backward; each nullable */
  void* workspace; size_t workspace_bytes;    /* backward with dgamma or dbeta */
  double p;                                   /* dropout probability of the branch output, [0, 1) */
  double p_path;                              /* DropPath probability, [0, 1) */
  double eps;
  int64_t rows;
  int64_t rows_per_sample;
  int32_t hidden;
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 | TADMM_CHAIN_F16 (forward only) */
  int32_t param_dtype;                        /* TADMM_CHAIN_F32 | dtype */
  int32_t reserved;
} tadmm_prenorm_desc;
/* sizeof(tadmm_prenorm_desc) as the library was built */
int tadmm_prenorm_desc_bytes(void);
int tadmm_prenorm_fits(const tadmm_prenorm_desc* d, int* hmax);
int tadmm_prenorm_workspace_bytes(const tadmm_prenorm_desc* d, size_t* bytes);
int tadmm_prenorm_fwd(tadmm_handle h, const tadmm_prenorm_desc* d, void* stream);
int tadmm_prenorm_bwd(tadmm_handle h, const tadmm_prenorm_desc* d, void* stream);

/* ---- ResNet block tail: BatchNorm2d, shortcut add and ReLU (csrc/bnact.hip) -------------------------------------------
 * resnet_cifar_tt.py / resnet_inet_tt.py: relu(bn(conv(x))) and relu(bn(conv(x)) + shortcut(x)).  x: (N, C, H, W) of
 * `dtype`, NCHW contiguous, any element-aligned base (16-byte accesses when every contiguous base is 16-byte aligned and
 * H W is a whole number of 16-byte units; element accesses otherwise).  M = N H W values per channel.  gamma, beta,
 * running_mean, running_var: float32 (C).
 *   z = gamma_c (x - mean_c) rstd_c + beta_c + [c0 <= c < c0 + Cr] res[n, c - c0, h, w],   y = relu ? max(z, 0) : z
 * res (nullable) is (N, Cr, H, W) of `dtype` read through the four element strides res_stride (>= 0): a plain tensor, or
 * the option-A shortcut x_in[:, :, ::2, ::2] at channel offset c0 = planes / 4; channels outside the window get none.
 * tadmm_bnact_fwd with training != 0, two launches: per-(channel, split) sums of x - K and (x - K)^2 in double to the
 * workspace (K = x[0, c, 0, 0], so a channel with mean >> std keeps its variance), then every workgroup adds its
 * channel's partials in a fixed order, mean_c and rstd_c = 1 / sqrt(var_c + eps) (biased variance) stay in double for
 * y and are rounded once into stats (float32 (C, 2) = (mean, rstd); nullable).  running_mean and running_var (given
 * together, or both NULL) become (1 - momentum) old + momentum new, the new variance unbiased (M / (M - 1));
 * num_batches_tracked (int64, nullable) rises by one.  With training == 0, one launch: a_c = gamma_c / sqrt(running_var_c
 * + eps), b_c = beta_c - running_mean_c a_c, y = act(a x + b + res); stats, the running statistics and the counter are
 * not written and no workspace is needed.
 * tadmm_bnact_bwd (training mode; float32 and bfloat16) reads g (the gradient of y, contiguous), y as the forward stored
 * it (only when relu), x, stats and gamma; gz = g (y > 0), or g without relu; xhat = (x - mean) rstd from stats.  Two
 * launches: partial sums of gz and gz xhat in double (and dres = gz over the window, contiguous (N, Cr, H, W)), then
 *   dbeta_c = sum gz,  dgamma_c = sum gz xhat  (float32 (C)),   dx = gamma rstd (gz - dbeta / M - xhat dgamma / M).
 * Every output is nullable; without dx the second launch only adds the partials; with dres alone there is one launch and
 * no workspace; with no output nothing is launched.  c0 and Cr are read when dres is given.
 * No atomics; grids depend on (N, C, H W, dtype) alone: bitwise reproducible; no host synchronisation.  The workspace
 * (tadmm_bnact_workspace_bytes, reads N, C, H, W, dtype; 16-byte aligned) is sized for C min(trips, 128, ceil(2048 / C))
 * pairs of doubles, a trip being 256 * 16 / sizeof(element) values (at most 2048); a channel's splits are that many,
 * evened out so that none is empty.  The size never falls as N, H or W grows.  tadmm_bnact_plan is host only and refuses
 * as _workspace_bytes does: plan3 = S, span, cap -- the S workgroups of a channel own `span` consecutive values each (a
 * whole number of trips) and the workspace is sized for `cap` of them.
 * tadmm_bnact_fits is host only: 1 for N H W <= 2^31 - 4096 (*max_m, nullable, receives the bound), 0 above,
 * TADMM_ERR_INVALID for a NULL descriptor or N, C, H or W < 1.  The launches return TADMM_ERR_UNSUPPORTED where _fits
 * returns 0 and TADMM_ERR_INVALID, with nothing launched, for: a NULL handle or descriptor; N, C, H or W < 1; training
 * (and _bwd) with M < 2; an unknown dtype; TADMM_CHAIN_F16 in _bwd; res (dres in _bwd) with c0 < 0, Cr < 1 or
 * c0 + Cr > C; a negative stride; eps negative or not finite; momentum outside [0, 1]; x or gamma NULL; a pointer not
 * aligned to its element; in _fwd beta or y NULL, y == x or y == res, eval mode without running statistics, one running
 * statistic without the other; in _bwd stats or g NULL, y NULL with relu, dx == dres.  TADMM_ERR_WORKSPACE: the
 * workspace is needed and NULL, misaligned or short. */
typedef struct {
  const void* x; const void* res;             /* res nullable (forward) */
  int64_t res_stride[4];                      /* elements: n, channel, h, w */
  const float* gamma; const float* beta;      /* (C) */
  float* running_mean; float* running_var;    /* (C); training updates them (nullable there), eval reads them */
  int64_t* num_batches_tracked;               /* training: += 1; nullable */
  void* y;                                    /* forward writes it, backward reads it when relu */
  float* stats;                               /* training forward writes it (nullable), backward reads it */
  const void* g;                              /* backward */
  void* dx; void* dres;                       /* backward; each nullable */
  float* dgamma; float* dbeta;                /* backward; each nullable */
  void* workspace; size_t workspace_bytes;    /* training forward; backward with dx, dgamma or dbeta */
  double eps;
  double momentum;                            /* [0, 1] */
  int32_t N, C, H, W;
  int32_t c0, Cr;                             /* the residual's channel window */
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 | TADMM_CHAIN_F16 (forward only) */
  int32_t training;                           /* forward: nonzero = batch statistics, 0 = running statistics */
  int32_t relu;
  int32_t reserved;
} tadmm_bnact_desc;
/* sizeof(tadmm_bnact_desc) as the library was built */
int tadmm_bnact_desc_bytes(void);
int tadmm_bnact_fits(const tadmm_bnact_desc* d, int64_t* max_m);
int tadmm_bnact_workspace_bytes(const tadmm_bnact_desc* d, size_t* bytes);
int tadmm_bnact_plan(const tadmm_bnact_desc* d, int32_t* plan3);
int tadmm_bnact_fwd(tadmm_handle h, const tadmm_bnact_desc* d, void* stream);
int tadmm_bnact_bwd(tadmm_handle h, const tadmm_bnact_desc* d, void* stream);

/* ---- MobileNetV2 depthwise stage: depthwise 3x3 convolution, BatchNorm2d and ReLU6 (csrc/dwbn.hip) -------------------
 * mobilenetv2_cifar_tt.py / mobilenetv2_tt.py: relu6(bn(depthwise_conv3x3(x))).  x: (N, C, H, W) of `dtype`, NCHW
 * contiguous; w: float32 (C, 1, 3, 3); kernel 3, padding 1, dilation 1, depth multiplier 1, no bias, stride s = 1 or 2.
 * The output plane is Ho = (H - 1) / s + 1 by Wo = (W - 1) / s + 1; M = N Ho Wo output values per channel.  gamma, beta,
 * running_mean, running_var: float32 (C).
 *   z[n,c,i,j] = sum_{a,b} w[c,a,b] x[n,c, i s + a - 1, j s + b - 1]   (zero outside the plane; float32, taps in the order
 *                                                                       a, b ascending)
 *   y = min(max(gamma_c (z - mean_c) rstd_c + beta_c, 0), 6)
 * Accesses are 16 bytes wide when x, y (z, g, dx) are 16-byte aligned and W and Wo are whole numbers of 16-byte units, one
 * element otherwise; any element-aligned base is taken.
 * tadmm_dwbn_fwd with training != 0, two launches: z, stored in `dtype` (N, C, Ho, Wo), with per-(channel, split) sums
 * of z - K and (z - K)^2 of z as stored, in double, K = z[0, c, 0, 0]; then every workgroup adds its channel's partials in
 * a fixed order, mean_c and rstd_c = 1 / sqrt(var_c + eps) (biased variance) stay in double for y and are rounded once
 * into stats (float32 (C, 2) = (mean, rstd); nullable).  running_mean and running_var (given together, or both NULL)
 * become (1 - momentum) old + momentum new, the new variance unbiased (M / (M - 1)); num_batches_tracked (int64,
 * nullable) rises by one.  With training == 0, one launch: a_c = gamma_c / sqrt(running_var_c + eps), b_c = beta_c -
 * running_mean_c a_c (folded in double), y = clamp(a conv(x) + b); z, stats, the running statistics and the counter are
 * not written and no workspace is needed.
 * tadmm_dwbn_bwd (training mode; float32 and bfloat16) reads g (the gradient of y, contiguous), y and z as the forward
 * stored them, x, w, stats and gamma; gz = g (0 < y < 6); xhat = (z - mean) rstd from stats.  Three launches: partial
 * sums of gz and gz xhat in double; then dbeta_c = sum gz, dgamma_c = sum gz xhat (float32 (C)),
 *   dz = gamma rstd (gz - dbeta / M - xhat dgamma / M)   (formed on a haloed tile on chip, never stored),
 *   dx[n,c,h,w] = sum_{a,b} w[c,a,b] dz[n,c,(h + 1 - a) / s,(w + 1 - b) / s]   (terms with whole quotients inside the plane)
 * and per-workgroup partials of dw[c,a,b] = sum_{n,i,j} dz[n,c,i,j] x[n,c, i s + a - 1, j s + b - 1] in double; then dw
 * (float32 (C, 1, 3, 3)) from the partials in a fixed order, in double.  dx, dw, dgamma and dbeta are each nullable;
 * without dw there are two launches; with no output nothing is launched.
 * No atomics; grids depend on (N, C, H, W, stride) alone: bitwise reproducible; no host synchronisation.  Ownership
 * (tadmm_dwbn_plan, host only, plan6 = G, RB, NB, U, S, per): a plane whose haloed input and haloed dz each fit 4096
 * floats is taken whole, G images to a tile (at most 2048 outputs); a larger one is cut into NB bands of RB output rows;
 * the U = ceil(N / G) NB units of a channel go to S workgroups of `per` consecutive units.  The workspace
 * (tadmm_dwbn_workspace_bytes; 16-byte aligned) holds 11 doubles for each of C min(128, ceil(1024 / C)) splits; it
 * depends on C alone, so it never falls as N, H or W grows.
 * tadmm_dwbn_fits is host only: 1 for W <= 1363 (*max_w, nullable, receives the bound) and N H W <= 2^31 - 4096, 0
 * above, TADMM_ERR_INVALID for a NULL descriptor, N, C, H or W < 1 or a stride other than 1 and 2.  The launches return
 * TADMM_ERR_UNSUPPORTED where _fits returns 0 and TADMM_ERR_INVALID, with nothing launched, for: a NULL handle or
 * descriptor; N, C, H or W < 1; a stride other than 1 and 2; training (and _bwd) with M < 2; an unknown dtype;
 * TADMM_CHAIN_F16 in _bwd; eps negative or not finite; momentum outside [0, 1]; x, w, gamma or y NULL; z NULL in
 * training mode and _bwd; a pointer not aligned to its element; in _fwd beta NULL, y == x, z == x or z == y, eval mode
 * without running statistics, one running statistic without the other; in _bwd stats or g NULL, dx equal to x, g, y or
 * z.  TADMM_ERR_WORKSPACE: the workspace is needed and NULL, misaligned or short. */
typedef struct {
  const void* x;                              /* (N, C, H, W) */
  const float* w;                             /* (C, 1, 3, 3) */
  const float* gamma; const float* beta;      /* (C) */
  float* running_mean; float* running_var;    /* (C); training updates them (nullable there), eval reads them */
  int64_t* num_batches_tracked;               /* training: += 1; nullable */
  void* z;                                    /* (N, C, Ho, Wo); training forward writes it, backward reads it */
  void* y;                                    /* (N, C, Ho, Wo); forward writes it, backward reads it */
  float* stats;                               /* training forward writes it (nullable), backward reads it */
  const void* g;                              /* backward */
  void* dx;                                   /* backward; nullable */
  float* dw; float* dgamma; float* dbeta;     /* backward; each nullable */
  void* workspace; size_t workspace_bytes;    /* training forward; backward with any output */
  double eps;
  double momentum;                            /* [0, 1] */
  int32_t N, C, H, W;
  int32_t stride;                             /* 1 or 2 */
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 | TADMM_CHAIN_F16 (forward only) */
  int32_t training;                           /* forward: nonzero = batch statistics, 0 = running statistics */
  int32_t reserved;
} tadmm_dwbn_desc;
/* sizeof(tadmm_dwbn_desc) as the library was built */
int tadmm_dwbn_desc_bytes(void);
int tadmm_dwbn_fits(const tadmm_dwbn_desc* d, int32_t* max_w);
int tadmm_dwbn_plan(const tadmm_dwbn_desc* d, int32_t* plan6);
int tadmm_dwbn_workspace_bytes(const tadmm_dwbn_desc* d, size_t* bytes);
int tadmm_dwbn_fwd(tadmm_handle h, const tadmm_dwbn_desc* d, void* stream);
int tadmm_dwbn_bwd(tadmm_handle h, const tadmm_dwbn_desc* d, void* stream);

/* ---- DenseNet pre-activation: BatchNorm2d and ReLU over a list of feature tensors (csrc/densebn.hip) ------------------
 * densenet_cifar_tt.py / densenet_inet_tt.py: relu(bn(torch.cat(features, 1))) in front of every convolution of a dense
 * block, with neither the concatenation nor a second statistics pass over channels an earlier layer has seen.
 * Segment k = 0 .. nseg - 1 (nseg <= TADMM_DENSEBN_MAX_SEGMENTS) is x_k: (N, C_k, H, W) of `dtype`, NCHW contiguous, any
 * element-aligned base; channel c of the concatenation, C = sum C_k wide, is channel c - first_k of the segment with
 * first_k <= c < first_k + C_k.  M = N H W values per channel.  16-byte accesses when every base in use is 16-byte
 * aligned and H W is a whole number of 16-byte units; element accesses otherwise.  The segment table travels in the
 * kernel arguments: no host-to-device copy, no host synchronisation.  gamma, beta, running_mean, running_var: float32
 * (C), those of the consuming layer.
 * tadmm_densebn_stats takes ONE segment (nseg == 1; seg[0].x, seg[0].stats, seg[0].C), two launches: per-(channel,
 * split) sums of x - K and (x - K)^2 in double to the workspace (K = x[0, c, 0, 0], so a channel with mean >> std keeps
 * its variance), then the partials of a channel are added in ascending order into stats_k, double (C_k, 2) = (mean,
 * biased variance).  The variance is stored, not rstd: a channel's batch statistics are the same for every later layer
 * of the block, and every consuming layer applies its own eps.
 * tadmm_densebn_fwd with training != 0, ONE launch: rstd_c = 1 / sqrt(var_c + eps) in double from the segment's stats,
 *   y[n, c, h, w] = act(gamma_c (x_k[n, c - first_k, h, w] - mean_c) rstd_c + beta_c),    act = relu or the identity,
 * written to one contiguous (N, C, H, W) tensor.  running_mean and running_var (given together, or both NULL) become
 * (1 - momentum) old + momentum new, the new variance unbiased (M / (M - 1)); num_batches_tracked (int64, nullable)
 * rises by one.  With training == 0, one launch: a_c = gamma_c / sqrt(running_var_c + eps), b_c = beta_c -
 * running_mean_c a_c, y = act(a x + b); no stats are read, nothing but y is written.  The forward needs no workspace.
 * tadmm_densebn_bwd (training mode; float32 and bfloat16) reads g (the gradient of y, contiguous (N, C, H, W)), y as the
 * forward stored it (only when relu), every x_k and stats_k, gamma and eps; gz = g (y > 0), or g without relu; xhat =
 * (x - mean) rstd.  Two launches: partial sums of gz and gz xhat in double, then
 *   dbeta_c = sum gz,  dgamma_c = sum gz xhat  (float32 (C), each nullable),   dx = gamma rstd (gz - dbeta / M - xhat dgamma / M)
 * with dx written per segment into seg[k].dx, that segment's own contiguous (N, C_k, H, W) output.  A NULL seg[k].dx
 * means the segment wants no gradient: its channels are only summed (and not even that without dgamma and dbeta).
 * With no output nothing is launched.
 * No atomics; grids depend on (N, C, H W, dtype) alone: bitwise reproducible.  The workspace
 * (tadmm_densebn_workspace_bytes, reads N, H, W, dtype, nseg and every C_k; 16-byte aligned) is sized as bnact's for the
 * C = sum C_k channels of the call: C min(trips, 128, ceil(2048 / C)) pairs of doubles.  _stats and _bwd need it.
 * tadmm_densebn_plan is host only and refuses as _workspace_bytes does: plan3 = S, span, cap as tadmm_bnact_plan writes
 * them, over the descriptor's channels -- one segment for the plan of its _stats launch, all of them for _fwd and _bwd.
 * tadmm_densebn_fits is host only: 1 for N H W <= 2^31 - 4096 (*max_m, nullable, receives the bound), nseg <=
 * TADMM_DENSEBN_MAX_SEGMENTS and C <= (2^31 - 1) / 128, 0 above, TADMM_ERR_INVALID for a NULL descriptor, N, H, W or nseg
 * < 1 or a C_k < 1.  The launches return TADMM_ERR_UNSUPPORTED where N H W or C is above the bound and
 * TADMM_ERR_INVALID, with nothing launched, for: a NULL handle or descriptor; N, H or W < 1; nseg < 1 or above the
 * maximum (other than 1 in _stats); a C_k < 1; training (_stats, _bwd) with M < 2; an unknown dtype; TADMM_CHAIN_F16 in
 * _bwd; eps negative or not finite; momentum outside [0, 1]; an x_k or gamma NULL; a pointer not aligned to its element;
 * stats_k NULL in training mode, _stats and _bwd; in _fwd beta or y NULL, y overlapping a segment, eval mode without
 * running statistics, one running statistic without the other; in _bwd g NULL, y NULL with relu, a dx_k equal to x_k, g
 * or y.  TADMM_ERR_WORKSPACE: the workspace is needed and NULL, misaligned or short. */
#define TADMM_DENSEBN_MAX_SEGMENTS 128
typedef struct {
  const void* x;                              /* (N, C, H, W) */
  double* stats;                              /* (C, 2) = (mean, biased variance); _stats writes it, training reads it */
  void* dx;                                   /* backward; (N, C, H, W); nullable */
  int32_t C;
  int32_t reserved;
} tadmm_densebn_seg;
typedef struct {
  tadmm_densebn_seg seg[TADMM_DENSEBN_MAX_SEGMENTS];
  const float* gamma; const float* beta;      /* (sum C_k) */
  float* running_mean; float* running_var;    /* training updates them (nullable there), eval reads them */
  int64_t* num_batches_tracked;               /* training: += 1; nullable */
  void* y;                                    /* (N, sum C_k, H, W); forward writes it, backward reads it when relu */
  const void* g;                              /* backward */
  float* dgamma; float* dbeta;                /* backward; each nullable */
  void* workspace; size_t workspace_bytes;    /* _stats; backward with any output */
  double eps;
  double momentum;                            /* [0, 1] */
  int32_t N, H, W;
  int32_t nseg;
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 | TADMM_CHAIN_F16 (forward only) */
  int32_t training;                           /* forward: nonzero = batch statistics, 0 = running statistics */
  int32_t relu;
  int32_t reserved;
} tadmm_densebn_desc;
/* sizeof(tadmm_densebn_desc) as the library was built */
int tadmm_densebn_desc_bytes(void);
int tadmm_densebn_max_segments(void);
int tadmm_densebn_fits(const tadmm_densebn_desc* d, int64_t* max_m);
int tadmm_densebn_workspace_bytes(const tadmm_densebn_desc* d, size_t* bytes);
int tadmm_densebn_plan(const tadmm_densebn_desc* d, int32_t* plan3);
int tadmm_densebn_stats(tadmm_handle h, const tadmm_densebn_desc* d, void* stream);
int tadmm_densebn_fwd(tadmm_handle h, const tadmm_densebn_desc* d, void* stream);
int tadmm_densebn_bwd(tadmm_handle h, const tadmm_densebn_desc* d, void* stream);

/* ---- TinyBERT layer losses: masked attention MSE and hidden-state MSE with gradients (csrc/layermse.hip) -------------
 * xcompression/task_distill.py:810-828 (also task_distill1.py, task_distill2.py, general_distill.py:438-451) for all
 * pairs of a step in two launches.  A call carries npairs <= TADMM_LAYER_MSE_MAX_PAIRS pairs; pair i is s (student)
 * and t (teacher), n elements each, flat and dense, of `dtype` (TADMM_CHAIN_F32 / _BF16 / _F16; one type per call),
 * any element-aligned base (16-byte loads where both bases of the pair are 16-byte aligned, element loads otherwise).
 * With every value widened to float32 on load:
 *   s' = (clamp && s <= thr) ? 0 : s,  t' = (clamp && t <= thr) ? 0 : t,  d = s' - t'
 *   terms_dev[i] = scale * sum_e d^2                 (the caller folds weight / denominator into `scale`)
 *   grad[e]      = (clamp && s <= thr) ? 0 : 2 scale d      (float32, n elements, 4-byte aligned; nullable: not written)
 *   loss_dev[g]  = sum of terms_dev[i] over the pairs of group g, in pair order (0 when the group has none)
 * -inf is clamped; a NaN compares false and propagates.  d, d^2 and the sums are double; grad is rounded once.
 * Outputs: terms_dev[npairs] and loss_dev[2] (double), loss_f32_dev[2] (nullable: loss_dev rounded once); overwritten.
 * workspace: tadmm_layer_mse_workspace_bytes (host only; reads npairs and every n) bytes, 8-byte aligned: one double per
 * pair and workgroup of the streaming launch, min(chunks, max_blocks) of them, rounded up to 256 bytes, where a pair of n
 * elements has ceil(n / chunk_elems) chunks and tadmm_layer_mse_geometry reports chunk_elems and max_blocks.
 * No floating-point atomics; bitwise reproducible; no host synchronisation; all element offsets are 64-bit.
 * TADMM_ERR_INVALID, with nothing launched: a NULL handle or descriptor, npairs outside [1, max], n < 1, an unknown
 * dtype or group, s or t NULL, a pointer not aligned to its element, terms_dev or loss_dev NULL.  TADMM_ERR_UNSUPPORTED:
 * more than 2^31 - 1 chunks.  TADMM_ERR_WORKSPACE: workspace NULL, misaligned or short. */
#define TADMM_LAYER_MSE_MAX_PAIRS 32
enum { TADMM_LAYER_MSE_ATT = 0, TADMM_LAYER_MSE_REP = 1 };
typedef struct {
  const void* s; const void* t;
  float* grad;                                /* nullable */
  int64_t n;
  double scale;
  float thr;
  int32_t clamp;                              /* 0: thr is not read */
  int32_t group;                              /* TADMM_LAYER_MSE_ATT | TADMM_LAYER_MSE_REP */
  int32_t reserved;
} tadmm_layer_mse_pair;
typedef struct {
  tadmm_layer_mse_pair pairs[TADMM_LAYER_MSE_MAX_PAIRS];
  void* workspace; size_t workspace_bytes;
  double* terms_dev;                          /* [npairs] */
  double* loss_dev;                           /* [attention, hidden] */
  float* loss_f32_dev;                        /* nullable */
  int32_t npairs;
  int32_t dtype;                              /* TADMM_CHAIN_F32 | TADMM_CHAIN_BF16 | TADMM_CHAIN_F16 */
} tadmm_layer_mse_desc;
/* sizeof(tadmm_layer_mse_desc) as the library was built */
int tadmm_layer_mse_desc_bytes(void);
int tadmm_layer_mse_max_pairs(void);
int tadmm_layer_mse_geometry(int* chunk_elems, int* max_blocks);
int tadmm_layer_mse_workspace_bytes(const tadmm_layer_mse_desc* d, size_t* bytes);
int tadmm_layer_mse(tadmm_handle h, const tadmm_layer_mse_desc* d, void* stream);

/* G = A A^T (m<=n) or A^T A (m>n) of a row-major float32 m x n matrix, exact fp32 products
 * accumulated in fp64 on v_mfma_f64_16x16x4_f64.  G is written as double[Npad][ldg] (zero padded; see tadmm_gram_ld), N=min(m,n).
 * partial_dev: scratch of tadmm_gram_scratch_bytes(m,n). */
size_t tadmm_gram_scratch_bytes(int m, int n);
/* returns N=min(m,n); *Npad rows and *ld doubles per row of the G image */
int tadmm_gram_ld(int m, int n, int* Npad, int* ld);
int tadmm_gram_f64(tadmm_handle h, const float* A, int m, int n, double* G, int ldg,
                   void* partial_dev, size_t partial_bytes, void* stream);

/* Symmetric eigen-decomposition of double[N][N] G (row-major, symmetric PSD) by the route the plans take:
 * N <= 64 the direct solver (Householder tridiagonalisation, bisection, inverse iteration), with one-sided
 * Jacobi in one launch for whatever it does not certify; larger N the Jacobi tournament kernels.
 * evals_out: double[N] descending; evecs_out: double[N][N], row j = eigenvector j (zero where the eigenvalue
 * is at most 1e-12 of the largest).  Synchronous.  scratch: tadmm_eigh_scratch_bytes(N).
 * *sweeps_out: 0 when the direct route solved it. */
size_t tadmm_eigh_scratch_bytes(int N);
int tadmm_eigh_f64(tadmm_handle h, const double* G, int N, double* evals_out, double* evecs_out,
                   void* scratch_dev, size_t scratch_bytes, int* sweeps_out, void* stream);
/* The same solve for the leading r pairs only (1 <= r <= N, as the plans run it): evals_out double[r],
 * evecs_out double[r][N].  *route_out (nullable): 0 = direct route certified the result, 1 = single-launch
 * Jacobi (jacobi_small_kernel), 2 = Jacobi tournament (N > 64, or any N with TADMM_EIGH_TICK=1).
 * scratch: tadmm_eigh_scratch_bytes(N). */
int tadmm_eigh_partial_f64(tadmm_handle h, const double* G, int N, int r, double* evals_out, double* evecs_out,
                           void* scratch_dev, size_t scratch_bytes, int* route_out, void* stream);

/* ---- building blocks of the filtered eigen-solver (csrc/dgemm.hip, csrc/chol.hip), exposed for tests ---- */
/* C[M][N] = A[M][K] * B^T (b_transposed=1: B is [N][K]) or A * B (b_transposed=0: B is [K][N]); row-major fp64 on
 * v_mfma_f64_16x16x4_f64.  M, N multiples of 32, K multiple of 16, even leading dimensions. */
size_t tadmm_dgemm_scratch_bytes(int M, int N);
int tadmm_dgemm_f64(tadmm_handle h, const double* A, const double* B, double* C, int M, int N, int K, int lda, int ldb,
                    int ldc, int b_transposed, void* scratch, size_t scratch_bytes, void* stream);
/* C[M][N] = A[M][N] * G[N][N]^T at fp32 accuracy on the bf16 matrix cores (csrc/dgemm3.hip: the block products of the
 * filter's early stages; every value rounded to fp32 and split exactly into three bf16 terms, six MFMA products per
 * fp32 product).  M, N multiples of 32; `repeats` launches of the product (timing). */
size_t tadmm_dgemm3_scratch_bytes(int M, int N);
int tadmm_dgemm3_f64(tadmm_handle h, const double* A, const double* G, double* C, int M, int N, int lda, int ldg, int ldc,
                     int repeats, void* scratch, size_t scratch_bytes, void* stream);
/* Cholesky QR of a block stored as its transposed image YT[n][ldy] (row j = column j, `ncols` entries): on return the
 * rows are orthonormal (one pass: to ~cond^2 * 1e-16).  *bad_out_host = 1 when a pivot broke down (numerically
 * rank-deficient block; YT is then unspecified).  n multiple of 32, <= 256; ncols multiple of 64.  Synchronous. */
size_t tadmm_cholqr_scratch_bytes(int n, int ncols);
int tadmm_cholqr_f64(tadmm_handle h, double* YT, int n, int ncols, int ldy, void* scratch, size_t scratch_bytes,
                     int* bad_out_host, void* stream);
/* One grouped launch of the filter's NT tile product (dgemm_nt_tile_kernel) or of daxpby_kernel on `nprob` problems
 * exactly as the filter describes them, for tests: C = epilogue(A * B^T) with the epilogue modes, the ring of three
 * buffers addressed as (*rot + sel) % 3 (sel < 0: the explicit pointer) and the gate word of csrc/dgemm.hip.
 * (tile_m, tile_n) = (32, 32), (64, 32) or (64, 64).  M, N multiples of 32, K of 32, even leading dimensions;
 * rowpart (modes 2, 3) holds ceil(N / tile_n) * M doubles.  axpby = 1: C <- coef[0]*C + coef[1]*P over M * ldc elements
 * instead of the product.  Synchronous. */
typedef struct {
  const double* A; const double* B; double* C;
  const double* P; const double* Q;
  double* ring[3];
  const int32_t* rot;                         /* device word, nullable */
  int32_t selA, selB, selC, selP, selQ;
  int32_t M, N, K;
  int32_t lda, ldb, ldc;
  int32_t mode;                               /* 0 .. 3 */
  const double* coef;                         /* device, mode 1 and axpby */
  const double* theta;                        /* device, mode 3 */
  double* rowpart;                            /* device, modes 2 and 3 */
  const int32_t* gate; int32_t gate_min;      /* device word, nullable */
} tadmm_dgemm_tile_prob;
int tadmm_dgemm_tile_prob_bytes(void);
/* host only, no device needed: TADMM_OK, or TADMM_ERR_INVALID for arguments tadmm_dgemm_tile_f64 refuses */
int tadmm_dgemm_tile_check(int nprob, const tadmm_dgemm_tile_prob* probs, int tile_m, int tile_n, int axpby);
size_t tadmm_dgemm_tile_scratch_bytes(int nprob, const tadmm_dgemm_tile_prob* probs);
int tadmm_dgemm_tile_f64(tadmm_handle h, int nprob, const tadmm_dgemm_tile_prob* probs, int tile_m, int tile_n, int axpby,
                         void* scratch, size_t scratch_bytes, void* stream);
/* Host only, no device needed: the block map that the filter and tadmm_dgemm_tile_f64 give one grouped launch of the tile
 * product on `nprob` problems C[M][N] = A[M][K] * B[N][K]^T in tile_m x tile_n tiles.  Position i of the map is
 * (prob, local) = (map_out[2i], map_out[2i + 1]) with local = tm * ceil(N / tile_n) + tn, and is expected on XCD i % 8:
 * a permutation of the problem-major order that keeps the tiles of one slot on few operand panels (csrc/host.h).
 * Returns the number of blocks (map_out and cost_out both NULL: only that), TADMM_ERR_WORKSPACE when `capacity`
 * (entries) is smaller, TADMM_ERR_INVALID for non-positive sizes.  cost_out[0] is the modelled operand traffic of the
 * map in bytes, cost_out[1] that of the problem-major order.  Honours TADMM_XCD_MAP / TADMM_TILE_MAP like the plans. */
typedef struct { int32_t M, N, K, tile_m, tile_n; } tadmm_tile_map_prob;
int64_t tadmm_tile_map(int nprob, const tadmm_tile_map_prob* probs, int32_t* map_out, int64_t capacity, double* cost_out);

#ifdef __cplusplus
}
#endif
#endif /* TADMM_H_ */
