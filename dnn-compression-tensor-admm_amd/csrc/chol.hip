// Cholesky QR of a tall block on the fp64 matrix cores: the orthonormalisation step of the filtered
// eigen-solver (filter.hip).  Given the Gram matrix C = Y^T Y (n x n, n <= 256) of a block image
// YT[n][ldy] (row j = column j of Y):
//
//   chol_factor : C = R^T R.  One 512-thread workgroup per problem keeps all upper 16x16 tiles of C in
//                 registers (MFMA accumulator layout) and runs the right-looking block algorithm
//                    W_k = R_kk^{-T}  (16x16 Cholesky + triangular inverse, one wave, in LDS)
//                    R_kj = W_k C_kj                      (panel, one MFMA tile product each)
//                    C_ij -= R_ki^T R_kj   (k < i <= j)   (trailing update, operands from the LDS panel)
//                 Only the pivot chain W_k -> R_k,k+1 -> C_k+1,k+1 -> W_k+1 is serial: one wave owns both tiles of
//                 it and hands the diagonal tile on; the rest of the panel and the trailing update run beside it.
//                 A non-positive pivot (numerically rank deficient block) sets the problem's `bad` word.
//   chol_solve  : Q^T = R^{-T} Y^T in place, by right-looking block forward substitution.  A workgroup owns one
//                 strip of 16 columns of the image, its waves share the strip's 16x16 tiles; the solved tile
//                    X_j = W_j (Y_j - sum_{i<j} R_i,j^T X_i)
//                 is handed to them through LDS (the D layout of one product is the B-operand layout of the next)
//                 and each applies it to its own tiles kb > j.
// Used twice in a row ("CholQR2") the result is orthonormal to rounding for condition numbers up to ~1e7.
#include "common.h"

namespace tadmm {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int kCT = 16;            // tile edge
constexpr int kCLd = kCT + 1;      // padded leading dimension of the LDS tiles
constexpr int kCMaxT = 16;         // n <= 256

__device__ __forceinline__ double rsqrt_f64(double x) {
  double y = __builtin_amdgcn_rsq(x);                    // ~2^-26 relative
  y = y * (1.5 - 0.5 * x * y * y);
  y = y * (1.5 - 0.5 * x * y * y);                       // (second step kept: 16 pivots in a row feed one another)
  return y;
}

// W = L^-1 for the 16x16 SPD tile Dg = L L^T, one wave, blocked by 4 so that every rank-4 update is ONE
// v_mfma_f64_16x16x4 on a register-resident tile:
//   S (accumulator layout) starts as Dg; for block b: the 4x4 block S_bb is factored and inverted redundantly by
//   every lane (M = L_bb^-1, four dependent rsqrt), the block column P = S[:, b] M^T gives columns 4b..4b+3 of L,
//   and S -= P P^T eliminates them.  The inverse is carried along: R starts as I, X_b = M R[b, :] are rows 4b..4b+3 of
//   W, and R -= L[:, b] X_b -- again one MFMA, whose operands (P of this lane, X of this lane) are already in place.
// Returns false (uniformly) on a pivot <= tiny.
__device__ __forceinline__ bool diag_inverse(const double (*Dg)[kCLd], double (*Cb)[5], double (*Wt)[kCLd],
                                             double* __restrict__ Wg, int lane, double tiny) {
  const int r = lane & 15, q = lane >> 4;
  double4_t S, R;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    S[e] = Dg[q + 4 * e][r];
    R[e] = (q + 4 * e == r) ? 1.0 : 0.0;
  }
  bool ok = true;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    // block column 4b..4b+3 of S -> LDS (lanes whose column r lies in the block hold it, rows q + 4e)
    if ((r >> 2) == b) {
#pragma unroll
      for (int e = 0; e < 4; ++e) Cb[q + 4 * e][r & 3] = S[e];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const double s00 = Cb[4 * b][0], s10 = Cb[4 * b + 1][0], s20 = Cb[4 * b + 2][0], s30 = Cb[4 * b + 3][0];
    const double s11 = Cb[4 * b + 1][1], s21 = Cb[4 * b + 2][1], s31 = Cb[4 * b + 3][1];
    const double s22 = Cb[4 * b + 2][2], s32 = Cb[4 * b + 3][2], s33 = Cb[4 * b + 3][3];
    const double c0 = Cb[r][0], c1 = Cb[r][1], c2 = Cb[r][2], c3 = Cb[r][3];
    ok = ok && (s00 > tiny);
    const double i0 = rsqrt_f64(fmax(s00, tiny));
    const double l10 = s10 * i0, l20 = s20 * i0, l30 = s30 * i0;
    const double t11 = s11 - l10 * l10;
    ok = ok && (t11 > tiny);
    const double i1 = rsqrt_f64(fmax(t11, tiny));
    const double l21 = (s21 - l20 * l10) * i1, l31 = (s31 - l30 * l10) * i1;
    const double t22 = s22 - l20 * l20 - l21 * l21;
    ok = ok && (t22 > tiny);
    const double i2 = rsqrt_f64(fmax(t22, tiny));
    const double l32 = (s32 - l30 * l20 - l31 * l21) * i2;
    const double t33 = s33 - l30 * l30 - l31 * l31 - l32 * l32;
    ok = ok && (t33 > tiny);
    const double i3 = rsqrt_f64(fmax(t33, tiny));
    // M = L_bb^-1 (lower)
    const double m00 = i0, m11 = i1, m22 = i2, m33 = i3;
    const double m10 = -l10 * m00 * i1;
    const double m20 = -(l20 * m00 + l21 * m10) * i2, m21 = -l21 * m11 * i2;
    const double m30 = -(l30 * m00 + l31 * m10 + l32 * m20) * i3, m31 = -(l31 * m11 + l32 * m21) * i3, m32 = -l32 * m22 * i3;
    // P[r][q] = sum_{m <= q} S[r][4b+m] M[q][m]   (zero above the block: those rows are eliminated already)
    const double p0 = c0 * m00, p1 = c0 * m10 + c1 * m11, p2 = c0 * m20 + c1 * m21 + c2 * m22,
                 p3 = c0 * m30 + c1 * m31 + c2 * m32 + c3 * m33;
    double P = q == 0 ? p0 : (q == 1 ? p1 : (q == 2 ? p2 : p3));
    if (r < 4 * b) P = 0.0;
    S = __builtin_amdgcn_mfma_f64_16x16x4f64(-P, P, S, 0, 0, 0);
    // rows 4b..4b+3 of W: X[4b+q][r] = sum_m M[q][m] R[4b+m][r]; R[4b+m][r] is register b of lane (r, m)
    // (rows 4b..4b+3 of R are exchanged through the rows of Wt they are about to define)
    Wt[4 * b + q][r] = R[b];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const double r0 = Wt[4 * b][r], r1 = Wt[4 * b + 1][r], r2 = Wt[4 * b + 2][r], r3 = Wt[4 * b + 3][r];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const double x0 = m00 * r0, x1 = m10 * r0 + m11 * r1, x2 = m20 * r0 + m21 * r1 + m22 * r2,
                 x3 = m30 * r0 + m31 * r1 + m32 * r2 + m33 * r3;
    const double X = q == 0 ? x0 : (q == 1 ? x1 : (q == 2 ? x2 : x3));
    Wt[4 * b + q][r] = X;
    Wg[(4 * b + q) * kCT + r] = X;
    R = __builtin_amdgcn_mfma_f64_16x16x4f64(-P, X, R, 0, 0, 0);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  return ok;
}

#ifdef TADMM_CHOL_STAMPS
__device__ long long g_cstamps[128];
#define CSTAMP(i) do { if (blockIdx.x == 0 && lane == 0) g_cstamps[i] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define CSTAMP(i) do { } while (0)
#endif

// Barrier that orders LDS traffic only.  __syncthreads() also waits for the wave's outstanding GLOBAL stores (vmcnt(0));
// the factor rows and inverse tiles this kernel writes to memory are never read back by it, and waiting for their
// write acknowledgements at three barriers per step cost ~3 k cycles of every 12 k-cycle step (scripts/stamp_chol.sh).
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Wave 0 owns no tiles: it only inverts diagonal tiles; the other seven waves hold the upper tiles of C.
//
// Schedule.  Once W_k exists, only tile (k,k+1) -- R_k,k+1 = W_k C_k,k+1 -- and the update C_k+1,k+1 -= R_k,k+1^T R_k,k+1
// stand between it and the inversion of the next diagonal tile.  Both tiles of such a PAIR (k,k+1), (k+1,k+1) belong to
// the same wave, which does the two products back to back (the D layout of the first is both operand layouts of the
// second: no LDS round trip) and hands the diagonal tile over.  The rest of row panel k belongs to the OTHER six tile
// waves, which form it beside the pair wave; the trailing update runs behind the hand-over, beside diag_inverse(k+1):
//
//     wave 0                                   tile waves
//     A_k   tile (k,k) is in Dg, panel k-1 is complete in Pn
//     diag_inverse(k)                          trailing update k-1 of every tile but (k,k)
//     B_k   W_k is in Wt, `fail` is final, trailing update k-1 is complete
//     (waits at A_k+1)                         pair wave: R_k,k+1 -> Pn, R;  update of (k+1,k+1) -> Dg
//                                              the others: R_k,j = W_k C_k,j, j > k + 1  -> Pn, R
//
// Barrier discipline: every wave of the workgroup executes the barriers A_0 B_0 A_1 B_1 ... in this order and nothing
// else; the early returns in front of them (gate, bad) are uniform over the workgroup.  `fail` is written only by wave 0
// in front of B_k and read by every wave only behind B_k, and a wave that reads it set leaves at once: on breakdown in
// step k every wave has executed exactly 2k + 2 barriers, otherwise exactly 2 nbt.
constexpr int kCTileWaves = 7;
constexpr int kCSlots7 = 20;            // the most tiles a wave gets (n = 256); checked by chol_slots_fit below

// Where tile (i,j) != (0,0) of an nbt x nbt upper triangle lives: wave in the low byte, slot above it.  Column j's
// diagonal tile and the one above it are a pair: wave j mod 7, slots 2p and 2p + 1 with p = (j - 1) / 7.  The other
// tiles of row i (j >= i + 2) go round the six waves that do NOT own the pair (i,i+1), (i+1,i+1) -- wave (i+1) mod 7 is
// busy with the pivot chain while row i's panel is formed -- continuing where the row before stopped, into the slots
// behind the wave's pairs in row order.  Tile (0,0) needs no slot: it goes to the diagonal wave as it is.
__host__ __device__ constexpr int chol_rest_base(int i, int nbt) { return i * (nbt - 2) - (i * (i - 1)) / 2; }   // panel tiles in rows < i
__host__ __device__ constexpr int chol_slot_of(int i, int j, int nbt) {
  const int rem = j - i;
  if (rem <= 1) return ((2 * ((j - 1) / kCTileWaves) + rem) << 8) | (j % kCTileWaves);
  const int p = rem - 2;
  const int w = (i + 2 + (p + chol_rest_base(i, nbt)) % 6) % kCTileWaves;
  int cnt = 2 * (w > 0 ? (nbt - 1 - w + kCTileWaves) / kCTileWaves : (nbt - 1) / kCTileWaves);   // the wave's pair slots
  for (int ii = 0; ii < i; ++ii) {      // + its panel tiles of the rows above
    const int len = nbt - ii - 2, o = (w - (ii + 2) % kCTileWaves + kCTileWaves) % kCTileWaves;
    if (o < 6) {
      const int p0 = ((o - chol_rest_base(ii, nbt)) % 6 + 6) % 6;
      if (len > p0) cnt += (len - p0 + 5) / 6;
    }
  }
  return ((cnt + p / 6) << 8) | w;
}
constexpr bool chol_slots_fit() {
  for (int nbt = 1; nbt <= kCMaxT; ++nbt)
    for (int i = 0; i < nbt; ++i)
      for (int j = i; j < nbt; ++j)
        if (j > 0 && (chol_slot_of(i, j, nbt) >> 8) >= kCSlots7) return false;
  return true;
}
static_assert(chol_slots_fit(), "kCSlots7 too small");

__global__ __launch_bounds__(512) void chol_factor_kernel(const CholDesc* __restrict__ descs) {
  __shared__ double Dg[kCT][kCLd];
  __shared__ double Wt[kCT][kCLd];
  __shared__ double Cb[kCT][5];        // current 16x4 block column of the diagonal tile's Schur complement
  __shared__ double Pn[kCMaxT][kCT][kCLd];
  __shared__ double red[8];
  // tile (i,j) of wave w, slot s as (j << 8) | i (chol_slot_of); 0 = empty
  __shared__ unsigned short tab[kCTileWaves][kCSlots7];
  __shared__ int fail;
  const CholDesc d = descs[blockIdx.x];
  if (d.gate && *d.gate < d.gate_min) return;
  if (*d.bad) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // scalar: the per-slot tests below become branches
  const int r = lane & 15, q = lane >> 4;
  const int nbt = d.n / kCT;
  const int ntile = nbt * (nbt + 1) / 2;
  for (int t = tid; t < kCTileWaves * kCSlots7; t += 512) (&tab[0][0])[t] = 0;
  if (tid == 0) fail = 0;
  double scale = 0.0;                   // largest diagonal entry of C: pivots are judged relative to it
  for (int i = tid; i < d.n; i += 512) scale = fmax(scale, d.C[(int64_t)i * d.ldc + i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) scale = fmax(scale, __shfl_xor(scale, o, 64));
  if (lane == 0) red[wave] = scale;
  __syncthreads();
  for (int t = tid; t < ntile; t += 512) {
    int i = 0, rem = t, rowlen = nbt;
    while (rem >= rowlen) { rem -= rowlen; ++i; --rowlen; }
    const int j = i + rem;
    if (j > 0) {
      const int ws = chol_slot_of(i, j, nbt);
      tab[ws & 0xff][ws >> 8] = (unsigned short)((j << 8) | i);
    }
  }
  scale = 0.0;
#pragma unroll
  for (int w = 0; w < 8; ++w) scale = fmax(scale, red[w]);
  const double tiny = scale * 1e-15;    // a pivot this small relative to the largest norm: numerically rank deficient
  __syncthreads();

  if (wave == 0) {
    // ---------------- diagonal wave ----------------
    for (int k = 0; k < nbt; ++k) {
      lds_barrier();                                               // A_k: tile (k,k) is in Dg
      CSTAMP(3 * k);
      if (!diag_inverse(Dg, Cb, Wt, d.Wd + (int64_t)k * (kCT * kCT), lane, tiny) && lane == 0) fail = 1;
      CSTAMP(3 * k + 1);
      lds_barrier();                                               // B_k: W_k is in Wt (and trailing k-1 is complete)
      CSTAMP(3 * k + 2);
      if (fail) { if (tid == 0) *d.bad = 1; return; }
    }
    return;
  }
  // ---------------- tile waves ----------------
  const int tw = wave - 1;
  double4_t acc[kCSlots7];
  // tile coordinates of this wave's slots, read from the LDS table ONCE (packed, one vector register per slot): looked
  // up per slot and step -- two dependent LDS reads in front of every branch -- they cost the panel phase ~3 k cycles of
  // a 12 k-cycle step.  Whether a slot takes part in a phase is scalar arithmetic on its coordinates.
  int sij[kCSlots7];
  auto row_of = [](int v) { return v & 0xff; };
  auto col_of = [](int v) { return v >> 8; };
  // the LDS addresses derived from a slot's coordinates are loop invariant; hoisted out of the step loop for all slots
  // they would cost 40 vector registers and spill.  The empty volatile asm makes the compiler rebuild them where used.
  auto fresh = [](int v) { v = __builtin_amdgcn_readfirstlane(v); asm volatile("" : "+s"(v)); return v; };
#pragma unroll
  for (int s = 0; s < kCSlots7; ++s) {
    acc[s] = double4_t{0, 0, 0, 0};
    sij[s] = tab[tw][s];
    if (sij[s] != 0) {
      const int i = row_of(sij[s]), j = col_of(sij[s]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[s][e] = d.C[(int64_t)(kCT * i + q + 4 * e) * d.ldc + kCT * j + r];
    }
  }
  // trailing update of ONE slot with the panel of step k (tile (i,j), i > k)
  auto trail = [&](double4_t& a, int i, int j) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      a = __builtin_amdgcn_mfma_f64_16x16x4f64(-Pn[i][q + 4 * e][r], Pn[j][q + 4 * e][r], a, 0, 0, 0);
  };
  // R_k,pj = W_k C_k,pj in place, to the LDS panel and to the factor
  auto panel = [&](double4_t& a, const double (&wa)[4], int k, int pj) {
    double4_t o = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) o = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[e], a[e], o, 0, 0, 0);
    a = o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      Pn[pj][q + 4 * e][r] = o[e];
      d.R[(int64_t)(kCT * k + q + 4 * e) * d.ldr + kCT * pj + r] = o[e];
    }
  };
  if (tw == 0) {                            // tile (0,0) goes to the diagonal wave as it is
#pragma unroll
    for (int e = 0; e < 4; ++e) Dg[q + 4 * e][r] = d.C[(int64_t)(q + 4 * e) * d.ldc + r];
  }
  for (int k = 0; k < nbt; ++k) {
    lds_barrier();                                                 // A_k
    // ---- trailing update of step k-1 for everything but tile (k,k), which was updated before it was handed over ----
    if (k > 0) {
#pragma unroll
      for (int s = 0; s < kCSlots7; ++s) {
        const int c = fresh(sij[s]);
        if (row_of(c) >= k && c != ((k << 8) | k)) trail(acc[s], row_of(c), col_of(c));
        __builtin_amdgcn_sched_barrier(0);     // keep the operand loads of one slot from being hoisted over the others
      }
    }
    if (wave == 1) CSTAMP(64 + 2 * k);
    lds_barrier();                                                 // B_k
    if (fail) return;
    double wa[4];                           // W_k as the A operand of the panel products
#pragma unroll
    for (int e = 0; e < 4; ++e) wa[e] = Wt[r][q + 4 * e];
    if (k + 1 < nbt && tw == (k + 1) % kCTileWaves) {
      // ---- the pivot chain: R_k,k+1, then tile (k+1,k+1) brought up to date from registers and handed over ----
#pragma unroll
      for (int p = 0; p < (kCMaxT + kCTileWaves - 2) / kCTileWaves; ++p)
        if (k / kCTileWaves == p) {
          panel(acc[2 * p + 1], wa, k, k + 1);
          const double4_t o = acc[2 * p + 1];      // o[e] = R_k,k+1[q + 4e][r]: the A and the B operand of its own square
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[2 * p] = __builtin_amdgcn_mfma_f64_16x16x4f64(-o[e], o[e], acc[2 * p], 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e) Dg[q + 4 * e][r] = acc[2 * p][e];
        }
      CSTAMP(65 + 2 * k);
    }
    // ---- the rest of panel k: R_k,j = W C_k,j, j > k + 1 (none of these tiles belongs to the pair wave) ----
#pragma unroll
    for (int s = 0; s < kCSlots7; ++s) {
      const int c = fresh(sij[s]);
      if (row_of(c) == k && col_of(c) > k + 1) panel(acc[s], wa, k, col_of(c));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

void launch_chol_factor(const CholDesc* descs_dev, int nprob, hipStream_t s) {
  if (nprob <= 0) return;
#ifdef TADMM_CHOL_STAMPS
  if (getenv("TADMM_CHOL_STAMPS_DUMP")) {
    long long h[128];
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_cstamps), sizeof h);
    fprintf(stderr, "[chol stamps] step: diag | wait B | B_k to A_k+1 | (first tile wave: trail done after A_k; pair wave: hand-over after B_k)\n");
    for (int k = 0; k < 16 && h[3 * k + 2]; ++k)
      fprintf(stderr, "  k=%2d A_k@%6lld  diag %5lld  toB %5lld  toA %5lld   trail@%5lld pair@%5lld\n", k, h[3 * k] - h[0], h[3 * k + 1] - h[3 * k],
              h[3 * k + 2] - h[3 * k + 1], h[3 * k + 3] ? h[3 * k + 3] - h[3 * k + 2] : 0, h[64 + 2 * k] - h[3 * k],
              h[65 + 2 * k] ? h[65 + 2 * k] - h[3 * k + 2] : 0);
  }
#endif
  hipLaunchKernelGGL(chol_factor_kernel, dim3(nprob), dim3(512), 0, s, descs_dev);
}

// Block forward substitution, right-looking: a workgroup owns ONE strip of kCholStrip = 16 columns of the image, i.e.
// n/16 tiles of 16x16, and wave w keeps the tiles kb = w (mod kCSolveWaves) of it in accumulator layout.  Step j:
//   the owner of tile j forms X_j = W_j tile_j, stores it to the image and publishes -X_j in LDS (the D layout of that
//   product IS the B-operand layout of the updates); after ONE workgroup barrier every wave applies
//   tile_kb -= R_j,kb^T X_j to its own tiles kb > j.  The owner of tile j+1 updates that tile first and forms X_j+1 at
//   once, so the serial path of a step is eight dependent MFMAs and one LDS hand-off; the other updates of the step run
//   beside it on the other waves.  R is complete before the launch: every wave reads ITS R_j,kb tiles straight from L2,
//   one step ahead.  Each tile sums its updates in a fixed order (even and odd j apart, each ascending, no atomics):
//   bitwise reproducible.
// Barriers: the gate / bad / strip tests are uniform over the workgroup and precede the first barrier; after them every
// wave executes exactly nbt - 1 barriers (one per step, under a test on the step number alone).  X_j+1 goes to the
// other half of Xs, whose last readers (step j-1) have all passed barrier j before the owner of tile j+1 -- who also
// waited there -- writes it.
constexpr int kCSolveWaves = 4;
constexpr int kCSolveSlots = kCMaxT / kCSolveWaves;

__global__ __launch_bounds__(64 * kCSolveWaves) void chol_solve_kernel(const CholDesc* __restrict__ descs,
                                                                       const BlockRef* __restrict__ map) {
  __shared__ double Xs[2][kCT][kCLd];
  const BlockRef br = map[blockIdx.x];
  const CholDesc d = descs[br.prob];
  if (d.gate && *d.gate < d.gate_min) return;
  if (*d.bad) return;
  if (br.local * kCholStrip >= d.ncols) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // scalar: the per-slot tests below become branches
  const int r = lane & 15, q = lane >> 4;
  const int nbt = d.n / kCT;
  int ring = d.rot ? *d.rot + d.sel : d.sel;
  ring -= (ring >= 3) ? 3 : 0;
  ring -= (ring >= 3) ? 3 : 0;
  if (d.rot_out && br.local == 0 && tid == 0) *d.rot_out = ring;
  G<double>* __restrict__ Y = gp(ring == 0 ? d.ring[0] : (ring == 1 ? d.ring[1] : d.ring[2])) + br.local * kCholStrip + r;
  const G<const double>* __restrict__ R = gp((const double*)d.R);
  const G<const double>* __restrict__ Wd = gp((const double*)d.Wd);
  const int64_t ldy = d.ldy, ldr = d.ldr;

  // tile kb = kCSolveWaves * s + wave, rows q + 4e, column r, as two sums: Te = Y_kb - (updates of even steps j), To =
  // - (updates of odd steps), added when the tile is solved.  Two chains per tile is the summation order this kernel has
  // always had (a single chain of dependent MFMAs was the latency floor of the one-wave version); keeping it keeps the
  // results of every plan bit for bit.
  double4_t Te[kCSolveSlots], To[kCSolveSlots];
  double4_t Ra[kCSolveSlots], Rb[kCSolveSlots];   // R_j,kb of even / odd steps j, A operand: A[m = r][k = q] of MFMA e is R[16j + q + 4e][16kb + r]
  double4_t Wn;                     // W of this wave's next own tile, A[m = r][k = q] of MFMA e is W[r][q + 4e]
  auto fetch_r = [&](double4_t& a, int j, int kb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = R[(int64_t)(kCT * j + q + 4 * e) * ldr + kCT * kb + r];
  };
  auto fetch_w = [&](int kb) {
    if (kb < nbt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) Wn[e] = Wd[(int64_t)kb * (kCT * kCT) + r * kCT + q + 4 * e];
    }
  };
  // t -= R^T X; LDS holds -X, so that nothing has to be negated between a load of R and its use
  auto update = [&](double4_t& t, const double4_t& a, const double4_t& xneg) {
#pragma unroll
    for (int e = 0; e < 4; ++e) t = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], xneg[e], t, 0, 0, 0);
  };
  // X_kb = W_kb tile_kb: to the image, and (negated) to LDS for the updates of every wave
  auto finish = [&](const double4_t& t, int kb) {
    double4_t o = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) o = __builtin_amdgcn_mfma_f64_16x16x4f64(Wn[e], t[e], o, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) Xs[kb & 1][q + 4 * e][r] = -o[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) Y[(int64_t)(kCT * kb + q + 4 * e) * ldy] = o[e];
    fetch_w(kb + kCSolveWaves);
  };
  // step j, once -X_j is published: `cur` holds this wave's R_j,kb, `nxt` receives R_j+1,kb (tiles kb > j + 1) for the coming step
  auto step = [&](int j, double4_t (&T)[kCSolveSlots], double4_t (&cur)[kCSolveSlots], double4_t (&nxt)[kCSolveSlots]) {
    if (j + 1 >= nbt) return;                                      // uniform over the workgroup
    lds_barrier();                                                 // -X_j is in Xs[j & 1]
    double4_t x;
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = Xs[j & 1][q + 4 * e][r];
    // the owner of tile j + 1 brings it up to date and solves it before anything else: the next step waits for that
#pragma unroll
    for (int s = 0; s < kCSolveSlots; ++s)
      if (kCSolveWaves * s + wave == j + 1) {
        update(T[s], cur[s], x);
        finish(Te[s] + To[s], j + 1);
      }
#pragma unroll
    for (int s = 0; s < kCSolveSlots; ++s) {
      const int kb = kCSolveWaves * s + wave;
      if (kb > j + 1 && kb < nbt) update(T[s], cur[s], x);
      __builtin_amdgcn_sched_barrier(0);       // keep one slot's operand waits from being hoisted over the others
    }
    // Loads return in order: issued in front of the updates, the wait for `cur` in the first MFMA would also wait for
    // these.  Behind them they are in flight while the wave stands at the next barrier.
#pragma unroll
    for (int s = 0; s < kCSolveSlots; ++s) {
      const int kb = kCSolveWaves * s + wave;
      if (kb > j + 1 && kb < nbt) fetch_r(nxt[s], j + 1, kb);
    }
  };

  Wn = double4_t{0, 0, 0, 0};
  fetch_w(wave);
#pragma unroll
  for (int s = 0; s < kCSolveSlots; ++s) {
    const int kb = kCSolveWaves * s + wave;
    Te[s] = To[s] = Ra[s] = Rb[s] = double4_t{0, 0, 0, 0};
    if (kb < nbt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) Te[s][e] = Y[(int64_t)(kCT * kb + q + 4 * e) * ldy];
      if (kb > 0) fetch_r(Ra[s], 0, kb);
    }
  }
  if (wave == 0) finish(Te[0], 0);
  for (int j = 0; j + 1 < nbt; j += 2) {
    step(j, Te, Ra, Rb);
    step(j + 1, To, Rb, Ra);
  }
}

void launch_chol_solve(const CholDesc* descs_dev, const BlockRef* map_dev, int nblocks, hipStream_t s) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(chol_solve_kernel, dim3(nblocks), dim3(64 * kCSolveWaves), 0, s, descs_dev, map_dev);
}

}  // namespace tadmm
