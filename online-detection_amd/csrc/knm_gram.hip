// The M x M sufficient statistics of an incremental FALKON model (odx/incremental.py) and the product the CG takes with them.
//   odx_knm_gram_f64 : G = beta G + K' diag(w) K and b = beta b + K' (w o y) from an f32 K_nM block (or a row sub-block), every
//                      product and sum f64 on v_mfma_f64_16x16x4_f64.  rls_gram_rows32_kernel's shape (rls.hip): k-tiles of 32
//                      ROWS staged as [k][column], 128 x 64 lower tiles, three workgroups per CU, the skinny products on the
//                      vector ALU in the first tile column — with contiguous rows, the row weight folded into the B operand on
//                      its way into LDS (which therefore holds doubles), a read-modify-write epilogue and a mirrored store.
//   odx_knm_gram_rhsn_f64 : the same G, and B[t] = beta B[t] + K' (w o Y[:, t]) for nt label columns from the same read: the
//                      right-hand sides are further tile columns of the launch, 64 label columns wide, whose B operand is
//                      w o Y[k-tile, t0 : t0 + 64] (doubles already) and whose 128 x 64 accumulators are stored transposed.
//   odx_symvn_f64    : Y[q] = alpha G X[q] for up to 8 vectors from one read of the full matrix (trmvn_f64_kernel's rows, loads
//                      and reduction over the whole row).
// Neither uses scratch or atomics: one workgroup (one wave) owns an output tile (a row block) and sums in one fixed order.
#include "odx_internal.h"

namespace odx {

typedef double f64x2g __attribute__((ext_vector_type(2)));
typedef double f64x4g __attribute__((ext_vector_type(4)));
typedef float f32x2g __attribute__((ext_vector_type(2)));

constexpr int KG_BM = 128, KG_BN = 64, KG_BK = 32;
constexpr int KG_LDA = KG_BM + 16;      // floats per LDS row of the A side: the four k-rows of a 64-lane ds_read_b32 on four bank quarters
constexpr int KG_LDB = KG_BN + 16;      // DOUBLES per LDS row of the B side: 160 dwords, so the two k-rows a 32-lane half of a
                                        // ds_read_b64 touches (16 doubles = 32 banks each) fall on the two halves of the 64 banks

// Two neighbouring columns col, col + 1 of a row (col even: 8-byte aligned).  mode 2: both are columns of the block; 1: only the
// first (M odd, the last column); 0: neither.  A column >= M is never read.
__device__ __forceinline__ f32x2g kg_load2(const float* __restrict__ x, int col, int mode) {
  if (mode == 2) return *reinterpret_cast<const f32x2g*>(x + col);
  f32x2g v = {0.f, 0.f};
  if (mode == 1) v[0] = x[col];
  return v;
}

// One output tile.  HALF: the tile right of the diagonal's first half (columns i0 + 64 .. against rows i0 ..): its upper 64 rows
// lie strictly above the diagonal, so the four waves share the LOWER 64 x 64 block, 32 x 32 each, and issue half the matrix
// instructions; every other tile's waves own 64 x 32 outputs each.  XTY: the tile also forms its 128 entries of b (the tiles of
// the first tile column when y is given).  Both are template arguments so that the k loop holds no branch.
// RHS (knm_gram_rhsn_kernel; neither HALF nor XTY): the tile is 128 columns of K against 64 label columns, j0 the first of them.
// y is then the (n, nt) row-major label matrix, ldy doubles a row; the B operand is w o Y[k-tile, j0 : j0 + 64], zero past column
// nt; the accumulators (K column i0 + i, label column j0 + t) go to bout[(j0 + t) * ldb + i0 + i], transposed through LDS as the
// mirror store is, with beta applied from bout.  G is not touched.
template <bool HALF, bool XTY, bool RHS = false>
__device__ __forceinline__ void knm_gram_tile(const float* __restrict__ K, int64_t ldk, int64_t n, int M, const double* __restrict__ w,
                                              const double* __restrict__ y, double beta, double* G, int64_t ldg, double* bout, int i0,
                                              int j0, float* lds_a, double* lds_b, double* lds_wy, int64_t ldy = 0, int nt = 0,
                                              int64_t ldb = 0) {
  constexpr bool half = HALF, xty = XTY, rhs = RHS;
  static_assert(!(RHS && (HALF || XTY)), "a right-hand-side tile is a full tile without the skinny product");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int arow = half ? 64 + wr * 32 : wr * 64;
  const int krow = tid >> 4, seg = tid & 15;                  // this thread stages k-rows krow and krow + 16 of a k-tile
  int ca[4], cb[2], ma[4], mb[2];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    ca[q] = i0 + q * 32 + seg * 2;
    ma[q] = ca[q] + 1 < M ? 2 : (ca[q] < M ? 1 : 0);
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    cb[q] = j0 + q * 32 + seg * 2;
    const int nb = rhs ? nt : M;                              // (the B side's columns: label columns in a right-hand-side tile)
    mb[q] = cb[q] + 1 < nb ? 2 : (cb[q] < nb ? 1 : 0);
  }
  // RHS: the label columns this thread loads, clamped to nt - 1, so that the k loop loads without a branch and never reads a
  // column >= nt; what a clamped load brings is dropped on the way into LDS (mb)
  int cy[2][2] = {{0, 0}, {0, 0}};
  if constexpr (rhs) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      cy[q][0] = cb[q] < nt ? cb[q] : nt - 1;
      cy[q][1] = cb[q] + 1 < nt ? cb[q] + 1 : nt - 1;
    }
  }
  int aoff[4];                                                // (a half tile has two row blocks: it reads them twice, in bounds)
#pragma unroll
  for (int t = 0; t < 4; ++t) aoff[t] = arow + (half ? (t & 1) : t) * 16 + (lane & 15);
  f64x4g acc[4][2];
#pragma unroll
  for (int tm = 0; tm < 4; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = f64x4g{0.0, 0.0, 0.0, 0.0};
  const int64_t nk = n > 0 ? (n + KG_BK - 1) / KG_BK : 0;
  f32x2g ra[2][4], rb[2][2];
  f64x2g rbd[2][2];                                           // (RHS: the B side's entries, doubles)
  double rw[2] = {1.0, 1.0}, ry[2] = {0.0, 0.0};
  bool valid[2] = {false, false};
  // the rows of k-tile kt this thread stages, into registers: a row past n is not read (its place takes row n - 1's values, which
  // the store into LDS replaces by zeros)
  auto load = [&](int64_t kt, int h) {
    const int64_t row = kt * KG_BK + krow + 16 * h;
    valid[h] = row < n;
    const int64_t r = valid[h] ? row : n - 1;
    const float* x = K + r * ldk;
#pragma unroll
    for (int q = 0; q < 4; ++q) ra[h][q] = kg_load2(x, ca[q], ma[q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if constexpr (rhs) {
        const double* yr = y + r * ldy;
        rbd[h][q] = f64x2g{yr[cy[q][0]], yr[cy[q][1]]};
      } else {
        rb[h][q] = kg_load2(x, cb[q], mb[q]);
      }
    }
    if (w != nullptr) rw[h] = w[r];
    if (xty) ry[h] = y[r];
  };
  double ysum = 0.0;
  const int ycol = tid & 127, yhalf = tid >> 7;               // b: column ycol of the A side, two k-rows of every step
  const int r16 = lane & 15, kq = lane >> 4;
  if (nk > 0) {
    load(0, 0);
    load(0, 1);
  }
  for (int64_t kt = 0; kt < nk; ++kt) {
    __syncthreads();                                           // everyone finished reading the previous k-tile
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float* da = lds_a + (krow + 16 * h) * KG_LDA + seg * 2;
      double* db = lds_b + (krow + 16 * h) * KG_LDB + seg * 2;
      const bool ok = valid[h];                                // (selected, not multiplied by 0)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f32x2g*>(da + q * 32) = f32x2g{ok ? ra[h][q][0] : 0.f, ok ? ra[h][q][1] : 0.f};
      // the row weight, once per entry of the B operand: w K in f64 (one rounding; w = 1 changes no bit)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if constexpr (rhs)                                     // w y, rounded once as an XTY tile rounds it
          *reinterpret_cast<f64x2g*>(db + q * 32) =
              f64x2g{ok && mb[q] >= 1 ? rw[h] * rbd[h][q][0] : 0.0, ok && mb[q] == 2 ? rw[h] * rbd[h][q][1] : 0.0};
        else
          *reinterpret_cast<f64x2g*>(db + q * 32) = f64x2g{ok ? rw[h] * (double)rb[h][q][0] : 0.0, ok ? rw[h] * (double)rb[h][q][1] : 0.0};
      }
      if (xty && seg == 0) lds_wy[krow + 16 * h] = ok ? rw[h] * ry[h] : 0.0;
    }
    __syncthreads();
    load(kt + 1, 0);                                           // (past the last k-tile: row n - 1 again, dropped)
    load(kt + 1, 1);
    __builtin_amdgcn_sched_barrier(0);                         // (the loads stay in front of the MFMAs they hide under)
    float a[2][4];
    double b[2][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) a[0][t] = lds_a[kq * KG_LDA + aoff[t]];
#pragma unroll
    for (int t = 0; t < 2; ++t) b[0][t] = lds_b[kq * KG_LDB + wc * 32 + t * 16 + r16];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int cur = ks & 1, nxt = cur ^ 1;
      if (ks < 7) {
#pragma unroll
        for (int t = 0; t < 4; ++t) a[nxt][t] = lds_a[((ks + 1) * 4 + kq) * KG_LDA + aoff[t]];
#pragma unroll
        for (int t = 0; t < 2; ++t) b[nxt][t] = lds_b[((ks + 1) * 4 + kq) * KG_LDB + wc * 32 + t * 16 + r16];
        __builtin_amdgcn_sched_barrier(0);                     // (reads first: the scheduler sinks them below the multiplies otherwise)
      }
      double ad[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) ad[t] = (double)a[cur][t];
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[tm], b[cur][tn], acc[tm][tn], 0, 0, 0);
      if constexpr (!half) {
#pragma unroll
        for (int tm = 2; tm < 4; ++tm)
#pragma unroll
          for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[tm], b[cur][tn], acc[tm][tn], 0, 0, 0);
      }
      if constexpr (xty) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int kr = ks * 4 + yhalf * 2 + r;
          ysum = fma((double)lds_a[kr * KG_LDA + ycol], lds_wy[kr], ysum);
        }
      }
    }
  }
  if (xty) {
    __syncthreads();
    double* red = lds_b;                                       // (128 doubles of the 32 x 80)
    if (yhalf == 1) red[ycol] = ysum;
    __syncthreads();
    if (yhalf == 0 && i0 + ycol < M) {
      const double s = ysum + red[ycol];
      bout[i0 + ycol] = beta != 0.0 ? fma(beta, bout[i0 + ycol], s) : s;
    }
  }
  // the entries on and below the diagonal, and each one's mirror: G[i][j] and G[j][i] are one value.  With beta != 0 the LOWER
  // entry is the one read (nobody reads above the diagonal, so no workgroup reads what another one writes).  The mirror goes
  // through LDS, a 16 x 16 block per wave at a time, so that its stores run along G's rows as the lower ones do.
  __syncthreads();                                             // everyone is through with lds_b
  double* tr = lds_b + wave * (16 * 17);
  if constexpr (rhs) {
    // the 16 x 16 blocks as below, every entry stored at its transposed place only: 16 lanes run along a row of bout
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        const int r0 = i0 + arow + tm * 16, c0 = j0 + wc * 32 + tn * 16;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) tr[(kq + 4 * reg) * 17 + r16] = acc[tm][tn][reg];
        __syncthreads();
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = r0 + r16, col = c0 + kq + 4 * reg;   // K column `row`, label column `col`
          if (row < M && col < nt) {
            double v = tr[r16 * 17 + kq + 4 * reg];
            double* dst = bout + (int64_t)col * ldb + row;
            if (beta != 0.0) v = fma(beta, *dst, v);
            *dst = v;
          }
        }
        __syncthreads();
      }
    return;
  }
#pragma unroll
  for (int tm = 0; tm < (half ? 2 : 4); ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int r0 = i0 + arow + tm * 16, c0 = j0 + wc * 32 + tn * 16;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = r0 + kq + 4 * reg, col = c0 + r16;
        double v = acc[tm][tn][reg];
        if (row < M && col <= row) {                           // (col <= row < M)
          if (beta != 0.0) v = fma(beta, G[(int64_t)row * ldg + col], v);
          G[(int64_t)row * ldg + col] = v;
        }
        tr[(kq + 4 * reg) * 17 + r16] = v;
      }
      __syncthreads();
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = r0 + r16, col = c0 + kq + 4 * reg;     // the block's entry (row, col), stored at G[col][row]
        if (row < M && col < row) G[(int64_t)col * ldg + row] = tr[r16 * 17 + kq + 4 * reg];
      }
      __syncthreads();
    }
}

// The tile (bi, bj) of workgroup blockIdx.x: gridDim.x = 8 x ceil(tile rows / 8) x tile columns, workgroup x runs on XCD x & 7
// (round-robin dispatch), and that XCD walks the tile rows xcd, xcd + 8, ... left to right (the tiles that share an A panel
// share one L2), as rls_gram_tile_of.
__global__ __launch_bounds__(256, 3) void knm_gram_kernel(const float* __restrict__ K, int64_t ldk, int64_t n, int M,
                                                          const double* __restrict__ w, const double* __restrict__ y, double beta,
                                                          double* G, int64_t ldg, double* bout) {
  __shared__ __attribute__((aligned(16))) float lds_a[KG_BK * KG_LDA];
  __shared__ __attribute__((aligned(16))) double lds_b[KG_BK * KG_LDB];
  __shared__ double lds_wy[KG_BK];
  const int tiles_n = (M + KG_BN - 1) / KG_BN;
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int bi = 8 * (local / tiles_n) + xcd, bj = local % tiles_n;
  const int i0 = bi * KG_BM, j0 = bj * KG_BN;
  if (i0 >= M || j0 >= M || j0 > i0 + KG_BM - 1) return;      // lower tiles only
  if (j0 == 0 && y != nullptr && bout != nullptr)
    knm_gram_tile<false, true>(K, ldk, n, M, w, y, beta, G, ldg, bout, i0, j0, lds_a, lds_b, lds_wy);
  else if (j0 == i0 + 64)
    knm_gram_tile<true, false>(K, ldk, n, M, w, y, beta, G, ldg, bout, i0, j0, lds_a, lds_b, lds_wy);
  else
    knm_gram_tile<false, false>(K, ldk, n, M, w, y, beta, G, ldg, bout, i0, j0, lds_a, lds_b, lds_wy);
}

// knm_gram_kernel's tiles with ceil(nt / 64) further tile columns behind the tiles_n of G: tile column tiles_n + c of tile row bi
// holds B[64 c .. 64 c + 63][128 bi .. 128 bi + 127].  gridDim.x = 8 x ceil(tile rows / 8) x (tiles_n + ceil(nt / 64)).  The G tiles
// keep knm_gram_kernel's map (XCD x walks the tile rows x, x + 8, ...); a tile row's lower tiles grow with its index, so XCD 7
// carries the most of every round and XCD 0 the fewest, and the right-hand-side tiles go the other way round: those of tile row
// 8 r + 7 - x run on XCD x.  The G tiles are knm_gram_tile<HALF, false>, so G has knm_gram_kernel's bits.
__global__ __launch_bounds__(256, 3) void knm_gram_rhsn_kernel(const float* __restrict__ K, int64_t ldk, int64_t n, int M,
                                                               const double* __restrict__ w, const double* __restrict__ Y,
                                                               int64_t ldy, int nt, double beta, double* G, int64_t ldg, double* B,
                                                               int64_t ldb) {
  __shared__ __attribute__((aligned(16))) float lds_a[KG_BK * KG_LDA];
  __shared__ __attribute__((aligned(16))) double lds_b[KG_BK * KG_LDB];
  const int tiles_n = (M + KG_BN - 1) / KG_BN, tiles_all = tiles_n + (nt + KG_BN - 1) / KG_BN;
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int bj = local % tiles_all;
  const int bi = 8 * (local / tiles_all) + (bj >= tiles_n ? 7 - xcd : xcd);
  const int i0 = bi * KG_BM;
  if (i0 >= M) return;
  if (bj >= tiles_n) {
    knm_gram_tile<false, false, true>(K, ldk, n, M, w, Y, beta, nullptr, 0, B, i0, (bj - tiles_n) * KG_BN, lds_a, lds_b, nullptr, ldy, nt,
                                      ldb);
    return;
  }
  const int j0 = bj * KG_BN;
  if (j0 >= M || j0 > i0 + KG_BM - 1) return;                  // lower tiles only
  if (j0 == i0 + 64)
    knm_gram_tile<true, false>(K, ldk, n, M, w, nullptr, beta, G, ldg, nullptr, i0, j0, lds_a, lds_b, nullptr);
  else
    knm_gram_tile<false, false>(K, ldk, n, M, w, nullptr, beta, G, ldg, nullptr, i0, j0, lds_a, lds_b, nullptr);
}

// Y[q][i] = alpha * sum_{j < M} G[i][j] X[q][j] for q < nv <= NV vectors from ONE read of G: trmvn_f64_kernel (dense_f64.hip)
// over whole rows.  A wave owns RB = 4 consecutive rows and uses every 16-byte fragment of X[q] it loads for all four; the
// pairs [0, M / 2) go through the 16-byte loop, the last element of an odd M is lane 0's first term; the RB x NV sums of a wave
// are reduced transposing.  Every order of additions is fixed.  Vectors past nv repeat vector nv - 1 and are not stored.
template <int NV>
__global__ __launch_bounds__(256) void symvn_f64_kernel(const double* __restrict__ G, int64_t ldg, int64_t M, int nv,
                                                        const double* __restrict__ X, int64_t ldx, double alpha,
                                                        double* __restrict__ Y, int64_t ldy) {
  constexpr int RB = 4, N = RB * NV;
  static_assert((N & (N - 1)) == 0 && N <= 64, "the transposing reduction needs a power-of-two count of sums");
  const int lane = threadIdx.x & 63;
  const int64_t nrb = (M + RB - 1) / RB;
  const int64_t rb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rb >= nrb) return;
  const int64_t i0 = rb * RB;
  const double* row[RB];
  const double* xq[NV];
#pragma unroll
  for (int k = 0; k < RB; ++k) row[k] = G + (i0 + k < M ? i0 + k : M - 1) * ldg;
#pragma unroll
  for (int q = 0; q < NV; ++q) xq[q] = X + (int64_t)(q < nv ? q : nv - 1) * ldx;
  double acc[RB][NV];
#pragma unroll
  for (int k = 0; k < RB; ++k)
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[k][q] = 0.0;
  if (lane == 0 && (M & 1)) {
#pragma unroll
    for (int k = 0; k < RB; ++k) {
      const double a = row[k][M - 1];
#pragma unroll
      for (int q = 0; q < NV; ++q) acc[k][q] = a * xq[q][M - 1];
    }
  }
  const int64_t q1 = M >> 1;
#pragma unroll 2
  for (int64_t p = lane; p < q1; p += 64) {
    f64x2g a[RB];
#pragma unroll
    for (int k = 0; k < RB; ++k) a[k] = *reinterpret_cast<const f64x2g*>(row[k] + 2 * p);
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const f64x2g b = *reinterpret_cast<const f64x2g*>(xq[q] + 2 * p);
#pragma unroll
      for (int k = 0; k < RB; ++k) acc[k][q] = fma(a[k][1], b[1], fma(a[k][0], b[0], acc[k][q]));
    }
  }
  // transposing reduction: at every step a lane hands half of its values to its partner and keeps the sums of the other
  // half; lane l ends with the total of value idx(l)
  double* s = &acc[0][0];
  int off = 32;
#pragma unroll
  for (int hf = N / 2; hf >= 1; hf >>= 1, off >>= 1) {
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < hf; ++i) {
      const double give = up ? s[i] : s[hf + i], keep = up ? s[hf + i] : s[i];
      s[i] = keep + __shfl_xor(give, off);
    }
  }
#pragma unroll
  for (; off > 0; off >>= 1) s[0] += __shfl_xor(s[0], off);
  int idx = 0, bit = 32;
#pragma unroll
  for (int hf = N / 2; hf >= 1; hf >>= 1, bit >>= 1) idx += (lane & bit) ? hf : 0;
  if ((lane & (64 / N - 1)) == 0 || N == 64) {
    const int k = idx / NV, q = idx % NV;
    const int64_t i = i0 + k;
    if (i < M && q < nv) Y[(int64_t)q * ldy + i] = alpha * s[0];
  }
}

}  // namespace odx

extern "C" int odx_knm_gram_f64(const float* K, int64_t ldk, int64_t n, int64_t M, const double* w, const double* y, double beta,
                                double* G, int64_t ldg, double* b, odx_stream_t stream) {
  using namespace odx;
  if (M <= 0) return ODX_OK;
  if (n <= 0 && beta == 1.0) return ODX_OK;
  ODX_REQUIRE(G, "odx_knm_gram_f64: null G");
  ODX_REQUIRE(M < (1ll << 20), "odx_knm_gram_f64: M must be below 2^20");
  ODX_REQUIRE(ldg >= M && (reinterpret_cast<uintptr_t>(G) & 7u) == 0, "odx_knm_gram_f64: G needs ldg >= M and 8-byte alignment");
  ODX_REQUIRE((y == nullptr) == (b == nullptr), "odx_knm_gram_f64: y and b are given together or not at all");
  if (n > 0) {
    ODX_REQUIRE(K, "odx_knm_gram_f64: null K");
    ODX_REQUIRE(aligned16(K) && ldk % 4 == 0 && ldk >= M, "odx_knm_gram_f64: K must be 16-byte aligned with ldk %% 4 == 0 and ldk >= M");
  }
  const int64_t tiles_m = ceil_div(M, KG_BM), tiles_n = ceil_div(M, KG_BN);
  const int64_t grid = 8 * ceil_div(tiles_m, 8) * tiles_n;
  ODX_REQUIRE(grid < (1ll << 31), "odx_knm_gram_f64: too many tiles");
  const int64_t nn = n > 0 ? n : 0;
  hipLaunchKernelGGL(knm_gram_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), K, ldk, nn, (int)M, w, y, beta, G, ldg, b);
  ODX_CHECK_LAUNCH("odx_knm_gram_f64");
  return ODX_OK;
}

extern "C" int odx_knm_gram_rhsn_f64(const float* K, int64_t ldk, int64_t n, int64_t M, const double* w, const double* Y, int64_t ldy,
                                     int nt, double beta, double* G, int64_t ldg, double* B, int64_t ldb, odx_stream_t stream) {
  using namespace odx;
  if (M <= 0) return ODX_OK;
  ODX_REQUIRE(nt >= 1 && nt <= 1024, "odx_knm_gram_rhsn_f64: 1 .. 1024 label columns per call (got %d)", nt);
  ODX_REQUIRE(G, "odx_knm_gram_rhsn_f64: null G");
  ODX_REQUIRE(M < (1ll << 20), "odx_knm_gram_rhsn_f64: M must be below 2^20");
  ODX_REQUIRE(ldg >= M && (reinterpret_cast<uintptr_t>(G) & 7u) == 0, "odx_knm_gram_rhsn_f64: G needs ldg >= M and 8-byte alignment");
  ODX_REQUIRE(Y && aligned16(Y) && ldy >= nt && ldy % 2 == 0, "odx_knm_gram_rhsn_f64: Y must be 16-byte aligned with ldy even and ldy >= nt");
  ODX_REQUIRE(B && (reinterpret_cast<uintptr_t>(B) & 7u) == 0 && ldb >= M, "odx_knm_gram_rhsn_f64: B needs ldb >= M and 8-byte alignment");
  {  // the doubles G and B span must not share one (a tile of B is stored while other workgroups read and store G)
    const double* ge = G + (M - 1) * ldg + M;
    const double* be = B + (int64_t)(nt - 1) * ldb + M;
    ODX_REQUIRE(ge <= B || be <= G, "odx_knm_gram_rhsn_f64: B must not overlap G");
  }
  if (n > 0) {
    ODX_REQUIRE(K, "odx_knm_gram_rhsn_f64: null K");
    ODX_REQUIRE(aligned16(K) && ldk % 4 == 0 && ldk >= M, "odx_knm_gram_rhsn_f64: K must be 16-byte aligned with ldk %% 4 == 0 and ldk >= M");
  }
  if (n <= 0 && beta == 1.0) return ODX_OK;
  const int64_t tiles_m = ceil_div(M, KG_BM), tiles_all = ceil_div(M, (int64_t)KG_BN) + ceil_div((int64_t)nt, (int64_t)KG_BN);
  const int64_t grid = 8 * ceil_div(tiles_m, 8) * tiles_all;
  ODX_REQUIRE(grid < (1ll << 31), "odx_knm_gram_rhsn_f64: too many tiles");
  const int64_t nn = n > 0 ? n : 0;
  hipLaunchKernelGGL(knm_gram_rhsn_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), K, ldk, nn, (int)M, w, Y, ldy, nt, beta, G,
                     ldg, B, ldb);
  ODX_CHECK_LAUNCH("odx_knm_gram_rhsn_f64");
  return ODX_OK;
}

extern "C" int odx_symvn_f64(const double* G, int64_t ldg, int64_t M, int nv, const double* X, int64_t ldx, double alpha, double* Y,
                             int64_t ldy, odx_stream_t stream) {
  using namespace odx;
  ODX_REQUIRE(nv >= 1 && nv <= 8, "odx_symvn_f64: 1 .. 8 vectors per call (got %d)", nv);
  if (M <= 0) return ODX_OK;
  ODX_REQUIRE(G && X && Y, "odx_symvn_f64: null pointer");
  ODX_REQUIRE(ldg % 2 == 0 && ldg >= M && aligned16(G) && aligned16(X) && ldx % 2 == 0,
              "odx_symvn_f64: G/X must be 16-byte aligned, ldg and ldx even, ldg >= M");
  ODX_REQUIRE(nv == 1 || (ldx >= M && ldy >= M), "odx_symvn_f64: rows of X and Y must be M apart or more");
  {  // the doubles X and Y span, [first, last]: they must not share one (the kernel reads X while other rows' sums are stored)
    const double* xe = X + (int64_t)(nv - 1) * ldx + M;
    const double* ye = Y + (int64_t)(nv - 1) * ldy + M;
    ODX_REQUIRE(xe <= Y || ye <= X, "odx_symvn_f64: X and Y must not overlap");
  }
  const dim3 grid((unsigned)ceil_div(ceil_div(M, (int64_t)4), (int64_t)4));      // four row blocks of four rows per workgroup
#define ODX_SYMVN(NV_) \
  hipLaunchKernelGGL(symvn_f64_kernel<NV_>, grid, dim3(256), 0, as_stream(stream), G, ldg, M, nv, X, ldx, alpha, Y, ldy)
  if (nv <= 2) ODX_SYMVN(2);
  else if (nv <= 4) ODX_SYMVN(4);
  else ODX_SYMVN(8);
#undef ODX_SYMVN
  ODX_CHECK_LAUNCH("odx_symvn_f64");
  return ODX_OK;
}
