// Ridge leverage scores (odx/leverage.py): the row quadratic form q_r = |Li k_r|^2 of an f32 K_nM block against the f64
// inverse Cholesky factor of the dictionary's matrix, and that matrix itself for any radial kernel and diagonal.
//   odx_knm_rowquad_f64 : one workgroup per 128 rows walks the 64-column tiles of Li k_r on v_mfma_f64_16x16x4_f64
//                         (gemm_core.h's f64 tile in the 128 x 64 shape of the f64 NT GEMM), squares the accumulators into
//                         per-lane row sums and stores ONE number per row: the n x M product Li K' is never written (the
//                         composition convert + NT GEMM + reduction writes and re-reads 2 x n M 8 bytes for the same n
//                         numbers)
//   odx_radial_kmm_f64  : gauss_kmm_f64 exported, with a diagonal VECTOR
#include "odx_internal.h"
#include "gemm_core.h"

namespace odx {

// The tile: 128 rows x RQ_BN columns of Li k_r per step, as gemm_nt_kernel<double, 64> has it — 64 accumulator registers, so
// that two workgroups share a CU and hide each other's barriers (the 128 x 128 tile, alone on its CU, ran at 0.55 of the GEMM's
// rate, this one runs at it: profiles/leverage_scores.md; three per CU would spill: the 16 row sums and the f32 stage sit
// beside the accumulators).
constexpr int RQ_BN = 64;
constexpr int RQ_TN = GemmTileN<double, RQ_BN>::TN;       // 2
constexpr int RQ_LDS_BYTES = (GEMM_BM + RQ_BN) * GEMM_LDS_ROW;

struct RowquadStage {
  f32x4 a[2];
  u32x4 b[RQ_BN / 32];
};

template <bool VEC16>
__device__ __forceinline__ void rowquad_load_stage(RowquadStage& st, const float* __restrict__ K, int64_t ldk, int64_t n,
                                                   const double* __restrict__ Li, int64_t ldl, int64_t M, int64_t i0, int64_t j0,
                                                   int64_t kt, int64_t ke) {
  // (a mask right behind a load would make the prefetch wait for it: the k-tiles that need none take the loaders' CLEAN form)
  if (kt + GemmTraits<double>::BK <= ke) gemm_load_operand_f32<true>(st.a, K, ldk, i0, n, kt, ke);
  else gemm_load_operand_f32<false>(st.a, K, ldk, i0, n, kt, ke);
  if (kt + GemmTraits<double>::BK <= j0) gemm_load_operand_lower<VEC16, true, RQ_BN / 32>(st.b, Li, ldl, j0, M, kt, ke);
  else gemm_load_operand_lower<VEC16, false, RQ_BN / 32>(st.b, Li, ldl, j0, M, kt, ke);
}

// q[r] = sum_j (sum_{c <= j} K[r, c] Li[j, c])^2 for the rows [128 blockIdx.x, ...).  Per column tile jt the contraction runs
// over c < min(M, 64 (jt + 1)) in gemm_mainloop's order (k-tiles of 16 ascending); the lane that holds accumulator (row, col)
// adds its square to the row's running sum, column tiles ascending, the tile's two 16-column blocks ascending.  The 16 lanes
// of a row are then summed by a butterfly (the same value in all of them: a + b is b + a) and the two column waves in wave
// order.  Nothing in that order depends on the row's place in its block, on n or on the other rows: q[r] is the same bits
// in every call that holds row r.
template <bool VEC16>
__global__ __launch_bounds__(GEMM_THREADS, 2) void knm_rowquad_kernel(const float* __restrict__ K, int64_t ldk, int64_t n,
                                                                     int64_t M, const double* __restrict__ Li, int64_t ldl,
                                                                     double* __restrict__ q) {
  constexpr int BK = GemmTraits<double>::BK;
  __shared__ __attribute__((aligned(16))) char lds[RQ_LDS_BYTES];
  __shared__ double red[2][GEMM_BM];
  char* ldsA = lds;
  char* ldsB = lds + GEMM_BM * GEMM_LDS_ROW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t i0 = (int64_t)blockIdx.x * GEMM_BM;
  double rs[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; ++tm)
#pragma unroll
    for (int r = 0; r < 4; ++r) rs[tm][r] = 0.0;
  for (int64_t j0 = 0; j0 < M; j0 += RQ_BN) {
    const int64_t ke = j0 + RQ_BN < M ? j0 + RQ_BN : M;
    f64x4 acc[4][RQ_TN];
    gemm_zero_acc<double>(acc);
    RowquadStage st;
    rowquad_load_stage<VEC16>(st, K, ldk, n, Li, ldl, M, i0, j0, 0, ke);
    for (int64_t kt = 0; kt < ke; kt += BK) {
      __syncthreads();  // everyone finished reading the previous k-tile
      gemm_store_operand_f32(st.a, ldsA);
      gemm_store_operand(st.b, ldsB);
      __syncthreads();
      if (kt + BK < ke) rowquad_load_stage<VEC16>(st, K, ldk, n, Li, ldl, M, i0, j0, kt + BK, ke);
      gemm_compute_ktile(acc, ldsA, ldsB, wr, wc, lane);
    }
#pragma unroll
    for (int tn = 0; tn < RQ_TN; ++tn)
#pragma unroll
      for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) rs[tm][r] = fma(acc[tm][tn][r], acc[tm][tn][r], rs[tm][r]);
  }
#pragma unroll
  for (int tm = 0; tm < 4; ++tm)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = rs[tm][r];
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if ((lane & 15) == 0) red[wc][wr * 64 + gemm_acc_row<double>(tm, r, lane)] = v;
    }
  __syncthreads();
  if (threadIdx.x < GEMM_BM) {
    const int64_t row = i0 + threadIdx.x;
    if (row < n) q[row] = red[0][threadIdx.x] + red[1][threadIdx.x];
  }
}

__global__ __launch_bounds__(256) void add_diag_vec_f64_kernel(double* __restrict__ A, int64_t lda, int64_t M,
                                                               const double* __restrict__ diag, double scale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < M) A[i * lda + i] = fma(scale, diag[i], A[i * lda + i]);
}

}  // namespace odx

extern "C" int odx_knm_rowquad_f64(const float* K, int64_t ldk, int64_t n, int64_t M, const double* Li, int64_t ldl, double* q,
                                   odx_stream_t stream) {
  using namespace odx;
  if (n <= 0 || M < 0) return ODX_OK;
  ODX_REQUIRE(q, "odx_knm_rowquad_f64: null output");
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    ODX_CHECK_HIP(hipMemsetAsync(q, 0, (size_t)n * sizeof(double), s));
    return ODX_OK;
  }
  ODX_REQUIRE(K && Li, "odx_knm_rowquad_f64: null operand");
  ODX_REQUIRE(aligned16(K) && ldk % 4 == 0 && ldk >= M, "odx_knm_rowquad_f64: K must be 16-byte aligned with ldk %% 4 == 0 and ldk >= M");
  ODX_REQUIRE(ldl >= M && (reinterpret_cast<uintptr_t>(Li) & 7u) == 0, "odx_knm_rowquad_f64: Li needs ldl >= M and 8-byte alignment");
  const int64_t blocks = ceil_div(n, GEMM_BM);
  ODX_REQUIRE(blocks < (1ll << 31), "odx_knm_rowquad_f64: too many rows");
  // (an odd ldl or a factor that starts off a 16-byte boundary is read by 8-byte loads: the same values, the same bits)
  if (aligned16(Li) && ldl % 2 == 0)
    hipLaunchKernelGGL(knm_rowquad_kernel<true>, dim3((unsigned)blocks), dim3(GEMM_THREADS), 0, s, K, ldk, n, M, Li, ldl, q);
  else
    hipLaunchKernelGGL(knm_rowquad_kernel<false>, dim3((unsigned)blocks), dim3(GEMM_THREADS), 0, s, K, ldk, n, M, Li, ldl, q);
  ODX_CHECK_LAUNCH("odx_knm_rowquad_f64");
  return ODX_OK;
}

extern "C" int odx_radial_kmm_f64(const double* Zd, int64_t ldz, int64_t M, int D, double sigma, int kind, const double* diag,
                                  double diag_scale, double* Kmm, int64_t ldk, double* zsq, odx_stream_t stream) {
  using namespace odx;
  ODX_REQUIRE(kind == ODX_KERNEL_GAUSS || kind == ODX_KERNEL_MATERN32 || kind == ODX_KERNEL_MATERN52,
              "odx_radial_kmm_f64: unknown kernel kind %d", kind);
  if (M <= 0) return ODX_OK;
  ODX_REQUIRE(Zd && Kmm && zsq, "odx_radial_kmm_f64: null pointer");
  ODX_REQUIRE(D > 0 && sigma > 0.0 && ldz >= D && ldk >= M && M < 65536, "odx_radial_kmm_f64: needs D > 0, sigma > 0, ldz >= D, M <= ldk, M < 65536");
  hipStream_t s = as_stream(stream);
  ODX_PROPAGATE(gauss_kmm_f64(Zd, ldz, M, D, sigma, diag ? 0.0 : diag_scale, Kmm, ldk, zsq, s, kind));
  if (diag) {
    hipLaunchKernelGGL(add_diag_vec_f64_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, s, Kmm, ldk, M, diag, diag_scale);
    ODX_CHECK_LAUNCH("odx_radial_kmm_f64");
  }
  return ODX_OK;
}
