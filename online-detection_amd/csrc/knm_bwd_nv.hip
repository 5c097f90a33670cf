// The backward-only NV pass  out[q] = K' W[q],  q = 0 .. nv - 1,  1 <= nv <= 8,  from ONE read of a K_nM shard stored in a
// compact format (24-bit fixed point or bf16, knm_pass_q.hip): the right-hand sides of a multi-output fit
// (solver.falkon_fit_multi: one block, T label columns).  A loop of single passes odx_knm_fwd_bwd_q(v = null, w = W[q]) reads the
// block nv times; a further vector costs one f64 FMA per entry here.
//
// This is phase 2 of knm_passnv_kernel with the row dots given instead of computed.  Without a phase 1 no vector lives in
// LDS and a workgroup does not need a whole row, so the LDS limit of the NV pass (8 vectors up to M = 2524) does not
// apply: the block is tiled as column BANDS x row ranges.  A 256-thread workgroup owns one band of 256 4-column chunks
// (thread t: chunk band * 256 + t, CH = 1) and walks the row blocks g, g + G, ... of R = 16 / NV rows; a thread keeps its
// NV x 4 column sums in f64 registers (8 NV VGPRs) and decodes each chunk once for all NV vectors.  The raw rows are
// double-buffered in registers (2 x R x 3 VGPRs): the loads of block i + 1 are in flight while block i is multiplied.  No
// LDS, no barrier: a CU holds as many workgroups as its registers allow.
//
// The weights of a row block are wave-uniform.  They are read through uniform addresses, which the compiler turns into
// scalar loads, and enter the FMAs as scalar operands; the weights of block i + 1 are requested as soon as those of block
// i are dead (one set of NV x R = 16 doubles fits the scalar registers beside the descriptors and row pointers, two do
// not).  Nothing in the source forces the loads to stay scalar: after a compiler change check the kernels' s_load count
// in the assembly, and tools/kernel_resources.py (scratch must stay 0) with sgpr_spill_count in the code object's metadata
// — 27 .. 47 scalars are parked in lanes of a vector register today, by v_writelane / v_readlane, without memory traffic.
//
// K is read through one buffer descriptor per plane and row block, as in knm_passq_body (hardware range check: nothing is
// read past the block's last row).  The n % R rows behind the last whole block are added one by one by the first row
// range.  A lane whose chunk lies past the row's end reads the start of the next row or the range check's zero (finite
// entries) and stores nothing.  One slab per (vector, row-range workgroup) — the bands of a row range write disjoint
// columns of it — and the fixed-order reducer of knm_pass.hip: no atomics, bitwise reproducible.  Widths 1, 3 and 5 .. 7
// run on the next instantiated width (2, 4, 8) with vector nv - 1 repeated behind them; those column sums are neither
// stored nor reduced.
#include <algorithm>
#include <stdlib.h>

#include "knm_q.h"
#include "odx_internal.h"

namespace odx {

constexpr int BW_NT = 256;      // threads of a workgroup = chunks of a band
// rows of a row block at the instantiated width nvt: NV x R = 16 weights.  (With 32 the compiler parked 394 scalars in vector
// lanes and the NV = 8 kernel took 117 VGPRs instead of 83.)
constexpr int bw_rows(int nvt) { return 16 / nvt; }
constexpr int BW_WPC = 4;       // workgroups per CU the grid is sized for

template <int NV, int FMT>
__global__ __launch_bounds__(BW_NT) void knm_bwdnv_kernel(const unsigned short* __restrict__ Khi, int64_t ldk,
                                                          const unsigned char* __restrict__ Klo, int64_t ldlo, int64_t n, int64_t M,
                                                          int nv, const double* __restrict__ W, int64_t ldw,
                                                          double* __restrict__ slab, int64_t slab_ld) {
  constexpr int NT = BW_NT, R = bw_rows(NV), CW = QCW;
  const int band = (int)blockIdx.x, g = (int)blockIdx.y, G = (int)gridDim.y;
  const int tid = threadIdx.x;
  const int nchunk = (int)((M + CW - 1) / CW);
  const double vscale = FMT == QF_U24 ? 5.9604644775390625e-08 : 1.0;      // 2^-24 (exact)
  double acc[NV][CW];
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int e = 0; e < CW; ++e) acc[q][e] = 0.0;

  const int rowb_hi = (int)ldk * 2, rowb_lo = (int)ldlo;
  const int voff_hi = tid * (2 * CW), voff_lo = tid * CW;      // the lane's place inside the band
  const int band_hi = band * (NT * 2 * CW), band_lo = band * (NT * CW);
  const int64_t nfull = n / R;      // the streaming loop walks whole row blocks; the n % R rows behind them follow it
  // rows [blk R, blk R + R) of this band into kr; a block past the last whole one re-reads that one (nobody uses it)
  auto load_block = [&](int64_t blk, QChunk<FMT, CW>(&kr)[R]) {
    if (blk >= nfull) blk = nfull - 1;
    const int64_t row0 = blk * R;
    const __amdgpu_buffer_rsrc_t rs_hi =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(Khi + row0 * ldk), (short)0, R * rowb_hi, 0x00020000);
    __amdgpu_buffer_rsrc_t rs_lo;
    if (FMT == QF_U24)
      rs_lo = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(Klo + row0 * ldlo), (short)0, R * rowb_lo, 0x00020000);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const u32x2q th = __builtin_amdgcn_raw_buffer_load_b64(rs_hi, voff_hi, r * rowb_hi + band_hi, 0);
      kr[r].hi[0] = th[0], kr[r].hi[1] = th[1];
      if (FMT == QF_U24) kr[r].lo[0] = __builtin_amdgcn_raw_buffer_load_b32(rs_lo, voff_lo, r * rowb_lo + band_lo, 0);
    }
  };
  // the NV x R weights of a whole block: uniform addresses, R consecutive doubles per vector.  The vectors past nv repeat
  // vector nv - 1: their column sums are never stored.
  auto load_weights = [&](int64_t blk, double (&t)[NV][R]) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const double* wq = W + (int64_t)(q < nv ? q : nv - 1) * ldw + blk * R;
#pragma unroll
      for (int r = 0; r < R; ++r) t[q][r] = wq[r];
    }
  };
  auto multiply = [&](const QChunk<FMT, CW>(&kr)[R], const double (&t)[NV][R]) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int e = 0; e < CW; ++e) {
        const double kd = q_entry<FMT, CW>(kr[r], e);
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[q][e] = fma(kd, t[q][r], acc[q][e]);
      }
  };

  QChunk<FMT, CW> ka[R], kb[R];
  double t[NV][R];
  int64_t blk = g;
  if (blk < nfull) {
    load_block(blk, ka);
    load_weights(blk, t);
  }
  for (; blk < nfull; blk += 2 * (int64_t)G) {
    load_block(blk + G, kb);
    multiply(ka, t);
    if (blk + G >= nfull) break;
    load_weights(blk + G, t);
    load_block(blk + 2 * (int64_t)G, ka);
    multiply(kb, t);
    if (blk + 2 * (int64_t)G < nfull) load_weights(blk + 2 * (int64_t)G, t);
  }
  // the n % R rows behind the whole blocks, one at a time, by the first row range (a one-row descriptor: a chunk past the
  // row's end reads as zero)
  if (g == 0) {
    for (int64_t row = nfull * R; row < n; ++row) {
      QChunk<FMT, CW> k1;
      const __amdgpu_buffer_rsrc_t rs_hi =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(Khi + row * ldk), (short)0, rowb_hi, 0x00020000);
      const u32x2q th = __builtin_amdgcn_raw_buffer_load_b64(rs_hi, voff_hi, band_hi, 0);
      k1.hi[0] = th[0], k1.hi[1] = th[1];
      if (FMT == QF_U24) {
        const __amdgpu_buffer_rsrc_t rs_lo =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(Klo + row * ldlo), (short)0, rowb_lo, 0x00020000);
        k1.lo[0] = __builtin_amdgcn_raw_buffer_load_b32(rs_lo, voff_lo, band_lo, 0);
      }
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const double wv = W[(int64_t)(q < nv ? q : nv - 1) * ldw + row];
#pragma unroll
        for (int e = 0; e < CW; ++e) acc[q][e] = fma(q_entry<FMT, CW>(k1, e), wv, acc[q][e]);
      }
    }
  }
  // slab[q][g][slab_ld]: vector q's slabs are contiguous, one "class" of the batched fixed-order reducer
  const int ch = band * NT + tid;
  if (ch < nchunk) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      if (q >= nv) break;
      double* my = slab + ((int64_t)q * G + g) * slab_ld + (int64_t)ch * CW;      // (slab_ld = roundup(M, 4): the chunk is inside)
      f64x2q lo2, hi2;
      lo2[0] = acc[q][0] * vscale, lo2[1] = acc[q][1] * vscale;
      hi2[0] = acc[q][2] * vscale, hi2[1] = acc[q][3] * vscale;
      *reinterpret_cast<f64x2q*>(my) = lo2;
      *reinterpret_cast<f64x2q*>(my + 2) = hi2;
    }
  }
}

static int bw_bands(int64_t M) { return (int)ceil_div(ceil_div(M, (int64_t)QCW), (int64_t)BW_NT); }

// row-range workgroups per band: the grid fills `cus` compute units BW_WPC times over (monotone in cus: the workspace is
// sized for the device's, a launch may be confined to fewer)
static int bw_ranges(int64_t n, int64_t M, int nv, int cus) {
  int64_t G = ceil_div((int64_t)cus * BW_WPC, (int64_t)bw_bands(M));
  const int64_t nfull = n / bw_rows(q_nvt(nv));      // whole row blocks (the rows behind them go to the first range)
  if (G > nfull) G = nfull;
  return (int)(G < 1 ? 1 : G);
}

// launch(kernel) for the instantiated width that serves nv
template <int FMT, typename Launch>
static int dispatch_bwdnv(int nv, Launch&& launch) {
  if (q_nvt(nv) == 2) return launch(knm_bwdnv_kernel<2, FMT>);
  if (q_nvt(nv) == 4) return launch(knm_bwdnv_kernel<4, FMT>);
  return launch(knm_bwdnv_kernel<8, FMT>);
}

}  // namespace odx

using namespace odx;

extern "C" int64_t odx_knm_bwdn_q_workspace_bytes(int64_t n, int64_t M, int fmt, int nv) {
  if (!q_nv_supported(M, fmt, nv)) return ODX_ERR_UNSUPPORTED;
  if (n <= 0) return 0;
  return (int64_t)nv * bw_ranges(n, M, nv, workspace_cus()) * round_up(M, 4) * (int64_t)sizeof(double);
}

extern "C" int odx_knm_bwdn_q(const void* K, int64_t ldk, const void* Klo, int64_t ldlo, int fmt, int64_t n, int64_t M, int nv,
                              const double* W, int64_t ldw, double* out, int64_t ldo, void* workspace, int64_t workspace_bytes,
                              odx_stream_t stream) {
  ODX_REQUIRE_Q_NV("odx_knm_bwdn_q", M, fmt, nv);
  ODX_REQUIRE(out && aligned16(out) && ldo % 2 == 0 && ldo >= M, "odx_knm_bwdn_q: out must be 16-byte aligned with even ldo >= M");
  hipStream_t s = as_stream(stream);
  if (n <= 0) {
    ODX_CHECK_HIP(hipMemset2DAsync(out, (size_t)ldo * sizeof(double), 0, (size_t)M * sizeof(double), (size_t)nv, s));
    return ODX_OK;
  }
  ODX_REQUIRE(W && aligned16(W) && ldw % 2 == 0 && ldw >= n, "odx_knm_bwdn_q: W must be 16-byte aligned with even ldw >= n");
  ODX_PROPAGATE(check_q_block("odx_knm_bwdn_q", K, ldk, Klo, ldlo, fmt, M));
  const int G = bw_ranges(n, M, nv, pass_cus());
  const int64_t slab_ld = round_up(M, 4);
  ODX_PROPAGATE(require_workspace("odx_knm_bwdn_q", workspace, workspace_bytes, (int64_t)nv * G * slab_ld * (int64_t)sizeof(double)));
  ODX_REQUIRE(G < 65536, "odx_knm_bwdn_q: too many row ranges");
  double* slab = static_cast<double*>(workspace);
  const dim3 grid((unsigned)bw_bands(M), (unsigned)G);
  ODX_PROPAGATE(q_dispatch(q_block(K, ldk, Klo, ldlo, fmt, n, M), [&](auto f, const QBlock& b) {
    return dispatch_bwdnv<decltype(f)::value>(nv, [&](auto* kernel) {
      return q_launch(kernel, grid, BW_NT, 0, s, b.hi, b.ldk, b.lo, b.ldlo, b.n, b.M, nv, W, ldw, slab, slab_ld);
    });
  }));
  ODX_CHECK_LAUNCH("odx_knm_bwdn_q");
  return reduce_nv(nv, M, G, slab, slab_ld, out, ldo, s);
}
