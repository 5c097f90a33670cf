// The forward-only NV pass  T[q] = K V[q],  q = 0 .. nv - 1,  1 <= nv <= 8,  from ONE read of a K_nM shard stored in a
// compact format (24-bit fixed point or bf16, knm_pass_q.hip), at every M the compact passes serve (M <= 20440).  With
// odx_knm_bwdn_q (knm_bwd_nv.hip: out[q] = K' T[q], also one read at every M) it makes the two-read pass of up to 8 CG
// states above the LDS limit of the one-read NV pass (knm_pass_nv.hip: 8 vectors up to M = 2524, 4 up to M = 5084), where
// pairs of vectors cost one read each.
//
// The vectors live in LDS as f64 (the precision policy of the passes: an f32 copy would put an iteration-dependent 6e-8
// into every product), the 2^-24 of the fixed-point scale folded in on the way (exact).  NV x M doubles do not fit, so the
// block is tiled as column BANDS x row ranges: a band is FW_CH = 5 chunk columns of 64 four-column chunks = 1280 columns,
// NV x 1280 x 8 B = 80 KB at NV = 8, two 256-thread workgroups per CU.
//
// Band sums, the order: ONE workgroup owns a set of row groups and walks the bands in order.  For every band it reloads its
// band of V, streams its rows of that band and adds the band's partial row dots into its own cells of T (band 0 stores,
// band b > 0 reads the cell back and adds).  The cell T[q][row] is written and re-read by the same lane of the same wave in
// every band, so no other workgroup touches it and no workspace, slab or atomic is needed: T[q][row] = ((b0 + b1) + b2) + ...
// in band order, bitwise reproducible.
//
// Inside a band it is knm_mv.hip's scheme: each WAVE owns groups of R = 4 rows (groups wave, wave + waves, ...) and walks a
// group over the band by itself — lane l holds the chunks l, l + 64, ... of each row, all CH chunk columns of the R rows in
// registers as loaded.  A chunk is decoded ONCE into doubles (q_entry) and used for all NV vectors; the loads of the wave's
// next group are re-issued chunk by chunk as soon as a chunk's raw registers are decoded, so R x CH loads per wave stay in
// flight under the FMAs.  The NV x R row dots of a wave are finished by the transposing (reduce-scatter) butterfly of
// trmvn_f64_kernel: NV R - 1 exchanges instead of 6 NV R, and lane idx ends with the total of ONE value, which it adds into T.
//
// LDS layout: vs[q][half][chunk] of 16-byte pairs (half 0: columns 0, 1 of the chunk; half 1: columns 2, 3).  A lane's two
// ds_read_b128 per vector then fall 16 bytes apart from its neighbours' (conflict-free in the instruction's lane groups); the
// natural [q][chunk][4] layout puts lanes 32 bytes apart, a two-way conflict.
//
// Addressing: one buffer descriptor per plane and row group (base = the group's first row, length = the bytes of its rows
// that exist).  The WHOLE offset of a load — row inside the group, band, chunk column, lane — is its per-lane offset, the one
// the hardware range-checks (the scalar offset is not checked and stays zero), so nothing is read past the group's last
// existing row: a chunk past the row's end reads the start of the next row or, in the last row, zero, and meets zeros in LDS
// either way (the columns [M, ld) hold the builds' finite zeros).  The row index is clamped to the group's last existing row:
// rows past n repeat row n - 1 and are not stored.  A group past the last has a zero-length descriptor and reads nothing.  The streaming loop has no branch: it starts on a
// tile of zeros "before" the wave's first group (knm_mv.hip says why).  Widths 1, 3 and 5 .. 7 run on the next instantiated
// width (2, 4, 8) with vector nv - 1 repeated behind them; those row dots are not stored.
#include <algorithm>
#include <stdlib.h>

#include "knm_q.h"
#include "odx_internal.h"

namespace odx {

constexpr int FW_NT = 256;      // threads of a workgroup: 4 waves sharing one band of V
constexpr int FW_R = 4;         // rows of a wave's group
constexpr int FW_CH = 5;        // chunk columns (64 chunks of 4 columns) of a band
constexpr int FW_BCH = FW_CH * 64, FW_BCOLS = FW_BCH * QCW;      // chunks / columns of a band: 320 / 1280
constexpr int FW_WPC = 2;       // workgroups per CU the grid is sized for (2 x 80 KB of LDS at NV = 8)

template <int NV, int FMT>
__global__ __launch_bounds__(FW_NT, 2) void knm_fwdnv_kernel(const unsigned short* __restrict__ Khi, int64_t ldk,
                                                             const unsigned char* __restrict__ Klo, int64_t ldlo, int64_t n, int64_t M,
                                                             int nv, const double* __restrict__ V, int64_t ldv, double* T, int64_t ldt) {
  constexpr int NW = FW_NT / 64, R = FW_R, CH = FW_CH, CW = QCW, BCH = FW_BCH, BCOLS = FW_BCOLS, N = NV * R;
  static_assert((N & (N - 1)) == 0 && N <= 64, "the transposing reduction needs a power-of-two count of row dots");
  extern __shared__ __attribute__((aligned(16))) double vs[];      // [NV][2][BCH] pairs
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (wave-uniform: keeps the descriptors in SGPRs)
  const double vscale = FMT == QF_U24 ? 5.9604644775390625e-08 : 1.0;      // 2^-24 (exact)
  const int nbands = (int)((M + BCOLS - 1) / BCOLS);
  const int64_t ngrp = (n + R - 1) / R;
  const int64_t gstep = (int64_t)gridDim.x * NW;
  const int64_t g0 = (int64_t)blockIdx.x * NW + wave;
  const int rowb_hi = (int)ldk * 2, rowb_lo = (int)ldlo;

  // the value this lane owns after the transposing reduction: flat index idx = q * R + r of t[q][r]
  int idx = 0;
  {
    int bit = 32;
#pragma unroll
    for (int half = N / 2; half >= 1; half >>= 1, bit >>= 1) idx += (lane & bit) ? half : 0;
  }
  const int my_q = idx / R, my_r = idx % R;
  const bool writer = ((lane & (64 / N - 1)) == 0 || N == 64) && my_q < nv;
  double* const Tq = T + (int64_t)my_q * ldt;

  int rows_open = 0;
  auto open = [&](int64_t g, __amdgpu_buffer_rsrc_t& a, __amdgpu_buffer_rsrc_t& b) {
    const int64_t row0 = g * R;
    const bool live = row0 >= 0 && row0 < n;
    rows_open = live ? (int)(n - row0 < R ? n - row0 : R) : 0;
    const int64_t base = live ? row0 : 0;
    a = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(Khi + base * ldk), (short)0, rows_open * rowb_hi, 0x00020000);
    if (FMT == QF_U24)
      b = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(Klo + base * ldlo), (short)0, rows_open * rowb_lo, 0x00020000);
  };

  for (int band = 0; band < nbands; ++band) {
    __syncthreads();      // every wave is done with the previous band of V
    for (int i = tid; i < NV * BCOLS; i += FW_NT) {
      const int q = i / BCOLS, j = i % BCOLS;
      const int64_t col = (int64_t)band * BCOLS + j;
      const double x = col < M ? V[(int64_t)(q < nv ? q : nv - 1) * ldv + col] * vscale : 0.0;
      vs[((q * 2 + ((j >> 1) & 1)) * BCH + (j >> 2)) * 2 + (j & 1)] = x;
    }
    __syncthreads();

    const int voff_hi = band * (BCOLS * 2) + lane * (2 * CW), voff_lo = band * BCOLS + lane * CW;
    QChunk<FMT, CW> kr[R][CH];
    auto load = [&](const __amdgpu_buffer_rsrc_t& a, const __amdgpu_buffer_rsrc_t& b, int c) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int rr = r < rows_open ? r : (rows_open > 0 ? rows_open - 1 : 0);      // (scalar) never a row past the group's last
        const u32x2q th = __builtin_amdgcn_raw_buffer_load_b64(a, voff_hi + c * (64 * 2 * CW) + rr * rowb_hi, 0, 0);
        kr[r][c].hi[0] = th[0], kr[r][c].hi[1] = th[1];
        if (FMT == QF_U24) kr[r][c].lo[0] = __builtin_amdgcn_raw_buffer_load_b32(b, voff_lo + c * (64 * CW) + rr * rowb_lo, 0, 0);
      }
    };
    // the loop starts on a tile of zeros before the wave's first group: every load is issued at ONE place
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        kr[r][c].hi[0] = 0u, kr[r][c].hi[1] = 0u;
        if (FMT == QF_U24) kr[r][c].lo[0] = 0u;
      }
    int64_t g = g0 - gstep;
    while (g < ngrp) {
      const int64_t gn = g + gstep;
      __amdgpu_buffer_rsrc_t na, nb;
      open(gn, na, nb);
      // the lane's cell of T: what the earlier bands left there, requested ahead of the FMAs
      const int64_t row = g * R + my_r;
      const bool store = writer && row >= 0 && row < n;
      double told = 0.0;
      if (store && band > 0) told = Tq[row];
      double t[NV][R];
#pragma unroll
      for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int r = 0; r < R; ++r) t[q][r] = 0.0;
      // an opaque zero in the LDS index keeps the (loop-invariant) reads of V inside the loop — hoisted they would hold
      // NV x CH x CW doubles for good
      int zofs;
      asm volatile("v_mov_b32 %0, 0" : "=v"(zofs));
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        double kd[R][CW];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int e = 0; e < CW; ++e) kd[r][e] = q_entry<FMT, CW>(kr[r][c], e);
        // (unconditional: past the wave's last group the descriptor has zero length and the loads touch no memory)
        load(na, nb, c);
        const int ch = c * 64 + lane + zofs;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
          const f64x2q a01 = *reinterpret_cast<const f64x2q*>(&vs[((q * 2) * BCH + ch) * 2]);
          const f64x2q a23 = *reinterpret_cast<const f64x2q*>(&vs[((q * 2 + 1) * BCH + ch) * 2]);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            t[q][r] = fma(kd[r][0], a01[0], t[q][r]);
            t[q][r] = fma(kd[r][1], a01[1], t[q][r]);
            t[q][r] = fma(kd[r][2], a23[0], t[q][r]);
            t[q][r] = fma(kd[r][3], a23[1], t[q][r]);
          }
          if (q % 2 == 1) __builtin_amdgcn_sched_barrier(0);      // two vectors' LDS reads at a time (register pressure)
        }
        __builtin_amdgcn_sched_barrier(0);      // one chunk column's decoded entries at a time (register pressure)
      }
      // transposing reduction: at every step a lane hands half of its values to its partner and keeps the sums of the other
      // half; lane l ends with the total of value idx(l).  Every order of additions is fixed.
      {
        double* s = &t[0][0];
        int off = 32;
#pragma unroll
        for (int half = N / 2; half >= 1; half >>= 1, off >>= 1) {
          const bool up = (lane & off) != 0;
#pragma unroll
          for (int i = 0; i < half; ++i) {
            const double give = up ? s[i] : s[half + i], keep = up ? s[half + i] : s[i];
            s[i] = keep + __shfl_xor(give, off);
          }
        }
#pragma unroll
        for (; off > 0; off >>= 1) s[0] += __shfl_xor(s[0], off);
        if (store) Tq[row] = told + s[0];
      }
      g = gn;
    }
  }
}

// launch(kernel) for the instantiated width that serves nv
template <int FMT, typename Launch>
static int dispatch_fwdnv(int nv, Launch&& launch) {
  if (q_nvt(nv) == 2) return launch(knm_fwdnv_kernel<2, FMT>);
  if (q_nvt(nv) == 4) return launch(knm_fwdnv_kernel<4, FMT>);
  return launch(knm_fwdnv_kernel<8, FMT>);
}

}  // namespace odx

using namespace odx;

// (no workspace: the band partials are added into T itself, by the lane that owns the cell)
extern "C" int64_t odx_knm_fwdn_q_workspace_bytes(int64_t n, int64_t M, int fmt, int nv) {
  (void)n;
  return q_nv_supported(M, fmt, nv) ? 0 : ODX_ERR_UNSUPPORTED;
}

extern "C" int odx_knm_fwdn_q(const void* K, int64_t ldk, const void* Klo, int64_t ldlo, int fmt, int64_t n, int64_t M, int nv,
                              const double* V, int64_t ldv, double* T, int64_t ldt, void* workspace, int64_t workspace_bytes,
                              odx_stream_t stream) {
  (void)workspace, (void)workspace_bytes;
  ODX_REQUIRE_Q_NV("odx_knm_fwdn_q", M, fmt, nv);
  ODX_REQUIRE(T && aligned16(T) && ldt % 2 == 0 && ldt >= n, "odx_knm_fwdn_q: T must be 16-byte aligned with even ldt >= n");
  if (n <= 0) return ODX_OK;
  ODX_REQUIRE(V && aligned16(V) && ldv % 2 == 0 && ldv >= M, "odx_knm_fwdn_q: V must be 16-byte aligned with even ldv >= M");
  ODX_PROPAGATE(check_q_block("odx_knm_fwdn_q", K, ldk, Klo, ldlo, fmt, M));
  hipStream_t s = as_stream(stream);
  const int64_t need = ceil_div(ceil_div(n, (int64_t)FW_R), (int64_t)(FW_NT / 64));      // workgroups that give every wave one row group
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(need, (int64_t)pass_cus() * FW_WPC));
  const size_t lds = (size_t)q_nvt(nv) * FW_BCOLS * sizeof(double);      // a band of the vectors of the instantiated width
  ODX_PROPAGATE(q_dispatch(q_block(K, ldk, Klo, ldlo, fmt, n, M), [&](auto f, const QBlock& b) {
    return dispatch_fwdnv<decltype(f)::value>(nv, [&](auto* kernel) {
      return q_launch(kernel, dim3(grid), FW_NT, lds, s, b.hi, b.ldk, b.lo, b.ldlo, b.n, b.M, nv, V, ldv, T, ldt);
    });
  }));
  ODX_CHECK_LAUNCH("odx_knm_fwdn_q");
  return ODX_OK;
}
