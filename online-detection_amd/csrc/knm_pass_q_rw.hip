// The row-weighted pass over a COMPACT-format K_nM block (24-bit fixed point or bf16, knm_q.h):  out = K' (d o (K v))  from ONE
// read of K, at every width the compact passes serve (M = 1 .. 20440) — the product of a sample-weighted squared-loss fit
// (odx/weighted.py: d = the rows' weights).  odx_knm_fwd_bwdn_q_rw gives it from one read up to M = 5084 only; above, the
// route was odx_knm_fwdn_q + odx_knm_bwdn_q: two reads of an HBM-bound block.
//
// The scheme is the barrier form of knm_pass_q.hip's one-vector pass (knm_passq_body, NV = 1), restated here so that no
// existing kernel's code moves: a persistent workgroup streams blocks of R rows; thread t owns the 4-column chunks t, t + NT,
// ... (CH of them) of every row, read through ONE buffer descriptor per plane and row block, keeps their running column sums
// as f64 registers beside the R x CH chunks of the current block as loaded; v sits in LDS as f64 with the 2^-24 of the
// fixed-point scale folded in.  Phase 1 forms the R row dots and reduces them over the workgroup (wave shuffles + one LDS
// exchange, ping-pong buffers: one barrier per block), phase 2 adds K[r, cols] t_r into the column sums and re-issues the
// next block's loads chunk by chunk.  A slab per workgroup and knm_pass.hip's fixed-order reducer: no atomics, bitwise
// reproducible.
//
// The one difference: where that body ADDS w[row] to the reduced row dot, this one MULTIPLIES by d[row].  The R weights of a
// block are wave-uniform values loaded ahead of phase 1 (as knm_pass_rw_kernel loads its weight: the row dots cover the
// latency); t_out is stored as reduced, BEFORE the weight.  d == NULL multiplies by 1.0, which is exact: the bits of a vector
// of ones.
//
// Nothing is read past the block's last existing row (the descriptor's length) and nothing of what the pad holds reaches a
// sum: a chunk past the row's end meets the zero chunk behind v in phase 1 and its column sums are never stored; the columns
// [M, roundup(M, 4)) of the last chunk meet zeros of v, and their column sums land in slab columns the reducer does not read.
// A bf16 pad may hold NaN or Inf bit patterns, which a product with zero does not remove: the bf16 form clears the bits of
// every column >= M in phase 1 (one v_and per loaded dword).  Every 24-bit pattern is a finite integer.
//
// The free-running halves of knm_pass_q.hip are not ported: their rendezvous would have to carry the weight as well, and the
// headline's unweighted pass keeps them to itself.  Every width runs in a barrier configuration (pick_qrwcfg).
#include "odx_internal.h"
#include "knm_q.h"

namespace odx {

template <int NT, int CH, int R, int FMT, int WPE>
__global__ __launch_bounds__(NT, WPE) void knm_passq_rw_kernel(const unsigned short* __restrict__ Khi, int64_t ldk,
                                                               const unsigned char* __restrict__ Klo, int64_t ldlo, int64_t n,
                                                               int64_t M, const double* __restrict__ v,
                                                               const double* __restrict__ d, double* __restrict__ slab,
                                                               int64_t slab_ld, double* __restrict__ t_out) {
  constexpr int NW = NT / 64;
  constexpr int CW = QCW;
  extern __shared__ __attribute__((aligned(16))) double vsrw[];      // [vcap]
  __shared__ double red[2][NW][R];
  const int wg = (int)blockIdx.x, nwg = (int)gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = (int)((M + CW - 1) / CW);
  const int vcap = (nchunk + 1) * CW;      // one chunk of zeros behind the row: where the chunks past the row's end point
  const int64_t nblk = (n + R - 1) / R;
  const double vscale = FMT == QF_U24 ? 5.9604644775390625e-08 : 1.0;      // 2^-24 (exact)
  for (int i = tid; i < vcap; i += NT) vsrw[i] = i < M ? v[i] * vscale : 0.0;
  double acc[CH][CW];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int e = 0; e < CW; ++e) acc[c][e] = 0.0;

  // Addressing as in knm_passq_body: ONE descriptor per plane and row block (base = the block's first row, length = the bytes
  // of its rows that exist); a load takes the lane's place inside a chunk column as its vector offset and [row inside the
  // block] x [row stride] + [chunk column] as its scalar offset, and the hardware checks their SUM against the length.  Rows
  // past n are read as the block's last existing row and their row dots are set to zero before phase 2.
  QChunk<FMT, CW> kr[R][CH];
  const int rowb_hi = (int)ldk * 2, rowb_lo = (int)ldlo;
  const int voff_hi = tid * (2 * CW), voff_lo = tid * CW;
  __amdgpu_buffer_rsrc_t rs_hi, rs_lo;
  int rows_open = R;
  auto open_block = [&](int64_t blk) {
    const int64_t row0 = blk * R;
    rows_open = (int)(n - row0 < R ? n - row0 : R);
    rs_hi = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(Khi + row0 * ldk), (short)0, rows_open * rowb_hi, 0x00020000);
    if (FMT == QF_U24)
      rs_lo = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(Klo + row0 * ldlo), (short)0, rows_open * rowb_lo, 0x00020000);
  };
  auto load_block = [&](int c) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int rr = r < rows_open ? r : rows_open - 1;
      const u32x2q th = __builtin_amdgcn_raw_buffer_load_b64(rs_hi, voff_hi, rr * rowb_hi + c * (NT * 2 * CW), 0);
      kr[r][c].hi[0] = th[0], kr[r][c].hi[1] = th[1];
      if (FMT == QF_U24) kr[r][c].lo[0] = __builtin_amdgcn_raw_buffer_load_b32(rs_lo, voff_lo, rr * rowb_lo + c * (NT * CW), 0);
    }
  };

  int64_t blk = wg;
  if (blk < nblk) {
    open_block(blk);
#pragma unroll
    for (int c = 0; c < CH; ++c) load_block(c);
  }
  __syncthreads();  // vsrw is complete
  int pp = 0;
  for (; blk < nblk; blk += nwg) {
    // the block's R weights: wave-uniform, loaded ahead of the row dots; rows past n and a call without weights keep 1.0
    double wgt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = blk * R + r;
      wgt[r] = (d != nullptr && row < n) ? d[row] : 1.0;
    }
    double t[R];
#pragma unroll
    for (int r = 0; r < R; ++r) t[r] = 0.0;
    {
      // phase 1: row dots.  An opaque zero in the LDS index keeps the (loop-invariant) reads of v inside the loop — hoisted
      // they would hold CH x CW doubles for good (knm_passq_body, same reason).
      int zofs;
      asm volatile("v_mov_b32 %0, 0" : "=v"(zofs));
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        // a chunk past the row's end holds the next row's entries or the pad, not zeros: it is multiplied by the zero chunk
        // behind v
        const int ch = tid + c * NT + zofs;
        const int vi = (ch < nchunk ? ch : nchunk) * CW;
        double vv[CW];
#pragma unroll
        for (int u = 0; u < CW / 2; ++u) {
          const f64x2q a = *reinterpret_cast<const f64x2q*>(&vsrw[vi + 2 * u]);
          vv[2 * u] = a[0];
          vv[2 * u + 1] = a[1];
        }
        if (FMT == QF_BF16) {
          // bf16 only: the bit patterns of the columns >= M are cleared (a NaN or Inf of the pad times the zero of v is NaN).
          // Dword u of a chunk holds columns 2 u (low half) and 2 u + 1; `left` columns of the chunk exist.
          const int left = (int)M - ch * CW;
          unsigned keep[CW / 2];
#pragma unroll
          for (int u = 0; u < CW / 2; ++u) keep[u] = left >= 2 * u + 2 ? 0xffffffffu : (left == 2 * u + 1 ? 0x0000ffffu : 0u);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            QChunk<FMT, CW> k;
#pragma unroll
            for (int u = 0; u < CW / 2; ++u) k.hi[u] = kr[r][c].hi[u] & keep[u];
#pragma unroll
            for (int e = 0; e < CW; ++e) t[r] = fma(q_entry<FMT, CW>(k, e), vv[e], t[r]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < CW; ++e) t[r] = fma(q_entry<FMT, CW>(kr[r][c], e), vv[e], t[r]);
        }
        __builtin_amdgcn_sched_barrier(0);      // one chunk column's decoded entries at a time (register pressure)
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double s = t[r];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) red[pp][wave][r] = s;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < NW; ++u) s += red[pp][u][r];
        t[r] = s;
      }
      pp ^= 1;
    }
    // t_out: the row products K v as reduced, BEFORE the weight.  Every thread holds them; one lane stores, outside the
    // streaming part.
    if (t_out != nullptr) {
      if (tid == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (blk * R + r < n) t_out[blk * R + r] = t[r];
      }
    }
    // the weight, once per row; (the last block only) a repeated row, not a zero one, was read for a row past n
#pragma unroll
    for (int r = 0; r < R; ++r) t[r] = blk * R + r < n ? t[r] * wgt[r] : 0.0;
    // the decoded doubles of phase 1 must not stay live into phase 2 (R x CH x CW doubles: spills): make the raw registers
    // opaque here, phase 2 decodes again
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int u = 0; u < CW / 2; ++u) asm volatile("" : "+v"(kr[r][c].hi[u]));
        if (FMT == QF_U24) {
#pragma unroll
          for (int u = 0; u < CW / 4; ++u) asm volatile("" : "+v"(kr[r][c].lo[u]));
        }
      }
    // phase 2: column sums, and the next block's loads re-issued chunk by chunk.  (The sums of the columns >= M may take up
    // whatever the pad holds: they are the columns nobody reads.)
    const int64_t nxt = blk + nwg;
    if (nxt < nblk) open_block(nxt);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < CW; ++e) acc[c][e] = fma(q_entry<FMT, CW>(kr[r][c], e), t[r], acc[c][e]);
      // (unconditional — behind the last block the loads re-read it and nobody waits for them: a branch around the loads
      // turns every register of the block into a loop-carried select)
      load_block(c);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  double* my = slab + (int64_t)wg * slab_ld;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = tid + c * NT;
    if (ch < nchunk) {
#pragma unroll
      for (int e = 0; e < CW; ++e)
        if ((int64_t)ch * CW + e < slab_ld) my[(int64_t)ch * CW + e] = acc[c][e] * vscale;
    }
  }
}

// The configurations: knm_pass_q.hip's one-vector table with every free-running entry replaced by the barrier form of the
// same (chunks, rows).  The 512 x 5 row streams 6 rows per block: 90 registers of loaded chunks beside 40 of column sums in
// the 256 a wave of a 512-thread workgroup may use (the code object shows no scratch; profiles/weighted_falkon.md).
struct QRwCfg {
  int nt, ch, r, wg_per_cu;
};

static bool pick_qrwcfg(int64_t M, QRwCfg* cfg) {
  if (M < 1 || M > Q_MAX_M) return false;
  const int64_t chunks = (M + 3) / 4;
  if (chunks <= 256) *cfg = {256, 1, 16, 2};
  else if (chunks <= 512) *cfg = {256, 2, 8, 2};
  else if (chunks <= 1024) *cfg = {256, 4, 4, 2};
  else if (chunks <= 2048) *cfg = {256, 8, 3, 2};
  else if (chunks <= 2560) *cfg = {512, 5, 6, 1};
  else if (chunks <= 3072) *cfg = {512, 6, 4, 1};
  else *cfg = {1024, 5, 1, 1};      // v + its zero chunk + the reduction scratch in 160 KB of LDS: M <= 20440
  return true;
}

template <int FMT>
static int dispatch_passq_rw(const QRwCfg& cfg, const QBlock& b, int grid, size_t lds, hipStream_t s, const double* v,
                             const double* d, double* slab, int64_t slab_ld, double* t_out) {
#define ODX_QRW(NT_, CH_, R_)                                                                                                 \
  return q_launch(knm_passq_rw_kernel<NT_, CH_, R_, FMT, (NT_ >= 1024 ? 4 : 2)>, dim3(grid), NT_, lds, s, b.hi, b.ldk, b.lo, \
                  b.ldlo, b.n, b.M, v, d, slab, slab_ld, t_out)
  if (cfg.nt == 256 && cfg.ch == 1) ODX_QRW(256, 1, 16);
  if (cfg.nt == 256 && cfg.ch == 2) ODX_QRW(256, 2, 8);
  if (cfg.nt == 256 && cfg.ch == 4) ODX_QRW(256, 4, 4);
  if (cfg.nt == 256 && cfg.ch == 8) ODX_QRW(256, 8, 3);
  if (cfg.nt == 512 && cfg.ch == 5) ODX_QRW(512, 5, 6);
  if (cfg.nt == 512 && cfg.ch == 6) ODX_QRW(512, 6, 4);
  ODX_QRW(1024, 5, 1);
#undef ODX_QRW
}

}  // namespace odx

using namespace odx;

extern "C" int odx_knm_fwd_bwd_q_rw(const void* K, int64_t ldk, const void* Klo, int64_t ldlo, int fmt, int64_t n, int64_t M,
                                    const double* v, const double* d, double* out, double* t_out, void* workspace,
                                    int64_t workspace_bytes, odx_stream_t stream) {
  ODX_REQUIRE(M > 0 && out, "odx_knm_fwd_bwd_q_rw: M <= 0 or null out");
  hipStream_t s = as_stream(stream);
  if (n <= 0) {
    ODX_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)M * sizeof(double), s));
    return ODX_OK;
  }
  ODX_REQUIRE(v, "odx_knm_fwd_bwd_q_rw: null v");
  ODX_PROPAGATE(check_q_block("odx_knm_fwd_bwd_q_rw", K, ldk, Klo, ldlo, fmt, M));
  QRwCfg cfg;
  if (!pick_qrwcfg(M, &cfg)) {
    set_error("odx_knm_fwd_bwd_q_rw: M = %lld exceeds the %lld columns the compact-format pass kernels are built for", (long long)M,
              (long long)Q_MAX_M);
    return ODX_ERR_UNSUPPORTED;
  }
  // the grid on the WHOLE device, a slab per workgroup: the CUs odx_set_pass_cus / odx_set_pass_reserved_cus leave to
  // concurrent streams are NOT left out (as in odx_knm_fwd_bwd_rw: a weighted fit runs no chain beside its passes).  The
  // slabs lie within odx_knm_fwd_bwd_q_workspace_bytes(n, M, fmt): at every width pick_qrwcfg's workgroups per CU are at
  // most the slabs per CU of that entry's configuration (knm_pass_q.hip, pick_qcfg: a free-running workgroup leaves two)
  const int64_t nblk = ceil_div(n, cfg.r);
  int64_t g = (int64_t)workspace_cus() * cfg.wg_per_cu;
  if (g > nblk) g = nblk;
  const int grid = (int)(g < 1 ? 1 : g);
  const int64_t slab_ld = round_up(M, 4);
  if (workspace == nullptr || workspace_bytes < (int64_t)grid * slab_ld * (int64_t)sizeof(double)) {
    set_error("odx_knm_fwd_bwd_q_rw: workspace too small (%lld < %lld)", (long long)workspace_bytes,
              (long long)((int64_t)grid * slab_ld * (int64_t)sizeof(double)));
    return ODX_ERR_WORKSPACE;
  }
  double* slab = static_cast<double*>(workspace);
  const size_t lds = (size_t)(slab_ld + 4) * sizeof(double);      // v + the zero chunk
  ODX_PROPAGATE(q_dispatch(q_block(K, ldk, Klo, ldlo, fmt, n, M), [&](auto f, const QBlock& b) {
    return dispatch_passq_rw<decltype(f)::value>(cfg, b, grid, lds, s, v, d, slab, slab_ld, t_out);
  }));
  ODX_CHECK_LAUNCH("odx_knm_fwd_bwd_q_rw");
  return slab_reduce_f64(slab, slab_ld, grid, M, out, s);
}
