// The NV-vector pass  out[q] = K' (K v[q]),  q = 0 .. nv - 1,  3 <= nv <= 8,  from ONE read of a K_nM shard stored in a
// compact format (24-bit fixed point or bf16, knm_pass_q.hip): the pass a lambda path is driven by (solver.falkon_fit_path:
// one CG state per lambda, all of them multiplying the same block).  A single-vector pass is HBM-bound at the chip's copy
// rate, so a further vector costs arithmetic only: 2 f64 FMAs per entry and vector against 3 (2) bytes read once.
//
// The scheme is knm_passq_body's: persistent workgroups stream blocks of R rows; thread t owns the 4-column chunks t,
// t + NT, ... (CH of them) of every row and keeps their NV x CH x 4 running column sums in f64 registers; the vectors sit
// in LDS as f64 (NV x (chunks + 1) x 4 doubles: one chunk of zeros behind each, where the chunks past a row's end point);
// phase 1 forms the NV x R row dots and reduces them over the workgroup, phase 2 adds K[r, cols] t[q][r] into the column
// sums and re-issues the next block's loads chunk by chunk.  K is read through one buffer descriptor per plane and row
// block (hardware range check: nothing is read past the block's last row).  A slab per (vector, workgroup) and the
// fixed-order reducer of knm_pass.hip: no atomics, bitwise reproducible.  Unlike phase 1 of the one- and two-vector
// kernels, a chunk column's entries are decoded ONCE into doubles and used for all NV vectors (R x 4 doubles live): at
// NV = 8 the decode would otherwise be the larger half of the vector work.
//
// Which (M, NV) exist is decided by LDS: NV (chunks + 1) 32 bytes + the reduction scratch within the CU's 160 KB — NV = 8
// up to M = 2524, NV = 4 up to M = 5084; widths 3 and 5 .. 7 run on the next instantiated width with zero vectors behind
// them (their column sums are neither stored nor reduced).  The vectors stay f64: an f32 copy would fit twice the width
// but put an iteration-dependent 6e-8 into every product.
//
// Configurations (NT, CH, R), all one 512-thread workgroup per CU except the narrowest, and why: the register budget at
// two waves per SIMD is 256 VGPRs; the column sums take 8 NV CH of them, the row dots 2 NV R, a chunk column's decoded
// entries 8 R, the raw block 3 R CH (2 R CH for bf16).
//   NV = 8:  chunks <= 256  (256, 1, 4), two workgroups per CU (their LDS fits twice)
//            chunks <= 512  (512, 1, 4)      64 + 64 + 32 + 12
//            chunks <= 631  (512, 2, 2)     128 + 32 + 16 + 12
//   NV = 4:  chunks <= 256  (256, 1, 8), two workgroups per CU
//            chunks <= 512  (512, 1, 8)      32 + 64 + 64 + 24
//            chunks <= 1024 (512, 2, 4)      64 + 32 + 32 + 24
//            chunks <= 1271 (512, 3, 2)      96 + 16 + 16 + 18
// (Between the phases the row dots are wave-uniform scalars: the waves' partials are reduced by a transposing exchange — NV R - 1
// exchanges instead of 6 NV R — and every wave adds the NW partials of 'its' value and hands the totals out by v_readlane;
// a reduction in which every thread reads all partials from LDS, as the narrower kernels do, spilled at NV R = 32.)
// R is as large as the budget allows without scratch: the bytes a CU keeps in flight are NT x CH x R chunks.
// (tools/kernel_resources.py lists registers and scratch of every instantiation; profiles/falkon_path.md quotes it.)
//
// The row-weighted form  out[q] = K' (d_q o (K v[q]))  (odx_knm_fwd_bwdn_q_rw, 1 <= nv <= 8: the states of a K-fold
// cross-validation, solver.falkon_fit_cv, each a fit with row weights) is the same kernel template with one more parameter (NvRows).  Between
// the phases a row dot is ONE value in one lane (`s` of lane q R + r): that lane loads the row's weight ahead of phase 1,
// multiplies once, and wave 0 stores the unweighted value to T_out — no per-thread weights, nothing further held in
// vector registers across a phase (profiles/cross_validation.md quotes the registers of both forms).
#include <algorithm>
#include <stdlib.h>

#include "knm_q.h"
#include "odx_internal.h"

namespace odx {

// The row weights and row products of the weighted form (odx_knm_fwd_bwdn_q_rw), carried by value: vector q multiplies its
// row dots with row w[q] of D (-1: with nothing) before phase 2, and T (when given) receives them as they were before.
struct NvRows {
  const double* D;
  int64_t ldd;
  int w[8];
  double* T;
  int64_t ldt;
};

__device__ __forceinline__ const NvRows& nv_rows(const NvRows& rw) { return rw; }

// ROWS: nothing (the unweighted kernel: neither its parameters nor its code depend on the weighted form), or one NvRows (the
// weighted form: every statement of it sits under `if constexpr (RW)`).  A pack and not a shared body under two kernels:
// the unweighted kernels' code generation stays what profiles/falkon_path.md measured.
template <int NT, int CH, int R, int NV, int FMT, typename... ROWS>
__global__ __launch_bounds__(NT, 2) void knm_passnv_kernel(const unsigned short* __restrict__ Khi, int64_t ldk,
                                                           const unsigned char* __restrict__ Klo, int64_t ldlo, int64_t n,
                                                           int64_t M, int nv, const double* __restrict__ V, int64_t ldv,
                                                           double* __restrict__ slab, int64_t slab_ld, ROWS... rows) {
  constexpr bool RW = sizeof...(ROWS) != 0;
  static_assert(sizeof...(ROWS) <= 1, "at most one NvRows");
  constexpr int NW = NT / 64;
  constexpr int CW = QCW;
  extern __shared__ __attribute__((aligned(16))) double vsq[];       // [NV][vcap]
  __shared__ double red[2][NW][NV * R];
  const int wg = (int)blockIdx.x, nwg = (int)gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = (int)((M + CW - 1) / CW);
  const int vcap = (nchunk + 1) * CW;      // one chunk of zeros behind the row: where the chunks past the row's end point
  const int64_t nblk = (n + R - 1) / R;
  const double vscale = FMT == QF_U24 ? 5.9604644775390625e-08 : 1.0;      // 2^-24 (exact)
#pragma unroll
  for (int q = 0; q < NV; ++q)
    for (int i = tid; i < vcap; i += NT) vsq[q * vcap + i] = (q < nv && i < M) ? V[(int64_t)q * ldv + i] * vscale : 0.0;
  double acc[NV][CH][CW];
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int e = 0; e < CW; ++e) acc[q][c][e] = 0.0;

  // Addressing as in knm_passq_body: ONE descriptor per plane and row block (base = the block's first row, length = the
  // bytes of its rows that exist); a load's vector offset is the lane's place inside a chunk column, its scalar offset
  // [row inside the block] x [row stride] + [chunk column], and the hardware checks their sum against the length.  Rows
  // past n are read as the block's last existing row and their row dots are set to zero before phase 2; a lane whose
  // chunk lies past the row's end reads the start of the next row: it multiplies the zero chunk behind v in phase 1 and
  // its column sums are never stored.
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
  __syncthreads();  // vsq is complete
  int pp = 0;
  for (; blk < nblk; blk += nwg) {
    // (weighted form) lane q R + r is the one that ends phase 1 with row dot r of vector q in `s` below: it loads that
    // row's weight here, ahead of phase 1, which covers the latency; the other lanes, vectors without a weight row and
    // rows past n keep 1.0 and load nothing
    double wgt = 1.0;
    if constexpr (RW) {
      const NvRows& rw = nv_rows(rows...);
      // (an opaque lane index: the address is formed here, block by block, not kept in registers for the whole loop)
      int ln;
      asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
      if (ln < NV * R) {
        int wr = -1;
#pragma unroll
        for (int q = 0; q < NV; ++q) wr = ln / R == q ? rw.w[q] : wr;
        const int64_t row = blk * R + ln % R;
        if (wr >= 0 && row < n) wgt = rw.D[(int64_t)wr * rw.ldd + row];
      }
    }
    double t[NV][R];
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int r = 0; r < R; ++r) t[q][r] = 0.0;
    // phase 1: row dots.  An opaque zero in the LDS index keeps the (loop-invariant) reads of v inside the loop — hoisted
    // they would hold NV x CH x CW doubles for good.
    int zofs;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zofs));
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      double kd[R][CW];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < CW; ++e) kd[r][e] = q_entry<FMT, CW>(kr[r][c], e);
      const int ch = tid + c * NT + zofs;
      const int vi = (ch < nchunk ? ch : nchunk) * CW;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        double vv[CW];
#pragma unroll
        for (int u = 0; u < CW / 2; ++u) {
          const f64x2q a = *reinterpret_cast<const f64x2q*>(&vsq[q * vcap + vi + 2 * u]);
          vv[2 * u] = a[0];
          vv[2 * u + 1] = a[1];
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int e = 0; e < CW; ++e) t[q][r] = fma(kd[r][e], vv[e], t[q][r]);
      }
      __builtin_amdgcn_sched_barrier(0);      // one chunk column's decoded entries at a time (register pressure)
    }
    // The NV x R row dots of a wave are reduced TRANSPOSING: at every step a lane hands half of its values to its partner
    // and keeps the sums of the other half, so after log2(NV R) steps each lane holds one value summed over a lane group
    // (NV R - 1 exchanges instead of 6 NV R), and plain exchanges finish it.  Lane l ends with the total of value
    // nv_red_index(l); every order of additions is fixed.
    {
      double* a = &t[0][0];
      constexpr int N = NV * R;
      static_assert((N & (N - 1)) == 0 && N <= 64, "the transposing reduction needs a power-of-two count of row dots");
      int off = 32;
#pragma unroll
      for (int half = N / 2; half >= 1; half >>= 1, off >>= 1) {
        const bool up = (lane & off) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
          const double give = up ? a[i] : a[half + i], keep = up ? a[half + i] : a[i];
          a[i] = keep + __shfl_xor(give, off);
        }
      }
#pragma unroll
      for (; off > 0; off >>= 1) a[0] += __shfl_xor(a[0], off);
      int idx = 0, bit = 32;
#pragma unroll
      for (int half = N / 2; half >= 1; half >>= 1, bit >>= 1) idx += (lane & bit) ? half : 0;
      if ((lane & (64 / N - 1)) == 0 || N == 64) red[pp][wave][idx] = a[0];
    }
    __syncthreads();
    // every wave adds the waves' partials of value `lane` (fixed order) and hands the totals out as wave-uniform scalars:
    // NW LDS reads per wave instead of NV R NW broadcast reads, and the row dots leave the vector registers
    {
      double s = 0.0;
      const int vi = lane < NV * R ? lane : 0;
#pragma unroll
      for (int u = 0; u < NW; ++u) s += red[pp][u][vi];
      if constexpr (RW) {
        // the row product K v as it is (wave 0 stores it: every wave holds the same totals), then the weight, once
        const NvRows& rw = nv_rows(rows...);
        const int64_t row = blk * R + lane % R;
        if (rw.T != nullptr && wave == 0 && lane < NV * R && lane / R < nv && row < n) rw.T[(int64_t)(lane / R) * rw.ldt + row] = s;
        s *= wgt;
      }
      const int slo = __double2loint(s), shi = __double2hiint(s);
#pragma unroll
      for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double tot = __hiloint2double(__builtin_amdgcn_readlane(shi, q * R + r), __builtin_amdgcn_readlane(slo, q * R + r));
          t[q][r] = blk * R + r < n ? tot : 0.0;      // (the last block only) a repeated row, not a zero one, was read for it
        }
    }
    pp ^= 1;
    // the decoded doubles of phase 1 must not stay live into phase 2: make the raw registers opaque here, phase 2 decodes
    // again (one row at a time)
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
    // phase 2: column sums, and the next block's loads re-issued chunk by chunk
    const int64_t nxt = blk + nwg;
    if (nxt < nblk) open_block(nxt);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < CW; ++e) {
          const double kd = q_entry<FMT, CW>(kr[r][c], e);
#pragma unroll
          for (int q = 0; q < NV; ++q) acc[q][c][e] = fma(kd, t[q][r], acc[q][c][e]);
        }
      // (unconditional — behind the last block the loads re-read it and nobody waits for them: a branch around the loads
      // turns every register of the block into a loop-carried select)
      load_block(c);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // slab[q][wg][slab_ld]: vector q's slabs are contiguous, one "class" of the batched fixed-order reducer
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    if (q >= nv) break;
    double* my = slab + ((int64_t)q * nwg + wg) * slab_ld;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = tid + c * NT;
      if (ch < nchunk) {
#pragma unroll
        for (int e = 0; e < CW; ++e)
          if ((int64_t)ch * CW + e < slab_ld) my[(int64_t)ch * CW + e] = acc[q][c][e] * vscale;
      }
    }
  }
}

// the two kernels' types (the template's pack of trailing parameters is closed by the conversion)
using NvKernel = void (*)(const unsigned short*, int64_t, const unsigned char*, int64_t, int64_t, int64_t, int, const double*, int64_t,
                          double*, int64_t);
using NvRowsKernel = void (*)(const unsigned short*, int64_t, const unsigned char*, int64_t, int64_t, int64_t, int, const double*,
                              int64_t, double*, int64_t, NvRows);

struct NvCfg {
  int nt, ch, r, nvt, wg_per_cu;      // nvt: the instantiated width (4 or 8) that serves the call's nv
};

static int64_t nv_lds_bytes(const NvCfg& c, int64_t chunks) {
  return (int64_t)c.nvt * (chunks + 1) * 4 * 8;      // dynamic part; the static red[2][NT / 64][nvt * r] comes on top
}

// the configuration of an nv-vector pass over M columns, or false: the vectors (and the reduction scratch) do not fit in LDS.
// nv_min: the narrowest call the entry takes — 3 for the unweighted entry (pairs and singles have kernels of their own in
// knm_pass_q.hip), 1 for the weighted one (nv = 1 and 2 run on the 4-wide instantiation, as nv = 3 does)
static bool pick_nvcfg(int64_t M, int nv, NvCfg* cfg, int nv_min = 3) {
  if (M <= 0 || nv < nv_min || nv > 8) return false;
  const int64_t chunks = (M + 3) / 4;
  const int nvt = nv <= 4 ? 4 : 8;
  NvCfg c;
  if (nvt == 8) {
    if (chunks <= 256) c = {256, 1, 4, 8, 2};
    else if (chunks <= 512) c = {512, 1, 4, 8, 1};
    else c = {512, 2, 2, 8, 1};
  } else {
    if (chunks <= 256) c = {256, 1, 8, 4, 2};
    else if (chunks <= 512) c = {512, 1, 8, 4, 1};
    else if (chunks <= 1024) c = {512, 2, 4, 4, 1};
    else c = {512, 3, 2, 4, 1};
  }
  if (chunks > (int64_t)c.nt * c.ch) return false;
  const int64_t red = 2 * (c.nt / 64) * (int64_t)c.nvt * c.r * 8;
  if (c.wg_per_cu * (nv_lds_bytes(c, chunks) + red) > 163840) return false;
  *cfg = c;
  return true;
}

static int nvgrid_for(const NvCfg& cfg, int64_t n, int cus) {
  int64_t g = (int64_t)cus * cfg.wg_per_cu;
  const int64_t nblk = ceil_div(n, cfg.r);
  if (g > nblk) g = nblk;
  return (int)(g < 1 ? 1 : g);
}

// launch(kernel, threads) for the instantiation cfg names (RW: of the weighted kernel): exactly the configurations
// pick_nvcfg hands out
template <int FMT, bool RW, typename Launch>
static int dispatch_passnv(const NvCfg& cfg, Launch&& launch) {
#define ODX_NV(NT_, CH_, R_, NV_)                                                                        \
  do {                                                                                                   \
    if constexpr (RW)                                                                                    \
      return launch(static_cast<NvRowsKernel>(knm_passnv_kernel<NT_, CH_, R_, NV_, FMT, NvRows>), NT_);    \
    else                                                                                                 \
      return launch(static_cast<NvKernel>(knm_passnv_kernel<NT_, CH_, R_, NV_, FMT>), NT_);                \
  } while (0)
  if (cfg.nvt == 8) {
    if (cfg.nt == 256) ODX_NV(256, 1, 4, 8);
    if (cfg.ch == 1) ODX_NV(512, 1, 4, 8);
    ODX_NV(512, 2, 2, 8);
  }
  if (cfg.nt == 256) ODX_NV(256, 1, 8, 4);
  if (cfg.ch == 1) ODX_NV(512, 1, 8, 4);
  if (cfg.ch == 2) ODX_NV(512, 2, 4, 4);
  ODX_NV(512, 3, 2, 4);
#undef ODX_NV
}

static int64_t passnv_workspace_bytes(int64_t n, int64_t M, int fmt, int nv, int nv_min) {
  NvCfg cfg;
  if (!q_format(fmt) || !pick_nvcfg(M, nv, &cfg, nv_min)) return ODX_ERR_UNSUPPORTED;
  if (n <= 0) return 0;
  return (int64_t)nv * workspace_cus() * cfg.wg_per_cu * round_up(M, 4) * (int64_t)sizeof(double);
}

// The two entries' host code.  rw: the weights and row products of the weighted entry (its caller has checked them), or
// nullptr — the unweighted entry, which launches the unweighted kernels.
static int passnv_run(const char* who, int nv_min, const void* K, int64_t ldk, const void* Klo, int64_t ldlo, int fmt, int64_t n,
                      int64_t M, int nv, const double* V, int64_t ldv, double* out, int64_t ldo, const NvRows* rw, void* workspace,
                      int64_t workspace_bytes, odx_stream_t stream) {
  ODX_REQUIRE(M > 0 && nv >= nv_min && nv <= 8, "%s: M <= 0 or nv outside %d .. 8", who, nv_min);
  ODX_REQUIRE(V && out && aligned16(V) && aligned16(out) && ldv % 2 == 0 && ldo % 2 == 0 && ldv >= M && ldo >= M,
              "%s: V and out must be 16-byte aligned with even ldv, ldo >= M", who);
  hipStream_t s = as_stream(stream);
  if (n <= 0) {
    ODX_CHECK_HIP(hipMemset2DAsync(out, (size_t)ldo * sizeof(double), 0, (size_t)M * sizeof(double), (size_t)nv, s));
    return ODX_OK;
  }
  ODX_PROPAGATE(check_q_block(who, K, ldk, Klo, ldlo, fmt, M));
  NvCfg cfg;
  if (!pick_nvcfg(M, nv, &cfg, nv_min)) {
    set_error("%s: %d vectors of M = %lld do not fit in LDS (use narrower groups)", who, nv, (long long)M);
    return ODX_ERR_UNSUPPORTED;
  }
  const int grid = nvgrid_for(cfg, n, pass_cus());
  const int64_t slab_ld = round_up(M, 4);
  ODX_PROPAGATE(require_workspace(who, workspace, workspace_bytes, (int64_t)nv * grid * slab_ld * (int64_t)sizeof(double)));
  double* slab = static_cast<double*>(workspace);
  const size_t lds = (size_t)nv_lds_bytes(cfg, (M + 3) / 4);
  ODX_PROPAGATE(q_dispatch(q_block(K, ldk, Klo, ldlo, fmt, n, M), [&](auto f, const QBlock& b) {
    constexpr int FMT = decltype(f)::value;
    if (rw != nullptr)
      return dispatch_passnv<FMT, true>(cfg, [&](auto* kernel, int threads) {
        return q_launch(kernel, dim3(grid), threads, lds, s, b.hi, b.ldk, b.lo, b.ldlo, b.n, b.M, nv, V, ldv, slab, slab_ld, *rw);
      });
    return dispatch_passnv<FMT, false>(cfg, [&](auto* kernel, int threads) {
      return q_launch(kernel, dim3(grid), threads, lds, s, b.hi, b.ldk, b.lo, b.ldlo, b.n, b.M, nv, V, ldv, slab, slab_ld);
    });
  }));
  ODX_CHECK_LAUNCH(who);
  return reduce_nv(nv, M, grid, slab, slab_ld, out, ldo, s);
}

}  // namespace odx

using namespace odx;

extern "C" int64_t odx_knm_fwd_bwdn_q_workspace_bytes(int64_t n, int64_t M, int fmt, int nv) {
  return passnv_workspace_bytes(n, M, fmt, nv, 3);
}

extern "C" int odx_knm_fwd_bwdn_q(const void* K, int64_t ldk, const void* Klo, int64_t ldlo, int fmt, int64_t n, int64_t M, int nv,
                                  const double* V, int64_t ldv, double* out, int64_t ldo, void* workspace, int64_t workspace_bytes,
                                  odx_stream_t stream) {
  return passnv_run("odx_knm_fwd_bwdn_q", 3, K, ldk, Klo, ldlo, fmt, n, M, nv, V, ldv, out, ldo, nullptr, workspace, workspace_bytes,
                    stream);
}

extern "C" int64_t odx_knm_fwd_bwdn_q_rw_workspace_bytes(int64_t n, int64_t M, int fmt, int nv) {
  return passnv_workspace_bytes(n, M, fmt, nv, 1);
}

extern "C" int odx_knm_fwd_bwdn_q_rw(const void* K, int64_t ldk, const void* Klo, int64_t ldlo, int fmt, int64_t n, int64_t M, int nv,
                                     const double* V, int64_t ldv, const double* D, int64_t ldd, const int32_t* wrow, double* out,
                                     int64_t ldo, double* T_out, int64_t ldt, void* workspace, int64_t workspace_bytes,
                                     odx_stream_t stream) {
  const char* who = "odx_knm_fwd_bwdn_q_rw";
  ODX_REQUIRE(nv >= 1 && nv <= 8 && wrow != nullptr, "%s: nv outside 1 .. 8, or no wrow", who);
  NvRows rw = {D, ldd, {-1, -1, -1, -1, -1, -1, -1, -1}, T_out, ldt};
  bool weighted = false;
  for (int q = 0; q < nv; ++q) {
    rw.w[q] = wrow[q] < 0 ? -1 : (int)wrow[q];
    weighted = weighted || rw.w[q] >= 0;
  }
  ODX_REQUIRE(!weighted || (D != nullptr && ldd % 2 == 0 && ldd >= n), "%s: D must be rows of n weights, an even ldd >= n apart", who);
  ODX_REQUIRE(T_out == nullptr || ldt >= n, "%s: T_out must be rows of n doubles, ldt >= n apart", who);
  return passnv_run(who, 1, K, ldk, Klo, ldlo, fmt, n, M, nv, V, ldv, out, ldo, &rw, workspace, workspace_bytes, stream);
}
