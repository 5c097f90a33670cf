// The row-weighted pass over an f32-format K_nM block:  out = K' (d o (K v))  from ONE read of K — the Hessian product of a
// Newton step on a loss over the rows (odx/logistic.py: d = the loss's second derivatives), which the two-call route
// ktk(v, t_out), ktk(w = d o t) reads twice.
//
// The scheme is knm_pass.hip's, one vector: a persistent workgroup streams blocks of R rows; thread t owns the float4 column
// chunks t, t + NT, ... (CH of them) of every row and keeps their running column sums in f64 registers beside the R x CH
// float4 of the current block; v sits in LDS as f64.  Phase 1 forms the R row dots and reduces them over the workgroup (wave
// shuffles + one LDS exchange, ping-pong buffers: one barrier per block); phase 2 adds K[r, cols] t_r into the column sums
// and, chunk by chunk, re-issues the loads of the NEXT block into the registers it has just finished with.  Each workgroup
// writes its column sums as one slab and knm_pass.hip's fixed-order reducer adds the slabs: no atomics, bitwise reproducible.
//
// The weight, as in knm_pass_nv.hip's weighted form: between the phases lane r < R of every wave adds the waves' partials of
// row dot r (in wave order, the order knm_pass.hip adds them in), so a row dot is ONE value in one lane.  That lane loads the
// row's weight ahead of phase 1, which covers the latency, wave 0 stores the unweighted value to t_out, the lane multiplies
// once, and the products go out to the wave as uniform scalars (v_readlane): no per-thread weights, and the row dots leave
// the vector registers.  d == NULL multiplies with 1.0, which is exact: the same bits as a vector of ones.
//
// Requirements as for odx_knm_fwd_bwd: ldk % 4 == 0, K 16-byte aligned, columns [M, roundup(M, 4)) of K are zero.  Nothing
// is read past row n - 1 or past column roundup(M, 4) - 1 of a row.
#include "odx_internal.h"

namespace odx {

typedef float f32x4rw __attribute__((ext_vector_type(4)));
typedef double f64x2rw __attribute__((ext_vector_type(2)));

template <int NT, int CH, int R>
__global__ __launch_bounds__(NT) void knm_pass_rw_kernel(const float* __restrict__ K, int64_t ldk, int64_t n, int64_t M,
                                                         const double* __restrict__ v, const double* __restrict__ d,
                                                         double* __restrict__ slab, int64_t slab_ld,
                                                         double* __restrict__ t_out) {
  constexpr int NW = NT / 64;
  constexpr int VCAP = (NT * CH * 4 < 20000) ? NT * CH * 4 : 20000;  // 160,000 B of the 163,840 B LDS at most
  constexpr bool VFULL = NT * CH * 4 <= VCAP;                        // v zero-filled up to every chunk a thread walks
  static_assert(R <= 64, "a row dot per lane between the phases");
  __shared__ __attribute__((aligned(16))) double vs[VCAP];
  __shared__ double red[2][NW][R];
  const int64_t wg = blockIdx.x, nwg = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t nchunk = (M + 3) >> 2;
  const int64_t nblk = (n + R - 1) / R;

  for (int i = tid; i < VCAP; i += NT) vs[i] = i < M ? v[i] : 0.0;

  double acc[CH][4];
  bool cvalid[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    cvalid[c] = (tid + (int64_t)c * NT) < nchunk;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[c][e] = 0.0;
  }

  // Loads are unconditional, as in knm_pass.hip: a row past n is read as row n - 1 and its row dot is set to zero before
  // phase 2; a chunk past the row's end is read as the thread's chunk 0 — it meets zeros of v in phase 1 (VFULL; otherwise
  // the guard on v stays) and its column sums are never stored.
  f32x4rw kr[R][CH];
  uint32_t kcol[CH];       // element offset of the thread's chunk inside a row (32 bits; the row base is wave-uniform)
#pragma unroll
  for (int c = 0; c < CH; ++c) kcol[c] = cvalid[c] ? (uint32_t)(tid + c * NT) * 4u : 0u;
  auto load_block = [&](int64_t blk, int c) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = blk * R + r < n ? blk * R + r : n - 1;
      const float* rowp = K + row * ldk;
      kr[r][c] = *reinterpret_cast<const f32x4rw*>(rowp + kcol[c]);
    }
  };

  int64_t blk = wg;
  if (blk < nblk) {
#pragma unroll
    for (int c = 0; c < CH; ++c) load_block(blk, c);
  }
  __syncthreads();  // vs is complete
  int pp = 0;
  for (; blk < nblk; blk += nwg) {
    // lane r < R of every wave ends phase 1 with row dot r in `s` below: it loads that row's weight here; the other lanes,
    // rows past n and a call without weights keep 1.0 and load nothing
    double wgt = 1.0;
    {
      // (an opaque lane index: the address is formed here, block by block, not kept in registers for the whole loop)
      int ln;
      asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
      const int64_t row = blk * R + ln;
      if (d != nullptr && ln < R && row < n) wgt = d[row];
    }
    // phase 1: row dots
    double t[R];
#pragma unroll
    for (int r = 0; r < R; ++r) t[r] = 0.0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      double vv[4] = {0.0, 0.0, 0.0, 0.0};
      if (VFULL || cvalid[c]) {
        const f64x2rw a = *reinterpret_cast<const f64x2rw*>(&vs[(tid + c * NT) * 4]);
        const f64x2rw b = *reinterpret_cast<const f64x2rw*>(&vs[(tid + c * NT) * 4 + 2]);
        vv[0] = a[0]; vv[1] = a[1]; vv[2] = b[0]; vv[3] = b[1];
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) t[r] = fma((double)kr[r][c][e], vv[e], t[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double s = t[r];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (lane == 0) red[pp][wave][r] = s;
    }
    __syncthreads();
    {
      // every wave adds the waves' partials of row dot `lane` in wave order; wave 0 stores K v as it is, then the weight, once
      double s = 0.0;
      const int vi = lane < R ? lane : 0;
#pragma unroll
      for (int u = 0; u < NW; ++u) s += red[pp][u][vi];
      const int64_t row = blk * R + lane;
      if (t_out != nullptr && wave == 0 && lane < R && row < n) t_out[row] = s;
      s *= wgt;
      const int slo = __double2loint(s), shi = __double2hiint(s);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double tot = __hiloint2double(__builtin_amdgcn_readlane(shi, r), __builtin_amdgcn_readlane(slo, r));
        t[r] = blk * R + r < n ? tot : 0.0;      // (the last block only) a repeated row, not a zero one, was read for it
      }
    }
    pp ^= 1;
    // the doubles phase 1 converted the block to must not stay live into phase 2 (R x CH x 4 of them: spills); an empty asm
    // makes the f32 registers opaque here, phase 2 converts again
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int r = 0; r < R; ++r) asm volatile("" : "+v"(kr[r][c]));
    // phase 2: column sums, and the next block's loads re-issued chunk by chunk (unconditionally — behind the last block
    // they re-read it and nobody waits for them: a branch around them makes every register of the block a loop-carried select)
    const int64_t nxt = blk + nwg < nblk ? blk + nwg : blk;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c][e] = fma((double)kr[r][c][e], t[r], acc[c][e]);
      load_block(nxt, c);
      __builtin_amdgcn_sched_barrier(0);      // the loads of chunk column c go into the registers just consumed, not ahead of them
    }
  }
  double* my = slab + wg * slab_ld;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int64_t ch = tid + (int64_t)c * NT;
    if (cvalid[c]) {
#pragma unroll
      for (int e = 0; e < 4; ++e) my[ch * 4 + e] = acc[c][e];
    }
  }
}

// The configurations of odx_knm_fwd_bwd (knm_pass.hip, pick_cfg), restated: the entry's workspace is that entry's, so the
// workgroups per CU must be the same ones, and the same (threads, chunks, rows) keep the measured streaming behaviour.
struct RwCfg {
  int nt, ch, r, wg_per_cu;
};

static bool pick_rwcfg(int64_t M, RwCfg* cfg) {
  const int64_t chunks = (M + 3) / 4;
  if (chunks <= 256) { *cfg = {256, 1, 16, 2}; return true; }
  if (chunks <= 512) { *cfg = {256, 2, 8, 2}; return true; }
  if (chunks <= 1024) { *cfg = {256, 4, 4, 2}; return true; }
  if (chunks <= 2048) { *cfg = {512, 4, 4, 1}; return true; }
  if (chunks <= 2560) { *cfg = {512, 5, 4, 1}; return true; }
  if (chunks <= 3072) { *cfg = {512, 6, 2, 1}; return true; }
  if (chunks <= 5000) { *cfg = {1024, 5, 1, 1}; return true; }
  return false;
}

}  // namespace odx

using namespace odx;

#define ODX_PASS_RW_LAUNCH(NT_, CH_, R_)                                                                                \
  hipLaunchKernelGGL((knm_pass_rw_kernel<NT_, CH_, R_>), dim3(grid), dim3(NT_), 0, s, K, ldk, n, M, v, d, slab, slab_ld, \
                     t_out)

extern "C" int odx_knm_fwd_bwd_rw(const float* K, int64_t ldk, int64_t n, int64_t M, const double* v, const double* d,
                                  double* out, double* t_out, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  ODX_REQUIRE(M > 0 && out, "odx_knm_fwd_bwd_rw: M <= 0 or null out");
  hipStream_t s = as_stream(stream);
  if (n <= 0) {
    ODX_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)M * sizeof(double), s));
    return ODX_OK;
  }
  ODX_REQUIRE(K && v, "odx_knm_fwd_bwd_rw: null K or v");
  ODX_REQUIRE(ldk % 4 == 0 && ldk >= round_up(M, 4) && aligned16(K),
              "odx_knm_fwd_bwd_rw: K must be 16-byte aligned, ldk %% 4 == 0, ldk >= roundup(M, 4)");
  RwCfg cfg;
  if (!pick_rwcfg(M, &cfg)) {
    set_error("odx_knm_fwd_bwd_rw: M = %lld exceeds the 20000 columns the pass kernels are built for", (long long)M);
    return ODX_ERR_UNSUPPORTED;
  }
  // odx_knm_fwd_bwd's grid on the WHOLE device: a slab per workgroup, within odx_knm_fwd_bwd_workspace_bytes(n, M).  The CUs
  // odx_set_pass_reserved_cus leaves to concurrent streams are NOT left out here (the count is knm_pass.hip's own): a Newton
  // step runs no chain beside its passes
  int cus = odx_device_cus();
  if (cus <= 0) cus = 256;
  const int64_t nblk = ceil_div(n, cfg.r);
  int64_t g = (int64_t)cus * cfg.wg_per_cu;
  if (g > nblk) g = nblk;
  const int grid = (int)(g < 1 ? 1 : g);
  const int64_t slab_ld = round_up(M, 4);
  if (workspace == nullptr || workspace_bytes < (int64_t)grid * slab_ld * (int64_t)sizeof(double)) {
    set_error("odx_knm_fwd_bwd_rw: workspace too small (%lld < %lld)", (long long)workspace_bytes,
              (long long)((int64_t)grid * slab_ld * (int64_t)sizeof(double)));
    return ODX_ERR_WORKSPACE;
  }
  double* slab = static_cast<double*>(workspace);
  if (cfg.nt == 256 && cfg.ch == 1) ODX_PASS_RW_LAUNCH(256, 1, 16);
  else if (cfg.nt == 256 && cfg.ch == 2) ODX_PASS_RW_LAUNCH(256, 2, 8);
  else if (cfg.nt == 256 && cfg.ch == 4) ODX_PASS_RW_LAUNCH(256, 4, 4);
  else if (cfg.nt == 512 && cfg.ch == 4) ODX_PASS_RW_LAUNCH(512, 4, 4);
  else if (cfg.nt == 512 && cfg.ch == 5) ODX_PASS_RW_LAUNCH(512, 5, 4);
  else if (cfg.nt == 512 && cfg.ch == 6) ODX_PASS_RW_LAUNCH(512, 6, 2);
  else ODX_PASS_RW_LAUNCH(1024, 5, 1);
  ODX_CHECK_LAUNCH("odx_knm_fwd_bwd_rw");
  return slab_reduce_f64(slab, slab_ld, grid, M, out, s);
}
