// out[r * ldo] = (float) sum_j K[r, j] alpha[j] over a STORED K_nM block (odx_knm_mv): the scores of a fitted class from the
// block its CG passes streamed, instead of a second Gaussian contraction (odx_gauss_mmv_h2: 2 n M D flop on the matrix
// cores).  One read of the block — the traffic of one CG pass, HBM-bound — in any of the three storage formats of
// odx_gauss_knm_h2_store: f32, 24-bit fixed point (u16 + u8 planes) and bf16.
//
// It is the CG pass's phase 1 alone (knm_pass_q.hip): alpha in LDS as f64 (the 2^-24 of the fixed-point scale folded in),
// row dots in f64.  Without the pass's column sums nothing needs the whole workgroup: each WAVE owns groups of R rows and
// walks them over all columns by itself — lane l holds the 4-column chunks l, l + 64, ... of each row, CH chunk columns of
// R rows at a time in registers as loaded — and finishes a row group with a butterfly over its 64 lanes.  No slab, no
// workspace, no barrier after alpha is in LDS; every sum is formed in a fixed order (bitwise reproducible).  The loads of
// the next tile (the next chunk columns of the group, or the first ones of the wave's next group) are issued chunk by chunk
// as the current tile's registers are consumed, so R x CH loads per wave stay in flight.
//
// Addressing as in the pass kernels: one buffer descriptor per plane and row group (base = the group's first row, length =
// the bytes of its rows that exist), a per-lane 32-bit offset (the chunk inside a chunk column) and a scalar one (row inside
// the group, chunk column).  The hardware range check reads rows past n as zero and a group past the last as nothing at all
// (zero length).  A chunk past the row's end (the last chunk column) reads the start of the next row: it meets the zero
// chunk behind alpha in LDS.
#include <algorithm>

#include "odx_internal.h"

namespace odx {

typedef unsigned int u32x4m __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2m __attribute__((ext_vector_type(2)));
typedef double f64x2m __attribute__((ext_vector_type(2)));

constexpr int MV_NT = 512;           // threads per workgroup: 8 waves sharing one copy of alpha
constexpr int MV_R = 2;              // rows per wave and tile
constexpr int MV_OVERSUB = 4;        // workgroups per resident slot: a CU held by another stream's work delays a quarter

// A lane's chunk of 4 entries: f32 w[0..3]; u24 w[0..1] = the u16 pairs, w[2] = the four low bytes; bf16 w[0..1].
template <int FMT>
__device__ __forceinline__ double mv_entry(const unsigned (&k)[4], int e) {
  if (FMT == ODX_KNM_F32) return (double)__uint_as_float(k[e]);
  const unsigned h = k[e >> 1];
  if (FMT == ODX_KNM_U24) {
    // v_perm_b32: [low byte e of the second source | u16 (e & 1) of the first << 8], the top byte zero (0x0c)
    const unsigned sel = ((e & 1) ? 0x0c070600u : 0x0c050400u) | (unsigned)(e & 3);
    return (double)__builtin_amdgcn_perm(h, k[2], sel);
  }
  return (double)__uint_as_float((e & 1) ? (h & 0xffff0000u) : (h << 16));
}

template <int FMT, int R, int CH>
__global__ __launch_bounds__(MV_NT, 2) void knm_mv_kernel(const void* __restrict__ K, int64_t ldk,
                                                          const unsigned char* __restrict__ Klo, int64_t ldlo, int64_t n,
                                                          int64_t M, const double* __restrict__ alpha, float* __restrict__ out,
                                                          int64_t ldo) {
  constexpr int NW = MV_NT / 64;
  constexpr int HB = FMT == ODX_KNM_F32 ? 16 : 8;      // bytes of a chunk in the main plane (the u8 plane: 4)
  extern __shared__ __attribute__((aligned(16))) double av[];    // [(nchunk + 1) * 4]: alpha, then one chunk of zeros
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (wave-uniform: keeps the descriptors in SGPRs)
  const int nchunk = (int)((M + 3) / 4);
  const double scale = FMT == ODX_KNM_U24 ? 5.9604644775390625e-08 : 1.0;      // 2^-24 (exact)
  for (int i = tid; i < (nchunk + 1) * 4; i += MV_NT) av[i] = i < M ? alpha[i] * scale : 0.0;
  __syncthreads();

  const int nset = (int)((nchunk + 64 * CH - 1) / (64 * CH));  // tiles of CH chunk columns per row group
  const int64_t ngrp = (n + R - 1) / R;
  const int64_t gstep = (int64_t)gridDim.x * NW;
  const int rowb = (int)ldk * (HB / 4), rowb_lo = (int)ldlo;
  const int voff = lane * HB, voff_lo = lane * 4;
  auto open = [&](int64_t g, __amdgpu_buffer_rsrc_t& a, __amdgpu_buffer_rsrc_t& b) {
    const int64_t row0 = g * R;
    const int rows = (row0 >= 0 && row0 < n) ? (int)(n - row0 < R ? n - row0 : R) : 0;      // 0: nothing is read
    a = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(K)) + row0 * rowb, (short)0, rows * rowb, 0x00020000);
    if (FMT == ODX_KNM_U24)
      b = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(Klo) + row0 * ldlo, (short)0, rows * rowb_lo, 0x00020000);
  };
  unsigned kr[R][CH][4];
  auto load = [&](const __amdgpu_buffer_rsrc_t& a, const __amdgpu_buffer_rsrc_t& b, int s, int c) {
    const int col = s * CH + c;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (FMT == ODX_KNM_F32) {
        const u32x4m w = __builtin_amdgcn_raw_buffer_load_b128(a, voff, r * rowb + col * (64 * HB), 0);
        kr[r][c][0] = w[0], kr[r][c][1] = w[1], kr[r][c][2] = w[2], kr[r][c][3] = w[3];
      } else {
        const u32x2m w = __builtin_amdgcn_raw_buffer_load_b64(a, voff, r * rowb + col * (64 * HB), 0);
        kr[r][c][0] = w[0], kr[r][c][1] = w[1];
        if (FMT == ODX_KNM_U24) kr[r][c][2] = __builtin_amdgcn_raw_buffer_load_b32(b, voff_lo, r * rowb_lo + col * 256, 0);
      }
    }
  };

  // The loop starts on a tile of zeros "before" the wave's first group (group g0 - gstep, last chunk columns): every load
  // is then issued at ONE place, into the same registers each trip, and each chunk's first use waits for its own loads
  // only (loads issued ahead of the loop land in other registers, and the wait at the loop's head becomes vmcnt(0))
  int64_t g = (int64_t)blockIdx.x * NW + wave - gstep;
  int s = nset - 1;
  __amdgpu_buffer_rsrc_t ra, rb;
  open(-1, ra, rb);
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int u = 0; u < 4; ++u) kr[r][c][u] = 0u;
  double t[R];
#pragma unroll
  for (int r = 0; r < R; ++r) t[r] = 0.0;
  while (g < ngrp) {
    int64_t gn = g;
    int sn = s + 1;
    __amdgpu_buffer_rsrc_t na = ra, nb = rb;
    if (sn == nset) {
      gn = g + gstep, sn = 0;
      open(gn, na, nb);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = lane + (s * CH + c) * 64;
      const int vi = (ch < nchunk ? ch : nchunk) * 4;
      const f64x2m a01 = *reinterpret_cast<const f64x2m*>(&av[vi]);
      const f64x2m a23 = *reinterpret_cast<const f64x2m*>(&av[vi + 2]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        t[r] = fma(mv_entry<FMT>(kr[r][c], 0), a01[0], t[r]);
        t[r] = fma(mv_entry<FMT>(kr[r][c], 1), a01[1], t[r]);
        t[r] = fma(mv_entry<FMT>(kr[r][c], 2), a23[0], t[r]);
        t[r] = fma(mv_entry<FMT>(kr[r][c], 3), a23[1], t[r]);
      }
      // (unconditional: past the wave's last group the descriptor has zero length and the loads touch no memory)
      load(na, nb, sn, c);
      __builtin_amdgcn_sched_barrier(0);      // one chunk column's decoded entries at a time (register pressure)
    }
    if (sn == 0) {                            // the group's rows are complete
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double v = t[r];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        const int64_t row = g * R + r;
        if (lane == 0 && row >= 0 && row < n) out[row * ldo] = (float)v;
        t[r] = 0.0;
      }
    }
    g = gn, s = sn, ra = na, rb = nb;
  }
}

// R x CH = 16 chunk loads in flight per wave (48 VGPRs of them for u24, 64 for f32; no spills), 16 waves per
// CU at two workgroups (alpha of M <= ~10 200 twice in LDS)
template <int FMT>
static int launch_mv(int grid, size_t lds, hipStream_t s, const void* K, int64_t ldk, const unsigned char* Klo, int64_t ldlo,
                     int64_t n, int64_t M, const double* alpha, float* out, int64_t ldo) {
  constexpr int CH = 8;
  ODX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(knm_mv_kernel<FMT, MV_R, CH>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((knm_mv_kernel<FMT, MV_R, CH>), dim3(grid), dim3(MV_NT), lds, s, K, ldk, Klo, ldlo, n, M, alpha, out, ldo);
  return ODX_OK;
}

}  // namespace odx

using namespace odx;

extern "C" int odx_knm_mv(const void* K, int64_t ldk, const void* Klo, int64_t ldlo, int fmt, int64_t n, int64_t M,
                          const double* alpha, float* out, int64_t ldo, odx_stream_t stream) {
  ODX_REQUIRE(fmt == ODX_KNM_F32 || fmt == ODX_KNM_U24 || fmt == ODX_KNM_BF16, "odx_knm_mv: unknown storage format %d", fmt);
  ODX_REQUIRE(n >= 0 && M > 0 && alpha && out && ldo >= 1, "odx_knm_mv: n < 0, M <= 0, null alpha / out or ldo < 1");
  if (n == 0) return ODX_OK;
  const size_t lds = (size_t)((M + 3) / 4 + 1) * 4 * sizeof(double);
  ODX_REQUIRE(lds <= 163840, "odx_knm_mv: M = %lld exceeds the 20476 centres whose alpha fits in LDS", (long long)M);
  const int per = fmt == ODX_KNM_F32 ? 4 : 2;      // bytes per entry of the main plane
  ODX_REQUIRE(K && ldk % 4 == 0 && ldk >= round_up(M, 4) && (reinterpret_cast<uintptr_t>(K) & (fmt == ODX_KNM_F32 ? 15u : 7u)) == 0,
              "odx_knm_mv: K must be %d-byte aligned with ldk %% 4 == 0, ldk >= roundup(M, 4)", fmt == ODX_KNM_F32 ? 16 : 8);
  ODX_REQUIRE(2 * ldk * per < (int64_t)1 << 30, "odx_knm_mv: row stride too large");
  if (fmt == ODX_KNM_U24)
    ODX_REQUIRE(Klo && ldlo % 4 == 0 && ldlo >= round_up(M, 4) && ldlo < ((int64_t)1 << 28) && (reinterpret_cast<uintptr_t>(Klo) & 3u) == 0,
                "odx_knm_mv: the low-byte plane must be 4-byte aligned with ldlo %% 4 == 0, ldlo >= roundup(M, 4)");
  hipStream_t s = as_stream(stream);
  int cus = odx_device_cus();
  if (cus <= 0) cus = 256;
  const int64_t per_cu = std::min<int64_t>(2, std::max<int64_t>(1, 163840 / (int64_t)lds));
  const int64_t need = ceil_div(ceil_div(n, MV_R), MV_NT / 64);          // workgroups that give every wave one row group
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(need, cus * per_cu * MV_OVERSUB));
  const unsigned char* lo = static_cast<const unsigned char*>(Klo);
  if (fmt == ODX_KNM_U24) ODX_PROPAGATE(launch_mv<ODX_KNM_U24>(grid, lds, s, K, ldk, lo, ldlo, n, M, alpha, out, ldo));
  else if (fmt == ODX_KNM_F32) ODX_PROPAGATE(launch_mv<ODX_KNM_F32>(grid, lds, s, K, ldk, nullptr, 0, n, M, alpha, out, ldo));
  else ODX_PROPAGATE(launch_mv<ODX_KNM_BF16>(grid, lds, s, K, ldk, nullptr, 0, n, M, alpha, out, ldo));
  ODX_CHECK_LAUNCH("odx_knm_mv");
  return ODX_OK;
}
