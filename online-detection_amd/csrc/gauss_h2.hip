// Gaussian-kernel blocks with the -2 X Z' contraction on the f16 matrix cores (gfx950), at f32 accuracy.
//
// Every f32 operand value is split once into two f16 terms, x * s = hi + lo (s a power of two that puts
// max |x| into [2^13, 2^14)): hi carries the top 11 significant bits, lo the next 11.  Then
//     x . z  =  (hi_x . hi_z  +  hi_x . lo_z  +  lo_x . hi_z) / (s_x s_z)   (+ a lo.lo term of relative size 2^-22)
// Each f16 x f16 product is exact in f32 and v_mfma_f32_16x16x32_f16 accumulates in f32, so the contraction
// keeps ~22 bits per factor — tools/precision_study.py: the fitted alpha moves exactly as with the all-f32
// v_mfma_f32_32x32x2_f32 chain — at 3 MFMAs of the f16 rate (16 x the f32 MFMA rate) per f32 MFMA replaced.
//
// Packed operand ("h2") layout, produced by odx_split_f16: a row is ldp 4-byte units; granule t of a row
// (32 consecutive features) is 128 contiguous, 128-byte aligned bytes — one cache line: 32 f16 hi, then 32 f16 lo.
// Features past D are zero; ldp covers a whole number of 64-feature pairs of granules.
// Two tile cores read it:
//   "s16"  128 x 128 outputs, 256 threads (2 x 2 waves of 64 x 64), k-tile = two granules through XOR-swizzled 256-B
//          LDS rows, two workgroups per CU.  Draws (128 + 128) x 4 B of operand per k from L2 for 128 x 128 products:
//          at the headline shapes that is 10.7 TB/s of L2 -> LDS traffic and the L2, not the MFMA, sets its pace
//          (with two of the three MFMAs removed it still takes 68 % of its time).  Kept for small problems.
//   "w256" 256 x 256 outputs, 512 threads (2 x 4 waves of 128 x 64), k-stage = one granule through XOR-swizzled 128-B
//          LDS rows, double-buffered (2 x 64 KiB), one barrier per stage, one workgroup per CU: half the L2 traffic
//          per product.
#include <stdlib.h>
#include <type_traits>
#include "gemm_core.h"
#include "odx_internal.h"

namespace odx {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int H2_KT = 64;                   // features per k-tile

// ---------------------------------------------------------------- split
__global__ __launch_bounds__(256) void absmax_f32_kernel(const float* __restrict__ X, int64_t ldx, int64_t n, int D,
                                                         unsigned int* __restrict__ out) {
  unsigned int m = 0;
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
    const float* x = X + r * ldx;
    // ldx % 4 == 0 and X 16-byte aligned (checked by the caller).  Four 16-byte loads of a lane are issued before the
    // first is consumed: with one load in flight per wave a 2000-row call took 52 us for 32 MB.
    for (int c0 = lane * 4; c0 < D; c0 += 1024) {
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + 256 * u;
        v[u] = (c < D) ? *reinterpret_cast<const u32x4*>(x + c) : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c0 + 256 * u + q < D) m = max(m, v[u][q] & 0x7fffffffu);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, off));
  // one atomic per workgroup: with one per wave (one wave per row) a 2000-row call spent its 27 us queueing 2000 atomics
  // on one address
  __shared__ unsigned int wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
    if (m) atomicMax(out, m);
  }
}

// The two meta words of a matrix are cleared by a KERNEL, not by hipMemsetAsync: these calls are captured into HIP graphs (the
// feature forward), and a graph's memset nodes were not reliably ordered against the kernel nodes around them on this runtime —
// a forward replayed from the harvest loop's second thread now and then cleared the words AFTER the packing kernel had left its
// scale there (scale 0 -> 1 / 0 in the next product -> NaN -> an all-zero map behind the ReLU, for as long as the timing held).
__global__ void meta_zero_kernel(float* __restrict__ meta) {
  if (threadIdx.x < 2) meta[threadIdx.x] = 0.f;
}

// scale = 2^(13 - e) for absmax = 1.m x 2^e  (1 for an all-zero, denormal or non-finite matrix)
__device__ __forceinline__ float h2_scale_from_absmax(unsigned int bits) {
  const int ef = (int)((bits >> 23) & 0xffu);
  if (ef == 0 || ef == 255) return 1.f;
  int se = 127 + 13 - (ef - 127);
  se = se < 1 ? 1 : (se > 254 ? 254 : se);
  return __uint_as_float((unsigned int)se << 23);
}

__global__ __launch_bounds__(256) void split_f16_kernel(const float* __restrict__ X, int64_t ldx, int64_t n, int D,
                                                        uint32_t* __restrict__ P, int64_t ldp, float* __restrict__ meta) {
  const float s = h2_scale_from_absmax(__float_as_uint(meta[1]));
  if (blockIdx.x == 0 && threadIdx.x == 0) meta[0] = s;
  if (n <= 0) return;
  const int groups = (int)((D + H2_KT - 1) / H2_KT) * 8;  // 8-feature groups per row, zero padded to whole k-tiles
  // a flat index over (row, group): with one workgroup per row a 64-channel activation kept 8 of its 256 lanes busy
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / groups;
  const int g = (int)(idx - row * groups);
  if (row >= n) return;
  const float* x = X + row * ldx + (int64_t)g * 8;
  float v[8];
  if (g * 8 + 8 <= D) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x), b = *reinterpret_cast<const f32x4*>(x + 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) { v[q] = a[q]; v[4 + q] = b[q]; }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = (g * 8 + q < D) ? x[q] : 0.f;
  }
  f16x8 hi, lo;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float t = v[q] * s;
    const _Float16 h = (_Float16)t;
    hi[q] = h;
    lo[q] = (_Float16)(t - (float)h);
  }
  uint32_t* dst = P + row * ldp + (int64_t)(g >> 2) * 32 + (g & 3) * 4;   // 4-byte units: granule, 16-B chunk
  *reinterpret_cast<f16x8*>(dst) = hi;
  *reinterpret_cast<f16x8*>(dst + 16) = lo;
}

// The packed split of the 3 x 3 neighbourhood matrix of an NHWC row matrix Y (R * H * W rows of C channels): row (r, h, w)
// of the result holds, tap (ky, kx) after tap, the C channels of Y's row (r, h + ky - 1, w + kx - 1) — zeros outside the
// map.  That is the operand of a 3 x 3 convolution (padding 1) run as a GEMM; it is written in the packed form directly,
// never as floats (9 x the bytes of Y).  C % 8 == 0; the scale comes from Y's own absmax (the zeros add nothing).
__global__ __launch_bounds__(256) void split_f16_taps3x3_kernel(const float* __restrict__ Y, int64_t ldy, int H, int W, int C,
                                                                uint32_t* __restrict__ P, int64_t ldp, float* __restrict__ meta,
                                                                int64_t nrows) {
  const float s = h2_scale_from_absmax(__float_as_uint(meta[1]));
  if (blockIdx.x == 0 && threadIdx.x == 0) meta[0] = s;
  const int D = 9 * C;
  const int groups = (int)((D + H2_KT - 1) / H2_KT) * 8;
  // a flat index over (row, 8-feature group): with the rows on grid.y a 64-channel layer (72 groups) kept 72 of a workgroup's
  // 256 lanes busy and a trunk stage of 120 000 rows needed two launches
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / groups;
  const int g = (int)(idx - row * groups);
  if (row >= nrows) return;
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = 0.f;
  const int f = g * 8;                                   // first feature of the group: tap f / C, channel f % C
  if (f < D) {
    const int tap = f / C, c = f - tap * C;
    const int w = (int)(row % W), h = (int)((row / W) % H);
    const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
    if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
      const float* x = Y + (row + (int64_t)(hh - h) * W + (ww - w)) * ldy + c;
      const f32x4 a = *reinterpret_cast<const f32x4*>(x), b = *reinterpret_cast<const f32x4*>(x + 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) { v[q] = a[q]; v[4 + q] = b[q]; }
    }
  }
  f16x8 hi, lo;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float t = v[q] * s;
    const _Float16 hq = (_Float16)t;
    hi[q] = hq;
    lo[q] = (_Float16)(t - (float)hq);
  }
  uint32_t* dst = P + row * ldp + (int64_t)(g >> 2) * 32 + (g & 3) * 4;
  *reinterpret_cast<f16x8*>(dst) = hi;
  *reinterpret_cast<f16x8*>(dst + 16) = lo;
}

// The same neighbourhood matrix from rows that are ALREADY packed (a chain layer's output, H2PackOut): a gather of 16-byte
// pieces — feature group g of tap t comes from group (g's channels) of the neighbour's row, hi and lo pieces alike; same scale.
__global__ __launch_bounds__(256) void taps3x3_packed_kernel(const uint32_t* __restrict__ PY, int64_t ldpy, int H, int W, int C,
                                                             uint32_t* __restrict__ P, int64_t ldp, int64_t nrows) {
  const int D = 9 * C;
  const int groups = (int)((D + H2_KT - 1) / H2_KT) * 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / groups;
  const int g = (int)(idx - row * groups);
  if (row >= nrows) return;
  u32x4 hi = {0u, 0u, 0u, 0u}, lo = {0u, 0u, 0u, 0u};
  const int f = g * 8;
  if (f < D) {
    const int tap = f / C, c = f - tap * C;
    const int w = (int)(row % W), h = (int)((row / W) % H);
    const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
    if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
      const int gs = c >> 3;
      const uint32_t* src = PY + (row + (int64_t)(hh - h) * W + (ww - w)) * ldpy + (int64_t)(gs >> 2) * 32 + (gs & 3) * 4;
      hi = *reinterpret_cast<const u32x4*>(src);
      lo = *reinterpret_cast<const u32x4*>(src + 16);
    }
  }
  uint32_t* dst = P + row * ldp + (int64_t)(g >> 2) * 32 + (g & 3) * 4;
  *reinterpret_cast<u32x4*>(dst) = hi;
  *reinterpret_cast<u32x4*>(dst + 16) = lo;
}

// ---------------------------------------------------------------- tile mainloop
struct H2Stage {
  u32x4 a[8], b[8];
};

// Rows past the operand's end are read as its last row (never branch around a load: the eight loads of an operand
// issue back to back); whatever they produce is masked in the epilogues.  voff: per-thread 32-bit offsets (4-byte
// units) from the uniform tile base, so the loads take the scalar-base + vector-offset form.
// PERM (the B operand of the plain products): LDS row 64 b + 16 t + i of the image holds operand row 64 b + 4 i + t, so that the
// four accumulator blocks tn = 0..3 of a lane are four ADJACENT output columns 64 wc + 4 (lane & 15) + tn (as on the wide
// core, w_dma_offsets<true>): the epilogue moves 16 bytes per lane instead of four scattered floats.
template <bool PERM = false>
__device__ __forceinline__ void h2_row_offsets(uint32_t (&voff)[8], int64_t ld, int64_t row0, int64_t nrows) {
  const int tid = threadIdx.x;
  const int last = (int)(nrows - 1 - row0);          // >= 0: the tile starts inside the operand
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int ri = (tid >> 4) + 16 * p;
    const int r = PERM ? ((ri & ~63) | ((ri & 15) << 2) | ((ri >> 4) & 3)) : ri;
    voff[p] = (uint32_t)(r < last ? r : last) * (uint32_t)ld + (uint32_t)(tid & 15) * 4u;
  }
}

__device__ __forceinline__ void h2_load_operand(u32x4 (&r)[8], const uint32_t* __restrict__ tile, const uint32_t (&voff)[8]) {
#pragma unroll
  for (int p = 0; p < 8; ++p) r[p] = *reinterpret_cast<const u32x4*>(tile + voff[p]);
}

__device__ __forceinline__ void s16_clear_stage(H2Stage& st) {
#pragma unroll
  for (int p = 0; p < 8; ++p) st.a[p] = st.b[p] = u32x4{0u, 0u, 0u, 0u};
}

constexpr float LOG2E = 1.4426950408889634f;

// ---------------------------------------------------------------- tile core
// v_mfma_f32_16x16x32_f16, 4 x 4 blocks per wave.  LDS rows are exactly 256 B (two granules) with the
// 16-byte slots of a row XOR-swizzled by (row & 15): logical slot q (granule ks: hi chunks 8 ks .. 8 ks + 3, lo chunks
// 8 ks + 4 .. 8 ks + 7) lives at q ^ (row & 15).  A 16-lane group of ds_read_b128 then touches lanes of two k-groups whose chunk numbers differ only in
// their low two bits, which keeps the 16 slots distinct (conflict-free), with no padding: 64 KiB per workgroup.
constexpr int S16_ROW = 256;
constexpr int S16_LDS_BYTES = (GEMM_BM + GEMM_BN) * S16_ROW;   // 65,536 B

__device__ __forceinline__ void s16_store_operand(const u32x4 (&r)[8], char* lds) {
  const int tid = threadIdx.x;
  const int row = tid >> 4;
  char* d = lds + row * S16_ROW + (((tid & 15) ^ (row & 15)) << 4);     // (row + 16 p) & 15 == row & 15
#pragma unroll
  for (int p = 0; p < 8; ++p) *reinterpret_cast<u32x4*>(d + 16 * p * S16_ROW) = r[p];
}

// CORE (declared with the wide core below): S16_H2 = two-term f16 splits, three MFMAs per product block; S16_BF16 / S16_F16 =
// plain 16-bit operands (a 256-byte LDS row is 128 features: the "hi" and "lo" chunks of a lane are simply two 8-feature
// pieces of its row, the same ones for A and B), two MFMAs per product block and k-group.
enum { S16_H2 = 0, S16_BF16 = 2, S16_F16 = 3 };
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <int CORE = S16_H2>
__device__ __forceinline__ void s16_compute_ktile(f32x4 (&acc)[4][4], const char* ldsA, const char* ldsB, int wr, int wc,
                                                  int lane) {
  const int r = lane & 15, g = lane >> 4;
  const char* pa = ldsA + (wr * 64 + r) * S16_ROW;
  const char* pb = ldsB + (wc * 64 + r) * S16_ROW;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int hi = (((ks * 8 + g) ^ r) << 4), lo = hi ^ 64;
    f16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      ah[t] = *reinterpret_cast<const f16x8*>(pa + t * 16 * S16_ROW + hi);
      al[t] = *reinterpret_cast<const f16x8*>(pa + t * 16 * S16_ROW + lo);
      bh[t] = *reinterpret_cast<const f16x8*>(pb + t * 16 * S16_ROW + hi);
      bl[t] = *reinterpret_cast<const f16x8*>(pb + t * 16 * S16_ROW + lo);
    }
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        if (CORE == S16_BF16) {
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah[tm]), __builtin_bit_cast(bf16x8, bh[tn]),
                                                                acc[tm][tn], 0, 0, 0);
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, al[tm]), __builtin_bit_cast(bf16x8, bl[tn]),
                                                                acc[tm][tn], 0, 0, 0);
        } else if (CORE == S16_F16) {
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[tm], bh[tn], acc[tm][tn], 0, 0, 0);
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[tm], bl[tn], acc[tm][tn], 0, 0, 0);
        } else {
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[tm], bh[tn], acc[tm][tn], 0, 0, 0);
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[tm], bl[tn], acc[tm][tn], 0, 0, 0);
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[tm], bh[tn], acc[tm][tn], 0, 0, 0);
        }
      }
  }
}

// The k-tile -> (tap, channel offset) cursor of a TAPS operand on this core: a k-tile is 64 channels of one tap (C % 64 == 0).
struct S16Tap {
  int kin, dy, dx;           // 4-byte units into the tap's channels; tap offset (ky - 1, kx - 1)
};
__device__ __forceinline__ S16Tap s16_tap_next(S16Tap c, int C) {
  c.kin += H2_KT;
  if (c.kin == C) {
    c.kin = 0;
    if (++c.dx == 2) {
      c.dx = -1;
      ++c.dy;
    }
  }
  return c;
}

// the eight row offsets (4-byte units from A) of this lane for one tap: the neighbour (h + dy, w + dx) of each of its rows, or
// the all-zero row behind the operand for a neighbour outside the map (hw: h << 16 | w, negative for a row past the end)
__device__ __forceinline__ void s16_tap_offsets(uint32_t (&off)[8], const uint32_t (&rowoff)[8], const int (&hw)[8], uint32_t zoff, int lda,
                                                int H, int W, const S16Tap& c) {
  const int shift = (c.dy * W + c.dx) * lda;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int h = hw[p] >> 16, w = hw[p] & 0xffff;
    const bool in = hw[p] >= 0 && (unsigned)(h + c.dy) < (unsigned)H && (unsigned)(w + c.dx) < (unsigned)W;
    off[p] = (in ? rowoff[p] + (uint32_t)shift : zoff) + (uint32_t)c.kin;
  }
}

// TAPS: A is the 3 x 3 neighbourhood matrix of the packed NHWC rows at A (m rows of tapC channels + one all-zero row), gathered in
// the operand loads as on the wide core (w_mainloop_dma): the eight row offsets of a lane are recomputed per k-tile.
// HALF (16-bit rows whose stride is a multiple of 64 features only, the Gaussian kernels' operand contract): with half_tail
// the LAST k-tile holds 64 features — 128 bytes — per row, and the lanes of the upper eight 16-byte slots must not read
// on into the next row (or past the operand's end).  They fetch the slot 128 bytes below their own instead, always inside
// the row, and stage zeros: no branch around a load, nothing out of bounds, and zeros add nothing to a product.
template <int CORE = S16_H2, bool PERMB = false, bool TAPS = false, bool HALF = false>
__device__ __forceinline__ void s16_mainloop(f32x4 (&acc)[4][4], const uint32_t* __restrict__ A, int64_t lda, int64_t m,
                                             const uint32_t* __restrict__ B, int64_t ldb, int64_t n, int64_t i0, int64_t j0,
                                             int ktiles, char* lds, int tapH = 0, int tapW = 0, int tapC = 0, bool half_tail = false) {
  static_assert(!HALF || (CORE != S16_H2 && !TAPS), "a half k-tile exists for plain 16-bit rows only");
  char* ldsA = lds;
  char* ldsB = lds + GEMM_BM * S16_ROW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  uint32_t offa[8], offb[8];
  h2_row_offsets<PERMB>(offb, ldb, j0, n);
  const uint32_t* ta = A + i0 * lda;
  const uint32_t* tb = B + j0 * ldb;
  int hw[8];
  uint32_t zoff = 0;
  S16Tap tc{0, -1, -1};
  if (TAPS) {
    const int tid = threadIdx.x;
    ta = A;                                               // offsets are absolute: a neighbour's row may lie in front of the tile
    zoff = (uint32_t)(m * lda) + (uint32_t)(tid & 15) * 4u;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int64_t r = i0 + (tid >> 4) + 16 * p;
      hw[p] = r < m ? (int)((((r / tapW) % tapH) << 16) | (r % tapW)) : -1;
      offa[p] = (uint32_t)(r * lda) + (uint32_t)(tid & 15) * 4u;
    }
  } else {
    h2_row_offsets<false>(offa, lda, i0, m);
  }
  H2Stage st;
  const bool upper = HALF && half_tail && (threadIdx.x & 15) >= 8;      // this lane's slot does not exist in the last k-tile
  const uint32_t back = upper ? 32u : 0u;                                // 4-byte units: the slot 128 bytes below
  if (TAPS) {
    uint32_t off[8];
    s16_tap_offsets(off, offa, hw, zoff, (int)lda, tapH, tapW, tc);
    h2_load_operand(st.a, ta, off);
  } else if (HALF) {
    const uint32_t bk = ktiles == 1 ? back : 0u;
    h2_load_operand(st.a, ta - bk, offa);
    h2_load_operand(st.b, tb - bk, offb);
  } else {
    h2_load_operand(st.a, ta, offa);
  }
  if (!HALF) h2_load_operand(st.b, tb, offb);
  for (int kt = 0; kt < ktiles; ++kt) {
    __syncthreads();
    if (HALF && upper && kt + 1 == ktiles) s16_clear_stage(st);      // (what these lanes fetched for the last k-tile is not theirs)
    s16_store_operand(st.a, ldsA);
    s16_store_operand(st.b, ldsB);
    __syncthreads();
    // (unconditional: behind the last k-tile the loads re-read it and nobody waits for them — a branch around the loads
    // makes the 64 staging registers loop-carried selects)
    const int64_t nk = (int64_t)(kt + 1 < ktiles ? kt + 1 : kt) * H2_KT;
    if (TAPS) {
      if (kt + 1 < ktiles) tc = s16_tap_next(tc, tapC);
      uint32_t off[8];
      s16_tap_offsets(off, offa, hw, zoff, (int)lda, tapH, tapW, tc);
      h2_load_operand(st.a, ta, off);
    } else if (HALF) {
      const uint32_t bk = kt + 2 >= ktiles ? back : 0u;      // the tile fetched here is the last one
      h2_load_operand(st.a, ta + nk - bk, offa);
      h2_load_operand(st.b, tb + nk - bk, offb);
    } else {
      h2_load_operand(st.a, ta + nk, offa);
    }
    if (!HALF) h2_load_operand(st.b, tb + nk, offb);
    s16_compute_ktile<CORE>(acc, ldsA, ldsB, wr, wc, lane);
  }
}

__device__ __forceinline__ void s16_zero(f32x4 (&acc)[4][4]) {
#pragma unroll
  for (int tm = 0; tm < 4; ++tm)
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// The tile (i0, j0) of a K_nM build's workgroup; false = a row block past the end of the last band.  The tiles run in bands
// of `gr` row blocks: inside an XCD's run of workgroups (xcd_remap) the row blocks of a band take one column position after
// the other, so a Z tile is shared in L2 by the row blocks of the band and the X panel of a row block by its columns.
template <int BM, int BN>
__device__ __forceinline__ bool knm_place(int gr, int64_t n, int64_t M, int64_t& i0, int64_t& j0) {
  const int64_t GR = gr;
  const int64_t tiles_n = (M + BN - 1) / BN;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * tiles_n), within = wg % (GR * tiles_n);
  i0 = (band * GR + within % GR) * BM, j0 = (within / GR) * BN;
  return i0 < n;
}

// The f64 reduce-scatter butterfly of the scoring kernels over the 16 lanes of a lane quarter (bits b8 b4 b2 b1 of the lane
// number).  A lane holds the sums over its columns of 16 row slots; a stage leaves it the half of its values that its bit
// selects, each added to the partner lane's.  QUARTER_STAGE is one stage for one pair (lo, hi): the first stage takes slots j
// and j + 8 as they are formed (w8[j]); QUARTER_STAGES_4_2 declares w4 and w2, the stages 4 and 2 of those eight; stage 1 of
// w2[0], w2[1] is the quarter's sum of slot l & 15 in lane l.  Every scoring kernel is held bit for bit to the others
// through the order of selects, shuffles and additions here.  (Macros, not functions: as inlined functions the same
// operations left the per-class and per-column kernels with other instruction streams than they had.)
#define QUARTER_STAGE(b, lo, hi, off) (((b) ? (hi) : (lo)) + __shfl_xor((b) ? (lo) : (hi), off))
#define QUARTER_STAGES_4_2(w8)                                                                  \
  double w4[4], w2[2];                                                                          \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) w4[j] = QUARTER_STAGE(b4, w8[j], w8[j + 4], 4); \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) w2[j] = QUARTER_STAGE(b2, w4[j], w4[j + 2], 2)

// -2 / (s_x s_z) of a Gaussian epilogue.  The scales of the two-term splits (and of the e4m3 packing) are powers of two: exact.
// Plain 16-bit rows (S16_BF16 / S16_F16, the wide core's CORE_BF16 / CORE_F16) carry no scale and no meta words.
template <int CORE>
__device__ __forceinline__ float core_m2(const float* __restrict__ metax, const float* __restrict__ metaz) {
  if (CORE == S16_BF16 || CORE == S16_F16) return -2.f;
  return -2.f / (metax[0] * metaz[0]);
}

// accumulator element (tm, tn, q) of a wave's 64 x 64 share: row 16 tm + 4 (lane >> 4) + q, column 16 tn + (lane & 15)
__global__ __launch_bounds__(GEMM_THREADS, 2) void gauss_knm_h2s16_kernel(
    const uint32_t* __restrict__ PX, int64_t ldpx, const float* __restrict__ metax, const float* __restrict__ xsq, int64_t n,
    const uint32_t* __restrict__ PZ, int64_t ldpz, const float* __restrict__ metaz, const float* __restrict__ zsq, int64_t M,
    int ktiles, float gamma_log2e, float* __restrict__ K, int64_t ldk, int gr) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int64_t i0, j0;
  if (!knm_place<GEMM_BM, GEMM_BN>(gr, n, M, i0, j0)) return;

  // (epilogue as in gauss_knm_h2w256_kernel: exponent formed already scaled from norms pre-multiplied by gamma log2(e), pad
  // columns through exp2(-inf) = 0, store addresses advanced by the row pitch instead of a 64-bit product per store)
  __shared__ __attribute__((aligned(16))) float xg_s[GEMM_BM];
  if (threadIdx.x < GEMM_BM) xg_s[threadIdx.x] = (i0 + threadIdx.x < n) ? xsq[i0 + threadIdx.x] * gamma_log2e : 0.f;

  f32x4 acc[4][4];
  s16_zero(acc);
  s16_mainloop(acc, PX, ldpx, n, PZ, ldpz, M, i0, j0, ktiles, lds);

  const float m2g = -2.f / (metax[0] * metaz[0]) * gamma_log2e;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const bool interior = i0 + GEMM_BM <= n && j0 + GEMM_BN <= M;
  const int64_t mpad = (M + 3) & ~int64_t(3);
  const int rl0 = wr * 64 + 4 * (lane >> 4);                // first of this lane's rows inside the tile
  const int64_t rows_left = n - i0 - rl0;
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) {
    const int cl = wc * 64 + tn * 16 + (lane & 15);
    const float zg = (j0 + cl < M) ? zsq[j0 + cl] * gamma_log2e : -__builtin_inff();
    const bool col_in = j0 + cl < mpad;
    float* pr = K + (i0 + rl0) * ldk + j0 + cl;
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
      const f32x4 xg = *reinterpret_cast<const f32x4*>(&xg_s[rl0 + tm * 16]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = __builtin_amdgcn_exp2f(fminf(fmaf(m2g, acc[tm][tn][q], xg[q]) + zg, 0.f));     // gamma < 0: d^2 >= 0 <=> e <= 0
        if (interior || (tm * 16 + q < rows_left && col_in)) *pr = v;
        pr += ldk;
      }
      pr += 12 * ldk;
    }
  }
}

// Fused scoring, tiled in two dimensions: a workgroup owns one 128-row block and one GROUP of `tg` consecutive column
// tiles of class c's centre range, and leaves its f64 partial row sums in slab[c][group][row]; mmv_reduce_kernel adds
// the groups in fixed order.  Workgroups are ordered like the K_nM build (bands of 8 row blocks x all groups inside an
// XCD's run), so the X panel of a row block is shared in L2 by the groups working on it and a Z tile by the row blocks
// of the band — one workgroup per row block walking all 79 column tiles re-fetched its 512-KB X panel for every tile
// (458 GB of L2 misses per launch at n = 1e6, M = 1e4, against 132 GB for the build).
// CORE S16_BF16 / S16_F16: PX / PZ are plain 16-bit rows (no meta), a k-tile is 128 features and `half_tail` says that the
// last one holds 64 (s16_mainloop<.., HALF>).
template <int CORE = S16_H2>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gauss_mmv_h2s16_kernel(
    const uint32_t* __restrict__ PX, int64_t ldpx, const float* __restrict__ metax, const float* __restrict__ xsq, int64_t n,
    const uint32_t* __restrict__ PZ, int64_t ldpz, const float* __restrict__ metaz, const float* __restrict__ zsq, int ktiles,
    float gamma_log2e, const double* __restrict__ V, int64_t ldv, const int32_t* __restrict__ ranges, int tg, int G,
    double* __restrict__ slab, int64_t slab_ld, int half_tail) {
  constexpr bool B16 = CORE != S16_H2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ double red[2][2][64];
  __shared__ __attribute__((aligned(16))) float xg_s[GEMM_BM];      // row norms times gamma log2(e)
  constexpr int64_t GR = 8;
  const int c = blockIdx.y;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * G), within = wg % (GR * G);
  const int64_t i0 = (band * GR + within % GR) * GEMM_BM;
  const int g = (int)(within / GR);
  const int64_t r0 = ranges[2 * c], r1 = ranges[2 * c + 1];
  const int64_t s0 = r0 + (int64_t)g * tg * GEMM_BN;
  const int64_t s1 = (s0 + (int64_t)tg * GEMM_BN < r1) ? s0 + (int64_t)tg * GEMM_BN : r1;
  if (i0 >= n || s0 >= r1) return;       // mmv_reduce_kernel only visits the groups that exist
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const float m2g = core_m2<CORE>(metax, metaz) * gamma_log2e;

  if (threadIdx.x < GEMM_BM) xg_s[threadIdx.x] = (i0 + threadIdx.x < n) ? xsq[i0 + threadIdx.x] * gamma_log2e : 0.f;
  // Lane l ends every tile with the f64 sum over the tile's 64 columns of this wave of row slot (l & 15) of its lane
  // quarter (slot = 4 tm + q, row 16 tm + 4 (l >> 4) + q): see QUARTER_STAGE.
  double tot = 0.0;
  const bool b8 = lane & 8, b4 = lane & 4, b2 = lane & 2, b1 = lane & 1;

  for (int64_t j0 = s0; j0 < s1; j0 += GEMM_BN) {
    f32x4 acc[4][4];
    s16_zero(acc);
    s16_mainloop<CORE, false, false, B16>(acc, PX, ldpx, n, PZ + j0 * ldpz, ldpz, r1 - j0, i0, 0, ktiles, lds, 0, 0, 0, half_tail != 0);
    float zs[4];
    double al[4];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int64_t col = j0 + wc * 64 + tn * 16 + (lane & 15);
      const bool cv = col < s1;
      zs[tn] = cv ? zsq[col] * gamma_log2e : 0.f;
      al[tn] = cv ? V[col * ldv + c] : 0.0;     // weight 0 removes the columns past the group / range
    }
    double w8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {       // slots j (tm = j >> 2) and j + 8 (tm = 2 + (j >> 2)), q = j & 3
      double v[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int tm = 2 * u + (j >> 2), q = j & 3;
        const float xs = xg_s[wr * 64 + tm * 16 + 4 * (lane >> 4) + q];
        v[u] = 0.0;
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) {
          const float e = fminf(fmaf(m2g, acc[tm][tn][q], xs) + zs[tn], 0.f);     // gamma < 0: d^2 >= 0 <=> e <= 0
          v[u] = fma((double)__builtin_amdgcn_exp2f(e), al[tn], v[u]);
        }
      }
      w8[j] = QUARTER_STAGE(b8, v[0], v[1], 8);
    }
    QUARTER_STAGES_4_2(w8);
    tot += QUARTER_STAGE(b1, w2[0], w2[1], 1);
  }
  {
    const int slot = lane & 15;
    red[wr][wc][(slot >> 2) * 16 + 4 * (lane >> 4) + (slot & 3)] = tot;
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int w = threadIdx.x >> 6, rr = threadIdx.x & 63;
    const int64_t row = i0 + w * 64 + rr;
    if (row < n) slab[((int64_t)c * G + g) * slab_ld + row] = red[w][0][rr] + red[w][1][rr];
  }
}

__global__ __launch_bounds__(256) void mmv_reduce_kernel(const double* __restrict__ slab, int64_t slab_ld, int G, int tg, int bn,
                                                         const int32_t* __restrict__ ranges, int64_t n,
                                                         float* __restrict__ out, int64_t ldo) {
  const int c = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const int64_t len = (int64_t)ranges[2 * c + 1] - ranges[2 * c];
  const int64_t tiles = len > 0 ? (len + bn - 1) / bn : 0;
  int groups = (int)((tiles + tg - 1) / tg);
  groups = groups < G ? groups : G;     // the caller promised max_range >= every range length
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s += slab[((int64_t)c * G + g) * slab_ld + row];
  out[row * ldo + c] = (float)s;
}

// The entries of a tile are read once per column of the group; without this the compiler converts all of them to f64 ONCE
// and keeps the doubles (twice the accumulators' registers: scratch).  No instruction: the values just become opaque.
template <int TM>
__device__ __forceinline__ void mmvn_fresh(f32x4 (&acc)[TM][4]) {
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {        // (component by component: as whole 4-register tuples they cost the wide kernels scratch)
      float e0 = acc[tm][tn][0], e1 = acc[tm][tn][1], e2 = acc[tm][tn][2], e3 = acc[tm][tn][3];
      asm volatile("" : "+v"(e0), "+v"(e1), "+v"(e2), "+v"(e3));
      acc[tm][tn][0] = e0, acc[tm][tn][1] = e1, acc[tm][tn][2] = e2, acc[tm][tn][3] = e3;
    }
}

// Shared-centre form of gauss_mmv_h2s16_kernel for a DENSE V (every column weighs all M centres): blockIdx.y is a group of
// up to NV columns c0 .. c0 + NV - 1 of V, and a tile's entries exp2(.) are formed ONCE — written over the accumulators —
// and then weighed by one column after the other.  Per column the f64 operations and their order (the fma chain over tn,
// the butterflies, the sum over the tiles, the two halves in `red`, the slab) are those of gauss_mmv_h2s16_kernel with the
// range [0, M): the same bits.  Columns past T (the padding of a group narrower than NV) weigh 0 and are not stored.
//
// PERCOL (odx_gauss_mmvn_h2_sigmas, the members of a (sigma, lambda) grid): a kernel width per column.  The accumulators
// then keep what does not depend on sigma — the raw product here, whose form pre-scales the norms by gamma; the clamped d^2
// in the wide kernel's form — and every column forms its entries with its own exponent, by the per-column kernels' own
// expressions (gauss_mmv_h2s16_kernel / gauss_mmv_h2w256_kernel): column c is bit for bit the per-column launch with
// sigma_c.  The price is NV times the exps (64 / 128 v_exp_f32 per lane, column and tile).  A launch's scaled exponents
// gamma log2(e) come by value: one group of up to 8 columns with PERCOL (padding columns repeat the last one), g[0] for every
// column without.  Per width every constant is formed by single f32 operations (no contraction into a neighbouring add).
struct MmvnGammas {
  float g[8];
};

template <int NV, bool PERCOL, int CORE = S16_H2>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gauss_mmvn_h2s16_kernel(
    const uint32_t* __restrict__ PX, int64_t ldpx, const float* __restrict__ metax, const float* __restrict__ xsq, int64_t n,
    const uint32_t* __restrict__ PZ, int64_t ldpz, const float* __restrict__ metaz, const float* __restrict__ zsq, int64_t M,
    int ktiles, MmvnGammas gm, const double* __restrict__ V, int64_t ldv, int cbase, int T, int tg, int G,
    double* __restrict__ slab, int64_t slab_ld, int half_tail) {
#pragma clang fp contract(off)
  constexpr bool B16 = CORE != S16_H2;          // plain 16-bit rows: see gauss_mmv_h2s16_kernel
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ __attribute__((aligned(16))) float xg_s[PERCOL ? NV : 1][GEMM_BM];      // row norms times (each column's) gamma log2(e)
  constexpr int64_t GR = 8;
  const int c0 = cbase + (int)blockIdx.y * NV;
  const int nc = T - c0 < NV ? T - c0 : NV;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * G), within = wg % (GR * G);
  const int64_t i0 = (band * GR + within % GR) * GEMM_BM;
  const int g = (int)(within / GR);
  const int64_t s0 = (int64_t)g * tg * GEMM_BN;
  const int64_t s1 = (s0 + (int64_t)tg * GEMM_BN < M) ? s0 + (int64_t)tg * GEMM_BN : M;
  if (i0 >= n || s0 >= M) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const float m2 = core_m2<CORE>(metax, metaz);

  if (threadIdx.x < GEMM_BM) {
    const bool in = i0 + threadIdx.x < n;
    const float xq = in ? xsq[i0 + threadIdx.x] : 0.f;
#pragma unroll
    for (int c = 0; c < (PERCOL ? NV : 1); ++c) xg_s[c][threadIdx.x] = in ? xq * gm.g[c] : 0.f;
  }
  double tot[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) tot[c] = 0.0;
  const bool b8 = lane & 8, b4 = lane & 4, b2 = lane & 2, b1 = lane & 1;

  for (int64_t j0 = s0; j0 < s1; j0 += GEMM_BN) {
    f32x4 acc[4][4];
    s16_zero(acc);
    s16_mainloop<CORE, false, false, B16>(acc, PX, ldpx, n, PZ + j0 * ldpz, ldpz, M - j0, i0, 0, ktiles, lds, 0, 0, 0,
                                          half_tail != 0);     // its barriers also publish xg_s
    float zq[4];                        // column norms; without PERCOL: times gamma log2(e) already
    int64_t voff[4];                    // < 0: a column past the group / M (weight 0)
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int64_t col = j0 + wc * 64 + tn * 16 + (lane & 15);
      const bool cv = col < s1;
      zq[tn] = cv ? (PERCOL ? zsq[col] : zsq[col] * gm.g[0]) : 0.f;
      voff[tn] = cv ? col * ldv + c0 : -1;
    }
    if (!PERCOL) {
      const float m2g = m2 * gm.g[0];
#pragma unroll
      for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float xs = xg_s[0][wr * 64 + tm * 16 + 4 * (lane >> 4) + q];
#pragma unroll
          for (int tn = 0; tn < 4; ++tn)      // gamma < 0: d^2 >= 0 <=> e <= 0
            acc[tm][tn][q] = __builtin_amdgcn_exp2f(fminf(fmaf(m2g, acc[tm][tn][q], xs) + zq[tn], 0.f));
        }
    }
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      mmvn_fresh(acc);
      const float gc = gm.g[c];
      const float m2g = m2 * gc;
      float zs[4];
      double al[4];
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        zs[tn] = voff[tn] >= 0 ? zq[tn] * gc : 0.f;
        al[tn] = (voff[tn] >= 0 && c < nc) ? V[voff[tn] + c] : 0.0;
      }
      double w8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {       // slots j (tm = j >> 2) and j + 8 (tm = 2 + (j >> 2)), q = j & 3
        double v[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int tm = 2 * u + (j >> 2), q = j & 3;
          const float xs = xg_s[PERCOL ? c : 0][wr * 64 + tm * 16 + 4 * (lane >> 4) + q];
          v[u] = 0.0;
#pragma unroll
          for (int tn = 0; tn < 4; ++tn) {
            const float e = fminf(fmaf(m2g, acc[tm][tn][q], xs) + zs[tn], 0.f);
            v[u] = fma((double)(PERCOL ? __builtin_amdgcn_exp2f(e) : acc[tm][tn][q]), al[tn], v[u]);
          }
        }
        w8[j] = QUARTER_STAGE(b8, v[0], v[1], 8);
      }
      QUARTER_STAGES_4_2(w8);
      tot[c] += QUARTER_STAGE(b1, w2[0], w2[1], 1);
    }
  }
  __syncthreads();                            // every wave is done with the operand images: `red` takes their place
  double* red = reinterpret_cast<double*>(lds);       // [NV][2 (wr)][2 (wc)][64]
  {
    const int slot = lane & 15;
#pragma unroll
    for (int c = 0; c < NV; ++c) red[((c * 2 + wr) * 2 + wc) * 64 + (slot >> 2) * 16 + 4 * (lane >> 4) + (slot & 3)] = tot[c];
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int w = threadIdx.x >> 6, rr = threadIdx.x & 63;
    const int64_t row = i0 + w * 64 + rr;
    if (row < n)
      for (int c = 0; c < nc; ++c)
        slab[((int64_t)(c0 + c) * G + g) * slab_ld + row] = red[((c * 2 + w) * 2 + 0) * 64 + rr] + red[((c * 2 + w) * 2 + 1) * 64 + rr];
  }
}

// mmv_reduce_kernel for a dense V: every column has all G groups.
__global__ __launch_bounds__(256) void mmvn_reduce_kernel(const double* __restrict__ slab, int64_t slab_ld, int G, int64_t n,
                                                          float* __restrict__ out, int64_t ldo) {
  const int c = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += slab[((int64_t)c * G + g) * slab_ld + row];
  out[row * ldo + c] = (float)s;
}

// ---------------------------------------------------------------- 256 x 256 tile core ("w256")
// 512 threads = 8 waves as 2 (rows) x 4 (columns); a wave owns 128 x 64 outputs = 8 x 4 blocks of v_mfma_f32_16x16x32_f16
// (128 accumulator registers).  A k-stage is one granule (32 features = 128 B) of 256 rows of each operand: 64 KiB, held
// twice.  Stage s + 1 is written to the other buffer and stage s + 2 is fetched into registers while stage s is
// multiplied: one barrier per stage.  LDS rows are exactly 128 B; the 16-byte slot q of row r lives at q ^ ((r >> 1) & 7):
// rows of equal parity share their banks, and a 16-lane group of ds_read_b128 reads, per parity, 4 rows at chunk c and 4
// rows at chunk c ^ 1 whose keys (r >> 1) are all different => 16 distinct slots, conflict-free; a ds_write_b128 group
// of 8 lanes writes the 8 slots of one row.
constexpr int W_BM = 256, W_BN = 256, W_THREADS = 512;
constexpr int W_KS = 32;                                  // features per stage (one granule)
constexpr int W_ROW = 128;                                // bytes per LDS row
constexpr int W_OPND_BYTES = W_BM * W_ROW;                // 32,768
constexpr int W_STAGE_BYTES = 2 * W_OPND_BYTES;           // 65,536
constexpr int W_LDS_BYTES = 2 * W_STAGE_BYTES;            // 131,072

// PERM (the B operand of the K_nM builds): LDS row 64 w + 16 t + r of the image holds operand row 64 w + 4 r + t, so that
// the four accumulator blocks tn = 0..3 of a lane are four ADJACENT output columns 64 wc + 4 (lane & 15) + tn and the
// epilogue stores 16 bytes per lane (a whole 256-byte row segment per 16 lanes) instead of four scattered floats.  The
// image's geometry — and with it the conflict-free fragment reads — is unchanged: only which operand row a lane fetches.

// CORE_H2: operands are two-term f16 splits, three v_mfma_f32_16x16x32_f16 per product block (lo.hi, hi.lo, hi.hi).
// CORE_F8: operands are OCP e4m3 bytes (odx_split_f8): a stage's 128 bytes per row are 128 FEATURES, and the 16-byte
// pieces a lane reads as "hi" and "lo" — chunks g and g + 4 of the row — are simply its 32 of them: ONE
// v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales, 2^0) per product block.  Both operands split the row the same way,
// so the order in which a lane group's 32 features enter the sum is the same permutation for A and B — a dot product does
// not care.  Same loads, same LDS image, same stores: 4 x the features per stage in 1/3 of the MFMA issue slots.
enum { CORE_H2 = 0, CORE_F8 = 1, CORE_BF16 = S16_BF16, CORE_F16 = S16_F16 };   // the 16-bit cores: see s16_compute_ktile
typedef int i32x8 __attribute__((ext_vector_type(8)));
constexpr int F8_SCALE_ONE = 0x7f7f7f7f;      // E8M0 exponent 127 = 2^0 in every byte (op_sel picks byte 0)

__device__ __forceinline__ i32x8 f8_frag(const f16x8& lo16, const f16x8& hi16) {
  const u32x4 a = __builtin_bit_cast(u32x4, lo16), b = __builtin_bit_cast(u32x4, hi16);
  return i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}

// ---- the stage pipeline: operands staged by LDS-DMA (buffer_load_dwordx4 ... lds).  (Round 3's register-staged loop — global ->
// registers -> ds_write — measured 8-10 % slower in same-process A/B runs and is gone.)
// A wave-instruction of the DMA fills 1 KiB of LDS — 8 rows of the image — as wave-uniform base + lane * 16: lane l lands in
// slot l & 7 of image row 8 P + (l >> 3), so the XOR swizzle of the image is applied on the SOURCE side (the lane fetches chunk
// (l & 7) ^ ((row >> 1) & 7) of its row: the same 128-byte line, its 16-byte pieces permuted).  Wave w moves pieces w, w + 8,
// w + 16, w + 24 of each operand: 8 DMAs per wave and stage, no staging registers (32 fewer VGPRs), no ds_write (a quarter
// of the LDS instructions, none of the 13-cycle register -> LDS transfers).  The freed registers hold the NEXT part's A
// fragments, read before the current part's MFMAs are issued, so that no MFMA waits for an LDS read inside a stage.
// Stage s + 1 is fetched into the other buffer during stage s; every wave waits for its own DMAs (vmcnt(0)) before the
// barrier that ends the stage — nothing else orders a ds_read behind an LDS-DMA.  Rows are addressed through one buffer
// descriptor per operand (tile base, rows clamped to the operand's last row), the stage on the scalar
// offset: no vector address arithmetic in the loop.
typedef __attribute__((address_space(3))) void* lds_ptr_t;

template <bool PERM>
__device__ __forceinline__ void w_dma_offsets(uint32_t (&voff)[4], int64_t ld, int64_t row0, int64_t nrows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t l64 = nrows - 1 - row0;               // >= 0: the tile starts inside the operand
  const int last = l64 < W_BM - 1 ? (int)l64 : W_BM - 1;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int ri = 8 * wave + 64 * p + (lane >> 3);    // image row this lane fills
    const int r = PERM ? ((ri & ~63) | ((ri & 15) << 2) | ((ri >> 4) & 3)) : ri;
    const int q = (lane & 7) ^ ((ri >> 1) & 7);        // chunk of the row that belongs in slot lane & 7
    voff[p] = ((uint32_t)(r < last ? r : last) * (uint32_t)ld + (uint32_t)q * 4u) * 4u;      // bytes
  }
}

struct WDma {
  __amdgpu_buffer_rsrc_t ra, rb;
  uint32_t va[4], vb[4];       // per-lane byte offsets of this wave's four 8-row pieces of each operand
  int fa, fb, hi, lo;          // LDS: fragment rows of this lane in the A / B image, hi / lo chunk inside a row
  // TAPS (A = the 3 x 3 neighbourhood matrix of packed NHWC rows, never materialised: see w_mainloop_dma):
  int th[4], tw[4];            // map position (h, w) of the lane's four rows (h = -4 for a row past the operand's end)
  int tH, tW, tld, tkb;        // map size, row stride in bytes, bytes of one tap inside a packed row (4 C)
  uint32_t tzero;              // this lane's chunk of the all-zero row behind the operand's last row
};

// Stage -> (tap, channel offset) for the TAPS operand, kept as a cursor: stage s covers the 32 channels at byte `kin` of tap
// (dy, dx) = (ky - 1, kx - 1), taps in the order ky kx of the weight matrix's K axis.
struct WTapCur {
  int kin, dy, dx;
};
__device__ __forceinline__ WTapCur w_tap_next(WTapCur c, int kbytes) {
  c.kin += W_KS * 4;
  if (c.kin == kbytes) {
    c.kin = 0;
    if (++c.dx == 2) {
      c.dx = -1;
      ++c.dy;
    }
  }
  return c;
}

// pieces q0 .. q1 - 1 (0..7: A pieces 0..3, B pieces 0..3) of stage `koff` (bytes into the rows) -> image `dst`
template <int Q0, int Q1, bool TAPS = false>
__device__ __forceinline__ void w_dma_pieces(const WDma& ad, char* dst, int koff, const WTapCur tc = WTapCur{0, 0, 0}) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int q = Q0; q < Q1; ++q) {
    char* d = dst + (q >> 2) * W_OPND_BYTES + wave * 1024 + (q & 3) * 8192;
    if (q < 4) {
      if (TAPS) {
        // the row of the neighbour (h + dy, w + dx) of this lane's row, or the zero row when that is outside the map
        const bool in = (unsigned)(ad.th[q & 3] + tc.dy) < (unsigned)ad.tH && (unsigned)(ad.tw[q & 3] + tc.dx) < (unsigned)ad.tW;
        const uint32_t v = in ? ad.va[q & 3] + (uint32_t)((tc.dy * ad.tW + tc.dx) * ad.tld) : ad.tzero;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ad.ra, (lds_ptr_t)d, 16, v, tc.kin, 0, 0);
      } else {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ad.ra, (lds_ptr_t)d, 16, ad.va[q & 3], koff, 0, 0);
      }
    } else {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ad.rb, (lds_ptr_t)d, 16, ad.vb[q & 3], koff, 0, 0);
    }
  }
}

struct WFrag {
  f16x8 bh[4], bl[4];       // the stage's B fragments (4 column blocks)
  f16x8 a0h[2], a0l[2];     // A fragments of parts 0 and 2 (2 row blocks each)
  f16x8 a1h[2], a1l[2];     // A fragments of parts 1 and 3
};

__device__ __forceinline__ void w_read_b1(WFrag& f, const char* img, const WDma& ad, int t) {
  f.bh[t] = *reinterpret_cast<const f16x8*>(img + ad.fb + t * 16 * W_ROW + ad.hi);
  f.bl[t] = *reinterpret_cast<const f16x8*>(img + ad.fb + t * 16 * W_ROW + ad.lo);
}

__device__ __forceinline__ void w_read_a(f16x8 (&ah)[2], f16x8 (&al)[2], const char* img, const WDma& ad, int part) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    ah[u] = *reinterpret_cast<const f16x8*>(img + ad.fa + (2 * part + u) * 16 * W_ROW + ad.hi);
    al[u] = *reinterpret_cast<const f16x8*>(img + ad.fa + (2 * part + u) * 16 * W_ROW + ad.lo);
  }
}

// the MFMAs of row blocks tm0, tm0 + 1 against column block tn (every accumulator sees its products in the same order
// whatever the order of the blocks: the sums do not depend on the schedule)
template <int CORE>
__device__ __forceinline__ void w_mfma_col(f32x4 (&acc)[8][4], const f16x8 (&ah)[2], const f16x8 (&al)[2], const f16x8& bh,
                                           const f16x8& bl, int tm0, int tn) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (CORE == CORE_F8) {
      acc[tm0 + u][tn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(f8_frag(ah[u], al[u]), f8_frag(bh, bl), acc[tm0 + u][tn], 0, 0,
                                                                           0, F8_SCALE_ONE, 0, F8_SCALE_ONE);
    } else if (CORE == CORE_BF16) {
      acc[tm0 + u][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah[u]), __builtin_bit_cast(bf16x8, bh), acc[tm0 + u][tn], 0, 0, 0);
      acc[tm0 + u][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, al[u]), __builtin_bit_cast(bf16x8, bl), acc[tm0 + u][tn], 0, 0, 0);
    } else if (CORE == CORE_F16) {
      acc[tm0 + u][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], bh, acc[tm0 + u][tn], 0, 0, 0);
      acc[tm0 + u][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[u], bl, acc[tm0 + u][tn], 0, 0, 0);
    } else {
      acc[tm0 + u][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[u], bh, acc[tm0 + u][tn], 0, 0, 0);
      acc[tm0 + u][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], bl, acc[tm0 + u][tn], 0, 0, 0);
      acc[tm0 + u][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], bh, acc[tm0 + u][tn], 0, 0, 0);
    }
  }
}

// the order a part's instructions are to be issued in: 4 x (one LDS read, then PER MFMAs), NV x (one DMA, then PER MFMAs)
template <int PER, int NV>
__device__ __forceinline__ void w_sched_part() {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // DS read
    __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);    // MFMA
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // VMEM read (the DMA)
    __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
  }
}

// One stage (s).  On entry `f` holds the stage's B fragments and the A fragments of part 0 (read behind the barrier of the
// stage before), and pieces 0..2 of stage s + 1 are on their way into `nxt`.  Parts 0..2 read the next part's A fragments
// under their own MFMAs; parts 0 and 1 also issue the other five DMAs of stage s + 1 (F1), one per few MFMAs — a DMA costs
// its wave ~60 cycles of issue, and eight of them in one place, in both waves of a SIMD at once, are 500 cycles in which
// the matrix pipe has nothing to do.  In front of part 3 every LDS read of the stage has been issued: the wave waits for
// them and for its own DMAs of stage s + 1, meets the others at the barrier, then — the image of stage s is free, that of
// stage s + 1 complete — starts the DMAs of stage s + 2 (pieces 0..2, F2) and reads the first A fragments and, column block
// by column block as part 3 is done with them, the B fragments of stage s + 1 (F1), all UNDER the 24 MFMAs of part 3:
// neither the barrier's skew nor the LDS latency of a stage's first fragments stops the matrix pipe, and the B fragments
// need no second register set.
template <bool F1, bool F2, int CORE, bool TAPS = false>
__device__ __forceinline__ void w_stage_dma(f32x4 (&acc)[8][4], WFrag& f, const char* cur, char* nxt, int koff1, const WDma& ad,
                                            const WTapCur tc1 = WTapCur{0, 0, 0}) {
  constexpr int PER = CORE == CORE_F8 ? 1 : (CORE == CORE_H2 ? 3 : 2);
  // part 0, reading part 1
  w_read_a(f.a1h, f.a1l, cur, ad, 1);
  if (F1) w_dma_pieces<3, 6, TAPS>(ad, nxt, koff1, tc1);
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) w_mfma_col<CORE>(acc, f.a0h, f.a0l, f.bh[tn], f.bl[tn], 0, tn);
  w_sched_part<PER, F1 ? 3 : 0>();
  __builtin_amdgcn_sched_barrier(0);
  // part 1, reading part 2
  w_read_a(f.a0h, f.a0l, cur, ad, 2);
  if (F1) w_dma_pieces<6, 8>(ad, nxt, koff1);
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) w_mfma_col<CORE>(acc, f.a1h, f.a1l, f.bh[tn], f.bl[tn], 2, tn);
  w_sched_part<PER, F1 ? 2 : 0>();
  __builtin_amdgcn_sched_barrier(0);
  // part 2, reading part 3
  w_read_a(f.a1h, f.a1l, cur, ad, 3);
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) w_mfma_col<CORE>(acc, f.a0h, f.a0l, f.bh[tn], f.bl[tn], 4, tn);
  w_sched_part<PER, 0>();
  __builtin_amdgcn_sched_barrier(0);
  if (F1) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (F2) w_dma_pieces<0, 3, TAPS>(ad, const_cast<char*>(cur), koff1 + W_KS * 4, TAPS ? w_tap_next(tc1, ad.tkb) : tc1);
    w_read_a(f.a0h, f.a0l, nxt, ad, 0);
  }
  // part 3, column block by column block; each block's B registers take the next stage's fragments as soon as it is done
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) {
    w_mfma_col<CORE>(acc, f.a1h, f.a1l, f.bh[tn], f.bl[tn], 6, tn);
    __builtin_amdgcn_sched_barrier(0);
    if (F1) w_read_b1(f, nxt, ad, tn);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// TAPS: A is not an (m x K) matrix in memory but the 3 x 3 neighbourhood matrix (K = 9 C, tap after tap) of the packed NHWC
// rows Y (m = R H W rows of C channels, C % 32 == 0, followed by ONE all-zero row; (m + 1) ld 4 < 2^31 bytes): row r of
// stage s is read from Y's row of the neighbour (h + dy, w + dx) at the stage's channels, or from the zero row outside the
// map.  The gather costs two compares and a select per DMA; the 9 x copy of the activation that odx_split_f16_taps3x3 writes
// (2.2 GB per conv5-head layer at 2400 RoIs) and this loop would read back is never made.
template <bool PERMB = false, int CORE = CORE_H2, bool TAPS = false>
__device__ __forceinline__ void w_mainloop_dma(f32x4 (&acc)[8][4], const uint32_t* __restrict__ A, int64_t lda, int64_t m,
                                               const uint32_t* __restrict__ B, int64_t ldb, int64_t n, int64_t i0, int64_t j0,
                                               int stages, char* lds, int tapH = 0, int tapW = 0, int tapC = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  WDma ad;
  w_dma_offsets<PERMB>(ad.vb, ldb, j0, n);
  const int64_t la = m - i0 < W_BM ? m - i0 : W_BM, lb = n - j0 < W_BN ? n - j0 : W_BN;       // rows of the tile that exist
  if (TAPS) {
    ad.tH = tapH;
    ad.tW = tapW;
    ad.tld = (int)(lda * 4);
    ad.tkb = tapC;                       // bytes of one tap inside a row: 4 C (packed two-term rows), 2 C (16-bit rows)
    const uint32_t chunk = (uint32_t)(((lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7)) * 16);   // (ri >> 1) & 7 is the same for the four pieces
    ad.tzero = (uint32_t)(m * lda * 4) + chunk;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int64_t r = i0 + 8 * wave + 64 * p + (lane >> 3);
      const bool real = r < m;
      ad.th[p] = real ? (int)((r / tapW) % tapH) : -4;
      ad.tw[p] = real ? (int)(r % tapW) : -4;
      ad.va[p] = (uint32_t)(r * lda * 4) + chunk;
    }
    ad.ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(A), (short)0, (int)((m + 1) * lda * 4), 0x00020000);
  } else {
    w_dma_offsets<false>(ad.va, lda, i0, m);
    ad.ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(A + i0 * lda), (short)0, (int)(la * lda * 4), 0x00020000);
  }
  ad.rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(B + j0 * ldb), (short)0, (int)(lb * ldb * 4), 0x00020000);
  const int r = lane & 15, g = lane >> 4;
  ad.hi = ((g ^ ((r >> 1) & 7)) << 4);
  ad.lo = ad.hi ^ 64;
  ad.fa = (wr * 128 + r) * W_ROW;
  ad.fb = W_OPND_BYTES + (wc * 64 + r) * W_ROW;
  // (the caller's last use of the LDS ended on a barrier)
  WTapCur tc{0, -1, -1};                 // stage 0: tap (ky, kx) = (0, 0), first channels
  w_dma_pieces<0, 8, TAPS>(ad, lds, 0, tc);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (TAPS) tc = w_tap_next(tc, ad.tkb);                // from here on: the cursor of stage s + 1
  if (stages > 1) w_dma_pieces<0, 3, TAPS>(ad, lds + W_STAGE_BYTES, W_KS * 4, tc);
  WFrag f;
#pragma unroll
  for (int t = 0; t < 4; ++t) w_read_b1(f, lds, ad, t);
  w_read_a(f.a0h, f.a0l, lds, ad, 0);
  int s = 0;
  for (; s + 2 < stages; ++s) {
    w_stage_dma<true, true, CORE, TAPS>(acc, f, lds + (s & 1) * W_STAGE_BYTES, lds + ((s + 1) & 1) * W_STAGE_BYTES, (s + 1) * (W_KS * 4), ad, tc);
    if (TAPS) tc = w_tap_next(tc, ad.tkb);
  }
  if (s + 1 < stages) {
    w_stage_dma<true, false, CORE, TAPS>(acc, f, lds + (s & 1) * W_STAGE_BYTES, lds + ((s + 1) & 1) * W_STAGE_BYTES, (s + 1) * (W_KS * 4), ad, tc);
    ++s;
  }
  w_stage_dma<false, false, CORE, TAPS>(acc, f, lds + (s & 1) * W_STAGE_BYTES, lds, 0, ad);
  __syncthreads();          // every wave has read its last fragments: the LDS is the caller's again
}

// ---- A/B of the MFMA shape (round-4 review, item 3 iii): the SAME stage pipeline — LDS-DMA staging, the LDS image, the DMA
// issue spread over the parts, the barrier in front of the last part — with v_mfma_f32_32x32x16_f16 instead of
// v_mfma_f32_16x16x32_f16: half the MFMA instructions for the same products (12 instead of 24 per part, each twice as long), the
// same number of fragment reads (a 32-row block of one 16-feature step is 16 bytes per lane: row lane & 31, k-chunk lane >> 5
// + 2 step), the same registers (4 x 2 accumulator blocks of 16 instead of 8 x 4 of 4; 8 B and 2 x 4 A fragment registers).
// A wave's share is still 128 x 64.  Used by the debug entry odx_debug_gemm_h2_mf32 only (tools/ab_mfma_shape.py).
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct WFrag32 {
  f16x8 bh[2][2], bl[2][2];   // [column block of 32][k-step]
  f16x8 a0h[2], a0l[2];       // A fragments of parts 0 and 2 (one 32-row block, two k-steps)
  f16x8 a1h[2], a1l[2];       // parts 1 and 3
};

struct WOff32 {
  int fa, fb;                 // LDS row of this lane in the A / B image (row lane & 31 of block 0)
  int hi[2];                  // byte offset of the hi chunk of k-step 0 / 1 inside the lane's row; lo = hi ^ 64
};

__device__ __forceinline__ void w32_read_a(f16x8 (&ah)[2], f16x8 (&al)[2], const char* img, const WOff32& o, int part) {
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    ah[st] = *reinterpret_cast<const f16x8*>(img + o.fa + part * 32 * W_ROW + o.hi[st]);
    al[st] = *reinterpret_cast<const f16x8*>(img + o.fa + part * 32 * W_ROW + (o.hi[st] ^ 64));
  }
}

__device__ __forceinline__ void w32_read_b1(WFrag32& f, const char* img, const WOff32& o, int c, int st) {
  f.bh[c][st] = *reinterpret_cast<const f16x8*>(img + o.fb + c * 32 * W_ROW + o.hi[st]);
  f.bl[c][st] = *reinterpret_cast<const f16x8*>(img + o.fb + c * 32 * W_ROW + (o.hi[st] ^ 64));
}

__device__ __forceinline__ void w32_mfma(f32x16& acc, const f16x8& ah, const f16x8& al, const f16x8& bh, const f16x8& bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
}

template <bool F1, bool F2>
__device__ __forceinline__ void w32_stage(f32x16 (&acc)[4][2], WFrag32& f, const char* cur, char* nxt, int koff1, const WDma& ad, const WOff32& o) {
  // part 0, reading part 1
  w32_read_a(f.a1h, f.a1l, cur, o, 1);
  if (F1) w_dma_pieces<3, 6>(ad, nxt, koff1);
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int st = 0; st < 2; ++st) w32_mfma(acc[0][c], f.a0h[st], f.a0l[st], f.bh[c][st], f.bl[c][st]);
  w_sched_part<3, F1 ? 3 : 0>();
  __builtin_amdgcn_sched_barrier(0);
  // part 1, reading part 2
  w32_read_a(f.a0h, f.a0l, cur, o, 2);
  if (F1) w_dma_pieces<6, 8>(ad, nxt, koff1);
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int st = 0; st < 2; ++st) w32_mfma(acc[1][c], f.a1h[st], f.a1l[st], f.bh[c][st], f.bl[c][st]);
  w_sched_part<3, F1 ? 2 : 0>();
  __builtin_amdgcn_sched_barrier(0);
  // part 2, reading part 3
  w32_read_a(f.a1h, f.a1l, cur, o, 3);
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int st = 0; st < 2; ++st) w32_mfma(acc[2][c], f.a0h[st], f.a0l[st], f.bh[c][st], f.bl[c][st]);
  w_sched_part<3, 0>();
  __builtin_amdgcn_sched_barrier(0);
  if (F1) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (F2) w_dma_pieces<0, 3>(ad, const_cast<char*>(cur), koff1 + W_KS * 4);
    w32_read_a(f.a0h, f.a0l, nxt, o, 0);
  }
  // part 3; each (column block, k-step) pair's B registers take the next stage's fragments as soon as it is done
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      w32_mfma(acc[3][c], f.a1h[st], f.a1l[st], f.bh[c][st], f.bl[c][st]);
      __builtin_amdgcn_sched_barrier(0);
      if (F1) w32_read_b1(f, nxt, o, c, st);
    }
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ void w32_mainloop_dma(f32x16 (&acc)[4][2], const uint32_t* __restrict__ A, int64_t lda, int64_t m,
                                                 const uint32_t* __restrict__ B, int64_t ldb, int64_t n, int64_t i0, int64_t j0, int stages,
                                                 char* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  WDma ad;
  w_dma_offsets<false>(ad.va, lda, i0, m);
  w_dma_offsets<false>(ad.vb, ldb, j0, n);
  const int64_t la = m - i0 < W_BM ? m - i0 : W_BM, lb = n - j0 < W_BN ? n - j0 : W_BN;
  ad.ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(A + i0 * lda), (short)0, (int)(la * lda * 4), 0x00020000);
  ad.rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(B + j0 * ldb), (short)0, (int)(lb * ldb * 4), 0x00020000);
  const int r = lane & 31, kh = lane >> 5;
  WOff32 o;
  o.fa = (wr * 128 + r) * W_ROW;
  o.fb = W_OPND_BYTES + (wc * 64 + r) * W_ROW;
#pragma unroll
  for (int st = 0; st < 2; ++st) o.hi[st] = (((kh + 2 * st) ^ ((r >> 1) & 7)) << 4);
  w_dma_pieces<0, 8>(ad, lds, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (stages > 1) w_dma_pieces<0, 3>(ad, lds + W_STAGE_BYTES, W_KS * 4);
  WFrag32 f;
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int st = 0; st < 2; ++st) w32_read_b1(f, lds, o, c, st);
  w32_read_a(f.a0h, f.a0l, lds, o, 0);
  int s = 0;
  for (; s + 2 < stages; ++s)
    w32_stage<true, true>(acc, f, lds + (s & 1) * W_STAGE_BYTES, lds + ((s + 1) & 1) * W_STAGE_BYTES, (s + 1) * (W_KS * 4), ad, o);
  if (s + 1 < stages) {
    w32_stage<true, false>(acc, f, lds + (s & 1) * W_STAGE_BYTES, lds + ((s + 1) & 1) * W_STAGE_BYTES, (s + 1) * (W_KS * 4), ad, o);
    ++s;
  }
  w32_stage<false, false>(acc, f, lds + (s & 1) * W_STAGE_BYTES, lds, 0, ad, o);
  __syncthreads();
}

// out = A B' / (s_A s_B) with the 32 x 32 x 16 loop above: plain f32 stores, no bias / residual (a measurement and its check)
__global__ __launch_bounds__(W_THREADS, 1) void gemm_h2w256_mf32_kernel(
    const uint32_t* __restrict__ PA, int64_t ldpa, const float* __restrict__ metaa, int64_t m, const uint32_t* __restrict__ PB,
    int64_t ldpb, const float* __restrict__ metab, int64_t n, int stages, float* __restrict__ out, int64_t ldo, int gr) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int64_t GR = gr;
  const int64_t tiles_n = (n + W_BN - 1) / W_BN;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * tiles_n), within = wg % (GR * tiles_n);
  const int64_t i0 = (band * GR + within % GR) * W_BM, j0 = (within / GR) * W_BN;
  if (i0 >= m) return;
  f32x16 acc[4][2];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[p][c][j] = 0.f;
  w32_mainloop_dma(acc, PA, ldpa, m, PB, ldpb, n, i0, j0, stages, lds);
  const float inv = 1.f / (metaa[0] * metab[0]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int r = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int64_t col = j0 + wc * 64 + c * 32 + r;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int64_t row = i0 + wr * 128 + p * 32 + (j >> 2) * 8 + kh * 4 + (j & 3);
        if (row < m && col < n) out[row * ldo + col] = acc[p][c][j] * inv;
      }
    }
}

__device__ __forceinline__ void w_zero(f32x4 (&acc)[8][4]) {
#pragma unroll
  for (int tm = 0; tm < 8; ++tm)
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Storage formats of a K_nM block (what the CG passes stream):
//   KF_F32   n x ldk floats (ldk = roundup(M, 4)), the parity format
//   KF_U24   24-bit fixed point on [0, 1]: q = round(K 2^24) (2^24 - 1 for K = 1) as a u16 plane of q >> 8 and a u8 plane of
//            q & 255 (both n x ld8, ld8 = roundup(M, 8)): 3 bytes per entry.  Absolute step 2^-24 — f32's own on [0.5, 1),
//            coarser than f32 below; tools/precision_storage_study.py: alpha moves against the f64 evaluation as with f32
//            storage on the problems whose entries sit near 1 (the ill-conditioned ones) and stays 5 x under the 1e-4 bar
//            on the small-sigma ones where it is coarser
//   KF_BF16  K rounded to bf16 (n x ld8 u16): BASELINE config 2's throughput-only storage, 2 bytes per entry
enum { KF_F32 = 0, KF_U24 = 1, KF_BF16 = 2 };

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t u24_of(float v) {
  const uint32_t q = (uint32_t)__builtin_rintf(v * 16777216.f);       // v in [0, 1]; exact scaling, one rounding
  return q > 16777215u ? 16777215u : q;
}

__device__ __forceinline__ unsigned short bf16_of(float v) {          // round to nearest even (v is finite, >= 0)
  const uint32_t u = __float_as_uint(v);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// The value of radial kernel KIND (ODX_KERNEL_*) from the Gaussian tiles' scaled exponent e = gamma log2(e) d^2 <= 0, gamma =
// -1 / (2 sigma^2): the Gaussian is exp2(e).  For a Matern kind d^2 / sigma^2 = -2 ln(2) e, so u = sqrt(2 nu d^2) / sigma =
// sqrt(-4 nu ln(2) e) needs no constant per width, and k = poly(u) exp2(-u log2(e)): a square root, an exp2 and three
// (nu = 3/2) or four (nu = 5/2) f32 operations.  Both are smooth in d^2 at 0 (k = 1 - u^2 / 2 + ..., u^2 linear in d^2), slopes
// 3 / (2 sigma^2) and 5 / (6 sigma^2) against the Gaussian's 1 / (2 sigma^2).  e = -inf gives inf * 0: callers that mark columns
// that way select.
template <int KIND>
__device__ __forceinline__ float radial_value(float e) {
  static_assert(KIND == ODX_KERNEL_GAUSS || KIND == ODX_KERNEL_MATERN32 || KIND == ODX_KERNEL_MATERN52, "unknown kernel kind");
  if constexpr (KIND == ODX_KERNEL_GAUSS) {
    return __builtin_amdgcn_exp2f(e);
  } else {
    constexpr float c = KIND == ODX_KERNEL_MATERN32 ? -4.1588830833596715f : -6.9314718055994531f;      // -4 nu ln(2)
    const float u = __builtin_amdgcn_sqrtf(c * e);
    const float p = KIND == ODX_KERNEL_MATERN32 ? 1.f + u : fmaf(u, fmaf(u, 0.33333333333333333f, 1.f), 1.f);
    return p * __builtin_amdgcn_exp2f(u * -LOG2E);
  }
}

// One lane's share of a tile's epilogue.  The exponent is formed already scaled, e = gamma log2(e) d^2 = fma(m2g, acc, xg) + zg
// with the row / column norms pre-multiplied (xg in LDS, zg in registers; zg = -inf for the pad columns [M, mpad), which
// are thereby stored as exp2(-inf) = 0 without a select — a Matern KIND would make inf * 0 of that and selects an exact
// zero): two operations per entry instead of three; the store addresses
// advance by the row pitch (the 64-bit products row * ld per store were a quarter-rate multiply chain of six instructions
// per row); the two planes of the 24-bit format are cut out of the four words by two + three v_perm_b32 / v_or_b32.
// `interior`: the tile lies inside the block, every store happens.
template <bool RHS, int FMT, int KIND = ODX_KERNEL_GAUSS>
__device__ __forceinline__ void knm_tile_epilogue(const f32x4 (&acc)[8][4], const float* xg_s, const double* ws_s, int rl0,
                                                  float m2g, const float (&zg)[4], bool interior, bool cols_in,
                                                  int64_t rows_left, char* phi, int64_t shi, char* plo, int64_t slo,
                                                  double (&csum)[4]) {
#pragma unroll
  for (int tm = 0; tm < 8; ++tm) {
    const f32x4 xg = *reinterpret_cast<const f32x4*>(&xg_s[rl0 + tm * 16]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double wq = RHS ? ws_s[rl0 + tm * 16 + q] : 0.0;
      f32x4 v;
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {   // gamma < 0: d^2 >= 0 <=> e <= 0
        v[tn] = radial_value<KIND>(fminf(fmaf(m2g, acc[tm][tn][q], xg[q]) + zg[tn], 0.f));
        if (KIND != ODX_KERNEL_GAUSS) v[tn] = zg[tn] == -__builtin_inff() ? 0.f : v[tn];      // pad columns: exact zeros
      }
      const bool store = interior || (tm * 16 + q < rows_left && cols_in);
      if (FMT == KF_F32) {
        if (RHS) {
#pragma unroll
          for (int tn = 0; tn < 4; ++tn) csum[tn] = fma((double)v[tn], wq, csum[tn]);
        }
        if (store) *reinterpret_cast<f32x4*>(phi) = v;      // (non-temporal stores: no difference)
      } else if (FMT == KF_U24) {
        uint32_t qv[4];
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) {
          qv[tn] = u24_of(v[tn]);
          if (RHS) csum[tn] = fma((double)qv[tn], wq, csum[tn]);                       // scaled by 2^-24 below
        }
        if (store) {
          // bytes 1, 2 of each word -> the u16 plane; byte 0 of each -> the u8 plane
          const uint32_t h01 = __builtin_amdgcn_perm(qv[1], qv[0], 0x06050201u), h23 = __builtin_amdgcn_perm(qv[3], qv[2], 0x06050201u);
          *reinterpret_cast<uint2*>(phi) = make_uint2(h01, h23);
          *reinterpret_cast<uint32_t*>(plo) =
              __builtin_amdgcn_perm(qv[1], qv[0], 0x0c0c0400u) | __builtin_amdgcn_perm(qv[3], qv[2], 0x04000c0cu);
        }
      } else {
        u16x4 b;
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) {
          b[tn] = bf16_of(v[tn]);
          if (RHS) csum[tn] = fma((double)__uint_as_float((uint32_t)b[tn] << 16), wq, csum[tn]);
        }
        if (store) *reinterpret_cast<u16x4*>(phi) = b;
      }
      phi += shi;
      if (FMT == KF_U24) plo += slo;
    }
    phi += 12 * shi;
    if (FMT == KF_U24) plo += 12 * slo;
    if (RHS) __builtin_amdgcn_sched_barrier(0);      // keep the row weights of later blocks out of registers until needed
  }
}

// accumulator element (tm, tn, q) of a wave's 128 x 64 share (B rows permuted, w_mainloop_dma<true>):
// row 16 tm + 4 (lane >> 4) + q, column 4 (lane & 15) + tn — a lane holds four adjacent columns of every one of its rows.
// RHS: also leave wslab[row block][j] = sum over the tile's rows i of K_ij w_i (f64), K_ij being the value the block
// STORES (the dequantised one for KF_U24 / KF_BF16): the column sums K' w of the right-hand side of the fit come out of
// the build, and the first pass over the stored K_nM is not needed.
// KIND: the radial kernel of the entries (radial_value; the Gaussian instantiations are the code they were before the parameter).
template <bool RHS, int FMT, int CORE, int KIND = ODX_KERNEL_GAUSS>
__global__ __launch_bounds__(W_THREADS, 1) void gauss_knm_h2w256_kernel(
    const uint32_t* __restrict__ PX, int64_t ldpx, const float* __restrict__ metax, const float* __restrict__ xsq, int64_t n,
    const uint32_t* __restrict__ PZ, int64_t ldpz, const float* __restrict__ metaz, const float* __restrict__ zsq, int64_t M,
    int stages, float gamma_log2e, void* __restrict__ Kp, int64_t ldk, unsigned char* __restrict__ Klo, int64_t ldlo, int gr,
    const double* __restrict__ w, double* __restrict__ wslab, int64_t wslab_ld) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int64_t i0, j0;
  if (!knm_place<W_BM, W_BN>(gr, n, M, i0, j0)) return;

  __shared__ __attribute__((aligned(16))) float xg_s[W_BM];
  __shared__ double ws_s[RHS ? W_BM : 1];
  if (threadIdx.x < W_BM) {
    xg_s[threadIdx.x] = (i0 + threadIdx.x < n) ? xsq[i0 + threadIdx.x] * gamma_log2e : 0.f;
    if (RHS) ws_s[threadIdx.x] = (i0 + threadIdx.x < n) ? w[i0 + threadIdx.x] : 0.0;   // rows past the end weigh nothing
  }

  f32x4 acc[8][4];
  w_zero(acc);
  w_mainloop_dma<true, CORE>(acc, PX, ldpx, n, PZ, ldpz, M, i0, j0, stages, lds);      // its barriers also publish xg_s

  const float m2g = core_m2<CORE>(metax, metaz) * gamma_log2e;     // the scales are powers of two (16-bit rows: none): m2 is exact
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int cb = wc * 64 + 4 * (lane & 15);                 // first of this lane's four adjacent columns inside the tile
  const int rl0 = wr * 128 + 4 * (lane >> 4);               // first of this lane's rows inside the tile
  const int64_t mpad = FMT == KF_F32 ? ((M + 3) & ~int64_t(3)) : ((M + 7) & ~int64_t(7));
  const bool interior = i0 + W_BM <= n && j0 + W_BN <= M;
  const bool cols_in = j0 + cb < mpad;                      // groups of four: entirely inside the padded row or not at all
  double csum[4] = {0.0, 0.0, 0.0, 0.0};
  float zg[4];
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) zg[tn] = j0 + cb + tn < M ? zsq[j0 + cb + tn] * gamma_log2e : -__builtin_inff();
  const int64_t e0 = (i0 + rl0) * ldk + j0 + cb;            // this lane's first entry
  const int esz = FMT == KF_F32 ? 4 : 2;
  char* phi = static_cast<char*>(Kp) + e0 * esz;
  char* plo = FMT == KF_U24 ? reinterpret_cast<char*>(Klo) + (i0 + rl0) * ldlo + j0 + cb : nullptr;
  knm_tile_epilogue<RHS, FMT, KIND>(acc, xg_s, ws_s, rl0, m2g, zg, interior, cols_in, n - i0 - rl0, phi, ldk * esz, plo, ldlo, csum);
  if (RHS) {
    // lanes l, l + 16, l + 32, l + 48 hold the same columns: add them, then the two row halves of the tile through LDS
    double* red2 = reinterpret_cast<double*>(lds);          // the stage buffers are free: the main loop ended on a barrier
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      double c = csum[tn];
      c += __shfl_xor(c, 16);
      c += __shfl_xor(c, 32);
      if (lane < 16) red2[wr * W_BN + cb + tn] = FMT == KF_U24 ? c * 5.9604644775390625e-08 : c;   // 2^-24: exact
    }
    __syncthreads();
    if (threadIdx.x < W_BN && j0 + threadIdx.x < M)
      wslab[(i0 / W_BM) * wslab_ld + j0 + threadIdx.x] = red2[threadIdx.x] + red2[W_BN + threadIdx.x];
  }
}

// ---- a grid of kernel widths from ONE contraction (odx_gauss_knm_h2_store_sigmas)
// Nothing in the main loop depends on sigma: the accumulators hold x . z, and the width enters in the epilogue only.  This
// sibling of gauss_knm_h2w256_kernel<RHS, FMT, CORE_H2> runs the main loop once and then knm_tile_epilogue once per width
// against that width's block, planes and slab: S blocks for one contraction plus S epilogues.  Per width every constant is
// formed by the single f32 operations of the kernel above (m2g = (-2 / (s_x s_z)) * g, xg = xsq * g, zg = zsq * g; no
// contraction into a neighbouring add: fp contract is off in this body) and the epilogue is the same code: block s is bit
// for bit what the kernel above stores for sigma_s.  The widths' scaled exponents and pointers come by value.
struct KnmSigmaArgs {
  float g2[ODX_GRID_MAX_SIGMAS];              // gamma log2(e) of each width
  void* K[ODX_GRID_MAX_SIGMAS];
  unsigned char* Klo[ODX_GRID_MAX_SIGMAS];
  double* wslab[ODX_GRID_MAX_SIGMAS];
};

template <bool RHS, int FMT>
__global__ __launch_bounds__(W_THREADS, 1) void gauss_knm_sigmas_h2w256_kernel(
    const uint32_t* __restrict__ PX, int64_t ldpx, const float* __restrict__ metax, const float* __restrict__ xsq, int64_t n,
    const uint32_t* __restrict__ PZ, int64_t ldpz, const float* __restrict__ metaz, const float* __restrict__ zsq, int64_t M,
    int stages, int S, KnmSigmaArgs sg, int64_t ldk, int64_t ldlo, int gr, const double* __restrict__ w, int64_t wslab_ld) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int64_t i0, j0;
  if (!knm_place<W_BM, W_BN>(gr, n, M, i0, j0)) return;

  __shared__ __attribute__((aligned(16))) float xg_s[ODX_GRID_MAX_SIGMAS][W_BM];      // row norms times each width's gamma log2(e)
  __shared__ double ws_s[RHS ? W_BM : 1];
  if (threadIdx.x < W_BM) {
    const bool in = i0 + threadIdx.x < n;
    const float xq = in ? xsq[i0 + threadIdx.x] : 0.f;
#pragma unroll 1
    for (int s = 0; s < S; ++s) xg_s[s][threadIdx.x] = in ? xq * sg.g2[s] : 0.f;
    if (RHS) ws_s[threadIdx.x] = in ? w[i0 + threadIdx.x] : 0.0;   // rows past the end weigh nothing
  }

  f32x4 acc[8][4];
  w_zero(acc);
  w_mainloop_dma<true, CORE_H2>(acc, PX, ldpx, n, PZ, ldpz, M, i0, j0, stages, lds);      // its barriers also publish xg_s

  const float m2 = -2.f / (metax[0] * metaz[0]);            // the scales are powers of two: exact
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int cb = wc * 64 + 4 * (lane & 15);                 // first of this lane's four adjacent columns inside the tile
  const int rl0 = wr * 128 + 4 * (lane >> 4);               // first of this lane's rows inside the tile
  const int64_t mpad = FMT == KF_F32 ? ((M + 3) & ~int64_t(3)) : ((M + 7) & ~int64_t(7));
  const bool interior = i0 + W_BM <= n && j0 + W_BN <= M;
  const bool cols_in = j0 + cb < mpad;                      // groups of four: entirely inside the padded row or not at all
  float zq[4];
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) zq[tn] = j0 + cb + tn < M ? zsq[j0 + cb + tn] : 0.f;
  const int64_t e0 = (i0 + rl0) * ldk + j0 + cb;            // this lane's first entry
  const int esz = FMT == KF_F32 ? 4 : 2;
  // the accumulators stay live across the S epilogues; the stage buffers are free (the main loop ended on a barrier) and
  // take the S pairs of half-tile column sums in disjoint regions: one barrier for all of them
#pragma unroll 1
  for (int s = 0; s < S; ++s) {
    const float g = sg.g2[s];
    const float m2g = m2 * g;
    float zg[4];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) zg[tn] = j0 + cb + tn < M ? zq[tn] * g : -__builtin_inff();
    double csum[4] = {0.0, 0.0, 0.0, 0.0};
    // What the epilogue derives from the lane's place and the pitches (32 row offsets, 32 store predicates) does not depend
    // on s, and hoisted out of this loop it would live beside the 128 accumulators: they went to scratch.  The values are
    // made opaque per width (no instruction), so every epilogue derives them anew, as the one of the kernel above does.
    int64_t shi = ldk * esz, slo = ldlo, rows_left = n - i0 - rl0;
    int rl = rl0;
    asm volatile("" : "+s"(shi), "+s"(slo), "+v"(rows_left), "+v"(rl));
    char* phi = static_cast<char*>(sg.K[s]) + e0 * esz;
    char* plo = FMT == KF_U24 ? reinterpret_cast<char*>(sg.Klo[s]) + (i0 + rl0) * ldlo + j0 + cb : nullptr;
    knm_tile_epilogue<RHS, FMT>(acc, xg_s[s], ws_s, rl, m2g, zg, interior, cols_in, rows_left, phi, shi, plo, slo, csum);
    if (RHS) {
      double* red2 = reinterpret_cast<double*>(lds) + s * 2 * W_BN;
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        double c = csum[tn];
        c += __shfl_xor(c, 16);
        c += __shfl_xor(c, 32);
        if (lane < 16) red2[wr * W_BN + cb + tn] = FMT == KF_U24 ? c * 5.9604644775390625e-08 : c;   // 2^-24: exact
      }
    }
  }
  if (RHS) {
    __syncthreads();
    if (threadIdx.x < W_BN && j0 + threadIdx.x < M) {
#pragma unroll 1
      for (int s = 0; s < S; ++s) {
        const double* red2 = reinterpret_cast<const double*>(lds) + s * 2 * W_BN;
        sg.wslab[s][(i0 / W_BM) * wslab_ld + j0 + threadIdx.x] = red2[threadIdx.x] + red2[W_BN + threadIdx.x];
      }
    }
  }
}

// ---------------------------------------------------------------- plain products on the split tile cores
// out (m x n) = act(A B' + bias[col] + residual) for operands in the packed two-term f16 form (odx_split_f16): the f32
// product at f32 accuracy on the f16 matrix cores, 3 MFMAs per product — ~3 x the rate of the f32 MFMA path for the
// GEMM-shaped layers of the feature forward (the conv5 head as row GEMMs).  Same tile order and main loops as the
// Gaussian builds; the epilogue scales by 1 / (s_A s_B) (powers of two: exact) and adds bias / residual, optional ReLU.
__device__ __forceinline__ float gemm_h2_finish(float acc, float inv, float b, const float* __restrict__ res_entry, int relu) {
  float v = fmaf(acc, inv, b);
  if (res_entry != nullptr) v += *res_entry;
  return relu ? fmaxf(v, 0.f) : v;
}

// max |out| of a launch for the NEXT layer's packing (odx_split_f16_premax scales by it): every lane keeps the largest
// magnitude it stored, a wave adds ONE atomic — the absmax pass over the activation (a read of the whole matrix per layer)
// is not made.  amax: the IEEE bits of a non-negative float, 0 on entry.
__device__ __forceinline__ void gemm_h2_publish_max(unsigned int mx, unsigned int* __restrict__ amax) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off));
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(amax, mx);
}

// A layer of a CHAIN writes its output as the next layer's operand: the packed two-term split (odx_split_f16's form) straight
// from the accumulators, beside or instead of the f32 matrix — no split pass (a read and a write of the whole activation per
// layer) and, for an activation only GEMMs consume, no f32 copy at all.  The packing scale must be known BEFORE the maximum
// of the output is: it comes from a bound, max |out| <= amax(A) bound_w + bound_add + amax(residual) with bound_w >= sqrt(K)
// max_j |B_j|_2 (Cauchy-Schwarz) and bound_add >= max |bias| — the caller's promise.  A bound that is 2^b too generous costs
// b of the ~17 binades below the maximum in which the split keeps its full 22 bits; the absolute error stays below 2^-39+b of
// the maximum (f32's own rounding of the maximum: 2^-24).  meta[0] = the scale, meta[1] = the TRUE maximum (for the next
// layer's bound), as odx_split_f16 leaves them.
struct H2PackOut {
  uint32_t* P;             // nullptr: no packed output
  int64_t ldp;             // row stride, 4-byte units
  float* meta;             // (scale, max bits); meta[1] is what `amax` points at
  float bound_w, bound_add;
  const float* rmeta;      // the residual's meta words (its maximum in [1]) or nullptr
};

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float h2_chain_scale(const H2PackOut& po, const float* __restrict__ metaa) {
  float bound = metaa[1] * po.bound_w + po.bound_add;
  if (po.rmeta != nullptr) bound += po.rmeta[1];
  bound *= 1.001f;                                   // (the f32 sums round: a hair of slack; the scale has 4 x headroom anyway)
  return h2_scale_from_absmax(__float_as_uint(bound));
}

// The epilogue of both plain-product kernels.  A lane holds, for each of its TM row blocks (rows rb + 16 tm + q, q = 0..3), the
// four ADJACENT columns col .. col + 3 (B rows fetched in the permuted order): bias / residual / f32 output move 16 bytes per
// lane, the packed output 8 + 8.
template <int TM>
__device__ __forceinline__ void gemm_h2_store(const f32x4 (&acc)[TM][4], float inv, int64_t m, int64_t n, int64_t rb, int64_t col,
                                              const float* __restrict__ metaa, const float* __restrict__ bias,
                                              const float* __restrict__ res, int64_t ldr, int relu, float* __restrict__ out,
                                              int64_t ldo, unsigned int* __restrict__ amax, const H2PackOut& pk) {
  unsigned int mx = 0;
  float so = 1.f;
  if (pk.P != nullptr) {
    so = h2_chain_scale(pk, metaa);
    if (blockIdx.x == 0 && threadIdx.x == 0) pk.meta[0] = so;
  }
  const int64_t ncols = pk.P != nullptr ? ((n + H2_KT - 1) / H2_KT) * H2_KT : n;     // the packed rows are zero up to a whole k-tile
  if (col < ncols) {
    const bool full = col + 4 <= n;
    const bool vec = full && (out == nullptr || (ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0)) &&
                     (res == nullptr || (ldr % 4 == 0 && (reinterpret_cast<uintptr_t>(res) & 15u) == 0));
    float b[4];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) b[tn] = (bias != nullptr && col + tn < n) ? bias[col + tn] : 0.f;
    // running addresses: a 64-bit row * ld product per store is a quarter-rate multiply chain
    float* po = out != nullptr ? out + rb * ldo + col : nullptr;
    const float* pr = res != nullptr ? res + rb * ldr + col : nullptr;
    // packed form: granule col / 32 of the row = 32 f16 "hi" then 32 f16 "lo"; this lane's four columns are 8 + 8 bytes
    uint32_t* pp = pk.P != nullptr ? pk.P + rb * pk.ldp + (col >> 5) * 32 + ((col & 31) >> 1) : nullptr;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      // the four identity rows of this block are requested before the first of them is used: one load at a time in front of
      // its three stores left the epilogue of the K = 512 products of the conv5 head waiting on HBM latency row by row
      f32x4 rq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        rq[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (vec && pr != nullptr && rb + tm * 16 + q < m) rq[q] = *reinterpret_cast<const f32x4*>(pr + (int64_t)q * ldr);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (rb + tm * 16 + q < m) {
          f32x4 v;
          if (vec) {
            const f32x4 r4 = rq[q];
#pragma unroll
            for (int tn = 0; tn < 4; ++tn) {
              v[tn] = fmaf(acc[tm][tn][q], inv, b[tn]) + r4[tn];
              if (relu) v[tn] = fmaxf(v[tn], 0.f);
            }
            if (po != nullptr) *reinterpret_cast<f32x4*>(po) = v;
          } else {
#pragma unroll
            for (int tn = 0; tn < 4; ++tn) {
              v[tn] = col + tn < n ? gemm_h2_finish(acc[tm][tn][q], inv, b[tn], pr != nullptr ? pr + tn : nullptr, relu) : 0.f;
              if (po != nullptr && col + tn < n) po[tn] = v[tn];
            }
          }
          f16x4 hi, lo;
#pragma unroll
          for (int tn = 0; tn < 4; ++tn) {
            mx = max(mx, __float_as_uint(v[tn]) & 0x7fffffffu);
            const float t = v[tn] * so;
            hi[tn] = (_Float16)t;
            lo[tn] = (_Float16)(t - (float)hi[tn]);
          }
          if (pp != nullptr) {
            *reinterpret_cast<f16x4*>(pp) = hi;
            *reinterpret_cast<f16x4*>(pp + 16) = lo;
          }
        }
        if (po != nullptr) po += ldo;
        if (pr != nullptr) pr += ldr;
        if (pp != nullptr) pp += pk.ldp;
      }
      if (po != nullptr) po += 12 * ldo;
      if (pr != nullptr) pr += 12 * ldr;
      if (pp != nullptr) pp += 12 * pk.ldp;
    }
  }
  if (amax != nullptr) gemm_h2_publish_max(mx, amax);
}

template <bool TAPS = false>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_h2s16_kernel(
    const uint32_t* __restrict__ PA, int64_t ldpa, const float* __restrict__ metaa, int64_t m, const uint32_t* __restrict__ PB,
    int64_t ldpb, const float* __restrict__ metab, int64_t n, int ktiles, const float* __restrict__ bias,
    const float* __restrict__ res, int64_t ldr, int relu, float* __restrict__ out, int64_t ldo, int gr,
    unsigned int* __restrict__ amax, H2PackOut pk, int tapH, int tapW, int tapC) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int64_t GR = gr;
  const int64_t tiles_n = (n + GEMM_BN - 1) / GEMM_BN;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * tiles_n), within = wg % (GR * tiles_n);
  const int64_t i0 = (band * GR + within % GR) * GEMM_BM, j0 = (within / GR) * GEMM_BN;
  if (i0 >= m) return;
  f32x4 acc[4][4];
  s16_zero(acc);
  s16_mainloop<S16_H2, true, TAPS>(acc, PA, ldpa, m, PB, ldpb, n, i0, j0, ktiles, lds, tapH, tapW, tapC);
  const float inv = 1.f / (metaa[0] * metab[0]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  gemm_h2_store<4>(acc, inv, m, n, i0 + wr * 64 + 4 * (lane >> 4), j0 + wc * 64 + 4 * (lane & 15), metaa, bias, res, ldr, relu, out, ldo,
                   amax, pk);
}

template <bool TAPS = false>
__global__ __launch_bounds__(W_THREADS, 1) void gemm_h2w256_kernel(
    const uint32_t* __restrict__ PA, int64_t ldpa, const float* __restrict__ metaa, int64_t m, const uint32_t* __restrict__ PB,
    int64_t ldpb, const float* __restrict__ metab, int64_t n, int stages, const float* __restrict__ bias,
    const float* __restrict__ res, int64_t ldr, int relu, float* __restrict__ out, int64_t ldo, int gr,
    unsigned int* __restrict__ amax, int tapH, int tapW, int tapC, H2PackOut pk) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int64_t GR = gr;
  const int64_t tiles_n = (n + W_BN - 1) / W_BN;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * tiles_n), within = wg % (GR * tiles_n);
  const int64_t i0 = (band * GR + within % GR) * W_BM, j0 = (within / GR) * W_BN;
  if (i0 >= m) return;
  f32x4 acc[8][4];
  w_zero(acc);
  // B rows in the permuted order of the K_nM builds: a lane holds four ADJACENT output columns 64 wc + 4 (lane & 15) + tn
  // of each of its rows, and stores them (loads bias / residual) 16 bytes at a time when the matrices allow it
  w_mainloop_dma<true, CORE_H2, TAPS>(acc, PA, ldpa, m, PB, ldpb, n, i0, j0, stages, lds, tapH, tapW, tapC * 4);
  const float inv = 1.f / (metaa[0] * metab[0]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  gemm_h2_store<8>(acc, inv, m, n, i0 + wr * 128 + 4 * (lane >> 4), j0 + wc * 64 + 4 * (lane & 15), metaa, bias, res, ldr, relu, out, ldo,
                   amax, pk);
}

// ---------------------------------------------------------------- 16-bit operands (bf16 / f16), one term
// out = act(A B' + bias (+ residual)) for plain 16-bit row-major operands — the layers of a forward run in bf16 / f16 (BASELINE
// config 2's stated dtype): no split, no scale, TWO MFMAs per product block and 64 features where the f32-accurate form needs
// three per 32.  An operand row is its features back to back, zero beyond K up to a multiple of 128 (the 128 x 128 core's
// k-tile; the wide core consumes 64 per stage), 16-byte aligned: a row-major bf16 matrix with K % 128 == 0 IS the operand.
// Sums in f32; the result is rounded ONCE (bias and residual are added in f32 before it) to the operands' type, or left f32.
template <int CORE>
__device__ __forceinline__ float b16_load(const unsigned short* p) {
  if (CORE == CORE_BF16) return __uint_as_float((uint32_t)*p << 16);
  return (float)__builtin_bit_cast(_Float16, *p);
}

template <int CORE>
__device__ __forceinline__ unsigned short b16_round(float v) {
  if (CORE == CORE_BF16) {
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);     // NaN stays NaN
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                     // round to nearest even
  }
  return __builtin_bit_cast(unsigned short, (_Float16)v);
}

template <int CORE, bool OUT16>
__device__ __forceinline__ void b16_finish(float acc, float b, const void* __restrict__ res, int64_t ri, int relu, void* __restrict__ out,
                                           int64_t oi) {
  float v = acc + b;
  if (res != nullptr) v += OUT16 ? b16_load<CORE>(static_cast<const unsigned short*>(res) + ri) : static_cast<const float*>(res)[ri];
  if (relu) v = fmaxf(v, 0.f);
  if (OUT16) static_cast<unsigned short*>(out)[oi] = b16_round<CORE>(v);
  else static_cast<float*>(out)[oi] = v;
}

// The epilogue of both 16-bit product kernels: a lane holds, for each of its TM row blocks, four ADJACENT columns (B rows fetched
// in the permuted order): 8 (16-bit output / residual) or 16 bytes per lane and row.
template <int TM, int CORE, bool OUT16>
__device__ __forceinline__ void gemm_b16_store(const f32x4 (&acc)[TM][4], int64_t m, int64_t n, int64_t rb, int64_t col,
                                               const float* __restrict__ bias, const void* __restrict__ res, int64_t ldr, int relu,
                                               void* __restrict__ out, int64_t ldo) {
  if (col >= n) return;
  constexpr int ESZ = OUT16 ? 2 : 4;
  const bool vec = col + 4 <= n && (ldo * ESZ) % (4 * ESZ) == 0 && (reinterpret_cast<uintptr_t>(out) & (4 * ESZ - 1)) == 0 &&
                   (res == nullptr || ((ldr * ESZ) % (4 * ESZ) == 0 && (reinterpret_cast<uintptr_t>(res) & (4 * ESZ - 1)) == 0));
  float b[4];
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) b[tn] = (bias != nullptr && col + tn < n) ? bias[col + tn] : 0.f;
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    // (the four identity rows of a block are requested before the first is used, as in gemm_h2_store)
    u16x4 rq16[4];
    f32x4 rq32[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = rb + tm * 16 + q;
      rq16[q] = u16x4{0, 0, 0, 0};
      rq32[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (vec && res != nullptr && row < m) {
        if (OUT16) rq16[q] = *reinterpret_cast<const u16x4*>(static_cast<const unsigned short*>(res) + row * ldr + col);
        else rq32[q] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(res) + row * ldr + col);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = rb + tm * 16 + q;
      if (row >= m) continue;
      if (vec) {
        float v[4];
        if (OUT16) {
          const u16x4 r4 = rq16[q];
          u16x4 o;
#pragma unroll
          for (int tn = 0; tn < 4; ++tn) {
            v[tn] = acc[tm][tn][q] + b[tn];
            if (res != nullptr) { const unsigned short h = r4[tn]; v[tn] += b16_load<CORE>(&h); }
            if (relu) v[tn] = fmaxf(v[tn], 0.f);
            o[tn] = b16_round<CORE>(v[tn]);
          }
          *reinterpret_cast<u16x4*>(static_cast<unsigned short*>(out) + row * ldo + col) = o;
        } else {
          const f32x4 r4 = rq32[q];
          f32x4 o;
#pragma unroll
          for (int tn = 0; tn < 4; ++tn) {
            o[tn] = acc[tm][tn][q] + b[tn] + r4[tn];
            if (relu) o[tn] = fmaxf(o[tn], 0.f);
          }
          *reinterpret_cast<f32x4*>(static_cast<float*>(out) + row * ldo + col) = o;
        }
      } else {
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
          if (col + tn < n) b16_finish<CORE, OUT16>(acc[tm][tn][q], b[tn], res, row * ldr + col + tn, relu, out, row * ldo + col + tn);
      }
    }
  }
}

template <int CORE, bool OUT16, bool TAPS = false>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_b16s16_kernel(
    const uint32_t* __restrict__ PA, int64_t ldpa, int64_t m, const uint32_t* __restrict__ PB, int64_t ldpb, int64_t n, int ktiles,
    const float* __restrict__ bias, const void* __restrict__ res, int64_t ldr, int relu, void* __restrict__ out, int64_t ldo, int gr,
    int tapH, int tapW, int tapC) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int64_t GR = gr;
  const int64_t tiles_n = (n + GEMM_BN - 1) / GEMM_BN;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * tiles_n), within = wg % (GR * tiles_n);
  const int64_t i0 = (band * GR + within % GR) * GEMM_BM, j0 = (within / GR) * GEMM_BN;
  if (i0 >= m) return;
  f32x4 acc[4][4];
  s16_zero(acc);
  // (a lane holds four ADJACENT columns per row; TAPS: a k-tile is 128 channels of one tap, tapC / 2 four-byte units per tap)
  s16_mainloop<CORE, true, TAPS>(acc, PA, ldpa, m, PB, ldpb, n, i0, j0, ktiles, lds, tapH, tapW, tapC / 2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  gemm_b16_store<4, CORE, OUT16>(acc, m, n, i0 + wr * 64 + 4 * (lane >> 4), j0 + wc * 64 + 4 * (lane & 15), bias, res, ldr, relu, out, ldo);
}

// TAPS: A = the 3 x 3 neighbourhood matrix of 16-bit NHWC rows (C % 64 == 0: a stage is 64 channels of one tap), gathered inside
// the operand loads as in gemm_h2w256_kernel<.., true>; A's rows are followed by one all-zero row.
template <int CORE, bool OUT16, bool TAPS = false>
__global__ __launch_bounds__(W_THREADS, 1) void gemm_b16w256_kernel(
    const uint32_t* __restrict__ PA, int64_t ldpa, int64_t m, const uint32_t* __restrict__ PB, int64_t ldpb, int64_t n, int stages,
    const float* __restrict__ bias, const void* __restrict__ res, int64_t ldr, int relu, void* __restrict__ out, int64_t ldo, int gr,
    int tapH, int tapW, int tapC) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int64_t GR = gr;
  const int64_t tiles_n = (n + W_BN - 1) / W_BN;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * tiles_n), within = wg % (GR * tiles_n);
  const int64_t i0 = (band * GR + within % GR) * W_BM, j0 = (within / GR) * W_BN;
  if (i0 >= m) return;
  f32x4 acc[8][4];
  w_zero(acc);
  w_mainloop_dma<true, CORE, TAPS>(acc, PA, ldpa, m, PB, ldpb, n, i0, j0, stages, lds, tapH, tapW, tapC * 2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  gemm_b16_store<8, CORE, OUT16>(acc, m, n, i0 + wr * 128 + 4 * (lane >> 4), j0 + wc * 64 + 4 * (lane & 15), bias, res, ldr, relu, out, ldo);
}

// The operand of a 3 x 3 convolution (padding 1) run as a GEMM over 16-bit NHWC rows Y (R * H * W rows of C channels): row
// (r, h, w) of P holds, tap after tap, the C channels of Y's row (r, h + ky - 1, w + kx - 1), zeros outside the map and beyond
// 9 C up to ldp.  One thread per 16 bytes (8 channels).
__global__ __launch_bounds__(256) void taps3x3_b16_kernel(const unsigned short* __restrict__ Y, int64_t ldy, int H, int W, int C,
                                                          unsigned short* __restrict__ P, int64_t ldp, int64_t row0) {
  const int D = 9 * C;
  const int groups = (int)(ldp / 8);
  const int64_t row = row0 + blockIdx.y;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  u32x4 v = {0u, 0u, 0u, 0u};
  const int f = g * 8;
  if (f < D) {
    const int tap = f / C, c = f - tap * C;
    const int w = (int)(row % W), h = (int)((row / W) % H);
    const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
    if (hh >= 0 && hh < H && ww >= 0 && ww < W) v = *reinterpret_cast<const u32x4*>(Y + (row + (int64_t)(hh - h) * W + (ww - w)) * ldy + c);
  }
  *reinterpret_cast<u32x4*>(P + row * ldp + f) = v;
}

// ---------------------------------------------------------------- f64 matrices through the split core
// C (f64) = alpha (A B') + beta C for f64 operands packed as two-term f16 splits (split_f64_kernel): the products carry ~22
// bits per factor relative to the operand's largest entry, the sum is formed in f32 and scaled / added into C in f64.  Used
// for the GEMM-shaped work of the A factor of the FALKON preconditioner (T T' / M and the rank-512 updates of its Cholesky,
// dense_f64.hip) — A only PRECONDITIONS the system, so f32-accurate products are what the reference's all-f32 falkon gives
// it too — at ~6 x the rate of the f64 MFMA.  The operands' scales are powers of two chosen by the caller from a bound of
// the entries.
__global__ __launch_bounds__(256) void split_f64_kernel(const double* __restrict__ X, int64_t ldx, int64_t zsx, int64_t rows, int cols,
                                                        float s, uint32_t* __restrict__ P, int64_t ldp, int64_t zsp) {
  const int groups = (int)((cols + H2_KT - 1) / H2_KT) * 8;  // 8-column groups per row, zero padded to whole k-tiles
  const int64_t row = blockIdx.y;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= groups || row >= rows) return;
  const double* x = X + (int64_t)blockIdx.z * zsx + row * ldx + (int64_t)g * 8;
  double v[8];
  if (g * 8 + 8 <= cols) {
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
      const f64x2 a = *reinterpret_cast<const f64x2*>(x + q);
      v[q] = a[0];
      v[q + 1] = a[1];
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = (g * 8 + q < cols) ? x[q] : 0.0;
  }
  f16x8 hi, lo;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float t = (float)(v[q] * (double)s);       // (the f32 rounding is below the second term's last bit)
    const _Float16 h = (_Float16)t;
    hi[q] = h;
    lo[q] = (_Float16)(t - (float)h);
  }
  uint32_t* dst = P + (int64_t)blockIdx.z * zsp + row * ldp + (int64_t)(g >> 2) * 32 + (g & 3) * 4;
  *reinterpret_cast<f16x8*>(dst) = hi;
  *reinterpret_cast<f16x8*>(dst + 16) = lo;
}

struct H2F64Params {
  const uint32_t* PA; int64_t ldpa, zsa, bsa;  // packed A (m x k); class / block strides in 4-byte units
  const uint32_t* PB; int64_t ldpb, zsb, bsb;  // packed B (n x k)
  double* C; int64_t ldc, zsc, bsc;
  double* C2; int64_t ldc2, zsc2, bsc2;        // optional transposed copy C2[j, i]
  int64_t m, n, k;
  int64_t rg_total, rg_off, rg_step;           // ragged blocks: m_b = clamp(total - off - b step, 0, m)
  int k_is_m;                                  // k_b = m_b
  int flags;                                   // ODX_GEMM_LOWER_ONLY | A_UPPER | B_UPPER | A_LOWER | B_LOWER | STORE_T
  double beta;
  double alpha[ODX_MAX_ZBATCH];                // per class, 1 / (s_A s_B) folded in
};

// The same packing for a batch of blocks of f64 matrices (the pairs of a triangular-inverse merge level, for every class):
// block (b, z) starts bsx * b + zsx * z doubles into X and has rows_b x cols_b entries, rows_b / cols_b = the ragged extent
// clamp(total - off - b step, 0, rows / cols) where asked for (the last pair of a level may be short).  Rows past rows_b are
// not written (the products clamp their row reads), columns past cols_b are written as zeros up to a whole k-tile.
struct SplitBlocks {
  const double* X; int64_t ldx, bsx, zsx;
  uint32_t* P; int64_t ldp, bsp, zsp;
  int64_t rows, cols;                         // extent of a full block
  int64_t rg_total, rg_off, rg_step;          // ragged extent: total - off - b * step
  int rows_ragged, cols_ragged, Z;
  float s;
};

__global__ __launch_bounds__(256) void split_f64_blocks_kernel(SplitBlocks p) {
  const int b = blockIdx.z / p.Z, z = blockIdx.z % p.Z;
  int64_t rg = p.rg_total - p.rg_off - (int64_t)b * p.rg_step;
  const int64_t rows = p.rows_ragged ? (rg < p.rows ? (rg > 0 ? rg : 0) : p.rows) : p.rows;
  const int64_t cols = p.cols_ragged ? (rg < p.cols ? (rg > 0 ? rg : 0) : p.cols) : p.cols;
  const int64_t row = blockIdx.y;
  const int groups = (int)((cols + H2_KT - 1) / H2_KT) * 8;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= groups || row >= rows) return;
  const double* x = p.X + (int64_t)b * p.bsx + (int64_t)z * p.zsx + row * p.ldx + (int64_t)g * 8;
  double v[8];
  if (g * 8 + 8 <= cols) {
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
      const f64x2 a = *reinterpret_cast<const f64x2*>(x + q);
      v[q] = a[0];
      v[q + 1] = a[1];
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = (g * 8 + q < cols) ? x[q] : 0.0;
  }
  f16x8 hi, lo;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float t = (float)(v[q] * (double)p.s);
    const _Float16 h = (_Float16)t;
    hi[q] = h;
    lo[q] = (_Float16)(t - (float)h);
  }
  uint32_t* dst = p.P + (int64_t)b * p.bsp + (int64_t)z * p.zsp + row * p.ldp + (int64_t)(g >> 2) * 32 + (g & 3) * 4;
  *reinterpret_cast<f16x8*>(dst) = hi;
  *reinterpret_cast<f16x8*>(dst + 16) = lo;
}

__global__ __launch_bounds__(W_THREADS, 1) void gemm_h2w256_f64_kernel(H2F64Params p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int64_t GR = 4;
  const int z = blockIdx.y, b = blockIdx.z;
  int64_t m = p.m, k = p.k;
  if (p.rg_total > 0) {                                               // ragged batch: the last pair of a merge level may be short
    int64_t mb = p.rg_total - p.rg_off - (int64_t)b * p.rg_step;
    if (mb > p.m) mb = p.m;
    if (mb <= 0) return;
    m = mb;
    if (p.k_is_m) k = mb;
  }
  const int64_t tiles_n = (p.n + W_BN - 1) / W_BN;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * tiles_n), within = wg % (GR * tiles_n);
  const int64_t i0 = (band * GR + within % GR) * W_BM, j0 = (within / GR) * W_BN;
  if (i0 >= m) return;
  const bool lower = (p.flags & ODX_GEMM_LOWER_ONLY) != 0;
  if (lower && j0 > i0 + W_BM - 1) return;
  int64_t kb = 0, ke = k;                                             // operands known to be zero left of kb / right of ke
  if (p.flags & ODX_GEMM_A_UPPER) kb = i0;
  if ((p.flags & ODX_GEMM_B_UPPER) && j0 > kb) kb = j0;
  if ((p.flags & ODX_GEMM_A_LOWER) && i0 + W_BM < ke) ke = i0 + W_BM;
  if ((p.flags & ODX_GEMM_B_LOWER) && j0 + W_BN < ke) ke = j0 + W_BN;
  const int s0 = (int)(kb / W_KS);                                    // i0, j0 are multiples of 256
  const int stages = (int)((((ke + H2_KT - 1) / H2_KT) * H2_KT) / W_KS) - s0;
  f32x4 acc[8][4];
  w_zero(acc);
  if (stages > 0)
    w_mainloop_dma<true>(acc, p.PA + (int64_t)b * p.bsa + (int64_t)z * p.zsa + (int64_t)s0 * W_KS, p.ldpa, m,
                         p.PB + (int64_t)b * p.bsb + (int64_t)z * p.zsb + (int64_t)s0 * W_KS, p.ldpb, p.n, i0, j0, stages, lds);
  const double alpha = p.alpha[z], beta = p.beta;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int64_t col = j0 + wc * 64 + 4 * (lane & 15);                 // four adjacent columns per lane (permuted B rows)
  const int64_t rb = i0 + wr * 128 + 4 * (lane >> 4);
  if (col >= p.n) return;
  double* C = p.C + (int64_t)b * p.bsc + (int64_t)z * p.zsc;
  double* C2 = p.C2 ? p.C2 + (int64_t)b * p.bsc2 + (int64_t)z * p.zsc2 : nullptr;
  const bool st = (p.flags & ODX_GEMM_STORE_T) != 0;
  if (!st) {
    double* pc = C + rb * p.ldc + col;
#pragma unroll
    for (int tm = 0; tm < 8; ++tm) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t row = rb + tm * 16 + q;
        if (row < m) {
          // lower-only: what the f64 kernel's 128-row tiles write — every column up to the end of the row's 128-block
          const int64_t lim = lower ? (((row | 127) + 1 < p.n) ? (row | 127) + 1 : p.n) : p.n;
          if (col + 4 <= lim) {
            f64x2 c0 = {0.0, 0.0}, c1 = {0.0, 0.0};
            if (beta != 0.0) {
              c0 = *reinterpret_cast<const f64x2*>(pc);
              c1 = *reinterpret_cast<const f64x2*>(pc + 2);
            }
            c0[0] = fma(alpha, (double)acc[tm][0][q], beta * c0[0]);
            c0[1] = fma(alpha, (double)acc[tm][1][q], beta * c0[1]);
            c1[0] = fma(alpha, (double)acc[tm][2][q], beta * c1[0]);
            c1[1] = fma(alpha, (double)acc[tm][3][q], beta * c1[1]);
            *reinterpret_cast<f64x2*>(pc) = c0;
            *reinterpret_cast<f64x2*>(pc + 2) = c1;
          } else {
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
              if (col + tn < lim) pc[tn] = fma(alpha, (double)acc[tm][tn][q], beta != 0.0 ? beta * pc[tn] : 0.0);
          }
        }
        pc += p.ldc;
      }
      pc += 12 * p.ldc;
    }
  }
  if (st || C2 != nullptr) {
    // transposed store(s): for a column, the lane's rows q = 0..3 of a row block are four adjacent doubles (beta = 0 forms only)
    double* ct = st ? C : C2;
    const int64_t ldt = st ? p.ldc : p.ldc2;
#pragma unroll
    for (int tm = 0; tm < 8; ++tm) {
      const int64_t row = rb + tm * 16;
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        if (col + tn >= p.n) continue;
        double* pt = ct + (col + tn) * ldt + row;
        if (row + 4 <= m) {
          f64x2 c0, c1;
          c0[0] = alpha * (double)acc[tm][tn][0];
          c0[1] = alpha * (double)acc[tm][tn][1];
          c1[0] = alpha * (double)acc[tm][tn][2];
          c1[1] = alpha * (double)acc[tm][tn][3];
          *reinterpret_cast<f64x2*>(pt) = c0;
          *reinterpret_cast<f64x2*>(pt + 2) = c1;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (row + q < m) pt[q] = alpha * (double)acc[tm][tn][q];
        }
      }
    }
  }
}

// Fused scoring on the 256 x 256 core: same decomposition as gauss_mmv_h2s16_kernel (row block x group of `tg` column
// tiles, f64 partial row sums per group in the slab, mmv_reduce_kernel adds the groups), 256-row blocks, 256-column tiles.
// KIND: the radial kernel of the entries (radial_value).  Columns past the group / range have a finite exponent (their norm is
// read as 0) and weight 0: no select is needed for them.
template <int CORE, int KIND = ODX_KERNEL_GAUSS>
__global__ __launch_bounds__(W_THREADS, 1) void gauss_mmv_h2w256_kernel(
    const uint32_t* __restrict__ PX, int64_t ldpx, const float* __restrict__ metax, const float* __restrict__ xsq, int64_t n,
    const uint32_t* __restrict__ PZ, int64_t ldpz, const float* __restrict__ metaz, const float* __restrict__ zsq, int stages,
    float gamma_log2e, const double* __restrict__ V, int64_t ldv, const int32_t* __restrict__ ranges, int tg, int G,
    double* __restrict__ slab, int64_t slab_ld) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ double red[4][W_BM];
  __shared__ __attribute__((aligned(16))) float xs_s[W_BM];
  constexpr int64_t GR = 8;
  const int c = blockIdx.y;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * G), within = wg % (GR * G);
  const int64_t i0 = (band * GR + within % GR) * W_BM;
  const int g = (int)(within / GR);
  const int64_t r0 = ranges[2 * c], r1 = ranges[2 * c + 1];
  const int64_t s0 = r0 + (int64_t)g * tg * W_BN;
  const int64_t s1 = (s0 + (int64_t)tg * W_BN < r1) ? s0 + (int64_t)tg * W_BN : r1;
  if (i0 >= n || s0 >= r1) return;       // mmv_reduce_kernel only visits the groups that exist
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const float m2 = core_m2<CORE>(metax, metaz);

  if (threadIdx.x < W_BM) xs_s[threadIdx.x] = (i0 + threadIdx.x < n) ? xsq[i0 + threadIdx.x] : 0.f;
  // Lane l ends every tile with two f64 sums over the tile's 64 columns of this wave: for half h of the wave's rows,
  // row slot (l & 15) of its lane quarter (slot = 4 tm' + q, row 64 h + 16 tm' + 4 (l >> 4) + q).
  double tot[2] = {0.0, 0.0};
  const bool b8 = lane & 8, b4 = lane & 4, b2 = lane & 2, b1 = lane & 1;

  for (int64_t j0 = s0; j0 < s1; j0 += W_BN) {
    f32x4 acc[8][4];
    w_zero(acc);
    w_mainloop_dma<false, CORE>(acc, PX, ldpx, n, PZ + j0 * ldpz, ldpz, r1 - j0, i0, 0, stages, lds);
    float zs[4];
    double al[4];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int64_t col = j0 + wc * 64 + tn * 16 + (lane & 15);
      const bool cv = col < s1;
      zs[tn] = cv ? zsq[col] : 0.f;
      al[tn] = cv ? V[col * ldv + c] : 0.0;     // weight 0 removes the columns past the group / range
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double w8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {       // slots j (tm' = j >> 2) and j + 8 (tm' = 2 + (j >> 2)), q = j & 3
        double v[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int tm = 4 * h + 2 * u + (j >> 2), q = j & 3;
          const float xs = xs_s[wr * 128 + tm * 16 + 4 * (lane >> 4) + q];
          v[u] = 0.0;
#pragma unroll
          for (int tn = 0; tn < 4; ++tn) {
            // (the build's shorter form — exponent from pre-scaled norms, fma + add + min — was measured here and is
            // SLOWER: 50.3 against 49.5 ms, with 125 instead of 75 GB fetched from beyond L2 per launch; how far the
            // workgroups of an XCD drift apart in k decides how often they share a fetched slice, and this form's timing
            // keeps them closer)
            float d2 = fmaf(m2, acc[tm][tn][q], xs) + zs[tn];
            d2 = fmaxf(d2, 0.f);
            v[u] = fma((double)radial_value<KIND>(d2 * gamma_log2e), al[tn], v[u]);
          }
        }
        w8[j] = QUARTER_STAGE(b8, v[0], v[1], 8);
      }
      QUARTER_STAGES_4_2(w8);
      tot[h] += QUARTER_STAGE(b1, w2[0], w2[1], 1);
    }
  }
  {
    const int slot = lane & 15;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      red[wc][wr * 128 + 64 * h + (slot >> 2) * 16 + 4 * (lane >> 4) + (slot & 3)] = tot[h];
  }
  __syncthreads();
  if (threadIdx.x < W_BM) {
    const int64_t row = i0 + threadIdx.x;
    if (row < n)
      slab[((int64_t)c * G + g) * slab_ld + row] =
          (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// Shared-centre form of gauss_mmv_h2w256_kernel (see gauss_mmvn_h2s16_kernel): the entries of a tile replace its
// accumulators, then today's weighted sum and butterflies run once per column of the group.  Same f64 operations in the
// same order per column as gauss_mmv_h2w256_kernel with the range [0, M).  The accumulators stay live through all NV
// columns (there they die as they are read), so the column sums are kept out of the registers: see `park` and `mine`.
// PERCOL: a kernel width per column (see gauss_mmvn_h2s16_kernel): the accumulators become the clamped squared distances,
// the part of an entry every width shares, and each column takes its own exp2.
// KIND: the radial kernel of the entries (radial_value), with one width (PERCOL = false) only.
template <int NV, int CORE, bool PERCOL, int KIND = ODX_KERNEL_GAUSS>
__global__ __launch_bounds__(W_THREADS, 1) void gauss_mmvn_h2w256_kernel(
    const uint32_t* __restrict__ PX, int64_t ldpx, const float* __restrict__ metax, const float* __restrict__ xsq, int64_t n,
    const uint32_t* __restrict__ PZ, int64_t ldpz, const float* __restrict__ metaz, const float* __restrict__ zsq, int64_t M,
    int stages, MmvnGammas gm, const double* __restrict__ V, int64_t ldv, int cbase, int T, int tg, int G,
    double* __restrict__ slab, int64_t slab_ld) {
#pragma clang fp contract(off)
  static_assert(!PERCOL || KIND == ODX_KERNEL_GAUSS, "a width per column is Gaussian-only");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ __attribute__((aligned(16))) float xs_s[W_BM];
  // The sums of the first PARK columns stay in LDS of their own for the whole kernel: 3 x 8 KiB is what the CU has left
  // beside the operand images, and the 4 NV registers of all NV sums do not fit beside the main loop's at NV = 8.
  constexpr int PARK = NV < 3 ? NV : 3;
  __shared__ double park[PARK][4][W_BM];
  constexpr int64_t GR = 8;
  const int c0 = cbase + (int)blockIdx.y * NV;
  const int nc = T - c0 < NV ? T - c0 : NV;
  const int64_t wg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t band = wg / (GR * G), within = wg % (GR * G);
  const int64_t i0 = (band * GR + within % GR) * W_BM;
  const int g = (int)(within / GR);
  const int64_t s0 = (int64_t)g * tg * W_BN;
  const int64_t s1 = (s0 + (int64_t)tg * W_BN < M) ? s0 + (int64_t)tg * W_BN : M;
  if (i0 >= n || s0 >= M) return;
  const float m2 = core_m2<CORE>(metax, metaz);
  double* red = reinterpret_cast<double*>(lds);       // [NV][4 (wc)][W_BM], over the operand images (w_mainloop_dma ends on a barrier)

  if (threadIdx.x < W_BM) xs_s[threadIdx.x] = (i0 + threadIdx.x < n) ? xsq[i0 + threadIdx.x] : 0.f;
  double tot[NV - PARK + 1][2];           // (+ 1: no empty array at NV = 2)
#pragma unroll
  for (int c = 0; c < NV - PARK; ++c) tot[c][0] = tot[c][1] = 0.0;
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* mine = &park[0][wave & 3][(wave >> 2) * 128 + 16 * ((lane & 15) >> 2) + 4 * (lane >> 4) + (lane & 3)];
#pragma unroll
    for (int c = 0; c < PARK; ++c) mine[c * 4 * W_BM] = mine[c * 4 * W_BM + 64] = 0.0;
  }

  for (int64_t j0 = s0; j0 < s1; j0 += W_BN) {
    f32x4 acc[8][4];
    w_zero(acc);
    w_mainloop_dma<false, CORE>(acc, PX, ldpx, n, PZ + j0 * ldpz, ldpz, M - j0, i0, 0, stages, lds);
    // The lane's place in the tile is derived HERE, from a thread index the compiler cannot see through: computed at kernel
    // entry, the offsets and masks below are live across the main loop beside 2 NV sums, and that is more than 256 registers.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wr = tid >> 8, wc = (tid >> 6) & 3;
    const bool b8 = lane & 8, b4 = lane & 4, b2 = lane & 2, b1 = lane & 1;
    // During the epilogue the other sums live in this lane's own slots of `red` (the operand images are free until the next
    // main loop starts), not in registers beside the accumulators; they are registers only ACROSS a main loop.
    const int slot = wc * W_BM + wr * 128 + 16 * ((lane & 15) >> 2) + 4 * (lane >> 4) + (lane & 3);
    double* mine = red + slot;
    double* parked = &park[0][0][0] + slot;
#pragma unroll
    for (int c = 0; c < NV - PARK; ++c) mine[c * 4 * W_BM] = tot[c][0], mine[c * 4 * W_BM + 64] = tot[c][1];
    float zs[4];
    const int64_t col0 = j0 + wc * 64 + (lane & 15);       // this lane's columns: col0 + 16 tn; past the group / M: weight 0
    const double* vp = V + col0 * ldv + c0;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) zs[tn] = col0 + 16 * tn < s1 ? zsq[col0 + 16 * tn] : 0.f;
#pragma unroll
    for (int tm = 0; tm < 8; ++tm)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float xs = xs_s[wr * 128 + tm * 16 + 4 * (lane >> 4) + q];
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) {    // (the form of gauss_mmv_h2w256_kernel: its bits are the contract)
          float d2 = fmaf(m2, acc[tm][tn][q], xs) + zs[tn];
          d2 = fmaxf(d2, 0.f);
          acc[tm][tn][q] = PERCOL ? d2 : radial_value<KIND>(d2 * gm.g[0]);
        }
      }
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      mmvn_fresh(acc);
      const float gc = gm.g[c];
      double al[4];
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) al[tn] = (col0 + 16 * tn < s1 && c < nc) ? vp[16 * tn * ldv + c] : 0.0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double w8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {       // slots j (tm' = j >> 2) and j + 8 (tm' = 2 + (j >> 2)), q = j & 3
          double v[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int tm = 4 * h + 2 * u + (j >> 2), q = j & 3;
            v[u] = 0.0;
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
              v[u] = fma((double)(PERCOL ? __builtin_amdgcn_exp2f(acc[tm][tn][q] * gc) : acc[tm][tn][q]), al[tn], v[u]);
          }
          w8[j] = QUARTER_STAGE(b8, v[0], v[1], 8);
        }
        QUARTER_STAGES_4_2(w8);
        double* sum = c < PARK ? parked + c * 4 * W_BM + 64 * h : mine + (c - PARK) * 4 * W_BM + 64 * h;
        *sum += QUARTER_STAGE(b1, w2[0], w2[1], 1);
      }
    }
    if (j0 + W_BN < s1) {
#pragma unroll
      for (int c = 0; c < NV - PARK; ++c) tot[c][0] = mine[c * 4 * W_BM], tot[c][1] = mine[c * 4 * W_BM + 64];
    }
    __syncthreads();                  // the next main loop writes the images at once; behind the last tile: `red` is complete
  }
  if (threadIdx.x < W_BM) {
    const int64_t row = i0 + threadIdx.x;
    if (row < n)
      for (int c = 0; c < nc; ++c) {
        const double* rc = (c < PARK ? &park[0][0][0] + c * 4 * W_BM : red + (c - PARK) * 4 * W_BM) + threadIdx.x;
        slab[((int64_t)(c0 + c) * G + g) * slab_ld + row] = (rc[0] + rc[W_BM]) + (rc[2 * W_BM] + rc[3 * W_BM]);
      }
  }
}

constexpr int MMV_TG = 4;   // column tiles per workgroup (2 / 4 / 8 / 16 / 40 measured: 342 / 341 / 335 / 321 / 305 TF)

constexpr int W_MMV_TG = 2; // column tiles per workgroup on the 256 x 256 core (1 / 2 / 4 / 8 measured: 409 / 419 / 412 / 395 TF)

static int h2_enable_lds(const void* fn, int bytes = S16_LDS_BYTES) {   // > 64 KiB of LDS per workgroup has to be asked for
  ODX_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return ODX_OK;
}

// Tile core for a launch of `tiles256` 256 x 256 tiles: the wide core once it fills the chip twice over, the 128 x 128
// core (4 x as many, smaller workgroups) below that.  The option h2_tile (odx_set_option / odx_set_h2_tile: 128 | 256) pins one
// (tests, measurements).  The wide core stages its operands by LDS-DMA (round 4: 0.925 / 0.900 of the register-staged loop's
// times in same-process A/B runs; the register-staged instantiations are gone).
static bool h2_use_w256(int64_t tiles256) {
  const int t = lib_option(OPT_H2_TILE);
  if (t == 128) return false;
  if (t == 256) return true;
  return tiles256 >= 512;
}

// the kernels' scaled exponent: exp(-d^2 / (2 sigma^2)) = exp2(d^2 gamma log2(e))
static float h2_gamma_log2e(double sigma) { return (float)(-0.5 / (sigma * sigma)) * LOG2E; }

// The pair of packed operands of a Gaussian entry `who`; dp: the least ld (4-byte units) its tile core reads.
static int check_packed_pair(const char* who, int64_t dp, int64_t ldpx, int64_t ldpz, const void* PX, const void* PZ) {
  ODX_REQUIRE(ldpx % 4 == 0 && ldpz % 4 == 0 && ldpx >= dp && ldpz >= dp && aligned16(PX) && aligned16(PZ),
              "%s: packed operands must be 16-byte aligned with ld %% 4 == 0 and ld >= %lld 4-byte units", who, (long long)dp);
  ODX_REQUIRE(ldpx < (1 << 24) && ldpz < (1 << 24), "%s: leading dimensions must stay below 2^24 (32-bit tile offsets)", who);
  return ODX_OK;
}

// A stored K_nM block in format fmt (ODX_KNM_*) and, for the 24-bit format, its low-byte plane.
static int check_knm_block(const char* who, int fmt, int64_t M, const void* K, int64_t ldk, const void* Klo, int64_t ldlo) {
  const int64_t ldmin = odx_knm_ld(M, fmt);
  ODX_REQUIRE(K && ldk >= ldmin && ldk % (fmt == ODX_KNM_F32 ? 4 : 8) == 0 && aligned16(K),
              "%s: K must be 16-byte aligned with ldk a multiple of %d and >= %lld", who, fmt == ODX_KNM_F32 ? 4 : 8, (long long)ldmin);
  if (fmt == ODX_KNM_U24)
    ODX_REQUIRE(Klo && ldlo >= ldmin && ldlo % 8 == 0 && aligned16(Klo), "%s: the low-byte plane must be 16-byte aligned with ldlo %% 8 == 0, ldlo >= roundup(M, 8)", who);
  ODX_REQUIRE(ldk < (1 << 24), "%s: leading dimensions must stay below 2^24 (32-bit tile offsets)", who);
  return ODX_OK;
}

// (internal, odx_internal.h) packed bytes of a (rows x cols) f64 operand of gemm_h2_f64
int64_t h2_f64_packed_ld(int64_t cols) { return round_up(cols, H2_KT); }

int split_f64(const double* X, int64_t ldx, int64_t zsx, int64_t rows, int64_t cols, float scale, uint32_t* P, int64_t ldp,
              int64_t zsp, int z, hipStream_t stream) {
  if (rows <= 0 || cols <= 0 || z <= 0) return ODX_OK;
  ODX_REQUIRE(ldx % 2 == 0 && aligned16(X) && zsx % 2 == 0, "split_f64: X must be 16-byte aligned with even ld / class stride");
  ODX_REQUIRE(ldp % 4 == 0 && ldp >= round_up(cols, H2_KT) && aligned16(P) && zsp % 4 == 0, "split_f64: packed rows cover roundup(cols, 64)");
  ODX_REQUIRE(rows < 65536 && z < 65536, "split_f64: too many rows");
  const int groups = (int)(round_up(cols, H2_KT) / 8);
  hipLaunchKernelGGL(split_f64_kernel, dim3((unsigned)ceil_div(groups, 256), (unsigned)rows, (unsigned)z), dim3(256), 0, stream, X, ldx, zsx,
                     rows, (int)cols, scale, P, ldp, zsp);
  ODX_CHECK_LAUNCH("split_f64");
  return ODX_OK;
}

int split_f64_blocks(const SplitBlocksArgs& a, hipStream_t stream) {
  if (a.rows <= 0 || a.cols <= 0 || a.nb <= 0 || a.Z <= 0) return ODX_OK;
  ODX_REQUIRE(a.ldx % 2 == 0 && aligned16(a.X) && a.zsx % 2 == 0 && a.bsx % 2 == 0, "split_f64_blocks: X blocks must be 16-byte aligned");
  ODX_REQUIRE(a.ldp % 4 == 0 && a.ldp >= round_up(a.cols, H2_KT) && aligned16(a.P) && a.zsp % 4 == 0 && a.bsp % 4 == 0,
              "split_f64_blocks: packed rows cover roundup(cols, 64)");
  ODX_REQUIRE(a.rows < 65536 && (int64_t)a.nb * a.Z < 65536, "split_f64_blocks: too many rows / blocks");
  SplitBlocks p;
  p.X = a.X; p.ldx = a.ldx; p.bsx = a.bsx; p.zsx = a.zsx; p.P = a.P; p.ldp = a.ldp; p.bsp = a.bsp; p.zsp = a.zsp;
  p.rows = a.rows; p.cols = a.cols; p.rg_total = a.rg_total; p.rg_off = a.rg_off; p.rg_step = a.rg_step;
  p.rows_ragged = a.rows_ragged; p.cols_ragged = a.cols_ragged; p.Z = a.Z; p.s = a.scale;
  const int groups = (int)(round_up(a.cols, H2_KT) / 8);
  hipLaunchKernelGGL(split_f64_blocks_kernel, dim3((unsigned)ceil_div(groups, 256), (unsigned)a.rows, (unsigned)(a.nb * a.Z)), dim3(256), 0,
                     stream, p);
  ODX_CHECK_LAUNCH("split_f64_blocks");
  return ODX_OK;
}

int gemm_h2_f64_ex(const H2F64Args& a, hipStream_t stream) {
  if (a.m <= 0 || a.n <= 0 || a.zcount <= 0 || a.nb <= 0) return ODX_OK;
  ODX_REQUIRE(a.zcount <= ODX_MAX_ZBATCH && a.nb < 65536 && a.ldc % 2 == 0 && a.zsc % 2 == 0 && a.bsc % 2 == 0 && aligned16(a.C),
              "gemm_h2_f64: C must be 16-byte aligned, even ld / strides");
  ODX_REQUIRE(a.C2 == nullptr || (a.ldc2 % 2 == 0 && a.zsc2 % 2 == 0 && a.bsc2 % 2 == 0 && aligned16(a.C2)), "gemm_h2_f64: C2 alignment");
  ODX_REQUIRE(!(a.flags & ODX_GEMM_STORE_T) || a.beta == 0.0, "gemm_h2_f64: a transposed store cannot accumulate");
  ODX_REQUIRE(a.ldpa < (1 << 24) && a.ldpb < (1 << 24) && a.ldpa >= round_up(a.k, H2_KT) && a.ldpb >= round_up(a.k, H2_KT),
              "gemm_h2_f64: packed leading dimensions");
  H2F64Params p;
  p.PA = a.PA; p.ldpa = a.ldpa; p.zsa = a.zsa; p.bsa = a.bsa; p.PB = a.PB; p.ldpb = a.ldpb; p.zsb = a.zsb; p.bsb = a.bsb;
  p.C = a.C; p.ldc = a.ldc; p.zsc = a.zsc; p.bsc = a.bsc; p.C2 = a.C2; p.ldc2 = a.ldc2; p.zsc2 = a.zsc2; p.bsc2 = a.bsc2;
  p.m = a.m; p.n = a.n; p.k = a.k; p.rg_total = a.rg_total; p.rg_off = a.rg_off; p.rg_step = a.rg_step; p.k_is_m = a.k_is_m;
  p.flags = a.flags; p.beta = a.beta;
  for (int z = 0; z < a.zcount; ++z) p.alpha[z] = a.alpha[z] / ((double)a.sa * (double)a.sb);
  const int64_t wt = round_up(ceil_div(a.m, W_BM), 4) * ceil_div(a.n, W_BN);
  ODX_REQUIRE(wt < (1ll << 31), "gemm_h2_f64: grid too large");
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_h2w256_f64_kernel), W_LDS_BYTES));
  hipLaunchKernelGGL(gemm_h2w256_f64_kernel, dim3((unsigned)wt, (unsigned)a.zcount, (unsigned)a.nb), dim3(W_THREADS), W_LDS_BYTES, stream, p);
  ODX_CHECK_LAUNCH("gemm_h2_f64");
  return ODX_OK;
}

// C_z = alpha_z (A_z B_z') / (sa sb) + beta C_z for z = 0 .. zcount - 1; k = columns of the operands
int gemm_h2_f64(const uint32_t* PA, int64_t ldpa, int64_t zsa, float sa, const uint32_t* PB, int64_t ldpb, int64_t zsb, float sb,
                double* C, int64_t ldc, int64_t zsc, int64_t m, int64_t n, int64_t k, const double* alpha, double beta, int flags,
                int zcount, hipStream_t stream) {
  H2F64Args a;
  a.PA = PA; a.ldpa = ldpa; a.zsa = zsa; a.sa = sa; a.PB = PB; a.ldpb = ldpb; a.zsb = zsb; a.sb = sb;
  a.C = C; a.ldc = ldc; a.zsc = zsc; a.m = m; a.n = n; a.k = k; a.beta = beta; a.flags = flags; a.zcount = zcount;
  for (int z = 0; z < zcount && z < ODX_MAX_ZBATCH; ++z) a.alpha[z] = alpha[z];
  return gemm_h2_f64_ex(a, stream);
}

}  // namespace odx

using namespace odx;

extern "C" int odx_set_option(const char* name, int value);
extern "C" int odx_set_h2_tile(int tile) {
  ODX_REQUIRE(tile == 0 || tile == 128 || tile == 256, "odx_set_h2_tile: tile must be 0 (automatic), 128 or 256");
  return odx_set_option("h2_tile", tile);
}

extern "C" int odx_split_f16(const float* X, int64_t ldx, int64_t n, int D, void* P, int64_t ldp, float* meta,
                             odx_stream_t stream) {
  ODX_REQUIRE(meta, "odx_split_f16: meta is null");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(meta_zero_kernel, dim3(1), dim3(64), 0, s, meta);
  if (n <= 0) {
    // scale of an empty matrix: 1
    hipLaunchKernelGGL(split_f16_kernel, dim3(1, 1), dim3(256), 0, s, X, ldx, 0, 0, (uint32_t*)P, ldp, meta);
    ODX_CHECK_LAUNCH("odx_split_f16");
    return ODX_OK;
  }
  ODX_REQUIRE(X && P && D > 0 && ldx >= D && ldx % 4 == 0 && aligned16(X), "odx_split_f16: X must be 16-byte aligned with ldx %% 4 == 0 and ldx >= D");
  ODX_REQUIRE(ldp >= round_up(D, H2_KT) && ldp % 4 == 0 && aligned16(P), "odx_split_f16: P must be 16-byte aligned, ldp %% 4 == 0, ldp >= roundup(D, 64)");
  const unsigned blocks = (unsigned)(ceil_div(n, 4) > 1024 ? 1024 : ceil_div(n, 4));
  hipLaunchKernelGGL(absmax_f32_kernel, dim3(blocks), dim3(256), 0, s, X, ldx, n, D, reinterpret_cast<unsigned int*>(meta + 1));
  ODX_CHECK_LAUNCH("odx_split_f16(absmax)");
  const int groups = (int)ceil_div(D, H2_KT) * 8;
  ODX_REQUIRE(ceil_div(n * groups, 256) < (1ll << 31), "odx_split_f16: too many rows");
  hipLaunchKernelGGL(split_f16_kernel, dim3((unsigned)ceil_div(n * groups, 256)), dim3(256), 0, s, X, ldx, n, D, (uint32_t*)P, ldp, meta);
  ODX_CHECK_LAUNCH("odx_split_f16");
  return ODX_OK;
}

// odx_split_f16 for a matrix whose largest |entry| is already in meta[1] (odx_row_sqnorm_absmax_f32 left it there with the
// row norms): the packing only — no memset, no pass over the matrix for the maximum.
extern "C" int odx_split_f16_premax(const float* X, int64_t ldx, int64_t n, int D, void* P, int64_t ldp, float* meta,
                                    odx_stream_t stream) {
  ODX_REQUIRE(meta, "odx_split_f16_premax: meta is null");
  hipStream_t s = as_stream(stream);
  if (n <= 0) {
    hipLaunchKernelGGL(split_f16_kernel, dim3(1, 1), dim3(256), 0, s, X, ldx, 0, 0, (uint32_t*)P, ldp, meta);
    ODX_CHECK_LAUNCH("odx_split_f16_premax");
    return ODX_OK;
  }
  ODX_REQUIRE(X && P && D > 0 && ldx >= D && ldx % 4 == 0 && aligned16(X), "odx_split_f16_premax: X must be 16-byte aligned with ldx %% 4 == 0 and ldx >= D");
  ODX_REQUIRE(ldp >= round_up(D, H2_KT) && ldp % 4 == 0 && aligned16(P), "odx_split_f16_premax: P must be 16-byte aligned, ldp %% 4 == 0, ldp >= roundup(D, 64)");
  const int groups = (int)ceil_div(D, H2_KT) * 8;
  ODX_REQUIRE(ceil_div(n * groups, 256) < (1ll << 31), "odx_split_f16_premax: too many rows");
  hipLaunchKernelGGL(split_f16_kernel, dim3((unsigned)ceil_div(n * groups, 256)), dim3(256), 0, s, X, ldx, n, D, (uint32_t*)P, ldp, meta);
  ODX_CHECK_LAUNCH("odx_split_f16_premax");
  return ODX_OK;
}

// The build instantiation for (w != nullptr, storage format): launch(RHS, FMT) gets the two as integral constants.
static_assert(KF_F32 == ODX_KNM_F32 && KF_U24 == ODX_KNM_U24 && KF_BF16 == ODX_KNM_BF16, "the kernels' FMT is the interface's fmt");
template <bool B> using BoolC = std::integral_constant<bool, B>;
template <int I> using IntC = std::integral_constant<int, I>;
template <typename L>
static int knm_rhs_fmt(bool rhs, int kf, L&& launch) {
  if (rhs) return kf == KF_F32 ? launch(BoolC<true>(), IntC<KF_F32>()) : kf == KF_U24 ? launch(BoolC<true>(), IntC<KF_U24>()) : launch(BoolC<true>(), IntC<KF_BF16>());
  return kf == KF_F32 ? launch(BoolC<false>(), IntC<KF_F32>()) : kf == KF_U24 ? launch(BoolC<false>(), IntC<KF_U24>()) : launch(BoolC<false>(), IntC<KF_BF16>());
}

// the band height of the wide builds' tile order (2 / 4 / 8 / 16 / 32 measured alone: 395 / 397 / 391 / 376 / 347 TF) and their grid
constexpr int W_KNM_GR = 4;
static int64_t knm_w256_grid(int64_t n, int64_t M) { return round_up(ceil_div(n, W_BM), W_KNM_GR) * ceil_div(M, W_BN); }

// The radial kernels (ODX_KERNEL_*) as the wide kernels' KIND: f(kind as an integral constant).  The Matern kinds exist on the
// 256 x 256 core with the split-f16 operands only; the entries check the kind before they get here.
static bool radial_kind_known(int kind) { return kind == ODX_KERNEL_GAUSS || kind == ODX_KERNEL_MATERN32 || kind == ODX_KERNEL_MATERN52; }
template <typename L>
static int with_matern_kind(int kind, L&& f) {
  return kind == ODX_KERNEL_MATERN32 ? f(IntC<ODX_KERNEL_MATERN32>()) : f(IntC<ODX_KERNEL_MATERN52>());
}

template <bool RHS, int FMT, int CORE, int KIND = ODX_KERNEL_GAUSS>
static int launch_knm_w256_t(unsigned wt, hipStream_t s, const uint32_t* PX, int64_t ldpx, const float* metax, const float* xsq,
                             int64_t n, const uint32_t* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M,
                             int stages, float g2, void* K, int64_t ldk, unsigned char* Klo, int64_t ldlo, int wgr,
                             const double* w, double* wslab, int64_t wslab_ld) {
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gauss_knm_h2w256_kernel<RHS, FMT, CORE, KIND>), W_LDS_BYTES));
  hipLaunchKernelGGL((gauss_knm_h2w256_kernel<RHS, FMT, CORE, KIND>), dim3(wt), dim3(W_THREADS), W_LDS_BYTES, s, PX, ldpx, metax,
                     xsq, n, PZ, ldpz, metaz, zsq, M, stages, g2, K, ldk, Klo, ldlo, wgr, w, wslab, wslab_ld);
  return ODX_OK;
}

// `core`: CORE_H2 (operands from odx_split_f16, ld in 4-byte units >= roundup(D, 64)) or CORE_F8 (operands from
// odx_split_f8, ld in 4-byte units >= roundup(D, 128) / 4) or CORE_BF16 / CORE_F16 (plain 16-bit rows, ld in 4-byte units >=
// roundup(D, 64) / 2, no meta words); `stages` = 128-byte pieces per operand row.
static int launch_knm_w256(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n, const void* PZ,
                           int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int stages, double sigma, int fmt,
                           void* K, int64_t ldk, void* Klo, int64_t ldlo, const double* w, double* wslab, int64_t wslab_ld,
                           odx_stream_t stream, int core = CORE_H2, int kind = ODX_KERNEL_GAUSS) {
  const int64_t wt = knm_w256_grid(n, M);
  ODX_REQUIRE(wt < (1ll << 31), "odx_gauss_knm_h2: grid too large");
  ODX_REQUIRE(kind == ODX_KERNEL_GAUSS || core == CORE_H2, "odx_gauss_knm_h2: a Matern kernel needs the split-f16 operands");
  const float g2 = h2_gamma_log2e(sigma);
  hipStream_t s = as_stream(stream);
  const uint32_t *px = (const uint32_t*)PX, *pz = (const uint32_t*)PZ;
  unsigned char* lo = static_cast<unsigned char*>(Klo);
  ODX_PROPAGATE(knm_rhs_fmt(w != nullptr, fmt, [&](auto rhs, auto kf) {
    constexpr bool RHS = decltype(rhs)::value;
    constexpr int FMT = decltype(kf)::value;
    if (kind != ODX_KERNEL_GAUSS)
      return with_matern_kind(kind, [&](auto k) {
        return launch_knm_w256_t<RHS, FMT, CORE_H2, decltype(k)::value>((unsigned)wt, s, px, ldpx, metax, xsq, n, pz, ldpz, metaz, zsq, M,
                                                                        stages, g2, K, ldk, lo, ldlo, W_KNM_GR, w, wslab, wslab_ld);
      });
    auto run = [&](auto c) {
      return launch_knm_w256_t<RHS, FMT, decltype(c)::value>((unsigned)wt, s, px, ldpx, metax, xsq, n, pz, ldpz, metaz, zsq, M, stages, g2, K,
                                                             ldk, lo, ldlo, W_KNM_GR, w, wslab, wslab_ld);
    };
    return core == CORE_F8 ? run(IntC<CORE_F8>()) : core == CORE_BF16 ? run(IntC<CORE_BF16>()) : core == CORE_F16 ? run(IntC<CORE_F16>())
                                                                                                                   : run(IntC<CORE_H2>());
  }));
  ODX_CHECK_LAUNCH("odx_gauss_knm_h2(w256)");
  return ODX_OK;
}

static int split_taps3x3_launch(const float* Y, int64_t ldy, int64_t R, int H, int W, int C, void* P, int64_t ldp, float* meta,
                                bool premax, odx_stream_t stream, const char* who) {
  ODX_REQUIRE(meta, "odx_split_f16_taps3x3: meta is null");
  hipStream_t s = as_stream(stream);
  if (!premax) hipLaunchKernelGGL(meta_zero_kernel, dim3(1), dim3(64), 0, s, meta);
  const int64_t n = R * H * W;
  if (n <= 0) return ODX_OK;
  ODX_REQUIRE(Y && P && H > 0 && W > 0 && C > 0 && C % 8 == 0 && ldy >= C && ldy % 4 == 0 && aligned16(Y),
              "odx_split_f16_taps3x3: Y must be 16-byte aligned with ldy %% 4 == 0, ldy >= C, C %% 8 == 0");
  const int D = 9 * C;
  ODX_REQUIRE(ldp >= round_up(D, H2_KT) && ldp % 4 == 0 && aligned16(P), "odx_split_f16_taps3x3: P must be 16-byte aligned, ldp %% 4 == 0, ldp >= roundup(9 C, 64)");
  const int groups = (int)ceil_div(D, H2_KT) * 8;
  ODX_REQUIRE(ceil_div(n * groups, 256) < (1ll << 31), "odx_split_f16_taps3x3: too many rows");
  if (!premax) {
    const unsigned blocks = (unsigned)(ceil_div(n, 4) > 1024 ? 1024 : ceil_div(n, 4));
    hipLaunchKernelGGL(absmax_f32_kernel, dim3(blocks), dim3(256), 0, s, Y, ldy, n, C, reinterpret_cast<unsigned int*>(meta + 1));
    ODX_CHECK_LAUNCH("odx_split_f16_taps3x3(absmax)");
  }
  hipLaunchKernelGGL(split_f16_taps3x3_kernel, dim3((unsigned)ceil_div(n * groups, 256)), dim3(256), 0, s, Y, ldy, H, W, C,
                     (uint32_t*)P, ldp, meta, n);
  ODX_CHECK_LAUNCH(who);
  return ODX_OK;
}

extern "C" int odx_split_f16_taps3x3(const float* Y, int64_t ldy, int64_t R, int H, int W, int C, void* P, int64_t ldp,
                                     float* meta, odx_stream_t stream) {
  return split_taps3x3_launch(Y, ldy, R, H, W, C, P, ldp, meta, false, stream, "odx_split_f16_taps3x3");
}

// The same with max |Y| already in meta[1] (odx_gemm_h2_max_f32 left it there): no maximum pass.
extern "C" int odx_split_f16_taps3x3_premax(const float* Y, int64_t ldy, int64_t R, int H, int W, int C, void* P, int64_t ldp,
                                            float* meta, odx_stream_t stream) {
  return split_taps3x3_launch(Y, ldy, R, H, W, C, P, ldp, meta, true, stream, "odx_split_f16_taps3x3_premax");
}

static int h2_pack_out(H2PackOut& pk, const char* who, float* out, int64_t n, float* out_meta, void* out_packed, int64_t ldop,
                       float bound_w, float bound_add, const float* residual_meta) {
  pk = H2PackOut{nullptr, 0, nullptr, 0.f, 0.f, nullptr};
  if (out_packed == nullptr) {
    ODX_REQUIRE(out != nullptr, "%s: neither an f32 nor a packed output", who);
    return ODX_OK;
  }
  ODX_REQUIRE(out_meta != nullptr, "%s: a packed output needs out_meta", who);
  ODX_REQUIRE(ldop % 4 == 0 && ldop >= round_up(n, H2_KT) && aligned16(out_packed), "%s: out_packed must be 16-byte aligned, ldop %% 4 == 0, ldop >= roundup(n, 64)", who);
  ODX_REQUIRE(bound_w >= 0.f && bound_add >= 0.f && bound_w == bound_w && bound_add == bound_add, "%s: bounds must be non-negative numbers", who);
  pk = H2PackOut{static_cast<uint32_t*>(out_packed), ldop, out_meta, bound_w, bound_add, residual_meta};
  return ODX_OK;
}

static int gemm_h2_launch(const void* PA, int64_t ldpa, const float* metaa, int64_t m, const void* PB, int64_t ldpb,
                          const float* metab, int64_t n, int K, const float* bias, const float* residual, int64_t ldr,
                          int relu, float* out, int64_t ldo, float* out_meta, const H2PackOut& pk, odx_stream_t stream) {
  if (m <= 0 || n <= 0) return ODX_OK;
  ODX_REQUIRE(PA && PB && metaa && metab && (out || pk.P) && K > 0, "odx_gemm_h2_f32: bad argument");
  const int64_t dp = round_up(K, H2_KT);
  ODX_REQUIRE(ldpa % 4 == 0 && ldpb % 4 == 0 && ldpa >= dp && ldpb >= dp && aligned16(PA) && aligned16(PB),
              "odx_gemm_h2_f32: packed operands must be 16-byte aligned with ld %% 4 == 0 and ld >= roundup(K, 64)");
  ODX_REQUIRE((out == nullptr || ldo >= n) && (residual == nullptr || ldr >= n), "odx_gemm_h2_f32: ldo / ldr < n");
  ODX_REQUIRE(ldpa < (1 << 24) && ldpb < (1 << 24), "odx_gemm_h2_f32: leading dimensions must stay below 2^24 (32-bit tile offsets)");
  const int gr = 8;
  unsigned int* amax = out_meta ? reinterpret_cast<unsigned int*>(out_meta + 1) : nullptr;
  const int64_t t256 = ceil_div(m, W_BM) * ceil_div(n, W_BN);
  // (a product of at most 128 columns leaves at least half of a 256-wide tile idle: the 128 x 128 core takes it)
  if (t256 >= 256 && n > GEMM_BN) {           // the 256 x 256 core once it fills the chip (one workgroup per CU), else 128 x 128 tiles
    const int64_t wt = round_up(ceil_div(m, W_BM), gr) * ceil_div(n, W_BN);
    ODX_REQUIRE(wt < (1ll << 31), "odx_gemm_h2_f32: grid too large");
    ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_h2w256_kernel<false>), W_LDS_BYTES));
    hipLaunchKernelGGL(gemm_h2w256_kernel<false>, dim3((unsigned)wt), dim3(W_THREADS), W_LDS_BYTES, as_stream(stream),
                       (const uint32_t*)PA, ldpa, metaa, m, (const uint32_t*)PB, ldpb, metab, n, (int)(dp / W_KS), bias, residual,
                       ldr, relu, out, ldo, gr, amax, 0, 0, 0, pk);
    ODX_CHECK_LAUNCH("odx_gemm_h2_f32(w256)");
    return ODX_OK;
  }
  const int64_t tiles = round_up(ceil_div(m, GEMM_BM), gr) * ceil_div(n, GEMM_BN);
  ODX_REQUIRE(tiles < (1ll << 31), "odx_gemm_h2_f32: grid too large");
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_h2s16_kernel<false>)));
  hipLaunchKernelGGL(gemm_h2s16_kernel<false>, dim3((unsigned)tiles), dim3(GEMM_THREADS), S16_LDS_BYTES, as_stream(stream),
                     (const uint32_t*)PA, ldpa, metaa, m, (const uint32_t*)PB, ldpb, metab, n, (int)(dp / H2_KT), bias, residual,
                     ldr, relu, out, ldo, gr, amax, pk, 0, 0, 0);
  ODX_CHECK_LAUNCH("odx_gemm_h2_f32");
  return ODX_OK;
}

extern "C" int odx_gemm_h2_f32(const void* PA, int64_t ldpa, const float* metaa, int64_t m, const void* PB, int64_t ldpb,
                               const float* metab, int64_t n, int K, const float* bias, const float* residual, int64_t ldr,
                               int relu, float* out, int64_t ldo, odx_stream_t stream) {
  ODX_REQUIRE(out, "odx_gemm_h2_f32: out is null");
  return gemm_h2_launch(PA, ldpa, metaa, m, PB, ldpb, metab, n, K, bias, residual, ldr, relu, out, ldo, nullptr,
                        H2PackOut{nullptr, 0, nullptr, 0.f, 0.f, nullptr}, stream);
}

// odx_gemm_h2_f32 that also leaves max |out| in out_meta[1] (IEEE bits; out_meta[1] must be 0 on entry, out_meta[0] is not
// touched): the meta words odx_split_f16_premax / odx_split_f16_taps3x3_premax pack `out` with, so a chain of layers makes no
// maximum pass over its activations.
extern "C" int odx_gemm_h2_max_f32(const void* PA, int64_t ldpa, const float* metaa, int64_t m, const void* PB, int64_t ldpb,
                                   const float* metab, int64_t n, int K, const float* bias, const float* residual, int64_t ldr,
                                   int relu, float* out, int64_t ldo, float* out_meta, odx_stream_t stream) {
  ODX_REQUIRE(out_meta && out, "odx_gemm_h2_max_f32: out / out_meta is null");
  return gemm_h2_launch(PA, ldpa, metaa, m, PB, ldpb, metab, n, K, bias, residual, ldr, relu, out, ldo, out_meta,
                        H2PackOut{nullptr, 0, nullptr, 0.f, 0.f, nullptr}, stream);
}

// A layer of a chain (H2PackOut above): odx_gemm_h2_max_f32 that ALSO (out_packed != NULL) writes its output as the next
// layer's packed operand — rows of ldop 4-byte units, ldop %% 4 == 0, ldop >= roundup(n, 64), columns n .. roundup(n, 64) zero
// — with out_meta[0] = the scale it packed with, out_meta[1] = max |out|; `out` may then be NULL (an activation only GEMMs
// read).  The caller promises  max |out| <= amax(A) bound_w + bound_add + amax(residual)  (amax(A) = metaa[1],
// amax(residual) = residual_meta[1]; residual_meta may be NULL when there is no residual): bound_w >= sqrt(K) max_j |B_j|_2,
// bound_add >= max |bias|.
extern "C" int odx_gemm_h2_chain_f32(const void* PA, int64_t ldpa, const float* metaa, int64_t m, const void* PB, int64_t ldpb,
                                     const float* metab, int64_t n, int K, const float* bias, const float* residual, int64_t ldr,
                                     int relu, float* out, int64_t ldo, float* out_meta, void* out_packed, int64_t ldop,
                                     float bound_w, float bound_add, const float* residual_meta, odx_stream_t stream) {
  H2PackOut pk;
  ODX_PROPAGATE(h2_pack_out(pk, "odx_gemm_h2_chain_f32", out, n, out_meta, out_packed, ldop, bound_w, bound_add, residual_meta));
  ODX_REQUIRE(residual == nullptr || out_packed == nullptr || residual_meta != nullptr, "odx_gemm_h2_chain_f32: a packed output with a residual needs residual_meta");
  return gemm_h2_launch(PA, ldpa, metaa, m, PB, ldpb, metab, n, K, bias, residual, ldr, relu, out, ldo, out_meta, pk, stream);
}

// odx_split_f16_taps3x3 of rows that are already packed (a chain layer's output): P ((R H W) x ldp, ldp >= roundup(9 C, 64)) =
// the 3 x 3 neighbourhood matrix of PY ((R H W) x C channels, C % 8 == 0) in packed form, same meta words as PY.
// The top-down step of a feature pyramid on NHWC rows, in place: lat[b, h, w, :] += top[b, h Hp / H, w Wp / W, :] (nearest-
// neighbour upsampling, F.interpolate's index rule) — one pass instead of two row gathers and an addition (1.3 GB of traffic for
// the 245-MB P2 rows of eight images against 0.55), and the maximum of the sum left for the packing of the 3 x 3 output
// convolution's operand (amax: IEEE bits of a non-negative float, zero on entry; nullptr: not wanted).  T = float, or a 16-bit
// type added in f32 and rounded once (what the tensor statement `a + b` of two 16-bit maps does).
template <typename T> struct UpAdd;
template <> struct UpAdd<float> {
  static __device__ __forceinline__ void run(float* __restrict__ d, const float* __restrict__ s, unsigned int& mx) {
    f32x4 a = *reinterpret_cast<f32x4*>(d);
    const f32x4 b = *reinterpret_cast<const f32x4*>(s);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[k] += b[k];
      mx = max(mx, __float_as_uint(fabsf(a[k])));
    }
    *reinterpret_cast<f32x4*>(d) = a;
  }
};
template <bool BF16> struct UpAdd16 {
  static __device__ __forceinline__ float dec(unsigned short v) {
    if (BF16) return __uint_as_float((uint32_t)v << 16);
    _Float16 h;
    __builtin_memcpy(&h, &v, 2);
    return (float)h;
  }
  static __device__ __forceinline__ unsigned short enc(float f) {
    if (BF16) return bf16_of(f);
    const _Float16 h = (_Float16)f;
    unsigned short v;
    __builtin_memcpy(&v, &h, 2);
    return v;
  }
  static __device__ __forceinline__ void run(unsigned short* __restrict__ d, const unsigned short* __restrict__ s, unsigned int& mx) {
    u16x4 a = *reinterpret_cast<u16x4*>(d);
    const u16x4 b = *reinterpret_cast<const u16x4*>(s);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = enc(dec(a[k]) + dec(b[k]));
    *reinterpret_cast<u16x4*>(d) = a;
  }
};

template <typename T, typename OP>
__global__ __launch_bounds__(256) void upsample_add_rows_kernel(T* __restrict__ lat, int64_t ldl, const T* __restrict__ top, int64_t ldt,
                                                                int H, int W, int Hp, int Wp, int C4, int64_t total,
                                                                unsigned int* __restrict__ amax) {
  // (a grid-stride walk of a bounded grid: a workgroup per 256 elements would end in a quarter of a million atomics on ONE word —
  // 12 ms at P2's size, measured)
  unsigned int mx = 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(e % C4);
    const int64_t row = e / C4;
    const int w = (int)(row % W), h = (int)((row / W) % H);
    const int64_t b = row / ((int64_t)W * H);
    const int64_t src = (b * Hp + ((int64_t)h * Hp) / H) * Wp + ((int64_t)w * Wp) / W;
    OP::run(lat + row * ldl + c4 * 4, top + src * ldt + c4 * 4, mx);
  }
  if (amax != nullptr) {                       // one atomic per workgroup
    __shared__ unsigned int wmx[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off));
    if ((threadIdx.x & 63) == 0) wmx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      mx = max(max(wmx[0], wmx[1]), max(wmx[2], wmx[3]));
      if (mx) atomicMax(amax, mx);
    }
  }
}

extern "C" int odx_upsample_add_rows_f32(float* lat, int64_t ldl, const float* top, int64_t ldt, int B, int H, int W, int Hp, int Wp, int C,
                                         float* meta, odx_stream_t stream) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return ODX_OK;
  ODX_REQUIRE(lat && top && Hp > 0 && Wp > 0, "odx_upsample_add_rows_f32: null pointer or empty source map");
  ODX_REQUIRE(C % 4 == 0 && ldl % 4 == 0 && ldt % 4 == 0 && ldl >= C && ldt >= C && aligned16(lat) && aligned16(top),
              "odx_upsample_add_rows_f32: C, ldl, ldt in fours, rows 16-byte aligned");
  const int64_t total = (int64_t)B * H * W * (C / 4);
  ODX_REQUIRE(ceil_div(total, 256) < (1ll << 31), "odx_upsample_add_rows_f32: too many elements");
  const int64_t wgs = ceil_div(total, 256);
  hipLaunchKernelGGL((upsample_add_rows_kernel<float, UpAdd<float>>), dim3((unsigned)(wgs < 2048 ? wgs : 2048)), dim3(256), 0, as_stream(stream), lat,
                     ldl, top, ldt, H, W, Hp, Wp, C / 4, total, meta ? reinterpret_cast<unsigned int*>(meta + 1) : nullptr);
  ODX_CHECK_LAUNCH("odx_upsample_add_rows_f32");
  return ODX_OK;
}

extern "C" int odx_upsample_add_rows_16(void* lat, int64_t ldl, const void* top, int64_t ldt, int is_bf16, int B, int H, int W, int Hp, int Wp,
                                        int C, odx_stream_t stream) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return ODX_OK;
  ODX_REQUIRE(lat && top && Hp > 0 && Wp > 0, "odx_upsample_add_rows_16: null pointer or empty source map");
  ODX_REQUIRE(C % 4 == 0 && ldl % 4 == 0 && ldt % 4 == 0 && ldl >= C && ldt >= C && (reinterpret_cast<uintptr_t>(lat) & 7u) == 0 &&
              (reinterpret_cast<uintptr_t>(top) & 7u) == 0, "odx_upsample_add_rows_16: C, ldl, ldt in fours, rows 8-byte aligned");
  const int64_t total = (int64_t)B * H * W * (C / 4);
  ODX_REQUIRE(ceil_div(total, 256) < (1ll << 31), "odx_upsample_add_rows_16: too many elements");
  unsigned short* l = static_cast<unsigned short*>(lat);
  const unsigned short* t = static_cast<const unsigned short*>(top);
  const int64_t wgs = ceil_div(total, 256);
  if (is_bf16)
    hipLaunchKernelGGL((upsample_add_rows_kernel<unsigned short, UpAdd16<true>>), dim3((unsigned)(wgs < 2048 ? wgs : 2048)), dim3(256), 0, as_stream(stream),
                       l, ldl, t, ldt, H, W, Hp, Wp, C / 4, total, (unsigned int*)nullptr);
  else
    hipLaunchKernelGGL((upsample_add_rows_kernel<unsigned short, UpAdd16<false>>), dim3((unsigned)(wgs < 2048 ? wgs : 2048)), dim3(256), 0, as_stream(stream),
                       l, ldl, t, ldt, H, W, Hp, Wp, C / 4, total, (unsigned int*)nullptr);
  ODX_CHECK_LAUNCH("odx_upsample_add_rows_16");
  return ODX_OK;
}

extern "C" int odx_taps3x3_packed(const void* PY, int64_t ldpy, int64_t R, int H, int W, int C, void* P, int64_t ldp,
                                  odx_stream_t stream) {
  const int64_t n = R * H * W;
  if (n <= 0) return ODX_OK;
  ODX_REQUIRE(PY && P && H > 0 && W > 0 && C > 0 && C % 8 == 0 && ldpy % 4 == 0 && ldpy >= round_up(C, 32) && aligned16(PY),
              "odx_taps3x3_packed: PY must be 16-byte aligned with ldpy %% 4 == 0, ldpy >= roundup(C, 32), C %% 8 == 0");
  const int D = 9 * C;
  ODX_REQUIRE(ldp >= round_up(D, H2_KT) && ldp % 4 == 0 && aligned16(P), "odx_taps3x3_packed: P must be 16-byte aligned, ldp %% 4 == 0, ldp >= roundup(9 C, 64)");
  const int groups = (int)ceil_div(D, H2_KT) * 8;
  ODX_REQUIRE(ceil_div(n * groups, 256) < (1ll << 31), "odx_taps3x3_packed: too many rows");
  hipLaunchKernelGGL(taps3x3_packed_kernel, dim3((unsigned)ceil_div(n * groups, 256)), dim3(256), 0, as_stream(stream),
                     static_cast<const uint32_t*>(PY), ldpy, H, W, C, static_cast<uint32_t*>(P), ldp, n);
  ODX_CHECK_LAUNCH("odx_taps3x3_packed");
  return ODX_OK;
}

// 1 when odx_gemm_h2_taps_f32 serves this layer: the 256 x 256 LDS-DMA core (it fills the chip: >= 256 tiles, more than 128
// output columns), whole 32-channel stages per tap, 32-bit byte offsets over the packed rows.
static bool h2_taps_wide(int64_t m, int64_t n, int C) {        // the layer goes to the 256 x 256 LDS-DMA core (gemm_h2_launch's rule)
  return n > GEMM_BN && C % W_KS == 0 && ceil_div(m, W_BM) * ceil_div(n, W_BN) >= 256;
}

extern "C" int odx_gemm_h2_taps_supported(int64_t m, int64_t n, int C, int64_t ldpy) {
  if (m <= 0 || n <= 0 || C <= 0) return 0;
  if (!h2_taps_wide(m, n, C) && C % H2_KT != 0) return 0;       // (the 128 x 128 core: a k-tile is 64 channels of one tap)
  return (m + 1) * ldpy * 4 < (1ll << 31) ? 1 : 0;
}

// out (R H W x n) = act(taps3x3(Y) B' + bias + residual): odx_gemm_h2_max_f32 whose A operand is the 3 x 3 neighbourhood matrix of
// the packed NHWC rows PY (R H W rows of C channels in odx_split_f16's form, row stride ldpy 4-byte units, metay) gathered
// INSIDE the product's operand loads — odx_split_f16_taps3x3's matrix is never written.  PY must be followed by one all-zero
// row (row R H W: what a position outside the map reads).  B (n x 9 C, tap after tap: K index (ky kx c)) packed as for
// odx_gemm_h2_f32.  out_meta may be NULL.  Only where odx_gemm_h2_taps_supported says so.
extern "C" int odx_gemm_h2_taps_f32(const void* PY, int64_t ldpy, const float* metay, int64_t R, int H, int W, int C,
                                    const void* PB, int64_t ldpb, const float* metab, int64_t n, const float* bias,
                                    const float* residual, int64_t ldr, int relu, float* out, int64_t ldo, float* out_meta,
                                    void* out_packed, int64_t ldop, float bound_w, float bound_add, const float* residual_meta,
                                    odx_stream_t stream) {
  const int64_t m = R * H * W;
  if (m <= 0 || n <= 0) return ODX_OK;
  H2PackOut pk;
  ODX_PROPAGATE(h2_pack_out(pk, "odx_gemm_h2_taps_f32", out, n, out_meta, out_packed, ldop, bound_w, bound_add, residual_meta));
  ODX_REQUIRE(residual == nullptr || out_packed == nullptr || residual_meta != nullptr, "odx_gemm_h2_taps_f32: a packed output with a residual needs residual_meta");
  ODX_REQUIRE(PY && PB && metay && metab && H > 0 && W > 0, "odx_gemm_h2_taps_f32: bad argument");
  ODX_REQUIRE(odx_gemm_h2_taps_supported(m, n, C, ldpy), "odx_gemm_h2_taps_f32: layer not served (odx_gemm_h2_taps_supported)");
  const int64_t K = 9 * (int64_t)C;
  ODX_REQUIRE(ldpy % 4 == 0 && ldpb % 4 == 0 && ldpy >= C && ldpb >= round_up(K, H2_KT) && aligned16(PY) && aligned16(PB),
              "odx_gemm_h2_taps_f32: packed operands must be 16-byte aligned with ld %% 4 == 0, ldpy >= C, ldpb >= roundup(9 C, 64)");
  ODX_REQUIRE((out == nullptr || ldo >= n) && (residual == nullptr || ldr >= n), "odx_gemm_h2_taps_f32: ldo / ldr < n");
  ODX_REQUIRE(ldpb < (1 << 24), "odx_gemm_h2_taps_f32: leading dimensions must stay below 2^24 (32-bit tile offsets)");
  const int gr = 8;
  unsigned int* amax = out_meta ? reinterpret_cast<unsigned int*>(out_meta + 1) : nullptr;
  if (!h2_taps_wide(m, n, C)) {          // narrow or small layers: the 128 x 128 core, the taps gathered in its register-staged loads
    const int64_t tiles = round_up(ceil_div(m, GEMM_BM), gr) * ceil_div(n, GEMM_BN);
    ODX_REQUIRE(tiles < (1ll << 31), "odx_gemm_h2_taps_f32: grid too large");
    ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_h2s16_kernel<true>)));
    hipLaunchKernelGGL(gemm_h2s16_kernel<true>, dim3((unsigned)tiles), dim3(GEMM_THREADS), S16_LDS_BYTES, as_stream(stream), (const uint32_t*)PY,
                       ldpy, metay, m, (const uint32_t*)PB, ldpb, metab, n, (int)(K / H2_KT), bias, residual, ldr, relu, out, ldo, gr, amax,
                       pk, H, W, C);
    ODX_CHECK_LAUNCH("odx_gemm_h2_taps_f32(s16)");
    return ODX_OK;
  }
  const int64_t wt = round_up(ceil_div(m, W_BM), gr) * ceil_div(n, W_BN);
  ODX_REQUIRE(wt < (1ll << 31), "odx_gemm_h2_taps_f32: grid too large");
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_h2w256_kernel<true>), W_LDS_BYTES));
  hipLaunchKernelGGL((gemm_h2w256_kernel<true>), dim3((unsigned)wt), dim3(W_THREADS), W_LDS_BYTES, as_stream(stream),
                     (const uint32_t*)PY, ldpy, metay, m, (const uint32_t*)PB, ldpb, metab, n, (int)(K / W_KS), bias, residual, ldr,
                     relu, out, ldo, gr, amax, H, W, C, pk);
  ODX_CHECK_LAUNCH("odx_gemm_h2_taps_f32");
  return ODX_OK;
}

// Measurement only (tools/ab_mfma_shape.py): out (m x n) f32 = A B' for packed operands on the 256 x 256 LDS-DMA loop built from
// v_mfma_f32_32x32x16_f16 — the A/B partner of odx_gemm_h2_f32 (v_mfma_f32_16x16x32_f16) on the same operands.
extern "C" int odx_debug_gemm_h2_mf32(const void* PA, int64_t ldpa, const float* metaa, int64_t m, const void* PB, int64_t ldpb,
                                      const float* metab, int64_t n, int K, float* out, int64_t ldo, odx_stream_t stream) {
  if (m <= 0 || n <= 0) return ODX_OK;
  ODX_REQUIRE(PA && PB && metaa && metab && out && K > 0, "odx_debug_gemm_h2_mf32: bad argument");
  const int64_t dp = round_up(K, H2_KT);
  ODX_REQUIRE(ldpa % 4 == 0 && ldpb % 4 == 0 && ldpa >= dp && ldpb >= dp && aligned16(PA) && aligned16(PB) && ldo >= n,
              "odx_debug_gemm_h2_mf32: packed operands as for odx_gemm_h2_f32");
  ODX_REQUIRE(ldpa < (1 << 24) && ldpb < (1 << 24), "odx_debug_gemm_h2_mf32: leading dimensions must stay below 2^24");
  const int gr = 8;
  const int64_t wt = round_up(ceil_div(m, W_BM), gr) * ceil_div(n, W_BN);
  ODX_REQUIRE(wt < (1ll << 31), "odx_debug_gemm_h2_mf32: grid too large");
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_h2w256_mf32_kernel), W_LDS_BYTES));
  hipLaunchKernelGGL(gemm_h2w256_mf32_kernel, dim3((unsigned)wt), dim3(W_THREADS), W_LDS_BYTES, as_stream(stream), (const uint32_t*)PA, ldpa,
                     metaa, m, (const uint32_t*)PB, ldpb, metab, n, (int)(dp / W_KS), out, ldo, gr);
  ODX_CHECK_LAUNCH("odx_debug_gemm_h2_mf32");
  return ODX_OK;
}

extern "C" int odx_taps3x3_16(const void* Y, int64_t ldy, int64_t R, int H, int W, int C, void* P, int64_t ldp, odx_stream_t stream) {
  const int64_t n = R * H * W;
  if (n <= 0) return ODX_OK;
  ODX_REQUIRE(Y && P && H > 0 && W > 0 && C > 0 && C % 8 == 0 && ldy >= C && ldy % 8 == 0 && aligned16(Y),
              "odx_taps3x3_16: Y must be 16-byte aligned with ldy %% 8 == 0, ldy >= C, C %% 8 == 0");
  ODX_REQUIRE(ldp >= 9 * (int64_t)C && ldp % 8 == 0 && aligned16(P), "odx_taps3x3_16: P must be 16-byte aligned with ldp %% 8 == 0, ldp >= 9 C");
  hipStream_t s = as_stream(stream);
  const int groups = (int)(ldp / 8);
  for (int64_t r0 = 0; r0 < n; r0 += 65535) {
    const int64_t nr = n - r0 < 65535 ? n - r0 : 65535;
    hipLaunchKernelGGL(taps3x3_b16_kernel, dim3((unsigned)ceil_div(groups, 256), (unsigned)nr), dim3(256), 0, s,
                       static_cast<const unsigned short*>(Y), ldy, H, W, C, static_cast<unsigned short*>(P), ldp, r0);
    ODX_CHECK_LAUNCH("odx_taps3x3_16");
  }
  return ODX_OK;
}

template <int CORE, bool OUT16>
static int launch_gemm_b16(const void* A, int64_t lda, int64_t m, const void* B, int64_t ldb, int64_t n, int K, const float* bias,
                           const void* residual, int64_t ldr, int relu, void* out, int64_t ldo, hipStream_t s) {
  const int gr = 8;
  const int64_t t256 = ceil_div(m, W_BM) * ceil_div(n, W_BN);
  const int pin = lib_option(OPT_H2_TILE);
  const bool wide = pin == 256 || (pin != 128 && t256 >= 256 && n > GEMM_BN);     // (<= 128 columns: half a wide tile idle)
  if (wide) {                  // the 256 x 256 core once it fills the chip (one workgroup per CU), else 128 x 128 tiles
    const int64_t wt = round_up(ceil_div(m, W_BM), gr) * ceil_div(n, W_BN);
    ODX_REQUIRE(wt < (1ll << 31), "odx_gemm_b16: grid too large");
    ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_b16w256_kernel<CORE, OUT16>), W_LDS_BYTES));
    hipLaunchKernelGGL((gemm_b16w256_kernel<CORE, OUT16>), dim3((unsigned)wt), dim3(W_THREADS), W_LDS_BYTES, s, (const uint32_t*)A, lda / 2, m,
                       (const uint32_t*)B, ldb / 2, n, (int)(round_up(K, 64) / 64), bias, residual, ldr, relu, out, ldo, gr, 0, 0, 0);
    ODX_CHECK_LAUNCH("odx_gemm_b16(w256)");
    return ODX_OK;
  }
  const int64_t tiles = round_up(ceil_div(m, GEMM_BM), gr) * ceil_div(n, GEMM_BN);
  ODX_REQUIRE(tiles < (1ll << 31), "odx_gemm_b16: grid too large");
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_b16s16_kernel<CORE, OUT16>)));
  hipLaunchKernelGGL((gemm_b16s16_kernel<CORE, OUT16>), dim3((unsigned)tiles), dim3(GEMM_THREADS), S16_LDS_BYTES, s, (const uint32_t*)A, lda / 2,
                     m, (const uint32_t*)B, ldb / 2, n, (int)(round_up(K, 128) / 128), bias, residual, ldr, relu, out, ldo, gr, 0, 0, 0);
  ODX_CHECK_LAUNCH("odx_gemm_b16");
  return ODX_OK;
}

extern "C" int odx_gemm_b16(const void* A, int64_t lda, int64_t m, const void* B, int64_t ldb, int64_t n, int K, int is_bf16,
                            const float* bias, const void* residual, int64_t ldr, int relu, void* out, int64_t ldo, int out_16,
                            odx_stream_t stream) {
  if (m <= 0 || n <= 0) return ODX_OK;
  ODX_REQUIRE(A && B && out && K > 0, "odx_gemm_b16: bad argument");
  const int64_t kp = round_up(K, 128);
  ODX_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && lda >= kp && ldb >= kp && aligned16(A) && aligned16(B),
              "odx_gemm_b16: operands must be 16-byte aligned with ld %% 8 == 0 and ld >= roundup(K, 128) elements (zero beyond K)");
  ODX_REQUIRE(ldo >= n && (residual == nullptr || ldr >= n), "odx_gemm_b16: ldo / ldr < n");
  ODX_REQUIRE(lda < (1 << 25) && ldb < (1 << 25), "odx_gemm_b16: leading dimensions must stay below 2^25 (32-bit tile offsets)");
  hipStream_t s = as_stream(stream);
  if (is_bf16) {
    return out_16 ? launch_gemm_b16<CORE_BF16, true>(A, lda, m, B, ldb, n, K, bias, residual, ldr, relu, out, ldo, s)
                  : launch_gemm_b16<CORE_BF16, false>(A, lda, m, B, ldb, n, K, bias, residual, ldr, relu, out, ldo, s);
  }
  return out_16 ? launch_gemm_b16<CORE_F16, true>(A, lda, m, B, ldb, n, K, bias, residual, ldr, relu, out, ldo, s)
                : launch_gemm_b16<CORE_F16, false>(A, lda, m, B, ldb, n, K, bias, residual, ldr, relu, out, ldo, s);
}

// odx_gemm_h2_taps_supported / odx_gemm_h2_taps_f32 for 16-bit rows: out = act(taps3x3(Y) B' + bias + residual) with the taps of the
// 16-bit NHWC rows Y (R H W rows of C channels, C % 64 == 0, row stride ldy elements, FOLLOWED BY ONE ALL-ZERO ROW) gathered
// inside the product's operand loads — odx_taps3x3_16's matrix is never written.  B (n x 9 C) as for odx_gemm_b16.
static bool b16_taps_wide(int64_t m, int64_t n, int C) {       // launch_gemm_b16's rule for the 256 x 256 core
  const int pin = lib_option(OPT_H2_TILE);
  return C % 64 == 0 && (pin == 256 || (pin != 128 && ceil_div(m, W_BM) * ceil_div(n, W_BN) >= 256 && n > GEMM_BN));
}

extern "C" int odx_gemm_b16_taps_supported(int64_t m, int64_t n, int C, int64_t ldy) {
  if (m <= 0 || n <= 0 || C <= 0) return 0;
  if (!b16_taps_wide(m, n, C) && C % 128 != 0) return 0;        // (the 128 x 128 core: a k-tile is 128 channels of one tap)
  return (m + 1) * ldy * 2 < (1ll << 31) ? 1 : 0;
}

template <int CORE, bool OUT16>
static int launch_gemm_b16_taps(const void* Y, int64_t ldy, int64_t m, int H, int W, int C, const void* B, int64_t ldb, int64_t n,
                                const float* bias, const void* residual, int64_t ldr, int relu, void* out, int64_t ldo, hipStream_t s) {
  const int gr = 8;
  if (!b16_taps_wide(m, n, C)) {
    const int64_t tiles = round_up(ceil_div(m, GEMM_BM), gr) * ceil_div(n, GEMM_BN);
    ODX_REQUIRE(tiles < (1ll << 31), "odx_gemm_b16_taps: grid too large");
    ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_b16s16_kernel<CORE, OUT16, true>)));
    hipLaunchKernelGGL((gemm_b16s16_kernel<CORE, OUT16, true>), dim3((unsigned)tiles), dim3(GEMM_THREADS), S16_LDS_BYTES, s, (const uint32_t*)Y,
                       ldy / 2, m, (const uint32_t*)B, ldb / 2, n, (int)(9 * (int64_t)C / 128), bias, residual, ldr, relu, out, ldo, gr, H, W, C);
    ODX_CHECK_LAUNCH("odx_gemm_b16_taps(s16)");
    return ODX_OK;
  }
  const int64_t wt = round_up(ceil_div(m, W_BM), gr) * ceil_div(n, W_BN);
  ODX_REQUIRE(wt < (1ll << 31), "odx_gemm_b16_taps: grid too large");
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gemm_b16w256_kernel<CORE, OUT16, true>), W_LDS_BYTES));
  hipLaunchKernelGGL((gemm_b16w256_kernel<CORE, OUT16, true>), dim3((unsigned)wt), dim3(W_THREADS), W_LDS_BYTES, s, (const uint32_t*)Y, ldy / 2, m,
                     (const uint32_t*)B, ldb / 2, n, (int)(9 * (int64_t)C / 64), bias, residual, ldr, relu, out, ldo, gr, H, W, C);
  ODX_CHECK_LAUNCH("odx_gemm_b16_taps");
  return ODX_OK;
}

extern "C" int odx_gemm_b16_taps(const void* Y, int64_t ldy, int64_t R, int H, int W, int C, const void* B, int64_t ldb, int64_t n,
                                 int is_bf16, const float* bias, const void* residual, int64_t ldr, int relu, void* out, int64_t ldo,
                                 int out_16, odx_stream_t stream) {
  const int64_t m = R * H * W;
  if (m <= 0 || n <= 0) return ODX_OK;
  ODX_REQUIRE(Y && B && out && H > 0 && W > 0, "odx_gemm_b16_taps: bad argument");
  ODX_REQUIRE(odx_gemm_b16_taps_supported(m, n, C, ldy), "odx_gemm_b16_taps: layer not served (odx_gemm_b16_taps_supported)");
  ODX_REQUIRE(ldy % 8 == 0 && ldb % 8 == 0 && ldy >= C && ldb >= round_up(9 * (int64_t)C, 128) && aligned16(Y) && aligned16(B),
              "odx_gemm_b16_taps: operands must be 16-byte aligned with ld %% 8 == 0, ldy >= C, ldb >= roundup(9 C, 128)");
  ODX_REQUIRE(ldo >= n && (residual == nullptr || ldr >= n), "odx_gemm_b16_taps: ldo / ldr < n");
  ODX_REQUIRE(ldb < (1 << 25), "odx_gemm_b16_taps: leading dimensions must stay below 2^25 (32-bit tile offsets)");
  hipStream_t s = as_stream(stream);
  if (is_bf16) {
    return out_16 ? launch_gemm_b16_taps<CORE_BF16, true>(Y, ldy, m, H, W, C, B, ldb, n, bias, residual, ldr, relu, out, ldo, s)
                  : launch_gemm_b16_taps<CORE_BF16, false>(Y, ldy, m, H, W, C, B, ldb, n, bias, residual, ldr, relu, out, ldo, s);
  }
  return out_16 ? launch_gemm_b16_taps<CORE_F16, true>(Y, ldy, m, H, W, C, B, ldb, n, bias, residual, ldr, relu, out, ldo, s)
                : launch_gemm_b16_taps<CORE_F16, false>(Y, ldy, m, H, W, C, B, ldb, n, bias, residual, ldr, relu, out, ldo, s);
}

extern "C" int odx_gauss_h2_tile(int64_t n, int64_t M) {
  if (n <= 0 || M <= 0) return 0;
  return h2_use_w256(ceil_div(n, W_BM) * ceil_div(M, W_BN)) ? W_BM : GEMM_BM;
}

extern "C" int odx_gauss_knm_h2(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D,
                                double sigma, float* K, int64_t ldk, odx_stream_t stream) {
  if (n <= 0 || M <= 0) return ODX_OK;
  ODX_REQUIRE(PX && PZ && metax && metaz && xsq && zsq && K && D > 0 && sigma > 0, "odx_gauss_knm_h2: bad argument");
  const int64_t dp = round_up(D, H2_KT);
  ODX_PROPAGATE(check_packed_pair("odx_gauss_knm_h2", dp, ldpx, ldpz, PX, PZ));
  ODX_PROPAGATE(check_knm_block("odx_gauss_knm_h2", ODX_KNM_F32, M, K, ldk, nullptr, 0));
  const int gr = 8;   // band height of the tile order: 2..32 measured within 2 % of each other at n = 2.5e5, M = 1e4
  if (h2_use_w256(ceil_div(n, W_BM) * ceil_div(M, W_BN)))
    return launch_knm_w256(PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, M, (int)(dp / W_KS), sigma, KF_F32, K, ldk, nullptr, 0, nullptr, nullptr, 0, stream);
  const int64_t tiles = round_up(ceil_div(n, GEMM_BM), gr) * ceil_div(M, GEMM_BN);
  ODX_REQUIRE(tiles < (1ll << 31), "odx_gauss_knm_h2: grid too large");
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gauss_knm_h2s16_kernel)));
  hipLaunchKernelGGL(gauss_knm_h2s16_kernel, dim3((unsigned)tiles), dim3(GEMM_THREADS), S16_LDS_BYTES, as_stream(stream),
                     (const uint32_t*)PX, ldpx, metax, xsq, n, (const uint32_t*)PZ, ldpz, metaz, zsq, M, (int)(dp / H2_KT),
                     h2_gamma_log2e(sigma), K, ldk, gr);
  ODX_CHECK_LAUNCH("odx_gauss_knm_h2");
  return ODX_OK;
}

extern "C" int64_t odx_gauss_knm_h2_rhs_workspace_bytes(int64_t n, int64_t M) {
  if (n <= 0 || M <= 0) return 0;
  return ceil_div(n, W_BM) * round_up(M, 4) * (int64_t)sizeof(double);
}

extern "C" int odx_gauss_knm_h2_rhs(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                    const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D,
                                    double sigma, float* K, int64_t ldk, const double* w, double* ktw, void* workspace,
                                    int64_t workspace_bytes, odx_stream_t stream) {
  ODX_REQUIRE(M > 0 && ktw, "odx_gauss_knm_h2_rhs: M <= 0 or null output");
  if (n <= 0) {
    ODX_CHECK_HIP(hipMemsetAsync(ktw, 0, (size_t)M * sizeof(double), as_stream(stream)));
    return ODX_OK;
  }
  ODX_REQUIRE(PX && PZ && metax && metaz && xsq && zsq && K && w && D > 0 && sigma > 0, "odx_gauss_knm_h2_rhs: bad argument");
  const int64_t dp = round_up(D, H2_KT);
  ODX_PROPAGATE(check_packed_pair("odx_gauss_knm_h2_rhs", dp, ldpx, ldpz, PX, PZ));
  ODX_PROPAGATE(check_knm_block("odx_gauss_knm_h2_rhs", ODX_KNM_F32, M, K, ldk, nullptr, 0));
  if (workspace == nullptr || workspace_bytes < odx_gauss_knm_h2_rhs_workspace_bytes(n, M)) {
    set_error("odx_gauss_knm_h2_rhs: workspace too small");
    return ODX_ERR_WORKSPACE;
  }
  const int64_t wld = round_up(M, 4);
  ODX_PROPAGATE(launch_knm_w256(PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, M, (int)(dp / W_KS), sigma, KF_F32, K, ldk, nullptr, 0, w,
                                static_cast<double*>(workspace), wld, stream));
  return slab_reduce_f64(static_cast<const double*>(workspace), wld, (int)ceil_div(n, W_BM), M, ktw, as_stream(stream));
}

extern "C" int64_t odx_knm_ld(int64_t M, int fmt) {
  if (M <= 0) return 0;
  return fmt == ODX_KNM_F32 ? round_up(M, 4) : round_up(M, 8);
}

extern "C" int64_t odx_knm_bytes(int64_t n, int64_t M, int fmt) {
  if (n <= 0 || M <= 0) return 0;
  const int64_t per = fmt == ODX_KNM_F32 ? 4 : (fmt == ODX_KNM_U24 ? 3 : 2);
  return n * odx_knm_ld(M, fmt) * per;
}

// ld (4-byte units) an operand row needs for `core`, and the 128-byte stages of a row
static bool core_is_b16(int core) { return core == CORE_BF16 || core == CORE_F16; }
static int64_t core_min_ld(int D, int core) {
  if (core_is_b16(core)) return round_up(D, 64) / 2;        // 64 features per stage: D <= 64 is ONE stage (the split has two from D = 1 on)
  return core == CORE_F8 ? round_up(D, 128) / 4 : round_up(D, H2_KT);
}
static int core_stages(int D, int core) { return (int)(core_min_ld(D, core) / W_KS); }

// The pair of 16-bit row operands of a Gaussian entry `who` (odx_gemm_b16's contract at 64-feature granularity): 16-byte
// aligned, row strides (elements) multiples of 64 — whole 128-byte stages — that cover D; the columns D .. stride are zero.
static int check_b16_pair(const char* who, int D, int64_t ldx, int64_t ldz, const void* X, const void* Z) {
  ODX_REQUIRE(ldx % 64 == 0 && ldz % 64 == 0 && ldx >= round_up(D, 64) && ldz >= round_up(D, 64) && aligned16(X) && aligned16(Z),
              "%s: 16-bit operands must be 16-byte aligned with row strides that are multiples of 64 elements and >= roundup(D, 64) "
              "(zero beyond D)", who);
  ODX_REQUIRE(ldx < (1 << 25) && ldz < (1 << 25), "%s: row strides must stay below 2^25 elements (32-bit tile offsets)", who);
  return ODX_OK;
}

static int knm_store_impl(const char* who, int core, const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                          const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D, double sigma,
                          int fmt, void* K, int64_t ldk, void* Klo, int64_t ldlo, const double* w, double* ktw, void* workspace,
                          int64_t workspace_bytes, odx_stream_t stream, int kind = ODX_KERNEL_GAUSS) {
  ODX_REQUIRE(radial_kind_known(kind), "%s: unknown kernel kind %d", who, kind);
  ODX_REQUIRE(M > 0, "%s: M <= 0", who);
  ODX_REQUIRE(fmt == ODX_KNM_F32 || fmt == ODX_KNM_U24 || fmt == ODX_KNM_BF16, "%s: unknown storage format %d", who, fmt);
  ODX_REQUIRE((w == nullptr) == (ktw == nullptr), "%s: w and ktw go together", who);
  if (n <= 0) {
    if (ktw) ODX_CHECK_HIP(hipMemsetAsync(ktw, 0, (size_t)M * sizeof(double), as_stream(stream)));
    return ODX_OK;
  }
  ODX_REQUIRE(PX && PZ && ((metax && metaz) || core_is_b16(core)) && xsq && zsq && K && D > 0 && sigma > 0, "%s: bad argument", who);
  ODX_PROPAGATE(check_packed_pair(who, core_min_ld(D, core), ldpx, ldpz, PX, PZ));
  ODX_PROPAGATE(check_knm_block(who, fmt, M, K, ldk, Klo, ldlo));
  if (w != nullptr && (workspace == nullptr || workspace_bytes < odx_gauss_knm_h2_rhs_workspace_bytes(n, M))) {
    set_error("%s: workspace too small", who);
    return ODX_ERR_WORKSPACE;
  }
  const int64_t wld = round_up(M, 4);
  ODX_PROPAGATE(launch_knm_w256(PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, M, core_stages(D, core), sigma, fmt, K, ldk, Klo, ldlo,
                                w, static_cast<double*>(workspace), wld, stream, core, kind));
  if (w == nullptr) return ODX_OK;
  return slab_reduce_f64(static_cast<const double*>(workspace), wld, (int)ceil_div(n, W_BM), M, ktw, as_stream(stream));
}

extern "C" int odx_gauss_knm_h2_store(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                      const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D,
                                      double sigma, int fmt, void* K, int64_t ldk, void* Klo, int64_t ldlo, const double* w,
                                      double* ktw, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  return knm_store_impl("odx_gauss_knm_h2_store", CORE_H2, PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, M, D, sigma, fmt, K, ldk,
                        Klo, ldlo, w, ktw, workspace, workspace_bytes, stream);
}

extern "C" int odx_radial_knm_h2_store(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                       const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D,
                                       double sigma, int kind, int fmt, void* K, int64_t ldk, void* Klo, int64_t ldlo, const double* w,
                                       double* ktw, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  return knm_store_impl("odx_radial_knm_h2_store", CORE_H2, PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, M, D, sigma, fmt, K, ldk,
                        Klo, ldlo, w, ktw, workspace, workspace_bytes, stream, kind);
}

// ---- rows that are 16-bit already (bf16 / f16): the Gaussian kernels at native width
// A bf16 x bf16 product has 8 + 8 significant bits, an f16 x f16 one 11 + 11: exact in the f32 accumulator of ONE MFMA, so K
// is f32-accurate for the rows as given with a third of the split's matrix instructions and half its operand bytes, nothing
// packed and no f32 copy made.  The norms are the f32 sums of the exact squares, one wave per row (pad columns are zero: whole
// 16-byte pieces are read).
template <int CORE>
__global__ __launch_bounds__(256) void row_sqnorm_b16_kernel(const unsigned short* __restrict__ X, int64_t ldx, int64_t n, int D,
                                                             float* __restrict__ sq) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const unsigned short* x = X + row * ldx;
  float acc = 0.f;
  for (int c = lane * 8; c < D; c += 512) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(x + c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned short lo = (unsigned short)(v[q] & 0xffffu), hi = (unsigned short)(v[q] >> 16);
      const float a = b16_load<CORE>(&lo), b = b16_load<CORE>(&hi);
      acc = fmaf(a, a, acc);
      acc = fmaf(b, b, acc);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) sq[row] = acc;
}

extern "C" int odx_row_sqnorm_b16(const void* X, int64_t ldx, int64_t n, int D, int is_bf16, float* sq, odx_stream_t stream) {
  if (n <= 0) return ODX_OK;
  ODX_REQUIRE(X && sq && D > 0, "odx_row_sqnorm_b16: bad argument");
  ODX_PROPAGATE(check_b16_pair("odx_row_sqnorm_b16", D, ldx, ldx, X, X));
  ODX_REQUIRE(ceil_div(n, 4) < (1ll << 31), "odx_row_sqnorm_b16: too many rows");
  const unsigned short* x = static_cast<const unsigned short*>(X);
  if (is_bf16)
    hipLaunchKernelGGL(row_sqnorm_b16_kernel<CORE_BF16>, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, as_stream(stream), x, ldx, n, D, sq);
  else
    hipLaunchKernelGGL(row_sqnorm_b16_kernel<CORE_F16>, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, as_stream(stream), x, ldx, n, D, sq);
  ODX_CHECK_LAUNCH("odx_row_sqnorm_b16");
  return ODX_OK;
}

extern "C" int64_t odx_gauss_knm_b16_store_workspace_bytes(int64_t n, int64_t M) { return odx_gauss_knm_h2_rhs_workspace_bytes(n, M); }

// odx_gauss_knm_h2_store for 16-bit rows: the same wide core, tile order, epilogue (unit scales) and slab reduction; a stage is
// 64 features, so D <= 64 runs the pipeline with a single stage.
extern "C" int odx_gauss_knm_b16_store(const void* X, int64_t ldx, const float* xsq, int64_t n, const void* Z, int64_t ldz,
                                       const float* zsq, int64_t M, int D, int is_bf16, double sigma, int fmt, void* K, int64_t ldk,
                                       void* Klo, int64_t ldlo, const double* w, double* ktw, void* workspace,
                                       int64_t workspace_bytes, odx_stream_t stream) {
  if (n > 0 && M > 0 && D > 0) ODX_PROPAGATE(check_b16_pair("odx_gauss_knm_b16_store", D, ldx, ldz, X, Z));
  return knm_store_impl("odx_gauss_knm_b16_store", is_bf16 ? CORE_BF16 : CORE_F16, X, ldx / 2, nullptr, xsq, n, Z, ldz / 2, nullptr, zsq, M,
                        D, sigma, fmt, K, ldk, Klo, ldlo, w, ktw, workspace, workspace_bytes, stream);
}

// ---- S blocks, one per kernel width, from one contraction (gauss_knm_sigmas_h2w256_kernel)
extern "C" int64_t odx_gauss_knm_h2_store_sigmas_workspace_bytes(int64_t n, int64_t M, int S) {
  if (S <= 0) return 0;
  return (int64_t)S * odx_gauss_knm_h2_rhs_workspace_bytes(n, M);
}

template <bool RHS, int FMT>
static int launch_knm_sigmas_t(unsigned wt, hipStream_t s, const uint32_t* PX, int64_t ldpx, const float* metax, const float* xsq,
                               int64_t n, const uint32_t* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M,
                               int stages, int S, const KnmSigmaArgs& sg, int64_t ldk, int64_t ldlo, int wgr, const double* w,
                               int64_t wslab_ld) {
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gauss_knm_sigmas_h2w256_kernel<RHS, FMT>), W_LDS_BYTES));
  hipLaunchKernelGGL((gauss_knm_sigmas_h2w256_kernel<RHS, FMT>), dim3(wt), dim3(W_THREADS), W_LDS_BYTES, s, PX, ldpx, metax, xsq, n,
                     PZ, ldpz, metaz, zsq, M, stages, S, sg, ldk, ldlo, wgr, w, wslab_ld);
  return ODX_OK;
}

extern "C" int odx_gauss_knm_h2_store_sigmas(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                             const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D,
                                             const double* sigmas, int S, int fmt, void* const* K, int64_t ldk, void* const* Klo,
                                             int64_t ldlo, const double* w, double* ktw, int64_t ldktw, void* workspace,
                                             int64_t workspace_bytes, odx_stream_t stream) {
  const char* who = "odx_gauss_knm_h2_store_sigmas";
  ODX_REQUIRE(M > 0, "%s: M <= 0", who);
  ODX_REQUIRE(S >= 1 && S <= ODX_GRID_MAX_SIGMAS, "%s: S = %d outside 1 .. %d", who, S, ODX_GRID_MAX_SIGMAS);
  ODX_REQUIRE(fmt == ODX_KNM_F32 || fmt == ODX_KNM_U24 || fmt == ODX_KNM_BF16, "%s: unknown storage format %d", who, fmt);
  ODX_REQUIRE(sigmas && K && (fmt != ODX_KNM_U24 || Klo), "%s: null list of widths or blocks", who);
  for (int s = 0; s < S; ++s) ODX_REQUIRE(sigmas[s] > 0, "%s: sigma[%d] <= 0", who, s);
  if (n <= 0) return ODX_OK;
  ODX_REQUIRE(PX && PZ && metax && metaz && xsq && zsq && D > 0, "%s: bad argument", who);
  ODX_REQUIRE(w == nullptr || (ktw != nullptr && ldktw >= M), "%s: w needs ktw with ldktw >= M", who);
  const int64_t dp = round_up(D, H2_KT);
  ODX_PROPAGATE(check_packed_pair(who, dp, ldpx, ldpz, PX, PZ));
  KnmSigmaArgs sg;
  for (int s = 0; s < ODX_GRID_MAX_SIGMAS; ++s) sg.g2[s] = 0.f, sg.K[s] = nullptr, sg.Klo[s] = nullptr, sg.wslab[s] = nullptr;
  for (int s = 0; s < S; ++s) {
    ODX_PROPAGATE(check_knm_block(who, fmt, M, K[s], ldk, fmt == ODX_KNM_U24 ? Klo[s] : nullptr, ldlo));
    sg.g2[s] = h2_gamma_log2e(sigmas[s]);
    sg.K[s] = K[s];
    sg.Klo[s] = fmt == ODX_KNM_U24 ? static_cast<unsigned char*>(Klo[s]) : nullptr;
  }
  const int64_t per = odx_gauss_knm_h2_rhs_workspace_bytes(n, M);
  if (w != nullptr && (workspace == nullptr || !aligned16(workspace) || workspace_bytes < (int64_t)S * per)) {
    set_error("%s: workspace too small", who);
    return ODX_ERR_WORKSPACE;
  }
  const int64_t wld = round_up(M, 4);
  if (w != nullptr)
    for (int s = 0; s < S; ++s) sg.wslab[s] = reinterpret_cast<double*>(static_cast<char*>(workspace) + s * per);
  const int64_t wt = knm_w256_grid(n, M);             // launch_knm_w256's: the same tile order
  ODX_REQUIRE(wt < (1ll << 31), "%s: grid too large", who);
  hipStream_t hs = as_stream(stream);
  const uint32_t *px = (const uint32_t*)PX, *pz = (const uint32_t*)PZ;
  const int stages = (int)(dp / W_KS);
  ODX_PROPAGATE(knm_rhs_fmt(w != nullptr, fmt, [&](auto rhs, auto kf) {
    return launch_knm_sigmas_t<decltype(rhs)::value, decltype(kf)::value>((unsigned)wt, hs, px, ldpx, metax, xsq, n, pz, ldpz, metaz, zsq, M,
                                                                          stages, S, sg, ldk, ldlo, W_KNM_GR, w, wld);
  }));
  ODX_CHECK_LAUNCH("odx_gauss_knm_h2_store_sigmas");
  if (w == nullptr) return ODX_OK;
  for (int s = 0; s < S; ++s)
    ODX_PROPAGATE(slab_reduce_f64(sg.wslab[s], wld, (int)ceil_div(n, W_BM), M, ktw + s * ldktw, hs));
  return ODX_OK;
}

// ---------------------------------------------------------------- fp8 (OCP e4m3) contraction: BASELINE config 5's path
// x . z with both operands rounded once to e4m3 (4 significant bits): K entries off by ~1e-3, scores by ~5e-3
// (tools/precision_scoring_study.py) — a THROUGHPUT-ONLY variant, never the default; the fit's 1e-4 bar on alpha needs the
// f16-split kernels.  odx_split_f8 packs rows as e4m3 bytes, x s with s a power of two putting max |x| into [128, 256)
// (e4m3's largest finite value is 448): row = ldp8 bytes, ldp8 % 128 == 0, features past D zero; meta as odx_split_f16.
__global__ __launch_bounds__(256) void split_f8_kernel(const float* __restrict__ X, int64_t ldx, int64_t n, int D,
                                                       uint32_t* __restrict__ P, int64_t ldp, float* __restrict__ meta) {
  // scale = 2^(7 - e) for absmax = 1.m x 2^e
  const unsigned int bits = __float_as_uint(meta[1]);
  const int ef = (int)((bits >> 23) & 0xffu);
  float s = 1.f;
  if (ef != 0 && ef != 255) {
    int se = 127 + 7 - (ef - 127);
    se = se < 1 ? 1 : (se > 254 ? 254 : se);
    s = __uint_as_float((unsigned int)se << 23);
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) meta[0] = s;
  const int groups = (int)((D + 127) / 128) * 16;        // 8-feature groups per row, zero padded to whole 128-byte stages
  const int64_t row = blockIdx.y;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  const float* x = X + row * ldx + (int64_t)g * 8;
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = (g * 8 + q < D) ? x[q] * s : 0.f;
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], hi, true);
  uint32_t* dst = P + row * ldp + (int64_t)g * 2;
  dst[0] = (uint32_t)lo;
  dst[1] = (uint32_t)hi;
}

// qsq[row] = |e4m3(s x_row)|^2 / s^2: the squared norm of the row AS THE CONTRACTION SEES IT.  With these norms
// d^2 = |q(x)|^2 + |q(z)|^2 - 2 q(x) . q(z) is the squared distance of the rounded points: never negative beyond rounding,
// exactly 0 for duplicates (K = 1), and off the true d^2 by unbiased rounding noise — with the norms of the unrounded rows
// a duplicate pair came out at K = 0.93 (the rounding shrinks |q(x)|^2 by ~1 % of 400).  One wave per row.
__global__ __launch_bounds__(256) void f8_row_sqnorm_kernel(const uint32_t* __restrict__ P, int64_t ldp, int64_t n, int dwords,
                                                            const float* __restrict__ meta, float* __restrict__ qsq) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  float acc = 0.f;
  for (int i = lane; i < dwords; i += 64) {
    const uint32_t u = P[row * ldp + i];
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, true);
    acc = fmaf(a[0], a[0], acc);
    acc = fmaf(a[1], a[1], acc);
    acc = fmaf(b[0], b[0], acc);
    acc = fmaf(b[1], b[1], acc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) qsq[row] = acc / (meta[0] * meta[0]);
}

extern "C" int odx_split_f8(const float* X, int64_t ldx, int64_t n, int D, void* P, int64_t ldp8, float* meta, float* qsq,
                            odx_stream_t stream) {
  ODX_REQUIRE(meta, "odx_split_f8: meta is null");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(meta_zero_kernel, dim3(1), dim3(64), 0, s, meta);
  if (n <= 0) {
    hipLaunchKernelGGL(split_f8_kernel, dim3(1, 1), dim3(256), 0, s, X, ldx, 0, 0, (uint32_t*)P, 0, meta);
    ODX_CHECK_LAUNCH("odx_split_f8");
    return ODX_OK;
  }
  ODX_REQUIRE(X && P && D > 0 && ldx >= D && ldx % 4 == 0 && aligned16(X), "odx_split_f8: X must be 16-byte aligned with ldx %% 4 == 0 and ldx >= D");
  ODX_REQUIRE(ldp8 >= round_up(D, 128) && ldp8 % 16 == 0 && aligned16(P), "odx_split_f8: P must be 16-byte aligned, ldp8 %% 16 == 0, ldp8 >= roundup(D, 128) bytes");
  const unsigned blocks = (unsigned)(ceil_div(n, 4) > 1024 ? 1024 : ceil_div(n, 4));
  hipLaunchKernelGGL(absmax_f32_kernel, dim3(blocks), dim3(256), 0, s, X, ldx, n, D, reinterpret_cast<unsigned int*>(meta + 1));
  ODX_CHECK_LAUNCH("odx_split_f8(absmax)");
  const int groups = (int)ceil_div(D, 128) * 16;
  for (int64_t r0 = 0; r0 < n; r0 += 65535) {
    const int64_t nr = n - r0 < 65535 ? n - r0 : 65535;
    hipLaunchKernelGGL(split_f8_kernel, dim3((unsigned)ceil_div(groups, 256), (unsigned)nr), dim3(256), 0, s, X + r0 * ldx, ldx, nr, D,
                       (uint32_t*)P + r0 * (ldp8 / 4), ldp8 / 4, meta);
    ODX_CHECK_LAUNCH("odx_split_f8");
  }
  if (qsq != nullptr) {
    hipLaunchKernelGGL(f8_row_sqnorm_kernel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, s, (const uint32_t*)P, ldp8 / 4, n,
                       (int)(round_up(D, 128) / 4), meta, qsq);
    ODX_CHECK_LAUNCH("odx_split_f8(norms)");
  }
  return ODX_OK;
}

extern "C" int odx_gauss_knm_f8_store(const void* PX, int64_t ldpx8, const float* metax, const float* xsq, int64_t n,
                                      const void* PZ, int64_t ldpz8, const float* metaz, const float* zsq, int64_t M, int D,
                                      double sigma, int fmt, void* K, int64_t ldk, void* Klo, int64_t ldlo, const double* w,
                                      double* ktw, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  ODX_REQUIRE(ldpx8 % 16 == 0 && ldpz8 % 16 == 0, "odx_gauss_knm_f8_store: operand row strides (bytes) must be multiples of 16");
  return knm_store_impl("odx_gauss_knm_f8_store", CORE_F8, PX, ldpx8 / 4, metax, xsq, n, PZ, ldpz8 / 4, metaz, zsq, M, D, sigma, fmt, K,
                        ldk, Klo, ldlo, w, ktw, workspace, workspace_bytes, stream);
}

// Column tiles per workgroup on the 128 x 128 core: MMV_TG when that still gives every CU two workgroups, fewer for
// small scoring calls (a Minibootstrap predict of 2000 rows against 2000 centres is 16 x 16 tiles: 64 workgroups of 4
// tiles each left three quarters of the chip idle for 300 us; 256 workgroups of one tile take 90 us).  A function of the
// call's shape only, so equal calls give equal bits.
static int mmv_tg(int64_t n, int64_t max_range, int C) {
  const int64_t rb = ceil_div(n, GEMM_BM), ct = ceil_div(max_range, GEMM_BN);
  int tg = MMV_TG;
  while (tg > 1 && rb * ceil_div(ct, tg) * C < 512) tg >>= 1;
  return tg;
}

// groups of column tiles (counted from the range's own first row) a centre range of at most `max_range` rows spans
static int64_t mmv_groups(int64_t max_range, int tg) { return ceil_div(ceil_div(max_range, GEMM_BN), tg); }

extern "C" int64_t odx_gauss_mmv_h2_workspace_bytes(int64_t n, int64_t max_range, int T) {
  if (n <= 0 || max_range <= 0 || T <= 0) return 0;
  return (int64_t)T * mmv_groups(max_range, mmv_tg(n, max_range, T)) * round_up(n, 2) * (int64_t)sizeof(double);
}

template <int CORE, int KIND = ODX_KERNEL_GAUSS>
static int launch_mmv_w256(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n, const void* PZ,
                           int64_t ldpz, const float* metaz, const float* zsq, int64_t max_range, int stages, double sigma,
                           const double* V, int64_t ldv, const int32_t* ranges, int C, float* out, int64_t ldo, double* slab,
                           int64_t slab_ld, odx_stream_t stream) {
  const int64_t Gw = ceil_div(ceil_div(max_range, W_BN), W_MMV_TG);      // <= mmv_groups(max_range): the slab is large enough
  const int64_t wgs = round_up(ceil_div(n, W_BM), 8) * Gw;
  ODX_REQUIRE(wgs < (1ll << 31), "odx_gauss_mmv: grid too large");
  ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gauss_mmv_h2w256_kernel<CORE, KIND>), W_LDS_BYTES));
  hipLaunchKernelGGL((gauss_mmv_h2w256_kernel<CORE, KIND>), dim3((unsigned)wgs, (unsigned)C), dim3(W_THREADS), W_LDS_BYTES,
                     as_stream(stream), (const uint32_t*)PX, ldpx, metax, xsq, n, (const uint32_t*)PZ, ldpz, metaz, zsq, stages,
                     h2_gamma_log2e(sigma), V, ldv, ranges, W_MMV_TG, (int)Gw, slab, slab_ld);
  ODX_CHECK_LAUNCH("odx_gauss_mmv(w256)");
  hipLaunchKernelGGL(mmv_reduce_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)C), dim3(256), 0, as_stream(stream), slab,
                     slab_ld, (int)Gw, W_MMV_TG, W_BN, ranges, n, out, ldo);
  ODX_CHECK_LAUNCH("odx_gauss_mmv(reduce)");
  return ODX_OK;
}

// The fused scoring with per-column centre ranges behind the entries' own operand checks: the tile core, the groups of
// column tiles, the launch and the sum of the groups.  core: CORE_H2 (packed two-term rows with their meta words) or
// CORE_BF16 / CORE_F16 (plain 16-bit rows, no meta); ld in 4-byte units either way.
static int mmv_ranges_run(const char* who, int core, const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                          const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t max_range, int D, double sigma,
                          const double* V, int64_t ldv, const int32_t* ranges, int C, float* out, int64_t ldo, void* workspace,
                          int64_t workspace_bytes, odx_stream_t stream, int kind = ODX_KERNEL_GAUSS) {
  ODX_REQUIRE(ldo >= C && C < 65536, "%s: ldo < C or too many classes", who);
  if (workspace == nullptr || workspace_bytes < odx_gauss_mmv_h2_workspace_bytes(n, max_range, C)) {
    set_error("%s: workspace too small", who);
    return ODX_ERR_WORKSPACE;
  }
  double* slab = static_cast<double*>(workspace);
  const int64_t slab_ld = round_up(n, 2);
  const int stages = core_stages(D, core);             // 128-byte pieces of an operand row; a k-tile of the 128 x 128 core is two
  if (kind != ODX_KERNEL_GAUSS) {      // a Matern kind: the wide core at every shape (its groups never outnumber the slab's: launch_mmv_w256)
    ODX_REQUIRE(core == CORE_H2, "%s: a Matern kernel needs the split-f16 operands", who);
    return with_matern_kind(kind, [&](auto k) {
      return launch_mmv_w256<CORE_H2, decltype(k)::value>(PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, max_range, stages, sigma, V, ldv,
                                                          ranges, C, out, ldo, slab, slab_ld, stream);
    });
  }
  if (h2_use_w256(ceil_div(n, W_BM) * ceil_div(ceil_div(max_range, W_BN), W_MMV_TG) * C)) {
    auto run = [&](auto c) {
      return launch_mmv_w256<decltype(c)::value>(PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, max_range, stages, sigma, V, ldv, ranges, C,
                                                 out, ldo, slab, slab_ld, stream);
    };
    return core == CORE_BF16 ? run(IntC<CORE_BF16>()) : core == CORE_F16 ? run(IntC<CORE_F16>()) : run(IntC<CORE_H2>());
  }
  const int tg = mmv_tg(n, max_range, C);
  const int G = (int)mmv_groups(max_range, tg);
  const int64_t wgs = round_up(ceil_div(n, GEMM_BM), 8) * G;
  ODX_REQUIRE(wgs < (1ll << 31), "%s: grid too large", who);
  auto run = [&](auto c) {
    constexpr int CORE = decltype(c)::value;
    ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gauss_mmv_h2s16_kernel<CORE>)));
    hipLaunchKernelGGL(gauss_mmv_h2s16_kernel<CORE>, dim3((unsigned)wgs, (unsigned)C), dim3(GEMM_THREADS), S16_LDS_BYTES,
                       as_stream(stream), (const uint32_t*)PX, ldpx, metax, xsq, n, (const uint32_t*)PZ, ldpz, metaz, zsq,
                       (stages + 1) / 2, h2_gamma_log2e(sigma), V, ldv, ranges, tg, G, slab, slab_ld, stages & 1);
    return (int)ODX_OK;
  };
  ODX_PROPAGATE(core == CORE_BF16 ? run(IntC<S16_BF16>()) : core == CORE_F16 ? run(IntC<S16_F16>()) : run(IntC<S16_H2>()));
  ODX_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(mmv_reduce_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)C), dim3(256), 0, as_stream(stream), slab,
                     slab_ld, G, tg, GEMM_BN, ranges, n, out, ldo);
  ODX_CHECK_LAUNCH(who);
  return ODX_OK;
}

static int mmv_h2_entry(const char* who, const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n, const void* PZ,
                        int64_t ldpz, const float* metaz, const float* zsq, int64_t max_range, int D, double sigma, int kind,
                        const double* V, int64_t ldv, const int32_t* ranges, int C, float* out, int64_t ldo, void* workspace,
                        int64_t workspace_bytes, odx_stream_t stream) {
  ODX_REQUIRE(radial_kind_known(kind), "%s: unknown kernel kind %d", who, kind);
  if (n <= 0 || C <= 0) return ODX_OK;
  ODX_REQUIRE(PX && PZ && metax && metaz && xsq && zsq && V && ranges && out && D > 0 && sigma > 0 && ldv >= C && max_range > 0,
              "%s: bad argument", who);
  ODX_PROPAGATE(check_packed_pair(who, round_up(D, H2_KT), ldpx, ldpz, PX, PZ));
  return mmv_ranges_run(who, CORE_H2, PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, max_range, D, sigma, V, ldv, ranges, C,
                        out, ldo, workspace, workspace_bytes, stream, kind);
}

extern "C" int odx_gauss_mmv_h2(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t max_range, int D,
                                double sigma, const double* V, int64_t ldv, const int32_t* ranges, int C, float* out,
                                int64_t ldo, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  return mmv_h2_entry("odx_gauss_mmv_h2", PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, max_range, D, sigma, ODX_KERNEL_GAUSS, V, ldv,
                      ranges, C, out, ldo, workspace, workspace_bytes, stream);
}

extern "C" int odx_radial_mmv_h2(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                 const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t max_range, int D,
                                 double sigma, int kind, const double* V, int64_t ldv, const int32_t* ranges, int C, float* out,
                                 int64_t ldo, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  return mmv_h2_entry("odx_radial_mmv_h2", PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, max_range, D, sigma, kind, V, ldv, ranges, C,
                      out, ldo, workspace, workspace_bytes, stream);
}

extern "C" int64_t odx_gauss_mmv_b16_workspace_bytes(int64_t n, int64_t max_range, int T) {
  return odx_gauss_mmv_h2_workspace_bytes(n, max_range, T);
}

// odx_gauss_mmv_h2 for 16-bit rows (both tile cores; h2_tile pins one as for the split kernels)
extern "C" int odx_gauss_mmv_b16(const void* X, int64_t ldx, const float* xsq, int64_t n, const void* Z, int64_t ldz, const float* zsq,
                                 int64_t max_range, int D, int is_bf16, double sigma, const double* V, int64_t ldv,
                                 const int32_t* ranges, int C, float* out, int64_t ldo, void* workspace, int64_t workspace_bytes,
                                 odx_stream_t stream) {
  if (n <= 0 || C <= 0) return ODX_OK;
  ODX_REQUIRE(X && Z && xsq && zsq && V && ranges && out && D > 0 && sigma > 0 && ldv >= C && max_range > 0, "odx_gauss_mmv_b16: bad argument");
  ODX_PROPAGATE(check_b16_pair("odx_gauss_mmv_b16", D, ldx, ldz, X, Z));
  return mmv_ranges_run("odx_gauss_mmv_b16", is_bf16 ? CORE_BF16 : CORE_F16, X, ldx / 2, nullptr, xsq, n, Z, ldz / 2, nullptr, zsq, max_range,
                        D, sigma, V, ldv, ranges, C, out, ldo, workspace, workspace_bytes, stream);
}

// ---- shared-centre scoring: all T columns of a dense V from one evaluation of K per group of up to 8 columns
struct MmvnArgs {
  const char* who;
  const uint32_t *PX, *PZ;
  int64_t ldpx, ldpz, n, M, ldv, slab_ld;
  const float *metax, *xsq, *metaz, *zsq;
  const double* V;
  double* slab;
  int kt, T, tg, G;          // kt: k-tiles (128 x 128 core) or stages (256 x 256 core)
  int core, half_tail;       // CORE_H2, or CORE_BF16 / CORE_F16 (plain 16-bit rows, one width); 128 x 128 core: the last k-tile is half a one
  int kind;                  // ODX_KERNEL_*; a Matern kind: CORE_H2, the wide core, one width
  unsigned wgs;
  hipStream_t stream;
};

// `groups` groups of NV columns from column cbase on
template <int NV, bool WIDE, bool PERCOL, int CORE, int KIND = ODX_KERNEL_GAUSS>
static int launch_mmvn_group_core(const MmvnArgs& a, const MmvnGammas& gm, int cbase, int groups) {
  if (WIDE) {
    ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gauss_mmvn_h2w256_kernel<NV, CORE, PERCOL, KIND>), W_LDS_BYTES));
    hipLaunchKernelGGL((gauss_mmvn_h2w256_kernel<NV, CORE, PERCOL, KIND>), dim3(a.wgs, (unsigned)groups), dim3(W_THREADS), W_LDS_BYTES,
                       a.stream, a.PX, a.ldpx, a.metax, a.xsq, a.n, a.PZ, a.ldpz, a.metaz, a.zsq, a.M, a.kt, gm, a.V, a.ldv, cbase, a.T,
                       a.tg, a.G, a.slab, a.slab_ld);
  } else {
    ODX_PROPAGATE(h2_enable_lds(reinterpret_cast<const void*>(gauss_mmvn_h2s16_kernel<NV, PERCOL, CORE>)));
    hipLaunchKernelGGL((gauss_mmvn_h2s16_kernel<NV, PERCOL, CORE>), dim3(a.wgs, (unsigned)groups), dim3(GEMM_THREADS), S16_LDS_BYTES,
                       a.stream, a.PX, a.ldpx, a.metax, a.xsq, a.n, a.PZ, a.ldpz, a.metaz, a.zsq, a.M, a.kt, gm, a.V, a.ldv, cbase, a.T,
                       a.tg, a.G, a.slab, a.slab_ld, a.half_tail);
  }
  ODX_CHECK_LAUNCH(a.who);
  return ODX_OK;
}

template <int NV, bool WIDE, bool PERCOL>
static int launch_mmvn_group(const MmvnArgs& a, const MmvnGammas& gm, int cbase, int groups) {
  if constexpr (!PERCOL && WIDE) {  // (a Matern kind: the wide core, the split rows, one width: mmvn_run)
    if (a.kind != ODX_KERNEL_GAUSS)
      return with_matern_kind(a.kind, [&](auto k) {
        return launch_mmvn_group_core<NV, true, false, CORE_H2, decltype(k)::value>(a, gm, cbase, groups);
      });
  }
  if constexpr (!PERCOL) {          // (a width per column exists for the split rows only: mmvn_run)
    if (a.core == CORE_BF16) return launch_mmvn_group_core<NV, WIDE, false, CORE_BF16>(a, gm, cbase, groups);
    if (a.core == CORE_F16) return launch_mmvn_group_core<NV, WIDE, false, CORE_F16>(a, gm, cbase, groups);
  }
  return launch_mmvn_group_core<NV, WIDE, PERCOL, CORE_H2>(a, gm, cbase, groups);
}

// one group of `rest` <= 8 columns on the next instantiated width
template <bool WIDE, bool PERCOL>
static int launch_mmvn_rest(const MmvnArgs& a, const MmvnGammas& gm, int cbase, int rest) {
  if (rest > 4) return launch_mmvn_group<8, WIDE, PERCOL>(a, gm, cbase, 1);
  if (rest > 2) return launch_mmvn_group<4, WIDE, PERCOL>(a, gm, cbase, 1);
  return launch_mmvn_group<2, WIDE, PERCOL>(a, gm, cbase, 1);
}

// One width (sigmas == nullptr): the full groups of 8 columns in one launch, what remains in one more.  A width per column:
// one launch per group of up to 8 columns, its scaled exponents by value (padding columns repeat the last one).
template <bool WIDE>
static int launch_mmvn(const MmvnArgs& a, double sigma, const double* sigmas) {
  MmvnGammas gm;
  if (sigmas == nullptr) {
    for (int c = 0; c < 8; ++c) gm.g[c] = h2_gamma_log2e(sigma);
    const int full = a.T / 8, rest = a.T % 8;
    if (full) ODX_PROPAGATE((launch_mmvn_group<8, WIDE, false>(a, gm, 0, full)));
    return rest ? launch_mmvn_rest<WIDE, false>(a, gm, 8 * full, rest) : ODX_OK;
  }
  for (int cbase = 0; cbase < a.T; cbase += 8) {
    const int rest = a.T - cbase < 8 ? a.T - cbase : 8;
    for (int c = 0; c < 8; ++c) gm.g[c] = h2_gamma_log2e(sigmas[cbase + (c < rest ? c : rest - 1)]);
    ODX_PROPAGATE((launch_mmvn_rest<WIDE, true>(a, gm, cbase, rest)));
  }
  return ODX_OK;
}

// Both entries behind their own checks of the widths: the tile core, the groups of column tiles and the slab of
// odx_gauss_mmv_h2 for T columns (the same bits per column), the launches, the sum of the groups.
static int mmvn_run(const char* who, const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n, const void* PZ,
                    int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D, double sigma, const double* sigmas,
                    const double* V, int64_t ldv, int T, float* out, int64_t ldo, void* workspace, int64_t workspace_bytes,
                    odx_stream_t stream, int core = CORE_H2, int kind = ODX_KERNEL_GAUSS) {
  ODX_REQUIRE(PX && PZ && ((metax && metaz) || core_is_b16(core)) && xsq && zsq && V && out && D > 0 && ldv >= T && M > 0, "%s: bad argument", who);
  ODX_REQUIRE(kind == ODX_KERNEL_GAUSS || (core == CORE_H2 && sigmas == nullptr), "%s: a Matern kernel needs the split-f16 operands and one width", who);
  ODX_REQUIRE(!(core_is_b16(core) && sigmas), "%s: a width per column needs the split rows", who);
  const int stages = core_stages(D, core);            // 128-byte pieces of an operand row; a k-tile of the 128 x 128 core is two
  ODX_PROPAGATE(check_packed_pair(who, core_min_ld(D, core), ldpx, ldpz, PX, PZ));
  ODX_REQUIRE(ldo >= T && T < 65536, "%s: ldo < T or too many columns", who);
  if (workspace == nullptr || workspace_bytes < odx_gauss_mmv_h2_workspace_bytes(n, M, T)) {
    set_error("%s: workspace too small", who);
    return ODX_ERR_WORKSPACE;
  }
  MmvnArgs a;
  a.who = who, a.PX = (const uint32_t*)PX, a.PZ = (const uint32_t*)PZ, a.ldpx = ldpx, a.ldpz = ldpz, a.n = n, a.M = M, a.ldv = ldv;
  a.metax = metax, a.xsq = xsq, a.metaz = metaz, a.zsq = zsq, a.V = V, a.T = T, a.core = core, a.half_tail = 0, a.kind = kind;
  a.slab = static_cast<double*>(workspace), a.slab_ld = round_up(n, 2), a.stream = as_stream(stream);
  // (a Matern kind: the wide core at every shape; its groups never outnumber the slab's, as in launch_mmv_w256)
  const bool wide = kind != ODX_KERNEL_GAUSS || h2_use_w256(ceil_div(n, W_BM) * ceil_div(ceil_div(M, W_BN), W_MMV_TG) * T);
  int64_t wgs;
  if (wide) {
    a.tg = W_MMV_TG, a.G = (int)ceil_div(ceil_div(M, W_BN), W_MMV_TG), a.kt = stages;
    wgs = round_up(ceil_div(n, W_BM), 8) * a.G;
  } else {
    a.tg = mmv_tg(n, M, T), a.G = (int)mmv_groups(M, a.tg), a.kt = (stages + 1) / 2, a.half_tail = stages & 1;
    wgs = round_up(ceil_div(n, GEMM_BM), 8) * a.G;
  }
  ODX_REQUIRE(wgs < (1ll << 31), "%s: grid too large", who);
  a.wgs = (unsigned)wgs;
  ODX_PROPAGATE(wide ? launch_mmvn<true>(a, sigma, sigmas) : launch_mmvn<false>(a, sigma, sigmas));
  hipLaunchKernelGGL(mmvn_reduce_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)T), dim3(256), 0, a.stream, a.slab, a.slab_ld,
                     a.G, n, out, ldo);
  ODX_CHECK_LAUNCH(who);
  return ODX_OK;
}

extern "C" int64_t odx_gauss_mmvn_h2_workspace_bytes(int64_t n, int64_t M, int T) {
  return odx_gauss_mmv_h2_workspace_bytes(n, M, T);
}

static int mmvn_h2_entry(const char* who, const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n, const void* PZ,
                         int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D, double sigma, int kind, const double* V,
                         int64_t ldv, int T, float* out, int64_t ldo, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  ODX_REQUIRE(radial_kind_known(kind), "%s: unknown kernel kind %d", who, kind);
  if (n <= 0 || T <= 0) return ODX_OK;
  ODX_REQUIRE(sigma > 0, "%s: bad argument", who);
  return mmvn_run(who, PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, M, D, sigma, nullptr, V, ldv, T, out, ldo, workspace, workspace_bytes,
                  stream, CORE_H2, kind);
}

extern "C" int odx_gauss_mmvn_h2(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n, const void* PZ,
                                 int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D, double sigma,
                                 const double* V, int64_t ldv, int T, float* out, int64_t ldo, void* workspace,
                                 int64_t workspace_bytes, odx_stream_t stream) {
  return mmvn_h2_entry("odx_gauss_mmvn_h2", PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, M, D, sigma, ODX_KERNEL_GAUSS, V, ldv, T, out, ldo,
                       workspace, workspace_bytes, stream);
}

extern "C" int odx_radial_mmvn_h2(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n, const void* PZ,
                                  int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D, double sigma, int kind,
                                  const double* V, int64_t ldv, int T, float* out, int64_t ldo, void* workspace,
                                  int64_t workspace_bytes, odx_stream_t stream) {
  return mmvn_h2_entry("odx_radial_mmvn_h2", PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, M, D, sigma, kind, V, ldv, T, out, ldo,
                       workspace, workspace_bytes, stream);
}

extern "C" int64_t odx_gauss_mmvn_b16_workspace_bytes(int64_t n, int64_t M, int T) { return odx_gauss_mmv_h2_workspace_bytes(n, M, T); }

// odx_gauss_mmvn_h2 for 16-bit rows (both tile cores)
extern "C" int odx_gauss_mmvn_b16(const void* X, int64_t ldx, const float* xsq, int64_t n, const void* Z, int64_t ldz, const float* zsq,
                                  int64_t M, int D, int is_bf16, double sigma, const double* V, int64_t ldv, int T, float* out,
                                  int64_t ldo, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  if (n <= 0 || T <= 0) return ODX_OK;
  ODX_REQUIRE(sigma > 0 && D > 0, "odx_gauss_mmvn_b16: bad argument");
  ODX_PROPAGATE(check_b16_pair("odx_gauss_mmvn_b16", D, ldx, ldz, X, Z));
  return mmvn_run("odx_gauss_mmvn_b16", X, ldx / 2, nullptr, xsq, n, Z, ldz / 2, nullptr, zsq, M, D, sigma, nullptr, V, ldv, T, out, ldo,
                  workspace, workspace_bytes, stream, is_bf16 ? CORE_BF16 : CORE_F16);
}

extern "C" int64_t odx_gauss_mmvn_h2_sigmas_workspace_bytes(int64_t n, int64_t M, int T) {
  return odx_gauss_mmv_h2_workspace_bytes(n, M, T);
}

extern "C" int odx_gauss_mmvn_h2_sigmas(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                        const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D,
                                        const double* sigmas, const double* V, int64_t ldv, int T, float* out, int64_t ldo,
                                        void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  if (n <= 0 || T <= 0) return ODX_OK;
  ODX_REQUIRE(sigmas, "odx_gauss_mmvn_h2_sigmas: bad argument");
  for (int c = 0; c < T; ++c) ODX_REQUIRE(sigmas[c] > 0, "odx_gauss_mmvn_h2_sigmas: sigma[%d] <= 0", c);
  return mmvn_run("odx_gauss_mmvn_h2_sigmas", PX, ldpx, metax, xsq, n, PZ, ldpz, metaz, zsq, M, D, 0.0, sigmas, V, ldv, T, out, ldo,
                  workspace, workspace_bytes, stream);
}

// Fused scoring with the e4m3 contraction (throughput-only, see odx_split_f8): always on the 256 x 256 core; workspace as
// odx_gauss_mmv_h2_workspace_bytes.
extern "C" int odx_gauss_mmv_f8(const void* PX, int64_t ldpx8, const float* metax, const float* xsq, int64_t n,
                                const void* PZ, int64_t ldpz8, const float* metaz, const float* zsq, int64_t max_range, int D,
                                double sigma, const double* V, int64_t ldv, const int32_t* ranges, int C, float* out,
                                int64_t ldo, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  if (n <= 0 || C <= 0) return ODX_OK;
  ODX_REQUIRE(PX && PZ && metax && metaz && xsq && zsq && V && ranges && out && D > 0 && sigma > 0 && ldv >= C && max_range > 0,
              "odx_gauss_mmv_f8: bad argument");
  ODX_REQUIRE(ldpx8 % 16 == 0 && ldpz8 % 16 == 0 && ldpx8 >= round_up(D, 128) && ldpz8 >= round_up(D, 128) && aligned16(PX) && aligned16(PZ),
              "odx_gauss_mmv_f8: packed operands must be 16-byte aligned with row strides %% 16 == 0 and >= roundup(D, 128) bytes");
  ODX_REQUIRE(ldo >= C && C < 65536, "odx_gauss_mmv_f8: ldo < C or too many classes");
  ODX_REQUIRE(ldpx8 < (1 << 26) && ldpz8 < (1 << 26), "odx_gauss_mmv_f8: row strides must stay below 2^26 bytes (32-bit tile offsets)");
  if (workspace == nullptr || workspace_bytes < odx_gauss_mmv_h2_workspace_bytes(n, max_range, C)) {
    set_error("odx_gauss_mmv_f8: workspace too small");
    return ODX_ERR_WORKSPACE;
  }
  return launch_mmv_w256<CORE_F8>(PX, ldpx8 / 4, metax, xsq, n, PZ, ldpz8 / 4, metaz, zsq, max_range, core_stages(D, CORE_F8), sigma, V,
                                  ldv, ranges, C, out, ldo, static_cast<double*>(workspace), round_up(n, 2), stream);
}
