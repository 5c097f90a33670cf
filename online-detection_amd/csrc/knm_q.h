// Decoding of the compact K_nM formats (24-bit fixed point, bf16), shared by the pass kernels that read a stored block
// through 4-column chunks: knm_pass_q.hip (one and two vectors) and knm_pass_nv.hip (3 .. 8 vectors).
#pragma once
#include "odx_internal.h"

namespace odx {

typedef unsigned int u32x4q __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2q __attribute__((ext_vector_type(2)));
typedef double f64x2q __attribute__((ext_vector_type(2)));

enum { QF_U24 = 1, QF_BF16 = 2 };      // = ODX_KNM_U24 / ODX_KNM_BF16

// A thread's chunk: CW = 4 consecutive columns of a row — two dwords of the u16 plane, one of the u8 plane (the f32 kernel's
// columns per thread, so the same (NT, CH) cover a row; 8-column chunks with 16-byte loads measured no faster).
constexpr int QCW = 4;
template <int FMT, int CW>
struct QChunk {
  unsigned hi[CW / 2];
  unsigned lo[CW / 4];
};

// entry e (0 .. CW - 1) of a chunk as a double: the integer q for QF_U24 (value = q 2^-24), the value itself for QF_BF16
template <int FMT, int CW>
__device__ __forceinline__ double q_entry(const QChunk<FMT, CW>& k, int e) {
  const unsigned h = k.hi[e >> 1];
  if (FMT == QF_U24) {
    // v_perm_b32: selector bytes 0..3 pick bytes of the second source (the low-byte dword), 4..7 bytes of the first (the
    // u16 pair), 0x0c a zero byte: result = [low byte (e & 3) | u16 << 8]
    const unsigned sel = ((e & 1) ? 0x0c070600u : 0x0c050400u) | (unsigned)(e & 3);
    return (double)__builtin_amdgcn_perm(h, k.lo[e >> 2], sel);
  }
  return (double)__uint_as_float((e & 1) ? (h & 0xffff0000u) : (h << 16));
}

}  // namespace odx
