// Decoding of the compact K_nM formats (24-bit fixed point, bf16), shared by the pass kernels that read a stored block
// through 4-column chunks: knm_pass_q.hip (one and two vectors), knm_pass_nv.hip (3 .. 8 vectors), knm_bwd_nv.hip and
// knm_fwd_nv.hip (1 .. 8 vectors, one direction); below it the host code those four files share.
#pragma once
#include <type_traits>

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

// ---------------------------------------------------------------------------------------------------- distinct columns
// A block may hold only the DISTINCT columns of a centre list of Mv positions that names some centres more than once
// (M <= Mv columns, in order of first occurrence).  The map: col_of[j] = the column of position j; start / pos = the
// positions of every column as a CSR list, ascending (start has M + 1 entries, pos Mv).  K_full v = K fold(v) and
// (K_full' t)[j] = (K' t)[col_of[j]].  Every index read from the map is clamped into its range: a malformed map gives wrong
// sums, never an access outside v or the slabs.
struct QCols {
  int64_t Mv = 0;
  const int* col_of = nullptr;
  const int* start = nullptr;
  const int* pos = nullptr;
  bool on() const { return start != nullptr; }
};

// fold(v)[d]: the sum of v over the positions of column d, left to right from 0.0 (the one statement of it: the pass
// kernels' load of v and odx_cols_fold_f64 give the same bits)
__device__ __forceinline__ double cols_fold_entry(const double* __restrict__ v, int64_t d, int64_t Mv, const int* __restrict__ start,
                                                  const int* __restrict__ pos) {
  const int last = (int)Mv - 1;
  int k = start[d], e = start[d + 1];
  k = k < 0 ? 0 : k;
  e = e > (int)Mv ? (int)Mv : e;
  double s = 0.0;
  for (; k < e; ++k) {
    int j = pos[k];
    j = j < 0 ? 0 : (j > last ? last : j);
    s += v[j];
  }
  return s;
}

// what slot i of a pass kernel's copy of v receives: v[i], or with a column map fold(v)[i]
__device__ __forceinline__ double q_v_entry(const double* __restrict__ v, int64_t i, int64_t Mv, const int* __restrict__ start,
                                            const int* __restrict__ pos) {
  return start == nullptr ? v[i] : cols_fold_entry(v, i, Mv, start, pos);
}

// ---------------------------------------------------------------------------------------------------- host side
// A compact block as the entries receive it.  The launches unpack it into the kernels' parameters.
struct QBlock {
  const unsigned short* hi;      // the u16 plane (u24: q >> 8; bf16: the bit patterns)
  int64_t ldk;
  const unsigned char* lo;       // the low-byte plane of u24
  int64_t ldlo;
  int fmt;
  int64_t n, M;
};

inline QBlock q_block(const void* K, int64_t ldk, const void* Klo, int64_t ldlo, int fmt, int64_t n, int64_t M) {
  return {static_cast<const unsigned short*>(K), ldk, static_cast<const unsigned char*>(Klo), ldlo, fmt, n, M};
}

inline bool q_format(int fmt) { return fmt == ODX_KNM_U24 || fmt == ODX_KNM_BF16; }

// f(format, block) with the block's format as a compile-time constant (std::integral_constant<int, QF_U24 | QF_BF16>: the
// kernels' FMT) and, for bf16, without the low-byte plane.  b.fmt has passed check_q_block.
template <typename F>
int q_dispatch(QBlock b, F&& f) {
  if (b.fmt == ODX_KNM_U24) return f(std::integral_constant<int, QF_U24>(), b);
  b.lo = nullptr, b.ldlo = 0;
  return f(std::integral_constant<int, QF_BF16>(), b);
}

// one launch; a kernel with dynamic LDS is allowed that much first
template <typename... P, typename... A>
int q_launch(void (*kernel)(P...), dim3 grid, int threads, size_t lds, hipStream_t s, A... args) {
  if (lds > 0)
    ODX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, s, args...);
  return ODX_OK;
}

// The NV-vector entries (odx_knm_fwd_bwdn_q, odx_knm_bwdn_q, odx_knm_fwdn_q): kernels exist for 2, 4 and 8 vectors, a call
// runs on the next width with zero vectors behind its own.  The two one-direction entries serve every M the compact
// passes serve.
constexpr int64_t Q_MAX_M = 20440;
inline int q_nvt(int nv) { return nv <= 2 ? 2 : nv <= 4 ? 4 : 8; }
inline bool q_nv_supported(int64_t M, int fmt, int nv) { return q_format(fmt) && M > 0 && M <= Q_MAX_M && nv >= 1 && nv <= 8; }
#define ODX_REQUIRE_Q_NV(who, M, fmt, nv)                                                                                          \
  do {                                                                                                                             \
    if (!q_nv_supported(M, fmt, nv)) {                                                                                             \
      set_error("%s: needs ODX_KNM_U24 or ODX_KNM_BF16, 1 <= M <= %lld and 1 <= nv <= 8 (got fmt %d, M %lld, nv %d)", who,         \
                (long long)Q_MAX_M, fmt, (long long)(M), nv);                                                                      \
      return ODX_ERR_UNSUPPORTED;                                                                                                  \
    }                                                                                                                              \
  } while (0)

// The compute units a workspace twin sizes for: the device's (256 where none is visible).  Not pass_cus(): a launch may be
// confined to fewer units (odx_set_pass_cus), never to more, so a workspace of this size serves every partition.
inline int workspace_cus() {
  const int cus = odx_device_cus();
  return cus > 0 ? cus : 256;
}

inline int require_workspace(const char* who, const void* workspace, int64_t workspace_bytes, int64_t need) {
  if (workspace != nullptr && workspace_bytes >= need) return ODX_OK;
  set_error("%s: workspace too small", who);
  return ODX_ERR_WORKSPACE;
}

// out[q] = the sum of vector q's nslab slabs, q = 0 .. nv - 1 <= 7 (slab[q][g][slab_ld]; the fixed-order reducer of knm_pass.hip)
inline int reduce_nv(int nv, int64_t M, int nslab, const double* slab, int64_t slab_ld, double* out, int64_t ldo, hipStream_t s) {
  int64_t Ms[8];
  int ns[8];
  for (int q = 0; q < nv; ++q) Ms[q] = M, ns[q] = nslab;
  return slab_reduce_batched_f64(nv, Ms, ns, slab, slab_ld, (int64_t)nslab * slab_ld, out, ldo, s);
}

}  // namespace odx
