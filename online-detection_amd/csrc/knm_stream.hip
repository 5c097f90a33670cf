// Streamed CG pass (knm_storage "stream"): out = K'(K v + w) and, optionally, out2 = K'(K v2) over a shard whose K_nM block is
// NEVER stored whole.  K = K(X, Z) is recomputed for every pass, chunk of R rows by chunk, into a ring the size of a slice of
// the Infinity Cache, and each chunk is read back by the compact-format pass kernel while it is still resident there.
//
// Per chunk c (rows [r0, r0 + R)), all on the caller's stream, in order:
//   1. gauss_knm_h2w256_kernel (odx_gauss_knm_h2_store, 24-bit fixed point) writes K[r0 : r0 + R, :] into the ring: the very
//      entries a stored build of the whole shard holds in those rows (every entry depends on its row of X, its row of Z and
//      the two matrices' split scales only; the tile core is the same), so each entry is computed once per pass;
//   2. odx_knm_fwd_bwd_q (or odx_knm_fwd_bwd2_q for two vectors where it exists) makes K_c'(K_c v + w_c) from the ring;
//   3. stream_acc_kernel adds that chunk's M-vector into out (the first chunk's pass writes out directly).
// Every sum is f64 in a fixed order (the pass kernels' slab reductions, then the chunks in row order): bitwise reproducible run
// to run, no atomics.  Against a stored pass over the same entries only the f64 summation order differs.
//
// The ring's rows R: the residency rule of the Infinity Cache (a table stays resident while it plus every byte loaded or
// stored between two uses fits in about 256 MiB).  Between a chunk's write and its read the GPU touches the ring, the packed
// Z (re-read by every build), the chunk's packed X rows and the pass's slab workspace; R is the largest multiple of 256 rows
// that keeps those under STREAM_BUDGET, then trimmed to the row-tile count whose 256 x 256 tiles fill the CUs best (the build
// runs one tile per CU: 480 tiles at M = 1e4 leave 6 % of the second wave idle, 520 would leave 49 % of the third).
#include <algorithm>

#include "odx_internal.h"

namespace odx {

constexpr int64_t STREAM_BUDGET = 224ll << 20;     // bytes kept in flight between a chunk's write and its read (of 256 MiB)
constexpr int64_t STREAM_TILE = 256;               // rows / columns of one tile of the build (gauss_knm_h2w256_kernel)
constexpr int64_t STREAM_ALIGN = 256;              // alignment of the workspace's parts

__global__ __launch_bounds__(256) void stream_acc_kernel(double* __restrict__ out, const double* __restrict__ part, int64_t M) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < M) out[j] += part[j];
}

static int stream_acc(double* out, const double* part, int64_t M, hipStream_t s) {
  hipLaunchKernelGGL(stream_acc_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, s, out, part, M);
  ODX_CHECK_LAUNCH("odx_gauss_ktk_stream_h2(acc)");
  return ODX_OK;
}

// slab workspace of the pass kernels over a chunk (independent of the rows: the persistent grids are sized by the CUs)
static int64_t stream_pass_ws(int64_t M) {
  const int64_t one = odx_knm_fwd_bwd_q_workspace_bytes(1, M, ODX_KNM_U24);
  const int64_t two = odx_knm_fwd_bwd2_q_workspace_bytes(1, M, ODX_KNM_U24);
  return std::max(one, two);
}

// pass_ws: the slab workspace of the passes that read a chunk (default: the one- and two-vector passes')
static int64_t stream_rows(int64_t M, int D, int64_t pass_ws = -1) {
  if (M <= 0 || D <= 0 || odx_knm_fwd_bwd_q_workspace_bytes(1, M, ODX_KNM_U24) < 0) return 0;
  if (pass_ws < 0) pass_ws = stream_pass_ws(M);
  const int64_t ldp = round_up(D, 64) * 4;                          // bytes of one packed operand row
  const int64_t per_row = odx_knm_ld(M, ODX_KNM_U24) * 3 + ldp + 8;  // ring row + packed X row + its norm
  const int64_t fixed = M * (ldp + 4) + pass_ws;
  int64_t rt_max = (STREAM_BUDGET - fixed) / (per_row * STREAM_TILE);
  rt_max = std::max<int64_t>(1, std::min<int64_t>(rt_max, 64));
  int cus = odx_device_cus();
  if (cus <= 0) cus = 256;
  const int64_t ct = ceil_div(M, STREAM_TILE);
  // the row-tile count with the fewest idle tile slots per useful tile; a shorter chunk only when it is clearly better
  int64_t best = rt_max;
  double best_eff = 0.0;
  for (int64_t rt = rt_max; rt >= 1; --rt) {
    const int64_t tiles = rt * ct;
    const double eff = (double)tiles / (double)(round_up(tiles, cus));
    if (eff > best_eff + 0.02) best = rt, best_eff = eff;
  }
  return best * STREAM_TILE;
}

struct StreamLayout {
  int64_t R, ld, hi, lo, pass, part, part2, total;
};

static StreamLayout stream_layout(int64_t M, int D) {
  StreamLayout L{};
  L.R = stream_rows(M, D);
  if (L.R <= 0) return L;
  L.ld = odx_knm_ld(M, ODX_KNM_U24);
  int64_t off = 0;
  L.hi = off, off = round_up(off + L.R * L.ld * 2, STREAM_ALIGN);
  L.lo = off, off = round_up(off + L.R * L.ld, STREAM_ALIGN);
  L.pass = off, off = round_up(off + stream_pass_ws(M), STREAM_ALIGN);
  L.part = off, off = round_up(off + M * (int64_t)sizeof(double), STREAM_ALIGN);
  L.part2 = off, off = round_up(off + M * (int64_t)sizeof(double), STREAM_ALIGN);
  L.total = off;
  return L;
}

// ---- several vectors from ONE build of each chunk (odx_gauss_ktk_stream_h2n) ----

// out[q][j] += part[q][j] for the nv vectors of a chunk in one launch (blockIdx.y = q)
__global__ __launch_bounds__(256) void stream_accn_kernel(double* __restrict__ out, int64_t ldo, const double* __restrict__ part, int64_t ldp,
                                                          int64_t M) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t q = blockIdx.y;
  if (j < M) out[q * ldo + j] += part[q * ldp + j];
}

// the widest pass that exists over a 24-bit ring of M columns: 8 or 4 vectors (odx_knm_fwd_bwdn_q), 2 (odx_knm_fwd_bwd2_q), else 1
static int stream_group_width(int64_t M) {
  if (odx_knm_fwd_bwdn_q_workspace_bytes(1, M, ODX_KNM_U24, 8) >= 0) return 8;
  if (odx_knm_fwd_bwdn_q_workspace_bytes(1, M, ODX_KNM_U24, 4) >= 0) return 4;
  return odx_knm_fwd_bwd2_q_workspace_bytes(1, M, ODX_KNM_U24) >= 0 ? 2 : 1;
}

// slab workspace of the group passes over a chunk: the largest over the kernels this M uses (they run one after the other in it)
static int64_t streamn_pass_ws(int64_t M) {
  int64_t ws = stream_pass_ws(M);
  const int width = stream_group_width(M);
  if (width >= 4) ws = std::max(ws, odx_knm_fwd_bwdn_q_workspace_bytes(1, M, ODX_KNM_U24, width));
  return ws;
}

struct StreamNLayout {
  int64_t R, ld, hi, lo, pass, pass_bytes, part, ldp, total;
};

// ring rows: the rule of stream_rows with the group passes' slabs in place of the one- and two-vector passes'
static StreamNLayout streamn_layout(int64_t M, int D) {
  StreamNLayout L{};
  if (M <= 0 || D <= 0 || odx_knm_fwd_bwd_q_workspace_bytes(1, M, ODX_KNM_U24) < 0) return L;
  L.pass_bytes = streamn_pass_ws(M);
  L.R = stream_rows(M, D, L.pass_bytes);
  if (L.R <= 0) return L;
  L.ld = odx_knm_ld(M, ODX_KNM_U24);
  L.ldp = round_up(M, 2);                                           // rows of the part matrix stay 16-byte aligned
  int64_t off = 0;
  L.hi = off, off = round_up(off + L.R * L.ld * 2, STREAM_ALIGN);
  L.lo = off, off = round_up(off + L.R * L.ld, STREAM_ALIGN);
  L.pass = off, off = round_up(off + L.pass_bytes, STREAM_ALIGN);
  L.part = off, off = round_up(off + ODX_STREAM_MAX_VECTORS * L.ldp * (int64_t)sizeof(double), STREAM_ALIGN);
  L.total = off;
  return L;
}

}  // namespace odx

using namespace odx;

extern "C" int64_t odx_gauss_ktk_stream_h2_rows(int64_t M, int D) {
  const int64_t R = stream_rows(M, D);
  return R > 0 ? R : ODX_ERR_UNSUPPORTED;
}

extern "C" int64_t odx_gauss_ktk_stream_h2_workspace_bytes(int64_t n, int64_t M, int D) {
  if (n <= 0 || M <= 0) return 0;
  const StreamLayout L = stream_layout(M, D);
  return L.R > 0 ? L.total : ODX_ERR_UNSUPPORTED;
}

extern "C" int odx_gauss_ktk_stream_h2(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                       const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D,
                                       double sigma, const double* v, const double* v2, const double* w, double* out,
                                       double* out2, void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  ODX_REQUIRE(M > 0 && out, "odx_gauss_ktk_stream_h2: M <= 0 or null out");
  ODX_REQUIRE((v2 == nullptr) == (out2 == nullptr), "odx_gauss_ktk_stream_h2: v2 and out2 go together");
  hipStream_t s = as_stream(stream);
  const bool one = v != nullptr || w != nullptr;      // v = w = 0: out = 0 without a pass
  if (n <= 0 || !one) ODX_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)M * sizeof(double), s));
  if (n <= 0 && out2) ODX_CHECK_HIP(hipMemsetAsync(out2, 0, (size_t)M * sizeof(double), s));
  if (n <= 0 || (!one && v2 == nullptr)) return ODX_OK;
  ODX_REQUIRE(PX && PZ && metax && metaz && xsq && zsq && D > 0 && sigma > 0, "odx_gauss_ktk_stream_h2: bad argument");
  const StreamLayout L = stream_layout(M, D);
  if (L.R <= 0) {
    set_error("odx_gauss_ktk_stream_h2: M = %lld exceeds the 20440 columns the compact-format pass kernels are built for", (long long)M);
    return ODX_ERR_UNSUPPORTED;
  }
  if (workspace == nullptr || workspace_bytes < L.total || !aligned16(workspace)) {
    set_error("odx_gauss_ktk_stream_h2: workspace too small or not 16-byte aligned (%lld bytes needed)", (long long)L.total);
    return ODX_ERR_WORKSPACE;
  }
  char* ws = static_cast<char*>(workspace);
  void* hi = ws + L.hi;
  void* lo = ws + L.lo;
  void* pws = ws + L.pass;
  const int64_t pws_bytes = stream_pass_ws(M);
  double* part = reinterpret_cast<double*>(ws + L.part);
  double* part2 = reinterpret_cast<double*>(ws + L.part2);
  // two vectors from one read of the chunk where that pass exists (and w is absent); else two reads of the resident chunk
  const bool fused2 = one && v2 != nullptr && w == nullptr && v != nullptr && odx_knm_fwd_bwd2_q_workspace_bytes(1, M, ODX_KNM_U24) >= 0;
  const char* px = static_cast<const char*>(PX);
  for (int64_t r0 = 0; r0 < n; r0 += L.R) {
    const int64_t rows = std::min(L.R, n - r0);
    const bool first = r0 == 0;
    ODX_PROPAGATE(odx_gauss_knm_h2_store(px + r0 * ldpx * 4, ldpx, metax, xsq + r0, rows, PZ, ldpz, metaz, zsq, M, D, sigma, ODX_KNM_U24,
                                         hi, L.ld, lo, L.ld, nullptr, nullptr, nullptr, 0, stream));
    double* o1 = first ? out : part;
    double* o2 = first ? out2 : part2;
    if (fused2) {
      ODX_PROPAGATE(odx_knm_fwd_bwd2_q(hi, L.ld, lo, L.ld, ODX_KNM_U24, rows, M, v, v2, o1, o2, pws, pws_bytes, stream));
    } else {
      if (one) ODX_PROPAGATE(odx_knm_fwd_bwd_q(hi, L.ld, lo, L.ld, ODX_KNM_U24, rows, M, v, w ? w + r0 : nullptr, o1, pws, pws_bytes, stream));
      if (v2) ODX_PROPAGATE(odx_knm_fwd_bwd_q(hi, L.ld, lo, L.ld, ODX_KNM_U24, rows, M, v2, nullptr, o2, pws, pws_bytes, stream));
    }
    if (!first) {
      if (one) ODX_PROPAGATE(stream_acc(out, part, M, s));
      if (v2) ODX_PROPAGATE(stream_acc(out2, part2, M, s));
    }
  }
  return ODX_OK;
}

extern "C" int64_t odx_gauss_ktk_stream_h2n_rows(int64_t M, int D) {
  const StreamNLayout L = streamn_layout(M, D);
  return L.R > 0 ? L.R : ODX_ERR_UNSUPPORTED;
}

extern "C" int64_t odx_gauss_ktk_stream_h2n_workspace_bytes(int64_t n, int64_t M, int D, int nv) {
  if (nv < 1 || nv > ODX_STREAM_MAX_VECTORS) return ODX_ERR_UNSUPPORTED;
  const StreamNLayout L = streamn_layout(M, D);
  if (L.R <= 0) return ODX_ERR_UNSUPPORTED;
  return n <= 0 ? 0 : L.total;
}

extern "C" int odx_gauss_ktk_stream_h2n(const void* PX, int64_t ldpx, const float* metax, const float* xsq, int64_t n,
                                        const void* PZ, int64_t ldpz, const float* metaz, const float* zsq, int64_t M, int D,
                                        double sigma, int nv, const double* V, int64_t ldv, double* out, int64_t ldo,
                                        void* workspace, int64_t workspace_bytes, odx_stream_t stream) {
  ODX_REQUIRE(M > 0 && nv >= 1 && nv <= ODX_STREAM_MAX_VECTORS, "odx_gauss_ktk_stream_h2n: M <= 0 or nv outside 1 .. %d", ODX_STREAM_MAX_VECTORS);
  ODX_REQUIRE(V && out && aligned16(V) && aligned16(out) && ldv % 2 == 0 && ldo % 2 == 0 && ldv >= M && ldo >= M,
              "odx_gauss_ktk_stream_h2n: V and out must be 16-byte aligned with even ldv, ldo >= M");
  hipStream_t s = as_stream(stream);
  if (n <= 0) {
    ODX_CHECK_HIP(hipMemset2DAsync(out, (size_t)ldo * sizeof(double), 0, (size_t)M * sizeof(double), (size_t)nv, s));
    return ODX_OK;
  }
  ODX_REQUIRE(PX && PZ && metax && metaz && xsq && zsq && D > 0 && sigma > 0, "odx_gauss_ktk_stream_h2n: bad argument");
  const StreamNLayout L = streamn_layout(M, D);
  if (L.R <= 0) {
    set_error("odx_gauss_ktk_stream_h2n: M = %lld exceeds the 20440 columns the compact-format pass kernels are built for", (long long)M);
    return ODX_ERR_UNSUPPORTED;
  }
  if (workspace == nullptr || workspace_bytes < L.total || !aligned16(workspace)) {
    set_error("odx_gauss_ktk_stream_h2n: workspace too small or not 16-byte aligned (%lld bytes needed)", (long long)L.total);
    return ODX_ERR_WORKSPACE;
  }
  char* ws = static_cast<char*>(workspace);
  void* hi = ws + L.hi;
  void* lo = ws + L.lo;
  void* pws = ws + L.pass;
  double* part = reinterpret_cast<double*>(ws + L.part);
  const int width = stream_group_width(M);
  const bool pairs = odx_knm_fwd_bwd2_q_workspace_bytes(1, M, ODX_KNM_U24) >= 0;
  const char* px = static_cast<const char*>(PX);
  for (int64_t r0 = 0; r0 < n; r0 += L.R) {
    const int64_t rows = std::min(L.R, n - r0);
    const bool first = r0 == 0;
    ODX_PROPAGATE(odx_gauss_knm_h2_store(px + r0 * ldpx * 4, ldpx, metax, xsq + r0, rows, PZ, ldpz, metaz, zsq, M, D, sigma, ODX_KNM_U24,
                                         hi, L.ld, lo, L.ld, nullptr, nullptr, nullptr, 0, stream));
    double* o = first ? out : part;
    const int64_t ld = first ? ldo : L.ldp;
    // the vectors in groups of the widest pass, each reading the resident chunk and reusing the one slab workspace
    for (int q = 0; q < nv;) {
      const int g = std::min(width, nv - q);
      const double* vq = V + (int64_t)q * ldv;
      double* oq = o + (int64_t)q * ld;
      if (g >= 3) {
        ODX_PROPAGATE(odx_knm_fwd_bwdn_q(hi, L.ld, lo, L.ld, ODX_KNM_U24, rows, M, g, vq, ldv, oq, ld, pws, L.pass_bytes, stream));
        q += g;
      } else if (g == 2 && pairs) {
        ODX_PROPAGATE(odx_knm_fwd_bwd2_q(hi, L.ld, lo, L.ld, ODX_KNM_U24, rows, M, vq, vq + ldv, oq, oq + ld, pws, L.pass_bytes, stream));
        q += 2;
      } else {
        ODX_PROPAGATE(odx_knm_fwd_bwd_q(hi, L.ld, lo, L.ld, ODX_KNM_U24, rows, M, vq, nullptr, oq, pws, L.pass_bytes, stream));
        q += 1;
      }
    }
    if (!first) {
      hipLaunchKernelGGL(stream_accn_kernel, dim3((unsigned)ceil_div(M, 256), (unsigned)nv), dim3(256), 0, s, out, ldo, part, L.ldp, M);
      ODX_CHECK_LAUNCH("odx_gauss_ktk_stream_h2n(acc)");
    }
  }
  return ODX_OK;
}
