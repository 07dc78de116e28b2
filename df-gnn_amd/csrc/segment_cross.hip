// segment_cross.hip -- multi-head CROSS attention over batched graphs: the queries of segment g, in one node array, attend to
// the keys of segment g in another.  The C entries of include/dfgnn_segment_cross.h.
//
// Two forms of the forward and of dQ.  WIDE: the bodies of dfgnn_segment.hpp with the query side's extent and bounds -- a
// 128-row query window and a head per workgroup, the kernels of segment_mha.hip on two arrays.  SPLIT
// (dfgnn_segment_cross.hpp): one 16-row query strip and a head per workgroup of four waves that divide every key tile
// between them, for few queries against many keys.  dK / dV has one form: 128-row KEY windows, the dK / dV body with the
// keys' bounds on the strip side and the queries' on the tile side.
//
// Grids follow from m_q, m_k and h alone; nothing here reads the device from the host, allocates or synchronises.
#include <hip/hip_runtime.h>

#include "../../include/dfgnn_segment_cross.h"
#include "dfgnn_segment_cross.hpp"

namespace dfgnn {

// one thread per row of either array: thread i < m_q is query i, thread m_q + j is key j.  The row's segment is the last one
// that starts at or before it in its OWN seg_ptr (empty segments in front of it share that start and are passed over); what
// it stores is that segment's range in the OTHER array, clamped into [0, other extent].
__global__ void segment_cross_bounds_kernel(int m_q, int m_k, int n_seg, const int *__restrict__ seg_ptr_q,
                                            const int *__restrict__ seg_ptr_k, int *__restrict__ qbounds,
                                            int *__restrict__ kbounds) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m_q + m_k) return;
  const bool key = i >= m_q;
  if (key) i -= m_q;
  const int *mine = key ? seg_ptr_k : seg_ptr_q, *other = key ? seg_ptr_q : seg_ptr_k;
  const int other_m = key ? m_q : m_k;
  int a = 0, b = n_seg - 1;  // mine[a] <= i (mine[0] = 0); the answer lies in [a, b]
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (mine[mid] <= i) a = mid;
    else b = mid - 1;
  }
  int *dst = key ? kbounds : qbounds;
  dst[2 * i] = min(max(other[a], 0), other_m);
  dst[2 * i + 1] = min(max(other[a + 1], 0), other_m);
}

// ---- the wide form: the bodies of dfgnn_segment.hpp, the strip side named ----------------------------------------------
template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_cross_fwd_kernel(int m_q, int h, float scale, const int *__restrict__ qbounds,
                                                                          const float *__restrict__ Q, const float *__restrict__ K,
                                                                          const float *__restrict__ V, float *__restrict__ out,
                                                                          float *__restrict__ row_max, float *__restrict__ row_sum) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_fwd_body<FR>(lds, m_q, h, scale, qbounds, Q, K, V, out, row_max, row_sum);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_cross_dq_kernel(int m_q, int h, float scale, const int *__restrict__ qbounds,
                                                                         const float *__restrict__ Q, const float *__restrict__ K,
                                                                         const float *__restrict__ V,
                                                                         const float *__restrict__ row_max,
                                                                         const float *__restrict__ row_sum,
                                                                         const float *__restrict__ dO, float *__restrict__ dQ,
                                                                         float *__restrict__ delta) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dq_body<FR>(lds, m_q, h, scale, qbounds, Q, K, V, row_max, row_sum, dO, dQ, delta);
}

// key strips: m_k and kbounds on the strip side, tiles of Q and dO whose staged (lo, hi) come from qbounds
template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_cross_dkv_kernel(int m_k, int h, float scale, const int *__restrict__ kbounds,
                                                                          const int *__restrict__ qbounds,
                                                                          const float *__restrict__ Q, const float *__restrict__ K,
                                                                          const float *__restrict__ V,
                                                                          const float *__restrict__ row_max,
                                                                          const float *__restrict__ row_sum,
                                                                          const float *__restrict__ dO,
                                                                          const float *__restrict__ delta, float *__restrict__ dK,
                                                                          float *__restrict__ dV) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dkv_body<FR>(lds, m_k, h, scale, kbounds, qbounds, Q, K, V, row_max, row_sum, dO, delta, dK, dV);
}

// ---- the split form (dfgnn_segment_cross.hpp) --------------------------------------------------------------------------
template <int FR>
__global__ __launch_bounds__(kSplitThreads) void segment_split_fwd_kernel(int m_q, int h, float scale, const int *__restrict__ qbounds,
                                                                          const float *__restrict__ Q, const float *__restrict__ K,
                                                                          const float *__restrict__ V, float *__restrict__ out,
                                                                          float *__restrict__ row_max, float *__restrict__ row_sum) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_split_fwd_body<FR>(lds, m_q, h, scale, qbounds, Q, K, V, out, row_max, row_sum);
}

template <int FR>
__global__ __launch_bounds__(kSplitThreads) void segment_split_dq_kernel(int m_q, int h, float scale, const int *__restrict__ qbounds,
                                                                         const float *__restrict__ Q, const float *__restrict__ K,
                                                                         const float *__restrict__ V,
                                                                         const float *__restrict__ row_max,
                                                                         const float *__restrict__ row_sum,
                                                                         const float *__restrict__ dO, float *__restrict__ dQ,
                                                                         float *__restrict__ delta) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_split_dq_body<FR>(lds, m_q, h, scale, qbounds, Q, K, V, row_max, row_sum, dO, dQ, delta);
}

static bool cross_width_ok(int f) { return f == 16 || f == 32 || f == 64 || f == 128; }

// extents (and the form) first, then the limits: 32-bit byte offsets into the feature rows of either side, heads are the grid's y
static int cross_check(int m_q, int m_k, int h, int f, int form) {
  if (m_q < 0 || m_k < 0 || h < 1 || f < 1 || form < DFGNN_SEGMENT_CROSS_AUTO || form > DFGNN_SEGMENT_CROSS_SPLIT) return kErrBadArg;
  if (!cross_width_ok(f) || h > 65535) return kErrUnsupported;
  const unsigned long long row = (unsigned long long)(unsigned)h * (unsigned)f * 4ull;
  if ((unsigned)m_q * row >= (1ull << 32) || (unsigned)m_k * row >= (1ull << 32)) return kErrUnsupported;
  return 0;
}

// AUTO, from the extents alone (DESIGN.md 3.3n has the table this was read from): the split form where a query has at least
// kCrossAutoRatio keys on average.  On the measured rows split wins a training step from 5.9 keys per query on, the forms
// tie at 1.5 and wide wins at 1; no row separated the forms by the size of the wide grid, so the rule does not look at it.
constexpr long long kCrossAutoRatio = 4;
static bool cross_split(int m_q, int m_k, int form) {
  if (form != DFGNN_SEGMENT_CROSS_AUTO) return form == DFGNN_SEGMENT_CROSS_SPLIT;
  return (long long)m_k >= kCrossAutoRatio * m_q;
}

template <class Fn>
static int dispatch_cross(int f, Fn &&fn) {
  if (f == 16) return fn(std::integral_constant<int, 16>{});
  if (f == 32) return fn(std::integral_constant<int, 32>{});
  if (f == 64) return fn(std::integral_constant<int, 64>{});
  if (f == 128) return fn(std::integral_constant<int, 128>{});
  return kErrUnsupported;
}

}  // namespace dfgnn

using namespace dfgnn;

extern "C" {

int dfgnn_segment_cross_abi_version(void) { return DFGNN_SEGMENT_CROSS_ABI_VERSION; }

int dfgnn_segment_cross_bounds(int m_q, int m_k, int n_seg, const int *seg_ptr_q, const int *seg_ptr_k, int *qbounds, int *kbounds,
                               dfgnn_stream_t stream) {
  if (m_q < 0 || m_k < 0 || n_seg < 0 || ((m_q > 0 || m_k > 0) && n_seg == 0)) return kErrBadArg;  // a row needs a segment
  if (m_q >= (1 << 30) || m_k >= (1 << 30)) return kErrUnsupported;                               // (2 m ints)
  if (m_q == 0 && m_k == 0) return 0;
  if (!seg_ptr_q || !seg_ptr_k || (m_q > 0 && !qbounds) || (m_k > 0 && !kbounds)) return kErrBadArg;
  const unsigned rows = (unsigned)m_q + (unsigned)m_k;
  segment_cross_bounds_kernel<<<(rows + 255) / 256, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(m_q, m_k, n_seg, seg_ptr_q,
                                                                                                      seg_ptr_k, qbounds, kbounds);
  return launch_status();
}

int dfgnn_segment_mha_cross_fwd(int m_q, int m_k, int h, int f, float scale, int form, const int *qbounds, const float *Q,
                                const float *K, const float *V, float *out, float *row_max, float *row_sum, dfgnn_stream_t stream) {
  if (int rc = cross_check(m_q, m_k, h, f, form)) return rc;
  if ((row_max == nullptr) != (row_sum == nullptr)) return kErrBadArg;
  if (m_q == 0) return 0;
  if (!qbounds || !Q || !out || (m_k > 0 && (!K || !V))) return kErrBadArg;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool split = cross_split(m_q, m_k, form);
  return dispatch_cross(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (split) {
      if (int rc = set_max_lds_cached(segment_split_fwd_kernel<FR>)) return rc;
      segment_split_fwd_kernel<FR><<<dim3((m_q + 15) / 16, h), kSplitThreads, SplitCfg<FR>::kLds, s>>>(m_q, h, scale, qbounds, Q, K, V,
                                                                                                       out, row_max, row_sum);
    } else {
      if (int rc = set_max_lds_cached(segment_cross_fwd_kernel<FR>)) return rc;
      segment_cross_fwd_kernel<FR><<<dim3((m_q + kSegWindow - 1) / kSegWindow, h), kDenseThreads, SegFwdCfg<FR>::kLds, s>>>(
          m_q, h, scale, qbounds, Q, K, V, out, row_max, row_sum);
    }
    return launch_status();
  });
}

int dfgnn_segment_mha_cross_bwd(int m_q, int m_k, int h, int f, float scale, int form, const int *qbounds, const int *kbounds,
                                const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                                const float *dO, float *dQ, float *dK, float *dV, float *delta, dfgnn_stream_t stream) {
  if (int rc = cross_check(m_q, m_k, h, f, form)) return rc;
  if (m_q == 0 && m_k == 0) return 0;
  if (m_q > 0 && (!qbounds || !Q || !row_max || !row_sum || !dO || !dQ || !delta)) return kErrBadArg;
  if (m_k > 0 && (!kbounds || !K || !V || !dK || !dV)) return kErrBadArg;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool split = cross_split(m_q, m_k, form);
  return dispatch_cross(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (m_q > 0) {  // dQ and delta
      if (split) {
        if (int rc = set_max_lds_cached(segment_split_dq_kernel<FR>)) return rc;
        segment_split_dq_kernel<FR><<<dim3((m_q + 15) / 16, h), kSplitThreads, SplitCfg<FR>::kLds, s>>>(
            m_q, h, scale, qbounds, Q, K, V, row_max, row_sum, dO, dQ, delta);
      } else {
        if (int rc = set_max_lds_cached(segment_cross_dq_kernel<FR>)) return rc;
        segment_cross_dq_kernel<FR><<<dim3((m_q + kSegWindow - 1) / kSegWindow, h), kDenseThreads, SegDqCfg<FR>::kLds, s>>>(
            m_q, h, scale, qbounds, Q, K, V, row_max, row_sum, dO, dQ, delta);
      }
    }
    if (m_k > 0) {  // dK, dV: every key row is written, zeros where no query sees it (all of them for m_q == 0)
      if (int rc = set_max_lds_cached(segment_cross_dkv_kernel<FR>)) return rc;
      segment_cross_dkv_kernel<FR><<<dim3((m_k + kSegWindow - 1) / kSegWindow, h), kDenseThreads, SegDkvCfg<FR>::kLds, s>>>(
          m_k, h, scale, kbounds, qbounds, Q, K, V, row_max, row_sum, dO, delta, dK, dV);
    }
    return launch_status();
  });
}

}  // extern "C"
