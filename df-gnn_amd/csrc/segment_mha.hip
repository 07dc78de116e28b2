// segment_mha.hip -- multi-head attention of every node over the nodes of its own graph in a batch: the C entries of
// include/dfgnn_segment.h, of include/dfgnn_segment_bias.h: the same pair with a per-pair bias added to the logits, and of
// include/dfgnn_segment_tbias.h: that bias looked up in the kernels from a table by the pair's type.  The kernel bodies and
// the design are in dfgnn_segment.hpp.
//
// The whole structure of the problem is seg_ptr [n_seg + 1].  dfgnn_segment_bounds turns it into (lo, hi) per node once
// per batch; every layer, head and direction reads that.  Grids follow from m alone -- ceil(m / 128) windows x h heads --
// so nothing here reads the device from the host, allocates or synchronises: the calls can be captured in a HIP graph.
#include <hip/hip_runtime.h>

#include "../../include/dfgnn_segment.h"
#include "../../include/dfgnn_segment_bias.h"
#include "../../include/dfgnn_segment_tbias.h"
#include "dfgnn_segment.hpp"

namespace dfgnn {

// one thread per node: the last segment that starts at or before it (empty segments in front of it share that start and
// are passed over), clamped into [0, m] so that no later kernel forms an address from an unchecked seg_ptr
__global__ void segment_bounds_kernel(int m, int n_seg, const int *__restrict__ seg_ptr, int *__restrict__ bounds) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  int a = 0, b = n_seg - 1;  // seg_ptr[a] <= i (seg_ptr[0] = 0); the answer lies in [a, b]
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (seg_ptr[mid] <= i) a = mid;
    else b = mid - 1;
  }
  bounds[2 * i] = min(max(seg_ptr[a], 0), m);
  bounds[2 * i + 1] = min(max(seg_ptr[a + 1], 0), m);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_fwd_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                        const float *__restrict__ Q, const float *__restrict__ K,
                                                                        const float *__restrict__ V, float *__restrict__ out,
                                                                        float *__restrict__ row_max, float *__restrict__ row_sum) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_fwd_body<FR>(lds, m, h, scale, bounds, Q, K, V, out, row_max, row_sum);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_dq_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                       const float *__restrict__ Q, const float *__restrict__ K,
                                                                       const float *__restrict__ V,
                                                                       const float *__restrict__ row_max,
                                                                       const float *__restrict__ row_sum,
                                                                       const float *__restrict__ dO, float *__restrict__ dQ,
                                                                       float *__restrict__ delta) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dq_body<FR>(lds, m, h, scale, bounds, Q, K, V, row_max, row_sum, dO, dQ, delta);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_dkv_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                        const float *__restrict__ Q, const float *__restrict__ K,
                                                                        const float *__restrict__ V,
                                                                        const float *__restrict__ row_max,
                                                                        const float *__restrict__ row_sum,
                                                                        const float *__restrict__ dO,
                                                                        const float *__restrict__ delta, float *__restrict__ dK,
                                                                        float *__restrict__ dV) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dkv_body<FR>(lds, m, h, scale, bounds, bounds, Q, K, V, row_max, row_sum, dO, delta, dK, dV);
}

// ---- the pair bias (include/dfgnn_segment_bias.h): the same bodies with BIAS, and the offsets they read ----------------------
// pair_ptr = exclusive prefix sum of n_g^2 by ONE workgroup walking the segments 1024 at a time: a wave scan, the waves'
// totals through LDS, the running total carried from chunk to chunk in a register.  Sizes come from seg_ptr clamped as
// segment_bounds_kernel clamps it.
constexpr int kPairScanThreads = 1024;
__global__ __launch_bounds__(kPairScanThreads) void segment_pair_ptr_kernel(int m, int n_seg, const int *__restrict__ seg_ptr,
                                                                            long long *__restrict__ pair_ptr) {
  __shared__ long long wave_total[kPairScanThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  long long carry = 0;
  for (int base = 0; base < n_seg; base += kPairScanThreads) {
    const int g = base + tid;
    long long n = 0;
    if (g < n_seg) n = max(min(max(seg_ptr[g + 1], 0), m) - min(max(seg_ptr[g], 0), m), 0);
    const long long v = n * n;
    long long incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
      const long long up = __shfl_up(incl, d, kWave);
      if (lane >= d) incl += up;
    }
    if (lane == kWave - 1) wave_total[wave] = incl;
    __syncthreads();
    long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kPairScanThreads / kWave; ++w) {
      const long long x = wave_total[w];
      if (w < wave) before += x;
      total += x;
    }
    if (g < n_seg) pair_ptr[g] = carry + before + incl - v;
    carry += total;
    __syncthreads();  // wave_total is posted to again
  }
  if (tid == 0) pair_ptr[n_seg] = carry;
}

// one thread per node: its segment as in segment_bounds_kernel, then row_off_i = pair_ptr[g] + (i - lo) n
__global__ void segment_row_off_kernel(int m, int n_seg, const int *__restrict__ seg_ptr, const long long *__restrict__ pair_ptr,
                                       long long *__restrict__ row_off) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  int a = 0, b = n_seg - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (seg_ptr[mid] <= i) a = mid;
    else b = mid - 1;
  }
  const int lo = min(max(seg_ptr[a], 0), m), hi = min(max(seg_ptr[a + 1], 0), m);
  row_off[i] = pair_ptr[a] + (long long)(i - lo) * max(hi - lo, 0);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_bias_fwd_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                             SegBias sb, const float *__restrict__ Q,
                                                                             const float *__restrict__ K, const float *__restrict__ V,
                                                                             float *__restrict__ out, float *__restrict__ row_max,
                                                                             float *__restrict__ row_sum) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_fwd_body<FR, SegKind::Plane>(lds, m, h, scale, bounds, Q, K, V, out, row_max, row_sum, sb);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_bias_dq_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                            SegBias sb, const float *__restrict__ Q,
                                                                            const float *__restrict__ K, const float *__restrict__ V,
                                                                            const float *__restrict__ row_max,
                                                                            const float *__restrict__ row_sum,
                                                                            const float *__restrict__ dO, float *__restrict__ dQ,
                                                                            float *__restrict__ delta) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dq_body<FR, SegKind::Plane>(lds, m, h, scale, bounds, Q, K, V, row_max, row_sum, dO, dQ, delta, sb);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_bias_dkv_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                             SegBias sb, const float *__restrict__ Q,
                                                                             const float *__restrict__ K, const float *__restrict__ V,
                                                                             const float *__restrict__ row_max,
                                                                             const float *__restrict__ row_sum,
                                                                             const float *__restrict__ dO,
                                                                             const float *__restrict__ delta, float *__restrict__ dK,
                                                                             float *__restrict__ dV) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dkv_body<FR, SegKind::Plane>(lds, m, h, scale, bounds, bounds, Q, K, V, row_max, row_sum, dO, delta, dK, dV, sb);
}

// ---- the typed pair bias (include/dfgnn_segment_tbias.h): the same bodies with SegKind::Typed ----------------------------------
template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_tbias_fwd_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                              SegTBias tb, const float *__restrict__ Q,
                                                                              const float *__restrict__ K, const float *__restrict__ V,
                                                                              float *__restrict__ out, float *__restrict__ row_max,
                                                                              float *__restrict__ row_sum) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_fwd_body<FR, SegKind::Typed, SegTBias>(lds, m, h, scale, bounds, Q, K, V, out, row_max, row_sum, tb);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_tbias_dq_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                             SegTBias tb, const float *__restrict__ Q,
                                                                             const float *__restrict__ K, const float *__restrict__ V,
                                                                             const float *__restrict__ row_max,
                                                                             const float *__restrict__ row_sum,
                                                                             const float *__restrict__ dO, float *__restrict__ dQ,
                                                                             float *__restrict__ delta) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dq_body<FR, SegKind::Typed, SegTBias>(lds, m, h, scale, bounds, Q, K, V, row_max, row_sum, dO, dQ, delta, tb);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_tbias_dkv_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                              SegTBias tb, const float *__restrict__ Q,
                                                                              const float *__restrict__ K, const float *__restrict__ V,
                                                                              const float *__restrict__ row_max,
                                                                              const float *__restrict__ row_sum,
                                                                              const float *__restrict__ dO,
                                                                              const float *__restrict__ delta, float *__restrict__ dK,
                                                                              float *__restrict__ dV) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dkv_body<FR, SegKind::Typed, SegTBias>(lds, m, h, scale, bounds, bounds, Q, K, V, row_max, row_sum, dO, delta, dK, dV, tb);
}

// dB[c] = sum over the work items' partials parts[p, c], c = t h + head: 64 columns per workgroup, wave w adds the partials
// w, w + 16, .. in that order, the 16 sums are added in wave order.  nparts == 0 writes zeros.
constexpr int kSegReduceWaves = 16;
__global__ __launch_bounds__(kSegReduceWaves *kWave) void segment_tbias_reduce_kernel(const float *__restrict__ parts, int nparts,
                                                                                      int th, float *__restrict__ dB) {
  __shared__ float red[kSegReduceWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = blockIdx.x * kWave + lane;
  float s = 0.f;
  if (c < th)
    for (int p = wave; p < nparts; p += kSegReduceWaves) s += parts[(size_t)p * th + c];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < th) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kSegReduceWaves; ++w) t += red[w][lane];
    dB[c] = t;
  }
}

// the typed kernels' LDS: the tile, the staged column of the table and, in a dQ kernel that sums dB, 8 wave tables
template <int FR>
constexpr int seg_tbias_dq_lds(int T, bool want_db) {
  return SegDqCfg<FR>::kLds + kSegTabBytes + (want_db ? kDenseWaves * T * seg_tbias_slots(T) * 4 : 0);
}
template <int FR>
constexpr bool seg_tbias_lds_ok() {
  return SegFwdCfg<FR>::kLds % 16 == 0 && SegDqCfg<FR>::kLds % 16 == 0 && SegDkvCfg<FR, true>::kLds % 16 == 0 &&
         SegFwdCfg<FR>::kLds + kSegTabBytes <= kBlockLdsBudget && SegDkvCfg<FR, true>::kLds + kSegTabBytes <= kBlockLdsBudget &&
         SegDqCfg<FR>::kLds + kSegTabBytes + kDenseWaves * kSegWaveTabFloats * 4 <= kBlockLdsBudget;
}
static_assert(seg_tbias_lds_ok<16>() && seg_tbias_lds_ok<32>() && seg_tbias_lds_ok<64>() && seg_tbias_lds_ok<128>(),
              "tile + staged table + 8 wave tables stay inside the LDS budget");

static bool segment_width_ok(int f) { return f == 16 || f == 32 || f == 64 || f == 128; }

// extents first, then the limits: the kernels address feature rows with 32-bit byte offsets, heads are the grid's y
static int segment_check(int m, int h, int f) {
  if (m < 0 || h < 1 || f < 1) return kErrBadArg;
  if (!segment_width_ok(f) || h > 65535) return kErrUnsupported;
  if ((unsigned long long)m * (unsigned)h * (unsigned)f * 4ull >= (1ull << 32)) return kErrUnsupported;
  return 0;
}

template <class Fn>
static int dispatch_segment(int f, Fn &&fn) {
  if (f == 16) return fn(std::integral_constant<int, 16>{});
  if (f == 32) return fn(std::integral_constant<int, 32>{});
  if (f == 64) return fn(std::integral_constant<int, 64>{});
  if (f == 128) return fn(std::integral_constant<int, 128>{});
  return kErrUnsupported;
}

}  // namespace dfgnn

using namespace dfgnn;

extern "C" {

int dfgnn_segment_abi_version(void) { return DFGNN_SEGMENT_ABI_VERSION; }

int dfgnn_segment_mha_applies(int h, int f) { return (h >= 1 && h <= 65535 && segment_width_ok(f)) ? 1 : 0; }

int dfgnn_segment_bounds(int m, int n_seg, const int *seg_ptr, int *bounds, dfgnn_stream_t stream) {
  if (m < 0 || n_seg < 0 || (m > 0 && n_seg == 0)) return kErrBadArg;  // a node needs a segment
  if (m >= (1 << 30)) return kErrUnsupported;                           // (2 m ints)
  if (m == 0) return 0;
  if (!seg_ptr || !bounds) return kErrBadArg;
  segment_bounds_kernel<<<(m + 255) / 256, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(m, n_seg, seg_ptr, bounds);
  return launch_status();
}

int dfgnn_segment_mha_fwd(int m, int h, int f, float scale, const int *bounds, const float *Q, const float *K, const float *V,
                          float *out, float *row_max, float *row_sum, dfgnn_stream_t stream) {
  if (int rc = segment_check(m, h, f)) return rc;
  if ((row_max == nullptr) != (row_sum == nullptr)) return kErrBadArg;
  if (m == 0) return 0;
  if (!bounds || !Q || !K || !V || !out) return kErrBadArg;
  const dim3 grid((m + kSegWindow - 1) / kSegWindow, h);
  return dispatch_segment(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (int rc = set_max_lds_cached(segment_mha_fwd_kernel<FR>)) return rc;
    segment_mha_fwd_kernel<FR><<<grid, kDenseThreads, SegFwdCfg<FR>::kLds, reinterpret_cast<hipStream_t>(stream)>>>(
        m, h, scale, bounds, Q, K, V, out, row_max, row_sum);
    return launch_status();
  });
}

int dfgnn_segment_mha_bwd(int m, int h, int f, float scale, const int *bounds, const float *Q, const float *K, const float *V,
                          const float *out, const float *row_max, const float *row_sum, const float *dO, float *dQ, float *dK,
                          float *dV, float *delta, dfgnn_stream_t stream) {
  (void)out;  // (delta comes from P and dP, not from the stored rows: dfgnn_segment.hpp)
  if (int rc = segment_check(m, h, f)) return rc;
  if (m == 0) return 0;
  if (!bounds || !Q || !K || !V || !row_max || !row_sum || !dO || !dQ || !dK || !dV || !delta) return kErrBadArg;
  const dim3 grid((m + kSegWindow - 1) / kSegWindow, h);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return dispatch_segment(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (int rc = set_max_lds_cached(segment_mha_dq_kernel<FR>)) return rc;
    if (int rc = set_max_lds_cached(segment_mha_dkv_kernel<FR>)) return rc;
    segment_mha_dq_kernel<FR><<<grid, kDenseThreads, SegDqCfg<FR>::kLds, s>>>(m, h, scale, bounds, Q, K, V, row_max,
                                                                                          row_sum, dO, dQ, delta);
    segment_mha_dkv_kernel<FR><<<grid, kDenseThreads, SegDkvCfg<FR>::kLds, s>>>(m, h, scale, bounds, Q, K, V, row_max,
                                                                                           row_sum, dO, delta, dK, dV);
    return launch_status();
  });
}

// ---- include/dfgnn_segment_bias.h ------------------------------------------------------------------------------------------
int dfgnn_segment_bias_abi_version(void) { return DFGNN_SEGMENT_BIAS_ABI_VERSION; }

int dfgnn_segment_pair_rows(int m, int n_seg, const int *seg_ptr, long long *pair_ptr, long long *row_off, dfgnn_stream_t stream) {
  if (m < 0 || n_seg < 0 || (m > 0 && n_seg == 0)) return kErrBadArg;
  if (m >= (1 << 30)) return kErrUnsupported;  // (as dfgnn_segment_bounds)
  if (m == 0) return 0;
  if (!seg_ptr || !pair_ptr || !row_off) return kErrBadArg;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  segment_pair_ptr_kernel<<<1, kPairScanThreads, 0, s>>>(m, n_seg, seg_ptr, pair_ptr);
  segment_row_off_kernel<<<(m + 255) / 256, 256, 0, s>>>(m, n_seg, seg_ptr, pair_ptr, row_off);
  return launch_status();
}

int dfgnn_segment_mha_bias_fwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                               const float *bias, const float *Q, const float *K, const float *V, float *out, float *row_max,
                               float *row_sum, dfgnn_stream_t stream) {
  if (n_pairs < 0) return kErrBadArg;
  if (int rc = segment_check(m, h, f)) return rc;
  if ((row_max == nullptr) != (row_sum == nullptr)) return kErrBadArg;
  if (m == 0) return 0;
  if (!bounds || !row_off || !bias || !Q || !K || !V || !out) return kErrBadArg;
  const dim3 grid((m + kSegWindow - 1) / kSegWindow, h);
  const SegBias sb{row_off, n_pairs, bias, nullptr};
  return dispatch_segment(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (int rc = set_max_lds_cached(segment_mha_bias_fwd_kernel<FR>)) return rc;
    segment_mha_bias_fwd_kernel<FR><<<grid, kDenseThreads, SegFwdCfg<FR>::kLds, reinterpret_cast<hipStream_t>(stream)>>>(
        m, h, scale, bounds, sb, Q, K, V, out, row_max, row_sum);
    return launch_status();
  });
}

int dfgnn_segment_mha_bias_bwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                               const float *bias, const float *Q, const float *K, const float *V, const float *row_max,
                               const float *row_sum, const float *dO, float *dQ, float *dK, float *dV, float *dbias,
                               float *delta, dfgnn_stream_t stream) {
  if (n_pairs < 0) return kErrBadArg;
  if (int rc = segment_check(m, h, f)) return rc;
  if (m == 0) return 0;
  if (!bounds || !row_off || !bias || !Q || !K || !V || !row_max || !row_sum || !dO || !dQ || !dK || !dV || !delta) return kErrBadArg;
  const dim3 grid((m + kSegWindow - 1) / kSegWindow, h);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const SegBias sb{row_off, n_pairs, bias, dbias};
  return dispatch_segment(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (int rc = set_max_lds_cached(segment_mha_bias_dq_kernel<FR>)) return rc;
    if (int rc = set_max_lds_cached(segment_mha_bias_dkv_kernel<FR>)) return rc;
    segment_mha_bias_dq_kernel<FR><<<grid, kDenseThreads, SegDqCfg<FR>::kLds, s>>>(m, h, scale, bounds, sb, Q, K, V, row_max,
                                                                                   row_sum, dO, dQ, delta);
    segment_mha_bias_dkv_kernel<FR><<<grid, kDenseThreads, SegDkvCfg<FR, true>::kLds, s>>>(m, h, scale, bounds, sb, Q, K, V, row_max,
                                                                                           row_sum, dO, delta, dK, dV);
    return launch_status();
  });
}

// ---- include/dfgnn_segment_tbias.h -----------------------------------------------------------------------------------------
int dfgnn_segment_tbias_abi_version(void) { return DFGNN_SEGMENT_TBIAS_ABI_VERSION; }

static int segment_tbias_check(int m, int h, int f, long long n_pairs, int T) {
  if (n_pairs < 0 || m < 0 || h < 1 || f < 1 || T < 1) return kErrBadArg;
  if (T > kSegMaxTypes) return kErrUnsupported;
  return segment_check(m, h, f);
}

long long dfgnn_segment_mha_tbias_ws_floats(int m, int h, int T) {
  if (m < 0 || h < 1 || T < 1) return kErrBadArg;
  if (T > kSegMaxTypes || h > 65535 || m >= (1 << 30)) return kErrUnsupported;
  return (long long)((m + kSegWindow - 1) / kSegWindow) * h * T;
}

int dfgnn_segment_mha_tbias_fwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                                const unsigned char *types, int T, const float *B, const float *Q, const float *K, const float *V,
                                float *out, float *row_max, float *row_sum, dfgnn_stream_t stream) {
  if (int rc = segment_tbias_check(m, h, f, n_pairs, T)) return rc;
  if ((row_max == nullptr) != (row_sum == nullptr)) return kErrBadArg;
  if (m == 0) return 0;
  if (!bounds || !row_off || !types || !B || !Q || !K || !V || !out) return kErrBadArg;
  const dim3 grid((m + kSegWindow - 1) / kSegWindow, h);
  const SegTBias tb{row_off, n_pairs, types, B, T, nullptr, 0, 0};
  return dispatch_segment(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (int rc = set_max_lds_cached(segment_mha_tbias_fwd_kernel<FR>)) return rc;
    segment_mha_tbias_fwd_kernel<FR><<<grid, kDenseThreads, SegFwdCfg<FR>::kLds + kSegTabBytes, reinterpret_cast<hipStream_t>(stream)>>>(
        m, h, scale, bounds, tb, Q, K, V, out, row_max, row_sum);
    return launch_status();
  });
}

int dfgnn_segment_mha_tbias_bwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                                const unsigned char *types, int T, const float *B, const float *Q, const float *K, const float *V,
                                const float *row_max, const float *row_sum, const float *dO, float *dQ, float *dK, float *dV,
                                float *dB, float *ws, float *delta, dfgnn_stream_t stream) {
  if (int rc = segment_tbias_check(m, h, f, n_pairs, T)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int th = T * h, nparts = (m + kSegWindow - 1) / kSegWindow;
  if (m == 0) {  // nothing to differentiate, but a wanted dB is zeros
    if (dB) segment_tbias_reduce_kernel<<<(th + kWave - 1) / kWave, kSegReduceWaves * kWave, 0, s>>>(nullptr, 0, th, dB);
    return dB ? launch_status() : 0;
  }
  if (!bounds || !row_off || !types || !B || !Q || !K || !V || !row_max || !row_sum || !dO || !dQ || !dK || !dV || !delta ||
      (dB && !ws))
    return kErrBadArg;
  const dim3 grid(nparts, h);
  int W = seg_tbias_slots(T), wshift = 0;
  while ((1 << wshift) < W) ++wshift;
  const SegTBias tb{row_off, n_pairs, types, B, T, dB ? ws : nullptr, W, wshift};
  return dispatch_segment(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (int rc = set_max_lds_cached(segment_mha_tbias_dq_kernel<FR>)) return rc;
    if (int rc = set_max_lds_cached(segment_mha_tbias_dkv_kernel<FR>)) return rc;
    segment_mha_tbias_dq_kernel<FR><<<grid, kDenseThreads, seg_tbias_dq_lds<FR>(T, dB != nullptr), s>>>(m, h, scale, bounds, tb, Q, K, V,
                                                                                                      row_max, row_sum, dO, dQ, delta);
    segment_mha_tbias_dkv_kernel<FR><<<grid, kDenseThreads, SegDkvCfg<FR, true>::kLds + kSegTabBytes, s>>>(
        m, h, scale, bounds, tb, Q, K, V, row_max, row_sum, dO, delta, dK, dV);
    if (dB) segment_tbias_reduce_kernel<<<(th + kWave - 1) / kWave, kSegReduceWaves * kWave, 0, s>>>(ws, nparts, th, dB);
    return launch_status();
  });
}

}  // extern "C"
