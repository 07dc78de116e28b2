// segment_gate.hip -- the segment multi-head attention pair with a per-pair sigmoid gate on the attention weights, after the
// softmax, and the logits as an output whose gradient re-enters the backward: out = (softmax(x) o sigmoid(gate)) V with
// x = scale Q K^T + bias.  The C entries of include/dfgnn_segment_gate.h: EGT-style attention, the dense
// counterpart of gt_gate_train.hip.
//
// The kernels are the three bodies of dfgnn_segment.hpp with SegKind::Gated: the bias planes' addressing serves four more
// planes (gate, logits in the forward; gate, dlogits, dgate in the backward), each optional -- a null plane is a wave-uniform
// test inside these instances, not a further kernel.  The row statistic of the backward still collapses to one number per
// row, t_i = sum_j P g dA, so nothing of size n^2 is kept between the calls and delta[m, h] stays the only scratch.
//
// Grids follow from m and h alone -- ceil(m / 128) windows x h heads; nothing here reads the device from the host, allocates
// or synchronises.
#include <hip/hip_runtime.h>

#include "../../include/dfgnn_segment_gate.h"
#include "dfgnn_segment.hpp"

namespace dfgnn {

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_gate_fwd_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                             SegGate sg, const float *__restrict__ Q,
                                                                             const float *__restrict__ K, const float *__restrict__ V,
                                                                             float *__restrict__ out, float *__restrict__ row_max,
                                                                             float *__restrict__ row_sum) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_fwd_body<FR, SegKind::Gated, SegGate>(lds, m, h, scale, bounds, Q, K, V, out, row_max, row_sum, sg);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_gate_dq_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                            SegGate sg, const float *__restrict__ Q,
                                                                            const float *__restrict__ K, const float *__restrict__ V,
                                                                            const float *__restrict__ row_max,
                                                                            const float *__restrict__ row_sum,
                                                                            const float *__restrict__ dO, float *__restrict__ dQ,
                                                                            float *__restrict__ delta) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dq_body<FR, SegKind::Gated, SegGate>(lds, m, h, scale, bounds, Q, K, V, row_max, row_sum, dO, dQ, delta, sg);
}

template <int FR>
__global__ __launch_bounds__(kDenseThreads) void segment_mha_gate_dkv_kernel(int m, int h, float scale, const int *__restrict__ bounds,
                                                                             SegGate sg, const float *__restrict__ Q,
                                                                             const float *__restrict__ K, const float *__restrict__ V,
                                                                             const float *__restrict__ row_max,
                                                                             const float *__restrict__ row_sum,
                                                                             const float *__restrict__ dO,
                                                                             const float *__restrict__ delta, float *__restrict__ dK,
                                                                             float *__restrict__ dV) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  segment_dkv_body<FR, SegKind::Gated, SegGate>(lds, m, h, scale, bounds, bounds, Q, K, V, row_max, row_sum, dO, delta, dK, dV, sg);
}

// extents first, then the limits (as segment_mha.hip: 32-bit byte offsets into the feature rows, heads are the grid's y)
static int gate_check(int m, int h, int f, long long n_pairs) {
  if (n_pairs < 0 || m < 0 || h < 1 || f < 1) return kErrBadArg;
  if (!(f == 16 || f == 32 || f == 64 || f == 128) || h > 65535) return kErrUnsupported;
  if ((unsigned long long)m * (unsigned)h * (unsigned)f * 4ull >= (1ull << 32)) return kErrUnsupported;
  return 0;
}

template <class Fn>
static int dispatch_gate(int f, Fn &&fn) {
  if (f == 16) return fn(std::integral_constant<int, 16>{});
  if (f == 32) return fn(std::integral_constant<int, 32>{});
  if (f == 64) return fn(std::integral_constant<int, 64>{});
  if (f == 128) return fn(std::integral_constant<int, 128>{});
  return kErrUnsupported;
}

}  // namespace dfgnn

using namespace dfgnn;

extern "C" {

int dfgnn_segment_gate_abi_version(void) { return DFGNN_SEGMENT_GATE_ABI_VERSION; }

int dfgnn_segment_mha_gate_fwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                               const float *bias, const float *gate, const float *Q, const float *K, const float *V,
                               float *out, float *row_max, float *row_sum, float *logits, dfgnn_stream_t stream) {
  if (int rc = gate_check(m, h, f, n_pairs)) return rc;
  if ((row_max == nullptr) != (row_sum == nullptr)) return kErrBadArg;
  if (m == 0) return 0;
  if (!bounds || !row_off || !bias || !Q || !K || !V || !out) return kErrBadArg;
  const dim3 grid((m + kSegWindow - 1) / kSegWindow, h);
  const SegGate sg{{row_off, n_pairs, bias, nullptr}, gate, nullptr, logits, nullptr};
  return dispatch_gate(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (int rc = set_max_lds_cached(segment_mha_gate_fwd_kernel<FR>)) return rc;
    segment_mha_gate_fwd_kernel<FR><<<grid, kDenseThreads, SegFwdCfg<FR>::kLds, reinterpret_cast<hipStream_t>(stream)>>>(
        m, h, scale, bounds, sg, Q, K, V, out, row_max, row_sum);
    return launch_status();
  });
}

int dfgnn_segment_mha_gate_bwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                               const float *bias, const float *gate, const float *Q, const float *K, const float *V,
                               const float *row_max, const float *row_sum, const float *dO, const float *dlogits,
                               float *dQ, float *dK, float *dV, float *dbias, float *dgate, float *delta, dfgnn_stream_t stream) {
  if (int rc = gate_check(m, h, f, n_pairs)) return rc;
  if (m == 0) return 0;
  if (!bounds || !row_off || !bias || !Q || !K || !V || !row_max || !row_sum || !dO || !dQ || !dK || !dV || !delta) return kErrBadArg;
  if (dgate && !gate) return kErrBadArg;  // there is no gate to differentiate
  const dim3 grid((m + kSegWindow - 1) / kSegWindow, h);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const SegGate sg{{row_off, n_pairs, bias, dbias}, gate, dgate, nullptr, dlogits};
  return dispatch_gate(f, [&](auto fc) {
    constexpr int FR = decltype(fc)::value;
    if (int rc = set_max_lds_cached(segment_mha_gate_dq_kernel<FR>)) return rc;
    if (int rc = set_max_lds_cached(segment_mha_gate_dkv_kernel<FR>)) return rc;
    segment_mha_gate_dq_kernel<FR><<<grid, kDenseThreads, SegDqCfg<FR>::kLds, s>>>(m, h, scale, bounds, sg, Q, K, V, row_max,
                                                                                   row_sum, dO, dQ, delta);
    segment_mha_gate_dkv_kernel<FR><<<grid, kDenseThreads, SegDkvCfg<FR, true>::kLds, s>>>(m, h, scale, bounds, sg, Q, K, V, row_max,
                                                                                           row_sum, dO, delta, dK, dV);
    return launch_status();
  });
}

}  // extern "C"
