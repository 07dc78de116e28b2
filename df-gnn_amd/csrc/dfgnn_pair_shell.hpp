// dfgnn_pair_shell.hpp -- the kernel shell of the plain any-graph training pairs: what stands between an operator's
// per-row device routines and its launch_*_fwd / launch_*_bwd* functions, once for gt_train.hip, gt_bias_train.hip,
// gt_edge_train.hip, gt_gate_train.hip, gat_edge_train.hip, agnn_train.hip and gatedgcn_train.hip.  (The pairs with capped
// grids, partial-sum reduce kernels or tables in dynamic LDS -- gatv2*, gt_tbias, gt_typed -- and gat_train.hip with its row
// lists keep shells of their own.)
//
// An operator is three passes -- PASS: 0 forward, 1 backward CSR pass, 2 backward CSC pass -- each in two forms: a wave per
// row / column (any degree) and, for low-degree graphs (low_degree(n, nnz)), a group of G lanes per row / column.  The
// operator file describes itself with a traits type:
//   struct Op {
//     using Args = ...;                              // the argument struct: m, n_cols, nnz, h, f, row_ptr, col_ptr, at_head()
//     static constexpr int kGroupMaxDegree = ...;    // the cooperative switch's threshold, a constant of the operator file
//     static constexpr bool kFwdTiles = ...;         // the forward's wave form works in 64-edge tiles through LDS scratch
//     template <class C> static __device__ void fwd_row_wave(const Args &, int r, int lane, float *sw, int *sc);  // kFwdTiles
//     template <class C, int PASS, bool COOP> static __device__ void group_pass(const Args &, int r, int gid, int gl);
//   };
// group_pass is the pass's lane-group routine.  COOP: the row is taken by all EPW groups of the wave together (group gid:
// edges gid, gid + EPW, ...) and the partial results are merged across the groups.
#pragma once
#include "dfgnn_launch.hpp"

namespace dfgnn {

// general: a wave per row / column, grid-strided over the whole graph.  With Op::kFwdTiles the forward works in 64-edge
// tiles through the wave's LDS scratch; every other pass is the COOP form of the group routines (no LDS).
template <class Op, class C, int PASS>
__global__ __launch_bounds__(kBlock) void pair_wave_kernel(typename Op::Args a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  const int beg = blockIdx.x * kWavesPerBlock + wave, step = gridDim.x * kWavesPerBlock;
  if constexpr (PASS == 0 && Op::kFwdTiles) {
    __shared__ __attribute__((aligned(16))) float lds[kWavesPerBlock * kScratchFloatsPerWave];
    float *sw = lds + wave * kScratchFloatsPerWave;
    int *sc = reinterpret_cast<int *>(sw + kWave);
    for (int r = beg; r < n; r += step) Op::template fwd_row_wave<C>(a, r, lane, sw, sc);
  } else {
    for (int r = beg; r < n; r += step) Op::template group_pass<C, PASS, true>(a, r, lane / C::G, lane % C::G);
  }
}

// low-degree graphs: a workgroup takes blocks of kBlock / G consecutive rows, one lane group per row -- unless a wave's
// EPW rows include one of more than Op::kGroupMaxDegree entries (a hub of a citation graph), which a single lane group
// would walk serially while the rest of the wave waits: that wave takes its rows one after the other with all its
// groups on each (COOP).  The choice is wave-uniform (ballot): no barrier, no LDS.  As group_row_loop of gt_lowdeg.hip.
template <class Op, class C, int PASS>
__global__ __launch_bounds__(kBlock) void pair_group_kernel(typename Op::Args a) {
  constexpr int G = C::G, R = kBlock / G;  // rows per block
  const int gid = (threadIdx.x & (kWave - 1)) / G, gl = threadIdx.x % G, wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int *ptr = PASS == 2 ? a.col_ptr : a.row_ptr;
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  for (int b0 = blockIdx.x * R; b0 < n; b0 += gridDim.x * R) {
    const int r = b0 + threadIdx.x / G;
    const int deg = r < n ? ptr[r + 1] - ptr[r] : 0;
    if (__any(deg > Op::kGroupMaxDegree)) {
      for (int rr = b0 + wave * C::EPW; rr < min(n, b0 + (wave + 1) * C::EPW); ++rr)
        Op::template group_pass<C, PASS, true>(a, rr, gid, gl);
    } else if (r < n) {
      Op::template group_pass<C, PASS, false>(a, r, gid, gl);
    }
  }
}

inline dim3 pair_group_grid(int m, int h, int G) {
  const long per = kBlock / G;
  long blocks = ((long)m + per - 1) / per;
  if (blocks > 16384) blocks = 16384;
  return dim3((unsigned)(blocks < 1 ? 1 : blocks), h);
}
inline dim3 pair_wave_grid(int m, int h) {
  const long want = ((long)m + kWavesPerBlock - 1) / kWavesPerBlock;
  return dim3((unsigned)(want > (1 << 20) ? (1 << 20) : want), h);
}

template <class Op, int PASS>
int launch_pair_pass(const typename Op::Args &a, bool v4, hipStream_t s) {
  const int n = PASS == 2 ? a.n_cols : a.m;  // the form is chosen per pass, by the average degree of what it walks
  if (n == 0) return 0;  // nothing to walk and nothing to write (a rectangular graph without rows / without columns)
  const bool groups = low_degree(n, a.nnz);
  return dispatch_cfg(a.f, v4, [&](auto cfg) {
    using C = decltype(cfg);
    if (groups) pair_group_kernel<Op, C, PASS><<<pair_group_grid(n, a.h, C::G), kBlock, 0, s>>>(a);
    else pair_wave_kernel<Op, C, PASS><<<pair_wave_grid(n, a.h), kBlock, 0, s>>>(a);
    return launch_status();
  });
}

}  // namespace dfgnn
