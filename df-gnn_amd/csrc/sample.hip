// sample.hip -- one hop of uniform neighbour sampling without replacement on the GPU (include/dfgnn_sample.h): the sampled
// block comes out with its CSR and CSC arrays made, in two calls around the one host read of the output sizes.
//
// What DFGNN.utils.graph.sample_block does in torch ops -- expand every candidate edge of every seed, draw a key per
// candidate, two argsorts over all candidates, torch.unique, two arrays of parent-graph size -- followed by the row sort of
// dfgnn_preprocess_hyper_rect, becomes:
//   select  a key is a hash of the edge's CSR position, so nothing is stored per candidate: a row with more than `fanout`
//           edges finds its fanout-th smallest key by a radix select (four 8-bit histogram passes that recompute the hashes),
//           every kept edge ORs its column into a bitmap of n bits; the block's row_ptr is a prefix sum of min(d, fanout)
//   emit    a row keeps key <= threshold by a ballot / popcount compaction, which IS parent order: no sort by row; a column's
//           block id is its seed's row (an int[n] read only where the seed bitmap is set) or m + its rank among the marked
//           nodes that are no seeds (a popcount scan over the bitmap words); the CSC half is preprocess.hip's column sort
// The two prefix sums (over m + 1 row counts and n / 32 + 1 word counts) are one workgroup each that walks its input in tiles:
// no temporary storage, one launch, and the workspace has a closed formula a host without a device can evaluate.
// Integer arithmetic only; the atomics are ORs into bitmaps and adds into histograms, whose results do not depend on order.
#include "../../include/dfgnn_sample.h"
#include "dfgnn_launch.hpp"

namespace dfgnn {

constexpr int kSampleGroup = 8;      // lanes per row of the kernels that copy a row (d <= fanout)
constexpr int kSampleThreads = 256;  // ... whose workgroups hold 32 rows

__host__ __device__ inline unsigned mix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// a node id clamped into [0, n): an id out of range cannot make a kernel touch anything out of bounds
__host__ __device__ inline int clamp_id(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

struct SeedRow {
  int start, deg;
};
__device__ inline SeedRow seed_row(const int *__restrict__ row_ptr, int node) {
  const int start = row_ptr[node], deg = row_ptr[node + 1] - start;
  return {start, deg < 0 ? 0 : deg};
}

// edges the block's row r keeps: min(d, fanout); r == m: 0 (the prefix sum then ends on nnz_b)
struct RowCount {
  const int *row_ptr, *seeds;
  int n, m, fanout;
  __device__ int operator()(int r) const {
    if (r >= m) return 0;
    const int s = clamp_id(seeds[r], n), d = row_ptr[s + 1] - row_ptr[s];
    return d < 0 ? 0 : (d < fanout ? d : fanout);
  }
};
// nodes of bitmap word w that are reached and no seeds; w == W: 0 (the prefix sum then ends on their total)
struct WordCount {
  const unsigned *seedmask, *marks;
  int W;
  __device__ int operator()(int w) const { return w >= W ? 0 : __popc(marks[w] & ~seedmask[w]); }
};

// out[i] = in(0) + ... + in(i - 1) for i < count: one workgroup, a tile of kScanThreads values per step and a running carry
constexpr int kScanThreads = 1024;
template <class In>
__global__ __launch_bounds__(kScanThreads) void sample_scan_kernel(In in, int count, int *__restrict__ out) {
  __shared__ int wave_sum[kScanThreads / kWave];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  int carry = 0;
  for (long long base = 0; base < count; base += kScanThreads) {
    const long long i = base + tid;
    const int v = i < count ? in((int)i) : 0;
    int incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / kWave; ++w) {
      const int sum = wave_sum[w];
      if (w < wave) before += sum;
      total += sum;
    }
    if (i < count) out[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();  // wave_sum is rewritten by the next tile
  }
}

// ---- select ----------------------------------------------------------------------------------------------------------------
// A lane group per row: registers the seed (bitmap bit, block row) and, for a row that keeps all its edges, marks their columns.
__global__ __launch_bounds__(kSampleThreads) void sample_select_copy_kernel(
    int n, int m, int fanout, const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
    const int *__restrict__ seeds, unsigned *__restrict__ seedmask, unsigned *__restrict__ marks, int *__restrict__ seedpos) {
  const int t = blockIdx.x * kSampleThreads + threadIdx.x;
  const int r = t / kSampleGroup, sub = t % kSampleGroup;
  if (r >= m) return;
  const int s = clamp_id(seeds[r], n);
  const SeedRow row = seed_row(row_ptr, s);
  if (sub == 0) {
    atomicOr(&seedmask[s >> 5], 1u << (s & 31));
    seedpos[s] = r;
  }
  if (row.deg > fanout) return;  // (the wave kernel's)
  for (int i = sub; i < row.deg; i += kSampleGroup) {
    const int c = clamp_id(col_ind[row.start + i], n);
    atomicOr(&marks[c >> 5], 1u << (c & 31));
  }
}

// A wave per row with more than `fanout` edges: the fanout-th smallest key of the row by a radix select, most significant
// byte first.  Pass k counts, among the keys that agree with the bytes found so far, the values of the next byte in a
// 256-bin histogram in LDS; the bin that holds the wanted rank is the next byte.  Keys are recomputed, never stored.  The
// last loop marks the columns of the kept edges, the only reads of col_ind.
__global__ __launch_bounds__(kWave) void sample_select_wave_kernel(
    int n, int fanout, unsigned mseed, const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
    const int *__restrict__ seeds, unsigned *__restrict__ marks, unsigned *__restrict__ thr) {
  __shared__ int hist[256];
  const int r = blockIdx.x, lane = threadIdx.x;
  const SeedRow row = seed_row(row_ptr, clamp_id(seeds[r], n));
  if (row.deg <= fanout) return;  // (uniform over the workgroup)
  unsigned prefix = 0;
  int k = fanout;  // the rank wanted among the keys that carry `prefix`, 1-based
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
#pragma unroll
    for (int j = 0; j < 4; ++j) hist[lane + kWave * j] = 0;
    __syncthreads();
    for (int i = lane; i < row.deg; i += kWave) {
      const unsigned key = mix32((unsigned)(row.start + i) ^ mseed);
      if ((unsigned)((unsigned long long)key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    int c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = hist[4 * lane + j];
      sum += c[j];
    }
    int incl = sum;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int v = __shfl_up(incl, off);
      if (lane >= off) incl += v;
    }
    int acc = incl - sum, bin = 0, rank = 0;
    const bool own = acc < k && k <= incl;  // exactly one lane: the histogram holds at least k keys
    if (own) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // the first bin whose running count reaches k (rank >= 1 once it is found)
        if (rank == 0 && k <= acc + c[j]) {
          bin = 4 * lane + j;
          rank = k - acc;
        }
        acc += c[j];
      }
    }
    const int src = __ffsll((long long)__ballot(own)) - 1;
    bin = __shfl(bin, src);
    k = __shfl(rank, src);
    prefix = (prefix << 8) | (unsigned)bin;
    __syncthreads();  // every lane has read the histogram before the next pass clears it
  }
  if (lane == 0) thr[r] = prefix;
  for (int i = lane; i < row.deg; i += kWave) {
    const int p = row.start + i;
    if (mix32((unsigned)p ^ mseed) <= prefix) {
      const int c = clamp_id(col_ind[p], n);
      atomicOr(&marks[c >> 5], 1u << (c & 31));
    }
  }
}

// the two sizes, and the mixed seed behind the thresholds: emit takes the key function from the workspace
__global__ void sample_counts_kernel(int m, int W, unsigned mseed, const int *__restrict__ blk_row_ptr,
                                     const int *__restrict__ word_rank, int *__restrict__ counts, unsigned *__restrict__ thr) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts[0] = blk_row_ptr[m];
    counts[1] = m + word_rank[W];
    thr[m] = mseed;
  }
}

// ---- emit ------------------------------------------------------------------------------------------------------------------
struct ColMap {
  const unsigned *seedmask, *marks;
  const int *word_rank, *seedpos;
  int n, m, n_cols_b;
  // the block's column id of parent node c (clamped below n_cols_b: whatever the workspace holds, a column id stays in range)
  __device__ int operator()(int c) const {
    c = clamp_id(c, n);
    const unsigned w = (unsigned)c >> 5, bit = 1u << (c & 31), sm = seedmask[w];
    const int id = (sm & bit) ? seedpos[c] : m + word_rank[w] + __popc(marks[w] & ~sm & (bit - 1u));
    return clamp_id(id, n_cols_b);
  }
};

struct EdgeOut {
  int nnz_b;
  int *parent_edge, *blk_col_ind, *rows;
  __device__ void operator()(int slot, int p, int r, int col) const {
    if (slot < 0 || slot >= nnz_b) return;  // (never, for the sizes select reported)
    parent_edge[slot] = p;
    blk_col_ind[slot] = col;
    rows[slot] = r;
  }
};

// rows that keep all their edges: slot = blk_row_ptr[r] + position in the row
__global__ __launch_bounds__(kSampleThreads) void sample_emit_copy_kernel(
    int n, int m, int fanout, const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
    const int *__restrict__ seeds, const int *__restrict__ blk_row_ptr, ColMap cols, EdgeOut out) {
  const int t = blockIdx.x * kSampleThreads + threadIdx.x;
  const int r = t / kSampleGroup, sub = t % kSampleGroup;
  if (r >= m) return;
  const SeedRow row = seed_row(row_ptr, clamp_id(seeds[r], n));
  if (row.deg > fanout) return;
  const int base = blk_row_ptr[r];
  for (int i = sub; i < row.deg; i += kSampleGroup) out(base + i, row.start + i, r, cols(col_ind[row.start + i]));
}

// rows that were sampled: the edges with key <= the row's threshold, compacted 64 at a time in parent order
__global__ __launch_bounds__(kWave) void sample_emit_wave_kernel(
    int n, int m, int fanout, const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
    const int *__restrict__ seeds, const int *__restrict__ blk_row_ptr, const unsigned *__restrict__ thr, ColMap cols,
    EdgeOut out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const unsigned mseed = thr[m];
  const SeedRow row = seed_row(row_ptr, clamp_id(seeds[r], n));
  if (row.deg <= fanout) return;
  const unsigned limit = thr[r];
  const int base = blk_row_ptr[r];
  int done = 0;
  for (int i0 = 0; i0 < row.deg && done < fanout; i0 += kWave) {
    const int i = i0 + lane, p = row.start + i;
    const bool keep = i < row.deg && mix32((unsigned)p ^ mseed) <= limit;
    const unsigned long long kept = __ballot(keep);
    const int at = done + __popcll(kept & ((1ull << lane) - 1ull));
    if (keep && at < fanout) out(base + at, p, r, cols(col_ind[p]));
    done += __popcll(kept);
  }
}

// col_nodes: the seeds, then the set bits of marks & ~seedmask in increasing id (thread w: the bits of word w)
__global__ __launch_bounds__(256) void sample_col_nodes_kernel(int n, int m, int W, int n_cols_b,
                                                               const int *__restrict__ seeds,
                                                               const unsigned *__restrict__ seedmask,
                                                               const unsigned *__restrict__ marks,
                                                               const int *__restrict__ word_rank,
                                                               int *__restrict__ col_nodes) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < m && t < n_cols_b) col_nodes[t] = clamp_id(seeds[t], n);
  if (t >= W) return;
  unsigned bits = marks[t] & ~seedmask[t];
  int at = m + word_rank[t];
  while (bits) {
    if (at >= m && at < n_cols_b) col_nodes[at] = 32 * t + (__ffs((int)bits) - 1);
    ++at;
    bits &= bits - 1u;
  }
}

// ---- workspace -------------------------------------------------------------------------------------------------------------
static inline size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

struct SampleWs {
  unsigned *seedmask, *marks;  // W words each, contiguous: one memset
  int *word_rank;              // W + 1
  int *seedpos;                // n
  unsigned *thr;               // m + 1: per row the largest key kept (sampled rows only), then the mixed seed
  void *sort_temp;
  size_t sort_bytes;
  int *sorted_cols;            // m * fanout
  size_t total;
};

// the layout of dfgnn_sample.h's formula over `base` (may be null: sizes only); m > 0
static void sample_layout(int n, int m, int fanout, void *base, SampleWs &w) {
  const size_t W = ((size_t)n + 31) / 32, E = (size_t)m * (size_t)fanout;
  // rocPRIM's storage for the column sort of E pairs, bounded without asking it (it cannot say without a device): the two
  // alternate buffers (8 E), the decoupled look-back states (one word per digit value and block of >= 1024 items: <= 2 E)
  // and the digit histograms; dfgnn_sample_emit compares what the sort really asks for with this
  w.sort_bytes = 10 * E + 65536;
  char *p = static_cast<char *>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char *at = p ? p + off : nullptr;
    off += a256(bytes);
    return at;
  };
  w.seedmask = reinterpret_cast<unsigned *>(take(8 * W));
  w.marks = w.seedmask ? w.seedmask + W : nullptr;
  w.word_rank = reinterpret_cast<int *>(take(4 * (W + 1)));
  w.seedpos = reinterpret_cast<int *>(take(4 * (size_t)n));
  w.thr = reinterpret_cast<unsigned *>(take(4 * ((size_t)m + 1)));
  w.sort_temp = take(w.sort_bytes);
  w.sorted_cols = reinterpret_cast<int *>(take(4 * E));
  w.total = off;
}

static int check_extents(int n, int m, int fanout) {
  if (n < 0 || m < 0 || fanout < 1) return kErrBadArg;
  if ((long long)m * (long long)fanout >= (1ll << 31) || m == 0x7fffffff) return kErrUnsupported;  // (m + 1 is an int)
  if (m > 0 && n == 0) return kErrBadArg;  // a seed needs a node
  return 0;
}

}  // namespace dfgnn

using namespace dfgnn;

extern "C" {

int dfgnn_sample_abi_version(void) { return DFGNN_SAMPLE_ABI_VERSION; }

int dfgnn_sample_ws_bytes(int n, int m, int fanout, size_t *bytes) {
  if (!bytes) return kErrBadArg;
  if (int rc = check_extents(n, m, fanout)) return rc;
  *bytes = 256;
  if (m == 0) return 0;
  SampleWs w;
  sample_layout(n, m, fanout, nullptr, w);
  *bytes = w.total;
  return 0;
}

int dfgnn_sample_select(int n, int m, int fanout, unsigned seed, const int *row_ptr, const int *col_ind, const int *seeds,
                        int *blk_row_ptr, int *counts, void *ws, size_t ws_bytes, dfgnn_stream_t stream) {
  if (int rc = check_extents(n, m, fanout)) return rc;
  if (!blk_row_ptr || !counts) return kErrBadArg;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (m == 0) {
    if (hipError_t rc = hipMemsetAsync(blk_row_ptr, 0, sizeof(int), s)) return (int)rc;
    return (int)hipMemsetAsync(counts, 0, 2 * sizeof(int), s);
  }
  if (!row_ptr || !seeds || !ws) return kErrBadArg;
  SampleWs w;
  sample_layout(n, m, fanout, ws, w);
  if (ws_bytes < w.total) return kErrBadArg;
  const int W = (n + 31) / 32;
  const unsigned mseed = mix32(seed);
  if (hipError_t rc = hipMemsetAsync(w.seedmask, 0, 8 * (size_t)W, s)) return (int)rc;
  sample_scan_kernel<<<1, kScanThreads, 0, s>>>(RowCount{row_ptr, seeds, n, m, fanout}, m + 1, blk_row_ptr);
  const int groups = (int)(((long long)m * kSampleGroup + kSampleThreads - 1) / kSampleThreads);
  sample_select_copy_kernel<<<groups, kSampleThreads, 0, s>>>(n, m, fanout, row_ptr, col_ind, seeds, w.seedmask, w.marks,
                                                              w.seedpos);
  sample_select_wave_kernel<<<m, kWave, 0, s>>>(n, fanout, mseed, row_ptr, col_ind, seeds, w.marks, w.thr);
  if (int rc = launch_status()) return rc;
  sample_scan_kernel<<<1, kScanThreads, 0, s>>>(WordCount{w.seedmask, w.marks, W}, W + 1, w.word_rank);
  sample_counts_kernel<<<1, 64, 0, s>>>(m, W, mseed, blk_row_ptr, w.word_rank, counts, w.thr);
  return launch_status();
}

int dfgnn_sample_emit(int n, int m, int fanout, int nnz_b, int n_cols_b, const int *row_ptr, const int *col_ind,
                      const int *seeds, const int *blk_row_ptr, int *parent_edge, int *blk_col_ind, int *rows,
                      int *col_nodes, int *col_ptr, int *row_ind, int *val_idx, void *ws, size_t ws_bytes,
                      dfgnn_stream_t stream) {
  if (nnz_b < 0 || n_cols_b < 0) return kErrBadArg;
  if (int rc = check_extents(n, m, fanout)) return rc;
  if ((long long)nnz_b > (long long)m * fanout || n_cols_b < m || (long long)n_cols_b > (long long)m + nnz_b)
    return kErrBadArg;
  const bool want_csc = col_ptr || row_ind || val_idx;
  if (want_csc && !col_ptr) return kErrBadArg;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (m == 0) return want_csc ? (int)hipMemsetAsync(col_ptr, 0, sizeof(int), s) : 0;
  if (!row_ptr || !seeds || !blk_row_ptr || !col_nodes || !ws) return kErrBadArg;
  if (nnz_b > 0 && (!col_ind || !parent_edge || !blk_col_ind || !rows || (want_csc && (!row_ind || !val_idx))))
    return kErrBadArg;
  SampleWs w;
  sample_layout(n, m, fanout, ws, w);
  if (ws_bytes < w.total) return kErrBadArg;
  const int W = (n + 31) / 32;
  const int most = m > W ? m : W;
  sample_col_nodes_kernel<<<(most + 255) / 256, 256, 0, s>>>(n, m, W, n_cols_b, seeds, w.seedmask, w.marks, w.word_rank,
                                                             col_nodes);
  if (nnz_b > 0) {
    const ColMap cols{w.seedmask, w.marks, w.word_rank, w.seedpos, n, m, n_cols_b};
    const EdgeOut out{nnz_b, parent_edge, blk_col_ind, rows};
    const int groups = (int)(((long long)m * kSampleGroup + kSampleThreads - 1) / kSampleThreads);
    sample_emit_copy_kernel<<<groups, kSampleThreads, 0, s>>>(n, m, fanout, row_ptr, col_ind, seeds, blk_row_ptr, cols, out);
    sample_emit_wave_kernel<<<m, kWave, 0, s>>>(n, m, fanout, row_ptr, col_ind, seeds, blk_row_ptr, w.thr, cols, out);
  }
  if (int rc = launch_status()) return rc;
  if (!want_csc) return 0;
  if (nnz_b == 0) return (int)hipMemsetAsync(col_ptr, 0, ((size_t)n_cols_b + 1) * sizeof(int), s);
  size_t need = 0;
  if (csc_sort_temp_bytes(n_cols_b, nnz_b, need)) return kErrUnsupported;
  if (need > w.sort_bytes) return kErrUnsupported;  // (never, by the bound in sample_layout)
  return launch_csc_of_csr(n_cols_b, nnz_b, blk_col_ind, rows, col_ptr, row_ind, val_idx, w.sort_temp, w.sort_bytes,
                           w.sorted_cols, s);
}

}  // extern "C"
