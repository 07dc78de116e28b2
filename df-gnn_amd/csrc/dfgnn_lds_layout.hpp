// dfgnn_lds_layout.hpp -- where the elements of the backward's P / dS tile and of a feature image live in LDS.
//
// Plain constexpr functions (no HIP types), so that the kernels and a host program see the same formulas:
// tests/test_lds_layout_host.py compiles this header on the CPU, prints the byte address of every lane for each access
// pattern of the one-head backward and runs them through a model of the LDS banks.  All offsets are in fp16 elements.
//
// LDS banking (MI355X): a wave's access is served in fixed lane groups, one cycle per group unless two lanes of a group
// want different dwords of one bank.  ds_write_b64: 4 groups of 16 contiguous lanes, 32 banks; ds_read_b64 and
// ds_read_b64_tr_b16: 2 groups of 32 lanes, 64 banks; ds_read_b128: 4 groups of 16 lanes, 64 banks.
//
// The tile.  Row r holds 2 TS fp16: the hi halves of its columns at +0, the lo halves at +TS (TS = columns + 8, so a
// row is TS dwords = 8 mod 32).  Every vector access moves whole 4-column chunks (8 bytes).  With the chunks in natural
// order, rows 4 apart lie 32 dwords apart: the 16 rows a strip writes with one ds_write_b64 share banks four ways, and
// the rows r, r + 8 of a strip's ds_read_b64 two ways.  So the chunk index is XORed with a function g of (r >> 2) & 3
// that touches its two low bits only -- a row's chunks stay inside their aligned group of four (32 bytes), which is all
// the transposed reads of the column products need (8 consecutive rows x 4 chunks = 64 distinct banks either way):
//   * one ds_write_b64 / 16 rows r0 .. r0 + 15, one chunk:   rows r, r + 4, r + 8, r + 12 need four different g
//   * one ds_read_b64 / 16 rows x chunks {c, c + 1}:          g(s) ^ g(s + 2) must not be 0 or 1
//   * one ds_read_b64 / 16 rows x chunks {c, c + 2}:          g(s) ^ g(s + 2) must not be 0 or 2
// hence g(s + 2) = g(s) ^ 3 and g one-to-one: g = 0, 1, 3, 2 (the Gray code of s).  A 16-byte read of 8 consecutive
// columns cannot be kept (its two chunks may land in either order), so the natural-order reads of dQ are two 8-byte
// reads of one chunk each.
//
// The K image of the dQ product.  An image row is RS = F + 16 fp16 (RS / 2 dwords = 8 mod 64 for F = 128, 40 for F = 64).
// The product reads k-rows 32 jb + 8 mq + tq (and + 4) through ds_read_b64_tr_b16: the rows of mq and mq + 1 are 8 apart,
// i.e. 64 banks, and collide two ways.  That image alone is therefore stored with the two 4-row halves of every odd
// group of 8 rows exchanged (row r at r ^ 4 when r & 8), which moves them 32 banks apart; the k-slot a row is
// multiplied in does not change.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DFGNN_LAYOUT_FN __host__ __device__ constexpr
#else
#define DFGNN_LAYOUT_FN constexpr
#endif

namespace dfgnn {

// ---- tile ---------------------------------------------------------------------------------------------------------
DFGNN_LAYOUT_FN int tile_ts(int columns) { return columns + 8; }           // TS: floats (= fp16 pairs) per tile row
DFGNN_LAYOUT_FN int tile_elems(int ts, int rows) { return rows * 2 * ts; }  // fp16 footprint of `rows` rows
// what a row XORs onto its column index: 4 g((row >> 2) & 3), g = 0, 1, 3, 2
DFGNN_LAYOUT_FN int tile_swizzle(int row) { return (row & 12) ^ ((row >> 1) & 4); }
// element (row, column, half): half 0 = hi, 1 = lo.  Periodic in 16 rows and in 16 columns:
//   tile_at(ts, row + 16 a, col + 16 b, half) = tile_at(ts, row, col, half) + 16 a 2 ts + 16 b
// so the kernels take the offset of (row & 15, col & 15) once per lane and add the strip / tile steps as constants.
DFGNN_LAYOUT_FN int tile_at(int ts, int row, int col, int half) { return row * 2 * ts + (col ^ tile_swizzle(row)) + half * ts; }

// ---- feature image ------------------------------------------------------------------------------------------------
DFGNN_LAYOUT_FN int image_rs(int f) { return f + 16; }                     // RS: fp16 per image row
// the row of the image that matrix row `row` is stored in; kswap: the K image of the dQ product (see above)
DFGNN_LAYOUT_FN int image_row(int row, bool kswap) { return kswap ? row ^ ((row >> 1) & 4) : row; }
// element (row, feature, half) of an image of `rows` rows: the lo plane follows the hi plane.  Periodic in 16 rows.
DFGNN_LAYOUT_FN int image_at(int rs, int rows, int row, int feat, int half, bool kswap = false) {
  return half * rows * rs + image_row(row, kswap) * rs + feat;
}

static_assert(tile_at(136, 16 + 5, 32 + 12, 1) == tile_at(136, 5, 12, 1) + 16 * 272 + 32, "tile_at is periodic");
static_assert(image_at(144, 128, 32 + 9, 20, 0, true) == image_at(144, 128, 9, 20, 0, true) + 32 * 144, "image_at is periodic");

}  // namespace dfgnn
