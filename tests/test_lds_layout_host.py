"""LDS bank model of the one-head GT backward's tile and image accesses (CPU; csrc/dfgnn_lds_layout.hpp).

A small host program (its own main) includes the layout header the kernels use and prints, for the three geometries of
the one-head backward (tile of 128 x 128, 160 x 160 and 96 x 192 values: TS = 136 / 168 / 200; image rows of RS = 144 / 80
fp16), the byte address of every lane for each deterministic access, at the first and last strip / k-block / tile.  A
model of the LDS banks written from the MI355X table -- lane groups and bank count per instruction, identical addresses
broadcast, every further distinct dword on a busy bank of a group costs one more cycle -- counts the LDS cycles of each
wave-instruction and asserts the conflict-free count.  The same model on the formulas of the layout this one replaced
(written out below) gives 4 x for the strips' ds_write_b64, 2 x for their ds_read_b64 and 2 x for the K fragments of the
dQ product: it can see what it is meant to rule out.  The program also checks that no two tile or image elements share a
byte and reports the footprints, which are held against the LDS carve-up of each body."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "df-gnn_amd", "csrc")
LDS_BYTES = 160 * 1024                       # csrc/dfgnn_launch.hpp: kLdsBytes
SLOTS_BYTES = 2 * 8 * 4                      # the two 8-entry workgroup-maximum arrays behind the tile

# (tile rows, tile columns, image rows, image width F): dense_bwd_body<128, 1> at f = 128 and 64, dense_bwd_wide_body<160>,
# dense_bwd_wide2_body (a row block of 96 rows against 192 columns); the wide bodies stage 64 features at a time
GEOMETRIES = ((128, 128, 128, 128), (128, 128, 128, 64), (160, 160, 160, 64), (96, 192, 192, 64))

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "dfgnn_lds_layout.hpp"
using namespace dfgnn;

struct Lane { int mi, mq, tq, tp; };
static Lane lane(int l) { return Lane{l & 15, l >> 4, (l & 15) >> 2, l & 3}; }

template <class Fn>
static void emit(const char *name, const char *instr, int width, int ts, int rs, int a, int b, int c, int d, Fn at) {
  std::printf("A %s %s %d %d %d %d %d %d %d |", name, instr, width, ts, rs, a, b, c, d);
  for (int l = 0; l < 64; ++l) std::printf(" %d", 2 * at(lane(l)));
  std::printf("\n");
}

int main() {
  const int geoms[4][4] = {{128, 128, 128, 128}, {128, 128, 128, 64}, {160, 160, 160, 64}, {96, 192, 192, 64}};
  for (const auto &g : geoms) {
    const int rows = g[0], cols = g[1], irows = g[2], f = g[3];
    const int ts = tile_ts(cols), rs = image_rs(f);
    const int strips[2] = {0, rows / 16 - 1}, tiles[2] = {0, cols / 16 - 1}, kb_rows[2] = {0, rows / 32 - 1};
    const int kb_cols[2] = {0, (cols + 31) / 32 - 1}, fts[2] = {0, f / 16 - 1}, kts[2] = {0, f / 32 - 1};
    const int ikb[2] = {0, irows / 32 - 1}, iu[2] = {0, irows / 16 - 1};
    for (int half = 0; half < 2; ++half) {
      for (int s : strips) {
        for (int u : tiles) {
          // a strip's own values: row 16 s + mi, columns 16 u + 4 mq .. (strip_to_tile, the P read-back)
          auto own = [&](Lane L) { return tile_at(ts, 16 * s + L.mi, 16 * u + 4 * L.mq, half); };
          emit("strip_to_tile", "ds_write_b64", 8, ts, rs, s, u, half, 0, own);
          emit("p_read_back", "ds_read_b64", 8, ts, rs, s, u, half, 0, own);
        }
        for (int jb : kb_cols)
          for (int part = 0; part < 2; ++part)  // natural-order operand of dQ: row 16 s + mi, columns 32 jb + 8 mq + 4 part ..
            emit("tile_row", "ds_read_b64", 8, ts, rs, s, jb, half, part,
                 [&](Lane L) { return tile_at(ts, 16 * s + L.mi, 32 * jb + 8 * L.mq + 4 * part, half); });
      }
      for (int second = 0; second < 2; ++second) {
        for (int ib : kb_rows)
          for (int cs : tiles)  // transposed operand of the column products: rows 32 ib + 4 mq + tq (+ 16), columns 16 cs + 4 tp ..
            emit("tile_tr", "ds_read_b64_tr_b16", 8, ts, rs, ib, cs, half, second,
                 [&](Lane L) { return tile_at(ts, 32 * ib + 4 * L.mq + L.tq + 16 * second, 16 * cs + 4 * L.tp, half); });
        for (int ft : fts) {
          for (int jb : ikb)  // K image fragments of dQ: k-rows 32 jb + 8 mq + tq (+ 4), features 16 ft + 4 tp ..
            emit("image_k", "ds_read_b64_tr_b16", 8, ts, rs, jb, ft, half, second,
                 [&](Lane L) { return image_at(rs, irows, 32 * jb + 8 * L.mq + L.tq + 4 * second, 16 * ft + 4 * L.tp, half, true); });
          for (int ib : ikb)  // image fragments of the column products: rows 32 ib + 4 mq + tq (+ 16)
            emit("image_tr", "ds_read_b64_tr_b16", 8, ts, rs, ib, ft, half, second,
                 [&](Lane L) { return image_at(rs, irows, 32 * ib + 4 * L.mq + L.tq + 16 * second, 16 * ft + 4 * L.tp, half); });
        }
      }
      for (int u : iu)
        for (int t : kts)  // image rows as operands (dP, S, the strips' dO rows): row 16 u + mi, features 32 t + 8 mq ..
          emit("image_row", "ds_read_b128", 16, ts, rs, u, t, half, 0,
               [&](Lane L) { return image_at(rs, irows, 16 * u + L.mi, 32 * t + 8 * L.mq, half); });
    }
    // no two elements share a byte; every element lies inside the footprint; the periods the kernels rely on
    int bad = 0;
    std::vector<char> seen(tile_elems(ts, rows), 0);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c)
        for (int half = 0; half < 2; ++half) {
          const int at = tile_at(ts, r, c, half);
          if (at < 0 || at >= (int)seen.size() || seen[at]++) ++bad;
          if (at != tile_at(ts, r & 15, c & 15, half) + (r & ~15) * 2 * ts + (c & ~15)) ++bad;
          if ((c & 3) == 0 && (at & 3) != 0) ++bad;  // a 4-column chunk stays 8-byte aligned and contiguous
          if ((c & 3) != 0 && at != tile_at(ts, r, c - 1, half) + 1) ++bad;
        }
    for (int kswap = 0; kswap < 2; ++kswap) {
      std::vector<char> iseen(2 * irows * rs, 0);
      for (int r = 0; r < irows; ++r)
        for (int c = 0; c < f; ++c)
          for (int half = 0; half < 2; ++half) {
            const int at = image_at(rs, irows, r, c, half, kswap);
            if (at < 0 || at >= (int)iseen.size() || iseen[at]++) ++bad;
            if (at != image_at(rs, irows, r & 15, c, half, kswap) + (r & ~15) * rs) ++bad;
            if (c > 0 && at != image_at(rs, irows, r, c - 1, half, kswap) + 1) ++bad;
          }
    }
    std::printf("C %d %d %d %d bad %d tile_bytes %d image_bytes %d\n", rows, cols, irows, f, bad, 2 * tile_elems(ts, rows),
                2 * 2 * irows * rs);
  }
  return 0;
}
"""

# lane groups that are served in one LDS cycle each, and the number of banks, per instruction (MI355X LDS table)
_B128 = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])
RULES = {
    "ds_write_b64": ([list(range(16 * k, 16 * k + 16)) for k in range(4)], 32),
    "ds_read_b64": ([list(range(32 * k, 32 * k + 32)) for k in range(2)], 64),
    "ds_read_b64_tr_b16": ([list(range(32 * k, 32 * k + 32)) for k in range(2)], 64),
    "ds_read_b128": ([g for k in range(2) for g in ([x + 32 * k for x in _B128[0]], [x + 32 * k for x in _B128[1]])], 64),
}


def lds_cycles(instr, width, addrs):
    """LDS-array cycles of one wave-instruction: per lane group, the largest number of distinct dwords on one bank."""
    groups, banks = RULES[instr]
    assert len(addrs) == 64 and all(a % width == 0 for a in addrs), "natural alignment of every lane's access"
    total = 0
    for lanes in groups:
        dwords = {a // 4 + k for a in (addrs[l] for l in lanes) for k in range(width // 4)}   # identical addresses broadcast
        per_bank = {}
        for d in dwords:
            per_bank[d % banks] = per_bank.get(d % banks, 0) + 1
        total += max(per_bank.values())
    return total


def clean_cycles(instr):
    return len(RULES[instr][0])


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("lds_layout")
    src, exe = d / "lds_layout_host.cpp", d / "lds_layout_host"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    accesses, checks = [], []
    for line in lines:
        if line.startswith("A "):
            head, addrs = line[2:].split("|")
            name, instr, *nums = head.split()
            accesses.append((name, instr, tuple(int(x) for x in nums), [int(x) for x in addrs.split()]))
        elif line.startswith("C "):
            checks.append(line.split())
    return accesses, checks


def test_every_deterministic_access_is_conflict_free(report):
    accesses, _ = report
    names = {a[0] for a in accesses}
    assert names == {"strip_to_tile", "p_read_back", "tile_row", "tile_tr", "image_k", "image_tr", "image_row"}
    geoms = {(a[2][1], a[2][2]) for a in accesses}
    assert geoms == {(136, 144), (136, 80), (168, 80), (200, 80)}
    worst = {}
    for name, instr, nums, addrs in accesses:
        cyc = lds_cycles(instr, nums[0], addrs)
        worst[(name, instr)] = max(worst.get((name, instr), 0), cyc)
        assert cyc == clean_cycles(instr), (name, instr, nums, cyc)
    for (name, instr), cyc in sorted(worst.items()):
        print(f"lds-layout {name} {instr}: {cyc} cycles per wave-instruction (conflict-free {clean_cycles(instr)})")


def _lanes():
    return [(l & 15, l >> 4, (l & 15) >> 2, l & 3) for l in range(64)]


@pytest.mark.parametrize("ts,rs", ((136, 144), (136, 80), (168, 80), (200, 80)))
def test_the_model_sees_the_conflicts_of_the_previous_layout(ts, rs):
    """The layout before: tile element (row, column, half) at row 2 TS + half TS + column, K image row r at r RS."""
    tb = 2 * ts
    for s in (0, 5):
        for u in (0, 7):
            for half in (0, 1):
                own = [2 * ((16 * s + mi) * tb + half * ts + 16 * u + 4 * mq) for mi, mq, _, _ in _lanes()]
                assert lds_cycles("ds_write_b64", 8, own) == 4 * clean_cycles("ds_write_b64") == 16
                assert lds_cycles("ds_read_b64", 8, own) == 2 * clean_cycles("ds_read_b64") == 4
    for jb in (0, 3):
        for ft in (0, rs // 16 - 2):
            for second in (0, 1):
                k = [2 * ((32 * jb + 8 * mq + tq + 4 * second) * rs + 4 * tp + 16 * ft) for _, mq, tq, tp in _lanes()]
                assert lds_cycles("ds_read_b64_tr_b16", 8, k) == 2 * clean_cycles("ds_read_b64_tr_b16") == 4
    # ... and what was clean then is clean in the model: the transposed tile reads, the 16-byte natural-order reads of dQ
    for ib in (0, 2):
        for second in (0, 1):
            tr = [2 * ((32 * ib + 4 * mq + tq + 16 * second) * tb + 16 + 4 * tp) for _, mq, tq, tp in _lanes()]
            assert lds_cycles("ds_read_b64_tr_b16", 8, tr) == 2
    nat = [2 * (mi * tb + 8 * mq + 32) for mi, mq, _, _ in _lanes()]
    assert lds_cycles("ds_read_b128", 16, nat) == 4


def test_elements_are_distinct_and_the_footprint_fits(report):
    _, checks = report
    assert len(checks) == len(GEOMETRIES)
    for c, (rows, cols, irows, f) in zip(checks, GEOMETRIES):
        assert tuple(int(x) for x in c[1:5]) == (rows, cols, irows, f)
        bad, tile_bytes, image_bytes = int(c[6]), int(c[8]), int(c[10])
        assert bad == 0, c
        assert tile_bytes == rows * (cols + 8) * 4 and image_bytes == 2 * irows * (f + 16) * 2    # the same bytes as before
        assert image_bytes + tile_bytes + SLOTS_BYTES <= LDS_BYTES, c
    # the general body's other geometries (same tile formulas): 160 columns in row blocks of 80 (padded to 96) rows at
    # f = 128, and two column blocks of 128 -- images first, then the tile, then the slots
    assert 2 * 160 * 144 * 2 + 96 * 168 * 4 + SLOTS_BYTES <= LDS_BYTES
    assert 2 * 128 * 144 * 2 + 128 * 136 * 4 + SLOTS_BYTES <= LDS_BYTES
