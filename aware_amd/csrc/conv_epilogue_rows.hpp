// Layout algebra of the wide form's row-major epilogue (conv_block.hpp, conv_block_uniform<P, RG, EPI, 4, 4, true>).
//
// After the K loop a wave of the wide form holds a 32 RG x 64 tile in the MFMA accumulator layout: lane (r16 = lane & 15,
// kg = lane >> 4), register (m, n, e)  <->  row 16 m + 4 kg + e, column 16 n + r16.  Global memory wants rows: 16 bytes per
// lane, eight lanes per 128-byte row piece.  The wave turns its tile through a private LDS region of 32 RG rows x 32 floats
// (4 RG KiB: a quarter of the staging memory, which is free by then), one half of the tile (two column tiles, 32 columns) at
// a time.  The data-gradient epilogue takes its `act` operand the other way through the same region.
//
// The region is [row][32 floats] with the column swizzled by the row: at a pitch of 32 floats the four rows 4 kg + e of one
// accumulator store (kg = 0..3, stride 4 rows = 128 floats) fall on the same 16 banks.  XOR-ing bit 4 of the column with bit
// 2 of the row (= bit 0 of kg) sends two of the four to the other 16 columns: 2-way over 64 lanes and 64 banks, and free of
// conflicts on the hardware, which serves 4-byte accesses in halves of 32 lanes.  The swizzle moves whole 64-byte pieces, so a
// lane's four consecutive floats of the row-major side stay consecutive.  No padding: the region has none to give.
//
// Plain functions, host and device: tests/host_sim/conv_epilogue_rows_check.cpp walks them on the CPU.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define AWARE_HD __host__ __device__
#else
#define AWARE_HD
#endif

namespace aware {
namespace epi_rows {

constexpr int kCols = 32;                         // columns of the region = one half of a wave's 64 (two column tiles)
AWARE_HD constexpr int region_floats(int RG) { return 32 * RG * kCols; }
AWARE_HD constexpr int row_passes(int RG) { return 4 * RG; }        // row-major wave instructions per half: 8 rows each

// float index of element (row, col) of the region
AWARE_HD inline int slot(int row, int col) { return row * kCols + (col ^ (((row >> 2) & 1) << 4)); }

// accumulator layout: element of lane's register (m, nl, e), nl = column tile inside the half
AWARE_HD inline int acc_row(int lane, int m, int e) { return 16 * m + 4 * (lane >> 4) + e; }
AWARE_HD inline int acc_col(int lane, int nl) { return 16 * nl + (lane & 15); }
// row-major layout: pass j of a lane covers four consecutive columns of one row
AWARE_HD inline int rm_row(int lane, int j) { return 8 * j + (lane >> 3); }
AWARE_HD inline int rm_col(int lane) { return 4 * (lane & 7); }

// the four maps, as float indices into the wave's region (the row-major ones: the first of four consecutive floats)
AWARE_HD inline int c_write(int lane, int m, int nl, int e) { return slot(acc_row(lane, m, e), acc_col(lane, nl)); }      // ds_write_b32
AWARE_HD inline int c_read(int lane, int j) { return slot(rm_row(lane, j), rm_col(lane)); }                               // ds_read_b128
AWARE_HD inline int act_write(int lane, int j) { return slot(rm_row(lane, j), rm_col(lane)); }                            // ds_write_b128
AWARE_HD inline int act_read(int lane, int m, int nl, int e) { return slot(acc_row(lane, m, e), acc_col(lane, nl)); }     // ds_read_b32

}  // namespace epi_rows
}  // namespace aware
