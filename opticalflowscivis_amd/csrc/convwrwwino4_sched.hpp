// convwrwwino4_sched.hpp -- the STEP SCHEDULE of conv3d_wrw_wino4_kernel (convwrwwino4.hpp, round 12): plain C++
// constexpr functions, included by the kernel and by tests/tools/wrw_wino4_sched_check.cpp, which simulates both roles of
// every run on the host.  A hang (the roles disagreeing on the barrier count) or a stale source row would come from here.
//
// A STEP is one gradient row: (sample b, plane z, x-brick xb, row y), y fastest -- global step q = ((b D + z) BXN + xb) H + y.
// With one x-brick per row (W = 64) this is the order of the two-row bricks the grid is cut in; with two, a run walks down
// an x-column before it moves to the next, so that consecutive steps share two source rows in either case.  Run `bx` of
// the grid owns the steps [2 spw bx, min(2 spw (bx + 1), 2 bricks)): N of them, local step n = 0 .. N - 1.
//
// Source rows.  Local ROW s = 0 .. N + 1 is the source row at the centre of global step q0 + s - 1 (same b, xb, y; plane
// z + kz - 1), so step n multiplies its gradient row with rows n, n + 1, n + 2 for ky = 0, 1, 2 -- where those are rows
// of ITS x-column: for y + ky - 1 outside [0, H) the operand is the padding row, which is no ring row at all but the
// permanently zero slot W4S_ZERO.  Rows 0 and N + 1 belong to the neighbouring runs' steps (or to no step: then they are
// staged as zeros and never read).  A row of a plane outside [0, D) is staged as zeros and transformed like any other.
//
// Pipeline, one barrier at the end of every step, W4S_PRO virtual steps n = -4 .. -1 in front (loaders only):
//   step n, loaders:       LDS-DMA of raw row n + 4 into raw buffer (n + 4) % 2 and of gradient row n + 1 into gradient
//                          buffer (n + 1) % 2; transform + split of raw row n + 3 into ring slot (n + 3) % 4
//   step n, matrix waves:  gradient row n; ring slots n % 4, (n + 1) % 4, (n + 2) % 4 (or W4S_ZERO)
// Slot (n + 3) % 4 held row n - 1, last read in step n - 1; raw buffer (n + 4) % 2 held row n + 2, transformed in step
// n - 1; gradient buffer (n + 1) % 2 held row n - 1.
#pragma once

constexpr int W4S_RING = 4;  // ring slots that carry rows; slot W4S_ZERO is all-zero pieces, written once
constexpr int W4S_ZERO = 4;
constexpr int W4S_PRO = 4;   // virtual steps (barriers) in front of step 0

struct W4SRow { int b, z, xb, y; };  // of a global step: its gradient row, and the centre (ky = 1) source row of plane z + kz - 1

// global step q -> position (q = -1 gives y = -1 of the first column, q = total gives b = B: both are `!w4s_live`)
constexpr W4SRow w4s_row(long long q, int D, int H, int bxn) {
  if (q < 0) return {0, 0, 0, (int)q};
  const int y = (int)(q % H); q /= H;
  const int xb = (int)(q % bxn); q /= bxn;
  const int z = (int)(q % D);
  return {(int)(q / D), z, xb, y};
}
constexpr W4SRow w4s_next(W4SRow r, int D, int H, int bxn) {
  if (++r.y == H) { r.y = 0; if (++r.xb == bxn) { r.xb = 0; if (++r.z == D) { r.z = 0; ++r.b; } } }
  return r;
}
constexpr bool w4s_live(const W4SRow& r, int B) { return r.y >= 0 && r.b < B; }

// steps and barriers of a run of `bricks_in_run` two-row bricks (both roles execute exactly w4s_barriers of them before
// the loaders leave)
constexpr long long w4s_steps(long long bricks_in_run) { return 2 * bricks_in_run; }
constexpr long long w4s_barriers(long long N) { return N + W4S_PRO; }

// what the loaders do during step n (-W4S_PRO <= n < N)
struct W4SFill {
  bool src; long long src_row; int src_buf;     // LDS-DMA: raw source row src_row -> raw buffer src_buf
  bool grad; long long grad_step; int grad_buf; // LDS-DMA: gradient row of local step grad_step -> gradient buffer grad_buf
  bool tf; long long tf_row; int tf_buf, tf_slot;  // transform + split: raw buffer tf_buf (row tf_row) -> ring slot tf_slot
};
constexpr W4SFill w4s_fill(long long n, long long N) {
  const long long s = n + 4, g = n + 1, t = n + 3;
  return {s >= 0 && s <= N + 1, s, (int)(s & 1), g >= 0 && g < N, g, (int)(g & 1), t >= 0 && t <= N + 1, t, (int)(t & 1),
          (int)(t & 3)};
}

// what the matrix waves read during step n (0 <= n < N), whose gradient row is row y of its plane
constexpr int w4s_grad_buf(long long n) { return (int)(n & 1); }
constexpr int w4s_read_slot(long long n, int ky, int y, int H) {
  const int sy = y + ky - 1;
  return sy >= 0 && sy < H ? (int)((n + ky) & 3) : W4S_ZERO;
}
constexpr long long w4s_read_row(long long n, int ky) { return n + ky; }  // the local row that slot must hold
