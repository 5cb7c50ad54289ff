// Host model of conv3d_wrw_wino4_kernel's step schedule (csrc/convwrwwino4_sched.hpp): for every run of every geometry
// below and every kz it plays the loader waves and the matrix waves window by window (a window = what lies between two
// barriers) and checks that
//   1. the three ring slots a step reads hold exactly the source rows (b, z + kz - 1, y - 1 .. y + 1, x-brick) it needs --
//      all-zero pieces for a plane outside the volume, the zero slot for a row outside the plane -- and the gradient
//      buffer the step's own row; LDS starts as garbage in every workgroup, so nothing may be inherited;
//   2. nothing is written in a window in which the matrix waves may still read it.  The matrix waves' barrier sits INSIDE
//      their step: in the window of loader step n they run the head of step n (every read) and the tail of step n - 1
//      (the ky = 1, 2 slots again, and the gradient row of step n for its first component);
//   3. both roles count the same number of barriers, w4s_barriers(N);
// and that the runs' steps cover every gradient row exactly once.  Built with a host compiler and run directly
// (tests/test_wrw_wino4_sched.py); exit status 0 and "OK" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "convwrwwino4_sched.hpp"

namespace {

struct Content {  // what an LDS row holds
  enum Kind { GARBAGE, ZERO, ROW } kind = GARBAGE;
  int b = 0, z = 0, y = 0, xb = 0;  // ROW: source row (b, plane z, row y, x-brick xb)
  long long local = -1;             // the run's local row number (raw buffers, ring slots) or step (gradient buffers)
};

int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                           \
  } while (0)

struct Geo { const char* name; int B, D, H, W; };

void run_check(const Geo& g, int kz, long long q0, long long N, std::vector<int>& covered, const char* tag) {
  const int bxn = g.W / 64;
  Content ring[W4S_RING + 1], raw[2], grad[2];
  ring[W4S_ZERO].kind = Content::ZERO;  // written once by the loaders in front of the first barrier
  W4SRow rs = w4s_row(q0 - 1, g.D, g.H, bxn), rg = w4s_row(q0, g.D, g.H, bxn);
  long long src_fills = 0, grad_fills = 0, loader_barriers = 0, matrix_barriers = 0;

  // the reads of step n that fall into a window: head = all of them, tail = what may follow the step's own barrier
  auto check_reads = [&](long long n, bool tail, const W4SFill* f) {
    const W4SRow st = w4s_row(q0 + n, g.D, g.H, bxn);
    for (int ky = tail ? 1 : 0; ky < 3; ++ky) {
      const int slot = w4s_read_slot(n, ky, st.y, g.H);
      CHECK(slot >= 0 && slot <= W4S_ZERO, "%s: slot %d", tag, slot);
      if (f && f->tf) CHECK(f->tf_slot != slot, "%s: step %lld ky %d reads slot %d while it is written", tag, n, ky, slot);
      const int sy = st.y + ky - 1, sz = st.z + kz - 1;
      const Content& c = ring[slot];
      if (sy < 0 || sy >= g.H) {
        CHECK(slot == W4S_ZERO && c.kind == Content::ZERO, "%s: step %lld ky %d: padding row not the zero slot", tag, n, ky);
      } else {
        CHECK(slot != W4S_ZERO && c.local == w4s_read_row(n, ky), "%s: step %lld ky %d: slot %d holds local row %lld", tag, n, ky, slot, c.local);
        if (sz < 0 || sz >= g.D) CHECK(c.kind == Content::ZERO, "%s: step %lld ky %d: padding plane not zero", tag, n, ky);
        else CHECK(c.kind == Content::ROW && c.b == st.b && c.z == sz && c.y == sy && c.xb == st.xb,
                   "%s: step %lld ky %d: slot %d holds (%d %d %d %d), kind %d", tag, n, ky, slot, c.b, c.z, c.y, c.xb, (int)c.kind);
      }
    }
  };
  auto check_grad = [&](long long n, const W4SFill* f) {  // the matrix waves read step n's gradient row in this window
    const int buf = w4s_grad_buf(n);
    if (f && f->grad) CHECK(f->grad_buf != buf, "%s: gradient buffer %d of step %lld is written while read", tag, buf, n);
    CHECK(grad[buf].kind == Content::ROW && grad[buf].local == n, "%s: gradient buffer %d holds step %lld, not %lld", tag, buf, grad[buf].local, n);
  };

  for (long long n = -W4S_PRO; n < N; ++n) {
    const W4SFill f = w4s_fill(n, N);
    // ---- matrix waves in this window (the state is that of the window's start: the loaders' writes of the window land
    // at its barrier, and check 2 forbids them to touch what is read)
    if (n >= 0) { check_reads(n, false, &f); check_grad(n, &f); }
    if (n >= 1) check_reads(n - 1, true, &f);
    ++matrix_barriers;  // (the virtual steps n < 0: barriers only)
    // ---- loader waves, step n
    Content nraw, ngrad, nring;
    if (f.src) {
      CHECK(f.src_row == src_fills, "%s: source rows staged out of order", tag);
      CHECK(!(f.tf && f.tf_buf == f.src_buf), "%s: raw buffer %d staged while it is transformed", tag, f.src_buf);
      const W4SRow want = w4s_row(q0 - 1 + f.src_row, g.D, g.H, bxn);
      if (w4s_live(rs, g.B)) CHECK(rs.b == want.b && rs.z == want.z && rs.y == want.y && rs.xb == want.xb, "%s: row walk", tag);
      const int sz = rs.z + kz - 1;
      const bool ok = w4s_live(rs, g.B) && sz >= 0 && sz < g.D;
      nraw.kind = ok ? Content::ROW : Content::ZERO;
      nraw.b = rs.b; nraw.z = sz; nraw.y = rs.y; nraw.xb = rs.xb; nraw.local = f.src_row;
      rs = w4s_next(rs, g.D, g.H, bxn);
      ++src_fills;
    }
    if (f.grad) {
      CHECK(f.grad_step == grad_fills, "%s: gradient rows staged out of order", tag);
      CHECK(w4s_live(rg, g.B), "%s: gradient row outside the volume", tag);
      const long long q = (((long long)rg.b * g.D + rg.z) * bxn + rg.xb) * g.H + rg.y;
      CHECK(q == q0 + f.grad_step, "%s: gradient row walk", tag);
      if (q >= 0 && q < (long long)covered.size()) ++covered[q];
      ngrad.kind = Content::ROW; ngrad.local = f.grad_step;
      rg = w4s_next(rg, g.D, g.H, bxn);
      ++grad_fills;
    }
    if (f.tf) {
      CHECK(f.tf_slot >= 0 && f.tf_slot < W4S_RING, "%s: transform into slot %d", tag, f.tf_slot);
      CHECK(raw[f.tf_buf].kind != Content::GARBAGE && raw[f.tf_buf].local == f.tf_row, "%s: raw buffer %d holds row %lld, not %lld", tag,
            f.tf_buf, raw[f.tf_buf].local, f.tf_row);
      nring = raw[f.tf_buf];
    }
    if (f.src) raw[f.src_buf] = nraw;
    if (f.grad) grad[f.grad_buf] = ngrad;
    if (f.tf) ring[f.tf_slot] = nring;
    ++loader_barriers;
  }
  if (N > 0) check_reads(N - 1, true, nullptr);  // the tail of the last step, behind the last barrier
  CHECK(grad_fills == N, "%s: %lld gradient rows for %lld steps", tag, grad_fills, N);
  CHECK(src_fills == N + 2, "%s: %lld source rows for %lld steps", tag, src_fills, N);
  CHECK(loader_barriers == w4s_barriers(N) && matrix_barriers == w4s_barriers(N), "%s: barriers %lld / %lld, want %lld", tag,
        loader_barriers, matrix_barriers, w4s_barriers(N));
}

void geometry(const Geo& g, bool one_brick_runs) {
  const long long bricks = (long long)g.B * g.D * (g.H / 2) * (g.W / 64);
  const long long spw = one_brick_runs ? 1 : (bricks + 41) / 42;  // launch_wrw_wino4
  const long long gx = (bricks + spw - 1) / spw;
  for (int kz = 0; kz < 3; ++kz) {  // (the channel half changes addresses only: both halves of a kz are one case)
    std::vector<int> covered(2 * bricks, 0);
    for (long long bx = 0; bx < gx; ++bx) {
      const long long s0 = bx * spw, s1 = s0 + spw < bricks ? s0 + spw : bricks;
      char tag[128];
      std::snprintf(tag, sizeof tag, "%s spw=%lld kz=%d run=%lld", g.name, spw, kz, bx);
      run_check(g, kz, 2 * s0, w4s_steps(s1 - s0), covered, tag);
    }
    for (size_t q = 0; q < covered.size(); ++q) CHECK(covered[q] == 1, "%s kz=%d: gradient row %zu staged %d times", g.name, kz, q, covered[q]);
  }
  std::printf("%-6s B=%d (%d, %d, %d) spw=%lld runs=%lld\n", g.name, g.B, g.D, g.H, g.W, spw, gx);
}

}  // namespace

int main() {
  const Geo geos[] = {{"a", 1, 16, 128, 64}, {"b", 2, 33, 32, 64},  {"c", 1, 16, 64, 128}, {"d", 1, 512, 4, 64},
                      {"e", 1, 1024, 2, 64}, {"f", 8, 4, 64, 64},   {"g", 1, 64, 16, 128}, {"bench", 2, 64, 64, 64}};
  for (const Geo& g : geos) {
    geometry(g, false);
    geometry(g, true);
  }
  {  // an empty run: both roles still agree
    std::vector<int> none;
    run_check(geos[0], 1, 0, 0, none, "empty run");
  }
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("OK\n");
  return 0;
}
