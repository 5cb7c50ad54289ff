// Host program of tests/test_tr_p8_s3_build.py: the words of the split FS_WPREP_P8 table (csrc/wprep.hpp) for a small
// layer, computed on the CPU by the library's own element function.  Weights: element i of w[ci][co][tap] is
// 1 + i / 2^12 + (i % 7) / 2^20 + 2^-23 -- exact in fp32; the last bit keeps the second and third bf16 pieces non-zero.
//   p8s_words CIN COUT RT  ->  one line "index word" per table word
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>

#include "flowsci_hip.h"

namespace {
#include "wprep.hpp"
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int cin = atoi(argv[1]), cout = atoi(argv[2]), rt = atoi(argv[3]);
  const int cinp = (cin + 3) / 4 * 4;
  std::vector<float> w((size_t)cin * cout * 64);
  for (size_t i = 0; i < w.size(); ++i) w[i] = 1.f + (float)i / 4096.f + (float)(i % 7) / 1048576.f + 1.f / 8388608.f;
  const int total = cinp / 4 * rt * 768;
  FsWprepJob j = wprep_job(FS_WPREP_P8, w.data(), nullptr, total, cin, cout, cinp, rt, 1);
  for (int e = 0; e < total; ++e) printf("%d %08x\n", e, wprep_p8s_word(j, e));
  return 0;
}
