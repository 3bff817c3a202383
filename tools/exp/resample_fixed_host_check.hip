// Stand-alone host check of the fixed-ratio resampler's host code, for a sanitizer build on the CPU (no GPU is touched):
// the table builder, par_resample_fixed_out_len and every argument check of par_resample_fixed_f32 that returns before the
// first device call.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/exp/resample_fixed_host_check.hip pyaudiorestoration_amd/csrc/resample_fixed.hip \
//         pyaudiorestoration_amd/csrc/common.hip -o /tmp/resample_fixed_host_check && /tmp/resample_fixed_host_check
//
// Prints "ok" and exits 0, or names the first check that failed.  With --dump FILE it also writes the Z = 8 table as raw
// float32 pairs (win, delta) for a comparison with tests/fixed_rate_np.table.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/par_hip.h"
#include "../../pyaudiorestoration_amd/csrc/resample_fixed.h"

#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      printf("FAILED line %d: %s\n", __LINE__, #c);          \
      return 1;                                              \
    }                                                        \
  } while (0)

int main(int argc, char** argv) {
  for (int Z : {1, 3, 8, 64}) {
    std::vector<float2> nat;
    std::vector<float> phase;
    par::rs_build_table(Z, &nat, &phase);
    const size_t N = (size_t)par::kRsP * Z;
    CHECK(nat.size() == N + 1);
    CHECK(nat[0].x == (float)par::kRsRolloff);
    CHECK(fabsf(nat[N].x) < 1e-12f && nat[N].y == 0.0f);
    double sum = 0.0;
    for (size_t j = 0; j < N; ++j) {
      CHECK(fabs((double)nat[j].y - ((double)nat[j + 1].x - (double)nat[j].x)) < 2e-7);
      sum += nat[j].y;
    }
    CHECK(fabs(sum + par::kRsRolloff) < 1e-4);           // the deltas walk win from rolloff down to 0
    CHECK(phase.size() == (size_t)(par::kRsP + 1) * 20);
    if (Z == 8) {
      for (int off = 0; off <= par::kRsP; ++off)
        for (int i = 0; i < 8; ++i) {
          const size_t j = (size_t)off + (size_t)i * par::kRsP;
          const float w = phase[(size_t)off * 20 + 2 * i], d = phase[(size_t)off * 20 + 2 * i + 1];
          if (j <= N) CHECK(w == nat[j].x && d == nat[j].y);
          else CHECK(w == 0.0f && d == 0.0f);
        }
      for (int off = 0; off <= par::kRsP; ++off)
        for (int k = 16; k < 20; ++k) CHECK(phase[(size_t)off * 20 + k] == 0.0f);
      if (argc == 3 && !strcmp(argv[1], "--dump")) {
        FILE* f = fopen(argv[2], "wb");
        CHECK(f);
        CHECK(fwrite(nat.data(), sizeof(float2), nat.size(), f) == nat.size());
        fclose(f);
      }
    }
  }
  std::vector<float2> only_nat;
  par::rs_build_table(2, &only_nat, nullptr);
  CHECK(only_nat.size() == 1025);

  CHECK(par_resample_fixed_out_len(700, 48000.0, 44100.0) == 643);
  CHECK(par_resample_fixed_out_len(700, 44100.0, 48000.0) == 761);
  CHECK(par_resample_fixed_out_len(0, 44100.0, 48000.0) == 0);
  CHECK(par_resample_fixed_out_len(700000000, 44100.0, 48000.0) == (int64_t)(700000000.0 * 48000.0 / 44100.0));
  CHECK(par_resample_fixed_out_len(-1, 1.0, 1.0) == -1);
  CHECK(par_resample_fixed_out_len(5, 0.0, 1.0) == -1 && par_resample_fixed_out_len(5, 1.0, NAN) == -1);
  CHECK(par_resample_fixed_out_len(5, INFINITY, 1.0) == -1 && par_resample_fixed_out_len(INT64_MAX, 1.0, 16.0) == -1);

  float xs[8] = {0}, ys[8] = {0};
  char msg[256];
  CHECK(par_resample_fixed_f32(0, nullptr, 8, 1, 1.0, 1.0, 8, ys, 8, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 1, 1.0, 1.0, 8, nullptr, 8, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 1, 0.0, 1.0, 8, ys, 8, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 1, 1.0, NAN, 8, ys, 8, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 1, 1.0, -INFINITY, 8, ys, 8, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 1, 1.0, 1.0, 0, ys, 8, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 1, 1.0, 1.0, 65, ys, 8, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 0, 1.0, 1.0, 8, ys, 8, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 1, 1.0, 1.0, 8, ys, 8, -1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 1, 1.0, 1.0, 8, ys, 9, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_last_error(msg, sizeof(msg)) == PAR_OK && strstr(msg, "n_out"));
  CHECK(par_resample_fixed_f32(0, xs, -8, 1, 1.0, 1.0, 8, ys, 0, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(0, xs, 8, 1, 1.0, 1.0, 8, xs, 8, 1, nullptr) == PAR_ERR_ARG);
  CHECK(par_resample_fixed_f32(99, xs, 0, 1, 1.0, 1.0, 8, ys, 0, 1, nullptr) == PAR_OK);
  CHECK(par_resample_fixed_f32(99, xs, 3, 1, 48000.0, 8000.0, 8, ys, 0, 1, nullptr) == PAR_OK);
  CHECK(par_resample_fixed_f32(99, xs, 8, 1, 1.0, 17.0, 8, ys, 136, 1, nullptr) == PAR_ERR_UNSUPPORTED);
  CHECK(par_resample_fixed_f32(99, xs, 170, 1, 17.0, 1.0, 8, ys, 10, 1, nullptr) == PAR_ERR_UNSUPPORTED);
  CHECK(par_last_error(msg, sizeof(msg)) == PAR_OK && strstr(msg, "ratio"));
  printf("ok\n");
  return 0;
}
