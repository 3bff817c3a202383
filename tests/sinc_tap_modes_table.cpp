// Driver of tests/test_sinc_tap_modes_cpu.py: prints what csrc/sinc_tap_modes.h answers for the NT values read from stdin,
// one line "p1_from p0_from" per value.
#include <stdio.h>
#include <vector>
#include "sinc_tap_modes.h"

int main() {
  int NT;
  while (scanf("%d", &NT) == 1) {
    if (NT < 1) return 2;
    par::TapModes tm{0, 0};
    std::vector<double> lin_a, lin_b, cst;
    par::choose_tap_modes(NT, &tm, &lin_a, &lin_b, &cst);
    printf("%d %d\n", tm.p1_from, tm.p0_from);
  }
  return 0;
}
