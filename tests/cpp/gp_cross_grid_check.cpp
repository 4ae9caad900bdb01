// Host check of cross_grid (math_amd/csrc/gp_family.h), the grid that the
// rectangular GP walks of gp.hip and gp_ard.hip's cross reverse share: prints
// "n1 n2 rows gx gy" for each (n1, n2, rows) triple of its arguments.
// Built (host code only) and run by tests/test_gp_cross_grid.py; links nothing
// of the library and needs no GPU.
#include "../../math_amd/csrc/gp_family.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  for (int a = 1; a + 2 < argc; a += 3) {
    const int n1 = std::atoi(argv[a]), n2 = std::atoi(argv[a + 1]), rows = std::atoi(argv[a + 2]);
    const dim3 g = cross_grid(n1, n2, rows);
    std::printf("%d %d %d %u %u\n", n1, n2, rows, g.x, g.y);
  }
  return 0;
}
