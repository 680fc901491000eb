// Prints the tile-config table as the preprocessor sees it: one line
// "id family bm bn" per config found by tile_config(id), over a range of ids
// well past both ends of the table (tests/test_tile_table.py builds this under
// ASan + UBSan and compares the lines with what the Python reader parsed).
#include <cstdio>

#include "tile_configs.h"

int main() {
  static const char* const kNames[] = {"igemm", "cgemm", "cgemm_pf", "cgemm32", "bgemm", "halo", "halo_pf",
                                       "halo_persist"};
  for (int id = -64; id <= 320; ++id) {
    const tfsk::TileConfig* c = tfsk::tile_config(id);
    if (c == nullptr) continue;
    if (c->id != id) return 1;
    std::printf("%d %s %d %d\n", id, kNames[int(c->family)], c->bm, c->bn);
  }
  std::printf("igemm_configs %d\n", tfsk::kNumIGemmConfigs);
  return 0;
}
