// SemanticDSPMap::worldBricks / worldImport / worldRetain (include/semantic_dsp_map.h, "additions") on the wall scene of
// tests/cpp/adapter_world.cpp: one map archives the wall, a second map takes its bricks.  Built against
// tests/mock_includes and linked with libsdm_hip.so.  Without an argument: construction only (no device needed).  With
// `run`: exit code 0 = the second map's archive is the first's byte for byte after an import at offset 0, the same
// obstacles 11 cells further after one at offset (11, 0, -3), FILL onto itself changes nothing, worldRetain removes what
// the C ABI removes when called directly, and an emptied archive takes the bricks again.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adapter_scene.h"
#include "semantic_dsp_map.h"

int main(int argc, char **argv) {
  const bool run = argc > 1;
  SemanticDSPMap a, b;
  SdmGridPreset p;
  preset(a, p);
  preset(b, p);
  std::vector<sdm_world_brick> bricks, got;
  std::vector<uint32_t> cells, got_cells;
  if (!run) {
    bricks.resize(1);
    cells.resize(512);
    if (a.worldImport(bricks, cells) || a.worldRetain(Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(1, 1, 1)) != -1) return 4;  // no map yet
    if (a.worldBricks(got, got_cells) != 0 || !got.empty() || !got_cells.empty()) return 4;
    std::printf("adapter constructed\n");
    return 0;
  }
  for (int t = 0; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  wall_frame(b, p, 0.0);
  const size_t n = a.worldBricks(bricks, cells);
  sdm_world_info ia, ib;
  if (!n || cells.size() != 512 * n || !a.worldInfo(ia) || ia.n_bricks != n || ia.n_occupied == 0) return 6;
  std::printf("%zu bricks, %llu archived obstacles\n", n, (unsigned long long)ia.n_occupied);
  const std::vector<uint32_t> whole = cells;
  cells.pop_back();
  if (b.worldImport(bricks, cells)) return 7;  // not 512 words per brick
  // offset 0: every byte
  if (!b.worldImport(bricks, whole) || b.worldBricks(got, got_cells) != n) return 8;
  if (std::memcmp(got.data(), bricks.data(), n * sizeof(sdm_world_brick)) != 0 || got_cells != whole) return 9;
  if (!b.worldInfo(ib) || ib.n_updates != 0 || ib.created_last != n || ib.n_occupied != ia.n_occupied || ib.n_free != ia.n_free) return 10;
  // FILL onto itself: nothing writes
  if (!b.worldImport(bricks, whole, Eigen::Vector3i(0, 0, 0), SDM_WORLD_IMPORT_FILL) || b.worldBricks(got, got_cells) != n) return 11;
  if (std::memcmp(got.data(), bricks.data(), n * sizeof(sdm_world_brick)) != 0 || got_cells != whole) return 11;
  // the same obstacles, 11 cells further in x and 3 back in z
  std::vector<sdm_point> pa, pb;
  if (a.worldOccupied(pa) != ia.n_occupied) return 12;
  if (b.worldRetain(Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(-1, 0, 0)) != (int64_t)n) return 12;  // an empty box empties it
  if (!b.worldInfo(ib) || ib.n_bricks != 0 || ib.max_bricks != ia.max_bricks) return 12;
  if (!b.worldImport(bricks, whole, Eigen::Vector3i(11, 0, -3)) || b.worldOccupied(pb) != pa.size()) return 13;
  std::vector<Eigen::Vector3d> centres;
  for (const sdm_point &v : pa) centres.push_back(Eigen::Vector3d(v.x + (11 + 0.5) * p.voxel_size, v.y + 0.5 * p.voxel_size, v.z + (0.5 - 3) * p.voxel_size));
  std::vector<sdm_world_cell> at;
  if (b.queryWorld(centres, at) != pa.size()) return 14;
  for (size_t i = 0; i < pa.size(); ++i)
    if (at[i].track != pa[i].track || at[i].label != pa[i].label || at[i].occ != pa[i].occ) return 15;
  // worldRetain against the C ABI called directly, on two archives that hold the same
  if (!b.worldInfo(ib)) return 16;
  sdm_world_retain_options o;
  std::memset(&o, 0, sizeof(o));
  for (int k = 0; k < 3; ++k) o.bmin[k] = ib.bmin[k], o.bmax[k] = ib.bmax[k];
  o.bmax[0] = ib.bmin[0];  // the lowest x only
  if (b.worldRetain(Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(-1, 0, 0)) != (int64_t)ib.n_bricks) return 16;
  if (!a.worldImport(bricks, whole, Eigen::Vector3i(11, 0, -3)) || !b.worldImport(bricks, whole, Eigen::Vector3i(11, 0, -3))) return 17;
  if (a.worldRetain(Eigen::Vector3i(-32768, -32768, -32768), Eigen::Vector3i(32767, 32767, 32767), 0xffffffffu) < (int64_t)n) return 17;  // no stamp is that late
  if (!a.worldImport(bricks, whole, Eigen::Vector3i(11, 0, -3))) return 17;
  int64_t direct = -1;
  if (sdm_world_retain(a.handle(), &o, &direct) != SDM_OK) return 18;
  const int64_t through = b.worldRetain(Eigen::Vector3i(o.bmin[0], o.bmin[1], o.bmin[2]), Eigen::Vector3i(o.bmax[0], o.bmax[1], o.bmax[2]));
  std::printf("retain removed %lld of %u bricks\n", (long long)through, ib.n_bricks);
  if (through != direct || through <= 0 || through >= (int64_t)ib.n_bricks) return 19;
  std::vector<sdm_world_brick> ha, hb;
  std::vector<uint32_t> ca, cb;
  if (a.worldBricks(ha, ca) != b.worldBricks(hb, cb) || ha.empty() || std::memcmp(ha.data(), hb.data(), ha.size() * sizeof(sdm_world_brick)) != 0 || ca != cb)
    return 20;
  for (const sdm_world_brick &h : ha)
    if (h.bx != o.bmin[0]) return 21;
  std::printf("world io ok\n");
  return 0;
}
