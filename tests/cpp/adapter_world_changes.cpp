// SemanticDSPMap::worldChanges / queryWorldChanges (include/semantic_dsp_map.h, "additions") on the wall scene of
// tests/cpp/adapter_world_reach.cpp.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an
// argument: construction only (no device needed).  With `run`: exit code 0 = right after an archiving the block and the
// archive agree (no change, the same cells on both sides); after the camera has moved on and the block has seen more, the
// changes are what the counters say - the table is the C ABI's called directly, its entries are consistent (ascending,
// boxes round first cells, float fields by the header's formulas, the counts add up to info's) -, a region's first cell is
// answered with its index and class, all-zero masks list nothing, and the build outlives the archiving that follows it,
// after which a second build lists nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adapter_scene.h"
#include "semantic_dsp_map.h"

static sdm_world_changes_options all_changes() {
  sdm_world_changes_options o;
  std::memset(&o, 0, sizeof(o));
  for (int i = 0; i < 8; ++i) o.labels[i] = 0xffffffffu;
  o.classes = (1u << SDM_WORLD_CHANGE_APPEARED) | (1u << SDM_WORLD_CHANGE_VANISHED) | (1u << SDM_WORLD_CHANGE_RELABELLED);
  return o;
}

int main(int argc, char **argv) {
  const bool run = argc > 1;
  SemanticDSPMap a;
  SdmGridPreset p;
  preset(a, p);
  std::vector<sdm_world_change_region> table;
  std::vector<sdm_world_change_result> res;
  sdm_world_changes_options o = all_changes();
  if (!run) {
    if (a.worldChanges(o, table) || !table.empty()) return 4;  // no map yet
    if (a.queryWorldChanges({Eigen::Vector3d(0, 0, 0)}, res) != 0 || !res.empty()) return 4;
    std::printf("adapter constructed\n");
    return 0;
  }
  wall_frame(a, p, 0.0);
  if (a.worldChanges(o, table)) return 5;  // no archive yet
  if (!a.worldUpdate()) return 5;
  sdm_world_changes_info info;
  // what has just been archived is what the block sees
  if (!a.worldChanges(o, table, &info)) return 6;
  if (!table.empty() || info.n_cells != 0 || info.n_appeared || info.n_vanished || info.n_relabelled || info.n_new_occupied || info.n_new_free ||
      info.n_known_now == 0 || info.n_known_now != info.n_same_occupied + info.n_same_free)
    return 6;
  // the camera moves on: the block sees more than the archive remembers
  for (int t = 1; t < 4; ++t) wall_frame(a, p, 0.1 * t);
  if (!a.worldChanges(o, table, &info)) return 7;
  std::printf("%u candidates, %u bricks, %lld cells, %u regions of %u; appeared %llu vanished %llu relabelled %llu new %llu + %llu\n", info.n_candidates,
              info.n_bricks, (long long)info.n_cells, info.n_regions, info.n_regions_total, (unsigned long long)info.n_appeared,
              (unsigned long long)info.n_vanished, (unsigned long long)info.n_relabelled, (unsigned long long)info.n_new_occupied,
              (unsigned long long)info.n_new_free);
  const uint64_t changes = info.n_appeared + info.n_vanished + info.n_relabelled;
  if (table.size() != info.n_regions || info.n_regions != info.n_regions_total || (uint64_t)info.n_cells != changes || info.flags != 0u) return 7;
  if (info.n_known_now != changes + info.n_same_occupied + info.n_same_free + info.n_new_occupied + info.n_new_free) return 7;
  if (info.n_known_before != changes + info.n_same_occupied + info.n_same_free + info.n_remembered) return 7;
  std::vector<sdm_world_change_region> direct(table.size());
  int32_t n = 0;
  if (sdm_get_world_changes(a.handle(), direct.data(), (int32_t)direct.size(), &n, nullptr) != SDM_OK || n != (int32_t)table.size()) return 8;
  if (!table.empty() && std::memcmp(direct.data(), table.data(), table.size() * sizeof(sdm_world_change_region)) != 0) return 8;
  int64_t cells = 0;
  for (size_t i = 0; i < table.size(); ++i) {
    const sdm_world_change_region &c = table[i];
    if (i && c.first_index <= table[i - 1].first_index) return 9;
    if (c.n_cells == 0 || c.pad || c.mixed > 1 || c.cls < SDM_WORLD_CHANGE_APPEARED || c.cls > SDM_WORLD_CHANGE_RELABELLED) return 10;
    for (int ax = 0; ax < 3; ++ax) {
      if (c.first_cell[ax] < c.cell_min[ax] || c.first_cell[ax] > c.cell_max[ax]) return 11;
      if (c.cell_sum[ax] < (int64_t)c.cell_min[ax] * c.n_cells || c.cell_sum[ax] > (int64_t)c.cell_max[ax] * c.n_cells) return 11;
      if (c.box_min[ax] != (float)c.cell_min[ax] * p.voxel_size || c.box_max[ax] != (float)(c.cell_max[ax] + 1) * p.voxel_size) return 12;
      if (c.centroid[ax] != (float)(((double)c.cell_sum[ax] / (double)c.n_cells + 0.5) * (double)p.voxel_size)) return 12;
    }
    cells += c.n_cells;
  }
  if (cells != info.n_cells) return 13;
  if (!table.empty()) {  // where is the first change?  its first cell, asked as a point
    const sdm_world_change_region &c = table[0];
    const double vs = p.voxel_size;
    const Eigen::Vector3d first((c.first_cell[0] + 0.5) * vs, (c.first_cell[1] + 0.5) * vs, (c.first_cell[2] + 0.5) * vs);
    if (a.queryWorldChanges({first}, res) != 1) return 14;
    if (res[0].region != 0u || res[0].index != c.first_index || res[0].cls != c.cls) return 14;
  }
  // all-zero masks list nothing, the counters stay
  std::vector<sdm_world_change_region> none;
  sdm_world_changes_info none_info;
  sdm_world_changes_options z = all_changes();
  z.classes = 0u;
  if (!a.worldChanges(z, none, &none_info) || !none.empty() || none_info.n_cells != 0 || none_info.n_appeared != info.n_appeared ||
      none_info.n_new_occupied != info.n_new_occupied)
    return 15;
  z.classes = 1u;  // bit 0 is no class
  if (a.worldChanges(z, none)) return 15;
  // the build is a snapshot: the archiving that follows leaves it alone, and a second build of the same frame lists nothing
  if (!a.worldChanges(o, table, &info)) return 16;
  if (!a.worldUpdate()) return 16;
  direct.resize(table.size());
  if (sdm_get_world_changes(a.handle(), direct.data(), (int32_t)direct.size(), &n, nullptr) != SDM_OK || n != (int32_t)table.size()) return 17;
  if (!table.empty() && std::memcmp(direct.data(), table.data(), table.size() * sizeof(sdm_world_change_region)) != 0) return 17;
  sdm_world_changes_info after;
  if (!a.worldChanges(o, none, &after) || !none.empty() || after.n_cells != 0 || after.n_appeared || after.n_vanished || after.n_relabelled ||
      after.n_new_occupied || after.n_new_free)
    return 18;
  std::printf("world changes ok\n");
  return 0;
}
