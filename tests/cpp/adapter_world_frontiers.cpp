// SemanticDSPMap::worldFrontiers (include/semantic_dsp_map.h, "additions") on the wall scene of
// tests/cpp/adapter_world_reach.cpp.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an
// argument: construction only (no device needed).  With `run`: exit code 0 = the archive of the wall scene has frontier
// clusters, the table is the C ABI's called directly, its entries are consistent (ascending, boxes round first cells, float
// fields by the header's formulas), inside_bricks takes away the faces towards absent bricks and min_cells the small
// clusters, a cluster's first cell is reached by
// worldReach(), and the build outlives sdm_world_clear.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adapter_scene.h"
#include "semantic_dsp_map.h"

int main(int argc, char **argv) {
  const bool run = argc > 1;
  SemanticDSPMap a;
  SdmGridPreset p;
  preset(a, p);
  std::vector<sdm_world_frontier_cluster> table;
  if (!run) {
    if (a.worldFrontiers(table) || !table.empty()) return 4;  // no map yet
    std::printf("adapter constructed\n");
    return 0;
  }
  wall_frame(a, p, 0.0);
  if (a.worldFrontiers(table)) return 5;  // no archive yet
  for (int t = 1; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  sdm_world_frontiers_info info;
  if (!a.worldFrontiers(table, 1, false, false, &info)) return 6;
  std::printf("%u bricks, %lld cells, %u clusters of %u, %lld unknown faces, %lld towards absent bricks\n", info.n_bricks, (long long)info.n_cells,
              info.n_clusters, info.n_clusters_total, (long long)info.n_unknown_faces, (long long)info.n_absent_faces);
  if (table.empty() || table.size() != info.n_clusters || info.n_clusters != info.n_clusters_total || info.n_cells < 10 || info.flags != 0u) return 7;
  // the C ABI called directly gives the same table
  std::vector<sdm_world_frontier_cluster> direct(table.size());
  int32_t n = 0;
  if (sdm_get_world_frontier_clusters(a.handle(), direct.data(), (int32_t)direct.size(), &n, nullptr) != SDM_OK || n != (int32_t)table.size()) return 8;
  if (std::memcmp(direct.data(), table.data(), table.size() * sizeof(sdm_world_frontier_cluster)) != 0) return 8;
  int64_t cells = 0, faces = 0;
  for (size_t i = 0; i < table.size(); ++i) {
    const sdm_world_frontier_cluster &c = table[i];
    if (i && c.first_index <= table[i - 1].first_index) return 9;
    if (c.n_cells == 0 || c.n_unknown_faces < c.n_cells || c.pad0 || c.pad1 || c.pad2) return 10;
    for (int ax = 0; ax < 3; ++ax) {
      if (c.first_cell[ax] < c.cell_min[ax] || c.first_cell[ax] > c.cell_max[ax]) return 11;
      if (c.cell_sum[ax] < (int64_t)c.cell_min[ax] * c.n_cells || c.cell_sum[ax] > (int64_t)c.cell_max[ax] * c.n_cells) return 11;
      if (c.box_min[ax] != (float)c.cell_min[ax] * p.voxel_size || c.box_max[ax] != (float)(c.cell_max[ax] + 1) * p.voxel_size) return 12;
      if (c.centroid[ax] != (float)(((double)c.cell_sum[ax] / (double)c.n_cells + 0.5) * (double)p.voxel_size)) return 12;
    }
    cells += c.n_cells;
    faces += c.n_unknown_faces;
  }
  if (cells != info.n_cells || faces != info.n_unknown_faces || info.n_absent_faces < 0 || info.n_absent_faces > info.n_unknown_faces) return 13;
  // without the bricks the archive does not have, and without small clusters, there is less
  std::vector<sdm_world_frontier_cluster> inside, large;
  sdm_world_frontiers_info inside_info, large_info;
  if (!a.worldFrontiers(inside, 1, true, true, &inside_info)) return 14;
  // (the faces towards bricks the archive does not have are exactly what INSIDE_BRICKS takes away)
  if (inside_info.n_absent_faces != 0 || inside_info.n_cells > info.n_cells ||
      inside_info.n_unknown_faces != info.n_unknown_faces - info.n_absent_faces ||
      inside_info.flags != (SDM_WORLD_FRONTIERS_FACE_CONNECTED | SDM_WORLD_FRONTIERS_INSIDE_BRICKS))
    return 14;
  if (!a.worldFrontiers(large, 1 << 30, false, false, &large_info) || !large.empty() || large_info.n_clusters != 0 ||
      large_info.n_clusters_total != info.n_clusters_total || large_info.n_cells != info.n_cells)
    return 15;
  // where to go: the first cell of a cluster is free, so the route planner reaches it from the camera - or says why not
  if (!a.worldFrontiers(table, 1, false, false, &info)) return 16;
  const Eigen::Vector3d cam(0.1, 0.1, 0.1);
  if (!a.worldReach(cam, true)) return 16;
  std::vector<int32_t> goal_cells;
  for (const sdm_world_frontier_cluster &c : table)
    for (int ax = 0; ax < 3; ++ax) goal_cells.push_back(c.first_cell[ax]);
  std::vector<sdm_world_reach_result> res(table.size());
  if (sdm_query_world_reach(a.handle(), nullptr, goal_cells.data(), (int64_t)table.size(), res.data(), 0u) != SDM_OK) return 17;
  size_t reached = 0;
  for (size_t i = 0; i < res.size(); ++i) {
    if (res[i].status > 1) return 18;  // (a frontier cell is a free cell of an archived brick: traversable)
    reached += res[i].status == 0;
  }
  std::printf("%zu of %zu clusters reached from the camera\n", reached, res.size());
  if (reached == 0) return 18;
  // the build is a snapshot: the archive goes, the table stays
  if (sdm_world_clear(a.handle()) != SDM_OK) return 19;
  if (sdm_get_world_frontier_clusters(a.handle(), direct.data(), (int32_t)direct.size(), &n, nullptr) != SDM_OK || n != (int32_t)table.size()) return 19;
  if (std::memcmp(direct.data(), table.data(), table.size() * sizeof(sdm_world_frontier_cluster)) != 0) return 19;
  if (a.worldFrontiers(large)) return 20;  // (no archive any more)
  std::printf("world frontiers ok\n");
  return 0;
}
