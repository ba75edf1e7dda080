// SemanticDSPMap::worldReach / queryWorldReach / worldReachPaths (include/semantic_dsp_map.h, "additions") on the wall
// scene of tests/cpp/adapter_world.cpp.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an
// argument: construction only (no device needed).  With `run`: exit code 0 = a build from the camera's position reaches
// archived cells, the results are those of the C ABI called directly, the archived obstacles read "not traversable", every
// path runs from its goal to the start in steps of one cell and within cost / 10 + 1 cells, a budget cuts the field, and the
// build outlives sdm_world_clear.
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
  const Eigen::Vector3d cam(0.1, 0.1, 0.1);
  std::vector<Eigen::Vector3d> goals{cam};
  std::vector<sdm_world_reach_result> res;
  std::vector<std::vector<Eigen::Vector3i>> paths;
  if (!run) {
    if (a.worldReach(cam) || a.queryWorldReach(goals, res) != 0 || !res.empty() || a.worldReachPaths(goals, paths) != 0) return 4;  // no map yet
    std::printf("adapter constructed\n");
    return 0;
  }
  wall_frame(a, p, 0.0);
  if (a.worldReach(cam)) return 5;  // no archive yet
  for (int t = 1; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  if (a.queryWorldReach(goals, res) != 0) return 5;  // no build yet
  sdm_world_reach_info info;
  if (!a.worldReach(cam, true, 0.f, 0, false, &info)) return 6;
  std::printf("%u bricks, %u traversable, %u reached, largest cost %u, %u rounds\n", info.n_bricks, info.n_traversable, info.n_reached,
              info.max_cost_reached, info.rounds);
  if (info.n_starts_used != 1 || info.n_reached < 100 || info.flags != SDM_WORLD_REACH_THROUGH_UNKNOWN) return 7;
  // goals: a grid round the camera, and the archived obstacles
  for (int k = -6; k <= 6; ++k)
    for (int j = -6; j <= 6; ++j)
      for (int i = -6; i <= 6; ++i) goals.push_back(Eigen::Vector3d(cam.x() + 0.8 * i, cam.y() + 0.8 * j, cam.z() + 0.8 * k));
  const size_t n_grid = goals.size();
  std::vector<sdm_point> occ;
  if (!a.worldOccupied(occ)) return 8;
  for (const sdm_point &v : occ) goals.push_back(Eigen::Vector3d(v.x + 0.5 * p.voxel_size, v.y + 0.5 * p.voxel_size, v.z + 0.5 * p.voxel_size));
  goals.push_back(Eigen::Vector3d(1e5, 0, 0));  // in no brick
  if (a.queryWorldReach(goals, res) != goals.size()) return 9;
  std::vector<float> xyz;
  for (const Eigen::Vector3d &g : goals) xyz.push_back((float)g.x()), xyz.push_back((float)g.y()), xyz.push_back((float)g.z());
  std::vector<sdm_world_reach_result> direct(goals.size());
  if (sdm_query_world_reach(a.handle(), xyz.data(), nullptr, (int64_t)goals.size(), direct.data(), 0u) != SDM_OK) return 10;
  if (std::memcmp(direct.data(), res.data(), res.size() * sizeof(sdm_world_reach_result)) != 0) return 10;
  if (res[0].status != 0 || res[0].cost != 0 || res[0].next != 13 || res[0].metres != 0.f) return 11;
  size_t reached = 0;
  for (size_t i = 0; i < n_grid; ++i) reached += res[i].status == 0;
  for (size_t i = n_grid; i + 1 < goals.size(); ++i)
    if (res[i].status != 2 || res[i].cost != 0xffffffffu || res[i].metres != -1.f) return 12;
  if (res.back().status != 3 || reached < 20) return 13;
  // the paths
  if (a.worldReachPaths(goals, paths) != goals.size()) return 14;
  for (size_t i = 0; i < goals.size(); ++i) {
    if ((res[i].status == 0) != !paths[i].empty()) return 15;
    if (paths[i].empty()) continue;
    const std::vector<Eigen::Vector3i> &w = paths[i];
    if (w.size() > res[i].cost / 10u + 1u || w.front().x() != res[i].cell[0] || w.front().y() != res[i].cell[1] || w.front().z() != res[i].cell[2]) return 16;
    if (w.back().x() != res[0].cell[0] || w.back().y() != res[0].cell[1] || w.back().z() != res[0].cell[2]) return 17;
    for (size_t k = 1; k < w.size(); ++k)
      if (std::abs(w[k].x() - w[k - 1].x()) > 1 || std::abs(w[k].y() - w[k - 1].y()) > 1 || std::abs(w[k].z() - w[k - 1].z()) > 1) return 18;
  }
  // the build is a snapshot: the archive goes, the answers stay
  if (sdm_world_clear(a.handle()) != SDM_OK) return 19;
  std::vector<sdm_world_reach_result> again;
  if (a.queryWorldReach(goals, again) != goals.size() || std::memcmp(again.data(), res.data(), res.size() * sizeof(sdm_world_reach_result)) != 0) return 19;
  if (a.worldReach(cam)) return 19;  // (no archive any more)
  // a budget of 2 m cuts the field
  if (!a.worldUpdate()) return 20;
  sdm_world_reach_info cut;
  if (!a.worldReach(cam, true, 2.0f, 0, false, &cut)) return 20;
  std::printf("with 2 m: %u reached, largest cost %u of %u\n", cut.n_reached, cut.max_cost_reached, cut.max_cost);
  if ((cut.max_cost != 50 && cut.max_cost != 49) || cut.max_cost_reached > cut.max_cost || cut.n_reached == 0 || cut.n_reached >= info.n_reached) return 21;
  sdm_world_reach_info wide;
  if (!a.worldReach(cam, true, 0.f, 1, true, &wide) || wide.inflate != 1 || wide.n_traversable >= info.n_traversable) return 22;
  if (a.worldReach(cam, true, 0.f, 3)) return 23;  // inflate > 2
  std::printf("world reach ok\n");
  return 0;
}
