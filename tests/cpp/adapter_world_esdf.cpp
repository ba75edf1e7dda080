// SemanticDSPMap::worldEsdf / queryWorldDistance (include/semantic_dsp_map.h, "additions") on the wall scene of
// tests/cpp/adapter_world_reach.cpp.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an
// argument: construction only (no device needed).  With `run`: exit code 0 = the distance field of the wall scene's
// archive answers like the C ABI called directly, an archived obstacle reads 0, the distance grows by one voxel per cell
// walked away from the wall up to the radius and reads "far" behind it, a point in no brick reads -1, and the build
// outlives a worldRetain that removes every brick.
#include <cmath>
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
  std::vector<Eigen::Vector3d> points{Eigen::Vector3d(0.1, 0.1, 0.1)};
  std::vector<sdm_world_distance_result> res;
  if (!run) {
    if (a.worldEsdf(1.f) || a.queryWorldDistance(points, res) != 0 || !res.empty()) return 4;  // no map yet
    std::printf("adapter constructed\n");
    return 0;
  }
  wall_frame(a, p, 0.0);
  if (a.worldEsdf(1.f)) return 5;  // no archive yet
  for (int t = 1; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  if (a.queryWorldDistance(points, res) != 0) return 5;  // no build yet
  sdm_world_esdf_info info;
  if (!a.worldEsdf(1.9f, false, false, &info)) return 6;  // ceil(1.9 / 0.4) = 5 cells
  std::printf("%u bricks, radius %u, %lld obstacle cells, %lld cells within the radius\n", info.n_bricks, info.radius, (long long)info.n_obstacle_cells,
              (long long)info.n_near_cells);
  if (info.radius != 5 || info.flags != 0u || info.n_bricks == 0 || info.n_obstacle_cells < 20 || info.n_near_cells <= info.n_obstacle_cells) return 7;
  // the wall: the archived obstacles lie in one plane of cells; the axis across it, and the obstacle nearest to their middle
  std::vector<sdm_point> occ;
  if (!a.worldOccupied(occ) || (int64_t)occ.size() != info.n_obstacle_cells) return 8;
  double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30}, mid[3] = {0, 0, 0};
  for (const sdm_point &v : occ) {
    const double c[3] = {v.x, v.y, v.z};
    for (int ax = 0; ax < 3; ++ax) lo[ax] = std::min(lo[ax], c[ax]), hi[ax] = std::max(hi[ax], c[ax]), mid[ax] += c[ax] / (double)occ.size();
  }
  int across = 0;
  for (int ax = 1; ax < 3; ++ax)
    if (hi[ax] - lo[ax] < hi[across] - lo[across]) across = ax;
  if (hi[across] - lo[across] > 2.5 * p.voxel_size) return 9;  // a layer of cells, or two where the depth noise straddles a border
  // (of the layer nearest to the camera, so that no obstacle is nearer to the cells walked than the one behind them)
  const double towards = lo[across] > 0 ? -1.0 : 1.0, front = towards < 0 ? lo[across] : hi[across];
  size_t best = 0;
  double best_d = 1e30;
  for (size_t i = 0; i < occ.size(); ++i) {
    const double c[3] = {occ[i].x, occ[i].y, occ[i].z};
    if (std::fabs(c[across] - front) > 0.25 * p.voxel_size) continue;
    double d = 0;
    for (int ax = 0; ax < 3; ++ax) d += ax == across ? 0.0 : (c[ax] - mid[ax]) * (c[ax] - mid[ax]);
    if (d < best_d) best_d = d, best = i;
  }
  // from that obstacle's cell towards the camera, a cell a step; then every obstacle, and a point in no brick
  const double h = 0.5 * p.voxel_size;
  points.clear();
  for (int k = 0; k <= 6; ++k) {
    double c[3] = {occ[best].x + h, occ[best].y + h, occ[best].z + h};
    c[across] += towards * k * (double)p.voxel_size;
    points.push_back(Eigen::Vector3d(c[0], c[1], c[2]));
  }
  const size_t n_walk = points.size();
  for (const sdm_point &v : occ) points.push_back(Eigen::Vector3d(v.x + h, v.y + h, v.z + h));
  points.push_back(Eigen::Vector3d(1e5, 0, 0));
  if (a.queryWorldDistance(points, res) != points.size()) return 10;
  std::vector<float> xyz;
  for (const Eigen::Vector3d &g : points) xyz.push_back((float)g.x()), xyz.push_back((float)g.y()), xyz.push_back((float)g.z());
  std::vector<sdm_world_distance_result> direct(points.size());
  if (sdm_query_world_distance(a.handle(), xyz.data(), nullptr, (int64_t)points.size(), direct.data(), 0u) != SDM_OK) return 11;
  if (std::memcmp(direct.data(), res.data(), res.size() * sizeof(sdm_world_distance_result)) != 0) return 11;
  for (int k = 0; k <= 5; ++k) {  // one voxel per cell walked away from the wall
    const sdm_world_distance_result &r = res[(size_t)k];
    std::printf("%d cells from the wall: d2 %u, %.3f m\n", k, r.d2, r.distance);
    if (r.d2 != (uint32_t)(k * k) || r.distance != std::sqrt((float)(k * k)) * p.voxel_size) return 12;
    for (int ax = 0; ax < 3; ++ax)
      if (r.nearest[ax] != res[0].cell[ax] || (ax != across && r.cell[ax] != res[0].cell[ax])) return 13;
    if (std::abs(r.cell[across] - res[0].cell[across]) != k) return 13;
  }
  const sdm_world_distance_result &far = res[6];
  if (far.d2 != SDM_WORLD_ESDF_FAR || far.distance != std::sqrt((float)26) * p.voxel_size || far.nearest[across] != far.cell[across]) return 14;
  for (size_t i = n_walk; i + 1 < points.size(); ++i)
    if (res[i].d2 != 0u || res[i].distance != 0.f || std::memcmp(res[i].cell, res[i].nearest, sizeof(res[i].cell)) != 0) return 15;
  if (res.back().d2 != 0xffffffffu || res.back().distance != -1.f) return 16;
  // the build is a snapshot: a retain that keeps nothing empties the archive, the answers stay
  const int64_t removed = a.worldRetain(Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(-1, 0, 0));
  if (removed != (int64_t)info.n_bricks) return 17;
  std::vector<sdm_world_distance_result> again;
  if (a.queryWorldDistance(points, again) != points.size() || std::memcmp(again.data(), res.data(), res.size() * sizeof(sdm_world_distance_result)) != 0)
    return 18;
  // the next build sees the empty archive: a field of no bricks
  sdm_world_esdf_info empty;
  if (!a.worldEsdf(100.f, true, true, &empty) || empty.n_bricks != 0 || empty.radius != SDM_WORLD_ESDF_MAX_RADIUS ||
      empty.flags != (SDM_WORLD_ESDF_UNKNOWN_IS_OBSTACLE | SDM_WORLD_ESDF_STATIC_ONLY))
    return 19;
  if (a.queryWorldDistance(points, again) != points.size() || again[0].d2 != 0xffffffffu) return 20;
  if (a.worldEsdf(0.f) || a.worldEsdf(-1.f)) return 21;
  std::printf("world distance field ok\n");
  return 0;
}
