// SemanticDSPMap::worldGroundReach / queryWorldGroundReach / worldGroundReachPaths (include/semantic_dsp_map.h, "additions")
// on the wall scene of tests/cpp/adapter_world_reach.cpp, the wall taken as the ground as in
// tests/cpp/adapter_world_ground.cpp.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an
// argument: construction only (no device needed).  With `run`: exit code 0 = the field over the wall's ground layer answers
// like the C ABI called directly, a goal (du, dv) columns from the start on the flat wall costs 10 max + 4 min and its path
// has max + 1 cells, each of them ground one cell under the robot's base, a point in no tile reads status 3, and the build
// outlives a worldRetain that removes every brick and a ground build of the emptied archive.
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
  sdm_world_ground_options o;
  std::memset(&o, 0, sizeof(o));
  o.up_axis = 2, o.up_sign = 1, o.h_hi = 7, o.radius = 4;
  sdm_world_ground_reach_options ro;
  std::memset(&ro, 0, sizeof(ro));
  ro.max_climb = 1;
  std::vector<int16_t> coords;
  std::vector<sdm_ground_cell> cells;
  std::vector<uint16_t> d2;
  std::vector<Eigen::Vector3d> points{Eigen::Vector3d(0.1, 0.1, 0.1)};
  std::vector<sdm_world_ground_reach_result> res;
  std::vector<std::vector<Eigen::Vector3i>> paths;
  bool ok = true;
  if (!run) {
    if (a.worldGroundReach(points[0], ro) || a.queryWorldGroundReach(points, res) != 0 || !res.empty() || a.worldGroundReachPaths(points, paths) != 0)
      return 4;  // no map yet
    std::printf("adapter constructed\n");
    return 0;
  }
  wall_frame(a, p, 0.0);
  for (int t = 1; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  if (a.worldGroundReach(points[0], ro)) return 5;  // no ground build yet
  // the wall: the archived obstacles lie in one plane of cells; the axis across it, and the obstacle nearest to their middle
  std::vector<sdm_point> occ;
  if (!a.worldOccupied(occ) || occ.size() < 20) return 8;
  double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30}, mid[3] = {0, 0, 0};
  for (const sdm_point &v : occ) {
    const double c[3] = {v.x, v.y, v.z};
    for (int ax = 0; ax < 3; ++ax) lo[ax] = std::min(lo[ax], c[ax]), hi[ax] = std::max(hi[ax], c[ax]), mid[ax] += c[ax] / (double)occ.size();
  }
  int across = 0;
  for (int ax = 1; ax < 3; ++ax)
    if (hi[ax] - lo[ax] < hi[across] - lo[across]) across = ax;
  if (hi[across] - lo[across] > 2.5 * p.voxel_size) return 9;  // a layer of cells, or two where the depth noise straddles a border
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
  const double h = 0.5 * p.voxel_size;
  const double wall[3] = {occ[best].x + h, occ[best].y + h, occ[best].z + h};  // the centre of that obstacle's cell
  // the wall as the ground: up is towards the camera, the band two cells either side of the wall's front layer
  const int sign = towards > 0 ? 1 : -1, au = across == 0 ? 1 : 0, av = across == 2 ? 1 : 2;
  const int g_wall = (int)std::floor(wall[across] / p.voxel_size), h_wall = sign > 0 ? g_wall : -1 - g_wall;
  o.up_axis = across, o.up_sign = sign;
  o.h_lo = h_wall - 2, o.h_hi = h_wall + 2;
  o.clearance = 2, o.max_step = 1, o.radius = 5;
  for (int k = 0; k < 8; ++k) o.support_labels[k] = 0xffffffffu;  // whatever label the wall carries
  sdm_world_ground_info info;
  const size_t n = a.worldGround(o, coords, cells, d2, &info, &ok);
  if (!ok || n == 0) return 6;
  if (a.queryWorldGroundReach(points, res) != 0 || a.worldGroundReachPaths(points, paths) != 0) return 5;  // no build yet
  // the start over the wall's middle, two cells in front of it: only its column counts
  double s[3] = {wall[0], wall[1], wall[2]};
  s[across] += towards * 2.0 * (double)p.voxel_size;
  const Eigen::Vector3d start(s[0], s[1], s[2]);
  sdm_world_ground_reach_info ri;
  if (!a.worldGroundReach(start, ro, &ri)) return 7;
  std::printf("%u tiles, %u traversable, %u reached, largest cost %u, %u rounds\n", ri.n_tiles, ri.n_traversable, ri.n_reached, ri.max_cost_reached,
              ri.rounds);
  if (ri.n_tiles != n || ri.n_starts_used != 1u || ri.n_reached < 20u || ri.n_reached > ri.n_traversable || ri.stamp != info.stamp) return 7;
  if (std::memcmp(&ri.options, &ro, sizeof(ro)) != 0 || ri.pad != 0u) return 7;
  // goals (du, dv) columns from the start, and a point in no tile
  const int off[6][2] = {{0, 0}, {1, 0}, {0, -2}, {2, 1}, {-2, -2}, {-1, 2}};
  points.clear();
  for (int k = 0; k < 6; ++k) {
    double c[3] = {wall[0], wall[1], wall[2]};
    c[au] += off[k][0] * (double)p.voxel_size, c[av] += off[k][1] * (double)p.voxel_size;
    points.push_back(Eigen::Vector3d(c[0], c[1], c[2]));
  }
  points.push_back(Eigen::Vector3d(1e4, 1e4, 1e4));
  if (a.queryWorldGroundReach(points, res) != points.size()) return 10;
  std::vector<float> xyz;
  for (const Eigen::Vector3d &g : points) xyz.push_back((float)g.x()), xyz.push_back((float)g.y()), xyz.push_back((float)g.z());
  std::vector<sdm_world_ground_reach_result> direct(points.size());
  if (sdm_query_world_ground_reach(a.handle(), xyz.data(), nullptr, (int64_t)points.size(), direct.data(), 0u) != SDM_OK) return 11;
  if (std::memcmp(direct.data(), res.data(), res.size() * sizeof(sdm_world_ground_reach_result)) != 0) return 11;
  if (a.worldGroundReachPaths(points, paths) != points.size()) return 12;
  std::vector<int32_t> lens(points.size()), rows(points.size() * 8 * 3, -1);
  if (sdm_world_ground_reach_paths(a.handle(), xyz.data(), nullptr, (int64_t)points.size(), 8, rows.data(), lens.data(), 0u) != SDM_OK) return 12;
  std::vector<Eigen::Vector3d> on_path;
  for (int k = 0; k < 6; ++k) {
    const sdm_world_ground_reach_result &r = res[(size_t)k];
    const int du = std::abs(off[k][0]), dv = std::abs(off[k][1]), far = std::max(du, dv), near = std::min(du, dv);
    std::printf("goal (%d, %d): status %u, cost %u, %.3f m, next %u, level %u, %zu cells\n", off[k][0], off[k][1], r.status, r.cost, r.metres, r.next,
                r.level, paths[(size_t)k].size());
    if (r.status != 0u || r.cost != (uint32_t)(10 * far + 4 * near) || r.metres != (float)r.cost * (p.voxel_size * 0.1f)) return 13;
    if (r.col[0] != res[0].col[0] + off[k][0] || r.col[1] != res[0].col[1] + off[k][1] || (r.next == 4u) != (k == 0) || r.pad != 0u) return 13;
    if (paths[(size_t)k].size() != (size_t)far + 1 || lens[(size_t)k] != far + 1) return 14;   // the closed form: a diagonal while it can
    for (size_t q = 0; q < paths[(size_t)k].size(); ++q) {
      const Eigen::Vector3i &c = paths[(size_t)k][q];
      const int32_t *d = rows.data() + ((size_t)k * 8 + q) * 3;
      if (c(0) != d[0] || c(1) != d[1] || c(2) != d[2]) return 14;
      on_path.push_back(Eigen::Vector3d((c(0) + 0.5) * p.voxel_size, (c(1) + 0.5) * p.voxel_size, (c(2) + 0.5) * p.voxel_size));
    }
    const Eigen::Vector3i &last = paths[(size_t)k].back();
    if (last(au) != res[0].col[0] || last(av) != res[0].col[1]) return 14;  // it ends at the start
  }
  if (res.back().status != 3u || res.back().cost != 0xffffffffu || res.back().metres != -1.f || res.back().next != 255u || res.back().level != 0xffffu)
    return 15;
  if (!paths.back().empty() || lens.back() != 0) return 15;
  // every cell of every path stands on ground: one cell above the level, not lethal
  std::vector<sdm_world_ground_result> under;
  if (a.queryWorldGround(on_path, under) != on_path.size()) return 16;
  for (const sdm_world_ground_result &g : under)
    if (g.status != 0u || (g.cell.cls & 3u) != 1u || (g.cell.cls & 8u) != 0u || g.above != 1) return 16;
  // the build is a snapshot: a retain that keeps nothing empties the archive, a ground build of it has no tiles, the answers stay
  if (a.worldRetain(Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(-1, 0, 0)) <= 0) return 18;
  if (a.worldGround(o, coords, cells, d2, &info, &ok) != 0 || !ok || info.n_tiles != 0u) return 18;
  std::vector<sdm_world_ground_reach_result> again;
  if (a.queryWorldGroundReach(points, again) != points.size() ||
      std::memcmp(again.data(), res.data(), res.size() * sizeof(sdm_world_ground_reach_result)) != 0)
    return 19;
  std::vector<std::vector<Eigen::Vector3i>> paths_again;
  if (a.worldGroundReachPaths(points, paths_again) != points.size() || paths_again[4].size() != paths[4].size()) return 19;
  // the next build stands on the empty ground layer: a field of no tiles, which is no failure
  if (!a.worldGroundReach(start, ro, &ri) || ri.n_tiles != 0u || ri.n_starts_used != 0u) return 20;
  if (a.queryWorldGroundReach(points, again) != points.size() || again[0].status != 3u) return 20;
  ro.penalty = 65536u;
  if (a.worldGroundReach(start, ro)) return 21;
  std::printf("world ground reach ok\n");
  return 0;
}
