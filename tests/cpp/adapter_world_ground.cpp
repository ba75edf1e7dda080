// SemanticDSPMap::worldGround / queryWorldGround / checkWorldFootprints (include/semantic_dsp_map.h, "additions") on the
// wall scene of tests/cpp/adapter_world_reach.cpp, the wall taken as the ground: the up axis is the axis across the wall,
// up is towards the camera.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an argument:
// construction only (no device needed).  With `run`: exit code 0 = the layer of the wall scene's archive answers like the
// C ABI called directly, the wall's middle is ground, a point k cells in front of it stands k cells above the level, a
// footprint of three by three columns covers nine, a point in no tile reads status 3, and the build outlives a
// worldRetain that removes every brick.
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
  std::vector<int16_t> coords;
  std::vector<sdm_ground_cell> cells;
  std::vector<uint16_t> d2;
  std::vector<Eigen::Vector3d> points{Eigen::Vector3d(0.1, 0.1, 0.1)};
  std::vector<sdm_world_ground_result> res;
  std::vector<sdm_footprint> fps(1);
  std::memset(fps.data(), 0, sizeof(sdm_footprint));
  std::vector<sdm_world_footprint_result> fres;
  bool ok = true;
  if (!run) {
    if (a.worldGround(o, coords, cells, d2, nullptr, &ok) != 0 || ok || a.queryWorldGround(points, res) != 0 || !res.empty() ||
        a.checkWorldFootprints(fps, fres) != 0)
      return 4;  // no map yet
    std::printf("adapter constructed\n");
    return 0;
  }
  wall_frame(a, p, 0.0);
  if (a.worldGround(o, coords, cells, d2, nullptr, &ok) != 0 || ok) return 5;  // no archive yet
  for (int t = 1; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  if (a.queryWorldGround(points, res) != 0 || a.checkWorldFootprints(fps, fres) != 0) return 5;  // no build yet
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
  std::printf("%zu tiles, %lld ground, %lld obstacle, %lld none, %lld step, %lld lethal columns, levels %u .. %u\n", n, (long long)info.n_ground,
              (long long)info.n_obstacle, (long long)info.n_none, (long long)info.n_step, (long long)info.n_lethal, info.level_min, info.level_max);
  if (!ok || n == 0 || n != info.n_tiles || coords.size() != 2 * n || cells.size() != 64 * n || d2.size() != 64 * n) return 6;
  if (info.n_ground < 20 || info.n_ground + info.n_obstacle + info.n_none != (int64_t)(64 * n) || info.level_max > 4u) return 7;
  if (std::memcmp(&info.options, &o, sizeof(o)) != 0) return 7;
  int64_t ground = 0;
  for (const sdm_ground_cell &c : cells) ground += (c.cls & 3u) == 1u;
  if (ground != info.n_ground) return 7;
  // from the wall's cell towards the camera, a cell a step; a point in no tile
  points.clear();
  for (int k = 0; k <= 4; ++k) {
    double c[3] = {wall[0], wall[1], wall[2]};
    c[across] += towards * k * (double)p.voxel_size;
    points.push_back(Eigen::Vector3d(c[0], c[1], c[2]));
  }
  points.push_back(Eigen::Vector3d(1e4, 1e4, 1e4));
  if (a.queryWorldGround(points, res) != points.size()) return 10;
  std::vector<float> xyz;
  for (const Eigen::Vector3d &g : points) xyz.push_back((float)g.x()), xyz.push_back((float)g.y()), xyz.push_back((float)g.z());
  std::vector<sdm_world_ground_result> direct(points.size());
  if (sdm_query_world_ground(a.handle(), xyz.data(), nullptr, (int64_t)points.size(), direct.data(), 0u) != SDM_OK) return 11;
  if (std::memcmp(direct.data(), res.data(), res.size() * sizeof(sdm_world_ground_result)) != 0) return 11;
  const int k_face = sign > 0 ? g_wall + 1 : g_wall;  // the world coordinate of the wall cell's face towards the camera
  for (int k = 0; k <= 4; ++k) {
    const sdm_world_ground_result &r = res[(size_t)k];
    std::printf("%d cells in front of the wall: level %u, above %d, surface %.3f, d2 %u\n", k, r.cell.level, r.above, r.surface, r.d2);
    if (r.status != 0u || (r.cell.cls & 3u) != 1u || r.cell.level != 2u || r.above != k || r.surface != (float)k_face * p.voxel_size) return 12;
    if (r.col[0] != res[0].col[0] || r.col[1] != res[0].col[1] || r.cell.headroom < 2u) return 13;
  }
  if (res.back().status != 3u || res.back().d2 != 0xffffffffu || res.back().dist != -1.f || res.back().cell.level != 0xffffu) return 14;
  // a footprint of three by three columns round the wall's middle, and one far away
  fps.resize(2);
  fps[0].center_u = (float)wall[au], fps[0].center_v = (float)wall[av];
  fps[0].dir_u = 1.f, fps[0].dir_v = 0.f;
  fps[0].half_len = fps[0].half_wid = 1.5f * p.voxel_size;
  fps[1] = fps[0];
  fps[1].center_u = fps[0].center_u + 4000.f * p.voxel_size;  // (a cell's centre again, within a float32 step)
  if (a.checkWorldFootprints(fps, fres) != 2) return 15;
  std::vector<sdm_world_footprint_result> fdirect(2);
  if (sdm_query_world_footprints(a.handle(), fps.data(), 2, fdirect.data(), 0u) != SDM_OK) return 16;
  if (std::memcmp(fdirect.data(), fres.data(), 2 * sizeof(sdm_world_footprint_result)) != 0) return 16;
  std::printf("footprint: %u columns, %u ground, %u lethal, %u absent\n", fres[0].n_cols, fres[0].n_ground, fres[0].n_lethal, fres[0].n_absent);
  if (fres[0].n_cols + fres[0].n_absent != 9u || fres[0].n_ground < 1u || fres[0].level_min > 4u) return 17;
  if (fres[1].n_cols != 0u || fres[1].n_absent != 9u || fres[1].min_d2 != 0xffffffffu) return 17;
  // the build is a snapshot: a retain that keeps nothing empties the archive, the answers stay
  if (a.worldRetain(Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(-1, 0, 0)) <= 0) return 18;
  std::vector<sdm_world_ground_result> again;
  if (a.queryWorldGround(points, again) != points.size() || std::memcmp(again.data(), res.data(), res.size() * sizeof(sdm_world_ground_result)) != 0)
    return 18;
  // the next build sees the empty archive: a layer of no tiles, which is no failure
  if (a.worldGround(o, coords, cells, d2, &info, &ok) != 0 || !ok || info.n_tiles != 0u || !cells.empty()) return 19;
  if (a.queryWorldGround(points, again) != points.size() || again[0].status != 3u) return 20;
  o.radius = 0;
  if (a.worldGround(o, coords, cells, d2, nullptr, &ok) != 0 || ok) return 21;
  std::printf("world ground layer ok\n");
  return 0;
}
