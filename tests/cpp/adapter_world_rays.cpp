// SemanticDSPMap::queryWorldSegments / scoreWorldViews (include/semantic_dsp_map.h, "additions") on the wall scene of
// tests/cpp/adapter_world_reach.cpp.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an
// argument: construction only (no device needed).  With `run`: exit code 0 = both members answer like the C ABI called
// directly, a ray toward the wall hits at the wall's cell, a ray away from it runs into bricks the archive does not have
// with unknown > 0, and a view toward the wall sees free cells, the wall and - beside it - unknown space.
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
  // toward the wall, away from it, and one that is too long
  std::vector<Eigen::Vector3d> from(3, Eigen::Vector3d(0.1, 0.1, 0.1)), to{Eigen::Vector3d(0.1, 0.1, 5.0), Eigen::Vector3d(0.1, 0.1, -30.1),
                                                                             Eigen::Vector3d(0.1, 0.1, 4000.0)};
  std::vector<sdm_world_segment_hit> hits;
  sdm_view v;
  std::memset(&v, 0, sizeof(v));
  v.q[0] = 1.f;
  v.pos[0] = v.pos[1] = v.pos[2] = 0.1f;
  v.range = 5.f;
  std::vector<sdm_view> views{v};
  std::vector<sdm_view_gain> gains;
  if (!run) {
    if (a.queryWorldSegments(from, to, hits) != 0 || !hits.empty() || a.scoreWorldViews(views, 8, 4.f, gains) != 0 || !gains.empty()) return 4;  // no map yet
    std::printf("adapter constructed\n");
    return 0;
  }
  wall_frame(a, p, 0.0);
  if (a.queryWorldSegments(from, to, hits) != 0 || a.scoreWorldViews(views, 8, 4.f, gains) != 0) return 5;  // no archive yet
  for (int t = 1; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  if (a.queryWorldSegments(from, to, hits) != 3) return 6;
  std::vector<float> ab;
  for (size_t i = 0; i < from.size(); ++i) {
    ab.push_back((float)from[i].x()), ab.push_back((float)from[i].y()), ab.push_back((float)from[i].z());
    ab.push_back((float)to[i].x()), ab.push_back((float)to[i].y()), ab.push_back((float)to[i].z());
  }
  std::vector<sdm_world_segment_hit> direct(3);
  if (sdm_query_world_segments(a.handle(), ab.data(), 3, direct.data(), 0u) != SDM_OK) return 7;
  if (std::memcmp(direct.data(), hits.data(), 3 * sizeof(sdm_world_segment_hit)) != 0) return 7;
  const sdm_world_segment_hit &wall = hits[0], &away = hits[1], &far = hits[2];
  std::printf("toward the wall: t %.4f, cell (%d, %d, %d), occ %d, track %u, %d cells, %d unknown, stamp %u\n", wall.t, wall.cell[0], wall.cell[1],
              wall.cell[2], (int)wall.occ, (unsigned)wall.track, wall.cells, wall.unknown, wall.stamp);
  // the wall stands 3 m ahead: cell 7 along z at 0.4 m voxels, or the one beside it where the depth noise straddles a border
  if (!(wall.t > 0.f && wall.t < 1.f) || wall.occ < 1 || wall.cell[0] != 0 || wall.cell[1] != 0 || std::abs(wall.cell[2] - 7) > 1) return 8;
  if (wall.cells != wall.cell[2] + 1 || wall.track == 0 || wall.stamp == 0u) return 8;
  std::printf("away from it: t %.1f, %d cells, %d unknown\n", away.t, away.cells, away.unknown);
  if (away.t != -1.f || away.cells != 77 || away.unknown < 60 || away.stamp != 0u) return 9;  // cells 0 .. -76 along z: floor(-30.1 / 0.4) = -76
  if (far.t != -1.f || far.cells != -1 || far.unknown != 0) return 10;
  // with UNKNOWN_BLOCKS the ray away from the wall is stopped by the first cell nobody has observed
  std::vector<sdm_world_segment_hit> blocked;
  if (a.queryWorldSegments(from, to, blocked, true) != 3 || !(blocked[1].t >= 0.f) || blocked[1].occ != -1 || blocked[1].cells > away.cells) return 11;
  // the view toward the wall
  if (a.scoreWorldViews(views, 8, 4.f, gains) != 1) return 12;
  const std::vector<float> &rays = a.viewRays(8);
  sdm_view_gain g;
  if (sdm_query_world_views(a.handle(), views.data(), 1, rays.data(), (int32_t)(rays.size() / 3), 10, &g, nullptr, 0u) != SDM_OK) return 13;  // ceil(4 / 0.4)
  if (std::memcmp(&g, gains.data(), sizeof(g)) != 0) return 13;
  std::printf("view: %u unknown, %u free, %u occupied cells, %u of %u rays hit\n", g.n_unknown, g.n_free, g.n_occupied, g.rays_hit, g.rays_in_map);
  if (g.rays_in_map != rays.size() / 3 || g.n_free == 0 || g.n_occupied == 0 || g.rays_hit == 0 || g.pad != 0u) return 14;
  if (a.scoreWorldViews(views, 8, 0.f, gains) != 0 || a.scoreWorldViews(views, 0, 4.f, gains) != 0) return 15;
  from.pop_back();
  if (a.queryWorldSegments(from, to, hits) != 0) return 16;  // lists of different lengths
  std::printf("world rays ok\n");
  return 0;
}
