// SemanticDSPMap::reach (include/semantic_dsp_map.h, "additions") on the wall scene of tests/cpp/adapter_views.cpp: a
// wall with one movable object in front of it, seen from two places, driven through update().  Built against
// tests/mock_includes and linked with libsdm_hip.so.  Without an argument: construction only (no device needed).  With
// `run`: exit code 0 = the adapter's results are the bytes the C ABI gives when called directly, a goal four cells ahead
// of the camera is reached at no less than four face moves, its path leads from its cell to the start's cell by
// neighbouring cells, a goal far outside the map is refused, and a budget cuts the far goals off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "semantic_dsp_map.h"

int main(int argc, char **argv) {
  const bool run = argc > 1;
  SemanticDSPMap map;
  SdmGridPreset p = SdmGridPreset::VirtualKitti2();
  p.x_n = p.y_n = p.z_n = 5;
  p.voxel_size = 0.4f;
  p.width = 128;
  p.height = 80;
  p.fx = p.fy = 80.f;
  p.cx = 64.f;
  p.cy = 40.f;
  p.depth_max = 12.f;
  p.window_half = 3;
  map.setGridPreset(p);
  map.setMapParameters(0.98f, 0.001f, 1, 0.5f, 5, 1.0f, 3, 0.6f, 0.2f);
  map.setMapOptions(true, false);
  map.setDepthNoiseModelParameters(0.01f, 0.2f);
  const Eigen::Vector3d start(0, 4.4, 0);
  std::vector<Eigen::Vector3d> goals;
  goals.push_back(Eigen::Vector3d(0, 4.4, 1.6));     // four cells ahead of the camera, in front of the object
  goals.push_back(Eigen::Vector3d(0, 4.4, 0));       // the start itself
  goals.push_back(Eigen::Vector3d(-3.0, 4.4, 5.0));  // beside and behind the wall: never observed
  goals.push_back(Eigen::Vector3d(100, 0, 0));       // far outside the map
  std::vector<sdm_reach_result> got, ref;
  std::vector<std::vector<uint32_t>> paths;
  if (!run) {
    if (map.reach(start, goals, got, true, 0.f, 0, &paths) != 0 || !got.empty() || !paths.empty()) return 4;  // no map yet
    std::printf("adapter constructed\n");
    return 0;
  }
  cv::Mat depth(p.height, p.width, 4);
  MaskKpts st, car;
  st.track_id = 65535;
  st.label = "static";
  st.mask = cv::Mat(p.height, p.width, 1);
  car.track_id = 2;
  car.label = "Car";
  car.mask = cv::Mat(p.height, p.width, 1);
  car.bbox = BBox2D{40, 20, 90, 60};
  for (int i = 0; i < p.height; ++i)
    for (int j = 0; j < p.width; ++j) {
      const bool on_car = i >= 20 && i < 60 && j >= 40 && j < 90;
      depth.at<float>(i, j) = on_car ? 2.0f : 3.0f;  // a wall 3 m ahead, the object 2 m ahead
      st.mask.at<uchar>(i, j) = 5;                   // pixel value + 1 = label 6 (Building)
      car.mask.at<uchar>(i, j) = on_car ? 255 : 0;
    }
  car.kpts_current = {Eigen::Vector3d(-0.3, -0.2, 2), Eigen::Vector3d(0.3, -0.2, 2), Eigen::Vector3d(-0.3, 0.3, 2), Eigen::Vector3d(0.3, 0.3, 2)};
  car.kpts_previous = car.kpts_current;
  std::vector<MaskKpts> seg{st, car};
  Eigen::Quaterniond q(1, 0, 0, 0);
  for (int t = 0; t < 6; ++t) {
    Eigen::Vector3d pos(0, t < 4 ? 0.0 : 4.4, 0);
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr occ(new pcl::PointCloud<pcl::PointXYZRGB>), fr(new pcl::PointCloud<pcl::PointXYZRGB>);
    map.update(depth, seg, pos, q, occ, fr, false, 0.1 * t);
    std::printf("frame %d: %zu occupied voxels\n", t, occ->size());
  }
  if (map.reach(start, goals, got, true, 0.f, 0, &paths) != goals.size() || got.size() != goals.size() || paths.size() != goals.size()) return 5;
  // the C ABI directly, on the field the adapter has just built
  std::vector<float> xyz;
  for (const auto &g : goals) {
    xyz.push_back((float)g.x());
    xyz.push_back((float)g.y());
    xyz.push_back((float)g.z());
  }
  ref.resize(goals.size());
  if (sdm_query_reach(map.handle(), xyz.data(), nullptr, (int64_t)goals.size(), ref.data(), 0u) != SDM_OK) return 6;
  if (std::memcmp(got.data(), ref.data(), got.size() * sizeof(sdm_reach_result)) != 0) return 7;
  sdm_reach_info info;
  if (sdm_get_reach(map.handle(), nullptr, &info, nullptr) != SDM_OK) return 8;
  std::printf("field: %u of %u traversable cells reached in %u rounds, farthest %u\n", info.n_reached, info.n_traversable, info.rounds,
              info.max_cost_reached);
  for (size_t i = 0; i < got.size(); ++i)
    std::printf("goal %zu: status %u, cost %u (%.2f m), cell %u, next %u, path of %zu cells\n", i, got[i].status, got[i].cost, got[i].metres,
                got[i].cell, got[i].next, paths[i].size());
  if (info.n_starts_used != 1 || info.flags != SDM_REACH_THROUGH_UNKNOWN || info.n_reached < 1000) return 9;
  const float scale = p.voxel_size * 0.1f;
  if (got[0].status != 0 || got[0].cost < 40 || got[0].metres != (float)got[0].cost * scale || got[0].next == 13 || got[0].next > 26) return 10;
  if (got[1].status != 0 || got[1].cost != 0 || got[1].next != 13 || got[1].metres != 0.f || paths[1].size() != 1 || paths[1][0] != got[1].cell)
    return 11;
  if (got[2].status != 0 || got[2].cost <= got[0].cost) return 12;
  if (got[3].status != 3 || got[3].cost != 0xffffffffu || got[3].metres != -1.f || got[3].cell != 0xffffffffu || got[3].next != 255 ||
      !paths[3].empty())
    return 13;
  for (size_t i = 0; i < 3; ++i) {  // from the goal's cell to the start's, by neighbouring cells, no longer than cost / 10 + 1
    const std::vector<uint32_t> &w = paths[i];
    if (w.empty() || w.front() != got[i].cell || w.back() != got[1].cell || w.size() > got[i].cost / 10 + 1) return 14;
    for (size_t k = 1; k < w.size(); ++k)
      for (int a = 0; a < 3; ++a) {
        const int c0 = (int)((w[k - 1] >> (5 * a)) & 31u), c1 = (int)((w[k] >> (5 * a)) & 31u);
        if (std::abs(c0 - c1) > 1) return 15;
      }
    if (got[i].pad != 0) return 16;
  }
  // a budget of 2.5 m: the goal ahead stays, the one behind the wall is beyond it
  std::vector<sdm_reach_result> near;
  if (map.reach(start, goals, near, true, 2.5f) != goals.size()) return 17;
  if (near[0].status != 0 || near[0].cost != got[0].cost || near[2].status != 1 || near[2].cost != 0xffffffffu) return 18;
  // free cells only: whatever the goals read, the call works and the field is the new one
  if (map.reach(start, goals, near, false, 0.f, 1) != goals.size() || near[3].status != 3) return 19;
  if (sdm_get_reach(map.handle(), nullptr, &info, nullptr) != SDM_OK || info.flags != 0u || info.min_d2 != 1u) return 20;
  std::printf("reach ok\n");
  return 0;
}
