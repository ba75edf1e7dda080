// SemanticDSPMap::worldUpdate / worldInfo / worldOccupied / queryWorld (include/semantic_dsp_map.h, "additions") on the
// wall scene of tests/cpp/adapter_mesh.cpp, the camera then moved sideways by more than half the map: what the block has
// left stays in the archive.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an argument:
// construction only (no device needed).  With `run`: exit code 0 = the adapter's vectors are the bytes the C ABI gives when
// called directly, every archived obstacle answers for itself through queryWorld, and obstacles archived before the move
// lie outside the block the ring covers after it.
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
  std::vector<sdm_point> pts;
  std::vector<sdm_world_cell> cells;
  sdm_world_info info;
  if (!run) {
    pts.resize(1);
    cells.resize(1);
    if (map.worldUpdate() || map.worldInfo(info) || info.n_bricks != 0 || map.worldOccupied(pts) != 0 || !pts.empty()) return 4;  // no map yet
    if (map.queryWorld({Eigen::Vector3d(0, 0, 0)}, cells) != 0 || !cells.empty()) return 4;
    std::printf("adapter constructed\n");
    return 0;
  }
  cv::Mat depth(p.height, p.width, 4);
  MaskKpts st;
  st.track_id = 65535;
  st.label = "static";
  st.mask = cv::Mat(p.height, p.width, 1);
  for (int i = 0; i < p.height; ++i)
    for (int j = 0; j < p.width; ++j) {
      depth.at<float>(i, j) = 3.0f;   // a wall 3 m ahead
      st.mask.at<uchar>(i, j) = 5;    // pixel value + 1 = label 6 (Building)
    }
  std::vector<MaskKpts> seg{st};
  Eigen::Quaterniond q(1, 0, 0, 0);
  size_t before = 0;
  for (int t = 0; t < 6; ++t) {
    Eigen::Vector3d pos(0, t < 4 ? 0.0 : 8.8, 0);   // 22 of the map's 32 cells sideways
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr occ(new pcl::PointCloud<pcl::PointXYZRGB>), fr(new pcl::PointCloud<pcl::PointXYZRGB>);
    map.update(depth, seg, pos, q, occ, fr, false, 0.1 * t);
    if (!map.worldUpdate()) return 5;
    if (t == 3) before = map.worldOccupied(pts);
    std::printf("frame %d: %zu occupied voxels in the block, %zu archived\n", t, occ->size(), map.worldOccupied(pts));
  }
  if (!map.worldInfo(info) || info.n_updates != 6 || info.n_bricks == 0 || info.dropped_total != 0) return 6;
  const size_t n = map.worldOccupied(pts);
  std::printf("%u bricks, %zu archived obstacles (%zu before the move)\n", info.n_bricks, n, before);
  if (before == 0 || n < before || n != info.n_occupied) return 7;
  // the C ABI directly
  sdm_world_info ref_info;
  if (sdm_get_world_info(map.handle(), &ref_info) != SDM_OK || std::memcmp(&info, &ref_info, sizeof(info)) != 0) return 8;
  std::vector<sdm_point> ref(n + 2);
  int64_t got = 0;
  if (sdm_get_world_occupied(map.handle(), ref.data(), (int64_t)ref.size(), &got, 0u) != SDM_OK || got != (int64_t)n) return 9;
  if (std::memcmp(ref.data(), pts.data(), n * sizeof(sdm_point)) != 0) return 10;
  // every archived obstacle answers for itself at its cell's centre
  std::vector<Eigen::Vector3d> centres;
  for (const sdm_point &v : pts) centres.push_back(Eigen::Vector3d(v.x + 0.5 * p.voxel_size, v.y + 0.5 * p.voxel_size, v.z + 0.5 * p.voxel_size));
  if (map.queryWorld(centres, cells) != n) return 11;
  for (size_t i = 0; i < n; ++i)
    if (cells[i].track != pts[i].track || cells[i].label != pts[i].label || cells[i].occ != pts[i].occ || cells[i].stamp == 0) return 12;
  // ... and some of them lie outside the block now, where the map itself says nothing
  sdm_ring_state ring;
  if (sdm_get_ring_state(map.handle(), &ring) != SDM_OK) return 13;
  size_t outside = 0, wall = 0;
  for (const sdm_point &v : pts) {
    const float y0 = (float)(ring.moved_steps[1] - 16) * p.voxel_size, y1 = (float)(ring.moved_steps[1] + 16) * p.voxel_size;
    outside += v.y < y0 - 0.01f || v.y > y1 - 0.01f;
    wall += v.label == 6;
  }
  std::printf("%zu of them outside the block, %zu on the wall\n", outside, wall);
  if (outside == 0 || wall == 0) return 14;
  std::vector<sdm_world_cell> far;
  if (map.queryWorld({Eigen::Vector3d(100.0, 100.0, 100.0)}, far) != 1 || far[0].occ != -1 || far[0].stamp != 0) return 15;
  std::printf("world ok\n");
  return 0;
}
