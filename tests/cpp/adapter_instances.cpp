// SemanticDSPMap::instances (include/semantic_dsp_map.h, "additions") on a wall scene with one movable object in front of
// it, driven through update() like tests/cpp/adapter_smoke.cpp.  Built against tests/mock_includes and linked with
// libsdm_hip.so.  Without an argument: construction only (no device needed).  With `run`: exit code 0 = the table of all
// instances accounts for every occupied voxel, ascends by track, and the movable-only table is its movable subset and
// holds the object.
#include <cstdio>
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
  std::vector<sdm_instance> all, movable;
  if (!run) {
    if (map.instances(all) != 0 || !all.empty()) return 2;  // no map yet: an empty table, no call into the library
    std::printf("adapter constructed\n");
    return 0;
  }
  const int movable_limit = 65523;  // the class's limit with the default label tables (utils/data_base.h:196)
  const int car_track = 2;
  cv::Mat depth(p.height, p.width, 4);
  MaskKpts st, car;
  st.track_id = 65535;
  st.label = "static";
  st.mask = cv::Mat(p.height, p.width, 1);
  car.track_id = car_track;
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
  Eigen::Vector3d pos(0, 0, 0);
  Eigen::Quaterniond q(1, 0, 0, 0);
  for (int t = 0; t < 4; ++t) {
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr occ(new pcl::PointCloud<pcl::PointXYZRGB>), fr(new pcl::PointCloud<pcl::PointXYZRGB>);
    map.update(depth, seg, pos, q, occ, fr, false, 0.1 * t);
    std::printf("frame %d: %zu occupied voxels\n", t, occ->size());
  }
  float origin[3] = {0, 0, 0};
  const size_t n_all = map.instances(all, false, origin);
  const size_t n_mov = map.instances(movable, true);
  std::vector<sdm_voxel_result> vox((size_t)1 << (p.x_n + p.y_n + p.z_n));
  if (sdm_get_voxels(map.handle(), vox.data()) != SDM_OK) return 3;
  size_t n_occ = 0;
  for (const auto &v : vox) n_occ += v.occ >= 1;
  size_t cells = 0;
  for (size_t i = 0; i < all.size(); ++i) {
    cells += all[i].n_cells;
    std::printf("track %u label %u: %u cells, centroid %.2f %.2f %.2f\n", all[i].track, all[i].label, all[i].n_cells, all[i].centroid[0],
                all[i].centroid[1], all[i].centroid[2]);
    if (i && all[i].track <= all[i - 1].track) return 4;  // ascending
    if (all[i].n_cells == 0) return 5;
  }
  std::printf("%zu instances (%zu movable), %zu cells, %zu occupied voxels, origin %.2f %.2f %.2f\n", n_all, n_mov, cells, n_occ, origin[0],
              origin[1], origin[2]);
  if (n_all != all.size() || n_mov != movable.size() || n_occ < 50 || cells != n_occ) return 6;
  // the movable-only table: the entries of the first with 1 <= track <= the limit, field for field
  size_t k = 0;
  bool has_car = false;
  for (const auto &e : all) {
    if (e.track < 1 || e.track > movable_limit) continue;
    if (k >= movable.size() || std::memcmp(&e, &movable[k], sizeof(e)) != 0) return 7;
    has_car = has_car || e.track == car_track;
    ++k;
  }
  if (k != movable.size()) return 8;
  if (!has_car) return 9;  // the object in front of the wall
  std::printf("instances ok\n");
  return 0;
}
