// SemanticDSPMap::frontiers (include/semantic_dsp_map.h, "additions") on a wall scene with one movable object in front of
// it, seen from two places, driven through update() like tests/cpp/adapter_instances.cpp.  Built against tests/mock_includes and linked with
// libsdm_hip.so.  Without an argument: construction only (no device needed).  With `run`: exit code 0 = the adapter's
// table is the one the C ABI gives when called directly - also where the adapter's first guess, the capacity of the
// vector it is handed, was too small -, it ascends by first cell, and with min_cells it is the subset of the large clusters.
#include <cstdio>
#include <cstring>
#include <vector>

#include "semantic_dsp_map.h"

static bool same(const std::vector<sdm_frontier_cluster> &a, const std::vector<sdm_frontier_cluster> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(sdm_frontier_cluster)) == 0);
}

// the table by the C ABI alone
static bool direct(sdm_map *m, uint32_t flags, int32_t min_cells, std::vector<sdm_frontier_cluster> &out, float origin[3]) {
  if (sdm_frontiers_update(m, flags, min_cells, 0) != SDM_OK) return false;
  int32_t n = 0;
  if (sdm_get_frontier_clusters(m, nullptr, 0, &n, origin) != SDM_OK) return false;
  out.resize((size_t)n);
  return n == 0 || sdm_get_frontier_clusters(m, out.data(), n, &n, origin) == SDM_OK;
}

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
  std::vector<sdm_frontier_cluster> all, large, ref;
  if (!run) {
    if (map.frontiers(all) != 0 || !all.empty()) return 2;  // no map yet: an empty table, no call into the library
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
  Eigen::Vector3d pos(0, 0, 0);
  Eigen::Quaterniond q(1, 0, 0, 0);
  for (int t = 0; t < 4; ++t) {
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr occ(new pcl::PointCloud<pcl::PointXYZRGB>), fr(new pcl::PointCloud<pcl::PointXYZRGB>);
    map.update(depth, seg, pos, q, occ, fr, false, 0.1 * t);
    std::printf("frame %d: %zu occupied voxels\n", t, occ->size());
  }
  // a second look from 4.4 m further along y: the ring follows the camera by eleven cells, the first frustum (four cells
  // up and down at the wall) stays inside the map, and two cells that nobody saw lie between the two: two frontiers
  pos = Eigen::Vector3d(0, 4.4, 0);
  for (int t = 4; t < 6; ++t) {
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr occ(new pcl::PointCloud<pcl::PointXYZRGB>), fr(new pcl::PointCloud<pcl::PointXYZRGB>);
    map.update(depth, seg, pos, q, occ, fr, false, 0.1 * t);
    std::printf("frame %d: %zu occupied voxels\n", t, occ->size());
  }
  float origin[3] = {0, 0, 0}, origin_ref[3] = {1, 1, 1};
  const size_t n_all = map.frontiers(all, 1, origin);
  if (!direct(map.handle(), 0u, 1, ref, origin_ref)) return 3;
  size_t cells = 0;
  for (size_t i = 0; i < all.size(); ++i) {
    cells += all[i].n_cells;
    if (i && all[i].first_cell <= all[i - 1].first_cell) return 4;  // ascending
    if (all[i].n_cells == 0 || all[i].n_unknown_faces < all[i].n_cells) return 5;
  }
  for (const auto &e : all)
    std::printf("cluster at cell %u: %u cells, box %u..%u %u..%u %u..%u\n", e.first_cell, e.n_cells, e.cell_min[0], e.cell_max[0], e.cell_min[1],
                e.cell_max[1], e.cell_min[2], e.cell_max[2]);
  int64_t n_cells = 0;
  if (sdm_get_frontier_cells(map.handle(), nullptr, nullptr, nullptr, 0, &n_cells) != SDM_OK) return 6;
  std::printf("%zu clusters, %zu cells (%lld in the list), origin %.2f %.2f %.2f\n", n_all, cells, (long long)n_cells, origin[0], origin[1],
              origin[2]);
  if (n_all != all.size() || n_all < 1 || cells < 50 || (int64_t)cells != n_cells) return 7;
  if (!same(all, ref) || std::memcmp(origin, origin_ref, sizeof(origin)) != 0) return 8;
  // min_cells: the subset of the large clusters, in the same order
  const int big = 8;
  map.frontiers(large, big);
  size_t k = 0;
  for (const auto &e : all)
    if (e.n_cells >= (uint32_t)big) {
      if (k >= large.size() || large[k].first_cell != e.first_cell || large[k].n_cells != e.n_cells) return 9;
      ++k;
    }
  if (k != large.size()) return 10;
  // a vector whose capacity - the adapter's first guess - is too small for the table: asked again with the count
  std::vector<sdm_frontier_cluster> small;
  small.reserve(1);
  if (all.size() < 2) return 11;
  if (map.frontiers(small) != all.size() || !same(small, all)) return 12;
  std::printf("frontiers ok\n");
  return 0;
}
