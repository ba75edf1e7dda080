// SemanticDSPMap::scoreViews (include/semantic_dsp_map.h, "additions") on the wall scene of tests/cpp/adapter_frontiers.cpp:
// a wall with one movable object in front of it, seen from two places, driven through update().  Built against
// tests/mock_includes and linked with libsdm_hip.so.  Without an argument: construction only (no device needed).  With
// `run`: exit code 0 = the adapter's gains are the bytes the C ABI gives when called directly with the table the adapter
// built, that table is the pinhole table of the preset, a view towards the wall ends rays on it, and one turned away
// from it sees more unknown cells.
#include <cstdio>
#include <cstring>
#include <vector>

#include "semantic_dsp_map.h"

static sdm_view view_at(float x, float y, float z, float qw, float qy, float range) {
  sdm_view v;
  v.pos[0] = x;
  v.pos[1] = y;
  v.pos[2] = z;
  v.q[0] = qw;
  v.q[1] = 0.f;
  v.q[2] = qy;
  v.q[3] = 0.f;
  v.range = range;
  return v;
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
  const int stride = 8;
  std::vector<sdm_view> views;
  views.push_back(view_at(0.f, 4.4f, 0.f, 1.f, 0.f, 5.f));              // where the camera last stood, towards the wall
  views.push_back(view_at(0.f, 4.4f, 0.f, 0.f, 1.f, 5.f));              // turned round about y: away from it
  views.push_back(view_at(0.3f, 2.0f, 0.5f, 0.9238795f, 0.3826834f, 3.f));  // 45 degrees, between the two camera positions
  views.push_back(view_at(100.f, 0.f, 0.f, 1.f, 0.f, 5.f));             // far outside the map
  std::vector<sdm_view_gain> gains, ref;
  // the table: rows first, every stride-th pixel, ((u - cx) / fx, (v - cy) / fy, 1)
  const std::vector<float> &rays = map.viewRays(stride);
  const size_t n_rays = (size_t)((p.height + stride - 1) / stride) * (size_t)((p.width + stride - 1) / stride);
  if (rays.size() != 3 * n_rays) return 2;
  const size_t k = 3 * ((size_t)2 * (size_t)((p.width + stride - 1) / stride) + 5);  // row 2, column 5: pixel (40, 16)
  if (rays[k] != (40.f - p.cx) / p.fx || rays[k + 1] != (16.f - p.cy) / p.fy || rays[k + 2] != 1.f) return 3;
  if (!run) {
    if (map.scoreViews(views, stride, gains) != 0 || !gains.empty()) return 4;  // no map yet: nothing scored, no call into the library
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
  if (map.scoreViews(views, stride, gains) != views.size() || gains.size() != views.size()) return 5;
  ref.resize(views.size());
  if (sdm_query_views(map.handle(), views.data(), (int64_t)views.size(), rays.data(), (int32_t)n_rays, ref.data(), nullptr, nullptr, 0u) != SDM_OK)
    return 6;
  if (std::memcmp(gains.data(), ref.data(), gains.size() * sizeof(sdm_view_gain)) != 0) return 7;
  for (size_t i = 0; i < gains.size(); ++i)
    std::printf("view %zu: %u unknown, %u free, %u occupied cells; %u of %u rays end on an obstacle; %llu cells walked\n", i, gains[i].n_unknown,
                gains[i].n_free, gains[i].n_occupied, gains[i].rays_hit, gains[i].rays_in_map, (unsigned long long)gains[i].ray_cells);
  if (gains[0].rays_in_map != n_rays || gains[0].rays_hit < n_rays / 2 || gains[0].n_occupied == 0 || gains[0].n_free == 0) return 8;
  if (gains[1].rays_in_map != n_rays || gains[1].n_unknown <= gains[0].n_unknown) return 9;  // nobody has looked that way
  if (gains[3].rays_in_map != 0 || gains[3].ray_cells != 0 || gains[3].n_unknown != 0) return 10;
  for (const auto &g : gains)
    if (g.pad != 0 || g.n_occupied > g.rays_hit || (uint64_t)g.n_unknown + g.n_free + g.n_occupied > g.ray_cells) return 11;
  // another stride: another table, fewer rays, and the first one again
  std::vector<sdm_view_gain> coarse, again;
  if (map.scoreViews(views, 16, coarse) != views.size() || coarse[0].rays_in_map >= gains[0].rays_in_map) return 12;
  if (map.scoreViews(views, stride, again) != views.size() || std::memcmp(again.data(), gains.data(), gains.size() * sizeof(sdm_view_gain)) != 0)
    return 13;
  std::printf("views ok\n");
  return 0;
}
