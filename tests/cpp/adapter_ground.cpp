// SemanticDSPMap::ground / checkFootprints (include/semantic_dsp_map.h, "additions") on the wall scene of
// tests/cpp/adapter_views.cpp: a wall with one movable object in front of it, driven through update().  The camera looks
// along +z at the wall, so with the up axis (2, -1) the wall is a floor seen from above and the object stands on it.  Built
// against tests/mock_includes and linked with libsdm_hip.so.  Without an argument: construction only (no device needed).
// With `run`: exit code 0 = the adapter's vectors are the bytes the C ABI gives when called directly, the wall carries
// ground columns with the clearance asked for towards the camera, the object's columns are lethal unless movable cells are
// ignored, and a footprint on the object is refused where one beside it is not.
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
  sdm_ground_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.up_axis = 2;
  opt.up_sign = -1;
  opt.h_lo = 0;
  opt.h_hi = 31;
  opt.clearance = 1;
  opt.max_step = 1;
  opt.support_labels[0] = 1u << 6;  // Building: the wall
  std::vector<sdm_ground_cell> cells, ref_cells;
  std::vector<uint32_t> d2, ref_d2;
  std::vector<sdm_footprint> fps;
  std::vector<sdm_footprint_result> got, ref;
  sdm_ground_info info, ref_info;
  if (!run) {
    fps.push_back(sdm_footprint{0.f, 0.f, 1.f, 0.f, 0.4f, 0.4f});
    if (map.ground(opt, cells, d2, &info) != 0 || !cells.empty() || !d2.empty()) return 4;  // no map yet
    if (map.checkFootprints(fps, got) != 0 || !got.empty()) return 4;
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
  const size_t n_cols = 32 * 32;
  if (map.ground(opt, cells, d2, &info) != n_cols || cells.size() != n_cols || d2.size() != n_cols) return 5;
  // the C ABI directly, on the layer the adapter has just built
  ref_cells.resize(n_cols);
  ref_d2.resize(n_cols);
  float origin[3];
  if (sdm_get_ground(map.handle(), ref_cells.data(), ref_d2.data(), &ref_info, origin) != SDM_OK) return 6;
  if (std::memcmp(cells.data(), ref_cells.data(), n_cols * sizeof(sdm_ground_cell)) != 0 || std::memcmp(d2.data(), ref_d2.data(), n_cols * 4) != 0 ||
      std::memcmp(&info, &ref_info, sizeof(info)) != 0)
    return 7;
  std::printf("grid %u x %u (axes %u, %u): %u ground, %u obstacle, %u none, %u step, %u lethal, levels %u..%u\n", info.n_u, info.n_v, info.axis_u,
              info.axis_v, info.n_ground, info.n_obstacle, info.n_none, info.n_step, info.n_lethal, info.level_min, info.level_max);
  if (info.n_u != 32 || info.n_v != 32 || info.axis_u != 0 || info.axis_v != 1 || info.n_ground + info.n_obstacle + info.n_none != n_cols) return 8;
  if (info.n_ground < 20 || info.n_lethal < 4 || std::memcmp(&info.options, &opt, sizeof(opt)) != 0) return 9;
  // the camera's column (x = 0, y = 4.4 m) looks at the object: lethal there; a column of the wall beside the object: ground
  const float centre_u = 0.f, centre_v = 4.4f;
  const float pts[6] = {centre_u, centre_v, 0.f, centre_u + 1.6f, centre_v, 0.f};
  sdm_ground_result at[2];
  if (sdm_query_ground(map.handle(), pts, 2, at, 0u) != SDM_OK) return 10;
  for (int k = 0; k < 2; ++k)
    std::printf("point %d: col %u, level %u, top %u, label %u, cls %u, headroom %u, d2 %u, surface %.2f, above %d\n", k, at[k].col, at[k].cell.level,
                at[k].cell.top, at[k].cell.label, at[k].cell.cls, at[k].cell.headroom, at[k].d2, at[k].surface, at[k].above);
  if (at[0].status != 0 || !(at[0].cell.cls & 8u) || at[0].d2 != 0) return 11;
  if (at[1].status != 0 || (at[1].cell.cls & 3u) != 1u || at[1].cell.label != 6 || at[1].cell.headroom < opt.clearance || at[1].above <= 0) return 12;
  if (std::memcmp(&at[1].cell, &cells[at[1].col], sizeof(sdm_ground_cell)) != 0 || at[1].d2 != d2[at[1].col]) return 13;
  fps.push_back(sdm_footprint{centre_u, centre_v, 1.f, 0.f, 0.6f, 0.4f});          // on the object
  fps.push_back(sdm_footprint{centre_u + 1.6f, centre_v, 0.f, 1.f, 0.3f, 0.3f});   // beside it, on the wall
  fps.push_back(sdm_footprint{centre_u, centre_v, 1.f, 0.f, 100.f, 0.4f});         // too large: answers nothing
  if (map.checkFootprints(fps, got) != fps.size()) return 14;
  ref.resize(fps.size());
  if (sdm_query_footprints(map.handle(), fps.data(), (int64_t)fps.size(), ref.data(), 0u) != SDM_OK) return 15;
  if (std::memcmp(got.data(), ref.data(), got.size() * sizeof(sdm_footprint_result)) != 0) return 16;
  for (size_t i = 0; i < got.size(); ++i)
    std::printf("footprint %zu: %u columns, %u lethal, %u none, %u ground, levels %u..%u, min d2 %u, first lethal %u\n", i, got[i].n_cols,
                got[i].n_lethal, got[i].n_none, got[i].n_ground, got[i].level_min, got[i].level_max, got[i].min_d2, got[i].first_lethal);
  if (got[0].n_cols < 4 || got[0].n_lethal == 0 || got[0].min_d2 != 0 || got[0].first_lethal == 0xffffffffu) return 17;
  if (got[1].n_cols == 0 || got[1].n_lethal != 0 || got[1].n_ground != got[1].n_cols || got[1].min_d2 == 0 || got[1].first_lethal != 0xffffffffu) return 18;
  if (got[2].n_cols != 0 || got[2].level_min != 0xffff || got[2].min_d2 != 0xffffffffu) return 19;
  // the object's cells ignored: its columns are the wall's, nothing of the first build is left
  opt.flags = SDM_GROUND_IGNORE_MOVABLE;
  if (map.ground(opt, cells, d2, &info) != n_cols || info.options.flags != SDM_GROUND_IGNORE_MOVABLE) return 20;
  if (map.checkFootprints(fps, got) != fps.size() || got[0].n_lethal >= ref[0].n_lethal) return 21;
  std::printf("ground ok\n");
  return 0;
}
