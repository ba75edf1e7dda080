// SemanticDSPMap::forecast and ::checkTrajectory (include/semantic_dsp_map.h, "additions") on the wall scene of
// tests/cpp/adapter_views.cpp: a wall with one movable object in front of it, driven through update().  Built against
// tests/mock_includes and linked with libsdm_hip.so.  Without an argument: construction only (no device needed).  With
// `run`: exit code 0 = with explicit motions the object's cells are sources that arrive one cell further at the first
// horizon and the field's counters add up; a trajectory through the place the object moves into is blocked by the
// prediction, with the bytes the C ABI gives when called directly, and is free without motions; the built-in object
// layer reports no motion while the object rests and, once it moves, the object's track with the velocity
// sdm_objects_query gives, and the marks of that build lie where the velocity points.
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
  const std::vector<float> horizons{0.5f, 1.f, 2.f};
  sdm_motion car_motion;
  car_motion.track = 2;
  car_motion.pad = 0;
  car_motion.v[0] = 0.f, car_motion.v[1] = 0.f, car_motion.v[2] = -0.8f;  // towards the camera: one cell at 0.5 s, two at 1 s, four at 2 s
  std::vector<sdm_forecast_hit> hits;
  std::vector<Eigen::Vector3d> way{Eigen::Vector3d(-2.0, 0, 0.6), Eigen::Vector3d(2.0, 0.1, 0.62)};  // across, 0.6 m ahead of the camera
  std::vector<double> when{1.2, 1.9};
  if (!run) {
    if (map.forecast(horizons) != 0 || map.forecast({car_motion}, horizons, true) != 0) return 4;  // no map yet
    if (map.checkTrajectory(way, when, hits) != 0 || !hits.empty()) return 4;
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
  Eigen::Vector3d pos(0, 0, 0);
  for (int t = 0; t < 4; ++t) {
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr occ(new pcl::PointCloud<pcl::PointXYZRGB>), fr(new pcl::PointCloud<pcl::PointXYZRGB>);
    map.update(depth, seg, pos, q, occ, fr, false, 0.1 * t);
    std::printf("frame %d: %zu occupied voxels\n", t, occ->size());
  }
  // explicit motions
  if (map.forecast({car_motion}, horizons, false) != 1) return 5;
  const size_t V = (size_t)1 << 15;
  std::vector<uint32_t> mask(V), first(V);
  sdm_forecast_info info;
  if (sdm_get_forecast(map.handle(), mask.data(), first.data(), &info, nullptr) != SDM_OK) return 6;
  std::printf("field: %u sources, %u marked cells, %llu marks inside, %llu outside, %u stamps\n", info.n_sources, info.n_marked,
              (unsigned long long)info.n_marks_in, (unsigned long long)info.n_marks_out, info.n_stamps);
  if (info.n_motions != 1 || info.n_horizons != 3 || info.n_stamps != 3 || info.flags != 0u || info.n_sources < 4) return 7;
  if (info.n_marks_in + info.n_marks_out != 3ull * info.n_sources || info.n_marked < info.n_sources) return 8;
  size_t moved = 0;
  for (size_t c = 0; c < V; ++c) {
    if (((mask[c] >> 16) & 3u) != 3u) continue;
    const size_t z = c >> 10;  // one cell towards the camera at horizon 0, two at horizon 1, four at horizon 2
    if (z >= 4 && (!(mask[c - (1u << 10)] & 1u) || !(mask[c - (2u << 10)] & 2u) || !(mask[c - (4u << 10)] & 4u))) return 9;
    if (z >= 4 && (first[c - (4u << 10)] & 0xffffu) != 2u) return 10;
    ++moved;
  }
  if (moved != info.n_sources) return 11;
  // a trajectory across the cells the object sweeps between 1 s and 2 s (three and four cells from where it is: swept,
  // whichever of the two cell layers round 2 m its cells are in): blocked by the prediction; the C ABI says the same
  if (map.forecast({car_motion}, horizons, true) != 1) return 12;
  if (sdm_get_forecast(map.handle(), nullptr, nullptr, &info, nullptr) != SDM_OK || info.n_stamps != 4 || info.flags != SDM_FORECAST_SWEPT) return 12;
  if (map.checkTrajectory(way, when, hits) != 1 || hits.size() != 1) return 12;
  const float leg[8] = {-2.0f, 0.f, 0.6f, 1.2f, 2.0f, 0.1f, 0.62f, 1.9f};
  sdm_forecast_hit ref;
  if (sdm_query_forecast_segments(map.handle(), leg, 1, &ref, 0u) != SDM_OK) return 13;
  if (std::memcmp(&hits[0], &ref, sizeof(ref)) != 0) return 14;
  std::printf("leg: t %.3f, cell %u, %d cells, track %u, state %d, horizon %u\n", hits[0].t, hits[0].cell, hits[0].cells, hits[0].track,
              hits[0].state, hits[0].horizon);
  if (hits[0].state != 2 || hits[0].track != 2 || hits[0].horizon != 2 || !(hits[0].t > 0.f && hits[0].t < 1.f)) return 15;
  // the same way before the object is there, and without motions at all: free
  std::vector<double> early{0.0, 0.2};
  if (map.checkTrajectory(way, early, hits) != 1 || hits[0].state != 0 || hits[0].t != -1.f || hits[0].cell != 0xffffffffu) return 16;
  if (map.forecast(std::vector<sdm_motion>(), horizons, false) != 1 || map.checkTrajectory(way, when, hits) != 1 || hits[0].t != -1.f) return 17;
  if (map.checkTrajectory(way, std::vector<double>{1.0}, hits) != 0) return 18;  // not one time per waypoint
  // the built-in object layer's motions.  The object has been at rest (and came with four key points, too few for the
  // layer to estimate a motion from): none
  std::vector<sdm_motion> used;
  if (map.forecast(horizons, true, &used) != 1 || !used.empty()) return 19;
  if (sdm_get_forecast(map.handle(), nullptr, nullptr, &info, nullptr) != SDM_OK || info.n_motions != 0 || info.flags != SDM_FORECAST_SWEPT) return 20;
  // now it moves: 0.15 m along +x per frame of 0.1 s, six matched key points, mask and depth following it.  After a few
  // frames the layer holds it for moving and predicts it, and motions() must say so with the layer's own velocity
  auto key_points = [](double x) {
    return std::vector<Eigen::Vector3d>{Eigen::Vector3d(x - 0.3, -0.2, 2),  Eigen::Vector3d(x + 0.3, -0.2, 2), Eigen::Vector3d(x - 0.3, 0.3, 2),
                                        Eigen::Vector3d(x + 0.3, 0.3, 2),   Eigen::Vector3d(x, 0.05, 2.1),     Eigen::Vector3d(x + 0.1, -0.1, 2.05)};
  };
  for (int t = 4; t < 11; ++t) {
    const double x = 0.15 * (t - 3), x_before = 0.15 * (t - 4);
    const int shift = (int)(40.0 * x);  // fx * x / depth
    for (int i = 0; i < p.height; ++i)
      for (int j = 0; j < p.width; ++j) {
        const bool on_car = i >= 20 && i < 60 && j >= 40 + shift && j < 90 + shift;
        depth.at<float>(i, j) = on_car ? 2.0f : 3.0f;
        seg[1].mask.at<uchar>(i, j) = on_car ? 255 : 0;
      }
    seg[1].bbox = BBox2D{40 + shift, 20, 90 + shift, 60};
    seg[1].kpts_current = key_points(x);
    seg[1].kpts_previous = key_points(x_before);
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr occ(new pcl::PointCloud<pcl::PointXYZRGB>), fr(new pcl::PointCloud<pcl::PointXYZRGB>);
    map.update(depth, seg, pos, q, occ, fr, false, 0.1 * t);
  }
  if (!map.builtinObjectLayer()) return 21;
  sdm_object_info oi;
  if (sdm_objects_query(map.builtinObjectLayer()->handle(), 2, &oi) != SDM_OK) return 22;
  std::printf("object 2: exists %d, moving %d, prediction %d, v %.3f %.3f %.3f\n", oi.exists, oi.moving, oi.prediction_available,
              oi.translation_velocity[0], oi.translation_velocity[1], oi.translation_velocity[2]);
  if (!oi.exists || !oi.moving || !oi.prediction_available || !(oi.translation_velocity[0] > 0.5)) return 23;
  if (map.forecast(horizons, false, &used) != 1) return 24;
  if (used.size() != 1 || used[0].track != 2 || used[0].pad != 0) return 25;  // the static track and tracks without particles: not among them
  for (int a = 0; a < 3; ++a)
    if (used[0].v[a] != (float)oi.translation_velocity[a]) return 26;
  if (sdm_get_forecast(map.handle(), mask.data(), first.data(), &info, nullptr) != SDM_OK) return 27;
  std::printf("moving: %u sources, %u marked cells, %llu marks inside\n", info.n_sources, info.n_marked, (unsigned long long)info.n_marks_in);
  if (info.n_motions != 1 || info.n_stamps != 3 || info.flags != 0u || info.n_sources < 4 || info.n_marked < 4) return 28;
  // the marks of the first horizon lie where v points: their mean x is the sources' plus the shift of 0.5 s, in cells
  double src_x = 0, mark_x = 0;
  size_t n_src = 0, n_mark = 0;
  for (size_t c = 0; c < V; ++c) {
    if (((mask[c] >> 16) & 3u) == 3u) src_x += (double)(c & 31u), ++n_src;
    if (mask[c] & 1u) mark_x += (double)(c & 31u), ++n_mark;
  }
  const double want = std::nearbyint(((double)used[0].v[0] * 0.5) / (double)p.voxel_size);
  std::printf("mean x of the sources %.2f, of the first horizon's marks %.2f, shift %.0f cells\n", src_x / n_src, mark_x / n_mark, want);
  if (n_src != info.n_sources || n_mark == 0 || want < 1.0 || std::fabs(mark_x / n_mark - (src_x / n_src + want)) > 0.5) return 29;
  // without an object layer there are no motions, and the class builds from that as well
  map.setObjectLayer(nullptr);
  if (map.forecast(horizons, false, &used) != 1 || !used.empty()) return 30;
  std::printf("forecast ok\n");
  return 0;
}
