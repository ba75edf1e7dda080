// TEST INFRASTRUCTURE: the scene the world adapter programs (tests/cpp/adapter_world_*.cpp) share - a 32^3 grid of 0.4 m
// cells behind a 128 x 80 camera, and a wall 3 m ahead of it.
#pragma once
#include <vector>

#include "semantic_dsp_map.h"

static inline void preset(SemanticDSPMap &map, SdmGridPreset &p) {
  p = SdmGridPreset::VirtualKitti2();
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
}

// one frame of the wall 3 m ahead: creates the map
static inline void wall_frame(SemanticDSPMap &map, const SdmGridPreset &p, double t) {
  cv::Mat depth(p.height, p.width, 4);
  MaskKpts st;
  st.track_id = 65535;
  st.label = "static";
  st.mask = cv::Mat(p.height, p.width, 1);
  for (int i = 0; i < p.height; ++i)
    for (int j = 0; j < p.width; ++j) {
      depth.at<float>(i, j) = 3.0f;
      st.mask.at<uchar>(i, j) = 5;
    }
  std::vector<MaskKpts> seg{st};
  pcl::PointCloud<pcl::PointXYZRGB>::Ptr occ(new pcl::PointCloud<pcl::PointXYZRGB>), fr(new pcl::PointCloud<pcl::PointXYZRGB>);
  Eigen::Vector3d pos(0, 0, 0);
  Eigen::Quaterniond q(1, 0, 0, 0);
  map.update(depth, seg, pos, q, occ, fr, false, t);
}
