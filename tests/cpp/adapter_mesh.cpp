// SemanticDSPMap::mesh (include/semantic_dsp_map.h, "additions") on the wall scene of tests/cpp/adapter_ground.cpp: a wall
// with one movable object in front of it, driven through update().  Built against tests/mock_includes and linked with
// libsdm_hip.so.  Without an argument: construction only (no device needed).  With `run`: exit code 0 = the adapter's
// vectors are the bytes the C ABI gives when called directly, the triangles are the quads' two halves, a build with a tiny
// first capacity is repeated once with the true counts and gives the same mesh, and MOVABLE_ONLY leaves the object alone.
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
  sdm_mesh_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.track = -1;
  std::memset(opt.labels, 0xff, sizeof(opt.labels));
  opt.max_faces = 6 * 32 * 32 * 32;
  std::vector<float> xyz, xyz2;
  std::vector<uint32_t> tri, tri2;
  std::vector<sdm_mesh_face> faces, faces2;
  sdm_mesh_info info, info2, ref_info;
  if (!run) {
    xyz.push_back(1.f);
    tri.push_back(1u);
    faces.resize(1);
    if (map.mesh(opt, xyz, tri, &faces, &info) != 0 || !xyz.empty() || !tri.empty() || !faces.empty()) return 4;  // no map yet
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
  const size_t n_tri = map.mesh(opt, xyz, tri, &faces, &info);
  std::printf("%zu triangles, %u faces, %u vertices, %u solid cells\n", n_tri, info.n_faces, info.n_vertices, info.n_solid);
  if (n_tri == 0 || n_tri != 2 * (size_t)info.n_faces || tri.size() != 3 * n_tri || faces.size() != info.n_faces || xyz.size() != 3 * (size_t)info.n_vertices)
    return 5;
  if (info.n_solid < 20 || info.options.max_faces != opt.max_faces) return 6;
  // the C ABI directly, on the mesh the adapter has just built
  const size_t nf = info.n_faces, nv = info.n_vertices;
  std::vector<sdm_mesh_face> ref_faces(nf);
  std::vector<uint32_t> ref_quads(4 * nf);
  std::vector<float> ref_xyz(3 * nv);
  std::vector<sdm_mesh_vertex> ref_corners(nv);
  int64_t n = 0;
  float origin[3];
  if (sdm_get_mesh_info(map.handle(), &ref_info, origin) != SDM_OK || std::memcmp(&info, &ref_info, sizeof(info)) != 0) return 7;
  if (sdm_get_mesh_faces(map.handle(), ref_faces.data(), ref_quads.data(), (int64_t)nf, &n) != SDM_OK || n != (int64_t)nf) return 8;
  if (sdm_get_mesh_vertices(map.handle(), ref_corners.data(), ref_xyz.data(), (int64_t)nv, &n) != SDM_OK || n != (int64_t)nv) return 9;
  if (std::memcmp(faces.data(), ref_faces.data(), nf * sizeof(sdm_mesh_face)) != 0 || std::memcmp(xyz.data(), ref_xyz.data(), 12 * nv) != 0) return 10;
  for (size_t f = 0; f < nf; ++f) {
    const uint32_t *qd = &ref_quads[4 * f], *t = &tri[6 * f];
    if (t[0] != qd[0] || t[1] != qd[1] || t[2] != qd[2] || t[3] != qd[0] || t[4] != qd[2] || t[5] != qd[3]) return 11;
  }
  for (size_t v = 0; v < nv; ++v)
    for (int a = 0; a < 3; ++a) {
      const uint16_t c = a == 0 ? ref_corners[v].i : (a == 1 ? ref_corners[v].j : ref_corners[v].k);
      const float step = (float)c * p.voxel_size;
      if (xyz[3 * v + a] != origin[a] + step) return 12;
    }
  bool wall = false, object = false;
  for (size_t f = 0; f < nf; ++f) {
    wall = wall || (faces[f].label == 6 && faces[f].dir == 4 && faces[f].kind == 0);   // the wall's side towards the camera
    object = object || faces[f].track == 2;
  }
  if (!wall || !object) return 13;
  // a tiny first capacity: the build is repeated once with the true counts
  sdm_mesh_options tiny = opt;
  tiny.max_faces = 4;
  tiny.max_vertices = 4;
  if (map.mesh(tiny, xyz2, tri2, &faces2, &info2) != n_tri) return 14;
  if (info2.options.max_faces != (int64_t)nf || info2.options.max_vertices != (int64_t)nv) return 15;   // (what the second build asked for)
  if (xyz2 != xyz || tri2 != tri || std::memcmp(faces2.data(), faces.data(), nf * sizeof(sdm_mesh_face)) != 0) return 16;
  // the moving object alone
  opt.flags = SDM_MESH_MOVABLE_ONLY;
  const size_t n_obj = map.mesh(opt, xyz2, tri2, &faces2, &info2);
  std::printf("the object: %zu triangles, %u solid cells\n", n_obj, info2.n_solid);
  if (n_obj == 0 || n_obj >= n_tri || info2.n_solid >= info.n_solid) return 17;
  for (size_t f = 0; f < faces2.size(); ++f)
    if (faces2[f].track != 2) return 18;
  std::printf("mesh ok\n");
  return 0;
}
