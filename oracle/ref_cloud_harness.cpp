/*
 * oracle/ref_cloud_harness.cpp - drives the reference's own PointCloudTools::generateLabeledPointCloud (and the
 * manualResize it calls in BOOST mode), compiled over the stand-in headers of oracle/ref_shims/, from a scenario file.
 *
 * TEST INFRASTRUCTURE ONLY.  utils/pointcloud_tools.h is included by path at build time (oracle/Makefile, target `ref`,
 * one executable per ref_variants/cloud_<variant>.sed); none of its text is in this file.  The build-time copy has lost
 * the members that need PCL or cv::ml (ref_cloud_members.sed); the two functions under test are compiled as they stand.
 * The function reads one constant of mc_ring/buffer.h, the largest of the three axis exponents; this translation unit
 * leaves mc_ring/ out, so that constant is defined below from the numbers of settings/settings.h.
 *
 *   ref_cloud_harness <scenario> <result>
 *
 * Both files are text: whitespace-separated tokens, integers in decimal, every float as the 8 hex digits of its
 * binary32 pattern, every double as the 16 hex digits of its binary64 pattern.  oracle/ref_cloud.py writes the one and
 * reads the other.  Scenario:
 *   noise flag first zero          setFlagConsiderDepthNoise(flag); the two coefficients handed to the function
 *   pose px py pz qw qx qy qz      updateCameraPose, doubles
 *   depth rows cols runs (n v)*    the depth image at sensor size, run-length coded floats
 *   entries n, then n x            the vector of MaskKpts, in this order
 *     track label kpts (x y z)* rows cols runs (n v)*     label is a word ("static": the static mask), v a byte
 * One process runs one scenario: the label tables are globals that the function grows by default insertion.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "settings/settings.h"
const uint32_t C_VOXEL_NUM_AXIS_N_BIGGEST = std::max({C_VOXEL_NUM_AXIS_X_N, C_VOXEL_NUM_AXIS_Y_N, C_VOXEL_NUM_AXIS_Z_N});
#include "utils/pointcloud_tools.h"

namespace {

FILE *in = nullptr, *out = nullptr;

[[noreturn]] void die(const char *what) {
  std::fprintf(stderr, "ref_cloud_harness: %s\n", what);
  std::exit(2);
}
long rd_int() {
  long v;
  if (std::fscanf(in, "%ld", &v) != 1) die("integer expected");
  return v;
}
float rd_f() {
  unsigned u;
  if (std::fscanf(in, "%x", &u) != 1) die("float pattern expected");
  float f;
  uint32_t w = u;
  std::memcpy(&f, &w, 4);
  return f;
}
double rd_d() {
  unsigned long long u;
  if (std::fscanf(in, "%llx", &u) != 1) die("double pattern expected");
  double d;
  uint64_t w = u;
  std::memcpy(&d, &w, 8);
  return d;
}
void expect(const char *word) {
  char got[64];
  if (std::fscanf(in, "%63s", got) != 1 || std::strcmp(got, word) != 0) die(word);
}
void wr_f(float f) {
  uint32_t w;
  std::memcpy(&w, &f, 4);
  std::fprintf(out, " %08x", w);
}

// rows cols runs (n v)*
template <class T, class Read> cv::Mat rd_image(int type, Read read) {
  long rows = rd_int(), cols = rd_int(), runs = rd_int(), at = 0;
  if (rows <= 0 || cols <= 0 || rows > 4096 || cols > 4096) die("image size");
  cv::Mat m(int(rows), int(cols), type);
  for (long r = 0; r < runs; ++r) {
    long n = rd_int();
    T v = read();
    for (long i = 0; i < n; ++i, ++at) {
      if (at >= rows * cols) die("image too long");
      m.at<T>(int(at / cols), int(at % cols)) = v;
    }
  }
  if (at != rows * cols) die("image too short");
  return m;
}

#if BOOST_MODE == 1
const float rescale = g_image_rescale;
#else
const float rescale = 1.f;
#endif

// what a lookup with default insertion would answer, without inserting
template <class M, class K> typename M::mapped_type peek(const M &m, const K &k) {
  auto it = m.find(k);
  return it == m.end() ? typename M::mapped_type() : it->second;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) die("usage: ref_cloud_harness <scenario> <result>");
  in = std::fopen(argv[1], "r");
  out = std::fopen(argv[2], "w");
  if (!in || !out) die("cannot open files");

  // ---- the configuration, before the run grows the tables
  std::fprintf(out, "variant %d %d %d %d %d\n", SETTING, BOOST_MODE, g_consider_instance ? 1 : 0, g_image_width, g_image_height);
  std::fprintf(out, "camera");
  wr_f(g_camera_fx), wr_f(g_camera_fy), wr_f(g_camera_cx), wr_f(g_camera_cy), wr_f(g_depth_range_min), wr_f(g_depth_range_max), wr_f(rescale);
  std::fprintf(out, "\nmax_movable %d\n", g_max_movable_object_instance_id);
  std::fprintf(out, "sky %d\n", g_label_to_instance_id_map_default.count("Sky") ? g_label_to_instance_id_map_default.at("Sky") : -1);
  std::fprintf(out, "label_to_instance 257");  // :137-138, g_label_to_instance_id_map_default[g_label_id_map_reversed[label]]
  for (int l = 0; l <= 256; ++l) std::fprintf(out, " %d", peek(g_label_to_instance_id_map_default, peek(g_label_id_map_reversed, l)));
  std::fprintf(out, "\n");
  {
    std::map<int, int> t;  // :279, g_label_id_map_static[g_instance_id_to_label_map_default[instance]]
    for (const auto &kv : g_instance_id_to_label_map_default) t[kv.first] = peek(g_label_id_map_static, kv.second);
    std::fprintf(out, "instance_to_label %zu", t.size());
    for (const auto &kv : t) std::fprintf(out, " %d %d", kv.first, kv.second);
    std::fprintf(out, "\n");
  }

  // ---- the scenario
  expect("noise");
  const long noise_flag = rd_int();
  const float first_order = rd_f(), zero_order = rd_f();
  expect("pose");
  Eigen::Vector3d pos;
  pos[0] = rd_d(), pos[1] = rd_d(), pos[2] = rd_d();
  const double qw = rd_d(), qx = rd_d(), qy = rd_d(), qz = rd_d();
  expect("depth");
  cv::Mat depth = rd_image<float>(CV_32FC1, rd_f);
  expect("entries");
  const long n_entries = rd_int();
  std::vector<MaskKpts> seg(n_entries);
  std::fprintf(out, "entry_labels %ld", n_entries);  // :168, g_label_id_map_default[label]; -1: no such name (the lookup inserts 0)
  for (long e = 0; e < n_entries; ++e) {
    MaskKpts &s = seg[e];
    s.track_id = int(rd_int());
    char word[64];
    if (std::fscanf(in, "%63s", word) != 1) die("label expected");
    s.label = word;
    const long nk = rd_int();
    for (long k = 0; k < nk; ++k) {
      Eigen::Vector3d p;
      p[0] = rd_d(), p[1] = rd_d(), p[2] = rd_d();
      s.kpts_current.push_back(p);
    }
    s.mask = rd_image<uchar>(CV_8UC1, [] { return uchar(rd_int()); });
    s.bbox = BBox2D{0, 0, 0, 0};
    std::fprintf(out, " %d", g_label_id_map_default.count(s.label) ? g_label_id_map_default.at(s.label) : -1);
  }
  std::fprintf(out, "\n");
  if (int(depth.rows * rescale) != g_image_height || int(depth.cols * rescale) != g_image_width) die("the depth image does not have the sensor's size");

  // ---- the run
  PointCloudTools tools;
  tools.updateCameraPose(pos, Eigen::Quaterniond(qw, qx, qy, qz));
  setFlagConsiderDepthNoise(noise_flag != 0);
  std::vector<std::vector<LabeledPoint>> cloud(g_image_height, std::vector<LabeledPoint>(g_image_width));
  std::unordered_map<uint16_t, std::vector<Eigen::Vector3d>> tracked_objects_points;
  std::unordered_map<int, int> track_to_label_id_map;
  const int rc = tools.generateLabeledPointCloud(depth, seg, cloud, tracked_objects_points, track_to_label_id_map, first_order, zero_order);
  if (rc != 0) die("generateLabeledPointCloud failed");
  if (depth.rows != g_image_height || depth.cols != g_image_width) die("the depth image was not reduced to the configured size");

  // ---- the answer
  std::fprintf(out, "depth %d %d", depth.rows, depth.cols);
  for (int i = 0; i < depth.rows; ++i) for (int j = 0; j < depth.cols; ++j) wr_f(depth.at<float>(i, j));
  std::fprintf(out, "\n");
  // A point that the SETTING 3 box filter turned into Background (:254-272) has no sigma: the reference leaves it
  // unset, so printing it would print whatever the stack held.  Such a point is told from a genuine Background point
  // here, not by the reference: it has track 65535 and label 0, and either the frame has a static mask - whose values
  // name label ids of 1 and more, none of which is Background's - or one of the (by now reduced) object masks covers it.
  bool has_static = false;
  for (const MaskKpts &s : seg) has_static = has_static || s.label == "static";
  long n_valid = 0;
  for (const auto &row : cloud) for (const LabeledPoint &p : row) n_valid += p.is_valid ? 1 : 0;
  std::fprintf(out, "cloud %ld", n_valid);
  for (int i = 0; i < g_image_height; ++i)
    for (int j = 0; j < g_image_width; ++j) {
      const LabeledPoint &p = cloud[i][j];
      if (!p.is_valid) continue;
      bool clipped = false;
      if (SETTING == 3 && g_consider_instance && p.track_id == 65535 && p.label_id == 0) {
        clipped = has_static;
        for (const MaskKpts &s : seg)
          if (s.label != "static" && s.mask.at<uchar>(i, j) > 0) clipped = true;
      }
      std::fprintf(out, "\n %d", i * g_image_width + j);
      wr_f(p.position.x()), wr_f(p.position.y()), wr_f(p.position.z());
      if (clipped) std::fprintf(out, " --------");
      else wr_f(p.sigma);
      std::fprintf(out, " %u %u", unsigned(p.track_id), unsigned(p.label_id));
    }
  std::fprintf(out, "\n");
  {
    std::map<int, int> t(track_to_label_id_map.begin(), track_to_label_id_map.end());
    std::fprintf(out, "track_to_label %zu", t.size());
    for (const auto &kv : t) std::fprintf(out, " %d %d", kv.first, kv.second);
    std::fprintf(out, "\n");
  }
  {
    std::map<int, size_t> t;  // tracked_objects_points (:291-296): how many points each movable id collected
    for (const auto &kv : tracked_objects_points) t[kv.first] = kv.second.size();
    std::fprintf(out, "tracked_points %zu", t.size());
    for (const auto &kv : t) std::fprintf(out, " %d %zu", kv.first, kv.second);
    std::fprintf(out, "\n");
  }
  std::fprintf(out, "end\n");
  std::fclose(out);
  std::fclose(in);
  return 0;
}
