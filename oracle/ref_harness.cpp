/*
 * oracle/ref_harness.cpp - drives the reference's own ring buffer (mc_ring/*.h over utils/data_base.h and
 * utils/basic_algorithms.h), compiled over the stand-in headers of oracle/ref_shims/, from a scenario file.
 *
 * TEST INFRASTRUCTURE ONLY.  The reference's headers are included by path at build time (oracle/Makefile, target
 * `ref`, one executable per variant of settings/settings.h); none of their text is in this file.  The reference keeps
 * its map in globals and in a function-static last position (operations.h:70), so one process runs one scenario:
 * a shifted ring is reached by `ego` commands from the origin and particles are loaded into PARTICLE_ARRAY after it.
 *
 *   ref_harness <scenario> <result>
 *
 * Both files are text: whitespace-separated tokens, integers in decimal, every float as the 8 hex digits of its
 * binary32 pattern.  oracle/ref_ring.py writes the one and reads the other; the commands are listed in main().
 */
#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <queue>
#include <string>
#include <vector>

#include "utils/data_base.h"
#include "utils/basic_algorithms.h"
#include "mc_ring/mt_operations.h"

namespace {

// what the harness needs of RingBufferOperations' protected part
class Probe : public MTRingBufferOperations {
 public:
  using RingBufferOperations::globalFramePostoVoxelIdx;
};

FILE *in = nullptr, *out = nullptr;

[[noreturn]] void die(const char *what) {
  std::fprintf(stderr, "ref_harness: %s\n", what);
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
void wr_f(float f) {
  uint32_t w;
  std::memcpy(&w, &f, 4);
  std::fprintf(out, " %08x", w);
}
Eigen::Matrix4f rd_mat4() {
  Eigen::Matrix4f m;
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m(r, c) = rd_f();
  return m;
}
Eigen::Matrix3f intrinsic() {  // as operations.h:1309-1310 builds it
  Eigen::Matrix3f k;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) k(r, c) = r == c ? 1.f : 0.f;
  k(0, 0) = g_camera_fx;
  k(1, 1) = g_camera_fy;
  k(0, 2) = g_camera_cx;
  k(1, 2) = g_camera_cy;
  return k;
}

std::vector<float> noise_table;
void fill_noise() {
  if (noise_table.empty()) return;
  for (int i = 0; i < GAUSSIAN_RANDOM_NUM; ++i) gaussian_randoms[i] = noise_table[i % noise_table.size()];
}

bool slot_is_cleared(uint32_t idx) {  // the state RingBufferOperations::clear() leaves, operations.h:701-722
  const Particle &p = PARTICLE_ARRAY[idx];
  const bool time_slot = (idx & (C_MAX_PARTICLE_NUM_PER_VOXEL - 1)) == 0;
  return p.status == (time_slot ? Particle_Status::TIMEPTC : Particle_Status::INVALID) && p.pos.x == 0.f && p.pos.y == 0.f &&
         p.pos.z == 0.f && p.pos.weight == 0.f && p.time_stamp == 0 && p.track_id == 0 && p.label_id == 0 && p.forget_count == 0 &&
         !std::signbit(p.pos.x) && !std::signbit(p.pos.y) && !std::signbit(p.pos.z) && !std::signbit(p.pos.weight);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) die("usage: ref_harness <scenario> <result>");
  in = std::fopen(argv[1], "r");
  out = std::fopen(argv[2], "w");
  if (!in || !out) die("cannot open files");

  static Probe op;  // constructs the ring: runSystemChecking + initialize, operations.h:44-49
  GaussianRandomCalculator calc;
  Eigen::Vector3f last_ego = Eigen::Vector3f::Zero();  // mirrors the function-static of operations.h:70
  std::fprintf(out, "variant %u %u %u %u %d %d\n", C_VOXEL_NUM_AXIS_X, C_VOXEL_NUM_AXIS_Y, C_VOXEL_NUM_AXIS_Z,
               unsigned(C_MAX_PARTICLE_NUM_PER_VOXEL), g_image_width, g_image_height);
  std::fprintf(out, "camera");
  wr_f(C_VOXEL_SIZE), wr_f(g_camera_fx), wr_f(g_camera_fy), wr_f(g_camera_cx), wr_f(g_camera_cy), wr_f(g_depth_range_min), wr_f(g_depth_range_max);
  std::fprintf(out, "\n");

  char cmd[64];
  while (std::fscanf(in, "%63s", cmd) == 1) {
    const std::string c(cmd);
    if (c == "noise") {  // noise n v...: gaussian_randoms[i] = v[i mod n], as the oracle's set_noise_table of the tiled table
      long n = rd_int();
      noise_table.resize(n);
      for (long i = 0; i < n; ++i) noise_table[i] = rd_f();
      fill_noise();
    } else if (c == "ts") {  // ts t: global_time_stamp = t (semantic_dsp_map.h:173 increments it once per frame)
      global_time_stamp = uint32_t(rd_int());
    } else if (c == "ego") {  // ego x y z: updateEgoCenterPos, operations.h:68-96
      Eigen::Vector3f p;
      p[0] = rd_f(), p[1] = rd_f(), p[2] = rd_f();
      op.updateEgoCenterPos(p);
      last_ego = p;
    } else if (c == "load") {  // load n, then n x (index x y z w ts track label status forget): written straight into PARTICLE_ARRAY
      long n = rd_int();
      for (long i = 0; i < n; ++i) {
        long idx = rd_int();
        if (idx < 0 || idx >= long(C_MAX_PARTICLE_NUM)) die("load: index out of range");
        Particle &p = PARTICLE_ARRAY[idx];
        p.pos.x = rd_f(), p.pos.y = rd_f(), p.pos.z = rd_f(), p.pos.weight = rd_f();
        p.time_stamp = uint16_t(rd_int());
        p.track_id = uint16_t(rd_int());
        p.label_id = uint16_t(rd_int());
        p.status = Particle_Status(uint8_t(rd_int()));
        p.forget_count = uint8_t(rd_int());
      }
    } else if (c == "pos_to_voxel") {  // globalFramePostoVoxelIdx, operations.h:841-883
      long n = rd_int();
      std::fprintf(out, "pos_to_voxel %ld", n);
      for (long i = 0; i < n; ++i) {
        ParticleBasicState s;
        s.x = rd_f(), s.y = rd_f(), s.z = rd_f(), s.weight = 0.f;
        uint32_t v;
        op.globalFramePostoVoxelIdx(s, v);
        std::fprintf(out, " %u", v);
      }
      std::fprintf(out, "\n");
    } else if (c == "voxel_to_pos") {  // getVoxelGlobalPosition, operations.h:645-648, 940-983
      long n = rd_int();
      std::fprintf(out, "voxel_to_pos %ld", n);
      for (long i = 0; i < n; ++i) {
        Eigen::Vector3f p;
        op.getVoxelGlobalPosition(uint32_t(rd_int()), p);
        wr_f(p[0]), wr_f(p[1]), wr_f(p[2]);
      }
      std::fprintf(out, "\n");
    } else if (c == "add") {  // add kind label track n points: addNewParticleWithSemantics (0) / addGuessedParticles (1), operations.h:171-205
      long kind = rd_int(), label = rd_int(), track = rd_int(), n = rd_int();
      std::fprintf(out, "add %ld", n);
      for (long i = 0; i < n; ++i) {
        Eigen::Vector3f p;
        p[0] = rd_f(), p[1] = rd_f(), p[2] = rd_f();
        uint32_t v = 0, pi = 0;
        if (kind == 0) op.addNewParticleWithSemantics(p, uint8_t(label), uint16_t(track), v, pi);
        else op.addGuessedParticles(p, uint8_t(label), uint16_t(track), v, pi);
        std::fprintf(out, " %u %u", v, pi);
      }
      std::fprintf(out, "\n");
    } else if (c == "move") {  // move k, then k x (16 matrix floats, n, n indices): moveParticlesInSetsByTransformations, operations.h:321-362
      long k = rd_int();
      std::vector<std::unordered_set<uint32_t>> sets(k), moved;
      std::vector<Eigen::Matrix4f> mats(k);
      for (long s = 0; s < k; ++s) {
        mats[s] = rd_mat4();
        long n = rd_int();
        for (long i = 0; i < n; ++i) sets[s].insert(uint32_t(rd_int()));
      }
      op.moveParticlesInSetsByTransformations(sets, mats, moved);
      std::fprintf(out, "move %zu", moved.size());
      for (auto &m : moved) {
        std::vector<uint32_t> v(m.begin(), m.end());
        std::sort(v.begin(), v.end());
        std::fprintf(out, " %zu", v.size());
        for (uint32_t i : v) std::fprintf(out, " %u", i);
      }
      std::fprintf(out, "\n");
    } else if (c == "delete") {  // delete n indices: deleteParticlesInSet, operations.h:216-221
      long n = rd_int();
      std::unordered_set<uint32_t> s;
      for (long i = 0; i < n; ++i) s.insert(uint32_t(rd_int()));
      op.deleteParticlesInSet(s);
    } else if (c == "visible") {  // visible form, 16 extrinsic floats, run-length depth image: (mt)UpdateVisibleParitlcesWithBFS
      long form = rd_int();
      Eigen::Matrix4f e = rd_mat4();
      cv::Mat depth(g_image_height, g_image_width);
      long runs = rd_int(), at = 0;
      for (long r = 0; r < runs; ++r) {
        long n = rd_int();
        float v = rd_f();
        for (long i = 0; i < n; ++i, ++at) {
          if (at >= long(g_image_height) * g_image_width) die("visible: depth image too long");
          depth.at<float>(int(at / g_image_width), int(at % g_image_width)) = v;
        }
      }
      if (at != long(g_image_height) * g_image_width) die("visible: depth image too short");
      // The BFS indexes its vertex grid with the start vertex unchecked (operations.h:1321-1335, mt_basic.h:60-66): outside
      // of it that is undefined behaviour, so the harness says so instead of running it.  The single-threaded form
      // starts 1 m down the optical axis, the two threads of the other form at depth_max / 1.26 and depth_max
      // (mt_operations.h:115-127).
      Eigen::Matrix4f inv = e.inverse().eval();
      bool inside = true;
      const uint32_t n_axis[3] = {C_VOXEL_NUM_AXIS_X, C_VOXEL_NUM_AXIS_Y, C_VOXEL_NUM_AXIS_Z};
      std::vector<float> start_z;
      if (form == 0) start_z = {1.f};
      else start_z = {float(g_depth_range_max / std::pow(1.26f, 1.f)), g_depth_range_max};
      for (float z : start_z)
        for (int a = 0; a < 3; ++a) {
          float s = ((inv(a, 2) * z + inv(a, 3)) - map_center_pos[a] + map_p_max_const[a]) * voxel_size_recip;
          if (!(s > -1.f && s < float(n_axis[a] + 1))) inside = false;
        }
      std::fprintf(out, "visible %d\n", inside ? 1 : 0);
      if (inside) {
        if (form == 0) op.updateVisibleParitlcesWithBFS(e, depth);  // the form the frame uses, semantic_dsp_map.h:749
        else op.mtUpdateVisibleParitlcesWithBFS(e, depth);
      }
    } else if (c == "frustum") {  // frustum 16 extrinsic floats, n points: checkIfPointInFrustum, operations.h:676-679, 1240-1258
      Eigen::Matrix4f e = rd_mat4();
      long n = rd_int();
      std::fprintf(out, "frustum %ld", n);
      for (long i = 0; i < n; ++i) {
        Eigen::Vector3f p;
        p[0] = rd_f(), p[1] = rd_f(), p[2] = rd_f();
        std::fprintf(out, " %d", op.checkIfPointInFrustum(p, e, intrinsic(), g_image_width, g_image_height) ? 1 : 0);
      }
      std::fprintf(out, "\n");
    } else if (c == "occupancy") {  // the frame's sweep, semantic_dsp_map.h:1244-1255: determineIfVoxelOccupied over every voxel
      float thr = rd_f();
      std::vector<uint32_t> rows;
      long unknown = 0;
      for (uint32_t i = 0; i < C_VOXEL_NUM_TOTAL; ++i) {
        uint16_t track_id = 0;  // locals the frame leaves uninitialised (semantic_dsp_map.h:1245-1246); 0 here
        uint8_t label_id = 0;
        int occ = op.determineIfVoxelOccupied(i, label_id, track_id, thr);
        if (occ < 0) { ++unknown; continue; }
        rows.push_back(i), rows.push_back(uint32_t(occ)), rows.push_back(label_id), rows.push_back(track_id);
      }
      std::fprintf(out, "occupancy %ld %zu", unknown, rows.size() / 4);
      for (uint32_t v : rows) std::fprintf(out, " %u", v);
      std::fprintf(out, "\n");
    } else if (c == "fusion") {  // fusion neighbours threshold n voxels: calculateWeightAndSemanticsInVoxel[ConsiderNeighbors], operations.h:390-600
      long nb = rd_int();
      float thr = rd_f();
      long n = rd_int();
      std::fprintf(out, "fusion %ld", n);
      for (long i = 0; i < n; ++i) {
        uint32_t v = uint32_t(rd_int());
        float wsum = 0.f, guessed = 0.f;
        uint8_t label = 0;
        uint16_t track = 0;
        if (nb) op.calculateWeightAndSemanticsInVoxelConsiderNeighbors(v, thr, wsum, guessed, label, track);
        else op.calculateWeightAndSemanticsInVoxel(v, wsum, guessed, label, track);
        wr_f(wsum), wr_f(guessed);
        std::fprintf(out, " %u %u", unsigned(label), unsigned(track));
      }
      std::fprintf(out, "\n");
    } else if (c == "pdf_table") {  // calculateGaussianTable, basic_algorithms.h:394-410; the random part is overwritten again
      calc.calculateGaussianTable(1.0);
      fill_noise();
      std::fprintf(out, "pdf_table %d", GAUSSIAN_PDF_NUM);
      for (int i = 0; i < GAUSSIAN_PDF_NUM; ++i) wr_f(standard_gaussian_pdf[i]);
      std::fprintf(out, "\n");
    } else if (c == "query_pdf") {  // query_pdf n x (x mu sigma): queryNormalPDF, basic_algorithms.h:417-422
      long n = rd_int();
      std::fprintf(out, "query_pdf %ld", n);
      for (long i = 0; i < n; ++i) {
        float x = rd_f(), mu = rd_f(), sigma = rd_f();
        wr_f(calc.queryNormalPDF(x, mu, sigma));
      }
      std::fprintf(out, "\n");
    } else if (c == "forgetting_factor") {  // forgetting_factor stability max n counts: getForgettingFactor, basic_algorithms.h:32-48
      float stability = rd_f();
      long max_count = rd_int(), n = rd_int();
      std::fprintf(out, "forgetting_factor %ld", n);
      for (long i = 0; i < n; ++i) wr_f(getForgettingFactor(int(rd_int()), stability, int(max_count)));
      std::fprintf(out, "\n");
    } else if (c == "dump_ring") {
      std::fprintf(out, "ring %u %d %d %d %d %d %d", global_time_stamp, buffer_moved_steps_x, buffer_moved_steps_y, buffer_moved_steps_z,
                   buffer_moved_equivalent_steps_x, buffer_moved_equivalent_steps_y, buffer_moved_equivalent_steps_z);
      for (int a = 0; a < 3; ++a) wr_f(map_center_pos[a]);
      for (int a = 0; a < 3; ++a) wr_f(last_ego[a]);
      std::fprintf(out, "\n");
    } else if (c == "dump_stamps") {
      std::fprintf(out, "stamps %u %u %u", C_VOXEL_NUM_AXIS_X, C_VOXEL_NUM_AXIS_Y, C_VOXEL_NUM_AXIS_Z);
      for (uint32_t i = 0; i < C_VOXEL_NUM_AXIS_X; ++i) std::fprintf(out, " %u", voxel_time_stamps_x[i]);
      for (uint32_t i = 0; i < C_VOXEL_NUM_AXIS_Y; ++i) std::fprintf(out, " %u", voxel_time_stamps_y[i]);
      for (uint32_t i = 0; i < C_VOXEL_NUM_AXIS_Z; ++i) std::fprintf(out, " %u", voxel_time_stamps_z[i]);
      std::fprintf(out, "\n");
    } else if (c == "dump_state") {  // every slot that is not as clear() leaves it
      long n = 0;
      for (uint32_t i = 0; i < C_MAX_PARTICLE_NUM; ++i) n += slot_is_cleared(i) ? 0 : 1;
      std::fprintf(out, "state %ld", n);
      for (uint32_t i = 0; i < C_MAX_PARTICLE_NUM; ++i) {
        if (slot_is_cleared(i)) continue;
        const Particle &p = PARTICLE_ARRAY[i];
        std::fprintf(out, "\n %u", i);
        wr_f(p.pos.x), wr_f(p.pos.y), wr_f(p.pos.z), wr_f(p.pos.weight);
        std::fprintf(out, " %u %u %u %u %u", unsigned(p.time_stamp), unsigned(p.track_id), unsigned(p.label_id), unsigned(p.status), unsigned(p.forget_count));
      }
      std::fprintf(out, "\n");
    } else if (c == "dump_bins") {  // per pixel with a count: id, count, the indices in the order they were pushed
      long npix = 0;
      for (int r = 0; r < g_image_height; ++r) for (int q = 0; q < g_image_width; ++q) npix += particle_to_pixel_num_array[r][q] ? 1 : 0;
      std::fprintf(out, "bins %ld", npix);
      for (int r = 0; r < g_image_height; ++r)
        for (int q = 0; q < g_image_width; ++q) {
          uint32_t n = particle_to_pixel_num_array[r][q];
          if (!n) continue;
          const uint32_t id = uint32_t(r) * g_image_width + q;
          const std::vector<uint32_t> &b = particle_to_pixel_index_map[id];
          if (b.size() != n) die("dump_bins: count and list disagree");
          std::fprintf(out, "\n %u %u", id, n);
          for (uint32_t i : b) std::fprintf(out, " %u", i);
        }
      std::fprintf(out, "\n");
    } else {
      die("unknown command");
    }
  }
  std::fprintf(out, "end\n");
  std::fclose(out);
  std::fclose(in);
  return 0;
}
