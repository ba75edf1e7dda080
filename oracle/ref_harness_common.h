/*
 * oracle/ref_harness_common.h - what oracle/ref_harness.cpp and oracle/ref_filter_harness.cpp share: the text protocol
 * (integers in decimal, every float as the 8 hex digits of its binary32 pattern) and the commands that put the
 * reference's ring buffer into a state and read it back.
 *
 * TEST INFRASTRUCTURE ONLY.  Included after the reference's own headers (by path, at build time: oracle/Makefile, target
 * `ref`); none of their text is in this file.  `ring_command` runs one command on the MTRingBufferOperations it is given
 * and says whether the word was one of its own.
 */
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

namespace {

FILE *in = nullptr, *out = nullptr;
const char *harness_name = "ref_harness";

[[noreturn]] void die(const char *what) {
  std::fprintf(stderr, "%s: %s\n", harness_name, what);
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

std::vector<float> noise_table;
void fill_noise() {
  if (noise_table.empty()) return;
  for (int i = 0; i < GAUSSIAN_RANDOM_NUM; ++i) gaussian_randoms[i] = noise_table[i % noise_table.size()];
}

Eigen::Vector3f last_ego = Eigen::Vector3f::Zero();  // mirrors the function-static of operations.h:70

bool slot_is_cleared(uint32_t idx) {  // the state RingBufferOperations::clear() leaves, operations.h:701-722
  const Particle &p = PARTICLE_ARRAY[idx];
  const bool time_slot = (idx & (C_MAX_PARTICLE_NUM_PER_VOXEL - 1)) == 0;
  return p.status == (time_slot ? Particle_Status::TIMEPTC : Particle_Status::INVALID) && p.pos.x == 0.f && p.pos.y == 0.f &&
         p.pos.z == 0.f && p.pos.weight == 0.f && p.time_stamp == 0 && p.track_id == 0 && p.label_id == 0 && p.forget_count == 0 &&
         !std::signbit(p.pos.x) && !std::signbit(p.pos.y) && !std::signbit(p.pos.z) && !std::signbit(p.pos.weight);
}

void open_files(int argc, char **argv) {
  if (argc != 3) die("usage: <harness> <scenario> <result>");
  in = std::fopen(argv[1], "r");
  out = std::fopen(argv[2], "w");
  if (!in || !out) die("cannot open files");
}

void write_head() {
  std::fprintf(out, "variant %u %u %u %u %d %d\n", C_VOXEL_NUM_AXIS_X, C_VOXEL_NUM_AXIS_Y, C_VOXEL_NUM_AXIS_Z,
               unsigned(C_MAX_PARTICLE_NUM_PER_VOXEL), g_image_width, g_image_height);
  std::fprintf(out, "camera");
  wr_f(C_VOXEL_SIZE), wr_f(g_camera_fx), wr_f(g_camera_fy), wr_f(g_camera_cx), wr_f(g_camera_cy), wr_f(g_depth_range_min), wr_f(g_depth_range_max);
  std::fprintf(out, "\n");
}

bool ring_command(const std::string &c, MTRingBufferOperations &op) {
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
  } else if (c == "dump_state" || c == "dump_particles") {  // every slot that is not as clear() leaves it; particles: but for the time slots
    const bool all = c == "dump_state";
    auto listed = [all](uint32_t i) { return !slot_is_cleared(i) && (all || (i & (C_MAX_PARTICLE_NUM_PER_VOXEL - 1)) != 0); };
    long n = 0;
    for (uint32_t i = 0; i < C_MAX_PARTICLE_NUM; ++i) n += listed(i) ? 1 : 0;
    std::fprintf(out, "%s %ld", all ? "state" : "particles", n);
    for (uint32_t i = 0; i < C_MAX_PARTICLE_NUM; ++i) {
      if (!listed(i)) continue;
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
    return false;
  }
  return true;
}

}  // namespace
