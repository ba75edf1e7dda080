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

#include "ref_harness_common.h"

namespace {

// what the harness needs of RingBufferOperations' protected part
class Probe : public MTRingBufferOperations {
 public:
  using RingBufferOperations::globalFramePostoVoxelIdx;
};

Eigen::Matrix3f intrinsic() {  // as operations.h:1309-1310 builds it
  Eigen::Matrix3f k;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) k(r, c) = r == c ? 1.f : 0.f;
  k(0, 0) = g_camera_fx;
  k(1, 1) = g_camera_fy;
  k(0, 2) = g_camera_cx;
  k(1, 2) = g_camera_cy;
  return k;
}

}  // namespace

int main(int argc, char **argv) {
  open_files(argc, argv);

  static Probe op;  // constructs the ring: runSystemChecking + initialize, operations.h:44-49
  GaussianRandomCalculator calc;
  write_head();

  char cmd[64];
  while (std::fscanf(in, "%63s", cmd) == 1) {
    const std::string c(cmd);
    if (ring_command(c, op)) {
      // noise, ts, ego, load, move, visible, dump_ring, dump_stamps, dump_state, dump_bins: ref_harness_common.h
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
    } else if (c == "delete") {  // delete n indices: deleteParticlesInSet, operations.h:216-221
      long n = rd_int();
      std::unordered_set<uint32_t> s;
      for (long i = 0; i < n; ++i) s.insert(uint32_t(rd_int()));
      op.deleteParticlesInSet(s);
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
    } else {
      die("unknown command");
    }
  }
  std::fprintf(out, "end\n");
  std::fclose(out);
  std::fclose(in);
  return 0;
}
