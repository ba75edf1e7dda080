/*
 * oracle/ref_filter_harness.cpp - drives the reference's own particle filter, the members of SemanticDSPMap that touch
 * neither PCL nor OpenCV: updateParticles (semantic_dsp_map.h:960-1121), addGuessedParticle (1126-1142),
 * addNewbornParticleAndResample (1148-1171), addNewbornParticleWithNoiseAndResample (1177-1230) and
 * resampleParticlesInVoxel (1448-1519), over ObjectParticleHashMap (object_layer.h:20-52), from a scenario file.
 *
 * TEST INFRASTRUCTURE ONLY.  The reference's headers are included by path at build time (oracle/Makefile, target `ref`,
 * one ref_filter_<variant> executable per variant of settings/settings.h); none of their text is in this file.  The
 * build-time copy of semantic_dsp_map.h loses, by the line numbers of ref_filter_members.sed, the includes and members
 * that need PCL or OpenCV, the `private:` line and pt_tools_; the copy of object_layer.h ends after
 * ObjectParticleHashMap (ref_filter_object_layer.sed), and the two members of ObjectSet that the kept code uses are
 * declared below.  Everything else of the class - constructor, clear, setters, data members, the five members above -
 * is compiled as it stands.
 *
 * One thing here is this file's own reading and not compiled reference text: the order in which `births` visits the
 * pixels.  That loop (semantic_dsp_map.h:777-800) sits inside subObjectLevelUpdate, which had to be cut.
 *
 *   ref_filter_harness <scenario> <result>
 *
 * The protocol and the ring commands are those of ref_harness.cpp (ref_harness_common.h); oracle/ref_filter.py writes
 * the one file and reads the other; the commands of this harness are listed in main().
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
#include "settings/external_settings.h"  // the flag getters and setters; the reference reaches it through utils/pointcloud_tools.h
#include "object_layer.h"  // the build-time copy: ObjectParticleHashMap only

// what the kept members of SemanticDSPMap use of ObjectSet (object_layer.h:376, 379-384)
class ObjectSet {
 public:
  ObjectParticleHashMap obj_ptc_hash_map;
  void clear() { obj_ptc_hash_map.clear(); }
};

#include "semantic_dsp_map.h"  // the build-time copy reduced by ref_filter_members.sed

#include "ref_harness_common.h"

namespace {

// GaussianRandomCalculator keeps its cursor private and basic_algorithms.h is compiled as it stands: an explicit
// instantiation may name a private member, which is all this needs to read it.
int GaussianRandomCalculator::*cursor_member();
template <int GaussianRandomCalculator::*M> struct CursorAccess {
  friend int GaussianRandomCalculator::*cursor_member() { return M; }
};
template struct CursorAccess<&GaussianRandomCalculator::gaussian_random_seq_>;

typedef std::vector<std::vector<LabeledPoint>> Cloud;

}  // namespace

int main(int argc, char **argv) {
  harness_name = "ref_filter_harness";
  open_files(argc, argv);

  static SemanticDSPMap map;  // constructs the ring (operations.h:44-49) and fills the tables (semantic_dsp_map.h:66)
  MTRingBufferOperations &op = map.op_mt_;
  Cloud cloud(g_image_height, std::vector<LabeledPoint>(g_image_width));
  write_head();

  char cmd[64];
  while (std::fscanf(in, "%63s", cmd) == 1) {
    const std::string c(cmd);
    if (ring_command(c, op)) {
      // noise, ts, ego, load, move, visible, dump_ring, dump_stamps, dump_state, dump_bins: ref_harness_common.h
    } else if (c == "params") {  // setMapParameters, setMapOptions, setDepthNoiseModelParameters: semantic_dsp_map.h:101-125, 161-166
      float pd = rd_f(), noise_number = rd_f();
      long nb = rd_int();
      float occ = rd_f();
      long lost = rd_int();
      float rate = rd_f();
      long max_forget = rd_int();
      float match = rd_f(), id_transition = rd_f();
      long depth_noise = rd_int(), independent = rd_int();
      float first = rd_f(), zero = rd_f();
      map.setMapParameters(pd, noise_number, int(nb), occ, int(lost), rate, int(max_forget), match, id_transition);
      map.setMapOptions(depth_noise != 0, independent != 0);
      map.setDepthNoiseModelParameters(first, zero);
    } else if (c == "cloud") {  // cloud sigma n, then n x (row col x y z sigma label track valid); a pixel not listed is invalid with `sigma`
      float sigma = rd_f();
      for (auto &row : cloud)
        for (auto &pt : row) {
          pt.position << 0.f, 0.f, 0.f;
          pt.sigma = sigma, pt.track_id = 0, pt.label_id = 0, pt.is_valid = false;
        }
      long n = rd_int();
      for (long i = 0; i < n; ++i) {
        long r = rd_int(), q = rd_int();
        if (r < 0 || r >= g_image_height || q < 0 || q >= g_image_width) die("cloud: pixel outside the image");
        LabeledPoint &pt = cloud[r][q];
        float x = rd_f(), y = rd_f(), z = rd_f();
        pt.position << x, y, z;
        pt.sigma = rd_f();
        pt.label_id = uint8_t(rd_int());
        pt.track_id = uint16_t(rd_int());
        pt.is_valid = rd_int() != 0;
      }
    } else if (c == "set_owners") {  // set_owners k, then k x (track n indices): updatePtcIndicesOfObj, object_layer.h:26-28
      long k = rd_int();
      for (long s = 0; s < k; ++s) {
        int track = int(rd_int());
        long n = rd_int();
        std::unordered_set<uint32_t> set;
        for (long i = 0; i < n; ++i) set.insert(uint32_t(rd_int()));
        map.object_set_.obj_ptc_hash_map.updatePtcIndicesOfObj(track, set);
      }
    } else if (c == "permute_bins") {  // data only: 0 as pushed, 1 ascending by index, 2 reversed
      long k = rd_int();
      for (int r = 0; r < g_image_height; ++r)
        for (int q = 0; q < g_image_width; ++q) {
          if (!particle_to_pixel_num_array[r][q]) continue;
          std::vector<uint32_t> &b = particle_to_pixel_index_map[uint32_t(r) * g_image_width + q];
          if (k == 1) std::sort(b.begin(), b.end());
          else if (k == 2) std::reverse(b.begin(), b.end());
        }
    } else if (c == "update_particles") {  // semantic_dsp_map.h:960-1121; its ck_kappa_array is a local and is not read
      map.updateParticles(cloud);
    } else if (c == "births") {  // births mode (-1: as the flag stands, 0 / 1: setFlagConsiderDepthNoise first)
      long mode = rd_int();
      if (mode >= 0) setFlagConsiderDepthNoise(mode != 0);
      uint32_t added = 0;
      std::unordered_set<uint32_t> resampled;
      // THIS FILE'S OWN WORDS, read from semantic_dsp_map.h:777-800: nine passes over the image, pass (row_start,
      // col_start) visiting every third row and column from there in row-major order; valid pixels only
      for (int row_start = 0; row_start < 3; ++row_start)
        for (int col_start = 0; col_start < 3; ++col_start)
          for (int i = row_start; i < int(cloud.size()); i += 3)
            for (int j = col_start; j < int(cloud[0].size()); j += 3) {
              const LabeledPoint &pt = cloud[i][j];
              if (!pt.is_valid) continue;
              if (!getFlagConsiderDepthNoise()) map.addNewbornParticleAndResample(pt, added, resampled);
              else map.addNewbornParticleWithNoiseAndResample(pt, added, resampled);
            }
      std::vector<uint32_t> v(resampled.begin(), resampled.end());
      std::sort(v.begin(), v.end());
      std::fprintf(out, "births %u %zu", added, v.size());
      for (uint32_t i : v) std::fprintf(out, " %u", i);
      std::fprintf(out, "\n");
    } else if (c == "resample") {  // resample n voxels: resampleParticlesInVoxel, semantic_dsp_map.h:1448-1519
      long n = rd_int();
      std::fprintf(out, "resample %ld", n);
      for (long i = 0; i < n; ++i) {
        uint32_t v = uint32_t(rd_int());
        if (v >= C_VOXEL_NUM_TOTAL) die("resample: voxel out of range");
        std::fprintf(out, " %d", map.resampleParticlesInVoxel(v, map.object_set_.obj_ptc_hash_map) ? 1 : 0);
      }
      std::fprintf(out, "\n");
    } else if (c == "guessed") {  // guessed label track n points: addGuessedParticle, semantic_dsp_map.h:1126-1142
      long label = rd_int(), track = rd_int(), n = rd_int();
      for (long i = 0; i < n; ++i) {
        LabeledPoint pt;
        float x = rd_f(), y = rd_f(), z = rd_f();
        pt.position << x, y, z;
        pt.sigma = 0.f, pt.label_id = uint8_t(label), pt.track_id = uint16_t(track), pt.is_valid = true;
        map.addGuessedParticle(pt);
      }
    } else if (c == "burn") {  // burn n: n queries on the map's own calculator, basic_algorithms.h:426-433
      long n = rd_int();
      for (long i = 0; i < n; ++i) map.gaussian_random_.queryNormalRandomPresetSD();
    } else if (c == "dump_cursor") {
      std::fprintf(out, "cursor %d\n", map.gaussian_random_.*cursor_member());
    } else if (c == "dump_owners") {  // every track of indices_map with its indices, both sorted; empty sets included
      auto &im = map.object_set_.obj_ptc_hash_map.indices_map;
      std::map<int, std::vector<uint32_t>> sorted;
      for (auto &kv : im) {
        std::vector<uint32_t> v(kv.second.begin(), kv.second.end());
        std::sort(v.begin(), v.end());
        sorted[kv.first] = v;
      }
      std::fprintf(out, "owners %zu", sorted.size());
      for (auto &kv : sorted) {
        std::fprintf(out, "\n %d %zu", kv.first, kv.second.size());
        for (uint32_t i : kv.second) std::fprintf(out, " %u", i);
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
