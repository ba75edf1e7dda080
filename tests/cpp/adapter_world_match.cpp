// SemanticDSPMap::worldMatch (include/semantic_dsp_map.h, "additions") on the wall scene of tests/cpp/adapter_world.cpp: one
// map archives the wall, a second map imports its bricks under a planted offset, and worldMatch on the second finds that
// offset again.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an argument: construction only
// (no device needed).  With `run`: exit code 0 = the planted offset is the best candidate, with every occupied source cell
// on an occupied cell of the same label and no conflict, the runner-up below it; the scores are in candidate order; the
// match through the C ABI called directly gives the same result; the archive is left as it was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adapter_scene.h"
#include "semantic_dsp_map.h"

int main(int argc, char **argv) {
  const bool run = argc > 1;
  SemanticDSPMap a, b;
  SdmGridPreset p;
  preset(a, p);
  preset(b, p);
  std::vector<sdm_world_brick> bricks, before, after;
  std::vector<uint32_t> cells, before_cells, after_cells;
  std::vector<sdm_world_match_score> scores(3);
  Eigen::Vector3i found(9, 9, 9);
  if (!run) {
    bricks.resize(1);
    cells.resize(512);
    if (a.worldMatch(bricks, cells, found, Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(1, 1, 1), nullptr, &scores) || !scores.empty()) return 4;  // no map yet
    if (found.x() != 9) return 4;
    std::printf("adapter constructed\n");
    return 0;
  }
  for (int t = 0; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  wall_frame(b, p, 0.0);
  const size_t n = a.worldBricks(bricks, cells);
  sdm_world_info ia;
  if (!n || !a.worldInfo(ia) || ia.n_occupied == 0) return 6;
  if (b.worldMatch(bricks, cells, found)) return 7;  // no archive yet
  const Eigen::Vector3i planted(3, -2, 1);
  if (!b.worldImport(bricks, cells, planted) || b.worldBricks(before, before_cells) == 0) return 8;
  if (b.worldMatch(bricks, cells, found, Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(9, 0, 0))) return 9;  // a radius beyond 8
  sdm_world_match_result r;
  if (!b.worldMatch(bricks, cells, found, Eigen::Vector3i(1, 0, 0), Eigen::Vector3i(4, 4, 2), &r, &scores)) return 10;
  std::printf("%zu bricks, %u occupied and %u free source cells, best (%d, %d, %d) score %lld, runner-up %lld\n", n, r.src_occupied, r.src_free,
              found.x(), found.y(), found.z(), (long long)r.best_score, (long long)r.runner_up);
  if (found.x() != planted.x() || found.y() != planted.y() || found.z() != planted.z()) return 11;
  if (r.n_candidates != 9 * 9 * 5 || scores.size() != r.n_candidates || r.n_sources != n || r.src_occupied != ia.n_occupied || r.src_free != ia.n_free) return 12;
  const sdm_world_match_score &s = scores[(size_t)r.best];
  if (s.offset[0] != 3 || s.offset[1] != -2 || s.offset[2] != 1 || s.n_oo != r.src_occupied || s.n_same != s.n_oo || s.n_of || s.n_fo || s.n_ff != r.src_free) return 13;
  if (r.best_score != 5 * (int64_t)s.n_oo || r.runner_up >= r.best_score) return 14;
  if (scores[0].offset[0] != -3 || scores[0].offset[1] != -4 || scores[0].offset[2] != -2 || scores[1].offset[0] != -2 || scores[9].offset[1] != -3) return 15;
  // the C ABI called directly
  sdm_world_match_options o;
  std::memset(&o, 0, sizeof(o));
  o.cell_offset[0] = 1;
  o.radius[0] = o.radius[1] = 4, o.radius[2] = 2;
  o.w_oo = 4, o.w_same = 1, o.w_of = o.w_fo = -2;
  sdm_world_match_result direct;
  if (sdm_world_match(b.handle(), &o, bricks.data(), cells.data(), (int64_t)n, nullptr, &direct) != SDM_OK) return 16;
  if (std::memcmp(&direct, &r, sizeof(r)) != 0) return 17;
  // weights of the caller's: only conflicts count, and the planted offset is still the only one without any
  const int32_t w[5] = {0, 0, -1, -1, 0};
  if (!b.worldMatch(bricks, cells, found, Eigen::Vector3i(3, -2, 1), Eigen::Vector3i(0, 0, 0), &r, nullptr, w) || r.best_score != 0 || r.n_candidates != 1) return 18;
  if (b.worldBricks(after, after_cells) != before.size() || std::memcmp(after.data(), before.data(), before.size() * sizeof(sdm_world_brick)) != 0 ||
      after_cells != before_cells)
    return 19;
  std::printf("world match ok\n");
  return 0;
}
