// SemanticDSPMap::worldObjects / queryWorldObjects (include/semantic_dsp_map.h, "additions") on the wall scene of
// tests/cpp/adapter_world_reach.cpp.  Built against tests/mock_includes and linked with libsdm_hip.so.  Without an
// argument: construction only (no device needed).  With `run`: exit code 0 = the archive of the wall scene has objects, the
// table is the C ABI's called directly, its entries are consistent (ascending, boxes round first cells, float fields by the
// header's formulas, the counts add up to info's), the objects of one label are those of every label that carry it, a
// label the archive does not hold and a min_cells above every object give an empty table, the point at an object's
// centroid's cell is answered like that cell, an object's first cell with its index, and the build outlives sdm_world_clear.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adapter_scene.h"
#include "semantic_dsp_map.h"

int main(int argc, char **argv) {
  const bool run = argc > 1;
  SemanticDSPMap a;
  SdmGridPreset p;
  preset(a, p);
  std::vector<sdm_world_object> table;
  std::vector<sdm_world_object_result> res;
  if (!run) {
    if (a.worldObjects(table, -1) || !table.empty()) return 4;  // no map yet
    if (a.queryWorldObjects({Eigen::Vector3d(0, 0, 0)}, res) != 0 || !res.empty()) return 4;
    std::printf("adapter constructed\n");
    return 0;
  }
  wall_frame(a, p, 0.0);
  if (a.worldObjects(table, -1)) return 5;  // no archive yet
  for (int t = 1; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  sdm_world_objects_info info;
  if (!a.worldObjects(table, -1, 1, false, false, &info)) return 6;
  std::printf("%u bricks, %lld cells (%lld guessed), %u objects of %u\n", info.n_bricks, (long long)info.n_cells, (long long)info.n_guessed,
              info.n_objects, info.n_objects_total);
  if (table.empty() || table.size() != info.n_objects || info.n_objects != info.n_objects_total || info.n_cells < 10 || info.flags != 0u) return 7;
  // the C ABI called directly gives the same table
  std::vector<sdm_world_object> direct(table.size());
  int32_t n = 0;
  if (sdm_get_world_objects(a.handle(), direct.data(), (int32_t)direct.size(), &n, nullptr) != SDM_OK || n != (int32_t)table.size()) return 8;
  if (std::memcmp(direct.data(), table.data(), table.size() * sizeof(sdm_world_object)) != 0) return 8;
  int64_t cells = 0, guessed = 0;
  size_t largest = 0;
  for (size_t i = 0; i < table.size(); ++i) {
    const sdm_world_object &c = table[i];
    if (i && c.first_index <= table[i - 1].first_index) return 9;
    if (c.n_cells == 0 || c.n_guessed > c.n_cells || c.pad0 || c.pad1 || c.mixed_tracks > 1) return 10;
    for (int ax = 0; ax < 3; ++ax) {
      if (c.first_cell[ax] < c.cell_min[ax] || c.first_cell[ax] > c.cell_max[ax]) return 11;
      if (c.cell_sum[ax] < (int64_t)c.cell_min[ax] * c.n_cells || c.cell_sum[ax] > (int64_t)c.cell_max[ax] * c.n_cells) return 11;
      if (c.cell_sq[ax] < 0) return 11;
      if (c.box_min[ax] != (float)c.cell_min[ax] * p.voxel_size || c.box_max[ax] != (float)(c.cell_max[ax] + 1) * p.voxel_size) return 12;
      if (c.centroid[ax] != (float)(((double)c.cell_sum[ax] / (double)c.n_cells + 0.5) * (double)p.voxel_size)) return 12;
    }
    cells += c.n_cells;
    guessed += c.n_guessed;
    if (c.n_cells > table[largest].n_cells) largest = i;
  }
  if (cells != info.n_cells || guessed != info.n_guessed) return 13;
  // one label: the objects of every label that carry it
  const int label = table[largest].label;
  std::vector<sdm_world_object> one, none, large;
  sdm_world_objects_info one_info, large_info;
  if (!a.worldObjects(one, label, 1, false, false, &one_info)) return 14;
  size_t with_label = 0;
  for (const sdm_world_object &c : table) with_label += c.label == label;
  if (one.size() != with_label || one.empty() || one_info.n_cells > info.n_cells) return 14;
  for (const sdm_world_object &c : one)
    if (c.label != label) return 14;
  bool held[256] = {};
  for (const sdm_world_object &c : table) held[c.label] = true;
  int absent = 0;
  while (absent < 256 && held[absent]) ++absent;
  if (absent < 256 && (!a.worldObjects(none, absent) || !none.empty())) return 15;
  if (a.worldObjects(none, 256)) return 15;
  if (!a.worldObjects(large, -1, 1 << 30, false, false, &large_info) || !large.empty() || large_info.n_objects != 0 ||
      large_info.n_objects_total != info.n_objects_total || large_info.n_cells != info.n_cells)
    return 15;
  // what is the thing at this point?  the largest object of the label: its first cell, and the cell of its centroid
  if (!a.worldObjects(one, label)) return 16;
  size_t big = 0;
  for (size_t i = 0; i < one.size(); ++i)
    if (one[i].n_cells > one[big].n_cells) big = i;
  const sdm_world_object &c = one[big];
  const double vs = p.voxel_size;
  const Eigen::Vector3d first((c.first_cell[0] + 0.5) * vs, (c.first_cell[1] + 0.5) * vs, (c.first_cell[2] + 0.5) * vs);
  const Eigen::Vector3d centre(c.centroid[0], c.centroid[1], c.centroid[2]);
  if (a.queryWorldObjects({first, centre}, res) != 2) return 17;
  if (res[0].object != (uint32_t)big || res[0].index != c.first_index || res[0].pad != 0u) return 17;
  for (int ax = 0; ax < 3; ++ax)
    if (res[0].cell[ax] != c.first_cell[ax] || res[1].cell[ax] < c.cell_min[ax] || res[1].cell[ax] > c.cell_max[ax]) return 17;
  // (a centroid need not lie in its object; the point is answered like its cell)
  sdm_world_object_result by_cell;
  if (sdm_query_world_objects(a.handle(), nullptr, res[1].cell, 1, &by_cell, 0u) != SDM_OK) return 18;
  if (by_cell.object != res[1].object || by_cell.index != res[1].index) return 18;
  if (res[1].object != SDM_WORLD_OBJECT_NONE && res[1].object >= one.size()) return 18;
  std::printf("the cell of the centroid of object %zu (%u cells, label %d) belongs to object %d\n", big, c.n_cells, label, (int)res[1].object);
  // the build is a snapshot: the archive goes, the table and the query stay
  direct.resize(one.size());
  if (sdm_world_clear(a.handle()) != SDM_OK) return 19;
  if (sdm_get_world_objects(a.handle(), direct.data(), (int32_t)direct.size(), &n, nullptr) != SDM_OK || n != (int32_t)one.size()) return 19;
  if (std::memcmp(direct.data(), one.data(), one.size() * sizeof(sdm_world_object)) != 0) return 19;
  std::vector<sdm_world_object_result> again;
  if (a.queryWorldObjects({first, centre}, again) != 2 || std::memcmp(again.data(), res.data(), 2 * sizeof(sdm_world_object_result)) != 0) return 19;
  if (a.worldObjects(large, -1)) return 20;  // (no archive any more)
  std::printf("world objects ok\n");
  return 0;
}
