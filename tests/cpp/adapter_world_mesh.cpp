// SemanticDSPMap::worldMesh (include/semantic_dsp_map.h, "additions") on the wall scene of tests/cpp/adapter_world_esdf.cpp.
// Built against tests/mock_includes and linked with libsdm_hip.so.  Without an argument: construction only (no device
// needed).  With `run`: exit code 0 = the mesh of the wall scene's archive is the C ABI's called directly - positions,
// triangles, records and coordinates -, every triangle's normal is its face's direction, every solid cell is an archived
// obstacle, the mesh is closed (per axis the signed sum of the faces' planes is the number of solid cells), a cap below the
// counts gives nothing, a box cuts the field, and the build outlives a worldRetain that removes every brick.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adapter_scene.h"
#include "semantic_dsp_map.h"

static sdm_world_mesh_options all_cells() {
  sdm_world_mesh_options o;
  std::memset(&o, 0, sizeof(o));
  o.track = -1;
  for (int k = 0; k < 8; ++k) o.labels[k] = 0xffffffffu;
  return o;
}

int main(int argc, char **argv) {
  const bool run = argc > 1;
  SemanticDSPMap a;
  SdmGridPreset p;
  preset(a, p);
  std::vector<float> xyz;
  std::vector<uint32_t> tri;
  std::vector<sdm_world_mesh_face> faces;
  std::vector<int16_t> coords;
  sdm_world_mesh_info info;
  sdm_world_mesh_options o = all_cells();
  if (!run) {
    if (a.worldMesh(o, xyz, tri, &faces, &coords, &info) != 0 || !xyz.empty() || !tri.empty()) return 4;  // no map yet
    std::printf("adapter constructed\n");
    return 0;
  }
  wall_frame(a, p, 0.0);
  if (a.worldMesh(o, xyz, tri) != 0) return 5;  // no archive yet
  for (int t = 1; t < 4; ++t) {
    wall_frame(a, p, 0.1 * t);
    if (!a.worldUpdate()) return 5;
  }
  const size_t n_tri = a.worldMesh(o, xyz, tri, &faces, &coords, &info);
  std::printf("%u bricks, %u vertex bricks, %lld faces, %lld vertices, %lld solid cells\n", info.n_bricks, info.n_vertex_bricks, (long long)info.n_faces,
              (long long)info.n_vertices, (long long)info.n_solid);
  if (n_tri == 0 || n_tri != 2 * (size_t)info.n_faces || tri.size() != 3 * n_tri || xyz.size() != 3 * (size_t)info.n_vertices) return 6;
  if (faces.size() != (size_t)info.n_faces || coords.size() != 3 * (size_t)info.n_bricks || info.n_solid < 20 || info.n_bricks == 0) return 6;
  // every solid cell is an archived obstacle
  std::vector<sdm_point> occ;
  if (!a.worldOccupied(occ) || (int64_t)occ.size() != info.n_solid) return 7;
  // the C ABI called directly: the same lists
  const size_t nf = (size_t)info.n_faces, nv = (size_t)info.n_vertices;
  std::vector<int16_t> c2(coords.size());
  std::vector<sdm_world_mesh_face> f2(nf);
  std::vector<uint32_t> quads(4 * nf);
  std::vector<int32_t> corners(3 * nv);
  std::vector<float> x2(3 * nv);
  int64_t n = 0;
  if (sdm_get_world_mesh_faces(a.handle(), c2.data(), f2.data(), quads.data(), 0, (int64_t)nf, &n) != SDM_OK || n != (int64_t)nf) return 8;
  if (sdm_get_world_mesh_vertices(a.handle(), corners.data(), x2.data(), 0, (int64_t)nv, &n) != SDM_OK || n != (int64_t)nv) return 8;
  if (std::memcmp(c2.data(), coords.data(), coords.size() * sizeof(int16_t)) != 0 || std::memcmp(f2.data(), faces.data(), nf * sizeof(sdm_world_mesh_face)) != 0 ||
      std::memcmp(x2.data(), xyz.data(), xyz.size() * sizeof(float)) != 0)
    return 9;
  long long flux[3] = {0, 0, 0};
  for (size_t f = 0; f < nf; ++f) {
    const uint32_t *q = &quads[4 * f], *t = &tri[6 * f];
    if (t[0] != q[0] || t[1] != q[1] || t[2] != q[2] || t[3] != q[0] || t[4] != q[2] || t[5] != q[3]) return 10;
    const sdm_world_mesh_face &fc = faces[f];
    if (fc.brick >= info.n_bricks || fc.dir > 5 || fc.kind > 3 || fc.occ < 1 || fc.cell > 511) return 11;
    // (q1 - q0) x (q3 - q0): the outward unit normal of dir, in lattice corners and - scaled - in positions
    long long e1[3], e3[3];
    for (int ax = 0; ax < 3; ++ax) {
      if (q[0] >= nv || q[1] >= nv || q[3] >= nv) return 11;
      e1[ax] = corners[3 * q[1] + ax] - corners[3 * q[0] + ax], e3[ax] = corners[3 * q[3] + ax] - corners[3 * q[0] + ax];
      if (xyz[3 * q[0] + ax] != (float)corners[3 * q[0] + ax] * p.voxel_size) return 12;
    }
    const long long nrm[3] = {e1[1] * e3[2] - e1[2] * e3[1], e1[2] * e3[0] - e1[0] * e3[2], e1[0] * e3[1] - e1[1] * e3[0]};
    for (int ax = 0; ax < 3; ++ax)
      if (nrm[ax] != (ax == fc.dir / 2 ? (fc.dir & 1 ? 1 : -1) : 0)) return 13;
    // the face's plane: the cell's coordinate along the axis, plus one for the upper face
    const int axis = fc.dir / 2, local = (fc.cell >> (3 * axis)) & 7;
    const long long plane = (long long)coords[3 * fc.brick + axis] * 8 + local + (fc.dir & 1);
    if (corners[3 * q[0] + axis] != plane) return 14;
    flux[axis] += (fc.dir & 1 ? 1 : -1) * plane;
  }
  for (int ax = 0; ax < 3; ++ax)
    if (flux[ax] != (long long)info.n_solid) return 15;  // closed: the divergence theorem in integers
  long long by_dir = 0, by_kind = 0;
  for (int k = 0; k < 6; ++k) by_dir += info.faces_by_dir[k];
  for (int k = 0; k < 4; ++k) by_kind += info.faces_by_kind[k];
  if (by_dir != info.n_faces || by_kind != info.n_faces || info.options.track != -1) return 16;
  // a cap below the counts: nothing
  std::vector<float> x3;
  std::vector<uint32_t> t3;
  sdm_world_mesh_options capped = o;
  capped.max_faces = info.n_faces - 1;
  if (a.worldMesh(capped, x3, t3) != 0 || !x3.empty() || !t3.empty()) return 17;
  // a box of one brick: a field of one brick, no more faces than before
  sdm_world_mesh_options boxed = o;
  boxed.flags = SDM_WORLD_MESH_BOX;
  for (int ax = 0; ax < 3; ++ax) boxed.bmin[ax] = boxed.bmax[ax] = coords[(size_t)ax];
  sdm_world_mesh_info bi;
  const size_t part = a.worldMesh(boxed, x3, t3, nullptr, nullptr, &bi);
  if (bi.n_bricks != 1 || part > n_tri || part != 2 * (size_t)bi.n_faces) return 18;
  // the build is a snapshot: a retain that keeps nothing empties the archive, the lists stay
  if (a.worldMesh(o, xyz, tri, &faces, &coords, &info) != n_tri) return 19;
  if (a.worldRetain(Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(-1, 0, 0)) != (int64_t)info.n_bricks) return 20;
  if (sdm_get_world_mesh_vertices(a.handle(), nullptr, x2.data(), 0, (int64_t)nv, &n) != SDM_OK || std::memcmp(x2.data(), xyz.data(), xyz.size() * sizeof(float)) != 0)
    return 21;
  // the next build sees the empty archive
  if (a.worldMesh(o, x3, t3, nullptr, nullptr, &bi) != 0 || bi.n_bricks != 0 || bi.n_faces != 0) return 22;
  std::printf("world mesh ok\n");
  return 0;
}
