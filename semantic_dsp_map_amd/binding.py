"""ctypes binding of libsdm_hip (include/sdm.h) — plumbing for tests and bench.py.

The product is the C-ABI library; this module only marshals numpy / torch
buffers into it.  There is no CPU path: if the HIP library is missing or no
GPU is visible, loading / creating a map fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDM_LIB_PATH") or os.path.join(_HERE, "csrc", "libsdm_hip.so")  # override: debug builds only

LABELED_POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("sigma", "<f4"),
                          ("track_id", "<u2"), ("label_id", "u1"), ("is_valid", "u1")])
OBJECT_MOVE = np.dtype([("track_id", "<i4"), ("T", "<f4", (16,))])
VOXEL_RESULT = np.dtype([("wsum", "<f4"), ("track", "<u2"), ("label", "u1"), ("occ", "i1")])
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("track", "<u2"), ("label", "u1"), ("occ", "i1")])
# sdm_point_xyzrgb = pcl::PointXYZRGB's 32 bytes
POINT_XYZRGB = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("one", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"),
                         ("pad", "<u4", (3,))])
assert LABELED_POINT.itemsize == 20 and OBJECT_MOVE.itemsize == 68 and VOXEL_RESULT.itemsize == 8 and POINT.itemsize == 16
# the batched map queries (sdm.h: sdm_query_segments / sdm_query_boxes)
SEGMENT_HIT = np.dtype([("t", "<f4"), ("voxel", "<u4"), ("cells", "<i4"), ("track", "<u2"), ("label", "u1"), ("occ", "i1")])
BOX_RESULT = np.dtype([("n_occupied", "<i4"), ("n_free", "<i4"), ("n_unknown", "<i4"), ("first_occupied", "<u4"), ("clipped", "<i4")])
assert SEGMENT_HIT.itemsize == 16 and BOX_RESULT.itemsize == 20
QUERY_ON_DEVICE = 0x1
QUERY_UNKNOWN_BLOCKS = 0x2
# the distance field (sdm.h: sdm_esdf_update / sdm_query_distance)
DISTANCE_RESULT = np.dtype([("distance", "<f4"), ("gradient", "<f4", (3,)), ("nearest", "<f4", (3,)), ("d2", "<u4"), ("track", "<u2"),
                            ("label", "u1"), ("occ", "i1")])
assert DISTANCE_RESULT.itemsize == 36
ESDF_UNKNOWN_IS_OBSTACLE = 0x1
ESDF_STATIC_ONLY = 0x2
# the instance table (sdm.h: sdm_instances_update / sdm_get_instances / sdm_get_label_cells)
INSTANCE = np.dtype([("track", "<u2"), ("label", "u1"), ("mixed_labels", "u1"), ("n_cells", "<u4"), ("n_guessed", "<u4"),
                     ("first_cell", "<u4"), ("cell_min", "<u2", (3,)), ("cell_max", "<u2", (3,)), ("wsum_max", "<f4"),
                     ("cell_sum", "<u8", (3,)), ("cell_sq", "<u8", (6,)), ("box_min", "<f4", (3,)), ("box_max", "<f4", (3,)),
                     ("centroid", "<f4", (3,)), ("pad", "<u4")])
assert INSTANCE.itemsize == 144
INSTANCES_MOVABLE_ONLY = 0x1
INSTANCES_OBSERVED_ONLY = 0x2
# the frontiers (sdm.h: sdm_frontiers_update / sdm_get_frontier_clusters / sdm_get_frontier_cells)
FRONTIER_CLUSTER = np.dtype([("first_cell", "<u4"), ("n_cells", "<u4"), ("n_unknown_faces", "<u4"), ("first_index", "<u4"),
                             ("cell_min", "<u2", (3,)), ("cell_max", "<u2", (3,)), ("pad0", "<u4"), ("cell_sum", "<u8", (3,)),
                             ("box_min", "<f4", (3,)), ("box_max", "<f4", (3,)), ("centroid", "<f4", (3,)), ("pad1", "<u4")])
assert FRONTIER_CLUSTER.itemsize == 96
FRONTIERS_FACE_CONNECTED = 0x1
FRONTIER_NO_CLUSTER = 0xFFFFFFFF

# view scoring (sdm.h: sdm_query_views)
VIEW = np.dtype([("pos", "<f4", (3,)), ("q", "<f4", (4,)), ("range", "<f4")])
VIEW_GAIN = np.dtype([("n_unknown", "<u4"), ("n_free", "<u4"), ("n_occupied", "<u4"), ("rays_hit", "<u4"), ("rays_in_map", "<u4"),
                      ("pad", "<u4"), ("ray_cells", "<u8"), ("ray_unknown", "<u8")])
assert VIEW.itemsize == 32 and VIEW_GAIN.itemsize == 40
VIEW_MAX_RAYS = 65536
# the travel-cost field (sdm.h: sdm_reach_update / sdm_get_reach / sdm_query_reach / sdm_reach_paths)
REACH_INFO = np.dtype([("n_starts_used", "<u4"), ("n_traversable", "<u4"), ("n_reached", "<u4"), ("max_cost_reached", "<u4"),
                       ("rounds", "<u4"), ("flags", "<u4"), ("min_d2", "<u4"), ("max_cost", "<u4")])
REACH_RESULT = np.dtype([("cost", "<u4"), ("metres", "<f4"), ("cell", "<u4"), ("next", "u1"), ("status", "u1"), ("pad", "<u2")])
assert REACH_INFO.itemsize == 32 and REACH_RESULT.itemsize == 16
REACH_FACE_CONNECTED = 0x1
REACH_THROUGH_UNKNOWN = 0x2
REACH_COST_PER_CELL = 10
REACH_NO_COST = 0xFFFFFFFF
# the forecast (sdm.h: sdm_motion, sdm_forecast_stamp / _info / _result / _hit)
MOTION = np.dtype([("track", "<u2"), ("pad", "<u2"), ("v", "<f4", (3,))])
FORECAST_STAMP = np.dtype([("track", "<u2"), ("horizon", "u1"), ("pad", "u1"), ("d", "<i2", (3,)), ("pad2", "<i2")])
FORECAST_INFO = np.dtype([("n_motions", "<u4"), ("n_horizons", "<u4"), ("n_stamps", "<u4"), ("flags", "<u4"), ("n_sources", "<u4"),
                          ("n_marked", "<u4"), ("n_marks_in", "<u8"), ("n_marks_out", "<u8")])
FORECAST_RESULT = np.dtype([("state", "i1"), ("horizon", "u1"), ("track", "<u2"), ("mask", "<u2"), ("first_horizon", "u1"), ("pad", "u1")])
FORECAST_HIT = np.dtype([("t", "<f4"), ("cell", "<u4"), ("cells", "<i4"), ("track", "<u2"), ("state", "i1"), ("horizon", "u1")])
FORECAST_SWEPT = 0x1
FORECAST_VACATED_BLOCKS = 0x4
FORECAST_MAX_HORIZONS = 16
FORECAST_MAX_STAMPS = 65536
FORECAST_NOTHING = 0xFFFFFFFF
# the ground layer (sdm.h: sdm_ground_update / sdm_get_ground / sdm_query_ground / sdm_query_footprints)
GROUND_OPTIONS = np.dtype([("up_axis", "<i4"), ("up_sign", "<i4"), ("h_lo", "<i4"), ("h_hi", "<i4"), ("clearance", "<u4"),
                           ("max_step", "<u4"), ("support_labels", "<u4", (8,)), ("flags", "<u4")])
GROUND_CELL = np.dtype([("level", "<u2"), ("top", "<u2"), ("label", "u1"), ("cls", "u1"), ("headroom", "u1"), ("n_unknown", "u1")])
GROUND_INFO = np.dtype([("n_u", "<u4"), ("n_v", "<u4"), ("axis_u", "<u4"), ("axis_v", "<u4"), ("n_ground", "<u4"), ("n_obstacle", "<u4"),
                        ("n_none", "<u4"), ("n_step", "<u4"), ("n_lethal", "<u4"), ("level_min", "<u4"), ("level_max", "<u4"),
                        ("options", GROUND_OPTIONS)])
GROUND_RESULT = np.dtype([("col", "<u4"), ("d2", "<u4"), ("surface", "<f4"), ("above", "<i4"), ("cell", GROUND_CELL), ("dist", "<f4"),
                          ("status", "<u4")])
FOOTPRINT = np.dtype([("center_u", "<f4"), ("center_v", "<f4"), ("dir_u", "<f4"), ("dir_v", "<f4"), ("half_len", "<f4"), ("half_wid", "<f4")])
FOOTPRINT_RESULT = np.dtype([("n_cols", "<u4"), ("n_lethal", "<u4"), ("n_none", "<u4"), ("n_ground", "<u4"), ("level_min", "<u2"),
                             ("level_max", "<u2"), ("min_d2", "<u4"), ("first_lethal", "<u4"), ("pad", "<u4")])
assert GROUND_OPTIONS.itemsize == 60 and GROUND_CELL.itemsize == 8 and GROUND_INFO.itemsize == 104 and GROUND_RESULT.itemsize == 32
assert FOOTPRINT.itemsize == 24 and FOOTPRINT_RESULT.itemsize == 32
GROUND_UNKNOWN_PASSABLE = 0x1
GROUND_IGNORE_MOVABLE = 0x2
GROUND_NONE_IS_LETHAL = 0x4
GROUND_NO_LEVEL = 0xFFFF
GROUND_MAX_FOOTPRINT_CELLS = 64   # half_len + half_wid of a footprint, in voxels
# the surface mesh (sdm.h: sdm_mesh_update / sdm_get_mesh_info / sdm_get_mesh_faces / sdm_get_mesh_vertices / sdm_mesh_device)
MESH_OPTIONS = np.dtype([("flags", "<u4"), ("track", "<i4"), ("labels", "<u4", (8,)), ("max_faces", "<i8"), ("max_vertices", "<i8")])
MESH_FACE = np.dtype([("cell", "<u4"), ("track", "<u2"), ("label", "u1"), ("occ", "i1"), ("dir", "u1"), ("kind", "u1"), ("pad", "<u2")])
MESH_VERTEX = np.dtype([("i", "<u2"), ("j", "<u2"), ("k", "<u2"), ("pad", "<u2")])
MESH_INFO = np.dtype([("n_faces", "<u4"), ("n_vertices", "<u4"), ("n_solid", "<u4"), ("faces_by_dir", "<u4", (6,)),
                      ("faces_by_kind", "<u4", (4,)), ("pad", "<u4"), ("options", MESH_OPTIONS)])
assert MESH_OPTIONS.itemsize == 56 and MESH_FACE.itemsize == 12 and MESH_VERTEX.itemsize == 8 and MESH_INFO.itemsize == 112
MESH_STATIC_ONLY = 0x01
MESH_MOVABLE_ONLY = 0x02
MESH_OBSERVED_ONLY = 0x04
MESH_SKIP_UNKNOWN_FACES = 0x08
MESH_SKIP_BORDER_FACES = 0x10
# the world archive (sdm.h: sdm_world_update / sdm_get_world_info / sdm_get_world_bricks / sdm_get_world_occupied /
# sdm_query_world_points / sdm_get_world_region / sdm_world_clear)
WORLD_OPTIONS = np.dtype([("flags", "<u4"), ("pad", "<u4"), ("max_bricks", "<i8")])
WORLD_BRICK = np.dtype([("bx", "<i2"), ("by", "<i2"), ("bz", "<i2"), ("n_occupied", "<u2"), ("n_free", "<u2"), ("pad", "<u2"),
                        ("first_stamp", "<u4"), ("last_stamp", "<u4")])
WORLD_CELL = np.dtype([("track", "<u2"), ("label", "u1"), ("occ", "i1"), ("stamp", "<u4")])
WORLD_INFO = np.dtype([("n_bricks", "<u4"), ("max_bricks", "<u4"), ("n_updates", "<u4"), ("created_last", "<u4"), ("dropped_last", "<u4"),
                       ("out_of_range_last", "<u4"), ("dropped_total", "<u8"), ("n_occupied", "<u8"), ("n_free", "<u8"),
                       ("bmin", "<i4", (3,)), ("bmax", "<i4", (3,)), ("flags", "<u4"), ("stamp", "<u4")])
assert WORLD_OPTIONS.itemsize == 16 and WORLD_BRICK.itemsize == 20 and WORLD_CELL.itemsize == 8 and WORLD_INFO.itemsize == 80
WORLD_STATIC_ONLY = 0x01
WORLD_OBSERVED_ONLY = 0x02
WORLD_UNKNOWN_WORD = 0xFF000000
# ... its way back in and its trim (sdm.h: sdm_world_import / sdm_world_retain)
WORLD_IMPORT_OPTIONS = np.dtype([("flags", "<u4"), ("cell_offset", "<i4", (3,)), ("max_bricks", "<i8")])
WORLD_RETAIN_OPTIONS = np.dtype([("bmin", "<i4", (3,)), ("bmax", "<i4", (3,)), ("min_last_stamp", "<u4"), ("flags", "<u4")])
assert WORLD_IMPORT_OPTIONS.itemsize == 24 and WORLD_RETAIN_OPTIONS.itemsize == 32
WORLD_IMPORT_FILL = 0x10
WORLD_IMPORT_ON_DEVICE = 0x20
# ... and the step in front of an import: which whole-cell offset fits (sdm.h: sdm_world_match)
WORLD_MATCH_OPTIONS = np.dtype([("flags", "<u4"), ("cell_offset", "<i4", (3,)), ("radius", "<i4", (3,)), ("w_oo", "<i4"), ("w_same", "<i4"),
                                ("w_of", "<i4"), ("w_fo", "<i4"), ("w_ff", "<i4"), ("pad", "<u4", (2,))])
WORLD_MATCH_SCORE = np.dtype([("offset", "<i4", (3,)), ("n_oo", "<u4"), ("n_of", "<u4"), ("n_fo", "<u4"), ("n_ff", "<u4"), ("n_same", "<u4")])
WORLD_MATCH_RESULT = np.dtype([("n_candidates", "<u4"), ("n_sources", "<u4"), ("src_occupied", "<u4"), ("src_free", "<u4"),
                               ("best_score", "<i8"), ("runner_up", "<i8"), ("best", "<i4"), ("best_offset", "<i4", (3,)), ("pad", "<u4", (2,))])
assert WORLD_MATCH_OPTIONS.itemsize == 56 and WORLD_MATCH_SCORE.itemsize == 32 and WORLD_MATCH_RESULT.itemsize == 56
WORLD_MATCH_ON_DEVICE = 0x20
WORLD_MATCH_MAX_RADIUS = 8
WORLD_MATCH_WEIGHTS = (4, 1, -2, -2, 0)     # w_oo, w_same, w_of, w_fo, w_ff: the binding's default, not tuned
# world reach (sdm.h: sdm_world_reach_update / sdm_get_world_reach / sdm_query_world_reach / sdm_world_reach_paths)
WORLD_REACH_OPTIONS = np.dtype([("flags", "<u4"), ("inflate", "<u4"), ("max_cost", "<u4"), ("pad", "<u4"), ("bmin", "<i4", (3,)),
                                ("bmax", "<i4", (3,))])
WORLD_REACH_INFO = np.dtype([("n_bricks", "<u4"), ("n_starts_used", "<u4"), ("n_traversable", "<u4"), ("n_reached", "<u4"),
                             ("max_cost_reached", "<u4"), ("rounds", "<u4"), ("flags", "<u4"), ("inflate", "<u4"), ("max_cost", "<u4"),
                             ("stamp", "<u4")])
WORLD_REACH_RESULT = np.dtype([("cost", "<u4"), ("metres", "<f4"), ("cell", "<i4", (3,)), ("next", "u1"), ("status", "u1"), ("pad", "<u2")])
assert WORLD_REACH_OPTIONS.itemsize == 40 and WORLD_REACH_INFO.itemsize == 40 and WORLD_REACH_RESULT.itemsize == 24
WORLD_REACH_FACE_CONNECTED = 0x01
WORLD_REACH_THROUGH_UNKNOWN = 0x02
WORLD_REACH_IGNORE_MOVABLE = 0x04
WORLD_REACH_BOX = 0x08
WORLD_REACH_NO_CELL = -0x80000000   # what world_reach_paths fills its rows with behind a path
# world frontiers (sdm.h: sdm_world_frontiers_update / sdm_get_world_frontier_clusters / sdm_get_world_frontier_cells)
WORLD_FRONTIERS_OPTIONS = np.dtype([("flags", "<u4"), ("min_cells", "<i4"), ("max_cells", "<i8"), ("bmin", "<i4", (3,)), ("bmax", "<i4", (3,))])
WORLD_FRONTIER_CLUSTER = np.dtype([("first_index", "<u4"), ("n_cells", "<u4"), ("n_unknown_faces", "<u4"), ("pad0", "<u4"),
                                   ("first_cell", "<i4", (3,)), ("cell_min", "<i4", (3,)), ("cell_max", "<i4", (3,)), ("pad1", "<u4"),
                                   ("cell_sum", "<i8", (3,)), ("box_min", "<f4", (3,)), ("box_max", "<f4", (3,)), ("centroid", "<f4", (3,)),
                                   ("pad2", "<u4")])
WORLD_FRONTIERS_INFO = np.dtype([("n_bricks", "<u4"), ("n_clusters", "<u4"), ("n_clusters_total", "<u4"), ("flags", "<u4"), ("n_cells", "<i8"),
                                 ("n_unknown_faces", "<i8"), ("n_absent_faces", "<i8"), ("min_cells", "<i4"), ("stamp", "<u4")])
assert WORLD_FRONTIERS_OPTIONS.itemsize == 40 and WORLD_FRONTIER_CLUSTER.itemsize == 120 and WORLD_FRONTIERS_INFO.itemsize == 48
WORLD_FRONTIERS_FACE_CONNECTED = 0x1
WORLD_FRONTIERS_BOX = 0x2
WORLD_FRONTIERS_INSIDE_BRICKS = 0x4
WORLD_FRONTIER_NO_CLUSTER = 0xFFFFFFFF
# world distance field (sdm.h: sdm_world_esdf_update / sdm_get_world_esdf / sdm_query_world_distance)
WORLD_ESDF_OPTIONS = np.dtype([("flags", "<u4"), ("radius", "<u4"), ("bmin", "<i4", (3,)), ("bmax", "<i4", (3,))])
WORLD_ESDF_INFO = np.dtype([("n_bricks", "<u4"), ("flags", "<u4"), ("radius", "<u4"), ("stamp", "<u4"), ("n_obstacle_cells", "<i8"),
                            ("n_near_cells", "<i8")])
WORLD_DISTANCE_RESULT = np.dtype([("cell", "<i4", (3,)), ("nearest", "<i4", (3,)), ("d2", "<u4"), ("distance", "<f4")])
assert WORLD_ESDF_OPTIONS.itemsize == 32 and WORLD_ESDF_INFO.itemsize == 32 and WORLD_DISTANCE_RESULT.itemsize == 32
WORLD_ESDF_UNKNOWN_IS_OBSTACLE = 0x1
WORLD_ESDF_STATIC_ONLY = 0x2
WORLD_ESDF_BOX = 0x4
WORLD_ESDF_MAX_RADIUS = 16
WORLD_ESDF_NONE = 0xFFFF          # in world_esdf()'s d2
WORLD_ESDF_FAR = 0xFFFFFFFE       # in a WORLD_DISTANCE_RESULT's d2
# world ground layer (sdm.h: sdm_world_ground_update / sdm_get_world_ground / sdm_query_world_ground / sdm_query_world_footprints)
WORLD_GROUND_OPTIONS = np.dtype([("flags", "<u4"), ("up_axis", "<i4"), ("up_sign", "<i4"), ("h_lo", "<i4"), ("h_hi", "<i4"), ("clearance", "<u4"),
                                 ("max_step", "<u4"), ("radius", "<u4"), ("tmin", "<i4", (2,)), ("tmax", "<i4", (2,)),
                                 ("support_labels", "<u4", (8,))])
WORLD_GROUND_INFO = np.dtype([("n_tiles", "<u4"), ("level_min", "<u4"), ("level_max", "<u4"), ("stamp", "<u4"), ("n_ground", "<i8"),
                              ("n_obstacle", "<i8"), ("n_none", "<i8"), ("n_step", "<i8"), ("n_lethal", "<i8"), ("options", WORLD_GROUND_OPTIONS)])
WORLD_GROUND_RESULT = np.dtype([("col", "<i4", (2,)), ("d2", "<u4"), ("surface", "<f4"), ("above", "<i4"), ("cell", GROUND_CELL), ("dist", "<f4"),
                                ("status", "<u4"), ("pad", "<u4")])
WORLD_FOOTPRINT_RESULT = np.dtype([("n_cols", "<u4"), ("n_lethal", "<u4"), ("n_none", "<u4"), ("n_ground", "<u4"), ("n_absent", "<u4"),
                                   ("level_min", "<u2"), ("level_max", "<u2"), ("min_d2", "<u4"), ("first_lethal", "<i4", (2,)), ("pad", "<u4")])
assert WORLD_GROUND_OPTIONS.itemsize == 80 and WORLD_GROUND_INFO.itemsize == 136
assert WORLD_GROUND_RESULT.itemsize == 40 and WORLD_FOOTPRINT_RESULT.itemsize == 40
WORLD_GROUND_UNKNOWN_PASSABLE = 0x1
WORLD_GROUND_IGNORE_MOVABLE = 0x2
WORLD_GROUND_NONE_IS_LETHAL = 0x4
WORLD_GROUND_ABSENT_IS_LETHAL = 0x8
WORLD_GROUND_BOX = 0x10
WORLD_GROUND_MAX_SPAN = 4096
WORLD_GROUND_MAX_RADIUS = 16
WORLD_GROUND_NONE = 0xFFFF        # in world_ground()'s d2
WORLD_GROUND_FAR = 0xFFFFFFFE     # in a WORLD_GROUND_RESULT's d2 and a WORLD_FOOTPRINT_RESULT's min_d2
# world ground reach (sdm.h: sdm_world_ground_reach_update / sdm_get_world_ground_reach / sdm_query_world_ground_reach /
# sdm_world_ground_reach_paths)
WORLD_GROUND_REACH_OPTIONS = np.dtype([("flags", "<u4"), ("min_d2", "<u4"), ("soft_d2", "<u4"), ("penalty", "<u4"), ("max_climb", "<u4"),
                                       ("max_cost", "<u4"), ("tmin", "<i4", (2,)), ("tmax", "<i4", (2,)), ("pad", "<u4", (2,))])
WORLD_GROUND_REACH_INFO = np.dtype([("n_tiles", "<u4"), ("n_starts_used", "<u4"), ("n_traversable", "<u4"), ("n_reached", "<u4"),
                                    ("max_cost_reached", "<u4"), ("rounds", "<u4"), ("stamp", "<u4"), ("pad", "<u4"),
                                    ("options", WORLD_GROUND_REACH_OPTIONS)])
WORLD_GROUND_REACH_RESULT = np.dtype([("cost", "<u4"), ("metres", "<f4"), ("col", "<i4", (2,)), ("level", "<u2"), ("next", "u1"), ("status", "u1"),
                                      ("pad", "<u4")])
assert WORLD_GROUND_REACH_OPTIONS.itemsize == 48 and WORLD_GROUND_REACH_INFO.itemsize == 80 and WORLD_GROUND_REACH_RESULT.itemsize == 24
WORLD_GROUND_REACH_FACE_CONNECTED = 0x1
WORLD_GROUND_REACH_BOX = 0x2
WORLD_GROUND_REACH_BYTES_PER_TILE = 464

WORLD_SEGMENT_HIT = np.dtype([("t", "<f4"), ("cells", "<i4"), ("cell", "<i4", (3,)), ("track", "<u2"), ("label", "u1"), ("occ", "i1"),
                              ("unknown", "<i4"), ("stamp", "<u4")])
WORLD_RAYS_IGNORE_MOVABLE = 0x10
WORLD_SEGMENT_MAX_CELLS = 8192
WORLD_VIEW_MAX_REACH = 255

# the world mesh (sdm.h: sdm_world_mesh_update / sdm_get_world_mesh_info / sdm_get_world_mesh_faces / sdm_get_world_mesh_vertices /
# sdm_world_mesh_device)
WORLD_MESH_OPTIONS = np.dtype([("flags", "<u4"), ("track", "<i4"), ("labels", "<u4", (8,)), ("bmin", "<i4", (3,)), ("bmax", "<i4", (3,)),
                               ("max_faces", "<i8"), ("max_vertices", "<i8")])
WORLD_MESH_FACE = np.dtype([("brick", "<u4"), ("cell", "<u2"), ("dir", "u1"), ("kind", "u1"), ("track", "<u2"), ("label", "u1"), ("occ", "i1")])
WORLD_MESH_INFO = np.dtype([("n_bricks", "<u4"), ("n_vertex_bricks", "<u4"), ("n_faces", "<i8"), ("n_vertices", "<i8"), ("n_solid", "<i8"),
                            ("faces_by_dir", "<i8", (6,)), ("faces_by_kind", "<i8", (4,)), ("stamp", "<u4"), ("pad", "<u4"),
                            ("options", WORLD_MESH_OPTIONS)])
assert WORLD_MESH_OPTIONS.itemsize == 80 and WORLD_MESH_FACE.itemsize == 12 and WORLD_MESH_INFO.itemsize == 200
WORLD_MESH_STATIC_ONLY = 0x01
WORLD_MESH_MOVABLE_ONLY = 0x02
WORLD_MESH_OBSERVED_ONLY = 0x04
WORLD_MESH_SKIP_UNKNOWN_FACES = 0x08
WORLD_MESH_SKIP_ABSENT_FACES = 0x10
WORLD_MESH_BOX = 0x20
WORLD_MESH_BYTES_PER_ARCHIVED_BRICK = 200
WORLD_MESH_BYTES_PER_BRICK = 132
WORLD_MESH_BYTES_PER_VERTEX_SLOT = 80
WORLD_MESH_BYTES_PER_VERTEX_BRICK = 48
WORLD_MESH_BYTES_PER_FACE = 28
WORLD_MESH_BYTES_PER_VERTEX = 12

# world objects (sdm.h: sdm_world_objects_update / sdm_get_world_objects / sdm_get_world_object_cells /
# sdm_get_world_object_labels / sdm_query_world_objects)
WORLD_OBJECTS_OPTIONS = np.dtype([("flags", "<u4"), ("min_cells", "<i4"), ("max_cells", "<i8"), ("labels", "<u4", (8,)), ("bmin", "<i4", (3,)),
                                  ("bmax", "<i4", (3,))])
WORLD_OBJECT = np.dtype([("first_index", "<u4"), ("n_cells", "<u4"), ("n_guessed", "<u4"), ("track", "<u2"), ("label", "u1"), ("mixed_tracks", "u1"),
                         ("first_cell", "<i4", (3,)), ("cell_min", "<i4", (3,)), ("cell_max", "<i4", (3,)), ("pad0", "<u4"),
                         ("cell_sum", "<i8", (3,)), ("cell_sq", "<i8", (6,)), ("box_min", "<f4", (3,)), ("box_max", "<f4", (3,)),
                         ("centroid", "<f4", (3,)), ("pad1", "<u4")])
WORLD_OBJECTS_INFO = np.dtype([("n_bricks", "<u4"), ("n_objects", "<u4"), ("n_objects_total", "<u4"), ("flags", "<u4"), ("n_cells", "<i8"),
                               ("n_guessed", "<i8"), ("min_cells", "<i4"), ("stamp", "<u4")])
WORLD_OBJECT_RESULT = np.dtype([("cell", "<i4", (3,)), ("object", "<u4"), ("index", "<u4"), ("pad", "<u4")])
assert WORLD_OBJECTS_OPTIONS.itemsize == 72 and WORLD_OBJECT.itemsize == 168 and WORLD_OBJECTS_INFO.itemsize == 40
assert WORLD_OBJECT_RESULT.itemsize == 24
WORLD_OBJECTS_FACE_CONNECTED = 0x01
WORLD_OBJECTS_BOX = 0x02
WORLD_OBJECTS_BY_TRACK = 0x04
WORLD_OBJECTS_STATIC_ONLY = 0x08
WORLD_OBJECTS_MOVABLE_ONLY = 0x10
WORLD_OBJECTS_OBSERVED_ONLY = 0x20
WORLD_OBJECT_UNLISTED = 0xFFFFFFFE   # a counted cell of an object below min_cells
WORLD_OBJECT_NONE = 0xFFFFFFFF       # no counted cell of the field
WORLD_OBJECTS_BYTES_PER_ARCHIVED_BRICK = 8
WORLD_OBJECTS_BYTES_PER_BRICK = 240
WORLD_OBJECTS_BYTES_PER_CELL = 28
WORLD_OBJECTS_BYTES_PER_OBJECT = 288
ALL_LABELS = tuple(range(256))

# world changes (sdm.h: sdm_world_changes_update / sdm_get_world_changes / sdm_get_world_change_cells /
# sdm_get_world_change_labels / sdm_query_world_changes); the client is the class WorldChanges below
WORLD_CHANGES_COUNTERS = ("n_appeared", "n_vanished", "n_relabelled", "n_same_occupied", "n_same_free", "n_new_occupied", "n_new_free",
                          "n_remembered", "n_known_now", "n_known_before", "n_outside")
WORLD_CHANGES_OPTIONS = np.dtype([("flags", "<u4"), ("min_cells", "<i4"), ("max_cells", "<i8"), ("labels", "<u4", (8,)), ("classes", "<u4"),
                                  ("max_last_stamp", "<u4"), ("pad", "<u4", (2,))])
WORLD_CHANGE_REGION = np.dtype([("first_index", "<u4"), ("n_cells", "<u4"), ("cls", "u1"), ("label_now", "u1"), ("label_before", "u1"),
                                ("mixed", "u1"), ("first_cell", "<i4", (3,)), ("cell_min", "<i4", (3,)), ("cell_max", "<i4", (3,)),
                                ("cell_sum", "<i8", (3,)), ("box_min", "<f4", (3,)), ("box_max", "<f4", (3,)), ("centroid", "<f4", (3,)),
                                ("pad", "<u4")])
WORLD_CHANGES_INFO = np.dtype([(name, "<u8") for name in WORLD_CHANGES_COUNTERS] +
                              [("n_candidates", "<u4"), ("n_bricks", "<u4"), ("n_cells", "<i8"), ("n_regions", "<u4"), ("n_regions_total", "<u4"),
                               ("flags", "<u4"), ("min_cells", "<i4"), ("frame_stamp", "<u4"), ("stamp", "<u4")])
WORLD_CHANGE_RESULT = np.dtype([("cell", "<i4", (3,)), ("region", "<u4"), ("index", "<u4"), ("cls", "<u4")])
assert WORLD_CHANGES_OPTIONS.itemsize == 64 and WORLD_CHANGE_REGION.itemsize == 112 and WORLD_CHANGES_INFO.itemsize == 128
assert WORLD_CHANGE_RESULT.itemsize == 24
WORLD_CHANGES_FACE_CONNECTED = 0x01
WORLD_CHANGES_BY_LABEL = 0x02
WORLD_CHANGES_STATIC_ONLY = 0x04
WORLD_CHANGES_OBSERVED_ONLY = 0x08
WORLD_CHANGES_OLDER = 0x10
WORLD_CHANGE_APPEARED, WORLD_CHANGE_VANISHED, WORLD_CHANGE_RELABELLED = 1, 2, 3
ALL_CHANGE_CLASSES = (WORLD_CHANGE_APPEARED, WORLD_CHANGE_VANISHED, WORLD_CHANGE_RELABELLED)
WORLD_CHANGE_UNLISTED = 0xFFFFFFFE   # a listed cell of a region below min_cells
WORLD_CHANGE_NONE = 0xFFFFFFFF       # no listed cell
WORLD_CHANGES_BYTES_PER_CANDIDATE = 204
WORLD_CHANGES_BYTES_PER_BRICK = 368
WORLD_CHANGES_BYTES_PER_CELL = 37
WORLD_CHANGES_BYTES_PER_REGION = 176

STATE_FIELDS = [("px", np.float32), ("py", np.float32), ("pz", np.float32), ("w", np.float32),
                ("ts", np.uint16), ("track", np.uint16), ("label", np.uint8), ("status", np.uint8),
                ("forget", np.uint8), ("owner", np.uint16)]

STAGES = {"all": 0, "ego": 1, "move": 2, "remove": 3, "visibility": 4, "weight": 5, "birth": 6, "occupancy": 7}
INPUT_ON_DEVICE = 0x1
SKIP_OCCUPANCY = 0x2
NO_INSTANCES = 0x4     # sdm_update_raw: ignore the object masks (g_consider_instance == false)

STATUS_NAMES = {0: "SDM_OK", 1: "SDM_ERR_INVALID_ARGUMENT", 2: "SDM_ERR_NO_DEVICE", 3: "SDM_ERR_HIP",
                4: "SDM_ERR_CAPACITY", 5: "SDM_ERR_NOT_CONVERGED", 6: "SDM_ERR_COMM"}


def label_mask(labels):
    """the 256-bit label mask of sdm_ground_options::support_labels: bit l of word l // 32 for every label id given"""
    m = np.zeros(8, np.uint32)
    for l in ([] if labels is None else labels):
        if not 0 <= int(l) <= 255:
            raise ValueError("label %r is not in 0..255" % (l,))
        m[int(l) >> 5] |= np.uint32(1 << (int(l) & 31))
    return m


def mesh_triangles(quads):
    """[n, 4] vertex ids of quads (q0, q1, q2, q3) -> [2n, 3]: the triangles (q0, q1, q2) and (q0, q2, q3) of each, in
    the quads' order and with their winding"""
    q = np.asarray(quads).reshape(-1, 4)
    return q[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)


def write_ply(path, xyz, quads, face_rgb=None):
    """ASCII PLY of a mesh: vertices xyz [m, 3], two triangles per quad (mesh_triangles), optionally one colour per quad
    (face_rgb [n, 3], 0..255) written to both of its triangles.  Plain host code."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    tri = mesh_triangles(quads)
    rgb = None
    if face_rgb is not None:
        rgb = np.repeat(np.asarray(face_rgb).reshape(-1, 3).astype(np.uint8), 2, axis=0)
        if len(rgb) != len(tri):
            raise ValueError("face_rgb needs one colour per quad")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(xyz))
        f.write("element face %d\nproperty list uchar int vertex_indices\n" % len(tri))
        if rgb is not None:
            f.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        f.write("end_header\n")
        for p in xyz:
            f.write("%.9g %.9g %.9g\n" % (p[0], p[1], p[2]))   # (9 digits: float32 round-trips)
        for k, t in enumerate(tri):
            f.write("3 %d %d %d" % (t[0], t[1], t[2]))
            f.write(" %d %d %d\n" % tuple(rgb[k]) if rgb is not None else "\n")


def ground_band(cfg, origin, up, lo_m, hi_m):
    """the ground layer's band from metres: global coordinates lo_m <= hi_m along the up axis -> (h_lo, h_hi), the heights
    of the cells that hold them, clamped to the map.  cfg: the map's configuration (dict); origin: the global position of
    the min corner of cell (0, 0, 0) (ground()'s, or map centre + pmin); up: (axis, sign).  Host arithmetic in float64."""
    axis, sign = int(up[0]), int(up[1])
    if axis not in (0, 1, 2) or sign not in (1, -1) or not lo_m <= hi_m:
        raise ValueError("up must be (0..2, +1 / -1) and lo_m <= hi_m")
    n = 1 << int(cfg[("x_n", "y_n", "z_n")[axis]])
    idx = [int(np.clip(np.floor((float(m) - float(origin[axis])) / float(cfg["voxel_size"])), 0, n - 1)) for m in (lo_m, hi_m)]
    h = idx if sign > 0 else [n - 1 - i for i in idx]
    return min(h), max(h)


def world_ground_band(voxel_size, up, lo_m, hi_m):
    """the world ground layer's band from metres: world coordinates lo_m <= hi_m along the up axis -> (h_lo, h_hi), the
    heights of the world cells that hold them (cell = floor(p / voxel_size); h = g for sign +1, -1 - g for -1).  up: (axis,
    sign).  Host arithmetic in float64; the span is the caller's to keep within WORLD_GROUND_MAX_SPAN."""
    axis, sign = int(up[0]), int(up[1])
    if axis not in (0, 1, 2) or sign not in (1, -1) or not lo_m <= hi_m:
        raise ValueError("up must be (0..2, +1 / -1) and lo_m <= hi_m")
    g = [int(np.floor(float(m) / float(voxel_size))) for m in (lo_m, hi_m)]
    h = g if sign > 0 else [-1 - v for v in g]
    return min(h), max(h)


class Config(C.Structure):
    _fields_ = [("x_n", C.c_int32), ("y_n", C.c_int32), ("z_n", C.c_int32), ("p_n", C.c_int32),
                ("voxel_size", C.c_float),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32),
                ("depth_min", C.c_float), ("depth_max", C.c_float),
                ("window_half", C.c_int32), ("max_movable_track", C.c_int32),
                ("device", C.c_int32), ("shard_rank", C.c_int32), ("shard_count", C.c_int32),
                ("max_visible", C.c_int64)]


class Params(C.Structure):
    _fields_ = [("detection_probability", C.c_float), ("noise_number", C.c_float),
                ("nb_ptc_num_per_point", C.c_int32), ("occupancy_threshold", C.c_float),
                ("max_obersevation_lost_time", C.c_int32), ("forgetting_rate", C.c_float),
                ("max_forget_count", C.c_int32), ("match_score_threshold", C.c_float),
                ("id_transition_probability", C.c_float),
                ("if_consider_depth_noise", C.c_int32), ("if_use_independent_filter", C.c_int32),
                ("depth_noise_first_order", C.c_float), ("depth_noise_zero_order", C.c_float)]


class InstanceMask(C.Structure):
    _fields_ = [("track_id", C.c_int32), ("label_id", C.c_int32), ("mask", C.c_void_p)]


class RawOptions(C.Structure):
    _fields_ = [("src_width", C.c_int32), ("src_height", C.c_int32), ("rescale", C.c_float), ("sky_instance", C.c_int32),
                ("object_bbox", C.c_void_p)]


class RingState(C.Structure):
    _fields_ = [("global_time_stamp", C.c_uint32), ("moved_steps", C.c_int32 * 3), ("eq_steps", C.c_int32 * 3),
                ("map_center", C.c_float * 3), ("last_pos", C.c_float * 3),
                ("birth_cursor", C.c_int32), ("move_cursor", C.c_int32)]


class ColourConfig(C.Structure):
    _fields_ = [("label_bgr", (C.c_uint8 * 3) * 256), ("perm", C.c_uint8 * 256), ("background_label", C.c_int32),
                ("colour_by_label", C.c_int32), ("jet_axis", C.c_int32), ("evaluation_format", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("live_particles", C.c_int64), ("n_visible", C.c_int64), ("n_birth_attempts", C.c_int64),
                ("n_birth_success", C.c_int64), ("n_resampled_voxels", C.c_int64), ("n_moved", C.c_int64),
                ("n_move_reinserted", C.c_int64), ("n_frustum_voxels", C.c_int64), ("n_occupied", C.c_int64),
                ("flood_rounds", C.c_int64), ("bfs_start_in_frustum", C.c_int64), ("live_voxels", C.c_int64), ("sweep_live_voxels", C.c_int64),
                ("sweep_tiles", C.c_int64),
                ("stage_ms", C.c_double * 8), ("restamped_slabs", C.c_int64 * 3),
                ("graph_frames", C.c_int64), ("direct_frames", C.c_int64), ("host_enqueue_us", C.c_double),
                ("halo_dropped", C.c_int64), ("alias_entries", C.c_int64), ("alias_overflowed", C.c_int64)]


class SdmError(RuntimeError):
    pass


_lib = None


HOST_NUMA_NODE = None  # what sdm_bind_host_thread answered when the library was loaded (-1: nothing done)


def load_library():
    """Load libsdm_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SdmError("libsdm_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "or `make -C semantic_dsp_map_amd/csrc`.  There is no CPU path.")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    i32, u32, i64 = C.c_int32, C.c_uint32, C.c_int64
    sig = {
        "sdm_create": [C.POINTER(Config), C.POINTER(vp)],
        "sdm_destroy": [vp],
        "sdm_clear": [vp],
        "sdm_set_params": [vp, C.POINTER(Params)],
        "sdm_generate_noise_table": [vp, C.c_uint64, i32, C.c_float],
        "sdm_upload_noise_table": [vp, vp, i32],
        "sdm_download_noise_table": [vp, vp, i32],
        "sdm_download_pdf_table": [vp, vp, i32],
        "sdm_update": [vp, vp, vp, vp, vp, vp, i32, vp, i32, u32, i32],
        "sdm_update_raw": [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, i32, u32, i32],
        "sdm_update_raw_ex": [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, i32, u32, i32, vp],
        "sdm_get_labeled_cloud": [vp, vp],
        "sdm_host_alloc": [C.c_size_t, C.POINTER(vp)],
        "sdm_host_free": [vp],
        "sdm_update_begin": [vp, vp, vp, vp, vp, vp, i32, vp, i32, u32, i32, C.POINTER(vp)],
        "sdm_update_finish": [vp, vp, i32, u32, i32],
        "sdm_frame_start": [vp, vp, vp, vp, vp, vp, i32, vp, i32, u32, i32],
        "sdm_frame_moves": [vp],
        "sdm_frame_moves_pending": [vp, C.POINTER(C.c_int32)],
        "sdm_frame_predict": [vp, C.POINTER(vp)],
        "sdm_set_halo_buffers": [vp, vp, vp, vp, vp, i32],
        "sdm_comm_unique_id": [vp],
        "sdm_comm_init": [vp, vp, i32],
        "sdm_ipc_create": [vp, i32, vp],
        "sdm_ipc_connect": [vp, vp],
        "sdm_update_sharded": [vp, vp, vp, vp, vp, vp, i32, vp, i32, u32],
        "sdm_ck_chunk_elems": [vp, C.POINTER(i64)],
        "sdm_ck_reduce": [vp, vp, vp],
        "sdm_comm_timing": [vp, i32],
        "sdm_get_comm_times": [vp, vp],
        "sdm_device_alloc": [vp, C.c_size_t, C.POINTER(vp)],
        "sdm_device_free": [vp, vp],
        "sdm_device_upload": [vp, vp, vp, C.c_size_t],
        "sdm_device_download": [vp, vp, vp, C.c_size_t],
        "sdm_device_synchronize": [vp],
        "sdm_stream": [vp, C.POINTER(vp)],
        "sdm_set_stream": [vp, vp],
        "sdm_set_ck_buffer": [vp, vp],
        "sdm_synchronize": [vp],
        "sdm_get_voxels": [vp, vp],
        "sdm_get_occupied": [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), i32],
        "sdm_get_occupied_rgb": [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), i32],
        "sdm_get_freespace_rgb": [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), i32],
        "sdm_set_colours": [vp, vp],
        "sdm_get_freespace": [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), i32],
        "sdm_voxels_device_ptr": [vp, C.POINTER(vp)],
        "sdm_query_points": [vp, vp, i64, vp, vp, u32],
        "sdm_query_segments": [vp, vp, i64, vp, u32],
        "sdm_query_boxes": [vp, vp, i64, vp, u32],
        "sdm_esdf_update": [vp, u32],
        "sdm_get_esdf": [vp, vp, vp, vp],
        "sdm_query_distance": [vp, vp, i64, vp, u32],
        "sdm_instances_update": [vp, u32],
        "sdm_get_instances": [vp, vp, i32, C.POINTER(i32), vp],
        "sdm_get_label_cells": [vp, vp],
        "sdm_frontiers_update": [vp, u32, i32, i64],
        "sdm_get_frontier_clusters": [vp, vp, i32, C.POINTER(i32), vp],
        "sdm_get_frontier_cells": [vp, vp, vp, vp, i64, C.POINTER(i64)],
        "sdm_query_views": [vp, vp, i64, vp, i32, vp, vp, vp, u32],
        "sdm_debug_view_batch": [vp, i32],
        "sdm_reach_update": [vp, vp, vp, i64, u32, u32, u32],
        "sdm_get_reach": [vp, vp, vp, vp],
        "sdm_query_reach": [vp, vp, vp, i64, vp, u32],
        "sdm_reach_paths": [vp, vp, vp, i64, i32, vp, vp, u32],
        "sdm_debug_reach_tiles": [vp, C.POINTER(i64)],
        "sdm_ground_update": [vp, vp],
        "sdm_get_ground": [vp, vp, vp, vp, vp],
        "sdm_query_ground": [vp, vp, i64, vp, u32],
        "sdm_query_footprints": [vp, vp, i64, vp, u32],
        "sdm_mesh_update": [vp, vp],
        "sdm_get_mesh_info": [vp, vp, vp],
        "sdm_get_mesh_faces": [vp, vp, vp, i64, C.POINTER(i64)],
        "sdm_get_mesh_vertices": [vp, vp, vp, i64, C.POINTER(i64)],
        "sdm_mesh_device": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)],
        "sdm_world_update": [vp, vp],
        "sdm_world_clear": [vp],
        "sdm_get_world_info": [vp, vp],
        "sdm_get_world_bricks": [vp, vp, vp, i64, i64, C.POINTER(i64)],
        "sdm_get_world_occupied": [vp, vp, i64, C.POINTER(i64), u32],
        "sdm_query_world_points": [vp, vp, i64, vp, u32],
        "sdm_get_world_region": [vp, vp, vp, vp, u32],
        "sdm_world_import": [vp, vp, vp, vp, i64],
        "sdm_world_retain": [vp, vp, C.POINTER(i64)],
        "sdm_world_match": [vp, vp, vp, vp, i64, vp, vp],
        "sdm_world_reach_update": [vp, vp, vp, vp, i64],
        "sdm_get_world_reach": [vp, vp, vp, i64, i64, C.POINTER(i64), vp],
        "sdm_query_world_reach": [vp, vp, vp, i64, vp, u32],
        "sdm_world_reach_paths": [vp, vp, vp, i64, i32, vp, vp, u32],
        "sdm_debug_world_reach_bricks": [vp, C.POINTER(i64)],
        "sdm_world_frontiers_update": [vp, vp],
        "sdm_get_world_frontier_clusters": [vp, vp, i32, C.POINTER(i32), vp],
        "sdm_get_world_frontier_cells": [vp, vp, vp, vp, i64, i64, C.POINTER(i64)],
        "sdm_world_objects_update": [vp, vp],
        "sdm_get_world_objects": [vp, vp, i32, C.POINTER(i32), vp],
        "sdm_get_world_object_cells": [vp, vp, vp, vp, i64, i64, C.POINTER(i64)],
        "sdm_get_world_object_labels": [vp, vp, vp],
        "sdm_query_world_objects": [vp, vp, vp, i64, vp, u32],
        "sdm_world_changes_update": [vp, vp],
        "sdm_get_world_changes": [vp, vp, i32, C.POINTER(i32), vp],
        "sdm_get_world_change_cells": [vp, vp, vp, vp, vp, vp, i64, i64, C.POINTER(i64)],
        "sdm_get_world_change_labels": [vp, vp, vp, vp],
        "sdm_query_world_changes": [vp, vp, vp, i64, vp, u32],
        "sdm_world_esdf_update": [vp, vp],
        "sdm_get_world_esdf": [vp, vp, vp, vp, i64, i64, C.POINTER(i64), vp],
        "sdm_query_world_distance": [vp, vp, vp, i64, vp, u32],
        "sdm_world_ground_update": [vp, vp],
        "sdm_get_world_ground": [vp, vp, vp, vp, i64, i64, C.POINTER(i64), vp],
        "sdm_query_world_ground": [vp, vp, vp, i64, vp, u32],
        "sdm_query_world_footprints": [vp, vp, i64, vp, u32],
        "sdm_world_ground_reach_update": [vp, vp, vp, vp, i64],
        "sdm_get_world_ground_reach": [vp, vp, vp, i64, i64, C.POINTER(i64), vp],
        "sdm_query_world_ground_reach": [vp, vp, vp, i64, vp, u32],
        "sdm_world_ground_reach_paths": [vp, vp, vp, i64, i32, vp, vp, u32],
        "sdm_debug_world_ground_reach_tiles": [vp, C.POINTER(i64)],
        "sdm_query_world_segments": [vp, vp, i64, vp, u32],
        "sdm_query_world_views": [vp, vp, i64, vp, i32, i32, vp, vp, u32],
        "sdm_world_mesh_update": [vp, vp],
        "sdm_get_world_mesh_info": [vp, vp],
        "sdm_get_world_mesh_faces": [vp, vp, vp, vp, i64, i64, C.POINTER(i64)],
        "sdm_get_world_mesh_vertices": [vp, vp, vp, i64, i64, C.POINTER(i64)],
        "sdm_world_mesh_device": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)],
        "sdm_debug_world_view_batch": [vp, i32],
        "sdm_forecast_stamps": [C.c_float, vp, i32, vp, i32, u32, vp, i64, C.POINTER(i64)],
        "sdm_forecast_update": [vp, vp, i32, vp, i32, u32],
        "sdm_get_forecast": [vp, vp, vp, vp, vp],
        "sdm_get_forecast_cells": [vp, vp, vp, vp, i64, C.POINTER(i64)],
        "sdm_query_forecast": [vp, vp, i64, vp, u32],
        "sdm_query_forecast_segments": [vp, vp, i64, vp, u32],
        "sdm_object_particle_count": [vp, i32, C.POINTER(i64)],
        "sdm_tracks_with_particles": [vp, vp, i32, C.POINTER(i32)],
        "sdm_comm_set_options": [vp, i32, i32],
        "sdm_get_stats": [vp, C.POINTER(Stats), i32],
        "sdm_set_profiling": [vp, i32],
        "sdm_debug_force_generic_flood": [vp, i32],
        "sdm_get_ring_state": [vp, C.POINTER(RingState)],
        "sdm_set_ring_state": [vp, C.POINTER(RingState)],
        "sdm_get_stamps": [vp, vp, vp, vp],
        "sdm_set_stamps": [vp, vp, vp, vp],
        "sdm_dump_state": [vp] + [vp] * 10,
        "sdm_load_state": [vp] + [vp] * 10,
        "sdm_get_ck_kappa": [vp, vp],
        "sdm_get_bin_counts": [vp, vp],
        "sdm_get_bins": [vp, vp, i64, C.POINTER(i64)],
        "sdm_get_extrinsic": [vp, vp],
        "sdm_time_occupancy_sweep": [vp, i32, C.POINTER(C.c_float)],
        "sdm_set_issue_mode": [vp, i32],
        "sdm_bind_host_thread": [i32],
        "sdm_host_numa_node_early": [i32],
        "sdm_debug_fill_dense": [vp],
        "sdm_debug_fill_dense_ex": [vp, i32],
        "sdm_debug_hinted_groups": [vp, C.POINTER(C.c_int64)],
        "sdm_debug_sweep_lists": [vp, i32],
        "sdm_debug_sweep_mode": [vp, C.POINTER(i32)],
        "sdm_debug_alias_cap": [vp, i32],
        "sdm_test_scan": [vp, vp, i64],
        "sdm_test_sort_pairs": [vp, vp, vp, vp, i64, i32],
        "sdm_test_scratch_elems": [i32, i64, C.POINTER(i64)],
        "sdm_test_scan_seq": [i32, vp, vp, u32, vp, vp, C.POINTER(i32), vp],
        "sdm_test_sort_pairs_seq": [i32, vp, vp, vp, u32, vp, vp, vp, vp, vp, C.POINTER(i32), vp],
    }
    for name, argtypes in sig.items():
        fn = getattr(L, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    L.sdm_last_error.restype = C.c_char_p
    L.sdm_version.restype = C.c_char_p
    # The process belongs on the NUMA node of its GPU before the HIP runtime makes its first allocations (sdm.h,
    # sdm_bind_host_thread; SDM_NUMA_BIND=0 switches it off): nothing of HIP has been called yet at this point.
    global HOST_NUMA_NODE
    HOST_NUMA_NODE = L.sdm_bind_host_thread(int(os.environ.get("LOCAL_RANK", "0")))
    _lib = L
    return L


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


def _check(L, rc, what):
    if rc != 0:
        raise SdmError("%s failed: %s (%s)" % (what, STATUS_NAMES.get(rc, rc), L.sdm_last_error().decode()))


def _call(name, *args):
    """Calls the library function `name`, which takes no map, and raises SdmError on any status but SDM_OK."""
    L = load_library()
    _check(L, getattr(L, name)(*args), name)


def _dev(p):
    """an optional device address as a pointer: a falsy one (None, 0) is the null pointer"""
    return _ptr(int(p)) if p else None


def _goals(xyz, cells, cell_dtype, cell_row):
    """The goal form "exactly one of xyz / cells" -> (positions float32 [n, 3] or None, cells of cell_dtype shaped cell_row or
    None, n).  With neither, n is 0 and the library refuses the call."""
    p = None if xyz is None else np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    w = None if cells is None else np.ascontiguousarray(cells, dtype=cell_dtype).reshape(cell_row)
    return p, w, len(p) if p is not None else len(w) if w is not None else 0


def _rows6(a, b, on_device):
    """two (n, 3) arrays side by side as float32 [n, 6]; on_device: a already is the device address of such rows and b None"""
    if on_device:
        assert b is None
        return a
    return np.concatenate([np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)], axis=1)


_WORDS = (np.uint32, (-1,))        # how the block's layers name a cell: its map-index word
_WORLD_CELLS = (np.int32, (-1, 3))  # how the world layers name one: (x, y, z)


class SdmMap:
    """One map on one GPU (or one Z-slab shard of a map)."""

    def __init__(self, cfg, params=None, noise_table=None, device=0, shard_rank=0, shard_count=1, max_visible=0):
        self.L = load_library()
        c = Config()
        for k, _ in Config._fields_:
            if k in cfg:
                setattr(c, k, cfg[k])
        c.device, c.shard_rank, c.shard_count, c.max_visible = device, shard_rank, shard_count, max_visible
        self.cfg = c
        h = C.c_void_p()
        _check(self.L, self.L.sdm_create(C.byref(c), C.byref(h)), "sdm_create")
        self.h = h
        self.V = 1 << (c.x_n + c.y_n + c.z_n)
        self.S = 1 << c.p_n
        self.v_count = self.V // shard_count
        self.W, self.H = c.width, c.height
        if params is not None:
            self.set_params(params)
        if noise_table is not None:
            self.upload_noise_table(noise_table)

    def close(self):
        if getattr(self, "h", None):
            self.L.sdm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the calling protocols of sdm.h, each stated once; the methods below name the function and its types.
    def _call(self, name, *args):
        """Calls the library function `name` on this map and raises SdmError on any status but SDM_OK."""
        rc = getattr(self.L, name)(self.h, *args)
        if rc != 0:
            _check(self.L, rc, name)

    def _out(self, name, ctype, *args):
        """_call for a function whose last argument is one scalar it writes -> that scalar's value"""
        v = ctype()
        self._call(name, *args, C.byref(v))
        return v.value

    def _query(self, name, src, dtype, row, res, flags, on_device, n, out):
        """A batched query `name(map, in, n, out, flags)` in either of its modes (the comment above query_points).
        on_device: src and out are device addresses of n entries, QUERY_ON_DEVICE joins the flags and nothing is returned.
        Otherwise src becomes an array of dtype shaped `row`, and an array of res, one entry per row, is filled and returned.
        A function with a second, optional output takes res and out as pairs (None: not asked for) and returns a pair."""
        res, out = (res, out) if isinstance(res, tuple) else ((res,), (out,))
        if on_device:
            self._call(name, _ptr(int(src)), int(n), _ptr(int(out[0])), *[_dev(o) for o in out[1:]], flags | QUERY_ON_DEVICE)
            return None
        p = np.ascontiguousarray(src, dtype=dtype).reshape(row)
        r = [None if d is None else np.empty(len(p), d) for d in res]
        self._call(name, _ptr(p), len(p), *[_ptr(a) for a in r], flags)
        return r[0] if len(r) == 1 else tuple(r)

    def _goal_query(self, name, xyz, cells, cell_form, res, on_device, n, out):
        """_query for `name(map, xyz, cells, n, out, flags)`, whose entries come in the goal form (_goals); cell_form: _WORDS
        or _WORLD_CELLS.  on_device: the one given of xyz / cells is a device address, the other falsy."""
        if on_device:
            self._call(name, _dev(xyz), _dev(cells), int(n), _ptr(int(out)), QUERY_ON_DEVICE)
            return None
        p, w, n = _goals(xyz, cells, *cell_form)
        r = np.empty(n, res)
        self._call(name, _ptr(p), _ptr(w), n, _ptr(r), 0)
        return r

    def _goal_paths(self, name, xyz, cells, cell_form, max_len, fill, on_device, n, cells_out, len_out):
        """The same for `name(map, xyz, cells, n, max_len, cells_out, len_out, flags)` -> (rows of max_len cells in the cell
        form, holding `fill` where the call writes nothing; lengths int32 [n]).  on_device: cells_out may be falsy."""
        if on_device:
            self._call(name, _dev(xyz), _dev(cells), int(n), int(max_len), _dev(cells_out), _ptr(int(len_out)), QUERY_ON_DEVICE)
            return None
        p, w, n = _goals(xyz, cells, *cell_form)
        rows, lens = np.full((n, int(max_len)) + cell_form[1][1:], fill, cell_form[0]), np.zeros(n, np.int32)
        self._call(name, _ptr(p), _ptr(w), n, int(max_len), _ptr(rows), _ptr(lens), 0)
        return rows, lens

    def _window(self, name, cols, first=0, cap=None, info=None):
        """Count, then fetch, for `name(map, columns..., [first,] cap, &count[, info])`: one call with null columns for the
        count (and the info record, where info names its dtype), one for rows first .. first + cap - 1 of what there is (cap
        None: all of them).  cols: (dtype, shape of one row) per column, None for a column not asked for; first None: the
        function has no such argument -> (the columns, the info record or None, the count)"""
        got = C.c_int64(0)
        rec = None if info is None else np.zeros(1, info)
        at = () if first is None else (0,)
        self._call(name, *[None] * len(cols), *at, 0, C.byref(got), *(() if info is None else (_ptr(rec),)))
        take = max(min(got.value - int(first or 0), got.value if cap is None else int(cap)), 0)
        out = [None if c is None else np.empty((take,) + c[1], c[0]) for c in cols]
        at = () if first is None else (int(first),)
        self._call(name, *[_ptr(a) for a in out], *at, take, C.byref(got), *(() if info is None else (None,)))
        return out, None if info is None else rec[0], got.value

    def clear(self):
        self._call("sdm_clear")

    def set_params(self, params):
        p = Params()
        for k, _ in Params._fields_:
            setattr(p, k, params[k])
        self._call("sdm_set_params", C.byref(p))

    def generate_noise_table(self, seed=20250217, n=1000000, stddev=0.05):
        self._call("sdm_generate_noise_table", seed, n, stddev)

    def upload_noise_table(self, table):
        t = np.ascontiguousarray(table, dtype=np.float32)
        self._call("sdm_upload_noise_table", _ptr(t), t.size)

    def download_noise_table(self, n=1000000):
        t = np.empty(n, np.float32)
        self._call("sdm_download_noise_table", _ptr(t), n)
        return t

    def download_pdf_table(self):
        t = np.empty(20000, np.float32)
        self._call("sdm_download_pdf_table", _ptr(t), 20000)
        return t

    def _frame_args(self, depth, cloud, cam_pos, cam_q, moves, remove_tracks, on_device, flags, stop_after=None):
        """-> (the arrays the pointers point into, the arguments of a frame entry point behind the map: the frame, the flags
        and, where stop_after is given, the stage)"""
        keep = []
        if on_device:
            dp, cp = _ptr(int(depth)), _ptr(int(cloud))
        else:
            depth = np.ascontiguousarray(depth, dtype=np.float32)
            cloud = np.ascontiguousarray(cloud, dtype=LABELED_POINT)
            assert depth.size == self.W * self.H and cloud.size == self.W * self.H
            keep += [depth, cloud]
            dp, cp = _ptr(depth), _ptr(cloud)
        pos = np.ascontiguousarray(cam_pos, dtype=np.float32)
        q = np.ascontiguousarray(cam_q, dtype=np.float32)
        mv = np.ascontiguousarray(moves if moves is not None else np.zeros(0, OBJECT_MOVE), dtype=OBJECT_MOVE)
        rm = np.ascontiguousarray(remove_tracks if remove_tracks is not None else [], dtype=np.int32)
        keep += [pos, q, mv, rm]
        fl = flags | (INPUT_ON_DEVICE if on_device else 0)
        if stop_after is None:
            return keep, (dp, cp, _ptr(pos), _ptr(q), _ptr(mv) if mv.size else None, mv.size, _ptr(rm) if rm.size else None, rm.size, fl)
        return keep, (dp, cp, _ptr(pos), _ptr(q), _ptr(mv) if mv.size else None, mv.size, _ptr(rm) if rm.size else None, rm.size, fl,
                      STAGES[stop_after] if isinstance(stop_after, str) else stop_after)

    def update(self, depth, cloud, cam_pos, cam_q, moves=None, remove_tracks=None, stop_after="all",
               on_device=False, flags=0, sync=False):
        keep, args = self._frame_args(depth, cloud, cam_pos, cam_q, moves, remove_tracks, on_device, flags, stop_after)
        self._call("sdm_update", *args)
        if sync:
            self.synchronize()

    def update_raw(self, depth, static_mask, label_to_inst, objects, cam_pos, cam_q, moves=None, remove_tracks=None,
                   stop_after="all", flags=0, sync=False, src_size=None, rescale=1.0, sky_instance=-1, object_bbox=None,
                   on_device=False):
        """SURVEY row N1 on the device.  objects: list of (track_id, label_id, mask HxW uint8); pose in double.
        on_device: depth, static_mask and every object's mask are device pointers (device_put) instead of arrays."""
        tab = np.ascontiguousarray(label_to_inst, dtype=np.uint16)
        assert tab.size == 256
        arr = (InstanceMask * max(len(objects), 1))()
        if on_device:
            flags |= INPUT_ON_DEVICE
            depth = int(depth)
            sm = None if static_mask is None else int(static_mask)
            masks = [int(o[2]) for o in objects]
        else:
            depth = np.ascontiguousarray(depth, dtype=np.float32)
            sm = None if static_mask is None else np.ascontiguousarray(static_mask, dtype=np.uint8)
            masks = [np.ascontiguousarray(o[2], dtype=np.uint8) for o in objects]
        for k, o in enumerate(objects):
            arr[k].track_id, arr[k].label_id, arr[k].mask = int(o[0]), int(o[1]), masks[k] if on_device else masks[k].ctypes.data
        pos = np.ascontiguousarray(cam_pos, dtype=np.float64)
        q = np.ascontiguousarray(cam_q, dtype=np.float64)
        mv = np.ascontiguousarray(moves if moves is not None else np.zeros(0, OBJECT_MOVE), dtype=OBJECT_MOVE)
        rm = np.ascontiguousarray(remove_tracks if remove_tracks is not None else [], dtype=np.int32)
        st = STAGES[stop_after] if isinstance(stop_after, str) else stop_after
        opt = RawOptions()
        opt.src_width, opt.src_height = src_size if src_size else (0, 0)
        opt.rescale = float(rescale)
        opt.sky_instance = int(sky_instance)
        bb = None if object_bbox is None else np.ascontiguousarray(object_bbox, dtype=np.float64)
        opt.object_bbox = bb.ctypes.data if bb is not None else None
        self._call("sdm_update_raw_ex", _ptr(depth), _ptr(sm), _ptr(tab), C.cast(arr, C.c_void_p), len(objects), _ptr(pos), _ptr(q),
                   _ptr(mv) if mv.size else None, mv.size, _ptr(rm) if rm.size else None, rm.size, flags, st, C.byref(opt))
        if sync:
            self.synchronize()

    def labeled_cloud(self):
        out = np.empty(self.W * self.H, LABELED_POINT)
        self._call("sdm_get_labeled_cloud", _ptr(out))
        return out

    def update_begin(self, depth, cloud, cam_pos, cam_q, moves=None, remove_tracks=None, stop_after="all",
                     on_device=False, flags=0):
        keep, args = self._frame_args(depth, cloud, cam_pos, cam_q, moves, remove_tracks, on_device, flags, stop_after)
        return self._out("sdm_update_begin", C.c_void_p, *args)

    def frame_start(self, depth, cloud, cam_pos, cam_q, moves=None, remove_tracks=None, stop_after="all", on_device=False, flags=0):
        keep, args = self._frame_args(depth, cloud, cam_pos, cam_q, moves, remove_tracks, on_device, flags, stop_after)
        self._call("sdm_frame_start", *args)

    def frame_moves(self):
        self._call("sdm_frame_moves")

    def frame_moves_pending(self):
        """True: a further batch of a long object list has published its counts and waits for their exchange"""
        return bool(self._out("sdm_frame_moves_pending", C.c_int32))

    def frame_predict(self):
        return self._out("sdm_frame_predict", C.c_void_p)

    def set_halo_buffers(self, counts_local, counts_all, send, recv_all, cap_records):
        self._call("sdm_set_halo_buffers", _ptr(int(counts_local)), _ptr(int(counts_all)), _ptr(int(send)), _ptr(int(recv_all)), cap_records)

    def comm_init(self, id_bytes, halo_cap=0):
        buf = np.frombuffer(bytes(id_bytes), np.uint8).copy()
        assert buf.size == 128
        self._call("sdm_comm_init", _ptr(buf), halo_cap)

    def ipc_create(self, halo_cap=0):
        """This shard's receive arena for the exchanges without RCCL; returns its 64-byte hipIpc handle (sdm_ipc_create)."""
        buf = np.zeros(64, np.uint8)
        self._call("sdm_ipc_create", halo_cap, _ptr(buf))
        return buf.tobytes()

    def ipc_connect(self, handles_all):
        """handles_all: the handles of all shards, in shard order (shard_count x 64 bytes)"""
        buf = np.frombuffer(bytes(handles_all), np.uint8).copy()
        self._call("sdm_ipc_connect", _ptr(buf))

    def comm_set_options(self, ck_exchange=-1, timeout_ms=0):
        """ck_exchange: 0 chunk-owner reduction, 1 one all-gather of the whole partial images, -1 unchanged"""
        self._call("sdm_comm_set_options", ck_exchange, timeout_ms)

    def update_sharded(self, depth, cloud, cam_pos, cam_q, moves=None, remove_tracks=None, on_device=False, flags=0):
        keep, args = self._frame_args(depth, cloud, cam_pos, cam_q, moves, remove_tracks, on_device, flags)
        self._call("sdm_update_sharded", *args)

    def ck_chunk_elems(self):
        """pixels per shard of the chunk-owner ck exchange (sdm_ck_chunk_elems)"""
        return int(self._out("sdm_ck_chunk_elems", C.c_int64))

    def ck_reduce(self, stage_dev, full_dev):
        self._call("sdm_ck_reduce", _ptr(int(stage_dev)), _ptr(int(full_dev)))

    def comm_timing(self, on=True):
        self._call("sdm_comm_timing", 1 if on else 0)

    def comm_times(self):
        """GPU microseconds of the last sharded frame's collectives: counts, halo, ck all-to-all, ck all-gather."""
        out = np.zeros(4, np.float64)
        self._call("sdm_get_comm_times", _ptr(out))
        return dict(zip(("counts_allgather", "halo_alltoall", "ck_alltoall", "ck_allgather"), [float(x) for x in out]))

    def device_alloc(self, nbytes):
        return self._out("sdm_device_alloc", C.c_void_p, nbytes)

    def device_free(self, ptr):
        self._call("sdm_device_free", _ptr(int(ptr)))

    def device_upload(self, ptr, array):
        a = np.ascontiguousarray(array)
        self._call("sdm_device_upload", _ptr(int(ptr)), _ptr(a), a.nbytes)

    def device_put(self, array):
        a = np.ascontiguousarray(array)
        p = self.device_alloc(a.nbytes)
        self.device_upload(p, a)
        return p

    def device_download(self, ptr, nbytes, dtype=np.uint8):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype)
        self._call("sdm_device_download", _ptr(out), _ptr(int(ptr)), out.nbytes)
        return out

    def device_synchronize(self):
        self._call("sdm_device_synchronize")

    def update_finish(self, ck_parts_dev=None, n_parts=1, stop_after="all", flags=0):
        st = STAGES[stop_after] if isinstance(stop_after, str) else stop_after
        self._call("sdm_update_finish", _ptr(ck_parts_dev), n_parts, flags, st)

    def stream(self):
        return self._out("sdm_stream", C.c_void_p) or 0

    def set_stream(self, hip_stream):
        self._call("sdm_set_stream", _ptr(int(hip_stream)) if hip_stream else None)

    def set_ck_buffer(self, dev_ptr):
        self._call("sdm_set_ck_buffer", _ptr(int(dev_ptr)) if dev_ptr else None)

    def set_issue_mode(self, mode):
        """0 launch by launch, 1 branched graph, 2 by the host's speed, 3 chain graph, 4 five chain graphs (sdm.h SDM_ISSUE_*)"""
        self._call("sdm_set_issue_mode", int(mode))

    def synchronize(self):
        self._call("sdm_synchronize")

    def voxels(self):
        out = np.empty(self.v_count, VOXEL_RESULT)
        self._call("sdm_get_voxels", _ptr(out))
        return out

    # ---- batched map queries (sdm.h).  Host mode: numpy in, numpy structured arrays out, the call waits.  on_device=True:
    # the arguments are integer device pointers plus n, as update(on_device=True) takes them (device_alloc / device_put
    # buffers, or a tensor's data_ptr() where the tensor lives on the runtime the library uses - INTEGRATION.md 3); the
    # kernel is enqueued on the map's stream and the call returns at once.  The caller must have finished writing the
    # inputs on its own stream first, and reads the outputs after synchronize() (or in stream order on stream()).
    def query_points(self, xyz, with_index=False, on_device=False, n=None, out=None, voxel_out=None):
        """xyz: (n, 3) global positions -> VOXEL_RESULT per point (and the storage indices if with_index).
        on_device: xyz, out (n VOXEL_RESULT) and voxel_out (n uint32, or None) are device pointers."""
        r = self._query("sdm_query_points", xyz, np.float32, (-1, 3), (VOXEL_RESULT, np.uint32 if with_index else None), 0, on_device, n,
                        (out, voxel_out))
        return r if with_index or on_device else r[0]

    def query_segments(self, a, b=None, unknown_blocks=False, on_device=False, n=None, out=None):
        """a, b: (n, 3) end points -> SEGMENT_HIT per segment.  on_device: a is a device pointer to n rows of
        (ax ay az bx by bz) floats, b is None, out a device pointer to n SEGMENT_HIT."""
        fl = QUERY_UNKNOWN_BLOCKS if unknown_blocks else 0
        return self._query("sdm_query_segments", _rows6(a, b, on_device), np.float32, (-1, 6), SEGMENT_HIT, fl, on_device, n, out)

    def query_boxes(self, lo, hi=None, on_device=False, n=None, out=None):
        """lo, hi: (n, 3) box corners (min, max) -> BOX_RESULT per box.  on_device: lo is a device pointer to n rows of
        (min xyz, max xyz) floats, hi is None, out a device pointer to n BOX_RESULT."""
        return self._query("sdm_query_boxes", _rows6(lo, hi, on_device), np.float32, (-1, 6), BOX_RESULT, 0, on_device, n, out)

    # ---- the distance field (sdm.h).  esdf_update enqueues a build on the map's stream from the last frame's results;
    # esdf() and query_distance() answer for that frame until the next build.
    def esdf_update(self, unknown_is_obstacle=False, static_only=False):
        fl = (ESDF_UNKNOWN_IS_OBSTACLE if unknown_is_obstacle else 0) | (ESDF_STATIC_ONLY if static_only else 0)
        self._call("sdm_esdf_update", fl)

    def esdf(self):
        """-> (d2, site, origin): uint32 arrays shaped [NZ, NY, NX] in map-index order, origin the global position of the
        min corner of cell (0, 0, 0) of the field's snapshot (float32[3])"""
        c = self.cfg
        shape = (1 << c.z_n, 1 << c.y_n, 1 << c.x_n)
        d2, site, origin = np.empty(shape, np.uint32), np.empty(shape, np.uint32), np.empty(3, np.float32)
        self._call("sdm_get_esdf", _ptr(d2), _ptr(site), _ptr(origin))
        return d2, site, origin

    def query_distance(self, xyz, on_device=False, n=None, out=None):
        """xyz: (n, 3) global positions -> DISTANCE_RESULT per point.  on_device: xyz and out (n DISTANCE_RESULT) are
        device pointers, as for query_points."""
        return self._query("sdm_query_distance", xyz, np.float32, (-1, 3), DISTANCE_RESULT, 0, on_device, n, out)

    # ---- the instance table (sdm.h).  instances_update enqueues a build on the map's stream from the last frame's
    # results; instances() and label_cells() answer for that frame until the next build.
    def instances_update(self, movable_only=False, observed_only=False):
        fl = (INSTANCES_MOVABLE_ONLY if movable_only else 0) | (INSTANCES_OBSERVED_ONLY if observed_only else 0)
        self._call("sdm_instances_update", fl)

    def instances(self, cap=64):
        """-> (table, origin): INSTANCE entries in ascending track id, origin the global position of the min corner of
        cell (0, 0, 0) of the table's snapshot (float32[3]).  cap: the first guess of the table's length."""
        origin, n = np.empty(3, np.float32), C.c_int32(0)
        while True:
            out = np.empty(cap, INSTANCE)
            self._call("sdm_get_instances", _ptr(out), cap, C.byref(n), _ptr(origin))
            if n.value <= cap:
                return out[:n.value].copy(), origin
            cap = n.value

    def label_cells(self):
        """counted cells per label id (256 uint32) under the flags of the last instances_update"""
        out = np.empty(256, np.uint32)
        self._call("sdm_get_label_cells", _ptr(out))
        return out

    # ---- the frontiers (sdm.h).  frontiers_update enqueues a build on the map's stream from the last frame's results;
    # frontiers() and frontier_cells() answer for that frame until the next build.
    def frontiers_update(self, face_connected=False, min_cells=1, max_cells=0):
        fl = FRONTIERS_FACE_CONNECTED if face_connected else 0
        self._call("sdm_frontiers_update", fl, int(min_cells), int(max_cells))

    def frontiers(self, cap=64):
        """-> (table, origin): FRONTIER_CLUSTER entries in ascending first_cell, origin the global position of the min
        corner of cell (0, 0, 0) of the snapshot (float32[3]).  cap: the first guess of the table's length."""
        origin, n = np.empty(3, np.float32), C.c_int32(0)
        while True:
            out = np.empty(cap, FRONTIER_CLUSTER)
            self._call("sdm_get_frontier_clusters", _ptr(out), cap, C.byref(n), _ptr(origin))
            if n.value <= cap:
                return out[:n.value].copy(), origin
            cap = n.value

    def frontier_cells(self):
        """-> (cell, cluster, unknown_faces): the frontier cells in ascending map-index cell word (uint32), per cell the
        index of its cluster in the table (FRONTIER_NO_CLUSTER: below min_cells) and its number of unknown faces (uint8)"""
        return tuple(self._window("sdm_get_frontier_cells", [(np.uint32, ()), (np.uint32, ()), (np.uint8, ())], first=None)[0])

    # ---- view scoring (sdm.h).  Like the batched queries: host mode takes numpy and waits, on_device=True takes device
    # pointers, enqueues on the map's stream and returns at once.
    def query_views(self, views, dirs, with_rays=False, on_device=False, n_views=None, n_rays=None, out=None, rays_out=None,
                    ray_unknown_out=None):
        """views: VIEW records, dirs: (n_rays, 3) camera-frame ray vectors -> VIEW_GAIN per view; with_rays: also the
        SEGMENT_HIT and the unknown-cell count of every ray, shaped (n_views, n_rays).  on_device: views, dirs, out
        (n_views VIEW_GAIN), rays_out (n_views * n_rays SEGMENT_HIT, or None) and ray_unknown_out (int32, or None) are
        device pointers, n_views and n_rays their lengths."""
        if on_device:
            self._call("sdm_query_views", _ptr(int(views)), int(n_views), _ptr(int(dirs)), int(n_rays), _ptr(int(out)), _dev(rays_out),
                       _dev(ray_unknown_out), QUERY_ON_DEVICE)
            return None
        v = np.ascontiguousarray(views, dtype=VIEW).reshape(-1)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        gain = np.empty(len(v), VIEW_GAIN)
        rays = np.empty((len(v), len(d)), SEGMENT_HIT) if with_rays else None
        unk = np.empty((len(v), len(d)), np.int32) if with_rays else None
        self._call("sdm_query_views", _ptr(v), len(v), _ptr(d), len(d), _ptr(gain), _ptr(rays), _ptr(unk), 0)
        return (gain, rays, unk) if with_rays else gain

    def set_view_batch(self, max_views_in_flight):
        """Test hook: query_views keeps at most this many views in flight (<= 0: the library's choice) (sdm_debug_view_batch)."""
        self._call("sdm_debug_view_batch", int(max_views_in_flight))

    # ---- the travel-cost field (sdm.h).  reach_update builds the field from the last frame's results (or, with min_d2 > 0,
    # from the distance field's snapshot) and WAITS until it is complete; reach(), query_reach() and reach_paths() answer
    # for that build until the next one.
    def reach_update(self, starts=None, start_cells=None, min_d2=0, max_cost=0, face_connected=False, through_unknown=False):
        """starts: (n, 3) global positions, or start_cells: n map-index cell words (exactly one of the two)"""
        fl = (REACH_FACE_CONNECTED if face_connected else 0) | (REACH_THROUGH_UNKNOWN if through_unknown else 0)
        p, w, n = _goals(starts, start_cells, *_WORDS)
        self._call("sdm_reach_update", _ptr(p), _ptr(w), n, int(min_d2), int(max_cost), fl)

    def reach(self):
        """-> (cost, info, origin): cost uint32 shaped [NZ, NY, NX] in map-index order, info a REACH_INFO record, origin the
        global position of the min corner of cell (0, 0, 0) of the snapshot (float32[3])"""
        c = self.cfg
        cost = np.empty((1 << c.z_n, 1 << c.y_n, 1 << c.x_n), np.uint32)
        info, origin = np.zeros(1, REACH_INFO), np.empty(3, np.float32)
        self._call("sdm_get_reach", _ptr(cost), _ptr(info), _ptr(origin))
        return cost, info[0], origin

    def query_reach(self, xyz=None, cells=None, on_device=False, n=None, out=None):
        """goals as (n, 3) global positions or as n cell words -> REACH_RESULT per goal.  on_device: the one given of xyz /
        cells and out (n REACH_RESULT) are device pointers."""
        return self._goal_query("sdm_query_reach", xyz, cells, _WORDS, REACH_RESULT, on_device, n, out)

    def reach_paths(self, xyz=None, cells=None, max_len=0, on_device=False, n=None, cells_out=None, len_out=None, fill=REACH_NO_COST):
        """-> (cells_out, len_out): row g holds the first min(len, max_len) cell words of goal g's path, goal first, and
        `fill` behind them; len_out the true lengths (int32, 0: no path).  on_device: the pointers are device pointers
        (cells_out n * max_len uint32, len_out n int32) and nothing is returned."""
        return self._goal_paths("sdm_reach_paths", xyz, cells, _WORDS, max_len, fill, on_device, n, cells_out, len_out)

    def reach_tiles(self):
        """Diagnostic: the tiles the last reach_update relaxed, summed over its rounds (sdm_debug_reach_tiles)."""
        return self._out("sdm_debug_reach_tiles", C.c_int64)

    # ---- the forecast (sdm.h).  forecast_update enqueues a build on the map's stream from the last frame's results and the
    # motions given; forecast(), forecast_cells() and the two queries answer for that frame until the next build.
    def forecast_update(self, motions, horizons, swept=False):
        """motions: MOTION records (or None: none), horizons: ascending times in seconds"""
        mo = np.zeros(0, MOTION) if motions is None else np.ascontiguousarray(motions, dtype=MOTION).reshape(-1)
        t = np.ascontiguousarray(horizons, dtype=np.float32).reshape(-1)
        self._call("sdm_forecast_update", _ptr(mo), len(mo), _ptr(t), len(t), FORECAST_SWEPT if swept else 0)

    def forecast(self):
        """-> (mask, first, info, origin): uint32 arrays shaped [NZ, NY, NX] in map-index order, a FORECAST_INFO record,
        origin the global position of the min corner of cell (0, 0, 0) of the snapshot (float32[3])"""
        c = self.cfg
        shape = (1 << c.z_n, 1 << c.y_n, 1 << c.x_n)
        mask, first = np.empty(shape, np.uint32), np.empty(shape, np.uint32)
        info, origin = np.zeros(1, FORECAST_INFO), np.empty(3, np.float32)
        self._call("sdm_get_forecast", _ptr(mask), _ptr(first), _ptr(info), _ptr(origin))
        return mask, first, info[0], origin

    def forecast_cells(self, cap=None):
        """-> (cell, mask, first): the cells with any horizon bit in ascending map-index cell word and their field words;
        cap: at most so many of them (-> also the true count, as a fourth value)"""
        cols, _, n = self._window("sdm_get_forecast_cells", [(np.uint32, ())] * 3, first=None, cap=cap)
        return tuple(cols) if cap is None else (*cols, n)

    def query_forecast(self, xyzt, on_device=False, n=None, out=None):
        """xyzt: (n, 4) global positions and times -> FORECAST_RESULT per point.  on_device: xyzt and out (n FORECAST_RESULT)
        are device pointers."""
        return self._query("sdm_query_forecast", xyzt, np.float32, (-1, 4), FORECAST_RESULT, 0, on_device, n, out)

    def query_forecast_segments(self, seg, unknown_blocks=False, vacated_blocks=False, on_device=False, n=None, out=None):
        """seg: (n, 8) rows ax ay az ta bx by bz tb -> FORECAST_HIT per segment.  on_device: seg and out (n FORECAST_HIT)
        are device pointers."""
        fl = (QUERY_UNKNOWN_BLOCKS if unknown_blocks else 0) | (FORECAST_VACATED_BLOCKS if vacated_blocks else 0)
        return self._query("sdm_query_forecast_segments", seg, np.float32, (-1, 8), FORECAST_HIT, fl, on_device, n, out)

    # ---- the ground layer (sdm.h).  ground_update enqueues a build on the map's stream from the last frame's results;
    # ground(), query_ground() and query_footprints() answer for that frame until the next build.
    def ground_update(self, up=(1, -1), h_lo=0, h_hi=0, clearance=0, max_step=0, support_labels=None, unknown_passable=False,
                      ignore_movable=False, none_is_lethal=False):
        """up: (axis, sign); h_lo, h_hi, clearance, max_step in cells (ground_band gives a band from metres);
        support_labels: the label ids that may carry the robot (None: none)"""
        o = np.zeros(1, GROUND_OPTIONS)
        o["up_axis"], o["up_sign"], o["h_lo"], o["h_hi"], o["clearance"], o["max_step"] = up[0], up[1], h_lo, h_hi, clearance, max_step
        o["support_labels"] = label_mask(support_labels)
        o["flags"] = ((GROUND_UNKNOWN_PASSABLE if unknown_passable else 0) | (GROUND_IGNORE_MOVABLE if ignore_movable else 0) |
                      (GROUND_NONE_IS_LETHAL if none_is_lethal else 0))
        self._call("sdm_ground_update", _ptr(o))

    def ground(self):
        """-> (cells, d2, info, origin): GROUND_CELL and uint32 arrays shaped [N_v, N_u] (column word = i_u + j_v * N_u), a
        GROUND_INFO record, origin the global position of the min corner of cell (0, 0, 0) of the snapshot (float32[3])"""
        info, origin = np.zeros(1, GROUND_INFO), np.empty(3, np.float32)
        self._call("sdm_get_ground", None, None, _ptr(info), _ptr(origin))
        shape = (int(info["n_v"][0]), int(info["n_u"][0]))
        cells, d2 = np.empty(shape, GROUND_CELL), np.empty(shape, np.uint32)
        self._call("sdm_get_ground", _ptr(cells), _ptr(d2), None, None)
        return cells, d2, info[0], origin

    def query_ground(self, xyz, on_device=False, n=None, out=None):
        """xyz: (n, 3) global positions -> GROUND_RESULT per point.  on_device: xyz and out (n GROUND_RESULT) are device
        pointers, as for query_points."""
        return self._query("sdm_query_ground", xyz, np.float32, (-1, 3), GROUND_RESULT, 0, on_device, n, out)

    def query_footprints(self, footprints, on_device=False, n=None, out=None):
        """footprints: FOOTPRINT records -> FOOTPRINT_RESULT per footprint.  on_device: footprints and out (n
        FOOTPRINT_RESULT) are device pointers."""
        return self._query("sdm_query_footprints", footprints, FOOTPRINT, (-1,), FOOTPRINT_RESULT, 0, on_device, n, out)

    # ---- the surface mesh (sdm.h).  mesh_update enqueues a build on the map's stream from the last frame's results;
    # mesh() and mesh_device() answer for that frame until the next build.
    def mesh_update(self, labels=None, track=-1, static_only=False, movable_only=False, observed_only=False, skip_unknown_faces=False,
                    skip_border_faces=False, max_faces=0, max_vertices=0):
        """labels: the label ids whose cells may be solid (None: all 256); track: -1 any, else that track's cells only;
        max_faces / max_vertices: the lists' capacities (0: the defaults, V / 8 faces and 3 / 2 as many vertices)"""
        o = np.zeros(1, MESH_OPTIONS)
        o["labels"] = np.full(8, 0xFFFFFFFF, np.uint32) if labels is None else label_mask(labels)
        o["track"], o["max_faces"], o["max_vertices"] = track, max_faces, max_vertices
        o["flags"] = ((MESH_STATIC_ONLY if static_only else 0) | (MESH_MOVABLE_ONLY if movable_only else 0) |
                      (MESH_OBSERVED_ONLY if observed_only else 0) | (MESH_SKIP_UNKNOWN_FACES if skip_unknown_faces else 0) |
                      (MESH_SKIP_BORDER_FACES if skip_border_faces else 0))
        self._call("sdm_mesh_update", _ptr(o))

    def mesh_info(self):
        """-> (info, origin): a MESH_INFO record (true counts, also of a build over capacity) and the global position of the
        min corner of cell (0, 0, 0) of the snapshot (float32[3])"""
        info, origin = np.zeros(1, MESH_INFO), np.empty(3, np.float32)
        self._call("sdm_get_mesh_info", _ptr(info), _ptr(origin))
        return info[0], origin

    def mesh(self):
        """-> dict(faces MESH_FACE[n], quads uint32[n, 4], corners MESH_VERTEX[m], xyz float32[m, 3], info, origin).  A build
        over capacity raises SdmError (SDM_ERR_CAPACITY): mesh_info() has the counts to ask for."""
        info, origin = self.mesh_info()
        n, k = int(info["n_faces"]), int(info["n_vertices"])
        faces, quads = np.empty(n, MESH_FACE), np.empty((n, 4), np.uint32)
        corners, xyz = np.empty(k, MESH_VERTEX), np.empty((k, 3), np.float32)
        got = C.c_int64(0)
        self._call("sdm_get_mesh_faces", _ptr(faces), _ptr(quads), n, C.byref(got))
        self._call("sdm_get_mesh_vertices", _ptr(corners), _ptr(xyz), k, C.byref(got))
        return dict(faces=faces, quads=quads, corners=corners, xyz=xyz, info=info, origin=origin)

    def mesh_device(self):
        """-> (faces, quads, corners): device addresses of the last build's lists (MESH_FACE, 4 uint32 per face, MESH_VERTEX),
        valid until the next mesh_update, to be read in stream order on the map's stream"""
        p = [C.c_void_p() for _ in range(3)]
        self._call("sdm_mesh_device", *(C.byref(x) for x in p))
        return tuple(x.value for x in p)

    # ---- the world archive (sdm.h).  world_update enqueues the merge of the last frame's results into the archive on the
    # map's stream; the getters and queries answer for everything archived so far, wherever the block is now.
    def world_update(self, static_only=False, observed_only=False, max_bricks=0):
        o = np.zeros(1, WORLD_OPTIONS)
        o["flags"] = (WORLD_STATIC_ONLY if static_only else 0) | (WORLD_OBSERVED_ONLY if observed_only else 0)
        o["max_bricks"] = int(max_bricks)
        self._call("sdm_world_update", _ptr(o))

    def world_clear(self):
        self._call("sdm_world_clear")

    def world_info(self):
        """-> a WORLD_INFO record; zeros (bmax -1) before any update and after world_clear"""
        info = np.zeros(1, WORLD_INFO)
        self._call("sdm_get_world_info", _ptr(info))
        return info[0]

    def world_bricks(self, with_cells=True, first=0, cap=None):
        """-> (bricks WORLD_BRICK[n], cells uint32[n, 512] or None) in brick order: ascending in (bz, by, bx)"""
        got = C.c_int64()
        if cap is None:
            self._call("sdm_get_world_bricks", None, None, 0, 0, C.byref(got))
            cap = max(got.value - int(first), 0)
        bricks = np.empty(cap, WORLD_BRICK)
        cells = np.empty((cap, 512), np.uint32) if with_cells else None
        self._call("sdm_get_world_bricks", _ptr(bricks), _ptr(cells), int(first), cap, C.byref(got))
        n = max(min(got.value - int(first), cap), 0)
        return bricks[:n], (cells[:n] if with_cells else None)

    def world_occupied(self, cap=None):
        """-> (points POINT[min(n, cap)], n): every archived cell with occ >= 1, ascending in (brick order, cell word)"""
        got = C.c_int64()
        if cap is None:
            self._call("sdm_get_world_occupied", None, 0, C.byref(got), 0)
            cap = got.value
        out = np.empty(cap, POINT)
        self._call("sdm_get_world_occupied", _ptr(out), cap, C.byref(got), 0)
        return out[:min(got.value, cap)], got.value

    def query_world(self, xyz, on_device=False, n=None, out=None):
        """xyz: (n, 3) global positions -> WORLD_CELL per point.  on_device: xyz and out (n WORLD_CELL) are device pointers,
        as for query_points."""
        return self._query("sdm_query_world_points", xyz, np.float32, (-1, 3), WORLD_CELL, 0, on_device, n, out)

    def world_region(self, cell_min, size, on_device=False, out=None):
        """-> uint32 [size z, size y, size x]: the words of the box of world cells from cell_min (x, y, z) on; on_device: out is
        a device pointer to size x * y * z words, filled in stream order"""
        lo, sz = np.ascontiguousarray(cell_min, np.int32).reshape(3), np.ascontiguousarray(size, np.int32).reshape(3)
        if on_device:
            self._call("sdm_get_world_region", _ptr(lo), _ptr(sz), _ptr(int(out)), QUERY_ON_DEVICE)
            return None
        words = np.empty((max(int(sz[2]), 0), max(int(sz[1]), 0), max(int(sz[0]), 0)), np.uint32)
        self._call("sdm_get_world_region", _ptr(lo), _ptr(sz), _ptr(words), 0)
        return words

    def world_import(self, bricks, cells, offset=(0, 0, 0), fill=False, static_only=False, observed_only=False, max_bricks=0, on_device=False,
                     n=None):
        """Merges foreign bricks - WORLD_BRICK[n] and uint32 [n, 512], as world_bricks returns them - into the archive, the
        source's world cells moved by `offset` cells; fill: only where the archive reads unknown.  on_device: bricks and
        cells are device pointers to n bricks, read in stream order on the map's stream; the call does not wait."""
        o = np.zeros(1, WORLD_IMPORT_OPTIONS)
        o["flags"] = ((WORLD_STATIC_ONLY if static_only else 0) | (WORLD_OBSERVED_ONLY if observed_only else 0) | (WORLD_IMPORT_FILL if fill else 0) |
                      (WORLD_IMPORT_ON_DEVICE if on_device else 0))
        o["cell_offset"][0] = np.asarray(offset, np.int64).reshape(3)
        o["max_bricks"] = int(max_bricks)
        if on_device:
            self._call("sdm_world_import", _ptr(o), _ptr(int(bricks)), _ptr(int(cells)), int(n))
            return
        b = np.ascontiguousarray(bricks, WORLD_BRICK).reshape(-1)
        c = np.ascontiguousarray(cells, np.uint32).reshape(-1, 512)
        if len(b) != len(c):
            raise ValueError("world_import: %d headers and %d bricks of cells" % (len(b), len(c)))
        self._call("sdm_world_import", _ptr(o), _ptr(b), _ptr(c), len(b) if n is None else int(n))

    def world_match(self, bricks, cells, offset=(0, 0, 0), radius=(2, 2, 1), weights=WORLD_MATCH_WEIGHTS, static_only=False,
                    observed_only=False, on_device=False, n=None, scores=True, result=None):
        """Scores foreign bricks - as for world_import - against the archive under every whole-cell offset `offset` + d,
        |d| <= radius per axis (0 .. 8) -> (result WORLD_MATCH_RESULT, scores WORLD_MATCH_SCORE[n_candidates] in candidate
        order, x fastest).  Reads the archive, writes nothing; result["best_offset"] is what world_import takes as offset.
        weights: (w_oo, w_same, w_of, w_fo, w_ff); the default (4, 1, -2, -2, 0) is this binding's - agreement of occupied
        cells counts, a conflict costs half as much, free on free counts nothing - and is not tuned on anything.
        scores False: only the result.  on_device: bricks and cells are device pointers to n bricks, scores (or None) and
        result device pointers the call fills in stream order on the map's stream; it does not wait and returns None."""
        o = np.zeros(1, WORLD_MATCH_OPTIONS)
        o["flags"] = ((WORLD_STATIC_ONLY if static_only else 0) | (WORLD_OBSERVED_ONLY if observed_only else 0) |
                      (WORLD_MATCH_ON_DEVICE if on_device else 0))
        o["cell_offset"][0] = np.asarray(offset, np.int64).reshape(3)
        o["radius"][0] = np.asarray(radius, np.int64).reshape(3)
        for name, w in zip(("w_oo", "w_same", "w_of", "w_fo", "w_ff"), weights):
            o[name] = int(w)
        if on_device:
            self._call("sdm_world_match", _ptr(o), _ptr(int(bricks)), _ptr(int(cells)), int(n),
                       None if scores is None or isinstance(scores, bool) else _ptr(int(scores)), _ptr(int(result)))
            return None
        b = np.ascontiguousarray(bricks, WORLD_BRICK).reshape(-1)
        c = np.ascontiguousarray(cells, np.uint32).reshape(-1, 512)
        if len(b) != len(c):
            raise ValueError("world_match: %d headers and %d bricks of cells" % (len(b), len(c)))
        r = [int(v) for v in o["radius"][0]]
        res = np.zeros(1, WORLD_MATCH_RESULT)
        sc = np.zeros(max((2 * r[0] + 1) * (2 * r[1] + 1) * (2 * r[2] + 1), 0), WORLD_MATCH_SCORE) if scores else None
        self._call("sdm_world_match", _ptr(o), _ptr(b), _ptr(c), len(b) if n is None else int(n), _ptr(sc), _ptr(res))
        return res[0], sc

    def world_align(self, bricks, cells, offset=(0, 0, 0), search=(8, 8, 2), **kw):
        """world_match over a search of `search` cells per axis round `offset`, wider than one match may be: tiled on the host
        into windows of at most 17 candidates per axis, combined under the same rule relative to `offset` - the highest
        score, then the smallest squared distance from `offset`, then the candidate order of the whole search ->
        (best_offset int32[3], best_score, runner_up); runner_up: the best score among the candidates of the whole search
        at Chebyshev distance >= 2 from the best, None if there is none.  Host pointers only; kw: world_match's."""
        if kw.get("on_device"):
            raise ValueError("world_align works on host arrays")
        c0, R = np.asarray(offset, np.int64).reshape(3), np.asarray(search, np.int64).reshape(3)
        if (R < 0).any():
            raise ValueError("world_align: a negative search")
        tiles = []
        for a in range(3):                                # per axis: windows (centre d, radius) that cover -R .. R once
            axis, lo = [], -int(R[a])
            while lo <= R[a]:
                hi = min(lo + 2 * WORLD_MATCH_MAX_RADIUS, int(R[a]))
                r = (hi - lo + 1) // 2                     # (an even count is covered by one candidate more, inside the search's hull or not)
                axis.append((lo + r, r, lo, hi))
                lo = hi + 1
            tiles.append(axis)
        n = [2 * int(v) + 1 for v in R]
        score = np.zeros((n[2], n[1], n[0]), np.int64)
        w = [int(v) for v in kw.get("weights", WORLD_MATCH_WEIGHTS)]
        for tz in tiles[2]:
            for ty in tiles[1]:
                for tx in tiles[0]:
                    t = (tx, ty, tz)
                    _, sc = self.world_match(bricks, cells, offset=c0 + [v[0] for v in t], radius=[v[1] for v in t], **kw)
                    d = sc["offset"].astype(np.int64) - c0
                    keep = np.all([(d[:, a] >= t[a][2]) & (d[:, a] <= t[a][3]) for a in range(3)], axis=0)
                    s = (w[0] * sc["n_oo"].astype(np.int64) + w[1] * sc["n_same"].astype(np.int64) + w[2] * sc["n_of"].astype(np.int64) +
                         w[3] * sc["n_fo"].astype(np.int64) + w[4] * sc["n_ff"].astype(np.int64))
                    d = d[keep] + R
                    score[d[:, 2], d[:, 1], d[:, 0]] = s[keep]
        dz, dy, dx = np.meshgrid(*(np.arange(-int(v), int(v) + 1) for v in R[::-1]), indexing="ij")
        d2 = dx * dx + dy * dy + dz * dz
        flat = np.lexsort((np.arange(score.size), d2.ravel(), -score.ravel()))[0]      # the smallest k last among the keys
        bz, by, bx = np.unravel_index(flat, score.shape)
        best = np.array([bx, by, bz], np.int64) - R
        far = np.maximum(np.maximum(np.abs(dx - best[0]), np.abs(dy - best[1])), np.abs(dz - best[2])) >= 2
        runner_up = int(score[far].max()) if far.any() else None
        return (c0 + best).astype(np.int32), int(score[bz, by, bx]), runner_up

    def world_retain(self, bmin=None, bmax=None, min_last_stamp=0):
        """Keeps the bricks inside the inclusive brick box bmin .. bmax (None: no bound) whose last_stamp >= min_last_stamp,
        removes the others -> how many were removed"""
        o = np.zeros(1, WORLD_RETAIN_OPTIONS)
        o["bmin"][0] = np.asarray((-32768,) * 3 if bmin is None else bmin, np.int64).reshape(3)
        o["bmax"][0] = np.asarray((32767,) * 3 if bmax is None else bmax, np.int64).reshape(3)
        o["min_last_stamp"] = int(min_last_stamp)
        return self._out("sdm_world_retain", C.c_int64, _ptr(o))

    # ---- world reach (sdm.h).  world_reach_update builds the travel-cost field over the archive's bricks and WAITS until it
    # is complete; world_reach(), query_world_reach() and world_reach_paths() answer for that build - a snapshot that later
    # updates, imports, retains and clears of the archive do not touch - until the next one.
    def world_reach_update(self, starts=None, start_cells=None, inflate=0, max_cost=0, face_connected=False, through_unknown=False,
                           ignore_movable=False, box=None):
        """starts: (n, 3) global positions, or start_cells: (n, 3) world cells (exactly one of the two); box: (bmin, bmax),
        an inclusive box of brick coordinates the field is cut to"""
        o = np.zeros(1, WORLD_REACH_OPTIONS)
        o["flags"] = ((WORLD_REACH_FACE_CONNECTED if face_connected else 0) | (WORLD_REACH_THROUGH_UNKNOWN if through_unknown else 0) |
                      (WORLD_REACH_IGNORE_MOVABLE if ignore_movable else 0) | (WORLD_REACH_BOX if box is not None else 0))
        o["inflate"], o["max_cost"] = int(inflate), int(max_cost)
        if box is not None:
            o["bmin"], o["bmax"] = box[0], box[1]
        p, w, n = _goals(starts, start_cells, *_WORLD_CELLS)
        self._call("sdm_world_reach_update", _ptr(o), _ptr(p), _ptr(w), n)

    def world_reach(self, with_cost=True, first=0, cap=None):
        """-> (coords int16 [n, 3] (bx, by, bz), cost uint32 [n, 512] or None, info a WORLD_REACH_INFO record): the bricks of
        the field in brick order, rows first .. first + cap - 1"""
        cols = [(np.int16, (3,)), (np.uint32, (512,)) if with_cost else None]
        (coords, cost), info, _ = self._window("sdm_get_world_reach", cols, first, cap, WORLD_REACH_INFO)
        return coords, cost, info

    def query_world_reach(self, xyz=None, cells=None, on_device=False, n=None, out=None):
        """goals as (n, 3) global positions or as (n, 3) world cells -> WORLD_REACH_RESULT per goal.  on_device: the one
        given of xyz / cells and out (n WORLD_REACH_RESULT) are device pointers."""
        return self._goal_query("sdm_query_world_reach", xyz, cells, _WORLD_CELLS, WORLD_REACH_RESULT, on_device, n, out)

    def world_reach_paths(self, xyz=None, cells=None, max_len=0, on_device=False, n=None, cells_out=None, len_out=None,
                          fill=WORLD_REACH_NO_CELL):
        """-> (cells_out int32 [n, max_len, 3], len_out): row g holds the first min(len, max_len) world cells of goal g's
        path, goal first, and `fill` behind them; len_out the true lengths (int32, 0: no path).  on_device: the pointers are
        device pointers (cells_out n * max_len * 3 int32, len_out n int32) and nothing is returned."""
        return self._goal_paths("sdm_world_reach_paths", xyz, cells, _WORLD_CELLS, max_len, fill, on_device, n, cells_out, len_out)

    def world_reach_bricks_relaxed(self):
        """Diagnostic: the bricks the last world_reach_update relaxed, summed over its rounds (sdm_debug_world_reach_bricks)."""
        return self._out("sdm_debug_world_reach_bricks", C.c_int64)

    # ---- world frontiers (sdm.h).  world_frontiers_update builds the frontier cells of the archive's bricks and their
    # clusters and WAITS until they are complete; world_frontiers() and world_frontier_cells() answer for that build - a
    # snapshot that later updates, imports, retains and clears of the archive do not touch - until the next one.
    def world_frontiers_update(self, face_connected=False, box=None, inside_bricks=False, min_cells=1, max_cells=0):
        """box: (bmin, bmax), an inclusive box of brick coordinates the field is cut to; inside_bricks: a neighbour in no
        archived brick does not read unknown"""
        o = np.zeros(1, WORLD_FRONTIERS_OPTIONS)
        o["flags"] = ((WORLD_FRONTIERS_FACE_CONNECTED if face_connected else 0) | (WORLD_FRONTIERS_BOX if box is not None else 0) |
                      (WORLD_FRONTIERS_INSIDE_BRICKS if inside_bricks else 0))
        o["min_cells"], o["max_cells"] = int(min_cells), int(max_cells)
        if box is not None:
            o["bmin"], o["bmax"] = box[0], box[1]
        self._call("sdm_world_frontiers_update", _ptr(o))

    def world_frontiers(self):
        """-> (clusters, info): WORLD_FRONTIER_CLUSTER entries in ascending first_index, a WORLD_FRONTIERS_INFO record"""
        got = C.c_int32(0)
        info = np.zeros(1, WORLD_FRONTIERS_INFO)
        self._call("sdm_get_world_frontier_clusters", None, 0, C.byref(got), _ptr(info))
        out = np.empty(got.value, WORLD_FRONTIER_CLUSTER)
        self._call("sdm_get_world_frontier_clusters", _ptr(out), got.value, C.byref(got), None)
        return out, info[0]

    def world_frontier_cells(self, first=0, cap=None):
        """-> (cells int32 [n, 3] world cells, cluster uint32, unknown_faces uint8): rows first .. first + cap - 1 of the cell
        list, ascending in (brick order, cell word); cluster indexes the table (WORLD_FRONTIER_NO_CLUSTER: below min_cells)"""
        return tuple(self._window("sdm_get_world_frontier_cells", [(np.int32, (3,)), (np.uint32, ()), (np.uint8, ())], first, cap)[0])

    # ---- world objects (sdm.h).  world_objects_update builds the connected same-key components of the archive's occupied
    # cells and WAITS until they are complete; world_objects(), world_object_cells(), world_object_labels() and
    # query_world_objects() answer for that build - a snapshot that later updates, imports, retains and clears of the
    # archive do not touch - until the next one.
    def world_objects_update(self, face_connected=False, by_track=False, static_only=False, movable_only=False, observed_only=False,
                             labels=ALL_LABELS, box=None, min_cells=1, max_cells=0):
        """labels: the label ids whose cells count (default: all; none: a field without objects); by_track: the key is label
        and track; box: (bmin, bmax), an inclusive box of brick coordinates the field is cut to"""
        o = np.zeros(1, WORLD_OBJECTS_OPTIONS)
        o["flags"] = ((WORLD_OBJECTS_FACE_CONNECTED if face_connected else 0) | (WORLD_OBJECTS_BOX if box is not None else 0) |
                      (WORLD_OBJECTS_BY_TRACK if by_track else 0) | (WORLD_OBJECTS_STATIC_ONLY if static_only else 0) |
                      (WORLD_OBJECTS_MOVABLE_ONLY if movable_only else 0) | (WORLD_OBJECTS_OBSERVED_ONLY if observed_only else 0))
        o["min_cells"], o["max_cells"] = int(min_cells), int(max_cells)
        o["labels"] = label_mask(labels)
        if box is not None:
            o["bmin"], o["bmax"] = box[0], box[1]
        self._call("sdm_world_objects_update", _ptr(o))

    def world_objects(self):
        """-> (table, info): WORLD_OBJECT entries in ascending first_index, a WORLD_OBJECTS_INFO record"""
        got = C.c_int32(0)
        info = np.zeros(1, WORLD_OBJECTS_INFO)
        self._call("sdm_get_world_objects", None, 0, C.byref(got), _ptr(info))
        out = np.empty(got.value, WORLD_OBJECT)
        self._call("sdm_get_world_objects", _ptr(out), got.value, C.byref(got), None)
        return out, info[0]

    def world_object_cells(self, first=0, cap=None):
        """-> (cells int32 [n, 3] world cells, object uint32, words uint32): rows first .. first + cap - 1 of the cell list,
        ascending in (brick order, cell word); object indexes the table (WORLD_OBJECT_UNLISTED: below min_cells)"""
        return tuple(self._window("sdm_get_world_object_cells", [(np.int32, (3,)), (np.uint32, ()), (np.uint32, ())], first, cap)[0])

    def world_object_labels(self):
        """-> (cells uint64 [256], objects uint32 [256]): per label the counted cells and the objects in all"""
        cells, objects = np.zeros(256, np.uint64), np.zeros(256, np.uint32)
        self._call("sdm_get_world_object_labels", _ptr(cells), _ptr(objects))
        return cells, objects

    def world_object_members(self, i):
        """-> (cells, words) of table entry i: its rows of the cell list, selected on the host"""
        cells, obj, words = self.world_object_cells()
        mine = obj == np.uint32(i)
        return cells[mine], words[mine]

    def query_world_objects(self, xyz=None, cells=None, on_device=False, n=None, out=None):
        """(n, 3) global positions or (n, 3) world cells -> WORLD_OBJECT_RESULT per entry.  on_device: the one given of
        xyz / cells and out (n WORLD_OBJECT_RESULT) are device pointers."""
        return self._goal_query("sdm_query_world_objects", xyz, cells, _WORLD_CELLS, WORLD_OBJECT_RESULT, on_device, n, out)

    # ---- world distance field (sdm.h).  world_esdf_update builds the truncated distance field over the archive's bricks
    # (it waits once, for the field's brick count); world_esdf() and query_world_distance() answer for that build - a
    # snapshot that later updates, imports, retains and clears of the archive do not touch - until the next one.
    def world_esdf_update(self, radius, unknown_is_obstacle=False, static_only=False, box=None):
        """radius: 1 .. WORLD_ESDF_MAX_RADIUS cells, up to which the field is exact; box: (bmin, bmax), an inclusive box of
        brick coordinates the field is cut to (obstacles still come from the whole archive)"""
        o = np.zeros(1, WORLD_ESDF_OPTIONS)
        o["flags"] = ((WORLD_ESDF_UNKNOWN_IS_OBSTACLE if unknown_is_obstacle else 0) | (WORLD_ESDF_STATIC_ONLY if static_only else 0) |
                      (WORLD_ESDF_BOX if box is not None else 0))
        o["radius"] = int(radius)
        if box is not None:
            o["bmin"], o["bmax"] = box[0], box[1]
        self._call("sdm_world_esdf_update", _ptr(o))

    def world_esdf(self, first=0, cap=None):
        """-> (coords int16 [n, 3] (bx, by, bz), d2 uint16 [n, 512] (WORLD_ESDF_NONE: beyond the radius), offset int8
        [n, 512, 3] (dx, dy, dz) to the nearest obstacle, info a WORLD_ESDF_INFO record): the bricks of the field in brick
        order, rows first .. first + cap - 1"""
        cols = [(np.int16, (3,)), (np.uint16, (512,)), (np.int8, (512, 3))]
        (coords, d2, offset), info, _ = self._window("sdm_get_world_esdf", cols, first, cap, WORLD_ESDF_INFO)
        return coords, d2, offset, info

    def query_world_distance(self, xyz=None, cells=None, on_device=False, n=None, out=None):
        """(n, 3) global positions or (n, 3) world cells -> WORLD_DISTANCE_RESULT per entry.  on_device: the one given of
        xyz / cells and out (n WORLD_DISTANCE_RESULT) are device pointers."""
        return self._goal_query("sdm_query_world_distance", xyz, cells, _WORLD_CELLS, WORLD_DISTANCE_RESULT, on_device, n, out)

    # ---- world ground layer (sdm.h).  world_ground_update builds the height map, the costmap and the truncated distance
    # to the nearest lethal column over the archive's bricks (it waits once, for the tile count); world_ground(),
    # query_world_ground() and query_world_footprints() answer for that build - a snapshot - until the next one.
    def world_ground_update(self, up=(2, 1), h_lo=0, h_hi=0, clearance=0, max_step=0, radius=8, support_labels=None, unknown_passable=False,
                            ignore_movable=False, none_is_lethal=False, absent_is_lethal=False, box=None):
        """up: (axis, sign); h_lo, h_hi: world heights in cells (world_ground_band gives a band from metres); clearance,
        max_step in cells; radius: 1 .. WORLD_GROUND_MAX_RADIUS columns; support_labels: label ids (label_mask); box:
        (tmin, tmax), an inclusive box of tile coordinates (bu, bv) the layer is cut to"""
        o = np.zeros(1, WORLD_GROUND_OPTIONS)
        o["up_axis"], o["up_sign"] = int(up[0]), int(up[1])
        o["h_lo"], o["h_hi"], o["clearance"], o["max_step"], o["radius"] = int(h_lo), int(h_hi), int(clearance), int(max_step), int(radius)
        o["support_labels"] = label_mask(support_labels)
        o["flags"] = ((WORLD_GROUND_UNKNOWN_PASSABLE if unknown_passable else 0) | (WORLD_GROUND_IGNORE_MOVABLE if ignore_movable else 0) |
                      (WORLD_GROUND_NONE_IS_LETHAL if none_is_lethal else 0) | (WORLD_GROUND_ABSENT_IS_LETHAL if absent_is_lethal else 0) |
                      (WORLD_GROUND_BOX if box is not None else 0))
        if box is not None:
            o["tmin"], o["tmax"] = box[0], box[1]
        self._call("sdm_world_ground_update", _ptr(o))

    def world_ground(self, first=0, cap=None):
        """-> (coords int16 [n, 2] (bu, bv), cells GROUND_CELL [n, 64], d2 uint16 [n, 64] (WORLD_GROUND_NONE: beyond the
        radius), info a WORLD_GROUND_INFO record): the tiles in (bv, bu) order, rows first .. first + cap - 1; a column's
        word is cu | cv << 3; level and top are relative to h_lo"""
        cols = [(np.int16, (2,)), (GROUND_CELL, (64,)), (np.uint16, (64,))]
        (coords, cells, d2), info, _ = self._window("sdm_get_world_ground", cols, first, cap, WORLD_GROUND_INFO)
        return coords, cells, d2, info

    def query_world_ground(self, xyz=None, cells=None, on_device=False, n=None, out=None):
        """(n, 3) global positions or (n, 3) world cells -> WORLD_GROUND_RESULT per entry.  on_device: the one given of
        xyz / cells and out (n WORLD_GROUND_RESULT) are device pointers."""
        return self._goal_query("sdm_query_world_ground", xyz, cells, _WORLD_CELLS, WORLD_GROUND_RESULT, on_device, n, out)

    def query_world_footprints(self, footprints, on_device=False, n=None, out=None):
        """footprints: FOOTPRINT records (centre in world metres along u and v) -> WORLD_FOOTPRINT_RESULT per footprint.
        on_device: footprints and out (n WORLD_FOOTPRINT_RESULT) are device pointers."""
        return self._query("sdm_query_world_footprints", footprints, FOOTPRINT, (-1,), WORLD_FOOTPRINT_RESULT, 0, on_device, n, out)

    # ---- world ground reach (sdm.h).  world_ground_reach_update builds the 2-D travel-cost field over the last
    # world_ground_update's costmap and WAITS until it is complete; world_ground_reach(), query_world_ground_reach() and
    # world_ground_reach_paths() answer for that build - a snapshot that later ground builds and changes of the archive do
    # not touch - until the next one.
    def world_ground_reach_update(self, starts=None, start_cells=None, min_d2=0, soft_d2=0, penalty=0, max_climb=0, max_cost=0,
                                  face_connected=False, box=None):
        """starts: (n, 3) global positions, or start_cells: (n, 3) world cells (exactly one of the two; only the column
        counts); min_d2, soft_d2: thresholds on the ground layer's d2, 0 .. R^2 + 1; penalty: what a column below soft_d2
        costs more; max_climb in cells; box: (tmin, tmax), an inclusive box of tile coordinates (bu, bv) the field is cut to"""
        o = np.zeros(1, WORLD_GROUND_REACH_OPTIONS)
        o["flags"] = (WORLD_GROUND_REACH_FACE_CONNECTED if face_connected else 0) | (WORLD_GROUND_REACH_BOX if box is not None else 0)
        o["min_d2"], o["soft_d2"], o["penalty"], o["max_climb"], o["max_cost"] = int(min_d2), int(soft_d2), int(penalty), int(max_climb), int(max_cost)
        if box is not None:
            o["tmin"], o["tmax"] = box[0], box[1]
        p, w, n = _goals(starts, start_cells, *_WORLD_CELLS)
        self._call("sdm_world_ground_reach_update", _ptr(o), _ptr(p), _ptr(w), n)

    def world_ground_reach(self, with_cost=True, first=0, cap=None):
        """-> (coords int16 [n, 2] (bu, bv), cost uint32 [n, 64] or None, info a WORLD_GROUND_REACH_INFO record): the tiles
        of the field in (bv, bu) order, rows first .. first + cap - 1; a column's word is cu | cv << 3"""
        cols = [(np.int16, (2,)), (np.uint32, (64,)) if with_cost else None]
        (coords, cost), info, _ = self._window("sdm_get_world_ground_reach", cols, first, cap, WORLD_GROUND_REACH_INFO)
        return coords, cost, info

    def query_world_ground_reach(self, xyz=None, cells=None, on_device=False, n=None, out=None):
        """goals as (n, 3) global positions or as (n, 3) world cells -> WORLD_GROUND_REACH_RESULT per goal.  on_device: the
        one given of xyz / cells and out (n WORLD_GROUND_REACH_RESULT) are device pointers."""
        return self._goal_query("sdm_query_world_ground_reach", xyz, cells, _WORLD_CELLS, WORLD_GROUND_REACH_RESULT, on_device, n, out)

    def world_ground_reach_paths(self, xyz=None, cells=None, max_len=0, on_device=False, n=None, cells_out=None, len_out=None,
                                 fill=WORLD_REACH_NO_CELL):
        """-> (cells_out int32 [n, max_len, 3], len_out): row g holds the first min(len, max_len) world cells of goal g's
        path, goal first - the cells the robot's base stands in -, and `fill` behind them; len_out the true lengths (int32,
        0: no path).  on_device: the pointers are device pointers (cells_out n * max_len * 3 int32, len_out n int32) and
        nothing is returned."""
        return self._goal_paths("sdm_world_ground_reach_paths", xyz, cells, _WORLD_CELLS, max_len, fill, on_device, n, cells_out, len_out)

    def world_ground_reach_tiles_relaxed(self):
        """Diagnostic: the tiles the last world_ground_reach_update relaxed, summed over its rounds."""
        return self._out("sdm_debug_world_ground_reach_tiles", C.c_int64)

    # ---- world rays (sdm.h).  Segments and views through the archive, read live in stream order: host mode takes numpy
    # and waits, on_device=True takes device pointers (outputs 8-byte aligned), enqueues on the map's stream and returns.
    def query_world_segments(self, a, b=None, unknown_blocks=False, ignore_movable=False, on_device=False, n=None, out=None):
        """a, b: (n, 3) end points -> WORLD_SEGMENT_HIT per segment.  on_device: a is a device pointer to n rows of
        (ax ay az bx by bz) floats, b is None, out a device pointer to n WORLD_SEGMENT_HIT."""
        fl = (QUERY_UNKNOWN_BLOCKS if unknown_blocks else 0) | (WORLD_RAYS_IGNORE_MOVABLE if ignore_movable else 0)
        return self._query("sdm_query_world_segments", _rows6(a, b, on_device), np.float32, (-1, 6), WORLD_SEGMENT_HIT, fl, on_device, n, out)

    def query_world_views(self, views, dirs, reach_cells, with_rays=False, ignore_movable=False, on_device=False, n_views=None, n_rays=None,
                          out=None, rays_out=None):
        """views: VIEW records, dirs: (n_rays, 3) camera-frame ray vectors, reach_cells: the window's half width in world
        cells (1 .. WORLD_VIEW_MAX_REACH) -> VIEW_GAIN per view; with_rays: also the WORLD_SEGMENT_HIT of every ray, shaped
        (n_views, n_rays).  on_device: views, dirs, out (n_views VIEW_GAIN) and rays_out (n_views * n_rays
        WORLD_SEGMENT_HIT, or None) are device pointers, n_views and n_rays their lengths."""
        fl = WORLD_RAYS_IGNORE_MOVABLE if ignore_movable else 0
        if on_device:
            self._call("sdm_query_world_views", _ptr(int(views)), int(n_views), _ptr(int(dirs)), int(n_rays), int(reach_cells), _ptr(int(out)),
                       _dev(rays_out), fl | QUERY_ON_DEVICE)
            return None
        v = np.ascontiguousarray(views, dtype=VIEW).reshape(-1)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        gain = np.empty(len(v), VIEW_GAIN)
        rays = np.empty((len(v), len(d)), WORLD_SEGMENT_HIT) if with_rays else None
        self._call("sdm_query_world_views", _ptr(v), len(v), _ptr(d), len(d), int(reach_cells), _ptr(gain), _ptr(rays), fl)
        return (gain, rays) if with_rays else gain

    def set_world_view_batch(self, max_views_in_flight):
        """Test hook: query_world_views keeps at most this many views in flight (<= 0: the library's choice)
        (sdm_debug_world_view_batch)."""
        self._call("sdm_debug_world_view_batch", int(max_views_in_flight))

    # ---- the world mesh (sdm.h).  world_mesh_update builds the faces and welded vertices of the archive's surface and WAITS
    # for the counts that size its lists; world_mesh() and world_mesh_device() answer for that build - a snapshot - until the
    # next one, whatever happens to the archive in between.
    def world_mesh_update(self, labels=None, track=-1, static_only=False, movable_only=False, observed_only=False, skip_unknown_faces=False,
                          skip_absent_faces=False, box=None, max_faces=0, max_vertices=0):
        """labels: the label ids whose cells may be solid (None: all 256); track: -1 any, else that track's cells only; box:
        (bmin, bmax), the inclusive brick box of the field (None: every archived brick); max_faces / max_vertices: caps of the
        two lists (0: none) - a build over one raises SdmError (SDM_ERR_CAPACITY), world_mesh_info() has the true counts"""
        o = np.zeros(1, WORLD_MESH_OPTIONS)
        o["labels"] = np.full(8, 0xFFFFFFFF, np.uint32) if labels is None else label_mask(labels)
        o["track"], o["max_faces"], o["max_vertices"] = track, max_faces, max_vertices
        o["flags"] = ((WORLD_MESH_STATIC_ONLY if static_only else 0) | (WORLD_MESH_MOVABLE_ONLY if movable_only else 0) |
                      (WORLD_MESH_OBSERVED_ONLY if observed_only else 0) | (WORLD_MESH_SKIP_UNKNOWN_FACES if skip_unknown_faces else 0) |
                      (WORLD_MESH_SKIP_ABSENT_FACES if skip_absent_faces else 0) | (WORLD_MESH_BOX if box is not None else 0))
        if box is not None:
            o["bmin"], o["bmax"] = np.asarray(box[0], np.int32), np.asarray(box[1], np.int32)
        self._call("sdm_world_mesh_update", _ptr(o))

    def world_mesh_info(self):
        """-> a WORLD_MESH_INFO record (true counts, also of a build over a cap)"""
        info = np.zeros(1, WORLD_MESH_INFO)
        self._call("sdm_get_world_mesh_info", _ptr(info))
        return info[0]

    def world_mesh(self):
        """-> dict(coords int16[b, 3], faces WORLD_MESH_FACE[n], quads uint32[n, 4], corners int32[m, 3], xyz float32[m, 3],
        info): the field bricks' coordinates (faces["brick"] indexes them), the faces, their vertex ids, the vertices as world
        lattice corners and as positions.  A build over a cap raises SdmError (SDM_ERR_CAPACITY)."""
        info = self.world_mesh_info()
        n, k, b = int(info["n_faces"]), int(info["n_vertices"]), int(info["n_bricks"])
        coords, faces, quads = np.empty((b, 3), np.int16), np.empty(n, WORLD_MESH_FACE), np.empty((n, 4), np.uint32)
        corners, xyz = np.empty((k, 3), np.int32), np.empty((k, 3), np.float32)
        got = C.c_int64(0)
        self._call("sdm_get_world_mesh_faces", _ptr(coords), _ptr(faces), _ptr(quads), 0, n, C.byref(got))
        self._call("sdm_get_world_mesh_vertices", _ptr(corners), _ptr(xyz), 0, k, C.byref(got))
        return dict(coords=coords, faces=faces, quads=quads, corners=corners, xyz=xyz, info=info)

    def world_mesh_device(self):
        """-> (faces, quads, corners): device addresses of the last build's lists (WORLD_MESH_FACE, 4 uint32 per face, 3 int32
        per vertex), valid until the next world_mesh_update, to be read in stream order on the map's stream"""
        p = [C.c_void_p() for _ in range(3)]
        self._call("sdm_world_mesh_device", *(C.byref(x) for x in p))
        return tuple(x.value for x in p)

    def save_world_ply(self, path, **update_kwargs):
        """world_mesh_update(**update_kwargs), then the mesh as an ASCII PLY (write_ply: two triangles a quad) -> the dict of
        world_mesh().  Host code."""
        self.world_mesh_update(**update_kwargs)
        mesh = self.world_mesh()
        write_ply(path, mesh["xyz"], mesh["quads"])
        return mesh

    def save_world(self, path):
        """the archive as a NumPy .npz: bricks (WORLD_BRICK), cells (uint32 [n, 512]) and the map's voxel_size (float32)"""
        bricks, cells = self.world_bricks()
        with open(path, "wb") as f:
            np.savez(f, bricks=bricks, cells=cells, voxel_size=np.float32(self.cfg.voxel_size))

    def load_world(self, path, **import_kwargs):
        """world_import of a file save_world wrote -> the number of bricks in it; ValueError if the file's voxel_size is not,
        bit for bit, this map's"""
        with np.load(path) as z:
            bricks, cells, size = z["bricks"], z["cells"], z["voxel_size"]
        if size.dtype != np.float32 or size.tobytes() != np.float32(self.cfg.voxel_size).tobytes():
            raise ValueError("load_world: the file's voxel_size %r is not the map's %r" % (size, np.float32(self.cfg.voxel_size)))
        self.world_import(bricks.astype(WORLD_BRICK, copy=False), cells, **import_kwargs)
        return len(bricks)

    def occupied(self, cap=None, zero_center=False, free=False, mark_fov=False):
        cap = cap or self.v_count
        out = np.empty(cap, POINT)
        n = C.c_size_t()
        fn = self.L.sdm_get_freespace if free else self.L.sdm_get_occupied
        _check(self.L, fn(self.h, _ptr(out), cap, C.byref(n), (1 if zero_center else 0) | (2 if mark_fov else 0)),
               "sdm_get_occupied")
        return out[:min(n.value, cap)], n.value

    def set_colours(self, label_bgr, perm, background_label=0, colour_by_label=False, jet_axis=0, evaluation_format=False):
        """label_bgr: (256, 3) uint8 BGR per label id; perm: 256 uint8 (color_map_int_256_)."""
        c = ColourConfig()
        lb = np.ascontiguousarray(label_bgr, np.uint8).reshape(256, 3)
        pm = np.ascontiguousarray(perm, np.uint8).reshape(256)
        C.memmove(c.label_bgr, lb.ctypes.data, 768)
        C.memmove(c.perm, pm.ctypes.data, 256)
        c.background_label, c.colour_by_label = int(background_label), 1 if colour_by_label else 0
        c.jet_axis, c.evaluation_format = int(jet_axis), 1 if evaluation_format else 0
        self._call("sdm_set_colours", C.byref(c))

    def occupied_rgb(self, cap=None, zero_center=False, free=False):
        """getOccupancyResult's cloud coloured and packed on the device: POINT_XYZRGB records."""
        cap = cap or self.v_count
        out = np.empty(cap, POINT_XYZRGB)
        n = C.c_size_t()
        fn = self.L.sdm_get_freespace_rgb if free else self.L.sdm_get_occupied_rgb
        _check(self.L, fn(self.h, _ptr(out), cap, C.byref(n), 1 if zero_center else 0), "sdm_get_occupied_rgb")
        return out[:min(n.value, cap)], n.value

    def object_particle_count(self, track):
        return self._out("sdm_object_particle_count", C.c_int64, track)

    def tracks_with_particles(self):
        """Track ids that own at least one slot, ascending (the non-empty keys of the reference's indices_map)."""
        out = np.zeros(65536, np.int32)
        n = C.c_int32(0)
        self._call("sdm_tracks_with_particles", _ptr(out), out.size, C.byref(n))
        return out[:n.value].copy()

    def stats_unchecked(self):
        """sdm_get_stats without raising on the status it returns (it reports the frame's capacity errors and fills the
        structure all the same)"""
        return self.stats(check=False)

    def stats(self, count_live=False, check=True):
        s = Stats()
        rc = self.L.sdm_get_stats(self.h, C.byref(s), 1 if count_live else 0)
        if check:
            _check(self.L, rc, "sdm_get_stats")
        d = {k: getattr(s, k) for k, _ in Stats._fields_ if k not in ("stage_ms", "restamped_slabs")}
        d["stage_ms"] = list(s.stage_ms)
        d["restamped_slabs"] = list(s.restamped_slabs)
        return d

    def set_profiling(self, on=True):
        self._call("sdm_set_profiling", 1 if on else 0)

    def force_generic_flood(self, on=True):
        self._call("sdm_debug_force_generic_flood", 1 if on else 0)

    def ring_state(self):
        r = RingState()
        self._call("sdm_get_ring_state", C.byref(r))
        return {"global_time_stamp": r.global_time_stamp, "moved_steps": list(r.moved_steps),
                "eq_steps": list(r.eq_steps), "map_center": list(r.map_center), "last_pos": list(r.last_pos),
                "birth_cursor": r.birth_cursor, "move_cursor": r.move_cursor}

    def set_ring_state(self, d):
        r = RingState()
        r.global_time_stamp = d["global_time_stamp"]
        for i in range(3):
            r.moved_steps[i] = d["moved_steps"][i]
            r.eq_steps[i] = d["eq_steps"][i]
            r.map_center[i] = d["map_center"][i]
            r.last_pos[i] = d["last_pos"][i]
        r.birth_cursor = d["birth_cursor"]
        r.move_cursor = d["move_cursor"]
        self._call("sdm_set_ring_state", C.byref(r))

    def stamps(self):
        c = self.cfg
        sx = np.empty(1 << c.x_n, np.uint32)
        sy = np.empty(1 << c.y_n, np.uint32)
        sz = np.empty(1 << c.z_n, np.uint32)
        self._call("sdm_get_stamps", _ptr(sx), _ptr(sy), _ptr(sz))
        return sx, sy, sz

    def set_stamps(self, sx, sy, sz):
        sx, sy, sz = (np.ascontiguousarray(a, dtype=np.uint32) for a in (sx, sy, sz))
        self._call("sdm_set_stamps", _ptr(sx), _ptr(sy), _ptr(sz))

    def dump_state(self):
        n = self.v_count * self.S
        st = {k: np.empty(n, dt) for k, dt in STATE_FIELDS}
        self._call("sdm_dump_state", *[_ptr(st[k]) for k, _ in STATE_FIELDS])
        return st

    def load_state(self, st):
        arrs = [np.ascontiguousarray(st[k], dtype=dt) for k, dt in STATE_FIELDS]
        self._call("sdm_load_state", *[_ptr(a) for a in arrs])

    def ck_kappa(self):
        out = np.empty(self.W * self.H, np.float32)
        self._call("sdm_get_ck_kappa", _ptr(out))
        return out.reshape(self.H, self.W)

    def bin_counts(self):
        out = np.empty(self.W * self.H, np.uint32)
        self._call("sdm_get_bin_counts", _ptr(out))
        return out.reshape(self.H, self.W)

    def bins(self):
        n = C.c_int64()
        self._call("sdm_get_bins", None, 0, C.byref(n))
        out = np.empty(max(n.value, 1), np.uint32)
        self._call("sdm_get_bins", _ptr(out), n.value, C.byref(n))
        return out[:n.value]

    def extrinsic(self):
        out = np.empty(16, np.float32)
        self._call("sdm_get_extrinsic", _ptr(out))
        return out.reshape(4, 4)

    def fill_dense_ex(self, mode):
        self._call("sdm_debug_fill_dense_ex", mode)

    def hinted_groups(self):
        return self._out("sdm_debug_hinted_groups", C.c_int64)

    def force_sweep_lists(self, mode):
        """Test hook: 1 / 0 = the non-incremental sweeps always / never hand their sparse voxels to per-tile lists, -1 = the
        library picks per sweep (sdm_debug_sweep_lists)."""
        self._call("sdm_debug_sweep_lists", int(mode))

    def sweep_mode(self):
        """Test hook: bit 0 - the next non-incremental sweep uses per-tile lists; bit 1 - it is one launch (every group of
        512 voxels was dense in the last one) (sdm_debug_sweep_mode)."""
        return self._out("sdm_debug_sweep_mode", C.c_int32)

    def set_alias_cap(self, cap):
        """Test hook: the table of older owner-set memberships reports its overflow at `cap` entries (before the first frame)."""
        self._call("sdm_debug_alias_cap", int(cap))

    def fill_dense(self):
        self._call("sdm_debug_fill_dense")

    def time_occupancy_sweep(self, iters=20):
        return self._out("sdm_time_occupancy_sweep", C.c_float, iters)


def forecast_stamps(voxel_size, motions, horizons, swept=False, cap=None):
    """The stamps a forecast build makes of these motions and horizons (sdm_forecast_stamps: host code, no map, no device)
    -> FORECAST_STAMP records (with cap: at most so many, and the true count as a second value)"""
    mo = np.zeros(0, MOTION) if motions is None else np.ascontiguousarray(motions, dtype=MOTION).reshape(-1)
    t = np.ascontiguousarray(horizons, dtype=np.float32).reshape(-1)
    fl, n = FORECAST_SWEPT if swept else 0, C.c_int64(0)
    if cap is None:
        _call("sdm_forecast_stamps", float(voxel_size), _ptr(mo), len(mo), _ptr(t), len(t), fl, None, 0, C.byref(n))
    k = n.value if cap is None else int(cap)
    out = np.zeros(k, FORECAST_STAMP)
    _call("sdm_forecast_stamps", float(voxel_size), _ptr(mo), len(mo), _ptr(t), len(t), fl, _ptr(out), k, C.byref(n))
    return out if cap is None else (out[:min(k, n.value)], n.value)


def pinhole_rays(cfg, stride=1):
    """The camera-frame ray table of every `stride`-th pixel centre of cfg's pinhole camera: ((u - cx) / fx, (v - cy) / fy, 1)
    in float32, shaped (rows, columns, 3), rows v = 0, stride, ... and columns u = 0, stride, ...  With a view's range
    r the ray of pixel (u, v) ends at planar depth r (query_views)."""
    get = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
    u = np.arange(0, int(get("width")), int(stride), dtype=np.float32)
    v = np.arange(0, int(get("height")), int(stride), dtype=np.float32)
    x = (u - np.float32(get("cx"))) / np.float32(get("fx"))
    y = (v - np.float32(get("cy"))) / np.float32(get("fy"))
    out = np.empty((len(v), len(u), 3), np.float32)
    out[..., 0], out[..., 1], out[..., 2] = x[None, :], y[:, None], 1.0
    return out


def comm_unique_id():
    """128-byte RCCL id drawn on this process (rank 0 broadcasts it to the other ranks)."""
    buf = np.zeros(128, np.uint8)
    _call("sdm_comm_unique_id", _ptr(buf))
    return buf.tobytes()


def test_scan(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    out = np.empty_like(a)
    _call("sdm_test_scan", _ptr(a), _ptr(out), a.size)
    return out


def test_sort_pairs(keys, vals, nbits):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    vals = np.ascontiguousarray(vals, dtype=np.uint32)
    ko, vo = np.empty_like(keys), np.empty_like(vals)
    _call("sdm_test_sort_pairs", _ptr(keys), _ptr(vals), _ptr(ko), _ptr(vo), keys.size, nbits)
    return ko, vo


TEST_IN_PLACE, TEST_COUNT_ON_DEVICE, TEST_GUARD_WORDS = 1, 2, 64  # sdm.h, SDM_TEST_*


def test_scratch_elems(sort, n):
    """words of scratch the scan (sort = False) or the sort (True) asks for at n elements (sdm_test_scratch_elems)"""
    v = C.c_int64(0)
    _call("sdm_test_scratch_elems", int(bool(sort)), int(n), C.byref(v))
    return v.value


def _seq_args(capacity, count, arrays):
    capacity = np.ascontiguousarray(capacity, dtype=np.int64)
    count = capacity.copy() if count is None else np.ascontiguousarray(count, dtype=np.int64)
    if capacity.ndim != 1 or capacity.size == 0 or count.shape != capacity.shape:
        raise ValueError("one capacity and one count per call")
    arrays = [np.ascontiguousarray(a, dtype=np.uint32) for a in arrays]
    if any(a.shape != (int(capacity.sum()),) for a in arrays):
        raise ValueError("the arrays hold one slice of `capacity` words per call")
    return capacity, count, arrays


def test_scan_seq(capacity, a, out, count=None, in_place=False, count_on_device=False, want_scratch=False):
    """sdm_test_scan_seq: scans of the slices of `a` (capacity[i] words each) back to back on one scratch.  `out` is what the
    output buffer holds before the calls.  Returns (the output buffer after them, guard words intact, the scratch as the last
    call left it or None)."""
    capacity, count, (a, out) = _seq_args(capacity, count, [a, out])
    out = out.copy()
    flags = (TEST_IN_PLACE if in_place else 0) | (TEST_COUNT_ON_DEVICE if count_on_device else 0)
    scratch = np.empty(test_scratch_elems(False, capacity.max()), np.uint32) if want_scratch else None
    ok = C.c_int32(0)
    _call("sdm_test_scan_seq", capacity.size, _ptr(capacity), _ptr(count), flags, _ptr(a), _ptr(out), C.byref(ok), _ptr(scratch))
    return out, bool(ok.value), scratch


def test_sort_pairs_seq(capacity, nbits, keys, vals, keys_out, vals_out, count=None, count_on_device=False, want_scratch=False):
    """sdm_test_sort_pairs_seq: sorts of the slices of (keys, vals) back to back on one scratch; keys_out / vals_out are what
    the second pair of buffers holds before the calls.  Returns (keys, vals of the pair each call named, the value each call
    returned, guard words intact, the scratch as the last call left it or None)."""
    capacity, count, (keys, vals, keys_out, vals_out) = _seq_args(capacity, count, [keys, vals, keys_out, vals_out])
    nbits = np.ascontiguousarray(np.broadcast_to(np.asarray(nbits, np.int32), capacity.shape))
    keys_out, vals_out = keys_out.copy(), vals_out.copy()
    which = np.zeros(capacity.size, np.int32)
    scratch = np.empty(test_scratch_elems(True, capacity.max()), np.uint32) if want_scratch else None
    ok = C.c_int32(0)
    _call("sdm_test_sort_pairs_seq", capacity.size, _ptr(capacity), _ptr(count), _ptr(nbits), TEST_COUNT_ON_DEVICE if count_on_device else 0,
          _ptr(keys), _ptr(vals), _ptr(keys_out), _ptr(vals_out), _ptr(which), C.byref(ok), _ptr(scratch))
    return keys_out, vals_out, which, bool(ok.value), scratch


class WorldChanges:
    """What the block sees against what the archive remembers (sdm.h, "world changes"): the client of one map's change
    layer.  update() compares the last frame's results with the archive and WAITS until the build is complete; regions(),
    cells(), labels() and query() answer for that build - a snapshot that later frames, updates, imports, retains and clears
    leave alone.  The intended use is one update() between a frame and its world_update()."""

    def __init__(self, map):
        self.map = map

    def update(self, face_connected=False, by_label=False, static_only=False, observed_only=False, max_last_stamp=None,
               labels=ALL_LABELS, classes=ALL_CHANGE_CLASSES, min_cells=1, max_cells=0):
        """labels: the label ids that admit a changed cell (default: all); classes: the change classes listed (default: all
        three); max_last_stamp: only bricks last archived at or before that stamp are compared; by_label: a region's key is
        class and label pair"""
        o = np.zeros(1, WORLD_CHANGES_OPTIONS)
        o["flags"] = ((WORLD_CHANGES_FACE_CONNECTED if face_connected else 0) | (WORLD_CHANGES_BY_LABEL if by_label else 0) |
                      (WORLD_CHANGES_STATIC_ONLY if static_only else 0) | (WORLD_CHANGES_OBSERVED_ONLY if observed_only else 0) |
                      (WORLD_CHANGES_OLDER if max_last_stamp is not None else 0))
        o["min_cells"], o["max_cells"] = int(min_cells), int(max_cells)
        o["labels"] = label_mask(labels)
        o["classes"] = sum(1 << int(c) for c in set(classes))
        o["max_last_stamp"] = 0 if max_last_stamp is None else int(max_last_stamp)
        self.map._call("sdm_world_changes_update", _ptr(o))

    def regions(self):
        """-> (table, info): WORLD_CHANGE_REGION entries in ascending first_index, a WORLD_CHANGES_INFO record"""
        got = C.c_int32(0)
        info = np.zeros(1, WORLD_CHANGES_INFO)
        self.map._call("sdm_get_world_changes", None, 0, C.byref(got), _ptr(info))
        out = np.empty(got.value, WORLD_CHANGE_REGION)
        self.map._call("sdm_get_world_changes", _ptr(out), got.value, C.byref(got), None)
        return out, info[0]

    def cells(self, first=0, cap=None):
        """-> (cells int32 [n, 3], now uint32 [n], before uint32 [n], cls uint8 [n], region uint32 [n]): rows first ..
        first + cap - 1 of the cell list, ascending in (brick order, cell word); region indexes the table
        (WORLD_CHANGE_UNLISTED: below min_cells)"""
        cols = [(np.int32, (3,)), (np.uint32, ()), (np.uint32, ()), (np.uint8, ()), (np.uint32, ())]
        return tuple(self.map._window("sdm_get_world_change_cells", cols, first, cap)[0])

    def labels(self):
        """-> (appeared, vanished, relabelled), uint64 [256] each: the listed cells per label"""
        out = [np.zeros(256, np.uint64) for _ in range(3)]
        self.map._call("sdm_get_world_change_labels", *[_ptr(a) for a in out])
        return tuple(out)

    def query(self, xyz=None, cells=None, on_device=False, n=None, out=None):
        """(n, 3) global positions or (n, 3) world cells -> WORLD_CHANGE_RESULT per entry.  on_device: the one given of
        xyz / cells and out (n WORLD_CHANGE_RESULT) are device pointers."""
        return self.map._goal_query("sdm_query_world_changes", xyz, cells, _WORLD_CELLS, WORLD_CHANGE_RESULT, on_device, n, out)
