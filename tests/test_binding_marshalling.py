"""The binding's method bodies, without a device: every wrapper marshals its smallest valid host-mode arguments - one
point, one segment, max_len=2 - into its C entry point on a map that was never created (h = None, a null sdm_map *).  The
entry point refuses the null map before it touches it, so the wrapper must raise SdmError naming that function with
SDM_ERR_INVALID_ARGUMENT: not TypeError or ctypes.ArgumentError (arguments that do not fit the `sig` table), and it must
not return.

CASES: (method, or method-variant; the C function its error names; the call).  A wrapper that makes several calls names
its first, and occupied(free=True) / occupied_rgb(free=True) name the function of their free=False form, as they always
have.

Every entry point the binding calls on a map refuses a null one before it touches it, so no wrapper is left out for the
library's sake.  LEFT_OUT names the three public methods without a case, each with its reason; the module-level
functions (forecast_stamps, comm_unique_id, test_*) take no map.
"""
import ctypes

import numpy as np
import pytest

from semantic_dsp_map_amd import binding as B

P1 = np.array([[0.5, 0.25, 0.125]], np.float32)
C1 = np.array([[1, 2, 3]], np.int32)
W1 = np.array([7], np.uint32)
POSE = ([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])
W, H = 4, 2


def _frame():
    return (np.ones(W * H, np.float32), np.zeros(W * H, B.LABELED_POINT)) + POSE


def _bricks():
    return np.zeros(1, B.WORLD_BRICK), np.zeros((1, 512), np.uint32)


CASES = [
    ("clear", "sdm_clear", lambda g: g.clear()),
    ("set_params", "sdm_set_params", lambda g: g.set_params({k: 0 for k, _ in B.Params._fields_})),
    ("generate_noise_table", "sdm_generate_noise_table", lambda g: g.generate_noise_table(n=4)),
    ("upload_noise_table", "sdm_upload_noise_table", lambda g: g.upload_noise_table(np.zeros(4, np.float32))),
    ("download_noise_table", "sdm_download_noise_table", lambda g: g.download_noise_table(4)),
    ("download_pdf_table", "sdm_download_pdf_table", lambda g: g.download_pdf_table()),
    ("update", "sdm_update", lambda g: g.update(*_frame())),
    ("update_raw", "sdm_update_raw_ex",
     lambda g: g.update_raw(np.ones((H, W), np.float32), np.zeros((H, W), np.uint8), np.zeros(256, np.uint16), [], *POSE)),
    ("labeled_cloud", "sdm_get_labeled_cloud", lambda g: g.labeled_cloud()),
    ("update_begin", "sdm_update_begin", lambda g: g.update_begin(*_frame())),
    ("frame_start", "sdm_frame_start", lambda g: g.frame_start(*_frame())),
    ("frame_moves", "sdm_frame_moves", lambda g: g.frame_moves()),
    ("frame_moves_pending", "sdm_frame_moves_pending", lambda g: g.frame_moves_pending()),
    ("frame_predict", "sdm_frame_predict", lambda g: g.frame_predict()),
    ("set_halo_buffers", "sdm_set_halo_buffers", lambda g: g.set_halo_buffers(8, 16, 24, 32, 1)),
    ("comm_init", "sdm_comm_init", lambda g: g.comm_init(bytes(128))),
    ("ipc_create", "sdm_ipc_create", lambda g: g.ipc_create()),
    ("ipc_connect", "sdm_ipc_connect", lambda g: g.ipc_connect(bytes(64))),
    ("comm_set_options", "sdm_comm_set_options", lambda g: g.comm_set_options()),
    ("update_sharded", "sdm_update_sharded", lambda g: g.update_sharded(*_frame())),
    ("ck_chunk_elems", "sdm_ck_chunk_elems", lambda g: g.ck_chunk_elems()),
    ("ck_reduce", "sdm_ck_reduce", lambda g: g.ck_reduce(8, 16)),
    ("comm_timing", "sdm_comm_timing", lambda g: g.comm_timing()),
    ("comm_times", "sdm_get_comm_times", lambda g: g.comm_times()),
    ("device_alloc", "sdm_device_alloc", lambda g: g.device_alloc(16)),
    ("device_free", "sdm_device_free", lambda g: g.device_free(8)),
    ("device_upload", "sdm_device_upload", lambda g: g.device_upload(8, np.zeros(2, np.float32))),
    ("device_put", "sdm_device_alloc", lambda g: g.device_put(np.zeros(2, np.float32))),
    ("device_download", "sdm_device_download", lambda g: g.device_download(8, 8)),
    ("device_synchronize", "sdm_device_synchronize", lambda g: g.device_synchronize()),
    ("update_finish", "sdm_update_finish", lambda g: g.update_finish()),
    ("stream", "sdm_stream", lambda g: g.stream()),
    ("set_stream", "sdm_set_stream", lambda g: g.set_stream(0)),
    ("set_ck_buffer", "sdm_set_ck_buffer", lambda g: g.set_ck_buffer(None)),
    ("set_issue_mode", "sdm_set_issue_mode", lambda g: g.set_issue_mode(0)),
    ("synchronize", "sdm_synchronize", lambda g: g.synchronize()),
    ("voxels", "sdm_get_voxels", lambda g: g.voxels()),
    ("query_points", "sdm_query_points", lambda g: g.query_points(P1)),
    ("query_points-with_index", "sdm_query_points", lambda g: g.query_points(P1, with_index=True)),
    ("query_segments", "sdm_query_segments", lambda g: g.query_segments(P1, P1 + 1)),
    ("query_boxes", "sdm_query_boxes", lambda g: g.query_boxes(P1, P1 + 1)),
    ("esdf_update", "sdm_esdf_update", lambda g: g.esdf_update()),
    ("esdf", "sdm_get_esdf", lambda g: g.esdf()),
    ("query_distance", "sdm_query_distance", lambda g: g.query_distance(P1)),
    ("instances_update", "sdm_instances_update", lambda g: g.instances_update()),
    ("instances", "sdm_get_instances", lambda g: g.instances(cap=1)),
    ("label_cells", "sdm_get_label_cells", lambda g: g.label_cells()),
    ("frontiers_update", "sdm_frontiers_update", lambda g: g.frontiers_update()),
    ("frontiers", "sdm_get_frontier_clusters", lambda g: g.frontiers(cap=1)),
    ("frontier_cells", "sdm_get_frontier_cells", lambda g: g.frontier_cells()),
    ("query_views", "sdm_query_views", lambda g: g.query_views(np.zeros(1, B.VIEW), P1)),
    ("query_views-with_rays", "sdm_query_views", lambda g: g.query_views(np.zeros(1, B.VIEW), P1, with_rays=True)),
    ("set_view_batch", "sdm_debug_view_batch", lambda g: g.set_view_batch(1)),
    ("reach_update", "sdm_reach_update", lambda g: g.reach_update(starts=P1)),
    ("reach_update-cells", "sdm_reach_update", lambda g: g.reach_update(start_cells=W1)),
    ("reach", "sdm_get_reach", lambda g: g.reach()),
    ("query_reach", "sdm_query_reach", lambda g: g.query_reach(xyz=P1)),
    ("query_reach-cells", "sdm_query_reach", lambda g: g.query_reach(cells=W1)),
    ("reach_paths", "sdm_reach_paths", lambda g: g.reach_paths(xyz=P1, max_len=2)),
    ("reach_paths-cells", "sdm_reach_paths", lambda g: g.reach_paths(cells=W1, max_len=2)),
    ("reach_tiles", "sdm_debug_reach_tiles", lambda g: g.reach_tiles()),
    ("forecast_update", "sdm_forecast_update", lambda g: g.forecast_update(np.zeros(1, B.MOTION), [0.5])),
    ("forecast", "sdm_get_forecast", lambda g: g.forecast()),
    ("forecast_cells", "sdm_get_forecast_cells", lambda g: g.forecast_cells()),
    ("query_forecast", "sdm_query_forecast", lambda g: g.query_forecast(np.zeros((1, 4), np.float32))),
    ("query_forecast_segments", "sdm_query_forecast_segments", lambda g: g.query_forecast_segments(np.zeros((1, 8), np.float32))),
    ("ground_update", "sdm_ground_update", lambda g: g.ground_update()),
    ("ground", "sdm_get_ground", lambda g: g.ground()),
    ("query_ground", "sdm_query_ground", lambda g: g.query_ground(P1)),
    ("query_footprints", "sdm_query_footprints", lambda g: g.query_footprints(np.zeros(1, B.FOOTPRINT))),
    ("mesh_update", "sdm_mesh_update", lambda g: g.mesh_update()),
    ("mesh_info", "sdm_get_mesh_info", lambda g: g.mesh_info()),
    ("mesh", "sdm_get_mesh_info", lambda g: g.mesh()),
    ("mesh_device", "sdm_mesh_device", lambda g: g.mesh_device()),
    ("world_update", "sdm_world_update", lambda g: g.world_update()),
    ("world_clear", "sdm_world_clear", lambda g: g.world_clear()),
    ("world_info", "sdm_get_world_info", lambda g: g.world_info()),
    ("world_bricks", "sdm_get_world_bricks", lambda g: g.world_bricks()),
    ("world_bricks-window", "sdm_get_world_bricks", lambda g: g.world_bricks(with_cells=False, first=0, cap=1)),
    ("world_occupied", "sdm_get_world_occupied", lambda g: g.world_occupied()),
    ("query_world", "sdm_query_world_points", lambda g: g.query_world(P1)),
    ("world_region", "sdm_get_world_region", lambda g: g.world_region((0, 0, 0), (1, 1, 1))),
    ("world_import", "sdm_world_import", lambda g: g.world_import(*_bricks())),
    ("world_match", "sdm_world_match", lambda g: g.world_match(*_bricks(), radius=(0, 0, 0))),
    ("world_align", "sdm_world_match", lambda g: g.world_align(*_bricks(), search=(0, 0, 0))),
    ("world_retain", "sdm_world_retain", lambda g: g.world_retain()),
    ("world_reach_update", "sdm_world_reach_update", lambda g: g.world_reach_update(starts=P1)),
    ("world_reach_update-cells", "sdm_world_reach_update", lambda g: g.world_reach_update(start_cells=C1)),
    ("world_reach", "sdm_get_world_reach", lambda g: g.world_reach()),
    ("query_world_reach", "sdm_query_world_reach", lambda g: g.query_world_reach(xyz=P1)),
    ("query_world_reach-cells", "sdm_query_world_reach", lambda g: g.query_world_reach(cells=C1)),
    ("world_reach_paths", "sdm_world_reach_paths", lambda g: g.world_reach_paths(xyz=P1, max_len=2)),
    ("world_reach_paths-cells", "sdm_world_reach_paths", lambda g: g.world_reach_paths(cells=C1, max_len=2)),
    ("world_reach_bricks_relaxed", "sdm_debug_world_reach_bricks", lambda g: g.world_reach_bricks_relaxed()),
    ("world_frontiers_update", "sdm_world_frontiers_update", lambda g: g.world_frontiers_update()),
    ("world_frontiers", "sdm_get_world_frontier_clusters", lambda g: g.world_frontiers()),
    ("world_frontier_cells", "sdm_get_world_frontier_cells", lambda g: g.world_frontier_cells()),
    ("world_objects_update", "sdm_world_objects_update", lambda g: g.world_objects_update()),
    ("world_objects", "sdm_get_world_objects", lambda g: g.world_objects()),
    ("world_object_cells", "sdm_get_world_object_cells", lambda g: g.world_object_cells()),
    ("world_object_labels", "sdm_get_world_object_labels", lambda g: g.world_object_labels()),
    ("world_object_members", "sdm_get_world_object_cells", lambda g: g.world_object_members(0)),
    ("query_world_objects", "sdm_query_world_objects", lambda g: g.query_world_objects(xyz=P1)),
    ("query_world_objects-cells", "sdm_query_world_objects", lambda g: g.query_world_objects(cells=C1)),
    ("world_esdf_update", "sdm_world_esdf_update", lambda g: g.world_esdf_update(1)),
    ("world_esdf", "sdm_get_world_esdf", lambda g: g.world_esdf()),
    ("query_world_distance", "sdm_query_world_distance", lambda g: g.query_world_distance(xyz=P1)),
    ("query_world_distance-cells", "sdm_query_world_distance", lambda g: g.query_world_distance(cells=C1)),
    ("world_ground_update", "sdm_world_ground_update", lambda g: g.world_ground_update()),
    ("world_ground", "sdm_get_world_ground", lambda g: g.world_ground()),
    ("query_world_ground", "sdm_query_world_ground", lambda g: g.query_world_ground(xyz=P1)),
    ("query_world_ground-cells", "sdm_query_world_ground", lambda g: g.query_world_ground(cells=C1)),
    ("query_world_footprints", "sdm_query_world_footprints", lambda g: g.query_world_footprints(np.zeros(1, B.FOOTPRINT))),
    ("world_ground_reach_update", "sdm_world_ground_reach_update", lambda g: g.world_ground_reach_update(starts=P1)),
    ("world_ground_reach_update-cells", "sdm_world_ground_reach_update", lambda g: g.world_ground_reach_update(start_cells=C1)),
    ("world_ground_reach", "sdm_get_world_ground_reach", lambda g: g.world_ground_reach()),
    ("query_world_ground_reach", "sdm_query_world_ground_reach", lambda g: g.query_world_ground_reach(xyz=P1)),
    ("query_world_ground_reach-cells", "sdm_query_world_ground_reach", lambda g: g.query_world_ground_reach(cells=C1)),
    ("world_ground_reach_paths", "sdm_world_ground_reach_paths", lambda g: g.world_ground_reach_paths(xyz=P1, max_len=2)),
    ("world_ground_reach_paths-cells", "sdm_world_ground_reach_paths", lambda g: g.world_ground_reach_paths(cells=C1, max_len=2)),
    ("world_ground_reach_tiles_relaxed", "sdm_debug_world_ground_reach_tiles", lambda g: g.world_ground_reach_tiles_relaxed()),
    ("query_world_segments", "sdm_query_world_segments", lambda g: g.query_world_segments(P1, P1 + 1)),
    ("query_world_views", "sdm_query_world_views", lambda g: g.query_world_views(np.zeros(1, B.VIEW), P1, 1)),
    ("query_world_views-with_rays", "sdm_query_world_views", lambda g: g.query_world_views(np.zeros(1, B.VIEW), P1, 1, with_rays=True)),
    ("set_world_view_batch", "sdm_debug_world_view_batch", lambda g: g.set_world_view_batch(1)),
    ("world_mesh_update", "sdm_world_mesh_update", lambda g: g.world_mesh_update()),
    ("world_mesh_info", "sdm_get_world_mesh_info", lambda g: g.world_mesh_info()),
    ("world_mesh", "sdm_get_world_mesh_info", lambda g: g.world_mesh()),
    ("world_mesh_device", "sdm_world_mesh_device", lambda g: g.world_mesh_device()),
    ("save_world_ply", "sdm_world_mesh_update", lambda g: g.save_world_ply("unwritten.ply")),
    ("save_world", "sdm_get_world_bricks", lambda g: g.save_world("unwritten.npz")),
    ("occupied", "sdm_get_occupied", lambda g: g.occupied()),
    ("occupied-free", "sdm_get_occupied", lambda g: g.occupied(free=True)),
    ("set_colours", "sdm_set_colours", lambda g: g.set_colours(np.zeros((256, 3), np.uint8), np.arange(256))),
    ("occupied_rgb", "sdm_get_occupied_rgb", lambda g: g.occupied_rgb()),
    ("occupied_rgb-free", "sdm_get_occupied_rgb", lambda g: g.occupied_rgb(free=True)),
    ("object_particle_count", "sdm_object_particle_count", lambda g: g.object_particle_count(1)),
    ("tracks_with_particles", "sdm_tracks_with_particles", lambda g: g.tracks_with_particles()),
    ("stats", "sdm_get_stats", lambda g: g.stats()),
    ("set_profiling", "sdm_set_profiling", lambda g: g.set_profiling()),
    ("force_generic_flood", "sdm_debug_force_generic_flood", lambda g: g.force_generic_flood()),
    ("ring_state", "sdm_get_ring_state", lambda g: g.ring_state()),
    ("set_ring_state", "sdm_set_ring_state",
     lambda g: g.set_ring_state(dict(global_time_stamp=0, moved_steps=[0] * 3, eq_steps=[0] * 3, map_center=[0.0] * 3, last_pos=[0.0] * 3,
                                     birth_cursor=0, move_cursor=0))),
    ("stamps", "sdm_get_stamps", lambda g: g.stamps()),
    ("set_stamps", "sdm_set_stamps", lambda g: g.set_stamps([0, 0], [0, 0], [0, 0])),
    ("dump_state", "sdm_dump_state", lambda g: g.dump_state()),
    ("load_state", "sdm_load_state", lambda g: g.load_state({k: np.zeros(16, dt) for k, dt in B.STATE_FIELDS})),
    ("ck_kappa", "sdm_get_ck_kappa", lambda g: g.ck_kappa()),
    ("bin_counts", "sdm_get_bin_counts", lambda g: g.bin_counts()),
    ("bins", "sdm_get_bins", lambda g: g.bins()),
    ("extrinsic", "sdm_get_extrinsic", lambda g: g.extrinsic()),
    ("fill_dense_ex", "sdm_debug_fill_dense_ex", lambda g: g.fill_dense_ex(0)),
    ("hinted_groups", "sdm_debug_hinted_groups", lambda g: g.hinted_groups()),
    ("force_sweep_lists", "sdm_debug_sweep_lists", lambda g: g.force_sweep_lists(-1)),
    ("sweep_mode", "sdm_debug_sweep_mode", lambda g: g.sweep_mode()),
    ("set_alias_cap", "sdm_debug_alias_cap", lambda g: g.set_alias_cap(1)),
    ("fill_dense", "sdm_debug_fill_dense", lambda g: g.fill_dense()),
    ("time_occupancy_sweep", "sdm_time_occupancy_sweep", lambda g: g.time_occupancy_sweep(1)),
]

LEFT_OUT = {
    "close": "calls sdm_destroy only on a handle that is set, and never checks its status",
    "stats_unchecked": "is stats() without the check: it returns whatever sdm_get_stats filled in",
    "load_world": "reads a file first; its one call into the library is world_import's, which has a case",
}


@pytest.fixture(scope="module")
def unmade():
    """an SdmMap that sdm_create never saw: the loaded library, a null handle and the attributes the methods read"""
    g = object.__new__(B.SdmMap)
    g.L, g.h = B.load_library(), None
    g.cfg = B.Config(x_n=1, y_n=1, z_n=1, p_n=1, width=W, height=H, voxel_size=0.5)
    g.V, g.S, g.v_count, g.W, g.H = 8, 2, 8, W, H
    return g


@pytest.mark.parametrize("method, c_name, call", CASES, ids=[c[0] for c in CASES])
def test_wrapper_reaches_its_entry_point(unmade, method, c_name, call, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)      # (a wrapper that went on after its call would write its file here, not into the tree)
    with pytest.raises(B.SdmError) as e:
        call(unmade)
    assert not isinstance(e.value, (TypeError, ctypes.ArgumentError))
    assert str(e.value).startswith("%s failed: SDM_ERR_INVALID_ARGUMENT (" % c_name), str(e.value)


def test_cases_and_left_out_name_every_public_method():
    public = {n for n in vars(B.SdmMap) if not n.startswith("_") and callable(getattr(B.SdmMap, n))}
    named = {c[0].split("-")[0] for c in CASES} | set(LEFT_OUT)
    assert named == public, sorted(named ^ public)
