# Variant "cloud_static": SETTING 0 (no BOOST mode, g_consider_instance = false) with T0's grid, camera and image.
s/^\(#define SETTING \)[0-9]/\10/
/^#if SETTING == 0/,/^#elif SETTING == 1/{
s/\(C_VOXEL_NUM_AXIS_X_N = \)[0-9]*/\15/
s/\(C_VOXEL_NUM_AXIS_Y_N = \)[0-9]*/\15/
s/\(C_VOXEL_NUM_AXIS_Z_N = \)[0-9]*/\15/
s/\(C_MAX_PARTICLE_NUM_PER_VOXEL_N = \)[0-9]*/\13/
s/\(C_VOXEL_SIZE = \)[0-9.]*f/\10.4f/
s/\(g_camera_fx_set = \)[0-9.]*/\180.0/
s/\(g_camera_fy_set = \)[0-9.]*/\180.0/
s/\(g_camera_cx_set = \)[0-9.]*/\164.0/
s/\(g_camera_cy_set = \)[0-9.]*/\140.0/
s/\(g_image_width_set = \)[0-9]*/\1128/
s/\(g_image_height_set = \)[0-9]*/\180/
s/\(g_depth_range_max = \)[0-9.]*f/\112.f/
}
