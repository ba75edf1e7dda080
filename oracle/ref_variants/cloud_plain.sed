# Variant "cloud_plain": SETTING 2 (no BOOST mode, no Sky exclusion, no box filter) with T0's grid, a 128 x 80 image and
# a camera of powers of two (f = 64, c = (64, 40)), for which the inverse intrinsics are exact in double.
s/^\(#define SETTING \)[0-9]/\12/
/^#elif SETTING == 2/,/^#elif SETTING == 3/{
s/\(C_VOXEL_NUM_AXIS_X_N = \)[0-9]*/\15/
s/\(C_VOXEL_NUM_AXIS_Y_N = \)[0-9]*/\15/
s/\(C_VOXEL_NUM_AXIS_Z_N = \)[0-9]*/\15/
s/\(C_MAX_PARTICLE_NUM_PER_VOXEL_N = \)[0-9]*/\13/
s/\(C_VOXEL_SIZE = \)[0-9.]*f/\10.4f/
s/\(g_camera_fx_set = \)[0-9.]*f/\164.0f/
s/\(g_camera_fy_set = \)[0-9.]*f/\164.0f/
s/\(g_camera_cx_set = \)[0-9.]*f/\164.0f/
s/\(g_camera_cy_set = \)[0-9.]*f/\140.0f/
s/\(g_image_width_set = \)[0-9]*/\1128/
s/\(g_image_height_set = \)[0-9]*/\180/
s/\(g_depth_range_max = \)[0-9.]*f/\112.f/
}
