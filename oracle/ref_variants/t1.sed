# Variant "t1": the SETTING 3 block with the numbers of the project's T1 configuration (64 x 32 x 64 voxels of 0.3 m,
# 4 slots, 384 x 216 halved to 192 x 108 by the block's BOOST mode, f = 120, c = (96, 54) after halving, 15 m).
/^#elif SETTING == 3/,/^#else/{
s/\(C_VOXEL_NUM_AXIS_X_N = \)[0-9]*/\16/
s/\(C_VOXEL_NUM_AXIS_Y_N = \)[0-9]*/\15/
s/\(C_VOXEL_NUM_AXIS_Z_N = \)[0-9]*/\16/
s/\(C_MAX_PARTICLE_NUM_PER_VOXEL_N = \)[0-9]*/\12/
s/\(C_VOXEL_SIZE = \)[0-9.]*f/\10.3f/
s/\(g_camera_fx_set = \)[0-9.]*/\1240.0/
s/\(g_camera_fy_set = \)[0-9.]*/\1240.0/
s/\(g_camera_cx_set = \)[0-9.]*/\1192.0/
s/\(g_camera_cy_set = \)[0-9.]*/\1108.0/
s/\(g_image_width_set = \)[0-9]*/\1384/
s/\(g_image_height_set = \)[0-9]*/\1216/
s/\(g_depth_range_max = \)[0-9.]*f/\115.f/
}
