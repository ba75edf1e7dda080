# Variant "cloud_zed2": SETTING 3 / BOOST with the numbers of the project's T0 configuration, as t0.sed (32^3 voxels of
# 0.4 m, 8 slots, 256 x 160 halved to 128 x 80, f = 80, c = (64, 40) after halving, 12 m).
/^#elif SETTING == 3/,/^#else/{
s/\(C_VOXEL_NUM_AXIS_X_N = \)[0-9]*/\15/
s/\(C_VOXEL_NUM_AXIS_Y_N = \)[0-9]*/\15/
s/\(C_VOXEL_NUM_AXIS_Z_N = \)[0-9]*/\15/
s/\(C_MAX_PARTICLE_NUM_PER_VOXEL_N = \)[0-9]*/\13/
s/\(C_VOXEL_SIZE = \)[0-9.]*f/\10.4f/
s/\(g_camera_fx_set = \)[0-9.]*/\1160.0/
s/\(g_camera_fy_set = \)[0-9.]*/\1160.0/
s/\(g_camera_cx_set = \)[0-9.]*/\1128.0/
s/\(g_camera_cy_set = \)[0-9.]*/\180.0/
s/\(g_image_width_set = \)[0-9]*/\1256/
s/\(g_image_height_set = \)[0-9]*/\1160/
s/\(g_depth_range_max = \)[0-9.]*f/\112.f/
}
