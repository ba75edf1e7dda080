# Variant "cloud_third": SETTING 3 / BOOST with T0's grid and g_image_rescale = 0.3f: 427 x 267 reduced to 128 x 80,
# where the float product int(i * (1.f / 0.3f)) and floor(i / 0.3) name different source rows.  The sensor's camera
# numbers are arbitrary; after the rescale f is about 96.3 and 93.9, c about (63.2, 40.9), none of them round.
/^#elif SETTING == 3/,/^#else/{
s/\(C_VOXEL_NUM_AXIS_X_N = \)[0-9]*/\15/
s/\(C_VOXEL_NUM_AXIS_Y_N = \)[0-9]*/\15/
s/\(C_VOXEL_NUM_AXIS_Z_N = \)[0-9]*/\15/
s/\(C_MAX_PARTICLE_NUM_PER_VOXEL_N = \)[0-9]*/\13/
s/\(C_VOXEL_SIZE = \)[0-9.]*f/\10.4f/
s/\(g_camera_fx_set = \)[0-9.]*/\1321.13/
s/\(g_camera_fy_set = \)[0-9.]*/\1312.87/
s/\(g_camera_cx_set = \)[0-9.]*/\1210.71/
s/\(g_camera_cy_set = \)[0-9.]*/\1136.29/
s/\(g_image_width_set = \)[0-9]*/\1427/
s/\(g_image_height_set = \)[0-9]*/\1267/
s/\(g_depth_range_max = \)[0-9.]*f/\112.f/
}
s/\(g_image_rescale = \)[0-9.]*f/\10.3f/
