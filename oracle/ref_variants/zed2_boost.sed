# Variant "zed2_boost": settings/settings.h as shipped (SETTING 3: 128 x 32 x 128 voxels of 0.15 m, 4 slots,
# 1280 x 720 halved to 640 x 360).  Nothing is rewritten.
