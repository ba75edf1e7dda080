# Applied to the build-time copy of the reference's semantic_dsp_map.h (oracle/Makefile, target `ref`): removes, by line
# number, the includes of utils/pointcloud_tools.h, utils/tracking_result_handler.h and utils/object_info_handler.h, the
# members that need PCL or OpenCV (setTemplatePath, update, objectLevelUpdate, subObjectLevelUpdate, getOccupancyResult,
# showSimplePyramidImage), the `private:` line and pt_tools_.  What stays is compiled as it stands: the constructor,
# clear, the setters, the data members, updateParticles (960-1121), the three birth members (1126-1230), getBoundingBox,
# isPointOutOfFOV and resampleParticlesInVoxel (1448-1519).  Addresses only.
15d
17,18d
83,88d
169,251d
254d
259d
302,566d
569,955d
1233,1383d
1522,1570d
