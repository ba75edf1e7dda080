# Applied to the build-time copy of the reference's utils/pointcloud_tools.h (oracle/Makefile, target `ref`): removes,
# by line number, the includes and the members that need PCL or cv::ml.  What stays is the class head, the constructor,
# the pose setter, lines 88-310 and 1104-1133 as they stand, and the data members those read.  Addresses only.
3d
5,7d
9,10d
31,44d
57,79d
311,467d
478,480d
482,1099d
