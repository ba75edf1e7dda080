# Applied to the build-time copy of the reference's object_layer.h (oracle/Makefile, target `ref`): keeps the includes
# and ObjectParticleHashMap (lines 1-52) and removes everything after it - MotionEstimation, ObjectTransformations,
# MJObject and ObjectSet, which need more of Eigen than the stand-in header has.  Addresses only.
53,$d
