// oracle/ref_shims/opencv2/opencv.hpp - a stand-in for the two OpenCV types the reference's ring-buffer translation
// unit names: cv::Mat (as a depth image read with at<float>(row, col)) and cv::Vec3b (in the colour table of
// utils/data_base.h).  TEST INFRASTRUCTURE ONLY, for oracle/ref_harness.cpp.  No arithmetic happens here.
#pragma once
#include <memory>
#include <vector>

namespace cv {

struct Vec3b {
  unsigned char val[3];
  Vec3b() : val{0, 0, 0} {}
  Vec3b(unsigned char a, unsigned char b, unsigned char c) : val{a, b, c} {}
};

// a single-channel float image whose copies share the pixels, like cv::Mat's
class Mat {
 public:
  int rows = 0, cols = 0;
  Mat() {}
  Mat(int r, int c) : rows(r), cols(c), d_(std::make_shared<std::vector<float>>(size_t(r) * c, 0.f)) {}
  template <class T> T &at(int r, int c) const {
    static_assert(sizeof(T) == sizeof(float), "float images only");
    return reinterpret_cast<T &>((*d_)[size_t(r) * cols + c]);
  }
 private:
  std::shared_ptr<std::vector<float>> d_;
};

}  // namespace cv
