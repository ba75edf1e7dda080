// oracle/ref_shims/opencv2/opencv.hpp - a stand-in for the OpenCV types the reference's translation units name:
// cv::Mat as a single-channel image of float, uchar or uint16_t pixels (a depth image, a MONO8 mask, the track-id
// image of utils/pointcloud_tools.h) and cv::Vec3b (in the colour table of utils/data_base.h).  TEST INFRASTRUCTURE
// ONLY, for oracle/ref_harness.cpp and oracle/ref_cloud_harness.cpp.  No arithmetic happens here.
//
// Copies share the pixels, like cv::Mat's; clone() does not.  Mat(rows, cols[, type]) and zeros() both start at zero
// (OpenCV leaves the former uninitialised).  at<T>() checks the element size and the index and aborts on a miss: a
// stand-in that read out of bounds would record garbage as the reference's answer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

typedef unsigned char uchar;

#define CV_8UC1 0
#define CV_16UC1 2
#define CV_32FC1 5

namespace cv {

struct Vec3b {
  unsigned char val[3];
  Vec3b() : val{0, 0, 0} {}
  Vec3b(unsigned char a, unsigned char b, unsigned char c) : val{a, b, c} {}
};

class Mat {
 public:
  int rows = 0, cols = 0;
  Mat() {}
  Mat(int r, int c, int type = CV_32FC1)
      : rows(r), cols(c), type_(type), d_(std::make_shared<std::vector<unsigned char>>(size_t(r) * c * elem_size(type), 0)) {}
  static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
  Mat clone() const {
    Mat m;
    m.rows = rows, m.cols = cols, m.type_ = type_;
    if (d_) m.d_ = std::make_shared<std::vector<unsigned char>>(*d_);
    return m;
  }
  int type() const { return type_; }
  bool empty() const { return !d_ || rows <= 0 || cols <= 0; }
  template <class T> T &at(int r, int c) const {
    if (!d_ || sizeof(T) != elem_size(type_) || r < 0 || r >= rows || c < 0 || c >= cols) {
      std::fprintf(stderr, "ref_shims/opencv2: at<%zu bytes>(%d, %d) of a %d x %d image of type %d\n", sizeof(T), r, c, rows, cols, type_);
      std::abort();
    }
    return reinterpret_cast<T *>(d_->data())[size_t(r) * cols + c];
  }
 private:
  static size_t elem_size(int type) {
    if (type == CV_8UC1) return 1;
    if (type == CV_16UC1) return 2;
    if (type == CV_32FC1) return 4;
    std::fprintf(stderr, "ref_shims/opencv2: image type %d is not provided\n", type);
    std::abort();
  }
  int type_ = CV_32FC1;
  std::shared_ptr<std::vector<unsigned char>> d_;
};

}  // namespace cv
