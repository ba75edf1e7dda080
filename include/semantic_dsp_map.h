/**
 * semantic_dsp_map.h — the reference's `class SemanticDSPMap` (public API verbatim, reference
 * include/semantic_dsp_map.h:21-251) on top of libsdm_hip (include/sdm.h).
 *
 * Drop-in for the particle-update path only: everything the reference does inside
 * subObjectLevelUpdate (semantic_dsp_map.h:576-955) runs on the MI355X behind sdm_update(); what stays on the
 * host is what the reference also does outside that function:
 *   - track-id reallocation (semantic_dsp_map.h:179-186),
 *   - the object layer (objectLevelUpdate, :306-566): the library's own restatement (sdm_objects.h, SdmBuiltinObjectLayer)
 *     is switched on at the first update() of a preset with consider_instance, like the reference's built-in one;
 *     another implementation (e.g. the reference's ObjectSet) plugs in through SdmObjectLayer / setObjectLayer(),
 *   - packing of the depth image and the MONO8 masks for sdm_update_raw_ex(), which runs generateLabeledPointCloud
 *     (utils/pointcloud_tools.h:88-310) on the device, including the BOOST-mode manualResize and
 *     the ZED2 sky / bounding-box filters (SdmGridPreset::Zed2Boost); the per-object boxes are computed here from the
 *     key points,
 *   - nothing of the output side: occupied / free voxels are compacted, coloured (semantic_dsp_map.h:1274-1351,
 *     including OpenCV's 8-bit RGB <-> HSV round trip and the "V x 0.7" dimming outside the view) and packed as
 *     pcl::PointXYZRGB on the device (sdm_get_occupied_rgb, row N2); update() copies the array into the cloud.
 *
 * Label tables: with SDM_HAVE_REFERENCE_TRACKING_TYPES defined (the node includes the reference's utils/data_base.h
 * first) the class reads g_label_id_map_default, g_label_color_map_default, g_instance_id_to_label_map_default and
 * g_max_movable_object_instance_id at the first update(), i.e. after ObjectInfoHandler::readObjectInfo has filled them
 * from the CSV (src/mapping.cpp:89-93) - an unchanged node needs no extra call.
 *
 * Compile-time grid/camera constants of settings/settings.h become SdmGridPreset.  Like the reference, the class picks
 * its preset from the macros SETTING (0 KITTI_360, 1 CODA, 2 VIRTUAL_KITTI2, 3 ZED2; settings.h:22) and BOOST_MODE
 * (:25-29) when the translation unit defines them - the node still includes the reference's settings/settings.h, or is
 * built with -DSETTING=n [-DBOOST_MODE=b] - and from what the reference ships (SETTING 3, hence BOOST_MODE 1) when it
 * does not: an unchanged node gets the grid it was built for.  setGridPreset() before the first update() overrides it.
 *
 * Needs Eigen3, OpenCV and PCL headers like the reference does.  They are not available in the build image of this
 * repository, where this file is only compile-checked against minimal stand-in headers (tests/mock_includes).
 */
#pragma once

#include <Eigen/Dense>
#include <opencv2/opencv.hpp>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <limits>
#include <map>
#include <set>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "sdm.h"
#include "sdm_objects.h"

// settings/settings.h:22-29: `#define SETTING 3` as shipped, BOOST_MODE 1 for SETTING 3 and 0 otherwise
#ifdef SETTING
#define SDM_SETTING (SETTING)
#else
#define SDM_SETTING 3
#endif
#ifdef BOOST_MODE
#define SDM_BOOST_MODE (BOOST_MODE)
#else
#define SDM_BOOST_MODE ((SDM_SETTING) == 3 ? 1 : 0)
#endif

#ifndef SDM_HAVE_REFERENCE_TRACKING_TYPES
/// utils/data_base.h:25-31
struct BBox2D {
  int x1, y1, x2, y2;
};
/// utils/tracking_result_handler.h:15-26 (the mask_kpts_msgs input format, docs/custom_files.md:16-45)
struct MaskKpts {
  int track_id;
  std::string label;
  std::vector<Eigen::Vector3d> kpts_current;
  std::vector<Eigen::Vector3d> kpts_previous;
  cv::Mat mask;
  BBox2D bbox;
};
#endif

/// settings/settings.h:32-141 as data
struct SdmGridPreset {
  int x_n, y_n, z_n, p_n;
  float voxel_size, fx, fy, cx, cy;
  int width, height;
  float depth_min, depth_max;
  int window_half;
  bool consider_instance;
  /// BOOST_MODE (settings.h:26, 137-143): inputs arrive at src_width x src_height and are reduced by `rescale`
  /// (manualResize); width/height and the intrinsics above are the reduced ones.  src_width = 0: no BOOST mode.
  int src_width = 0, src_height = 0;
  float rescale = 1.f;
  /// SETTING 3 (ZED2): sky pixels are dropped and every movable object's points are clipped to the box of its
  /// current key points +- 1 m (pointcloud_tools.h:174-196, 236-242, 254-272)
  bool zed2_filters = false;
  /// the reference's SETTING for the object layer (settings.h:22): 1 CODA, 2 VIRTUAL_KITTI2, 3 ZED2
  int object_mode = 2;
  static SdmGridPreset Kitti360() { return {8, 8, 8, 3, 0.15f, 552.554261f, 552.554261f, 682.049453f, 238.769549f, 1408, 376, 0.3f, 30.f, 5, false}; }
  static SdmGridPreset Coda() { return {8, 8, 7, 2, 0.15f, 569.8286f, 565.4818f, 439.2660f, 360.5810f, 960, 540, 0.3f, 10.f, 5, true}; }
  static SdmGridPreset VirtualKitti2() { return {8, 7, 8, 3, 0.2f, 725.0087f, 725.0087f, 620.5f, 187.f, 1242, 375, 0.3f, 30.f, 5, true}; }
  /// SETTING 3 with BOOST_MODE 1, the reference's ZED2 configuration (settings.h:24-27, 100-119, 137-143, semantic_dsp_map.h:964-970)
  static SdmGridPreset Zed2Boost() {
    SdmGridPreset p{7, 5, 7, 2, 0.15f, 0.5f * 527.8191528320312f, 0.5f * 527.8191528320312f, 0.5f * 633.9357299804688f,
                    0.5f * 366.3338623046875f, 640, 360, 0.3f, 15.f, 3, true};
    p.src_width = 1280;
    p.src_height = 720;
    p.rescale = 0.5f;
    p.zed2_filters = true;
    p.object_mode = 3;
    return p;
  }
  /// SETTING 3 without BOOST_MODE: the ZED2 grid at the sensor's 1280 x 720 (settings.h:100-119, 128-134), window 5
  static SdmGridPreset Zed2() {
    SdmGridPreset p{7, 5, 7, 2, 0.15f, 527.8191528320312f, 527.8191528320312f, 633.9357299804688f, 366.3338623046875f, 1280, 720, 0.3f, 15.f, 5, true};
    p.zed2_filters = true;
    p.object_mode = 3;
    return p;
  }
  /// BOOST_MODE 1 on top of a full-size preset (settings.h:135-143: image and intrinsics scaled by g_image_rescale = 0.5;
  /// semantic_dsp_map.h:964-970: neighbour half-size 3 instead of 5; pointcloud_tools.h:101, 129, 175: inputs resized)
  static SdmGridPreset Boosted(SdmGridPreset p) {
    const float r = 0.5f;
    p.src_width = p.width;
    p.src_height = p.height;
    p.rescale = r;
    p.fx = r * p.fx;
    p.fy = r * p.fy;
    p.cx = r * p.cx;
    p.cy = r * p.cy;
    p.width = (int)(r * (float)p.width);
    p.height = (int)(r * (float)p.height);
    p.window_half = 3;
    return p;
  }
  /// the preset the reference compiles in for `#define SETTING setting` / `#define BOOST_MODE boost` (settings.h:22-143);
  /// throws std::invalid_argument where the reference has `#error`
  static SdmGridPreset FromSetting(int setting, int boost) {
    SdmGridPreset p;
    switch (setting) {
      case 0: p = Kitti360(); p.object_mode = 2; break;
      case 1: p = Coda(); p.object_mode = 1; break;
      case 2: p = VirtualKitti2(); p.object_mode = 2; break;
      case 3: p = Zed2(); break;
      default: throw std::invalid_argument("SETTING must be 0 (KITTI_360), 1 (CODA), 2 (VIRTUAL_KITTI2) or 3 (ZED2)");
    }
    return boost ? Boosted(p) : p;
  }
};

/// What the particle layer needs from the object layer each frame (semantic_dsp_map.h:588-736).
struct SdmObjectLayer {
  virtual ~SdmObjectLayer() {}
  /// objectLevelUpdate (semantic_dsp_map.h:306-566)
  virtual void update(const std::vector<MaskKpts> &ins_seg_result, const Eigen::Vector3d &camera_position,
                      const Eigen::Quaterniond &camera_orientation, double time_stamp) = 0;
  /// objects to move this frame, in a deterministic order (ascending track id), and objects to wipe
  virtual void collect(uint32_t global_time_stamp, int max_obersevation_lost_time, std::vector<sdm_object_move> &moves,
                       std::vector<int32_t> &remove_tracks) = 0;
  virtual void clear() = 0;
  /// global_time_stamp after the increment at the head of update() (semantic_dsp_map.h:173), told before update()
  virtual void setGlobalTimeStamp(uint32_t) {}
  /// the track ids that own particles in the map right now (sdm_tracks_with_particles: the non-empty keys of the
  /// reference's obj_ptc_hash_map.indices_map, which its floating-object check walks, semantic_dsp_map.h:712-736), told
  /// before collect()
  virtual void setTracksWithParticles(const int32_t *, int32_t) {}
  /// the velocities the layer predicts the moving objects with, for SemanticDSPMap::forecast (sdm.h, "forecast"); a layer
  /// that estimates none reports none
  virtual void motions(std::vector<sdm_motion> &out) { out.clear(); }
};

/// The library's own object layer (sdm_objects.h): objectLevelUpdate and the object loop of the
/// prediction step restated on plain doubles with a seeded RANSAC sampler.  "Floating" objects (tracks that own
/// particles but are not tracked, semantic_dsp_map.h:713-733): the map says which track ids own particles
/// (setTracksWithParticles; SemanticDSPMap::update asks sdm_tracks_with_particles every frame) and those go to
/// sdm_objects_collect as "present".  Driven without a map (nobody tells), it falls back on its own bookkeeping: every
/// movable track id that came with a mask may have particles born under it and counts as present until wiped.
class SdmBuiltinObjectLayer : public SdmObjectLayer {
 public:
  SdmBuiltinObjectLayer(const sdm_objects_config &cfg, const std::unordered_map<std::string, int> &label_ids)
      : h_(nullptr), label_ids_(label_ids), global_time_stamp_(0), max_movable_(cfg.max_movable_instance_id) {
    if (sdm_objects_create(&cfg, &h_) != SDM_OK) throw std::invalid_argument("sdm_objects_create: bad configuration");
  }
  ~SdmBuiltinObjectLayer() override { sdm_objects_destroy(h_); }
  SdmBuiltinObjectLayer(const SdmBuiltinObjectLayer &) = delete;
  SdmBuiltinObjectLayer &operator=(const SdmBuiltinObjectLayer &) = delete;

  void setGlobalTimeStamp(uint32_t t) override { global_time_stamp_ = t; }
  void update(const std::vector<MaskKpts> &ins_seg_result, const Eigen::Vector3d &camera_position,
              const Eigen::Quaterniond &camera_orientation, double time_stamp) override {
    std::vector<sdm_object_observation> obs(ins_seg_result.size());
    std::vector<std::vector<double>> cur(ins_seg_result.size()), prev(ins_seg_result.size());
    seen_this_frame_.clear();
    for (size_t i = 0; i < ins_seg_result.size(); ++i) {
      const MaskKpts &s = ins_seg_result[i];
      for (const Eigen::Vector3d &p : s.kpts_current) cur[i].insert(cur[i].end(), {p.x(), p.y(), p.z()});
      for (const Eigen::Vector3d &p : s.kpts_previous) prev[i].insert(prev[i].end(), {p.x(), p.y(), p.z()});
      auto it = label_ids_.find(s.label);
      obs[i].track_id = s.track_id;
      obs[i].label_id = it == label_ids_.end() ? -1 : it->second;
      obs[i].is_static = s.label == "static";
      obs[i].n_kpts = (int32_t)s.kpts_current.size();
      obs[i].kpts_current = cur[i].empty() ? nullptr : cur[i].data();
      obs[i].kpts_previous = prev[i].size() == cur[i].size() && !prev[i].empty() ? prev[i].data() : nullptr;
      if (!obs[i].is_static && s.track_id <= max_movable_) {
        maybe_present_.insert(s.track_id);
        seen_this_frame_.insert(s.track_id);
      }
    }
    const double pos[3] = {camera_position.x(), camera_position.y(), camera_position.z()};
    const double q[4] = {camera_orientation.w(), camera_orientation.x(), camera_orientation.y(), camera_orientation.z()};
    if (sdm_objects_update(h_, obs.empty() ? nullptr : obs.data(), (int32_t)obs.size(), pos, q, time_stamp, global_time_stamp_) != SDM_OK)
      std::cerr << "sdm_objects_update failed" << std::endl;
  }
  void collect(uint32_t global_time_stamp, int max_obersevation_lost_time, std::vector<sdm_object_move> &moves,
               std::vector<int32_t> &remove_tracks) override {
    int32_t n_tracked = 0;
    sdm_objects_count(h_, &n_tracked);
    const std::vector<int32_t> present = have_owner_tracks_ ? owner_tracks_ : std::vector<int32_t>(maybe_present_.begin(), maybe_present_.end());
    have_owner_tracks_ = false;  // (told anew before every collect)
    const int32_t cap = n_tracked + (int32_t)present.size();
    moves.resize((size_t)cap);
    remove_tracks.resize((size_t)cap);
    int32_t n_moves = 0, n_remove = 0;
    if (sdm_objects_collect(h_, global_time_stamp, max_obersevation_lost_time, present.empty() ? nullptr : present.data(),
                            (int32_t)present.size(), moves.data(), cap, &n_moves, remove_tracks.data(), cap, &n_remove) != SDM_OK) {
      std::cerr << "sdm_objects_collect failed" << std::endl;
      n_moves = n_remove = 0;
    }
    moves.resize((size_t)n_moves);
    remove_tracks.resize((size_t)n_remove);
    // wiped: nothing of it is left in the map - unless it also came with a mask THIS frame: sdm_update applies the
    // removals before this frame's births, so particles are born under the id again right away and it has to be
    // offered as "present" next frame like the reference's obj_ptc_hash_map would (semantic_dsp_map.h:713-736)
    for (int32_t id : remove_tracks)
      if (!seen_this_frame_.count(id)) maybe_present_.erase(id);
  }
  void setTracksWithParticles(const int32_t *ids, int32_t n) override {
    owner_tracks_.assign(ids, ids + (n > 0 ? n : 0));
    have_owner_tracks_ = true;
    told_owner_tracks_ = true;
  }
  /// the frame these removals belonged to was not applied: offer them again
  void requeue(const std::vector<int32_t> &remove_tracks) {
    for (int32_t id : remove_tracks) maybe_present_.insert(id);
  }
  void setBayes(double distance_threshold, double probability_threshold, double increment, double decrement) {
    sdm_objects_set_bayes(h_, distance_threshold, probability_threshold, increment, decrement);
  }
  void clear() override {
    sdm_objects_clear(h_);
    maybe_present_.clear();
    owner_tracks_.clear();
    have_owner_tracks_ = told_owner_tracks_ = false;
  }
  sdm_objects *handle() { return h_; }
  /// Of the tracks that own particles (as last told by the map - also when it told of none -, which collect() leaves in
  /// place; a layer nobody ever told falls back on its own bookkeeping): those the layer tracks,
  /// has seen move and can predict, with the translation velocity it predicts them with (MotionEstimation: identity
  /// rotation, v * dt), ascending track id.
  void motions(std::vector<sdm_motion> &out) override {
    out.clear();
    const std::set<int32_t> present = told_owner_tracks_ ? std::set<int32_t>(owner_tracks_.begin(), owner_tracks_.end()) : maybe_present_;
    for (int32_t id : present) {
      sdm_object_info info;
      if (id < 1 || id > max_movable_ || id > 65535 || sdm_objects_query(h_, id, &info) != SDM_OK) continue;
      if (!info.exists || !info.moving || !info.prediction_available) continue;
      sdm_motion mo;
      mo.track = (uint16_t)id;
      mo.pad = 0;
      for (int a = 0; a < 3; ++a) mo.v[a] = (float)info.translation_velocity[a];
      if (std::isfinite(mo.v[0]) && std::isfinite(mo.v[1]) && std::isfinite(mo.v[2])) out.push_back(mo);
    }
  }

 private:
  sdm_objects *h_;
  std::unordered_map<std::string, int> label_ids_;
  uint32_t global_time_stamp_;
  int max_movable_;
  std::set<int32_t> maybe_present_, seen_this_frame_;
  std::vector<int32_t> owner_tracks_;
  bool have_owner_tracks_ = false;    // told since the last collect()
  bool told_owner_tracks_ = false;    // told ever (since the last clear()): owner_tracks_ is the map's last word
};

/// Where the last update() call spent its wall-clock time (milliseconds); see SemanticDSPMap::lastUpdateTimes().
struct SdmUpdateTimes {
  double objects = 0;  ///< object layer: update, owner-track query (waits for the previous frame), collect
  double pack = 0;     ///< depth image and masks into the staging buffers
  double frame = 0;    ///< sdm_update_raw_ex: uploads, labelled cloud, the frame's launches (returns when the uploads are done)
  double emit = 0;     ///< waiting for the frame + occupied / free-space clouds back to the host
  double total = 0;
};

/// Page-locked host staging for the images handed to sdm_update_raw_ex (sdm_host_alloc): an upload from it is one DMA
/// transfer at PCIe speed; from a std::vector the runtime first copies through bounce buffers of its own.
template <typename T>
class SdmPinnedBuffer {
 public:
  SdmPinnedBuffer() = default;
  SdmPinnedBuffer(const SdmPinnedBuffer &) = delete;
  SdmPinnedBuffer &operator=(const SdmPinnedBuffer &) = delete;
  ~SdmPinnedBuffer() { sdm_host_free(p_); }
  /// n elements, contents undefined after a growth
  void resize(size_t n) {
    if (n > cap_) {
      sdm_host_free(p_);
      p_ = nullptr;
      cap_ = 0;
      void *q = nullptr;
      if (sdm_host_alloc(n * sizeof(T), &q) != SDM_OK) throw std::bad_alloc();
      p_ = static_cast<T *>(q);
      cap_ = n;
    }
    n_ = n;
  }
  size_t size() const { return n_; }
  T *data() { return p_; }
  T &operator[](size_t i) { return p_[i]; }

 private:
  T *p_ = nullptr;
  size_t n_ = 0, cap_ = 0;
};

class SemanticDSPMap {
 public:
  /// semantic_dsp_map.h:25-67
  SemanticDSPMap()
      : map_(nullptr), object_layer_(nullptr), preset_(SdmGridPreset::FromSetting(SDM_SETTING, SDM_BOOST_MODE)), device_(0),
        global_time_stamp_(0), visualize_with_zero_center_(false), if_out_evaluation_format_(false) {
    params_.detection_probability = 0.95f;
    params_.noise_number = 0.1f;
    params_.nb_ptc_num_per_point = 3;
    params_.occupancy_threshold = 0.2f;
    params_.max_obersevation_lost_time = 5;
    params_.forgetting_rate = 1.0f;
    params_.max_forget_count = 5;
    params_.match_score_threshold = 0.3f;
    params_.id_transition_probability = 0.1f;
    params_.if_consider_depth_noise = 0;
    params_.if_use_independent_filter = 0;
    params_.depth_noise_first_order = 0.0f;
    params_.depth_noise_zero_order = 0.1f;
    for (int i = 0; i < 256; ++i) color_map_int_256_.push_back(i);
    // semantic_dsp_map.h:45-48 shuffles with an unseeded generator; a fixed LCG permutation keeps runs reproducible
    uint32_t s = 12345u;
    for (int i = 255; i > 0; --i) {
      s = s * 1664525u + 1013904223u;
      std::swap(color_map_int_256_[i], color_map_int_256_[(s >> 8) % (i + 1)]);
    }
    for (int i = 0; i < 256; ++i) {  // jet map, semantic_dsp_map.h:50-63
      Eigen::Vector3i c;
      if (i < 64) c << 0, 0, i * 4;
      else if (i < 128) c << 0, (i - 64) * 4, 255;
      else if (i < 192) c << (i - 128) * 4, 255, 255 - (i - 128) * 4;
      else c << 255, 255 - (i - 192) * 4, 0;
      color_map_jet_256_.push_back(c);
    }
    defaultLabelTables();
  }
  ~SemanticDSPMap() {
    if (map_) sdm_destroy(map_);
  }
  SemanticDSPMap(const SemanticDSPMap &) = delete;
  SemanticDSPMap &operator=(const SemanticDSPMap &) = delete;

  // ---- additions (the reference fixes these at compile time / inside the class) ----
  void setGridPreset(const SdmGridPreset &p) { preset_ = p; }
  const SdmGridPreset &gridPreset() const { return preset_; }
  void setDevice(int hip_device) { device_ = hip_device; }
  /// The Gaussian table the prediction step and the noisy births draw from (basic_algorithms.h:394-402: 1,000,000 draws
  /// with standard deviation prediction_stddev_ = 0.05, seeded from std::random_device in the reference).  By default the
  /// map fills its own with rocRAND (fixed seed); a caller that needs a particular table - a reproducible run, a parity
  /// test - hands it over before the first update().
  void setNoiseTable(const float *table, size_t n) { noise_table_.assign(table, table + n); }
  void setObjectLayer(SdmObjectLayer *layer) { object_layer_ = layer; }
  /// the built-in object layer, once useBuiltinObjectLayer() or the first update() has made it (else null): its handle
  /// answers sdm_objects_query
  SdmBuiltinObjectLayer *builtinObjectLayer() { return builtin_layer_.get(); }
  /// Use the library's object layer (sdm_objects.h).  mode = the reference's SETTING (settings.h:22); call after
  /// setGridPreset / setLabelTables / setBeyesianMovementParameters.
  void useBuiltinObjectLayer(int mode, uint64_t seed = 20250217ull) {
    sdm_objects_config c;
    c.mode = mode;
    c.max_movable_instance_id = max_movable_track_;
    c.movement_distance_threshold = beyesian_[0];
    c.movement_probability_threshold = beyesian_[1];
    c.movement_increment = beyesian_[2];
    c.movement_decrement = beyesian_[3];
    const int n_biggest = std::max(std::max(preset_.x_n, preset_.y_n), preset_.z_n);
    c.map_half_size_scaled = (double)preset_.voxel_size * (double)(1 << (n_biggest - 1)) * 1.2;  // semantic_dsp_map.h:356
    c.fx = preset_.fx;
    c.fy = preset_.fy;
    c.cx = preset_.cx;
    c.cy = preset_.cy;
    c.image_width = preset_.width;
    c.image_height = preset_.height;
    c.seed = seed;
    builtin_layer_.reset(new SdmBuiltinObjectLayer(c, label_id_));
    object_layer_ = builtin_layer_.get();
  }
  /// label tables of utils/object_info_handler.h:28-91 (CSV): label name -> label id, static label -> instance id
  void setLabelTables(const std::map<std::string, int> &label_ids, const std::map<std::string, int> &static_instance_ids) {
    label_id_.clear();
    static_instance_to_label_.clear();
    for (auto &kv : label_ids) label_id_[kv.first] = kv.second;
    int min_static = 65536;
    for (auto &kv : static_instance_ids) {
      static_instance_to_label_[kv.second] = label_id_[kv.first];
      min_static = std::min(min_static, kv.second);
    }
    const int max_movable = min_static - 1;  // object_info_handler.h:84
    if (map_ && max_movable != max_movable_track_)
      std::cerr << "setLabelTables: g_max_movable_object_instance_id changed after the map was created (" << max_movable_track_
                << " -> " << max_movable << "): the device keeps the value of the first update()" << std::endl;
    max_movable_track_ = max_movable;
    rebuildLabelToInstance();
    pushColours();  // the emitted colours are baked on the device: tables set after the first update() take effect too
  }
  /// g_label_color_map_default (utils/data_base.h:216-232): BGR colour of a label id
  void setLabelColours(const std::map<int, cv::Vec3b> &label_colours) {
    label_color_.clear();
    for (const auto &kv : label_colours) label_color_[kv.first] = kv.second;
    pushColours();
  }
  /// The map by object (sdm.h, "instance table"): builds the table from the results of the last update() and fetches it -
  /// per winning track id its cell count, box, centroid and second moments, ascending track id.  movable_only: only the
  /// tracks 1 .. g_max_movable_object_instance_id, the objects a planner treats apart from the static field.  origin
  /// (3 floats, may be null): the global position of the min corner of map cell (0, 0, 0).  Returns the number of
  /// instances; 0 (and an empty vector) before the first update() or when a call fails.
  size_t instances(std::vector<sdm_instance> &out, bool movable_only = true, float *origin = nullptr) {
    out.clear();
    if (!map_) return 0;
    if (!check(sdm_instances_update(map_, movable_only ? SDM_INSTANCES_MOVABLE_ONLY : 0u), "sdm_instances_update")) return 0;
    int32_t n = 0;
    out.resize(64);
    if (!check(sdm_get_instances(map_, out.data(), (int32_t)out.size(), &n, origin), "sdm_get_instances")) n = 0;
    if ((size_t)n > out.size()) {
      out.resize((size_t)n);
      if (!check(sdm_get_instances(map_, out.data(), (int32_t)out.size(), &n, origin), "sdm_get_instances")) n = 0;
    }
    out.resize((size_t)n);
    return out.size();
  }
  /// Where to explore (sdm.h, "frontiers"): builds the frontiers from the results of the last update() and fetches the
  /// table - per connected cluster (26-connectivity) of free cells that border never-observed space its first cell, cell
  /// count, unknown faces, box and centroid, ascending first cell.  min_cells: clusters with fewer cells are left out.
  /// The cell list takes the library's default capacity (a sixteenth of the map's cells).  origin (3 floats, may be
  /// null): the global position of the min corner of map cell (0, 0, 0).  The table is fetched into the room `out`
  /// already has (64 entries if it has none) and once more if there are more clusters than that.  Returns the number of
  /// clusters; 0 (and an empty vector) before the first update() or when a call fails.
  size_t frontiers(std::vector<sdm_frontier_cluster> &out, int min_cells = 1, float *origin = nullptr) {
    out.clear();
    if (!map_) return 0;
    if (!check(sdm_frontiers_update(map_, 0u, (int32_t)min_cells, 0), "sdm_frontiers_update")) return 0;
    int32_t n = 0;
    out.resize(out.capacity() ? out.capacity() : 64);  // the first guess: what the vector already holds room for
    if (!check(sdm_get_frontier_clusters(map_, out.data(), (int32_t)out.size(), &n, origin), "sdm_get_frontier_clusters")) n = 0;
    if ((size_t)n > out.size()) {
      out.resize((size_t)n);
      if (!check(sdm_get_frontier_clusters(map_, out.data(), (int32_t)out.size(), &n, origin), "sdm_get_frontier_clusters")) n = 0;
    }
    out.resize((size_t)n);
    return out.size();
  }
  /// What would a camera there see (sdm.h, "view scoring")?  Scores candidate poses against the results of the last
  /// update(): per view the distinct unknown, free and occupied cells its rays visit.  The rays are those of this map's
  /// own camera through every stride-th pixel, ((u - cx) / fx, (v - cy) / fy, 1) in float32 for u = 0, stride, ... < width
  /// and v = 0, stride, ... < height, rows first: a view's range is then the planar depth its rays end at, as depth_max
  /// is meant.  The table is built from the preset's intrinsics at the first call and kept until the stride changes.
  /// Returns the number of views scored; 0 (and an empty vector) before the first update() or when the call fails.
  size_t scoreViews(const std::vector<sdm_view> &views, int stride, std::vector<sdm_view_gain> &out) {
    out.clear();
    if (!map_ || views.empty() || stride < 1) return 0;
    const std::vector<float> &rays = viewRays(stride);
    out.resize(views.size());
    if (!check(sdm_query_views(map_, views.data(), (int64_t)views.size(), rays.data(), (int32_t)(rays.size() / 3), out.data(), nullptr,
                               nullptr, 0u),
               "sdm_query_views"))
      out.clear();
    return out.size();
  }
  /// How far is it to get there (sdm.h, "travel cost")?  Builds the travel-cost field from `start` (a global position,
  /// the robot's) over the results of the last update() and answers for every goal position: cost (ten per cell along a
  /// face, 14 and 17 along diagonals, never squeezing between two blocked cells), the same in metres, the goal's cell,
  /// the first step of the way back and a status.  through_unknown: never-observed cells can be crossed as well as free
  /// ones.  max_metres > 0 bounds the search: goals farther than that read "unreachable".  clearance_cells > 0 keeps the
  /// path that many cells away from every obstacle; it needs, and builds, the distance field of the same frame with flags 0 - a field the caller
  /// built before, with whatever flags, is replaced: build it again after this call if it is still wanted.  paths
  /// (may be null): per goal the cell words from the goal to the start, empty where there is no path.  The call waits
  /// for the build.  Returns the number of goals answered; 0 (and an empty vector) before the first update() or when a
  /// call fails.
  size_t reach(const Eigen::Vector3d &start, const std::vector<Eigen::Vector3d> &goals, std::vector<sdm_reach_result> &costs_out,
               bool through_unknown = false, float max_metres = 0.f, int clearance_cells = 0,
               std::vector<std::vector<uint32_t>> *paths = nullptr) {
    costs_out.clear();
    if (paths) paths->clear();
    if (!map_ || goals.empty()) return 0;
    const float s[3] = {(float)start.x(), (float)start.y(), (float)start.z()};
    // (0 would mean "no budget": a positive max_metres below a cost unit asks for one; 4294967040 is the largest float below 2^32)
    const uint32_t budget = max_metres > 0.f ? (uint32_t)std::min(std::max(max_metres / (preset_.voxel_size * 0.1f), 1.f), 4294967040.f) : 0u;
    const uint32_t min_d2 = clearance_cells > 0 ? (uint32_t)clearance_cells * (uint32_t)clearance_cells : 0u;
    if (min_d2 && !check(sdm_esdf_update(map_, 0u), "sdm_esdf_update")) return 0;
    if (!check(sdm_reach_update(map_, s, nullptr, 1, min_d2, budget, through_unknown ? SDM_REACH_THROUGH_UNKNOWN : 0u), "sdm_reach_update"))
      return 0;
    std::vector<float> xyz(3 * goals.size());
    for (size_t i = 0; i < goals.size(); ++i) {
      xyz[3 * i] = (float)goals[i].x();
      xyz[3 * i + 1] = (float)goals[i].y();
      xyz[3 * i + 2] = (float)goals[i].z();
    }
    costs_out.resize(goals.size());
    if (!check(sdm_query_reach(map_, xyz.data(), nullptr, (int64_t)goals.size(), costs_out.data(), 0u), "sdm_query_reach")) {
      costs_out.clear();
      return 0;
    }
    if (paths) {
      uint32_t longest = 0;
      for (const sdm_reach_result &r : costs_out)
        if (r.cost != 0xffffffffu) longest = std::max(longest, r.cost / (uint32_t)SDM_REACH_COST_PER_CELL + 1u);  // a path's longest
      std::vector<uint32_t> rows(goals.size() * (size_t)longest);
      std::vector<int32_t> lens(goals.size());
      if (!check(sdm_reach_paths(map_, xyz.data(), nullptr, (int64_t)goals.size(), (int32_t)longest, rows.empty() ? nullptr : rows.data(),
                                 lens.data(), 0u),
                 "sdm_reach_paths")) {
        costs_out.clear();
        return 0;
      }
      paths->resize(goals.size());
      for (size_t i = 0; i < goals.size(); ++i) (*paths)[i].assign(rows.begin() + i * longest, rows.begin() + i * longest + lens[i]);
    }
    return costs_out.size();
  }
  /// Where will the moving objects be (sdm.h, "forecast")?  Builds the forecast over the results of the last update() from
  /// the velocities the object layer predicts its moving objects with (SdmObjectLayer::motions) at the given horizons -
  /// ascending times in seconds from now, at most SDM_FORECAST_MAX_HORIZONS; swept: a horizon covers the whole interval
  /// since the one before it.  The build is enqueued, the call does not wait.  used (may be null): the motions it was
  /// built from.  Returns 1 when the build is enqueued; 0 before the first update(), without horizons or when the call fails.
  size_t forecast(const std::vector<float> &horizons, bool swept = false, std::vector<sdm_motion> *used = nullptr) {
    std::vector<sdm_motion> mo;
    if (object_layer_) object_layer_->motions(mo);
    if (used) *used = mo;
    return forecast(mo, horizons, swept);
  }
  /// the same from motions of the caller's (one per track id, 1 .. the largest movable id)
  size_t forecast(const std::vector<sdm_motion> &motions, const std::vector<float> &horizons, bool swept = false) {
    if (!map_ || horizons.empty()) return 0;
    return check(sdm_forecast_update(map_, motions.empty() ? nullptr : motions.data(), (int32_t)motions.size(), horizons.data(),
                                     (int32_t)horizons.size(), swept ? SDM_FORECAST_SWEPT : 0u),
                 "sdm_forecast_update")
               ? 1
               : 0;
  }
  /// Is the path still free when the robot gets there?  waypoints: positions (global frame); times: per waypoint when
  /// the robot passes it, in seconds from the forecast's frame and ascending; out[i] answers for the leg from waypoint i
  /// to i + 1: the first cell on it that is occupied while the robot is inside it - by an obstacle that stays or by a
  /// predicted object - or t = -1.  unknown_blocks / vacated_blocks: as the flags of sdm_query_forecast_segments.  Waits.
  /// Returns the number of legs answered; 0 (and an empty vector) before the first update() and forecast(), with fewer
  /// than two waypoints, with not one time per waypoint, or when the call fails.
  size_t checkTrajectory(const std::vector<Eigen::Vector3d> &waypoints, const std::vector<double> &times, std::vector<sdm_forecast_hit> &out,
                         bool unknown_blocks = false, bool vacated_blocks = false) {
    out.clear();
    if (!map_ || waypoints.size() < 2 || times.size() != waypoints.size()) return 0;
    const size_t n = waypoints.size() - 1;
    std::vector<float> seg(8 * n);
    for (size_t i = 0; i < n; ++i)
      for (size_t e = 0; e < 2; ++e) {
        const Eigen::Vector3d &w = waypoints[i + e];
        seg[8 * i + 4 * e] = (float)w.x();
        seg[8 * i + 4 * e + 1] = (float)w.y();
        seg[8 * i + 4 * e + 2] = (float)w.z();
        seg[8 * i + 4 * e + 3] = (float)times[i + e];
      }
    out.resize(n);
    const uint32_t flags = (unknown_blocks ? SDM_QUERY_UNKNOWN_BLOCKS : 0u) | (vacated_blocks ? SDM_FORECAST_VACATED_BLOCKS : 0u);
    if (!check(sdm_query_forecast_segments(map_, seg.data(), (int64_t)n, out.data(), flags), "sdm_query_forecast_segments")) out.clear();
    return out.size();
  }
  /// Where can a ground robot stand (sdm.h, "ground layer")?  Builds the height map, the costmap and its distance
  /// transform over the results of the last update() under `options` (all in cells: the up axis and its sign, the band,
  /// the clearance, the largest step, the labels that carry the robot, flags) and copies them out: one cell and one
  /// squared distance per column, column word i_u + j_v * n_u.  info (may be null): the grid, the counts and the options
  /// echoed.  The call waits.  Returns the number of columns; 0 (and empty vectors) before the first update() or when a
  /// call fails.
  size_t ground(const sdm_ground_options &options, std::vector<sdm_ground_cell> &cells_out, std::vector<uint32_t> &d2_out,
                sdm_ground_info *info = nullptr) {
    cells_out.clear();
    d2_out.clear();
    if (!map_) return 0;
    sdm_ground_info gi;
    if (!check(sdm_ground_update(map_, &options), "sdm_ground_update")) return 0;
    if (!check(sdm_get_ground(map_, nullptr, nullptr, &gi, nullptr), "sdm_get_ground")) return 0;
    cells_out.resize((size_t)gi.n_u * gi.n_v);
    d2_out.resize(cells_out.size());
    if (!check(sdm_get_ground(map_, cells_out.data(), d2_out.data(), nullptr, nullptr), "sdm_get_ground")) {
      cells_out.clear();
      d2_out.clear();
      return 0;
    }
    if (info) *info = gi;
    return cells_out.size();
  }
  /// Does the robot's body fit there?  Every footprint - a rectangle on the ground layer's plane: centre, heading as a unit
  /// vector, half length, half width - against the layer ground() built last: the columns it covers, how many of them are
  /// lethal, unknown ground or ground, the levels under it and the distance to the nearest lethal column.  Waits.  Returns
  /// the number of footprints answered; 0 (and an empty vector) before the first ground() or when the call fails.
  size_t checkFootprints(const std::vector<sdm_footprint> &footprints, std::vector<sdm_footprint_result> &out) {
    return batched(sdm_query_footprints, "sdm_query_footprints", footprints, 1, out);
  }
  /// What does the map look like (sdm.h, "surface mesh")?  Builds the face mesh of the results of the last update() under
  /// `options` - one unit quad per face between a solid cell and a neighbour that is not, the lattice corners as welded
  /// vertices - and copies it out: xyz holds three floats per vertex, triangles three vertex indices per triangle, two
  /// triangles per face in the faces' order ((q0, q1, q2) and (q0, q2, q3), counter-clockwise seen from outside).  faces
  /// (may be null): per face the cell, its track, label and occ, the direction and what lies behind it, for colouring.
  /// info (may be null): the counts and the options echoed, capacities resolved.  A build that needs longer lists than
  /// `options` asks for (0: the library's defaults) is repeated once with the true counts.  The call waits.  Returns the
  /// number of triangles; 0 (and empty vectors) before the first update() or when a call fails.
  size_t mesh(const sdm_mesh_options &options, std::vector<float> &xyz, std::vector<uint32_t> &triangles,
              std::vector<sdm_mesh_face> *faces = nullptr, sdm_mesh_info *info = nullptr) {
    xyz.clear();
    triangles.clear();
    if (faces) faces->clear();
    if (!map_) return 0;
    sdm_mesh_options opt = options;
    sdm_mesh_info mi;
    for (int attempt = 0;; ++attempt) {
      if (!check(sdm_mesh_update(map_, &opt), "sdm_mesh_update")) return 0;
      if (!check(sdm_get_mesh_info(map_, &mi, nullptr), "sdm_get_mesh_info")) return 0;
      if ((int64_t)mi.n_faces <= mi.options.max_faces && (int64_t)mi.n_vertices <= mi.options.max_vertices) break;
      if (attempt == 1) return 0;  // (the counts of one frame do not change between two builds)
      opt.max_faces = std::max<int64_t>(mi.n_faces, 1);
      opt.max_vertices = std::max<int64_t>(mi.n_vertices, 1);
    }
    std::vector<uint32_t> quads(4 * (size_t)mi.n_faces);
    std::vector<sdm_mesh_face> own;
    std::vector<sdm_mesh_face> &fc = faces ? *faces : own;
    if (faces) fc.resize(mi.n_faces);
    xyz.resize(3 * (size_t)mi.n_vertices);
    int64_t n = 0;
    if (!check(sdm_get_mesh_faces(map_, faces ? fc.data() : nullptr, quads.data(), (int64_t)mi.n_faces, &n), "sdm_get_mesh_faces") ||
        !check(sdm_get_mesh_vertices(map_, nullptr, xyz.data(), (int64_t)mi.n_vertices, &n), "sdm_get_mesh_vertices")) {
      xyz.clear();
      if (faces) faces->clear();
      return 0;
    }
    triangles.resize(6 * (size_t)mi.n_faces);
    for (size_t f = 0; f < mi.n_faces; ++f) {
      const uint32_t *q = &quads[4 * f];
      uint32_t *t = &triangles[6 * f];
      t[0] = q[0], t[1] = q[1], t[2] = q[2], t[3] = q[0], t[4] = q[2], t[5] = q[3];
    }
    if (info) *info = mi;
    return 2 * (size_t)mi.n_faces;
  }
  /// What does everything the map remembers look like (sdm.h, "world mesh")?  mesh() over the bricks of the world archive:
  /// builds the face mesh of the archive under `options` (the solid rule, the skip flags, the brick box; caps 0: none) and
  /// copies it out: xyz holds three floats per vertex in the global frame, triangles three vertex indices per triangle, two
  /// triangles per face in the faces' order ((q0, q1, q2) and (q0, q2, q3), counter-clockwise seen from outside).  faces
  /// (may be null): per face its brick's rank, cell, direction, what lies behind it and the cell's track, label and occ,
  /// for colouring; coords (may be null): (bx, by, bz) per brick of the field, which a face's `brick` indexes.  info (may
  /// be null): the counts and the options echoed.  The archive is what is read: call worldUpdate() first.  The call waits.
  /// Returns the number of triangles; 0 (and empty vectors) before the first worldUpdate() or worldImport(), over a cap, or
  /// when a call fails.
  size_t worldMesh(const sdm_world_mesh_options &options, std::vector<float> &xyz, std::vector<uint32_t> &triangles,
                   std::vector<sdm_world_mesh_face> *faces = nullptr, std::vector<int16_t> *coords = nullptr, sdm_world_mesh_info *info = nullptr) {
    xyz.clear();
    triangles.clear();
    if (faces) faces->clear();
    if (coords) coords->clear();
    if (!map_) return 0;
    sdm_world_mesh_info mi;
    if (!check(sdm_world_mesh_update(map_, &options), "sdm_world_mesh_update")) return 0;
    if (!check(sdm_get_world_mesh_info(map_, &mi), "sdm_get_world_mesh_info")) return 0;
    std::vector<uint32_t> quads(4 * (size_t)mi.n_faces);
    if (faces) faces->resize((size_t)mi.n_faces);
    if (coords) coords->resize(3 * (size_t)mi.n_bricks);
    xyz.resize(3 * (size_t)mi.n_vertices);
    int64_t n = 0;
    if (!check(sdm_get_world_mesh_faces(map_, coords ? coords->data() : nullptr, faces ? faces->data() : nullptr, quads.data(), 0, mi.n_faces, &n),
               "sdm_get_world_mesh_faces") ||
        !check(sdm_get_world_mesh_vertices(map_, nullptr, xyz.data(), 0, mi.n_vertices, &n), "sdm_get_world_mesh_vertices")) {
      xyz.clear();
      if (faces) faces->clear();
      if (coords) coords->clear();
      return 0;
    }
    triangles.resize(6 * (size_t)mi.n_faces);
    for (size_t f = 0; f < (size_t)mi.n_faces; ++f) {
      const uint32_t *q = &quads[4 * f];
      uint32_t *t = &triangles[6 * f];
      t[0] = q[0], t[1] = q[1], t[2] = q[2], t[3] = q[0], t[4] = q[2], t[5] = q[3];
    }
    if (info) *info = mi;
    return 2 * (size_t)mi.n_faces;
  }
  /// What did the map know about a place the block has left (sdm.h, "world archive")?  worldUpdate merges the results of
  /// the last update() into the world-fixed archive (flags: SDM_WORLD_STATIC_ONLY, SDM_WORLD_OBSERVED_ONLY; the
  /// library's default capacity); it does not wait.  Call it after every update() whose results are to be remembered.
  /// Returns false before the first update() or when the call fails.
  bool worldUpdate(uint32_t flags = 0) {
    if (!map_) return false;
    sdm_world_options o;
    std::memset(&o, 0, sizeof(o));
    o.flags = flags;
    return check(sdm_world_update(map_, &o), "sdm_world_update");
  }
  /// The archive's counts and brick bounds; zeros before the first worldUpdate().  Waits.
  bool worldInfo(sdm_world_info &info) {
    std::memset(&info, 0, sizeof(info));
    if (!map_) return false;
    return check(sdm_get_world_info(map_, &info), "sdm_get_world_info");
  }
  /// Every archived cell with occ >= 1, the world-wide counterpart of the occupied cloud: min corner, track, label, occ,
  /// ascending in (brick order, cell word).  Waits.  Returns the number of points; 0 (and an empty vector) before the
  /// first worldUpdate() or when a call fails.
  size_t worldOccupied(std::vector<sdm_point> &out) {
    out.clear();
    if (!map_) return 0;
    int64_t n = 0;
    if (!check(sdm_get_world_occupied(map_, nullptr, 0, &n, 0u), "sdm_get_world_occupied")) return 0;
    out.resize((size_t)n);
    if (n && !check(sdm_get_world_occupied(map_, out.data(), n, &n, 0u), "sdm_get_world_occupied")) out.clear();
    return out.size();
  }
  /// What the archive holds at each position (global frame): the cell's track, label and occ and the stamp of the last
  /// update that wrote into its brick; occ -1 where nothing is archived.  Waits.  Returns the number of points answered;
  /// 0 (and an empty vector) before the first worldUpdate() or when the call fails.
  size_t queryWorld(const std::vector<Eigen::Vector3d> &points, std::vector<sdm_world_cell> &out) {
    return batched(sdm_query_world_points, "sdm_query_world_points", flat_points(points), 3, out);
  }
  /// The archive as sdm_get_world_bricks gives it: headers and 512 words per brick, in brick order - what worldImport of this
  /// or of another map takes.  Waits.  Returns the number of bricks; 0 (and empty vectors) before the first worldUpdate() or
  /// worldImport() or when a call fails.
  size_t worldBricks(std::vector<sdm_world_brick> &bricks, std::vector<uint32_t> &cells) {
    bricks.clear();
    cells.clear();
    if (!map_) return 0;
    int64_t n = 0;
    if (!check(sdm_get_world_bricks(map_, nullptr, nullptr, 0, 0, &n), "sdm_get_world_bricks") || !n) return 0;
    bricks.resize((size_t)n);
    cells.resize(512 * (size_t)n);
    if (!check(sdm_get_world_bricks(map_, bricks.data(), cells.data(), 0, n, &n), "sdm_get_world_bricks")) bricks.clear(), cells.clear();
    return bricks.size();
  }
  /// Merges foreign bricks (headers and 512 words each, e.g. another map's worldBricks) into the archive, their world cells
  /// moved by `offset` cells (flags: SDM_WORLD_STATIC_ONLY, SDM_WORLD_OBSERVED_ONLY, SDM_WORLD_IMPORT_FILL; the library's
  /// default capacity).  Waits.  Returns false without a map, when cells does not hold 512 words per brick or when the call
  /// fails.
  bool worldImport(const std::vector<sdm_world_brick> &bricks, const std::vector<uint32_t> &cells, const Eigen::Vector3i &offset = Eigen::Vector3i(0, 0, 0),
                   uint32_t flags = 0) {
    if (!map_ || cells.size() != 512 * bricks.size()) return false;
    sdm_world_import_options o;
    std::memset(&o, 0, sizeof(o));
    o.flags = flags & ~(uint32_t)SDM_WORLD_IMPORT_ON_DEVICE;
    o.cell_offset[0] = offset.x(), o.cell_offset[1] = offset.y(), o.cell_offset[2] = offset.z();
    return check(sdm_world_import(map_, &o, bricks.data(), cells.data(), (int64_t)bricks.size()), "sdm_world_import");
  }
  /// Which whole-cell offset fits?  Scores foreign bricks (as for worldImport) against the archive under every offset
  /// centre + d, |d| <= radius per axis (0 .. SDM_WORLD_MATCH_MAX_RADIUS), and returns the best one in `offset` - what
  /// worldImport takes - with the counts and the runner-up in `result` (may be null) and every candidate's counts in
  /// `scores` (may be null).  Reads the archive, writes nothing.  weights: w_oo, w_same, w_of, w_fo, w_ff; null: 4, 1, -2,
  /// -2, 0, a default that is not tuned on anything.  flags: SDM_WORLD_STATIC_ONLY | SDM_WORLD_OBSERVED_ONLY.  Waits.
  /// Returns false before the first worldUpdate() or worldImport() or when the call fails.
  bool worldMatch(const std::vector<sdm_world_brick> &bricks, const std::vector<uint32_t> &cells, Eigen::Vector3i &offset,
                  const Eigen::Vector3i &centre = Eigen::Vector3i(0, 0, 0), const Eigen::Vector3i &radius = Eigen::Vector3i(2, 2, 1),
                  sdm_world_match_result *result = nullptr, std::vector<sdm_world_match_score> *scores = nullptr, const int32_t *weights = nullptr,
                  uint32_t flags = 0) {
    if (scores) scores->clear();
    if (!map_ || cells.size() != 512 * bricks.size()) return false;
    for (int a = 0; a < 3; ++a)
      if (radius(a) < 0 || radius(a) > SDM_WORLD_MATCH_MAX_RADIUS) return false;
    sdm_world_match_options o;
    std::memset(&o, 0, sizeof(o));
    o.flags = flags & ~(uint32_t)SDM_WORLD_MATCH_ON_DEVICE;
    o.cell_offset[0] = centre.x(), o.cell_offset[1] = centre.y(), o.cell_offset[2] = centre.z();
    o.radius[0] = radius.x(), o.radius[1] = radius.y(), o.radius[2] = radius.z();
    o.w_oo = weights ? weights[0] : 4, o.w_same = weights ? weights[1] : 1, o.w_of = weights ? weights[2] : -2;
    o.w_fo = weights ? weights[3] : -2, o.w_ff = weights ? weights[4] : 0;
    if (scores) scores->resize((size_t)(2 * radius.x() + 1) * (size_t)(2 * radius.y() + 1) * (size_t)(2 * radius.z() + 1));
    sdm_world_match_result r;
    if (!check(sdm_world_match(map_, &o, bricks.data(), cells.data(), (int64_t)bricks.size(), scores ? scores->data() : nullptr, &r), "sdm_world_match")) {
      if (scores) scores->clear();
      return false;
    }
    offset = Eigen::Vector3i(r.best_offset[0], r.best_offset[1], r.best_offset[2]);
    if (result) *result = r;
    return true;
  }
  /// Keeps the archived bricks inside the inclusive brick box bmin .. bmax whose last_stamp >= min_last_stamp and removes
  /// the others.  Waits.  Returns the number of bricks removed; -1 before the first worldUpdate() or worldImport() or when
  /// the call fails.
  int64_t worldRetain(const Eigen::Vector3i &bmin, const Eigen::Vector3i &bmax, uint32_t min_last_stamp = 0) {
    if (!map_) return -1;
    sdm_world_retain_options o;
    std::memset(&o, 0, sizeof(o));
    o.bmin[0] = bmin.x(), o.bmin[1] = bmin.y(), o.bmin[2] = bmin.z();
    o.bmax[0] = bmax.x(), o.bmax[1] = bmax.y(), o.bmax[2] = bmax.z();
    o.min_last_stamp = min_last_stamp;
    int64_t removed = 0;
    return check(sdm_world_retain(map_, &o, &removed), "sdm_world_retain") ? removed : -1;
  }
  /// positions as the batched calls take them: three floats each
  static std::vector<float> flat_points(const std::vector<Eigen::Vector3d> &points) {
    std::vector<float> xyz(3 * points.size());
    for (size_t i = 0; i < points.size(); ++i) {
      xyz[3 * i] = (float)points[i].x();
      xyz[3 * i + 1] = (float)points[i].y();
      xyz[3 * i + 2] = (float)points[i].z();
    }
    return xyz;
  }
  /// How far is it, through everything the map remembers (sdm.h, "world reach")?  Builds the travel-cost field over the
  /// bricks of the world archive from `start` (a global position, the robot's): the moves and weights of reach(), in world
  /// cells, so it reaches what has left the block.  through_unknown: archived cells that were never observed can be crossed
  /// as well as free ones (a cell of no brick never).  max_metres > 0 bounds the search.  inflate_cells (0, 1 or 2) keeps
  /// the path that many cells away from every archived obstacle.  ignore_movable: obstacles on movable tracks count as
  /// free.  The build is a snapshot: queryWorldReach() and worldReachPaths() answer for it until the next worldReach(),
  /// whatever happens to the archive.  The call waits for the build.  info (may be null): the build's counts.  Returns
  /// false before the first worldUpdate() or worldImport() or when the call fails.
  bool worldReach(const Eigen::Vector3d &start, bool through_unknown = false, float max_metres = 0.f, int inflate_cells = 0,
                  bool ignore_movable = false, sdm_world_reach_info *info = nullptr) {
    if (!map_ || inflate_cells < 0) return false;
    const float s[3] = {(float)start.x(), (float)start.y(), (float)start.z()};
    sdm_world_reach_options o;
    std::memset(&o, 0, sizeof(o));
    o.flags = (through_unknown ? SDM_WORLD_REACH_THROUGH_UNKNOWN : 0u) | (ignore_movable ? SDM_WORLD_REACH_IGNORE_MOVABLE : 0u);
    o.inflate = (uint32_t)inflate_cells;
    // (0 would mean "no budget": a positive max_metres below a cost unit asks for one; 4294967040 is the largest float below 2^32)
    o.max_cost = max_metres > 0.f ? (uint32_t)std::min(std::max(max_metres / (preset_.voxel_size * 0.1f), 1.f), 4294967040.f) : 0u;
    if (!check(sdm_world_reach_update(map_, &o, s, nullptr, 1), "sdm_world_reach_update")) return false;
    int64_t n = 0;
    return !info || check(sdm_get_world_reach(map_, nullptr, nullptr, 0, 0, &n, info), "sdm_get_world_reach");
  }
  /// Per goal position (global frame) of the last worldReach(): cost, the same in metres, the goal's world cell, the first
  /// step of the way back and a status.  Waits.  Returns the number of goals answered; 0 (and an empty vector) before the
  /// first worldReach() or when the call fails.
  size_t queryWorldReach(const std::vector<Eigen::Vector3d> &goals, std::vector<sdm_world_reach_result> &out) {
    return batched(sdm_query_world_reach, "sdm_query_world_reach", flat_points(goals), 3, out, nullptr);
  }
  /// Per goal position of the last worldReach() the world cells from the goal to the start, both included; empty where
  /// there is no path.  Waits.  Returns the number of goals answered; 0 (and an empty vector) before the first worldReach()
  /// or when a call fails.
  size_t worldReachPaths(const std::vector<Eigen::Vector3d> &goals, std::vector<std::vector<Eigen::Vector3i>> &paths) {
    return goalPaths(sdm_world_reach_paths, "sdm_world_reach_paths", goals, paths);
  }
  /// Where, beyond the block, is it worth going (sdm.h, "world frontiers")?  Builds the frontier cells of the world archive
  /// - free cells beside never-observed space, bricks the archive does not have included unless inside_bricks - and their
  /// clusters across brick borders (26-connected, 6-connected with face_connected), and returns the table of the clusters
  /// of at least min_cells cells in `out`, ascending in first_index; a cluster's first_cell is a world cell to hand to
  /// sdm_query_world_reach.  The archive is what is read: call worldUpdate() first.  The call waits for the build.  info
  /// (may be null): the build's counts.  Returns false before the first worldUpdate() or worldImport() or when a call fails.
  bool worldFrontiers(std::vector<sdm_world_frontier_cluster> &out, int min_cells = 1, bool face_connected = false, bool inside_bricks = false,
                      sdm_world_frontiers_info *info = nullptr) {
    out.clear();
    if (!map_) return false;
    sdm_world_frontiers_options o;
    std::memset(&o, 0, sizeof(o));
    o.flags = (face_connected ? SDM_WORLD_FRONTIERS_FACE_CONNECTED : 0u) | (inside_bricks ? SDM_WORLD_FRONTIERS_INSIDE_BRICKS : 0u);
    o.min_cells = min_cells;
    if (!check(sdm_world_frontiers_update(map_, &o), "sdm_world_frontiers_update")) return false;
    int32_t n = 0;
    if (!check(sdm_get_world_frontier_clusters(map_, nullptr, 0, &n, info), "sdm_get_world_frontier_clusters")) return false;
    out.resize((size_t)n);
    if (n && !check(sdm_get_world_frontier_clusters(map_, out.data(), n, &n, nullptr), "sdm_get_world_frontier_clusters")) out.clear();
    return (int32_t)out.size() == n;
  }
  /// What things does the map remember out there, where is each and how large (sdm.h, "world objects")?  Builds the
  /// connected components of occupied archived cells that carry the same label, across brick borders (26-connected,
  /// 6-connected with face_connected), of the labels whose bit is set in label_mask (bit l & 31 of word l >> 5), and
  /// returns the table of the objects of at least min_cells cells in `out`, ascending in first_index: count, box, sums and
  /// second moments in world cells, box and centroid in metres; an object's first_cell or centroid is what to hand to
  /// sdm_query_world_reach.  static_only: cells on movable tracks do not count.  The build is a snapshot:
  /// queryWorldObjects() answers for it until the next worldObjects(), whatever happens to the archive.  The archive is what
  /// is read: call worldUpdate() first.  The call waits for the build.  info (may be null): the build's counts.  Returns
  /// false before the first worldUpdate() or worldImport() or when a call fails.
  bool worldObjects(std::vector<sdm_world_object> &out, const uint32_t label_mask[8], int min_cells = 1, bool face_connected = false,
                    bool static_only = false, sdm_world_objects_info *info = nullptr) {
    out.clear();
    if (!map_ || !label_mask) return false;
    sdm_world_objects_options o;
    std::memset(&o, 0, sizeof(o));
    o.flags = (face_connected ? SDM_WORLD_OBJECTS_FACE_CONNECTED : 0u) | (static_only ? SDM_WORLD_OBJECTS_STATIC_ONLY : 0u);
    o.min_cells = min_cells;
    for (int i = 0; i < 8; ++i) o.labels[i] = label_mask[i];
    if (!check(sdm_world_objects_update(map_, &o), "sdm_world_objects_update")) return false;
    int32_t n = 0;
    if (!check(sdm_get_world_objects(map_, nullptr, 0, &n, info), "sdm_get_world_objects")) return false;
    out.resize((size_t)n);
    if (n && !check(sdm_get_world_objects(map_, out.data(), n, &n, nullptr), "sdm_get_world_objects")) out.clear();
    return (int32_t)out.size() == n;
  }
  /// ... of a single label (0 .. 255); a negative label: of every label
  bool worldObjects(std::vector<sdm_world_object> &out, int label, int min_cells = 1, bool face_connected = false, bool static_only = false,
                    sdm_world_objects_info *info = nullptr) {
    uint32_t mask[8];
    for (int i = 0; i < 8; ++i) mask[i] = label < 0 ? 0xffffffffu : 0u;
    if (label > 255) {
      out.clear();
      return false;
    }
    if (label >= 0) mask[label >> 5] = 1u << (label & 31);
    return worldObjects(out, mask, min_cells, face_connected, static_only, info);
  }
  /// Per position (global frame) of the last worldObjects(): its world cell, the index of the object it belongs to in that
  /// call's table - SDM_WORLD_OBJECT_UNLISTED for a cell of an object below min_cells, SDM_WORLD_OBJECT_NONE where nothing
  /// was counted - and its place in the cell list.  Waits.  Returns the number of points answered; 0 (and an empty vector)
  /// before the first worldObjects() or when the call fails.
  size_t queryWorldObjects(const std::vector<Eigen::Vector3d> &points, std::vector<sdm_world_object_result> &out) {
    return batched(sdm_query_world_objects, "sdm_query_world_objects", flat_points(points), 3, out, nullptr);
  }
  /// Is the place the block has come back to still as the map remembers it (sdm.h, "world changes")?  Compares the last
  /// frame's results with the archive cell by cell and returns the table of the regions of changed cells - appeared,
  /// vanished, relabelled - that the options admit, ascending in first_index.  Call it between a frame and its
  /// worldUpdate(), which overwrites what this call finds.  The build is a snapshot: queryWorldChanges() answers for it
  /// until the next worldChanges().  The call waits for the build.  info (may be null): the counters and the build's counts.
  /// Returns false before the first worldUpdate() or worldImport() or when a call fails.
  bool worldChanges(const sdm_world_changes_options &options, std::vector<sdm_world_change_region> &regions, sdm_world_changes_info *info = nullptr) {
    regions.clear();
    if (!map_) return false;
    if (!check(sdm_world_changes_update(map_, &options), "sdm_world_changes_update")) return false;
    int32_t n = 0;
    if (!check(sdm_get_world_changes(map_, nullptr, 0, &n, info), "sdm_get_world_changes")) return false;
    regions.resize((size_t)n);
    if (n && !check(sdm_get_world_changes(map_, regions.data(), n, &n, nullptr), "sdm_get_world_changes")) regions.clear();
    return (int32_t)regions.size() == n;
  }
  /// Per position (global frame) of the last worldChanges(): its world cell, the index of the region it belongs to in that
  /// call's table - SDM_WORLD_CHANGE_UNLISTED for a cell of a region below min_cells, SDM_WORLD_CHANGE_NONE where nothing
  /// changed -, its place in the cell list and its class.  Waits.  Returns the number of points answered; 0 (and an empty
  /// vector) before the first worldChanges() or when the call fails.
  size_t queryWorldChanges(const std::vector<Eigen::Vector3d> &points, std::vector<sdm_world_change_result> &out) {
    return batched(sdm_query_world_changes, "sdm_query_world_changes", flat_points(points), 3, out, nullptr);
  }
  /// How close is a remembered place to an obstacle (sdm.h, "world distance field")?  Builds the truncated Euclidean
  /// distance field over the bricks of the world archive: exact up to max_metres - radius = ceil(max_metres / voxel_size)
  /// cells, at least 1 and at most SDM_WORLD_ESDF_MAX_RADIUS - and "far" beyond.  unknown_is_obstacle: never-observed
  /// cells, and every cell of a brick the archive does not have, are obstacles too; static_only: obstacles on movable tracks
  /// are none.  The build is a snapshot: queryWorldDistance() answers for it until the next worldEsdf(), whatever happens to
  /// the archive.  The archive is what is read: call worldUpdate() first.  info (may be null): the build's counts (the call
  /// then waits for them).  Returns false before the first worldUpdate() or worldImport() or when a call fails.
  bool worldEsdf(float max_metres, bool unknown_is_obstacle = false, bool static_only = false, sdm_world_esdf_info *info = nullptr) {
    if (!map_ || !(max_metres > 0.f)) return false;
    sdm_world_esdf_options o;
    std::memset(&o, 0, sizeof(o));
    o.flags = (unknown_is_obstacle ? SDM_WORLD_ESDF_UNKNOWN_IS_OBSTACLE : 0u) | (static_only ? SDM_WORLD_ESDF_STATIC_ONLY : 0u);
    o.radius = (uint32_t)std::min(std::max(std::ceil(max_metres / preset_.voxel_size), 1.f), (float)SDM_WORLD_ESDF_MAX_RADIUS);
    if (!check(sdm_world_esdf_update(map_, &o), "sdm_world_esdf_update")) return false;
    int64_t n = 0;
    return !info || check(sdm_get_world_esdf(map_, nullptr, nullptr, nullptr, 0, 0, &n, info), "sdm_get_world_esdf");
  }
  /// Per position (global frame) of the last worldEsdf(): its world cell, the world cell of the nearest archived obstacle,
  /// the squared distance in cells and the distance in metres - SDM_WORLD_ESDF_FAR and a lower bound beyond the radius,
  /// 0xffffffff and -1 in no brick of the field.  Waits.  Returns the number of points answered; 0 (and an empty vector)
  /// before the first worldEsdf() or when the call fails.
  size_t queryWorldDistance(const std::vector<Eigen::Vector3d> &points, std::vector<sdm_world_distance_result> &out) {
    return batched(sdm_query_world_distance, "sdm_query_world_distance", flat_points(points), 3, out, nullptr);
  }
  /// Where can a ground robot stand at a place the map only remembers (sdm.h, "world ground layer")?  ground() over the
  /// bricks of the world archive: builds the height map, the costmap and the truncated distance to the nearest lethal
  /// column under `options` (all in world cells: the up axis and its sign, the band, the clearance, the largest step, the
  /// radius, the labels that carry the robot, flags, the tile box) and copies them out: per tile of 8 x 8 columns its
  /// coordinates (bu, bv), 64 cells - level and top relative to options.h_lo - and 64 squared distances
  /// (SDM_WORLD_GROUND_NONE beyond the radius), a column's word cu | cv << 3.  info (may be null): the counts and the
  /// options echoed.  The build is a snapshot: queryWorldGround() and checkWorldFootprints() answer for it until the next
  /// worldGround(), whatever happens to the archive.  The call waits.  Returns the number of tiles; 0 (and empty vectors)
  /// before the first worldUpdate() or worldImport(), for an archive with no brick in the band, or when a call fails
  /// (ok, may be null, tells the last two apart).
  size_t worldGround(const sdm_world_ground_options &options, std::vector<int16_t> &coords_out, std::vector<sdm_ground_cell> &cells_out,
                     std::vector<uint16_t> &d2_out, sdm_world_ground_info *info = nullptr, bool *ok = nullptr) {
    coords_out.clear();
    cells_out.clear();
    d2_out.clear();
    if (ok) *ok = false;
    if (!map_) return 0;
    sdm_world_ground_info gi;
    int64_t n = 0;
    if (!check(sdm_world_ground_update(map_, &options), "sdm_world_ground_update")) return 0;
    if (!check(sdm_get_world_ground(map_, nullptr, nullptr, nullptr, 0, 0, &n, &gi), "sdm_get_world_ground")) return 0;
    coords_out.resize(2 * (size_t)n);
    cells_out.resize(64 * (size_t)n);
    d2_out.resize(64 * (size_t)n);
    if (n && !check(sdm_get_world_ground(map_, coords_out.data(), cells_out.data(), d2_out.data(), 0, n, &n, nullptr), "sdm_get_world_ground")) {
      coords_out.clear();
      cells_out.clear();
      d2_out.clear();
      return 0;
    }
    if (info) *info = gi;
    if (ok) *ok = true;
    return (size_t)n;
  }
  /// Per position (global frame) of the last worldGround(): its column, the column's cell, the squared distance in columns
  /// to the nearest lethal column and that distance in metres (SDM_WORLD_GROUND_FAR and a lower bound beyond the radius),
  /// the height of the position above the level and the world coordinate of the level's surface; status 3, d2 0xffffffff
  /// and dist -1 in no tile.  Waits.  Returns the number of points answered; 0 (and an empty vector) before the first
  /// worldGround() or when the call fails.
  size_t queryWorldGround(const std::vector<Eigen::Vector3d> &points, std::vector<sdm_world_ground_result> &out) {
    return batched(sdm_query_world_ground, "sdm_query_world_ground", flat_points(points), 3, out, nullptr);
  }
  /// Does the robot's body fit at that remembered place?  checkFootprints() against the layer worldGround() built last:
  /// the footprints' centres are world metres along the layer's u and v axes; n_absent counts the covered columns of no
  /// tile.  Waits.  Returns the number of footprints answered; 0 (and an empty vector) before the first worldGround() or
  /// when the call fails.
  size_t checkWorldFootprints(const std::vector<sdm_footprint> &footprints, std::vector<sdm_world_footprint_result> &out) {
    return batched(sdm_query_world_footprints, "sdm_query_world_footprints", footprints, 1, out);
  }
  /// How does a robot on wheels get there, over everything the map remembers (sdm.h, "world ground reach")?  Builds the
  /// 2-D travel-cost field over the costmap worldGround() built last, from `start` (a global position, the robot's: only
  /// its column counts): straight moves weigh 10, diagonal ones 14, a column closer than options.min_d2 to a lethal one
  /// cannot be entered, one closer than options.soft_d2 costs options.penalty more, a move climbs at most
  /// options.max_climb cells.  The build is a snapshot: queryWorldGroundReach() and worldGroundReachPaths() answer for it
  /// until the next worldGroundReach(), whatever happens to the ground layer or the archive.  The call waits for the
  /// build.  info (may be null): the build's counts.  Returns false before the first worldGround() or when a call fails.
  bool worldGroundReach(const Eigen::Vector3d &start, const sdm_world_ground_reach_options &options, sdm_world_ground_reach_info *info = nullptr) {
    if (!map_) return false;
    const float s[3] = {(float)start.x(), (float)start.y(), (float)start.z()};
    if (!check(sdm_world_ground_reach_update(map_, &options, s, nullptr, 1), "sdm_world_ground_reach_update")) return false;
    int64_t n = 0;
    return !info || check(sdm_get_world_ground_reach(map_, nullptr, nullptr, 0, 0, &n, info), "sdm_get_world_ground_reach");
  }
  /// Per goal position (global frame) of the last worldGroundReach(): cost, the same in metres, the goal's column and its
  /// level, the first step of the way back and a status.  Waits.  Returns the number of goals answered; 0 (and an empty
  /// vector) before the first worldGroundReach() or when the call fails.
  size_t queryWorldGroundReach(const std::vector<Eigen::Vector3d> &goals, std::vector<sdm_world_ground_reach_result> &out) {
    return batched(sdm_query_world_ground_reach, "sdm_query_world_ground_reach", flat_points(goals), 3, out, nullptr);
  }
  /// Per goal position of the last worldGroundReach() the world cells the robot's base stands in on the way from the goal
  /// to the start, both included; empty where there is no path.  Waits.  Returns the number of goals answered; 0 (and an
  /// empty vector) before the first worldGroundReach() or when a call fails.
  size_t worldGroundReachPaths(const std::vector<Eigen::Vector3d> &goals, std::vector<std::vector<Eigen::Vector3i>> &paths) {
    return goalPaths(sdm_world_ground_reach_paths, "sdm_world_ground_reach_paths", goals, paths);
  }
  /// Is this straight leg free, through everything the map remembers (sdm.h, "world rays")?  Per segment from[i] -> to[i]
  /// (global frame), walked through the world archive without clipping: where it enters its first blocking cell, that
  /// cell, its word and its brick's stamp, the cells visited and how many of them are unknown - cells of bricks the archive
  /// does not have included.  unknown_blocks: unknown cells block as well as occupied ones; ignore_movable: occupied cells
  /// on movable tracks count as free.  A segment of more than SDM_WORLD_SEGMENT_MAX_CELLS cells reads cells = -1.  Waits.
  /// Returns the number of segments answered; 0 (and an empty vector) before the first worldUpdate() or worldImport(),
  /// for lists of different lengths or when the call fails.
  size_t queryWorldSegments(const std::vector<Eigen::Vector3d> &from, const std::vector<Eigen::Vector3d> &to, std::vector<sdm_world_segment_hit> &out,
                            bool unknown_blocks = false, bool ignore_movable = false) {
    out.clear();
    if (!map_ || from.empty() || from.size() != to.size()) return 0;
    const std::vector<float> a = flat_points(from), b = flat_points(to);
    std::vector<float> ab(6 * from.size());
    for (size_t i = 0; i < from.size(); ++i)
      for (int k = 0; k < 3; ++k) ab[6 * i + k] = a[3 * i + k], ab[6 * i + 3 + k] = b[3 * i + k];
    out.resize(from.size());
    const uint32_t flags = (unknown_blocks ? SDM_QUERY_UNKNOWN_BLOCKS : 0u) | (ignore_movable ? SDM_WORLD_RAYS_IGNORE_MOVABLE : 0u);
    if (!check(sdm_query_world_segments(map_, ab.data(), (int64_t)from.size(), out.data(), flags), "sdm_query_world_segments")) out.clear();
    return out.size();
  }
  /// What would a camera at a remembered place see (sdm.h, "world rays")?  scoreViews() through the world archive instead of
  /// the block: the same views and ray table (every stride-th pixel), every ray bounded by a window of reach_metres round the
  /// view's cell (rounded up to cells, 1 .. SDM_WORLD_VIEW_MAX_REACH) instead of by the block; cells of bricks the archive
  /// does not have count as unknown - they are the gain.  Waits.  Returns the number of views scored; 0 (and an empty
  /// vector) before the first worldUpdate() or worldImport() or when the call fails.
  size_t scoreWorldViews(const std::vector<sdm_view> &views, int stride, float reach_metres, std::vector<sdm_view_gain> &out,
                         bool ignore_movable = false) {
    out.clear();
    if (!map_ || views.empty() || stride < 1 || !(reach_metres > 0.f)) return 0;
    const std::vector<float> &rays = viewRays(stride);
    const int32_t reach = (int32_t)std::min(std::max(std::ceil(reach_metres / preset_.voxel_size), 1.f), (float)SDM_WORLD_VIEW_MAX_REACH);
    out.resize(views.size());
    if (!check(sdm_query_world_views(map_, views.data(), (int64_t)views.size(), rays.data(), (int32_t)(rays.size() / 3), reach, out.data(), nullptr,
                                     ignore_movable ? SDM_WORLD_RAYS_IGNORE_MOVABLE : 0u),
               "sdm_query_world_views"))
      out.clear();
    return out.size();
  }
  /// the ray table scoreViews uses at `stride`: three floats per ray
  const std::vector<float> &viewRays(int stride) {
    if (stride != view_rays_stride_ || view_rays_.empty()) {
      view_rays_.clear();
      for (int v = 0; v < preset_.height; v += stride)
        for (int u = 0; u < preset_.width; u += stride) {
          view_rays_.push_back(((float)u - preset_.cx) / preset_.fx);
          view_rays_.push_back(((float)v - preset_.cy) / preset_.fy);
          view_rays_.push_back(1.f);
        }
      view_rays_stride_ = stride;
    }
    return view_rays_;
  }

  // ---- the reference's public interface ----
  /// semantic_dsp_map.h:74-81
  void clear() {
    if (map_) check(sdm_clear(map_), "sdm_clear");
    if (object_layer_) object_layer_->clear();
    global_time_stamp_ = 0;
  }
  /// semantic_dsp_map.h:85-88 (template matching is dead code in the shipped node)
  void setTemplatePath(std::string) {}
  /// semantic_dsp_map.h:101-115
  void setMapParameters(float detection_probability, float noise_number, int nb_ptc_num_per_point, float occupancy_threshold,
                        int max_obersevation_lost_time, float forgetting_rate = 1.f, int max_forget_count = 5,
                        float match_score_threshold = 0.5, float id_transition_probability = 0.1) {
    params_.detection_probability = detection_probability;
    params_.noise_number = noise_number;
    params_.nb_ptc_num_per_point = nb_ptc_num_per_point;
    params_.occupancy_threshold = occupancy_threshold;
    params_.max_obersevation_lost_time = max_obersevation_lost_time;
    params_.forgetting_rate = forgetting_rate;
    params_.max_forget_count = max_forget_count;
    params_.match_score_threshold = match_score_threshold;
    params_.id_transition_probability = id_transition_probability;
    std::cout << "max_obersevation_lost_time_ = " << max_obersevation_lost_time << std::endl;
    std::cout << "id_transition_probability_ = " << id_transition_probability << std::endl;
    pushParams();
  }
  /// semantic_dsp_map.h:121-125
  void setMapOptions(bool if_consider_depth_noise, bool if_use_independent_filter) {
    params_.if_consider_depth_noise = if_consider_depth_noise ? 1 : 0;
    params_.if_use_independent_filter = if_use_independent_filter ? 1 : 0;
    pushParams();
  }
  /// semantic_dsp_map.h:130-134
  void setVisualizeOptions(bool visualize_with_zero_center, bool if_out_evaluation_format) {
    visualize_with_zero_center_ = visualize_with_zero_center;
    if_out_evaluation_format_ = if_out_evaluation_format;
    pushColours();
  }
  /// semantic_dsp_map.h:142-148 (consumed by the object layer)
  void setBeyesianMovementParameters(double distance_threshold, double probability_threshold, double increment, double decrement) {
    beyesian_[0] = distance_threshold;
    beyesian_[1] = probability_threshold;
    beyesian_[2] = increment;
    beyesian_[3] = decrement;
    if (builtin_layer_) builtin_layer_->setBayes(distance_threshold, probability_threshold, increment, decrement);
  }
  const double *beyesianMovementParameters() const { return beyesian_; }
  /// semantic_dsp_map.h:153-156
  void setOccupancyThreshold(float threshold) {
    params_.occupancy_threshold = threshold;
    pushParams();
  }
  /// semantic_dsp_map.h:161-166
  void setDepthNoiseModelParameters(float first_order, float zero_order) {
    params_.depth_noise_first_order = first_order;
    params_.depth_noise_zero_order = zero_order;
    std::cout << "Noise model is " << first_order << " * distance + " << zero_order << std::endl;
    pushParams();
  }

  /// semantic_dsp_map.h:170-251.  Like the reference: no return code, diagnostics on stderr, output clouds are
  /// appended to and neither cleared nor given width/height.
  void update(cv::Mat &depth_value_mat, std::vector<MaskKpts> &ins_seg_result, Eigen::Vector3d &camera_position,
              Eigen::Quaterniond &camera_orientation, pcl::PointCloud<pcl::PointXYZRGB>::Ptr &occupied_point_cloud,
              pcl::PointCloud<pcl::PointXYZRGB>::Ptr &freespace_point_cloud, bool if_get_freespace = false,
              double time_stamp_double = 0.0) {
    using clock = std::chrono::steady_clock;
    const auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
    const clock::time_point t_begin = clock::now();
    times_ = SdmUpdateTimes();
    ensureMap();
    if (preset_.consider_instance && !object_layer_) useBuiltinObjectLayer(preset_.object_mode);  // like the reference's built-in one
    global_time_stamp_ += 1;
    for (size_t i = 0; i < ins_seg_result.size(); ++i) {  // :179-186
      if (ins_seg_result[i].label != "static" && ins_seg_result[i].track_id > max_movable_track_) {
        std::cout << "Reach the maximum movable object instance id. ID reallocated." << std::endl;
        ins_seg_result[i].track_id = ins_seg_result[i].track_id % max_movable_track_;
      }
    }
    std::vector<sdm_object_move> moves;
    std::vector<int32_t> removals;
    if (preset_.consider_instance && object_layer_) {  // :189-191
      object_layer_->setGlobalTimeStamp(global_time_stamp_);
      object_layer_->update(ins_seg_result, camera_position, camera_orientation, time_stamp_double);
      {  // the keys of the owner sets as the previous frame left them (semantic_dsp_map.h:712-736 walks them here)
        int32_t n_own = 0;
        if (owner_tracks_.size() < 64) owner_tracks_.resize(64);
        if (check(sdm_tracks_with_particles(map_, owner_tracks_.data(), (int32_t)owner_tracks_.size(), &n_own), "sdm_tracks_with_particles")) {
          if ((size_t)n_own > owner_tracks_.size()) {
            owner_tracks_.resize((size_t)n_own);
            check(sdm_tracks_with_particles(map_, owner_tracks_.data(), (int32_t)owner_tracks_.size(), &n_own), "sdm_tracks_with_particles");
          }
          object_layer_->setTracksWithParticles(owner_tracks_.data(), n_own);
        }
      }
      object_layer_->collect(global_time_stamp_, params_.max_obersevation_lost_time, moves, removals);
    }
    // (the lists go to the library whole: it works lists longer than SDM_MAX_MOVES / SDM_MAX_REMOVALS off in batches inside
    // the frame, with the reference's order - semantic_dsp_map.h:588-736 loops over whatever the object layer hands it)
    removals.insert(removals.begin(), pending_removals_.begin(), pending_removals_.end());
    pending_removals_.clear();
    times_.objects = ms_since(t_begin);
    clock::time_point t_phase = clock::now();
    if (packRawInputs(depth_value_mat, ins_seg_result) != 0) {
      frameLost(removals);
      return;
    }
    times_.pack = ms_since(t_phase);
    t_phase = clock::now();

    // pose in double for the back-projection (pointcloud_tools.h:243-247); the library casts it to float for the
    // map update like the reference does (semantic_dsp_map.h:584, 745)
    const double cam_pos_d[3] = {camera_position.x(), camera_position.y(), camera_position.z()};
    const double cam_q_d[4] = {camera_orientation.w(), camera_orientation.x(), camera_orientation.y(), camera_orientation.z()};
    sdm_raw_options opt;
    opt.src_width = preset_.src_width;
    opt.src_height = preset_.src_height;
    opt.rescale = preset_.rescale;
    opt.sky_instance = -1;
    if (preset_.zed2_filters && label_id_.count("Sky")) {  // g_label_to_instance_id_map_default["Sky"]
      const int sky_label = label_id_["Sky"];
      if (sky_label >= 0 && sky_label < 256) opt.sky_instance = label_to_inst_[sky_label];
    }
    static const double no_boxes[6] = {0, 0, 0, 0, 0, 0};  // (a frame without objects keeps the filter on, :254-272)
    opt.object_bbox = preset_.zed2_filters ? (boxes_.empty() ? no_boxes : boxes_.data()) : nullptr;
    if (!check(sdm_update_raw_ex(map_, depth_.data(), have_static_ ? static_mask_.data() : nullptr, label_to_inst_,
                                 objects_.empty() ? nullptr : objects_.data(), (int32_t)objects_.size(), cam_pos_d, cam_q_d,
                                 moves.empty() ? nullptr : moves.data(), (int32_t)moves.size(),
                                 removals.empty() ? nullptr : removals.data(), (int32_t)removals.size(),
                                 preset_.consider_instance ? 0u : SDM_NO_INSTANCES, SDM_STAGE_ALL, &opt),
               "sdm_update_raw_ex")) {
      frameLost(removals);
      return;
    }
    times_.frame = ms_since(t_phase);
    t_phase = clock::now();
    emit(occupied_point_cloud, false);
    if (if_get_freespace) emit(freespace_point_cloud, true);
    // the getters above waited for the frame: surface what the device flagged (work-list overflows are recorded in
    // counters that the next frame resets)
    check(sdm_synchronize(map_), "sdm_update (device status)");
    times_.emit = ms_since(t_phase);
    times_.total = ms_since(t_begin);
  }

  sdm_map *handle() { return map_; }
  /// not in the reference: the phases of the last update() call
  const SdmUpdateTimes &lastUpdateTimes() const { return times_; }

 private:
  sdm_map *map_;
  SdmObjectLayer *object_layer_;
  std::unique_ptr<SdmBuiltinObjectLayer> builtin_layer_;
  SdmGridPreset preset_;
  sdm_params params_;
  int device_;
  uint32_t global_time_stamp_;
  bool visualize_with_zero_center_, if_out_evaluation_format_;
  double beyesian_[4] = {0.1, 0.69, 0.1, 0.15};
  int max_movable_track_ = 65523;  // utils/data_base.h:196
  std::vector<int> color_map_int_256_;
  std::vector<Eigen::Vector3i> color_map_jet_256_;
  std::unordered_map<std::string, int> label_id_;          // g_label_id_map_default
  std::unordered_map<int, int> static_instance_to_label_;   // g_instance_id_to_label_map_default -> label id
  std::unordered_map<int, cv::Vec3b> label_color_;          // g_label_color_map_default (BGR)
  SdmPinnedBuffer<float> depth_;
  SdmPinnedBuffer<uint8_t> static_mask_, object_masks_;
  std::vector<sdm_instance_mask> objects_;
  std::vector<double> boxes_;  // ZED2: per object min x, max x, min y, max y, min z, max z
  uint16_t label_to_inst_[256];  // g_label_to_instance_id_map_default as a table (65535 = Background's instance)
  bool have_static_ = false;
  std::vector<sdm_point_xyzrgb> points_;
  std::vector<int32_t> pending_removals_;
  std::vector<int32_t> owner_tracks_;
  std::vector<float> noise_table_;
  SdmUpdateTimes times_;
  bool tables_from_reference_ = false;
  std::vector<float> view_rays_;  // scoreViews' ray table at view_rays_stride_
  int view_rays_stride_ = 0;

  /// a frame that did not reach the map: its removals are offered again
  void frameLost(const std::vector<int32_t> &removals) {
    if (builtin_layer_) builtin_layer_->requeue(removals);
    else pending_removals_.insert(pending_removals_.end(), removals.begin(), removals.end());
  }
  /// colour tables + output format -> device (row N2)
  void pushColours() {
    if (!map_) return;
    sdm_colour_config c;
    std::memset(&c, 0, sizeof(c));
    for (const auto &kv : label_color_)
      if (kv.first >= 0 && kv.first < 256)
        for (int k = 0; k < 3; ++k) c.label_bgr[kv.first][k] = kv.second[k];
    for (int i = 0; i < 256; ++i) c.perm[i] = (uint8_t)color_map_int_256_[i];
    c.background_label = label_id_.count("Background") ? label_id_["Background"] : 0;
    c.colour_by_label = preset_.consider_instance ? 0 : 1;  // SETTING == 0 (semantic_dsp_map.h:1296-1302)
    c.jet_axis = preset_.zed2_filters ? 1 : 0;              // SETTING == 3 colours by y (:1281-1286)
    c.evaluation_format = if_out_evaluation_format_ ? 1 : 0;
    check(sdm_set_colours(map_, &c), "sdm_set_colours");
  }

  bool check(sdm_status s, const char *what) {
    if (s == SDM_OK) return true;
    std::cerr << what << " failed: " << sdm_last_error() << std::endl;  // the reference reports on stdout/stderr and carries on
    return false;
  }
  /// The batched queries' one body: sizes `out` to the entries of `in` (`per` values each: flat_points' three floats, or
  /// one record), calls `query` - `what` by name -, and clears `out` if the call fails -> the number of entries answered.
  /// cells: the null `cells` argument, for the entry points that take their entries as positions or as cells.  (A caller
  /// that hands in flat_points(...) has flattened its points before the map is looked at: one copy more on a map that was
  /// never made, the same return value.)
  template <class Query, class In, class Out, class... Cells>
  size_t batched(Query query, const char *what, const std::vector<In> &in, size_t per, std::vector<Out> &out, Cells... cells) {
    out.clear();
    if (!map_ || in.empty()) return 0;
    out.resize(in.size() / per);
    if (!check(query(map_, in.data(), cells..., (int64_t)out.size(), out.data(), 0u), what)) out.clear();
    return out.size();
  }
  /// The world layers' paths: the true lengths first (whatever max_len), then the rows at the longest of them, unpacked into
  /// one list of world cells per goal -> the number of goals answered
  template <class Paths>
  size_t goalPaths(Paths query, const char *what, const std::vector<Eigen::Vector3d> &goals, std::vector<std::vector<Eigen::Vector3i>> &paths) {
    paths.clear();
    if (!map_ || goals.empty()) return 0;
    const std::vector<float> xyz = flat_points(goals);
    std::vector<int32_t> lens(goals.size());
    if (!check(query(map_, xyz.data(), nullptr, (int64_t)goals.size(), 0, nullptr, lens.data(), 0u), what)) return 0;
    const int32_t longest = *std::max_element(lens.begin(), lens.end());
    std::vector<int32_t> rows(goals.size() * (size_t)longest * 3);
    if (longest && !check(query(map_, xyz.data(), nullptr, (int64_t)goals.size(), longest, rows.data(), lens.data(), 0u), what)) return 0;
    paths.resize(goals.size());
    for (size_t i = 0; i < goals.size(); ++i)
      for (int32_t k = 0; k < lens[i]; ++k) {
        const int32_t *c = rows.data() + (i * (size_t)longest + (size_t)k) * 3;
        paths[i].push_back(Eigen::Vector3i(c[0], c[1], c[2]));
      }
    return paths.size();
  }
  void pushParams() {
    if (map_) check(sdm_set_params(map_, &params_), "sdm_set_params");
  }
  void ensureMap() {
    if (map_) return;
#ifdef SDM_HAVE_REFERENCE_TRACKING_TYPES
    // the reference's label globals (utils/data_base.h:108-232), as ObjectInfoHandler::readObjectInfo left them
    // (utils/object_info_handler.h:76-87, called at src/mapping.cpp:89-93 before the first frame)
    if (!tables_from_reference_) {
      label_id_.clear();
      static_instance_to_label_.clear();
      label_color_.clear();
      for (const auto &kv : g_label_id_map_default) label_id_[kv.first] = kv.second;
      for (const auto &kv : g_instance_id_to_label_map_default)
        if (label_id_.count(kv.second)) static_instance_to_label_[kv.first] = label_id_[kv.second];
      for (const auto &kv : g_label_color_map_default) label_color_[kv.first] = kv.second;
      max_movable_track_ = g_max_movable_object_instance_id;
      rebuildLabelToInstance();
      tables_from_reference_ = true;
    }
#endif
    sdm_config c{};
    c.x_n = preset_.x_n;
    c.y_n = preset_.y_n;
    c.z_n = preset_.z_n;
    c.p_n = preset_.p_n;
    c.voxel_size = preset_.voxel_size;
    c.fx = preset_.fx;
    c.fy = preset_.fy;
    c.cx = preset_.cx;
    c.cy = preset_.cy;
    c.width = preset_.width;
    c.height = preset_.height;
    c.depth_min = preset_.depth_min;
    c.depth_max = preset_.depth_max;
    c.window_half = preset_.window_half;
    c.max_movable_track = max_movable_track_;
    c.device = device_;
    c.shard_rank = 0;
    c.shard_count = 1;
    if (sdm_create(&c, &map_) != SDM_OK) throw std::runtime_error(std::string("sdm_create: ") + sdm_last_error());
    // prediction_stddev_ = 0.05 table of 1,000,000 draws (semantic_dsp_map.h:40,66; basic_algorithms.h:394-402)
    if (noise_table_.empty()) check(sdm_generate_noise_table(map_, 20250217ull, 1000000, 0.05f), "sdm_generate_noise_table");
    else check(sdm_upload_noise_table(map_, noise_table_.data(), (int32_t)noise_table_.size()), "sdm_upload_noise_table");
    pushParams();
    pushColours();
    depth_.resize((size_t)c.width * c.height);
    static_mask_.resize((size_t)c.width * c.height);
  }
  void rebuildLabelToInstance() {
    for (int l = 0; l < 256; ++l) label_to_inst_[l] = 65535;
    for (const auto &kv : static_instance_to_label_)
      if (kv.second >= 0 && kv.second < 256) label_to_inst_[kv.second] = (uint16_t)kv.first;
  }

  void defaultLabelTables() {  // utils/data_base.h:108-232
    const char *names[] = {"Background", "Terrain", "Sky", "Tree", "Vegetation", "Building", "Road", "GuardRail",
                           "TrafficSign", "TrafficLight", "Pole", "Misc", "Truck", "Car", "Person"};
    const int ids[] = {0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    for (int i = 0; i < 15; ++i) label_id_[names[i]] = ids[i];
    for (int i = 0; i < 12; ++i) static_instance_to_label_[65535 - i] = ids[i];
    const int bgr[15][4] = {{0, 0, 0, 0},      {2, 200, 0, 210},  {3, 255, 200, 90}, {4, 0, 199, 0},    {5, 0, 240, 90},
                            {6, 140, 140, 140}, {7, 100, 60, 100}, {8, 255, 100, 250}, {9, 0, 255, 255},  {10, 0, 200, 200},
                            {11, 0, 130, 255},  {12, 80, 80, 80},  {13, 60, 60, 160},  {14, 80, 127, 255}, {15, 139, 139, 0}};
    for (auto &c : bgr) label_color_[c[0]] = cv::Vec3b((uchar)c[1], (uchar)c[2], (uchar)c[3]);
    max_movable_track_ = 65523;
    rebuildLabelToInstance();
  }

  /// Host half of PointCloudTools::generateLabeledPointCloud (utils/pointcloud_tools.h:88-213): validate the depth
  /// image and lay the MONO8 masks out as dense H x W buffers; the per-pixel work (:218-304) is the device kernel
  /// behind sdm_update_raw.
  /// one MONO8 mask into a W x H staging image; what the mask does not cover is set to `fill`
  static void copyMask(const cv::Mat &mask, uint8_t *dst, int W, int H, int fill) {
    const int rows = std::max(std::min(mask.rows, H), 0), cols = std::max(std::min(mask.cols, W), 0);
    for (int j = 0; j < rows; ++j) {
      std::memcpy(dst + (size_t)j * W, mask.ptr<uchar>(j), (size_t)cols);
      if (cols < W) std::memset(dst + (size_t)j * W + cols, fill, (size_t)(W - cols));
    }
    if (rows < H) std::memset(dst + (size_t)rows * W, fill, (size_t)(H - rows) * W);
  }
  int packRawInputs(const cv::Mat &depth, const std::vector<MaskKpts> &seg) {
    if (depth.empty()) {
      std::cerr << "Error: depth image is empty." << std::endl;
      return -1;
    }
    // BOOST mode: the images keep the sensor's size here, the library reduces them (manualResize) on the device
    const int W = preset_.src_width > 0 ? preset_.src_width : preset_.width;
    const int H = preset_.src_width > 0 ? preset_.src_height : preset_.height;
    if (depth.cols != W || depth.rows != H) {
      std::cerr << "Error: depth image size does not match the grid preset." << std::endl;
      return -1;
    }
    const size_t hw = (size_t)W * H;
    if (depth_.size() != hw) {
      depth_.resize(hw);
      static_mask_.resize(hw);
    }
    for (int i = 0; i < H; ++i) std::memcpy(&depth_[(size_t)i * W], depth.ptr<float>(i), (size_t)W * sizeof(float));  // (row by row: a cv::Mat need not be continuous)
    have_static_ = false;
    for (const auto &s : seg) {  // :121-143, the first "static" entry
      if (s.label != "static") continue;
      // uncovered pixels: no label -> Background's instance
      copyMask(s.mask, static_mask_.data(), W, H, 255);
      have_static_ = true;
      break;
    }
    objects_.clear();
    boxes_.clear();
    size_t n_obj = 0;
    if (preset_.consider_instance)
      for (const auto &s : seg) n_obj += s.label != "static";
    object_masks_.resize(n_obj * hw);
    if (preset_.consider_instance) {  // :163-213, later masks override earlier ones
      size_t k_obj = 0;
      for (const auto &s : seg) {
        if (s.label == "static") continue;
        uint8_t *dst = object_masks_.data() + k_obj * hw;
        copyMask(s.mask, dst, W, H, 0);
        auto it = label_id_.find(s.label);
        sdm_instance_mask o;
        o.track_id = s.track_id;
        o.label_id = it == label_id_.end() ? 0 : it->second;
        o.mask = dst;
        objects_.push_back(o);
        if (preset_.zed2_filters) {  // pointcloud_tools.h:174-196 (max starts at the smallest positive double there)
          double lo[3] = {std::numeric_limits<double>::max(), std::numeric_limits<double>::max(), std::numeric_limits<double>::max()};
          double hi[3] = {std::numeric_limits<double>::min(), std::numeric_limits<double>::min(), std::numeric_limits<double>::min()};
          for (const auto &kpt : s.kpts_current)
            for (int a = 0; a < 3; ++a) {
              if (kpt(a) < lo[a]) lo[a] = kpt(a);
              if (kpt(a) > hi[a]) hi[a] = kpt(a);
            }
          const double margin = 1.0;
          for (int a = 0; a < 3; ++a) {
            boxes_.push_back(lo[a] - margin);
            boxes_.push_back(hi[a] + margin);
          }
        }
        ++k_obj;
      }
    }
    return 0;
  }

  /// getOccupancyResult output side (semantic_dsp_map.h:1258-1376): compacted, coloured and packed as pcl::PointXYZRGB
  /// on the device; appended to the cloud as they come (the reference appends too).
  void emit(pcl::PointCloud<pcl::PointXYZRGB>::Ptr &out, bool free_space) {
    static_assert(sizeof(pcl::PointXYZRGB) == sizeof(sdm_point_xyzrgb), "sdm_point_xyzrgb is pcl::PointXYZRGB's layout");
    size_t n = 0;
    const size_t cap = (size_t)1 << (preset_.x_n + preset_.y_n + preset_.z_n);
    if (points_.size() < 1024) points_.resize(1024);
    auto get = free_space ? sdm_get_freespace_rgb : sdm_get_occupied_rgb;
    const int32_t flags = visualize_with_zero_center_ ? SDM_POINTS_ZERO_CENTER : 0;
    if (!check(get(map_, points_.data(), points_.size(), &n, flags), "sdm_get_occupied_rgb")) return;
    if (n > points_.size()) {  // (with headroom: a map that grows a little every frame would come here every frame)
      points_.resize(std::min(n + n / 2 + 1024, cap));
      if (!check(get(map_, points_.data(), points_.size(), &n, flags), "sdm_get_occupied_rgb")) return;
    }
    n = std::min(n, points_.size());
    const size_t first_new = out->points.size();
    out->points.resize(first_new + n);
    if (n) std::memcpy(static_cast<void *>(&out->points[first_new]), points_.data(), n * sizeof(sdm_point_xyzrgb));
  }
};
