// x/vision/types.h -- the input types the update path reads (include/x/vision/types.h:83-198, feature.h:29,
// track.h:32 of the reference): Feature::getX()/getY(), Track (a feature list with a unique id), the window lists,
// the match records the multi-agent updates consume (MsckfMatch / SlamMatch, types.h:83-116), and what the tracker's
// outlier removal reads and writes: TrackedFeature (a Feature with its distorted pixels), FeatureList, Match / MatchList (types.h:39-57).
#pragma once
#include <array>
#include <cstring>
#include <memory>
#include <vector>

namespace x {
struct Attitude { double ax = 0, ay = 0, az = 0, aw = 1; };     // (x,y,z,w)
struct Translation { double tx = 0, ty = 0, tz = 0; };
using AttitudeList = std::vector<Attitude>;
using TranslationList = std::vector<Translation>;

class Feature {
 public:
  Feature() = default;
  Feature(double x, double y) : x_(x), y_(y) {}
  double getX() const { return x_; }   // undistorted image coordinates: normalised on the update path, pixels in the tracker
  double getY() const { return y_; }
  void setX(double x) { x_ = x; }
  void setY(double y) { y_ = y; }
 private:
  double x_ = 0, y_ = 0;               // (nothing else: the update path copies whole tracks as pairs of doubles)
};
// A Feature as the tracker holds it (feature.h:141-146: x_dist_, y_dist_): the distorted pixels as detected beside the undistorted ones.
class TrackedFeature : public Feature {
 public:
  TrackedFeature() = default;
  TrackedFeature(double x, double y, double x_dist, double y_dist) : Feature(x, y), x_dist_(x_dist), y_dist_(y_dist) {}
  double getXDist() const { return x_dist_; }
  double getYDist() const { return y_dist_; }
  void setXDist(double x_dist) { x_dist_ = x_dist; }
  void setYDist(double y_dist) { y_dist_ = y_dist; }
  // what the detection and the tile bookkeeping attach (feature.h: fast_score_, pyramid_level_, tile_row_, tile_col_).  They
  // live here, not in Feature: the update path copies whole tracks as pairs of doubles.
  double getFastScore() const { return fast_score_; }
  void setFastScore(double fast_score) { fast_score_ = fast_score; }
  unsigned int getPyramidLevel() const { return pyramid_level_; }
  void setPyramidLevel(unsigned int pyramid_level) { pyramid_level_ = pyramid_level; }
  int getTileRow() const { return tile_row_; }
  int getTileCol() const { return tile_col_; }
  void setTile(int row, int col) { tile_row_ = row; tile_col_ = col; }
  // the rotated-BRIEF descriptor the description attaches (feature.h: descriptor_, one row of a cv::Mat of CV_8U) and whether
  // there is one.  Here for the same reason: vio_updater.cpp asserts the size of Feature.
  bool hasDescriptor() const { return has_descriptor_; }
  const std::array<unsigned char, 32> &getDescriptor() const { return descriptor_; }
  void setDescriptor(const unsigned char *bytes32) { std::memcpy(descriptor_.data(), bytes32, 32); has_descriptor_ = true; }
  // the box-mean intensity a PHOTOMETRIC_CALI build attaches (feature.h: intensity_; tracker.cpp:461, :666).  fp64 here: the
  // exact integer sum over 255 count
  double getIntensity() const { return intensity_; }
  void setIntensity(double intensity) { intensity_ = intensity; }
 private:
  double x_dist_ = 0, y_dist_ = 0;
  double fast_score_ = 0;
  unsigned int pyramid_level_ = 0;
  int tile_row_ = 0, tile_col_ = 0;
  std::array<unsigned char, 32> descriptor_{};
  bool has_descriptor_ = false;
  double intensity_ = 0;
};
using FeatureList = std::vector<TrackedFeature>;      // the tracker's lists (types.h:49)
struct Match { TrackedFeature previous, current; };   // types.h:39-42, :57
using MatchList = std::vector<Match>;

typedef unsigned long long uniqueId;                  // types.h:81
// Track (track.h:32): a std::vector<Feature> with an id unique across the run (the tracker assigns it).
class Track : public std::vector<Feature> {
 public:
  using std::vector<Feature>::vector;
  Track() = default;
  uniqueId getId() const { return id_; }
  void setId(uniqueId id) { id_ = id; }
 private:
  uniqueId id_ = 0;
};
using TrackList = std::vector<Track>;
using TrackPtr = std::shared_ptr<Track>;

class SimpleState;
// One of this agent's MSCKF tracks also seen by agent `uav_id` (types.h:83-103).
struct MsckfMatch {
  std::shared_ptr<SimpleState> state;
  int uav_id = -1;
  TrackPtr received_track_ptr;
  uniqueId id_current_track = (uniqueId)-1;
  uniqueId id_received_track = (uniqueId)-1;
  MsckfMatch(int uav_id_, uniqueId id_current_track_, uniqueId id_received_track_, TrackPtr received_track,
             std::shared_ptr<SimpleState> state_)
      : state(std::move(state_)), uav_id(uav_id_), received_track_ptr(std::move(received_track)),
        id_current_track(id_current_track_), id_received_track(id_received_track_) {}
};
using MsckfMatches = std::vector<MsckfMatch>;

// One of this agent's persistent features matched to a persistent feature of agent `uav_id` (types.h:105-116).
struct SlamMatch {
  std::shared_ptr<SimpleState> state;
  int uav_id = -1;
  int current_feature_id = -1;     // slot in this agent's feature state
  int received_feature_id = -1;    // slot in the sender's
  SlamMatch(int uav_id_, int current_feature_id_, int received_feature_id_, std::shared_ptr<SimpleState> state_)
      : state(std::move(state_)), uav_id(uav_id_), current_feature_id(current_feature_id_),
        received_feature_id(received_feature_id_) {}
  SlamMatch() = delete;
};
using SlamMatches = std::vector<SlamMatch>;
}  // namespace x
