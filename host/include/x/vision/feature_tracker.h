// x/vision/feature_tracker.h -- Tracker::featureTracking (src/x/vision/tracker.cpp:623-690) on the mirror:
// cv::calcOpticalFlowPyrLK(previous image, current image, pts1, pts2, status, err, win_size_, max_level_, term_crit_,
// cv::OPTFLOW_LK_GET_MIN_EIGENVALS, min_eig_thr_) on the previous features' distorted pixels, then the pairs that were tracked
// and stayed inside the frame.  All of it runs on the GPU behind xk_trk_push_image / xk_trk_track (include/xk.h); the lists it
// returns are what x::MatchFilter::filter takes.  There is no CPU fallback.
// Tracker::featureDetection (tracker.cpp:390-590) -- cv::FAST, the border, the sort by score and the selection outside the old
// features' neighbourhoods -- runs on the GPU too, behind xk_trk_detect.  The tile bookkeeping around it,
// TiledImage::setTileForFeature (tiled_image.cpp:139-158) and Tracker::removeOverflowFeatures (tracker.cpp:592-620), is host
// code here as it is there: list walks over a few hundred items.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "x/vision/camera.h"
#include "xk.h"

namespace x {
// The tile parameters and counts of a TiledImage (tiled_image.cpp:98-158).
class TileGrid {
 public:
  TileGrid(unsigned int width, unsigned int height, unsigned int n_tiles_h, unsigned int n_tiles_w, unsigned int max_feat_per_tile);
  // TiledImage::setTileForFeature: the fp64 subtraction loops as written there
  void setTileForFeature(TrackedFeature &feature) const;
  void resetFeatureCounts();
  void incrementFeatureCountAtTile(int row, int col);          // (a tile outside the grid is not counted)
  unsigned int getFeatureCountAtTile(int row, int col) const;  // (0 outside the grid)
  unsigned int getMaxFeatPerTile() const { return max_feat_per_tile_; }
  double getTileHeight() const { return tile_height_; }
  double getTileWidth() const { return tile_width_; }

 private:
  unsigned int rows_, n_tiles_h_, n_tiles_w_, max_feat_per_tile_;
  double tile_height_, tile_width_;
  std::vector<unsigned int> tiles_;
};

class FeatureTracker {
 public:
  // the image size is the camera's; the other defaults are the reference's (tracker.h:234-261)
  FeatureTracker(xk_handle *xk, const Camera &camera, int max_features = 1024, int win_w = 31, int win_h = 31, int max_level = 2,
                 int max_iter = 30, double eps = 0.01, double min_eig_thr = 0.003);
  ~FeatureTracker();
  FeatureTracker(const FeatureTracker &) = delete;
  FeatureTracker &operator=(const FeatureTracker &) = delete;

  // the next frame, height rows of stride bytes: the current image becomes the previous one (tracker.cpp:302)
  void pushImage(const uint8_t *image, int stride);
  // previous: the features of the previous image, distorted pixels in getXDist / getYDist.  -> the kept features of the
  // previous list and, row for row, where they are in the current image (getXDist / getYDist; getX / getY are left for
  // the undistortion).  kept_indices (optional): their positions in the input list, ascending.
  std::pair<FeatureList, FeatureList> track(const FeatureList &previous, std::vector<int> *kept_indices = nullptr);
  int levels() const { return xk_trk_klt_levels(trk_); }

  // the parameters of the detection (tracker.h:245-255: 9, true, 20, 20) and the most candidates one image may have
  void setDetection(int threshold = 9, bool non_max_supp = true, int block_half_length = 20, int margin = 20, int max_candidates = 8192);
  // Tracker::featureDetection on the current image (the previous one: current_image = false, the reference's re-detection,
  // tracker.cpp:214): the new features outside the neighbourhood of old_features (getXDist / getYDist), best score first.
  // getXDist / getYDist are the integer pixels as doubles, pyramid level 0, getFastScore the score.
  FeatureList detect(const FeatureList &old_features, bool current_image = true);
  // Tracker::removeOverflowFeatures (tracker.cpp:592-620) with its quirks: both loops run on i - 1 and the second starts at
  // size - 1, so the last pair is never examined; the counts are the current list's, against max_feat_per_tile.
  static void removeOverflow(TileGrid &grid, FeatureList &previous, FeatureList &current);

 private:
  xk_handle *xk_;
  xk_trk *trk_ = nullptr;
  int max_features_ = 0;
  // staging for one call, sized once by max_features: points in, everything xk_trk_track reports out
  std::vector<float> prev_in_;
  std::vector<double> cur_, min_eig_, kept_prev_, kept_cur_;
  std::vector<unsigned char> status_;
  std::vector<int> keep_;
  std::vector<double> old_in_;
  std::vector<int> det_xy_, det_score_;
};
}  // namespace x
