// x/vision/feature_tracker.h -- Tracker::featureTracking (src/x/vision/tracker.cpp:623-690) on the mirror:
// cv::calcOpticalFlowPyrLK(previous image, current image, pts1, pts2, status, err, win_size_, max_level_, term_crit_,
// cv::OPTFLOW_LK_GET_MIN_EIGENVALS, min_eig_thr_) on the previous features' distorted pixels, then the pairs that were tracked
// and stayed inside the frame.  All of it runs on the GPU behind xk_trk_push_image / xk_trk_track (include/xk.h); the lists it
// returns are what x::MatchFilter::filter takes.  There is no CPU fallback.
// Tracker::featureDetection (tracker.cpp:390-590) -- cv::FAST, the border, the sort by score and the selection outside the old
// features' neighbourhoods -- runs on the GPU too, behind xk_trk_detect.  The tile bookkeeping around it,
// TiledImage::setTileForFeature (tiled_image.cpp:139-158) and Tracker::removeOverflowFeatures (tracker.cpp:592-620), is host
// code here as it is there: list walks over a few hundred items.
// PlaceRecognition::compute (place_recognition.cpp:72-94), the cv::ORB::compute a MULTI_UAV build runs on the keypoints of every
// detection (tracker.cpp:440-444), runs on the GPU behind xk_trk_describe.
// Tracker::calibrateImage (tracker.cpp:761-858), the photometric calibration a PHOTOMETRIC_CALI build runs on every frame after the
// first, runs on the GPU behind xk_trk_photo_calibrate.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "x/place_recognition/database.h"
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
  unsigned int getNTilesH() const { return n_tiles_h_; }
  unsigned int getNTilesW() const { return n_tiles_w_; }

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
  // The second parameter set of a PHOTOMETRIC_CALI build (win_size_photo_, max_level_photo_, min_eig_thr_photo_; xk_trk_klt_second).
  // A setup: the pushed images are forgotten and setDetection, setDescription, setPhotometric and setSpatialCalibration have to be
  // called again.  After setPhotometric track() picks the set from this object's own calibration, as tracker.cpp:641 does: the second
  // set once a calibrate() has estimated gains, the first before; calibrate() itself always tracks with the first (:784-787).
  void setSecondKlt(int win_w, int win_h, int max_level, double min_eig_thr);
  // the set track() uses without a photometric calibration (xk_trk_klt_select): 0, or 1 after setSecondKlt
  void selectKlt(int set);
  int selectedKlt() const { return xk_trk_klt_selected(trk_); }   // the set the last track() used
  int levelsOf(int set) const { return xk_trk_klt_levels_of(trk_, set); }

  // the parameters of the detection (tracker.h:245-255: 9, true, 20, 20) and the most candidates one image may have
  void setDetection(int threshold = 9, bool non_max_supp = true, int block_half_length = 20, int margin = 20, int max_candidates = 8192);
  // Tracker::featureDetection on the current image (the previous one: current_image = false, the reference's re-detection,
  // tracker.cpp:214): the new features outside the neighbourhood of old_features (getXDist / getYDist), best score first.
  // getXDist / getYDist are the integer pixels as doubles, pyramid level 0, getFastScore the score.
  FeatureList detect(const FeatureList &old_features, bool current_image = true);
  // Tracker::removeOverflowFeatures (tracker.cpp:592-620) with its quirks: both loops run on i - 1 and the second starts at
  // size - 1, so the last pair is never examined; the counts are the current list's, against max_feat_per_tile.
  static void removeOverflow(TileGrid &grid, FeatureList &previous, FeatureList &current);

  // The description of detected features (xk_trk_describe_setup): centroid_orientation false takes every descriptor at the fixed
  // angle_deg -- what cv::ORB::compute sees on cv::FAST keypoints, whose angle is -1 -- true at the intensity centroid's; edge is
  // OpenCV's edgeThreshold; pattern [256][4] (x1 y1 x2 y2), nullptr: the project's default; max_descriptors the most keypoints one
  // describe() takes.  The reference drops the keypoints within edge of the border BEFORE the selection.  So that the features
  // detect() returns are the same ones, the detection's margin is RAISED to edge from here on (now, if setDetection was called,
  // and in every later setDetection): with margin >= edge the description drops nothing, and describing the accepted features
  // equals the reference's order, describe all and then select, because descriptors do not influence the selection.
  // From then on detect() fills getDescriptor() of what it returns and track() hands it from the previous to the current feature
  // (tracker.cpp:675-679).
  void setDescription(bool centroid_orientation = false, double angle_deg = -1.0, int edge = 31, const signed char *pattern = nullptr,
                      int max_descriptors = 8192);
  // cv::ORB::compute on pixels of the caller's choice, e.g. every candidate of a detection, the reference's descriptros_
  // (place_recognition.cpp:92): the rows of the keypoints at least edge inside the image, in input order; kept_indices
  // (optional): their positions in the input list.
  Descriptors describe(const std::vector<std::pair<int, int>> &pixels, bool current_image = true, std::vector<int> *kept_indices = nullptr);

  // The photometric calibration (xk_trk_photo_setup): kernel_size is intensities_kernel_size_ (tracker.h:366), epsilon_gap and
  // epsilon_base the drift parameters of IRPhotoCalib, n_hyp the most hypotheses of a gain estimate (a frame evaluates
  // min(features, n_hyp); the reference runs as many as it has features).  From then on detect() fills getIntensity() from the
  // working image (tracker.cpp:461) and track() from the raw current image (:666).
  void setPhotometric(int kernel_size = 30, double epsilon_gap = 0.0, double epsilon_base = 0.0, int n_hyp = 512);
  struct Calibration {
    bool estimated = false;              // gains were estimated by this call
    int kept = 0, support = 0;           // features the raw tracking kept, inliers of the estimate
    double a_rel = 1.0, b_rel = 0.0;     // the estimate against the previous frame
    double frame_ab[4] = {0, 0, 0, 0};   // the pair after the drift adjustments, the frame's origin pair
  };
  // Tracker::calibrateImage (tracker.cpp:761-858) on the features of the previous image (getXDist / getYDist, getIntensity):
  // call it between pushImage and track, as tracker.cpp:186-195 orders them.  The current image is corrected on the device.
  Calibration calibrate(const FeatureList &previous, unsigned long seed = 0);
  // The spatial map of IRPhotoCalib (xk_trk_photo_spatial_setup), after setPhotometric: div is the reference's
  // temporal_params_div, thr its spatial_params_thr (spatial_params switches it on: calling this is that switch); the cap per cell,
  // the row capacity and the GP's hyperparameters are IRPhotoCalib's own (500; 5, 0.01, 0.01).  From then on calibrate() also
  // accumulates the frame's rows on the device, reads the status after its call, and once the coverage passes thr runs the
  // estimate and installs the map.  That is synchronous, on the caller's thread; the reference starts a std::thread
  // (irPhotoCalib.cpp:204).  An estimate that does not converge installs nothing and the accumulation goes on (:372-385).
  void setSpatialCalibration(int div = 16, double thr = 0.9, int max_rows = 1 << 18);
  bool spatialCalibrated() const { return spatial_done_; }   // IRPhotoCalib::isReady
  struct SpatialStatus {
    int rows = 0, covered = 0, cells = 0, dropped = 0, state = 0;   // state: 0 accumulating, 1 estimated, 2 failed and accumulating
    bool ready = false;
  };
  SpatialStatus spatialStatus();
  const xk_photo_spatial_outcome &spatialOutcome() const { return spatial_outcome_; }   // of the last estimate calibrate() ran
  std::vector<float> spatialMap();   // the last estimate's map, height rows of width floats
  // level 0 of the current (or previous) image as the device holds it, height rows of width bytes: the working image, which the
  // tracking, the detection and the description read, or with raw = true (after setPhotometric) the image as pushed
  std::vector<uint8_t> image(bool current_image = true, bool raw = false);

 private:
  void fillIntensity(FeatureList &features, bool current_image, bool raw_plane);
  void applyDetection();
  xk_handle *xk_;
  xk_trk *trk_ = nullptr;
  int max_features_ = 0;
  int width_ = 0, height_ = 0;
  // staging for one call, sized once by max_features: points in, everything xk_trk_track reports out
  std::vector<float> prev_in_;
  std::vector<double> cur_, min_eig_, kept_prev_, kept_cur_;
  std::vector<unsigned char> status_;
  std::vector<int> keep_;
  std::vector<double> old_in_;
  std::vector<int> det_xy_, det_score_;
  bool detection_set_ = false;
  int det_threshold_ = 9, det_nms_ = 1, det_b_ = 20, det_margin_ = 20, det_max_candidates_ = 8192;
  int desc_edge_ = 0, max_descriptors_ = 0;   // 0: no description set up
  std::vector<int> desc_xy_, desc_keep_, desc_dir_, desc_mom_;
  std::vector<unsigned char> desc_out_;
  int photo_hyp_ = 0;                         // 0: no photometric calibration set up
  bool second_klt_ = false, photo_done_ = false;   // setSecondKlt was called; a calibrate() has estimated gains (CALIBRATION_DONE)
  std::vector<double> photo_val_, photo_in_;
  std::vector<int> photo_xy_, photo_sum_, photo_cnt_;
  bool spatial_set_ = false, spatial_done_ = false;
  xk_photo_spatial_outcome spatial_outcome_ = {};
};
}  // namespace x
