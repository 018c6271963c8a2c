// Mirror of Tracker::featureTracking, Tracker::featureDetection and Tracker::calibrateImage, src/x/vision/tracker.cpp:623-690,
// :390-590 and :761-858; the arithmetic runs in libxk.so.  The tile bookkeeping (tiled_image.cpp:139-158, tracker.cpp:592-620) is host code, as in the reference.
#include "x/vision/feature_tracker.h"

#include <algorithm>
#include <stdexcept>
#include <string>

using namespace x;

static void check(xk_handle *h, int rc, const char *what) {
  if (rc != XK_OK) throw std::runtime_error(std::string(what) + ": " + xk_strerror(rc) + " (" + (h ? xk_last_error(h) : "") + ")");
}

FeatureTracker::FeatureTracker(xk_handle *xk, const Camera &camera, int max_features, int win_w, int win_h, int max_level, int max_iter,
                               double eps, double min_eig_thr)
    : xk_(xk), max_features_(max_features), width_((int)camera.getWidth()), height_((int)camera.getHeight()) {
  if (max_features < 1) throw std::runtime_error("FeatureTracker: max_features < 1");
  const size_t m = (size_t)max_features;                      // (the staging first: nothing below can throw once the handle exists)
  prev_in_.resize(2 * m); cur_.resize(2 * m); min_eig_.resize(m); kept_prev_.resize(2 * m); kept_cur_.resize(2 * m);
  status_.resize(m); keep_.resize(m);
  old_in_.resize(2 * m); det_xy_.resize(2 * m); det_score_.resize(m);
  check(xk_, xk_trk_create(xk_, max_features, camera.getFx(), camera.getFy(), camera.getCx(), camera.getCy(), camera.getS(), &trk_),
        "xk_trk_create");
  const int rc = xk_trk_klt_setup(trk_, (int)camera.getWidth(), (int)camera.getHeight(), win_w, win_h, max_level, max_iter, eps, min_eig_thr);
  if (rc != XK_OK) {
    xk_trk_destroy(trk_);
    check(xk_, rc, "xk_trk_klt_setup");
  }
}

FeatureTracker::~FeatureTracker() { xk_trk_destroy(trk_); }

void FeatureTracker::pushImage(const uint8_t *image, int stride) { check(xk_, xk_trk_push_image(trk_, image, stride), "xk_trk_push_image"); }

std::pair<FeatureList, FeatureList> FeatureTracker::track(const FeatureList &previous, std::vector<int> *kept_indices) {
  const size_t n = previous.size();
  if (n > status_.size()) throw std::runtime_error("FeatureTracker::track: more features than max_features");
  for (size_t i = 0; i < n; ++i) {                            // Feature::getDistPoint2f, tracker.cpp:629-633
    prev_in_[2 * i] = (float)previous[i].getXDist(); prev_in_[2 * i + 1] = (float)previous[i].getYDist();
  }
  int n_kept = 0;
  if (second_klt_ && photo_hyp_ > 0) check(xk_, xk_trk_klt_select(trk_, photo_done_ ? 1 : 0), "xk_trk_klt_select");   // tracker.cpp:641
  check(xk_, xk_trk_track(trk_, prev_in_.data(), (int)n, cur_.data(), status_.data(), min_eig_.data(), keep_.data(), kept_prev_.data(),
                          kept_cur_.data(), &n_kept),
        "xk_trk_track");
  std::pair<FeatureList, FeatureList> out;                    // features1 after the erase loop, features2 (:658-686)
  out.first.reserve((size_t)n_kept); out.second.reserve((size_t)n_kept);
  for (int k = 0; k < n_kept; ++k) {
    out.first.push_back(previous[(size_t)keep_[k]]);
    out.second.emplace_back(0.0, 0.0, kept_cur_[2 * k], kept_cur_[2 * k + 1]);
    out.second.back().setPyramidLevel(out.first.back().getPyramidLevel());   // :670-678: level and score of the previous feature
    out.second.back().setFastScore(out.first.back().getFastScore());
    if (out.first.back().hasDescriptor()) out.second.back().setDescriptor(out.first.back().getDescriptor().data());   // :675-679
  }
  if (kept_indices) kept_indices->assign(keep_.begin(), keep_.begin() + n_kept);
  if (photo_hyp_ > 0) fillIntensity(out.second, true, true);   // computeIntensity(img2, ...) of the raw current image, :666
  return out;
}

void FeatureTracker::setSecondKlt(int win_w, int win_h, int max_level, double min_eig_thr) {
  check(xk_, xk_trk_klt_second(trk_, win_w, win_h, max_level, min_eig_thr), "xk_trk_klt_second");
  second_klt_ = true;
  detection_set_ = false; desc_edge_ = 0; max_descriptors_ = 0; photo_hyp_ = 0;   // (every setup behind the KLT setup went with it)
  spatial_set_ = spatial_done_ = photo_done_ = false;
}

void FeatureTracker::selectKlt(int set) { check(xk_, xk_trk_klt_select(trk_, set), "xk_trk_klt_select"); }

void FeatureTracker::setPhotometric(int kernel_size, double epsilon_gap, double epsilon_base, int n_hyp) {
  check(xk_, xk_trk_photo_setup(trk_, kernel_size, epsilon_gap, epsilon_base, n_hyp), "xk_trk_photo_setup");
  photo_hyp_ = n_hyp;
  photo_done_ = false;                                           // (a new photo setup starts the ring over)
  spatial_set_ = spatial_done_ = false;                          // (a new photo setup drops the spatial one)
  const size_t m = (size_t)max_features_;
  photo_val_.resize(m); photo_in_.resize(m); photo_xy_.resize(2 * m); photo_sum_.resize(m); photo_cnt_.resize(m);
}

// computeIntensity at static_cast<int> of the distorted pixels (tracker.cpp:461, :666)
void FeatureTracker::fillIntensity(FeatureList &features, bool current_image, bool raw_plane) {
  const size_t n = features.size();
  if (n == 0) return;
  for (size_t i = 0; i < n; ++i) { photo_xy_[2 * i] = (int)features[i].getXDist(); photo_xy_[2 * i + 1] = (int)features[i].getYDist(); }
  check(xk_, xk_trk_photo_intensity(trk_, current_image ? 1 : 0, raw_plane ? 0 : 1, photo_xy_.data(), (int)n, photo_val_.data(),
                                    photo_sum_.data(), photo_cnt_.data()),
        "xk_trk_photo_intensity");
  for (size_t i = 0; i < n; ++i) features[i].setIntensity(photo_val_[i]);
}

FeatureTracker::Calibration FeatureTracker::calibrate(const FeatureList &previous, unsigned long seed) {
  if (photo_hyp_ == 0) throw std::runtime_error("FeatureTracker::calibrate: before setPhotometric");
  const size_t n = previous.size();
  if (n > (size_t)max_features_) throw std::runtime_error("FeatureTracker::calibrate: more features than max_features");
  for (size_t i = 0; i < n; ++i) {
    prev_in_[2 * i] = (float)previous[i].getXDist(); prev_in_[2 * i + 1] = (float)previous[i].getYDist();
    photo_in_[i] = previous[i].getIntensity();
  }
  Calibration c;
  int estimated = 0;
  const int n_hyp = std::max(1, std::min((int)n, photo_hyp_));
  check(xk_, xk_trk_photo_calibrate(trk_, prev_in_.data(), photo_in_.data(), (int)n, n_hyp, seed, keep_.data(), photo_val_.data(),
                                    photo_sum_.data(), photo_cnt_.data(), &c.kept, &c.a_rel, &c.b_rel, &c.support, c.frame_ab, &estimated),
        "xk_trk_photo_calibrate");
  c.estimated = estimated != 0;
  photo_done_ = photo_done_ || c.estimated;                       // tracker.cpp:849
  if (spatial_set_ && !spatial_done_ && c.estimated && spatialStatus().ready) {   // irPhotoCalib.cpp:199-209, without the thread
    check(xk_, xk_trk_photo_spatial_estimate(trk_, 1, &spatial_outcome_), "xk_trk_photo_spatial_estimate");
    spatial_done_ = spatial_outcome_.converged != 0;
  }
  return c;
}

void FeatureTracker::setSpatialCalibration(int div, double thr, int max_rows) {
  if (photo_hyp_ == 0) throw std::runtime_error("FeatureTracker::setSpatialCalibration: before setPhotometric");
  check(xk_, xk_trk_photo_spatial_setup(trk_, div, thr, 500, max_rows, 5.0, 0.01, 0.01), "xk_trk_photo_spatial_setup");
  spatial_set_ = true; spatial_done_ = false;
  spatial_outcome_ = xk_photo_spatial_outcome{};
}

FeatureTracker::SpatialStatus FeatureTracker::spatialStatus() {
  SpatialStatus s;
  int ready = 0;
  check(xk_, xk_trk_photo_spatial_status(trk_, &s.rows, &s.covered, &s.cells, &ready, &s.dropped, &s.state), "xk_trk_photo_spatial_status");
  s.ready = ready != 0;
  return s;
}

std::vector<float> FeatureTracker::spatialMap() {
  std::vector<float> out((size_t)width_ * height_);
  check(xk_, xk_trk_photo_spatial_stage(trk_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out.data()), "xk_trk_photo_spatial_stage");
  return out;
}

std::vector<uint8_t> FeatureTracker::image(bool current_image, bool raw) {
  std::vector<uint8_t> out((size_t)width_ * height_);
  if (raw) check(xk_, xk_trk_photo_raw(trk_, current_image ? 1 : 0, out.data()), "xk_trk_photo_raw");
  else check(xk_, xk_trk_klt_level(trk_, current_image ? 1 : 0, 0, out.data(), nullptr, nullptr, nullptr, nullptr), "xk_trk_klt_level");
  return out;
}

void FeatureTracker::setDetection(int threshold, bool non_max_supp, int block_half_length, int margin, int max_candidates) {
  const int keep[5] = {det_threshold_, det_nms_, det_b_, det_margin_, det_max_candidates_};
  det_threshold_ = threshold; det_nms_ = non_max_supp ? 1 : 0; det_b_ = block_half_length; det_margin_ = margin; det_max_candidates_ = max_candidates;
  try {
    applyDetection();
  } catch (...) {                                               // (the device kept its earlier setup: so do the members)
    det_threshold_ = keep[0]; det_nms_ = keep[1]; det_b_ = keep[2]; det_margin_ = keep[3]; det_max_candidates_ = keep[4];
    throw;
  }
  detection_set_ = true;
}

// the detection setup as asked for, its margin raised to the description's edge
void FeatureTracker::applyDetection() {
  check(xk_, xk_trk_detect_setup(trk_, det_threshold_, det_nms_, det_b_, std::max(det_margin_, desc_edge_), det_max_candidates_),
        "xk_trk_detect_setup");
}

void FeatureTracker::setDescription(bool centroid_orientation, double angle_deg, int edge, const signed char *pattern, int max_descriptors) {
  check(xk_, xk_trk_describe_setup(trk_, centroid_orientation ? 1 : 0, angle_deg, edge, pattern, max_descriptors), "xk_trk_describe_setup");
  desc_edge_ = edge; max_descriptors_ = max_descriptors;
  const size_t m = (size_t)max_descriptors;
  desc_xy_.resize(2 * m); desc_keep_.resize(m); desc_dir_.resize(2 * m); desc_mom_.resize(2 * m); desc_out_.resize(32 * m);
  if (detection_set_) applyDetection();
}

Descriptors FeatureTracker::describe(const std::vector<std::pair<int, int>> &pixels, bool current_image, std::vector<int> *kept_indices) {
  if (max_descriptors_ == 0) throw std::runtime_error("FeatureTracker::describe: before setDescription");
  const size_t n = pixels.size();
  if (n > (size_t)max_descriptors_) throw std::runtime_error("FeatureTracker::describe: more keypoints than max_descriptors");
  for (size_t i = 0; i < n; ++i) { desc_xy_[2 * i] = pixels[i].first; desc_xy_[2 * i + 1] = pixels[i].second; }
  int n_kept = 0;
  check(xk_, xk_trk_describe(trk_, current_image ? 1 : 0, n ? desc_xy_.data() : nullptr, (int)n, desc_out_.data(), desc_keep_.data(),
                             desc_dir_.data(), desc_mom_.data(), &n_kept),
        "xk_trk_describe");
  Descriptors out;
  out.rows = n_kept; out.cols = 32;
  out.data.assign(desc_out_.begin(), desc_out_.begin() + 32 * (size_t)n_kept);
  if (kept_indices) kept_indices->assign(desc_keep_.begin(), desc_keep_.begin() + n_kept);
  return out;
}

FeatureList FeatureTracker::detect(const FeatureList &old_features, bool current_image) {
  const size_t n_old = old_features.size();
  if (n_old > (size_t)max_features_) throw std::runtime_error("FeatureTracker::detect: more old features than max_features");
  for (size_t i = 0; i < n_old; ++i) { old_in_[2 * i] = old_features[i].getXDist(); old_in_[2 * i + 1] = old_features[i].getYDist(); }
  int n_found = 0, n_candidates = 0;
  check(xk_, xk_trk_detect(trk_, current_image ? 1 : 0, n_old ? old_in_.data() : nullptr, (int)n_old, det_xy_.data(), det_score_.data(),
                           &n_found, &n_candidates),
        "xk_trk_detect");
  FeatureList out;
  out.reserve((size_t)n_found);
  for (int k = 0; k < n_found; ++k) {                          // Feature(..., pt.x * scale_factor, pt.y * scale_factor, level, response), :464-467
    out.emplace_back(0.0, 0.0, (double)det_xy_[2 * k], (double)det_xy_[2 * k + 1]);
    out.back().setPyramidLevel(0);
    out.back().setFastScore((double)det_score_[k]);
  }
  if (max_descriptors_ > 0 && n_found > 0) {                   // PlaceRecognition::compute of the keypoints, tracker.cpp:440-444
    std::vector<std::pair<int, int>> pixels((size_t)n_found);
    for (int k = 0; k < n_found; ++k) pixels[(size_t)k] = {det_xy_[2 * k], det_xy_[2 * k + 1]};
    const Descriptors d = describe(pixels, current_image);
    if (d.rows != n_found) throw std::runtime_error("FeatureTracker::detect: the description dropped a detected feature");   // (margin >= edge)
    for (int k = 0; k < n_found; ++k) out[(size_t)k].setDescriptor(d.data.data() + 32 * (size_t)k);
  }
  if (photo_hyp_ > 0) fillIntensity(out, current_image, false);   // computeIntensity of the (corrected) image, tracker.cpp:461
  return out;
}

TileGrid::TileGrid(unsigned int width, unsigned int height, unsigned int n_tiles_h, unsigned int n_tiles_w, unsigned int max_feat_per_tile)
    : rows_(height), n_tiles_h_(n_tiles_h), n_tiles_w_(n_tiles_w), max_feat_per_tile_(max_feat_per_tile) {
  if (n_tiles_h < 1 || n_tiles_w < 1) throw std::runtime_error("TileGrid: no tiles");
  tile_height_ = (double)height / n_tiles_h;                   // tiled_image.cpp:104-105
  tile_width_ = (double)width / n_tiles_w;
  tiles_.assign((size_t)n_tiles_h * n_tiles_w, 0u);
}

void TileGrid::setTileForFeature(TrackedFeature &feature) const {
  double c = feature.getXDist() - tile_width_ - 0.5;           // tiled_image.cpp:141-146
  int col = 0;
  while (c > 0) {
    col += 1;
    c -= tile_width_;
  }
  double r = rows_ - feature.getYDist() - 0.5;                 // :149-154
  int row = static_cast<int>(n_tiles_h_) - 1;
  while (r > tile_height_) {
    row -= 1;
    r -= tile_height_;
  }
  feature.setTile(row, col);
}

void TileGrid::resetFeatureCounts() { std::fill(tiles_.begin(), tiles_.end(), 0u); }

void TileGrid::incrementFeatureCountAtTile(int row, int col) {
  if (row >= 0 && row < (int)n_tiles_h_ && col >= 0 && col < (int)n_tiles_w_) tiles_[(size_t)row * n_tiles_w_ + col] += 1;
}

unsigned int TileGrid::getFeatureCountAtTile(int row, int col) const {
  return (row >= 0 && row < (int)n_tiles_h_ && col >= 0 && col < (int)n_tiles_w_) ? tiles_[(size_t)row * n_tiles_w_ + col] : 0u;
}

void FeatureTracker::removeOverflow(TileGrid &grid, FeatureList &features1, FeatureList &features2) {
  if (features1.size() != features2.size()) throw std::runtime_error("FeatureTracker::removeOverflow: lists differ in length");
  grid.resetFeatureCounts();
  for (auto i = features2.size(); i >= 1; i--) {               // tracker.cpp:598-606
    grid.setTileForFeature(features1[i - 1]);
    grid.setTileForFeature(features2[i - 1]);
    grid.incrementFeatureCountAtTile(features2[i - 1].getTileRow(), features2[i - 1].getTileCol());
  }
  for (int i = (int)features2.size() - 1; i >= 1; i--) {       // :610-619
    const unsigned int count = grid.getFeatureCountAtTile(features2[i - 1].getTileRow(), features2[i - 1].getTileCol());
    if (count > grid.getMaxFeatPerTile()) {
      features1.erase(features1.begin() + i - 1);
      features2.erase(features2.begin() + i - 1);
    }
  }
}
