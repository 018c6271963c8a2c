// Mirror of Tracker::track, src/x/vision/tracker.cpp:134-306; the frame runs in libxk.so behind xk_trk_frame, and behind
// xk_trk_photo_frame after setPhotometric.
#include "x/vision/tracker.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

using namespace x;

static void check(xk_handle *h, int rc, const char *what) {
  if (rc != XK_OK) throw std::runtime_error(std::string(what) + ": " + xk_strerror(rc) + " (" + (h ? xk_last_error(h) : "") + ")");
}

Tracker::Tracker(xk_handle *xk, const Camera &cam, int fast_detection_delta, bool non_max_supp, unsigned int block_half_length,
                 unsigned int margin, unsigned int n_feat_min, int outlier_method, double outlier_param1, double /*outlier_param2*/,
                 int win_size_w, int win_size_h, int max_level, double min_eig_thr, int max_features, int n_hyp)
    : xk_(xk), width_((int)cam.getWidth()), height_((int)cam.getHeight()), max_features_(max_features), threshold_(fast_detection_delta),
      nms_(non_max_supp ? 1 : 0), b_((int)block_half_length), margin_((int)margin), n_feat_min_((int)n_feat_min), win_w_(win_size_w),
      win_h_(win_size_h), max_level_(max_level), n_hyp_(n_hyp), outlier_method_(outlier_method == XK_TRK_LMEDS ? XK_TRK_LMEDS : XK_TRK_RANSAC),
      threshold_px_(outlier_param1), min_eig_thr_(min_eig_thr) {
  if (max_features < 1) throw std::runtime_error("Tracker: max_features < 1");
  const size_t m = (size_t)max_features;                      // (the staging first: nothing below can throw once the handle exists)
  prev_xy_.resize(2 * m); cur_xy_.resize(2 * m); prev_dist_.resize(2 * m); cur_dist_.resize(2 * m);
  score_.resize(m); origin_.resize(m); tiles_.resize(4 * m); desc_.resize(32 * m);
  out_.prev_xy = prev_xy_.data(); out_.cur_xy = cur_xy_.data(); out_.prev_dist_xy = prev_dist_.data(); out_.cur_dist_xy = cur_dist_.data();
  out_.score = score_.data(); out_.origin = origin_.data(); out_.tiles = tiles_.data(); out_.desc = desc_.data();
  check(xk_, xk_trk_create(xk_, max_features, cam.getFx(), cam.getFy(), cam.getCx(), cam.getCy(), cam.getS(), &trk_), "xk_trk_create");
  int rc = XK_OK;
  if (cam.getModel() != XK_CAM_FOV) {                           // the camera's lens (Camera::setDistortion)
    const std::vector<double> k = cam.getCoeffs();
    rc = xk_trk_camera_model(trk_, cam.getModel(), k.data(), (int)k.size());
    if (rc != XK_OK) {
      xk_trk_destroy(trk_);
      check(xk_, rc, "xk_trk_camera_model");
    }
  }
  rc = xk_trk_klt_setup(trk_, width_, height_, win_w_, win_h_, max_level_, 30, 0.01, min_eig_thr_);   // term_crit_, tracker.cpp:47
  if (rc != XK_OK) {
    xk_trk_destroy(trk_);
    check(xk_, rc, "xk_trk_klt_setup");
  }
}

Tracker::~Tracker() { xk_trk_destroy(trk_); }

void Tracker::setTiles(unsigned int n_tiles_h, unsigned int n_tiles_w, unsigned int max_feat_per_tile) {
  tiles_h_ = n_tiles_h; tiles_w_ = n_tiles_w; max_per_tile_ = std::min(max_feat_per_tile, 1u << 30);
  dirty_ = true;
}

void Tracker::setDescription(bool centroid_orientation, double angle_deg, int edge, const signed char *pattern) {
  described_ = true; centroid_ = centroid_orientation; angle_deg_ = angle_deg; edge_ = edge;
  own_pattern_ = pattern != nullptr;
  if (pattern) std::memcpy(pattern_, pattern, sizeof pattern_);
  dirty_ = true;
}

void Tracker::setPhotometric(int kernel_size, double epsilon_gap, double epsilon_base, int n_hyp_photo, int fast_detection_delta_photo) {
  photo_ = true; photo_kernel_ = kernel_size; eps_gap_ = epsilon_gap; eps_base_ = epsilon_base; photo_hyp_ = n_hyp_photo;
  photo_threshold_ = fast_detection_delta_photo;
  const size_t m = (size_t)max_features_;
  prev_int_.resize(m); cur_int_.resize(m);
  dirty_ = true;
}

void Tracker::setSecondKlt(int win_size_w, int win_size_h, int max_level, double min_eig_thr) {
  second_ = second_pending_ = true;
  win_w2_ = win_size_w; win_h2_ = win_size_h; max_level2_ = max_level; min_eig_thr2_ = min_eig_thr;
  dirty_ = true;
}

void Tracker::setSpatialCalibration(int div, double thr, int max_rows) {
  if (!photo_) throw std::runtime_error("Tracker::setSpatialCalibration: before setPhotometric");
  spatial_ = true; spatial_div_ = div; spatial_thr_ = thr; spatial_rows_ = max_rows;
  dirty_ = true;
}

bool Tracker::lastLmeds(double *median, double *sigma) {
  double last[2] = {0.0, 0.0};
  if (xk_trk_fundamental_medians(trk_, 0, 0, nullptr, last) != XK_OK) return false;
  if (median) *median = last[0];
  if (sigma) *sigma = last[1];
  return true;
}

void Tracker::reset() {
  img_id_ = 0;
  matches_.clear();
  if (!dirty_) check(xk_, xk_trk_frame_reset(trk_), "xk_trk_frame_reset");
}

// detection, description and frame setups, in the order each needs the one before; a new one starts the tracker over
void Tracker::apply() {
  check(xk_, xk_trk_outlier_method(trk_, outlier_method_), "xk_trk_outlier_method");
  if (second_pending_) {                                      // before every setup below: it drops them and forgets the images
    check(xk_, xk_trk_klt_second(trk_, win_w2_, win_h2_, max_level2_, min_eig_thr2_), "xk_trk_klt_second");
    second_pending_ = false;
  }
  check(xk_, xk_trk_detect_setup(trk_, threshold_, nms_, b_, described_ ? std::max(margin_, edge_) : margin_, 32768), "xk_trk_detect_setup");
  if (described_)
    check(xk_, xk_trk_describe_setup(trk_, centroid_ ? 1 : 0, angle_deg_, edge_, own_pattern_ ? pattern_ : nullptr, max_features_),
          "xk_trk_describe_setup");
  check(xk_, xk_trk_frame_setup(trk_, n_feat_min_, (int)tiles_h_, (int)tiles_w_, (int)max_per_tile_, threshold_px_, n_hyp_), "xk_trk_frame_setup");
  if (photo_) {                                               // a new photo setup: the ring starts over, as the tracker does
    check(xk_, xk_trk_photo_setup(trk_, photo_kernel_, eps_gap_, eps_base_, photo_hyp_), "xk_trk_photo_setup");
    if (spatial_)
      check(xk_, xk_trk_photo_spatial_setup(trk_, spatial_div_, spatial_thr_, 500, spatial_rows_, 5.0, 0.01, 0.01), "xk_trk_photo_spatial_setup");
    check(xk_, xk_trk_photo_frame_setup(trk_, photo_hyp_, photo_threshold_), "xk_trk_photo_frame_setup");
    spatial_done_ = false;
    spatial_outcome_ = xk_photo_spatial_outcome{};
  }
  calibration_ = Calibration{};
  dirty_ = false;
  img_id_ = 0;
}

const MatchList &Tracker::track(const uint8_t *img, int stride, double /*timestamp*/, unsigned int /*frame_number*/) {
  if (dirty_) apply();
  matches_.clear();
  origin_v_.clear();
  int rc;
  if (photo_) {
    pout_.prev_xy = out_.prev_xy; pout_.cur_xy = out_.cur_xy; pout_.prev_dist_xy = out_.prev_dist_xy; pout_.cur_dist_xy = out_.cur_dist_xy;
    pout_.score = out_.score; pout_.origin = out_.origin; pout_.tiles = out_.tiles; pout_.desc = out_.desc;
    pout_.prev_intensity = prev_int_.data(); pout_.cur_intensity = cur_int_.data();
    rc = xk_trk_photo_frame(trk_, img, stride, seed_++, seed_photo_++, &pout_);
    out_.n_tracked = pout_.n_tracked; out_.n_left = pout_.n_left; out_.redetected = pout_.redetected; out_.n_candidates = pout_.n_candidates;
    out_.n_accepted = pout_.n_accepted; out_.n_new_tracked = pout_.n_new_tracked; out_.n_matches = pout_.n_matches; out_.winner = pout_.winner;
    Calibration &c = calibration_;
    c.estimated = pout_.estimated != 0; c.done = pout_.done != 0; c.kept = pout_.n_cal_kept; c.support = pout_.support;
    c.a_rel = pout_.a_rel; c.b_rel = pout_.b_rel;
    std::memcpy(c.frame_ab, pout_.frame_ab, sizeof c.frame_ab);
  } else {
    rc = xk_trk_frame(trk_, img, stride, seed_++, &out_);
  }
  if (rc != XK_OK) img_id_ = 0;                               // (the device starts over too)
  check(xk_, rc, photo_ ? "xk_trk_photo_frame" : "xk_trk_frame");
  if (spatial_ && !spatial_done_ && calibration_.estimated) {  // irPhotoCalib.cpp:199-209, without the thread: as FeatureTracker::calibrate
    int rows, covered, cells, ready = 0, dropped, state;
    check(xk_, xk_trk_photo_spatial_status(trk_, &rows, &covered, &cells, &ready, &dropped, &state), "xk_trk_photo_spatial_status");
    if (ready) {
      check(xk_, xk_trk_photo_spatial_estimate(trk_, 1, &spatial_outcome_), "xk_trk_photo_spatial_estimate");
      spatial_done_ = spatial_outcome_.converged != 0;
    }
  }
  img_id_++;                                                  // tracker.cpp:137
  const size_t n = (size_t)out_.n_matches;
  matches_.resize(n);
  origin_v_.assign(origin_.begin(), origin_.begin() + n);
  for (size_t i = 0; i < n; ++i) {                            // tracker.cpp:286-293
    Match &m = matches_[i];
    m.previous = TrackedFeature(prev_xy_[2 * i], prev_xy_[2 * i + 1], prev_dist_[2 * i], prev_dist_[2 * i + 1]);
    m.current = TrackedFeature(cur_xy_[2 * i], cur_xy_[2 * i + 1], cur_dist_[2 * i], cur_dist_[2 * i + 1]);
    m.previous.setTile(tiles_[4 * i], tiles_[4 * i + 1]);
    m.current.setTile(tiles_[4 * i + 2], tiles_[4 * i + 3]);
    for (TrackedFeature *f : {&m.previous, &m.current}) {
      f->setFastScore((double)score_[i]);                     // :670-679: level, score and descriptor of the previous feature
      f->setPyramidLevel(0);
      if (described_) f->setDescriptor(desc_.data() + 32 * i);
    }
    if (photo_) { m.previous.setIntensity(prev_int_[i]); m.current.setIntensity(cur_int_[i]); }   // tracker.cpp:461, :666
  }
  return matches_;
}
