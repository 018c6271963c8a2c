// x::Camera of the mirror: pinhole intrinsics and the inverse of the FOV distortion, host arithmetic.  The formula is
// the one csrc/xk_fundamental.hip.h applies on the device (xk_fund_undistort1): same threshold, same order of operations.
#include "x/vision/camera.h"

#include <cmath>
#include <stdexcept>

#include "../../x_multi_agent_amd/csrc/xk_camera.h"   // the radial-tangential and the equidistant model: the text the device compiles

namespace x {

Camera::Camera(double fx, double fy, double cx, double cy, double s, unsigned int img_width, unsigned int img_height)
    : focal_{fx * img_width, fy * img_height}, centre_{cx * img_width, cy * img_height}, fov_(s),
      half_cot_(s != 0.0 ? 0.5 / std::tan(0.5 * s) : 0.0), width_(img_width), height_(img_height) {}

double Camera::radialGain(double r_d) const {
  // below a hundredth of the focal length the model is the identity to first order, and r_d = 0 would divide by zero
  if (fov_ == 0.0 || !(r_d > 0.01)) return 1.0;
  return std::tan(r_d * fov_) * half_cot_ / r_d;
}

void Camera::setDistortion(int model, const std::vector<double> &coeffs) {
  const size_t n = coeffs.size();
  const bool count_ok = model == XK_CAM_MODEL_FOV ? n == 1 : model == XK_CAM_MODEL_RADTAN ? (n == 4 || n == 5) :
                        model == XK_CAM_MODEL_EQUIDISTANT ? n == 4 : false;
  if (!count_ok) throw std::invalid_argument("Camera::setDistortion: model is 0 (1 coefficient), 1 (4 or 5) or 2 (4)");
  for (double c : coeffs)
    if (!std::isfinite(c)) throw std::invalid_argument("Camera::setDistortion: coefficient not finite");
  model_ = model; n_coeffs_ = (int)n;
  for (double &c : k_) c = 0.0;
  if (model == XK_CAM_MODEL_FOV) {
    fov_ = coeffs[0];
    half_cot_ = fov_ != 0.0 ? 0.5 / std::tan(0.5 * fov_) : 0.0;
  } else {
    for (size_t i = 0; i < n; ++i) k_[i] = coeffs[i];
  }
}

std::vector<double> Camera::getCoeffs() const {
  if (model_ == XK_CAM_MODEL_FOV) return {fov_};
  return std::vector<double>(k_, k_ + n_coeffs_);
}

bool Camera::undistort(double u_dist, double v_dist, double *u, double *v, int *steps) const {
  const double xd = toPlane(u_dist, 0), yd = toPlane(v_dist, 1);
  double x, y;
  int it = 0;
  bool ok = true;
  if (model_ == XK_CAM_MODEL_FOV) {
    const double gain = radialGain(std::sqrt(xd * xd + yd * yd));
    x = gain * xd; y = gain * yd;
  } else {
    ok = xk_cam_inverse(model_, k_, xd, yd, &x, &y, &it);
  }
  *u = ok ? toPixel(x, 0) : u_dist;                            // an invalid point keeps its distorted pixel
  *v = ok ? toPixel(y, 1) : v_dist;
  if (steps) *steps = it;
  return ok;
}

void Camera::undistort(TrackedFeature &feature) const {
  double u, v;
  undistort(feature.getXDist(), feature.getYDist(), &u, &v);
  feature.setX(u);
  feature.setY(v);
}

void Camera::distort(double u, double v, double *u_dist, double *v_dist) const {
  const double x = toPlane(u, 0), y = toPlane(v, 1);
  double xd = x, yd = y;
  if (model_ != XK_CAM_MODEL_FOV) {
    xk_cam_forward(model_, k_, x, y, &xd, &yd);
  } else if (fov_ != 0.0) {                                     // r_d = atan(2 r tan(s/2)) / s, the identity where undistort is
    const double r = std::sqrt(x * x + y * y);
    const double rd = std::atan(r / half_cot_) / fov_;
    if (rd > 0.01) { xd = x * (rd / r); yd = y * (rd / r); }
  }
  *u_dist = toPixel(xd, 0);
  *v_dist = toPixel(yd, 1);
}

void Camera::distort(TrackedFeature &feature) const {
  double u, v;
  distort(feature.getX(), feature.getY(), &u, &v);
  feature.setXDist(u);
  feature.setYDist(v);
}

void Camera::undistort(FeatureList &features) const {
  for (TrackedFeature &f : features) undistort(f);
}

Feature Camera::normalize(const Feature &feature) const {
  return Feature(toPlane(feature.getX(), 0), toPlane(feature.getY(), 1));
}

TrackedFeature Camera::normalize(const TrackedFeature &feature) const {
  return TrackedFeature(toPlane(feature.getX(), 0), toPlane(feature.getY(), 1), toPlane(feature.getXDist(), 0),
                        toPlane(feature.getYDist(), 1));
}

Track Camera::normalize(const Track &track, size_t max_size) const {
  // the newest max_size features: the tail of the track
  const size_t skip = (max_size != 0 && track.size() > max_size) ? track.size() - max_size : 0;
  Track out;
  out.setId(track.getId());
  out.reserve(track.size() - skip);
  for (auto it = track.begin() + (std::ptrdiff_t)skip; it != track.end(); ++it) out.push_back(normalize(*it));
  return out;
}

TrackList Camera::normalize(const TrackList &tracks, size_t max_size) const {
  TrackList out;
  out.reserve(tracks.size());
  for (const Track &t : tracks) out.push_back(normalize(t, max_size));
  return out;
}

}  // namespace x
