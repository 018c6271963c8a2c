// x::Camera of the mirror: pinhole intrinsics and the inverse of the FOV distortion, host arithmetic.  The formula is
// the one csrc/xk_fundamental.hip.h applies on the device (xk_fund_undistort1): same threshold, same order of operations.
#include "x/vision/camera.h"

#include <cmath>

namespace x {

Camera::Camera(double fx, double fy, double cx, double cy, double s, unsigned int img_width, unsigned int img_height)
    : focal_{fx * img_width, fy * img_height}, centre_{cx * img_width, cy * img_height}, fov_(s),
      half_cot_(s != 0.0 ? 0.5 / std::tan(0.5 * s) : 0.0), width_(img_width), height_(img_height) {}

double Camera::radialGain(double r_d) const {
  // below a hundredth of the focal length the model is the identity to first order, and r_d = 0 would divide by zero
  if (fov_ == 0.0 || !(r_d > 0.01)) return 1.0;
  return std::tan(r_d * fov_) * half_cot_ / r_d;
}

void Camera::undistort(TrackedFeature &feature) const {
  const double x = toPlane(feature.getXDist(), 0), y = toPlane(feature.getYDist(), 1);
  const double gain = radialGain(std::sqrt(x * x + y * y));
  feature.setX(toPixel(gain * x, 0));
  feature.setY(toPixel(gain * y, 1));
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
