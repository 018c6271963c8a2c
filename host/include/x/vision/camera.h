// x/vision/camera.h -- x::Camera for the mirror: the public interface a caller of the reference's camera class expects
// (construction from intrinsics given as fractions of the image size, undistort and normalize on features, tracks and
// track lists), written here from the model itself: a pinhole camera with the one-parameter FOV distortion,
//   r_u = tan(r_d s) / (2 tan(s / 2)),
// as csrc/xk_fundamental.hip.h states it (xk_fund_undistort1).  Plain host arithmetic; x::MatchFilter runs the same
// undistortion on the device for whole match lists.
// setDistortion replaces the FOV lens by the radial-tangential (Kalibr's radtan) or the equidistant (Kannala-Brandt) model of
// xk_trk_camera_model (include/xk.h); their per-point functions are the text the device compiles (csrc/xk_camera.h).
// normalize stays pinhole: it takes undistorted pixels.
#pragma once
#include <cstddef>
#include <vector>

#include "x/vision/types.h"

namespace x {
class Camera {
 public:
  Camera() = default;
  // fx, fy, cx, cy as fractions of the image size (the way the parameter files give them), s: FOV parameter, 0 = none
  Camera(double fx, double fy, double cx, double cy, double s, unsigned int img_width, unsigned int img_height);

  unsigned int getWidth() const { return width_; }
  unsigned int getHeight() const { return height_; }
  double getFx() const { return focal_[0]; }                      // pixels
  double getFy() const { return focal_[1]; }
  double getCx() const { return centre_[0]; }
  double getCy() const { return centre_[1]; }
  double getS() const { return fov_; }
  // model: 0 FOV (coeffs = {s}), 1 radial-tangential (k1 k2 p1 p2 [k3]), 2 equidistant (k1 k2 k3 k4); throws std::invalid_argument on
  // an unknown model, a count the model does not take or a non-finite coefficient, and the camera stays what it was
  void setDistortion(int model, const std::vector<double> &coeffs);
  int getModel() const { return model_; }
  std::vector<double> getCoeffs() const;                          // what setDistortion would take to make this camera's lens
  double getInvFx() const { return 1.0 / focal_[0]; }
  double getInvFy() const { return 1.0 / focal_[1]; }
  double getCxN() const { return centre_[0] / focal_[0]; }        // principal point over focal length
  double getCyN() const { return centre_[1] / focal_[1]; }

  void undistort(FeatureList &features) const;                    // every feature of the list
  void undistort(TrackedFeature &feature) const;                  // distorted pixels -> setX / setY, undistorted pixels
  // the same on one pixel; false: the point is invalid under the model (it folds there or Newton did not converge) and (u, v) is the
  // distorted pixel itself.  steps (optional): Newton steps taken
  bool undistort(double u_dist, double v_dist, double *u, double *v, int *steps = nullptr) const;
  void distort(double u, double v, double *u_dist, double *v_dist) const;   // the forward map: undistorted -> distorted pixels
  void distort(TrackedFeature &feature) const;                    // getX / getY -> setXDist / setYDist
  Feature normalize(const Feature &feature) const;                // pixels -> (u - cx) / fx, (v - cy) / fy
  TrackedFeature normalize(const TrackedFeature &feature) const;  // ... the distorted pair too
  Track normalize(const Track &track, size_t max_size = 0) const;             // the newest max_size features (0: all)
  TrackList normalize(const TrackList &tracks, size_t max_size = 0) const;

 private:
  double toPlane(double pixel, int axis) const { return (pixel - centre_[axis]) / focal_[axis]; }
  double toPixel(double plane, int axis) const { return plane * focal_[axis] + centre_[axis]; }
  double radialGain(double r_d) const;                            // r_u / r_d of the FOV model; 1 near the centre and for s = 0
  double focal_[2] = {1.0, 1.0}, centre_[2] = {0.0, 0.0};
  double fov_ = 0.0, half_cot_ = 0.0;                             // s, 1 / (2 tan(s / 2))
  int model_ = 0, n_coeffs_ = 1;                                  // XK_CAM_FOV; the count setDistortion was given
  double k_[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                       // the coefficients of models 1 and 2
  unsigned int width_ = 0, height_ = 0;
};
}  // namespace x
