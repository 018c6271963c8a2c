// track_manager_run.h -- the body of the two track manager examples: x::TrackManager (track_manager_main.cpp, the host walk) and
// x::ResidentTrackManager (resident_tracks_main.cpp, the tracks on the device) have one interface, so one run serves both.  The case
// file, the modes and the output are described in track_manager_main.cpp.  make(xk, camera, min_baseline_x_n, min_baseline_y_n,
// max_tracks, multi_uav, tiles_h, tiles_w) -> std::unique_ptr<Manager>.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <optional>

#include "x/ekf/ekf.h"
#include "x/vio/track_manager.h"

using namespace x;

static inline void print_tracks(const char *name, const TrackList &tracks) {
  for (const Track &t : tracks) {
    std::printf("T %s %llu %zu", name, t.getId(), t.size());
    for (const Feature &f : t) std::printf(" %.17g %.17g", f.getX(), f.getY());
    std::printf("\n");
  }
}

static inline void print_ids(const char *name, const TrackList &tracks) {
  std::printf("M %s", name);
  for (const Track &t : tracks) std::printf(" %llu", t.getId());
  std::printf("\n");
}

struct FrameIn {
  MatchList matches;
  AttitudeList cam_rots;
  OppIDList ids;
  double px = 0, py = 0;
};

// The scripted motion: position p = v t, attitude a turn of yaw_rate t about y (camera-to-global, Hamilton), the IMU in the camera.
struct Motion {
  double dt = 0, v[3] = {0, 0, 0}, yaw_rate = 0, sigma_img = 0;
  int imu_per_frame = 0;
  Quaternion attitude(double t) const { return Quaternion(std::cos(0.5 * yaw_rate * t), 0.0, std::sin(0.5 * yaw_rate * t), 0.0); }
  Vector3 gyro() const { return Vector3(0.0, yaw_rate, 0.0); }
  Vector3 accel(double t, const Vector3 &g) const {      // constant velocity: the specific force is C(q)^T (-g)
    double r[9];
    attitude(t).toRotationMatrix(r);
    return Vector3(-(r[0] * g(0) + r[3] * g(1) + r[6] * g(2)), -(r[1] * g(0) + r[4] * g(1) + r[7] * g(2)),
                   -(r[2] * g(0) + r[5] * g(1) + r[8] * g(2)));
  }
};

static inline bool all_finite(const Matrix &m) {
  for (size_t i = 0; i < m.size(); ++i)
    if (!std::isfinite(m.data()[i])) return false;
  return true;
}

template <class Manager, class Make>
int track_manager_run(int argc, char **argv, Make make) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s case.txt [update]\n", argv[0]); return 2; }
  const bool update = argc > 2 && std::strcmp(argv[2], "update") == 0;
  std::ifstream in(argv[1]);
  double fx, fy, cx, cy, s, min_bx, min_by;
  unsigned int width, height, tiles_h, tiles_w;
  int max_tracks, multi_uav, n_frames;
  size_t n_poses_max, n_slam_max, min_track_length;
  in >> fx >> fy >> cx >> cy >> s >> width >> height >> min_bx >> min_by >> max_tracks >> multi_uav >> n_poses_max >> n_slam_max >>
      min_track_length >> tiles_h >> tiles_w >> n_frames;
  if (!in || n_frames < 0) { std::fprintf(stderr, "bad case file\n"); return 2; }
  std::vector<FrameIn> frames((size_t)n_frames);
  for (FrameIn &fr : frames) {
    int n_matches, n_quats, n_ids;
    in >> n_matches >> n_quats >> n_ids >> fr.px >> fr.py;
    if (!in || n_matches < 0 || n_quats < 0 || n_ids < 0) { std::fprintf(stderr, "bad frame header\n"); return 2; }
    fr.matches.resize((size_t)n_matches);
    for (Match &m : fr.matches) {
      double v[9];
      for (double &d : v) in >> d;
      m.previous = TrackedFeature(v[0], v[1], v[2], v[3]);
      m.current = TrackedFeature(v[4], v[5], v[6], v[7]);
      m.previous.setFastScore(v[8]);
      m.current.setFastScore(v[8]);
    }
    fr.cam_rots.resize((size_t)n_quats);
    for (Attitude &a : fr.cam_rots) in >> a.ax >> a.ay >> a.az >> a.aw;
    for (int i = 0; i < n_ids; ++i) { uniqueId id; in >> id; fr.ids.push_back(id); }
    if (!in) { std::fprintf(stderr, "bad frame\n"); return 2; }
  }
  Motion mo;
  if (update) {
    in >> mo.dt >> mo.v[0] >> mo.v[1] >> mo.v[2] >> mo.yaw_rate >> mo.sigma_img >> mo.imu_per_frame;
    if (!in || !(mo.dt > 0) || mo.imu_per_frame < 1 || !(mo.sigma_img > 0)) { std::fprintf(stderr, "bad motion line\n"); return 2; }
    if (multi_uav) { std::fprintf(stderr, "update runs the single-agent order\n"); return 2; }
  }
  const Camera camera(fx, fy, cx, cy, s, width, height);
  const int N = (int)n_poses_max, M = (int)n_slam_max;
  int rc = 0;
  try {
    // the handle: the updater's in the end-to-end run (one engine serves the filter and the manager), a plain one otherwise
    std::unique_ptr<VioUpdater> updater;
    xk_handle *xk = nullptr;
    if (update) {
      updater.reset(new VioUpdater(0, N, M, max_tracks, mo.sigma_img));
      updater->setManageWindow(true);
      updater->setWindow(0, {}, false);                       // an empty window: every frame's manage() adds its pose
      xk = updater->engine();
    } else if (xk_create(0, 4, 0, 4, &xk) != XK_OK) {
      std::fprintf(stderr, "xk_create failed\n");
      return 1;
    }
    {
      std::unique_ptr<Manager> manager_p = make(xk, camera, min_bx, min_by, max_tracks, multi_uav != 0, tiles_h, tiles_w);
      Manager &manager = *manager_p;
      TileGrid grid(width, height, tiles_h, tiles_w, 0);
      OppIDListPtr opp_ids = std::make_shared<OppIDList>();
      if (multi_uav) manager.setOppUpgradesMSCKF(opp_ids);

      const Vector3 g(0, 0, -9.81);
      Propagator prop(g, ImuNoise());
      std::unique_ptr<Ekf> ekf;
      const double t0 = 10.0, dt_imu = update ? mo.dt / mo.imu_per_frame : 0.0;
      unsigned int seq = 0;
      if (update) {
        Propagator::acknowledgeModelProcessNoise();           // (the mirror's clean process-noise model, knowingly)
        prop.setEngine(xk);
        ekf.reset(new Ekf(*updater));
        ekf->set(4 * mo.imu_per_frame + 8, State(N, M), &prop, 0.5 * dt_imu);
        State init(N, M);
        init.setTime(t0);
        init.p_ = Vector3(0, 0, 0);
        init.v_ = Vector3(mo.v[0], mo.v[1], mo.v[2]);
        init.q_ = mo.attitude(0.0);
        init.q_ic_ = Quaternion(1, 0, 0, 0);
        const int n = init.nErrorStates();
        init.cov_ = Matrix::Zero(n, n);
        for (int i = 0; i < n; ++i) init.cov_(i, i) = 1e-4;   // 1 cm, 0.01 rad; the window and feature blocks are written by manage / postUpdate
        for (int i = 0; i < 3; ++i) { init.cov_(kIdxV + i, kIdxV + i) = 1e-2; init.cov_(kIdxBw + i, kIdxBw + i) = 1e-6; }
        ekf->initializeFromState(init);
        ekf->processImu(t0, seq++, mo.gyro(), mo.accel(0.0, g));     // first message: stand-by -> initialised
        VioMeasurement none;                                         // camera frame 0: no matches yet, its pose enters the window
        none.timestamp = t0;
        updater->setMeasurement(none);
        if (!ekf->processUpdateMeasurement()) throw std::runtime_error("camera frame 0 was not processed");
      }

      for (int f = 0; f < n_frames; ++f) {
        FrameIn &fr = frames[(size_t)f];
        MatchList matches = fr.matches;
        AttitudeList cam_rots = fr.cam_rots;
        *opp_ids = fr.ids;
        const double t_frame = t0 + (f + 1) * mo.dt;
        if (update) {
          for (int i = 1; i <= mo.imu_per_frame; ++i) {
            const double t = (f * mo.imu_per_frame + i) * dt_imu;
            ekf->processImu(t0 + t, seq++, mo.gyro(), mo.accel(t, g));
          }
          // vio_updater.cpp:143-153: the newest n_poses_max - 1 attitudes of the window (it has not slid yet), then the current one;
          // while the window fills, the oldest one stands in for the missing entries
          const State &tail = ekf->tail();
          const int np = updater->stateManager().getNPoses();
          const Matrix &qa = tail.getOrientationArray();
          cam_rots.clear();
          for (int k = N - 1; k >= 1; --k) {
            const int i = std::max(np - k, 0);
            cam_rots.push_back(Attitude{qa(4 * i), qa(4 * i + 1), qa(4 * i + 2), qa(4 * i + 3)});
          }
          cam_rots.push_back(tail.computeCameraAttitude());
        }
        const auto c0 = std::chrono::steady_clock::now();
        manager.manageTracks(matches, cam_rots, n_poses_max, n_slam_max, min_track_length, grid);
        const double total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
        std::printf("F %d %.4f %.4f %zu %d %d\nL", f, manager.lastDeviceCallMs(), total_ms, fr.matches.size(), manager.lastCandidateCount(),
                    manager.lastCandidateObservations());
        for (unsigned int i : manager.getLostSlamTrackIndexes()) std::printf(" %u", i);
        std::printf("\n");
        print_tracks("msckf", manager.getMsckfTracks());
        print_tracks("short", manager.getShortMsckfTracks());
        print_tracks("new_std", manager.getNewSlamStdTracks());
        print_tracks("new_msckf", manager.getNewSlamMsckfTracks());
        print_tracks("slam", manager.normalizeSlamTracks((int)n_poses_max));
        print_tracks("opp", manager.getOppTracks());
        std::printf("S");
        for (const TrackedTrack &t : manager.persistentTracks()) std::printf(" %llu", t.getId());
        std::printf(" |");
        for (const TrackedTrack &t : manager.newPersistentTracks()) std::printf(" %llu", t.getId());
        std::printf("\nO");
        for (const TrackedTrack &t : manager.opportunisticTracks()) std::printf(" %llu:%zu", t.getId(), t.size());
        std::printf("\nP");
        for (const TrackedTrack &t : manager.getMostPromisingTracks(3)) std::printf(" %llu", t.getId());
        std::printf("\nA");
        for (int i : manager.featureTriangleAtPoint(TrackedFeature(0.0, 0.0, fr.px, fr.py), width, height)) std::printf(" %d", i);
        std::printf("\nG");
        for (const Feature &ft : manager.getOppFeatures()) std::printf(" %.17g %.17g", ft.getX(), ft.getY());
        std::printf("\n");
        VioMeasurement meas;
        manager.fill(meas);
        print_ids("slam", meas.slam_tracks);
        print_ids("msckf", meas.msckf_tracks);
        print_ids("short", meas.msckf_short_tracks);
        print_ids("new_msckf", meas.new_msckf_slam_tracks);
        print_ids("new_std", meas.new_slam_std_tracks);
        std::printf("M lost");
        for (unsigned int i : meas.lost_slam_track_idxs) std::printf(" %u", i);
        std::printf("\n");
        if (update) {
          meas.timestamp = t_frame;
          const size_t given = meas.msckf_tracks.size(), given_short = meas.msckf_short_tracks.size();
          const bool requested = !(meas.msckf_tracks.empty() && meas.slam_tracks.empty() && meas.new_slam_std_tracks.empty() &&
                                   meas.new_msckf_slam_tracks.empty());
          updater->setMeasurement(std::move(meas));
          const std::optional<State> post = ekf->processUpdateMeasurement();
          // what the main update staged: its gate flags, one per MSCKF track (none if this frame asked for no update)
          const size_t consumed = requested ? updater->getMsckfInlierFlags().size() : 0;
          int inliers = 0;
          if (requested) for (int v : updater->getMsckfInlierFlags()) inliers += v;
          int finite = 0;                                     // bits: covariance, position, attitude and feature arrays, core states
          double asym = -1.0, perr = -1.0;
          if (post) {
            const State &st = *post;
            double dyn[16];
            st.getDynamicStates(dyn);
            bool core = true;
            for (double d : dyn) core = core && std::isfinite(d);
            finite = (all_finite(st.cov_) ? 1 : 0) | (all_finite(st.p_array_) ? 2 : 0) | (all_finite(st.q_array_) ? 4 : 0) |
                     (all_finite(st.f_array_) ? 8 : 0) | (core ? 16 : 0);
            for (size_t i = 0; i < st.cov_.size() && !(finite & 1); ++i)
              if (!std::isfinite(st.cov_.data()[i])) {
                std::fprintf(stderr, "frame %d: covariance entry (%zu, %zu) of %d is %g\n", f, i % (size_t)st.cov_.rows(), i / (size_t)st.cov_.rows(),
                             st.cov_.rows(), st.cov_.data()[i]);
                break;
              }
            asym = 0.0;
            for (int i = 0; i < st.cov_.rows(); ++i)
              for (int j = 0; j < i; ++j) asym = std::max(asym, std::abs(st.cov_(i, j) - st.cov_(j, i)));
            const double tt = (f + 1) * mo.dt;
            perr = std::sqrt(std::pow(st.p_(0) - mo.v[0] * tt, 2) + std::pow(st.p_(1) - mo.v[1] * tt, 2) + std::pow(st.p_(2) - mo.v[2] * tt, 2));
          }
          std::printf("U %d %d %d %d %zu %zu %d %zu %d %.3e %.3e\n", f, post ? 1 : 0, updater->stateManager().getNPoses(),
                      updater->stateManager().getNFeatures(), given, consumed, inliers, given_short, finite, asym, perr);
        }
      }
      if (!update) {
        // the removal calls a caller makes when the update rejects a feature (vio_updater.cpp), and clear()
        size_t after_remove = 0, after_remove_new = 0;
        if (!manager.persistentTracks().empty()) manager.removePersistentTracksAtIndex(0);
        after_remove = manager.persistentTracks().size();
        if (!manager.newPersistentTracks().empty()) manager.removeNewPersistentTracksAtIndexes({0});
        after_remove_new = manager.newPersistentTracks().size();
        manager.clear();
        std::printf("R %zu %zu %zu\n", after_remove, after_remove_new,
                    manager.persistentTracks().size() + manager.newPersistentTracks().size() + manager.opportunisticTracks().size() +
                        manager.getMsckfTracks().size() + manager.getShortMsckfTracks().size() + manager.getLostSlamTrackIndexes().size());
      }
    }
    if (!update) xk_destroy(xk);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  return rc;
}
