// x/vio/resident_track_manager.h -- x::TrackManager's interface over the track store that stays on the device (xk_trk_tracks_*,
// include/xk.h).  manageTracks is ONE device call per frame: the association, the rebuild of the opportunistic tracks, the
// baseline batch, the dead-track pass, the promotion walk and the MSCKF-SLAM / standard split all run there, and the tracks live in device
// memory from frame to frame.  What this class holds on the host is the last call's result block (the four measurement lists, the lost
// indices) and, fetched on demand through xk_trk_tracks_lists, a copy of the store's own three lists.  There is no CPU fallback.
//
// manageFrame is the same step fed from the block the tracker's last frame left on the device: no match goes up.  It works on the
// x::Tracker's own xk_trk, where that block lies; the store is set up there on the first call (or by attach), and a manager that has
// started on one xk_trk stays on it.
//
// Where it differs from x::TrackManager, on purpose:
//   - the tile grid is fixed at construction (the store bins on the device); manageTracks refuses a TileGrid of other tile counts;
//   - the store keeps a track's newest 64 observations: a TrackedTrack of the own lists holds those, trueLength() says how long the
//     track is; the persistent measurement list is cropped to min(n_poses_max, 64);
//   - a previous feature's tile is computed from its distorted pixels, the FAST score is kept as the tracker's int;
//   - min_track_length must lie in 1 ... n_poses_max.
// Everything else -- ids, order, lengths, lost indices, every coordinate bit for bit -- equals x::TrackManager.
#pragma once
#include <vector>

#include "x/vio/track_manager.h"
#include "x/vision/tracker.h"

namespace x {
class ResidentTrackManager {
 public:
  // max_tracks (1 ... 2^20): the store's slots.  max_matches: the most matches of a frame.  The grid is TiledImage's of the camera's image.
  ResidentTrackManager(xk_handle *xk, const Camera &camera, double min_baseline_x_n, double min_baseline_y_n, int max_tracks, bool multi_uav,
                       unsigned int n_tiles_h, unsigned int n_tiles_w, int max_matches = 1024);
  ~ResidentTrackManager();
  ResidentTrackManager(const ResidentTrackManager &) = delete;
  ResidentTrackManager &operator=(const ResidentTrackManager &) = delete;

  // As x::TrackManager::manageTracks; the matches a persistent track claims are erased.  Throws std::runtime_error on a frame it
  // cannot take (the limits, a match outside the tile grid, over max_tracks): the store is then what it was.
  void manageTracks(MatchList &matches, const AttitudeList &cam_rots, size_t n_poses_max, size_t n_slam_features_max, size_t min_track_length,
                    TileGrid &grid);
  // The same on the matches of tracker's last frame, which never leave the device.  Returns that frame's `claimed` flags (1: a
  // persistent track took the match), for a caller that keeps the match list.
  std::vector<unsigned char> manageFrame(Tracker &tracker, const AttitudeList &cam_rots, size_t n_poses_max, size_t n_slam_features_max,
                                         size_t min_track_length);
  void attach(Tracker &tracker);                        // the store moves to the tracker's xk_trk (empty, ids from 1)

  TrackList getMsckfTracks() const { return msckf_trks_n_; }
  TrackList getShortMsckfTracks() const { return msckf_trks_short_n_; }
  TrackList getNewSlamStdTracks() const { return new_slam_std_trks_n_; }
  TrackList getNewSlamMsckfTracks() const { return new_slam_msckf_trks_n_; }
  TrackList normalizeSlamTracks(int size_out) const;
  TrackList getOppTracks() const;                       // cropped to the LIST's size, as the reference has it (:60)
  std::vector<Feature> getOppFeatures() const;
  std::vector<unsigned int> getLostSlamTrackIndexes() const { return lost_slam_idxs_; }
  TrackedTrackList getMostPromisingTracks(int k) const;
  void removePersistentTracksAtIndex(unsigned int idx);
  void removeNewPersistentTracksAtIndexes(const std::vector<unsigned int> &invalid_tracks_idx);   // increasing order
  void setOppUpgradesMSCKF(const OppIDListPtr &opp_ids) { opp_ids_ = opp_ids; }   // multi_uav: consumed and cleared by manageTracks
  void clear();
  void fill(VioMeasurement &m) const;
  std::vector<int> featureTriangleAtPoint(const TrackedFeature &lrf_img_pt, unsigned int width, unsigned int height) const;

  // the store's own lists as the device holds them (the newest 64 observations of each track), and their true lengths
  const TrackedTrackList &persistentTracks() const { return list(0); }
  const TrackedTrackList &newPersistentTracks() const { return list(1); }
  const TrackedTrackList &opportunisticTracks() const { return list(2); }
  const std::vector<int> &trueLengths(int which) const { list(which); return cache_[which].lengths; }
  int lastCandidateCount() const { return n_candidates_; }
  int lastCandidateObservations() const { return n_candidate_obs_; }
  double lastDeviceCallMs() const { return device_ms_; }   // wall time of the last frame's device call: all of manageTracks but the host copies

 private:
  struct Cached {
    bool valid = false;
    TrackedTrackList tracks;
    std::vector<int> lengths;
  };
  const TrackedTrackList &list(int which) const;
  void setup();
  void call(const MatchList *matches, const AttitudeList &cam_rots, size_t n_poses_max, size_t n_slam_features_max, size_t min_track_length,
            std::vector<unsigned char> &claimed);
  void invalidate() { for (Cached &c : cache_) c.valid = false; }
  Track normalizeHost(const TrackedTrack &trk, size_t max_size) const;

  xk_handle *xk_;
  xk_trk *trk_ = nullptr;
  bool own_trk_ = true;
  Camera camera_;
  double min_baseline_x_n_, min_baseline_y_n_;
  int max_tracks_, max_matches_;
  bool multi_uav_;
  unsigned int tiles_h_, tiles_w_;
  size_t n_poses_max_ = 0;
  int n_lists_[3] = {0, 0, 0};                          // the store's list lengths, from the last result block and the removals since
  OppIDListPtr opp_ids_;
  TrackList msckf_trks_n_, msckf_trks_short_n_, new_slam_std_trks_n_, new_slam_msckf_trks_n_;
  std::vector<unsigned int> lost_slam_idxs_;
  int n_candidates_ = 0, n_candidate_obs_ = 0;
  double device_ms_ = 0.0;
  mutable Cached cache_[3];
  // a call's columns and outputs, grown as needed
  std::vector<double> c_prev_, c_cur_, c_dprev_, c_dcur_, c_quat_, o_xy_;
  std::vector<int> c_score_, o_lost_, o_off_;
  std::vector<long long> o_ids_, c_ids_;
};
}  // namespace x
