// x/vio/track_manager.h -- mirror of x::TrackManager (include/x/vio/track_manager.h, src/x/vio/track_manager.cpp): the link between
// the tracker's matches and the update's track lists.  manageTracks (track_manager.cpp:115-432) associates a frame's matches with the
// live tracks, extends the persistent (SLAM) and the opportunistic tracks, promotes tracks to SLAM features under the per-tile
// balancing rule, turns over-long and just-ended tracks into MSCKF measurements and reports the persistent features that
// StateManager::manage must drop.  Its outputs are the track and index fields of x::VioMeasurement (fill()).
//
// The list walk is host code here as it is there.  Its numerical part -- Camera::normalize and checkBaseline (:576-636) of every track
// that may become a measurement -- does not depend on where the walk stands, so ONE xk_trk_baseline call per frame, made after the
// association, computes it for all candidates on the GPU; the walk reads the flags and takes its normalised tracks from
// that call's output.  There is no CPU fallback.
//
// Where this differs from the reference, on purpose:
//   - the opportunistic tracks are sorted by length with std::stable_sort: the reference's std::sort leaves the order among equal
//     lengths unspecified, here it is the order in which the matches arrived;
//   - track ids come from a per-manager counter from 1, given when an opportunistic track is created and kept through promotion and
//     normalisation (the reference's process-wide counter also counts temporaries: only uniqueness carries over);
//   - MULTI_UAV is a run-time flag, as elsewhere in the mirror;
//   - plotting is left out.
// The association is by Feature::operator== on the undistorted pixels (feature.cpp:47-68: a relative test at machine epsilon, not bit
// equality); the first equal item in list order wins.  The lookup goes through a list sorted by x, searched in the few-ulp
// neighbourhood; its result is the quadratic scan's.
#pragma once
#include <memory>
#include <vector>

#include "x/vio/vio_updater.h"
#include "x/vision/camera.h"
#include "x/vision/feature_tracker.h"
#include "xk.h"

namespace x {
// A track as the manager holds it: TrackedFeatures (the distorted pixels, FAST score and tile are needed), the id, and for the length
// of one manageTracks call its row in the frame's baseline batch.
class TrackedTrack : public std::vector<TrackedFeature> {
 public:
  using std::vector<TrackedFeature>::vector;
  TrackedTrack() = default;
  uniqueId getId() const { return id_; }
  void setId(uniqueId id) { id_ = id; }
  int candidate = -1;
 private:
  uniqueId id_ = 0;
};
using TrackedTrackList = std::vector<TrackedTrack>;
using OppIDList = std::vector<uniqueId>;
using OppIDListPtr = std::shared_ptr<OppIDList>;

// TrackManager::featureTriangleAtPoint on the persistent tracks' newest features (below): the search itself, shared with
// x::ResidentTrackManager, whose tracks live on the device.
std::vector<int> featureTriangleAtPoint(const std::vector<TrackedFeature> &newest, const TrackedFeature &lrf_img_pt, unsigned int width,
                                        unsigned int height);

class TrackManager {
 public:
  // max_tracks (1 ... 2^20): the most candidate tracks of one frame.  manageTracks refuses a frame, before it changes anything, whose
  // opportunistic tracks (each dies or goes on: a candidate either way) plus, with min_track_length <= 2, its matches exceed it
  static constexpr int kMaxTracks = 1 << 20, kMaxObs = 64;
  TrackManager(xk_handle *xk, const Camera &camera, double min_baseline_x_n, double min_baseline_y_n, int max_tracks, bool multi_uav = false);
  ~TrackManager();
  TrackManager(const TrackManager &) = delete;
  TrackManager &operator=(const TrackManager &) = delete;

  // matches: the frame's matches, undistorted pixels in getX / getY (descending FAST order, as the tracker leaves them); the ones a
  // persistent track claims are erased.  cam_rots: the window's camera attitudes with the current one last (3 ... 64 entries).
  // n_poses_max >= 3.  Throws std::runtime_error on a frame it cannot take (those limits, a match outside the tile grid, too many
  // candidates) BEFORE any list changes; an error of the device call itself leaves the lists of this frame half-built: clear() then.
  void manageTracks(MatchList &matches, const AttitudeList &cam_rots, size_t n_poses_max, size_t n_slam_features_max, size_t min_track_length,
                    TileGrid &grid);

  TrackList getMsckfTracks() const { return msckf_trks_n_; }
  TrackList getShortMsckfTracks() const { return msckf_trks_short_n_; }
  TrackList getNewSlamStdTracks() const { return new_slam_std_trks_n_; }
  TrackList getNewSlamMsckfTracks() const { return new_slam_msckf_trks_n_; }
  TrackList normalizeSlamTracks(int size_out) const;
  TrackList getOppTracks() const;                       // cropped to the LIST's size, as the reference has it (:60)
  std::vector<Feature> getOppFeatures() const;          // the newest observation of every opportunistic track, normalised (:64-71)
  std::vector<unsigned int> getLostSlamTrackIndexes() const { return lost_slam_idxs_; }
  TrackedTrackList getMostPromisingTracks(int k) const; // the k persistent tracks of the highest FAST score (:103-113; stable here)
  void removePersistentTracksAtIndex(unsigned int idx);
  void removeNewPersistentTracksAtIndexes(const std::vector<unsigned int> &invalid_tracks_idx);   // increasing order
  void setOppUpgradesMSCKF(const OppIDListPtr &opp_ids) { opp_ids_ = opp_ids; }   // multi_uav: consumed and cleared by manageTracks
  void clear();
  // the six track and index fields, in the order VioUpdater::preProcess reads them (vio_updater.cpp:172-179); the persistent tracks
  // are cropped to the n_poses_max of the last manageTracks
  void fill(VioMeasurement &m) const;

  // TrackManager::featureTriangleAtPoint (:443-544) by the project's definition: the Delaunay triangle of the persistent
  // tracks' newest distorted pixels (rounded to float, plus the three outer vertices of cv::Subdiv2D around Rect(-1, -1, w + 2, h + 2))
  // whose closed area contains the point (getXDist / getYDist, rounded to float) and whose circumcircle is empty -> the three
  // track indices, ascending; empty if that triangle uses an outer vertex, with fewer than 3 tracks, or for a point outside the
  // rectangle.  Several qualifying triangles (a set of measure zero): the lexicographically smallest.  Plain host code, fp64 predicates.
  std::vector<int> featureTriangleAtPoint(const TrackedFeature &lrf_img_pt, unsigned int width, unsigned int height) const;

  // the manager's own lists, for inspection
  const TrackedTrackList &persistentTracks() const { return slam_trks_; }
  const TrackedTrackList &newPersistentTracks() const { return new_slam_trks_; }
  const TrackedTrackList &opportunisticTracks() const { return opp_trks_; }
  int lastCandidateCount() const { return (int)b_drop_.size(); }    // tracks and observations of the last frame's batch
  int lastCandidateObservations() const { return (int)(b_obs_.size() / 2); }
  double lastDeviceCallMs() const { return device_ms_; }   // wall time of the last frame's xk_trk_baseline call (tools/bench_track_manager.py)

 private:
  Track normalizedCandidate(const TrackedTrack &trk) const;    // out of the frame's batch
  bool candidateFlag(const TrackedTrack &trk) const;
  int addCandidate(TrackedTrack &trk, bool drop_last);
  void runBatch(const AttitudeList &cam_rots);
  Track normalizeHost(const TrackedTrack &trk, size_t max_size) const;

  xk_handle *xk_;
  xk_trk *trk_ = nullptr;
  Camera camera_;
  double min_baseline_x_n_, min_baseline_y_n_;
  int max_tracks_;
  bool multi_uav_;
  size_t n_poses_max_ = 0;
  uniqueId next_id_ = 1;
  OppIDListPtr opp_ids_;
  TrackedTrackList slam_trks_, new_slam_trks_, opp_trks_;
  TrackList msckf_trks_n_, msckf_trks_short_n_, new_slam_std_trks_n_, new_slam_msckf_trks_n_;
  std::vector<unsigned int> lost_slam_idxs_;
  // the frame's batch: CSR in, what xk_trk_baseline returns out
  std::vector<int> b_off_, b_norm_off_;
  std::vector<double> b_obs_, b_quat_, b_norm_, b_delta_;
  std::vector<unsigned char> b_drop_, b_flag_;
  double device_ms_ = 0.0;
};
}  // namespace x
