// x::TrackManager's interface over the device-resident track store (xk_trk_tracks_*): one device call per frame, the own
// lists fetched on demand, everything a getter returns built from the result block and the lists entry.
#include "x/vio/resident_track_manager.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>
#include <string>

using namespace x;

static void check(xk_handle *h, int rc, const char *what) {
  if (rc != XK_OK) throw std::runtime_error(std::string(what) + ": " + xk_strerror(rc) + " (" + (h ? xk_last_error(h) : "") + ")");
}

ResidentTrackManager::ResidentTrackManager(xk_handle *xk, const Camera &camera, double min_baseline_x_n, double min_baseline_y_n, int max_tracks,
                                           bool multi_uav, unsigned int n_tiles_h, unsigned int n_tiles_w, int max_matches)
    : xk_(xk), camera_(camera), min_baseline_x_n_(min_baseline_x_n), min_baseline_y_n_(min_baseline_y_n), max_tracks_(max_tracks),
      max_matches_(max_matches), multi_uav_(multi_uav), tiles_h_(n_tiles_h), tiles_w_(n_tiles_w) {
  check(xk_, xk_trk_create(xk_, max_matches, camera.getFx(), camera.getFy(), camera.getCx(), camera.getCy(), camera.getS(), &trk_), "xk_trk_create");
  try {
    setup();
  } catch (...) {
    xk_trk_destroy(trk_);
    throw;
  }
}

ResidentTrackManager::~ResidentTrackManager() {
  if (own_trk_) xk_trk_destroy(trk_);
}

void ResidentTrackManager::setup() {
  check(xk_, xk_trk_tracks_setup(trk_, max_tracks_, (int)tiles_h_, (int)tiles_w_, (int)camera_.getWidth(), (int)camera_.getHeight(), min_baseline_x_n_,
                                 min_baseline_y_n_, multi_uav_ ? 1 : 0),
        "xk_trk_tracks_setup");
  n_lists_[0] = n_lists_[1] = n_lists_[2] = 0;
  invalidate();
}

void ResidentTrackManager::attach(Tracker &tracker) {
  if (trk_ == tracker.handle()) return;
  xk_trk *old = own_trk_ ? trk_ : nullptr;
  trk_ = tracker.handle();
  own_trk_ = false;
  max_matches_ = tracker.maxFeatures();
  if (old) xk_trk_destroy(old);
  setup();
  clear();
}

void ResidentTrackManager::clear() {
  check(xk_, xk_trk_tracks_clear(trk_), "xk_trk_tracks_clear");
  n_lists_[0] = n_lists_[1] = n_lists_[2] = 0;
  invalidate();
  lost_slam_idxs_.clear(); msckf_trks_n_.clear(); msckf_trks_short_n_.clear();
}

// One manage call.  matches: the host's list, or nullptr for the block the tracker's last frame left on the device.
void ResidentTrackManager::call(const MatchList *matches, const AttitudeList &cam_rots, size_t n_poses_max, size_t n_slam_features_max,
                                size_t min_track_length, std::vector<unsigned char> &claimed) {
  if (n_poses_max < 3) throw std::runtime_error("ResidentTrackManager::manageTracks: n_poses_max < 3");
  if (cam_rots.size() < 3 || cam_rots.size() > 64) throw std::runtime_error("ResidentTrackManager::manageTracks: 3 ... 64 camera attitudes");
  if (multi_uav_ && !opp_ids_) throw std::runtime_error("ResidentTrackManager::manageTracks: multi_uav without setOppUpgradesMSCKF");
  if (n_poses_max > (size_t)1 << 30 || n_slam_features_max > (size_t)1 << 30 || min_track_length > (size_t)1 << 30)
    throw std::runtime_error("ResidentTrackManager::manageTracks: a parameter beyond 2^30");
  const size_t n = matches ? matches->size() : (size_t)max_matches_;     // (frame-fed: the bound; the call knows the frame's count)
  if (n > (size_t)max_matches_) throw std::runtime_error("ResidentTrackManager::manageTracks: more matches than max_matches");
  c_quat_.clear();
  for (const Attitude &a : cam_rots) { c_quat_.push_back(a.ax); c_quat_.push_back(a.ay); c_quat_.push_back(a.az); c_quat_.push_back(a.aw); }
  if (matches) {
    c_prev_.resize(2 * n); c_cur_.resize(2 * n); c_dprev_.resize(2 * n); c_dcur_.resize(2 * n); c_score_.resize(n);
    for (size_t i = 0; i < n; ++i) {
      const Match &m = (*matches)[i];
      c_prev_[2 * i] = m.previous.getX(); c_prev_[2 * i + 1] = m.previous.getY();
      c_cur_[2 * i] = m.current.getX(); c_cur_[2 * i + 1] = m.current.getY();
      c_dprev_[2 * i] = m.previous.getXDist(); c_dprev_[2 * i + 1] = m.previous.getYDist();
      c_dcur_[2 * i] = m.current.getXDist(); c_dcur_[2 * i + 1] = m.current.getYDist();
      c_score_[i] = (int)m.current.getFastScore();
    }
  }
  // the output capacities by the bounds of include/xk.h
  const size_t P = (size_t)n_lists_[0] + (size_t)n_lists_[1], O = (size_t)n_lists_[2];
  const size_t entries = O + n + P, obs = (O + n) * cam_rots.size() + P * std::min<size_t>(n_poses_max, 64);
  o_lost_.resize(P + 1); o_ids_.resize(entries + 1); o_off_.resize(entries + 2); o_xy_.resize(2 * obs + 2);
  claimed.assign(n + 1, 0);
  xk_trk_tracks_out out{};
  out.cap_lost = (int)P; out.cap_entries = (int)entries; out.cap_obs = (int)obs;
  out.lost_slam_idxs = o_lost_.data(); out.claimed = claimed.data(); out.ids = o_ids_.data(); out.off = o_off_.data(); out.xy = o_xy_.data();
  c_ids_.clear();
  if (opp_ids_) for (uniqueId id : *opp_ids_) c_ids_.push_back((long long)id);
  c_ids_.push_back(0);
  int n_ids = opp_ids_ ? (int)opp_ids_->size() : 0;
  int *n_ids_p = opp_ids_ ? &n_ids : nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = matches ? xk_trk_tracks_manage(trk_, c_prev_.data(), c_cur_.data(), c_dprev_.data(), c_dcur_.data(), c_score_.data(), (int)n,
                                                c_quat_.data(), (int)cam_rots.size(), (int)n_poses_max, (int)n_slam_features_max, (int)min_track_length,
                                                c_ids_.data(), n_ids_p, &out)
                         : xk_trk_tracks_manage_frame(trk_, c_quat_.data(), (int)cam_rots.size(), (int)n_poses_max, (int)n_slam_features_max,
                                                      (int)min_track_length, c_ids_.data(), n_ids_p, &out);
  device_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  check(xk_, rc, matches ? "xk_trk_tracks_manage" : "xk_trk_tracks_manage_frame");
  if (opp_ids_ && multi_uav_) opp_ids_->clear();                  // consumed (track_manager.cpp:355)
  n_poses_max_ = n_poses_max;
  n_lists_[0] = out.n_persistent; n_lists_[1] = out.n_new_persistent; n_lists_[2] = out.n_opportunistic;
  n_candidates_ = out.n_candidates; n_candidate_obs_ = out.n_candidate_obs;
  invalidate();
  lost_slam_idxs_.assign(o_lost_.begin(), o_lost_.begin() + out.n_lost);
  TrackList *lists[4] = {&msckf_trks_n_, &msckf_trks_short_n_, &new_slam_std_trks_n_, &new_slam_msckf_trks_n_};
  size_t e = 0;
  for (int l = 0; l < 4; ++l) {
    lists[l]->clear();
    for (int k = 0; k < out.n_list[l]; ++k, ++e) {
      Track t;
      t.setId((uniqueId)o_ids_[e]);
      for (int i = o_off_[e]; i < o_off_[e + 1]; ++i) t.emplace_back(o_xy_[2 * (size_t)i], o_xy_[2 * (size_t)i + 1]);
      lists[l]->push_back(std::move(t));
    }
  }
}

void ResidentTrackManager::manageTracks(MatchList &matches, const AttitudeList &cam_rots, size_t n_poses_max, size_t n_slam_features_max,
                                        size_t min_track_length, TileGrid &grid) {
  if (grid.getNTilesH() != tiles_h_ || grid.getNTilesW() != tiles_w_)
    throw std::runtime_error("ResidentTrackManager::manageTracks: the grid's tile counts are not the store's");
  std::vector<unsigned char> claimed;
  call(&matches, cam_rots, n_poses_max, n_slam_features_max, min_track_length, claimed);
  size_t kept = 0;                                                  // a claimed match leaves the list, the rest keep their order
  for (size_t m = 0; m < matches.size(); ++m)
    if (!claimed[m]) {
      if (kept != m) matches[kept] = std::move(matches[m]);
      ++kept;
    }
  matches.resize(kept);
}

std::vector<unsigned char> ResidentTrackManager::manageFrame(Tracker &tracker, const AttitudeList &cam_rots, size_t n_poses_max,
                                                             size_t n_slam_features_max, size_t min_track_length) {
  attach(tracker);
  std::vector<unsigned char> claimed;
  call(nullptr, cam_rots, n_poses_max, n_slam_features_max, min_track_length, claimed);
  claimed.resize((size_t)std::max(tracker.counts().n_matches, 0));
  return claimed;
}

const TrackedTrackList &ResidentTrackManager::list(int which) const {
  Cached &c = cache_[which];
  if (c.valid) return c.tracks;
  const size_t cap = (size_t)std::max(n_lists_[which], 1);
  std::vector<long long> ids(cap);
  std::vector<int> lengths(cap), score(cap * 64), tiles(cap * 128);
  std::vector<double> obs(cap * 256);
  int n = 0;
  check(xk_, xk_trk_tracks_lists(trk_, which, ids.data(), lengths.data(), obs.data(), score.data(), tiles.data(), &n), "xk_trk_tracks_lists");
  c.tracks.clear();
  c.lengths.assign(lengths.begin(), lengths.begin() + n);
  for (int t = 0; t < n; ++t) {
    TrackedTrack trk;
    trk.setId((uniqueId)ids[(size_t)t]);
    const int cnt = std::min(lengths[(size_t)t], 64);
    for (int i = 0; i < cnt; ++i) {
      const size_t at = (size_t)t * 64 + (size_t)i;
      TrackedFeature f(obs[4 * at], obs[4 * at + 1], obs[4 * at + 2], obs[4 * at + 3]);
      f.setFastScore((double)score[at]);
      f.setTile(tiles[2 * at], tiles[2 * at + 1]);
      trk.push_back(f);
    }
    c.tracks.push_back(std::move(trk));
  }
  c.valid = true;
  return c.tracks;
}

Track ResidentTrackManager::normalizeHost(const TrackedTrack &trk, size_t max_size) const {
  const size_t skip = (max_size != 0 && trk.size() > max_size) ? trk.size() - max_size : 0;
  Track out;
  out.setId(trk.getId());
  out.reserve(trk.size() - skip);
  for (size_t i = skip; i < trk.size(); ++i) out.push_back(camera_.normalize(static_cast<const Feature &>(trk[i])));
  return out;
}

TrackList ResidentTrackManager::normalizeSlamTracks(int size_out) const {
  TrackList out;
  for (const TrackedTrack &t : list(0)) out.push_back(normalizeHost(t, (size_t)size_out));
  return out;
}

TrackList ResidentTrackManager::getOppTracks() const {
  TrackList out;
  const TrackedTrackList &opp = list(2);
  for (const TrackedTrack &t : opp) out.push_back(normalizeHost(t, opp.size()));
  return out;
}

std::vector<Feature> ResidentTrackManager::getOppFeatures() const {
  std::vector<Feature> out;
  for (const TrackedTrack &t : list(2))
    if (!t.empty()) out.push_back(camera_.normalize(static_cast<const Feature &>(t.back())));
  return out;
}

TrackedTrackList ResidentTrackManager::getMostPromisingTracks(int k) const {
  TrackedTrackList tmp = list(0);
  std::stable_sort(tmp.begin(), tmp.end(), [](const TrackedTrack &a, const TrackedTrack &b) { return a.back().getFastScore() > b.back().getFastScore(); });
  if (k >= 0 && tmp.size() >= (size_t)k) tmp.resize((size_t)k);
  return tmp;
}

void ResidentTrackManager::removePersistentTracksAtIndex(unsigned int idx) {
  check(xk_, xk_trk_tracks_remove_persistent(trk_, idx), "xk_trk_tracks_remove_persistent");
  n_lists_[0] -= 1;
  invalidate();
}

void ResidentTrackManager::removeNewPersistentTracksAtIndexes(const std::vector<unsigned int> &invalid_tracks_idx) {
  check(xk_, xk_trk_tracks_remove_new_persistent(trk_, invalid_tracks_idx.data(), (int)invalid_tracks_idx.size()), "xk_trk_tracks_remove_new_persistent");
  n_lists_[1] -= (int)invalid_tracks_idx.size();
  invalidate();
}

void ResidentTrackManager::fill(VioMeasurement &m) const {
  m.slam_tracks = normalizeSlamTracks((int)n_poses_max_);     // vio_updater.cpp:172-179
  m.msckf_tracks = msckf_trks_n_;
  m.msckf_short_tracks = msckf_trks_short_n_;
  m.new_slam_std_tracks = new_slam_std_trks_n_;
  m.new_msckf_slam_tracks = new_slam_msckf_trks_n_;
  m.lost_slam_track_idxs = lost_slam_idxs_;
}

std::vector<int> ResidentTrackManager::featureTriangleAtPoint(const TrackedFeature &lrf_img_pt, unsigned int width, unsigned int height) const {
  std::vector<TrackedFeature> newest;
  for (const TrackedTrack &t : list(0)) newest.push_back(t.back());
  return x::featureTriangleAtPoint(newest, lrf_img_pt, width, height);
}
