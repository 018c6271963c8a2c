// Mirror of src/x/vio/track_manager.cpp: the list walk of manageTracks on the host, its normalisation and baseline checks in one
// xk_trk_baseline call per frame (libxk.so), the facet search as plain host code.
#include "x/vio/track_manager.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>

using namespace x;

static void check(xk_handle *h, int rc, const char *what) {
  if (rc != XK_OK) throw std::runtime_error(std::string(what) + ": " + xk_strerror(rc) + " (" + (h ? xk_last_error(h) : "") + ")");
}

// Feature::nearlyEqual (feature.cpp:51-68)
static bool nearlyEqual(double a, double b) {
  const double abs_a = std::abs(a), abs_b = std::abs(b), diff = std::abs(a - b);
  if (a == b) return true;
  if (a == 0 || b == 0 || (abs_a + abs_b < std::numeric_limits<double>::min()))
    return diff < (std::numeric_limits<double>::epsilon() * std::numeric_limits<double>::min());
  return diff / std::min(abs_a + abs_b, std::numeric_limits<double>::max()) < std::numeric_limits<double>::epsilon();
}
static bool sameFeature(const Feature &a, const Feature &b) { return nearlyEqual(a.getX(), b.getX()) && nearlyEqual(a.getY(), b.getY()); }

namespace {
// "The first item of a list, in list order, that equals this feature", without the quadratic scan: the items sorted by x, a query
// looks at those within a few ulp of its x (every item nearlyEqual accepts lies there: |a - b| < eps (|a| + |b|) bounds the
// difference by a little over 2 eps |a|) and takes the alive one of the lowest position that passes the test itself.  Items that leave
// the list are marked dead; the others keep their order.  An item with a NaN x equals nothing and stays out; an infinite x equals only
// the same infinity (the test's a == b shortcut) and has no neighbourhood to search: those few items are kept in a list of their
// own and scanned in order.
class FirstEqual {
 public:
  template <class List, class Get>
  FirstEqual(const List &items, Get get) : alive_(items.size(), 1) {
    for (size_t i = 0; i < items.size(); ++i) {
      const Feature &f = get(items[i]);
      feats_.push_back(f);
      if (std::isfinite(f.getX())) by_x_.push_back({f.getX(), i});
      else if (std::isinf(f.getX())) infinite_.push_back(i);
    }
    std::sort(by_x_.begin(), by_x_.end());
  }
  long find(const Feature &q) const {
    const double x = q.getX();
    if (std::isnan(x)) return -1;
    if (std::isinf(x)) {
      for (size_t i : infinite_)                                   // in list order
        if (alive_[i] && sameFeature(q, feats_[i])) return (long)i;
      return -1;
    }
    const double w = 8.0 * std::numeric_limits<double>::epsilon() * std::abs(x) + 1e-300;
    long best = -1;
    for (auto it = std::lower_bound(by_x_.begin(), by_x_.end(), std::make_pair(x - w, (size_t)0)); it != by_x_.end() && it->first <= x + w; ++it)
      if (alive_[it->second] && (best < 0 || (long)it->second < best) && sameFeature(q, feats_[it->second])) best = (long)it->second;
    return best;
  }
  void remove(size_t i) { alive_[i] = 0; }
  bool alive(size_t i) const { return alive_[i] != 0; }

 private:
  std::vector<Feature> feats_;
  std::vector<std::pair<double, size_t>> by_x_;
  std::vector<size_t> infinite_;
  std::vector<unsigned char> alive_;
};
}  // namespace

TrackManager::TrackManager(xk_handle *xk, const Camera &camera, double min_baseline_x_n, double min_baseline_y_n, int max_tracks, bool multi_uav)
    : xk_(xk), camera_(camera), min_baseline_x_n_(min_baseline_x_n), min_baseline_y_n_(min_baseline_y_n), max_tracks_(max_tracks),
      multi_uav_(multi_uav) {
  if (max_tracks < 1 || max_tracks > kMaxTracks) throw std::runtime_error("TrackManager: max_tracks outside 1 ... 2^20");
  check(xk_, xk_trk_create(xk_, 1, camera.getFx(), camera.getFy(), camera.getCx(), camera.getCy(), camera.getS(), &trk_), "xk_trk_create");
  const int rc = xk_trk_baseline_setup(trk_, max_tracks, max_tracks * kMaxObs);   // a candidate goes up with its newest 64 observations at most (<= 2^26)
  if (rc != XK_OK) {
    xk_trk_destroy(trk_);
    check(xk_, rc, "xk_trk_baseline_setup");
  }
}                                                                                 // (the batch's host vectors grow with the frames)

TrackManager::~TrackManager() { xk_trk_destroy(trk_); }

void TrackManager::clear() {
  slam_trks_.clear(); new_slam_trks_.clear(); lost_slam_idxs_.clear(); opp_trks_.clear();
  msckf_trks_n_.clear(); msckf_trks_short_n_.clear();
}

Track TrackManager::normalizeHost(const TrackedTrack &trk, size_t max_size) const {
  const size_t skip = (max_size != 0 && trk.size() > max_size) ? trk.size() - max_size : 0;
  Track out;
  out.setId(trk.getId());
  out.reserve(trk.size() - skip);
  for (size_t i = skip; i < trk.size(); ++i) out.push_back(camera_.normalize(static_cast<const Feature &>(trk[i])));
  return out;
}

TrackList TrackManager::normalizeSlamTracks(int size_out) const {
  TrackList out;
  out.reserve(slam_trks_.size());
  for (const TrackedTrack &t : slam_trks_) out.push_back(normalizeHost(t, (size_t)size_out));
  return out;
}

TrackList TrackManager::getOppTracks() const {
  TrackList out;
  out.reserve(opp_trks_.size());
  for (const TrackedTrack &t : opp_trks_) out.push_back(normalizeHost(t, opp_trks_.size()));
  return out;
}

std::vector<Feature> TrackManager::getOppFeatures() const {
  std::vector<Feature> out;
  for (const TrackedTrack &t : opp_trks_)
    if (!t.empty()) out.push_back(camera_.normalize(static_cast<const Feature &>(t.back())));
  return out;
}

TrackedTrackList TrackManager::getMostPromisingTracks(int k) const {
  TrackedTrackList tmp = slam_trks_;
  std::stable_sort(tmp.begin(), tmp.end(), [](const TrackedTrack &a, const TrackedTrack &b) { return a.back().getFastScore() > b.back().getFastScore(); });
  if (k >= 0 && tmp.size() >= (size_t)k) tmp.resize((size_t)k);
  return tmp;
}

void TrackManager::removePersistentTracksAtIndex(unsigned int idx) {
  if (idx >= slam_trks_.size()) throw std::runtime_error("TrackManager::removePersistentTracksAtIndex: no such track");
  slam_trks_.erase(slam_trks_.begin() + idx);
}

void TrackManager::removeNewPersistentTracksAtIndexes(const std::vector<unsigned int> &invalid_tracks_idx) {
  for (size_t i = invalid_tracks_idx.size(); i; --i) {
    if (invalid_tracks_idx[i - 1] >= new_slam_trks_.size()) throw std::runtime_error("TrackManager::removeNewPersistentTracksAtIndexes: no such track");
    new_slam_trks_.erase(new_slam_trks_.begin() + invalid_tracks_idx[i - 1]);
  }
}

void TrackManager::fill(VioMeasurement &m) const {
  m.slam_tracks = normalizeSlamTracks((int)n_poses_max_);     // vio_updater.cpp:172-179
  m.msckf_tracks = msckf_trks_n_;
  m.msckf_short_tracks = msckf_trks_short_n_;
  m.new_slam_std_tracks = new_slam_std_trks_n_;
  m.new_msckf_slam_tracks = new_slam_msckf_trks_n_;
  m.lost_slam_track_idxs = lost_slam_idxs_;
}

// ---- the frame's batch ------------------------------------------------------------------------------------------------------------
int TrackManager::addCandidate(TrackedTrack &trk, bool drop_last) {
  const int k = (int)b_drop_.size();
  if (k >= max_tracks_) throw std::runtime_error("TrackManager::manageTracks: more candidate tracks than max_tracks");
  const size_t first = trk.size() > (size_t)kMaxObs ? trk.size() - (size_t)kMaxObs : 0;   // (the kernel keeps the newest min(length, list size <= 64) anyway)
  for (size_t i = first; i < trk.size(); ++i) { b_obs_.push_back(trk[i].getX()); b_obs_.push_back(trk[i].getY()); }
  b_off_.push_back((int)(b_obs_.size() / 2));
  b_drop_.push_back(drop_last ? 1 : 0);
  trk.candidate = k;
  return k;
}

void TrackManager::runBatch(const AttitudeList &cam_rots) {
  const int K = (int)b_drop_.size();
  device_ms_ = 0.0;
  if (K == 0) return;
  b_quat_.clear();
  b_norm_off_.resize((size_t)K + 1); b_norm_.resize(b_obs_.size()); b_delta_.resize(2 * (size_t)K); b_flag_.resize((size_t)K);
  for (const Attitude &a : cam_rots) { b_quat_.push_back(a.ax); b_quat_.push_back(a.ay); b_quat_.push_back(a.az); b_quat_.push_back(a.aw); }
  const auto t0 = std::chrono::steady_clock::now();
  check(xk_, xk_trk_baseline(trk_, b_off_.data(), b_obs_.data(), b_drop_.data(), K, b_quat_.data(), (int)cam_rots.size(), min_baseline_x_n_,
                             min_baseline_y_n_, b_norm_off_.data(), b_norm_.data(), b_delta_.data(), b_flag_.data()),
        "xk_trk_baseline");
  device_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

Track TrackManager::normalizedCandidate(const TrackedTrack &trk) const {
  if (trk.candidate < 0) throw std::logic_error("TrackManager: a track outside the frame's batch");
  Track out;
  out.setId(trk.getId());
  for (int i = b_norm_off_[(size_t)trk.candidate]; i < b_norm_off_[(size_t)trk.candidate + 1]; ++i)
    out.emplace_back(b_norm_[2 * (size_t)i], b_norm_[2 * (size_t)i + 1]);
  return out;
}

bool TrackManager::candidateFlag(const TrackedTrack &trk) const {
  if (trk.candidate < 0) throw std::logic_error("TrackManager: a track outside the frame's batch");
  return b_flag_[(size_t)trk.candidate] != 0;
}

void TrackManager::manageTracks(MatchList &matches, const AttitudeList &cam_rots, size_t n_poses_max, size_t n_slam_features_max,
                                size_t min_track_length, TileGrid &grid) {
  if (n_poses_max < 3) throw std::runtime_error("TrackManager::manageTracks: n_poses_max < 3");
  if (cam_rots.size() < 3 || cam_rots.size() > 64) throw std::runtime_error("TrackManager::manageTracks: 3 ... 64 camera attitudes");
  if (multi_uav_ && !opp_ids_) throw std::runtime_error("TrackManager::manageTracks: multi_uav without setOppUpgradesMSCKF");
  // Everything that can refuse the frame is checked before anything changes, so that an exception leaves the manager as it was:
  // every feature that will be binned is a match's current one, and every candidate of the batch is an opportunistic track that
  // lived before this frame (it dies or goes on) or, with min_track_length <= 2, one a match starts.
  const unsigned int n_tiles_w = grid.getNTilesW(), n_bins = grid.getNTilesH() * n_tiles_w;
  for (Match &m : matches) {
    grid.setTileForFeature(m.current);
    const long b = (long)m.current.getTileRow() * n_tiles_w + m.current.getTileCol();
    if (b < 0 || b >= (long)n_bins) throw std::runtime_error("TrackManager::manageTracks: a match outside the tile grid");
  }
  if (opp_trks_.size() + (min_track_length <= 2 ? matches.size() : 0) > (size_t)max_tracks_)
    throw std::runtime_error("TrackManager::manageTracks: the frame may have more candidate tracks than max_tracks");
  n_poses_max_ = n_poses_max;
  // the new persistent tracks of the last image join the persistent ones (:122-124)
  slam_trks_.insert(slam_trks_.end(), new_slam_trks_.begin(), new_slam_trks_.end());
  new_slam_trks_.clear();

  // tracks per tile: bin_track_idx counts persistent and new persistent tracks with the new ones' indices behind the persistent
  // ones'; bin_track_idx_per holds the persistent ones' indices BEFORE this frame's deletions, which is what the state needs
  std::vector<std::vector<unsigned int>> bin_track_idx(n_bins), bin_track_idx_per(n_bins);
  const auto bin_of = [&](TrackedFeature &f) {                       // (inside the grid: checked above)
    grid.setTileForFeature(f);
    return (unsigned int)(f.getTileRow() * (int)n_tiles_w + f.getTileCol());
  };
  unsigned int idx_bin_max_per = 0;

  // 1. persistent tracks: extended by the first match whose previous feature equals their last one, else lost (:140-191)
  unsigned int t = 0, lost_per_count = 0;
  lost_slam_idxs_.clear();
  {
    FirstEqual first(matches, [](const Match &m) -> const Feature & { return m.previous; });
    while (t < slam_trks_.size()) {
      const long m = first.find(slam_trks_[t].back());
      if (m >= 0) {
        TrackedFeature &feature = matches[(size_t)m].current;
        const unsigned int bin_nbr = bin_of(feature);
        bin_track_idx[bin_nbr].push_back(t);
        bin_track_idx_per[bin_nbr].push_back(t + lost_per_count);
        if (bin_track_idx[bin_nbr].size() > bin_track_idx[idx_bin_max_per].size()) idx_bin_max_per = bin_nbr;
        slam_trks_[t].push_back(feature);
        first.remove((size_t)m);                                   // a claimed match leaves the list
        ++t;
      } else {
        lost_slam_idxs_.push_back(t + lost_per_count);             // its index before this frame's deletions
        slam_trks_.erase(slam_trks_.begin() + t);
        ++lost_per_count;
      }
    }
    size_t kept = 0;
    for (size_t m = 0; m < matches.size(); ++m)
      if (first.alive(m)) {
        if (kept != m) matches[kept] = std::move(matches[m]);
        ++kept;
      }
    matches.resize(kept);
  }

  // 2. opportunistic tracks, rebuilt in match order: extended, or started from the match's two features (:197-232)
  msckf_trks_n_.clear();
  msckf_trks_short_n_.clear();
  TrackedTrackList previous_opp_trks;
  previous_opp_trks.swap(opp_trks_);
  {
    FirstEqual first(previous_opp_trks, [](const TrackedTrack &trk) -> const Feature & { return trk.back(); });
    for (Match &match : matches) {
      const long o = first.find(match.previous);
      if (o >= 0) {
        previous_opp_trks[(size_t)o].push_back(match.current);
        opp_trks_.push_back(std::move(previous_opp_trks[(size_t)o]));
        first.remove((size_t)o);
      } else {
        TrackedTrack opp_track;
        opp_track.setId(next_id_++);
        opp_track.push_back(match.previous);
        opp_track.push_back(match.current);
        opp_trks_.push_back(std::move(opp_track));
      }
    }
    TrackedTrackList dead;
    for (size_t o = 0; o < previous_opp_trks.size(); ++o)
      if (first.alive(o)) dead.push_back(std::move(previous_opp_trks[o]));
    previous_opp_trks.swap(dead);
  }

  // 3. every track that may become a measurement this frame, in one device call: the dead tracks (against the attitude list without
  // its last entry: they ended at the previous frame) and the live ones long enough to be promoted or consumed
  b_off_.assign(1, 0); b_obs_.clear(); b_drop_.clear();
  for (TrackedTrack &trk : previous_opp_trks) {
    trk.candidate = -1;
    if (multi_uav_) {
      if (trk.size() >= 3 && std::find(opp_ids_->begin(), opp_ids_->end(), trk.getId()) != opp_ids_->end()) addCandidate(trk, false);
    } else if (trk.size() >= 2) {
      addCandidate(trk, true);
    }
  }
  for (TrackedTrack &trk : opp_trks_) {
    trk.candidate = -1;
    if (trk.size() > min_track_length - 1 && trk.size() >= 2) addCandidate(trk, false);
  }
  runBatch(cam_rots);

  // 4. the dead tracks (:234-273)
  if (multi_uav_) {
    for (const TrackedTrack &dead_track : previous_opp_trks) {
      if (dead_track.size() < 3) continue;
      for (size_t o = 0; o < opp_ids_->size(); ++o)
        if (dead_track.getId() == opp_ids_->at(o)) {
          msckf_trks_short_n_.push_back(normalizedCandidate(dead_track));   // no baseline check on this branch (:252-253)
          opp_ids_->erase(opp_ids_->begin() + (std::ptrdiff_t)o);
          break;
        }
    }
  } else {
    for (const TrackedTrack &a : previous_opp_trks) {
      if (a.size() < 2) continue;
      if (candidateFlag(a)) msckf_trks_short_n_.push_back(normalizedCandidate(a));
    }
  }

  // 5. the promotion walk, longest track first (:274-395)
  std::stable_sort(opp_trks_.begin(), opp_trks_.end(), [](const TrackedTrack &a, const TrackedTrack &b) { return a.size() > b.size(); });
  t = 0;
  while (t < opp_trks_.size()) {
    const unsigned int bin_nbr = bin_of(opp_trks_[t].back());
    if (opp_trks_[t].size() > min_track_length - 1) {
      if ((slam_trks_.size() + new_slam_trks_.size()) < n_slam_features_max) {
        // a free slot
        new_slam_trks_.push_back(std::move(opp_trks_[t]));
        opp_trks_.erase(opp_trks_.begin() + t);
        bin_track_idx[bin_nbr].push_back((unsigned int)(slam_trks_.size() + new_slam_trks_.size() - 1));
        if (bin_track_idx[bin_nbr].size() > bin_track_idx[idx_bin_max_per].size()) idx_bin_max_per = bin_nbr;
      } else if (bin_track_idx[idx_bin_max_per].size() > bin_track_idx[bin_nbr].size() + 1) {
        // the fullest tile holds more than one track more than this one's: its youngest track goes
        const unsigned int gone = bin_track_idx[idx_bin_max_per].back();
        if (gone >= slam_trks_.size()) {
          new_slam_trks_.erase(new_slam_trks_.begin() + (gone - slam_trks_.size()));
        } else {
          if (bin_track_idx_per[idx_bin_max_per].empty()) throw std::logic_error("TrackManager::manageTracks: tile bookkeeping out of step");
          lost_slam_idxs_.push_back(bin_track_idx_per[idx_bin_max_per].back());
          bin_track_idx_per[idx_bin_max_per].pop_back();
          slam_trks_.erase(slam_trks_.begin() + gone);
        }
        for (auto &bin : bin_track_idx)
          for (unsigned int &idx : bin)
            if (idx > gone) --idx;
        bin_track_idx[idx_bin_max_per].pop_back();
        new_slam_trks_.push_back(std::move(opp_trks_[t]));
        opp_trks_.erase(opp_trks_.begin() + t);
        bin_track_idx[bin_nbr].push_back((unsigned int)(slam_trks_.size() + new_slam_trks_.size() - 1));
        for (unsigned int i = 0; i < n_bins; ++i)
          if (bin_track_idx[i].size() > bin_track_idx[idx_bin_max_per].size()) idx_bin_max_per = i;
      } else if (opp_trks_[t].size() > n_poses_max - 1) {
        // too long for the window: an MSCKF measurement iff its baseline passes, gone either way
        if (candidateFlag(opp_trks_[t])) msckf_trks_n_.push_back(normalizedCandidate(opp_trks_[t]));
        opp_trks_.erase(opp_trks_.begin() + t);
      } else {
        ++t;
      }
    } else {
      ++t;
    }
  }
  if (multi_uav_) opp_ids_->clear();

  // 6. the new persistent tracks: MSCKF-SLAM where the baseline passes, standard otherwise; the own list MSCKF-SLAM first, the order
  // in which the update inserts their states (:400-432)
  new_slam_std_trks_n_.clear();
  new_slam_msckf_trks_n_.clear();
  TrackedTrackList new_slam_std_trks, new_slam_msckf_trks;
  for (TrackedTrack &trk : new_slam_trks_) {
    if (candidateFlag(trk)) {
      new_slam_msckf_trks_n_.push_back(normalizedCandidate(trk));
      new_slam_msckf_trks.push_back(std::move(trk));
    } else {
      new_slam_std_trks_n_.push_back(normalizedCandidate(trk));
      new_slam_std_trks.push_back(std::move(trk));
    }
  }
  new_slam_trks_.clear();
  for (TrackedTrack &trk : new_slam_msckf_trks) new_slam_trks_.push_back(std::move(trk));
  for (TrackedTrack &trk : new_slam_std_trks) new_slam_trks_.push_back(std::move(trk));
}

// ---- the facet around a point --------------------------------------------------------------------------------------------------------
namespace {
struct P2 { double x, y; };
double orient(const P2 &a, const P2 &b, const P2 &c) { return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x); }
// > 0 iff d lies strictly inside the circle through a, b, c taken counter-clockwise
double inCircle(const P2 &a, const P2 &b, const P2 &c, const P2 &d) {
  const double ax = a.x - d.x, ay = a.y - d.y, bx = b.x - d.x, by = b.y - d.y, cx = c.x - d.x, cy = c.y - d.y;
  const double a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
  return ax * (by * c2 - b2 * cy) - ay * (bx * c2 - b2 * cx) + a2 * (bx * cy - by * cx);
}
}  // namespace

std::vector<int> TrackManager::featureTriangleAtPoint(const TrackedFeature &lrf_img_pt, unsigned int width, unsigned int height) const {
  std::vector<TrackedFeature> newest;
  newest.reserve(slam_trks_.size());
  for (const TrackedTrack &trk : slam_trks_) newest.push_back(trk.back());
  return x::featureTriangleAtPoint(newest, lrf_img_pt, width, height);
}

std::vector<int> x::featureTriangleAtPoint(const std::vector<TrackedFeature> &newest, const TrackedFeature &lrf_img_pt, unsigned int width,
                                           unsigned int height) {
  const int n = (int)newest.size();
  const P2 p{(double)(float)lrf_img_pt.getXDist(), (double)(float)lrf_img_pt.getYDist()};
  if (n < 3 || !(p.x >= -1.0 && p.x < (double)width + 1.0 && p.y >= -1.0 && p.y < (double)height + 1.0)) return {};
  std::vector<P2> pts;
  pts.reserve((size_t)n + 3);
  for (const TrackedFeature &f : newest) pts.push_back(P2{(double)(float)f.getXDist(), (double)(float)f.getYDist()});
  const double big = 3.0 * (double)std::max(width + 2, height + 2);
  pts.push_back(P2{-1.0 + big, -1.0}); pts.push_back(P2{-1.0, -1.0 + big}); pts.push_back(P2{-1.0 - big, -1.0 - big});
  const int m = n + 3;
  for (int i = 0; i < m; ++i)
    for (int j = i + 1; j < m; ++j)
      for (int k = j + 1; k < m; ++k) {                       // lexicographic order: the first that qualifies is the smallest
        const P2 &a = pts[(size_t)i];
        const double o = orient(a, pts[(size_t)j], pts[(size_t)k]);
        if (o == 0.0) continue;
        const P2 &b = o > 0.0 ? pts[(size_t)j] : pts[(size_t)k], &c = o > 0.0 ? pts[(size_t)k] : pts[(size_t)j];
        if (orient(a, b, p) < 0.0 || orient(b, c, p) < 0.0 || orient(c, a, p) < 0.0) continue;
        bool empty = true;
        for (int l = 0; l < m && empty; ++l)
          if (l != i && l != j && l != k && inCircle(a, b, c, pts[(size_t)l]) > 0.0) empty = false;
        if (!empty) continue;
        if (k >= n) return {};                                  // it reaches an outer vertex
        return {i, j, k};
      }
  return {};
}
