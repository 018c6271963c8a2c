// x/place_recognition/database.h -- mirror of x::VLAD, x::Keyframe and x::Database
// (include/x/place_recognition/{vlad,keyframe,database}.h, src/x/place_recognition/{vlad,keyframe,database}.cpp)
// and of the matching front half of PlaceRecognition::findCorrespondences (place_recognition.cpp:137-390); and the
// training of the vocabulary they take (DBoW3::Vocabulary::create).
//
// The reference keeps descriptors and VLADs in cv::Mat and the vocabulary in a DBoW3::Vocabulary; here a
// descriptor set is a row-major byte matrix and the vocabulary is the plain tree DBoW3 stores (PRVocabulary).
// Every bit operation -- the vocabulary descent, the XOR / OR aggregation, the Hamming norms, the 2-NN search --
// runs on the GPU behind the xk_pr_* entry points (include/xk.h); keyframes (SimpleState payload, tracks,
// descriptors, VLAD) stay in device memory.  There is no CPU fallback.
//
// findCorrespondences exists twice: Database::findCorrespondences is the reference's function as one device call (match,
// ratio test, essential-matrix filter, mask, duplicate removal, classification; the lists never visit the host in
// between), and knnMatch / essentialInliers with the free functions ratioTestMatches / goodMatches / classifyMatches are
// the same thing stage by stage, with the list work on the host.  Both give the same lists.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "xk.h"

namespace x {

struct Descriptors {               // cv::Mat of CV_8UC1 rows
  int rows = 0, cols = 32;
  std::vector<unsigned char> data;
  const unsigned char *ptr() const { return data.empty() ? nullptr : data.data(); }
};
using VLADVec = std::vector<unsigned char>;   // clusters x descriptor bytes (types.h:36: cv::Mat)

struct PRVocabulary {              // what DBoW3::Vocabulary holds (types.h:33), as Vocabulary::fromStream reads it
  int k = 0, L = 0, kmax = 0, desc_bytes = 32;
  std::vector<unsigned char> node_desc;       // [n_nodes][desc_bytes]
  std::vector<int> children;                  // [n_nodes][kmax], -1 padded, file order
  std::vector<int> word_of_node, node_of_word;
  int nNodes() const { return (int)word_of_node.size(); }
};

class Keyframe {                   // keyframe.h / keyframe.cpp: the store keeps its payload on the device
 public:
  Keyframe(Descriptors descriptors, const double *d_payload, const double *d_tracks, long tag)
      : descriptors_(std::move(descriptors)), d_payload_(d_payload), d_tracks_(d_tracks), tag_(tag) {}
  const Descriptors &getDescriptors() const { return descriptors_; }   // MSCKF, SLAM, OPP order (keyframe.cpp:40-52)
  const double *payload() const { return d_payload_; }                 // DEVICE, xk_pack_payload layout (SimpleState)
  const double *tracks() const { return d_tracks_; }                   // DEVICE, packed track observations
  long tag() const { return tag_; }
 private:
  Descriptors descriptors_;
  const double *d_payload_, *d_tracks_;
  long tag_;
};
using KeyframePtr = std::shared_ptr<Keyframe>;

struct Candidate {                 // what VIO::processOtherRequests sends back (vio.cpp:489-495), device pointers
  int index = -1;                  // position in the database, oldest first; -1: no candidate
  double score = 0.0;
  long tag = -1;
  const double *d_payload = nullptr, *d_tracks = nullptr;
  int n_descriptors = 0;
};

// What findCorrespondences hands to the CI update, before the bookkeeping of :518-577.
struct GoodMatch { int queryIdx, trainIdx; };
enum class MatchKind { MSCKF_OPP, SLAM_SLAM, SLAM_OPP, OPP_OPP };
struct ClassifiedMatch { MatchKind kind; int current, received; };
struct Correspondences {
  int status = 0;                  // xk_pr_corr_out::status: 0 matched, 1...5 the reference's early returns
  int n_candidates = 0, n_inliers = 0;
  std::vector<GoodMatch> good;     // after the mask and the duplicate removal (:275-302)
  std::vector<ClassifiedMatch> classified;   // :311-383
  double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};

class Database {                   // database.h / database.cpp
 public:
  // payload_doubles / tracks_doubles: sizes of the per-keyframe device buffers the store copies
  Database(xk_handle *xk, const PRVocabulary &vocabulary, double pr_score_thr, long payload_doubles, long tracks_doubles,
           int max_descriptors = 1024);
  ~Database();
  Database(const Database &) = delete;
  Database &operator=(const Database &) = delete;

  void addKeyframe(const KeyframePtr &keyframe);                         // database.cpp:51-61
  void findCandidate(int uav_id, const VLADVec &query_vlad, Candidate &best_candidate);   // :30-49
  VLADVec computeVLAD(const Descriptors &descriptors);                   // :26-28 -> VLAD::computeVLAD (vlad.cpp:40-66)
  Descriptors keyframeDescriptors(int index);
  int size() const;

  // matcher_->knnMatch(received, current, matches_, 2) (place_recognition.cpp:249): idx / dist [rows][2]
  void knnMatch(const Descriptors &received, const Descriptors &current, std::vector<int> &idx, std::vector<int> &dist);

  // cv::findEssentialMat(current_points, received_points, K, cv::RANSAC, 0.99, threshold, mask) (:269-281): the inlier
  // mask of the good matches' pixel positions ([n][2], x then y), from n_hyp five-point hypotheses on the device
  // (xk_pr_essential_ransac; every hypothesis is evaluated, so there is no `prob`).  All zero for fewer than 5 points.
  std::vector<unsigned char> essentialInliers(const std::vector<float> &current_points, const std::vector<float> &received_points,
                                              double fx, double fy, double cx, double cy, double threshold = 1.0,
                                              int n_hyp = 1024, unsigned long seed = 0);

  // PlaceRecognition::findCorrespondences (place_recognition.cpp:137-385, the non-GT branch) in one call
  // (xk_pr_find_correspondences): 2-NN match, distance + ratio test, essential-matrix filter, mask, duplicate removal and
  // classification on the device, one copy in, one result block out, one wait.  Descriptors and pixels ([rows][2], x then
  // y) of both sides in MSCKF | SLAM | OPP order.  The same lists as knnMatch -> ratioTestMatches -> essentialInliers ->
  // goodMatches -> classifyMatches.
  Correspondences findCorrespondences(const Descriptors &received, const std::vector<float> &received_points,
                                      const Descriptors &current, const std::vector<float> &current_points, int n_cur_msckf,
                                      int n_cur_slam, int n_rec_msckf, int n_rec_slam, double pr_min_distance,
                                      double pr_ratio_thr, double fx, double fy, double cx, double cy, double threshold = 1.0,
                                      int n_hyp = 1024, unsigned long seed = 0);

 private:
  xk_handle *xk_;
  xk_pr *pr_ = nullptr;
  double pr_score_thr_;
  int desc_bytes_;
};

// DBoW3::Vocabulary::create (third_party/DBow3/src/Vocabulary.cpp:157-186) for binary descriptors on the device
// (xk_voc_*): hierarchical k-means with k-means++ seeding and bit-majority means.  The reference seeds with rand(); here
// the tree is a function of (descriptors in the order added, k, L, seed, max_iter).
class VocabularyTrainer {
 public:
  using Outcome = xk_voc_outcome;
  VocabularyTrainer(xk_handle *xk, int k, int L, int desc_bytes = 32, int max_descriptors = 1 << 16);
  ~VocabularyTrainer();
  VocabularyTrainer(const VocabularyTrainer &) = delete;
  VocabularyTrainer &operator=(const VocabularyTrainer &) = delete;

  void add(const Descriptors &descriptors);                             // getFeatures (:220-228): appended in call order
  int count() const;
  void clear();
  PRVocabulary train(unsigned long seed = 0, int max_iter = 100, Outcome *outcome = nullptr);   // kmax = k

 private:
  xk_handle *xk_;
  xk_voc *voc_ = nullptr;
  int k_, L_, desc_bytes_;
};

// The rest of findCorrespondences' non-GT branch on the 2-NN result: distance + ratio test (:252-263), optional
// RANSAC inlier mask (:268-281; Database::essentialInliers estimates it on the device), duplicate removal (:283-301).
// The stage-by-stage path: Database::findCorrespondences computes the same lists in one call.
// The survivors of the distance + ratio test alone (:252-263), before the mask and the duplicate removal: the matches whose
// pixel positions the reference collects for findEssentialMat (:264-267), and the list an inlier mask is indexed by.
std::vector<GoodMatch> ratioTestMatches(const std::vector<int> &idx, const std::vector<int> &dist, double pr_min_distance,
                                        double pr_ratio_thr);
std::vector<GoodMatch> goodMatches(const std::vector<int> &idx, const std::vector<int> &dist, double pr_min_distance,
                                   double pr_ratio_thr, const std::vector<unsigned char> *inlier_mask = nullptr);

// Classification of place_recognition.cpp:311-388.
std::vector<ClassifiedMatch> classifyMatches(const std::vector<GoodMatch> &good, int n_cur_msckf, int n_cur_slam,
                                             int n_rec_msckf, int n_rec_slam);
}  // namespace x
