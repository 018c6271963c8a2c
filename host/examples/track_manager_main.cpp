// x::TrackManager on a scripted sequence of match lists (written by tests/test_gpu_track_manager_host.py).
//   usage  : xk_track_manager_example case.txt            every frame's matches go through manageTracks, and every list it leaves
//                                                         is printed, one line per track, for the comparison with the restatement
//            xk_track_manager_example case.txt update     the end-to-end run: a filter (x::Ekf + x::Propagator + x::VioUpdater with
//                                                         manage_window on) runs beside the manager; the IMU of the scripted motion
//                                                         carries it from frame to frame, the attitude list comes from ITS window,
//                                                         and every frame's fill() goes into setMeasurement / processUpdateMeasurement
//   case   : fx fy cx cy s width height min_baseline_x_n min_baseline_y_n max_tracks multi_uav n_poses_max n_slam_max min_track_length
//            tiles_h tiles_w n_frames          (fx ... cy as fractions of the image size)
//            per frame: n_matches n_quats n_opp_ids point_x point_y
//                       n_matches rows  prev_x prev_y prev_x_dist prev_y_dist cur_x cur_y cur_x_dist cur_y_dist fast_score
//                       n_quats rows    x y z w
//                       n_opp_ids ids   (multi_uav: the ids the caller upgrades this frame)
//            behind the frames, read by `update` only: dt v_x v_y v_z yaw_rate sigma_img imu_per_frame -- the camera (= the IMU) starts
//            at the origin with the identity attitude, moves at the constant velocity v and turns about its y axis at yaw_rate;
//            the case's first frame is camera frame 1
//   output : per frame
//            F <frame> <ms of the xk_trk_baseline call> <ms of manageTracks, that call included> <matches> <candidate tracks> <their observations>
//            L <index ...>                              getLostSlamTrackIndexes
//            T <list> <id> <length> <x y ...>           one per track of msckf, short, new_std, new_msckf, slam (normalizeSlamTracks(n_poses_max)),
//                                                       opp (getOppTracks), %.17g
//            S <id ...> | <id ...>                      the manager's persistent and new persistent tracks, in its own order
//            O <id:length ...>                          its opportunistic tracks
//            P <id ...>                                 getMostPromisingTracks(3)
//            A <index ...>                              featureTriangleAtPoint at the frame's point
//            G <x y ...>                                getOppFeatures, %.17g
//            M <list> <id ...>                          the ids of each of the five track fields fill() set (slam, msckf, short, new_msckf,
//                                                       new_std), then M lost <index ...>
//            `update` adds per frame
//            U <frame> <applied> <poses> <features> <msckf given> <msckf consumed> <msckf inliers> <short given> <finite> <max |P - P^T|>
//                      <position error> (applied: processUpdateMeasurement returned a state; finite: 31 when the covariance (1), the position (2),
//                      attitude (4) and feature (8) arrays and the core states (16) all are)
//            after the last frame, without `update`: the removal calls on the manager
//            R <persistent after removePersistentTracksAtIndex(0)> <new persistent after removeNewPersistentTracksAtIndexes({0})>
//              <tracks of every list after clear()>
#include "track_manager_run.h"

int main(int argc, char **argv) {
  return track_manager_run<TrackManager>(argc, argv, [](xk_handle *xk, const Camera &camera, double min_bx, double min_by, int max_tracks, bool multi_uav,
                                                        unsigned int, unsigned int) {
    return std::make_unique<TrackManager>(xk, camera, min_bx, min_by, max_tracks, multi_uav);
  });
}
