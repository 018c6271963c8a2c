// x::ResidentTrackManager (the track manager on tracks that stay on the device) on a scripted sequence of match lists
// (written by tests/test_gpu_resident_tracks_host.py): the modes, the case file and the output of track_manager_main.cpp, through the
// same body.
//   usage  : xk_resident_tracks_example case.txt            the sequence, every list dumped per frame; the facet cases are sequences too
//            xk_resident_tracks_example case.txt update     the end-to-end run with x::Ekf + x::VioUpdater on one engine handle
// The F line's first time is the device call (all of manageTracks but the host's copies), its second the whole of manageTracks.
#include "x/vio/resident_track_manager.h"

#include "track_manager_run.h"

int main(int argc, char **argv) {
  return track_manager_run<ResidentTrackManager>(argc, argv, [](xk_handle *xk, const Camera &camera, double min_bx, double min_by, int max_tracks,
                                                                bool multi_uav, unsigned int tiles_h, unsigned int tiles_w) {
    return std::make_unique<ResidentTrackManager>(xk, camera, min_bx, min_by, max_tracks, multi_uav, tiles_h, tiles_w);
  });
}
