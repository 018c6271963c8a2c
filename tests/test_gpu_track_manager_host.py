"""host/examples/track_manager_main.cpp -- x::TrackManager of the C++ mirror (host list walk, one xk_trk_baseline call per frame) --
on the scripted sequence written to a temporary file, against the Python restatement (track_manager_np.TrackManagerNp): after
every frame every list (ids, lengths, normalised coordinates bit for bit), the lost indices, the manager's own order of its tracks
and the facet at the frame's point must be the restatement's.  The facet cases of track_manager_cases (up to 12 persistent
tracks) go through the same example: two frames that make every point a persistent track, then the query.

The example's second mode is the end-to-end run: the manager in front of the x::VioUpdater mirror with manage_window on, inside an
x::Ekf that the scripted motion's IMU carries from frame to frame, for 12 frames.  Every update must be applied, the state stay
finite, P be symmetric to 1e-12 and the update consume as many MSCKF tracks as the manager handed out."""
import os
import subprocess

import numpy as np
import pytest

import track_manager_cases as tc
import track_manager_np as tm

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")
ENV = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
MOTION = dict(dt=0.1, v=(1.2, 0.1, 0.0), yaw_rate=0.12, sigma_img=0.0025, imu_per_frame=10)     # track_manager_cases.sequence, 10 frames a second


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(PKG, "xk_track_manager_example")
    if not os.path.exists(path):
        from x_multi_agent_amd import build
        build.build_host()
    return path


def write_case(path, frames, multi_uav, max_tracks=64, s=tc.SEQ, motion=None):
    rows = [f"{tc.CAM_FRACTIONS[0]!r} {tc.CAM_FRACTIONS[1]!r} {tc.CAM_FRACTIONS[2]!r} {tc.CAM_FRACTIONS[3]!r} 0.0 {tc.WIDTH} {tc.HEIGHT} "
            f"{tc.MIN_BASELINE[0]!r} {tc.MIN_BASELINE[1]!r} {max_tracks} {int(multi_uav)} {s['n_poses_max']} {s['n_slam_max']} {s['min_track_length']} "
            f"{s['tiles'][0]} {s['tiles'][1]} {len(frames)}"]
    for fr in frames:
        rows.append(f"{len(fr['matches'])} {len(fr['cam_rots'])} {len(fr['opp_ids'])} {fr['point'][0]!r} {fr['point'][1]!r}")
        for p, c in fr["matches"]:
            rows.append(" ".join(repr(v) for v in (p.x, p.y, p.xd, p.yd, c.x, c.y, c.xd, c.yd, c.score)))
        rows.extend(" ".join(repr(float(v)) for v in q) for q in fr["cam_rots"])
        rows.append(" ".join(str(i) for i in fr["opp_ids"]))
    if motion:
        rows.append(f"{motion['dt']!r} {motion['v'][0]!r} {motion['v'][1]!r} {motion['v'][2]!r} {motion['yaw_rate']!r} {motion['sigma_img']!r} "
                    f"{motion['imu_per_frame']}")
    path.write_text("\n".join(rows) + "\n")


def expected_frames(multi_uav):
    """The restatement over the sequence -> (frames as written, per frame what the example prints)."""
    frames, want = tc.sequence(multi_uav), []

    def on_frame(i, fr, m):
        slam_xy = [(t[-1].xd, t[-1].yd) for t in m.slam]
        lists = dict(msckf=m.msckf_n, short=m.msckf_short_n, new_std=m.new_slam_std_n, new_msckf=m.new_slam_msckf_n,
                     slam=m.normalize_slam_tracks(tc.SEQ["n_poses_max"]), opp=m.get_opp_tracks())
        want.append(dict(L=list(m.lost), T={k: [(t.id, np.array(t, np.float64).reshape(-1, 2)) for t in v] for k, v in lists.items()},
                         S=([t.id for t in m.slam], [t.id for t in m.new_slam]), O=[(t.id, len(t)) for t in m.opp],
                         P=[t.id for t in m.most_promising(3)],
                         G=np.array([((t[-1].x - tc.K[2]) / tc.K[0], (t[-1].y - tc.K[3]) / tc.K[1]) for t in m.opp], np.float64).reshape(-1, 2),
                         R=[max(len(m.slam) - 1, 0), max(len(m.new_slam) - 1, 0), 0],
                         A=tc.assert_general_position(slam_xy, fr["point"], tc.WIDTH, tc.HEIGHT)))    # (so fp64 predicates decide as exact ones)

    mgr = tc.run_sequence(multi_uav, frames=frames, on_frame=on_frame)
    return frames, want, mgr


def parse(stdout):
    got = []
    for line in stdout.strip().splitlines():
        w = line.split()
        if w[0] == "F":
            got.append(dict(L=[], T={k: [] for k in ("msckf", "short", "new_std", "new_msckf", "slam", "opp")}, ms=float(w[2])))
        elif w[0] == "T":
            xy = np.array([float(v) for v in w[4:]], np.float64).reshape(-1, 2)
            assert len(xy) == int(w[3])
            got[-1]["T"][w[1]].append((int(w[2]), xy))
        elif w[0] == "S":
            bar = w.index("|")
            got[-1]["S"] = ([int(v) for v in w[1:bar]], [int(v) for v in w[bar + 1:]])
        elif w[0] == "O":
            got[-1]["O"] = [tuple(int(v) for v in item.split(":")) for item in w[1:]]
        elif w[0] == "M":
            got[-1].setdefault("M", {})[w[1]] = [int(v) for v in w[2:]]
        elif w[0] == "G":
            got[-1]["G"] = np.array([float(v) for v in w[1:]], np.float64).reshape(-1, 2)
        elif w[0] == "U":
            got[-1]["U"] = dict(applied=int(w[2]), poses=int(w[3]), features=int(w[4]), given=int(w[5]), consumed=int(w[6]), inliers=int(w[7]),
                                short=int(w[8]), finite=int(w[9]), asym=float(w[10]), perr=float(w[11]))
        else:
            got[-1][w[0]] = [int(v) for v in w[1:]]
    return got


@pytest.mark.parametrize("multi_uav", [False, True], ids=["single", "multi_uav"])
def test_cpp_track_manager_follows_the_restatement(tmp_path, exe, multi_uav):
    frames, want, mgr = expected_frames(multi_uav)
    case = tmp_path / "case.txt"
    write_case(case, frames, multi_uav)
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = parse(r.stdout)
    assert len(got) == len(want) == len(frames)
    n_tracks = 0
    for f, (g, w) in enumerate(zip(got, want)):
        assert g["L"] == w["L"], f
        assert g["S"] == w["S"] and g["O"] == w["O"] and g["P"] == w["P"] and g["A"] == w["A"], f
        for name, tracks in w["T"].items():
            assert [i for i, _ in g["T"][name]] == [i for i, _ in tracks], (f, name)
            for (_, a), (_, b) in zip(g["T"][name], tracks):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (f, name)
            n_tracks += len(tracks)
        assert g["G"].shape == w["G"].shape and g["G"].tobytes() == w["G"].tobytes(), f
        # fill(): the six fields, by track id (their coordinates are the T lines' above: the same lists)
        assert g["M"] == dict(lost=w["L"], **{k: [i for i, _ in w["T"][k]] for k in ("slam", "msckf", "short", "new_msckf", "new_std")}), f
    # removePersistentTracksAtIndex(0), removeNewPersistentTracksAtIndexes({0}) and clear() after the last frame
    assert got[-1]["R"] == want[-1]["R"]
    assert n_tracks > 100 and any(w["A"] for w in want) and any(w["L"] for w in want)
    assert sum(len(w["T"]["msckf"]) for w in want) > 0 and sum(len(w["T"]["short"]) for w in want) > 0


FACETS = tc.facet_cases()


@pytest.mark.parametrize("name", sorted(FACETS))
def test_cpp_facet_cases(tmp_path, exe, name):
    """Two frames turn the case's points into persistent tracks in their order (min_track_length 2 and a free slot for each: promoted
    at the first frame, none moves far enough for a baseline, persistent from the second); the second frame's query is the case's."""
    c = FACETS[name]
    params = dict(n_poses_max=6, n_slam_max=12, min_track_length=2, tiles=(2, 2))
    quats = [[0.0, 0.0, 0.0, 1.0]] * 6
    pts = c["points"]
    frames = [dict(matches=[[tm.Feat(x - 2.0, y), tm.Feat(x - 1.0, y)] for x, y in pts], cam_rots=quats, point=(1.0, 1.0), opp_ids=[]),
              dict(matches=[[tm.Feat(x - 1.0, y), tm.Feat(x, y)] for x, y in pts], cam_rots=quats, point=c["query"], opp_ids=[])]
    mgr = tm.TrackManagerNp(tc.K, *tc.MIN_BASELINE)
    grid = tm.TileGridNp(tc.WIDTH, tc.HEIGHT, 2, 2)
    for fr in frames:
        mgr.manage([[p.copy(), q.copy()] for p, q in fr["matches"]], quats, 6, 12, 2, grid)
    assert [(t[-1].xd, t[-1].yd) for t in mgr.slam] == [tuple(p) for p in pts]
    case = tmp_path / "case.txt"
    write_case(case, frames, False, s=params)
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = parse(r.stdout)
    assert got[1]["S"] == ([t.id for t in mgr.slam], []) and len(got[1]["S"][0]) == len(pts)
    assert got[1]["A"] == c["expect"]


def test_manager_in_front_of_the_vio_updater(tmp_path, exe):
    """The end-to-end run, 12 frames: matches -> x::TrackManager -> fill() -> x::VioUpdater (manage_window on) inside an x::Ekf driven
    by the scripted motion's IMU; the attitude list of every frame comes from the filter's own window."""
    frames = tc.sequence()[:12]
    case = tmp_path / "case.txt"
    write_case(case, frames, False, motion=MOTION)
    r = subprocess.run([exe, str(case), "update"], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = parse(r.stdout)
    assert len(got) == 12
    for f, g in enumerate(got):
        u = g["U"]
        print(f"frame {f}: poses {u['poses']} features {u['features']} msckf given {u['given']} consumed {u['consumed']} inliers {u['inliers']} "
              f"short {u['short']} finite {u['finite']} max |P - P^T| {u['asym']:.3e} position error {u['perr']:.3e}")
    for f, g in enumerate(got):
        u = g["U"]
        assert u["applied"] == 1 and u["finite"] == 31, (f, u["finite"], r.stderr)     # 31: covariance, the three arrays and the core states
        assert 0.0 <= u["asym"] <= 1e-12, f
        assert u["consumed"] == u["given"] == len(g["M"]["msckf"]), f
        assert u["poses"] == min(f + 2, tc.SEQ["n_poses_max"]), f                 # camera frame 0's pose, then one a frame until it slides
        assert u["features"] == len(g["S"][0]) + len(g["S"][1]), f                # the state's features are the manager's persistent tracks
    assert sum(g["U"]["given"] for g in got) > 0 and sum(g["U"]["short"] for g in got) > 0 and max(g["U"]["features"] for g in got) > 0
    assert any(g["M"]["lost"] for g in got)
