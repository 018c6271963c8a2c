"""The device-resident track manager's entries are declared in include/xk.h, exported by all three libraries that the
build makes, listed in README and DESIGN, and their kernel file is part of the build.  CPU only: nothing here touches a device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(ROOT, "x_multi_agent_amd")
NEW = ("xk_trk_tracks_setup", "xk_trk_tracks_manage", "xk_trk_tracks_manage_frame", "xk_trk_tracks_lists", "xk_trk_tracks_remove_persistent",
       "xk_trk_tracks_remove_new_persistent", "xk_trk_tracks_clear")
KERNELS = ("xk_ts_associate", "xk_ts_candidates", "xk_ts_baseline", "xk_ts_walk", "xk_ts_remove", "xk_ts_clear", "xk_ts_gather")


def test_the_new_symbols_are_declared_and_listed():
    from x_multi_agent_amd import engine
    header = open(os.path.join(ROOT, "include", "xk.h")).read()
    readme, design = open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()
    for s in NEW:
        assert s in engine.SYMBOLS and re.search(r"\bint %s\(" % s, header), s
        assert s in design, s
    assert "xk_trk_tracks_manage" in readme and "xk_track_store.hip.h" in readme
    assert re.search(r"^### 3\.21 ", design, re.M) and re.search(r"^### 6\.13 ", design, re.M)
    assert "typedef struct xk_trk_tracks_out" in header


@pytest.mark.parametrize("lib", ["libxk.so", os.path.join("lab", "libxk.so"), "libxk_strict.so"])
def test_every_library_exports_them(lib):
    path = os.path.join(PKG, lib)
    assert os.path.exists(path), "%s: built by `python __graft_entry__.py`" % lib
    exported = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert [s for s in NEW if s not in names] == []


def test_the_kernel_file_is_part_of_the_build():
    from x_multi_agent_amd import build
    src = os.path.join(PKG, "csrc", "xk_track_store.hip.h")
    assert src in [os.path.abspath(d) for d in build.DEPS]
    assert '#include "xk_track_store.hip.h"' in open(os.path.join(PKG, "csrc", "xk_tracker_api.hip.h")).read()
    # its kernels were compiled for gfx950: their names are in the library's device code object
    blob = open(os.path.join(PKG, "libxk.so"), "rb").read()
    assert b"gfx950" in blob
    assert [k for k in KERNELS if k.encode() not in blob] == []


def test_the_shared_device_functions_have_both_callers():
    csrc = os.path.join(PKG, "csrc")
    store, tracks, frame = (open(os.path.join(csrc, f)).read() for f in ("xk_track_store.hip.h", "xk_tracks.hip.h", "xk_frame.hip.h"))
    assert "xk_tracks_baseline_body(" in store and tracks.count("xk_tracks_baseline_body(") == 2      # its definition and xk_tracks_baseline
    assert "xk_tile_for_feature(" in store and frame.count("xk_tile_for_feature(") == 2                  # its definition and xk_frame_tile
    assert "asm" not in store and "atomic" not in store.replace("atomicMin(s_min", "").replace("Integer atomics on LDS only", "")


def test_the_new_example_builds():
    """host/examples/resident_tracks_main.cpp goes through build.py's loop over the examples like the others, and the build made it;
    the host mirror's class is in libx_host.so."""
    src = os.path.join(ROOT, "host", "examples", "resident_tracks_main.cpp")
    assert os.path.exists(src) and os.path.exists(os.path.join(ROOT, "host", "examples", "track_manager_run.h"))
    assert os.path.exists(os.path.join(ROOT, "host", "include", "x", "vio", "resident_track_manager.h"))
    assert os.path.exists(os.path.join(ROOT, "host", "src", "resident_track_manager.cpp"))
    exe = os.path.join(PKG, "xk_resident_tracks_example")
    assert os.path.exists(exe) and os.access(exe, os.X_OK), "built by `python __graft_entry__.py`"
    lib = subprocess.run(["nm", "-D", "--defined-only", "-C", os.path.join(PKG, "libx_host.so")], check=True, capture_output=True, text=True).stdout
    for method in ("x::ResidentTrackManager::manageTracks(", "x::ResidentTrackManager::manageFrame(", "x::featureTriangleAtPoint("):
        assert method in lib, method
    # without a device the example still starts and says what it wants
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib"), timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
