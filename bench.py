#!/usr/bin/env python
"""bench.py -- EKF visual updates/s on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config 4] [--dump-outputs DIR] [--full]

One process per GPU.  N > 1: either a launcher started the ranks (torch.distributed.run -- RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* in the environment) or the plain command `python bench.py --gpus N` starts them itself by
re-running under torch.distributed.run on 127.0.0.1; a world size that is not --gpus is refused.  Rank r is agent r with its own synthetic window/tracks/prior (seed
0x5EED0000 + 1000*config + agent).  A step = one Updater::update()-equivalent
visual update (per-feature build -> CAQR compression -> Kalman update) on
inputs already resident in HBM; P stays on the device.  Every CI_EVERY steps
the agents exchange their SimpleState payloads (state + full covariance) with
one RCCL all-gather and fuse the shared tracks against them on the device
(config 4); --config 5 runs the reference's request/response protocol instead,
every 6 updates: binary-VLAD request, the responder's best keyframe back.
value = (N * K updates) / max-over-ranks wall time; ms_per_step = that wall time / K.
--dump-outputs DIR writes what the last timed step computed (posterior P, correction, inlier masks, gamma) as
DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.

With --full the JSON line also carries
  roofline      fp64 roofline of the dominant stage (CAQR kernels), timed with
                HIP events on the engine's stream: achieved TFLOP/s from the rows
                actually stacked, against the spec peak AND the ceiling measured
                in this run; per-kernel fabric GB/s, MFMA-busy %, L2 hit % from
                the PMC file of this round (refused if taken from other kernels)
  frame_loop    whole filter frames through the C++ mirror of the reference API
                (7 IMU steps, manage(), update, State::correct) with the
                covariance resident on the device -- the drop-in's own rate
  other_configs BASELINE configs 2 (SLAM rows, 331 columns) and 3 (50-pose window, 800 tracks) on the
                same path: updates/s, stage times, QR roofline fraction, parity against the oracle
  cpu_baseline  the C restatement of the reference path (oracle/xk_oracle.c),
                single thread, timed on this box's host cores (rank 0, N=1)
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

FP64_PEAK_TFLOPS = 78.6   # MI355X fp64 vector = fp64 matrix dense peak (AMD public spec)
ROUND_TAG = "r06"         # profiles/<tag>_pmc_traffic.json is the PMC file this bench line may quote
CLOCK_RAMP_S = 0.2        # untimed: the same update replayed for this long before the W warm-up steps (GPU clocks up after the host-side set-up)
CI_EVERY = 10             # BASELINE.json config 4: CI fusion messages every 10 updates
CI_TRACKS = 2             # shared MSCKF tracks fused per CI round
PR_SCORE_THR = 0.6        # pr_score_thr (vio.cpp:670): minimum VLAD similarity for a keyframe to be sent back
CI_MSCKF_W = 0.05         # fixed CI weight per other agent (w0 = 1 - k*w > 0 for k <= 7)


def alg_flops(N, K, M, rows=None):
    """SURVEY.md 8(d) F_alg, split into (per-feature, QR, update)."""
    L = N
    d = 2 * L - 3
    c = 6 * N + 3 * M + 1
    n = 15 + 6 * N + 3 * M
    r = K * d + 2 * M if rows is None else rows
    feat = K * (12 * 2 * L * (6 * L + 1) + 144 * L * L + 48 * L * L + 2 * d * (2 * L) ** 2 + 2 * d * d * (2 * L) + d ** 3 / 3)
    qr = 2.0 * r * c * c - (2.0 / 3.0) * c ** 3
    upd = 7.0 * n ** 3
    return feat, qr, upd


def as_written_flops(N, K, M):
    """What the reference does AS WRITTEN (and oracle/xk_oracle.c restates) per update, SURVEY 8(a): per track the dense
    A^T jac ((2L-3) x 2L x n), jac0 P jac0^T and the inverse of S; full Householder QR of the r x (n+1) stack, zero rows of
    rejected tracks included; S, its inverse, the gain and (I - K H) P as dense n^3 products."""
    L = N
    d = 2 * L - 3
    n = 15 + 6 * N + 3 * M
    r = K * d + 2 * M
    feat = K * (2.0 * d * 2 * L * n + 2.0 * d * n * n + 2.0 * d * d * n + 2.0 * d ** 3)
    slam = M * (2.0 * 2 * n * n + 2.0 * 2 * 2 * n)
    qr = 2.0 * r * (n + 1) ** 2 - (2.0 / 3.0) * (n + 1) ** 3 if r > n + 1 else 0.0
    upd = 14.0 * n ** 3
    return feat + slam + qr + upd


def csrc_sha16():
    """Hash of the kernel sources (the same one tools/summarize_prof.py stores next to the PMC numbers)."""
    hh = hashlib.sha256()
    d = os.path.join(HERE, "x_multi_agent_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".h", ".hip")):
            hh.update(open(os.path.join(d, f), "rb").read())
    return hh.hexdigest()[:16]


def pmc_of_this_round(config):
    """Per-kernel counters of profiles/<round>[_cfgN]_pmc_traffic.json -- only if they were taken from THESE kernels."""
    suf = "" if config in (4, 5) else f"_cfg{config}"
    path = os.path.join(HERE, "profiles", f"{ROUND_TAG}{suf}_pmc_traffic.json")
    if not os.path.exists(path):
        print(f"bench.py: WARNING no {os.path.relpath(path, HERE)}: roofline.traffic / per_kernel are null", file=sys.stderr)
        return None, "missing"
    d = json.load(open(path))
    if d.get("csrc_sha16") != csrc_sha16():
        print(f"bench.py: WARNING {os.path.relpath(path, HERE)} was taken from other kernel sources "
              f"({d.get('csrc_sha16')} != {csrc_sha16()}): STALE, not quoted; rerun tools/profile_round.sh", file=sys.stderr)
        return None, "stale"
    return d, "fresh"


def frame_loop(sc, frames=600, imu_per_frame=7):
    """Whole frames through the C++ mirror (host/examples/frame_loop_main.cpp), covariance resident on the device."""
    import subprocess
    import tempfile
    pkg = os.path.join(HERE, "x_multi_agent_amd")
    exe = os.path.join(pkg, "xk_frame_loop_example")
    if not os.path.exists(exe) or len(sc.get("slam_anchor_idxs", [])):
        return None
    N = sc["n_poses_max"]
    off = sc["trk_off"]
    K = len(off) - 1
    parts = [np.array([N, K, frames, imu_per_frame, 1, sc["sigma_img"]], float), sc["C_q_G"].ravel(), sc["G_p_C"].ravel(),
             np.diff(off).astype(float), sc["obs_xy"].ravel(), np.asfortranarray(sc["P"]).ravel(order="F")]
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        np.concatenate(parts).astype("<f8").tofile(fin)
        env = dict(os.environ, LD_LIBRARY_PATH=pkg + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=600)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-300:]}
        out = np.fromfile(fout, dtype="<f8")
    n = 15 + 6 * N
    ms = out[n * n + 7 * N + 16:][min(100, frames // 4):]        # (the first frames run on a host core that is still ramping up)
    return {"ms_per_frame": float(np.median(ms)), "frames_per_s": float(1e3 / np.median(ms)), "ms_mean": float(ms.mean()),
            "ms_p95": float(np.percentile(ms, 95)), "frames": int(len(ms)), "imu_steps_per_frame": imu_per_frame,
            "what": "Ekf::processImu x7 -> VioUpdater::setMeasurement -> Ekf::processUpdateMeasurement (covariance propagation, "
                    "StateManager::manage, constructUpdate, applyUpdate, State::correct, postUpdate) through the C++ mirror of the "
                    "reference API, covariance resident in HBM, wall clock per frame; the prior is restored by a device-side copy",
            "log": r.stdout.strip()[-400:]}


def cpu_baseline(sc, budget_s=20.0):
    """Time the as-written C restatement on one host core (bounded sample)."""
    from oracle import c_oracle
    so = "/tmp/libxk_oracle_native.so"
    try:
        c_oracle.build(march="native", out=so, force=True)
        L = c_oracle.lib(so)
        flags = "-O3 -march=native"
    except Exception:
        L = c_oracle.lib()
        flags = "-O3 -march=x86-64-v3 (prebuilt)"
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
        pinned = True
    except Exception:
        pinned = False
    times = []
    t_start = time.perf_counter()
    ref = None
    for i in range(3 + 20):
        t0 = time.perf_counter()
        ref = c_oracle.visual_update(sc, library=L)
        dt = time.perf_counter() - t0
        if i >= 3:
            times.append(dt)
        if time.perf_counter() - t_start > budget_s and len(times) >= 3:
            break
    try:
        os.sched_setaffinity(0, set(range(os.cpu_count())))
    except Exception:
        pass
    med = statistics.median(times)
    N, K = sc["n_poses_max"], len(sc["trk_off"]) - 1
    M = len(sc.get("slam_anchor_idxs", []))
    as_written_gf = as_written_flops(N, K, M)
    out = {"value": 1.0 / med, "unit": "updates/s", "cores": 1, "kind": "port",
           "sample": f"median of {len(times)} updates after 3 warm-ups, same inputs as the GPU run, "
                     f"oracle/xk_oracle.c {flags}, pinned={pinned}",
           "ms_per_update": 1e3 * med, "host_cpus": os.cpu_count(),
           "as_written_flops_per_update": as_written_gf,
           "approx_gflops": as_written_gf / med / 1e9}
    # footnote: the reference's dense rows x rows noise matrix (vio_updater.cpp:417), which the baseline keeps as a
    # diagonal vector -- what allocating and filling it costs on this host, where it fits in memory
    try:
        import ctypes as C
        rows = K * (2 * N - 3) + 2 * M
        nbytes = 8 * rows * rows
        avail = None
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable"):
                avail = 1024 * int(ln.split()[1])
        L.xo_dense_noise_footnote.restype = C.c_double
        if avail is not None and avail > 3 * nbytes:
            t0 = time.perf_counter()
            tr = L.xo_dense_noise_footnote(C.c_int(rows), None)
            dtn = time.perf_counter() - t0
            out["as_written_dense_R"] = {"rows": rows, "bytes": nbytes, "ms": 1e3 * dtn, "ok": tr > 0,
                                         "updates_per_s_with_it": 1.0 / (med + dtn),
                                         "note": "r = r_diag.asDiagonal() as a dense Matrix (vio_updater.cpp:417), allocated, zero-filled, "
                                                 "diagonal written, freed: the as-written cost the baseline is spared"}
        else:
            out["as_written_dense_R"] = {"rows": rows, "bytes": nbytes, "ms": None, "note": "does not fit this host's free memory three times over: not timed"}
    except Exception as e:
        out["as_written_dense_R"] = {"error": str(e)[:200]}
    # footnotes, each a few seconds: the reference's Release flags use unsafe math; and one agent
    # per core on the cores of this box (independent filters, so this is plain replication)
    try:
        so2 = "/tmp/libxk_oracle_fastmath.so"
        c_oracle.build(march="native", out=so2, force=True, extra_flags=("-ffast-math",))
        L2 = c_oracle.lib(so2)
        t2 = []
        for i in range(6):
            t0 = time.perf_counter()
            c_oracle.visual_update(sc, library=L2)
            if i:
                t2.append(time.perf_counter() - t0)
        out["fast_math"] = {"value": 1.0 / statistics.median(t2), "unit": "updates/s", "cores": 1,
                            "flags": "-O3 -march=native -ffast-math"}
    except Exception as e:  # a footnote must not take the bench line down
        out["fast_math"] = {"error": str(e)[:200]}
    try:
        import subprocess
        import tempfile
        ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        workers = max(1, min(ncpu, 64))
        reps = 3
        with tempfile.TemporaryDirectory() as td:
            f = os.path.join(td, "sc.npz")
            np.savez(f, **{k: v for k, v in sc.items() if isinstance(v, (np.ndarray, int, float))})
            cmd = [sys.executable, os.path.join(HERE, "oracle", "bench_worker.py"), f,
                   so if flags.endswith("native") else "-", str(reps)]
            procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for _ in range(workers)]
            ts = [float(p_.communicate(timeout=180)[0].strip().splitlines()[-1]) for p_ in procs]
        out["all_core"] = {"value": reps * workers / max(ts), "unit": "updates/s", "cores": workers, "host_cpus": os.cpu_count(),
                           "note": "independent agents, one process per core, 3 updates each, slowest worker's time"}
    except Exception as e:
        out["all_core"] = {"error": str(e)[:200]}
    # footnote: the true-Eigen variant of a9 / a11 / a12, if this box has Eigen3 ("absent" on this image)
    try:
        out["eigen_variant"] = c_oracle.eigen_variant(sc)
    except Exception as e:
        out["eigen_variant"] = {"error": str(e)[:200]}
    out["_ref"] = ref          # the oracle's posterior on these inputs: main() turns it into the line's `parity` block
    return out


NOMINAL_KW = dict(err_scale=0.3, outlier_frac=0.0)   # the headline shape with (nearly) every track passing the gate: see nominal_rows()


def nominal_rows(engine, synth, cfg, dev, steps, with_cpu=True, with_frame_loop=True):
    """The headline at NOMINAL work.  The default scenario plants 5 % outliers and draws the window error
    from the prior at full size; the gate's covariance is built from observability-constrained Jacobians that do not model all of
    that error, so only ~82 % of the tracks pass and 18 639 of the nominal 22 800 rows are stacked.  Here: the same shape, window
    error at 0.3 sigma of the prior, no planted outliers -- >= 95 % of the tracks pass -- on the same path, timed the same way
    (device-only replay), with its own parity check and its own CPU leg."""
    N, K, M = synth.CONFIGS[cfg]
    sc = synth.make_config(cfg, **NOMINAL_KW)
    eng = engine.Engine(N, M, K, device=dev)
    eng.stage(sc)
    # untimed: the clocks sag while the host builds scenarios and runs the CPU legs of the other configs (seconds of an idle GPU); a
    # 20-step warm-up (8 ms) has been seen to leave the 100 timed steps of a short driver run at 0.92 ms each (round 6)
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < 0.15:
        eng.run_steps(sc["sigma_img"], 100)
    t0 = time.perf_counter()
    eng.run_steps(sc["sigma_img"], steps)
    dt = time.perf_counter() - t0
    tm = eng.bench_staged(sc["sigma_img"], 2, 10)
    rows = tm["rows_stacked"]
    f_feat, f_qr, f_upd = alg_flops(N, K, M, rows=rows)
    st = tm["stages"]
    qr_ms = sum(v["ms"] for k, v in st.items() if k.startswith("xk_caqr"))
    kal_fused = st.get("xk_kalman_update", {}).get("launches", 1) == 0
    f_dom = f_qr + (f_upd if kal_fused else 0.0)
    out = {"scenario": f"BASELINE.json configs[{cfg - 1}] shape, synth.make_config({cfg}, err_scale=0.3, outlier_frac=0.0)",
           "value": steps / dt, "unit": "updates/s", "ms_per_step": 1e3 * dt / steps, "steps": steps,
           "rows_stacked": rows, "rows_nominal": K * (2 * N - 3) + 2 * M, "stages_ms": {k: v["ms"] for k, v in st.items() if v["launches"]},
           "qr_schedule": eng.caqr_status()["schedule"],
           "roofline_frac_dominant_launch": f_dom / (qr_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, "alg_flops_dominant_launch": f_dom,
           "alg_flops_update": f_feat + f_qr + f_upd}
    if with_cpu:
        from oracle import c_oracle
        eng.stage(sc)
        got = eng.visual_update_staged(sc["sigma_img"])
        P = eng.download_P()
        ts = []
        ref = None
        for i in range(4):
            t0 = time.perf_counter()
            ref = c_oracle.visual_update(sc)
            if i:
                ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        out["tracks_passing_the_gate"] = int(np.sum(ref["inlier"]))
        out["parity"] = {"rel_dP_fro": float(np.linalg.norm(P - ref["P"]) / np.linalg.norm(ref["P"])),
                         "rel_dcorrection": float(np.linalg.norm(got["correction"] - ref["correction"]) / np.linalg.norm(ref["correction"])),
                         "inlier_masks_identical": bool(np.array_equal(got["inlier"], ref["inlier"])), "bar_rel_dP": 1e-6}
        out["cpu_baseline"] = {"value": 1.0 / med, "unit": "updates/s", "cores": 1, "kind": "port",
                               "sample": "median of 3 updates after 1 warm-up, oracle/xk_oracle.c (prebuilt flags), same inputs"}
        out["speedup_vs_cpu_1core"] = out["value"] / out["cpu_baseline"]["value"]
    eng.close()
    if with_frame_loop:
        try:                                  # whole frames through the C++ mirror on the same (nominal-rows) scenario
            fl = frame_loop(sc, frames=400)
            if fl and "ms_per_frame" in fl:
                fl["ratio_to_replay"] = fl["ms_per_frame"] / out["ms_per_step"]
                fl.pop("what", None)
            out["frame_loop"] = fl
        except Exception as ex:
            out["frame_loop"] = {"error": repr(ex)[:200]}
    return out


def small_frames(engine, synth, dev, with_frame_loop=True):
    """Not a BASELINE config: the frames a running filter sees most -- a handful of tracks end, or none (SLAM rows alone).  Stacks of at most n
    nominal rows are not compressed (the reference's `rows > cols` branch, vio_updater.cpp:487): replay rate of three such
    updates and, for the MSCKF-only one, whole frames through the C++ mirror."""
    out = {}
    cases = {"eight_short_tracks_n195": dict(N=30, K=8, M=0, kw=dict(seed=4308, track_len=(4, 12))),
             "three_full_tracks_n195": dict(N=30, K=3, M=0, kw=dict(seed=4303)),
             "slam_rows_alone_n345": dict(N=30, K=0, M=50, kw=dict(seed=4242))}
    for name, c in cases.items():
        try:
            sc = synth.make_scenario(c["N"], c["K"], c["M"], **c["kw"])
            eng = engine.Engine(c["N"], c["M"], max(c["K"], 1), device=dev)
            eng.stage(sc)
            t_w = time.perf_counter()
            while time.perf_counter() - t_w < 0.1:
                eng.run_steps(sc["sigma_img"], 50)
            ts = []
            for _ in range(5):                       # (median of five: hundreds of tiny launches queued back to back stall the runtime's queue now and then)
                t0 = time.perf_counter()
                eng.run_steps(sc["sigma_img"], 100)
                ts.append((time.perf_counter() - t0) / 100)
            dt = statistics.median(ts)
            e = {"updates_per_s": 1.0 / dt, "ms_per_update": 1e3 * dt, "qr_schedule": eng.caqr_status()["schedule"],
                 "nominal_rows": int(sum(2 * (sc["trk_off"][k + 1] - sc["trk_off"][k]) - 3 for k in range(c["K"])) + 2 * c["M"])}
            eng.close()
            if with_frame_loop and c["M"] == 0:
                fl = frame_loop(sc, frames=400)
                if fl and "frames_per_s" in fl:
                    e["frames_per_s_through_the_mirror"] = fl["frames_per_s"]
            out[name] = e
        except Exception as ex:
            out[name] = {"error": repr(ex)[:200]}
    return out


def other_configs(engine, synth, with_cpu=True):
    """BASELINE.json configs 2 and 3 on the same path (one GPU, device-only replay like `value`): updates/s, stage times,
    QR roofline fraction on the rows actually stacked, and one update checked against the C oracle on the same inputs."""
    out = {}
    for cfg, steps in ((2, 200), (3, 60)):
        try:
            N, K, M = synth.CONFIGS[cfg]
            sc = synth.make_config(cfg)
            eng = engine.Engine(N, M, K)
            eng.stage(sc)
            t_w = time.perf_counter()                          # untimed: the clocks sag while the host builds the scenario
            while time.perf_counter() - t_w < 0.2:
                eng.run_steps(sc["sigma_img"], max(20, steps // 2))
            t0 = time.perf_counter()
            eng.run_steps(sc["sigma_img"], steps)
            dt = time.perf_counter() - t0
            tm = eng.bench_staged(sc["sigma_img"], 2, 10)
            st = tm["stages"]
            rows = tm["rows_stacked"]
            _, f_qr, _ = alg_flops(N, K, M, rows=rows)
            qr_ms = sum(v["ms"] for k, v in st.items() if k.startswith("xk_caqr"))
            # Systems with SLAM features whose update does not ride in the launch (config 2): the SPLIT compression factors the tracks'
            # rows only, in the 6 N pose columns + the residual -- what that launch computes is 2 r_t c_s^2 - 2/3 c_s^3
            # flops, not the whole stack's 2 r c^2 - 2/3 c^3 that SURVEY 8(d) counts for the reference's dense QR.  Both are printed;
            # the fraction of peak is taken on what the launch does.
            split = M > 0 and (15 + 6 * N + 3 * M) > 206 and eng.caqr_status()["schedule"] == 2
            f_qr_run = f_qr
            if split:
                r_t, c_s = rows - 2 * M, 6 * N + 1          # (the gated-in SLAM rows are at most 2 M of `rows`: a lower bound on the tracks' rows)
                f_qr_run = 2.0 * r_t * c_s * c_s - (2.0 / 3.0) * c_s ** 3
            e = {"workload": f"BASELINE.json configs[{cfg - 1}]: N={N}, K={K}, M={M}, n={15 + 6 * N + 3 * M}",
                 "value": steps / dt, "unit": "updates/s", "ms_per_step": 1e3 * dt / steps, "steps": steps,
                 "stages_ms": {k: v["ms"] for k, v in st.items() if v["launches"]},
                 "qr_launches": sum(v["launches"] for k, v in st.items() if k.startswith("xk_caqr")),
                 "qr_schedule": eng.caqr_status()["schedule"], "rows_stacked": rows,
                 "qr_frac_of_fp64_peak": f_qr_run / (qr_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                 "qr_alg_flops_of_the_launches": f_qr_run, "qr_alg_flops_whole_stack_dense": f_qr,
                 "split_compression": bool(split)}
            pmc_c, pmc_state_c = pmc_of_this_round(cfg)
            if pmc_c and pmc_c.get("qr_bytes_per_update"):
                # HBM-side view: PMC bytes between the L2s and the fabric per update (QR kernels) over the QR
                # stage's time, against the 8 TB/s peak -- next to the fp64-side fraction above
                e["qr_l2_fabric_bytes_per_update"] = pmc_c["qr_bytes_per_update"]
                e["qr_frac_of_hbm_peak"] = pmc_c["qr_bytes_per_update"] / (qr_ms * 1e-3) / 8.0e12
            e["pmc_file"] = pmc_state_c
            if with_cpu:
                from oracle import c_oracle
                eng.stage(sc)
                got = eng.visual_update_staged(sc["sigma_img"])
                P = eng.download_P()
                t0 = time.perf_counter()
                ref = c_oracle.visual_update(sc)
                e["cpu_ms_per_update_1core"] = 1e3 * (time.perf_counter() - t0)
                e["parity"] = {"rel_dP_fro": float(np.linalg.norm(P - ref["P"]) / np.linalg.norm(ref["P"])),
                               "inlier_masks_identical": bool(np.array_equal(got["inlier"], ref["inlier"])),
                               "inliers": int(np.sum(ref["inlier"])), "of": int(K), "bar_rel_dP": 1e-6}
            eng.close()
            out[f"config{cfg}"] = e
        except Exception as ex:      # an extra must not take the headline line down
            out[f"config{cfg}"] = {"error": repr(ex)[:300]}
    return out


def full_legs(args, engine, synth, eng, sc, sigma, dev, world, dt):
    """--full: what the benchmark measures and checks beyond the headline -- fp64 roofline of the dominant stage (per-stage
    HIP events, the fp64 ceiling probe, the PMC file of this round), whole frames through the C++ mirror, BASELINE configs 2
    and 3, the nominal-rows and small-frames legs, the single-core CPU baseline and the parity check against the C oracle
    (rank 0, after the timed steps).  Returns the fields they fill: those of the line's `config` block, those of the line."""
    N, K, M = eng.N, eng.K, eng.M
    # per-stage HIP-event timing of the same staged update (untimed region)
    tm = eng.bench_staged(sigma, 2, min(20, max(5, args.steps)))
    rows = tm["rows_stacked"]                          # gated-out tracks leave zero rows: they do no algorithmic work
    f_feat, f_qr, f_upd = alg_flops(N, K, M, rows=rows)
    f_alg = f_feat + f_qr + f_upd
    st = tm["stages"]
    qr_keys = [k for k in st if k.startswith("xk_caqr")]
    qr_ms = sum(st[k]["ms"] for k in qr_keys)
    dom = max(st.items(), key=lambda kv: kv[1]["ms"])
    pmc, pmc_state = pmc_of_this_round(args.config)
    try:                                # (the probe kernels live in the lab build of the library, include/xk_lab.h)
        pe = engine.LabEngine(2, 0, 1, device=dev)
        ceil_fma, ceil_mfma = pe.probe_fp64_peak(False), pe.probe_fp64_peak(True)
        pe.close()
    except Exception:
        ceil_fma = ceil_mfma = None
    # the Kalman update rides INSIDE the compression launch where the geometry allows it (xk_pipe_kalman): the dominant launch then
    # does the QR's and the update's algorithmic flops, and there is no Kalman stage behind it
    kal_fused = st.get("xk_kalman_update", {}).get("launches", 1) == 0
    f_dom = f_qr + (f_upd if kal_fused else 0.0)
    ach = f_dom / (qr_ms * 1e-3) / 1e12
    per_kernel = None
    if pmc:
        per_kernel = {k: {a: v for a, v in e.items() if a in ("avg_us", "l2_fabric_GBps", "mfma_util_pct", "wait_any_pct_of_wave_cycles", "l2_hit_pct")}
                      for k, e in pmc["per_kernel"].items()}
    roof = {"bound": "fp64-valu/latency",
            "bound_note": "compute-side roofline (the compulsory HBM traffic of an update is < 1 MB); the QR kernels are Householder "
                          "steps on the vector pipe -- fp64 vector and matrix peaks are the same 78.6 TFLOP/s on MI355X -- and what "
                          "binds them is the dependent chain of reflector steps and the hand-offs between merge levels (launch boundaries in "
                          "the multi-launch schedule), not flops or bytes",
            "achieved": ach, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / FP64_PEAK_TFLOPS,
            "measured_ceiling": {"v_fma_f64": ceil_fma, "v_mfma_f64_16x16x4": ceil_mfma,
                                 "frac_of_fma_ceiling": (ach / ceil_fma) if ceil_fma else None},
            "traffic": pmc["qr_bytes_per_update"] if pmc else None,
            "traffic_note": "bytes between the L2s and the fabric per update, QR kernels, PMC FETCH_SIZE (x2, gfx950) + WRITE_SIZE from "
                            f"profiles/{ROUND_TAG}_pmc_traffic.json; Infinity-Cache hits are included (no counter separates them)",
            "pmc_file": pmc_state, "per_kernel": per_kernel,
            "kernel": ("xk_caqr_pipe (Householder QR compression of the stacked [H|res]: ONE launch, the row stack resident in "
                       "registers, the three levels of the CAQR tree pipelined on workgroups of their own"
                       + ("; the Kalman update -- gain, P = (I - K H) P, correction -- applied block by block inside the same launch as "
                          "the panels' rows of R become final, on the one workgroup the tree does not need" if kal_fused else "")
                       + "; stage keys " + "+".join(qr_keys) + ")") if tm.get("n_levels") == 1 else
                      "+".join(qr_keys) + " (Householder QR compression of the stacked [H|res], multi-launch CAQR)",
            "alg_flops_per_update": f_dom, "alg_flops_qr": f_qr, "alg_flops_kalman_in_the_launch": (f_upd if kal_fused else 0.0),
            "kalman_update_inside_the_launch": kal_fused, "rows_stacked": rows, "stage_ms": qr_ms,
            "launches_per_update": sum(st[k]["launches"] for k in qr_keys),
            "dominant_kernel_by_time": dom[0], "dominant_kernel_ms": dom[1]["ms"],
            "dominant_kernel_launches": dom[1]["launches"],
            "whole_update": {"alg_flops": f_alg, "ms": tm["total_ms"],
                             "achieved": f_alg / (tm["total_ms"] * 1e-3) / 1e12,
                             "frac": f_alg / (tm["total_ms"] * 1e-3) / 1e12 / FP64_PEAK_TFLOPS},
            "stages_ms": {k: v["ms"] for k, v in st.items() if v["launches"]},
            "dtype_peak_note": "fp64 dense peak, vector = matrix = 78.6 TFLOP/s (AMD public MI355X spec)"}
    # what the device path computes on these inputs (untimed; checked against the CPU baseline's result below)
    gpu_res = None
    if world == 1 and not args.no_cpu:
        eng.stage(sc)
        gpu_res = eng.visual_update_staged(sigma)
        gpu_res["P"] = eng.download_P()
    fl = None
    if world == 1 and not args.no_frame_loop and args.config in (1, 3, 4):
        eng.close()                       # the mirror creates its own handle
        fl = frame_loop(sc)
        if fl and "ms_per_frame" in fl:
            fl["ratio_to_replay"] = fl["ms_per_frame"] / (1e3 * dt / args.steps)
    others = None
    if world == 1 and args.config == 4 and not args.no_other_configs:
        try:
            eng.close()
        except Exception:
            pass
        others = other_configs(engine, synth, with_cpu=not args.no_cpu)
    nominal = None
    if world == 1 and args.config in (4, 5) and not args.no_other_configs:
        try:
            nominal = nominal_rows(engine, synth, args.config, dev, max(100, min(args.steps, 1000)), with_cpu=not args.no_cpu,
                                   with_frame_loop=not args.no_frame_loop)
            # (the nominal-rows scenario is the one to read against BASELINE.md's F_alg = 2.008 GFLOP)
            roof["frac_at_nominal_rows"] = nominal.get("roofline_frac_dominant_launch")
            roof["achieved_at_nominal_rows"] = (nominal["roofline_frac_dominant_launch"] * FP64_PEAK_TFLOPS
                                                if nominal.get("roofline_frac_dominant_launch") is not None else None)
        except Exception as ex:      # an extra must not take the headline line down
            nominal = {"error": repr(ex)[:300]}
    small = None
    if world == 1 and args.config in (4, 5) and not args.no_other_configs:
        try:
            small = small_frames(engine, synth, dev, with_frame_loop=not args.no_frame_loop)
        except Exception as ex:
            small = {"error": repr(ex)[:200]}
    cpu = None
    parity = None
    if world == 1 and not args.no_cpu:
        cpu = cpu_baseline(sc)
        ref = cpu.pop("_ref", None)
        if ref is not None and gpu_res is not None:
            def _rel(a, b):
                nb = float(np.linalg.norm(b))
                return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / nb) if nb > 0 else float(np.linalg.norm(a))
            parity = {"rel_dP_fro": _rel(gpu_res["P"], ref["P"]), "rel_dcorrection": _rel(gpu_res["correction"], ref["correction"]),
                      "inlier_masks_identical": bool(np.array_equal(gpu_res["inlier"], ref["inlier"])),
                      "inliers": int(np.sum(ref["inlier"])), "bar_rel_dP": 1e-6,
                      "checker": "oracle/xk_oracle.c on the same inputs (the cpu_baseline leg's result; parity unpinned, DESIGN 5)"}
    value = world * args.steps / dt
    return ({"tracks_passing_the_gate_rank0": (int(np.sum(gpu_res["inlier"])) if gpu_res is not None else None), "rows_stacked_rank0": rows},
            {"value_at_nominal_rows": (nominal.get("value") if nominal else None), "nominal_rows": nominal,
             "roofline": roof, "frame_loop": fl, "other_configs": others, "small_frames": small, "parity": parity, "cpu_baseline": cpu,
             "speedup_vs_cpu_1core": (value / world / cpu["value"]) if cpu else None})


def last_step_outputs(eng, sigma):
    """What the timed path computed in its last step: the posterior covariance, the correction and the gates' results.  Every timed
    step recomputes the same update from the staged prior (xk_run_steps leaves the prior resident; a CI round restores it), so one
    more such update, untimed, hands them out; the staged prior is restored on the device afterwards."""
    got = eng.visual_update_staged(sigma)
    got["P"] = eng.download_P()
    eng.snapshot_P(restore=True)
    return got


def dump_outputs(d, got):
    """--dump-outputs: one DIR/<name>.npy per array, float64 (inlier masks as 0 / 1); arrays a config does not have are left out."""
    os.makedirs(d, exist_ok=True)
    for name, a in got.items():
        a = np.asarray(a, dtype=np.float64)
        if a.size:
            np.save(os.path.join(d, f"{name}.npy"), a)


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-run this command line under torch.distributed.run with N ranks on
    this node (rendezvous on 127.0.0.1, a free port), pass rank 0's JSON line through and return the launcher's exit code."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, XK_BENCH_SELF_LAUNCHED="1")
    env.setdefault("OMP_NUM_THREADS", "1")
    print(f"bench.py: --gpus {n} without a launcher: starting {n} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        raise SystemExit(rc)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None, help="agents = ranks = GPUs; default: WORLD_SIZE if a launcher set it, else 1")
    ap.add_argument("--steps", type=int, default=1000)     # ~0.65 s of timed work at the headline size
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--full", action="store_true", help="after the headline, the legs it does not need (full_legs): roofline, frame loop, "
                    "other configs, nominal rows, small frames, CPU baseline, parity against the C oracle")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the CPU baseline and the parity checks")
    ap.add_argument("--no-frame-loop", action="store_true", help="--full without the frame loops through the C++ mirror")
    ap.add_argument("--no-clock-ramp", action="store_true", help="skip the untimed 0.2 s clock ramp in front of the warm-up steps (profiling runs: tools/profile_round.sh counts launches)")
    ap.add_argument("--no-other-configs", action="store_true", help="--full without configs 2 / 3, nominal rows and small frames")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="rank 0 / the dry-run rank: write what the timed path computed in "
                    "its last step as DIR/<name>.npy (float64)")
    # First-contact insurance for the multi-GPU run (no multi-GPU node is available to the builder): ONE process walks rank
    # --dry-run-rank of a fleet of --dry-run-ranks agents -- rank-indexed scenario, payload sizes, ring pattern, device-side
    # pack into the RCCL send buffer, the collective itself on a ONE-RANK nccl communicator (its own slot really travels
    # through RCCL), the CI round on the receive buffer against the other agents' payloads, which are packed into that
    # buffer in HBM beforehand.  Prints a short JSON report instead of the bench line.
    ap.add_argument("--dry-run-ranks", type=int, default=0)
    ap.add_argument("--dry-run-rank", type=int, default=0)
    ap.add_argument("--dump-posterior", default=None, help="rank 0 / the dry-run rank: save the covariance the last CI round fused (no round: the resident one) as .npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dry = args.dry_run_ranks >= 2
    launched = "WORLD_SIZE" in os.environ          # torch.distributed.run (the driver's form for N > 1) or another launcher
    if args.gpus is None:
        args.gpus = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and not launched and not dry:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU) and become their launcher
        return self_launch(args.gpus)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not dry and world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks: refusing to report a "
                         f"line whose n_gpus is not what was asked for")
    if dry and world != 1:
        raise SystemExit("--dry-run-ranks is a single-process mode")
    real_world = world
    if dry:
        world, rank = args.dry_run_ranks, args.dry_run_rank
        if not 0 <= rank < world:
            raise SystemExit("--dry-run-rank outside the fleet")

    import torch
    from x_multi_agent_amd import engine, fleet, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (MI355X); no CPU fallback exists")
    # XK_BENCH_BACKEND=gloo XK_BENCH_DEVICE=0 lets several ranks share one GPU with CPU exchange buffers
    # (functional check of the N>1 path on a single-GPU box); the default is one GPU per rank over RCCL.
    backend = os.environ.get("XK_BENCH_BACKEND", "nccl")
    dev = int(os.environ.get("XK_BENCH_DEVICE", local_rank))
    torch.cuda.set_device(dev)
    dist = None
    if dry:
        import socket
        import torch.distributed as dist
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        kw = dict(device_id=torch.device("cuda", dev)) if backend == "nccl" else {}
        dist.init_process_group(backend=backend, init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, **kw)
    elif world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(backend=backend)
    xdev = f"cuda:{dev}" if backend == "nccl" else "cpu"
    pg_world = dist.get_world_size() if dist is not None else 1
    if not dry and pg_world != args.gpus:
        raise SystemExit(f"bench.py: the process group has {pg_world} ranks, --gpus asked for {args.gpus}")

    N, K, M = synth.CONFIGS[args.config]
    ci_every = 6 if args.config == 5 else CI_EVERY    # config 5: 5 Hz requests at a 30 Hz update rate
    sc = fleet.shared_scenario(synth, args.config, rank)
    eng = engine.Engine(N, M, K, device=dev)
    eng.stage(sc)
    sigma = sc["sigma_img"]

    # CI payload exchange (torch owns the buffers so RCCL sends/receives them in place)
    pay_n = eng.payload_doubles()
    ex = fleet.Exchange(dist, world, rank, pay_n, xdev, real_world=real_world)
    pay_dev = torch.zeros(pay_n, dtype=torch.float64, device=f"cuda:{dev}")
    dyn16 = np.zeros(16)
    dyn16[9] = 1.0

    # observations of the shared tracks travel next to the SimpleState payload
    tex = fleet.Exchange(dist, world, rank, CI_TRACKS * (1 + 2 * N), xdev, real_world=real_world)
    tex.send.copy_(torch.from_numpy(fleet.pack_tracks(sc, CI_TRACKS, N).ravel()))
    ci_stats = {"rounds": 0, "fused": 0}
    if dry:
        # the other agents of the virtual fleet: their scenarios (rank-indexed, as their own processes would build them), their
        # SimpleState payloads packed ON THE DEVICE by an engine of their own, straight into their slots of the receive buffers
        for v in range(world):
            if v == rank:
                continue
            scv = fleet.shared_scenario(synth, args.config, v)
            ev = engine.Engine(N, M, K, device=dev)
            ev.stage(scv)
            slot = ex.recv.view(world, pay_n)[v]
            if slot.is_cuda:
                ev.pack_payload_into(v, 0.0, dyn16, slot.data_ptr())
            else:
                tmp = torch.zeros(pay_n, dtype=torch.float64, device=f"cuda:{dev}")
                ev.pack_payload_into(v, 0.0, dyn16, tmp.data_ptr())
                slot.copy_(tmp)
            tex.recv.view(world, tex.n)[v].copy_(torch.from_numpy(fleet.pack_tracks(scv, CI_TRACKS, N).ravel()))
            ev.close()
    if args.config == 5 and world > 1:
        # keyframe database + request filter on the device (place.Database = x::Database, reference vocabulary)
        from x_multi_agent_amd import place
        trk_n = CI_TRACKS * (1 + 2 * N)
        kdb = place.Database(eng, place.load_vocabulary("visual"), PR_SCORE_THR, payload_doubles=pay_n, tracks_doubles=trk_n,
                             max_desc=256)
        pr_scene = synth.make_descriptors(96, 32, seed=0x5EED)        # the place every agent of the fleet looks at
        # what the cameras see at every tick, made before the clock starts (synthetic input, 0.5 ms of host time per view)
        n_ticks = args.steps // ci_every + 1
        seen = {}

        def view(kind, agent, tick):
            key = (kind, agent, tick)
            if key not in seen:
                seen[key] = synth.observe_descriptors(pr_scene, 4, seed=(7919 if kind == "kf" else 104729) * agent + tick)
            return seen[key]

        for t_ in range(n_ticks):
            view("kf", rank, t_), view("q", rank, t_)
            if dry:
                rsp_ = fleet.ring_requests(world, t_)[rank][1]
                asker_ = [a for a, b in fleet.ring_requests(world, t_) if b == rank]
                view("kf", rsp_, t_)
                for a_ in asker_:
                    view("q", a_, t_)
        vex = fleet.Exchange(dist, world, rank, kdb.vlad_bytes, xdev, dtype=torch.uint8, real_world=real_world)
        rex = fleet.Exchange(dist, world, rank, 2 + pay_n + trk_n, xdev, real_world=real_world)
        resp_dev = torch.zeros(2 + pay_n + trk_n, dtype=torch.float64, device=f"cuda:{dev}")
        trk_dev = torch.zeros(trk_n, dtype=torch.float64, device=f"cuda:{dev}")
        if dry:
            # virtual partners of the request/response tick: the requester that asks ME sends the VLAD of what it sees; the
            # responder I ask keeps a keyframe database of its own (its payload slot + tracks + descriptors), searches it with
            # MY VLAD and answers in the response layout
            vdbs, dry_tick = {}, [0]

            def peer_vlad(requester):
                return torch.from_numpy(kdb.compute_vlad(view("q", requester, dry_tick[0])).ravel()).to(xdev)

            def peer_response(rsp):
                if rsp not in vdbs:
                    vdbs[rsp] = place.Database(eng, place.load_vocabulary("visual"), PR_SCORE_THR, payload_doubles=pay_n,
                                               tracks_doubles=trk_n, max_desc=256)
                pv = ex.recv.view(world, pay_n)[rsp].cuda(dev).contiguous()
                tv = tex.recv.view(world, tex.n)[rsp].cuda(dev).contiguous()
                vdbs[rsp].add_keyframe(view("kf", rsp, dry_tick[0]), pv.data_ptr(), tv.data_ptr(),
                                       tag=dry_tick[0])
                out = torch.zeros(2 + pay_n + trk_n, dtype=torch.float64, device=f"cuda:{dev}")
                idx, _score, tag = vdbs[rsp].find_candidate(int(rank), vex.send.cpu().numpy())
                if idx >= 0:
                    vdbs[rsp].copy_keyframe(idx, out.data_ptr() + 16, out.data_ptr() + 8 * (2 + pay_n))
                    out[0], out[1] = 1.0, float(tag)
                return out.to(xdev)

            vex.peer_answer, rex.peer_answer = peer_vlad, peer_response

    def exchange(step):
        """CI round: all-gather the snapshots over RCCL, then fuse the shared tracks against them on the device."""
        if world == 1:
            return
        if ex.send.is_cuda and args.config != 5:
            eng.pack_payload_into(rank, float(step), dyn16, ex.send.data_ptr())   # packed on the device straight into the RCCL send buffer
        else:
            eng.pack_payload_into(rank, float(step), dyn16, pay_dev.data_ptr())   # (gloo functional mode / keyframe snapshot)
            ex.send.copy_(pay_dev)
        if args.config == 5:
            # request/response mode (VIO::processOtherRequests, vio.cpp:462-496): every tick an agent stores a keyframe
            # (snapshot + tracks + descriptors, all resident in HBM), sends the binary VLAD of what it sees to one
            # responder, and fuses against the keyframe that comes back -- if the responder's database has one
            tick = step // ci_every
            if dry:
                dry_tick[0] = tick
            trk_dev.copy_(tex.send)
            torch.cuda.current_stream().synchronize()      # (torch's stream wrote trk_dev; the keyframe store copies on the engine's stream)
            kdb.add_keyframe(view("kf", rank, tick), pay_dev.data_ptr(),
                             trk_dev.data_ptr(), tag=step)
            my_vlad = torch.from_numpy(kdb.compute_vlad(view("q", rank, tick)).ravel())

            def answer(requester, vlad):
                idx, _score, tag = kdb.find_candidate(int(requester), vlad.cpu().numpy())
                if idx >= 0:
                    kdb.copy_keyframe(idx, resp_dev.data_ptr() + 16, resp_dev.data_ptr() + 8 * (2 + pay_n))
                    resp_dev[0], resp_dev[1] = 1.0, float(tag)
                    rex.send.copy_(resp_dev)

            got = fleet.request_round(vex, rex, fleet.ring_requests(world, tick), my_vlad, answer)
            (rsp, buf), = got.items()
            ci_stats["rounds"] += 1
            if float(buf[0]) == 0.0:
                return
            allp = torch.stack([ex.send, buf[2:2 + pay_n]])
            allt = torch.stack([tex.send, buf[2 + pay_n:]])
            if allp.device.type != "cuda":
                allp, allt = allp.cuda(dev), allt.cuda(dev)
            fused, _ = fleet.ci_round_device(eng, sc, 0, 2, allp, allt, CI_TRACKS, CI_MSCKF_W)
            if args.dump_posterior:
                ci_stats["P"] = eng.download_P()
            eng.snapshot_P(restore=True)
            ci_stats["fused"] += fused
            ci_stats["keyframes_received"] = ci_stats.get("keyframes_received", 0) + 1
            return
        allp, allt = ex.all_gather(), tex.all_gather()
        if allp.device.type != "cuda":           # gloo functional mode: the exchange ran on host tensors
            allp, allt = allp.cuda(dev), allt.cuda(dev)
        # the gathered snapshots stay in HBM: every per-agent stage of the CI block is batched on the device
        fused, _ = fleet.ci_round_device(eng, sc, rank, world, allp, allt, CI_TRACKS, CI_MSCKF_W)
        # A replay: like the update's posterior, the fused covariance does not become the next prior -- every round fuses the
        # staged prior with the snapshots that arrive.  (Fed back without the visual updates and the propagation between two
        # rounds, a prior that only ever takes covariance intersections grows by 1 / w0 per fusion -- 1 / 0.65 with seven other
        # agents -- and leaves the filter's numerical range after about eight rounds: XK_ESINGULAR at step ~90 of a fleet of 8.)
        if args.dump_posterior:
            ci_stats["P"] = eng.download_P()     # (checks only: what the last round fused, before the prior comes back)
        eng.snapshot_P(restore=True)
        ci_stats["rounds"] += 1
        ci_stats["fused"] += fused

    def sync():
        torch.cuda.synchronize()
        if real_world > 1 or dry:
            dist.barrier()
        torch.cuda.synchronize()

    # untimed warmup (also validates the staged path end to end)
    eng.snapshot_P()                     # the staged prior: what every CI round starts from (see exchange())
    # Clock ramp (untimed, before the W warm-up steps): the GPU has idled for seconds while the host built the scenario, and the
    # driver's W = 5 warm-up updates are 1.7 ms of work -- the K timed steps would sample the ramp, not the path (round 5: box-to-box
    # spread of the 20-step driver sample 2 %).  The same replayed update for CLOCK_RAMP_S of wall time; stated in the line.
    t_r = time.perf_counter()
    while not args.no_clock_ramp and time.perf_counter() - t_r < CLOCK_RAMP_S:
        eng.run_steps(sigma, 50)
    eng.run_steps(sigma, args.warmup)
    exchange(0)
    sync()
    t0 = time.perf_counter()
    done = 0
    while done < args.steps:
        chunk = min(ci_every, args.steps - done)
        eng.run_steps(sigma, chunk)          # `chunk` sequential updates, device-resident
        done += chunk
        if done % ci_every == 0:
            exchange(done)
    sync()
    dt = time.perf_counter() - t0
    if real_world > 1 or dry:
        tt = torch.tensor([dt], dtype=torch.float64, device=xdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())

    if args.dump_posterior and (dry or rank == 0):
        np.save(args.dump_posterior, ci_stats["P"] if "P" in ci_stats else eng.download_P())
    if args.dump_outputs and (dry or rank == 0):
        dump_outputs(args.dump_outputs, last_step_outputs(eng, sigma))
    if dry:
        rep = {"dry_run": True, "fleet": world, "rank": rank, "config": args.config, "backend": backend,
               "real_ranks_in_the_communicator": real_world, "steps": args.steps, "ms_per_step": 1e3 * dt / args.steps,
               "payload_bytes": 8 * pay_n, "ci_every": ci_every, "ci_rounds": ci_stats["rounds"], "ci_fused": ci_stats["fused"],
               "keyframes_received": ci_stats.get("keyframes_received"),
               "ring_partner_per_tick": [fleet.ring_requests(world, t)[rank][1] for t in range(min(4, world))] if args.config == 5 else None,
               "send_buffer_device": str(ex.send.device), "receive_buffer_doubles": int(ex.recv.numel())}
        print(json.dumps(rep), flush=True)
        eng.close()
        dist.destroy_process_group()
        return
    if rank == 0:
        cfg_full, line_full = full_legs(args, engine, synth, eng, sc, sigma, dev, world, dt) if args.full else ({}, {})
        value = world * args.steps / dt
        out = {"metric": "EKF updates/sec (window=30, 400 MSCKF feats)" if args.config in (4, 5)
               else f"EKF updates/sec (config {args.config})",
               "value": value, "unit": "updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "clock_ramp_s_before_warmup": (0.0 if args.no_clock_ramp else CLOCK_RAMP_S),
               "process_group": {"backend": (backend if world > 1 else None), "ranks": pg_world,
                                 "launcher": ("bench.py itself (torch.distributed.run)" if os.environ.get("XK_BENCH_SELF_LAUNCHED")
                                              else "external" if launched else None),
                                 "devices_visible": torch.cuda.device_count(), "device_of_rank0": dev},
               "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "f64", "data": "synthetic",
               "config": {"workload": f"BASELINE.json configs[{args.config - 1}]: one agent per GPU, window N={N}, "
                                      f"K={K} MSCKF tracks (L=N), M={M} SLAM features, n={15 + 6 * N + 3 * M}; "
                                      + (f"request/response every {ci_every} updates: binary-VLAD request, best keyframe of the responder's database back (ring)" if args.config == 5
                                         else f"CI payload all-gather every {ci_every} updates"),
                          "n_poses_max": N, "k_msckf": K, "m_slam": M, "agents": world,
                          "tracks_passing_the_gate_rank0": cfg_full.get("tracks_passing_the_gate_rank0"),
                          "rows_stacked_rank0": cfg_full.get("rows_stacked_rank0"),
                          "ci_every": ci_every, "payload_bytes": 8 * pay_n, "ci_tracks_per_round": CI_TRACKS,
                          "ci_replay": "every CI round fuses the STAGED prior with the snapshots that arrive and the prior is restored on the device "
                                       "afterwards (xk_snapshot_P), like every update of the replay: in the reference applyCI's posterior becomes the "
                                       "next prior (updater.cpp:155) with updates and propagation between two rounds; fed back WITHOUT those, the block "
                                       "scaling by 1 / w0 per fusion leaves the filter's range after ~8 rounds at 8 agents "
                                       "(tests/test_gpu_dense_ci.py::test_fused_covariance_fed_back_with_updates_and_propagation_between_rounds "
                                       "runs the fed-back form with filter steps in between)",
                          "ci_rounds_rank0": ci_stats["rounds"], "ci_fused_rank0": ci_stats["fused"],
                          **({"keyframes_received_rank0": ci_stats.get("keyframes_received", 0)} if args.config == 5 else {})},
               **line_full}
        print(json.dumps(out), flush=True)
    try:
        eng.close()
    except Exception:
        pass
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
