"""Three device-resident CI rounds for a kernel trace (run under rocprofv3 --kernel-trace, see ci_round_kernels.sh).
    --world W (2..8, default 8)   --tracks T (shared tracks, default 2)   --searched (weight -1, option "ci_weight_search" on)"""
import sys
sys.path.insert(0, '.')
import numpy as np, torch
import os as _os; _os.environ.setdefault("XK_LIB_PATH", _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "..", "..", "x_multi_agent_amd", "lab", "libxk.so"))   # the lab build: env switches, hooks, probes (include/xk_lab.h)
from x_multi_agent_amd import engine, fleet, synth


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


WORLD, TRACKS, SEARCHED = arg("--world", 8), arg("--tracks", 2), "--searched" in sys.argv
N, K, M = synth.CONFIGS[4]
scs = [fleet.shared_scenario(synth, 4, r) for r in range(WORLD)]
eng = engine.Engine(N, M, K)
eng.set_option("ci_weight_search", 1 if SEARCHED else 0)
eng.stage(scs[0]); eng.run_steps(scs[0]["sigma_img"], 2)
dyn = np.zeros(16); dyn[9] = 1
pays = np.stack([fleet.pack_payload_host(r, 0.0, dyn, scs[r]["C_q_G"], scs[r]["G_p_C"], None, None, scs[r]["P"], N, M) for r in range(WORLD)])
trks = np.stack([fleet.pack_tracks(scs[r], TRACKS, N).ravel() for r in range(WORLD)])
dev = torch.from_numpy(pays).cuda(); tdev = torch.from_numpy(trks).cuda()
for rep in range(3):
    eng.stage(scs[0]); torch.cuda.synchronize()
    fused, _ = fleet.ci_round_device(eng, scs[0], 0, WORLD, dev, tdev, TRACKS, -1.0 if SEARCHED else 0.05)
torch.cuda.synchronize()
print(f"world {WORLD}, {TRACKS} shared track(s), {'searched' if SEARCHED else 'fixed'}: fused {fused}"
      + (f", weights {[np.round(eng.ci_round_weights(j)[0], 4).tolist() for j in range(TRACKS)]}" if SEARCHED else ""))
