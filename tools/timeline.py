"""Per-phase shader-cycle timeline of one row wave and one grad wave of the backward kernel
(first tile of workgroup 0, transform 0), and of the transform boundaries between the tiles (write-out of the partial
gradients against the staging of the next weight image).  Run with SBI_AMD_TIMELINE=1 on the GPU box."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["SBI_AMD_TIMELINE"] = "1"
os.environ.setdefault("SBI_AMD_LIB", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbi_amd", "libsbi_amd_nsf_debug.so"))   # python -m sbi_amd._build --debug
from bench import make_data, build_estimator
from sbi_amd.inference.trainers.fused import FusedTrainStep
dev = torch.device("cuda:0")
theta, x = make_data(65536, dev)
est = build_estimator(*make_data(65536, "cpu"), dev)
st = FusedTrainStep(est)
for _ in range(3): st.step(theta, x)
torch.cuda.synchronize()
ts = st.workspace[-2048:].view(torch.int64).cpu().reshape(-1, 64)
for w, name in ((0, "row wave 0"), (4, "grad wave 0")):
    t = ts[w]
    pts = [(i, int(t[i])) for i in range(64) if int(t[i]) != 0]
    pts.sort(key=lambda a: a[1])
    if not pts:
        print(name, 'no timestamps'); continue
    t0 = pts[0][1]
    print(name, "total cycles", pts[-1][1] - t0)
    prev = t0
    for i, v in pts:
        print(f"  TS{i:2d} +{v - prev:7d}  @{v - t0:7d}")
        prev = v

# ---- transform boundaries of workgroup 0 (TSX stamps, rows 8..15 of the buffer: one row per wave, 8 slots per
# transform).  Boundary t+1 -> t: the grad waves write transform t+1's partial gradients while the row waves stage
# transform t's weight image; both then meet at S0 of transform t's first tile.
T = est.net.hyper.num_transforms
print("transform boundaries, cycles relative to the grad wave's write-out start (workgroup 0; waves 0 and 4, then the"
      " slowest of each kind)")
for t in range(T - 2, -1, -1):
    g, r = ts[8 + 4:8 + 8, 8 * (t + 1):8 * (t + 1) + 8], ts[8:8 + 4, 8 * (t + 1):8 * (t + 1) + 8]
    gs, rs = ts[8 + 4:8 + 8, 8 * t:8 * t + 8], ts[8:8 + 4, 8 * t:8 * t + 8]
    if int(g[0, 0]) == 0:
        print(f"  {t + 1} -> {t}: no stamps"); continue
    t0 = int(g[0, 0])
    f = lambda v: f"{int(v) - t0:7d}"
    print(f"  {t + 1} -> {t}: write-out {f(g[0, 0])} ..{f(g[0, 1])} (= {int(g[0, 1] - g[0, 0])}; slowest wave"
          f" {int((g[:, 1] - g[:, 0]).max())}) | stage_layer {f(r[0, 2])} ..{f(r[0, 3])} (= {int(r[0, 3] - r[0, 2])};"
          f" slowest wave {int((r[:, 3] - r[:, 2]).max())})")
    print(f"          S0 arrival: grad {f(gs[0, 4])} (last {f(gs[:, 4].max())}), row {f(rs[0, 4])} (last"
          f" {f(rs[:, 4].max())}) | release {f(gs[0, 5])}")

# ---- forward kernel: timestamps land in the noise_out buffer (debug only)
from sbi_amd.neural_nets.estimators.nsf_flow import _log_prob_call
with torch.no_grad():
    for _ in range(2):
        lp, noise = _log_prob_call(est.net, theta, x, want_noise=True)
        noise.zero_() if _ == 0 else None
torch.cuda.synchronize()
ts = noise.reshape(-1)[:4096].view(torch.int64).cpu().reshape(-1, 64)
for w in (0, 4):
    t = ts[w]
    pts = sorted([(i, int(t[i])) for i in range(64) if 0 < int(t[i]) < 2**62], key=lambda a: a[1])
    if not pts:
        print("fwd wave", w, "no timestamps"); continue
    t0 = pts[0][1]
    print("forward wave", w, "layer 1 total cycles", pts[-1][1] - t0)
    prev = t0
    for i, v in pts:
        print(f"  TSF{i:2d} +{v - prev:7d}  @{v - t0:7d}")
        prev = v
