#!/usr/bin/env python3
"""dev tool (EXPERIMENTS build): the work items of the general rows of k1z_tile_kernel, one clock record each (strip,
general tiles, a tile that is not LDS-DMA as it stands, start, end; wall clock, 10 ns ticks), and the end of the last
class-A workgroup against the end of the launch.  python tools/k1z_gen_items.py [sigma]"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import elasticdeform_amd as ed  # noqa
n = 256
sigma = float(sys.argv[1]) if len(sys.argv) > 1 else 5.0
BASE = 1 << 16
dev = torch.device("cuda", 0)
X = torch.from_numpy(np.random.default_rng(2).random((n, n, n), dtype=np.float32)).to(dev)
d = torch.from_numpy(np.random.default_rng(22).standard_normal((3, 5, 5, 5)) * sigma).to(dev)
for _ in range(5):
    ed.deform_grid(X, d, order=3, mode="mirror", prefilter=False)
torch.cuda.synchronize()
buf = torch.zeros(1 << 18, dtype=torch.int64, device=dev)
os.environ["EDHIP_DEBUG_PTR"] = "%x" % buf.data_ptr()
ed.deform_grid(X, d, order=3, mode="mirror", prefilter=False)
torch.cuda.synchronize()
del os.environ["EDHIP_DEBUG_PTR"]
b = buf.cpu().numpy()[BASE:]
nrec, end_a, end_all, t0 = (int(v) for v in b[:4])
rec = b[8:8 + 4 * min(nrec, 40000)].reshape(-1, 4)
us = 0.01
print("sigma %g: %d work items; launch start -> end %.1f us; last class-A workgroup ends at %.1f us, %.1f us before the launch's end"
      % (sigma, nrec, (end_all - t0) * us, (end_a - t0) * us, (end_all - end_a) * us))
if len(rec):
    tiles, slow, xcd = (rec[:, 0] >> 32) & 255, (rec[:, 0] >> 40) & 1, (rec[:, 0] >> 48) & 7
    dur, start, end = (rec[:, 2] - rec[:, 1]) * us, (rec[:, 1] - t0) * us, (rec[:, 2] - t0) * us
    print("general rows: first item starts at %.1f us, last item ends at %.1f us; sum of item times %.0f us"
          % (start.min(), end.max(), dur.sum()))
    print("  %-34s %6s %8s %8s %8s %8s" % ("kind", "items", "mean us", "p50", "p90", "max"))
    for s in (1, 0):
        for t in sorted(set(tiles[slow == s].tolist())):
            m = (slow == s) & (tiles == t)
            print("  %-34s %6d %8.2f %8.2f %8.2f %8.2f" % ("%d general tile(s)%s" % (t, ", staged by rows" if s else ""),
                  m.sum(), dur[m].mean(), np.median(dur[m]), np.percentile(dur[m], 90), dur[m].max()))
    print("  items per XCD: %s" % " ".join(str(int((xcd == x).sum())) for x in range(8)))
    late = np.sort(end)[-5:]
    print("  the five latest item ends: %s us" % " ".join("%.1f" % v for v in late))
