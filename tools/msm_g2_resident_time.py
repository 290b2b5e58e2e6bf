"""Milliseconds for `count` G2 multi-exponentiations over one fixed base set, three ways, in one process on one box:
  (a) plain     a loop of `count` zkg_msm_g2_dev calls on the bases as they are (sort, accumulation, one reduction per window, the Horner
                doublings on the host) — the yardstick: code this tool's subject does not touch
  (b) resident  a loop of `count` zkg_msm_g2_resident calls on the handle's per-window tables (zkg_msm_g2_bases_upload), each returning its
                point to the host
  (c) async     ONE zkg_msm_g2_resident_async call over the `count` vectors (groups of zkg_msm_g2_resident_batch_max share a sort, an
                accumulation, a fold and a reduction; the epilogue is k_msm_combine on the device), then ONE stream synchronisation
for n = 2^15 and 2^18 points and count = 1, 4 and the handle's batch_max (--logs, --counts; 0 stands for batch_max).  Host clock around the
calls, scalars resident and everything allocated outside the clock; one warm-up of each leg, then --reps repetitions with the legs
alternated; min / median / max per leg, in ms for all `count` vectors.  The points of the three legs are compared.  The figures are reported,
not judged.
Usage: python tools/msm_g2_resident_time.py [--logs 15 18] [--counts 1 4 0] [--reps 5] [--out profiles/msm_g2_resident_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import zklaim_amd as zkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--logs", nargs="*", type=int, default=[15, 18])
ap.add_argument("--counts", nargs="*", type=int, default=[1, 4, 0])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--commit", default=None)
ap.add_argument("--note", action="append", default=[])
ap.add_argument("--out", default=None)
cli = ap.parse_args()

import torch  # noqa: E402

zkg.init(0)


def stats(samples):
    s = sorted(samples)
    return {"min": round(s[0], 4), "median": round(s[len(s) // 2], 4), "max": round(s[-1], 4)}


res = {"tool": "msm_g2_resident_time", "commit": cli.commit, "reps": cli.reps, "device": zkg.device_info(), "notes": cli.note,
       "unit": "ms for all `count` vectors", "sizes": {}}
all_same = True
for lg in cli.logs:
    n = 1 << lg
    d_k = torch.from_numpy(bench.splitmix_fr(n, 0x5A4B4C41494D0021).view(np.int64)).cuda()
    d_bases = torch.empty((n, 16), dtype=torch.int64, device="cuda")
    zkg.fixed_base_g2_dev(bench.G2_GEN_MONT, d_k.data_ptr(), n, d_bases.data_ptr())
    torch.cuda.synchronize()
    del d_k
    h = zkg.ResidentBasesG2(d_bases.data_ptr(), n)
    bmax = h.batch_max()
    counts = sorted(set(bmax if c == 0 else c for c in cli.counts))
    cmax = max(counts)
    d_sc = torch.from_numpy(bench.splitmix_fr(n * cmax, 0x5A4B4C41494D0022 + lg).reshape(cmax, n, 4).view(np.int64)).cuda()
    d_out = torch.zeros((cmax, 24), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    size = {"batch_max": bmax, "counts": {}}
    for count in counts:
        def plain_leg():
            return np.stack([zkg.msm_g2_dev(d_bases.data_ptr(), d_sc[i].data_ptr(), n, stream=stream.cuda_stream) for i in range(count)])

        def resident_leg():
            return np.stack([h.msm(d_sc[i].data_ptr(), stream=stream.cuda_stream) for i in range(count)])

        def async_leg():
            h.msm_async(d_sc.data_ptr(), d_out.data_ptr(), count=count, stream=stream.cuda_stream)
            stream.synchronize()

        want = plain_leg(); got_b = resident_leg(); async_leg()         # warm-up of the legs (the workspace grows here)
        same = bool(np.array_equal(got_b, want) and np.array_equal(d_out[:count].cpu().numpy().view(np.uint64), want))
        all_same = all_same and same
        legs = (("plain", plain_leg), ("resident", resident_leg), ("async", async_leg))
        t = {name: [] for name, _ in legs}
        for _ in range(cli.reps):
            for name, fn in legs:
                t0 = time.perf_counter()
                fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
        r = {name: stats(t[name]) for name, _ in legs}
        r["async_stats"] = zkg.msm_resident_async_stats(); r["same_points"] = same
        size["counts"][count] = r
        print(f"n=2^{lg} count={count:2d}  plain {r['plain']}  resident {r['resident']}  async {r['async']}  groups {r['async_stats'][1]} "
              f"host waits {r['async_stats'][2]}  same points {same}", flush=True)
    res["sizes"][f"2^{lg}"] = size
    h.free()
    del d_sc, d_out, d_bases
res["same_points"] = all_same
line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
zkg.shutdown()
sys.exit(0 if all_same else 1)
