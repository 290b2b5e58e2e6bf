"""Milliseconds for `count` multi-exponentiations over one resident base set (zkg_msm_g1_bases_upload), two ways, in one process on one box:
  (a) sync   a loop of `count` zkg_msm_g1_resident calls, each returning its point to the host (the host epilogue per call)
  (b) async  ONE zkg_msm_g1_resident_async call over the `count` vectors (groups of zkg_msm_g1_resident_batch_max share a sort, an
             accumulation, a fold and a reduction; the epilogue is k_msm_combine on the device), then ONE stream synchronisation
for n = 2^16 and 2^20 points and count = 1, 4, 16 (--logs, --counts).  Host clock around the calls, scalars resident and everything allocated
outside the clock; one warm-up of each leg, then --reps repetitions with the legs alternated; min / median / max per leg, in ms for all
`count` vectors.  The points of the two legs are compared.  The figures are reported, not judged: the yardstick for leg (a) is the same leg on
a build of the parent commit (--commit names the source state in the JSON).
Usage: python tools/msm_resident_async_time.py [--logs 16 20] [--counts 1 4 16] [--reps 5] [--out profiles/msm_resident_async_time.json]"""
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
ap.add_argument("--logs", nargs="*", type=int, default=[16, 20])
ap.add_argument("--counts", nargs="*", type=int, default=[1, 4, 16])
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


res = {"tool": "msm_resident_async_time", "commit": cli.commit, "reps": cli.reps, "device": zkg.device_info(), "notes": cli.note,
       "unit": "ms for all `count` vectors", "sizes": {}}
for lg in cli.logs:
    n = 1 << lg
    d_k = torch.from_numpy(bench.splitmix_fr(n, 0x5A4B4C41494D0001).view(np.int64)).cuda()
    d_bases = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    zkg.fixed_base_g1_dev(bench.G1_GEN_MONT, d_k.data_ptr(), n, d_bases.data_ptr())
    torch.cuda.synchronize()
    del d_k
    h = zkg.ResidentBases(d_bases.data_ptr(), n)
    cmax = max(cli.counts)
    d_sc = torch.from_numpy(bench.splitmix_fr(n * cmax, 0x5A4B4C41494D0002 + lg).reshape(cmax, n, 4).view(np.int64)).cuda()
    d_out = torch.zeros((cmax, 12), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    size = {"batch_max": h.batch_max(), "counts": {}}
    for count in cli.counts:
        def sync_leg():
            return np.stack([h.msm(d_sc[i].data_ptr(), stream=stream.cuda_stream) for i in range(count)])

        def async_leg():
            h.msm_async(d_sc.data_ptr(), d_out.data_ptr(), count=count, stream=stream.cuda_stream)
            stream.synchronize()

        want = sync_leg(); async_leg()                                   # warm-up of both legs (the workspace grows here)
        same = bool(np.array_equal(d_out[:count].cpu().numpy().view(np.uint64), want))
        t = {"sync": [], "async": []}
        for _ in range(cli.reps):
            for name, fn in (("sync", sync_leg), ("async", async_leg)):
                t0 = time.perf_counter()
                fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
        r = {"sync": stats(t["sync"]), "async": stats(t["async"]), "async_stats": zkg.msm_resident_async_stats(), "same_points": same}
        size["counts"][count] = r
        print(f"n=2^{lg} count={count:2d}  sync {r['sync']}  async {r['async']}  groups {r['async_stats'][1]} host waits {r['async_stats'][2]}  same points {same}", flush=True)
    res["sizes"][f"2^{lg}"] = size
    h.free()
    del d_sc, d_out, d_bases
line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
zkg.shutdown()
