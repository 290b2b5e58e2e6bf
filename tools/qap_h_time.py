"""Milliseconds per witness of zkg_qap_witness_h_async (the QAP handle: device witnesses -> coefficients_for_H in device memory) on zklaim
systems of --ks payloads (default 1 and 8: m = 2^15 and 2^18), for --counts witnesses per call (default 1, 3, 8, 16), against two baselines
measured in the same process on the same box:
  (a) host_entry    zkg_qap_witness_h on a key over the same system: one host witness up, a prover slot leased, a wait, m x 32 bytes back —
                    the round trip the handle replaces (the output array is allocated outside the clock)
  (b) prove_stages  the mat-vec and the transform stage ([0] + [1] of zkg_prove_stage_ms, device events) of one zkg_groth16_prove of the same
                    key: the same work inside a proof, beside the proof's multi-exponentiations
The handle's legs: host clock around ONE call and the synchronisation of its stream, the device idle before the clock starts; witnesses
resident and every buffer allocated outside the clock.  One warm-up of every leg (the workspace grows there), then --reps repetitions with the
legs alternated; the median is reported, with min and max, in ms per call and ms per witness.  H of every witness of the largest count is
compared with zkg_qap_witness_h's bytes.  The figures are reported, not judged.
Usage: python tools/qap_h_time.py [--ks 1 8] [--counts 1 3 8 16] [--reps 15] [--out profiles/qap_h_time.json]"""
import argparse
import ctypes as C
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
ap.add_argument("--ks", nargs="*", type=int, default=[1, 8])
ap.add_argument("--counts", nargs="*", type=int, default=[1, 3, 8, 16])
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--commit", default=None)
ap.add_argument("--note", action="append", default=[])
ap.add_argument("--out", default=None)
cli = ap.parse_args()

import torch  # noqa: E402

zkg.init(0)
L = zkg.lib()
L.zkg_qap_witness_h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]


def stats(samples, per=1):
    s = sorted(samples)
    return {"min": round(s[0] / per, 4), "median": round(s[len(s) // 2] / per, 4), "max": round(s[-1] / per, 4)}


def key_and_witnesses(k, count):
    """one k-payload key and `count` distinct credentials' dense witnesses"""
    keep, ws, ck0 = [], [], None
    for v in range(count):
        pls = [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i + 131 * v)
               for i in range(k)]
        ck = zkg.ZklaimCircuit(zkg.make_ctx(pls, keep))
        ws.append(ck.witness())
        if ck0 is None:
            ck0 = ck
        else:
            ck.free()
    kp = zkg.Keypair(ck0.r1cs, bench.splitmix_fr(5, 77))
    return zkg.Crs(kp.pk), kp, ws, keep + [ck0]


res = {"tool": "qap_h_time", "commit": cli.commit, "reps": cli.reps, "device": zkg.device_info(), "notes": cli.note,
       "unit": "ms; per_witness = per_call / count", "payloads": {}}
all_same = True
for k in cli.ks:
    cmax = max(cli.counts)
    crs, kp, ws, keep = key_and_witnesses(k, cmax)
    qap = zkg.Qap(kp.pk.cs)                                             # the system as the key stores it: the same matrices on both sides
    n, m = qap.num_variables(), qap.domain_size()
    assert n == ws[0].shape[0] and m == (kp.pk.domain_size or (1 << kp.pk.log_m))
    h_stride = m + 1
    d_w = torch.from_numpy(np.stack(ws).view(np.int64)).cuda()
    d_h = torch.zeros((cmax, h_stride, 4), dtype=torch.int64, device="cuda")
    d_f = torch.zeros((cmax,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    rs = bench.splitmix_fr(2, 9)
    w0 = np.ascontiguousarray(ws[0]); h_out = np.zeros((m + 1, 4), np.uint64)

    def async_leg(count):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            qap.witness_h_async(d_w.data_ptr(), count, n, d_h.data_ptr(), h_stride, d_f.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3
        return run

    def host_entry():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.zkg_qap_witness_h(C.c_void_p(crs._h), w0.ctypes.data, h_out.ctypes.data)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0
        return dt

    def prove_stages():
        rc, _ = crs.prove(w0, rs[0], rs[1])
        assert rc == 0
        ms = crs.stage_ms()
        return ms[0] + ms[1]

    legs = [(f"async_{c}", async_leg(c)) for c in cli.counts] + [("host_entry", host_entry), ("prove_stages", prove_stages)]
    for _, fn in legs:                                                   # warm-up: the largest group's workspace, the prover's slot and tables
        fn()
    async_leg(cmax)()
    got = d_h.cpu().numpy().view(np.uint64).reshape(cmax, h_stride, 4)
    same = not d_f.cpu().numpy().any()
    for i in range(cmax):
        same = same and got[i].tobytes() == crs.qap_witness_h(ws[i]).tobytes()
    all_same = all_same and same
    t = {name: [] for name, _ in legs}
    for _ in range(cli.reps):
        for name, fn in legs:                                            # alternated
            t[name].append(fn())
    r = {"num_variables": n, "domain_size": m, "batch_max": qap.batch_max(), "same_bytes_as_zkg_qap_witness_h": bool(same),
         "host_entry": stats(t["host_entry"]), "prove_stages": stats(t["prove_stages"]), "counts": {}}
    for c in cli.counts:
        r["counts"][c] = {"per_call": stats(t[f"async_{c}"]), "per_witness": stats(t[f"async_{c}"], c)}
        print(f"k={k} m={m} count={c:2d}  per call {r['counts'][c]['per_call']}  per witness {r['counts'][c]['per_witness']}", flush=True)
    print(f"k={k} m={m} host entry {r['host_entry']}  prove stages [0] + [1] {r['prove_stages']}  same bytes {same}", flush=True)
    res["payloads"][k] = r
    qap.free(); crs.free(); kp.free()
    del d_w, d_h, d_f
res["same_bytes"] = bool(all_same)
line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
zkg.shutdown()
sys.exit(0 if all_same else 1)
