"""Milliseconds per call of the device-witness prove entries against the unchanged host-dense entries, in one process on one box (host clock
around the synchronous C calls, their arguments prepared outside the clock; kernel times come from a separate `rocprofv3 --kernel-trace --stats`
run, see --trace-only).
  single proofs at --ks payloads (default 1, 8, 37: m = 2^15, 2^18, 2^20): zkg_groth16_prove on a PINNED host witness, measured twice as two
    legs (host_a, host_b), against zkg_groth16_prove_dev on the same vector resident on the device (dev)
  batches --batches P:k (default 16:1 and 8:4: 16 one-payload items, 8 four-payload items): zkg_groth16_prove_batch with dense host items,
    twice, against zkg_groth16_prove_batch_dev on the same witnesses packed in one device buffer
One warm-up of every leg, then --reps repetitions per leg, the legs alternated (host_a, dev, host_b, host_a, ...); a repetition is --calls calls
back to back, reported as milliseconds per call; min / median / max over the repetitions.  The two host legs run the same code on the same
data: the gap between their medians is the session's noise floor, and the device leg is compared with the mean of their medians.  Proof bytes
are compared between the legs.  Prints a table and one JSON line; --out writes the JSON to a file.  --commit names the source state in the JSON.
Usage: python tools/prove_dev_time.py [--ks 1 8 37] [--batches 16:1 8:4] [--reps 5] [--calls 10] [--out profiles/prove_dev_time.json]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/prove_dev_time.py --trace-only [--ks 1 8] [--batches 16:1]
                                           (key setup, then 11 times the device leg of every size: the runs to trace, no counters with them)"""
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
ap.add_argument("--ks", nargs="*", type=int, default=[1, 8, 37])
ap.add_argument("--batches", nargs="*", default=["16:1", "8:4"], help="P:k — P items of a k-payload key")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--calls", type=int, default=10, help="calls back to back per repetition")
ap.add_argument("--commit", default=None)
ap.add_argument("--note", action="append", default=[])
ap.add_argument("--out", default=None)
ap.add_argument("--trace-only", action="store_true")
cli = ap.parse_args()
TRACE_CALLS = 11

import torch  # noqa: E402

zkg.init(0)
L = zkg.lib()
L.zkg_groth16_prove.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
L.zkg_groth16_prove_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
L.zkg_groth16_prove_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
L.zkg_groth16_prove_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]


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


def pinned(a):
    """a numpy uint64 array copied into pinned host memory -> (the torch tensor that owns it, a numpy view of it)"""
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).pin_memory()
    return t, t.numpy().view(np.uint64)


def measure(legs):
    """legs: name -> callable (one call, returns the proof bytes).  -> (name -> {min, median, max} ms per call, the legs' bytes agree)"""
    outs = {name: fn() for name, fn in legs.items()}                              # warm-up
    same = len(set(outs.values())) == 1
    samples = {name: [] for name in legs}
    for _ in range(cli.reps):
        for name, fn in legs.items():                                           # alternated
            t0 = time.perf_counter()
            for _ in range(cli.calls):
                out = fn()
            samples[name].append((time.perf_counter() - t0) * 1e3 / cli.calls)
            same = same and out == outs[name]
    res = {}
    for name, s in samples.items():
        s.sort()
        res[name] = {"min": round(s[0], 4), "median": round(s[len(s) // 2], 4), "max": round(s[-1], 4)}
    return res, same


def verdict(r):
    host = (r["host_a"]["median"] + r["host_b"]["median"]) / 2
    floor = abs(r["host_a"]["median"] - r["host_b"]["median"])
    return {"host_median_ms": round(host, 4), "noise_floor_ms": round(floor, 4), "dev_minus_host_ms": round(r["dev"]["median"] - host, 4),
            "dev_no_slower_than_noise_floor": bool(r["dev"]["median"] - host <= floor)}


def single_legs(crs, w, rs):
    n = w.shape[0]
    keep_pin, w_pin = pinned(w)
    d_w = torch.from_numpy(w.view(np.int64)).cuda()
    torch.cuda.synchronize()
    h = C.c_void_p(crs._h)

    def host():
        out = np.zeros(256, np.uint8); ln = C.c_size_t(0)
        assert L.zkg_groth16_prove(h, w_pin.ctypes.data, rs[0].ctypes.data, rs[1].ctypes.data, 1, out.ctypes.data, C.byref(ln)) == 0
        return out[:ln.value].tobytes()

    def dev():
        out = np.zeros(256, np.uint8); ln = C.c_size_t(0)
        assert L.zkg_groth16_prove_dev(h, d_w.data_ptr(), rs[0].ctypes.data, rs[1].ctypes.data, 1, out.ctypes.data, C.byref(ln), None) == 0
        return out[:ln.value].tobytes()
    return {"host_a": host, "dev": dev, "host_b": host}, (keep_pin, d_w), n


def batch_legs(crs, ws, rss):
    P, n = len(ws), ws[0].shape[0]
    pins = [pinned(w) for w in ws]
    rs_a = np.ascontiguousarray(np.stack([np.concatenate([rs[0], rs[1]]) for rs in rss]), np.uint64)
    items = (zkg.api.ProveItem * P)(*[zkg.api.ProveItem(pins[j][1].ctypes.data, None, None, None, 0, rs_a[j].ctypes.data, rs_a[j, 4:].ctypes.data) for j in range(P)])
    d_ws = torch.from_numpy(np.stack(ws).view(np.int64)).cuda()
    torch.cuda.synchronize()
    h = C.c_void_p(crs._h)

    def host():
        out = np.zeros((P, 134), np.uint8); st = np.full(P, -1, np.int32)
        assert L.zkg_groth16_prove_batch(h, C.cast(items, C.c_void_p), P, 1, out.ctypes.data, st.ctypes.data) == 0 and not st.any()
        return out.tobytes()

    def dev():
        out = np.zeros((P, 134), np.uint8); st = np.full(P, -1, np.int32)
        assert L.zkg_groth16_prove_batch_dev(h, d_ws.data_ptr(), n, P, rs_a.ctypes.data, 1, out.ctypes.data, st.ctypes.data, None) == 0 and not st.any()
        return out.tobytes()
    return {"host_a": host, "dev": dev, "host_b": host}, (pins, rs_a, items, d_ws), n


res = {"tool": "prove_dev_time", "commit": cli.commit, "reps": cli.reps, "calls_per_repetition": cli.calls, "device": zkg.device_info(), "notes": cli.note,
       "unit": "ms per call", "single": {}, "batch": {}}
for k in cli.ks:
    crs, kp, ws, keep = key_and_witnesses(k, 1)
    rs = bench.splitmix_fr(2, 9)
    legs, hold, n = single_legs(crs, ws[0], rs)
    if cli.trace_only:
        for _ in range(TRACE_CALLS):
            legs["dev"]()
    else:
        r, same = measure(legs)
        r.update(verdict(r), dev_stats=zkg.prove_dev_stats(), num_variables=int(n), domain_size=int(kp.pk.domain_size or (1 << kp.pk.log_m)), witness_bytes=int(32 * n), same_bytes=same)
        res["single"][k] = r
        print(f"single k={k:2d} n={n:8d}  host_a {r['host_a']}  dev {r['dev']}  host_b {r['host_b']}  dev - host {r['dev_minus_host_ms']:+.4f} ms"
              f" (noise floor {r['noise_floor_ms']:.4f})  same bytes {same}", flush=True)
    del legs, hold
    crs.free(); kp.free()
for spec in cli.batches:
    P, k = (int(x) for x in spec.split(":"))
    crs, kp, ws, keep = key_and_witnesses(k, P)
    rss = [bench.splitmix_fr(2, 9 + v) for v in range(P)]
    legs, hold, n = batch_legs(crs, ws, rss)
    if cli.trace_only:
        for _ in range(TRACE_CALLS):
            legs["dev"]()
    else:
        r, same = measure(legs)
        r.update(verdict(r), items=P, payloads=k, num_variables=int(n), chunk=crs.prove_batch_chunk(), dev_stats=zkg.prove_dev_stats(), same_bytes=same)
        res["batch"][spec] = r
        print(f"batch {P:2d} x k={k}  host_a {r['host_a']}  dev {r['dev']}  host_b {r['host_b']}  dev - host {r['dev_minus_host_ms']:+.4f} ms"
              f" (noise floor {r['noise_floor_ms']:.4f})  same bytes {same}", flush=True)
    del legs, hold
    crs.free(); kp.free()
if not cli.trace_only:
    line = json.dumps(res)
    print(line)
    if cli.out:
        with open(cli.out, "w") as f:
            f.write(line + "\n")
zkg.shutdown()
