"""Batch verification against the single verifier, wall clock around the synchronous calls (host clock; kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this tool).  Proofs: zklaim credential keys at 1, 8 and 20 payloads (libsnark_trusted_setup /
libsnark_prove on a zklaim_ctx, the resident-key prover path), every presentation with fresh (r, s) and a changed public reference value.
Prints one JSON line:
  batch_ms[k][N]      zkg_groth16_verify_batch of N proofs under one key (k payloads), median of --reps calls after one warm-up call
  serial_ms[k][N]     the same N items through zkg_groth16_verify one after another
  multi_vk_ms         1024 items spread over 8 keys (8 payloads each), batch and serial
Usage: python tools/verify_batch_time.py [--ks 1 8 20] [--ns 1 64 1024 4096] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zklaim_amd as zkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ks", nargs="*", type=int, default=[1, 8, 20])
ap.add_argument("--ns", nargs="*", type=int, default=[1, 64, 1024, 4096])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
cli = ap.parse_args()
zkg.init(0)


def credential(k, salt, keep):
    pls = [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=salt + i)
           for i in range(k)]
    ctx = zkg.make_ctx(pls, keep)
    keep.append(ctx)
    assert zkg.libsnark_trusted_setup(ctx) == 0
    return ctx


def presentations(ctx, n):
    head = ctx.pl_ctx_head.contents
    vk = zkg.ctx_blob(ctx, "vk")
    items = []
    for j in range(n):
        head.pl.data_ref[0] = 2100 + j % 97                 # a changed public reference value; the claim attr0 < ref still holds
        assert zkg.libsnark_prove(ctx) == 0
        items.append((vk, zkg.zklaim_input_map(ctx), zkg.ctx_blob(ctx, "proof")))
    return items


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), r


def batch_ms(items):
    got = zkg.groth16_verify_batch(items)                   # warm-up (key preparation, code objects)
    assert not got.any()
    ms, got = timed(lambda: zkg.groth16_verify_batch(items), cli.reps)
    assert not got.any()
    return round(ms, 3)


def serial_ms(items):
    ms, v = timed(lambda: [zkg.groth16_verify(*it) for it in items], 1)
    assert not any(v)
    return round(ms, 3)


res = {"tool": "verify_batch_time", "batch_ms": {}, "serial_ms": {}, "speedup": {}}
keep = []
nmax = max(cli.ns)
for k in cli.ks:
    ctx = credential(k, 0x5A4B, keep)
    items = presentations(ctx, nmax)
    res["batch_ms"][k] = {}; res["serial_ms"][k] = {}; res["speedup"][k] = {}
    for n in cli.ns:
        b = batch_ms(items[:n]); s = serial_ms(items[:n])
        res["batch_ms"][k][n] = b; res["serial_ms"][k][n] = s; res["speedup"][k][n] = round(s / b, 2)
    zkg.lib().zkg_compat_reset()
multi = []
for v in range(8):
    ctx = credential(8, 0x7000 + 97 * v, keep)
    multi += presentations(ctx, 128)
multi = [multi[128 * (j % 8) + j // 8] for j in range(1024)]          # interleaved keys
b = batch_ms(multi); s = serial_ms(multi)
res["multi_vk_ms"] = {"n": 1024, "keys": 8, "payloads": 8, "batch_ms": b, "serial_ms": s, "speedup": round(s / b, 2)}
line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
