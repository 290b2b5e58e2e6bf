"""Per-proof verification on the GPU (zkg_groth16_verify_each) against the batch entry and the single verifier, by the share of invalid
proofs.  Wall clock around the synchronous calls (host clock; kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of
this tool with --legs each).  Proofs: one zklaim credential key of 8 payloads (libsnark_trusted_setup / libsnark_prove on a zklaim_ctx),
every presentation with fresh (r, s) and a changed public reference value; an invalid proof is a valid one with the sign of C flipped.
Prints one JSON line: ms[N][share][leg] = {min, median, max} over --reps timed calls after one warm-up round; the legs alternate within a
round (serial: zkg_groth16_verify one item after another; batch: zkg_groth16_verify_batch; each: zkg_groth16_verify_each), and their
verdicts are asserted equal.
Usage: python tools/verify_each_time.py [--k 8] [--ns 1 64 1024] [--shares none one half all] [--legs serial batch each] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zklaim_amd as zkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--ns", nargs="*", type=int, default=[1, 64, 1024])
ap.add_argument("--shares", nargs="*", default=["none", "one", "half", "all"])
ap.add_argument("--legs", nargs="*", default=["serial", "batch", "each"])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
cli = ap.parse_args()
zkg.init(0)

keep = []
pls = [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i)
       for i in range(cli.k)]
ctx = zkg.make_ctx(pls, keep)
assert zkg.libsnark_trusted_setup(ctx) == 0
head = ctx.pl_ctx_head.contents
vk = zkg.ctx_blob(ctx, "vk")
valid = []
for j in range(max(cli.ns)):
    head.pl.data_ref[0] = 2100 + j % 97                     # a changed public reference value; the claim attr0 < ref still holds
    assert zkg.libsnark_prove(ctx) == 0
    valid.append((vk, zkg.zklaim_input_map(ctx), zkg.ctx_blob(ctx, "proof")))


def spoiled(item):
    b = bytearray(item[2]); b[133] ^= 1                     # -C: decodes, fails its equation
    return (item[0], item[1], bytes(b))


def mix(n, share):
    bad = {"none": [], "one": [n // 2], "half": list(range(0, n, 2)), "all": list(range(n))}[share]
    items = list(valid[:n])
    for p in bad:
        items[p] = spoiled(items[p])
    expect = np.zeros(n, np.uint8); expect[bad] = 1
    return items, expect


LEGS = {"serial": lambda items: np.array([zkg.groth16_verify(*it) for it in items], np.uint8),
        "batch": zkg.groth16_verify_batch, "each": zkg.groth16_verify_each}
res = {"tool": "verify_each_time", "payloads": cli.k, "reps": cli.reps, "ms": {}, "each_stats": {}}
for n in cli.ns:
    res["ms"][n] = {}; res["each_stats"][n] = {}
    for share in cli.shares:
        if share == "one" and n == 1:
            continue                                        # the same batch as "all"
        items, expect = mix(n, share)
        ts = {leg: [] for leg in cli.legs}
        for rep in range(cli.reps + 1):                     # round 0 is the warm-up
            for leg in cli.legs:
                t0 = time.perf_counter(); got = LEGS[leg](items); dt = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(got, expect), (n, share, leg)
                if leg == "each":
                    res["each_stats"][n][share] = zkg.verify_each_stats()
                if rep:
                    ts[leg].append(dt)
        res["ms"][n][share] = {leg: {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)} for leg, v in ts.items()}
line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
zkg.lib().zkg_compat_reset()
zkg.shutdown()
