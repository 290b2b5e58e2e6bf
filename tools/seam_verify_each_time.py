"""The seam's per-proof verification (zkg_zklaim_verify_each) against what a verifier service had before it, wall clock around the
synchronous calls (host clock; kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool with --legs each).
One key at 1 payload and one at 8; N contexts (64 distinct presentations, repeated) with none / one / all of them invalid, an invalid proof
being a valid one with the sign of C flipped.  Legs, alternating within a round, one warm-up round and then --reps timed ones:
  a  a serial libsnark_verify loop
  b  zkg_zklaim_verify_batch (the default front end per group)
  c  zkg_zklaim_input_map per context and then zkg_groth16_verify_each on the items, the input maps inside the timed region: what a caller
     who wants exact verdicts does today
  d  zkg_zklaim_verify_each; its first call per key, before the rounds, is the one that builds the key's bit table (d_cold, at the largest N)
All return codes are asserted equal.  Prints one JSON line: ms[k][N][share][leg] = {min, median, max}.
Usage: python tools/seam_verify_each_time.py [--ks 1 8] [--ns 64 1024] [--shares none one all] [--legs a b c d | each] [--reps 5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zklaim_amd as zkg  # noqa: E402
from zklaim_amd.api import VerifyItem  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ks", nargs="*", type=int, default=[1, 8])
ap.add_argument("--ns", nargs="*", type=int, default=[64, 1024])
ap.add_argument("--shares", nargs="*", default=["none", "one", "all"])
ap.add_argument("--legs", nargs="*", default=["a", "b", "c", "d"], help="a b c d, or `each`: the new entry alone (for a kernel trace)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
cli = ap.parse_args()
LEGS = ["d"] if cli.legs == ["each"] else cli.legs
DISTINCT = 64


def payloads(k, v):
    pls = [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i)
           for i in range(k)]
    pls[0] = dict(pls[0], attrs=[1980 + v % 97, 0, 42 + v, 0, 5], refs=[2100 + v, 0, 41, 0, 5], salt=0x7400 + v)
    return pls


def contexts(k, keep):
    """64 proved presentations of one key and, for each, its twin with the sign of C flipped"""
    owner = zkg.make_ctx(payloads(k, 0), keep)
    assert zkg.libsnark_trusted_setup(owner) == 0
    good, bad = [], []
    for v in range(DISTINCT):
        c = zkg.make_ctx(payloads(k, v), keep)
        c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
        good.append(c)
    assert zkg.zklaim_prove_batch(good) == [0] * DISTINCT
    for v, g in enumerate(good):
        c = zkg.make_ctx(payloads(k, v), keep)
        c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
        buf = bytearray(zkg.ctx_blob(g, "proof")); buf[133] ^= 1             # -C: decodes, fails its equation
        held = (C.c_ubyte * 134)(*buf); keep.append(held)
        c.proof, c.proof_size = C.addressof(held), 134
        bad.append(c)
    return good, bad


L = zkg.lib()
L.zkg_zklaim_input_map.restype = C.c_size_t
L.zkg_zklaim_input_map.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
L.zkg_groth16_verify_each.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
L.zkg_zklaim_verify_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
L.zkg_zklaim_verify_each.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
L.libsnark_verify.argtypes = [C.c_void_p]


class Shape:
    """N contexts of one key and everything the legs need allocated ahead, so that the timed regions hold the library calls only"""

    def __init__(self, good, bad, n, share):
        self.n = n
        spoiled = {"none": set(), "one": {n // 2}, "all": set(range(n))}[share]
        self.ctxs = [(bad if i in spoiled else good)[i % DISTINCT] for i in range(n)]
        self.expect = [1 if i in spoiled else 0 for i in range(n)]
        self.addr = [C.addressof(c) for c in self.ctxs]
        self.ptrs = (C.c_void_p * n)(*self.addr)
        self.rc = (C.c_int * n)()
        self.l = int(L.zkg_zklaim_input_map(self.addr[0], None, 0))
        self.inputs = np.zeros((n, self.l, 4), np.uint64)
        self.in_ptr = [self.inputs[i].ctypes.data for i in range(n)]
        self.items = (VerifyItem * n)()
        for i, c in enumerate(self.ctxs):
            self.items[i] = VerifyItem(c.vk, c.vk_size, self.in_ptr[i], self.l, c.proof, c.proof_size)
        self.verdicts = np.zeros(n, np.uint8)

    def a(self):
        fn = L.libsnark_verify
        return [fn(p) for p in self.addr]

    def b(self):
        assert L.zkg_zklaim_verify_batch(self.ptrs, self.n, self.rc) == 0
        return list(self.rc)

    def c(self):
        fn = L.zkg_zklaim_input_map
        for p, q in zip(self.addr, self.in_ptr):
            fn(p, q, self.l)
        assert L.zkg_groth16_verify_each(C.cast(self.items, C.c_void_p), self.n, self.verdicts.ctypes.data_as(C.c_void_p)) == 0
        return [int(v) for v in self.verdicts]

    def d(self):
        assert L.zkg_zklaim_verify_each(self.ptrs, self.n, self.rc) == 0
        return list(self.rc)


def main():
    zkg.init(0)
    res = {"tool": "seam_verify_each_time", "reps": cli.reps, "distinct": DISTINCT, "legs": LEGS, "ms": {}, "d_cold": {}, "d_stats": {}}
    keep = []
    for k in cli.ks:
        good, bad = contexts(k, keep)
        res["ms"][k] = {}; res["d_stats"][k] = {}
        if "d" in LEGS:
            # the key's table cold: everything else the call needs (code objects, the workspace at this size, the prepared key) is warm
            sh = Shape(good, bad, max(cli.ns), "none")
            for leg in ("b", "c"):
                if leg in LEGS:
                    assert getattr(sh, leg)() == sh.expect
            t0 = time.perf_counter(); got = sh.d(); dt = (time.perf_counter() - t0) * 1e3
            st = zkg.zklaim_verify_each_stats()
            assert got == sh.expect and st[3] == 1, st
            res["d_cold"][k] = {"n": sh.n, "ms": round(dt, 3)}
        for n in cli.ns:
            res["ms"][k][n] = {}; res["d_stats"][k][n] = {}
            for share in cli.shares:
                sh = Shape(good, bad, n, share)
                ts = {leg: [] for leg in LEGS}
                for rep in range(cli.reps + 1):                 # round 0 is the warm-up
                    for leg in LEGS:
                        t0 = time.perf_counter(); got = getattr(sh, leg)(); dt = (time.perf_counter() - t0) * 1e3
                        assert got == sh.expect, (k, n, share, leg)
                        if leg == "d":
                            res["d_stats"][k][n][share] = list(zkg.zklaim_verify_each_stats())
                            assert res["d_stats"][k][n][share] == [n, 0, 1, 0]
                        if rep:
                            ts[leg].append(dt)
                res["ms"][k][n][share] = {leg: {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)} for leg, v in ts.items()}
        zkg.lib().zkg_compat_reset()
    line = json.dumps(res)
    print(line)
    if cli.out:
        with open(cli.out, "w") as f:
            f.write(line + "\n")
    zkg.shutdown()


if __name__ == "__main__":
    main()
