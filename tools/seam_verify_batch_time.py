"""The seam's batch verification (zkg_zklaim_verify_batch) against the paths a verifier service had before it, wall clock around the
synchronous calls (host clock).  One key per payload count through the seam (libsnark_trusted_setup), 64 distinct presentations proved on
it (zkg_zklaim_prove_batch), N contexts verified, the presentations repeated to fill the batch.  --reps repetitions after one warm-up call,
min / median / max in ms, for four legs:
  a  a loop of libsnark_verify
  b  the items built by hand: zkg_zklaim_input_map per context into its zkg_verify_item, then zkg_groth16_verify_batch (the path before
     this entry existed; b_input_map: the part of it spent in the input maps)
  c  zkg_zklaim_verify_batch with the device front end for every group (this process sets ZKG_SEAM_GPU_VERIFY=1 before the library reads it)
  d  leg c in a child process started with ZKG_SEAM_GPU_VERIFY=0 (the host front end)
The yardstick is leg b: `device_keeps` says per shape whether c's median stays within b's median plus b's own max - min.
Prints one JSON line.  --laps: one call of legs b and c per shape, for a run with ZKG_VERIFY_BATCH_LAPS=1 (the lap lines go to stderr behind
a `# k N leg` line each).
Usage: python tools/seam_verify_batch_time.py [--ks 1 8 20] [--ns 64 1024 4096] [--reps 5] [--out FILE] [--laps]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("ZKG_SEAM_GPU_VERIFY", "1")           # leg c measures the device front end whatever the default for a group is
import zklaim_amd as zkg  # noqa: E402
from zklaim_amd.api import VerifyItem  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ks", nargs="*", type=int, default=[1, 8, 20])
ap.add_argument("--ns", nargs="*", type=int, default=[64, 1024, 4096])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
ap.add_argument("--laps", action="store_true")
ap.add_argument("--only-c", action="store_true", help="leg c alone (what the child process of leg d runs)")
cli = ap.parse_args()
DISTINCT = 64


def payloads(k, v):
    pls = [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i)
           for i in range(k)]
    pls[0] = dict(pls[0], attrs=[1980 + v % 97, 0, 42 + v, 0, 5], refs=[2100 + v, 0, 41, 0, 5], salt=0x7300 + v)
    return pls


def contexts(k, keep):
    owner = zkg.make_ctx(payloads(k, 0), keep)
    assert zkg.libsnark_trusted_setup(owner) == 0
    ctxs = []
    for v in range(DISTINCT):
        c = zkg.make_ctx(payloads(k, v), keep)
        c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
        ctxs.append(c)
    assert zkg.zklaim_prove_batch(ctxs) == [0] * DISTINCT
    return ctxs


def timed(fn, reps):
    fn()                                                    # warm-up (key preparation, code objects, workspaces)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"min": round(min(ts), 3), "median": round(statistics.median(ts), 3), "max": round(max(ts), 3)}


L = zkg.lib()
L.zkg_zklaim_input_map.restype = C.c_size_t
L.zkg_zklaim_input_map.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
L.zkg_groth16_verify_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
L.zkg_zklaim_verify_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
L.libsnark_verify.argtypes = [C.c_void_p]


class Shape:
    """N contexts of one key and everything the legs need allocated ahead, so that the timed regions hold the library calls only"""

    def __init__(self, ctxs, n):
        self.n = n
        self.ctxs = [ctxs[i % DISTINCT] for i in range(n)]
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
        self.map_ms = 0.0

    def leg_a(self):
        fn = L.libsnark_verify
        assert not any(fn(a) for a in self.addr)

    def leg_b(self):
        fn = L.zkg_zklaim_input_map
        t0 = time.perf_counter()
        for a, p in zip(self.addr, self.in_ptr):
            fn(a, p, self.l)
        self.map_ms = (time.perf_counter() - t0) * 1e3
        assert L.zkg_groth16_verify_batch(C.cast(self.items, C.c_void_p), self.n, self.verdicts.ctypes.data_as(C.c_void_p)) == 0
        assert not self.verdicts.any()

    def leg_c(self):
        assert L.zkg_zklaim_verify_batch(self.ptrs, self.n, self.rc) == 0
        assert not any(self.rc)


def main():
    res = {"tool": "seam_verify_batch_time", "reps": cli.reps, "distinct": DISTINCT, "legs": {}}
    keep = []
    for k in cli.ks:
        ctxs = contexts(k, keep)
        res["legs"][k] = {}
        for n in cli.ns:
            sh = Shape(ctxs, n)
            if cli.laps:
                sys.stderr.write(f"# k={k} N={n} warm-up\n"); sys.stderr.flush()
                sh.leg_b(); sh.leg_c()                      # warm, then one call each behind its header
                for leg, fn in (("b", sh.leg_b), ("c", sh.leg_c)):
                    sys.stderr.write(f"# k={k} N={n} leg={leg}\n"); sys.stderr.flush()
                    fn()
                continue
            row = {}
            if not cli.only_c:
                row["a"] = timed(sh.leg_a, cli.reps)
                row["b"] = timed(sh.leg_b, cli.reps)
                row["b_input_map"] = round(sh.map_ms, 3)
            row["c"] = timed(sh.leg_c, cli.reps)
            row["c_stats"] = list(zkg.zklaim_verify_batch_stats())
            res["legs"][k][n] = row
        zkg.lib().zkg_compat_reset()
    if cli.laps:
        return
    if not cli.only_c:
        # leg d: this tool's leg c in a process of its own, the switch set before the library reads it
        env = dict(os.environ, ZKG_SEAM_GPU_VERIFY="0")
        cmd = [sys.executable, os.path.abspath(__file__), "--only-c", "--reps", str(cli.reps), "--ks", *map(str, cli.ks), "--ns", *map(str, cli.ns)]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-4000:])
            raise SystemExit(f"leg d: the child process failed ({out.returncode})")
        child = json.loads(out.stdout.strip().splitlines()[-1])
        res["device_keeps"] = {}
        for k in cli.ks:
            res["device_keeps"][k] = {}
            for n in cli.ns:
                row = res["legs"][k][n]
                row["d"] = child["legs"][str(k)][str(n)]["c"]
                row["d_stats"] = child["legs"][str(k)][str(n)]["c_stats"]
                res["device_keeps"][k][n] = row["c"]["median"] <= row["b"]["median"] + (row["b"]["max"] - row["b"]["min"])
    line = json.dumps(res)
    print(line)
    if cli.out:
        with open(cli.out, "w") as f:
            f.write(line + "\n")


main()
zkg.shutdown()
