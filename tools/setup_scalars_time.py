"""Key generation with the scalars on the host (zkg_groth16_setup) against the same with the scalars on the device (zkg_groth16_setup_dev),
on real zklaim circuits of --ks payloads (default 1, 8 and 20) in one process:
  (a) calls          host clock around each entry, the two alternated, --reps repetitions after one warm-up of each; median, min, max
  (b) scalars        what the two paths spend before the fixed-base batches, from the ZKG_DEBUG_TIMING laps of the same calls: the host path's
                     `lagrange` and `qap evaluation + scalars`, the device path's `qap handle` (host checks and the upload of the matrices) and
                     `qap instance + scalars (device)` (index build, Lagrange kernel, gathers, powers and combination kernels; the generator
                     synchronises before that lap when the laps are on).  And the instance call alone on a handle whose index exists, the
                     stream synchronised: host clock, median
  (c) columns        the largest column degree per matrix of the stored (possibly swapped) system, the columns above LONG_COLUMN = 24 and the
                     segments of 2048 terms they make
  (d) index_build    the first instance call of a fresh handle (index build and its wait included) minus the median of the later ones
The keys of the two entries are compared (vk blob, A, B_g1, B_g2, H, L arrays).  The figures are reported, not judged.
Usage: python tools/setup_scalars_time.py [--ks 1 8 20] [--reps 5] [--out profiles/setup_scalars_time.json]"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

os.environ["ZKG_DEBUG_TIMING"] = "1"                                    # read once by the library, at the first call of each entry

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import zklaim_amd as zkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ks", nargs="*", type=int, default=[1, 8, 20])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--commit", default=None)
ap.add_argument("--note", action="append", default=[])
ap.add_argument("--out", default=None)
cli = ap.parse_args()

import torch  # noqa: E402

zkg.init(0)
LONG_COLUMN, COLUMN_SEGMENT = 24, 2048


def stats(samples):
    s = sorted(samples)
    return {"min": round(s[0], 3), "median": round(s[len(s) // 2], 3), "max": round(s[-1], 3)}


class Stderr:
    """file descriptor 2 into a temporary file for the time of a call: the library writes its laps there"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def laps(text):
    """[zkg setup] lines -> {name: ms spent in that lap} (the library prints the time since the call began)"""
    out, last = {}, 0.0
    for name, ms in re.findall(r"\[zkg setup\] (.+?)\s+([0-9.]+) ms", text):
        out[name.strip()] = float(ms) - last
        last = float(ms)
    return out


def csr_columns(cs, which):
    rp = np.ctypeslib.as_array(C.cast(getattr(cs, which + "_rowptr"), C.POINTER(C.c_uint32)), shape=(cs.num_constraints + 1,))
    nnz = int(rp[-1])
    if not nnz:
        return np.zeros(0, np.uint32)
    return np.ctypeslib.as_array(C.cast(getattr(cs, which + "_col"), C.POINTER(C.c_uint32)), shape=(nnz,))


def timed_key(cs, td, dev):
    torch.cuda.synchronize()
    with Stderr() as err:
        t0 = time.perf_counter()
        kp = zkg.Keypair(cs, td, dev=dev)
        dt = (time.perf_counter() - t0) * 1e3
    return kp, dt, laps(err.text)


res = {"tool": "setup_scalars_time", "commit": cli.commit, "reps": cli.reps, "device": zkg.device_info(), "notes": cli.note, "unit": "ms", "payloads": {}}
all_same = True
td = bench.splitmix_fr(5, 77)
for k in cli.ks:
    keep = []
    pls = [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i) for i in range(k)]
    ck = zkg.ZklaimCircuit(zkg.make_ctx(pls, keep))
    cs = ck.r1cs
    n, l = cs.num_variables, cs.num_inputs
    # warm-up of both entries, and the comparison of what they make
    host, _, _ = timed_key(cs, td, False)
    dev, _, _ = timed_key(cs, td, True)
    m = host.pk.domain_size or (1 << host.pk.log_m)
    same = host.vk_blob() == dev.vk_blob() and host.swapped == dev.swapped
    for name, count, lim in (("A_query", n + 1, 8), ("B_g1", n + 1, 8), ("B_g2", n + 1, 16), ("H_query", m - 1, 8), ("L_query", n - l, 8)):
        same = same and np.array_equal(host.array(name, count, lim), dev.array(name, count, lim))
    all_same = all_same and same
    columns = {}
    for which in "abc":                                                  # (c): the system as the key stores it
        deg = np.bincount(csr_columns(host.pk.cs, which).astype(np.int64), minlength=n + 1)
        long_ = deg[deg > LONG_COLUMN]
        columns[which] = {"nnz": int(deg.sum()), "max_degree": int(deg.max()), "untouched": int((deg == 0).sum()), "long_columns": int(len(long_)),
                          "segments": int(((long_ + COLUMN_SEGMENT - 1) // COLUMN_SEGMENT).sum())}
    swapped = bool(host.swapped)
    host.free(); dev.free()
    # (a) and (b): the two entries alternated
    t = {"host": [], "dev": []}
    lap_samples = {"host": {}, "dev": {}}
    for _ in range(cli.reps):
        for leg, is_dev in (("host", False), ("dev", True)):
            kp, dt, lp = timed_key(cs, td, is_dev)
            kp.free()
            t[leg].append(dt)
            for name, ms in lp.items():
                lap_samples[leg].setdefault(name, []).append(ms)
    lap_medians = {leg: {name: stats(v)["median"] for name, v in d.items()} for leg, d in lap_samples.items()}
    # (b) the instance call alone, (d) the index build: a fresh handle over the same matrices (not swapped: the work is the same)
    qap = zkg.Qap(cs)
    d_abc = torch.zeros((3 * (n + 1), 4), dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    t_mont = bench.splitmix_fr(1, 78)[0]                                 # any element below r serves as Montgomery limbs

    def instance():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        qap.instance_async(t_mont, d_abc.data_ptr(), n + 1, 0, stream.cuda_stream)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    first = instance()
    built = zkg.qap_instance_stats()
    later = [instance() for _ in range(max(cli.reps, 5))]
    qap.free()
    r = {"num_variables": n, "num_constraints": cs.num_constraints, "domain_size": m, "swapped": swapped, "same_key": bool(same),
         "calls": {"zkg_groth16_setup": stats(t["host"]), "zkg_groth16_setup_dev": stats(t["dev"])},
         "laps_median": lap_medians,
         "scalars": {"host_lagrange": lap_medians["host"].get("lagrange"), "host_qap_evaluation_and_scalars": lap_medians["host"].get("qap evaluation + scalars"),
                     "dev_qap_handle": lap_medians["dev"].get("qap handle"), "dev_instance_and_scalars_with_index_build": lap_medians["dev"].get("qap instance + scalars (device)"),
                     "instance_call_alone": stats(later)},
         "columns": columns,
         "index_build": {"first_call": round(first, 3), "later_calls_median": stats(later)["median"], "one_off": round(first - stats(later)["median"], 3),
                         "stats_of_first_call": list(built)}}
    res["payloads"][k] = r
    print(f"k={k} n={n} m={m} swapped={swapped} same={same}", flush=True)
    print(f"  calls   {r['calls']}", flush=True)
    print(f"  scalars {r['scalars']}", flush=True)
    print(f"  columns {columns}", flush=True)
    print(f"  index   {r['index_build']}", flush=True)
    ck.free()
    del d_abc
res["same_keys"] = bool(all_same)
line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
zkg.shutdown()
sys.exit(0 if all_same else 1)
