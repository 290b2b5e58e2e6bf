"""Key generation with the key left on the device, in ONE session on one box (host clock around synchronous calls; nothing is judged here).
  (1) seam       wall time of libsnark_trusted_setup with ZKG_SEAM_NO_WARM=1 on contexts of --ks payloads (default 1, 8, 20): this build
                 against a build of the parent commit given as --parent-root DIR (a tree with zklaim_amd/libzkg.so built in it).  --pairs
                 alternating pairs; every leg of a pair is a fresh child process of this tool that, per size, runs one call to warm the
                 process up (code objects, fixed-base tables, allocations) and then --reps timed calls, the resident key dropped
                 (zkg_compat_reset) outside the clock.  Per size and build: min / median / max over every timed call of every pair and
                 spread_pct = (max - min) / median, next to new_over_parent_pct of the medians.  One more child per build runs each size
                 with ZKG_DEBUG_TIMING=1 and keeps the laps of its last call.
  (2) public     zkg_groth16_setup_resident against zkg_groth16_setup + zkg_keypair_pk_blob + zkg_crs_upload (the key to the host and
                 straight back) on the circuits of the same sizes under one trapdoor, in one process of this build, the two alternated,
                 --reps repetitions after a warm-up of each; the C entries are called directly, the blob buffers are not copied again.
                 The pk blobs of the two are compared.
Prints a table and one JSON line; --out writes the JSON to a file.
Usage: python tools/seam_keygen_time.py --parent-root build_variants/parent [--ks 1 8 20] [--pairs 5] [--reps 3] --out profiles/seam_keygen_dev_time.json"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--ks", nargs="*", type=int, default=[1, 8, 20])
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--commit", default=None)
ap.add_argument("--note", action="append", default=[])
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, metavar="ROOT", help="(internal) the seam leg of one build: the library of the tree at ROOT, figures as JSON")
ap.add_argument("--public", action="store_true", help="(internal) run (2) in this process")
cli = ap.parse_args()


def payloads(k, v):
    return [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i + 131 * v)
            for i in range(k)]


def stats(samples):
    s = sorted(samples)
    return {"min": round(s[0], 3), "median": round(s[len(s) // 2], 3), "max": round(s[-1], 3), "spread_pct": round(100 * (s[-1] - s[0]) / s[len(s) // 2], 2),
            "all": [round(x, 3) for x in samples]}


def seam_child(root):
    sys.path.insert(0, root)
    import zklaim_amd as zkg
    assert os.path.dirname(os.path.abspath(zkg.__file__)) == os.path.join(os.path.abspath(root), "zklaim_amd"), zkg.__file__
    import torch
    zkg.init(0)
    res = {}
    for k in cli.ks:
        ms = []
        for v in range(cli.reps + 1):                                          # the first call is the warm-up
            keep = []
            ctx = zkg.make_ctx(payloads(k, v), keep)
            torch.cuda.synchronize()
            if v == cli.reps:
                print(f"LAPS-BEGIN {k}", file=sys.stderr, flush=True)         # (the laps of the last call, when the library prints them)
            t0 = time.perf_counter()
            rc = zkg.libsnark_trusted_setup(ctx)
            dt = (time.perf_counter() - t0) * 1e3
            if v == cli.reps:
                print("LAPS-END", file=sys.stderr, flush=True)
            assert rc == 0 and ctx.pk_size > 0
            if v:
                ms.append(dt)
            rk = {"pk_size": int(ctx.pk_size)}
            if hasattr(zkg, "setup_resident_stats"):
                rk["setup_resident_stats"] = zkg.setup_resident_stats()
            zkg.lib().zkg_compat_reset()
        rk["ms"] = ms
        res[k] = rk
    zkg.shutdown()
    print("RESULT " + json.dumps(res))


def public_leg():
    import ctypes as C
    sys.path.insert(0, HERE_ROOT)
    import numpy as np
    import torch
    import bench
    import zklaim_amd as zkg
    zkg.init(0)
    L = zkg.lib()
    L.zkg_groth16_setup.restype = C.c_void_p; L.zkg_groth16_setup.argtypes = [C.c_void_p, C.c_void_p]
    L.zkg_keypair_pk.restype = C.c_void_p; L.zkg_keypair_pk.argtypes = [C.c_void_p]
    L.zkg_keypair_free.argtypes = [C.c_void_p]
    L.zkg_keypair_pk_blob.restype = C.c_size_t; L.zkg_keypair_pk_blob.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.zkg_groth16_setup_resident.argtypes = [C.c_void_p] * 7
    L.zkg_free.argtypes = [C.c_void_p]; L.zkg_free.restype = None
    td = bench.splitmix_fr(5, 77)
    res = {}
    for k in cli.ks:
        keep = []
        ck = zkg.ZklaimCircuit(zkg.make_ctx(payloads(k, 0), keep))
        cs = ck.r1cs

        def round_trip():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kp = L.zkg_groth16_setup(C.byref(cs), td.ctypes.data)
            size = L.zkg_keypair_pk_blob(kp, None, 0)
            blob = np.empty(size, np.uint8)
            assert kp and L.zkg_keypair_pk_blob(kp, blob.ctypes.data, size) == size
            crs = L.zkg_crs_upload(L.zkg_keypair_pk(kp))
            dt = (time.perf_counter() - t0) * 1e3
            assert crs
            L.zkg_crs_free(crs); L.zkg_keypair_free(kp)
            return dt, blob.tobytes()

        def resident():
            pk = C.c_void_p(None); vk = C.c_void_p(None); crs = C.c_void_p(None); pk_len = C.c_size_t(0); vk_len = C.c_size_t(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = L.zkg_groth16_setup_resident(C.byref(cs), td.ctypes.data, C.byref(pk), C.byref(pk_len), C.byref(vk), C.byref(vk_len), C.byref(crs))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, L.zkg_last_error().decode()
            blob = C.string_at(pk.value, pk_len.value)
            L.zkg_crs_free(crs); L.zkg_free(pk); L.zkg_free(vk)
            return dt, blob

        same = round_trip()[1] == resident()[1]                                # warm-up of both, and what they make
        t = {"round_trip": [], "resident": []}
        for _ in range(cli.reps):
            t["round_trip"].append(round_trip()[0])
            t["resident"].append(resident()[0])
        res[k] = {"num_variables": int(cs.num_variables), "num_constraints": int(cs.num_constraints), "same_pk_blob": bool(same),
                  "setup_resident_stats": zkg.setup_resident_stats(),
                  "zkg_groth16_setup+pk_blob+crs_upload": stats(t["round_trip"]), "zkg_groth16_setup_resident": stats(t["resident"])}
        ck.free()
    zkg.shutdown()
    print("RESULT " + json.dumps(res))


def run_child(args, env):
    clean = {k: v for k, v in os.environ.items() if k not in ("ZKG_DEBUG_TIMING", "ZKG_SEAM_NO_WARM", "ZKG_SEAM_ISSUER_ONLY")}
    out = subprocess.run([sys.executable, os.path.abspath(__file__), *args, "--reps", str(cli.reps), "--ks", *map(str, cli.ks)], env=dict(clean, **env), capture_output=True, text=True)
    if out.returncode != 0:
        sys.exit(f"child {args} failed:\n{out.stderr[-3000:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):]), out.stderr


if cli.child:
    seam_child(cli.child)
    sys.exit(0)
if cli.public:
    public_leg()
    sys.exit(0)

builds = [("new", HERE_ROOT)]
if cli.parent_root:
    builds.insert(0, ("parent", os.path.abspath(cli.parent_root)))
res = {"tool": "seam_keygen_time", "commit": cli.commit, "notes": cli.note, "unit": "ms", "ks": cli.ks, "pairs": cli.pairs, "reps": cli.reps,
       "seam": {name: {} for name, _ in builds}, "seam_laps": {}, "seam_compare": {}, "public": {}}
for pair in range(cli.pairs):
    for name, root in (builds if pair % 2 == 0 else builds[::-1]):            # the order within a pair alternates too
        got, _ = run_child(["--child", root], {"ZKG_SEAM_NO_WARM": "1"})
        for k in cli.ks:
            e = res["seam"][name].setdefault(str(k), {"ms": []})
            e["ms"] += got[str(k)]["ms"]
            e["pk_size"] = got[str(k)]["pk_size"]
            if "setup_resident_stats" in got[str(k)]:
                e["setup_resident_stats"] = got[str(k)]["setup_resident_stats"]
            print(f"pair {pair} {name:6s} k={k:2d}  {[round(x, 2) for x in got[str(k)]['ms']]}", flush=True)
for name, root in builds:
    for k in cli.ks:
        e = res["seam"][name][str(k)]
        e.update(stats(e.pop("ms")))
    _, err = run_child(["--child", root, ], {"ZKG_SEAM_NO_WARM": "1", "ZKG_DEBUG_TIMING": "1"})
    laps = {}
    for part in err.split("LAPS-BEGIN ")[1:]:
        k, _, text = part.partition("\n")
        text = text.partition("LAPS-END")[0]
        laps[k.strip()] = [f"{tag}: {what.strip()} {ms}" for tag, what, ms in re.findall(r"\[zkg ([a-z ]+)\] (.+?)\s+([0-9.]+) ms", text)]
    res["seam_laps"][name] = laps                                              # "<who>: <lap> <ms since that function began>"
for k in cli.ks:
    new = res["seam"]["new"][str(k)]
    c = {"new_median": new["median"], "new_spread_pct": new["spread_pct"]}
    if "parent" in res["seam"]:
        par = res["seam"]["parent"][str(k)]
        c.update(parent_median=par["median"], parent_spread_pct=par["spread_pct"], new_over_parent_pct=round(100 * (new["median"] / par["median"] - 1), 2))
    res["seam_compare"][str(k)] = c
    print(f"seam   k={k:2d}  {c}", flush=True)
res["public"], _ = run_child(["--public"], {})
for k in cli.ks:
    p = res["public"][str(k)]
    a, b = p["zkg_groth16_setup_resident"], p["zkg_groth16_setup+pk_blob+crs_upload"]
    p["resident_over_round_trip_pct"] = round(100 * (a["median"] / b["median"] - 1), 2)
    print(f"public k={k:2d}  resident {a['median']} ({a['min']} - {a['max']})  round trip {b['median']} ({b['min']} - {b['max']})  same blob {p['same_pk_blob']}", flush=True)
line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
