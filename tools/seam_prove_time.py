"""Milliseconds per libsnark_prove on a resident key, in ONE session on one box, by who makes the witness (host clock around the synchronous
calls; kernel times come from a separate `rocprofv3 --kernel-trace --stats` run, see --trace-only).  For every k (payloads): the key of
libsnark_trusted_setup, one context, one warm-up loop, then --reps repetitions of --calls calls; min / median / max of the repetitions' ms per
call.  Three legs, each a child process of this tool (the witness switch is read once per process, and the parent build is another library):
  parent         a build of the parent commit, given as --parent-root DIR (a tree with zklaim_amd/libzkg.so built in it)
  host_witness   this build with ZKG_SEAM_GPU_WITNESS=0: the host witness pass, this build's scalar draw
  default        this build as it comes: the witness made on the GPU (zkg_groth16_prove_zklaim)
--rounds runs the three legs that many times, alternating, so that the JSON shows the run-to-run spread next to the differences.  The default
leg also records "ceiling": Crs.prove_sparse on a ready witness of the same key and context with fixed (r, s).
Prints a table and one JSON line; --out writes the JSON to a file.
Usage: python tools/seam_prove_time.py --parent-root build_variants/parent [--ks 1 3 8 20] [--reps 5] [--calls 200] [--rounds 2] --out profiles/prove_zklaim_time.json
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/seam_prove_time.py --trace-only 8     (key setup, then 11 libsnark_prove calls at 8
                                                                                                      payloads: the run to trace, no counters with it)"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--ks", nargs="*", type=int, default=[1, 3, 8, 20])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--commit", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--trace-only", type=int, default=None, metavar="K")
ap.add_argument("--child", default=None, metavar="ROOT", help="(internal) one leg: the library of the tree at ROOT, figures as JSON")
ap.add_argument("--ceiling", action="store_true", help="(internal) the child also times Crs.prove_sparse on ready witnesses")
cli = ap.parse_args()
TRACE_CALLS = 11


def payloads(k, v):
    return [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i + 131 * v)
            for i in range(k)]


def ms_per_call(fn, calls, reps):
    for _ in range(calls // 4 + 1):                                            # warm-up: workspaces, witness tables, the confirmed key
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    out.sort()
    return {"min": round(out[0], 4), "median": round(out[len(out) // 2], 4), "max": round(out[-1], 4), "all": [round(x, 4) for x in out]}


def seam_key(zkg, k, keep):
    owner = zkg.make_ctx(payloads(k, 0), keep)
    assert zkg.libsnark_trusted_setup(owner) == 0
    ctx = zkg.make_ctx(payloads(k, 1), keep)
    ctx.pk, ctx.pk_size, ctx.vk, ctx.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
    return owner, ctx


def child(root):
    import ctypes as C
    sys.path.insert(0, root)
    import zklaim_amd as zkg
    assert os.path.dirname(os.path.abspath(zkg.__file__)) == os.path.join(os.path.abspath(root), "zklaim_amd"), zkg.__file__
    libc_free = C.CDLL(None).free
    libc_free.argtypes = [C.c_void_p]
    zkg.init(0)
    res = {}
    for k in cli.ks:
        keep = []
        owner, ctx = seam_key(zkg, k, keep)

        def prove():
            if ctx.proof:                                                      # ctx->proof is the caller's to free (zklaim_ctx_free)
                libc_free(ctx.proof)
            ctx.proof = None; ctx.proof_size = 0
            assert zkg.libsnark_prove(ctx) == 0

        prove()
        assert zkg.libsnark_verify(ctx) == 0
        rk = {"libsnark_prove_ms": ms_per_call(prove, cli.calls, cli.reps)}
        if hasattr(zkg, "prove_zklaim_stats"):
            rk["prove_zklaim_stats"] = list(zkg.prove_zklaim_stats())
        if cli.ceiling:                                                        # last: its key (the same blob, resident a second time) is loaded after the seam's figures
            import numpy as np
            core = zkg.Crs(blob=zkg.ctx_blob(owner, "pk"))
            ck = zkg.ZklaimCircuit(ctx, witness_only=True)
            w = ck.sparse_witness()
            r = np.array([3, 1, 4, 1], np.uint64); s = np.array([2, 7, 1, 8], np.uint64)
            assert core.prove_sparse(*w, r, s)[0] == 0
            rk["ceiling_prove_sparse_ms"] = ms_per_call(lambda: core.prove_sparse(*w, r, s), cli.calls, cli.reps)
            ck.free(); core.free()
        res[k] = rk
        zkg.lib().zkg_compat_reset()
    zkg.shutdown()
    print("RESULT " + json.dumps(res))


if cli.child:
    child(cli.child)
    sys.exit(0)
if cli.trace_only is not None:
    sys.path.insert(0, HERE_ROOT)
    import zklaim_amd as zkg
    zkg.init(0)
    keep = []
    owner, ctx = seam_key(zkg, cli.trace_only, keep)
    for _ in range(TRACE_CALLS):
        assert zkg.libsnark_prove(ctx) == 0
    zkg.lib().zkg_compat_reset()
    zkg.shutdown()
    sys.exit(0)

legs = [("host_witness", HERE_ROOT, {"ZKG_SEAM_GPU_WITNESS": "0"}), ("default", HERE_ROOT, {})]
if cli.parent_root:
    legs.insert(0, ("parent", os.path.abspath(cli.parent_root), {}))
res = {"tool": "seam_prove_time", "commit": cli.commit, "calls": cli.calls, "reps": cli.reps, "rounds": cli.rounds, "ks": cli.ks, "unit": "ms per libsnark_prove call",
       "legs": {name: {} for name, _, _ in legs}, "ceiling_prove_sparse": {}, "compare": {}}
for rnd in range(cli.rounds):
    for name, root, env in legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--reps", str(cli.reps), "--calls", str(cli.calls), "--ks", *map(str, cli.ks)]
        if name == "default" and rnd == 0:
            cmd.append("--ceiling")
        clean = {k: v for k, v in os.environ.items() if k != "ZKG_SEAM_GPU_WITNESS"}
        out = subprocess.run(cmd, env=dict(clean, **env), capture_output=True, text=True)
        if out.returncode != 0:
            sys.exit(f"leg {name} failed:\n{out.stderr[-3000:]}")
        got = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
        for k in cli.ks:
            g = got[str(k)]
            res["legs"][name].setdefault(str(k), {"rounds": []})["rounds"].append(g["libsnark_prove_ms"])
            if "prove_zklaim_stats" in g:
                res["legs"][name][str(k)]["prove_zklaim_stats"] = g["prove_zklaim_stats"]
            if "ceiling_prove_sparse_ms" in g:
                res["ceiling_prove_sparse"][str(k)] = g["ceiling_prove_sparse_ms"]
            print(f"round {rnd} {name:13s} k={k:2d}  {g['libsnark_prove_ms']}" + (f"  ceiling {g['ceiling_prove_sparse_ms']}" if "ceiling_prove_sparse_ms" in g else ""), flush=True)
for name, _, _ in legs:
    for k in cli.ks:
        e = res["legs"][name][str(k)]
        every = sorted(x for r in e["rounds"] for x in r["all"])
        e["min"], e["median"], e["max"] = every[0], every[len(every) // 2], every[-1]
        e["spread_pct"] = round(100 * (every[-1] - every[0]) / e["median"], 2)  # every repetition of every round of this leg: the run-to-run spread
for k in cli.ks:
    d, h = res["legs"]["default"][str(k)], res["legs"]["host_witness"][str(k)]
    c = {"default_over_host_witness_pct": round(100 * (d["median"] / h["median"] - 1), 2), "spread_pct": max(d["spread_pct"], h["spread_pct"])}
    if "parent" in res["legs"]:
        c["default_over_parent_pct"] = round(100 * (d["median"] / res["legs"]["parent"][str(k)]["median"] - 1), 2)
    res["compare"][str(k)] = c
    print(f"k={k:2d}  {c}", flush=True)
line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
