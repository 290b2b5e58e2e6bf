"""Proofs per second of zkg_groth16_prove_batch against the single-proof path, in one process on one box (host clock around the synchronous
calls; kernel times come from a separate `rocprofv3 --kernel-trace --stats` run, see --trace-only).  For every k (payloads) and P (batch size),
P distinct credentials of one key, sparse witnesses, fresh (r, s):
  sequential    P Crs.prove_sparse calls one after another                       (leg a)
  three_callers three threads on the key's prover slots, --caller-proofs proofs each: the figure of tools/prove_throughput.py, once per k  (leg b)
  batch         one Crs.prove_batch of the P items                              (leg c)
--reps timed repetitions each after one warm-up; min / median / max proofs/s.  The batch's bytes are compared with the sequential leg's.
Prints a table and one JSON line; --out writes the JSON to a file.  --commit names the source state in the JSON.
--seam measures the zklaim seam instead: P contexts of one key (libsnark_trusted_setup's) through a loop of libsnark_prove calls (sequential)
against one zkg_zklaim_prove_batch (batch), witness generation included in both; same output shape, no three-callers leg.  The batch is
measured per witness source: "batch" as the process is configured (GPU witnesses unless ZKG_SEAM_GPU_WITNESS=0), and — the switch is read
once per process — "batch_host_witness" from a child process of this tool with the switch off (--seam-child, not for direct use).  "core"
is zkg_groth16_prove_batch on ready-made sparse witnesses of the same key and contexts: the ceiling a seam batch can reach.
Usage: python tools/prove_batch_time.py [--ks 1 2 4] [--ps 1 2 4 8 16 32] [--reps 5] [--out profiles/prove_batch_time.json]
       python tools/prove_batch_time.py --ks 3 5 6 7 --ps 1 4 8 16        (the step-domain keys below 2^18)
       python tools/prove_batch_time.py --seam --ks 1 3 --ps 8 16
       python tools/prove_batch_time.py --seam --ks 1 --ps 1 16 --out profiles/prove_batch_gpu_witness_time.json
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/prove_batch_time.py --trace-only seam [--trace-k K]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/prove_batch_time.py --trace-only single|batch [--trace-k K]
                                           (key setup, then 11 times one proof / one batch of the key's chunk at K payloads, default 1: the runs to
                                            trace, no counters with them)
       python tools/prove_batch_time.py --merge-stats SINGLE_kernel_stats.csv BATCH_kernel_stats.csv profiles/prove_batch_kernel_stats.csv"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import zklaim_amd as zkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ks", nargs="*", type=int, default=[1, 2, 4])
ap.add_argument("--ps", nargs="*", type=int, default=[1, 2, 4, 8, 16, 32])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--caller-proofs", type=int, default=40)
ap.add_argument("--commit", default=None)
ap.add_argument("--note", action="append", default=[], help="free text recorded in the JSON (e.g. the parent build's prove_throughput lines)")
ap.add_argument("--out", default=None)
ap.add_argument("--trace-only", choices=["single", "batch", "seam"], default=None)
ap.add_argument("--trace-k", type=int, default=1, help="payload count of the --trace-only runs")
ap.add_argument("--seam", action="store_true", help="libsnark_prove loop against zkg_zklaim_prove_batch")
ap.add_argument("--seam-child", action="store_true", help="(internal) the host-witness leg: batch figures only, as JSON")
ap.add_argument("--merge-stats", nargs=3, metavar=("SINGLE_CSV", "BATCH_CSV", "OUT_CSV"), default=None)
ap.add_argument("--merge-batch-size", type=int, default=16, help="proofs per traced batch, for the column names of --merge-stats")
cli = ap.parse_args()
TRACE_CALLS = 11


def key_and_items(k, count):
    keep = []
    items = []
    ck0 = None
    for v in range(count):
        pls = [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i + 131 * v)
               for i in range(k)]
        ck = zkg.ZklaimCircuit(zkg.make_ctx(pls, keep))
        rs = bench.splitmix_fr(2, 9 + v)
        items.append(ck.sparse_witness() + (rs[0], rs[1]))
        if ck0 is None:
            ck0 = ck
    kp = zkg.Keypair(ck0.r1cs, bench.splitmix_fr(5, 77))
    return zkg.Crs(kp.pk), items, keep + [kp]


def rates(fn, proofs, reps):
    fn()                                                        # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append(proofs / (time.perf_counter() - t0))
    out.sort()
    return {"min": round(out[0], 1), "median": round(out[len(out) // 2], 1), "max": round(out[-1], 1)}


if cli.merge_stats:
    # two rocprofv3 *_kernel_stats.csv (the --trace-only single / batch runs) side by side, per kernel and per call of the traced loop
    import csv
    single, batch, out = cli.merge_stats
    rows = {}
    for col, path in ((0, single), (1, batch)):
        for r in csv.DictReader(open(path)):
            rows.setdefault(r["Name"], [[0, 0], [0, 0]])[col] = [int(r["Calls"]), int(r["TotalDurationNs"])]
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        b_ = f"batch{cli.merge_batch_size}"
        w.writerow(["Name", "single_launches", "single_total_us", b_ + "_launches", b_ + "_total_us", "traced_calls_each"])
        for name, (a, b) in sorted(rows.items(), key=lambda kv: -kv[1][1][1]):
            w.writerow([name, a[0], round(a[1] / 1e3, 1), b[0], round(b[1] / 1e3, 1), TRACE_CALLS])
    sys.exit(0)
zkg.init(0)


def seam_contexts(k, count, keep):
    """a key from libsnark_trusted_setup and `count` contexts of their own on it"""
    def payloads(v):
        return [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i + 131 * v)
                for i in range(k)]
    owner = zkg.make_ctx(payloads(0), keep)
    assert zkg.libsnark_trusted_setup(owner) == 0
    ctxs = []
    for v in range(count):
        c = zkg.make_ctx(payloads(v), keep)
        c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
        ctxs.append(c)
    return owner, ctxs


if cli.trace_only == "seam":
    keep = []
    owner, ctxs = seam_contexts(cli.trace_k, 16, keep)
    for _ in range(TRACE_CALLS):
        assert zkg.zklaim_prove_batch(ctxs) == [0] * 16
    zkg.lib().zkg_compat_reset()
    zkg.shutdown()
    sys.exit(0)
if cli.trace_only:
    crs, items, keep = key_and_items(cli.trace_k, 16)
    items = items[:crs.prove_batch_chunk() or 16]
    for _ in range(TRACE_CALLS):                                # (the first call is the warm-up: witness tables, workspaces)
        if cli.trace_only == "single":
            assert crs.prove_sparse(*items[0])[0] == 0
        else:
            assert all(g[0] == 0 for g in crs.prove_batch(items))
    crs.free()
    zkg.shutdown()
    sys.exit(0)

res = {"tool": "prove_batch_time", "commit": cli.commit, "reps": cli.reps, "device": zkg.device_info() if hasattr(zkg, "device_info") else None,
       "notes": cli.note, "results": {}}
if cli.seam:
    import ctypes as C
    libc_free = C.CDLL(None).free
    libc_free.argtypes = [C.c_void_p]
    res["leg"] = "seam"
    for k in cli.ks:
        keep = []
        owner, ctxs = seam_contexts(k, max(cli.ps), keep)
        want_core = not cli.seam_child and hasattr(zkg, "zklaim_witness_stats")

        def drop_proofs(sub):                                   # ctx->proof is the caller's to free (zklaim_ctx_free)
            for c in sub:
                if c.proof:
                    libc_free(c.proof)
                c.proof = None; c.proof_size = 0

        rk = {"P": {}}
        for P in cli.ps:
            sub = ctxs[:P]

            def loop():
                drop_proofs(sub)
                assert [zkg.libsnark_prove(c) for c in sub] == [0] * P

            def batch():
                drop_proofs(sub)
                assert zkg.zklaim_prove_batch(sub) == [0] * P

            batch()
            stats = zkg.prove_batch_stats()
            wstats = zkg.zklaim_witness_stats() if hasattr(zkg, "zklaim_witness_stats") else None
            assert all(zkg.libsnark_verify(c) == 0 for c in sub)
            if cli.seam_child:
                rk["P"][P] = {"batch": rates(batch, P, cli.reps), "batch_stats": stats, "witness_stats": wstats}
                continue
            seq = rates(loop, P, cli.reps)
            bat = rates(batch, P, cli.reps)
            rk["P"][P] = {"sequential": seq, "batch": bat, "batch_stats": stats, "witness_stats": wstats, "batch_min_over_sequential_max": round(bat["min"] / seq["max"], 3)}
            print(f"seam k={k} P={P:3d}  libsnark_prove loop {seq}  zkg_zklaim_prove_batch {bat}  batch min / loop max = {bat['min'] / seq['max']:.2f}", flush=True)
        # the ceiling last: its key (the same blob, resident a second time) is loaded only after the seam's legs have been measured
        core = zkg.Crs(blob=zkg.ctx_blob(owner, "pk")) if want_core else None
        for P in (cli.ps if core is not None else []):
            items = []
            for v, c in enumerate(ctxs[:P]):
                ck = zkg.ZklaimCircuit(c, witness_only=True)
                rs = bench.splitmix_fr(2, 9 + v)
                items.append(ck.sparse_witness() + (rs[0], rs[1]))
                ck.free()
            assert all(g[0] == 0 for g in core.prove_batch(items))
            rk["P"][P]["core"] = rates(lambda: core.prove_batch(items), P, cli.reps)
        drop_proofs(ctxs)
        if core is not None:
            core.free()
        res["results"][k] = rk
        zkg.lib().zkg_compat_reset()
    if not cli.seam_child and hasattr(zkg, "zklaim_witness_stats") and os.environ.get("ZKG_SEAM_GPU_WITNESS", "1")[:1] != "0":
        # the other witness source: the switch is read once per process, so a child of this tool measures it after this process has gone quiet
        import subprocess
        cmd = [sys.executable, os.path.abspath(__file__), "--seam", "--seam-child", "--reps", str(cli.reps), "--ks", *map(str, cli.ks), "--ps", *map(str, cli.ps)]
        out = subprocess.run(cmd, env=dict(os.environ, ZKG_SEAM_GPU_WITNESS="0"), capture_output=True, text=True, check=True).stdout
        child = json.loads(out.strip().splitlines()[-1])["results"]
        for k in cli.ks:
            for P in cli.ps:
                here, there = res["results"][k]["P"][P], child[str(k)]["P"][str(P)]
                assert there["witness_stats"][0] == 0, "the child did not keep the host witnesses"
                here["batch_host_witness"] = there["batch"]
                print(f"seam k={k} P={P:3d}  batch, host witnesses {there['batch']}  core {here.get('core')}", flush=True)
for k in ([] if cli.seam else cli.ks):
    crs, items, keep = key_and_items(k, max(cli.ps))
    chunk = crs.prove_batch_chunk()
    expect = [crs.prove_sparse(*it) for it in items]
    assert all(e[0] == 0 for e in expect)
    bad = []

    def caller():
        for j in range(cli.caller_proofs):
            if crs.prove_sparse(*items[j % len(items)]) != expect[j % len(items)]:
                bad.append(j)

    def three_callers():
        th = [threading.Thread(target=caller) for _ in range(3)]
        for t in th:
            t.start()
        for t in th:
            t.join()

    rk = {"chunk": chunk, "three_callers": rates(three_callers, 3 * cli.caller_proofs, cli.reps), "P": {}}
    assert not bad
    print(f"k={k} (batch chunk {chunk})  three callers: {rk['three_callers']} proofs/s", flush=True)
    for P in cli.ps:
        sub = items[:P]
        assert crs.prove_batch(sub) == expect[:P]
        stats = zkg.prove_batch_stats()
        seq = rates(lambda: [crs.prove_sparse(*it) for it in sub], P, cli.reps)
        bat = rates(lambda: crs.prove_batch(sub), P, cli.reps)
        rk["P"][P] = {"sequential": seq, "batch": bat, "batch_stats": stats, "batch_min_over_sequential_max": round(bat["min"] / seq["max"], 3),
                      "batch_median_over_three_callers_median": round(bat["median"] / rk["three_callers"]["median"], 3)}
        print(f"k={k} P={P:3d}  sequential {seq}  batch {bat}  batch min / sequential max = {bat['min'] / seq['max']:.2f}", flush=True)
    res["results"][k] = rk
    crs.free()
line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
zkg.shutdown()
