"""The stream-ordered prover (zkg_prover_prove_async) against zkg_groth16_prove_batch_dev on the same witnesses, in one process on one box.
  per key of --ks payloads (default 1, 3, 8) and per --counts proofs per call (default 1, 16):
    sync   zkg_groth16_prove_batch_dev: host clock around the synchronous call (proofs land in host memory)
    async  zkg_prover_prove_async on a stream of its own: device time from HIP events around the call, and wall time from before the call
           until the host has the proofs (a device-to-host copy queued behind the call, then a stream synchronise)
    pipe   --pipeline calls (default 8) back to back on one stream, one synchronise at the end: wall and device time per call
One warm-up of every leg, then --reps repetitions, the legs alternated (sync, async, pipe, sync, ...); medians, with min and max.  Proof bytes
are compared between the legs.  The ladder kernel's own time comes from a separate run under `rocprofv3 --kernel-trace --stats` (--trace-only:
key setup, then 11 calls of one proof); --merge RAW.json --kernel-stats DIR/x_results.db (the trace's SQLite database, its `kernels` view)
adds the k_proof_* and k_msm_combine kernels' times to a result written earlier, without a GPU.
Prints a table and one JSON line; --out writes the JSON to a file.
Usage: python tools/prove_async_time.py [--ks 1 3 8] [--counts 1 16] [--pipeline 8] [--reps 7] [--out RAW.json]
       rocprofv3 --kernel-trace --stats -d DIR -o x -- python tools/prove_async_time.py --trace-only --ks 1
       python tools/prove_async_time.py --merge RAW.json --kernel-stats DIR/x_results.db --out profiles/prove_async_time.json"""
import argparse
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
ap.add_argument("--ks", nargs="*", type=int, default=[1, 3, 8])
ap.add_argument("--counts", nargs="*", type=int, default=[1, 16])
ap.add_argument("--pipeline", type=int, default=8)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--commit", default=None)
ap.add_argument("--note", action="append", default=[])
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--merge", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--trace-only", action="store_true")
cli = ap.parse_args()


def kernel_stats(db):
    """us per launch of the epilogue kernels and the jobs' combines in a rocprofv3 kernel trace (one payload, one proof per call)"""
    import sqlite3
    con = sqlite3.connect(db)
    rows = con.execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels "
                       "where name like '%k_proof_%' or name like '%k_msm_combine%' group by name order by name").fetchall()
    short = lambda n: n.replace("void ", "").replace("zk::", "").split("(")[0]     # noqa: E731
    return [{"kernel": short(n), "launches": c, "mean_us": round(a / 1e3, 1), "min_us": round(lo / 1e3, 1), "max_us": round(hi / 1e3, 1)} for n, c, a, lo, hi in rows]


if cli.merge:
    with open(cli.merge) as f:
        merged = json.load(f)
    merged["kernel_stats_one_payload_one_proof"] = kernel_stats(cli.kernel_stats)
    merged["notes"] = merged.get("notes", []) + cli.note
    line = json.dumps(merged)
    print(line)
    if cli.out:
        with open(cli.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

zkg.init(0)


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


def stat(s):
    s = sorted(s)
    return {"min": round(s[0], 4), "median": round(s[len(s) // 2], 4), "max": round(s[-1], 4)}


def legs_for(crs, prover, ws, rss, count):
    n = ws[0].shape[0]
    d_w = torch.from_numpy(np.stack(ws[:count]).view(np.int64)).cuda()
    rs_a = np.ascontiguousarray(np.stack([np.concatenate([r, s]) for r, s in rss[:count]]), np.uint64)
    d_rs = torch.from_numpy(rs_a.view(np.int64)).cuda()
    d_pr = [torch.zeros((count * 134,), dtype=torch.uint8, device="cuda") for _ in range(cli.pipeline)]
    d_st = [torch.zeros((count,), dtype=torch.int32, device="cuda") for _ in range(cli.pipeline)]
    h_pr = torch.empty((count * 134,), dtype=torch.uint8).pin_memory()
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()

    def sync():
        t0 = time.perf_counter()
        rc, got = crs.prove_batch_dev(d_w.data_ptr(), n, count, rss[:count])
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and all(st == 0 for st, _ in got)
        return {"wall": wall}, b"".join(p for _, p in got)

    def run_async(calls):
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            e0.record()
            for c in range(calls):
                prover.prove_async(d_w.data_ptr(), n, count, d_rs.data_ptr(), d_pr[c].data_ptr(), 134, d_st[c].data_ptr(), True, stream.cuda_stream)
            e1.record()
            h_pr.copy_(d_pr[calls - 1], non_blocking=True)
        t_enq = (time.perf_counter() - t0) * 1e3
        stream.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert int(d_st[calls - 1].abs().sum()) == 0
        return {"wall": wall / calls, "device": e0.elapsed_time(e1) / calls, "enqueue": t_enq / calls}, h_pr.numpy().tobytes()
    return {"sync": sync, "async": lambda: run_async(1), "pipe": lambda: run_async(cli.pipeline)}, (d_w, d_rs, d_pr, d_st, h_pr)


def measure(legs):
    outs = {name: fn()[1] for name, fn in legs.items()}                          # warm-up (the handle's workspaces grow here)
    same = len(set(outs.values())) == 1
    samples = {name: {} for name in legs}
    for _ in range(cli.reps):
        for name, fn in legs.items():                                           # alternated
            t, out = fn()
            same = same and out == outs[name]
            for key, v in t.items():
                samples[name].setdefault(key, []).append(v)
    return {name: {key: stat(v) for key, v in s.items()} for name, s in samples.items()}, same


res = {"tool": "prove_async_time", "commit": cli.commit, "reps": cli.reps, "pipeline_calls": cli.pipeline, "device": zkg.device_info(), "notes": cli.note,
       "unit": "ms per call (pipe: per call of the pipeline); wall = host clock until the proofs are in host memory, device = HIP events around the call(s) on the caller's stream",
       "keys": {}}
for k in cli.ks:
    P = 1 if cli.trace_only else max(cli.counts)
    crs, kp, ws, keep = key_and_witnesses(k, P)
    rss = [tuple(bench.splitmix_fr(2, 9 + v)) for v in range(P)]
    prover = zkg.Prover(crs)
    entry = {"num_variables": int(ws[0].shape[0]), "domain_size": int(kp.pk.domain_size or (1 << kp.pk.log_m)), "prover_batch_max": prover.batch_max(),
             "sync_chunk": crs.prove_batch_chunk(), "counts": {}}
    for count in ([1] if cli.trace_only else cli.counts):
        legs, hold = legs_for(crs, prover, ws, rss, count)
        if cli.trace_only:
            for _ in range(11):
                legs["async"]()
            continue
        r, same = measure(legs)
        r["same_bytes"] = same
        r["prover_stats_last_call"] = zkg.prover_stats()
        r["async_wall_over_sync_wall"] = round(r["async"]["wall"]["median"] / r["sync"]["wall"]["median"], 3)
        r["pipe_wall_over_sync_wall"] = round(r["pipe"]["wall"]["median"] / r["sync"]["wall"]["median"], 3)
        entry["counts"][count] = r
        print(f"k={k:2d} count={count:2d}  sync wall {r['sync']['wall']['median']:.3f}  async wall {r['async']['wall']['median']:.3f} device {r['async']['device']['median']:.3f}"
              f"  pipe/call wall {r['pipe']['wall']['median']:.3f} device {r['pipe']['device']['median']:.3f}  same bytes {same}", flush=True)
        del legs, hold
    res["keys"][k] = entry
    prover.free(); crs.free(); kp.free()
if not cli.trace_only:
    line = json.dumps(res)
    print(line)
    if cli.out:
        with open(cli.out, "w") as f:
            f.write(line + "\n")
zkg.shutdown()
