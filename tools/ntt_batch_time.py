"""Device time per transform of the zkg_domain handle against the single-vector entries, and of its Lagrange kernel against the host loop,
in one process on one box.

Transforms, for m = 2^16, 2^18, 2^20 and 2^19 + 2^11 (--sizes) and count = 1, 3, 8, 16 (--counts), forward plain transforms in place:
  (a) loop    `count` calls of zkg_ntt_dev (zkg_ntt_domain_dev at a step size), one vector each, on one stream — entries this change does not
              touch, so these are the parent commit's figures
  (b) handle  ONE zkg_domain_ntt_async call over the `count` vectors on the same stream
HIP events around a window of --iters repetitions of a leg (default max(10, 400 / count)); microseconds per transform = window / (iters * count).
One warm-up of each leg, then --pairs pairs, loop and handle alternating.  The bytes the two legs leave are compared.  At count 1 the handle
adds no kernel: `count1_within_loop_spread` says whether its mean stays within the loop's mean plus the loop's own spread (max - min).

Lagrange, at m = 2^20 and 2^19 + 2^11 (--lagrange-sizes): events around --lagrange-calls zkg_domain_lagrange_async calls, microseconds per
call, in child processes, one per run length (--runs; ZKG_LAGRANGE_RUN, 0 = the library's default), each reporting a digest of the values
it computed; and the host loop's lap, read from the `[zkg setup]` lines a libsnark_trusted_setup of 37 (2^20) and 19 (2^19 + 2^11)
payloads prints under ZKG_DEBUG_TIMING=1, second setup of a child process.

Usage: python tools/ntt_batch_time.py [--out profiles/ntt_batch_time.json]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEP_19_11 = (1 << 19) + (1 << 11)
PAYLOADS = {1 << 20: 37, STEP_19_11: 19}                     # zklaim payload counts whose circuits land on these domains

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", nargs="*", type=int, default=[1 << 16, 1 << 18, 1 << 20, STEP_19_11])
ap.add_argument("--counts", nargs="*", type=int, default=[1, 3, 8, 16])
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--lagrange-sizes", nargs="*", type=int, default=[1 << 20, STEP_19_11])
ap.add_argument("--lagrange-calls", type=int, default=10)
ap.add_argument("--runs", nargs="*", type=int, default=[0, 4, 8, 16, 32, 64])
ap.add_argument("--no-host-lap", action="store_true")
ap.add_argument("--note", action="append", default=[])
ap.add_argument("--out", default=None)
ap.add_argument("--child", choices=["lagrange", "setup"], default=None)       # internal: the child processes of the Lagrange part
ap.add_argument("--payloads", type=int, default=0)
cli = ap.parse_args()

import torch  # noqa: E402
import zklaim_amd as zkg  # noqa: E402
from util import random_fr_canonical  # noqa: E402

zkg.init(0)


def events_us(stream, fn, reps):
    """microseconds per repetition of fn, HIP events around `reps` of them on `stream`"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def lagrange_child():
    """one line of JSON: {m: {"kernel_us": [...], "digest": ...}} at this process's run length"""
    stream = torch.cuda.Stream()
    out = {}
    for m in cli.lagrange_sizes:
        dom = zkg.Domain(m)
        t = random_fr_canonical(1, 0x7A6 + m)[0]              # any limbs below r are some element's Montgomery form
        d_u = torch.zeros((m, 4), dtype=torch.int64, device="cuda")
        d_z = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
        call = lambda: dom.lagrange_async(t, d_u.data_ptr(), d_z.data_ptr(), stream=stream.cuda_stream)  # noqa: E731
        call(); stream.synchronize()
        us = [round(events_us(stream, call, cli.lagrange_calls), 2) for _ in range(cli.pairs)]
        digest = hashlib.sha256(d_u.cpu().numpy().tobytes() + d_z.cpu().numpy().tobytes()).hexdigest()[:16]
        out[str(m)] = {"kernel_us": us, "digest": digest}
        dom.free()
    print("LAGRANGE " + json.dumps(out), flush=True)


def setup_child():
    """two trusted setups of cli.payloads payloads; the library prints its laps to stderr, the domain size goes to stdout"""
    from gpu_util import credential_payloads
    keep = []
    ctx = zkg.make_ctx(credential_payloads(cli.payloads), keep)
    ck = zkg.ZklaimCircuit(ctx, with_witness=False)
    print("DOMAIN %d" % zkg.evaluation_domain_size(ck.r1cs.num_constraints + ck.r1cs.num_inputs + 1)[0], flush=True)
    for _ in range(2):
        assert zkg.libsnark_trusted_setup(ctx) == 0


if cli.child == "lagrange":
    lagrange_child(); zkg.shutdown(); sys.exit(0)
if cli.child == "setup":
    setup_child(); zkg.shutdown(); sys.exit(0)


def spawn(args, env_extra):
    env = dict(os.environ); env.update(env_extra)
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=900)


res = {"tool": "ntt_batch_time", "device": zkg.device_info(), "pairs": cli.pairs, "notes": cli.note,
       "unit": "microseconds of device time per transform (HIP events around a window of iters x count transforms on one stream)",
       "transforms": {}, "count1_within_loop_spread": {}, "lagrange": {}}
stream = torch.cuda.Stream()
sp = stream.cuda_stream
for m in cli.sizes:
    step = m & (m - 1) != 0
    logm = m.bit_length() - 1
    cmax = max(cli.counts)
    src = torch.from_numpy(random_fr_canonical(m * cmax, 0x17B + m).reshape(cmax, m, 4).view(np.int64)).cuda()
    a = src.clone(); b = src.clone()
    dom = zkg.Domain(m)
    L = zkg.lib()
    size = {"batch_max": dom.batch_max(), "counts": {}}
    for count in cli.counts:
        iters = cli.iters or max(10, 400 // count)

        def loop_leg(buf=a):
            for i in range(count):
                if step:
                    zkg.api._check(L.zkg_ntt_domain_dev(zkg.api._vp(buf[i].data_ptr()), zkg.api.C.c_size_t(m), 0, 0, zkg.api._vp(sp)), "zkg_ntt_domain_dev")
                else:
                    zkg.ntt_dev(buf[i].data_ptr(), logm, stream=sp)

        def handle_leg(buf=b):
            dom.ntt_async(buf.data_ptr(), count=count, stream=sp)

        a.copy_(src); b.copy_(src); torch.cuda.synchronize()
        loop_leg(); handle_leg(); stream.synchronize()                 # warm-up of both legs, and the bytes they leave
        same = bool(torch.equal(a[:count], b[:count]))
        stats = zkg.domain_stats()
        t = {"loop": [], "handle": []}
        for _ in range(cli.pairs):
            for name, fn in (("loop", loop_leg), ("handle", handle_leg)):
                t[name].append(round(events_us(stream, fn, iters) / count, 3))
        lm, hm = sum(t["loop"]) / cli.pairs, sum(t["handle"]) / cli.pairs
        r = {"iters": iters, "loop_us": t["loop"], "handle_us": t["handle"], "loop_mean": round(lm, 3), "handle_mean": round(hm, 3),
             "loop_spread": round(max(t["loop"]) - min(t["loop"]), 3), "handle_minus_loop": round(hm - lm, 3), "same_bytes": same,
             "groups_and_waits_of_the_warm_up": stats[1:]}
        size["counts"][str(count)] = r
        if count == 1:
            res["count1_within_loop_spread"][str(m)] = bool(hm - lm <= r["loop_spread"])
        print(f"m={m} count={count:2d} loop {r['loop_mean']:8.2f} us (spread {r['loop_spread']:.2f})  handle {r['handle_mean']:8.2f} us  same bytes {same}", flush=True)
    res["transforms"][str(m)] = size
    dom.free()
    del a, b, src
torch.cuda.synchronize()

by_run = {}
for run in cli.runs:
    p = spawn(["--child", "lagrange", "--pairs", str(cli.pairs), "--lagrange-calls", str(cli.lagrange_calls), "--lagrange-sizes"] + [str(m) for m in cli.lagrange_sizes],
              {"ZKG_LAGRANGE_RUN": str(run)} if run else {"ZKG_LAGRANGE_RUN": ""})
    line = [x for x in p.stdout.splitlines() if x.startswith("LAGRANGE ")]
    if p.returncode != 0 or not line:
        print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
        raise SystemExit(f"lagrange child (run {run}) failed with {p.returncode}")
    by_run[run] = json.loads(line[0][len("LAGRANGE "):])
    print(f"lagrange run {run}: {by_run[run]}", flush=True)
for m in cli.lagrange_sizes:
    first = by_run[cli.runs[0]][str(m)]["digest"]
    entry = {"unit": "microseconds per zkg_domain_lagrange_async call (events around %d calls), run 0 = the library's default run length" % cli.lagrange_calls,
             "by_run_length": {str(run): by_run[run][str(m)]["kernel_us"] for run in cli.runs},
             "same_values_at_every_run_length": all(by_run[run][str(m)]["digest"] == first for run in cli.runs)}
    if not cli.no_host_lap and m in PAYLOADS:
        p = spawn(["--child", "setup", "--payloads", str(PAYLOADS[m])], {"ZKG_DEBUG_TIMING": "1"})
        dm = re.findall(r"^DOMAIN (\d+)", p.stdout, re.M)
        laps = re.findall(r"\[zkg setup\] (copy \+ swap|lagrange)\s+([0-9.]+) ms", p.stderr)
        if p.returncode != 0 or not dm or int(dm[0]) != m or len(laps) < 4:
            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
            raise SystemExit(f"setup child ({PAYLOADS[m]} payloads) failed with {p.returncode}")
        before, after = [float(v) for k, v in laps if k.startswith("copy")], [float(v) for k, v in laps if k == "lagrange"]
        entry["host_loop_ms"] = [round(y - x, 3) for x, y in zip(before, after)]
        entry["host_loop_from"] = "the lagrange lap of libsnark_trusted_setup, %d payloads, first and second setup of one process" % PAYLOADS[m]
    res["lagrange"][str(m)] = entry
    print(f"lagrange m={m}: {entry}", flush=True)

line = json.dumps(res, indent=1)
print(json.dumps(res))
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
zkg.shutdown()
