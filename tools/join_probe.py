#!/usr/bin/env python3
"""Two tables set against each other on the device, beside the route through the host (one MI355X).  Records; judges nothing.

    python tools/join_probe.py --reads 10000000 > profiles/r10_join_probe.json

Two k = 21 tables from synthetic 150 bp reads of one seed (kh_synth_reads_device): a = reads [0, N), b = reads [N / 2, 3 N / 2).
Every figure is the median of 5 runs after one warm call, with the spread (max - min) of the five beside it:
  compare        kh_compare(a, b)
  union_sum      kh_combine_into(dst, a, b, UNION, SUM) into a reset context that keeps its table
  host_route     what stood in their place: kh_result_copy of both tables, a join in numpy (union of the sorted key arrays,
                 counts added), kh_merge_pairs of the result into a reset context -- and its three parts on their own
The measurement runs in a child process with a timeout; a failure is reported as {"error": ...}."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=5):
    fn()  # warm
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "spread_s": ts[-1] - ts[0]}


def measure(args):
    import numpy as np
    import torch
    from krust_amd import native
    k, rl, n = args.k, 150, args.reads

    def table(first):
        t = torch.empty(n * (rl + 1), dtype=torch.uint8, device="cuda:0")
        native.synth_reads_device(t.data_ptr(), None, 20260130, 1 << 28, rl, first, n, device=0)
        torch.cuda.synchronize()
        dc = native.DeviceCounter(k, device=0)
        dc.push_device(t.data_ptr(), None, t.numel())
        st = dc.finish()
        del t
        return dc, st

    a, sa = table(0)
    b, sb = table(n // 2)
    out = {"k": k, "reads_per_table": n, "a": {f: sa[f] for f in ("distinct", "kmers", "table_slots", "slot_bytes")},
           "b": {f: sb[f] for f in ("distinct", "kmers", "table_slots", "slot_bytes")}}
    out["words"] = a.compare(b)
    out["compare"] = timed(lambda: a.compare(b))
    with native.DeviceCounter(k, capacity_hint=sa["distinct"] + sb["distinct"], device=0) as dst:
        def union():
            dst.reset()
            return dst.combine_into(a, b, native.SET_UNION, native.CALC_SUM)
        out["union_pairs"] = union()
        out["union_sum"] = timed(union)

        parts = {}

        def host_route():
            t0 = time.perf_counter()
            ka, va = a.result(sort=False)
            kb, vb = b.result(sort=False)
            t1 = time.perf_counter()
            keys = np.concatenate((ka, kb))
            vals = np.concatenate((va, vb))
            u, inv = np.unique(keys, return_inverse=True)
            c = np.zeros(u.size, dtype=np.uint64)
            np.add.at(c, inv, vals)
            t2 = time.perf_counter()
            dst.reset()
            dst.merge_pairs(u, c)
            dst.finish()
            t3 = time.perf_counter()
            parts.setdefault("result_copy_s", []).append(t1 - t0)
            parts.setdefault("numpy_join_s", []).append(t2 - t1)
            parts.setdefault("merge_pairs_s", []).append(t3 - t2)
            return u.size

        assert host_route() == out["union_pairs"]
        parts.clear()
        out["host_route"] = timed(host_route)
        out["host_route_parts_median_s"] = {name: sorted(v[1:])[len(v[1:]) // 2] for name, v in parts.items()}
    a.close()
    b.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        measure(args)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reads", str(args.reads), "--k", str(args.k)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        res = json.loads(line[-1][7:]) if p.returncode == 0 and line else {"error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]}
    except subprocess.TimeoutExpired:
        res = {"error": f"no result within {args.timeout} s"}
    print(json.dumps({"probe": "join", "result": res}, indent=1))


if __name__ == "__main__":
    main()
