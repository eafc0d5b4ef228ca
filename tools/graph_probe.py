#!/usr/bin/env python3
"""The de Bruijn graph degrees of a count table on the device, beside the routes to set them against (one MI355X).  Records; judges
nothing.

    python tools/graph_probe.py --reads 1000000 10000000 > profiles/r12_graph_probe.json

Per size: a k = 21 table from synthetic 150 bp reads of one seed (kh_synth_reads_device).  Every figure is the median of 5 runs
after one warm call, with the spread (max - min) of the five beside it:
  graph_stats        kh_graph_stats(1): a scan of the table's slots, eight probes per node
  graph_masks_device kh_graph_masks_device over the keys kh_result_sorted_device produced (device arrays, nothing crosses the link)
  both also as nodes / s and as probed lines / s (8 per node)
  self_compare       kh_compare(a, a): ONE probe per live slot with the same probe code -- eight times its time is the yardstick
                     for "the eight loads overlap"
  host_route         the route the two calls replace: kh_result_copy, the 8 x n neighbour keys rolled in numpy, eight kh_lookup
                     calls (16 bytes per probe over the link), the masks assembled on the host -- and its parts on their own
                     (above 20 M nodes: ONE run, not a median)
The measurement runs in a child process with a timeout; a failure is reported as {"error": ...}."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=5, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "spread_s": ts[-1] - ts[0]}


def np_neighbours(x, k):
    import numpy as np
    U = np.uint64
    m, top = U((1 << (2 * k)) - 1 if k < 32 else (1 << 64) - 1), U(2 * (k - 1))
    r = np.zeros_like(x)
    for i in range(k):
        r = (r << U(2)) | (U(3) - ((x >> U(2 * i)) & U(3)))
    out = []
    for c in range(4):
        out.append(np.minimum(((x << U(2)) | U(c)) & m, (r >> U(2)) | (U(3 - c) << top)))
    for c in range(4):
        out.append(np.minimum((x >> U(2)) | (U(c) << top), ((r << U(2)) | U(3 - c)) & m))
    return out


def measure_one(n, k, host_max):
    import numpy as np
    import torch
    from krust_amd import native
    rl = 150
    t = torch.empty(n * (rl + 1), dtype=torch.uint8, device="cuda:0")
    native.synth_reads_device(t.data_ptr(), None, 20260130, 1 << 28, rl, 0, n, device=0)
    torch.cuda.synchronize()
    a = native.DeviceCounter(k, device=0)
    a.push_device(t.data_ptr(), None, t.numel())
    st = a.finish()
    del t
    out = {"k": k, "reads": n, "table": {f: st[f] for f in ("distinct", "kmers", "table_slots", "slot_bytes")}}
    words = a.graph_stats(1)
    nodes = int(words[native.GRAPH_NODES])
    out["nodes"] = nodes
    out["arcs"] = sum(int(words[m]) * bin(m).count("1") for m in range(256))
    rate = lambda r: dict(r, nodes_per_s=nodes / r["median_s"], lines_per_s=8 * nodes / r["median_s"])
    out["graph_stats"] = rate(timed(lambda: a.graph_stats(1)))
    dk = torch.empty(nodes, dtype=torch.int64, device="cuda:0")
    dc = torch.empty(nodes, dtype=torch.int64, device="cuda:0")
    dm = torch.empty(nodes, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert a.result_sorted_device(dk.data_ptr(), dc.data_ptr(), nodes, 1) == nodes
    out["graph_masks_device"] = rate(timed(lambda: a.graph_masks_device(dk, nodes, dm, 1)))
    dev_masks = dm.cpu().numpy()
    assert np.array_equal(np.bincount(dev_masks, minlength=256).astype(np.uint64), words[:256])
    out["self_compare"] = timed(lambda: a.compare(a))
    out["stats_over_8_self_compares"] = out["graph_stats"]["median_s"] / (8 * out["self_compare"]["median_s"])

    parts = {}
    got = {}

    def host_route():
        t0 = time.perf_counter()
        keys, _ = a.result(sort=False)
        t1 = time.perf_counter()
        nb = np_neighbours(keys, k)
        t2 = time.perf_counter()
        masks = np.zeros(keys.size, dtype=np.uint8)
        for j in range(8):
            masks |= ((a.lookup(nb[j]) > 0).astype(np.uint8) << np.uint8(j))
        t3 = time.perf_counter()
        parts.setdefault("result_copy_s", []).append(t1 - t0)
        parts.setdefault("numpy_neighbours_s", []).append(t2 - t1)
        parts.setdefault("eight_lookups_s", []).append(t3 - t2)
        got["hist"] = np.bincount(masks, minlength=256).astype(np.uint64)

    if nodes > host_max:
        out["host_route"] = {"skipped": f"more than --host-route-max-nodes {host_max} nodes"}
        a.close()
        return out
    # (tens of millions of nodes: 64 bytes of neighbour keys per node on the host and 16 bytes per probe over the link -- one run)
    big = nodes > 20_000_000
    out["host_route"] = dict(rate(timed(host_route, reps=1 if big else 5, warm=not big)), runs=1 if big else 5)
    assert np.array_equal(got["hist"], words[:256])
    out["host_route_parts_median_s"] = {name: sorted(v[0 if big else 1:])[len(v[0 if big else 1:]) // 2] for name, v in parts.items()}
    a.close()
    return out


def measure(args):
    print("RESULT " + json.dumps([measure_one(n, args.k, args.host_route_max_nodes) for n in args.reads]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--host-route-max-nodes", type=int, default=1 << 62, help="skip the host route on tables with more nodes (it takes minutes and 64 B of host memory per node)")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        measure(args)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--k", str(args.k), "--host-route-max-nodes", str(args.host_route_max_nodes), "--reads"] + [str(n) for n in args.reads]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        res = json.loads(line[-1][7:]) if p.returncode == 0 and line else {"error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]}
    except subprocess.TimeoutExpired:
        res = {"error": f"no result within {args.timeout} s"}
    print(json.dumps({"probe": "graph", "result": res}, indent=1))


if __name__ == "__main__":
    main()
