#!/usr/bin/env python3
"""The device radix sort of a table's pairs, beside the unsorted copy and the route through the host (one MI355X).  Records; judges nothing.

    python tools/sort_probe.py --reads 1000000 10000000 --out profiles/r11_sort_probe.json

Per size: one k-mer table from synthetic 150 bp reads of one seed (kh_synth_reads_device), then on that table, each figure the
median of 5 runs after one warm call with the spread (max - min) of the five beside it:
  copy_device     kh_result_copy_device    the pairs compacted into device arrays, in table order
  sorted_device   kh_result_sorted_device  the same plus the radix passes; per_pass_s = (sorted - copy) / passes, and
                  pass_traffic_gbps = 2 x 16 B x n / per_pass_s (what a pass must move: the pairs read and written once)
  text_unsorted   a whole tsv stream into a device buffer (kh_result_text_next_device), table order
  text_sorted     the same with KH_OUT_SORTED
  host_route      what stood in its place: kh_result_copy, then a sort of the pairs on 16 cores (the key range cut into 16 slices
                  by a sample of the keys, one numpy argsort per slice on a thread of its own, the slices laid end to end)
                  -- and its two parts on their own
The measurement runs in a child process with a timeout; a failure is reported as {"error": ...}."""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CORES = 16


def timed(fn, reps=5):
    fn()  # warm
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "spread_s": ts[-1] - ts[0]}


def host_sort(keys, counts):
    """Ascending by key on CORES threads (numpy releases the GIL while it sorts)."""
    import numpy as np
    if keys.size < 1 << 16:
        o = np.argsort(keys)
        return keys[o], counts[o]
    cuts = np.sort(keys[:: max(1, keys.size // 4096)])[:: max(1, 4096 // CORES)][1:CORES]
    which = np.searchsorted(cuts, keys, side="right")

    def one(i):
        sel = np.flatnonzero(which == i)
        o = sel[np.argsort(keys[sel])]
        return keys[o], counts[o]

    with ThreadPoolExecutor(CORES) as ex:
        parts = list(ex.map(one, range(cuts.size + 1)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def measure_one(k, n_reads):
    import numpy as np
    import torch
    from krust_amd import native
    rl = 150
    t = torch.empty(n_reads * (rl + 1), dtype=torch.uint8, device="cuda:0")
    native.synth_reads_device(t.data_ptr(), None, 20260130, 1 << 28, rl, 0, n_reads, device=0)
    torch.cuda.synchronize()
    dc = native.DeviceCounter(k, device=0)
    dc.push_device(t.data_ptr(), None, t.numel())
    st = dc.finish()
    del t
    n = st["distinct"]
    passes = (2 * k + 7) // 8
    out = {"k": k, "reads": n_reads, "pairs": n, "passes": passes, "table": {f: st[f] for f in ("distinct", "kmers", "table_slots", "slot_bytes")}}
    dk = torch.empty(n, dtype=torch.int64, device="cuda:0")
    dn = torch.empty(n, dtype=torch.int64, device="cuda:0")

    def copy_device():
        assert dc.result_device(dk.data_ptr(), dn.data_ptr(), n) == n
        torch.cuda.synchronize()

    def sorted_device():
        assert dc.result_sorted_device(dk.data_ptr(), dn.data_ptr(), n) == n
        torch.cuda.synchronize()

    out["copy_device"] = timed(copy_device)
    out["sorted_device"] = timed(sorted_device)
    gk = dk.cpu().numpy().view(np.uint64)
    assert (gk[1:] > gk[:-1]).all()
    per_pass = (out["sorted_device"]["median_s"] - out["copy_device"]["median_s"]) / passes
    out["per_pass_s"] = per_pass
    out["pass_traffic_bytes"] = 2 * 16 * n
    out["pass_traffic_gbps"] = 2 * 16 * n / per_pass / 1e9 if per_pass > 0 else None

    _, nbytes = dc.result_text_begin("tsv")
    buf = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda:0")

    def text(sort):
        def run():
            dc.result_text_begin("tsv", sorted=sort)
            got = 0
            while True:
                m = dc.result_text_device(buf.data_ptr() + got, cap=nbytes + 64 - got)
                if m == 0:
                    break
                got += m
            torch.cuda.synchronize()
            assert got == nbytes
        return run

    out["text_bytes"] = nbytes
    out["text_unsorted"] = timed(text(False))
    out["text_sorted"] = timed(text(True))
    del buf, dk, dn

    parts = {}

    def host_route():
        t0 = time.perf_counter()
        keys, counts = dc.result(sort=False)
        t1 = time.perf_counter()
        sk, sc = host_sort(keys, counts)
        t2 = time.perf_counter()
        parts.setdefault("result_copy_s", []).append(t1 - t0)
        parts.setdefault("host_sort_s", []).append(t2 - t1)
        return sk

    assert np.array_equal(host_route(), gk)
    parts.clear()
    out["host_route"] = timed(host_route, reps=3)
    out["host_route_parts_median_s"] = {name: sorted(v[1:])[len(v[1:]) // 2] for name, v in parts.items()}
    out["host_sort_threads"] = CORES
    dc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=None, help="the JSON file to write (default: stdout)")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        for n in args.reads:
            print("RESULT " + json.dumps(measure_one(args.k, n)), flush=True)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--k", str(args.k), "--reads"] + [str(n) for n in args.reads]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
        res = [json.loads(l[7:]) for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            res = {"error": f"exit {p.returncode}", "stderr": p.stderr[-2000:], "partial": res}
    except subprocess.TimeoutExpired:
        res = {"error": f"no result within {args.timeout} s"}
    doc = json.dumps({"probe": "sort", "result": res}, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
