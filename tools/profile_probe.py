#!/usr/bin/env python3
"""Rates of kh_profile / kh_profile_device beside the existing paths they are judged against (one MI355X).

    python tools/profile_probe.py --reads 10000000 > profiles/r08_profile_probe.json

Every leg is a child process of its own with a timeout; a leg that fails is reported as {"error": ...} and nothing more is started on
the device after it.
For k = 21 and for k = 31 with -Q 20, on synthetic 150 bp reads (kh_synth_reads_device):
  a  kh_profile_device against the table of the same reads                 ms, G windows/s (entries written per second)
  b  the same against a table of other reads (most windows absent)
  c  kh_profile from pageable and from pinned host memory                  s, GB/s of bases in, GB/s of profile out
  d  what they are judged against, from the EXISTING paths: the direct counting kernel over the same buffer into a table of the
     same size (KMERHIP_PATH=direct, kh_stats.stage_ms[direct]), and kh_lookup fed the canonical keys of the windows of the
     first --lookup-reads reads from host memory (s, M keys/s)
and the two ratios: a / direct count (expected <= 1.05), and kh_lookup's time over kh_profile's on the same reads (leg d_lookup
times both from pageable memory; expected > 1).
The per-record reduction (kh_profile_records*), k = 21 only, every figure the median of 5 runs after the context's first call,
with the spread (max - min) of the runs beside it:
  r_host  the summary's route before kh_profile_records -- kh_profile into host memory plus the six numbers per record folded on
          one host thread (numpy here: segment sums over the profile) -- against kh_profile_records from pageable and from pinned
          memory, on the same reads
  r_dev   the kernels alone: kh_profile_device against kh_profile_records_device"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(native, torch, seed, n_reads, rl=150):
    n = n_reads * (rl + 1)
    tb = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    tq = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    native.synth_reads_device(tb.data_ptr(), tq.data_ptr(), seed, 1 << 28, rl, 0, n_reads, device=0)
    torch.cuda.synchronize()
    return tb, tq


def canonical_keys(np, flat, k):
    """Canonical keys of the valid windows of a flat buffer (host; no qualities)."""
    code = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = code[ch + 32] = i
    c = code[flat]
    bad = np.concatenate(([0], np.cumsum(c == 255, dtype=np.int64)))
    nw = flat.size - k + 1
    good = (bad[k:] - bad[:-k]) == 0
    c64 = (c & 3).astype(np.uint64)
    fwd = np.zeros(nw, dtype=np.uint64)
    rc = np.zeros(nw, dtype=np.uint64)
    for j in range(k):
        fwd |= c64[j:j + nw] << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - c64[j:j + nw]) << np.uint64(2 * j)
    return np.minimum(fwd, rc)[good]


def leg(args):
    import numpy as np
    import torch
    from krust_amd import native
    k, minq, reps = args.k, (args.minq if args.minq >= 0 else None), 3
    tb, tq = synth(native, torch, 20260130, args.reads)
    n = tb.numel()
    q = tq.data_ptr() if minq is not None else None
    out = {"leg": args.leg, "k": k, "min_quality": minq, "reads": args.reads, "bytes": n}

    def timed(f):
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best

    if args.leg in ("a", "b", "c"):
        src_b, src_q = (tb, tq) if args.leg != "b" else synth(native, torch, 777, args.reads)
        with native.DeviceCounter(k, min_quality=minq) as dc:
            dc.push_device(src_b.data_ptr(), src_q.data_ptr() if minq is not None else None, n)
            st = dc.finish()
            out.update(table_slots=st["table_slots"], slot_bytes=st["slot_bytes"], distinct=st["distinct"])
            if args.leg in ("a", "b"):
                to = torch.empty(n, dtype=torch.int32, device="cuda:0")
                dc.profile_device(tb.data_ptr(), q, n, to.data_ptr())      # warm-up
                s = timed(lambda: dc.profile_device(tb.data_ptr(), q, n, to.data_ptr()))
                res = to.view(torch.int32)
                valid = int((res != -1).sum().item())
                present = int(((res != -1) & (res != 0)).sum().item())
                out.update(ms=s * 1e3, g_entries_per_s=n / s / 1e9, valid_windows=valid, present_windows=present,
                           g_valid_windows_per_s=valid / s / 1e9)
            else:
                hb, hq = tb.cpu().numpy(), tq.cpu().numpy()
                res = {}
                ho = np.empty(n, dtype=np.uint32)
                dc.profile(hb[: 1 << 20], hq[: 1 << 20] if minq is not None else None)   # buffers
                s = timed(lambda: dc.profile(hb, hq if minq is not None else None, out=ho))
                res["pageable"] = {"s": s, "gb_per_s_in": n * (2 if minq is not None else 1) / s / 1e9, "gb_per_s_out": 4 * n / s / 1e9, "m_entries_per_s": n / s / 1e6}
                with native.PinnedArray(n) as pb, native.PinnedArray(n) as pq, native.PinnedArray(n, dtype=np.uint32) as po:
                    pb.array[:] = hb
                    pq.array[:] = hq
                    s = timed(lambda: dc.profile(pb.array, pq.array if minq is not None else None, out=po.array))
                    res["pinned"] = {"s": s, "gb_per_s_in": n * (2 if minq is not None else 1) / s / 1e9, "gb_per_s_out": 4 * n / s / 1e9, "m_entries_per_s": n / s / 1e6}
                    assert np.array_equal(po.array, ho)
                out.update(res)
    elif args.leg in ("r_host", "r_dev"):
        def med5(f):
            f()                                     # the context's first call of this kind: buffers
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t0)
            ts.sort()
            return {"median_s": ts[2], "spread_s": ts[-1] - ts[0]}
        nrec = args.reads
        rs = np.arange(nrec + 1, dtype=np.uint64) * np.uint64(151)
        with native.DeviceCounter(k, min_quality=minq) as dc:
            dc.push_device(tb.data_ptr(), q, n)
            dc.finish()
            if args.leg == "r_dev":
                to = torch.empty(n, dtype=torch.int32, device="cuda:0")
                trs = torch.from_numpy(rs.view(np.int64)).to("cuda:0")
                trows = torch.empty(nrec * 8, dtype=torch.int32, device="cuda:0")
                out["profile_device"] = med5(lambda: dc.profile_device(tb.data_ptr(), q, n, to.data_ptr()))
                out["profile_records_device"] = med5(lambda: dc.profile_records_device(tb.data_ptr(), q, n, trs, nrec, trows))
                rows = trows.cpu().numpy().view(np.uint32).reshape(nrec, 8)
                res = to.cpu().numpy().view(np.uint32)
                win = res != 0xFFFFFFFF
                assert int(rows[:, 0].sum()) == int(win.sum()) and int(rows[:, 1].sum()) == int((win & (res > 0)).sum())
            else:
                hb = tb.cpu().numpy()
                hq = tq.cpu().numpy() if minq is not None else None
                ho = np.empty(n, dtype=np.uint32)
                hrows = np.empty((nrec, 8), dtype=np.uint32)

                def host_summary():   # (a stand-in for the CLI's write_profile_lines: vectorised, and no formatting)
                    dc.profile(hb, hq, out=ho)
                    P = ho.reshape(nrec, 151)
                    w = P != 0xFFFFFFFF
                    v = np.where(w, P, 0)
                    return w.sum(axis=1), (v > 0).sum(axis=1), np.where(w, P, 0xFFFFFFFF).min(axis=1), v.max(axis=1), v.sum(axis=1, dtype=np.uint64)
                out["profile_plus_host_summary"] = med5(host_summary)
                out["profile_alone"] = med5(lambda: dc.profile(hb, hq, out=ho))
                out["profile_records_pageable"] = med5(lambda: dc.profile_records(hb, rs, hq, out=hrows))
                ref = host_summary()
                assert np.array_equal(hrows[:, 0], ref[0]) and np.array_equal(hrows[:, 1], ref[1]) and np.array_equal(hrows[:, 4], ref[3])
                with native.PinnedArray(n) as pb, native.PinnedArray(n) as pq, native.PinnedArray(nrec * 8, dtype=np.uint32) as po:
                    pb.array[:] = hb
                    if hq is not None:
                        pq.array[:] = hq
                    out["profile_records_pinned"] = med5(lambda: dc.profile_records(pb.array, rs, pq.array if hq is not None else None, out=po.array))
                    assert np.array_equal(po.array.reshape(nrec, 8), hrows)
                out["bytes_back_per_record"] = {"profile": 604, "profile_records": 32}
    elif args.leg == "d_count":
        # the direct counting kernel over the same buffer into a table of the size leg a's table has
        with native.DeviceCounter(k, min_quality=minq) as dc:
            dc.push_device(tb.data_ptr(), q, n)
            st = dc.finish()
            distinct = st["distinct"]
        with native.DeviceCounter(k, min_quality=minq, capacity_hint=distinct, path="direct") as dc:
            best = None
            for _ in range(reps):
                dc.reset()
                dc.push_device(tb.data_ptr(), q, n)
                st = dc.finish()
                ms = st["stage_ms"]["direct"]
                best = ms if best is None else min(best, ms)
            out.update(direct_ms=best, table_slots=st["table_slots"], kmers=st["kmers"], g_kmers_per_s=st["kmers"] / best / 1e6)
    elif args.leg == "d_lookup":
        m = args.lookup_reads * 151
        hb = tb[:m].cpu().numpy()
        keys = canonical_keys(np, hb, k)
        with native.DeviceCounter(k) as dc:
            dc.push_device(tb.data_ptr(), None, n)
            dc.finish()
            dc.lookup(keys[:1000])
            s = timed(lambda: dc.lookup(keys))
            out.update(keys=int(keys.size), s=s, m_keys_per_s=keys.size / s / 1e6, bytes_per_key_over_the_link=16)
            ho = np.empty(m, dtype=np.uint32)
            s2 = timed(lambda: dc.profile(hb, out=ho))
            out.update(profile_same_windows_s=s2, profile_m_entries_per_s=m / s2 / 1e6)
    print("LEG " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--lookup-reads", type=int, default=250_000)
    ap.add_argument("--leg")
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--minq", type=int, default=-1)
    ap.add_argument("--timeout", type=int, help="seconds per leg (default 240; 900 with --records-only: r_host makes some 30 calls over all reads)")
    ap.add_argument("--records-only", action="store_true", help="only the legs of the per-record reduction (r_host, r_dev), k = 21")
    args = ap.parse_args()
    if args.timeout is None:
        args.timeout = 900 if args.records_only else 240
    if args.leg:
        return leg(args)
    if args.records_only:
        report = {"tool": "tools/profile_probe.py --records-only", "reads": args.reads, "read_len": 150, "k": 21}
        for name in ("r_dev", "r_host"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--k", "21", "--minq", "-1", "--reads", str(args.reads)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
                lines = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
                report[name] = json.loads(lines[-1][4:]) if p.returncode == 0 and lines else {"error": f"exit {p.returncode}", "stderr": p.stderr[-600:]}
            except subprocess.TimeoutExpired:
                report[name] = {"error": f"timeout after {args.timeout} s"}
            if "error" in report[name]:
                report["stopped"] = f"leg {name} failed: nothing more is started on the device"
                print(json.dumps(report, indent=1))
                return 1
        print(json.dumps(report, indent=1))
        return 0
    report = {"tool": "tools/profile_probe.py", "reads": args.reads, "read_len": 150, "configs": []}
    for k, minq in ((21, -1), (31, 20)):
        cfg = {"k": k, "min_quality": None if minq < 0 else minq}
        for name in ("a", "b", "c", "d_count", "d_lookup"):
            if name == "d_lookup" and minq >= 0:
                continue   # (kh_lookup takes keys: the quality rule would be the caller's)
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--k", str(k), "--minq", str(minq), "--reads", str(args.reads),
                   "--lookup-reads", str(args.lookup_reads)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
                lines = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
                cfg[name] = json.loads(lines[-1][4:]) if p.returncode == 0 and lines else {"error": f"exit {p.returncode}", "stderr": p.stderr[-600:]}
            except subprocess.TimeoutExpired:
                cfg[name] = {"error": f"timeout after {args.timeout} s"}
            if "error" in cfg[name]:   # (whatever ended a leg -- a HIP error, a fault, a time limit -- may have left the device unwell)
                cfg["stopped"] = f"leg {name} failed: nothing more is started on the device"
                report["configs"].append(cfg)
                print(json.dumps(report, indent=1))
                return 1
        a, d = cfg.get("a", {}), cfg.get("d_count", {})
        if "ms" in a and "direct_ms" in d:
            cfg["ratio_profile_device_over_direct_count"] = a["ms"] / d["direct_ms"]
        lk = cfg.get("d_lookup", {})
        if "m_keys_per_s" in lk and "profile_same_windows_s" in lk:   # both timed on the same reads, in the same leg
            cfg["ratio_profile_over_lookup_same_windows"] = lk["s"] / lk["profile_same_windows_s"]
        report["configs"].append(cfg)
    print(json.dumps(report, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
