"""The output path measured: text formatted on the device (kh_result_text_*) against the link and against the host writer.
python tools/format_probe.py [--reads 10000000] [--k 21] [--cli-runs 3] [--out FILE]   -- on the GPU box; prints ONE JSON object.

On one table (synthetic reads counted on the device):
  (a) kh_result_copy into pinned host arrays: seconds, GB/s -- the rate of the link on this box
  (b) the text stream into a pinned host buffer, fasta and tsv: seconds, text GB/s, records/s
  (c) the formatting kernels alone through kh_result_text_next_device: ms, (bytes read + written) / time
Then `kmerust <k> <FASTQ of the same reads> -q > /dev/null`, --cli-runs times each with and without KMERUST_HOST_FORMAT=1: the
result_s + write_s wall of KMERUST_TIMING.  The host-writer run is the code path of the commit before the device writer."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import krust_amd
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--k", type=int, default=21)
ap.add_argument("--cli-runs", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
stride, BATCH = 151, 10_000_000
res = {"reads": args.reads, "k": args.k, "read_len": 150}


def synth(r0, nr, qual):
    tb = torch.empty(nr * stride, dtype=torch.uint8, device=dev)
    tq = torch.empty(nr * stride, dtype=torch.uint8, device=dev) if qual else None
    krust_amd.synth_reads_device(tb.data_ptr(), tq.data_ptr() if qual else None, bench.SEED, bench.GENOME_LEN, 150, r0, nr, device=0,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tb, tq


with krust_amd.DeviceCounter(args.k, device=0) as dc:
    for r0 in range(0, args.reads, BATCH):
        tb, _ = synth(r0, min(BATCH, args.reads - r0), False)
        dc.push_device(tb.data_ptr(), None, tb.numel())
        dc.finish()
        del tb
    st = dc.finish()
    n = dc.result_size()
    res.update(kmers=st["kmers"], distinct=st["distinct"], table_slots=st["table_slots"], slot_bytes=st["slot_bytes"])
    # (a) the pairs into pinned arrays
    with krust_amd.PinnedArray(n, np.uint64) as pk, krust_amd.PinnedArray(n, np.uint64) as pc:
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            dc.result(sort=False, out=(pk.array, pc.array))
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    res["pairs_copy"] = {"s": round(best, 4), "bytes": 16 * n, "GBps": round(16 * n / best / 1e9, 2)}
    # (b) the text stream into a pinned buffer
    with krust_amd.PinnedArray(64 << 20) as pa:
        for fmt in ("fasta", "tsv"):
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                nr, nb = dc.result_text_begin(fmt)
                got = 0
                while True:
                    m = dc.result_text_next(pa.array)
                    if m == 0:
                        break
                    got += m
                dt = time.perf_counter() - t0
                assert got == nb and nr == n
                best = dt if best is None else min(best, dt)
            res[f"text_{fmt}"] = {"s": round(best, 4), "bytes": nb, "GBps": round(nb / best / 1e9, 2), "records_per_s": round(n / best)}
    # (c) the kernels alone: text left in device memory
    dbuf = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    for fmt in ("fasta", "tsv"):
        t0 = time.perf_counter()
        nr, nb = dc.result_text_begin(fmt)
        t1 = time.perf_counter()
        while dc.result_text_device(dbuf):
            pass
        t2 = time.perf_counter()
        moved = st["table_slots"] * st["slot_bytes"] + nb   # the format pass reads every slot once and writes the text
        res[f"kernels_{fmt}"] = {"size_pass_ms": round((t1 - t0) * 1e3, 2), "format_pass_ms": round((t2 - t1) * 1e3, 2),
                                 "format_pass_GBps": round(moved / (t2 - t1) / 1e9, 1)}
    del dbuf
torch.cuda.empty_cache()

# the command line on the same reads
exe = os.path.join(ROOT, "krust_amd", "host", "kmerust")
path = f"/dev/shm/kmerust_format_probe_{os.getpid()}.fq"
W = 166 + 150
try:
    with open(path, "wb") as f:
        for r0 in range(0, args.reads, BATCH):
            nr = min(BATCH, args.reads - r0)
            tb, tq = synth(r0, nr, True)
            rec = torch.empty((nr, W), dtype=torch.uint8, device=dev)
            rec[:, 0], rec[:, 1], rec[:, 11] = ord("@"), ord("r"), 10
            r = torch.arange(r0, r0 + nr, device=dev)
            for j in range(9):
                rec[:, 10 - j] = ((r // 10 ** j) % 10 + 48).to(torch.uint8)
            rec[:, 12:162] = tb.view(nr, stride)[:, :150]
            rec[:, 162], rec[:, 163], rec[:, 164] = 10, ord("+"), 10
            rec[:, 165:315] = tq.view(nr, stride)[:, :150]
            rec[:, 315] = 10
            torch.cuda.synchronize()
            rec.cpu().numpy().tofile(f)
            del rec, tb, tq, r
    torch.cuda.empty_cache()
    res["fastq_bytes"] = os.path.getsize(path)
    for name, var in (("device", {}), ("host", {"KMERUST_HOST_FORMAT": "1"})):
        runs = []
        for _ in range(args.cli_runs):
            with open(os.devnull, "wb") as null:
                p = subprocess.run([exe, str(args.k), path, "-q"], stdout=null, stderr=subprocess.PIPE, timeout=1200,
                                   env=dict(os.environ, KMERUST_TIMING="1", **var))
            assert p.returncode == 0, p.stderr[-2000:]
            t = [json.loads(l)["kmerust_timing"] for l in p.stderr.decode().splitlines() if l.startswith('{"kmerust_timing"')][-1]
            assert t["writer"] == name, t
            runs.append({"result_plus_write_s": round(t["result_s"] + t["write_s"], 3), "total_s": round(t["total_s"], 3)})
        res[f"cli_{name}_writer"] = runs
finally:
    if os.path.exists(path):
        os.remove(path)
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
