#!/usr/bin/env python3
"""The unitigs of a count table on the device, beside the steps to set them against (one MI355X).  Records; judges nothing.

    python tools/unitig_probe.py --reads 1000000 10000000 > profiles/r13_unitig_probe.json

Per size: a k = 21 table from synthetic 150 bp reads of one seed (kh_synth_reads_device).  Every figure is the median of 5 runs
after one warm call, with the spread (max - min) of the five beside it:
  unitigs_begin        kh_unitigs_begin(1): sort, ids, links, chain ranking, emit -- also as nodes / s
  unitigs_begin_linked kh_unitigs_begin_linked(1): the same plus the links between the unitigs (end degrees, scan, link words);
                       links_share = the part of its median that is not unitigs_begin's; n_links beside it
  unitigs_links_copy   kh_unitigs_links_copy into a host array (8 bytes per link over the link)
  unitigs_copy_device  kh_unitigs_copy_device into device arrays (nothing crosses the link)
  unitigs_copy         kh_unitigs_copy into host arrays (32 bytes per unitig and one per base over the link)
  result_sorted_device the sort alone, begin's first step
  graph_stats          kh_graph_stats(1): eight probes per node, as begin's index pass makes
With --clip, per size and in one process, only these two, on the same table:
  unitigs_begin_linked kh_unitigs_begin_linked(1), as above
  clip_tips_into       kh_clip_tips_into(1, max_kmers = k) into a fresh context hinted with the node count, kh_reset (not timed)
                       before every call; clip_share = the part of its median that is not unitigs_begin_linked's; the eight words beside it
With --pop, per size and in one process, these three, on the same table:
  unitigs_begin_linked kh_unitigs_begin_linked(1), as above
  clip_tips_into       kh_clip_tips_into(1, max_kmers = k), as with --clip
  pop_bubbles_into     kh_pop_bubbles_into(1, max_kmers = 2 k) into the same fresh context, kh_reset (not timed) before every call;
                       pop_share = the part of its median that is not unitigs_begin_linked's; the nine words beside it
With --text, in ONE PROCESS PER SIZE, the GFA text of the unitigs formatted on the device (kh_unitigs_text_*), on the same table:
  unitigs_begin_linked kh_unitigs_begin_linked(1), as above
  text_begin           kh_unitigs_text_begin(gfa): a length per record and per link line, two scans; n_bytes beside it
  text_drain_device    every kh_unitigs_text_next_device into one 64 MiB device buffer, then a device synchronise -- also as bytes / s;
                       text_share = (text_begin + text_drain_device) / unitigs_begin_linked
  text_drain_pinned    every kh_unitigs_text_next into three pinned 64 MiB buffers in turn -- also as bytes / s
  copies_pinned        the yardstick for the link: kh_unitigs_copy + kh_unitigs_links_copy of the same unitigs into pinned arrays, as
                       bytes / s of what they move (32 B per unitig, 1 per base, 8 per link)
With --locate, in ONE PROCESS PER SIZE, the reads located on the unitigs of their own table (kh_unitigs_locate*):
  unitigs_begin          kh_unitigs_begin(1), as above
  locate_first           a begin (not timed), then the first kh_unitigs_locate_device of 1 M reads: it builds the place map
  index_build            locate_first minus locate_device; index_share = that over unitigs_begin
  locate_device          kh_unitigs_locate_device of 1 M resident reads (151 M window starts) -- also as window starts / s and
                         bytes / s of output; profile_device = kh_profile_device on the same reads, the two alternating
  locate_pinned          kh_unitigs_locate from and into pinned memory; profile_pinned = kh_profile likewise, alternating
With --paths, in ONE PROCESS PER SIZE, the same resident reads as run-compressed paths (kh_unitigs_paths*), one record per read:
  runs, runs_per_read    the runs of the 1 M reads; bytes_out = 16 per run + 8 per read, against locate's 8 per window start
  paths_device           kh_unitigs_paths_device with room for every run and a coverage array; locate_device = kh_unitigs_locate_device
                         on the same reads, the two alternating; paths_over_locate = the ratio of the medians
  paths_pinned           kh_unitigs_paths from pinned memory into pinned arrays; locate_pinned = kh_unitigs_locate likewise, alternating
  split_ms               the device form's time on the device per step -- locate_range, path_flags_kernel, the scan, path_emit_kernel,
                         path_cover_kernel -- from HIP events round every launch (a second context with KH_FLAG_TRACE, one call)
With --support, in ONE PROCESS PER SIZE, the read support per link (kh_unitigs_link_support*) on the rows the paths call left on the device:
  paths_device           kh_unitigs_paths_device alone (no coverage array); paths_then_support = the same followed by
                         kh_unitigs_link_support_device on its rows, the two alternating; support_over_paths = the difference of the medians
                         over paths_device
  crossings, links, links_without_support   ADJACENT of the call, n_links, and the share of links with support 0
  split_ms               the traced split of one support call (the index build, link_support_kernel) and of the paths call before it
                         (path_cover_kernel is the yardstick: one lane per row, atomics per row) -- a second context with KH_FLAG_TRACE
  host_route             what the call replaces: the rows copied back, then np.searchsorted of the crossing words in the link array
With --components, in ONE PROCESS PER SIZE, the connected components of the unitig graph (kh_unitigs_components*) and the drop rule:
  unitigs_begin_linked   kh_unitigs_begin_linked(1), as above; components_first = the first kh_unitigs_components_device behind it (it
                         builds the labels), components_cached = the second (copies only) -- six begins, the first not counted;
                         first_over_begin = the ratio of the medians
  stats                  components, singletons, largest_kmers, rounds of the call
  split_ms               the traced split of one first call -- the rounds (hook, compress and the flag read-back per round), the sums,
                         ids and rows -- a second context with KH_FLAG_TRACE
  drop_components_into   kh_drop_components_into(1, min_kmers = 2 k) into a fresh context hinted with the node count; clip_tips_into =
                         kh_clip_tips_into(1, k) into the same, the two alternating, kh_reset (not timed) before every call
  host_route             what the call replaces: kh_unitigs_links_copy, then connected components on the host -- scipy.sparse.csgraph
                         where scipy is importable, else a numpy hook-and-compress; host_route_by names which; its labels must agree
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


def measure_one(n, k):
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
    nu, nb = a.unitigs_begin(1)
    out.update(nodes=nodes, unitigs=nu, bases=nb)
    rate = lambda r: dict(r, nodes_per_s=nodes / r["median_s"])
    out["unitigs_begin"] = rate(timed(lambda: a.unitigs_begin(1)))
    linked = timed(lambda: a.unitigs_begin_linked(1))
    nu2, nb2, nl = a.unitigs_begin_linked(1)
    assert (nu2, nb2) == (nu, nb)
    out["unitigs_begin_linked"] = dict(rate(linked), links_share=max(linked["median_s"] - out["unitigs_begin"]["median_s"], 0.0) / linked["median_s"])
    out["n_links"] = nl
    got_links = {}

    def copy_links():
        got_links["links"] = a.unitigs_links_copy(nl)

    out["unitigs_links_copy"] = timed(copy_links)
    links = got_links["links"]
    assert links.size == nl and (links[1:] > links[:-1]).all()
    d_rows = torch.empty(max(4 * nu, 1), dtype=torch.int64, device="cuda:0")
    d_bases = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    out["unitigs_copy_device"] = timed(lambda: a.unitigs_copy_device(d_rows, nu, d_bases, nb))
    got = {}

    def copy():
        got["rows"], got["bases"] = a.unitigs_copy(nu, nb)

    out["unitigs_copy"] = timed(copy)
    rows = got["rows"]
    assert int(np.sum(rows[:, native.UNI_KMERS], dtype=np.uint64)) == nodes
    assert int(np.sum(rows[:, native.UNI_COUNT_SUM], dtype=np.uint64)) == int(words[native.GRAPH_KMERS])
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64)[:4 * nu].reshape(nu, 4), rows)
    lens = rows[:, native.UNI_KMERS] + np.uint64(k - 1)
    out["circular"] = int(np.sum(rows[:, native.UNI_FLAGS] & np.uint64(1)))
    out["longest_bases"] = int(lens.max()) if nu else 0
    a.unitigs_end()
    dk = torch.empty(nodes, dtype=torch.int64, device="cuda:0")
    dc = torch.empty(nodes, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    out["result_sorted_device"] = rate(timed(lambda: a.result_sorted_device(dk.data_ptr(), dc.data_ptr(), nodes, 1)))
    out["graph_stats"] = rate(timed(lambda: a.graph_stats(1)))
    a.close()
    return out


def measure_clip_one(n, k, pop=False):
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
    nodes = st["distinct"]
    rate = lambda r: dict(r, nodes_per_s=nodes / r["median_s"])
    linked = timed(lambda: a.unitigs_begin_linked(1))
    a.unitigs_end()
    out["unitigs_begin_linked"] = rate(linked)
    b = native.DeviceCounter(k, device=0, capacity_hint=nodes)
    got = {}
    ts = []
    for rep in range(6):                      # one warm call, then five
        b.reset()
        t0 = time.perf_counter()
        got["words"] = b.clip_tips_into(a, 1, k)
        ts.append(time.perf_counter() - t0)
    ts = sorted(ts[1:])
    clip = {"median_s": ts[len(ts) // 2], "spread_s": ts[-1] - ts[0]}
    out["clip_tips_into"] = dict(rate(clip), clip_share=max(clip["median_s"] - linked["median_s"], 0.0) / clip["median_s"])
    out["words"] = got["words"]
    sb = b.finish()
    assert sb["distinct"] == got["words"]["kept_kmers"] and sb["kmers"] == got["words"]["kept_count"]
    assert got["words"]["kept_kmers"] + got["words"]["clipped_kmers"] == nodes and a.finish()["distinct"] == nodes
    out["dst_grows"] = sb["grows"]
    if pop:
        ts = []
        for rep in range(6):                  # one warm call, then five
            b.reset()
            t0 = time.perf_counter()
            got["pop"] = b.pop_bubbles_into(a, 1, 2 * k)
            ts.append(time.perf_counter() - t0)
        ts = sorted(ts[1:])
        popt = {"median_s": ts[len(ts) // 2], "spread_s": ts[-1] - ts[0]}
        out["pop_bubbles_into"] = dict(rate(popt), pop_share=max(popt["median_s"] - linked["median_s"], 0.0) / popt["median_s"])
        out["pop_words"] = got["pop"]
        sb = b.finish()
        assert sb["distinct"] == got["pop"]["kept_kmers"] and sb["kmers"] == got["pop"]["kept_count"]
        assert got["pop"]["kept_kmers"] + got["pop"]["popped_kmers"] == nodes and a.finish()["distinct"] == nodes
        assert got["pop"]["unitigs"] == got["words"]["unitigs"] and got["pop"]["links"] == got["words"]["links"]
        out["pop_dst_grows"] = sb["grows"]
    b.close()
    a.close()
    return out


def measure_text_one(n, k):
    import ctypes as C
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
    nodes = st["distinct"]
    linked = timed(lambda: a.unitigs_begin_linked(1))
    nu, nb, nl = a.unitigs_begin_linked(1)
    out.update(nodes=nodes, unitigs=nu, bases=nb, n_links=nl)
    out["unitigs_begin_linked"] = dict(linked, nodes_per_s=nodes / linked["median_s"])
    out["text_begin"] = timed(lambda: a.unitigs_text_begin("gfa"))
    total = a.unitigs_text_begin("gfa")
    out["n_bytes"] = total
    piece = 64 << 20
    d_buf = torch.empty(piece, dtype=torch.uint8, device="cuda:0")
    pins = [native.PinnedArray(piece) for _ in range(3)]

    def timed_drain(next_piece):
        ts = []
        for rep in range(6):                  # one warm drain, then five; the begin in front of each is not timed
            assert a.unitigs_text_begin("gfa") == total
            torch.cuda.synchronize()
            got, i = 0, 0
            t0 = time.perf_counter()
            while True:
                m = next_piece(i)
                if m == 0:
                    break
                got += m
                i += 1
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            assert got == total
        ts = sorted(ts[1:])
        r = {"median_s": ts[len(ts) // 2], "spread_s": ts[-1] - ts[0]}
        return dict(r, bytes_per_s=total / r["median_s"])

    out["text_drain_device"] = timed_drain(lambda i: a.unitigs_text_next_device(d_buf))
    heads = []

    def next_pinned(i):
        m = a.unitigs_text_next(pins[i % 3].array)
        if i == 0:
            heads.append(bytes(pins[0].array[:11]))
        return m

    out["text_drain_pinned"] = timed_drain(next_pinned)
    out["text_share"] = (out["text_begin"]["median_s"] + out["text_drain_device"]["median_s"]) / linked["median_s"]
    assert len(heads) == 6 and set(heads) == {b"H\tVN:Z:1.0\n"}, heads
    for p in pins:
        p.close()
    rows = native.PinnedArray(max(4 * nu, 1), np.uint64)
    bases = native.PinnedArray(max(nb, 1))
    links = native.PinnedArray(max(nl, 1), np.uint64)
    L = native.lib()

    def copies():
        assert L.kh_unitigs_copy(a._h, rows.array.ctypes.data, nu, bases.array.ctypes.data, nb) == 0
        assert L.kh_unitigs_links_copy(a._h, links.array.ctypes.data, nl) == 0

    moved = 32 * nu + nb + 8 * nl
    c = timed(copies)
    out["copies_pinned"] = dict(c, bytes=moved, bytes_per_s=moved / c["median_s"])
    a.unitigs_end()
    a.close()
    return out


def measure_locate_one(n, k):
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
    out = {"k": k, "reads": n, "table": {f: st[f] for f in ("distinct", "kmers", "table_slots", "slot_bytes")}}
    begin = timed(lambda: a.unitigs_begin(1))
    nu, nb = a.unitigs_begin(1)
    out.update(nodes=st["distinct"], unitigs=nu, bases=nb, unitigs_begin=begin, index_bytes=8 * st["table_slots"])
    m = min(n, 1_000_000) * (rl + 1)            # the reads that are located: the first million of the table's own
    d_in = t[:m]
    d_loc = torch.empty(m, dtype=torch.int64, device="cuda:0")
    d_pro = torch.empty(m, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    out["window_starts"] = m

    def alternating(f, g, reps=5):
        """Medians of f and g, called in turn after one warm call of each."""
        f(), g()
        tf, tg = [], []
        for _ in range(reps):
            for fn, ts in ((f, tf), (g, tg)):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
        tf.sort(), tg.sort()
        return ({"median_s": tf[reps // 2], "spread_s": tf[-1] - tf[0]}, {"median_s": tg[reps // 2], "spread_s": tg[-1] - tg[0]})

    firsts = []
    for _ in range(5):                          # a begin releases the map: the next call builds it again
        a.unitigs_begin(1)
        t0 = time.perf_counter()
        a.unitigs_locate_device(d_in, None, m, d_loc)
        firsts.append(time.perf_counter() - t0)
    firsts.sort()
    out["locate_first"] = {"median_s": firsts[2], "spread_s": firsts[-1] - firsts[0]}
    loc, pro = alternating(lambda: a.unitigs_locate_device(d_in, None, m, d_loc), lambda: a.profile_device(d_in, None, m, d_pro))
    out["locate_device"] = dict(loc, starts_per_s=m / loc["median_s"], out_bytes_per_s=8 * m / loc["median_s"])
    out["profile_device"] = dict(pro, starts_per_s=m / pro["median_s"], out_bytes_per_s=4 * m / pro["median_s"])
    build = max(out["locate_first"]["median_s"] - loc["median_s"], 0.0)
    out["index_build"] = {"median_s": build, "index_share": build / begin["median_s"]}
    words, counts = d_loc.cpu().numpy().view(np.uint64), d_pro.cpu().numpy().view(np.uint32)
    assert np.array_equal(words == np.uint64(native.LOC_NO_WINDOW), counts == native.PROFILE_NO_WINDOW)
    assert np.array_equal(native.loc_is_place(words), (counts != native.PROFILE_NO_WINDOW) & (counts >= 1))
    out["places"] = int(np.sum(native.loc_is_place(words)))
    with native.PinnedArray(m) as pb, native.PinnedArray(m, np.uint64) as pl, native.PinnedArray(m, np.uint32) as pp:
        pb.array[:] = d_in.cpu().numpy()
        loc, pro = alternating(lambda: a.unitigs_locate(pb.array, out=pl.array), lambda: a.profile(pb.array, out=pp.array))
        assert np.array_equal(pl.array, words) and np.array_equal(pp.array, counts)
    out["locate_pinned"] = dict(loc, starts_per_s=m / loc["median_s"], out_bytes_per_s=8 * m / loc["median_s"])
    out["profile_pinned"] = dict(pro, starts_per_s=m / pro["median_s"], out_bytes_per_s=4 * m / pro["median_s"])
    a.unitigs_end()
    a.close()
    return out


def measure_paths_one(n, k):
    import ctypes as C
    import re
    import tempfile
    import numpy as np
    import torch
    from krust_amd import native
    rl = 150
    t = torch.empty(n * (rl + 1), dtype=torch.uint8, device="cuda:0")
    native.synth_reads_device(t.data_ptr(), None, 20260130, 1 << 28, rl, 0, n, device=0)
    torch.cuda.synchronize()
    nrec = min(n, 1_000_000)
    m = nrec * (rl + 1)                         # the reads that are walked: the first million of the table's own
    d_in = t[:m]
    rs = np.arange(0, m + 1, rl + 1, dtype=np.uint64)
    d_rs = torch.from_numpy(rs.view(np.int64)).cuda()
    d_st = torch.empty(nrec + 1, dtype=torch.int64, device="cuda:0")
    d_loc = torch.empty(m, dtype=torch.int64, device="cuda:0")
    out = {"k": k, "reads": n, "records": nrec, "window_starts": m}

    def alternating(f, g, reps=5):
        f(), g()
        tf, tg = [], []
        for _ in range(reps):
            for fn, ts in ((f, tf), (g, tg)):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
        tf.sort(), tg.sort()
        return ({"median_s": tf[reps // 2], "spread_s": tf[-1] - tf[0]}, {"median_s": tg[reps // 2], "spread_s": tg[-1] - tg[0]})

    def table(trace):
        a = native.DeviceCounter(k, device=0, trace=trace)
        a.push_device(t.data_ptr(), None, t.numel())
        a.finish()
        return a, a.unitigs_begin(1)

    a, (nu, nb) = table(False)
    d_cov = torch.zeros(nu * native.COV_WORDS, dtype=torch.int64, device="cuda:0")
    rc, runs = a.unitigs_paths_device(d_in, None, m, d_rs, nrec, d_st, None, 0, None)      # sizes, and builds the place map
    d_runs = torch.empty(max(runs, 1) * native.RUN_WORDS, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    out.update(unitigs=nu, runs=runs, runs_per_read=runs / nrec, bytes_out=16 * runs + 8 * (nrec + 1), locate_bytes_out=8 * m)
    pth, loc = alternating(lambda: a.unitigs_paths_device(d_in, None, m, d_rs, nrec, d_st, d_runs, runs, d_cov),
                           lambda: a.unitigs_locate_device(d_in, None, m, d_loc))
    out["paths_device"] = dict(pth, starts_per_s=m / pth["median_s"])
    out["locate_device"] = dict(loc, starts_per_s=m / loc["median_s"])
    out["paths_over_locate_device"] = pth["median_s"] / loc["median_s"]
    rows = d_runs.cpu().numpy().view(np.uint32).reshape(-1, native.RUN_WORDS)[:runs]
    words = d_loc.cpu().numpy().view(np.uint64)
    windows = int((rows[:, native.RUN_QEND] - rows[:, native.RUN_QSTART]).astype(np.int64).sum())
    assert windows == int(np.sum(native.loc_is_place(words)))      # every place lies in one run (a read's separator is no window)
    out["places"] = windows
    with native.PinnedArray(m) as pb, native.PinnedArray(m, np.uint64) as pl, native.PinnedArray(nrec + 1, np.uint64) as ps, \
            native.PinnedArray(max(runs, 1) * native.RUN_WORDS, np.uint32) as pr, native.PinnedArray(nu * native.COV_WORDS, np.uint64) as pc:
        pb.array[:] = d_in.cpu().numpy()
        pc.array[:] = 0
        total = C.c_uint64(0)

        def host_paths():
            rc = native.lib().kh_unitigs_paths(a._h, pb.array.ctypes.data, None, m, rs.ctypes.data, nrec, ps.array.ctypes.data, pr.array.ctypes.data,
                                               runs, pc.array.ctypes.data, C.byref(total))
            assert rc == native.KH_OK and total.value == runs
        pth, loc = alternating(host_paths, lambda: a.unitigs_locate(pb.array, out=pl.array))
        assert np.array_equal(pr.array.reshape(-1, native.RUN_WORDS)[:runs], rows) and np.array_equal(pl.array, words)
    out["paths_pinned"] = dict(pth, starts_per_s=m / pth["median_s"])
    out["locate_pinned"] = dict(loc, starts_per_s=m / loc["median_s"])
    out["paths_over_locate_pinned"] = pth["median_s"] / loc["median_s"]
    a.unitigs_end()
    a.close()
    # the split: one traced call of a second context, its line read back from the process's stderr
    b, _ = table(True)
    b.unitigs_paths_device(d_in, None, m, d_rs, nrec, d_st, d_runs, runs, d_cov)           # (warm: builds the place map)
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            b.unitigs_paths_device(d_in, None, m, d_rs, nrec, d_st, d_runs, runs, d_cov)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    line = [l for l in text.splitlines() if "kh_unitigs_paths_device:" in l]
    out["split_ms"] = {name: float(v) for name, v in re.findall(r"(\w+) ([0-9.]+) ms", line[-1])} if line else {"error": text[-500:]}
    b.unitigs_end()
    b.close()
    return out


def measure_support_one(n, k):
    import re
    import tempfile
    import numpy as np
    import torch
    from krust_amd import native
    rl = 150
    t = torch.empty(n * (rl + 1), dtype=torch.uint8, device="cuda:0")
    native.synth_reads_device(t.data_ptr(), None, 20260130, 1 << 28, rl, 0, n, device=0)
    torch.cuda.synchronize()
    nrec = min(n, 1_000_000)
    m = nrec * (rl + 1)                         # the reads that are walked: the first million of the table's own
    d_in = t[:m]
    rs = np.arange(0, m + 1, rl + 1, dtype=np.uint64)
    d_rs = torch.from_numpy(rs.view(np.int64)).cuda()
    d_st = torch.empty(nrec + 1, dtype=torch.int64, device="cuda:0")
    out = {"k": k, "reads": n, "records": nrec, "window_starts": m}

    def alternating(f, g, reps=5):
        f(), g()
        tf, tg = [], []
        for _ in range(reps):
            for fn, ts in ((f, tf), (g, tg)):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
        tf.sort(), tg.sort()
        return ({"median_s": tf[reps // 2], "spread_s": tf[-1] - tf[0]}, {"median_s": tg[reps // 2], "spread_s": tg[-1] - tg[0]})

    def table(trace):
        a = native.DeviceCounter(k, device=0, trace=trace)
        a.push_device(t.data_ptr(), None, t.numel())
        a.finish()
        return a, a.unitigs_begin_linked(1)

    a, (nu, nb, nl) = table(False)
    rc, runs = a.unitigs_paths_device(d_in, None, m, d_rs, nrec, d_st, None, 0, None)      # sizes, and builds the place map
    d_runs = torch.empty(max(runs, 1) * native.RUN_WORDS, dtype=torch.int32, device="cuda:0")
    d_sup = torch.zeros(max(nl, 1), dtype=torch.int64, device="cuda:0")
    d_cov = torch.zeros(nu * native.COV_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    out.update(unitigs=nu, links=nl, runs=runs)
    paths = lambda: a.unitigs_paths_device(d_in, None, m, d_rs, nrec, d_st, d_runs, runs, None)
    stats = {}

    def paths_then_support():
        paths()
        stats.update(a.unitigs_link_support_device(d_st, nrec, d_runs, runs, d_sup, nl))
    alone, with_support = alternating(paths, paths_then_support)
    out["paths_device"], out["paths_then_support"] = alone, with_support
    out["support_s"] = with_support["median_s"] - alone["median_s"]
    out["support_over_paths"] = out["support_s"] / alone["median_s"]
    d_sup.zero_()
    torch.cuda.synchronize()
    stats = a.unitigs_link_support_device(d_st, nrec, d_runs, runs, d_sup, nl)
    support = d_sup.cpu().numpy().view(np.uint64)[:nl]
    out.update(stats=stats, crossings=stats["adjacent"], links_without_support=float(np.mean(support == 0)) if nl else 0.0)
    assert stats["missing"] == 0 and int(support.sum()) == stats["credited"]

    def host_route():                           # the rows copied back, the crossing words looked up in the link array on the CPU
        run_start = d_st.cpu().numpy().view(np.uint64)
        rows = d_runs.cpu().numpy().view(np.uint32).reshape(-1, native.RUN_WORDS)[:runs]
        last = np.zeros(runs, dtype=bool)
        last[run_start[1:][run_start[1:] > run_start[:-1]] - np.uint64(1)] = True          # the last row of every record that has one
        pair = ~last[:-1] & (rows[:-1, native.RUN_QEND] == rows[1:, native.RUN_QSTART])
        words = (rows[:-1, native.RUN_STATE].astype(np.uint64) << np.uint64(32)) | rows[1:, native.RUN_STATE].astype(np.uint64)
        words = words[pair]
        at = np.searchsorted(links, words)
        hit = (at < nl) & (links[np.minimum(at, nl - 1)] == words)
        return np.bincount(at[hit], minlength=nl).astype(np.uint64)
    links = a.unitigs_links_copy(nl)
    assert np.array_equal(host_route(), support)
    out["host_route"] = timed(host_route)
    a.unitigs_end()
    a.close()
    # the split: one traced call each of a second context, the lines read back from the process's stderr
    b, _ = table(True)
    b.unitigs_paths_device(d_in, None, m, d_rs, nrec, d_st, d_runs, runs, d_cov)           # (warm: builds the place map)
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            b.unitigs_paths_device(d_in, None, m, d_rs, nrec, d_st, d_runs, runs, d_cov)
            b.unitigs_link_support_device(d_st, nrec, d_runs, runs, d_sup, nl)             # the first: builds the index
            b.unitigs_link_support_device(d_st, nrec, d_runs, runs, d_sup, nl)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    split = lambda l: {name: float(v) for name, v in re.findall(r"(\w+) ([0-9.]+) ms", l)}
    sup = [l for l in text.splitlines() if "kh_unitigs_link_support_device:" in l]
    pth = [l for l in text.splitlines() if "kh_unitigs_paths_device:" in l]
    out["split_ms"] = ({"first": split(sup[0]), "later": split(sup[-1]), "paths": split(pth[-1])} if len(sup) == 2 and pth else {"error": text[-500:]})
    b.unitigs_end()
    b.close()
    return out


def measure_components_one(n, k):
    import re
    import tempfile
    import numpy as np
    import torch
    from krust_amd import native
    rl = 150
    t = torch.empty(n * (rl + 1), dtype=torch.uint8, device="cuda:0")
    native.synth_reads_device(t.data_ptr(), None, 20260130, 1 << 28, rl, 0, n, device=0)
    torch.cuda.synchronize()

    def table(trace):
        a = native.DeviceCounter(k, device=0, trace=trace)
        a.push_device(t.data_ptr(), None, t.numel())
        return a, a.finish()

    a, st = table(False)
    nodes = st["distinct"]
    out = {"k": k, "reads": n, "table": {f: st[f] for f in ("distinct", "kmers", "table_slots", "slot_bytes")}}
    nu, nb, nl = a.unitigs_begin_linked(1)
    rc, stats = a.unitigs_components_device(None, 0, None, 0)
    nc = stats["components"]
    d_comp = torch.empty(max(nu, 1), dtype=torch.int32, device="cuda:0")
    d_rows = torch.empty(max(nc, 1) * native.COMP_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    out.update(unitigs=nu, links=nl, stats=stats)
    tb, tf, tc = [], [], []
    for rep in range(6):                          # one warm round, then five
        t0 = time.perf_counter()
        a.unitigs_begin_linked(1)
        t1 = time.perf_counter()
        a.unitigs_components_device(d_comp, nu, d_rows, nc)
        t2 = time.perf_counter()
        a.unitigs_components_device(d_comp, nu, d_rows, nc)
        t3 = time.perf_counter()
        tb.append(t1 - t0), tf.append(t2 - t1), tc.append(t3 - t2)
    med = lambda ts: {"median_s": sorted(ts[1:])[len(ts[1:]) // 2], "spread_s": max(ts[1:]) - min(ts[1:])}
    out["unitigs_begin_linked"], out["components_first"], out["components_cached"] = med(tb), med(tf), med(tc)
    out["first_over_begin"] = out["components_first"]["median_s"] / out["unitigs_begin_linked"]["median_s"]
    comp = d_comp.cpu().numpy().view(np.uint32)[:nu]
    rows = d_rows.cpu().numpy().view(np.uint64)[:nc * native.COMP_WORDS].reshape(nc, native.COMP_WORDS)
    assert int(rows[:, native.COMP_UNITIGS].sum()) == nu and int(rows[:, native.COMP_KMERS].sum()) == nodes
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        by = "scipy.sparse.csgraph.connected_components"
    except ImportError:
        connected_components, by = None, "numpy hook and compress"
    got = {}

    def host_route():
        links = a.unitigs_links_copy(nl)
        fr, to = (links >> np.uint64(33)).astype(np.int64), ((links & np.uint64(0xFFFFFFFF)) >> np.uint64(1)).astype(np.int64)
        if connected_components is not None:
            g = coo_matrix((np.ones(fr.size, dtype=np.int8), (fr, to)), shape=(nu, nu))
            got["n"], got["labels"] = connected_components(g, directed=False)
            return
        sel = fr < to
        x, y = fr[sel], to[sel]
        parent = np.arange(nu, dtype=np.int64)
        while True:
            ra, rb = parent[x], parent[y]
            d = ra != rb
            if not d.any():
                break
            np.minimum.at(parent, np.maximum(ra, rb)[d], np.minimum(ra, rb)[d])
            while True:
                nxt = parent[parent]
                if np.array_equal(nxt, parent):
                    break
                parent = nxt
        got["labels"], got["n"] = parent, int(np.sum(parent == np.arange(nu)))

    out["host_route"] = dict(timed(host_route), host_route_by=by)
    first = np.full(got["labels"].max() + 1 if nu else 0, nu, dtype=np.int64)           # the host's labels, made the library's: by first unitig
    np.minimum.at(first, got["labels"], np.arange(nu))
    assert got["n"] == nc and np.array_equal(np.searchsorted(np.unique(first[got["labels"]]), first[got["labels"]]), comp)
    a.unitigs_end()
    b = native.DeviceCounter(k, device=0, capacity_hint=nodes)
    words = {}
    tcl, tdr = [], []
    for rep in range(6):                          # one warm round, then five, the two calls alternating
        for name, fn, ts in (("clip", lambda: b.clip_tips_into(a, 1, k), tcl), ("drop", lambda: b.drop_components_into(a, 1, 2 * k), tdr)):
            b.reset()
            t0 = time.perf_counter()
            words[name] = fn()
            ts.append(time.perf_counter() - t0)
    out["clip_tips_into"], out["drop_components_into"] = med(tcl), med(tdr)
    out["drop_words"] = words["drop"]
    sb = b.finish()
    assert sb["distinct"] == words["drop"]["kept_kmers"] and words["drop"]["kept_kmers"] + words["drop"]["dropped_kmers"] == nodes
    assert words["drop"]["components"] == nc and words["drop"]["dropped"] == int(np.sum(rows[:, native.COMP_KMERS] < np.uint64(2 * k)))
    b.close()
    a.close()
    # the split: one traced first call of a second context, the line read back from the process's stderr
    c, _ = table(True)
    c.unitigs_begin_linked(1)
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            c.unitigs_components_device(d_comp, nu, d_rows, nc)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    line = [l for l in text.splitlines() if "kh_unitigs_components_device:" in l]
    out["split_ms"] = ({name.strip().replace(" ", "_"): float(v) for name, v in re.findall(r"([a-z ]+) ([0-9.]+) ms", line[-1])} if line else {"error": text[-500:]})
    c.unitigs_end()
    c.close()
    return out


def measure(args):
    if args.components:
        print("RESULT " + json.dumps([measure_components_one(n, args.k) for n in args.reads]))
        return
    if args.support:
        print("RESULT " + json.dumps([measure_support_one(n, args.k) for n in args.reads]))
        return
    if args.paths:
        print("RESULT " + json.dumps([measure_paths_one(n, args.k) for n in args.reads]))
        return
    if args.locate:
        print("RESULT " + json.dumps([measure_locate_one(n, args.k) for n in args.reads]))
        return
    if args.text:
        print("RESULT " + json.dumps([measure_text_one(n, args.k) for n in args.reads]))
        return
    one = (lambda n, k: measure_clip_one(n, k, pop=True)) if args.pop else measure_clip_one if args.clip else measure_one
    print("RESULT " + json.dumps([one(n, args.k) for n in args.reads]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--clip", action="store_true", help="kh_clip_tips_into beside kh_unitigs_begin_linked, nothing else")
    ap.add_argument("--pop", action="store_true", help="kh_pop_bubbles_into beside kh_clip_tips_into and kh_unitigs_begin_linked, nothing else")
    ap.add_argument("--text", action="store_true", help="kh_unitigs_text_* beside kh_unitigs_begin_linked and the copies, one process per size")
    ap.add_argument("--locate", action="store_true", help="kh_unitigs_locate* beside kh_profile* and kh_unitigs_begin, one process per size")
    ap.add_argument("--paths", action="store_true", help="kh_unitigs_paths* beside kh_unitigs_locate* on the reads of --locate, one process per size")
    ap.add_argument("--support", action="store_true", help="kh_unitigs_link_support_device behind kh_unitigs_paths_device on the reads of --paths, one process per size")
    ap.add_argument("--components", action="store_true", help="kh_unitigs_components_device behind kh_unitigs_begin_linked, kh_drop_components_into beside kh_clip_tips_into, one process per size")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        measure(args)
        return
    if args.text or args.locate or args.paths or args.support or args.components:   # one process per size
        which = "--components" if args.components else "--support" if args.support else "--paths" if args.paths else "--locate" if args.locate else "--text"
        res = []
        for n in args.reads:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--k", str(args.k), "--reads", str(n)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
                line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    res.append({"reads": n, "error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]})
                    break   # (nothing more is started on a device that may have faulted)
                res += json.loads(line[-1][7:])
            except subprocess.TimeoutExpired:
                res.append({"reads": n, "error": f"no result within {args.timeout} s"})
                break
        print(json.dumps({"probe": "unitig-components" if args.components else "unitig-link-support" if args.support else "unitig-paths" if args.paths else "unitig-locate" if args.locate else "unitig-text", "result": res}, indent=1))
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--k", str(args.k)] + (["--clip"] if args.clip else []) + (["--pop"] if args.pop else []) + ["--reads"] + [str(n) for n in args.reads]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        res = json.loads(line[-1][7:]) if p.returncode == 0 and line else {"error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]}
    except subprocess.TimeoutExpired:
        res = {"error": f"no result within {args.timeout} s"}
    print(json.dumps({"probe": "unitig-pop" if args.pop else "unitig-clip" if args.clip else "unitig", "result": res}, indent=1))


if __name__ == "__main__":
    main()
