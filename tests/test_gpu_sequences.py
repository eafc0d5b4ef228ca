"""Random call sequences across the whole C ABI, on tables in every form, against the model of tests/seq_model.py.

Every kh_* call enters its context through one of the presets of krust_amd/csrc/ctx.hip.h; what they count, widen, clear and end
shows only in what the NEXT calls return.  The hand-written interleaving tests each script one order on one table form.  Here the
committed seeds walk about a hundred calls each over three contexts A, B and D -- pushes of three kinds, merges, set operations,
clipping and popping between them, every reader, text streams in pieces, unitigs and their copies, a one-rank merge -- and after
every call hold the device to the model: the status, every returned value (exactly: integers and bytes), canaries on a refusal,
kh_stats unchanged under everything the header classes as reading, and every ten steps the full content of every context.
Nothing but the sequence's own calls enters a context behind a reset, a push or a merge: the next call finds what they left.
tests/test_seq_model.py shows on the CPU that these seeds reach the states that matter.

The graph walks (test_graph_sequence) are a second committed family: sessions on live unitigs that draw kh_unitigs_text_begin /
_next / _next_device and kh_unitigs_locate / _locate_device between everything above -- pieces of the unitig text (a byte range: the
count and the bytes exact, nothing at or behind buf[n], the device form at an odd offset into a torch buffer) in turns with pieces
of a kh_result_text_* stream, locate words of both forms (exact, and a walk in the links where there are links), restarts, second
begins, kh_profile next to the host form that shares its chunk buffers -- with KMERHIP_UNI_TEXT_CHUNK_KB=8 and
KMERHIP_PROFILE_CHUNK_KB=1, so that the stream's two chunks turn over and the host forms take several chunks at the pool's size.

Both families run under KMERHIP_ALLOC_TRACE (the Trace of tests/test_gpu_alloc_fail.py).  The place map of kh_unitigs_locate* is
the one allocation of table_slots * 8 bytes that a successful first locate call of a begin makes and leaves live; a later
kh_unitigs_locate_device allocates nothing; the map's release is among the events of the call that releases the unitigs -- those
the header names: kh_unitigs_end, the next begin, kh_reset, and the src of clip and pop (a writer only makes the unitigs stale:
their memory stays the context's until one of these; kh_merge_across over a communicator resets inside) --; and after the last
kh_destroy nothing the library allocated since the runner was built is live.

A failure prints the seed, the forms, the step and the calls up to it as lines that replay() runs again: a regression test for a
bug found here is `replay([...], forms, monkeypatch)` (for a graph walk: `env=seq_model.GRAPH_ENV`)."""
import ctypes as C
import os

import numpy as np
import pytest

import seq_model as M
import test_gpu_join as T
from krust_amd import native
from test_gpu_alloc_fail import tr  # noqa: F401  (the module's trace fixture: a Trace over KMERHIP_ALLOC_TRACE)

pytestmark = pytest.mark.gpu

U64 = np.uint64
CANARY = 0xA5
CANARY64 = 0xA5A5A5A5A5A5A5A5
DEVICE_OFFSET = 13       # kh_unitigs_text_next_device writes at this odd offset into a torch buffer
# what releases the unitigs' memory, the place map with it: "kh_unitigs_end, the next begin, kh_reset, kh_destroy" -- and the src of
# clip and pop, whose begin it is.  (A push or a merge makes them stale; the memory stays the context's until one of these.)
RELEASES = ("unitigs_end", "unitigs_begin", "unitigs_begin_linked", "reset", "clip_tips_into.src", "pop_bubbles_into.src")
SEEDS = int(os.environ.get("KMERHIP_SEQ_SEEDS", str(M.SEEDS)))   # (more: KMERHIP_SEQ_SEEDS=100 pytest tests/test_gpu_sequences.py)
GRAPH_SEEDS = int(os.environ.get("KMERHIP_SEQ_SEEDS", str(M.GRAPH_SEEDS)))


# ---- the three contexts, each in its form ------------------------------------------------------------------------------------------
def build(form, k, r, monkeypatch):
    """A counter that holds the reads r in the form asked for, built as test_gpu_join.table() builds them; the form it reports is
    asserted.  The path stays forced for the context's lifetime: the form changes only through the calls themselves."""
    if form in ("wide", "image", "regions3072"):
        return T.table(form, k, r, monkeypatch)
    if form == "grown":          # a first table of 64 regions that has to grow needs more keys than the pool has: grown, reset, filled
        dc = T.table("grown", k, T.reads(0, 6000), monkeypatch)
        dc.reset()
        dc.push(r)
        st = dc.finish()
        assert st["grows"] >= 1 and st["table_slots"] > 64 * 4096
        return dc
    dc = native.DeviceCounter(k, capacity_hint=3_000_000, path="partition")
    if form == "borrow":         # `image` with a communicator of one rank (before anything is counted: kh_comm_init enters as a writer)
        dc.comm_init(1, 0, native.comm_unique_id())
    dc.push(r)
    st = dc.finish()
    if form == "borrow":
        assert st["slot_bytes"] == 8 and st["part_batches"] >= 1 and st["table_slots"] == (1 << 11) * 4096
    else:                        # wide-part, k = 31: a 16-byte table AND partition buffers
        assert form == "wide-part" and st["slot_bytes"] == 16 and st["part_batches"] >= 1
    return dc


class Runner:
    """The model and the three device contexts, one call at a time."""

    def __init__(self, forms, monkeypatch, trace=None):
        import torch
        self.forms, self.k = tuple(forms), M.k_of(forms)
        # the allocation trace: what was live before the first context was built, and per context the pointer of its place map
        self.tr = trace
        self.live_before = set(trace.snapshot()) if trace else None
        self.where = {name: None for name in M.CTXS}
        self.model = M.Model(self.k)
        self.pool = self.model.pool
        self.L = native.lib()
        self.dc = {}
        try:
            for name, form in zip(M.CTXS, forms):
                self.dc[name] = build(form, self.k, self.pool.reads[0], monkeypatch)
            self.d_reads = [torch.from_numpy(r).to("cuda:0") for r in self.pool.reads]     # (alive for the whole sequence)
            torch.cuda.synchronize()
            self.stats = {name: self.held(name) for name in M.CTXS}    # kh_stats as of the last call, None while a push is pending
        except BaseException:
            self.close()
            raise

    def close(self):
        for dc in self.dc.values():
            dc.close()
        self.dc = {}

    def leaked(self):
        """After close(): what the library allocated since the runner was built and has not released."""
        return {p: v for p, v in self.tr.snapshot().items() if p not in self.live_before}

    def held(self, name):
        """stats_of() of a context with nothing pending; its distinct and kmers are the model's."""
        st = T.stats_of(self.dc[name])
        c = self.model.ctx[name]
        assert (st[1], st[2]) == (c.keys.size, c.total()), (name, "distinct, kmers", st[1], st[2], "model", c.keys.size, c.total())
        return st

    def refused(self, name, arrays):
        for a in arrays:
            assert (a == CANARY).all(), "a refused call wrote to its output"
        assert self.L.kh_last_error(self.dc[name]._h), "a refused call left no error text"

    # -- one call: what it returns against exp ---------------------------------------------------------------------------------------
    def call(self, op, exp):
        dc = self.dc
        kind = op.kind
        if kind == "push":
            dc[op.ctx].push(self.pool.reads[op.chunk])
        elif kind == "push_device":
            t = self.d_reads[op.chunk]
            dc[op.ctx].push_device(t.data_ptr(), None, t.numel())
        elif kind == "push_text":
            dc[op.ctx].push_text(self.pool.fasta[op.chunk], "fasta")
        elif kind == "reset":
            dc[op.ctx].reset()
        elif kind == "merge_pairs":
            dc[op.ctx].merge_pairs(*self.pool.pairs[op.chunk])
        elif kind == "combine_into":
            assert dc[op.dst].combine_into(dc[op.a], dc[op.b], op.op, op.calc) == exp["n_pairs"]
        elif kind in ("clip_tips_into", "pop_bubbles_into"):
            words = getattr(dc[op.dst], kind)(dc[op.src], op.mc)
            assert list(words.values()) == exp["words"], (words, exp["words"])
        elif kind == "merge_across":
            info = dc[op.ctx].merge_across()
            assert (info["owned_distinct"], info["conserved"], info["merged_count_sum"], info["nranks"]) == \
                (exp["owned_distinct"], exp["conserved"], exp["merged_count_sum"], 1), info
        elif kind == "finish":
            st = dc[op.ctx].finish()
            assert (st["kmers"], st["distinct"]) == (exp["kmers"], exp["distinct"])
        elif kind == "result_size":
            assert dc[op.ctx].result_size(op.mc) == exp["n"]
        elif kind in ("result", "result_sorted"):
            gk, gc = getattr(dc[op.ctx], kind)(op.mc)
            assert np.array_equal(gk, exp["keys"]) and np.array_equal(gc, exp["counts"])
        elif kind == "audit":
            gk, gc = dc[op.ctx].result_sorted(1)
            assert np.array_equal(gk, exp["keys"]) and np.array_equal(gc, exp["counts"]), "the table is not the model's content"
            assert dc[op.ctx].histogram(1) == exp["histogram"]
        elif kind == "histogram":
            assert dc[op.ctx].histogram(op.mc) == exp["histogram"]
        elif kind == "lookup":
            assert np.array_equal(dc[op.ctx].lookup(exp["query"]), exp["counts"])
        elif kind == "profile":
            assert np.array_equal(dc[op.ctx].profile(exp["bases"]), exp["profile"])
        elif kind == "compare":
            assert dc[op.a].compare(dc[op.b]) == exp["words"]
        elif kind == "graph_stats":
            assert np.array_equal(dc[op.ctx].graph_stats(op.mc), exp["words"])
        elif kind == "graph_masks":
            assert np.array_equal(dc[op.ctx].graph_masks(exp["query"], op.mc), exp["masks"])
        elif kind == "text_begin":
            assert dc[op.ctx].result_text_begin(op.fmt, op.mc, sorted=op.sorted) == (exp["n_records"], exp["n_bytes"])
        elif kind == "text_next":
            buf = np.full(op.cap + 16, CANARY, dtype=np.uint8)
            n = C.c_uint64(0)
            rc = self.L.kh_result_text_next(dc[op.ctx]._h, buf.ctypes.data, op.cap, C.byref(n))
            assert rc == exp.status, (rc, exp.status, self.L.kh_last_error(dc[op.ctx]._h))
            if rc != M.OK:
                self.refused(op.ctx, [buf])
            else:
                # (exp["n"], as many whole records as fit, is what the coverage walk moves on by: the header promises whole records
                #  and at most cap bytes, not the most that fit, so the device's n is not held to it)
                assert n.value <= op.cap and (buf[n.value:] == CANARY).all()
                self.model.text_piece(op.ctx, int(n.value), buf[:n.value].tobytes(), op.cap)
        elif kind in ("unitigs_begin", "unitigs_begin_linked"):
            got = getattr(dc[op.ctx], kind)(op.mc)
            want = (exp["n_unitigs"], exp["n_bases"]) + ((exp["n_links"],) if kind == "unitigs_begin_linked" else ())
            assert got == want, (got, want)
        elif kind == "unitigs_copy":
            ok = exp.status == M.OK
            nu, nb = (exp["rows"].shape[0], len(exp["bases"])) if ok else (4, 16)
            rows = np.full((nu + 1, native.UNI_WORDS), CANARY, dtype=U64)
            bases = np.full(nb + 8, CANARY, dtype=np.uint8)
            rc = self.L.kh_unitigs_copy(dc[op.ctx]._h, rows.ctypes.data, nu, bases.ctypes.data, nb)
            assert rc == exp.status, (rc, exp.status, self.L.kh_last_error(dc[op.ctx]._h))
            if not ok:
                self.refused(op.ctx, [rows, bases])
            else:
                assert (rows[nu:] == CANARY).all() and (bases[nb:] == CANARY).all()
                assert np.array_equal(rows[:nu], exp["rows"]) and bases[:nb].tobytes() == exp["bases"]
        elif kind == "links_copy":
            ok = exp.status == M.OK
            nl = exp["links"].size if ok else 8
            links = np.full(nl + 1, CANARY, dtype=U64)
            rc = self.L.kh_unitigs_links_copy(dc[op.ctx]._h, links.ctypes.data, nl)
            assert rc == exp.status, (rc, exp.status, self.L.kh_last_error(dc[op.ctx]._h))
            if not ok:
                self.refused(op.ctx, [links])
            else:
                assert links[nl] == CANARY and np.array_equal(links[:nl], exp["links"])
        elif kind == "unitigs_end":
            dc[op.ctx].unitigs_end()
        elif kind == "unitigs_text_begin":
            nb = C.c_uint64(0)
            rc = self.L.kh_unitigs_text_begin(dc[op.ctx]._h, {"fasta": native.KH_UNI_TEXT_FASTA, "gfa": native.KH_UNI_TEXT_GFA}[op.fmt], C.byref(nb))
            assert rc == exp.status, (rc, exp.status, self.L.kh_last_error(dc[op.ctx]._h))
            if rc != M.OK:
                self.refused(op.ctx, [])
            else:
                assert nb.value == exp["n_bytes"], (nb.value, exp["n_bytes"])
        elif kind == "unitigs_text_next":
            n = C.c_uint64(0)
            if op.device:       # into a torch buffer at an odd offset, canaries in front and behind
                import torch
                t = torch.full((DEVICE_OFFSET + op.cap + 19,), CANARY, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                rc = self.L.kh_unitigs_text_next_device(dc[op.ctx]._h, t.data_ptr() + DEVICE_OFFSET, op.cap, C.byref(n))
                buf = t.cpu().numpy()
                assert (buf[:DEVICE_OFFSET] == CANARY).all(), "kh_unitigs_text_next_device wrote in front of d_buf"
                buf = buf[DEVICE_OFFSET:]
            else:
                buf = np.full(op.cap + 16, CANARY, dtype=np.uint8)
                rc = self.L.kh_unitigs_text_next(dc[op.ctx]._h, buf.ctypes.data, op.cap, C.byref(n))
            assert rc == exp.status, (rc, exp.status, self.L.kh_last_error(dc[op.ctx]._h))
            if rc != M.OK:
                self.refused(op.ctx, [buf])
            else:               # a byte range: the count is exact, the bytes are the document's, nothing at or behind buf[n]
                assert n.value == exp["n"], (n.value, exp["n"], op.cap)
                assert (buf[n.value:] == CANARY).all(), "a piece wrote at or behind buf[n]"
                self.model.unitig_text_piece(op.ctx, int(n.value), buf[:n.value].tobytes())
        elif kind == "unitigs_locate":
            flat = self.model.flat(op)
            out = np.full(flat.size + 2, CANARY64, dtype=U64)
            if op.device:
                import torch
                a = op.read * (M.READ_LEN + 1)
                d_in = self.d_reads[op.chunk][a:a + flat.size]      # (a view: at whatever alignment the read starts)
                d_out = torch.from_numpy(out.view(np.int64)).to("cuda:0")
                torch.cuda.synchronize()
                rc = self.L.kh_unitigs_locate_device(dc[op.ctx]._h, d_in.data_ptr(), None, flat.size, d_out.data_ptr())
                out = d_out.cpu().numpy().view(U64)
            else:
                rc = self.L.kh_unitigs_locate(dc[op.ctx]._h, flat.ctypes.data, None, flat.size, out.ctypes.data)
            assert rc == exp.status, (rc, exp.status, self.L.kh_last_error(dc[op.ctx]._h))
            if rc != M.OK:
                self.refused(op.ctx, [out.view(np.uint8)])
            else:
                import test_locate_ref as LO
                assert (out[flat.size:] == U64(CANARY64)).all(), "kh_unitigs_locate wrote behind its n words"
                words = out[:flat.size]
                if not np.array_equal(words, exp["words"]):
                    i = int(np.flatnonzero(words != exp["words"])[0])
                    raise AssertionError("window %d of %d: %r for %r" % (i, flat.size, LO.fields(words[i:i + 1]), LO.fields(exp["words"][i:i + 1])))
                if exp["links"] is not None:                           # a read is a walk in the GFA
                    LO.check_walk(words, exp["rows"], exp["links"], self.k)
        else:
            raise AssertionError(kind)

    # -- the allocation trace: the place map's lifetime --------------------------------------------------------------------------
    def before_call(self, op):
        """What the model knows before the call is applied: which contexts' unitigs this call releases, and whether a locate call
        finds the place map built."""
        self.tr.sync()
        self.releasing = [name for role, name, _ in op.roles() if M.role_name(op.kind, role) in RELEASES]
        u = self.model.ctx[op.ctx].unitigs if op.kind == "unitigs_locate" else None
        self.located_before = None if u is None else u["located"]

    def after_call(self, op, exp):
        """Right after the call returned, before anything else enters a context: the events of this call alone."""
        ev = self.tr.sync()
        # A map that no call has released is the context's still -- live unitigs or stale ones: a writer only makes them stale.  The one
        # call outside RELEASES that may give it back is kh_merge_across over a communicator, which resets inside -- and then stale ones only.
        for name in M.CTXS:
            if self.where[name] is not None and name not in self.releasing and ("F", self.where[name]) in ev:
                assert op.kind == "merge_across" and op.ctx == name, (name, "the place map was released by a call that releases no unitigs", op)
                assert self.model.ctx[name].unitigs is None, (name, "the place map of live unitigs was released")
                self.where[name] = None
        for name in self.releasing:
            if self.where[name] is not None:   # (its release in this call's events: the address may be live again as something else)
                assert ("F", self.where[name]) in ev, (name, "the place map outlived the call that releases the unitigs", self.where[name], ev)
                self.where[name] = None
        if op.kind == "unitigs_locate" and exp.status == M.OK:
            new = [e for e in ev if e[0] == "A" and e[2] in self.tr.live]            # allocated by this call, live when it returned
            if self.located_before:
                assert self.where[op.ctx] in self.tr.live, "the place map is gone while its unitigs are live"
                if op.device:
                    assert not [e for e in ev if e[0] == "A"], ("a later kh_unitigs_locate_device allocates nothing", ev)
            else:                   # the first locate call of this begin: one allocation of table_slots * 8 bytes stays, the place map
                slots = T.stats_of(self.dc[op.ctx])[4]
                index = [e for e in new if e[1] == "dev" and int(e[3]) == 8 * slots]
                assert len(index) == 1, ("the first locate call after a begin builds one place map of table_slots * 8 bytes", slots, ev)
                if op.device:
                    assert len(new) == 1, ("... and nothing else of it stays allocated", new)
                self.where[op.ctx] = index[0][2]

    def step(self, op):
        """One call, then kh_stats of the contexts it READ or added to as a `dst` -- and of no other: after kh_reset, a push or
        kh_merge_pairs nothing enters the context before the next call of the sequence does, so that call finds the table as the
        writer left it (lazily reset, pending, not yet widened), not as a kh_finish in between would have made it."""
        before = {name: self.stats[name] for _, name, _ in op.roles()}
        if self.tr:
            self.before_call(op)
        exp = self.model.apply(op)
        self.call(op, exp)
        if self.tr:
            self.after_call(op, exp)
        for role, name, cls in op.roles():
            if cls is None:
                continue
            reading = cls in M.READING_CLASSES
            if self.model.ctx[name].pending or not (reading or role == "dst"):
                self.stats[name] = None            # (kh_finish would count what is pending, and clear what is lazily reset)
                continue
            st = self.held(name)                   # distinct and kmers are the model's
            # a reader never widens, grows or recounts -- kh_merge_across apart, which reads the table and builds it again
            if reading and before[name] is not None and op.kind != "merge_across":
                assert st == before[name], (name, "kh_stats changed under a reading call", before[name], st)
            self.stats[name] = st


def run(ops, forms, monkeypatch, label="", trace=None):
    """trace: a test_gpu_alloc_fail.Trace.  With one, the place map's lifetime is held to the header after every call, and after
    close() nothing the library allocated since the runner was built may be live."""
    r = Runner(forms, monkeypatch, trace)
    try:
        for i, op in enumerate(ops):
            try:
                r.step(op)
            except Exception as e:
                lines = "\n".join("    %r," % repr(o) for o in ops[:i + 1])
                raise AssertionError(f"{label} forms {tuple(forms)} step {i}: {op!r}: {type(e).__name__}: {e}\n"
                                     f"replay([\n{lines}\n], {tuple(forms)!r}, monkeypatch)") from e
    finally:
        r.close()
    if trace:
        left = r.leaked()
        assert not left, f"{label} forms {tuple(forms)}: still allocated after every context was destroyed: {left}"


def replay(lines, forms, monkeypatch, env=None, trace=None):
    """Runs a list of op lines (the repr of seq_model.Op, as a failure prints them) on contexts of the given forms.  env: the
    switches the failing test ran under (seq_model.GRAPH_ENV for a graph walk)."""
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    run([M.parse(line) for line in lines], forms, monkeypatch, label="replay", trace=trace)


@pytest.mark.parametrize("seed,forms", M.cases(SEEDS), ids=lambda v: "-".join(v) if isinstance(v, tuple) else f"s{v}")
def test_sequence(seed, forms, monkeypatch, tr):  # noqa: F811
    run(M.case_sequence(seed, forms), forms, monkeypatch, label=f"seed {seed}", trace=tr)


@pytest.mark.parametrize("seed,forms", M.graph_cases(GRAPH_SEEDS), ids=lambda v: "-".join(v) if isinstance(v, tuple) else f"s{v}")
def test_graph_sequence(seed, forms, monkeypatch, tr):  # noqa: F811
    """The graph walks: sessions on live unitigs, with one tile per chunk of the unitig text stream and 1024 window starts per chunk
    of the two host forms, under the allocation trace."""
    for name, value in M.GRAPH_ENV.items():
        monkeypatch.setenv(name, value)
    run(M.graph_case_sequence(seed, forms), forms, monkeypatch, label=f"graph seed {seed}", trace=tr)


def test_replay_runs_a_printed_list(monkeypatch):
    """The helper itself: a stream cut short by a push, the refusals behind it, and the audit."""
    replay(["Op('text_begin', ctx='A', fmt='json', mc=1, sorted=True)",
            "Op('text_next', ctx='A', cap=8)",
            "Op('text_next', ctx='A', cap=65536)",
            "Op('unitigs_begin', ctx='A', mc=2)",
            "Op('text_next', ctx='A', cap=65536)",
            "Op('lookup', ctx='A', pick=1)",
            "Op('unitigs_copy', ctx='A')",
            "Op('links_copy', ctx='A')",
            "Op('push', ctx='A', chunk=1)",
            "Op('unitigs_copy', ctx='A')",
            "Op('audit', ctx='A')"], ("image", "wide", "wide"), monkeypatch)


def test_replay_runs_the_graph_kinds(monkeypatch, tr):  # noqa: F811
    """The same for the three kinds of the graph walks, under their switches and the trace: a stream in pieces of both forms with a
    locate call of each form and a kh_result_text_* piece between, a restart, a second begin, the end by kh_unitigs_end."""
    replay(["Op('unitigs_begin_linked', ctx='A', mc=1)",
            "Op('unitigs_text_begin', ctx='A', fmt='gfa')",
            "Op('unitigs_text_next', ctx='A', cap=0, device=False)",
            "Op('unitigs_text_next', ctx='A', cap=7, device=True)",
            "Op('unitigs_locate', ctx='A', chunk=1, read=3, device=True)",
            "Op('text_begin', ctx='A', fmt='tsv', mc=2, sorted=True)",
            "Op('unitigs_text_next', ctx='A', cap=20001, device=False)",
            "Op('text_next', ctx='A', cap=65536)",
            "Op('profile', ctx='A', chunk=2, read=7)",
            "Op('unitigs_locate', ctx='A', chunk=2, read=7, reads=16, device=False)",
            "Op('profile', ctx='A', chunk=2, read=9, reads=8)",
            "Op('unitigs_text_next', ctx='A', cap=9999, device=True)",
            "Op('unitigs_text_begin', ctx='A', fmt='fasta')",
            "Op('unitigs_text_next', ctx='A', cap=65536, device=False)",
            "Op('unitigs_begin', ctx='A', mc=2)",
            "Op('unitigs_text_next', ctx='A', cap=100, device=False)",
            "Op('unitigs_locate', ctx='A', chunk=0, read=499, device=False)",
            "Op('unitigs_text_begin', ctx='A', fmt='fasta')",
            "Op('unitigs_text_next', ctx='A', cap=65536, device=True)",
            "Op('unitigs_text_next', ctx='A', cap=65536, device=True)",
            "Op('unitigs_end', ctx='A')",
            "Op('unitigs_locate', ctx='A', chunk=0, read=0, device=True)",
            "Op('text_next', ctx='A', cap=65536)",
            "Op('audit', ctx='A')"], ("image", "wide", "wide"), monkeypatch, env=M.GRAPH_ENV, trace=tr)


@pytest.mark.parametrize("first", ["Op('clip_tips_into', dst='A', src='B', mc=2)", "Op('pop_bubbles_into', dst='A', src='B', mc=1)",
                                   "Op('combine_into', dst='A', a='B', b='D', op='union', calc='sum')", "Op('merge_pairs', ctx='A', chunk=2)",
                                   "Op('push_device', ctx='A', chunk=2)", "Op('lookup', ctx='A', pick=7)"],
                         ids=lambda line: line.split("'")[1])
@pytest.mark.parametrize("forms", [("wide", "image", "wide"), ("image", "wide", "image"), ("wide-part", "wide-part", "wide-part")],
                         ids=lambda f: "-".join(f))
def test_the_first_call_after_reset_finds_the_table_lazily_reset(first, forms, monkeypatch):
    """kh_reset is lazy: the slots keep their stale pairs until the next call clears or overwrites them.  A held content, the
    reset, and at once -- no call between -- each kind of first call; then the content.  (A writer whose entry skips the clear
    leaves the stale pairs in: the audit, or `distinct` of the dst, shows them.)"""
    replay(["Op('merge_pairs', ctx='A', chunk=1)",        # (an image becomes a 16-byte table that exists and holds content)
            "Op('reset', ctx='A')",
            first,
            "Op('audit', ctx='A')"], forms, monkeypatch)
