"""A plain model of the C ABI's contexts, and random call sequences drawn against it.  No device: numpy, the oracle and the Python
references the other tests already hold the kernels to.

Every kh_* call enters its context through one of six presets (krust_amd/csrc/ctx.hip.h, Entry) that decide what is counted,
widened, cleared and ended on the way in.  The model knows none of that machinery: a context is its expected content -- a sorted
(keys, counts) pair --, whether something is pushed and not yet counted, a text stream or none, unitigs or none.  ENTRY below
restates from include/kmerhip.h which call enters which context how, and the one rule that follows from it: whatever does not
enter as a reader ends the stream and the unitigs.  Model.apply(op) gives the status and the values a call must return;
sequence(seed, n_steps) draws calls with weights that depend on the model, so that streams and unitigs are interleaved with
readers and cut short by writers; coverage() says what a set of sequences reaches.  tests/test_seq_model.py holds the model to the
oracle and the committed sequences to their coverage; tests/test_gpu_sequences.py runs them on the device.

The model never records which form a table is in (16-byte table, 8-byte image, grown, borrowed): no return value may depend on
it.

Two families of committed sequences.  The first walk (cases(), case_sequence()) draws the 27 kinds of BASE_KINDS; its draws are
pinned by tests/golden/seq_walk_digest.json, so everything below that the first walk reads -- draw(), make_op() without `graph`,
IDLE_WEIGHTS, BASE_READ_ROLES, Ctx.probe -- must keep drawing from the rng exactly as it does.  The graph walks (graph_cases(),
graph_case_sequence(), draw_graph()) add the three kinds of GRAPH_KINDS: the live unitigs as text (kh_unitigs_text_*: a UStream in
Ctx.unitigs["text"], its document from test_gpu_unitig_text.document() over unitig_ref / link_ref) and reads located on them
(kh_unitigs_locate*: test_locate_ref.locate_ref(); Ctx.unitigs["located"] says that the place map exists).  Both end with the
unitigs -- with everything ends() names, the next begin, and kh_unitigs_end, which does not enter the context and leaves the
kh_result_text_* stream alone.  What the header does not say is not asked: a REFUSED kh_unitigs_text_begin on a running stream."""
import hashlib
from collections import Counter

import numpy as np

import oracle_lib as O

U64 = np.uint64
OK, ERR_STATE, ERR_RANGE = 0, -7, -8
CTXS = ("A", "B", "D")

# ---- the committed walk: what tests/test_gpu_sequences.py runs and tests/test_seq_model.py checks the coverage of ----------------
STEPS = 100           # drawn calls per sequence (the audits every AUDIT_EVERY steps and at the end come on top)
AUDIT_EVERY = 10
GRAPH_AUDIT_EVERY = 40    # (an audit ends every session: the graph walks audit less often)
SEEDS = 8             # KMERHIP_SEQ_SEEDS raises it
# forms of A, B and D (tests/test_gpu_sequences.py builds them)
TRIPLES = [("image", "image", "image"), ("wide", "wide", "wide"), ("image", "wide", "regions3072"), ("grown", "image", "image"),
           ("wide-part", "wide-part", "wide-part"), ("borrow", "image", "wide")]


def k_of(forms):
    return 31 if "wide-part" in forms else 21


def cases(seeds=SEEDS):
    return [(seed, forms) for forms in TRIPLES for seed in range(seeds)]


# ---- which call enters which context how: include/kmerhip.h and the preset comments of ctx.hip.h, never a run -------------------
# role -> entry class; a role is the name of the op's argument that holds the context.  None: the call does not enter.
_ONE = lambda cls: {"ctx": cls}
ENTRY = {
    "push": _ONE("PUSH"), "push_text": _ONE("PUSH"), "reset": _ONE("PUSH"),          # touch no slot, count nothing
    "push_device": _ONE("PUSH_DEVICE"),                                               # as PUSH, what is pending counted first
    "merge_pairs": _ONE("WRITE"),
    "combine_into": {"a": "READ", "b": "READ", "dst": "WRITE"},                       # "a and b are only read ... dst is entered as a writer"
    "clip_tips_into": {"src": "READ_TAKE", "dst": "WRITE"},                          # src "as kh_unitigs_begin_linked enters it"
    "pop_bubbles_into": {"src": "READ_TAKE", "dst": "WRITE"},
    "finish": _ONE("READ"), "result_size": _ONE("READ"), "histogram": _ONE("READ"), "lookup": _ONE("READ"), "profile": _ONE("READ"),
    "compare": {"a": "READ", "b": "READ"},
    "graph_stats": _ONE("READ"), "graph_masks": _ONE("READ"),
    "result": _ONE("READ_TAKE"), "result_sorted": _ONE("READ_TAKE"),                  # "they take the same scratch memory"
    "audit": _ONE("READ_TAKE"),                                                       # result_sorted(1), then histogram(1)
    "text_begin": _ONE("READ"), "text_next": _ONE("TEXT_NEXT"),
    "unitigs_begin": _ONE("READ_TAKE"), "unitigs_begin_linked": _ONE("READ_TAKE"),    # "a kh_result_text_* stream in progress ends"
    "unitigs_copy": _ONE("READ"), "links_copy": _ONE("READ"),                         # "the link copies enter as readers"
    "unitigs_end": _ONE(None),
    "merge_across": _ONE("READ_TAKE"),
    # the live unitigs as text and the k-mers of reads located on them (the graph walks draw these three; the first walk never does)
    "unitigs_text_begin": _ONE("READ"),                                               # "begin enters as a reader"
    "unitigs_text_next": _ONE("TEXT_NEXT"),                                           # "a pull interface like kh_result_text_*"
    "unitigs_locate": _ONE("READ"),                                                   # "both enter as readers, like kh_profile*"
}
READER_CLASSES = ("READ", "TEXT_NEXT")                               # everything else ends the text stream and the unitigs
READING_CLASSES = ("READ", "READ_TAKE", "TEXT_NEXT")                 # what the header classes as reading: kh_stats stay what they were
FLUSHING_CLASSES = ("WRITE", "READ", "READ_TAKE", "PUSH_DEVICE")     # what is pending is counted first
KINDS = tuple(ENTRY)
GRAPH_KINDS = ("unitigs_text_begin", "unitigs_text_next", "unitigs_locate")   # drawn by the graph walks only
BASE_KINDS = tuple(kd for kd in KINDS if kd not in GRAPH_KINDS)
PUSHES = ("push", "push_device", "push_text")


def ends(cls):
    return cls is not None and cls not in READER_CLASSES


# what ends a stream / the unitigs of some context, as "kind" or "kind.role" where a call has several roles
def role_name(kind, role):
    return kind if len(ENTRY[kind]) == 1 else f"{kind}.{role}"


ENDING = tuple(role_name(kd, r) for kd in KINDS for r, cls in ENTRY[kd].items() if ends(cls))
READ_ROLES = tuple(role_name(kd, r) for kd in KINDS for r, cls in ENTRY[kd].items() if cls == "READ")
BASE_READ_ROLES = tuple(rn for rn in READ_ROLES if rn not in GRAPH_KINDS)        # what the first walk draws its readers from
# what ends the unitigs -- and with them their text stream and their place map -- of a context: the above (the two begins are among
# them) and kh_unitigs_end, which does not enter the context
UNITIG_ENDING = ENDING + ("unitigs_end",)


class Op:
    """One call: its kind and its arguments.  repr() is one line that eval() turns back into the Op (replay)."""

    def __init__(self, kind, **kw):
        assert kind in ENTRY, kind
        self.kind, self.kw = kind, kw

    def __getattr__(self, name):
        try:
            return self.__dict__["kw"][name]
        except KeyError:
            raise AttributeError(name)

    def __repr__(self):
        return "Op(%r%s)" % (self.kind, "".join(", %s=%r" % kv for kv in self.kw.items()))

    def __eq__(self, other):
        return isinstance(other, Op) and (self.kind, self.kw) == (other.kind, other.kw)

    def roles(self):
        """(role, context name, entry class) in the order the call enters them."""
        return [(r, self.kw[r], cls) for r, cls in ENTRY[self.kind].items()]


def parse(line):
    return eval(line, {"Op": Op, "__builtins__": {}})


# ---- the content pool --------------------------------------------------------------------------------------------------------------
POOL_SEED, GENOME, READ_LEN, CHUNK_READS, N_CHUNKS = 4242, 1 << 13, 150, 500, 4


class Pool:
    """Four chunks of 500 reads of 150 bases off one genome of 2^13 bases: the flat buffer, the same reads as FASTA text, and the
    oracle's (keys, counts), computed once per k."""

    def __init__(self, k):
        self.k = k
        self.reads, self.fasta, self.pairs = [], [], []
        for i in range(N_CHUNKS):
            b, _ = O.synth_reads(POOL_SEED, GENOME, READ_LEN, i * CHUNK_READS, CHUNK_READS, with_qual=False)
            b = np.asarray(b).copy()
            self.reads.append(b)
            rows = b.reshape(CHUNK_READS, READ_LEN + 1)
            assert (rows[:, READ_LEN] == ord("\n")).all()
            self.fasta.append(b"".join(b">r%d\n" % j + rows[j].tobytes() for j in range(CHUNK_READS)))
            self.pairs.append(oracle_pairs(b, k))

    def read(self, chunk, r):
        return self.reads[chunk][r * (READ_LEN + 1):(r + 1) * (READ_LEN + 1)]


def oracle_pairs(flat, k):
    m = O.OracleMap()
    m.process(flat, k)
    keys, counts = m.arrays()
    return np.asarray(keys, dtype=U64).copy(), np.asarray(counts, dtype=U64).copy()


_POOLS = {}


def pool(k):
    if k not in _POOLS:
        _POOLS[k] = Pool(k)
    return _POOLS[k]


def add_pairs(keys, counts, k2, c2):
    """count[key] += c over two sorted pair lists (uint64, wrapping like the device's add)."""
    if k2.size == 0:
        return keys, counts
    u, inv = np.unique(np.concatenate((keys, k2)), return_inverse=True)
    c = np.zeros(u.size, dtype=U64)
    np.add.at(c, inv, np.concatenate((counts, c2)))
    return u, c


def absent_keys(keys, k):
    """Three canonical keys the content does not hold (fixed candidates, the first three that are absent)."""
    rng = np.random.default_rng(99)
    out = []
    while len(out) < 3:
        s = bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8))
        x = O.canonical(s)[0]
        if not np.isin(U64(x), keys):
            out.append(x)
    return np.array(out, dtype=U64)


# ---- references, computed once per content -----------------------------------------------------------------------------------------
_REFS = {}


def content_hash(keys, counts):
    return hashlib.sha1(keys.tobytes() + b"|" + counts.tobytes()).hexdigest()


def cached(kind, keys, counts, extra, make):
    key = (kind, content_hash(keys, counts)) + tuple(extra)
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def unitig_ref(keys, counts, k, mc):
    import test_gpu_unitigs as U
    return cached("unitigs", keys, counts, (k, max(mc, 1)), lambda: U.Ref(U.node_dict(keys, counts, k, mc), k))


def link_ref(keys, counts, k, mc):
    import test_gpu_unitig_links as LR
    return cached("links", keys, counts, (k, max(mc, 1)), lambda: LR.LinkRef(unitig_ref(keys, counts, k, mc)))


def clip_ref(keys, counts, k, mc, max_kmers):
    import test_clip_ref as CR
    return cached("clip", keys, counts, (k, max(mc, 1), max_kmers),
                  lambda: CR.ClipRef(unitig_ref(keys, counts, k, mc), link_ref(keys, counts, k, mc), max_kmers))


def pop_ref(keys, counts, k, mc, max_kmers):
    import test_pop_ref as PR
    return cached("pop", keys, counts, (k, max(mc, 1), max_kmers),
                  lambda: PR.PopRef(unitig_ref(keys, counts, k, mc), link_ref(keys, counts, k, mc), max_kmers))


def selected(keys, counts, mc):
    sel = counts >= U64(max(mc, 1))
    return keys[sel], counts[sel]


def record_lens(fmt, k, counts):
    """Bytes of every record (test_gpu_format.record), from the digits of its count."""
    import test_gpu_format as F
    base = len(F.record(fmt, "A" * k, 1)) - 1
    digits = np.ones(counts.size, dtype=np.int64)
    c = counts.copy()
    while True:
        c = c // U64(10)
        more = c > 0
        if not more.any():
            break
        digits += more
    return base + digits


def sorted_doc(fmt, k, keys, counts):
    """The whole document of a sorted stream: record() over the pairs in ascending key order, and the JSON tail."""
    import test_gpu_format as F
    import test_gpu_unitigs as U

    def make():
        if keys.size == 0:
            return F.empty_doc(fmt)
        names = U.unpack(keys, k)
        body = b"".join(F.record(fmt, names[i].decode(), int(counts[i]), first=(i == 0)) for i in range(keys.size))
        return body + (b"\n]\n" if fmt == "json" else b"")
    return cached("doc", keys, counts, (fmt, k), make)


class Stream:
    """A text stream: what kh_result_text_begin sized and how far the pieces have come."""

    def __init__(self, fmt, mc, is_sorted, k, keys, counts):
        self.fmt, self.mc, self.sorted, self.k = fmt, mc, is_sorted, k
        self.keys, self.counts = selected(keys, counts, mc)
        self.lens = record_lens(fmt, k, self.counts)
        self.cum = np.concatenate(([0], np.cumsum(self.lens)))
        self.rec_total = int(self.cum[-1])
        self.tail = 3 if fmt == "json" else 0                  # "\n]\n", or the whole of "[]\n"
        self.n_records, self.n_bytes = int(self.keys.size), self.rec_total + self.tail
        self.pos = 0                                            # bytes handed out
        self.ended = False                                      # a call has returned 0 bytes
        self.counted = False                                    # (coverage() has counted its end)
        self.pieces = []

    def outstanding(self):
        return self.n_bytes - self.pos

    def expect(self, cap):
        """(status, bytes) of the next call with room for cap bytes: as many whole records as fit, the JSON tail behind the last one
        when it fits too.  An unsorted stream's records come in table-slot order: the byte count is exact only where no record is cut
        off (the generator draws caps below every record or above a few), the status always."""
        if self.pos < self.rec_total:
            i = int(np.searchsorted(self.cum, self.pos, side="right")) - 1      # the record at pos (sorted order)
            nxt = int(self.lens[i]) if self.sorted else int(self.lens.min())
            if cap < nxt:
                return ERR_RANGE, 0
            assert self.sorted or cap >= int(self.lens.max()), "a cap between two record lengths of an unsorted stream"
            j = int(np.searchsorted(self.cum, self.pos + cap, side="right")) - 1
            n = int(self.cum[j]) - self.pos
            if j == self.lens.size and self.tail and n + self.tail <= cap:
                n += self.tail
            return OK, n
        left = self.n_bytes - self.pos                           # the tail alone, or nothing
        if left and cap < left:
            return ERR_RANGE, 0
        return OK, left

    def advance(self, n, piece=None, cap=None):
        """A call handed out n bytes (piece: those bytes, where there is a device).  Checks all the header promises of a piece."""
        import test_gpu_format as F
        assert self.pos + n <= self.n_bytes, (self.pos, n, self.n_bytes)
        if n == 0:
            assert self.pos == self.n_bytes, f"the stream ended after {self.pos} of {self.n_bytes} bytes"
            if piece is not None and not self.ended and not self.sorted:         # an unsorted stream: the records as a multiset
                import test_gpu_unitigs as U
                names = U.unpack(self.keys, self.k)
                d = {names[i].decode(): int(self.counts[i]) for i in range(self.keys.size)}
                got = F.split_records(self.fmt, b"".join(self.pieces))
                assert sorted(got) == F.expected_records(self.fmt, d), "an unsorted stream's records are not the table's"
            self.ended = True
            return
        if piece is not None:
            assert len(piece) == n and (cap is None or n <= cap)
            last = self.pos + n == self.n_bytes
            assert F.ends_at_record_end(self.fmt, piece, last), (self.fmt, piece[-40:], last)
            if self.sorted:
                doc = sorted_doc(self.fmt, self.k, self.keys, self.counts)
                assert len(doc) == self.n_bytes
                assert piece == doc[self.pos:self.pos + n], f"a sorted stream's piece at byte {self.pos} is not the document's"
            self.pieces.append(piece)
        self.pos += n


def unitig_doc(fmt, k, keys, counts, mc):
    """(document, middles) of the unitig text of the node set: test_gpu_unitig_text.document() over unitig_ref / link_ref, and the
    offset of the middle byte of every unitig's sequence in it (where the generator lets a piece end)."""
    import test_gpu_unitig_text as UT

    def make():
        r = unitig_ref(keys, counts, k, mc)
        links = link_ref(keys, counts, k, mc).links if fmt == "gfa" else []
        layout = []
        doc = UT.document(fmt, r.rows, np.frombuffer(r.bases, dtype=np.uint8), links, k, layout)
        mids = [e[1] + len(e[2]) + len(e[3]) // 2 for e in layout if e[0] == "S"]
        return doc, np.array(mids, dtype=np.int64)
    return cached("udoc", keys, counts, (fmt, k, max(mc, 1)), make)


class UStream:
    """A kh_unitigs_text_* stream: the document kh_unitigs_text_begin sized and how far the pieces have come.  A piece is a byte
    range: the count and the bytes of every piece are exact."""

    def __init__(self, fmt, doc, mids):
        self.fmt, self.doc, self.mids = fmt, doc, mids
        self.n_bytes = len(doc)
        self.pos = 0
        self.ended = False                                      # a call has returned 0 bytes
        self.counted = False                                    # (coverage() has counted its end)

    def outstanding(self):
        return self.n_bytes - self.pos

    def expect(self, cap):
        left = self.outstanding()
        if left and cap == 0:
            return ERR_RANGE, 0                                 # "cap = 0 while bytes are left ... consumes nothing"
        return OK, min(cap, left)

    def advance(self, n, piece=None):
        assert self.pos + n <= self.n_bytes, (self.pos, n, self.n_bytes)
        if piece is not None:
            assert len(piece) == n
            if piece != self.doc[self.pos:self.pos + n]:
                at = next(i for i in range(n) if piece[i] != self.doc[self.pos + i])
                raise AssertionError(f"a {self.fmt} piece at byte {self.pos} differs from the document at byte {self.pos + at}: "
                                     f"{piece[max(at - 20, 0):at + 20]!r} for {self.doc[max(self.pos + at - 20, 0):self.pos + at + 20]!r}")
        if n == 0:
            assert self.pos == self.n_bytes
            self.ended = True
        self.pos += n

    def mid_cap(self, rng):
        """A cap whose piece ends in the middle of a sequence: that of the first unitig whose middle lies 1500 to 4000 bytes on, or of
        the last one there is (None: no sequence is left to end in)."""
        i = int(np.searchsorted(self.mids, self.pos + int(rng.integers(1500, 4000))))
        i = min(i, self.mids.size - 1)
        return int(self.mids[i]) - self.pos if i >= 0 and int(self.mids[i]) > self.pos else None


class Ctx:
    def __init__(self, keys, counts):
        self.keys, self.counts = keys, counts
        self.pending = False             # something pushed and not yet counted
        self.stream = None
        self.unitigs = None              # None, or {"mc":, "linked":, "text": None or a UStream, "located": a locate call has succeeded}
        self.gprobe = ()                 # as probe below with the three graph kinds; kh_unitigs_end sets it too (the graph walks read it)
        self.empty_since_reset = False
        self.after_reset = False         # kh_reset was the last call that entered this context
        self.last = None                 # the kind of that call
        self.last_op = None              # ... and the call
        self.probe = ()                  # what that call ended: the calls that must now be refused

    def total(self):
        return int(np.sum(self.counts, dtype=U64))


class Expect:
    def __init__(self, status=OK, **values):
        self.status, self.values = status, values

    def __getitem__(self, name):
        return self.values[name]


class Model:
    """Three contexts of one k, each holding chunk 0 counted at the start."""

    def __init__(self, k):
        self.k, self.pool = k, pool(k)
        self.drawn = Counter()           # (the generator's: what a graph walk has drawn how often, to draw the roles evenly)
        self.ctx = {name: Ctx(*self.pool.pairs[0]) for name in CTXS}

    # -- entering --------------------------------------------------------------------------------------------------------------------
    def enter(self, c, cls):
        if cls is None:
            return
        c.probe = c.gprobe = ()
        if ends(cls):
            c.probe = (("text_next",) if c.stream is not None else ()) + \
                (("unitigs_copy", "links_copy") if c.unitigs is not None else ())
            c.gprobe = c.probe + self.graph_probe(c)
            c.stream = None
            c.unitigs = None
        if cls in FLUSHING_CLASSES:
            c.pending = False

    @staticmethod
    def graph_probe(c):
        """What ending the unitigs of c adds to the calls that must now be refused."""
        if c.unitigs is None:
            return ()
        return (("unitigs_text_next",) if c.unitigs["text"] is not None else ()) + ("unitigs_locate",)

    def apply(self, op, refs=True):
        """The status and the values op must return, and its effect on the model.  refs=False: the effect alone (the generator and
        the coverage walk: no reference that costs time is computed)."""
        for _, name, cls in op.roles():
            self.enter(self.ctx[name], cls)
        exp = getattr(self, "_" + op.kind)(op, refs)
        for _, name, cls in op.roles():
            if cls is not None:
                self.ctx[name].after_reset = op.kind == "reset"
                self.ctx[name].last = op.kind
                self.ctx[name].last_op = op
        return exp

    def add(self, c, keys, counts):
        c.keys, c.counts = add_pairs(c.keys, c.counts, keys, counts)
        if keys.size:
            c.empty_since_reset = False

    # -- content ---------------------------------------------------------------------------------------------------------------------
    def _push(self, op, refs):
        c = self.ctx[op.ctx]
        self.add(c, *self.pool.pairs[op.chunk])
        c.pending = True
        return Expect()

    _push_device = _push_text = _push

    def _reset(self, op, refs):
        c = self.ctx[op.ctx]
        c.keys, c.counts = np.empty(0, dtype=U64), np.empty(0, dtype=U64)
        c.pending, c.empty_since_reset = False, True
        return Expect()

    def _merge_pairs(self, op, refs):
        self.add(self.ctx[op.ctx], *self.pool.pairs[op.chunk])
        return Expect()

    def combined(self, op):
        import test_gpu_join as T
        a, b = self.ctx[op.a], self.ctx[op.b]
        u, ca, cb = T.align(a.keys, a.counts, b.keys, b.counts)
        return T.np_combine(u, ca, cb, op.op, op.calc)

    def _combine_into(self, op, refs):
        ek, ec = self.combined(op)
        self.add(self.ctx[op.dst], ek, ec)
        return Expect(n_pairs=int(ek.size))

    def _clip_tips_into(self, op, refs, make=clip_ref, bound=1):
        s = self.ctx[op.src]
        r = make(s.keys, s.counts, self.k, op.mc, bound * self.k)       # (the binding's default bounds: k, and 2 k for bubbles)
        self.add(self.ctx[op.dst], r.keys, r.counts)
        return Expect(words=[int(w) for w in r.words])

    def _pop_bubbles_into(self, op, refs):
        return self._clip_tips_into(op, refs, make=pop_ref, bound=2)

    def _merge_across(self, op, refs):
        c = self.ctx[op.ctx]        # one rank: the shard of one is the whole table, the content stays, nothing is refused afterwards
        return Expect(owned_distinct=int(c.keys.size), conserved=1, merged_count_sum=c.total())

    # -- reading ---------------------------------------------------------------------------------------------------------------------
    def _finish(self, op, refs):
        c = self.ctx[op.ctx]
        return Expect(kmers=c.total(), distinct=int(c.keys.size))

    def _result_size(self, op, refs):
        c = self.ctx[op.ctx]
        return Expect(n=int((c.counts >= U64(max(op.mc, 1))).sum()))

    def _result(self, op, refs):
        c = self.ctx[op.ctx]
        k, v = selected(c.keys, c.counts, op.mc)
        return Expect(keys=k, counts=v)

    _result_sorted = _result

    def _audit(self, op, refs):
        c = self.ctx[op.ctx]
        v, f = np.unique(c.counts, return_counts=True)
        return Expect(keys=c.keys, counts=c.counts, histogram=list(zip(v.tolist(), f.tolist())))

    def _histogram(self, op, refs):
        c = self.ctx[op.ctx]
        v, f = np.unique(selected(c.keys, c.counts, op.mc)[1], return_counts=True)
        return Expect(histogram=list(zip(v.tolist(), f.tolist())))

    def sample(self, c, pick, n=64):
        rng = np.random.default_rng(pick)
        some = c.keys[rng.integers(0, c.keys.size, size=n)] if c.keys.size else np.empty(0, dtype=U64)
        return np.concatenate((some, absent_keys(c.keys, self.k)))

    def _lookup(self, op, refs):
        c = self.ctx[op.ctx]
        q = self.sample(c, op.pick)
        want = np.zeros(q.size, dtype=U64)
        if c.keys.size:
            i = np.minimum(np.searchsorted(c.keys, q), c.keys.size - 1)
            want = np.where(c.keys[i] == q, c.counts[i], U64(0))
        assert (want[-3:] == 0).all()
        return Expect(query=q, counts=want)

    def flat(self, op):
        """The bytes of a profile or locate op: the read `read` of the chunk, or `reads` consecutive reads from there on (the graph
        walks: more than one chunk of the host forms)."""
        n = op.kw.get("reads", 1)
        return self.pool.reads[op.chunk][op.read * (READ_LEN + 1):(op.read + n) * (READ_LEN + 1)]

    def _profile(self, op, refs):
        import profile_expect as PE
        c = self.ctx[op.ctx]
        flat = self.flat(op)
        return Expect(bases=flat, profile=PE.np_profile(flat, self.k, c.keys, c.counts) if refs else None)

    def _compare(self, op, refs):
        import test_gpu_join as T
        a, b = self.ctx[op.a], self.ctx[op.b]
        _, ca, cb = T.align(a.keys, a.counts, b.keys, b.counts)
        return Expect(words=T.np_words(ca, cb))

    def _graph_stats(self, op, refs):
        import test_gpu_graph as G
        c = self.ctx[op.ctx]
        return Expect(words=G.np_words(c.keys, c.counts, op.mc, self.k) if refs else None)

    def _graph_masks(self, op, refs):
        import test_gpu_graph as G
        c = self.ctx[op.ctx]
        q = self.sample(c, op.pick)
        return Expect(query=q, masks=G.np_masks(q, G.node_set(c.keys, c.counts, op.mc)[0], self.k) if refs else None)

    # -- the text stream -------------------------------------------------------------------------------------------------------------
    def _text_begin(self, op, refs):
        c = self.ctx[op.ctx]
        c.stream = Stream(op.fmt, op.mc, op.sorted, self.k, c.keys, c.counts)
        return Expect(n_records=c.stream.n_records, n_bytes=c.stream.n_bytes)

    def _text_next(self, op, refs):
        s = self.ctx[op.ctx].stream
        if s is None:
            return Expect(ERR_STATE)
        status, n = s.expect(op.cap)
        return Expect(status, n=n)

    def text_piece(self, name, n, piece=None, cap=None):
        """What a text_next that returned KH_OK handed out: the stream moves on by it (the coverage walk passes the expected n)."""
        self.ctx[name].stream.advance(n, piece, cap)

    # -- unitigs ---------------------------------------------------------------------------------------------------------------------
    def _unitigs_begin(self, op, refs, linked=False):
        c = self.ctx[op.ctx]
        c.unitigs = {"mc": op.mc, "linked": linked, "text": None, "located": False}
        if not refs:
            return Expect()
        r = unitig_ref(c.keys, c.counts, self.k, op.mc)
        exp = Expect(n_unitigs=int(r.rows.shape[0]), n_bases=len(r.bases))
        if linked:
            exp.values["n_links"] = int(link_ref(c.keys, c.counts, self.k, op.mc).links.size)
        return exp

    def _unitigs_begin_linked(self, op, refs):
        return self._unitigs_begin(op, refs, linked=True)

    def _unitigs_copy(self, op, refs):
        c = self.ctx[op.ctx]
        if c.unitigs is None:
            return Expect(ERR_STATE)                      # "a copy without a live begin ... is KH_ERR_STATE"
        if not refs:
            return Expect()
        r = unitig_ref(c.keys, c.counts, self.k, c.unitigs["mc"])
        return Expect(rows=r.rows, bases=r.bases)

    def _links_copy(self, op, refs):
        c = self.ctx[op.ctx]
        if c.unitigs is None or not c.unitigs["linked"]:
            return Expect(ERR_STATE)                      # "stale or not begun ... and so is a copy after a plain kh_unitigs_begin"
        if not refs:
            return Expect()
        return Expect(links=link_ref(c.keys, c.counts, self.k, c.unitigs["mc"]).links)

    def _unitigs_end(self, op, refs):
        c = self.ctx[op.ctx]             # (it does not enter: the kh_result_text_* stream, what is pending and `probe` stay)
        if c.unitigs is not None:
            c.gprobe = ("unitigs_copy",) + self.graph_probe(c)
        c.unitigs = None
        return Expect()

    # -- the unitigs as text, and reads located on them -----------------------------------------------------------------------------
    def _unitigs_text_begin(self, op, refs):
        """The document is computed even with refs=False: the generator and the coverage walk need its length."""
        u = self.ctx[op.ctx].unitigs
        if u is None or (op.fmt == "gfa" and not u["linked"]):
            # (the header does not say what a REFUSED begin does to a running stream: the generator never asks)
            assert u is None or u["text"] is None, "a refused kh_unitigs_text_begin on a running stream: nothing says what becomes of it"
            return Expect(ERR_STATE)
        c = self.ctx[op.ctx]
        u["text"] = UStream(op.fmt, *unitig_doc(op.fmt, self.k, c.keys, c.counts, u["mc"]))     # (a running stream restarts)
        return Expect(n_bytes=u["text"].n_bytes)

    def _unitigs_text_next(self, op, refs):
        u = self.ctx[op.ctx].unitigs
        if u is None or u["text"] is None:
            return Expect(ERR_STATE)
        status, n = u["text"].expect(op.cap)
        return Expect(status, n=n)

    def unitig_text_piece(self, name, n, piece=None):
        """What a unitigs_text_next that returned KH_OK handed out: n is the model's own, piece the device's bytes."""
        self.ctx[name].unitigs["text"].advance(n, piece)

    def _unitigs_locate(self, op, refs):
        c = self.ctx[op.ctx]
        if c.unitigs is None:
            return Expect(ERR_STATE)
        c.unitigs["located"] = True
        flat = self.flat(op)
        if not refs:
            return Expect(bases=flat)
        import test_locate_ref as LO
        mc = c.unitigs["mc"]
        r = unitig_ref(c.keys, c.counts, self.k, mc)
        places = cached("places", c.keys, c.counts, (self.k, max(mc, 1)), lambda: LO.place_dict(r.rows, r.bases, self.k))
        links = link_ref(c.keys, c.counts, self.k, mc).links if c.unitigs["linked"] else None
        return Expect(bases=flat, words=LO.locate_ref(r.rows, r.bases, self.k, flat, places=places), rows=r.rows, links=links)


# ---- the generator -----------------------------------------------------------------------------------------------------------------
FORMATS = ("fasta", "tsv", "json")
READERS = ("finish", "result_size", "histogram", "lookup", "profile", "compare", "graph_stats", "graph_masks")
# what is drawn while nothing is in progress on the chosen context
IDLE_WEIGHTS = {
    "push": 1.5, "push_device": 1.5, "push_text": 1.5, "reset": 1.5, "merge_pairs": 1.5, "combine_into": 2.0, "clip_tips_into": 1.2,
    "pop_bubbles_into": 1.2, "result": 0.8, "result_sorted": 0.8, "text_begin": 7.0, "text_next": 0.5, "unitigs_begin": 2.2,
    "unitigs_begin_linked": 2.2, "unitigs_copy": 0.4, "links_copy": 0.4, "unitigs_end": 0.4, **{r: 0.5 for r in READERS},
}
ENDERS = tuple(rn for rn in ENDING if rn != "audit")
GROWTH_LIMIT = 1 << 40        # no count is let past this: a combine that could is drawn again as a reset of its target


def draw_mc(rng, c, high=0.5):
    """A threshold: 0, 1, 2, or -- with probability `high` -- one that leaves about a tenth of the keys (a stream of it ends within
    a call or two)."""
    top = int(np.quantile(c.counts, 0.9)) + 1 if c.counts.size else 3
    rest = (1.0 - high) / 0.5
    return int(rng.choice([0, 1, 2, top], p=[0.1 * rest, 0.25 * rest, 0.15 * rest, high]))


def busy(c):
    return (c.stream is not None and not c.stream.ended) or c.unitigs is not None


def make_op(rng, m, name, rn, graph=False):
    """The call rn = "kind" or "kind.role" with the context `name` in that role, its other arguments drawn.  graph: for a graph walk
    (its thresholds and its profile calls are drawn differently; the first walk's draws stay what they were)."""
    kind, _, role = rn.partition(".")
    c = m.ctx[name]
    others = [x for x in CTXS if x != name]
    pick = lambda: int(rng.integers(0, 1 << 30))
    if kind in PUSHES or kind == "merge_pairs":
        return Op(kind, ctx=name, chunk=int(rng.integers(0, N_CHUNKS)))
    if kind == "combine_into":          # (a == b is allowed)
        import test_gpu_join as T
        op, calc = T.CASES[int(rng.integers(0, len(T.CASES)))]
        if role == "dst":
            dst = name
            a, b = (str(x) for x in rng.choice(others, size=2))
        else:
            dst = str(rng.choice(others))
            a, b = name, str(rng.choice([x for x in CTXS if x != dst]))
            if role == "b":
                a, b = b, a
        peak = lambda x: int(m.ctx[x].counts.max()) if m.ctx[x].counts.size else 0
        if peak(dst) + peak(a) + peak(b) >= GROWTH_LIMIT:
            return Op("reset", ctx=dst)
        return Op(kind, dst=dst, a=a, b=b, op=op, calc=calc)
    if kind in ("clip_tips_into", "pop_bubbles_into"):
        dst, src = (name, str(rng.choice(others))) if role == "dst" else (str(rng.choice(others)), name)
        return Op(kind, dst=dst, src=src, mc=draw_mc(rng, m.ctx[src], high=0.7))
    if graph and kind in ("unitigs_begin", "unitigs_begin_linked"):
        return Op(kind, ctx=name, mc=draw_graph_mc(rng, c))
    if kind in ("result_size", "result", "result_sorted", "histogram", "graph_stats", "unitigs_begin", "unitigs_begin_linked"):
        return Op(kind, ctx=name, mc=draw_mc(rng, c))
    if kind == "lookup":
        return Op(kind, ctx=name, pick=pick())
    if kind == "graph_masks":
        return Op(kind, ctx=name, mc=draw_mc(rng, c), pick=pick())
    if kind in ("profile", "unitigs_locate") and graph:
        # the host forms: one read, or 8 or 16 of them -- 1208 and 2416 bytes, two and three chunks of 1024 window starts
        device = kind == "unitigs_locate" and bool(rng.random() < 0.5)
        reads = 1 if device else int(rng.choice([1, 8, 16], p=[0.4, 0.3, 0.3]))
        kw = dict(ctx=name, chunk=int(rng.integers(0, N_CHUNKS)), read=int(rng.integers(0, CHUNK_READS - reads + 1)))
        if reads > 1:
            kw["reads"] = reads
        return Op(kind, **kw, device=device) if kind == "unitigs_locate" else Op(kind, **kw)
    if kind == "unitigs_text_begin":        # gfa behind a plain begin is refused: asked only where no stream is running
        u = c.unitigs
        if u is None or u["linked"]:
            fmt = str(rng.choice(UNITIG_FORMATS, p=[0.4, 0.6]))
        else:
            fmt = "gfa" if u["text"] is None and rng.random() < 0.25 else "fasta"
        return Op(kind, ctx=name, fmt=fmt)
    if kind == "unitigs_text_next":         # 0; less than a header line; one that ends in the middle of a sequence; 64 KiB
        t = c.unitigs["text"] if c.unitigs is not None else None
        mid = t.mid_cap(rng) if t is not None and t.outstanding() else None
        cap = int(rng.choice([0, 7, mid or 2999, 64 << 10], p=[0.07, 0.1, 0.58, 0.25]))
        return Op(kind, ctx=name, cap=cap, device=bool(rng.random() < 0.4))
    if kind == "profile":
        return Op(kind, ctx=name, chunk=int(rng.integers(0, N_CHUNKS)), read=int(rng.integers(0, CHUNK_READS)))
    if kind == "compare":
        other = str(rng.choice(CTXS))
        return Op(kind, a=name, b=other) if role == "a" else Op(kind, a=other, b=name)
    if kind == "text_begin":
        return Op(kind, ctx=name, fmt=str(rng.choice(FORMATS)), mc=draw_mc(rng, c, high=0.6), sorted=bool(rng.random() < 0.5))
    if kind == "text_next":             # below any record; a few records; 64 KiB
        few = 4 * (m.k + 64)
        return Op(kind, ctx=name, cap=int(rng.choice([8, few, 64 << 10], p=[0.12, 0.18, 0.7])))
    return Op(kind, ctx=name)           # finish, unitigs_copy, links_copy, unitigs_end, merge_across


def draw(rng, m, borrow):
    ended = [n for n in CTXS if m.ctx[n].probe]
    if ended and rng.random() < 0.5:            # something was just ended: the call that must now be refused
        name = str(rng.choice(ended))
        return make_op(rng, m, name, str(rng.choice(m.ctx[name].probe)))
    names = [n for n in CTXS if busy(m.ctx[n])]
    name = str(rng.choice(names)) if names and rng.random() < 0.85 else str(rng.choice(CTXS))   # (stay with what is in progress)
    c = m.ctx[name]
    live_stream = c.stream is not None and not c.stream.ended
    u = rng.random()
    if live_stream or c.unitigs is not None:
        # in progress: its own next call, a reader between (every ENTER_READ role alike), or something that ends it (every role alike)
        if live_stream and c.unitigs is not None:       # both: a piece, a copy of the unitigs, a piece
            if c.last == "text_next" and u < 0.6:
                return make_op(rng, m, name, "links_copy" if c.unitigs["linked"] and rng.random() < 0.5 else "unitigs_copy")
            if c.last in ("unitigs_copy", "links_copy") and u < 0.7:
                return make_op(rng, m, name, "text_next")
        own = 0.25 if c.last in ("text_next", "text_begin", "unitigs_begin", "unitigs_begin_linked", "unitigs_copy") else 0.62
        if u < own:                     # (next, reader, next: a reader is likely behind its own call, its own call behind a reader)
            if live_stream and (c.unitigs is None or rng.random() < 0.6):
                return make_op(rng, m, name, "text_next")
            return make_op(rng, m, name, str(rng.choice(["unitigs_copy", "links_copy", "unitigs_end"],
                                                        p=[0.45, 0.45, 0.1] if c.unitigs["linked"] else [0.75, 0.15, 0.1])))
        if c.unitigs is not None and not live_stream and rng.random() < 0.2:   # (a stream beside live unitigs: their copies between its pieces)
            return make_op(rng, m, name, "text_begin")
        if u < 0.80:
            roles = [rn for rn in BASE_READ_ROLES if not (live_stream and rn == "text_begin")]
            return make_op(rng, m, name, str(rng.choice(roles)))
        if name in borrow and rng.random() < 0.6:
            return make_op(rng, m, name, "merge_across")
        return make_op(rng, m, name, str(rng.choice([rn for rn in ENDERS if rn != "merge_across"])))
    w = dict(IDLE_WEIGHTS)
    if c.stream is not None:                    # it has ended: once more, or on to something else
        w["text_next"] = 1.5
    if name in borrow:
        w["merge_across"] = 3.0
    if c.after_reset:                           # what comes first after a reset
        for kd in ("merge_pairs", "combine_into", "clip_tips_into", "pop_bubbles_into") + PUSHES:
            w[kd] *= 2.5
        w["clip_tips_into"] = w["pop_bubbles_into"] = w["merge_pairs"] = 6.0
        w["text_begin"] = w["unitigs_begin"] = w["unitigs_begin_linked"] = 0.5
    if c.pending:                               # a reader first after a push
        for r in READERS:
            w[r] *= 4.0
    kinds = list(w)
    p = np.array([w[kd] for kd in kinds])
    kind = str(rng.choice(kinds, p=p / p.sum()))
    roles = list(ENTRY[kind])
    role = "dst" if c.after_reset and "dst" in roles and rng.random() < 0.8 else str(rng.choice(roles))
    return make_op(rng, m, name, role_name(kind, role))


# ---- the graph walks: sessions on live unitigs -------------------------------------------------------------------------------------
UNITIG_FORMATS = ("fasta", "gfa")
GRAPH_STEPS = 120
GRAPH_SEEDS = 5          # KMERHIP_SEQ_SEEDS raises it
UT_CHUNK = 8 << 10       # the device test runs them with KMERHIP_UNI_TEXT_CHUNK_KB=8 (one tile per chunk of a unitig text stream) ...
PF_CHUNK = 1 << 10       # ... and KMERHIP_PROFILE_CHUNK_KB=1 (window starts per chunk of kh_profile and kh_unitigs_locate)
GRAPH_ENV = {"KMERHIP_UNI_TEXT_CHUNK_KB": str(UT_CHUNK >> 10), "KMERHIP_PROFILE_CHUNK_KB": str(PF_CHUNK >> 10)}
# what is drawn on a context without live unitigs: mostly a begin; a little of everything that changes the content; the new calls, refused
GRAPH_IDLE_WEIGHTS = {
    "unitigs_begin": 3.0, "unitigs_begin_linked": 4.5, "push": 0.5, "push_device": 0.5, "push_text": 0.5, "reset": 0.9, "merge_pairs": 0.6,
    "combine_into": 0.6, "clip_tips_into": 0.5, "pop_bubbles_into": 0.5, "text_begin": 0.8, "text_next": 0.3, "unitigs_text_begin": 0.5,
    "unitigs_text_next": 0.4, "unitigs_locate": 0.6, "unitigs_copy": 0.2, "unitigs_end": 0.2, "profile": 0.3, "finish": 0.3,
}


def draw_graph_mc(rng, c, other_than=None):
    """A threshold for a begin: 0, 1 and 2 (long documents) more often than draw_mc has them, the one that leaves a tenth of the keys,
    and one above every count (an empty S).  other_than: a threshold whose node set the new one must not repeat."""
    top = int(np.quantile(c.counts, 0.9)) + 1 if c.counts.size else 3
    above = int(c.counts.max()) + 1 if c.counts.size else 5
    cand, p = [0, 1, 2, top, above], [0.15, 0.35, 0.2, 0.25, 0.05]
    if other_than is not None:
        keep = [i for i, x in enumerate(cand) if max(x, 1) != max(other_than, 1)]
        cand, p = [cand[i] for i in keep], [p[i] for i in keep]
    p = np.array(p)
    return int(rng.choice(cand, p=p / p.sum()))


def draw_graph(rng, m, borrow):
    """One call of a graph walk.  Where unitigs are live: the next piece of their text, a locate call, a copy, a reader between (every
    ENTER_READ role alike), a piece of a kh_result_text_* stream beside it, a restart, a second begin with another threshold, or
    something that ends them (every ending role alike); behind everything that ended something the probe, with probability 1/2."""
    go = lambda name, rn: make_op(rng, m, name, rn, graph=True)

    def evenly(what, names):        # one of `names`, among those this walk has drawn least often as a `what`
        least = min(m.drawn[what, x] for x in names)
        x = str(rng.choice([x for x in names if m.drawn[what, x] == least]))
        m.drawn[what, x] += 1
        return x

    ended = [n for n in CTXS if m.ctx[n].gprobe]
    if ended and rng.random() < 0.5:
        name = str(rng.choice(ended))
        return go(name, str(rng.choice(m.ctx[name].gprobe)))
    live = [n for n in CTXS if m.ctx[n].unitigs is not None]
    name = str(rng.choice(live)) if live and rng.random() < 0.85 else str(rng.choice(CTXS))
    c = m.ctx[name]
    u = c.unitigs
    if u is None:
        w = dict(GRAPH_IDLE_WEIGHTS)
        if name in borrow:
            w["merge_across"] = 1.0
        if c.keys.size == 0:                    # behind a reset: a begin on the empty table, or something to fill it
            w["merge_pairs"] = w["push"] = 1.5
        kinds = list(w)
        p = np.array([w[kd] for kd in kinds])
        kind = str(rng.choice(kinds, p=p / p.sum()))
        return go(name, role_name(kind, str(rng.choice(list(ENTRY[kind])))))
    t, s = u["text"], c.stream
    running = t is not None and t.outstanding() > 0
    beside = s is not None and not s.ended
    host_locate = c.last == "unitigs_locate" and not c.last_op.device
    if c.last == "profile" and rng.random() < 0.35:      # the two host forms that share the chunk buffers, next to each other
        op = go(name, "unitigs_locate")
        return Op("unitigs_locate", **{**op.kw, "device": False})
    if host_locate and rng.random() < 0.15:
        return go(name, "profile")
    w = {"utext_next": 7.0 if running else 3.0 if t is not None else 0.3,      # (at the end: once more; no stream: refused)
         "utext_begin": 0.5 if running else 2.0,                               # (on a running stream: a restart)
         "locate": 1.5, "profile": 0.4, "copy": 0.8, "reader": 3.0,
         "beside_next": 2.0 if beside else 0.2, "beside_begin": 0.3 if beside else 1.0,
         "rebegin": 0.4, "end": 0.3, "ender": 2.2 if running else 1.0 if u["located"] else 0.4}    # (mostly where it cuts a stream short or releases a place map)
    if name in borrow:                                  # (one context of one triple: its own weight, or too few walks get there)
        w["merge_across"] = 6.0 if running and u["located"] else 3.0 if running or u["located"] else 0.5
    is_reader = c.last not in GRAPH_KINDS and (ENTRY[c.last].get("ctx") == "READ" or len(ENTRY[c.last]) > 1)
    if running:                                         # piece, reader, piece: a reader is likely behind a piece, a piece behind a reader
        if t.pos == 0:
            w["utext_next"] = 14.0                      # (the first piece first: only behind it does a reader lie between two)
        elif c.last == "unitigs_text_next":
            w["utext_next"], w["reader"] = 3.5, 7.0
        elif is_reader:
            w["utext_next"] = 40.0
    if running and beside:                              # the two streams' pieces in turns
        if c.last == "unitigs_text_next":
            w["beside_next"] = 6.0
        elif c.last == "text_next":
            w["utext_next"], w["beside_next"] = 12.0, 4.0
    if not running and u["located"]:                    # locate, reader, locate
        if c.last == "unitigs_locate":
            w["reader"] = 6.0
        elif is_reader:
            w["locate"] = 20.0
    what = list(w)
    p = np.array([w[x] for x in what])
    pick = str(rng.choice(what, p=p / p.sum()))
    if pick == "utext_next":
        return go(name, "unitigs_text_next")
    if pick == "utext_begin":
        return go(name, "unitigs_text_begin")
    if pick == "locate":
        return go(name, "unitigs_locate")
    if pick == "profile":
        return go(name, "profile")
    if pick == "copy":
        return go(name, "links_copy" if rng.random() < (0.5 if u["linked"] else 0.15) else "unitigs_copy")
    if pick == "reader":
        roles = [rn for rn in READ_ROLES if u["linked"] or rn != "links_copy"]        # (no reader where it is refused)
        return go(name, evenly("reader between pieces" if running and t.pos else "reader", roles))
    if pick == "beside_next":
        return go(name, "text_next")
    if pick == "beside_begin":
        return go(name, "text_begin")
    if pick == "rebegin":                               # no kh_unitigs_end between: the begin releases what the last one built
        kind = str(rng.choice(["unitigs_begin", "unitigs_begin_linked"]))
        return Op(kind, ctx=name, mc=draw_graph_mc(rng, c, other_than=u["mc"]))
    if pick in ("end", "merge_across"):
        return go(name, "unitigs_end" if pick == "end" else "merge_across")
    # (merge_across and the two begins have their own picks above; evenly per state: on a running stream or not, located or not)
    enders = [rn for rn in ENDERS if rn not in ("merge_across", "unitigs_begin", "unitigs_begin_linked")]
    return go(name, evenly(("ender", running, u["located"]), enders))


def walk(ops, k, refs=False, visit=None):
    """Applies ops to a fresh model (refs=False: effects only; a text_next hands out what Stream.expect says).  visit(i, op, m) is
    called before every op."""
    m = Model(k)
    for i, op in enumerate(ops):
        if visit:
            visit(i, op, m)
        exp = m.apply(op, refs)
        if op.kind == "text_next" and exp.status == OK:
            m.text_piece(op.ctx, exp["n"])
        if op.kind == "unitigs_text_next" and exp.status == OK:
            m.unitig_text_piece(op.ctx, exp["n"])
    return m


def sequence(seed, n_steps=STEPS, k=21, borrow=(), salt=0, graph=False):
    """n_steps drawn calls, an audit of every context after every AUDIT_EVERY of them and at the end.  borrow: the contexts that have
    a one-rank communicator (merge_across is drawn for them).  graph: a graph walk (draw_graph).  The same arguments give the same list."""
    rng = np.random.default_rng([seed, k, len(borrow), salt, 20261020] + ([1] if graph else []))
    m = Model(k)
    ops = []

    def put(op):
        ops.append(op)
        exp = m.apply(op, refs=False)
        if op.kind == "text_next" and exp.status == OK:
            m.text_piece(op.ctx, exp["n"])
        if op.kind == "unitigs_text_next" and exp.status == OK:
            m.unitig_text_piece(op.ctx, exp["n"])

    for step in range(n_steps):
        if step and step % (GRAPH_AUDIT_EVERY if graph else AUDIT_EVERY) == 0:
            for name in CTXS:
                put(Op("audit", ctx=name))
        put(draw_graph(rng, m, borrow) if graph else draw(rng, m, borrow))
    for name in CTXS:
        put(Op("audit", ctx=name))
    return ops


def graph_cases(seeds=GRAPH_SEEDS):
    return [(seed, forms) for forms in TRIPLES for seed in range(seeds)]


def graph_case_sequence(seed, forms):
    return sequence(seed, GRAPH_STEPS, k_of(forms), borrow=tuple(n for n, f in zip(CTXS, forms) if f == "borrow"),
                    salt=TRIPLES.index(tuple(forms)), graph=True)


def case_sequence(seed, forms):
    return sequence(seed, STEPS, k_of(forms), borrow=tuple(n for n, f in zip(CTXS, forms) if f == "borrow"), salt=TRIPLES.index(tuple(forms)))


# ---- what a set of sequences reaches -------------------------------------------------------------------------------------------------
class GraphCoverage:
    """The counters of the graph walks: what reaches the unitig text stream, the place map and the chunk buffers of the two host
    forms.  visit() sees every op before the model applies it."""
    NAMES = ("utext_begin", "utext_next", "locate", "ustreams_ended", "ends_ustream", "ends_located", "read_between_unexts",
             "read_between_locates", "alternate", "locate_after_rebegin", "host_pair", "empty_S")

    def __init__(self, cov):
        self.cov = cov
        # per context: the READ roles since the last piece with bytes of the running unitig stream / since the last successful locate
        # call of the live begin (None: there is none); for X = "unitig" and "result", None: no piece with bytes of the running X
        # stream yet, 0: one, 1: one and a piece of the other stream behind it; whether the live begin followed a located one directly
        self.since_unext = {n: None for n in CTXS}
        self.since_locate = {n: None for n in CTXS}
        self.piece = {n: {"unitig": None, "result": None} for n in CTXS}
        self.rebegun = {n: False for n in CTXS}

    def visit(self, i, op, m):
        cov, kind = self.cov, op.kind
        for role, name, cls in op.roles():
            c = m.ctx[name]
            u = c.unitigs
            rn = role_name(kind, role)
            if ends(cls) or kind == "unitigs_end":
                if u is not None and u["text"] is not None and u["text"].outstanding() > 0:
                    cov["ends_ustream"][rn] += 1
                if u is not None and u["located"]:
                    cov["ends_located"][rn] += 1
                if kind in ("unitigs_begin", "unitigs_begin_linked"):
                    self.rebegun[name] = u is not None and u["located"] and max(u["mc"], 1) != max(op.mc, 1)
                else:
                    self.rebegun[name] = False
                self.since_unext[name] = self.since_locate[name] = None
                self.piece[name]["unitig"] = None
                if kind != "unitigs_end":                  # (kh_unitigs_end leaves the kh_result_text_* stream alone)
                    self.piece[name]["result"] = None
            refused = (kind in ("unitigs_copy", "links_copy", "unitigs_locate", "unitigs_text_begin") and u is None) or \
                (kind == "links_copy" and u is not None and not u["linked"]) or \
                (kind == "unitigs_text_begin" and u is not None and op.fmt == "gfa" and not u["linked"])
            if cls == "READ" and not refused:
                if self.since_unext[name] is not None and kind != "unitigs_text_begin":
                    self.since_unext[name].append(rn)
                if self.since_locate[name] is not None and kind != "unitigs_locate":      # (a locate call: below)
                    self.since_locate[name].append(rn)
        if kind in ("unitigs_begin", "unitigs_begin_linked"):
            c = m.ctx[op.ctx]
            if selected(c.keys, c.counts, op.mc)[0].size == 0:
                cov["empty_S"]["begin"] += 1
        if kind == "unitigs_text_begin":
            c = m.ctx[op.ctx]
            u = c.unitigs
            if u is None:
                cov["utext_begin"]["state: no unitigs"] += 1
            elif op.fmt == "gfa" and not u["linked"]:
                cov["utext_begin"]["state: gfa behind a plain begin"] += 1
            else:
                cov["utext_begin"]["ok " + op.fmt] += 1
                if u["text"] is not None and 0 < u["text"].pos < u["text"].n_bytes:
                    cov["utext_begin"]["restart with bytes outstanding"] += 1
                if selected(c.keys, c.counts, u["mc"])[0].size == 0:
                    cov["empty_S"]["text"] += 1
                self.since_unext[op.ctx] = None
                self.piece[op.ctx]["unitig"] = None
        if kind == "text_begin":
            self.piece[op.ctx]["result"] = None
        if kind in ("text_next", "unitigs_text_next"):
            mine = "unitig" if kind == "unitigs_text_next" else "result"
            c = m.ctx[op.ctx]
            t = (c.unitigs["text"] if c.unitigs is not None else None) if mine == "unitig" else c.stream
            status, n = (ERR_STATE, 0) if t is None else t.expect(op.cap)
            if mine == "unitig":
                what = ("state" if status == ERR_STATE else "range" if status == ERR_RANGE else "ok bytes" if n else
                        "ok 0 again" if t.ended else "ok 0 at the end")
                cov["utext_next"][what] += 1
                cov["utext_next"][what + (", device" if op.device else ", host")] += 1
                if what == "ok 0 at the end":
                    cov["ustreams_ended"][t.fmt] += 1
                    if t.n_bytes > 2 * UT_CHUNK:
                        cov["ustreams_ended"]["longer than two chunks"] += 1
                if status == OK and n:
                    for rn in self.since_unext[op.ctx] or ():
                        cov["read_between_unexts"][rn] += 1
                    self.since_unext[op.ctx] = []
            if status == OK and n:                              # a piece with bytes
                other = "result" if mine == "unitig" else "unitig"
                st = self.piece[op.ctx]
                if st[mine] == 1:
                    cov["alternate"]["a %s piece between two %s pieces" % (other, mine)] += 1
                st[mine] = 0
                if st[other] == 0:
                    st[other] = 1
        if kind == "unitigs_locate":
            c = m.ctx[op.ctx]
            form = "device" if op.device else "host"
            if c.unitigs is None:
                cov["locate"]["state, " + form] += 1
            else:
                cov["locate"]["ok, " + form] += 1
                if op.kw.get("reads", 1) * (READ_LEN + 1) > PF_CHUNK:
                    cov["locate"]["ok, host, more than one chunk"] += 1
                for rn in self.since_locate[op.ctx] or ():
                    cov["read_between_locates"][rn] += 1
                # (with a successful call in front of it this one lies between that and the next)
                self.since_locate[op.ctx] = ["unitigs_locate"] if self.since_locate[op.ctx] is not None else []
                if self.rebegun[op.ctx]:
                    cov["locate_after_rebegin"]["located"] += 1
                    self.rebegun[op.ctx] = False
                if selected(c.keys, c.counts, c.unitigs["mc"])[0].size == 0:
                    cov["empty_S"]["locate"] += 1
                if c.last == "profile" and not op.device:
                    cov["host_pair"]["profile, then locate"] += 1
        if kind == "profile":
            c = m.ctx[op.ctx]
            if c.last == "unitigs_locate" and not c.last_op.device and c.unitigs is not None:     # (live now: that call was not refused)
                cov["host_pair"]["locate, then profile"] += 1


def coverage(case_list, graph=False, sequences=None):
    """Counters over the walks of case_list = [(seed, forms)]: the conditions tests/test_seq_model.py holds the committed walks to.
    graph: the graph walks (graph_case_sequence) and the counters of GraphCoverage on top.  sequences: {(seed, forms): ops} where
    the caller has drawn them already."""
    cov = {name: Counter() for name in ("kinds", "ends_stream", "ends_unitigs", "read_between_nexts", "read_between_begin_and_copy",
                                        "reader_after_push", "after_reset", "next_status", "streams_ended") + GraphCoverage.NAMES}
    for seed, forms in case_list:
        ops = sequences[seed, forms] if sequences else graph_case_sequence(seed, forms) if graph else case_sequence(seed, forms)
        gc = GraphCoverage(cov)
        # per context: the readers since the last text_next of the running stream / since unitigs_begin; the last push kind
        since_next = {n: None for n in CTXS}
        since_begin = {n: None for n in CTXS}
        last_push = {n: None for n in CTXS}

        def visit(i, op, m):
            cov["kinds"][op.kind] += 1
            gc.visit(i, op, m)
            if op.kind == "unitigs_copy" and m.ctx[op.ctx].unitigs is not None:   # (before the copy itself joins the list below)
                for rn in since_begin[op.ctx] or ():
                    cov["read_between_begin_and_copy"][rn] += 1
                since_begin[op.ctx] = []
            for role, name, cls in op.roles():
                c = m.ctx[name]
                rn = role_name(op.kind, role)
                # a copy that is refused returns nothing: it is no reader for the conditions below
                refused = (op.kind in ("unitigs_copy", "links_copy") and c.unitigs is None) or \
                    (op.kind == "links_copy" and c.unitigs is not None and not c.unitigs["linked"])
                if ends(cls):
                    if c.stream is not None and c.stream.outstanding() > 0:
                        cov["ends_stream"][rn] += 1
                    if c.unitigs is not None:
                        cov["ends_unitigs"][rn] += 1
                    since_next[name] = since_begin[name] = None
                if cls == "READ" and not refused:
                    if since_next[name] is not None and op.kind != "text_begin":
                        since_next[name].append(rn)
                    if since_begin[name] is not None:
                        since_begin[name].append(rn)
                if cls is not None:
                    if last_push[name] and op.kind not in PUSHES and op.kind != "reset" and c.pending and cls == "READ" and not refused:
                        cov["reader_after_push"][last_push[name]] += 1
                    if c.after_reset:
                        what = ("push" if op.kind in PUSHES else "merge_pairs" if op.kind == "merge_pairs" else
                                "dst." + op.kind if role == "dst" else "reader" if cls == "READ" and c.keys.size == 0 else None)
                        if what:
                            cov["after_reset"][what] += 1
                    last_push[name] = op.kind if op.kind in PUSHES else None
            if op.kind == "text_begin":
                since_next[op.ctx] = None
            if op.kind == "text_next":
                s = m.ctx[op.ctx].stream
                status, n = (ERR_STATE, 0) if s is None else s.expect(op.cap)
                cov["next_status"][status] += 1
                if status == OK:
                    for rn in since_next[op.ctx] or ():
                        cov["read_between_nexts"][rn] += 1
                    since_next[op.ctx] = []
                if status == OK and n == 0 and not s.counted:
                    s.counted = True
                    cov["streams_ended"][s.fmt] += 1
                    cov["streams_ended"]["sorted" if s.sorted else "unsorted"] += 1
            if op.kind in ("unitigs_begin", "unitigs_begin_linked"):
                since_begin[op.ctx] = []
            if op.kind == "unitigs_end":
                since_begin[op.ctx] = None

        walk(ops, k_of(forms), visit=visit)
    return cov
