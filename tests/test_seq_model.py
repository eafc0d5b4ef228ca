"""The model and the generator of tests/seq_model.py, on the CPU: the model's content against the oracle, the generator against
itself, and the committed sequences -- what tests/test_gpu_sequences.py runs -- against the states they must reach, so that the
device test cannot pass by never getting there.

Two committed families.  The first walk (seq_model.cases(): 8 seeds x 6 triples of forms) is pinned call by call: a SHA-256 of every
sequence, recorded before the generator learnt the graph walks, is in tests/golden/seq_walk_digest.json.  The graph walks
(seq_model.graph_cases(): 5 seeds x the same triples) draw kh_unitigs_text_* and kh_unitigs_locate* in sessions on live unitigs;
their conditions (every one with a least count of 3) are the second half of this file."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import seq_model as M

U64 = np.uint64
CONTENT_OPS = M.PUSHES + ("merge_pairs", "reset", "combine_into", "clip_tips_into", "pop_bubbles_into")


def oracle_of(parts, k):
    """OracleMap over the concatenation of the chunks pushed or merged, plus pairs added as they are."""
    m = O.OracleMap()
    for p in parts:
        if isinstance(p, int):
            m.process(M.pool(k).reads[p], k)
        else:
            for key, c in zip(p[0].tolist(), p[1].tolist()):
                m.add(key, c)
    keys, counts = m.arrays()
    return np.asarray(keys, dtype=U64), np.asarray(counts, dtype=U64)


def first_seed_with_every_content_op(forms):
    return next(seed for seed in range(M.SEEDS) if {op.kind for op in M.case_sequence(seed, forms)} >= set(CONTENT_OPS))


@pytest.mark.parametrize("forms", [M.TRIPLES[0], M.TRIPLES[2], M.TRIPLES[4], M.TRIPLES[5]], ids=lambda f: "-".join(f))
def test_model_content_is_the_oracles(forms):
    """After every content op each context holds what the oracle counts in everything pushed or merged into it; what combine, clip
    and pop add is their reference applied to the ORACLE's maps of the sources, not to the model's."""
    import test_clip_ref as CR
    import test_gpu_join as T
    import test_gpu_unitig_links as LR
    import test_gpu_unitigs as U
    import test_pop_ref as PR
    k = M.k_of(forms)
    ops = M.case_sequence(first_seed_with_every_content_op(forms), forms)
    parts = {name: [0] for name in M.CTXS}       # what went into each context since its last reset
    seen = set()

    def visit(i, op, m):
        if i:
            prev = ops[i - 1]
            if prev.kind in CONTENT_OPS:
                for _, name, _ in prev.roles():
                    ek, ec = oracle_of(parts[name], k)
                    assert np.array_equal(m.ctx[name].keys, ek) and np.array_equal(m.ctx[name].counts, ec), (i - 1, prev, name)
        if op.kind in M.PUSHES or op.kind == "merge_pairs":
            parts[op.ctx].append(op.chunk)
        elif op.kind == "reset":
            parts[op.ctx] = []
        elif op.kind == "combine_into":
            (ka, va), (kb, vb) = oracle_of(parts[op.a], k), oracle_of(parts[op.b], k)
            parts[op.dst].append(T.np_combine(*T.align(ka, va, kb, vb), op.op, op.calc))
        elif op.kind in ("clip_tips_into", "pop_bubbles_into"):
            ks, vs = oracle_of(parts[op.src], k)
            ref = U.Ref(U.node_dict(ks, vs, k, op.mc), k)
            r = CR.ClipRef(ref, LR.LinkRef(ref), k) if op.kind == "clip_tips_into" else PR.PopRef(ref, LR.LinkRef(ref), 2 * k)
            parts[op.dst].append((r.keys, r.counts))
        seen.add(op.kind)

    M.walk(ops, k, visit=visit)
    assert seen >= set(CONTENT_OPS)


def test_the_same_seed_gives_the_same_ops():
    for make, case_list in ((M.case_sequence, M.cases()[::7]), (M.graph_case_sequence, M.graph_cases()[::7])):
        for seed, forms in case_list:
            a, b = make(seed, forms), make(seed, forms)
            assert a == b and [repr(x) for x in a] == [repr(x) for x in b]
            assert [M.parse(repr(x)) for x in a] == a                   # every op's repr is the op again
    assert M.graph_case_sequence(0, M.TRIPLES[0]) != M.graph_case_sequence(1, M.TRIPLES[0])
    assert M.case_sequence(0, M.TRIPLES[0]) != M.case_sequence(1, M.TRIPLES[0])
    n_audits = (M.STEPS - 1) // M.AUDIT_EVERY + 1
    assert len(M.case_sequence(0, M.TRIPLES[0])) == M.STEPS + 3 * n_audits


@pytest.fixture(scope="module")
def first_walk():
    return {(seed, forms): M.case_sequence(seed, forms) for seed, forms in M.cases()}


def test_the_first_walk_is_the_one_recorded(first_walk):
    """The 48 sequences of the first family are, call by call, what they were before the generator learnt the three graph kinds:
    the digests were recorded at that commit."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_walk_digest.json")) as f:
        want = json.load(f)["sha256"]
    assert len(want) == 48 == len(first_walk) and M.SEEDS == 8
    for (seed, forms), ops in first_walk.items():
        assert not {op.kind for op in ops} & set(M.GRAPH_KINDS)
        got = hashlib.sha256("".join(repr(op) + "\n" for op in ops).encode()).hexdigest()
        assert got == want["%s/%d" % ("-".join(forms), seed)], (seed, forms)


def test_the_entry_table_names_every_preset_and_every_op():
    """Pins seq_model.ENTRY against an accidental edit: the expected set below is the same table typed a second time, not a check
    against include/kmerhip.h (that is what reading the two side by side is for)."""
    classes = {cls for roles in M.ENTRY.values() for cls in roles.values()}
    assert classes == {"WRITE", "READ", "READ_TAKE", "PUSH", "PUSH_DEVICE", "TEXT_NEXT", None}
    assert set(M.ENDING) == {"push", "push_text", "reset", "push_device", "merge_pairs", "combine_into.dst", "clip_tips_into.src",
                             "clip_tips_into.dst", "pop_bubbles_into.src", "pop_bubbles_into.dst", "result", "result_sorted", "audit",
                             "unitigs_begin", "unitigs_begin_linked", "merge_across"}
    assert all(hasattr(M.Model, "_" + kind) for kind in M.KINDS)
    # the three kinds of the graph walks: readers all (none is in ENDING above); kh_unitigs_end ends unitigs without entering
    assert {kd: M.ENTRY[kd] for kd in M.GRAPH_KINDS} == {"unitigs_text_begin": {"ctx": "READ"}, "unitigs_text_next": {"ctx": "TEXT_NEXT"},
                                                         "unitigs_locate": {"ctx": "READ"}}
    assert set(M.KINDS) == set(M.BASE_KINDS) | set(M.GRAPH_KINDS) and len(M.BASE_KINDS) == 27
    assert set(M.UNITIG_ENDING) == set(M.ENDING) | {"unitigs_end"} and M.ENTRY["unitigs_end"] == {"ctx": None}
    assert set(M.READ_ROLES) == set(M.BASE_READ_ROLES) | {"unitigs_text_begin", "unitigs_locate"}


@pytest.fixture(scope="module")
def cov(first_walk):
    return M.coverage(M.cases(), sequences=first_walk)


def at_least(counter, names, n):
    low = {name: counter[name] for name in names if counter[name] < n}
    assert not low, low


def test_every_op_kind_occurs(cov):
    at_least(cov["kinds"], M.BASE_KINDS, 10)          # (the 27 kinds of the first walk; the other three: the graph walks below)
    assert not [kd for kd in M.GRAPH_KINDS if cov["kinds"][kd]]


def test_every_ending_op_hits_a_running_stream_and_live_unitigs(cov):
    at_least(cov["ends_stream"], M.ENDING, 3)          # (a stream that is on, with bytes still outstanding)
    at_least(cov["ends_unitigs"], M.ENDING, 3)


def test_every_reader_runs_inside_a_stream_and_inside_unitigs(cov):
    # kh_result_text_begin enters as a reader too, but between two kh_result_text_next calls it restarts the stream: those two calls
    # are then not of ONE stream.  It is held to the other condition (it leaves the unitigs alone), and to ends_stream above by
    # nothing: a restart is no end.
    at_least(cov["read_between_nexts"], [rn for rn in M.BASE_READ_ROLES if rn != "text_begin"], 3)
    at_least(cov["read_between_begin_and_copy"], M.BASE_READ_ROLES, 3)


def test_a_reader_is_the_first_call_after_every_kind_of_push(cov):
    at_least(cov["reader_after_push"], M.PUSHES, 3)


def test_reset_is_followed_by_every_kind_of_first_write_and_by_a_reader(cov):
    at_least(cov["after_reset"], ("push", "merge_pairs", "dst.combine_into", "dst.clip_tips_into", "dst.pop_bubbles_into", "reader"), 3)


def test_text_next_returns_each_of_its_statuses(cov):
    at_least(cov["next_status"], (M.OK, M.ERR_STATE, M.ERR_RANGE), 3)


def test_streams_run_to_their_end(cov):
    at_least(cov["streams_ended"], M.FORMATS + ("sorted",), 5)


# ---- the model's rules for the unitig text stream and locate, against the references applied here -----------------------------------
def test_the_models_unitig_text_and_locate_rules():
    """One scripted walk through Model.apply: the statuses of the header's rules, the document against document() over the string
    walk's unitigs, the locate words against locate_ref(), and an empty S."""
    import test_gpu_unitig_text as UT
    import test_gpu_unitig_links as LK
    import test_gpu_unitigs as U
    import test_locate_ref as LO
    k = 21
    m = M.Model(k)
    c = m.ctx["A"]
    do = lambda kind, **kw: m.apply(M.Op(kind, ctx="A", **kw))
    ref = U.Ref(U.node_dict(c.keys, c.counts, k, 2), k)
    bases = np.frombuffer(ref.bases, dtype=np.uint8)
    fasta = UT.document("fasta", ref.rows, bases, [], k)
    gfa = UT.document("gfa", ref.rows, bases, LK.LinkRef(ref).links, k)
    assert fasta.startswith(b">0 LN:i:") and gfa.startswith(UT.HEADER + b"S\t0\t") and b"\nL\t" in gfa
    # nothing begun: all three refuse
    assert do("unitigs_text_begin", fmt="fasta").status == M.ERR_STATE and do("unitigs_text_next", cap=10, device=False).status == M.ERR_STATE
    assert do("unitigs_locate", chunk=0, read=0, device=True).status == M.ERR_STATE
    # a plain begin: fasta, no gfa; no stream yet
    do("unitigs_begin", mc=2)
    assert do("unitigs_text_next", cap=10, device=True).status == M.ERR_STATE
    assert do("unitigs_text_begin", fmt="gfa").status == M.ERR_STATE
    assert do("unitigs_text_begin", fmt="fasta")["n_bytes"] == len(fasta)
    e = do("unitigs_text_next", cap=0, device=False)
    assert e.status == M.ERR_RANGE and c.unitigs["text"].pos == 0                          # consumes nothing
    e = do("unitigs_text_next", cap=100, device=False)
    assert (e.status, e["n"]) == (M.OK, 100)
    m.unitig_text_piece("A", 100, fasta[:100])
    with pytest.raises(AssertionError):
        m.unitig_text_piece("A", 3, b"xyz")
    assert do("unitigs_text_begin", fmt="fasta")["n_bytes"] == len(fasta) and c.unitigs["text"].pos == 0      # a restart
    e = do("unitigs_text_next", cap=1 << 30, device=True)
    assert e["n"] == len(fasta)
    m.unitig_text_piece("A", e["n"], fasta)
    for _ in range(2):                                                                       # the end, and the end again
        e = do("unitigs_text_next", cap=0, device=False)
        assert (e.status, e["n"]) == (M.OK, 0)
        m.unitig_text_piece("A", 0, b"")
    # locate: the reference's words, every reader leaves them; kh_unitigs_end ends the stream and the place map, not the other stream
    flat = m.pool.reads[1][5 * 151:13 * 151]
    e = do("unitigs_locate", chunk=1, read=5, reads=8, device=False)
    assert np.array_equal(e["words"], LO.locate_ref(ref.rows, ref.bases, k, flat)) and np.array_equal(e["bases"], flat)
    assert (e["words"] < np.uint64(LO.ABSENT)).sum() > 500 and e["links"] is None and c.unitigs["located"]
    do("text_begin", fmt="tsv", mc=1, sorted=True)
    do("unitigs_end")
    assert c.stream is not None and c.unitigs is None and set(c.gprobe) == {"unitigs_copy", "unitigs_text_next", "unitigs_locate"}
    assert do("unitigs_text_next", cap=10, device=False).status == M.ERR_STATE and do("unitigs_locate", chunk=0, read=0, device=False).status == M.ERR_STATE
    # the linked begin: both formats; a second begin and a writer end the stream
    do("unitigs_begin_linked", mc=2)
    assert do("unitigs_text_begin", fmt="gfa")["n_bytes"] == len(gfa) and do("unitigs_text_begin", fmt="fasta")["n_bytes"] == len(fasta)
    assert do("unitigs_locate", chunk=0, read=0, device=True)["links"] is not None
    do("unitigs_begin", mc=1)
    assert c.unitigs["text"] is None and not c.unitigs["located"] and do("unitigs_text_next", cap=10, device=False).status == M.ERR_STATE
    do("unitigs_text_begin", fmt="fasta")
    do("push", chunk=1)
    assert c.unitigs is None and set(c.gprobe) == {"unitigs_copy", "links_copy", "unitigs_text_next", "unitigs_locate"}
    # an empty S: a threshold above every count, and a context behind kh_reset
    for empty in (lambda: do("unitigs_begin_linked", mc=int(c.counts.max()) + 1), lambda: (do("reset"), do("unitigs_begin_linked", mc=1))):
        empty()
        assert do("unitigs_text_begin", fmt="fasta")["n_bytes"] == 0 and do("unitigs_text_next", cap=5, device=False)["n"] == 0
        assert do("unitigs_text_begin", fmt="gfa")["n_bytes"] == len(UT.HEADER) and c.unitigs["text"].doc == UT.HEADER
        words = do("unitigs_locate", chunk=0, read=0, device=False)["words"]
        assert set(words.tolist()) == {LO.NO_WINDOW, LO.ABSENT}


# ---- the graph walks: what they must reach, each at least 3 times ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def gcov():
    return M.coverage(M.graph_cases(), graph=True)


def test_graph_every_new_op_kind_occurs(gcov):
    at_least(gcov["kinds"], M.GRAPH_KINDS, 3)


def test_graph_every_outcome_of_the_three_calls(gcov):
    at_least(gcov["utext_begin"], ("ok fasta", "ok gfa", "state: no unitigs", "state: gfa behind a plain begin", "restart with bytes outstanding"), 3)
    at_least(gcov["utext_next"], ("ok bytes", "ok 0 at the end", "ok 0 again", "state", "range"), 3)
    at_least(gcov["utext_next"], ("ok bytes, host", "ok bytes, device"), 3)
    at_least(gcov["locate"], ("ok, device", "ok, host", "state, device", "state, host"), 3)


def test_graph_streams_run_to_their_end_and_past_two_chunks(gcov):
    """With KMERHIP_UNI_TEXT_CHUNK_KB=8 a document of more than 16 KiB turns the two chunks over; with KMERHIP_PROFILE_CHUNK_KB=1 a
    host call over more than 1024 bytes takes more than one chunk.  Both from the model's own lengths."""
    assert M.GRAPH_ENV == {"KMERHIP_UNI_TEXT_CHUNK_KB": "8", "KMERHIP_PROFILE_CHUNK_KB": "1"} and M.UT_CHUNK == 8192 and M.PF_CHUNK == 1024
    at_least(gcov["ustreams_ended"], M.UNITIG_FORMATS + ("longer than two chunks",), 3)
    at_least(gcov["locate"], ("ok, host, more than one chunk",), 3)


def test_graph_every_ending_role_hits_a_running_unitig_stream_and_a_place_map(gcov):
    at_least(gcov["ends_ustream"], M.UNITIG_ENDING, 3)      # (a stream with bytes outstanding)
    at_least(gcov["ends_located"], M.UNITIG_ENDING, 3)      # (unitigs that a locate call has built the place map of)


def test_graph_every_reader_runs_between_two_pieces_and_between_two_locate_calls(gcov):
    # kh_unitigs_text_begin between two pieces restarts the stream: exempt there, as kh_result_text_begin is in the first walk
    at_least(gcov["read_between_unexts"], [rn for rn in M.READ_ROLES if rn != "unitigs_text_begin"], 3)
    at_least(gcov["read_between_locates"], M.READ_ROLES, 3)


def test_graph_the_two_text_streams_alternate(gcov):
    at_least(gcov["alternate"], ("a result piece between two unitig pieces", "a unitig piece between two result pieces"), 3)


def test_graph_a_locate_call_follows_a_second_begin_on_located_unitigs(gcov):
    at_least(gcov["locate_after_rebegin"], ("located",), 3)


def test_graph_profile_and_host_locate_next_to_each_other(gcov):
    at_least(gcov["host_pair"], ("profile, then locate", "locate, then profile"), 3)


def test_graph_an_empty_node_set(gcov):
    at_least(gcov["empty_S"], ("begin", "text", "locate"), 3)
