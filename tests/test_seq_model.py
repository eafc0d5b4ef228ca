"""The model and the generator of tests/seq_model.py, on the CPU: the model's content against the oracle, the generator against
itself, and the committed sequences -- what tests/test_gpu_sequences.py runs -- against the states they must reach, so that the
device test cannot pass by never getting there."""
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
    for seed, forms in M.cases()[::7]:
        a, b = M.case_sequence(seed, forms), M.case_sequence(seed, forms)
        assert a == b and [repr(x) for x in a] == [repr(x) for x in b]
        assert [M.parse(repr(x)) for x in a] == a                       # every op's repr is the op again
    assert M.case_sequence(0, M.TRIPLES[0]) != M.case_sequence(1, M.TRIPLES[0])
    n_audits = (M.STEPS - 1) // M.AUDIT_EVERY + 1
    assert len(M.case_sequence(0, M.TRIPLES[0])) == M.STEPS + 3 * n_audits


def test_the_entry_table_names_every_preset_and_every_op():
    """Pins seq_model.ENTRY against an accidental edit: the expected set below is the same table typed a second time, not a check
    against include/kmerhip.h (that is what reading the two side by side is for)."""
    classes = {cls for roles in M.ENTRY.values() for cls in roles.values()}
    assert classes == {"WRITE", "READ", "READ_TAKE", "PUSH", "PUSH_DEVICE", "TEXT_NEXT", None}
    assert set(M.ENDING) == {"push", "push_text", "reset", "push_device", "merge_pairs", "combine_into.dst", "clip_tips_into.src",
                             "clip_tips_into.dst", "pop_bubbles_into.src", "pop_bubbles_into.dst", "result", "result_sorted", "audit",
                             "unitigs_begin", "unitigs_begin_linked", "merge_across"}
    assert all(hasattr(M.Model, "_" + kind) for kind in M.KINDS)


@pytest.fixture(scope="module")
def cov():
    return M.coverage(M.cases())


def at_least(counter, names, n):
    low = {name: counter[name] for name in names if counter[name] < n}
    assert not low, low


def test_every_op_kind_occurs(cov):
    at_least(cov["kinds"], M.KINDS, 10)


def test_every_ending_op_hits_a_running_stream_and_live_unitigs(cov):
    at_least(cov["ends_stream"], M.ENDING, 3)          # (a stream that is on, with bytes still outstanding)
    at_least(cov["ends_unitigs"], M.ENDING, 3)


def test_every_reader_runs_inside_a_stream_and_inside_unitigs(cov):
    # kh_result_text_begin enters as a reader too, but between two kh_result_text_next calls it restarts the stream: those two calls
    # are then not of ONE stream.  It is held to the other condition (it leaves the unitigs alone), and to ends_stream above by
    # nothing: a restart is no end.
    at_least(cov["read_between_nexts"], [rn for rn in M.READ_ROLES if rn != "text_begin"], 3)
    at_least(cov["read_between_begin_and_copy"], M.READ_ROLES, 3)


def test_a_reader_is_the_first_call_after_every_kind_of_push(cov):
    at_least(cov["reader_after_push"], M.PUSHES, 3)


def test_reset_is_followed_by_every_kind_of_first_write_and_by_a_reader(cov):
    at_least(cov["after_reset"], ("push", "merge_pairs", "dst.combine_into", "dst.clip_tips_into", "dst.pop_bubbles_into", "reader"), 3)


def test_text_next_returns_each_of_its_statuses(cov):
    at_least(cov["next_status"], (M.OK, M.ERR_STATE, M.ERR_RANGE), 3)


def test_streams_run_to_their_end(cov):
    at_least(cov["streams_ended"], M.FORMATS + ("sorted",), 5)
