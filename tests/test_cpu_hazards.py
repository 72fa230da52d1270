"""Self-tests of the happens-before checker (tests/hazards.py) — no device: the clock and overlap logic is driven with fake
streams, events and addresses, and the ACCESS / EXEMPT tables are held against the package source."""
import ast
import os
import random
import re

import pytest

from tests import hazards as H
from tests.hazards import A, R, W, Model

BUF = 0x10000                       # a fake buffer address
S1, S2, S3 = "s1", "s2", "s3"


def acc(mode, off=0, n=64):
    return (mode, BUF + off, 1, n, n)


def cols(mode, c0, c1, rows=8, ld=256):
    """Columns [c0, c1) of every row of a row-strided buffer."""
    return (mode, BUF + c0, rows, ld, c1 - c0)


def pairs(m):
    return [(h.first.split("#")[0], h.second.split("#")[0]) for h in m.hazards()]


# ---- conflicts that must be reported -------------------------------------------------------------------------------------
CONFLICTS = {"raw": (W, R), "waw": (W, W), "war": (R, W)}


@pytest.mark.parametrize("kind", sorted(CONFLICTS))
def test_unordered_conflict_across_streams_is_reported(kind):
    first, second = CONFLICTS[kind]
    m = Model()
    m.launch(S1, "producer", [acc(first)])
    m.launch(S2, "consumer", [acc(second)])
    hz = m.hazards()
    assert len(hz) == 1 and hz[0].first == f"producer@s1#0 {first}" and hz[0].second == f"consumer@s2#1 {second}"


def test_wait_issued_before_the_record_it_was_meant_for():
    """The stale-snapshot case: a wait takes the snapshot the event holds WHEN THE WAIT IS ISSUED — none here."""
    m = Model()
    m.launch(S1, "producer", [acc(W)])
    m.wait("ev", S2)                  # nothing recorded yet: adds nothing
    m.record("ev", S1)
    m.launch(S2, "consumer", [acc(R)])
    assert pairs(m) == [("producer@s1", "consumer@s2")]


def test_wait_on_an_older_record_does_not_cover_later_work():
    m = Model()
    m.record("ev", S1)                # last step's record
    m.launch(S1, "producer", [acc(W)])
    m.wait("ev", S2)                  # the record of THIS step has not been issued yet
    m.launch(S2, "consumer", [acc(R)])
    m.record("ev", S1)
    assert pairs(m) == [("producer@s1", "consumer@s2")]


def test_event_re_recorded_between_record_and_wait():
    m = Model()
    m.launch(S1, "producer", [acc(W)])
    m.record("ev", S1)
    m.record("ev", S3)                # replaces the snapshot: the waiter now waits for s3, not for the producer
    m.wait("ev", S2)
    m.launch(S2, "consumer", [acc(R)])
    assert pairs(m) == [("producer@s1", "consumer@s2")]


def test_two_lanes_writing_the_same_columns():
    m = Model()
    m.launch(S1, "lane1", [cols(W, 0, 128)])
    m.launch(S2, "lane2", [cols(W, 64, 192)])
    assert pairs(m) == [("lane1@s1", "lane2@s2")]


def test_atomic_against_a_plain_access_is_reported():
    for other in (R, W):
        m = Model()
        m.launch(S1, "flag", [acc(A, n=4)])
        m.launch(S2, "plain", [acc(other, n=4)])
        assert len(m.hazards()) == 1


def test_an_ignored_wait_is_left_out_of_the_model():
    m = Model()
    m.launch(S1, "producer", [acc(W)])
    m.record("ev", S1)
    m.wait("ev", S2, ignored=True)
    m.launch(S2, "consumer", [acc(R)])
    assert len(m.hazards()) == 1


def test_happens_before_is_not_symmetric_a_later_wait_does_not_order_an_earlier_launch():
    m = Model()
    m.launch(S2, "consumer", [acc(R)])
    m.launch(S1, "producer", [acc(W)])
    m.record("ev", S1)
    m.wait("ev", S2)
    assert len(m.hazards()) == 1


# ---- the same conflicts, ordered: clean ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(CONFLICTS))
@pytest.mark.parametrize("how", ["same_stream", "event", "event_transitive", "wait_stream", "host_sync_all", "host_sync_stream",
                                 "host_sync_event"])
def test_ordered_conflict_is_clean(kind, how):
    first, second = CONFLICTS[kind]
    m = Model()
    m.launch(S1, "producer", [acc(first)])
    s2 = S2
    if how == "same_stream":
        s2 = S1
    elif how == "event":
        m.record("ev", S1)
        m.wait("ev", S2)
    elif how == "event_transitive":       # s1 -> s3 -> s2
        m.record("e1", S1)
        m.wait("e1", S3)
        m.launch(S3, "middle", [])
        m.record("e2", S3)
        m.wait("e2", S2)
    elif how == "wait_stream":
        m.wait_stream(S2, S1)
    elif how == "host_sync_all":
        m.host_sync()
    elif how == "host_sync_stream":
        m.host_sync(stream=S1)
    elif how == "host_sync_event":
        m.record("ev", S1)
        m.host_sync(event="ev")
    m.launch(s2, "consumer", [acc(second)])
    assert m.hazards() == []


def test_host_sync_of_another_stream_orders_nothing():
    m = Model()
    m.launch(S1, "producer", [acc(W)])
    m.launch(S3, "bystander", [])
    m.host_sync(stream=S3)
    m.launch(S2, "consumer", [acc(R)])
    assert len(m.hazards()) == 1


def test_two_lanes_writing_disjoint_column_slices_of_one_buffer():
    m = Model()
    m.launch(S1, "lane1", [cols(W, 0, 128)])
    m.launch(S2, "lane2", [cols(W, 128, 256)])
    m.launch(S3, "lane3", [(W, BUF + 8 * 256, 1, 64, 64)])        # the rows behind them
    assert m.hazards() == []


def test_per_image_row_ranges_of_one_tensor_are_disjoint():
    """Three head levels write [B, anchors, C] on different lanes: per image its own run of rows (the batch form)."""
    c, n = 16, (8, 4, 2)
    m = Model()
    off = 0
    for l, s in enumerate((S1, S2, S3)):
        m.launch(s, f"level{l}", [(W, BUF + off * c, n[l], c, c, 3, sum(n) * c)])
        off += n[l]
    assert m.hazards() == []
    m.launch("s4", "whole", [(R, BUF, 1, 3 * sum(n) * c, 3 * sum(n) * c)])
    assert len(m.hazards()) == 3


def test_atomic_atomic_on_the_same_word_is_clean():
    m = Model()
    for s in (S1, S2, S3):
        m.launch(s, "flag", [acc(A, n=4)])
    assert m.hazards() == []


def test_reads_never_conflict_and_buckets_keep_buffers_apart():
    m = Model(bucket_of=lambda addr: addr >> 16)
    m.launch(S1, "r1", [acc(R)])
    m.launch(S2, "r2", [acc(R)])
    m.launch(S1, "w-other", [(W, 0x50000, 1, 64, 64)])
    m.launch(S2, "r-other", [(R, 0x60000, 1, 64, 64)])
    assert m.hazards() == []


# ---- rectangle intersection against brute force ---------------------------------------------------------------------------
def _bytes(r):
    base, rows, stride, width = r
    return {base + i * stride + x for i in range(rows) for x in range(width)}


def test_rectangle_intersection_matches_a_brute_force_byte_set():
    rng = random.Random(7)
    exact = conservative = 0
    for _ in range(600):
        stride = rng.choice([8, 12, 16, 24])
        rs = []
        for _ in range(2):
            s = stride if rng.random() < 0.8 else rng.choice([8, 12, 16, 24])
            acc_ = (W, 1000 + rng.randrange(0, 96), rng.randrange(1, 6), s, rng.randrange(1, s + 1))
            rs.append(H.normalise(acc_)[0][1:])
        truth = bool(_bytes(rs[0]) & _bytes(rs[1]))
        got = H.rects_intersect(*rs)
        if rs[0][1] == 1 or rs[1][1] == 1 or rs[0][2] == rs[1][2]:
            assert got == truth, (rs, truth)              # a run against anything, or equal strides: exact
            exact += 1
        else:
            assert got or not truth, (rs, truth)          # different strides: may over-report, never under-report
            conservative += 1
        assert H.rects_intersect(rs[1], rs[0]) == got
    assert exact > 300 and conservative > 20


def test_normalise_expands_batches_and_merges_dense_rows():
    assert H.normalise((R, 100, 4, 16, 16)) == [(R, 100, 1, 64, 64)]
    assert H.normalise((R, 100, 4, 32, 16)) == [(R, 100, 4, 32, 16)]
    assert H.normalise((W, 100, 4, 16, 16, 3, 1000)) == [(W, 100, 3, 1000, 64)]
    assert H.normalise((W, 100, 2, 32, 16, 2, 1000)) == [(W, 100, 2, 32, 16), (W, 1100, 2, 32, 16)]
    assert H.normalise((W, 0, 2, 32, 16)) == [] and H.normalise((W, 100, 0, 32, 16)) == []


# ---- the tables against the package source ---------------------------------------------------------------------------------
def _launching_functions():
    """module.function of every function in wedetect_amd/*.py whose body calls stream_ptr()."""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wedetect_amd")
    found = set()
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(pkg, fn)).read())
        for node in ast.walk(tree):
            if not isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                continue
            for call in ast.walk(node):
                f = getattr(call, "func", None)
                if isinstance(call, ast.Call) and (getattr(f, "id", None) == "stream_ptr" or getattr(f, "attr", None) == "stream_ptr"):
                    found.add(f"{fn[:-3]}.{node.name}")
    return found


def test_every_launching_function_is_in_access_or_exempt():
    found = _launching_functions()
    assert len(found) >= 30, found
    known = set(H.ACCESS) | set(H.EXEMPT)
    assert found - known == set(), f"launch without an ACCESS entry or an EXEMPT reason: {sorted(found - known)}"
    assert known - found == set(), f"table entries that launch nothing: {sorted(known - found)}"
    assert not set(H.ACCESS) & set(H.EXEMPT)
    assert all(isinstance(v, str) and len(v) > 10 and "\n" not in v for v in H.EXEMPT.values())


def test_benign_names_only_flag_words_with_a_source_line():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert {w for w, _, _ in H.BENIGN} <= set(H.ACCESS)
    for wrapper, arg, cite in H.BENIGN:
        assert arg in ("range_flag", "range_flags"), (wrapper, arg)
        assert "csrc/" in cite or "split_gemm_impl.h" in cite
    # every csrc/<file>:<line> cited shows, within a few lines of it (unrelated edits move lines), the plain store of the
    # constant 1 or the hand-over of the flag pointer to the shared epilogues that it is cited for
    checked = 0
    for _, _, cite in H.BENIGN:
        for part in re.split(r"csrc/", cite)[1:]:
            fn = re.match(r"[\w.]+", part).group(0)
            head = part.split("`")[0]
            lines = [int(n) for n in re.findall(r"(?<![\w.])(\d{2,4})(?![\w.])", head)]
            src = open(os.path.join(root, "wedetect_amd", "csrc", fn)).read().splitlines()
            for ln in lines:
                near = "\n".join(src[max(0, ln - 16): ln + 15])
                assert "*p.range_flag = 1u;" in near or "range_flag = q.range_flag" in near or "p.range_flag = range_flag" in near, (fn, ln)
                checked += 1
    assert checked >= 10
    # and the kernels store into the flag in no other way
    for fn in sorted(f for f in os.listdir(os.path.join(root, "wedetect_amd", "csrc")) if f.endswith((".hip", ".h"))):
        for line in open(os.path.join(root, "wedetect_amd", "csrc", fn)).read().splitlines():
            if re.search(r"\*\s*\w+\.range_flag\s*[|&+^]?=", line):
                assert "*p.range_flag = 1u;" in line, (fn, line)
