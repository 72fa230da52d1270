"""Self-tests of the guard-band allocator (tests/arena.py) on CPU tensors, and the coverage condition of the extent tests:
every entry point of include/wedetect_hip.h that takes device memory has a case in tests/test_gpu_extents.py.

The "stray stores" below are ordinary torch indexing inside the arena's own allocation: no kernel is built to misbehave and
nothing is written outside an allocation."""
import fnmatch
import re

import pytest
import torch

from tests.abi_decl import declared
from tests.arena import ALT_PATTERN, GUARD_MIN_BYTES, Arena, GuardViolation, pattern_value


def _arena(pattern=0x00, cap=8 << 20):
    return Arena(cap, "cpu", pattern)


def _one(ar):
    v = ar.violations()
    assert len(v) == 1, v
    return v[0]


@pytest.mark.parametrize("pattern", [0x00, 0xFF])
def test_clean_run_reports_nothing(pattern):
    ar = _arena(pattern)
    x = ar.take("x", (7, 12), ld=20, role="input", misalign=16, data=torch.arange(84.).view(7, 12))
    y = ar.take("y", (7, 12), ld=16, role="output", misalign=4)
    idx = ar.take("idx", (3, 8), torch.int32, role="output", fillers=(-1,))
    ws = ar.take("ws", (1000,), torch.uint8, role="workspace", fill=0xFF)
    assert x.data_ptr() % 256 == 16 and y.data_ptr() % 256 == 4 and idx.data_ptr() % 256 == 0
    assert x.stride() == (20, 1) and y.stride() == (16, 1) and bool((ws == 255).all())
    ar.arm()
    y.copy_(x * 2)                      # every payload byte of the outputs written, filler included
    idx.fill_(-1)
    ws.fill_(3)
    ar.check()
    assert torch.equal(y, torch.arange(84.).view(7, 12) * 2)


def test_geometry_guard_is_at_least_64k_and_256_rows():
    ar = _arena(cap=64 << 20)
    ar.take("narrow", (4, 8), ld=8)
    ar.take("wide", (4, 100), ld=3000)
    b = ar.buffers
    assert b["narrow"].guard == GUARD_MIN_BYTES
    assert b["wide"].guard == 256 * 3000 * 4 >= GUARD_MIN_BYTES
    assert b["wide"].start - b["wide"].guard >= b["narrow"].end + b["narrow"].guard     # guards are not shared
    t = ar.take("t3", (2, 3, 5), ld=8)
    assert t.stride() == (24, 8, 1)
    with pytest.raises(MemoryError):
        _arena(cap=100 << 10).take("big", (1 << 20,))
    with pytest.raises(ValueError):
        ar.take("narrow", (1,))
    with pytest.raises(ValueError):
        ar.take("bad", (4, 8), ld=4)


@pytest.mark.parametrize("pattern", [0x00, 0xFF])
def test_one_byte_store_at_distance_one_on_each_side(pattern):
    for side in ("low", "high"):
        ar = _arena(pattern)
        ar.take("a", (5, 6), ld=6, misalign=16)
        ar.take("b", (4,), torch.int32)
        buf = ar.buffers["a"]
        ar.arm()
        ar.mem[buf.start - 1 if side == "low" else buf.end] = 0x5A
        v = _one(ar)
        assert v == dict(buffer="a", side=f"{side} guard", first=1, last=1, count=1)
        with pytest.raises(GuardViolation, match=rf"a: {side} guard: 1 byte\(s\), first at 1, last at 1"):
            ar.check()


def test_store_at_the_far_end_of_a_guard():
    ar = _arena(0xFF)
    ar.take("a", (3, 4))
    buf = ar.buffers["a"]
    ar.arm()
    ar.mem[buf.end + buf.guard - 1] = 0
    ar.mem[buf.end + 99] = 0
    assert _one(ar) == dict(buffer="a", side="high guard", first=100, last=buf.guard, count=2)
    ar.mem[buf.end + buf.guard - 1] = 0xFF
    ar.mem[buf.end + 99] = 0xFF
    ar.mem[buf.start - buf.guard] = 1
    assert _one(ar) == dict(buffer="a", side="low guard", first=buf.guard, last=buf.guard, count=1)


def test_store_into_a_spare_column_of_a_middle_row():
    ar = _arena(0x00)
    y = ar.take("y", (9, 10), ld=16, role="output")
    buf = ar.buffers["y"]
    ar.arm()
    y.fill_(1.0)
    ar.check()                                            # payload writes are legitimate
    ar.mem[buf.start + 4 * buf.pitch + buf.row_bytes] = 7            # row 4, first spare byte
    ar.mem[buf.start + 6 * buf.pitch + buf.pitch - 1] = 7            # row 6, last spare byte
    assert _one(ar) == dict(buffer="y", side="spare columns", first=(4, 1), last=(6, 24), count=2)
    # the spare bytes behind the LAST row belong to the high guard
    ar2 = _arena(0x00)
    ar2.take("y", (9, 10), ld=16)
    b2 = ar2.buffers["y"]
    ar2.arm()
    ar2.mem[b2.end] = 1
    assert _one(ar2)["side"] == "high guard"


def test_changed_input_is_reported_and_inout_is_not():
    ar = _arena()
    x = ar.take("x", (4, 8), ld=12, role="input", data=torch.ones(4, 8))
    r = ar.take("res", (4, 8), role="inout", data=torch.ones(4, 8))
    ar.arm()
    r.add_(1)
    ar.check()
    x[2, 3] = 5.0
    v = _one(ar)
    assert v["buffer"] == "x" and v["side"] == "input changed" and v["first"][0] == 2 and 12 <= v["first"][1] < 16
    with pytest.raises(RuntimeError):
        _arena().check()                                  # never armed


def test_a_stray_filler_store_differs_from_the_guard_of_an_integer_output():
    """The -1 rows of the top-k index output: with the 0xFF surroundings a stray int32 -1 would equal the guard, so the
    pattern around such a buffer is 0x7F; a float buffer of the same arena keeps 0xFF."""
    ar = _arena(0xFF)
    idx = ar.take("idx", (2, 8), torch.int32, ld=12, role="output", fillers=(-1,))
    f = ar.take("f", (2, 8), role="output")
    bi, bf = ar.buffers["idx"], ar.buffers["f"]
    assert bi.pattern == ALT_PATTERN and bf.pattern == 0xFF
    assert pattern_value(0xFF, torch.int32) == -1 and pattern_value(ALT_PATTERN, torch.int32) != -1
    assert bool((ar.mem[bi.start - bi.guard:bi.start] == ALT_PATTERN).all()) and bool((ar.mem[bi.end:bi.end + bi.guard] == ALT_PATTERN).all())
    ar.arm()
    idx.fill_(-1)
    ar.check()
    wide = ar.mem.as_strided((2, 12 * 4), (bi.pitch, 1), bi.start).view(torch.int32)      # the rows with their spare columns
    wide[0, 8] = -1                                       # a filler store one element past the row
    v = _one(ar)
    assert v == dict(buffer="idx", side="spare columns", first=(0, 1), last=(0, 4), count=4)
    assert Arena(1 << 20, "cpu", 0x00).take("i0", (4,), torch.int32, fillers=(-1,)).numel() == 4    # 0x00 differs from -1 already
    with pytest.raises(ValueError):
        _arena(0xFF).take("x", (4,), torch.int32, fillers=(-1, pattern_value(ALT_PATTERN, torch.int32)))


def test_shrunk_extent_reports_legitimate_stores_at_the_edge():
    """What the device sensitivity tests rely on: declare the extent smaller than the truth and the ordinary stores of the last
    row / column / 16 bytes are reported at the right offsets."""
    ar = _arena()
    y = ar.take("y", (6, 8), ld=8, role="output")
    ar.shrink("y", rows=1)
    ar.arm()
    y.fill_(pattern_value(0x3C, torch.float32))    # no byte equals the pattern
    assert _one(ar) == dict(buffer="y", side="high guard", first=1, last=32, count=32)
    ar = _arena()
    y = ar.take("y", (6, 8), ld=12, role="output")
    ar.shrink("y", cols=1)
    ar.arm()
    y.fill_(pattern_value(0x3C, torch.float32))    # no byte equals the pattern
    v = ar.violations()
    assert v[0] == dict(buffer="y", side="high guard", first=1, last=4, count=4)          # last row's dropped column
    assert v[1] == dict(buffer="y", side="spare columns", first=(0, 1), last=(4, 4), count=20)
    ar = _arena()
    w = ar.take("w", (100,), torch.uint8, role="workspace")
    ar.shrink("w", tail_bytes=16)
    ar.arm()
    w.fill_(9)
    assert _one(ar) == dict(buffer="w", side="high guard", first=1, last=16, count=16)


def test_guard_bytes_widens_the_guard_and_the_blocked_walk_finds_what_the_mask_finds():
    """The guard-size parameter of the large-offset tests (tests/test_gpu_offsets.py: 2 GiB per side there, 1 MiB here) and the
    block-wise check that goes with it: the same stores, found at the same places as by violations(), with blocks far smaller
    than the buffers and not aligned to anything."""
    ar = _arena(0xFF, cap=16 << 20)
    x = ar.take("x", (9, 10), ld=16, role="input", guard_bytes=1 << 20, data=torch.ones(9, 10))
    ar.take("small", (4, 8), guard_bytes=100)                                 # the caller's figure stands, rounded up to 256
    ar.take("img", (3, 4, 6), ld=8, batch_stride=7, misalign=16, guard_bytes=(1 << 20) + 1)
    b, bs, bi = ar.buffers["x"], ar.buffers["small"], ar.buffers["img"]
    assert b.guard == 1 << 20 and bs.guard == 256 < GUARD_MIN_BYTES and bi.guard == (1 << 20) + 256 and (bi.start - ar._base) % 256 == 16
    assert bs.start - bs.guard >= b.end + b.guard and bi.start - bi.guard >= bs.end + bs.guard
    with pytest.raises(ValueError):
        ar.take("neg", (4,), guard_bytes=-1)
    with pytest.raises(RuntimeError):
        ar.check_blocked()
    ar.arm()
    for blk in (1 << 30, 4096, 1001):
        ar.check_blocked(blk)
        assert ar.violations_blocked(blk) == []
    stores = [(b.start - (1 << 20), dict(buffer="x", side="low guard", first=1 << 20)),
              (b.end + (1 << 20) - 1, dict(buffer="x", side="high guard", first=1 << 20)),
              (b.start + 3 * b.pitch + b.row_bytes + 2, dict(buffer="x", side="spare columns", first=(3, 3))),
              (bi.start + 4 * bi.pitch, dict(buffer="img", side="spare columns", first=(3, 32 - 24 + 1))),      # first row between two images
              (bi.start + 7 * bi.pitch - 1, dict(buffer="img", side="spare columns", first=(3, 3 * 32 + 8))),       # last byte before image 1
              (bi.start + (7 + 2) * bi.pitch + bi.row_bytes, dict(buffer="img", side="spare columns", first=(6, 1)))]
    for at, want in stores:
        keep = int(ar.mem[at])
        ar.mem[at] = 0x5A
        full = _one(ar)
        for blk in (1 << 30, 1001):
            got = ar.violations_blocked(blk)
            assert len(got) == 1 and {k: got[0][k] for k in want} == want, (at, blk, got)
            assert (full["buffer"], full["side"], full["first"]) == (want["buffer"], want["side"], want["first"])
        with pytest.raises(GuardViolation, match=want["buffer"] + ": " + want["side"]):
            ar.check_blocked(1001)
        ar.mem[at] = keep
    x[8, 9] = 2.0
    got = ar.violations_blocked(1001)
    assert len(got) == 1 and got[0]["side"] == "input changed" and got[0]["first"][0] == 8 and 36 <= got[0]["first"][1] < 40


# ------------------------------------------------------------------------------------------ coverage of the C ABI
# The closed set the extent tests may leave out: functions without device memory and the two diagnostics.  wd_recall_scratch_floats
# and wd_topk_capacity are pointer-free size queries like the *_bytes family (their names just do not end in _bytes); the
# _takes_memory() check below holds every name here except the two probes and the event hook to "no pointer parameter".
EXEMPT_ALLOWED = ("wd_abi_version", "wd_strerror", "wd_sizeof_*", "*_bytes", "*_config", "wd_time_next_gemm",
                  "wd_probe_lds_dma", "wd_probe_issue", "wd_recall_scratch_floats", "wd_topk_capacity")


def _takes_memory(proto) -> bool:
    """A pointer parameter other than the stream handle (the WdConvGemm description counts: it carries device pointers).
    ``proto``: a (return type, [parameter strings]) entry of ``abi_decl.declared``."""
    return any("*" in p and not re.search(r"\bvoid\s*\*\s*stream$", p) for p in proto[1])


def test_every_entry_point_with_device_memory_has_an_extents_case():
    from tests.test_gpu_extents import CASES, EXEMPT
    decl = declared("wedetect_hip.h")
    assert len(decl) >= 55 and {"wd_conv_gemm", "wd_topk_candidates", "wd_det_match", "wd_stem_fused"} <= set(decl)
    covered = {c.entry for c in CASES}
    for name in sorted(decl):
        assert name in covered or name in EXEMPT, f"{name}: new ABI entry without a case in tests/test_gpu_extents.py (or an EXEMPT reason)"
        assert not (name in covered and name in EXEMPT), f"{name}: both covered and exempt"
    for name, reason in EXEMPT.items():
        assert name in decl, f"EXEMPT names {name}, which the header does not declare"
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason
        assert any(fnmatch.fnmatch(name, pat) for pat in EXEMPT_ALLOWED), f"{name} may not be exempt: it must have a case"
        if name not in ("wd_probe_lds_dma", "wd_probe_issue", "wd_time_next_gemm"):
            assert not _takes_memory(decl[name]), f"{name} takes device memory: it must have a case"
    unknown = covered - set(decl)
    assert not unknown, f"cases for entry points the header does not declare: {sorted(unknown)}"
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)), "case ids must be unique"
