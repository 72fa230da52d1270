"""Guard-band tests (GPU) of include/wedetect_hip_groups.h, run as tests/test_gpu_topn_extents.py runs the entry points of the
top-n header (the harness of tests/test_gpu_extents.py: its Ctx / Run / Case / execute): every operand is carved from a
tests/arena.py Arena with guard bands, the case runs in 0x00 and in 0xFF surroundings (outputs bit-identical, inputs unchanged, no
range flag) and its values are checked once.  The output buffer STARTS AS 0xFF bytes (a NaN pattern) in both surroundings and must
come out finite: every element is written, nothing relies on a cleared buffer.

tests/test_cpu_groups.py asserts on the CPU that every function of the header that takes device memory has a case here."""
from __future__ import annotations

import math
from typing import List

import pytest
import torch
import torch.nn.functional as F

import tests.groups_hazards  # noqa: F401
import tests.test_gpu_extents as X
from tests import groups_ref as GR

pytestmark = pytest.mark.gpu

f32, i32, f64 = torch.float32, torch.int32, torch.float64

CASES: List[X.Case] = []


def case(entry: str, name: str, cap: int = 64 << 20, **kw):
    def deco(fn):
        CASES.append(X.Case(entry, name, (lambda ctx, _fn=fn, _kw=kw: _fn(ctx, **_kw)), cap))
        return fn
    return deco


def _plan(sizes):
    from wedetect_amd.groups import PromptGroups
    return PromptGroups.from_sizes(sizes)


def _out(ctx, rows, G, ldo):
    """The output, carved with its payload at 0xFF whatever the surroundings."""
    return ctx.ar.take("out", (rows, G), f32, ld=ldo, misalign=4, role="output", fill=0xFF)


@case("wd_group_similarity_split", "2 x 85 rows (buffer padded to 176), one bin of 8 classes, ldo G + 3", b=2, ntot=85, ends=(64, 80), sizes=GR.ONE_BIN, pad=3)
@case("wd_group_similarity_split", "1 x 300 rows, K_pad 352 (two column tiles), the second launch of two (offset 256)", b=1, ntot=300, ends=(200, 280),
      sizes=GR.K352, pad=0, c0=256)
@case("wd_group_similarity_split", "1 x 85 rows, K_pad 352 whole", b=1, ntot=85, ends=(64, 80), sizes=GR.K352, pad=1)
def _group_sim(ctx, b, ntot, ends, sizes, pad, c0=0, dim=768, es_scale=4.0):
    """The rows of e_split behind the last one keep the surroundings' pattern; out[r][first class of the launch ..) is the only
    thing written, and the tables are read from the launch's first bin on."""
    from wedetect_amd import groups as PG
    pg = _plan(sizes)
    rows = b * ntot
    rows8 = (rows + 7) // 8 * 8
    e, flat = X._rand(91, rows, dim, scale=0.8), F.normalize(X._rand(92, pg.P, dim), dim=-1)
    t = flat[pg.rows]
    es_val = X.split_cpu(e * es_scale)
    es = ctx.ar.take("e_split", (rows8, dim), f32, misalign=16, role="input")
    es[:rows].copy_(es_val.cuda())
    tsc = 2.0 ** (13 - math.floor(math.log2(float(t.abs().max()))))
    ts = X._padded_split(ctx, "t_split", t[c0:], tsc)
    g_first = int(pg.bin_first[c0 // 32])
    # the tables of the launch alone, addressed as the whole tables would be: the entries in front of the launch are outside the arena
    go = ctx.inp("group_of", pg.group_of[c0:].clone(), mis=4)
    bf = ctx.inp("bin_first", pg.bin_first[c0 // 32:].clone(), mis=4)
    G = pg.G
    ldo = G + pad
    out = _out(ctx, rows, G - g_first, ldo)
    flag = ctx.flag()
    seg = (ntot, ends[0], ends[1], (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))

    def launch():
        PG.group_similarity_split(es, rows, ts, (1.0 / tsc) / es_scale, pg.K_pad - c0, dim, go.data_ptr() - c0 * 4, bf.data_ptr() - c0 // 32 * 4, c0,
                                  out.data_ptr() - g_first * 4, ldo, G, seg=seg, range_flag=flag)

    def value(o):
        lvl = torch.arange(rows) % ntot
        lvl = (lvl >= ends[0]).long() + (lvl >= ends[1]).long()
        sc, bi = torch.tensor(seg[3], dtype=f64)[lvl][:, None], torch.tensor(seg[4], dtype=f64)[lvl][:, None]
        ref = torch.sigmoid((X.unsplit(es_val) / es_scale) @ t.double().T * sc + bi)
        ref = GR.class_amax(ref, pg.group_of.numpy())[:, g_first:]
        X.assert_close("class scores", o["out"].cpu(), ref, *X.TOL_SIM_SPLIT)
    return X.Run(launch, lambda: {"out": out}, value, f"rows {rows} K_pad {pg.K_pad} from row {c0}: classes {g_first} .. {G}, ldo {ldo}", [flag])


@case("wd_group_rows", "37 rows, K_pad 352 in a block of ld 357, ldo G + 3", rows=37, sizes=GR.K352, ld_pad=5, pad=3)
@case("wd_group_rows", "9 rows, the bins from row 256 on of K_pad 352", rows=9, sizes=GR.K352, ld_pad=0, pad=0, c0=256)
@case("wd_group_rows", "5 rows, one bin", rows=5, sizes=GR.ONE_BIN, ld_pad=0, pad=0)
def _group_rows(ctx, rows, sizes, ld_pad, pad, c0=0):
    from wedetect_amd import groups as PG
    pg = _plan(sizes)
    n_cls = pg.K_pad - c0
    blk = torch.rand(rows, n_cls, generator=torch.Generator().manual_seed(3))
    b_d = ctx.inp("block", blk, ld=n_cls + ld_pad, mis=4)
    g_first = int(pg.bin_first[c0 // 32])
    go = ctx.inp("group_of", pg.group_of[c0:].clone(), mis=4)
    bf = ctx.inp("bin_first", pg.bin_first[c0 // 32:].clone(), mis=4)
    G = pg.G
    ldo = G + pad
    out = _out(ctx, rows, G - g_first, ldo)

    def launch():
        PG.group_rows(b_d, rows, n_cls, n_cls + ld_pad, go.data_ptr() - c0 * 4, bf.data_ptr() - c0 // 32 * 4, c0, out.data_ptr() - g_first * 4, ldo, G)

    def value(o):
        assert torch.equal(o["out"].cpu(), GR.class_amax(blk, pg.group_of.numpy()[c0:]))
    return X.Run(launch, lambda: {"out": out}, value, f"rows {rows} columns {n_cls} from row {c0}, ldo {ldo}")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_groups_extents(c):
    run0, o0, f0 = X.execute(c, 0x00, 0xFF)
    run1, o1, f1 = X.execute(c, 0xFF, 0xFF)
    assert not any(f0) and not any(f1), f"range flags raised: surroundings 0x00 {f0}, 0xFF {f1}"
    X._same(o0, o1, "surroundings 0x00 vs 0xFF")
    for k, v in o1.items():
        assert bool(torch.isfinite(v).all()), f"output {k!r}: elements left at their 0xFF start"
    run0.value(o0)
    print(f"{c.id}: {run0.info}: guards clean, 0x00 == 0xFF, every element written, flags 0")
