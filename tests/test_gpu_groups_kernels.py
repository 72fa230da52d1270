"""The device entry points of include/wedetect_hip_groups.h (GPU): the fused similarity + class maximum against the materialising
launch it must equal bit for bit, wd_group_rows over that launch's output, torch's amax per class, float64, the range flag, the
refusals.

Shapes: 252 and 300 region rows (one ragged 256-row tile; a tile boundary with a ragged second tile whose last 32-row group is
cut at 12 rows), level boundaries at 64 / 80 of every 84 rows (inside a wave's 32 rows).  Plans: one bin; K_pad = 352 (a whole
256-column tile and a ragged one; a singleton, a class that ends its bin exactly, 32-prompt classes, a bin closed with 31 padding
rows); the LVIS-en plan (2048 rows, eight column tiles).  Output row strides G and G + 3."""
import functools

import pytest
import torch

import tests.groups_hazards  # noqa: F401
from tests import groups_ref as GR
from tests.test_gpu_split import _rand, _to_split_padded

pytestmark = pytest.mark.gpu

NTOT, ENDS, DIM, ES_SCALE = 84, (64, 80), 768, 4.0
SEG = (NTOT, ENDS[0], ENDS[1], (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))
TOL = (2e-6, 1e-6)                       # tests/test_gpu_split.py: wd_similarity_split with the sigmoid against float64 (atol, rtol)
FILL = 7.0


@functools.lru_cache(maxsize=None)
def _plan(name):
    from wedetect_amd.groups import PromptGroups
    if name == "lvis":
        return PromptGroups.from_texts(GR.lvis_texts())
    return PromptGroups.from_sizes({"one_bin": GR.ONE_BIN, "k352": GR.K352}[name])


@functools.lru_cache(maxsize=None)
def _case(name, rows):
    """Operands and the materialised scores of (plan, rows), computed once and left unchanged."""
    from wedetect_amd import lib as L
    pg = _plan(name)
    e = _rand((rows, DIM), 401, 0.8)
    flat = torch.nn.functional.normalize(_rand((pg.P, DIM), 402), dim=-1)
    t = pg.pad_bank(flat)
    es, ts = _to_split_padded(e, ES_SCALE), L.split_weights(t)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    dense = torch.empty(rows, pg.K_pad, device="cuda")
    L.similarity_split(es, rows, ts[0], ts[1] / ES_SCALE, dense, pg.K_pad, DIM, pg.K_pad, seg=SEG, sigmoid=True, range_flag=flag)
    torch.cuda.synchronize()
    assert int(flag) == 0
    want = GR.class_amax(dense, pg.group_of.numpy())
    return dict(pg=pg, e=e, flat=flat, es=es, ts=ts, dense=dense, want=want, rows=rows)


def _out(rows, ldo):
    return torch.full((rows + 1, ldo), FILL, device="cuda")


def _fused(c, out, ldo, c0=0, kc=None, flag=None):
    from wedetect_amd import groups as PG
    pg = c["pg"]
    _, go, bf = pg.device("cuda")
    PG.group_similarity_split(c["es"], c["rows"], c["ts"][0], c["ts"][1] / ES_SCALE, pg.K_pad - c0 if kc is None else kc, DIM, go, bf, c0,
                              out, ldo, pg.G, seg=SEG, range_flag=flag, t_row=c0)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("rows", [252, 300])
@pytest.mark.parametrize("name", ["one_bin", "k352", "lvis"])
def test_fused_kernel_group_rows_and_torch_amax_agree_bit_for_bit(name, rows, pad):
    from wedetect_amd import groups as PG
    c = _case(name, rows)
    pg, want = c["pg"], c["want"]
    assert pg.K_pad == {"one_bin": 32, "k352": 352, "lvis": 2048}[name]
    G, ldo = pg.G, pg.G + pad
    _, go, bf = pg.device("cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    fused, rowsk = _out(rows, ldo), _out(rows, ldo)
    _fused(c, fused, ldo, flag=flag)
    PG.group_rows(c["dense"], rows, pg.K_pad, pg.K_pad, go, bf, 0, rowsk, ldo, G)
    torch.cuda.synchronize()
    assert int(flag) == 0
    for got in (fused, rowsk):
        assert torch.equal(got[:rows, :G], want)
        assert bool((got[:rows, G:] == FILL).all()) and bool((got[rows:] == FILL).all())      # the stride's tail and the row behind stay
    assert torch.equal(pg.class_max(c["dense"]), want)                                        # the package's own restatement
    for _ in range(2):                                                                        # no race between runs
        again = _out(rows, ldo)
        _fused(c, again, ldo)
        torch.cuda.synchronize()
        assert torch.equal(again, fused)


@pytest.mark.parametrize("name", ["k352", "lvis"])
def test_two_launches_cut_at_row_256_equal_one(name):
    from wedetect_amd import groups as PG
    c = _case(name, 300)
    pg = c["pg"]
    G = pg.G
    _, go, bf = pg.device("cuda")
    two, two_rows = _out(300, G), _out(300, G)
    _fused(c, two, G, c0=256)                                  # out of order: disjoint columns
    _fused(c, two, G, c0=0, kc=256)
    blk = c["dense"]
    PG.group_rows(blk[:, 256:].contiguous(), 300, pg.K_pad - 256, pg.K_pad - 256, go, bf, 256, two_rows, G, G)
    PG.group_rows(blk, 300, 256, pg.K_pad, go, bf, 0, two_rows, G, G)
    torch.cuda.synchronize()
    assert torch.equal(two[:300], c["want"]) and torch.equal(two_rows[:300], c["want"])
    first = int(pg.bin_first[8])                               # the first launch alone writes the classes of bins 0 .. 7 only
    part = _out(300, G)
    _fused(c, part, G, c0=0, kc=256)
    torch.cuda.synchronize()
    assert torch.equal(part[:300, :first], c["want"][:, :first]) and bool((part[:, first:] == FILL).all())


@pytest.mark.parametrize("name,rows", [("k352", 252), ("lvis", 300)])
def test_fused_kernel_against_float64(name, rows):
    """Within the similarity tests' tolerance of the float64 class maximum over the UNPADDED prompts."""
    c = _case(name, rows)
    pg = c["pg"]
    out = _out(rows, pg.G)
    _fused(c, out, pg.G)
    lvl = torch.arange(rows, device="cuda") % NTOT
    lvl = (lvl >= ENDS[0]).long() + (lvl >= ENDS[1]).long()
    sc = torch.tensor(SEG[3], device="cuda", dtype=torch.float64)[lvl][:, None]
    bi = torch.tensor(SEG[4], device="cuda", dtype=torch.float64)[lvl][:, None]
    ref = torch.sigmoid((c["e"].double() @ c["flat"].double().T) * sc + bi)
    first = pg.first_of().tolist()
    ref = torch.stack([ref[:, a:a + n].amax(dim=1) for a, n in zip(first, pg.sizes)], dim=1)
    err = (out[:rows].double() - ref).abs()
    print(f"{name} rows {rows}: max |class score - float64| {float(err.max()):.3g}")
    assert bool((err <= TOL[0] + TOL[1] * ref.abs()).all())


def test_fused_kernel_raises_its_range_flag_and_stores_nan_in_that_row_only():
    from wedetect_amd import groups as PG
    from wedetect_amd import lib as L
    rows = 64
    pg = _plan("k352")
    e = _rand((rows, DIM), 411)
    e[5, 100] = 1e6                                           # hi half = inf
    t = pg.pad_bank(torch.nn.functional.normalize(_rand((pg.P, DIM), 412), dim=-1))
    ts = L.split_weights(t)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    seg = (rows, 32, 48, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    out = _out(rows, pg.G)
    _, go, bf = pg.device("cuda")
    PG.group_similarity_split(_to_split_padded(e), rows, ts[0], ts[1], pg.K_pad, DIM, go, bf, 0, out, pg.G, pg.G, seg=seg, range_flag=flag)
    torch.cuda.synchronize()
    assert int(flag) == 1
    nan = torch.isnan(out[:rows])
    assert bool(nan[5].all()) and not bool(nan[torch.arange(rows, device="cuda") != 5].any())
    assert bool(torch.isfinite(out[:rows][~nan]).all())
    # ... which the top-k guard reports for the image
    idx = torch.empty(1, L.topk_capacity(100), dtype=torch.int32, device="cuda")
    sc, cnt = torch.empty(1, idx.shape[1], device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.topk_workspace_bytes(1, rows * pg.G, 100) + 256, dtype=torch.uint8, device="cuda")
    ws = ws[(-ws.data_ptr()) % 256:]
    L.topk_candidates(out[:rows].contiguous(), 1, rows * pg.G, 0.0, 100, idx, sc, cnt, ws)
    assert int(cnt) == -1


def test_group_rows_keeps_a_nan_and_reads_ld_strided_blocks():
    from wedetect_amd import groups as PG
    pg = _plan("k352")
    rows, ld = 19, pg.K_pad + 5
    g = torch.Generator(device="cuda").manual_seed(5)
    blk = torch.rand(rows, ld, device="cuda", generator=g)
    blk[:, pg.K_pad:] = 9.0                                   # beyond n_cls: never read
    blk[3, 40] = float("nan")                                # a row of the 32-prompt class of bin 1
    _, go, bf = pg.device("cuda")
    out = _out(rows, pg.G + 3)
    PG.group_rows(blk, rows, pg.K_pad, ld, go, bf, 0, out, pg.G + 3, pg.G)
    torch.cuda.synchronize()
    want = GR.class_amax(blk[:, :pg.K_pad], pg.group_of.numpy())
    assert bool(torch.isnan(out[3, 2])) and bool(torch.isnan(want[3, 2]))
    assert torch.equal(torch.nan_to_num(out[:rows, :pg.G], nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    assert bool((out[:rows, pg.G:] == FILL).all()) and bool((out[rows:] == FILL).all())


def test_group_entries_refuse_bad_arguments():
    from wedetect_amd import groups as PG
    from wedetect_amd import lib as L
    c = _case("k352", 252)
    pg, rows = c["pg"], 252
    G, K = pg.G, pg.K_pad
    _, go, bf = pg.device("cuda")
    out = _out(rows, G)
    es, ts, un = c["es"], c["ts"][0], c["ts"][1] / ES_SCALE
    fused = lambda **kw: PG.group_similarity_split(**{**dict(e_split=es, rows=rows, t_split=ts, unscale=un, n_cls=K, dim=DIM, group_of=go,
                                                              bin_first=bf, cls_offset=0, out=out, ldo=G, n_groups=G, seg=SEG), **kw})
    rowsk = lambda **kw: PG.group_rows(**{**dict(block=c["dense"], rows=rows, n_cls=K, ld=K, group_of=go, bin_first=bf, cls_offset=0, out=out,
                                                  ldo=G, n_groups=G), **kw})
    bad = [dict(out=out.data_ptr() + 2), dict(group_of=go.data_ptr() + 2), dict(bin_first=bf.data_ptr() + 1),       # misaligned pointers
           dict(cls_offset=8), dict(cls_offset=-32), dict(n_cls=K - 8), dict(ldo=G - 1), dict(group_of=None), dict(bin_first=None),
           dict(out=None), dict(n_groups=0)]
    for kw in bad:
        with pytest.raises(L.WedetectHipError):
            fused(**kw)
        with pytest.raises(L.WedetectHipError):
            rowsk(**kw)
    with pytest.raises(L.WedetectHipError):                   # dim % 32
        fused(e_split=_to_split_padded(c["e"][:, :48].contiguous()), dim=48)
    with pytest.raises(L.WedetectHipError):                   # operands not 16-byte aligned
        fused(e_split=es.data_ptr() + 4)
    with pytest.raises(L.WedetectHipError):
        fused(t_split=ts.data_ptr() + 8)
    with pytest.raises(L.WedetectHipError):
        rowsk(ld=K - 1)
    with pytest.raises(L.WedetectHipError):
        rowsk(block=c["dense"].data_ptr() + 2)
    with pytest.raises(L.WedetectHipError):
        rowsk(rows=0)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())                          # nothing was launched
