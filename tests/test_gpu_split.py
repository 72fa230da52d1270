"""fp16x3 GEMM (wd_conv_gemm_split) parity: against float64 math and against the fp32 MFMA
kernel, over every tile configuration, conv geometry, epilogue mode and ragged size."""
import numpy as np
import pytest
import torch

from tests.util import assert_close, to_np

pytestmark = pytest.mark.gpu

ALL_CFGS = [-1, 41, 50, 51, 52, 53, 55]


def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g) * scale


def test_split_weights_layout_bit_exact():
    """wd_split_weights == numpy restatement: per row, per 8 k: [8 hi | 8 lo] fp16 of w * scale."""
    from wedetect_amd import lib as L
    for n, k in ((5, 48), (130, 24), (64, 1152)):
        w = _rand((n, k), 1, 0.05)
        buf, unscale = L.split_weights(w)
        scale = 1.0 / unscale
        assert scale == 2.0 ** round(np.log2(scale)) and float(w.abs().max()) * scale <= 2 ** 14
        k16 = (k + 15) // 16 * 16
        x = np.zeros((n, k16), np.float32)
        x[:, :k] = to_np(w) * np.float32(scale)
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
        want = np.stack([hi.reshape(n, k16 // 8, 8), lo.reshape(n, k16 // 8, 8)], axis=2).reshape(n, 2 * k16)
        n8 = (n + 7) // 8 * 8                      # round 5: rows zero-padded to whole groups of eight (DMA-fed kernels fetch 8-row groups)
        got = to_np(buf).view(np.float16).reshape(n8, 2 * k16)
        assert np.array_equal(got[:n].view(np.uint16), want.view(np.uint16)) and not got[n:].view(np.uint16).any()
        # hi + lo reproduces the scaled weight to 2^-22 relative
        rec = hi.astype(np.float64) + lo.astype(np.float64)
        assert np.max(np.abs(rec - x) / np.maximum(np.abs(x), 1e-30)) < 2.0 ** -21


def _ref64(a, w, b, act, res=None, res_alpha=1.0):
    y = a.double() @ w.double().T + b.double()
    if act == "relu":
        y = torch.relu(y)
    elif act == "silu":
        y = y * torch.sigmoid(y)
    elif act == "gelu":
        y = torch.nn.functional.gelu(y)
    if res is not None:
        y = y + res_alpha * res.double()
    return y


@pytest.mark.parametrize("cfg", ALL_CFGS)
def test_split_gemm_plain_all_tiles(cfg):
    """Ragged m / n / k (tails in every dimension), bias + GELU, then residual: vs float64."""
    from wedetect_amd import lib as L
    m, n, k = 1000, 328, 200
    a, w, b = _rand((m, k), 2), _rand((n, k), 3, k ** -0.5), _rand((n,), 4)
    ws = L.split_weights(w)
    c = torch.full((m, n), float("nan"), device="cuda")
    L.conv_gemm(a, None, b, c, batch=1, hin=1, win=m, cin=k, lda=k, n=n, ldc=n, act=L.ACT_GELU, w_split=ws,
                split_cfg=cfg)
    assert_close(f"split gelu cfg{cfg}", c, _ref64(a, w, b, "gelu"), 6e-6, 2e-6)
    r = _rand((m, n), 5)
    L.conv_gemm(a, None, b, c, batch=1, hin=1, win=m, cin=k, lda=k, n=n, ldc=n, res=r, ldres=n, res_alpha=0.5,
                w_split=ws, split_cfg=cfg)
    assert_close(f"split res cfg{cfg}", c, _ref64(a, w, b, None, r, 0.5), 6e-6, 2e-6)


def test_split_gemm_accuracy_is_fp32_level():
    """Long K, wide dynamic range: the fp16x3 error against float64 stays within 2x of the fp32 MFMA
    kernel's own error (both are accumulation-rounding dominated)."""
    from wedetect_amd import lib as L
    m, n, k = 512, 256, 4096
    g = torch.Generator(device="cuda").manual_seed(11)
    a = torch.randn(m, k, device="cuda", generator=g) * torch.exp(2.0 * torch.randn(m, k, device="cuda", generator=g))
    w = _rand((n, k), 12, k ** -0.5) * torch.exp(_rand((n, k), 13))
    b = _rand((n,), 14)
    ref = _ref64(a, w, b, None)
    c32, c16 = torch.empty(m, n, device="cuda"), torch.empty(m, n, device="cuda")
    L.conv_gemm(a, w, b, c32, batch=1, hin=1, win=m, cin=k, lda=k, n=n, ldc=n)
    L.conv_gemm(a, None, b, c16, batch=1, hin=1, win=m, cin=k, lda=k, n=n, ldc=n, w_split=L.split_weights(w))
    e32 = float((c32.double() - ref).abs().max())
    e16 = float((c16.double() - ref).abs().max())
    rms32 = float((c32.double() - ref).pow(2).mean().sqrt())
    rms16 = float((c16.double() - ref).pow(2).mean().sqrt())
    print(f"max err fp32 {e32:.3e} fp16x3 {e16:.3e}; rms fp32 {rms32:.3e} fp16x3 {rms16:.3e}; |ref| max {float(ref.abs().max()):.1f}")
    assert rms16 <= 2.0 * rms32 + 1e-7 and e16 <= 3.0 * e32 + 1e-6


@pytest.mark.parametrize("cfg", [-1, 41, 50, 51, 52])
@pytest.mark.parametrize("geom", [(3, 1, 1), (3, 2, 1), (2, 2, 0)])
def test_split_conv_geometries(cfg, geom):
    """Implicit-GEMM conv loader (3x3 s1/s2 with padding, 2x2 s2) + SiLU vs torch conv in float64."""
    from wedetect_amd import lib as L
    kk, stride, pad = geom
    b_, h, w_, ci, co = 2, 18, 22, 32, 96
    x = _rand((b_, h, w_, ci), 21)
    wt = _rand((co, ci, kk, kk), 22, (ci * kk * kk) ** -0.5)
    bias = _rand((co,), 23)
    wrow = wt.permute(0, 2, 3, 1).reshape(co, kk * kk * ci).contiguous()
    ho, wo = (h + 2 * pad - kk) // stride + 1, (w_ + 2 * pad - kk) // stride + 1
    c = torch.empty(b_ * ho * wo, co, device="cuda")
    L.conv_gemm(x, None, bias, c, batch=b_, hin=h, win=w_, cin=ci, lda=ci, kh=kk, kw=kk, stride=stride, pad=pad, n=co,
                ldc=co, act=L.ACT_SILU, w_split=L.split_weights(wrow), split_cfg=cfg)
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), bias.double(), stride=stride,
                                     padding=pad)
    ref = (ref * torch.sigmoid(ref)).permute(0, 2, 3, 1).reshape(-1, co)
    assert_close(f"split conv k{kk}s{stride} cfg{cfg}", c, ref, 6e-6, 2e-6)


def test_split_special_epilogues_match_fp32_kernel():
    """Channel-slice output (ldc > n), batch-strided rows, per-level affine + sigmoid, deconv scatter:
    the fp16x3 kernel must land every element where the fp32 kernel does."""
    from wedetect_amd import lib as L
    # similarity-style: seg affine + sigmoid into [B, ntot, K] rows
    m, n, k = 2 * 84, 80, 768
    a, w = _rand((m, k), 31), torch.nn.functional.normalize(_rand((n, k), 32), dim=-1)
    seg = (84, 64, 80, (0.7, 0.58, 0.82), (-2.6, -2.2, -1.9))
    c0, c1 = torch.zeros(m, n, device="cuda"), torch.zeros(m, n, device="cuda")
    kw = dict(batch=2, hin=1, win=84, cin=k, lda=k, n=n, ldc=n, sigmoid=True, seg=seg)
    L.conv_gemm(a, w, None, c0, **kw)
    L.conv_gemm(a, None, None, c1, w_split=L.split_weights(w), **kw)
    assert_close("split seg+sigmoid", c1, c0, 2e-6)
    # concat slice + batch stride: level rows written into a [B, 100, 64+32] buffer at column 64, row 10
    bsz, hw, cin, co = 2, 36, 64, 32
    a = _rand((bsz * hw, cin), 33)
    w, bias = _rand((co, cin), 34, 0.1), _rand((co,), 35)
    big0 = torch.zeros(bsz, 100, 96, device="cuda")
    big1 = torch.zeros(bsz, 100, 96, device="cuda")
    kw = dict(batch=bsz, hin=6, win=6, cin=cin, lda=cin, n=co, ldc=96, act=L.ACT_RELU, c_batch_stride=100)
    L.conv_gemm(a, w, bias, big0[0, 10:, 64:], **kw)
    L.conv_gemm(a, None, bias, big1[0, 10:, 64:], w_split=L.split_weights(w), **kw)
    assert_close("split slice/batch-stride", big1, big0, 2e-6)
    assert float(big1[:, :10].abs().max()) == 0 and float(big1[:, :, :64].abs().max()) == 0
    # 2x2 transposed conv scatter
    bsz, h, w_, cin, co = 2, 5, 7, 32, 16
    a = _rand((bsz * h * w_, cin), 36)
    wd, bias = _rand((4 * co, cin), 37, 0.1), _rand((4 * co,), 38)
    o0 = torch.zeros(bsz * 2 * h * 2 * w_, co, device="cuda")
    o1 = torch.zeros_like(o0)
    kw = dict(batch=bsz, hin=h, win=w_, cin=cin, lda=cin, n=4 * co, ldc=co, out_mode=L.OUT_DECONV2X2)
    L.conv_gemm(a, wd, bias, o0, **kw)
    L.conv_gemm(a, None, bias, o1, w_split=L.split_weights(wd), **kw)
    assert_close("split deconv scatter", o1, o0, 2e-6)


def test_split_gemm_rejects_bad_arguments():
    from wedetect_amd import lib as L
    a, w = _rand((64, 32), 41), _rand((32, 32), 42)
    ws = L.split_weights(w)
    c = torch.empty(64, 32, device="cuda")
    with pytest.raises(L.WedetectHipError):
        L.conv_gemm(a, None, None, c, batch=1, hin=1, win=64, cin=32, lda=32, n=32, ldc=32, w_split=(ws[0], 0.0))
    with pytest.raises(L.WedetectHipError):
        L.conv_gemm(a, None, None, c, batch=1, hin=1, win=64, cin=32, lda=32, n=32, ldc=32, w_split=ws, split_cfg=99)
    with pytest.raises(L.WedetectHipError):
        L.conv_gemm(a, None, None, c, batch=1, hin=1, win=64, cin=32, lda=32, n=32, ldc=16, w_split=ws)


def _decode_split(buf_f32_view, rows, c):
    """fp16 hi/lo groups ([8 x hi | 8 x lo] per 8 elements, stored in a float32-typed buffer) -> (hi, lo) float64."""
    raw = to_np(buf_f32_view).reshape(rows, c).view(np.float16).reshape(rows, c // 8, 2, 8)
    return raw[:, :, 0, :].reshape(rows, c).astype(np.float64), raw[:, :, 1, :].reshape(rows, c).astype(np.float64)


def _expect_halves(y32):
    hi = y32.astype(np.float16)
    lo = (y32 - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


@pytest.mark.parametrize("rows,c", [(1000, 128), (77, 512), (33, 1024), (5, 96)])
def test_layernorm_split_output_is_the_split_of_the_fp32_output(rows, c):
    from wedetect_amd import lib as L
    x, g, b = _rand((rows, c), 51, 3.0), _rand((c,), 52), _rand((c,), 53)
    y32 = torch.empty(rows, c, device="cuda")
    ys = torch.empty(rows, c, device="cuda")
    L.layernorm_rows(x, y32, g, b, rows, c)
    L.layernorm_rows(x, ys, g, b, rows, c, split=True)
    hi, lo = _decode_split(ys, rows, c)
    ehi, elo = _expect_halves(to_np(y32))
    assert np.array_equal(hi, ehi) and np.array_equal(lo, elo)
    # in place, as the engine uses it
    xi = x.clone()
    L.layernorm_rows(xi, xi, g, b, rows, c, split=True)
    assert torch.equal(xi.view(torch.int32), ys.view(torch.int32))


@pytest.mark.parametrize("cfg", [-1, 50, 51, 55, 60, 63, 64])
def test_presplit_operands_give_bit_identical_results(cfg):
    """LN(split) -> GEMM(A split, C split, GELU) -> GEMM(A split, residual) == the same chain with
    fp32 buffers and the loader-side split, bit for bit; the split C is the split of the fp32 C."""
    from wedetect_amd import lib as L
    m, c = 1000, 128
    x, g, b = _rand((m, c), 61, 2.0), _rand((c,), 62), _rand((c,), 63, 0.1)
    w1, b1 = _rand((4 * c, c), 64, c ** -0.5), _rand((4 * c,), 65, 0.1)
    w2, b2 = _rand((c, 4 * c), 66, (4 * c) ** -0.5), _rand((c,), 67, 0.1)
    ws1, ws2 = L.split_weights(w1), L.split_weights(w2)
    res = _rand((m, c), 68)
    # reference chain: fp32 intermediates
    t32, h32, o32 = torch.empty(m, c, device="cuda"), torch.empty(m, 4 * c, device="cuda"), torch.empty(m, c, device="cuda")
    L.layernorm_rows(x, t32, g, b, m, c)
    kw1 = dict(batch=1, hin=1, win=m, cin=c, lda=c, n=4 * c, ldc=4 * c, act=L.ACT_GELU)
    kw2 = dict(batch=1, hin=1, win=m, cin=4 * c, lda=4 * c, n=c, ldc=c, res=res, ldres=c)
    c1 = cfg if cfg != 55 else 50
    ref1 = {60: 51, 63: 51, 64: 51}.get(c1, c1)  # the direct-to-LDS kernels sum k in the order of the BK 16 tile
    ref2 = {60: 51, 63: 51, 64: 51}.get(cfg, cfg)
    L.conv_gemm(t32, None, b1, h32, w_split=ws1, split_cfg=ref1, **kw1)
    L.conv_gemm(h32, None, b2, o32, w_split=ws2, split_cfg=ref2, **kw2)
    # pre-split chain
    ts, hs, os_ = torch.empty(m, c, device="cuda"), torch.empty(m, 4 * c, device="cuda"), torch.empty(m, c, device="cuda")
    L.layernorm_rows(x, ts, g, b, m, c, split=True)
    L.conv_gemm(ts, None, b1, hs, w_split=ws1, split_cfg=c1, split_flags=L.SPLIT_A | L.SPLIT_C, **kw1)
    L.conv_gemm(hs, None, b2, os_, w_split=ws2, split_cfg=cfg, split_flags=L.SPLIT_A, **kw2)
    hi, lo = _decode_split(hs, m, 4 * c)
    ehi, elo = _expect_halves(to_np(h32))
    assert np.array_equal(hi, ehi) and np.array_equal(lo, elo), "split C must be the split of the fp32 C"
    assert torch.equal(os_, o32), "pre-split operands must not change a single bit of the result"


def test_presplit_downsample_conv_bit_identical():
    """LN(split) -> 2x2 stride-2 conv with the implicit-im2col loader reading fp16 hi/lo groups."""
    from wedetect_amd import lib as L
    b_, h, w_, ci, co = 2, 12, 10, 64, 128
    x, g, b = _rand((b_ * h * w_, ci), 71, 2.0), _rand((ci,), 72), _rand((ci,), 73, 0.1)
    wt, bias = _rand((co, 4 * ci), 74, (4 * ci) ** -0.5), _rand((co,), 75, 0.1)
    ws = L.split_weights(wt)
    t32, ts = torch.empty_like(x), torch.empty_like(x)
    L.layernorm_rows(x, t32, g, b, x.shape[0], ci)
    L.layernorm_rows(x, ts, g, b, x.shape[0], ci, split=True)
    kw = dict(batch=b_, hin=h, win=w_, cin=ci, lda=ci, kh=2, kw=2, stride=2, pad=0, n=co, ldc=co)
    o32 = torch.empty(b_ * (h // 2) * (w_ // 2), co, device="cuda")
    os_ = torch.empty_like(o32)
    L.conv_gemm(t32, None, bias, o32, w_split=ws, **kw)
    L.conv_gemm(ts, None, bias, os_, w_split=ws, split_flags=L.SPLIT_A, **kw)
    assert torch.equal(os_, o32)


def test_presplit_flags_are_validated():
    from wedetect_amd import lib as L
    m, k, n = 256, 128, 128
    a, w = _rand((m, k), 81), _rand((n, k), 82, 0.1)
    ws = L.split_weights(w)
    c = torch.empty(m, n, device="cuda")
    base = dict(batch=1, hin=1, win=m, cin=k, lda=k, n=n, ldc=n, w_split=ws)
    with pytest.raises(L.WedetectHipError):                       # unknown flag bit
        L.conv_gemm(a, None, None, c, split_flags=4, **base)
    with pytest.raises(L.WedetectHipError):                       # C split of a loader-split layer (fp32 A): no residual
        L.conv_gemm(a, None, None, c, split_flags=L.SPLIT_C, res=c, ldres=n, **base)
    with pytest.raises(L.WedetectHipError):                       # an fp32 copy (c2) only exists next to a split output
        L.conv_gemm(a, None, None, c, split_flags=L.SPLIT_A, c2=torch.empty_like(c), ldc2=n, **base)
    with pytest.raises(L.WedetectHipError):                       # split output rows are groups of 8 channels: ldc % 8
        L.conv_gemm(a, None, None, torch.empty(m, n + 4, device="cuda"), split_flags=L.SPLIT_A | L.SPLIT_C, res=c, ldres=n,
                    **dict(base, ldc=n + 4))
    a12, w12 = _rand((m, 12), 83), _rand((n, 12), 84)
    with pytest.raises(L.WedetectHipError):                       # groups of 8 need k % 8 == 0
        L.conv_gemm(a12, None, None, c, batch=1, hin=1, win=m, cin=12, lda=12, n=n, ldc=n, w_split=L.split_weights(w12),
                    split_flags=L.SPLIT_A)
    x = _rand((8, 12), 85)
    with pytest.raises(L.WedetectHipError):                       # LayerNorm split output needs c % 8 == 0
        L.layernorm_rows(x, torch.empty_like(x), torch.ones(12, device="cuda"), torch.zeros(12, device="cuda"), 8, 12,
                         split=True)


def test_retrieval_max_split_matches_fp32_kernel_and_shards():
    """fp16x3 retrieval (ping-pong GEMM + segmented max + atomic max) == the fp32 kernel within 2e-6 on
    ragged counts (rows of one MFMA tile belonging to two images), and class-sharded == whole bank bit for bit."""
    from wedetect_amd import lib as L
    from wedetect_amd.parallel import shard_range
    n_img, rows, k, dim = 5, 300, 10_000, 768
    g = torch.Generator(device="cuda").manual_seed(7)
    e = torch.randn(n_img, rows, dim, device="cuda", generator=g) * 1.4
    t = torch.nn.functional.normalize(torch.randn(k, dim, device="cuda", generator=g), dim=-1)
    scale = torch.randn(n_img, rows, device="cuda", generator=g) * 0.1 - 0.35
    bias = torch.randn(n_img, rows, device="cuda", generator=g) * 0.2 - 2.6
    cnt = torch.tensor([300, 211, 0, 1, 299], dtype=torch.int32, device="cuda")
    ref = torch.empty(n_img, k, device="cuda")
    L.retrieval_max(e, t, scale, bias, cnt, ref, n_img, rows, k, dim)
    out = torch.full((n_img, k), -1.0, device="cuda")
    L.retrieval_max_split(e, L.split_weights(t), scale, bias, cnt, out, n_img, rows, k, dim)
    assert float(out[2].abs().max()) == 0.0                       # an image without regions scores 0 everywhere
    assert_close("retrieval fp16x3 vs fp32", out, ref, 2e-6)
    parts = []
    for r in range(4):
        sr = shard_range(k, 4, r)
        o = torch.empty(n_img, len(sr), device="cuda")
        L.retrieval_max_split(e, L.split_weights(t[sr.start:sr.stop].contiguous()), scale, bias, cnt, o, n_img, rows,
                              len(sr), dim)
        parts.append(o)
    # every shard picks its own power-of-two weight scale: exact, so the shards reproduce the whole-bank bits
    assert torch.equal(torch.cat(parts, dim=1), out)


@pytest.mark.parametrize("n_img,rows,k,dim", [(5, 300, 10_000, 768), (3, 300, 1203, 768), (7, 20, 515, 64), (33, 7, 264, 96),
                                              (2, 301, 81, 768), (1, 64, 8, 32), (4, 129, 2049, 256), (100, 1, 40, 64), (1, 300, 1, 768)])
def test_retrieval_on_the_256_tile_kernel(n_img, rows, k, dim, monkeypatch):
    """Round 5: wd_retrieval_max_split on the 256 x 256 kernel with the operand roles swapped (bank = lane axis, region rows =
    register axis, in-register max, ONE sigmoid per (image, class)) against (a) fp64 torch on the definition of
    retrieval_metric.py:369-375, (b) the 256 x 128 ping-pong form it replaces ($WEDETECT_RETR_P8=0), (c) itself on a
    class-sharded bank (bit for bit).  Shapes: class counts that are no multiple of 8 (padded split buffers), images of
    7 / 20 rows (many images per 64-row wave block), 301 rows (every wave block straddles), ragged and zero counts."""
    import os
    from wedetect_amd import lib as L
    from wedetect_amd.parallel import shard_range
    g = torch.Generator(device="cuda").manual_seed(11 + n_img)
    e = torch.randn(n_img, rows, dim, device="cuda", generator=g) * (1.4 * (768 / dim) ** 0.5)
    t = torch.nn.functional.normalize(torch.randn(k, dim, device="cuda", generator=g), dim=-1)
    scale = torch.randn(n_img, rows, device="cuda", generator=g) * 0.1 - 0.35
    bias = torch.randn(n_img, rows, device="cuda", generator=g) * 0.2 - 2.6
    cnt = torch.randint(0, rows + 1, (n_img,), device="cuda", generator=g, dtype=torch.int32)
    cnt[0] = rows
    if n_img > 2:
        cnt[1], cnt[2] = 0, 1
    ts = L.split_weights(t)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    monkeypatch.setenv("WEDETECT_RETR_P8", "1")
    out = torch.full((n_img, k), -1.0, device="cuda")
    L.retrieval_max_split(e, ts, scale, bias, cnt, out, n_img, rows, k, dim, range_flag=flag)
    monkeypatch.setenv("WEDETECT_RETR_P8", "0")
    old = torch.full((n_img, k), -1.0, device="cuda")
    L.retrieval_max_split(e, ts, scale, bias, cnt, old, n_img, rows, k, dim)
    monkeypatch.setenv("WEDETECT_RETR_P8", "1")
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    lg = torch.einsum("nrd,kd->nrk", e.double(), t.double()) * scale.double().exp()[..., None] + bias.double()[..., None]
    valid = torch.arange(rows, device="cuda")[None, :] < cnt[:, None]
    ref = torch.where(valid[..., None], torch.sigmoid(lg), torch.zeros((), dtype=torch.float64, device="cuda")).amax(dim=1)
    assert_close("retrieval p8 vs fp64", out, ref, 3e-6)
    assert_close("retrieval p8 vs the ping-pong form", out, old, 1e-6)
    assert torch.equal(out == 0, ref == 0)                             # images / rows without regions: exactly 0
    parts = []
    for r in range(3):
        sr = shard_range(k, 3, r)
        o = torch.empty(n_img, len(sr), device="cuda")
        if len(sr):                                                    # a bank of fewer classes than ranks leaves shards empty
            L.retrieval_max_split(e, L.split_weights(t[sr.start:sr.stop].contiguous()), scale, bias, cnt, o, n_img, rows, len(sr), dim)
        parts.append(o)
    assert torch.equal(torch.cat(parts, dim=1), out)
    # the range guard: one embedding beyond the fp16 maximum raises the flag
    e2 = e.clone()
    e2[0, 0, 0] = 1e5
    L.retrieval_max_split(e2, ts, scale, bias, cnt, out, n_img, rows, k, dim, range_flag=flag)
    assert int(flag.item()) == 1


def test_bank_scorer_falls_back_to_fp32_when_an_embedding_leaves_the_fp16_range():
    from wedetect_amd.parallel import BankScorer
    g = torch.Generator(device="cuda").manual_seed(3)
    n, r, d, k = 4, 300, 768, 640
    e = torch.randn(n, r, d, device="cuda", generator=g)
    bank = torch.nn.functional.normalize(torch.randn(k, d, device="cuda", generator=g), dim=-1)
    sc, bi = torch.full((n, r), -0.4, device="cuda"), torch.full((n, r), -2.0, device="cuda")
    cnt = torch.full((n,), r, dtype=torch.int32, device="cuda")
    fast, exact = BankScorer(bank), BankScorer(bank, "fp32")
    assert fast.precision == "fp16x3"
    assert_close("fp16x3 scorer vs fp32 scorer", fast(e, cnt, sc, bi), exact(e, cnt, sc, bi), 3e-6)
    assert not fast.overflowed
    e[1, 5, 7] = 9e4
    with pytest.warns(UserWarning, match="fp16 range"):
        got = fast(e, cnt, sc, bi)
    assert fast.overflowed and fast.precision == "fp32" and torch.equal(got, exact(e, cnt, sc, bi))


@pytest.mark.parametrize("m,n,k", [(264, 320, 64), (1000, 256, 96), (520, 512, 128), (2048, 768, 1024), (304, 40, 160), (257, 320, 64), (8, 8, 32)])
@pytest.mark.parametrize("mode", ["gelu_csplit", "residual"])
def test_p8_kernel_bit_identical_to_the_128_tile_kernel(m, n, k, mode):
    """cfg 64 (256 x 256 tiles, K tiles of 32, counted LDS-DMA waits, two staggered wave groups) against cfg 60 on
    ragged shapes: partial row / column tiles (clamped DMA rows), K tiles 2 (prologue only), 3 (first tail form) and
    more, both epilogues.  Same per-accumulator MFMA order => the same bits."""
    from wedetect_amd import lib as L
    x, g, b = _rand((m, k), 91, 2.0), _rand((k,), 92), _rand((k,), 93, 0.1)
    w, bias = _rand((n, k), 94, k ** -0.5), _rand((n,), 95, 0.1)
    ws = L.split_weights(w)
    xs = torch.empty(m, k, device="cuda")
    L.layernorm_rows(x, xs, g, b, m, k, split=True)
    kw = dict(batch=1, hin=1, win=m, cin=k, lda=k, n=n, ldc=n)
    if mode == "gelu_csplit":
        kw.update(act=L.ACT_GELU)
        flags = L.SPLIT_A | L.SPLIT_C
    else:
        kw.update(res=_rand((m, n), 96), ldres=n)
        flags = L.SPLIT_A
    outs = []
    for cfg in (60, 64):
        c = torch.full((m, n), 7.0, device="cuda")
        if m % 8 or n % 8:                                        # the 256-tile kernel clamps DMA row groups of 8 as a whole
            if cfg == 64:
                with pytest.raises(L.WedetectHipError):
                    L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=cfg, split_flags=flags, **kw)
                return
        L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=cfg, split_flags=flags, **kw)
        outs.append(c)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"max|d| {float((outs[0] - outs[1]).abs().max())}"
    for _ in range(3):                                            # no race between runs
        c = torch.full((m, n), 7.0, device="cuda")
        L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=64, split_flags=flags, **kw)
        assert torch.equal(c.view(torch.int32), outs[1].view(torch.int32))


def _to_split_padded(x, scale=1.0):
    """fp32 rows -> fp16 hi/lo groups of x * scale in a buffer padded to a multiple of eight rows (wd_split_weights_padded)."""
    from wedetect_amd import lib as L
    rows, k = x.shape
    out = torch.empty(L.LIB.wd_split_weights_bytes(rows, k), dtype=torch.uint8, device="cuda")
    L.check(L.LIB.wd_split_weights_padded(x.data_ptr(), rows, k, float(scale), out.data_ptr(), L.stream_ptr()), "split")
    return out


@pytest.mark.parametrize("b_,ntot,ends,k_cls", [(2, 84, (64, 80), 80), (3, 84, (64, 80), 256), (1, 525, (400, 500), 1203), (5, 84, (64, 80), 7),
                                                (2, 8400, (6400, 8000), 1203)])
@pytest.mark.parametrize("sigmoid", [True, False])
def test_similarity_split_matches_float64_and_the_fp32_kernel(b_, ntot, ends, k_cls, sigmoid):
    """wd_similarity_split (round 6): region x text logits on the fp16x3 256 x 256 kernel — per-level scale / bias by
    row % anchors, sigmoid, ragged class counts (7, 1203: scalar stores, partial column tiles), row counts that are no multiple of
    eight (the padded buffer's spare rows are never stored), an embedding split scale folded into the unscale — against float64
    and against the fp32-MFMA similarity launch of wd_conv_gemm."""
    from wedetect_amd import lib as L
    rows, dim = b_ * ntot, 768
    e = _rand((rows, dim), 301, 0.8)
    t = torch.nn.functional.normalize(_rand((k_cls, dim), 302), dim=-1)
    seg = (ntot, ends[0], ends[1], (1.9, 1.6, 2.2), (-2.6, -2.2, -1.9))
    es_scale = 4.0
    es = _to_split_padded(e, es_scale)
    ts = L.split_weights(t)
    out = torch.full((rows + 3, k_cls), 7.0, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.similarity_split(es, rows, ts[0], ts[1] / es_scale, out, k_cls, dim, k_cls, seg=seg, sigmoid=sigmoid, range_flag=flag)
    ref32 = torch.empty(rows, k_cls, device="cuda")
    L.conv_gemm(e, t, None, ref32, batch=1, hin=1, win=rows, cin=dim, lda=dim, n=k_cls, ldc=k_cls, sigmoid=sigmoid, seg=seg)
    torch.cuda.synchronize()
    assert int(flag) == 0 and bool((out[rows:] == 7.0).all())
    lvl = (torch.arange(rows, device="cuda") % ntot)
    lvl = (lvl >= ends[0]).long() + (lvl >= ends[1]).long()
    sc = torch.tensor(seg[3], device="cuda", dtype=torch.float64)[lvl][:, None]
    bi = torch.tensor(seg[4], device="cuda", dtype=torch.float64)[lvl][:, None]
    ref = (e.double() @ t.double().T) * sc + bi
    if sigmoid:
        ref = torch.sigmoid(ref)
    tol = 2e-6 if sigmoid else 2e-5
    assert_close("similarity_split vs float64", out[:rows], ref, tol, 1e-6)
    assert_close("similarity_split vs fp32 kernel", out[:rows], ref32, tol, 1e-6)


def test_similarity_split_raises_its_range_flag_and_rejects_bad_arguments():
    from wedetect_amd import lib as L
    rows, dim, k_cls = 64, 768, 16
    e = _rand((rows, dim), 311)
    e[5, 100] = 1e6                                           # hi half = inf
    t = torch.nn.functional.normalize(_rand((k_cls, dim), 312), dim=-1)
    ts = L.split_weights(t)
    out = torch.empty(rows, k_cls, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    seg = (rows, 32, 48, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    L.similarity_split(_to_split_padded(e), rows, ts[0], ts[1], out, k_cls, dim, k_cls, seg=seg, range_flag=flag)
    torch.cuda.synchronize()
    assert int(flag) == 1
    with pytest.raises(L.WedetectHipError):                   # ldo < classes
        L.similarity_split(_to_split_padded(e), rows, ts[0], ts[1], out, k_cls, dim, k_cls - 1, seg=seg)
    with pytest.raises(L.WedetectHipError):                   # dim % 32
        L.similarity_split(_to_split_padded(e[:, :48].contiguous()), rows, ts[0], ts[1], out, k_cls, 48, k_cls, seg=seg)


@pytest.mark.parametrize("m,n,k", [(272, 320, 16), (1008, 256, 32), (528, 512, 48), (2048, 768, 1024), (304, 48, 160), (144, 272, 64), (16, 16, 96),
                                   (264, 320, 64)])
@pytest.mark.parametrize("mode", ["gelu_csplit", "residual"])
def test_p4_kernel_bit_identical_to_the_128_tile_kernel(m, n, k, mode):
    """cfg 66 (128 x 256 tiles, four waves, two workgroups per CU, three-slot ring of k16 steps, one barrier per phase)
    against cfg 60: partial row / column tiles (DMA row groups of 16 clamped as a whole), 1, 2, 3 (tail forms only), 4, 6,
    10 and 64 K steps, both epilogues (the residual one prefetches).  Same per-accumulator MFMA order => same bits."""
    from wedetect_amd import lib as L
    x, g, b = _rand((m, k), 191, 2.0), _rand((k,), 192), _rand((k,), 193, 0.1)
    w, bias = _rand((n, k), 194, k ** -0.5), _rand((n,), 195, 0.1)
    ws = L.split_weights(w)
    xs = torch.empty(m, k, device="cuda")
    L.layernorm_rows(x, xs, g, b, m, k, split=True)
    kw = dict(batch=1, hin=1, win=m, cin=k, lda=k, n=n, ldc=n)
    if mode == "gelu_csplit":
        kw.update(act=L.ACT_GELU)
        flags = L.SPLIT_A | L.SPLIT_C
    else:
        kw.update(res=_rand((m, n), 196), ldres=n)
        flags = L.SPLIT_A
    outs = []
    for cfg in (60, 66):
        c = torch.full((m, n), 7.0, device="cuda")
        if (m % 16 or n % 16) and cfg == 66:
            with pytest.raises(L.WedetectHipError):
                L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=cfg, split_flags=flags, **kw)
            return
        L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=cfg, split_flags=flags, **kw)
        outs.append(c)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"max|d| {float((outs[0] - outs[1]).abs().max())}"
    for _ in range(3):                                            # no race between runs
        c = torch.full((m, n), 7.0, device="cuda")
        L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=66, split_flags=flags, **kw)
        assert torch.equal(c.view(torch.int32), outs[1].view(torch.int32))
    if mode == "residual":                                        # in place over the residual, as the engine runs pwconv2
        c = kw["res"].clone()
        kw2 = dict(kw, res=c)
        L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=66, split_flags=flags, **kw2)
        assert torch.equal(c.view(torch.int32), outs[1].view(torch.int32))
        c = kw["res"].clone()
        L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=64 if k % 32 == 0 and m % 8 == 0 and n % 8 == 0 else 60, split_flags=flags, **dict(kw, res=c))
        assert torch.equal(c.view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("m,n,k,mode", [(51200, 512, 2048, "residual"), (51200, 2048, 512, "gelu_csplit"), (65536 + 8, 256, 96, "residual"),
                                         (66000, 512, 32, "gelu_csplit"), (131064, 256, 64, "residual"),
                                         (40008, 1024, 64, "gelu_csplit"), (70000, 768, 96, "residual")])   # round 4: gangs of 4 / of 1 with three column tiles
def test_p8_persistent_kernel_bit_identical_and_repeatable(m, n, k, mode):
    """cfg 65: one workgroup per CU walks a contiguous range of (tile, K tile) units; tiles cut between two CUs are
    started by one, parked in the workspace, and finished by the other from the parked accumulators.  Same MFMA chain
    per accumulator => bit-identical to the 128-tile kernel; the flag words return to zero, so launches repeat; K tile
    counts 1, 2, 3 and many; partial last row tile."""
    from wedetect_amd import lib as L
    x = _rand((m, k), 101, 1.5)
    xs = torch.empty(m, k, device="cuda")
    L.layernorm_rows(x, xs, torch.ones(k, device="cuda"), torch.zeros(k, device="cuda"), m, k, split=True) if k <= 512 else None
    if k > 512:                                                   # wide rows: split through the weight splitter (scale 1)
        buf = torch.empty(L.LIB.wd_split_weights_bytes(m, k), dtype=torch.uint8, device="cuda")
        L.check(L.LIB.wd_split_weights(x.data_ptr(), m, k, 1.0, buf.data_ptr(), L.stream_ptr()), "wd_split_weights")
        xs = buf.view(torch.float32).view(-1, k)[:m]
    w, bias = _rand((n, k), 104, k ** -0.5), _rand((n,), 105, 0.1)
    ws = L.split_weights(w)
    kw = dict(batch=1, hin=1, win=m, cin=k, lda=k, n=n, ldc=n)
    if mode == "gelu_csplit":
        kw.update(act=L.ACT_GELU)
        flags = L.SPLIT_A | L.SPLIT_C
    else:
        kw.update(res=_rand((m, n), 106), ldres=n)
        flags = L.SPLIT_A
    ref = torch.full((m, n), 7.0, device="cuda")
    L.conv_gemm(xs, None, bias, ref, w_split=ws, split_cfg=60, split_flags=flags, **kw)
    park = torch.zeros(L.p8_workspace_bytes() // 4, dtype=torch.float32, device="cuda")
    for rep in range(3):
        c = torch.full((m, n), 7.0, device="cuda")
        L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=65, split_flags=flags, workspace=park, **kw)
        torch.cuda.synchronize()
        assert torch.equal(c.view(torch.int32), ref.view(torch.int32)), f"run {rep}: max|d| {float((c - ref).abs().max())}"
        assert int(park[:1024].view(torch.int32).abs().max()) == 0, "flag words must be zero again after a launch"
    with pytest.raises(L.WedetectHipError):                       # no workspace
        L.conv_gemm(xs, None, bias, c, w_split=ws, split_cfg=65, split_flags=flags, **kw)
    small = torch.full((2048, n), 7.0, device="cuda")
    with pytest.raises(L.WedetectHipError):                       # fewer tiles than CUs: ranges shorter than a tile would chain
        L.conv_gemm(xs[:2048], None, bias, small, w_split=ws, split_cfg=65, split_flags=flags, workspace=park,
                    **dict(kw, win=2048, **({"res": kw["res"][:2048]} if "res" in kw else {})))


# ------------------------------------------------------------------------------------------ pre-split implicit-GEMM (split_gemm_conv.hip)
def _to_split(x2d: torch.Tensor) -> torch.Tensor:
    """fp32 rows -> the fp16 hi/lo group format a WD_SPLIT_C producer writes, in a buffer of the same byte size
    (wd_split_weights with scale 1: the same two roundings as the GEMM loader's split)."""
    from wedetect_amd import lib as L
    rows, k = x2d.shape
    assert k % 16 == 0
    out = torch.empty(rows, k, dtype=torch.float32, device="cuda")
    L.check(L.LIB.wd_split_weights(x2d.contiguous().data_ptr(), rows, k, 1.0, out.data_ptr(), L.stream_ptr()), "split")
    return out


def _from_split(buf: torch.Tensor) -> torch.Tensor:
    """hi + lo of a split-format buffer as float64 (for checking a WD_SPLIT_C output against its fp32 twin)."""
    rows, k = buf.shape
    h = buf.contiguous().view(torch.float16).view(rows, k // 8, 2, 8)
    return (h[:, :, 0].double() + h[:, :, 1].double()).reshape(rows, k)


CONV_PP_CASES = [
    # name,            b, h,  w,  cin, n,   k, s, act,  res,   form
    ("3x3 c128 40x40", 3, 40, 40, 128, 128, 3, 1, "silu", True, "dual"),
    ("3x3 c128 s2",    2, 40, 40, 128, 128, 3, 2, "relu", False, "split_slice"),
    ("3x3 c64 n64",    2, 26, 30, 64,  64,  3, 1, "silu", True, "f32"),
    ("3x3 c256 20x20", 2, 20, 20, 256, 256, 3, 1, "silu", False, "split"),
    ("3x3 ragged",     1, 13, 17, 32,  96,  3, 1, "silu", True, "split"),
    ("1x1 wide n",     2, 9,  31, 256, 768, 1, 1, "none", False, "batch_stride"),
    ("1x1 dual",       2, 12, 20, 384, 128, 1, 1, "silu", False, "dual"),
    ("2x2 s2",         2, 16, 12, 64,  128, 2, 2, "none", False, "f32"),
]


def _same(got: torch.Tensor, ref: torch.Tensor, exact: bool, what: str) -> None:
    """bit-identical, or — for the row-sharing 3 x 3 kernel of round 4, whose K order is (kh, chunk, kw) instead of (kh, kw,
    ci) — equal up to the rounding of an fp32 sum of up to 4608 products taken in another order: 3e-5 of the tensor's rms
    (measured on the benchmark layers, scripts/conv3_bench.py: 3e-6 ... 1e-5)"""
    if exact:
        assert torch.equal(got, ref), what
    else:
        rms = float(ref.double().pow(2).mean().sqrt())
        err = float((got.double() - ref.double()).abs().max())
        assert err <= 3e-5 * max(rms, 1e-30) + 1e-7, f"{what}: max|d| {err:.3e} vs rms {rms:.3e}"


@pytest.mark.parametrize("case", CONV_PP_CASES, ids=[c[0] for c in CONV_PP_CASES])
@pytest.mark.parametrize("cfg", [-1, 73, 74, 75, 78])
def test_conv_pp_bit_identical_to_loader_split(case, cfg):
    """The LDS-DMA implicit-GEMM kernel on pre-split activations (every output form: fp32, fp16 hi/lo, both at once,
    channel slices, batch-strided rows; fp32 residual) against the register-staged loader-split kernel on the fp32 twin
    of the same tensor: same halves, same K order, same epilogue arithmetic -> the same bits."""
    from wedetect_amd import lib as L
    name, b_, h, w_, ci, co, kk, stride, act, with_res, form = case
    conv3 = kk == 3 and stride == 1                               # production (and cfg 75) run the row-sharing kernel there
    if cfg in (75, 78) and not conv3:
        pytest.skip("cfg 75 / 78 = the 3 x 3 / stride 1 kernel (production K loop / the in-step K loop of round 4)")
    exact = not (conv3 and cfg in (-1, 75, 78))
    pad = 1 if kk == 3 else 0
    ho, wo = (h + 2 * pad - kk) // stride + 1, (w_ + 2 * pad - kk) // stride + 1
    m = b_ * ho * wo
    x = _rand((b_ * h * w_, ci), 41)
    wrow = _rand((co, kk * kk * ci), 42, (ci * kk * kk) ** -0.5)
    bias = _rand((co,), 43)
    res = _rand((m, co), 44) if with_res else None
    ws = L.split_weights(wrow)
    actc = dict(none=L.ACT_NONE, relu=L.ACT_RELU, silu=L.ACT_SILU)[act]
    geo = dict(batch=b_, hin=h, win=w_, cin=ci, lda=ci, kh=kk, kw=kk, stride=stride, pad=pad, n=co, act=actc, res=res,
               ldres=co if with_res else 0, res_alpha=0.625, w_split=ws)
    xs = _to_split(x)
    if form == "batch_stride":
        rows = ho * wo + 7
        ref = torch.zeros(b_, rows, co, device="cuda")
        got = torch.zeros(b_, rows, co, device="cuda")
        L.conv_gemm(x, None, bias, ref[0, 3:], ldc=co, c_batch_stride=rows, **geo)
        L.conv_gemm(xs, None, bias, got[0, 3:], ldc=co, c_batch_stride=rows, split_flags=L.SPLIT_A, split_cfg=cfg if cfg > 0 else -1, **geo)
        _same(got, ref, exact, f"{name} cfg{cfg}: batch-strided fp32 output differs")
        return
    ldc = co + 64 if form == "split_slice" else co
    ref = torch.zeros(m, ldc, device="cuda")
    L.conv_gemm(x, None, bias, ref[:, ldc - co:], ldc=ldc, **geo)
    if form == "f32":
        got = torch.zeros(m, ldc, device="cuda")
        L.conv_gemm(xs, None, bias, got, ldc=ldc, split_flags=L.SPLIT_A, split_cfg=cfg if cfg > 0 else (75 if conv3 else 70), **geo)
        _same(got, ref, exact, f"{name} cfg{cfg}: fp32 output differs from the loader-split kernel")
        return
    got = torch.zeros(m, ldc, device="cuda")
    c2 = torch.full((m, co), float("nan"), device="cuda") if form == "dual" else None
    L.conv_gemm(xs, None, bias, got[:, ldc - co:], ldc=ldc, split_flags=L.SPLIT_A | L.SPLIT_C, split_cfg=cfg if cfg > 0 else -1,
                c2=c2, ldc2=co if c2 is not None else 0, **geo)
    want = _to_split(ref[:, ldc - co:].contiguous())                  # split of the loader-split kernel's fp32 output
    if exact:
        assert torch.equal(got[:, ldc - co:].contiguous().view(torch.int32), want.view(torch.int32)), f"{name} cfg{cfg}: hi/lo output differs"
    else:
        _same(_from_split(got[:, ldc - co:].contiguous()), ref[:, ldc - co:].double(), False, f"{name} cfg{cfg}: hi/lo output")
    assert float(got[:, : ldc - co].abs().max()) == 0.0 if ldc > co else True
    if c2 is not None:
        _same(c2, ref, exact, f"{name} cfg{cfg}: fp32 copy differs")
        if not exact:                                                # the two outputs of one launch are the same values
            assert float((_from_split(got[:, ldc - co:].contiguous()) - c2.double()).abs().max()) <= 1e-6 * float(c2.abs().max())


@pytest.mark.parametrize("b_,h,w_,ci,co", [(1, 2, 2, 16, 8), (2, 5, 3, 32, 64), (3, 40, 40, 128, 128), (1, 80, 80, 64, 256), (2, 19, 23, 48, 136),
                                            (32, 20, 20, 256, 64)])
@pytest.mark.parametrize("cfg", [77, 78, 79])
def test_conv3_row_sharing_kernel_against_fp64(b_, h, w_, ci, co, cfg):
    """split_conv3_kernel (cfg 75): every border case of the register-masked left / right padding and the zero-page top /
    bottom padding — maps narrower than a tile row group, tiles that start and end mid-row and mid-image, a 2 x 2 map where
    every pixel touches every border — against a float64 convolution of the same (hi + lo) operands."""
    from wedetect_amd import lib as L
    x = _rand((b_ * h * w_, ci), 71)
    wrow = _rand((co, 9 * ci), 72, (9 * ci) ** -0.5)
    bias = _rand((co,), 73)
    ws = L.split_weights(wrow)
    xs = _to_split(x)
    got = torch.empty(b_ * h * w_, co, device="cuda")
    L.conv_gemm(xs, None, bias, got, batch=b_, hin=h, win=w_, cin=ci, lda=ci, kh=3, kw=3, stride=1, pad=1, n=co, ldc=co,
                act=L.ACT_NONE, w_split=ws, split_flags=L.SPLIT_A, split_cfg=cfg)
    xd = _from_split(xs).view(b_, h, w_, ci).permute(0, 3, 1, 2)
    wd = wrow.double().view(co, 3, 3, ci).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(xd, wd, bias.double(), padding=1).permute(0, 2, 3, 1).reshape(b_ * h * w_, co)
    err = float((got.double() - ref).abs().max())
    assert err < 2e-5 * float(ref.abs().max()), f"max|d| {err:.3e}"


@pytest.mark.parametrize("b_,h,w_,ci,co,splits", [(2, 5, 3, 32, 64, 1), (3, 40, 40, 128, 128, 1), (1, 80, 80, 64, 256, 1), (2, 19, 23, 48, 136, 1),
                                                   (4, 20, 20, 256, 256, 2), (2, 20, 20, 256, 64, 2), (1, 33, 31, 16, 64, 1), (2, 20, 20, 512, 256, 3)])
def test_conv3_staggered_k_loop_bit_identical_to_in_step(b_, h, w_, ci, co, splits):
    """Round 6: the two-row-group staggered K loop (cfg 77; one barrier per read phase and per MFMA phase, DMA of stage s + 2 issued in
    the tap-1 / tap-2 phases, border lanes reading the zero staged row) and the twelve-wave producer / consumer kernel (cfg 79: four
    DMA waves beside eight free-running MFMA waves, the ds_reads pinned into the MFMA stream by inline asm) run the same MFMA chain per accumulator as the in-step loop of round 4 (cfg 78): every
    output form equal bit for bit, with and without the fixed split-K."""
    from wedetect_amd import lib as L
    m = b_ * h * w_
    x = _rand((m, ci), 171)
    wrow = _rand((co, 9 * ci), 172, (9 * ci) ** -0.5)
    bias = _rand((co,), 173)
    res = _rand((m, co), 174)
    ws = L.split_weights(wrow)
    xs = _to_split(x)
    geo = dict(batch=b_, hin=h, win=w_, cin=ci, lda=ci, kh=3, kw=3, stride=1, pad=1, n=co, ldc=co, act=L.ACT_SILU, res=res, ldres=co,
               res_alpha=0.5, w_split=ws)
    if splits > 1:
        geo.update(workspace=torch.empty(splits * m * co + 64, device="cuda"), k_splits=splits)
    out = {}
    for cfg in (77, 78, 79):
        c = torch.full((m, co), float("nan"), device="cuda")
        cs = torch.full((m, co), float("nan"), device="cuda")
        c2 = torch.full((m, co), float("nan"), device="cuda")
        L.conv_gemm(xs, None, bias, c, split_flags=L.SPLIT_A, split_cfg=cfg, **geo)
        L.conv_gemm(xs, None, bias, cs, split_flags=L.SPLIT_A | L.SPLIT_C, split_cfg=cfg, c2=c2, ldc2=co, **geo)
        out[cfg] = (c, cs, c2)
    for cfg in (77, 79):
        for a, b, what in zip(out[cfg], out[78], ("fp32", "hi/lo", "fp32 twin")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"cfg {cfg}: {what}"
    assert bool(torch.isfinite(out[77][0]).all())


def test_conv_pp_split_k_deconv_and_c_only_split():
    """(a) two-way split-K (the 20 x 20 maps): equal to the loader-split kernel's split-K result; (b) the 2x2 transposed
    conv scatter written as fp16 hi/lo groups; (c) WD_SPLIT_C without WD_SPLIT_A (fp32 activations in, split out)."""
    from wedetect_amd import lib as L
    b_, h, w_, ci, co = 2, 20, 20, 256, 256
    x = _rand((b_ * h * w_, ci), 51)
    wrow = _rand((co, 9 * ci), 52, (9 * ci) ** -0.5)
    bias = _rand((co,), 53)
    res = _rand((b_ * h * w_, co), 54)
    ws = L.split_weights(wrow)
    work = torch.empty(2 * b_ * h * w_ * co + 64, device="cuda")
    geo = dict(batch=b_, hin=h, win=w_, cin=ci, lda=ci, kh=3, kw=3, stride=1, pad=1, n=co, ldc=co, act=L.ACT_SILU, res=res,
               ldres=co, res_alpha=0.3, w_split=ws, workspace=work, k_splits=2)
    ref = torch.empty(b_ * h * w_, co, device="cuda")
    L.conv_gemm(x, None, bias, ref, **geo)
    got = torch.empty_like(ref)
    c2 = torch.empty_like(ref)
    L.conv_gemm(_to_split(x), None, bias, got, split_flags=L.SPLIT_A | L.SPLIT_C, c2=c2, ldc2=co, split_cfg=70, **geo)   # tap-per-stage kernel
    assert torch.equal(c2, ref) and torch.equal(got.view(torch.int32), _to_split(ref).view(torch.int32))
    # production: the row-sharing kernel with the same two-way split (another K order: rounding noise of an fp32 sum)
    got3, c23 = torch.empty_like(ref), torch.empty_like(ref)
    L.conv_gemm(_to_split(x), None, bias, got3, split_flags=L.SPLIT_A | L.SPLIT_C, c2=c23, ldc2=co, **geo)
    _same(c23, ref, False, "conv3 split-K fp32 copy")
    _same(_from_split(got3), ref.double(), False, "conv3 split-K hi/lo output")
    # (b) deconv scatter, hi/lo output into the first third of a concat buffer
    b_, h, w_, ci, co = 2, 5, 7, 64, 32
    a = _rand((b_ * h * w_, ci), 55)
    wd, bias = _rand((4 * co, ci), 56, 0.1), _rand((4 * co,), 57)
    wsd = L.split_weights(wd)
    kw = dict(batch=b_, hin=h, win=w_, cin=ci, lda=ci, n=4 * co, ldc=3 * co, out_mode=L.OUT_DECONV2X2, w_split=wsd)
    ref = torch.zeros(b_ * 4 * h * w_, 3 * co, device="cuda")
    L.conv_gemm(a, None, bias, ref, **kw)
    got = torch.zeros_like(ref)
    L.conv_gemm(_to_split(a), None, bias, got, split_flags=L.SPLIT_A | L.SPLIT_C, **kw)
    assert torch.equal(got[:, :co].contiguous().view(torch.int32), _to_split(ref[:, :co].contiguous()).view(torch.int32))
    assert float(got[:, co:].abs().max()) == 0.0
    # (c) loader-split kernel writing hi/lo (C-only split): 1x1, ReLU, channel slice
    m, ci, co = 5000, 512, 128
    a, w, bias = _rand((m, ci), 58), _rand((co, ci), 59, ci ** -0.5), _rand((co,), 60)
    wsw = L.split_weights(w)
    ref = torch.zeros(m, 3 * co, device="cuda")
    kw = dict(batch=1, hin=1, win=m, cin=ci, lda=ci, n=co, ldc=3 * co, act=L.ACT_RELU, w_split=wsw)
    L.conv_gemm(a, None, bias, ref[:, co:], **kw)
    got = torch.zeros_like(ref)
    L.conv_gemm(a, None, bias, got[:, co:], split_flags=L.SPLIT_C, **kw)
    assert torch.equal(got[:, co:2 * co].contiguous().view(torch.int32), _to_split(ref[:, co:2 * co].contiguous()).view(torch.int32))
    assert float(got[:, :co].abs().max()) == 0.0 and float(got[:, 2 * co:].abs().max()) == 0.0
    assert float((_from_split(got[:, co:2 * co].contiguous()) - ref[:, co:2 * co].double()).abs().max()) < 1e-6


@pytest.mark.parametrize("m", [128, 1280, 128 * 257])
@pytest.mark.parametrize("hid_scale", [1.0, 0.25])
def test_fused_mlp_bit_identical_to_the_two_kernel_chain(m, hid_scale):
    """wd_mlp_fused_split (LN rows -> pwconv1 -> GELU -> split -> pwconv2 -> + residual in one kernel, hidden tensor in LDS)
    against the chain the engine otherwise runs: wd_conv_gemm_split(SPLIT_A | SPLIT_C, GELU) into a hidden buffer, then
    wd_conv_gemm_split(SPLIT_A, residual in place).  Same halves, same K order, same epilogue arithmetic: the same bits,
    with and without a range scale on the hidden activations; repeated launches agree (no race on the LDS operands)."""
    from wedetect_amd import lib as L
    c, h = 128, 512
    x0, g, b = _rand((m, c), 301, 2.0), _rand((c,), 302), _rand((c,), 303, 0.1)
    w1, b1 = _rand((h, c), 304, c ** -0.5), _rand((h,), 305, 0.1)
    w2, b2 = _rand((c, h), 306, h ** -0.5), _rand((c,), 307, 0.1)
    ws1, ws2 = L.split_weights(w1), L.split_weights(w2)
    ws2s = (ws2[0], ws2[1] / hid_scale)
    xs = torch.empty(m, c, device="cuda")
    L.layernorm_rows(x0, xs, g, b, m, c, split=True)
    hid = torch.empty(m, h, device="cuda")
    want = x0.clone()
    L.conv_gemm(xs, None, b1, hid, w_split=ws1, batch=1, hin=1, win=m, cin=c, lda=c, n=h, ldc=h, act=L.ACT_GELU,
                split_flags=L.SPLIT_A | L.SPLIT_C, c_split_scale=hid_scale)
    L.conv_gemm(hid, None, b2, want, w_split=ws2s, batch=1, hin=1, win=m, cin=h, lda=h, n=c, ldc=c, res=want, ldres=c,
                split_flags=L.SPLIT_A)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for _ in range(3):
        got = x0.clone()
        L.mlp_fused(xs, m, c, h, ws1, b1, ws2s, b2, got, hid_scale=hid_scale, range_flag=flag)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"max|d| {float((got - want).abs().max())}"
    assert int(flag.item()) == 0
    # and it is a real MLP: against float64
    y = torch.nn.functional.layer_norm(x0.double(), (c,), g.double(), b.double(), 1e-6)
    ref = x0.double() + torch.nn.functional.gelu(y @ w1.double().T + b1.double()) @ w2.double().T + b2.double()
    assert float((got.double() - ref).abs().max()) < 2e-5 * float(ref.abs().max())


@pytest.mark.parametrize("c,m", [(512, 128), (512, 128 * 9), (512, 51200), (512, 128 * 257), (256, 128), (256, 128 * 37), (256, 128 * 300)])
@pytest.mark.parametrize("hid_scale", [1.0, 0.25])
def test_fused_mlp_wide_bit_identical_to_the_two_kernel_chain(c, m, hid_scale):
    """wd_mlp_fused_wide (round 4: the block MLP of the 256 / 512-channel stages as one kernel — output tile in the four
    waves' accumulators, hidden chunks of 128 columns through LDS, weights fragment-major straight from global memory) against
    the two launches the engine otherwise runs (the 256 x 256 kernel twice).  Same halves, same K order per output, same
    epilogue arithmetic: the same bits, with and without a range scale; repeated launches agree."""
    from wedetect_amd import lib as L
    h = 4 * c
    x0, g, b = _rand((m, c), 311, 2.0), _rand((c,), 312), _rand((c,), 313, 0.1)
    w1, b1 = _rand((h, c), 314, c ** -0.5), _rand((h,), 315, 0.1)
    w2, b2 = _rand((c, h), 316, h ** -0.5), _rand((c,), 317, 0.1)
    ws1, ws2 = L.split_weights(w1), L.split_weights(w2)
    ws2s = (ws2[0], ws2[1] / hid_scale)
    wf1 = (L.mlp_wide_pack(ws1[0], h, c), ws1[1])
    wf2 = (L.mlp_wide_pack(ws2[0], c, h), ws2s[1])
    xs = torch.empty(m, c, device="cuda")
    L.layernorm_rows(x0, xs, g, b, m, c, split=True)
    hid = torch.empty(m, h, device="cuda")
    want = x0.clone()
    L.conv_gemm(xs, None, b1, hid, w_split=ws1, batch=1, hin=1, win=m, cin=c, lda=c, n=h, ldc=h, act=L.ACT_GELU,
                split_flags=L.SPLIT_A | L.SPLIT_C, c_split_scale=hid_scale)
    L.conv_gemm(hid, None, b2, want, w_split=ws2s, batch=1, hin=1, win=m, cin=h, lda=h, n=c, ldc=c, res=want, ldres=c,
                split_flags=L.SPLIT_A)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    # with the park workspace and more row blocks than CUs: the persistent form (a row block cut between two CUs)
    park = torch.zeros(L.p8_workspace_bytes() // 4, dtype=torch.float32, device="cuda")
    for ws in (None, park):
        for _ in range(3):
            got = x0.clone()
            L.mlp_fused_wide(xs, m, c, h, wf1, b1, wf2, b2, got, hid_scale=hid_scale, range_flag=flag, workspace=ws)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"workspace {ws is not None}: max|d| {float((got - want).abs().max())}"
            assert int(park[:1024].view(torch.int32).abs().max()) == 0, "flag words must be zero again after a launch"
    assert int(flag.item()) == 0
    if m <= 128 * 37:                                             # and it is a real MLP: against float64
        y = torch.nn.functional.layer_norm(x0.double(), (c,), g.double(), b.double(), 1e-6)
        ref = x0.double() + torch.nn.functional.gelu(y @ w1.double().T + b1.double()) @ w2.double().T + b2.double()
        assert float((got.double() - ref).abs().max()) < 2e-5 * float(ref.abs().max())


def test_fused_mlp_wide_refuses_other_shapes_and_flags_overflow():
    from wedetect_amd import lib as L
    c, h, m = 256, 1024, 256
    assert L.mlp_wide_supported(m, c, h) and L.mlp_wide_supported(m, 512, 2048)
    assert not L.mlp_wide_supported(m + 8, c, h) and not L.mlp_wide_supported(m, 128, 512) and not L.mlp_wide_supported(m, 1024, 4096)
    xs = torch.zeros(m, c, device="cuda")
    ws1, ws2 = L.split_weights(_rand((h, c), 1, 0.1)), L.split_weights(_rand((c, h), 2, 0.1))
    wf1, wf2 = (L.mlp_wide_pack(ws1[0], h, c), ws1[1]), (L.mlp_wide_pack(ws2[0], c, h), ws2[1])
    b1, b2, x = torch.zeros(h, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(m, c, device="cuda")
    with pytest.raises(L.WedetectHipError):
        L.mlp_fused_wide(xs, m + 8, c, h, wf1, b1, wf2, b2, x)
    with pytest.raises(L.WedetectHipError):
        L.mlp_fused_wide(xs, m, 128, 512, wf1, b1, wf2, b2, x)
    with pytest.raises(L.WedetectHipError):
        L.mlp_wide_pack(ws1[0], h + 8, c)
    b1big = torch.full((h,), 1e6, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.mlp_fused_wide(xs, m, c, h, wf1, b1big, wf2, b2, x, range_flag=flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1


def test_fused_mlp_refuses_other_shapes_and_flags_overflow():
    from wedetect_amd import lib as L
    c, h, m = 128, 512, 256
    assert L.mlp_fused_supported(m, c, h) and not L.mlp_fused_supported(m + 8, c, h) and not L.mlp_fused_supported(m, 256, 1024)
    xs = torch.zeros(m, c, device="cuda")
    ws1, ws2 = L.split_weights(_rand((h, c), 1, 0.1)), L.split_weights(_rand((c, h), 2, 0.1))
    b1, b2, x = torch.zeros(h, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(m, c, device="cuda")
    with pytest.raises(L.WedetectHipError):
        L.mlp_fused(xs, m + 8, c, h, ws1, b1, ws2, b2, x)
    with pytest.raises(L.WedetectHipError):
        L.mlp_fused(xs, m, 256, 1024, ws1, b1, ws2, b2, x)
    # hidden activations beyond the fp16 range: the halves overflow to inf, the accumulators of GEMM 2 go non-finite, flag set
    b1big = torch.full((h,), 1e6, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.mlp_fused(xs, m, c, h, ws1, b1big, ws2, b2, x, range_flag=flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1


@pytest.mark.parametrize("b,h,w,c", [(2, 40, 40, 512), (1, 20, 20, 1024), (3, 13, 21, 256), (1, 9, 7, 64)])
def test_layernorm_folded_into_the_gemm(b, h, w, c):
    """Round 5: dwconv -> LayerNorm -> pwconv1 (mm_backbone.py:113-118) with the LayerNorm FOLDED into the GEMM.  (a)
    wd_dwconv7_stats writes the depthwise output bit-identically to wd_dwconv7 followed by a split, and its per-block partials
    finalise to the row mean / rstd of an fp64 LayerNorm; (b) the GEMM on W' = W gamma with the (mean, rstd, u, v) epilogue equals
    fp64 GELU(W LN(d) + b) to the accuracy of the fp16x3 kernels, and the LayerNorm-kernel path to 2e-5 of the output's scale."""
    from wedetect_amd import lib as L
    g = torch.Generator(device="cuda").manual_seed(c + h)
    rows, n = b * h * w, 4 * c
    x = torch.randn(rows, c, device="cuda", generator=g) * 2.0 + 0.7
    w7 = torch.randn(49, c, device="cuda", generator=g) * 0.15
    bdw = torch.randn(c, device="cuda", generator=g) * 0.1
    gam = torch.rand(c, device="cuda", generator=g) + 0.5
    bet = torch.randn(c, device="cuda", generator=g) * 0.1
    w1 = torch.randn(n, c, device="cuda", generator=g) * c ** -0.5
    b1 = torch.randn(n, device="cuda", generator=g) * 0.1
    # ---- (a) the depthwise kernel with statistics
    d = torch.empty_like(x)
    L.dwconv7(x, w7, bdw, d, b, h, w, c)
    ds = torch.empty_like(x)
    part = torch.empty(c // 32, rows, 2, device="cuda")
    L.dwconv7_stats(x, w7, bdw, ds, part, b, h, w, c, scale=4.0)
    assert torch.equal(ds.view(torch.int32), _to_split(d * 4.0).view(torch.int32)), "split depthwise output differs from dwconv + split"
    stats = torch.empty(rows, 2, device="cuda")
    L.ln_stats_finalize(part, stats, rows, c)
    d64 = d.double()
    mu, var = d64.mean(dim=1), d64.var(dim=1, unbiased=False)
    assert_close("row mean", stats[:, 0], mu, 1e-6, 2e-6)
    assert_close("row rstd", stats[:, 1], 1.0 / torch.sqrt(var + 1e-6), 0, 3e-6)
    # ---- (b) the folded GEMM
    w1g = (w1.double() * gam.double()[None, :]).float()
    u = w1g.double().sum(dim=1).float()
    v = (w1.double() @ bet.double() + b1.double()).float()
    ws = L.split_weights(w1g)
    ws = (ws[0], ws[1] / 4.0)                                         # the operand carries d * 4
    got = torch.empty(rows, n, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.conv_gemm(ds, None, v, got, w_split=ws, batch=1, hin=1, win=rows, cin=c, lda=c, n=n, ldc=n, act=L.ACT_GELU,
                split_flags=L.SPLIT_A | L.SPLIT_C, ln_stats=stats, ln_u=u, range_flag=flag)
    y64 = torch.nn.functional.layer_norm(d64, (c,), gam.double(), bet.double(), 1e-6)
    ref = torch.nn.functional.gelu(y64 @ w1.double().T + b1.double())
    out = _from_split(got)
    scale = float(ref.abs().max())
    assert int(flag.item()) == 0
    assert_close("folded LayerNorm + pwconv1 + GELU vs fp64", out, ref, 1e-5 * scale)
    # the path it replaces: LayerNorm kernel (split output) -> GEMM
    ys = torch.empty_like(x)
    L.layernorm_rows(d, ys, gam, bet, rows, c, split=True)
    old = torch.empty(rows, n, device="cuda")
    L.conv_gemm(ys, None, b1, old, w_split=L.split_weights(w1), batch=1, hin=1, win=rows, cin=c, lda=c, n=n, ldc=n, act=L.ACT_GELU,
                split_flags=L.SPLIT_A | L.SPLIT_C)
    assert_close("folded vs LayerNorm-kernel path", out, _from_split(old), 2e-5 * scale)
    # refusals: the fold exists in the plain pre-split C-split epilogue only
    with pytest.raises(L.WedetectHipError):
        L.conv_gemm(ds, None, v, got, w_split=ws, batch=1, hin=1, win=rows, cin=c, lda=c, n=n, ldc=n, split_flags=L.SPLIT_A, ln_stats=stats, ln_u=u)
    with pytest.raises(L.WedetectHipError):
        L.conv_gemm(d, w1g, v, got, batch=1, hin=1, win=rows, cin=c, lda=c, n=n, ldc=n, ln_stats=stats, ln_u=u)


@pytest.mark.parametrize("ratio", [1.0, 30.0, 1000.0])
def test_layernorm_fold_error_grows_with_mean_over_std(ratio):
    """the fold centres AFTER the contraction (rstd (W'd - mean u)), so rows whose mean is large against their spread
    lose |mean| / std x 2^-22 of relative accuracy to cancellation.  Measured here on rows of mean ``ratio`` x std: within
    (4 + ratio) x 2^-21 of the output's scale — at the fp16x3 kernels' own level up to a ratio of ~64, which is where
    ImageTower.calibrate() stops folding a block (engine.FOLD_MAX_MEAN_OVER_STD; test_gpu_precision covers the gate)."""
    from wedetect_amd import lib as L
    g = torch.Generator(device="cuda").manual_seed(7)
    rows, c = 2048, 256
    n = 4 * c
    d = torch.randn(rows, c, device="cuda", generator=g) + ratio          # std 1, mean `ratio`
    gam = torch.rand(c, device="cuda", generator=g) + 0.5
    bet = torch.randn(c, device="cuda", generator=g) * 0.1
    w1 = torch.randn(n, c, device="cuda", generator=g) * c ** -0.5
    b1 = torch.randn(n, device="cuda", generator=g) * 0.1
    d64 = d.double()
    stats = torch.stack([d64.mean(dim=1), 1.0 / torch.sqrt(d64.var(dim=1, unbiased=False) + 1e-6)], dim=1).float().contiguous()
    w1g = (w1.double() * gam.double()[None, :]).float()
    u = w1g.double().sum(dim=1).float()
    v = (w1.double() @ bet.double() + b1.double()).float()
    sc = 2.0 ** (9 - int(np.floor(np.log2(float(d.abs().max())))))       # as calibrate() would place the operand
    ws = L.split_weights(w1g)
    got = torch.empty(rows, n, device="cuda")
    L.conv_gemm(_to_split(d * sc), None, v, got, w_split=(ws[0], ws[1] / sc), batch=1, hin=1, win=rows, cin=c, lda=c, n=n, ldc=n,
                act=L.ACT_NONE, split_flags=L.SPLIT_A | L.SPLIT_C, ln_stats=stats, ln_u=u)
    ref = torch.nn.functional.layer_norm(d64, (c,), gam.double(), bet.double(), 1e-6) @ w1.double().T + b1.double()
    err = float((_from_split(got).double() - ref).abs().max()) / float(ref.abs().max())
    assert err <= (4.0 + ratio) * 2.0 ** -21, (ratio, err)
    if ratio >= 1000.0:
        assert err > 1e-5, "the bound is loose here: revisit FOLD_MAX_MEAN_OVER_STD"


@pytest.mark.parametrize("m", [128, 128 * 37, 128 * 300])
@pytest.mark.parametrize("hid_scale", [1.0, 0.25])
def test_fused_mlp_wide_with_the_layernorm_folded_is_bit_identical_to_the_two_launch_fold(m, hid_scale):
    """Round 6: wd_mlp_fused_wide_ln — the 256-channel one-kernel block MLP reading the RAW depthwise output and applying the
    block's LayerNorm in its hidden epilogue (rstd (W'd - mean u) + v) — against the two launches of the round-5 fold (the 256 x 256
    kernel with WdConvGemm.ln_stats / ln_u, then pwconv2 + residual): the same bits, tile form and persistent form, repeated
    launches; and against float64 LayerNorm -> MLP."""
    from wedetect_amd import lib as L
    c, h = 256, 1024
    d = _rand((m, c), 411, 2.0) + 0.7
    x0 = _rand((m, c), 412, 1.5)
    gam, bet = torch.rand(c, device="cuda") + 0.5, _rand((c,), 413, 0.1)
    w1, b1 = _rand((h, c), 414, c ** -0.5), _rand((h,), 415, 0.1)
    w2, b2 = _rand((c, h), 416, h ** -0.5), _rand((c,), 417, 0.1)
    d64 = d.double()
    stats = torch.stack([d64.mean(dim=1), 1.0 / torch.sqrt(d64.var(dim=1, unbiased=False) + 1e-6)], dim=1).float().contiguous()
    w1g = (w1.double() * gam.double()[None, :]).float()
    u = w1g.double().sum(dim=1).float()
    v = (w1.double() @ bet.double() + b1.double()).float()
    dsc = 4.0
    ds = _to_split(d * dsc)
    ws1, ws2 = L.split_weights(w1g), L.split_weights(w2)
    ws1s, ws2s = (ws1[0], ws1[1] / dsc), (ws2[0], ws2[1] / hid_scale)
    hid = torch.empty(m, h, device="cuda")
    want = x0.clone()
    L.conv_gemm(ds, None, v, hid, w_split=ws1s, batch=1, hin=1, win=m, cin=c, lda=c, n=h, ldc=h, act=L.ACT_GELU,
                split_flags=L.SPLIT_A | L.SPLIT_C, c_split_scale=hid_scale, ln_stats=stats, ln_u=u)
    L.conv_gemm(hid, None, b2, want, w_split=ws2s, batch=1, hin=1, win=m, cin=h, lda=h, n=c, ldc=c, res=want, ldres=c,
                split_flags=L.SPLIT_A)
    wf1, wf2 = (L.mlp_wide_pack(ws1[0], h, c), ws1s[1]), (L.mlp_wide_pack(ws2[0], c, h), ws2s[1])
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    park = torch.zeros(L.p8_workspace_bytes() // 4, dtype=torch.float32, device="cuda")
    for ws in (None, park):
        for _ in range(3):
            got = x0.clone()
            L.mlp_fused_wide_ln(ds, m, c, h, wf1, v, u, stats, wf2, b2, got, hid_scale=hid_scale, range_flag=flag, workspace=ws)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"workspace {ws is not None}: max|d| {float((got - want).abs().max())}"
            assert int(park[:1024].view(torch.int32).abs().max()) == 0
    assert int(flag.item()) == 0
    if m <= 128 * 37:
        y = torch.nn.functional.layer_norm(d64, (c,), gam.double(), bet.double(), 1e-6)
        ref = x0.double() + torch.nn.functional.gelu(y @ w1.double().T + b1.double()) @ w2.double().T + b2.double()
        assert float((got.double() - ref).abs().max()) < 2e-5 * float(ref.abs().max())
    with pytest.raises(L.WedetectHipError):
        L.mlp_fused_wide_ln(ds, m, 512, 2048, wf1, v, u, stats, wf2, b2, got)


# ---- every activation through every pre-split kernel's epilogue, both output forms
ACT_FORM_SHAPE = (272, 256, 64)       # the smallest m, n, k all five kernels accept (cfg 66: m % 16, n % 256; cfg 64: k % 32); 272 = 256 + 16: a ragged row tile
ACT_FORM_SPLIT_SCALE = 1.0


@pytest.fixture(scope="module")
def act_form_data():
    """Inputs of test_presplit_kernels_every_activation_and_form, the float64 reference per activation, and the first output seen
    per (activation, form) — what every other configuration's output must equal bit for bit.  Built once, never changed."""
    from wedetect_amd import lib as L
    m, n, k = ACT_FORM_SHAPE
    a, w, b = _rand((m, k), 301), _rand((n, k), 302, k ** -0.5), _rand((n,), 303)
    return dict(xs=_to_split(a), ws=L.split_weights(w), b=b, ref={act: _ref64(a, w, b, act) for act in ("none", "relu", "silu", "gelu")},
                first={})


@pytest.mark.parametrize("cfg", [51, 60, 63, 64, 66])
@pytest.mark.parametrize("form", ["f32", "csplit"])
@pytest.mark.parametrize("act", ["none", "relu", "silu", "gelu"])
def test_presplit_kernels_every_activation_and_form(act, form, cfg, act_form_data):
    """The activation dispatch of every plain pre-split kernel (register-staged 128 x 128, direct-to-LDS, ping-pong, 256 x 256,
    128 x 256), fp32 rows and fp16 hi/lo (C-split) output: N(0, 1) data with a bias, on which the four activations differ by
    O(1) on a large share of the elements, so an arm that instantiates the wrong one fails the float64 comparison; and the
    kernels run the same MFMA order per accumulator, so for one activation and form all five give the same bits."""
    from wedetect_amd import lib as L
    d = act_form_data
    m, n, k = ACT_FORM_SHAPE
    c = torch.full((m, n), float("nan"), device="cuda")
    flags = L.SPLIT_A | (L.SPLIT_C if form == "csplit" else 0)
    L.conv_gemm(d["xs"], None, d["b"], c, batch=1, hin=1, win=m, cin=k, lda=k, n=n, ldc=n, w_split=d["ws"], split_cfg=cfg, split_flags=flags,
                act=dict(none=L.ACT_NONE, relu=L.ACT_RELU, silu=L.ACT_SILU, gelu=L.ACT_GELU)[act], c_split_scale=ACT_FORM_SPLIT_SCALE)
    got = _from_split(c) / ACT_FORM_SPLIT_SCALE if form == "csplit" else c
    assert_close(f"{act} {form} cfg{cfg}", got, d["ref"][act], 6e-6, 2e-6)
    first_cfg, first = d["first"].setdefault((act, form), (cfg, c))
    assert torch.equal(c.view(torch.int32), first.view(torch.int32)), f"{act} {form}: cfg {cfg} differs from cfg {first_cfg}"


@pytest.mark.parametrize("cfg", [70, 75])
@pytest.mark.parametrize("form", ["f32", "csplit"])
def test_conv3x3_kernels_gelu(form, cfg):
    """GELU through the 3 x 3 kernels' (row, 8 channels) epilogue — the tap-per-stage kernel (cfg 70) and the row-sharing one
    (cfg 75); CONV_PP_CASES has none / relu / silu only — against a float64 convolution of the same (hi + lo) operands:
    several row tiles with a ragged last one, n no multiple of the column tile."""
    from wedetect_amd import lib as L
    b_, h, w_, ci, co = 2, 19, 23, 48, 136
    x = _rand((b_ * h * w_, ci), 311)
    wrow = _rand((co, 9 * ci), 312, (9 * ci) ** -0.5)
    bias = _rand((co,), 313)
    xs = _to_split(x)
    c = torch.full((b_ * h * w_, co), float("nan"), device="cuda")
    L.conv_gemm(xs, None, bias, c, batch=b_, hin=h, win=w_, cin=ci, lda=ci, kh=3, kw=3, stride=1, pad=1, n=co, ldc=co, act=L.ACT_GELU,
                w_split=L.split_weights(wrow), split_flags=L.SPLIT_A | (L.SPLIT_C if form == "csplit" else 0), split_cfg=cfg)
    xd = _from_split(xs).view(b_, h, w_, ci).permute(0, 3, 1, 2)
    wd = wrow.double().view(co, 3, 3, ci).permute(0, 3, 1, 2)
    ref = torch.nn.functional.gelu(torch.nn.functional.conv2d(xd, wd, bias.double(), padding=1)).permute(0, 2, 3, 1).reshape(b_ * h * w_, co)
    assert_close(f"3x3 gelu {form} cfg{cfg}", _from_split(c) if form == "csplit" else c, ref, 6e-6, 2e-6)
