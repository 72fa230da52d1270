"""The text bank folded into the head's embedding conv (ImageTower.fold_text, $WEDETECT_FOLD_TEXT): a detect() step scores every
anchor from c2 with [K, 256] folded weights, never writes the [B, N, 768] embeddings and embeds the kept rows only.  Base at
64 x 64 (level maps 8^2 / 4^2 / 2^2, 84 anchors) and 128 x 128 (16^2 / 8^2 / 4^2, 336 anchors); both arms run on ONE tower
(``tower.fold_text`` is the switch the environment variable sets)."""

import pytest
import torch

from tests.util import to_np

pytestmark = pytest.mark.gpu

ARCH = "base"
THR = 0.0          # every positive score is a candidate: the kept lists are full whatever the synthetic checkpoint's score level
_CACHE = {}


def _packed():
    if "packed" not in _CACHE:
        from wedetect_amd import weights as W
        from wedetect_amd.pack import pack
        _CACHE["packed"] = pack(W.make_state_dict(ARCH), ARCH)
    return _CACHE["packed"]


def _tower(b, hw, precision="fp16x3", key=None):
    """Towers are shared between the tests of this module (same checkpoint); every test sets ``fold_text`` itself."""
    k = (b, hw, precision, key)
    if k not in _CACHE:
        from wedetect_amd.engine import ImageTower
        _CACHE[k] = ImageTower(ARCH, _packed(), b, hw, hw, max_classes=300, precision=precision)
    t = _CACHE[k]
    t.fold_text = True
    return t


def _images(b, hw, seed):
    from wedetect_amd import weights as W
    return torch.from_numpy(W.make_images(b, hw, hw, seed=seed)).cuda()


def _bank(k, seed=4321):
    from wedetect_amd import weights as W
    return torch.from_numpy(W.make_text_bank(k, seed=seed)).cuda()


def _meta(t):
    m = t.identity_meta()
    m[:, 7] = 1.0
    return m


def _step(t, x, bank, normalize, fold, score_thr=THR, **kw):
    t.fold_text = fold
    r = t.detect(x, bank, _meta(t), normalize_text=normalize, score_thr=score_thr, with_embed=True, **kw)
    torch.cuda.synchronize()
    k = bank.shape[0]
    return {n: v.clone() for n, v in r.items()}, t.scores.view(-1)[: t.B * t.ntot * k].view(t.B, t.ntot, k).clone()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("k", [1, 80, 81, 300])
def test_folded_scores_stay_within_the_fp16x3_budget_of_the_fp32_tower(k, normalize):
    """B = 2 @ 128.  Against an fp32 tower's scores the folded arm stays within the 1e-5 tests/test_gpu_precision.py grants the
    fp16x3 step, and is no worse than the unfolded arm by more than that arm's own distance."""
    t, ref = _tower(2, 128), _tower(2, 128, "fp32")
    x, bank = _images(2, 128, 31), _bank(k)
    _, s_ref = _step(ref, x, bank, normalize, False)
    launches = t.fold_launches
    r_f, s_f = _step(t, x, bank, normalize, True)
    assert t.fold_launches == launches + 1 and not t._embed_valid, "the folded arm did not run"
    r_u, s_u = _step(t, x, bank, normalize, False)
    assert t._embed_valid and not bool(t.range_flags.any())
    d_f, d_u = float((s_f - s_ref).abs().max()), float((s_u - s_ref).abs().max())
    print(f"K {k} normalize {normalize}: max |score - fp32 tower| folded {d_f:.3e}, unfolded {d_u:.3e}; folded vs unfolded "
          f"{float((s_f - s_u).abs().max()):.3e}")
    assert d_f <= 1e-5
    assert d_f <= 2.0 * d_u, "the fold is worse than the unfolded arm by more than that arm's own distance"


def test_level_boundary_rows_take_their_own_levels_weights_scale_and_bias():
    """B = 3 @ 64: rows off[1] - 1, off[1], off[2] - 1, off[2], ntot - 1 of every image against a float64 host computation from
    the tower's own c2 buffers (the level's folded weights, exp(logit_scale), bias), K = 81."""
    from wedetect_amd.arch import EMBED_DIM
    t = _tower(3, 64)
    x, bank = _images(3, 64, 32), _bank(81)
    for normalize in (True, False):
        _, s = _step(t, x, bank, normalize, True)
        t64 = bank.double().cpu()
        if normalize:
            t64 = t64 / t64.norm(dim=1, keepdim=True)
        rows = [t.off[1] - 1, t.off[1], t.off[2] - 1, t.off[2], t.ntot - 1]
        worst = 0.0
        for r in rows:
            l = (r >= t.off[1]) + (r >= t.off[2])
            c2 = t.unsplit(t.hc[l][1], t.sscale.get(f"h{l}.c2", 1.0)).double().cpu().view(t.B, t.nl[l], -1)
            w_e = t.P[f"head{l}.embed.w"].view(EMBED_DIM, -1).double().cpu()
            b_e = t.P[f"head{l}.embed.b"].double().cpu()
            logit = (c2[:, r - t.off[l]] @ (t64 @ w_e).T + t64 @ b_e) * float(t.lvl_scale[l]) + float(t.lvl_bias[l])
            d = float((torch.sigmoid(logit) - s[:, r].double().cpu()).abs().max())
            worst = max(worst, d)
            assert d <= 1e-5, f"row {r} (level {l}), normalize {normalize}: {d:.3e}"
        print(f"normalize {normalize}: boundary rows {rows}: max |score - float64 host| {worst:.3e}")


def test_an_image_alone_gets_the_bits_it_gets_in_a_batch_of_three():
    t1, t3 = _tower(1, 64), _tower(3, 64)
    x3, bank = _images(3, 64, 33), _bank(80)
    r3, s3 = _step(t3, x3, bank, True, True)
    for i in range(3):
        r1, s1 = _step(t1, x3[i:i + 1].contiguous(), bank, True, True)
        assert torch.equal(s1[0], s3[i]), f"image {i}: scores alone != in the batch"
        n = int(r1["count"][0])
        assert n == int(r3["count"][i]) and n > 0
        assert torch.equal(r1["anchors"][0], r3["anchors"][i]) and torch.equal(r1["embeddings"][0], r3["embeddings"][i]), \
            f"image {i}: kept embeddings alone != in the batch"


def test_kept_embeddings_are_the_rows_of_the_full_tensor_and_of_the_unfolded_arm():
    t = _tower(2, 128)
    x = _images(2, 128, 34)
    for k in (80, 300):                                    # 300: the unfolded arm writes the embeddings through the dual-format epilogue
        bank = _bank(k)
        r_f, _ = _step(t, x, bank, True, True)
        full = t.embed.clone()                             # materialised from the c2 the folded step left behind
        r_u, _ = _step(t, x, bank, True, False)
        for b in range(2):
            n = int(r_f["count"][b])
            assert n > 0
            a = r_f["anchors"][b, :n].long()
            assert torch.equal(r_f["embeddings"][b, :n], full[b, a]), f"K {k} image {b}: kept rows != rows of tower.embed"
        same = all(torch.equal(r_f[n_], r_u[n_]) for n_ in ("anchors", "labels", "count"))
        if same:
            assert torch.equal(r_f["embeddings"], r_u["embeddings"]), f"K {k}: kept embeddings differ from the unfolded arm's"
        else:                                              # a score tie broken the other way: compare anchor by anchor
            for b in range(2):
                pos = {int(v): i for i, v in enumerate(to_np(r_u["anchors"][b, : int(r_u["count"][b])]))}
                for i, v in enumerate(to_np(r_f["anchors"][b, : int(r_f["count"][b])])):
                    if int(v) in pos:
                        assert torch.equal(r_f["embeddings"][b, i], r_u["embeddings"][b, pos[int(v)]])
    # nothing kept: what the unfolded arm leaves
    bank = _bank(80)
    r_f, _ = _step(t, x, bank, True, True, score_thr=0.9999)
    r_u, _ = _step(t, x, bank, True, False, score_thr=0.9999)
    assert int(r_f["count"].max()) == 0 and int(r_u["count"].max()) == 0
    assert torch.equal(r_f["embeddings"], r_u["embeddings"]) and not bool(r_f["embeddings"].any())


@pytest.mark.parametrize("k", [80, 300])
def test_a_folded_step_returns_the_scores_and_the_order_of_the_unfolded_step(k):
    """The kept rows are re-scored by the unfolded similarity GEMM on their embeddings and re-ordered (ImageTower._kept_rows;
    K = 300: the fp16x3 similarity kernel): where both arms keep the same (image, anchor, label) triples — asserted for these
    seeded inputs, B = 2 @ 128 — every returned tensor is the unfolded arm's, bit for bit, with and without embeddings."""
    t = _tower(2, 128)
    x, bank = _images(2, 128, 37), _bank(k)
    r_f, s_f = _step(t, x, bank, True, True)
    assert not t._embed_valid, "the folded arm did not run"
    r_u, s_u = _step(t, x, bank, True, False)
    assert not torch.equal(s_f, s_u), "the arms' full score tensors are expected to differ in their last bits"
    assert torch.equal(r_f["count"], r_u["count"]) and int(r_f["count"].min()) > 1
    for b in range(2):
        n = int(r_u["count"][b])
        trip = lambda r: sorted(zip(to_np(r["anchors"][b, :n]).tolist(), to_np(r["labels"][b, :n]).tolist()))
        assert trip(r_f) == trip(r_u), f"image {b}: the arms keep different triples (a score tie decided a cut): choose another seed"
        sc = r_f["scores"][b, :n]
        assert bool((sc[:-1] >= sc[1:]).all())
    for n_ in ("bboxes", "scores", "labels", "anchors", "count", "embeddings"):
        assert torch.equal(r_f[n_], r_u[n_]), f"K {k}: {n_} differs from the unfolded arm's"
    t.fold_text = True
    r_n = t.detect(x, bank, _meta(t), normalize_text=True, score_thr=THR, with_embed=False)
    torch.cuda.synchronize()
    for n_ in ("bboxes", "scores", "labels", "anchors", "count"):
        assert torch.equal(r_n[n_], r_u[n_]), f"K {k}, no embeddings: {n_} differs from the unfolded arm's"


def test_embed_materialises_on_demand_once_per_step():
    t = _tower(2, 128)
    x, x2, bank = _images(2, 128, 35), _images(2, 128, 36), _bank(80)
    _step(t, x, bank, True, False)
    want = t.embed.clone()
    _step(t, x, bank, True, True)
    n0 = t.embed_materialised
    assert not t._embed_valid
    got = t.embed
    assert t.embed_materialised == n0 + 1 and torch.equal(got, want)
    assert torch.equal(t.embed, want) and t.embed_materialised == n0 + 1, "a second read must not launch again"
    _step(t, x2, bank, True, True)
    assert not t._embed_valid, "stale after the next step"
    got2 = t.embed.clone()
    assert t.embed_materialised == n0 + 2
    _step(t, x2, bank, True, False)
    assert torch.equal(got2, t.embed) and t.embed_materialised == n0 + 2
    # head() / features() on their own write the embeddings eagerly, as ever
    t.features(x2, num_classes=80)
    assert t._embed_valid and torch.equal(t.embed, got2)


def test_fold_cache_follows_the_bank_tensor_its_version_and_normalize():
    t = _tower(2, 128)
    x = _images(2, 128, 37)
    bank = _bank(80, seed=1)
    n0 = t.fold_launches
    _, s0 = _step(t, x, bank, True, True)
    _, s0b = _step(t, x, bank, True, True)
    assert t.fold_launches == n0 + 1 and torch.equal(s0, s0b), "the same tensor must not refold"
    _step(t, x, bank, False, True)
    assert t.fold_launches == n0 + 2, "another text handling is another fold"
    bank.copy_(_bank(80, seed=2))                           # in place: version bump
    _, s1 = _step(t, x, bank, True, True)
    assert t.fold_launches == n0 + 3 and not torch.equal(s1, s0)
    _, s1u = _step(t, x, bank, True, False)
    assert float((s1 - s1u).abs().max()) <= 1e-5, "the refold must be the fold of the NEW contents"
    ptr = bank.data_ptr()
    del bank
    bank2 = _bank(80, seed=3)                               # the allocator usually hands the freed block out again
    print(f"new bank at the freed address: {bank2.data_ptr() == ptr}")
    _, s2 = _step(t, x, bank2, True, True)
    assert t.fold_launches == n0 + 4, "a new tensor object is a new bank whatever its address"
    _, s2u = _step(t, x, bank2, True, False)
    assert float((s2 - s2u).abs().max()) <= 1e-5
    assert len(t._text_fold) <= 3


def test_a_bank_first_seen_under_capture_takes_the_unfolded_path():
    t = _tower(2, 128, key="capture")
    x, seen, fresh = _images(2, 128, 38), _bank(80, seed=5), _bank(80, seed=6)
    meta = _meta(t)
    kw = dict(normalize_text=True, score_thr=THR, with_embed=True)
    want, _ = _step(t, x, fresh.clone(), True, False)      # the unfolded result (a clone: ``fresh`` itself stays unseen)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # both arms' one-time set-up, eagerly
        for fold in (False, True):
            t.fold_text = fold
            t.detect(x, seen, meta, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    n0 = t.fold_launches
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = t.detect(x, fresh, meta, **kw)
    assert t.fold_launches == n0 and t._fold_cur is None and t._embed_valid, "no fold under capture"
    g.replay()
    torch.cuda.synchronize()
    for n in want:
        assert torch.equal(out[n], want[n]), f"{n}: captured step of an unseen bank != the unfolded step"


def test_graphed_detect_follows_a_changed_bank_through_an_in_place_refold():
    from wedetect_amd.engine import GraphedDetect
    t = _tower(2, 128, key="graphed")
    x = _images(2, 128, 39)
    meta = _meta(t)
    g = GraphedDetect(t, 80, normalize_text=True, score_thr=THR)
    assert g._fold is not None, "the captured step is the folded one"
    for seed in (7, 8, 7):
        bank = _bank(80, seed=seed)
        n0 = t.fold_launches
        out = {n: v.clone() for n, v in g(x, bank, meta).items()}
        out2 = {n: v.clone() for n, v in g(x, bank, meta).items()}     # the same bank again: no refold
        assert t.fold_launches == n0 + 1
        want, _ = _step(t, x, bank, True, True)
        for n in want:
            assert torch.equal(out[n], want[n]) and torch.equal(out2[n], want[n]), f"bank {seed}: {n} differs from the eager folded step"


def test_a_graph_survives_an_eager_step_with_a_larger_bank():
    """A folded graph captured at K = 80 points into the tower's kept-row score buffer; an eager step with K = 300 (within
    max_classes: the scores are not re-allocated, the graph stays valid) must not move it: same pointer, same generation, and
    the replay afterwards gives what it gave before."""
    from wedetect_amd.engine import GraphedDetect
    t = _tower(2, 128, key="graphed_grow")
    x, meta = _images(2, 128, 43), _meta(t)
    bank = _bank(80, seed=9)
    g = GraphedDetect(t, 80, normalize_text=True, score_thr=THR)
    assert g._fold is not None, "the captured step is the folded one"
    before = {n: v.clone() for n, v in g(x, bank, meta).items()}
    torch.cuda.synchronize()
    ptr, gen = t._kept_s.data_ptr(), t.generation
    assert t._kept_s.numel() >= 3 * t.B * t.max_out * t.max_classes
    r, _ = _step(t, x, _bank(300), True, True)             # eager, folded, the largest bank the tower takes
    assert not t._embed_valid and int(r["count"].min()) > 0
    assert t._kept_s.data_ptr() == ptr and t.generation == gen, "a buffer a captured graph points into moved"
    after = g(x, bank, meta)
    torch.cuda.synchronize()
    for n in before:
        assert torch.equal(after[n], before[n]), f"{n}: the replay after a larger eager bank differs"


def test_folded_similarity_rows_do_not_depend_on_the_ring_depth():
    """wd_fold_similarity at K = 80: 65 836 rows make 258 row tiles (the 3-stage ring of the full launches, what level 0 of the
    flagship runs), the first 300 of them alone make 2 (the 4-stage ring of every smaller test): the same bits row for row."""
    from tests.test_gpu_extents import split_cpu
    from wedetect_amd import fold as FD
    from wedetect_amd import lib as L
    rows, few, cin, n = 65536 + 300, 300, 256, 80
    g = torch.Generator(device="cuda").manual_seed(44)
    a = split_cpu(torch.randn(rows, cin, generator=g, device="cuda"))
    w = torch.randn(n, cin, generator=g, device="cuda") * cin ** -0.5
    ws = L.split_weights(w)
    bias = torch.randn(n, generator=g, device="cuda") * 0.3
    u = torch.ones(1, device="cuda")
    outs = []
    for m in (rows, few):
        c = torch.empty(m, n, device="cuda")
        FD.fold_similarity(a, ws[0], float(ws[1]), u, bias, c, batch=1, rows=m, cin=cin, n=n, c_batch_stride=m, out_scale=1.5,
                           out_bias=-0.25, sigmoid=True)
        outs.append(c)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][:few], outs[1])
    assert bool(((outs[1] > 0) & (outs[1] < 1)).all()) and float(outs[1].std()) > 0.05


def test_pipelined_steps_equal_the_in_line_steps():
    """Four detect(overlap_post=True) steps over two alternating batches: c2 must outlive the head until the post stream has
    embedded the kept rows, and the next head must wait for that."""
    t = _tower(2, 128, key="pipe")
    xs, bank = [_images(2, 128, 40), _images(2, 128, 41)], _bank(80)
    want = [_step(t, x, bank, True, True)[0] for x in xs]
    t.fold_text = True
    meta = _meta(t)
    got = []
    for i in range(4):                                     # no synchronisation between the calls
        r = t.detect(xs[i % 2], bank, meta, normalize_text=True, score_thr=THR, with_embed=True, overlap_post=True)
        with torch.cuda.stream(t.post_stream):
            got.append({n: v.clone() for n, v in r.items()})
    t.wait_post()
    torch.cuda.synchronize()
    for i, r in enumerate(got):
        for n in r:
            assert torch.equal(r[n], want[i % 2][n]), f"step {i}: {n} differs between the pipelined and the in-line step"
    lazy = t.embed.clone()                                 # materialised behind the pipelined step's head
    _step(t, xs[1], bank, True, False)
    assert torch.equal(lazy, t.embed)


def test_a_tower_that_served_per_image_banks_keeps_the_shared_path_unfolded():
    """similarity() promises image b of a per-image-bank step the bits of a shared-bank step with bank b; the per-image path is
    not folded, so from the first per-image step on the tower's shared-bank steps are the unfolded ones."""
    t = _tower(2, 128, key="per-image")
    x, bank = _images(2, 128, 42), _bank(80)
    _, s_u = _step(t, x, bank, True, False)
    _, s_f = _step(t, x, bank, True, True)
    assert not t._embed_valid
    bank3 = torch.stack([bank, bank]).contiguous()
    t.fold_text = True
    t.detect(x, bank3, _meta(t), normalize_text=True, score_thr=THR, with_embed=True)
    pi = t.scores.view(-1)[: 2 * t.ntot * 80].view(2, t.ntot, 80).clone()
    n0 = t.fold_launches
    _, s_after = _step(t, x, bank, True, True)
    assert t._embed_valid and t.fold_launches == n0, "no fold after a per-image step"
    assert torch.equal(s_after, s_u) and torch.equal(pi, s_u)
