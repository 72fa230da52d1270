"""Text tower against the float64 HuggingFace model (tests/text_ref.py) on checkpoints rescaled out of the window in which
an fp16 (hi, lo) pair carries an fp32 value, at full depth and length, at many names, under padding — and the tower's
range management made observable.  The bound is ``text_ref.limit``: 8 x HuggingFace's own fp32 error + 2 x what the fitted
GELU moves the bank by, both computed on the CPU from the reference class.  Every test prints what it measured first."""
import numpy as np
import pytest
import torch

from tests import text_ref as R

pytestmark = pytest.mark.gpu


def encode(ref, precision, ids=None, mask=None):
    from wedetect_amd.text import TextTower
    tower = TextTower(ref["state"], ref["heads"], precision=precision, eps=ref["eps"])
    ids = ref["ids"] if ids is None else ids
    mask = (ids != R.PAD).long() if mask is None else mask
    bank = tower.encode(ids.cuda(), mask.cuda())
    assert bank.shape == (ids.shape[0], R.OUT_DIM) and bank.dtype == torch.float32
    return tower, bank


def did(rep):
    """One phrase for what the fp16x3 tower's range management did."""
    n = len(rep["gemms"])
    sc = sorted({f"2^{int(np.log2(s))}" for s in rep["scales"].values()})
    why = sorted(set(rep["fp32"].values()))
    return (f"{n - len(rep['fp32'])}/{n} GEMMs fp16x3, {len(rep['scales'])} scaled {sc}, {len(rep['fp32'])} fp32 {why}, "
            f"{len(rep['left_fp16_range'])} inputs beyond fp16, flag {'tripped' if rep['flag_tripped'] else 'clear'}")


def check(tag, ref, lim=None):
    """Both precisions against bank64: print the line, then assert finite and within the limit."""
    lim = R.limit(ref) if lim is None else lim
    _, b32 = encode(ref, "fp32")
    tower, b16 = encode(ref, "fp16x3")
    e32, e16 = R.max_err(b32.cpu().numpy(), ref), R.max_err(b16.cpu().numpy(), ref)
    print(f"[text-range] {tag}: e32_hf {ref['e32_hf']:.2e} e_gelu {ref['e_gelu']:.2e} limit {lim:.2e} | device fp32 {e32:.2e} "
          f"fp16x3 {e16:.2e} | {did(tower.range_report)}")
    assert np.isfinite(e32) and np.isfinite(e16), f"{tag}: non-finite bank (fp32 {e32}, fp16x3 {e16})"
    assert e32 <= lim, f"{tag}: fp32 tower {e32:.3e} > limit {lim:.3e}"
    assert e16 <= lim, f"{tag}: fp16x3 tower {e16:.3e} > limit {lim:.3e}"
    norm = b16.double().norm(dim=1)
    assert float((norm - 1.0).abs().max()) <= 1e-6
    return tower


# ------------------------------------------------------------------------------------------- a. every case, both precisions
@pytest.mark.parametrize("dims", ["small", "base3"])
@pytest.mark.parametrize("case", R.CASES)
def test_every_case_within_the_limit(case, dims):
    check(f"{dims} {case} 37x11", R.reference(case, dims))


# ------------------------------------------------------------------------------------------------ b. full depth and length
@pytest.mark.parametrize("dims,n,ln", [("base12", 40, 64), ("dh16", 37, 11), ("large2", 37, 11)])
def test_full_depth_length_and_head_geometries(dims, n, ln):
    ref = R.reference("plain", dims, n, ln)
    tower = check(f"{dims} plain {n}x{ln}", ref)
    assert tower.layers == ref["cfg"].num_hidden_layers and tower.dh == ref["cfg"].hidden_size // ref["heads"]
    rep = tower.range_report                                 # an ordinary checkpoint: nothing to report, the unguarded tower's bits
    assert rep["scales"] == {} and rep["fp32"] == {} and rep["left_fp16_range"] == [] and rep["flag_tripped"] is False
    assert torch.equal(tower.encode(ref["ids"].cuda(), ref["mask"].cuda()), encode_unguarded(tower, ref["ids"], ref["mask"]))


# ---------------------------------------------------------------------------------------------------------- c. many names
@pytest.mark.parametrize("dims", ["small", "base2"])
def test_many_names(dims):
    """m = 9624 rows in the dense layers instead of 407: other tile choices, the same limit."""
    check(f"{dims} plain 1203x8", R.reference("plain", dims, 1203, 8))


# --------------------------------------------------------------------------------------------------- d. padding invariance
@pytest.mark.parametrize("case", ["plain", "ctx_hi"])
@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_padding_invariance(precision, case):
    """The same sequences padded to 11 and to 32 tokens: masked keys and pad positions must not leak, so each bank is
    within the limit of the OTHER padding's float64 reference too."""
    a, b = R.reference(case, "small"), R.reference(case, "small", pad_to=32)
    assert torch.equal(b["ids"][:, :11], a["ids"])
    _, ba = encode(a, precision)
    _, bb = encode(b, precision)
    ea, eb, ab = R.max_err(ba.cpu().numpy(), b), R.max_err(bb.cpu().numpy(), a), float((ba - bb).abs().max())
    lim = min(R.limit(a), R.limit(b))
    print(f"[text-range] small {case} {precision} padding: L=11 vs bank64(L=32) {ea:.2e}, L=32 vs bank64(L=11) {eb:.2e}, "
          f"device L=11 vs L=32 {ab:.2e}, limit {lim:.2e}")
    assert ea <= lim and eb <= lim


# ----------------------------------------------------------------------------------------------- e. the guard is observable
def encode_unguarded(tower, ids, mask):
    """The fp16x3 tower as it was issued before it had range management: every dense layer one loader-split GEMM with no
    scale and no flag.  On an ordinary checkpoint the guarded tower must return these bits."""
    from wedetect_amd import lib as L
    from wedetect_amd.text import position_ids
    w, n, ln, h = tower.w, ids.shape[0], ids.shape[1], tower.hidden
    m = n * ln
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device="cuda")

    def gemm(a, name, c, rows, k, nn, act=L.ACT_NONE, res=None):
        kw = dict(batch=1, hin=1, win=rows, cin=k, lda=a.shape[1], n=nn, ldc=c.shape[1], act=act)
        if res is not None:
            kw.update(res=res, ldres=res.shape[1])
        L.conv_gemm(a, None, w[name + ".bias"], c, w_split=L.split_weights(w[name + ".weight"]), **kw)

    ids = ids.cuda().to(torch.int32).contiguous()
    mask = mask.cuda().to(torch.int32).contiguous()
    x, y, qkv, att = f(m, h), f(m, h), f(m, 3 * h), f(m, h)
    inter = f(m, w["encoder.layer.0.intermediate.dense.weight"].shape[0])
    e = "embeddings."
    L.text_embed(ids.view(-1), position_ids(ids, tower.pad_id).view(-1), w[e + "word_embeddings.weight"],
                 w[e + "position_embeddings.weight"], w[e + "token_type_embeddings.weight"][0].contiguous(), x)
    L.layernorm_rows(x, x, w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], m, h, eps=tower.eps)
    for i in range(tower.layers):
        p = f"encoder.layer.{i}."
        gemm(x, p + "attention.self.qkv", qkv, m, h, 3 * h)
        L.attention_small(qkv, mask, att, n, ln, tower.heads, tower.dh)
        gemm(att, p + "attention.output.dense", y, m, h, h, res=x)
        L.layernorm_rows(y, y, w[p + "attention.output.LayerNorm.weight"], w[p + "attention.output.LayerNorm.bias"], m, h, eps=tower.eps)
        gemm(y, p + "intermediate.dense", inter, m, h, inter.shape[1], act=L.ACT_GELU)
        gemm(inter, p + "output.dense", x, m, inter.shape[1], h, res=y)
        L.layernorm_rows(x, x, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], m, h, eps=tower.eps)
    feats, out = f(n, tower.out_dim), f(n, tower.out_dim)
    gemm(x.view(n, ln, h)[:, 0].contiguous(), "head", feats, n, h, tower.out_dim)
    L.l2norm_rows(feats, out)
    return out


@pytest.mark.parametrize("dims", ["small", "base3"])
def test_plain_checkpoint_is_left_alone_bit_for_bit(dims, monkeypatch):
    from wedetect_amd import lib as L
    ref = R.reference("plain", dims)
    real, fp32_launches = L.conv_gemm, []

    def counting(a, w, *args, **kw):
        if kw.get("w_split") is None:
            fp32_launches.append(kw["n"])
        return real(a, w, *args, **kw)

    monkeypatch.setattr(L, "conv_gemm", counting)
    tower, bank = encode(ref, "fp16x3")
    monkeypatch.undo()
    rep = tower.range_report
    print(f"[text-range] {dims} plain report: {did(rep)}; max |input| {min(g['amax'] for g in rep['gemms']):.3g} .. "
          f"{max(g['amax'] for g in rep['gemms']):.3g}")
    assert len(rep["gemms"]) == 4 * tower.layers + 1
    assert rep["scales"] == {} and rep["fp32"] == {} and rep["left_fp16_range"] == [] and rep["flag_tripped"] is False
    assert all(g["kernel"] == "fp16x3" and g["a_scale"] == 1.0 for g in rep["gemms"])
    assert fp32_launches == []
    assert torch.equal(bank, encode_unguarded(tower, ref["ids"], ref["mask"]))


@pytest.mark.parametrize("case", ["stream_hi", "ctx_hi"])
def test_leaving_the_fp16_range_is_reported_and_handled(case):
    ref = R.reference(case, "small")
    tower, bank = encode(ref, "fp16x3")
    rep, err = tower.range_report, R.max_err(bank.cpu().numpy(), ref)
    print(f"[text-range] small {case} report: {did(rep)}; beyond fp16: {rep['left_fp16_range']}; error {err:.2e}, limit {R.limit(ref):.2e}")
    assert rep["left_fp16_range"], "no GEMM input beyond 65504: the case does not stress, or the tower does not say so"
    for name in rep["left_fp16_range"]:                      # what it did about each: a scale below 1, or the fp32 kernel
        assert rep["scales"].get(name, 1.0) < 1.0 or name in rep["fp32"]
    assert err <= R.limit(ref)
    unguarded = encode_unguarded(tower, ref["ids"], ref["mask"])
    assert not bool(torch.isfinite(unguarded).all()), "the unguarded issue order survives this case: nothing was at stake"


def test_column_spread_runs_fp32_and_low_ranges_are_scaled():
    ref = R.reference("ctx_mixed", "small")
    tower, _ = encode(ref, "fp16x3")
    rep = tower.range_report
    print(f"[text-range] small ctx_mixed report: {did(rep)}: {rep['fp32']}")
    assert rep["fp32"] == {f"encoder.layer.{i}.attention.output.dense": "column spread" for i in range(tower.layers)}
    for case in ("stream_lo", "ctx_lo", "hidden_lo"):
        tower, _ = encode(R.reference(case, "small"), "fp16x3")
        rep = tower.range_report
        print(f"[text-range] small {case} report: {did(rep)}: {rep['scales']}")
        assert rep["scales"] and all(s > 1.0 for s in rep["scales"].values()) and rep["fp32"] == {} and not rep["flag_tripped"]
    tower, _ = encode(R.reference("stream_hi", "small"), "fp32")
    assert tower.range_report["scales"] == {} and tower.range_report["fp32"] == {} and not tower.range_report["flag_tripped"]


def test_language_backbone_exposes_the_report():
    from wedetect_amd.text import XLMRobertaLanguageBackbone
    ref = R.reference("ctx_hi", "base3")                     # 12 heads: the "base" geometry; eps is the default one
    tb = XLMRobertaLanguageBackbone(model_size="base").load_state_dict({"backbone.text_model." + k: v for k, v in ref["state"].items()})
    assert tb.range_report == {}
    bank = tb.forward_ids(ref["ids"], ref["mask"])
    tower, direct = encode(ref, "fp16x3")
    assert torch.equal(bank, direct)
    assert tb.range_report["left_fp16_range"] == tower.range_report["left_fp16_range"] != []
    assert tb.range_report["scales"] == tower.range_report["scales"]


# ------------------------------------------------------------------------------------------------------------ f. validation
@pytest.mark.parametrize("what", ["id >= vocab", "negative id", "position table", "mask shape"])
def test_bad_inputs_raise_before_any_launch(what, monkeypatch):
    from wedetect_amd import lib as L
    from wedetect_amd.text import TextTower
    ref = R.reference("plain", "dh16")
    ids = ref["ids"].clone()
    mask = ref["mask"]
    state = dict(ref["state"])
    if what == "id >= vocab":
        ids[3, 1] = R.VOCAB
    elif what == "negative id":
        ids[0, 2] = -1
    elif what == "position table":                           # the longest sequence's last position id is the first row past the table
        longest = int((ids != R.PAD).sum(1).max())
        state["embeddings.position_embeddings.weight"] = state["embeddings.position_embeddings.weight"][:R.PAD + longest].clone()
    else:
        mask = mask[:, :10]
    tower = TextTower(state, ref["heads"])

    def launched(*a, **k):
        raise AssertionError("a kernel was launched on invalid input")

    for name in ("text_embed", "layernorm_rows", "conv_gemm", "attention_small", "l2norm_rows"):
        monkeypatch.setattr(L, name, launched)
    with pytest.raises(ValueError):
        tower.encode(ids.cuda(), mask.cuda())
    with pytest.raises(ValueError):
        tower.encode(ids, mask)                              # host tensors are checked where they live
