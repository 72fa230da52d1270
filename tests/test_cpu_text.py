"""The text tower's range cases do what tests/text_ref.py says they do (no device): the rescaled checkpoints preserve the
function in float64, every stress case breaks an fp16 hi/lo split without range management while the controls do not, and
``TextTower.encode`` refuses ids / masks that would index outside a table before it touches a device."""
import numpy as np
import pytest
import torch

from tests import text_ref as R

DIMS = ("small", "base3")


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("case", R.PRESERVING)
def test_rescaling_preserves_the_function(case, dims):
    """Power-of-two scales: what differs from ``plain`` is float64 rounding only (the stream cases scale eps with s^2, which
    is the plain model's eps in the scaled units)."""
    ref, plain = R.reference(case, dims), R.reference("plain", dims)
    assert ref["eps"] == R.BASE_EPS * R.STREAM.get(case, 1.0) ** 2 and ref["cfg"].layer_norm_eps == ref["eps"]
    d = float(np.abs(ref["bank64"] - plain["bank64"]).max())
    print(f"{dims} {case}: max |bank64 - bank64(plain)| {d:.2e}")
    assert d <= 1e-9


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("case", R.CASES)
def test_cases_stress_and_controls_do_not(case, dims):
    ref = R.reference(case, dims)
    err = R.max_err(R.bank_unscaled_split(ref["model"], ref["head"], ref["ids"], ref["mask"]), ref)
    lim = R.limit(ref)
    print(f"{dims} {case}: e32_hf {ref['e32_hf']:.2e} e_gelu {ref['e_gelu']:.2e} limit {lim:.2e} unscaled split {err:.2e} "
          f"= {err / lim:.2f} x limit")
    assert np.isfinite(ref["bank64"]).all() and ref["e32_hf"] > 0.0 and ref["e_gelu"] > 0.0
    if case in R.STRESS:
        assert not np.isfinite(err) or err > 3.0 * lim
    else:
        assert err < lim


def test_gelu_fit_is_the_documented_fit():
    """csrc/common.h: 5.5e-7 absolute over the whole line, GELU(x) -> x / 2 with a relative error below 1e-6 at 0."""
    x = torch.linspace(-12.0, 12.0, 400001, dtype=torch.float64)
    exact = 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))
    err = float((R.gelu_fit64(x) - exact).abs().max())
    assert 4.0e-7 < err < 5.6e-7, err
    t = torch.tensor([1e-6, -1e-6, 1e-3], dtype=torch.float64)
    exact = 0.5 * t * (1.0 + torch.erf(t / 2.0 ** 0.5))
    assert float(((R.gelu_fit64(t) - exact) / exact).abs().max()) < 1e-6


def test_reference_is_cached_and_padding_is_invariant_in_float64():
    a = R.reference("plain", "small")
    assert R.reference("plain", "small") is a
    b = R.reference("plain", "small", pad_to=32)
    assert b["ids"].shape == (37, 32) and torch.equal(b["ids"][:, :11], a["ids"]) and bool((b["ids"][:, 11:] == R.PAD).all())
    assert float(np.abs(a["bank64"] - b["bank64"]).max()) <= 1e-12


# ------------------------------------------------------------------------------------------------------ input validation
def _bad_inputs():
    ids = R.make_ids(5, 11)
    mask = (ids != R.PAD).long()
    big, neg = ids.clone(), ids.clone()
    big[2, 1] = R.VOCAB
    neg[4, 0] = -1
    long_ids = torch.full((2, 64), 7, dtype=torch.int64)             # 64 non-pad tokens: position id 65 in a table of 64 rows
    return {"id >= vocab": (big, mask, R.POSITIONS), "negative id": (neg, mask, R.POSITIONS),
            "position table": (long_ids, None, 64), "mask shape": (ids, mask[:, :10], R.POSITIONS)}


@pytest.mark.parametrize("what", ["id >= vocab", "negative id", "position table", "mask shape"])
def test_validate_tokens(what):
    from wedetect_amd.text import validate_tokens
    ids, mask, positions = _bad_inputs()[what]
    with pytest.raises(ValueError):
        validate_tokens(ids, mask, R.VOCAB, positions)


def test_validate_tokens_accepts_the_edges():
    from wedetect_amd.text import validate_tokens
    ids = R.make_ids(5, 11)
    ids[0, 1], ids[1, 1] = R.VOCAB - 1, 0
    validate_tokens(ids, (ids != R.PAD).long(), R.VOCAB, R.POSITIONS)
    validate_tokens(torch.full((2, 62), 7), None, R.VOCAB, 64)       # position ids reach 63, the last row
    with pytest.raises(ValueError):
        validate_tokens(torch.full((2, 63), 7), None, R.VOCAB, 64)


@pytest.mark.parametrize("what", ["id >= vocab", "negative id", "position table", "mask shape"])
def test_encode_refuses_before_touching_a_device(what):
    """A tower whose tensors live on the host has nothing to launch with: encode() must raise ValueError first."""
    from wedetect_amd.text import TextTower
    ref = R.reference("plain", "dh16")
    state = dict(ref["state"])
    ids, mask, positions = _bad_inputs()[what]
    state["embeddings.position_embeddings.weight"] = state["embeddings.position_embeddings.weight"][:positions]
    tower = TextTower(state, ref["heads"], device="cpu")
    with pytest.raises(ValueError):
        tower.encode(ids, mask)
    assert tower.range_report == {}
