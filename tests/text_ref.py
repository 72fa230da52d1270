"""Float64 reference of the text tower and the rescaled checkpoints its range tests run (CPU only).

The model is HuggingFace's ``XLMRobertaModel`` (the class the reference instantiates, mm_backbone.py:355) with the seeded
weights of tests/test_gpu_text.py, followed by the reference's head + normalisation (mm_backbone.py:384-386).  A *case*
rescales that checkpoint with POWERS OF TWO — exact in fp32 and float64 — so that a tensor the fp16x3 GEMMs split into fp16
(hi, lo) pairs leaves the window in which such a pair carries an fp32 value: below ~2^-3 the lo half is a subnormal fp16
number, above 65504 the hi half is inf.  The ``stream_*`` and ``ctx_*`` cases preserve the function; ``hidden_lo`` changes it
(through the GELU) — the float64 model of the same weights is the reference either way.

``limit(ref)`` = 8 * e32_hf + 2 * e_gelu bounds the device bank's error against the float64 bank:
  e32_hf  the error of HuggingFace's own fp32 evaluation of the same weights (8 x: the margin tests/test_gpu_tune_kernels.py
          ``check_grad`` gives a device fp32-level evaluation over a host one — summation order and MFMA K-chunking differ);
  e_gelu  what the project's fitted GELU (csrc/common.h ``wd_gelu``, 5.5e-7 absolute, deliberate and deterministic) moves the
          float64 bank by.
Both are computed here, on the CPU, from the reference class: neither depends on the code under test."""
from __future__ import annotations

import copy

import numpy as np
import torch

VOCAB, POSITIONS, OUT_DIM, PAD = 1000, 80, 768, 1
BASE_EPS = 1e-5

DIMS = {
    "small": dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256),
    "dh16": dict(hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256),
    "base2": dict(hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072),
    "base3": dict(hidden_size=768, num_hidden_layers=3, num_attention_heads=12, intermediate_size=3072),
    "base12": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072),
    "large2": dict(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096),
}

STREAM = {"stream_lo": 2.0 ** -13, "stream_hi": 2.0 ** 15}
CTX = {"ctx_lo": (2.0 ** -13, 2.0 ** -13), "ctx_hi": (2.0 ** 17, 2.0 ** 17), "ctx_mixed": (2.0 ** -13, 8.0)}   # (even, odd) channels
STRESS = ("stream_lo", "stream_hi", "ctx_lo", "ctx_hi", "ctx_mixed", "hidden_lo")
CONTROLS = ("plain", "sharp")
CASES = CONTROLS + STRESS
PRESERVING = tuple(STREAM) + tuple(CTX)          # same function as ``plain`` in exact arithmetic

_REF = {}                                        # (case, dims, n, ln) -> reference(): computed once, shared, left unchanged


def eps_of(case: str) -> float:
    return BASE_EPS * STREAM.get(case, 1.0) ** 2


def make_ids(n, ln, vocab=VOCAB, seed=4):
    """tests/test_gpu_text.py::_ids: <s> + 1 .. ln - 2 tokens + </s>, padded with 1."""
    g = np.random.default_rng(seed)
    ids = np.full((n, ln), PAD, np.int64)
    for i in range(n):
        k = int(g.integers(1, ln - 1))
        ids[i, 0] = 0
        ids[i, 1:1 + k] = g.integers(4, vocab, k)
        ids[i, 1 + k] = 2
    return torch.from_numpy(ids)


def repad(ids: torch.Tensor, ln: int) -> torch.Tensor:
    out = torch.full((ids.shape[0], ln), PAD, dtype=ids.dtype)
    out[:, :ids.shape[1]] = ids
    return out


def build(case: str, dims, seed: int = 3):
    """(cfg, model, head): the seeded fp32 HuggingFace model of tests/test_gpu_text.py::_hf, rescaled for ``case``."""
    from transformers import XLMRobertaConfig, XLMRobertaModel
    if case not in CASES:
        raise KeyError(case)
    dims = DIMS[dims] if isinstance(dims, str) else dims
    torch.manual_seed(seed)
    cfg = XLMRobertaConfig(type_vocab_size=1, pad_token_id=PAD, layer_norm_eps=eps_of(case), hidden_act="gelu",
                           hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=VOCAB,
                           max_position_embeddings=POSITIONS, **dims)
    model = XLMRobertaModel(cfg, add_pooling_layer=False).eval()
    head = torch.nn.Linear(cfg.hidden_size, OUT_DIM)
    with torch.no_grad():
        for n_, p_ in model.named_parameters():            # trained-like spread instead of the 0.02-std init
            if p_.dim() == 2 and "embeddings" not in n_:
                p_.mul_(2.5)
        if case in STREAM:
            s = STREAM[case]
            emb = model.embeddings
            for t in (emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight,
                      emb.LayerNorm.weight, emb.LayerNorm.bias):
                t.mul_(s)
            for ly in model.encoder.layer:
                for mod in (ly.attention.output.dense, ly.output.dense, ly.attention.output.LayerNorm, ly.output.LayerNorm):
                    mod.weight.mul_(s)
                    mod.bias.mul_(s)
                for mod in (ly.attention.self.query, ly.attention.self.key, ly.attention.self.value, ly.intermediate.dense):
                    mod.weight.div_(s)
            head.weight.div_(s)
        elif case in CTX:
            even, odd = CTX[case]
            v = torch.full((cfg.hidden_size,), odd)
            v[0::2] = even
            for ly in model.encoder.layer:
                ly.attention.self.value.weight.mul_(v[:, None])
                ly.attention.self.value.bias.mul_(v)
                ly.attention.output.dense.weight.div_(v[None, :])
        elif case == "hidden_lo":
            for ly in model.encoder.layer:
                ly.intermediate.dense.weight.mul_(2.0 ** -10)
                ly.intermediate.dense.bias.mul_(2.0 ** -10)
                ly.output.dense.weight.mul_(2.0 ** 10)
        elif case == "sharp":
            for ly in model.encoder.layer:
                ly.attention.self.query.weight.mul_(12.0)
                ly.attention.self.query.bias.mul_(12.0)
    return cfg, model, head


def state_of(model, head):
    """The fp32 state dict ``TextTower`` takes."""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd["head.weight"], sd["head.bias"] = head.weight.detach().clone(), head.bias.detach().clone()
    return sd


def _bank(model, head, ids, mask, dtype, gelu=None, split_inputs=False):
    model, head = copy.deepcopy(model).to(dtype), copy.deepcopy(head).to(dtype)
    if gelu is not None:
        class Act(torch.nn.Module):
            def forward(self, x):
                return gelu(x)
        for ly in model.encoder.layer:
            ly.intermediate.intermediate_act_fn = Act()
    if split_inputs:
        def pre(_mod, args):
            x = args[0]
            hi = x.to(torch.float16).to(x.dtype)
            return (hi + (x - hi).to(torch.float16).to(x.dtype),) + tuple(args[1:])
        for mod in list(model.modules()) + [head]:
            if isinstance(mod, torch.nn.Linear):
                mod.register_forward_pre_hook(pre)
    with torch.no_grad():
        hs = model(input_ids=ids, attention_mask=mask)["last_hidden_state"][:, 0]
        return torch.nn.functional.normalize(head(hs), dim=-1).double().numpy()


def bank64(model, head, ids, mask):
    return _bank(model, head, ids, mask, torch.float64)


def bank32(model, head, ids, mask):
    return _bank(model, head, ids, mask, torch.float32)


# csrc/common.h wd_gelu: GELU(x) = max(x, 0) - |x| Phi(-|x|) with Phi(-a) = exp2(P5(a)); the coefficients as the fp32 numbers
# the kernel holds, everything else in float64.
_P5 = [float(np.float32(c)) for c in (-4.8865197459e-04, 7.2031705640e-03, -5.2158899605e-02, -4.5958217978e-01,
                                      -1.1510057449e+00, -1.0)]


def gelu_fit64(x: torch.Tensor) -> torch.Tensor:
    ax = x.abs()
    p = torch.full_like(ax, _P5[0])
    for c in _P5[1:]:
        p = p * ax + c
    return x.clamp_min(0.0) - ax * torch.exp2(p)


def bank_gelu(model, head, ids, mask):
    """The float64 model with the project's fitted GELU in place of the exact one."""
    return _bank(model, head, ids, mask, torch.float64, gelu=gelu_fit64)


def bank_unscaled_split(model, head, ids, mask):
    """The float64 model with every Linear input x replaced by fp16(x) + fp16(x - fp16(x)): the operand rounding of the
    loader split without range management (nothing else of the device is emulated).  Beyond 65504 it is non-finite."""
    return _bank(model, head, ids, mask, torch.float64, split_inputs=True)


def reference(case: str, dims: str, n: int = 37, ln: int = 11, pad_to: int = 0):
    """ids / mask / state dict of a case with its float64 bank, e32_hf, e_gelu and the limit.  ``pad_to``: the same sequences
    padded to that length."""
    key = (case, dims, n, ln, pad_to)
    if key not in _REF:
        cfg, model, head = build(case, dims)
        ids = make_ids(n, ln)
        if pad_to:
            ids = repad(ids, pad_to)
        mask = (ids != PAD).long()
        b64 = bank64(model, head, ids, mask)
        e32 = float(np.abs(bank32(model, head, ids, mask) - b64).max())
        eg = float(np.abs(bank_gelu(model, head, ids, mask) - b64).max())
        _REF[key] = dict(case=case, dims=dims, cfg=cfg, model=model, head=head, ids=ids, mask=mask, bank64=b64, e32_hf=e32,
                         e_gelu=eg, limit=8.0 * e32 + 2.0 * eg, heads=cfg.num_attention_heads, eps=eps_of(case),
                         state=state_of(model, head))
    return _REF[key]


def limit(ref) -> float:
    return ref["limit"]


def max_err(bank, ref) -> float:
    """max |bank - bank64|; inf when the bank is not finite."""
    b = np.asarray(bank, dtype=np.float64)
    return float(np.abs(b - ref["bank64"]).max()) if np.isfinite(b).all() else float("inf")
