"""The text bank folded into the head's embedding conv, on the CPU: the algebra of the fold against the oracle in float64
(before any kernel is involved), and the C ABI of include/wedetect_hip_fold.h."""
import numpy as np
import torch
import torch.nn.functional as F


def _c2_of_level(sd, l, feat):
    """The input of the embedding conv: cls_preds.{l} without its last 1x1 conv (oracle/ref_cpu.py _head_branch)."""
    from oracle.ref_cpu import HD
    x = feat
    for s in ("0", "1"):
        q = HD + f"cls_preds.{l}.{s}"
        x = F.conv2d(x, sd[q + ".conv.weight"], None, padding=1)
        x = F.batch_norm(x, sd[q + ".bn.running_mean"], sd[q + ".bn.running_var"], sd[q + ".bn.weight"], sd[q + ".bn.bias"],
                         False, 0.03, 1e-3)
        x = F.silu(x)
    return x


def _oracle_logits64(sd, feats, text, normalize):
    """The class half of oracle.ref_cpu.head_level / head_flat, from the oracle's own pieces, in float64 (head_flat itself
    cannot run in float64: its box half pins a float32 projection vector)."""
    from oracle import ref_cpu as orc
    out = []
    for l, f in enumerate(feats):
        q = orc.HD + f"cls_contrasts.{l}"
        e = orc._head_branch(sd, orc.HD + f"cls_preds.{l}", f)
        e = F.batch_norm(e, sd[q + ".norm.running_mean"], sd[q + ".norm.running_var"], sd[q + ".norm.weight"], sd[q + ".norm.bias"],
                         False, 0.03, 1e-3)
        t = F.normalize(text, dim=-1, p=2) if normalize else text
        lg = torch.einsum("bchw,kc->bkhw", e, t) * sd[q + ".logit_scale"].exp() + sd[q + ".bias"]
        out.append(lg.permute(0, 2, 3, 1).reshape(lg.shape[0], -1, lg.shape[1]))
    return torch.cat(out, dim=1)


def test_scores_from_c2_with_folded_weights_equal_the_oracle_head_in_float64():
    """logit = <W_e c2 + b_e, t^> e^s + b  ==  <c2, t^ W_e> e^s + <b_e, t^> e^s + b  with W_e / b_e as pack() folds the contrastive
    BatchNorm into the embedding conv: Base @ 64, both text handlings — to float64 rounding against the oracle's class branch
    in float64, and to float32 rounding against head_flat itself (float32)."""
    from oracle import ref_cpu as orc
    from wedetect_amd import weights as W
    from wedetect_amd.arch import HD, get_arch
    from wedetect_amd.pack import _conv_rows, _fold_bn
    arch, b, hw, k = "base", 2, 64, 81
    sd_np = W.make_state_dict(arch)
    sd32 = orc.to_torch(sd_np)
    sd = {n: (v.double() if v.is_floating_point() else v) for n, v in sd32.items()}
    imgs = W.make_images(b, hw, hw, seed=77)
    bank = torch.from_numpy(W.make_text_bank(k)).double() * 1.7          # rows of norm 1.7: normalisation must matter
    with torch.no_grad():
        x = orc.preprocess_u8(imgs).double()
        feats = orc.neck(sd, get_arch(arch), orc.backbone(sd, get_arch(arch), x))
        _, feats32 = orc.forward_features(sd32, arch, imgs)
        for normalize in (True, False):
            flat32 = orc.head_flat(sd32, feats32, bank.float(), normalize_text=normalize)
            ref = _oracle_logits64(sd, feats, bank, normalize)
            flat = dict(logits=ref, scores=ref.sigmoid())
            t = F.normalize(bank, dim=-1, p=2) if normalize else bank
            logits = []
            for l, f in enumerate(feats):
                q = HD + f"cls_contrasts.{l}"
                g = lambda n: np.asarray(sd_np[n], np.float64)
                wf, bf = _fold_bn(g(HD + f"cls_preds.{l}.2.weight"), g(HD + f"cls_preds.{l}.2.bias"), g(q + ".norm.weight"),
                                  g(q + ".norm.bias"), g(q + ".norm.running_mean"), g(q + ".norm.running_var"), 1e-3)
                w_e, b_e = torch.from_numpy(np.asarray(_conv_rows(wf), np.float64)), torch.from_numpy(np.asarray(bf, np.float64))
                w_fold, b_fold = t @ w_e, t @ b_e                                     # [K, 256], [K]
                c2 = _c2_of_level(sd, l, f).permute(0, 2, 3, 1).reshape(b, -1, w_e.shape[1])
                logits.append((c2 @ w_fold.T + b_fold) * sd[q + ".logit_scale"].exp() + sd[q + ".bias"])
            got = torch.cat(logits, dim=1)
            assert got.shape == flat["logits"].shape
            d_l = float((got - flat["logits"]).abs().max())
            d_s = float((got.sigmoid() - flat["scores"]).abs().max())
            print(f"normalize={normalize}: max |d logit| {d_l:.2e} (max |logit| {float(flat['logits'].abs().max()):.2f}), max |d score| {d_s:.2e}")
            # float64 rounding of two 768- / 256-term contractions in a different order: 1e-12 is four decades above it
            assert d_l <= 1e-12 * max(1.0, float(flat["logits"].abs().max())) and d_s <= 1e-12
            d_32 = float((got.sigmoid() - flat32["scores"].double()).abs().max())
            print(f"normalize={normalize}: max |d score| against head_flat (float32) {d_32:.2e}")
            assert d_32 <= 1e-5            # the float32 oracle's own rounding (its scores sit ~1e-6 from a float64 run, split_gemm.hip)


def test_library_exports_the_fold_header_and_every_memory_entry_has_an_extents_case():
    from tests.abi_decl import declared
    from tests.test_cpu_arena import _takes_memory
    from tests.test_gpu_fold_extents import CASES, EXEMPT
    from wedetect_amd import build as wb
    from wedetect_amd import fold as FD
    decl = declared("wedetect_hip_fold.h")
    assert set(decl) == set(FD.EXPORTS)
    assert "wedetect_hip_fold.h" in wb.PUBLIC_HEADERS and "fold.hip" in wb.SOURCES
    assert FD.LIB.wd_fold_abi_version() == FD.FOLD_ABI_VERSION == 1
    covered = {c.entry for c in CASES}
    for name, params in decl.items():
        assert (name in covered) != (name in EXEMPT), f"{name}: needs exactly one of an extents case and an EXEMPT reason"
        if name in EXEMPT:
            assert not _takes_memory(params), f"{name} takes device memory: it must have a case"
