"""Prompt groups on the CPU: the packing invariants of wedetect_amd/groups.py on random class sizes and on the two LVIS class-text
fixtures, a numpy model of the class maximum over the padded bank against the unpadded prompts, the public switches and refusals,
both command lines, the header against the binding."""
import os
import re

import numpy as np
import pytest
import torch

import tests.groups_hazards  # noqa: F401  (declares the wrappers of wedetect_amd/groups.py to tests/hazards.py)
from tests import groups_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_plan(pg, sizes):
    rows, go, bf = pg.rows.numpy(), pg.group_of.numpy(), pg.bin_first.numpy()
    G, P = len(sizes), int(sum(sizes))
    assert (pg.G, pg.P) == (G, P) and pg.K_pad == len(rows) == len(go) and pg.K_pad % 32 == 0 and len(bf) == pg.K_pad // 32 + 1
    assert rows.dtype == np.int64 and go.dtype == np.int32 and bf.dtype == np.int32
    # group_of is non-decreasing, covers every class, and a bin starts with its first class
    assert bool((np.diff(go) >= 0).all()) and go[0] == 0 and go[-1] == G - 1 and set(go.tolist()) == set(range(G))
    assert np.array_equal(go[::32], bf[:-1]) and bf[-1] == G and bool((np.diff(bf) >= 1).all()) and bool((np.diff(bf) <= 32).all())
    # every class lies inside one bin
    for a, z in GR.class_ranges(go):
        assert a // 32 == (z - 1) // 32, (a, z)
    # first occurrences are the flat list in order; every other row repeats the row before it (padding), in the same class
    first = np.r_[True, rows[1:] != rows[:-1]]
    assert np.array_equal(rows[first], np.arange(P))
    pad = np.flatnonzero(~first)
    assert np.array_equal(rows[pad], rows[pad - 1]) and np.array_equal(go[pad], go[pad - 1])
    assert len(pad) == pg.K_pad - P
    # padding closes a bin: behind a padding row comes padding or a bin boundary
    assert all((i + 1) % 32 == 0 or not first[i + 1] for i in pad.tolist())
    # the rows of class g are the flat rows of class g
    start = np.cumsum(np.r_[0, sizes[:-1]])
    assert np.array_equal(go[first], np.repeat(np.arange(G), sizes)) and np.array_equal(pg.first_of().numpy(), start)
    # next-fit: a bin was closed only because the next class did not fit
    for s in range(1, len(bf) - 1):
        used = int(first[32 * (s - 1): 32 * s].sum())
        assert used + sizes[bf[s]] > 32, s


def test_packing_invariants_on_random_sizes():
    from wedetect_amd.groups import PromptGroups
    g = np.random.default_rng(11)
    for trial in range(200):
        hi = (2, 4, 12, 33)[trial % 4]
        sizes = g.integers(1, hi, int(g.integers(1, 120))).tolist()
        if trial % 10 == 0:
            sizes[int(g.integers(0, len(sizes)))] = 32
        _check_plan(PromptGroups.from_sizes(sizes), sizes)
    for sizes in (GR.ONE_BIN, GR.K352, (32,), (1,), (32, 32), (31, 2), (1,) * 33):
        _check_plan(PromptGroups.from_sizes(sizes), list(sizes))
    assert PromptGroups.from_sizes(GR.ONE_BIN).K_pad == 32 and PromptGroups.from_sizes(GR.K352).K_pad == 352
    k352 = PromptGroups.from_sizes(GR.K352)
    assert k352.bin_first.tolist()[:5] == [0, 2, 3, 4, 5] and int((k352.rows[64:96] == k352.rows[64]).sum()) == 32      # 31 copies of the singleton


@pytest.mark.parametrize("name,want", [(GR.LVIS_EN, (1203, 1983, 2048)), (GR.LVIS_ZH, (1203, 1775, 1824))])
def test_lvis_fixtures_pack_to_the_expected_sizes(name, want):
    from wedetect_amd.groups import PromptGroups
    texts = GR.lvis_texts(name)
    pg = PromptGroups.from_texts(texts)
    assert (pg.G, pg.P, pg.K_pad) == want
    _check_plan(pg, [len(t) for t in texts])
    assert pg.flat == [p for t in texts for p in t] and 2 <= max(pg.sizes) <= 10
    if name == GR.LVIS_EN:
        assert texts[0] == ["aerosol can", "spray can"] and sum(len(t) > 1 for t in texts) == 463
    assert os.path.getsize(os.path.join(GR.GOLDEN, name)) < 64 << 10


def test_coco_singletons_and_refusals():
    from wedetect_amd.groups import PromptGroups
    pg = PromptGroups.from_texts([[f"c{i}"] for i in range(80)])
    assert (pg.G, pg.P, pg.K_pad) == (80, 80, 96) and pg.rows[:80].tolist() == list(range(80)) and pg.rows[80:].tolist() == [79] * 16
    assert PromptGroups.from_texts(["a", ["b", "c"]]).sizes == (1, 2)          # a bare string is a class of one prompt
    with pytest.raises(ValueError, match=r"class 1 \('dog'\) has 33 prompts"):
        PromptGroups.from_texts([["cat"], ["dog"] + ["d"] * 32])
    with pytest.raises(ValueError, match="class 2 .* has 0 prompts"):
        PromptGroups.from_texts([["cat"], ["dog"], []])
    with pytest.raises(ValueError, match="class 0 has 33 prompts"):
        PromptGroups.from_sizes([33])
    with pytest.raises(ValueError):
        PromptGroups.from_sizes([])
    with pytest.raises(ValueError, match=r"expected \(80, D\)"):
        pg.pad_bank(torch.zeros(81, 8))


def test_padding_changes_nothing_numpy_model():
    """The class maximum over the padded bank equals the maximum over the unpadded prompts, on scores with ties and negatives."""
    from wedetect_amd.groups import PromptGroups
    g = np.random.default_rng(5)
    for sizes in (GR.K352, tuple(len(t) for t in GR.lvis_texts()), GR.ONE_BIN):
        pg = PromptGroups.from_sizes(sizes)
        flat = (np.round(g.standard_normal((7, pg.P)).astype(np.float32) * 4) / 4).astype(np.float32)
        want = np.stack([flat[:, a:a + n].max(axis=1) for a, n in zip(pg.first_of().tolist(), sizes)], axis=1)
        padded = flat[:, pg.rows.numpy()]
        assert np.array_equal(pg.class_max(padded), want)
        assert np.array_equal(pg.class_max(torch.from_numpy(padded)).numpy(), want)
        assert np.array_equal(GR.class_amax(torch.from_numpy(padded), pg.group_of.numpy()).numpy(), want)
        bank = torch.from_numpy(g.standard_normal((pg.P, 8)).astype(np.float32))
        assert torch.equal(pg.pad_bank(bank), bank[pg.rows])


def test_chunks_of_the_tower_cut_no_class():
    from wedetect_amd import groups as PG
    assert PG.FUSED_CHUNK % PG.BIN == 0 and PG.ROWS_CHUNK % PG.BIN == 0 and PG.BIN == 32


def test_public_switches_and_refusals():
    from wedetect_amd.detector import YOLOWorldDetector
    for kw in (dict(best_class=True), dict(sparse_scores=True), dict(best_class=True, top_names=3)):
        with pytest.raises(ValueError, match="prompt_groups"):
            YOLOWorldDetector("nano", prompt_groups=True, **kw)
    assert YOLOWorldDetector("nano").prompt_groups is False
    d = YOLOWorldDetector("nano", prompt_groups=True)
    assert d.prompt_groups is True
    for fn, what in ((lambda: d.predict_stream([], 1, []), "predict_stream"), (lambda: d.predict_tiled(np.zeros((64, 64, 3), np.uint8)), "predict_tiled"),
                     (lambda: d.predict_views([], {}), "predict_views")):
        with pytest.raises(NotImplementedError, match=f"{what} with prompt_groups"):
            fn()
    # the bank of a grouped detector holds one row per prompt and is kept padded, under the key of the first captions
    texts = [["person", "man", "woman"], ["dog", "puppy"], [" "]]
    with pytest.raises(ValueError, match=r"\(6, 768\)"):
        d.set_text_embeddings(torch.zeros(3, 768), texts)
    with pytest.raises(ValueError, match="texts"):
        d.set_text_embeddings(torch.zeros(6, 768))
    bank = torch.arange(6, dtype=torch.float32)[:, None].expand(6, 768).contiguous()
    d.set_text_embeddings(bank, texts)
    assert d.text_feats.shape == (32, 768) and d.text_feats[:, 0].tolist() == [0, 1, 2, 3, 4, 5] + [5] * 26
    assert d._banks[("person", "dog", " ")] is d.text_feats and d._plan_cur.sizes == (3, 2, 1)
    assert d._plan_for(dict(texts=["person", "dog", " "])) is d._plan_cur and d._plan_for(None) is d._plan_cur
    # reparameterize encodes ALL prompts, class after class
    seen = []
    d2 = YOLOWorldDetector("nano", prompt_groups=True, text_encoder=lambda flat: (seen.append(list(flat)), torch.zeros(len(flat), 768))[1])
    d2.reparameterize(texts)
    assert seen == [["person", "man", "woman", "dog", "puppy", " "]] and d2.text_feats.shape == (32, 768)
    # ... and the first-caption form keeps working when the flag is off
    seen.clear()
    d3 = YOLOWorldDetector("nano", text_encoder=lambda flat: (seen.append(list(flat)), torch.zeros(len(flat), 768))[1])
    d3.reparameterize(texts)
    assert seen == [["person", "dog", " "]] and d3.text_feats.shape == (3, 768)
    d3.set_text_embeddings(torch.zeros(3, 768), texts)


def test_tower_detect_refuses_the_exclusive_modes_before_any_device_work():
    """ImageTower.detect validates the keyword first: the checks need neither a tower nor a device."""
    from wedetect_amd.engine import ImageTower
    from wedetect_amd.groups import PromptGroups
    pg = PromptGroups.from_sizes(GR.ONE_BIN)
    kw = dict(normalize_text=True, score_thr=0.1, prompt_groups=pg)
    for bad in (dict(best_class=True), dict(sparse_scores=True), dict(best_class=True, top_names=2)):
        with pytest.raises(ValueError, match="prompt_groups"):
            ImageTower.detect(None, None, torch.zeros(32, 768), None, **bad, **kw)
    with pytest.raises(NotImplementedError, match="per-image"):
        ImageTower.detect(None, None, torch.zeros(2, 32, 768), None, **kw)
    with pytest.raises(NotImplementedError, match="per-image"):
        ImageTower.detect(None, None, torch.zeros(32, 768), None, text_counts=torch.zeros(2, dtype=torch.int32), **kw)


def test_keyword_reaches_the_detector_from_a_config_and_from_both_scripts(capsys):
    import json

    import infer_wedetect
    import test as test_script
    from wedetect_amd.config import build_detector
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "model_cfgs.json")))["base"]["model"]
    assert build_detector(dict(ref, prompt_groups=True)).prompt_groups is True
    assert build_detector(ref).prompt_groups is False
    assert infer_wedetect.parse_args(["--config", "c", "--prompt-groups"]).prompt_groups
    assert not infer_wedetect.parse_args(["--config", "c"]).prompt_groups
    # '/' separates the names of one class, only under the flag
    assert infer_wedetect.read_texts("person/man/woman, dog/puppy,cat", True) == [["person", "man", "woman"], ["dog", "puppy"], ["cat"], [" "]]
    assert infer_wedetect.read_texts("person/man, dog") == [["person/man"], ["dog"], [" "]]
    for extra in (["--best-class"], ["--sparse-scores"], ["--tile", "640"]):
        with pytest.raises(SystemExit) as ei:
            infer_wedetect.parse_args(["--config", "c", "--prompt-groups", *extra])
        assert ei.value.code == 2 and "--prompt-groups" in capsys.readouterr().err
    assert test_script.parse_args(["c", "k", "--prompt-groups"]).prompt_groups and not test_script.parse_args(["c", "k"]).prompt_groups
    for extra in (["--best-class"], ["--sparse-scores"], ["--aug-test"], ["--loader", "stream"]):
        with pytest.raises(SystemExit) as ei:
            test_script.parse_args(["c", "k", "--prompt-groups", *extra])
        assert ei.value.code == 2 and "--prompt-groups" in capsys.readouterr().err
    # the --text-bank shape messages name P
    src = open(os.path.join(ROOT, "test.py")).read()
    assert "({n_prompts}, 768) with --prompt-groups" in src
    src = open(os.path.join(ROOT, "infer_wedetect.py")).read()
    assert "sum(len(t) for t in texts) if args.prompt_groups" in src


def test_header_prototypes_match_the_binding_and_every_entry_has_an_extent_case():
    from tests.abi_decl import declared
    from tests.test_cpu_abi import check_header
    from wedetect_amd import best, fold, sparse, topn
    from wedetect_amd import build as WB
    from wedetect_amd import groups as PG
    from wedetect_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "wedetect_hip_groups.h")).read()
    protos = declared("wedetect_hip_groups.h")
    assert sorted(protos) == sorted(PG.EXPORTS) == ["wd_group_rows", "wd_group_similarity_split", "wd_groups_abi_version"]
    assert all(ret == "int" for ret, _ in protos.values())
    assert "wedetect_hip_groups.h" in WB.PUBLIC_HEADERS and "groups.hip" in WB.SOURCES
    assert WB.NO_SCRATCH["groups.hip"] == ["group_rows_kernel"] and "split_gemm_p8_kernel" in WB.NO_SCRATCH["split_gemm_p8.hip"]
    check_header("wedetect_hip_groups.h")                     # argtypes / restype against the prototypes
    assert re.search(r"#define\s+WD_GROUP_BIN\s+32\b", hdr) and PG.BIN == 32
    assert PG.LIB.wd_groups_abi_version() == PG.GROUPS_ABI_VERSION == 1
    assert L.LIB.wd_abi_version() == L.ABI_VERSION == 15       # the main ABI and the other add-on headers stay
    assert best.LIB.wd_best_abi_version() == 1 and sparse.LIB.wd_sparse_abi_version() == 1 and topn.LIB.wd_topn_abi_version() == 1
    assert fold.LIB.wd_fold_abi_version() == fold.FOLD_ABI_VERSION
    for name in protos:                                       # each entry states its extents once ...
        if name != "wd_groups_abi_version":
            doc = hdr[: hdr.index(f"int {name}(")].rsplit("/* ----", 1)[1]
            assert doc.count("Extents:") == 1, name
    ext = open(os.path.join(ROOT, "tests", "test_gpu_groups_extents.py")).read()
    for name in protos:                                       # ... and has a guard-band case
        assert name == "wd_groups_abi_version" or f'"{name}"' in ext, f"{name}: no guard-band case"


def test_wrappers_are_declared_to_the_happens_before_checker():
    from tests import hazards as H
    assert {"groups.group_similarity_split", "groups.group_rows"} <= set(H.ACCESS)
    cite = [c for w, _, c in H.BENIGN if w == "groups.group_similarity_split"]
    assert len(cite) == 1
    ln = int(re.search(r"split_gemm_p8\.hip:(\d+)", cite[0]).group(1))
    src = open(os.path.join(ROOT, "wedetect_amd", "csrc", "split_gemm_p8.hip")).read().splitlines()
    assert "*p.range_flag = 1u;" in src[ln - 1]
    body = max(i for i, l in enumerate(src) if "p8_group_epilogue(" in l and l.startswith("__device__"))
    assert body < ln - 1 and not any(l.startswith("__device__") and "epilogue(" in l for l in src[body + 1: ln])     # inside the class-max epilogue
