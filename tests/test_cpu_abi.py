"""Every binding table against the prototypes of its header.  ctypes converts silently — an ``int64_t rows`` typed c_int32
truncates a row count past 2^31 without an error — so each of the public headers is read (tests/abi_decl.py) and the ``restype``
/ ``argtypes`` of its module, as they stand on the loaded library, must be what the prototypes ask for."""
import ctypes as C
import importlib
import os

import pytest

from tests.abi_decl import ROOT, bound, declared, mismatches
from wedetect_amd import build as WB

MODULES = {
    "wedetect_hip.h": "lib", "wedetect_hip_feed.h": "feed", "wedetect_hip_tile.h": "tile", "wedetect_hip_views.h": "views",
    "wedetect_hip_fold.h": "fold", "wedetect_hip_best.h": "best", "wedetect_hip_sparse.h": "sparse", "wedetect_hip_topn.h": "topn",
    "wedetect_hip_groups.h": "groups", "wedetect_hip_exemplar.h": "exemplar", "wedetect_hip_tune.h": "tune",
    "wedetect_hip_track.h": "track",
}


def _module(header):
    return importlib.import_module("wedetect_amd." + MODULES[header])


def check_header(header: str) -> None:
    """The names ``header`` declares are exactly its module's EXPORTS (= its SIGNATURES), and every function of the bound
    library carries the types of its prototype.  The per-feature files call this for their header."""
    mod, decl = _module(header), declared(header)
    assert sorted(decl) == sorted(mod.EXPORTS) and mod.EXPORTS == tuple(mod.SIGNATURES)
    assert not mismatches(decl, mod.SIGNATURES)
    assert not mismatches(decl, bound(mod))


@pytest.mark.parametrize("header", WB.PUBLIC_HEADERS)
def test_binding_matches_the_prototypes(header):
    check_header(header)


def test_every_header_has_one_module_and_no_name_is_bound_twice():
    on_disk = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    assert on_disk == sorted(WB.PUBLIC_HEADERS) == sorted(MODULES) and len(set(MODULES.values())) == len(MODULES)
    names = [n for h in MODULES for n in _module(h).EXPORTS]
    assert len(names) == len(set(names)) >= 104


def test_the_comparison_reports_a_wrong_table_by_function_name():
    """On data only: three edits of a copy of the main table, each of the kind ctypes would accept without a word."""
    from wedetect_amd import lib as L
    decl = declared("wedetect_hip.h")
    assert mismatches(decl, L.SIGNATURES) == []
    table = dict(L.SIGNATURES)
    rt, at = table["wd_similarity_split"]
    assert at[1] is C.c_int64
    table["wd_similarity_split"] = (rt, [at[0], C.c_int32] + at[2:])                   # int64_t rows typed i32
    table["wd_det_match"] = (table["wd_det_match"][0], table["wd_det_match"][1][:-1])  # the last argument dropped
    table["wd_topk_workspace_bytes"] = (None, table["wd_topk_workspace_bytes"][1])     # int64_t result left c_int
    bad = mismatches(decl, table)
    assert len(bad) == 3 and [b.split(":")[0] for b in sorted(bad)] == ["wd_det_match", "wd_similarity_split", "wd_topk_workspace_bytes"]
    by = {b.split(":")[0]: b for b in bad}
    assert "argument 1 of 16 (int64_t rows)" in by["wd_similarity_split"] and "argument 23 of 24" in by["wd_det_match"]
    assert "restype None for `int64_t`" in by["wd_topk_workspace_bytes"]
    del table["wd_det_sort"]
    assert "wd_det_sort: declared, not bound" in mismatches(decl, table)
