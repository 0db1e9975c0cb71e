"""No GPU: the host side of impop_tree_scan — the ABI declaration and its binding, the record layouts on both sides, the plain
restatement on the known answer of the header and against scipy where it is installed, what the GPU tests' cases rest on
(tree_cases.preconditions), and impop_amd/tree.py's derived values (heights, Newick, cut, Robinson-Foulds)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairdist_cases as pc
import plain_pca as pl
import plain_tree as pt
import tree_cases as tc
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
KNOWN = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 0, 1]], np.uint8)
KNOWN_MERGES = {"average": [(1, 3, 1, 1, 0), (0, 1, 1, 2, 2), (0, 2, 3, 1, 7)],
                "single": [(1, 3, 1, 1, 0), (0, 1, 1, 2, 1), (0, 2, 3, 1, 2)],
                "complete": [(1, 3, 1, 1, 0), (0, 1, 1, 2, 1), (0, 2, 3, 1, 3)]}
FIELDS = {"impop_tree_params": ["struct_size", "linkage"],
          "impop_tree_window": ["n_members", "n_sites", "n_zero_merges", "n_tied_merges", "sum_h", "root_num", "root_size_a", "root_size_b",
                                "reserved"],
          "impop_tree_merge": ["a", "b", "size_a", "size_b", "num"],
          "impop_tree_panel": ["n_members", "largest_clade", "mrca_size", "mrca_merge"]}


def test_abi_declares_tree_scan():
    import impop_amd
    from impop_amd import _lib
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", HEADER) and _lib.ABI_VERSION == 4
    assert re.search(r"#define IMPOP_TREE_MAX_N\s+1024u\b", HEADER) and _lib.TREE_MAX_N == 1024
    assert re.search(r"enum \{ IMPOP_LINKAGE_SINGLE = 0, IMPOP_LINKAGE_COMPLETE = 1, IMPOP_LINKAGE_AVERAGE = 2 \};", HEADER)
    assert _lib.TREE_LINKAGES == {"single": 0, "complete": 1, "average": 2}
    for fn, n_args in (("impop_tree_scan", 11), ("impop_ctx_tree_elapsed", 3)):
        assert re.search(r"^int %s\(" % fn, HEADER, re.M) and len(_lib.SIGNATURES[fn][1]) == n_args
        decl = re.search(r"^int %s\((.*?)\);" % fn, HEADER, re.M | re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == n_args
    sides = ((_lib.TreeParams, None, 8), (_lib.TreeWindow, impop_amd.TREE_WINDOW_DTYPE, 48), (_lib.TreeMerge, impop_amd.TREE_MERGE_DTYPE, 24),
             (_lib.TreePanel, impop_amd.TREE_PANEL_DTYPE, 16))
    for (struct, want), (ct, dt, size) in zip(FIELDS.items(), sides):
        assert C.sizeof(ct) == size and (dt is None or dt.itemsize == size)
        assert re.search(r"typedef struct %s \{\s*/\* %d bytes" % (struct, size), HEADER), struct
        assert [n for n, _ in ct._fields_] == want and (dt is None or list(dt.names) == want)
        if dt is not None:
            for name in want:  # same offsets on both sides
                assert getattr(ct, name).offset == dt.fields[name][1]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want, struct
    assert _lib.TreeWindow.sum_h.offset == 16 and _lib.TreeWindow.root_num.offset == 24 and _lib.TreeWindow.reserved.offset == 40
    assert _lib.TreeMerge.num.offset == 16
    assert hasattr(impop_amd.BitMatrix, "tree_scan") and hasattr(impop_amd.Context, "tree_elapsed")
    for name in ("heights", "to_newick", "cut", "rf_distance", "tree", "TREE_WINDOW_DTYPE", "TREE_MERGE_DTYPE", "TREE_PANEL_DTYPE"):
        assert hasattr(impop_amd, name), name
    lib = _lib.load()
    assert hasattr(lib, "impop_tree_scan") and hasattr(lib, "impop_ctx_tree_elapsed")
    # what the header must state about the call
    doc = " ".join(HEADER[HEADER.index("#define IMPOP_TREE_MAX_N"):HEADER.index("typedef struct impop_tree_params")].replace("*", " ").split())
    for text in ("smallest (value, a, b), lexicographic", "full 128-bit products", "m^4 / 64 = 2^34", "a product reaches 2^65",
                 "non-decreasing in merge order", "reducible", "monophyletic IN THE TREE AS OUTPUT iff mrca_size == n_members",
                 "[impop_tree_scan] route=<dense|compact> linkage=<single|complete|average> members= pops= windows= chunks= launches= "
                 "rows_recomputed= tied_windows=", "(1, 3, 1, 1, 0); then", "(0, 2, 3, 1, 7), value 7/3", "mrca_size 3 / 4, mrca_merge 1 / 2",
                 "IMPOP_E_UNSUPPORTED", "a panel member outside mask_p"):
        assert text in doc, text


@pytest.mark.parametrize("linkage", pt.LINKAGES)
def test_known_answer_of_the_header(linkage):
    H = pl.distances(KNOWN, 0, 4)
    assert [int(H[i, j]) for i in range(4) for j in range(i + 1, 4)] == [1, 3, 1, 2, 0, 2]
    t = pt.window(H, 4, linkage, [[0, 1], [2, 3]])
    assert t["merges"] == KNOWN_MERGES[linkage]
    assert (t["n_zero"], t["n_tied"], t["sum_h"], t["n_members"], t["n_sites"]) == (1, 0, 9, 4, 4)
    if linkage == "average":
        assert [(p["largest_clade"], p["mrca_size"], p["mrca_merge"]) for p in t["panels"]] == [(1, 3, 1), (1, 4, 2)]
    one = pt.tree(H, linkage, [[2]])["panels"][0]
    assert (one["n_members"], one["largest_clade"], one["mrca_size"], one["mrca_merge"]) == (1, 1, 1, 0xFFFFFFFF)


def test_the_cases_hold_what_the_gpu_tests_rest_on():
    seen = tc.preconditions()
    assert seen["tied"] and seen["untied"] and seen["all_zero"]


def test_the_128_bit_case_needs_more_than_64_bits():
    assert tc.wide_preconditions() >= 2 ** 64
    ref = tc.wide_reference()
    assert ref["merges"][-2][:4] == (0, 512, 512, 255) and ref["merges"][-1][:4] == (0, 767, 767, 257)


def value_pairs(ref, linkage):
    return [(num, sa * sb if linkage == "average" else 1) for _, _, sa, sb, num in ref["merges"]]


@pytest.mark.parametrize("linkage", pt.LINKAGES)
def test_values_never_decrease(linkage):
    for n in tc.NS:
        for shape in ("tiling", "sliding"):
            for mask in tc.MASKS:
                for ref in tc.references(n, shape, mask, linkage, 0):
                    v = value_pairs(ref, linkage)
                    assert all(v[i][0] * v[i + 1][1] <= v[i + 1][0] * v[i][1] for i in range(len(v) - 1)), (n, shape, mask)
                    assert sum(num == 0 for num, _ in v) == ref["n_zero"]


def condensed(H):
    m = H.shape[0]
    return np.array([H[i, j] for i in range(m) for j in range(i + 1, m)], np.float64)


def test_single_linkage_heights_equal_scipy_on_every_case():
    """the sorted merge values of single linkage are a function of the distances alone (the minimum spanning tree), ties or not"""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    for n in tc.NS:
        m01 = tc.matrix(n)
        for shape in ("tiling", "sliding"):
            for mask in tc.MASKS:
                for w, ref in zip(pc.window_lists()[shape], tc.references(n, shape, mask, "single", 0)):
                    H = pl.distances(m01, w[0], w[1], tc.members(n, mask))
                    Z = hierarchy.linkage(condensed(H), "single")
                    assert sorted(g[4] for g in ref["merges"]) == sorted(int(x) for x in Z[:, 2]), (n, shape, mask)


@pytest.mark.parametrize("linkage", pt.LINKAGES)
def test_heights_equal_scipy_without_ties(linkage):
    """random integer matrices whose entries are all different: no step has a choice, so every linkage's merge values are scipy's
    (average: within the rounding of scipy's floating-point Lance-Williams recurrence, 4 m eps relative)"""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from impop_amd import tree
    rng = np.random.default_rng(7)
    for m in (2, 3, 17, 40):
        vals = rng.permutation(np.arange(1, 20 * m * m))[: m * (m - 1) // 2] * 2  # even: complete/single heights are integers
        H = np.zeros((m, m), np.int64)
        H[np.triu_indices(m, 1)] = vals
        H = H + H.T
        t = pt.tree(H, linkage)
        Z = hierarchy.linkage(condensed(H), linkage)
        got = tree.heights(pt.merges_array(t), linkage) * 2.0
        if linkage == "average":
            assert np.abs(got - Z[:, 2]).max() <= 4 * m * 2.0 ** -52 * Z[:, 2].max()
        else:
            assert (got == Z[:, 2]).all() and t["n_tied"] == 0
        assert [g[2] + g[3] for g in t["merges"]] == [int(x) for x in Z[:, 3]]


def test_newick_cut_and_rf():
    from impop_amd import tree
    H = pl.distances(KNOWN, 0, 4)
    names = ["s0", "s1", "s2", "s3"]
    t = {l: pt.tree(H, l) for l in pt.LINKAGES}
    arr = {l: pt.merges_array(t[l]) for l in pt.LINKAGES}
    assert list(tree.heights(arr["average"], "average")) == [0.0, 0.5, 7 / 3 / 2] and list(tree.heights(arr["complete"], "complete")) == [0.0, 0.5, 1.5]
    nwk = tree.to_newick(arr["average"], names, "average")
    assert nwk == "((s0:0.5,(s1:0.0,s3:0.0):0.5):%r,s2:%r);" % (7 / 3 / 2 - 0.5, 7 / 3 / 2)
    for l in pt.LINKAGES:
        assert tree.to_newick(arr[l], names, l) == pt.newick(t[l]["merges"], names, l)
        assert sorted(re.findall(r"[(,]([^(),:;]+):", tree.to_newick(arr[l], names, l))) == names
    quoted = tree.to_newick(arr["single"], ["a b", "c:1", "it's", "plain"], "single")
    assert quoted == pt.newick(t["single"]["merges"], ["a b", "c:1", "it's", "plain"], "single")
    assert quoted == "(('a b':0.5,('c:1':0.0,plain:0.0):0.5):0.5,'it''s':1.0);"
    assert list(tree.cut(arr["average"], 0)) == [0, 1, 2, 1] and list(tree.cut(arr["average"], 0.5)) == [0, 0, 2, 0]
    assert list(tree.cut(arr["average"], 100)) == [0, 0, 0, 0] and list(tree.cut(arr["single"], -1, "single")) == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        tree.heights(arr["average"], "ward")
    with pytest.raises(ValueError):
        tree.rf_distance(arr["average"], arr["average"][:2])
    # on the cases: RF of a tree with itself is 0, symmetric, equal to the plain one; cut at 0 gives the identical-haplotype classes
    n = 31
    m01 = tc.matrix(n)
    refs = tc.references(n, "tiling", "all", "average", 0)
    arrs = [pt.merges_array(r) for r in refs]
    seen_far = False
    for w, win in enumerate(pc.window_lists()["tiling"]):
        assert tree.rf_distance(arrs[w], arrs[w]) == 0
        if w:
            d = tree.rf_distance(arrs[w - 1], arrs[w])
            assert d == tree.rf_distance(arrs[w], arrs[w - 1]) == pt.rf(refs[w - 1]["merges"], refs[w]["merges"]) and 0 <= d <= 2 * (n - 2)
            seen_far = seen_far or d > 0
        rows = m01[:, win[0]:win[1]]
        first = {}
        want = [first.setdefault(rows[i].tobytes(), i) for i in range(n)]
        assert list(tree.cut(arrs[w], 0)) == want and len(set(want)) == n - refs[w]["n_zero"]
        assert tree.to_newick(arrs[w], list(range(n)), "average") == pt.newick(refs[w]["merges"], list(range(n)), "average")
    assert seen_far
