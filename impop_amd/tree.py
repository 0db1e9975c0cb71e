"""Values derived on the host from the merge records of BitMatrix.tree_scan (impop_tree_scan), and the rows scripts/impop_tree.py
writes from them.  No GPU and no library is needed here: a window's merges are a structured array (or any sequence of records with
the fields a, b, size_a, size_b, num) of m - 1 merges over the member positions 0 .. m - 1, in merge order.

A merge joins the clusters NAMED a < b (a cluster's name is its lowest member position) into one that keeps the name a.  Its value
is num for single and complete linkage and num / (size_a size_b) for average linkage; the height of the node is half of it, the
distance being shared by the two branches, as in UPGMA."""
import numpy as np

LINKAGES = ("single", "complete", "average")

MAIN_COLUMNS = ("chrom", "start", "end", "n_members", "n_sites", "distinct", "tied_merges", "root_height", "rf_prev")
MERGE_COLUMNS = ("chrom", "start", "end", "merge", "a", "b", "size_a", "size_b", "num", "height")
PANEL_COLUMNS = ("chrom", "start", "end", "panel", "n_members", "largest_clade", "mrca_size", "mrca_merge", "monophyletic")


def _check(linkage):
    if linkage not in LINKAGES:
        raise ValueError("linkage must be one of %s" % ", ".join(LINKAGES))


def heights(merges, linkage):
    """-> float64 [m - 1]: the height of every merge's node, num / 2 (single, complete) or num / (size_a size_b) / 2 (average)"""
    _check(linkage)
    out = np.empty(len(merges), np.float64)
    for i, g in enumerate(merges):
        v = float(int(g["num"]))
        if linkage == "average":
            v = v / float(int(g["size_a"]) * int(g["size_b"]))
        out[i] = v / 2.0
    return out


def clades(merges):
    """-> per merge the frozenset of member positions of the cluster it forms"""
    m = len(merges) + 1
    held = {i: frozenset((i,)) for i in range(m)}
    out = []
    for g in merges:
        a, b = int(g["a"]), int(g["b"])
        held[a] = held[a] | held.pop(b)
        out.append(held[a])
    return out


def newick_label(name):
    """a leaf name as Newick takes it: quoted, with quotes doubled, when it holds one of ()[]':;, or white space"""
    name = str(name)
    if any(c in name for c in "()[]':;,") or any(c.isspace() for c in name):
        return "'" + name.replace("'", "''") + "'"
    return name


def to_newick(merges, names, linkage):
    """The tree as a Newick string over `names` (one per member position).  Children are written a then b; a branch is as long as
    its parent's height minus its child's (leaves are at 0), written with repr() of the double; the root carries no length; names
    that hold Newick's punctuation (a PanSN name has a colon) are quoted."""
    h = heights(merges, linkage)
    if len(names) != len(merges) + 1:
        raise ValueError("%d names for %d members" % (len(names), len(merges) + 1))
    node = {i: (newick_label(names[i]), 0.0) for i in range(len(names))}
    for i, g in enumerate(merges):
        a, b = int(g["a"]), int(g["b"])
        (ta, ha), (tb, hb) = node[a], node.pop(b)
        node[a] = ("(%s:%s,%s:%s)" % (ta, repr(float(h[i] - ha)), tb, repr(float(h[i] - hb))), float(h[i]))
    (text, _), = node.values()
    return text + ";"


def cut(merges, height, linkage="average"):
    """-> uint32 [m]: per member the name (lowest member position) of its cluster once every merge of height <= `height` is made.
    Heights never decrease along the merges, so these are a prefix.  cut(merges, 0) gives the classes of identical haplotypes."""
    h = heights(merges, linkage)
    label = np.arange(len(merges) + 1, dtype=np.uint32)
    for i, g in enumerate(merges):
        if h[i] > height:
            break
        label[label == int(g["b"])] = int(g["a"])
    return label


def rf_distance(merges_x, merges_y):
    """Robinson-Foulds distance of two merge lists over the same members: the size of the symmetric difference of their sets of
    non-trivial clades (at least two members, not all of them)"""
    if len(merges_x) != len(merges_y):
        raise ValueError("the two trees have %d and %d members" % (len(merges_x) + 1, len(merges_y) + 1))
    m = len(merges_x) + 1
    cx = {c for c in clades(merges_x) if 1 < len(c) < m}
    cy = {c for c in clades(merges_y) if 1 < len(c) < m}
    return len(cx ^ cy)


def root_height(rec, linkage):
    """the height of the root from a window record alone"""
    _check(linkage)
    v = float(int(rec["root_num"]))
    if linkage == "average":
        v = v / float(int(rec["root_size_a"]) * int(rec["root_size_b"]))
    return v / 2.0


def tables(rows, names, recs, merges, panels, panel_names, linkage, want_merges=False):
    """The rows scripts/impop_tree.py writes for the windows of ONE matrix.  rows: (chrom, start, end) per window.
    -> (main rows, merge rows, panel rows, newick lines) as lists of string lists / strings; rf_prev is the Robinson-Foulds distance
    to the previous window of this matrix, NA for the first."""
    main, mrows, prows, nwk = [], [], [], []
    for w, (chrom, start, end) in enumerate(rows):
        r = recs[w]
        rf = "NA" if w == 0 else str(rf_distance(merges[w - 1], merges[w]))
        where = [str(chrom), str(start), str(end)]
        main.append(where + [str(int(r["n_members"])), str(int(r["n_sites"])), str(int(r["n_members"]) - int(r["n_zero_merges"])),
                             str(int(r["n_tied_merges"])), repr(root_height(r, linkage)), rf])
        nwk.append(to_newick(merges[w], names, linkage))
        if want_merges:
            h = heights(merges[w], linkage)
            for i, g in enumerate(merges[w]):
                mrows.append(where + [str(i), str(int(g["a"])), str(int(g["b"])), str(int(g["size_a"])), str(int(g["size_b"])),
                                      str(int(g["num"])), repr(float(h[i]))])
        if panels is not None:
            for p, name in enumerate(panel_names):
                q = panels[w, p]
                prows.append(where + [str(name), str(int(q["n_members"])), str(int(q["largest_clade"])), str(int(q["mrca_size"])),
                                      "NA" if int(q["mrca_merge"]) == 0xFFFFFFFF else str(int(q["mrca_merge"])),
                                      "1" if int(q["mrca_size"]) == int(q["n_members"]) else "0"])
    return main, mrows, prows, nwk
