"""A plain numpy / Python restatement of impop_tree_scan, written from the prose of include/impop_hip.h and from nothing else: per
step a GLOBAL search over all live pairs for the smallest (value, a, b) — no cached neighbours, nothing of the kernel's scheme —
with Python integers deciding every comparison of two average-linkage values that a float could get wrong.  The tested library
is never the standard.

    tree(H, linkage, pops)           -> dict: merges [(a, b, size_a, size_b, num)], n_zero, n_tied, sum_h, panels, max_product
    window(H, n_sites, linkage, pops) -> the same with n_members / n_sites, as the records must hold them
    heights / newick / clade_sets / rf -> the derived values of impop_amd.tree, written again

The float prefilter: the candidates of a step are the pairs whose double value is within a relative 1e-9 of the smallest double
value (a double quotient of two integers below 2^53 is off by at most 2^-52 relative, so the true minimum and all its exact ties
are among them); among the candidates the distinct (S, D) are compared as Python integers, S1 D2 against S2 D1.  max_product is
the largest such product the search formed: tests/tree_cases.py asserts that the 128-bit case really needs more than 64 bits.
"""
import numpy as np

LINKAGES = ("single", "complete", "average")
NONE = 0xFFFFFFFF


def tree(H, linkage, pops=None):
    """H: symmetric integer distances over the member positions; pops: K lists of member POSITIONS (disjoint)"""
    assert linkage in LINKAGES
    H = np.asarray(H, np.int64)
    m = H.shape[0]
    average = linkage == "average"
    pops = [sorted(int(x) for x in p) for p in (pops or [])]
    K = len(pops)
    cnt = np.zeros((K, m), np.int64)
    for p, members in enumerate(pops):
        cnt[p, members] = 1
    panels = [dict(n_members=len(p), largest_clade=1, mrca_size=1 if len(p) == 1 else 0, mrca_merge=NONE) for p in pops]

    names = np.arange(m)
    size = np.ones(m, np.int64)
    alive = np.ones(m, bool)
    S = H.copy()
    V = S.astype(np.float64)
    np.fill_diagonal(V, np.inf)
    merges, n_zero, n_tied, max_product = [], 0, 0, 0
    for step in range(m - 1):
        n = len(names)
        vmin = V.min()
        if not average:  # integers below 2^53: the doubles are exact
            i, j = divmod(int(V.argmin()), n)  # row-major first occurrence: the smallest a, then the smallest b
            tied = int((V == vmin).sum()) // 2
        else:
            ii, jj = np.nonzero(V <= vmin * (1.0 + 1e-9))
            if len(ii) == 2 or vmin == 0.0:  # one pair; or sums that are exactly 0, all equal whatever their denominators
                i, j, tied = int(ii[0]), int(jj[0]), len(ii) // 2
            else:
                sd = np.stack([S[ii, jj], size[ii] * size[jj]], axis=1)
                uniq, inverse = np.unique(sd, axis=0, return_inverse=True)
                inverse = np.asarray(inverse).reshape(-1)
                bs, bd = int(uniq[0][0]), int(uniq[0][1])
                for s, d in uniq[1:]:
                    l, r = int(s) * bd, bs * int(d)
                    max_product = max(max_product, l, r)
                    if l < r:
                        bs, bd = int(s), int(d)
                exact = np.array([int(s) * bd == bs * int(d) for s, d in uniq], bool)[inverse]
                first = int(np.flatnonzero(exact)[0])
                i, j, tied = int(ii[first]), int(jj[first]), int(exact.sum()) // 2
        assert i < j and alive[i] and alive[j]
        a, b, sa, sb, num = int(names[i]), int(names[j]), int(size[i]), int(size[j]), int(S[i, j])
        merges.append((a, b, sa, sb, num))
        n_zero += num == 0
        n_tied += tied >= 2
        row = np.minimum(S[i], S[j]) if linkage == "single" else np.maximum(S[i], S[j]) if linkage == "complete" else S[i] + S[j]
        S[i, :] = row
        S[:, i] = row
        size[i] = sa + sb
        vrow = row / (size[i] * size).astype(np.float64) if average else row.astype(np.float64)
        vrow[~alive] = np.inf
        vrow[i] = np.inf
        vrow[j] = np.inf
        V[i, :] = vrow
        V[:, i] = vrow
        V[j, :] = np.inf
        V[:, j] = np.inf
        alive[j] = False
        for p in range(K):
            cnt[p, a] += cnt[p, b]
            inside = int(cnt[p, a])
            if inside == sa + sb:
                panels[p]["largest_clade"] = max(panels[p]["largest_clade"], sa + sb)
            if panels[p]["mrca_size"] == 0 and inside == panels[p]["n_members"]:
                panels[p]["mrca_size"], panels[p]["mrca_merge"] = sa + sb, step
        if alive.sum() * 4 < n * 3:  # drop the dead rows and columns: the order of the names is kept
            keep = np.flatnonzero(alive)
            names, size, S, V = names[keep], size[keep], S[np.ix_(keep, keep)], V[np.ix_(keep, keep)]
            alive = np.ones(len(keep), bool)
    return dict(merges=merges, n_zero=int(n_zero), n_tied=int(n_tied), sum_h=int(np.triu(H, 1).sum()), panels=panels,
                max_product=max_product)


def window(H, n_sites, linkage, pops=None):
    t = tree(H, linkage, pops)
    t.update(n_members=int(np.asarray(H).shape[0]), n_sites=int(n_sites))
    return t


def merges_array(t):
    """the merges as the structured array BitMatrix.tree_scan returns per window"""
    out = np.zeros(len(t["merges"]), np.dtype([("a", "<u4"), ("b", "<u4"), ("size_a", "<u4"), ("size_b", "<u4"), ("num", "<u8")]))
    for i, g in enumerate(t["merges"]):
        out[i] = g
    return out


def heights(merges, linkage):
    return [num / (sa * sb) / 2 if linkage == "average" else num / 2 for _, _, sa, sb, num in merges]


def clade_sets(merges):
    """the set of non-trivial clades: at least two members, not all"""
    m = len(merges) + 1
    held = [{i} for i in range(m)]
    out = set()
    for a, b, _, _, _ in merges:
        held[a] = held[a] | held[b]
        held[b] = None
        if len(held[a]) < m:
            out.add(frozenset(held[a]))
    return out


def rf(merges_x, merges_y):
    x, y = clade_sets(merges_x), clade_sets(merges_y)
    return len(x - y) + len(y - x)


def newick(merges, names, linkage):
    """children a then b, branch = parent height - child height, repr of the double; labels with Newick punctuation quoted"""
    h = heights(merges, linkage)
    made = {}  # cluster name -> index of the merge that made its current node

    def text(node):  # node: ("leaf", position) or ("merge", index)
        if node[0] == "leaf":
            label = str(names[node[1]])
            if set(label) & set("()[]':;, \t\n"):
                label = "'%s'" % label.replace("'", "''")
            return label, 0.0
        a_node, b_node = kids[node[1]]
        (ta, ha), (tb, hb) = text(a_node), text(b_node)
        top = h[node[1]]
        return "(%s:%r,%s:%r)" % (ta, top - ha, tb, top - hb), top

    kids = []
    for i, (a, b, _, _, _) in enumerate(merges):
        kids.append((("merge", made[a]) if a in made else ("leaf", a), ("merge", made[b]) if b in made else ("leaf", b)))
        made[a] = i
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * len(merges) + 100))
    return text(("merge", len(merges) - 1))[0] + ";"
