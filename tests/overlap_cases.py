"""Inputs and call sequence of tests/test_gpu_irregular_overlap.py: the three windowed all-pairs calls (pairwise_scan,
pairwise_scan_panel, cluster_scan) on ONE irregular, unsorted, overlapping window list.  Seeded, so that the parent and every
child process build the same matrices and their records can be compared byte for byte.

    python tests/overlap_cases.py OUT.npz [each]

runs every call (behind a "@@call TAG" marker on stderr, for the parent to sort the IMPOP_TRACE=1 lines by) and saves every
array; with `each` also every call made one window at a time.  A child process is needed because IMPOP_PAIRWISE_CHUNK,
IMPOP_GRAM_U16, IMPOP_EPILOGUE_SMALL and IMPOP_TRACE are read once per process.

The module imports without a GPU (tests/test_host_logic.py takes WINDOWS from it); importing it checks the window list against
a small model of the planner's elementary-segment rule, so that an edit of the list cannot silently lose a case."""
import sys

import numpy as np

from panel_cases import founders, panels

# (site_begin, site_end, seq_len): not sorted; duplicates (100,164); nested windows; an empty one; one-site windows on a column
# that is all ones (410) and all zeros (150); (776,779) ends on two all-ones columns; (800,870) is a single cell behind the
# uncovered gap 779..800.  seq_len is the width except for (37,230) (0: pi_site undefined) and (200,417) (another length).
WINDOWS = [(599, 777, 178), (100, 164, 64), (0, 600, 600), (410, 411, 1), (300, 300, 0), (100, 164, 64),
           (800, 870, 70), (37, 230, 0), (150, 151, 1), (200, 417, 5000), (776, 779, 3), (99, 412, 313)]
SEG_COUNTS = [3, 3, 14, 1, 0, 3, 1, 7, 1, 5, 2, 9]  # Gram matrices summed per window, as the host driver of pair_plan.h reports them
N_CELLS = 18
N_SITE = 900
SHAPES = (40, 130, 300, 513)  # one 64-bit word of members | nw <= 4 (NWK = 4) | nw > 4 (NWK = 8) | the general kernels by size
PANEL_SIZES = {130: [50, 30, 44], 300: [110, 77, 100]}  # class boundaries inside 64-wide words, 6 / 13 haplotypes in no panel
PANEL_PAIRS = ((0, 1), (0, 2), (1, 2))  # the pair order of the panel call
WEIGHTED_N = 130

# pairwise_scan: `match` rounded, `dice` unrounded, and hud.py's grouped Fst (keys as test_gpu_batch_regimes._check reads them)
PS_CALLS = {"match": {"kind": "match", "thr": 0.98, "rd": 4, "fm": "direct"},
            "dice": {"kind": "dice", "thr": 0.97, "rd": None, "fm": "direct"},
            "grouped": {"kind": "match", "thr": 0.98, "rd": 4, "fm": "grouped"}}
CL_CALLS = {"match": {"kind": "match", "thr": 0.98, "rd": 4}, "dice": {"kind": "dice", "thr": 0.97, "rd": None}}
PANEL_CALL = {"kind": "match", "thr": 0.98, "rd": 4, "fm": "direct"}


def segment_model(wins):
    """The elementary-segment rule of csrc/pair_plan.h, restated: the cuts are the boundaries of the non-empty windows, a cell is
    an interval between neighbouring cuts that some window covers, a window sums the cells inside it, and the cells are shared
    when they hold under 95 % of the windows' sites.  -> (segmented, cells, cells per window, the order the chunks take the
    windows in: by first cell, windows without cells last, ties in the caller's order)"""
    live = [(a, b) for a, b, *_ in wins if b > a]
    cuts = sorted({x for w in live for x in w})
    cells = [(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:]) if any(a <= lo and hi <= b for a, b in live)]
    first = [next((k for k, c in enumerate(cells) if c[0] == a), 0) if b > a else 0 for a, b, *_ in wins]
    count = [sum(1 for lo, hi in cells if a <= lo and hi <= b) if b > a else 0 for a, b, *_ in wins]
    shared = 20 * sum(hi - lo for lo, hi in cells) < 19 * sum(b - a for a, b in live)
    order = sorted(range(len(wins)), key=lambda i: (count[i] == 0, first[i] if count[i] else 0, i))
    return shared, len(cells), count, order


def _check_window_list():
    shared, cells, count, order = segment_model(WINDOWS)
    assert shared and cells == N_CELLS and count == SEG_COUNTS, (shared, cells, count)
    have = set(count)
    assert {0, 1, 2} <= have and any(c % 2 and c >= 5 for c in have) and any(c % 2 == 0 and c >= 6 for c in have), have
    assert order != list(range(len(WINDOWS))) and order[-1] == 4  # a real permutation; the empty window goes last
    assert [w[:2] for w in WINDOWS].count((100, 164)) == 2
    assert sum(1 for a, b, L in WINDOWS if L == 0 and b > a) == 1 and sum(1 for a, b, L in WINDOWS if L not in (0, b - a)) == 1
    a, b, _ = WINDOWS[6]  # the disjoint window: one cell, nothing else touches it, an uncovered gap in front of it
    assert count[6] == 1 and max(e for _, e, _ in WINDOWS[:6] + WINDOWS[7:]) < a


_check_window_list()


def matrix(n):
    """founder haplotypes with noise; column 150 all zero, 410 / 777 / 778 all one; inside 800..870 ten all-zero and ten all-one
    columns between columns that really vary"""
    rng = np.random.default_rng(9000 + n)
    m = founders(rng, n, N_SITE, pf=0.02, pp=0.004)
    m[:, 150] = 0
    m[:, [410, 777, 778]] = 1
    k = np.arange(800, 870)
    zero, one, rest = k[k % 7 == 1], k[k % 7 == 4], k[(k % 7 != 1) & (k % 7 != 4)]
    m[:, rest] ^= (rng.random((n, rest.size)) < 0.1).astype(np.uint8)
    m[:, zero] = 0
    m[:, one] = 1
    c = m[:, rest].sum(0)
    assert zero.size >= 10 and one.size >= 10 and int(((c > 0) & (c < n)).sum()) >= 10
    return m


def masks(n):
    """a subset P and disjoint A / B"""
    rng = np.random.default_rng(9100 + n)
    inP = (rng.random(n) < 0.8).astype(np.uint8)
    inA = (rng.random(n) < 0.35).astype(np.uint8)
    inB = ((rng.random(n) < 0.45) & (inA == 0)).astype(np.uint8)
    assert 2 < inP.sum() < n and inA.sum() >= 2 and inB.sum() >= 2
    return inP, inA, inB


def panel_flags(n):
    return panels(np.random.default_rng(9200 + n), n, PANEL_SIZES[n])


def weighted_inputs():
    """-> (node matrix, node lengths 1..39, the list in node coordinates, the same list in bp coordinates): a window's seq_len is
    its length in bp, with the list's two exceptions kept"""
    node = matrix(WEIGHTED_N)
    wt = np.random.default_rng(9300).integers(1, 40, size=N_SITE).astype(np.uint32)
    pre = np.concatenate([[0], np.cumsum(wt)]).astype(np.int64)
    node_wins = [(a, b, L if L in (0, 5000) else int(pre[b] - pre[a])) for a, b, L in WINDOWS]
    bp_wins = [(int(pre[a]), int(pre[b]), L) for a, b, L in node_wins]
    return node, wt, node_wins, bp_wins


def matrices():
    """tag -> (n, the windows of that matrix, s_scope of its calls); the order run() uploads them in.  The weighted matrix counts
    nodes where its bp-expanded form counts base pairs: compared without S (s_scope 2)."""
    out = {}
    for n in SHAPES:
        for form in ("plain", "compact"):
            out[f"n{n}.{form}"] = (n, WINDOWS, 1)
    _, _, node_wins, bp_wins = weighted_inputs()
    for form, wins in (("node", node_wins), ("node_compact", node_wins), ("bp", bp_wins)):
        out[f"w{WEIGHTED_N}.{form}"] = (WEIGHTED_N, wins, 2)
    return out


def call_names(n):
    names = ["ps_" + k for k in PS_CALLS] + ["cl_" + k for k in CL_CALLS]
    if n in PANEL_SIZES:
        names += ["panel"] + [f"pp{j}" for j in range(len(PANEL_PAIRS))]
    return names


def _concat(results):
    if isinstance(results[0], tuple):
        return tuple(np.concatenate(x) for x in zip(*results))
    return np.concatenate(results)


def _calls(call, tag, mat, n, wins, s_scope, each):
    inP, inA, inB = masks(n)

    def both(name, fn):
        call(f"{tag}.{name}", lambda: fn(wins))
        if each:
            call(f"{tag}.{name}.each", lambda: _concat([fn([w]) for w in wins]))

    for name, c in PS_CALLS.items():
        both("ps_" + name, lambda ww, c=c: mat.pairwise_scan(ww, inP, inA, inB, kind=c["kind"], threshold=c["thr"], round_digits=c["rd"],
                                                             fst_method=c["fm"], s_scope=s_scope))
    for name, c in CL_CALLS.items():
        both("cl_" + name, lambda ww, c=c: mat.cluster_scan(ww, mask_p=inP, kind=c["kind"], threshold=c["thr"], round_digits=c["rd"]))
    if n in PANEL_SIZES:
        pops, c = panel_flags(n), PANEL_CALL
        kw = dict(kind=c["kind"], threshold=c["thr"], round_digits=c["rd"], s_scope=s_scope)
        both("panel", lambda ww: mat.pairwise_scan_panel(ww, pops, **kw))
        # what the panel call must agree with: pairwise_scan with panel j as its subset and pair j as its A / B
        for j, (k, l) in enumerate(PANEL_PAIRS):
            call(f"{tag}.pp{j}", lambda j=j, k=k, l=l: mat.pairwise_scan(wins, pops[j], pops[k], pops[l], **kw))


def run(ctx, call, each=False):
    """every call of every matrix: call(tag, fn) runs fn and keeps what it returns under tag"""
    todo = matrices()
    for n in SHAPES:
        bm = ctx.upload_dense(matrix(n), keep_hap_major=True)
        bc = bm.compact()
        for form, mat in (("plain", bm), ("compact", bc)):
            _calls(call, f"n{n}.{form}", mat, *todo[f"n{n}.{form}"], each)
        bc.free()
        bm.free()
    node, wt, _, _ = weighted_inputs()
    bw = ctx.upload_dense(node, keep_hap_major=True)
    bw.set_site_weights(wt)
    bwc = bw.compact()
    be = ctx.upload_dense(np.repeat(node, wt, axis=1), keep_hap_major=True)
    for form, mat in (("node", bw), ("node_compact", bwc), ("bp", be)):
        _calls(call, f"w{WEIGHTED_N}.{form}", mat, *todo[f"w{WEIGHTED_N}.{form}"], each)
    bwc.free()
    bw.free()
    be.free()


def parts(got, tag):
    """the arrays a call returned: one (pairwise_scan) or three (panel: panels, pairs, windows; cluster: records, cluster_of, sizes)"""
    return (got[tag],) if tag in got else tuple(got[f"{tag}#{i}"] for i in range(3))


if __name__ == "__main__":
    import impop_amd
    c = impop_amd.Context(0)
    saved = {}

    def _call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        r = fn()
        if isinstance(r, tuple):
            saved.update({f"{tag}#{i}": x for i, x in enumerate(r)})
        else:
            saved[tag] = r

    run(c, _call, each=len(sys.argv) > 2 and sys.argv[2] == "each")
    np.savez(sys.argv[1], **saved)
    c.close()
