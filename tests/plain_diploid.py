"""A plain restatement of impop_diploid_scan's definitions (include/impop_hip.h) from a hap-major 0/1 array: Python integers and
floats, one site at a time.  It uses no code of the library, so that the device's integers and the host's doubles can be compared
with it bit for bit."""
import numpy as np

STATS_DTYPE = np.dtype([("n_ind", "<u4"), ("n_sites", "<u4"), ("s_p", "<u4"), ("het_sites", "<u4"), ("het_total", "<u8"), ("sum_p", "<u8"),
                        ("roh_sites_total", "<u8"), ("roh_runs_total", "<u4"), ("longest_run", "<u4"), ("ho", "<f8"), ("he", "<f8"),
                        ("f_is", "<f8"), ("f_roh", "<f8")])
IND_DTYPE = np.dtype([("het", "<u4"), ("hom_alt", "<u4"), ("longest_run", "<u4"), ("roh_runs", "<u4"), ("roh_sites", "<u4"),
                      ("reserved", "<u4")])
NAN = float("nan")


def runs_of(het_positions, b, e):
    """the runs of window [b, e) of an individual heterozygous at het_positions (ascending, inside the window): p_1 - b, the gaps
    p_{j+1} - p_j - 1, e - 1 - p_k; none heterozygous: one run of e - b.  Runs of length 0 are not runs."""
    if len(het_positions) == 0:
        runs = [e - b]
    else:
        runs = [het_positions[0] - b]
        runs += [q - p - 1 for p, q in zip(het_positions, het_positions[1:])]
        runs.append(e - 1 - het_positions[-1])
    return [int(r) for r in runs if r > 0]


def individual_row(row1, row2, b, e, min_run):
    """(het, hom_alt, longest_run, roh_runs, roh_sites) of one individual: row1 / row2 = its two copies, all sites"""
    het_positions = [b + int(s) for s in np.nonzero(row1[b:e] != row2[b:e])[0]]
    hom_alt = int(np.count_nonzero(row1[b:e] & row2[b:e]))
    runs = runs_of(het_positions, b, e)
    roh = [r for r in runs if r >= min_run]
    return len(het_positions), hom_alt, max(runs, default=0), len(roh), sum(roh)


def doubles(N, W, seq_len, het_total, sum_p, roh_sites_total):
    """ho, he, f_is, f_roh in the header's operation order"""
    L = seq_len if seq_len > 0 else W
    n = 2 * N
    ho = float(het_total) / (float(N) * float(L)) if L else NAN
    he = 2.0 * float(sum_p) / (float(n) * float(n - 1) * float(L)) if L else NAN
    f_is = 1.0 - float(het_total * (n - 1)) / float(sum_p) if sum_p else NAN
    f_roh = float(roh_sites_total) / (float(N) * float(W)) if W else NAN
    return ho, he, f_is, f_roh


def reference(m01, pairs, windows, min_run):
    """-> (records [n_windows], rows [n_windows, N]) for windows = (site_begin, site_end[, seq_len]) rows"""
    m = np.asarray(m01).astype(np.uint8)
    pairs = [(int(a), int(b)) for a, b in pairs]
    N = len(pairs)
    members = [h for p in pairs for h in p]
    rec = np.zeros(len(windows), dtype=STATS_DTYPE)
    ind = np.zeros((len(windows), N), dtype=IND_DTYPE)
    for k, w in enumerate(windows):
        b, e = int(w[0]), int(w[1])
        seq_len = int(w[2]) if len(w) > 2 else 0
        W = e - b
        c = m[members, b:e].sum(axis=0).astype(np.int64) if W else np.zeros(0, np.int64)
        any_het = np.zeros(W, dtype=bool)
        for i, (h1, h2) in enumerate(pairs):
            het, hom_alt, longest, runs, sites = individual_row(m[h1], m[h2], b, e, min_run)
            ind[k, i] = (het, hom_alt, longest, runs, sites, 0)
            any_het |= m[h1, b:e] != m[h2, b:e]
        het_total = int(ind["het"][k].astype(np.uint64).sum())
        sum_p = int((c * (2 * N - c)).sum())
        roh_sites_total = int(ind["roh_sites"][k].astype(np.uint64).sum())
        rec[k] = (N, W, int(((c > 0) & (c < 2 * N)).sum()), int(any_het.sum()), het_total, sum_p, roh_sites_total,
                  int(ind["roh_runs"][k].sum()), int(ind["longest_run"][k].max()) if N else 0) + doubles(N, W, seq_len, het_total, sum_p,
                                                                                                        roh_sites_total)
    return rec, ind


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def assert_matches(got, want, tag=""):
    """every integer equal, every double equal bit for bit (== except NaN against NaN), rows byte for byte"""
    (rec, ind), (wrec, wind) = got, want
    assert len(rec) == len(wrec), tag
    for name in STATS_DTYPE.names:
        a, b = np.asarray(rec[name]), np.asarray(wrec[name])
        if STATS_DTYPE[name].kind == "f":
            both_nan = np.isnan(a) & np.isnan(b)
            assert ((a == b) | both_nan).all(), (tag, name, a[~((a == b) | both_nan)][:4], b[~((a == b) | both_nan)][:4])
        else:
            assert np.array_equal(a, b), (tag, name, a[a != b][:6], b[a != b][:6], np.nonzero(a != b)[0][:6])
    if ind is not None:
        assert ind.shape == wind.shape, (tag, ind.shape, wind.shape)
        for name in IND_DTYPE.names:
            bad = np.argwhere(ind[name] != wind[name])
            assert len(bad) == 0, (tag, name, bad[:5].tolist(), ind[name][tuple(bad[0])], wind[name][tuple(bad[0])])
