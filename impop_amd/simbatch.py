"""Batches of `.sim` identity tables: the list reader, the threaded native ingest, per-table population flags and the
chunked pipeline in front of Context.stats_from_identity_batch — what `scripts/impop_scan.py --sim-list` is made of.
One table per window is the reference's real data flow (run_pica2_impg.sh:162-175, run_h-fst.sh:65-81,
run_tajd.sh:160-180 start one python3 process per window); here the tables of a chunk share two kernel launches, and
chunk c + 1 is parsed on the host threads while chunk c is on the GPU.  Marshalling only: no statistics here."""
from __future__ import annotations

import ctypes as C
import io
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import List, NamedTuple, Optional

import numpy as np

from . import _lib, simfile
from .drivers import bed_row_ok
from .pica2 import seed_rank_of
from .popnames import expand_population

MAX_BATCH_N = 1023  # impop_stats_from_identity_batch; larger tables go through the single-problem entry points


class SimRow(NamedTuple):
    chrom: str
    start: int
    end: int
    sim_path: str
    S: Optional[str]  # segregating sites, as typed (tajd); None when the column is absent


class SimTable(NamedTuple):
    names: list          # sorted
    dense: np.ndarray    # [n, n], NaN = pair absent
    n_rows: int
    elements: set        # the reference reader's name set, rebuilt in first-seen order (pica2.py:45-46)


class SimFailure(NamedTuple):
    message: str         # what the per-window script would have printed before exiting 1


def read_sim_list(path, fmt="tajd") -> List[SimRow]:
    """TSV rows `chrom  start  end  sim_path  [S]`.  `#` and empty lines are skipped; a relative sim_path resolves against
    the list file's directory; the BED columns are validated (and warned about) like read_bed(fmt) of the batch driver."""
    base = os.path.dirname(os.path.abspath(path))
    rows = []
    with open(path) as f:
        for line_no, line in enumerate(f, 1):
            p = line.rstrip("\n").split("\t")
            if not p or not p[0] or p[0].startswith("#"):
                continue
            chrom = p[0]
            start, end = (p[1] if len(p) > 1 else ""), (p[2] if len(p) > 2 else "")
            if not bed_row_ok(chrom, start, end, line_no, fmt):
                continue
            sim = p[3].strip() if len(p) > 3 else ""
            if not sim:
                raise ValueError(f"{path}: line {line_no}: no sim_path column")
            s_col = p[4].strip() if len(p) > 4 and p[4].strip() else None
            rows.append(SimRow(chrom, int(start), int(end), sim if os.path.isabs(sim) else os.path.join(base, sim), s_col))
    return rows


def _python_reader(path, flavor):
    """The reference-faithful reader for what the native parser declines or found a bad value in.  Its messages are
    collected, not printed by the reader (it may run beside the main thread): where the per-window script would have
    exited they are the window's failure text, else (h-fst's skipped values) they go to stderr as they would have."""
    buf = io.StringIO()
    try:
        names, dense, n_rows, elements = simfile.python_read_dense(path, flavor, stream=buf)
    except SystemExit:
        return SimFailure(buf.getvalue().rstrip("\n"))
    except OSError as e:  # h-fst.py lets these escape as a traceback; the window fails either way
        return SimFailure(f"Error reading file {path}: {e}")
    if buf.getvalue():
        sys.stderr.write(buf.getvalue())
    return SimTable(names, dense, n_rows, elements)


def ingest(paths, flavor="pica2", n_threads=0):
    """paths -> [SimTable | SimFailure], parsed by impop_sim_parse_many on at most n_threads host threads (0 =
    OMP_NUM_THREADS, else 16).  A table the native parser declines goes through the Python reader, as in the CLIs."""
    lib = _lib.load()
    k = len(paths)
    if not k:
        return []
    c_paths = (C.c_char_p * k)(*[os.fsencode(p) for p in paths])
    handles = (C.c_void_p * k)()
    rcs = (C.c_int32 * k)()
    _lib.check(lib.impop_sim_parse_many(c_paths, k, 0 if flavor == "pica2" else 1, int(n_threads), handles, rcs))
    out = []
    try:
        for i, path in enumerate(paths):
            if rcs[i] == _lib.E_NOMEM:
                raise _lib.ImpopError(_lib.E_NOMEM, f"out of memory while parsing {path}")
            got = simfile.table_from_handle(lib, C.c_void_p(handles[i]), with_elements=True) if rcs[i] == 0 else None
            out.append(SimTable(*got) if got is not None else _python_reader(path, flavor))
    finally:
        for i in range(k):
            if handles[i]:
                lib.impop_sim_free(C.c_void_p(handles[i]))
    return out


class PopulationFlags:
    """expand_population of one list file's identifiers against each table's own names; tables of one chromosome
    usually share their names, so the result is cached on the name tuple."""

    def __init__(self, raw_ids):
        self.raw = raw_ids
        self._cache = {}

    def __call__(self, names):
        key = tuple(names)
        hit = self._cache.get(key)
        if hit is None:
            members, missing = expand_population(self.raw, set(names))
            flags = np.fromiter((1 if n in members else 0 for n in names), dtype=np.uint8, count=len(names))
            hit = self._cache[key] = (flags, len(missing))
        return hit


def _chunks(rows, max_tables=64):
    """the list cut into runs of at most max_tables rows: the unit that is parsed while the previous one is on the GPU"""
    for i in range(0, len(rows), max_tables):
        yield i, rows[i:i + max_tables]


def run_pipeline(ctx, rows, flavor, make_problem, threshold, round_digits, fst_round_digits, n_threads=0, tables_per_chunk=64,
                 max_chunk_bytes=0, timings=None):
    """For every row: ("ok", record, table) | ("fail", message).  make_problem(row, table) -> problem dict for
    stats_from_identity_batch, or a SimFailure.  Chunk c + 1 is parsed (native threads, GIL released) while chunk c runs."""
    import time
    results = [None] * len(rows)
    parts = list(_chunks(rows, tables_per_chunk))
    if not parts:
        return results
    t_parse = t_gpu = 0.0
    with ThreadPoolExecutor(max_workers=1) as ex:
        def parse(part):
            t0 = time.perf_counter()
            r = ingest([row.sim_path for row in part], flavor, n_threads)
            return r, time.perf_counter() - t0
        fut = ex.submit(parse, parts[0][1])
        for c, (first, part) in enumerate(parts):
            tables, dt = fut.result()
            t_parse += dt
            if c + 1 < len(parts):
                fut = ex.submit(parse, parts[c + 1][1])
            problems, where = [], []
            for j, (row, tab) in enumerate(zip(part, tables)):
                if isinstance(tab, SimFailure):
                    results[first + j] = ("fail", tab.message)
                    continue
                pr = make_problem(row, tab)
                if isinstance(pr, SimFailure):
                    results[first + j] = ("fail", pr.message)
                    continue
                problems.append(pr)
                where.append((first + j, tab))
            t0 = time.perf_counter()
            recs, _ = ctx.stats_from_identity_batch(problems, threshold, round_digits, fst_round_digits, max_chunk_bytes,
                                                    with_groups=False)
            for (i, tab), rec, pr in zip(where, recs, problems):
                if int(rec["status"]) == _lib.E_UNSUPPORTED:  # 1024 names or more: the single-problem entry points
                    rec = rec.copy()
                    rec["fst"], rec["tajima_d"] = np.nan, np.nan  # "none", as in a batch record
                    pi, ps, _, G = ctx.pi_from_identity(pr["ident"], threshold, round_digits, pr.get("seq_len"), pr.get("seed_rank"))
                    rec["pi"], rec["pi_site"], rec["n_groups"], rec["status"] = pi, ps, G, 0
                    if pr.get("in_a") is not None:
                        rec["fst"], rec["fst_counts"] = ctx.fst_from_identity(pr["ident"], pr["in_a"], pr["in_b"], pr.get("seq_len"),
                                                                              fst_round_digits)
                    if pr.get("tajima_n") is not None and pr["tajima_n"] >= 2 and ps == ps:
                        rec["tajima_d"] = ctx.tajimas_d(pr["tajima_n"], pr["tajima_S"], float(f"{ps:.8f}"))[0]
                results[i] = ("ok", rec, tab)
            t_gpu += time.perf_counter() - t0
    if timings is not None:
        timings["parse_s"] = timings.get("parse_s", 0.0) + t_parse
        timings["gpu_call_s"] = timings.get("gpu_call_s", 0.0) + t_gpu
    return results


def seed_rank(table: SimTable):
    """the reference's set.pop() order of this table under this interpreter's PYTHONHASHSEED (pica2.seed_rank_of)"""
    return seed_rank_of(table.elements, table.names)


def tajimas_d_from_pi_site(n: int, S: float, pi_site: float) -> float:
    """The tajima_d of a batch record, on the host: tj_d.py's D for (n, S) and pi = pica2's "%.8f" text of pi per site
    (run_tajd.sh:174-180); NaN where tj_d.py would refuse the arguments."""
    D = C.c_double()
    _lib.check(_lib.load().impop_tajimas_d_from_pi_site(int(n), float(S), float(pi_site), C.byref(D)))
    return D.value
