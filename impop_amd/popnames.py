"""Population list -> sequence names (the matching rules of h-fst.py:18-82, 121-128): an assembly
name such as `HG00097_hap1_hprc_r2_v1.0.1` selects the PanSN sequences starting with `HG00097#1#`.
String handling only."""
from __future__ import annotations

import sys

# assembly-name endings and the haplotype digit they stand for, tried in this order
_HAPLOTYPE_OF_ENDING = (("_hap1", "1"), ("_hap2", "2"), ("_mat", "1"), ("_pat", "2"))


def canonicalize_identifier(identifier: str) -> str:
    """The `startswith` prefix an identifier selects; "" for blank lines and `#` comments."""
    name = (identifier or "").strip()
    if name == "" or name[0] == "#":
        return ""
    name = name.partition("_hprc")[0]  # release metadata behind the assembly name
    for ending, digit in _HAPLOTYPE_OF_ENDING:
        if name.endswith(ending):
            return name[: len(name) - len(ending)] + "#" + digit + "#"
    # a name that already ends a PanSN field is kept; anything else (a bare sample: both haplotypes) gets one
    return name if name.endswith("#") else name + "#"


def expand_population(raw_ids, all_sequences):
    """-> (set of sequence names selected by any identifier, identifiers that selected nothing)"""
    pool = tuple(all_sequences)
    selected, unmatched = set(), []
    for rid in raw_ids:
        key = canonicalize_identifier(rid)
        if not key:
            continue
        hits = [seq for seq in pool if seq.startswith(key)]
        if hits:
            selected.update(hits)
        else:
            unmatched.append(rid)
    return selected, unmatched


def read_subset_file(filename):
    """Non-blank lines that do not start with `#`, stripped; a missing file ends the process like the
    reference's reader does (message on stderr, exit code 1)."""
    try:
        handle = open(filename)
    except FileNotFoundError:
        print(f"Error: Subset file not found: {filename}", file=sys.stderr)
        sys.exit(1)
    with handle:
        return {ln.strip() for ln in handle if ln.strip() and ln[0] != "#"}


def pair_haplotypes(names, subset=None):
    """The diploid individuals among PanSN sequence names: `sample#1#...` and `sample#2#...` are the two copies of one person.
    names: the sequences in matrix order (anything behind the first ':' is cut first, as af.py cuts it); subset: the names that take
    part (default: all).  -> (pairs, sample_names, unpaired): pairs[i] = (index of sample i's haplotype 1, index of its haplotype 2),
    samples in order of first appearance; unpaired = the taking-part names of samples that are not exactly one `#1#` and one `#2#`
    sequence (a haploid assembly such as CHM13#0#chr1, half a person, a sample with more than two haplotypes, a name without a
    haplotype field), in matrix order."""
    chosen = None if subset is None else set(subset)
    by_sample = {}
    for idx, name in enumerate(names):
        if chosen is not None and name not in chosen:
            continue
        fields = name.partition(":")[0].split("#")
        sample = fields[0] if len(fields) >= 2 else name
        by_sample.setdefault(sample, []).append((idx, fields[1] if len(fields) >= 2 else None))
    pairs, sample_names, unpaired = [], [], []
    for sample, members in by_sample.items():
        if sorted(str(h) for _, h in members) == ["1", "2"]:
            first, second = sorted(members, key=lambda m: m[1])
            pairs.append((first[0], second[0]))
            sample_names.append(sample)
        else:
            unpaired.extend(idx for idx, _ in members)
    return pairs, sample_names, [names[i] for i in sorted(unpaired)]
