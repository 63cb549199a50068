#!/usr/bin/env python3
"""Writes tests/golden/genome_stats.tsv: the assembly statistics of the 27
golden genomes (tests/golden/data/*/*.fna.gz) as galah's
calculate_genome_stats gives them (reference src/genome_stats.rs:11-51).

A plain-Python restatement of that function, independent of the library:
FASTA records split at the lines that start with '>', a contig's length its
sequence bytes other than '\\n' and '\\r', the ambiguous bases the N / n among
them, and the reference's own n50 loop (lengths ascending, the first at which
the running sum reaches total // 2).  The reference pins two of the rows in
its tests (src/genome_stats.rs:61-87): abisko4/73.20110600_S2D.10 = 161 /
6506 / 8289 and set1/1mbp = 1 / 0 / 1000000; this script checks them before
it writes anything.

    python tests/golden/make_genome_stats.py
"""
import gzip
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def genome_stats(text):
    lens, amb = [], 0
    for rec in text.split(b"\n>"):  # (the file starts with '>': the first piece keeps it, harmlessly in its header)
        seq = rec.partition(b"\n")[2]
        lens.append(len(seq) - seq.count(b"\n") - seq.count(b"\r"))
        amb += seq.count(b"N") + seq.count(b"n")
    total, run, n50 = sum(lens), 0, None
    for length in sorted(lens):
        run += length
        if run >= total // 2:
            n50 = length
            break
    return len(lens), amb, n50, total


def main():
    with np.load(os.path.join(HERE, "sketches_k21_s1000.npz")) as z:
        names = [str(x) for x in z["names"]]
    rows = []
    for name in names:
        with gzip.open(os.path.join(HERE, "data", name + ".gz"), "rb") as f:
            text = f.read()
        assert text.startswith(b">"), name
        rows.append((name,) + genome_stats(text))
    by_name = {r[0]: r[1:] for r in rows}
    assert by_name["abisko4/73.20110600_S2D.10.fna"][:3] == (161, 6506, 8289)
    assert by_name["set1/1mbp.fna"][:3] == (1, 0, 1000000)
    with open(os.path.join(HERE, "genome_stats.tsv"), "w") as f:
        f.write("path\tnum_contigs\tnum_ambiguous_bases\tn50\ttotal_bases\n")
        for r in rows:
            f.write("%s\t%d\t%d\t%d\t%d\n" % r)
    print("wrote %d rows" % len(rows))


if __name__ == "__main__":
    main()
