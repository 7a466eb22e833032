"""Held-out SNPs for MarginAlignSnpCaller: mutated copies of a reference and the truth files that go with them
(nanopore/analyses/mutate_reference.py:11-37).

For every reference FASTA and every rate in SNP_RATES, `mutateReferenceSequences` writes

    <stem>_<100 * rate>_percent_SNPs_0.0_percent_InDels.fasta              the reference with that fraction of its bases substituted
    <stem>_<100 * rate>_percent_SNPs_0.0_percent_InDels.fasta_Index.txt    every sequence as it was, then as `<name>_mutated`

(<stem> = the file name up to its `.fa` / `.fasta`; 100 * rate prints as 1.0, 5.0, 10.0, 20.0) -- the pair
`marginAlignSnpCaller.loadHeldOutSnps` reads.  Reads from the true genome are then aligned to the mutated copy and the caller is asked
for the bases that were held out.  Sequences are upper-cased (soft-masking is not kept), sequence names are cut at the first blank.  No
indels are made: the reference's indel rate is 0 times the SNP rate.

Differences from the reference: the random numbers come from a `random.Random` the caller may seed, and the substitute of a base is drawn
from the other bases in the order A C G T, not in the order of a set, so a seed gives the same files on every run.
"""
import os
import random

from ..bioio import fastaRead, fastaWrite

SNP_RATES = (0.01, 0.05, 0.10, 0.20)
INDEL_RATE = 0.0  # per SNP rate; part of the file names only


def mutateSequence(sequence, snpRate, rng=random):
    """The sequence in upper case, every base replaced with probability snpRate by one of the other bases of ACGT (a base outside ACGT:
    by any of the four)."""
    out = []
    for base in sequence.upper():
        if rng.random() < snpRate:
            base = rng.choice([b for b in "ACGT" if b != base])
        out.append(base)
    return "".join(out)


def mutatedFileNames(referenceFastaFile, snpRate):
    """(mutated reference, its truth file) for one rate."""
    directory, name = os.path.split(referenceFastaFile)
    stem = os.path.join(directory, name.split(".fa")[0])
    mutated = "%s_%s_percent_SNPs_%s_percent_InDels.fasta" % (stem, snpRate * 100, INDEL_RATE * snpRate * 100)
    return mutated, mutated + "_Index.txt"


def mutateReferenceSequences(referenceFastaFiles, rng=None):
    """-> the given files followed by their mutated copies, one per rate.  A file whose name contains `percent` is a mutated copy already
    and is not mutated again; a copy that exists is kept as it is (with whatever truth file it has)."""
    rng = random.Random() if rng is None else rng
    updated = list(referenceFastaFiles)
    for referenceFastaFile in referenceFastaFiles:
        if "percent" in os.path.basename(referenceFastaFile):
            continue
        for snpRate in SNP_RATES:
            mutatedFile, indexFile = mutatedFileNames(referenceFastaFile, snpRate)
            updated.append(mutatedFile)
            if os.path.exists(mutatedFile):
                continue
            with open(mutatedFile, "w") as fasta, open(indexFile, "w") as index:
                for header, sequence in fastaRead(referenceFastaFile):
                    name = header.split()[0]
                    mutated = mutateSequence(sequence, snpRate, rng)
                    fastaWrite(fasta, name, mutated)
                    fastaWrite(index, name, sequence.upper())
                    fastaWrite(index, name + "_mutated", mutated)
    return updated
