"""makeFastqSequenceNamesUnique / makeFastaSequenceNamesUnique: the processed copies of the input files the pipeline maps and
analyses (interface of nanopore/analyses/utils.py:247-274; called at nanopore/pipeline.py:185 and :191).

The rule, for both formats: a record's name is its header cut at the first blank; the first record of a name keeps it; a later
record whose name is taken gets `<name>_1`, `<name>_2`, ... -- the smallest number that gives a name no earlier record has.  (The
reference appends the letter "i" until the name is free, and cuts only FASTQ headers; a numeric suffix says which copy a read is,
and FastaTable cuts FASTA headers at the first blank anyway.)  Nothing else changes: the files are copied line by line as bytes,
so sequence and quality lines, their letter case, their line breaks and the line lengths of a multi-line FASTA stay as they are.
FASTQ records are the four-line records ingest.FastqTable and bioio.fastqRead read.
"""


def _uniqueName(header, taken):
    """The name a header line (without its '>' or '@', without the line break) gets: cut at the first blank, numbered when taken."""
    fields = header.split(None, 1)
    name = fields[0] if fields else b""
    if name in taken:
        k = 1
        while name + b"_%d" % k in taken:
            k += 1
        name = name + b"_%d" % k
    taken.add(name)
    return name


def makeFastqSequenceNamesUnique(inputFastqFile, outputFastqFile):
    """Writes outputFastqFile: inputFastqFile with unique names.  Returns outputFastqFile."""
    taken = set()
    with open(inputFastqFile, "rb") as fin, open(outputFastqFile, "wb") as fout:
        k = 0  # line of the record: 0 header, 1 sequence, 2 '+', 3 quality
        for line in fin:
            if k == 0:
                if not line.strip():
                    fout.write(line)  # blank lines between records, as fastqRead skips them
                    continue
                if not line.startswith(b"@"):
                    raise RuntimeError("Malformed FASTQ record header in %s: %r" % (inputFastqFile, line[:80]))
                fout.write(b"@" + _uniqueName(line[1:].rstrip(b"\r\n"), taken) + b"\n")
            else:
                fout.write(line)
            k = (k + 1) % 4
    return outputFastqFile


def makeFastaSequenceNamesUnique(inputFastaFile, outputFastaFile):
    """Writes outputFastaFile: inputFastaFile with unique names.  Returns outputFastaFile."""
    taken = set()
    with open(inputFastaFile, "rb") as fin, open(outputFastaFile, "wb") as fout:
        for line in fin:
            if line.startswith(b">"):
                fout.write(b">" + _uniqueName(line[1:].rstrip(b"\r\n"), taken) + b"\n")
            else:
                fout.write(line)
    return outputFastaFile
